"""solver.Book on the host: the object and its file, and ``solve_host(book=)`` / ``drive_host(book=)`` against the exhaustive
oracle's scores of tests/golden/solver_exact.npz.

The rows are the file's rows with 4..12 empty squares, all of them, one book a depth: the distinct descendants three
plies down (``_build_graph``), solved by ``solve_host``.  The file's rows with 1..3 empty squares are left out: three plies
down from them the board is full or the game over, so there is no position to put into a book.  A book never changes an answer -- every entry is a true bound --
so every windowed search with a book must obey the oracle exactly as the search without one does; it may only enter fewer
nodes.  Rows with fewer than six empty squares reach no interior node three plies down (with two empty squares left the
window closes in enter_node), so hits are demanded from six on."""
import numpy as np
import pytest

import solver_exact_cases as X
from conftest import load_npz

DEPTHS = list(range(4, 13))
PLIES = 3


def windowed(answers):
    """A ``Windowed`` of HostWindowAnswers."""
    from connect4_amd.solver import Windowed
    return Windowed(np.array([a.status for a in answers], dtype=np.int8), np.array([a.score for a in answers], dtype=np.int8),
                    np.array([a.bound for a in answers], dtype=np.int8), None, None, np.array([a.nodes for a in answers]), None)


@pytest.fixture(scope="module")
def gold():
    z = load_npz("solver_exact.npz")
    return {k: z[k] for k in ("c0", "c1", "score", "empties")}


@pytest.fixture(scope="module")
def books(gold):
    """Per depth e: the rows, their leaves three plies down, the exact book and the outcome book of those leaves, and the
    bookless search of every (row, window): computed once, read by every test."""
    from connect4_amd.solver import Book, _build_graph, _children_host, solve_host
    out = {}
    windows = X.windows(gold["score"])
    for e in DEPTHS:
        at = np.nonzero(gold["empties"] == e)[0]
        rows = np.stack([gold["c0"][at], gold["c1"][at]], axis=1)
        g = _build_graph(rows, None, None, PLIES, _children_host)
        first = int(g.level_start[-2])
        leaves = np.stack([g.color0[first:], g.color1[first:]], axis=1)
        pairs = [(int(a), int(b)) for a, b in leaves]
        exact = Book.from_answers(leaves, windowed([solve_host(p, window=(-42, 42)) for p in pairs]), age=42 - e + PLIES)
        outcome = Book.from_answers(leaves, windowed([solve_host(p, window=(-1, 1)) for p in pairs]), age=42 - e + PLIES)
        plain = {name: [solve_host((int(r[0]), int(r[1])), window=(int(a[i]), int(b[i]))) for r, i in zip(rows, at)] for name, a, b in windows}
        out[e] = {"at": at, "rows": rows, "leaves": leaves, "exact": exact, "outcome": outcome, "plain": plain}
    return out, windows


def search(rows, at, windows, book, gold, plain=None):
    """Every row from every window with `book`: the oracle's rule must hold; returns (nodes, hits) summed.  plain: the
    bookless answers, which no search with a book may exceed in nodes, row by row."""
    from connect4_amd import _lib as L
    from connect4_amd.solver import solve_host
    nodes = hits = 0
    for name, a, b in windows:
        got = []
        for k, (r, i) in enumerate(zip(rows, at)):
            ans = solve_host((int(r[0]), int(r[1])), window=(int(a[i]), int(b[i])), book=book)
            assert ans.status == L.SOLVE_SOLVED
            if plain is not None:
                assert ans.nodes <= plain[name][k].nodes, (name, int(i), ans, plain[name][k])
            hits += ans.hits
            nodes += ans.nodes
            got.append(ans)
        bad = X.window_violations([g.score for g in got], [g.bound for g in got], a[at], b[at], gold["score"][at].astype(np.int64))
        assert len(bad) == 0, "window %s: rows %s break the oracle's rule" % (name, at[bad][:5].tolist())
    return nodes, hits


# -- the object --------------------------------------------------------------------------------------------------------------
def test_entries_are_the_leaves_interior_positions(books):
    from connect4_amd.solver import _EXACT, _book_keys, _interior_rows, entry_fields
    for e, b in books[0].items():
        leaves = b["leaves"]
        leaves = leaves[~(X.four(leaves[:, 0]) | X.four(leaves[:, 1])) & (X.ages(leaves[:, 0], leaves[:, 1]) < 42)]      # unfinished
        keys = np.unique(_book_keys(leaves[_interior_rows(leaves)]))
        assert np.array_equal(b["exact"].keys, keys) and np.array_equal(b["outcome"].keys, keys)
        assert len(b["exact"].unknown) == 0
        f = entry_fields(b["exact"].words)
        assert (f.kind == _EXACT).all() and (f.age == 42 - e + PLIES).all()
        assert e < 6 or (entry_fields(b["outcome"].words).kind != _EXACT).any()        # the outcome book holds bounds


def test_round_trip_and_merge(books, tmp_path):
    from connect4_amd.solver import Book, _book_keys
    book = books[0][12]["exact"]
    half = Book(book.age, book.words[::2], books[0][12]["leaves"][:5])
    path = str(tmp_path / "book.npz")
    half.save(path)
    back = Book.load(path)
    assert back.age == half.age and np.array_equal(back.words, half.words) and np.array_equal(back.unknown, half.unknown)
    with np.load(path) as z:
        assert sorted(z.files) == ["age", "unknown", "words"]
    whole = back.merge(Book(book.age, book.words[1::2]))
    assert np.array_equal(whole.words, book.words)
    # an exact entry beats a bound of the same key, and rows that now have an entry leave the unknown ones
    merged = books[0][12]["outcome"].merge(book)
    assert np.array_equal(merged.words, book.words)
    assert len(whole.unknown) <= 5 and not np.isin(_book_keys(whole.unknown), whole.keys).any()
    with pytest.raises(ValueError):
        book.merge(books[0][11]["exact"])


def test_the_constructor_rejects_what_a_probe_could_not_trust(books):
    from connect4_amd.solver import Book, _mirror_key
    book = books[0][10]["exact"]
    w, age = book.words, book.age
    Book(age, w)
    Book(age, w[:0])
    with pytest.raises(ValueError, match="sorted"):
        Book(age, w[::-1])
    with pytest.raises(ValueError, match="sorted"):
        Book(age, np.concatenate([w[:1], w]))
    keys = w & np.uint64((1 << 49) - 1)
    lopsided = np.nonzero(_mirror_key(keys) != keys)[0]
    other = (w[lopsided] & ~np.uint64((1 << 49) - 1)) | _mirror_key(keys[lopsided])
    other = other[np.argsort(other & np.uint64((1 << 49) - 1))]
    with pytest.raises(ValueError, match="canonical"):
        Book(age, other)
    with pytest.raises(ValueError, match="stones"):
        Book(age - 1, w)
    with pytest.raises(ValueError, match="stones"):
        Book(age, np.array([5 | (64 << 49) | (3 << 56)], dtype=np.uint64))         # a key that is no position
    with pytest.raises(ValueError, match="kind"):
        Book(age, w & ~np.uint64(3 << 56))
    with pytest.raises(ValueError):
        Book(age, w | np.uint64(1 << 58))
    with pytest.raises(ValueError, match="score"):
        Book(age, (w & ~np.uint64(0x7f << 49)) | np.uint64((64 + 43) << 49))
    with pytest.raises(ValueError):
        Book(42, w[:0])


def test_mirror_key_is_the_mirror_images_key(books):
    from connect4_amd.board import BOTTOM
    from connect4_amd.solver import _mirror_bits, _mirror_key
    rows = books[0][12]["leaves"]
    occ = rows[:, 0] | rows[:, 1]
    for mine in (rows[:, 0], rows[:, 1]):
        key = mine + occ + np.uint64(BOTTOM)
        assert np.array_equal(_mirror_key(key), _mirror_bits(mine) + _mirror_bits(occ) + np.uint64(BOTTOM))
        assert [_mirror_key(int(k)) for k in key[:50]] == _mirror_key(key[:50]).tolist()


# -- the search ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("e", DEPTHS)
def test_a_book_changes_no_answer_and_saves_nodes(gold, books, e):
    by_depth, windows = books
    b = by_depth[e]
    plain_nodes = sum(a.nodes for name in b["plain"] for a in b["plain"][name])
    nodes, hits = search(b["rows"], b["at"], windows, b["exact"], gold, b["plain"])
    print("%d empty squares, %d rows, %d entries: %d nodes with the book, %d without, %d hits" % (e, len(b["rows"]), len(b["exact"]), nodes,
                                                                                                plain_nodes, hits))
    assert nodes <= plain_nodes and (hits > 0 or e < 6) and (nodes < plain_nodes or e < 6)


@pytest.mark.parametrize("e", [6, 9, 12])
@pytest.mark.parametrize("which", ["half", "outcome", "empty"])
def test_partial_books_are_sound(gold, books, e, which):
    from connect4_amd.solver import Book
    by_depth, windows = books
    b = by_depth[e]
    book = {"half": lambda: Book(b["exact"].age, b["exact"].words[::2]), "outcome": lambda: b["outcome"],
            "empty": lambda: Book.empty(b["exact"].age)}[which]()
    nodes, hits = search(b["rows"], b["at"], windows, book, gold, b["plain"])
    plain_nodes = sum(a.nodes for name in b["plain"] for a in b["plain"][name])
    if which == "empty":         # nothing to find: the bookless search
        assert (nodes, hits) == (plain_nodes, 0)
    else:
        assert hits > 0 and nodes < plain_nodes


def test_a_book_of_a_ply_no_path_reaches_is_the_bookless_search(gold, books):
    by_depth, windows = books
    b = by_depth[6]
    assert by_depth[12]["exact"].age < 42 - 6
    nodes, hits = search(b["rows"], b["at"], windows, by_depth[12]["exact"], gold, b["plain"])
    assert (nodes, hits) == (sum(a.nodes for name in b["plain"] for a in b["plain"][name]), 0)


def test_a_mirrored_root_hits_the_unmirrored_book(gold, books):
    from connect4_amd.solver import _mirror_bits
    by_depth, windows = books
    b = by_depth[10]
    nodes, hits = search(_mirror_bits(b["rows"]), b["at"], windows, b["exact"], gold)
    assert hits > 0


def test_a_book_at_the_roots_ply_answers_in_the_root(gold, books):
    """The leaves of depth 12 are roots of their own: with their book every interior one is answered by the root's probe,
    one node, and the others by that one node as before."""
    from connect4_amd.solver import _interior_rows, solve_host
    b = books[0][12]
    leaves = b["leaves"]
    leaves = leaves[~(X.four(leaves[:, 0]) | X.four(leaves[:, 1]))][::7]        # the unfinished ones
    inner = _interior_rows(leaves)
    for row, is_inner in zip(leaves, inner):
        at = (int(row[0]), int(row[1]))
        want = solve_host(at, deep=True)
        got = solve_host(at, book=b["exact"])
        assert got[:4] == want[:4] and got.nodes == 1 and got.hits == got.book_probes == int(is_inner)


def test_drive_host_with_a_book(gold, books):
    """The root driver's leaves probe the book like any search: the answers are the bookless driver's, the hits are
    reported per node and per row, and no leaf enters more nodes."""
    from connect4_amd import _lib as L
    from connect4_amd.solver import drive_host
    b = books[0][12]
    rows = b["rows"][::16]
    want, rep0 = drive_host(rows, -1, 1, 2)
    got, rep1 = drive_host(rows, -1, 1, 2, book=b["exact"])
    assert np.array_equal(got.status, want.status) and (got.status == L.SOLVE_SOLVED).all() and np.array_equal(got.bound, want.bound)
    assert np.array_equal(np.sign(got.score), np.sign(want.score))
    assert (rep1["nodes"] <= rep0["nodes"]).all() and (rep0["table_hits"] == 0).all() and (want.table_hits == 0).all()
    assert got.table_hits.sum() > 0 and rep1["table_hits"].sum() >= got.table_hits.max()
