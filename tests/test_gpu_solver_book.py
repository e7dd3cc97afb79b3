"""The book in the kernel (connect4_amd/csrc/c4_solve.hip book_probe, behind ``book=`` of connect4_amd/solver.py) on the rows
of tests/golden/solver_exact.npz with 19..22 empty squares (32 + 32 + 16 + 16), pinned to the exhaustive oracle.

One book a depth -- a book holds one ply: the distinct descendants four plies down (``_build_graph``), 18..15 empty squares,
solved table-free by the default ``solve``.  Table-free with a book every answer is the fixture's bit for bit and every
node and hit count is the host mirror's (``solve_host(book=)``, ``drive_host(book=)``), whatever the launch quota."""
import numpy as np
import pytest

import solver_audit as A
import solver_exact_cases as X
from conftest import load_npz
from solver_helpers import gpu_oracle, packed

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEPTHS = (19, 20, 21, 22)
PLIES = 4


@pytest.fixture(scope="module")
def cases():
    """Per depth: the rows with what follows from the oracle's scores, the leaves four plies down, their exact and outcome
    books, and the host mirror's (nodes, hits, book probes) of the full-window search with the exact book.  Computed once, not modified."""
    from connect4_amd import _lib as L
    from connect4_amd.solver import Book, _build_graph, _children_host, solve, solve_host, solve_window, value_from_answer
    z = load_npz("solver_exact.npz")
    out = {}
    for e in DEPTHS:
        at = np.nonzero(z["empties"] == e)[0]
        assert len(at) == X.ROWS_PER_EMPTIES[e]
        rows = np.stack([z["c0"][at], z["c1"][at]], axis=1)
        score = z["score"][at].astype(np.int64)
        outcome, final_age = X.answer_of_score(score, 42 - e)
        g = _build_graph(rows, None, None, PLIES, _children_host)
        first = int(g.level_start[-2])
        leaves = np.stack([g.color0[first:], g.color1[first:]], axis=1)
        assert len(leaves) <= len(rows) * 7 ** PLIES
        res = solve(packed(leaves))
        assert not (res.status == L.SOLVE_UNKNOWN).any() and (res.table_hits == 0).all()
        book = Book.from_answers(leaves, res, age=42 - e + PLIES)
        win = solve_window(packed(leaves), -1, 1)
        assert not (win.status == L.SOLVE_UNKNOWN).any()
        host = []
        for r in rows:
            a = solve_host((int(r[0]), int(r[1])), book=book)
            host.append((a.nodes, a.hits, a.book_probes))
        out[e] = {"at": at, "rows": rows, "t": packed(rows), "score": score, "outcome": outcome, "final_age": final_age,
                  "value": value_from_answer(outcome, final_age), "child_score": z["child_score"][at], "leaves": leaves, "book": book,
                  "outcome_book": Book.from_answers(leaves, win, age=42 - e + PLIES), "host": np.array(host, dtype=np.int64)}
        print("%d empty squares: %d rows, %d leaves, %d entries" % (e, len(rows), len(leaves), len(book)))
    yield out
    for c in out.values():
        c["book"].close()
        c["outcome_book"].close()


def assert_answers(res, c, label):
    from connect4_amd import _lib as L
    assert (res.status == L.SOLVE_SOLVED).all(), label
    assert np.array_equal(res.outcome, c["outcome"]) and np.array_equal(res.final_age, c["final_age"]), label
    assert res.value.tobytes() == c["value"].tobytes(), label


# -- 1, 2. the entry points, and the launch quota -------------------------------------------------------------------------------
@pytest.mark.parametrize("quota", [None, 64])
def test_solve_is_the_fixture_and_the_host_mirror(cases, quota):
    from connect4_amd.solver import solve
    for e, c in cases.items():
        res = solve(c["t"], book=c["book"], nodes_per_launch=quota)
        assert_answers(res, c, "solve, %d empty" % e)
        assert np.array_equal(res.nodes, c["host"][:, 0]) and np.array_equal(res.table_hits, c["host"][:, 1]), e
        plain = solve(c["t"], deep=True)
        assert (res.nodes <= plain.nodes).all() and res.nodes.sum() < plain.nodes.sum()
        # a row has hits iff its search reaches the book's ply (the host mirror counts the nodes at which it looks the book
        # up; the book is complete and exact, so every lookup is a hit), and only such a row can have saved a node
        reaches = c["host"][:, 2] > 0
        assert reaches.any() and np.array_equal(res.table_hits > 0, reaches) and reaches[res.nodes < plain.nodes].all()
        rows = [(int(a), int(b)) for a, b in c["rows"]]        # the entry point that takes host arrays
        again = solve(rows, book=c["book"], nodes_per_launch=quota)
        assert np.array_equal(again.nodes, res.nodes) and np.array_equal(again.table_hits, res.table_hits)
        assert_answers(again, c, "c4_solve_deep, %d empty" % e)


@pytest.mark.parametrize("quota", [None, 64])
def test_windows_are_the_oracles_and_the_host_mirrors(cases, quota):
    from connect4_amd import _lib as L
    from connect4_amd.solver import solve_host, solve_window
    for e, c in cases.items():
        full = np.zeros(max(c["at"]) + 1, dtype=np.int64)
        full[c["at"]] = c["score"]
        for name, alpha, beta in X.windows(full):
            a, b = alpha[c["at"]], beta[c["at"]]
            res = solve_window(c["t"], a, b, book=c["book"], nodes_per_launch=quota)
            assert (res.status == L.SOLVE_SOLVED).all()
            assert len(X.window_violations(res.score, res.bound, a, b, c["score"])) == 0, (e, name)
            for i, r in enumerate(c["rows"]):
                want = solve_host((int(r[0]), int(r[1])), window=(int(a[i]), int(b[i])), book=c["book"])
                assert (res.score[i], res.bound[i], res.nodes[i], res.table_hits[i]) == (want.score, want.bound, want.nodes, want.hits), (e, name, i)


def test_outcomes_labels_split_and_driver(cases):
    from connect4_amd import _lib as L
    from connect4_amd.solver import drive_host, label, label_values, outcomes, solve, solve_window
    for e, c in cases.items():
        book = c["book"]
        assert outcomes(c["t"], book=book).tobytes() == c["outcome"].tobytes()
        v, keep, prior = X.labels_of_children(c["score"], c["child_score"])
        for how in ("staged", "values", "exact"):
            ls, report = (label(c["t"], exact=False, book=book) if how == "staged" else label_values(c["t"], book=book) if how == "values"
                          else label(c["t"], book=book))
            assert report["labelled"] == len(c["rows"]) and report["unknown"] == 0 and report["table_hits"] > 0 and report["book_age"] == book.age
            assert np.array_equal(ls.boards.cpu().numpy().view(np.uint64), c["rows"])
            assert ls.values.cpu().numpy().tobytes() == c["outcome"].astype(np.float32).tobytes()
            assert (ls.priors is None) if how == "values" else ls.priors.cpu().numpy().tobytes() == prior.tobytes()
        assert_answers(solve(c["t"], split_plies=2, book=book), c, "split, %d empty" % e)
        for quota in (None, 64):
            got = solve_window(c["t"], -1, 1, driver_plies=2, book=book, nodes_per_launch=quota)
            want, _ = drive_host(c["rows"], -1, 1, 2, book=book, nodes_per_launch=quota)
            assert (got.status == L.SOLVE_SOLVED).all() and np.array_equal(np.sign(got.score), np.sign(c["score"]))
            for f in ("status", "score", "bound", "nodes", "table_hits"):
                assert np.array_equal(getattr(got, f), getattr(want, f)), (e, quota, f)
            assert got.table_hits.sum() > 0


# -- 3. where the book sits --------------------------------------------------------------------------------------------------------
def test_book_placements(cases):
    from connect4_amd.solver import Book, _interior_rows, solve
    c, other = cases[19], cases[22]
    plain = solve(c["t"], deep=True)
    own = Book.from_answers(c["rows"], plain)
    try:
        res = solve(c["t"], book=own)             # at the roots' own ply: the root's probe answers, no move is entered
        assert_answers(res, c, "own ply")
        assert (res.nodes == 1).all() and np.array_equal(res.table_hits, _interior_rows(c["rows"]).astype(np.int64))
    finally:
        own.close()
    early = Book.from_answers(other["rows"], solve(other["t"], deep=True))      # 20 stones: no search from 23 stones gets there
    empty = Book.empty(c["book"].age)
    try:
        for book in (early, empty):
            res = solve(c["t"], book=book)
            assert_answers(res, c, "no entry to find")
            assert np.array_equal(res.nodes, plain.nodes) and (res.table_hits == 0).all()
    finally:
        early.close()
        empty.close()


# -- 4. with a table ---------------------------------------------------------------------------------------------------------------
def as_table_images(words, log2_entries):
    """The book's words laid into table images by the table's slot function -- a word whose slot is taken goes to the next
    image -- so that solver_audit.audit applies to them as it stands."""
    from connect4_amd.solver import _TT_HASH, _TT_KEY_MASK
    slot = ((words & np.uint64(_TT_KEY_MASK)) * np.uint64(_TT_HASH)) >> np.uint64(64 - log2_entries)
    images, left = [], np.arange(len(words))
    while len(left):
        _, first = np.unique(slot[left], return_index=True)
        image = np.zeros(1 << log2_entries, dtype=np.uint64)
        image[slot[left[first]].astype(np.int64)] = words[left[first]]
        images.append(image)
        left = np.delete(left, first)
    return images


def test_table_and_book_together(cases):
    from connect4_amd.solver import Table, solve
    exact_score_of_rows = gpu_oracle(24, 1 << 26)
    for e, c in cases.items():
        with Table(16) as table:
            res = solve(c["t"], table=table, book=c["book"])
            assert_answers(res, c, "table and book, %d empty" % e)
            assert res.table_hits.sum() > 0
            assert table.book is None
            again = solve(c["t"], table=table)          # the book is detached again: the table alone
            assert_answers(again, c, "table alone, %d empty" % e)
            table.attach_book(c["outcome_book"])        # an attachment of the caller's survives a call's own book
            assert_answers(solve(c["t"], table=table, book=c["book"]), c, "two books, %d empty" % e)
            assert table.book is c["outcome_book"]
            kept = solve(c["t"], table=table)
            assert_answers(kept, c, "attached book, %d empty" % e)
            assert kept.table_hits.sum() > 0
            table.attach_book(None)
            bad = A.audit(table.read(), 16, exact_score_of_rows)
        assert bad == [], bad[:5]
        report, n = {}, 0
        for image in as_table_images(c["book"].words, 20):
            assert A.audit(image, 20, exact_score_of_rows, report) == []
            n += report["entries"]
            assert report["left_out"] == 0
        assert n == len(c["book"])


# -- 5. partial books and mirror images -------------------------------------------------------------------------------------------
def test_partial_books_and_mirrored_roots(cases):
    from connect4_amd.solver import Book, _mirror_bits, solve, solve_host
    for e, c in cases.items():
        plain = solve(c["t"], deep=True)
        half = Book(c["book"].age, c["book"].words[::2])
        try:
            for name, book in (("half", half), ("outcome", c["outcome_book"])):
                res = solve(c["t"], book=book)
                assert_answers(res, c, "%s book, %d empty" % (name, e))
                assert (res.nodes <= plain.nodes).all() and res.table_hits.sum() > 0
                i = int(np.argmax(res.nodes))               # the dearest row against the host mirror
                want = solve_host((int(c["rows"][i, 0]), int(c["rows"][i, 1])), book=book)
                assert (res.nodes[i], res.table_hits[i]) == (want.nodes, want.hits)
        finally:
            half.close()
        m = _mirror_bits(c["rows"])
        res = solve(packed(m), book=c["book"])
        assert_answers(res, c, "mirrored roots, %d empty" % e)
        assert res.table_hits.sum() > 0
        for i in range(0, len(m), 5):
            want = solve_host((int(m[i, 0]), int(m[i, 1])), book=c["book"])
            assert (res.nodes[i], res.table_hits[i]) == (want.nodes, want.hits)


def test_the_abi_refuses_what_it_cannot_probe(cases):
    import ctypes as C
    from connect4_amd import _lib as L
    from connect4_amd.solver import Table, _mirror_key, _ptr
    lib, h = L.load(), C.c_void_p()
    book = cases[19]["book"]
    w = book.words
    assert lib.c4_solve_book_create(0, _ptr(w), len(w), 42, C.byref(h)) == L.EINVAL
    assert lib.c4_solve_book_create(0, _ptr(w), -1, book.age, C.byref(h)) == L.EINVAL
    assert lib.c4_solve_book_create(0, _ptr(w), len(w), book.age - 1, C.byref(h)) == L.EINVAL       # keys of another ply
    no_position = np.array([5 | (64 << 49) | (3 << 56)], dtype=np.uint64)
    assert lib.c4_solve_book_create(0, _ptr(no_position), 1, 2, C.byref(h)) == L.EINVAL
    assert lib.c4_solve_book_create(0, None, 3, book.age, C.byref(h)) == L.EINVAL
    assert lib.c4_solve_book_create(0, _ptr(w), len(w), book.age, None) == L.EINVAL
    twice = np.concatenate([w[:4], w[:1]])
    assert lib.c4_solve_book_create(0, _ptr(twice), len(twice), book.age, C.byref(h)) == L.EINVAL
    keys = w & np.uint64((1 << 49) - 1)
    i = int(np.nonzero(_mirror_key(keys) != keys)[0][0])
    other = np.array([(int(w[i]) & ~((1 << 49) - 1)) | int(_mirror_key(keys[i:i + 1])[0])], dtype=np.uint64)
    assert lib.c4_solve_book_create(0, _ptr(other), 1, book.age, C.byref(h)) == L.EINVAL
    assert lib.c4_solve_table_attach_book(None, None) == L.EINVAL and lib.c4_solve_table_create_entryless(0, None) == L.EINVAL
    with Table.entryless() as t:
        with pytest.raises(L.EngineError):
            t.read()
        with pytest.raises(L.EngineError):
            t.clear()


# -- 6. a whole ply on the device --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [5, 6, 8])
@pytest.mark.parametrize("unforced", [False, True])
def test_enumerate_ply_on_the_device_is_the_hosts(k, unforced):
    from connect4_amd.solver import enumerate_ply
    host, dev = enumerate_ply(k, unforced), enumerate_ply(k, unforced, device=0)
    assert dev.dtype == np.uint64 and dev.tobytes() == host.tobytes() and dev.shape == host.shape
