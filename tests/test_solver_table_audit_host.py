"""The host's statement of the solver's transposition table (solver.HostTable, solver.entry_fields) and the audit of its
entries (tests/solver_audit.py), no GPU: entry_fields inverts the key on every fixture position; tables filled by the host
mirror under the kernel's slots and always-replace hold only true bounds; and the audit finds the false entries of three
mutated store rules whose root answers barely move -- which is why roots alone do not pin the table
(tests/test_gpu_solver_table_audit.py runs the same audit on the device's table)."""
import numpy as np
import pytest

import solver_audit as A
from conftest import load_npz

DEPTHS = (14, 16, 20)


@pytest.fixture(scope="module")
def roots():
    """Two roots per depth with their table-free answers: [(board, HostAnswer of solve_host(deep=True))]."""
    from connect4_amd.solver import solve_host
    return [(b, solve_host(b, deep=True)) for e in DEPTHS for b, _ in A.pick_roots(e, 2, seed=e)]


@pytest.fixture(scope="module")
def oracle():
    return A.host_oracle({})


def fill(table, roots):
    """Solve the roots one after the other against `table`: the number of answers that are not the table-free ones."""
    from connect4_amd.solver import solve_host
    wrong = 0
    for b, free in roots:
        a = solve_host(b, table=table)
        wrong += (a.status, a.outcome, a.final_age) != (free.status, free.outcome, free.final_age)
    return wrong


def fixture_positions():
    from connect4_amd.solver import _mirror_bits
    rows = np.concatenate([np.stack([z["c0"], z["c1"]], axis=1).astype(np.uint64)
                           for z in (load_npz("solver.npz"), load_npz("solver_deep.npz"), load_npz("solver_open.npz"))])
    return np.concatenate([rows, _mirror_bits(rows)])


def test_entry_fields_inverts_the_key_on_every_fixture_position():
    from connect4_amd.board import BOTTOM
    from connect4_amd.solver import entry_fields
    rows = fixture_positions()
    assert len(rows) == 2 * (64 + 256 + 62)
    occ = rows[:, 0] | rows[:, 1]
    age = np.array([bin(int(x)).count("1") for x in occ])
    mine = np.where(age & 1, rows[:, 1], rows[:, 0])
    key = mine + occ + np.uint64(BOTTOM)
    assert (key < np.uint64(1 << 49)).all() and len(set(key.tolist())) == len(set(map(tuple, rows.tolist())))    # injective
    score = (np.arange(len(rows)) % 79) - 39
    kind = np.arange(len(rows)) % 3 + 1
    words = key | ((score + 64).astype(np.uint64) << np.uint64(49)) | (kind.astype(np.uint64) << np.uint64(56))
    words = np.stack([words, np.zeros_like(words)], axis=1).reshape(-1)        # empty words in between are skipped
    e = entry_fields(words)
    assert np.array_equal(e.index, 2 * np.arange(len(rows))) and np.array_equal(e.key, key)
    assert np.array_equal(e.score, score) and np.array_equal(e.kind, kind) and np.array_equal(e.age, age)
    assert np.array_equal(e.mine, mine) and np.array_equal(e.occ, occ)
    assert np.array_equal(e.color0, rows[:, 0]) and np.array_equal(e.color1, rows[:, 1])
    assert e.key.dtype == e.mine.dtype == e.occ.dtype == e.color0.dtype == e.color1.dtype == np.uint64


def test_the_audits_position_tests_are_the_solvers():
    """solver_audit writes the position tests out again on arrays: they must say what solver._classify and
    solver._winning_squares say, on the fixtures and on positions that are finished or not positions at all."""
    from connect4_amd import _lib as L
    from connect4_amd.board import Board, _wins
    from connect4_amd.solver import DEEP_MAX_EMPTIES, _classify, _winning_squares, random_playout
    rows = fixture_positions().tolist()
    won = Board()
    for m in (3, 2, 3, 2, 3, 2, 3):
        won.make_move(m)
    c0, c1 = rows[0]
    rows += [list(won.color), [c0, c1 | (c0 & -c0)], [0b1111 | 1 << 14, 0b1111 << 7], [c0 | 1 << 48, c1], [1 << 1, 0], [0, 1], [0, 0],
             [c0 | c1, 0]]
    rng = np.random.RandomState(3)
    for n in (36, 38, 40, 41):                                                   # the end of the board
        for _ in range(8):
            rows.append(list(random_playout(rng, n).color))
    full = Board()
    for m in [0, 1, 0, 1, 0, 1, 1, 0, 1, 0, 1, 0, 2, 3, 2, 3, 2, 3, 3, 2, 3, 2, 3, 2, 4, 5, 4, 5, 4, 5, 5, 4, 5, 4, 5, 4, 6, 6, 6, 6, 6, 6]:
        full.make_move(m)
    rows.append(list(full.color))
    a = np.array(rows, dtype=np.uint64)
    want = np.array([_classify(int(x), int(y), DEEP_MAX_EMPTIES) == L.SOLVE_SOLVED for x, y in rows])
    assert np.array_equal(A.searchable(a[:, 0], a[:, 1]), want) and want.any() and (~want).sum() >= 8
    ok = a[want]
    occ = ok[:, 0] | ok[:, 1]
    for p in (ok[:, 0], ok[:, 1]):
        assert A.winning_squares(p, occ).tolist() == [_winning_squares(int(x), int(o)) for x, o in zip(p, occ)]
    for p in (a[:, 0], a[:, 1]):
        assert A.wins(p).tolist() == [_wins(int(x)) for x in p]


@pytest.mark.parametrize("log2_entries", [10, 14])
def test_host_tables_are_sound(roots, oracle, log2_entries):
    from connect4_amd.solver import HostTable
    table = HostTable(log2_entries)
    assert fill(table, roots) == 0
    report = {}
    bad = A.audit(table.words, log2_entries, oracle, report)
    print("2^%d entries: %d stores, %d replaced another key; %s; %d violations" % (
        log2_entries, table.stores, table.replaced, A.summary(report), len(bad)))
    assert bad == [] and report["left_out"] == 0
    assert report["entries"] >= 200 and min(report["lower"], report["upper"], report["exact"]) > 0
    if log2_entries == 10:
        assert table.replaced > 0                       # always-replace has replaced
    assert report["entries"] == np.count_nonzero(table.words) <= table.stores - table.replaced


def test_a_table_that_never_replaces_is_the_dict(roots):
    """With room for every key HostTable is the dict it stands in for: the same nodes, the same entries.  And the dict path
    answers what it answered: the table-free answers."""
    from connect4_amd.solver import HostTable, _Search, solve_host
    as_dict, table = {}, HostTable(26)      # zero pages nobody touches: no key shares a slot (replaced == 0 below says so)
    for b, free in roots:
        a, t = solve_host(b, table=as_dict), solve_host(b, table=table)
        assert a == t and a[:4] == free[:4] and a.nodes <= free.nodes
    assert table.replaced == 0 and table.stores >= len(as_dict) >= 200
    assert all(table.get(key) == entry for key, entry in as_dict.items())
    assert table.get(12345) is None and HostTable(10).get(as_dict.popitem()[0]) is None
    assert isinstance(_Search(1, table).table, HostTable)
    with pytest.raises(ValueError):
        HostTable(9)


def mutants():
    from connect4_amd.solver import _EXACT, _LOWER, _UPPER, HostTable

    class UpperAsExact(HostTable):
        def __setitem__(self, key, entry):
            super().__setitem__(key, (_EXACT if entry[0] == _UPPER else entry[0], entry[1]))

    class LowerAsExact(HostTable):
        def __setitem__(self, key, entry):
            super().__setitem__(key, (_EXACT if entry[0] == _LOWER else entry[0], entry[1]))

    class OffByOne(HostTable):
        def __setitem__(self, key, entry):
            super().__setitem__(key, (entry[0], entry[1] + 1))

    return [UpperAsExact, LowerAsExact, OffByOne]


def test_the_audit_is_not_vacuous(roots, oracle):
    """Three wrong store rules (the kernel is not touched): each fills a table with false entries while the roots hardly
    notice, and the audit must report them on the inputs on which the store rule as written audits clean."""
    from connect4_amd.solver import HostTable
    clean = HostTable(12)
    report = {}
    assert fill(clean, roots) == 0 and A.audit(clean.words, 12, oracle, report) == []
    assert min(report["lower"], report["upper"], report["exact"]) > 0          # every kind is there to be got wrong
    for cls in mutants():
        table = cls(12)
        wrong = fill(table, roots)
        report = {}
        bad = A.audit(table.words, 12, oracle, report)
        false_entries = [v for v in bad if v[2].startswith("false entry")]
        print("%s: %s; %d violations, %d of them false entries; %d of %d root answers changed" % (
            cls.__name__, A.summary(report), len(bad), len(false_entries), wrong, len(roots)))
        assert len(false_entries) >= 1 and report["left_out"] <= len(bad) - len(false_entries)    # left out: out of range only


def test_the_structural_checks_fire(oracle):
    """One sound entry, then the same entry spoilt in each way the structural half of the audit looks for."""
    from connect4_amd.board import BOTTOM, Board
    from connect4_amd.solver import _LOWER, HostTable, solve_host
    (b, _), = A.pick_roots(16, 1, seed=1)
    table = HostTable(10)
    solve_host(b, table=table)
    assert A.audit(table.words, 10, oracle) == []
    at = int(np.nonzero(table.words)[0][0])
    word = int(table.words[at])

    def what(words):
        return sorted(set(w for _, _, w in A.audit(np.array(words, dtype=np.uint64), 10, oracle)))

    def image(slot, w):
        words = [0] * 1024
        words[slot] = w
        return words

    def entry(board, score, kind=_LOWER, table=HostTable(10)):
        c0, c1 = board.color
        key = (c1 if board.age & 1 else c0) + (c0 | c1) + BOTTOM
        return image(table.slot(key), key | (score + 64) << 49 | kind << 56)

    assert what(image(at, word)) == []
    assert what(image(at, word | 1 << 60)) == ["bits 58..63 are not zero"]
    assert what(image(at, word & ~(3 << 56))) == ["the kind is none of lower, upper, exact"]
    assert what(image(at ^ 1, word)) == ["the word is not in the slot its key hashes to"]
    assert "the key is no position" in what(image(at, word & ~0x7f))             # a column field of 0
    def play(moves):
        board = Board()
        for m in moves:
            board.make_move(m)
        return board

    assert what(entry(play([3, 2, 3, 2, 3, 2, 3]), 0)) == ["the position is invalid or finished"]
    assert what(entry(play([3, 2, 3, 2, 3, 2]), 0)) == ["the mover wins at once: no interior node"]
    late = A.pick_roots(8, 1, seed=1, min_stores=1)[0][0]                       # age 34: scores -5 .. 6
    assert what(entry(late, 7)) == what(entry(late, -6)) == ["the score is outside the window enter_node allows at this age"]
    later = A.pick_roots(5, 1, seed=1, min_stores=0)[0][0]
    assert what(entry(later, 0)) == ["fewer than TT_MIN_EMPTIES empty squares"]


def test_table_read_refuses_a_null_argument():
    import ctypes as C
    import __graft_entry__ as g
    from connect4_amd import _lib as L
    g.build_engine()
    lib = L.load()
    buf = (C.c_uint64 * 1024)()
    assert lib.c4_solve_table_read(None, buf, 1024) == L.EINVAL and b"null" in lib.c4_solve_last_error()
