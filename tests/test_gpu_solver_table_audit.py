"""The entries of the solver's transposition table on the GPU (k_solve_search<DEEP_MAX_PLY, TableRef> of
connect4_amd/csrc/c4_solve.hip), read back with solver.Table.read() after the searches have returned and audited by
tests/solver_audit.py: DESIGN 3.13's argument that
answers do not depend on the table holds if every entry is a true bound of its position, and root answers do not show a
false one (tests/test_solver_table_audit_host.py).

* One row is one lane: probes and stores happen in program order, launches one after the other, so the image is defined and
  must be solver.HostTable's word for word, parked or not.
* Many rows, the split, opening positions: store order is the device's own, so every entry is held to the exact score of
  its position instead -- from k_solve_search<MAX_PLY, NoTable> (the default solve(): no table code is compiled into it), and for
  entries with more than 20 empty squares from the table-free deep search under a node budget."""
import time

import numpy as np
import pytest

import solver_audit as A
from conftest import load_npz
from solver_helpers import gpu_oracle, one_lane_is_the_host_model, packed

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ORACLE_MAX_EMPTIES = 20         # k_solve_search<MAX_PLY, NoTable> answers these in about a second (profiles/solver.json)
DEEP_ORACLE_BUDGET = 1 << 16    # nodes a deeper entry gets from the table-free deep search: about 0.3 s a lane


def audited(table, label):
    """Read `table` back and audit it; prints the entries by kind and the violations, returns (violations, report)."""
    t0 = time.perf_counter()
    words = table.read()
    report = {}
    bad = A.audit(words, table.log2_entries, gpu_oracle(ORACLE_MAX_EMPTIES, DEEP_ORACLE_BUDGET), report)
    print("%s: %s; %d violations; read + audit %.2f s" % (label, A.summary(report), len(bad), time.perf_counter() - t0))
    for v in bad[:10]:
        print("   slot %d, word %#x: %s" % v)
    return bad, report


def is_host_answer(res, roots):
    from connect4_amd import _lib as L
    return ((res.status == L.SOLVE_SOLVED).all() and res.outcome.tolist() == [a.outcome for _, a in roots]
            and res.final_age.tolist() == [a.final_age for _, a in roots])


@pytest.fixture(scope="module")
def single_rows():
    """One row at 14, 16 and 20 empty squares: the mover cannot win at once, the host model stores at least 200 entries."""
    return [A.pick_roots(e, 1, seed=7, min_stores=200)[0][0] for e in (14, 16, 20)]


@pytest.fixture(scope="module")
def many_roots():
    """130 roots at 14..20 empty squares (the first 65 for the first call and, mirrored, its other half; the last 65 for the
    call on the warm table), with the host's answers."""
    first, second = [], []
    for e, n in zip(range(14, 21), (10, 9, 9, 9, 9, 9, 10)):
        r = A.pick_roots(e, 2 * n, seed=40 + e)
        first += r[:n]
        second += r[n:]
    assert len(first) == len(second) == 65
    return first, second


# -- 1. one lane is the host model, word for word -----------------------------------------------------------------------------
@pytest.mark.parametrize("log2_entries, per_launch", [(10, None), (10, 256), (14, None), (14, 256)])
def test_one_lane_is_the_host_model_word_for_word(single_rows, log2_entries, per_launch):
    from connect4_amd.solver import HostTable, Table

    def same_step(table, host, row, label):
        return one_lane_is_the_host_model(table, host, row, label, per_launch)

    for row in single_rows:                                  # each row alone, a fresh table
        with Table(log2_entries) as table:
            host = HostTable(log2_entries)
            nodes = same_step(table, host, row, "%d empty squares alone" % (42 - row.age))
            assert host.stores >= 200
            assert per_launch is None or nodes > per_launch          # the lane has parked
    with Table(log2_entries) as table:                       # the three one after the other, one table
        host = HostTable(log2_entries)
        for row in single_rows:
            same_step(table, host, row, "%d empty squares, after the others" % (42 - row.age))
        assert host.hits > 0 and (log2_entries > 10 or host.replaced > 0)


# -- 2. many lanes: every entry is true -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("log2_entries", [10, 14, 20])
@pytest.mark.parametrize("per_launch", [256, None])
def test_many_lanes_write_only_true_entries(many_roots, log2_entries, per_launch):
    from connect4_amd.solver import Table, solve
    first, second = many_roots
    rows = [b for b, _ in first] + [b.create_fliplr() for b, _ in first]
    with Table(log2_entries) as table:
        res = solve(packed(rows), table=table, nodes_per_launch=per_launch)
        assert is_host_answer(res, first + first)
        bad, report = audited(table, "2^%d entries, quota %s, 130 rows" % (log2_entries, per_launch))
        assert bad == [] and report["left_out"] == 0
        assert min(report["lower"], report["upper"], report["exact"]) > 0 and res.table_hits.sum() > 0
        warm = solve(packed([b for b, _ in second]), table=table, nodes_per_launch=per_launch)
        assert is_host_answer(warm, second)
        bad, report = audited(table, "2^%d entries, quota %s, 65 other rows on the warm table" % (log2_entries, per_launch))
        print("   nodes %d + %d, hits %d + %d" % (res.nodes.sum(), warm.nodes.sum(), res.table_hits.sum(), warm.table_hits.sum()))
        assert bad == [] and report["left_out"] == 0
        assert min(report["lower"], report["upper"], report["exact"]) > 0 and warm.table_hits.sum() > 0


# -- 3. the split ---------------------------------------------------------------------------------------------------------------
def test_the_split_writes_only_true_entries():
    from connect4_amd.solver import Table, solve
    roots = A.pick_roots(20, 16, seed=77)
    with Table(14) as table:
        res = solve(packed([b for b, _ in roots]), table=table, split_plies=2)
        assert is_host_answer(res, roots)
        bad, report = audited(table, "split_plies=2, 16 roots at 20 empty squares, 2^14 entries")
        assert bad == [] and report["left_out"] == 0 and report["empties"][19:].sum() == 0       # the descendants have 18
        assert min(report["lower"], report["upper"], report["exact"]) > 0 and res.table_hits.sum() > 0


# -- 4. opening positions -------------------------------------------------------------------------------------------------------
def test_opening_positions_write_only_true_entries():
    """The six rows of solver_open.npz that search most cheaply (25..32 empty squares).  Entries with more than 20 empty
    squares that the table-free deep search does not answer within its budget are left out of the value check: at most
    15 % of the entries may be."""
    from connect4_amd import _lib as L
    from connect4_amd.solver import Table, solve
    z = load_npz("solver_open.npz")
    pick = [61, 37, 0, 57, 3, 36]
    assert z["nodes"][pick].tolist() == [588, 7397, 13317, 15089, 28940, 44226]          # table-free
    rows = np.stack([z["c0"][pick], z["c1"][pick]], axis=1).astype(np.uint64)
    with Table(16) as table:
        res = solve(packed(rows), table=table, nodes_per_launch=256)
        assert (res.status == L.SOLVE_SOLVED).all() and np.array_equal(res.final_age, z["final_age"][pick])
        assert res.outcome.tolist() == z["outcome"][pick].tolist()
        bad, report = audited(table, "6 opening rows, 2^16 entries, quota 256")
    share = report["left_out"] / report["entries"]
    hist = report["empties"]
    print("   empty squares: " + ", ".join("%d: %d" % (e, hist[e]) for e in range(len(hist)) if hist[e]))
    print("   %.1f %% of the entries have at most %d empty squares; %.2f %% are left out of the value check" % (
        100.0 * hist[:ORACLE_MAX_EMPTIES + 1].sum() / report["entries"], ORACLE_MAX_EMPTIES, 100.0 * share))
    assert bad == [] and share <= 0.15
    assert min(report["lower"], report["upper"], report["exact"]) > 0 and res.table_hits.sum() > 0


# -- 5. the read itself -----------------------------------------------------------------------------------------------------------
def test_table_read_sizes_and_clear(single_rows):
    import ctypes as C
    from connect4_amd import _lib as L
    from connect4_amd.solver import Table, solve
    lib = L.load()
    with Table(10) as table:
        assert table.read().dtype == np.uint64 and table.read().shape == (1024,) and not table.read().any()
        buf = (C.c_uint64 * 2048)()
        for n in (0, 1023, 2048):
            assert lib.c4_solve_table_read(table.handle, buf, n) == L.EINVAL and b"1024" in lib.c4_solve_last_error()
        assert lib.c4_solve_table_read(table.handle, None, 1024) == L.EINVAL
        assert lib.c4_solve_table_read(table.handle, buf, 1024) == L.OK and not any(buf)
        solve(packed(single_rows[:1]), table=table)
        assert table.read().any()
        table.clear()
        assert not table.read().any()
    with pytest.raises(ValueError):
        table.read()
