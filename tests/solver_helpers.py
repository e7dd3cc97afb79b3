"""What the GPU tests of the exact solver (tests/test_gpu_solver*.py) share: boards and packed tensors, bit-for-bit comparisons
of answers, the table-free GPU oracle of tests/solver_audit.py's audit, and the comparison of one lane's table image with the
host model's.  A plain module: nothing here is a fixture or a test."""
import numpy as np

import solver_audit as A


def boards_of(c0, c1):
    from connect4_amd.board import Board
    return [Board.from_bits(int(a), int(b)) for a, b in zip(c0, c1)]


def packed(rows, cuda=True):
    """int64 [n, 2] tensor of Boards, (color0, color1) pairs or uint64 [n, 2] rows; on the GPU unless cuda=False."""
    import torch
    if not isinstance(rows, np.ndarray):
        rows = np.array([b.color if hasattr(b, "color") else b for b in rows], dtype=np.uint64)
    t = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1, 2).view(np.int64))
    return t.cuda() if cuda else t


def same_bits(a, b):
    return np.asarray(a, dtype=np.float64).tobytes() == np.asarray(b, dtype=np.float64).tobytes()


def same_answers(a, b, rows=slice(None)):
    return (np.array_equal(a.status[rows], b.status[rows]) and same_bits(a.outcome[rows], b.outcome[rows])
            and np.array_equal(a.final_age[rows], b.final_age[rows]) and same_bits(a.value[rows], b.value[rows]))


def gpu_oracle(max_empties, deep_budget):
    """solver_audit.audit's exact_score_of_rows: one batched table-free solve of the decoded positions.  Up to `max_empties`
    empty squares that is the default solve() (k_solve_search<MAX_PLY, NoTable>: no table code is compiled into it); deeper
    rows go to solve(deep=True) under `deep_budget` nodes and stay UNSOLVED where it does not suffice."""
    def exact_score_of_rows(rows):
        from connect4_amd import _lib as L
        from connect4_amd.solver import _popcount64, solve
        age = _popcount64(rows[:, 0] | rows[:, 1])
        out = np.full(len(rows), A.UNSOLVED, dtype=np.int64)
        late = 42 - age <= max_empties
        for pick, kw in ((late, {}), (~late, {"deep": True, "node_budget": deep_budget})):
            if pick.any():
                res = solve(packed(rows[pick]), **kw)
                assert (res.table_hits == 0).all() and np.isin(res.status, (L.SOLVE_SOLVED, L.SOLVE_UNKNOWN)).all()
                assert kw or (res.status == L.SOLVE_SOLVED).all()
                ok = res.status == L.SOLVE_SOLVED
                out[pick] = np.where(ok, A.mover_score(np.where(ok, res.outcome, 0.5), res.final_age, age[pick]), A.UNSOLVED)
        return out

    return exact_score_of_rows


def one_lane_is_the_host_model(table, host, row, label, per_launch=None):
    """Solve `row` alone against the device `table` and, in Python, against the ``HostTable`` `host` that has seen the same rows
    in the same order: the answer, the node count, the hits and every word of the table must be the host model's.  Returns the
    node count."""
    from connect4_amd import _lib as L
    from connect4_amd.solver import solve, solve_host
    hits_before = host.hits
    want = solve_host(row, table=host)
    got = solve(packed([row]), table=table, nodes_per_launch=per_launch)
    image = table.read()
    differ = np.nonzero(image != host.words)[0]
    print("%s: nodes %d (host %d), hits %d (host %d), %d entries (host %d), %d words differ" % (
        label, got.nodes[0], want.nodes, got.table_hits[0], host.hits - hits_before, np.count_nonzero(image),
        np.count_nonzero(host.words), len(differ)))
    assert got.status[0] == want.status == L.SOLVE_SOLVED and (got.outcome[0], got.final_age[0]) == (want.outcome, want.final_age)
    assert len(differ) == 0, [(int(i), hex(int(image[i])), hex(int(host.words[i]))) for i in differ[:8]]
    assert got.nodes[0] == want.nodes and got.table_hits[0] == host.hits - hits_before
    return int(got.nodes[0])
