"""c4_exact_leaves_dev, the kernel alone: the late rows of a batch get the exhaustive oracle's outcome, nothing else moves.

The batch is every row of tests/golden/solver_exact.npz (7,456 undecided positions at 1..22 empty squares; its scores are
``oracle.c4oracle.Exact``'s, pinned to the live oracle by tests/test_exact_oracle.py) followed by the rows of
exact_leaf_cases.extra_rows: the zero row, two finished positions and three rows that are no position.  `values` starts as
a sentinel, 0.25f, which no answer equals.

* max_empties in {0, 8, 14, 22}, budget 2^20 (the file's dearest row takes 74,256 nodes under the full window): the
  overridden rows are exactly the fixture rows with at most that many empty squares, their values are the oracle's outcomes,
  every other row keeps the sentinel's bits, the counters are the host's counts -- the node sum is c4_solve_window_dev's
  table-free count -- and no row is over budget.
* max_empties = 14 with a budget of 8 and of 64: the overridden rows are the rows ``solver.solve_window(rows, -1, 1,
  node_budget=B)`` reports solved, with its outcomes, and the node sum is the sum of its nodes over all late rows.  Both
  budgets leave rows of the fixture unanswered and answer others (asserted).
* n in {1, 63, 64, 65, 257} out of a batch whose late rows are scattered: ragged waves and workgroups; rows beyond n and
  a priors-sized guard buffer behind `values` are untouched.
* Counters accumulate over calls; argument errors are C4_EINVAL with a message."""
import ctypes as C

import numpy as np
import pytest

import exact_leaf_cases as K
import solver_exact_cases as X

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BUDGET = 1 << 20


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def run_overlay(c0_dev, c1_dev, n, max_empties, budget, values, counters):
    from connect4_amd import _lib as L
    from connect4_amd.solver import _check
    stream = torch.cuda.current_stream().cuda_stream
    rc = L.load().c4_exact_leaves_dev(0, C.c_void_p(stream), C.c_void_p(c0_dev.data_ptr()), C.c_void_p(c1_dev.data_ptr()), n, max_empties,
                                      budget, C.c_void_p(values.data_ptr()), None if counters is None else C.c_void_p(counters.data_ptr()))
    _check(rc)
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def batch():
    g = K.fixture_rows()
    g["age"] = K.ages(g["c0"], g["c1"])
    g["exact_value"] = K.value_of_score(g["score"], g["age"])
    g["c0_dev"], g["c1_dev"] = _dev(g["c0"]), _dev(g["c1"])
    return g


@pytest.fixture(scope="module")
def windowed(batch):
    """solver.solve_window(-1, +1), table-free, of the fixture rows with at most 22 / 14 empty squares under the budgets used."""
    from connect4_amd.solver import solve_window
    from solver_helpers import packed
    out = {}
    for e, budgets in ((22, (BUDGET,)), (14, (8, 64))):
        at = np.nonzero(batch["late_ok"] & (batch["empties"] <= e))[0]
        t = packed(np.stack([batch["c0"][at], batch["c1"][at]], axis=1))
        for b in budgets:
            out[(e, b)] = (at, solve_window(t, -1, 1, node_budget=b))
    return out


@pytest.mark.parametrize("max_empties", [0, 8, 14, 22])
def test_late_rows_get_the_oracles_outcome_and_nothing_else_moves(batch, windowed, max_empties):
    from connect4_amd import _lib as L
    n = len(batch["c0"])
    values = torch.full((n,), float(K.SENTINEL), dtype=torch.float32, device="cuda")
    counters = torch.zeros(4, dtype=torch.int64, device="cuda")
    run_overlay(batch["c0_dev"], batch["c1_dev"], n, max_empties, BUDGET, values, counters)
    got = values.cpu().numpy()
    late = batch["late_ok"] & (batch["empties"] <= max_empties)
    assert late.sum() == sum(k for e, k in X.ROWS_PER_EMPTIES.items() if e <= max_empties)
    assert np.array_equal(got != K.SENTINEL, late)
    assert got[late].tobytes() == batch["exact_value"][late].tobytes()
    assert got[~late].tobytes() == np.full(int((~late).sum()), K.SENTINEL).tobytes()
    at, res = windowed[(22, BUDGET)]
    assert (res.status == L.SOLVE_SOLVED).all()
    nodes = int(res.nodes[batch["empties"][at] <= max_empties].sum())
    print("max_empties %d: %d late rows, %d nodes" % (max_empties, late.sum(), nodes))
    assert dict(zip(L.EXACT_LEAVES_COLUMNS, counters.cpu().tolist())) == dict(overridden=int(late.sum()), over_budget=0, nodes=nodes,
                                                                              late=int(late.sum()))


@pytest.mark.parametrize("budget", [8, 64])
def test_small_budgets_answer_what_the_windowed_solver_answers(batch, windowed, budget):
    from connect4_amd import _lib as L
    n = len(batch["c0"])
    values = torch.full((n,), float(K.SENTINEL), dtype=torch.float32, device="cuda")
    counters = torch.zeros(4, dtype=torch.int64, device="cuda")
    run_overlay(batch["c0_dev"], batch["c1_dev"], n, 14, budget, values, counters)
    got = values.cpu().numpy()
    at, res = windowed[(14, budget)]
    solved = res.status == L.SOLVE_SOLVED
    assert ((res.status == L.SOLVE_UNKNOWN) | solved).all()
    print("budget %d: %d of %d late rows answered, %d nodes" % (budget, solved.sum(), len(at), res.nodes.sum()))
    assert 0 < solved.sum() < len(at)               # the fixture has rows on both sides of this budget
    want = np.full(n, K.SENTINEL)
    sign = np.sign(res.score.astype(np.int64))
    outcome = ((np.where(batch["age"][at] & 1, -sign, sign) + 1) * 0.5).astype(np.float32)
    want[at[solved]] = outcome[solved]
    assert got.tobytes() == want.tobytes()
    assert outcome[solved].tobytes() == batch["exact_value"][at[solved]].tobytes()       # and the solver agrees with the oracle
    assert counters.cpu().tolist() == [int(solved.sum()), int((~solved).sum()), int(res.nodes.sum()), len(at)]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_ragged_batches_touch_no_row_beyond_n(batch, n):
    """A shuffled batch of 320 rows -- late rows, deeper rows and the extra rows mixed within every wave -- of which the first
    n are given; `values` has 320 entries and a guard the size of the priors behind it."""
    rng = np.random.RandomState(11)
    pick = np.concatenate([rng.choice(np.nonzero(batch["late_ok"])[0], 320 - 12, replace=False), np.tile(np.nonzero(~batch["late_ok"])[0], 2)])
    rng.shuffle(pick)
    c0, c1 = _dev(batch["c0"][pick]), _dev(batch["c1"][pick])
    buf = torch.full((320 + 320 * 7,), float(K.SENTINEL), dtype=torch.float32, device="cuda")
    counters = torch.zeros(4, dtype=torch.int64, device="cuda")
    run_overlay(c0, c1, n, 12, BUDGET, buf[:320], counters)
    got = buf.cpu().numpy()
    late = batch["late_ok"][pick] & (batch["empties"][pick] <= 12) & (np.arange(320) < n)
    want = np.full(len(got), K.SENTINEL)
    want[:320][late] = batch["exact_value"][pick][late]
    assert got.tobytes() == want.tobytes()
    assert counters.cpu().tolist()[0::3] == [int(late.sum())] * 2 and counters.cpu().tolist()[1] == 0
    if n >= 63:
        assert 0 < late.sum() < n


def test_counters_accumulate_and_are_optional(batch):
    n = len(batch["c0"])
    values = torch.full((n,), float(K.SENTINEL), dtype=torch.float32, device="cuda")
    counters = torch.zeros(4, dtype=torch.int64, device="cuda")
    run_overlay(batch["c0_dev"], batch["c1_dev"], n, 8, 64, values, counters)
    once = counters.cpu().tolist()
    first = values.cpu().numpy()
    run_overlay(batch["c0_dev"], batch["c1_dev"], n, 8, 64, values, counters)
    assert counters.cpu().tolist() == [2 * x for x in once] and once[0] + once[1] == once[3] > 0
    values.fill_(float(K.SENTINEL))
    run_overlay(batch["c0_dev"], batch["c1_dev"], n, 8, 64, values, None)
    assert values.cpu().numpy().tobytes() == first.tobytes()


def test_argument_errors(batch):
    from connect4_amd import _lib as L
    lib = L.load()
    values = torch.full((8,), float(K.SENTINEL), dtype=torch.float32, device="cuda")
    c0, c1, v = (C.c_void_p(t.data_ptr()) for t in (batch["c0_dev"], batch["c1_dev"], values))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for args in ((c0, c1, -1, 8, 64, v, None), (c0, c1, 8, -1, 64, v, None), (c0, c1, 8, L.SOLVE_MAX_EMPTIES + 1, 64, v, None),
                 (c0, c1, 8, 8, 0, v, None), (c0, c1, 8, 8, -5, v, None), (None, c1, 8, 8, 64, v, None), (c0, None, 8, 8, 64, v, None),
                 (c0, c1, 8, 8, 64, None, None)):
        assert lib.c4_exact_leaves_dev(0, stream, *args) == L.EINVAL
        assert lib.c4_solve_last_error()
    assert lib.c4_exact_leaves_dev(0, stream, c0, c1, 0, 8, 64, v, None) == L.OK
    torch.cuda.synchronize()
    assert (values.cpu().numpy() == K.SENTINEL).all()
