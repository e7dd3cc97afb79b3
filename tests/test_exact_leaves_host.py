"""``exact_leaves.overlay_host``: the rule of c4_exact_leaves_dev on the host, against the exhaustive oracle.

300 rows of tests/golden/solver_exact.npz with at most 10 empty squares (30 per count, evenly spread over the file's 512) and
the rows of exact_leaf_cases.extra_rows that are no searchable position.  For E in {0, 6, 10} the overridden rows are exactly
the fixture rows with at most E empty squares, their values are the outcomes ``oracle.c4oracle.Exact`` computes here, and
every other row keeps the bits it came with.  No GPU."""
import numpy as np
import pytest

import exact_leaf_cases as K

PER_COUNT = 30


@pytest.fixture(scope="module")
def rows(oracle):
    z = K.fixture_rows()
    pick = []
    for e in range(1, 11):
        at = np.nonzero(z["late_ok"] & (z["empties"] == e))[0]
        pick.extend(at[np.linspace(0, len(at) - 1, PER_COUNT).astype(np.int64)].tolist())
    pick.extend(np.nonzero(~z["late_ok"])[0].tolist())
    g = {k: v[pick] for k, v in z.items()}
    n_fix = int(g["late_ok"].sum())
    assert n_fix == 10 * PER_COUNT
    with oracle.Exact(20) as memo:
        score, _, status = memo.scores(g["c0"][:n_fix], g["c1"][:n_fix])
    assert (status == oracle.EXACT_SEARCHED).all() and np.array_equal(score, g["score"][:n_fix])
    g["exact_value"] = np.concatenate([K.value_of_score(score, 42 - g["empties"][:n_fix]), np.full(len(pick) - n_fix, K.SENTINEL)])
    assert set(np.unique(g["exact_value"][:n_fix]).tolist()) == {0.0, 0.5, 1.0}
    return g


@pytest.mark.parametrize("max_empties", [0, 6, 10])
def test_overlay_host_is_the_oracle_on_late_rows_and_nothing_elsewhere(rows, max_empties):
    from connect4_amd.exact_leaves import overlay_host
    n = len(rows["c0"])
    # values that are no exact value, different in every row, a NaN and a negative zero among them
    before = (0.125 + 0.25 * np.random.RandomState(3).random_sample(n)).astype(np.float32)
    before[0], before[-1] = np.float32(np.nan), np.float32(-0.0)
    given = before.copy()
    values, overridden = overlay_host(rows["c0"], rows["c1"], given, max_empties)
    assert given.tobytes() == before.tobytes()                      # the argument is not written
    assert values.dtype == np.float32 and overridden.dtype == bool and values.shape == overridden.shape == (n,)
    late = rows["late_ok"] & (rows["empties"] <= max_empties)
    assert np.array_equal(overridden, late)
    assert late.sum() == PER_COUNT * max_empties
    assert values[late].tobytes() == rows["exact_value"][late].tobytes()
    assert values[~late].tobytes() == before[~late].tobytes()


def test_overlay_host_over_budget_rows_keep_their_value(rows):
    """Budget 1 is the root alone: answered are the rows whose root needs no second node, and those answers are the
    oracle's; the rest keep their value."""
    from connect4_amd import _lib as L
    from connect4_amd.exact_leaves import overlay_host
    from connect4_amd.solver import solve_host
    before = np.full(len(rows["c0"]), K.SENTINEL)
    values, overridden = overlay_host(rows["c0"], rows["c1"], before, 10, node_budget=1)
    late = rows["late_ok"]
    solved = np.array([late[i] and solve_host((int(rows["c0"][i]), int(rows["c1"][i])), node_budget=1, window=(-1, 1)).status == L.SOLVE_SOLVED
                       for i in range(len(late))])
    assert np.array_equal(overridden, solved) and 0 < solved.sum() < late.sum()
    assert values[solved].tobytes() == rows["exact_value"][solved].tobytes()
    assert values[~solved].tobytes() == before[~solved].tobytes()


def test_argument_errors(rows):
    from connect4_amd.exact_leaves import MAX_EMPTIES, overlay_host
    c0, c1 = rows["c0"][:4], rows["c1"][:4]
    v = np.zeros(4, dtype=np.float32)
    assert MAX_EMPTIES == 24
    for bad in (-1, MAX_EMPTIES + 1, 2.5, None, True):
        with pytest.raises(ValueError):
            overlay_host(c0, c1, v, bad)
    for bad in (0, -3, 1.5, False):
        with pytest.raises(ValueError):
            overlay_host(c0, c1, v, 6, node_budget=bad)
    with pytest.raises(ValueError):
        overlay_host(c0, c1, v[:3], 6)
    with pytest.raises(ValueError):
        overlay_host(c0[:3], c1, v, 6)
    with pytest.raises(TypeError):
        overlay_host(c0, c1, v)                                     # max_empties has no default
