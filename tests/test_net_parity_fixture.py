"""tests/golden/net_parity.json / net_parity_tables.npz (written by tests/golden/gen_net_parity_golden.py from the unmodified
reference): the reference's searches with example_net.pth at 800 simulations -- 48 random positions, four of them at
3200 simulations as well, and every ply of three noisy training games -- each marked `decided` when six re-runs with
every evaluator answer moved by up to tol_f32x3(3) leave its visit counts unchanged.  tests/test_gpu_net_parity.py holds
the GPU nets to the decided ones; here, on the host:
  * the fixture has the shape the GPU test relies on;
  * the CPU oracle, driven by the recorded tables and tapes, reproduces every case that has a table bit for bit
    (with test_oracle_golden.py's 15: about 40 net-driven searches, these at 800 simulations);
  * the float64 model of the net (tests/net_models.float64_outputs) agrees with the reference's float32 answers on every
    table position -- positions that searches and self-play actually reach -- within the bound
    test_net_models.py::test_float64_model_matches_reference_golden states for net_golden.npz's 96 (1e-5)."""
import numpy as np
import pytest
import torch

import net_models as M
from conftest import load_json, load_npz, table_from_npz

F64_VS_REFERENCE = 1e-5     # test_net_models.py::test_float64_model_matches_reference_golden


@pytest.fixture(scope="module")
def fixture():
    return load_json("net_parity.json")


@pytest.fixture(scope="module")
def tables():
    return load_npz("net_parity_tables.npz")


def test_fixture_shape(fixture, tables):
    from connect4_amd.board import Board
    cases = fixture["cases"]
    assert fixture["eps"] == M.tol_f32x3(3) == 16 * 9 * 2.0 ** -22 and fixture["K"] >= 6
    assert len({c["name"] for c in cases}) == len(cases)
    a800 = [c for c in cases if c["family"] == "A" and c["config"]["simulations"] == 800]
    a3200 = [c for c in cases if c["family"] == "A" and c["config"]["simulations"] == 3200]
    b = [c for c in cases if c["family"] == "B"]
    assert len(a800) == 48 and len(a3200) == 4 and len(a800) + len(a3200) + len(b) == len(cases)
    assert len({(c["board"]["c0"], c["board"]["c1"]) for c in a800}) == 48
    assert {(c["board"]["c0"], c["board"]["c1"]) for c in a3200} <= {(c["board"]["c0"], c["board"]["c1"]) for c in a800}
    ages = sorted(c["board"]["age"] for c in a800)
    assert ages[0] == 0 and ages[-1] == 33 and len(set(ages)) >= 30           # spread over 0..33
    assert max(y - x for x, y in zip(ages, ages[1:])) <= 1
    for c in cases:
        assert c["board"]["result"] is None and c["root_N"] == c["config"]["simulations"] + 1
        assert sum(c["N"]) == c["config"]["simulations"]
        assert isinstance(c["decided"], bool) and 0.0 <= c["self_tv"] <= 1.0
        assert c["decided"] == (c["self_tv"] == 0.0)
        bd = Board.from_bits(c["board"]["c0"], c["board"]["c1"])
        assert bd.age == c["board"]["age"] and sorted(bd.valid_moves) == c["board"]["valid"]
    for c in a800 + a3200:
        assert c["noise"] is None and c["uniform"] is None and c["move"] == c["best_move"]
        assert c["config"]["root_dirichlet_alpha"] == 0 and c["config"]["num_sampling_moves"] == 0
    # both decided shares, recomputed, are the recorded ones and at least one half
    for fam in ("A", "B"):
        share = float(np.mean([c["decided"] for c in cases if c["family"] == fam]))
        assert share == fixture["decided_share"][fam] and share >= 0.5
    # family B: three whole games, every ply, each board the previous board plus the previous move
    assert [g["seed"] for g in fixture["games"]] == [0, 1, 2]
    for g in fixture["games"]:
        plies = [c for c in b if c["game"] == g["seed"]]
        assert [c["ply"] for c in plies] == list(range(len(g["moves"]))) and [c["move"] for c in plies] == g["moves"]
        bd = Board()
        for c in plies:
            assert (int(bd.color[0]), int(bd.color[1]), bd.age) == (c["board"]["c0"], c["board"]["c1"], c["ply"])
            cfg = c["config"]
            assert (cfg["simulations"], cfg["root_dirichlet_alpha"], cfg["root_exploration_fraction"],
                    cfg["num_sampling_moves"]) == (800, 0.3, 0.25, 6)
            assert len(c["noise"]) == 7 and (c["uniform"] is not None) == (c["ply"] < 6)
            if c["uniform"] is None:
                assert c["move"] == c["best_move"]
            assert c["policy"] == c["values_policy"] and c["move"] in c["board"]["valid"]
            bd.make_move(c["move"])
        assert bd.result is not None and bd.result.value == g["result"]
    # tables: the first eight of family A and every fourth ply of each game; decided and undecided cases among them
    want = [c["name"] for c in a800[:8]] + [c["name"] for c in b if c["ply"] % 4 == 0]
    assert sorted(fixture["table_cases"]) == sorted(want)
    assert sorted({k.rsplit("__", 1)[0] for k in tables.files}) == sorted(want)
    flags = {c["decided"] for c in cases if c["name"] in want}
    assert flags == {True, False}
    n_pos = sum(len(tables[n + "__c0"]) for n in want)
    print("%d cases (%d + %d + %d), decided shares A %.2f B %.2f, %d tables with %d positions" %
          (len(cases), len(a800), len(a3200), len(b), fixture["decided_share"]["A"], fixture["decided_share"]["B"],
           len(want), n_pos))
    assert n_pos >= 12000


def test_oracle_reproduces_the_table_cases(oracle, fixture, tables):
    """N, W, values_policy, n_expansions and the move, bit for bit, for every case that has a table: the oracle answers
    from the case's float32 position table, takes its gamma draws as the root noise and its uniform for the move."""
    by_name = {c["name"]: c for c in fixture["cases"]}
    assert len(fixture["table_cases"]) >= 20
    for name in fixture["table_cases"]:
        case = by_name[name]
        ev = oracle.TableEvaluator(*table_from_npz(tables, name), prior_f32=True)
        cfg = oracle.make_config(**case["config"])
        b = oracle.Board.from_bits(case["board"]["c0"], case["board"]["c1"])
        assert b.age == case["board"]["age"]
        u = -1.0 if case["uniform"] is None else case["uniform"]
        info, mv, av = oracle.search_and_pick(cfg, b, ev, case["noise"], u)
        assert ev.table.misses == 0 and info.n_evals >= len(tables[name + "__c0"]), name     # (transpositions ask twice)
        assert info.root_visits == case["root_N"] and info.root_value_sum == case["root_W"], name
        assert list(info.child_visits) == case["N"], name
        assert list(info.child_value_sum) == case["W"], name
        assert list(info.child_status) == case["status"], name
        assert list(info.values_policy) == case["values_policy"], name
        assert list(info.visit_policy) == case["visit_policy"], name
        assert list(info.root_prior) == case["root_prior"], name
        assert info.n_expansions == case["n_expansions"] and info.n_nodes == case["n_nodes"], name
        assert info.best_move == case["best_move"] and mv == case["move"], name
        if case["family"] == "B":
            assert (case["value"] is None and np.isnan(av)) or av == case["value"], name


def test_float64_model_matches_the_table_answers(fixture, tables):
    """Every position of every table (about 19 k, as searches and self-play reach them, not random playouts): the
    float64 model against the reference's float32 answers."""
    z = load_npz("net_golden.npz")
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w__")}
    pos = {}
    for name in fixture["table_cases"]:
        c0, c1, v, p = table_from_npz(tables, name)
        for a, b, vv, pp in zip(c0, c1, v, p):
            k = (int(a), int(b))
            if k in pos:                     # one net, one answer per position, whichever search met it
                assert pos[k][0] == vv and np.array_equal(pos[k][1], pp)
            pos[k] = (vv, pp)
    keys = sorted(pos)
    c0 = np.array([k[0] for k in keys], dtype=np.uint64)
    c1 = np.array([k[1] for k in keys], dtype=np.uint64)
    rv = np.array([pos[k][0] for k in keys], dtype=np.float32)
    rp = np.stack([pos[k][1] for k in keys]).astype(np.float32)
    assert rv.min() >= 0.0 and rv.max() <= 1.0 and np.abs(rp.sum(1) - 1.0).max() < 1e-5
    v, p = M.float64_outputs(sd, c0, c1)
    dv, dp = np.abs(v - rv).max(), np.abs(p - rp).max()
    print("float64 model vs the reference on %d table positions: max |dv| %.2e  max |dp| %.2e" % (len(keys), dv, dp))
    assert dv <= F64_VS_REFERENCE and dp <= F64_VS_REFERENCE
