"""The 64-filter reference-precision forward ("f32x3w": net_forward_wave16x, a layer in two cout halves) on the device.

  1. against float64 on the stressed 64-filter nets of net_models.GRID (0, 1 and 7 residual blocks) at tol_f32x3(R), both
     entry points and every batch size bit for bit (one wave; a partial, a full and two workgroups of the four-wave kernel);
  2. over the dynamic range 2^-6 .. 2^8 of the tower's activations;
  3. against the reference's own answers on the positions its 800-simulation searches reached (net64_parity_tables.npz),
     at tol_f32x3(6) + the distance of the recorded float32 answers from float64;
  4. the searches of net64_parity.json as test_gpu_net_parity.py::test_searches_against_the_reference runs the 32-filter
     ones: decided cases must be the reference's search, near-ties replay on the oracle bit for bit, and the persistent
     self-play kernel reaches the stepped roots bit for bit;
  5. fused self-play at 16 and at 32 slots per workgroup: cached answers bit for bit, the same games, oracle replays;
  6. the refusals: "f32x3w" at 32 filters, "f32x3" at 64, C4_FUSED_MODE=wave.
All of them fail without the forward (FusedNet knows no "f32x3w")."""
import numpy as np
import pytest
import torch

import net_models as M
import test_gpu_net_parity as P
from conftest import load_json, load_npz, table_from_npz

pytestmark = pytest.mark.gpu

PREC = "f32x3w"
BATCHES = (1, 3, 4, 5, 9, 17)   # one wave, a partial workgroup of the four-wave kernel, a full one, its boundary, more
TOL_F16 = 2e-2


@pytest.fixture(scope="module")
def positions():
    c0, c1 = M.grid_positions()
    return c0, c1, M.planes_of(c0, c1)


@pytest.fixture(scope="module")
def fixture():
    return load_json("net64_parity.json")


@pytest.fixture(scope="module")
def fixture_net(fixture):
    from connect4_amd.net import NetConfig
    n = fixture["net"]
    return M.stressed_state_dict(NetConfig(filters=n["filters"], n_residuals=n["n_residuals"], n_fc_layers=n["n_fc_layers"]), seed=n["seed"])


def _err(a, b):
    return max(float(np.abs(a[0] - b[0]).max()), float(np.abs(a[1] - b[1]).max()))


# ------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("n_res", [0, 1, 7])
def test_against_float64(positions, n_res):
    from connect4_amd.fused_net import FusedNet
    c0, c1, planes = positions
    sd = M.grid_net(64, n_res)
    net = FusedNet(sd, precision=PREC)
    out = net.evaluate_bits(c0, c1)
    wout = net.evaluate_bits(c0, c1, wave=True)
    assert np.array_equal(out[0], wout[0]) and np.array_equal(out[1], wout[1])
    for n in BATCHES:
        for wave in (False, True):
            v, p = net.evaluate_bits(c0[-n:], c1[-n:], wave=wave)
            assert np.array_equal(v, out[0][-n:]) and np.array_equal(p, out[1][-n:]), (n, wave)
    net.close()
    assert np.isfinite(out[0]).all() and np.isfinite(out[1]).all()
    np.testing.assert_allclose(out[1].sum(1), 1.0, atol=1e-5)
    e64 = _err(out, M.float64_outputs(sd, c0, c1, planes))
    print("64f/%dres %s |kernel - float64| %.3g (tolerance %.3g)" % (n_res, PREC, e64, M.tol_f32x3(n_res)))
    assert e64 <= M.tol_f32x3(n_res)


# ------------------------------------------------------------------------------------------ 2
def test_dynamic_range(positions):
    """As test_gpu_net_float64.py::test_dynamic_range for "f32x3": the tower rescaled by c computes the same function, and the
    kernel holds tol_f32x3 from c = 2^-6 to 2^8; the sweep runs from 2^-12 until the largest activation passes 2^15."""
    from connect4_amd.fused_net import FusedNet
    c0, c1, planes = positions
    n_res = 1
    sd = M.grid_net(64, n_res)
    ref = M.float64_outputs(sd, c0, c1, planes)
    top = M.float64_max_activation(sd, c0, c1, planes)
    holds = {}
    k = -12
    while True:
        c = 2.0 ** k
        sdc = M.rescaled_state_dict(sd, c)
        refc = M.float64_outputs(sdc, c0, c1, planes)
        assert _err(refc, ref) <= 1e-12          # the same function in exact arithmetic
        net = FusedNet(sdc, precision=PREC)
        out = net.evaluate_bits(c0, c1)
        net.close()
        if c * top < 65504 * (1 - 2.0 ** -12):
            assert np.isfinite(out[0]).all() and np.isfinite(out[1]).all(), "non-finite answer at c = 2^%d" % k
        e, tol = _err(out, refc), M.tol_f32x3(n_res)
        holds[k] = e <= tol
        print("64f/%dres %s c = 2^%-3d largest activation %.3g  error %.3g (tolerance %.3g)%s" %
              (n_res, PREC, k, c * top, e, tol, "" if holds[k] else "  EXCEEDED"))
        if c * top > 2.0 ** 15:
            break
        k += 1
    good = [k for k in holds if holds[k]]
    lo = min(good)
    hi = lo
    while hi + 1 in holds and holds[hi + 1]:
        hi += 1
    print("64f/%dres %s holds its tolerance for c = 2^%d .. 2^%d (largest activation %.3g at c = 1)" % (n_res, PREC, lo, hi, top))
    assert all(holds[k] for k in range(-6, 9))


# ------------------------------------------------------------------------------------------ 3
def test_answers_on_the_reference_search_positions(fixture, fixture_net):
    from connect4_amd.fused_net import FusedNet
    npz = load_npz("net64_parity_tables.npz")
    pos = {}
    for name in fixture["table_cases"]:
        for a, b, v, p in zip(*table_from_npz(npz, name)):
            pos[(int(a), int(b))] = (v, p)
    keys = sorted(pos)
    c0 = np.array([k[0] for k in keys], dtype=np.uint64)
    c1 = np.array([k[1] for k in keys], dtype=np.uint64)
    rv = np.array([pos[k][0] for k in keys], dtype=np.float32)
    rp = np.stack([pos[k][1] for k in keys]).astype(np.float32)
    assert len(keys) >= 1000
    recorded_vs_f64 = _err((rv.astype(np.float64), rp.astype(np.float64)), M.float64_outputs(fixture_net, c0, c1))
    tol = M.tol_f32x3(fixture["net"]["n_residuals"]) + recorded_vs_f64
    print("bound on %d positions: tol_f32x3(6) %.3g + |recorded - float64| %.3g = %.3g" %
          (len(keys), M.tol_f32x3(fixture["net"]["n_residuals"]), recorded_vs_f64, tol))
    net = FusedNet(fixture_net, precision=PREC)
    v, p = net.evaluate_bits(c0, c1)
    wv, wp = net.evaluate_bits(c0, c1, wave=True)
    net.close()
    h = FusedNet(fixture_net, precision="f16")
    hv, hp = h.evaluate_bits(c0, c1)
    h.close()
    for name, (gv, gp), t in (("f32x3w c4_net_forward", (v, p), tol), ("f32x3w c4_net_forward_wave", (wv, wp), tol),
                              ("f16 c4_net_forward", (hv, hp), TOL_F16)):
        dv, dp = np.abs(gv - rv).max(), np.abs(gp - rp).max()
        print("%-27s vs the reference: max |dv| %.3g  max |dp| %.3g  (bound %.3g)" % (name, dv, dp, t))
        assert np.isfinite(gv).all() and np.isfinite(gp).all()
        assert dv <= t and dp <= t, name
    assert np.array_equal(v, wv) and np.array_equal(p, wp)


# ------------------------------------------------------------------------------------------ 4
def test_searches_against_the_reference(oracle, fixture, fixture_net, monkeypatch):
    from connect4_amd.board import Board
    from connect4_amd.fused_net import make_selfplay_net, FusedNet
    from connect4_amd.tree import Tree
    net = make_selfplay_net(fixture_net, precision=PREC)
    assert isinstance(net, FusedNet) and net.precision == PREC
    groups = {}
    for c in fixture["cases"]:
        groups.setdefault(P.cfg_key(c["config"]), []).append(c)
    assert len(groups) == 2
    identical = {True: 0, False: 0}
    total = {True: 0, False: 0}
    lost = 0
    for group in groups.values():
        with P.make_engine(group) as eng:
            P.drive_steps(eng, net)
            roots = eng.read_roots()
            assert eng.stats()["bad_evals"] == 0
            for slot, (case, r) in enumerate(zip(group, roots)):
                assert r.state == 2 and (r.color0, r.color1) == (case["board"]["c0"], case["board"]["c1"])
                equal = r.child_visits[:] == case["N"]
                total[case["decided"]] += 1
                identical[case["decided"]] += equal
                if equal:
                    tree = Tree(r, Board.from_bits(case["board"]["c0"], case["board"]["c1"]))
                    assert list(tree.get_visit_count_policy()) == case["visit_policy"], case["name"]
                if case["decided"]:
                    P.check_decided(case, r)
                else:
                    lost += P.replay_on_oracle(oracle, eng, net, slot, case, r)
                    print("%s near-tie %-12s TV against the reference %.4f (the reference against itself under +-tol_f32x3: %.4f)%s" %
                          (PREC, case["name"], P.total_variation(r.child_visits[:], case["N"]), case["self_tv"], "" if equal else "  differs"))
            stepped = [P.root_dict(r) for r in roots]
        monkeypatch.setenv("C4_FUSED_MODE", "split")
        with P.make_engine(group) as eng:
            P.drive_fused(eng, net)
            assert eng.stats()["bad_evals"] == 0
            for case, a, r in zip(group, stepped, eng.read_roots()):
                b = P.root_dict(r)
                assert all(P.same(a[k], b[k]) for k in a), (case["name"], a, b)
    net.close()
    n = total[True] + total[False]
    print("%s: visit counts identical to the reference's on %d of %d searches (%.1f %%): %d of %d decided, %d of %d near-ties; "
          "%d replayed answers came from the net instead of the cache" %
          (PREC, identical[True] + identical[False], n, 100.0 * (identical[True] + identical[False]) / n, identical[True],
           total[True], identical[False], total[False], lost))
    assert n == len(fixture["cases"]) and identical[True] == total[True]


# ------------------------------------------------------------------------------------------ 5
def test_selfplay(oracle, monkeypatch):
    from connect4_amd import _lib as L
    from connect4_amd.config import MCTSConfig
    from connect4_amd.fused_net import FusedNet
    from connect4_amd.selfplay import SelfPlay
    from oracle.replay import oracle_config, random_tapes, replay_game
    net = FusedNet(M.grid_net(64, 7), precision=PREC)
    cfg = MCTSConfig.self_play(24)
    monkeypatch.setenv("C4_FUSED_MODE", "split")
    games = {}
    for mapping in ("default", "32-dense"):
        if mapping == "32-dense":
            monkeypatch.setenv("C4_FUSED_SLOTS", "32")
            monkeypatch.setenv("C4_FUSED_PACK", "dense")
        sp = SelfPlay(net, 64, cfg, seed=4, games_target=48, record_capacity_games=64, use_graph=False, fused_loop=True,
                      steps_per_launch=16, eval_cache_log2_entries=22)
        for _ in range(1000):
            sp.run_steps(64)
            if sp.stats()["active_slots"] == 0:
                break
        st = sp.stats()
        recs = sp.engine.drain_games()
        assert len(recs) == 48 and st["bad_evals"] == 0
        games[mapping] = sorted((r.game_id, list(r.move[:r.length]), list(r.value[:r.length]), r.result) for r in recs)
        roots = [(int(r.color0[i]), int(r.color1[i])) for r in recs for i in range(r.length)]
        c0 = np.array([x[0] for x in roots], dtype=np.uint64)
        c1 = np.array([x[1] for x in roots], dtype=np.uint64)
        v, p, found = sp.engine.cache_lookup(c0, c1)
        print("%s, %s: %d games, %d of %d positions found in the cache" % (PREC, mapping, len(recs), int(found.sum()), len(roots)))
        assert found.mean() > 0.95
        nv, npri = net.evaluate_bits(c0, c1, wave=True)
        assert np.array_equal(v[found], nv[found]) and np.array_equal(p[found], npri[found])
        sp.close()
    assert games["default"] == games["32-dense"]
    monkeypatch.delenv("C4_FUSED_SLOTS")
    monkeypatch.delenv("C4_FUSED_PACK")
    sp = SelfPlay(net, 40, cfg, seed=1, games_target=40, record_capacity_games=40, use_graph=False, fused_loop=True,
                  steps_per_launch=16, rng_mode=L.RNG_TAPE)
    noise, u = random_tapes(40, cfg.root_dirichlet_alpha, seed=2)
    sp.engine.set_tapes(noise, u)
    sp.engine.reset()
    for _ in range(1000):
        sp.run_steps(64)
        if sp.stats()["active_slots"] == 0:
            break
    recs = sp.engine.drain_games()
    assert len(recs) == 40 and sp.stats()["dropped_games"] == 0
    for r in recs[:5]:
        replay_game(oracle_config(cfg), sp.engine, net, r, noise[r.game_id], u[r.game_id])
    sp.close()
    net.close()


# ------------------------------------------------------------------------------------------ 6
def test_refusals(monkeypatch):
    from connect4_amd import _lib as L
    from connect4_amd.config import MCTSConfig
    from connect4_amd.fused_net import FusedNet
    from connect4_amd.selfplay import SelfPlay
    with pytest.raises(L.EngineError, match="C4_NET_F32X3 "):
        FusedNet(M.grid_net(32, 1), precision=PREC)
    with pytest.raises(L.EngineError, match="f32x3w"):
        FusedNet(M.grid_net(64, 1), precision="f32x3")
    assert FusedNet.reference_precision(32) == "f32x3" and FusedNet.reference_precision(64) == PREC
    assert FusedNet.default_precision(64) == "f16"
    net = FusedNet(M.grid_net(64, 1), precision=PREC)
    monkeypatch.setenv("C4_FUSED_MODE", "wave")
    sp = SelfPlay(net, 16, MCTSConfig.self_play(8), seed=1, games_target=16, record_capacity_games=16, use_graph=False,
                  fused_loop=True, steps_per_launch=4)
    with pytest.raises(L.EngineError, match="C4_FUSED_MODE=wave"):
        sp.run_steps(4)
    sp.close()
    net.close()
