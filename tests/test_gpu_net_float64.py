"""The fused network forwards against float64 models (tests/net_models.py) on stressed nets -- per-channel batch norm,
non-zero biases everywhere, answers that vary strongly between positions -- over the configurations c4_net_create
accepts: 32 filters with 0, 1, 2, 5 and 16 residual blocks in both precisions, 64 filters with 0, 1 and 7, value-head
Linear stacks of 0, 1, 3 and 6 layers.

Every test runs the nets of net_models.grid_net on net_models.grid_positions, the very nets and positions
test_net_models.py shows to be non-degenerate and sensitive to the modelled mistakes.

Tolerances (derivations in net_models.tol_f32x3 / f16_tolerances):
  * "f32x3" vs float64_outputs: 16 x (2R + 3) x 2^-22, fixed before the first run on the device (measured: <= 6.2e-6);
  * "f16" and 64 filters vs fp16_storage_outputs, per position: at most 3x the largest difference of an fp32-accumulating
    copy of the model from the model + 1e-5 (1e-5 without residual blocks), and 1.5x its mean difference + 4e-5 (raised
    twice after runs on the device; f16_tolerances says why); and the existing
    2e-2 against float64 wherever the fp16 storage itself (|fp16_storage_outputs - float64_outputs|) stays below it.
Both entry points (c4_net_forward, c4_net_forward_wave) must agree bit for bit, at every batch size.

Dynamic range: a net whose tower activations are all multiplied by a power of two c computes the same function
(rescaled_state_dict).  Swept from c = 2^-12 up to the first c at which the float64 model's largest activation passes
2^15, f32x3 holds its tolerance and the fp16 forwards their mean bound against fp16_storage_outputs over the whole sweep that
keeps every activation finite in fp16.  The test asserts 2^-6 .. 2^8 and prints the range it finds (first measured
on MI355X: 2^-12 .. 2^13 for each of the three nets, whose largest activation is about 6 at c = 1)."""
import numpy as np
import pytest

import net_models as M

pytestmark = pytest.mark.gpu

RAGGED = (1, 7, 9, 17)
F16_VS_F64 = 2e-2


@pytest.fixture(scope="module")
def positions():
    c0, c1 = M.grid_positions()
    return c0, c1, M.planes_of(c0, c1)


def _err(a, b):
    return max(float(np.abs(a[0] - b[0]).max()), float(np.abs(a[1] - b[1]).max()))


@pytest.mark.parametrize("filters,n_res,n_fc,prec", [(f, r, fc, p) for f, r, fc, ps in M.GRID for p in ps])
def test_fused_net_vs_float64(positions, filters, n_res, n_fc, prec):
    from connect4_amd.fused_net import FusedNet, fold_for_fused
    c0, c1, planes = positions
    sd = M.grid_net(filters, n_res)
    net = FusedNet(sd, precision=prec)
    out = net.evaluate_bits(c0, c1)
    wout = net.evaluate_bits(c0, c1, wave=True)
    assert np.array_equal(out[0], wout[0]) and np.array_equal(out[1], wout[1])
    for n in RAGGED:
        for wave in (False, True):
            v, p = net.evaluate_bits(c0[-n:], c1[-n:], wave=wave)
            assert np.array_equal(v, out[0][-n:]) and np.array_equal(p, out[1][-n:])
    net.close()
    assert np.isfinite(out[0]).all() and np.isfinite(out[1]).all()
    np.testing.assert_allclose(out[1].sum(1), 1.0, atol=1e-5)
    ref = M.float64_outputs(sd, c0, c1, planes)
    e64 = _err(out, ref)
    tag = "%df/%2dres/%dfc %-5s" % (filters, n_res, n_fc, prec)
    if prec == "f32x3":
        print("%s |kernel - float64| %.3g (tolerance %.3g)" % (tag, e64, M.tol_f32x3(n_res)))
        assert e64 <= M.tol_f32x3(n_res)
        return
    m16 = M.fp16_storage_outputs(sd, c0, c1, planes)
    e = M.per_position_error(out, m16)
    tmax, tmean = M.f16_tolerances(fold_for_fused(sd), planes)
    room = _err(m16, ref)
    print("%s |kernel - fp16 storage model| max %.3g (tolerance %.3g) mean %.3g (tolerance %.3g)  |kernel - float64| %.3g"
          "  |fp16 model - float64| %.3g" % (tag, e.max(), tmax, e.mean(), tmean, e64, room))
    assert e.max() <= tmax and e.mean() <= tmean
    if room < F16_VS_F64:
        assert e64 <= F16_VS_F64


@pytest.mark.parametrize("filters,n_res,prec", [(32, 2, "f32x3"), (32, 2, "f16"), (64, 1, "f16")])
def test_dynamic_range(positions, filters, n_res, prec):
    """f16: the mean bound of f16_tolerances at each scale (the fp32-accumulating copy of the model runs at that scale);
    the max and its bound are printed.  (Asserting the max as well failed on the device for the 1-block 64-filter net at
    c = 2^-6 and 2^-4 -- 3.5e-4 and 5.5e-4 against 3.4e-4 and 2.9e-4 -- where small activations reach fp16's subnormal
    range and a one-block net's few flips decide the largest error; the error is exactly 1.08e-4 at every c >= 2^-2,
    and far from the O(1) a flushed subnormal would cost at c = 2^-12, where most activations are subnormal.)"""
    from connect4_amd.fused_net import FusedNet, fold_for_fused
    c0, c1, planes = positions
    sd = M.grid_net(filters, n_res)
    ref = M.float64_outputs(sd, c0, c1, planes)
    top = M.float64_max_activation(sd, c0, c1, planes)
    holds = {}
    k = -12
    while True:
        c = 2.0 ** k
        sdc = M.rescaled_state_dict(sd, c)
        refc = M.float64_outputs(sdc, c0, c1, planes)
        assert _err(refc, ref) <= 1e-12          # the same function in exact arithmetic
        net = FusedNet(sdc, precision=prec)
        out = net.evaluate_bits(c0, c1)
        net.close()
        finite16 = c * top < 65504 * (1 - 2.0 ** -12)
        if finite16:
            assert np.isfinite(out[0]).all() and np.isfinite(out[1]).all(), "non-finite answer at c = 2^%d" % k
        if prec == "f32x3":
            e, tol = _err(out, refc), M.tol_f32x3(n_res)
            holds[k] = e <= tol
        else:
            pe = M.per_position_error(out, M.fp16_storage_outputs(sdc, c0, c1, planes))
            tmax, tol = M.f16_tolerances(fold_for_fused(sdc), planes)
            e = float(pe.mean())
            holds[k] = e <= tol
            print("    max error %.3g (max bound %.3g)" % (pe.max(), tmax))
        print("%df/%dres %-5s c = 2^%-3d largest activation %.3g  error %.3g (tolerance %.3g)%s" %
              (filters, n_res, prec, k, c * top, e, tol, "" if holds[k] else "  EXCEEDED"))
        if c * top > 2.0 ** 15:
            break
        k += 1
    good = [k for k in holds if holds[k]]
    lo = min(good)
    hi = lo
    while hi + 1 in holds and holds[hi + 1]:
        hi += 1
    print("%df/%dres %-5s holds its tolerance for c = 2^%d .. 2^%d (largest activation %.3g at c = 1)" %
          (filters, n_res, prec, lo, hi, top))
    assert all(holds[k] for k in range(-6, 9))


@pytest.mark.parametrize("kind", ["32f-0-f32x3", "32f-16-f32x3", "32f-16-f16", "64f-7-f16"])
def test_selfplay_caches_the_stressed_nets_answers(oracle, monkeypatch, kind):
    """Short fused self-play runs in the default split mode: every evaluation-cache entry -- of the games' positions and
    of their children (speculative passes of the fp16 net) -- equals evaluate_bits(wave=True) bit for bit.  The fp16 run
    uses 32 slots per workgroup, where network waves evaluate two waiting positions per pass.  The 16-block fp16 net
    also plays the same games, id by id, in the wave-autonomous mode."""
    from connect4_amd.config import MCTSConfig
    from connect4_amd.fused_net import FusedNet
    from connect4_amd.selfplay import SelfPlay
    filters, n_res, prec = kind.split("-")
    filters, n_res = int(filters[:-1]), int(n_res)
    net = FusedNet(M.grid_net(filters, n_res), precision=prec)
    if kind == "32f-16-f16":
        monkeypatch.setenv("C4_FUSED_SLOTS", "32")
        monkeypatch.setenv("C4_FUSED_PACK", "dense")
    games = {}
    for mode in (("split", "wave") if kind == "32f-16-f16" else ("split",)):
        monkeypatch.setenv("C4_FUSED_MODE", mode)
        sp = SelfPlay(net, 64, MCTSConfig.self_play(24), seed=4, games_target=48, record_capacity_games=64,
                      use_graph=False, fused_loop=True, steps_per_launch=16, eval_cache_log2_entries=22)
        for _ in range(1000):
            sp.run_steps(64)
            if sp.stats()["active_slots"] == 0:
                break
        st = sp.stats()
        recs = sp.engine.drain_games()
        assert len(recs) == 48 and st["bad_evals"] == 0
        games[mode] = sorted((r.game_id, list(r.move[:r.length]), list(r.value[:r.length]), r.result) for r in recs)
        if mode == "split":
            if prec == "f16" and filters == 32:
                assert st["speculative_evals"] > 0
            roots = [(int(r.color0[i]), int(r.color1[i])) for r in recs for i in range(r.length)]
            kids = []
            for a, b in roots:
                brd = oracle.Board.from_bits(a, b)
                for col in range(7):
                    if (brd.valid_mask() >> col) & 1:
                        kid = brd.copy()
                        kid.make_move(col)
                        kids.append(kid.key())
            c0 = np.array([x[0] for x in roots + kids], dtype=np.uint64)
            c1 = np.array([x[1] for x in roots + kids], dtype=np.uint64)
            v, p, found = sp.engine.cache_lookup(c0, c1)
            print("%s: %d games, %d cached positions checked (%d roots)" % (kind, len(recs), int(found.sum()), len(roots)))
            assert found[:len(roots)].mean() > 0.95
            nv, npri = net.evaluate_bits(c0, c1, wave=True)
            assert np.array_equal(v[found], nv[found]) and np.array_equal(p[found], npri[found])
        sp.close()
    if len(games) == 2:
        assert games["split"] == games["wave"]
    net.close()


def test_weights_beyond_fp16_range_fall_back_to_inference_net():
    """make_selfplay_net hands a net that c4_net_create refuses (a folded conv weight beyond +-65504) to the PyTorch-ROCm
    plan, which answers it with finite values and priors."""
    import torch
    from connect4_amd.fused_net import FusedNet, make_selfplay_net
    from connect4_amd.engine import board_planes
    from connect4_amd.net import InferenceNet
    sd = M.grid_net(32, 1)
    sd["body.1.0.conv1.weight"][3, 4, 1, 1] = 1e6
    for prec in ("f32x3", "f16"):
        with pytest.raises(Exception, match="conv_w"):
            FusedNet(sd, precision=prec)
        ev = make_selfplay_net(sd, precision=prec)
        assert isinstance(ev, InferenceNet)
    c0, c1 = M.position_set(64, seed=6)
    v, p = ev(torch.from_numpy(board_planes(c0, c1)).cuda())
    print("InferenceNet fallback vs float64: %.3g" % _err((v.cpu().numpy(), p.cpu().numpy()), M.float64_outputs(sd, c0, c1)))
    assert np.isfinite(v.cpu().numpy()).all() and np.isfinite(p.cpu().numpy()).all()
