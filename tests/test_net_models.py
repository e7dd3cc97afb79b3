"""The float64 models the GPU net tests compare against (tests/net_models.py), checked on the host:
  * float64_outputs is the reference's net (its outputs on example_net.pth, tests/golden/net_golden.npz);
  * fold_for_fused -- what FusedNet hands to the kernels -- computes that same net, for every configuration of the grid;
  * the stressed nets are not degenerate: their answers vary from position to position by far more than any GPU
    tolerance (today's random-init nets are printed next to them);
  * every modelled host or kernel mistake listed below moves the float64 outputs by at least 10x the tolerance each
    precision's GPU test applies to that configuration, so the GPU tests would see it.
All of it on the nets and positions the GPU tests run (net_models.grid_net, grid_positions)."""
import numpy as np
import pytest
import torch

import net_models as M
from conftest import load_npz

F16_VS_F64 = 2e-2    # the existing fp16 tolerance against the reference (test_gpu_fused_net.py)


@pytest.fixture(scope="module")
def positions():
    c0, c1 = M.grid_positions()
    return c0, c1, M.planes_of(c0, c1)


def test_position_sets():
    from connect4_amd.board import Board
    c0, c1 = M.seeded_positions(168, seed=3)
    plies = [bin(int(a)).count("1") + bin(int(b)).count("1") for a, b in zip(c0, c1)]
    assert sorted(set(plies)) == list(range(42))
    for a, b in zip(c0, c1):
        assert Board.from_bits(int(a), int(b)).result is None and not int(a) & int(b)
    e0, e1 = M.edge_positions()
    assert e0[0] == 0 and e1[0] == 0
    full_cols = [sum(((int(a) | int(b)) >> (7 * c)) & 0x3F == 0x3F for c in range(7)) for a, b in zip(e0, e1)]
    assert set(full_cols) == set(range(8))     # the empty board ... full boards (a stone in every column's top row)
    assert sum(f == 7 for f in full_cols) >= 4


def test_float64_model_matches_reference_golden():
    z = load_npz("net_golden.npz")
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w__")}
    assert np.array_equal(M.planes_of(z["in_c0"], z["in_c1"]), z["in_planes"])
    v, p = M.float64_outputs(sd, z["in_c0"], z["in_c1"])
    print("float64 model vs reference golden: max |dv| %.2e  max |dp| %.2e" %
          (np.abs(v - z["out_values"]).max(), np.abs(p - z["out_priors"]).max()))
    np.testing.assert_allclose(v, z["out_values"], atol=1e-5, rtol=0)
    np.testing.assert_allclose(p, z["out_priors"], atol=1e-5, rtol=0)


@pytest.mark.parametrize("filters,n_res,n_fc,prec", M.GRID)
def test_fold_for_fused_is_the_net(positions, filters, n_res, n_fc, prec):
    """A float64 evaluation of the fold_for_fused arrays (desc_outputs, written from include/c4_engine.h's layout) equals
    float64_outputs: BN folding, head order, the Linear collapse (also for 0 and 6 layers), vout / w1 / w2 plumbing.  The
    float32 arrays FusedNet hands over are the float64 fold rounded once."""
    from connect4_amd.fused_net import fold_for_fused
    c0, c1, planes = positions
    sd = M.grid_net(filters, n_res)
    a64 = fold_for_fused(sd, np.float64)
    v, p = M.float64_outputs(sd, c0, c1, planes)
    fv, fp = M.desc_outputs(a64, planes)
    print("%df/%dres/%dfc: fold vs float64 net: %.2e" % (filters, n_res, n_fc, max(np.abs(fv - v).max(), np.abs(fp - p).max())))
    assert np.abs(fv - v).max() <= 1e-10 and np.abs(fp - p).max() <= 1e-10
    a32 = fold_for_fused(sd)
    for k, a in a64.items():
        if isinstance(a, np.ndarray):
            assert a32[k].dtype == np.float32 and a32[k].flags.c_contiguous and np.array_equal(a32[k], a.astype(np.float32))
        else:
            assert a32[k] == a


def test_stressed_nets_are_not_degenerate(positions):
    """Spread of values and priors over the position set, stressed nets next to today's random-init nets: the largest
    deviation from the mean is at least 20x every GPU tolerance of the configuration (the existing 2e-2 included)."""
    from connect4_amd.fused_net import fold_for_fused
    from connect4_amd.net import NetConfig, random_init_state_dict
    c0, c1, planes = positions
    for filters, n_res, n_fc, prec in M.GRID:
        sd = M.grid_net(filters, n_res)
        tols = [F16_VS_F64] + ([M.tol_f32x3(n_res)] if "f32x3" in prec else []) + list(M.f16_tolerances(fold_for_fused(sd), planes))
        rinit = random_init_state_dict(NetConfig(filters=filters, n_residuals=n_res, n_fc_layers=n_fc), seed=20 + n_res)
        for name, net in (("stressed", sd), ("random-init", rinit)):
            v, p = M.float64_outputs(net, c0, c1, planes)
            sv, sp = v.std(), p.std(0).mean()
            dv, dp = np.abs(v - v.mean()).max(), np.abs(p - p.mean(0)).max()
            print("%df/%2dres/%dfc %-11s std(values) %.4f  mean std(priors) %.4f  max|v - mean| %.4f  max|p - mean| %.4f  "
                  "(20x tolerance %.3g)" % (filters, n_res, n_fc, name, sv, sp, dv, dp, 20 * max(tols)))
            if name == "stressed":
                assert sv >= 0.1 and sp >= 0.05
                assert dv >= 20 * max(tols) and dp >= 20 * max(tols)


@torch.no_grad()
def _mutations(sd, a, n_res, planes):
    """(name, mutated folded arrays) of each modelled mistake.  The tower bias is the one of the last layer's channel
    the heads listen to most: largest |head weights| x the fraction of (position, pixel) where the channel is positive
    (a channel that LeakyReLU holds at 0.01x for most inputs barely reaches the heads)."""
    import copy
    x = M._module(sd).body(torch.from_numpy(planes))
    live = (x > 0).double().mean((0, 2, 3)).numpy()
    ch = int((np.abs(a["head_w"]).sum(0) * live).argmax())
    out = []
    b = copy.deepcopy(a)
    if n_res:
        b["conv_b"][-1, ch] += 0.05      # one bias of the tower's last layer
    else:
        b["stem_b"][ch] += 0.05
    out.append(("last-layer bias +0.05", b))
    b = copy.deepcopy(a)
    b["head_w"][[1, 2]] = b["head_w"][[2, 1]]
    b["head_b"][[1, 2]] = b["head_b"][[2, 1]]
    out.append(("policy channels swapped", b))
    b = copy.deepcopy(a)
    b["w2"] = a["w2"] + 0.03
    out.append(("w2 + 0.03", b))
    b = copy.deepcopy(a)
    b["vfc_w"] = np.roll(a["vfc_w"], 1, axis=0)
    b["vfc_b"] = np.roll(a["vfc_b"], 1)
    out.append(("collapsed fc rows off by one", b))
    return out


@pytest.mark.parametrize("filters,n_res,n_fc,prec", M.GRID)
def test_gpu_tolerances_see_modelled_mistakes(positions, filters, n_res, n_fc, prec):
    """Each mistake moves the float64 outputs by at least 10x what each precision's GPU test tolerates.  f32x3: the
    largest move >= 10 x tol_f32x3.  f16 (the test there bounds the max AND the mean of the per-position error): the
    mean move >= 10x the mean tolerance.  The max tolerance of the deep fp16 nets is dominated by a few positions whose
    flipped fp16 roundings add up; against it the smallest mistake (one bias + 0.05) moves the outputs by less than 10x
    (the margins are printed), and it is the mean bound that holds every mistake to 10x."""
    from connect4_amd.fused_net import fold_for_fused
    c0, c1, planes = positions
    sd = M.grid_net(filters, n_res)
    a = fold_for_fused(sd, np.float64)
    base = M.desc_outputs(a, planes)
    moved = [(name, M.desc_outputs(b, planes)) for name, b in _mutations(sd, a, n_res, planes)]
    if n_res:
        cut = {k: t for k, t in sd.items() if not k.startswith("body.1.%d." % (n_res - 1))}
        moved.append(("last residual block dropped", M.float64_outputs(cut, c0, c1, planes)))
    t16max, t16mean = M.f16_tolerances(fold_for_fused(sd), planes)
    for name, out in moved:
        d = M.per_position_error(out, base)
        line = "%df/%2dres/%dfc %-30s moves the outputs by max %.3g, mean %.3g:" % (filters, n_res, n_fc, name, d.max(), d.mean())
        if "f32x3" in prec:
            line += "  f32x3 %.0fx (max vs %.3g)" % (d.max() / M.tol_f32x3(n_res), M.tol_f32x3(n_res))
            assert d.max() >= 10 * M.tol_f32x3(n_res), name
        if "f16" in prec:
            line += "  f16 %.0fx (mean vs %.3g; max vs %.3g: %.1fx)" % (d.mean() / t16mean, t16mean, t16max, d.max() / t16max)
            assert d.mean() >= 10 * t16mean, name
        print(line)


def _create(arrays, filters, n_res, precision):
    """c4_net_create on hand-made c4_net_desc arrays: (return code, message)."""
    import ctypes as C
    from connect4_amd import _lib as L
    from connect4_amd.fused_net import FusedNet
    d = L.NetDesc()
    d.channels, d.filters, d.n_residuals, d.precision = 3, filters, n_res, FusedNet.PRECISIONS[precision]
    for k, a in arrays.items():
        setattr(d, k, a.ctypes.data_as(C.POINTER(C.c_float)) if isinstance(a, np.ndarray) else a)
    lib, h = L.load(), C.c_void_p()
    rc = lib.c4_net_create(0, C.byref(d), C.byref(h))
    msg = (lib.c4_net_last_error() or b"").decode()
    if rc == L.OK:
        lib.c4_net_destroy(h)
    return rc, msg


def test_fp16_range_check_of_the_folded_weights():
    """c4_net_create refuses a folded 3x3 / 1x1 weight beyond +-65504 (it would become inf in fp16, and NaN times the
    zero padding) with C4_EINVAL, naming the array; +-65504 itself and NaN pass (NaN is contained by the kernels).  It
    checks before it looks for a device, so this runs without one (an accepted net then fails with C4_EDEVICE there)."""
    import __graft_entry__ as g
    from connect4_amd import _lib as L
    from connect4_amd.fused_net import FusedNet, fold_for_fused
    g.build_engine()
    sd = M.grid_net(32, 1)
    a = fold_for_fused(sd)
    for name, v, ok in (("conv_w", 65504.0, True), ("conv_w", -65504.0, True), ("conv_w", 65505.0, False),
                        ("stem_w", -7e4, False), ("head_w", np.inf, False), ("conv_w", np.nan, True)):
        b = dict(a)
        b[name] = a[name].copy()
        b[name].flat[7] = v
        for prec in ("f32x3", "f16"):
            rc, msg = _create(b, 32, 1, prec)
            assert (rc != L.EINVAL) == ok, (name, v, prec, msg)
            if not ok:
                assert name in msg and "fp16" in msg
    for key, name in (("body.0.0.weight", "stem_w"), ("body.1.0.conv2.weight", "conv_w"), ("policy_head.conv1.weight", "head_w")):
        bad = {k: t.clone() for k, t in sd.items()}
        bad[key].view(-1)[5] = 1e6
        for prec in ("f32x3", "f16"):
            with pytest.raises(L.EngineError) as ei:
                FusedNet(bad, precision=prec)
            assert ei.value.code == L.EINVAL and name in str(ei.value) and "fp16" in str(ei.value)
