"""Host checks for the 64-filter reference-precision forward ("f32x3w"; tests/test_gpu_net64_precise.py runs it):
  * tests/golden/net64_parity.json / net64_parity_tables.npz (written by tests/golden/gen_net64_parity_golden.py from the
    unmodified reference with a stressed 64/6/6 net) have the shape the GPU tests rely on: the weights are the ones
    stressed_state_dict generates, eps is tol_f32x3(6), half of each family is decided, the tables hold both kinds;
  * the split arithmetic itself (net_models_wide.f32x3_split_outputs: hi + lo / 2^11 in fp16 wherever the kernel stores,
    float32 sums) lies within tol_f32x3(R) of float64 on the grid's 64-filter nets, and so does the float32 module, the
    reference's own precision -- so the bound the kernel is held to is one the reference itself clears.
    Measured on the grid's 1,023 positions (split model / float32 module / bound): 0 blocks 2.9e-7 / 1.2e-6 / 1.14e-5;
    1 block 2.7e-6 / 2.3e-6 / 1.91e-5; 7 blocks 2.5e-6 / 2.9e-6 / 6.48e-5; the fixture's 64/6/6 net 1.0e-6 / 4.9e-6 / 5.72e-5;
  * the ABI: C4_NET_F32X3_WIDE in the header, in _lib and behind FusedNet.PRECISIONS["f32x3w"]."""
import hashlib
import re

import numpy as np
import pytest

import net_models as M
import net_models_wide as W
from conftest import load_json, load_npz, table_from_npz


@pytest.fixture(scope="module")
def fixture():
    return load_json("net64_parity.json")


@pytest.fixture(scope="module")
def tables():
    return load_npz("net64_parity_tables.npz")


def fixture_state_dict(fixture):
    from connect4_amd.net import NetConfig
    n = fixture["net"]
    return M.stressed_state_dict(NetConfig(filters=n["filters"], n_residuals=n["n_residuals"], n_fc_layers=n["n_fc_layers"]), seed=n["seed"])


def _err(a, b):
    return max(float(np.abs(a[0] - b[0]).max()), float(np.abs(a[1] - b[1]).max()))


def test_fixture_integrity(fixture, tables):
    from connect4_amd.board import Board
    assert fixture["net"] == dict(filters=64, n_residuals=6, n_fc_layers=6, seed=26)
    sd = fixture_state_dict(fixture)
    h = hashlib.sha256()
    for k in sorted(sd):
        if not k.endswith("num_batches_tracked"):
            h.update(np.ascontiguousarray(sd[k].numpy().astype(np.float32)).tobytes())
    assert h.hexdigest() == fixture["weights_sha256"]
    assert fixture["eps"] == M.tol_f32x3(6) == 16 * 15 * 2.0 ** -22 and fixture["K"] == 6
    cases = fixture["cases"]
    assert len({c["name"] for c in cases}) == len(cases)
    a = [c for c in cases if c["family"] == "A"]
    b = [c for c in cases if c["family"] == "B"]
    assert len(a) == 24 and len(a) + len(b) == len(cases) and len(fixture["games"]) == 1
    assert len({(c["board"]["c0"], c["board"]["c1"]) for c in a}) == 24
    ages = sorted(c["board"]["age"] for c in a)
    assert ages[0] == 0 and ages[-1] == 33 and max(y - x for x, y in zip(ages, ages[1:])) <= 2      # spread over 0..33
    for c in cases:
        assert c["config"]["simulations"] == 800 and c["root_N"] == 801 and sum(c["N"]) == 800
        assert c["board"]["result"] is None
        assert isinstance(c["decided"], bool) and c["decided"] == (c["self_tv"] == 0.0)
        bd = Board.from_bits(c["board"]["c0"], c["board"]["c1"])
        assert bd.age == c["board"]["age"] and sorted(bd.valid_moves) == c["board"]["valid"]
    for c in a:
        assert c["noise"] is None and c["uniform"] is None and c["move"] == c["best_move"]
    g = fixture["games"][0]
    assert g["seed"] == 0 and [c["ply"] for c in b] == list(range(len(g["moves"]))) and [c["move"] for c in b] == g["moves"]
    bd = Board()
    for c in b:
        assert (int(bd.color[0]), int(bd.color[1]), bd.age) == (c["board"]["c0"], c["board"]["c1"], c["ply"])
        cfg = c["config"]
        assert (cfg["root_dirichlet_alpha"], cfg["root_exploration_fraction"], cfg["num_sampling_moves"]) == (0.3, 0.25, 6)
        assert len(c["noise"]) == 7 and (c["uniform"] is not None) == (c["ply"] < 6)
        bd.make_move(c["move"])
    assert bd.result is not None and bd.result.value == g["result"]
    for fam in ("A", "B"):
        share = float(np.mean([c["decided"] for c in cases if c["family"] == fam]))
        assert share == fixture["decided_share"][fam] and share >= 0.5
    # tables: whole tables of the first eight A cases and of every fourth ply (thinned from the end only), both kinds among them
    want = [c["name"] for c in a[:8]] + [c["name"] for c in b if c["ply"] % 4 == 0]
    kept = fixture["table_cases"]
    assert kept == want[:len(kept)] and len(kept) >= 8
    assert sorted({k.rsplit("__", 1)[0] for k in tables.files}) == sorted(kept)
    by_name = {c["name"]: c for c in cases}
    assert any(by_name[n]["decided"] for n in kept) and any(not by_name[n]["decided"] for n in kept)
    for n in kept:
        c0, c1, v, p = table_from_npz(tables, n)
        assert 0 < len(c0) == len(c1) == len(v) == len(p) and v.dtype == np.float32 and p.dtype == np.float32      # each distinct position once
        assert len(set(zip(c0.tolist(), c1.tolist()))) == len(c0)
        assert (by_name[n]["board"]["c0"], by_name[n]["board"]["c1"]) in set(zip(c0.tolist(), c1.tolist()))


@pytest.fixture(scope="module")
def positions():
    c0, c1 = M.grid_positions()
    return c0, c1, M.planes_of(c0, c1)


@pytest.mark.parametrize("n_res", [0, 1, 7])
def test_split_arithmetic_and_float32_clear_the_bound(positions, n_res):
    c0, c1, planes = positions
    sd = M.grid_net(64, n_res)
    ref = M.float64_outputs(sd, c0, c1, planes)
    es = _err(W.split_model_outputs(sd, c0, c1, planes), ref)
    e32 = _err(W.float32_module_outputs(sd, c0, c1, planes), ref)
    print("grid_net(64, %d): split model %.3g, float32 module %.3g, bound %.3g" % (n_res, es, e32, M.tol_f32x3(n_res)))
    assert es <= M.tol_f32x3(n_res) and e32 <= M.tol_f32x3(n_res)


def test_fixture_net_clears_the_bound(fixture, tables):
    """... and on the fixture's net, over the positions the reference's searches reached: the split model, the float32
    module and the reference's recorded float32 answers all lie within tol_f32x3(6) of float64."""
    sd = fixture_state_dict(fixture)
    pos = {}
    for name in fixture["table_cases"]:
        for a, b, v, p in zip(*table_from_npz(tables, name)):
            pos[(int(a), int(b))] = (v, p)
    keys = sorted(pos)[::4]
    c0 = np.array([k[0] for k in keys], dtype=np.uint64)
    c1 = np.array([k[1] for k in keys], dtype=np.uint64)
    planes = M.planes_of(c0, c1)
    ref = M.float64_outputs(sd, c0, c1, planes)
    rec = (np.array([pos[k][0] for k in keys], dtype=np.float64), np.stack([pos[k][1] for k in keys]).astype(np.float64))
    es, e32, er = _err(W.split_model_outputs(sd, c0, c1, planes), ref), _err(W.float32_module_outputs(sd, c0, c1, planes), ref), _err(rec, ref)
    print("fixture net, %d positions: split model %.3g, float32 module %.3g, recorded reference %.3g, bound %.3g" %
          (len(keys), es, e32, er, M.tol_f32x3(6)))
    assert max(es, e32, er) <= M.tol_f32x3(6)


def test_split_rounding_is_the_kernels():
    """split_round keeps ~22 bits: |x - (hi + lo / 2^11)| <= 2^-22 |x| for normal fp16 magnitudes, and a value that is
    exact in fp16 has no low part."""
    import torch
    x = torch.from_numpy(np.random.RandomState(0).normal(0.0, 3.0, 4096)).double()
    x32 = x.float().double()
    r = W.split_round(x)
    assert float(((r - x32).abs() / x32.abs()).max()) <= 2.0 ** -22
    e = torch.tensor([0.0, 1.0, -0.5, 1024.0], dtype=torch.float64)
    assert torch.equal(W.split_round(e), e)


def test_abi_names_the_wide_precision():
    from connect4_amd import _lib as L
    from connect4_amd.fused_net import FusedNet
    with open(L.HEADER_PATH) as f:
        header = f.read()
    m = re.search(r"^#define\s+C4_NET_F32X3_WIDE\s+(\d+)", header, re.M)
    assert m, "include/c4_engine.h does not define C4_NET_F32X3_WIDE"
    assert int(m.group(1)) == L.NET_F32X3_WIDE == FusedNet.PRECISIONS["f32x3w"] == 2
    assert FusedNet.PRECISIONS["f16"] == L.NET_F16 == 0 and FusedNet.PRECISIONS["f32x3"] == L.NET_F32X3 == 1
    assert FusedNet.reference_precision(32) == "f32x3" and FusedNet.reference_precision(64) == "f32x3w"
    assert FusedNet.default_precision(32) == "f32x3" and FusedNet.default_precision(64) == "f16"
