"""The device statistics (c4_score_update_dev, connect4_amd/stats.py) on the GPU, against the reference's recorded
figures (tests/golden/stats.npz / stats.json) and against the host classes that tests/test_stats_host.py pins to it.

Exact everywhere a count, a minimum or a maximum is compared, and bit for bit between different ways of feeding the same
rows.  The three sums are float64 on the device and float32 batch means in the reference: they are compared with a float64
recomputation at 1e-10 relative (at most 21,000 float64 terms of a few 2^-53 each, plus the kernel's grid of 2^-36 / 2^-32
per row: 3,000 x 2^-37 = 2.2e-8 absolute at worst on sums of several hundred), and with the reference's own figures at the
recorded float32-vs-float64 gap on top of that.  Where score() and Trainer.evaluate are compared with the host classes on
the forward's own outputs, counts, minimum and maximum are exact and the sums are held to that float64 recomputation:
the host classes add float32 batch means, the device float64 row losses, so those two can not be equal bit for bit."""
import ctypes as C
import os
import pickle
import struct

import numpy as np
import pytest
import torch

from conftest import load_json, load_npz

pytestmark = pytest.mark.gpu

M = 5e-5          # the f32x3 forward's tolerance on the shipped net (tests/test_gpu_fused_net.py)
KEYS = (0.0, 0.5, 1.0)


@pytest.fixture(scope="module")
def fx():
    return load_npz("stats.npz"), load_json("stats.json")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(acc):
    """Every field of a c4_score_acc, floats as bit patterns."""
    return (acc.n, tuple(acc.total), tuple(acc.correct), acc.prior_n, acc.prior_correct, acc.non_finite,
            struct.pack("<3d2f", acc.sum_outputs, acc.value_sq_err_sum, acc.prior_bce_sum, acc.smallest, acc.largest))


def float64_sums(xv, yv, xp=None, yp=None):
    x, y = xv.astype(np.float64), yv.astype(np.float64)
    out = [float(x.sum()), float(((x - y) ** 2).sum()), 0.0]
    if xp is not None and len(xp):
        a, b = xp.astype(np.float64), yp.astype(np.float64)
        with np.errstate(divide="ignore"):
            out[2] = float((-(b * np.maximum(np.log(a), -100.0) + (1.0 - b) * np.maximum(np.log(1.0 - a), -100.0))).sum())
    return out


def host_stats(xv, yv, xp=None, yp=None):
    """The host classes on one batch (the losses play no part in what is compared with them: counts, min, max)."""
    from connect4_amd.stats import CombinedStats, ValueStats
    if xp is None:
        st = ValueStats()
        st.update(xv, yv, 0.0)
        return st, None
    st = CombinedStats()
    st.update(xv, yv, 0.0, xp, yp, 0.0)
    return st.value_stats, st.prior_stats


def accumulate(parts, with_priors=True, pad_to=None):
    """A fresh DeviceStats fed `parts` (tuples of NumPy arrays), each padded with NaN rows to pad_to rows; -> c4_score_acc."""
    from connect4_amd.stats import DeviceStats
    ds = DeviceStats("cuda", with_priors=with_priors)
    for part in parts:
        k = len(part[0])
        if pad_to is not None:
            part = tuple(np.concatenate([a, np.full((pad_to - k,) + a.shape[1:], np.nan, dtype=np.float32)]) for a in part)
        t = [dev(a) for a in part]
        ds.update(t[0], t[1], *(t[2:] if with_priors else ()), valid_rows=k)
    return ds.read_accumulator()


def close(a, b, rel=1e-10):
    return abs(a - b) <= rel * abs(b)


def close_on_grid(a, b, rows, q):
    """For sums of few rows, which may be tiny: 1e-10 relative plus what the kernel's grid of 2^-q per row allows (each
    row's term is rounded to it once: at most 2^-(q+1) off; include/c4_engine.h)."""
    return abs(a - b) <= 1e-10 * abs(b) + rows * 2.0 ** -(q + 1)


def check_exact(acc, xv, yv, xp, yp):
    """Counts, min and max of the accumulator == the host classes on the same rows; sums against float64 (close_on_grid)."""
    from connect4_amd.stats import PriorStats, ValueStats
    hv, hp = host_stats(xv, yv, xp, yp)
    got = ValueStats.from_accumulator(acc)
    assert (got.n, got.total, got.correct, got.smallest, got.largest) == (hv.n, hv.total, hv.correct, hv.smallest, hv.largest)
    assert acc.non_finite == 0
    sums = float64_sums(xv, yv, xp, yp)
    rows = len(xv)
    assert close_on_grid(acc.sum_outputs, sums[0], rows, 36) and close_on_grid(acc.value_sq_err_sum, sums[1], rows, 36), \
        (acc.sum_outputs, acc.value_sq_err_sum, sums)
    if xp is not None:
        gp = PriorStats.from_accumulator(acc)
        assert (gp.n, gp.correct) == (hp.n, hp.correct)
        assert close_on_grid(acc.prior_bce_sum, sums[2], rows, 32), (acc.prior_bce_sum, sums[2])
    else:
        assert acc.prior_n == 0 and acc.prior_correct == 0 and acc.prior_bce_sum == 0.0


def check_reference(acc, ref, with_priors=True):
    """Against the reference's recorded to_dict(): every count, smallest / largest bit-equal, sums at the recorded gap."""
    from connect4_amd.stats import CombinedStats, ValueStats
    st = (CombinedStats if with_priors else ValueStats).from_accumulator(acc)
    got, want, gap, f64 = st.to_dict(), ref["to_dict"], ref["gap"], ref["float64"]
    for k in KEYS:
        assert list(got["correct"][k]) == want["correct"][repr(k)]
    assert got["Accuracy"] == want["Accuracy"] and got["Smallest"] == want["Smallest"] and got["Largest"] == want["Largest"]
    assert close(acc.sum_outputs, f64["sum_outputs"]) and close(acc.value_sq_err_sum, f64["value_sq_err_sum"])
    assert abs(got["Average loss"] - want["Average loss"]) <= gap["value_loss"] + 1e-10 * abs(want["Average loss"])
    assert abs(got["Average"] - want["Average"]) <= gap["average"] + 1e-10 * abs(want["Average"])
    if with_priors:
        assert got["prior Accuracy"] == want["prior Accuracy"]
        assert close(acc.prior_bce_sum, f64["prior_bce_sum"])
        assert abs(got["prior Average loss"] - want["prior Average loss"]) <= gap["prior_loss"] + 1e-10 * abs(want["prior Average loss"])
    return st


# -- 1. the kernel alone on the reference's outputs ----------------------------------------------------------------------
def test_kernel_on_the_reference_outputs(fx):
    z, meta = fx
    n_all = (z["N_xv"], z["N_values"], z["N_xp"], z["N_priors"])
    st = check_reference(accumulate([n_all]), meta["N"]["evaluate"])
    assert repr(st).split("\n")[1] == meta["N"]["evaluate"]["repr"].split("\n")[1]       # the counts line, as text
    check_reference(accumulate([(z["N_vo_xv"], z["N_values"])], with_priors=False), meta["N"]["evaluate_value_only"], False)
    e_all = (z["E_xv"], z["E_yv"], z["E_xp"], z["E_yp"])
    acc = accumulate([e_all])
    check_reference(acc, meta["E"])
    assert acc.n == 64 and sum(acc.total) == 63 and acc.largest == 1.0 and acc.smallest == 0.0


# -- 2. shapes and splits ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 257, 3000])
def test_shapes_and_valid_rows(fx, rows):
    from connect4_amd.stats import DeviceStats
    z, _ = fx
    arrays = [z[k][:rows] for k in ("N_xv", "N_values", "N_xp", "N_priors")]
    t = [dev(a) for a in arrays]
    for valid in sorted({rows, rows - 1, 1}):
        ds = DeviceStats("cuda")
        ds.update(*t, valid_rows=valid)
        acc = ds.read_accumulator()
        if valid == 0:
            assert bits(acc) == bits(DeviceStats("cuda").read_accumulator()) and acc.n == 0
            continue
        check_exact(acc, *[a[:valid] for a in arrays])
        dv = DeviceStats("cuda", with_priors=False)
        dv.update(t[0], t[1], valid_rows=valid)
        check_exact(dv.read_accumulator(), arrays[0][:valid], arrays[1][:valid], None, None)


def test_splits_paddings_and_grids_give_the_same_bits(fx):
    z, meta = fx
    xv, yv, xp, yp = z["N_xv"], z["N_values"], z["N_xp"], z["N_priors"]
    cut = lambda idx: (xv[idx], yv[idx], xp[idx], yp[idx])  # noqa: E731
    bs, perm = meta["N"]["batch_size"], z["N_perm"]
    one = accumulate([(xv, yv, xp, yp)])
    ways = {
        "the reference's 256-row batches": accumulate([cut(perm[i:i + bs]) for i in range(0, 3000, bs)]),
        "1 + 2,999": accumulate([cut(slice(0, 1)), cut(slice(1, 3000))]),
        "padded to 3,001 rows": accumulate([(xv, yv, xp, yp)], pad_to=3001),
        "padded to 70,000 rows (the largest grid)": accumulate([(xv, yv, xp, yp)], pad_to=70000),
        "reversed": accumulate([cut(slice(None, None, -1))]),
    }
    for name, acc in ways.items():
        assert bits(acc) == bits(one), name
    assert one.non_finite == 0 and one.n == one.prior_n == 3000
    # the value-only form is the value half of the combined form
    vo = accumulate([(xv, yv)], with_priors=False)
    assert (vo.n, tuple(vo.total), tuple(vo.correct), vo.non_finite) == (one.n, tuple(one.total), tuple(one.correct), 0)
    assert struct.pack("<2d2f", vo.sum_outputs, vo.value_sq_err_sum, vo.smallest, vo.largest) == \
        struct.pack("<2d2f", one.sum_outputs, one.value_sq_err_sum, one.smallest, one.largest)
    assert (vo.prior_n, vo.prior_correct, vo.prior_bce_sum) == (0, 0, 0.0)


def test_more_rows_than_one_pass_of_the_largest_grid(fx):
    """More than 256 workgroups x 256 rows valid in ONE call: lanes take a second row (the grid-stride loop).  Family N
    22 times over, against the same 66,000 rows fed in chunks of 3,000 and of 4,096: the same bits (the sums stay inside
    the range in which they are exact: 34,012 and 10,697 of 131,072, 253,089 of 2,097,152)."""
    z, _ = fx
    tiled = tuple(np.concatenate([z[k]] * 22) for k in ("N_xv", "N_values", "N_xp", "N_priors"))
    n = len(tiled[0])
    assert n == 66000 > 256 * 256
    one = accumulate([tiled])
    for step in (3000, 4096):
        assert bits(accumulate([tuple(a[i:i + step] for a in tiled) for i in range(0, n, step)])) == bits(one), step
    single = accumulate([tuple(z[k] for k in ("N_xv", "N_values", "N_xp", "N_priors"))])
    assert one.n == n and tuple(one.total) == tuple(22 * t for t in single.total) and tuple(one.correct) == tuple(22 * c for c in single.correct)
    assert one.prior_correct == 22 * single.prior_correct and one.non_finite == 0
    assert (one.sum_outputs, one.value_sq_err_sum, one.prior_bce_sum) == \
        (22 * single.sum_outputs, 22 * single.value_sq_err_sum, 22 * single.prior_bce_sum)      # exact: whole grid units
    assert one.sum_outputs < 131072 and one.value_sq_err_sum < 131072 and one.prior_bce_sum < 2097152


def test_reset_snapshot_and_non_finite_rows(fx):
    from connect4_amd.stats import DeviceStats
    z, _ = fx
    t = [dev(z[k]) for k in ("E_xv", "E_yv", "E_xp", "E_yp")]
    ds = DeviceStats("cuda")
    empty = bits(ds.read_accumulator())
    ds.update(*t)
    snap = ds.snapshot()
    first = bits(ds.read_accumulator())
    ds.update(*t)
    assert bits(ds.read_accumulator(snap)) == first and ds.read_accumulator().n == 128
    ds.reset()
    assert bits(ds.read_accumulator()) == empty
    st = ds.read()
    assert (st.value_stats.smallest, st.value_stats.largest, st.value_stats.n) == (1.0, 0.0, 0)
    bad = t[0].clone()
    bad[3] = float("nan")
    bad[7] = float("inf")
    bad[9] = 3.0e30           # finite, but its terms would not fit the integer sums: counted like the other two
    ds.update(bad, *t[1:])
    acc = ds.read_accumulator()
    assert acc.n == 64 and acc.non_finite == 3
    assert [s.value_stats.n for s in ds.read([snap, snap])] == [64, 64] and ds.read([]) == []


def test_bad_arguments_are_refused(fx):
    from connect4_amd import _lib as L
    from connect4_amd.stats import DeviceStats
    lib = L.load()
    ds = DeviceStats("cuda")
    t = [torch.zeros(8, device="cuda"), torch.zeros(8, device="cuda"), torch.full((8, 7), 0.5, device="cuda"), torch.zeros(8, 7, device="cuda")]
    p = [C.c_void_p(x.data_ptr()) for x in t]
    acc, ws = C.c_void_p(ds._acc.data_ptr()), C.c_void_p(ds._ws.data_ptr())
    before = bits(ds.read_accumulator())
    call = lambda xv, yv, xp, yp, rows, valid, a=acc, w=ws: lib.c4_score_update_dev(0, None, xv, yv, xp, yp, rows, valid, a, w)  # noqa: E731
    assert call(p[0], p[1], p[2], p[3], 0, 0) == L.EINVAL and b"rows" in lib.c4_score_last_error()
    assert call(p[0], p[1], p[2], None, 8, 8) == L.EINVAL and call(p[0], p[1], None, p[3], 8, 8) == L.EINVAL
    assert call(p[0], p[1], p[2], p[3], 8, 9) == L.EINVAL and call(p[0], p[1], p[2], p[3], 8, -1) == L.EINVAL
    assert call(None, p[1], p[2], p[3], 8, 8) == L.EINVAL and call(p[0], p[1], p[2], p[3], 8, 8, a=None) == L.EINVAL
    assert call(p[0], p[1], p[2], p[3], 8, 8, w=None) == L.EINVAL
    assert lib.c4_score_workspace_bytes(0) == L.EINVAL and lib.c4_score_reset_dev(0, None, None) == L.EINVAL
    assert 0 < lib.c4_score_workspace_bytes(1) <= lib.c4_score_workspace_bytes(3000) <= lib.c4_score_workspace_bytes(1 << 40) == ds._ws.numel()
    assert call(p[0], p[1], p[2], p[3], 8, 0) == L.OK          # nothing valid: nothing added
    torch.cuda.synchronize()
    assert bits(ds.read_accumulator()) == before
    with pytest.raises(ValueError):
        ds.update(t[0], t[1])
    with pytest.raises(ValueError):
        ds.update(t[0].double(), t[1], t[2], t[3])
    with pytest.raises(RuntimeError):
        DeviceStats("cpu")


# -- 3. end to end -------------------------------------------------------------------------------------------------------
def shipped_state_dict():
    z = load_npz("net_golden.npz")
    return {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w__")}


def categories(v):
    return np.floor(v.astype(np.float32) * np.float32(3.0)) / np.float32(2.0)


def check_near_reference(st, ref, z, mask, what, xv, xp=None, order=None):
    """Another forward of the same net (outputs xv, xp, given in row order `order` of the fixture).  Row by row: off the
    fixture's near-boundary mask the category -- and the predicted move -- is the reference's.  So every count lies within
    the masked rows OF THAT CATEGORY of the reference's, the policy count within the near-ties; losses within gap + 7 M."""
    rows_xv = np.empty_like(xv)
    order = np.arange(len(xv)) if order is None else order
    rows_xv[order] = xv
    assert np.array_equal(categories(rows_xv)[~mask], categories(z["N_xv"])[~mask]), what
    got, want, gap = st.to_dict(), ref["to_dict"], ref["gap"]
    for k in KEYS:
        total, correct = got["correct"][k]
        rt, rc = want["correct"][repr(k)]
        masked = int((mask & (z["N_values"] == np.float32(k))).sum())
        print("%s: category %s: %d of %d correct, the reference %d of %d (masked rows of the category: %d)" % (what, k, correct, total, rc, rt, masked))
        assert total == rt and abs(correct - rc) <= masked
    for key, g in (("Average loss", "value_loss"), ("prior Average loss", "prior_loss"), ("Average", "average")):
        if key in got:
            print("%s: %s %.9g, the reference %.9g, difference %.3g (bound %.3g)" %
                  (what, key, got[key], want[key], abs(got[key] - want[key]), gap[g] + 7 * M))
            assert abs(got[key] - want[key]) <= gap[g] + 7 * M
    if xp is not None:
        rows_xp = np.empty_like(xp)
        rows_xp[order] = xp
        assert np.array_equal(np.argmax(rows_xp, axis=1)[~mask], np.argmax(z["N_xp"], axis=1)[~mask]), what
        top = np.sort(z["N_xp"].astype(np.float64), axis=1)
        near_ties = int(((top[:, -1] - top[:, -2]) <= 2 * M).sum())
        moved = abs(st.prior_stats.correct - round(want["prior Accuracy"] * 3000))
        print("%s: %d policy rows counted differently (near-ties: %d)" % (what, moved, near_ties))
        assert moved <= near_ties


def test_score_and_trainer_evaluate_on_the_shipped_net(fx):
    from connect4_amd.fused_net import FusedNet
    from connect4_amd.net import InferenceNet, PolicyValueNet
    from connect4_amd.stats import CombinedStats, LabelledSet, ValueStats, score
    from connect4_amd.training import ModelConfig, Trainer, dataloader_permutation
    z, meta = fx
    sd = shipped_state_dict()
    ls = LabelledSet(dev(z["N_boards"]), dev(z["N_values"]), dev(z["N_priors"]))
    ref, mask = meta["N"]["evaluate"], z["N_mask"]
    assert int(mask.sum()) == meta["N"]["mask_rows"]

    def same_as_host(st, xv, xp, yv, yp, what):      # noqa: E306
        """== the host classes on the forward's own outputs: counts, min and max exactly.  The sums cannot be equal to the
        host classes': those add float32 batch means times the batch length (stats.py:56, 101), the device adds float64 row
        losses, as the accumulator is specified; they are held to float64 sums of the same outputs at 1e-10 instead."""
        hv, hp = host_stats(xv, yv, xp, yp)
        v = st.value_stats if isinstance(st, CombinedStats) else st
        assert (v.n, v.total, v.correct, v.smallest, v.largest, v.non_finite) == (hv.n, hv.total, hv.correct, hv.smallest, hv.largest, 0), what
        sums = float64_sums(xv, yv, xp, yp)
        assert close(float(v.average_value), sums[0]) and close(float(v.total_loss), sums[1]), what
        if xp is not None:
            assert (st.prior_stats.n, st.prior_stats.correct) == (hp.n, hp.correct), what
            assert close(7.0 * st.prior_stats.total_loss, sums[2]), what

    class Fused:
        """The FusedNet as score() drives it, keeping the tensors it filled."""
        from_bitboards = True

        def __init__(self, net):
            self.net, self.seen = net, []

        def forward_bitboards(self, c0, c1, n, values, priors):
            self.net.forward_bitboards(c0, c1, n, values, priors)
            self.seen.append((values, priors))

    class Planes:
        def __init__(self, net):
            self.net, self.seen = net, []

        def __call__(self, planes):
            self.seen.append(self.net(planes))
            return self.seen[-1]

    def outputs(seen):
        return np.concatenate([v.cpu().numpy() for v, _ in seen]), np.concatenate([p.cpu().numpy() for _, p in seen])

    # score(): the fused forward in its default precision on the packed boards, 16 B per position
    net = FusedNet(sd)
    assert net.precision == "f32x3"
    rec = Fused(net)
    st = score(rec, ls, batch_size=2048)
    assert len(rec.seen) == 2
    xv, xp = outputs(rec.seen)
    same_as_host(st, xv, xp, z["N_values"], z["N_priors"], "score(FusedNet)")
    check_near_reference(st, ref, z, mask, "score(FusedNet)", xv, xp)
    vo = score(net, LabelledSet(ls.boards, ls.values), batch_size=2048)
    assert isinstance(vo, ValueStats) and vo.to_dict() == st.value_stats.to_dict()
    net.close()
    # ... and an evaluator that is fed planes
    rec = Planes(InferenceNet(sd, device="cuda"))
    st = score(rec, ls)
    xv, xp = outputs(rec.seen)
    same_as_host(st, xv, xp, z["N_values"], z["N_priors"], "score(InferenceNet)")
    check_near_reference(st, ref, z, mask, "score(InferenceNet)", xv, xp)

    # Trainer.evaluate: the trainer's own net, the reference's batches
    tr = Trainer(ModelConfig(net_config=PolicyValueNet.config_from_state_dict(sd)), device="cuda")
    tr.net.load_state_dict(sd)
    seen = []
    hook = tr.net.register_forward_hook(lambda m, i, o: seen.append((o[0].detach().cpu().numpy(), o[1].detach().cpu().numpy())))
    torch.manual_seed(0)
    st = tr.evaluate(ls, batch_size=meta["N"]["batch_size"])
    torch.manual_seed(0)
    vo = tr.evaluate_value_only((ls.planes(), ls.values))
    hook.remove()
    torch.manual_seed(0)
    perm = dataloader_permutation(3000).numpy()
    assert np.array_equal(perm, z["N_perm"]) and len(seen) == 12 + 1 and not tr.net.training
    xv, xp = np.concatenate([s[0] for s in seen[:12]]), np.concatenate([s[1] for s in seen[:12]])
    same_as_host(st, xv, xp, z["N_values"][perm], z["N_priors"][perm], "Trainer.evaluate")
    check_near_reference(st, ref, z, mask, "Trainer.evaluate", xv, xp, perm)
    same_as_host(vo, seen[12][0], None, z["N_values"][perm], None, "Trainer.evaluate_value_only")
    check_near_reference(vo, meta["N"]["evaluate_value_only"], z, z["N_vo_mask"], "Trainer.evaluate_value_only", seen[12][0], None, perm)


def test_labelled_set_round_trips_planes(fx, tmp_path):
    from connect4_amd.engine import board_planes
    from connect4_amd.stats import LabelledSet
    z, _ = fx
    u = z["N_boards"].view(np.uint64)[:300]
    planes = torch.from_numpy(np.asarray(board_planes(u[:, 0], u[:, 1]), dtype=np.float32).reshape(-1, 3, 6, 7))
    path = os.path.join(str(tmp_path), "set.pth")
    torch.save({"boards": planes, "values": torch.from_numpy(z["N_values"][:300]), "priors": torch.from_numpy(z["N_priors"][:300])}, path)
    ls = LabelledSet.load(path, device="cuda")
    assert torch.equal(ls.boards.cpu(), torch.from_numpy(z["N_boards"][:300])) and torch.equal(ls.planes().cpu(), planes)
    assert torch.equal(ls.priors.cpu(), torch.from_numpy(z["N_priors"][:300])) and len(ls) == 300
    broken = planes.clone()
    broken[5, 1] = broken[5, 2] = 1.0
    with pytest.raises(ValueError):
        LabelledSet.from_tensors(broken, torch.zeros(300))


# -- 4. training ---------------------------------------------------------------------------------------------------------
def training_data():
    g = torch.Generator().manual_seed(11)
    n = 64 * 6 + 17
    boards = (torch.rand(n, 3, 6, 7, generator=g) < 0.3).float()
    values = torch.randint(0, 3, (n,), generator=g).float() / 2
    priors = torch.zeros(n, 7)
    priors[torch.arange(n), torch.randint(0, 7, (n,), generator=g)] = 1.0
    return n, boards, values, priors


def test_train_stats_eager_is_the_host_classes_on_the_steps_outputs():
    from connect4_amd.stats import DeviceStats
    from connect4_amd.training import ModelConfig, Trainer, dataloader_permutation
    n, boards, values, priors = training_data()
    torch.manual_seed(2)
    tr = Trainer(ModelConfig(batch_size=64, n_training_epochs=2), device="cuda", use_graph=False)
    assert tr.pad_ragged_batches
    seen = []
    hook = tr.net.register_forward_hook(lambda m, i, o: seen.append((o[0].detach().clone(), o[1].detach().clone())))
    calls = DeviceStats.calls
    tr.train(boards, values, priors, generator=torch.Generator().manual_seed(7), stats=True)
    hook.remove()
    assert DeviceStats.calls - calls == 2 * 7 == len(seen) and len(tr.epoch_stats) == 2
    g = torch.Generator().manual_seed(7)
    step = 0
    for st in tr.epoch_stats:
        perm = dataloader_permutation(n, g)
        xv, xp = [], []
        for i in range(0, n, 64):
            k = len(perm[i:i + 64])
            assert tuple(seen[step][0].shape) == (64,)          # the ragged batch was padded: 47 rows that must not count
            xv.append(seen[step][0][:k].cpu().numpy())
            xp.append(seen[step][1][:k].cpu().numpy())
            step += 1
        xv, xp, yv, yp = np.concatenate(xv), np.concatenate(xp), values[perm].numpy(), priors[perm].numpy()
        hv, hp = host_stats(xv, yv, xp, yp)
        v = st.value_stats
        assert v.n == st.prior_stats.n == 401 and v.non_finite == 0
        assert (v.total, v.correct, v.smallest, v.largest) == (hv.total, hv.correct, hv.smallest, hv.largest)
        assert st.prior_stats.correct == hp.correct
        sums = float64_sums(xv, yv, xp, yp)
        assert close(float(v.average_value), sums[0]) and close(float(v.total_loss), sums[1]) and close(7.0 * st.prior_stats.total_loss, sums[2])


def test_train_stats_in_the_captured_step_and_off_by_default():
    from connect4_amd.stats import DeviceStats
    from connect4_amd.training import ModelConfig, Trainer
    n, boards, values, priors = training_data()
    torch.manual_seed(2)
    tr = Trainer(ModelConfig(batch_size=64, n_training_epochs=2), device="cuda")
    assert tr.use_graph
    calls = DeviceStats.calls
    loss = tr.train(boards, values, priors, generator=torch.Generator().manual_seed(7), stats=True)
    # two eager full steps and the capture launch the update from Python; the replays launch it from the graph
    assert 0 < DeviceStats.calls - calls < 2 * 7 and np.isfinite(loss) and len(tr.epoch_stats) == 2
    hist = {k: int((values == k).sum()) for k in KEYS}
    for st in tr.epoch_stats:
        v = st.value_stats
        assert v.n == st.prior_stats.n == 401 and v.total == hist and v.non_finite == 0
        assert all(0 <= v.correct[k] <= v.total[k] for k in KEYS) and 0 <= st.prior_stats.correct <= 401
        assert np.isfinite([st.loss, v.loss, v.average, v.smallest, v.largest, st.prior_stats.loss]).all()
        assert v.smallest <= v.average <= v.largest
        assert st.to_dict().keys() == {"prior Average loss", "prior Accuracy", "Average loss", "Accuracy", "Smallest", "Largest", "Average", "correct"}
    # stats=False: the parent's step, nothing launched, nothing kept
    calls = DeviceStats.calls
    tr.train(boards, values, priors, generator=torch.Generator().manual_seed(7))
    assert DeviceStats.calls == calls and tr.epoch_stats == []


# -- 5. one toy generation -----------------------------------------------------------------------------------------------
def test_run_generations_scores_its_test_sets(fx, tmp_path):
    from connect4_amd.config import MCTSConfig
    from connect4_amd.generation import run_generations
    from connect4_amd.stats import LabelledSet
    from connect4_amd.training import ModelConfig, Trainer
    z, meta = fx
    d = str(tmp_path)
    ls = LabelledSet(dev(z["N_boards"]), dev(z["N_values"]), dev(z["N_priors"]))
    torch.manual_seed(0)
    tr = Trainer(ModelConfig(batch_size=256, n_training_epochs=2, use_gpu=True))
    timings = []
    run_generations(tr, MCTSConfig.self_play(16), 16, d, 2, first_gen=1, n_slots=16, timings=timings,
                    test_sets={"t": ls, "v": LabelledSet(ls.boards, ls.values)}, train_stats=True)
    keys = set(meta["N"]["evaluate"]["to_dict"])
    for name, want in (("t", keys), ("v", set(meta["N"]["evaluate_value_only"]["to_dict"]))):
        with open(os.path.join(d, name + ".pkl"), "rb") as f:
            hist = pickle.load(f)
        assert [e["generation"] for e in hist] == [1, 2]
        for e, t in zip(hist, timings):
            assert set(e) == want | {"generation"} and sum(tc[0] for tc in e["correct"].values()) == 3000
            assert {k: v for k, v in e.items() if k != "generation"} == t[name]
    assert all(len(t["train_stats"]) == 2 and t["train_stats"][0]["correct"] for t in timings)
