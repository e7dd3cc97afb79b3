#!/usr/bin/env python3
"""Generate tests/golden/stats.npz and stats.json: the reference's value / policy statistics (oinkoink/neural/stats.py)
as ModelWrapper.evaluate and evaluate_value_only (neural/pytorch/model.py:180-198, 307-342) accumulate them with
data/example_net.pth, and on hand-made edge rows.

Like gen_net_parity_golden.py this imports the UNMODIFIED reference over oracle/refshim and runs in the build container only:

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 \
      PYTHONPATH=<repo>/oracle/refshim:<reference> python <repo>/tests/golden/gen_stats_golden.py

Everything written is data (inputs + expected outputs, no reference source text); a re-run reproduces both files byte for
byte (torch on one thread; fixed zip timestamps).

Family N -- the shipped net.  1,500 distinct seeded undecided positions, ages 0..33, followed by their 1,500 mirrors (the
row order of a data.pth), as bitboards.  Value labels in {0, 0.5, 1}: the category of the net's own output on most rows,
a seeded other one on the rest, so that every category has correct and incorrect members (asserted).  Policy labels over
the legal moves: one-hot rows and multi-hot rows of 2 or 3 tied ones; a mirror carries its original's labels, reversed.
Recorded from ModelWrapper(example_net.pth):
  N_xv, N_xp          its float32 outputs, as the batches of evaluate(batch_size=256) produced them, in row order;
  N_perm              the row order of that pass under torch.manual_seed(0) (batch b = N_perm[256 b : 256 b + 256]; asserted
                      against the boards the net was called with);
  N_vloss, N_ploss    the float32 batch losses handed to CombinedStats.update;
  N_vo_vloss          evaluate_value_only's batch losses (same seed, its own batch size 4096);
  json: to_dict() and repr of both, the float64 recomputations of the three sums from N_xv / N_xp alone, the gaps
  |reference's figure - float64 figure|, and N_mask.
N_mask marks the rows that a change of at most M = 5e-5 in an output could re-categorise (M: the tolerance
tests/test_gpu_fused_net.py holds the f32x3 forward to on this net): |3v - 1| or |3v - 2| <= 3M, or v >= 1 - M (reaching
exactly 1.0 changes the category), or a top-two policy gap <= 2M.  Cap (a condition, not a tolerance): at most 3 % of
the rows, asserted below.

Family E -- edges.  64 hand-made rows pushed straight through CombinedStats.update in two batches (40 + 24), losses by
torch's MSELoss / BCELoss as model.py:318-319 computes them: outputs of exactly 1.0 and 0.0, the float32 neighbours of 1/3
and 2/3 on both sides, tied policy outputs, all-zero policy labels, a value label of 0.25, policy outputs of exactly 0 and
1 (the BCE's -100 clamp).
"""
import json
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(OUT))
sys.path.insert(0, REPO)
sys.path.insert(0, OUT)

import torch  # noqa: E402

from gen_golden import random_position  # noqa: E402
from gen_net_parity_golden import write_npz  # noqa: E402
from oinkoink.neural.config import ModelConfig  # noqa: E402
from oinkoink.neural.pytorch.data import Connect4Dataset  # noqa: E402
from oinkoink.neural.pytorch.model import ModelWrapper  # noqa: E402
from oinkoink.neural.stats import CombinedStats  # noqa: E402

from connect4_amd.training import dataloader_permutation  # noqa: E402

REF = os.path.dirname(os.path.dirname(os.path.abspath(sys.modules["oinkoink"].__file__)))

SEED, N_POS, AGE_MAX, BATCH = 0, 1500, 33, 256
M = 5e-5
CAP = 0.03


def jsonable(d):
    """to_dict() for JSON: numbers as Python floats / ints (exact), the float category keys as strings."""
    out = {}
    for k, v in d.items():
        if isinstance(v, dict):
            out[k] = {repr(float(c)): [int(t) for t in tc] for c, tc in v.items()}
        else:
            out[k] = float(v)
    return out


def categories(v):
    return np.floor(v * np.float32(3.0)) / np.float32(2.0)


def float64_sums(xv, yv, xp, yp):
    xv64, yv64 = xv.astype(np.float64), yv.astype(np.float64)
    out = dict(sum_outputs=float(np.sum(xv64)), value_sq_err_sum=float(np.sum((xv64 - yv64) ** 2)))
    if xp is not None:
        x, y = xp.astype(np.float64), yp.astype(np.float64)
        with np.errstate(divide="ignore"):
            bce = -(y * np.maximum(np.log(x), -100.0) + (1.0 - y) * np.maximum(np.log(1.0 - x), -100.0))
        out["prior_bce_sum"] = float(np.sum(bce))
    return out


def gaps(stats_value, stats_prior, f64):
    """|reference's figure - float64 figure|: for the three sums, and for the figures to_dict() reports -- `average` is the
    reference's own quotient, a float32 one (stats.py:22-24 divides the float32 sum), so its rounding is part of the gap."""
    n = stats_value.n
    g = dict(sum_outputs=abs(float(stats_value.average_value) - f64["sum_outputs"]),
             value_sq_err_sum=abs(float(stats_value.total_loss) - f64["value_sq_err_sum"]),
             average=abs(float(stats_value.average) - f64["sum_outputs"] / n),
             value_loss=abs(float(stats_value.loss) - f64["value_sq_err_sum"] / n))
    if stats_prior is not None:
        g["prior_bce_sum"] = abs(7.0 * float(stats_prior.total_loss) - f64["prior_bce_sum"])
        g["prior_loss"] = abs(float(stats_prior.loss) - f64["prior_bce_sum"] / (7.0 * n))
    return g


class Recorder:
    """Forward hooks on the net and the two criteria of a ModelWrapper: what went in and what came out, per batch."""

    def __init__(self, model):
        self.boards, self.xv, self.xp, self.vloss, self.ploss = [], [], [], [], []
        self.handles = [
            model.net.register_forward_hook(self._net),
            model.value_loss.register_forward_hook(lambda m, i, o: self.vloss.append(o.detach().clone())),
            model.prior_loss.register_forward_hook(lambda m, i, o: self.ploss.append(o.detach().clone()))]

    def _net(self, module, inputs, outputs):
        self.boards.append(inputs[0].detach().clone())
        self.xv.append(outputs[0].detach().clone())
        self.xp.append(outputs[1].detach().clone())

    def close(self):
        for h in self.handles:
            h.remove()


def family_n(model, blobs, meta):
    rng = np.random.RandomState(SEED)
    seen, boards = set(), []
    while len(boards) < N_POS:
        age = int(rng.randint(0, AGE_MAX + 1))
        for _ in range(20):       # (the youngest ages have fewer distinct positions than draws)
            b = random_position(rng, age)
            key = (int(b.color[0]), int(b.color[1]))
            if key not in seen:
                seen.add(key)
                boards.append(b)
                break
    mirrors = [b.create_fliplr() for b in boards]
    everyone = boards + mirrors
    n = len(everyone)
    planes = torch.FloatTensor(np.array([b.to_array() for b in everyone]))
    bits = np.array([[int(b.color[0]), int(b.color[1])] for b in everyone], dtype=np.uint64).view(np.int64)
    ages = np.array([int(b.age) for b in everyone], dtype=np.int32)
    assert ages.min() == 0 and ages.max() == AGE_MAX

    # labels from a first look at the net's answers (one forward; the recorded outputs are the evaluate() pass's)
    with torch.no_grad():
        pv, pp = model.net(planes[:N_POS])
    cat = categories(pv.numpy())
    values = np.empty(N_POS, dtype=np.float32)
    priors = np.zeros((N_POS, 7), dtype=np.float32)
    for i, b in enumerate(boards):
        own = float(cat[i]) if float(cat[i]) in (0.0, 0.5, 1.0) else 1.0
        values[i] = own if rng.rand() < 0.6 else float(rng.choice([0.0, 0.5, 1.0]))
        legal = sorted(int(m) for m in b.valid_moves)
        kind = rng.rand()
        if kind < 0.5 or len(legal) == 1:
            best = int(np.argmax(pp[i].numpy()))
            move = best if (best in legal and rng.rand() < 0.5) else int(rng.choice(legal))
            priors[i, move] = 1.0
        else:
            k = min(len(legal), 2 if kind < 0.8 else 3)
            priors[i, rng.choice(legal, size=k, replace=False)] = 1.0
    values = np.concatenate([values, values])
    priors = np.concatenate([priors, priors[:, ::-1]])
    values_t, priors_t = torch.from_numpy(values), torch.from_numpy(np.ascontiguousarray(priors))

    # ModelWrapper.evaluate(batch_size=256) under torch.manual_seed(0)
    rec = Recorder(model)
    torch.manual_seed(0)
    stats = model.evaluate(Connect4Dataset(planes, values_t, priors_t), batch_size=BATCH)
    rec.close()
    torch.manual_seed(0)
    perm = dataloader_permutation(n)
    xv = np.empty(n, dtype=np.float32)
    xp = np.empty((n, 7), dtype=np.float32)
    for b, (pl, v, p) in enumerate(zip(rec.boards, rec.xv, rec.xp)):
        idx = perm[b * BATCH:(b + 1) * BATCH]
        assert torch.equal(pl, planes[idx]), "batch %d is not rows N_perm[%d:%d]" % (b, b * BATCH, (b + 1) * BATCH)
        xv[idx.numpy()] = v.numpy()
        xp[idx.numpy()] = p.numpy()
    assert len(rec.vloss) == len(rec.ploss) == (n + BATCH - 1) // BATCH
    vloss = np.array([float(x) for x in rec.vloss], dtype=np.float32)
    ploss = np.array([float(x) for x in rec.ploss], dtype=np.float32)
    assert all(np.float32(float(x)) == float(x) for x in rec.vloss)

    # evaluate_value_only (model.py:192-198: its own batch size, loss.item())
    rec2 = Recorder(model)
    torch.manual_seed(0)
    vstats = model.evaluate_value_only(Connect4Dataset(planes, values_t, None))
    rec2.close()
    torch.manual_seed(0)
    perm_vo = dataloader_permutation(n)
    assert len(rec2.xv) == 1 and torch.equal(rec2.boards[0], planes[perm_vo])
    vo_xv = np.empty(n, dtype=np.float32)
    vo_xv[perm_vo.numpy()] = rec2.xv[0].numpy()
    vo_vloss = np.array([float(x) for x in rec2.vloss], dtype=np.float64)

    # every category has members, correct and incorrect ones
    for k, (total, correct) in stats.value_stats.to_dict()["correct"].items():
        assert 0 < correct < total, (k, total, correct)
    assert 0 < stats.prior_stats.correct < n

    # near-boundary mask
    v64 = xv.astype(np.float64)
    top = np.sort(xp.astype(np.float64), axis=1)
    near_third = (np.abs(3 * v64 - 1) <= 3 * M) | (np.abs(3 * v64 - 2) <= 3 * M)
    near_one = v64 >= 1 - M
    near_tie = (top[:, -1] - top[:, -2]) <= 2 * M
    mask = near_third | near_one | near_tie
    share = float(mask.mean())
    print("family N: mask %d of %d rows (near 1/3, 2/3: %d; within M of 1.0: %d; policy near-ties: %d)" %
          (mask.sum(), n, near_third.sum(), near_one.sum(), near_tie.sum()))
    assert share <= CAP, share
    # the value-only pass's outputs (one batch of 3,000) are categorised like the 256-row batches': one mask serves both
    assert np.array_equal(categories(vo_xv), categories(xv))
    vo_mask = mask.copy()

    f64 = float64_sums(xv, values, xp, priors)
    f64_vo = float64_sums(vo_xv, values, None, None)
    blobs.update(N_boards=bits, N_ages=ages, N_values=values, N_priors=np.ascontiguousarray(priors), N_xv=xv, N_xp=xp,
                 N_perm=perm.numpy().astype(np.int32), N_vloss=vloss, N_ploss=ploss, N_mask=mask, N_vo_xv=vo_xv,
                 N_vo_perm=perm_vo.numpy().astype(np.int32), N_vo_vloss=vo_vloss, N_vo_mask=vo_mask)
    meta["N"] = dict(
        rows=n, batch_size=BATCH, M=M, cap=CAP, mask_rows=int(mask.sum()), mask_share=share,
        mask_near_third=int(near_third.sum()), mask_near_one=int(near_one.sum()), mask_near_tie=int(near_tie.sum()),
        evaluate=dict(to_dict=jsonable(stats.to_dict()), repr=repr(stats), float64=f64,
                      gap=gaps(stats.value_stats, stats.prior_stats, f64)),
        evaluate_value_only=dict(to_dict=jsonable(vstats.to_dict()), repr=repr(vstats), float64=f64_vo,
                                 gap=gaps(vstats, None, f64_vo), batch_size=4096))
    print(repr(stats))
    print(repr(vstats))


def family_e(blobs, meta):
    f = np.float32
    third, two_thirds = f(1.0) / f(3.0), f(2.0) / f(3.0)
    lo, hi = f(-np.inf), f(np.inf)
    rng = np.random.RandomState(SEED + 1)
    xv = rng.rand(64).astype(np.float32)
    yv = rng.choice(np.array([0.0, 0.5, 1.0], dtype=np.float32), size=64)
    edge_x = [f(1.0), f(1.0), f(0.0), f(0.0), np.nextafter(third, lo), third, np.nextafter(third, hi), np.nextafter(third, lo),
              third, np.nextafter(third, hi), np.nextafter(two_thirds, lo), two_thirds, np.nextafter(two_thirds, hi),
              np.nextafter(two_thirds, lo), two_thirds, np.nextafter(two_thirds, hi), np.nextafter(f(1.0), lo), f(0.3), f(0.3)]
    edge_y = [1.0, 0.5, 0.0, 1.0, 0.0, 0.0, 0.0, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 1.0, 1.0, 1.0, 1.0, 0.25, 0.0]
    xv[:len(edge_x)] = edge_x
    yv[:len(edge_y)] = edge_y
    xp = rng.dirichlet(np.ones(7), size=64).astype(np.float32)
    yp = np.zeros((64, 7), dtype=np.float32)
    for i in range(64):
        k = int(rng.randint(1, 4))
        yp[i, rng.choice(7, size=k, replace=False)] = 1.0
    xp[0] = [0.25, 0.25, 0.1, 0.1, 0.1, 0.1, 0.1]          # tied outputs: argmax is the first
    yp[0] = [0, 1, 0, 0, 0, 0, 0]
    xp[1] = [0.1, 0.3, 0.3, 0.1, 0.1, 0.05, 0.05]
    yp[1] = [0, 1, 1, 0, 0, 0, 0]
    xp[2] = [0.1, 0.1, 0.3, 0.3, 0.1, 0.05, 0.05]
    yp[2] = [0, 0, 0, 1, 0, 0, 0]
    yp[3] = 0.0                                             # all-zero label rows: always correct
    yp[4] = 0.0
    xp[5] = [1, 0, 0, 0, 0, 0, 0]                           # outputs of exactly 0 and 1: log(0) clamped at -100
    yp[5] = [1, 0, 0, 0, 0, 0, 0]
    xp[6] = [1, 0, 0, 0, 0, 0, 0]
    yp[6] = [0, 1, 0, 0, 0, 0, 0]
    xp[7] = [0, 0, 0, 0, 0, 0, 1]
    yp[7] = [0, 0, 0, 0, 0, 1, 1]
    xp[40] = [0, 0.5, 0.5, 0, 0, 0, 0]
    yp[40] = [0, 0, 1, 0, 0, 0, 0]
    yp[8] = [0.5, 0.5, 0, 0, 0, 0, 0]                       # fractional tied labels
    splits = [0, 40, 64]
    stats = CombinedStats()
    mse, bce = torch.nn.MSELoss(), torch.nn.BCELoss()
    vloss, ploss = [], []
    for a, b in zip(splits[:-1], splits[1:]):
        tv, ty = torch.from_numpy(xv[a:b]), torch.from_numpy(yv[a:b])
        tp, tq = torch.from_numpy(xp[a:b]), torch.from_numpy(yp[a:b])
        lv, lp = mse(tv, ty), bce(tp, tq)
        stats.update(tv.numpy(), ty.numpy(), lv, tp.numpy(), tq.numpy(), lp)
        vloss.append(float(lv))
        ploss.append(float(lp))
    f64 = float64_sums(xv, yv, xp, yp)
    blobs.update(E_xv=xv, E_yv=yv, E_xp=xp, E_yp=yp, E_splits=np.array(splits, dtype=np.int32),
                 E_vloss=np.array(vloss, dtype=np.float32), E_ploss=np.array(ploss, dtype=np.float32))
    meta["E"] = dict(rows=64, to_dict=jsonable(stats.to_dict()), repr=repr(stats), float64=f64,
                     gap=gaps(stats.value_stats, stats.prior_stats, f64))
    print(repr(stats))


def main():
    torch.manual_seed(0)
    torch.set_num_threads(1)
    model = ModelWrapper(ModelConfig(use_gpu=False), os.path.join(REF, "oinkoink", "data", "example_net.pth"))
    blobs, meta = {}, dict(seed=SEED)
    family_n(model, blobs, meta)
    family_e(blobs, meta)
    write_npz(os.path.join(OUT, "stats.npz"), blobs)
    with open(os.path.join(OUT, "stats.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print("stats.npz: %d bytes" % os.path.getsize(os.path.join(OUT, "stats.npz")))


if __name__ == "__main__":
    main()
