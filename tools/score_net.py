#!/usr/bin/env python3
"""Score checkpoints on a labelled set with the reference's statistics (neural/stats.py), on the GPU.

    python tools/score_net.py NET DATASET [--precision f32x3|f16|f32x3w] [--device 0]
    python tools/score_net.py --bench          wall time of stats.score on tests/golden's 3,000 labelled rows and on 135,000

NET is a net.pth (ModelWrapper.save / Trainer.save) or a directory of generations (<g>/net.pth, as run_generations writes
them): every checkpoint is scored, in generation order.  DATASET is a file of the reference's Connect4Dataset.save (a dict
of boards / values / priors; priors may be missing or None: a value-only set).  No training net is built: the weights go
to the fastest evaluator of make_selfplay_net (the fused forward reads the packed boards, 16 B per position) and the
outputs to the device accumulator (connect4_amd/stats.py: score).  Per checkpoint the reference's stats lines are printed
(CombinedStats.__repr__ / ValueStats.__repr__)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def checkpoints(path):
    if os.path.isfile(path):
        return [(os.path.basename(os.path.dirname(os.path.abspath(path))), path)]
    gens = sorted(int(f.name) for f in os.scandir(path) if f.is_dir() and f.name.isdigit() and os.path.exists(os.path.join(f.path, "net.pth")))
    if not gens:
        raise SystemExit("%s holds no <generation>/net.pth" % path)
    return [(str(g), os.path.join(path, str(g), "net.pth")) for g in gens]


def bench(device, precision):
    import numpy as np
    import torch
    from connect4_amd.fused_net import make_selfplay_net
    from connect4_amd.stats import LabelledSet, score
    z = np.load(os.path.join(ROOT, "tests", "golden", "stats.npz"))
    w = np.load(os.path.join(ROOT, "tests", "golden", "net_golden.npz"))
    sd = {k[3:]: torch.from_numpy(w[k]) for k in w.files if k.startswith("w__")}
    net = make_selfplay_net(sd, device=device, precision=precision)
    dev = torch.device("cuda", device)
    small = LabelledSet(*(torch.from_numpy(z[k]).to(dev) for k in ("N_boards", "N_values", "N_priors")))
    large = LabelledSet(small.boards.repeat(45, 1), small.values.repeat(45), small.priors.repeat(45, 1))
    for ls in (small, large):
        score(net, ls)      # warm
        times = []
        for _ in range(5):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            st = score(net, ls)         # (read() waits for the device)
            times.append(time.perf_counter() - t0)
        print("score on %d rows (%s, %s): median %.3f ms, min %.3f ms of 5" %
              (len(ls), type(net).__name__, getattr(net, "precision", "fp32"), sorted(times)[2] * 1e3, min(times) * 1e3))
    print(st)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("net", nargs="?")
    ap.add_argument("dataset", nargs="?")
    ap.add_argument("--precision", default=None, choices=("f32x3", "f16", "f32x3w"))
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--bench", action="store_true")
    a = ap.parse_args()
    import torch
    import __graft_entry__ as entry
    entry.build()
    if a.bench:
        return bench(a.device, a.precision)
    if not a.net or not a.dataset:
        ap.error("NET and DATASET are needed")
    from connect4_amd.fused_net import make_selfplay_net
    from connect4_amd.stats import LabelledSet, score
    ls = LabelledSet.load(a.dataset, device="cuda:%d" % a.device)
    for name, path in checkpoints(a.net):
        sd = torch.load(path, map_location="cpu", weights_only=True)["net_state_dict"]
        net = make_selfplay_net(sd, device=a.device, precision=a.precision)
        try:
            print("%s (%s, %d positions)\n%s" % (name, path, len(ls), score(net, ls)))
        finally:
            if hasattr(net, "close"):
                net.close()


if __name__ == "__main__":
    main()
