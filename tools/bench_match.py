#!/usr/bin/env python3
"""Time of a net-vs-net match inside the fused kernel (connect4_amd.match.DeviceMatch, c4_match_steps) against the host
lock-step Match (one c4_step + one c4_net_forward launch per simulation round) on the same GPU: Match(plies=2,
switch=True) -- 98 games -- at 800 simulations, the net of tests/golden/net_golden.npz (32 filters, 3 residual blocks)
against a copy whose weights are perturbed by seeded noise, reference precision (f32x3).  One warm-up match per path, then
the best of --repeat.  The device time is also taken over --steps: the quanta (80,000 shader cycles each) a launch may
run; a launch ends earlier when every slot of its net has moved, so this is an upper bound per launch and the one tunable.
Both paths must report the same result dict.  Prints one JSON object; --out writes it too."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def nets(precision, noise, seed):
    import torch
    from connect4_amd.fused_net import FusedNet
    z = np.load(os.path.join(ROOT, "tests", "golden", "net_golden.npz"), allow_pickle=False)
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w__")}
    g = torch.Generator().manual_seed(seed)
    other = {k: (v + noise * v.abs().mean() * torch.randn(v.shape, generator=g) if (v.is_floating_point() and "running_var" not in k and v.ndim > 0) else v.clone())
             for k, v in sd.items()}
    return FusedNet(sd, precision=precision), FusedNet(other, precision=precision)


def timed(fn, repeat):
    fn()                              # warm-up match
    best, out = None, None
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--simulations", type=int, default=800)
    ap.add_argument("--plies", type=int, default=2)
    ap.add_argument("--precision", default="f32x3")
    ap.add_argument("--noise", type=float, default=0.05)
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--steps", type=int, nargs="*", default=[8, 32, 128, 512, 2048])
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    from connect4_amd.evaluators import DeviceNetEvaluator
    from connect4_amd.match import DEFAULT_STEPS_PER_LAUNCH, DeviceMatch, Match
    from connect4_amd.mcts import MCTS, MCTSConfig
    na, nb = nets(args.precision, args.noise, 1)
    cfg = MCTSConfig(args.simulations)
    p1, p2 = MCTS("net", cfg, DeviceNetEvaluator(na)), MCTS("perturbed", cfg, DeviceNetEvaluator(nb))
    out = {"simulations": args.simulations, "plies": args.plies, "precision": args.precision, "noise": args.noise,
           "default_steps_per_launch": DEFAULT_STEPS_PER_LAUNCH, "device": {}}
    results = []
    for n_steps in args.steps:
        m = DeviceMatch(False, p1, p2, plies=args.plies, switch=True, n_steps=n_steps)
        t, res = timed(m.play, args.repeat)
        results.append(res)
        out["games"] = len(m.games)
        out["device"][str(n_steps)] = {"seconds": t, "launches": m.stats["launches"] // n_steps, "moves": m.stats["moves"],
                                       "simulations": m.stats["simulations"], "eval_cache_hits": m.stats["eval_cache_hits"],
                                       "leaf_evals": m.stats["leaf_evals"]}
        print("device, %5d quanta per launch: %.3f s  %r" % (n_steps, t, res), file=sys.stderr)
    out["result"] = results[0]
    assert all(r == results[0] for r in results), results
    if not args.skip_host:
        t, res = timed(lambda: Match(False, p1, p2, plies=args.plies, switch=True).play(), 1)   # (play() consumes the boards)
        out["host"] = {"seconds": t}
        print("host lock-step Match: %.3f s  %r" % (t, res), file=sys.stderr)
        assert res == results[0], (res, results[0])
        best = min(v["seconds"] for v in out["device"].values())
        out["speedup_best"] = t / best
    for p in (p1, p2):
        if p._searcher is not None:
            p._searcher.close()
    na.close()
    nb.close()
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
