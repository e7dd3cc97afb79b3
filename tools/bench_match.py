#!/usr/bin/env python3
"""Time of a net-vs-net match inside the fused kernel (connect4_amd.match.DeviceMatch, c4_match_steps) against the host
lock-step Match (one c4_step + one c4_net_forward launch per simulation round) on the same GPU: Match(plies=2,
switch=True) -- 98 games -- at 800 simulations, the net of tests/golden/net_golden.npz (32 filters, 3 residual blocks)
against a copy whose weights are perturbed by seeded noise, reference precision (f32x3).  One warm-up match per path, then
the best of --repeat.  The device time is also taken over --steps: the quanta (80,000 shader cycles each) a launch may
run; a launch ends earlier when every slot of its net has moved, so this is an upper bound per launch and the one tunable.
Both paths must report the same result dict.  Prints one JSON object; --out writes it too.

--kernel wave|split names the match kernel of both nets (default: c4_match_wave_kernel, unconfigured).  --unlike describes
each player to the engine on its own (c4_match_configure), which admits players that are not alike: --filters / --residuals
play a seeded random-init net of that shape instead of the golden one (64 filters in "f32x3w" need --unlike or --kernel
split), and --opponent-filters / --opponent-residuals / --opponent-precision / --opponent-simulations make the second
player differ from the first.  Besides the best time every entry has the median and the range of the --repeat runs."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def weights(filters, residuals):
    """The golden net (32 filters, 3 blocks), or seeded random-init weights of the shape asked for."""
    import torch
    if filters is None and residuals is None:
        z = np.load(os.path.join(ROOT, "tests", "golden", "net_golden.npz"), allow_pickle=False)
        return {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w__")}
    from connect4_amd.net import NetConfig, random_init_state_dict
    return random_init_state_dict(NetConfig(filters=filters or 32, n_residuals=3 if residuals is None else residuals), seed=0)


def perturbed(sd, noise, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    return {k: (v + noise * v.abs().mean() * torch.randn(v.shape, generator=g) if (v.is_floating_point() and "running_var" not in k and v.ndim > 0) else v.clone())
            for k, v in sd.items()}


def nets(precision, noise, seed, filters=None, residuals=None, other_shape=None, other_precision=None):
    """The first player's net and its opponent's: a perturbed copy, or (other_shape = (filters, residuals)) a net of another shape."""
    from connect4_amd.fused_net import FusedNet
    sd = weights(filters, residuals)
    other = perturbed(sd, noise, seed) if other_shape is None else perturbed(weights(*other_shape), noise, seed)
    return FusedNet(sd, precision=precision), FusedNet(other, precision=other_precision or precision)


def timed(fn, repeat):
    """(best seconds, the last result, {"median_seconds", "min_seconds", "max_seconds", "runs"}) of `repeat` runs after one warm-up."""
    fn()                              # warm-up match
    times, out = [], None
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    spread = {"median_seconds": float(np.median(times)), "min_seconds": min(times), "max_seconds": max(times), "runs": len(times)}
    return min(times), out, spread


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--simulations", type=int, default=800)
    ap.add_argument("--plies", type=int, default=2)
    ap.add_argument("--precision", default="f32x3")
    ap.add_argument("--noise", type=float, default=0.05)
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--steps", type=int, nargs="*", default=[8, 32, 128, 512, 2048])
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--host-repeat", type=int, default=1)
    ap.add_argument("--unlike", action="store_true", help="configure every player on its own (c4_match_configure)")
    ap.add_argument("--kernel", choices=["wave", "split"], default=None, help="the match kernel of both nets")
    ap.add_argument("--filters", type=int, default=None)
    ap.add_argument("--residuals", type=int, default=None)
    ap.add_argument("--opponent-filters", type=int, default=None)
    ap.add_argument("--opponent-residuals", type=int, default=None)
    ap.add_argument("--opponent-precision", default=None)
    ap.add_argument("--opponent-simulations", type=int, default=None)
    ap.add_argument("--out")
    args = ap.parse_args()
    from connect4_amd.evaluators import DeviceNetEvaluator
    from connect4_amd.match import DEFAULT_STEPS_PER_LAUNCH, DeviceMatch, Match
    from connect4_amd.mcts import MCTS, MCTSConfig
    other_shape = None
    if args.opponent_filters is not None or args.opponent_residuals is not None:
        other_shape = (args.opponent_filters or 32, 3 if args.opponent_residuals is None else args.opponent_residuals)
    na, nb = nets(args.precision, args.noise, 1, args.filters, args.residuals, other_shape, args.opponent_precision)
    cfg = MCTSConfig(args.simulations)
    cfg2 = cfg if args.opponent_simulations is None else MCTSConfig(args.opponent_simulations)
    p1, p2 = MCTS("net", cfg, DeviceNetEvaluator(na)), MCTS("perturbed", cfg2, DeviceNetEvaluator(nb))
    out = {"simulations": args.simulations, "plies": args.plies, "precision": args.precision, "noise": args.noise,
           "default_steps_per_launch": DEFAULT_STEPS_PER_LAUNCH, "unlike": args.unlike, "kernel": args.kernel,
           "nets": [{"filters": n.config.filters, "residuals": n.config.n_residuals, "precision": n.precision} for n in (na, nb)],
           "device": {}}
    if cfg2 is not cfg:
        out["opponent_simulations"] = args.opponent_simulations
    results = []
    kernels = set()
    for n_steps in args.steps:
        m = DeviceMatch(False, p1, p2, plies=args.plies, switch=True, n_steps=n_steps, unlike=args.unlike, kernel=args.kernel,
                        on_launch=lambda eng: kernels.add(eng.last_fused_kernel().split(" ")[0]))
        t, res, spread = timed(m.play, args.repeat)
        results.append(res)
        out["games"] = len(m.games)
        out["device"][str(n_steps)] = dict(spread, seconds=t, launches=m.stats["launches"] // n_steps, moves=m.stats["moves"],
                                           simulations=m.stats["simulations"], eval_cache_hits=m.stats["eval_cache_hits"],
                                           leaf_evals=m.stats["leaf_evals"])
        print("device, %5d quanta per launch: best %.3f s, median %.3f s  %r" % (n_steps, t, spread["median_seconds"], res), file=sys.stderr)
    out["kernels"] = sorted(kernels)
    out["result"] = results[0]
    assert all(r == results[0] for r in results), results
    if not args.skip_host:
        t, res, spread = timed(lambda: Match(False, p1, p2, plies=args.plies, switch=True).play(), args.host_repeat)   # (play() consumes the boards)
        out["host"] = dict(spread, seconds=t)
        print("host lock-step Match: %.3f s  %r" % (t, res), file=sys.stderr)
        assert res == results[0], (res, results[0])
        best = min(v["seconds"] for v in out["device"].values())
        out["speedup_best"] = t / best
        out["speedup_median"] = spread["median_seconds"] / min(v["median_seconds"] for v in out["device"].values())
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
