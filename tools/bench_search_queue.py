#!/usr/bin/env python3
"""Time of searching a list of given positions through the position queue (connect4_amd.analysis, c4_queue_positions: G slots
pull N positions inside the fused kernel) against the path every such search took before it: `_Searcher.run` on chunks of G
positions, one slot per position, host-driven (one c4_step + one c4_net_forward launch per simulation round; c4_reset and
c4_read_roots per chunk) -- the code behind MCTS.make_moves, unchanged.

    python tools/bench_search_queue.py [--positions 16384] [--slots 4096] [--plies 8] [--simulations 800] [--repeat 5] [--out FILE]

Positions: seeded random play of --plies moves from the empty board, undecided ones kept.  Net: tests/golden/net_golden.npz
(32 filters, 3 residual blocks), reference precision (f32x3).  Both paths run in one process on the same stream, each on an
engine created once: a warm-up run, then --repeat timed runs, alternating.  The queue is timed from c4_queue_positions_dev to
the rows on the host, once with its evaluation cache (automatic size, cleared before every run, outside the timing) and
once without, so that what the cache adds is told apart from what the queue and the fused launches add; the existing path
has no cache (a stop-after-move engine never had one).  The rows of all three must be equal, bit for bit.  Prints one JSON
object (median, min, max per path; no ratio is asked of it); --out writes it too."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def random_positions(n, plies, seed):
    from connect4_amd.board import Board
    rng = np.random.RandomState(seed)
    out = []
    while len(out) < n:
        b = Board()
        for _ in range(plies):
            if b.result is not None:
                break
            b.make_move(int(rng.choice(sorted(b.valid_moves))))
        if b.result is None and b.age == plies:
            out.append(b)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", type=int, default=16384)
    ap.add_argument("--slots", type=int, default=4096)
    ap.add_argument("--plies", type=int, default=8)
    ap.add_argument("--simulations", type=int, default=800)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--steps", type=int, default=64, help="quanta of 80,000 shader cycles per c4_selfplay_steps launch")
    ap.add_argument("--poll", type=int, default=4, help="launches between two looks at c4_stats.active_slots")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from connect4_amd import _lib as L
    from connect4_amd.analysis import _drive_fused
    from connect4_amd.engine import Engine
    from connect4_amd.evaluators import DeviceNetEvaluator
    from connect4_amd.fused_net import FusedNet
    from connect4_amd.mcts import MCTSConfig, _Searcher
    z = np.load(os.path.join(ROOT, "tests", "golden", "net_golden.npz"), allow_pickle=False)
    net = FusedNet({k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w__")}, precision="f32x3")
    cfg = MCTSConfig(a.simulations)
    boards = random_positions(a.positions, a.plies, seed=1)
    n, G = len(boards), min(a.slots, len(boards))
    packed = torch.from_numpy(np.array([[b.color[0], b.color[1]] for b in boards], dtype=np.uint64).view(np.int64)).cuda()
    dt = L.search_result_dtype()

    engines = {}
    for name, bits in (("queue", 0), ("queue_cache_off", -1)):
        engines[name] = Engine(G, eval_mode=L.EVAL_EXTERNAL_F32, rng_mode=L.RNG_TAPE, stop_after_move=True, position_queue=True,
                               max_inner_iters=32, time_budget_cycles=80000, eval_cache_log2_entries=bits, **cfg.engine_kwargs())
    searcher = _Searcher(cfg, DeviceNetEvaluator(net))
    stats = {}

    def queue_run(name):
        eng = engines[name]
        eng.clear_eval_cache()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.queue_positions_dev(packed)
        _drive_fused(eng, net, a.steps, a.poll)
        rows = eng.queue_results()
        dt_s = time.perf_counter() - t0
        stats[name] = eng.stats()
        return dt_s, rows

    def existing_run():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        parts = [searcher.run(boards[i:i + G]) for i in range(0, n, G)]
        dt_s = time.perf_counter() - t0
        rows = np.frombuffer(b"".join(bytes(r) for p in parts for r in p), dtype=dt)
        return dt_s, rows

    runs = {"queue": lambda: queue_run("queue"), "queue_cache_off": lambda: queue_run("queue_cache_off"), "existing_path": existing_run}
    times = {k: [] for k in runs}
    rows = {}
    for rep in range(a.repeat + 1):      # the first round is the warm-up
        for name, fn in runs.items():
            t, r = fn()
            if rep == 0:
                rows[name] = r
            else:
                times[name].append(t)
            print("%s %s: %.3f s" % ("warm-up" if rep == 0 else "run %d" % rep, name, t), file=sys.stderr)
    for name in ("queue", "queue_cache_off"):
        for f in dt.names:
            assert np.asarray(rows[name][f]).tobytes() == np.asarray(rows["existing_path"][f]).tobytes(), (name, f)
    out = {"positions": n, "slots": G, "plies": a.plies, "simulations": a.simulations, "net": "32f/3res f32x3", "repeat": a.repeat,
           "steps_per_launch": a.steps, "launches_per_poll": a.poll, "rows_equal_bit_for_bit": True,
           "chunks_of_existing_path": -(-n // G)}
    for name, ts in times.items():
        out[name] = {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts), "runs_s": ts,
                     "positions_per_s_at_median": n / statistics.median(ts)}
    for name in ("queue", "queue_cache_off"):
        s = stats[name]
        out[name].update(eval_cache_hits=s["eval_cache_hits"], leaf_evals=s["leaf_evals"], speculative_evals=s["speculative_evals"])
    for e in engines.values():
        e.close()
    searcher.close()
    net.close()
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
