#!/usr/bin/env python3
"""Time of the device-side tree export (c4_export_trees) at size: 4096 searches x 800 simulations of the in-kernel centre
evaluator from seeded openings (the run of tests/test_gpu_tree_export.py::test_4096_slots_800_simulations), then all 4096
trees exported in full and with min_visits=2 -- count pass (c4_tree_sizes) and the whole call, host copy included, with nodes
and bytes written.  Next to it the naive alternative: ONE device-to-host copy of as many bytes as those slots' node pools hold
in use (256 B per sibling block; the pools themselves have no entry in the C ABI, a device buffer of that size stands in),
which would still leave the decoding to the host.  Each figure is the best of --repeat calls after one warm-up.
Prints one JSON object; --out writes it too."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def openings(n, seed, max_plies):
    from connect4_amd.board import Board
    rng = np.random.RandomState(seed)
    out = []
    while len(out) < n:
        b = Board()
        for _ in range(int(rng.randint(0, max_plies))):
            b.make_move(int(rng.choice(sorted(b.valid_moves))))
            if b.result is not None:
                break
        if b.result is None:
            out.append(b)
    return out


def best_of(fn, repeat):
    fn()
    best = None
    for _ in range(repeat):
        t0 = time.perf_counter()
        r = fn()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=4096)
    ap.add_argument("--simulations", type=int, default=800)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    from connect4_amd import _lib as L
    from connect4_amd.engine import Engine
    G = args.slots
    boards = openings(G, 11, 20)
    out = {"slots": G, "simulations": args.simulations, "node_bytes": L.tree_node_dtype().itemsize}
    with Engine(G, args.simulations, eval_mode=L.EVAL_CENTRE, stop_after_move=True) as eng:
        eng.reset([b.color[0] for b in boards], [b.color[1] for b in boards])
        t0 = time.perf_counter()
        eng.run_centre()
        out["search_seconds"] = time.perf_counter() - t0
        st = eng.stats()
        for name, mv in (("full", 0), ("min_visits_2", 2)):
            t_count, sizes = best_of(lambda: eng.tree_sizes(min_visits=mv), args.repeat)
            total = int(sizes.sum())
            t_all, tables = best_of(lambda: eng.export_trees(min_visits=mv, capacity=total), args.repeat)
            assert sum(len(t) for t in tables) == total
            del tables
            out[name] = {"nodes": total, "bytes": total * out["node_bytes"], "count_pass_seconds": t_count,
                         "export_seconds": t_all, "nodes_per_s": total / t_all}
            print("%s: %d nodes, %.1f MB, count pass %.4f s, export %.4f s" % (name, total, total * out["node_bytes"] / 1e6, t_count, t_all),
                  file=sys.stderr)
        pool_bytes = (st["leaf_evals"] + G) * 256       # one sibling block per evaluated node + the block that holds node 0
        dev = torch.zeros(pool_bytes, dtype=torch.uint8, device="cuda")
        host = np.zeros(pool_bytes, dtype=np.uint8)

        def copy():
            torch.from_numpy(host).copy_(dev)
            torch.cuda.synchronize()
        t_copy, _ = best_of(copy, args.repeat)
        out["raw_pool_copy"] = {"bytes": pool_bytes, "seconds": t_copy}
        print("raw pools: %.1f MB, %.4f s" % (pool_bytes / 1e6, t_copy), file=sys.stderr)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
