#!/usr/bin/env python3
"""GridSearch throughput (connect4_amd/csrc/c4_grid.hip): 4096 seeded random 8-ply positions searched at
depths 4, 5 and 6 with the in-kernel evaluate_centre, one batched call per depth (timed after one warm-up
call), plus the plain-Python host mirror on a few positions for scale.  "open leaves" are the undecided
positions at full depth (the evaluations the reference makes), counted by c4_grid_frontier; "c_call" times
the c4_grid_search call alone, without building the Python tree views.  Prints one JSON object; --out writes it too."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def positions(n, plies, seed):
    from connect4_amd.board import Board
    rng = np.random.RandomState(seed)
    out = []
    while len(out) < n:
        b = Board()
        for _ in range(plies):
            b.make_move(int(rng.choice(sorted(b.valid_moves))))
            if b.result is not None:
                break
        if b.result is None:
            out.append(b)
    return out


def count_leaves(boards, plies):
    """Undecided positions `plies` deep, from the device frontier."""
    from connect4_amd import _lib as L
    from connect4_amd.board import boards_to_bits
    lib = L.load()
    c0, c1 = boards_to_bits(boards)
    got = np.zeros(1, dtype=np.int64)
    rc = lib.c4_grid_frontier(0, c0.ctypes.data_as(L._u64p), c1.ctypes.data_as(L._u64p), len(boards), plies,
                              None, None, 0, got.ctypes.data_as(L._i64p))
    assert rc in (L.OK, L.ECAPACITY), rc
    return int(got[0])


def raw_call_seconds(boards, plies):
    """The c4_grid_search call alone (no Python tree views)."""
    from connect4_amd import _lib as L
    from connect4_amd.board import boards_to_bits
    lib = L.load()
    c0, c1 = boards_to_bits(boards)
    n = len(boards)
    child = np.zeros((n, 7))
    root = np.zeros(n)
    move = np.zeros(n, dtype=np.int32)
    t0 = time.perf_counter()
    rc = lib.c4_grid_search(0, c0.ctypes.data_as(L._u64p), c1.ctypes.data_as(L._u64p), n, plies,
                            child.ctypes.data_as(L._f64p), root.ctypes.data_as(L._f64p), move.ctypes.data_as(L._i32p))
    dt = time.perf_counter() - t0
    assert rc == L.OK, rc
    return dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", type=int, default=4096)
    ap.add_argument("--depths", default="4,5,6")
    ap.add_argument("--host", type=int, default=4, help="positions for the host mirror (depth 4)")
    ap.add_argument("--out")
    args = ap.parse_args()
    from connect4_amd.evaluators import Evaluator, evaluate_centre
    from connect4_amd.grid_search import grid_search, nega_max_host
    boards = positions(args.positions, 8, 0)
    out = {"positions": len(boards), "opening_plies": 8, "device": {}}
    for d in (int(x) for x in args.depths.split(",")):
        grid_search(boards[:64], d, Evaluator(evaluate_centre))        # warm-up (code object load)
        t0 = time.perf_counter()
        grid_search(boards, d, Evaluator(evaluate_centre))
        dt = time.perf_counter() - t0
        leaves = count_leaves(boards, d)
        raw = raw_call_seconds(boards, d)
        out["device"][str(d)] = {"seconds": dt, "positions_per_s": len(boards) / dt, "open_leaves": leaves,
                                 "open_leaves_per_s": leaves / dt, "c_call_seconds": raw,
                                 "c_call_open_leaves_per_s": leaves / raw}
        print("depth %d: %.3f s, %.0f positions/s, %.3g leaves/s" % (d, dt, len(boards) / dt, leaves / dt),
              file=sys.stderr)
    t0 = time.perf_counter()
    for b in boards[:args.host]:
        nega_max_host(b, 4, Evaluator(evaluate_centre))
    dt = time.perf_counter() - t0
    out["host_mirror_depth4"] = {"positions": args.host, "seconds": dt, "positions_per_s": args.host / dt}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
