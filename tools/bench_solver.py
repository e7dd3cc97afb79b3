#!/usr/bin/env python3
"""Measure the exact solver on one GPU (nothing is gated on these figures):

    python tools/bench_solver.py [--out profiles/solver.json]

  nodes_per_empties  512 seeded random playouts per empty-square count 12..24 at the default budget: mean and max nodes, wall time
  kernel_rate        65,536 positions with 20 empty squares (1,024 waves) in one solve(): nodes per second of wall time
  solve_host         the Python mirror's nodes per second on 64 rows of tests/golden/solver_deep.npz, for scale
  generation         4,096 self-play games of a random 32-filter net at 100 simulations; every distinct position with
                     age >= 18 labelled (solver.label): seconds, share unknown, label histogram"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402
entry.build()
from connect4_amd import _lib as L  # noqa: E402
from connect4_amd.solver import label, random_playout, solve, solve_host  # noqa: E402

ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "solver.json"))
args = ap.parse_args()
out = {"command": "python tools/bench_solver.py --out profiles/solver.json", "device": torch.cuda.get_device_name(0)}


def dump():
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


def packed(boards):
    return torch.from_numpy(np.array([b.color for b in boards], dtype=np.uint64).reshape(len(boards), 2).view(np.int64)).cuda()


# 1. nodes per empty-square count: 512 seeded random playouts each, default budget
rng = np.random.RandomState(2024)
solve(packed([random_playout(rng, 30)]))        # warm
per_e = {}
for e in range(12, 25):
    t = packed([random_playout(rng, 42 - e) for _ in range(512)])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = solve(t)
    dt = time.perf_counter() - t0
    per_e[e] = {"positions": 512, "mean_nodes": float(r.nodes.mean()), "max_nodes": int(r.nodes.max()),
                "unknown": int((r.status == L.SOLVE_UNKNOWN).sum()), "seconds": dt}
    print(e, per_e[e], flush=True)
out["nodes_per_empties"] = per_e
dump()

# 2. kernel rate: a batch that fills the device (65,536 positions with 20 empty squares: 1,024 waves)
base = [random_playout(rng, 22) for _ in range(4096)]
t = packed(base).repeat(16, 1).contiguous()
torch.cuda.synchronize()
t0 = time.perf_counter()
r = solve(t)
dt = time.perf_counter() - t0
out["kernel_rate"] = {"positions": int(t.shape[0]), "empties": 20, "nodes": int(r.nodes.sum()), "seconds": dt,
                      "nodes_per_second": float(r.nodes.sum() / dt), "unknown": int((r.status == L.SOLVE_UNKNOWN).sum()),
                      "note": "wall time of solve(): all launches, the compaction between them and the copies of the answers"}
print(out["kernel_rate"], flush=True)
dump()

# 3. solve_host for scale
z = np.load(os.path.join(ROOT, "tests", "golden", "solver_deep.npz"))
t0 = time.perf_counter()
n = 0
for i in range(0, 256, 4):
    n += solve_host((int(z["c0"][i]), int(z["c1"][i]))).nodes
dt = time.perf_counter() - t0
out["solve_host"] = {"positions": 64, "nodes": int(n), "seconds": dt, "nodes_per_second": n / dt}
print(out["solve_host"], flush=True)
dump()

# 4. one 4,096-game generation: every distinct position with age >= 18, labelled
from connect4_amd.config import MCTSConfig  # noqa: E402
from connect4_amd.fused_net import FusedNet  # noqa: E402
from connect4_amd.net import random_init_state_dict  # noqa: E402
from connect4_amd.selfplay import SelfPlay  # noqa: E402
SIMS = 100
net = FusedNet(random_init_state_dict(seed=0))
sp = SelfPlay(net, 4096, MCTSConfig.self_play(SIMS), seed=1, games_target=4096, record_capacity_games=4096, use_graph=False,
              fused_loop=True, steps_per_launch=64)
t0 = time.perf_counter()
while time.perf_counter() - t0 < 200.0:
    sp.run_steps(256)
    if sp.stats()["active_slots"] == 0:
        break
games = sp.engine.export_games()
play_s = time.perf_counter() - t0
sp.close()
net.close()
b = games.boards
bits = b.cpu().numpy().view(np.uint64)
ages = np.array([bin(int(x | y)).count("1") for x, y in bits])
late = b[torch.from_numpy(ages >= 18).to(b.device)].contiguous()
torch.cuda.synchronize()
ls, report = label(late)
hist = {str(k): int((ls.values == k).sum().item()) for k in (0.0, 0.5, 1.0)}
out["generation"] = {"games": int(games.n_games), "simulations": SIMS, "net": "random 32-filter net (random_init_state_dict(seed=0))",
                     "selfplay_seconds": play_s, "positions": int(b.shape[0]), "positions_age_ge_18": int(late.shape[0]),
                     "report": report, "share_unknown": report["unknown"] / max(1, report["distinct"]), "labels": hist}
print(out["generation"], flush=True)
dump()
