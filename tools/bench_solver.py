#!/usr/bin/env python3
"""Measure the exact solver on one GPU (nothing is gated on these figures):

    python tools/bench_solver.py [--out profiles/solver.json]

  nodes_per_empties  512 seeded random playouts per empty-square count 12..24 at the default budget: mean and max nodes, wall time
  kernel_rate        65,536 positions with 20 empty squares (1,024 waves) in one solve(): nodes per second of wall time
  solve_host         the Python mirror's nodes per second on 64 rows of tests/golden/solver_deep.npz, for scale
  generation         4,096 self-play games of a random 32-filter net at 100 simulations; every distinct position with
                     age >= 18 labelled (solver.label): seconds, share unknown, label histogram

    python tools/bench_solver.py --table [--budget-log2 20] [--out profiles/solver_table.json]

  the deep search, its transposition table and the split instead: see bench_table below

    python tools/bench_solver.py --window [--part open,seven,seven_big] [--out profiles/solver_window.json]

  labelling by outcome (label(exact=False)) against the exact labelling: see bench_window below"""
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
ap.add_argument("--out", default=None)
ap.add_argument("--table", action="store_true", help="measure the deep search and its transposition table instead (below)")
ap.add_argument("--budget-log2", type=int, default=20, help="--table: the node budget of one row in the budgeted parts")
ap.add_argument("--window", action="store_true", help="measure the labelling by outcome windows instead (below)")
ap.add_argument("--driver", action="store_true", help="measure the root driver against the undriven labelling instead (below)")
ap.add_argument("--driver-budgets-log2", default="20,24", help="--driver: the node budgets of one row")
ap.add_argument("--driver-plies", default="0,2,3", help="--driver: the driver_plies to run, 0 = undriven")
ap.add_argument("--book", default=None, metavar="FILE", help="measure the cost and the gain of carrying a book (tools/make_book.py; 'empty': an empty one) instead (below)")
ap.add_argument("--repeats", type=int, default=7, help="--book: repeats per arm, the median is reported")
ap.add_argument("--part", default="open,seven,seven_big", help="--window: the parts to run; the others are kept from the file")
ap.add_argument("--big-budget-log2", type=int, default=24, help="--window: the node budget of one row in seven_big")
ap.add_argument("--big-count", type=int, default=4096, help="--window: seven_big takes the first N of the 4,096 positions")
args = ap.parse_args()
if args.out is None:
    args.out = os.path.join(ROOT, "profiles", "solver_book.json" if args.book else "solver_driver.json" if args.driver else "solver_window.json" if args.window else "solver_table.json" if args.table else "solver.json")
out = {"command": "python tools/bench_solver.py%s --out profiles/%s" % (" --book %s" % args.book if args.book else " --driver" if args.driver else " --window" if args.window else " --table" if args.table else "",
                                                                       os.path.basename(args.out)),
       "device": torch.cuda.get_device_name(0)}


def dump():
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


def packed(boards):
    return torch.from_numpy(np.array([b.color for b in boards], dtype=np.uint64).reshape(len(boards), 2).view(np.int64)).cuda()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    return r, time.perf_counter() - t0


def summary(r, dt):
    known = (r.status == L.SOLVE_SOLVED) | (r.status == L.SOLVE_TERMINAL)
    return {"positions": int(len(r.status)), "share_solved": float(known.mean()), "unknown": int((r.status == L.SOLVE_UNKNOWN).sum()),
            "mean_nodes": float(r.nodes.mean()), "max_nodes": int(r.nodes.max()), "nodes": int(r.nodes.sum()),
            "table_hits": int(r.table_hits.sum()), "seconds": dt}


def bench_table():
    """--table: writes profiles/solver_table.json (nothing is gated on these figures)

      late          the 512 positions per depth of profiles/solver.json at 20..24 empty squares (same seed, same draws) with
                    Table(24), cleared per depth, default budget; the table-free baseline is that file's
      deep          64 random playouts per depth 25..35 under 2^budget-log2 nodes a row, tables of 2^20 / 2^24 / 2^27
                    entries (cleared per depth) and table-free: share solved, nodes, hits, seconds
      split         64 positions with 30 empty squares, split_plies 0..3, Table(24) cleared per run, the same budget per
                    descendant
      seven_ply     4,096 random 7-ply positions through label(), Table(27), split_plies 0 and 1: seconds, share unknown
      empty_board   the empty board at split_plies 4, 2^22 nodes a descendant: its answer (published: o wins with the 41st
                    stone) or UNKNOWN with the nodes spent"""
    from connect4_amd.solver import Table, random_openings
    budget = 1 << args.budget_log2
    out["budget"] = budget
    rng = np.random.RandomState(2024)
    solve(packed([random_playout(rng, 30)]))        # warm; the draw keeps the sequence of profiles/solver.json
    base = json.load(open(os.path.join(ROOT, "profiles", "solver.json")))["nodes_per_empties"]
    late = {}
    with Table(24) as table:
        for e in range(12, 25):
            boards = [random_playout(rng, 42 - e) for _ in range(512)]
            if e < 20:
                continue
            table.clear()
            r, dt = timed(lambda: solve(packed(boards), table=table))
            late[e] = dict(summary(r, dt), table_free_mean_nodes=base[str(e)]["mean_nodes"], table_free_max_nodes=base[str(e)]["max_nodes"],
                           table_free_seconds=base[str(e)]["seconds"])
            print(e, late[e], flush=True)
    out["late"] = late
    dump()

    rng = np.random.RandomState(2025)
    samples = {e: packed([random_playout(rng, 42 - e) for _ in range(64)]) for e in range(25, 36)}
    deep = {}
    for log2 in (None, 20, 24, 27):
        table = Table(log2) if log2 is not None else None
        for e, t in samples.items():
            if table is not None:
                table.clear()
            r, dt = timed(lambda: solve(t, node_budget=budget, table=table, deep=True))
            deep.setdefault(e, {})["table_free" if log2 is None else "2^%d" % log2] = summary(r, dt)
            print(e, log2, deep[e]["table_free" if log2 is None else "2^%d" % log2], flush=True)
        if table is not None:
            table.close()
    out["deep"] = deep
    dump()

    split = {}
    with Table(24) as table:
        for k in range(4):
            table.clear()
            r, dt = timed(lambda: solve(samples[30], node_budget=budget, table=table, split_plies=k))
            split[k] = summary(r, dt)
            print("split", k, split[k], flush=True)
    out["split"] = split
    dump()

    openings = packed(random_openings(7, 4096, seed=7))
    seven = {}
    with Table(27) as table:
        for k in (0, 1):
            table.clear()
            (ls, report), dt = timed(lambda: label(openings, node_budget=budget, table=table, split_plies=k))
            seven[k] = {"report": report, "share_unknown": report["unknown"] / max(1, report["distinct"]), "seconds": dt}
            print("7-ply", k, seven[k], flush=True)
    out["seven_ply"] = seven
    dump()

    with Table(27) as table:
        r, dt = timed(lambda: solve(torch.zeros((1, 2), dtype=torch.int64).cuda(), node_budget=1 << 22, table=table, split_plies=4))
    out["empty_board"] = dict(summary(r, dt), status=int(r.status[0]), outcome=None if np.isnan(r.outcome[0]) else float(r.outcome[0]),
                              final_age=int(r.final_age[0]), split_plies=4, budget_per_descendant=1 << 22)
    print("empty board", out["empty_board"], flush=True)
    dump()


def bench_book():
    """--book FILE: writes profiles/solver_book.json (nothing is gated on these figures)

      overhead      the 512 positions with 24 empty squares of profiles/solver_table.json's `late` part (same seed, same
                    draws), Table(24) cleared before every run, with the book attached and with none, interleaved in one
                    process after a warm-up: seconds and nodes of every repeat, the medians, and the spread of each arm"""
    from connect4_amd.solver import Book, Table
    rng = np.random.RandomState(2024)
    solve(packed([random_playout(rng, 30)]))
    for e in range(12, 25):
        boards = [random_playout(rng, 42 - e) for _ in range(512)]
    t = packed(boards)
    book = Book.empty(20) if args.book == "empty" else Book.load(args.book)
    runs = {"none": [], "book": []}
    with Table(24) as table:
        solve(t, table=table)       # warm
        for _ in range(args.repeats):
            for arm in ("none", "book"):
                table.clear()
                r, dt = timed(lambda: solve(t, table=table, book=book if arm == "book" else None))
                runs[arm].append({"seconds": dt, "nodes": int(r.nodes.sum()), "table_hits": int(r.table_hits.sum()), "unknown": int((r.status == L.SOLVE_UNKNOWN).sum())})
    book.close()
    out["book"] = {"file": args.book, "age": book.age, "entries": len(book)}
    out["overhead"] = {arm: {"runs": rs, "median_seconds": float(np.median([x["seconds"] for x in rs])),
                             "min_seconds": min(x["seconds"] for x in rs), "max_seconds": max(x["seconds"] for x in rs)} for arm, rs in runs.items()}
    print(json.dumps({arm: {k: v for k, v in o.items() if k != "runs"} for arm, o in out["overhead"].items()}), flush=True)
    dump()


def bench_window():
    """--window: writes profiles/solver_window.json (single runs; nothing is gated on these figures)

      open          the 62 roots of tests/golden/solver_open.npz (25..32 empty squares) through label(exact=True) and
                    label(exact=False), table-free and with a fresh Table(24) each: nodes (per stage), rows, seconds
      seven         random_openings(7, 4096, seed) for seed 0 and for seed 7 (the positions of profiles/solver_table.json's
                    seven_ply) through label(exact=False), Table(27) cleared per run, 2^20 nodes a row: labelled, unknown,
                    nodes per stage, seconds; label_values on the same positions and a cleared table
      seven_big     the first --big-count of the seed-0 positions, Table(27), 2^--big-budget-log2 nodes a row"""
    import threading
    from connect4_amd.solver import Table, label_values, random_openings
    if os.path.exists(args.out):
        out.update({k: v for k, v in json.load(open(args.out)).items() if k in ("open", "seven", "seven_big")})
    parts = [p for p in args.part.split(",") if p]
    threading.Thread(target=lambda: [(time.sleep(60), print("... %d min" % (i + 1), flush=True)) for i in range(60)], daemon=True).start()
    solve(packed([random_playout(np.random.RandomState(1), 30)]))        # warm

    def run(fn):
        (ls, report), dt = timed(fn)
        return {"report": report, "share_unknown": report["unknown"] / max(1, report["distinct"]), "seconds": dt}

    if "open" in parts:
        z = np.load(os.path.join(ROOT, "tests", "golden", "solver_open.npz"))
        t = torch.from_numpy(np.stack([z["c0"], z["c1"]], axis=1).astype(np.uint64).view(np.int64)).cuda()
        res = {"table_free": {"exact": run(lambda: label(t, deep=True)), "staged": run(lambda: label(t, exact=False))}}
        with Table(24) as one, Table(24) as two:
            res["2^24"] = {"exact": run(lambda: label(t, table=one)), "staged": run(lambda: label(t, exact=False, table=two))}
        res["host_mirror_nodes"] = {"table_free": {"exact": 3827125, "staged": 968101, "stage1": 259422},
                                    "note": "solver._Search on the same rows; the table-free device counts must equal these"}
        out["open"] = res
        print("open", json.dumps(res), flush=True)
        dump()
    if "seven" in parts:
        seven = {}
        with Table(27) as table:
            for seed in (0, 7):
                t = packed(random_openings(7, 4096, seed=seed))
                table.clear()
                seven["seed_%d" % seed] = {"staged": run(lambda: label(t, node_budget=1 << 20, table=table, exact=False))}
                table.clear()
                seven["seed_%d" % seed]["values_only"] = run(lambda: label_values(t, node_budget=1 << 20, table=table))
                print("7-ply seed", seed, json.dumps(seven["seed_%d" % seed]), flush=True)
        seven["budget"] = 1 << 20
        seven["parent"] = {"labelled": 164, "share_unknown": 0.9599609375, "nodes": 25831368710, "seconds": 6.30,
                           "note": "label(exact=True), seed 7, Table(27), 2^20 nodes a row: profiles/solver_table.json seven_ply[0]"}
        out["seven"] = seven
        dump()
    if "seven_big" in parts:
        t = packed(random_openings(7, 4096, seed=0)[:args.big_count])
        with Table(27) as table:
            big = run(lambda: label(t, node_budget=1 << args.big_budget_log2, table=table, exact=False))
        out["seven_big"] = dict(big, budget=1 << args.big_budget_log2, positions=int(t.shape[0]), seed=0)
        print("7-ply big", json.dumps(out["seven_big"]), flush=True)
        dump()


def bench_driver():
    """--driver: writes profiles/solver_driver.json (single runs; nothing is gated on these figures)

      the workload of profiles/solver_window.json's seven / seven_big: random_openings(7, 4096, seed 0) through
      label(exact=False), Table(27) cleared before each run, at each budget of --driver-budgets-log2 and each driver_plies of
      --driver-plies (0: the undriven labelling, the baseline of the same session): positions labelled, share unknown, nodes
      entered, seconds, and the graphs' leaves answered, over budget and dropped.  The file is rewritten after every run."""
    from connect4_amd.solver import Table, random_openings
    if os.path.exists(args.out):
        out.update({k: v for k, v in json.load(open(args.out)).items() if k.startswith("budget_")})
    t = packed(random_openings(7, 4096, seed=0))
    solve(packed([random_playout(np.random.RandomState(1), 30)]))        # warm
    with Table(27) as table:
        for log2 in [int(x) for x in args.driver_budgets_log2.split(",") if x]:
            for k in [int(x) for x in args.driver_plies.split(",") if x]:
                table.clear()
                (ls, report), dt = timed(lambda: label(t, node_budget=1 << log2, table=table, exact=False, driver_plies=k))
                run = {"labelled": report["labelled"], "share_unknown": report["unknown"] / max(1, report["distinct"]), "nodes": report["nodes"],
                       "seconds": dt, "leaves": report.get("driver_nodes"), "report": report}
                out.setdefault("budget_2^%d" % log2, {})["driver_plies_%d" % k] = run
                print("2^%d nodes a row, driver_plies %d: %s" % (log2, k, json.dumps(run)), flush=True)
                dump()


if args.book:
    bench_book()
    sys.exit(0)
if args.driver:
    bench_driver()
    sys.exit(0)
if args.table:
    bench_table()
    sys.exit(0)
if args.window:
    bench_window()
    sys.exit(0)

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
