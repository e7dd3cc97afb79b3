"""What the exact-leaf overlay costs and buys on the step path (connect4_amd/exact_leaves.py, c4_exact_leaves_dev).

    python tools/bench_exact_leaves.py --out profiles/exact_leaves.json [--games 4096] [--slots 4096] [--simulations 800]
                                       [--empties 6 8 10 12] [--budgets 64 256 1024] [--repeats 5] [--time-limit S]

One process.  Step-path self-play (c4_step, forward, overlay; captured graph) of `games` games on `slots` slots with the
random-init 32-filter / 3-block net in f32x3, seed 0: once to warm up and `repeats` times measured (host clock around work that
ends in a device synchronise, median), without the overlay -- the same path with the plain net -- and with every max_empties x
node_budget.  Per combination: seconds, the ratio to the run without, the counters of the last run (late leaf rows, the share
overridden and over budget, nodes).  The combinations with max_empties = 10 come first, then the launch alone on a batch of
positions drawn from the games played (events around 200 launches), then the rest; --time-limit stops starting new
combinations after that many seconds and says which are missing.  Last, blunders per game (review at 12 empty squares,
connect4_amd.review.review_games, what tools/review_games.py prints) of a batch played with the overlay at max_empties = 10 and
of one played without, same net, same seed.  default_node_budget is the smallest budget whose over-budget share at
max_empties = 10 is under 1 %.  The file is rewritten after every combination."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def play(net, cfg, n_games, n_slots, seed):
    """`n_games` games to the end on the step path (a captured graph of c4_step + forward [+ overlay]); PackedGames."""
    import torch
    from connect4_amd.selfplay import SelfPlay
    sp = SelfPlay(net, n_slots, cfg, seed=seed, games_target=n_games, record_capacity_games=n_games, use_graph=True, fused_loop=False,
                  max_inner_iters=32)
    try:
        while True:
            sp.run_steps(256)
            st = sp.stats()
            if st["active_slots"] == 0:
                break
        if st["dropped_games"] or st["bad_evals"]:
            raise RuntimeError("self-play lost games or answers: %r" % (st,))
        packed = sp.engine.export_games(n_games)
        torch.cuda.synchronize()
        return packed.sorted_by_id(), sp.steps_done
    finally:
        sp.close()


def timed(net, cfg, a, repeats):
    import torch
    seconds, games, steps = [], None, 0
    for run in range(repeats + 1):          # the first is the warm-up
        if hasattr(net, "reset_counters"):
            net.reset_counters()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        games, steps = play(net, cfg, a.games, a.slots, a.seed)
        torch.cuda.synchronize()
        seconds.append(time.perf_counter() - t0)
    return seconds[1:], games, steps


def launch_alone(games, max_empties, budget, n_rows, launches=200):
    """Milliseconds per c4_exact_leaves_dev launch over n_rows positions drawn from the games (seeded), and its counters."""
    import torch
    from connect4_amd import _lib as L
    from connect4_amd.solver import _check
    lib = L.load()
    g = torch.Generator(device="cpu").manual_seed(7)
    rows = games.boards[torch.randint(0, int(games.boards.shape[0]), (n_rows,), generator=g).to(games.boards.device)]
    c0, c1 = rows[:, 0].contiguous(), rows[:, 1].contiguous()
    values = torch.full((n_rows,), 0.25, dtype=torch.float32, device=rows.device)
    counters = torch.zeros(4, dtype=torch.int64, device=rows.device)
    stream = torch.cuda.current_stream().cuda_stream

    def launch():
        _check(lib.c4_exact_leaves_dev(0, C.c_void_p(stream), C.c_void_p(c0.data_ptr()), C.c_void_p(c1.data_ptr()), n_rows, max_empties, budget,
                                       C.c_void_p(values.data_ptr()), C.c_void_p(counters.data_ptr())))
    for _ in range(20):
        launch()
    counters.zero_()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(launches):
        launch()
    end.record()
    torch.cuda.synchronize()
    c = [int(x) // launches for x in counters.cpu().tolist()]
    return {"rows": n_rows, "max_empties": max_empties, "node_budget": budget, "ms_per_launch": start.elapsed_time(end) / launches,
            "counters_per_launch": dict(zip(L.EXACT_LEAVES_COLUMNS, c))}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", required=True)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--slots", type=int, default=4096)
    ap.add_argument("--simulations", type=int, default=800)
    ap.add_argument("--empties", type=int, nargs="+", default=[6, 8, 10, 12])
    ap.add_argument("--budgets", type=int, nargs="+", default=[64, 256, 1024])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1000)
    ap.add_argument("--time-limit", type=float, default=None, help="start no new combination after this many seconds")
    a = ap.parse_args()

    import torch
    from connect4_amd.config import MCTSConfig
    from connect4_amd.exact_leaves import ExactLeafNet
    from connect4_amd.fused_net import FusedNet
    from connect4_amd.net import random_init_state_dict
    from connect4_amd.review import review_games
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    t_start = time.perf_counter()
    cfg = MCTSConfig.self_play(a.simulations)
    net = FusedNet(random_init_state_dict(seed=0), precision="f32x3")
    out = {"workload": "step-path self-play (c4_step, forward, overlay; captured graph): %d games at %d simulations on %d slots" % (
               a.games, a.simulations, a.slots),
           "net": "random-init 32 filters / 3 blocks, seed 0, f32x3", "seed": a.seed, "repeats": a.repeats,
           "timing": "host clock around a run that ends in a device synchronise; median of `repeats` after one warm-up, one process",
           "without": None, "table": [], "not_measured": [], "launch_alone": [], "default_node_budget": None, "blunders": None}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out + ".tmp", "w") as f:
            json.dump(out, f, indent=1)
        os.replace(a.out + ".tmp", a.out)

    try:
        runs, plain_games, steps = timed(net, cfg, a, a.repeats)
        base = statistics.median(runs)
        out["without"] = {"seconds": base, "runs_s": runs, "positions": int(plain_games.n_positions), "steps": steps}
        print(json.dumps({"without": out["without"]}), flush=True)
        save()
        order = [(e, b) for e in a.empties if e == 10 for b in a.budgets] + [(e, b) for e in a.empties if e != 10 for b in a.budgets]
        done_alone = False
        for e, b in order:
            if e != 10 and not done_alone:
                done_alone = True
                for bb in a.budgets:
                    out["launch_alone"].append(launch_alone(plain_games, 10, bb, a.slots))
                    print(json.dumps({"launch_alone": out["launch_alone"][-1]}), flush=True)
                save()
            if a.time_limit is not None and time.perf_counter() - t_start > a.time_limit:
                out["not_measured"].append({"max_empties": e, "node_budget": b})
                continue
            exact = ExactLeafNet(net, e, node_budget=b)
            runs, games, steps = timed(exact, cfg, a, a.repeats)
            c = exact.counters()
            med = statistics.median(runs)
            row = {"max_empties": e, "node_budget": b, "seconds": med, "runs_s": runs, "ratio_to_without": med / base,
                   "positions": int(games.n_positions), "steps": steps, "leaf_rows": steps * a.slots, "late": c["late"], "overridden": c["overridden"],
                   "over_budget": c["over_budget"], "nodes": c["nodes"],
                   "overridden_share_of_late": c["overridden"] / c["late"] if c["late"] else None,
                   "over_budget_share_of_late": c["over_budget"] / c["late"] if c["late"] else None,
                   "late_share_of_leaf_rows": c["late"] / (steps * a.slots)}
            out["table"].append(row)
            print(json.dumps(row), flush=True)
            save()
        if not done_alone:
            for bb in a.budgets:
                out["launch_alone"].append(launch_alone(plain_games, 10, bb, a.slots))
                print(json.dumps({"launch_alone": out["launch_alone"][-1]}), flush=True)
            save()
        at10 = sorted((r["node_budget"], r["over_budget_share_of_late"], r["ratio_to_without"]) for r in out["table"] if r["max_empties"] == 10)
        fit = [x for x in at10 if x[1] is not None and x[1] < 0.01]
        if fit:
            out["default_node_budget"] = {"node_budget": fit[0][0], "over_budget_share_at_10": fit[0][1], "ratio_to_without_at_10": fit[0][2],
                                          "rule": "the smallest budget of the table whose over-budget share at max_empties = 10 is under 1 %"}
        save()
        # blunders per game, reviewed at 12 empty squares: with the overlay (max_empties = 10, that budget) and without
        budget = fit[0][0] if fit else max(a.budgets)
        exact = ExactLeafNet(net, 10, node_budget=budget)
        with_games, _ = play(exact, cfg, a.games, a.slots, a.seed)
        blunders = {}
        for name, games in (("without", plain_games), ("with_overlay", with_games)):
            s = review_games(games, max_empties=12).summary()
            blunders[name] = {k: s[k] for k in ("games", "positions", "late", "unknown", "blunders", "blunders_per_game", "contradictions", "target_agreement")}
        out["blunders"] = dict(blunders, review_max_empties=12, overlay_max_empties=10, overlay_node_budget=budget,
                               note="a measurement of these two batches; no claim that nets trained this way are stronger")
        print(json.dumps({"blunders": out["blunders"]}), flush=True)
        save()
    finally:
        net.close()


if __name__ == "__main__":
    main()
