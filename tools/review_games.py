#!/usr/bin/env python3
"""Review finished self-play games against exact play (connect4_amd/review.py).

    python tools/review_games.py GAMES [--generation G] [--max-empties E] [--table-log2 N] [--moves] [--host] [--json]
        GAMES: a games.pkl (data.GameStorage) or the directory that holds one; with --generation G a run directory, whose
        G/games.pkl is read (run_generation(s) with write_games_pkl=True).  Prints the review's summary and its by-ply table;
        --json prints one JSON object {"summary", "report"} instead.  --moves also finds the moves that keep the outcome and
        prints how much of the policy target lies on them.  --host reviews with the host mirror (no GPU).

    python tools/review_games.py --bench OUT.json [--games 8192] [--simulations 800] [--slots 4096] [--net NET.pth]
                                 [--max-empties 8 12 16 20] [--table-log2 24] [--repeats 5]
        Plays one generation (NET.pth: a checkpoint of Trainer.save; default: the random-init 32-filter net, seed 0, in its
        default precision), once to warm up and `repeats` times measured, and reviews the last batch at every E, table-free and
        with a table cleared before each run: after one warm-up review the median of `repeats` runs.  Writes seconds, nodes,
        unknown rows, blunders per game, target agreement and the self-play seconds of the same batch to OUT.json."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def load_games(path, generation=None):
    from connect4_amd.data import GameStorage
    from connect4_amd.packed import PackedGames
    if generation is not None:
        path = os.path.join(path, str(generation))
    return PackedGames.from_game_data(GameStorage().load(path))


def print_review(review):
    from connect4_amd.review import BY_PLY_COLUMNS
    s = review.summary()
    share = lambda v: "-" if v is None else "%.4f" % v  # noqa: E731
    print("games %d  positions %d  max_empties %d  late %d  distinct %d  nodes %d  unknown %d  contradictions %d  %.3f s" % (
        s["games"], s["positions"], s["max_empties"], s["late"], review.report["distinct"], review.report["nodes"], s["unknown"],
        s["contradictions"], review.report["seconds"]))
    print("blunders per game %s  target agreement %s" % (share(s["blunders_per_game"]), share(s["target_agreement"])))
    for side in ("o", "x"):
        b = s["by_side"][side]
        print("  %s to move: late %d  blunders %d (%s per game)  target agreement %s" % (
            side, b["late"], b["blunders"], share(b["blunders_per_game"]), share(b["target_agreement"])))
    print(" age " + " ".join("%14s" % c for c in BY_PLY_COLUMNS))
    on_kept = s.get("policy_on_kept_by_ply")
    if on_kept is not None:
        print("policy on keeping moves %s over %d rows" % (share(s["policy_on_kept"]), s["policy_on_kept_rows"]))
    for age, row in enumerate(s["by_ply"]):
        if row[0]:
            print("%4d " % age + " ".join("%14d" % v for v in row) + ("" if on_kept is None else "  policy on kept %s" % share(on_kept[age])))


def games_mode(a):
    from connect4_amd.review import review_games
    from connect4_amd.solver import Table
    games = load_games(a.games_path, a.generation)
    e = a.max_empties[0] if a.max_empties else None
    kw = dict({} if e is None else {"max_empties": e}, moves=a.moves)
    if a.host:
        review = review_games(games, host=True, **kw)
    else:
        table = Table(a.table_log2) if a.table_log2 else None
        try:
            review = review_games(games.to("cuda"), table=table, **kw)
        finally:
            if table is not None:
                table.close()
    if a.json:
        print(json.dumps({"summary": review.summary(), "report": review.report}))
    else:
        print_review(review)


def bench_mode(a):
    import torch
    from connect4_amd.config import MCTSConfig
    from connect4_amd.fused_net import make_selfplay_net
    from connect4_amd.net import random_init_state_dict
    from connect4_amd.review import review_games
    from connect4_amd.selfplay import generate_games_packed
    from connect4_amd.solver import Table
    state = torch.load(a.net, map_location="cpu", weights_only=True)["net_state_dict"] if a.net else random_init_state_dict(seed=0)
    net = make_selfplay_net(state, device=0)
    cfg = MCTSConfig.self_play(a.simulations)
    try:
        selfplay = []
        for run in range(a.repeats + 1):        # the first is the warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            games = generate_games_packed(cfg, net, a.games, n_slots=a.slots, seed=1000)
            torch.cuda.synchronize()
            selfplay.append(time.perf_counter() - t0)
    finally:
        if hasattr(net, "close"):
            net.close()
    selfplay_s = statistics.median(selfplay[1:])
    out = {"workload": "%d self-play games at %d simulations on %d slots, reviewed against exact play" % (a.games, a.simulations, a.slots),
           "net": a.net or "random-init 32 filters, seed 0", "games": games.n_games, "positions": games.n_positions, "repeats": a.repeats,
           "selfplay_s": selfplay_s, "selfplay_runs_s": selfplay[1:], "reviews": []}
    for e in a.max_empties or [8, 12, 16, 20]:
        for log2 in (None, a.table_log2 or 24):
            table = Table(log2) if log2 else None
            try:
                seconds = []
                for run in range(a.repeats + 1):
                    if table is not None:
                        table.clear()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    review = review_games(games, max_empties=e, table=table)
                    torch.cuda.synchronize()
                    seconds.append(time.perf_counter() - t0)
            finally:
                if table is not None:
                    table.close()
            s = review.summary()
            med = statistics.median(seconds[1:])
            out["reviews"].append({"max_empties": e, "table_log2_entries": log2, "seconds": med, "runs_s": seconds[1:],
                                   "seconds_over_selfplay": med / selfplay_s, "late": s["late"], "distinct": review.report["distinct"],
                                   "nodes": review.report["nodes"], "table_hits": review.report["table_hits"], "unknown": s["unknown"],
                                   "contradictions": s["contradictions"], "blunders_per_game": s["blunders_per_game"],
                                   "target_agreement": s["target_agreement"], "by_side": s["by_side"]})
            print(json.dumps(out["reviews"][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.bench)), exist_ok=True)
    with open(a.bench, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "reviews"}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("games_path", nargs="?", help="a games.pkl, its directory, or with --generation a run directory")
    ap.add_argument("--generation", type=int, default=None)
    ap.add_argument("--max-empties", type=int, nargs="+", default=None, help="games mode: one value (default: the library's); --bench: a list")
    ap.add_argument("--table-log2", type=int, default=0, help="games mode: review with a Table of 2^N entries (0: table-free); --bench: the table's size (default 24)")
    ap.add_argument("--moves", action="store_true", help="games mode: also the moves that keep the outcome")
    ap.add_argument("--host", action="store_true", help="the host mirror: no GPU")
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--bench", metavar="OUT.json", default=None)
    ap.add_argument("--games", type=int, default=8192)
    ap.add_argument("--simulations", type=int, default=800)
    ap.add_argument("--slots", type=int, default=4096)
    ap.add_argument("--net", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    if a.bench:
        return bench_mode(a)
    if not a.games_path:
        ap.error("give GAMES, or --bench OUT.json")
    if a.max_empties and len(a.max_empties) != 1:
        ap.error("games mode takes one --max-empties")
    games_mode(a)


if __name__ == "__main__":
    main()
