#!/usr/bin/env python3
"""The reference's scripts/matches.py on the device: a head-to-head table of a run's checkpoints, every pairing as
Match(plies=2, switch=True) at 800 simulations, all pairings' games in ONE engine inside the fused kernel
(connect4_amd.match.tournament).

    python tools/head_to_head.py SAVE_DIR 20 40 60 80 100 120

plays save_dir/<g>/net.pth for the generations named, every pair once (matches.py plays the later checkpoints against the
earlier ones: name the generations in descending order for its rows), prints the table and writes
SAVE_DIR/head_to_head_results.pkl: a pickled list of {"name": "mcts_nn_<i> vs mcts_nn_<j>", "wins", "draws", "losses",
"return"} -- the frame of matches.py without pandas; wins are the first-named net's.

By default the checkpoints must be alike (shape, precision) and all search alike.  --unlike drops that: checkpoints of
different filters and blocks meet, --precision and --simulations take one value per generation (or one for all), and a
64-filter "f32x3w" net plays in the split match kernel; --kernel split puts every net there.

    python tools/head_to_head.py SAVE_DIR 120 60 --unlike --simulations 800 1000"""
import argparse
import os
import pickle
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("save_dir")
    ap.add_argument("generations", type=int, nargs="+")
    ap.add_argument("--simulations", type=int, nargs="+", default=[800], help="one value, or with --unlike one per generation")
    ap.add_argument("--plies", type=int, default=2)
    ap.add_argument("--precision", nargs="+", default=[None],
                    help="FusedNet precision (default: the reference's for the net's width); with --unlike one per generation")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--unlike", action="store_true", help="checkpoints may differ in shape, precision and simulations")
    ap.add_argument("--kernel", choices=["wave", "split"], default=None, help="the match kernel of every net")
    args = ap.parse_args()
    n = len(args.generations)
    for what, values in (("--simulations", args.simulations), ("--precision", args.precision)):
        if len(values) not in (1, n) or (len(values) > 1 and not args.unlike):
            ap.error("%s takes one value, or with --unlike one per generation" % what)
    sims = args.simulations * (n if len(args.simulations) == 1 else 1)
    precisions = args.precision * (n if len(args.precision) == 1 else 1)
    import torch
    from connect4_amd.evaluators import DeviceNetEvaluator
    from connect4_amd.fused_net import make_selfplay_net
    from connect4_amd.match import tournament
    from connect4_amd.mcts import MCTS, MCTSConfig
    players = []
    for g, s, precision in zip(args.generations, sims, precisions):
        ckpt = torch.load(os.path.join(args.save_dir, str(g), "net.pth"), map_location="cpu", weights_only=True)
        net = make_selfplay_net(ckpt["net_state_dict"], device=args.device, precision=precision)
        players.append(MCTS("mcts_nn_%d" % g, MCTSConfig(s), DeviceNetEvaluator(net, args.device), device=args.device))
    table = tournament(players, plies=args.plies, switch=True, unlike=args.unlike, kernel=args.kernel)
    width = max(len(r["name"]) for r in table)
    print("%-*s  %5s %5s %6s %7s" % (width, "name", "wins", "draws", "losses", "return"))
    for r in table:
        print("%-*s  %5d %5d %6d %7.3f" % (width, r["name"], r["wins"], r["draws"], r["losses"], r["return"]))
    with open(os.path.join(args.save_dir, "head_to_head_results.pkl"), "wb") as f:
        pickle.dump(table, f)
    for p in players:
        if hasattr(p.evaluator.net, "close"):
            p.evaluator.net.close()


if __name__ == "__main__":
    main()
