#!/usr/bin/env python3
"""The reference's scripts/matches.py on the device: a head-to-head table of a run's checkpoints, every pairing as
Match(plies=2, switch=True) at 800 simulations, all pairings' games in ONE engine inside the fused kernel
(connect4_amd.match.tournament).

    python tools/head_to_head.py SAVE_DIR 20 40 60 80 100 120

plays save_dir/<g>/net.pth for the generations named, every pair once (matches.py plays the later checkpoints against the
earlier ones: name the generations in descending order for its rows), prints the table and writes
SAVE_DIR/head_to_head_results.pkl: a pickled list of {"name": "mcts_nn_<i> vs mcts_nn_<j>", "wins", "draws", "losses",
"return"} -- the frame of matches.py without pandas; wins are the first-named net's."""
import argparse
import os
import pickle
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("save_dir")
    ap.add_argument("generations", type=int, nargs="+")
    ap.add_argument("--simulations", type=int, default=800)
    ap.add_argument("--plies", type=int, default=2)
    ap.add_argument("--precision", default=None, help="FusedNet precision (default: the reference's for the net's width)")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    import torch
    from connect4_amd.evaluators import DeviceNetEvaluator
    from connect4_amd.fused_net import make_selfplay_net
    from connect4_amd.match import tournament
    from connect4_amd.mcts import MCTS, MCTSConfig
    players = []
    for g in args.generations:
        ckpt = torch.load(os.path.join(args.save_dir, str(g), "net.pth"), map_location="cpu", weights_only=True)
        net = make_selfplay_net(ckpt["net_state_dict"], device=args.device, precision=args.precision)
        players.append(MCTS("mcts_nn_%d" % g, MCTSConfig(args.simulations), DeviceNetEvaluator(net, args.device), device=args.device))
    table = tournament(players, plies=args.plies, switch=True)
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
