#!/usr/bin/env python3
"""Search one position on the GPU and print the tree that chose the move.

    python tools/show_tree.py 3344 --simulations 800 --max-depth 3 --min-visits 5
    python tools/show_tree.py 334455 --checkpoint net.pth

The position is a string of columns (0-6) played from the empty board, o first.  The evaluator is the centre
heuristic (evaluators.py:28-38) or, with --checkpoint, a network loaded from a state dict.  Prints the board,
Tree.render() under the two filters and both principal variations (by value and by visit count)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("moves", nargs="?", default="", help="columns played so far, e.g. 3344")
    ap.add_argument("--simulations", type=int, default=800)
    ap.add_argument("--checkpoint", help="state dict of the network (default: the centre evaluator)")
    ap.add_argument("--max-depth", type=int, default=2)
    ap.add_argument("--min-visits", type=int, default=1)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    from connect4_amd.board import Board
    from connect4_amd.config import MCTSConfig
    from connect4_amd.evaluators import DeviceNetEvaluator, Evaluator, evaluate_centre_with_prior
    from connect4_amd.mcts import search
    board = Board()
    for ch in args.moves:
        if board.result is not None or int(ch) not in board.valid_moves:
            sys.exit("move %s cannot be played in\n%s" % (ch, board))
        board.make_move(int(ch))
    if board.result is not None:
        sys.exit("the game is over:\n%s" % board)
    if args.checkpoint:
        import torch
        from connect4_amd.fused_net import FusedNet
        ckpt = torch.load(args.checkpoint, map_location="cpu", weights_only=True)
        net = FusedNet(ckpt.get("net_state_dict", ckpt))     # a trainer's net.pth, or a bare state dict
        evaluator = DeviceNetEvaluator(net)
    else:
        evaluator = Evaluator(evaluate_centre_with_prior)
    tree = search(MCTSConfig(args.simulations), board, evaluator, device=args.device, full_tree=True)
    print(board)
    print("%s to move, %d simulations, %d nodes, %d with children" % ("ox"[board.age % 2], tree.simulations, tree.n_nodes, tree.expansions))
    print(tree.render(max_depth=args.max_depth, min_visits=args.min_visits))
    for rule in ("value", "visits"):
        line = tree.principal_variation(rule)
        print("principal variation by %s: %s" % (rule, " ".join(
            "%d(n=%d,v=%s)" % (m, n, "-" if v is None else "%.3f" % v) for m, n, v in line)))


if __name__ == "__main__":
    main()
