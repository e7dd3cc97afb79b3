#!/usr/bin/env python3
"""Search given positions with a checkpoint through the position queue (connect4_amd/analysis.py, c4_queue_positions).

    python tools/search_positions.py NET DATASET.pth [--simulations 800] [--slots 4096] [--precision f32x3|f16|f32x3w]
        DATASET is a labelled set as the reference's Connect4Dataset.save writes it (boards / values / priors; priors may be
        missing: the 7- and 8-ply sets).  Prints the reference's stats lines twice: the raw net (stats.score) and the net
        with a search on top (stats.score_search: root mean value and values policy of every position against the labels).
    python tools/search_positions.py NET GRID.txt [--simulations 800]
        GRID is a text grid in the format of the reference's scripts/evaluate_posn.py: six rows of seven characters
        separated by blanks, `o` / `x` for the stones, anything else for an empty cell, the top row first.  Prints the
        board, the net's own value and policy, and the search's move, value, values policy and visit-count policy.

NET is a net.pth (ModelWrapper.save / Trainer.save).  No training net is built: the weights go to make_selfplay_net."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def board_from_grid(path):
    """scripts/evaluate_posn.py:17-23"""
    from connect4_amd.board import Board
    array = np.genfromtxt(path, dtype="c")
    if array.shape != (6, 7):
        raise SystemExit("%s: a grid is six rows of seven characters separated by blanks, got %s" % (path, array.shape))
    return Board.from_pieces(array == b"o", array == b"x")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("net")
    ap.add_argument("positions", help="a labelled set (.pth) or a text grid")
    ap.add_argument("--simulations", type=int, default=800)
    ap.add_argument("--slots", type=int, default=None)
    ap.add_argument("--precision", default=None, choices=("f32x3", "f16", "f32x3w"))
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as entry
    entry.build()
    from connect4_amd.analysis import search_positions, trees
    from connect4_amd.evaluators import DeviceNetEvaluator
    from connect4_amd.fused_net import make_selfplay_net
    from connect4_amd.mcts import MCTSConfig
    from connect4_amd.stats import LabelledSet, score, score_search
    sd = torch.load(a.net, map_location="cpu", weights_only=True)
    net = make_selfplay_net(sd.get("net_state_dict", sd), device=a.device, precision=a.precision)
    cfg = MCTSConfig(a.simulations)
    np.set_printoptions(4)
    try:
        if a.positions.endswith(".pth"):
            ls = LabelledSet.load(a.positions, device="cuda:%d" % a.device)
            print("%d positions\nraw net\n%s" % (len(ls), score(net, ls)))
            print("net + %d simulations\n%s" % (a.simulations, score_search(cfg, net, ls, n_slots=a.slots)))
        else:
            board = board_from_grid(a.positions)
            ev = DeviceNetEvaluator(net, a.device)
            value, prior = ev(board)
            print("{}\nvalue {}, policy {}".format(board, value, np.asarray(prior)))
            rows = search_positions(cfg, [board], ev, device=a.device)
            tree = trees(rows, [board])[0]
            r = rows[0]
            print("move {}, value {}, policy {}\nvisit-count policy {}".format(
                int(r.move), "None" if np.isnan(r.value) else "{:4f}".format(float(r.value)), tree.get_values_policy(),
                tree.get_visit_count_policy()))
    finally:
        if hasattr(net, "close"):
            net.close()


if __name__ == "__main__":
    main()
