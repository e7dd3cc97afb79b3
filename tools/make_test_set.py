#!/usr/bin/env python3
"""Turn the late positions of self-play generations into an exactly labelled test set, on the GPU.

    python tools/make_test_set.py SAVE_DIR_OR_DATA_PTH... [--min-age 18] [--max-positions N] [--seed S] -o endgame.pth

Each argument is a data.pth, a generation's directory (holding data.pth) or a run's directory (<g>/data.pth, as
run_generations writes them).  A data.pth holds every position and, in its second half, the mirrored copy of the flip
augmentation (data.py:78-105): the copies are dropped, and of what remains each distinct position is kept once.  Positions
with fewer than --min-age stones are dropped (the solver reaches positions with at most 24 empty squares: age 18);
--max-positions keeps a random subset (--seed).  The rest is solved exactly together with its children
(connect4_amd/solver.py: label -- value = the game-theoretic outcome, prior = uniform over the moves that keep it) and
saved in the format of the reference's Connect4Dataset.save, which LabelledSet.load, tools/score_net.py and
run_generations(test_sets={"endgame": "endgame.pth"}) read.  The labeller's report is printed.

    python tools/make_test_set.py --openings 7 --count 4096 --seed 0 --table-log2 27 --split-plies 2 -o 7ply.pth

--openings PLIES draws --count distinct undecided positions after PLIES uniformly random legal moves (--seed) instead of
reading self-play data: the reference's make_random_ips (scripts/generate_7ply.py), labelled by the same rule.  Positions
with more than 24 empty squares need --table-log2 N (a shared transposition table of 2^N entries; solver.Table) and may
use --split-plies K (solver.solve); --node-budget bounds the nodes of one row.  Positions the budget leaves unknown are
dropped and counted.

    python tools/make_test_set.py --openings 7 --count 4096 --outcome-only --table-log2 27 -o 7ply.pth
    python tools/make_test_set.py --openings 8 --count 4096 --values-only --table-log2 27 -o 8ply.pth

--outcome-only labels the same set from outcomes alone (label(exact=False)): one search per position with the window
(-1, +1) and one null-window search per child that could keep the outcome, instead of exact scores of the position and all
its children -- the same file wherever both label a row, for a fraction of the nodes.  --values-only stops after the first
of those searches and writes values without priors (label_values), the kind of set the reference scores by value only.
Both take positions of any depth with or without --table-log2, from --openings or from data sources; neither splits.
--driver-plies K (1..8) runs their searches through the root driver (solver.solve_window driver_plies): each position is
spread over the lanes of its descendants K plies down and their bounds are folded back, so a position stays unknown only
where a descendant its proof needs does.  The file is the same wherever both label a row.

    python tools/make_test_set.py --all-positions 8 --unforced --values-only --table-log2 27 -o 8ply.pth
    python tools/make_test_set.py --all-positions 7 --outcome-only --book 8ply.npz -o 7ply.pth

--all-positions PLIES is a third source: every undecided position of that ply, one a mirror pair (solver.enumerate_ply);
with --unforced only those where neither side completes four by a playable square -- at 8 plies the 67,557 positions of
the reference's 8-ply set.  --book FILE (tools/make_book.py) is probed by every search wherever it reaches the book's ply:
with an 8-ply book a 7-ply position is labelled by lookups alone."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def data_files(path):
    if os.path.isfile(path):
        return [path]
    own = os.path.join(path, "data.pth")
    if os.path.exists(own):
        return [own]
    gens = sorted(int(f.name) for f in os.scandir(path) if f.is_dir() and f.name.isdigit() and os.path.exists(os.path.join(f.path, "data.pth")))
    if not gens:
        raise SystemExit("%s is no data.pth and holds neither data.pth nor <generation>/data.pth" % path)
    return [os.path.join(path, str(g), "data.pth") for g in gens]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("sources", nargs="*", metavar="SAVE_DIR_OR_DATA_PTH")
    ap.add_argument("--openings", type=int, default=None, metavar="PLIES", help="random positions after PLIES moves, not self-play data")
    ap.add_argument("--count", type=int, default=4096, help="with --openings: how many distinct positions")
    ap.add_argument("--all-positions", type=int, default=None, metavar="PLIES", help="every undecided position of that ply, mirror images merged")
    ap.add_argument("--unforced", action="store_true", help="with --all-positions: only positions where no playable square completes four")
    ap.add_argument("--book", default=None, metavar="FILE", help="a solved ply (tools/make_book.py) the searches probe")
    ap.add_argument("--table-log2", type=int, default=None, metavar="N", help="solve with a transposition table of 2^N entries")
    ap.add_argument("--split-plies", type=int, default=0, metavar="K")
    ap.add_argument("--driver-plies", type=int, default=0, metavar="K", help="with --outcome-only / --values-only: the root driver, K plies deep")
    ap.add_argument("--outcome-only", action="store_true", help="label from outcome windows and null windows (label(exact=False))")
    ap.add_argument("--values-only", action="store_true", help="values without priors, one outcome-window search a position (label_values)")
    ap.add_argument("--node-budget", type=int, default=None)
    ap.add_argument("--min-age", type=int, default=18)
    ap.add_argument("--max-positions", type=int, default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("-o", "--output", required=True)
    a = ap.parse_args(argv)
    if sum([a.openings is not None, a.all_positions is not None, bool(a.sources)]) != 1:
        ap.error("give either sources, --openings or --all-positions")
    if a.all_positions is not None and not 0 <= a.all_positions <= 12:
        ap.error("--all-positions takes 0..12 plies")
    if a.unforced and a.all_positions is None:
        ap.error("--unforced belongs to --all-positions")
    if a.openings is not None and not 0 <= a.openings <= 41:
        ap.error("--openings takes 0..41 plies")
    if a.outcome_only and a.values_only:
        ap.error("--outcome-only and --values-only are two kinds of set: give one")
    staged = a.outcome_only or a.values_only
    if staged and a.split_plies:
        ap.error("--split-plies belongs to the exact labelling")
    if a.driver_plies and not staged:
        ap.error("--driver-plies belongs to --outcome-only and --values-only")
    if a.driver_plies and not 1 <= a.driver_plies <= 8:
        ap.error("--driver-plies takes 1..8")
    plies = a.openings if a.openings is not None else a.all_positions
    if plies is not None and 42 - plies > 24 and a.table_log2 is None and not a.split_plies and not staged and not a.book:
        ap.error("positions with more than 24 empty squares need --table-log2 (or --split-plies)")
    import torch
    import __graft_entry__ as entry
    entry.build()
    from connect4_amd import engine
    from connect4_amd.solver import Book, Table, enumerate_ply, label, label_values, random_openings
    dev = torch.device("cuda", a.device)
    table = Table(a.table_log2, a.device) if a.table_log2 is not None else None
    book = Book.load(a.book) if a.book else None
    parts, rows = [], 0
    if a.openings is not None:
        boards = random_openings(a.openings, a.count, a.seed)
        rows = len(boards)
        bits = np.array([b.color for b in boards], dtype=np.uint64).reshape(rows, 2)
        parts.append(torch.from_numpy(bits.view(np.int64)).to(dev))
    if a.all_positions is not None:
        bits = enumerate_ply(a.all_positions, a.unforced, device=a.device)
        rows = len(bits)
        parts.append(torch.from_numpy(bits.view(np.int64)).to(dev))
    for src in a.sources:
        for path in data_files(src):
            planes = torch.load(path, map_location="cpu", weights_only=True)["boards"]
            if planes.shape[0] % 2:
                raise SystemExit("%s: %d rows -- a data.pth holds every position and its mirror" % (path, planes.shape[0]))
            planes = planes[:planes.shape[0] // 2].to(dev, torch.float32)
            rows += int(planes.shape[0])
            with torch.cuda.device(dev):
                boards, n_bad = engine.planes_to_boards(planes)
            if int(n_bad.item()):
                raise SystemExit("%s: %d rows are not the planes of a board" % (path, int(n_bad.item())))
            age = planes[:, 1:].sum(dim=(1, 2, 3))
            parts.append(boards[age >= a.min_age])
    boards = torch.unique(torch.cat(parts), dim=0)
    late = int(boards.shape[0])
    if a.max_positions is not None and late > a.max_positions:
        g = torch.Generator().manual_seed(a.seed)
        pick = torch.sort(torch.randperm(late, generator=g)[:a.max_positions]).values
        boards = boards[pick.to(dev)].contiguous()
    if a.values_only:
        ls, report = label_values(boards, node_budget=a.node_budget, device=a.device, table=table, driver_plies=a.driver_plies, book=book)
    elif a.outcome_only:
        ls, report = label(boards, node_budget=a.node_budget, device=a.device, table=table, exact=False, driver_plies=a.driver_plies, book=book)
    else:
        ls, report = label(boards, node_budget=a.node_budget, device=a.device, table=table, split_plies=a.split_plies, book=book)
    if table is not None:
        table.close()
    if book is not None:
        book.close()
    ls.save(a.output)
    report = dict(report, rows_read=rows, distinct_late=late, min_age=a.min_age, output=a.output, openings=a.openings, all_positions=a.all_positions, unforced=a.unforced, book=a.book,
                  mode="values-only" if a.values_only else "outcome-only" if a.outcome_only else "exact")
    print(json.dumps(report))
    hist = {k: int((ls.values == k).sum().item()) for k in (0.0, 0.5, 1.0)}
    print("%s: %d positions labelled (x wins %d, draws %d, o wins %d); %d unknown, %.2f s, %d nodes" % (
        a.output, len(ls), hist[0.0], hist[0.5], hist[1.0], report["unknown"], report["seconds"], report["nodes"]))
    return report


if __name__ == "__main__":
    main()
