#!/usr/bin/env python3
"""Solve a whole ply once and keep it: the book the solver's searches probe (connect4_amd/solver.py Book).

    python tools/make_book.py --ply 8 --table-log2 27 --node-budget 1048576 -o 8ply.npz
    python tools/make_book.py --ply 8 --table-log2 27 --node-budget 16777216 --resume -o 8ply.npz

Every undecided position of the ply, one a mirror pair (solver.enumerate_ply; --unforced: only those where no playable
square completes four), is searched in chunks against one shared transposition table: with the window (-1, +1) -- an
outcome book -- or, --exact, with the full window.  Either book is sound for every caller: its entries are true bounds.
The book is written after every chunk, with the rows the budget left unknown, so a run may be stopped at any time;
--resume loads the file and goes on with its unknown rows only, with whatever budget it is given, and merges.  A partial
book is sound too: a missing entry means the search goes on.  --driver-plies K spreads each row over its descendants K
plies down (solver.solve_window).  Per chunk and at the end: solved / unknown / seconds / nodes."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--ply", type=int, required=True, help="the stones of the book's positions, 0..12")
    ap.add_argument("--unforced", action="store_true")
    ap.add_argument("--exact", action="store_true", help="full windows: exact scores instead of outcomes")
    ap.add_argument("--table-log2", type=int, default=None, metavar="M")
    ap.add_argument("--node-budget", type=int, default=None, metavar="B")
    ap.add_argument("--driver-plies", type=int, default=0, metavar="K")
    ap.add_argument("--chunk", type=int, default=8192, help="rows of one call")
    ap.add_argument("--resume", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("-o", "--output", required=True)
    a = ap.parse_args(argv)
    if not 0 <= a.ply <= 12:
        ap.error("--ply takes 0..12")
    if a.chunk < 1:
        ap.error("--chunk must be positive")
    import __graft_entry__ as entry
    entry.build()
    from connect4_amd import _lib as L
    from connect4_amd.solver import Book, Table, enumerate_ply, solve_window
    if a.resume:
        book = Book.load(a.output)
        if book.age != a.ply:
            raise SystemExit("%s is a book of %d stones, not %d" % (a.output, book.age, a.ply))
        todo = book.unknown
    else:
        book, todo = Book.empty(a.ply), enumerate_ply(a.ply, a.unforced, device=a.device)
    window = (None, None) if a.exact else (-1, 1)
    table = Table(a.table_log2, a.device) if a.table_log2 is not None else None
    t0, nodes, total = time.perf_counter(), 0, len(todo)
    solved, open_rows = 0, []       # of the rows searched so far: how many got an answer, and the ones the budget left unknown
    try:
        for lo in range(0, total, a.chunk):
            rows = np.ascontiguousarray(todo[lo:lo + a.chunk])
            res = solve_window(rows, *window, node_budget=a.node_budget, device=a.device, table=table, driver_plies=a.driver_plies)
            nodes += int(res.nodes.sum())
            solved += int((res.status == L.SOLVE_SOLVED).sum())
            part = Book.from_answers(rows, res, age=a.ply)
            open_rows.append(part.unknown)
            # the file after this chunk: every entry so far, and as unknown the rows the budget left and the rows not yet searched
            book = Book(a.ply, Book(a.ply, book.words).merge(part).words, np.concatenate(open_rows + [todo[lo + a.chunk:]]))
            book.save(a.output)
            print("rows %d..%d: %d solved, %d unknown, %.1f s, %d nodes" % (lo, lo + len(rows), int((res.status == L.SOLVE_SOLVED).sum()),
                                                                            int((res.status == L.SOLVE_UNKNOWN).sum()), time.perf_counter() - t0, nodes), flush=True)
    finally:
        if table is not None:
            table.close()
    if total == 0:
        book = Book(a.ply, book.words)
    book.save(a.output)
    report = {"ply": a.ply, "unforced": a.unforced, "exact": a.exact, "rows": total, "solved": solved, "entries": len(book), "unknown": len(book.unknown),
              "seconds": time.perf_counter() - t0, "nodes": nodes, "table_log2_entries": a.table_log2, "node_budget": a.node_budget,
              "driver_plies": a.driver_plies, "output": a.output}
    print(json.dumps(report))
    return report


if __name__ == "__main__":
    main()
