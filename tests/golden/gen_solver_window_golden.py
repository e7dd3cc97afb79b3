#!/usr/bin/env python3
"""Generate tests/golden/solver_window.npz: every row of solver.npz, solver_deep.npz and solver_open.npz answered table-free
by this project's host mirror of the windowed search (connect4_amd.solver.solve_host(window=...)) under the six windows of
tests/solver_window_cases.py.  CPU only, a minute or two.

    PYTHONPATH=<repo>:<repo>/tests python tests/golden/gen_solver_window_golden.py

Arrays: windows int8 [6, 2]; per fixture <name>__score, <name>__bound, <name>__nodes, int8 / int8 / int64 [rows, 6].  Every
row is searched to the end (status SOLVED): the fixtures hold no other."""
import os
import sys
from multiprocessing import Pool

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))


def answer(job):
    from connect4_amd import _lib as L
    from connect4_amd.solver import solve_host
    c0, c1, window = job
    a = solve_host((c0, c1), window=window)
    assert a.status == L.SOLVE_SOLVED, job
    return a.score, a.bound, a.nodes


def main():
    from solver_window_cases import FIXTURES, WINDOWS, fixture_rows
    z = {"windows": np.array(WINDOWS, dtype=np.int8)}
    with Pool(min(16, os.cpu_count() or 1)) as pool:
        for name in FIXTURES:
            rows = fixture_rows(name)
            jobs = [(int(a), int(b), w) for a, b in zip(rows.c0, rows.c1) for w in WINDOWS]
            got = np.array(pool.map(answer, jobs, chunksize=4), dtype=np.int64).reshape(len(rows.c0), len(WINDOWS), 3)
            z[name[:-4] + "__score"] = got[:, :, 0].astype(np.int8)
            z[name[:-4] + "__bound"] = got[:, :, 1].astype(np.int8)
            z[name[:-4] + "__nodes"] = got[:, :, 2]
            print("%s: %d rows, nodes per window %s" % (name, len(rows.c0), got[:, :, 2].sum(axis=0).tolist()))
    np.savez_compressed(os.path.join(OUT, "solver_window.npz"), **z)


if __name__ == "__main__":
    main()
