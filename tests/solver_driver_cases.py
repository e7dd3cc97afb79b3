"""What the root-driver tests share (tests/test_solver_driver_host.py, tests/test_gpu_solver_driver.py) with the generator of
tests/golden/solver_driver.npz (tests/golden/gen_solver_driver_golden.py): the stratified sample of tests/golden/solver_exact.npz,
the batches with finished and invalid rows mixed in, the cases of the golden file and how they are stored.

A case is a call of ``solver.drive_host``: rows, a window per row, driver_plies, a quota and a budget; the file holds what the
host mirror answers -- per row and per node -- table-free.  Nothing here is code of the search under test."""
from collections import namedtuple

import numpy as np

from conftest import load_npz
from solver_exact_cases import STRATA
from solver_window_cases import WINDOWS

AMPLE = 1 << 26                 # the default budget: no leaf of any case comes near it
DEFAULT_QUOTA = 1 << 14
SAMPLE_MAX_EMPTIES = 18         # what the host mirror searches in seconds
BATCH_MAX_EMPTIES = 13
BATCH_SIZES = (1, 63, 65, 257)
PLIES = (1, 2, 3)
OPEN_ROOTS = 3                  # open roots with the window (-1, 1): the hardest ones every leaf of which 2^16 nodes answer
OPEN_LEAF_BUDGET = 1 << 16
ROW_FIELDS = ("status", "score", "bound", "outcome", "final_age", "nodes")
NODE_FIELDS = ("lo", "hi", "state", "node_nodes")

Case = namedtuple("Case", "name rows alpha beta plies quota budget")


def exact_rows():
    z = load_npz("solver_exact.npz")
    return z


def stratified_sample(z, per_stratum=5, seed=5):
    """Indices into solver_exact.npz: `per_stratum` rows of every stratum (forced blocks, double threats, every move under an
    opposing win, ...) and of the rows whose mover wins at once, with at most SAMPLE_MAX_EMPTIES empty squares, spread over the
    numbers of empty squares."""
    rng = np.random.RandomState(seed)
    ok = z["empties"] <= SAMPLE_MAX_EMPTIES
    picked = []
    for name in STRATA + ("immediate",):
        member = (~z["tree"] if name == "immediate" else z[name]) & ok
        idx = np.nonzero(member)[0]
        idx = idx[np.argsort(z["empties"][idx], kind="stable")]
        at = np.linspace(0, len(idx) - 1, per_stratum).astype(int) if len(idx) >= per_stratum else np.arange(len(idx))
        at = np.clip(at + rng.randint(0, 3, size=len(at)), 0, len(idx) - 1)
        picked.extend(idx[at].tolist())
    return np.array(sorted(set(picked)), dtype=np.int64)


def specials():
    """(color0, color1) of a finished position (o has won at age 7) and three invalid ones."""
    won0 = sum(1 << (7 * 3 + h) for h in range(4))
    won1 = sum(1 << (7 * 2 + h) for h in range(3))
    c0, c1 = 0b0111, 0b0111 << 7
    return [(won0, won1), (c0, c1 | 1), (0b1111 | 1 << 14, 0b1111 << 7), (c0 | 1 << 48, c1)]


def batch_rows(z, n):
    """n rows of solver_exact.npz with at most BATCH_MAX_EMPTIES empty squares, the specials at 1, 6, 11, 16 where the batch
    has room: (rows uint64 [n, 2], index int64 [n] into the fixture, -1 for a special)."""
    pool = np.nonzero((z["empties"] <= BATCH_MAX_EMPTIES) & (z["empties"] >= 4))[0]
    at = np.random.RandomState(n).choice(pool, size=n, replace=False)
    rows = np.stack([z["c0"][at], z["c1"][at]], axis=1).astype(np.uint64)
    index = at.astype(np.int64)
    for k, sp in enumerate(specials()):
        if 1 + 5 * k < n:
            rows[1 + 5 * k] = sp
            index[1 + 5 * k] = -1
    return rows, index


def cycled_windows(n, shift):
    w = np.array([WINDOWS[(i + shift) % len(WINDOWS)] for i in range(n)], dtype=np.int8).reshape(n, 2)
    return np.ascontiguousarray(w[:, 0]), np.ascontiguousarray(w[:, 1])


def fixed_cases(z):
    """The cases on solver_exact.npz rows, in the file's order: the stratified sample under k = 1, 2, 3 at the quota 256 and
    the default one; the batches under k = 1, 2, 3 with a budget of 64 (quota 16, so that rows park before they run out) and
    an ample one (quota 256 and the default one); two cases whose graph ends in an empty level."""
    out = []
    idx = stratified_sample(z)
    rows = np.stack([z["c0"][idx], z["c1"][idx]], axis=1).astype(np.uint64)
    for k in PLIES:
        a, b = cycled_windows(len(rows), k)
        for quota in (256, DEFAULT_QUOTA):
            out.append(Case("sample_k%d_q%d" % (k, quota), rows, a, b, k, quota, AMPLE))
    for n in BATCH_SIZES:
        rows, _ = batch_rows(z, n)
        for k in PLIES:
            a, b = cycled_windows(n, n + k)
            out.append(Case("batch%d_k%d_b64" % (n, k), rows, a, b, k, 16, 64))
            out.append(Case("batch%d_k%d_ample" % (n, k), rows, a, b, k, 256, AMPLE))
            out.append(Case("batch%d_k%d_default" % (n, k), rows, a, b, k, DEFAULT_QUOTA, AMPLE))
    # graphs whose last level is empty: rows that all answer for themselves, and rows with fewer empty squares than plies
    rows = np.array(specials(), dtype=np.uint64)
    a, b = cycled_windows(len(rows), 0)
    out.append(Case("all_self_k2", rows, a, b, 2, 256, AMPLE))
    short = np.concatenate([np.nonzero(z["empties"] == e)[0][:6] for e in (1, 2)])
    rows = np.stack([z["c0"][short], z["c1"][short]], axis=1).astype(np.uint64)
    a, b = cycled_windows(len(rows), 1)
    out.append(Case("short_k3", rows, a, b, 3, 256, AMPLE))
    return out


def golden_cases():
    """[(Case, {field: array})] of tests/golden/solver_driver.npz."""
    g = load_npz("solver_driver.npz")
    out = []
    for i, name in enumerate(g["names"].tolist()):
        p = "c%02d__" % i
        case = Case(name, g[p + "rows"], g[p + "alpha"], g[p + "beta"], int(g[p + "plies"]), int(g[p + "quota"]), int(g[p + "budget"]))
        out.append((case, {f: g[p + f] for f in ROW_FIELDS + NODE_FIELDS}))
    return out


def mover_score_of_finished(c0, c1):
    """The score for the side to move of a finished position: age - 43 if four are in a row (the mover has lost), else 0."""
    from solver_exact_cases import four
    occ = int(c0) | int(c1)
    lost = bool(four(np.array([c0], dtype=np.uint64))[0] or four(np.array([c1], dtype=np.uint64))[0])
    return bin(occ).count("1") - 43 if lost else 0
