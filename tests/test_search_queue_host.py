"""Host side of the position queue (c4_queue_positions ..., connect4_amd.analysis): the row struct against the header, the
bindings, the documentation of the engine flag, Tree over a row, and the argument checks that run before the GPU is
touched.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from connect4_amd import _lib as L
from connect4_amd import analysis
from connect4_amd.board import Board
from connect4_amd.config import MCTSConfig
from connect4_amd.engine import check_packed_boards
from connect4_amd.evaluators import evaluate_centre_with_prior
from connect4_amd.tree import Tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "c4_engine.h")).read()
QUEUE_SYMBOLS = ("c4_queue_positions", "c4_queue_positions_dev", "c4_queue_progress", "c4_queue_results", "c4_queue_results_dev",
                 "c4_queue_export_dev")
C_TYPES = {"int32_t": (C.c_int32, "<i4"), "uint32_t": (C.c_uint32, "<u4"), "double": (C.c_double, "<f8"),
           "uint64_t": (C.c_uint64, "<u8"), "int64_t": (C.c_int64, "<i8")}


def header_struct(name):
    """[(field, ctype, numpy code, array length or None)] of `typedef struct { ... } name;` in the header."""
    body = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % name, HEADER).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        for item in names.split(","):
            m = re.fullmatch(r"(\w+)(?:\[(\d+)\])?", item.strip())
            out.append((m.group(1), C_TYPES[ctype][0], C_TYPES[ctype][1], int(m.group(2)) if m.group(2) else None))
    return out


def test_search_result_matches_the_header():
    fields = header_struct("c4_search_result")
    assert [f[0] for f in fields] == ["state", "move", "value", "root_visits", "root_value_sum", "child_visits", "child_value_sum",
                                      "child_status", "root_prior", "values_policy", "color0", "color1", "expansions", "simulations"]

    class FromHeader(C.Structure):
        _fields_ = [(n, ct * k if k else ct) for n, ct, _, k in fields]
    assert [n for n, _ in L.SearchResult._fields_] == [f[0] for f in fields]
    assert C.sizeof(L.SearchResult) == C.sizeof(FromHeader) == 296
    dt = L.search_result_dtype()
    assert dt.itemsize == C.sizeof(FromHeader) and list(dt.names) == [f[0] for f in fields]
    for n, ct, code, k in fields:
        assert getattr(L.SearchResult, n).offset == getattr(FromHeader, n).offset == dt.fields[n][1], n
        assert getattr(L.SearchResult, n).size == getattr(FromHeader, n).size, n
        assert dt.fields[n][0] == (np.dtype((code, (k,))) if k else np.dtype(code)), n
    # a row reads like a root read-out: the same fields in the same places
    assert header_struct("c4_root_result") == fields
    assert [(n, getattr(L.RootResult, n).offset) for n, _ in L.RootResult._fields_] == [(n, dt.fields[n][1]) for n in dt.names]


def test_queue_symbols_declared_and_bound():
    text = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    for name in QUEUE_SYMBOLS:
        assert re.search(r"\bint %s\s*\(c4_engine \*e" % name, text), name + " is not declared in the header"
        assert name in L.SIGNATURES and L.SIGNATURES[name][0] is C.c_int, name
    assert len(L.SIGNATURES["c4_queue_positions"][1]) == 4 and len(L.SIGNATURES["c4_queue_positions_dev"][1]) == 3
    assert len(L.SIGNATURES["c4_queue_progress"][1]) == 3 and len(L.SIGNATURES["c4_queue_results"][1]) == 4
    assert len(L.SIGNATURES["c4_queue_results_dev"][1]) == 3 and len(L.SIGNATURES["c4_queue_export_dev"][1]) == 7
    assert re.search(r"#define C4_ABI_VERSION 4\b", HEADER) and L.ABI_VERSION == 4      # additions only


def test_library_exports_the_queue_symbols():
    import __graft_entry__ as g
    g.build_engine()
    lib = L.load()
    for name in QUEUE_SYMBOLS:
        assert hasattr(lib, name)


def test_reserved_1_is_documented():
    cfg = re.search(r"typedef struct \{(.*?)\}\s*c4_config;", HEADER, flags=re.S).group(1)
    doc = cfg[cfg.index("reserved[4]"):]
    assert "reserved[1] = 1" in doc and "position-queue" in doc and "stop_after_move = 1" in doc and "C4_EINVAL" in doc
    assert "c4_reset on a queue engine drops the queue" in HEADER
    assert "C4_ESTATE" in HEADER[HEADER.index("-- position queue"):HEADER.index("int c4_queue_export_dev")]


def synthetic_row(rng, board):
    legal = sorted(board.valid_moves)
    r = L.RootResult()
    r.state, r.color0, r.color1 = 2, board.color[0], board.color[1]
    for m in range(7):
        r.child_status[m] = -2
    vis = 0
    for m in legal:
        kind = rng.randint(0, 4)
        r.child_status[m] = int(rng.randint(0, 3)) if kind == 0 else -1     # a finished child now and then
        r.child_visits[m] = 0 if kind == 1 else int(rng.randint(1, 40))     # and a never-visited one
        r.child_value_sum[m] = float(rng.random_sample() * r.child_visits[m])
        r.root_prior[m] = float(rng.random_sample())
        vis += r.child_visits[m]
    pol = rng.random_sample(7) * [m in legal for m in range(7)]
    for m in range(7):
        r.values_policy[m] = float(pol[m] / pol.sum())
    r.root_visits, r.root_value_sum = vis + 1, float(rng.random_sample() * (vis + 1))
    r.move, r.value = int(legal[0]), float("nan")
    r.expansions, r.simulations = int(rng.randint(1, 50)), vis
    return r


def test_trees_over_rows_equal_tree_over_root_results():
    rng = np.random.RandomState(5)
    boards, roots = [], []
    while len(boards) < 24:
        b = Board()
        for _ in range(int(rng.randint(0, 30))):
            if b.result is not None:
                break
            b.make_move(int(rng.choice(sorted(b.valid_moves))))
        if b.result is None:
            boards.append(b)
            roots.append(synthetic_row(rng, b))
    rows = np.zeros(len(roots), dtype=L.search_result_dtype())
    for i, r in enumerate(roots):       # the same bytes, as Engine.queue_results returns them
        rows[i] = np.frombuffer(bytes(r), dtype=rows.dtype)[0]
    rows = rows.view(np.recarray)
    got = analysis.trees(rows, boards)
    assert len(got) == len(boards)
    for t, t_own_board, r, b in zip(got, analysis.trees(rows), roots, boards):
        want = Tree(r, b)
        for tr in (t, t_own_board):
            assert tr.side == want.side
            assert tr.get_values_policy().tolist() == want.get_values_policy().tolist()
            assert tr.get_visit_count_policy().tolist() == want.get_visit_count_policy().tolist()
            assert tr.best_move().name == want.best_move().name
            assert tr.most_visited().name == want.most_visited().name
            assert tr.root_prior.tolist() == want.root_prior.tolist()
            assert (tr.expansions, tr.simulations) == (want.expansions, want.simulations)
            assert [c.name for c in tr.root.children] == [c.name for c in want.root.children]
            assert [c.data.absolute_value for c in tr.root.children] == [c.data.absolute_value for c in want.root.children]
            assert tr.root.data.search_value.visit_count == want.root.data.search_value.visit_count
            assert tr.root.data.board.color == b.color


def finished_board():
    b = Board()
    for m in (0, 1, 0, 1, 0, 1, 0):
        b.make_move(m)
    assert b.result is not None
    return b


def test_argument_checks_run_before_the_gpu():
    cfg = MCTSConfig(8)
    with pytest.raises(ValueError, match="empty"):
        analysis.search_positions(cfg, [], evaluate_centre_with_prior)
    with pytest.raises(ValueError, match="position 1 is finished"):
        analysis.search_positions(cfg, [Board(), finished_board(), Board()], evaluate_centre_with_prior)
    with pytest.raises(ValueError, match="not a Board"):
        analysis.search_positions(cfg, [Board(), (0, 0)], evaluate_centre_with_prior)
    for bad in (torch.zeros((4, 3), dtype=torch.int64), torch.zeros((4, 2), dtype=torch.int32), torch.zeros(8, dtype=torch.int64),
                torch.zeros((4, 2), dtype=torch.float32), torch.zeros((0, 2), dtype=torch.int64)):
        with pytest.raises(ValueError):
            analysis.search_positions(cfg, bad, evaluate_centre_with_prior)
        with pytest.raises(ValueError):
            check_packed_boards(bad)
    with pytest.raises(ValueError):
        analysis.search_positions(cfg, np.zeros((4, 2), dtype=np.int64), evaluate_centre_with_prior)
    c0, c1, ages = analysis.pack_boards([Board()])
    assert c0.dtype == np.uint64 and c0.tolist() == [0] and c1.tolist() == [0] and ages.tolist() == [0]
    t = torch.zeros((3, 2), dtype=torch.int64)
    assert analysis.pack_boards(t) is t
