"""tools/make_book.py and the book options of tools/make_test_set.py, run in-process at a small scale: the 8,231 positions
of ply 6 under budgets that leave most of them unknown, so that the chunk loop, the file written after every chunk,
--resume and the merge all have work to do.  What the tools compute is pinned elsewhere (tests/test_gpu_solver_book.py);
this is about the tools: their files, their reports and that a later sitting keeps what an earlier one proved."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_make_book_resumes_and_make_test_set_reads_the_book(tmp_path):
    from connect4_amd.solver import Book, _book_keys, _interior_rows, enumerate_ply
    path = str(tmp_path / "6ply.npz")
    make_book, make_test_set = tool("make_book"), tool("make_test_set")
    rows = enumerate_ply(6)
    first = make_book.main(["--ply", "6", "--node-budget", "4096", "--chunk", "3000", "-o", path])
    one = Book.load(path)
    assert first["rows"] == len(rows) == 8231 and first["entries"] == len(one) and first["unknown"] == len(one.unknown) > 0
    assert one.age == 6 and 0 < len(one) < len(rows)
    # every row the search can look up is an entry or still unknown; the others (answered by the node that meets them) are neither
    assert np.array_equal(np.sort(np.concatenate([one.keys, _book_keys(one.unknown)])), np.sort(_book_keys(rows[_interior_rows(rows)])))
    second = make_book.main(["--ply", "6", "--node-budget", "65536", "--table-log2", "20", "--chunk", "3000", "--resume", "-o", path])
    two = Book.load(path)
    assert second["rows"] == len(one.unknown) and len(two) > len(one) and len(two.unknown) < len(one.unknown)
    assert np.isin(one.words, two.words).all()              # an outcome bound proved once stays: both sittings used (-1, +1)
    assert not np.isin(_book_keys(two.unknown), two.keys).any()
    with pytest.raises(SystemExit):
        make_book.main(["--ply", "5", "--resume", "-o", path])

    # the 5-ply positions labelled by value with the 6-ply book, against the same run without it
    out = [str(tmp_path / n) for n in ("with.pth", "without.pth")]
    with_book = make_test_set.main(["--all-positions", "5", "--unforced", "--values-only", "--node-budget", "16384", "--book", path, "-o", out[0]])
    without = make_test_set.main(["--all-positions", "5", "--unforced", "--values-only", "--node-budget", "16384", "-o", out[1]])
    assert with_book["rows_read"] == without["rows_read"] == 1922 and with_book["book_entries"] == len(two)
    assert with_book["labelled"] >= without["labelled"] and with_book["table_hits"] > 0
    if not without["labelled"]:
        return
    from connect4_amd.stats import LabelledSet
    a, b = LabelledSet.load(out[0]), LabelledSet.load(out[1])
    rows_a, rows_b = a.boards.cpu().numpy().view(np.uint64), b.boards.cpu().numpy().view(np.uint64)
    both = np.isin(_book_keys(rows_a), _book_keys(rows_b))
    assert both.sum() == len(rows_b)                        # the book loses no row, and where both label a row they agree
    va = dict(zip(_book_keys(rows_a).tolist(), a.values.cpu().numpy().tolist()))
    assert all(va[k] == v for k, v in zip(_book_keys(rows_b).tolist(), b.values.cpu().numpy().tolist()))
