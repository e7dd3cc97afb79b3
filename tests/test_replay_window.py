"""Host side of the device-resident training window (connect4_amd/replay.py, generation.latest_generation): the row
order, which generations a window keeps, the resume rule, the C struct.  No GPU and no kernel call."""
import ctypes
import os

import pytest
import torch


def _segment(n, device="cpu"):
    return (torch.zeros((n, 2), dtype=torch.int64, device=device), torch.zeros(n, dtype=torch.float32, device=device),
            torch.zeros((n, 7), dtype=torch.float32, device=device))


def test_locate_is_the_row_order_of_get_dataset():
    """get_dataset (connect4_amd/data.py:111-116) concatenates, newest generation first, tensors that hold a generation's
    positions followed by their mirrors: the brute-force list below is built exactly that way."""
    from connect4_amd.data import window_generations
    from connect4_amd.replay import ReplayWindow
    sizes = {3: 5, 4: 1, 5: 7}
    w = ReplayWindow("cpu")
    for g, n in sizes.items():
        w.append(g, _segment(n))
    w.select(5)
    assert window_generations(5) == [5, 4, 3] and w.generations == [5, 4, 3]
    expect = []
    for g in window_generations(5):
        expect += [(g, p, False) for p in range(sizes[g])] + [(g, p, True) for p in range(sizes[g])]
    assert w.rows == len(expect) == 26 and w.n_positions == 13
    assert [w.locate(i) for i in range(w.rows)] == expect
    assert w.locate(torch.arange(w.rows)) == expect and w.locate(list(range(w.rows))) == expect
    for bad in (-1, w.rows, 2 ** 40):
        with pytest.raises(IndexError):
            w.locate(bad)
    assert w.nbytes == 48 * 13           # two bitboards, a target, seven priors per position; no table without a GPU


@pytest.mark.parametrize("device", ["cpu", "meta"])
def test_select_keeps_exactly_the_reference_window(device):
    from connect4_amd.data import window_generations
    from connect4_amd.replay import ReplayWindow
    # every generation appended up front: select() alone decides what a window is
    w = ReplayWindow("cpu")
    for g in range(1, 46):
        w.append(g, _segment(g, device))
    for gen in range(1, 46):
        w.select(gen)
        assert w.generations == window_generations(gen)
        assert w.n_positions == sum(window_generations(gen)) and w.rows == 2 * w.n_positions
    # the training loop's order: append a generation, select it; nothing a later window needs was dropped on the way
    w = ReplayWindow("cpu")
    for gen in range(1, 46):
        w.append(gen, _segment(1, device))
        w.select(gen)
        assert w.generations == window_generations(gen)
        assert sorted(w._held) == sorted(window_generations(gen))        # ... and nothing older is kept alive
    assert len(window_generations(45)) == 20
    with pytest.raises(ValueError):
        w.append(45, _segment(1, device))                                # a generation is appended once
    with pytest.raises(ValueError):
        w.append(46, (torch.zeros((3, 2), dtype=torch.int32), torch.zeros(3), torch.zeros((3, 7))))


def test_window_without_a_gpu_says_so():
    from connect4_amd.replay import ReplayWindow
    from connect4_amd.training import ModelConfig, Trainer
    w = ReplayWindow("cpu")
    w.append(1, _segment(3))
    w.select(1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        w.gather(torch.arange(6))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ReplayWindow.from_directory("/nonexistent", 3, "cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Trainer(ModelConfig(use_gpu=False), device="cpu").train_window(w)


def test_latest_generation_is_the_reference_resume_rule(tmp_path):
    """oinkoink/neural/training.py:31-47."""
    from connect4_amd.generation import latest_generation
    d = str(tmp_path)

    def gen_dir(g, net=True):
        os.makedirs(os.path.join(d, str(g)), exist_ok=True)
        if net:
            open(os.path.join(d, str(g), "net.pth"), "wb").close()

    assert latest_generation(d) == (1, None)                            # empty
    assert latest_generation(os.path.join(d, "missing")) == (1, None)
    gen_dir(1)
    assert latest_generation(d) == (1, None)                            # ONE directory: the reference starts over
    os.makedirs(os.path.join(d, "tmp"))
    assert latest_generation(d) == (1, None)                            # ... and a directory that is no generation does not count
    gen_dir(2)
    gen_dir(3)
    assert latest_generation(d) == (4, os.path.join(d, "3", "net.pth"))
    os.remove(os.path.join(d, "3", "net.pth"))
    assert latest_generation(d) == (3, os.path.join(d, "2", "net.pth"))
    os.remove(os.path.join(d, "2", "net.pth"))
    with pytest.raises(FileNotFoundError):
        latest_generation(d)
    gen_dir(10)                                                         # largest by VALUE, not by name
    assert latest_generation(d) == (11, os.path.join(d, "10", "net.pth"))


def test_segment_struct_and_binding():
    from connect4_amd import _lib as L
    assert ctypes.sizeof(L.WindowSegment) == 32
    assert [n for n, _ in L.WindowSegment._fields_] == ["boards", "targets", "policy", "n_positions"]
    assert L.WindowSegment.n_positions.offset == 24
    text = open(L.HEADER_PATH).read()
    assert "#define C4_WINDOW_MAX_SEGMENTS %d" % L.WINDOW_MAX_SEGMENTS in text and L.WINDOW_MAX_SEGMENTS == 64
    for name in ("c4_window_gather_dev", "c4_planes_to_boards_dev", "c4_window_last_error"):
        assert name in L.SIGNATURES and name in text
    assert len(L.SIGNATURES["c4_window_gather_dev"][1]) == 10 and len(L.SIGNATURES["c4_planes_to_boards_dev"][1]) == 6
