"""The device-resident training window on the GPU (connect4_amd/replay.py, csrc/c4_window.hip): c4_window_gather_dev against
indexing the materialised window that c4_training_tensors_dev + torch.cat build (the parent's path), its bounds handling,
c4_planes_to_boards_dev against c4_board_planes, data.pth round trips, Trainer.train_window against Trainer.train and
run_generations against the files it writes.  Everything is compared bit for bit; the one place a tolerance can apply says so.

Positions: seeded random legal playouts with connect4_amd.board.Board; policies random float32 rows, targets from {0, 0.5, 1}."""
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DRAWN_GAME = "361313645534311043046626105524515600224220"      # a random playout that fills the board without a four


def playout_positions(n, seed):
    """(color0, color1) of n undecided positions, in playout order (every age occurs)."""
    from connect4_amd.board import Board
    rng = random.Random(seed)
    out = []
    while len(out) < n:
        b = Board()
        while b.result is None and len(out) < n:
            out.append((b.color[0], b.color[1]))
            b.make_move(rng.choice(sorted(b.valid_moves)))
    return out


def make_segment(n, seed):
    g = torch.Generator().manual_seed(seed)
    boards = torch.tensor(playout_positions(n, seed), dtype=torch.int64).reshape(n, 2)
    targets = torch.randint(0, 3, (n,), generator=g).float() * 0.5
    policy = torch.rand((n, 7), generator=g)
    return boards.cuda(), targets.cuda(), policy.cuda()


def materialised(segments):
    """The window as the parent builds it: torch.cat, newest first, of each generation's training tensors."""
    from connect4_amd import engine
    parts = [engine.training_tensors(*seg) for seg in segments]
    return tuple(torch.cat([p[k] for p in parts]) for k in range(3))


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def assert_gathers(window, mat, idx):
    got = window.gather(idx)
    for g, m, what in zip(got, mat, ("boards", "values", "priors")):
        assert same_bits(g, m[idx.to(m.device)]), (what, int(idx.numel()))


def windows():
    """gen -> segment for two windows: {1, 2, 3} of 5, 1 and 7 positions, and {3, 4, 5} of 7, 3 and 70."""
    a = {1: make_segment(5, 1), 2: make_segment(1, 2), 3: make_segment(7, 3)}
    b = {3: a[3], 4: make_segment(3, 4), 5: make_segment(70, 5)}
    return a, b


def build(segs, gen):
    from connect4_amd.replay import ReplayWindow
    w = ReplayWindow("cuda")
    for g, s in segs.items():
        w.append(g, s)
    return w.select(gen)


def test_gather_is_the_materialised_window():
    a, b = windows()
    for segs, gen, expect_gens in ((a, 3, [3, 2]), (b, 5, [5, 4, 3]), ({1: a[1]}, 1, [1])):
        w = build(segs, gen)
        assert w.generations == expect_gens and w.n_segments == len(expect_gens)      # (generation 1 is outside 3's window)
        mat = materialised([segs[g] for g in expect_gens])
        rows = w.rows
        assert rows == mat[0].shape[0] == 2 * sum(int(segs[g][0].shape[0]) for g in expect_gens)
        assert w.nbytes <= 48 * sum(int(s[0].shape[0]) for s in segs.values()) + 4096
        ar = torch.arange(rows, device="cuda")
        edges, at = [], 0
        for g in expect_gens:       # first and last row of every segment and of every mirrored half
            n = int(segs[g][0].shape[0])
            edges += [at, at + n - 1, at + n, at + 2 * n - 1]
            at += 2 * n
        rnd = torch.randint(0, rows, (4099,), generator=torch.Generator().manual_seed(gen))
        for idx in (ar, ar.flip(0), torch.tensor(edges, device="cuda"), rnd.cuda(), rnd[:1].cuda(), torch.tensor([rows - 1])):
            assert_gathers(w, mat, idx)
        # out= is written in place; a host index list is accepted
        out = tuple(torch.full_like(m[:3], 7.0) for m in mat)
        assert w.gather([rows - 1, 0, 1], out=out)[0] is out[0]
        assert all(same_bits(o, m[[rows - 1, 0, 1]]) for o, m in zip(out, mat))
        # the answer is where locate() says it is
        seg_of = {g: materialised([segs[g]]) for g in expect_gens}
        for i in edges:
            g, pos, mirrored = w.locate(i)
            n = int(segs[g][0].shape[0])
            assert same_bits(mat[0][i], seg_of[g][0][pos + (n if mirrored else 0)])


def test_gather_more_rows_than_one_launch_has_waves():
    """Beyond 4 x 65,536 rows the kernel's waves stride over the batch."""
    _, b = windows()
    w = build(b, 5)
    mat = materialised([b[5], b[4], b[3]])
    idx = torch.randint(0, w.rows, (4 * 65536 + 3,), generator=torch.Generator().manual_seed(9)).cuda()
    assert_gathers(w, mat, idx)


def test_gather_bounds():
    from connect4_amd import _lib as L
    from connect4_amd import engine
    a, _ = windows()
    w = build(a, 3)
    mat = materialised([a[3], a[2]])
    rows = w.rows
    idx = torch.arange(rows).repeat(3)
    bad_at = [0, 17, int(idx.numel()) - 1]
    for at, v in zip(bad_at, (-1, rows, 2 ** 40)):
        idx[at] = v
    idx = idx.cuda()
    m = int(idx.numel())
    out = (torch.full((m, 3, 6, 7), 9.0, device="cuda"), torch.full((m,), 9.0, device="cuda"), torch.full((m, 7), 9.0, device="cuda"))
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    engine.window_gather(w.table_ptr, w.n_segments, idx, *out, counter=counter)
    assert int(counter.item()) == 3
    good = torch.ones(m, dtype=torch.bool)
    good[bad_at] = False
    for o, ref in zip(out, mat):
        assert same_bits(o[good.cuda()], ref[idx[good.cuda()]])
        assert int(o[bad_at].abs().sum().item()) == 0 and same_bits(o[bad_at], torch.zeros_like(o[bad_at]))
    engine.window_gather(w.table_ptr, w.n_segments, idx, *out)          # no counter: same rows, nothing counted
    assert int(out[0][bad_at].abs().sum().item()) == 0
    with pytest.raises(IndexError):
        w.gather(idx)
    unchecked = w.gather(idx, check=False)
    assert same_bits(unchecked[0], out[0])
    lib = L.load()
    stream = torch.cuda.current_stream().cuda_stream
    args = lambda n_segments: (0, stream, w.table_ptr, n_segments, idx.data_ptr(), m, out[0].data_ptr(), out[1].data_ptr(),  # noqa: E731
                               out[2].data_ptr(), None)
    assert lib.c4_window_gather_dev(*args(0)) == L.EINVAL and lib.c4_window_gather_dev(*args(65)) == L.EINVAL
    assert lib.c4_window_gather_dev(*args(-3)) == L.EINVAL and b"segments" in lib.c4_window_last_error()
    assert lib.c4_window_gather_dev(*args(w.n_segments)) == L.OK
    torch.cuda.synchronize()


def test_planes_to_boards_inverts_board_planes():
    from connect4_amd import engine
    from connect4_amd.board import Board
    pos = playout_positions(2000, 7) + [(0, 0)]
    full = Board()
    for ch in DRAWN_GAME:
        full.make_move(int(ch))
    assert full.age == 42 and full.result is not None and full.result.value == 0.5
    pos.append((full.color[0], full.color[1]))
    pos += [(Board.flip_color(c0), Board.flip_color(c1)) for c0, c1 in pos]
    c0 = np.array([p[0] for p in pos], dtype=np.uint64)
    c1 = np.array([p[1] for p in pos], dtype=np.uint64)
    planes = torch.from_numpy(engine.board_planes(c0, c1)).cuda()
    boards, n_bad = engine.planes_to_boards(planes)
    assert int(n_bad.item()) == 0
    assert np.array_equal(boards.cpu().numpy().view(np.uint64), np.stack([c0, c1], 1))
    # rows that no board encodes, each kind alone and the four together
    stone = (planes[:, 1] == 1).flatten(1).float().argmax(1)           # per row: a cell that holds an o stone (rows with one)
    has_o = (planes[:, 1] == 1).flatten(1).any(1)
    r_half, r_both, r_ragged, r_parity = 3, int(has_o.nonzero()[5].item()), 1000, 2001
    bad = planes.clone()
    bad[r_half, 2, 5, 3] = 0.5                                           # neither 0.0 nor 1.0
    bad[r_both, 2].view(-1)[stone[r_both]] = 1.0                         # one cell in both colours
    bad[r_ragged, 0, 2, 4] = 1.0 - bad[r_ragged, 0, 2, 4]                # to-move plane not constant
    bad[r_parity, 0] = 1.0 - bad[r_parity, 0]                            # constant, but the other side's
    rows_bad = [r_half, r_both, r_ragged, r_parity]
    assert len(set(rows_bad)) == 4
    assert int(engine.planes_to_boards(bad)[1].item()) == 4
    for r in rows_bad:
        assert int(engine.planes_to_boards(bad[r:r + 1])[1].item()) == 1
        assert int(engine.planes_to_boards(planes[r:r + 1])[1].item()) == 0
    nan = planes[:2].clone()
    nan[1, 1, 0, 0] = float("nan")
    assert int(engine.planes_to_boards(nan)[1].item()) == 1
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        engine.planes_to_boards(planes[:2].cpu())


def packed(seg):
    from connect4_amd.packed import PackedGames
    b, t, p = seg
    n = int(b.shape[0])
    z = lambda dt, *s: torch.zeros(s, dtype=dt, device=b.device)  # noqa: E731
    return PackedGames(b, z(torch.uint8, n), z(torch.float32, n), p, t, z(torch.int32, n), torch.tensor([n], dtype=torch.int32, device=b.device),
                       z(torch.int8, 1), z(torch.int64, 1))


def test_directory_round_trip(tmp_path):
    from connect4_amd.data import TrainingDataStorage, save_generation
    from connect4_amd.replay import ReplayWindow
    a, _ = windows()
    d = str(tmp_path)
    for g, seg in a.items():
        save_generation(packed(seg), os.path.join(d, str(g)))
    w = ReplayWindow.from_directory(d, 3, "cuda")
    assert w.generations == [3, 2]
    disk = TrainingDataStorage().get_dataset(d, 3)
    got = w.gather(torch.arange(w.rows, device="cuda"))
    assert all(same_bits(g, t.cuda()) for g, t in zip(got, disk))
    assert all(same_bits(x, y) for x, y in zip(w._held[3], a[3]))          # the packed form is the one that was saved
    # lenient about missing generations, as existing_window
    assert ReplayWindow.from_directory(d, 5, "cuda").generations == [3]
    # a second half that is not the mirror of the first: refused, naming the file
    path = os.path.join(d, "3", "data.pth")
    good = torch.load(path, weights_only=True)
    n = good["boards"].shape[0] // 2
    for key, where in (("priors", (n + 2, 6)), ("values", (2 * n - 1,)), ("boards", (n, 1, 5, 0))):
        t = {k: v.clone() for k, v in good.items()}
        t[key][where] = 1.0 - t[key][where] if key == "boards" else t[key][where] + 0.25
        torch.save(t, path)
        with pytest.raises(ValueError, match="3.data.pth"):
            ReplayWindow.from_directory(d, 3, "cuda")
    t = {k: v[:-1].clone() for k, v in good.items()}                         # an odd number of rows
    torch.save(t, path)
    with pytest.raises(ValueError, match="3.data.pth"):
        ReplayWindow.from_directory(d, 3, "cuda")
    t = {k: v.clone() for k, v in good.items()}                              # a first half that is no board
    t["boards"][1, 1, 0, 0] = 0.5
    torch.save(t, path)
    with pytest.raises(ValueError, match="3.data.pth.*not the planes"):
        ReplayWindow.from_directory(d, 3, "cuda")
    torch.save(good, path)
    assert ReplayWindow.from_directory(d, 3, "cuda").rows == w.rows


def test_train_window_is_train_on_the_materialised_window():
    """One dataset of 3 x 64 + 8 rows, batch 64, 2 epochs: two eager full steps, a captured step replayed four times, a
    padded ragged batch of 8 per epoch (the shape of tests/test_gpu_training.py).  train() is run twice from the same
    seeds.  If those two runs agree bit for bit -- the library's reductions have a fixed order -- train_window must agree
    with them bit for bit.  If they do not, the two paths are two draws of the same noise and the bound is the one
    tests/test_gpu_training.py states for the same quantities against its fixture: 5e-5 absolute on weights and batch-norm
    statistics, 5e-4 on the momentum buffers."""
    from connect4_amd.net import NetConfig
    from connect4_amd.replay import ReplayWindow
    from connect4_amd.training import ModelConfig, Trainer
    segs = {3: make_segment(60, 30), 2: make_segment(40, 20)}            # 2 * (60 + 40) = 200 rows
    mat = materialised([segs[3], segs[2]])
    w = ReplayWindow("cuda")
    for g, s in segs.items():
        w.append(g, s)
    w.select(3)
    assert w.rows == mat[0].shape[0] == 3 * 64 + 8

    def run(use_window):
        torch.manual_seed(5)
        tr = Trainer(ModelConfig(net_config=NetConfig(n_residuals=1), batch_size=64, n_training_epochs=2), device="cuda")
        assert tr.use_graph and tr.pad_ragged_batches
        torch.manual_seed(6)
        loss = tr.train_window(w) if use_window else tr.train(*mat)
        assert loss == loss
        state = {"net/" + k: v.detach().clone() for k, v in tr.net.state_dict().items()}
        state.update({"momentum/" + k: tr.optimiser.state[p]["momentum_buffer"].detach().clone() for k, p in tr.net.named_parameters()
                      if tr.optimiser.state[p].get("momentum_buffer") is not None})        # (a parameter without a gradient has none)
        assert sum(k.startswith("momentum/") for k in state) >= 10
        return state, loss, torch.get_rng_state(), [g["lr"] for g in tr.optimiser.param_groups]

    a1, a2, b = run(False), run(False), run(True)
    assert torch.equal(a1[2], b[2]), "train_window consumed torch's RNG differently"
    assert set(a1[0]) == set(a2[0]) == set(b[0])
    assert a1[3] == b[3] and int(b[0]["net/body.0.1.num_batches_tracked"]) == int(a1[0]["net/body.0.1.num_batches_tracked"]) == 8
    reproducible = all(torch.equal(a1[0][k], a2[0][k]) for k in a1[0])

    def worst(x, y, prefix):
        return max(float((x[k].double() - y[k].double()).abs().max()) for k in x if k.startswith(prefix))
    print("train twice: %s (weights %.3g, momentum %.3g); train_window vs train: weights %.3g, momentum %.3g, loss %r vs %r"
          % ("bit-identical" if reproducible else "NOT bit-identical", worst(a1[0], a2[0], "net/"), worst(a1[0], a2[0], "momentum/"),
             worst(a1[0], b[0], "net/"), worst(a1[0], b[0], "momentum/"), a1[1], b[1]))
    if reproducible:
        print("case: the existing path repeats itself bit for bit -> bit-identity required")
        assert all(torch.equal(a1[0][k], b[0][k]) for k in a1[0]) and a1[1] == b[1]
    else:
        print("case: the existing path does not repeat itself -> the fixture test's bounds")
        assert worst(a1[0], b[0], "net/") <= 5e-5 and worst(a1[0], b[0], "momentum/") <= 5e-4
    with pytest.raises(ValueError):
        Trainer(ModelConfig(), device="cuda").train_window(ReplayWindow("cpu"))


def test_run_generations_keeps_the_window_on_the_device(tmp_path):
    from connect4_amd.config import MCTSConfig
    from connect4_amd.data import TrainingDataStorage, window_generations
    from connect4_amd.generation import latest_generation, run_generations
    from connect4_amd.replay import ReplayWindow
    from connect4_amd.training import ModelConfig, Trainer
    d = str(tmp_path)
    torch.manual_seed(0)
    tr = Trainer(ModelConfig(batch_size=256, n_training_epochs=2, use_gpu=True))
    seen = []
    inner = tr.train_window

    def checked_train_window(window, generator=None):
        # what is about to be trained on == the reference's dataset of this generation, read back from disk
        gen = window.generations[0]
        disk = TrainingDataStorage().get_dataset(d, gen)
        got = window.gather(torch.arange(window.rows, device=window.device))
        assert all(same_bits(g, t.to(g.device)) for g, t in zip(got, disk))
        seen.append((gen, window.generations, window.rows, window.n_positions))
        return inner(window, generator)
    tr.train_window = checked_train_window
    timings = []
    cfg = MCTSConfig.self_play(16)
    w0 = tr.net.state_dict()["body.0.0.weight"].detach().clone()
    window, losses = run_generations(tr, cfg, 16, d, 4, first_gen=1, n_slots=16, timings=timings)
    assert [s[0] for s in seen] == [1, 2, 3, 4] and [s[1] for s in seen] == [window_generations(g) for g in (1, 2, 3, 4)]
    assert len(losses) == 4 and all(x == x for x in losses) and not torch.equal(w0, tr.net.state_dict()["body.0.0.weight"])
    assert len(timings) == 4
    for t, (gen, _, rows, n_pos) in zip(timings, seen):
        assert t["generation"] == gen and t["training_rows"] == t["window_rows"] == rows > 0
        assert t["window_bytes"] <= 48 * n_pos + 4096
        assert {"selfplay_and_gather_s", "tensors_and_write_s", "train_s", "positions"} <= set(t)
        assert os.path.exists(os.path.join(d, str(gen), "data.pth")) and os.path.exists(os.path.join(d, str(gen), "net.pth"))
    assert timings[3]["window_rows"] == 2 * (timings[3]["positions"] + timings[2]["positions"])
    assert window.generations == [4, 3]
    # resume: the directory says generation 5 is next; its window is rebuilt from the files
    assert latest_generation(d) == (5, os.path.join(d, "4", "net.pth"))
    tr2 = Trainer(ModelConfig(batch_size=256, n_training_epochs=2, use_gpu=True))
    inner2, seen[:] = tr2.train_window, []

    def checked_resumed(window, generator=None):
        assert all(torch.equal(x, y) for x, y in zip(tr2.net.state_dict().values(), torch.load(
            os.path.join(d, "4", "net.pth"), map_location="cuda", weights_only=True)["net_state_dict"].values()))
        rebuilt = ReplayWindow.from_directory(d, 5, window.device)
        assert rebuilt.generations == window.generations == [5, 4, 3]
        ar = torch.arange(window.rows, device=window.device)
        assert all(same_bits(x, y) for x, y in zip(window.gather(ar), rebuilt.gather(ar)))
        seen.append(5)
        return inner2(window, generator)
    tr2.train_window = checked_resumed
    t2 = []
    run_generations(tr2, cfg, 16, d, 1, n_slots=16, timings=t2)
    assert seen == [5] and t2[0]["generation"] == 5
    assert t2[0]["window_rows"] == 2 * (t2[0]["positions"] + timings[3]["positions"] + timings[2]["positions"])
    assert latest_generation(d) == (6, os.path.join(d, "5", "net.pth"))
