"""ReplayWindow.merged (c4_window_merge_dev, csrc/c4_window.hip) against replay.merge_host, the rule in NumPy that
tests/test_window_merge_host.py pins to an independent grouping.  Every comparison is bit for bit, on int32 / int64 views:
the sums are integers, so no order of arrival and no table size may show in a result.  Then the merged window downstream:
gather, Trainer.train_window and run_generations(merge_duplicates=True)."""
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def stones(moves):
    from connect4_amd.board import Board
    b = Board()
    for m in moves:
        b.make_move(m)
    return b.color[0], b.color[1]


def flip(pos):
    from connect4_amd.board import Board
    return Board.flip_color(pos[0]), Board.flip_color(pos[1])


def segment(positions, seed, policy=None, targets=None):
    """(boards, targets, policy) as numpy arrays: random float32 priors in [0, 1), targets from {0, 0.5, 1}."""
    n = len(positions)
    rng = np.random.RandomState(seed)
    t = (rng.randint(0, 3, n) * 0.5).astype(np.float32) if targets is None else np.asarray(targets, dtype=np.float32)
    p = rng.rand(n, 7).astype(np.float32) if policy is None else np.asarray(policy, dtype=np.float32).reshape(n, 7)
    return np.array(positions, dtype=np.uint64).reshape(n, 2).view(np.int64), t, p


def playouts(n, seed, max_plies=6):
    from connect4_amd.board import Board
    rng = random.Random(seed)
    pos = []
    while len(pos) < n:
        b = Board()
        for _ in range(rng.randint(0, max_plies)):
            if b.result is None:
                b.make_move(rng.choice(sorted(b.valid_moves)))
        pos.append((b.color[0], b.color[1]))
    return pos


def window_of(segments, first_gen=1):
    """Segments oldest first, as generations first_gen, first_gen + 1, ...: the window lists them newest first."""
    from connect4_amd.replay import ReplayWindow
    w = ReplayWindow("cuda")
    for g, seg in enumerate(segments, first_gen):
        w.append(g, tuple(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in seg))
    w._activate(sorted(w._held, reverse=True))
    return w


def table_order(segments):
    return tuple(np.concatenate([seg[k] for seg in reversed(segments)]) for k in range(3))


def bits(x):
    if isinstance(x, torch.Tensor):
        x = x.cpu().numpy()
    x = np.ascontiguousarray(x)
    return x.view(np.int32) if x.dtype == np.float32 else x


def same(a, b):
    return len(a) == len(b) and all(bits(x).dtype == bits(y).dtype and bits(x).shape == bits(y).shape and np.array_equal(bits(x), bits(y))
                                    for x, y in zip(a, b))


def outputs(w):
    (gen,) = w.generations
    return tuple(w._held[gen]) + (w.merge_counts,)


def raw_merge(w, mirror, log2_capacity, wave_combine):
    """c4_window_merge_dev itself, with the plain or the wave-combining insert: the rows written and the bad-row count."""
    from connect4_amd import engine
    b, t, p, c, heads = engine.window_merge(w.table_ptr, w.n_segments, w.n_positions, w.device, mirror, log2_capacity, wave_combine)
    d, bad = heads.tolist()
    return (b[:d], t[:d], p[:d], c[:d]), bad


def check(segments, mirror=True, log2_capacity=None):
    from connect4_amd.replay import merge_host
    w = window_of(segments)
    before = [tuple(t.clone() for t in w._held[g]) for g in w.generations]
    ref = merge_host(*table_order(segments), mirror=mirror)
    m = w.merged(mirror=mirror, log2_capacity=log2_capacity)
    got = outputs(m)
    assert same(got, ref), (len(ref[3]), int(got[3].numel()))
    for wave_combine in (False, True):
        rows, bad = raw_merge(w, mirror, log2_capacity, wave_combine)
        assert bad == 0 and same(rows, ref), wave_combine
    assert m.generations == [w.generations[0]] and m.merged_from == w.n_positions == int(ref[3].sum())
    assert m.n_positions == len(ref[3]) and m.rows == 2 * len(ref[3]) and m.device == w.device
    assert got[3].dtype == torch.int32 and got[0].dtype == torch.int64
    assert all(same(x, y) for x, y in zip(before, [w._held[g] for g in w.generations]))        # the source is untouched
    return got, ref


def test_small_shapes():
    one, pair = stones([2, 2, 5]), stones([6, 0])
    for mirror in (True, False):
        got, _ = check([segment([one], 1)], mirror)                              # n = 1: a table of two slots
        assert got[3].tolist() == [1]
        check([segment([one], 1)], mirror, log2_capacity=0)                      # ... and of one
        got, _ = check([segment([one, one], 2)], mirror)
        assert got[3].tolist() == [2]
        got, _ = check([segment([pair, flip(pair)], 3)], mirror)
        assert got[3].tolist() == ([2] if mirror else [1, 1])
        got, _ = check([segment([flip(pair), pair], 3)], mirror)                 # (one of the two orders has a reversed first member)
    # three segments, duplicates within and across them; table order is newest first
    a, b, c = stones([3]), stones([3, 4]), stones([0, 6, 1])
    segs = [segment([a, b, flip(c), a], 4), segment([c, stones([])], 5), segment([b, flip(b), a, stones([]), c, stones([1])], 6)]
    got, ref = check(segs)
    assert got[3].tolist() == [3, 3, 2, 3, 1] and int(got[0][0, 0]) == b[0]       # (b, its image and b again; a three times; ...)
    check(segs, mirror=False)


def test_contention():
    from connect4_amd.replay import merge_host
    hot, other = stones([3, 3]), playouts(300, 7)
    check([segment([hot] * 65, 1)])                                              # one group that crosses a wave
    check([segment([hot] * 64 + [flip(stones([1]))] + [hot], 1)])
    crowd = other[:150] + [hot if i % 3 else flip(hot) for i in range(1000)] + other[150:]      # crosses workgroups
    random.Random(2).shuffle(crowd)
    got, _ = check([segment(crowd, 2)])
    assert int(got[3].max()) >= 1000
    got, _ = check([segment([stones([])] * 700, 3), segment([stones([])] * 77, 4)])      # a window that is one single group
    assert got[3].tolist() == [777]
    exact = segment([hot] * 1000, 5, policy=np.tile(np.arange(7) / 8.0, (1000, 1)), targets=np.full(1000, 0.5))
    got = outputs(window_of([exact]).merged())                                   # dyadic inputs: the mean is the input
    assert got[1].tolist() == [0.5] and got[2][0].tolist() == (np.arange(7) / 8.0).tolist() and same(got, merge_host(*exact))


@pytest.fixture(scope="module")
def playout_rows():
    """4,097 positions from random playouts of 0..6 plies, in three segments, and what merge_host makes of them."""
    from connect4_amd.replay import merge_host
    pos = playouts(4097, 11)
    segs = [segment(pos[:1000], 1), segment(pos[1000:1003], 2), segment(pos[1003:], 3)]
    ref = {m: merge_host(*table_order(segs), mirror=m) for m in (True, False)}
    assert len(ref[True][3]) < len(ref[False][3]) < 3000 and int(ref[True][3].max()) > 64
    return segs, ref


@pytest.mark.parametrize("mirror", [True, False])
def test_random_playouts(playout_rows, mirror):
    from connect4_amd import _lib as L
    segs, ref = playout_rows
    w = window_of(segs)
    assert w.n_positions == 4097
    default = outputs(w.merged(mirror=mirror))
    assert same(default, ref[mirror])
    assert same(outputs(w.merged(mirror=mirror, log2_capacity=13)), ref[mirror])          # 8,192 slots: the smallest legal table
    assert same(outputs(w.merged(mirror=mirror)), default)                                  # the same merge twice
    for log2_capacity in (None, 13):
        for wave_combine in (False, True):
            assert same(raw_merge(w, mirror, log2_capacity, wave_combine)[0], ref[mirror]), (log2_capacity, wave_combine)
    with pytest.raises(L.EngineError, match="cannot hold 4097 positions"):
        w.merged(mirror=mirror, log2_capacity=12)
    with pytest.raises(L.EngineError):
        w.merged(mirror=mirror, log2_capacity=31)


def test_table_at_load_one():
    """4,096 distinct keys (mirror off: no two rows share one) in 4,096 slots: every slot is taken, probes wrap around."""
    pos, seed = [], 13
    while len(pos) < 4096:
        pos = list(dict.fromkeys(pos + playouts(1024, seed, max_plies=14)))[:4096]
        seed += 1
    got, ref = check([segment(pos, 1)], mirror=False, log2_capacity=12)
    assert got[3].tolist() == [1] * 4096
    mixed = pos[:2048] + pos[:2048]
    check([segment(mixed, 2)], mirror=True, log2_capacity=12)


def test_order_of_later_members_does_not_show(playout_rows):
    from connect4_amd.board import Board
    segs, ref = playout_rows
    data = table_order(segs)
    groups = {}
    for i, (c0, c1) in enumerate(data[0].view(np.uint64).tolist()):
        groups.setdefault(frozenset([(c0, c1), (Board.flip_color(c0), Board.flip_color(c1))]), []).append(i)
    rng = random.Random(3)
    perm = np.arange(4097)
    for g in groups.values():                   # rows move among the places of their own group's later members
        moved = g[1:]
        rng.shuffle(moved)
        perm[g[1:]] = moved
    assert int((perm != np.arange(4097)).sum()) > 2000
    moved = window_of([tuple(x[perm] for x in data)])
    assert same(outputs(moved.merged()), ref[True]) and same(raw_merge(moved, True, None, False)[0], ref[True])


def test_bad_rows_raise_and_are_counted():
    pos = playouts(300, 17)
    b, t, p = segment(pos, 1)
    ub = b.view(np.uint64)
    ub[5, 0] |= ub[5, 1] | np.uint64(1)                     # overlap (or a stone of o's where none was)
    ub[5, 1] |= np.uint64(1)
    ub[70] = (1 << 23, 1 << 21)                             # floating
    ub[131, 0] |= np.uint64(1 << 63)                        # outside the board
    t[200] = np.nan
    p[255, 3] = 1.5
    p[256, 0] = -1e-30
    p[299, 6] = np.inf
    w = window_of([(b, t, p), segment(pos[:40], 2)])
    with pytest.raises(ValueError, match="7 of 340 rows"):
        w.merged()
    with pytest.raises(ValueError, match="7 of 340 rows"):
        w.merged(mirror=False, log2_capacity=9)
    assert [raw_merge(w, True, None, wave_combine)[1] for wave_combine in (False, True)] == [7, 7]
    from connect4_amd.replay import ReplayWindow
    with pytest.raises(RuntimeError, match="empty"):
        ReplayWindow("cuda").merged()


def test_gather_and_train_on_the_merged_window():
    from connect4_amd.net import NetConfig
    from connect4_amd.replay import merge_host
    from connect4_amd.training import ModelConfig, Trainer
    segs = [segment(playouts(200, 21, max_plies=10), 1), segment(playouts(260, 22, max_plies=10), 2)]
    m = window_of(segs).merged()
    hb, ht, hp, hc = merge_host(*table_order(segs))
    host = window_of([(hb, ht, hp)], first_gen=2)
    assert 64 * 2 < m.n_positions == len(hc) < 460 and m.generations == host.generations == [2]
    idx = torch.randperm(m.rows, generator=torch.Generator().manual_seed(1)).cuda()
    assert same(m.gather(idx), host.gather(idx))
    torch.manual_seed(5)
    tr = Trainer(ModelConfig(net_config=NetConfig(n_residuals=1), batch_size=64, n_training_epochs=2), device="cuda")
    assert tr.use_graph and (m.rows // 64) * 2 >= 4                      # two eager full steps, then the captured one
    loss = tr.train_window(m)
    assert np.isfinite(float(loss))


def test_run_generations_trains_on_the_merged_window(tmp_path):
    from connect4_amd.config import MCTSConfig
    from connect4_amd.generation import run_generations
    from connect4_amd.training import ModelConfig, Trainer
    cfg = MCTSConfig.self_play(16)
    runs = {}
    for merge in (True, False):
        d = str(tmp_path / ("merged" if merge else "plain"))
        torch.manual_seed(0)
        tr = Trainer(ModelConfig(batch_size=256, n_training_epochs=2, use_gpu=True))
        seen, inner = [], tr.train_window

        def spy(window, generator=None, inner=inner, seen=seen):
            seen.append((window.n_positions, window.merged_from))
            return inner(window, generator)
        tr.train_window = spy
        timings = []
        window, losses = run_generations(tr, cfg, 48, d, 2, first_gen=1, n_slots=48, timings=timings, merge_duplicates=merge)
        assert len(losses) == 2 and all(np.isfinite(float(x)) for x in losses)
        runs[merge] = (d, timings, seen, window)
    d, timings, seen, window = runs[True]
    for t, (trained, merged_from) in zip(timings, seen):
        assert t["window_distinct"] == trained <= t["window_rows"] // 2 == merged_from and t["merge_s"] >= 0
        assert t["training_rows"] == 2 * trained
    assert timings[0]["window_distinct"] < timings[0]["positions"]         # 48 games share at least the empty board
    assert window.n_positions == timings[1]["window_rows"] // 2 and window.merged_from is None     # the kept window is unmerged
    assert all("window_distinct" not in t and "merge_s" not in t for t in runs[False][1])
    assert [s[1] for s in runs[False][2]] == [None, None]
    a = torch.load(os.path.join(d, "1", "data.pth"), weights_only=True)
    b = torch.load(os.path.join(runs[False][0], "1", "data.pth"), weights_only=True)
    assert set(a) == set(b) and all(same([a[k]], [b[k]]) for k in a)
