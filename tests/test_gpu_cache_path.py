"""The evaluation cache's memory path -- cache_probe / cache_insert of c4_engine.hip -- read back through
Engine.cache_lookup (k_cache_lookup: the very probe the tree waves run).

The probe asks for an entry's key + check word and for ONE payload word per lane (lane k < 7 its prior, lane 7 the value,
which reaches the other lanes inside the wave) in one round trip.  What must hold whatever the probe's instructions
are:

* a hit is the net's answer for that position -- c4_net_forward's bits, value and all seven priors; never one position's
  key with another's payload, never lane 7's word in a prior;
* the table is direct mapped: of the positions that hash to one entry at most one is found, and a miss next to a
  slot-mate that hits is a real absence -- the slot-mate's answer is its own;
* the fused kernel with a table plays the games of the host-driven path without one.

Runs: 40 games of 24 simulations on 35 slots, c4_selfplay_split_kernel<16,1,4,false> (16 slots per workgroup), the f32x3
net of tests/golden/net_golden.npz; a 2^8-entry table (thousands of insertions into 256 entries of 48 bytes: every entry
is overwritten many times, and an entry starts at each of the eight offsets 0, 48, 96, 16, 64, 112, 32, 80 of a 128-byte
line) and a 2^16-entry one.  Everything is exact; no tolerance anywhere."""
import ctypes as C
import os

import numpy as np
import pytest

import fused_matrix as fm
from conftest import load_npz

pytestmark = pytest.mark.gpu

N_SLOTS, SIMS, GAMES, RING = 35, 24, 40, 64
SEED = (1 << 33) + 13                  # the key's high word is set
KERNEL = "c4_selfplay_split_kernel<16,1,4,false>"
ENV = {"C4_FUSED_SLOTS": "16"}
M64 = (1 << 64) - 1
BOARD_BITS = 49                        # 7 columns x 7 bits


# ---------------------------------------------------------------- the table's addressing, on the host
def cache_key(c0, c1):
    return (int(c0) + (int(c0) | int(c1))) & M64


def cache_slot(key, bits):
    return ((key * 0x9E3779B97F4A7C15) & M64) >> (64 - bits)


def position_of_key(key):
    """The position a key denotes, or None.  Column by column key = stones of colour 0 + all stones = c + 2^h - 1 with
    c < 2^h, h <= 6: any 7-bit value but 127 is some column, so the key decodes without the board."""
    if key >> BOARD_BITS:
        return None
    c0 = c1 = 0
    for col in range(7):
        x = (key >> (7 * col)) & 0x7F
        if x == 127:
            return None
        h = (x + 1).bit_length() - 1
        occ = (1 << h) - 1
        a = x - occ
        c0 |= a << (7 * col)
        c1 |= (occ ^ a) << (7 * col)
    assert cache_key(c0, c1) == key
    return c0, c1


def test_key_decoding_is_the_inverse_of_the_key(oracle):
    """(host only in substance, but it guards the GPU checks below) random play: every position is what its key denotes."""
    rng = np.random.RandomState(5)
    seen = 0
    for _ in range(20):
        b = oracle.Board.empty()
        while b.result == oracle.NONE:
            m = b.valid_mask()
            b.make_move(int(rng.choice([c for c in range(7) if (m >> c) & 1])))
            assert position_of_key(cache_key(*b.key())) == b.key()
            seen += 1
    assert seen > 200
    assert position_of_key(127) is None and position_of_key(1 << BOARD_BITS) is None and position_of_key(0) == (0, 0)


# ---------------------------------------------------------------- runs
@pytest.fixture(scope="module")
def net():
    import torch
    from connect4_amd.fused_net import FusedNet
    z = load_npz("net_golden.npz")
    n = FusedNet({k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w__")}, precision="f32x3")
    assert n.precision == "f32x3"
    yield n
    n.close()


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64).tolist()


def games_of(recs):
    return [(r.game_id, r.length, r.result, list(r.move[:r.length]), list(r.color0[:r.length]), list(r.color1[:r.length]),
             _bits(list(r.value[:r.length])), np.asarray([list(p) for p in r.policy[:r.length]], dtype=np.float64).tobytes()) for r in recs]


def new_selfplay(net, fused, cache_bits):
    from connect4_amd.config import MCTSConfig
    from connect4_amd.selfplay import SelfPlay
    return SelfPlay(net, N_SLOTS, MCTSConfig.self_play(SIMS), seed=SEED, games_target=GAMES, record_capacity_games=RING,
                    use_graph=False, fused_loop=fused, steps_per_launch=16, eval_cache_log2_entries=cache_bits)


def play_out(sp, steps=None):
    """Runs sp to the end of its games: (games in comparable form, statistics).  `steps`: what advances it by k steps."""
    steps = steps or sp.run_steps
    for _ in range(4000):
        steps(64)
        st = sp.stats()
        if st["active_slots"] == 0:
            break
    assert st["active_slots"] == 0 and st["games_finished"] == GAMES
    assert st["bad_evals"] == 0 and st["dropped_games"] == 0
    recs = sorted(sp.engine.drain_games(), key=lambda r: r.game_id)
    assert [r.game_id for r in recs] == list(range(GAMES))
    return games_of(recs), st


def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def fused_env(monkeypatch):
    for k in fm.ENV_VARS:
        monkeypatch.delenv(k, raising=False)
    for k, v in ENV.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("C4_FUSED_PACK", "dense")
    expect = fm.reported("selfplay", "f32x3", N_SLOTS, ENV, cus(), pack_dense=True)
    assert expect.startswith(KERNEL + " spread=0 grid=3")
    return expect


@pytest.fixture(scope="module")
def reference(net):
    """The host-driven path (c4_step + c4_net_forward, eager, one stream) with the cache off."""
    sp = new_selfplay(net, False, -1)
    try:
        games, st = play_out(sp)
    finally:
        sp.close()
    assert st["eval_cache_probes"] == 0 and st["leaf_evals"] > 0
    assert len({tuple(g[3]) for g in games}) >= 30, "the reference's games are too much alike"
    return games


def assert_same_games(games, reference):
    for mine, want in zip(games, reference):
        assert mine[3] == want[3], "game %d: moves differ from the host-driven path's" % want[0]
        assert mine == want, "game %d: values, policies, boards or result differ from the host-driven path's" % want[0]


def lookup_set(games):
    """Every recorded position (the root of a search) and the children of each, without repeats."""
    from connect4_amd.engine import board_make_move, board_valid_mask
    r0 = np.array([c for g in games for c in g[4]], dtype=np.uint64)
    r1 = np.array([c for g in games for c in g[5]], dtype=np.uint64)
    mask = board_valid_mask(r0, r1)
    pos = set(zip(r0.tolist(), r1.tolist()))
    n_roots = len(pos)
    for col in range(7):
        ok = ((mask >> col) & 1).astype(bool)
        k0, k1, _ = board_make_move(r0[ok], r1[ok], np.full(int(ok.sum()), col, dtype=np.int32))
        pos.update(zip(k0.tolist(), k1.tolist()))
    pos = sorted(pos)
    return np.array([p[0] for p in pos], dtype=np.uint64), np.array([p[1] for p in pos], dtype=np.uint64), n_roots


def assert_hits_are_the_nets_answers(net, c0, c1, v, p, found, what):
    if not found.any():
        return
    nv, npri = net.evaluate_bits(c0[found], c1[found])
    assert nv.dtype == np.float32 and npri.dtype == np.float32 and v.dtype == np.float32 and p.dtype == np.float32
    bad_v = np.flatnonzero(nv.view(np.uint32) != v[found].view(np.uint32))
    bad_p = np.flatnonzero((npri.view(np.uint32) != p[found].view(np.uint32)).any(axis=1))
    assert len(bad_v) == 0, "%s: %d of %d hits carry a value that is not c4_net_forward's (first: position %d)" % (
        what, len(bad_v), int(found.sum()), int(np.flatnonzero(found)[bad_v[0]]))
    assert len(bad_p) == 0, "%s: %d of %d hits carry priors that are not c4_net_forward's (first: position %d)" % (
        what, len(bad_p), int(found.sum()), int(np.flatnonzero(found)[bad_p[0]]))


@pytest.mark.parametrize("cache_bits", [8, 16])
def test_table_answers_with_the_nets_bits_or_not_at_all(monkeypatch, net, reference, cache_bits):
    expect = fused_env(monkeypatch)
    sp = new_selfplay(net, True, cache_bits)
    try:
        # ---- nothing was inserted yet: the empty board (key 0, entry 0 of a table filled with 0xFF) and others miss
        e0 = np.array([0, 1, 1 << 21, 0], dtype=np.uint64), np.array([0, 0, 1, 1 << 21], dtype=np.uint64)
        assert not sp.engine.cache_lookup(*e0)[2].any(), "an untouched table reports a hit"
        games, st = play_out(sp)
        assert sp.engine.last_fused_kernel() == expect
        assert_same_games(games, reference)
        assert st["eval_cache_probes"] > 0 and st["eval_cache_hits"] > 0
        inserted = st["leaf_evals"] - st["eval_cache_hits"] + st["speculative_evals"]

        # ---- every recorded position and the roots' children
        c0, c1, n_roots = lookup_set(games)
        v, p, found = sp.engine.cache_lookup(c0, c1)
        assert_hits_are_the_nets_answers(net, c0, c1, v, p, found, "2^%d entries" % cache_bits)
        assert not v[~found].any() and not p[~found].any()
        keys = [cache_key(a, b) for a, b in zip(c0.tolist(), c1.tolist())]
        assert len(set(keys)) == len(keys), "two positions share a key"
        slots = np.array([cache_slot(k, cache_bits) for k in keys])
        hit_slots = slots[found]
        # Direct mapped: an entry holds one position.  A miss whose slot-mate hits is therefore a real absence -- the entry is
        # the slot-mate's, whose answer was checked above against ITS net answer (a mix of the two positions' words would have
        # failed there or in the check word).  That no two slot-mates are BOTH found is printed, not asserted: the table is
        # read and written without a coherence qualifier (a stale view costs a repeated evaluation, never a wrong answer), and
        # one of the 16 runs of the 2^8 table made on an MI355X while this file was written did report two slot-mates, each with
        # its own net answer (profiles/README.md, "The tree wave's memory path").
        shared = len(hit_slots) - len(set(hit_slots.tolist()))
        evicted = int((~found & np.isin(slots, hit_slots)).sum())
        unknown = int((~found).sum()) - evicted          # the entry is empty, or holds a position deeper in some tree
        phases = sorted({int(s) % 8 for s in hit_slots.tolist()})
        print("2^%d entries: %d insertions; %d positions looked up (%d roots): %d hits in %d entries at line phases %s, %d misses "
              "next to a slot-mate that hits, %d other misses, %d hits share an entry with another hit" % (
                  cache_bits, inserted, len(c0), n_roots, int(found.sum()), len(set(hit_slots.tolist())), phases, evicted, unknown, shared))
        assert phases == list(range(8)), "not every offset of an entry inside a 128-byte line was read"
        roots = {(a, b) for g in games for a, b in zip(g[4], g[5])}
        is_root = np.array([(a, b) in roots for a, b in zip(c0.tolist(), c1.tolist())])
        assert is_root.sum() == n_roots
        if cache_bits == 8:
            # more than 16 insertions per entry, and every root was inserted (a search starts with its root's evaluation,
            # or with a hit on it): all but 256 of them at the most have been overwritten, many next to a known occupant
            assert inserted > 16 * 256 and n_roots > 2 * 256
            assert 1 <= found.sum() <= 256 and (is_root & ~found).sum() >= n_roots - 256 and evicted >= 1
        else:
            # a given root was overwritten by one of the later insertions with probability 1 - (1 - 2^-16)^later <= p =
            # insertions / 2^16; the share of roots gone then has a standard deviation of about sqrt(p (1 - p) / roots), under
            # 0.02 for 800 roots, so p + 0.1 leaves five of them
            p_gone = inserted / float(1 << 16)
            assert p_gone < 0.25 and n_roots >= 600
            assert found[is_root].sum() >= (1.0 - p_gone - 0.1) * n_roots

        # ---- keys one bit away from a stored key: the key (0, t) has key t.  Bits 49..63 denote no position at all; a low bit
        # may lead to another real position's key (a child differs from its parent in one bit of the key when nothing carries),
        # so a hit is legitimate exactly when it is the net's answer for the position its key denotes.
        stored = [k for k, f in zip(keys, found.tolist()) if f][:64]
        t = np.array([k ^ (1 << b) for k in stored for b in range(64)], dtype=np.uint64)
        tv, tp, tf = sp.engine.cache_lookup(np.zeros(len(t), dtype=np.uint64), t)
        high = np.tile(np.arange(64) >= BOARD_BITS, len(stored))
        assert not tf[high].any(), "a key that differs from a stored key in a bit above the board's was found"
        denoted = [position_of_key(int(k)) for k in t[tf].tolist()]
        assert all(d is not None for d in denoted), "a hit for a key that denotes no position"
        if denoted:
            d0 = np.array([d[0] for d in denoted], dtype=np.uint64)
            d1 = np.array([d[1] for d in denoted], dtype=np.uint64)
            assert_hits_are_the_nets_answers(net, d0, d1, tv[tf], tp[tf], np.ones(len(d0), dtype=bool), "one bit away")
        print("one bit away from %d stored keys: %d of %d looked up are other stored positions" % (len(stored), int(tf.sum()), len(t)))
        assert tf.sum() <= len(t) // 8
    finally:
        sp.close()


def _other_library():
    """C4_ENGINE_LIB_PARENT: another build of the engine with the same ABI and the same host structures (the parent commit's,
    when this file's commit changed device code only), bound like connect4_amd._lib binds its own."""
    from connect4_amd import _lib as L
    path = os.environ.get("C4_ENGINE_LIB_PARENT")
    if not path:
        return None
    lib = C.CDLL(os.path.abspath(path))
    for name in ("c4_abi_version", "c4_selfplay_steps"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = L.SIGNATURES[name]
    assert lib.c4_abi_version() == L.ABI_VERSION
    return lib


@pytest.mark.parametrize("cache_bits", [8, 16])
def test_a_table_written_by_the_other_library_reads_the_same(monkeypatch, net, reference, cache_bits):
    """Entries written by one build's cache_insert are read by the other's cache_probe, in both directions: the games are
    played once by the other library's kernel on this library's engine (c4_reset keeps the table), then again by this
    library's on the table the other one left, and the other way round.  All four runs are the reference's games."""
    import torch
    from connect4_amd import _lib as L
    other = _other_library()
    if other is None:
        pytest.skip("C4_ENGINE_LIB_PARENT names no other build of the engine")
    fused_env(monkeypatch)

    def stepper(sp, lib):
        def steps(k):
            stream = torch.cuda.current_stream(sp.device).cuda_stream
            sp.engine.set_stream(stream)
            while k > 0:
                n = min(k, 16)
                L.check(lib.c4_selfplay_steps(sp.engine._h, sp.net._h, C.c_void_p(sp.values.data_ptr()),
                                              C.c_void_p(sp.priors.data_ptr()), n, C.c_void_p(stream)), sp.engine._h)
                k -= n
        return steps

    for first, second in ((other, L.load()), (L.load(), other)):
        sp = new_selfplay(net, True, cache_bits)
        try:
            games, st1 = play_out(sp, stepper(sp, first))
            assert_same_games(games, reference)
            sp.engine.reset()
            games, st2 = play_out(sp, stepper(sp, second))
            assert_same_games(games, reference)
            # (c4_reset zeroes the counters) the same games make the same probes; where nearly nothing is overwritten the
            # second run finds what the first one left and misses less
            assert st2["eval_cache_probes"] == st1["eval_cache_probes"]
            if cache_bits == 16:
                assert st2["eval_cache_hits"] > st1["eval_cache_hits"]
        finally:
            sp.close()
