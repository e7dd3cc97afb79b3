"""The host model of the production random streams (oracle/philox_ref.py) on its own, no GPU: Philox4x32-10 known-answer
vectors (Random123's), the vectorised model against a scalar pure-Python transliteration of c4_engine.hip's rng_uniform2 /
rng_gamma on keys that reach every part of the counter (gid >= 2^32, seeds with the high word set, ply 41, stream 32) and
every branch of the Gamma draw (alpha < 1 with the boost, alpha = 1 without it, alpha > 1), and a moment check.
tests/test_gpu_rng.py ties the model to the device's read-outs."""
import numpy as np
import pytest

from oracle import philox_ref as R

KAT = [  # (counter, key, Philox4x32-10 output)
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]
ALPHAS = [0.03, 0.3, 1.0, 2.5]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox4x32_10_known_answers(ctr, key, want):
    assert [int(x) for x in R.philox4x32_10(ctr, key)] == list(want)
    assert R.philox4x32_10_scalar(ctr, key) == list(want)


def test_philox_vectorised_over_many_counters_equals_scalar():
    rng = np.random.RandomState(0)
    ctr = rng.randint(0, 1 << 32, size=(4, 300), dtype=np.uint64)
    key = rng.randint(0, 1 << 32, size=(2, 300), dtype=np.uint64)
    out = np.stack(R.philox4x32_10(ctr, key))
    for j in range(300):
        assert list(out[:, j]) == R.philox4x32_10_scalar(ctr[:, j], key[:, j])


def _keys(n, seed):
    """(seed, gid, ply, stream) keys that set every word of the counter and the key."""
    rng = np.random.RandomState(seed)
    seeds = rng.randint(0, 1 << 62, size=n, dtype=np.uint64) * np.uint64(3)     # high words set, some above 2^63
    seeds[:4] = [0, 1, (1 << 32) + 5, (1 << 64) - 1]
    gid = rng.randint(0, 1 << 40, size=n).astype(np.int64)
    gid[:6] = [0, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 40) + 7, (1 << 62) + 3]
    ply = rng.randint(0, 42, size=n).astype(np.int64)
    ply[::7] = 41
    stream = rng.randint(0, 7, size=n).astype(np.int64)
    stream[::5] = R.MOVE_STREAM
    return seeds, gid, ply, stream


def test_uniform2_vectorised_equals_scalar():
    seeds, gid, ply, stream = _keys(400, 1)
    assert seeds.max() >= np.uint64(1 << 63) and gid.max() >= 1 << 32 and ply.max() == 41 and stream.max() == R.MOVE_STREAM
    for idx in (0, 1, 48, 49):
        u0, u1 = R.uniform2(seeds, gid, ply, stream, idx)
        for j in range(len(gid)):
            assert (u0[j], u1[j]) == R.uniform2_scalar(int(seeds[j]), int(gid[j]), int(ply[j]), int(stream[j]), idx)
    assert np.all((u0 >= 0) & (u0 < 1)) and np.all((u1 >= 0) & (u1 < 1))


def test_uniform2_counter_words_all_matter():
    """Each input reaches the block: gid's high word, ply vs stream (ply*64 + stream), the seed's high word, idx."""
    base = R.uniform2_scalar(5, 3, 2, 1, 0)
    for other in (R.uniform2_scalar(5, 3 + (1 << 32), 2, 1, 0), R.uniform2_scalar(5, 3, 3, 1, 0), R.uniform2_scalar(5, 3, 2, 2, 0),
                  R.uniform2_scalar(5, 3, 2, 1, 1), R.uniform2_scalar(5 + (1 << 32), 3, 2, 1, 0)):
        assert other[0] != base[0] and other[1] != base[1]
    # the counter's third word is ply*64 + stream: (ply, stream + 64) is (ply + 1, stream)
    assert R.uniform2_scalar(5, 3, 2, 65, 0) == R.uniform2_scalar(5, 3, 3, 1, 0)


@pytest.mark.parametrize("alpha", ALPHAS)
def test_gamma_vectorised_equals_scalar(alpha):
    seeds, gid, ply, stream = _keys(300, 2)
    g, rnd = R.gamma_with_round(seeds, gid, ply, stream, alpha)
    want = np.array([R.gamma_scalar(int(s), int(a), int(p), int(c), alpha) for s, a, p, c in zip(seeds, gid, ply, stream)])
    assert np.array_equal(g.view(np.uint64), want.view(np.uint64))
    assert np.all(g >= 0) and np.all(np.isfinite(g)) and np.all(rnd != 0)
    if alpha < 1.0:        # the boost u0^(1/alpha): at alpha = 0.03 it reaches far down (denormals need u0 < 6e-10: no sample here)
        assert g.min() < (1e-50 if alpha == 0.03 else 1e-3)
    assert (rnd < 0).any()      # the second, log-based acceptance test is reached too


def test_production_tapes_layout():
    gids = np.array([0, 5, (1 << 32) + 9])
    noise, u = R.production_tapes((1 << 40) + 17, 0.3, gids)
    assert noise.shape == (3, 42, 7) and u.shape == (3, 42)
    for i, g in enumerate(gids.tolist()):
        for ply in (0, 17, 41):
            assert u[i, ply] == R.uniform2_scalar((1 << 40) + 17, g, ply, R.MOVE_STREAM, 0)[0]
            for col in (0, 6):
                assert noise[i, ply, col] == R.gamma_scalar((1 << 40) + 17, g, ply, col, 0.3)


def test_gamma_moments():
    n = 100_000
    a = 0.3
    g = R.gamma(123, np.arange(n) // 7, (np.arange(n) // 3) % 42, np.arange(n) % 7, a)
    assert abs(g.mean() - a) < 5 * np.sqrt(a / n)
    assert abs(g.var() - a) < 5 * np.sqrt((6 * a + 2 * a ** 2) / n)
