"""Host model of the engine's PRODUCTION random streams (C4_RNG_PHILOX) -- TEST INFRASTRUCTURE ONLY (tests/ import
this; connect4_amd/ never does).

Operation for operation it is rng_uniform2 / rng_gamma of connect4_amd/csrc/c4_engine.hip:

- philox4x32_10(ctr, key): Philox4x32-10 (Salmon et al. 2011), multipliers 0xD2511F53 / 0xCD9E8D57, Weyl key bumps
  0x9E3779B9 / 0xBB67AE85;
- uniform2(seed, gid, ply, stream, idx): one Philox block on the counter {gid lo, gid hi, ply*64 + stream, idx} keyed by
  the 64-bit seed; u = (hi:lo >> 11) * 2^-53 for each 64-bit half of the block;
- gamma(seed, gid, ply, stream, alpha): Marsaglia-Tsang with the alpha < 1 boost u0^(1/alpha), at most 24 rounds, the
  1e-300 guards in front of log / pow and the fallback boost*dd.

The stream numbers: root noise uses stream = the column (0..6), the opening-move uniform is stream 32, idx 0 (u0).

The integer part is exact (uint64 arithmetic, masked to 32 bits).  The floating-point part follows the C's operation order
exactly (the library is built with -ffp-contract=off: no fused multiply-adds), and every transcendental goes through
Python's math module, i.e. the host C library -- the vectorised functions evaluate them element by element for that reason,
so they equal the scalar ones bit for bit on any CPU.  The device's log / cos / pow are ocml's; how close those are to the
host's is what tests/test_gpu_rng.py measures.
"""
import math

import numpy as np

M32 = np.uint64(0xFFFFFFFF)
_MUL0, _MUL1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_BUMP0, _BUMP1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_TWO_M53 = 1.0 / 9007199254740992.0
NOISE_STREAMS = 7           # root noise: stream = column
MOVE_STREAM = 32            # opening-move uniform
MAX_ROUNDS = 24             # Marsaglia-Tsang rounds before the fallback


def _u64(x):
    return np.asarray(x).astype(np.uint64)


def philox4x32_10(ctr, key):
    """ctr: 4 arrays (or ints) of 32-bit words, key: 2.  Returns the 4 output words as uint64 arrays (< 2^32)."""
    c0, c1, c2, c3 = (_u64(c) & M32 for c in ctr)
    k0, k1 = (_u64(k) & M32 for k in key)
    for _ in range(10):
        p0 = _MUL0 * c0
        p1 = _MUL1 * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32)
        k0 = (k0 + _BUMP0) & M32
        k1 = (k1 + _BUMP1) & M32
    return c0, c1, c2, c3


def _split_seed(seed):
    s = _u64(seed)
    return s & M32, s >> np.uint64(32)


def uniform2(seed, gid, ply, stream, idx):
    """The pair (u0, u1) of float64 arrays in [0, 1) that rng_uniform2 returns; arguments broadcast."""
    g = np.asarray(gid, dtype=np.int64).astype(np.uint64)
    ctr = (g & M32, g >> np.uint64(32), (_u64(ply) * np.uint64(64) + _u64(stream)) & M32, _u64(idx))
    c0, c1, c2, c3 = philox4x32_10(ctr, _split_seed(seed))
    s11 = np.uint64(11)
    u0 = (((c0 << np.uint64(32)) | c1) >> s11).astype(np.float64) * _TWO_M53
    u1 = (((c2 << np.uint64(32)) | c3) >> s11).astype(np.float64) * _TWO_M53
    return u0, u1


def _each(fn, x):
    """Host libm, element by element (see the module docstring)."""
    x = np.asarray(x, dtype=np.float64)
    return np.fromiter(map(fn, x.ravel().tolist()), dtype=np.float64, count=x.size).reshape(x.shape)


def gamma_with_round(seed, gid, ply, stream, alpha):
    """rng_gamma for every key (arguments broadcast; alpha is a scalar).  Returns (draws float64, round int32): the
    Marsaglia-Tsang round that accepted (1..24; 0 = none did, the fallback boost*dd), negated when the second, log-based
    test accepted -- so two sides that disagree can say which branch each took."""
    seed, gid, ply, stream = np.broadcast_arrays(*(np.asarray(a) for a in (seed, gid, ply, stream)))
    shape = gid.shape
    seed, gid, ply, stream = (a.reshape(-1) for a in (seed, gid, ply, stream))
    n = gid.size
    alpha = float(alpha)
    u0, _ = uniform2(seed, gid, ply, stream, 0)
    boost = np.ones(n)
    if alpha < 1.0:
        y = 1.0 / alpha
        boost = _each(lambda u: math.pow(u if u > 0.0 else 1e-300, y), u0)
        alpha += 1.0
    dd = alpha - 1.0 / 3.0
    cc = 1.0 / math.sqrt(9.0 * dd)
    out = boost * dd                                  # the fallback, overwritten where a round accepts
    rnd = np.zeros(n, dtype=np.int32)
    live = np.arange(n)
    for it in range(1, MAX_ROUNDS + 1):
        if live.size == 0:
            break
        s, g, p, st = seed[live], gid[live], ply[live], stream[live]
        a, b = uniform2(s, g, p, st, 2 * it)
        uu, _ = uniform2(s, g, p, st, 2 * it + 1)
        la = _each(lambda t: math.log(t if t > 0.0 else 1e-300), a)
        x = np.sqrt(-2.0 * la) * _each(math.cos, 6.283185307179586 * b)
        v = 1.0 + cc * x
        ok = v > 0.0
        v = v * v * v
        acc1 = ok & (uu < 1.0 - 0.0331 * x * x * x * x)
        rest = ok & ~acc1
        acc2 = np.zeros_like(ok)
        if rest.any():
            r = np.nonzero(rest)[0]
            lu = _each(lambda t: math.log(t if t > 0.0 else 1e-300), uu[r])
            xr, vr = x[r], v[r]
            acc2[r] = lu < 0.5 * xr * xr + dd * (1.0 - vr + _each(math.log, vr))
        done = acc1 | acc2
        k = live[done]
        out[k] = boost[k] * dd * v[done]
        rnd[k] = np.where(acc1[done], it, -it)
        live = live[~done]
    return out.reshape(shape), rnd.reshape(shape)


def gamma(seed, gid, ply, stream, alpha):
    """rng_gamma (float64 array)."""
    return gamma_with_round(seed, gid, ply, stream, alpha)[0]


def production_tapes(seed, alpha, gids):
    """The tapes a C4_RNG_PHILOX engine with this seed effectively plays game ids `gids` with: (noise[len(gids)][42][7]
    raw Gamma(alpha) draws, u[len(gids)][42] opening-move uniforms) -- the formats c4_set_tapes and c4o_replay_new take."""
    g = np.asarray(gids, dtype=np.int64).reshape(-1, 1, 1)
    ply = np.arange(42, dtype=np.int64).reshape(1, 42, 1)
    col = np.arange(NOISE_STREAMS, dtype=np.int64).reshape(1, 1, NOISE_STREAMS)
    noise = gamma(seed, g, ply, col, alpha)
    u, _ = uniform2(seed, g[:, :, 0], ply[:, :, 0], MOVE_STREAM, 0)
    return noise, u


# -- a scalar transliteration (pure Python ints and floats), the cross-check for the vectorised model ---------------
def philox4x32_10_scalar(ctr, key):
    c = [int(x) & 0xFFFFFFFF for x in ctr]
    k = [int(x) & 0xFFFFFFFF for x in key]
    for _ in range(10):
        p0 = 0xD2511F53 * c[0]
        p1 = 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


def uniform2_scalar(seed, gid, ply, stream, idx):
    seed &= 0xFFFFFFFFFFFFFFFF
    gid &= 0xFFFFFFFFFFFFFFFF
    c = philox4x32_10_scalar([gid & 0xFFFFFFFF, gid >> 32, (ply * 64 + stream) & 0xFFFFFFFF, idx],
                             [seed & 0xFFFFFFFF, seed >> 32])
    return (((c[0] << 32) | c[1]) >> 11) * _TWO_M53, (((c[2] << 32) | c[3]) >> 11) * _TWO_M53


def gamma_scalar(seed, gid, ply, stream, alpha):
    u0, _ = uniform2_scalar(seed, gid, ply, stream, 0)
    boost = 1.0
    if alpha < 1.0:
        boost = math.pow(u0 if u0 > 0.0 else 1e-300, 1.0 / alpha)
        alpha += 1.0
    dd = alpha - 1.0 / 3.0
    cc = 1.0 / math.sqrt(9.0 * dd)
    for it in range(1, MAX_ROUNDS + 1):
        a, b = uniform2_scalar(seed, gid, ply, stream, 2 * it)
        uu, _ = uniform2_scalar(seed, gid, ply, stream, 2 * it + 1)
        x = math.sqrt(-2.0 * math.log(a if a > 0.0 else 1e-300)) * math.cos(6.283185307179586 * b)
        v = 1.0 + cc * x
        if v <= 0.0:
            continue
        v = v * v * v
        if uu < 1.0 - 0.0331 * x * x * x * x:
            return boost * dd * v
        if math.log(uu if uu > 0.0 else 1e-300) < 0.5 * x * x + dd * (1.0 - v + math.log(v)):
            return boost * dd * v
    return boost * dd


def gamma_round_values_scalar(seed, gid, ply, stream, alpha):
    """Diagnostics for a draw two sides disagree on: {round: (value that round returns if it accepts, branch)} for every
    round with v > 0 -- branch 1 or 2 is the test that accepts it here, 0 neither -- and {0: (fallback, 0)}."""
    u0, _ = uniform2_scalar(seed, gid, ply, stream, 0)
    boost = 1.0
    if alpha < 1.0:
        boost = math.pow(u0 if u0 > 0.0 else 1e-300, 1.0 / alpha)
        alpha += 1.0
    dd = alpha - 1.0 / 3.0
    cc = 1.0 / math.sqrt(9.0 * dd)
    out = {0: (boost * dd, 0)}
    for it in range(1, MAX_ROUNDS + 1):
        a, b = uniform2_scalar(seed, gid, ply, stream, 2 * it)
        uu, _ = uniform2_scalar(seed, gid, ply, stream, 2 * it + 1)
        x = math.sqrt(-2.0 * math.log(a if a > 0.0 else 1e-300)) * math.cos(6.283185307179586 * b)
        v = 1.0 + cc * x
        if v <= 0.0:
            continue
        v = v * v * v
        branch = 1 if uu < 1.0 - 0.0331 * x * x * x * x else (
            2 if math.log(uu if uu > 0.0 else 1e-300) < 0.5 * x * x + dd * (1.0 - v + math.log(v)) else 0)
        out[it] = (boost * dd * v, branch)
    return out
