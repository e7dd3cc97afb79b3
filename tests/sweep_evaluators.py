"""Synthetic evaluators for the search sweep: deterministic functions (color0, color1) -> (value, prior[7]).

Pure Python + NumPy, integer arithmetic on the two bitboards only (a 64-bit mix of the key), and every output is
exactly representable in its dtype, so the same bits come out under any NumPy version on any machine.  Priors are
left UNNORMALISED (small integers): the normalisation over the legal columns (mcts.py:124-135, 197-202) is part of what
the sweep tests.  Values of the float32 kinds are float32-representable (they travel through a float32 buffer).

  const32   value 0.5, prior seven float32 ones: every score ties
  quant32   value k/8 (k in 0..8: 0.0 and 1.0 occur), prior entries integers 1..4 as float32
  quant64   the same in float64
  sparse32  value float32(k)/float32(15), prior entries from {0, 1, 16, 4096} as float32; at least one positive entry
            on a legal column by construction; zeros on legal columns and mass on illegal ones both occur
  sparse64  value k/15 in float64, prior as sparse32 in float64
"""
import numpy as np

M64 = (1 << 64) - 1
WIDTH, HEIGHT, H1 = 7, 6, 7

KINDS = ("const32", "quant32", "quant64", "sparse32", "sparse64")


def mix64(c0, c1, salt=0):
    """A 64-bit mix of the position key (splitmix64's finaliser over a multiplicative combination)."""
    x = (int(c0) * 0x9E3779B97F4A7C15 + int(c1) * 0xC2B2AE3D27D4EB4F + (salt + 1) * 0x165667B19E3779F9) & M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x


def legal_columns(c0, c1):
    occ = int(c0) | int(c1)
    return [c for c in range(WIDTH) if bin((occ >> (H1 * c)) & 0x3F).count("1") < HEIGHT]


def dtype_of(kind):
    return np.float32 if kind.endswith("32") else np.float64


def _const(c0, c1, dtype):
    return 0.5, np.ones(WIDTH, dtype=dtype)


def _quant(c0, c1, dtype):
    h = mix64(c0, c1, 1)
    value = (h % 9) / 8.0
    h >>= 8
    prior = np.array([1 + ((h >> (2 * c)) & 3) for c in range(WIDTH)], dtype=dtype)
    return value, prior


_SPARSE = (0, 0, 1, 16, 4096, 0, 1, 4096)   # half of the draws are zero


def _sparse(c0, c1, dtype):
    h = mix64(c0, c1, 2)
    k = h % 16
    value = float(np.float32(k) / np.float32(15)) if dtype == np.float32 else k / 15.0
    h >>= 8
    ints = [_SPARSE[(h >> (3 * c)) & 7] for c in range(WIDTH)]
    h >>= 24
    legal = legal_columns(c0, c1)
    if legal:           # one legal column always carries mass: chosen from the key, its mass from {1, 16, 4096}
        keep = legal[h % len(legal)]
        if ints[keep] == 0:
            ints[keep] = (1, 16, 4096)[(h >> 8) % 3]
    return value, np.array(ints, dtype=dtype)


def evaluate(kind, c0, c1):
    """(value as a Python float, prior as a fresh NumPy array of the kind's dtype)."""
    dt = dtype_of(kind)
    if kind.startswith("const"):
        return _const(c0, c1, dt)
    if kind.startswith("quant"):
        return _quant(c0, c1, dt)
    if kind.startswith("sparse"):
        return _sparse(c0, c1, dt)
    raise ValueError("unknown evaluator kind %r" % (kind,))


def make(kind):
    """fn(c0, c1) -> (value, prior[7])."""
    if kind not in KINDS:
        raise ValueError("unknown evaluator kind %r" % (kind,))
    return lambda c0, c1: evaluate(kind, c0, c1)


def output_bits(kind, c0, c1):
    """The answer as integers: the value's float64 bits and the prior's bits in its own dtype."""
    v, p = evaluate(kind, c0, c1)
    vb = int(np.array([v], dtype=np.float64).view(np.uint64)[0])
    pb = p.view(np.uint32 if p.dtype == np.float32 else np.uint64).tolist()
    return vb, [int(x) for x in pb]
