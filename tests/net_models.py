"""Independent models of the fused network forwards (csrc/c4_net.hip, c4_net_dev.h) for the tests.

* stressed_state_dict -- a seeded net of the reference architecture in which every term matters: per-channel batch-norm
  statistics, non-zero biases everywhere, activations O(1) through 16 residual blocks, heads whose answers vary strongly
  from position to position, value_head.w1 / w2 away from 1 / 0.5.
* float64_outputs -- PolicyValueNet in float64 on host-built planes (Board.to_array): no code of the fused path (no
  BatchNorm folding, no collapsed Linear stack, no device plane builder).  Pinned to the reference's own outputs by
  test_net.py::test_trainable_net_matches_reference_checkpoint and test_net_models.py.
* desc_outputs / fp16_storage_outputs -- float64 evaluation of the folded arrays of c4_net_desc (include/c4_engine.h),
  optionally rounded to fp16 exactly where the kernels store fp16.
* position sets: seeded legal positions over every ply, the empty board, boards with full columns, full boards.
"""
import numpy as np
import torch
import torch.nn.functional as F

from connect4_amd.board import Board
from connect4_amd.net import NetConfig, PolicyValueNet

LEAK = 0.01

# (filters, residual blocks, value-head Linear layers, precisions) of the float64 tests
GRID = [(32, 0, 1, ("f32x3", "f16")), (32, 1, 3, ("f32x3", "f16")), (32, 2, 0, ("f32x3", "f16")),
        (32, 5, 1, ("f32x3", "f16")), (32, 16, 3, ("f32x3", "f16")),
        (64, 0, 6, ("f16",)), (64, 1, 0, ("f16",)), (64, 7, 6, ("f16",))]


def tol_f32x3(n_res: int) -> float:
    """|f32x3 kernel - float64_outputs|, fixed before the first run on the device.  Every operand (folded weight,
    activation) is hi + lo / 2^11 in fp16: relative error 2^-22 per operand after the float32 rounding of the fold;
    products are exact, sums fp32 (2^-24 per add).  A layer therefore adds ~2 x 2^-22 relative error to activations of
    O(1) (the stressed nets keep them below 12), the tower passes it on with a gain of O(1), and the 2R + 3 layers that
    store activations (stem, 2R tower convs, heads as operands) add up linearly in the worst case.  The stressed nets'
    heads map an activation error to the outputs with a gain measured at <= 8 on the host (an fp32 plan of the same nets
    is off by 1.2e-6 .. 7e-6).  Bound: 16 x (2R + 3) x 2^-22 = 3.8e-6 per layer (1.1e-5 at 0 blocks, 3.4e-5 at 3)."""
    return 16 * (2 * n_res + 3) * 2.0 ** -22


def per_position_error(a, b):
    """max over a position's value and 7 priors of |a - b|, for (values, priors) pairs: [n]."""
    return np.maximum(np.abs(a[0] - b[0]), np.abs(a[1] - b[1]).max(1))


def f16_tolerances(folded, planes):
    """(max, mean) tolerances of |fp16-storage kernel - fp16_storage_outputs| per position.  The model rounds where the
    kernel rounds; what differs is the fp32 sums: now and then an fp32 accumulator lands on the other side of an fp16
    rounding boundary than the exact sum, the stored activation moves by one fp16 ulp (2^-11 relative), and the tower
    carries that on (the stressed heads turn one such flip into up to ~3e-4 on an output).  Any fp32-accumulating
    implementation of the same storage arithmetic shows this noise; the kernel sums in another order than the host, so it
    flips other roundings, but about as often and as far.  So the host's fp32-accumulating copy of the model
    (desc_outputs(acc32=True)) is compared with the model, and the kernel may differ by at most
      max:  3x that copy's largest difference + 1e-5,
      mean: 1.5x that copy's mean difference + 4e-5.
    1e-5 covers the fp32 sums of the heads and MLPs; without residual blocks nothing flips (the stem's 0/1 x fp16 sums
    are exact in fp32), so there the max bound is 1e-5 (measured 3e-7 / 1.3e-6 at 32 / 64 filters).
    History, with measurements on MI355X over the grid's 1,023 positions.  First run: 3e-4 x sqrt(2R + 3), exceeded at 16
    blocks (4.9e-3) and 64 filters / 7 blocks (3.1e-3): flips are larger and more frequent than that assumed.  Second run:
    2x the copy's max + 1e-5 and 1.5x its mean + 1e-5, the form above, exceeded twice where flips are RARE, so that a few
    events decide the statistic: the 1-block net's mean (2.1e-5 against the copy's 5.8e-6; at 2 .. 16 blocks the kernel's
    mean is 0.8 .. 1.0x the copy's) and, in the dynamic-range sweep over 300 positions, the 1-block 64-filter net's max
    at one scale (1.1e-4 against 2x 4.4e-5).  Hence the factor 3 on the max and the additive 4e-5 on the mean -- about
    a hundred extra flips of the largest effect over 1,000 positions -- which leaves the deep nets' mean bound where it
    was (1.4e-3 at 16 blocks, against 9.1e-4 measured)."""
    e = per_position_error(desc_outputs(folded, planes, fp16=True, acc32=True), desc_outputs(folded, planes, fp16=True))
    return 3 * float(e.max()) + 1e-5, 1.5 * float(e.mean()) + 4e-5


def grid_net(filters: int, n_res: int):
    """The stressed net of the GRID configuration (filters, n_res): the one every host and device test uses."""
    n_fc = [fc for f, r, fc, _ in GRID if (f, r) == (filters, n_res)][0]
    return stressed_state_dict(NetConfig(filters=filters, n_residuals=n_res, n_fc_layers=n_fc), seed=20 + n_res)


def grid_positions():
    """The positions every host and device test of the grid uses: 1,000 seeded positions + the edge positions."""
    return position_set(1000, seed=2)


# ---------------------------------------------------------------- nets
def stressed_state_dict(cfg: NetConfig, seed: int):
    """Every BatchNorm: gamma U[0.5, 1.5], beta N(0, 0.3), running mean N(0, 0.5), running var U[0.2, 2] per channel.
    3x3 convs N(0, g^2 / fan_in) with g = 1 for the stem and a block's first conv and g = 0.5 / sqrt(R) for its second
    (the residual branch), so the tower's activations stay O(1) up to 16 blocks; head 1x1 convs N(0, 1 / fan_in) with
    N(0, 0.3) biases; the Linear stack N(0, 1 / 42) (orthogonal-like: its collapse stays O(1) for 6 layers) with N(0, 0.1)
    biases; value fc1 and policy fc1 rescaled by _spread_heads so values and priors vary strongly; w1 = 1.1, w2 = 0.47."""
    net = PolicyValueNet(cfg)
    rng = np.random.RandomState(seed)
    R = cfg.n_residuals
    out = {}
    for k, v in net.state_dict().items():
        shape = tuple(v.shape)
        if k.endswith("num_batches_tracked"):
            a = v.numpy()
        elif k.endswith("running_mean"):
            a = rng.normal(0.0, 0.5, shape)
        elif k.endswith("running_var"):
            a = rng.uniform(0.2, 2.0, shape)
        elif ("batch_norm" in k or k.startswith("body.0.1.")) and k.endswith(".weight"):
            a = rng.uniform(0.5, 1.5, shape)
        elif ("batch_norm" in k or k.startswith("body.0.1.")) and k.endswith(".bias"):
            a = rng.normal(0.0, 0.3, shape)
        elif k.endswith("conv2.weight"):
            a = rng.normal(0.0, 0.5 / np.sqrt(max(R, 1)) / np.sqrt(np.prod(shape[1:])), shape)
        elif k.endswith("conv.weight") or k.endswith("conv1.weight") or k == "body.0.0.weight":
            a = rng.normal(0.0, 1.0 / np.sqrt(np.prod(shape[1:])), shape)
        elif k.endswith("conv1.bias"):
            a = rng.normal(0.0, 0.3, shape)
        elif k.startswith("value_head.fcN.") and k.endswith(".weight"):
            a = rng.normal(0.0, 1.0 / np.sqrt(42), shape)
        elif k.startswith("value_head.fcN.") and k.endswith(".bias"):
            a = rng.normal(0.0, 0.1, shape)
        elif k == "value_head.fc1.weight":
            a = rng.normal(0.0, 3.0 / np.sqrt(42), shape)
        elif k == "value_head.fc1.bias":
            a = rng.normal(0.0, 0.3, shape)
        elif k == "policy_head.fc1.weight":
            a = rng.normal(0.0, 4.0 / np.sqrt(84), shape)
        elif k == "policy_head.fc1.bias":
            a = rng.normal(0.0, 0.5, shape)
        elif k == "value_head.w1":
            a = np.array(1.1)
        elif k == "value_head.w2":
            a = np.array(0.47)
        else:
            raise KeyError(k)
        out[k] = torch.tensor(a, dtype=v.dtype).reshape(shape)
    return _spread_heads(out, rng, seed)


@torch.no_grad()
def _spread_heads(sd, rng, seed):
    """Rescale value fc1 and every policy fc1 row so that, over 256 seeded positions, the tanh argument has mean ~0 and
    standard deviation 0.7 and each logit a standard deviation of 1 (bias-dominated head inputs otherwise leave values
    saturated or priors near constant)."""
    net = _module(sd)
    c0, c1 = seeded_positions(256, seed + 1000)
    x = net.body(torch.from_numpy(planes_of(c0, c1)))
    vh, ph = net.value_head, net.policy_head
    u = F.leaky_relu(vh.fcN(vh.batch_norm(vh.conv1(x), slope=LEAK).flatten(1)), LEAK)
    s = u @ vh.fc1.weight.T
    k = 0.7 / float(s.std())
    sd["value_head.fc1.weight"] = (vh.fc1.weight * k).float()
    sd["value_head.fc1.bias"] = torch.tensor([-float(s.mean()) * k + rng.normal(0.0, 0.1)], dtype=torch.float32)
    lg = ph.batch_norm(ph.conv1(x), slope=LEAK).flatten(1) @ ph.fc1.weight.T
    k = 1.0 / lg.std(0)
    sd["policy_head.fc1.weight"] = (ph.fc1.weight * k[:, None]).float()
    sd["policy_head.fc1.bias"] = (-lg.mean(0) * k + torch.from_numpy(rng.normal(0.0, 0.3, 7))).float()
    return sd


def rescaled_state_dict(sd, c: float):
    """The same function computed with every tower activation multiplied by c (a power of two): stem BN gamma and beta
    x c, every tower BN beta and running mean x c, both head conv1 weights x 1/c (LeakyReLU is positively homogeneous)."""
    out = {k: v.clone() for k, v in sd.items()}
    out["body.0.1.weight"] *= c
    out["body.0.1.bias"] *= c
    for k in sd:
        if k.startswith("body.1.") and (k.endswith(".bias") or k.endswith(".running_mean")):
            out[k] *= c
    out["value_head.conv1.weight"] /= c
    out["policy_head.conv1.weight"] /= c
    return out


# ---------------------------------------------------------------- positions
def planes_of(c0, c1):
    """[n, 3, 6, 7] float64 planes built on the host by Board.to_array."""
    return np.stack([Board.from_bits(int(a), int(b)).to_array() for a, b in zip(c0, c1)]).astype(np.float64)


def _bits_of(moves):
    """Bitboards after playing `moves` (columns; o first) with no regard for wins: bit = 7 col + row from the bottom."""
    c = [0, 0]
    h = [0] * 7
    for i, m in enumerate(moves):
        c[i & 1] |= 1 << (7 * m + h[m])
        h[m] += 1
    return c[0], c[1]


def seeded_positions(n: int, seed: int):
    """n legal positions of random play, plies 0..41 in turn (both sides to move); games that end early are replayed."""
    rng = np.random.RandomState(seed)
    c0, c1 = [], []
    while len(c0) < n:
        ply = len(c0) % 42
        b = Board()
        for _ in range(ply):
            moves = sorted(b.valid_moves)
            if not moves:
                break
            b.make_move(int(rng.choice(moves)))
        if b.age != ply or (b.result is not None and ply < 42):
            continue
        c0.append(b.color[0])
        c1.append(b.color[1])
    return np.array(c0, dtype=np.uint64), np.array(c1, dtype=np.uint64)


def edge_positions(seed: int = 0):
    """The empty board; boards with 1..6 full columns; boards with a stone in the top row of every column (full boards)."""
    rng = np.random.RandomState(seed)
    out = [(0, 0)]
    for k in range(1, 7):
        for _ in range(3):
            cols = list(rng.permutation(7)[:k])
            moves = [c for c in cols for _ in range(6)]
            moves += [int(c) for c in rng.randint(0, 7, size=rng.randint(0, 8)) if c not in cols and moves.count(c) < 6]
            out.append(_bits_of(moves))
    for _ in range(4):
        out.append(_bits_of(list(rng.permutation([c for c in range(7) for _ in range(6)]))))
    return np.array([a for a, _ in out], dtype=np.uint64), np.array([b for _, b in out], dtype=np.uint64)


def position_set(n: int, seed: int):
    a0, a1 = seeded_positions(n, seed)
    b0, b1 = edge_positions(seed)
    return np.concatenate([a0, b0]), np.concatenate([a1, b1])


# ---------------------------------------------------------------- float64 reference
def _module(sd):
    cfg = PolicyValueNet.config_from_state_dict(sd)
    net = PolicyValueNet(cfg).double().eval()
    net.load_state_dict(sd, strict=True)
    return net


@torch.no_grad()
def float64_outputs(sd, c0, c1, planes=None):
    """(values [n], priors [n, 7]) of PolicyValueNet(cfg).double().eval() loaded with sd."""
    x = torch.from_numpy(planes_of(c0, c1) if planes is None else planes)
    v, p = _module(sd)(x)
    return v.numpy(), p.numpy()


@torch.no_grad()
def float64_max_activation(sd, c0, c1, planes=None):
    """Largest |activation| the tower stores (stem and every conv's output after LeakyReLU), in float64."""
    net = _module(sd)
    seen = [0.0]
    hooks = [m.register_forward_hook(lambda m, i, o: seen.__setitem__(0, max(seen[0], float(o.abs().max()))))
             for name, m in net.body.named_modules() if type(m).__name__ == "_BatchNorm2d"]
    net(torch.from_numpy(planes_of(c0, c1) if planes is None else planes))
    for h in hooks:
        h.remove()
    return seen[0]


# ---------------------------------------------------------------- models of the folded arrays (c4_net_desc)
def _r16(x):
    """fp32 accumulator -> fp16 store (round to nearest even, fp16 subnormals kept: numpy's gradual underflow)."""
    return torch.from_numpy(x.numpy().astype(np.float32).astype(np.float16).astype(np.float64))


@torch.no_grad()
def desc_outputs(a, planes, fp16=False, acc32=False):
    """float64 forward of the c4_net_desc arrays `a` (include/c4_engine.h: stem_w [F][3][3][3], stem_b [F], conv_w
    [2R][F][F][3][3], conv_b [2R][F], head_w [3][F] value then policy, head_b [3], vfc_w [42][42], vfc_b [42], vout_w
    [42], pfc_w [7][84], pfc_b [7]; scalars vout_b, w1, w2).  fp16=True: the fp16-storage arithmetic (see
    fp16_storage_outputs); acc32=True on top: the stem and tower convs summed in float32 (the host's order), as an
    fp32-accumulating implementation would (f16_tolerances)."""
    td = torch.float32 if acc32 else torch.float64
    t = lambda k: torch.from_numpy(np.asarray(a[k], dtype=np.float64))  # noqa: E731
    w16 = (lambda k: _r16(t(k))) if fp16 else t
    act = (lambda y: _r16(F.leaky_relu(y, LEAK)).to(td)) if fp16 else (lambda y: F.leaky_relu(y, LEAK))
    Fw = a["stem_b"].shape[0]
    R = (np.asarray(a["conv_b"]).size // Fw) // 2 if np.asarray(a["conv_b"]).size >= Fw else 0
    x = torch.from_numpy(planes).to(td)
    x = act(F.conv2d(x, w16("stem_w").reshape(Fw, 3, 3, 3).to(td), t("stem_b").to(td), padding=1))
    cw, cb = w16("conv_w").to(td), t("conv_b").to(td)
    for i in range(R):
        y = act(F.conv2d(x, cw[2 * i].reshape(Fw, Fw, 3, 3), cb[2 * i].reshape(Fw), padding=1))
        x = act(F.conv2d(y, cw[2 * i + 1].reshape(Fw, Fw, 3, 3), cb[2 * i + 1].reshape(Fw), padding=1) + x)
    x = x.double()
    h = F.leaky_relu(F.conv2d(x, w16("head_w").reshape(3, Fw, 1, 1), t("head_b")), LEAK)
    n = h.shape[0]
    hv, hp = h[:, 0].reshape(n, 42), h[:, 1:3].reshape(n, 84)
    v = F.leaky_relu(hv @ t("vfc_w").T + t("vfc_b"), LEAK)
    v = torch.tanh(v @ t("vout_w").reshape(42) + float(a["vout_b"]))
    values = (v + float(a["w1"])) * float(a["w2"])
    priors = torch.softmax(hp @ t("pfc_w").T + t("pfc_b"), dim=1)
    return values.numpy(), priors.numpy()


def fp16_storage_outputs(sd, c0, c1, planes=None):
    """float64 model of the fp16-storage forwards (precision "f16": net_forward_block / net_forward_wave16n /
    net_forward_wave16w).  Starting from the float32 arrays FusedNet hands to c4_net_create (fold_for_fused), it rounds to
    fp16 exactly where the kernels store fp16, and nowhere else:
      * the folded stem, 3x3 and head 1x1 weights (c4_net_create: (_Float16) of the float32 weight, the MFMA A operand);
      * every conv layer's output after LeakyReLU (store16: the fp32 accumulator -> lrelu -> fp16 plane; the residual
        skip adds that stored fp16 block input through an identity MFMA, exactly);
    the input planes are 0/1 (exact).  Unrounded, as in the kernels' fp32: the biases (the accumulators' initial value),
    the head convs' sums plus bias and their LeakyReLU (written to the fp32 head scratch), the value / policy MLPs, tanh
    and softmax.  fp16 subnormals are kept (gradual underflow), as the device's conversions and MFMAs treat them under
    the default fp16 denormal mode; accumulation order and fp32 rounding of the sums are not modelled."""
    from connect4_amd.fused_net import fold_for_fused
    return desc_outputs(fold_for_fused(sd), planes_of(c0, c1) if planes is None else planes, fp16=True)
