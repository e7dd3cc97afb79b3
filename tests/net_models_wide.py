"""Host model of the reference-precision forwards' storage arithmetic (csrc/c4_net_dev.h: net_forward_wave16q at 32
filters, net_forward_wave16x at 64), next to the fp16-storage model of net_models.desc_outputs.

f32x3_split_outputs is desc_outputs with every stored fp16 rounding replaced by the split rounding
    x  ->  hi + lo / 2^11,   hi = f16(x),   lo = f16((x - hi) * 2^11)
(a relative error of about 2^-22 instead of 2^-11) and the stem's and the tower's sums in float32 (the host's order).
What it does not model: the kernels' summation order, and the lo x lo products they drop (2^-22 relative to a product).
"""
import numpy as np
import torch
import torch.nn.functional as F

from net_models import LEAK, planes_of

LO_SCALE = 2048.0


def split_round(x):
    """float64 tensor -> float32 -> hi + lo / 2^11 with hi and lo in fp16 (numpy keeps fp16 subnormals, as the device does),
    returned as float64 (the sum of the two parts is exact there)."""
    x32 = x.numpy().astype(np.float32)
    hi = x32.astype(np.float16)
    lo = ((x32 - hi.astype(np.float32)) * np.float32(LO_SCALE)).astype(np.float16)
    return torch.from_numpy(hi.astype(np.float64) + lo.astype(np.float64) / LO_SCALE)


@torch.no_grad()
def f32x3_split_outputs(a, planes):
    """(values [n], priors [n, 7]) of the c4_net_desc arrays `a` (net_models.desc_outputs documents them) in the split
    arithmetic: folded stem / 3x3 / head 1x1 weights and every conv layer's output after LeakyReLU are rounded by
    split_round, the stem's and tower's sums run in float32; biases, head sums, MLPs, tanh and softmax as in desc_outputs."""
    td = torch.float32
    t = lambda k: torch.from_numpy(np.asarray(a[k], dtype=np.float64))  # noqa: E731
    ws = lambda k: split_round(t(k))  # noqa: E731
    act = lambda y: split_round(F.leaky_relu(y, LEAK).double()).to(td)  # noqa: E731
    Fw = a["stem_b"].shape[0]
    R = (np.asarray(a["conv_b"]).size // Fw) // 2 if np.asarray(a["conv_b"]).size >= Fw else 0
    x = torch.from_numpy(planes).to(td)
    x = act(F.conv2d(x, ws("stem_w").reshape(Fw, 3, 3, 3).to(td), t("stem_b").to(td), padding=1))
    cw, cb = ws("conv_w").to(td), t("conv_b").to(td)
    for i in range(R):
        y = act(F.conv2d(x, cw[2 * i].reshape(Fw, Fw, 3, 3), cb[2 * i].reshape(Fw), padding=1))
        x = act(F.conv2d(y, cw[2 * i + 1].reshape(Fw, Fw, 3, 3), cb[2 * i + 1].reshape(Fw), padding=1) + x)
    x = x.double()
    h = F.leaky_relu(F.conv2d(x, ws("head_w").reshape(3, Fw, 1, 1), t("head_b")), LEAK)
    n = h.shape[0]
    hv, hp = h[:, 0].reshape(n, 42), h[:, 1:3].reshape(n, 84)
    v = F.leaky_relu(hv @ t("vfc_w").T + t("vfc_b"), LEAK)
    v = torch.tanh(v @ t("vout_w").reshape(42) + float(a["vout_b"]))
    values = (v + float(a["w1"])) * float(a["w2"])
    priors = torch.softmax(hp @ t("pfc_w").T + t("pfc_b"), dim=1)
    return values.numpy(), priors.numpy()


def split_model_outputs(sd, c0, c1, planes=None):
    """f32x3_split_outputs of the arrays FusedNet hands to c4_net_create for the state dict sd."""
    from connect4_amd.fused_net import fold_for_fused
    return f32x3_split_outputs(fold_for_fused(sd), planes_of(c0, c1) if planes is None else planes)


@torch.no_grad()
def float32_module_outputs(sd, c0, c1, planes=None):
    """(values, priors) of this package's PolicyValueNet in float32, eval mode: the precision the reference evaluates in."""
    from connect4_amd.net import PolicyValueNet
    net = PolicyValueNet(PolicyValueNet.config_from_state_dict(sd)).float().eval()
    net.load_state_dict(sd, strict=True)
    x = torch.from_numpy((planes_of(c0, c1) if planes is None else planes).astype(np.float32))
    v, p = net(x)
    return v.double().numpy(), p.double().numpy()
