"""Exact values for late search leaves: the solver laid over the net.

``ExactLeafNet(net, max_empties)`` is an evaluator that is `net` everywhere except on late leaves -- undecided positions with
at most `max_empties` empty squares -- where the value is the game-theoretic outcome (1.0 o wins, 0.5 draw, 0.0 x wins: the
evaluator's convention and ``exact_targets``').  It plugs in wherever a ``from_bitboards`` net does: after the inner net's
forward, one more asynchronous launch on the same stream (c4_exact_leaves_dev, csrc/c4_solve.hip) searches the late rows of
the leaf batch table-free from the window (-1, +1) under a small node budget and overwrites their values.  A row over budget
keeps the net's value, and so does every row that is not late; priors are always the net's.  The launch allocates nothing and
waits for nothing, so the HIP graph of the step path (``SelfPlay._capture``) records it like the forward.

It is deliberately not a ``FusedNet``: it has no c4_net handle, so self-play takes the step path (c4_step, forward, overlay)
instead of the fused kernel, and ``play_match`` falls back to the host lock-step ``Match`` on its own.

``overlay_host`` is the same rule in NumPy over ``solver.solve_host(window=(-1, 1))``.
"""
import ctypes as C

import numpy as np

from . import _lib as L
from . import solver

__all__ = ["ExactLeafNet", "overlay_host", "DEFAULT_NODE_BUDGET", "MAX_EMPTIES"]

MAX_EMPTIES = L.SOLVE_MAX_EMPTIES
# The smallest budget of profiles/exact_leaves.json whose over-budget share at max_empties = 10 is under 1 %: 0.14 % of the late
# rows (64 leaves 1.14 %), at 3.68 times the step-path self-play without the overlay (4,096 games, 800 simulations, one MI355X).
DEFAULT_NODE_BUDGET = 256


def _check_args(max_empties, node_budget):
    if isinstance(max_empties, bool) or not isinstance(max_empties, (int, np.integer)) or not 0 <= max_empties <= MAX_EMPTIES:
        raise ValueError("max_empties must be a whole number in 0..%d; got %r" % (MAX_EMPTIES, max_empties))
    if node_budget is not None and (isinstance(node_budget, bool) or not isinstance(node_budget, (int, np.integer)) or node_budget < 1):
        raise ValueError("node_budget must be a whole number of at least 1; got %r" % (node_budget,))
    return int(max_empties), (None if node_budget is None else int(node_budget))


def overlay_host(c0, c1, values, max_empties, node_budget=None):
    """c4_exact_leaves_dev's rule on the host: ``(values, overridden)``, a float32 copy of `values` in which every late row that
    ``solver.solve_host(window=(-1, 1), node_budget=node_budget)`` answers holds 1.0 / 0.5 / 0.0 from o's side, and the bool
    mask of those rows.  A late row is one the solver would search (an undecided position) with at most `max_empties` empty
    squares; all other rows, and late rows over budget, keep their value bit for bit.  node_budget=None: the solver's
    default."""
    max_empties, node_budget = _check_args(max_empties, node_budget)
    c0 = np.asarray(c0, dtype=np.uint64).reshape(-1)
    c1 = np.asarray(c1, dtype=np.uint64).reshape(-1)
    out = np.array(values, dtype=np.float32).reshape(-1)
    if not (len(c0) == len(c1) == len(out)):
        raise ValueError("c0, c1 and values have one entry per row; got %d, %d and %d" % (len(c0), len(c1), len(out)))
    overridden = np.zeros(len(out), dtype=bool)
    if max_empties == 0:
        return out, overridden
    for i in range(len(out)):
        a, b = int(c0[i]), int(c1[i])
        if solver._classify(a, b, max_empties) != L.SOLVE_SOLVED:
            continue
        ans = solver.solve_host((a, b), node_budget=node_budget, window=(-1, 1))
        if ans.status != L.SOLVE_SOLVED:
            continue        # over budget
        sign = (ans.score > 0) - (ans.score < 0)
        if bin(a | b).count("1") & 1:       # o moves at even ages
            sign = -sign
        out[i] = np.float32(0.5 * (sign + 1))
        overridden[i] = True
    return out, overridden


class ExactLeafNet:
    """`net` with exact values on late leaves.  net: a ``from_bitboards`` net (``FusedNet``) -- the overlay runs on its device;
    max_empties: 0..24, required (0 overrides nothing and launches nothing); node_budget: the nodes a late row may enter, the
    root included -- a row that would need one more keeps the net's value."""
    from_bitboards = True

    def __init__(self, net, max_empties, node_budget=DEFAULT_NODE_BUDGET):
        import torch
        self.max_empties, self.node_budget = _check_args(max_empties, node_budget)
        if node_budget is None:
            raise ValueError("node_budget must be a whole number of at least 1; got None")
        device = getattr(net, "device", None)
        if not getattr(net, "from_bitboards", False) or not hasattr(net, "forward_bitboards") or isinstance(device, bool) or \
                not isinstance(device, int):
            raise ValueError("ExactLeafNet lays the solver over a from_bitboards net on a GPU (a FusedNet); got %r" % (net,))
        self.net = net
        self.device = device
        self.config = getattr(net, "config", None)
        self.precision = getattr(net, "precision", None)
        self._lib = L.load()
        self._counters = torch.zeros(len(L.EXACT_LEAVES_COLUMNS), dtype=torch.int64, device=torch.device("cuda", device))

    def forward_bitboards(self, c0_ptr, c1_ptr, n, values, priors, stream=None, wave=False):
        """``FusedNet.forward_bitboards``, then the overlay on the same stream: the late rows' `values` become exact."""
        import torch
        if values.device.type != "cuda" or values.device.index != self.device:
            raise ValueError("values live on %s, the net on cuda:%d" % (values.device, self.device))
        if stream is None:
            stream = torch.cuda.current_stream(values.device).cuda_stream
        self.net.forward_bitboards(c0_ptr, c1_ptr, n, values, priors, stream, wave=wave)
        rc = self._lib.c4_exact_leaves_dev(self.device, C.c_void_p(stream), C.c_void_p(c0_ptr), C.c_void_p(c1_ptr), int(n),
                                           self.max_empties, self.node_budget, C.c_void_p(values.data_ptr()),
                                           C.c_void_p(self._counters.data_ptr()))
        solver._check(rc)

    def evaluate_bits(self, color0, color1, wave=False):
        """NumPy uint64 rows -> (values, priors) NumPy; what ``DeviceNetEvaluator.__call__`` and the oracle's replay use."""
        import torch
        dev = torch.device("cuda", self.device)
        c0 = torch.from_numpy(np.ascontiguousarray(color0, dtype=np.uint64).view(np.int64)).to(dev)
        c1 = torch.from_numpy(np.ascontiguousarray(color1, dtype=np.uint64).view(np.int64)).to(dev)
        n = c0.numel()
        v = torch.zeros(n, dtype=torch.float32, device=dev)
        p = torch.zeros(n, 7, dtype=torch.float32, device=dev)
        self.forward_bitboards(c0.data_ptr(), c1.data_ptr(), n, v, p, wave=wave)
        torch.cuda.synchronize(dev)
        return v.cpu().numpy(), p.cpu().numpy()

    def counters(self):
        """{"overridden", "over_budget", "nodes", "late"}: the sums over every forward since the last reset_counters(), leaf
        rows as the engine hands them over (a slot without a new leaf repeats its last row).  One read-back; it waits for the
        work queued so far."""
        return dict(zip(L.EXACT_LEAVES_COLUMNS, (int(x) for x in self._counters.cpu().tolist())))

    def reset_counters(self):
        self._counters.zero_()
