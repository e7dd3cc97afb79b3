"""The reference's value and policy statistics (oinkoink/neural/stats.py), on the host and on the device.

``ValueStats`` / ``PriorStats`` / ``CombinedStats`` mirror the reference's classes: same attributes, properties, ``to_dict()``
keys, ``__repr__`` text and ``update(...)`` arithmetic (NumPy), pinned to the unmodified reference by
tests/test_stats_host.py.  Each also builds itself from a read-back device accumulator (``from_accumulator``).

``DeviceStats`` owns such an accumulator (c4_score_acc, include/c4_engine.h) and feeds it with c4_score_update_dev: two
launches per batch on the caller's stream, capturable in the train step's HIP graph, nothing read back until ``read()``.
``LabelledSet`` is a labelled test set on the device as packed boards; ``score(net, labelled_set)`` gives any self-play
evaluator's statistics on one, ``score_search(config, net, labelled_set)`` those of the net with a search on top.  What the device reports differs from ``update`` fed batch by batch in one documented way:
the losses are sums of float64 row losses instead of float32 batch means times the batch length (include/c4_engine.h).
"""
import ctypes as C

import numpy as np

from . import _lib as L

_KEYS = (0.0, 0.5, 1.0)


class ValueStats:
    """stats.py:4-71"""

    def __init__(self):
        self.n = 0
        self.average_value = 0.0
        self.total_loss = 0.0
        self.smallest = 1.0
        self.largest = 0.0
        self.correct = {i: 0 for i in _KEYS}
        self.total = {i: 0 for i in _KEYS}
        self.non_finite = 0          # (device accumulators only: rows with a NaN / inf output)

    @classmethod
    def from_accumulator(cls, acc):
        """From a read-back c4_score_acc (_lib.ScoreAcc).  The reference's starting values 1.0 / 0.0 of smallest / largest
        (stats.py:9-10) apply here, as its min(self.smallest, .) / max(self.largest, .) apply them."""
        s = cls()
        s.n = int(acc.n)
        s.average_value = float(acc.sum_outputs)
        s.total_loss = float(acc.value_sq_err_sum)
        s.smallest = min(1.0, float(acc.smallest))
        s.largest = max(0.0, float(acc.largest))
        for i, k in enumerate(_KEYS):
            s.total[k] = int(acc.total[i])
            s.correct[k] = int(acc.correct[i])
        s.non_finite = int(acc.non_finite)
        return s

    @property
    def loss(self):
        return float(self.total_loss) / self.n

    @property
    def accuracy(self):
        return float(sum(self.correct.values())) / self.n

    @property
    def average(self):
        return self.average_value / self.n

    def to_dict(self):
        dict_ = {'Average loss': self.loss,
                 'Accuracy': self.accuracy,
                 'Smallest': self.smallest,
                 'Largest': self.largest,
                 'Average': self.average}
        dict_['correct'] = {k: (self.total[k], self.correct[k]) for k in self.correct}
        return dict_

    def __repr__(self):
        x = ("Average loss:  {:.5f}  Accuracy:  {:.5f}  Smallest:  {:.5f}  Largest:  {:.5f}  Average:  {:.5f}"
             "\nCategory, # Members, # Correct Predictions:").format(self.loss, self.accuracy, self.smallest, self.largest,
                                                                     self.average)
        for k in self.correct:
            x += "  ({}, {}, {})".format(k, self.total[k], self.correct[k])
        return x

    def update(self, outputs, values, loss):
        """stats.py:53-65: outputs, values NumPy [m]; loss the batch's mean loss (whatever type the caller has: the
        reference hands a float32 tensor from evaluate and a Python float from evaluate_value_only)."""
        self.n += len(values)
        self.average_value += np.sum(outputs)
        self.total_loss += loss * len(values)
        self.smallest = min(self.smallest, np.min(outputs).item())
        self.largest = max(self.largest, np.max(outputs).item())
        categories = self.categorise_predictions(outputs)
        for k in self.correct:
            idx = np.where(values == k)[0]
            self.total[k] += len(idx)
            self.correct[k] += int(np.count_nonzero(np.equal(categories[idx], values[idx])))

    def categorise_predictions(self, preds):
        return np.floor(preds * 3.0) / 2.0


class PriorStats:
    """stats.py:74-113"""

    def __init__(self):
        self.n = 0
        self.total_loss = 0.0
        self.correct = 0

    @classmethod
    def from_accumulator(cls, acc):
        """The reference's total_loss adds mean-over-(rows x 7) losses times the rows: the BCE sum over 7."""
        s = cls()
        s.n = int(acc.prior_n)
        s.total_loss = float(acc.prior_bce_sum) / 7.0
        s.correct = int(acc.prior_correct)
        return s

    @property
    def loss(self):
        return float(self.total_loss) / self.n

    @property
    def accuracy(self):
        return float(self.correct) / self.n

    def to_dict(self):
        return {'Average loss': self.loss, 'Accuracy': self.accuracy}

    def __repr__(self):
        return "Average loss:  {:.5f}  Accuracy:  {:.5f}".format(self.loss, self.accuracy)

    def update(self, outputs, values, loss):
        """stats.py:99-113: a row is correct when np.argmax of its outputs is among the maxima of its label row."""
        self.n += len(values)
        self.total_loss += loss * len(values)
        if len(values):
            best = np.argmax(outputs, axis=1)
            picked = np.take_along_axis(np.asarray(values), best[:, None], axis=1)[:, 0]
            self.correct += int(np.count_nonzero(picked == np.amax(values, axis=1)))


class CombinedStats:
    """stats.py:116-142"""

    def __init__(self):
        self.value_stats = ValueStats()
        self.prior_stats = PriorStats()

    @classmethod
    def from_accumulator(cls, acc):
        s = cls()
        s.value_stats = ValueStats.from_accumulator(acc)
        s.prior_stats = PriorStats.from_accumulator(acc)
        return s

    @property
    def loss(self):
        return self.value_stats.loss + self.prior_stats.loss

    def update(self, value_outputs, values, value_loss, prior_outputs, priors, prior_loss):
        self.value_stats.update(value_outputs, values, value_loss)
        self.prior_stats.update(prior_outputs, priors, prior_loss)

    def to_dict(self):
        dict_ = {'prior ' + k: v for k, v in self.prior_stats.to_dict().items()}
        dict_.update(self.value_stats.to_dict())
        return dict_

    def __repr__(self):
        return "{}\n{}".format(self.value_stats.__repr__(), self.prior_stats.__repr__())


def plain_dict(stats):
    """to_dict() with nothing but Python floats, ints, tuples and dicts in it (what the report files pickle)."""
    out = {}
    for k, v in stats.to_dict().items():
        out[k] = {float(c): (int(t), int(r)) for c, (t, r) in v.items()} if isinstance(v, dict) else float(v)
    return out


# -- the device accumulator ---------------------------------------------------------------------------------------------
def _check(rc):
    if rc != L.OK:
        msg = L.load().c4_score_last_error()
        raise L.EngineError(rc, msg.decode("utf-8", "replace") if msg else "")


def _stream_handle(stream, device):
    import torch
    if stream is None:
        return torch.cuda.current_stream(device).cuda_stream
    return int(getattr(stream, "cuda_stream", stream))


class DeviceStats:
    """A c4_score_acc on `device` and the workspace of its updates.  update() launches and returns; snapshot() and reset()
    are queued on the current stream like it; read() is the one call that waits for the device."""

    calls = 0           # update launches of every instance, since import (tests assert that stats=False adds none)
    _MAX_ROWS = 1 << 40     # c4_score_workspace_bytes is capped by the largest grid: one allocation fits every batch size

    def __init__(self, device, with_priors=True):
        import torch
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("DeviceStats accumulates on the GPU (c4_score_update_dev) and there is no CPU fallback; "
                               "on the host use ValueStats / CombinedStats.update")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.with_priors = bool(with_priors)
        self._lib = L.load()
        self._acc = torch.zeros(C.sizeof(L.ScoreAcc), dtype=torch.uint8, device=self.device)
        self._ws = torch.zeros(int(self._lib.c4_score_workspace_bytes(self._MAX_ROWS)), dtype=torch.uint8, device=self.device)
        self.reset()

    def reset(self, stream=None):
        _check(self._lib.c4_score_reset_dev(self.device.index, C.c_void_p(_stream_handle(stream, self.device)),
                                            C.c_void_p(self._acc.data_ptr())))

    def update(self, x_value, y_value, x_prior=None, y_prior=None, valid_rows=None, stream=None):
        """Add the first valid_rows (default: all) rows of float32 device tensors x_value, y_value [rows] and -- when the
        accumulator was made with_priors -- x_prior, y_prior [rows, 7].  Contiguous tensors on this device; nothing is
        copied, allocated or waited for."""
        import torch
        rows = int(x_value.shape[0])
        pairs = [(x_value, (rows,)), (y_value, (rows,))]
        if self.with_priors:
            if x_prior is None or y_prior is None:
                raise ValueError("this accumulator was made with_priors: x_prior and y_prior are needed")
            pairs += [(x_prior, (rows, 7)), (y_prior, (rows, 7))]
        elif x_prior is not None or y_prior is not None:
            raise ValueError("this accumulator was made without priors")
        for t, shape in pairs:
            if t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != self.device:
                raise ValueError("DeviceStats.update takes contiguous float32 tensors on %s of shapes [rows] and [rows, 7]; got "
                                 "%s %s on %s" % (self.device, t.dtype, tuple(t.shape), t.device))
        k = rows if valid_rows is None else int(valid_rows)
        ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        DeviceStats.calls += 1
        _check(self._lib.c4_score_update_dev(self.device.index, C.c_void_p(_stream_handle(stream, self.device)), ptr(x_value),
                                             ptr(y_value), ptr(x_prior) if self.with_priors else None,
                                             ptr(y_prior) if self.with_priors else None, rows, k, ptr(self._acc), ptr(self._ws)))

    def snapshot(self):
        """A device copy of the accumulator as it is at this point of the current stream (asynchronous)."""
        return self._acc.clone()

    def decode(self, raw):
        """ValueStats / CombinedStats of the accumulator bytes `raw` (host uint8 [112])."""
        acc = L.ScoreAcc.from_buffer_copy(bytes(raw.numpy().tobytes()))
        return (CombinedStats if self.with_priors else ValueStats).from_accumulator(acc)

    def read_accumulator(self, snapshot=None):
        """The raw _lib.ScoreAcc (waits for the device)."""
        raw = (self._acc if snapshot is None else snapshot).cpu()
        return L.ScoreAcc.from_buffer_copy(bytes(raw.numpy().tobytes()))

    def read(self, snapshots=None):
        """The statistics accumulated so far -- or, given a list of snapshot()s, a list with the statistics of each, in
        ONE copy to the host.  The only call that synchronises."""
        import torch
        if snapshots is None:
            return self.decode(self._acc.cpu())
        if not snapshots:
            return []
        raw = torch.stack(list(snapshots)).cpu()
        return [self.decode(r) for r in raw]


# -- labelled sets --------------------------------------------------------------------------------------------------------
class LabelledSet:
    """Labelled positions on a device: boards int64 [n, 2] (packed, what c4_export_games_dev writes), values float32 [n],
    priors float32 [n, 7] or None (a value-only set, as the reference's 7- and 8-ply sets)."""

    def __init__(self, boards, values, priors=None):
        import torch
        n = int(boards.shape[0])
        if boards.dtype != torch.int64 or tuple(boards.shape) != (n, 2) or values.dtype != torch.float32 or tuple(values.shape) != (n,) \
                or (priors is not None and (priors.dtype != torch.float32 or tuple(priors.shape) != (n, 7))):
            raise ValueError("a labelled set is (boards int64 [n,2], values float32 [n], priors float32 [n,7] or None)")
        self.boards, self.values = boards.contiguous(), values.to(boards.device).contiguous()
        self.priors = None if priors is None else priors.to(boards.device).contiguous()

    def __len__(self):
        return int(self.boards.shape[0])

    @property
    def device(self):
        return self.boards.device

    @classmethod
    def from_tensors(cls, boards_f32, values, priors=None, device=None):
        """From the tensors of a Connect4Dataset (data.py:13-20): boards float32 [n, 3, 6, 7].  The planes are turned back
        into bitboards on the device (c4_planes_to_boards_dev); a row that no board encodes raises ValueError."""
        import torch
        from . import engine as _engine
        dev = torch.device(device) if device is not None else (boards_f32.device if boards_f32.device.type == "cuda" else torch.device("cuda"))
        planes = boards_f32.to(dev, torch.float32)
        with torch.cuda.device(dev):
            boards, n_bad = _engine.planes_to_boards(planes)
            n_bad = int(n_bad.item())
        if n_bad:
            raise ValueError("%d of %d rows are not the planes of a board" % (n_bad, int(planes.shape[0])))
        return cls(boards, values.to(dev, torch.float32), None if priors is None else priors.to(dev, torch.float32))

    @classmethod
    def load(cls, path, device=None):
        """A file written by the reference's Connect4Dataset.save (data.py:22-33): a dict of boards / values / priors."""
        import torch
        d = torch.load(path, map_location="cpu", weights_only=True)
        return cls.from_tensors(d["boards"], d["values"], d.get("priors"), device=device)

    def save(self, path):
        """Write the file the reference's Connect4Dataset.save writes (data.py:22-33): a dict of CPU tensors, boards float32
        [n, 3, 6, 7] (board.py:147-154), values float32 [n], priors float32 [n, 7] (None for a value-only set).  load() and
        the reference's Connect4Dataset.load read it back.  A set on the GPU builds its planes there; a set on the CPU is
        converted by the host Board."""
        import torch
        if self.device.type == "cuda":
            planes = self.planes().cpu()
        else:
            from .board import Board
            bits = self.boards.numpy().view(np.uint64)
            planes = torch.from_numpy(np.stack([Board.from_bits(int(a), int(b)).to_array() for a, b in bits]).astype(np.float32)
                                      if len(bits) else np.zeros((0, 3, 6, 7), dtype=np.float32))
        torch.save({"boards": planes, "values": self.values.cpu(), "priors": None if self.priors is None else self.priors.cpu()},
                   path)

    def planes(self):
        """The float32 planes [n, 3, 6, 7] of the boards (board.py:147-154), built on the device (c4_training_tensors_dev)."""
        import torch
        from . import engine as _engine
        if self.device.type != "cuda":
            raise RuntimeError("LabelledSet.planes runs on the GPU (c4_training_tensors_dev); there is no CPU fallback")
        policy = self.priors if self.priors is not None else torch.zeros((len(self), 7), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            return _engine.training_tensors(self.boards, self.values, policy, add_fliplr=False)[0]


def score(net, labelled_set, batch_size=32768):
    """The statistics of evaluate / evaluate_value_only (model.py:180-198) for an evaluator make_selfplay_net returns, on
    a LabelledSet: a FusedNet reads the packed boards themselves (forward_bitboards: 16 B per position, no planes), any
    other evaluator (InferenceNet) is called on planes().  CombinedStats, or ValueStats for a set without priors."""
    import torch
    ls = labelled_set
    if ls.device.type != "cuda":
        raise RuntimeError("score() runs on the GPU: the labelled set must live on a cuda device")
    n = len(ls)
    with torch.cuda.device(ls.device), torch.no_grad():
        ds = DeviceStats(ls.device, with_priors=ls.priors is not None)
        fused = getattr(net, "from_bitboards", False)
        if fused:
            c0, c1 = ls.boards[:, 0].contiguous(), ls.boards[:, 1].contiguous()
        else:
            planes = ls.planes()
        for a in range(0, n, batch_size):
            b = min(n, a + batch_size)
            if fused:
                xv = torch.empty(b - a, dtype=torch.float32, device=ls.device)
                xp = torch.empty((b - a, 7), dtype=torch.float32, device=ls.device)
                net.forward_bitboards(c0[a:b].data_ptr(), c1[a:b].data_ptr(), b - a, xv, xp)
            else:
                xv, xp = net(planes[a:b])
                xv, xp = xv.float().contiguous(), xp.float().contiguous()
            if ls.priors is not None:
                ds.update(xv, ls.values[a:b], xp, ls.priors[a:b])
            else:
                ds.update(xv, ls.values[a:b])
        return ds.read()


def score_search(config, net, labelled_set, n_slots=None, eval_cache_log2_entries=0, steps_per_launch=64):
    """score() for net + search: every position of the LabelledSet is searched with `config` (the position queue of
    connect4_amd.analysis: packed boards queued straight from the device, n_slots engine slots, default min(n, 4096)), and
    what the search says -- the root's mean value (root value sum / root visits) as the value output, the values policy
    (tree.get_values_policy()) as the policy output -- goes through the accumulator score() uses, against the same labels.
    The difference to score(net, labelled_set) is what the simulations add to the checkpoint.  net: what make_selfplay_net
    returns (or a DeviceNetEvaluator); CombinedStats, or ValueStats for a set without priors."""
    import torch
    from .analysis import run_queue
    from .evaluators import DeviceNetEvaluator
    ls = labelled_set
    if ls.device.type != "cuda":
        raise RuntimeError("score_search() runs on the GPU: the labelled set must live on a cuda device")
    dev_index = ls.device.index if ls.device.index is not None else torch.cuda.current_device()
    evaluator = net if isinstance(net, DeviceNetEvaluator) else DeviceNetEvaluator(net, dev_index)
    with torch.cuda.device(ls.device), torch.no_grad():
        eng = run_queue(config, ls.boards, evaluator, n_slots, dev_index, eval_cache_log2_entries, steps_per_launch)
        try:
            out = eng.queue_export(("policy", "root_values"))
            ds = DeviceStats(ls.device, with_priors=ls.priors is not None)
            if ls.priors is not None:
                ds.update(out["root_values"], ls.values, out["policy"], ls.priors)
            else:
                ds.update(out["root_values"], ls.values)
            return ds.read()
        finally:
            eng.close()
