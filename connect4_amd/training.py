"""Train step with the reference's recipe (oinkoink/neural/pytorch/model.py:138-169,
200-250): SGD(momentum 0.9, weight decay 1e-4) + MultiStepLR, loss = MSE(value) + BCE(policy), 5 epochs x
batch 4096 over a shuffled dataset, checkpoint dict with the three state dicts.  Stock PyTorch-ROCm; not
on the hot path.

Parity with ``ModelWrapper.train`` is pinned (tests/test_training_cpu.py against a fixture generated from
the reference by tests/golden/gen_golden.py): batches are drawn exactly as the reference's
``DataLoader(data, batch_size, shuffle=True)`` draws them -- same consumption of torch's global RNG,
same permutation, same batch boundaries -- but gathered with one tensor index per batch instead of
4096 Python ``__getitem__`` calls + collate.
"""
import os
from typing import Optional

import torch
import torch.nn as nn
from torch.optim.lr_scheduler import MultiStepLR

from .net import NetConfig, PolicyValueNet


class ModelConfig:
    """oinkoink/neural/config.py:19-39"""

    def __init__(self, net_config=None, weight_decay=1e-4, momentum=0.9, initial_lr=0.01,
                 milestones=(100, 300, 600), gamma=0.1, batch_size=4096, n_training_epochs=5, use_gpu=True):
        self.net_config = net_config or NetConfig()
        self.weight_decay = weight_decay
        self.momentum = momentum
        self.initial_lr = initial_lr
        self.milestones = list(milestones)
        self.gamma = gamma
        self.batch_size = batch_size
        self.n_training_epochs = n_training_epochs
        self.use_gpu = use_gpu


def dataloader_permutation(n: int, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """The index order one pass of ``DataLoader(dataset_of_n, shuffle=True)`` visits, consuming torch's global
    RNG exactly as that pass does (torch.utils.data: _BaseDataLoaderIter.__init__ draws a base seed, then
    RandomSampler.__iter__ draws the seed of a private generator for ``randperm``)."""
    if generator is not None:          # an explicit generator (tests): one permutation from it
        return torch.randperm(n, generator=generator)
    torch.empty((), dtype=torch.int64).random_()                       # DataLoader iterator: _base_seed
    seed = int(torch.empty((), dtype=torch.int64).random_().item())    # RandomSampler.__iter__
    g = torch.Generator()
    g.manual_seed(seed)
    return torch.randperm(n, generator=g)


class _TensorBatches:
    """Batch source of Trainer.train: the materialised dataset on the trainer's device, one tensor index per batch."""

    def __init__(self, boards, values, priors, device):
        self.rows = int(boards.shape[0])
        self.boards, self.values, self.priors = boards.to(device), values.to(device), priors.to(device)

    def static_out(self, batch_size):
        return None             # (the captured indexings allocate their results in the graph's pool)

    def __call__(self, idx, out=None):
        return self.boards[idx], self.values[idx], self.priors[idx]


class _WindowBatches:
    """Batch source of Trainer.train_window: a ReplayWindow; a batch is one launch of its gather kernel.  The indices are
    a permutation of range(window.rows), so the kernel's out-of-range counter is not read (no host synchronisation per
    step); the captured step writes into buffers allocated before the capture."""

    def __init__(self, window):
        self.window = window
        self.rows = int(window.rows)

    def static_out(self, batch_size):
        dev = self.window.device
        return (torch.empty((batch_size, 3, 6, 7), dtype=torch.float32, device=dev),
                torch.empty(batch_size, dtype=torch.float32, device=dev),
                torch.empty((batch_size, 7), dtype=torch.float32, device=dev))

    def __call__(self, idx, out=None):
        return self.window.gather(idx, out=out, check=False)


class Trainer:
    """ModelWrapper's training half (model.py:138-169, 200-250).  `device`: where the net trains; default =
    the reference's rule (cuda:0 when use_gpu and a GPU is there, model.py:143-147) -- a multi-rank caller
    passes its own GPU."""

    def __init__(self, config: ModelConfig = None, file_name: str = None, device=None, pad_ragged_batches=None,
                 fused_bn=None, use_graph=None):
        self.config = config or ModelConfig()
        self.net = PolicyValueNet(self.config.net_config)
        if device is not None:
            self.device = torch.device(device)
        else:
            self.device = torch.device("cuda:0" if self.config.use_gpu and torch.cuda.is_available() else "cpu")
        self.net.to(self.device)
        # the ragged last batch of an epoch is padded to the full batch size (see net._BatchNorm2d); on by default on a GPU
        self.pad_ragged_batches = (self.device.type == "cuda") if pad_ragged_batches is None else bool(pad_ragged_batches)
        # On a GPU: batch normalisation (+ residual add + LeakyReLU) of the train step runs on the library's HIP kernels
        # (bn_train.py), and the full batches of a train() call are ONE captured HIP graph replayed per batch -- a stock
        # step is ~150 launches of ~25 us kernels, i.e. as much host dispatch as GPU work.  Both default on for cuda.
        self.fused_bn = (self.device.type == "cuda") if fused_bn is None else bool(fused_bn)
        self.use_graph = ((self.device.type == "cuda") if use_graph is None else bool(use_graph)) and self.fused_bn
        # (no graph with stock batch normalisation: under capture MIOpen's batch-norm backward leaves a small non-zero mean in
        #  dx, which is the whole gradient of the head convolutions' biases -- mathematically zero -- and they drift: -6.6
        #  after 138 steps where the eager step leaves 0.02; measured, build/train_probe3.py of round 3)
        from .net import _BatchNorm2d
        for m in self.net.modules():
            if isinstance(m, _BatchNorm2d):
                m.fused = self.fused_bn
        self.optimiser = torch.optim.SGD(self.net.parameters(), lr=self.config.initial_lr,
                                         momentum=self.config.momentum, weight_decay=self.config.weight_decay)
        self.scheduler = MultiStepLR(self.optimiser, milestones=self.config.milestones, gamma=self.config.gamma)
        if file_name is not None:   # model.py:157-161
            ckpt = torch.load(file_name, map_location=self.device, weights_only=True)
            self.net.load_state_dict(ckpt["net_state_dict"])
            self.optimiser.load_state_dict(ckpt["optimiser_state_dict"])
            self.scheduler.load_state_dict(ckpt["scheduler_state_dict"])
        self.value_loss = nn.MSELoss()
        self.prior_loss = nn.BCELoss()
        self.epoch_stats = []       # train(..., stats=True): one CombinedStats per epoch of the last call
        self.net.eval()

    def train(self, boards, values, priors, generator=None, stats=False):
        """One generation (model.py:200-240): n_training_epochs shuffled passes over (boards F32[N,3,6,7],
        values F32[N], priors F32[N,7]) -- tensors on any device; they are moved to the trainer's device once.
        Returns the last batch's loss.  stats=True is the reference's print_stats (model.py:208-209, 228-237): every
        step's outputs and labels are added to a device accumulator (stats.DeviceStats; one more launch pair of the step,
        captured with it) and after the last batch ONE read-back fills self.epoch_stats, a CombinedStats per epoch."""
        if self.device.type == "cuda":
            with torch.cuda.device(self.device):    # graph capture / replay and the library's launches go to the current device
                return self._train(_TensorBatches(boards, values, priors, self.device), generator, stats)
        return self._train(_TensorBatches(boards, values, priors, self.device), generator, stats)

    def train_window(self, window, generator=None, stats=False):
        """train() over a device-resident ReplayWindow (connect4_amd/replay.py) instead of the materialised tensors: the
        same shuffles of window.rows (same consumption of torch's RNG), the same batch boundaries, padded ragged batch,
        eager first steps and captured step -- only that a batch is built from the packed positions by the window's
        gather kernel (the first node of the captured graph) instead of three tensor indexings.  Row r of the window is
        row r of TrainingDataStorage.get_dataset, so both forms train on the same batches.  GPU only."""
        if self.device.type != "cuda":
            raise RuntimeError("Trainer.train_window needs a GPU trainer: a ReplayWindow is gathered by a HIP kernel "
                               "(c4_window_gather_dev) and there is no CPU fallback; use train() on materialised tensors")
        mine = self.device if self.device.index is not None else torch.device("cuda", torch.cuda.current_device())
        if window.device != mine:
            raise ValueError("the window lives on %s, the trainer on %s" % (window.device, self.device))
        with torch.cuda.device(self.device):
            return self._train(_WindowBatches(window), generator, stats)

    def _train(self, batches, generator, stats=False):
        self.epoch_stats = []
        ds, snaps = None, []
        if stats:       # a pure observer of the step's xv, xp, v, p; without it nothing below differs from the plain step
            from .stats import CombinedStats, DeviceStats
            ds = DeviceStats(self.device) if self.device.type == "cuda" else CombinedStats()
        n = batches.rows
        bs = self.config.batch_size
        self.net.train()
        last = None
        graph = None            # the captured step of THIS call (the data source and the learning rate are baked into it)
        eager_full = 0
        want_graph = self.use_graph and self.device.type == "cuda" and (n // bs) * self.config.n_training_epochs >= 4
        for _ in range(self.config.n_training_epochs):
            perm = dataloader_permutation(n, generator).to(self.device)
            for i in range(0, n, bs):
                idx = perm[i:i + bs]
                k = int(idx.shape[0])
                if k == bs and want_graph:
                    if graph is None and eager_full >= 2:      # (the first steps run eagerly: momentum buffers, MIOpen's choices)
                        graph, sidx, sloss = self._capture_step(batches, ds)
                    if graph is not None:
                        sidx.copy_(idx)
                        graph.replay()
                        last = sloss
                        continue
                    eager_full += 1
                pad = self.pad_ragged_batches and k < bs and n > bs and k > 1
                if pad:   # DataLoader's drop_last=False batch (model.py:208-212), at the full batch's shape
                    idx = torch.cat([idx, idx[:1].expand(bs - k)])
                    self._set_valid_rows(k)
                last = self._eager_step(*batches(idx), k if pad else None, ds)
                if pad:
                    self._set_valid_rows(None)
            if ds is not None and self.device.type == "cuda":     # the epoch's statistics stay on the device for now
                snaps.append(ds.snapshot())
                ds.reset()
            elif ds is not None:
                self.epoch_stats.append(ds)
                ds = type(ds)()
        last = None if last is None else float(last)
        if snaps:
            self.epoch_stats = ds.read(snaps)
        del graph
        self.optimiser.zero_grad()            # (gradients that live in a graph's pool are not kept)
        self.scheduler.step()       # once per generation (model.py:239)
        self.net.eval()
        return last

    def _eager_step(self, b, v, p, k=None, ds=None):
        """model.py:214-230 for one batch (its first k rows when the batch is a padded ragged one).  Returns the detached
        loss (read back once, after the last batch: no host synchronisation per step); nothing of the step's autograd graph
        outlives the call -- a graph captured later must not find AccumulateGrad nodes bound to this stream."""
        self.optimiser.zero_grad()
        xv, xp = self.net(b)
        if ds is not None and self.device.type == "cuda":
            ds.update(xv.detach(), v, xp.detach(), p, valid_rows=k)
        if k is not None:
            xv, xp, v, p = xv[:k], xp[:k], v[:k], p[:k]
        vloss, ploss = self.value_loss(xv, v), self.prior_loss(xp, p)
        loss = vloss + ploss   # model.py:221-225
        loss.backward()
        self.optimiser.step()
        if ds is not None and self.device.type != "cuda":     # model.py:228-234, on the host classes
            ds.update(xv.detach().numpy(), v.numpy(), vloss.detach(), xp.detach().numpy(), p.numpy(), ploss.detach())
        return loss.detach()

    def _capture_step(self, batches, ds=None):
        """One full-batch train step -- gather by a static index tensor, forward, loss, backward, SGD -- captured as a HIP
        graph (torch.cuda.graph): replayed per batch with the batch's indices copied into `sidx`.  Same kernels, same order,
        same arithmetic as the eager step."""
        sidx = torch.zeros(self.config.batch_size, dtype=torch.int64, device=self.device)
        out = batches.static_out(self.config.batch_size)
        self.optimiser.zero_grad(set_to_none=True)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            b, v, p = batches(sidx, out)
            xv, xp = self.net(b)
            if ds is not None:      # two more launches of the captured step
                ds.update(xv.detach(), v, xp.detach(), p)
            loss = self.value_loss(xv, v) + self.prior_loss(xp, p)
            loss.backward()
            self.optimiser.step()
            sloss = loss.detach()
        return graph, sidx, sloss

    # -- test-set scores (model.py:180-198, 307-342) ---------------------------------------------------------------------
    def evaluate(self, data, batch_size=4096, shuffle=True):
        """ModelWrapper.evaluate: this trainer's net in eval mode over a labelled set -- a stats.LabelledSet or a
        (boards F32[n,3,6,7], values F32[n], priors F32[n,7]) tuple --, batches drawn as the reference's DataLoader draws
        them (same consumption of torch's RNG) and forwarded by PyTorch.  On a GPU the outputs go to a DeviceStats and
        are read back once; on a CPU trainer the host classes are fed as the reference feeds its own.  Returns a
        CombinedStats."""
        return self._evaluate(data, batch_size, shuffle, True)

    def evaluate_value_only(self, data):
        """ModelWrapper.evaluate_value_only (model.py:192-198): the value half, batches of 4096.  Returns a ValueStats."""
        return self._evaluate(data, 4096, True, False)

    def _evaluate(self, data, batch_size, shuffle, with_priors):
        from .stats import CombinedStats, DeviceStats, LabelledSet, ValueStats
        if isinstance(data, LabelledSet):
            if data.device.type != self.device.type:
                raise ValueError("the labelled set lives on %s, the trainer on %s" % (data.device, self.device))
            data = (data.planes(), data.values, data.priors)
        boards, values = data[0].to(self.device), data[1].to(self.device)
        priors = data[2].to(self.device) if len(data) > 2 and data[2] is not None else None
        if with_priors and priors is None:
            raise ValueError("evaluate needs a set with priors; use evaluate_value_only")
        n = int(boards.shape[0])
        on_gpu = self.device.type == "cuda"
        was_training = self.net.training
        self.net.eval()
        try:
            with torch.no_grad():
                order = dataloader_permutation(n).to(self.device) if shuffle else torch.arange(n, device=self.device)
                if on_gpu:
                    with torch.cuda.device(self.device):
                        out = DeviceStats(self.device, with_priors=with_priors)
                        for i in range(0, n, batch_size):
                            idx = order[i:i + batch_size]
                            xv, xp = self.net(boards[idx])
                            if with_priors:
                                out.update(xv.contiguous(), values[idx], xp.contiguous(), priors[idx])
                            else:
                                out.update(xv.contiguous(), values[idx])
                        return out.read()
                out = CombinedStats() if with_priors else ValueStats()
                for i in range(0, n, batch_size):
                    idx = order[i:i + batch_size]
                    xv, xp = self.net(boards[idx])
                    v = values[idx]
                    if with_priors:     # model.py:318-326: the losses go in as tensors
                        p = priors[idx]
                        out.update(xv.numpy(), v.numpy(), self.value_loss(xv, v), xp.numpy(), p.numpy(), self.prior_loss(xp, p))
                    else:               # model.py:337-341: loss.item()
                        out.update(xv.numpy(), v.numpy(), self.value_loss(xv, v).item())
                return out
        finally:
            self.net.train(was_training)

    def state(self):
        """The checkpoint dict of save() with CPU tensors (model.py:242-250)."""
        def cpu(o):
            if isinstance(o, torch.Tensor):
                return o.detach().cpu()
            if isinstance(o, dict):
                return {k: cpu(v) for k, v in o.items()}
            if isinstance(o, (list, tuple)):
                return type(o)(cpu(v) for v in o)
            return o
        return {"net_state_dict": cpu(self.net.state_dict()), "optimiser_state_dict": cpu(self.optimiser.state_dict()),
                "scheduler_state_dict": cpu(self.scheduler.state_dict())}

    def load_state(self, ckpt):
        self.net.load_state_dict(ckpt["net_state_dict"])
        self.optimiser.load_state_dict(ckpt["optimiser_state_dict"])     # (moves the momentum buffers to the parameters' device)
        self.scheduler.load_state_dict(ckpt["scheduler_state_dict"])

    def broadcast_state(self, src: int = 0, extra=None):
        """Every rank's trainer becomes rank `src`'s: net (weights, batch-norm statistics), optimiser (momentum buffers,
        learning rate) and scheduler state travel as one object (~0.5 MB for the default net; torch.distributed, RCCL or
        gloo).  The reference has ONE model per generation (training.py:147-153); ranks that trained by themselves would
        drift apart (non-deterministic GPU reductions, unshared shuffles).  `extra` (e.g. the loss) rides along; returns
        rank src's."""
        import torch.distributed as dist
        box = [(self.state(), extra) if dist.get_rank() == src else None]
        on_gpu = dist.get_backend() == "nccl" and self.device.type == "cuda"     # RCCL moves the pickled bytes through this rank's GPU
        dist.broadcast_object_list(box, src=src, device=self.device if on_gpu else None)
        if dist.get_rank() != src:
            self.load_state(box[0][0])
        return box[0][1]

    def _set_valid_rows(self, k):
        from .net import _BatchNorm2d
        for m in self.net.modules():
            if isinstance(m, _BatchNorm2d):
                m.valid_rows = k

    def save(self, folder_path):    # model.py:242-250
        os.makedirs(folder_path, exist_ok=True)
        torch.save({"net_state_dict": self.net.state_dict(),
                    "optimiser_state_dict": self.optimiser.state_dict(),
                    "scheduler_state_dict": self.scheduler.state_dict()}, os.path.join(folder_path, "net.pth"))
