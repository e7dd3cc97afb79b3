"""The sliding training window (oinkoink/neural/pytorch/data.py:66-75) kept on the device as packed positions.

The reference rebuilds the window every generation: ``get_dataset`` loads the ``data.pth`` of each of up to 20 generations
and concatenates them.  A materialised position costs 1,072 B (126 + 1 + 7 float32, stored plain and mirrored); the same
position in ``PackedGames`` costs 48 B (two bitboards, the target, seven priors).  ``ReplayWindow`` keeps the packed
form: one *segment* per generation, a small table of their device pointers, and a kernel that builds a training batch
straight from it (c4_window_gather_dev, connect4_amd/csrc/c4_window.hip).

Row order -- the reference's, so that one shuffle means the same batches on both forms: segments newest first, as
``window_generations`` lists them; inside the segment of a generation with n positions, rows [0, n) are its positions as
stored and rows [n, 2n) their left-right mirrors (data.py:78-105 with add_fliplr).  Row r of the window is row r of
``TrainingDataStorage.get_dataset``, bit for bit.

Device-only, like ``PackedGames.training_tensors``: ``locate`` and the bookkeeping are host arithmetic, ``gather`` and
``from_directory`` need a GPU and say so.
"""
import ctypes as C
import os
from typing import List, Optional, Tuple

from . import _lib as L
from .data import window_generations
from .packed import PackedGames

_NO_CPU = ("ReplayWindow.%s runs on the GPU (%s); keep the window on a cuda device -- there is no CPU fallback")


def _same_bits(a, b):
    import torch
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


_BAD_ROWS = ("%d of %d rows cannot be merged: overlapping or floating stones, stones outside the board, or a target or "
             "prior that is not a finite number in [0, 1]")
_BOTTOM = 0x40810204081                 # bit 7 c of every column (c4_board.h)
_BOARD = _BOTTOM * 0x3f                 # the 42 cells
_FIXED_ONE = 2.0 ** 40


def _flip_color(p: int) -> int:
    return sum(((p >> (7 * c)) & 0x7f) << (7 * (6 - c)) for c in range(7))


def _position_key(c0: int, c1: int) -> int:
    occ = c0 | c1
    return (c1 if bin(occ).count("1") & 1 else c0) + occ + _BOTTOM


def merge_host(boards, targets, policy, mirror: bool = True):
    """Identical positions merged into one row each -- the rule c4_window_merge_dev computes (include/c4_engine.h), in
    NumPy with Python integers; no GPU.  boards int64 [n,2], targets float32 [n], policy float32 [n,7] (arrays or
    tensors).  A position's key is mover's stones + occupied + BOTTOM; with `mirror` a group is keyed by the smaller
    of that and its mirror image's key, and a member whose own key is the larger one is *reversed*: its priors count
    for the mirrored columns.  Per group the targets and priors are summed as integers rne(x 2^40) and divided in
    float64 by count 2^40, rounded to float32; a group of one keeps its row bit for bit.  Groups come in the order of
    their first members, with that member's board as stored and, if it is reversed, its column order.
    Returns (boards int64 [g,2], targets float32 [g], policy float32 [g,7], counts int32 [g]); ValueError on bad rows
    (overlapping stones, stones outside the 42 cells or floating, a target or prior not finite or outside [0, 1])."""
    import numpy as np

    def host(x, dtype):
        return np.ascontiguousarray((x.detach().cpu() if hasattr(x, "detach") else x), dtype=dtype)
    b, t, p = host(boards, np.int64), host(targets, np.float32), host(policy, np.float32)
    n = int(b.shape[0])
    if b.shape != (n, 2) or t.shape != (n,) or p.shape != (n, 7):
        raise ValueError("merge_host takes (boards int64 [n,2], targets float32 [n], policy float32 [n,7])")
    if n >= L.WINDOW_MERGE_MAX_POSITIONS:
        raise ValueError("%d positions: the merge's int64 sums hold fewer than %d" % (n, L.WINDOW_MERGE_MAX_POSITIONS))
    tp = np.concatenate([t[:, None], p], axis=1)
    with np.errstate(invalid="ignore"):
        in_range = np.all((tp >= 0) & (tp <= 1), axis=1)                    # (False for NaN and inf)
        fixed = np.rint(tp.astype(np.float64) * _FIXED_ONE)                 # rne(x 2^40), exact in float64
    groups, order, n_bad = {}, [], 0        # group key -> [count, sums[8], first index, first is reversed]
    for i, (c0, c1) in enumerate(b.view(np.uint64).tolist()):
        occ = c0 | c1
        if (c0 & c1) or (occ & ~_BOARD) or (occ & (occ + _BOTTOM)) or not in_range[i]:
            n_bad += 1
            continue
        key = _position_key(c0, c1)
        mkey = _position_key(_flip_color(c0), _flip_color(c1))
        reversed_ = bool(mirror) and key > mkey
        v = [int(x) for x in fixed[i]]
        if reversed_:
            key, v = mkey, v[:1] + v[:0:-1]
        g = groups.get(key)
        if g is None:
            groups[key] = [1, v, i, reversed_]
            order.append(key)
        else:
            g[0] += 1
            g[1] = [x + y for x, y in zip(g[1], v)]
    if n_bad:
        raise ValueError(_BAD_ROWS % (n_bad, n))
    m = len(order)
    ob, ot, op, oc = np.empty((m, 2), np.int64), np.empty(m, np.float32), np.empty((m, 7), np.float32), np.empty(m, np.int32)
    for r, key in enumerate(order):
        count, sums, first, reversed_ = groups[key]
        ob[r], oc[r] = b[first], count
        if count == 1:
            ot[r], op[r] = t[first], p[first]
            continue
        if reversed_:
            sums = sums[:1] + sums[:0:-1]
        mean = [np.float32(np.float64(s) / (np.float64(count) * _FIXED_ONE)) for s in sums]
        ot[r], op[r] = mean[0], mean[1:]
    return ob, ot, op, oc


class ReplayWindow:
    def __init__(self, device=None):
        import torch
        if device is None:          # (without a GPU only the host bookkeeping works)
            device = "cuda" if torch.cuda.is_available() else "cpu"
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._held = {}             # generation -> (boards i64[n,2], targets f32[n], policy f32[n,7])
        self._active: List[int] = []    # the selected generations, newest first
        self._table = None          # device bytes of c4_window_segment[WINDOW_MAX_SEGMENTS]: ONE allocation for the window's life,
        self._counter = None        # so a captured graph that gathers from the window sees a fixed pointer
        self.merge_counts = None    # of a window that merged() made: int32 [n_positions], the members of every row,
        self.merged_from = None     # and the number of positions that went in

    # -- contents --------------------------------------------------------------------------------
    def append(self, gen: int, games_or_tensors):
        """Hold generation `gen`: a PackedGames, or (boards int64 [n,2], targets float32 [n], policy float32 [n,7]), on
        the window's device.  The tensors are referenced, not copied (a non-contiguous one is made contiguous); the
        generation becomes part of the window with the next select()."""
        import torch
        if isinstance(games_or_tensors, PackedGames):
            g = games_or_tensors
            boards, targets, policy = g.boards, g.targets, g.policy
        else:
            boards, targets, policy = games_or_tensors
        n = int(boards.shape[0])
        if (boards.dtype, targets.dtype, policy.dtype) != (torch.int64, torch.float32, torch.float32) or \
                tuple(boards.shape) != (n, 2) or tuple(targets.shape) != (n,) or tuple(policy.shape) != (n, 7):
            raise ValueError("a window segment is (boards int64 [n,2], targets float32 [n], policy float32 [n,7])")
        for t in (boards, targets, policy):
            if t.device.type != "meta" and t.device != self.device:
                raise ValueError("segment tensors live on %s, the window on %s" % (t.device, self.device))
        gen = int(gen)
        if gen in self._held:
            raise ValueError("generation %d is already in the window" % gen)
        self._held[gen] = (boards.contiguous(), targets.contiguous(), policy.contiguous())

    def select(self, gen: int):
        """Make the window that generation `gen` trains on: window_generations(gen) (data.py:66-75) of the generations
        held, newest first.  Generations older than that window are dropped -- the oldest generation of a window never
        moves back as gen grows, so no later window reaches them -- and the segment table is uploaded."""
        wanted = window_generations(int(gen)) or [int(gen)]     # (generation 0: itself, as run_generation trains it)
        for g in [g for g in self._held if g < wanted[-1]]:
            del self._held[g]
        self._activate([g for g in wanted if g in self._held])
        return self

    def _activate(self, gens):
        self._active = list(gens)
        if len(self._active) > L.WINDOW_MAX_SEGMENTS:
            raise ValueError("a window has at most %d segments" % L.WINDOW_MAX_SEGMENTS)
        if self.device.type != "cuda":
            return                              # host bookkeeping only (locate, rows, ...)
        import torch
        table = (L.WindowSegment * L.WINDOW_MAX_SEGMENTS)()
        for i, g in enumerate(self._active):
            b, t, p = self._held[g]
            table[i] = L.WindowSegment(b.data_ptr(), t.data_ptr(), p.data_ptr(), int(b.shape[0]))
        if self._table is None:
            self._table = torch.zeros(C.sizeof(table), dtype=torch.uint8, device=self.device)
            self._counter = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._table.copy_(torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8))

    # -- shape -----------------------------------------------------------------------------------
    @property
    def generations(self) -> List[int]:
        """The selected generations, newest first (the segment order)."""
        return list(self._active)

    @property
    def n_segments(self) -> int:
        return len(self._active)

    @property
    def table_ptr(self) -> int:
        """Device address of the c4_window_segment table (fixed for the window's life; rewritten by select())."""
        if self._table is None:
            raise RuntimeError("no segment table yet: select() a generation on a cuda window first")
        return self._table.data_ptr()

    def _sizes(self):
        return [int(self._held[g][0].shape[0]) for g in self._active]

    @property
    def n_positions(self) -> int:
        return sum(self._sizes())

    @property
    def rows(self) -> int:
        """Rows of the materialised window: every position and its mirror."""
        return 2 * self.n_positions

    @property
    def nbytes(self) -> int:
        """Device memory the window holds: 48 B per position of every generation held, plus the segment table."""
        n = sum(t.numel() * t.element_size() for seg in self._held.values() for t in seg)
        return n + sum(t.numel() * t.element_size() for t in (self._table, self._counter) if t is not None)

    def locate(self, index):
        """Where virtual row(s) `index` come from: (generation, position inside that generation, mirrored).  Host
        arithmetic over the segment sizes; an int gives one tuple, anything iterable a list."""
        if hasattr(index, "tolist"):
            index = index.tolist()
        if isinstance(index, int):
            return self._locate(index)
        return [self._locate(int(i)) for i in index]

    def _locate(self, i: int) -> Tuple[int, int, bool]:
        if not 0 <= i < self.rows:
            raise IndexError("row %d is outside the window's %d rows" % (i, self.rows))
        for g, n in zip(self._active, self._sizes()):
            if i < 2 * n:
                return (g, i - n, True) if i >= n else (g, i, False)
            i -= 2 * n
        raise AssertionError

    # -- batches ---------------------------------------------------------------------------------
    def gather(self, index, out=None, stream=None, check: Optional[bool] = None):
        """(boards F32[m,3,6,7], values F32[m], priors F32[m,7]) = rows `index` (int64 [m]) of the materialised window,
        built by c4_window_gather_dev; `out` = three such tensors to write into.  One launch on `stream` (default: the
        current one).  Called eagerly it then reads the kernel's out-of-range counter (one host synchronisation) and
        raises IndexError when an index was outside [0, rows); under stream capture, or with check=False, nothing is
        counted and such a row is zeros."""
        import torch
        from . import engine as _engine
        if self.device.type != "cuda":
            raise RuntimeError(_NO_CPU % ("gather", "c4_window_gather_dev"))
        if not self._active:
            raise RuntimeError("the window is empty: append() generations and select() one first")
        index = torch.as_tensor(index, dtype=torch.int64).to(self.device).reshape(-1).contiguous()
        m = int(index.numel())
        if out is None:
            out = (torch.empty((m, 3, 6, 7), dtype=torch.float32, device=self.device),
                   torch.empty(m, dtype=torch.float32, device=self.device),
                   torch.empty((m, 7), dtype=torch.float32, device=self.device))
        if check is None:
            check = not torch.cuda.is_current_stream_capturing()
        with torch.cuda.device(self.device):
            if check:
                self._counter.zero_()
            _engine.window_gather(self._table.data_ptr(), len(self._active), index, out[0], out[1], out[2],
                                  self._counter if check else None, stream or 0)
            if check:
                bad = int(self._counter.item())
                if bad:
                    raise IndexError("%d of %d indices are outside the window's %d rows" % (bad, m, self.rows))
        return out

    # -- duplicates ------------------------------------------------------------------------------
    def merged(self, mirror: bool = True, log2_capacity: Optional[int] = None):
        """A new one-segment ReplayWindow on the same device, labelled with the newest active generation, in which
        identical positions of this window (with `mirror`: and their left-right mirror images) are one row carrying the
        mean of their targets and priors -- merge_host's rule, computed by c4_window_merge_dev.  The result also has
        ``merge_counts`` (int32 [rows/2]: members per row) and ``merged_from`` (the positions that went in); gather and
        Trainer.train_window take it as any window.  `log2_capacity`: log2 of the hash table's slots (default: the next
        power of two at or above 2 n_positions; below n_positions is refused).  This window is left untouched.  One
        host synchronisation (the number of distinct positions); ValueError when the window holds bad rows."""
        import torch
        from . import engine as _engine
        if self.device.type != "cuda":
            raise RuntimeError(_NO_CPU % ("merged", "c4_window_merge_dev"))
        if not self._active:
            raise RuntimeError("the window is empty: append() generations and select() one first")
        n = self.n_positions
        if n >= L.WINDOW_MERGE_MAX_POSITIONS:
            raise ValueError("%d positions: the merge's int64 sums hold fewer than %d" % (n, L.WINDOW_MERGE_MAX_POSITIONS))
        with torch.cuda.device(self.device):
            boards, targets, policy, counts, heads = _engine.window_merge(self._table.data_ptr(), len(self._active), n, self.device,
                                                                          mirror, log2_capacity)
            n_distinct, n_bad = heads.tolist()
        if n_bad:
            raise ValueError(_BAD_ROWS % (n_bad, n))
        w = ReplayWindow(self.device)
        gen = self._active[0]
        w.append(gen, (boards[:n_distinct].clone(), targets[:n_distinct].clone(), policy[:n_distinct].clone()))
        w._activate([gen])
        w.merge_counts = counts[:n_distinct].clone()
        w.merged_from = n
        return w

    # -- from disk -------------------------------------------------------------------------------
    @classmethod
    def from_directory(cls, save_dir: str, gen: int, device=None):
        """The window of generation `gen` from the data.pth files under save_dir/<g>/ (data.py:47-75): those of
        window_generations(gen) that exist (lenient, as generation.existing_window).  data.pth stays the one on-disk
        format: each file's first half is turned back into bitboards on the device (c4_planes_to_boards_dev) and accepted
        only if every row is a legal encoding AND gathering all its rows from the packed segment reproduces the file's
        three tensors bit for bit; anything else raises ValueError naming the file."""
        import torch
        from . import engine as _engine
        w = cls(device)
        if w.device.type != "cuda":
            raise RuntimeError(_NO_CPU % ("from_directory", "c4_planes_to_boards_dev"))
        for g in window_generations(int(gen)):
            path = os.path.join(save_dir, str(g), "data.pth")
            if not os.path.exists(path):
                continue
            d = torch.load(path, map_location="cpu", weights_only=True)
            fb, fv, fp = (d[k].to(w.device) for k in ("boards", "values", "priors"))
            rows = int(fb.shape[0])
            if fb.dtype != torch.float32 or tuple(fb.shape[1:]) != (3, 6, 7) or tuple(fv.shape) != (rows,) or tuple(fp.shape) != (rows, 7) \
                    or fv.dtype != torch.float32 or fp.dtype != torch.float32:
                raise ValueError("%s: not the tensors of a data.pth (boards F32[m,3,6,7], values F32[m], priors F32[m,7])" % path)
            if rows % 2:
                raise ValueError("%s: %d rows -- a data.pth holds every position and its mirror" % (path, rows))
            n = rows // 2
            with torch.cuda.device(w.device):
                boards, n_bad = _engine.planes_to_boards(fb[:n])
                n_bad = int(n_bad.item())
            if n_bad:
                raise ValueError("%s: %d of the first %d rows are not the planes of a board" % (path, n_bad, n))
            seg = (boards, fv[:n].clone(), fp[:n].clone())
            if n:
                one = cls(w.device)
                one.append(g, seg)
                one._activate([g])
                gb, gv, gp = one.gather(torch.arange(rows, device=w.device))
                if not (_same_bits(gb, fb) and _same_bits(gv, fv) and _same_bits(gp, fp)):
                    raise ValueError("%s: its rows are not %d positions followed by their mirrors (the packed form does not "
                                     "reproduce the file)" % (path, n))
            w.append(g, seg)
        return w.select(gen)
