"""Helpers shared by the GPU parity tests: drive the HIP engine with a host-side evaluator."""
import functools
from copy import copy

import numpy as np


def table_lookup_fn(c0s, c1s, vs, ps):
    table = {(int(a), int(b)): (np.float32(v), np.asarray(p, dtype=np.float32))
             for a, b, v, p in zip(c0s, c1s, vs, ps)}

    def fn(c0, c1):
        return table[(int(c0), int(c1))]
    return fn


class PlanesAdapter:
    """A planes-fed evaluator with a FusedNet's exact answers: planes [n,3,6,7] (any float dtype) ->
    (values f32 [n], priors f32 [n,7]).  It decodes the planes back to bitboards on the device
    (c4_planes_to_boards_dev) and evaluates those with the fused forward, so a self-play run fed through the
    planes buffer plays the bitboard path's games bit for bit -- unless c4_step emitted wrong planes.  Two
    launches on the current stream and no host synchronisation: it can be captured in a HIP graph.  It does not
    set from_bitboards, so SelfPlay and the searchers treat it like any PyTorch net.  An all-zero row (a slot that
    has not emitted a leaf yet) decodes to the empty board; planes_to_boards counts it as bad, nobody reads that."""

    def __init__(self, fused_net):
        self.net = fused_net

    def __call__(self, planes):
        import torch
        from connect4_amd.engine import planes_to_boards
        boards, _ = planes_to_boards(planes.float())
        n = int(boards.shape[0])
        c0, c1 = boards[:, 0].contiguous(), boards[:, 1].contiguous()
        values = torch.empty(n, dtype=torch.float32, device=planes.device)
        priors = torch.empty((n, 7), dtype=torch.float32, device=planes.device)
        self.net.forward_bitboards(c0.data_ptr(), c1.data_ptr(), n, values, priors)
        return values, priors


def random_undecided_positions(oracle, n, seed, max_plies=30):
    """n seeded random positions of 0..max_plies plies that are not decided, as oracle Boards."""
    rng = np.random.RandomState(seed)
    boards = []
    while len(boards) < n:
        b = oracle.Board.empty()
        for _ in range(int(rng.randint(0, max_plies + 1))):
            m = b.valid_mask()
            if not m or b.result != -1:
                break
            b.make_move(int(rng.choice([c for c in range(7) if (m >> c) & 1])))
        if b.result == -1:
            boards.append(b)
    return boards


def root_fields(r):
    """Every field of a c4_root_result, floats as bit patterns (NaN compares equal to itself)."""
    bits = lambda x: np.asarray(x, dtype=np.float64).view(np.uint64).tolist()  # noqa: E731
    return dict(state=r.state, move=r.move, value=bits(r.value), root_visits=r.root_visits, root_value_sum=bits(r.root_value_sum),
                child_visits=list(r.child_visits), child_value_sum=bits(list(r.child_value_sum)), child_status=list(r.child_status),
                root_prior=bits(list(r.root_prior)), values_policy=bits(list(r.values_policy)), color0=r.color0, color1=r.color1,
                expansions=r.expansions, simulations=r.simulations)


def drive_external(eng, eval_fn, dtype, max_steps=10_000_000):
    """Run an EXTERNAL_* engine to completion with a Python evaluator (c0,c1)->(value, prior[7]).
    Mirrors how evaluators.py:18-25 serves mcts.py:130, one leaf per slot per step.  eval_fn may be a list with one
    evaluator per slot (searches of different evaluators side by side in one engine)."""
    import torch
    G = eng.n_slots
    per_slot = isinstance(eval_fn, (list, tuple))
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    values = torch.zeros(G, dtype=tdt, device="cuda")
    priors = torch.zeros(G, 7, dtype=tdt, device="cuda")
    hv = np.zeros(G, dtype=dtype)
    hp = np.zeros((G, 7), dtype=dtype)
    eng.step(None, None, None)
    n_evals = 0
    for _ in range(max_steps):
        c0, c1, has = eng.read_leaves()
        if not has.any():
            if eng.stats()["active_slots"] == 0:
                break
        for g in np.nonzero(has)[0]:
            v, p = (eval_fn[g] if per_slot else eval_fn)(c0[g], c1[g])
            hv[g] = v
            hp[g] = p
            n_evals += 1
        values.copy_(torch.from_numpy(hv))
        priors.copy_(torch.from_numpy(hp))
        eng.step(values, priors, None)
    else:
        raise RuntimeError("engine did not finish")
    return n_evals


# ---------------------------------------------------------------- position-queue rows
ROW_FIELDS = ("state", "move", "value", "root_visits", "root_value_sum", "child_visits", "child_value_sum", "child_status", "root_prior",
              "values_policy", "color0", "color1", "expansions", "simulations")


def same_rows(got, want, what=""):
    """Two lists of c4_root_result / c4_search_result rows, field for field and bit for bit."""
    assert len(got) == len(want)
    for i in range(len(want)):
        a, b = root_fields(got[i]), root_fields(want[i])
        for f in ROW_FIELDS:
            assert a[f] == b[f], "%s row %d: %s differs: %r != %r" % (what, i, f, a[f], b[f])


@functools.lru_cache(maxsize=None)
def _positions_50():
    from connect4_amd.board import Board
    out = []
    for a in range(7):
        for b in range(7):
            bd = Board()
            bd.make_move(a)
            bd.make_move(b)
            out.append(bd)
    mid = Board()
    for m in (3, 3, 2, 4, 4, 2, 5, 1, 3, 0, 6, 6, 1):
        mid.make_move(m)
    assert mid.result is None
    return tuple(out + [mid])


def positions_50():
    """The 49 two-ply openings and one mid-game position (the same Boards on every call: nobody moves on them)."""
    return list(_positions_50())


# ---------------------------------------------------------------- net-vs-net matches
def game_key(gd):
    """A game (GameData) as comparable Python values: moves, float64 values (None where the reference has None), the
    policies' bits, the boards before each move and the result."""
    return ([int(m) for m in gd.moves], list(gd.values), [np.asarray(p, dtype=np.float64).tobytes() for p in gd.priors],
            [b.to_int_tuple() for b in gd.boards], gd.result.value)


def host_lockstep_games(players, games):
    """`games` -- (opening Board, index of the player moving o, index of the player moving x) -- ply by ply on the host
    lock-step path: at every ply the boards where players[k] is to move are one MCTS.make_moves batch.  Returns GameData in
    the order of `games`."""
    from connect4_amd.training_game import GameData
    boards = [copy(g[0]) for g in games]
    out = [GameData() for _ in games]
    while any(b.result is None for b in boards):
        for k, p in enumerate(players):
            idx = [i for i, b in enumerate(boards) if b.result is None and games[i][1 + b.age % 2] == k]
            if not idx:
                continue
            before = [copy(boards[i]) for i in idx]
            for i, b0, (move, value, tree) in zip(idx, before, p.make_moves([boards[i] for i in idx])):
                out[i].add_move(b0, move, value, tree.get_values_policy())
    for gd, b in zip(out, boards):
        gd.result = b.result
    return out
