"""oracle/replay.py's replay_games_bulk on the CPU, with records the oracle itself played: tapes indexed by game id (the
tape tests) or aligned with the records (production replays, whose game ids index nothing), the net-only evaluator
(engine=None) and PackedGames records, whose float32 values / policies are compared after rounding the oracle's.  A
record that is off by one float32 ulp, or tapes that belong to another game, must fail."""
import zlib
from types import SimpleNamespace

import numpy as np
import pytest


def _answer(c0, c1):
    """A deterministic stand-in for the net: float32 value and priors from a hash of the position."""
    h = zlib.crc32(np.array([c0, c1], dtype=np.uint64).tobytes())
    rng = np.random.RandomState(h)
    p = rng.random_sample(7).astype(np.float32) + np.float32(0.05)
    return np.float32(rng.random_sample()), p / p.sum(dtype=np.float32)


class _Net:
    def evaluate_bits(self, c0, c1, wave=False):
        assert wave
        out = [_answer(int(a), int(b)) for a, b in zip(c0, c1)]
        return np.array([v for v, _ in out], dtype=np.float32), np.array([p for _, p in out], dtype=np.float32)


def _games(oracle, n, ids):
    from oracle import philox_ref as R
    cfg = oracle.make_config(24, root_dirichlet_alpha=0.3, root_exploration_fraction=0.25, num_sampling_moves=6)
    noise, u = R.production_tapes(99, 0.3, ids)
    fn = lambda c0, c1: (lambda v, p: (float(v), [float(x) for x in p], True))(*_answer(c0, c1))  # noqa: E731
    recs = []
    for j in range(n):
        g = oracle.selfplay_game(cfg, oracle.CallbackEvaluator(fn), noise[j], u[j])
        m = len(g["moves"])
        recs.append(SimpleNamespace(game_id=int(ids[j]), length=m, result=g["result"], move=g["moves"],
                                    color0=[b[0] for b in g["boards"]], color1=[b[1] for b in g["boards"]],
                                    value=np.array(g["values"]), policy=np.array(g["policies"])))
    return cfg, recs, noise, u


def _packed(recs):
    import torch
    from connect4_amd.packed import PackedGames
    L = [r.length for r in recs]
    boards = np.array([[a, b] for r in recs for a, b in zip(r.color0, r.color1)], dtype=np.uint64).view(np.int64)
    cat = lambda f, dt: torch.from_numpy(np.concatenate([np.asarray(f(r)) for r in recs]).astype(dt))  # noqa: E731
    return PackedGames(torch.from_numpy(boards), cat(lambda r: r.move, np.uint8), cat(lambda r: r.value, np.float32),
                       cat(lambda r: r.policy, np.float32), cat(lambda r: [0.5 * r.result] * r.length, np.float32),
                       torch.from_numpy(np.repeat(np.arange(len(recs)), L).astype(np.int32)),
                       torch.tensor(L, dtype=torch.int32), torch.tensor([r.result for r in recs], dtype=torch.int8),
                       torch.tensor([r.game_id for r in recs], dtype=torch.int64))


def test_aligned_tapes_net_only_and_packed_records(oracle):
    from oracle.replay import packed_records, replay_games_bulk
    ids = [(1 << 40) + 3, 7, (1 << 33) + 11]              # ids that index no tape array
    cfg, recs, noise, u = _games(oracle, 3, ids)
    res = replay_games_bulk(cfg, None, _Net(), recs, noise, u, threads=2, aligned=True)
    assert res["games"] == 3 and res["positions_asked"] > 0 and res["lost_by_the_table"] == 0
    packed = _packed(recs)
    prec = packed_records(packed)
    assert [r.game_id for r in prec] == ids and all(r.f32 for r in prec)
    assert replay_games_bulk(cfg, None, _Net(), prec, noise, u, aligned=True)["games"] == 3
    sub = packed_records(packed, [2, 0])
    assert [r.game_id for r in sub] == [ids[2], ids[0]]
    assert replay_games_bulk(cfg, None, _Net(), sub, noise[[2, 0]], u[[2, 0]], aligned=True)["games"] == 2
    # one float32 ulp in one policy entry is a mismatch
    k = int(np.argmax(prec[1].policy[0]))
    prec[1].policy[0, k] = np.nextafter(prec[1].policy[0, k], np.float32(2))
    with pytest.raises(AssertionError, match="policies differ"):
        replay_games_bulk(cfg, None, _Net(), prec, noise, u, aligned=True)
    # another game's tapes: the openings differ
    with pytest.raises(AssertionError):
        replay_games_bulk(cfg, None, _Net(), recs, noise[[1, 2, 0]], u[[1, 2, 0]], aligned=True)


def test_tapes_indexed_by_game_id_as_before(oracle):
    from oracle.replay import replay_games_bulk
    cfg, recs, noise, u = _games(oracle, 3, [0, 1, 2])
    assert replay_games_bulk(cfg, None, _Net(), [recs[2], recs[0]], noise, u)["games"] == 2
