"""What the review tests share: the games of tests/golden/review.npz (tests/golden/gen_review_golden.py) as ``PackedGames``.

The file, as its generator printed it: 257 games, 7,628 positions, 92 x wins / 9 draws / 156 o wins, 13 games of 42 plies; at
E = 12 the first 65 games have 219 late rows in 28 games (90 kept, 129 blunders), all 257 have 854 (348 kept, 506 blunders);
at E = 16 all 257 have 1,434 late rows in 196 games -- more than four workgroups of 256 lanes -- and the dearest row takes
3,205 nodes; the 85 games of kind (c) show no blunder; no contradiction anywhere; at E = 20 under a budget of 64 nodes 41 of
the 564 late rows of the first 65 games stay UNKNOWN."""
import numpy as np

BATCHES = (1, 3, 65, 257)
EMPTIES = (1, 8, 12, 16)
PER_POSITION = ("outcome", "kept", "target_agrees")


def positions_of(z, n_games):
    return int(z["lengths"][:n_games].sum())


def games_of(z, n_games, device="cpu"):
    """The first `n_games` games of the file.  values: NaN (no search value is recorded); policy: seeded float32 rows that
    sum to about one, every column positive (a batch's rows are the first rows of the whole file's); targets: the game's
    result value, 0.5 * its code; ids: the game's index."""
    import torch
    from connect4_amd.packed import PackedGames
    m = positions_of(z, n_games)
    moves = np.ascontiguousarray(z["moves"][:m])
    policy = np.random.RandomState(7).rand(len(z["moves"]), 7).astype(np.float32)[:m] + np.float32(0.01)
    policy = (policy / policy.sum(axis=1, keepdims=True)).astype(np.float32)
    gi = np.ascontiguousarray(z["game_index"][:m])
    results = np.ascontiguousarray(z["results"][:n_games])
    t = torch.from_numpy
    games = PackedGames(t(np.ascontiguousarray(z["boards"][:m]).view(np.int64)), t(moves), t(np.full(m, np.nan, dtype=np.float32)), t(policy),
                        t((results[gi].astype(np.float32) * np.float32(0.5))), t(gi), t(np.ascontiguousarray(z["lengths"][:n_games])),
                        t(results), t(np.arange(n_games, dtype=np.int64)))
    return games if device == "cpu" else games.to(device)


def expected(z, empties, n_games):
    """The golden arrays of one review: outcome, kept, target_agrees (per position), by_ply, per_game, nodes (table-free)."""
    m = positions_of(z, n_games)
    out = {k: z["%s_e%d" % (k, empties)][:m] for k in PER_POSITION}
    out["by_ply"] = z["by_ply_e%d_g%d" % (empties, n_games)]
    out["per_game"] = z["per_game_e%d" % empties][:n_games]
    ages = np.array([bin(int(a) | int(b)).count("1") for a, b in z["boards"][:m]], dtype=np.int64)
    out["nodes"] = np.where(42 - ages <= empties, z["nodes_e16"][:m], 0)
    return out


def expected_keep(z, empties, n_games):
    """The oracle's keep mask of the late rows: bool [n, 7], and which rows are late."""
    m = positions_of(z, n_games)
    late = z["outcome_e%d" % empties][:m] >= 0
    return z["keep"][:m] & late[:, None], late


def policy_on_kept(policy, keep, known):
    """The column-order float32 sum of `policy` over `keep`, NaN where not `known`: plain NumPy, one row at a time."""
    out = np.full(len(policy), np.nan, dtype=np.float32)
    for i in np.nonzero(known)[0]:
        acc = np.float32(0.0)
        for c in range(7):
            if keep[i, c]:
                acc = np.float32(acc + policy[i, c])
        out[i] = acc
    return out


def assert_review_equals(review, want, nodes=True):
    for k in PER_POSITION + ("by_ply", "per_game") + (("nodes",) if nodes else ()):
        got = getattr(review, k).cpu().numpy()
        assert got.dtype == want[k].dtype and got.shape == want[k].shape, k
        assert got.tobytes() == np.ascontiguousarray(want[k]).tobytes(), k


def assert_identities(review):
    """by_ply's column sums are the per-position counts, kept + blunders = kept_known, no contradiction, and per_game adds up
    to by_ply."""
    from connect4_amd import _lib as L
    by_ply, per_game = review.by_ply.cpu().numpy(), review.per_game.cpu().numpy()
    status, outcome, kept, agrees = (getattr(review, k).cpu().numpy() for k in ("status", "outcome", "kept", "target_agrees"))
    late = status != L.SOLVE_TOO_DEEP
    sums = by_ply.sum(axis=0)
    assert sums.tolist() == [int(late.sum()), int((outcome >= 0).sum()), int((kept >= 0).sum()), int((kept == 1).sum()), int((kept == 0).sum()),
                             int(agrees.sum()), 0]
    assert (by_ply[:, 3] + by_ply[:, 4] == by_ply[:, 2]).all()
    assert ((status == L.SOLVE_SOLVED) == (outcome >= 0)).all() and not (outcome[~late] >= 0).any() and not (kept[~late] >= 0).any()
    assert per_game[:, :3].sum(axis=0).tolist() == [int(sums[0]), int(sums[2]), int(sums[4])]
    assert ((per_game[:, 3] >= 0) == (per_game[:, 2] > 0)).all()
