"""The review of finished games against exact play on the device (connect4_amd/review.py, c4_review_*_dev) against
tests/golden/review.npz -- labels from the exhaustive oracle alone, node counts and tight-budget statuses from the host
mirror (tests/golden/gen_review_golden.py) -- and its use in run_generation(s) and tools/review_games.py."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

import review_cases as RC
from conftest import load_npz

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def z():
    f = load_npz("review.npz")
    return {k: f[k] for k in f.files}


@pytest.fixture(scope="module")
def batches(z):
    return {b: RC.games_of(z, b, "cuda") for b in RC.BATCHES}


@pytest.mark.parametrize("per_launch", [16, None])
@pytest.mark.parametrize("n_games", RC.BATCHES)
def test_device_review_equals_the_golden_file(z, batches, n_games, per_launch):
    from connect4_amd.review import review_games
    for empties in RC.EMPTIES:
        r = review_games(batches[n_games], max_empties=empties, nodes_per_launch=per_launch)
        assert r.status.device.type == "cuda"
        RC.assert_review_equals(r, RC.expected(z, empties, n_games))
        RC.assert_identities(r)
        assert r.report["contradictions"] == 0 and r.report["unknown"] == 0 and r.report["chain_errors"] == 0
        assert r.exact_targets.cpu().numpy().tobytes() == np.where(
            r.outcome.cpu().numpy() >= 0, r.outcome.cpu().numpy() * np.float32(0.5), batches[n_games].targets.cpu().numpy()).astype(np.float32).tobytes()


def test_device_review_equals_the_host_mirror(z, batches):
    """Every field and the report's counts, at a cut-off the file has no row for, and the two ends."""
    from connect4_amd import _lib as L
    from connect4_amd.review import review_games, review_host
    games = batches[65]
    for empties in (0, 10):
        dev, host = review_games(games, max_empties=empties), review_host(games, max_empties=empties)
        for k in ("status", "outcome", "kept", "target_agrees", "nodes", "by_ply", "per_game", "exact_targets", "distinct_boards",
                  "distinct_status", "distinct_outcome"):
            assert getattr(dev, k).cpu().equal(getattr(host, k)), k
        assert {k: v for k, v in dev.report.items() if k != "seconds"} == {k: v for k, v in host.report.items() if k != "seconds"}
        assert dev.summary() == host.summary()
    every = review_games(games, max_empties=42, node_budget=64)
    assert set(every.status.cpu().tolist()) == {L.SOLVE_SOLVED, L.SOLVE_UNKNOWN}
    RC.assert_identities(every)


@pytest.mark.parametrize("log2", [10, 20])
def test_a_table_changes_no_answer(z, batches, log2):
    from connect4_amd.review import review_games
    from connect4_amd.solver import Table
    with Table(log2) as table:
        for run in ("cold", "warm"):
            for empties in (12, 16):
                r = review_games(batches[257], max_empties=empties, table=table)
                RC.assert_review_equals(r, RC.expected(z, empties, 257), nodes=False)
                RC.assert_identities(r)
        assert r.report["table_hits"] > 0 and r.report["table_log2_entries"] == log2


def test_tight_budget(z, batches):
    from connect4_amd import _lib as L
    from connect4_amd.review import review_games
    e, budget, n_games = (int(v) for v in z["tight"])
    r = review_games(batches[n_games], max_empties=e, node_budget=budget)
    assert r.status.cpu().numpy().tobytes() == z["status_e20_b64"].tobytes()
    RC.assert_identities(r)
    known = r.outcome.cpu().numpy() >= 0
    gi = batches[n_games].game_index.cpu().numpy()
    same_game = np.zeros(len(known), dtype=bool)
    same_game[:-1] = gi[1:] == gi[:-1]
    assert ((r.kept.cpu().numpy() >= 0) == (known & np.where(same_game, np.roll(known, -1), True))).all()
    assert r.report["unknown"] == int((z["status_e20_b64"] == L.SOLVE_UNKNOWN).sum()) > 0


@pytest.mark.parametrize("n_games,empties", [(65, 8), (257, 16)])
def test_keep_masks_equal_the_oracle(z, batches, n_games, empties):
    from connect4_amd.review import review_games
    games = batches[n_games]
    r = review_games(games, max_empties=empties, moves=True)
    RC.assert_review_equals(r, RC.expected(z, empties, n_games))        # stage 1 is the search already made: the same node counts
    want, late = RC.expected_keep(z, empties, n_games)
    assert r.keep.cpu().numpy().tobytes() == want.tobytes() and r.keep_known.cpu().numpy().tobytes() == late.tobytes()
    policy = games.policy.cpu().numpy()
    assert r.policy_on_kept.cpu().numpy().tobytes() == RC.policy_on_kept(policy, want, late).tobytes()
    priors = np.where(late[:, None], want / np.maximum(want.sum(axis=1), 1)[:, None].astype(np.float32), policy).astype(np.float32)
    assert r.exact_priors.cpu().numpy().tobytes() == priors.tobytes()
    new = games.with_exact_targets(r, priors=True)
    assert new.policy.equal(r.exact_priors) and new.targets.equal(r.exact_targets) and new.boards is games.boards
    assert r.report["stage2_rows"] > 0 and r.summary()["policy_on_kept_rows"] == int(late.sum())


def test_refusals_and_chain_errors(z, batches):
    from test_review_host import broken_batches
    from connect4_amd.review import review_games
    from connect4_amd.solver import Table
    for bad in (-1, 43):
        with pytest.raises(ValueError, match="max_empties"):
            review_games(batches[3], max_empties=bad)
    with pytest.raises(ValueError, match="host=True"):
        review_games(batches[3].cpu())
    with Table(10) as table:
        table.device = 1        # as if it lived elsewhere
        try:
            with pytest.raises(ValueError, match="table lives on device"):
                review_games(batches[3], table=table)
        finally:
            table.device = 0
    with pytest.raises(ValueError, match="keep mask"):
        batches[3].with_exact_targets(review_games(batches[3]), priors=True)
    for name, games, row in broken_batches(z):
        with pytest.raises(ValueError, match=r"row %d breaks" % row):
            review_games(games.to("cuda"), max_empties=8)


def test_labelled_set_is_scored(z, batches):
    from connect4_amd.fused_net import make_selfplay_net
    from connect4_amd.net import random_init_state_dict
    from connect4_amd.review import review_games
    from connect4_amd.stats import score
    r = review_games(batches[65], max_empties=12)
    ls = r.labelled_set()
    assert len(ls) == r.report["distinct"] > 0 and ls.device.type == "cuda" and ls.priors is None
    net = make_selfplay_net(random_init_state_dict(seed=0), device=0)
    try:
        st = score(net, ls)
    finally:
        if hasattr(net, "close"):
            net.close()
    assert st.n == len(ls) and sum(st.total.values()) == len(ls)


# -- the training loop -------------------------------------------------------------------------------------------------------
def _trainer():
    from connect4_amd.training import ModelConfig, Trainer
    torch.manual_seed(0)
    return Trainer(ModelConfig(batch_size=256, n_training_epochs=2, use_gpu=True))


def _tool(*args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "review_games.py")] + [str(a) for a in args], cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    return out.stdout


def test_run_generation_reviews_and_trains_on_exact_targets(tmp_path):
    from connect4_amd.config import MCTSConfig
    from connect4_amd.generation import run_generation
    from connect4_amd.review import review_host
    cfg = MCTSConfig.self_play(16)
    plain, reviewed, exact = (str(tmp_path / k) for k in ("plain", "reviewed", "exact"))
    t0, t1, t2 = {}, {}, {}
    g0, _ = run_generation(_trainer(), cfg, 16, plain, gen=1, n_slots=16, timings=t0)
    g1, _ = run_generation(_trainer(), cfg, 16, reviewed, gen=1, n_slots=16, timings=t1, review_empties=8, write_games_pkl=True)
    g2, _ = run_generation(_trainer(), cfg, 16, exact, gen=1, n_slots=16, timings=t2, review_empties=16, exact_targets=True)
    # the same games every time; the review in the timings and in review.pkl
    assert all(getattr(g0, k).equal(getattr(g1, k)) and getattr(g0, k).equal(getattr(g2, k)) for k in ("boards", "moves", "targets", "results"))
    want = review_host(g1, max_empties=8)
    assert "review" not in t0 and not os.path.exists(os.path.join(plain, "review.pkl"))
    want16 = review_host(g2, max_empties=16)
    assert t1["review"] == want.summary() and t2["review"] == want16.summary() and t1["review_s"] > 0 and t1["review"]["late"] > 0
    with open(os.path.join(reviewed, "review.pkl"), "rb") as f:
        history = pickle.load(f)
    assert len(history) == 1 and history[0]["generation"] == 1 and {k: v for k, v in history[0].items() if k not in ("generation", "review_s")} == want.summary()
    # without exact_targets every byte is the parent's; with them the values are the exact targets, both halves
    d0, d1, d2 = (torch.load(os.path.join(d, "1", "data.pth"), weights_only=True) for d in (plain, reviewed, exact))
    assert all(d0[k].equal(d1[k]) for k in ("boards", "values", "priors"))
    with open(os.path.join(plain, "1", "data.pth"), "rb") as a, open(os.path.join(reviewed, "1", "data.pth"), "rb") as b:
        assert a.read() == b.read()
    n = g0.n_positions
    targets = want16.exact_targets
    assert d2["values"].shape == (2 * n,) and d2["values"][:n].equal(targets) and d2["values"][n:].equal(targets)
    assert d2["boards"].equal(d0["boards"]) and d2["priors"].equal(d0["priors"])
    # the values differ from the games' results exactly where the review says a target disagrees
    s16 = want16.summary()
    print("exact targets: %d late rows, %d agree with the game's result" % (s16["late"], s16["target_agrees"]))
    assert d2["values"].equal(d0["values"]) == (s16["target_agrees"] == s16["late"])
    assert int((d2["values"][:n] != d0["values"][:n]).sum()) == s16["late"] - s16["target_agrees"]
    # the tool on the run directory prints the same summary
    printed = json.loads(_tool(reviewed, "--generation", 1, "--max-empties", 8, "--json"))
    assert printed["summary"] == json.loads(json.dumps(want.summary()))


def test_run_generations_puts_exact_targets_into_the_window(tmp_path):
    from connect4_amd.config import MCTSConfig
    from connect4_amd.generation import run_generations
    from connect4_amd.review import review_host
    d = str(tmp_path)
    timings = []
    tr = _trainer()
    seen = []
    inner = tr.train_window

    def spy(window, generator=None):
        seen.append(tuple(t.clone() for t in window.gather(torch.arange(window.rows, device=window.device))))
        return inner(window, generator)
    tr.train_window = spy
    # generation 3 is the first whose window (data.py:66-75) has two generations, 3 and 2: the second segment is generation 2's
    window, _ = run_generations(tr, MCTSConfig.self_play(16), 16, d, 3, first_gen=1, n_slots=16, timings=timings, review_empties=8,
                                exact_targets=True, write_games_pkl=True)
    assert len(timings) == 3 and all(t["review"]["max_empties"] == 8 and t["review_s"] > 0 for t in timings)
    with open(os.path.join(d, "review.pkl"), "rb") as f:
        assert [e["generation"] for e in pickle.load(f)] == [1, 2, 3]
    from connect4_amd.data import GameStorage
    from connect4_amd.packed import PackedGames
    assert window.generations == [3, 2]
    values = seen[2][1].cpu()
    at = 0
    for gen in (3, 2):
        packed = PackedGames.from_game_data(GameStorage().load(os.path.join(d, str(gen))))
        exact = review_host(packed, max_empties=8).exact_targets
        n = packed.n_positions
        assert values[at:at + n].equal(exact) and values[at + n:at + 2 * n].equal(exact), gen
        assert packed.targets.equal(packed.results[packed.game_index.long()].float() * 0.5)     # games.pkl keeps the games as played
        at += 2 * n
    assert at == values.numel()
