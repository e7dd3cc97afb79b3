"""`python bench.py --gpus N` must start N ranks itself: the launcher path, the
rendezvous and the timing contract's MAX/SUM reductions, run here with 2 gloo ranks on CPU
(`--dry-run`: no engine, no GPU; the printed line is flagged dry_run and carries no measurement)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None, timeout=300):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra or {})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, env=env, timeout=timeout,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout     # ONE JSON line, from rank 0
    return json.loads(lines[0])


def test_gpus_2_starts_two_ranks_without_a_wrapper():
    out = _run(["--gpus", "2", "--dry-run"])
    assert out["n_gpus"] == 2 and out["world_size_observed"] == 2 and out["collective_backend"] == "gloo"
    assert out["max_check"] == 2.0      # MAX over ranks of (1 + rank)
    assert out["sum_check"] == 3.0      # SUM over ranks of (rank + 1)
    assert out["dry_run"] is True and out["value"] is None


def test_single_rank_needs_no_process_group():
    out = _run(["--gpus", "1", "--dry-run"])
    assert out["n_gpus"] == 1 and out["world_size_observed"] == 1 and out["collective_backend"] is None


def test_world_size_mismatch_is_an_error():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--dry-run"], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode != 0 and "WORLD_SIZE=2" in p.stderr


def test_plain_run_options():
    import bench
    a = bench.parse_args(["--steps", "7", "--warmup", "0"])
    assert a.steps == 7 and a.warmup == 0 and a.full is False and a.dump_outputs is None
    assert bench.parse_args(["--full", "--dump-outputs", "d"]).full is True
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        try:
            bench.parse_args(bad)
            raise AssertionError("accepted %r" % bad)
        except SystemExit as e:
            assert e.code == 2


def _games(games):
    """PackedGames on the host, ids unsorted, as an export leaves them."""
    import numpy as np
    import torch
    from connect4_amd.packed import PackedGames
    lengths = [3 + (g % 5) for g in range(games)]
    n = sum(lengths)
    gi = np.repeat(np.arange(games), lengths)
    return PackedGames(torch.arange(2 * n, dtype=torch.int64).reshape(n, 2), torch.from_numpy((gi % 7).astype(np.uint8)),
                       torch.from_numpy(gi.astype(np.float32)), torch.full((n, 7), 1.0 / 7.0), torch.full((n,), 0.5),
                       torch.from_numpy(gi.astype(np.int32)), torch.tensor(lengths, dtype=torch.int32),
                       torch.ones(games, dtype=torch.int8), torch.from_numpy((1000 - 7 * np.arange(games)).astype(np.int64)))


def test_write_outputs_float_arrays_and_size_cap(tmp_path, monkeypatch):
    import numpy as np
    import bench
    bench.write_outputs(_games(40).sorted_by_id(), str(tmp_path / "full"))
    a = {k: np.load(str(tmp_path / "full" / (k + ".npy"))) for k in ("boards", "values", "lengths", "ids", "game_index", "game_counts")}
    assert all(x.dtype in (np.float32, np.float64) for x in a.values())
    assert a["game_counts"].tolist() == [40, a["lengths"].sum()] and np.all(np.diff(a["ids"]) > 0)
    assert a["values"][:int(a["lengths"][0])].tolist() == [39.0] * int(a["lengths"][0])    # smallest id = last game
    assert not (tmp_path / "full" / "sampled_games.npy").exists()

    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4096)
    names = bench.write_outputs(_games(40).sorted_by_id(), str(tmp_path / "cut"))
    b = {k: np.load(str(tmp_path / "cut" / (k + ".npy"))) for k in names}
    assert sum(x.nbytes for x in b.values()) <= 4096 and 0 < len(b["lengths"]) < 40
    assert b["lengths"].sum() == len(b["boards"]) == len(b["game_index"])
    assert np.array_equal(np.bincount(b["game_index"].astype(int)), b["lengths"])
    again = bench.write_outputs(_games(40).sorted_by_id(), str(tmp_path / "cut2"))
    assert all(np.array_equal(b[k], np.load(str(tmp_path / "cut2" / (k + ".npy")))) for k in again)   # fixed sample
