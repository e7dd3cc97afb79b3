#!/usr/bin/env python3
"""How much of a real training window is duplicates, and what merging them costs: ReplayWindow.merged
(c4_window_merge_dev) on windows of real self-play.  The numbers of profiles/window_merge.json.

    python tools/bench_window_merge.py [--generations 12] [--games 1200] [--big-games 8192] [--sims 800] [--repeats 7] [--json OUT]
        Two windows: the one run_generations holds after `generations` generations of `games` games (the net trains one
        epoch per generation, so later generations are played by a net that has learnt something), and one generation of
        `big-games` games.  Per window: positions, distinct positions with and without mirror images, and, `repeats` times
        in alternation in this one process, the seconds of
          * the merge, plain and with equal keys combined inside a wave first (the same bits, or the tool stops),
          * the same merge from torch operations (keys from shifts and masks, torch.unique, index_add_ on int64; it does
            not look for bad rows) -- the same bits again, or the tool stops,
          * one Trainer.train_window epoch over the unmerged and over the merged window.
        Each as median / min / max."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BOTTOM = 0x40810204081
ONE = 2.0 ** 40


def torch_keys(c0, c1):
    import torch

    def flip(p):
        return sum(((p >> (7 * c)) & 0x7f) << (7 * (6 - c)) for c in range(7))

    def key(a, b):
        occ = a | b
        x = occ ^ (occ >> 32)
        for s in (16, 8, 4, 2, 1):
            x = x ^ (x >> s)
        return torch.where((x & 1) == 1, b, a) + occ + BOTTOM
    return key(c0, c1), key(flip(c0), flip(c1))


def torch_merge(boards, targets, policy, mirror=True):
    """merge_host's rule from torch operations, for valid rows."""
    import torch
    n = int(boards.shape[0])
    key, mkey = torch_keys(boards[:, 0], boards[:, 1])
    rev = (key > mkey) if mirror else torch.zeros_like(key, dtype=torch.bool)
    group = torch.where(rev, mkey, key)
    uniq, inverse = torch.unique(group, return_inverse=True)
    g = int(uniq.numel())
    fixed = torch.round(torch.cat([targets[:, None], torch.where(rev[:, None], policy.flip(1), policy)], 1).double() * ONE).long()
    sums = torch.zeros((g, 8), dtype=torch.int64, device=boards.device).index_add_(0, inverse, fixed)
    counts = torch.zeros(g, dtype=torch.int64, device=boards.device).index_add_(0, inverse, torch.ones_like(inverse))
    first = torch.full((g,), n, dtype=torch.int64, device=boards.device).scatter_reduce_(0, inverse, torch.arange(n, device=boards.device), "amin")
    first, order = torch.sort(first)
    sums, counts = sums[order], counts[order]
    mean = (sums.double() / (counts.double() * ONE)[:, None]).float()
    mean = torch.cat([mean[:, :1], torch.where(rev[first][:, None], mean[:, 1:].flip(1), mean[:, 1:])], 1)
    single = (counts == 1)[:, None]
    return (boards[first], torch.where(single[:, 0], targets[first], mean[:, 0]), torch.where(single, policy[first], mean[:, 1:]),
            counts.int())


def same_bits(a, b):
    import torch
    return all(x.shape == y.shape and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)) for x, y in zip(a, b))


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def measure(window, trainer, repeats):
    import torch
    from connect4_amd import engine
    n = window.n_positions
    table = tuple(torch.cat([window._held[g][k] for g in window.generations]) for k in range(3))        # the positions in table order

    def device_merge(mirror, combine):
        b, t, p, c, heads = engine.window_merge(window.table_ptr, window.n_segments, n, window.device, mirror, None, combine)
        d, bad = heads.tolist()
        assert bad == 0
        return b[:d], t[:d], p[:d], c[:d]

    res = {"positions": n, "segments": window.n_segments}
    for mirror in (True, False):
        ref = device_merge(mirror, False)
        assert same_bits(ref, device_merge(mirror, True)), "the wave-combining insert gives other bits"
        assert same_bits(ref, torch_merge(*table, mirror=mirror)), "the torch baseline gives other bits"
        res["distinct" if mirror else "distinct_without_mirror"] = int(ref[3].numel())
        res["largest_group" if mirror else "largest_group_without_mirror"] = int(ref[3].max())
    res["distinct_share"] = res["distinct"] / n
    merged = window.merged()
    runs = {"merge_plain_s": lambda: device_merge(True, False), "merge_wave_combined_s": lambda: device_merge(True, True),
            "merge_torch_ops_s": lambda: torch_merge(*table), "train_epoch_unmerged_s": lambda: trainer.train_window(window),
            "train_epoch_merged_s": lambda: trainer.train_window(merged)}
    times = {k: [] for k in runs}
    state = trainer.state()
    for r in range(repeats + 1):            # (round 0 warms up: allocator, MIOpen's choices for the shapes)
        for name, fn in runs.items():
            trainer.load_state(state)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r:
                times[name].append(time.perf_counter() - t0)
    res.update({k: spread(v) for k, v in times.items()})
    res["merged_rows"], res["unmerged_rows"] = merged.rows, window.rows
    res["wave_combined_over_plain"] = res["merge_wave_combined_s"]["median"] / res["merge_plain_s"]["median"]
    res["torch_ops_over_plain"] = res["merge_torch_ops_s"]["median"] / res["merge_plain_s"]["median"]
    res["merge_over_unmerged_epoch"] = res["merge_plain_s"]["median"] / res["train_epoch_unmerged_s"]["median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--generations", type=int, default=12)
    ap.add_argument("--games", type=int, default=1200)
    ap.add_argument("--big-games", type=int, default=8192)
    ap.add_argument("--sims", type=int, default=800)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--json", default=None, help="also write the result here")
    a = ap.parse_args()
    import torch
    import __graft_entry__ as entry
    entry.build()
    from connect4_amd.config import MCTSConfig
    from connect4_amd.generation import _self_play, run_generations
    from connect4_amd.replay import ReplayWindow
    from connect4_amd.training import ModelConfig, Trainer
    torch.manual_seed(0)
    cfg = MCTSConfig.self_play(a.sims)
    tr = Trainer(ModelConfig(n_training_epochs=1), device="cuda:0")
    res = {"games_per_generation": a.games, "generations": a.generations, "big_games": a.big_games, "sims": a.sims, "repeats": a.repeats,
           "batch_size": tr.config.batch_size}
    with tempfile.TemporaryDirectory(prefix="c4merge_") as d:
        window, _ = run_generations(tr, cfg, a.games, d, a.generations, first_gen=1, n_slots=min(a.games, 4096))
    res["window"] = dict(measure(window, tr, a.repeats), window_generations=window.generations)
    big = _self_play(tr, cfg, a.big_games, 0, a.generations + 1, 0, min(a.big_games, 4096), None)
    one = ReplayWindow("cuda:0")
    one.append(a.generations + 1, big)
    one.select(a.generations + 1)
    res["one_generation"] = measure(one, tr, a.repeats)
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
