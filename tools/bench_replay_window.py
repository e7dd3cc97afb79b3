#!/usr/bin/env python3
"""What the sliding training window costs per generation at a full 20-generation window: generation.run_generation (reloads
every earlier data.pth, copies it to the GPU, torch.cat) against generation.run_generations (replay.ReplayWindow: packed
positions stay on the GPU, batches built by c4_window_gather_dev).  The numbers of profiles/replay_window.json.

    python tools/bench_replay_window.py --games 1200 [--gen 40] [--repeats 3] [--epochs 1] [--sims 800] [--json OUT]
        One self-play generation is played for real; the 19 earlier generations of gen's window are seeded permutations of
        its positions, written as data.pth.  Then, alternating, `repeats` times each from the same trainer state:
        run_generation(gen) and run_generations(first_gen=gen, 1 generation).  Per run: seconds between the end of
        self-play and the first optimiser step (timings' tensors_and_write_s: training tensors, this generation's data.pth,
        and -- parent only -- reload + H2D + cat of the window), ms per train step (train_s / steps), peak
        torch.cuda.max_memory_allocated, and for run_generations the one-time rebuild of the window from disk.
    python tools/bench_replay_window.py --mode steps --games 1200
        One epoch of Trainer.train on the materialised 20-generation window, then one of Trainer.train_window on the
        packed one, nothing else: the run to put under `rocprofv3 --kernel-trace --stats` (gather kernel against the
        indexing kernels of the parent's captured step)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("compare", "steps"), default="compare")
    ap.add_argument("--games", type=int, default=1200)
    ap.add_argument("--slots", type=int, default=None)
    ap.add_argument("--sims", type=int, default=800)
    ap.add_argument("--gen", type=int, default=40, help="the generation measured (>= 39: a 20-generation window)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=1, help="training epochs per generation (the reference: 5)")
    ap.add_argument("--dir", default=None)
    ap.add_argument("--json", default=None, help="also write the result here")
    a = ap.parse_args()
    import torch
    import __graft_entry__ as entry
    entry.build()
    from connect4_amd import engine
    from connect4_amd.config import MCTSConfig
    from connect4_amd.data import window_generations
    from connect4_amd.generation import _self_play, run_generation, run_generations
    from connect4_amd.replay import ReplayWindow
    from connect4_amd.training import ModelConfig, Trainer
    torch.manual_seed(0)
    cfg = MCTSConfig.self_play(a.sims)
    slots = a.slots or min(a.games, 4096)
    tr = Trainer(ModelConfig(n_training_epochs=a.epochs), device="cuda:0")
    bs = tr.config.batch_size
    warm = Trainer(ModelConfig(n_training_epochs=1), device="cuda:0")      # MIOpen's one-time choices for the batch-4096 shapes
    warm.train((torch.rand(2 * bs, 3, 6, 7, device="cuda") > 0.7).float(), torch.rand(2 * bs, device="cuda"),
               torch.softmax(torch.rand(2 * bs, 7, device="cuda"), 1))
    del warm
    base = _self_play(tr, cfg, a.games, 0, 0, 0, slots, None)
    n = base.n_positions
    earlier = window_generations(a.gen)[1:]

    def synthetic(g):
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(g)).cuda()
        return base.boards[perm], base.targets[perm], base.policy[perm]

    res = {"mode": a.mode, "games_per_generation": a.games, "sims": a.sims, "generation": a.gen, "window_generations": 1 + len(earlier),
           "positions_per_generation": n, "epochs": a.epochs, "batch_size": bs}
    if a.mode == "steps":
        segs = {g: synthetic(g) for g in [a.gen] + earlier}
        w = ReplayWindow("cuda:0")
        for g, s in segs.items():
            w.append(g, s)
        w.select(a.gen)
        parts = [engine.training_tensors(*segs[g]) for g in w.generations]
        mat = tuple(torch.cat([p[k] for p in parts]) for k in range(3))
        del parts
        steps = a.epochs * -(-w.rows // bs)
        for name, fn in (("train", lambda: tr.train(*mat)), ("train_window", lambda: tr.train_window(w))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            res[name + "_ms_per_step"] = 1e3 * (time.perf_counter() - t0) / steps
        res.update(rows=w.rows, steps=steps)
    else:
        out = a.dir or tempfile.mkdtemp(prefix="c4window_")
        t0 = time.perf_counter()
        for g in earlier:
            b, v, p = engine.training_tensors(*synthetic(g))
            os.makedirs(os.path.join(out, str(g)), exist_ok=True)
            torch.save({"boards": b.cpu(), "values": v.cpu(), "priors": p.cpu()}, os.path.join(out, str(g), "data.pth"))
        del b, v, p
        res["write_synthetic_generations_s"] = time.perf_counter() - t0
        res["data_pth_bytes"] = os.path.getsize(os.path.join(out, str(earlier[0]), "data.pth"))
        state = tr.state()
        runs = {"run_generation": [], "run_generations": []}
        for _ in range(a.repeats):
            for name in runs:
                tr.load_state(state)
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                t0 = time.perf_counter()
                if name == "run_generation":
                    t = {}
                    run_generation(tr, cfg, a.games, out, gen=a.gen, n_slots=slots, timings=t)
                else:
                    tl = []
                    run_generations(tr, cfg, a.games, out, 1, first_gen=a.gen, n_slots=slots, timings=tl)
                    t = tl[0]
                torch.cuda.synchronize()
                total = time.perf_counter() - t0
                steps = a.epochs * -(-t["training_rows"] // bs)
                runs[name].append({"selfplay_end_to_first_step_s": t["tensors_and_write_s"], "train_s": t["train_s"],
                                   "ms_per_train_step": 1e3 * t["train_s"] / steps, "steps": steps, "training_rows": t["training_rows"],
                                   "selfplay_s": t["selfplay_and_gather_s"],
                                   "outside_the_generation_s": total - t["selfplay_and_gather_s"] - t["tensors_and_write_s"] - t["train_s"],
                                   "peak_memory_allocated_bytes": int(torch.cuda.max_memory_allocated()),
                                   "window_bytes": t.get("window_bytes")})
        res["runs"] = runs
        if a.dir is None:
            import shutil
            shutil.rmtree(out, ignore_errors=True)
        for key in ("selfplay_end_to_first_step_s", "ms_per_train_step", "peak_memory_allocated_bytes"):
            for name, rs in runs.items():
                xs = [r[key] for r in rs]
                res["%s.%s" % (name, key)] = {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}
            res["ratio_of_medians.%s" % key] = res["run_generations.%s" % key]["median"] / res["run_generation.%s" % key]["median"]
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
