"""One training generation on the engine (BASELINE.json configs[4] shape): sharded self-play on every
rank's GPU -> device-side export of the finished games -> all-gather of the packed tensors (RCCL over xGMI)
-> on rank 0: data.pth with flip augmentation built on the device, the reference's train recipe on the sliding
window, checkpoint -> broadcast of the trained state to every rank (one model, as in the reference).  Mirrors TrainingLoop._loop
(oinkoink/neural/training.py:78-153) with the hot path replaced.  The evaluation sets of TrainingLoop._evaluate
(training.py:155-170) are scored here too: after rank 0 has trained and checkpointed, every set of `test_sets` goes through
Trainer.evaluate / evaluate_value_only (statistics accumulated on the device, connect4_amd/stats.py) and the scores are
appended to save_dir/<name>.pkl; `train_stats` keeps the reference's per-epoch training statistics (print_stats).
TrainingLoop._match (training.py:176-207) is here as well: with `match_every`, rank 0 plays the freshly trained net against
the net of ten generations ago -- inside the fused kernel (connect4_amd.match.DeviceMatch) -- or, while gen <= 10, against
evaluate_centre_with_prior on the host lock-step Match, and appends the result to save_dir/match_results.pkl.  Visdom
stays with the reference's loop.  Not in the reference: with `review_empties` rank 0 reviews the generation's games against
exact play (connect4_amd/review.py) before the training tensors are built, appends the summary to save_dir/review.pkl and,
with `exact_targets`, trains on the exact value of every solved late position instead of the game's result (opt-in).  With `exact_leaves` the self-play net is
wrapped in an ExactLeafNet (connect4_amd/exact_leaves.py): the search itself scores late leaves with the solver, on the step
path instead of the fused kernel (opt-in).
"""
import os
import pickle
import time
from typing import Optional

from .config import MCTSConfig
from .data import GameStorage
from .distributed import generate_games_sharded_packed
from .fused_net import make_selfplay_net
from .training import Trainer


def existing_window(save_dir: str, gen: int):
    """Earlier generations of the sliding window (data.py:66-75) whose data.pth is there, newest first.  The reference
    concatenates all of window_generations(gen) and raises when one is missing; a run that starts or resumes at gen >= 3 in
    a directory without them trains on what exists (decided BEFORE self-play is paid for)."""
    from .data import window_generations
    return [g for g in window_generations(gen)[1:] if os.path.exists(os.path.join(save_dir, str(g), "data.pth"))]


def run_generation(trainer: Trainer, config: MCTSConfig, n_games: int, save_dir: Optional[str] = None, gen: int = 0,
                   seed: int = 0, device: int = 0, n_slots: Optional[int] = None, write_games_pkl: bool = False,
                   timings: Optional[dict] = None, precision: Optional[str] = None, test_sets: Optional[dict] = None,
                   train_stats: bool = False, match_every: Optional[int] = None, match_plies: int = 1,
                   review_empties: Optional[int] = None, review_table=None, exact_targets: bool = False,
                   exact_leaves: Optional[int] = None, exact_leaf_budget: Optional[int] = None, match_unlike: bool = False):
    """Returns (PackedGames of all ranks, last_loss).  With torch.distributed initialised every rank plays its shard and
    all ranks receive all games.  There is ONE model, as in the reference (training.py:147-153, model.py:143-147): rank 0
    writes save_dir/<gen>/{data.pth, games.pkl} (storage.py:15-16, data.py:47-64), trains on `trainer.device` over the
    window min(20, int((gen+1)/2)) generations (data.py:66-75; the earlier generations that save_dir holds), writes
    net.pth, and then every rank receives rank 0's net / optimiser / scheduler state (broadcast), so the next
    generation's shards are all played by the same net.  `precision`: see make_selfplay_net (None = the reference's).
    `test_sets` (name -> stats.LabelledSet or the path of a Connect4Dataset file) and `train_stats`: see score_test_sets and
    Trainer.train(stats=True); both are rank 0's work and add no collective.  A path is loaded on every call: a caller that
    loops over run_generation passes LabelledSets (load_test_sets once); run_generations loads each path once.
    `match_every` / `match_plies` / `match_unlike`: see generation_match (rank 0, after the checkpoint, when gen % match_every == 0).
    `review_empties` / `review_table` / `exact_targets`: see review_generation (rank 0, after the games are gathered and
    before the training tensors are built; no collective).  The games returned are the games as played.
    `exact_leaves` / `exact_leaf_budget`: see _self_play; timings["exact_leaves"] holds this rank's counters."""
    import torch
    _check_review_args(review_empties, exact_targets)
    _check_exact_leaf_args(exact_leaves, exact_leaf_budget)
    multi, rank = _ranks()
    test_sets = load_test_sets(test_sets, trainer.device) if rank == 0 else None
    earlier = existing_window(save_dir, gen) if (save_dir is not None and rank == 0) else []
    t0 = time.perf_counter()
    leaf_counters = {}
    games = _self_play(trainer, config, n_games, seed, gen, device, n_slots, precision, exact_leaves, exact_leaf_budget, leaf_counters)
    t1 = time.perf_counter()
    loss, rows = None, 0
    t2 = t1
    review = None
    if rank == 0:
        trained, review = review_generation(games, review_empties, review_table, exact_targets, save_dir, gen)
        boards, values, priors = trained.training_tensors(add_fliplr=True)       # on the device
        if save_dir is not None:
            _write_generation(games, (boards, values, priors), save_dir, gen, write_games_pkl)
            if earlier:   # data.py:66-75: this generation first, then the earlier ones, newest first
                parts = [torch.load(os.path.join(save_dir, str(g), "data.pth"), weights_only=True) for g in earlier]
                boards = torch.cat([boards] + [p["boards"].to(boards.device) for p in parts])
                values = torch.cat([values] + [p["values"].to(values.device) for p in parts])
                priors = torch.cat([priors] + [p["priors"].to(priors.device) for p in parts])
        torch.cuda.synchronize(device)
        t2 = time.perf_counter()
        rows = int(boards.shape[0])
        loss = trainer.train(boards, values, priors, stats=True) if train_stats else trainer.train(boards, values, priors)
        _checkpoint(trainer, save_dir, gen)
    if multi:
        loss = trainer.broadcast_state(src=0, extra=loss)
    t3 = time.perf_counter()
    if timings is not None:
        timings.update(selfplay_and_gather_s=t1 - t0, tensors_and_write_s=t2 - t1, train_s=t3 - t2,
                       positions=int(games.n_positions), training_rows=rows)
        if review is not None:
            timings.update(review)
        if exact_leaves is not None:
            timings["exact_leaves"] = leaf_counters
    if rank == 0:
        _report(trainer, test_sets, train_stats, save_dir, gen, timings)
        if match_every and gen % match_every == 0:
            generation_match(trainer, config, save_dir, gen, device, precision, match_plies, timings, unlike=match_unlike)
    return games, loss


# -- the steps run_generation and run_generations share ---------------------------------------------------------------
def _ranks():
    import torch.distributed as dist
    multi = dist.is_initialized() and dist.get_world_size() > 1
    return multi, (dist.get_rank() if dist.is_initialized() else 0)


def _check_exact_leaf_args(exact_leaves, exact_leaf_budget):
    if exact_leaf_budget is not None and exact_leaves is None:
        raise ValueError("exact_leaf_budget is the budget of exact_leaves: give exact_leaves")


def _self_play(trainer, config, n_games, seed, gen, device, n_slots, precision, exact_leaves=None, exact_leaf_budget=None,
               leaf_counters=None):
    """Every rank plays its shard with the trainer's current weights; all ranks receive all games (finished on return).
    exact_leaves=E: the net is wrapped in ExactLeafNet(net, E, exact_leaf_budget or its default), so the shard is played on
    the step path -- c4_step, forward, overlay, captured in a graph -- instead of the fused kernel, and `leaf_counters`
    (a dict) receives max_empties, node_budget and this rank's counters().  None: nothing changes."""
    import torch
    net = make_selfplay_net(trainer.net.state_dict(), device=device, precision=precision)   # weights are fixed within a generation
    try:
        player = net
        if exact_leaves is not None:
            from .exact_leaves import DEFAULT_NODE_BUDGET, ExactLeafNet
            player = ExactLeafNet(net, exact_leaves, DEFAULT_NODE_BUDGET if exact_leaf_budget is None else exact_leaf_budget)
        games = generate_games_sharded_packed(config, player, n_games, seed=seed + 1000 * gen, device=device, n_slots=n_slots)
        if exact_leaves is not None and leaf_counters is not None:
            leaf_counters.update(max_empties=player.max_empties, node_budget=player.node_budget, **player.counters())
    finally:
        if hasattr(net, "close"):
            net.close()
    torch.cuda.synchronize(device)
    return games


def _check_review_args(review_empties, exact_targets):
    if exact_targets and review_empties is None:
        raise ValueError("exact_targets=True trains on the review's answers: give review_empties")


def review_generation(games, review_empties, review_table, exact_targets, save_dir, gen):
    """The generation's games reviewed against exact play (connect4_amd.review.review_games with max_empties =
    `review_empties`, table = `review_table`); nothing at all with review_empties=None.  Returns (the games to train on,
    None or {"review": the review's summary(), "review_s": seconds} for the generation's timings / report dict); with a
    save_dir the summary and review_s are also appended to save_dir/review.pkl (append_history).  The games to train on are
    `games` themselves unless `exact_targets`: then ``games.with_exact_targets(review)`` -- data.pth, the replay window's
    segment and the training rows carry the exact value of every solved late position; games.pkl keeps the games as played.
    Opt-in: whether exact targets train a stronger net has not been measured."""
    if review_empties is None:
        return games, None
    from .review import review_games
    t0 = time.perf_counter()
    review = review_games(games, max_empties=review_empties, table=review_table)
    summary = review.summary()
    seconds = time.perf_counter() - t0
    if save_dir is not None:
        os.makedirs(save_dir, exist_ok=True)
        append_history(os.path.join(save_dir, "review.pkl"), gen, dict(summary, review_s=seconds))
    return (games.with_exact_targets(review) if exact_targets else games), {"review": summary, "review_s": seconds}


def _write_generation(games, tensors, save_dir, gen, write_games_pkl):
    """save_dir/<gen>/{data.pth, games.pkl} (storage.py:15-16, data.py:47-64) from the device tensors of this generation."""
    import torch
    boards, values, priors = tensors
    folder = os.path.join(save_dir, str(gen))
    os.makedirs(folder, exist_ok=True)
    if write_games_pkl:
        GameStorage().save(games, folder)
    torch.save({"boards": boards.cpu(), "values": values.cpu(), "priors": priors.cpu()}, os.path.join(folder, "data.pth"))


def _checkpoint(trainer, save_dir, gen):
    import torch
    if save_dir is not None:
        trainer.save(os.path.join(save_dir, str(gen)))
    if trainer.device.type == "cuda":
        torch.cuda.synchronize(trainer.device)


# -- scores after a generation (training.py:155-170) ------------------------------------------------------------------
def load_test_sets(test_sets, device):
    """name -> LabelledSet, the paths among the values loaded (stats.LabelledSet.load) onto `device`."""
    if not test_sets:
        return {}
    from .stats import LabelledSet
    return {name: s if not isinstance(s, (str, os.PathLike)) else LabelledSet.load(s, device=device) for name, s in test_sets.items()}


def score_test_sets(trainer, test_sets, save_dir=None, gen=0):
    """TrainingLoop._evaluate: every set scored by the trainer's net -- Trainer.evaluate, or evaluate_value_only for a set
    without priors (the reference's 7- and 8-ply sets) -- as {name: to_dict() of plain Python numbers}.  With a save_dir each
    result is also appended to save_dir/<name>.pkl: a pickled list of {"generation": gen, **to_dict()}, the reference's
    8ply.pkl / 7ply.pkl without pandas.  The file is re-read and extended (a resumed run goes on where it stopped).  The
    file follows the run: an entry of this generation is replaced, and entries of LATER generations -- left by a run that
    is being redone from an explicit lower first_gen -- are dropped, as their checkpoints are about to be overwritten."""
    from .stats import plain_dict
    out = {}
    for name, data in test_sets.items():
        priors = data.priors if hasattr(data, "priors") else (data[2] if len(data) > 2 else None)
        st = trainer.evaluate(data) if priors is not None else trainer.evaluate_value_only(data)
        out[name] = plain_dict(st)
        if save_dir is not None:
            append_history(os.path.join(save_dir, "%s.pkl" % name), gen, out[name])
    return out


def append_history(path, gen, row):
    """The history files of a run (score_test_sets' <name>.pkl, generation_match's match_results.pkl): a pickled list of
    {"generation": gen, **row}, re-read and extended.  An entry of this generation is replaced and entries of later
    generations are dropped; the file is replaced atomically.  Returns the list written."""
    history = []
    if os.path.exists(path):
        with open(path, "rb") as f:
            history = [e for e in pickle.load(f) if e["generation"] < gen]
    history.append(dict(generation=int(gen), **row))
    history.sort(key=lambda e: e["generation"])
    with open(path + ".tmp", "wb") as f:
        pickle.dump(history, f)
    os.replace(path + ".tmp", path)
    return history


# -- strength after a generation (training.py:176-207) ----------------------------------------------------------------
def generation_match(trainer, config, save_dir, gen, device=0, precision=None, plies=1, timings=None, unlike=False):
    """TrainingLoop._match: the trainer's net ("AlphaZero", the run's simulations / pb_c_base / pb_c_init, no noise, no
    sampled moves) against "Evaluate_centre_with_prior" while gen <= 10 and against "Older net" -- save_dir/<gen-10>/net.pth,
    MCTSConfig(simulations) -- afterwards, as Match(plies, switch=True).  Two nets meet inside the fused kernel
    (match.DeviceMatch); the centre opponent, and any pairing the device path refuses (match.device_match_reason), go
    through the host lock-step Match.  `unlike` is handed on to play_match: the players are then described to the engine one
    by one, so the two searches need not agree and a 64-filter reference-precision run ("f32x3w") plays on the device too, in
    the split match kernel.  The result -- wins / draws / losses / return from the new net's side -- is appended
    to save_dir/match_results.pkl (append_history) and, with "opponent" and the "path" taken ("device" / "host"), put into
    timings["match"].  Rank 0's work; no collective."""
    import torch
    from .evaluators import DeviceNetEvaluator, Evaluator, evaluate_centre_with_prior
    from .match import play_match
    from .mcts import MCTS
    nets = [make_selfplay_net(trainer.net.state_dict(), device=device, precision=precision)]
    players = [MCTS("AlphaZero", MCTSConfig(config.simulations, config.pb_c_base, config.pb_c_init),
                    DeviceNetEvaluator(nets[0], device), device=device)]
    try:
        if gen <= 10:
            players.append(MCTS("Evaluate_centre_with_prior", MCTSConfig(config.simulations), Evaluator(evaluate_centre_with_prior),
                                device=device))
        else:
            if save_dir is None:
                raise ValueError("the match of generation %d needs save_dir/%d/net.pth" % (gen, gen - 10))
            old = torch.load(os.path.join(save_dir, str(gen - 10), "net.pth"), map_location="cpu", weights_only=True)
            nets.append(make_selfplay_net(old["net_state_dict"], device=device, precision=precision))
            players.append(MCTS("Older net", MCTSConfig(config.simulations), DeviceNetEvaluator(nets[1], device), device=device))
        t0 = time.perf_counter()
        result, path = play_match(False, players[0], players[1], plies=plies, switch=True, **({"unlike": True} if unlike else {}))
        seconds = time.perf_counter() - t0
    finally:
        for p in players:
            if p._searcher is not None:
                p._searcher.close()
        for n in nets:
            if hasattr(n, "close"):
                n.close()
    row = {k: (float(v) if k == "return" else int(v)) for k, v in result.items()}
    if save_dir is not None:
        append_history(os.path.join(save_dir, "match_results.pkl"), gen, row)
    if timings is not None:
        timings["match"] = dict(row, opponent=players[1].name, path=path, match_s=seconds)
    return row, path


def _report(trainer, test_sets, train_stats, save_dir, gen, timings):
    """Rank 0, after the checkpoint: test-set scores and per-epoch training statistics into the generation's timings dict."""
    from .stats import plain_dict
    scores = score_test_sets(trainer, test_sets, save_dir, gen) if test_sets else {}
    if timings is not None:
        timings.update(scores)
        if train_stats:
            timings["train_stats"] = [plain_dict(s) for s in trainer.epoch_stats]


# -- many generations: the window stays on the device -----------------------------------------------------------------
def latest_generation(save_dir: str):
    """(next generation, path of the net.pth to resume from or None): the resume rule of TrainingLoop.__init__
    (oinkoink/neural/training.py:31-47) over the integer-named subdirectories of save_dir.  With MORE THAN ONE of them, the
    largest g is the last generation; when g/net.pth is missing (the run died between data.pth and the checkpoint) g - 1
    is, and when that has no net.pth either FileNotFoundError is raised; the next generation is the one after it.
    Otherwise -- no subdirectory, or exactly one: the reference applies its rule only to more than one and so starts a
    directory that holds a single generation over, which is reproduced here -- (1, None).  Subdirectories whose names
    are not integers are ignored (the reference raises on them)."""
    gens = []
    if os.path.isdir(save_dir):
        for f in os.scandir(save_dir):
            if f.is_dir():
                try:
                    gens.append(int(f.name))
                except ValueError:
                    pass
    if len(gens) <= 1:
        return 1, None
    g = max(gens)
    path = os.path.join(save_dir, str(g), "net.pth")
    if not os.path.exists(path):
        g -= 1
        path = os.path.join(save_dir, str(g), "net.pth")
        if not os.path.exists(path):
            raise FileNotFoundError("no net.pth in generation %d or %d of %s" % (g + 1, g, save_dir))
    return g + 1, path


def run_generations(trainer: Trainer, config: MCTSConfig, n_games: int, save_dir: str, n_generations: int,
                    first_gen: Optional[int] = None, seed: int = 0, device: int = 0, n_slots: Optional[int] = None,
                    precision: Optional[str] = None, write_games_pkl: bool = False, timings: Optional[list] = None,
                    test_sets: Optional[dict] = None, train_stats: bool = False, match_every: Optional[int] = None,
                    match_plies: int = 1, review_empties: Optional[int] = None, review_table=None, exact_targets: bool = False,
                    exact_leaves: Optional[int] = None, exact_leaf_budget: Optional[int] = None, merge_duplicates: bool = False,
                    merge_mirror: bool = True, match_unlike: bool = False):
    """n_generations generations of run_generation -- same seeds (seed + 1000 * gen), same files (data.pth, net.pth,
    optional games.pkl), same broadcast of the trained state -- with the sliding window (data.py:66-75) kept on rank 0's GPU
    as packed positions (replay.ReplayWindow): each generation's games are appended to it and trained with
    Trainer.train_window; no earlier data.pth is read back and no materialised window is concatenated (48 B instead
    of 1,072 B per position, nothing reloaded).  The batches are those of run_generation: row r of the window is row r of
    the concatenated files.

    first_gen=None resumes save_dir by the reference's rule (latest_generation): the trainer loads that net.pth and the
    window is rebuilt from the data.pth files (ReplayWindow.from_directory; each file is verified).  An explicit
    first_gen starts there with the trainer as it is and, like run_generation, with what earlier generations save_dir
    holds.  `timings`: a list that receives one dict per generation -- run_generation's keys, plus window_rows and
    window_bytes, and with `test_sets` / `train_stats` (as run_generation: scored on rank 0 after each checkpoint, appended
    to save_dir/<name>.pkl) the sets' names and train_stats, and with `match_every` (generation_match on rank 0 after the
    checkpoint of every generation with gen % match_every == 0, `match_unlike` as there; save_dir/match_results.pkl) "match", and with `review_empties`
    (review_generation, as run_generation; with `exact_targets` the window's segment carries the exact targets) "review" and
    "review_s", and with `exact_leaves` (as run_generation) "exact_leaves".  With `merge_duplicates` each generation trains on
    window.merged(mirror=merge_mirror) -- identical positions (and, with merge_mirror, mirror images) as one row with the mean
    of their targets and priors -- while the unmerged window is the one kept and appended to and data.pth is what it is
    without the option; `timings` then has "window_distinct" (the merged window's positions; training_rows is twice that) and
    "merge_s".  Returns (the window -- None on other ranks --, [last loss of each generation])."""
    import torch
    from .replay import ReplayWindow
    _check_review_args(review_empties, exact_targets)
    _check_exact_leaf_args(exact_leaves, exact_leaf_budget)
    multi, rank = _ranks()
    os.makedirs(save_dir, exist_ok=True)
    test_sets = load_test_sets(test_sets, trainer.device) if rank == 0 else None
    if first_gen is None:
        first_gen, net_path = latest_generation(save_dir)
        if net_path is not None:
            if rank == 0:
                trainer.load_state(torch.load(net_path, map_location=trainer.device, weights_only=True))
            if multi:
                trainer.broadcast_state(src=0)
    window = None
    if rank == 0:       # window_generations(first_gen - 1) covers the earlier generations of first_gen's window
        window = ReplayWindow.from_directory(save_dir, first_gen - 1, trainer.device) if first_gen > 1 else ReplayWindow(trainer.device)
    losses = []
    for gen in range(first_gen, first_gen + n_generations):
        t0 = time.perf_counter()
        leaf_counters = {}
        games = _self_play(trainer, config, n_games, seed, gen, device, n_slots, precision, exact_leaves, exact_leaf_budget, leaf_counters)
        t1 = time.perf_counter()
        loss, rows, nbytes = None, 0, 0
        t2 = t1
        review = None
        if rank == 0:
            trained, review = review_generation(games, review_empties, review_table, exact_targets, save_dir, gen)
            _write_generation(games, trained.training_tensors(add_fliplr=True), save_dir, gen, write_games_pkl)
            window.append(gen, tuple(t.to(window.device) for t in (trained.boards, trained.targets, trained.policy)))
            window.select(gen)
            torch.cuda.synchronize(device)
            t2 = time.perf_counter()
            rows, nbytes = window.rows, window.nbytes
            trained_on = window
            if merge_duplicates:
                trained_on = window.merged(mirror=merge_mirror)
                torch.cuda.synchronize(device)
                merge_report = dict(window_distinct=trained_on.n_positions, training_rows=trained_on.rows, merge_s=time.perf_counter() - t2)
            loss = trainer.train_window(trained_on, stats=True) if train_stats else trainer.train_window(trained_on)
            _checkpoint(trainer, save_dir, gen)
        if multi:
            loss = trainer.broadcast_state(src=0, extra=loss)
        t3 = time.perf_counter()
        losses.append(loss)
        report = dict(generation=gen, selfplay_and_gather_s=t1 - t0, tensors_and_write_s=t2 - t1, train_s=t3 - t2,
                      positions=int(games.n_positions), training_rows=rows, window_rows=rows, window_bytes=nbytes)
        if review is not None:
            report.update(review)
        if exact_leaves is not None:
            report["exact_leaves"] = leaf_counters
        if merge_duplicates and rank == 0:
            report.update(merge_report)
        if rank == 0:
            _report(trainer, test_sets, train_stats, save_dir, gen, report)
            if match_every and gen % match_every == 0:
                generation_match(trainer, config, save_dir, gen, device, precision, match_plies, report, unlike=match_unlike)
        if timings is not None:
            timings.append(report)
    return window, losses
