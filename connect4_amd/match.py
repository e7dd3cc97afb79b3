"""Strength-evaluation harness: the reference's Match
(oinkoink/match.py:15-70) over all `plies`-deep openings, both colours, scored from player_1's side.

Where the reference plays the games one after another (or in a process Pool, match.py:72-76), all
games here advance in lock-step: at every ply the boards waiting for player_1 form one GPU batch
(``MCTS.make_moves``), likewise for player_2.  Players without ``make_moves`` are called per board.

``DeviceMatch`` plays the same games inside the fused kernel (c4_match_steps): one slot per game, one launch per net
and round, no launch per simulation.  It serves matches between two noise-free ``MCTS`` players over ``FusedNet``s
(``device_match_reason`` lists the rules); ``play_match`` picks it when it can and ``Match`` otherwise, and
``tournament`` plays every pairing of a list of such players in ONE engine (scripts/matches.py's table).

By default the players of a device match are alike in every respect (net shape, precision, search config) and meet in
c4_match_wave_kernel.  ``unlike=True`` drops that: every player is described to the engine on its own
(c4_match_configure: its simulations, pb_c_base, pb_c_init and its match kernel), so nets of different filters, blocks
and precisions -- the 64-filter "f32x3w" among them, in c4_match_split_kernel -- and searches of different sizes meet in
one engine.  ``kernel`` ("wave" / "split") puts every net on one kernel.
"""
import time
from copy import copy

import numpy as np

from .board import make_random_ips


def _moves(player, boards):
    if not boards:
        return
    if hasattr(player, "make_moves"):
        player.make_moves(boards)
    else:
        for b in boards:
            player.make_move(b)


class Match:
    def __init__(self, display, player_1, player_2, plies: int = 0, switch: bool = False):
        self._player_1 = player_1
        self._player_2 = player_2
        ips = sorted(make_random_ips(plies), key=lambda b: b.to_int_tuple())
        # (board, player moving o, player moving x); switched games swap the colours (match.py:33-40)
        self.games = [(copy(b), player_1, player_2) for b in ips]
        self.n = len(self.games)
        if switch:
            self.games += [(copy(b), player_2, player_1) for b in ips]
        self.switch = switch
        self.display = display

    def play(self, agents=1):
        boards = [g[0] for g in self.games]
        while True:
            live = [i for i, b in enumerate(boards) if b.result is None]
            if not live:
                break
            for player in (self._player_1, self._player_2):
                todo = [boards[i] for i in live if boards[i].result is None and
                        (self.games[i][1] if boards[i].age % 2 == 0 else self.games[i][2]) is player]
                _moves(player, todo)
        results = np.array([b.result.value for b in boards], dtype="f")
        if self.switch:                       # flip the games where player_2 moved first (match.py:53-56)
            results[self.n:] *= -1.0
            results[self.n:] += 1.0
        wins = int(np.sum(results == 1))
        draws = int(np.sum(results == 0.5))
        losses = int(np.sum(results == 0))
        return_ = (1.0 * wins + 0.5 * draws) / (wins + draws + losses)
        if self.display:
            print("The results for {} vs {} are: {} wins, {} draws, {} losses, {:.3f} return".format(
                self._player_1.name, self._player_2.name, wins, draws, losses, return_))
        return {"wins": wins, "draws": draws, "losses": losses, "return": return_}


# -- matches inside the fused kernel ----------------------------------------------------------------------------------
def score_results(results, n, switch):
    """match.py:51-70 on the games' results (o's point of view, one per game in Match.games order; the first n games have
    player_1 on o): the games where player_2 moved first are flipped, then wins / draws / losses / return of player_1."""
    results = np.array(results, dtype="f")
    if switch:
        results[n:] *= -1.0
        results[n:] += 1.0
    wins = int(np.sum(results == 1))
    draws = int(np.sum(results == 0.5))
    losses = int(np.sum(results == 0))
    return {"wins": wins, "draws": draws, "losses": losses, "return": (1.0 * wins + 0.5 * draws) / (wins + draws + losses)}


def _device_net(player):
    """The FusedNet behind an MCTS player's evaluator, or the reason (str) why there is none."""
    from .evaluators import DeviceNetEvaluator, evaluate_centre_with_prior, unwrap
    from .fused_net import FusedNet
    from .mcts import MCTS
    if not isinstance(player, MCTS):
        return "player %r is not an MCTS player" % getattr(player, "name", player)
    fn = unwrap(player.evaluator)
    if fn is evaluate_centre_with_prior:
        return "player %r uses the centre evaluator (float64 scores): the device match serves nets only" % player.name
    ev = fn if isinstance(fn, DeviceNetEvaluator) else player.evaluator
    if not isinstance(ev, DeviceNetEvaluator):
        return "player %r's evaluator is not a DeviceNetEvaluator" % player.name
    if not isinstance(ev.net, FusedNet):
        return "player %r's net is not a FusedNet" % player.name
    return ev.net


def device_match_reason(players, unlike=False):
    """None when `players` (two or more) can meet in a DeviceMatch, else the reason as a string.  All must be MCTS over a
    DeviceNetEvaluator whose net is a FusedNet on one device, with the same filters, residual blocks and precision (not
    the 64-filter "f32x3w", which the wave kernels cannot hold), and their MCTSConfigs must agree in simulations,
    pb_c_base and pb_c_init, without root noise and with num_sampling_moves == 0.  unlike=True (a match whose players
    are configured one by one, see play_device_games) drops the rules on equal shape and precision, on "f32x3w" and on
    equal simulations / pb_c_base / pb_c_init; the others stay."""
    from . import _lib as L
    if len(players) < 2 or len(players) > L.MATCH_MAX_NETS:
        return "a device match takes 2 to %d players, not %d" % (L.MATCH_MAX_NETS, len(players))
    nets = []
    for p in players:
        net = _device_net(p)
        if isinstance(net, str):
            return net
        nets.append(net)
    first, c0 = nets[0], players[0].config
    if not unlike and first.precision == "f32x3w":
        return "the 64-filter reference-precision net (f32x3w) does not fit the match kernel"
    for p, net in zip(players, nets):
        if not unlike and (net.config.filters, net.config.n_residuals) != (first.config.filters, first.config.n_residuals):
            return "nets differ in shape: %d filters / %d blocks against %d / %d" % (
                net.config.filters, net.config.n_residuals, first.config.filters, first.config.n_residuals)
        if not unlike and net.precision != first.precision:
            return "nets differ in precision: %s against %s" % (net.precision, first.precision)
        if net.device != first.device or p.device != players[0].device:
            return "players live on different devices"
        c = p.config
        if not unlike and (c.simulations, c.pb_c_base, c.pb_c_init) != (c0.simulations, c0.pb_c_base, c0.pb_c_init):
            return "MCTSConfigs differ in simulations, pb_c_base or pb_c_init"
        if c.root_dirichlet_alpha and c.root_exploration_fraction:
            return "player %r searches with root noise" % p.name
        if c.num_sampling_moves != 0:
            return "player %r samples its first %d moves" % (p.name, c.num_sampling_moves)
    return None


DEFAULT_STEPS_PER_LAUNCH = 4096   # quanta per launch: an upper bound (a launch ends when its net's slots have all moved); tools/bench_match.py


def match_kernels(nets, unlike=False, kernel=None):
    """The match kernel of every net of a device match ("wave" / "split"), or None when nothing is to be configured
    (unlike=False, kernel=None: the engine's config and c4_match_wave_kernel for all, as ever).  kernel=None leaves the
    choice to the net: "split" for the 64-filter "f32x3w", which the wave kernel cannot hold, "wave" otherwise."""
    if kernel not in (None, "wave", "split"):
        raise ValueError("kernel must be None, 'wave' or 'split', not %r" % (kernel,))
    if kernel == "wave" and any(net.precision == "f32x3w" for net in nets):
        raise ValueError("kernel='wave' cannot hold the 64-filter reference-precision net (f32x3w); use kernel='split' or None")
    if not unlike and kernel is None:
        return None
    return [kernel or ("split" if net.precision == "f32x3w" else "wave") for net in nets]


def play_device_games(players, games, n_steps=None, eval_cache_log2_entries=0, net_order=None, timeout_s=3600.0, on_launch=None,
                      unlike=False, kernel=None):
    """Play `games` -- (Board opening, index of the player moving o, index of the player moving x) -- one per engine slot
    inside the fused match kernel and return their GameData (training_game.py:42-67: boards, moves, float64 values and
    visit policies, result) in the order of `games`, plus the engine's final statistics.  net_order: the order in which
    the nets are served each round (default 0, 1, ...); it and n_steps never change a game.  on_launch: called with the
    Engine after every c4_match_steps launch (e.g. to ask it for last_fused_kernel()).  unlike: the players may differ in net
    shape, precision and search config (device_match_reason(players, unlike=True)); the engine is created with the largest
    `simulations` among them and every player is configured on its own.  kernel: None, "wave" or "split" (match_kernels);
    with a kernel named, every player is configured as well.  Neither changes a game."""
    import torch
    from . import _lib as L
    from .engine import Engine
    from .training_game import game_data_from_record
    reason = device_match_reason(players, unlike)
    if reason is not None:
        raise ValueError(reason)
    nets = [_device_net(p) for p in players]
    kernels = match_kernels(nets, unlike, kernel)
    order = list(range(len(nets))) if net_order is None else [int(k) for k in net_order]
    if sorted(order) != list(range(len(nets))):
        raise ValueError("net_order must be a permutation of the players' indices")
    n_steps = DEFAULT_STEPS_PER_LAUNCH if n_steps is None else int(n_steps)
    G = len(games)
    if G == 0:
        return [], {}
    device = players[0].device
    dev = torch.device("cuda", device)
    eng = Engine(G, eval_mode=L.EVAL_EXTERNAL_F32, rng_mode=L.RNG_PHILOX, stop_after_move=False, games_target=G,
                 record_capacity_games=G, max_inner_iters=32, eval_cache_log2_entries=eval_cache_log2_entries,
                 time_budget_cycles=80000, device=device, n_match_nets=len(nets),
                 **dict(players[0].config.engine_kwargs(), simulations=max(p.config.simulations for p in players)))
    try:
        with torch.cuda.device(dev):
            values = torch.zeros(G, dtype=torch.float32, device=dev)
            priors = torch.zeros(G, 7, dtype=torch.float32, device=dev)
            stream = torch.cuda.current_stream(dev).cuda_stream
            eng.set_stream(stream)
            eng.reset([g[0].color[0] for g in games], [g[0].color[1] for g in games])
            if kernels is not None:   # one description per player: its own search, its own kernel
                for k, p in enumerate(players):
                    eng.match_configure(k, p.config.simulations, p.config.pb_c_base, p.config.pb_c_init, kernels[k])
            eng.match_assign([g[1] for g in games], [g[2] for g in games])
            t0 = time.time()
            while True:
                for k in order:
                    eng.match_steps(nets[k], k, values, priors, n_steps, stream)
                    if on_launch is not None:
                        on_launch(eng)
                st = eng.stats()
                if st["active_slots"] == 0:
                    break
                if time.time() - t0 > timeout_s:
                    raise TimeoutError("device match did not finish: %r" % (st,))
            if st["dropped_games"] or st["games_finished"] != G:
                raise RuntimeError("device match lost games: %r" % (st,))
            recs = eng.drain_games()
    finally:
        eng.close()
    recs = sorted(recs, key=lambda r: r.game_id)
    assert [int(r.game_id) for r in recs] == list(range(G)), [int(r.game_id) for r in recs]
    return [game_data_from_record(r) for r in recs], st


def _openings(plies):
    return sorted(make_random_ips(plies), key=lambda b: b.to_int_tuple())


class DeviceMatch:
    """Match(display, player_1, player_2, plies, switch) played inside the fused kernel: the same openings in the same
    order, play() returns the same dict.  Raises ValueError (with the reason) for players it cannot serve -- see
    device_match_reason; play_match falls back to Match for those.  After play(): `records`, the games in Match.games
    order as GameData (boards before each move, moves, float64 values, visit-count policies, result), and `stats`."""

    def __init__(self, display, player_1, player_2, plies: int = 0, switch: bool = False, n_steps=None,
                 eval_cache_log2_entries: int = 0, net_order=None, on_launch=None, unlike: bool = False, kernel=None):
        reason = device_match_reason([player_1, player_2], unlike)
        if reason is not None:
            raise ValueError(reason)
        match_kernels([_device_net(player_1), _device_net(player_2)], unlike, kernel)   # (raises for a kernel that cannot hold a net)
        self._player_1 = player_1
        self._player_2 = player_2
        ips = _openings(plies)
        # (board, index of the player moving o, index of the player moving x); switched games swap the colours
        self.games = [(copy(b), 0, 1) for b in ips]
        self.n = len(self.games)
        if switch:
            self.games += [(copy(b), 1, 0) for b in ips]
        self.switch = switch
        self.display = display
        self.n_steps = n_steps
        self.eval_cache_log2_entries = eval_cache_log2_entries
        self.net_order = net_order
        self.on_launch = on_launch
        self.unlike = unlike
        self.kernel = kernel
        self.records = None
        self.stats = None

    def play(self, agents=1):
        extra = {}   # only what was asked for: a stand-in for play_device_games need not know the later keywords
        if self.on_launch is not None:
            extra["on_launch"] = self.on_launch
        if self.unlike:
            extra["unlike"] = True
        if self.kernel is not None:
            extra["kernel"] = self.kernel
        self.records, self.stats = play_device_games([self._player_1, self._player_2], self.games, self.n_steps,
                                                     self.eval_cache_log2_entries, self.net_order, **extra)
        out = score_results([r.result.value for r in self.records], self.n, self.switch)
        if self.display:
            print("The results for {} vs {} are: {} wins, {} draws, {} losses, {:.3f} return".format(
                self._player_1.name, self._player_2.name, out["wins"], out["draws"], out["losses"], out["return"]))
        return out


def play_match(display, player_1, player_2, plies: int = 0, switch: bool = False, agents: int = 1, prefer_device: bool = True,
               unlike: bool = False, kernel=None, **device_kwargs):
    """One match by the fastest path that serves the two players: DeviceMatch when device_match_reason allows it (and
    prefer_device), the lock-step host Match otherwise (a centre or GridSearch opponent, noise, sampling, and -- without
    `unlike` -- other nets or searches).  unlike / kernel: as DeviceMatch.  Returns (result dict, "device" or "host")."""
    if prefer_device and device_match_reason([player_1, player_2], unlike) is None:
        if unlike:
            device_kwargs["unlike"] = True
        if kernel is not None:
            device_kwargs["kernel"] = kernel
        return DeviceMatch(display, player_1, player_2, plies, switch, **device_kwargs).play(agents), "device"
    return Match(display, player_1, player_2, plies, switch).play(agents), "host"


def tournament(players, plies: int = 2, switch: bool = True, display: bool = False, unlike: bool = False, kernel=None, **device_kwargs):
    """scripts/matches.py's head-to-head table: every pairing (i < j) of `players` as Match(players[i], players[j], plies,
    switch), all pairings' games in ONE engine (one evaluation cache per player).  Returns the table as a list of rows
    {"name": "<name i> vs <name j>", "wins", "draws", "losses", "return"} in pairing order -- the frame matches.py prints,
    without pandas.  unlike / kernel: as play_device_games (players of different nets and searches in one engine)."""
    reason = device_match_reason(list(players), unlike)
    if reason is not None:
        raise ValueError(reason)
    if unlike:
        device_kwargs["unlike"] = True
    if kernel is not None:
        device_kwargs["kernel"] = kernel
    ips = _openings(plies)
    games, spans = [], []
    for i in range(len(players)):
        for j in range(i + 1, len(players)):
            lo = len(games)
            games += [(copy(b), i, j) for b in ips]
            if switch:
                games += [(copy(b), j, i) for b in ips]
            spans.append((i, j, lo, len(games)))
    records, _ = play_device_games(list(players), games, **device_kwargs)
    table = []
    for i, j, lo, hi in spans:
        row = score_results([r.result.value for r in records[lo:hi]], len(ips), switch)
        if display:
            print("The results for {} vs {} are: {} wins, {} draws, {} losses, {:.3f} return".format(
                players[i].name, players[j].name, row["wins"], row["draws"], row["losses"], row["return"]))
        table.append(dict(name="{} vs {}".format(players[i].name, players[j].name), **row))
    return table
