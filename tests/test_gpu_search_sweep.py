"""The HIP search off the default configuration and on tie-heavy evaluators (tests/golden/search_sweep.json, captured from the
unmodified reference by tests/golden/gen_sweep_golden.py with the synthetic evaluators of tests/sweep_evaluators.py): all 16
pb_c_base x pb_c_init pairs of {1, 50, 19652, 10^9} x {-0.5, 0, 1.25, 4}, root noise mixed at 0.25 / 0.5 / 1.0 from tape rows with
zeros, 1e300 and 1e-300, the float32 score form with every score tied, unnormalised priors with zeros on legal columns, values
of exactly 0.0 and 1.0.  Every comparison is exact.

One engine per (config, evaluator dtype) with one slot per case; its rows are computed once (the `stepped` fixture) and the
other front ends -- evaluation cache and budgets, position queue, the Python mirror -- are compared with them."""
import numpy as np
import pytest

import sweep_evaluators as SE
from gpu_helpers import drive_external, random_undecided_positions, same_rows
from test_gpu_search import assert_root_matches, check_selfplay, make_engine, tapes_for
from test_oracle_sweep import load_sweep

pytestmark = pytest.mark.gpu

F32_KINDS = tuple(k for k in SE.KINDS if SE.dtype_of(k) == np.float32)
SUBSET_CONFIGS = (1, 3, 6, 10, 15)     # 5 configs x 3 positions = 15 cases per evaluator kind for the other front ends


@pytest.fixture(scope="module")
def sweep():
    return load_sweep()


def memo(kind):
    """The kind's evaluator behind a memo table (the answers are functions of the position)."""
    fn, table = SE.make(kind), {}

    def f(c0, c1):
        k = (int(c0), int(c1))
        if k not in table:
            table[k] = fn(*k)
        return table[k]
    return f


def grouped(cases, by_kind):
    """Cases by (config, evaluator dtype), or by (config, kind) where the evaluation cache is on: the cache knows a
    position, not who answered it."""
    groups = {}
    for c in cases:
        groups.setdefault((c["cfg"], c["kind"] if by_kind else SE.dtype_of(c["kind"]).__name__), []).append(c)
    return groups


def slot_evaluators(group):
    """One evaluator per slot: slot i searches group[i], whose kind answers its leaves."""
    fns = {k: memo(k) for k in {c["kind"] for c in group}}
    return [fns[c["kind"]] for c in group]


def run_group(group, **engine_kw):
    """The group's searches through c4_step with the host evaluators: (rows, value / visits lines, stats)."""
    from connect4_amd import _lib as L
    dtype = SE.dtype_of(group[0]["kind"])
    noisy = group[0]["config"]["root_exploration_fraction"] != 0.0
    mode = L.EVAL_EXTERNAL_F32 if dtype == np.float32 else L.EVAL_EXTERNAL_F64
    engine_kw.setdefault("eval_cache_log2_entries", -1)
    with make_engine(group[0]["config"], len(group), mode, rng_tape=noisy, stop_after_move=True, **engine_kw) as eng:
        if noisy:
            eng.set_tapes(*tapes_for(group))
        eng.reset([c["board"]["c0"] for c in group], [c["board"]["c1"] for c in group])
        drive_external(eng, slot_evaluators(group), dtype)
        rows = list(eng.read_roots())
        lines = {rule: eng.principal_variations(rule=rule) for rule in ("value", "visits")}
        st = eng.stats()
    return rows, lines, st


@pytest.fixture(scope="module")
def stepped(sweep):
    """name -> (row, {rule: line}) of every fixture search, through c4_step with a host evaluator."""
    out, bad = {}, 0
    groups = grouped(sweep["searches"], by_kind=False)
    for group in groups.values():
        rows, lines, st = run_group(group)
        bad += st["bad_evals"]
        assert st["simulations"] == sum(c["config"]["simulations"] for c in group)
        for i, c in enumerate(group):
            out[c["name"]] = (rows[i], {rule: lines[rule][i] for rule in lines})
    assert len(out) == len(sweep["searches"])
    print("%d searches in %d engines" % (len(out), len(groups)))
    return out, bad


def test_step_rows_equal_the_reference(sweep, stepped):
    rows, bad = stepped
    assert bad == 0
    for case in sweep["searches"]:
        r = rows[case["name"]][0]
        assert_root_matches(r, case)
        assert (r.color0, r.color1) == (case["board"]["c0"], case["board"]["c1"])
        assert (case["value"] is None and np.isnan(r.value)) or r.value == case["value"], case["name"]


def test_principal_variations_equal_the_reference(sweep, stepped):
    longest = 0
    for case in sweep["searches"]:
        lines = stepped[0][case["name"]][1]
        for rule, want in (("value", case["pv_value"]), ("visits", case["pv_visits"])):
            moves, visits, _ = lines[rule]
            assert moves.tolist() == want["moves"] and visits.tolist() == want["visits"], (case["name"], rule)
            longest = max(longest, len(want["moves"]))
    assert longest >= 6


def test_cache_and_budgets_are_transparent(sweep, stepped):
    """The float32 searches again with the evaluation cache on, three descent levels per launch and two evaluator-free
    simulations per step: the same rows.  (One engine per evaluator kind: the cache knows a position, not who answered.)"""
    cases = [c for c in sweep["searches"] if c["kind"] in F32_KINDS]
    hits = capped = 0
    for group in grouped(cases, by_kind=True).values():
        rows, _, st = run_group(group, eval_cache_log2_entries=12, level_budget=3, max_inner_iters=2)
        same_rows(rows, [stepped[0][c["name"]][0] for c in group], group[0]["name"])
        assert st["bad_evals"] == 0
        hits += st["eval_cache_hits"]
        capped += st["capped_slots"]
    assert hits > 0 and capped > 0


def subset(sweep, kind):
    cases = [c for c in sweep["searches"] if c["kind"] == kind and c["cfg"] in SUBSET_CONFIGS]
    assert 8 <= len(cases) <= 16
    assert any(c["noise"] is not None for c in cases) and any(c["noise"] is None for c in cases)
    return cases


@pytest.mark.parametrize("kind", SE.KINDS)
def test_position_queue_gives_the_same_rows(sweep, stepped, kind):
    from connect4_amd import _lib as L
    dtype = SE.dtype_of(kind)
    for group in grouped(subset(sweep, kind), by_kind=True).values():
        noisy = group[0]["noise"] is not None
        with make_engine(group[0]["config"], len(group) - 1, L.EVAL_EXTERNAL_F32 if dtype == np.float32 else L.EVAL_EXTERNAL_F64,
                         rng_tape=noisy, stop_after_move=True, position_queue=True, eval_cache_log2_entries=-1) as eng:
            assert eng.n_slots < len(group)
            if noisy:
                eng.set_tapes(*tapes_for(group))
            eng.queue_positions([c["board"]["c0"] for c in group], [c["board"]["c1"] for c in group])
            drive_external(eng, memo(kind), dtype)
            assert eng.queue_progress() == (len(group), len(group))
            same_rows(eng.queue_results(), [stepped[0][c["name"]][0] for c in group], "queue " + group[0]["name"])
            assert eng.stats()["bad_evals"] == 0


@pytest.mark.parametrize("kind", SE.KINDS)
def test_python_mirror_gives_the_same_rows(sweep, stepped, kind, monkeypatch):
    """connect4_amd.mcts with the evaluator as a plain callable on Boards: _Searcher takes the score form from the prior's
    dtype and draws the root noise from np.random.gamma, which here returns the fixture's tape rows."""
    from connect4_amd.board import Board
    from connect4_amd.mcts import MCTS, MCTSConfig, search
    fn = memo(kind)

    def evaluator(board):
        return fn(board.color[0], board.color[1])
    for group in grouped(subset(sweep, kind), by_kind=True).values():
        tape = [np.array(c["noise"]) for c in group if c["noise"] is not None]
        monkeypatch.setattr(np.random, "gamma", lambda *a, **k: tape.pop(0))
        boards = [Board.from_bits(c["board"]["c0"], c["board"]["c1"]) for c in group]
        outs = MCTS("mirror", MCTSConfig(**group[0]["config"]), evaluator).make_moves([b.__copy__() for b in boards])
        assert not tape
        for (move, value, tree), c, b in zip(outs, group, boards):
            same_rows([tree._result], [stepped[0][c["name"]][0]], "mirror " + c["name"])
            assert move == c["best_move"] and value == c["value"]
            assert list(tree.get_values_policy()) == c["values_policy"] and list(tree.get_visit_count_policy()) == c["visit_policy"]
        c = group[0]
        tape = [np.array(c["noise"])] if c["noise"] is not None else []
        tree = search(MCTSConfig(**c["config"]), boards[0], evaluator)
        assert tree.best_move().name == c["best_move"] and list(tree.get_values_policy()) == c["values_policy"]
        assert [ch.data.search_value.visit_count if ch.data.search_value else 0 for ch in tree.root.children] == \
            [n for n, s in zip(c["N"], c["status"]) if s != -2]


def test_games_equal_the_reference(sweep):
    from connect4_amd import _lib as L
    for g in sweep["games"]:
        check_selfplay(g, L.EVAL_EXTERNAL_F32, memo(g["kind"]))


WIDE_CONFIGS = (dict(simulations=65, pb_c_base=50, pb_c_init=0.0, root_dirichlet_alpha=0.3, root_exploration_fraction=1.0,
                     num_sampling_moves=0),
                dict(simulations=65, pb_c_base=10 ** 9, pb_c_init=4.0, root_dirichlet_alpha=0.3, root_exploration_fraction=0.5,
                     num_sampling_moves=0))


@pytest.fixture(scope="module")
def wide_positions(oracle):
    boards = random_undecided_positions(oracle, 256, seed=4711, max_plies=38)
    noise = np.zeros((256, 42, 7))
    noise[:, 0] = np.random.RandomState(12).gamma(0.3, 1.0, size=(256, 7))
    return boards, noise


@pytest.mark.parametrize("kind", SE.KINDS)
def test_engine_equals_oracle_on_256_positions(oracle, wide_positions, kind):
    """No fixture: 256 seeded positions of up to 38 plies x two off-default configurations, engine == oracle exactly."""
    from connect4_amd import _lib as L
    boards, noise = wide_positions
    dtype = SE.dtype_of(kind)
    fn = memo(kind)

    def cb(c0, c1):
        v, p = fn(c0, c1)
        return v, p, p.dtype == np.float32
    ev = oracle.CallbackEvaluator(cb)
    for c in WIDE_CONFIGS:
        with make_engine(c, len(boards), L.EVAL_EXTERNAL_F32 if dtype == np.float32 else L.EVAL_EXTERNAL_F64, rng_tape=True,
                         stop_after_move=True, eval_cache_log2_entries=-1) as eng:
            eng.set_tapes(noise, np.full((256, 42), -1.0))
            eng.reset([b.key()[0] for b in boards], [b.key()[1] for b in boards])
            drive_external(eng, fn, dtype)
            roots = eng.read_roots()
            st = eng.stats()
        assert st["bad_evals"] == 0 and st["simulations"] == 65 * len(boards)
        cfg = oracle.make_config(**c)
        for i, (r, b) in enumerate(zip(roots, boards)):
            info, mv, av = oracle.search_and_pick(cfg, b, ev, noise[i, 0], -1.0)
            assert r.root_visits == info.root_visits == 66
            assert r.root_value_sum == info.root_value_sum
            assert list(r.child_visits) == list(info.child_visits), i
            assert list(r.child_value_sum) == list(info.child_value_sum), i
            assert list(r.child_status) == list(info.child_status)
            assert list(r.root_prior) == list(info.root_prior)
            assert list(r.values_policy) == list(info.values_policy)
            assert r.move == mv
            assert (np.isnan(r.value) and np.isnan(av)) or r.value == av
            assert r.expansions == info.n_expansions
