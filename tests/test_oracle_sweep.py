"""The CPU oracle off the default configuration and on tie-heavy evaluators: tests/golden/search_sweep.json holds searches and
self-play games of the unmodified reference (tests/golden/gen_sweep_golden.py) with the synthetic evaluators of
tests/sweep_evaluators.py -- every pb_c_base / pb_c_init pair of {1, 50, 19652, 10^9} x {-0.5, 0, 1.25, 4}, root noise mixed
at 0.25 / 0.5 / 1.0 from designed tape rows, priors left unnormalised with zeros on legal columns, values of exactly 0 and 1.
Bar: every field exact; no case is skipped."""
import numpy as np
import pytest

import sweep_evaluators as SE
from conftest import load_json
from test_oracle_golden import check_game

SIMS = {1, 2, 3, 7, 8, 9, 64, 65, 200}
BASES = {1, 50, 19652, 10 ** 9}
INITS = {-0.5, 0.0, 1.25, 4.0}
FRACS = {0.0, 0.25, 0.5, 1.0}


def load_sweep():
    """The fixture with every search's config dict filled in from its index."""
    data = load_json("search_sweep.json")
    for c in data["searches"]:
        c["config"] = data["configs"][c["cfg"]]
    return data


@pytest.fixture(scope="module")
def sweep():
    return load_sweep()


def callback(oracle, kind):
    fn = SE.make(kind)
    f32 = SE.dtype_of(kind) == np.float32

    def cb(c0, c1):
        v, p = fn(c0, c1)
        return v, p, p.dtype == np.float32
    assert f32 == (fn(0, 0)[1].dtype == np.float32)
    return oracle.CallbackEvaluator(cb)


def test_fixture_covers_the_value_sets(sweep):
    cases = sweep["searches"]
    assert len(cases) >= 200
    for kind in SE.KINDS:
        cfgs = [c["config"] for c in cases if c["kind"] == kind]
        assert {c["simulations"] for c in cfgs} == SIMS
        assert {c["pb_c_base"] for c in cfgs} == BASES
        assert {c["pb_c_init"] for c in cfgs} == INITS
        assert {c["root_exploration_fraction"] for c in cfgs} == FRACS
    assert {(c["pb_c_base"], c["pb_c_init"]) for c in sweep["configs"]} == {(b, a) for b in BASES for a in INITS}
    # the tape rows: exact zeros on legal columns, 1e300, 1e-300, one-hot rows; never all zero on the legal columns
    zeros = huge = tiny = onehot = 0
    for c in cases:
        if c["noise"] is None:
            assert c["config"]["root_exploration_fraction"] == 0.0
            continue
        legal = [k for k in range(7) if c["status"][k] != -2]
        row = [c["noise"][k] for k in legal]
        assert sum(row) > 0.0
        zeros += 0.0 in row
        huge += 1e300 in row
        tiny += 1e-300 in row
        onehot += sum(x != 0.0 for x in c["noise"]) == 1
    assert min(zeros, huge, tiny, onehot) >= 8
    # the positions: one legal column, a winning move, a forced loss, one move from a full board -- several times each
    names = [c["name"] for c in cases]
    for what in ("one_legal", "winning_move", "forced_loss", "last_move"):
        assert sum(what in n for n in names) >= 8, what
    assert max(c["board"]["age"] for c in cases) == 41 and min(c["board"]["age"] for c in cases) == 0
    # ties decide something in a good share of the searches of the tie-heavy evaluators
    for kind in ("const32", "quant32", "quant64"):
        cs = [c for c in cases if c["kind"] == kind]
        assert sum(c["tie_steps"] > 0 for c in cs) >= 0.3 * len(cs), kind


def test_evaluator_outputs_are_the_recorded_bits(sweep):
    rows = sweep["evaluator_outputs"]
    assert len(rows) >= 24 and {r["kind"] for r in rows} == set(SE.KINDS)
    for r in rows:
        assert SE.output_bits(r["kind"], r["c0"], r["c1"]) == (r["value_bits"], r["prior_bits"]), r


def test_evaluators_keep_their_promises(sweep):
    """Values in [0, 1] with both ends met, priors finite, non-negative and at most 4096, a positive entry on a legal column;
    the sparse kinds put zeros on legal columns and mass on illegal ones."""
    boards = {(c["board"]["c0"], c["board"]["c1"]) for c in sweep["searches"]}
    for g in sweep["games"]:
        boards.update((a, b) for a, b in g["boards"])
    for kind in SE.KINDS:
        values, zero_on_legal, mass_on_illegal = set(), 0, 0
        for c0, c1 in sorted(boards):
            v, p = SE.evaluate(kind, c0, c1)
            legal = SE.legal_columns(c0, c1)
            assert isinstance(v, float) and 0.0 <= v <= 1.0 and p.dtype == SE.dtype_of(kind) and p.shape == (7,)
            assert np.isfinite(p).all() and (p >= 0).all() and (p <= 4096).all() and (p == np.floor(p)).all()
            assert any(p[k] > 0 for k in legal)
            if p.dtype == np.float32:
                assert float(np.float32(v)) == v
            values.add(v)
            zero_on_legal += any(p[k] == 0 for k in legal)
            mass_on_illegal += any(p[k] > 0 for k in range(7) if k not in legal)
        if kind.startswith("const"):
            assert values == {0.5}
        else:
            assert 0.0 in values and 1.0 in values
        if kind.startswith("sparse"):
            assert zero_on_legal >= 10 and mass_on_illegal >= 10


def check_sweep_search(oracle, case, evaluator):
    cfg = oracle.make_config(**case["config"])
    b = oracle.Board.from_bits(case["board"]["c0"], case["board"]["c1"])
    assert b.age == case["board"]["age"] and b.result == -1
    info, mv, av = oracle.search_and_pick(cfg, b, evaluator, case["noise"], -1.0)
    name = case["name"]
    assert info.root_visits == case["root_N"] == case["config"]["simulations"] + 1, name
    assert info.root_value_sum == case["root_W"], name
    assert list(info.child_visits) == case["N"], name
    assert list(info.child_value_sum) == case["W"], name
    assert list(info.child_status) == case["status"], name
    assert list(info.child_value) == case["child_value"], name
    assert list(info.values_policy) == case["values_policy"], name
    assert list(info.visit_policy) == case["visit_policy"], name
    assert list(info.root_prior) == case["root_prior"], name
    assert info.best_move == mv == case["best_move"], name
    assert (case["value"] is None and np.isnan(av)) or av == case["value"], name
    assert info.n_expansions == case["n_expansions"] and info.n_nodes == case["n_nodes"], name
    # the plain search call gives the same tree
    again = oracle.search(cfg, b, evaluator, case["noise"])
    assert list(again.child_visits) == case["N"] and list(again.child_value_sum) == case["W"], name
    # the recorded lines start where the root read-out says
    assert case["pv_value"]["moves"][0] == case["best_move"] and case["pv_value"]["visits"][0] == case["N"][case["best_move"]]
    top = max(range(7), key=lambda k: (case["N"][k] if case["status"][k] != -2 else -1, k))
    assert case["pv_visits"]["moves"][0] == top and case["pv_visits"]["visits"][0] == case["N"][top]


@pytest.mark.parametrize("kind", SE.KINDS)
def test_searches(oracle, sweep, kind):
    cases = [c for c in sweep["searches"] if c["kind"] == kind]
    assert len(cases) >= 40
    ev = callback(oracle, kind)
    for case in cases:
        check_sweep_search(oracle, case, ev)


def test_games(oracle, sweep):
    games = sweep["games"]
    assert {g["kind"] for g in games} == {"const32", "quant32", "sparse32"}
    assert {g["config"]["num_sampling_moves"] for g in games} == {0, 42}
    assert {g["config"]["root_exploration_fraction"] for g in games} == {0.25, 1.0}
    assert {g["config"]["simulations"] for g in games} == {9, 60}
    for g in games:
        assert len(g["noise_tape"]) == len(g["moves"])
        assert len(g["uniforms"]) == (len(g["moves"]) if g["config"]["num_sampling_moves"] else 0)
        check_game(oracle, g, callback(oracle, g["kind"]))
