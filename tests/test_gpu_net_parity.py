"""The shipped net against the reference at the production simulation count (tests/golden/net_parity.json, written by
tests/golden/gen_net_parity_golden.py from the unmodified reference with example_net.pth): 48 random positions at 800
simulations, four of them at 3200, and every ply of three noisy training games.

A search whose visit counts the reference keeps when every evaluator answer is moved by up to tol_f32x3(3) -- `decided`
in the fixture, a property of the reference alone -- must come out of the GPU with the reference's visit counts, child
states, expansions and move, whichever forward answers the leaves: the f32x3 FusedNet as shipped or the fp32
InferenceNet.  A near-tie may fall the other way for honest rounding, so nothing about it is compared with the
reference; instead the CPU oracle repeats it from the GPU net's OWN answers (the engine's evaluation cache, the net
for what the cache lost) and must arrive at the GPU's root bit for bit: what differs is then an answer's last bits, not
the tree walk.  How many searches of each kind equal the reference's is printed (profiles/README.md keeps the figures).

The forwards' answers are also compared directly with the reference's on the positions these searches reached
(net_parity_tables.npz, about 12 k distinct ones), at the tolerances test_gpu_fused_net.py states for net_golden.npz's
96 random positions: 5e-5 for f32x3 and for the fp32 plan, 2e-2 for fp16 storage."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_json, load_npz, table_from_npz

pytestmark = pytest.mark.gpu

TOL_REFERENCE = 5e-5        # test_gpu_fused_net.py::test_precise_net_vs_reference_golden
TOL_F16 = 2e-2              # test_gpu_fused_net.py::test_fused_net_vs_reference_golden
ROOT_W_PER_VISIT = 1e-4     # test_gpu_api.py::test_end_to_end_net_driven_search_matches_reference
CACHE_BITS = 22             # evaluation cache of the test engines (stop-after-move engines have none by default)


@pytest.fixture(scope="module")
def fixture():
    return load_json("net_parity.json")


@pytest.fixture(scope="module")
def state_dict():
    z = load_npz("net_golden.npz")
    return {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w__")}


def eval_positions(net, c0, c1, batch=None):
    """(values, priors) float32 of either kind of net on bitboards.  The fused forwards answer a position with the same
    bits whatever stands next to it; the fp32 plan runs library kernels chosen by batch size, so with `batch` it is asked
    in batches of exactly that many rows (the last one filled up with repeats), as the engine it stands in for asked."""
    from connect4_amd.engine import board_planes
    if getattr(net, "from_bitboards", False):
        return net.evaluate_bits(c0, c1, wave=True)
    n = len(c0)
    if batch:
        idx = np.resize(np.arange(n), -(-n // batch) * batch)
        c0, c1 = c0[idx], c1[idx]
    planes = torch.from_numpy(board_planes(c0, c1)).cuda()
    outs = [net(x) for x in planes.split(batch or len(planes))]
    v, p = torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])
    return v[:n].cpu().numpy(), p[:n].cpu().numpy()


# ------------------------------------------------------------------------------------------ (a) answers
def test_answers_on_search_positions(fixture, state_dict):
    from connect4_amd.fused_net import FusedNet, make_selfplay_net
    from connect4_amd.net import InferenceNet
    npz = load_npz("net_parity_tables.npz")
    pos = {}
    for name in fixture["table_cases"]:
        for a, b, v, p in zip(*table_from_npz(npz, name)):
            pos[(int(a), int(b))] = (v, p)
    keys = sorted(pos)
    c0 = np.array([k[0] for k in keys], dtype=np.uint64)
    c1 = np.array([k[1] for k in keys], dtype=np.uint64)
    rv = np.array([pos[k][0] for k in keys], dtype=np.float32)
    rp = np.stack([pos[k][1] for k in keys]).astype(np.float32)
    assert len(keys) >= 10000
    shipped = make_selfplay_net(state_dict)
    assert isinstance(shipped, FusedNet) and shipped.precision == "f32x3"
    v, p = shipped.evaluate_bits(c0, c1)
    wv, wp = shipped.evaluate_bits(c0, c1, wave=True)
    fv, fp = eval_positions(InferenceNet(state_dict, device="cuda", dtype=torch.float32), c0, c1)
    hv, hp = FusedNet(state_dict, precision="f16").evaluate_bits(c0, c1)
    for name, (gv, gp), tol in (("f32x3 c4_net_forward", (v, p), TOL_REFERENCE), ("f32x3 c4_net_forward_wave", (wv, wp), TOL_REFERENCE),
                                ("fp32 InferenceNet", (fv, fp), TOL_REFERENCE), ("f16 c4_net_forward", (hv, hp), TOL_F16)):
        dv, dp = np.abs(gv - rv).max(), np.abs(gp - rp).max()
        print("%-26s vs the reference on %d search positions: max |dv| %.3g  max |dp| %.3g  (bound %.0e)" % (name, len(keys), dv, dp, tol))
        assert np.isfinite(gv).all() and np.isfinite(gp).all()
        assert dv <= tol and dp <= tol, name
    assert np.array_equal(v, wv) and np.array_equal(p, wp)       # both entry points: one implementation


# ------------------------------------------------------------------------------------------ (b) searches
def cfg_key(c):
    return (c["simulations"], c["pb_c_base"], c["pb_c_init"], c["root_dirichlet_alpha"], c["root_exploration_fraction"],
            c["num_sampling_moves"])


def tapes_for(cases):
    """Root noise in row 0 of the tape (as test_gpu_search.py::tapes_for), the recorded uniform of a sampled ply next to it."""
    nz = np.zeros((len(cases), 42, 7))
    u = np.full((len(cases), 42), -1.0)
    for i, c in enumerate(cases):
        if c["noise"] is not None:
            nz[i, 0] = c["noise"]
        if c["uniform"] is not None:
            u[i, 0] = c["uniform"]
    return nz, u


def make_engine(group):
    from connect4_amd import _lib as L
    from connect4_amd.engine import Engine
    c = group[0]["config"]
    eng = Engine(len(group), c["simulations"], c["pb_c_base"], c["pb_c_init"], c["root_dirichlet_alpha"],
                 c["root_exploration_fraction"], c["num_sampling_moves"], eval_mode=L.EVAL_EXTERNAL_F32, rng_mode=L.RNG_TAPE,
                 stop_after_move=True, eval_cache_log2_entries=CACHE_BITS)
    eng.set_tapes(*tapes_for(group))
    eng.reset([c["board"]["c0"] for c in group], [c["board"]["c1"] for c in group])
    return eng


def drive_steps(eng, net):
    """c4_step and the net's forward in turn on one stream, as MCTS.make_moves drives a device net."""
    G = eng.n_slots
    values = torch.zeros(G, dtype=torch.float32, device="cuda")
    priors = torch.zeros(G, 7, dtype=torch.float32, device="cuda")
    planes = torch.zeros(G, 3, 6, 7, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    eng.set_stream(stream)
    bits = bool(getattr(net, "from_bitboards", False))
    c0p, c1p, _ = eng.leaf_buffers()
    eng.step(None, None, None if bits else planes)
    for step in range(1, 4 * eng.cfg.simulations + 129):
        if bits:
            net.forward_bitboards(c0p, c1p, G, values, priors, stream)
        else:
            v, p = net(planes)
            values.copy_(v)
            priors.copy_(p)
        eng.step(values, priors, None if bits else planes)
        if step % 64 == 0 and eng.stats()["active_slots"] == 0:
            return
    raise RuntimeError("searches did not finish: %r" % (eng.stats(),))


def drive_fused(eng, net):
    """The same searches inside the persistent self-play kernel (c4_selfplay_steps, tree waves + network waves)."""
    from connect4_amd import _lib as L
    G = eng.n_slots
    values = torch.zeros(G, dtype=torch.float32, device="cuda")
    priors = torch.full((G, 7), 1.0 / 7.0, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    eng.set_stream(stream)
    for _ in range(4 * eng.cfg.simulations // 64 + 4):
        L.check(eng._lib.c4_selfplay_steps(eng._h, net._h, C.c_void_p(values.data_ptr()), C.c_void_p(priors.data_ptr()), 64,
                                           C.c_void_p(stream)), eng._h)
        if eng.stats()["active_slots"] == 0:
            return
    raise RuntimeError("searches did not finish: %r" % (eng.stats(),))


def root_dict(r):
    return dict(state=int(r.state), move=int(r.move), value=float(r.value), root_visits=int(r.root_visits),
                root_value_sum=float(r.root_value_sum), child_visits=list(r.child_visits), child_value_sum=list(r.child_value_sum),
                child_status=list(r.child_status), root_prior=list(r.root_prior), values_policy=list(r.values_policy),
                color0=int(r.color0), color1=int(r.color1), expansions=int(r.expansions), simulations=int(r.simulations))


def same(a, b):
    """Bit for bit, NaN equal to NaN (the value of a move into an unvisited child); lists element by element."""
    if isinstance(a, list):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return a == b or (isinstance(a, float) and isinstance(b, float) and np.isnan(a) and np.isnan(b))


def check_decided(case, r):
    """The reference decides this search by a margin: the GPU's must be the same search."""
    name = case["name"]
    assert r.child_visits[:] == case["N"], (name, r.child_visits[:], case["N"])
    assert r.child_status[:] == case["status"], name
    assert r.expansions == case["n_expansions"], (name, r.expansions, case["n_expansions"])
    assert r.simulations == case["config"]["simulations"] and r.root_visits == case["root_N"], name
    assert r.move == case["move"], (name, r.move, case["move"])
    assert abs(r.root_value_sum - case["root_W"]) <= ROOT_W_PER_VISIT * case["root_N"], name


def replay_on_oracle(oracle, eng, net, slot, case, r):
    """The oracle, answered with what the GPU net answered (evaluation cache first, as oracle/replay.py), must walk to the
    GPU's root bit for bit."""
    t = eng.export_trees([slot])[0]
    asked = np.asarray(t.prior_kind) != 0                      # the nodes an evaluator answered
    keys = sorted({(int(a), int(b)) for a, b in zip(np.asarray(t.color0)[asked], np.asarray(t.color1)[asked])})
    c0 = np.array([k[0] for k in keys], dtype=np.uint64)
    c1 = np.array([k[1] for k in keys], dtype=np.uint64)
    v, p, found = eng.cache_lookup(c0, c1)
    if not found.all():
        miss = np.nonzero(~found)[0]
        v[miss], p[miss] = eval_positions(net, c0[miss], c1[miss], batch=eng.n_slots)
    ev = oracle.TableEvaluator(c0, c1, v, p, prior_f32=True)
    b = oracle.Board.from_bits(case["board"]["c0"], case["board"]["c1"])
    info, mv, av = oracle.search_and_pick(oracle.make_config(**case["config"]), b, ev, case["noise"],
                                          -1.0 if case["uniform"] is None else case["uniform"])
    name = case["name"]
    assert ev.table.misses == 0, name
    assert list(info.child_visits) == r.child_visits[:], (name, list(info.child_visits), r.child_visits[:])
    assert list(info.child_value_sum) == r.child_value_sum[:], name
    assert list(info.child_status) == r.child_status[:], name
    assert list(info.values_policy) == r.values_policy[:], name
    assert list(info.root_prior) == r.root_prior[:], name
    assert (info.root_visits, info.root_value_sum, info.n_expansions) == (r.root_visits, r.root_value_sum, r.expansions), name
    assert mv == r.move and same(float(av), float(r.value)), name
    return int((~found).sum())


def total_variation(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(0.5 * np.abs(a / a.sum() - b / b.sum()).sum())


@pytest.mark.parametrize("kind", ["f32x3", "fp32"])
def test_searches_against_the_reference(oracle, fixture, state_dict, monkeypatch, kind):
    from connect4_amd.board import Board
    from connect4_amd.fused_net import FusedNet, make_selfplay_net
    from connect4_amd.net import InferenceNet
    from connect4_amd.tree import Tree
    if kind == "f32x3":
        net = make_selfplay_net(state_dict)
        assert isinstance(net, FusedNet) and net.precision == "f32x3"
    else:
        net = InferenceNet(state_dict, device="cuda", dtype=torch.float32)
    groups = {}
    for c in fixture["cases"]:
        groups.setdefault(cfg_key(c["config"]), []).append(c)
    assert len(groups) == 3
    identical = {True: 0, False: 0}
    total = {True: 0, False: 0}
    lost = 0
    for group in groups.values():
        with make_engine(group) as eng:
            drive_steps(eng, net)
            roots = eng.read_roots()
            assert eng.stats()["bad_evals"] == 0
            for slot, (case, r) in enumerate(zip(group, roots)):
                assert r.state == 2 and (r.color0, r.color1) == (case["board"]["c0"], case["board"]["c1"])
                equal = r.child_visits[:] == case["N"]
                total[case["decided"]] += 1
                identical[case["decided"]] += equal
                if equal:       # the package's visit-count policy is then the recorded row
                    tree = Tree(r, Board.from_bits(case["board"]["c0"], case["board"]["c1"]))
                    assert list(tree.get_visit_count_policy()) == case["visit_policy"], case["name"]
                if case["decided"]:
                    check_decided(case, r)
                else:
                    lost += replay_on_oracle(oracle, eng, net, slot, case, r)
                    print("%s near-tie %-12s TV against the reference %.4f (the reference against itself under +-tol_f32x3: %.4f)%s" %
                          (kind, case["name"], total_variation(r.child_visits[:], case["N"]), case["self_tv"],
                           "" if equal else "  differs"))
            stepped = [root_dict(r) for r in roots]
        if kind == "f32x3":     # ... and inside the persistent self-play kernel, split mode: the same roots bit for bit
            monkeypatch.setenv("C4_FUSED_MODE", "split")
            with make_engine(group) as eng:
                drive_fused(eng, net)
                assert eng.stats()["bad_evals"] == 0
                for case, a, r in zip(group, stepped, eng.read_roots()):
                    b = root_dict(r)
                    assert all(same(a[k], b[k]) for k in a), (case["name"], a, b)
    n = total[True] + total[False]
    print("%s: visit counts identical to the reference's on %d of %d searches (%.1f %%): %d of %d decided, %d of %d near-ties; "
          "%d replayed answers came from the net instead of the cache" %
          (kind, identical[True] + identical[False], n, 100.0 * (identical[True] + identical[False]) / n, identical[True],
           total[True], identical[False], total[False], lost))
    assert n == len(fixture["cases"]) and identical[True] == total[True]
