"""The device-side tree export (c4_tree_sizes / c4_export_trees / c4_principal_variations) against WHOLE trees of the unmodified
reference (tests/golden/search_trees.npz): node count, structure, visit counts, statuses and boards equal, float64 value sums
and priors equal with ==, for every fixture case.  Then the public surface over it, batching, the two device-side filters, the
principal variations, a 4,096-slot run, a slot that is still searching, an engine driven by the fused self-play kernel, and
the error paths."""
import numpy as np
import pytest

from gpu_helpers import drive_external, table_lookup_fn
from conftest import load_npz, table_from_npz
from tree_fixture import load_tree_cases

pytestmark = pytest.mark.gpu

POPCOUNT7 = np.array([bin(i).count("1") for i in range(128)])
STRUCTURE = ("parent", "first_child", "n_children", "move", "depth", "visits", "status", "color0", "color1", "prior_kind")


def cfg_key(c):
    return tuple(c[k] for k in ("simulations", "pb_c_base", "pb_c_init", "root_dirichlet_alpha", "root_exploration_fraction",
                                "num_sampling_moves"))


def make_engine(c, n_slots, eval_mode, rng_tape=False, **kw):
    from connect4_amd import _lib as L
    from connect4_amd.engine import Engine
    return Engine(n_slots, c["simulations"], c["pb_c_base"], c["pb_c_init"], c["root_dirichlet_alpha"],
                  c["root_exploration_fraction"], c["num_sampling_moves"], eval_mode=eval_mode,
                  rng_mode=L.RNG_TAPE if rng_tape else L.RNG_PHILOX, **kw)


def tapes_for(cases):
    nz = np.zeros((len(cases), 42, 7))
    for i, c in enumerate(cases):
        if c.noise is not None:
            nz[i, 0] = c.noise
    return nz, np.full((len(cases), 42), -1.0)


def path_of(t, row):
    moves = []
    while row > 0:
        moves.append(int(t.move[row]))
        row = int(t.parent[row])
    return moves[::-1]


def assert_tables_equal(got, want, what):
    assert len(got) == len(want), "%s: %d nodes, expected %d" % (what, len(got), len(want))
    for f in STRUCTURE:
        assert (getattr(got, f) == getattr(want, f)).all(), (what, f)
    bad = np.nonzero(got.value_sum != want.value_sum)[0]
    assert len(bad) == 0, "%s: value_sum differs at %d nodes, first at path %s: %r != %r" % (
        what, len(bad), path_of(want, bad[0]), got.value_sum[bad[0]], want.value_sum[bad[0]])
    bad = np.nonzero((got.prior != want.prior).any(axis=1))[0]
    assert len(bad) == 0, "%s: prior differs at %d nodes, first at path %s: %r != %r" % (
        what, len(bad), path_of(want, bad[0]), got.prior[bad[0]], want.prior[bad[0]])


def check_invariants(t, what, complete=True):
    """What holds in every reference-shaped table, whatever searched it.  complete: exported with min_visits <= 1 and no depth limit."""
    from connect4_amd.tree import TreeTable
    n = len(t)
    assert n > 0 and t.parent[0] == -1 and t.move[0] == -1 and t.depth[0] == 0, what
    # structure, depth and boards follow from parent / move alone: the device's equal the host's replay
    ref = TreeTable.from_arrays(t.color0[0], t.color1[0], t.parent, t.move, t.visits, t.value_sum, t.status)
    for f in ("first_child", "n_children", "depth", "color0", "color1"):
        assert (getattr(t, f) == getattr(ref, f)).all(), (what, f)
    same = t.parent[2:] == t.parent[1:-1]
    assert (t.move[2:][same] > t.move[1:-1][same]).all(), what
    terminal = t.status >= 0
    kids = t.n_children > 0
    assert not (kids & terminal).any(), what
    if complete:
        assert (kids == (~terminal & (t.visits >= 2))).all(), what          # children iff visits >= 2
        below = np.bincount(t.parent[1:], weights=t.visits[1:], minlength=n).astype(np.int64)
        assert (t.visits[kids] == 1 + below[kids]).all(), what              # the sum rule
    assert ((t.prior_kind != 0) == (~terminal & (t.visits >= 1))).all(), what
    has = t.prior_kind != 0
    assert (t.prior[~has] == 0.0).all(), what
    occ = t.color0[has] | t.color1[has]
    for c in range(7):                                  # nothing on a full column
        full = POPCOUNT7[((occ >> np.uint64(7 * c)) & np.uint64(0x7f)).astype(np.int64)] >= 6
        assert (t.prior[has][full, c] == 0.0).all() and (t.prior[has][~full, c] > 0.0).all(), what
    assert (np.abs(t.prior[has].sum(axis=1) - 1.0) <= 1e-6).all(), what
    assert ((t.visits == 0) <= (t.value_sum == 0.0)).all(), what


# ---------------------------------------------------------------------------------------------- parity with the reference
@pytest.fixture(scope="module")
def cases():
    return load_tree_cases()


def run_centre_group(group, **kw):
    from connect4_amd import _lib as L
    noisy = group[0].config["root_dirichlet_alpha"] != 0
    eng = make_engine(group[0].config, len(group), L.EVAL_CENTRE, rng_tape=noisy, stop_after_move=True, **kw)
    if noisy:
        eng.set_tapes(*tapes_for(group))
    eng.reset([c.c0 for c in group], [c.c1 for c in group])
    eng.run_centre()
    return eng


def test_whole_tree_parity_centre(cases):
    """Every centre-evaluator fixture tree (the 49 pinned searches and the late positions), batched per config as
    test_search_centre_golden batches them: the device export IS the reference's tree."""
    groups = {}
    for c in cases:
        if c.kind != "net":
            groups.setdefault(cfg_key(c.config), []).append(c)
    assert sum(len(g) for g in groups.values()) >= 49 + 4
    for group in groups.values():
        with run_centre_group(group) as eng:
            tables = eng.export_trees()
            sizes = eng.tree_sizes()
        for t, size, c in zip(tables, sizes, group):
            assert size == len(c), c.name
            assert_tables_equal(t, c.table(), c.name)
            check_invariants(t, c.name)


def test_whole_tree_parity_net(cases):
    """The 15 net-driven searches, answered from the recorded float32 table as test_search_net_table_golden does: float32 priors
    (the noisy root float64) and the float32 score path, node for node."""
    from connect4_amd import _lib as L
    npz = load_npz("search_net_tables.npz")
    net = [c for c in cases if c.kind == "net"]
    assert len(net) == 15
    for c in net:
        fn = table_lookup_fn(*table_from_npz(npz, c.name))
        noisy = c.noise is not None
        with make_engine(c.config, 1, L.EVAL_EXTERNAL_F32, rng_tape=noisy, stop_after_move=True) as eng:
            if noisy:
                eng.set_tapes(*tapes_for([c]))
            eng.reset([c.c0], [c.c1])
            drive_external(eng, fn, np.float32)
            (t,) = eng.export_trees()
        assert_tables_equal(t, c.table(), c.name)
        check_invariants(t, c.name)


def test_public_api_full_tree(cases, monkeypatch):
    """search(..., full_tree=True) and MCTS(..., full_tree=True).make_moves(boards) return the whole trees; the default
    stays root-only and calls no export entry."""
    from connect4_amd.board import Board
    from connect4_amd.config import MCTSConfig
    from connect4_amd.engine import Engine
    from connect4_amd.evaluators import Evaluator, evaluate_centre_with_prior
    from connect4_amd.mcts import MCTS, search
    batch = [c for c in cases if c.name.startswith("random") and c.name.endswith("_s200")][:12]
    assert len(batch) == 12
    cfg = MCTSConfig(**batch[0].config)
    c = batch[3]
    tree = search(cfg, Board.from_bits(c.c0, c.c1), Evaluator(evaluate_centre_with_prior), full_tree=True)
    assert_tables_equal(tree.table, c.table(), c.name)
    assert tree.n_nodes == len(c) and tree.root.children[0].parent is tree.root
    want = c.table()
    deep = int(np.argmax(want.depth))
    node = tree.root
    for m in path_of(want, deep):          # walk to the deepest node through the reference's surface
        node = [k for k in node.children if k.name == m][0]
    assert node.data.search_value is None or node.data.search_value.visit_count == c.visits[deep]

    boards = [Board.from_bits(x.c0, x.c1) for x in batch]
    player = MCTS("whole", cfg, Evaluator(evaluate_centre_with_prior), full_tree=True)
    out = player.make_moves(boards)
    for (move, value, tree), x, b in zip(out, batch, boards):
        assert_tables_equal(tree.table, x.table(), x.name)
        assert move == tree.best_move().name and b.age == bin(x.c0 | x.c1).count("1") + 1
        assert value == tree.child(move).data.absolute_value
        assert tree.principal_variation("value")[0][0] == move

    player._searcher.close()

    # default: today's tree, no export call
    def forbidden(*a, **k):
        raise AssertionError("an export entry was called for a root-only tree")
    monkeypatch.setattr(Engine, "export_trees", forbidden)
    monkeypatch.setattr(Engine, "tree_sizes", forbidden)
    boards = [Board.from_bits(x.c0, x.c1) for x in batch]
    out2 = MCTS("roots", cfg, Evaluator(evaluate_centre_with_prior)).make_moves(boards)
    for (move, value, tree), (m1, v1, whole) in zip(out2, out):
        assert (move, value) == (m1, v1) and tree.n_nodes <= 8
        assert all(k.children == () for k in tree.root.children)
        assert list(tree.get_values_policy()) == list(whole.get_values_policy())
    small = search(cfg, Board.from_bits(c.c0, c.c1), Evaluator(evaluate_centre_with_prior))
    assert small.n_nodes <= 8


# ---------------------------------------------------------------------------------------------- batching, filters, lines
@pytest.fixture(scope="module")
def searched(cases):
    """One engine with 24 finished searches (the random*_s200 fixture cases) for the tests that only read."""
    group = [c for c in cases if c.name.startswith("random") and c.name.endswith("_s200")]
    assert len(group) == 24
    eng = run_centre_group(group)
    yield eng, group
    eng.close()


def test_batching_and_sizes(searched):
    eng, group = searched
    whole = eng.export_trees()
    assert [t.slot for t in whole] == list(range(24))
    assert eng.tree_sizes().tolist() == [len(t) for t in whole] == [len(c) for c in group]
    slots = np.random.RandomState(1).permutation(24)[:11]
    some = eng.export_trees(slots)
    assert [t.slot for t in some] == slots.tolist()
    assert eng.tree_sizes(slots).tolist() == [len(t) for t in some]
    for t, g in zip(some, slots):
        (one,) = eng.export_trees([int(g)])
        assert one.nodes.tobytes() == t.nodes.tobytes() == whole[g].nodes.tobytes()
    assert eng.export_trees([]) == []


def test_export_into_a_device_buffer(searched):
    """c4_export_trees_dev writes the same tables into caller-owned device memory."""
    import ctypes as C
    import torch
    from connect4_amd import _lib as L
    eng, group = searched
    slots = np.array([7, 0, 19], dtype=np.int32)
    want = eng.export_trees(slots, min_visits=1)
    total = sum(len(t) for t in want)
    item = L.tree_node_dtype().itemsize
    buf = torch.zeros((total + 1) * item, dtype=torch.uint8, device="cuda")      # one spare row: it must stay untouched
    off = np.zeros(4, dtype=np.int64)
    L.check(eng._lib.c4_export_trees_dev(eng._h, slots.ctypes.data_as(C.POINTER(C.c_int32)), 3, 1, -1, C.c_void_p(buf.data_ptr()),
                                         total, off.ctypes.data_as(C.POINTER(C.c_int64))), eng._h)
    assert off.tolist() == np.concatenate(([0], np.cumsum([len(t) for t in want]))).tolist()
    host = buf.cpu().numpy()
    assert host[:total * item].tobytes() == b"".join(t.nodes.tobytes() for t in want)
    assert not host[total * item:].any()


@pytest.mark.parametrize("min_visits,max_depth", [(1, None), (2, None), (10, None), (0, 0), (0, 1), (0, 3), (2, 3), (300, None)])
def test_device_filters_equal_the_host_filter(searched, min_visits, max_depth):
    eng, group = searched
    whole = eng.export_trees()
    got = eng.export_trees(min_visits=min_visits, max_depth=max_depth)
    sizes = eng.tree_sizes(min_visits=min_visits, max_depth=max_depth)
    for t, w, n in zip(got, whole, sizes):
        want = w.filtered(min_visits, max_depth)
        assert n == len(t) == len(want)
        assert t.nodes.tobytes() == want.nodes.tobytes()
    if min_visits == 300:
        assert all(len(t) == 0 for t in got)        # the roots have 201 visits: a dropped root drops the tree


def test_principal_variations_equal_the_host_walk(searched):
    from connect4_amd.tree import Tree
    eng, group = searched
    whole = eng.export_trees()
    for rule in ("value", "visits"):
        lines = eng.principal_variations(rule=rule)
        assert len(lines) == 24
        longest = 0
        for (moves, visits, values), t in zip(lines, whole):
            want = Tree(t).principal_variation(rule)
            assert moves.tolist() == [w[0] for w in want] and visits.tolist() == [w[1] for w in want], rule
            assert [None if np.isnan(v) else v for v in values.tolist()] == [w[2] for w in want], rule
            longest = max(longest, len(want))
        assert longest >= 4
        slots = [17, 3, 9]
        sub = eng.principal_variations(slots, rule=rule, max_len=2)
        for (moves, visits, values), g in zip(sub, slots):
            assert moves.tolist() == lines[g][0][:2].tolist() and values.tolist() == lines[g][2][:2].tolist()


# ---------------------------------------------------------------------------------------------- at size
def seeded_openings(n, seed, max_plies):
    from connect4_amd.board import Board
    rng = np.random.RandomState(seed)
    boards = []
    while len(boards) < n:
        b = Board()
        for _ in range(int(rng.randint(0, max_plies))):
            b.make_move(int(rng.choice(sorted(b.valid_moves))))
            if b.result is not None:
                break
        if b.result is None:
            boards.append(b)
    return boards


def test_4096_slots_800_simulations():
    """4,096 searches x 800 simulations of the centre evaluator from seeded openings.  The oracle gives roots only, so whole-tree
    truth at this size rests on invariants -- for EVERY slot the root row and the root's children equal c4_read_roots, the
    sum rule holds at every node, the nodes with children are the slot's expansions -- plus the fixtures' node-for-node parity
    above.  With min_visits=1 a tree has the root and one new node per simulation, 801 nodes, less the simulations that ended on a
    finished position visited before."""
    from connect4_amd import _lib as L
    G, S = 4096, 800
    boards = seeded_openings(G, 11, 20)
    c = dict(simulations=S, pb_c_base=19652, pb_c_init=1.25, root_dirichlet_alpha=0.0, root_exploration_fraction=0.0,
             num_sampling_moves=0)
    with make_engine(c, G, L.EVAL_CENTRE, stop_after_move=True) as eng:
        eng.reset([b.color[0] for b in boards], [b.color[1] for b in boards])
        eng.run_centre()
        roots = eng.read_roots()
        visited = eng.export_trees(min_visits=1)
        sizes = eng.tree_sizes(min_visits=1)
        sample = np.random.RandomState(2).choice(G, size=64, replace=False)
        full = eng.export_trees(sample)
    assert sizes.tolist() == [len(t) for t in visited]
    nodes = visited[0].nodes.base if visited[0].nodes.base is not None else visited[0].nodes
    assert len(nodes) == sizes.sum()
    # the sum rule and the expansion count for all 4,096 trees at once, on the one buffer they share
    start = np.concatenate(([0], np.cumsum(sizes)))
    tree_of = np.repeat(np.arange(G), sizes)
    parent = nodes["parent"].astype(np.int64) + start[tree_of]
    inner = nodes["parent"] >= 0
    below = np.bincount(parent[inner], weights=nodes["visits"][inner], minlength=len(nodes)).astype(np.int64)
    kids = nodes["n_children"] > 0
    assert (nodes["visits"][kids] == 1 + below[kids]).all()
    assert (kids == ((nodes["status"] < 0) & (nodes["visits"] >= 2))).all()
    assert (np.bincount(parent[inner], minlength=len(nodes)) == nodes["n_children"]).all()
    assert (nodes["visits"] >= 1).all()
    # every simulation visits one new node, except those that end on a finished position somebody has been to before
    terminal = nodes["status"] >= 0
    revisits = np.bincount(tree_of[terminal], weights=nodes["visits"][terminal] - 1, minlength=G).astype(np.int64)
    assert (sizes == S + 1 - revisits).all()
    assert (revisits == 0).sum() >= 64 and (revisits > 0).sum() >= 64      # both kinds of tree are here, 801-node ones included
    expansions = np.bincount(tree_of[kids], minlength=G)
    for g, (r, t, b) in enumerate(zip(roots, visited, boards)):
        assert r.state == 2 and t.slot == g
        assert (int(t.color0[0]), int(t.color1[0])) == (b.color[0], b.color[1]) == (r.color0, r.color1)
        assert t.visits[0] == r.root_visits == S + 1 and t.value_sum[0] == r.root_value_sum
        assert list(t.prior[0]) == list(r.root_prior) and t.prior_kind[0] == L.PRIOR_F64
        cols = [m for m in range(7) if r.child_status[m] != -2 and r.child_visits[m] >= 1]
        k0, k1 = int(t.first_child[0]), int(t.first_child[0]) + int(t.n_children[0])
        assert t.move[k0:k1].tolist() == cols
        assert t.visits[k0:k1].tolist() == [r.child_visits[m] for m in cols]
        assert t.value_sum[k0:k1].tolist() == [r.child_value_sum[m] for m in cols]
        assert t.status[k0:k1].tolist() == [r.child_status[m] for m in cols]
        assert expansions[g] == r.expansions
    for t, g in zip(full, sample):
        assert len(t) > len(visited[g])
        assert t.filtered(min_visits=1).nodes.tobytes() == visited[g].nodes.tobytes()
        check_invariants(t, "slot %d" % g)


# ---------------------------------------------------------------------------------------------- when a tree may be read
def test_slot_that_is_still_searching():
    """Between two launches of an unfinished search the export is a consistent snapshot: same root row as c4_read_roots at that
    moment, and the counts add up (what is under way has not been backed up)."""
    from connect4_amd import _lib as L
    c = dict(simulations=800, pb_c_base=19652, pb_c_init=1.25, root_dirichlet_alpha=0.0, root_exploration_fraction=0.0,
             num_sampling_moves=0)
    boards = seeded_openings(64, 5, 12)
    with make_engine(c, 64, L.EVAL_CENTRE, stop_after_move=True, max_inner_iters=40) as eng:
        eng.reset([b.color[0] for b in boards], [b.color[1] for b in boards])
        eng.run_centre(max_launches=1)
        roots = eng.read_roots()
        tables = eng.export_trees()
        for r, t in zip(roots, tables):
            assert r.state == 0                         # still searching
            assert 1 < r.root_visits < 801
            assert t.visits[0] == r.root_visits and t.value_sum[0] == r.root_value_sum
            k0, k1 = int(t.first_child[0]), int(t.first_child[0]) + int(t.n_children[0])
            assert t.visits[k0:k1].tolist() == [r.child_visits[int(m)] for m in t.move[k0:k1]]
            check_invariants(t, "snapshot")
        eng.run_centre()
        for r, t in zip(eng.read_roots(), eng.export_trees(min_visits=1)):
            assert r.state == 2 and len(t) == 801 - int((t.visits[t.status >= 0] - 1).sum())


def test_pending_leaf_and_pending_root():
    """An engine whose evaluator lives on the host: before the root's answer has arrived the slot has no tree (0 nodes); with a
    leaf waiting for its answer the tree is exported without that leaf's visit, and the sum rule holds."""
    import torch
    from connect4_amd import _lib as L
    from connect4_amd.board import Board
    from connect4_amd.evaluators import evaluate_centre_with_prior
    c = dict(simulations=100, pb_c_base=19652, pb_c_init=1.25, root_dirichlet_alpha=0.0, root_exploration_fraction=0.0,
             num_sampling_moves=0)
    with make_engine(c, 4, L.EVAL_EXTERNAL_F64, stop_after_move=True) as eng:
        eng.reset(n_active=3)                            # slot 3 parks without a tree
        assert eng.tree_sizes().tolist() == [0, 0, 0, 0]
        values = torch.zeros(4, dtype=torch.float64, device="cuda")
        priors = torch.zeros(4, 7, dtype=torch.float64, device="cuda")
        eng.step(None, None, None)                       # the roots now wait for the evaluator
        assert eng.tree_sizes().tolist() == [0, 0, 0, 0]
        assert all(len(m) == 0 for m, _, _ in eng.principal_variations())
        for step in range(30):
            c0, c1, has = eng.read_leaves()
            hv, hp = np.zeros(4), np.zeros((4, 7))
            for g in np.nonzero(has)[0]:
                hv[g], hp[g] = evaluate_centre_with_prior(Board.from_bits(int(c0[g]), int(c1[g])))
            values.copy_(torch.from_numpy(hv))
            priors.copy_(torch.from_numpy(hp))
            eng.step(values, priors, None)
        _, _, has = eng.read_leaves()
        assert has[:3].all()                             # a leaf of every live slot is with the evaluator
        tables = eng.export_trees()
        assert len(tables[3]) == 0
        for r, t in zip(eng.read_roots()[:3], tables[:3]):
            assert r.state == 0 and t.visits[0] == r.root_visits and r.root_visits >= 2
            check_invariants(t, "pending leaf")


def test_engine_driven_by_the_fused_selfplay_kernel():
    """c4_selfplay_steps (split mode) keeps node 0 and the pool current and writes the slot state back when a launch ends
    (include/c4_engine.h: "When a tree may be read"), so trees are readable between its launches: every slot either has no
    tree of its root position right now (its root waits for the network) or exports one that obeys every invariant and whose
    root row is what c4_read_roots reports."""
    from connect4_amd import _lib as L
    from connect4_amd.config import MCTSConfig
    from connect4_amd.fused_net import FusedNet
    from connect4_amd.net import random_init_state_dict
    from connect4_amd.selfplay import SelfPlay
    from connect4_amd.tree import Tree
    cfg = MCTSConfig.self_play(200)
    net = FusedNet(random_init_state_dict(seed=0))
    sp = SelfPlay(net, 64, cfg, seed=3, use_graph=False, fused_loop=True, steps_per_launch=16)
    try:
        sp.engine.reset()
        with_tree = 0
        for launch in range(4):
            sp.run_steps(16)
            sp.synchronize()
            roots = sp.engine.read_roots()
            tables = sp.engine.export_trees()
            lines = sp.engine.principal_variations(rule="visits")
            for r, t, (moves, _, _) in zip(roots, tables, lines):
                if len(t) == 0:
                    assert len(moves) == 0
                    continue
                with_tree += 1
                assert (int(t.color0[0]), int(t.color1[0])) == (r.color0, r.color1)
                assert t.visits[0] == r.root_visits and t.value_sum[0] == r.root_value_sum
                assert list(t.prior[0]) == list(r.root_prior) and t.prior_kind[0] == L.PRIOR_F64      # the noisy root
                assert (t.prior_kind[1:][t.prior_kind[1:] != 0] == L.PRIOR_F32).all()                  # the net's answers
                check_invariants(t, "fused launch %d" % launch)
                assert moves.tolist() == [m for m, _, _ in Tree(t).principal_variation("visits")]
        assert with_tree >= 128                          # most slots, most of the time
        assert sp.stats()["bad_evals"] == 0
    finally:
        sp.close()
        net.close()


# ---------------------------------------------------------------------------------------------- errors
def test_bad_calls_are_refused_and_the_engine_stays_usable(searched):
    import ctypes as C
    from connect4_amd import _lib as L
    eng, group = searched
    before = eng.export_trees([2, 5])
    total = sum(len(t) for t in before)
    for slots in ([24], [-1], [2, 5, 2], list(range(24)) + [0]):
        for call in (eng.export_trees, eng.tree_sizes, eng.principal_variations):
            with pytest.raises(L.EngineError) as ei:
                call(slots)
            assert ei.value.code == L.EINVAL and "slot" in str(ei.value)
    with pytest.raises(L.EngineError) as ei:
        eng.export_trees([2, 5], capacity=total - 1)     # one node short
    assert ei.value.code == L.EINVAL and str(total) in str(ei.value)
    with pytest.raises(L.EngineError):
        eng.export_trees([2, 5], min_visits=-1)
    with pytest.raises(L.EngineError):
        eng.principal_variations([2], max_len=0)
    off = np.zeros(3, dtype=np.int64)
    sl = np.array([2, 5], dtype=np.int32)
    rc = eng._lib.c4_export_trees(eng._h, sl.ctypes.data_as(C.POINTER(C.c_int32)), 2, 0, -1, None, total, off.ctypes.data_as(C.POINTER(C.c_int64)))
    assert rc == L.EINVAL and "null" in L.last_error(eng._h)
    rc = eng._lib.c4_tree_sizes(eng._h, None, 2, 0, -1, None)
    assert rc == L.EINVAL
    after = eng.export_trees([2, 5], capacity=total)      # exactly enough
    assert [t.nodes.tobytes() for t in after] == [t.nodes.tobytes() for t in before]
    assert_tables_equal(after[0], group[2].table(), group[2].name)
