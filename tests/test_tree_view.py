"""Whole search trees on the CPU: the fixtures of tests/golden/search_trees.npz (whole trees of the unmodified reference)
check themselves against the root rows that search_centre.json / search_net.json pin, and connect4_amd.tree.Tree built
from their arrays is walked through the reference's surface (tree.py:18-117) node by node."""
import numpy as np
import pytest

from conftest import load_json
from tree_fixture import load_tree_cases


@pytest.fixture(scope="module")
def cases():
    return load_tree_cases()


@pytest.fixture(scope="module")
def tables(cases):
    return {c.name: c.table() for c in cases}


@pytest.fixture(scope="module")
def pinned():
    return {c["name"]: c for c in load_json("search_centre.json") + load_json("search_net.json")}


def legal_columns(c0, c1):
    occ = int(c0) | int(c1)
    return [c for c in range(7) if bin((occ >> (7 * c)) & 0x7f).count("1") < 6]


def test_node_layout_matches_the_header():
    """c4_tree_node crosses the ABI as rows of a NumPy structured array: 104 bytes, fields where the C compiler puts them."""
    import ctypes
    from connect4_amd import _lib as L
    dt = L.tree_node_dtype()
    assert dt.itemsize == ctypes.sizeof(L.TreeNode) == 104
    for name, _ in L.TreeNode._fields_:
        assert dt.fields[name][1] == getattr(L.TreeNode, name).offset, name
    assert dt["prior"].shape == (7,)


def test_fixture_covers_the_pinned_searches(cases, pinned):
    names = {c.name for c in cases}
    want = {n for n, c in pinned.items() if c["config"]["simulations"] <= 3200}
    assert want <= names and len(want) == 49 + 15
    deep = [c for c in cases if c.kind == "deep"]
    assert len(deep) >= 4
    for c in deep:
        assert bin(c.c0 | c.c1).count("1") >= 30
    assert max(len(c) for c in cases) == 18064


def test_fixture_roots_equal_the_pinned_roots(cases, pinned):
    for c in cases:
        if c.kind == "deep":
            continue
        j = pinned[c.name]
        assert (c.c0, c.c1) == (j["board"]["c0"], j["board"]["c1"]) and c.config == j["config"]
        assert (c.noise is None) == (j["noise"] is None) and (c.noise is None or list(c.noise) == j["noise"])
        assert int(c.visits[0]) == j["root_N"] and float(c.value_sum[0]) == j["root_W"], c.name
        N, W, status = [0] * 7, [0.0] * 7, [-2] * 7
        for i in np.nonzero(c.parent == 0)[0]:
            N[c.move[i]], W[c.move[i]], status[c.move[i]] = int(c.visits[i]), float(c.value_sum[i]), int(c.status[i])
        assert N == j["N"] and W == j["W"] and status == j["status"], c.name
        assert list(c.prior[0]) == j["root_prior"], c.name
        assert len(c) == j["n_nodes"], c.name
        assert len(set(c.parent[1:].tolist())) == j["n_expansions"], c.name


def test_fixture_invariants(cases, tables):
    for c in cases:
        t = tables[c.name]
        n = len(c)
        kids = np.bincount(c.parent[1:], minlength=n)
        child_visits = np.bincount(c.parent[1:], weights=c.visits[1:], minlength=n).astype(np.int64)
        terminal = c.status >= 0
        assert not (kids[terminal] > 0).any(), c.name
        # children iff visits >= 2 (mcts.py:113-116), the root included
        assert ((kids > 0) == (~terminal & (c.visits >= 2))).all(), c.name
        # every visit of a node with children went on into one of them, except the one that evaluated it
        par = kids > 0
        assert (c.visits[par] == 1 + child_visits[par]).all(), c.name
        # breadth-first, within a parent by ascending column
        assert (np.diff(c.parent[1:]) >= 0).all(), c.name
        same = c.parent[2:] == c.parent[1:-1]
        assert (c.move[2:][same] > c.move[1:-1][same]).all(), c.name
        # position_value: present exactly at the evaluated (visited, undecided) nodes
        assert ((c.prior_kind != 0) == (~terminal & (c.visits >= 1))).all(), c.name
        for i in np.nonzero(c.prior_kind != 0)[0]:
            legal = legal_columns(t.color0[i], t.color1[i])
            p = c.prior[i]
            assert all(p[m] == 0.0 for m in range(7) if m not in legal), (c.name, i)
            # 1e-6 where the prior was normalised in float32, 1e-12 where in float64.  The dtype tells which, except at the
            # noisy root of a net search: mcts.py:180 mixes the net's float32-normalised prior with the noise in float64,
            # so that one float64 row carries float32's rounding (measured on the 7 such roots: up to 3.8e-8)
            f32_normalised = c.prior_kind[i] == 1 or (c.kind == "net" and i == 0)
            assert abs(float(np.sum(p[legal])) - 1.0) <= (1e-6 if f32_normalised else 1e-12), (c.name, i)
        # kinds: a net answers float32, the centre evaluator and a noisy root float64
        if c.kind == "net":
            assert (c.prior_kind[1:][c.prior_kind[1:] != 0] == 1).all()
            assert c.prior_kind[0] == (2 if c.noise is not None else 1)
        else:
            assert (c.prior_kind[c.prior_kind != 0] == 2).all()


def test_tree_walk_equals_the_arrays(cases, tables):
    """Every node of every fixture tree through the reference's surface."""
    from connect4_amd.board import Board
    from connect4_amd.tree import Tree
    from connect4_amd.utils import Side
    for c in cases:
        tree = Tree(tables[c.name])
        assert tree.n_nodes == len(c) and tree.side == Side(bin(c.c0 | c.c1).count("1") % 2)
        root = tree.root
        assert root.name == "root" and root.is_root and root.parent is None
        assert root.data.board == Board.from_bits(c.c0, c.c1)
        level, row = [root], 0
        while level:
            nxt = []
            for node in level:            # breadth-first walk = table order
                i = row
                row += 1
                assert node.row == i
                d = node.data
                if i:
                    assert node.name == c.move[i] and not node.is_root and node.parent.row == c.parent[i]
                    b = node.parent.data.board.copy()
                    b.make_move(int(c.move[i]))
                    assert d.board == b and d.board.age == b.age
                assert d.board.result == (None if c.status[i] < 0 else d.board.result) and \
                    (d.board.result is None) == (c.status[i] < 0)
                if c.status[i] >= 0:
                    assert d.board.result.value == 0.5 * c.status[i]
                assert d.valid_moves == d.board.valid_moves
                if c.visits[i] == 0:
                    assert d.search_value is None
                else:
                    assert d.search_value.visit_count == c.visits[i] and d.search_value.value_sum == c.value_sum[i]
                    assert float(d.search_value) == c.value_sum[i] / c.visits[i]
                if c.prior_kind[i] == 0:
                    assert d.position_value is None
                else:
                    pr = d.position_value.prior
                    assert pr.dtype == (np.float32 if c.prior_kind[i] == 1 else np.float64)
                    assert (pr.astype(np.float64) == c.prior[i]).all()
                    assert d.position_value.value == (c.value_sum[i] if c.visits[i] == 1 else None)
                av = 0.5 * c.status[i] if c.status[i] >= 0 else (c.value_sum[i] / c.visits[i] if c.visits[i] else None)
                assert d.absolute_value == av
                assert d.value(Side.o) == (0.0 if av is None else av) and d.value(Side.x) == (0.0 if av is None else 1.0 - av)
                kids = node.children
                assert isinstance(kids, tuple) and kids is node.children
                assert [k.name for k in kids] == sorted(k.name for k in kids)
                assert [k.row for k in kids] == np.nonzero(c.parent == i)[0].tolist() if len(c) < 2000 else True
                nxt.extend(kids)
            level = nxt
        assert row == len(c)


def test_root_answers_equal_the_pinned_ones(cases, tables, pinned):
    from connect4_amd.tree import Tree
    for c in cases:
        if c.kind == "deep":
            continue
        j, tree = pinned[c.name], Tree(tables[c.name])
        assert tree.best_move().name == j["best_move"], c.name
        assert list(tree.get_values_policy()) == j["values_policy"], c.name
        assert list(tree.get_visit_count_policy()) == j["visit_policy"], c.name
        assert [tree.get_node_value(k) for k in tree.root.children] == [j["child_value"][k.name] for k in tree.root.children]
        mv = tree.most_visited()
        assert (mv.data.search_value.visit_count if mv.data.search_value else 0) == max(j["N"])
        assert tree.child(j["best_move"]).name == j["best_move"]
        assert list(tree.root_prior) == j["root_prior"]
        assert tree.simulations == j["config"]["simulations"] and tree.expansions == j["n_expansions"]


def test_nodes_are_built_lazily(cases, tables):
    from connect4_amd.tree import Tree
    c = max(cases, key=len)
    assert len(c) == 18064
    tree = Tree(tables[c.name])
    assert tree.nodes_created == 1
    node, plies = tree.root, 0
    while node.children:      # one line: the most visited child at every node
        node = max(node.children, key=lambda k: (k.data.search_value.visit_count if k.data.search_value else 0, k.name))
        plies += 1
    assert plies >= 3 and tree.nodes_created < 200


def walk(c, kids, row, side, rule):
    """The principal variation below `row`, the plain way: Tree.best_move / most_visited of the reference at every node."""
    if not kids[row]:
        return []

    def absolute(k):
        return 0.5 * c.status[k] if c.status[k] >= 0 else (c.value_sum[k] / c.visits[k] if c.visits[k] else None)

    def key(k):
        if rule == "visits":
            return (int(c.visits[k]), int(c.move[k]))
        a = absolute(k)
        return (0.0 if a is None else (a if side == 0 else 1.0 - a), int(c.move[k]))
    best = max(kids[row], key=key)
    return [(int(c.move[best]), int(c.visits[best]), absolute(best))] + walk(c, kids, best, side ^ 1, rule)


def children_lists(c):
    kids = [[] for _ in range(len(c))]
    for i, p in enumerate(c.parent.tolist()[1:], 1):
        kids[p].append(i)
    return kids


def test_principal_variation(cases, tables):
    from connect4_amd.tree import Tree
    longest = 0
    for c in cases:
        tree, kids = Tree(tables[c.name]), children_lists(c)
        side = bin(c.c0 | c.c1).count("1") % 2
        for rule in ("value", "visits"):
            line = tree.principal_variation(rule)
            assert line == walk(c, kids, 0, side, rule), (c.name, rule)
            longest = max(longest, len(line))
        assert tree.nodes_created == 1          # the arrays were walked, no node objects
    assert longest >= 8
    with pytest.raises(ValueError):
        tree.principal_variation("depth")


def test_render_has_one_line_per_kept_node(cases, tables):
    from connect4_amd.tree import Tree
    for c in cases[::5] + [max(cases, key=len)]:
        tree, t = Tree(tables[c.name]), tables[c.name]
        for max_depth, min_visits in ((None, 1), (2, 1), (None, 5), (3, 0)):
            keep = np.zeros(len(c), dtype=bool)
            for i in range(len(c)):
                ok = c.visits[i] >= min_visits and (max_depth is None or t.depth[i] <= max_depth)
                keep[i] = ok and (i == 0 or keep[c.parent[i]])
            text = tree.render(max_depth=max_depth, min_visits=min_visits)
            lines = text.splitlines()
            assert len(lines) == int(keep.sum()), (c.name, max_depth, min_visits)
            assert not lines or lines[0].startswith("root  n=%d" % c.visits[0])
            assert len(t.filtered(min_visits, max_depth)) == int(keep.sum())
    assert len(Tree(tables[cases[0].name]).render().split("\n")) == int((cases[0].visits >= 1).sum())


def test_root_only_tree_keeps_its_surface(cases, tables, pinned):
    """Tree(root_result, board), today's root-only tree, answers as before and has the new helpers over its 1 + children rows."""
    from connect4_amd import _lib as L
    from connect4_amd.board import Board
    from connect4_amd.tree import Tree
    c = next(x for x in cases if x.name == "empty_s200")
    j = pinned[c.name]
    r = L.RootResult()
    r.state, r.move, r.root_visits, r.root_value_sum = 2, j["best_move"], j["root_N"], j["root_W"]
    r.color0, r.color1, r.expansions, r.simulations = c.c0, c.c1, j["n_expansions"], 200
    for m in range(7):
        r.child_visits[m], r.child_value_sum[m], r.child_status[m] = j["N"][m], j["W"][m], j["status"][m]
        r.root_prior[m], r.values_policy[m] = j["root_prior"][m], j["values_policy"][m]
    small, whole = Tree(r, Board.from_bits(c.c0, c.c1)), Tree(tables[c.name])
    assert small.n_nodes == 8 and all(k.children == () for k in small.root.children)
    assert small.best_move().name == whole.best_move().name == j["best_move"]
    assert list(small.get_values_policy()) == list(whole.get_values_policy())
    assert list(small.get_visit_count_policy()) == list(whole.get_visit_count_policy())
    assert small.principal_variation("value") == whole.principal_variation("value")[:1]
    assert small.principal_variation("visits") == whole.principal_variation("visits")[:1]
    assert small.render().split("\n") == whole.render(max_depth=1).split("\n")
