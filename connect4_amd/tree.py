"""Read-only view of a finished search with the reference's Tree surface
(oinkoink/tree.py:61-117): callers use ``tree.get_values_policy()`` (training_game.py:14),
``tree.get_visit_count_policy()`` (game.py:35) and, in tests/tools, the nodes'
``name`` / ``data.search_value.visit_count`` / ``data.absolute_value``.

Two backings.  ``Tree(root_result, board)`` is one c4_root_result copied from the device: the root and
its children; the tree itself stays in HBM.  ``Tree(table, board)`` with a :class:`TreeTable` -- what
``Engine.export_trees`` returns, or arrays of the same content -- is the WHOLE tree:
``tree.root.children[i].children[j]...`` with the reference's surface per node, built lazily from the
table's NumPy arrays (a node object exists only once somebody walks to it)."""
import numpy as np

from ._lib import PRIOR_F32, PRIOR_F64, PRIOR_NONE, tree_node_dtype
from .board import H1, Board
from .utils import Side, value_to_side


class _Search:
    def __init__(self, n, w):
        self.visit_count = int(n)
        self.value_sum = float(w)

    def __float__(self):
        return self.value_sum / self.visit_count


class _ChildData:
    def __init__(self, board, status, n, w):
        self.board = board
        self.search_value = _Search(n, w) if n > 0 else None
        self._status = status

    @property
    def absolute_value(self):          # tree.py:27-38
        if self._status >= 0:
            return 0.5 * self._status
        if self.search_value is not None:
            return float(self.search_value)
        return None

    def value(self, side):             # tree.py:40-44
        v = self.absolute_value
        return 0.0 if v is None else value_to_side(v, side)


class _Node:
    def __init__(self, name, data, parent=None):
        self.name = name
        self.data = data
        self.parent = parent
        self.children = ()

    @property
    def is_root(self):
        return self.parent is None

    def __gt__(self, other):           # tree.py:11-15
        return self.name > other.name


# ---------------------------------------------------------------------------------------------
# whole trees
# ---------------------------------------------------------------------------------------------
class TreeTable:
    """One exported tree: a structured NumPy array of c4_tree_node rows (include/c4_engine.h) in breadth-first
    order -- within a level by parent, within a parent by ascending column -- so a node's children are the rows
    ``first_child .. first_child + n_children - 1`` in the order of the reference's ``node.children``.  The fields
    (``parent``, ``move``, ``depth``, ``first_child``, ``n_children``, ``color0``, ``color1``, ``visits``,
    ``value_sum``, ``status``, ``prior``, ``prior_kind``) are attributes: views, no per-node copies."""
    FIELDS = ("parent", "first_child", "visits", "move", "depth", "n_children", "status", "value_sum", "color0",
              "color1", "prior", "prior_kind")

    def __init__(self, nodes, slot=None):
        self.nodes = nodes
        self.slot = slot

    def __len__(self):
        return len(self.nodes)

    def __getattr__(self, name):
        if name in TreeTable.FIELDS:
            return self.nodes[name]
        raise AttributeError(name)

    @classmethod
    def from_arrays(cls, color0, color1, parent, move, visits, value_sum, status, prior=None, prior_kind=None):
        """A table from the reference-side content alone (rows already in table order): depth, the children's
        rows and the boards are derived here, the boards by replaying the moves."""
        n = len(parent)
        t = np.zeros(n, dtype=tree_node_dtype())
        t["parent"], t["move"], t["visits"], t["value_sum"], t["status"] = parent, move, visits, value_sum, status
        if prior is not None:
            t["prior"], t["prior_kind"] = prior, prior_kind
        t["first_child"] = -1
        par = t["parent"]
        if n:
            assert par[0] == -1 and (n == 1 or (np.diff(par[1:]) >= 0).all()), "rows are not in breadth-first order"
            kids = np.bincount(par[1:], minlength=n)
            t["n_children"] = kids
            first = np.concatenate(([1], 1 + np.cumsum(kids)[:-1]))
            t["first_child"] = np.where(kids > 0, first, -1)
            c0, c1, depth = [int(color0)] + [0] * (n - 1), [int(color1)] + [0] * (n - 1), [0] * n
            mv = t["move"].tolist()
            for i, p in enumerate(par.tolist()[1:], 1):
                a, b = c0[p], c1[p]
                occ = a | b
                stone = 1 << (H1 * mv[i] + bin((occ >> (H1 * mv[i])) & 0x7f).count("1"))
                if bin(occ).count("1") & 1:
                    b ^= stone
                else:
                    a ^= stone
                c0[i], c1[i], depth[i] = a, b, depth[p] + 1
            t["color0"], t["color1"], t["depth"] = np.array(c0, dtype=np.uint64), np.array(c1, dtype=np.uint64), depth
        return cls(t)

    def filtered(self, min_visits=0, max_depth=None):
        """The table the device writes under the same filters: a dropped node drops its subtree."""
        n = len(self)
        keep = np.zeros(n, dtype=bool)
        ok = self.visits >= min_visits
        if max_depth is not None:
            ok &= self.depth <= max_depth
        par = self.parent
        for i in range(n):
            keep[i] = ok[i] and (i == 0 or keep[par[i]])
        new_row = np.cumsum(keep) - 1
        sub = self.nodes[keep].copy()
        if len(sub):
            sub["parent"][1:] = new_row[sub["parent"][1:]]
            kids = np.bincount(sub["parent"][1:], minlength=len(sub))
            sub["n_children"] = kids
            first = np.concatenate(([1], 1 + np.cumsum(kids)[:-1]))
            sub["first_child"] = np.where(kids > 0, first, -1)
        return TreeTable(sub, self.slot)


class _Position:
    """position_value (mcts.py:29-44).  ``value``, the node's own evaluation, is not kept by the engine once a node
    has more than one visit: it is exact where visits == 1 (it is the value sum) and None otherwise."""

    def __init__(self, value, prior):
        self.value = value
        self.prior = prior

    def __float__(self):
        return float(self.value)


class _TableData:
    """NodeData (tree.py:18-58) of one table row."""
    __slots__ = ("_t", "_i", "_board")

    def __init__(self, table, row):
        self._t, self._i, self._board = table, row, None

    @property
    def board(self):
        if self._board is None:
            self._board = Board.from_bits(int(self._t.color0[self._i]), int(self._t.color1[self._i]))
        return self._board

    @property
    def valid_moves(self):
        return self.board.valid_moves

    @property
    def search_value(self):
        n = int(self._t.visits[self._i])
        return _Search(n, self._t.value_sum[self._i]) if n > 0 else None

    @property
    def position_value(self):
        kind = int(self._t.prior_kind[self._i])
        if kind == PRIOR_NONE:
            return None
        prior = np.array(self._t.prior[self._i], dtype=np.float32 if kind == PRIOR_F32 else np.float64)
        return _Position(float(self._t.value_sum[self._i]) if self._t.visits[self._i] == 1 else None, prior)

    @property
    def absolute_value(self):          # tree.py:27-38
        st = int(self._t.status[self._i])
        if st >= 0:
            return 0.5 * st
        sv = self.search_value
        return None if sv is None else float(sv)

    def value(self, side):             # tree.py:40-44
        v = self.absolute_value
        return 0.0 if v is None else value_to_side(v, side)


class _TableNode:
    """anytree.Node as the reference uses it, over one table row; children are made when first asked for."""
    __slots__ = ("_tree", "_i", "parent", "_children", "_data")

    def __init__(self, tree, row, parent):
        self._tree, self._i, self.parent, self._children, self._data = tree, row, parent, None, None
        tree.nodes_created += 1

    @property
    def name(self):
        return "root" if self._i == 0 else int(self._tree.table.move[self._i])

    @property
    def row(self):
        return self._i

    @property
    def is_root(self):
        return self.parent is None

    @property
    def data(self):
        if self._data is None:
            self._data = _TableData(self._tree.table, self._i)
        return self._data

    @property
    def children(self):
        if self._children is None:
            t = self._tree.table
            first, n = int(t.first_child[self._i]), int(t.n_children[self._i])
            self._children = tuple(_TableNode(self._tree, first + k, self) for k in range(n))
        return self._children

    def __gt__(self, other):           # tree.py:11-15
        return self.name > other.name


class Tree:
    def __init__(self, root_result, board: Board = None, root_result_of_table=None):
        self.nodes_created = 0
        if isinstance(root_result, TreeTable):
            self._init_whole(root_result, board, root_result_of_table)
            return
        r = root_result
        self.side = Side(board.age % 2)
        rb = Board.from_bits(int(r.color0), int(r.color1))
        self.root = _Node("root", _ChildData(rb, -1, r.root_visits, r.root_value_sum))
        kids = []
        for m in range(7):
            st = r.child_status[m]
            if st == -2:
                continue
            cb = rb.__copy__()
            cb.make_move(m)
            kids.append(_Node(m, _ChildData(cb, st, r.child_visits[m], r.child_value_sum[m]), self.root))
        self.root.children = tuple(kids)
        self.root_prior = np.array(list(r.root_prior), dtype=np.float64)
        self._values_policy = np.array(list(r.values_policy), dtype=np.float64)
        self.expansions = int(r.expansions)
        self.simulations = int(r.simulations)
        self._table = None
        self._result = r

    def _init_whole(self, table, board, r):
        if len(table) == 0:
            raise ValueError("the table is empty: the slot held no tree")
        self._table = table
        self._result = r
        age = bin(int(table.color0[0])).count("1") + bin(int(table.color1[0])).count("1")
        if board is not None and (board.color[0] != int(table.color0[0]) or board.color[1] != int(table.color1[0])):
            raise ValueError("the table's root is not this board")
        self.side = Side(age % 2)
        self.root = _TableNode(self, 0, None)
        self.root_prior = np.array(table.prior[0], dtype=np.float64)
        self._values_policy = None if r is None else np.array(list(r.values_policy), dtype=np.float64)
        self.expansions = int(r.expansions) if r is not None else int((table.n_children > 0).sum())
        self.simulations = int(r.simulations) if r is not None else int(table.visits[0]) - 1

    # -- the table behind the tree ---------------------------------------------------------------
    @property
    def table(self):
        """The tree as a TreeTable; a root-only tree gives the root and its children."""
        if self._table is None:
            r = self._result
            cols = [m for m in range(7) if r.child_status[m] != -2]
            n = 1 + len(cols)
            prior = np.zeros((n, 7))
            prior[0] = list(r.root_prior)
            kind = np.zeros(n, dtype=np.int32)
            kind[0] = PRIOR_F64
            self._table = TreeTable.from_arrays(
                r.color0, r.color1, [-1] + [0] * len(cols), [-1] + cols, [r.root_visits] + [r.child_visits[m] for m in cols],
                [r.root_value_sum] + [r.child_value_sum[m] for m in cols], [-1] + [r.child_status[m] for m in cols], prior, kind)
        return self._table

    @property
    def n_nodes(self):
        return len(self.table)

    # -- the reference's Tree surface ------------------------------------------------------------
    def get_node_value(self, node):
        return node.data.value(self.side)

    def best_move(self):
        return max(((self.get_node_value(c), c) for c in self.root.children))[1]

    def most_visited(self):
        return max(((c.data.search_value.visit_count if c.data.search_value else 0, c)
                    for c in self.root.children))[1]

    def get_values_policy(self):
        """Computed on the device by the move-choice code (tree.py:104-109,139-147); for a tree built from arrays
        alone, the same operations here."""
        if self._values_policy is not None:
            return self._values_policy.copy()
        p = np.zeros(7)
        for c in self.root.children:
            p[c.name] = self.get_node_value(c)
        return self._normalise(p)

    def _normalise(self, p):            # tree.py:139-147
        s = np.sum(p)
        if s == 0.0:
            for c in self.root.children:
                p[c.name] = 1.0
            p /= len(self.root.children)
        else:
            p /= s
        return p

    def get_visit_count_policy(self):
        p = np.zeros(7)
        for c in self.root.children:
            if c.data.search_value is not None:
                p[c.name] = c.data.search_value.visit_count
        return self._normalise(p)

    def child(self, move):
        for c in self.root.children:
            if c.name == move:
                return c
        raise KeyError(move)

    # -- whole-tree helpers ----------------------------------------------------------------------
    def _abs_value(self, row):
        t = self.table
        st = int(t.status[row])
        if st >= 0:
            return 0.5 * st
        n = int(t.visits[row])
        return float(t.value_sum[row]) / n if n > 0 else None

    def principal_variation(self, rule="value"):
        """The line the search expects: from the root repeatedly the child ``best_move`` (rule "value": largest
        value for the side to move at that node) or ``most_visited`` (rule "visits") takes, ties to the higher
        column, until a node without children.  A list of (move, visits, absolute_value) per step."""
        if rule not in ("value", "visits"):
            raise ValueError("rule is 'value' or 'visits'")
        t = self.table
        row, side, line = 0, int(self.side), []
        while int(t.n_children[row]) > 0:
            first = int(t.first_child[row])
            best = None
            for k in range(first, first + int(t.n_children[row])):
                if rule == "visits":
                    key = int(t.visits[k])
                else:
                    v = self._abs_value(k)
                    key = 0.0 if v is None else value_to_side(v, Side(side))
                cand = (key, int(t.move[k]), k)
                if best is None or cand[:2] > best[:2]:
                    best = cand
            row = best[2]
            line.append((int(t.move[row]), int(t.visits[row]), self._abs_value(row)))
            side ^= 1
        return line

    def render(self, max_depth=None, min_visits=1):
        """Indented text, one node per line (depth first, children by column): move, visits, mean value, prior --
        what RenderTree prints in the reference's tests.  A node below min_visits or max_depth is left out with
        its subtree."""
        t = self.table
        lines = []
        stack = [0]
        while stack:
            i = stack.pop()
            if int(t.visits[i]) < min_visits or (max_depth is not None and int(t.depth[i]) > max_depth):
                continue
            v = self._abs_value(i)
            text = "%s%s  n=%d  v=%s" % ("  " * int(t.depth[i]), "root" if i == 0 else int(t.move[i]), int(t.visits[i]),
                                         "-" if v is None else "%.4f" % v)
            p = int(t.parent[i])
            if p >= 0 and int(t.prior_kind[p]) != PRIOR_NONE:
                text += "  p=%.4f" % float(t.prior[p][int(t.move[i])])
            st = int(t.status[i])
            if st >= 0:
                text += "  " + ("x wins", "draw", "o wins")[st]
            lines.append(text)
            first, n = int(t.first_child[i]), int(t.n_children[i])
            stack.extend(range(first + n - 1, first - 1, -1))
        return "\n".join(lines)
