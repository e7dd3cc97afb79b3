"""Whole reference trees of tests/golden/search_trees.npz (written by tests/golden/gen_tree_golden.py) as arrays and tables."""
import numpy as np

from conftest import load_npz


class TreeCase:
    def __init__(self, npz, name, kind):
        self.name, self.kind = name, kind
        g = lambda k: npz["%s__%s" % (name, k)]  # noqa: E731
        self.c0, self.c1 = int(g("board")[0]), int(g("board")[1])
        c = g("config")
        self.config = dict(simulations=int(c[0]), pb_c_base=int(c[1]), pb_c_init=float(c[2]), root_dirichlet_alpha=float(c[3]),
                           root_exploration_fraction=float(c[4]), num_sampling_moves=int(c[5]))
        self.noise = g("noise") if "%s__noise" % name in npz.files else None
        self.parent, self.move, self.visits = g("parent"), g("move"), g("visits")
        self.value_sum, self.status, self.prior_kind = g("value_sum"), g("status"), g("prior_kind")
        self.prior = np.zeros((len(self.parent), 7), dtype=np.float64)   # float32 priors widened exactly
        self.prior[self.prior_kind == 1] = g("prior32").astype(np.float64)
        self.prior[self.prior_kind == 2] = g("prior64")

    def __len__(self):
        return len(self.parent)

    def table(self):
        from connect4_amd.tree import TreeTable
        return TreeTable.from_arrays(self.c0, self.c1, self.parent, self.move, self.visits, self.value_sum, self.status,
                                     self.prior, self.prior_kind)


def load_tree_cases():
    npz = load_npz("search_trees.npz")
    return [TreeCase(npz, str(n), str(k)) for n, k in zip(npz["names"], npz["kinds"])]
