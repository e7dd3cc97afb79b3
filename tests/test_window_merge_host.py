"""replay.merge_host -- the rule by which ReplayWindow.merged (c4_window_merge_dev) merges identical positions -- against
a grouping written here independently: members are grouped by the set {position, mirror image}, their priors are taken
in the FIRST member's column order (a member that is the first's mirror image counts reversed), everything is summed as
Python integers rne(x 2^40) of exact Fractions, and the mean is the correctly rounded float64 quotient, rounded to
float32.  That needs no key, and no notion of which image is canonical: the rule's outputs must not depend on either.
Plus hand-made cases, the bad rows, and the no-CPU error of ReplayWindow.merged.  No GPU."""
import random
from fractions import Fraction

import numpy as np
import pytest

from connect4_amd import replay
from connect4_amd.board import Board
from connect4_amd.replay import merge_host

ONE = 1 << 40


def flip(p):
    return Board.flip_color(p)


def stones(moves):
    b = Board()
    for m in moves:
        b.make_move(m)
    return b.color[0], b.color[1]


def rows(positions, targets, policy):
    return (np.array(positions, dtype=np.uint64).reshape(-1, 2).view(np.int64), np.asarray(targets, dtype=np.float32),
            np.asarray(policy, dtype=np.float32).reshape(-1, 7))


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int32) if x.dtype == np.float32 else x


def same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def brute_force(boards, targets, policy, mirror=True):
    b = boards.view(np.uint64).tolist()
    groups, order = {}, []
    for i, (c0, c1) in enumerate(b):
        ident = frozenset([(c0, c1), (flip(c0), flip(c1))]) if mirror else (c0, c1)
        if ident not in groups:
            groups[ident] = []
            order.append(ident)
        groups[ident].append(i)
    out = []
    for ident in order:
        members = groups[ident]
        first = members[0]
        if len(members) == 1:
            out.append((boards[first], targets[first], policy[first], 1))
            continue
        sums = [0] * 8
        for i in members:
            p = [Fraction(float(x)) for x in policy[i]]
            if tuple(b[i]) != tuple(b[first]):
                p.reverse()
            for k, x in enumerate([Fraction(float(targets[i]))] + p):
                sums[k] += round(x * ONE)            # (round() of a Fraction: to nearest, ties to even)
        assert max(sums) < 1 << 53                   # so float64(sum) is the sum, and the quotient below the rule's
        mean = [np.float32(float(Fraction(s, len(members) * ONE))) for s in sums]
        out.append((boards[first], mean[0], mean[1:], len(members)))
    return (np.array([o[0] for o in out], dtype=np.int64).reshape(-1, 2), np.array([o[1] for o in out], dtype=np.float32),
            np.array([o[2] for o in out], dtype=np.float32).reshape(-1, 7), np.array([o[3] for o in out], dtype=np.int32))


def random_rows(n, seed, max_plies=6):
    rng = random.Random(seed)
    nrng = np.random.RandomState(seed)
    pos = []
    while len(pos) < n:
        b = Board()
        for _ in range(rng.randint(0, max_plies)):
            b.make_move(rng.choice(sorted(b.valid_moves)))
        pos.append((b.color[0], b.color[1]))
    return rows(pos, nrng.randint(0, 3, n) * 0.5, nrng.rand(n, 7))


@pytest.mark.parametrize("mirror", [True, False])
def test_merge_host_is_the_brute_force_grouping(mirror):
    data = random_rows(700, 1)
    got = merge_host(*data, mirror=mirror)
    assert same(got, brute_force(*data, mirror=mirror))
    assert int(got[3].sum()) == 700 and 1 < len(got[3]) < 700 and int(got[3].max()) > 2
    if mirror:
        assert len(got[3]) < len(merge_host(*data, mirror=False)[3])
    # torch tensors are taken as well
    import torch
    assert same(merge_host(*[torch.from_numpy(x) for x in data], mirror=mirror), got)


def test_mirror_pair_whose_first_member_is_reversed():
    right, left = stones([6]), stones([0])
    assert replay._position_key(*right) > replay._position_key(*left)          # the first member is the reversed one
    pa, pb = np.arange(7) / 8.0, np.array([0.5, 0.25, 0, 0, 0, 0.125, 1.0])
    b, t, p, c = merge_host(*rows([right, left], [1.0, 0.5], [pa, pb]))
    assert c.tolist() == [2] and b.view(np.uint64).tolist() == [list(right)]    # the board as stored, not canonicalised
    assert t.tolist() == [0.75]
    assert p[0].tolist() == ((pa + pb[::-1]) / 2).tolist()                      # (exact: dyadic inputs) in the first member's columns
    # the other way round the same sums come out in the other column order
    b2, t2, p2, _ = merge_host(*rows([left, right], [0.5, 1.0], [pb, pa]))
    assert b2.view(np.uint64).tolist() == [list(left)] and p2[0].tolist() == p[0][::-1].tolist() and t2.tolist() == [0.75]


def test_self_mirror_position_is_not_symmetrised():
    mid = stones([3])
    assert (flip(mid[0]), flip(mid[1])) == mid
    pa, pb = np.arange(7) / 8.0, np.array([0, 0, 0, 0, 0, 0, 1.0])
    _, _, p, c = merge_host(*rows([mid, mid], [0, 0], [pa, pb]))
    assert c.tolist() == [2] and p[0].tolist() == ((pa + pb) / 2).tolist() and p[0].tolist() != p[0][::-1].tolist()


def test_mirror_false_keeps_the_pair_apart():
    data = rows([stones([6]), stones([0])], [1.0, 0.5], [np.arange(7) / 8.0] * 2)
    out = merge_host(*data, mirror=False)
    assert out[3].tolist() == [1, 1] and same(out[:3], data)


def test_singletons_come_back_bit_for_bit():
    tiny = np.float32(1e-7)
    assert 0 < tiny < 2.0 ** -17 and float(tiny) * ONE != round(float(tiny) * ONE)      # no round trip through 2^-40 would keep it
    data = rows([stones([]), stones([1]), stones([1, 2])], [np.float32(1) / np.float32(3), 0.0, -0.0],
                [[tiny, 0.1, 0.2, 0.3, 0.15, 0.05, 1.0], np.full(7, 1 / 7), [np.float32(2.0 ** -140)] * 7])
    out = merge_host(*data)
    assert out[3].tolist() == [1, 1, 1] and same(out[:3], data)
    # a window without duplicates merges to itself
    distinct = rows([stones([3] * k) for k in range(6)], [0.5] * 6, np.random.RandomState(0).rand(6, 7))
    assert same(merge_host(*distinct)[:3], distinct)


def test_order_is_first_occurrence_and_later_members_may_come_in_any_order():
    data = random_rows(400, 5, max_plies=3)
    ref = merge_host(*data)
    perm = within_group_permutation(data[0], 6)
    firsts = sorted(first_members(data[0]))
    assert all(perm[i] == i for i in firsts)
    assert ref[0].view(np.uint64).tolist() == [data[0].view(np.uint64)[i].tolist() for i in firsts]
    assert int((perm != np.arange(400)).sum()) > 100
    assert same(merge_host(*[x[perm] for x in data]), ref)


def group_members(boards):
    groups = {}
    for i, row in enumerate(boards.view(np.uint64).tolist()):
        groups.setdefault(frozenset([tuple(row), (flip(row[0]), flip(row[1]))]), []).append(i)
    return list(groups.values())


def first_members(boards):
    return {g[0] for g in group_members(boards)}


def within_group_permutation(boards, seed):
    """Rows permuted among the places of their own group's later members: every first member stays where it is."""
    rng = random.Random(seed)
    perm = np.arange(len(boards))
    for g in group_members(boards):
        later = g[1:]
        moved = list(later)
        rng.shuffle(moved)
        perm[later] = moved
    return perm


@pytest.mark.parametrize("kind", ["overlap", "floating", "sentinel", "bit63", "nan_target", "prior_1.5", "negative_prior", "inf_prior"])
def test_bad_rows_raise(kind):
    pos = [stones([]), stones([3, 3]), stones([2])]
    t, p = [0.5, 0.5, 0.5], np.full((3, 7), 0.125)
    if kind == "overlap":
        pos[1] = (pos[1][0] | pos[1][1], pos[1][1])
    elif kind == "floating":
        pos[1] = (1 << (7 * 3 + 2), 1 << (7 * 3))           # nothing at height 1 of the column
    elif kind == "sentinel":
        pos[1] = (0x15 | 1 << 6, 0x2a)                        # column 0 full and its seventh bit set
    elif kind == "bit63":
        pos[1] = (pos[1][0] | 1 << 63, pos[1][1])
    elif kind == "nan_target":
        t[1] = float("nan")
    elif kind == "prior_1.5":
        p[1, 4] = 1.5
    elif kind == "negative_prior":
        p[1, 0] = -1e-30
    elif kind == "inf_prior":
        p[1, 6] = float("inf")
    with pytest.raises(ValueError, match="1 of 3 rows"):
        merge_host(*rows(pos, t, p))
    pos[1], t[1], p[1] = stones([3, 3]), 0.5, 0.125
    assert merge_host(*rows(pos, t, p))[3].tolist() == [1, 1, 1]


def test_merged_needs_a_gpu():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        replay.ReplayWindow(device="cpu").merged()
