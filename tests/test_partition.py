"""The CU partition decision, host side: vame_partition_table against the
reference's candidate map, the invariants of the reference itself
(tests/partition_ref.py) on every golden fixture, and the recursion against an
exhaustive enumeration of tilings.  No device work."""
import functools
import glob
import itertools
import os

import numpy as np
import pytest

import partition_ref as R

GOLD = os.path.join(os.path.dirname(__file__), "golden")
GOLDENS = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLD, "s416_*.npz"))) + ["s832_qp37_poc1"]


@functools.lru_cache(maxsize=None)
def load(name):
    return dict(np.load(os.path.join(GOLD, name + ".npz")))


def test_partition_table_equals_reference_map():
    from vame.partition import table
    t = table()
    assert t.dtype == np.int32 and t.shape == (1024,)
    np.testing.assert_array_equal(t, R.node_table())
    # every entry names its own rectangle
    cand = {v: k for k, v in R.candidates().items()}
    for s in np.nonzero(t >= 0)[0]:
        x, y, w, h = cand[(int(t[s]) >> 9, int(t[s]) & 511)]
        assert R.slot(x, y, w, h) == s


def test_reachable_nodes_and_leaf_candidates():
    """361 nodes are reachable from the root, 261 of the 485 candidates can be
    leaves; the candidates at a multiple of 16 are exactly those."""
    assert len(R.reachable()) == 361
    can = R.leaf_candidates()
    assert len(can) == 261
    assert sum(1 for a, _ in can.values() if a == 0) == 201  # every aligned candidate
    assert int((R.node_table() >= 0).sum()) == 261
    # the half-aligned groups that never take part: every CU at an odd multiple of 8
    never = R.never_leaf_groups()
    assert [g for _, _, g in never] == [2, 3, 4, 5, 8, 9, 11, 12, 14, 15, 16, 17, 19, 20, 21, 22, 23]
    # without the ternary splits only the aligned candidates are reachable
    assert sum(1 for n in R.reachable(False) if n in R.candidates()) == 201


def check_invariants(o, part: R.Partition):
    W, H = part.W, part.H
    # every fully in-frame 16x16 block is covered exactly once, no other block at all
    cover = np.zeros((H // 16 + 8, W // 16 + 8), np.int32)
    for x, y, w, h in o["cus"][:, :4]:
        assert x + w <= W and y + h <= H
        cover[y // 16:(y + h) // 16, x // 16:(x + w) // 16] += 1
    assert (cover[:H // 16, :W // 16] == 1).all() and cover.sum() == (H // 16) * (W // 16)
    # block_cu names the covering leaf
    for ctu in range(part.n_ctus):
        X0, Y0 = (ctu % part.cols) * 128, (ctu // part.cols) * 128
        for b in range(64):
            bx, by = X0 + (b & 7) * 16, Y0 + (b >> 3) * 16
            i = o["block_cu"][ctu * 64 + b]
            if bx + 16 <= W and by + 16 <= H:
                x, y, w, h = o["cus"][i, :4]
                assert x <= bx < x + w and y <= by < y + h
            else:
                assert i == -1
    # ctu_cost = sum of the leaf costs + penalty * splits
    info = o["ctu_info"]
    for ctu in range(part.n_ctus):
        first, count, _, splits = info[ctu]
        assert o["ctu_cost"][ctu] == o["leaf_cost"][first:first + count].sum() + part.penalty * int(splits)
    assert info[:, 1].sum() == o["ncus"] and (info[:, 0] == np.cumsum(info[:, 1]) - info[:, 1]).all()
    assert info[:, 3].sum() == o["splits"].sum()
    holes = (W // 16) * (-(-H // 16) - H // 16)
    assert info[:, 2].sum() == holes


def forced_splits(W, H):
    """The fewest splits a frame edge forces on each CTU: the cheapest tree by
    split count alone (unit cost per split, free leaves)."""
    ones = {}
    for m in range(4):
        n = ((W + 127) // 128) * ((H + 127) // 128) * R.PER[m >> 1]
        ones[(0, m)] = np.zeros(n, np.int64)
    part = R.Partition(W, H, ones, ones, 1, 15, 1)
    return np.array([part.solve_ctu(c)(0, 0, 128, 128)[0] for c in range(part.n_ctus)])


@pytest.mark.parametrize("name", GOLDENS)
def test_reference_invariants_on_goldens(name):
    z = load(name)
    W, H = int(z["W"]), int(z["H"])
    for mask in (1, 3, 15):
        for penalty in (0, 2000):
            cost = {(0, m): z[n + "_cost"] for m, n in enumerate(("FULL_2CP", "FULL_3CP", "HALF_2CP", "HALF_3CP"))}
            cpmv = {(0, m): z[n + "_cpmv"] for m, n in enumerate(("FULL_2CP", "FULL_3CP", "HALF_2CP", "HALF_3CP"))}
            part = R.Partition(W, H, cost, cpmv, 1, mask, penalty)
            check_invariants(part.run(), part)
    # a 2^40 penalty outweighs every cost: the split count is what the frame edge forces
    part = R.Partition(W, H, cost, cpmv, 1, 15, 1 << 40)
    o = part.run()
    check_invariants(o, part)
    assert max(int(c.max()) for c in cost.values()) * 64 < 1 << 40
    np.testing.assert_array_equal(o["ctu_info"][:, 3], forced_splits(W, H))


def test_split_penalty_leaf_counts():
    """288 / 275 / 23 leaves on s416_noise at penalties 0 / 2000 / 2^40."""
    z = load("s416_noise")
    assert [R.from_goldens([z], 15, p)["ncus"] for p in (0, 2000, 1 << 40)] == [288, 275, 23]


def tilings(node, leaf):
    """(sum of leaf costs, splits) of every tiling of a node by the splits
    whose leaves are all candidates -- enumerated, nothing minimised."""
    out = [] if leaf(node) is None else [(leaf(node), 0)]
    for kind in range(4):
        ch = R.children(*node, kind)
        if ch is None:
            continue
        for combo in itertools.product(*(tilings(c, leaf) for c in ch)):
            out.append((sum(c[0] for c in combo), 1 + sum(c[1] for c in combo)))
    return out


@pytest.mark.parametrize("penalty", [0, 300, 5000])
@pytest.mark.parametrize("node,count", [((0, 0, 32, 32), 9), ((96, 0, 32, 32), 9), ((96, 96, 32, 32), 9),
                                        ((64, 0, 64, 64), None)], ids=str)
def test_exhaustive_tilings_of_a_corner(node, count, penalty):
    """For 32x32 corners of one CTU (9 tilings each: the leaf and 2 x 4 binary
    trees) and one 64x64 quadrant (ternary splits and half-aligned leaves
    too), the cheapest of all tilings equals the recursion's value."""
    z = load("s416_noise")
    names = ("FULL_2CP", "FULL_3CP", "HALF_2CP", "HALF_3CP")
    cost = {(0, m): z[n + "_cost"] for m, n in enumerate(names)}
    part = R.Partition(416, 240, cost, cost, 1, 15, penalty)
    ctu = 1
    cand = R.candidates()

    @functools.lru_cache(maxsize=None)
    def leaf(n):
        if n not in cand:
            return None
        align, off = cand[n]
        return min(int(cost[(0, 2 * align + m)][ctu * R.PER[align] + off]) for m in (0, 1))
    every = tilings(node, leaf)
    if count is not None:
        assert len(every) == count
    else:
        assert len(every) > 10000
    assert part.solve_ctu(ctu)(*node)[0] == min(c + penalty * n for c, n in every)
