"""CPU reference of vame_partition (test infrastructure): a plain Python / numpy
restatement of the decision rule of DESIGN.md section 12, by memoised
recursion per CTU.  Geometry comes from vame.hostlogic.geometry (the product's
candidate tables); nothing here shares code with the kernel.

Rule.  A node is a CTU-relative rectangle (x, y, w, h), w, h in {16, 32, 64,
128}, x, y multiples of 16, inside the CTU.  At frame position (X, Y):
  outside  X >= W or Y >= H: value 0, nothing emitted
  hole     a 16x16 node that crosses the frame edge: value 0
  leaf     only a node wholly in the frame that is a candidate CU of a PRED in
           the mask: min of cost[r][m][row] over r (outer), m = 2-CP, 3-CP
           (inner), first minimum
  split    penalty + sum of the children's values, infeasible if a child is;
           BT-H, BT-V, TT-H, TT-V in this order, TT only with a HALF PRED
  value    the first minimum over leaf and the splits, under strict <
"""
from __future__ import annotations

import functools

import numpy as np

from vame.hostlogic import geometry

CTU = 128
SIZES = (16, 32, 64, 128)
PER = (201, 284)
SPLIT_NAMES = ("BT_H", "BT_V", "TT_H", "TT_V")
LEAF, OUTSIDE, HOLE = -1, -2, -3  # decisions besides the split kinds 0..3


@functools.lru_cache(maxsize=None)
def candidates():
    """{(x, y, w, h): (align, offset)} of the 485 candidate CUs of a CTU."""
    out = {}
    for align in (0, 1):
        for w, h, xs, ys, stride in geometry(align):
            for k, (x, y) in enumerate(zip(xs.tolist(), ys.tolist())):
                key = (x, y, w, h)
                assert key not in out, f"{key} is a candidate twice"
                out[key] = (align, stride + k)
    assert len(out) == 485
    return out


def slot(x, y, w, h):
    lw, lh = SIZES.index(w), SIZES.index(h)
    return ((lh * 4 + lw) * 8 + y // 16) * 8 + x // 16


def node_table():
    """The map vame_partition_table returns: int32[1024]."""
    t = np.full(1024, -1, np.int32)
    for (x, y, w, h), (align, off) in candidates().items():
        if x % 16 == 0 and y % 16 == 0:
            t[slot(x, y, w, h)] = align * 512 + off
    return t


def children(x, y, w, h, kind):
    """The children of a split, top to bottom / left to right, or None."""
    if kind == 0:
        return [(x, y, w, h // 2), (x, y + h // 2, w, h // 2)] if h >= 32 else None
    if kind == 1:
        return [(x, y, w // 2, h), (x + w // 2, y, w // 2, h)] if w >= 32 else None
    if kind == 2:
        return [(x, y, w, h // 4), (x, y + h // 4, w, h // 2), (x, y + 3 * h // 4, w, h // 4)] if h >= 64 else None
    return [(x, y, w // 4, h), (x + w // 4, y, w // 2, h), (x + 3 * w // 4, y, w // 4, h)] if w >= 64 else None


@functools.lru_cache(maxsize=None)
def reachable(tt: bool = True):
    """The nodes the splits reach from the 128x128 root (frame ignored)."""
    seen, todo = set(), [(0, 0, CTU, CTU)]
    while todo:
        n = todo.pop()
        if n in seen:
            continue
        seen.add(n)
        for kind in range(4 if tt else 2):
            todo += children(*n, kind) or []
    return seen


def leaf_candidates():
    """The candidates that can be leaves: the reachable nodes among them."""
    return {n: candidates()[n] for n in reachable() if n in candidates()}


def never_leaf_groups():
    """[(w, h, group)] of the half-aligned groups none of whose CUs is a node."""
    can = leaf_candidates()
    return [(w, h, g) for g, (w, h, xs, ys, _) in enumerate(geometry(1))
            if not any((x, y, w, h) in can for x, y in zip(xs.tolist(), ys.tolist()))]


class Partition:
    """The decision for one POC.  cost: {(refIdx, PRED): int64[nCtus*per]};
    cpmv: the same keys, [n, 6] or [n, 7] (last 6 columns LTx .. LBy)."""

    def __init__(self, W, H, cost, cpmv, nrefs, mask, penalty=0):
        assert mask & 3 and not mask & ~15 and 1 <= nrefs <= 4
        self.W, self.H, self.nrefs, self.mask, self.penalty = W, H, nrefs, mask, int(penalty)
        self.cols = (W + CTU - 1) // CTU
        self.n_ctus = self.cols * ((H + CTU - 1) // CTU)
        self.cpmv = cpmv
        self.tt = bool(mask & 12)
        # leaf minima per alignment: candidates in (r outer, m inner) order, first minimum
        self.leaf_cost, self.leaf_sel = {}, {}
        for align in (0, 1):
            order = [(r, m) for r in range(nrefs) for m in (0, 1) if (mask >> (2 * align + m)) & 1]
            if not order:
                continue
            stack = np.stack([np.asarray(cost[(r, 2 * align + m)], np.int64).reshape(self.n_ctus, PER[align])
                              for r, m in order])
            first = np.argmin(stack, axis=0)  # the first occurrence of the minimum
            self.leaf_cost[align] = np.take_along_axis(stack, first[None], 0)[0]
            self.leaf_sel[align] = np.array(order, np.int64)[first]  # [nCtus, per, 2]

    # ---- one CTU
    def solve_ctu(self, ctu):
        """value(node) -> (value or None, decision) memoised over the CTU."""
        X0, Y0 = (ctu % self.cols) * CTU, (ctu // self.cols) * CTU
        cand = candidates()

        @functools.lru_cache(maxsize=None)
        def value(x, y, w, h):
            X, Y = X0 + x, Y0 + y
            if X >= self.W or Y >= self.H:
                return 0, OUTSIDE
            if w == 16 and h == 16 and (X + 16 > self.W or Y + 16 > self.H):
                return 0, HOLE
            best, dec = None, None
            if X + w <= self.W and Y + h <= self.H and (x, y, w, h) in cand:
                align, off = cand[(x, y, w, h)]
                if align in self.leaf_cost:
                    best, dec = int(self.leaf_cost[align][ctu, off]), LEAF
            for kind in range(4 if self.tt else 2):
                ch = children(x, y, w, h, kind)
                if ch is None:
                    continue
                vals = [value(*c)[0] for c in ch]
                if any(v is None for v in vals):
                    continue
                v = self.penalty + sum(vals)
                if best is None or v < best:
                    best, dec = v, kind
            return best, dec

        return value

    def leaves_of_ctu(self, ctu):
        """(root value, [leaf nodes in output order], holes, [splits per kind])."""
        value = self.solve_ctu(ctu)
        root, _ = value(0, 0, CTU, CTU)
        assert root is not None, "the aligned 16x16 candidates tile everything in the frame"
        leaves, holes, splits = [], 0, [0, 0, 0, 0]
        todo = [(0, 0, CTU, CTU)]
        while todo:
            n = todo.pop()
            _, dec = value(*n)
            if dec == LEAF:
                leaves.append(n)
            elif dec == HOLE:
                holes += 1
            elif dec is not None and dec >= 0:
                splits[dec] += 1
                todo += children(*n, dec)
        leaves.sort(key=lambda n: (n[1], n[0]))
        return root, leaves, holes, splits

    # ---- the frame
    def run(self):
        cus, rows, info, costs, kinds = [], [], [], [], np.zeros(4, np.int64)
        block_cu = np.full(self.n_ctus * 64, -1, np.int32)
        leaf_costs = []
        cand = candidates()
        for ctu in range(self.n_ctus):
            root, leaves, holes, splits = self.leaves_of_ctu(ctu)
            X0, Y0 = (ctu % self.cols) * CTU, (ctu // self.cols) * CTU
            info.append((len(cus), len(leaves), holes, sum(splits)))
            costs.append(root)
            kinds += splits
            for x, y, w, h in leaves:
                align, off = cand[(x, y, w, h)]
                r, m = (int(v) for v in self.leaf_sel[align][ctu, off])
                row = ctu * PER[align] + off
                cp = np.asarray(self.cpmv[(r, 2 * align + m)][row])[-6:]
                for by in range(y // 16, (y + h) // 16):
                    for bx in range(x // 16, (x + w) // 16):
                        assert block_cu[ctu * 64 + by * 8 + bx] == -1, "leaves overlap"
                        block_cu[ctu * 64 + by * 8 + bx] = len(cus)
                cus.append([X0 + x, Y0 + y, w, h, r, 2 + m] + [int(v) for v in cp])
                rows.append(row)
                leaf_costs.append(int(self.leaf_cost[align][ctu, off]))
        return {"cus": np.array(cus, np.int32).reshape(-1, 12), "rows": np.array(rows, np.int32), "ncus": len(cus),
                "ctu_info": np.array(info, np.int32).reshape(-1, 4), "ctu_cost": np.array(costs, np.int64),
                "block_cu": block_cu, "splits": kinds, "leaf_cost": np.array(leaf_costs, np.int64)}


def partition(W, H, cost, cpmv, nrefs, mask, penalty=0):
    return Partition(W, H, cost, cpmv, nrefs, mask, penalty).run()


def from_goldens(zs, mask, penalty=0):
    """The decision on golden fixtures (one per refIdx, sharing `cur`)."""
    names = ("FULL_2CP", "FULL_3CP", "HALF_2CP", "HALF_3CP")
    cost = {(r, m): z[n + "_cost"] for r, z in enumerate(zs) for m, n in enumerate(names) if (mask >> m) & 1}
    cpmv = {(r, m): z[n + "_cpmv"] for r, z in enumerate(zs) for m, n in enumerate(names) if (mask >> m) & 1}
    return partition(int(zs[0]["W"]), int(zs[0]["H"]), cost, cpmv, len(zs), mask, penalty)


def synthetic(W, H, nrefs, seed, ties=False):
    """Cost and CPMV arrays with no search run, every PRED of every refIdx:
    cost = area * U(0.5, 1.5), or the tie-heavy (area / 256) * randint(0, 3);
    small CPMVs that are valid everywhere."""
    rng = np.random.default_rng(seed)
    n_ctus = ((W + CTU - 1) // CTU) * ((H + CTU - 1) // CTU)
    cost, cpmv = {}, {}
    for r in range(nrefs):
        for m in range(4):
            align = m >> 1
            area = np.concatenate([np.full(len(xs), w * h, np.int64) for w, h, xs, _, _ in geometry(align)])
            assert len(area) == PER[align]
            area = np.tile(area, n_ctus)
            if ties:
                cost[(r, m)] = (area // 256) * rng.integers(0, 3, len(area))
            else:
                cost[(r, m)] = (area * rng.uniform(0.5, 1.5, len(area))).astype(np.int64)
            cp = rng.integers(-64, 65, (len(area), 7)).astype(np.int32)
            cp[:, 0] = 2 + (m & 1)
            cpmv[(r, m)] = cp
    return cost, cpmv
