"""Affine bi-prediction, host side: the numpy restatement (tests/bipred_ref.py)
against the oracle's uni prediction, the bi sample's identity, vame.bipred's
selection code and descriptors on CPU tensors, and the bi partition reference
against partition_ref and an exhaustive enumeration.  No device work."""
import functools
import itertools

import numpy as np
import pytest
import torch

import bipred_ref as B
import mc_ref
import oracle_py as O
import partition_ref as R


def frame(W=64, H=48, seed=0):
    return np.random.default_rng(seed).integers(0, 1024, (H, W)).astype(np.uint16)


def oracle_block(ref, x0, y0, mvx, mvy):
    H, W = ref.shape
    out = np.zeros(16, np.int32)
    O.lib().vame_oracle_predict_4x4(O.ptr(ref), W, H, int(x0), int(y0), int(mvx), int(mvy), O.ptr(out))
    return out.reshape(4, 4)


def test_uni_path_equals_the_oracle_for_every_phase():
    """All 256 (fx, fy) phases, inside the frame and with the window crossing
    each frame edge and corner."""
    ref = frame()
    H, W = ref.shape
    spots = [(24, 20, 0, 0)]                                            # inside
    spots += [(0, 20, -9, 0), (W - 4, 20, 9, 0), (24, 0, 0, -9), (24, H - 4, 0, 9)]          # each edge
    spots += [(0, 0, -7, -7), (W - 4, 0, 7, -7), (0, H - 4, -7, 7), (W - 4, H - 4, 7, 7)]    # each corner
    spots += [(0, 0, -140, -140), (W - 4, H - 4, 200, 200)]             # wholly outside: all clamped
    x0, y0, mvx, mvy = [], [], [], []
    for x, y, ix, iy in spots:
        for fx in range(16):
            for fy in range(16):
                x0.append(x), y0.append(y), mvx.append(ix * 16 + fx), mvy.append(iy * 16 + fy)
    got = B.uni_sample(B.acc_blocks(ref, x0, y0, mvx, mvy))
    assert got.shape == (len(spots) * 256, 4, 4)
    for k in range(len(x0)):
        np.testing.assert_array_equal(got[k], oracle_block(ref, x0[k], y0[k], mvx[k], mvy[k]), err_msg=str(k))


def test_cu_prediction_and_cost_equal_mc_ref():
    ref, cur = frame(128, 64, 1), frame(128, 64, 2)
    for d in ([16, 0, 64, 32, 0, 3, 5, -7, 30, 4, -12, 9], [96, 48, 32, 16, 0, 2, -300, 250, -280, 240, 0, 0],
              [0, 0, 16, 16, 0, 3, 0, 0, 4000, 0, 0, 4000]):        # the last one: spread
        want, wcost, spread = mc_ref.predict_cu(ref, cur, d[0], d[1], d[2], d[3], d[5], d[6:], 17.5)
        got, cost = B.predict_bicu([ref], cur, d + [-1] + [0] * 7, 17.5)
        np.testing.assert_array_equal(got, want)
        assert cost == wcost
    assert spread


def test_identical_hypotheses_give_the_uni_sample():
    ref = frame(64, 64, 3)
    acc, _ = B.acc_cu(ref, 16, 16, 32, 32, 3, [37, -21, 45, -30, 20, 11])
    np.testing.assert_array_equal(B.bi_sample(acc, acc), B.uni_sample(acc))
    # and over the accumulator's whole range, negative values and the clip included
    a = np.arange(-(1 << 21), 1 << 21, 7, dtype=np.int64)
    np.testing.assert_array_equal(B.bi_sample(a, a), B.uni_sample(a))
    # a bi descriptor with ref0 == ref1 and equal CPMVs is the uni prediction; its cost carries two rates
    d = [16, 16, 32, 32, 0, 3, 37, -21, 45, -30, 20, 11]
    cur = frame(64, 64, 4)
    uni, ucost = B.predict_bicu([ref], cur, d + [-1] + [0] * 7, 10.0)
    bi, bcost = B.predict_bicu([ref], cur, d + d[4:], 10.0)
    np.testing.assert_array_equal(bi, uni)
    bits = B.bits_of(3, d[6:])
    assert bcost - ucost == B.rate(2 * bits + 4, 10.0) - B.rate(bits + 2, 10.0)
    # two different hypotheses: where neither uni sample is clipped, the once-rounded average lies within
    # one of their mean (a clipped uni sample lost what the unclipped accumulator still carries)
    acc2, _ = B.acc_cu(ref, 16, 16, 32, 32, 2, [-40, 8, -44, 2, 0, 0])
    u0, u1, bi = B.uni_sample(acc), B.uni_sample(acc2), B.bi_sample(acc, acc2)
    free = (u0 > 0) & (u0 < 1023) & (u1 > 0) & (u1 < 1023)
    assert free.sum() > 500 and np.abs(bi - (u0 + u1) / 2)[free].max() <= 1 and (bi != u0).any()


def test_sel_code_and_pairs_round_trip():
    from vame import bipred as V
    assert V.pairs(1) == [] and V.pairs(2) == [(0, 1)] and V.pairs(3) == [(0, 1), (0, 2), (1, 2)]
    assert V.pairs(4) == list(B.PAIRS)
    with pytest.raises(ValueError):
        V.pairs(5)
    seen = set()
    for r0, m0, r1, m1 in itertools.product(range(4), range(2), range(4), range(2)):
        s = V.encode_sel(r0, m0, r1, m1)
        assert 0 <= s < 64 and V.decode_sel(s) == (r0, m0, r1, m1)
        seen.add(s)
    assert len(seen) == 64
    t = torch.arange(64, dtype=torch.int32)
    assert torch.equal(V.encode_sel(*V.decode_sel(t)), t)
    assert len(V.BICU_FIELDS) == 20 and V.BICU_FIELDS[4] == "ref0" and V.BICU_FIELDS[12] == "ref1"
    out = V.alloc(3, "cpu")
    assert set(out) == set(V.KEYS) and out["cus"].shape == (192, 20) and out["sel"].shape == (192,)


def test_bicus_from_sel_on_cpu_tensors():
    from vame import bipred as V
    from vame.mc import candidate_geometry
    W, H = 416, 240
    cost, cpmv = R.synthetic(W, H, 3, 11)
    names = ("FULL_2CP", "FULL_3CP", "HALF_2CP", "HALF_3CP")
    result = {(r, names[m]): (torch.from_numpy(cost[(r, m)]), torch.from_numpy(cpmv[(r, m)]))
              for (r, m) in cost}
    for align in (0, 1):
        n = 8 * B.PER[align]
        rng = np.random.default_rng(align)
        r0 = rng.integers(0, 2, n)
        r1 = r0 + 1 + rng.integers(0, 2, n) * (r0 == 0)
        m0, m1 = rng.integers(0, 2, n), rng.integers(0, 2, n)
        sel = torch.from_numpy(V.encode_sel(r0, m0, r1, m1).astype(np.int32))
        sel[5] = -1
        rows = torch.tensor([0, 5, 17, 200, n - 1, 17])
        cus = V.bicus_from_sel(W, H, align, result, sel, rows)
        assert cus.shape == (6, 20) and cus.dtype == torch.int32 and cus.device.type == "cpu"
        geo = {int(r): k for k, r in enumerate(candidate_geometry(W, H, align)[0])}
        g = candidate_geometry(W, H, align)
        for i, row in enumerate(rows.tolist()):
            k = geo[row]
            assert cus[i, :4].tolist() == [int(g[j][k]) for j in (1, 2, 3, 4)]
            if row == 5:
                assert cus[i, 4] == -1 and cus[i, 12] == -1
                continue
            want = [r0[row], 2 + m0[row]] + cpmv[(r0[row], 2 * align + m0[row])][row][-6:].tolist() + \
                   [r1[row], 2 + m1[row]] + cpmv[(r1[row], 2 * align + m1[row])][row][-6:].tolist()
            assert cus[i, 4:].tolist() == [int(v) for v in want]
    with pytest.raises(ValueError):
        V.bicus_from_sel(W, H, 0, result, sel, rows)  # the half-aligned array for the aligned candidates


def synthetic_bi(W, H, nrefs, seed, cost, scale=(0.6, 1.4)):
    """bi arrays with no prediction run: bi_cost = U(scale) * the row's uni
    minimum, a random valid sel; rows of CUs leaving the frame INF / -1."""
    rng = np.random.default_rng(seed)
    bi = {}
    for align in (0, 1):
        cands = B.frame_candidates(W, H, align)
        uni = np.min([cost[(r, 2 * align + m)] for r in range(nrefs) for m in (0, 1)], axis=0)
        bc = (uni * rng.uniform(*scale, len(uni))).astype(np.int64)
        r0 = rng.integers(0, nrefs - 1, len(uni))
        sel = (r0 + 4 * rng.integers(0, 2, len(uni)) + 8 * (r0 + 1) + 32 * rng.integers(0, 2, len(uni))).astype(np.int32)
        out = np.array([x + w > W or y + h > H for _, x, y, w, h in cands])
        bc[out], sel[out] = B.INF, -1
        bi[align] = (bc, sel)
    return bi


@pytest.mark.parametrize("seed", [1, 2])
def test_huge_bi_penalty_is_the_uni_partition(seed):
    W, H = 416, 240
    cost, cpmv = R.synthetic(W, H, 3, seed)
    bi = synthetic_bi(W, H, 3, seed, cost)
    want = R.partition(W, H, cost, cpmv, 3, 15, 70)
    got = B.partition_bi(W, H, cost, cpmv, 3, 15, 70, bi, 1 << 40)
    for k in want:
        np.testing.assert_array_equal(got[k][:, :12] if k == "cus" else got[k], want[k], err_msg=k)
    assert (got["sel"] == -1).all() and (got["cus"][:, 12] == -1).all() and (got["cus"][:, 13:] == 0).all()
    # and with penalty 0 bi leaves appear, each with its two hypotheses
    got = B.partition_bi(W, H, cost, cpmv, 3, 15, 70, bi, 0)
    nb = int((got["sel"] >= 0).sum())
    assert 0 < nb < got["ncus"]
    cand = R.candidates()
    for d, s, row in zip(got["cus"], got["sel"], got["rows"]):
        align = cand[(d[0] % 128, d[1] % 128, d[2], d[3])][0]
        if s < 0:
            assert d[12] == -1 and (d[13:] == 0).all()
            continue
        assert bi[align][1][row] == s
        r0, m0, r1, m1 = s & 3, (s >> 2) & 1, (s >> 3) & 3, (s >> 5) & 1
        assert (d[4], d[5], d[12], d[13]) == (r0, 2 + m0, r1, 2 + m1)
        np.testing.assert_array_equal(d[6:12], cpmv[(r0, 2 * align + m0)][row][-6:])
        np.testing.assert_array_equal(d[14:], cpmv[(r1, 2 * align + m1)][row][-6:])
    for ctu, (first, count, _, splits) in enumerate(got["ctu_info"]):
        assert got["ctu_cost"][ctu] == got["leaf_cost"][first:first + count].sum() + 70 * int(splits)


def tilings(node, leaf):
    out = [] if leaf(node) is None else [(leaf(node), 0)]
    for kind in range(4):
        ch = R.children(*node, kind)
        if ch is None:
            continue
        for combo in itertools.product(*(tilings(c, leaf) for c in ch)):
            out.append((sum(c[0] for c in combo), 1 + sum(c[1] for c in combo)))
    return out


@pytest.mark.parametrize("penalty,bi_penalty", [(0, 0), (300, 0), (0, 2000), (5000, 700)])
def test_exhaustive_tilings_with_bi_leaves(penalty, bi_penalty):
    """One 64x64 quadrant (ternary splits and half-aligned leaves too): the
    cheapest of all tilings, each leaf at min(uni, bi + bi_penalty), equals
    the reference's value."""
    W, H, ctu = 416, 240, 1
    cost, cpmv = R.synthetic(W, H, 2, 5)
    bi = synthetic_bi(W, H, 2, 5, cost)
    part = B.PartitionBi(W, H, cost, cpmv, 2, 15, penalty, bi, bi_penalty)
    cand = R.candidates()

    @functools.lru_cache(maxsize=None)
    def leaf(n):
        if n not in cand:
            return None
        align, off = cand[n]
        row = ctu * R.PER[align] + off
        v = min(int(cost[(r, 2 * align + m)][row]) for r in (0, 1) for m in (0, 1))
        if bi[align][1][row] >= 0:
            v = min(v, int(bi[align][0][row]) + bi_penalty)
        return v
    node = (64, 0, 64, 64)
    every = tilings(node, leaf)
    assert len(every) > 10000
    assert part.solve_ctu(ctu)(*node)[0] == min(c + penalty * n for c, n in every)
    # with a free bi leaf the bi term matters here: the uni-only value is larger
    uni = R.Partition(W, H, cost, cpmv, 2, 15, penalty)
    assert bi_penalty > 0 or part.solve_ctu(ctu)(*node)[0] < uni.solve_ctu(ctu)(*node)[0]
