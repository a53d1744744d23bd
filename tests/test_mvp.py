"""Rates against a motion-vector predictor, host side:
the CPU reference tests/mvp_ref.py against the oracle and against the
references it extends, and the cases the GPU tests (tests/test_gpu_mvp.py) run,
with what they must exercise asserted on the reference alone."""
import functools

import numpy as np

import bipred_ref as B
import birefine_ref as F
import mvp_ref as R
import oracle_py as O
import seed_ref as S
from test_seed import sample

W, H = 416, 240
LAM = S.LAM
MV_MAX, MV_MIN = R.MV_MAX, R.MV_MIN
ZERO = list(R.ZERO)


# ------------------------------------------------------------------ the rule
def test_bits_p_with_a_zero_predictor_is_the_oracles_bits():
    rng = np.random.default_rng(171)
    cps = np.concatenate([rng.integers(MV_MIN, MV_MAX + 1, (1500, 6)), rng.integers(-600, 601, (1500, 6)),
                          rng.integers(-9, 10, (500, 6)), [[MV_MIN] * 6, [MV_MAX] * 6, [MV_MIN, MV_MAX] * 3,
                                                           [MV_MAX, MV_MIN] * 3, [0] * 6]])
    for cp in cps.tolist():
        for n in (2, 3):
            assert R.bits_p(cp, ZERO, n) == B.bits_of(n, cp), (cp, n)
    for v in list(range(-70, 71)) + [MV_MIN, MV_MAX, MV_MIN + 1, MV_MAX - 1]:
        assert R.q(v) == O.lib().vame_oracle_to_quarter(v)


def test_hand_checked_bits():
    seed = [-224, 112] * 3  # (-14, 7) samples: q = (-56, 28)
    assert [R.eg(-56), R.eg(28), R.eg(0)] == [13, 11, 1]
    assert R.bits_p(seed, ZERO, 2) + 2 == 28
    assert R.bits_p(seed, seed, 2) + 2 == 6 and R.bits_p(seed, seed, 3) + 2 == 8
    assert B.rate(28, LAM) == 2210 and B.rate(R.bits_p(ZERO, ZERO, 2) + 2, LAM) == 473
    # RT and LB are priced against the predictor's moved by the LT difference
    c, P = [40, -8, 48, -8, 40, 4], [32, 0, 36, 0, 32, 8]
    want = R.eg(10 - 8) + R.eg(-2 - 0) + R.eg(12 - R.q(36 + 8)) + R.eg(-2 - R.q(0 - 8)) + \
        R.eg(10 - R.q(32 + 8)) + R.eg(1 - R.q(8 - 8))
    assert R.bits_p(c, P, 3) == want and R.bits_p(c, P, 2) == want - R.eg(0) - R.eg(1)
    # the ends of the range: the composed predictor stays inside int32
    assert R.bits_p([MV_MAX] * 6, [MV_MIN, MV_MIN, MV_MAX, MV_MAX, MV_MAX, MV_MAX], 3) > 0


# ------------------------------------------------------------------ the cases of the GPU tests
@functools.lru_cache(maxsize=None)
def frames(nrefs=2):
    return S.shifted_camera(nrefs)


def near(mv, rng, spread):
    """A general affine predictor around the translational MV."""
    return (np.array(R.expand(mv)) + rng.integers(-spread, spread + 1, 6)).tolist()


@functools.lru_cache(maxsize=None)
def search_cases_p():
    """[(12-column descriptor, predictor [6])] on the shifted-camera pair:
    every size (so all three kernel classes) from its integer seed, 2-CP and the
    3-CP start derived from it, with general affine predictors near the seed,
    far from it, zero, and at the ends of the range; positions that are
    multiples of 4 only."""
    refs, cur = frames()
    rng = np.random.default_rng(1717)
    out = []
    for k, (row, x, y, w, h) in enumerate(sample(0, 12, salt=3)):
        r = k & 1
        mv, _ = S.seed_cu(refs[r], cur, x, y, w, h, 16, LAM)
        c2 = [mv[0], mv[1], mv[0], mv[1], 0, 0]
        cp = S.seed_3cp(c2, x, y, w, h, W, H) if k % 3 == 0 else c2
        out.append(([x, y, w, h, r, 3 if k % 3 == 0 else 2] + cp, near(mv, rng, 24 if k % 2 else 6)))
    out.append(([160, 96, 16, 16, 0, 2, -176, 96, -176, 96, 0, 0], [MV_MIN, MV_MAX, MV_MAX, MV_MIN, MV_MIN, MV_MAX]))
    out.append(([64, 64, 32, 32, 0, 3, -170, 100, -180, 90, -175, 99], ZERO))
    out.append(([20, 36, 16, 16, 1, 2, -170, 100, -172, 98, 0, 0], [-160, 90, -150, 80, 3, -3]))
    out.append(([100, 52, 32, 16, 0, 3, -180, 90, -176, 96, -170, 100], [-176, 96] * 3))
    out.append(([128, 0, 64, 64, 1, 2, -160, 80, -160, 80, 0, 0], [200, -300, 180, -280, 0, 0]))  # a far predictor
    return out


@functools.lru_cache(maxsize=None)
def bi_cases_p():
    """[(20-column descriptor, predictor of hypothesis 0, of hypothesis 1)]:
    bi descriptors of every kernel class with 2-CP and 3-CP hypotheses from the
    references' seeds, one with ref1 == ref0, and uni descriptors.  No two
    overlap, so one call predicts them all into one frame."""
    refs, cur = frames()
    rng = np.random.default_rng(1718)
    out = []
    geo = ((64, 64, 16, 16, 0, 1, 2, 2), (128, 32, 32, 32, 1, 0, 3, 2), (320, 64, 64, 16, 0, 1, 2, 3),
           (256, 128, 64, 64, 0, 1, 3, 3), (0, 0, 128, 64, 1, 0, 2, 2), (128, 64, 128, 128, 0, 1, 2, 3),
           (36, 148, 32, 64, 0, 0, 2, 2), (320, 16, 64, 32, 1, 1, 3, 2))
    for x, y, w, h, r0, r1, n0, n1 in geo:
        hyp = []
        for r, n in ((r0, n0), (r1, n1)):
            mv, _ = S.seed_cu(refs[r], cur, x, y, w, h, 16, LAM)
            c2 = [mv[0] + int(rng.integers(-6, 7)), mv[1] + int(rng.integers(-6, 7))] * 2 + [0, 0]
            hyp.append((mv, S.seed_3cp(c2, x, y, w, h, W, H) if n == 3 else c2))
        out.append(([x, y, w, h, r0, n0] + hyp[0][1] + [r1, n1] + hyp[1][1], near(hyp[0][0], rng, 10),
                    near(hyp[1][0], rng, 30)))
    out.append(([96, 96, 32, 32, 1, 3, -176, 96, -170, 90, -180, 100, -1, 0] + [0] * 6, [-170, 100, -172, 98, -168, 96], ZERO))
    out.append(([224, 32, 16, 16, 0, 2, -176, 96, -176, 96, 0, 0, -1, 9] + [7] * 6, [-176, 96] * 3, [1 << 20] * 6))
    return out


@functools.lru_cache(maxsize=None)
def search_reference_p(extra):
    refs, cur = frames()
    return [R.search_cu_p(refs[d[4]], cur, d[0], d[1], d[2], d[3], d[5], d[6:12], P, LAM, extra)
            for d, P in search_cases_p()]


@functools.lru_cache(maxsize=None)
def search_reference_zero():
    refs, cur = frames()
    return [S.search_cu(refs[d[4]], cur, d[0], d[1], d[2], d[3], d[5], d[6:12], LAM, 0) for d, _ in search_cases_p()]


@functools.lru_cache(maxsize=None)
def refine_reference_p():
    """Per bi case the trace [(descriptor, cost)] after 0, 1, 2 rounds."""
    refs, cur = frames()
    return [R.refine_bicu_p_trace(refs, cur, d, P0, P1, LAM, 2) for d, P0, P1 in bi_cases_p()]


@functools.lru_cache(maxsize=None)
def refine_reference_zero():
    refs, cur = frames()
    return [F.refine_bicu_trace(refs, cur, d, LAM, 2) for d, _, _ in bi_cases_p()]


# ---- rows for bipred_p and merged_p: three references, 2-CP winners from the seeds
@functools.lru_cache(maxsize=None)
def row_case():
    """Three references; for a few small in-frame FULL rows the 2-CP result of
    the search from zero (cost, CPMVs) per reference -- what the fused search
    leaves -- their seeds, and region-style predictors: the seed for references
    0 and 2, zero for reference 1."""
    refs, cur = frames(3)
    rows = [c for c in sample(0, 12, salt=7) if c[3] * c[4] <= 1024][:5]
    cost = {(r, 0): {} for r in range(3)}
    cpmv = {(r, 0): {} for r in range(3)}
    seed, mvp = {}, {}
    for row, x, y, w, h in rows:
        for r in range(3):
            mv, _ = S.seed_cu(refs[r], cur, x, y, w, h, 16, LAM)
            cp, c = S.search_cu(refs[r], cur, x, y, w, h, 2, [0] * 6, LAM)
            cost[(r, 0)][row], cpmv[(r, 0)][row] = c, [2] + cp[:4] + [0, 0]
            seed[(r, row)] = mv
            mvp.setdefault((r, 0), {})[row] = [0, 0] if r == 1 else list(mv)
    return rows, cost, cpmv, seed, mvp


# ------------------------------------------------------------------ zero predictors are the existing references
def test_zero_predictors_give_the_existing_references():
    refs, cur = frames()
    for (d, _), want in list(zip(search_cases_p(), search_reference_zero()))[::3]:
        assert R.search_cu_p(refs[d[4]], cur, d[0], d[1], d[2], d[3], d[5], d[6:12], ZERO, LAM) == want
    for (d, _, _), want in list(zip(bi_cases_p(), refine_reference_zero()))[::3]:
        assert R.refine_bicu_p_trace(refs, cur, d, ZERO, ZERO, LAM, 2) == want
    for d, _, _ in bi_cases_p()[::2]:
        s, c = R.predict_bicu_p(refs, cur, d, ZERO, ZERO, LAM)
        ws, wc = B.predict_bicu(refs, cur, d, LAM)
        assert c == wc and np.array_equal(s, ws)
    rows, cost, cpmv, seed, _ = row_case()
    refs3, cur3 = frames(3)
    zero = {(r, 0): {row: [0, 0] for row, *_ in rows} for r in range(3)}
    ids = [c[0] for c in rows]
    want = B.bipred(cur3, refs3, cost, cpmv, 1, LAM, rows={0: ids})[0]
    got = R.bipred_p(cur3, refs3, cost, cpmv, 1, LAM, zero, {0: ids})[0]
    for row in ids:
        assert got[row] == (int(want[0][row]), int(want[1][row]))
    row, x, y, w, h = rows[0]
    base = (cost[(0, 0)][row], cpmv[(0, 0)][row][1:])
    assert R.merged_p(refs3[0], cur3, x, y, w, h, seed[(0, row)], ZERO, LAM, base) == \
        S.merged(refs3[0], cur3, x, y, w, h, seed[(0, row)], LAM, base)


def test_reprice_row_is_the_cost_of_the_prediction():
    refs, cur = frames()
    for d, P in search_cases_p()[::2]:
        wide = d + [-1] + [0] * 7
        zero_cost = B.predict_bicu(refs, cur, wide, LAM)[1]
        assert R.reprice_row(zero_cost, d[6:12], d[5], P, LAM) == R.predict_bicu_p(refs, cur, wide, P, ZERO, LAM)[1]


def test_region_predictors_fall_back_to_smaller_squares():
    cands = B.frame_candidates(W, H, 0)
    seeds = {(0, 0): np.arange(2 * len(cands), dtype=np.int32).reshape(-1, 2)}
    got = R.region_predictors(W, H, seeds, 64)
    full = {(x, y, w): row for row, x, y, w, h in cands if w == h}
    for align in (0, 1):
        sides = set()
        for row, x, y, w, h in B.frame_candidates(W, H, align):
            side = next((s for s in (64, 32, 16) if x // s * s + s <= W and y // s * s + s <= H), 0)
            sides.add(side)
            assert (side == 0) == (x >= W or y >= H)  # only a CU whose top-left sample is outside gets (0, 0)
            want = seeds[(0, 0)][full[(x // side * side, y // side * side, side)]] if side else [0, 0]
            assert got[(0, align)][row].tolist() == list(want)
        assert sides == {64, 32, 16, 0}  # the cut CTU row: y >= 192 holds 32 (192..223) and 16 (224..239)


# ------------------------------------------------------------------ what the GPU cases exercise
def test_the_cases_cover_what_they_should():
    """The GPU tests compare the kernels with these references; an
    implementation that ignores the predictor must fail them, so the predictor
    has to change results, not only costs."""
    cs = search_cases_p()
    moved = {2: 0, 3: 0}
    for (d, _), (cp, _), (cpz, _) in zip(cs, search_reference_p(0), search_reference_zero()):
        moved[d[5]] += cp != cpz
    assert moved[2] >= 1 and moved[3] >= 1, moved
    bi = [t[-1][0] != z[-1][0] for (d, _, _), t, z in zip(bi_cases_p(), refine_reference_p(), refine_reference_zero())
          if d[12] >= 0]
    assert sum(bi) >= 1
    # every size class of the 64-, 256- and 512-thread instances, uni and bi
    for sizes in ({d[2] * d[3] // 16 for d, _ in cs}, {d[2] * d[3] // 16 for d, _, _ in bi_cases_p() if d[12] >= 0}):
        assert any(n <= 64 for n in sizes) and any(64 < n <= 256 for n in sizes) and any(n > 256 for n in sizes)
    assert {d[5] for d, _ in cs} == {2, 3} and any(d[12] < 0 for d, _, _ in bi_cases_p())
    # the refinement never raises the cost, and the costs differ from the zero-predictor ones
    for t in refine_reference_p():
        assert t[0][1] >= t[1][1] >= t[2][1]
    # bipred_p picks another pair than bipred for a row
    rows, cost, cpmv, seed, mvp = row_case()
    refs3, cur3 = frames(3)
    ids = [c[0] for c in rows]
    zero = B.bipred(cur3, refs3, cost, cpmv, 1, LAM, rows={0: ids})[0]
    new_cost = {k: dict(v) for k, v in cost.items()}
    for row in ids:
        for r in range(3):
            new_cost[(r, 0)][row] = R.reprice_row(cost[(r, 0)][row], cpmv[(r, 0)][row][1:], 2, R.expand(mvp[(r, 0)][row]), LAM)
    withp = R.bipred_p(cur3, refs3, new_cost, cpmv, 1, LAM, mvp, {0: ids})[0]
    assert any(withp[row][1] != int(zero[1][row]) for row in ids), (withp, [int(zero[1][row]) for row in ids])
    # merged_p takes a seeded row that merged leaves, or the other way round
    flips = 0
    for row, x, y, w, h in rows:
        for r, sd in ((0, seed[(0, row)]), (1, (16, 0))):
            base = (cost[(r, 0)][row], cpmv[(r, 0)][row][1:])
            P = R.expand(seed[(r, row)])
            took = S.merged(refs3[r], cur3, x, y, w, h, sd, LAM, base)[0][0] < base[0]
            base_p = (R.reprice_row(base[0], base[1], 2, P, LAM), base[1])
            took_p = R.merged_p(refs3[r], cur3, x, y, w, h, sd, P, LAM, base_p)[0][0] < base_p[0]
            flips += took != took_p
    assert flips >= 1
