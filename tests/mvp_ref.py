"""CPU reference of the rates against a motion-vector predictor (test
infrastructure), one CU or row per call.

bits_p            the rule of include/vame.h, from the oracle's exported
                  vame_oracle_eg_bits and the formula; the 1/16 -> 1/4 pel
                  rounding is restated here.
predict_bicu_p    vame_affine_mc_bi_p: bipred_ref's samples, the rate against
                  the hypotheses' predictors.
search_cu_p       vame_affine_search_p: seed_ref.search_cu's loop with bits_p.
refine_bicu_p     vame_bipred_refine_p: birefine_ref.refine_bicu_trace's loop
                  with bits_p per hypothesis.
bipred_p          vame_bipred_p: bipred_ref.bipred's rule, the pair's rate
                  against the row's predictors.
reprice_row       vame_reprice for one row.
merged_p          vame_affine_me_seeded_p's rule for one row.
region_predictors vame.mvp.region_predictors, restated with plain loops.
A predictor is 6 ints (LTx, LTy, RTx, RTy, LBx, LBy); a translational one
repeats (x, y) three times (expand).  Composed from bipred_ref (acc_cu,
uni_sample, bi_sample, satd_cu, rate) and birefine_ref.step.  Nothing here
shares code with the kernels.
"""
from __future__ import annotations

import numpy as np

import bipred_ref as B
import birefine_ref as F
import oracle_py as O
import seed_ref as S

INF = B.INF
ZERO = (0, 0, 0, 0, 0, 0)
MV_MAX, MV_MIN = (1 << 17) - 1, -(1 << 17)


def q(v: int) -> int:
    """1/16 -> 1/4 pel: (v + 1) >> 2 for v >= 0, (v + 2) >> 2 below."""
    v = int(v)
    return (v + 1) >> 2 if v >= 0 else (v + 2) >> 2


def eg(v: int) -> int:
    return int(O.lib().vame_oracle_eg_bits(int(v)))


def bits_p(c, P, n) -> int:
    c, P = [int(v) for v in c], [int(v) for v in P]
    dx, dy = c[0] - P[0], c[1] - P[1]
    b = eg(q(c[0]) - q(P[0])) + eg(q(c[1]) - q(P[1]))
    b += eg(q(c[2]) - q(P[2] + dx)) + eg(q(c[3]) - q(P[3] + dy))
    if int(n) == 3:
        b += eg(q(c[4]) - q(P[4] + dx)) + eg(q(c[5]) - q(P[5] + dy))
    return b


def expand(mv):
    return [int(mv[0]), int(mv[1])] * 3


def pred_ok(P) -> bool:
    return all(MV_MIN <= int(v) <= MV_MAX for v in P)


def predict_bicu_p(refs, cur, d, P0, P1=ZERO, lam=0.0):
    """(samples [h, w] uint16, cost or None) of one 20-column descriptor d with
    hypothesis h priced against P<h> (P1 unused when ref1 < 0)."""
    x, y, w, h, r0, n0 = (int(v) for v in d[:6])
    r1, n1 = int(d[12]), int(d[13])
    a0, _ = B.acc_cu(refs[r0], x, y, w, h, n0, d[6:12])
    if r1 < 0:
        s, bits = B.uni_sample(a0), bits_p(d[6:12], P0, n0) + 2
    else:
        a1, _ = B.acc_cu(refs[r1], x, y, w, h, n1, d[14:20])
        s, bits = B.bi_sample(a0, a1), bits_p(d[6:12], P0, n0) + bits_p(d[14:20], P1, n1) + 4
    cost = None if cur is None else B.satd_cu(cur, x, y, w, h, s) + B.rate(bits, lam)
    return B.to_frame(s, w, h).astype(np.uint16), cost


def search_cu_p(ref, cur, x, y, w, h, ncp, cp, P, lam, extra=0):
    """(best CPMVs [6 ints], cost): seed_ref.search_cu with the rate of every
    iteration against P."""
    H, W = cur.shape
    assert x + w <= W and y + h <= H
    curr = [int(v) for v in cp]
    best, best_cost = list(curr), None
    niter = (4 if ncp == 3 else 5) + extra
    cur_cu = cur[y:y + h, x:x + w].astype(np.int64)
    for it in range(niter + 1):
        Ps = B.uni_sample(B.acc_cu(ref, x, y, w, h, ncp, curr)[0])
        cost = B.satd_cu(cur, x, y, w, h, Ps) + B.rate(bits_p(curr, P, ncp) + 2, lam)
        if best_cost is None or cost < best_cost:
            best_cost, best = cost, list(curr)
        if it == niter:
            break
        Pf = B.to_frame(Ps, w, h)
        curr = F.step(curr, ncp, Pf, cur_cu - Pf, x, y, w, h, W, H)
    return best, best_cost


def _bi_cost_p(cur, x, y, w, h, acc0, acc1, bits0, bits1, lam):
    return B.satd_cu(cur, x, y, w, h, B.bi_sample(acc0, acc1)) + B.rate(bits0 + bits1 + 4, lam)


def refine_bicu_p_trace(refs, cur, d, P0, P1, lam, rounds):
    """[(descriptor [20 ints], cost)] after 0 .. `rounds` rounds:
    birefine_ref.refine_bicu_trace with hypothesis h priced against P<h>."""
    d = [int(v) for v in d]
    x, y, w, h = d[:4]
    if d[12] < 0:
        return [(d, predict_bicu_p(refs, cur, d, P0, P1, lam)[1])] * (rounds + 1)
    H, W = cur.shape
    ref = (refs[d[4]], refs[d[12]])
    ncp = (d[5], d[13])
    PP = (P0, P1)
    best = [d[6:12], d[14:20]]
    acc = [B.acc_cu(ref[k], x, y, w, h, ncp[k], best[k])[0] for k in (0, 1)]
    best_cost = _bi_cost_p(cur, x, y, w, h, acc[0], acc[1], bits_p(best[0], P0, ncp[0]), bits_p(best[1], P1, ncp[1]), lam)
    cur_cu = cur[y:y + h, x:x + w].astype(np.int64)
    trace = [(list(d), best_cost)]
    for t in range(rounds):
        m = 1 - (t & 1)
        f = 1 - m
        acc_f = B.acc_cu(ref[f], x, y, w, h, ncp[f], best[f])[0]
        Pf = B.to_frame(B.uni_sample(acc_f), w, h)
        bits_f = bits_p(best[f], PP[f], ncp[f])
        curr = list(best[m])
        niter = 4 if ncp[m] == 3 else 5
        for it in range(niter + 1):
            acc_m = B.acc_cu(ref[m], x, y, w, h, ncp[m], curr)[0]
            cost = _bi_cost_p(cur, x, y, w, h, acc_m, acc_f, bits_p(curr, PP[m], ncp[m]), bits_f, lam)
            if cost < best_cost:
                best_cost, best[m] = cost, list(curr)
            if it == niter:
                break
            Pm = B.to_frame(B.uni_sample(acc_m), w, h)
            curr = F.step(curr, ncp[m], Pm, 2 * cur_cu - Pf - Pm, x, y, w, h, W, H)
        trace.append((d[:6] + [int(v) for v in best[0]] + d[12:14] + [int(v) for v in best[1]], best_cost))
    return trace


def refine_bicu_p(refs, cur, d, P0, P1, lam, rounds):
    return refine_bicu_p_trace(refs, cur, d, P0, P1, lam, rounds)[-1]


def reprice_row(cost, cp, n, P, lam) -> int:
    """vame_reprice for one in-frame row: the zero-predictor rate out, the
    rate against P in."""
    return int(cost) - B.rate(B.bits_of(n, cp) + 2, lam) + B.rate(bits_p(cp, P, n) + 2, lam)


def bipred_p(cur, refs, cost, cpmv, mask, lam, mvp, rows):
    """vame_bipred_p for the rows {align: iterable}: {align: {row: (bi_cost,
    bi_sel)}}.  cost / cpmv: {(refIdx, PRED): array} (costs as the caller
    re-priced them); mvp: {(refIdx, align): [rows, 2]}."""
    H, W = cur.shape
    nrefs = len(refs)
    out = {}
    for align in (0, 1):
        if not (mask >> (2 * align)) & 3 or align not in rows:
            continue
        geo = {c[0]: c for c in B.frame_candidates(W, H, align)}
        out[align] = {}
        for row in rows[align]:
            _, x, y, w, h = geo[int(row)]
            bc, bs = INF, -1
            if x + w <= W and y + h <= H and nrefs >= 2 and all(pred_ok(mvp[(r, align)][row]) for r in range(nrefs)):
                hyp = []
                for r in range(nrefs):
                    m, cp, _ = B.hypothesis(cost, cpmv, r, align, row, mask)
                    hyp.append((m, B.acc_cu(refs[r], x, y, w, h, 2 + m, cp)[0],
                                bits_p(cp, expand(mvp[(r, align)][row]), 2 + m)))
                for r0, r1 in B.PAIRS:
                    if r1 >= nrefs:
                        continue
                    v = B.satd_cu(cur, x, y, w, h, B.bi_sample(hyp[r0][1], hyp[r1][1])) + \
                        B.rate(hyp[r0][2] + hyp[r1][2] + 4, lam)
                    if v < bc:
                        bc, bs = v, r0 + 4 * hyp[r0][0] + 8 * r1 + 32 * hyp[r1][0]
            out[align][int(row)] = (int(bc), int(bs))
    return out


def merged_p(ref, cur, x, y, w, h, seed, P, lam, base2, base3=None, extra=0):
    """vame_affine_me_seeded_p's rule for one row: seed_ref.merged with both
    searches priced against P; base2 / base3 = (cost re-priced under P, CPMVs
    [6])."""
    H, W = cur.shape
    out = [(int(base2[0]), [int(v) for v in base2[1]])]
    if base3 is not None:
        out.append((int(base3[0]), [int(v) for v in base3[1]]))
    if tuple(seed) == (0, 0) or x + w > W or y + h > H or not pred_ok(P):
        return out
    c2, k2 = search_cu_p(ref, cur, x, y, w, h, 2, [seed[0], seed[1], seed[0], seed[1], 0, 0], P, lam, extra)
    if k2 < out[0][0]:
        out[0] = (k2, c2[:4] + [0, 0])
    if base3 is not None:
        c3, k3 = search_cu_p(ref, cur, x, y, w, h, 3, S.seed_3cp(c2, x, y, w, h, W, H), P, lam, extra)
        if k3 < out[1][0]:
            out[1] = (k3, c3)
    return out


def region_predictors(W, H, seeds, size=64):
    """{(r, align): int32 [rows, 2]} from {(r, 0): [rows, 2]} FULL seeds: the
    seed of the FULL square of side S = size, size/2, .., 16 that holds the
    CU's top-left sample, the first S whose square lies in the frame; else 0."""
    full = {(x, y, w): row for row, x, y, w, h in B.frame_candidates(W, H, 0) if w == h}
    out = {}
    for (r, a), mv in seeds.items():
        if a != 0:
            continue
        mv = np.asarray(mv)
        for align in (0, 1):
            cands = B.frame_candidates(W, H, align)
            o = np.zeros((len(cands), 2), np.int32)
            for row, x, y, w, h in cands:
                s = size
                while s >= 16:
                    sx, sy = x // s * s, y // s * s
                    if sx + s <= W and sy + s <= H:
                        o[row] = mv[full[(sx, sy, s)]]
                        break
                    s //= 2
            out[(r, align)] = o
    return out
