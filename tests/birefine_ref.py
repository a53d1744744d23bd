"""CPU reference of vame_bipred_refine (test infrastructure; DESIGN.md section
14), one CU per call: oracle/vame_oracle.c:run_cu with two references.

One hypothesis of a bi descriptor is held, the other runs run_cu's loop against
what the held one leaves to explain, e = 2 cur - P_fixed - P_moving; round t
moves hypothesis 1 - (t & 1).  Predictions, samples, SATD, bits and rate come
from bipred_ref (acc_cu, uni_sample, bi_sample, satd_cu, bits_of, rate), the
solve and the delta scaling from the oracle's exported vame_oracle_solve and
vame_oracle_scale_delta; the Sobel gradients with CU-border replication, the
normal equations, the dd mapping, the clamp and clip_mv are restated here from
run_cu (oracle/vame_oracle.c:499-561) and clip_mv (:150-157).  Nothing here
shares code with the kernels.
"""
from __future__ import annotations

import ctypes

import numpy as np

import bipred_ref as B
import oracle_py as O

MV_MAX, MV_MIN = (1 << 17) - 1, -(1 << 17)


def _shl(a: int, s: int) -> int:
    v = (a << s) & 0xFFFFFFFF
    return v - (1 << 32) if v & 0x80000000 else v


def _wrap_add(a: int, b: int) -> int:
    """int32 a + b with the wrap of run_cu's unsigned add."""
    v = (a + b) & 0xFFFFFFFF
    return v - (1 << 32) if v & 0x80000000 else v


def clip_mv(mx, my, x, y, W, H):
    """oracle/vame_oracle.c clip_mv: block position = CU position."""
    hmax, hmin = _shl(W + 8 - x - 1, 4), _shl(-128 - 8 - x + 1, 4)
    vmax, vmin = _shl(H + 8 - y - 1, 4), _shl(-128 - 8 - y + 1, 4)
    return min(max(mx, hmin), hmax), min(max(my, vmin), vmax)


def sobel(P):
    """(gx, gy) int64 [h, w] of the samples P [h, w] with CU-border replication
    (run_cu: rr = clamp(r, 1, h - 2), cc = clamp(c, 1, w - 2))."""
    P = np.asarray(P, np.int64)
    h, w = P.shape
    gx = np.zeros((h, w), np.int64)
    gy = np.zeros((h, w), np.int64)
    up, mid, dn = P[:-2], P[1:-1], P[2:]
    gx[1:-1, 1:-1] = (up[:, 2:] - up[:, :-2]) + 2 * (mid[:, 2:] - mid[:, :-2]) + (dn[:, 2:] - dn[:, :-2])
    gy[1:-1, 1:-1] = (dn[:, :-2] - up[:, :-2]) + 2 * (dn[:, 1:-1] - up[:, 1:-1]) + (dn[:, 2:] - up[:, 2:])
    rr = np.clip(np.arange(h), 1, h - 2)
    cc = np.clip(np.arange(w), 1, w - 2)
    return gx[rr][:, cc], gy[rr][:, cc]


def equations(gx, gy, e, ncp):
    """run_cu's int64 system as the 7x7 row-major matrix solve_equal takes:
    rows 1 .. n hold [A | 8 b], row 0 and the unused columns zero."""
    h, w = gx.shape
    n = 2 * ncp
    cy = ((np.arange(h) >> 2) << 2)[:, None] + 2 + np.zeros((1, w), np.int64)
    cx = ((np.arange(w) >> 2) << 2)[None, :] + 2 + np.zeros((h, 1), np.int64)
    if ncp == 3:
        iC = [gx, cx * gx, gy, cx * gy, cy * gx, cy * gy]
    else:
        iC = [gx, cx * gx + cy * gy, gy, cy * gx - cx * gy]
    A = [[0] * 7 for _ in range(7)]
    for col in range(n):
        for row in range(n):
            A[col + 1][row] = int((iC[col] * iC[row]).sum())
        A[col + 1][n] = int((iC[col] * e).sum()) * 8
    for row in A:
        for v in row:
            assert abs(v) < 1 << 53, "the int64 sums convert exactly"
    return np.array(A, np.float64)


def step(cp, ncp, Pm, e, x, y, w, h, W, H):
    """One update of run_cu (lines 499-561) on the samples Pm with the error
    term e: the next CPMVs (6 ints; a 2-CP hypothesis keeps its LB)."""
    L = O.lib()
    L.vame_oracle_scale_delta.restype = ctypes.c_int
    gx, gy = sobel(Pm)
    D = np.ascontiguousarray(equations(gx, gy, np.asarray(e, np.int64), ncp))
    p = np.zeros(6, np.float64)
    L.vame_oracle_solve(O.ptr(D), 2 * ncp, O.ptr(p))
    dd = [0.0] * 6
    dd[0], dd[2] = p[0], p[2]
    if ncp == 3:
        dd[1] = p[1] * w + p[0]
        dd[3] = p[3] * w + p[2]
        dd[4] = p[4] * h + p[0]
        dd[5] = p[5] * h + p[2]
    else:
        dd[1] = p[1] * w + p[0]
        dd[3] = -p[3] * w + p[2]
    # LT = (d0, d2), RT = (d1, d3), LB = (d4, d5)
    order = (0, 2, 1, 3, 4, 5)
    out = [int(v) for v in cp]
    for j in range(2 * ncp):
        v = _wrap_add(out[j], int(L.vame_oracle_scale_delta(ctypes.c_double(dd[order[j]]))))
        out[j] = min(max(v, MV_MIN), MV_MAX)
    for k in range(ncp):
        out[2 * k], out[2 * k + 1] = clip_mv(out[2 * k], out[2 * k + 1], x, y, W, H)
    return out


def bi_cost(cur, x, y, w, h, acc0, acc1, bits0, bits1, lam):
    return B.satd_cu(cur, x, y, w, h, B.bi_sample(acc0, acc1)) + B.rate(bits0 + bits1 + 4, lam)


def refine_bicu_trace(refs, cur, d, lam, rounds):
    """[(descriptor [20 ints], cost)] after 0, 1, .. `rounds` rounds of one
    valid 20-column descriptor d (vame.bipred.BICU_FIELDS): entry r is
    vame_bipred_refine's result with rounds = r.  A uni descriptor (ref1 < 0)
    stays unchanged at its uni cost."""
    d = [int(v) for v in d]
    x, y, w, h = d[:4]
    if d[12] < 0:
        return [(d, B.predict_bicu(refs, cur, d, lam)[1])] * (rounds + 1)
    H, W = cur.shape
    ref = (refs[d[4]], refs[d[12]])
    ncp = (d[5], d[13])
    best = [d[6:12], d[14:20]]
    acc = [B.acc_cu(ref[k], x, y, w, h, ncp[k], best[k])[0] for k in (0, 1)]
    best_cost = bi_cost(cur, x, y, w, h, acc[0], acc[1], B.bits_of(ncp[0], best[0]), B.bits_of(ncp[1], best[1]), lam)
    cur_cu = cur[y:y + h, x:x + w].astype(np.int64)
    trace = [(list(d), best_cost)]
    for t in range(rounds):
        m = 1 - (t & 1)
        f = 1 - m
        acc_f = B.acc_cu(ref[f], x, y, w, h, ncp[f], best[f])[0]
        Pf = B.to_frame(B.uni_sample(acc_f), w, h)
        bits_f = B.bits_of(ncp[f], best[f])
        curr = list(best[m])
        niter = 4 if ncp[m] == 3 else 5
        for it in range(niter + 1):
            acc_m = B.acc_cu(ref[m], x, y, w, h, ncp[m], curr)[0]
            cost = bi_cost(cur, x, y, w, h, acc_m, acc_f, B.bits_of(ncp[m], curr), bits_f, lam)
            if cost < best_cost:
                best_cost, best[m] = cost, list(curr)
            if it == niter:
                break
            Pm = B.to_frame(B.uni_sample(acc_m), w, h)
            e = 2 * cur_cu - Pf - Pm
            assert np.abs(e).max() <= 2046
            curr = step(curr, ncp[m], Pm, e, x, y, w, h, W, H)
        trace.append((d[:6] + [int(v) for v in best[0]] + d[12:14] + [int(v) for v in best[1]], best_cost))
    return trace


def refine_bicu(refs, cur, d, lam, rounds):
    """(descriptor with refined CPMVs [20 ints], cost): the last entry of
    refine_bicu_trace."""
    return refine_bicu_trace(refs, cur, d, lam, rounds)[-1]
