"""CPU reference of the seeded search (test infrastructure; DESIGN.md section
15), one CU per call.

seed_cu    vame_seed_search's rule: the integer displacement of the smallest
           SAD + rate inside +-radius, first minimum in the order (0, 0), then
           dy outer, dx inner; plain numpy sums (sad_map), bits and rate from
           the oracle (rate_table), the selection (seed_from_map).
search_cu  vame_affine_search's rule: oracle/vame_oracle.c:run_cu with init =
           caller-given CPMVs.  Predictions, samples, SATD, bits and rate come
           from bipred_ref (acc_cu, uni_sample, satd_cu, bits_of, rate), one
           update from birefine_ref.step with e = cur - P.
seed_3cp   the oracle's exported vame_oracle_seed_3cp.
merged     vame_affine_me_seeded's rule for one row.
Nothing here shares code with the kernels.
"""
from __future__ import annotations

import functools

import numpy as np

import bipred_ref as B
import birefine_ref as F
import oracle_py as O

INF = (1 << 63) - 1
LAM = 78.949063


@functools.lru_cache(maxsize=None)
def rate_table(radius, lam):
    """int64 [2 radius + 1, 2 radius + 1] at [dy + radius, dx + radius]: the
    search's rate of the 2-CP CPMVs LT = RT = (16 dx, 16 dy), ruiBits included."""
    n = 2 * radius + 1
    t = np.zeros((n, n), np.int64)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            t[dy + radius, dx + radius] = B.rate(B.bits_of(2, (16 * dx, 16 * dy, 16 * dx, 16 * dy, 0, 0)) + 2, lam)
    return t


def sad_map(ref, cur, x, y, w, h, radius):
    """int64 [2 radius + 1, 2 radius + 1] at [dy + radius, dx + radius]: the
    SAD of the CU against the reference block displaced by (dx, dy), reference
    coordinates clamped to the frame."""
    H, W = cur.shape
    blk = cur[y:y + h, x:x + w].astype(np.int64)
    yy = np.clip(np.arange(y - radius, y + radius + h), 0, H - 1)
    xx = np.clip(np.arange(x - radius, x + radius + w), 0, W - 1)
    win = ref.astype(np.int64)[yy][:, xx]
    n = 2 * radius + 1
    out = np.zeros((n, n), np.int64)
    for j in range(n):
        rows = win[j:j + h]
        for i in range(n):
            out[j, i] = np.abs(blk - rows[:, i:i + w]).sum()
    return out


def seed_from_map(sads, x, y, w, h, W, H, radius, lam):
    """vame_seed_search's selection on a sad_map of at least `radius`."""
    if x + w > W or y + h > H:
        return (0, 0), INF
    big = (sads.shape[0] - 1) // 2
    d = np.arange(-radius, radius + 1)
    v = sads[big - radius:big + radius + 1, big - radius:big + radius + 1] + rate_table(radius, lam)
    v = np.where((d[:, None] <= H + 7 - y) & (d[None, :] <= W + 7 - x), v, INF)
    k = int(np.argmin(v))  # the first minimum in the order dy outer, dx inner
    j, i = divmod(k, 2 * radius + 1)
    if not v[j, i] < v[radius, radius]:  # (0, 0) comes first
        return (0, 0), int(v[radius, radius])
    return (16 * int(d[i]), 16 * int(d[j])), int(v[j, i])


def seed_cu(ref, cur, x, y, w, h, radius, lam):
    """((mvx, mvy) in 1/16 pel, cost) of the CU (x, y, w, h)."""
    H, W = cur.shape
    if x + w > W or y + h > H:
        return (0, 0), INF
    return seed_from_map(sad_map(ref, cur, x, y, w, h, radius), x, y, w, h, W, H, radius, lam)


def search_cu(ref, cur, x, y, w, h, ncp, cp, lam, extra=0):
    """(best CPMVs [6 ints], cost) of run_cu from the CPMVs cp (6 ints; a
    2-CP run keeps its LB), for a CU wholly in the frame."""
    H, W = cur.shape
    assert x + w <= W and y + h <= H
    curr = [int(v) for v in cp]
    best, best_cost = list(curr), None
    niter = (4 if ncp == 3 else 5) + extra
    cur_cu = cur[y:y + h, x:x + w].astype(np.int64)
    for it in range(niter + 1):
        P = B.uni_sample(B.acc_cu(ref, x, y, w, h, ncp, curr)[0])
        cost = B.satd_cu(cur, x, y, w, h, P) + B.rate(B.bits_of(ncp, curr) + 2, lam)
        assert cost < 1 << 30  # run_cu's start: iteration 0 always becomes the best
        if best_cost is None or cost < best_cost:
            best_cost, best = cost, list(curr)
        if it == niter:
            break
        Pf = B.to_frame(P, w, h)
        curr = F.step(curr, ncp, Pf, cur_cu - Pf, x, y, w, h, W, H)
    return best, best_cost


def seed_3cp(cp, x, y, w, h, W, H):
    """The 3-CP start (6 ints) the fused search derives from 2-CP CPMVs."""
    prev, out = np.zeros(1, O.CPMVS_DTYPE), np.zeros(1, O.CPMVS_DTYPE)
    prev[0] = (2,) + tuple(int(v) for v in cp[:4]) + (0, 0)
    O.lib().vame_oracle_seed_3cp(O.ptr(prev), w, h, x, y, W, H, O.ptr(out))
    return [int(v) for v in out[0].tolist()[1:]]


def merged(ref, cur, x, y, w, h, seed, lam, base2, base3=None, extra=0):
    """vame_affine_me_seeded's rule for one row: base2 / base3 = (cost, CPMVs
    [6]) of the row's 2-CP / 3-CP result (base3 None: 2-CP only).  Returns
    [(cost, CPMVs)] for 2-CP and, with base3, 3-CP."""
    H, W = cur.shape
    out = [(int(base2[0]), [int(v) for v in base2[1]])]
    if base3 is not None:
        out.append((int(base3[0]), [int(v) for v in base3[1]]))
    if tuple(seed) == (0, 0) or x + w > W or y + h > H:
        return out
    c2, k2 = search_cu(ref, cur, x, y, w, h, 2, [seed[0], seed[1], seed[0], seed[1], 0, 0], lam, extra)
    if k2 < out[0][0]:
        out[0] = (k2, c2[:4] + [0, 0])
    if base3 is not None:
        c3, k3 = search_cu(ref, cur, x, y, w, h, 3, seed_3cp(c2, x, y, w, h, W, H), lam, extra)
        if k3 < out[1][0]:
            out[1] = (k3, c3)
    return out


@functools.lru_cache(maxsize=None)
def shifted_camera(nrefs=1):
    """The shifted-camera pair at 416x240, seed 0xBEEF: (refs [nrefs, H, W],
    cur) -- cur is POC 2 seen through a window moved by (-11, +6) samples,
    refs[r] the QP-32 reconstruction of POC r (nrefs <= 4)."""
    from vame import synth
    W, H = 416, 240
    big = {p: synth.synth_frame(W + 128, H + 128, p, 0xBEEF) for p in {0, 1, 2} | set(range(nrefs))}
    refs = [synth.recon_frame(big[p], p, 32, 0xBEEF)[64:64 + H, 64:64 + W] for p in range(nrefs)]
    cur = big[2][70:70 + H, 53:53 + W]
    return np.ascontiguousarray(np.stack(refs)).astype(np.uint16), np.ascontiguousarray(cur).astype(np.uint16)
