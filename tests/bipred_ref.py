"""CPU reference of affine bi-prediction (test infrastructure; DESIGN.md
section 13): a vectorised numpy restatement, a whole CU per call, of
  * the two-stage 6-tap filter up to its second-stage accumulator
    acc = sum + 512 + (8192 << 6) (oracle/vame_oracle.c predict_4x4; the tap
    table below is that file's LUMA), the uni sample clip(acc >> 10) and the
    bi sample clip((acc0 + acc1) >> 11);
  * the bi cost: SATD of the bi block + floor(lam * (bits0 + bits1 + 4)), with
    SATD, bits and rate from the oracle (oracle_py);
  * vame_bipred's rule: per row and refIdx the cheaper model, the first minimum
    over the pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3);
  * vame_partition_bi's rule, as a subclass of partition_ref.Partition.
The sub-block MVs come from mc_ref.subblock_mvs.  Nothing here shares code with
the kernels.
"""
from __future__ import annotations

import ctypes

import numpy as np

import mc_ref
import oracle_py as O
import partition_ref as R
from vame.hostlogic import geometry

# oracle/vame_oracle.c LUMA (constants.cl:40-58 m_lumaFilter4x4)
LUMA = np.array([
    [0, 0, 0, 64, 0, 0, 0, 0], [0, 1, -3, 63, 4, -2, 1, 0], [0, 1, -5, 62, 8, -3, 1, 0], [0, 2, -8, 60, 13, -4, 1, 0],
    [0, 3, -10, 58, 17, -5, 1, 0], [0, 3, -11, 52, 26, -8, 2, 0], [0, 2, -9, 47, 31, -10, 3, 0],
    [0, 3, -11, 45, 34, -10, 3, 0], [0, 3, -11, 40, 40, -11, 3, 0], [0, 3, -10, 34, 45, -11, 3, 0],
    [0, 3, -10, 31, 47, -9, 2, 0], [0, 2, -8, 26, 52, -11, 3, 0], [0, 1, -5, 17, 58, -10, 3, 0],
    [0, 1, -4, 13, 60, -8, 2, 0], [0, 1, -3, 8, 62, -5, 1, 0], [0, 1, -2, 4, 63, -3, 1, 0]], np.int64)
INF = (1 << 63) - 1
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
PER = (201, 284)


def acc_blocks(ref: np.ndarray, x0, y0, mvx, mvy) -> np.ndarray:
    """The second-stage accumulators [n, 4, 4] (int64) of the 4x4 blocks at
    frame positions (x0[n], y0[n]) with MVs (mvx[n], mvy[n]) in 1/16 pel:
    window clamped to the frame edges."""
    H, W = ref.shape
    x0, y0, mvx, mvy = (np.asarray(a, np.int64).reshape(-1) for a in (x0, y0, mvx, mvy))
    fx, fy = mvx & 15, mvy & 15
    bx, by = x0 + (mvx >> 4) - 3, y0 + (mvy >> 4) - 3  # 11x11 window origin
    r, c, k = np.arange(11), np.arange(4), np.arange(8)
    yy = np.clip(by[:, None] + r[None, :], 0, H - 1)                                  # [n, 11]
    xx = np.clip(bx[:, None, None] + c[None, :, None] + k[None, None, :], 0, W - 1)   # [n, 4, 8]
    win = ref.astype(np.int64)[yy[:, :, None, None], xx[:, None, :, :]]               # [n, 11, 4, 8]
    tmp = ((win * LUMA[fx][:, None, None, :]).sum(-1) - 8192 * 4) >> 2                # [n, 11, 4]
    rows = np.arange(4)[:, None] + k[None, :]                                         # [4, 8]
    acc = (tmp[:, rows, :] * LUMA[fy][:, None, :, None]).sum(2)                       # [n, 4, 4]
    return acc + 512 + (8192 << 6)


def uni_sample(acc):
    return np.clip(acc >> 10, 0, 1023)


def bi_sample(acc0, acc1):
    return np.clip((acc0 + acc1) >> 11, 0, 1023)


def acc_cu(ref: np.ndarray, x, y, w, h, ncp, cp):
    """(accumulators [nsb, 4, 4] of the CU's sub-blocks in raster order, spread)."""
    H, W = ref.shape
    x, y, w, h, ncp = int(x), int(y), int(w), int(h), int(ncp)
    mvs, spread = mc_ref.subblock_mvs(cp, ncp, x, y, w, h, W, H)
    a = np.array(mvs, np.int64).reshape(-1, 4)
    return acc_blocks(ref, x + a[:, 0], y + a[:, 1], a[:, 2], a[:, 3]), spread


def to_frame(blocks, w, h):
    """[nsb, 4, 4] sub-blocks in raster order -> [h, w]."""
    return np.asarray(blocks).reshape(h // 4, w // 4, 4, 4).transpose(0, 2, 1, 3).reshape(h, w)


def satd_cu(cur: np.ndarray, x, y, w, h, blocks) -> int:
    """Sum of the oracle's satd_4x4 of the CU's sub-blocks against `cur`."""
    L = O.lib()
    p = np.ascontiguousarray(blocks, np.int32).reshape(-1, 16)
    o = np.ascontiguousarray(cur[y:y + h, x:x + w].astype(np.int32).reshape(h // 4, 4, w // 4, 4)
                             .transpose(0, 2, 1, 3)).reshape(-1, 16)
    po, pp = o.ctypes.data, p.ctypes.data
    return sum(L.vame_oracle_satd4x4(po + 64 * k, pp + 64 * k) for k in range(len(p)))


def bits_of(ncp, cp) -> int:
    rec = np.zeros(1, O.CPMVS_DTYPE)
    rec[0] = (int(ncp),) + tuple(int(v) for v in cp)
    return int(O.lib().vame_oracle_affine_bits(O.ptr(rec), int(ncp)))


def rate(bits: int, lam: float) -> int:
    return int(O.lib().vame_oracle_rate_cost(int(bits), ctypes.c_float(lam)))


def predict_bicu(refs, cur, d, lam=0.0):
    """(samples [h, w] uint16, cost or None) of one 20-column descriptor d
    (vame.bipred.BICU_FIELDS); ref1 < 0: the uni prediction of (ref0, cp0)."""
    x, y, w, h, r0, n0 = (int(v) for v in d[:6])
    r1, n1 = int(d[12]), int(d[13])
    a0, _ = acc_cu(refs[r0], x, y, w, h, n0, d[6:12])
    if r1 < 0:
        s, bits = uni_sample(a0), bits_of(n0, d[6:12]) + 2
    else:
        a1, _ = acc_cu(refs[r1], x, y, w, h, n1, d[14:20])
        s, bits = bi_sample(a0, a1), bits_of(n0, d[6:12]) + bits_of(n1, d[14:20]) + 4
    cost = None if cur is None else satd_cu(cur, x, y, w, h, s) + rate(bits, lam)
    return to_frame(s, w, h).astype(np.uint16), cost


def frame_candidates(W, H, align):
    """[(row, x, y, w, h)] of every candidate CU of the alignment, row order."""
    cols = (W + 127) // 128
    n_ctus = cols * ((H + 127) // 128)
    out = []
    for ctu in range(n_ctus):
        X0, Y0 = (ctu % cols) * 128, (ctu // cols) * 128
        for w, h, xs, ys, stride in geometry(align):
            for k, (x, y) in enumerate(zip(xs.tolist(), ys.tolist())):
                out.append((ctu * PER[align] + stride + k, X0 + x, Y0 + y, w, h))
    return out


def hypothesis(cost, cpmv, r, align, row, mask):
    """(m, cp) of refIdx r's hypothesis for a row: the first minimum under
    strict < over m = 2-CP, 3-CP among the PREDs in the mask."""
    best, bm = None, None
    for m in (0, 1):
        if (mask >> (2 * align + m)) & 1:
            c = int(cost[(r, 2 * align + m)][row])
            if best is None or c < best:
                best, bm = c, m
    return bm, np.asarray(cpmv[(r, 2 * align + bm)][row])[-6:], best


def bipred(cur, refs, cost, cpmv, mask, lam, rows=None):
    """vame_bipred's rule.  cost / cpmv: {(refIdx, PRED): array}; rows: None or
    {align: iterable of rows} to compute (the others stay INF / -1).  Returns
    {align: (bi_cost int64[n], bi_sel int32[n], uni_min int64[n])} for the
    alignments in the mask; uni_min is the row's cheapest hypothesis cost, for
    the rows computed."""
    H, W = cur.shape
    nrefs = len(refs)
    out = {}
    for align in (0, 1):
        if not (mask >> (2 * align)) & 3:
            continue
        cands = frame_candidates(W, H, align)
        bc = np.full(len(cands), INF, np.int64)
        bs = np.full(len(cands), -1, np.int32)
        um = np.full(len(cands), INF, np.int64)
        want = None if rows is None else set(int(v) for v in rows[align])
        for row, x, y, w, h in cands:
            if x + w > W or y + h > H or nrefs < 2 or (want is not None and row not in want):
                continue
            hyp = []
            for r in range(nrefs):
                m, cp, c = hypothesis(cost, cpmv, r, align, row, mask)
                hyp.append((m, acc_cu(refs[r], x, y, w, h, 2 + m, cp)[0], bits_of(2 + m, cp)))
                um[row] = min(um[row], c)
            for r0, r1 in PAIRS:
                if r1 >= nrefs:
                    continue
                v = satd_cu(cur, x, y, w, h, bi_sample(hyp[r0][1], hyp[r1][1])) + \
                    rate(hyp[r0][2] + hyp[r1][2] + 4, lam)
                if v < bc[row]:
                    bc[row], bs[row] = v, r0 + 4 * hyp[r0][0] + 8 * r1 + 32 * hyp[r1][0]
        out[align] = (bc, bs, um)
    return out


class PartitionBi(R.Partition):
    """vame_partition_bi: partition_ref.Partition whose leaf value is the first
    minimum, under strict <, of the uni leaf minimum and bi_cost + bi_penalty
    (only where bi_sel >= 0).  bi: {align: (bi_cost, bi_sel, ...)}."""

    def __init__(self, W, H, cost, cpmv, nrefs, mask, penalty=0, bi=None, bi_penalty=0):
        super().__init__(W, H, cost, cpmv, nrefs, mask, penalty)
        self.leaf_bi = {}
        for align in list(self.leaf_cost):
            bc = np.asarray(bi[align][0], np.int64).reshape(self.n_ctus, PER[align])
            bs = np.asarray(bi[align][1], np.int64).reshape(self.n_ctus, PER[align])
            ok = bs >= 0
            term = np.where(ok, bc, 0) + int(bi_penalty)  # never add to INT64_MAX
            take = ok & (term < self.leaf_cost[align])
            self.leaf_cost[align] = np.where(take, term, self.leaf_cost[align])
            self.leaf_bi[align] = np.where(take, bs, -1)
            # the base class fills the first hypothesis from leaf_sel
            s = np.where(take, bs, 0)
            self.leaf_sel[align] = np.where(take[..., None], np.stack([s & 3, (s >> 2) & 1], -1), self.leaf_sel[align])

    def run(self):
        o = super().run()
        n = o["ncus"]
        cus = np.zeros((n, 20), np.int32)
        cus[:, :12] = o["cus"]
        cus[:, 12] = -1
        sel = np.full(n, -1, np.int32)
        cand = R.candidates()
        for i, (d, row) in enumerate(zip(o["cus"], o["rows"])):
            align, _ = cand[(int(d[0]) % 128, int(d[1]) % 128, int(d[2]), int(d[3]))]
            s = int(self.leaf_bi[align].reshape(-1)[row])
            if s >= 0:
                r1, m1 = (s >> 3) & 3, (s >> 5) & 1
                sel[i] = s
                cus[i, 12], cus[i, 13] = r1, 2 + m1
                cus[i, 14:] = np.asarray(self.cpmv[(r1, 2 * align + m1)][row])[-6:]
        o["cus"], o["sel"] = cus, sel
        return o


def partition_bi(W, H, cost, cpmv, nrefs, mask, penalty=0, bi=None, bi_penalty=0):
    return PartitionBi(W, H, cost, cpmv, nrefs, mask, penalty, bi, bi_penalty).run()
