"""Per-CU reference for vame_affine_mc (test infrastructure): the prediction
and the cost of caller-given CPMVs, from the CPU oracle's exported pieces.

The sub-block MV derivation is restated here from the reference --
deriveMv{2,3}Cps_and_spread (aux_functions.cl:146-212) and roundAndClipMv
(aux_functions.cl:90-101: roundMv :38-47, clipMv :51-67) -- and drives the
oracle's vame_oracle_spread, _predict_4x4 / _predict_4x4_prof, _satd4x4,
_affine_bits and _rate_cost.
"""
from __future__ import annotations

import ctypes

import numpy as np

import oracle_py as O


def _shl(a: int, s: int) -> int:
    """int32 left shift of the reference's kernels (wraps)."""
    v = (a << s) & 0xFFFFFFFF
    return v - (1 << 32) if v & 0x80000000 else v


def subblock_mvs(cp, ncp: int, x: int, y: int, w: int, h: int, W: int, H: int):
    """[(sx, sy, mvx, mvy)] of the CU's 4x4 sub-blocks in raster order, and the
    spread flag.  cp = (LTx, LTy, RTx, RTy, LBx, LBy)."""
    x, y, w, h = int(x), int(y), int(w), int(h)
    lw, lh = w.bit_length() - 1, h.bit_length() - 1
    ltx, lty, rtx, rty, lbx, lby = (int(v) for v in cp)
    hx, hy = _shl(rtx - ltx, 7 - lw), _shl(rty - lty, 7 - lw)      # aux_functions.cl:146-212
    if ncp == 3:
        vx, vy = _shl(lbx - ltx, 7 - lh), _shl(lby - lty, 7 - lh)
    else:
        vx, vy = -hy, hx
    bx, by = _shl(ltx, 7), _shl(lty, 7)
    spread = bool(O.lib().vame_oracle_spread(hx, hy, vx, vy))
    # clipMv against the CU position (aux_functions.cl:51-67)
    hmin, hmax = _shl(-128 - 8 - x + 1, 4), _shl(W + 8 - x - 1, 4)
    vmin, vmax = _shl(-128 - 8 - y + 1, 4), _shl(H + 8 - y - 1, 4)
    sy, sx = (a.reshape(-1) for a in np.meshgrid(np.arange(0, h, 4), np.arange(0, w, 4), indexing="ij"))
    px, py = (np.full_like(sx, w >> 1), np.full_like(sy, h >> 1)) if spread else (sx + 2, sy + 2)
    mx = bx + hx * px + vx * py  # int64: within 2^32 for CPMV components of 18 bits
    my = by + hy * px + vy * py
    mx = np.clip((mx + 64 - (mx >= 0)) >> 7, hmin, hmax)  # roundMv (aux_functions.cl:38-47), clipMv
    my = np.clip((my + 64 - (my >= 0)) >> 7, vmin, vmax)
    out = list(zip(sx.tolist(), sy.tolist(), mx.tolist(), my.tolist()))
    return out, spread


def predict_cu(ref: np.ndarray, cur: np.ndarray | None, x: int, y: int, w: int, h: int, ncp: int, cp,
               lam: float = 0.0, prof: bool = False):
    """(samples [h, w] uint16, cost or None, spread) of one CU.  ref / cur:
    (H, W) uint16 frames; cost = sum of satd_4x4 + floor(lam * (bits + 2))
    (affine.cl:416-446: zero predictor, ruiBits = 2)."""
    L = O.lib()
    H, W = ref.shape
    x, y, w, h, ncp = int(x), int(y), int(w), int(h), int(ncp)
    ref = np.ascontiguousarray(ref, dtype=np.uint16)
    mvs, spread = subblock_mvs(cp, ncp, x, y, w, h, W, H)
    rec = np.zeros(1, O.CPMVS_DTYPE)
    rec[0] = (ncp,) + tuple(int(v) for v in cp)
    use_prof = prof and not spread  # applyPROF = enablePROF && !isSpread (aux_functions.cl:1101)
    if use_prof:
        dh, dv = O.prof_deltas(rec, ncp, w, h)
    # one oracle call per sub-block, on rows of [nsb, 16] arrays addressed directly
    nsb = len(mvs)
    out = np.zeros((nsb, 16), np.int32)
    pref, pout = O.ptr(ref), out.ctypes.data
    if use_prof:
        pdh, pdv = O.ptr(dh), O.ptr(dv)
        for k, (sx, sy, mx, my) in enumerate(mvs):
            L.vame_oracle_predict_4x4_prof(pref, W, H, x + sx, y + sy, mx, my, pdh, pdv, pout + 64 * k)
    else:
        for k, (sx, sy, mx, my) in enumerate(mvs):
            L.vame_oracle_predict_4x4(pref, W, H, x + sx, y + sy, mx, my, pout + 64 * k)
    pred = out.reshape(h // 4, w // 4, 4, 4).transpose(0, 2, 1, 3).reshape(h, w).astype(np.uint16)
    satd = 0
    if cur is not None:
        o = np.ascontiguousarray(cur[y:y + h, x:x + w].astype(np.int32).reshape(h // 4, 4, w // 4, 4)
                                 .transpose(0, 2, 1, 3)).reshape(nsb, 16)
        po = o.ctypes.data
        for k in range(nsb):
            satd += L.vame_oracle_satd4x4(po + 64 * k, pout + 64 * k)
    if cur is None:
        return pred, None, spread
    bits = L.vame_oracle_affine_bits(O.ptr(rec), ncp)
    return pred, satd + int(L.vame_oracle_rate_cost(bits + 2, ctypes.c_float(lam))), spread
