"""Descriptors for Engine.affine_mc (vame_affine_mc, include/vame.h) from the
search's result arrays.  Pure torch indexing: runs on CPU tensors too."""
from __future__ import annotations

import numpy as np
import torch

from ._lib import CUS_PER_CTU, lib
from .hostlogic import geometry

CU_FIELDS = ("x", "y", "w", "h", "ref", "nCPs", "LTx", "LTy", "RTx", "RTy", "LBx", "LBy")
CTU = 128


def candidate_geometry(W: int, H: int, align: int, groups=None):
    """(rows, x, y, w, h) int64 CPU tensors of the candidate CUs of an
    alignment in the frame, in the reference's index order
    ctu * CUS_PER_CTU[align] + RETURN_STRIDE[group] + cuIdx (affine.cl:936 / :1929).
    groups: group indices into vame_group_geometry(align, .) and / or (w, h)
    sizes; None = every group."""
    n_ctus = lib().vame_num_ctus(W, H)
    if not n_ctus or align not in (0, 1):
        raise ValueError(f"unsupported resolution {W}x{H} or alignment {align}")
    per = CUS_PER_CTU[align]
    cols = (W + CTU - 1) // CTU  # integer ceil, as the engine's ctusPerRow
    geo = geometry(align)
    if groups is None:
        sel = range(len(geo))
    else:
        want = list(groups)
        sel = [g for g, (w, h, _, _, _) in enumerate(geo) if g in want or (w, h) in want]
        if not sel:
            raise ValueError(f"no CU group of alignment {align} matches {want}")
    off, cx, cy, cw, ch = [], [], [], [], []
    for g in sel:
        w, h, xs, ys, stride = geo[g]
        off.append(stride + np.arange(len(xs)))
        cx.append(xs)
        cy.append(ys)
        cw.append(np.full(len(xs), w))
        ch.append(np.full(len(xs), h))
    off, cx, cy, cw, ch = (torch.from_numpy(np.concatenate(a).astype(np.int64)) for a in (off, cx, cy, cw, ch))
    ctu = torch.arange(n_ctus, dtype=torch.int64)[:, None]
    rows = (ctu * per + off[None, :]).reshape(-1)
    x = ((ctu % cols) * CTU + cx[None, :]).reshape(-1)
    y = ((ctu // cols) * CTU + cy[None, :]).reshape(-1)
    w = cw[None, :].expand(n_ctus, -1).reshape(-1)
    h = ch[None, :].expand(n_ctus, -1).reshape(-1)
    return rows, x, y, w, h


def cus_from_result(W: int, H: int, align: int, ncp: int, cpmv: torch.Tensor, ref: int = 0, groups=None,
                    inframe_only: bool = True):
    """Descriptors [n, 12] int32 (columns CU_FIELDS, on cpmv's device) for the
    candidate CUs of `align` -- or of the size groups in `groups` -- with the
    CPMVs of a result array `cpmv` ([nCtus * CUS_PER_CTU[align], 7] as the engine
    returns it, or its last 6 columns), and the int64 row indices kept.
    inframe_only drops the CUs that leave the frame (x + w > W or y + h > H),
    which the search prices at their rate alone and vame_affine_mc rejects."""
    if ncp not in (2, 3):
        raise ValueError("ncp must be 2 or 3")
    rows, x, y, w, h = candidate_geometry(W, H, align, groups)
    n_all = lib().vame_num_ctus(W, H) * CUS_PER_CTU[align]
    if cpmv.dim() != 2 or cpmv.shape[0] != n_all or cpmv.shape[1] not in (6, 7):
        raise ValueError(f"cpmv must be [{n_all}, 7] (or its last 6 columns)")
    if inframe_only:
        keep = (x + w <= W) & (y + h <= H)
        rows, x, y, w, h = (t[keep] for t in (rows, x, y, w, h))
    dev = cpmv.device
    rows = rows.to(dev)
    cus = torch.empty((rows.numel(), 12), dtype=torch.int32, device=dev)
    for k, t in enumerate((x, y, w, h)):
        cus[:, k] = t.to(dev)
    cus[:, 4] = ref
    cus[:, 5] = ncp
    cus[:, 6:] = cpmv[rows][:, -6:].to(torch.int32)
    return cus, rows
