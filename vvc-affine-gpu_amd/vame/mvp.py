"""Motion-vector predictors for the calls that price CPMVs against one
(Engine.reprice, affine_me_seeded_p, bipred_p, leaf_predictors; include/vame.h,
DESIGN.md section 17).

region_predictors is a MODEL, not an encoder's AMVP: one base MV per region and
reference, taken from the seed search.  A caller with real predictors
(neighbour-derived candidates, a merge list) passes its own arrays in the same
layout.  Pure torch indexing on the seeds' device: no host read, capturable."""
from __future__ import annotations

import functools

import numpy as np
import torch

from ._lib import CUS_PER_CTU as PER
from ._lib import lib
from .hostlogic import geometry


@functools.lru_cache(maxsize=None)
def _region_index(W: int, H: int, size: int):
    """Per alignment (src int64 [rows], ok bool [rows]), CPU tensors: the row
    of the FULL square candidate whose seed is the row's predictor, built once
    on the host from vame_group_geometry."""
    if size not in (16, 32, 64, 128):
        raise ValueError("size must be 16, 32, 64 or 128")
    n_ctus = lib().vame_num_ctus(W, H)
    if not n_ctus:
        raise ValueError(f"unsupported resolution {W}x{H}")
    cols = (W + 127) // 128
    square = {}  # (side, x, y) CTU-relative -> offset in the FULL arrays
    for w, h, xs, ys, stride in geometry(0):
        if w == h:
            for k, (x, y) in enumerate(zip(xs.tolist(), ys.tolist())):
                square[(w, x, y)] = stride + k
    out = []
    for align in (0, 1):
        src = np.zeros(n_ctus * PER[align], np.int64)
        ok = np.zeros(n_ctus * PER[align], bool)
        for ctu in range(n_ctus):
            X0, Y0 = (ctu % cols) * 128, (ctu // cols) * 128
            for w, h, xs, ys, stride in geometry(align):
                for k, (x, y) in enumerate(zip(xs.tolist(), ys.tolist())):
                    row = ctu * PER[align] + stride + k
                    S = size
                    while S >= 16:
                        sx, sy = x // S * S, y // S * S
                        if X0 + sx + S <= W and Y0 + sy + S <= H:
                            src[row], ok[row] = ctu * PER[0] + square[(S, sx, sy)], True
                            break
                        S //= 2
        out.append((torch.from_numpy(src), torch.from_numpy(ok)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _region_index_on(W: int, H: int, size: int, device: str):
    return tuple((s.to(device), o.to(device)) for s, o in _region_index(W, H, size))


def region_predictors(W: int, H: int, seeds: dict, size: int = 64) -> dict:
    """A stand-in for real AMVP candidates: {(r, a): int32 [rows, 2]} for both
    alignments of every refIdx r with FULL seeds (r, 0) in `seeds` (Engine.
    seed_search()["mv"]), in the layout the row-layout calls take.

    This is a model: one base MV per region and reference.  A row's predictor
    is the seed MV of the FULL square candidate CU of side S that holds the
    CU's top-left sample; S runs over size, size/2, ..., 16 and the first
    square that lies wholly in the frame wins; if none does, the predictor is
    (0, 0).  So every CU inside one size x size region shares one predictor
    per reference, as neighbouring CUs of an encoder share theirs; nothing is
    derived from coded neighbours.  A caller with real predictors passes its
    own arrays instead.  torch index ops on the seeds' device only."""
    out = {}
    for (r, a), mv in sorted(seeds.items()):
        if a != 0:
            continue
        idx = _region_index_on(W, H, int(size), str(mv.device))
        if mv.dim() != 2 or mv.shape[0] != idx[0][0].numel() or mv.shape[1] != 2:
            raise ValueError(f"seeds[{(r, a)}] must be [{idx[0][0].numel()}, 2]")
        for align in (0, 1):
            src, ok = idx[align]
            out[(r, align)] = torch.where(ok[:, None], mv[src], torch.zeros_like(mv[src])).to(torch.int32).contiguous()
    return out
