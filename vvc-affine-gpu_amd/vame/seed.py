"""Descriptors for Engine.affine_search (vame_affine_search, include/vame.h)
from seeds: the translational starts Engine.seed_search finds, or any other
MVs.  Pure torch indexing: runs on CPU tensors too."""
from __future__ import annotations

import torch

from ._lib import CUS_PER_CTU, lib
from .mc import candidate_geometry


def cus_from_seeds(W: int, H: int, align: int, mv: torch.Tensor, ref: int = 0, skip_zero: bool = True):
    """2-CP descriptors [n, 12] int32 (vame.mc.CU_FIELDS, on mv's device), LT =
    RT = the row's seed and LB = 0, for the candidate CUs of `align` that lie
    wholly in the frame, and the int64 row indices kept.  mv: [nCtus *
    CUS_PER_CTU[align], 2] in 1/16 pel, as Engine.seed_search returns it.  skip_zero
    drops the rows whose seed is (0, 0) -- the search's own start, which
    vame_affine_me_seeded skips."""
    n_all = lib().vame_num_ctus(W, H) * CUS_PER_CTU[bool(align)]
    if mv.dim() != 2 or tuple(mv.shape) != (n_all, 2):
        raise ValueError(f"mv must be [{n_all}, 2]")
    rows, x, y, w, h = candidate_geometry(W, H, align)
    keep = (x + w <= W) & (y + h <= H)
    rows, x, y, w, h = (t[keep].to(mv.device) for t in (rows, x, y, w, h))
    seed = mv[rows].to(torch.int32)
    if skip_zero:
        nz = (seed != 0).any(1)
        rows, x, y, w, h, seed = (t[nz] for t in (rows, x, y, w, h, seed))
    cus = torch.zeros((rows.numel(), 12), dtype=torch.int32, device=mv.device)
    for k, t in enumerate((x, y, w, h)):
        cus[:, k] = t
    cus[:, 4] = ref
    cus[:, 5] = 2
    cus[:, 6:8] = seed
    cus[:, 8:10] = seed
    return cus, rows
