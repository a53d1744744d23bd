"""Affine bi-prediction (vame_affine_mc_bi, vame_bipred, vame_partition_bi;
include/vame.h): the descriptor layout, the pair
selection code and descriptors from a selection.  Pure torch indexing: runs on
CPU tensors too."""
from __future__ import annotations

import torch

from ._lib import CUS_PER_CTU, MAX_PENALTY, MODES  # noqa: F401  (MAX_PENALTY: re-exported)
from .mc import CU_FIELDS, candidate_geometry
from .partition import alloc_keys, keys_to_host

# vame_mc_bicu: a vame_mc_cu, then ref1 (-1: uni-predicted) and the second hypothesis
BICU_FIELDS = CU_FIELDS[:4] + ("ref0", "nCPs0", "LTx0", "LTy0", "RTx0", "RTy0", "LBx0", "LBy0",
                               "ref1", "nCPs1", "LTx1", "LTy1", "RTx1", "RTy1", "LBx1", "LBy1")
KEYS = ("cus", "rows", "sel", "ncus", "ctu_info", "ctu_cost", "block_cu")
NONE_COST = (1 << 63) - 1  # bi_cost of a row without a pair


def pairs(nrefs: int):
    """The candidate reference pairs r0 < r1 in the order vame_bipred tries them."""
    if not 1 <= nrefs <= 4:
        raise ValueError("nrefs must be in 1..4")
    return [(r0, r1) for r0 in range(nrefs) for r1 in range(r0 + 1, nrefs)]


def encode_sel(r0, m0, r1, m1):
    """bi_sel = r0 + 4*m0 + 8*r1 + 32*m1 (m = 0: 2-CP, 1: 3-CP); ints or tensors."""
    return r0 + 4 * m0 + 8 * r1 + 32 * m1


def decode_sel(sel):
    """(r0, m0, r1, m1) of a bi_sel >= 0; ints or tensors."""
    return sel & 3, (sel >> 2) & 1, (sel >> 3) & 3, (sel >> 5) & 1


def bicus_from_sel(W: int, H: int, align: int, result: dict, sel: torch.Tensor, rows: torch.Tensor):
    """Descriptors [n, 20] int32 (columns BICU_FIELDS, on sel's device) of the
    candidate CUs `rows` (indices into the arrays of `align`) with the two
    hypotheses that sel[row] names; a row with sel < 0 comes out uni-less
    (ref0 = ref1 = -1: an invalid descriptor).  result: an alloc_poc dict
    {(refIdx, MODE): (cost, cpmv)}; sel: the whole bi_sel array of `align`."""
    geo_rows, x, y, w, h = candidate_geometry(W, H, align)
    n_all = geo_rows.numel()
    if sel.dim() != 1 or sel.numel() != n_all:
        raise ValueError(f"sel must hold {n_all} entries")
    dev = sel.device
    rows = rows.to(device=dev, dtype=torch.int64).reshape(-1)
    if rows.numel() and (int(rows.min()) < 0 or int(rows.max()) >= n_all):
        raise ValueError("rows outside the alignment's arrays")
    # candidate_geometry lists rows group by group per CTU: the inverse map
    inv = torch.empty(n_all, dtype=torch.int64)
    inv[geo_rows] = torch.arange(n_all)
    at = inv.to(dev)[rows]
    cus = torch.zeros((rows.numel(), 20), dtype=torch.int32, device=dev)
    for k, t in enumerate((x, y, w, h)):
        cus[:, k] = t.to(dev)[at].to(torch.int32)
    s = sel[rows].to(torch.int64)
    ok = s >= 0
    r0, m0, r1, m1 = decode_sel(torch.where(ok, s, torch.zeros_like(s)))
    cus[:, 4] = torch.where(ok, r0, -torch.ones_like(r0)).to(torch.int32)
    cus[:, 12] = torch.where(ok, r1, -torch.ones_like(r1)).to(torch.int32)
    for base, rr, mm in ((5, r0, m0), (13, r1, m1)):
        cus[:, base] = torch.where(ok, 2 + mm, torch.zeros_like(mm)).to(torch.int32)
        for (r, name), (_, cpmv) in result.items():
            m = MODES.index(name)
            if m >> 1 != align:
                continue
            pick = ok & (rr == r) & (mm == (m & 1))
            if bool(pick.any()):
                cus[pick, base + 1:base + 7] = cpmv.to(dev)[rows[pick]][:, -6:].to(torch.int32)
    return cus


def alloc(n_ctus: int, device) -> dict:
    """The outputs of vame_partition_bi."""
    return alloc_keys(KEYS, 20, n_ctus, device)


def alloc_bi(n_ctus: int, device) -> dict:
    """The outputs of vame_bipred: {"cost": [FULL, HALF], "sel": [FULL, HALF]}."""
    return {"cost": [torch.empty(n_ctus * per, dtype=torch.int64, device=device) for per in CUS_PER_CTU],
            "sel": [torch.empty(n_ctus * per, dtype=torch.int32, device=device) for per in CUS_PER_CTU]}


def to_host(part: dict) -> dict:
    """The outputs as numpy arrays, cus, rows and sel cut at the leaf count
    (synchronizes: reads the count)."""
    return keys_to_host(KEYS, part)
