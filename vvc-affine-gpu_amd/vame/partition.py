"""ctypes plumbing of vame_partition (include/vame.h): the CU partition
decision on the search's result arrays, its outputs as device tensors, and
to_host, which cuts them at the leaf count."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from ._lib import PocResult, check, lib

MODES = ("FULL_2CP", "FULL_3CP", "HALF_2CP", "HALF_3CP")
KEYS = ("cus", "rows", "ncus", "ctu_info", "ctu_cost", "block_cu")
MAX_PENALTY = 1 << 40


def table() -> np.ndarray:
    """vame_partition_table: int32[1024], slot ((lh*4 + lw)*8 + y/16)*8 + x/16 ->
    align*512 + output offset of the candidate CU, or -1."""
    t = np.empty(1024, np.int32)
    check(lib().vame_partition_table(t.ctypes.data_as(ctypes.c_void_p)))
    return t


def result_preds(result: dict) -> int:
    """The PRED mask (bit m of MODES) an alloc_poc dict holds."""
    mask = 0
    for _, name in result:
        mask |= 1 << MODES.index(name)
    return mask


def alloc(n_ctus: int, device) -> dict:
    i32 = dict(dtype=torch.int32, device=device)
    return {"cus": torch.empty((n_ctus * 64, 12), **i32), "rows": torch.empty(n_ctus * 64, **i32),
            "ncus": torch.empty((), **i32), "ctu_info": torch.empty((n_ctus, 4), **i32),
            "ctu_cost": torch.empty(n_ctus, dtype=torch.int64, device=device),
            "block_cu": torch.empty(n_ctus * 64, **i32)}


def partition(handle, n_ctus: int, device, result: dict, preds: int, split_penalty: int, stream, out=None) -> dict:
    """One vame_partition call on `stream`; `result` is an alloc_poc dict
    {(refIdx, MODE): (cost, cpmv)} that holds every PRED of `preds` for
    refIdx 0 .. nrefs-1."""
    nrefs = max(r for r, _ in result) + 1
    pr = PocResult()
    for (r, name), (cost, cpmv) in result.items():
        m = MODES.index(name)
        pr.cost[r][m] = cost.data_ptr()
        pr.cpmvs[r][m] = cpmv.data_ptr()
    part = out if out is not None else alloc(n_ctus, device)
    V = ctypes.c_void_p
    check(lib().vame_partition(handle, ctypes.byref(pr), nrefs, int(preds), int(split_penalty),
                               *(V(part[k].data_ptr()) for k in KEYS), stream))
    return part


def to_host(part: dict) -> dict:
    """The outputs as numpy arrays, cus and rows cut at the leaf count
    (synchronizes: reads the count)."""
    n = int(part["ncus"])
    out = {k: part[k].cpu().numpy() for k in KEYS}
    out["cus"], out["rows"], out["ncus"] = out["cus"][:n], out["rows"][:n], n
    return out
