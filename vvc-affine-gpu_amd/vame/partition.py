"""The outputs of vame_partition and vame_partition_bi (include/vame.h) as
device tensors, to_host, which cuts them at the leaf count, and the candidate
table.  Engine.partition / partition_bi make the calls."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from ._lib import MAX_PENALTY, MODES, check, lib  # noqa: F401  (MAX_PENALTY: re-exported)

KEYS = ("cus", "rows", "ncus", "ctu_info", "ctu_cost", "block_cu")


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


def alloc_keys(keys, cols: int, n_ctus: int, device) -> dict:
    """The outputs `keys` of vame_partition (cols = 12) / vame_partition_bi (20)."""
    shapes = {"cus": (n_ctus * 64, cols), "ncus": (), "ctu_info": (n_ctus, 4), "ctu_cost": (n_ctus,)}
    return {k: torch.empty(shapes.get(k, (n_ctus * 64,)), dtype=torch.int64 if k == "ctu_cost" else torch.int32,
                           device=device) for k in keys}


def keys_to_host(keys, part: dict) -> dict:
    """The outputs `keys` as numpy arrays, the per-leaf ones cut at the leaf
    count (synchronizes: reads the count)."""
    n = int(part["ncus"])
    out = {k: part[k].cpu().numpy()[:n] if k in ("cus", "rows", "sel") else part[k].cpu().numpy() for k in keys}
    out["ncus"] = n
    return out


def alloc(n_ctus: int, device) -> dict:
    return alloc_keys(KEYS, 12, n_ctus, device)


def to_host(part: dict) -> dict:
    """The outputs as numpy arrays, cus and rows cut at the leaf count
    (synchronizes: reads the count)."""
    return keys_to_host(KEYS, part)
