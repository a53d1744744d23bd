"""Motion compensation, host side: the per-CU reference (tests/mc_ref.py)
against the reference's own outputs, and vame.mc.cus_from_result's geometry
against the oracle's tables.  No device work.

For every row of every golden fixture
    golden cost == SATD(cur, prediction from the golden CPMVs) + rate(golden CPMVs, lambda)
because the search keeps the cost it computed for the CPMVs it kept -- so the
reference's outputs pin the prediction and cost of caller-given CPMVs."""
import os

import numpy as np
import pytest
import torch

import mc_ref
import oracle_py as O
from vame.mc import candidate_geometry, cus_from_result

GOLD = os.path.join(os.path.dirname(__file__), "golden")
MODES = {"FULL_2CP": (0, 2), "FULL_3CP": (0, 3), "HALF_2CP": (1, 2), "HALF_3CP": (1, 3)}


@pytest.mark.parametrize("name", ["s416_bigmotion", "s416_noise"])
def test_mc_ref_reproduces_golden_costs(name):
    z = dict(np.load(os.path.join(GOLD, name + ".npz")))
    W, H, lam = int(z["W"]), int(z["H"]), float(z["lam"])
    rows_checked = spread_rows = 0
    for mode, (align, ncp) in MODES.items():
        cus, rows = cus_from_result(W, H, align, ncp, torch.from_numpy(z[mode + "_cpmv"]))
        want = z[mode + "_cost"][rows.numpy()]
        got = np.zeros_like(want)
        for k, d in enumerate(cus.numpy()):
            _, got[k], spread = mc_ref.predict_cu(z["ref"], z["cur"], d[0], d[1], d[2], d[3], ncp, d[6:], lam)
            spread_rows += spread
        np.testing.assert_array_equal(got, want, err_msg=f"{name} {mode}")
        rows_checked += len(rows)
    assert rows_checked == 5588
    if name == "s416_bigmotion":  # the fixture that exercises the spread fallback
        assert spread_rows == 197


def oracle_rows(W, H, align):
    """(row, x, y, w, h) of every candidate CU from the oracle's group tables."""
    per = 284 if align else 201
    cols = (W + 127) // 128
    out = []
    for ctu in range(O.lib().vame_oracle_num_ctus(W, H)):
        for w, h, xs, ys, stride in O.group_geometry(align):
            for k in range(len(xs)):
                out.append((ctu * per + stride + k, (ctu % cols) * 128 + int(xs[k]), (ctu // cols) * 128 + int(ys[k]),
                            w, h))
    return np.array(out, np.int64)


@pytest.mark.parametrize("W,H", [(416, 240), (832, 480)])
def test_cus_from_result_geometry(W, H):
    kept_total = all_total = 0
    for mode, (align, ncp) in MODES.items():
        want = oracle_rows(W, H, align)
        n = len(want)
        assert n == O.lib().vame_oracle_num_ctus(W, H) * (284 if align else 201)
        cpmv = torch.arange(n * 7, dtype=torch.int32).reshape(n, 7)
        cus, rows = cus_from_result(W, H, align, ncp, cpmv, ref=2, inframe_only=False)
        assert cus.dtype == torch.int32 and tuple(cus.shape) == (n, 12) and rows.dtype == torch.int64
        order = np.argsort(rows.numpy(), kind="stable")
        got = cus.numpy()[order]
        np.testing.assert_array_equal(rows.numpy()[order], np.arange(n))  # every row exactly once
        w_sorted = want[np.argsort(want[:, 0], kind="stable")]
        np.testing.assert_array_equal(got[:, :4], w_sorted[:, 1:])
        assert (got[:, 4] == 2).all() and (got[:, 5] == ncp).all()
        np.testing.assert_array_equal(got[:, 6:], cpmv.numpy()[:, 1:])  # the row's own CPMVs
        # a 6-column array (the golden layout) gives the same descriptors
        cus6, rows6 = cus_from_result(W, H, align, ncp, cpmv[:, 1:].contiguous(), ref=2, inframe_only=False)
        assert torch.equal(cus6, cus) and torch.equal(rows6, rows)
        # in-frame set
        cus_in, rows_in = cus_from_result(W, H, align, ncp, cpmv)
        inside = (w_sorted[:, 1] + w_sorted[:, 3] <= W) & (w_sorted[:, 2] + w_sorted[:, 4] <= H)
        np.testing.assert_array_equal(np.sort(rows_in.numpy()), np.nonzero(inside)[0])
        ci = cus_in.numpy()
        assert ((ci[:, 0] + ci[:, 2] <= W) & (ci[:, 1] + ci[:, 3] <= H)).all()
        np.testing.assert_array_equal(ci[:, 6:], cpmv.numpy()[rows_in.numpy(), 1:])
        kept_total += len(rows_in)
        all_total += n
    if (W, H) == (416, 240):
        assert (kept_total, all_total) == (5588, 7760)


def test_affine_mc_rejects_bad_arguments_without_a_device():
    """Argument errors come back before any device work (no context, no
    outputs, too many references)."""
    import ctypes

    from vame import _lib
    L = _lib.lib()
    one = ctypes.c_void_p(8)  # never dereferenced
    refs = (ctypes.c_void_p * 4)(8, 8, 8, 8)
    assert L.vame_affine_mc(None, one, refs, 1, one, 1, 0.0, one, one, one, None) == -1
    assert _lib.EXPORTS.count("vame_affine_mc") == 1


def test_cus_from_result_groups():
    """Size groups by (w, h) or by group index; the aligned 128x128, 64x32 and
    16x16 groups each tile the CTU."""
    W, H = 416, 240
    cpmv = torch.zeros((8 * 201, 6), dtype=torch.int32)
    for size in ((128, 128), (64, 32), (16, 16)):
        cus, rows = cus_from_result(W, H, 0, 2, cpmv, groups=[size], inframe_only=False)
        c = cus.numpy()
        assert ((c[:, 2] == size[0]) & (c[:, 3] == size[1])).all()
        cover = np.zeros((256, 512), np.int32)
        for x, y, w, h in c[:, :4]:
            cover[y:y + h, x:x + w] += 1
        assert (cover == 1).all()
    geo = O.group_geometry(0)
    g = next(i for i, t in enumerate(geo) if t[:2] == (64, 32))
    a, ra = cus_from_result(W, H, 0, 2, cpmv, groups=[g])
    b, rb = cus_from_result(W, H, 0, 2, cpmv, groups=[(64, 32)])
    assert torch.equal(a, b) and torch.equal(ra, rb)
    rows, *_ = candidate_geometry(W, H, 0, groups=[g])
    assert len(rows) == 8 * len(geo[g][2])
    with pytest.raises(ValueError):
        cus_from_result(W, H, 0, 2, cpmv, groups=[(48, 48)])
    with pytest.raises(ValueError):
        cus_from_result(W, H, 0, 4, cpmv)
    with pytest.raises(ValueError):
        cus_from_result(W, H, 1, 2, cpmv)  # a FULL array for HALF
