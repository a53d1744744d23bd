"""Refinement of bi-predicted CUs, host side: the CPU restatement of
vame_bipred_refine's rule (tests/birefine_ref.py) on the two-reference goldens
-- its invariants, a pinned list of candidates that covers every size class,
and the flat-frame (singular system) path.  No device work."""
import functools
import os

import numpy as np
import pytest

import bipred_ref as B
import birefine_ref as F

GOLD = os.path.join(os.path.dirname(__file__), "golden")
NAMES = ("FULL_2CP", "FULL_3CP", "HALF_2CP", "HALF_3CP")

# aligned candidates of s416_qp32_poc2 (row in the FULL arrays): frame x, y, w, h, the models of refIdx 0 / 1's
# hypothesis and the bi cost after 0 and after 2 rounds.  Every size class w * h holds a row that two rounds
# strictly improve; row 1304 only improves in its second round (hypothesis 0 moving).
PINNED = {
    1164: ((224, 160, 16, 16), (2, 2), 3532, 3419),
    597: ((288, 112, 16, 16), (2, 2), 3858, 3706),
    182: ((80, 80, 16, 16), (2, 2), 3522, 3522),
    904: ((96, 224, 32, 16), (2, 2), 4645, 4348),
    1304: ((288, 224, 32, 16), (3, 2), 4132, 4034),
    524: ((272, 64, 16, 32), (2, 2), 4358, 4318),
    1259: ((256, 224, 64, 16), (2, 2), 6535, 6347),
    847: ((0, 144, 64, 16), (2, 2), 7003, 6827),
    1465: ((400, 128, 16, 64), (2, 2), 30829, 30829),
    10: ((64, 0, 64, 32), (2, 2), 10799, 10554),
    224: ((192, 64, 32, 64), (2, 2), 10661, 10299),
    810: ((64, 128, 64, 64), (2, 3), 18198, 18150),
    208: ((128, 64, 64, 64), (2, 2), 15651, 15629),
    205: ((192, 0, 64, 128), (3, 3), 35625, 35089),
    406: ((320, 0, 64, 128), (2, 3), 33292, 32927),
    805: ((0, 128, 128, 64), (3, 2), 32535, 32535),
    201: ((128, 0, 128, 128), (3, 3), 62714, 62600),
    0: ((0, 0, 128, 128), (2, 2), 60764, 60764),
}
SIZE_CLASSES = (256, 512, 1024, 2048, 4096, 8192, 16384)


@functools.lru_cache(maxsize=None)
def poc2_inputs():
    zs = [dict(np.load(os.path.join(GOLD, f"s416_qp32_poc2_ref{r}.npz"))) for r in (0, 1)]
    cost = {(r, m): z[n + "_cost"] for r, z in enumerate(zs) for m, n in enumerate(NAMES)}
    cpmv = {(r, m): z[n + "_cpmv"] for r, z in enumerate(zs) for m, n in enumerate(NAMES)}
    return [z["ref"] for z in zs], zs[0]["cur"], float(zs[0]["lam"]), cost, cpmv


def poc2_desc(row, geo):
    """The bi descriptor vame_bipred's pair (0, 1) gives the aligned candidate
    `row` at geo = (x, y, w, h): each reference's cheaper model."""
    _, _, _, cost, cpmv = poc2_inputs()
    hyp = [B.hypothesis(cost, cpmv, r, 0, row, 15) for r in (0, 1)]
    return list(geo) + [0, 2 + hyp[0][0]] + [int(v) for v in hyp[0][1]] + \
        [1, 2 + hyp[1][0]] + [int(v) for v in hyp[1][1]]


@functools.lru_cache(maxsize=None)
def pinned_traces():
    """{row: refine_bicu_trace(.., rounds = 2)} of the pinned rows, computed once."""
    refs, cur, lam, _, _ = poc2_inputs()
    return {row: F.refine_bicu_trace(refs, cur, poc2_desc(row, geo), lam, 2) for row, (geo, _, _, _) in PINNED.items()}


def test_pinned_rows_are_the_fixture_candidates():
    geo = {row: (x, y, w, h) for row, x, y, w, h in B.frame_candidates(416, 240, 0)}
    for row, (g, models, _, _) in PINNED.items():
        d = poc2_desc(row, g)
        assert geo[row] == g and (d[5], d[13]) == models, row
    assert {m for _, m, _, _ in PINNED.values()} == {(2, 2), (2, 3), (3, 2), (3, 3)}


def test_rounds_0_is_the_bi_cost():
    refs, cur, lam, _, _ = poc2_inputs()
    for row, (geo, _, before, _) in PINNED.items():
        d = poc2_desc(row, geo)
        out, cost = pinned_traces()[row][0]
        assert out == d and cost == B.predict_bicu(refs, cur, d, lam)[1] == before, row
        assert F.refine_bicu(refs, cur, d, lam, 0) == (d, before)


def test_cost_never_rises_and_is_the_cost_of_the_returned_descriptor():
    refs, cur, lam, _, _ = poc2_inputs()
    for row, trace in pinned_traces().items():
        costs = [c for _, c in trace]
        assert costs[0] >= costs[1] >= costs[2], row
        for out, cost in trace:
            assert cost == B.predict_bicu(refs, cur, out, lam)[1], row
            assert out[:6] == trace[0][0][:6] and out[12:14] == trace[0][0][12:14]
        # round 0 moves hypothesis 1 alone, round 1 hypothesis 0 alone
        assert trace[1][0][6:12] == trace[0][0][6:12] and trace[2][0][14:20] == trace[1][0][14:20], row
        # a 2-CP hypothesis keeps its LB
        for k, base in ((5, 10), (13, 18)):
            if trace[0][0][k] == 2:
                assert trace[2][0][base:base + 2] == trace[0][0][base:base + 2], row


def test_pinned_costs_and_a_gain_in_every_size_class():
    gained = set()
    for row, ((x, y, w, h), _, before, after) in PINNED.items():
        trace = pinned_traces()[row]
        assert (trace[0][1], trace[2][1]) == (before, after), row
        if after < before:
            gained.add(w * h)
            assert trace[2][0] != trace[0][0]
        else:
            assert trace[2][0] == trace[0][0]  # strict <: an equal cost keeps the CPMVs
    assert gained == set(SIZE_CLASSES)
    # a third and fourth round go on from the second's result
    refs, cur, lam, _, _ = poc2_inputs()
    t4 = F.refine_bicu_trace(refs, cur, poc2_desc(847, PINNED[847][0]), lam, 4)
    assert t4[:3] == pinned_traces()[847] and t4[4][1] <= t4[3][1] <= t4[2][1]


def test_uni_descriptor_passes_through():
    refs, cur, lam, _, _ = poc2_inputs()
    d = poc2_desc(597, PINNED[597][0])[:12] + [-1] + [7] * 7
    assert F.refine_bicu_trace(refs, cur, d, lam, 2) == [(d, B.predict_bicu(refs, cur, d, lam)[1])] * 3


@pytest.mark.parametrize("geo", [(0, 0, 16, 16), (64, 64, 64, 64), (288, 112, 128, 128)])
def test_flat_frames_leave_the_cpmvs_unchanged(geo):
    """Zero gradients: an all-zero system, NaN through solve_equal's division
    and scale_delta's conversion, a zero delta."""
    z = np.load(os.path.join(GOLD, "s416_flat.npz"))
    assert z["ref"].min() == z["ref"].max() and z["cur"].min() == z["cur"].max()
    refs, cur, lam = [z["ref"], z["ref"]], z["cur"], float(z["lam"])
    for n0, n1 in ((2, 3), (3, 2)):
        d = list(geo) + [0, n0, 5, -3, 9, 2, 7 * (n0 - 2), -4 * (n0 - 2), 1, n1, -6, 8, -2, 11, 3 * (n1 - 2), 0]
        gx, gy = F.sobel(np.full((geo[3], geo[2]), 512))
        assert not gx.any() and not gy.any()
        assert F.step(d[6:12], n0, np.full((geo[3], geo[2]), 512), np.zeros((geo[3], geo[2]), np.int64),
                      *geo, 416, 240) == d[6:12]
        trace = F.refine_bicu_trace(refs, cur, d, lam, 2)
        assert all(out == d for out, _ in trace) and trace[0][1] == trace[2][1]
