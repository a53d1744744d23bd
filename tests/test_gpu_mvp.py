"""Rates against a motion-vector predictor on the GPU (Engine.affine_mc_p,
affine_search_p, bipred_refine_p, reprice, affine_me_seeded_p, bipred_p,
leaf_predictors, vame.mvp.region_predictors): bit for bit
against the CPU restatement tests/mvp_ref.py, 416x240 throughout (8 CTUs, the
bottom CTU row cut, so rows leave the frame)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import bipred_ref as B
import mvp_ref as R
import seed_ref as S
import test_mvp as T
from test_gpu_bipred import NAMES, SENTINEL, blank, dev
from test_gpu_seed import clone_result
from test_seed import inframe, sample
from vame import mc as M
from vame import mvp as MVP
from vame import partition as PT
from vame import seed as V

pytestmark = pytest.mark.gpu

W, H = 416, 240
LAM = S.LAM
INF = B.INF
P_ = ctypes.c_void_p


@pytest.fixture(scope="module")
def eng():
    from vame.engine import Engine
    e = Engine(W, H, 0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def dev_frames(nrefs=2):
    refs, cur = T.frames(nrefs)
    return [dev(r) for r in refs], dev(cur)


def i32(a):
    return torch.tensor(np.asarray(a, np.int64).reshape(-1, np.asarray(a).shape[-1]), dtype=torch.int32).cuda()


def pred_rows(*Ps):
    """vame_cpmvs rows [n, 7] from 6-int predictors (nCPs column: anything)."""
    return i32([[9] + [int(v) for v in P] for P in Ps])


def search_inputs():
    cs = T.search_cases_p()
    return i32([d for d, _ in cs]), pred_rows(*[P for _, P in cs])


def bi_inputs():
    cs = T.bi_cases_p()
    return i32([d for d, _, _ in cs]), pred_rows(*[P for _, P0, P1 in cs for P in (P0, P1)])


# ------------------------------------------------------------------ 1. the three list calls against the reference
def test_affine_mc_p_against_reference(eng):
    refs, cur = T.frames()
    drefs, dcur = dev_frames()
    cus, preds = bi_inputs()
    pred = blank(H, W)
    _, cost, bad = eng.affine_mc_p(cus, preds, drefs, LAM, cur=dcur, pred=pred, want_cost=True)
    wpred, _, _ = eng.affine_mc_bi(cus, drefs, LAM, cur=dcur, pred=blank(H, W), want_cost=True)
    torch.cuda.synchronize()
    assert int(bad) == 0 and torch.equal(pred, wpred)  # the samples do not depend on the predictor
    for i, (d, P0, P1) in enumerate(T.bi_cases_p()):
        s, c = R.predict_bicu_p(refs, cur, d, P0, P1, LAM)
        assert int(cost[i]) == c, (i, d)
    # one descriptor alone: its samples are the reference's
    d, P0, P1 = T.bi_cases_p()[3]
    one = blank(H, W)
    eng.affine_mc_p(i32([d]), pred_rows(P0, P1), drefs, pred=one)
    torch.cuda.synchronize()
    s, _ = R.predict_bicu_p(refs, None, d, P0, P1)
    got = one.cpu().numpy().view(np.uint16)
    assert np.array_equal(got[d[1]:d[1] + d[3], d[0]:d[0] + d[2]], s)
    # 12-column descriptors are widened on the device
    cus12, p12 = search_inputs()
    _, cost12, bad = eng.affine_mc_p(cus12, p12, drefs, LAM, cur=dcur, want_cost=True)
    torch.cuda.synchronize()
    assert int(bad) == 0
    for i, (d, P) in enumerate(T.search_cases_p()):
        assert int(cost12[i]) == R.predict_bicu_p(refs, cur, d + [-1] + [0] * 7, P, R.ZERO, LAM)[1], (i, d)
    # lambda 0: the SATD, whatever the predictor
    _, c0, _ = eng.affine_mc_p(cus, preds, drefs, 0.0, cur=dcur, want_cost=True)
    _, w0, _ = eng.affine_mc_bi(cus, drefs, 0.0, cur=dcur, want_cost=True)
    torch.cuda.synchronize()
    assert torch.equal(c0, w0)


@pytest.mark.parametrize("extra", [0, 1])
def test_affine_search_p_against_reference(eng, extra):
    drefs, dcur = dev_frames()
    cus, preds = search_inputs()
    out, cost, bad = eng.affine_search_p(cus, preds, drefs, dcur, LAM, extra=extra)
    _, mc_cost, bad2 = eng.affine_mc_p(out, preds, drefs, LAM, cur=dcur, want_cost=True)
    torch.cuda.synchronize()
    assert int(bad) == 0 and int(bad2) == 0
    got = out.cpu().numpy()
    for i, ((d, _), (cp, c)) in enumerate(zip(T.search_cases_p(), T.search_reference_p(extra))):
        want = d[:6] + (cp if d[5] == 3 else cp[:4] + d[10:12])
        assert got[i].tolist() == want and int(cost[i]) == c, (i, d, got[i].tolist(), want, int(cost[i]), c)
    assert torch.equal(mc_cost, cost)  # bit for bit affine_mc_p's cost of out


@pytest.mark.parametrize("rounds", [0, 1, 2])
def test_bipred_refine_p_against_reference(eng, rounds):
    drefs, dcur = dev_frames()
    cus, preds = bi_inputs()
    out, cost, bad = eng.bipred_refine_p(cus, preds, drefs, dcur, LAM, rounds=rounds)
    _, mc_cost, _ = eng.affine_mc_p(out, preds, drefs, LAM, cur=dcur, want_cost=True)
    _, in_cost, _ = eng.affine_mc_p(cus, preds, drefs, LAM, cur=dcur, want_cost=True)
    torch.cuda.synchronize()
    assert int(bad) == 0
    got = out.cpu().numpy()
    for i, trace in enumerate(T.refine_reference_p()):
        wd, wc = trace[rounds]
        if wd[12] < 0:
            wd = T.bi_cases_p()[i][0]  # a uni descriptor is copied through as given
        assert got[i].tolist() == wd and int(cost[i]) == wc, (i, got[i].tolist(), wd, int(cost[i]), wc)
    assert torch.equal(mc_cost, cost) and (cost <= in_cost).all()


def test_no_predictor_and_zero_predictors_are_the_existing_calls(eng):
    drefs, dcur = dev_frames()
    cus, preds = bi_inputs()
    cus12, p12 = search_inputs()
    wp, wc, _ = eng.affine_mc_bi(cus, drefs, LAM, cur=dcur, pred=blank(H, W), want_cost=True)
    ws, wsc, _ = eng.affine_search(cus12, drefs, dcur, LAM, extra=1)
    wr, wrc, _ = eng.bipred_refine(cus, drefs, dcur, LAM, rounds=2)
    for zb, z12 in ((None, None), (torch.zeros_like(preds), torch.zeros_like(p12))):
        gp, gc, _ = eng.affine_mc_p(cus, zb, drefs, LAM, cur=dcur, pred=blank(H, W), want_cost=True)
        gs, gsc, _ = eng.affine_search_p(cus12, z12, drefs, dcur, LAM, extra=1)
        gr, grc, _ = eng.bipred_refine_p(cus, zb, drefs, dcur, LAM, rounds=2)
        torch.cuda.synchronize()
        assert torch.equal(gp, wp) and torch.equal(gc, wc)
        assert torch.equal(gs, ws) and torch.equal(gsc, wsc)
        assert torch.equal(gr, wr) and torch.equal(grc, wrc)


# ------------------------------------------------------------------ 2. invalid descriptors, the device count, in place
BAD_P = [1 << 17, 0, 0, 0, 0, 0]
BAD_LB = [0, 0, 0, 0, 0, -(1 << 17) - 1]


def invalid_bi():
    """[(descriptor, P0, P1)], one per cause of invalidity."""
    d, P0, P1 = T.bi_cases_p()[1]
    out = []
    for col, v in ((2, 17), (0, 404), (4, 2), (5, 4), (7, 1 << 17), (12, 2), (13, 1), (15, -(1 << 17) - 1)):
        e = list(d)
        e[col] = v
        out.append((e, P0, P1))
    out += [(list(d), BAD_P, P1), (list(d), P0, BAD_P), (list(d), BAD_LB, P1)]  # a predictor component out of range
    return out


def invalid_uni():
    d, P = T.search_cases_p()[1]
    out = []
    for col, v in ((3, 48), (1, 238), (4, -1), (5, 1), (9, 1 << 17)):
        e = list(d)
        e[col] = v
        out.append((e, P))
    return out + [(list(d), BAD_P), (list(d), BAD_LB)]


def test_invalid_descriptors_leave_their_neighbours_alone(eng):
    drefs, dcur = dev_frames()
    # bi list: valid, invalid, valid, invalid, ...
    good = T.bi_cases_p()
    mix = []
    for k, bad_case in enumerate(invalid_bi()):
        mix += [good[k % len(good)], bad_case]
    mix.append(good[0])
    cus, preds = i32([m[0] for m in mix]), pred_rows(*[P for m in mix for P in m[1:]])
    valid = list(range(0, len(mix), 2))
    alone, apred = cus[valid].contiguous(), preds.reshape(-1, 2, 7)[valid].reshape(-1, 7).contiguous()
    for k in range(1, len(mix), 2):  # every invalid descriptor on its own sets bad
        _, c1, b1 = eng.affine_mc_p(cus[k:k + 1].contiguous(), preds[2 * k:2 * k + 2].contiguous(), drefs, LAM, cur=dcur,
                                    want_cost=True)
        assert int(b1) == 1 and int(c1) == 0, k
    wp, wc, wb = eng.affine_mc_p(alone, apred, drefs, LAM, cur=dcur, pred=blank(H, W), want_cost=True)
    gp, gc, gb = eng.affine_mc_p(cus, preds, drefs, LAM, cur=dcur, pred=blank(H, W), want_cost=True)
    torch.cuda.synchronize()
    assert int(wb) == 0 and int(gb) == 1 and torch.equal(gp, wp) and torch.equal(gc[valid], wc)
    assert (gc[1::2] == 0).all()
    wo, wc, _ = eng.bipred_refine_p(alone, apred, drefs, dcur, LAM, rounds=1)
    go, gc, gb = eng.bipred_refine_p(cus, preds, drefs, dcur, LAM, rounds=1)
    torch.cuda.synchronize()
    assert int(gb) == 1 and torch.equal(go[valid], wo) and torch.equal(gc[valid], wc)
    assert torch.equal(go[1::2], cus[1::2]) and (gc[1::2] == 0).all()  # copied through, cost 0
    # uni list for the search
    good = T.search_cases_p()
    mix = []
    for k, bad_case in enumerate(invalid_uni()):
        mix += [good[k], bad_case]
    mix.append(good[-1])
    cus, preds = i32([m[0] for m in mix]), pred_rows(*[m[1] for m in mix])
    valid = list(range(0, len(mix), 2))
    for k in range(1, len(mix), 2):
        _, c1, b1 = eng.affine_search_p(cus[k:k + 1].contiguous(), preds[k:k + 1].contiguous(), drefs, dcur, LAM)
        assert int(b1) == 1 and int(c1) == 0, k
    wo, wc, _ = eng.affine_search_p(cus[valid].contiguous(), preds[valid].contiguous(), drefs, dcur, LAM)
    go, gc, gb = eng.affine_search_p(cus, preds, drefs, dcur, LAM)
    torch.cuda.synchronize()
    assert int(gb) == 1 and torch.equal(go[valid], wo) and torch.equal(gc[valid], wc)
    assert torch.equal(go[1::2], cus[1::2]) and (gc[1::2] == 0).all()


def test_device_count_and_in_place(eng):
    drefs, dcur = dev_frames()
    cus, preds = bi_inputs()
    cus12, p12 = search_inputs()
    n, n12 = cus.shape[0], cus12.shape[0]
    garbage = torch.full((3, 20), 1 << 20, dtype=torch.int32).cuda()
    gp = torch.full((6, 7), 1 << 20, dtype=torch.int32).cuda()
    count = torch.tensor(4, dtype=torch.int32).cuda()
    # affine_mc_p: costs past the count keep their value (the Engine allocates them: check through the C call)
    from vame._lib import lib
    ptrs = (P_ * 2)(*[r.data_ptr() for r in drefs])
    big, bigp = torch.cat([cus, garbage]), torch.cat([preds, gp])
    cost = torch.full((n + 3,), SENTINEL, dtype=torch.int64).cuda()
    bad = torch.zeros((), dtype=torch.int32).cuda()
    nd = torch.tensor(n, dtype=torch.int32).cuda()
    assert lib().vame_affine_mc_bi_p(eng._h, P_(dcur.data_ptr()), ptrs, 2, P_(big.data_ptr()), P_(bigp.data_ptr()), n + 3,
                                     P_(nd.data_ptr()), LAM, None, P_(cost.data_ptr()), P_(bad.data_ptr()), None) == 0
    _, wc, _ = eng.affine_mc_p(cus, preds, drefs, LAM, cur=dcur, want_cost=True)
    torch.cuda.synchronize()
    assert int(bad) == 0 and torch.equal(cost[:n], wc) and (cost[n:] == SENTINEL).all()
    # bipred_refine_p: count 4 of a list with garbage past it, out == cus
    wo, wc, _ = eng.bipred_refine_p(cus, preds, drefs, dcur, LAM, rounds=1)
    same = big.clone()
    cost = torch.full((n + 3,), SENTINEL, dtype=torch.int64).cuda()
    o, c, bad = eng.bipred_refine_p(same, bigp, drefs, dcur, LAM, rounds=1, count=count, out=same, cost=cost)
    torch.cuda.synchronize()
    assert o is same and int(bad) == 0 and torch.equal(same[:4], wo[:4]) and torch.equal(same[4:], big[4:])
    assert torch.equal(c[:4], wc[:4]) and (c[4:] == SENTINEL).all()
    # affine_search_p the same
    wo, wc, _ = eng.affine_search_p(cus12, p12, drefs, dcur, LAM)
    big12, bigp12 = torch.cat([cus12, garbage[:, :12]]), torch.cat([p12, gp[:3]])
    same = big12.clone()
    cost = torch.full((n12 + 3,), SENTINEL, dtype=torch.int64).cuda()
    o, c, bad = eng.affine_search_p(same, bigp12, drefs, dcur, LAM, ncus=count, out=same, cost=cost)
    torch.cuda.synchronize()
    assert o is same and int(bad) == 0 and torch.equal(same[:4], wo[:4]) and torch.equal(same[4:], big12[4:])
    assert torch.equal(c[:4], wc[:4]) and (c[4:] == SENTINEL).all()


# ------------------------------------------------------------------ 3. the row-layout calls
@functools.lru_cache(maxsize=None)
def poc_case():
    """The shifted-camera POC with three references, searched (modes 3), its
    seeds at radius 16, region predictors, and the chain reprice ->
    affine_me_seeded_p -> bipred_p, on the device, computed once."""
    from vame.engine import Engine
    e = Engine(W, H, 0)
    try:
        drefs, dcur = dev_frames(3)
        base = e.affine_me_poc(dcur, drefs, LAM, modes=3)
        seeds = e.seed_search(dcur, drefs, LAM, radius=16)["mv"]
        mvp = MVP.region_predictors(W, H, seeds, 64)
        priced, bad1 = e.reprice(LAM, clone_result(base), mvp)
        res, bad2 = e.affine_me_seeded_p(dcur, drefs, LAM, clone_result(priced), seeds, mvp, modes=3)
        bi = e.bipred_p(dcur, drefs, LAM, res, mvp)
        torch.cuda.synchronize()
        assert int(bad1) == 0 and int(bad2) == 0
        return base, seeds, mvp, priced, res, bi
    finally:
        e.close()


def test_region_predictors_against_reference():
    base, seeds, mvp, *_ = poc_case()
    want = R.region_predictors(W, H, {k: v.cpu().numpy() for k, v in seeds.items()}, 64)
    assert set(mvp) == set(want)
    for k in want:
        assert mvp[k].dtype == torch.int32 and np.array_equal(mvp[k].cpu().numpy(), want[k]), k
    # the rows of the cut CTU row fall back to 32 and 16
    full = {(x, y, w): row for row, x, y, w, h in B.frame_candidates(W, H, 0) if w == h}
    s0 = seeds[(0, 0)].cpu().numpy()
    c = next(c for c in B.frame_candidates(W, H, 1) if c[2] == 224 and c[1] < W)
    row = c[0]
    assert mvp[(0, 1)][row].tolist() == s0[full[(c[1] // 16 * 16, 224, 16)]].tolist()
    other = MVP.region_predictors(W, H, seeds, 32)
    assert np.array_equal(other[(1, 0)].cpu().numpy(),
                          R.region_predictors(W, H, {(1, 0): seeds[(1, 0)].cpu().numpy()}, 32)[(1, 0)])


def test_reprice_is_the_cost_of_the_prediction(eng):
    drefs, dcur = dev_frames(3)
    base, seeds, mvp, priced, *_ = poc_case()
    changed = 0
    for r in range(3):
        for m, name in enumerate(NAMES):
            align = m >> 1
            bc, bp = base[(r, name)]
            gc, gp = priced[(r, name)]
            assert torch.equal(gp, bp)  # CPMVs untouched
            cus, rows = M.cus_from_result(W, H, align, 2 + (m & 1), bp, ref=r)
            assert len(rows) == len(inframe(align))
            P = mvp[(r, align)][rows]
            preds = torch.cat([torch.full((len(rows), 1), 3, dtype=torch.int32).cuda(), P, P, P], 1).contiguous()
            _, want, bad = eng.affine_mc_p(cus, preds, drefs, LAM, cur=dcur, want_cost=True)
            _, zero, _ = eng.affine_mc(cus, drefs, LAM, cur=dcur, want_cost=True)
            torch.cuda.synchronize()
            assert int(bad) == 0 and torch.equal(zero, bc[rows])  # the search's cost is the zero-predictor cost
            assert torch.equal(gc[rows], want), (r, name)
            out = torch.ones_like(gc, dtype=torch.bool)
            out[rows] = False
            assert torch.equal(gc[out], bc[out])  # rows out of the frame unchanged
            changed += int((gc != bc).sum())
    assert changed > 5000
    # PREDs outside the mask are untouched; a second call prices twice
    got, bad = eng.reprice(LAM, clone_result(base), mvp, preds=0b0110)
    torch.cuda.synchronize()
    for (r, name), (c, p) in got.items():
        inside = name in ("FULL_3CP", "HALF_2CP")
        assert torch.equal(c, (priced if inside else base)[(r, name)][0]) and torch.equal(p, base[(r, name)][1])
    # a predictor out of range: the row is skipped, bad is set
    row = inframe(0)[40][0]
    odd = {k: v.clone() for k, v in mvp.items()}
    odd[(1, 0)][row] = torch.tensor([0, 1 << 17], dtype=torch.int32)
    got, bad = eng.reprice(LAM, clone_result(base), odd)
    torch.cuda.synchronize()
    assert int(bad) == 1
    for k in got:
        want = priced[k][0].clone()
        if k[0] == 1 and k[1].startswith("FULL"):
            want[row] = base[k][0][row]
        assert torch.equal(got[k][0], want), k
    # reprice_row on sampled rows
    for row, x, y, w, h in sample(1, 12, salt=9):
        for m in (2, 3):
            c, p = base[(2, NAMES[m])][0][row], base[(2, NAMES[m])][1][row].tolist()
            assert int(priced[(2, NAMES[m])][0][row]) == R.reprice_row(int(c), p[1:], p[0], R.expand(mvp[(2, 1)][row].tolist()), LAM)


def test_seeded_p_equals_the_composition_and_the_reference(eng):
    drefs, dcur = dev_frames(3)
    refs, cur = T.frames(3)
    base, seeds, mvp, priced, res, _ = poc_case()
    improved = 0
    for r in range(3):
        for align in (0, 1):
            cus, rows = V.cus_from_seeds(W, H, align, seeds[(r, align)], ref=r)
            P = mvp[(r, align)][rows]
            preds = torch.cat([torch.full((len(rows), 1), 3, dtype=torch.int32).cuda(), P, P, P], 1).contiguous()
            o2, c2, b2 = eng.affine_search_p(cus, preds, drefs, dcur, LAM)
            torch.cuda.synchronize()
            d2 = o2.cpu().numpy()
            start = [S.seed_3cp(d[6:10], int(d[0]), int(d[1]), int(d[2]), int(d[3]), W, H) for d in d2]
            cus3 = o2.clone()
            cus3[:, 5] = 3
            cus3[:, 6:] = torch.tensor(start, dtype=torch.int32).cuda()
            o3, c3, b3 = eng.affine_search_p(cus3, preds, drefs, dcur, LAM)
            torch.cuda.synchronize()
            assert int(b2) == 0 and int(b3) == 0
            for m, o, c in ((0, o2, c2), (1, o3, c3)):
                bc, bp = priced[(r, NAMES[2 * align + m])]
                wc, wp = bc.clone(), bp.clone()
                take = c < bc[rows]
                wc[rows[take]] = c[take]
                new = torch.cat([torch.full((len(rows), 1), 2 + m, dtype=torch.int32).cuda(), o[:, 6:]], 1)
                if m == 0:
                    new[:, 5:] = 0
                wp[rows[take]] = new[take]
                gc, gp = res[(r, NAMES[2 * align + m])]
                assert torch.equal(gc, wc) and torch.equal(gp, wp), (r, align, m)
                improved += int(take.sum())
    assert improved >= 3000
    # sampled rows against merged_p
    n = 0
    for align in (0, 1):
        b = {m: tuple(t.cpu().numpy() for t in priced[(1, NAMES[2 * align + m])]) for m in (0, 1)}
        g = {m: tuple(t.cpu().numpy() for t in res[(1, NAMES[2 * align + m])]) for m in (0, 1)}
        seed, pm = seeds[(1, align)].cpu().numpy(), mvp[(1, align)].cpu().numpy()
        for row, x, y, w, h in sample(align, 12, salt=5)[::2]:
            want = R.merged_p(refs[1], cur, x, y, w, h, tuple(seed[row].tolist()), R.expand(pm[row]), LAM,
                              (b[0][0][row], b[0][1][row][1:]), (b[1][0][row], b[1][1][row][1:]))
            for m in (0, 1):
                assert int(g[m][0][row]) == want[m][0] and g[m][1][row].tolist() == [2 + m] + want[m][1], (align, row, m)
            n += 1
    assert n >= 10
    # an all-zero mvp is affine_me_seeded
    zero = {k: torch.zeros_like(v) for k, v in mvp.items()}
    want, wbad = eng.affine_me_seeded(dcur, drefs, LAM, clone_result(base), seeds, modes=3)
    got, gbad = eng.affine_me_seeded_p(dcur, drefs, LAM, clone_result(base), seeds, zero, modes=3)
    torch.cuda.synchronize()
    assert int(wbad) == 0 and int(gbad) == 0
    for k in want:
        assert torch.equal(got[k][0], want[k][0]) and torch.equal(got[k][1], want[k][1]), k
    # a predictor out of range skips its row
    row = inframe(1)[30][0]
    odd = {k: v.clone() for k, v in mvp.items()}
    assert seeds[(2, 1)][row].tolist() != [0, 0]
    odd[(2, 1)][row] = torch.tensor([-(1 << 17) - 1, 0], dtype=torch.int32)
    got, gbad = eng.affine_me_seeded_p(dcur, drefs, LAM, clone_result(priced), seeds, odd, modes=3)
    torch.cuda.synchronize()
    assert int(gbad) == 1
    for k in res:
        c, p = res[k][0].clone(), res[k][1].clone()
        if k[0] == 2 and k[1].startswith("HALF"):
            c[row], p[row] = priced[k][0][row], priced[k][1][row]
        assert torch.equal(got[k][0], c) and torch.equal(got[k][1], p), k


def test_bipred_p_against_reference(eng):
    drefs, dcur = dev_frames(3)
    refs, cur = T.frames(3)
    base, seeds, mvp, priced, res, bi = poc_case()
    cost = {(r, m): res[(r, NAMES[m])][0].cpu().numpy() for r in range(3) for m in range(4)}
    cpmv = {(r, m): res[(r, NAMES[m])][1].cpu().numpy() for r in range(3) for m in range(4)}
    pm = {k: v.cpu().numpy() for k, v in mvp.items()}
    rows = {a: [c[0] for c in sample(a, 12, salt=11)] + [c[0] for c in B.frame_candidates(W, H, a) if c[2] + c[4] > H][:2]
            for a in (0, 1)}
    want = R.bipred_p(cur, refs, cost, cpmv, 15, LAM, pm, rows)
    plain = eng.bipred(dcur, drefs, LAM, res)
    torch.cuda.synchronize()
    for a in (0, 1):
        gc, gs = bi["cost"][a].cpu().numpy(), bi["sel"][a].cpu().numpy()
        for row in rows[a]:
            assert (int(gc[row]), int(gs[row])) == want[a][row], (a, row)
        outside = np.array([c[1] + c[3] > W or c[2] + c[4] > H for c in B.frame_candidates(W, H, a)])
        assert (gc[outside] == INF).all() and (gs[outside] == -1).all() and (gs[~outside] >= 0).all()
        assert not torch.equal(bi["cost"][a], plain["cost"][a])
    # one reference: every row INT64_MAX and -1
    one = {k: v for k, v in res.items() if k[0] == 0}
    got = eng.bipred_p(dcur, drefs[:1], LAM, one, mvp)
    torch.cuda.synchronize()
    for a in (0, 1):
        assert (got["cost"][a] == INF).all() and (got["sel"][a] == -1).all()
    # a predictor out of range: its row keeps INT64_MAX and -1, the others as before
    row = inframe(0)[17][0]
    odd = {k: v.clone() for k, v in mvp.items()}
    odd[(2, 0)][row] = torch.tensor([1 << 17, 0], dtype=torch.int32)
    got = eng.bipred_p(dcur, drefs, LAM, res, odd)
    torch.cuda.synchronize()
    wc, ws = bi["cost"][0].clone(), bi["sel"][0].clone()
    wc[row], ws[row] = INF, -1
    assert torch.equal(got["cost"][0], wc) and torch.equal(got["sel"][0], ws) and torch.equal(got["cost"][1], bi["cost"][1])


def host_leaf_predictors(cus, n, mvp):
    """The lookup of vame_mvp_gather on the host, through vame_partition_table."""
    table = PT.table()
    cols = (W + 127) // 128
    out = np.zeros((2 * len(cus), 7), np.int32)
    lg = {16: 0, 32: 1, 64: 2, 128: 3}
    for i in range(n):
        d = cus[i]
        x, y, w, h = (int(v) for v in d[:4])
        e = -1
        if w in lg and h in lg and x >= 0 and y >= 0 and x % 16 == 0 and y % 16 == 0 and x // 128 < cols:
            e = int(table[((lg[h] * 4 + lg[w]) * 8 + (y % 128) // 16) * 8 + (x % 128) // 16])
        ctu = (y // 128) * cols + x // 128
        for hyp, ref in enumerate((int(d[4]), int(d[12]) if len(d) > 12 else -1)):
            mv = [0, 0]
            if e >= 0 and (ref, e >> 9) in mvp and ctu < 8:
                mv = mvp[(ref, e >> 9)][ctu * (284 if e >> 9 else 201) + (e & 511)].tolist()
            out[2 * i + hyp] = [3] + mv * 3
    return out


def test_leaf_predictors_against_the_host_lookup(eng):
    base, seeds, mvp, priced, res, bi = poc_case()
    pm = {k: v.cpu().numpy() for k, v in mvp.items()}
    part = eng.partition(res, split_penalty=100)
    part_bi = eng.partition_bi(res, bi, split_penalty=100, bi_penalty=20)
    for p in (part, part_bi):
        got = eng.leaf_predictors(p, mvp)
        torch.cuda.synchronize()
        n = int(p["ncus"])
        want = host_leaf_predictors(p["cus"].cpu().numpy(), n, pm)
        assert n >= 8 and np.array_equal(got.cpu().numpy(), want)
        assert (want[:2 * n:2, 1:3] != 0).any()
    assert (part_bi["cus"][:int(part_bi["ncus"]), 12] >= 0).any()
    # descriptors that are no candidates get zero; a reference without an array too
    odd = i32([[8, 0, 16, 16, 0, 2] + [0] * 6 + [1, 2] + [0] * 6, [64, 64, 32, 32, 3, 2] + [0] * 6 + [0, 2] + [0] * 6,
               [0, 0, 128, 16, 0, 2] + [0] * 6 + [-1, 0] + [0] * 6, [400, 224, 16, 16, 2, 2] + [0] * 6 + [1, 2] + [0] * 6])
    fake = {"cus": odd, "ncus": torch.tensor(4, dtype=torch.int32).cuda()}
    got = eng.leaf_predictors(fake, mvp).cpu().numpy()
    torch.cuda.synchronize()
    assert np.array_equal(got, host_leaf_predictors(odd.cpu().numpy(), 4, pm))
    assert (got[0:3, 1:] == 0).all() and (got[:, 0] == 3).all()
    # a count below the capacity: rows past it keep their value
    out = torch.full((8, 7), SENTINEL, dtype=torch.int32).cuda()
    fake["ncus"] = torch.tensor(1, dtype=torch.int32).cuda()
    eng.leaf_predictors(fake, mvp, out=out)
    torch.cuda.synchronize()
    assert np.array_equal(out[:2].cpu().numpy(), got[:2]) and (out[2:] == SENTINEL).all()


# ------------------------------------------------------------------ 4. one graph
def test_the_chain_in_one_graph():
    """seeds -> reprice -> affine_me_seeded_p -> bipred_p -> partition_bi ->
    leaf_predictors -> bipred_refine_p -> affine_mc_p captured on a fresh
    engine (after the search), replayed after the inputs were overwritten:
    equal to direct calls on a second engine."""
    from vame.engine import Engine
    from test_gpu_bipred import load
    a = load("s416_noise")
    refs_np, cur_np = T.frames(2)
    eng, direct = Engine(W, H, 0), Engine(W, H, 0)

    def chain(e, cur, refs, res, pred):
        seeds = e.seed_search(cur, refs, LAM, radius=16)
        mvp = MVP.region_predictors(W, H, seeds["mv"], 64)
        _, b1 = e.reprice(LAM, res, mvp)
        _, b2 = e.affine_me_seeded_p(cur, refs, LAM, res, seeds["mv"], mvp, modes=3)
        bi = e.bipred_p(cur, refs, LAM, res, mvp)
        part = e.partition_bi(res, bi, split_penalty=100, bi_penalty=20)
        lp = e.leaf_predictors(part, mvp)
        cus, rcost, b3 = e.bipred_refine_p(part["cus"], lp, refs, cur, LAM, rounds=1, count=part["ncus"])
        _, cost, b4 = e.affine_mc_p(cus, lp, refs, LAM, cur=cur, pred=pred, want_cost=True, ncus=part["ncus"])
        return {"seeds": seeds, "mvp": mvp, "bi": bi, "part": part, "lp": lp, "cus": cus, "rcost": rcost, "cost": cost,
                "bad": [b1, b2, b3, b4]}
    try:
        cur, refs = dev(a["cur"]), [dev(a["ref"]), dev(np.roll(a["ref"], 2, 1))]
        res = eng.alloc_poc(2, 3)
        pred = blank(H, W)
        MVP.region_predictors(W, H, {(0, 0): torch.zeros((eng.n_cus(0), 2), dtype=torch.int32).cuda()}, 64)  # index built
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            eng.affine_me_poc(cur, refs, LAM, modes=3, out=res)
            got = chain(eng, cur, refs, res, pred)
        cur.copy_(dev(cur_np))
        refs[0].copy_(dev(refs_np[0]))
        refs[1].copy_(dev(refs_np[1]))
        pred.fill_(-1)
        for b in got["bad"]:
            b.fill_(5)
        g.replay()
        torch.cuda.synchronize()
        wres = direct.affine_me_poc(cur, refs, LAM, modes=3)
        wpred = blank(H, W)
        want = chain(direct, cur, refs, wres, wpred)
        torch.cuda.synchronize()
        n = int(want["part"]["ncus"])
        assert n >= 8 and int(got["part"]["ncus"]) == n
        assert all(int(b) == 0 for b in want["bad"]) and all(int(b) == 0 for b in got["bad"])
        for k in wres:
            assert torch.equal(res[k][0], wres[k][0]) and torch.equal(res[k][1], wres[k][1]), k
        for k in want["mvp"]:
            assert torch.equal(got["mvp"][k], want["mvp"][k])
        for k in ("cost", "sel"):
            for x in (0, 1):
                assert torch.equal(got["bi"][k][x], want["bi"][k][x]), (k, x)
        assert torch.equal(got["part"]["cus"][:n], want["part"]["cus"][:n])
        assert torch.equal(got["lp"][:2 * n], want["lp"][:2 * n]) and torch.equal(got["cus"][:n], want["cus"][:n])
        assert torch.equal(got["rcost"][:n], want["rcost"][:n]) and torch.equal(got["cost"][:n], want["cost"][:n])
        assert torch.equal(got["cost"][:n], got["rcost"][:n])  # the refinement's cost is affine_mc_p's of its out
        assert torch.equal(pred, wpred)
        assert (want["part"]["cus"][:n, 12] >= 0).any() and (want["lp"][:2 * n, 1:] != 0).any()
    finally:
        eng.close()
        direct.close()


# ------------------------------------------------------------------ 5. errors and PROF write nothing
def test_errors_and_prof_write_nothing(eng):
    from vame._lib import Mvp, PocResult, lib
    from vame.engine import Engine, _poc_result
    L = lib()
    drefs, dcur = dev_frames(2)
    ptrs = (P_ * 2)(*[r.data_ptr() for r in drefs])
    cus, preds = bi_inputs()
    cus12, p12 = search_inputs()
    n, n12 = cus.shape[0], cus12.shape[0]
    out = torch.full((n, 20), SENTINEL, dtype=torch.int32).cuda()
    out12 = torch.full((n12, 12), SENTINEL, dtype=torch.int32).cuda()
    cost = torch.full((max(n, n12),), SENTINEL, dtype=torch.int64).cuda()
    pred = torch.full((H, W), SENTINEL, dtype=torch.int16).cuda()
    bad = torch.zeros((), dtype=torch.int32).cuda()
    lp = torch.full((2 * n, 7), SENTINEL, dtype=torch.int32).cuda()
    res = {(r, name): (torch.full((eng.n_cus(m >> 1),), SENTINEL, dtype=torch.int64).cuda(),
                       torch.full((eng.n_cus(m >> 1), 7), SENTINEL, dtype=torch.int32).cuda())
           for r in (0, 1) for m, name in enumerate(NAMES)}
    pr = _poc_result(res)
    seeds = {(r, a): torch.full((eng.n_cus(a), 2), 16, dtype=torch.int32).cuda() for r in (0, 1) for a in (0, 1)}
    sp = ((P_ * 2) * 4)()
    mv = Mvp()
    for (r, a), t in seeds.items():
        sp[r][a] = t.data_ptr()
        mv.mv[r][a] = t.data_ptr()
    hole = Mvp()
    for (r, a), t in seeds.items():
        if (r, a) != (1, 1):
            hole.mv[r][a] = t.data_ptr()
    bi_c = [torch.full((eng.n_cus(a),), SENTINEL, dtype=torch.int64).cuda() for a in (0, 1)]
    bi_s = [torch.full((eng.n_cus(a),), SENTINEL, dtype=torch.int32).cuda() for a in (0, 1)]
    bic, bis = (P_ * 2)(*[t.data_ptr() for t in bi_c]), (P_ * 2)(*[t.data_ptr() for t in bi_s])
    wbytes = L.vame_seeded_p_work_bytes(eng._h, 2, 3)
    assert wbytes > L.vame_seeded_work_bytes(eng._h, 2, 3) > 0 and L.vame_seeded_p_work_bytes(eng._h, 2, 2) == 0
    work = torch.zeros((wbytes + 7) // 8, dtype=torch.int64).cuda()
    D = lambda t: P_(t.data_ptr())  # noqa: E731

    def mc(h=None, cur=D(dcur), refs=ptrs, nrefs=2, c=D(cus), p=D(preds), k=n, o=D(pred), co=D(cost), b=D(bad)):
        return L.vame_affine_mc_bi_p(h or eng._h, cur, refs, nrefs, c, p, k, None, LAM, o, co, b, None)

    def search(h=None, cur=D(dcur), refs=ptrs, nrefs=2, c=D(cus12), p=D(p12), k=n12, extra=0, o=D(out12), co=D(cost), b=D(bad)):
        return L.vame_affine_search_p(h or eng._h, cur, refs, nrefs, c, p, k, None, LAM, extra, o, co, b, None)

    def refine(h=None, cur=D(dcur), refs=ptrs, nrefs=2, c=D(cus), p=D(preds), k=n, rounds=1, o=D(out), co=D(cost), b=D(bad)):
        return L.vame_bipred_refine_p(h or eng._h, cur, refs, nrefs, c, p, k, None, LAM, rounds, o, co, b, None)

    def reprice(h=None, nrefs=2, mask=15, m=mv, r=pr, b=D(bad)):
        return L.vame_reprice(h or eng._h, nrefs, LAM, mask, ctypes.byref(m) if m else None,
                              ctypes.byref(r) if r else None, b, None)

    def seeded(h=None, cur=D(dcur), refs=ptrs, nrefs=2, modes=3, extra=0, s=sp, m=mv, r=pr, w=D(work), wb=None, b=D(bad)):
        return L.vame_affine_me_seeded_p(h or eng._h, cur, refs, nrefs, LAM, modes, extra, s, ctypes.byref(m) if m else None,
                                         ctypes.byref(r) if r else None, w, work.numel() * 8 if wb is None else wb, b, None)

    def bipred(h=None, cur=D(dcur), refs=ptrs, nrefs=2, mask=15, m=mv, r=pr, c=bic, s=bis):
        return L.vame_bipred_p(h or eng._h, cur, refs, nrefs, LAM, ctypes.byref(r) if r else None, mask,
                               ctypes.byref(m) if m else None, c, s, None)

    def gather(h=None, m=mv, c=D(cus), k=n, o=D(lp)):
        return L.vame_mvp_gather(h or eng._h, ctypes.byref(m) if m else None, c, k, None, o, None)

    def untouched():
        torch.cuda.synchronize()
        ts = [out, out12, cost, pred, lp] + bi_c + bi_s + [t for pair in res.values() for t in pair]
        return all(bool((t == SENTINEL).all()) for t in ts) and int(bad) == 0

    odd = P_(dcur.data_ptr() + 2)
    INVALID = -1
    null_pr = PocResult()
    for call, kws in ((mc, [dict(nrefs=0), dict(nrefs=5), dict(refs=None), dict(c=None), dict(b=None), dict(k=-1),
                            dict(k=(1 << 20) + 1), dict(o=None, co=None), dict(cur=None), dict(cur=odd)]),
                      (search, [dict(nrefs=0), dict(cur=None), dict(refs=None), dict(c=None), dict(o=None), dict(co=None),
                                dict(b=None), dict(extra=65), dict(extra=-1), dict(k=-1), dict(cur=odd)]),
                      (refine, [dict(nrefs=5), dict(cur=None), dict(c=None), dict(o=None), dict(co=None), dict(b=None),
                                dict(rounds=5), dict(rounds=-1), dict(k=(1 << 20) + 1), dict(cur=odd)]),
                      (reprice, [dict(nrefs=0), dict(nrefs=5), dict(mask=0), dict(mask=16), dict(m=None), dict(r=None),
                                 dict(b=None), dict(m=hole), dict(r=null_pr)]),
                      (seeded, [dict(nrefs=0), dict(cur=None), dict(modes=2), dict(modes=16), dict(extra=65), dict(m=None),
                                dict(m=hole), dict(r=None), dict(w=None), dict(wb=wbytes - 8), dict(b=None), dict(cur=odd),
                                dict(s=None)]),
                      (bipred, [dict(nrefs=0), dict(cur=None), dict(mask=0), dict(mask=16), dict(m=None), dict(m=hole),
                                dict(r=None), dict(c=None), dict(s=None), dict(cur=odd)]),
                      (gather, [dict(m=None), dict(c=None), dict(o=None), dict(k=-1), dict(k=(1 << 20) + 1)])):
        for kw in kws:
            assert call(**kw) == INVALID, (call.__name__, kw)
            assert untouched(), (call.__name__, kw)
    # the seeded call's plain work size is too small for the _p call
    assert seeded(wb=L.vame_seeded_work_bytes(eng._h, 2, 3)) == INVALID and untouched()
    # PROF on: unsupported, nothing written (reprice and gather make no prediction: PROF does not enter)
    e = Engine(W, H, 0)
    try:
        e.set_prof(True)
        for call in (mc, search, refine, seeded, bipred):
            assert call(h=e._h) == -4 and untouched(), call.__name__
    finally:
        e.close()
    # the Engine's own checks
    with pytest.raises(ValueError):
        eng.affine_mc_p(cus, preds[:-1].contiguous(), drefs, LAM, cur=dcur, want_cost=True)
    with pytest.raises(ValueError):
        eng.affine_search_p(cus12, preds, drefs, dcur, LAM)
    with pytest.raises(ValueError):
        eng.bipred_refine_p(cus, preds.to(torch.int64), drefs, dcur, LAM)
    with pytest.raises(ValueError):
        eng.reprice(LAM, res, {k: v for k, v in seeds.items() if k != (0, 1)})
    with pytest.raises(ValueError):
        MVP.region_predictors(W, H, seeds, 48)


def test_two_calls_agree(eng):
    drefs, dcur = dev_frames(3)
    base, seeds, mvp, priced, res, bi = poc_case()
    p2, _ = eng.reprice(LAM, clone_result(base), mvp)
    r2, _ = eng.affine_me_seeded_p(dcur, drefs, LAM, clone_result(p2), seeds, mvp, modes=3)
    b2 = eng.bipred_p(dcur, drefs, LAM, r2, mvp)
    torch.cuda.synchronize()
    for k in res:
        assert torch.equal(p2[k][0], priced[k][0]) and torch.equal(r2[k][0], res[k][0]) and torch.equal(r2[k][1], res[k][1])
    for a in (0, 1):
        assert torch.equal(b2["cost"][a], bi["cost"][a]) and torch.equal(b2["sel"][a], bi["sel"][a])
    cus, preds = bi_inputs()
    a = eng.bipred_refine_p(cus, preds, drefs[:2], dcur, LAM, rounds=2)
    b = eng.bipred_refine_p(cus, preds, drefs[:2], dcur, LAM, rounds=2)
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
