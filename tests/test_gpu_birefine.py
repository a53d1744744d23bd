"""Refinement of bi-predicted CUs on the GPU (Engine.bipred_refine,
Engine.refine_partition, Engine.refine_bipred): refined descriptors and costs
bit for bit against the CPU restatement tests/birefine_ref.py, 416x240
throughout."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import bipred_ref as B
import birefine_ref as F
from test_birefine import PINNED, poc2_desc, poc2_inputs
from test_gpu_bipred import SENTINEL, blank, dev, load, poc2, result_dict
from vame import bipred as V

pytestmark = pytest.mark.gpu

W, H = 416, 240
MV_MAX, MV_MIN = (1 << 17) - 1, -(1 << 17)
P_ = ctypes.c_void_p


@pytest.fixture(scope="module")
def eng():
    from vame.engine import Engine
    e = Engine(W, H, 0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def frames():
    refs, cur, lam, _, _ = poc2_inputs()
    return [dev(r) for r in refs], dev(cur), lam


# ------------------------------------------------------------------ 1. against the reference
def cases():
    """About 40 descriptors on the poc2 fixtures: every size and the four
    (moving, fixed) model combinations from the fixtures' own hypotheses (CUs
    on each frame edge among them), ref0 == ref1, large CPMVs (clip_mv and the
    window clamp act), components at the +-2^17 limit, a spread CU and
    positions off the 16-sample grid."""
    out = [poc2_desc(row, geo) for row, (geo, _, _, _) in PINNED.items()]
    for row, geo in ((696, (384, 80, 32, 16)), (403, (256, 0, 128, 64)), (436, (288, 64, 32, 32)),
                     (138, (16, 0, 16, 16)), (1240, (288, 192, 32, 32))):
        out.append(poc2_desc(row, geo))
    sizes = {(d[2], d[3]) for d in out}
    assert {(16, 16), (32, 32), (64, 64), (128, 128), (64, 16), (16, 64), (128, 64), (64, 128), (32, 16),
            (16, 32), (64, 32), (32, 64)} <= sizes
    assert {(d[5], d[13]) for d in out} == {(2, 2), (2, 3), (3, 2), (3, 3)}
    assert any(d[0] == 0 for d in out) and any(d[1] == 0 for d in out)            # left, top
    assert any(d[0] + d[2] == W for d in out) and any(d[1] + d[3] == H for d in out)  # right, bottom
    h0 = poc2_desc(182, (80, 80, 16, 16))
    out.append(h0[:12] + [0, 2, 0, 0, 0, 0, 0, 0])                                  # ref0 == ref1 == 0
    h1 = poc2_desc(436, (288, 64, 32, 32))
    out.append(h1[:4] + [1] + h1[13:20] + [1, 3, 0, 0, 0, 0, 0, 0])                # ref0 == ref1 == 1, a 3-CP zero
    same = poc2_desc(208, (128, 64, 64, 64))
    out.append(same[:12] + same[4:12])                                            # ref0 == ref1, equal CPMVs
    # large CPMVs: beyond clip_mv's bounds at the frame's corners, windows wholly outside the frame
    out.append([0, 0, 32, 32, 0, 2, -2500, -2400, -2480, -2390, 0, 0, 1, 3, -2300, -2300, -2290, -2310, -2305, -2280])
    out.append([384, 208, 32, 32, 0, 3, 900, 700, 910, 690, 905, 720, 1, 2, 800, 600, 805, 598, 0, 0])
    out.append([0, 176, 64, 64, 1, 2, -2400, 1500, -2390, 1490, 0, 0, 0, 2, 30, -20, 34, -18, 0, 0])
    out.append([288, 0, 128, 64, 0, 2, 2300, -2300, 2310, -2290, 0, 0, 1, 3, 12, 3, 10, 5, 14, 2])
    # components at the limits of the range
    out.append([160, 96, 16, 16, 0, 2, MV_MIN, MV_MAX, MV_MIN, MV_MAX, 0, 0, 1, 2, 5, 5, 6, 4, 0, 0])
    out.append([176, 96, 32, 32, 0, 3, 10, 10, 12, 9, MV_MAX, MV_MIN, 1, 2, -7, 3, -6, 2, 0, 0])
    out.append([208, 96, 16, 32, 1, 2, 3, -2, 4, -1, 0, 0, 0, 3, MV_MAX, 0, MV_MAX, 4, MV_MAX, -4])
    # a spread hypothesis (fixed in round 0, moving in round 1)
    out.append([128, 128, 16, 16, 0, 3, 0, 0, 4000, 0, 0, 4000, 1, 2, 3, 1, 2, 2, 0, 0])
    # positions that are multiples of 4 only; a 2-CP hypothesis with a non-zero LB (kept as it is)
    rng = np.random.default_rng(14)
    for x, y, w, h, n0, n1 in ((20, 36, 16, 16, 2, 3), (100, 52, 32, 16, 3, 2), (244, 132, 16, 32, 2, 2),
                               (332, 172, 64, 64, 3, 3), (4, 108, 128, 128, 2, 2)):
        c0, c1 = rng.integers(-60, 61, 6).tolist(), rng.integers(-60, 61, 6).tolist()
        out.append([x, y, w, h, 1, n0] + c0 + [0, n1] + c1)
    return out


@functools.lru_cache(maxsize=None)
def case_traces():
    """The reference after 0..3 rounds of every case, computed once."""
    refs, cur, lam, _, _ = poc2_inputs()
    return [F.refine_bicu_trace(refs, cur, d, lam, 3) for d in cases()]


def want_arrays(traces, rounds):
    return (np.array([t[rounds][0] for t in traces], np.int32), np.array([t[rounds][1] for t in traces], np.int64))


def test_the_cases_cover_what_they_should():
    cs, traces = cases(), case_traces()
    assert 38 <= len(cs) <= 45
    moved = [t[3][0] != t[0][0] for t in traces]
    assert sum(moved) >= 20
    # the clamps act: a refined component on clip_mv's bound, one at the range's end
    big = traces[[c[:4] for c in cs].index([0, 0, 32, 32])]
    assert min(big[0][0][6:10]) < -135 * 16  # given beyond the bound
    lim = traces[[c[:4] for c in cs].index([160, 96, 16, 16])]
    assert lim[0][0][6] == MV_MIN and lim[0][0][7] == MV_MAX


@pytest.mark.parametrize("rounds", [0, 1, 2, 3])
def test_against_reference(eng, rounds):
    drefs, dcur, lam = frames()
    cus = torch.tensor(cases(), dtype=torch.int32).cuda()
    out, cost, bad = eng.bipred_refine(cus, drefs, dcur, lam, rounds)
    torch.cuda.synchronize()
    want_out, want_cost = want_arrays(case_traces(), rounds)
    assert int(bad) == 0
    got_out, got_cost = out.cpu().numpy(), cost.cpu().numpy()
    for i in range(len(want_cost)):
        assert got_out[i].tolist() == want_out[i].tolist() and got_cost[i] == want_cost[i], \
            (i, cases()[i], got_out[i].tolist(), want_out[i].tolist(), int(got_cost[i]), int(want_cost[i]))
    if rounds == 0:
        assert torch.equal(out, cus)


def test_flat_frames(eng):
    z = load("s416_flat")
    flat, cur, lam = dev(z["ref"]), dev(z["cur"]), float(z["lam"])
    ds = []
    for geo in ((0, 0, 16, 16), (64, 64, 64, 64), (288, 112, 128, 128), (128, 0, 128, 64)):
        for n0, n1 in ((2, 3), (3, 2)):
            ds.append(list(geo) + [0, n0, 5, -3, 9, 2, 7 * (n0 - 2), -4 * (n0 - 2), 1, n1, -6, 8, -2, 11, 3 * (n1 - 2), 0])
    cus = torch.tensor(ds, dtype=torch.int32).cuda()
    out, cost, bad = eng.bipred_refine(cus, [flat, flat], cur, lam, 2)
    torch.cuda.synchronize()
    assert int(bad) == 0 and torch.equal(out, cus)
    want = [F.refine_bicu(np.stack([z["ref"]] * 2), z["cur"], d, lam, 2) for d in ds]
    assert [w[0] for w in want] == ds and cost.tolist() == [w[1] for w in want]


# ------------------------------------------------------------------ 2. bookkeeping
def raw_refine(eng, cus, count, rounds, out, cost, bad, nrefs=2, h=None, null=()):
    drefs, dcur, lam = frames()
    ptrs = (P_ * 2)(*[r.data_ptr() for r in drefs])
    ncus = None if count is None else torch.tensor(count, dtype=torch.int32).cuda()
    arg = {"cur": P_(dcur.data_ptr()), "refs": ptrs, "cus": P_(cus.data_ptr()), "out": P_(out.data_ptr()),
           "cost": P_(cost.data_ptr()), "bad": P_(bad.data_ptr())}
    for k in null:
        arg[k] = None
    from vame._lib import lib
    rc = lib().vame_bipred_refine(h or eng._h, arg["cur"], arg["refs"], nrefs, arg["cus"], cus.shape[0],
                                  None if ncus is None else P_(ncus.data_ptr()), lam, rounds, arg["out"], arg["cost"],
                                  arg["bad"], None)
    torch.cuda.synchronize()
    return rc


def sentinels(n):
    return (torch.full((n, 20), SENTINEL, dtype=torch.int32).cuda(), torch.full((n,), SENTINEL, dtype=torch.int64).cuda(),
            torch.zeros((), dtype=torch.int32).cuda())


def test_uni_and_invalid_descriptors(eng):
    drefs, dcur, lam = frames()
    cs = cases()
    bi = [cs[1], cs[7], cs[13]]
    uni = [c[:12] + [-1] + [1 << 30] * 7 for c in (cs[0], cs[9], cs[16])]  # cp1 is not read
    garbage = [-5, 3, 17, 9, 9, 7, 1 << 20, 0, 0, 0, 0, 0, 9, 7, 1 << 20, 0, 0, 0, 0, 0]
    half_bad = cs[4][:13] + [4] + cs[4][14:]  # nCPs1 = 4 alone
    mix = [bi[0], uni[0], garbage, bi[1], uni[1], half_bad, uni[2], bi[2]]
    cus = torch.tensor(mix, dtype=torch.int32).cuda()
    out, cost, bad = eng.bipred_refine(cus, drefs, dcur, lam, 2)
    torch.cuda.synchronize()
    assert int(bad) == 1
    # the valid ones as if alone
    alone = torch.tensor(bi, dtype=torch.int32).cuda()
    a_out, a_cost, a_bad = eng.bipred_refine(alone, drefs, dcur, lam, 2)
    _, u_cost, u_bad = eng.affine_mc(torch.tensor([u[:12] for u in uni], dtype=torch.int32).cuda(), drefs, lam,
                                     cur=dcur, want_cost=True)
    torch.cuda.synchronize()
    assert int(a_bad) == 0 and int(u_bad) == 0
    assert torch.equal(out[[0, 3, 7]], a_out) and torch.equal(cost[[0, 3, 7]], a_cost)
    assert (a_out != alone).any()
    assert torch.equal(out[[1, 4, 6]], cus[[1, 4, 6]]) and torch.equal(cost[[1, 4, 6]], u_cost)
    assert torch.equal(out[[2, 5]], cus[[2, 5]]) and cost[[2, 5]].tolist() == [0, 0]


def test_device_count_and_in_place(eng):
    cs = cases()
    pick = [cs[i] for i in (1, 3, 6, 9, 13, 16, 20, 22)]
    garbage = [[-5, 3, 17, 9, 9, 7, 1 << 20, 0, 0, 0, 0, 0, 9, 7, 1 << 20, 0, 0, 0, 0, 0]] * 4
    cus = torch.tensor(pick + garbage, dtype=torch.int32).cuda()
    drefs, dcur, lam = frames()
    w_out, w_cost, w_bad = eng.bipred_refine(cus[:8].contiguous(), drefs, dcur, lam, 2)
    torch.cuda.synchronize()
    assert int(w_bad) == 0
    # a count below the capacity, garbage past it: untouched entries, bad stays 0
    out, cost, bad = sentinels(12)
    assert raw_refine(eng, cus, 8, 2, out, cost, bad) == 0
    assert int(bad) == 0 and torch.equal(out[:8], w_out) and torch.equal(cost[:8], w_cost)
    assert (out[8:] == SENTINEL).all() and (cost[8:] == SENTINEL).all()
    # through Engine.bipred_refine(count=), into given arrays
    out, cost, _ = sentinels(12)
    o2, c2, bad = eng.bipred_refine(cus, drefs, dcur, lam, 2, count=torch.tensor(5, dtype=torch.int32).cuda(),
                                    out=out, cost=cost)
    torch.cuda.synchronize()
    assert o2 is out and c2 is cost and int(bad) == 0
    assert torch.equal(out[:5], w_out[:5]) and torch.equal(cost[:5], w_cost[:5])
    assert (out[5:] == SENTINEL).all() and (cost[5:] == SENTINEL).all()
    # count 0 and a negative count: nothing; above the capacity: the capacity; NULL: the capacity
    for count in (0, -3):
        out, cost, bad = sentinels(12)
        assert raw_refine(eng, cus, count, 2, out, cost, bad) == 0
        assert int(bad) == 0 and (out == SENTINEL).all() and (cost == SENTINEL).all()
    for count in (1000, None):
        out, cost, bad = sentinels(8)
        assert raw_refine(eng, cus[:8].contiguous(), count, 2, out, cost, bad) == 0
        assert int(bad) == 0 and torch.equal(out, w_out) and torch.equal(cost, w_cost)
    # an invalid descriptor below the count
    out, cost, bad = sentinels(12)
    assert raw_refine(eng, cus, 9, 2, out, cost, bad) == 0
    assert int(bad) == 1 and torch.equal(out[:8], w_out) and torch.equal(cost[:8], w_cost)
    assert torch.equal(out[8], cus[8]) and int(cost[8]) == 0 and (out[9:] == SENTINEL).all() and (cost[9:] == SENTINEL).all()
    # a few descriptors out of many: a grid sized for the capacity
    many = torch.tensor(pick * 200, dtype=torch.int32).cuda()
    out, cost, bad = sentinels(1600)
    assert raw_refine(eng, many, 3, 2, out, cost, bad) == 0
    assert torch.equal(out[:3], w_out[:3]) and (out[3:] == SENTINEL).all() and (cost[3:] == SENTINEL).all()
    # out is cus
    same = cus[:8].clone()
    o3, c3, bad = eng.bipred_refine(same, drefs, dcur, lam, 2, out=same)
    torch.cuda.synchronize()
    assert o3 is same and int(bad) == 0 and torch.equal(same, w_out) and torch.equal(c3, w_cost)
    assert (w_out != cus[:8]).any()
    with pytest.raises(ValueError):
        eng.bipred_refine(cus, drefs, dcur, lam, 2, count=torch.tensor(8).cuda())  # int64


# ------------------------------------------------------------------ 3. consistency
@pytest.mark.parametrize("rounds", [1, 4])
def test_cost_is_affine_mc_bi_of_the_result(eng, rounds):
    drefs, dcur, lam = frames()
    cus = torch.tensor(cases(), dtype=torch.int32).cuda()
    _, before, _ = eng.affine_mc_bi(cus, drefs, lam, cur=dcur, want_cost=True)
    out, cost, bad = eng.bipred_refine(cus, drefs, dcur, lam, rounds)
    _, after, bad2 = eng.affine_mc_bi(out, drefs, lam, cur=dcur, want_cost=True)
    torch.cuda.synchronize()
    assert int(bad) == 0 and int(bad2) == 0 and torch.equal(cost, after)
    assert (cost <= before).all() and (cost < before).any()


# ------------------------------------------------------------------ 4. errors write nothing
def test_errors_write_nothing(eng):
    from vame.engine import Engine
    drefs, dcur, lam = frames()
    cus = torch.tensor(cases()[:6], dtype=torch.int32).cuda()
    out, cost, bad = sentinels(6)

    def untouched():
        assert (out == SENTINEL).all() and (cost == SENTINEL).all() and int(bad) == 0

    assert raw_refine(eng, cus, None, 5, out, cost, bad) == -1 and raw_refine(eng, cus, None, -1, out, cost, bad) == -1
    assert raw_refine(eng, cus, None, 2, out, cost, bad, nrefs=0) == -1
    assert raw_refine(eng, cus, None, 2, out, cost, bad, nrefs=5) == -1
    for k in ("cur", "refs", "cus", "out", "cost", "bad"):
        assert raw_refine(eng, cus, None, 2, out, cost, bad, null=(k,)) == -1, k
    untouched()
    from vame._lib import lib
    ptrs = (P_ * 2)(*[r.data_ptr() for r in drefs])
    for n in (-1, (1 << 20) + 1):
        assert lib().vame_bipred_refine(eng._h, P_(dcur.data_ptr()), ptrs, 2, P_(cus.data_ptr()), n, None, lam, 2,
                                        P_(out.data_ptr()), P_(cost.data_ptr()), P_(bad.data_ptr()), None) == -1
    assert lib().vame_bipred_refine(eng._h, P_(dcur.data_ptr()), ptrs, 2, P_(cus.data_ptr()), 0, None, lam, 2,
                                    P_(out.data_ptr()), P_(cost.data_ptr()), P_(bad.data_ptr()), None) == 0  # a no-op
    torch.cuda.synchronize()
    untouched()
    # PROF on: unsupported, nothing written (an engine of its own)
    prof = Engine(W, H, 0)
    try:
        prof.set_prof(True)
        assert raw_refine(eng, cus, None, 2, out, cost, bad, h=prof._h) == -4
        untouched()
        with pytest.raises(Exception):
            prof.bipred_refine(cus, drefs, dcur, lam, 2)
        prof.set_prof(False)
        assert raw_refine(eng, cus, None, 2, out, cost, bad, h=prof._h) == 0
        assert (cost != SENTINEL).all() and int(bad) == 0
    finally:
        prof.close()
    # the Python layer refuses the same before any call
    for kw in (dict(rounds=5), dict(rounds=-1), dict(out=torch.empty((5, 20), dtype=torch.int32).cuda()),
               dict(cost=torch.empty(6, dtype=torch.int32).cuda())):
        with pytest.raises(ValueError):
            eng.bipred_refine(cus, drefs, dcur, lam, **kw)
    with pytest.raises(ValueError):
        eng.bipred_refine(cus[:, :12].contiguous(), drefs, dcur, lam)
    with pytest.raises(ValueError):
        eng.bipred_refine(cus, [], dcur, lam)
    with pytest.raises(ValueError):
        eng.refine_partition({"cus": cus[:, :12].contiguous(), "ncus": None}, drefs, dcur, lam)


# ------------------------------------------------------------------ 5. determinism
def test_two_calls_agree(eng):
    drefs, dcur, lam = frames()
    cus = torch.tensor(cases() * 8, dtype=torch.int32).cuda()
    a = eng.bipred_refine(cus, drefs, dcur, lam, 3)
    b = eng.bipred_refine(cus, drefs, dcur, lam, 3)
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and int(a[2]) == 0 and int(b[2]) == 0
    n = len(cases())
    assert torch.equal(a[0][:n], a[0][n:2 * n]) and torch.equal(a[1][:n], a[1][7 * n:])


# ------------------------------------------------------------------ 6. the chain
def test_chain_on_the_goldens(eng):
    """bipred -> refine_bipred -> partition_bi -> refine_partition ->
    predict_partition, penalties 0.  On the CPU (bipred_ref.partition_bi over
    birefine_ref's costs of every candidate with a pair) two rounds lower the
    ctu_cost of CTUs 1, 5 and 6 of this fixture and raise none."""
    g = poc2()
    drefs, dcur, lam = frames()
    res = result_dict(g["cost"], g["cpmv"])
    bi = eng.bipred(dcur, drefs, lam, res)
    keep = [[t.clone() for t in bi[k]] for k in ("cost", "sel")]
    rbi = eng.refine_bipred(dcur, drefs, lam, res, bi, rounds=2)
    plain = eng.partition_bi(res, bi)
    part = eng.partition_bi(res, rbi)
    rpart = eng.refine_partition(part, drefs, dcur, lam, rounds=2)
    pred, mc_cost, bad = eng.predict_partition(rpart, drefs, lam, cur=dcur, pred=blank(H, W), want_cost=True)
    torch.cuda.synchronize()
    # the input bi is not modified; sel is unchanged, costs never rise, and only rows with a pair change
    for a in (0, 1):
        assert torch.equal(bi["cost"][a], keep[0][a]) and torch.equal(bi["sel"][a], keep[1][a])
        assert torch.equal(rbi["sel"][a], bi["sel"][a]) and (rbi["cost"][a] <= bi["cost"][a]).all()
        assert (rbi["cost"][a] < bi["cost"][a]).any()
        rows = rbi["rows"][a].long()
        assert torch.equal(rows, torch.nonzero(bi["sel"][a] >= 0).reshape(-1))
        assert rbi["cus"][a].shape == (rows.numel(), 20)
        _, c, b2 = eng.affine_mc_bi(rbi["cus"][a], drefs, lam, cur=dcur, want_cost=True)
        torch.cuda.synchronize()
        assert int(b2) == 0 and torch.equal(c, rbi["cost"][a][rows])
        # a few of them against the reference
        sel = bi["sel"][a]
        for k in range(0, rows.numel(), max(1, rows.numel() // 6)):
            d = V.bicus_from_sel(W, H, a, res, sel, rows[k:k + 1])[0].tolist()
            want = F.refine_bicu(g["refs"], g["cur"], d, lam, 2)
            assert rbi["cus"][a][k].tolist() == want[0] and int(rbi["cost"][a][rows[k]]) == want[1], (a, k)
    n = int(part["ncus"])
    assert int(bad) == 0 and int(rpart["bad"]) == 0 and int(rpart["ncus"]) == n
    assert part["cus"] is not rpart["cus"] and (rpart["cus"][:n] != part["cus"][:n]).any()
    leaf = rpart["leaf_cost"].cpu().numpy()[:n]
    np.testing.assert_array_equal(mc_cost.cpu().numpy()[:n], leaf)
    info, ctu_cost = part["ctu_info"].cpu().numpy(), part["ctu_cost"].cpu().numpy()
    for ctu, (first, count, _, _) in enumerate(info):
        assert leaf[first:first + count].sum() == ctu_cost[ctu], ctu
    before = plain["ctu_cost"].cpu().numpy()
    assert (ctu_cost <= before).all() and (ctu_cost < before).any()
    assert (ctu_cost < before).tolist() == [False, True, False, False, False, True, True, False]
    frame = np.full((H, W), 0xFFFF, np.uint16)
    for d in rpart["cus"].cpu().numpy()[:n]:
        p, _ = B.predict_bicu(g["refs"], None, d)
        frame[d[1]:d[1] + d[3], d[0]:d[0] + d[2]] = p
    np.testing.assert_array_equal(pred.cpu().numpy().view(np.uint16), frame)


# ------------------------------------------------------------------ 7. one graph
def test_search_to_refined_prediction_in_one_graph():
    """search -> bipred -> partition_bi -> refine_partition ->
    predict_partition captured on a fresh engine, replayed after the inputs
    were overwritten: equal to direct calls on a second engine."""
    from vame.engine import Engine
    a, b = load("s416_noise"), load("s416_qp32_poc2_ref0")
    lam = float(b["lam"])
    eng, direct = Engine(W, H, 0), Engine(W, H, 0)
    try:
        cur, refs = dev(a["cur"]), [dev(a["ref"]), dev(np.roll(a["ref"], 2, 1))]
        res = eng.alloc_poc(2, 3)
        pred = blank(H, W)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            eng.affine_me_poc(cur, refs, lam, modes=3, out=res)
            bi = eng.bipred(cur, refs, lam, res)
            part = eng.partition_bi(res, bi, split_penalty=100, bi_penalty=20)
            rpart = eng.refine_partition(part, refs, cur, lam, rounds=2)
            _, cost, bad = eng.predict_partition(rpart, refs, lam, cur=cur, pred=pred, want_cost=True)
        cur.copy_(dev(b["cur"]))
        refs[0].copy_(dev(b["ref"]))
        refs[1].copy_(dev(load("s416_qp32_poc2_ref1")["ref"]))
        for t in [part[k] for k in V.KEYS] + [rpart["cus"], rpart["leaf_cost"], pred, cost]:
            t.fill_(-1)
        bad.fill_(5)
        rpart["bad"].fill_(5)
        g.replay()
        torch.cuda.synchronize()
        wres = direct.affine_me_poc(cur, refs, lam, modes=3)
        wbi = direct.bipred(cur, refs, lam, wres)
        wpart = direct.partition_bi(wres, wbi, split_penalty=100, bi_penalty=20)
        wrpart = direct.refine_partition(wpart, refs, cur, lam, rounds=2)
        wpred, wcost, wbad = direct.predict_partition(wrpart, refs, lam, cur=cur, pred=blank(H, W), want_cost=True)
        torch.cuda.synchronize()
        n = int(wpart["ncus"])
        assert n > 23 and int(part["ncus"]) == n and int(bad) == 0 and int(wbad) == 0 and int(rpart["bad"]) == 0
        assert torch.equal(part["cus"][:n], wpart["cus"][:n])
        assert torch.equal(rpart["cus"][:n], wrpart["cus"][:n])
        assert torch.equal(rpart["leaf_cost"][:n], wrpart["leaf_cost"][:n])
        assert (rpart["cus"][n:] == -1).all() and (rpart["leaf_cost"][n:] == -1).all() and (cost[n:] == -1).all()
        assert torch.equal(pred, wpred) and torch.equal(cost[:n], wcost[:n]) and torch.equal(cost[:n], rpart["leaf_cost"][:n])
        assert (wrpart["cus"][:n] != wpart["cus"][:n]).any()
    finally:
        eng.close()
        direct.close()
