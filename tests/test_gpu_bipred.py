"""Affine bi-prediction on the GPU (Engine.affine_mc_bi, Engine.bipred,
Engine.partition_bi, Engine.predict_partition on a bi partition): samples,
costs and every output array bit for bit against the numpy restatement
tests/bipred_ref.py."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import bipred_ref as B
from vame import bipred as V

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
NAMES = ("FULL_2CP", "FULL_3CP", "HALF_2CP", "HALF_3CP")
SENTINEL = -77
INF = B.INF
MV_MAX, MV_MIN = (1 << 17) - 1, -(1 << 17)


@functools.lru_cache(maxsize=None)
def load(name):
    return dict(np.load(os.path.join(GOLD, name + ".npz")))


@pytest.fixture(scope="module")
def engines():
    from vame.engine import Engine
    cache = {}

    def get(W, H):
        if (W, H) not in cache:
            cache[(W, H)] = Engine(W, H, 0)
        return cache[(W, H)]
    yield get
    for e in cache.values():
        e.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


def blank(H, W):
    return torch.full((H, W), -1, dtype=torch.int16, device="cuda")  # 0xFFFF


def result_dict(cost, cpmv, mask=15):
    """{(refIdx, PRED): arrays} -> an alloc_poc dict on the device."""
    out = {}
    for (r, m), c in cost.items():
        if not (mask >> m) & 1:
            continue
        p = np.asarray(cpmv[(r, m)], np.int32)
        if p.shape[1] == 6:
            p = np.concatenate([np.full((len(p), 1), 2 + (m & 1), np.int32), p], 1)
        out[(r, NAMES[m])] = (torch.from_numpy(np.ascontiguousarray(c, np.int64)).cuda(),
                              torch.from_numpy(np.ascontiguousarray(p)).cuda())
    return out


def result_arrays(res):
    """An alloc_poc dict on the device -> the reference's {(refIdx, PRED): array} pair."""
    cost = {(r, NAMES.index(n)): c.cpu().numpy() for (r, n), (c, _) in res.items()}
    cpmv = {(r, NAMES.index(n)): p.cpu().numpy() for (r, n), (_, p) in res.items()}
    return cost, cpmv


def bi_dict(bi):
    """The reference's {align: (cost, sel, ...)} -> Engine.partition_bi's bi argument."""
    return {"cost": [torch.from_numpy(np.array(bi[a][0])).cuda() if a in bi else None for a in (0, 1)],
            "sel": [torch.from_numpy(np.array(bi[a][1])).cuda() if a in bi else None for a in (0, 1)]}


# ------------------------------------------------------------------ the shared two-reference case
@functools.lru_cache(maxsize=None)
def poc2():
    """The two poc2 goldens (one POC, refIdx 0 and 1) and vame_bipred's
    reference on them, mask 15, computed once and left unchanged."""
    zs = [load("s416_qp32_poc2_ref0"), load("s416_qp32_poc2_ref1")]
    assert (zs[0]["cur"] == zs[1]["cur"]).all()
    cost = {(r, m): z[n + "_cost"] for r, z in enumerate(zs) for m, n in enumerate(NAMES)}
    cpmv = {(r, m): z[n + "_cpmv"] for r, z in enumerate(zs) for m, n in enumerate(NAMES)}
    refs, cur, lam = [z["ref"] for z in zs], zs[0]["cur"], float(zs[0]["lam"])
    want = B.bipred(cur, refs, cost, cpmv, 15, lam)
    for a in want:
        for t in want[a]:
            t.setflags(write=False)
    return {"cost": cost, "cpmv": cpmv, "refs": refs, "cur": cur, "lam": lam, "bi": want}


# ------------------------------------------------------------------ 1. uni descriptors
def test_uni_descriptors_equal_affine_mc(engines):
    from test_gpu_partition import mc_descs
    z = load("s416_noise")
    W, H, lam = 416, 240, float(z["lam"])
    eng = engines(W, H)
    refs, cur = [dev(z["ref"]), dev(np.roll(z["ref"], 3, 1))], dev(z["cur"])
    uni = torch.tensor(mc_descs(12, W, H), dtype=torch.int32).cuda()
    want_pred, want_cost, bad = eng.affine_mc(uni, refs, lam, cur=cur, pred=blank(H, W), want_cost=True)
    assert int(bad) == 0
    bi = torch.full((12, 20), 1 << 30, dtype=torch.int32).cuda()  # cp1 is not read
    bi[:, :12] = uni
    bi[:, 12] = -1
    pred, cost, bad = eng.affine_mc_bi(bi, refs, lam, cur=cur, pred=blank(H, W), want_cost=True)
    torch.cuda.synchronize()
    assert int(bad) == 0 and torch.equal(pred, want_pred) and torch.equal(cost, want_cost)
    assert (want_pred != -1).any()


# ------------------------------------------------------------------ 2. bi against the reference
def bi_cases():
    """Non-overlapping CUs at 416x240 over three references: the four sizes x
    the three model pairs, the frame's corners, ref0 == ref1, a spread CU and
    CPMVs at the ends of the range (the window clamps)."""
    rng = np.random.default_rng(9)

    def cp(ncp, big=90):
        v = rng.integers(-big, big + 1, 6).tolist()
        return [ncp] + (v if ncp == 3 else v[:4] + [0, 0])

    def d(x, y, w, h, r0, c0, r1, c1):
        return [x, y, w, h, r0] + c0 + [r1] + c1
    out = [d(0, 0, 128, 128, 0, cp(2), 1, cp(2)),          # top-left corner
           d(128, 0, 128, 128, 0, cp(2), 2, cp(3)),
           d(288, 112, 128, 128, 1, cp(3), 2, cp(3)),      # bottom-right corner
           d(400, 0, 16, 16, 0, cp(2), 1, cp(3)),          # top-right corner
           d(0, 224, 16, 16, 2, cp(3), 0, cp(3))]          # bottom-left corner
    for k, (n0, n1) in enumerate(((2, 2), (2, 3), (3, 3))):
        out.append(d(256, 16 * k, 64, 16, 0, cp(n0), 1, cp(n1)))
        out.append(d(16 * k, 128, 16, 64, 1, cp(n0), 2, cp(n1)))
        out.append(d(64 + 16 * k, 128, 16, 16, 2, cp(n0), 0, cp(n1)))
    same = cp(3)
    out.append(d(112, 128, 16, 16, 1, same, 1, same))                               # ref0 == ref1, equal CPMVs
    out.append(d(128, 128, 16, 16, 0, [3, 0, 0, 4000, 0, 0, 4000], 1, cp(2)))       # spread (hypothesis 0)
    out.append(d(144, 128, 16, 16, 0, [2, MV_MAX, MV_MAX, MV_MAX, MV_MAX, 0, 0], 1, cp(2)))
    out.append(d(160, 128, 16, 16, 0, cp(2), 1, [2, MV_MIN, MV_MIN, MV_MIN, MV_MIN, 0, 0]))
    out.append(d(64, 160, 32, 32, 2, [3, 5, -3, 9, 2, MV_MIN + 1, MV_MAX - 1], 0, cp(3)))
    return out


@functools.lru_cache(maxsize=None)
def bi_case_reference():
    z = load("s416_noise")
    refs = [z["ref"], np.roll(z["ref"], 3, 1), np.roll(z["ref"], -2, 0)]
    lams = (0.0, float(z["lam"]))
    cases = bi_cases()
    frame = np.full((240, 416), 0xFFFF, np.uint16)
    costs = {lam: [] for lam in lams}
    for c in cases:
        for lam in lams:
            p, v = B.predict_bicu(refs, z["cur"], c, lam)
            costs[lam].append(v)
        assert (frame[c[1]:c[1] + c[3], c[0]:c[0] + c[2]] == 0xFFFF).all(), "cases overlap"
        frame[c[1]:c[1] + c[3], c[0]:c[0] + c[2]] = p
    return refs, z["cur"], cases, frame, {lam: np.array(v, np.int64) for lam, v in costs.items()}


@pytest.mark.parametrize("lam_index", [0, 1], ids=["lam0", "lam"])
@pytest.mark.parametrize("outputs", ["pred", "cost", "both"])
def test_bi_against_reference(engines, outputs, lam_index):
    refs, cur, cases, frame, costs = bi_case_reference()
    lam = sorted(costs)[lam_index]
    eng = engines(416, 240)
    cus = torch.tensor(cases, dtype=torch.int32).cuda()
    want_pred, want_cost = outputs != "cost", outputs != "pred"
    pred, cost, bad = eng.affine_mc_bi(cus, [dev(r) for r in refs], lam, cur=dev(cur) if want_cost else None,
                                       pred=blank(240, 416) if want_pred else None, want_cost=want_cost)
    torch.cuda.synchronize()
    assert int(bad) == 0
    if want_pred:
        np.testing.assert_array_equal(pred.cpu().numpy().view(np.uint16), frame)
    if want_cost:
        np.testing.assert_array_equal(cost.cpu().numpy(), costs[lam])


def test_bi_special_cases_of_the_reference():
    """What the cases are meant to hold, asserted on the reference alone."""
    refs, cur, cases, frame, costs = bi_case_reference()
    same = next(c for c in cases if c[4] == c[12] and c[5:12] == c[13:20])
    uni, _ = B.predict_bicu(refs, None, same[:12] + [-1] + [0] * 7)
    np.testing.assert_array_equal(frame[same[1]:same[1] + 16, same[0]:same[0] + 16], uni)
    spread = next(c for c in cases if c[6:12] == [0, 0, 4000, 0, 0, 4000])
    assert B.acc_cu(refs[0], *spread[:4], 3, spread[6:12])[1]
    assert (costs[0.0] < costs[sorted(costs)[1]]).all()


# ------------------------------------------------------------------ 3. device count
def test_affine_mc_bi_device_count(engines):
    from vame._lib import lib
    refs, cur, cases, _, costs = bi_case_reference()
    lam = sorted(costs)[1]
    W, H = 416, 240
    eng = engines(W, H)
    drefs, dcur = [dev(r) for r in refs], dev(cur)
    valid = cases[3:11]
    garbage = [[-5, 3, 17, 9, 9, 7, 1 << 20, 0, 0, 0, 0, 0, 9, 7, 1 << 20, 0, 0, 0, 0, 0]] * 4  # invalid in every field
    cus = torch.tensor(valid + garbage, dtype=torch.int32).cuda()
    want_pred, want_cost, bad0 = eng.affine_mc_bi(cus[:8].contiguous(), drefs, lam, cur=dcur, pred=blank(H, W),
                                                  want_cost=True)
    torch.cuda.synchronize()
    assert int(bad0) == 0
    np.testing.assert_array_equal(want_cost.cpu().numpy(), costs[lam][3:11])
    V_ = ctypes.c_void_p

    def run(cus, count, pred):
        ncus = torch.tensor(count, dtype=torch.int32).cuda()
        cost = torch.full((cus.shape[0],), SENTINEL, dtype=torch.int64).cuda()
        bad = torch.zeros((), dtype=torch.int32).cuda()
        ptrs = (V_ * 3)(*[r.data_ptr() for r in drefs])
        rc = lib().vame_affine_mc_bi(eng._h, V_(dcur.data_ptr()), ptrs, 3, V_(cus.data_ptr()), cus.shape[0],
                                     V_(ncus.data_ptr()), lam, V_(pred.data_ptr()), V_(cost.data_ptr()),
                                     V_(bad.data_ptr()), None)
        torch.cuda.synchronize()
        assert rc == 0
        return cost, bad

    # count < capacity, garbage past it: bad stays 0, their cost and samples untouched
    pred = blank(H, W)
    cost, bad = run(cus, 8, pred)
    assert int(bad) == 0 and torch.equal(cost[:8], want_cost) and (cost[8:] == SENTINEL).all()
    assert torch.equal(pred, want_pred)
    # the same through Engine.affine_mc_bi(ncus=)
    pred = blank(H, W)
    _, cost, bad = eng.affine_mc_bi(cus, drefs, lam, cur=dcur, pred=pred, want_cost=True,
                                    ncus=torch.tensor(8, dtype=torch.int32).cuda())
    torch.cuda.synchronize()
    assert int(bad) == 0 and torch.equal(cost[:8], want_cost) and torch.equal(pred, want_pred)
    # count 0 and a negative count: nothing at all
    for count in (0, -3):
        pred = blank(H, W)
        cost, bad = run(cus, count, pred)
        assert int(bad) == 0 and (cost == SENTINEL).all() and (pred == -1).all()
    # count > capacity: the capacity
    pred = blank(H, W)
    cost, bad = run(cus[:8].contiguous(), 1000, pred)
    assert int(bad) == 0 and torch.equal(cost, want_cost) and torch.equal(pred, want_pred)
    # an invalid descriptor below the count sets bad, costs 0 and writes no sample
    pred = blank(H, W)
    cost, bad = run(cus, 9, pred)
    assert int(bad) == 1 and torch.equal(cost[:8], want_cost) and int(cost[8]) == 0 and (cost[9:] == SENTINEL).all()
    assert torch.equal(pred, want_pred)
    # invalid in the second hypothesis alone: ref1 = -2, ref1 = nrefs, nCPs1 = 4, a CPMV of hypothesis 1 out of range
    for col, val in ((12, -2), (12, 3), (13, 4), (16, MV_MAX + 1)):
        one = cus[:2].clone()
        one[1, col] = val
        pred = blank(H, W)
        cost, bad = run(one.contiguous(), 2, pred)
        only = blank(H, W)
        c0 = valid[0]
        only[c0[1]:c0[1] + c0[3], c0[0]:c0[0] + c0[2]] = want_pred[c0[1]:c0[1] + c0[3], c0[0]:c0[0] + c0[2]]
        assert int(bad) == 1 and int(cost[0]) == int(want_cost[0]) and int(cost[1]) == 0 and torch.equal(pred, only)
    # a count of a few descriptors out of many: a grid sized for the capacity
    many = torch.tensor(valid * 300, dtype=torch.int32).cuda()
    cost, bad = run(many, 3, blank(H, W))
    assert int(bad) == 0 and torch.equal(cost[:3], want_cost[:3]) and (cost[3:] == SENTINEL).all()
    # a NULL count: every descriptor
    cost = torch.full((8,), SENTINEL, dtype=torch.int64).cuda()
    bad = torch.zeros((), dtype=torch.int32).cuda()
    ptrs = (V_ * 3)(*[r.data_ptr() for r in drefs])
    first8 = cus[:8].contiguous()
    assert lib().vame_affine_mc_bi(eng._h, V_(dcur.data_ptr()), ptrs, 3, V_(first8.data_ptr()), 8, None, lam, None,
                                   V_(cost.data_ptr()), V_(bad.data_ptr()), None) == 0
    torch.cuda.synchronize()
    assert int(bad) == 0 and torch.equal(cost, want_cost)
    with pytest.raises(ValueError):
        eng.affine_mc_bi(cus, drefs, lam, cur=dcur, want_cost=True, ncus=torch.tensor(8).cuda())  # int64


# ------------------------------------------------------------------ 4. vame_bipred on the goldens
def test_bipred_on_two_reference_goldens(engines):
    g = poc2()
    want = g["bi"]
    # on the reference alone: bi wins for some in-frame rows and loses for others
    wins = sum(int(((bs >= 0) & (bc < um)).sum()) for bc, bs, um in want.values())
    loses = sum(int(((bs >= 0) & (bc >= um)).sum()) for bc, bs, um in want.values())
    assert wins > 0 and loses > 0
    aligned = want[0]
    assert int(((aligned[1] >= 0) & (aligned[0] < aligned[2])).sum()) > 0
    eng = engines(416, 240)
    res = result_dict(g["cost"], g["cpmv"])
    drefs, dcur = [dev(r) for r in g["refs"]], dev(g["cur"])
    out = {"cost": [torch.full((eng.n_cus(a),), SENTINEL, dtype=torch.int64).cuda() for a in (0, 1)],
           "sel": [torch.full((eng.n_cus(a),), SENTINEL, dtype=torch.int32).cuda() for a in (0, 1)]}
    bi = eng.bipred(dcur, drefs, g["lam"], res, preds=15, out=out)
    torch.cuda.synchronize()
    for a in (0, 1):
        np.testing.assert_array_equal(bi["cost"][a].cpu().numpy(), want[a][0], err_msg=f"cost {a}")
        np.testing.assert_array_equal(bi["sel"][a].cpu().numpy(), want[a][1], err_msg=f"sel {a}")
        assert (want[a][1] == -1).any() and ((want[a][1] == -1) == (want[a][0] == INF)).all()
    # identity: affine_mc_bi on the descriptors of 50 rows gives their bi_cost
    for a in (0, 1):
        rows = np.nonzero(want[a][1] >= 0)[0]
        rows = torch.from_numpy(rows[::max(1, len(rows) // 25)][:25].copy())
        cus = V.bicus_from_sel(416, 240, a, res, bi["sel"][a], rows)
        assert cus.shape == (25, 20)
        _, cost, bad = eng.affine_mc_bi(cus, drefs, g["lam"], cur=dcur, want_cost=True)
        torch.cuda.synchronize()
        assert int(bad) == 0 and torch.equal(cost, bi["cost"][a][rows.cuda()])


# ------------------------------------------------------------------ 5. four references
@functools.lru_cache(maxsize=None)
def four_refs():
    z = load("s416_qp32_poc2_ref0")
    ref = z["ref"]
    return [ref, np.roll(ref, (0, 3), (0, 1)), np.roll(ref, (2, 0), (0, 1)), np.roll(ref, (-1, -2), (0, 1))], \
        z["cur"], float(z["lam"])


def sample_rows(W, H):
    """Every 5th row of each alignment plus every 128-class row."""
    return {a: sorted({row for row, _, _, w, h in B.frame_candidates(W, H, a) if row % 5 == 0 or max(w, h) == 128})
            for a in (0, 1)}


def test_bipred_four_references(engines):
    refs, cur, lam = four_refs()
    eng = engines(416, 240)
    drefs, dcur = [dev(r) for r in refs], dev(cur)
    res = eng.affine_me_poc(dcur, drefs, lam, modes=3)
    torch.cuda.synchronize()
    cost, cpmv = result_arrays(res)
    rows = sample_rows(416, 240)
    chosen = set()
    for mask in (15, 5, 3):
        want = B.bipred(cur, refs, cost, cpmv, mask, lam, rows)
        sub = {k: v for k, v in res.items() if (mask >> NAMES.index(k[1])) & 1}
        bi = eng.bipred(dcur, drefs, lam, sub, preds=mask)
        torch.cuda.synchronize()
        for a in (0, 1):
            if a not in want:
                assert bi["cost"][a] is None and bi["sel"][a] is None  # mask 3: the HALF arrays are NULL
                continue
            r = np.array(rows[a])
            np.testing.assert_array_equal(bi["cost"][a].cpu().numpy()[r], want[a][0][r], err_msg=f"cost {mask} {a}")
            np.testing.assert_array_equal(bi["sel"][a].cpu().numpy()[r], want[a][1][r], err_msg=f"sel {mask} {a}")
            s = want[a][1][r]
            if mask == 15:
                chosen |= {(int(v) & 3, (int(v) >> 3) & 3) for v in s[s >= 0]}
            if mask == 5:
                assert ((s[s >= 0] & (4 | 32)) == 0).all()  # 2-CP hypotheses only
            # rows of CUs that leave the frame hold none
            got_sel = bi["sel"][a].cpu().numpy()
            outside = np.array([x + w > 416 or y + h > 240 for _, x, y, w, h in B.frame_candidates(416, 240, a)])
            assert (got_sel[outside] == -1).all() and (got_sel[~outside] >= 0).all()
            assert (bi["cost"][a].cpu().numpy()[outside] == INF).all()
    assert len(chosen) >= 2, chosen
    # one reference: no pair, every row none
    one = {k: v for k, v in res.items() if k[0] == 0}
    bi = eng.bipred(dcur, drefs[:1], lam, one)
    torch.cuda.synchronize()
    for a in (0, 1):
        assert (bi["cost"][a] == INF).all() and (bi["sel"][a] == -1).all()


# ------------------------------------------------------------------ 6. partition_bi
def sentinel_out(eng):
    out = V.alloc(eng.n_ctus, eng.device)
    for t in out.values():
        t.fill_(SENTINEL)
    return out


def run_partition_bi(eng, cost, cpmv, nrefs, mask, bi, penalty, bi_penalty):
    want = B.partition_bi(eng.W, eng.H, cost, cpmv, nrefs, mask, penalty, bi, bi_penalty)
    part = eng.partition_bi(result_dict(cost, cpmv, mask), bi_dict(bi), preds=mask, split_penalty=penalty,
                            bi_penalty=bi_penalty, out=sentinel_out(eng))
    torch.cuda.synchronize()
    n = int(part["ncus"])
    assert n == want["ncus"]
    for k in ("cus", "rows", "sel"):
        assert (part[k][n:] == SENTINEL).all(), k
    got = V.to_host(part)
    for k in V.KEYS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    return want, part


@pytest.mark.parametrize("penalty,bi_penalty", [(0, 0), (100, 0), (0, 500)])
def test_partition_bi_against_reference(engines, penalty, bi_penalty):
    g = poc2()
    want, _ = run_partition_bi(engines(416, 240), g["cost"], g["cpmv"], 2, 15, g["bi"], penalty, bi_penalty)
    if (penalty, bi_penalty) == (0, 0):
        assert (want["sel"] >= 0).any() and (want["sel"] < 0).any()
        assert ((want["cus"][:, 12] >= 0) == (want["sel"] >= 0)).all()


def test_partition_bi_with_a_huge_bi_penalty_is_partition(engines):
    from vame.partition import KEYS
    g = poc2()
    eng = engines(416, 240)
    res = result_dict(g["cost"], g["cpmv"])
    uni = eng.partition(res, preds=15, split_penalty=40)
    part = eng.partition_bi(res, bi_dict(g["bi"]), preds=15, split_penalty=40, bi_penalty=1 << 40,
                            out=sentinel_out(eng))
    torch.cuda.synchronize()
    n = int(uni["ncus"])
    assert int(part["ncus"]) == n
    for k in KEYS:
        a, b = part[k], uni[k]
        if k == "cus":
            a, b = a[:n, :12], b[:n]
        elif k == "rows":
            a, b = a[:n], b[:n]
        assert torch.equal(a, b), k
    assert (part["sel"][:n] == -1).all() and (part["cus"][:n, 12] == -1).all() and (part["cus"][:n, 13:] == 0).all()
    for k in ("cus", "rows", "sel"):
        assert (part[k][n:] == SENTINEL).all(), k


def test_partition_bi_at_832x480_on_a_gpu_search(engines):
    """Search, bipred and partition_bi on the GPU over two references; the
    decision equals the reference's on the downloaded arrays."""
    z = load("s832_qp37_poc1")
    W, H, lam = 832, 480, float(z["lam"])
    eng = engines(W, H)
    # the second reference: a shifted copy on the left half (uni leaves), the mirror image of the first
    # about `cur` on the right half (the average of the two is `cur` there: bi leaves)
    second = np.roll(z["ref"], (1, -2), (0, 1))
    mirror = np.clip(2 * z["cur"].astype(np.int32) - z["ref"], 0, 1023).astype(np.uint16)
    second[:, W // 2:] = mirror[:, W // 2:]
    refs = [z["ref"], second]
    drefs, dcur = [dev(r) for r in refs], dev(z["cur"])
    res = eng.affine_me_poc(dcur, drefs, lam, modes=3)
    bi = eng.bipred(dcur, drefs, lam, res)
    part = eng.partition_bi(res, bi, split_penalty=30, bi_penalty=10, out=sentinel_out(eng))
    torch.cuda.synchronize()
    cost, cpmv = result_arrays(res)
    hbi = {a: (bi["cost"][a].cpu().numpy(), bi["sel"][a].cpu().numpy()) for a in (0, 1)}
    want = B.partition_bi(W, H, cost, cpmv, 2, 15, 30, hbi, 10)
    got = V.to_host(part)
    assert (want["sel"] >= 0).any() and (want["sel"] < 0).any()
    for k in V.KEYS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert (part["cus"][want["ncus"]:] == SENTINEL).all()
    # and a few of its bi costs against the restatement
    rows = {a: [int(r) for r in np.nonzero(hbi[a][1] >= 0)[0][::397]] for a in (0, 1)}
    ref_bi = B.bipred(z["cur"], refs, cost, cpmv, 15, lam, rows)
    for a in (0, 1):
        np.testing.assert_array_equal(hbi[a][0][rows[a]], ref_bi[a][0][rows[a]])
        np.testing.assert_array_equal(hbi[a][1][rows[a]], ref_bi[a][1][rows[a]])


# ------------------------------------------------------------------ 7. pipeline identity
def test_pipeline_predicts_the_bi_partition(engines):
    g = poc2()
    W, H, lam = 416, 240, g["lam"]
    eng = engines(W, H)
    want, part = run_partition_bi(eng, g["cost"], g["cpmv"], 2, 15, g["bi"], 0, 0)
    drefs, dcur = [dev(r) for r in g["refs"]], dev(g["cur"])
    pred, mc_cost, bad = eng.predict_partition(part, drefs, lam, cur=dcur, pred=blank(H, W), want_cost=True)
    torch.cuda.synchronize()
    assert int(bad) == 0 and mc_cost.numel() == eng.n_ctus * 64
    frame = np.full((H, W), 0xFFFF, np.uint16)
    for d in want["cus"]:
        p, _ = B.predict_bicu(g["refs"], None, d)
        frame[d[1]:d[1] + d[3], d[0]:d[0] + d[2]] = p
    np.testing.assert_array_equal(pred.cpu().numpy().view(np.uint16), frame)
    # penalties 0, the fixture's lambda: a leaf's cost is its leaf value, their sum per CTU the root's value
    n = want["ncus"]
    got = mc_cost.cpu().numpy()[:n]
    np.testing.assert_array_equal(got, want["leaf_cost"])
    for ctu, (first, count, _, _) in enumerate(want["ctu_info"]):
        assert got[first:first + count].sum() == want["ctu_cost"][ctu]


# ------------------------------------------------------------------ 8. one graph
def test_search_bipred_partition_prediction_in_one_graph():
    """search -> bipred -> partition_bi -> predict_partition captured on a
    fresh engine, replayed after the inputs were overwritten: equal to direct
    calls on a second engine."""
    from vame.engine import Engine
    a, b = load("s416_noise"), load("s416_qp32_poc2_ref0")
    W, H, lam = 416, 240, float(b["lam"])
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
            _, cost, bad = eng.predict_partition(part, refs, lam, cur=cur, pred=pred, want_cost=True)
        cur.copy_(dev(b["cur"]))
        refs[0].copy_(dev(b["ref"]))
        refs[1].copy_(dev(load("s416_qp32_poc2_ref1")["ref"]))
        for t in list(part.values()) + bi["cost"] + bi["sel"] + [pred, cost]:
            t.fill_(-1)
        bad.fill_(5)
        g.replay()
        torch.cuda.synchronize()
        wres = direct.affine_me_poc(cur, refs, lam, modes=3)
        wbi = direct.bipred(cur, refs, lam, wres)
        wpart = direct.partition_bi(wres, wbi, split_penalty=100, bi_penalty=20)
        wpred, wcost, wbad = direct.predict_partition(wpart, refs, lam, cur=cur, pred=blank(H, W), want_cost=True)
        torch.cuda.synchronize()
        n = int(wpart["ncus"])
        assert n > 23 and int(part["ncus"]) == n and int(bad) == 0 and int(wbad) == 0
        for k in ("cost", "sel"):
            for x in (0, 1):
                assert torch.equal(bi[k][x], wbi[k][x]), (k, x)
        for k in V.KEYS:
            cut = n if k in ("cus", "rows", "sel") else None
            assert torch.equal(part[k][:cut] if cut else part[k], wpart[k][:cut] if cut else wpart[k]), k
        assert torch.equal(pred, wpred) and torch.equal(cost[:n], wcost[:n])
        assert (cost[n:] == -1).all() and (part["cus"][n:] == -1).all()
        assert (wpart["sel"][:n] >= 0).any()
        # the replayed search is the goldens' search: the chain equals the shared reference
        g2 = poc2()
        for x in (0, 1):
            np.testing.assert_array_equal(bi["cost"][x].cpu().numpy(), g2["bi"][x][0])
    finally:
        eng.close()
        direct.close()


# ------------------------------------------------------------------ 9. errors
def test_errors_write_nothing(engines):
    from vame._lib import PocResult, lib
    from vame.engine import Engine
    g = poc2()
    W, H = 416, 240
    eng = engines(W, H)
    res = result_dict(g["cost"], g["cpmv"])
    drefs, dcur = [dev(r) for r in g["refs"]], dev(g["cur"])
    bi_in = bi_dict(g["bi"])
    out = sentinel_out(eng)
    bi_out = {"cost": [torch.full((eng.n_cus(a),), SENTINEL, dtype=torch.int64).cuda() for a in (0, 1)],
              "sel": [torch.full((eng.n_cus(a),), SENTINEL, dtype=torch.int32).cuda() for a in (0, 1)]}
    mc_pred = blank(H, W)
    mc_cost = torch.full((4,), SENTINEL, dtype=torch.int64).cuda()
    mc_bad = torch.zeros((), dtype=torch.int32).cuda()
    mc_cus = torch.tensor([bi_cases()[i] for i in (3, 5, 8, 11)], dtype=torch.int32).cuda()  # refIdx 0 and 1 only
    P_ = ctypes.c_void_p

    def poc_result(drop=None):
        pr = PocResult()
        for (r, name), (c, p) in res.items():
            m = NAMES.index(name)
            if drop == (r, m):
                continue
            pr.cost[r][m] = c.data_ptr()
            pr.cpmvs[r][m] = p.data_ptr()
        return pr

    def pair(d, null=None):
        arr = (P_ * 2)()
        for a in (0, 1):
            if a != null:
                arr[a] = d[a].data_ptr()
        return arr

    def call_bipred(h=None, nrefs=2, mask=15, drop=None, null_cost=None, null_sel=None, cur=True):
        ptrs = (P_ * 2)(*[r.data_ptr() for r in drefs])
        return lib().vame_bipred(h or eng._h, P_(dcur.data_ptr()) if cur else None, ptrs, nrefs, g["lam"],
                                 ctypes.byref(poc_result(drop)), mask, pair(bi_out["cost"], null_cost),
                                 pair(bi_out["sel"], null_sel), None)

    def call_part(h=None, nrefs=2, mask=15, penalty=0, bi_penalty=0, drop=None, null_bi=None, cus=True, ncus=True):
        ptr = {k: P_(out[k].data_ptr()) for k in V.KEYS}
        return lib().vame_partition_bi(h or eng._h, ctypes.byref(poc_result(drop)), nrefs, mask, penalty,
                                       pair(bi_in["cost"], null_bi), pair(bi_in["sel"]), bi_penalty,
                                       ptr["cus"] if cus else None, ptr["rows"], ptr["sel"],
                                       ptr["ncus"] if ncus else None, ptr["ctu_info"], ptr["ctu_cost"],
                                       ptr["block_cu"], None)

    def call_mc(h=None, nrefs=2):
        ptrs = (P_ * 2)(*[r.data_ptr() for r in drefs])
        return lib().vame_affine_mc_bi(h or eng._h, P_(dcur.data_ptr()), ptrs, nrefs, P_(mc_cus.data_ptr()), 4, None,
                                       g["lam"], P_(mc_pred.data_ptr()), P_(mc_cost.data_ptr()),
                                       P_(mc_bad.data_ptr()), None)

    def untouched():
        torch.cuda.synchronize()
        assert all((t == SENTINEL).all() for t in out.values())
        assert all((t == SENTINEL).all() for t in bi_out["cost"] + bi_out["sel"])
        assert (mc_pred == -1).all() and (mc_cost == SENTINEL).all() and int(mc_bad) == 0

    # PROF on: unsupported, nothing written (an engine of its own: the shared ones stay PROF-off)
    prof = Engine(W, H, 0)
    try:
        prof.set_prof(True)
        assert call_bipred(h=prof._h) == -4 and call_part(h=prof._h) == -4 and call_mc(h=prof._h) == -4
        untouched()
        with pytest.raises(Exception):
            prof.bipred(dcur, drefs, g["lam"], res)
        prof.set_prof(False)
        assert call_mc(h=prof._h) == 0
        torch.cuda.synchronize()
        assert (mc_cost != SENTINEL).all() and int(mc_bad) == 0
        mc_pred.fill_(-1)
        mc_cost.fill_(SENTINEL)
    finally:
        prof.close()
    # argument errors
    assert call_bipred(nrefs=0) == -1 and call_bipred(nrefs=5) == -1 and call_part(nrefs=0) == -1
    assert call_part(nrefs=5) == -1 and call_mc(nrefs=0) == -1 and call_mc(nrefs=5) == -1
    assert call_part(mask=12) == -1 and call_part(mask=0) == -1 and call_part(mask=17) == -1  # no FULL bit / unknown bit
    assert call_bipred(mask=0) == -1 and call_bipred(mask=16) == -1
    assert call_bipred(drop=(1, 2)) == -1 and call_part(drop=(0, 1)) == -1       # a NULL array of a PRED in the mask
    assert call_bipred(null_cost=1) == -1 and call_bipred(null_sel=0) == -1    # NULL outputs of an alignment in the mask
    assert call_part(null_bi=0) == -1 and call_part(null_bi=1) == -1           # NULL bi_cost of an alignment in the mask
    assert call_part(bi_penalty=-1) == -1 and call_part(bi_penalty=(1 << 40) + 1) == -1
    assert call_part(penalty=-1) == -1 and call_part(penalty=(1 << 40) + 1) == -1
    assert call_part(cus=False) == -1 and call_part(ncus=False) == -1 and call_bipred(cur=False) == -1
    untouched()
    # an alignment outside the mask may pass NULL arrays
    assert call_bipred(mask=3, null_cost=1, null_sel=1, drop=(0, 2)) == 0
    assert call_part(mask=3, null_bi=1, drop=(1, 3)) == 0
    torch.cuda.synchronize()
    assert (bi_out["cost"][1] == SENTINEL).all() and (bi_out["cost"][0] != SENTINEL).all()
    assert int(out["ncus"]) > 0
    # the Python layer refuses the same before any call
    for kw in (dict(preds=12), dict(split_penalty=-1), dict(bi_penalty=-1), dict(bi_penalty=(1 << 40) + 1),
               dict(preds=31)):
        with pytest.raises(ValueError):
            eng.partition_bi(res, bi_in, **kw)
    with pytest.raises(ValueError):
        eng.partition_bi({k: v for k, v in res.items() if k != (1, "HALF_2CP")}, bi_in, preds=15)
    with pytest.raises(ValueError):
        eng.partition_bi(res, {"cost": [bi_in["cost"][0], None], "sel": bi_in["sel"]}, preds=15)
    with pytest.raises(ValueError):
        eng.partition_bi(res, bi_in, out={**sentinel_out(eng), "cus": torch.empty((eng.n_ctus * 64, 12),
                                                                                  dtype=torch.int32).cuda()})
    with pytest.raises(ValueError):
        eng.bipred(dcur, drefs, g["lam"], res, preds=0)
    with pytest.raises(ValueError):
        eng.bipred(dcur, drefs[:1], g["lam"], res)  # two references' results, one frame
    with pytest.raises(ValueError):
        eng.bipred(dcur, drefs, g["lam"], {k: v for k, v in res.items() if k != (0, "FULL_3CP")}, preds=15)
    with pytest.raises(ValueError):
        eng.bipred(dcur, drefs, g["lam"], res, out={"cost": bi_out["sel"], "sel": bi_out["sel"]})
    with pytest.raises(ValueError):
        eng.affine_mc_bi(mc_cus[:, :12].contiguous(), drefs, cur=dcur, want_cost=True)
    with pytest.raises(ValueError):
        eng.affine_mc_bi(mc_cus, drefs)  # neither pred nor cost


# ------------------------------------------------------------------ 10. determinism
def test_bipred_is_deterministic(engines):
    refs, cur, lam = four_refs()
    eng = engines(416, 240)
    drefs, dcur = [dev(r) for r in refs], dev(cur)
    res = eng.affine_me_poc(dcur, drefs, lam, modes=3)
    a = eng.bipred(dcur, drefs, lam, res)
    b = eng.bipred(dcur, drefs, lam, res)
    torch.cuda.synchronize()
    for k in ("cost", "sel"):
        for x in (0, 1):
            assert torch.equal(a[k][x], b[k][x]), (k, x)
    assert (a["sel"][0] >= 0).any()
