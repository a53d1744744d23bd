"""vame_partition and vame_affine_mc_dev on the GPU (Engine.partition,
Engine.affine_mc(ncus=), Engine.predict_partition): every output array bit for
bit against the CPU restatement of the rule (tests/partition_ref.py), the
predicted frame against the per-CU reference tests/mc_ref.py."""
import ctypes
import functools
import glob
import os

import numpy as np
import pytest
import torch

import mc_ref
import partition_ref as R
from vame.partition import KEYS, to_host

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
GOLDENS = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLD, "s416_*.npz"))) + ["s832_qp37_poc1"]
NAMES = ("FULL_2CP", "FULL_3CP", "HALF_2CP", "HALF_3CP")
SENTINEL = -77


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
    """{(refIdx, PRED): arrays} -> an alloc_poc dict on the device (7-column
    CPMV rows: nCPs, LT, RT, LB)."""
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


def golden_arrays(zs):
    cost = {(r, m): z[n + "_cost"] for r, z in enumerate(zs) for m, n in enumerate(NAMES)}
    cpmv = {(r, m): z[n + "_cpmv"] for r, z in enumerate(zs) for m, n in enumerate(NAMES)}
    return cost, cpmv


def sentinel_out(eng):
    from vame.partition import alloc
    out = alloc(eng.n_ctus, eng.device)
    for t in out.values():
        t.fill_(SENTINEL)
    return out


def run_and_compare(eng, cost, cpmv, nrefs, mask, penalty=0):
    """One Engine.partition call into sentinel-filled outputs: every array
    equals the reference, nothing at or past the count is written."""
    want = R.partition(eng.W, eng.H, cost, cpmv, nrefs, mask, penalty)
    part = eng.partition(result_dict(cost, cpmv, mask), preds=mask, split_penalty=penalty, out=sentinel_out(eng))
    torch.cuda.synchronize()
    n = int(part["ncus"])
    assert n == want["ncus"]
    assert (part["cus"][n:] == SENTINEL).all() and (part["rows"][n:] == SENTINEL).all()
    got = to_host(part)
    for k in KEYS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    return want, part


# ------------------------------------------------------------------ 1. goldens x masks
@pytest.mark.parametrize("mask", [1, 3, 15], ids=["F2", "F23", "all"])
@pytest.mark.parametrize("name", GOLDENS)
def test_goldens(engines, name, mask):
    z = load(name)
    cost, cpmv = golden_arrays([z])
    want, _ = run_and_compare(engines(int(z["W"]), int(z["H"])), cost, cpmv, 1, mask)
    if mask == 15 and name in ("s416_noise", "s416_bigmotion"):
        half = [R.candidates()[(c[0] % 128, c[1] % 128, c[2], c[3])][0] for c in want["cus"]]
        assert 70 <= want["ncus"] <= 300 and sum(half) > 0


# ------------------------------------------------------------------ 2. two references
@pytest.mark.parametrize("mask", [3, 15])
def test_two_references(engines, mask):
    zs = [load("s416_qp32_poc2_ref0"), load("s416_qp32_poc2_ref1")]
    assert (zs[0]["cur"] == zs[1]["cur"]).all()
    cost, cpmv = golden_arrays(zs)
    want, _ = run_and_compare(engines(416, 240), cost, cpmv, 2, mask)
    assert set(want["cus"][:, 4].tolist()) == {0, 1}


# ------------------------------------------------------------------ 3. split penalty
@pytest.mark.parametrize("penalty,leaves", [(0, 288), (2000, 275), (1 << 40, 23)])
def test_split_penalty(engines, penalty, leaves):
    cost, cpmv = golden_arrays([load("s416_noise")])
    want, _ = run_and_compare(engines(416, 240), cost, cpmv, 1, 15, penalty)
    assert want["ncus"] == leaves


# ------------------------------------------------------------------ 4. synthetic costs
@pytest.mark.parametrize("W,H,ties,penalty", [(416, 240, False, 0), (416, 240, True, 0), (416, 240, True, 1),
                                              (1920, 1080, False, 0), (1920, 1080, True, 0)])
def test_synthetic_costs(engines, W, H, ties, penalty):
    cost, cpmv = R.synthetic(W, H, 4, 1, ties)
    want, _ = run_and_compare(engines(W, H), cost, cpmv, 4, 15, penalty)
    if (W, ties) == (1920, False):
        half = [R.candidates()[(c[0] % 128, c[1] % 128, c[2], c[3])][0] for c in want["cus"]]
        assert (want["splits"] > 0).all(), want["splits"]
        assert set(want["cus"][:, 4].tolist()) == {0, 1, 2, 3} and set(want["cus"][:, 5].tolist()) == {2, 3}
        assert sum(half) > 0 and want["ctu_info"][:, 2].sum() == 120


def test_synthetic_subset_of_preds_with_null_arrays(engines):
    """PREDs outside the mask are not read: their arrays are absent (NULL)."""
    cost, cpmv = R.synthetic(416, 240, 3, 7)
    for mask in (2, 6, 9):
        run_and_compare(engines(416, 240), cost, cpmv, 3, mask, 50)


# ------------------------------------------------------------------ 5. pipeline
@pytest.mark.parametrize("name", ["s416_noise", "s832_qp37_poc1"])
def test_pipeline_predicts_the_partition(engines, name):
    z = load(name)
    W, H, lam = int(z["W"]), int(z["H"]), float(z["lam"])
    eng = engines(W, H)
    cost, cpmv = golden_arrays([z])
    want, part = run_and_compare(eng, cost, cpmv, 1, 15)
    pred, mc_cost, bad = eng.predict_partition(part, [dev(z["ref"])], lam, cur=dev(z["cur"]), pred=blank(H, W),
                                               want_cost=True)
    torch.cuda.synchronize()
    assert int(bad) == 0 and mc_cost.numel() == eng.n_ctus * 64
    frame = np.full((H, W), 0xFFFF, np.uint16)
    for d in want["cus"]:
        p, _, _ = mc_ref.predict_cu(z["ref"], None, d[0], d[1], d[2], d[3], d[5], d[6:])
        frame[d[1]:d[1] + d[3], d[0]:d[0] + d[2]] = p
    np.testing.assert_array_equal(pred.cpu().numpy().view(np.uint16), frame)
    # penalty 0, the fixture's lambda: the leaves' mc costs are the search's, their sum per CTU the root's value
    n = want["ncus"]
    got = mc_cost.cpu().numpy()[:n]
    np.testing.assert_array_equal(got, want["leaf_cost"])
    for ctu, (first, count, _, _) in enumerate(want["ctu_info"]):
        assert got[first:first + count].sum() == want["ctu_cost"][ctu]


# ------------------------------------------------------------------ 6. affine_mc(ncus=)
def mc_descs(n, W, H):
    rng = np.random.default_rng(5)
    out = []
    for k in range(n):
        w, h = [(16, 16), (32, 16), (64, 64), (16, 32)][k % 4]
        out.append([16 * (k % 4) * 4 + 0, 64 * (k // 4), w, h, k & 1, 2 + (k % 3 == 0)] + rng.integers(-90, 91, 6).tolist())
    return out


def test_affine_mc_device_count(engines):
    z = load("s416_noise")
    W, H, lam = 416, 240, float(z["lam"])
    eng = engines(W, H)
    refs, cur = [dev(z["ref"]), dev(np.roll(z["ref"], 3, 1))], dev(z["cur"])
    valid = mc_descs(12, W, H)
    garbage = [[-5, 3, 17, 9, 9, 7, 1 << 20, 0, 0, 0, 0, 0]] * 4  # invalid in every field
    cus = torch.tensor(valid[:8] + garbage, dtype=torch.int32).cuda()
    want_pred, want_cost, bad0 = eng.affine_mc(cus[:8].contiguous(), refs, lam, cur=cur, pred=blank(H, W), want_cost=True)
    assert int(bad0) == 0

    def run(cus, count, pred):
        ncus = torch.tensor(count, dtype=torch.int32).cuda()
        # the cost tensor of the call is uninitialised: give it a known fill through the C ABI
        cost = torch.full((cus.shape[0],), SENTINEL, dtype=torch.int64).cuda()
        bad = torch.zeros((), dtype=torch.int32).cuda()
        from vame._lib import lib
        V = ctypes.c_void_p
        ptrs = (V * 2)(refs[0].data_ptr(), refs[1].data_ptr())
        rc = lib().vame_affine_mc_dev(eng._h, V(cur.data_ptr()), ptrs, 2, V(cus.data_ptr()), cus.shape[0],
                                      V(ncus.data_ptr()), lam, V(pred.data_ptr()), V(cost.data_ptr()),
                                      V(bad.data_ptr()), None)
        torch.cuda.synchronize()
        assert rc == 0
        return cost, bad

    # count < capacity, garbage past it: bad stays 0, their cost and samples untouched
    pred = blank(H, W)
    cost, bad = run(cus, 8, pred)
    assert int(bad) == 0 and torch.equal(cost[:8], want_cost) and (cost[8:] == SENTINEL).all()
    assert torch.equal(pred, want_pred)
    # the same through Engine.affine_mc(ncus=)
    pred = blank(H, W)
    _, cost, bad = eng.affine_mc(cus, refs, lam, cur=cur, pred=pred, want_cost=True,
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
    # an invalid descriptor below the count still sets bad (and costs 0, writes nothing)
    pred = blank(H, W)
    cost, bad = run(cus, 9, pred)
    assert int(bad) == 1 and torch.equal(cost[:8], want_cost) and int(cost[8]) == 0 and (cost[9:] == SENTINEL).all()
    assert torch.equal(pred, want_pred)
    # a count of a few descriptors out of many: a grid sized for the capacity
    many = torch.tensor(mc_descs(12, W, H) * 200, dtype=torch.int32).cuda()
    cost, bad = run(many, 3, blank(H, W))
    assert int(bad) == 0 and torch.equal(cost[:3], want_cost[:3]) and (cost[3:] == SENTINEL).all()
    with pytest.raises(ValueError):
        eng.affine_mc(cus, refs, lam, cur=cur, want_cost=True, ncus=torch.tensor(8).cuda())  # int64


# ------------------------------------------------------------------ 7. one graph
def test_search_partition_prediction_in_one_graph():
    """search -> partition -> predict_partition captured on a fresh engine,
    replayed after the input frames were overwritten: equal to direct calls."""
    from vame.engine import Engine
    a, b = load("s416_noise"), load("s416_bigmotion")
    W, H, lam = 416, 240, float(b["lam"])
    eng, direct = Engine(W, H, 0), Engine(W, H, 0)
    try:
        cur, ref = dev(a["cur"]), dev(a["ref"])
        res = eng.alloc_poc(1, 3)
        pred = blank(H, W)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            eng.affine_me_poc(cur, [ref], lam, modes=3, out=res)
            part = eng.partition(res, split_penalty=100)
            _, cost, bad = eng.predict_partition(part, [ref], lam, cur=cur, pred=pred, want_cost=True)
        cur.copy_(dev(b["cur"]))
        ref.copy_(dev(b["ref"]))
        for t in list(part.values()) + [pred, cost]:
            t.fill_(-1)
        bad.fill_(5)
        g.replay()
        torch.cuda.synchronize()
        wres = direct.affine_me_poc(cur, [ref], lam, modes=3)
        wpart = direct.partition(wres, split_penalty=100)
        wpred, wcost, wbad = direct.predict_partition(wpart, [ref], lam, cur=cur, pred=blank(H, W), want_cost=True)
        torch.cuda.synchronize()
        n = int(wpart["ncus"])
        assert n > 23 and int(part["ncus"]) == n and int(bad) == 0 and int(wbad) == 0
        for k in KEYS:
            cut = n if k in ("cus", "rows") else None
            assert torch.equal(part[k][:cut] if cut else part[k], wpart[k][:cut] if cut else wpart[k]), k
        assert torch.equal(pred, wpred) and torch.equal(cost[:n], wcost[:n])
        assert (cost[n:] == -1).all() and (part["cus"][n:] == -1).all()
        # and the direct calls agree with the CPU reference on the search's golden results
        want = R.from_goldens([b], 15, 100)
        got = to_host(wpart)
        for k in KEYS:
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    finally:
        eng.close()
        direct.close()


# ------------------------------------------------------------------ 8. argument errors
def test_argument_errors_write_nothing(engines):
    from vame._lib import PocResult, lib
    eng = engines(416, 240)
    cost, cpmv = R.synthetic(416, 240, 2, 3)
    res = result_dict(cost, cpmv)
    out = sentinel_out(eng)
    V = ctypes.c_void_p

    def call(nrefs=2, mask=15, penalty=0, drop=None, cus=True, ncus=True, ctx=True, null_res=False):
        pr = PocResult()
        for (r, name), (c, p) in res.items():
            m = NAMES.index(name)
            if drop == (r, m):
                continue
            pr.cost[r][m] = c.data_ptr()
            pr.cpmvs[r][m] = p.data_ptr()
        ptr = {k: V(out[k].data_ptr()) for k in KEYS}
        return lib().vame_partition(eng._h if ctx else None, None if null_res else ctypes.byref(pr), nrefs, mask,
                                    penalty, ptr["cus"] if cus else None, ptr["rows"], ptr["ncus"] if ncus else None,
                                    ptr["ctu_info"], ptr["ctu_cost"], ptr["block_cu"], None)

    assert call(nrefs=0) == -1 and call(nrefs=5) == -1
    assert call(mask=12) == -1 and call(mask=0) == -1 and call(mask=16 | 1) == -1  # no FULL bit / unknown bit
    assert call(drop=(1, 2)) == -1 and call(drop=(0, 0)) == -1                     # NULL array of a PRED in the mask
    assert call(penalty=-1) == -1 and call(penalty=(1 << 40) + 1) == -1
    assert call(cus=False) == -1 and call(ncus=False) == -1 and call(ctx=False) == -1 and call(null_res=True) == -1
    torch.cuda.synchronize()
    assert all((t == SENTINEL).all() for t in out.values())
    # the nullable outputs: the call runs with cus and ncus alone
    pr = PocResult()
    for (r, name), (c, p) in res.items():
        pr.cost[r][NAMES.index(name)] = c.data_ptr()
        pr.cpmvs[r][NAMES.index(name)] = p.data_ptr()
    assert lib().vame_partition(eng._h, ctypes.byref(pr), 2, 15, 0, V(out["cus"].data_ptr()), None,
                                V(out["ncus"].data_ptr()), None, None, None, None) == 0
    torch.cuda.synchronize()
    want = R.partition(416, 240, cost, cpmv, 2, 15, 0)
    n = int(out["ncus"])
    assert n == want["ncus"]
    np.testing.assert_array_equal(out["cus"][:n].cpu().numpy(), want["cus"])
    assert all((out[k] == SENTINEL).all() for k in ("rows", "ctu_info", "ctu_cost", "block_cu"))
    # the Python layer refuses the same before any call
    for kw in (dict(preds=12), dict(split_penalty=-1), dict(split_penalty=(1 << 40) + 1), dict(preds=31)):
        with pytest.raises(ValueError):
            eng.partition(res, **kw)
    with pytest.raises(ValueError):
        eng.partition({k: v for k, v in res.items() if k != (1, "HALF_2CP")}, preds=15)
