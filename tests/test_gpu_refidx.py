"""Reference indices 2 and 3 through every stage after the search (DESIGN.md
sections 11 to 16), 416x240, four pairwise different references of one cur.

Check A, on the device: what a four-reference call gives for index r equals
the one-reference call on [refs[r]] (the rate does not depend on the index).
Check B, against the CPU restatements: a sample at r = 2 and r = 3, so that
two indices wrong in the same way do not pass."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import bipred_ref as B
import birefine_ref as F
import mc_ref
import oracle_py as O
import partition_ref as R
import seed_ref as S
import seedpyr_ref as P
from test_gpu_bipred import NAMES, SENTINEL, blank, dev, four_refs, load, result_arrays
from test_seed import inframe, sample

pytestmark = pytest.mark.gpu

W, H = 416, 240
LAM = S.LAM
INF = S.INF
P_ = ctypes.c_void_p
BI_PAIRS = ((2, 3), (3, 2), (0, 3), (2, 2))
PART_ROLLS = ((0, 0), (0, 1), (0, 2), (-1, 1))


@pytest.fixture(scope="module")
def eng():
    from vame.engine import Engine
    e = Engine(W, H, 0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(refs [4, H, W], cur, lambda): 'rolled' four_refs() (rolls of the poc2
    reference), 'camera' / 'wide' the shifted cameras of seed_ref / seedpyr_ref
    with the reconstructions of POC 0..3, 'part' the rolls PART_ROLLS of the
    poc2 reference."""
    if name == "rolled":
        refs, cur, lam = four_refs()
        return np.stack(refs), cur, lam
    if name == "part":
        z = load("s416_qp32_poc2_ref0")
        return np.stack([np.roll(z["ref"], s, (0, 1)) for s in PART_ROLLS]), z["cur"], float(z["lam"])
    refs, cur = S.shifted_camera(4) if name == "camera" else P.shifted_camera_wide((-43, 26), nrefs=4)
    return refs, cur, LAM


@functools.lru_cache(maxsize=None)
def dev_inputs(name):
    refs, cur, lam = inputs(name)
    return [dev(r) for r in refs], dev(cur), lam


def same_seeds(got, r, one):
    return all(torch.equal(got[k][(r, a)], one[k][(0, a)]) for k in ("mv", "cost") for a in (0, 1))


def clone_result(res):
    return {k: (c.clone(), p.clone()) for k, (c, p) in res.items()}


# ------------------------------------------------------------------ the cases
@functools.lru_cache(maxsize=None)
def mc_cases():
    """17 non-overlapping CUs, every size, the frame's four edges, 2-CP and
    3-CP in turn: [x, y, w, h, nCPs, 6 CPMV components]."""
    geo = [(0, 0, 128, 128), (128, 0, 128, 64), (128, 64, 64, 64), (192, 64, 64, 32), (192, 96, 64, 16),
           (192, 112, 32, 16), (224, 112, 16, 16), (256, 0, 64, 128), (320, 0, 32, 64), (352, 0, 16, 64),
           (368, 0, 16, 32), (384, 0, 32, 32), (320, 64, 64, 64), (0, 224, 16, 16), (400, 224, 16, 16),
           (288, 176, 64, 64), (0, 128, 32, 32)]
    assert {(g[2], g[3]) for g in geo} == {(c[3], c[4]) for c in B.frame_candidates(W, H, 0)}
    rng = np.random.default_rng(23)
    out = []
    for k, g in enumerate(geo):
        cp = rng.integers(-90, 91, 6).tolist()
        out.append(list(g) + ([3] + cp if k & 1 else [2] + cp[:4] + [0, 0]))
    return out


def uni_descs(r):
    return [c[:4] + [r] + c[4:] for c in mc_cases()]


SEARCH_ANCHORS = (0, 1, 2, 3, 4, 7, 9, 13)   # 128x128, 128x64, 64x64, 64x32, 64x16, 64x128, 16x64, 16x16


@functools.lru_cache(maxsize=None)
def bi_cases():
    """[(ref0, ref1), descriptor [20]]: two CUs per pair of BI_PAIRS, the four
    (nCPs0, nCPs1) combinations among them."""
    cs = mc_cases()
    rng = np.random.default_rng(24)
    out = []
    for k, i in enumerate((2, 3, 5, 8, 11, 13, 12, 16)):
        r0, r1 = BI_PAIRS[k % 4]
        n1 = 2 + ((k >> 1) & 1)
        cp1 = rng.integers(-60, 61, 6).tolist()
        out.append(((r0, r1), cs[i][:4] + [r0] + cs[i][4:] + [r1, n1] + (cp1 if n1 == 3 else cp1[:4] + [0, 0])))
    return out


@functools.lru_cache(maxsize=None)
def seed_anchor_maps(r, align):
    """{row: sad_map at radius 16} of about 24 in-frame rows, reference r of 'camera'."""
    refs, cur, _ = inputs("camera")
    return {c: S.sad_map(refs[r], cur, c[1], c[2], c[3], c[4], 16) for c in sample(align, 24, salt=21)}


@functools.lru_cache(maxsize=None)
def wide_want(r, levels, align):
    refs, cur, _ = inputs("wide")
    return searcher(r).run(LAM, 64, levels, align)


@functools.lru_cache(maxsize=None)
def searcher(r):
    refs, cur, _ = inputs("wide")
    return P.Searcher(refs[r], cur)


@functools.lru_cache(maxsize=None)
def part_reference():
    """The CPU oracle's search on the four references of 'part' and the
    partition of it (mask 15, no penalty)."""
    refs, cur, lam = inputs("part")
    cost, cpmv = {}, {}
    for r, ref in enumerate(refs):
        for (a, ncp), (c, p) in O.affine_me_pair(ref, cur, lam).items():
            cost[(r, 2 * a + ncp - 2)], cpmv[(r, 2 * a + ncp - 2)] = c, np.array(p.tolist(), np.int32)
    return cost, cpmv, R.partition(W, H, cost, cpmv, 4, 15, 0)


def test_the_refidx_cases_cover_what_they_should():
    """On the references alone: four different frames per input, seeds that
    differ between any two references, every size and model pair in the cases."""
    for name in ("rolled", "camera", "wide", "part"):
        refs, _, _ = inputs(name)
        assert len(refs) == 4 and all((refs[a] != refs[b]).any() for a in range(4) for b in range(a))
    one, two = S.shifted_camera(1), S.shifted_camera(2)  # what shifted_camera gave before it took four
    assert (inputs("camera")[0][:2] == two[0]).all() and (two[0][:1] == one[0]).all()
    assert (one[1] == inputs("camera")[1]).all() and (two[1] == one[1]).all()
    refs, cur, _ = inputs("wide")
    rows = {(0, c[0]) for c in inframe(0)}
    mv = [P.Searcher(refs[r], cur, rows=rows).run(LAM, 64, 2, 0)[0] for r in range(4)]
    for a in range(4):
        for b in range(a):
            assert ((mv[a] != mv[b]).any(1)).sum() >= 100, (a, b)
    assert len(bi_cases()) == 8 and {p for p, _ in bi_cases()} == set(BI_PAIRS)
    assert {(d[5], d[13]) for _, d in bi_cases()} == {(2, 2), (2, 3), (3, 2), (3, 3)}
    assert {max(mc_cases()[i][2:4]) for i in SEARCH_ANCHORS} == {16, 64, 128}
    assert {tuple(mc_cases()[i][2:4]) for i in SEARCH_ANCHORS} >= {(128, 128), (64, 64), (16, 16), (128, 64), (64, 128)}


def test_the_partition_leaves_use_every_reference():
    """On the CPU oracle's search alone.  With four_refs()' rolls index 2 wins
    no leaf, so 'part' rolls the poc2 reference by (rows, columns) = (0, 0),
    (0, 1), (0, 2) and (-1, 1): 6, 7, 9 and 9 leaves."""
    part = part_reference()[2]
    assert set(part["cus"][:, 4].tolist()) == {0, 1, 2, 3}
    assert np.bincount(part["cus"][:, 4]).min() >= 2


# ------------------------------------------------------------------ 1. the seed searches
def test_seed_search_four_references(eng):
    drefs, dcur, _ = dev_inputs("camera")
    refs, cur, _ = inputs("camera")
    for radius in (3, 16):
        got = eng.seed_search(dcur, drefs, LAM, radius=radius)
        for r in range(4):
            assert same_seeds(got, r, eng.seed_search(dcur, [drefs[r]], LAM, radius=radius)), (radius, r)
        for r in (2, 3):
            for align in (0, 1):
                mv, cost = got["mv"][(r, align)].cpu().numpy(), got["cost"][(r, align)].cpu().numpy()
                for (row, x, y, w, h), m in seed_anchor_maps(r, align).items():
                    want = S.seed_from_map(m, x, y, w, h, W, H, radius, LAM)
                    assert (tuple(mv[row].tolist()), int(cost[row])) == want, (radius, r, align, row)
    # the map's selection is seed_cu's
    c, m = next(iter(seed_anchor_maps(3, 1).items()))
    assert S.seed_from_map(m, *c[1:], W, H, 3, LAM) == S.seed_cu(refs[3], cur, *c[1:], 3, LAM)


@pytest.mark.parametrize("anchor", [2, 3])
@pytest.mark.parametrize("levels", [1, 2])
def test_seed_search_wide_four_references(eng, levels, anchor):
    drefs, dcur, _ = dev_inputs("wide")
    got = eng.seed_search_wide(dcur, drefs, LAM, radius=64, levels=levels)
    pyr = [None, None, eng.seed_pyramid(drefs[2]), eng.seed_pyramid(drefs[3])]
    pre = eng.seed_search_wide(dcur, drefs, LAM, radius=64, levels=levels, ref_pyrs=pyr)
    torch.cuda.synchronize()
    for r in range(4):
        one = eng.seed_search_wide(dcur, [drefs[r]], LAM, radius=64, levels=levels)
        assert same_seeds(got, r, one) and same_seeds(pre, r, one), r
    for r in (anchor,):  # every row against the Searcher on refs[anchor]
        for align in (0, 1):
            mv, cost = got["mv"][(r, align)].cpu().numpy(), got["cost"][(r, align)].cpu().numpy()
            wmv, wcost, _ = wide_want(r, levels, align)
            bad = np.nonzero((mv != wmv).any(1) | (cost != wcost))[0]
            assert bad.size == 0, (levels, r, align, len(bad), [(int(k), mv[k].tolist(), wmv[k].tolist()) for k in bad[:5]])


def seed_sentinels(eng):
    mv = {(r, a): torch.full((eng.n_cus(a), 2), SENTINEL, dtype=torch.int32).cuda() for r in range(4) for a in (0, 1)}
    cost = {(r, a): torch.full((eng.n_cus(a),), SENTINEL, dtype=torch.int64).cuda() for r in range(4) for a in (0, 1)}
    return mv, cost


def test_seed_errors_write_nothing_at_four_references(eng):
    from vame._lib import SeedResult, lib
    drefs, dcur, _ = dev_inputs("wide")
    mv, cost = seed_sentinels(eng)
    pyrs = [eng.seed_pyramid(t) for t in drefs]
    cpyr = eng.seed_pyramid(dcur)
    torch.cuda.synchronize()

    def result(drop=None):
        sr = SeedResult()
        for k in mv:
            if k != drop:
                sr.mv[k[0]][k[1]] = mv[k].data_ptr()
            sr.cost[k[0]][k[1]] = cost[k].data_ptr()
        return sr

    refs = (P_ * 4)(*[t.data_ptr() for t in drefs])
    full = (P_ * 4)(*[t.data_ptr() for t in pyrs])
    hole = (P_ * 4)(*[t.data_ptr() for t in pyrs[:3]], None)
    sr, nomv = result(), result(drop=(3, 1))
    L = lib()
    assert L.vame_seed_search(eng._h, P_(dcur.data_ptr()), refs, 4, LAM, 3, 16, ctypes.byref(nomv), None) == -1
    assert L.vame_seed_search_wide(eng._h, P_(dcur.data_ptr()), P_(cpyr.data_ptr()), refs, full, 4, LAM, 3, 64, 2,
                                   ctypes.byref(nomv), None) == -1
    assert L.vame_seed_search_wide(eng._h, P_(dcur.data_ptr()), P_(cpyr.data_ptr()), refs, hole, 4, LAM, 3, 64, 2,
                                   ctypes.byref(sr), None) == -1
    torch.cuda.synchronize()
    assert all((t == SENTINEL).all() for t in mv.values()) and all((t == SENTINEL).all() for t in cost.values())
    # the same arguments, complete: accepted, and the four-reference result
    assert L.vame_seed_search_wide(eng._h, P_(dcur.data_ptr()), P_(cpyr.data_ptr()), refs, full, 4, LAM, 3, 64, 2,
                                   ctypes.byref(sr), None) == 0
    torch.cuda.synchronize()
    want = eng.seed_search_wide(dcur, drefs, LAM, radius=64, levels=2)
    assert all(torch.equal(mv[k], want["mv"][k]) and torch.equal(cost[k], want["cost"][k]) for k in mv)


# ------------------------------------------------------------------ 2. affine_mc, affine_search
def test_affine_mc_four_references(eng):
    drefs, dcur, lam = dev_inputs("rolled")
    refs, cur, _ = inputs("rolled")
    for r in range(4):
        cus = torch.tensor(uni_descs(r), dtype=torch.int32).cuda()
        pred, cost, bad = eng.affine_mc(cus, drefs, lam, cur=dcur, pred=blank(H, W), want_cost=True)
        cus[:, 4] = 0
        pred1, cost1, bad1 = eng.affine_mc(cus, [drefs[r]], lam, cur=dcur, pred=blank(H, W), want_cost=True)
        torch.cuda.synchronize()
        assert int(bad) == 0 and int(bad1) == 0 and torch.equal(pred, pred1) and torch.equal(cost, cost1), r
        if r < 2:
            continue
        got, gcost = pred.cpu().numpy().view(np.uint16), cost.cpu().numpy()
        for i, (x, y, w, h, ncp, *cp) in enumerate(mc_cases()):
            p, c, _ = mc_ref.predict_cu(refs[r], cur, x, y, w, h, ncp, cp, lam)
            assert (got[y:y + h, x:x + w] == p).all() and gcost[i] == c, (r, i)


def test_affine_search_four_references(eng):
    drefs, dcur, lam = dev_inputs("rolled")
    refs, cur, _ = inputs("rolled")
    for r in range(4):
        cus = torch.tensor(uni_descs(r), dtype=torch.int32).cuda()
        out, cost, bad = eng.affine_search(cus, drefs, dcur, lam, extra=0)
        cus[:, 4] = 0
        out1, cost1, bad1 = eng.affine_search(cus, [drefs[r]], dcur, lam, extra=0)
        torch.cuda.synchronize()
        assert int(bad) == 0 and int(bad1) == 0 and (out[:, 4] == r).all() and (out1[:, 4] == 0).all()
        assert torch.equal(out[:, :4], out1[:, :4]) and torch.equal(out[:, 5:], out1[:, 5:]) and torch.equal(cost, cost1), r
        assert (out[:, 6:] != cus[:, 6:]).any()
        if r < 2:
            continue
        got, gcost = out.cpu().numpy(), cost.cpu().numpy()
        for i in SEARCH_ANCHORS:
            x, y, w, h, ncp, *cp = mc_cases()[i]
            wcp, wcost = S.search_cu(refs[r], cur, x, y, w, h, ncp, cp, lam, 0)
            assert got[i, 6:6 + 2 * ncp].tolist() == wcp[:2 * ncp] and gcost[i] == wcost, (r, i)


# ------------------------------------------------------------------ 3. affine_mc_bi, bipred_refine
def test_bi_stages_four_references(eng):
    drefs, dcur, lam = dev_inputs("rolled")
    refs, cur, _ = inputs("rolled")
    for pair in BI_PAIRS:
        ds = [d for p, d in bi_cases() if p == pair]
        cus = torch.tensor(ds, dtype=torch.int32).cuda()
        pred, cost, bad = eng.affine_mc_bi(cus, drefs, lam, cur=dcur, pred=blank(H, W), want_cost=True)
        out, rcost, rbad = eng.bipred_refine(cus, drefs, dcur, lam, 2)
        two = cus.clone()
        two[:, 4], two[:, 12] = 0, int(pair[0] != pair[1])
        sub = [drefs[pair[0]]] + ([drefs[pair[1]]] if pair[0] != pair[1] else [])
        pred2, cost2, bad2 = eng.affine_mc_bi(two, sub, lam, cur=dcur, pred=blank(H, W), want_cost=True)
        out2, rcost2, rbad2 = eng.bipred_refine(two, sub, dcur, lam, 2)
        torch.cuda.synchronize()
        assert int(bad) == 0 and int(bad2) == 0 and int(rbad) == 0 and int(rbad2) == 0
        assert torch.equal(pred, pred2) and torch.equal(cost, cost2) and torch.equal(rcost, rcost2), pair
        assert out[:, 4].tolist() == [pair[0]] * len(ds) and out[:, 12].tolist() == [pair[1]] * len(ds)
        keep = [c for c in range(20) if c not in (4, 12)]
        assert torch.equal(out[:, keep], out2[:, keep]), pair
        # the anchor: the reference's bi cost (round 0) and its refined descriptor (round 2)
        for i, d in enumerate(ds[:2 if pair != (2, 2) else 0]):
            trace = F.refine_bicu_trace(refs, cur, d, lam, 2)
            assert int(cost[i]) == trace[0][1] and out[i].tolist() == trace[2][0] and int(rcost[i]) == trace[2][1], (pair, i)


# ------------------------------------------------------------------ 4. affine_me_seeded
def test_affine_me_seeded_four_references(eng):
    from vame._lib import lib
    drefs, dcur, _ = dev_inputs("camera")
    assert lib().vame_seeded_work_bytes(eng._h, 4, 3) > lib().vame_seeded_work_bytes(eng._h, 2, 3) > 0
    base = eng.affine_me_poc(dcur, drefs, LAM, modes=3)
    seeds = eng.seed_search(dcur, drefs, LAM, radius=16)["mv"]
    res, bad = eng.affine_me_seeded(dcur, drefs, LAM, clone_result(base), seeds, modes=3)
    torch.cuda.synchronize()
    assert int(bad) == 0 and set(res) == {(r, n) for r in range(4) for n in NAMES}
    for r in range(4):
        one, bad1 = eng.affine_me_seeded(dcur, [drefs[r]], LAM, {(0, n): (base[(r, n)][0].clone(), base[(r, n)][1].clone())
                                                                 for n in NAMES},
                                         {(0, a): seeds[(r, a)] for a in (0, 1)}, modes=3)
        torch.cuda.synchronize()
        assert int(bad1) == 0
        for n in NAMES:
            assert torch.equal(res[(r, n)][0], one[(0, n)][0]) and torch.equal(res[(r, n)][1], one[(0, n)][1]), (r, n)
            assert (res[(r, n)][0] <= base[(r, n)][0]).all() and (res[(r, n)][0] < base[(r, n)][0]).sum() >= 100, (r, n)


# ------------------------------------------------------------------ 5. the partition's leaves
def test_predict_partition_four_references(eng):
    drefs, dcur, lam = dev_inputs("part")
    refs, cur, _ = inputs("part")
    res = eng.affine_me_poc(dcur, drefs, lam, modes=3)
    part = eng.partition(res)
    pred, cost, bad = eng.predict_partition(part, drefs, lam, cur=dcur, pred=blank(H, W), want_cost=True)
    torch.cuda.synchronize()
    n = int(part["ncus"])
    cus = part["cus"][:n].contiguous()
    assert int(bad) == 0 and set(cus[:, 4].tolist()) == {0, 1, 2, 3}
    pred1, cost1, bad1 = eng.affine_mc(cus, drefs, lam, cur=dcur, pred=blank(H, W), want_cost=True)
    torch.cuda.synchronize()
    assert int(bad1) == 0 and torch.equal(pred, pred1) and torch.equal(cost[:n], cost1)
    # the decision is the reference's on the device's own search, and the oracle's
    want = R.partition(W, H, *result_arrays(res), 4, 15, 0)
    assert want["ncus"] == n and (cus.cpu().numpy() == want["cus"]).all()
    assert (want["cus"] == part_reference()[2]["cus"]).all()
    got = pred.cpu().numpy().view(np.uint16)
    assert (got != 0xFFFF).all()
    for d in want["cus"]:
        if d[4] >= 2:
            p, c, _ = mc_ref.predict_cu(refs[d[4]], None, d[0], d[1], d[2], d[3], d[5], d[6:])
            assert (got[d[1]:d[1] + d[3], d[0]:d[0] + d[2]] == p).all(), d.tolist()
