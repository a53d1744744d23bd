"""The wide-range seed search on the GPU (Engine.seed_pyramid,
Engine.seed_search_wide): bit for bit against the CPU
restatement tests/seedpyr_ref.py on every row, 416x240 throughout (8 CTUs, CUs
leaving the frame at the right and the bottom)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import bipred_ref as B
import seed_ref as S
import seedpyr_ref as P
from test_gpu_bipred import NAMES, SENTINEL, blank, dev
from test_seed import inframe
from vame import seed as V

pytestmark = pytest.mark.gpu

W, H = 416, 240
LAM = S.LAM
INF = S.INF
P_ = ctypes.c_void_p
NPYR = (W // 2) * (H // 2) + (W // 4) * (H // 4)

# name -> (input, radius): what each is for is asserted in test_the_wide_cases_cover_what_they_should
CASES = {"wide": ("left_up", 64), "right_down": ("right_down", 64), "r128": ("left_up", 128), "odd": ("left_up", 37),
         "ties": ("stripes", 64)}
PARAMS = [(c, l, lam) for c in ("wide", "right_down", "odd") for l in (1, 2) for lam in (0.0, LAM)] + \
    [("r128", 2, 0.0), ("r128", 2, LAM), ("ties", 1, 0.0), ("ties", 2, 0.0)]


@pytest.fixture(scope="module")
def eng():
    from vame.engine import Engine
    e = Engine(W, H, 0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(refs [2, H, W], cur): the shifted camera moved by (-43, +26) / by
    (+40, +30), or vertical stripes of period 16 with cur = refs[0] moved by 4
    samples (refs[1]: by 8)."""
    if name == "left_up":
        return P.shifted_camera_wide((-43, 26), 2)
    if name == "right_down":
        return P.shifted_camera_wide((40, 30), 2)
    return P.stripes(W, H)


@functools.lru_cache(maxsize=None)
def dev_input(name):
    refs, cur = inputs(name)
    return [dev(r) for r in refs], dev(cur)


@functools.lru_cache(maxsize=None)
def searchers(name):
    refs, cur = inputs(name)
    return [P.Searcher(r, cur) for r in refs]


@functools.lru_cache(maxsize=None)
def want(name, r, lam, radius, levels, align):
    """(mv, cost, facts) of the reference, computed once and left unchanged."""
    return searchers(name)[r].run(lam, radius, levels, align)


def same(a, b):
    return all(torch.equal(a[k][key], b[k][key]) for k in ("mv", "cost") for key in b[k])


# ------------------------------------------------------------------ 1. the pyramid
def test_pyramid_equals_the_reference(eng):
    rng = np.random.default_rng(1600)
    f = rng.integers(0, 1024, (H, W)).astype(np.uint16)
    f[:4, :8], f[4:8, :8] = 1023, 0
    got = eng.seed_pyramid(dev(f))
    assert got.shape == (NPYR,)
    np.testing.assert_array_equal(got.cpu().numpy().view(np.uint16), P.packed(f))
    # into a given tensor, twice the same
    again = torch.full((NPYR,), SENTINEL, dtype=torch.int16).cuda()
    assert eng.seed_pyramid(dev(f), out=again) is again and torch.equal(again, got)
    with pytest.raises(ValueError):
        eng.seed_pyramid(dev(f), out=torch.zeros(NPYR - 1, dtype=torch.int16).cuda())
    with pytest.raises(ValueError):
        eng.seed_pyramid(dev(f), out=torch.zeros(NPYR + 4, dtype=torch.int16).cuda()[1:-3])  # not 8-byte aligned


# ------------------------------------------------------------------ 2. against the reference
def test_the_wide_cases_cover_what_they_should():
    for align in (0, 1):
        f = want("left_up", 0, LAM, 64, 2, align)[2]
        assert f["outside"] and len(f["outside"]) + len(inframe(align)) == len(B.frame_candidates(W, H, align))
        assert f[("moved", 0)] and f[("moved", 1)]           # winners off the coarse centre at each level
        assert want("left_up", 0, LAM, 64, 1, align)[2][("moved", 0)]
        f = want("right_down", 0, LAM, 64, 2, align)[2]
        assert f["cut_x"] and f["cut_y"]                     # Dx <= W+7-x and Dy <= H+7-y cut candidates
        mv = want("right_down", 0, LAM, 64, 2, align)[0]
        assert ((mv[:, 0] > 16 * 32) & (mv[:, 1] > 16 * 24)).sum() >= 100   # the winners point right and down
        assert want("ties", 0, 0.0, 64, 2, align)[2]["top_tie"] and want("ties", 0, 0.0, 64, 1, align)[2]["top_tie"]
        for levels in (1, 2):                                # 37: Rc * 2^L = 36 < radius, winners at the radius itself
            assert (37 >> levels) << levels == 36
            assert (np.abs(want("left_up", 0, LAM, 37, levels, align)[0]).max(1) == 16 * 37).sum() >= 100
        assert want("left_up", 0, LAM, 37, 2, align)[2]["cut_radius"]   # level 1: 2 * 9 + 1 stands for 38
        assert want("left_up", 0, LAM, 64, 1, align)[2]["cut_radius"]   # level 0: 2 * 32 + 1 = 65
        mv = want("left_up", 0, LAM, 128, 2, align)[0]
        assert (np.abs(mv) > 16 * 64).any()                  # radius 128 is used
    assert len(PARAMS) == 16 and {c for c, _, _ in PARAMS} == set(CASES)


@pytest.mark.parametrize("case,levels,lam", PARAMS)
def test_seed_search_wide_against_reference(eng, case, levels, lam):
    name, radius = CASES[case]
    drefs, dcur = dev_input(name)
    out = eng.seed_search_wide(dcur, drefs, lam, radius=radius, levels=levels)
    torch.cuda.synchronize()
    for r in (0, 1):
        for align in (0, 1):
            mv, cost = out["mv"][(r, align)].cpu().numpy(), out["cost"][(r, align)].cpu().numpy()
            wmv, wcost, facts = want(name, r, lam, radius, levels, align)
            bad = np.nonzero((mv != wmv).any(1) | (cost != wcost))[0]
            assert bad.size == 0, (case, levels, lam, r, align, len(bad),
                                   [(int(k), mv[k].tolist(), int(cost[k]), wmv[k].tolist(), int(wcost[k])) for k in bad[:5]])
            outside = sorted(facts["outside"])
            assert (cost[outside] == INF).all() and not mv[outside].any()


def test_radius_0_equals_seed_search(eng):
    drefs, dcur = dev_input("left_up")
    zero = eng.seed_search(dcur, drefs, LAM, radius=0)
    for levels in (1, 2):
        assert same(eng.seed_search_wide(dcur, drefs, LAM, radius=0, levels=levels), zero)


# ------------------------------------------------------------------ 3. the seed's cost is affine_mc's block
def test_wide_seed_cost_is_the_sad_of_affine_mc_plus_rate(eng):
    drefs, dcur = dev_input("left_up")
    _, cur = inputs("left_up")
    out = eng.seed_search_wide(dcur, drefs, LAM, radius=64, levels=2)
    n = far = 0
    for align in (0, 1):
        cus, rows = V.cus_from_seeds(W, H, align, out["mv"][(1, align)], ref=1, skip_zero=False)
        assert rows.tolist() == [c[0] for c in inframe(align)]
        cost = out["cost"][(1, align)][rows].cpu().numpy()
        step = max(1, len(rows) // 20)
        for k in range(0, len(rows), step):
            d = cus[k].tolist()
            pred, _, bad = eng.affine_mc(cus[k:k + 1].contiguous(), drefs, pred=blank(H, W))
            torch.cuda.synchronize()
            x, y, w, h = d[:4]
            p = pred.cpu().numpy().view(np.uint16)[y:y + h, x:x + w].astype(np.int64)
            sad = int(np.abs(cur[y:y + h, x:x + w].astype(np.int64) - p).sum())
            assert int(bad) == 0 and sad + B.rate(B.bits_of(2, d[6:12]) + 2, LAM) == cost[k], (align, k, d)
            n += 1
            far += max(abs(d[6]), abs(d[7])) > 16 * 32
    assert n >= 38 and far >= 10  # displacements beyond seed_search's range among them


# ------------------------------------------------------------------ 4. masks, errors
def sentinels(eng, nrefs=2):
    mv = {(r, a): torch.full((eng.n_cus(a), 2), SENTINEL, dtype=torch.int32).cuda() for r in range(nrefs) for a in (0, 1)}
    cost = {(r, a): torch.full((eng.n_cus(a),), SENTINEL, dtype=torch.int64).cuda() for r in range(nrefs) for a in (0, 1)}
    return mv, cost


@functools.lru_cache(maxsize=None)
def dev_pyramids(name):
    from vame.engine import Engine
    e = Engine(W, H, 0)
    try:
        drefs, dcur = dev_input(name)
        out = [e.seed_pyramid(r) for r in drefs], e.seed_pyramid(dcur)
        torch.cuda.synchronize()
        return out
    finally:
        e.close()


def raw_wide(eng, mv, cost, mask=3, radius=16, levels=2, nrefs=2, null=(), off=None, no_pyr=None):
    """vame_seed_search_wide on the left_up input with prebuilt pyramids.  null:
    arguments passed as NULL; off: {argument: bytes added to its pointer
    ('cur', 'cur_pyr', ('ref', r), ('ref_pyr', r))}; no_pyr: an r whose pyramid
    pointer is NULL."""
    from vame._lib import SeedResult, lib
    drefs, dcur = dev_input("left_up")
    rpyr, cpyr = dev_pyramids("left_up")
    off = off or {}
    sr = SeedResult()
    for (r, a), t in mv.items():
        sr.mv[r][a] = t.data_ptr()
    for (r, a), t in cost.items():
        sr.cost[r][a] = t.data_ptr()
    refs = (P_ * 4)(*[t.data_ptr() + off.get(("ref", r), 0) for r, t in enumerate(drefs)])
    pyrs = (P_ * 4)(*[None if r == no_pyr else t.data_ptr() + off.get(("ref_pyr", r), 0) for r, t in enumerate(rpyr)])
    arg = {"cur": P_(dcur.data_ptr() + off.get("cur", 0)), "cur_pyr": P_(cpyr.data_ptr() + off.get("cur_pyr", 0)),
           "refs": refs, "ref_pyrs": pyrs, "out": ctypes.byref(sr)}
    for k in null:
        arg[k] = None
    rc = lib().vame_seed_search_wide(eng._h, arg["cur"], arg["cur_pyr"], arg["refs"], arg["ref_pyrs"], nrefs, LAM, mask,
                                     radius, levels, arg["out"], None)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("mask", [1, 2])
def test_alignments_outside_the_mask_are_untouched(eng, mask):
    drefs, dcur = dev_input("left_up")
    both = eng.seed_search_wide(dcur, drefs, LAM, radius=16, levels=2)
    mv, cost = sentinels(eng)
    assert raw_wide(eng, mv, cost, mask=mask) == 0
    on, off = (0, 1) if mask == 1 else (1, 0)
    for r in (0, 1):
        assert torch.equal(mv[(r, on)], both["mv"][(r, on)]) and torch.equal(cost[(r, on)], both["cost"][(r, on)])
        assert (mv[(r, off)] == SENTINEL).all() and (cost[(r, off)] == SENTINEL).all()
    # through the Python view: only the mask's keys, written into given arrays
    one = eng.seed_search_wide(dcur, drefs, LAM, radius=16, aligns=mask, out={"mv": mv, "cost": cost})
    assert one["mv"] is mv and set(eng.seed_search_wide(dcur, drefs, LAM, radius=3, aligns=mask)["mv"]) == \
        {(0, on), (1, on)}


def test_errors_write_nothing(eng):
    from vame._lib import lib
    mv, cost = sentinels(eng)

    def untouched():
        assert all((t == SENTINEL).all() for t in mv.values()) and all((t == SENTINEL).all() for t in cost.values())

    assert raw_wide(eng, mv, cost, nrefs=0) == -1 and raw_wide(eng, mv, cost, nrefs=5) == -1
    for mask in (0, 4, 7):
        assert raw_wide(eng, mv, cost, mask=mask) == -1
    for radius in (-1, 129):
        assert raw_wide(eng, mv, cost, radius=radius) == -1
    for levels in (0, 3, -1):
        assert raw_wide(eng, mv, cost, levels=levels) == -1
    for k in ("cur", "cur_pyr", "refs", "ref_pyrs", "out"):
        assert raw_wide(eng, mv, cost, null=(k,)) == -1, k
    assert raw_wide(eng, mv, cost, no_pyr=1) == -1                                             # a NULL pyramid
    assert raw_wide(eng, {k: v for k, v in mv.items() if k != (1, 1)}, cost) == -1             # a NULL output
    assert raw_wide(eng, mv, {k: v for k, v in cost.items() if k != (0, 0)}, mask=1) == -1
    for off in ({"cur": 2}, {"cur": 4}, {"cur_pyr": 4}, {("ref_pyr", 1): 4}, {("ref_pyr", 0): 2}, {("ref", 1): 2}):
        assert raw_wide(eng, mv, cost, off=off) == -1, off
    untouched()
    # the pyramid call
    drefs, dcur = dev_input("left_up")
    pyr = torch.full((NPYR + 4,), SENTINEL, dtype=torch.int16).cuda()
    assert lib().vame_seed_pyramid_bytes(eng._h) == 2 * NPYR and lib().vame_seed_pyramid_bytes(None) == 0
    assert lib().vame_seed_pyramid(eng._h, None, P_(pyr.data_ptr()), None) == -1
    assert lib().vame_seed_pyramid(eng._h, P_(dcur.data_ptr()), None, None) == -1
    assert lib().vame_seed_pyramid(eng._h, P_(dcur.data_ptr() + 2), P_(pyr.data_ptr()), None) == -1
    assert lib().vame_seed_pyramid(eng._h, P_(dcur.data_ptr()), P_(pyr.data_ptr() + 4), None) == -1
    torch.cuda.synchronize()
    assert (pyr == SENTINEL).all()
    # the Python layer refuses the same before any call
    rpyr, cpyr = dev_pyramids("left_up")
    for kw in (dict(radius=129), dict(radius=-1), dict(levels=0), dict(levels=3), dict(aligns=0), dict(aligns=4),
               dict(out={"mv": {}, "cost": {}}), dict(out={"mv": cost, "cost": cost}), dict(ref_pyrs=rpyr[:1]),
               dict(cur_pyr=cpyr[:-1]), dict(ref_pyrs=[rpyr[0], cpyr.to(torch.int32)])):
        with pytest.raises(ValueError):
            eng.seed_search_wide(dcur, drefs, LAM, **kw)
    with pytest.raises(ValueError):
        eng.seed_search_wide(dcur, [], LAM)
    # the limits themselves are accepted
    assert raw_wide(eng, mv, cost, radius=128, levels=1) == 0 and raw_wide(eng, mv, cost, radius=0, levels=2) == 0


# ------------------------------------------------------------------ 5. determinism, prebuilt pyramids, PROF
def test_two_calls_agree_and_prebuilt_pyramids_change_nothing(eng):
    from vame.engine import Engine
    drefs, dcur = dev_input("left_up")
    a = eng.seed_search_wide(dcur, drefs, LAM, radius=64, levels=2)
    b = eng.seed_search_wide(dcur, drefs, LAM, radius=64, levels=2)
    rpyr, cpyr = dev_pyramids("left_up")
    c = eng.seed_search_wide(dcur, drefs, LAM, radius=64, levels=2, cur_pyr=cpyr, ref_pyrs=rpyr)
    d = eng.seed_search_wide(dcur, drefs, LAM, radius=64, levels=2, ref_pyrs=[None, rpyr[1]])
    torch.cuda.synchronize()
    assert same(a, b) and same(a, c) and same(a, d)
    prof = Engine(W, H, 0)  # PROF does not enter
    try:
        prof.set_prof(True)
        e = prof.seed_search_wide(dcur, drefs, LAM, radius=64, levels=2)
        torch.cuda.synchronize()
        assert same(a, e)
    finally:
        prof.close()


# ------------------------------------------------------------------ 6. the chain
def clone_result(res):
    return {k: (c.clone(), p.clone()) for k, (c, p) in res.items()}


def test_wide_seeds_beat_radius_32_seeds(eng):
    drefs, dcur = dev_input("left_up")
    base = eng.affine_me_poc(dcur, drefs[:1], LAM, modes=1)
    wide = eng.seed_search_wide(dcur, drefs[:1], LAM, radius=64, levels=2)
    near = eng.seed_search(dcur, drefs[:1], LAM, radius=32)
    rw, bw = eng.affine_me_seeded(dcur, drefs[:1], LAM, clone_result(base), wide["mv"], modes=1)
    rn, bn = eng.affine_me_seeded(dcur, drefs[:1], LAM, clone_result(base), near["mv"], modes=1)
    torch.cuda.synchronize()
    assert int(bw) == 0 and int(bn) == 0
    total = {}
    for tag, res in (("base", base), ("near", rn), ("wide", rw)):
        total[tag] = sum(int(res[(0, NAMES[2 * a])][0][[c[0] for c in inframe(a)]].sum()) for a in (0, 1))
    print(total)
    assert total["wide"] < total["near"] <= total["base"]


def test_pyramids_to_prediction_in_one_graph():
    """seed_pyramid x 3 -> affine_me_poc -> seed_search_wide -> affine_me_seeded
    -> partition -> predict_partition captured on a fresh engine, replayed
    after the inputs were overwritten: equal to direct calls on a second
    engine."""
    from vame.engine import Engine
    refs_np, cur_np = inputs("left_up")
    other_refs, other_cur = inputs("right_down")
    eng, direct = Engine(W, H, 0), Engine(W, H, 0)
    try:
        cur, refs = dev(other_cur), [dev(other_refs[0]), dev(other_refs[1])]
        res = eng.alloc_poc(2, 3)
        pred = blank(H, W)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            cpyr = eng.seed_pyramid(cur)
            rpyr = [eng.seed_pyramid(r) for r in refs]
            eng.affine_me_poc(cur, refs, LAM, modes=3, out=res)
            seeds = eng.seed_search_wide(cur, refs, LAM, radius=64, levels=2, cur_pyr=cpyr, ref_pyrs=rpyr)
            _, sbad = eng.affine_me_seeded(cur, refs, LAM, res, seeds["mv"], modes=3)
            part = eng.partition(res, split_penalty=100)
            _, cost, bad = eng.predict_partition(part, refs, LAM, cur=cur, pred=pred, want_cost=True)
        cur.copy_(dev(cur_np))
        refs[0].copy_(dev(refs_np[0]))
        refs[1].copy_(dev(refs_np[1]))
        for t in [part[k] for k in ("cus", "rows", "ctu_cost")] + [pred, cpyr] + rpyr + list(seeds["mv"].values()):
            t.fill_(-1)
        bad.fill_(5)
        sbad.fill_(5)
        g.replay()
        torch.cuda.synchronize()
        wres = direct.affine_me_poc(cur, refs, LAM, modes=3)
        wseeds = direct.seed_search_wide(cur, refs, LAM, radius=64, levels=2)
        _, wsbad = direct.affine_me_seeded(cur, refs, LAM, wres, wseeds["mv"], modes=3)
        wpart = direct.partition(wres, split_penalty=100)
        wpred, wcost, wbad = direct.predict_partition(wpart, refs, LAM, cur=cur, pred=blank(H, W), want_cost=True)
        torch.cuda.synchronize()
        n = int(wpart["ncus"])
        assert n >= 8 and int(part["ncus"]) == n and int(bad) == 0 and int(wbad) == 0
        assert int(sbad) == 0 and int(wsbad) == 0
        assert torch.equal(cpyr, direct.seed_pyramid(cur))
        for k in wres:
            assert torch.equal(res[k][0], wres[k][0]) and torch.equal(res[k][1], wres[k][1]), k
        assert same(seeds, wseeds)
        assert torch.equal(part["cus"][:n], wpart["cus"][:n]) and torch.equal(part["ctu_cost"], wpart["ctu_cost"])
        # (entries of cost past n may share memory with the seeded call's work buffer, freed during the capture)
        assert torch.equal(pred, wpred) and torch.equal(cost[:n], wcost[:n])
    finally:
        eng.close()
        direct.close()
