"""Seeding the affine search on the GPU (Engine.seed_search,
Engine.affine_search, Engine.affine_me_seeded): bit for
bit against the CPU restatement tests/seed_ref.py and the goldens, 416x240
throughout (8 CTUs, CUs leaving the frame at the right and the bottom)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import bipred_ref as B
import seed_ref as S
import seedpyr_ref as P
from test_gpu_bipred import NAMES, SENTINEL, blank, dev, load
from test_seed import inframe, sample
from vame import mc as M
from vame import seed as V

pytestmark = pytest.mark.gpu

W, H = 416, 240
LAM = S.LAM
INF = S.INF
MV_MAX, MV_MIN = (1 << 17) - 1, -(1 << 17)
P_ = ctypes.c_void_p
RADII = (0, 3, 16, 32)


@pytest.fixture(scope="module")
def eng():
    from vame.engine import Engine
    e = Engine(W, H, 0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def pairs():
    """{name: (refs [n, H, W], cur)}: the shifted-camera pair (two references),
    s416_noise, the tie inputs (seedpyr_ref.stripes and s416_flat) and the
    largest SAD there is (cur all 1023, the reference all 0)."""
    z, flat = load("s416_noise"), load("s416_flat")
    refs, cur = S.shifted_camera(2)
    full = np.full((H, W), 1023, np.uint16)
    return {"shifted": (refs, cur), "noise": (z["ref"][None], z["cur"]), "stripes": P.stripes(W, H),
            "flat": (flat["ref"][None], flat["cur"]), "bound": (np.zeros((1, H, W), np.uint16), full)}


@functools.lru_cache(maxsize=None)
def dev_pair(name):
    refs, cur = pairs()[name]
    return [dev(r) for r in refs], dev(cur)


# ------------------------------------------------------------------ 1. seed_search against seed_cu
@functools.lru_cache(maxsize=None)
def seed_rows(align):
    """About 60 rows of the alignment: every size, CUs on all four frame edges,
    16-wide CUs at x = W - 16 (dx <= 23 cuts the window at radius 32) and rows
    out of the frame."""
    cands = B.frame_candidates(W, H, align)
    inn = inframe(align)
    out = list(sample(align, 36, salt=1))
    out += [c for c in inn if c[1] == W - 16][:4] + [c for c in inn if c[2] + c[4] == H][:4]
    out += [c for c in inn if c[1] == 0][-3:] + [c for c in inn if c[2] == 0][-3:]
    out += [c for c in inn if c[1] + c[3] == W and c[3] >= 32][:3]
    out += [c for c in cands if c[1] + c[3] > W][:3] + [c for c in cands if c[2] + c[4] > H][:3]
    out = sorted(set(out))
    assert 45 <= len(out) <= 70
    assert {(c[3], c[4]) for c in out} >= {(c[3], c[4]) for c in cands}
    return out


@functools.lru_cache(maxsize=None)
def sad_maps(name, r, align):
    """{row: sad_map at radius 32} of the sampled in-frame rows (of a second
    reference: every fourth), computed once."""
    refs, cur = pairs()[name]
    return {row: S.sad_map(refs[r], cur, x, y, w, h, 32) for row, x, y, w, h in seed_rows(align)[::4 if r else 1]
            if x + w <= W and y + h <= H}


def test_the_seed_rows_cover_what_they_should():
    for align in (0, 1):
        rows = seed_rows(align)
        assert any(c[1] == 0 for c in rows) and any(c[2] == 0 for c in rows)
        assert any(c[1] + c[3] == W for c in rows) and any(c[2] + c[4] == H for c in rows)
        assert any(c[1] == W - 16 for c in rows)
        assert any(c[1] + c[3] > W for c in rows) and any(c[2] + c[4] > H for c in rows)
        # at x = W - 16 the rule cuts the window at dx = 23, inside radius 32
        assert all(W + 7 - c[1] == 23 for c in rows if c[1] == W - 16)


@pytest.mark.parametrize("name", ["shifted", "noise"])
@pytest.mark.parametrize("lam", [0.0, LAM])
def test_seed_search_against_reference(eng, name, lam):
    drefs, dcur = dev_pair(name)
    for radius in RADII:
        out = eng.seed_search(dcur, drefs, lam, radius=radius)
        torch.cuda.synchronize()
        for r in range(len(drefs)):
            for align in (0, 1):
                mv, cost = out["mv"][(r, align)].cpu().numpy(), out["cost"][(r, align)].cpu().numpy()
                maps = sad_maps(name, r, align)
                for row, x, y, w, h in seed_rows(align):
                    if row in maps:
                        want = S.seed_from_map(maps[row], x, y, w, h, W, H, radius, lam)
                    elif x + w > W or y + h > H:
                        want = ((0, 0), INF)
                    else:
                        continue
                    assert (tuple(mv[row].tolist()), int(cost[row])) == want, (name, lam, radius, r, align, row)
                # every row out of the frame, every row in it
                cands = B.frame_candidates(W, H, align)
                outside = np.array([c[1] + c[3] > W or c[2] + c[4] > H for c in cands])
                assert (cost[outside] == INF).all() and (mv[outside] == 0).all()
                assert (cost[~outside] < 1 << 40).all() and (cost[~outside] >= 0).all()
                assert (np.abs(mv) <= 16 * radius).all() and (mv % 16 == 0).all()


def test_seed_map_equals_seed_cu():
    refs, cur = pairs()["shifted"]
    for row, x, y, w, h in seed_rows(1)[::9]:
        if row in sad_maps("shifted", 0, 1):
            assert S.seed_from_map(sad_maps("shifted", 0, 1)[row], x, y, w, h, W, H, 3, LAM) == \
                S.seed_cu(refs[0], cur, x, y, w, h, 3, LAM)


# ------------------------------------------------------------------ 1b. ties and the largest SAD
def tie_rows(name, align):
    return seed_rows(align) if name == "stripes" else seed_rows(align)[::2]


@functools.lru_cache(maxsize=None)
def tie_maps(name, align):
    """{row: sad_map at radius 32 against refs[0]} of the sampled in-frame rows."""
    if name == "stripes":
        return sad_maps(name, 0, align)
    refs, cur = pairs()[name]
    return {row: S.sad_map(refs[0], cur, x, y, w, h, 32) for row, x, y, w, h in tie_rows(name, align)
            if x + w <= W and y + h <= H}


@pytest.mark.parametrize("align", [0, 1])
@pytest.mark.parametrize("name", ["stripes", "flat"])
def test_ties_go_to_the_first_of_the_order(eng, name, align):
    """lambda = 0 on inputs whose smallest SAD is attained many times: the
    64-bit minimum of value << 15 | order over the dy workgroups must give
    (0, 0) first, then dy outer, dx inner."""
    drefs, dcur = dev_pair(name)
    for radius in (3, 16, 32):
        out = eng.seed_search(dcur, drefs[:1], 0.0, radius=radius)
        torch.cuda.synchronize()
        mv, cost = out["mv"][(0, align)].cpu().numpy(), out["cost"][(0, align)].cpu().numpy()
        maps = tie_maps(name, align)
        assert len(maps) >= 20
        for row, x, y, w, h in tie_rows(name, align):
            want = S.seed_from_map(maps[row], x, y, w, h, W, H, radius, 0.0) if row in maps else ((0, 0), INF)
            assert (tuple(mv[row].tolist()), int(cost[row])) == want, (name, radius, align, row)
        if name == "flat":  # one value everywhere: every in-frame row stays at (0, 0)
            assert not mv.any() and (cost[[c[0] for c in inframe(align)]] < INF).all()


def test_the_stripe_rows_tie():
    """On the reference alone (the maps are those of the test above): at least
    half of the sampled rows attain their minimum more than once inside every
    radius, and not at (0, 0)."""
    for radius in (3, 16, 32):
        for align in (0, 1):
            maps = tie_maps("stripes", align)
            tied = moved = 0
            for row, x, y, w, h in seed_rows(align):
                if row not in maps:
                    continue
                m = maps[row][32 - radius:33 + radius, 32 - radius:33 + radius]
                d = np.arange(-radius, radius + 1)
                ok = (d[:, None] <= H + 7 - y) & (d[None, :] <= W + 7 - x)
                tied += int((m[ok] == m[ok].min()).sum() > 1)
                moved += S.seed_from_map(maps[row], x, y, w, h, W, H, radius, 0.0)[0] != (0, 0)
            assert 2 * tied >= len(maps) and 2 * moved >= len(maps), (radius, align, tied, moved, len(maps))


@pytest.mark.parametrize("lam", [0.0, LAM])
def test_the_largest_sad_stays_inside_the_key(eng, lam):
    """cur all 1023 against a reference of zeros: every displacement of a CU
    costs 1023 w h, the 128x128 CU 16,760,832 -- just under the 2^25 the key's
    layout relies on -- and (0, 0) comes first."""
    drefs, dcur = dev_pair("bound")
    zero = B.rate(B.bits_of(2, [0] * 6) + 2, lam)
    assert 1023 * 128 * 128 == 16760832 < 1 << 25
    for out in (eng.seed_search(dcur, drefs, lam, radius=32), eng.seed_search_wide(dcur, drefs, lam, radius=128, levels=2)):
        torch.cuda.synchronize()
        for align in (0, 1):
            cands = B.frame_candidates(W, H, align)
            want = np.array([1023 * w * h + zero if x + w <= W and y + h <= H else INF for _, x, y, w, h in cands], np.int64)
            assert not out["mv"][(0, align)].any()
            np.testing.assert_array_equal(out["cost"][(0, align)].cpu().numpy(), want)
        assert (out["cost"][(0, 0)] == 16760832 + zero).sum() == 3  # the 128x128 CUs of the three CTUs wholly in the frame


def raw_seed(eng, name, mask, radius, mv, cost, nrefs=None, h=None, null=(), lam=LAM):
    from vame._lib import SeedResult, lib
    drefs, dcur = dev_pair(name)
    sr = SeedResult()
    for (r, a), t in mv.items():
        sr.mv[r][a] = t.data_ptr()
    for (r, a), t in cost.items():
        sr.cost[r][a] = t.data_ptr()
    ptrs = (P_ * 4)(*[t.data_ptr() for t in drefs])
    arg = {"cur": P_(dcur.data_ptr()), "refs": ptrs, "out": ctypes.byref(sr)}
    for k in null:
        arg[k] = None
    rc = lib().vame_seed_search(h or eng._h, arg["cur"], arg["refs"], len(drefs) if nrefs is None else nrefs, lam, mask,
                                radius, arg["out"], None)
    torch.cuda.synchronize()
    return rc


def seed_sentinels(eng, nrefs):
    mv = {(r, a): torch.full((eng.n_cus(a), 2), SENTINEL, dtype=torch.int32).cuda() for r in range(nrefs) for a in (0, 1)}
    cost = {(r, a): torch.full((eng.n_cus(a),), SENTINEL, dtype=torch.int64).cuda() for r in range(nrefs) for a in (0, 1)}
    return mv, cost


@pytest.mark.parametrize("mask", [1, 2])
def test_alignments_outside_the_mask_are_untouched(eng, mask):
    drefs, dcur = dev_pair("shifted")
    both = eng.seed_search(dcur, drefs, LAM, radius=3)
    mv, cost = seed_sentinels(eng, 2)
    assert raw_seed(eng, "shifted", mask, 3, mv, cost) == 0
    on, off = (0, 1) if mask == 1 else (1, 0)
    for r in (0, 1):
        assert torch.equal(mv[(r, on)], both["mv"][(r, on)]) and torch.equal(cost[(r, on)], both["cost"][(r, on)])
        assert (mv[(r, off)] == SENTINEL).all() and (cost[(r, off)] == SENTINEL).all()
    # through the Python view: only the mask's keys, written into given arrays
    one = eng.seed_search(dcur, drefs, LAM, radius=3, aligns=mask, out={"mv": mv, "cost": cost})
    assert one["mv"] is mv


# ------------------------------------------------------------------ 2. the seed's cost is affine_mc's block
def test_seed_cost_is_the_sad_of_affine_mc_plus_rate(eng):
    drefs, dcur = dev_pair("shifted")
    _, cur = pairs()["shifted"]
    out = eng.seed_search(dcur, drefs, LAM, radius=16)
    n = 0
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
    assert n >= 38


# ------------------------------------------------------------------ 3. affine_search against search_cu
def search_cases():
    """About 40 descriptors on the shifted-camera pair: every size with its
    integer seed (2-CP) and the 3-CP start derived from it, fractional and
    non-translational starts, a spread start, components at +-2^17, starts
    beyond clip_mv's bounds, positions that are multiples of 4 only, a 2-CP
    descriptor with an LB (kept)."""
    refs, cur = pairs()["shifted"]
    out, sizes = [], set()
    for k, (row, x, y, w, h) in enumerate(sample(0, 12, salt=2) + sample(1, 8, salt=2)[::2]):
        sizes.add((w, h))
        r = k & 1
        mv, _ = S.seed_cu(refs[r], cur, x, y, w, h, 16, LAM)
        c2 = [mv[0], mv[1], mv[0], mv[1], 0, 0]
        out.append([x, y, w, h, r, 2] + c2)
        if k % 2 == 0:
            out.append([x, y, w, h, r, 3] + S.seed_3cp(c2, x, y, w, h, W, H))
    assert len(sizes) == 12
    rng = np.random.default_rng(15)
    for x, y, w, h, ncp in ((64, 64, 32, 32, 2), (128, 0, 64, 64, 3), (0, 128, 128, 64, 2), (256, 96, 16, 16, 3),
                            (288, 112, 128, 128, 2), (192, 176, 64, 16, 3)):
        c = (np.array([-176, 96] * 3) + rng.integers(-25, 26, 6)).tolist()  # fractional, non-translational
        out.append([x, y, w, h, 0, ncp] + c)
    out.append([128, 128, 16, 16, 0, 3, 0, 0, 4000, 0, 0, 4000])                      # spread
    out.append([160, 96, 16, 16, 0, 2, MV_MIN, MV_MAX, MV_MIN, MV_MAX, 0, 0])          # the range's ends
    out.append([176, 96, 32, 32, 1, 3, 10, 10, 12, 9, MV_MAX, MV_MIN])
    out.append([0, 0, 32, 32, 0, 2, -2500, -2400, -2480, -2390, 0, 0])                # beyond clip_mv's bounds
    out.append([384, 208, 32, 32, 1, 3, 900, 700, 910, 690, 905, 720])
    for x, y, w, h, ncp in ((20, 36, 16, 16, 2), (100, 52, 32, 16, 3), (244, 132, 16, 32, 2), (332, 172, 64, 64, 3),
                            (4, 108, 128, 128, 2)):                                      # multiples of 4 only
        out.append([x, y, w, h, 1, ncp] + (np.array([-170, 100] * 3) + rng.integers(-12, 13, 6)).tolist())
    out.append([96, 32, 32, 32, 0, 2, -176, 96, -170, 99, 555, -444])                   # a 2-CP LB stays
    return out


@functools.lru_cache(maxsize=None)
def search_reference(extra):
    refs, cur = pairs()["shifted"]
    return [S.search_cu(refs[d[4]], cur, d[0], d[1], d[2], d[3], d[5], d[6:12], LAM, extra) for d in search_cases()]


def want_search(extra):
    cs = search_cases()
    want = [d[:6] + (cp if d[5] == 3 else cp[:4] + d[10:12]) for d, (cp, _) in zip(cs, search_reference(extra))]
    return np.array(want, np.int32), np.array([c for _, c in search_reference(extra)], np.int64)


def test_the_search_cases_cover_what_they_should():
    cs = search_cases()
    assert 38 <= len(cs) <= 48
    assert {d[5] for d in cs} == {2, 3} and any(d[0] % 16 for d in cs)
    moved = [d[6:12] != w[6:12].tolist() for d, w in zip(cs, want_search(0)[0])]
    assert sum(moved) >= 20
    assert (want_search(1)[1] <= want_search(0)[1]).all()


@pytest.mark.parametrize("extra", [0, 1])
def test_affine_search_against_reference(eng, extra):
    drefs, dcur = dev_pair("shifted")
    cus = torch.tensor(search_cases(), dtype=torch.int32).cuda()
    out, cost, bad = eng.affine_search(cus, drefs, dcur, LAM, extra=extra)
    _, mc_cost, bad2 = eng.affine_mc(out, drefs, LAM, cur=dcur, want_cost=True)
    torch.cuda.synchronize()
    want_out, want_cost = want_search(extra)
    assert int(bad) == 0 and int(bad2) == 0
    got_out, got_cost = out.cpu().numpy(), cost.cpu().numpy()
    for i in range(len(want_cost)):
        assert got_out[i].tolist() == want_out[i].tolist() and got_cost[i] == want_cost[i], \
            (i, search_cases()[i], got_out[i].tolist(), want_out[i].tolist(), int(got_cost[i]), int(want_cost[i]))
    assert torch.equal(mc_cost, cost)  # bit for bit vame_affine_mc's cost of out


def raw_search(eng, cus, count, extra, out, cost, bad, nrefs=2, h=None, null=(), n=None):
    from vame._lib import lib
    drefs, dcur = dev_pair("shifted")
    ptrs = (P_ * 2)(*[r.data_ptr() for r in drefs])
    ncus = None if count is None else torch.tensor(count, dtype=torch.int32).cuda()
    arg = {"cur": P_(dcur.data_ptr()), "refs": ptrs, "cus": P_(cus.data_ptr()), "out": P_(out.data_ptr()),
           "cost": P_(cost.data_ptr()), "bad": P_(bad.data_ptr())}
    for k in null:
        arg[k] = None
    rc = lib().vame_affine_search(h or eng._h, arg["cur"], arg["refs"], nrefs, arg["cus"], cus.shape[0] if n is None else n,
                                  None if ncus is None else P_(ncus.data_ptr()), LAM, extra, arg["out"], arg["cost"],
                                  arg["bad"], None)
    torch.cuda.synchronize()
    return rc


def search_sentinels(n):
    return (torch.full((n, 12), SENTINEL, dtype=torch.int32).cuda(), torch.full((n,), SENTINEL, dtype=torch.int64).cuda(),
            torch.zeros((), dtype=torch.int32).cuda())


def test_invalid_descriptor_device_count_and_in_place(eng):
    drefs, dcur = dev_pair("shifted")
    cs = search_cases()
    pick = [cs[i] for i in (0, 1, 5, 9, 20, 30)]
    w_out, w_cost, w_bad = eng.affine_search(torch.tensor(pick, dtype=torch.int32).cuda(), drefs, dcur, LAM)
    torch.cuda.synchronize()
    assert int(w_bad) == 0
    garbage = [-5, 3, 17, 9, 9, 7, 1 << 20, 0, 0, 0, 0, 0]
    # an invalid descriptor in the middle: copied through, cost 0, its neighbours as if alone
    mix = torch.tensor(pick[:3] + [garbage] + pick[3:], dtype=torch.int32).cuda()
    out, cost, bad = eng.affine_search(mix, drefs, dcur, LAM)
    torch.cuda.synchronize()
    keep = [0, 1, 2, 4, 5, 6]
    assert int(bad) == 1 and torch.equal(out[keep], w_out) and torch.equal(cost[keep], w_cost)
    assert out[3].tolist() == garbage and int(cost[3]) == 0
    # a device count below the capacity, garbage past it: the tail untouched, bad stays 0
    cus = torch.tensor(pick + [garbage] * 3, dtype=torch.int32).cuda()
    out, cost, bad = search_sentinels(9)
    assert raw_search(eng, cus, 6, 0, out, cost, bad) == 0
    assert int(bad) == 0 and torch.equal(out[:6], w_out) and torch.equal(cost[:6], w_cost)
    assert (out[6:] == SENTINEL).all() and (cost[6:] == SENTINEL).all()
    for count in (0, -3):
        out, cost, bad = search_sentinels(9)
        assert raw_search(eng, cus, count, 0, out, cost, bad) == 0
        assert int(bad) == 0 and (out == SENTINEL).all() and (cost == SENTINEL).all()
    out, cost, bad = search_sentinels(9)
    assert raw_search(eng, cus, 1000, 0, out, cost, bad) == 0
    assert int(bad) == 1 and torch.equal(out[:6], w_out) and torch.equal(out[6:], cus[6:]) and (cost[6:] == 0).all()
    # through Engine.affine_search(ncus=), in place
    same = cus.clone()
    o2, c2, bad = eng.affine_search(same, drefs, dcur, LAM, ncus=torch.tensor(4, dtype=torch.int32).cuda(), out=same)
    torch.cuda.synchronize()
    assert o2 is same and int(bad) == 0 and torch.equal(same[:4], w_out[:4]) and torch.equal(same[4:], cus[4:])
    assert torch.equal(c2[:4], w_cost[:4])


# ------------------------------------------------------------------ 4. zero starts are the goldens
def test_zero_starts_equal_the_goldens(eng):
    z = load("s416_qp32_poc2_ref0")
    drefs, dcur, lam = [dev(z["ref"])], dev(z["cur"]), float(z["lam"])
    total = 0
    for align in (0, 1):
        n = eng.n_cus(align)
        cus, rows = M.cus_from_result(W, H, align, 2, torch.zeros((n, 6), dtype=torch.int32).cuda())
        out, cost, bad = eng.affine_search(cus, drefs, dcur, lam)
        torch.cuda.synchronize()
        rows_np = rows.cpu().numpy()
        g2c, g2p = z[NAMES[2 * align] + "_cost"], np.asarray(z[NAMES[2 * align] + "_cpmv"])[:, -6:]
        assert int(bad) == 0
        np.testing.assert_array_equal(cost.cpu().numpy(), g2c[rows_np])
        np.testing.assert_array_equal(out.cpu().numpy()[:, 6:], g2p[rows_np])
        # the 3-CP run from seed_3cp of the 2-CP winners
        geo = cus.cpu().numpy()
        start = [S.seed_3cp(g2p[row], int(d[0]), int(d[1]), int(d[2]), int(d[3]), W, H) for row, d in zip(rows_np, geo)]
        cus3 = cus.clone()
        cus3[:, 5] = 3
        cus3[:, 6:] = torch.tensor(start, dtype=torch.int32).cuda()
        out3, cost3, bad3 = eng.affine_search(cus3, drefs, dcur, lam)
        torch.cuda.synchronize()
        g3c, g3p = z[NAMES[2 * align + 1] + "_cost"], np.asarray(z[NAMES[2 * align + 1] + "_cpmv"])[:, -6:]
        assert int(bad3) == 0
        np.testing.assert_array_equal(cost3.cpu().numpy(), g3c[rows_np])
        np.testing.assert_array_equal(out3.cpu().numpy()[:, 6:], g3p[rows_np])
        total += 2 * len(rows_np)
    assert total >= 2700


# ------------------------------------------------------------------ 5. affine_me_seeded
def clone_result(res):
    return {k: (c.clone(), p.clone()) for k, (c, p) in res.items()}


@functools.lru_cache(maxsize=None)
def seeded_case():
    """The shifted-camera pair's search result (two references, modes 3), its
    seeds at radius 16 and the improved result, on the device, computed once."""
    from vame.engine import Engine
    e = Engine(W, H, 0)
    try:
        drefs, dcur = dev_pair("shifted")
        base = e.affine_me_poc(dcur, drefs, LAM, modes=3)
        seeds = e.seed_search(dcur, drefs, LAM, radius=16)["mv"]
        res, bad = e.affine_me_seeded(dcur, drefs, LAM, clone_result(base), seeds, modes=3)
        torch.cuda.synchronize()
        return base, seeds, res, int(bad)
    finally:
        e.close()


def test_zero_seeds_change_nothing(eng):
    drefs, dcur = dev_pair("shifted")
    base = seeded_case()[0]
    zero = {(r, a): torch.zeros((eng.n_cus(a), 2), dtype=torch.int32).cuda() for r in (0, 1) for a in (0, 1)}
    res, bad = eng.affine_me_seeded(dcur, drefs, LAM, clone_result(base), zero, modes=3)
    torch.cuda.synchronize()
    assert int(bad) == 0
    for k in base:
        assert torch.equal(res[k][0], base[k][0]) and torch.equal(res[k][1], base[k][1])


def test_seeded_equals_the_composition(eng):
    drefs, dcur = dev_pair("shifted")
    base, seeds, res, bad = seeded_case()
    assert bad == 0
    improved = 0
    for r in (0, 1):
        for align in (0, 1):
            cus, rows = V.cus_from_seeds(W, H, align, seeds[(r, align)], ref=r)
            assert len(rows) >= 0.8 * len(inframe(align))
            o2, c2, b2 = eng.affine_search(cus, drefs, dcur, LAM)
            torch.cuda.synchronize()
            d2 = o2.cpu().numpy()
            start = [S.seed_3cp(d[6:10], int(d[0]), int(d[1]), int(d[2]), int(d[3]), W, H) for d in d2]
            cus3 = o2.clone()
            cus3[:, 5] = 3
            cus3[:, 6:] = torch.tensor(start, dtype=torch.int32).cuda()
            o3, c3, b3 = eng.affine_search(cus3, drefs, dcur, LAM)
            torch.cuda.synchronize()
            assert int(b2) == 0 and int(b3) == 0
            for m, o, c in ((0, o2, c2), (1, o3, c3)):
                bc, bp = base[(r, NAMES[2 * align + m])]
                wc, wp = bc.clone(), bp.clone()
                take = c < bc[rows]
                wc[rows[take]] = c[take]
                new = torch.cat([torch.full((len(rows), 1), 2 + m, dtype=torch.int32).cuda(), o[:, 6:]], 1)
                if m == 0:
                    new[:, 5:] = 0
                wp[rows[take]] = new[take]
                gc, gp = res[(r, NAMES[2 * align + m])]
                assert torch.equal(gc, wc) and torch.equal(gp, wp), (r, align, m)
                assert (gc <= bc).all()  # no cost rose
                improved += int(take.sum())
    assert improved >= 3000


def test_seeded_against_reference():
    refs, cur = pairs()["shifted"]
    base, seeds, res, _ = seeded_case()
    n = 0
    for align in (0, 1):
        b = {m: (base[(0, NAMES[2 * align + m])][0].cpu().numpy(), base[(0, NAMES[2 * align + m])][1].cpu().numpy())
             for m in (0, 1)}
        g = {m: (res[(0, NAMES[2 * align + m])][0].cpu().numpy(), res[(0, NAMES[2 * align + m])][1].cpu().numpy())
             for m in (0, 1)}
        seed = seeds[(0, align)].cpu().numpy()
        for row, x, y, w, h in sample(align, 12, salt=5):
            want = S.merged(refs[0], cur, x, y, w, h, tuple(seed[row].tolist()), LAM, (b[0][0][row], b[0][1][row][1:]),
                            (b[1][0][row], b[1][1][row][1:]))
            for m in (0, 1):
                assert int(g[m][0][row]) == want[m][0] and g[m][1][row].tolist() == [2 + m] + want[m][1], (align, row, m)
            n += 1
    assert n >= 20


def test_out_of_range_seed_and_partition(eng):
    drefs, dcur = dev_pair("shifted")
    base, seeds, res, _ = seeded_case()
    # an out-of-range seed sets bad and leaves its row unchanged; the others as before
    row = inframe(0)[40][0]
    odd = {k: v.clone() for k, v in seeds.items()}
    assert odd[(1, 0)][row].tolist() != [0, 0]
    odd[(1, 0)][row] = torch.tensor([1 << 17, 16], dtype=torch.int32)
    got, bad = eng.affine_me_seeded(dcur, drefs, LAM, clone_result(base), odd, modes=3)
    torch.cuda.synchronize()
    assert int(bad) == 1
    for k in res:
        c, p = res[k][0].clone(), res[k][1].clone()
        if k[0] == 1 and k[1].startswith("FULL"):
            c[row], p[row] = base[k][0][row], base[k][1][row]
        assert torch.equal(got[k][0], c) and torch.equal(got[k][1], p), k
    # 2-CP only: the 3-CP arrays are not needed and the 2-CP ones equal those of modes 3
    base1 = {k: v for k, v in clone_result(base).items() if k[1].endswith("2CP")}
    got1, bad = eng.affine_me_seeded(dcur, drefs, LAM, base1, seeds, modes=1)
    torch.cuda.synchronize()
    assert int(bad) == 0 and all(torch.equal(got1[k][0], res[k][0]) and torch.equal(got1[k][1], res[k][1]) for k in got1)
    # the partition on better winners: no CTU costs more
    before, after = eng.partition(base), eng.partition(res)
    torch.cuda.synchronize()
    assert (after["ctu_cost"] <= before["ctu_cost"]).all() and (after["ctu_cost"] < before["ctu_cost"]).any()


# ------------------------------------------------------------------ 6. one graph
def test_seeded_search_to_prediction_in_one_graph():
    """affine_me_poc -> seed_search -> affine_me_seeded -> partition ->
    predict_partition captured on a fresh engine, replayed after the inputs
    were overwritten: equal to direct calls on a second engine."""
    from vame.engine import Engine
    a = load("s416_noise")
    refs_np, cur_np = pairs()["shifted"]
    eng, direct = Engine(W, H, 0), Engine(W, H, 0)
    try:
        cur, refs = dev(a["cur"]), [dev(a["ref"]), dev(np.roll(a["ref"], 2, 1))]
        res = eng.alloc_poc(2, 3)
        pred = blank(H, W)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            eng.affine_me_poc(cur, refs, LAM, modes=3, out=res)
            seeds = eng.seed_search(cur, refs, LAM, radius=16)
            _, sbad = eng.affine_me_seeded(cur, refs, LAM, res, seeds["mv"], modes=3)
            part = eng.partition(res, split_penalty=100)
            _, cost, bad = eng.predict_partition(part, refs, LAM, cur=cur, pred=pred, want_cost=True)
        cur.copy_(dev(cur_np))
        refs[0].copy_(dev(refs_np[0]))
        refs[1].copy_(dev(refs_np[1]))
        for t in [part[k] for k in ("cus", "rows", "ctu_cost")] + [pred] + list(seeds["mv"].values()):
            t.fill_(-1)
        bad.fill_(5)
        sbad.fill_(5)
        g.replay()
        torch.cuda.synchronize()
        wres = direct.affine_me_poc(cur, refs, LAM, modes=3)
        plain = direct.partition(clone_result(wres), split_penalty=100)
        wseeds = direct.seed_search(cur, refs, LAM, radius=16)
        _, wsbad = direct.affine_me_seeded(cur, refs, LAM, wres, wseeds["mv"], modes=3)
        wpart = direct.partition(wres, split_penalty=100)
        wpred, wcost, wbad = direct.predict_partition(wpart, refs, LAM, cur=cur, pred=blank(H, W), want_cost=True)
        torch.cuda.synchronize()
        n = int(wpart["ncus"])
        assert n >= 8 and int(part["ncus"]) == n and int(bad) == 0 and int(wbad) == 0
        assert int(sbad) == 0 and int(wsbad) == 0
        for k in wres:
            assert torch.equal(res[k][0], wres[k][0]) and torch.equal(res[k][1], wres[k][1]), k
        for k in wseeds["mv"]:
            assert torch.equal(seeds["mv"][k], wseeds["mv"][k]) and torch.equal(seeds["cost"][k], wseeds["cost"][k])
        assert torch.equal(part["cus"][:n], wpart["cus"][:n]) and torch.equal(part["ctu_cost"], wpart["ctu_cost"])
        # (entries of cost past n may share memory with the seeded call's work buffer, freed during the capture)
        assert torch.equal(pred, wpred) and torch.equal(cost[:n], wcost[:n])
        assert (wpart["ctu_cost"] < plain["ctu_cost"]).any()
    finally:
        eng.close()
        direct.close()


# ------------------------------------------------------------------ 7. errors write nothing
def test_seed_search_errors_write_nothing(eng):
    mv, cost = seed_sentinels(eng, 2)

    def untouched():
        assert all((t == SENTINEL).all() for t in mv.values()) and all((t == SENTINEL).all() for t in cost.values())

    assert raw_seed(eng, "shifted", 3, 16, mv, cost, nrefs=0) == -1 and raw_seed(eng, "shifted", 3, 16, mv, cost, nrefs=5) == -1
    for mask in (0, 4, 7):
        assert raw_seed(eng, "shifted", mask, 16, mv, cost) == -1
    for radius in (-1, 33):
        assert raw_seed(eng, "shifted", 3, radius, mv, cost) == -1
    for k in ("cur", "refs", "out"):
        assert raw_seed(eng, "shifted", 3, 16, mv, cost, null=(k,)) == -1, k
    assert raw_seed(eng, "shifted", 3, 16, {k: v for k, v in mv.items() if k != (1, 1)}, cost) == -1   # a NULL output
    assert raw_seed(eng, "shifted", 1, 16, mv, {k: v for k, v in cost.items() if k != (0, 0)}) == -1
    untouched()
    # a misaligned frame
    from vame._lib import SeedResult, lib
    drefs, dcur = dev_pair("shifted")
    sr = SeedResult()
    for k in mv:
        sr.mv[k[0]][k[1]], sr.cost[k[0]][k[1]] = mv[k].data_ptr(), cost[k].data_ptr()
    ptrs = (P_ * 2)(*[t.data_ptr() for t in drefs])
    assert lib().vame_seed_search(eng._h, P_(dcur.data_ptr() + 2), ptrs, 2, LAM, 3, 16, ctypes.byref(sr), None) == -1
    ptrs = (P_ * 2)(drefs[0].data_ptr(), drefs[1].data_ptr() + 2)
    assert lib().vame_seed_search(eng._h, P_(dcur.data_ptr()), ptrs, 2, LAM, 3, 16, ctypes.byref(sr), None) == -1
    torch.cuda.synchronize()
    untouched()
    for kw in (dict(radius=33), dict(radius=-1), dict(aligns=0), dict(aligns=4),
               dict(out={"mv": {}, "cost": {}}), dict(out={"mv": cost, "cost": cost})):
        with pytest.raises(ValueError):
            eng.seed_search(dcur, drefs, LAM, **kw)
    with pytest.raises(ValueError):
        eng.seed_search(dcur, [], LAM)
    # PROF does not enter
    from vame.engine import Engine
    prof = Engine(W, H, 0)
    try:
        prof.set_prof(True)
        a = prof.seed_search(dcur, drefs, LAM, radius=3)
        b = eng.seed_search(dcur, drefs, LAM, radius=3)
        torch.cuda.synchronize()
        assert all(torch.equal(a["mv"][k], b["mv"][k]) and torch.equal(a["cost"][k], b["cost"][k]) for k in b["mv"])
    finally:
        prof.close()


def test_affine_search_errors_write_nothing(eng):
    from vame.engine import Engine
    drefs, dcur = dev_pair("shifted")
    cus = torch.tensor(search_cases()[:6], dtype=torch.int32).cuda()
    out, cost, bad = search_sentinels(6)

    def untouched():
        assert (out == SENTINEL).all() and (cost == SENTINEL).all() and int(bad) == 0

    assert raw_search(eng, cus, None, 65, out, cost, bad) == -1 and raw_search(eng, cus, None, -1, out, cost, bad) == -1
    assert raw_search(eng, cus, None, 0, out, cost, bad, nrefs=0) == -1
    assert raw_search(eng, cus, None, 0, out, cost, bad, nrefs=5) == -1
    for k in ("cur", "refs", "cus", "out", "cost", "bad"):
        assert raw_search(eng, cus, None, 0, out, cost, bad, null=(k,)) == -1, k
    for n in (-1, (1 << 20) + 1):
        assert raw_search(eng, cus, None, 0, out, cost, bad, n=n) == -1
    assert raw_search(eng, cus, None, 0, out, cost, bad, n=0) == 0  # a no-op
    untouched()
    prof = Engine(W, H, 0)
    try:
        prof.set_prof(True)
        assert raw_search(eng, cus, None, 0, out, cost, bad, h=prof._h) == -4
        untouched()
        with pytest.raises(Exception):
            prof.affine_search(cus, drefs, dcur, LAM)
        base = prof.alloc_poc(2, 3)
        for c, p in base.values():
            c.fill_(SENTINEL)
            p.fill_(SENTINEL)
        seeds = {(r, a): torch.full((prof.n_cus(a), 2), 16, dtype=torch.int32).cuda() for r in (0, 1) for a in (0, 1)}
        with pytest.raises(Exception):
            prof.affine_me_seeded(dcur, drefs, LAM, base, seeds, modes=3)
        torch.cuda.synchronize()
        assert all((c == SENTINEL).all() and (p == SENTINEL).all() for c, p in base.values())
        prof.set_prof(False)
        assert raw_search(eng, cus, None, 0, out, cost, bad, h=prof._h) == 0
        assert (cost != SENTINEL).all() and int(bad) == 0
    finally:
        prof.close()
    for kw in (dict(extra=65), dict(extra=-1), dict(out=torch.empty((5, 12), dtype=torch.int32).cuda()),
               dict(cost=torch.empty(6, dtype=torch.int32).cuda()), dict(ncus=torch.tensor(3).cuda())):
        with pytest.raises(ValueError):
            eng.affine_search(cus, drefs, dcur, LAM, **kw)
    with pytest.raises(ValueError):
        eng.affine_search(torch.zeros((6, 20), dtype=torch.int32).cuda(), drefs, dcur, LAM)


def test_affine_me_seeded_errors_write_nothing(eng):
    from vame._lib import PocResult, lib
    drefs, dcur = dev_pair("shifted")
    res = eng.alloc_poc(2, 3)
    for c, p in res.values():
        c.fill_(SENTINEL)
        p.fill_(SENTINEL)
    seeds = {(r, a): torch.full((eng.n_cus(a), 2), 16, dtype=torch.int32).cuda() for r in (0, 1) for a in (0, 1)}
    nbytes = lib().vame_seeded_work_bytes(eng._h, 2, 3)
    assert nbytes > 0 and lib().vame_seeded_work_bytes(eng._h, 2, 1) < nbytes
    assert lib().vame_seeded_work_bytes(eng._h, 2, 1 | 4) < lib().vame_seeded_work_bytes(eng._h, 2, 1)
    assert lib().vame_seeded_work_bytes(eng._h, 0, 3) == 0 and lib().vame_seeded_work_bytes(eng._h, 2, 2) == 0
    work = torch.full((nbytes // 8 + 1,), SENTINEL, dtype=torch.int64).cuda()
    bad = torch.zeros((), dtype=torch.int32).cuda()
    pr = PocResult()
    for (r, name), (c, p) in res.items():
        pr.cost[r][NAMES.index(name)], pr.cpmvs[r][NAMES.index(name)] = c.data_ptr(), p.data_ptr()
    sp = ((P_ * 2) * 4)()
    for (r, a), t in seeds.items():
        sp[r][a] = t.data_ptr()
    ptrs = (P_ * 2)(*[t.data_ptr() for t in drefs])

    def call(nrefs=2, modes=3, extra=0, cur=dcur.data_ptr(), refs=ptrs, seed=sp, result=pr, w=work.data_ptr(),
             wb=nbytes, b=bad.data_ptr()):
        rc = lib().vame_affine_me_seeded(eng._h, P_(cur) if cur else None, refs, nrefs, LAM, modes, extra, seed,
                                         ctypes.byref(result) if result is not None else None, P_(w) if w else None,
                                         wb, P_(b) if b else None, None)
        torch.cuda.synchronize()
        return rc

    assert call(nrefs=0) == -1 and call(nrefs=5) == -1 and call(modes=2) == -1 and call(modes=16 | 1) == -1
    assert call(extra=-1) == -1 and call(extra=65) == -1 and call(cur=0) == -1 and call(refs=None) == -1
    assert call(seed=None) == -1 and call(result=None) == -1 and call(w=0) == -1 and call(b=0) == -1
    assert call(wb=nbytes - 1) == -1 and call(cur=dcur.data_ptr() + 2) == -1
    hole = PocResult()
    ctypes.memmove(ctypes.byref(hole), ctypes.byref(pr), ctypes.sizeof(pr))
    hole.cpmvs[1][3] = None
    assert call(result=hole) == -1
    nos = ((P_ * 2) * 4)()
    ctypes.memmove(nos, sp, ctypes.sizeof(sp))
    nos[1][1] = None
    assert call(seed=nos) == -1
    assert all((c == SENTINEL).all() and (p == SENTINEL).all() for c, p in res.values())
    assert (work == SENTINEL).all() and int(bad) == 0
    # the Python layer refuses the same before any call
    for kw in (dict(modes=2), dict(modes=17), dict(extra=65)):
        with pytest.raises(ValueError):
            eng.affine_me_seeded(dcur, drefs, LAM, res, seeds, **kw)
    with pytest.raises(ValueError):
        eng.affine_me_seeded(dcur, drefs, LAM, res, {k: v for k, v in seeds.items() if k != (0, 1)})
    with pytest.raises(ValueError):
        eng.affine_me_seeded(dcur, drefs[:1], LAM, res, seeds)
    with pytest.raises(ValueError):
        eng.affine_me_seeded(dcur, drefs, LAM, {k: v for k, v in res.items() if k != (1, "HALF_3CP")}, seeds)


# ------------------------------------------------------------------ 8. determinism
def test_two_calls_agree(eng):
    drefs, dcur = dev_pair("shifted")
    a, b = eng.seed_search(dcur, drefs, LAM, radius=32), eng.seed_search(dcur, drefs, LAM, radius=32)
    base, seeds, res, _ = seeded_case()
    again, _ = eng.affine_me_seeded(dcur, drefs, LAM, clone_result(base), seeds, modes=3)
    torch.cuda.synchronize()
    assert all(torch.equal(a["mv"][k], b["mv"][k]) and torch.equal(a["cost"][k], b["cost"][k]) for k in a["mv"])
    assert all(torch.equal(again[k][0], res[k][0]) and torch.equal(again[k][1], res[k][1]) for k in res)
