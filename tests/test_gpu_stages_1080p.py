"""The stages after the search on the 1920x1080 frame (DESIGN.md sections 11
to 16): bit for bit against the CPU restatements.  1080 is the one accepted
height that is no multiple of 16: the bottom CTU row (y0 = 1024) is 56 rows
tall, block row 6 is its last, and 22 half-aligned candidates per CTU (330
rows, 'the odd-cut rows') end exactly on frame row 1080.

The frames are synthesized: the reconstructions of POC 0..3 as references, cur
is POC 4 seen through a window moved by SHIFT = (-9, +24) samples (all cut from
frames 64 samples larger on every side, as seed_ref.shifted_camera does).

Two things the bottom row cannot show, proved in the coverage functions
below instead of assumed:
  * no winner of the exhaustive search has Dy == 23 on an odd-cut row: for
    Dy >= 15 every row of the displaced block clamps to frame row 1079, so the
    SAD of Dy = 15 .. 23 is one value, the rate does not fall with |Dy|, and the
    first minimum of the order is never the last.  What is asserted: at least
    20 odd-cut rows attain their minimum SAD on the line Dy == 23 as well (the
    order alone decides against it), and the cut lies inside the window;
  * no leaf of a partition ends on row 1080: leaves start and end on the 16
    grid of their CTU, 1080 = 1024 + 56.  The bottom CTUs' leaves end at 1072
    and rows 1072 .. 1079 are holes, so the predicted frame keeps its blank
    there (and only there)."""
import functools

import numpy as np
import pytest
import torch

import bipred_ref as B
import birefine_ref as F
import partition_ref as R
import seed_ref as S
import seedpyr_ref as P
from test_gpu_bipred import NAMES, blank, dev, result_arrays
from vame import bipred as VB
from vame import mc as M
from vame import seed as V

pytestmark = pytest.mark.gpu

W, H = 1920, 1080
SHIFT = (-9, 24)
LAM = S.LAM
INF = S.INF
PER = (201, 284)
BOTTOM, INTERIOR, CORNER = (120, 127, 134), (52, 66), (14,)
SIZES = ((416, 240), (832, 480), (1280, 720), (1920, 1080), (3840, 2160))


@pytest.fixture(scope="module")
def eng():
    from vame.engine import Engine
    e = Engine(W, H, 0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def frames():
    """(refs [4, H, W], cur)."""
    from vame import synth
    m = 64
    orig, recon = synth.synth_sequence(W + 2 * m, H + 2 * m, 4)
    refs = np.ascontiguousarray(recon[:, m:m + H, m:m + W])
    cur = np.ascontiguousarray(orig[3][m + SHIFT[1]:m + SHIFT[1] + H, m + SHIFT[0]:m + SHIFT[0] + W])
    return refs, cur


@functools.lru_cache(maxsize=None)
def dev_frames():
    refs, cur = frames()
    return [dev(r) for r in refs], dev(cur)


@functools.lru_cache(maxsize=None)
def cands(align):
    return B.frame_candidates(W, H, align)


def inside(c):
    return c[1] + c[3] <= W and c[2] + c[4] <= H


@functools.lru_cache(maxsize=None)
def outside_mask(align):
    return np.array([not inside(c) for c in cands(align)])


@functools.lru_cache(maxsize=None)
def odd_rows():
    """The half-aligned candidates that end on frame row 1080."""
    return [c for c in cands(1) if c[2] + c[4] == H and inside(c)]


def ctu_rows(ctu, align):
    return cands(align)[ctu * PER[align]:(ctu + 1) * PER[align]]


def test_the_odd_cut_rows_are_what_the_tables_say():
    odd = odd_rows()
    assert len(odd) == 330 and not [c for c in cands(0) if c[2] + c[4] == H]
    assert all(c[2] == 1064 and c[4] == 16 and H + 7 - c[2] == 23 for c in odd)
    assert {c[0] // PER[1] for c in odd} == set(range(120, 135)) and len({c[0] % PER[1] for c in odd}) == 22
    for a in (0, 1):
        assert all(c[0] // PER[a] == ctu for ctu in BOTTOM + INTERIOR + CORNER for c in ctu_rows(ctu, a))
    # no node of the partition ends on CTU row 56: leaves end at 1072, rows 1072 .. 1079 are holes
    ends = {n[1] + n[3] for n in R.leaf_candidates()}
    assert 56 not in ends and 48 in ends


# ------------------------------------------------------------------ 1. the pyramid
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pyramid_at_every_accepted_size(size):
    from vame._lib import lib
    from vame.engine import Engine
    w, h = size
    f = np.random.default_rng(1700 + h).integers(0, 1024, (h, w)).astype(np.uint16)
    f[-4:, -8:], f[:4, :8] = 1023, 0
    e = Engine(w, h, 0)
    try:
        assert lib().vame_seed_pyramid_bytes(e._h) == 2 * ((w // 2) * (h // 2) + (w // 4) * (h // 4))
        got = e.seed_pyramid(dev(f))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(got.cpu().numpy().view(np.uint16), P.packed(f))
    finally:
        e.close()


# ------------------------------------------------------------------ 2. seed_search
def seed_groups():
    """{name: [(align, candidate)]}: the odd-cut rows in three parts; the other
    in-frame rows of three bottom-row CTUs, per alignment; the rows of two
    interior CTUs and of the top-right one, per alignment in two or three parts."""
    odd = odd_rows()
    out = {f"odd{k}": [(1, c) for c in odd[k::3]] for k in range(3)}
    for ctu in BOTTOM:
        for a, tag in enumerate(("full", "half")):
            out[f"bottom{ctu}-{tag}"] = [(a, c) for c in ctu_rows(ctu, a) if inside(c) and c[2] + c[4] != H]
    for ctu in INTERIOR + CORNER:
        for a, tag, parts in ((0, "full", 2), (1, "half", 3)):
            for k in range(parts):
                out[f"ctu{ctu}-{tag}{k}"] = [(a, c) for c in ctu_rows(ctu, a)[k::parts]]
    return out


def map_radius(c):
    """The reference's window: radius 32 for the odd-cut rows and for CUs of at
    most 32x32 samples, radius 8 for the larger ones (their maps at 32 are what
    takes the time; they are compared at radius 8 only)."""
    return 32 if c[3] * c[4] <= 32 * 32 or c[2] + c[4] == H else 8


@functools.lru_cache(maxsize=None)
def seed_maps(name):
    """{(align, candidate): sad_map against refs[0]} of a group, computed once."""
    refs, cur = frames()
    return {(a, c): S.sad_map(refs[0], cur, c[1], c[2], c[3], c[4], map_radius(c)) for a, c in seed_groups()[name]}


@pytest.mark.parametrize("name", sorted(seed_groups()))
def test_seed_search_against_reference(eng, name):
    drefs, dcur = dev_frames()
    maps = seed_maps(name)
    n = 0
    for radius in (8, 32):
        for lam in (0.0, LAM):
            out = eng.seed_search(dcur, drefs[:1], lam, radius=radius)
            got = {a: (out["mv"][(0, a)].cpu().numpy(), out["cost"][(0, a)].cpu().numpy()) for a in (0, 1)}
            for (a, c), m in maps.items():
                if radius > map_radius(c):
                    continue
                row, x, y, w, h = c
                want = S.seed_from_map(m, x, y, w, h, W, H, radius, lam)
                assert (tuple(got[a][0][row].tolist()), int(got[a][1][row])) == want, (name, radius, lam, a, c)
                n += 1
    assert n >= 2 * len(maps) >= 100, n


@pytest.mark.parametrize("radius", [8, 32])
def test_seed_search_rows_outside_and_invariants(eng, radius):
    drefs, dcur = dev_frames()
    for lam in (0.0, LAM):
        out = eng.seed_search(dcur, drefs[:2], lam, radius=radius)
        for r in (0, 1):
            for a in (0, 1):
                mv, cost = out["mv"][(r, a)].cpu().numpy(), out["cost"][(r, a)].cpu().numpy()
                outside = outside_mask(a)
                assert (cost[outside] == INF).all() and (mv[outside] == 0).all()
                assert (cost[~outside] < 1 << 40).all() and (cost[~outside] >= 0).all()
                assert (np.abs(mv) <= 16 * radius).all() and (mv % 16 == 0).all()
                if a == 1:
                    odd = [c[0] for c in odd_rows()]
                    assert (mv[odd, 1] <= 16 * 23).all() and mv[odd].any()


def test_the_cut_lies_on_the_minimum_of_odd_cut_rows():
    """On the reference alone (the maps are those of the test above): see the
    module's first lines for why no winner can have Dy == 23."""
    on_line = 0
    for k in range(3):
        for (a, c), m in seed_maps(f"odd{k}").items():
            assert m.shape == (65, 65)
            low = m[:32 + 24].min()                     # the admissible dy: -32 .. 23
            on_line += int(m[32 + 23].min() == low)
            assert (m[32 + 15:] == m[32 + 15]).all()    # Dy >= 15: one value per dx
            mv, _ = S.seed_from_map(m, c[1], c[2], c[3], c[4], W, H, 32, 0.0)
            assert mv[1] < 16 * 23
    assert on_line >= 20, on_line


# ------------------------------------------------------------------ 3. seed_search_wide
WIDE = ((64, 2), (32, 1), (37, 2))


@functools.lru_cache(maxsize=None)
def wide_rows():
    rows = {(1, c[0]) for c in odd_rows()}
    return frozenset(rows | {(a, c[0]) for a in (0, 1) for ctu in BOTTOM + INTERIOR + CORNER for c in ctu_rows(ctu, a)})


@functools.lru_cache(maxsize=None)
def searcher():
    refs, cur = frames()
    return P.Searcher(refs[0], cur, rows=wide_rows())


@functools.lru_cache(maxsize=None)
def want_wide(radius, levels, align, lam=LAM):
    return searcher().run(lam, radius, levels, align)


@pytest.mark.parametrize("radius,levels", WIDE)
def test_seed_search_wide_against_reference(eng, radius, levels):
    drefs, dcur = dev_frames()
    out = eng.seed_search_wide(dcur, drefs[:1], LAM, radius=radius, levels=levels)
    torch.cuda.synchronize()
    for a in (0, 1):
        mv, cost = out["mv"][(0, a)].cpu().numpy(), out["cost"][(0, a)].cpu().numpy()
        wmv, wcost, _ = want_wide(radius, levels, a)
        rows = np.array([c[0] for c in searcher().inn[a]])
        assert len(rows) >= 700
        bad = rows[(mv[rows] != wmv[rows]).any(1) | (cost[rows] != wcost[rows])]
        assert bad.size == 0, (radius, levels, a, len(bad),
                               [(int(k), mv[k].tolist(), int(cost[k]), wmv[k].tolist(), int(wcost[k])) for k in bad[:5]])
        outside = outside_mask(a)
        assert (cost[outside] == INF).all() and (mv[outside] == 0).all() and (cost[~outside] < 1 << 40).all()
        assert (np.abs(mv) <= 16 * radius).all() and (mv % 16 == 0).all()


def test_the_wide_search_meets_the_cut_on_odd_cut_rows():
    """On the reference alone (computed by the test above)."""
    odd = {c[0] for c in odd_rows()}
    for radius, levels in WIDE[:2]:
        facts = want_wide(radius, levels, 1)[2]
        assert facts["cut_y"] & odd and facts[("moved", 0)] & odd, (radius, levels)
    assert len(wide_rows()) >= 6 * 485


# ------------------------------------------------------------------ 4. the seed's cost is affine_mc's block
@pytest.mark.parametrize("search", ["seed_search", "seed_search_wide"])
def test_seed_cost_is_the_sad_of_affine_mc_plus_rate(eng, search):
    drefs, dcur = dev_frames()
    _, cur = frames()
    if search == "seed_search":
        out = eng.seed_search(dcur, drefs[:2], LAM, radius=32)
    else:
        out = eng.seed_search_wide(dcur, drefs[:2], LAM, radius=64, levels=2)
    n = 0
    for align in (0, 1):
        cus, rows = V.cus_from_seeds(W, H, align, out["mv"][(1, align)], ref=1, skip_zero=False)
        cost = out["cost"][(1, align)][rows].cpu().numpy()
        rows = rows.tolist()
        assert rows == [c[0] for c in cands(align) if inside(c)]
        pick = list(range(0, len(rows), len(rows) // 10))
        if align:
            at = {row: k for k, row in enumerate(rows)}
            pick += [at[c[0]] for c in odd_rows()[::16]]
        for k in pick:
            d = cus[k].tolist()
            pred, _, bad = eng.affine_mc(cus[k:k + 1].contiguous(), drefs[:2], pred=blank(H, W))
            x, y, w, h = d[:4]
            p = pred[y:y + h, x:x + w].contiguous().cpu().numpy().view(np.uint16).astype(np.int64)
            sad = int(np.abs(cur[y:y + h, x:x + w].astype(np.int64) - p).sum())
            assert int(bad) == 0 and sad + B.rate(B.bits_of(2, d[6:12]) + 2, LAM) == cost[k], (align, k, d)
            n += 1
    assert n >= 20 + 21


# ------------------------------------------------------------------ 5. affine_search, affine_me_seeded
def clone_result(res):
    return {k: (c.clone(), p.clone()) for k, (c, p) in res.items()}


@functools.lru_cache(maxsize=None)
def searched(nrefs):
    """affine_me_poc's result over the first nrefs references, modes 3, on the
    device; computed once and cloned by its users."""
    from vame.engine import Engine
    e = Engine(W, H, 0)
    try:
        drefs, dcur = dev_frames()
        res = e.affine_me_poc(dcur, drefs[:nrefs], LAM, modes=3)
        torch.cuda.synchronize()
        return res
    finally:
        e.close()


@pytest.mark.parametrize("align", [0, 1])
def test_zero_starts_equal_the_search(eng, align):
    drefs, dcur = dev_frames()
    res = searched(1)
    n = eng.n_cus(align)
    cus, rows = M.cus_from_result(W, H, align, 2, torch.zeros((n, 6), dtype=torch.int32).cuda())
    out, cost, bad = eng.affine_search(cus, drefs[:1], dcur, LAM)
    torch.cuda.synchronize()
    c2, p2 = res[(0, NAMES[2 * align])]
    assert int(bad) == 0 and rows.tolist() == [c[0] for c in cands(align) if inside(c)]
    assert torch.equal(cost, c2[rows]) and torch.equal(out[:, 6:], p2[rows][:, 1:])
    # the 3-CP run from seed_3cp of the 2-CP winners
    geo, win = cus.cpu().numpy(), p2[rows][:, 1:].cpu().numpy()
    start = [S.seed_3cp(w, int(d[0]), int(d[1]), int(d[2]), int(d[3]), W, H) for w, d in zip(win, geo)]
    cus3 = cus.clone()
    cus3[:, 5] = 3
    cus3[:, 6:] = torch.tensor(start, dtype=torch.int32).cuda()
    out3, cost3, bad3 = eng.affine_search(cus3, drefs[:1], dcur, LAM)
    torch.cuda.synchronize()
    c3, p3 = res[(0, NAMES[2 * align + 1])]
    assert int(bad3) == 0 and torch.equal(cost3, c3[rows]) and torch.equal(out3[:, 6:], p3[rows][:, 1:])
    if align:
        odd = torch.tensor([c[0] for c in odd_rows()]).cuda()
        assert torch.isin(odd, rows).all() and (p2[odd][:, 1:] != 0).any()


def merged_rows(align):
    """6 odd-cut rows (half-aligned only) and 6 others: three spread over the
    frame, three of the alignment's two largest sizes in the last two CTU rows."""
    inn = [c for c in cands(align) if inside(c)]
    top = sorted({c[3] * c[4] for c in inn})[-2]
    out = inn[7::len(inn) // 3][:3] + [c for c in inn if c[2] >= 896 and c[3] * c[4] >= top][5::9][:3]
    return out + (odd_rows()[3::60] if align else [])


def test_affine_me_seeded_against_reference(eng):
    drefs, dcur = dev_frames()
    refs, cur = frames()
    base = searched(1)
    seeds = eng.seed_search(dcur, drefs[:1], LAM, radius=32)["mv"]
    res, bad = eng.affine_me_seeded(dcur, drefs[:1], LAM, clone_result(base), seeds, modes=3)
    torch.cuda.synchronize()
    assert int(bad) == 0
    improved = 0
    for align in (0, 1):
        b = [tuple(t.cpu().numpy() for t in base[(0, NAMES[2 * align + m])]) for m in (0, 1)]
        g = [tuple(t.cpu().numpy() for t in res[(0, NAMES[2 * align + m])]) for m in (0, 1)]
        for m in (0, 1):
            assert (g[m][0] <= b[m][0]).all()  # no cost rose
            improved += int((g[m][0] < b[m][0]).sum())
        seed = seeds[(0, align)].cpu().numpy()
        rows = merged_rows(align)
        assert len(rows) == (12 if align else 6)
        for row, x, y, w, h in rows:
            want = S.merged(refs[0], cur, x, y, w, h, tuple(seed[row].tolist()), LAM, (b[0][0][row], b[0][1][row][1:]),
                            (b[1][0][row], b[1][1][row][1:]))
            for m in (0, 1):
                assert int(g[m][0][row]) == want[m][0] and g[m][1][row].tolist() == [2 + m] + want[m][1], (align, row, m)
    assert improved >= 10000


# ------------------------------------------------------------------ 6. bi-prediction and its refinement
def bipred_rows(part):
    """{align: rows}: 'odd' the odd-cut rows, 'full' / 'half' every 50th row."""
    if part == "odd":
        return {0: [], 1: [c[0] for c in odd_rows()]}
    return {0: list(range(0, len(cands(0)), 50)), 1: []} if part == "full" else {0: [], 1: list(range(0, len(cands(1)), 50))}


@pytest.mark.parametrize("part", ["odd", "full", "half"])
def test_bipred_against_reference(eng, part):
    drefs, dcur = dev_frames()
    refs, cur = frames()
    res = searched(2)
    bi = eng.bipred(dcur, drefs[:2], LAM, res)
    torch.cuda.synchronize()
    cost, cpmv = result_arrays(res)
    rows = bipred_rows(part)
    want = B.bipred(cur, refs[:2], cost, cpmv, 15, LAM, rows)
    for a in (0, 1):
        r = np.array(rows[a], np.int64)
        got_cost, got_sel = bi["cost"][a].cpu().numpy(), bi["sel"][a].cpu().numpy()
        np.testing.assert_array_equal(got_cost[r], want[a][0][r], err_msg=f"cost {a}")
        np.testing.assert_array_equal(got_sel[r], want[a][1][r], err_msg=f"sel {a}")
        outside = outside_mask(a)
        assert (got_sel[outside] == -1).all() and (got_sel[~outside] >= 0).all() and (got_cost[outside] == INF).all()
    assert sum((want[a][1][rows[a]] >= 0).sum() for a in (0, 1)) >= (330 if part == "odd" else 300)


def refine_cases():
    """Six bi descriptors in the bottom CTU row: two that end on row 1080, a
    128x64 at y = 960, CPMVs that push the window below the frame (clip_mv and
    the clamp act), the bottom-right corner's last CU and a 64x64."""
    rng = np.random.default_rng(17)

    def cp(n, base=(-140, 380), big=20):
        v = (np.array(base * 3) + rng.integers(-big, big + 1, 6)).tolist()
        return [n] + (v if n == 3 else v[:4] + [0, 0])
    odd = odd_rows()
    a, b = odd[5], odd[-1]
    return [list(a[1:]) + [0] + cp(2) + [1] + cp(3),
            list(b[1:]) + [1] + cp(3) + [0] + cp(2),
            [512, 960, 128, 64, 0] + cp(2) + [1] + cp(2),
            [1024, 1056, 16, 16, 0] + cp(3, (40, 900), 60) + [1] + cp(2, (-30, 2000), 5),
            [1904, 1056, 16, 16, 1] + cp(2) + [0] + cp(3),
            [256, 960, 64, 64, 0] + cp(3) + [1] + cp(3)]


def test_bipred_refine_against_reference(eng):
    drefs, dcur = dev_frames()
    refs, cur = frames()
    cs = refine_cases()
    assert sum(d[1] + d[3] == H for d in cs) == 2 and [128, 64] in [d[2:4] for d in cs] and all(d[1] >= 896 for d in cs)
    out, cost, bad = eng.bipred_refine(torch.tensor(cs, dtype=torch.int32).cuda(), drefs[:2], dcur, LAM, 2)
    torch.cuda.synchronize()
    assert int(bad) == 0
    moved = 0
    for i, d in enumerate(cs):
        trace = F.refine_bicu_trace(refs[:2], cur, d, LAM, 2)
        assert out[i].tolist() == trace[2][0] and int(cost[i]) == trace[2][1], (i, d, out[i].tolist(), trace[2])
        moved += trace[2][0] != trace[0][0]
    assert moved >= 3


def test_refined_costs_are_affine_mc_bi_costs(eng):
    drefs, dcur = dev_frames()
    res = searched(2)
    bi = eng.bipred(dcur, drefs[:2], LAM, res)
    fine = eng.refine_bipred(dcur, drefs[:2], LAM, res, bi, rounds=2)
    lower = 0
    for a in (0, 1):
        cus, rows = fine["cus"][a], fine["rows"][a].to(torch.int64)
        assert rows.tolist() == [c[0] for c in cands(a) if inside(c)]
        _, cost, bad = eng.affine_mc_bi(cus, drefs[:2], LAM, cur=dcur, want_cost=True)
        torch.cuda.synchronize()
        assert int(bad) == 0 and torch.equal(cost, fine["cost"][a][rows])
        assert (cost <= bi["cost"][a][rows]).all()
        lower += int((cost < bi["cost"][a][rows]).sum())
    assert lower >= 10000


# ------------------------------------------------------------------ 7. the chain, four references
def test_the_chain_with_four_references(eng):
    drefs, dcur = dev_frames()
    refs, cur = frames()
    res = clone_result(searched(4))
    seeds = eng.seed_search_wide(dcur, drefs, LAM, radius=64, levels=2)
    _, sbad = eng.affine_me_seeded(dcur, drefs, LAM, res, seeds["mv"], modes=3)
    bi = eng.bipred(dcur, drefs, LAM, res)
    part = eng.partition_bi(res, bi, split_penalty=100, bi_penalty=10)
    fine = eng.refine_partition(part, drefs, dcur, LAM, rounds=2)
    pred, cost, bad = eng.predict_partition(fine, drefs, LAM, cur=dcur, pred=blank(H, W), want_cost=True)
    torch.cuda.synchronize()
    assert int(sbad) == 0 and int(bad) == 0 and int(fine["bad"]) == 0
    # the decision is the reference's on the device's own search result
    hcost, hcpmv = result_arrays(res)
    hbi = {a: (bi["cost"][a].cpu().numpy(), bi["sel"][a].cpu().numpy()) for a in (0, 1)}
    want = B.partition_bi(W, H, hcost, hcpmv, 4, 15, 100, hbi, 10)
    got = VB.to_host(part)
    for k in VB.KEYS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    n = want["ncus"]
    # the leaves' costs are affine_mc_bi's of the refined descriptors
    cus = fine["cus"][:n].contiguous()
    _, direct, dbad = eng.affine_mc_bi(cus, drefs, LAM, cur=dcur, want_cost=True)
    torch.cuda.synchronize()
    assert int(dbad) == 0 and torch.equal(direct, cost[:n]) and torch.equal(direct, fine["leaf_cost"][:n])
    leaves = cus.cpu().numpy()
    assert (leaves[:, 4] >= 2).any() and (leaves[:, 12] >= 0).any() and (leaves[:, 12] < 0).any()
    # the bottom CTU row: leaves end on 1072 (none on 1080, see the first lines), eight rows of holes below
    assert (leaves[:, 1] + leaves[:, 3]).max() == 1072 and (want["ctu_info"][120:, 2] > 0).all()
    got_pred = pred.cpu().numpy().view(np.uint16)
    assert (got_pred[:1072] != 0xFFFF).all() and (got_pred[1072:] == 0xFFFF).all()
    low = np.nonzero(leaves[:, 1] + leaves[:, 3] == 1072)[0]
    for i in list(range(0, n, n // 6))[:6] + low[::max(1, len(low) // 4)][:4].tolist():
        d = leaves[i]
        p, _ = B.predict_bicu(refs, None, d)
        assert (got_pred[d[1]:d[1] + d[3], d[0]:d[0] + d[2]] == p).all(), d.tolist()
