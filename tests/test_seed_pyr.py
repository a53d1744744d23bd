"""The wide-range seed search, host side: the CPU
restatement tests/seedpyr_ref.py against seed_ref where the two rules meet,
and what the pyramid search finds on a shift beyond the exhaustive search's
+-32.  No device work."""
import functools

import numpy as np

import bipred_ref as B
import seed_ref as S
import seedpyr_ref as P
from test_seed import sample

W, H = 416, 240
LAM = S.LAM


@functools.lru_cache(maxsize=None)
def searcher():
    refs, cur = P.shifted_camera_wide((-43, 26))
    return P.Searcher(refs[0], cur)


@functools.lru_cache(maxsize=None)
def wide(radius, levels, align, lam=LAM):
    return searcher().run(lam, radius, levels, align)


def seed_value(ref, cur, x, y, w, h, mv, lam):
    """seed_ref's value (sad_map's sum, rate_table's rate) of the displacement mv / 16."""
    dx, dy = mv[0] // 16, mv[1] // 16
    yy = np.clip(np.arange(y + dy, y + dy + h), 0, H - 1)
    xx = np.clip(np.arange(x + dx, x + dx + w), 0, W - 1)
    sad = int(np.abs(cur[y:y + h, x:x + w].astype(np.int64) - ref.astype(np.int64)[yy][:, xx]).sum())
    return sad + B.rate(B.bits_of(2, (mv[0], mv[1], mv[0], mv[1], 0, 0)) + 2, lam)


def test_pyramid_is_the_rounded_mean():
    rng = np.random.default_rng(16)
    f = rng.integers(0, 1024, (H, W)).astype(np.uint16)
    p = P.pyramid(f)
    assert [a.shape for a in p] == [(H, W), (H // 2, W // 2), (H // 4, W // 4)]
    for l in (0, 1):
        for y, x in ((0, 0), (7, 9), (p[l + 1].shape[0] - 1, p[l + 1].shape[1] - 1)):
            q = p[l][2 * y:2 * y + 2, 2 * x:2 * x + 2].astype(int)
            assert p[l + 1][y, x] == (q.sum() + 2) >> 2
    assert P.packed(f).shape == ((W // 2) * (H // 2) + (W // 4) * (H // 4),)
    assert (P.packed(f)[:(W // 2) * (H // 2)] == p[1].reshape(-1)).all()


def test_radius_0_equals_seed_cu():
    s = searcher()
    ref, cur = s.ref[0], s.cur[0]
    for levels in (1, 2):
        for align in (0, 1):
            mv, cost, _ = wide(0, levels, align)
            assert not mv.any()
            for row, x, y, w, h in sample(align, 24, salt=16):
                assert ((0, 0), int(cost[row])) == S.seed_cu(ref, cur, x, y, w, h, 0, LAM)
            out = [c[0] for c in B.frame_candidates(W, H, align) if c[1] + c[3] > W or c[2] + c[4] > H]
            assert (cost[out] == S.INF).all()


def test_cost_is_seed_refs_value_of_the_displacement_and_never_above_zero():
    s = searcher()
    ref, cur = s.ref[0], s.cur[0]
    for radius, levels in ((64, 2), (37, 1)):
        for align in (0, 1):
            mv, cost, _ = wide(radius, levels, align)
            zero = wide(0, levels, align)[1]
            for row, x, y, w, h in s.inn[align]:
                assert int(cost[row]) == seed_value(ref, cur, x, y, w, h, mv[row].tolist(), LAM), (radius, align, row)
                assert cost[row] <= zero[row]
                assert tuple(mv[row]) == (0, 0) or cost[row] < zero[row]  # a non-zero seed: strictly better
            assert (np.abs(mv) <= 16 * radius).all() and (mv % 16 == 0).all()


def test_the_wide_shift_is_found():
    """(-43, +26) lies beyond +-32: at radius 64, levels 2 the summed cost of
    the in-frame aligned rows is at most a fifth of the zero-displacement sum."""
    rows = [c[0] for c in searcher().inn[0]]
    assert len(rows) == 1143
    zero = int(wide(0, 2, 0)[1][rows].sum())
    got = int(wide(64, 2, 0)[1][rows].sum())
    print("zero", zero, "radius 64 levels 2", got, got / zero)
    assert 5 * got <= zero


def test_a_restricted_searcher_equals_the_unrestricted_on_its_rows():
    """Searcher(rows=) restricts the rows computed and nothing else: on its
    rows the unrestricted mv and cost, every other row (0, 0) / INF."""
    s = searcher()
    rows = {(a, c[0]) for a in (0, 1) for c in sample(a, 24, salt=17)}
    rows |= {(a, c[0]) for a in (0, 1) for c in B.frame_candidates(W, H, a)[-5:]}  # rows that leave the frame
    few = P.Searcher(s.ref[0], s.cur[0], rows=rows)
    for radius, levels in ((64, 2), (37, 1)):
        for align in (0, 1):
            mv, cost, facts = few.run(LAM, radius, levels, align)
            wmv, wcost, wfacts = wide(radius, levels, align)
            mine = np.array(sorted(r for a, r in rows if a == align))
            assert 20 <= len(mine) < len(wcost) // 10
            np.testing.assert_array_equal(mv[mine], wmv[mine])
            np.testing.assert_array_equal(cost[mine], wcost[mine])
            other = np.setdiff1d(np.arange(len(wcost)), mine)
            assert not mv[other].any() and (cost[other] == P.INF).all()
            assert (wcost[mine] < P.INF).sum() >= 20 and (wcost[mine] == P.INF).sum() == 5
            assert facts["outside"] == set(other.tolist()) | wfacts["outside"]  # 'outside' is what is not computed
            for k in facts:
                if k != "outside":
                    assert facts[k] == wfacts[k] & set(mine.tolist()), k
