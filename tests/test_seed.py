"""Seeding the affine search, host side: the CPU
restatement tests/seed_ref.py pinned to the oracle's outputs, the seed rule on a
pure translation, and what seeding gains on the shifted-camera pair.  No device
work."""
import functools
import os

import numpy as np

import bipred_ref as B
import oracle_py as O
import seed_ref as S

GOLD = os.path.join(os.path.dirname(__file__), "golden")
W, H = 416, 240
NAMES = ("FULL_2CP", "FULL_3CP", "HALF_2CP", "HALF_3CP")


def load(name):
    return dict(np.load(os.path.join(GOLD, name + ".npz")))


def inframe(align):
    """[(row, x, y, w, h)] of the alignment's candidates that lie in the frame."""
    return [c for c in B.frame_candidates(W, H, align) if c[1] + c[3] <= W and c[2] + c[4] <= H]


def sample(align, n, salt=0):
    """About n in-frame candidates of the alignment: every size, spread over the CTUs."""
    cands = inframe(align)
    by_size = {}
    for c in cands:
        by_size.setdefault((c[3], c[4]), []).append(c)
    rng = np.random.default_rng(1500 + 10 * align + salt)
    per = max(1, n // len(by_size))
    out = []
    for size in sorted(by_size):
        g = by_size[size]
        out += [g[i] for i in sorted(rng.choice(len(g), min(per, len(g)), replace=False))]
    return out


# ------------------------------------------------------------------ 1. the restatement is run_cu
def test_zero_start_is_the_oracle():
    for name, n in (("s416_qp32_poc2_ref0", 14), ("s416_bigmotion", 12)):
        z = load(name)
        ref, cur, lam = z["ref"], z["cur"], float(z["lam"])
        for align in (0, 1):
            cost2, cp2 = O.affine_me(ref, cur, lam, align, 2)
            np.testing.assert_array_equal(cost2, z[NAMES[2 * align] + "_cost"])
            g3c, g3p = z[NAMES[2 * align + 1] + "_cost"], z[NAMES[2 * align + 1] + "_cpmv"]
            for row, x, y, w, h in sample(align, n):
                cp, cost = S.search_cu(ref, cur, x, y, w, h, 2, [0] * 6, lam)
                assert cost == cost2[row] and cp == list(cp2[row].tolist())[1:], (name, align, row)
                start = S.seed_3cp(cp, x, y, w, h, W, H)
                cp, cost = S.search_cu(ref, cur, x, y, w, h, 3, start, lam)
                assert cost == g3c[row] and cp == [int(v) for v in np.asarray(g3p[row]).reshape(-1)[-6:]], \
                    (name, align, row)


# ------------------------------------------------------------------ 2. the seed rule
def test_pure_translation_is_found():
    from vame import synth
    big = synth.synth_frame(W + 128, H + 128, 3, 0xBEEF)
    ref = np.ascontiguousarray(big[64:64 + H, 64:64 + W])
    cur = np.ascontiguousarray(big[64 + 6:64 + 6 + H, 64 - 11:64 - 11 + W])  # cur[y][x] = ref[y + 6][x - 11]
    n = 0
    for align in (0, 1):
        for row, x, y, w, h in sample(align, 24, salt=3):
            if x - 11 < 0 or y + 6 + h > H:
                continue  # the displaced block leaves the reference: the clamp replaces samples
            mv, cost = S.seed_cu(ref, cur, x, y, w, h, 16, 0.0)
            assert cost == 0
            # the first zero-SAD displacement in the order: none before (-11, 6)
            blk = cur[y:y + h, x:x + w].astype(np.int64)
            first = None
            for dy, dx in [(0, 0)] + [(dy, dx) for dy in range(-16, 17) for dx in range(-16, 17)]:
                if dx > W + 7 - x or dy > H + 7 - y:
                    continue
                yy = np.clip(np.arange(y + dy, y + dy + h), 0, H - 1)
                xx = np.clip(np.arange(x + dx, x + dx + w), 0, W - 1)
                if not np.abs(blk - ref[yy][:, xx].astype(np.int64)).any():
                    first = (16 * dx, 16 * dy)
                    break
            assert mv == first, (align, row)
            n += mv == (-176, 96)
    assert n >= 20


def test_seed_rule_details():
    refs, cur = S.shifted_camera()
    # out of the frame: (0, 0) and INT64_MAX; radius 0: the value of (0, 0)
    assert S.seed_cu(refs[0], cur, 384, 128, 64, 128, 16, S.LAM) == ((0, 0), S.INF)
    mv, cost = S.seed_cu(refs[0], cur, 64, 64, 32, 32, 0, S.LAM)
    sad = int(np.abs(cur[64:96, 64:96].astype(np.int64) - refs[0][64:96, 64:96].astype(np.int64)).sum())
    assert mv == (0, 0) and cost == sad + B.rate(B.bits_of(2, [0] * 6) + 2, S.LAM)
    # at x = W - 16 the window is cut at dx = 23: with radius 32 no seed beyond it
    for y in (0, 112, 224):
        mv, _ = S.seed_cu(refs[0], cur, W - 16, y, 16, 16, 32, 0.0)
        assert mv[0] <= 16 * 23 and mv[1] <= 16 * (H + 7 - y)


# ------------------------------------------------------------------ 3. what seeding gains
@functools.lru_cache(maxsize=None)
def shifted_rows():
    """[(align, row, seed, base cost, merged cost)] on a sample of the
    shifted-camera pair, 2-CP, radius 16."""
    refs, cur = S.shifted_camera()
    out = []
    for align in (0, 1):
        cost2, cp2 = O.affine_me(refs[0], cur, S.LAM, align, 2)
        for row, x, y, w, h in sample(align, 30, salt=7):
            seed, _ = S.seed_cu(refs[0], cur, x, y, w, h, 16, S.LAM)
            m = S.merged(refs[0], cur, x, y, w, h, seed, S.LAM, (cost2[row], list(cp2[row].tolist())[1:]))
            out.append((align, row, seed, int(cost2[row]), m[0][0]))
    return out


def test_seeding_lowers_the_cost_on_the_shifted_camera():
    rows = shifted_rows()
    assert all(m <= b for _, _, _, b, m in rows)
    nz = [r for r in rows if r[2] != (0, 0)]
    assert len(nz) >= 0.8 * len(rows)
    assert sum(m < b for _, _, _, b, m in nz) >= 0.9 * len(nz)
