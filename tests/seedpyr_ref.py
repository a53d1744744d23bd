"""CPU reference of the wide-range seed search (test infrastructure; DESIGN.md
section 16): a numpy restatement of vame_seed_pyramid and
vame_seed_search_wide's rule for every row of a frame at once.

pyramid      levels 0..2 of a frame, level l+1 = (a + b + c + d + 2) >> 2
packed       levels 1 and 2 as vame_seed_pyramid lays them out
Searcher     the rule: the exhaustive top level (whole-frame |cur - displaced
             ref| and one integral image per displacement price every row),
             then +-1 around twice the winner per level (one clamped window
             per row), admissibility and the two orders; with per-row facts
             for the coverage test
value0       the level-0 value of one displacement of one CU
Bits and rate come from bipred_ref (the oracle's), CU geometry from the
library's host tables (bipred_ref.frame_candidates).  Nothing here shares code
with the kernels.
"""
from __future__ import annotations

import functools

import numpy as np

import bipred_ref as B

INF = (1 << 63) - 1


def pyramid(frame):
    """[level 0, level 1, level 2] (uint16) of a frame."""
    out = [np.ascontiguousarray(frame).astype(np.uint16)]
    for _ in range(2):
        a = out[-1].astype(np.int64)
        out.append(((a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2).astype(np.uint16))
    return out


def packed(frame):
    """Levels 1 and 2, dense and row-major, level 1 first (uint16 [n])."""
    p = pyramid(frame)
    return np.concatenate([p[1].reshape(-1), p[2].reshape(-1)])


@functools.lru_cache(maxsize=None)
def rate_of(Dx, Dy, lam):
    """The search's rate of the 2-CP CPMVs LT = RT = (16 Dx, 16 Dy), ruiBits included."""
    return B.rate(B.bits_of(2, (16 * Dx, 16 * Dy, 16 * Dx, 16 * Dy, 0, 0)) + 2, lam)


def shifted(ref, dx, dy):
    """ref[clamp(y + dy)][clamp(x + dx)] for every (y, x) of the level."""
    H, W = ref.shape
    return ref[np.clip(np.arange(H) + dy, 0, H - 1)][:, np.clip(np.arange(W) + dx, 0, W - 1)]


def top_sads(ref, cur, boxes, Rc):
    """int64 [rows, 2 Rc + 1, 2 Rc + 1] at [row, dy + Rc, dx + Rc]: the SAD of
    every box (x, y, w, h of the level) at every displacement of the level."""
    H, W = cur.shape
    ref, cur = ref.astype(np.int64), cur.astype(np.int64)
    x0, y0 = boxes[:, 0], boxes[:, 1]
    x1, y1 = x0 + boxes[:, 2], y0 + boxes[:, 3]
    n = 2 * Rc + 1
    out = np.zeros((len(boxes), n, n), np.int64)
    I = np.zeros((H + 1, W + 1), np.int64)
    for j, dy in enumerate(range(-Rc, Rc + 1)):
        for i, dx in enumerate(range(-Rc, Rc + 1)):
            I[1:, 1:] = np.abs(cur - shifted(ref, dx, dy)).cumsum(0).cumsum(1)
            out[:, j, i] = I[y1, x1] - I[y0, x1] - I[y1, x0] + I[y0, x0]
    return out


def top_sads_tiles(ref, cur, boxes, Rc, tile):
    """top_sads for boxes that cover little of the level: the same sums, one
    tile of `tile` x `tile` samples (no box crosses a tile's border) and its
    clamped reference window at a time, only the tiles that hold a box."""
    H, W = cur.shape
    ref, cur = ref.astype(np.int64), cur.astype(np.int64)
    n = 2 * Rc + 1
    out = np.zeros((len(boxes), n, n), np.int64)
    key = (boxes[:, 1] // tile) * W + boxes[:, 0] // tile
    for k in np.unique(key):
        sel = np.nonzero(key == k)[0]
        X0, Y0 = (boxes[sel[0], 0] // tile) * tile, (boxes[sel[0], 1] // tile) * tile
        hh, ww = min(tile, H - Y0), min(tile, W - X0)
        c = cur[Y0:Y0 + hh, X0:X0 + ww]
        yy, xx = np.clip(np.arange(Y0 - Rc, Y0 + hh + Rc), 0, H - 1), np.clip(np.arange(X0 - Rc, X0 + ww + Rc), 0, W - 1)
        win = ref[yy][:, xx]
        x0, y0 = boxes[sel, 0] - X0, boxes[sel, 1] - Y0
        x1, y1 = x0 + boxes[sel, 2], y0 + boxes[sel, 3]
        I = np.zeros((hh + 1, ww + 1), np.int64)
        for j in range(n):
            for i in range(n):
                I[1:, 1:] = np.abs(c - win[j:j + hh, i:i + ww]).cumsum(0).cumsum(1)
                out[sel, j, i] = I[y1, x1] - I[y0, x1] - I[y1, x0] + I[y0, x0]
    return out


def sad9(ref, cur, x, y, w, h, cx, cy):
    """int64 [3, 3] at [ey + 1, ex + 1]: the SAD of the level's box against the
    level's reference displaced by (cx + ex, cy + ey), coordinates clamped."""
    H, W = cur.shape
    blk = cur[y:y + h, x:x + w].astype(np.int64)
    yy = np.clip(np.arange(y + cy - 1, y + cy + h + 1), 0, H - 1)
    xx = np.clip(np.arange(x + cx - 1, x + cx + w + 1), 0, W - 1)
    win = ref[yy][:, xx].astype(np.int64)
    return np.array([[np.abs(blk - win[j:j + h, i:i + w]).sum() for i in range(3)] for j in range(3)], np.int64)


def value0(ref, cur, x, y, w, h, Dx, Dy, lam):
    """vame_seed_search's value of the displacement (Dx, Dy) of a CU in the frame."""
    H, W = cur.shape
    yy = np.clip(np.arange(y + Dy, y + Dy + h), 0, H - 1)
    xx = np.clip(np.arange(x + Dx, x + Dx + w), 0, W - 1)
    sad = int(np.abs(cur[y:y + h, x:x + w].astype(np.int64) - ref[yy][:, xx].astype(np.int64)).sum())
    return sad + rate_of(int(Dx), int(Dy), lam)


def admissible(Dx, Dy, x, y, W, H, radius):
    return abs(Dx) <= radius and abs(Dy) <= radius and Dx <= W + 7 - x and Dy <= H + 7 - y


class Searcher:
    """The rule on one (ref, cur) pair.  SADs do not depend on lambda, radius
    or (below the top) levels: they are kept between run() calls.  rows: a set
    of (align, row) that restricts the rows computed to those of it that lie
    in the frame (the others stay (0, 0) / INF); None: every in-frame row.  A
    restricted Searcher sums the top level CTU by CTU (top_sads_tiles), which
    is what makes a few CTUs of a large frame affordable."""

    def __init__(self, ref, cur, rows=None):
        self.ref, self.cur = pyramid(ref), pyramid(cur)
        self.H, self.W = cur.shape
        self.cands = {a: B.frame_candidates(self.W, self.H, a) for a in (0, 1)}
        self.inn = {a: [c for c in self.cands[a] if c[1] + c[3] <= self.W and c[2] + c[4] <= self.H
                        and (rows is None or (a, c[0]) in rows)] for a in (0, 1)}
        self.restricted = rows is not None
        self._top, self._nine, self._zero = {}, {}, {}

    def top(self, align, L, Rc):
        """top_sads of the alignment's in-frame rows at level L, at least +-Rc
        (both alignments in one pass over the displacements)."""
        if L not in self._top or (self._top[L].shape[1] - 1) // 2 < Rc:
            boxes = np.array([[c[1] >> L, c[2] >> L, c[3] >> L, c[4] >> L] for a in (0, 1) for c in self.inn[a]], np.int64)
            if self.restricted:
                self._top[L] = top_sads_tiles(self.ref[L], self.cur[L], boxes, Rc, 128 >> L)
            else:
                self._top[L] = top_sads(self.ref[L], self.cur[L], boxes, Rc)
        n0 = len(self.inn[0])
        t = self._top[L][n0:] if align else self._top[L][:n0]
        big = (t.shape[1] - 1) // 2
        return t[:, big - Rc:big + Rc + 1, big - Rc:big + Rc + 1]

    def nine(self, l, c, cx, cy):
        key = (l, c, cx, cy)
        if key not in self._nine:
            _, x, y, w, h = c
            self._nine[key] = sad9(self.ref[l], self.cur[l], x >> l, y >> l, w >> l, h >> l, cx, cy)
        return self._nine[key]

    def zero(self, c):
        """The level-0 SAD of (0, 0)."""
        if c not in self._zero:
            _, x, y, w, h = c
            self._zero[c] = value0(self.ref[0], self.cur[0], x, y, w, h, 0, 0, 0.0) - rate_of(0, 0, 0.0)
        return self._zero[c]

    def run(self, lam, radius, levels, align):
        """(mv int32 [n, 2], cost int64 [n], facts) of the alignment's rows.
        facts: {name: set of rows} -- 'outside', 'top_tie' (the top level's
        minimum is attained more than once), 'cut_x' / 'cut_y' (a candidate
        inside the radius cut by Dx <= W+7-x / Dy <= H+7-y), 'cut_radius' (a
        refinement candidate beyond the radius), ('moved', l) (the winner of
        level l < levels is not its centre)."""
        W, H, L = self.W, self.H, levels
        n = len(self.cands[align])
        mv, cost = np.zeros((n, 2), np.int32), np.full(n, INF, np.int64)
        facts = {k: set() for k in ("outside", "top_tie", "cut_x", "cut_y", "cut_radius")}
        facts.update({("moved", l): set() for l in range(L)})
        facts["outside"] = {c[0] for c in self.cands[align]} - {c[0] for c in self.inn[align]}
        Rc = radius >> L
        d = np.arange(-Rc, Rc + 1)
        rates = np.array([[rate_of(int(dx) << L, int(dy) << L, lam) for dx in d] for dy in d], np.int64)
        sads = self.top(align, L, Rc)
        for k, c in enumerate(self.inn[align]):
            row, x, y, w, h = c
            # ---- the top level: (0, 0), then dy outer, dx inner
            ok = ((d[:, None] << L) <= H + 7 - y) & ((d[None, :] << L) <= W + 7 - x)
            if not ((d << L) <= W + 7 - x).all():
                facts["cut_x"].add(row)
            if not ((d << L) <= H + 7 - y).all():
                facts["cut_y"].add(row)
            v = np.where(ok, (sads[k] << (2 * L)) + rates, INF)
            first = int(np.argmin(v))
            j, i = divmod(first, 2 * Rc + 1)
            if (v == v[j, i]).sum() > 1:
                facts["top_tie"].add(row)
            best = (int(d[i]), int(d[j])) if v[j, i] < v[Rc, Rc] else (0, 0)
            # ---- +-1 per level
            val = None
            for l in range(L - 1, -1, -1):
                cx, cy = 2 * best[0], 2 * best[1]
                s = self.nine(l, c, cx, cy)
                order = ([(0, 0)] if l == 0 else []) + [(cx, cy)] + \
                    [(cx + ex, cy + ey) for ey in (-1, 0, 1) for ex in (-1, 0, 1) if (ex, ey) != (0, 0)]
                val, best = None, None
                for dx, dy in order:
                    Dx, Dy = dx << l, dy << l
                    if not admissible(Dx, Dy, x, y, W, H, radius):
                        if abs(Dx) > radius or abs(Dy) > radius:
                            facts["cut_radius"].add(row)
                        else:
                            facts["cut_x" if Dx > W + 7 - x else "cut_y"].add(row)
                        continue
                    if abs(dx - cx) <= 1 and abs(dy - cy) <= 1:
                        sad = int(s[dy - cy + 1, dx - cx + 1])
                    else:  # (0, 0) at level 0, away from the centre
                        sad = self.zero(c)
                    t = (sad << (2 * l)) + rate_of(Dx, Dy, lam)
                    if val is None or t < val:
                        val, best = t, (dx, dy)
                if best != (cx, cy):
                    facts[("moved", l)].add(row)
            mv[row] = (16 * best[0], 16 * best[1])
            cost[row] = val
        return mv, cost, facts


@functools.lru_cache(maxsize=None)
def shifted_camera_wide(shift=(-43, 26), nrefs=1):
    """The shifted-camera pair of seed_ref at a wide shift: (refs [nrefs, H, W],
    cur) at 416x240, seed 0xBEEF -- cur is POC 2 seen through a window moved by
    `shift` samples, refs[r] the QP-32 reconstruction of POC r."""
    from vame import synth
    W, H, M = 416, 240, 64
    assert max(abs(shift[0]), abs(shift[1])) <= M
    big = {p: synth.synth_frame(W + 2 * M, H + 2 * M, p, 0xBEEF) for p in {0, 2} | set(range(nrefs))}
    refs = [synth.recon_frame(big[p], p, 32, 0xBEEF)[M:M + H, M:M + W] for p in range(nrefs)]
    cur = big[2][M + shift[1]:M + shift[1] + H, M + shift[0]:M + shift[0] + W]
    return np.ascontiguousarray(np.stack(refs)).astype(np.uint16), np.ascontiguousarray(cur).astype(np.uint16)


def stripes(W=416, H=240):
    """The tie input: (refs [2, H, W], cur) -- vertical stripes of period 16
    with cur = refs[0] moved by 4 samples (refs[1]: by 8), so a CU's smallest
    SAD is attained at every 16th dx and at every dy."""
    x = np.arange(W + 16)
    big = np.broadcast_to(np.where(x % 16 < 8, 900, 100).astype(np.uint16), (H, W + 16))
    return np.ascontiguousarray(np.stack([big[:, :W], big[:, 12:W + 12]])), np.ascontiguousarray(big[:, 4:W + 4])
