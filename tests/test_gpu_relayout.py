"""The hand-over of the 2-CP-only launches' two-sub-block quadrant waves (DESIGN
§4.5b: once a wave task's live CUs hold <= 64 sub-blocks, the wave finishes
them one sub-block per lane): frames whose content makes wave-mates settle at
different iterations, every cost and CPMV of FULL_2CP and HALF_2CP against the
CPU oracle bit for bit, through vame_affine_me_batch (modes = 1) and through
the per-launch entry point.

The frames are 416x240, the smallest resolution the engine and the oracle
take (a 256x128 frame is refused by both): each content comes as `two_ctu`,
the pattern on the frame's first two CTUs (256x128, every CU inside the frame)
with the rest of the frame identical to its reference, and as `frame`, the
pattern over the whole frame, whose right and bottom CTUs the frame edge cuts.

Run as a program (`python test_gpu_relayout.py OUT.npz`, VAME_LIB naming a
library) it writes case (a)'s batch results; the test uses that to compare the
build without the hand-over (lib/libvame_norelayout.so, `make variant
NAME=norelayout DEFS=-DVAME_RELAYOUT=0`) where that library has been built."""
import functools
import os
import subprocess
import sys

import numpy as np

W, H = 416, 240
LAM = 70.335619  # lambda_for_poc(32, 2)
NAMES = {"FULL_2CP": (0, 2), "HALF_2CP": (1, 2)}


def texture(rng, h, w):
    """A smooth 10-bit texture with gradients in every direction."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    t = np.zeros((h, w))
    for _ in range(6):
        fx, fy, ph = rng.uniform(0.02, 0.35), rng.uniform(0.02, 0.35), rng.uniform(0, 6.28)
        t += rng.uniform(0.4, 1.0) * np.sin(fx * x + fy * y + ph)
    t += 0.15 * rng.standard_normal((h, w))
    t = (t - t.min()) / (t.max() - t.min())
    return t * 900 + 60


def warp(t, ax, bx, cx, ay, by, cy):
    """t sampled at (x + ax + bx x + cx y, y + ay + by x + cy y), bilinear: a
    fractional affine displacement."""
    h, w = t.shape
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    sx = np.clip(x + ax + bx * (x % 64) + cx * (y % 64), 0, w - 1.001)
    sy = np.clip(y + ay + by * (x % 64) + cy * (y % 64), 0, h - 1.001)
    x0, y0 = np.floor(sx).astype(int), np.floor(sy).astype(int)
    fx, fy = sx - x0, sy - y0
    return ((1 - fy) * ((1 - fx) * t[y0, x0] + fx * t[y0, x0 + 1]) +
            fy * ((1 - fx) * t[y0 + 1, x0] + fx * t[y0 + 1, x0 + 1]))


def still_mask(h, w):
    """True where the original equals the reference: per 64x64 quadrant the
    top-left 32x32, the upper 32x16 of the bottom-left 32x32 and, in every
    other quadrant, the upper 32x16 of the bottom-right 32x32 -- so of the CUs
    sharing a wave some settle at the first update and some go on."""
    y, x = np.mgrid[0:h, 0:w]
    qx, qy = x % 64, y % 64
    odd = ((x // 64) + (y // 64)) % 2 == 1
    m = (qx < 32) & (qy < 32)
    m |= (qx < 32) & (qy >= 32) & (qy < 48)
    m |= odd & (qx >= 32) & (qy >= 32) & (qy < 48)
    return m


def to_frame(a):
    return np.ascontiguousarray(np.clip(np.rint(a), 0, 1023).astype(np.uint16))


@functools.lru_cache(maxsize=None)
def frames(kind, extent):
    """(ref, cur) of content `kind` over `extent` ('two_ctu' or 'frame')."""
    rng = np.random.default_rng({"mixed": 11, "same": 12, "noise": 13}[kind])
    if kind == "same":
        ref = to_frame(texture(rng, H, W))
        cur = ref.copy()
    elif kind == "mixed":
        t = texture(rng, H, W)
        ref = to_frame(t)
        moved = to_frame(warp(t, 1.3, 0.011, -0.007, -0.8, 0.006, 0.009))
        cur = np.where(still_mask(H, W), ref, moved)
    else:  # noise, displaced far: few CUs settle early
        t = rng.integers(0, 1024, (H + 32, W + 32)).astype(np.float64)
        t = (t + np.roll(t, 1, 0) + np.roll(t, 1, 1) + np.roll(t, (1, 1), (0, 1))) / 4
        ref = to_frame(t[16:16 + H, 16:16 + W])
        cur = to_frame(t[16 - 9:16 - 9 + H, 16 + 13:16 + 13 + W] + 8 * rng.standard_normal((H, W)))
    if extent == "two_ctu":  # the pattern on the first two CTUs, the rest identical
        keep = np.zeros((H, W), bool)
        keep[:128, :256] = True
        cur = np.where(keep, cur, ref)
    ref.setflags(write=False)
    cur = np.ascontiguousarray(cur)
    cur.setflags(write=False)
    return ref, cur


@functools.lru_cache(maxsize=None)
def oracle(kind, extent, extra):
    import oracle_py as O
    ref, cur = frames(kind, extent)
    return O.affine_me_pair(ref, cur, LAM, extra, modes=(2,))


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C").view(np.int16)).cuda()  # a writable copy


def run_batch(eng, kind, extent, extra, launches=1):
    """The batch entry point, modes = 1: `launches` jobs of one pair each."""
    import torch
    ref, cur = frames(kind, extent)
    jobs = [(dev(cur), [dev(ref)], LAM, eng.alloc_poc(1, 1)) for _ in range(launches)]
    eng.affine_me_batch(jobs, 1, extra)
    torch.cuda.synchronize()
    return [{n: (j[3][(0, n)][0].cpu().numpy(), j[3][(0, n)][1].cpu().numpy()) for n in NAMES} for j in jobs]


def cu_of_row(align, row):
    """'WxH at (x, y)' of a result row (failure messages)."""
    import oracle_py as O
    per = 284 if align else 201
    ctu, off = divmod(int(row), per)
    for w, h, xs, ys, stride in O.group_geometry(align):
        if stride <= off < stride + len(xs):
            return f"{w}x{h} at ({ctu % 4 * 128 + int(xs[off - stride])}, {ctu // 4 * 128 + int(ys[off - stride])})"
    return "?"


def check(got, kind, extent, extra, what):
    want = oracle(kind, extent, extra)
    for name, key in NAMES.items():
        cost, cp = got[name]
        oc, op = want[key]
        ocp = np.stack([op[f] for f in ("LTx", "LTy", "RTx", "RTy", "LBx", "LBy")], 1)
        bad = np.nonzero((cost != oc) | (cp[:, 1:7] != ocp).any(1))[0]
        where = "; ".join(f"row {r} = {cu_of_row(key[0], r)}: cost {cost[r]} want {oc[r]}, cpmv {cp[r, 1:5]} want "
                          f"{ocp[r, :4]}" for r in bad[:8])
        np.testing.assert_array_equal(cost, oc, err_msg=f"{what} {kind}/{extent} {name} cost: {where}")
        np.testing.assert_array_equal(cp[:, 1:7], ocp, err_msg=f"{what} {kind}/{extent} {name} cpmv: {where}")
        assert (cp[:, 0] == 2).all()


if __name__ == "__main__":  # case (a)'s batch results of the library VAME_LIB names
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "vvc-affine-gpu_amd"))
    from vame.engine import Engine
    e = Engine(W, H, 0)
    out = {}
    for ext in ("two_ctu", "frame"):
        for n, (c, p) in run_batch(e, "mixed", ext, 0)[0].items():
            out[f"{ext}_{n}_cost"], out[f"{ext}_{n}_cpmv"] = c, p
    e.close()
    np.savez(sys.argv[1], **out)
    sys.exit(0)

import pytest  # noqa: E402

pytestmark = pytest.mark.gpu
EXTENTS = ("two_ctu", "frame")


@pytest.fixture(scope="module")
def eng():
    from vame.engine import Engine
    e = Engine(W, H, 0)
    yield e
    e.close()


def both_entry_points(eng, kind, extent, extra):
    import torch
    check(run_batch(eng, kind, extent, extra)[0], kind, extent, extra, "batch")
    ref, cur = frames(kind, extent)
    d_ref, d_cur = dev(ref), dev(cur)
    got = {}
    for name, (align, _) in NAMES.items():
        c, p = eng.affine_me(d_ref, d_cur, LAM, align, 2, extra)
        torch.cuda.synchronize()
        got[name] = (c.cpu().numpy(), p.cpu().numpy())
    check(got, kind, extent, extra, "per-launch")


def test_content_settles_unevenly():
    """The premise of case (a), on the oracle's results: CUs of 32x32 and
    32x16 on a still region keep the zero CPMVs, their textured neighbours
    move -- so waves hold settled and live CUs side by side."""
    import oracle_py as O
    _, op = oracle("mixed", "two_ctu", 0)[(0, 2)]
    moved = (np.stack([op[f] for f in ("LTx", "LTy", "RTx", "RTy")], 1) != 0).any(1)
    n = 0
    for w, h, xs, ys, stride in O.group_geometry(0):
        if (w, h) not in ((32, 32), (32, 16)):
            continue
        for ctu in range(2):  # the two CTUs inside the 256x128 pattern
            for k in range(len(xs)):
                x, y = ctu * 128 + int(xs[k]), int(ys[k])
                still = bool(still_mask(H, W)[y:y + h, x:x + w].all())
                row = ctu * 201 + stride + k
                assert not (still and moved[row]), (w, h, x, y)
                n += still
    assert n >= 8 and moved.sum() > n


@pytest.mark.parametrize("extent", EXTENTS)
def test_mixed_settling(eng, extent):
    """(a) still 32x32 / 32x16 regions beside textured regions under a
    fractional affine motion."""
    both_entry_points(eng, "mixed", extent, 0)


@pytest.mark.parametrize("extent", EXTENTS)
def test_identical_frames(eng, extent):
    """(b) every CU settles at the first update: zero live CUs, no hand-over."""
    both_entry_points(eng, "same", extent, 0)
    for name, (cost, cp) in run_batch(eng, "same", extent, 0)[0].items():
        assert (cp[:, 1:7] == 0).all(), name


@pytest.mark.parametrize("extent", EXTENTS)
def test_noise_large_motion(eng, extent):
    """(c) noise displaced by (13, -9): few CUs settle."""
    both_entry_points(eng, "noise", extent, 0)


@pytest.mark.parametrize("extent", EXTENTS)
def test_mixed_settling_extra_iterations(eng, extent):
    """(d) case (a) with ExtraGradientIter = 2."""
    both_entry_points(eng, "mixed", extent, 2)


@pytest.mark.parametrize("extent", EXTENTS)
def test_mixed_settling_two_launches(extent):
    """(e) case (a) as a batch of two launches (one pair per launch)."""
    from vame.engine import Engine
    e = Engine(W, H, 0)
    try:
        e.set_max_pairs(1)
        for got in run_batch(e, "mixed", extent, 0, launches=2):
            check(got, "mixed", extent, 0, "two launches")
    finally:
        e.close()


def test_equals_build_without_handover(eng, tmp_path):
    """Case (a) with and without the hand-over, where the variant library has
    been built: equal outputs, both extents."""
    from vame import _lib
    variant = os.path.join(os.path.dirname(_lib.LIB_PATH), "libvame_norelayout.so")
    mine = {f"{ext}_{n}_{k}": v for ext in EXTENTS for n, cv in run_batch(eng, "mixed", ext, 0)[0].items()
            for k, v in zip(("cost", "cpmv"), cv)}
    if not os.path.exists(variant):
        return  # nothing to compare with: the oracle comparisons above stand alone
    out = str(tmp_path / "variant.npz")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=dict(os.environ, VAME_LIB=variant),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    z = np.load(out)
    assert sorted(z.files) == sorted(mine)
    for k in mine:
        np.testing.assert_array_equal(mine[k], z[k], err_msg=k)
