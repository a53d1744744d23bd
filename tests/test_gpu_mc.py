"""vame_affine_mc on the GPU (Engine.affine_mc): predictions and costs of
caller-given CPMVs, bit for bit against the reference's golden outputs (for
every row, golden cost == SATD of the prediction from the golden CPMVs + their
rate) and against the per-CU CPU reference tests/mc_ref.py."""
import ctypes
import functools
import glob
import os

import numpy as np
import pytest
import torch

import mc_ref
import oracle_py as O
from vame.mc import cus_from_result

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
IDENTITY = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLD, "s416_*.npz"))) + ["s832_qp37_poc1"]
MODES = {"FULL_2CP": (0, 2), "FULL_3CP": (0, 3), "HALF_2CP": (1, 2), "HALF_3CP": (1, 3)}
MVMAX = (1 << 17) - 1


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


def cus_dev(rows):
    return torch.tensor(np.asarray(rows, np.int64).reshape(-1, 12), dtype=torch.int32).cuda()


def blank(H, W):
    return torch.full((H, W), -1, dtype=torch.int16, device="cuda")  # 0xFFFF


def desc(x, y, w, h, ncp, lt, rt=None, lb=None, ref=0):
    rt = lt if rt is None else rt
    lb = lt if lb is None else lb
    return [x, y, w, h, ref, ncp, lt[0], lt[1], rt[0], rt[1], lb[0], lb[1]]


def reference(frames, cur, descs, lam, prof=False):
    """mc_ref per descriptor: ([samples], costs)."""
    preds, costs = [], []
    for d in descs:
        p, c, _ = mc_ref.predict_cu(frames[d[4]], cur, d[0], d[1], d[2], d[3], d[5], d[6:], lam, prof)
        preds.append(p)
        costs.append(c)
    return preds, np.array(costs, np.int64)


def run_and_check(eng, frames, cur, descs, lam, prof=False, check_pred=True):
    """One call for `descs` (non-overlapping when check_pred): every covered
    sample and every cost equal mc_ref, every other sample keeps 0xFFFF."""
    H, W = cur.shape
    pred = blank(H, W) if check_pred else None
    got_pred, cost, bad = eng.affine_mc(cus_dev(descs), [dev(f) for f in frames], lam, cur=dev(cur), pred=pred,
                                        want_cost=True)
    torch.cuda.synchronize()
    want_pred, want_cost = reference(frames, cur, descs, lam, prof)
    assert int(bad) == 0
    np.testing.assert_array_equal(cost.cpu().numpy(), want_cost)
    if check_pred:
        want = np.full((H, W), 0xFFFF, np.uint16)
        for d, p in zip(descs, want_pred):
            assert (want[d[1]:d[1] + d[3], d[0]:d[0] + d[2]] == 0xFFFF).all(), "descriptors overlap"
            want[d[1]:d[1] + d[3], d[0]:d[0] + d[2]] = p
        np.testing.assert_array_equal(got_pred.cpu().numpy().view(np.uint16), want)


# ------------------------------------------------------------------ 1. golden identity
@pytest.mark.parametrize("name", IDENTITY)
def test_golden_cost_identity(engines, name):
    z = load(name)
    W, H, lam = int(z["W"]), int(z["H"]), float(z["lam"])
    eng = engines(W, H)
    ref, cur = dev(z["ref"]), dev(z["cur"])
    for mode, (align, ncp) in MODES.items():
        cus, rows = cus_from_result(W, H, align, ncp, torch.from_numpy(z[mode + "_cpmv"]).cuda())
        _, cost, bad = eng.affine_mc(cus, [ref], lam, cur=cur, want_cost=True)
        torch.cuda.synchronize()
        assert int(bad) == 0
        np.testing.assert_array_equal(cost.cpu().numpy(), z[mode + "_cost"][rows.cpu().numpy()],
                                      err_msg=f"{name} {mode}")


# ------------------------------------------------------------------ 2. samples
@pytest.mark.parametrize("name", ["s416_bigmotion", "s416_noise", "s416_qp32_poc2_ref1"])
@pytest.mark.parametrize("size", [(128, 128), (64, 32), (16, 16)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("ncp", [3, 2])
def test_samples_of_tiling_groups(engines, name, size, ncp):
    z = load(name)
    W, H, lam = int(z["W"]), int(z["H"]), float(z["lam"])
    mode = f"FULL_{ncp}CP"
    cus, rows = cus_from_result(W, H, 0, ncp, torch.from_numpy(z[mode + "_cpmv"]), groups=[size])
    assert len(rows) > 0
    descs = cus.numpy().tolist()
    run_and_check(engines(W, H), [z["ref"]], z["cur"], descs, lam)
    # and the cost is the search's own
    _, cost, _ = engines(W, H).affine_mc(cus.cuda(), [dev(z["ref"])], lam, cur=dev(z["cur"]), want_cost=True)
    np.testing.assert_array_equal(cost.cpu().numpy(), z[mode + "_cost"][rows.numpy()])


# ------------------------------------------------------------------ 3. hand-made CPMVs
def frames416():
    z = load("s416_noise")
    return z["ref"], z["cur"], int(z["W"]), int(z["H"]), float(z["lam"])


@pytest.mark.parametrize("ncp", [2, 3])
def test_all_fractional_phases(engines, ncp):
    """Pure translations over every (fx, fy) phase, with varying integer parts:
    256 disjoint 16x16 CUs (samples and costs), 256 128x64 CUs (costs; they
    overlap) and one 128x64 CU per position of a 3 x 3 tiling (samples)."""
    ref, cur, W, H, lam = frames416()
    eng = engines(W, H)
    mv = lambda k: ((k & 15) + 16 * ((k % 7) - 3), (k >> 4) + 16 * ((k % 5) - 2))  # noqa: E731
    small = [desc(16 * (k % 26), 16 * (k // 26), 16, 16, ncp, mv(k)) for k in range(256)]
    run_and_check(eng, [ref], cur, small, lam)
    big = [desc(128 * (k % 3), 64 * ((k // 3) % 3), 128, 64, ncp, mv(k)) for k in range(256)]
    run_and_check(eng, [ref], cur, big, lam, check_pred=False)
    tiling = [desc(128 * (k % 3), 64 * (k // 3), 128, 64, ncp, mv(29 * k + 7)) for k in range(9)]
    run_and_check(eng, [ref], cur, tiling, lam)


def test_integer_translation_and_spread(engines):
    ref, cur, W, H, lam = frames416()
    eng = engines(W, H)
    descs = []
    for ncp in (2, 3):
        descs.append(desc(32 * ncp, 16, 16, 16, ncp, (32, -48)))             # integer MV
        descs.append(desc(128, 64 * (ncp - 2), 128, 64, ncp, (-160, 16)))
        # RT - LT far beyond the spread limit: every sub-block takes the centre MV
        descs.append(desc(32 * ncp, 64, 16, 16, ncp, (5, -3), (4005, 2997), (-1995, 5003)))
        descs.append(desc(272, 64 * (ncp - 2), 128, 64, ncp, (-7, 9), (30000, -20000), (15000, 25000)))
    for d in descs[2::4] + descs[3::4]:
        assert mc_ref.subblock_mvs(d[6:], d[5], d[0], d[1], d[2], d[3], W, H)[1], "case must fail the spread test"
    for d in descs[0::4] + descs[1::4]:
        assert not mc_ref.subblock_mvs(d[6:], d[5], d[0], d[1], d[2], d[3], W, H)[1]
    run_and_check(eng, [ref], cur, descs, lam)


@pytest.mark.parametrize("w,h", [(16, 16), (128, 64)])
def test_extreme_mvs_at_frame_corners(engines, w, h):
    """LT = +-(2^17 - 1) at the four corners: the MV is clipped against the CU
    position and the windows lie wholly off the frame."""
    ref, cur, W, H, lam = frames416()
    eng = engines(W, H)
    for sx, sy in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
        descs = [desc(x, y, w, h, 2 + (k & 1), (sx * MVMAX, sy * MVMAX))
                 for k, (x, y) in enumerate(((0, 0), (W - w, 0), (0, H - h), (W - w, H - h)))]
        run_and_check(eng, [ref], cur, descs, lam)
    # the most negative component the search clamps to, and a rotation-free zoom from it
    descs = [desc(0, 0, w, h, 3, (-MVMAX - 1, -MVMAX - 1)), desc(W - w, H - h, w, h, 2, (MVMAX, MVMAX), (MVMAX - 64, MVMAX))]
    run_and_check(eng, [ref], cur, descs, lam)


def test_left_and_right_edge_windows(engines):
    """CUs at x = 0 and x = W - 16 with MVs of about one sample: windows that
    cross the left / right frame edge take the per-sample clamped loads."""
    ref, cur, W, H, lam = frames416()
    eng = engines(W, H)
    descs = []
    mvs = [(16, 0), (-16, 0), (21, 7), (-21, -7), (-16, 16), (16, -16), (-27, 3), (27, -3)]
    for k, m in enumerate(mvs):
        descs.append(desc(0, 16 * k, 16, 16, 2 + (k & 1), m))
        descs.append(desc(W - 16, 16 * k, 16, 16, 3 - (k & 1), m))
    descs.append(desc(0, 128, 128, 64, 2, (-21, 5)))
    descs.append(desc(W - 128, 128, 128, 64, 3, (21, -5)))
    run_and_check(eng, [ref], cur, descs, lam)


# ------------------------------------------------------------------ 4. mapping
def mixed_descriptors(n, W, H, nrefs, seed=0x3C0DE):
    rng = np.random.default_rng(seed)
    sizes = [(128, 128), (16, 16), (64, 32), (32, 128), (16, 64), (128, 16), (32, 32), (64, 64)]
    out = []
    for k in range(n):
        w, h = sizes[k % len(sizes)]
        x = 4 * int(rng.integers(0, (W - w) // 4 + 1))
        y = 4 * int(rng.integers(0, (H - h) // 4 + 1))
        lt = rng.integers(-400, 401, 2)
        rt = lt + rng.integers(-60, 61, 2)
        lb = lt + rng.integers(-60, 61, 2)
        out.append(desc(x, y, w, h, 2 + int(rng.integers(0, 2)), lt.tolist(), rt.tolist(), lb.tolist(),
                        ref=int(rng.integers(0, nrefs))))
    order = rng.permutation(n)
    return [out[i] for i in order]


@pytest.fixture(scope="module")
def mapping_case(engines):
    """1025 shuffled descriptors of mixed sizes over two refs, and the cost of
    each one run alone (the first 17 also checked against mc_ref)."""
    ref, cur, W, H, lam = frames416()
    ref2 = np.ascontiguousarray(np.roll(ref, (3, -5), (0, 1)))
    eng = engines(W, H)
    descs = mixed_descriptors(1025, W, H, 2)
    refs, dcur = [dev(ref), dev(ref2)], dev(cur)
    allc = cus_dev(descs)
    alone = torch.stack([eng.affine_mc(allc[k:k + 1], refs, lam, cur=dcur, want_cost=True)[1][0]
                         for k in range(len(descs))])
    torch.cuda.synchronize()
    alone = alone.cpu().numpy()
    np.testing.assert_array_equal(alone[:17], reference([ref, ref2], cur, descs[:17], lam)[1])
    return eng, refs, dcur, lam, allc, alone


@pytest.mark.parametrize("n", [1, 3, 17, 1025])
def test_mapping_of_mixed_sizes(mapping_case, n):
    eng, refs, dcur, lam, allc, alone = mapping_case
    _, cost, bad = eng.affine_mc(allc[:n].contiguous(), refs, lam, cur=dcur, want_cost=True)
    torch.cuda.synchronize()
    assert int(bad) == 0
    np.testing.assert_array_equal(cost.cpu().numpy(), alone[:n])


# ------------------------------------------------------------------ 5. invalid descriptors
def test_invalid_descriptors(engines):
    from vame._lib import lib
    ref, cur, W, H, lam = frames416()
    eng = engines(W, H)
    refs, dcur = [dev(ref), dev(cur)], dev(cur)
    valid = [desc(0, 0, 16, 16, 2, (5, 9)), desc(64, 32, 64, 32, 3, (-33, 18), (-30, 20), (-35, 15), ref=1),
             desc(128, 64, 128, 128, 2, (100, -100), (110, -95)),
             # LB is not used by the 4-parameter model: out of range there is still valid
             desc(32, 0, 16, 16, 2, (1, 2), (3, 4), (1 << 17, -(1 << 17) - 1))]
    invalid = [desc(16, 200, 48, 16, 2, (0, 0)),                    # bad size
               desc(32, 200, 16, 8, 2, (0, 0)),
               desc(50, 200, 16, 16, 2, (0, 0)),                    # unaligned x
               desc(64, 202, 16, 16, 2, (0, 0)),                    # unaligned y
               desc(W - 8, 200, 16, 16, 2, (0, 0)),                 # out of frame
               desc(96, H - 8, 16, 16, 2, (0, 0)),
               desc(-4, 200, 16, 16, 2, (0, 0)),
               desc(112, 200, 16, 16, 2, (0, 0), ref=2),            # ref = nrefs
               desc(128, 200, 16, 16, 2, (0, 0), ref=-1),
               desc(144, 200, 16, 16, 1, (0, 0)),                   # nCPs
               desc(160, 200, 16, 16, 4, (0, 0)),
               desc(176, 200, 16, 16, 2, (1 << 17, 0)),             # component = 2^17
               desc(192, 200, 16, 16, 2, (0, 0), (0, -(1 << 17) - 1)),
               desc(208, 200, 16, 16, 3, (0, 0), (0, 0), (0, 1 << 17))]
    # valid rows alone
    pred0 = blank(H, W)
    _, cost0, bad0 = eng.affine_mc(cus_dev(valid), refs, lam, cur=dcur, pred=pred0, want_cost=True)
    assert int(bad0) == 0
    np.testing.assert_array_equal(cost0.cpu().numpy(), reference([ref, cur], cur, valid, lam)[1])
    # mixed: invalid rows between, before and after the valid ones
    mixed, is_valid = [], []
    vi = iter(valid)
    for k, d in enumerate(invalid):
        mixed.append(d)
        is_valid.append(False)
        if k % 4 == 1:
            mixed.append(next(vi))
            is_valid.append(True)
    assert next(vi, None) is None
    is_valid = np.array(is_valid)
    pred1 = blank(H, W)
    _, cost1, bad1 = eng.affine_mc(cus_dev(mixed), refs, lam, cur=dcur, pred=pred1, want_cost=True)
    torch.cuda.synchronize()
    assert int(bad1) == 1
    c1 = cost1.cpu().numpy()
    assert (c1[~is_valid] == 0).all()
    np.testing.assert_array_equal(c1[is_valid], cost0.cpu().numpy())
    assert torch.equal(pred1, pred0)  # the valid CUs' samples, 0xFFFF everywhere else
    assert (pred1[200:, :].cpu().numpy() == -1).all()
    # only invalid rows: nothing written
    pred2 = blank(H, W)
    _, cost2, bad2 = eng.affine_mc(cus_dev(invalid), refs, lam, cur=dcur, pred=pred2, want_cost=True)
    assert int(bad2) == 1 and (cost2 == 0).all() and (pred2 == -1).all()
    # no descriptors: a no-op
    empty = torch.empty((0, 12), dtype=torch.int32, device="cuda")
    pred3 = blank(H, W)
    _, cost3, bad3 = eng.affine_mc(empty, refs, lam, cur=dcur, pred=pred3, want_cost=True)
    assert cost3.numel() == 0 and int(bad3) == 0 and (pred3 == -1).all()
    # neither output
    with pytest.raises(ValueError):
        eng.affine_mc(cus_dev(valid), refs, lam)
    badflag = torch.zeros((), dtype=torch.int32, device="cuda")
    ptrs = (ctypes.c_void_p * 2)(refs[0].data_ptr(), refs[1].data_ptr())
    V = ctypes.c_void_p
    d = cus_dev(valid)
    L = lib()
    assert L.vame_affine_mc(eng._h, V(dcur.data_ptr()), ptrs, 2, V(d.data_ptr()), len(valid), lam, None, None,
                            V(badflag.data_ptr()), None) == -1
    assert L.vame_affine_mc(eng._h, None, ptrs, 2, V(d.data_ptr()), len(valid), lam, None, V(cost0.data_ptr()),
                            V(badflag.data_ptr()), None) == -1  # cost without cur
    assert L.vame_affine_mc(eng._h, V(dcur.data_ptr()), ptrs, 5, V(d.data_ptr()), len(valid), lam, None,
                            V(cost0.data_ptr()), V(badflag.data_ptr()), None) == -1
    assert L.vame_affine_mc(eng._h, V(dcur.data_ptr()), ptrs, 2, V(d.data_ptr()), (1 << 20) + 1, lam, None,
                            V(cost0.data_ptr()), V(badflag.data_ptr()), None) == -1
    assert L.vame_affine_mc(eng._h, V(dcur.data_ptr()), ptrs, 2, None, 0, lam, None, V(cost0.data_ptr()),
                            V(badflag.data_ptr()), None) == 0
    torch.cuda.synchronize()
    assert int(badflag) == 0
    # wrong shapes / dtypes / devices
    with pytest.raises(ValueError):
        eng.affine_mc(cus_dev(valid).to(torch.int64), refs, lam, cur=dcur, want_cost=True)
    with pytest.raises(ValueError):
        eng.affine_mc(cus_dev(valid)[:, :11], refs, lam, cur=dcur, want_cost=True)
    with pytest.raises(ValueError):
        eng.affine_mc(cus_dev(valid).cpu(), refs, lam, cur=dcur, want_cost=True)
    with pytest.raises(ValueError):
        eng.affine_mc(cus_dev(valid), refs, lam, want_cost=True)  # no cur
    with pytest.raises(ValueError):
        eng.affine_mc(cus_dev(valid), refs, lam, pred=blank(H, W + 16)[:, :W])


# ------------------------------------------------------------------ 6. PROF
def test_prof(engines):
    """With vame_set_prof on, the CPMVs of the oracle's PROF search cost what
    that search says, and the samples equal mc_ref's PROF prediction."""
    from vame.engine import Engine
    z = load("s416_qp32_poc1_ref0")
    W, H, lam = int(z["W"]), int(z["H"]), float(z["lam"])
    c2, p2 = O.affine_me(z["ref"], z["cur"], lam, 0, 2, prof=True)
    c3, p3 = O.affine_me(z["ref"], z["cur"], lam, 0, 3, prev=p2, prof=True)
    eng = Engine(W, H, 0)  # a context of its own: the others stay PROF-off
    try:
        eng.set_prof(True)
        ref, cur = dev(z["ref"]), dev(z["cur"])
        for ncp, c, p in ((2, c2, p2), (3, c3, p3)):
            cp6 = np.stack([p[f] for f in ("LTx", "LTy", "RTx", "RTy", "LBx", "LBy")], 1)
            cus, rows = cus_from_result(W, H, 0, ncp, torch.from_numpy(cp6).cuda())
            _, cost, bad = eng.affine_mc(cus, [ref], lam, cur=cur, want_cost=True)
            torch.cuda.synchronize()
            assert int(bad) == 0
            np.testing.assert_array_equal(cost.cpu().numpy(), c[rows.cpu().numpy()], err_msg=f"PROF {ncp}CP")
            g32, _ = cus_from_result(W, H, 0, ncp, torch.from_numpy(cp6), groups=[(32, 32)])
            run_and_check(eng, [z["ref"]], z["cur"], g32.numpy().tolist(), lam, prof=True)
    finally:
        eng.close()


# ------------------------------------------------------------------ 7. graph capture
def test_captured_call_replays(engines):
    z = load("s416_qp32_poc2_ref0")
    W, H, lam = int(z["W"]), int(z["H"]), float(z["lam"])
    eng = engines(W, H)
    ref, cur = dev(z["ref"]), dev(z["cur"])
    cus, _ = cus_from_result(W, H, 0, 3, torch.from_numpy(z["FULL_3CP_cpmv"]).cuda(), groups=[(32, 16)])
    want_pred, want_cost, _ = eng.affine_mc(cus, [ref], lam, cur=cur, pred=blank(H, W), want_cost=True)
    torch.cuda.synchronize()
    pred = blank(H, W)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _, cost, bad = eng.affine_mc(cus, [ref], lam, cur=cur, pred=pred, want_cost=True)
    pred.fill_(-1)
    cost.fill_(-1)
    bad.fill_(7)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(pred, want_pred) and torch.equal(cost, want_cost) and int(bad) == 0
