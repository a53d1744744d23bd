#!/usr/bin/env python3
"""Times vame_affine_mc at 1920x1080 on the synthetic QP32 pair of the c2
bench (POC 1 against the reconstructed POC 0), beside the 2-CP-only search of
the same pair in the same process:
  (a) pred only: the non-overlapping aligned 16x16 partition (8,040 in-frame
      CUs) with the search's best 2-CP CPMVs
  (b) cost only: every in-frame candidate of both alignments with the search's
      best 2-CP CPMVs (60,810 CUs, 2,661,600 sub-blocks); the costs must equal
      the search's
Device events around `--calls` queued calls after `--warmup`; the C ABI is
called directly on preallocated outputs, so the host adds as little as it can.
Writes the three times and their ratios as JSON (default profiles/mc_bench.json).

    python profiles/mc_bench.py [--calls 100] [--warmup 10] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vvc-affine-gpu_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn, calls, warmup):
    """Mean device milliseconds per call of `calls` queued calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(calls):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / calls


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mc_bench.json"))
    args = ap.parse_args()
    if args.calls < 50:
        ap.error("--calls must be at least 50")

    from vame import synth
    from vame._lib import check, lib
    from vame.engine import Engine
    from vame.hostlogic import lambda_for_poc
    from vame.mc import cus_from_result

    W, H, qp = 1920, 1080, 32
    orig, recon = synth.synth_sequence(W, H, 1, qp)
    lam = lambda_for_poc(qp, 1)
    dev = torch.device("cuda", 0)
    cur = torch.from_numpy(orig[0].view(np.int16)).to(dev)
    ref = torch.from_numpy(recon[0].view(np.int16)).to(dev)
    eng = Engine(W, H, 0)
    out = eng.alloc_poc(1, 1)
    eng.affine_me_poc(cur, [ref], lam, modes=1, out=out)
    torch.cuda.synchronize()

    # (a) the aligned 16x16 partition
    cus_a, _ = cus_from_result(W, H, 0, 2, out[(0, "FULL_2CP")][1], groups=[(16, 16)])
    # (b) every in-frame candidate of both alignments
    parts = [cus_from_result(W, H, a, 2, out[(0, name)][1]) for a, name in ((0, "FULL_2CP"), (1, "HALF_2CP"))]
    cus_b = torch.cat([p[0] for p in parts]).contiguous()
    want_b = torch.cat([out[(0, name)][0][p[1]] for p, name in zip(parts, ("FULL_2CP", "HALF_2CP"))])
    sub_b = int((cus_b[:, 2].long() * cus_b[:, 3].long()).sum().item()) // 16
    assert cus_a.shape[0] == 8040 and cus_b.shape[0] == 60810 and sub_b == 2661600, (cus_a.shape, cus_b.shape, sub_b)

    pred = torch.zeros((H, W), dtype=torch.int16, device=dev)
    cost = torch.empty(cus_b.shape[0], dtype=torch.int64, device=dev)
    bad = torch.zeros((), dtype=torch.int32, device=dev)
    refs = (ctypes.c_void_p * 1)(ref.data_ptr())
    V = ctypes.c_void_p
    L, h, stream = lib(), eng._h, V(torch.cuda.current_stream(dev).cuda_stream)

    def call_a():
        check(L.vame_affine_mc(h, None, refs, 1, V(cus_a.data_ptr()), cus_a.shape[0], lam, V(pred.data_ptr()), None,
                               V(bad.data_ptr()), stream))

    def call_b():
        check(L.vame_affine_mc(h, V(cur.data_ptr()), refs, 1, V(cus_b.data_ptr()), cus_b.shape[0], lam, None,
                               V(cost.data_ptr()), V(bad.data_ptr()), stream))

    def call_search():
        eng.affine_me_poc(cur, [ref], lam, modes=1, out=out)

    call_a()
    call_b()
    torch.cuda.synchronize()
    assert int(bad) == 0 and torch.equal(cost, want_b), "costs differ from the search's"
    rows = (H // 16) * 16  # the partition covers rows 0 .. 1071; the last 8 rows keep their zeros
    assert int(pred[:rows].min()) >= 0 and int(pred[:rows].max()) > 0 and int(pred[rows:].abs().max()) == 0

    res = {
        "device": torch.cuda.get_device_name(0),
        "resolution": [W, H], "qp": qp, "lambda": lam, "calls": args.calls, "warmup": args.warmup,
        "a_pred_16x16": {"cus": int(cus_a.shape[0]), "sub_blocks": int(cus_a.shape[0]) * 16},
        "b_cost_all_candidates": {"cus": int(cus_b.shape[0]), "sub_blocks": sub_b, "costs_equal_search": True},
    }
    # the search first and last: the clocks settle over the run
    s0 = timed(call_search, args.calls, args.warmup)
    ta = timed(call_a, args.calls, args.warmup)
    tb = timed(call_b, args.calls, args.warmup)
    s1 = timed(call_search, args.calls, args.warmup)
    ts = min(s0, s1)
    res["a_pred_16x16"]["ms"] = round(ta, 5)
    res["b_cost_all_candidates"]["ms"] = round(tb, 5)
    res["b_cost_all_candidates"]["sub_blocks_per_s"] = round(sub_b / (tb * 1e-3), 0)
    res["search_2cp"] = {"ms": round(ts, 5), "ms_first": round(s0, 5), "ms_last": round(s1, 5),
                         "what": "affine_me_poc, modes = 1, one ref, FULL + HALF"}
    res["ratio_a_over_search"] = round(ta / ts, 4)
    res["ratio_b_over_search"] = round(tb / ts, 4)
    res["b_below_search"] = bool(tb < ts)
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
