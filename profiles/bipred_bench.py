#!/usr/bin/env python3
"""Times affine bi-prediction at 1920x1080 and 3840x2160 on a synthetic QP32
POC with 4 reference frames and all four PREDs, in one process:
  (a) vame_bipred alone (the best reference pair of every candidate CU)
  (b) vame_bipred + vame_partition_bi + vame_affine_mc_bi on its leaves
      (predicted frame + costs)
  (c) the 2+3-CP search of the same POC (affine_me_poc, modes = 3, 4 refs):
      the yardstick
Device events around `--calls` queued calls after `--warmup`; the C ABI is
called directly on preallocated outputs.  Before timing, the leaves' mc costs
summed per CTU must equal ctu_cost, and two vame_bipred calls must agree.
Writes the times and their ratios to the search as JSON (default
profiles/bipred_bench.json).

    python profiles/bipred_bench.py [--calls 100] [--warmup 10] [--out FILE]
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


def one_resolution(W, H, calls, warmup):
    from vame import bipred as B
    from vame import synth
    from vame._lib import PocResult, check, lib
    from vame.engine import MODES, Engine
    from vame.hostlogic import lambda_for_poc

    qp, nrefs = 32, 4
    orig, recon = synth.synth_sequence(W, H, nrefs + 1, qp)
    lam = lambda_for_poc(qp, nrefs)
    dev = torch.device("cuda", 0)
    cur = torch.from_numpy(orig[nrefs].view(np.int16)).to(dev)
    refs = [torch.from_numpy(recon[nrefs - 1 - r].view(np.int16)).to(dev) for r in range(nrefs)]
    eng = Engine(W, H, 0)
    eng.set_max_pairs(nrefs)
    res = eng.alloc_poc(nrefs, 3)
    eng.affine_me_poc(cur, refs, lam, modes=3, out=res)
    torch.cuda.synchronize()

    pr = PocResult()
    for (r, name), (c, p) in res.items():
        pr.cost[r][MODES.index(name)] = c.data_ptr()
        pr.cpmvs[r][MODES.index(name)] = p.data_ptr()
    bi = B.alloc_bi(eng.n_ctus, dev)
    part = B.alloc(eng.n_ctus, dev)
    pred = torch.zeros((H, W), dtype=torch.int16, device=dev)
    cost = torch.zeros(eng.n_ctus * 64, dtype=torch.int64, device=dev)
    bad = torch.zeros((), dtype=torch.int32, device=dev)
    V = ctypes.c_void_p
    ref_ptrs = (V * nrefs)(*[r.data_ptr() for r in refs])
    bi_cost = (V * 2)(*[t.data_ptr() for t in bi["cost"]])
    bi_sel = (V * 2)(*[t.data_ptr() for t in bi["sel"]])
    L, h, stream = lib(), eng._h, V(torch.cuda.current_stream(dev).cuda_stream)

    def call_bipred():
        check(L.vame_bipred(h, V(cur.data_ptr()), ref_ptrs, nrefs, lam, ctypes.byref(pr), 15, bi_cost, bi_sel, stream))

    def call_chain():
        call_bipred()
        check(L.vame_partition_bi(h, ctypes.byref(pr), nrefs, 15, 0, bi_cost, bi_sel, 0,
                                  *(V(part[k].data_ptr()) for k in B.KEYS), stream))
        check(L.vame_affine_mc_bi(h, V(cur.data_ptr()), ref_ptrs, nrefs, V(part["cus"].data_ptr()), eng.n_ctus * 64,
                                  V(part["ncus"].data_ptr()), lam, V(pred.data_ptr()), V(cost.data_ptr()),
                                  V(bad.data_ptr()), stream))

    def call_search():
        eng.affine_me_poc(cur, refs, lam, modes=3, out=res)

    call_chain()
    torch.cuda.synchronize()
    first = [t.clone() for t in bi["cost"] + bi["sel"]]
    call_bipred()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, bi["cost"] + bi["sel"])), "vame_bipred is not deterministic"
    n = int(part["ncus"])
    info = part["ctu_info"].cpu().numpy()
    csum = np.concatenate([[0], np.cumsum(cost.cpu().numpy()[:n])])
    per_ctu = csum[info[:, 0] + info[:, 1]] - csum[info[:, 0]]
    assert int(bad) == 0 and (per_ctu == part["ctu_cost"].cpu().numpy()).all(), "mc costs differ from the decision's"
    sel = part["sel"].cpu().numpy()[:n]
    rows_with_pair = sum(int((t >= 0).sum()) for t in bi["sel"])
    out = {"resolution": [W, H], "nrefs": nrefs, "preds": 15, "qp": qp, "lambda": lam, "ctus": eng.n_ctus,
           "rows_with_a_pair": rows_with_pair, "leaves": n, "bi_leaves": int((sel >= 0).sum()),
           "mc_costs_equal_ctu_cost": True}
    # the search first and last: the clocks settle over the run
    s0 = timed(call_search, calls, warmup)
    tb = timed(call_bipred, calls, warmup)
    tc = timed(call_chain, calls, warmup)
    s1 = timed(call_search, calls, warmup)
    ts = min(s0, s1)
    out["bipred_ms"] = round(tb, 5)
    out["bipred_partition_mc_ms"] = round(tc, 5)
    out["search_2cp_3cp_ms"] = round(ts, 5)
    out["search_ms_first_last"] = [round(s0, 5), round(s1, 5)]
    out["ratio_bipred_over_search"] = round(tb / ts, 5)
    out["ratio_chain_over_search"] = round(tc / ts, 5)
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bipred_bench.json"))
    args = ap.parse_args()
    if args.calls < 50:
        ap.error("--calls must be at least 50")
    res = {"device": torch.cuda.get_device_name(0), "calls": args.calls, "warmup": args.warmup,
           "what": "device events around queued calls; bipred = vame_bipred, mask 15; bipred_partition_mc = + "
                   "vame_partition_bi (penalties 0) + vame_affine_mc_bi (pred + cost); search = affine_me_poc, "
                   "modes = 3",
           "runs": [one_resolution(W, H, args.calls, args.warmup) for W, H in ((1920, 1080), (3840, 2160))]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
