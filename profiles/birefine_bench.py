#!/usr/bin/env python3
"""Times the refinement of bi-predicted CUs (vame_bipred_refine, rounds = 2) at
1920x1080 and 3840x2160 on a synthetic QP32 POC with 4 reference frames and all
four PREDs, in one process:
  (a) refining the leaves of vame_partition_bi (their count read on the device)
  (b) refining every candidate CU with a pair (bi_sel >= 0), both alignments
  (c) vame_bipred and the 2+3-CP search of the same POC (affine_me_poc,
      modes = 3, 4 refs): for scale
Device events around `--calls` queued calls after `--warmup`; the C ABI is
called directly on preallocated outputs.  Before timing: vame_affine_mc_bi on
the refined descriptors must return exactly the refined costs, no cost may
rise, and two calls must agree.  Also reports how many candidates improved and
the summed cost before and after.  Writes JSON (default
profiles/birefine_bench.json).

    python profiles/birefine_bench.py [--calls 100] [--warmup 10] [--out FILE]
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

ROUNDS = 2


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
    from vame._lib import check, lib
    from vame.engine import Engine
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
    bi = eng.bipred(cur, refs, lam, res)
    part = eng.partition_bi(res, bi)
    torch.cuda.synchronize()

    # every candidate with a pair, both alignments, as one descriptor array
    rows = [torch.nonzero(bi["sel"][a] >= 0).reshape(-1) for a in (0, 1)]
    every = torch.cat([B.bicus_from_sel(W, H, a, res, bi["sel"][a], rows[a]) for a in (0, 1)]).contiguous()
    before_all = torch.cat([bi["cost"][a][rows[a]] for a in (0, 1)])
    cap = eng.n_ctus * 64
    V = ctypes.c_void_p
    ref_ptrs = (V * nrefs)(*[r.data_ptr() for r in refs])
    L, h, stream = lib(), eng._h, V(torch.cuda.current_stream(dev).cuda_stream)
    bad = torch.zeros((), dtype=torch.int32, device=dev)
    leaf_out, leaf_cost = torch.zeros_like(part["cus"]), torch.zeros(cap, dtype=torch.int64, device=dev)
    all_out, all_cost = torch.zeros_like(every), torch.zeros(every.shape[0], dtype=torch.int64, device=dev)

    def refine(cus, n, count, out, cost):
        check(L.vame_bipred_refine(h, V(cur.data_ptr()), ref_ptrs, nrefs, V(cus.data_ptr()), n,
                                   None if count is None else V(count.data_ptr()), lam, ROUNDS, V(out.data_ptr()),
                                   V(cost.data_ptr()), V(bad.data_ptr()), stream))

    def call_leaves():
        refine(part["cus"], cap, part["ncus"], leaf_out, leaf_cost)

    def call_all():
        refine(every, every.shape[0], None, all_out, all_cost)

    bi_out = B.alloc_bi(eng.n_ctus, dev)

    def call_bipred():
        eng.bipred(cur, refs, lam, res, out=bi_out)

    def call_search():
        eng.affine_me_poc(cur, refs, lam, modes=3, out=res)

    # consistency before timing
    call_leaves()
    call_all()
    torch.cuda.synchronize()
    n = int(part["ncus"])
    first = [t.clone() for t in (leaf_out[:n], leaf_cost[:n], all_out, all_cost)]
    call_leaves()
    call_all()
    _, mc_leaf, bad1 = eng.affine_mc_bi(leaf_out, refs, lam, cur=cur, want_cost=True, ncus=part["ncus"])
    _, mc_all, bad2 = eng.affine_mc_bi(all_out, refs, lam, cur=cur, want_cost=True)
    _, leaf_before, _ = eng.affine_mc_bi(part["cus"], refs, lam, cur=cur, want_cost=True, ncus=part["ncus"])
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, (leaf_out[:n], leaf_cost[:n], all_out, all_cost))), \
        "vame_bipred_refine is not deterministic"
    assert int(bad) == 0 and int(bad1) == 0 and int(bad2) == 0
    assert torch.equal(mc_leaf[:n], leaf_cost[:n]) and torch.equal(mc_all, all_cost), "costs differ from affine_mc_bi's"
    assert (all_cost <= before_all).all() and (leaf_cost[:n] <= leaf_before[:n]).all(), "a cost rose"
    bi_leaf = part["sel"][:n] >= 0
    out = {"resolution": [W, H], "nrefs": nrefs, "preds": 15, "qp": qp, "lambda": lam, "ctus": eng.n_ctus,
           "rounds": ROUNDS, "leaves": n, "bi_leaves": int(bi_leaf.sum()),
           "bi_leaves_improved": int((leaf_cost[:n] < leaf_before[:n]).sum()),
           "leaf_cost_before": int(leaf_before[:n].sum()), "leaf_cost_after": int(leaf_cost[:n].sum()),
           "candidates_with_a_pair": int(every.shape[0]), "candidates_improved": int((all_cost < before_all).sum()),
           "candidate_cost_before": int(before_all.sum()), "candidate_cost_after": int(all_cost.sum()),
           "costs_equal_affine_mc_bi": True}
    # the search first and last: the clocks settle over the run
    s0 = timed(call_search, calls, warmup)
    tb = timed(call_bipred, calls, warmup)
    tl = timed(call_leaves, calls, warmup)
    ta = timed(call_all, calls, warmup)
    s1 = timed(call_search, calls, warmup)
    ts = min(s0, s1)
    out["refine_leaves_ms"] = round(tl, 5)
    out["refine_candidates_ms"] = round(ta, 5)
    out["bipred_ms"] = round(tb, 5)
    out["search_2cp_3cp_ms"] = round(ts, 5)
    out["search_ms_first_last"] = [round(s0, 5), round(s1, 5)]
    out["ratio_refine_leaves_over_search"] = round(tl / ts, 5)
    out["ratio_refine_candidates_over_search"] = round(ta / ts, 5)
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "birefine_bench.json"))
    args = ap.parse_args()
    if args.calls < 50:
        ap.error("--calls must be at least 50")
    res = {"device": torch.cuda.get_device_name(0), "calls": args.calls, "warmup": args.warmup,
           "what": "device events around queued calls; refine_leaves = vame_bipred_refine on vame_partition_bi's "
                   "leaves (penalties 0, device-side count); refine_candidates = on every candidate CU with a pair; "
                   "bipred = vame_bipred, mask 15; search = affine_me_poc, modes = 3",
           "runs": [one_resolution(W, H, args.calls, args.warmup) for W, H in ((1920, 1080), (3840, 2160))]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
