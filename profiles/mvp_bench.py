#!/usr/bin/env python3
"""Times the calls that price CPMVs against a motion-vector predictor (DESIGN.md
section 17) against their zero-predictor counterparts, and reports what the
predictor changes, at 1920x1080 on a synthetic QP32 POC with 4 reference
frames and all four PREDs, radius-16 seeds and region_predictors(size = 64),
in one process:
  timing   affine_mc_p / affine_mc_bi and bipred_refine_p / bipred_refine on
           the leaves of partition_bi, affine_search_p / affine_search on the
           seeds' descriptors of refIdx 0, affine_me_seeded_p /
           affine_me_seeded, bipred_p / bipred, and reprice against
           affine_me_poc.  Device events around `--calls` queued calls after
           `--warmup`.
  effect   zero predictor (affine_me_poc -> affine_me_seeded -> bipred ->
           partition_bi) against predictor (affine_me_poc -> reprice ->
           affine_me_seeded_p -> bipred_p -> partition_bi -> leaf_predictors):
           the summed cost of the in-frame rows, the rows the seeded call
           improved, leaves per CTU, the share of bi leaves, and the summed
           SATD (affine_mc_p with lambda = 0) of the predicted frame.
Before timing: with an all-zero predictor every _p call must return its
counterpart's outputs.  Writes JSON (default profiles/mvp_bench.json).

    python profiles/mvp_bench.py [--calls 20] [--warmup 3] [--out FILE]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vvc-affine-gpu_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

W, H = 1920, 1080


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


def clone(res):
    return {k: (c.clone(), p.clone()) for k, (c, p) in res.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mvp_bench.json"))
    args = ap.parse_args()

    from vame import mc as M
    from vame import mvp as MVP
    from vame import seed as V
    from vame import synth
    from vame.engine import Engine
    from vame.hostlogic import lambda_for_poc

    qp, nrefs = 32, 4
    orig, recon = synth.synth_sequence(W, H, nrefs + 1, qp)
    lam = lambda_for_poc(qp, nrefs)
    dev = torch.device("cuda", 0)
    cur = torch.from_numpy(orig[nrefs].view(np.int16)).to(dev)
    refs = [torch.from_numpy(recon[nrefs - 1 - r].view(np.int16)).to(dev) for r in range(nrefs)]
    eng = Engine(W, H, 0)
    names = ("FULL_2CP", "FULL_3CP", "HALF_2CP", "HALF_3CP")

    base = eng.affine_me_poc(cur, refs, lam, modes=3)
    seeds = eng.seed_search(cur, refs, lam, radius=16)["mv"]
    mvp = MVP.region_predictors(W, H, seeds, 64)
    zero = {k: torch.zeros_like(v) for k, v in mvp.items()}
    inframe = {}
    for a in (0, 1):
        _, rows = M.cus_from_result(W, H, a, 2, base[(0, names[2 * a])][1])
        inframe[a] = rows

    def pipeline(with_p):
        res = clone(base)
        if with_p:
            eng.reprice(lam, res, mvp)
        before = {k: c.clone() for k, (c, _) in res.items()}
        if with_p:
            eng.affine_me_seeded_p(cur, refs, lam, res, seeds, mvp, modes=3)
            bi = eng.bipred_p(cur, refs, lam, res, mvp)
        else:
            eng.affine_me_seeded(cur, refs, lam, res, seeds, modes=3)
            bi = eng.bipred(cur, refs, lam, res)
        part = eng.partition_bi(res, bi)
        lp = eng.leaf_predictors(part, mvp if with_p else {})
        pred = torch.zeros((H, W), dtype=torch.int16, device=dev)
        _, satd, bad = eng.affine_mc_p(part["cus"], lp, refs, 0.0, cur=cur, pred=pred, want_cost=True, ncus=part["ncus"])
        _, cost, _ = eng.affine_mc_p(part["cus"], lp, refs, lam, cur=cur, want_cost=True, ncus=part["ncus"])
        torch.cuda.synchronize()
        n = int(part["ncus"])
        assert int(bad) == 0
        rows_cost = sum(int(res[(r, names[m])][0][inframe[m >> 1]].sum()) for r in range(nrefs) for m in range(4))
        improved = sum(int((res[k][0] < before[k]).sum()) for k in res)
        total = sum(len(inframe[m >> 1]) for m in range(4)) * nrefs
        return {"summed_cost_inframe_rows": rows_cost, "rows": total, "rows_improved_by_seeded": improved,
                "leaves": n, "leaves_per_ctu": n / eng.n_ctus, "bi_leaf_share": float((part["cus"][:n, 12] >= 0).sum()) / n,
                "summed_leaf_satd": int(satd[:n].sum()), "summed_leaf_cost": int(cost[:n].sum())}, res, bi, part, lp

    eff0, res0, bi0, part0, lp0 = pipeline(False)
    eff1, res1, bi1, part1, lp1 = pipeline(True)

    # zero predictors give the counterparts' outputs
    chk = clone(base)
    eng.reprice(lam, chk, zero)
    eng.affine_me_seeded_p(cur, refs, lam, chk, seeds, zero, modes=3)
    bz = eng.bipred_p(cur, refs, lam, chk, zero)
    torch.cuda.synchronize()
    for k in res0:
        assert torch.equal(chk[k][0], res0[k][0]) and torch.equal(chk[k][1], res0[k][1]), k
    for a in (0, 1):
        assert torch.equal(bz["cost"][a], bi0["cost"][a]) and torch.equal(bz["sel"][a], bi0["sel"][a])

    c, w = args.calls, args.warmup
    cus12, rows = V.cus_from_seeds(W, H, 0, seeds[(0, 0)], ref=0)
    P = mvp[(0, 0)][rows]
    p12 = torch.cat([torch.full((len(rows), 1), 3, dtype=torch.int32, device=dev), P, P, P], 1).contiguous()
    work = clone(base)

    def reset():
        for k in work:
            work[k][0].copy_(base[k][0])
            work[k][1].copy_(base[k][1])

    def seeded(p):
        reset()
        if p:
            eng.affine_me_seeded_p(cur, refs, lam, work, seeds, mvp, modes=3)
        else:
            eng.affine_me_seeded(cur, refs, lam, work, seeds, modes=3)

    t = {}
    t["reset_ms"] = timed(reset, c, w)
    t["affine_me_poc_ms"] = timed(lambda: eng.affine_me_poc(cur, refs, lam, modes=3, out=work), max(3, c // 4), 1)
    t["reprice_ms"] = timed(lambda: eng.reprice(lam, work, mvp), c, w)
    t["affine_mc_bi_ms"] = timed(lambda: eng.affine_mc_bi(part1["cus"], refs, lam, cur=cur, want_cost=True, ncus=part1["ncus"]), c, w)
    t["affine_mc_p_ms"] = timed(lambda: eng.affine_mc_p(part1["cus"], lp1, refs, lam, cur=cur, want_cost=True, ncus=part1["ncus"]), c, w)
    t["affine_search_ms"] = timed(lambda: eng.affine_search(cus12, refs, cur, lam), c, w)
    t["affine_search_p_ms"] = timed(lambda: eng.affine_search_p(cus12, p12, refs, cur, lam), c, w)
    t["bipred_refine_ms"] = timed(lambda: eng.bipred_refine(part1["cus"], refs, cur, lam, rounds=2, count=part1["ncus"]), c, w)
    t["bipred_refine_p_ms"] = timed(lambda: eng.bipred_refine_p(part1["cus"], lp1, refs, cur, lam, rounds=2, count=part1["ncus"]), c, w)
    t["affine_me_seeded_ms"] = timed(lambda: seeded(False), max(3, c // 4), 1) - t["reset_ms"]
    t["affine_me_seeded_p_ms"] = timed(lambda: seeded(True), max(3, c // 4), 1) - t["reset_ms"]
    t["bipred_ms"] = timed(lambda: eng.bipred(cur, refs, lam, res1, out=bi0), c, w)
    t["bipred_p_ms"] = timed(lambda: eng.bipred_p(cur, refs, lam, res1, mvp, out=bi1), c, w)
    t["leaf_predictors_ms"] = timed(lambda: eng.leaf_predictors(part1, mvp, out=lp1), c, w)
    ratios = {k: t[k + "_p_ms"] / t[k + "_ms"] for k in ("affine_search", "bipred_refine", "affine_me_seeded", "bipred")}
    ratios["affine_mc_p_over_affine_mc_bi"] = t["affine_mc_p_ms"] / t["affine_mc_bi_ms"]
    ratios["reprice_over_affine_me_poc"] = t["reprice_ms"] / t["affine_me_poc_ms"]
    out = {"resolution": [W, H], "qp": qp, "nrefs": nrefs, "lambda": lam, "seed_radius": 16, "region_size": 64,
           "search_descriptors": int(len(rows)), "device": torch.cuda.get_device_name(0), "calls": c,
           "timing_ms": t, "p_call_as_multiple_of_counterpart": ratios,
           "effect": {"zero_predictor": eff0, "predictor": eff1}}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
