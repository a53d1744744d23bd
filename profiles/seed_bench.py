#!/usr/bin/env python3
"""Times the seeding of the affine search at 1920x1080 and 3840x2160 on a
synthetic QP32 POC with 4 reference frames, in one process:
  (a) vame_seed_search at radius 8, 16 and 32, both alignments
  (b) vame_affine_me_seeded from the radius-16 seeds, modes 1 (2-CP) and 3
      (2-CP then 3-CP), on a preallocated work buffer
  (c) the search of the same POC (affine_me_poc, modes 1 and 3): for scale
Device events around `--calls` queued calls after `--warmup`.  Before timing:
vame_affine_mc on the improved rows must return exactly their stored costs, no
cost may rise, and two calls must agree.  Also reports the number of non-zero
seeds, the rows improved and the summed cost before and after.  Writes JSON
(default profiles/seed_bench.json).

    python profiles/seed_bench.py [--calls 50] [--warmup 5] [--out FILE]
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

RADII = (8, 16, 32)


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


def one_resolution(W, H, calls, warmup):
    from vame import mc as M
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
    base = eng.affine_me_poc(cur, refs, lam, modes=3)
    seed_out = {r: eng.seed_search(cur, refs, lam, radius=r) for r in RADII}
    seeds = seed_out[16]["mv"]
    torch.cuda.synchronize()

    # consistency before timing
    res, bad = eng.affine_me_seeded(cur, refs, lam, clone(base), seeds, modes=3)
    again, _ = eng.affine_me_seeded(cur, refs, lam, clone(base), seeds, modes=3)
    seed_again = eng.seed_search(cur, refs, lam, radius=16)
    torch.cuda.synchronize()
    assert int(bad) == 0
    assert all(torch.equal(res[k][0], again[k][0]) and torch.equal(res[k][1], again[k][1]) for k in res), \
        "vame_affine_me_seeded is not deterministic"
    assert all(torch.equal(seed_again["mv"][k], seeds[k]) and torch.equal(seed_again["cost"][k], seed_out[16]["cost"][k])
               for k in seeds), "vame_seed_search is not deterministic"
    improved = {n: 0 for n in MODES}
    before = after = nonzero = inframe = 0
    for (r, name), (c, p) in res.items():
        m = MODES.index(name)
        bc = base[(r, name)][0]
        assert (c <= bc).all(), "a cost rose"
        cus, rows = M.cus_from_result(W, H, m >> 1, 2 + (m & 1), p, ref=r)
        took = c[rows] < bc[rows]
        _, mc, b2 = eng.affine_mc(cus[took].contiguous(), refs, lam, cur=cur, want_cost=True)
        torch.cuda.synchronize()
        assert int(b2) == 0 and torch.equal(mc, c[rows][took]), "costs differ from affine_mc's"
        improved[name] += int(took.sum())
        before += int(bc[rows].sum())
        after += int(c[rows].sum())
        if not m & 1:
            nonzero += int((seeds[(r, m >> 1)][rows] != 0).any(1).sum())
            inframe += rows.numel()
    out = {"resolution": [W, H], "nrefs": nrefs, "qp": qp, "lambda": lam, "ctus": eng.n_ctus,
           "inframe_rows_per_model": inframe, "nonzero_seeds_radius16": nonzero, "rows_improved": improved,
           "cost_before": before, "cost_after": after, "costs_equal_affine_mc": True}

    V = ctypes.c_void_p
    L, h, stream = lib(), eng._h, V(torch.cuda.current_stream(dev).cuda_stream)
    ref_ptrs = (V * nrefs)(*[r.data_ptr() for r in refs])
    work = torch.empty(L.vame_seeded_work_bytes(h, nrefs, 3) // 8 + 1, dtype=torch.int64, device=dev)
    sbad = torch.zeros((), dtype=torch.int32, device=dev)
    sp = ((V * 2) * 4)()
    for (r, a), t in seeds.items():
        sp[r][a] = t.data_ptr()
    target = {3: clone(base), 1: {k: v for k, v in clone(base).items() if k[1].endswith("2CP")}}
    prs = {}
    for modes, d in target.items():
        prs[modes] = PocResult()
        for (r, name), (c, p) in d.items():
            prs[modes].cost[r][MODES.index(name)], prs[modes].cpmvs[r][MODES.index(name)] = c.data_ptr(), p.data_ptr()

    def call_seeded(modes):
        check(L.vame_affine_me_seeded(h, V(cur.data_ptr()), ref_ptrs, nrefs, lam, modes, 0, sp, ctypes.byref(prs[modes]),
                                      V(work.data_ptr()), work.numel() * 8, V(sbad.data_ptr()), stream))

    sres = {m: eng.alloc_poc(nrefs, m) for m in (1, 3)}

    def call_search(modes):
        eng.affine_me_poc(cur, refs, lam, modes=modes, out=sres[modes])

    def call_seed(radius):
        eng.seed_search(cur, refs, lam, radius=radius, out=seed_out[radius])

    # the search first and last: the clocks settle over the run
    s0 = {m: timed(lambda: call_search(m), calls, warmup) for m in (1, 3)}
    t_seed = {r: timed(lambda: call_seed(r), calls, warmup) for r in RADII}
    t_seeded = {m: timed(lambda: call_seeded(m), calls, warmup) for m in (1, 3)}
    s1 = {m: timed(lambda: call_search(m), calls, warmup) for m in (1, 3)}
    ts = {m: min(s0[m], s1[m]) for m in (1, 3)}
    for m in (1, 3):
        out[f"search_modes{m}_ms"] = round(ts[m], 5)
        out[f"search_modes{m}_ms_first_last"] = [round(s0[m], 5), round(s1[m], 5)]
        out[f"seeded_modes{m}_ms"] = round(t_seeded[m], 5)
        out[f"ratio_seeded_modes{m}_over_search_modes{m}"] = round(t_seeded[m] / ts[m], 5)
    for r in RADII:
        out[f"seed_search_radius{r}_ms"] = round(t_seed[r], 5)
        out[f"ratio_seed_search_radius{r}_over_search_modes3"] = round(t_seed[r] / ts[3], 5)
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "seed_bench.json"))
    args = ap.parse_args()
    if args.calls < 20:
        ap.error("--calls must be at least 20")
    res = {"device": torch.cuda.get_device_name(0), "calls": args.calls, "warmup": args.warmup,
           "what": "device events around queued calls; seed_search = vame_seed_search, both alignments, 4 refs; "
                   "seeded = vame_affine_me_seeded from the radius-16 seeds on a preallocated work buffer; "
                   "search = affine_me_poc of the same POC",
           "runs": [one_resolution(W, H, args.calls, args.warmup) for W, H in ((1920, 1080), (3840, 2160))]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
