#!/usr/bin/env python3
"""Times the wide-range seed search at 1920x1080 and 3840x2160 on a synthetic
QP32 POC with 4 reference frames, both alignments, in one process:
  (a) vame_seed_pyramid, one frame
  (b) vame_seed_search_wide at (radius, levels) = (32, 1), (64, 2), (128, 2) on
      prebuilt pyramids
  (c) vame_seed_search at radius 16 and 32 and the search of the same POC
      (affine_me_poc, modes 3): the yardsticks
Device events around `--calls` queued calls after `--warmup`.  Before timing:
on the 16x16 aligned CUs of reference 0 the SAD of vame_affine_mc's prediction
plus the rate must equal the returned cost, and two calls must agree.  Also
reports the summed cost of the search's rows after vame_affine_me_seeded from
the wide seeds and from the radius-32 seeds.  Writes JSON (default
profiles/seed_wide_bench.json).

    python profiles/seed_wide_bench.py [--calls 50] [--warmup 5] [--out FILE]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "vvc-affine-gpu_amd"), os.path.join(REPO, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

WIDE = ((32, 1), (64, 2), (128, 2))


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


def check_cost_identity(eng, W, H, cur, refs, lam, out):
    """cost == SAD of vame_affine_mc's prediction + rate on the 16x16 aligned
    CUs of reference 0 (they tile the frame: one prediction call)."""
    import bipred_ref as B
    from vame import seed as V
    cus, rows = V.cus_from_seeds(W, H, 0, out["mv"][(0, 0)], ref=0, skip_zero=False)
    keep = (cus[:, 2] == 16) & (cus[:, 3] == 16)
    cus, rows = cus[keep].contiguous(), rows[keep]
    pred = torch.zeros((H, W), dtype=torch.int16, device=cur.device)
    _, _, bad = eng.affine_mc(cus, refs, pred=pred)
    torch.cuda.synchronize()
    assert int(bad) == 0
    Hc, Wc = H // 16 * 16, W // 16 * 16
    diff = (cur[:Hc, :Wc].to(torch.int64) - pred[:Hc, :Wc].to(torch.int64)).abs()
    sad = diff.reshape(Hc // 16, 16, Wc // 16, 16).sum((1, 3))
    got = sad[(cus[:, 1] // 16).long(), (cus[:, 0] // 16).long()].cpu().numpy()
    mv = cus[:, 6:8].cpu().numpy()
    rate = {}
    for m in {tuple(v) for v in mv.tolist()}:
        rate[m] = B.rate(B.bits_of(2, (m[0], m[1], m[0], m[1], 0, 0)) + 2, lam)
    want = out["cost"][(0, 0)][rows].cpu().numpy()
    assert (got + np.array([rate[tuple(v)] for v in mv.tolist()]) == want).all(), "cost is not affine_mc's SAD + rate"
    return int(len(rows))


def one_resolution(W, H, calls, warmup):
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
    eng.set_max_pairs(nrefs)
    cpyr, rpyr = eng.seed_pyramid(cur), [eng.seed_pyramid(r) for r in refs]
    wide = {k: eng.seed_search_wide(cur, refs, lam, radius=k[0], levels=k[1], cur_pyr=cpyr, ref_pyrs=rpyr) for k in WIDE}
    near = {r: eng.seed_search(cur, refs, lam, radius=r) for r in (16, 32)}
    torch.cuda.synchronize()

    # consistency before timing
    out = {"resolution": [W, H], "nrefs": nrefs, "qp": qp, "lambda": lam, "ctus": eng.n_ctus}
    for k in WIDE:
        again = eng.seed_search_wide(cur, refs, lam, radius=k[0], levels=k[1])  # pyramids built inside
        torch.cuda.synchronize()
        assert all(torch.equal(again[n][key], wide[k][n][key]) for n in ("mv", "cost") for key in again[n]), \
            "vame_seed_search_wide is not deterministic"
        out["cost_identity_rows_checked"] = check_cost_identity(eng, W, H, cur, refs, lam, wide[k])
    out["two_calls_agree"] = True

    # what the seeds are worth to the search
    base = eng.affine_me_poc(cur, refs, lam, modes=3)
    ok = {a: (c < (1 << 62)) for (r, a), c in wide[WIDE[0]]["cost"].items() if r == 0}  # the in-frame rows

    def total(res):
        return sum(int(c[ok[name.startswith("HALF")]].sum()) for (r, name), (c, _) in res.items())

    out["search_cost"] = total(base)
    for tag, seeds in [("radius%d_levels%d" % k, wide[k]) for k in WIDE] + [("exhaustive_radius32", near[32])]:
        res, bad = eng.affine_me_seeded(cur, refs, lam, clone(base), seeds["mv"], modes=3)
        torch.cuda.synchronize()
        assert int(bad) == 0
        out["seeded_cost_" + tag] = total(res)
        out["seed_cost_" + tag] = sum(int(c[ok[a]].sum()) for (r, a), c in seeds["cost"].items())

    sres = eng.alloc_poc(nrefs, 3)
    pyr_out = torch.empty_like(cpyr)
    t = {}
    # the search first and last: the clocks settle over the run
    s0 = timed(lambda: eng.affine_me_poc(cur, refs, lam, modes=3, out=sres), calls, warmup)
    t["seed_pyramid"] = timed(lambda: eng.seed_pyramid(cur, out=pyr_out), calls, warmup)
    for r in (16, 32):
        t[f"seed_search_radius{r}"] = timed(lambda: eng.seed_search(cur, refs, lam, radius=r, out=near[r]), calls, warmup)
    for k in WIDE:
        t["seed_search_wide_radius%d_levels%d" % k] = timed(
            lambda: eng.seed_search_wide(cur, refs, lam, radius=k[0], levels=k[1], cur_pyr=cpyr, ref_pyrs=rpyr,
                                         out=wide[k]), calls, warmup)
    s1 = timed(lambda: eng.affine_me_poc(cur, refs, lam, modes=3, out=sres), calls, warmup)
    ts = min(s0, s1)
    out["search_modes3_ms"] = round(ts, 5)
    out["search_modes3_ms_first_last"] = [round(s0, 5), round(s1, 5)]
    for name, v in t.items():
        out[name + "_ms"] = round(v, 5)
    for k in WIDE:
        name = "seed_search_wide_radius%d_levels%d" % k
        for ys, yv in (("seed_search_radius16", t["seed_search_radius16"]), ("seed_search_radius32", t["seed_search_radius32"]),
                       ("search_modes3", ts)):
            out[f"ratio_{name}_over_{ys}"] = round(t[name] / yv, 5)
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "seed_wide_bench.json"))
    args = ap.parse_args()
    if args.calls < 20:
        ap.error("--calls must be at least 20")
    res = {"device": torch.cuda.get_device_name(0), "calls": args.calls, "warmup": args.warmup,
           "what": "device events around queued calls; seed_search_wide = vame_seed_search_wide on prebuilt pyramids, "
                   "both alignments, 4 refs; seed_pyramid = vame_seed_pyramid of one frame; seed_search = "
                   "vame_seed_search; search = affine_me_poc of the same POC; seeded_cost = the summed cost of the "
                   "search's in-frame rows (4 refs, 4 models) after vame_affine_me_seeded from those seeds",
           "runs": [one_resolution(W, H, args.calls, args.warmup) for W, H in ((1920, 1080), (3840, 2160))]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
