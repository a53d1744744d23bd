#!/usr/bin/env python3
"""Host cost of a descriptor-list call through vame.engine.Engine: on a 416x240
engine, 1000 back-to-back affine_search / bipred_refine calls on 8 descriptors
and one synchronise, five repetitions after 50 warm-up calls.  Prints per
repetition the microseconds per call with the synchronise, and of issuing the
calls alone (the Python body, ctypes and the launch).  To compare two trees'
Python layers over one library, give the other tree and set VAME_LIB.

    python profiles/engine_call_cost.py [TREE] [LABEL]
"""
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
root = sys.argv[1] if len(sys.argv) > 1 else REPO
label = sys.argv[2] if len(sys.argv) > 2 else "here"
sys.path.insert(0, os.path.join(root, "vvc-affine-gpu_amd"))

import torch  # noqa: E402

from vame import mc as M  # noqa: E402
from vame.engine import Engine  # noqa: E402

W, H, LAM, N = 416, 240, 57.0, 1000
dev = torch.device("cuda", 0)
eng = Engine(W, H, 0)
g = torch.Generator().manual_seed(1)
cur = torch.randint(0, 1024, (H, W), generator=g, dtype=torch.int16).to(dev)
refs = [torch.randint(0, 1024, (H, W), generator=g, dtype=torch.int16).to(dev)]
cpmv = torch.zeros((eng.n_cus(0), 7), dtype=torch.int32, device=dev)
cus = M.cus_from_result(W, H, 0, 2, cpmv, ref=0)[0][:8].contiguous()
bi = torch.zeros((8, 20), dtype=torch.int32, device=dev)  # both hypotheses on reference 0, 2-CP
bi[:, :12] = cus
bi[:, 13] = 2
for name, fn, d in (("affine_search", eng.affine_search, cus), ("bipred_refine", eng.bipred_refine, bi)):
    for _ in range(50):
        out = fn(d, refs, cur, LAM)
    torch.cuda.synchronize()
    assert int(out[2]) == 0, (name, "invalid descriptor")
    reps = []
    for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(N):
            fn(d, refs, cur, LAM)
        t_issue = time.perf_counter() - t0
        torch.cuda.synchronize()
        reps.append(((time.perf_counter() - t0) / N * 1e6, t_issue / N * 1e6))
    print(f"percall {label} {name} us_per_call(with sync) " + " ".join(f"{a:.2f}" for a, _ in reps)
          + "  issue-only " + " ".join(f"{b:.2f}" for _, b in reps), flush=True)
eng.close()
