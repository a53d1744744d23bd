"""What the pyramid search loses against an exhaustive search of the same range
(DESIGN.md section 16), on the CPU references alone: the (-43, +26) shifted
camera at 416x240, the in-frame aligned rows.  About a minute of numpy; run
once, the result goes to profiles/seed_wide_exhaustive.json.

    python profiles/seed_wide_exhaustive.py
"""
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "tests"), os.path.join(REPO, "vvc-affine-gpu_amd")]

import seed_ref as S  # noqa: E402
import seedpyr_ref as P  # noqa: E402

W, H = 416, 240


def main():
    refs, cur = P.shifted_camera_wide((-43, 26))
    s = P.Searcher(refs[0], cur)
    inn = s.inn[0]
    rows = [c[0] for c in inn]
    boxes = np.array([c[1:] for c in inn], np.int64)
    maps = P.top_sads(refs[0], cur, boxes, 64)  # [row, dy + 64, dx + 64]
    out = {"input": "416x240, seed 0xBEEF, ref = QP-32 reconstruction of POC 0, cur = POC 2 through a window moved by "
                    "(-43, +26), lambda = %r, %d in-frame aligned rows" % (S.LAM, len(rows)), "sums": {}}
    exh = {}
    for radius in (0, 32, 64):
        got = [S.seed_from_map(maps[k], c[1], c[2], c[3], c[4], W, H, radius, S.LAM) for k, c in enumerate(inn)]
        exh[radius] = got
        out["sums"]["exhaustive_radius%d" % radius] = sum(v for _, v in got)
    for radius, levels in ((64, 2), (64, 1), (128, 2)):
        mv, cost, _ = s.run(S.LAM, radius, levels, 0)
        out["sums"]["pyramid_radius%d_levels%d" % (radius, levels)] = int(cost[rows].sum())
        if radius == 64:
            out["rows_equal_exhaustive64_levels%d" % levels] = sum(
                (tuple(mv[r].tolist()), int(cost[r])) == exh[64][k] for k, r in enumerate(rows))
    path = os.path.join(REPO, "profiles", "seed_wide_exhaustive.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
