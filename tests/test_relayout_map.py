"""The hand-over's lane mapping (relayout_lane, vame_items.h) checked on the
host: tests/native/relayout_check.cpp, a stand-alone program built with the
host-only template unit under AddressSanitizer and UBSan, run directly."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_relayout_lane_mapping(tmp_path):
    """Every two-sub-block task of the product templates, every subset of live
    CUs that meets the hand-over's condition: each live sub-block on exactly
    one lane, aligned 32- / 64-lane segments, neighbour lanes inside the
    wave's rows (the program's header lists the checks)."""
    exe = str(tmp_path / "relayout_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-o", exe,
                        os.path.join(REPO, "tests", "native", "relayout_check.cpp"),
                        os.path.join(REPO, "vvc-affine-gpu_amd", "csrc", "vame_templates.cpp")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "relayout_check ok" in r.stdout, (r.stdout + r.stderr)[-2000:]
