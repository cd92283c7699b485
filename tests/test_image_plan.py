"""Host-side check of the fast path's image plan (rt_wf_plan.hpp:
wf_plan_image, lane_lds_layout), compiled with g++ from the library's own
header against the HIP headers and run without a device: over a sweep of
synthetic scenes and knob settings the plan equals the rules launch_fused_q
stated inline before, the dynamic LDS it asks for is the layout's end and fits
the limit with the kernel's static LDS, the layout's regions are aligned,
ordered and hold what each image's stage (LaneImage, which takes its offsets
from the layout) writes into them, and the sweep reaches every image, flag and
treelet outcome."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "raytracer-challenge-rs_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    if not os.path.isfile(os.path.join(ROCM, "include", "hip", "hip_runtime.h")):
        pytest.skip("no HIP headers")
    exe = str(tmp_path_factory.mktemp("plan") / "plan_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(ROCM, "include"), "-I", CSRC,
                    os.path.join(REPO, "tests", "cpp", "plan_check.cpp"), "-o", exe], check=True)
    return exe


def test_image_plan(plan_check):
    r = subprocess.run([plan_check], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
