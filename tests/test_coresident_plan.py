"""Host-side check of the co-resident launch shape's plan (rt_wf_plan.hpp: wf_plan_image's
`coresident` argument, coresident_lds_fits), compiled with g++ from the library's own header
and run without a device: for C3-sized scenes whose four-wide LDS image runs up to the limit
the plan picks blocks of 960 threads (form 1) or the capped kernels (form 2) exactly when the
CU's LDS still holds the combine's blocks beside the fused block, and 1024 threads otherwise;
the image and lane_lds_layout are the same for every form."""
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
    exe = str(tmp_path_factory.mktemp("coplan") / "coresident_plan_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(ROCM, "include"), "-I", CSRC,
                    os.path.join(REPO, "tests", "cpp", "coresident_plan_check.cpp"), "-o", exe], check=True)
    return exe


def test_coresident_plan(plan_check):
    r = subprocess.run([plan_check], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
