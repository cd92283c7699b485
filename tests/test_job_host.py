"""Host-side check of the render job's rules (rt_wavefront.hpp: WfJob,
wf_job_valid), compiled with g++ from the library's own header against the
HIP headers and run without a device: which jobs Wavefront::render accepts
(sample counts, ray batches, recursion depth, block patterns, frame batches),
that they are the rules its positional checks stated, and the size of the
kernels' argument block (WfArgs)."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "raytracer-challenge-rs_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


@pytest.fixture(scope="module")
def job_check(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    if not os.path.isfile(os.path.join(ROCM, "include", "hip", "hip_runtime.h")):
        pytest.skip("no HIP headers")
    exe = str(tmp_path_factory.mktemp("job") / "job_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall","-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(ROCM, "include"), "-I", CSRC,
                    os.path.join(REPO, "tests", "cpp", "job_check.cpp"), "-o", exe], check=True)
    return exe


def test_job_rules(job_check):
    r = subprocess.run([job_check], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
