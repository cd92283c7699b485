"""The stream form of the Csg filter (rt_csg.hpp: csg_batch_insert, csg_stream_pass, CsgNegTable),
CPU only: tests/cpp/csg_stream_check.cpp, a stand-alone program built under the address and
undefined-behaviour sanitizers, drives the functions the wide units' evaluator runs per ray against
a literally nested restatement (stable sort, filter per node bottom up, a literal fold)."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "raytracer-challenge-rs_amd", "csrc")


@pytest.fixture(scope="module")
def stream_check(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("csg_stream") / "csg_stream_check_san")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(REPO, "tests", "cpp", "csg_stream_check.cpp"), "-o", exe], check=True)
    return exe


def test_stream_equals_nested(stream_check):
    r = subprocess.run([stream_check], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
    fields = dict(f.split("=") for f in r.stdout.split()[1:])
    # at least a fifth of the cases needed more than one batch at the kernels' capacity
    assert int(fields["multi_batch"]) * 5 >= int(fields["cases"]) >= 1000
