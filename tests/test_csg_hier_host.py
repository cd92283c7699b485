"""Host side of the Csg units' hierarchy (CPU only): tests/cpp/unit_box_check.cpp, a stand-alone
program linking rt_bvh.cpp, holds csg_unit_box to its contract (every root any leaf of a unit
produces on the chained ray lies in the unit's box: seeded random units of 1-4 nested,
transformed Csgs over spheres, cubes and open and closed cylinders scaled up to 1e3, a few
thousand rays a unit, grazing and starting inside), its `false` cases, and build_unit_bvh over 40
units (every unit once, every box inside its parent's, the depth bound)."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "raytracer-challenge-rs_amd", "csrc")


@pytest.fixture(scope="module")
def unit_box_check(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("unit_box")
    exes = []
    for name, flags in (("unit_box_check", ["-O2"]),
                        ("unit_box_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(d / name)
        subprocess.run(["g++", "-std=c++17", "-Wall", "-ffp-contract=off", "-pthread", *flags, "-I", CSRC,
                        os.path.join(REPO, "tests", "cpp", "unit_box_check.cpp"), os.path.join(CSRC, "rt_bvh.cpp"),
                        "-o", exe], check=True)
        exes.append(exe)
    return exes


def test_unit_boxes_and_hierarchy(unit_box_check):
    for exe in unit_box_check:  # the plain build, then the same program under the address and undefined sanitizers
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), r.stdout + r.stderr
