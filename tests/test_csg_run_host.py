"""Host side of the run hierarchies inside wide and deep Csg units (CPU only): tests/cpp/csg_run_check.cpp,
a stand-alone program linking rt_bvh.cpp, holds tri_box with a run's bounds, csg_run_bounds and
build_csg_run to their contract, and the walk the evaluators make (rt_slab.hpp csg_run_admits /
csg_run_walk with rt_csg.hpp csg_batch_insert, the functions the device compiles) to the one-by-one
loop over the run's triangles: seeded runs of 16-400 triangles (axis-aligned flat ones, rays at
|det| of 1-4 EPSILON, edges 1e-3 .. 1e2) under chains of 0-4 rounded Csg inverses, and up to 12,
with uneven scales 1e-2 .. 1e2, rotations, shears and translations; a few thousand rays a run
(grazing, in a triangle's plane, zero direction components, from inside, from origins up to the
bound, just inside and outside the bounds). Every root above the watermark and at or below t_hi is
reached; the batch and `more` equal the loop's up to t_hi; a line that misses the root's box tests
no boxed triangle; the tree's structure. The program prints the mean leaf tests a walk beside each
run's size."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "raytracer-challenge-rs_amd", "csrc")


@pytest.fixture(scope="module")
def csg_run_check(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("csg_run")
    exes = []
    for name, flags in (("csg_run_check", ["-O2"]),
                        ("csg_run_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(d / name)
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-pthread", *flags, "-I", CSRC,
                        os.path.join(REPO, "tests", "cpp", "csg_run_check.cpp"), os.path.join(CSRC, "rt_bvh.cpp"),
                        "-o", exe], check=True)
        exes.append(exe)
    return exes


def test_run_hierarchies_and_their_walk(csg_run_check):
    for exe in csg_run_check:  # the plain build, then the same program under the address and undefined sanitizers
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), r.stdout[-4000:] + r.stderr[-4000:]
        assert "mean leaf tests per walk" in r.stdout
