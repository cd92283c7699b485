"""bench.py's plain run, `--full` and `--dump-outputs`.

CPU: the options parse (both off by default), and dump_outputs writes float64
arrays, whole below the size limit and as the same seeded sample of pixels
above it.
GPU: a plain run of a small scene times exactly --steps steps, prints the
headline fields without the parts that `--full` adds, and writes the last timed
frame, which equals a render of the same scene and camera through the library.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")
FULL_ONLY = ("roofline", "parity", "end_to_end", "distinct_cameras", "cold_ms", "cpu_baseline", "per_rank")


def _env():
    return {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}


def test_dump_outputs_whole_and_sampled(tmp_path):
    """In a child process (importing bench.py sets the HIP queue count of its
    process): a small array is written whole; one above its share of the limit
    as `limit // row bytes` rows, the same rows on every call, in ascending
    order, each a row of the input. `--full` and `--dump-outputs` are off
    unless given."""
    code = (
        "import sys, torch, numpy as np\n"
        "import bench\n"
        "g = torch.Generator().manual_seed(7)\n"
        "t = torch.rand((40, 50, 3), dtype=torch.float64, generator=g)\n"
        "t[..., 0] = torch.arange(2000, dtype=torch.float64).reshape(40, 50)\n"
        "bench.dump_outputs(sys.argv[1], {'whole': t})\n"
        "bench.dump_outputs(sys.argv[1], {'a': t, 'b': t.clone()}, limit=2 * 24 * 100)\n"
        "bench.dump_outputs(sys.argv[2], {'a': t}, limit=24 * 100)\n"
        "np.save(sys.argv[1] + '/input.npy', t.numpy())\n"
        "sys.argv[1:] = ['--steps', '5']\n"
        "a = bench.parse()\n"
        "assert a.full is False and a.dump_outputs is None and a.steps == 5\n"
        "sys.argv[1:] = ['--full', '--dump-outputs', 'somewhere']\n"
        "a = bench.parse()\n"
        "assert a.full is True and a.dump_outputs == 'somewhere'\n"
    )
    d1, d2 = tmp_path / "one", tmp_path / "two"
    r = subprocess.run([sys.executable, "-c", code, str(d1), str(d2)], capture_output=True, text=True, env=_env(),
                       timeout=300, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    t = np.load(d1 / "input.npy")
    whole, a, b, a2 = (np.load(p) for p in (d1 / "whole.npy", d1 / "a.npy", d1 / "b.npy", d2 / "a.npy"))
    assert whole.dtype == np.float64 and whole.tobytes() == t.tobytes() and whole.shape == t.shape
    assert a.dtype == np.float64 and a.shape == (100, 3)
    assert a.tobytes() == b.tobytes() == a2.tobytes()
    rows = a[:, 0].astype(int)  # channel 0 holds the pixel's index
    assert (np.diff(rows) > 0).all() and a.tobytes() == t.reshape(-1, 3)[rows].tobytes()


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_frame(tmp_path):
    from rtamd import scenes
    size = ["--width", "96", "--height", "54", "--spheres", "40"]
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "11", "--warmup", "3", "--dump-outputs",
                        str(tmp_path)] + size, capture_output=True, text=True, env=_env(), timeout=300, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["steps"] == 11 and out["warmup"] == 3 and out["full"] is False
    assert out["unit"] == "Mrays/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
    assert out["ms_per_step"] > 0
    # value = the frame's reference rays per timed millisecond (ms_per_step is printed to 1e-4 ms, value to 1e-3)
    assert out["value"] == pytest.approx(out["config"]["rays_per_frame"] / out["ms_per_step"] / 1e3,
                                         rel=5e-5 / out["ms_per_step"] + 1e-6, abs=1e-3)
    assert not [k for k in FULL_ONLY if k in out]
    assert sorted(os.listdir(tmp_path)) == ["canvas.npy"]
    canvas = np.load(tmp_path / "canvas.npy")
    assert canvas.dtype == np.float64 and canvas.shape == (54, 96, 3)
    w, cam, depth = scenes.c3(96, 54, 40)
    ref, st = cam.render(w, depth)  # the exhaustive frame
    assert canvas.tobytes() == ref.to_numpy().tobytes()
    assert out["config"]["rays_per_frame"] == sum(st[k] for k in ("rays_primary", "rays_reflect", "rays_refract",
                                                                  "rays_shadow"))
