"""rt_render_png against rt_render_ppm at the same build, in one process (dev probe): the
full-size C3 frame, warm, into the same reused pinned buffer, the two calls alternating;
then the two device encoders alone on a resident canvas, by stream events. Minimum and
median of --calls calls each. Writes the figures, the build id and the command as text.
Usage: png_probe.py [--calls K] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "raytracer-challenge-rs_amd")]
import torch  # noqa: E402

import rtamd  # noqa: E402
from rtamd import buildinfo, scenes  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=60)
ap.add_argument("--out", default=None)
a = ap.parse_args()
assert a.calls >= 30
if rtamd.device_count() < 1:
    sys.exit("png_probe: no GPU")
w, cam, depth = scenes.c3()
w.upload(0)
W, H = cam.hsize, cam.vsize
lines = [f"command: python tools/png_probe.py --calls {a.calls}", f"build id: {buildinfo.build_id()}",
         f"device: {torch.cuda.get_device_name(0)}", f"frame: C3 {W}x{H}, depth {depth}, min / median of {a.calls} calls, ms", ""]


def say(s):
    lines.append(s)
    print(s, flush=True)


def row(name, ts, note=""):
    say(f"{name:34s} {min(ts):8.3f} {statistics.median(ts):8.3f}  {note}")


ppm_cap = 32 + 12 * W * H + H
pinned = rtamd._rtamd.host_buffer(ppm_cap)
calls = {"render_ppm_into (pinned)": lambda: cam.render_ppm_into(w, pinned, depth),
         "render_png_into (pinned)": lambda: cam.render_png_into(w, pinned, depth)}
times = {k: [] for k in calls}
size = {}
for _ in range(5):
    for k, fn in calls.items():
        size[k] = fn()
for _ in range(a.calls):  # alternating: both see the same neighbours on a shared host
    for k, fn in calls.items():
        t0 = time.perf_counter()
        fn()
        times[k].append((time.perf_counter() - t0) * 1e3)
say(f"{'end to end, host clock':34s} {'min':>8s} {'median':>8s}")
for k in calls:
    row(k, times[k], f"{size[k]} bytes to the host")

# the encoders alone: a resident canvas (the frame itself), events around each call's kernels
canvas = torch.empty((H, W, 3), dtype=torch.float64, device="cuda")
stream = torch.cuda.current_stream().cuda_stream
cam.render_shard_device(w, depth, 8, 0, 1, canvas.data_ptr(), stream, False)
torch.cuda.synchronize()
d_out = torch.empty(ppm_cap, dtype=torch.uint8, device="cuda")
enc = {"canvas_to_ppm_device": lambda: rtamd._rtamd.canvas_to_ppm_device(canvas.data_ptr(), W, H, d_out.data_ptr(), ppm_cap, stream),
       "canvas_to_png_device": lambda: rtamd._rtamd.canvas_to_png_device(canvas.data_ptr(), W, H, d_out.data_ptr(), ppm_cap, stream)}
ev = {k: [] for k in enc}
for _ in range(5):
    for fn in enc.values():
        fn()
for _ in range(a.calls):
    for k, fn in enc.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        n = fn()
        e1.record()
        e1.synchronize()
        ev[k].append(e0.elapsed_time(e1))
        size[k] = n
say("")
say(f"{'encoder alone, stream events':34s} {'min':>8s} {'median':>8s}")
for k in enc:
    row(k, ev[k], f"{size[k]} bytes, reads {H * W * 24} bytes of canvas")

# the frame alone and the copies alone, to say where an end-to-end call's time goes
dev = []
for _ in range(a.calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    cam.render_shard_device(w, depth, 8, 0, 1, canvas.data_ptr(), stream, False)
    e1.record()
    e1.synchronize()
    dev.append(e0.elapsed_time(e1))
say("")
say(f"{'parts, stream events':34s} {'min':>8s} {'median':>8s}")
row("device frame (no encoder, no copy)", dev)
host = torch.from_numpy(pinned)
for k in enc:
    ts = []
    for _ in range(a.calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        host[:size[k]].copy_(d_out[:size[k]], non_blocking=True)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    row(f"copy of {size[k]} bytes to pinned", ts)
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
