"""rt_render_png_deflate against rt_render_png at the same build, in one process (dev probe):
the full-size C3 frame, warm, into the same reused pinned buffer, the two calls alternating
(as png_probe.py); then the two device encoders alone on the resident frame and each kernel
of the compressed one, by stream events; the bytes copied; the file's size against the
stored file and against zlib level 6 and Z_RLE over the same filtered bytes. Minimum and
median of --calls calls each. Writes the figures, the build id and the command as text.
Usage: png_deflate_probe.py [--calls K] [--out FILE]"""
import argparse
import os
import statistics
import struct
import sys
import time
import zlib

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
    sys.exit("png_deflate_probe: no GPU")
w, cam, depth = scenes.c3()
w.upload(0)
W, H = cam.hsize, cam.vsize
lines = [f"command: python tools/png_deflate_probe.py --calls {a.calls}", f"build id: {buildinfo.build_id()}",
         f"device: {torch.cuda.get_device_name(0)}", f"frame: C3 {W}x{H}, depth {depth}, min / median of {a.calls} calls, ms", ""]


def say(s):
    lines.append(s)
    print(s, flush=True)


def row(name, ts, note=""):
    say(f"{name:38s} {min(ts):8.3f} {statistics.median(ts):8.3f}  {note}")


cap = max(rtamd.png_deflate_bound(W, H), rtamd.png_size(W, H))
pinned = rtamd._rtamd.host_buffer(cap)
calls = {"render_png_into (pinned)": lambda: cam.render_png_into(w, pinned, depth),
         "render_png_deflate_into (pinned)": lambda: cam.render_png_deflate_into(w, pinned, depth)}
times = {k: [] for k in calls}
size = {}
for _ in range(5):
    for k, fn in calls.items():
        size[k] = fn()
png = pinned[:size["render_png_deflate_into (pinned)"]].tobytes()
for _ in range(a.calls):  # alternating: both see the same neighbours on a shared host
    for k, fn in calls.items():
        t0 = time.perf_counter()
        fn()
        times[k].append((time.perf_counter() - t0) * 1e3)
say(f"{'end to end, host clock':38s} {'min':>8s} {'median':>8s}")
for k in calls:
    row(k, times[k], f"{size[k]} bytes to the host")

# the encoders alone: a resident canvas (the frame itself), events around each call
canvas = torch.empty((H, W, 3), dtype=torch.float64, device="cuda")
stream = torch.cuda.current_stream().cuda_stream
cam.render_shard_device(w, depth, 8, 0, 1, canvas.data_ptr(), stream, False)
torch.cuda.synchronize()
d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
enc = {"canvas_to_png_device": lambda: rtamd._rtamd.canvas_to_png_device(canvas.data_ptr(), W, H, d_out.data_ptr(), cap, stream),
       "canvas_to_png_deflate_device": lambda: rtamd._rtamd.canvas_to_png_deflate_device(canvas.data_ptr(), W, H, d_out.data_ptr(), cap, stream)}
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
say(f"{'encoder alone, stream events':38s} {'min':>8s} {'median':>8s}")
for k in enc:
    row(k, ev[k], f"{size[k]} bytes, reads {H * W * 24} bytes of canvas (with the call's allocation and wait)")
assert d_out[:size["canvas_to_png_deflate_device"]].cpu().numpy().tobytes() == png

kern = [[], [], [], []]
for _ in range(a.calls):
    for k, ms in enumerate(rtamd._rtamd._pngz_kernel_times(canvas.data_ptr(), W, H, d_out.data_ptr(), cap, stream)):
        kern[k].append(ms)
say("")
say(f"{'kernels, stream events':38s} {'min':>8s} {'median':>8s}")
segs = -(-H // max(1, 16384 // (3 * W + 1)))
for name, ts in zip(("pngz_encode", "pngz_scan", "pngz_pack", "pngz_finish"), kern):
    row(name, ts, f"{segs} blocks" if name in ("pngz_encode", "pngz_pack") else "1 block")

host = torch.from_numpy(pinned)
say("")
say(f"{'copies, stream events':38s} {'min':>8s} {'median':>8s}")
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

# sizes: the IDAT's filtered bytes through zlib
n_idat, = struct.unpack(">I", png[33:37])
F = zlib.decompress(png[41:41 + n_idat])
assert len(F) == H * (3 * W + 1)
rle = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
say("")
say(f"file sizes, bytes: stored {rtamd.png_size(W, H)}, compressed {len(png)} "
    f"({len(png) / rtamd.png_size(W, H):.3f} of stored), bound {rtamd.png_deflate_bound(W, H)}")
say(f"IDAT payload {n_idat}; zlib over the same filtered bytes: Z_RLE {len(rle.compress(F) + rle.flush())}, "
    f"level 6 {len(zlib.compress(F, 6))}")
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
