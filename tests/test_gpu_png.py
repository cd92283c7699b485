"""The PNG writer on the device (image/png.rs:13-31; rt_canvas_to_png_device) and the
one-call render-to-PNG entry point (rt_render_png: camera.rs:133-148, canvas.rs:50-52).

The device encoder must write exactly the file png_ref.py builds by hand from
the format (and so the host encoder's bytes), and PIL must read the quantised
canvas back from it. Sizes: test_png.py's (stored-block boundaries, rows that
straddle blocks, the Adler worst case), the encoder's own segment boundaries,
and a 1920x1080 frame.
"""
import os
import subprocess

import numpy as np
import pytest

import png_ref

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "raytracer-challenge-rs_amd")
SCENES = os.path.join(REPO, "tests", "golden", "scenes")

# rt_png_dev.hpp's kPngSegment: the raw bytes (filter bytes and components) one block encodes
SEGMENT = 9211
# (H, W) with H * (3 W + 1) raw bytes = SEGMENT - 1, SEGMENT, SEGMENT + 1, 2 * SEGMENT
SEGMENT_SIZES = [(921, 3), (1, 3070), (2303, 1), (2, 3070)]
assert [h * (3 * w + 1) for h, w in SEGMENT_SIZES] == [SEGMENT - 1, SEGMENT, SEGMENT + 1, 2 * SEGMENT]


def _device_png(rt, canvas):
    import torch
    h, w = canvas.shape[0], canvas.shape[1]
    d = torch.from_numpy(np.ascontiguousarray(canvas, dtype=np.float64)).cuda()
    n = rt._rtamd.canvas_to_png_device(d.data_ptr(), w, h, 0, 0, 0)  # length query
    assert n == rt._rtamd.png_size(w, h) == png_ref.predicted_size(w, h)
    out = torch.full((n + 16,), 0xEE, dtype=torch.uint8, device="cuda")
    assert rt._rtamd.canvas_to_png_device(d.data_ptr(), w, h, out.data_ptr(), n,
                                          torch.cuda.current_stream().cuda_stream) == n
    got = out.cpu().numpy()
    assert (got[n:] == 0xEE).all(), "bytes written past the file"
    return got[:n].tobytes()


def _check(rt, oracle, canvas):
    got = _device_png(rt, canvas)
    png_ref.check_file(got, png_ref.quantised(oracle, canvas))
    assert got == rt.canvas_to_png(canvas)


@pytest.mark.parametrize("width", range(1, 41))
def test_device_png_edge_values(rt, oracle, width):
    _check(rt, oracle, png_ref.edge_canvas(3, width))


@pytest.mark.parametrize("name", [n for n, _, _ in png_ref.SIZES])
def test_device_png_block_boundaries_and_frames(rt, oracle, name):
    _check(rt, oracle, png_ref.sized_canvas(name))


@pytest.mark.parametrize("h,w", SEGMENT_SIZES)
def test_device_png_segment_boundaries(rt, oracle, h, w):
    _check(rt, oracle, png_ref.edge_canvas(h, w))


def test_device_png_1920x1080(rt, oracle):
    _check(rt, oracle, np.random.default_rng(1920).uniform(-0.1, 1.1, size=(1080, 1920, 3)))


def test_device_png_unaligned_output(rt, oracle):
    """The file at every byte alignment of the output pointer (the encoder writes aligned words)."""
    import torch
    canvas = png_ref.edge_canvas(5, 37)
    want = png_ref.expected_png(png_ref.quantised(oracle, canvas))
    d = torch.from_numpy(canvas).cuda()
    for shift in range(1, 4):
        out = torch.full((len(want) + 8,), 0xEE, dtype=torch.uint8, device="cuda")
        rt._rtamd.canvas_to_png_device(d.data_ptr(), 37, 5, out.data_ptr() + shift, len(want), 0)
        got = out.cpu().numpy()
        assert got[shift:shift + len(want)].tobytes() == want
        assert (got[:shift] == 0xEE).all() and (got[shift + len(want):] == 0xEE).all()


def test_device_png_short_buffer_and_refused_sizes(rt):
    import torch
    canvas = torch.full((4, 5, 3), 0.5, dtype=torch.float64, device="cuda")
    n = rt._rtamd.canvas_to_png_device(canvas.data_ptr(), 5, 4, 0, 0, 0)
    out = torch.zeros(n, dtype=torch.uint8, device="cuda")
    with pytest.raises(rt.RtError, match="too small"):
        rt._rtamd.canvas_to_png_device(canvas.data_ptr(), 5, 4, out.data_ptr(), n - 1, 0)
    assert not out.any().item()  # (nothing was written)
    assert rt._rtamd.canvas_to_png_device(canvas.data_ptr(), 5, 4, out.data_ptr(), n, 0) == n
    assert out.cpu().numpy().tobytes() == rt.canvas_to_png(canvas.cpu().numpy())
    for w, h, says in [(0, 4, "width"), (4, 0, "height"), (46341, 46341, "2.31"), (26754, 26754, "2.31")]:
        with pytest.raises(rt.RtError, match=says):
            rt._rtamd.canvas_to_png_device(canvas.data_ptr(), w, h, out.data_ptr(), n, 0)
        with pytest.raises(rt.RtError, match=says):
            rt._rtamd.canvas_to_png_device(canvas.data_ptr(), w, h, 0, 0, 0)


def test_render_png_slice_decodes_to_the_oracle_frame(rt, oracle):
    from rtamd import scenes
    w, cam, depth = scenes.c3(96, 54)
    png, st = cam.render_png(w, depth, want_stats=True)
    ref, rst = oracle.OracleWorld.from_world(w).render(cam.desc_bytes(), depth, nthreads=8)
    png_ref.check_file(png, png_ref.quantised(oracle, ref))
    for k in ("rays_primary", "rays_reflect", "rays_refract", "rays_shadow"):
        assert st[k] == rst[k], k


def test_render_png_c3_buffers_aa_and_overflow(rt):
    """rt_render_png on C3's full frame equals canvas_to_png of the rendered canvas: through the
    binding, with AA X2, into a reused pinned block and a reused pageable buffer, and after a
    forced arena overflow (the frame is rendered again before it is encoded); a buffer one
    byte short is refused."""
    from rtamd import scenes
    w, cam, depth = scenes.c3()
    canvas, _ = cam.render(w, depth, want_stats=False)
    whole = rt.canvas_to_png(canvas.to_numpy())
    png, _ = cam.render_png(w, depth)
    assert png == whole
    cam.render_opts.aa_samples(rt.AASamples.X2)
    canvas2, _ = cam.render_multithreaded(w, depth, want_stats=False)
    png2, _ = cam.render_png(w, depth, 2)
    assert png2 == rt.canvas_to_png(canvas2.to_numpy())
    pinned = rt._rtamd.host_buffer(len(whole) + 4096)
    pageable = np.zeros(len(whole) + 4096, dtype=np.uint8)
    for buf in (pinned, pageable, pinned):
        n = cam.render_png_into(w, buf, depth)
        assert n == len(whole) and buf[:n].tobytes() == whole
    w.tune("arena_pct", 5)
    try:
        over, _ = cam.render_png(w, depth)
    finally:
        w.tune("arena_pct", 100)
    assert over == whole
    short = np.zeros(len(whole) - 1, dtype=np.uint8)
    with pytest.raises(rt.RtError, match="too small"):
        cam.render_png_into(w, short, depth)
    w.check()


def _small_scene(tmp_path):
    text = open(os.path.join(SCENES, "reflect-refract.yml")).read().replace("width: 2560", "width: 96") \
        .replace("height: 1440", "height: 54")
    src = tmp_path / "scene.yml"
    src.write_text(text)
    return text, src


def test_scene_parser_and_cli_write_png_by_extension(rt, oracle, tmp_path):
    text, src = _small_scene(tmp_path)
    p = rt.SceneParser()
    p.load_str(text)
    ref, _ = oracle.OracleWorld.from_world(p.build_world()).render(p.camera.desc_bytes(), 5, nthreads=16)
    px = png_ref.quantised(oracle, ref)
    out = tmp_path / "x.PNG"
    p.render_to(str(out))
    png_ref.check_file(out.read_bytes(), px)
    exe = os.path.join(PKG, "bin", "render_scene")
    cli = tmp_path / "cli.png"
    r = subprocess.run([exe, str(src), str(cli)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    png_ref.check_file(cli.read_bytes(), px)
    ppm = tmp_path / "x.ppm"
    p.render_to(str(ppm))
    want = oracle.canvas_to_ppm(ref)
    assert ppm.read_bytes() == (want.encode() if isinstance(want, str) else bytes(want))
