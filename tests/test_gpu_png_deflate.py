"""The compressed PNG writer on the device (rt_canvas_to_png_deflate_device) and the one-call
render-to-compressed-PNG entry point (rt_render_png_deflate).

The format is one fixed file per canvas, so the device encoder must write the host
encoder's bytes (themselves held to png_deflate_ref.py's checker by test_png_deflate.py):
on the format's edges (png_deflate_ref.edge_canvases: codes cut at 15 and 7 bits, 513 segments,
the widest row, the tie between the two block forms, ...), over a sweep of widths, on a 640x360
frame of noise, and on golden canvases; without touching a byte past the file. A camera wider
than the device encoder's row is refused before it is rendered. The render call must equal the
host encoder applied to the rendered canvas and decode to the oracle's quantised frame;
render_png and `render_scene <scene> <out>` still give the stored file, and `--compress` the
compressed one (4000 segments: a file zlib inflates, with chunk CRCs that hold).
"""
import ctypes
import math
import os
import subprocess
import zlib

import numpy as np
import pytest

import png_deflate_ref as ref
import png_ref

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "raytracer-challenge-rs_amd")
GOLDEN = os.path.join(REPO, "tests", "golden")
SCENES = os.path.join(GOLDEN, "scenes")
POISON = 0xEE


def _device_png(rt, canvas, shift=0):
    """The device encoder's file, from a poisoned buffer of the bound (at byte offset `shift`)."""
    import torch
    h, w = canvas.shape[0], canvas.shape[1]
    d = torch.from_numpy(np.ascontiguousarray(canvas, dtype=np.float64)).cuda()
    bound = rt._rtamd.canvas_to_png_deflate_device(d.data_ptr(), w, h, 0, 0, 0)  # d_out NULL: the bound
    assert bound == rt._rtamd.png_deflate_bound(w, h) == ref.bound(w, h)
    out = torch.full((bound + 16,), POISON, dtype=torch.uint8, device="cuda")
    n = rt._rtamd.canvas_to_png_deflate_device(d.data_ptr(), w, h, out.data_ptr() + shift, bound,
                                               torch.cuda.current_stream().cuda_stream)
    got = out.cpu().numpy()
    assert n <= bound
    assert (got[:shift] == POISON).all() and (got[shift + n:] == POISON).all(), "bytes written outside the file"
    return got[shift:shift + n].tobytes()


def _check(rt, canvas):
    want = rt.canvas_to_png_deflate(canvas)
    got = _device_png(rt, canvas)
    assert len(got) == len(want)
    if got != want:
        bad = np.flatnonzero(np.frombuffer(got, np.uint8) != np.frombuffer(want, np.uint8))
        raise AssertionError(f"{bad.size} bytes differ, the first at offset {bad[0]} of {len(want)}")


@pytest.mark.parametrize("name", ref.EDGE_NAMES)
def test_device_equals_host_on_format_edges(rt, name):
    _check(rt, ref.edge_canvases()[name])


@pytest.mark.parametrize("w", ref.sweep_widths())
def test_device_equals_host_over_widths(rt, w):
    """Five rows of every width of the sweep (1..48, rows that cross 256, 512 and 1024 bytes, a width
    for every number of bytes a thread can own): where rows and runs fall in the threads' chunks and
    which threads own nothing follows from the width. test_png_deflate.py holds the host's files of
    the same canvases to the block checker and counts their block forms and matches."""
    _check(rt, ref.sweep_canvas(w))


def test_device_equals_host_on_a_frame(rt):
    _check(rt, png_ref.sized_canvas("frame_640x360"))


@pytest.mark.parametrize("name", ["c1", "first_scene_96x54", "yaml_reflect_refract_128x72"])
def test_device_equals_host_on_golden_canvases(rt, oracle, name):
    canvas = np.load(os.path.join(GOLDEN, name + ".npz"))["canvas"]
    _check(rt, canvas)
    ref.check_file(_device_png(rt, canvas), png_ref.quantised(oracle, canvas), size_against_rle=True)


def test_device_unaligned_output(rt):
    """Segments land at byte offsets that follow from the pixels; the output pointer may be unaligned too."""
    canvas = ref.edge_canvases()["rows_plus_1"]
    want = rt.canvas_to_png_deflate(canvas)
    for shift in range(1, 4):
        assert _device_png(rt, canvas, shift) == want


def test_device_buffer_conventions_and_refused_sizes(rt):
    import torch
    canvas = np.load(os.path.join(GOLDEN, "first_scene_96x54.npz"))["canvas"]
    h, w = canvas.shape[0], canvas.shape[1]
    want = rt.canvas_to_png_deflate(canvas)
    d = torch.from_numpy(canvas).cuda()
    out = torch.zeros(len(want), dtype=torch.uint8, device="cuda")
    with pytest.raises(rt.RtError, match="too small"):
        rt._rtamd.canvas_to_png_deflate_device(d.data_ptr(), w, h, out.data_ptr(), len(want) - 1, 0)
    assert not out.any().item()  # (nothing was written)
    # a cap below the bound succeeds when the file fits
    assert rt._rtamd.canvas_to_png_deflate_device(d.data_ptr(), w, h, out.data_ptr(), len(want), 0) == len(want)
    assert out.cpu().numpy().tobytes() == want
    for bw, bh, says in [(0, 4, "width"), (4, 0, "height"), (46341, 46341, "2.31"), (26754, 26754, "2.31")]:
        with pytest.raises(rt.RtError, match=says):
            rt._rtamd.canvas_to_png_deflate_device(d.data_ptr(), bw, bh, out.data_ptr(), len(want), 0)
        with pytest.raises(rt.RtError, match=says):
            rt._rtamd.canvas_to_png_deflate_device(d.data_ptr(), bw, bh, 0, 0, 0)
    with pytest.raises(rt.RtError, match="wider"):  # a row beyond the workgroup's LDS: the host encoder takes it
        rt._rtamd.canvas_to_png_deflate_device(d.data_ptr(), 8534, 1, out.data_ptr(), len(want), 0)


def test_render_png_deflate_refuses_a_wider_row(rt):
    """A camera one pixel wider than the device encoder's row: the size query still answers with the
    bound, the render call is refused before anything is rendered or written."""
    from rtamd import scenes
    w, cam, depth = scenes.first_scene(16, 9)
    cam.render(w, depth, want_stats=False)  # (the scene is on the device from here on)
    wide = rt.Camera(ref.DEVICE_MAX_WIDTH + 1, 1, math.pi / 3)
    lib = ctypes.CDLL(rt.LIB_PATH)
    lib.rt_render_png_deflate.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32,
                                          ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t),
                                          ctypes.c_void_p]
    lib.rt_last_error.restype = ctypes.c_char_p
    bound, n = ref.bound(ref.DEVICE_MAX_WIDTH + 1, 1), ctypes.c_size_t(0)
    assert lib.rt_render_png_deflate(w._scene_handle(), wide.desc_bytes(), depth, 1, None, 0, ctypes.byref(n), None) == 0
    assert n.value == bound == rt._rtamd.png_deflate_bound(ref.DEVICE_MAX_WIDTH + 1, 1)
    out = ctypes.create_string_buffer(bytes([POISON]) * bound, bound)
    stats = ctypes.create_string_buffer(bytes([POISON]) * 256, 256)  # (rt_stats is smaller)
    assert lib.rt_render_png_deflate(w._scene_handle(), wide.desc_bytes(), depth, 1, out, bound, ctypes.byref(n),
                                     stats) == -1  # RT_ERR_INVALID_ARGUMENT
    assert "wider" in lib.rt_last_error().decode()
    assert out.raw == bytes([POISON]) * bound and stats.raw == bytes([POISON]) * 256
    with pytest.raises(rt.RtError, match="wider"):
        wide.render_png_deflate(w, depth)
    # the widest camera it takes
    widest = rt.Camera(ref.DEVICE_MAX_WIDTH, 1, math.pi / 3)
    png, _ = widest.render_png_deflate(w, depth)
    canvas, _ = widest.render(w, depth, want_stats=False)
    assert png == rt.canvas_to_png_deflate(canvas.to_numpy())
    w.check()


def _cover_80x80(tmp_path):
    text = open(os.path.join(SCENES, "cover.yml")).read().replace("width: 4000", "width: 80") \
        .replace("height: 4000", "height: 80")
    src = tmp_path / "cover80.yml"
    src.write_text(text)
    return text, src


def _render_checks(rt, oracle, w, cam, depth):
    canvas, _ = cam.render(w, depth, want_stats=False)
    want = rt.canvas_to_png_deflate(canvas.to_numpy())
    png, st = cam.render_png_deflate(w, depth, want_stats=True)
    assert png == want
    ref_canvas, rst = oracle.OracleWorld.from_world(w).render(cam.desc_bytes(), depth, nthreads=16)
    px = png_ref.quantised(oracle, ref_canvas)
    ref.check_file(png, px)
    stored, pst = cam.render_png(w, depth, want_stats=True)
    for k in ("rays_primary", "rays_reflect", "rays_refract", "rays_shadow"):
        assert st[k] == rst[k] == pst[k], k
    png_ref.check_file(stored, px)  # render_png still returns the stored file
    assert len(png) < len(stored)
    # into the caller's buffer: the bound, the exact length, one byte short
    bound = rt._rtamd.png_deflate_bound(cam.hsize, cam.vsize)
    for buf in (rt._rtamd.host_buffer(bound), np.zeros(len(want), dtype=np.uint8)):
        n = cam.render_png_deflate_into(w, buf, depth)
        assert n == len(want) and buf[:n].tobytes() == want
    with pytest.raises(rt.RtError, match="too small"):
        cam.render_png_deflate_into(w, np.zeros(len(want) - 1, dtype=np.uint8), depth)
    w.check()


def test_render_png_deflate_first_scene(rt, oracle):
    from rtamd import scenes
    w, cam, depth = scenes.first_scene(96, 54)
    _render_checks(rt, oracle, w, cam, depth)


def test_render_png_deflate_yaml_cover(rt, oracle, tmp_path):
    text, _ = _cover_80x80(tmp_path)
    p = rt.SceneParser()
    p.load_str(text)
    _render_checks(rt, oracle, p.build_world(), p.camera, 5)


def test_render_png_deflate_aa_and_overflow(rt):
    """With AA X2, and after a forced arena overflow (the frame is rendered again before it is encoded)."""
    from rtamd import scenes
    w, cam, depth = scenes.c3(200, 113, n_spheres=600)
    cam.render_opts.aa_samples(rt.AASamples.X2)
    canvas2, _ = cam.render_multithreaded(w, depth, want_stats=False)
    want = rt.canvas_to_png_deflate(canvas2.to_numpy())
    assert cam.render_png_deflate(w, depth, 2)[0] == want
    w.tune("arena_pct", 5)
    try:
        over, _ = cam.render_png_deflate(w, depth, 2)
    finally:
        w.tune("arena_pct", 100)
    assert over == want
    w.check()


def test_render_scene_cli_compress_flag(rt, tmp_path):
    """`render_scene <scene> <out.png> --compress` writes the library call's compressed file, in a
    child process; without the flag it writes the stored file; any other argument list is refused."""
    exe = os.path.join(PKG, "bin", "render_scene")
    scene = os.path.join(SCENES, "cover.yml")
    p = rt.SceneParser()
    p.load_file(scene)
    w = p.build_world()
    out = tmp_path / "out.png"
    r = subprocess.run(["timeout", "-k", "10", "120", exe, scene, str(out), "--compress"], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == p.camera.render_png_deflate(w, 5)[0]
    lib_out = tmp_path / "lib.png"
    p.render_to(str(lib_out), 5, True)
    assert lib_out.read_bytes() == out.read_bytes()
    # 4000 segments the device agrees with itself on: the chunk CRCs hold, and zlib inflates the rows (the Adler-32)
    parts = ref.chunks(out.read_bytes())
    assert [k for k, _ in parts] == [b"IHDR", b"IDAT", b"IEND"] and ref.n_segments(4000, 4000) == 4000
    assert len(zlib.decompress(parts[1][1])) == 4000 * (3 * 4000 + 1)
    _, small = _cover_80x80(tmp_path)
    p80 = rt.SceneParser()
    p80.load_file(str(small))
    plain = tmp_path / "plain.png"
    r = subprocess.run(["timeout", "-k", "10", "120", exe, str(small), str(plain)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert plain.read_bytes() == p80.camera.render_png(p80.build_world(), 5)[0]
    for extra in (["--fast"], ["--compress", "x"]):
        r = subprocess.run(["timeout", "-k", "10", "120", exe, str(small), str(plain)] + extra, capture_output=True,
                           text=True)
        assert r.returncode == 2 and "usage: render_scene" in r.stdout
