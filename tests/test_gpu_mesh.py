"""Triangles, smooth triangles and OBJ meshes on the GPU, against the mesh
checker (tests/mesh_ref.py, pinned by tests/test_mesh_ref.py): hit records
bit for bit over all 24 outputs (schlick to 1e-12, as the existing hit tests
hold it), frames, counters, shadow and colour batches; the fast path (the
triangle hierarchy, tri_trace) against the exhaustive loops bit for bit on
every render entry point. Smallest shapes that reach every path: 8 loose
triangles stay in the exhaustive remainder (below the 16-record threshold),
the 200-triangle torus (10 x 10, divided with threshold 4, rotated and scaled)
plus one loose triangle go through the hierarchy with their group gates."""
import ctypes
import math

import numpy as np
import pytest

import mesh_ref

pytestmark = pytest.mark.gpu
W, H, DEPTH = 24, 16, 3
COUNTS = ("rays_primary", "rays_reflect", "rays_refract", "rays_shadow", "sphere_tests", "plane_tests", "other_tests")


def _loose8(rt):
    """8 loose triangles (flat and smooth) under random transforms, two diagonal
    spheres (so the scene has a hierarchy and takes the fast path) and a floor."""
    rng = np.random.default_rng(21)
    w = rt.World()
    floor = rt.Plane()
    floor.material.reflective = 0.3
    w.add_object(floor)
    for k in range(8):
        p = rng.uniform(-1, 1, size=(3, 3))
        if k % 2:
            n = rng.normal(size=(3, 3))
            t = rt.SmoothTriangle(*(rt.Point(*q) for q in p), *(rt.Vector(*q) for q in n))
        else:
            t = rt.Triangle(*(rt.Point(*q) for q in p))
        t.set_transform(rt.translation(*rng.uniform([-2, 0.5, -1], [2, 2.5, 2])) * rt.rotation_y(rng.uniform(0, 3)) *
                        rt.rotation_x(rng.uniform(0, 3)) * rt.scaling(*rng.uniform(0.5, 1.5, size=3)))
        t.material.color = rt.Color(*rng.uniform(0, 1, size=3))
        if k in (2, 5):
            t.material.transparency = 0.6
            t.material.refractive_index = 1.0 + 0.1 * k
        w.add_object(t)
    for x in (-1.5, 1.5):
        s = rt.glass_sphere()
        s.set_transform(rt.translation(x, 1.0, 0.5) * rt.scaling(0.6, 0.6, 0.6))
        w.add_object(s)
    w.add_light(rt.PointLight(rt.Point(-6, 8, -8), rt.Color(1, 1, 1)))
    cam = rt.Camera(W, H, math.pi / 3)
    cam.set_transform(rt.view_transform(rt.Point(0, 2, -6), rt.Point(0, 1, 0), rt.Vector(0, 1, 0)))
    return w, cam


def _rays(seed, n, box_lo, box_hi):
    """n unit rays; the first half start inside [box_lo, box_hi] (triangles lie
    behind them: n1 / n2 come from the containers walk), the rest around it."""
    rng = np.random.default_rng(seed)
    o = rng.uniform([-3.5, 0.05, -5], [3.5, 3.5, 3], size=(n, 3))
    o[: n // 2] = rng.uniform(box_lo, box_hi, size=(n // 2, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.hstack([o, d])


def _check_hits(w, rays, min_hits):
    got = w.hit_batch(rays)
    want = mesh_ref.MeshRef.from_world(w).hit_batch(rays)
    hits = want[:, 0] >= 0
    assert hits.sum() >= min_hits
    assert np.array_equal(got[:, 0], want[:, 0])  # the hit object, misses included
    # bitwise: t, point, over / under, eyev, normalv, inside, reflectv, n1, n2
    assert got[:, 1:23].tobytes() == want[:, 1:23].tobytes(), np.abs(got[:, 1:23] - want[:, 1:23]).max()
    assert np.abs(got[hits, 23] - want[hits, 23]).max() <= 1e-12  # schlick
    return want[hits]


def test_hit_batch_loose_triangles(rt):
    w, _ = _loose8(rt)
    hit = _check_hits(w, _rays(3, 1024, [-2.5, 0.2, -1.5], [2.5, 3.0, 2.5]), 300)
    kinds = np.frombuffer(w.descs_bytes(), dtype=mesh_ref.SHAPE)["kind"][hit[:, 0].astype(int)]
    assert (kinds == 5).sum() > 20 and (kinds == 6).sum() > 20
    assert len(set(hit[:, 21])) > 2 and len(set(hit[:, 22])) > 2  # triangles behind the origin are containers


@pytest.fixture(scope="module", params=[False, True], ids=["flat", "smooth"])
def torus(request, rt):
    from rtamd import scenes
    _, w, cam, depth = scenes.mesh_scene(W, H, 10, 10, request.param, 4, depth=DEPTH)
    assert len(w.triangles_bytes()) // 144 == 201 and len(w.groups_bytes()) // 56 > 10
    return w, cam, depth, request.param


def test_hit_batch_divided_torus(rt, torus):
    w, _, _, smooth = torus
    g = np.frombuffer(w.groups_bytes(), dtype=mesh_ref.GROUP)[0]  # the torus group's box
    hit = _check_hits(w, _rays(5, 1024, g["min"], g["max"]), 300)
    kinds = np.frombuffer(w.descs_bytes(), dtype=mesh_ref.SHAPE)["kind"][hit[:, 0].astype(int)]
    assert (kinds == (6 if smooth else 5)).sum() > 150
    assert len(set(hit[:, 21])) > 1 and (hit[:, 22] == 1.3).sum() > 20


def test_kat_rays_through_hit_batch(rt):  # triangle.rs:138-197
    w = rt.World()
    w.add_object(rt.Triangle(rt.Point(0, 1, 0), rt.Point(-1, 0, 0), rt.Point(1, 0, 0)))
    rays = np.array([[0, -1, -2, 0, 1, 0],    # parallel to the triangle
                     [1, 1, -2, 0, 0, 1],     # misses the p1-p3 edge
                     [-1, 1, -2, 0, 0, 1],    # misses the p1-p2 edge
                     [0, -1, -2, 0, 0, 1],    # misses the p2-p3 edge
                     [0, 0.5, -2, 0, 0, 1]], dtype=np.float64)  # strikes it at t = 2
    out = w.hit_batch(rays)
    assert (out[:4, 0] == -1).all() and not out[:4, 1:].any()
    assert out[4, 0] == 0 and abs(out[4, 1] - 2.0) < 1e-5
    assert np.allclose(out[4, 14:17], [0, 0, -1]) and out[4, 17] == 0  # the normal faces the eye
    # smooth_triangle.rs:148-184 (prepare_normal_on_smooth_triangle), with the ray's own u and v
    w = rt.World()
    w.add_object(rt.SmoothTriangle(rt.Point(0, 1, 0), rt.Point(-1, 0, 0), rt.Point(1, 0, 0), rt.Vector(0, 1, 0),
                                   rt.Vector(-1, 0, 0), rt.Vector(1, 0, 0)))
    out = w.hit_batch(np.array([[-0.2, 0.3, -2, 0, 0, 1]], dtype=np.float64))
    assert out[0, 0] == 0 and np.abs(out[0, 14:17] - [-0.5547, 0.83205, 0.0]).max() < 1e-5


@pytest.fixture(scope="module")
def frames(rt, torus):
    """The torus scene's fast and exhaustive frames with their counters, and the checker's."""
    w, cam, depth, _ = torus
    fast, fst = cam.render(w, depth, True, False)
    plan = rt._rtamd._wf_plan(w)
    exh, est = cam.render(w, depth, True, True)
    ref, rst = mesh_ref.MeshRef.from_world(w).render(cam.desc_bytes(), depth)
    return fast.to_numpy(), fst, exh.to_numpy(), est, ref, rst, plan


def test_frame_fast_equals_exhaustive_equals_checker(frames):
    fast, fst, exh, est, ref, rst, plan = frames
    assert fast.tobytes() == exh.tobytes()
    assert exh.tobytes() == ref.tobytes(), np.abs(exh - ref).max()
    assert rst["rays_reflect"] > 100 and rst["rays_refract"] > 50 and rst["other_tests"] > 0
    for k in COUNTS:
        assert fst[k] == rst[k] and est[k] == rst[k], (k, fst[k], est[k], rst[k])
    assert est["exhaustive"] and not fst["exhaustive"]


def test_plan_hook_reports_which_path_ran(rt, frames):
    plan = frames[6]["triangles"]
    assert plan["ran"] and plan["records"] == 201 and plan["nodes"] > 20 and 0 < plan["depth"] <= 60
    w, cam = _loose8(rt)
    fast, _ = cam.render(w, DEPTH, False)
    plan = rt._rtamd._wf_plan(w)  # (of the last render: read before the exhaustive one)
    exh, _ = cam.render(w, DEPTH, True, True)
    assert fast.to_numpy().tobytes() == exh.to_numpy().tobytes()
    assert plan["primary"]["lane"] >= 0  # a fused render (the spheres' hierarchy) ...
    assert not plan["triangles"]["ran"] and plan["triangles"]["records"] == 0  # ... the triangles in its remainder


def test_shadow_and_color_batches_equal_the_checker(rt, torus):
    w, cam, depth, _ = torus
    ref = mesh_ref.MeshRef.from_world(w)
    rng = np.random.default_rng(13)
    pts = rng.uniform([-3, 0.01, -2.5], [3, 3, 2.5], size=(512, 3))
    for light in (0, 1):
        got = w.is_shadowed_batch(pts, light).astype(bool)
        want = np.array([ref.is_shadowed(p, light) for p in pts])
        assert np.array_equal(got, want) and 20 < want.sum() < 492
    o = np.tile([0.0, 2.6, -6.0], (512, 1))
    d = rng.normal([0, -0.28, 1], [0.3, 0.15, 0.05], size=(512, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.hstack([o, d])
    ref.counts = dict.fromkeys(mesh_ref.COUNTERS, 0)
    want = ref.color_at_batch(rays, depth)
    got, st = w.color_at_batch(rays, depth)
    assert np.asarray(got).tobytes() == want.tobytes(), np.abs(np.asarray(got) - want).max()
    for k in COUNTS:
        assert st[k] == ref.counts[k], k
    assert (want.sum(axis=1) > 0).sum() > 400


def test_aa_fast_equals_exhaustive(rt, torus):
    w, cam, depth, _ = torus
    cam.render_opts.aa_samples(rt.AASamples.X4)
    try:
        fast, _ = cam.render_multithreaded(w, depth, False)
        exh, _ = cam.render_multithreaded(w, depth, True, True)
    finally:
        cam.render_opts.aa_samples(rt.AASamples.X1)
    assert fast.to_numpy().tobytes() == exh.to_numpy().tobytes()
    assert fast.to_numpy().sum() > 0


def test_batch_of_cameras_equals_single_renders(rt, torus):
    import torch
    w, cam, depth, _ = torus
    cams = [cam]
    for frm in ((3.0, 2.0, -5.0), (-4.0, 3.5, -3.0)):
        c = rt.Camera(W, H, math.pi / 3)
        c.set_transform(rt.view_transform(rt.Point(*frm), rt.Point(0, 0.9, 0), rt.Vector(0, 1, 0)))
        cams.append(c)
    bufs = [torch.full((H, W, 3), -1.0, dtype=torch.float64, device="cuda") for _ in cams]
    torch.cuda.synchronize()
    rt.render_frames_device(w, cams, depth, 8, 0, 1, [b.data_ptr() for b in bufs], torch.cuda.current_stream().cuda_stream,
                            False, 1)
    torch.cuda.synchronize()
    w.check()
    for c, b in zip(cams, bufs):
        one, _ = c.render(w, depth, True, True)
        assert b.cpu().numpy().tobytes() == one.to_numpy().tobytes()


def test_render_ppm_equals_canvas_to_ppm(rt, torus, frames):
    w, cam, depth, _ = torus
    ppm, _ = cam.render_ppm(w, depth)
    assert bytes(ppm) == bytes(rt.canvas_to_ppm(frames[0]))


def test_create_mesh_without_triangles_is_create_groups(rt):
    """An existing scene (scenes.groups: grouped solids, spheres and planes) through
    rt_scene_create_mesh with n_tris = 0 renders the rt_scene_create_groups frame bit for bit."""
    from rtamd import scenes
    w, cam, depth = scenes.groups(W, H)
    lib = ctypes.CDLL(rt.LIB_PATH)
    P, S, U = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32
    lib.rt_scene_create_mesh.argtypes = [P, S, P, P, S, P, S, P, S, ctypes.c_int, ctypes.POINTER(P)]
    lib.rt_scene_create_groups.argtypes = [P, S, P, P, S, P, S, ctypes.c_int, ctypes.POINTER(P)]
    lib.rt_render.argtypes = [P, ctypes.c_char_p, U, P, P]
    lib.rt_scene_destroy.argtypes = [P]
    lib.rt_last_error.restype = ctypes.c_char_p
    descs, groups, lights = w.descs_bytes(), w.groups_bytes(), w.lights_bytes()
    sg = np.asarray(w.shape_groups(), dtype=np.int32)
    n, ng, nl = len(descs) // 680, len(groups) // 56, len(lights) // 48
    a, b = P(), P()
    assert lib.rt_scene_create_groups(descs, n, sg.ctypes.data_as(P), groups, ng, lights, nl, 0, ctypes.byref(a)) == 0, \
        lib.rt_last_error()
    assert lib.rt_scene_create_mesh(descs, n, sg.ctypes.data_as(P), groups, ng, None, 0, lights, nl, 0,
                                    ctypes.byref(b)) == 0, lib.rt_last_error()
    try:
        out = [np.full((H, W, 3), -1.0), np.full((H, W, 3), -2.0)]
        for s, o in zip((a, b), out):
            assert lib.rt_render(s, cam.desc_bytes(), depth, o.ctypes.data_as(P), None) == 0, lib.rt_last_error()
        assert out[0].tobytes() == out[1].tobytes() and out[0].min() >= 0 and out[0].sum() > 0
    finally:
        lib.rt_scene_destroy(a)
        lib.rt_scene_destroy(b)
