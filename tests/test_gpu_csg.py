"""Csg (geometry/shape/csg.rs) on the GPU, against the checker (tests/csg_ref.py,
pinned by tests/test_csg_ref.py): hit records bit for bit over all 24 outputs
(schlick to 1e-12, as the existing hit tests hold it); frames and counters,
fast path = exhaustive path = checker; the other entry points; twelve seeded
random scenes; the caps. Every comparison is made on scenes in which no Csg
node's list holds two equal t (the checker's csg_ties is asserted 0), except
the one deliberate tie, which is held to the stable rule.

Shapes: 24x16 frames at depth 3-5, a handful of leaves per scene: every path of
the unit evaluation (gates, nesting up to the depth cap, groups inside and
around a Csg, a transformed Csg, plane and shadowless leaves) is reached at
that size."""
import ctypes
import math

import numpy as np
import pytest

import csg_ref

pytestmark = pytest.mark.gpu
W, H = 24, 16
COUNTS = ("rays_primary", "rays_reflect", "rays_refract", "rays_shadow", "sphere_tests", "plane_tests", "other_tests")
MAX_LEAVES, MAX_DEPTH = 16, 4  # RT_CSG_MAX_LEAVES, RT_CSG_MAX_DEPTH (include/rt_render.h)


def _camera(rt, frm=(0.0, 2.0, -6.0), to=(0.0, 0.5, 0.0), w=W, h=H):
    cam = rt.Camera(w, h, math.pi / 3)
    cam.set_transform(rt.view_transform(rt.Point(*frm), rt.Point(*to), rt.Vector(0, 1, 0)))
    return cam


def _glass(s, index, transparency=0.9):
    s.material.transparency = transparency
    s.material.refractive_index = index
    s.material.reflective = 0.3
    s.material.diffuse = 0.2
    return s


def _lights(rt, w, two=True):
    w.add_light(rt.PointLight(rt.Point(-6, 8, -8), rt.Color(1, 1, 1)))
    if two:
        w.add_light(rt.PointLight(rt.Point(5, 6, -4), rt.Color(0.35, 0.35, 0.35)))


# ---------------------------------------------------------------- scenes
def _three_ops(rt):
    """One Csg of each operation over a glass sphere and a glass cube of different indices."""
    w = rt.World()
    ops = (rt.Operation.Union, rt.Operation.Intersection, rt.Operation.Difference)
    for k, op in enumerate(ops):
        x = 2.6 * (k - 1)
        s = _glass(rt.Sphere(), 1.2 + 0.15 * k)
        s.set_transform(rt.translation(x + 0.35, 0.3, 0.1) * rt.scaling(0.9, 0.9, 0.9))
        c = _glass(rt.Cube(), 1.7 + 0.2 * k)
        c.set_transform(rt.translation(x - 0.25, -0.1, 0.0) * rt.rotation_y(0.3) * rt.scaling(0.7, 0.7, 0.7))
        w.add_object(rt.Csg(op, c, s))
    _lights(rt, w, False)
    return w


def _scene_a(rt):
    """One die on a reflective floor beside two diagonal glass spheres (the fast path's sphere image is live)."""
    from rtamd import scenes
    w = rt.World()
    floor = rt.Plane()
    floor.material.reflective = 0.3
    floor.material.color = rt.Color(0.8, 0.8, 0.7)
    w.add_object(floor)
    m = rt.Material()
    m.color = rt.Color(0.9, 0.3, 0.2)
    m.reflective = 0.2
    w.add_object(scenes.csg_die(rt.translation(0.0, 0.8, 0.0) * rt.rotation_y(0.6) * rt.scaling(0.8, 0.8, 0.8), m))
    for x, idx in ((-2.1, 1.5), (2.1, 1.33)):
        s = rt.glass_sphere()
        s.set_transform(rt.translation(x, 0.7, 0.4) * rt.scaling(0.7, 0.7, 0.7))
        s.material.refractive_index = idx
        s.material.reflective = 0.4
        w.add_object(s)
    _lights(rt, w)
    return w, _camera(rt), 4


def _scene_b(rt):
    """The quirks: a transformed Csg (its box and ray in different spaces), a Csg inside a
    transformed and divided group (the Csg's own transform takes the product), a group inside a Csg."""
    w = rt.World()
    floor = rt.Plane()
    floor.set_transform(rt.translation(0, -1.0, 0))
    w.add_object(floor)
    # a transformed Csg: small enough a move that the misplaced box still meets many local rays
    a = rt.Sphere()
    a.material.color = rt.Color(0.2, 0.8, 0.3)
    b = _glass(rt.Cube(), 1.4)
    b.set_transform(rt.translation(0.5, 0.2, 0.0) * rt.scaling(0.6, 0.6, 0.6))
    moved = rt.Csg(rt.Operation.Difference, a, b)
    moved.set_transform(rt.translation(0.3, 0.2, 0.1) * rt.rotation_y(0.4) * rt.scaling(1.1, 0.9, 1.0))
    w.add_object(moved)
    # a Csg and four spheres in a transformed group, divided
    g = rt.Group()
    c1 = rt.Cylinder(-1.0, 1.0, True)
    c1.material.color = rt.Color(0.8, 0.6, 0.1)
    c2 = rt.Sphere()
    c2.set_transform(rt.translation(0.0, 0.8, 0.0))
    c2.material.reflective = 0.5
    g.add_child(rt.Csg(rt.Operation.Union, c1, c2))
    for k in range(4):
        s = rt.Sphere()
        s.set_transform(rt.translation(-1.5 + k, 2.2, 0.3 * k) * rt.scaling(0.3, 0.3, 0.3))
        s.material.color = rt.Color(0.2 * k, 0.5, 1.0 - 0.2 * k)
        g.add_child(s)
    g.set_transform(rt.translation(-2.6, 0.0, 1.0) * rt.scaling(0.7, 0.7, 0.7))
    mat = rt.Material()
    mat.color = rt.Color(0.3, 0.3, 0.9)
    g.set_material(mat)  # reaches the spheres and the Csg's own, unused material; not the Csg's leaves
    g.divide(2)
    w.add_object(g)
    # a group inside a Csg
    inner = rt.Group()
    for k in range(2):
        s = _glass(rt.Sphere(), 1.3 + 0.3 * k)
        s.set_transform(rt.translation(2.4 + 0.7 * k, 0.2, 0.0) * rt.scaling(0.6, 0.6, 0.6))
        inner.add_child(s)
    cutter = rt.Cube()
    cutter.set_transform(rt.translation(2.75, 0.9, 0.0) * rt.scaling(1.2, 0.5, 1.2))
    w.add_object(rt.Csg(rt.Operation.Difference, inner, cutter))
    _lights(rt, w)
    return w, _camera(rt, (0.0, 2.5, -7.0)), 4


def _nest(rt, levels, x=0.0):
    """A chain of `levels` Csg nodes, each the difference / union / intersection of the chain
    below it and one more leaf: levels + 1 leaves."""
    ops = (rt.Operation.Difference, rt.Operation.Union, rt.Operation.Intersection, rt.Operation.Difference,
           rt.Operation.Union)
    node = rt.Sphere()
    node.set_transform(rt.translation(x, 0.0, 0.0) * rt.scaling(1.2, 1.2, 1.2))
    node.material.color = rt.Color(0.9, 0.5, 0.1)
    for k in range(levels):
        leaf = (rt.Cube(), rt.Sphere(), rt.Cylinder(-1.0, 1.0, True), rt.Cone(-1.0, 0.0, True), rt.Cube())[k % 5]
        leaf.set_transform(rt.translation(x + 0.5 - 0.3 * k, 0.3 * k - 0.2, -0.3) * rt.rotation_z(0.4 * k)
                           * rt.scaling(0.9 - 0.1 * k, 0.8, 1.0))
        leaf.material.color = rt.Color(0.2 + 0.15 * k, 0.3, 0.9 - 0.15 * k)
        if k % 2:
            _glass(leaf, 1.3 + 0.1 * k)
        node = rt.Csg(ops[k % 5], node, leaf)
    return node


def _scene_c(rt):
    """Nesting at the depth cap."""
    w = rt.World()
    floor = rt.Plane()
    floor.set_transform(rt.translation(0, -1.3, 0))
    floor.material.reflective = 0.2
    w.add_object(floor)
    w.add_object(_nest(rt, MAX_DEPTH))
    _lights(rt, w)
    return w, _camera(rt, (0.5, 1.5, -5.0), (0, 0, 0)), 4


def _scene_d(rt):
    """A shadowless leaf and a plane leaf (a sphere cut by a half-space)."""
    w = rt.World()
    floor = rt.Plane()
    floor.set_transform(rt.translation(0, -1.0, 0))
    w.add_object(floor)
    ball = rt.Sphere()
    ball.material.color = rt.Color(0.9, 0.2, 0.2)
    cut = rt.Plane()
    cut.set_transform(rt.translation(0, 0.3, 0) * rt.rotation_z(0.3))
    cut.material.color = rt.Color(0.2, 0.2, 0.9)
    cut.material.reflective = 0.4
    w.add_object(rt.Csg(rt.Operation.Intersection, ball, cut))
    ghost = rt.Cube()
    ghost.set_transform(rt.translation(2.2, 0.0, 0.0) * rt.scaling(0.7, 0.7, 0.7))
    ghost.no_shadow()
    solid = rt.Sphere()
    solid.set_transform(rt.translation(2.6, 0.5, -0.2) * rt.scaling(0.6, 0.6, 0.6))
    w.add_object(rt.Csg(rt.Operation.Union, ghost, solid))
    _lights(rt, w)
    return w, _camera(rt, (0.8, 2.0, -6.0), (0.8, 0.0, 0.0)), 3


def _scene_e(rt):
    """A lens (the intersection of two glass spheres) in front of a patterned wall."""
    w = rt.World()
    wall = rt.Plane()
    wall.set_transform(rt.translation(0, 0, 4) * rt.rotation_x(math.pi / 2))
    wall.material.set_pattern(rt.checkers_pattern(rt.Color(0.9, 0.9, 0.9), rt.Color(0.1, 0.1, 0.4)))
    w.add_object(wall)
    a = _glass(rt.Sphere(), 1.5, 1.0)
    a.set_transform(rt.translation(0, 0, -0.7))
    b = _glass(rt.Sphere(), 1.52, 1.0)
    b.set_transform(rt.translation(0, 0, 0.7))
    w.add_object(rt.Csg(rt.Operation.Intersection, a, b))
    for x in (-2.2, 2.2):
        s = rt.glass_sphere()
        s.set_transform(rt.translation(x, 0.0, 1.0) * rt.scaling(0.6, 0.6, 0.6))
        w.add_object(s)
    _lights(rt, w, False)
    return w, _camera(rt, (0, 0.3, -5.0), (0, 0, 0)), 5


FIXED = {"a": _scene_a, "b": _scene_b, "c": _scene_c, "d": _scene_d}


# ---------------------------------------------------------------- hit records
def _check_hits(w, rays, min_hits):
    got = w.hit_batch(rays)
    ref = csg_ref.CsgRef.from_world(w)
    want = ref.hit_batch(rays)
    hits = want[:, 0] >= 0
    assert hits.sum() >= min_hits
    assert np.array_equal(got[:, 0], want[:, 0])  # the hit object, misses included
    assert got[:, 1:23].tobytes() == want[:, 1:23].tobytes(), np.abs(got[:, 1:23] - want[:, 1:23]).max()
    assert np.abs(got[hits, 23] - want[hits, 23]).max() <= 1e-12  # schlick
    return ref, want


def _three_ops_rays():
    """The KAT rays and 1000 seeded rays over _three_ops, half starting inside the solids."""
    rng = np.random.default_rng(7)
    n = 1000
    o = rng.uniform([-4.5, -1.5, -5.0], [4.5, 2.0, 3.0], size=(n, 3))
    centre = np.array([[-2.6, 0.1, 0.0], [0.0, 0.1, 0.0], [2.6, 0.1, 0.0]])[rng.integers(0, 3, size=n // 2)]
    o[: n // 2] = centre + rng.uniform(-0.8, 0.8, size=(n // 2, 3))  # inside the solids
    d = rng.normal(size=(n, 3))
    d[n // 2:] = np.array([0.0, 0.1, 0.0]) - o[n // 2:] + rng.normal(scale=1.5, size=(n - n // 2, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    kat = np.array([[0, 2, -5, 0, 0, 1],          # csg.rs: a ray that misses a Csg
                    [-2.6, 0.1, -5, 0, 0, 1], [0.0, 0.1, -5, 0, 0, 1], [2.6, 0.1, -5, 0, 0, 1],
                    [2.6, 0.1, 5, 0, 0, -1]], dtype=np.float64)
    return np.vstack([kat, np.hstack([o, d])])


def test_hit_batch_three_operations(rt):
    w = _three_ops(rt)
    rays = _three_ops_rays()
    ref, want = _check_hits(w, rays, 400)
    assert ref.csg_ties == 0
    assert want[0, 0] == -1
    hit = want[want[:, 0] >= 0]
    assert len(set(hit[:, 21])) > 2 and len(set(hit[:, 22])) > 2
    # hits that are a leaf's second root whose first root was filtered away
    second = 0
    for r, h in zip(rays, want):
        if h[0] < 0:
            continue
        with np.errstate(all="ignore"):
            geo = ref._shape(int(h[0]), tuple(np.float64(x) for x in r[:3]), tuple(np.float64(x) for x in r[3:]))
        kept = {(x[0], x[1]) for x in ref.intersect(r[:3], r[3:])}
        if len(geo) == 2 and float(geo[1][0]) == h[1] and (float(geo[0][0]), int(h[0])) not in kept:
            second += 1
    assert second > 0


def _tie_case(rt):
    """cube - cube sharing a face, axis-aligned rays through both: the two roots on the shared face are equal."""
    w = rt.World()
    a = _glass(rt.Cube(), 1.5)
    b = _glass(rt.Cube(), 2.0)
    b.set_transform(rt.translation(2.0, 0.0, 0.0))
    w.add_object(rt.Csg(rt.Operation.Difference, a, b))
    rays = np.array([[-5, 0.25, 0.5, 1, 0, 0], [5, 0.25, 0.5, -1, 0, 0], [0, 0.25, 0.5, 1, 0, 0],
                     [2, 0.25, 0.5, -1, 0, 0], [2.5, 0.25, 0.5, 1, 0, 0]], dtype=np.float64)
    return w, rays


def test_hit_batch_deliberate_tie(rt):
    """Device = checker under the stable rule: left's root comes before right's."""
    w, rays = _tie_case(rt)
    ref, want = _check_hits(w, rays, 3)
    assert ref.csg_ties > 0


# ---------------------------------------------------------------- frames
@pytest.fixture(scope="module")
def rendered(rt):
    """Each fixed scene's fast and exhaustive frames with their counters, and the checker's."""
    out = {}
    for name, make in FIXED.items():
        w, cam, depth = make(rt)
        fast, fst = cam.render(w, depth, True, False)
        plan = rt._rtamd._wf_plan(w)
        exh, est = cam.render(w, depth, True, True)
        ref = csg_ref.CsgRef.from_world(w)
        img, rst = ref.render(cam.desc_bytes(), depth)
        out[name] = dict(w=w, cam=cam, depth=depth, fast=fast.to_numpy(), fst=fst, exh=exh.to_numpy(), est=est, ref=img,
                         rst=rst, plan=plan, ties=ref.csg_ties)
    return out


@pytest.mark.parametrize("name", sorted(FIXED))
def test_frame_fast_equals_exhaustive_equals_checker(rendered, name):
    r = rendered[name]
    assert r["ties"] == 0
    assert r["exh"].tobytes() == r["ref"].tobytes(), np.abs(r["exh"] - r["ref"]).max()
    assert r["fast"].tobytes() == r["exh"].tobytes()
    assert r["ref"].sum() > 0 and r["rst"]["rays_shadow"] > 100
    for k in COUNTS:
        assert r["fst"][k] == r["rst"][k] and r["est"][k] == r["rst"][k], (k, r["fst"][k], r["est"][k], r["rst"][k])
    assert r["est"]["sphere_disc_ge0"] == r["rst"]["sphere_disc_ge0"]
    assert r["est"]["exhaustive"]


def test_scene_a_runs_the_fused_kernels(rendered):
    r = rendered["a"]
    assert not r["fst"]["exhaustive"] and r["plan"]["secondary"]["lane"] == 15
    assert r["rst"]["rays_reflect"] > 100 and r["rst"]["rays_refract"] > 20


def test_scene_b_runs_the_lds_stack_image(rendered):
    """Scene (b) has no diagonal sphere: its grouped spheres' hierarchy opens the fused generations, and
    every one of them, generation 0 included, runs the Csg kernel of the LDS-stack image (lane 3)."""
    r = rendered["b"]
    assert not r["fst"]["exhaustive"]
    assert r["plan"]["primary"]["lane"] == 3 and r["plan"]["secondary"]["lane"] == 3


def test_lens_before_a_patterned_wall(rt):
    w, cam, depth = _scene_e(rt)
    ref = csg_ref.CsgRef.from_world(w)  # (the checker has the patterns: mesh_ref's `lighting`)
    img, rst = ref.render(cam.desc_bytes(), depth)
    assert ref.csg_ties == 0
    fast, fst = cam.render(w, depth, True, False)
    exh, est = cam.render(w, depth, True, True)
    assert exh.to_numpy().tobytes() == img.tobytes(), np.abs(exh.to_numpy() - img).max()
    assert fast.to_numpy().tobytes() == exh.to_numpy().tobytes()
    for k in COUNTS:
        assert fst[k] == rst[k] and est[k] == rst[k], (k, fst[k], est[k], rst[k])
    assert est["rays_refract"] > 50 and len(np.unique(exh.to_numpy().reshape(-1, 3), axis=0)) > 20


# ---------------------------------------------------------------- the other entry points, on scene (a)
def test_render_multithreaded_x4(rt, rendered):
    r = rendered["a"]
    w, cam, depth = r["w"], r["cam"], r["depth"]
    cam.render_opts.aa_samples(rt.AASamples.X4)
    try:
        fast, _ = cam.render_multithreaded(w, depth, False)
        exh, _ = cam.render_multithreaded(w, depth, True, True)
    finally:
        cam.render_opts.aa_samples(rt.AASamples.X1)
    assert fast.to_numpy().tobytes() == exh.to_numpy().tobytes() and fast.to_numpy().sum() > 0
    # the checker: rays_for_pixel's X4 offsets (camera.rs:71-126), Color::average (color.rs:26-33)
    ref = csg_ref.CsgRef.from_world(w)
    c = np.frombuffer(cam.desc_bytes(), dtype=csg_ref.CAMERA)[0]
    inv = [float(v) for v in c["inverse"]]
    want = np.zeros((H, W, 3))
    for y in range(H):
        for x in range(W):
            total = (0.0, 0.0, 0.0)
            for ox, oy in ((0.25, 0.25), (0.75, 0.25), (0.25, 0.75), (0.75, 0.75)):
                world_x = float(c["half_width"]) - (float(x) + ox) * float(c["pixel_size"])
                world_y = float(c["half_height"]) - (float(y) + oy) * float(c["pixel_size"])
                pixel = csg_ref.mat_point(inv, (world_x, world_y, -1.0))
                origin = csg_ref.mat_point(inv, (0.0, 0.0, 0.0))
                col = ref.color_at(origin, csg_ref.normalize(csg_ref.sub(pixel, origin)), depth)
                total = (total[0] + col[0], total[1] + col[1], total[2] + col[2])
            want[y, x] = (total[0] * (1.0 / 4.0), total[1] * (1.0 / 4.0), total[2] * (1.0 / 4.0))
    assert ref.csg_ties == 0
    assert exh.to_numpy().tobytes() == want.tobytes(), np.abs(exh.to_numpy() - want).max()


def test_batch_of_cameras(rt, rendered):
    import torch
    r = rendered["a"]
    w, depth = r["w"], r["depth"]
    cams = [r["cam"], _camera(rt, (3.0, 2.0, -5.0)), _camera(rt, (-4.0, 3.5, -3.0))]
    bufs = [torch.full((H, W, 3), -1.0, dtype=torch.float64, device="cuda") for _ in cams]
    torch.cuda.synchronize()
    rt.render_frames_device(w, cams, depth, 8, 0, 1, [b.data_ptr() for b in bufs], torch.cuda.current_stream().cuda_stream,
                            False, 1)
    torch.cuda.synchronize()
    w.check()
    ref = csg_ref.CsgRef.from_world(w)
    for c, b in zip(cams, bufs):
        one, _ = c.render(w, depth, True, True)
        assert b.cpu().numpy().tobytes() == one.to_numpy().tobytes()
        assert one.to_numpy().tobytes() == ref.render(c.desc_bytes(), depth)[0].tobytes()
    assert ref.csg_ties == 0


def test_shadow_and_color_batches(rt, rendered):
    r = rendered["a"]
    w, depth = r["w"], r["depth"]
    ref = csg_ref.CsgRef.from_world(w)
    rng = np.random.default_rng(13)
    pts = rng.uniform([-3, 0.01, -2.5], [3, 2.5, 2.5], size=(400, 3))
    for light in (0, 1):
        got = w.is_shadowed_batch(pts, light).astype(bool)
        want = np.array([ref.is_shadowed(p, light) for p in pts])
        assert np.array_equal(got, want) and 10 < want.sum() < 390
    o = np.tile([0.0, 2.0, -6.0], (400, 1))
    d = rng.normal([0, -0.25, 1], [0.3, 0.15, 0.05], size=(400, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.hstack([o, d])
    ref.counts = dict.fromkeys(csg_ref.COUNTERS, 0)
    want = ref.color_at_batch(rays, depth)
    for exhaustive in (False, True):
        got, st = w.color_at_batch(rays, depth, True, exhaustive)
        assert np.asarray(got).tobytes() == want.tobytes(), np.abs(np.asarray(got) - want).max()
        for k in COUNTS:
            assert st[k] == ref.counts[k], (k, exhaustive)
    assert ref.csg_ties == 0


def test_render_ppm(rt, rendered):
    r = rendered["a"]
    ppm, _ = r["cam"].render_ppm(r["w"], r["depth"])
    # (rt_render_ppm takes no flags: its exhaustive twin is the exhaustive frame's text)
    assert bytes(ppm) == bytes(rt.canvas_to_ppm(r["exh"])) and bytes(ppm) == bytes(rt.canvas_to_ppm(r["ref"]))


KNOB_DEFAULTS = {"image": 0, "wide": 1, "lds_wide": 1}  # tests/test_gpu_variants.py DEFAULTS


@pytest.mark.parametrize("knobs,lane", [({}, 15), ({"lds_wide": 0}, 14), ({"image": 3}, 4), ({"image": 3, "wide": 0}, 3),
                                        ({"image": 1}, 1)], ids=["lds", "pair", "wide16", "binary", "scratch"])
def test_fused_images(rt, rendered, knobs, lane):
    """Scene (a) over the default LDS image and the global-memory images (tests/test_gpu_variants.py ROWS)."""
    r = rendered["a"]
    w, cam, depth = r["w"], r["cam"], r["depth"]
    for k, v in knobs.items():
        w.tune(k, v)
    try:
        fast, fst = cam.render(w, depth, True, False)
        plan = rt._rtamd._wf_plan(w)
        plain, _ = cam.render(w, depth, False)
    finally:
        for k in knobs:
            w.tune(k, KNOB_DEFAULTS[k])
    assert plan["secondary"]["lane"] == lane, plan
    assert fast.to_numpy().tobytes() == r["ref"].tobytes() and plain.to_numpy().tobytes() == r["ref"].tobytes()
    for k in COUNTS:
        assert fst[k] == r["rst"][k], k


# ---------------------------------------------------------------- random scenes
@pytest.mark.parametrize("seed", range(12))
def test_random_scene(rt, seed):
    from rtamd import scenes
    w, cam, depth = scenes.csg_random(seed, W, H)
    ref = csg_ref.CsgRef.from_world(w)
    img, rst = ref.render(cam.desc_bytes(), depth)
    assert ref.csg_ties == 0
    fast, fst = cam.render(w, depth, True, False)
    exh, est = cam.render(w, depth, True, True)
    assert exh.to_numpy().tobytes() == img.tobytes(), np.abs(exh.to_numpy() - img).max()
    assert fast.to_numpy().tobytes() == img.tobytes()
    for k in COUNTS:
        assert fst[k] == rst[k] and est[k] == rst[k], (k, fst[k], est[k], rst[k])


# ---------------------------------------------------------------- caps and the older entry points
def _union_of(rt, n, x=0.0):
    """A balanced union of n small spheres: ceil(log2 n) levels."""
    items = []
    for k in range(n):
        s = rt.Sphere()
        s.set_transform(rt.translation(x + 0.25 * k - 0.125 * n, 0.1 * (k % 3), 0.05 * k) * rt.scaling(0.3, 0.3, 0.3))
        s.material.color = rt.Color(0.3 + 0.04 * k, 0.5, 0.9 - 0.04 * k)
        items.append(s)
    while len(items) > 1:
        nxt = [rt.Csg(rt.Operation.Union, items[i], items[i + 1]) for i in range(0, len(items) - 1, 2)]
        if len(items) % 2:
            nxt.append(items[-1])
        items = nxt
    return items[0]


def test_beyond_the_caps_is_refused(rt):
    def grouped(n):  # one leaf over the cap within the depth cap: a union of two groups of spheres
        halves = []
        for lo, hi in ((0, n // 2), (n // 2, n)):
            g = rt.Group()
            for k in range(lo, hi):
                s = rt.Sphere()
                s.set_transform(rt.translation(0.25 * k, 0.0, 0.0) * rt.scaling(0.3, 0.3, 0.3))
                g.add_child(s)
            halves.append(g)
        return rt.Csg(rt.Operation.Union, halves[0], halves[1])
    for make, word in ((lambda: grouped(MAX_LEAVES + 1), "RT_CSG_MAX_LEAVES"),
                       (lambda: _nest(rt, MAX_DEPTH + 1), "RT_CSG_MAX_DEPTH")):
        w = rt.World()
        w.add_object(make())
        _lights(rt, w, False)
        with pytest.raises(rt.RtError) as e:
            w.upload()
        assert e.value.args and word in str(e.value), str(e.value)
    w = rt.World()
    w.add_object(rt.Csg(rt.Operation.Union, rt.Triangle(rt.Point(0, 1, 0), rt.Point(-1, 0, 0), rt.Point(1, 0, 0)),
                        rt.Sphere()))
    with pytest.raises(rt.RtError) as e:
        w.upload()
    assert "Triangle under a Csg" in str(e.value)


def test_at_the_caps_renders_and_matches(rt):
    w = rt.World()
    floor = rt.Plane()
    floor.set_transform(rt.translation(0, -1.0, 0))
    w.add_object(floor)
    w.add_object(_union_of(rt, MAX_LEAVES))  # 16 leaves, 4 levels
    g = rt.Group()  # a mesh elsewhere in the same world is fine
    g.add_child(rt.Triangle(rt.Point(-3, 2, 1), rt.Point(-2, 0, 1), rt.Point(-4, 0, 1)))
    w.add_object(g)
    _lights(rt, w)
    cam = _camera(rt, (0, 1.0, -5.0), (0, 0, 0))
    fast, fst = cam.render(w, 3, True, False)
    exh, est = cam.render(w, 3, True, True)
    assert fast.to_numpy().tobytes() == exh.to_numpy().tobytes()
    ref = csg_ref.CsgRef.from_world(w)  # the whole world, the triangle included
    rays = np.array([cam_ray for cam_ray in _pixel_rays(ref, cam)])
    got = w.hit_batch(rays)
    want = ref.hit_batch(rays)
    assert ref.csg_ties == 0
    assert np.array_equal(got[:, 0], want[:, 0]) and got[:, 1:23].tobytes() == want[:, 1:23].tobytes()
    assert (want[:, 0] > 0).sum() > 30
    tri = int(np.flatnonzero(ref.s["kind"] == csg_ref.TRIANGLE)[0])
    assert (want[:, 0] == tri).sum() >= 3  # the triangle is in the frame
    img, rst = ref.render(cam.desc_bytes(), 3)
    assert exh.to_numpy().tobytes() == img.tobytes()
    for k in COUNTS:
        assert est[k] == rst[k] and fst[k] == rst[k], k


def _pixel_rays(ref, cam):
    c = np.frombuffer(cam.desc_bytes(), dtype=csg_ref.CAMERA)[0]
    for y in range(H):
        for x in range(W):
            o, d = ref.ray_for_pixel(c, x, y)
            yield list(o) + list(d)


def test_tree_without_csg_is_create_groups(rt):
    """rt_scene_create_tree with Group nodes only renders rt_scene_create_groups' frame, and the
    older entry points still refuse what they refused."""
    from rtamd import scenes
    w, cam, depth = scenes.groups(W, H)
    lib = ctypes.CDLL(rt.LIB_PATH)
    P, S, U = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32
    lib.rt_scene_create_tree.argtypes = [P, S, P, P, P, S, P, S, P, S, ctypes.c_int, ctypes.POINTER(P)]
    lib.rt_scene_create_groups.argtypes = [P, S, P, P, S, P, S, ctypes.c_int, ctypes.POINTER(P)]
    lib.rt_scene_create.argtypes = [P, S, P, S, ctypes.c_int, ctypes.POINTER(P)]
    lib.rt_render.argtypes = [P, ctypes.c_char_p, U, P, P]
    lib.rt_scene_destroy.argtypes = [P]
    lib.rt_last_error.restype = ctypes.c_char_p
    lib.rt_sizeof_node_desc.restype = S
    assert lib.rt_sizeof_node_desc() == csg_ref.NODE.itemsize == 192
    descs, groups, lights = w.descs_bytes(), w.groups_bytes(), w.lights_bytes()
    assert w.nodes_bytes() == b""
    sg = np.asarray(w.shape_groups(), dtype=np.int32)
    g = np.frombuffer(groups, dtype=csg_ref.GROUP)
    nodes = np.zeros(len(g), dtype=csg_ref.NODE)
    nodes["parent"], nodes["min"], nodes["max"] = g["parent"], g["min"], g["max"]
    n, ng, nl = len(descs) // 680, len(g), len(lights) // 48
    a, b = P(), P()
    assert lib.rt_scene_create_groups(descs, n, sg.ctypes.data_as(P), groups, ng, lights, nl, 0, ctypes.byref(a)) == 0, \
        lib.rt_last_error()
    assert lib.rt_scene_create_tree(descs, n, sg.ctypes.data_as(P), None, nodes.tobytes(), ng, None, 0, lights, nl, 0,
                                    ctypes.byref(b)) == 0, lib.rt_last_error()
    try:
        out = [np.full((H, W, 3), -1.0), np.full((H, W, 3), -2.0)]
        for s, o in zip((a, b), out):
            assert lib.rt_render(s, cam.desc_bytes(), depth, o.ctypes.data_as(P), None) == 0, lib.rt_last_error()
        assert out[0].tobytes() == out[1].tobytes() and out[0].min() >= 0 and out[0].sum() > 0
    finally:
        lib.rt_scene_destroy(a)
        lib.rt_scene_destroy(b)
    # rt_scene_create / _groups: no triangles without vertex data, as before
    tri = np.frombuffer(descs, dtype=csg_ref.SHAPE)[:1].copy()
    tri["kind"] = 5
    c = P()
    assert lib.rt_scene_create(tri.tobytes(), 1, lights, nl, 0, ctypes.byref(c)) == -2  # RT_ERR_UNSUPPORTED_SHAPE
    bad = sg.copy()
    bad[0] = ng
    assert lib.rt_scene_create_groups(descs, n, bad.ctypes.data_as(P), groups, ng, lights, nl, 0, ctypes.byref(c)) == -1
