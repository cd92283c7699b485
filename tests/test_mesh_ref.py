"""The mesh checker (tests/mesh_ref.py) pinned at both ends (CPU only).

Pin 1: on triangle-free worlds (spheres and planes under random transforms,
nested glass, groups, a shadowless shape, two lights) its canvas, hit records,
shadow answers and counters equal liboracle's bit for bit; the oracle is itself
pinned by the reference's KATs.
Pin 2: the reference's triangle KATs (triangle.rs:105-210,
smooth_triangle.rs:113-200) through the checker's triangle functions.
Pin 3: patterns. A sphere-and-plane world with all five pattern kinds, with
and without a pattern transform, equals liboracle's frame and counters bit for
bit; the reference's pattern KATs (stripe.rs, gradient.rs, ring.rs,
checkers.rs, test_pattern.rs) with their own expected colours.
"""
import math
import random

import numpy as np
import pytest

import mesh_ref


def _world(rt, seed):
    rnd = random.Random(seed)
    w = rt.World()
    floor = rt.Plane()
    floor.material.color = rt.Color(0.9, 0.85, 0.8)
    floor.material.reflective = 0.35
    w.add_object(floor)
    wall = rt.Plane()
    wall.set_transform(rt.translation(0, 0, 6) * rt.rotation_x(math.pi / 2 + 0.1 * rnd.random()))
    wall.material.color = rt.Color(0.3, 0.5, 0.7)
    wall.material.specular = 0.0
    w.add_object(wall)
    # nested glass: three spheres inside one another, different indices
    for k, (r, n) in enumerate([(1.2, 1.5), (0.8, 2.0), (0.4, 1.1)]):
        s = rt.glass_sphere()
        s.material.refractive_index = n
        s.material.reflective = 0.3 if k != 1 else 0.0
        s.material.diffuse = 0.2
        s.set_transform(rt.translation(-0.5, 1.2, 0.2 * k) * rt.scaling(r, r, r))
        w.add_object(s)

    def sphere():
        s = rt.Sphere()
        t = rt.translation(rnd.uniform(-3, 3), rnd.uniform(0.2, 2.5), rnd.uniform(-1, 3))
        t = t * rt.rotation_y(rnd.uniform(0, 3)) * rt.rotation_z(rnd.uniform(0, 3))
        if rnd.random() < 0.5:
            t = t * rt.shearing(rnd.uniform(-0.3, 0.3), 0, 0, rnd.uniform(-0.3, 0.3), 0, 0)
        s.set_transform(t * rt.scaling(rnd.uniform(0.2, 0.7), rnd.uniform(0.2, 0.7), rnd.uniform(0.2, 0.7)))
        s.material.color = rt.Color(rnd.random(), rnd.random(), rnd.random())
        s.material.reflective = rnd.choice([0.0, 0.0, 0.4])
        s.material.shininess = rnd.choice([10.0, 200.0, 37.5])
        if rnd.random() < 0.3:
            s.material.transparency = 0.7
            s.material.refractive_index = rnd.uniform(1.0, 1.6)
        if rnd.random() < 0.2:
            s.no_shadow()
        return s

    for _ in range(3):
        w.add_object(sphere())
    # groups: the transforms are set first, so every child's box is re-derived once (each
    # set_transform widens a rotated box, geometry/mod.rs:74-85), and the gates stay tight
    outer = rt.Group()
    outer.set_transform(rt.translation(0.3, 0.0, 0.5) * rt.scaling(1.1, 1.0, 0.9))
    inner = rt.Group()
    inner.set_transform(rt.rotation_y(0.4))
    for _ in range(4):
        inner.add_child(sphere())
    outer.add_child(inner)
    for _ in range(5):
        outer.add_child(sphere())
    outer.divide(2)
    w.add_object(outer)
    lidded = rt.Group()  # a plane inside a group: an infinite group box, a gate that never closes
    lid = rt.Plane()
    lid.set_transform(rt.translation(0, 4, 0))
    lid.material.transparency = 0.5
    lid.no_shadow()
    lidded.add_child(lid)
    lidded.add_child(sphere())
    w.add_object(lidded)
    w.add_light(rt.PointLight(rt.Point(-6, 8, -8), rt.Color(0.9, 0.9, 0.9)))
    w.add_light(rt.PointLight(rt.Point(4, 5, -3), rt.Color(0.3, 0.3, 0.4)))
    cam = rt.Camera(20, 14, math.pi / 3)
    cam.set_transform(rt.view_transform(rt.Point(0.2, 2.2, -6.0), rt.Point(0, 1, 0), rt.Vector(0, 1, 0)))
    return w, cam


@pytest.fixture(scope="module", params=[1, 2, 3])
def pinned(request, rt, oracle):
    w, cam = _world(rt, request.param)
    assert len(w.triangles_bytes()) == 0 and len(w.groups_bytes()) > 56
    return w, cam, mesh_ref.MeshRef.from_world(w), oracle.OracleWorld.from_world(w)


def test_checker_canvas_and_counters_equal_the_oracle_bitwise(pinned):
    w, cam, ref, ow = pinned
    for depth in (0, 3):
        img, st = ref.render(cam.desc_bytes(), depth)
        oimg, ost = ow.render(cam.desc_bytes(), depth)
        assert img.tobytes() == oimg.tobytes(), np.abs(img - oimg).max()
        assert st == {k: ost[k] for k in st}
    assert st["rays_reflect"] > 0 and st["rays_refract"] > 0 and st["sphere_tests"] < (
        st["rays_primary"] + st["rays_reflect"] + st["rays_refract"] + st["rays_shadow"]) * 16  # some gates closed


def test_checker_hit_records_equal_the_oracle_bitwise(pinned):
    w, cam, ref, ow = pinned
    rng = np.random.default_rng(7)
    n = 400
    o = rng.uniform([-3, 0.05, -5], [3, 3, 4], size=(n, 3))
    o[: n // 4] = rng.uniform([-1.2, 0.6, -0.4], [0.2, 1.8, 0.8], size=(n // 4, 3))  # inside the nested glass
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.hstack([o, d])
    got = ref.hit_batch(rays)
    want = np.array([ow.hit(r[:3], r[3:]) for r in rays])
    assert got.tobytes() == want.tobytes()
    hits = want[:, 0] >= 0
    assert hits.sum() > n // 2 and len(set(want[hits, 21])) > 2 and len(set(want[hits, 22])) > 2  # n1, n2 vary


def test_checker_shadows_and_colors_equal_the_oracle_bitwise(pinned):
    w, cam, ref, ow = pinned
    rng = np.random.default_rng(9)
    pts = rng.uniform([-3, -0.2, -3], [3, 3, 4], size=(300, 3))
    for light in (0, 1):
        got = [ref.is_shadowed(p, light) for p in pts]
        want = [ow.is_shadowed(p, light) for p in pts]
        assert got == want and 0 < sum(want) < len(want)
    o = np.tile([0.0, 1.5, -5.0], (60, 1))
    d = rng.normal([0, -0.1, 1], [0.35, 0.25, 0.05], size=(60, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.hstack([o, d])
    for depth in (0, 1, 4):
        ref.counts = dict.fromkeys(mesh_ref.COUNTERS, 0)
        got = ref.color_at_batch(rays, depth)
        want, ost = ow.color_at_batch(rays, depth)
        assert got.tobytes() == want.tobytes()
        assert ref.counts == {k: ost[k] for k in ref.counts}


def test_checker_refuses_what_it_does_not_restate(rt):
    w = rt.World()
    w.add_object(rt.Cube())
    with pytest.raises(ValueError):
        mesh_ref.MeshRef.from_world(w)
    w = rt.World()
    w.add_object(rt.Sphere())
    c = rt.Cube()
    c.material.set_pattern(rt.stripe_pattern(rt.Color(1, 1, 1), rt.Color(0, 0, 0)))
    w.add_object(c)
    with pytest.raises(ValueError):
        mesh_ref.MeshRef.from_world(w)


# ---- Pin 2: the reference's triangle KATs
def _eq(a, b):
    return all(abs(x - y) < mesh_ref.EPSILON for x, y in zip(a, b))


T = mesh_ref.triangle_new((0.0, 1.0, 0.0), (-1.0, 0.0, 0.0), (1.0, 0.0, 0.0))


def test_kat_construct_triangle():  # triangle.rs:105-120
    assert T["e1"] == (-1.0, -1.0, 0.0) and T["e2"] == (1.0, -1.0, 0.0) and _eq(T["normal"], (0.0, 0.0, -1.0))


def test_kat_normal_is_the_stored_one_everywhere(rt):  # find_normal_on_triangle, through normal_at
    w = rt.World()
    w.add_object(rt.Triangle(rt.Point(0, 1, 0), rt.Point(-1, 0, 0), rt.Point(1, 0, 0)))
    ref = mesh_ref.MeshRef.from_world(w)
    for p in ((0.0, 0.5, 0.0), (-0.5, 0.75, 0.0), (0.5, 0.25, 0.0)):
        assert ref.normal_at(0, p, (-100.0, 0, None, None)) == T["normal"]


@pytest.mark.parametrize("o,d", [((0, -1, -2), (0, 1, 0)),   # parallel to the triangle
                                 ((1, 1, -2), (0, 0, 1)),    # misses the p1-p3 edge
                                 ((-1, 1, -2), (0, 0, 1)),   # misses the p1-p2 edge
                                 ((0, -1, -2), (0, 0, 1))])  # misses the p2-p3 edge
def test_kat_rays_that_miss(o, d):  # triangle.rs:138-186
    assert mesh_ref.triangle_local_intersect(T, o, d) == []


def test_kat_ray_strikes_triangle():  # triangle.rs:188-197
    xs = mesh_ref.triangle_local_intersect(T, (0.0, 0.5, -2.0), (0, 0, 1))
    assert len(xs) == 1 and abs(xs[0][0] - 2.0) < mesh_ref.EPSILON


@pytest.mark.parametrize("smooth", [False, True])
def test_kat_triangle_bounding_box(smooth):  # triangle.rs:199-209, smooth_triangle.rs:186-199
    t = mesh_ref.triangle_new((-3.0, 7.0, 2.0), (6.0, 2.0, -4.0), (2.0, -1.0, -1.0))
    assert t["min"] == (-3.0, -1.0, -4.0) and t["max"] == (6.0, 7.0, 2.0)


def test_kat_smooth_triangle_stores_u_and_v():  # smooth_triangle.rs:133-146
    xs = mesh_ref.triangle_local_intersect(T, (-0.2, 0.3, -2.0), (0, 0, 1))
    assert abs(xs[0][1] - 0.45) < mesh_ref.EPSILON and abs(xs[0][2] - 0.25) < mesh_ref.EPSILON


def test_kat_smooth_triangle_interpolates_the_normal(rt):  # smooth_triangle.rs:148-184
    n = mesh_ref.smooth_normal((0.0, 1.0, 0.0), (-1.0, 0.0, 0.0), (1.0, 0.0, 0.0), 0.45, 0.25)
    assert _eq(mesh_ref.normalize(n), (-0.5547, 0.83205, 0.0))
    # prepare_normal_on_smooth_triangle: through normal_at and prepare
    w = rt.World()
    w.add_object(rt.SmoothTriangle(rt.Point(0, 1, 0), rt.Point(-1, 0, 0), rt.Point(1, 0, 0), rt.Vector(0, 1, 0),
                                   rt.Vector(-1, 0, 0), rt.Vector(1, 0, 0)))
    ref = mesh_ref.MeshRef.from_world(w)
    i = (1.0, 0, 0.45, 0.25)
    assert _eq(ref.normal_at(0, (0.0, 0.0, 0.0), i), (-0.5547, 0.83205, 0.0))
    comps = ref.prepare(i, (-0.2, 0.3, -2.0), (0.0, 0.0, 1.0), [i])
    assert _eq(comps["normalv"], (-0.5547, 0.83205, 0.0))
    # ... and the intersection the checker itself finds carries that u and v
    xs = ref.intersect((-0.2, 0.3, -2.0), (0.0, 0.0, 1.0))
    assert len(xs) == 1 and abs(xs[0][2] - 0.45) < mesh_ref.EPSILON and abs(xs[0][3] - 0.25) < mesh_ref.EPSILON


# ---- Pin 3: patterns
def _patterned_world(rt):
    rnd = random.Random(5)
    a, b = rt.Color(0.9, 0.2, 0.1), rt.Color(0.1, 0.3, 0.8)
    makes = [rt.test_pattern, lambda: rt.stripe_pattern(a, b), lambda: rt.gradient_pattern(a, b),
             lambda: rt.ring_pattern(a, b), lambda: rt.checkers_pattern(a, b)]
    w = rt.World()
    floor = rt.Plane()
    p = rt.checkers_pattern(rt.Color(0.9, 0.9, 0.9), rt.Color(0.2, 0.2, 0.2))
    p.set_transform(rt.rotation_y(0.3) * rt.scaling(0.7, 0.7, 0.7))
    floor.material.set_pattern(p)
    floor.material.reflective = 0.3
    w.add_object(floor)
    wall = rt.Plane()
    wall.set_transform(rt.translation(0, 0, 5) * rt.rotation_x(math.pi / 2))
    wall.material.set_pattern(rt.ring_pattern(a, b))
    w.add_object(wall)
    for k in range(10):  # every kind without and with its own transform
        s = rt.Sphere()
        s.set_transform(rt.translation(-3.2 + 1.4 * (k % 5), 0.7 + 1.5 * (k // 5), 0.5 * (k // 5)) * rt.rotation_z(0.2 * k)
                        * rt.scaling(0.6, 0.5 + 0.05 * k, 0.6))
        p = makes[k % 5]()
        if k >= 5:
            p.set_transform(rt.translation(0.1, 0.2, 0.3) * rt.rotation_y(rnd.uniform(0, 3)) * rt.scaling(0.3, 0.25, 0.2))
        s.material.set_pattern(p)
        if k in (2, 8):
            s.material.transparency = 0.6
            s.material.refractive_index = 1.4
        if k == 4:
            s.material.reflective = 0.4
        w.add_object(s)
    w.add_light(rt.PointLight(rt.Point(-6, 8, -8), rt.Color(0.9, 0.9, 0.9)))
    w.add_light(rt.PointLight(rt.Point(4, 5, -3), rt.Color(0.3, 0.3, 0.4)))
    cam = rt.Camera(24, 16, math.pi / 3)
    cam.set_transform(rt.view_transform(rt.Point(0.2, 2.0, -6.0), rt.Point(0, 1.2, 0), rt.Vector(0, 1, 0)))
    return w, cam


def test_checker_patterned_frame_and_counters_equal_the_oracle_bitwise(rt, oracle):
    w, cam = _patterned_world(rt)
    d = np.frombuffer(w.descs_bytes(), dtype=mesh_ref.SHAPE)
    ident = np.eye(4).ravel()
    cover = {(int(k), bool((t != ident).any())) for k, t in zip(d["pattern_kind"], d["pattern_transform"])}
    assert cover >= {(k, t) for k in range(5) for t in (False, True)} and set(d["kind"]) == {0, 1}
    ref = mesh_ref.MeshRef.from_world(w)
    img, st = ref.render(cam.desc_bytes(), 3)
    oimg, ost = oracle.OracleWorld.from_world(w).render(cam.desc_bytes(), 3)
    assert img.tobytes() == oimg.tobytes(), np.abs(img - oimg).max()
    assert st == {k: ost[k] for k in st}
    assert st["rays_reflect"] > 0 and st["rays_refract"] > 0
    assert len(np.unique(img.reshape(-1, 3), axis=0)) > 100


WHITE, BLACK = (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)


@pytest.mark.parametrize("kind,cases", [
    (mesh_ref.PATTERN_STRIPE, [((0, 0, 0), WHITE), ((0, 1, 0), WHITE), ((0, 2, 0), WHITE),       # stripe.rs: constant in y
                               ((0, 0, 1), WHITE), ((0, 0, 2), WHITE),                           # constant in z
                               ((0.9, 0, 0), WHITE), ((1, 0, 0), BLACK), ((-0.1, 0, 0), BLACK),  # alternates in x
                               ((-1, 0, 0), BLACK), ((-1.1, 0, 0), WHITE)]),
    (mesh_ref.PATTERN_GRADIENT, [((0, 0, 0), WHITE), ((0.25, 0, 0), (0.75, 0.75, 0.75)), ((0.5, 0, 0), (0.5, 0.5, 0.5)),
                                 ((0.75, 0, 0), (0.25, 0.25, 0.25))]),                           # gradient.rs
    (mesh_ref.PATTERN_RING, [((0, 0, 0), WHITE), ((1, 0, 0), BLACK), ((0, 0, 1), BLACK),
                             ((0.708, 0, 0.708), BLACK)]),                                       # ring.rs
    (mesh_ref.PATTERN_CHECKERS, [((0, 0, 0), WHITE), ((0.99, 0, 0), WHITE), ((1.01, 0, 0), BLACK),  # checkers.rs: x, y, z
                                 ((0, 0.99, 0), WHITE), ((0, 1.01, 0), BLACK), ((0, 0, 0.99), WHITE),
                                 ((0, 0, 1.01), BLACK)])], ids=["stripe", "gradient", "ring", "checkers"])
def test_kat_pattern_color_at(kind, cases):
    for p, want in cases:
        got = mesh_ref.pattern_color_at(kind, WHITE, BLACK, tuple(float(x) for x in p))
        assert _eq(got, want), (p, got)  # Color's PartialEq: within EPSILON


def test_kat_pattern_color_at_where_rust_and_python_differ():
    """`%` on an f64 keeps the dividend's sign (fmod); `as isize` saturates and sends a NaN to 0."""
    assert mesh_ref.pattern_color_at(mesh_ref.PATTERN_STRIPE, WHITE, BLACK, (-3.0, 0.0, 0.0)) == BLACK  # -3 % 2 == -1
    assert mesh_ref.pattern_color_at(mesh_ref.PATTERN_STRIPE, WHITE, BLACK, (float("inf"), 0.0, 0.0)) == BLACK  # NaN
    assert mesh_ref.pattern_color_at(mesh_ref.PATTERN_CHECKERS, WHITE, BLACK, (float("nan"), 0.0, 0.0)) == WHITE
    assert mesh_ref.pattern_color_at(mesh_ref.PATTERN_CHECKERS, WHITE, BLACK, (1e300, 0.0, 0.0)) == BLACK  # isize::MAX
    assert mesh_ref.pattern_color_at(mesh_ref.PATTERN_CHECKERS, WHITE, BLACK, (-1e300, 0.0, 0.0)) == WHITE  # isize::MIN
    assert mesh_ref.pattern_color_at(mesh_ref.PATTERN_CHECKERS, WHITE, BLACK, (-0.5, 0.0, 0.0)) == BLACK


@pytest.mark.parametrize("shape_t,pattern_t,point,want", [
    ((2, 2, 2), None, (2, 3, 4), (1.0, 1.5, 2.0)),                 # test_pattern.rs: an object transformation
    (None, ("s", 2, 2, 2), (2, 3, 4), (1.0, 1.5, 2.0)),            # a pattern transformation
    ((2, 2, 2), ("t", 0.5, 1.0, 1.5), (2.5, 3.0, 3.5), (0.75, 0.5, 0.25))])  # both
def test_kat_pattern_with_object_and_pattern_transformation(rt, shape_t, pattern_t, point, want):
    """Through the matrices of the library's own records, as `lighting` reads them."""
    s = rt.Sphere()
    if shape_t:
        s.set_transform(rt.scaling(*shape_t))
    p = rt.test_pattern()
    if pattern_t:
        p.set_transform((rt.scaling if pattern_t[0] == "s" else rt.translation)(*pattern_t[1:]))
    s.material.set_pattern(p)
    w = rt.World()
    w.add_object(s)
    d = np.frombuffer(w.descs_bytes(), dtype=mesh_ref.SHAPE)[0]
    got = mesh_ref.pattern_color_at_shape(int(d["pattern_kind"]), None, None, [float(x) for x in d["pattern_inverse"]],
                                          [float(x) for x in d["inverse"]], tuple(float(x) for x in point))
    assert _eq(got, want), got
    # ... and `lighting` takes that colour: ambient 1 under a white light in shadow gives it back
    d = d.copy()
    d["ambient"] = 1.0
    ref = mesh_ref.MeshRef(d.tobytes())
    L = np.array([0.0, 10.0, 0.0, 1.0, 1.0, 1.0])
    assert _eq(ref.lighting(0, L, tuple(float(x) for x in point), (0.0, 0.0, -1.0), (0.0, 0.0, -1.0), True), want)
