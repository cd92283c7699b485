"""The Csg checker (tests/csg_ref.py) pinned at both ends (CPU only).

Pin 1: on worlds without a Csg holding every kind 0-4 (spheres, planes, cubes,
closed / open / unbounded cylinders and cones under random transforms, nested
glass, a divided group, a shadowless shape, two lights) its hit records, a
24x16 frame and the counters equal liboracle's bit for bit; the oracle is
itself pinned by the reference's KATs.
Pin 2: the reference's Csg KATs (csg.rs:142-303) through the checker's functions.
"""
import math
import random

import numpy as np
import pytest

import csg_ref


def _world(rt, seed):
    rnd = random.Random(seed)
    w = rt.World()
    floor = rt.Plane()
    floor.material.color = rt.Color(0.9, 0.85, 0.8)
    floor.material.reflective = 0.35
    w.add_object(floor)
    for k, (r, n) in enumerate([(1.2, 1.5), (0.8, 2.0), (0.4, 1.1)]):  # nested glass
        s = rt.glass_sphere() if k != 1 else rt.Cube()
        s.material.transparency = 0.9
        s.material.refractive_index = n
        s.material.reflective = 0.3 if k != 1 else 0.0
        s.material.diffuse = 0.2
        s.set_transform(rt.translation(-0.5, 1.2, 0.2 * k) * rt.scaling(r, r, r))
        w.add_object(s)

    def shape():
        make = rnd.choice([rt.Sphere, rt.Cube, lambda: rt.Cylinder(-1.0, 1.0, True), lambda: rt.Cylinder(-0.5, 1.0, False),
                           lambda: rt.Cone(-1.0, 0.5, True), lambda: rt.Cone(-1.0, 0.0, False)])
        s = make()
        t = rt.translation(rnd.uniform(-3, 3), rnd.uniform(0.2, 2.5), rnd.uniform(-1, 3))
        t = t * rt.rotation_y(rnd.uniform(0, 3)) * rt.rotation_z(rnd.uniform(0, 3))
        if rnd.random() < 0.4:
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

    for _ in range(5):
        w.add_object(shape())
    pole = rt.Cylinder()  # unbounded
    pole.set_transform(rt.translation(2.5, 0, 2.5) * rt.scaling(0.15, 1.0, 0.15))
    w.add_object(pole)
    outer = rt.Group()
    outer.set_transform(rt.translation(0.3, 0.0, 0.5) * rt.scaling(1.1, 1.0, 0.9))
    inner = rt.Group()
    inner.set_transform(rt.rotation_y(0.4))
    for _ in range(4):
        inner.add_child(shape())
    outer.add_child(inner)
    for _ in range(4):
        outer.add_child(shape())
    outer.divide(2)
    w.add_object(outer)
    w.add_light(rt.PointLight(rt.Point(-6, 8, -8), rt.Color(0.9, 0.9, 0.9)))
    w.add_light(rt.PointLight(rt.Point(4, 5, -3), rt.Color(0.3, 0.3, 0.4)))
    cam = rt.Camera(24, 16, math.pi / 3)
    cam.set_transform(rt.view_transform(rt.Point(0.2, 2.2, -6.0), rt.Point(0, 1, 0), rt.Vector(0, 1, 0)))
    return w, cam


@pytest.fixture(scope="module", params=[1, 2])
def pinned(request, rt, oracle):
    w, cam = _world(rt, request.param)
    kinds = set(np.frombuffer(w.descs_bytes(), dtype=csg_ref.SHAPE)["kind"])
    assert kinds == {0, 1, 2, 3, 4} and len(w.groups_bytes()) > 56 and w.nodes_bytes() == b""
    return w, cam, csg_ref.CsgRef.from_world(w), oracle.OracleWorld.from_world(w)


def test_checker_frame_and_counters_equal_the_oracle_bitwise(pinned):
    w, cam, ref, ow = pinned
    img, st = ref.render(cam.desc_bytes(), 3)
    oimg, ost = ow.render(cam.desc_bytes(), 3)
    assert img.tobytes() == oimg.tobytes(), np.abs(img - oimg).max()
    assert st == {k: ost[k] for k in st}
    assert st["rays_reflect"] > 0 and st["rays_refract"] > 0 and st["other_tests"] > 0


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
    assert hits.sum() > n // 2 and len(set(want[hits, 21])) > 2 and len(set(want[hits, 22])) > 2


# ---------------------------------------------------------------- the reference's Csg KATs
def test_truth_table():  # csg.rs:156-205, 24 rows
    rows = [("union", True, True, True, False), ("union", True, True, False, True), ("union", True, False, True, False),
            ("union", True, False, False, True), ("union", False, True, True, False), ("union", False, True, False, False),
            ("union", False, False, True, True), ("union", False, False, False, True),
            ("intersection", True, True, True, True), ("intersection", True, True, False, False),
            ("intersection", True, False, True, True), ("intersection", True, False, False, False),
            ("intersection", False, True, True, True), ("intersection", False, True, False, True),
            ("intersection", False, False, True, False), ("intersection", False, False, False, False),
            ("difference", True, True, True, False), ("difference", True, True, False, True),
            ("difference", True, False, True, False), ("difference", True, False, False, True),
            ("difference", False, True, True, True), ("difference", False, True, False, True),
            ("difference", False, False, True, False), ("difference", False, False, False, False)]
    ops = {"union": csg_ref.UNION, "intersection": csg_ref.INTERSECTION, "difference": csg_ref.DIFFERENCE}
    assert len(rows) == 24
    for op, lhit, inl, inr, result in rows:
        assert csg_ref.intersection_allowed(ops[op], lhit, inl, inr) == result, (op, lhit, inl, inr)


@pytest.mark.parametrize("op,x0,x1", [(csg_ref.UNION, 0, 3), (csg_ref.INTERSECTION, 1, 2), (csg_ref.DIFFERENCE, 0, 1)])
def test_filtering_a_list_of_intersections(op, x0, x1):  # csg.rs:207-240: s1 = sphere, s2 = cube
    xs = [(1.0, "s1"), (2.0, "s2"), (3.0, "s1"), (4.0, "s2")]
    result = csg_ref.filter_intersections(op, lambda x: x[1] == "s1", xs)
    assert result == [xs[x0], xs[x1]]


def _csg_world(rt, op, left, right):
    w = rt.World()
    w.add_object(rt.Csg(op, left, right))
    return csg_ref.CsgRef.from_world(w)


def test_a_ray_misses_a_csg_object(rt):  # csg.rs:242-252
    ref = _csg_world(rt, rt.Operation.Union, rt.Sphere(), rt.Cube())
    assert ref.intersect((0, 2, -5), (0, 0, 1)) == []


def test_a_ray_hits_a_csg_object(rt):  # csg.rs:254-276
    s2 = rt.Sphere()
    s2.set_transform(rt.translation(0, 0, 0.5))
    ref = _csg_world(rt, rt.Operation.Union, rt.Sphere(), s2)
    xs = ref.intersect((0, 0, -5), (0, 0, 1))
    assert len(xs) == 2
    assert abs(xs[0][0] - 4.0) < 1e-5 and xs[0][1] == 0
    assert abs(xs[1][0] - 6.5) < 1e-5 and xs[1][1] == 1
    assert ref.csg_ties == 0


def test_a_csg_shape_has_a_bounding_box_that_contains_its_children(rt):  # csg.rs:278-302
    right = rt.Sphere()
    right.set_transform(rt.translation(2, 3, 4))
    c = rt.Csg(rt.Operation.Difference, rt.Sphere(), right)
    b = c.get_bounds()
    assert b.min == rt.Point(-1, -1, -1) and b.max == rt.Point(3, 4, 5)
    w = rt.World()
    w.add_object(c)
    node = np.frombuffer(w.nodes_bytes(), dtype=csg_ref.NODE)[0]
    assert list(node["min"]) == [-1, -1, -1] and list(node["max"]) == [3, 4, 5]
    assert node["kind"] == csg_ref.NODE_CSG and node["operation"] == csg_ref.DIFFERENCE and node["parent"] == -1
