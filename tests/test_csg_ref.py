"""The Csg checker (tests/csg_ref.py) pinned at both ends (CPU only).

Pin 1: on worlds without a Csg holding every kind 0-4 (spheres, planes, cubes,
closed / open / unbounded cylinders and cones under random transforms, nested
glass, a divided group, a shadowless shape, two lights) its hit records, a
24x16 frame and the counters equal liboracle's bit for bit; the oracle is
itself pinned by the reference's KATs.
Pin 2: the reference's Csg KATs (csg.rs:142-303) through the checker's functions.
Pin 3: on worlds with triangles (test_gpu_mesh.py's divided torus, flat and
smooth, and its 8 loose triangles) it equals the mesh checker (tests/mesh_ref.py,
itself pinned by tests/test_mesh_ref.py) bit for bit over all 24 outputs of the
hit records, a 24x16 frame and the counters.
Pin 4: on four rtamd.scenes.fuzz seeds that together hold all five pattern
kinds, each with and without a pattern transform (asserted from descs_bytes),
its 24x16 frame and counters equal liboracle's bit for bit.
Pin 5: on the tie worlds of tests/tie_worlds.py (intersections that tie bit for
bit, where the order of the world's list decides the hit, n1 and n2) the two
restatements of that order agree: the frame, the counters, the hit records of
the authored rays and color_at at depths 0 and 3 equal liboracle's bit for bit;
on the triangle grid of the `mesh` world the checker equals the mesh checker.
"""
import math
import random

import numpy as np
import pytest

import csg_ref
import mesh_ref


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


# ---------------------------------------------------------------- triangles: the mesh checker's worlds
def _mesh_world(rt, name):
    from rtamd import scenes
    if name == "loose8":
        from test_gpu_mesh import _loose8
        w, cam = _loose8(rt)
        return w, cam, [-2.5, 0.2, -1.5], [2.5, 3.0, 2.5]
    _, w, cam, _ = scenes.mesh_scene(24, 16, 10, 10, name == "smooth", 4, depth=3)
    g = np.frombuffer(w.groups_bytes(), dtype=mesh_ref.GROUP)[0]  # the torus group's box
    return w, cam, g["min"], g["max"]


@pytest.mark.parametrize("name", ["flat", "smooth", "loose8"])
def test_checker_equals_the_mesh_checker_on_triangle_worlds(rt, name):
    from test_gpu_mesh import _rays
    w, cam, lo, hi = _mesh_world(rt, name)
    kinds = np.frombuffer(w.descs_bytes(), dtype=csg_ref.SHAPE)["kind"]
    assert (kinds >= 5).sum() == (8 if name == "loose8" else 201) and w.nodes_bytes() == b""
    ref, mref = csg_ref.CsgRef.from_world(w), mesh_ref.MeshRef.from_world(w)
    rays = _rays(3, 400, lo, hi)
    got, want = ref.hit_batch(rays), mref.hit_batch(rays)
    assert got.tobytes() == want.tobytes()
    hit = want[want[:, 0] >= 0]
    assert (kinds[hit[:, 0].astype(int)] >= 5).sum() > 20 and len(set(hit[:, 21])) > 1
    assert ref.counts == mref.counts and ref.counts["other_tests"] > 0
    img, st = ref.render(cam.desc_bytes(), 3)
    mimg, mst = mref.render(cam.desc_bytes(), 3)
    assert img.tobytes() == mimg.tobytes(), np.abs(img - mimg).max()
    assert st == mst and st["other_tests"] > 0 and st["rays_reflect"] > 0 and st["rays_refract"] > 0
    assert ref.csg_ties == 0


def test_checker_refuses_a_triangle_under_a_csg(rt):
    """As the library does (test_gpu_csg.py::test_beyond_the_caps_is_refused); the records are made by
    hand, since the library does not flatten such a world."""
    w = rt.World()
    w.add_object(rt.Csg(rt.Operation.Union, rt.Sphere(), rt.Cube()))
    descs = np.frombuffer(w.descs_bytes(), dtype=csg_ref.SHAPE).copy()
    descs["kind"][1] = csg_ref.TRIANGLE
    tri = np.zeros(1, dtype=csg_ref.TRI)
    tri["p1"], tri["p2"], tri["p3"] = (0, 1, 0), (-1, 0, 0), (1, 0, 0)
    with pytest.raises(ValueError, match="under a Csg"):
        csg_ref.CsgRef(descs.tobytes(), w.nodes_bytes(), w.shape_nodes(), w.shape_sides(), w.lights_bytes(),
                       triangles_bytes=tri.tobytes())
    with pytest.raises(ValueError, match="does not match"):
        csg_ref.CsgRef(descs.tobytes(), w.nodes_bytes(), w.shape_nodes(), w.shape_sides(), w.lights_bytes())


# ---------------------------------------------------------------- patterns: the fuzz scenes
PATTERN_SEEDS = (0, 59, 17, 5)  # 0 and 59 are among test_gpu_variants.FUZZ_SEEDS


def _pattern_cover(w):
    """{(pattern kind, has a pattern transform)} of a world, from its shape records."""
    d = np.frombuffer(w.descs_bytes(), dtype=csg_ref.SHAPE)
    ident = np.eye(4).ravel()
    return {(int(k), bool((t != ident).any())) for k, t in zip(d["pattern_kind"], d["pattern_transform"]) if k >= 0}


def test_pattern_seeds_hold_every_kind_with_and_without_a_transform(rt):
    from rtamd import scenes
    import test_gpu_variants
    cover = set()
    for seed in PATTERN_SEEDS:
        cover |= _pattern_cover(scenes.fuzz(seed, 24, 16)[0])
    assert cover == {(k, t) for k in range(5) for t in (False, True)}
    assert len(PATTERN_SEEDS) == 4 and set(PATTERN_SEEDS) & set(test_gpu_variants.FUZZ_SEEDS)


@pytest.mark.parametrize("seed", PATTERN_SEEDS)
def test_checker_patterned_frame_and_counters_equal_the_oracle_bitwise(rt, oracle, seed):
    from rtamd import scenes
    w, cam, depth = scenes.fuzz(seed, 24, 16)
    assert _pattern_cover(w)
    ref = csg_ref.CsgRef.from_world(w)
    img, st = ref.render(cam.desc_bytes(), depth)
    oimg, ost = oracle.OracleWorld.from_world(w).render(cam.desc_bytes(), depth)
    assert img.tobytes() == oimg.tobytes(), np.abs(img - oimg).max()
    assert st == {k: ost[k] for k in st}


# ---------------------------------------------------------------- ties: the stable order, stated twice
import tie_worlds  # noqa: E402


@pytest.mark.parametrize("name", tie_worlds.ORACLE_WORLDS)
def test_checker_equals_oracle_on_tie_worlds(rt, oracle, name):
    """Where roots tie bit for bit the reference's order decides (world order, a group's children in
    order, also after divide; t1 before t2): the checker's stable sort and the oracle's stable merge
    sort are two independent restatements of it, held to each other here."""
    tw = tie_worlds.build(rt, name)
    ref, ow = csg_ref.CsgRef.from_world(tw.w), oracle.OracleWorld.from_world(tw.w)
    cls = tie_worlds.classify(ref, tw.rays)
    assert cls["H"].sum() >= 32  # (the floors proper: tests/test_tie_worlds.py)
    got = ref.hit_batch(tw.rays)
    want = np.array([ow.hit(r[:3], r[3:]) for r in tw.rays])
    assert got.tobytes() == want.tobytes(), int((got != want).any(axis=1).sum())
    for depth in (0, tw.depth):
        ref.counts = dict.fromkeys(csg_ref.COUNTERS, 0)
        col = ref.color_at_batch(tw.rays, depth)
        ocol, ost = ow.color_at_batch(tw.rays, depth)
        assert col.tobytes() == ocol.tobytes(), (depth, int((col != ocol).any(axis=1).sum()))
        assert ref.counts == {k: ost[k] for k in ref.counts}, depth
    img, st = ref.render(tw.cam.desc_bytes(), tw.depth)
    oimg, ost = ow.render(tw.cam.desc_bytes(), tw.depth)
    assert img.tobytes() == oimg.tobytes(), np.abs(img - oimg).max()
    assert st == {k: ost[k] for k in st}
    assert st["rays_reflect"] > 0 and st["rays_refract"] > 0


def test_checker_equals_the_mesh_checker_on_the_tie_grid(rt):
    """The `mesh` tie world without its two cubes (the mesh checker takes spheres, planes and
    triangles): 64 axis-aligned triangles whose shared edges and corners tie."""
    tw = tie_worlds.build(rt, "mesh_bare")
    ref, mref = csg_ref.CsgRef.from_world(tw.w), mesh_ref.MeshRef.from_world(tw.w)
    assert tie_worlds.classify(ref, tw.rays)["H"].sum() >= 32
    got, want = ref.hit_batch(tw.rays), mref.hit_batch(tw.rays)
    assert got.tobytes() == want.tobytes()
    for depth in (0, tw.depth):
        ref.counts, mref.counts = dict.fromkeys(csg_ref.COUNTERS, 0), dict.fromkeys(csg_ref.COUNTERS, 0)
        assert ref.color_at_batch(tw.rays, depth).tobytes() == mref.color_at_batch(tw.rays, depth).tobytes()
        assert ref.counts == mref.counts
    img, st = ref.render(tw.cam.desc_bytes(), tw.depth)
    mimg, mst = mref.render(tw.cam.desc_bytes(), tw.depth)
    assert img.tobytes() == mimg.tobytes() and st == mst and ref.csg_ties == 0
