"""The Csg units' hierarchy (rt_bvh.cpp csg_unit_box / build_unit_bvh, rt_trace.hpp unit_trace)
on the GPU: every frame, colour and counter of the fast path with the hierarchy equals the
exhaustive path's and the checker's (tests/csg_ref.py) bit for bit.

Shapes: 24x16 frames at depth 3-4. Sixteen dice are the smallest world that reaches the default
threshold (a hierarchy of several levels, leaves of one and of several units); every other world
holds one to four units and sets `csg_hier_min` to 1, so that a hierarchy of a single leaf, the
gates at the leaf, the remainder list and the count pass are all reached at that size. Each test
that needs the hierarchy sets the knob itself, creates its scene under it and restores it."""
import contextlib
import math

import numpy as np
import pytest

import csg_ref

pytestmark = pytest.mark.gpu
W, H = 24, 16
COUNTS = ("rays_primary", "rays_reflect", "rays_refract", "rays_shadow", "sphere_tests", "plane_tests", "other_tests")
MAX_DEPTH = 4  # RT_CSG_MAX_DEPTH (include/rt_render.h)
KNOB_DEFAULTS = {"image": 0, "wide": 1, "lds_wide": 1}  # tests/test_gpu_variants.py DEFAULTS


@contextlib.contextmanager
def creation_knobs(rt, **kv):
    """Scene-creation knobs (rtamd_tuning_set) for the scenes created inside; 0 restores each default."""
    try:
        for k, v in kv.items():
            rt._rtamd._tuning_set(k, v)
        yield
    finally:
        for k in kv:
            rt._rtamd._tuning_set(k, 0)


def _upload(rt, w, **kv):
    with creation_knobs(rt, **kv):
        w.upload()
    return w


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


def _floor(rt, w, y=-1.0):
    floor = rt.Plane()
    floor.set_transform(rt.translation(0, y, 0))
    floor.material.reflective = 0.2
    w.add_object(floor)


# ---------------------------------------------------------------- the small worlds (csg_hier_min = 1)
def _three_ops(rt):
    """Three units, one per operation, over a glass sphere and a glass cube of different indices: a Csg-only world."""
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
    return w, _camera(rt), 4, dict(units=3, records=3, remainder=0)


def _nested(rt):
    """One unit nested to the depth cap over boxed leaves (sphere, cube, cylinders open and closed)."""
    ops = (rt.Operation.Difference, rt.Operation.Union, rt.Operation.Intersection, rt.Operation.Difference)
    node = rt.Sphere()
    node.set_transform(rt.scaling(1.2, 1.2, 1.2))
    node.material.color = rt.Color(0.9, 0.5, 0.1)
    for k in range(MAX_DEPTH):
        leaf = (rt.Cube(), rt.Sphere(), rt.Cylinder(-1.0, 1.0, True), rt.Cylinder(-0.8, 0.9, False))[k]
        leaf.set_transform(rt.translation(0.5 - 0.3 * k, 0.3 * k - 0.2, -0.3) * rt.rotation_z(0.4 * k)
                           * rt.scaling(0.9 - 0.1 * k, 0.8, 1.0))
        leaf.material.color = rt.Color(0.2 + 0.15 * k, 0.3, 0.9 - 0.15 * k)
        if k % 2:
            _glass(leaf, 1.3 + 0.1 * k)
        node = rt.Csg(ops[k], node, leaf)
    w = rt.World()
    _floor(rt, w, -1.3)
    w.add_object(node)
    _lights(rt, w)
    return w, _camera(rt, (0.5, 1.5, -5.0), (0, 0, 0)), 4, dict(units=1, records=1, remainder=0)


def _moved(rt):
    """A transformed Csg: the reference gates its box against a ray of another space (csg.rs:115-118); the
    hierarchy's box comes from the leaves through the forward chain, and the quirky gate stays in the program."""
    w = rt.World()
    _floor(rt, w)
    a = rt.Sphere()
    a.material.color = rt.Color(0.2, 0.8, 0.3)
    b = _glass(rt.Cube(), 1.4)
    b.set_transform(rt.translation(0.5, 0.2, 0.0) * rt.scaling(0.6, 0.6, 0.6))
    moved = rt.Csg(rt.Operation.Difference, a, b)
    moved.set_transform(rt.translation(0.3, 0.2, 0.1) * rt.rotation_y(0.4) * rt.scaling(1.1, 0.9, 1.0))
    w.add_object(moved)
    _lights(rt, w)
    return w, _camera(rt, (0.0, 2.5, -7.0)), 4, dict(units=1, records=1, remainder=0)


def _grouped(rt):
    """A unit and four spheres inside a transformed, divided group: the unit's group gate is tested at
    the hierarchy's leaf, and a failed gate owes the unit's leaves through the count pass."""
    w = rt.World()
    _floor(rt, w)
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
    g.set_transform(rt.translation(-1.0, 0.0, 1.0) * rt.scaling(0.7, 0.7, 0.7))
    g.divide(2)
    w.add_object(g)
    _lights(rt, w)
    return w, _camera(rt, (0.0, 2.5, -7.0)), 3, dict(units=1, records=1, remainder=0)


def _group_inside(rt):
    """A group inside a unit: its gate (kCsgGroup) is part of the program."""
    w = rt.World()
    _floor(rt, w)
    inner = rt.Group()
    for k in range(2):
        s = _glass(rt.Sphere(), 1.3 + 0.3 * k)
        s.set_transform(rt.translation(-0.35 + 0.7 * k, 0.2, 0.0) * rt.scaling(0.6, 0.6, 0.6))
        inner.add_child(s)
    cutter = rt.Cube()
    cutter.set_transform(rt.translation(0.0, 0.9, 0.0) * rt.scaling(1.2, 0.5, 1.2))
    w.add_object(rt.Csg(rt.Operation.Difference, inner, cutter))
    _lights(rt, w)
    return w, _camera(rt, (0.0, 2.0, -5.0), (0, 0.2, 0)), 4, dict(units=1, records=1, remainder=0)


def _shadowless(rt):
    """A shadowless leaf: shadow rays through the hierarchy take the leaf's own has_shadow."""
    w = rt.World()
    _floor(rt, w)
    ghost = rt.Cube()
    ghost.set_transform(rt.translation(0.2, 0.0, 0.0) * rt.scaling(0.7, 0.7, 0.7))
    ghost.no_shadow()
    solid = rt.Sphere()
    solid.set_transform(rt.translation(0.6, 0.5, -0.2) * rt.scaling(0.6, 0.6, 0.6))
    w.add_object(rt.Csg(rt.Operation.Union, ghost, solid))
    _lights(rt, w)
    return w, _camera(rt, (0.8, 2.0, -6.0), (0.4, 0.0, 0.0)), 3, dict(units=1, records=1, remainder=0)


def _mixed(rt):
    """A unit with a plane leaf and one with a cone leaf (no box: the remainder list) beside two boxed units."""
    w = rt.World()
    _floor(rt, w)
    ball = rt.Sphere()
    ball.set_transform(rt.translation(-2.4, 0.0, 0.0))
    ball.material.color = rt.Color(0.9, 0.2, 0.2)
    cut = rt.Plane()
    cut.set_transform(rt.translation(0, 0.3, 0) * rt.rotation_z(0.3))
    cut.material.color = rt.Color(0.2, 0.2, 0.9)
    w.add_object(rt.Csg(rt.Operation.Intersection, ball, cut))
    cone = rt.Cone(-1.0, 0.0, True)
    cone.set_transform(rt.translation(-0.6, 0.6, 0.5))
    cone.material.color = rt.Color(0.9, 0.8, 0.1)
    bite = rt.Sphere()
    bite.set_transform(rt.translation(-0.3, 0.3, 0.0) * rt.scaling(0.5, 0.5, 0.5))
    w.add_object(rt.Csg(rt.Operation.Difference, cone, bite))
    for k in range(2):
        c = _glass(rt.Cube(), 1.5 + 0.2 * k) if k else rt.Cube()
        c.set_transform(rt.translation(1.2 + 1.7 * k, -0.2, 0.3 * k) * rt.rotation_y(0.5) * rt.scaling(0.6, 0.6, 0.6))
        s = rt.Sphere()
        s.set_transform(rt.translation(1.4 + 1.7 * k, 0.3, 0.2) * rt.scaling(0.6, 0.6, 0.6))
        s.material.color = rt.Color(0.3, 0.9 - 0.4 * k, 0.4)
        w.add_object(rt.Csg(rt.Operation.Union if k else rt.Operation.Difference, c, s))
    _lights(rt, w)
    return w, _camera(rt, (0.3, 2.5, -7.0)), 3, dict(units=4, records=2, remainder=2)


SMALL = {"three_ops": _three_ops, "nested": _nested, "moved": _moved, "grouped": _grouped, "group_inside": _group_inside,
         "shadowless": _shadowless, "mixed": _mixed}


@pytest.fixture(scope="module")
def small(rt):
    """Each small world, created with csg_hier_min = 1: its fast (counted and plain) and exhaustive
    frames, the plans of the fast render, and the checker's frame and counters."""
    out = {}
    for name, make in SMALL.items():
        w, cam, depth, want = make(rt)
        _upload(rt, w, csg_hier_min=1)
        fast, fst = cam.render(w, depth, True, False)
        plan, cplan = rt._rtamd._wf_plan(w), rt._rtamd._csg_plan(w)
        plain, _ = cam.render(w, depth, False, False)
        exh, est = cam.render(w, depth, True, True)
        ref = csg_ref.CsgRef.from_world(w)
        img, rst = ref.render(cam.desc_bytes(), depth)
        out[name] = dict(w=w, cam=cam, depth=depth, want=want, fast=fast.to_numpy(), plain=plain.to_numpy(), fst=fst,
                         exh=exh.to_numpy(), est=est, ref=img, rst=rst, plan=plan, cplan=cplan, ties=ref.csg_ties)
    return out


@pytest.mark.parametrize("name", sorted(SMALL))
def test_small_world_fast_equals_exhaustive_equals_checker(small, name):
    r = small[name]
    cp = r["cplan"]
    assert {k: cp[k] for k in r["want"]} == r["want"], cp
    assert cp["ran"] and cp["nodes"] >= 1 and not r["fst"]["exhaustive"]
    assert r["plan"]["primary"]["lane"] >= 0
    assert r["ties"] == 0
    assert r["exh"].tobytes() == r["ref"].tobytes(), np.abs(r["exh"] - r["ref"]).max()
    assert r["fast"].tobytes() == r["exh"].tobytes(), np.abs(r["fast"] - r["exh"]).max()
    assert r["plain"].tobytes() == r["exh"].tobytes(), np.abs(r["plain"] - r["exh"]).max()
    assert r["ref"].sum() > 0 and r["rst"]["rays_shadow"] > 100
    for k in COUNTS:
        assert r["fst"][k] == r["rst"][k] and r["est"][k] == r["rst"][k], (k, r["fst"][k], r["est"][k], r["rst"][k])
    assert r["est"]["exhaustive"]


def test_grouped_unit_is_gated_and_counted(small):
    """The world of the gate at the leaf: rays do miss the group's boxes (the count pass is what
    keeps other_tests and sphere_tests the reference's)."""
    r = small["grouped"]
    n_rays = sum(r["rst"][k] for k in COUNTS[:4])
    assert r["rst"]["sphere_tests"] < 5 * n_rays and r["rst"]["other_tests"] < n_rays  # 5 spheres, 1 cylinder


def test_rays_outside_the_padding_domain(rt, small):
    """The boxes' padding is argued for finite rays with |d|_inf >= 0.5 from |o|_inf <= 4096 (kUnitDirMin,
    kUnitOriginMax); a caller's ray outside that evaluates every unit of the hierarchy instead of walking
    it. Far origins and short directions, beside ordinary rays, against the checker."""
    r = small["three_ops"]
    w, depth = r["w"], 3
    rng = np.random.default_rng(11)
    n = 60
    aim = np.array([[-2.6, 0.1, 0.0], [0.0, 0.1, 0.0], [2.6, 0.1, 0.0]])[rng.integers(0, 3, size=n)]
    aim = aim + rng.uniform(-0.6, 0.6, size=(n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    dist = np.where(np.arange(n) % 3 == 0, 9000.0, 6.0)[:, None]  # a third from beyond the origin bound
    o = aim - dist * d
    d[1::3] *= 0.25  # a third with |d|_inf below the direction bound
    rays = np.hstack([o, d])
    assert (np.abs(o).max(axis=1) > 4096).sum() >= 15 and (np.abs(d).max(axis=1) < 0.5).sum() >= 15
    ref = csg_ref.CsgRef.from_world(w)
    want = ref.color_at_batch(rays, depth)
    assert ref.csg_ties == 0 and (want.sum(axis=1) > 0).sum() >= 20
    for exhaustive in (False, True):
        got, st = w.color_at_batch(rays, depth, True, exhaustive)
        assert np.asarray(got).tobytes() == want.tobytes(), (exhaustive, np.abs(np.asarray(got) - want).max())
        for k in COUNTS:
            assert st[k] == ref.counts[k], (k, exhaustive, st[k], ref.counts[k])
    assert rt._rtamd._csg_plan(w)["records"] == 3


# ---------------------------------------------------------------- 1, 5, 6: sixteen dice
@pytest.fixture(scope="module")
def dice(rt):
    from rtamd import scenes
    w, cam, _ = scenes.csg_dice(16, W, H)
    _upload(rt, w, csg_hier_min=16)
    return w, cam, 3


def test_csg_only_world_opens_the_fused_path(rt, dice):
    """A floor and sixteen dice: no sphere, solid or triangle hierarchy, so the units' hierarchy is
    what opens the fused generations (the parent renders this world with the exhaustive pipeline)."""
    w, cam, depth = dice
    fast, fst = cam.render(w, depth, True, False)
    plan, cp = rt._rtamd._wf_plan(w), rt._rtamd._csg_plan(w)
    plain, _ = cam.render(w, depth, False, False)
    exh, est = cam.render(w, depth, True, True)
    assert cp["units"] == 16 and cp["records"] == 16 and cp["remainder"] == 0 and cp["ran"], cp
    assert cp["nodes"] >= 8 and 1 <= cp["depth"] <= 60
    assert plan["primary"]["lane"] >= 0 and plan["secondary"]["lane"] >= 0, plan
    assert not fst["exhaustive"] and est["exhaustive"]
    assert fast.to_numpy().tobytes() == exh.to_numpy().tobytes()
    assert plain.to_numpy().tobytes() == exh.to_numpy().tobytes()
    assert exh.to_numpy().sum() > 0 and est["rays_reflect"] > 100 and est["rays_refract"] > 20
    for k in COUNTS:
        assert fst[k] == est[k], (k, fst[k], est[k])


@pytest.mark.parametrize("leaf", [1, 4])
def test_leaves_of_several_units(rt, dice, leaf):
    from rtamd import scenes
    w0, cam, depth = dice
    want, _ = cam.render(w0, depth, False, True)
    w, _, _ = scenes.csg_dice(16, W, H)
    _upload(rt, w, csg_hier_min=16, bvh_leaf=leaf)
    got, st = cam.render(w, depth, True, False)
    cp = rt._rtamd._csg_plan(w)
    assert cp["records"] == 16 and cp["ran"] and not st["exhaustive"]
    assert (cp["nodes"] >= 8) if leaf == 1 else (cp["nodes"] <= 8), cp
    assert got.to_numpy().tobytes() == want.to_numpy().tobytes()


def test_batch_of_cameras(rt, dice):
    import torch
    w, cam, depth = dice
    cams = [cam, _camera(rt, (3.0, 3.0, -5.0), (0.0, 0.3, 2.0))]
    bufs = [torch.full((H, W, 3), -1.0, dtype=torch.float64, device="cuda") for _ in cams]
    torch.cuda.synchronize()
    rt.render_frames_device(w, cams, depth, 8, 0, 1, [b.data_ptr() for b in bufs], torch.cuda.current_stream().cuda_stream,
                            False, 1)
    torch.cuda.synchronize()
    w.check()
    assert rt._rtamd._csg_plan(w)["ran"]
    for c, b in zip(cams, bufs):
        one, _ = c.render(w, depth, False, False)
        exh, _ = c.render(w, depth, False, True)
        assert b.cpu().numpy().tobytes() == one.to_numpy().tobytes()
        assert one.to_numpy().tobytes() == exh.to_numpy().tobytes() and one.to_numpy().sum() > 0


# ---------------------------------------------------------------- 3: the line rule
def _behind_world(rt, with_unit):
    """A glass target sphere ahead of the rays (they travel along +x from x = 2) before a checkered wall, and, wholly behind their
    origins, a glass cube minus a glass sphere that pokes out of its far side. Backwards along a ray's
    line: the cube's near face (a survivor of the cube), the sphere's end inside the cube (a survivor of
    the sphere), then two roots the difference filters away. Each leaf keeps ONE root behind the origin:
    both are `containers` entries at the hit ahead (intersection.rs:63-90), though [0, t_hi] never meets them."""
    w = rt.World()
    target = rt.glass_sphere()
    target.set_transform(rt.translation(5.0, 0.0, 0.0))
    target.material.refractive_index = 1.5
    target.material.reflective = 0.3  # Schlick: n1 reaches the colour through the reflectance too
    w.add_object(target)
    wall = rt.Plane()  # what the refracted rays land on: their direction depends on n1 / n2
    wall.set_transform(rt.translation(9.0, 0.0, 0.0) * rt.rotation_z(math.pi / 2))
    pattern = rt.checkers_pattern(rt.Color(0.9, 0.9, 0.9), rt.Color(0.1, 0.1, 0.4))
    pattern.set_transform(rt.scaling(0.2, 0.2, 0.2))
    wall.material.set_pattern(pattern)
    w.add_object(wall)
    if with_unit:
        cube = _glass(rt.Cube(), 1.9)
        poke = _glass(rt.Sphere(), 1.3)
        poke.set_transform(rt.translation(-1.0, 0.0, 0.0) * rt.scaling(0.8, 0.8, 0.8))
        w.add_object(rt.Csg(rt.Operation.Difference, cube, poke))
    _lights(rt, w, False)
    return w


def test_line_rule_unit_behind_the_origin(rt):
    rng = np.random.default_rng(5)
    n = 48
    o = np.column_stack([np.full(n, 2.0), rng.uniform(-0.3, 0.3, n), rng.uniform(-0.3, 0.3, n)])
    d = np.column_stack([np.ones(n), rng.uniform(-0.05, 0.05, n), rng.uniform(-0.05, 0.05, n)])
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.hstack([o, d])
    depth = 3
    w = _upload(rt, _behind_world(rt, True), csg_hier_min=1)
    ref = csg_ref.CsgRef.from_world(w)
    bare = csg_ref.CsgRef.from_world(_behind_world(rt, False))
    with_unit, without = ref.hit_batch(rays), bare.hit_batch(rays)
    # chosen on the CPU: the same hit ahead, on the target, with another n1
    assert np.array_equal(with_unit[:, 0], without[:, 0]) and (with_unit[:, 0] == 0).all()
    assert with_unit[:, 1].tobytes() == without[:, 1].tobytes() and (with_unit[:, 1] > 0).all()
    changed = int((with_unit[:, 21] != without[:, 21]).sum())
    assert changed >= 10, changed
    assert ref.csg_ties == 0
    ref.counts = dict.fromkeys(csg_ref.COUNTERS, 0)
    want = ref.color_at_batch(rays, depth)
    assert want.tobytes() != bare.color_at_batch(rays, depth).tobytes()  # n1 reaches the colours
    for exhaustive in (False, True):
        got, st = w.color_at_batch(rays, depth, True, exhaustive)
        if not exhaustive:
            cp = rt._rtamd._csg_plan(w)
            assert cp["records"] == 1 and cp["ran"] and not st["exhaustive"], cp
        assert np.asarray(got).tobytes() == want.tobytes(), (exhaustive, np.abs(np.asarray(got) - want).max())
        for k in COUNTS:
            assert st[k] == ref.counts[k], (k, exhaustive, st[k], ref.counts[k])
    # the frame too: Camera::render goes through the same walk
    cam = _camera(rt, (2.0, 0.1, 0.05), (5.0, 0.0, 0.0))
    fast, _ = cam.render(w, depth, False, False)
    img, _ = ref.render(cam.desc_bytes(), depth)
    assert fast.to_numpy().tobytes() == img.tobytes() and img.sum() > 0


# ---------------------------------------------------------------- 4: every CSG fused image
@pytest.fixture(scope="module")
def imaged(rt):
    """The transformed Csg of `_moved` beside two diagonal glass spheres (the sphere images are live)."""
    w, cam, depth, _ = _moved(rt)
    for x, idx in ((-2.1, 1.5), (2.3, 1.33)):
        s = rt.glass_sphere()
        s.set_transform(rt.translation(x, 0.7, 0.4) * rt.scaling(0.7, 0.7, 0.7))
        s.material.refractive_index = idx
        s.material.reflective = 0.4
        w.add_object(s)
    _upload(rt, w, csg_hier_min=1)
    ref = csg_ref.CsgRef.from_world(w)
    img, rst = ref.render(cam.desc_bytes(), depth)
    assert ref.csg_ties == 0
    return w, cam, depth, img, rst


@pytest.mark.parametrize("knobs,lane", [({}, 15), ({"lds_wide": 0}, 14), ({"image": 3}, 4), ({"image": 3, "wide": 0}, 3),
                                        ({"image": 1}, 1)], ids=["lds", "pair", "wide16", "binary", "scratch"])
def test_fused_images(rt, imaged, knobs, lane):
    """The five knob rows of tests/test_gpu_csg.py::test_fused_images, counted and plain, with the hierarchy."""
    w, cam, depth, img, rst = imaged
    for k, v in knobs.items():
        w.tune(k, v)
    try:
        fast, fst = cam.render(w, depth, True, False)
        plan, cp = rt._rtamd._wf_plan(w), rt._rtamd._csg_plan(w)
        plain, _ = cam.render(w, depth, False, False)
        cp_plain = rt._rtamd._csg_plan(w)
    finally:
        for k in knobs:
            w.tune(k, KNOB_DEFAULTS[k])
    assert plan["secondary"]["lane"] == lane, plan
    assert cp["records"] == 1 and cp["ran"] and cp_plain["ran"], cp
    assert fast.to_numpy().tobytes() == img.tobytes(), np.abs(fast.to_numpy() - img).max()
    assert plain.to_numpy().tobytes() == img.tobytes(), np.abs(plain.to_numpy() - img).max()
    assert img.sum() > 0 and rst["rays_refract"] > 20
    for k in COUNTS:
        assert fst[k] == rst[k], (k, fst[k], rst[k])


# ---------------------------------------------------------------- 7: the default threshold
def test_default_threshold_leaves_small_worlds_alone(rt):
    """With the knob at its default a world of a few units has no hierarchy and keeps its path: the
    Csg-only world the exhaustive pipeline, a random scene with plain spheres its fused LDS image."""
    from rtamd import scenes
    w, cam, depth, _ = _three_ops(rt)
    _, st = cam.render(w, depth, True, False)
    cp, plan = rt._rtamd._csg_plan(w), rt._rtamd._wf_plan(w)
    assert cp["units"] == 3 and cp["records"] == 0 and cp["nodes"] == 0 and cp["remainder"] == 3 and not cp["ran"], cp
    assert plan["primary"]["lane"] == -1 and plan["secondary"]["lane"] == -1 and st["exhaustive"]
    w, cam, depth = scenes.csg_random(0, W, H)
    _, st = cam.render(w, depth, True, False)
    cp, plan = rt._rtamd._csg_plan(w), rt._rtamd._wf_plan(w)
    assert cp["units"] >= 2 and cp["records"] == 0 and cp["remainder"] == cp["units"] and not cp["ran"], cp
    assert plan["secondary"]["lane"] == 15 and not st["exhaustive"], plan


def test_knob_range(rt):
    for bad in (-1, 65537):
        with pytest.raises(rt.RtError):
            rt._rtamd._tuning_set("csg_hier_min", bad)
    with creation_knobs(rt, csg_hier_min=65536):
        pass
