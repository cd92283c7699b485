"""Csg trees beyond the caps on the GPU (deep units: World.upload(deep_csg=True), rt_scene_create_ex with
RT_SCENE_DEEP_CSG, the evaluator csg_deep_eval), bit for bit against the checkers tests/csg_ref.py and
tests/csg_tri_ref.py, which restate the reference's nested sort and filter recursively and have no cap. Every frame is
rendered on the fast path (plain and counted) and with RT_RENDER_EXHAUSTIVE and compared with the checker's byte for
byte, the counters for equality (tests/test_gpu_csg_mesh.py's _check_frames / _check_hits). The floors asserted of each
world are the checker's own figures: a world that drifts cannot pass silently.

Shapes: 24x16 frames at depth 3-4 and a few hundred rays; units of 6 to 70 leaves, 2 to 69 levels: the smallest beyond
each cap, the book's die (22 leaves, 21 levels), rows whose roots need one, two and three batches of 64, a mesh under 36
nodes, flush cubes (ties), twelve random scenes; and every existing Csg scene through the deep evaluator under the
development knob csg_deep_all against the other two evaluators."""
import contextlib
import math

import numpy as np
import pytest

import csg_ref
import csg_tri_ref
import test_csg_deep_host as host
import tie_worlds
from test_gpu_csg import _glass, _lights
from test_gpu_csg_mesh import COUNTS, _check_frames, _check_hits

pytestmark = pytest.mark.gpu
W, H = 24, 16
EXACT = COUNTS + ("sphere_disc_ge0",)


def _camera(rt, frm, to, fov=math.pi / 3, w=W, h=H):
    cam = rt.Camera(w, h, fov)
    cam.set_transform(rt.view_transform(rt.Point(*frm), rt.Point(*to), rt.Vector(0, 1, 0)))
    return cam


def _floor_world(rt):
    w = rt.World()
    floor = rt.Plane()
    floor.set_transform(rt.translation(0, -1, 0))
    floor.material.reflective = 0.2
    w.add_object(floor)
    return w


def _deep(rt, w, units=1):
    """Uploads with the opt-in and holds the scene to deep units; returns the plan."""
    w.upload(deep_csg=True)
    plan = rt._rtamd._csg_deep_plan(w)
    assert plan["units"] >= units and plan["lane_bytes"] == 4 * (2 * ((plan["nodes"] + 31) // 32) + (plan["leaves"] + 31) // 32
                                                                 + 12 * plan["levels"]), plan
    return plan


def _x4_want(ref, cam, depth):
    """rays_for_pixel's X4 offsets (camera.rs:71-126) and Color::average (color.rs:26-33) over the checker."""
    c = np.frombuffer(cam.desc_bytes(), dtype=csg_ref.CAMERA)[0]
    inv = [float(v) for v in c["inverse"]]
    want = np.zeros((int(c["vsize"]), int(c["hsize"]), 3))
    origin = csg_ref.mat_point(inv, (0.0, 0.0, 0.0))
    for y in range(want.shape[0]):
        for x in range(want.shape[1]):
            total = (0.0, 0.0, 0.0)
            for ox, oy in ((0.25, 0.25), (0.75, 0.25), (0.25, 0.75), (0.75, 0.75)):
                world_x = float(c["half_width"]) - (float(x) + ox) * float(c["pixel_size"])
                world_y = float(c["half_height"]) - (float(y) + oy) * float(c["pixel_size"])
                pixel = csg_ref.mat_point(inv, (world_x, world_y, -1.0))
                col = ref.color_at(origin, csg_ref.normalize(csg_ref.sub(pixel, origin)), depth)
                total = (total[0] + col[0], total[1] + col[1], total[2] + col[2])
            want[y, x] = (total[0] * (1.0 / 4.0), total[1] * (1.0 / 4.0), total[2] * (1.0 / 4.0))
    return want


def _as_batches(rt, w, view, depth, ref, others, x4=(12, 8)):
    """The other entry points: an X4 frame (a smaller one: four checker rays a pixel), three cameras in one
    render_frames call, hit_batch, color_at_batch and is_shadowed_batch over the frame's pixel rays.
    `view`: the frame's camera as _camera's (from, to, fov)."""
    import torch
    cam = _camera(rt, *view)
    small = _camera(rt, *view, w=x4[0], h=x4[1])
    small.render_opts.aa_samples(rt.AASamples.X4)
    want4 = _x4_want(ref, small, depth)
    fast4, _ = small.render_multithreaded(w, depth, False)
    exh4, _ = small.render_multithreaded(w, depth, True, True)
    assert exh4.to_numpy().tobytes() == want4.tobytes() and fast4.to_numpy().tobytes() == want4.tobytes()
    cams = [cam] + list(others)
    bufs = [torch.full((H, W, 3), -1.0, dtype=torch.float64, device="cuda") for _ in cams]
    torch.cuda.synchronize()
    rt.render_frames_device(w, cams, depth, 8, 0, 1, [b.data_ptr() for b in bufs], torch.cuda.current_stream().cuda_stream,
                            False, 1)
    torch.cuda.synchronize()
    w.check()
    for c, b in zip(cams, bufs):
        assert b.cpu().numpy().tobytes() == ref.render(c.desc_bytes(), depth)[0].tobytes()
    rays = tie_worlds.pixel_rays(ref, cam)
    want = _check_hits(w, ref, rays, len(rays) // 4)
    ref.counts = dict.fromkeys(csg_ref.COUNTERS, 0)
    colors = ref.color_at_batch(rays, depth)
    for exhaustive in (False, True):
        got, st = w.color_at_batch(rays, depth, True, exhaustive)
        assert np.asarray(got).tobytes() == colors.tobytes(), np.abs(np.asarray(got) - colors).max()
        for k in COUNTS:
            assert st[k] == ref.counts[k], (k, exhaustive, st[k], ref.counts[k])
    pts = want[want[:, 0] >= 0][:, 5:8]  # the hits' over points
    for light in range(2):
        got = w.is_shadowed_batch(pts, light).astype(bool)
        assert np.array_equal(got, np.array([ref.is_shadowed(p, light) for p in pts]))
    return want


# ---------------------------------------------------------------- the smallest world beyond each cap
@pytest.mark.parametrize("name", ["leaves", "depth", "nodes"])
def test_smallest_beyond_each_cap(rt, name):
    if name == "nodes":
        w = host.nodes_world(rt)
        shape = None
    else:
        shape = host.BEYOND[name][0](rt)
        w = _floor_world(rt)
        w.add_object(shape)
    _lights(rt, w)
    with pytest.raises(rt.RtError, match="RT_CSG_MAX_" + {"leaves": "LEAVES", "depth": "DEPTH", "nodes": "NODES"}[name]):
        w.upload()
    plan = _deep(rt, w)
    assert (plan["leaves"] > 16, plan["levels"] > 4, plan["nodes"] > 32) == (name == "leaves", name == "depth", name == "nodes")
    ref = (csg_tri_ref.CsgTriRef if name == "nodes" else csg_ref.CsgRef).from_world(w)
    cam = _camera(rt, (0.4, 1.5, -5.0), (0.4 if name != "leaves" else 2.0, 0.0, 0.0))
    img, rst = _check_frames(rt, w, cam, 3, ref, fused=False)
    assert ref.csg_ties == 0 and len(np.unique(img.reshape(-1, 3), axis=0)) > 10 and rst["rays_shadow"] > 100


# ---------------------------------------------------------------- the die
def _die_world(rt):
    from rtamd import scenes
    w = _floor_world(rt)
    place = rt.translation(-1.4, 0, 0) * rt.rotation_y(0.5) * rt.rotation_x(0.4)
    m = rt.Material()
    m.color = rt.Color(0.1, 0.1, 0.2)
    m.transparency, m.refractive_index, m.reflective, m.diffuse = 0.9, 1.5, 0.3, 0.2
    w.add_object(scenes.csg_die21(place, m, glass_pips=4))
    m2 = rt.Material()
    m2.color = rt.Color(0.8, 0.25, 0.2)
    w.add_object(scenes.csg_die21(rt.translation(1.4, 0, 0.3) * rt.rotation_y(-0.6) * rt.rotation_z(0.3), m2, node_transform_every=5))
    _lights(rt, w)
    return w, _camera(rt, *DIE_VIEW), 4, (-1.4, 0.0, 0.0)


DIE_VIEW = ((0, 2, -5.5), (0, 0, 0), math.pi / 3)
DIE_RAY_SEED = 3


@pytest.fixture(scope="module")
def die(rt):
    w, cam, depth, centre = _die_world(rt)
    plan = _deep(rt, w, 2)
    assert (plan["leaves"], plan["levels"]) == (22, 21) and plan["nodes"] == 21
    return w, cam, depth, centre, csg_ref.CsgRef.from_world(w)


def test_die_frames(rt, die):
    w, cam, depth, centre, ref = die
    img, rst = _check_frames(rt, w, cam, depth, ref, fused=False)
    assert rst["rays_refract"] >= 100, rst["rays_refract"]


def test_die_as_batches(rt, die):
    w, cam, depth, centre, ref = die
    _as_batches(rt, w, DIE_VIEW, depth, ref, [_camera(rt, (3.0, 2.0, -4.5), (0, 0, 0)), _camera(rt, (-3.5, 3.0, -3.0), (0, 0, 0.2))])


def test_die_rays_from_inside(rt, die):
    """From the glass die's centre: the parity and container rule decide n1 and n2 (a pip behind the origin is the
    container, not the cube it is cut from)."""
    w, cam, depth, centre, ref = die
    rng = np.random.default_rng(DIE_RAY_SEED)
    d = rng.normal(size=(40, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.hstack([np.tile(np.array(centre), (40, 1)), d])
    want = _check_hits(w, ref, rays, 40)
    assert (want[:, 17] == 1.0).sum() >= 30, (want[:, 17] == 1.0).sum()
    assert len(set(want[:, 21]) - {1.0}) >= 2, sorted(set(want[:, 21]))


# ---------------------------------------------------------------- more than one walk
def _row_world(rt, n):
    from rtamd import scenes
    w = _floor_world(rt)
    w.add_object(scenes.csg_row(n))
    _lights(rt, w)
    return w, _camera(rt, (0.02, 0.03, -3), (0, 0, 5), math.pi / 8), 3


def _axis_rays(n=300, seed=7):
    """Rays down the row's axis from about the camera: within 0.02 rad of it, so most pass every sphere."""
    rng = np.random.default_rng(seed)
    o = np.array([0.02, 0.03, -3.0]) + rng.uniform(-0.05, 0.05, size=(n, 3))
    d = np.array([0.0, 0.0, 1.0]) + rng.uniform(-0.02, 0.02, size=(n, 3)) * np.array([1.0, 1.0, 0.0])
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.hstack([o, d])


def test_row_of_70_three_walks(rt):
    """The frame's own rays hold the floors on the roots per ray (253 rays with more than 64 roots and 170 with more
    than 128 here, 140 at the most: three walks); a batch of rays down the axis is shaded as well."""
    w, cam, depth = _row_world(rt, 70)
    plan = _deep(rt, w)
    assert (plan["leaves"], plan["nodes"], plan["levels"]) == (70, 69, 69)
    ref = csg_tri_ref.CsgTriRef.from_world(w)
    ref.keep_roots = True
    img, rst = _check_frames(rt, w, cam, depth, ref, fused=False)
    ref.keep_roots = False
    n = [len(r) for r in ref.unit_roots]
    over = sum(1 for k in n if k > 64), sum(1 for k in n if k > 128)
    assert over[0] >= 200 and over[1] >= 100 and max(n) == 140, (over, max(n))
    assert ref.csg_ties == 0 and rst["rays_refract"] > 100
    rays = _axis_rays()
    ref.counts = dict.fromkeys(csg_ref.COUNTERS, 0)
    colors = ref.color_at_batch(rays, depth)
    for exhaustive in (False, True):
        got, st = w.color_at_batch(rays, depth, True, exhaustive)
        assert np.asarray(got).tobytes() == colors.tobytes(), np.abs(np.asarray(got) - colors).max()
        for k in COUNTS:
            assert st[k] == ref.counts[k], (k, exhaustive, st[k], ref.counts[k])
    assert ref.counts["rays_refract"] > 100


def test_row_of_33_the_narrowest_deep_row(rt):
    w, cam, depth = _row_world(rt, 33)
    plan = _deep(rt, w)
    assert (plan["leaves"], plan["nodes"]) == (33, 32)
    ref = csg_tri_ref.CsgTriRef.from_world(w)
    ref.keep_roots = True
    _check_frames(rt, w, cam, depth, ref, fused=False)
    ref.keep_roots = False
    assert 64 < max(len(r) for r in ref.unit_roots) <= 66 and ref.csg_ties == 0


# ---------------------------------------------------------------- a mesh under many nodes
def _mesh_world(rt):
    from rtamd import scenes
    w = _floor_world(rt)
    m = rt.Material()
    m.color = rt.Color(0.9, 0.5, 0.2)
    m.reflective = 0.2
    ring = scenes._mesh_group(scenes.mesh_torus(6, 4), m, 3)
    cuts = None
    for k in range(36):
        a = 2.0 * math.pi * k / 36.0
        c = rt.Cube()
        c.set_transform(rt.translation(math.cos(a), 0.0, math.sin(a)) * rt.rotation_y(-a) * rt.scaling(0.55, 0.55, 0.03))
        c.material.color = rt.Color(0.2, 0.3 + 0.015 * k, 0.8)
        if k % 4 == 1:
            _glass(c, 1.3 + 0.01 * k)
        cuts = c if cuts is None else rt.Csg(rt.Operation.Union, cuts, c)
    w.add_object(rt.Csg(rt.Operation.Difference, ring, cuts))
    _lights(rt, w)
    return w, _camera(rt, *MESH_VIEW), 3


MESH_VIEW = ((0.3, 2.6, -3.6), (0, 0, 0), math.pi / 3)


@pytest.fixture(scope="module")
def mesh(rt):
    w, cam, depth = _mesh_world(rt)
    plan = _deep(rt, w)
    assert (plan["nodes"], plan["leaves"], plan["levels"]) == (36, 36, 36)  # (35 unions and the difference)
    ref = csg_tri_ref.CsgTriRef.from_world(w)
    assert len(ref.under_csg) == 48  # the ring's triangles
    return w, cam, depth, ref


def test_mesh_under_many_nodes_frames(rt, mesh):
    w, cam, depth, ref = mesh
    img, rst = _check_frames(rt, w, cam, depth, ref, fused=False)
    assert ref.csg_ties == 0 and len(np.unique(img.reshape(-1, 3), axis=0)) > 20


def test_mesh_under_many_nodes_as_batches(rt, mesh):
    w, cam, depth, ref = mesh
    _as_batches(rt, w, MESH_VIEW, depth, ref, [_camera(rt, (2.5, 2.0, -2.5), (0, 0, 0)), _camera(rt, (-0.2, 3.5, -0.4), (0, 0, 0))])


# ---------------------------------------------------------------- ties
def test_flush_cubes_hold_the_stable_order(rt):
    w = _floor_world(rt)
    chain = None
    for k in range(20):
        c = rt.Cube()
        c.set_transform(rt.translation(k - 8, 0, 0) * rt.scaling(0.5, 0.5, 0.5))
        c.material.color = rt.Color(0.9 - 0.03 * k, 0.4, 0.2 + 0.03 * k)
        if k % 2:
            _glass(c, 1.2 + 0.02 * k)
        chain = c if chain is None else rt.Csg(rt.Operation.Union, chain, c)
    w.add_object(chain)
    _lights(rt, w)
    plan = _deep(rt, w)
    assert (plan["leaves"], plan["levels"]) == (20, 19)
    ref = csg_ref.CsgRef.from_world(w)
    _check_frames(rt, w, _camera(rt, (-16, 0.25, -0.125), (0, 0, 0), math.pi / 6), 3, ref, fused=False)
    assert ref.csg_ties >= 1000, ref.csg_ties


# ---------------------------------------------------------------- random
@pytest.mark.parametrize("seed", range(12))
def test_deep_random_scene(rt, seed):
    from rtamd import scenes
    info = []
    w, cam, depth = scenes.csg_deep_random(seed, W, H, info)
    assert depth == 4 and len(info) == 2 and all(5 <= lv <= 12 and 17 <= n <= 60 for lv, n in info), info
    plan = _deep(rt, w, 2)
    assert plan["levels"] == max(lv for lv, _ in info)
    ref = csg_ref.CsgRef.from_world(w)
    img, rst = _check_frames(rt, w, cam, depth, ref, fused=False)
    assert ref.csg_ties == 0 and len(np.unique(img.reshape(-1, 3), axis=0)) > 30 and rst["rays_refract"] > 10


# ---------------------------------------------------------------- the old evaluators against the new
@contextlib.contextmanager
def deep_all(rt):
    try:
        rt._rtamd._tuning_set("csg_deep_all", 1)
        yield
    finally:
        rt._rtamd._tuning_set("csg_deep_all", 0)


def _deep_equals_the_others(rt, make):
    frames = []
    for knob in (False, True):
        w, cam, depth = make()
        if knob:
            with deep_all(rt):
                w.upload()
        else:
            w.upload()
        fast, fst = cam.render(w, depth, True, False)
        exh, est = cam.render(w, depth, True, True)
        deep, units = rt._rtamd._csg_deep_plan(w), rt._rtamd._csg_plan(w)
        assert deep["units"] == (units["units"] if knob else 0) and units["units"] > 0
        if knob:
            assert units["records"] == 0 and units["remainder"] == units["units"]  # none in the hierarchy
        frames.append((fast.to_numpy().tobytes(), {k: fst[k] for k in COUNTS}, exh.to_numpy().tobytes(), {k: est[k] for k in EXACT}))
    assert frames[0] == frames[1]
    assert frames[0][0] == frames[0][2]


@pytest.mark.parametrize("seed", range(6))
def test_deep_evaluator_equals_the_others_on_csg_random(rt, seed):
    from rtamd import scenes
    _deep_equals_the_others(rt, lambda: scenes.csg_random(seed))


@pytest.mark.parametrize("seed", range(4))
def test_deep_evaluator_equals_the_others_on_csg_mesh_random(rt, seed):
    from rtamd import scenes
    _deep_equals_the_others(rt, lambda: scenes.csg_mesh_random(seed))


def test_deep_evaluator_equals_the_others_on_dice(rt):
    from rtamd import scenes
    _deep_equals_the_others(rt, lambda: scenes.csg_dice(4, 48, 27))


def test_deep_evaluator_equals_the_others_on_the_tie_world(rt):
    def make():
        t = tie_worlds.build(rt, "csg")
        return t.w, t.cam, t.depth
    _deep_equals_the_others(rt, make)


# ---------------------------------------------------------------- every kernel of the classes
def test_every_csg_kernel_ran_a_deep_unit(rt, oracle):
    """tests/test_gpu_variants.py's sweep (every scene image, plain, counted, X4 and ray batches, each against the
    exhaustive result and that against the checker) over its three Csg scenes with every unit deep."""
    import test_gpu_variants as tv
    reached = set()
    for name in ("csg", "csg_nodiag", "mixed"):
        with deep_all(rt):
            s = tv._Sweep(rt, oracle, name)
        assert not s.failures, "\n".join(s.failures)
        deep, units = rt._rtamd._csg_deep_plan(s.w), rt._rtamd._csg_plan(s.w)
        assert deep["units"] == units["units"] > 0 and s.csg and s.fused
        reached |= s.reached
    want = {t for t, why in tv.LAUNCH_TABLE.items() if (t[1], t[4], t[5]) == (True, True, True) and why is None}
    assert len(want) == 22 and not (want - reached), sorted(want - reached)


def _alias_deep_world(rt, diag):
    """Both opt-ins: a deep unit (the glass die) beside an alias class. The aliased pair is opaque, so the walk by
    structural equality and the checker's walk by identity agree (no ray is ever inside an opaque shape). `diag`:
    with two diagonal glass spheres (the sphere image is live), else two turned ones (their hierarchy alone opens
    the fused generations: LANE 3 and 1 take the camera rays)."""
    from rtamd import scenes
    w = _floor_world(rt)
    m = rt.Material()
    m.color = rt.Color(0.1, 0.1, 0.2)
    m.transparency, m.refractive_index, m.reflective, m.diffuse = 0.9, 1.5, 0.3, 0.2
    w.add_object(scenes.csg_die21(rt.translation(0, 0, 0) * rt.rotation_y(0.5) * rt.rotation_x(0.4), m, glass_pips=4))
    for _ in range(2):  # the twins
        s = rt.Sphere()
        s.set_transform(rt.translation(2.2, -0.4, 0.5) * rt.scaling(0.6, 0.6, 0.6))
        s.material.color = rt.Color(0.2, 0.8, 0.3)
        w.add_object(s)
    for x in (-2.3, 3.4):
        s = rt.glass_sphere()
        turn = rt.scaling(0.7, 0.7, 0.7) if diag else rt.rotation_z(0.4) * rt.scaling(0.7, 0.6, 0.7)
        s.set_transform(rt.translation(x, -0.3, 1.0) * turn)
        w.add_object(s)
    _lights(rt, w)
    w.upload(aliases=True, deep_csg=True)
    plan = rt._rtamd._wf_plan(w)
    assert (plan["n_alias_members"], plan["n_alias_classes"]) == (2, 1) and rt._rtamd._csg_deep_plan(w)["units"] == 1
    return w


ALIAS_VIEW = ((0.5, 2, -5.5), (0.5, 0, 0), math.pi / 3)


def test_an_alias_class_beside_a_deep_unit(rt):
    w = _alias_deep_world(rt, True)
    ref = csg_ref.CsgRef.from_world(w)
    img, rst = _check_frames(rt, w, _camera(rt, *ALIAS_VIEW), 4, ref)
    _as_batches(rt, w, ALIAS_VIEW, 4, ref, [_camera(rt, (3.0, 2.0, -4.5), (0, 0, 0))])  # (the batch kernels of both classes)
    assert rst["rays_refract"] >= 100


def test_every_alias_kernel_ran_a_deep_unit(rt, oracle):
    """The same for the ALIAS class: tests/test_gpu_variants.py's sweep over the world above, with and without
    diagonal spheres; every fused ALIAS kernel the launch switch can produce (tests/test_gpu_alias.py ALIAS_TABLE)
    ran the deep unit beside the alias class and agrees with the exhaustive result, and that with the checker."""
    import test_gpu_alias as ta
    import test_gpu_variants as tv
    reached = set()
    names = {"alias_deep": True, "alias_deep_nodiag": False}
    new_scenes = tv.NEW_SCENES
    try:
        tv.NEW_SCENES = new_scenes + tuple(names)  # (the checker is their yardstick)
        for name, diag in names.items():
            tv.SCENES[name] = lambda rt_, d=diag: (_alias_deep_world(rt_, d), _camera(rt_, *ALIAS_VIEW, w=tv.W2, h=tv.H2), tv.DEPTH2)
            s = tv._Sweep(rt, oracle, name)
            assert not s.failures, "\n".join(s.failures)
            plan = rt._rtamd._wf_plan(s.w)
            assert plan["n_alias_members"] == 2 and rt._rtamd._csg_deep_plan(s.w)["units"] == 1 and s.fused and s.csg
            assert (s.prof["n_diag"] > 0) == diag
            reached |= {(lane, tally, cam) for lane, quads, tally, cam, tris, csg in s.reached}
    finally:
        tv.NEW_SCENES = new_scenes
        for name in names:
            tv.SCENES.pop(name, None)
    assert not (ta.ALIAS_TABLE - reached), sorted(ta.ALIAS_TABLE - reached)


# ---------------------------------------------------------------- two streams at once
def test_two_streams_render_one_scene_at_once(rt, die):
    """Two asynchronous batches of one scene on two streams: each workspace has its own deep state."""
    import torch
    w, cam, depth, centre, ref = die
    cams = [[cam, _camera(rt, (3.0, 2.0, -4.5), (0, 0, 0))], [_camera(rt, (-3.5, 3.0, -3.0), (0, 0, 0.2)), cam]]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    bufs = [[torch.full((H, W, 3), -1.0, dtype=torch.float64, device="cuda") for _ in cs] for cs in cams]
    torch.cuda.synchronize()
    for _ in range(2):  # (the second round finds both workspaces there)
        for cs, bs, st in zip(cams, bufs, streams):
            rt.render_frames_device(w, cs, depth, 8, 0, 1, [b.data_ptr() for b in bs], st.cuda_stream, False, 1)
    torch.cuda.synchronize()
    w.check()
    for cs, bs in zip(cams, bufs):
        for c, b in zip(cs, bs):
            assert b.cpu().numpy().tobytes() == ref.render(c.desc_bytes(), depth)[0].tobytes()
