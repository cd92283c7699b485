"""Triangles, smooth triangles and OBJ meshes under a Csg on the GPU (wide units: the streamed
evaluator csg_wide_eval), bit for bit against the checker tests/csg_tri_ref.py (pinned by
tests/test_csg_tri_ref.py): frames, hit records and the rt_stats counters; each world on the fast
path (plain and counted) and on the exhaustive path. Worlds: tests/csg_mesh_worlds.py and
rtamd.scenes.csg_mesh_random. Every comparison is made where no Csg node's list holds two equal t
(the checker's csg_ties is asserted 0).

Shapes: 32x24 frames at depth 5 (the fuzz scenes: their own 24x16 at depth 4), meshes of 2 to 96
triangles, 256 rays a world: every path of the evaluator is reached at that size (gates inside the
unit, nesting, a transformed Csg, survivors behind the origin on triangles, shadowless leaves, and
with the deck of 80 triangles more roots than one batch of 64 holds, before and behind the origin)."""
import contextlib

import numpy as np
import pytest

import csg_mesh_worlds as worlds
import csg_ref
import csg_tri_ref

pytestmark = pytest.mark.gpu
COUNTS = ("rays_primary", "rays_reflect", "rays_refract", "rays_shadow", "sphere_tests", "plane_tests", "other_tests")
DEPTH = worlds.DEPTH


def _check_hits(w, ref, rays, min_hits):
    got = w.hit_batch(rays)
    want = ref.hit_batch(rays)
    hits = want[:, 0] >= 0
    assert hits.sum() >= min_hits, hits.sum()
    assert np.array_equal(got[:, 0], want[:, 0])  # the hit object, misses included
    assert got[:, 1:23].tobytes() == want[:, 1:23].tobytes(), np.abs(got[:, 1:23] - want[:, 1:23]).max()
    assert np.abs(got[hits, 23] - want[hits, 23]).max() <= 1e-12  # schlick, as the existing hit tests hold it
    return want


def _check_frames(rt, w, cam, depth, ref, fused=True):
    """The plain fast frame, the counted fast frame and the exhaustive frame against the checker's."""
    img, rst = ref.render(cam.desc_bytes(), depth)
    plain, _ = cam.render(w, depth, False)
    fast, fst = cam.render(w, depth, True, False)
    plan = rt._rtamd._wf_plan(w)
    exh, est = cam.render(w, depth, True, True)
    assert exh.to_numpy().tobytes() == img.tobytes(), np.abs(exh.to_numpy() - img).max()
    assert fast.to_numpy().tobytes() == img.tobytes(), np.abs(fast.to_numpy() - img).max()
    assert plain.to_numpy().tobytes() == img.tobytes()
    for k in COUNTS:
        assert fst[k] == rst[k] and est[k] == rst[k], (k, fst[k], est[k], rst[k])
    assert est["sphere_disc_ge0"] == rst["sphere_disc_ge0"] and est["exhaustive"]
    if fused:  # the fast path ran the fused kernels of the Csg class (launch_fused chooses them by n_csg_units)
        assert not fst["exhaustive"] and plan["n_csg_units"] > 0, plan
        assert max(plan["primary"]["lane"], plan["secondary"]["lane"]) >= 0, plan
    return img, rst


# ---------------------------------------------------------------- 3: the known answers
@pytest.mark.parametrize("op", sorted(worlds.KNOWN_T))
def test_known_answers(rt, op):
    w = worlds.known_answer(rt, op)
    ref = csg_tri_ref.CsgTriRef.from_world(w)
    rays = np.array([worlds.KNOWN_RAY, worlds.KNOWN_INSIDE])
    want = _check_hits(w, ref, rays, 2)
    got = w.hit_batch(rays)
    assert got[0, 0] == (2 if op == "Intersection" else 0) and got[0, 1] == pytest.approx(worlds.KNOWN_T[op][0], abs=1e-9)
    obj, t, n1, n2 = worlds.KNOWN_INSIDE_HIT[op]
    assert got[1, 0] == obj and got[1, 1] == pytest.approx(t, abs=1e-9) and (got[1, 21], got[1, 22]) == (n1, n2)
    assert want[1, 0] == obj and ref.csg_ties == 0
    # ... and the ray through every survivor in turn: from just behind each known t the next one is the hit
    ts = worlds.KNOWN_T[op]
    steps = np.array([[0.1, 0.1, -5.0 + t + 1e-3, 0, 0, 1.0] for t in ts[:-1]])
    got = _check_hits(w, ref, steps, len(steps))
    assert got[:, 1] == pytest.approx([b - a - 1e-3 for a, b in zip(ts, ts[1:])], abs=1e-9)


# ---------------------------------------------------------------- 4: the small worlds
@pytest.fixture(scope="module", params=sorted(worlds.SMALL))
def small(request, rt):
    w, cam, box = worlds.SMALL[request.param](rt)
    return request.param, w, cam, box, csg_tri_ref.CsgTriRef.from_world(w)


def test_small_world_frames_and_counters(rt, small):
    name, w, cam, box, ref = small
    assert len(ref.under_csg) >= 2
    img, rst = _check_frames(rt, w, cam, DEPTH, ref)
    assert ref.csg_ties == 0
    assert img.sum() > 0 and rst["rays_shadow"] > 100 and rst["other_tests"] > 1000
    assert len(np.unique(img.reshape(-1, 3), axis=0)) > 20


def test_small_world_hit_records(rt, small):
    name, w, cam, box, ref = small
    rays = worlds.random_rays(box)
    want = _check_hits(w, ref, rays, 40)
    assert ref.csg_ties == 0
    on_tri = np.isin(want[:, 0], list(ref.under_csg))
    assert on_tri.sum() >= 10, on_tri.sum()  # hits on the triangles under the Csg
    if name == "smooth_nested":
        # the chained u and v differ from those of the world ray through the triangle's inverse alone,
        # and so do the normals: the old recomputation cannot pass
        differ = smooth = 0
        for r, h in zip(rays, want):
            if h[0] < 0 or int(ref.s["kind"][int(h[0])]) != csg_ref.SMOOTH:
                continue
            o, d = tuple(np.float64(x) for x in r[:3]), tuple(np.float64(x) for x in r[3:])
            hit = next(x for x in ref.intersect(o, d) if x[0] >= 0.0)
            j = ref.tri_of[int(h[0])]
            one = lambda cols: tuple(c[j] for c in cols)
            inv = ref.s["inverse"][int(h[0])]
            with np.errstate(all="ignore"):
                _, _, u, v = csg_ref.triangle_solve(one(ref.tp1), one(ref.te1), one(ref.te2), csg_ref.mat_point(inv, o),
                                                    csg_ref.mat_vector(inv, d))
            smooth += 1
            differ += (float(u), float(v)) != (hit[2], hit[3])
        assert smooth >= 10 and differ >= smooth // 2, (smooth, differ)
    if name == "glass_from_inside":
        # survivors behind the origin on triangle leaves: the container before the hit is a triangle
        n1_tri = sum(1 for r, h in zip(rays, want) if h[0] >= 0 and
                     any(x[0] < 0.0 and x[1] in ref.under_csg for x in ref.intersect(r[:3], r[3:])))
        assert n1_tri >= 20 and (want[:, 21] == 1.45).sum() >= 10, n1_tri
    if name == "divided_mesh":
        assert (ref.nodes["kind"] == csg_ref.NODE_GROUP).sum() >= 4  # subgroup gates inside the unit


def test_small_world_shadow_batch(rt, small):
    name, w, cam, box, ref = small
    rng = np.random.default_rng(11)
    lo, hi = np.array(box[0]) - 0.8, np.array(box[1]) + 0.8
    pts = rng.uniform(lo, hi, size=(200, 3))
    got = w.is_shadowed_batch(pts, 0).astype(bool)
    want = np.array([ref.is_shadowed(p, 0) for p in pts])
    assert np.array_equal(got, want) and want.sum() > 5


# ---------------------------------------------------------------- 5: more than one batch
def test_deck_more_roots_than_a_batch(rt):
    w = worlds.deck_minus_sphere(rt)
    ref = csg_tri_ref.CsgTriRef.from_world(w)
    rays = worlds.deck_rays()
    ref.keep_roots = True
    want = _check_hits(w, ref, rays, len(rays) // 2)
    ref.keep_roots = False
    roots = ref.unit_roots
    assert max(len(r) for r in roots) > 64 and max(sum(1 for t in r if t < 0.0) for r in roots) > 64
    assert ref.csg_ties == 0
    assert len(set(want[:, 21])) > 2 and len(set(want[:, 22])) > 2  # containers among the deck's triangles
    # shaded: the children pass through the deck again and again
    ref.counts = dict.fromkeys(csg_ref.COUNTERS, 0)
    colors = ref.color_at_batch(rays, DEPTH)
    for exhaustive in (False, True):
        got, st = w.color_at_batch(rays, DEPTH, True, exhaustive)
        assert np.asarray(got).tobytes() == colors.tobytes(), np.abs(np.asarray(got) - colors).max()
        for k in COUNTS:
            assert st[k] == ref.counts[k], (k, exhaustive, st[k], ref.counts[k])
    assert ref.counts["rays_refract"] > 50 and ref.csg_ties == 0
    # shadow rays from inside the deck
    pts = np.array([[0.3 * (k % 5) - 0.6, 0.2 * (k % 3) - 0.2, 0.05 * k + 0.02] for k in range(0, 80, 2)])
    got = w.is_shadowed_batch(pts, 0).astype(bool)
    assert np.array_equal(got, np.array([ref.is_shadowed(p, 0) for p in pts]))


def test_deck_with_shadowless_triangles(rt):
    """A shadow ray goes on past the survivors whose leaf casts no shadow: here past more than a batch of them."""
    w = rt.World()
    deck = rt.Group()
    for k in range(72):
        t = rt.Triangle(rt.Point(-3.0 - 0.001 * k, 0.05 * k, -2.5), rt.Point(3.0, 0.05 * k, -2.4 - 0.001 * k),
                        rt.Point(0.1, 0.05 * k, 3.0 + 0.001 * k))
        if k != 70:
            t.no_shadow()
        deck.add_child(t)
    ball = rt.Sphere()
    ball.set_transform(rt.translation(4.0, 1.0, 0.0) * rt.scaling(0.3, 0.3, 0.3))
    w.add_object(rt.Csg(rt.Operation.Union, deck, ball))
    w.add_light(rt.PointLight(rt.Point(0.3, 9.0, 0.2), rt.Color(1, 1, 1)))
    ref = csg_tri_ref.CsgTriRef.from_world(w)
    pts = np.array([[0.1, -1.0, 0.1], [0.2, 3.49, -0.1], [0.2, 3.51, -0.1], [0.1, 3.6, 0.3], [2.9, -0.5, 2.9]])
    want = np.array([ref.is_shadowed(p, 0) for p in pts])
    assert list(want) == [True, True, False, False, False]  # only triangle 70 (y = 3.5) casts a shadow
    assert np.array_equal(w.is_shadowed_batch(pts, 0).astype(bool), want)


# ---------------------------------------------------------------- 6: the evaluator alone
@contextlib.contextmanager
def wide_all(rt):
    try:
        rt._rtamd._tuning_set("csg_wide_all", 1)
        yield
    finally:
        rt._rtamd._tuning_set("csg_wide_all", 0)


def _wide_equals_narrow(rt, make):
    frames = []
    for knob in (False, True):
        w, cam, depth = make()
        if knob:
            with wide_all(rt):
                w.upload()
        else:
            w.upload()
        fast, fst = cam.render(w, depth, True, False)
        exh, est = cam.render(w, depth, True, True)
        units = rt._rtamd._csg_plan(w)
        frames.append((fast.to_numpy().tobytes(), {k: fst[k] for k in COUNTS}, exh.to_numpy().tobytes(),
                       {k: est[k] for k in COUNTS + ("sphere_disc_ge0",)}))
        if knob:
            assert units["records"] == 0 and units["remainder"] == units["units"] > 0  # all in the loop
    assert frames[0] == frames[1]
    assert frames[0][0] == frames[0][2] and frames[0][1]["rays_shadow"] > 100


def test_wide_evaluator_equals_narrow_on_dice(rt):
    from rtamd import scenes
    _wide_equals_narrow(rt, lambda: scenes.csg_dice(4, worlds.W, worlds.H))


@pytest.mark.parametrize("seed", range(8))
def test_wide_evaluator_equals_narrow_on_csg_random(rt, seed):
    from rtamd import scenes
    _wide_equals_narrow(rt, lambda: scenes.csg_random(seed))


# ---------------------------------------------------------------- 7: the fuzz scenes
@pytest.mark.parametrize("seed", range(16))
def test_csg_mesh_random(rt, seed):
    from rtamd import scenes
    w, cam, depth = scenes.csg_mesh_random(seed)
    ref = csg_tri_ref.CsgTriRef.from_world(w)
    assert len(ref.under_csg) >= 8
    img, rst = _check_frames(rt, w, cam, depth, ref)
    assert ref.csg_ties == 0 and img.sum() > 0


def test_csg_mesh_random_x4(rt):
    from rtamd import scenes
    w, cam, depth = scenes.csg_mesh_random(1)
    cam.render_opts.aa_samples(rt.AASamples.X4)
    fast, _ = cam.render_multithreaded(w, depth, False)
    exh, _ = cam.render_multithreaded(w, depth, True, True)
    # the checker: rays_for_pixel's X4 offsets (camera.rs:71-126), Color::average (color.rs:26-33)
    ref = csg_tri_ref.CsgTriRef.from_world(w)
    c = np.frombuffer(cam.desc_bytes(), dtype=csg_ref.CAMERA)[0]
    inv = [float(v) for v in c["inverse"]]
    want = np.zeros((int(c["vsize"]), int(c["hsize"]), 3))
    for y in range(want.shape[0]):
        for x in range(want.shape[1]):
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
    assert fast.to_numpy().tobytes() == want.tobytes()


def test_csg_mesh_random_batch_of_cameras(rt):
    import torch
    from rtamd import scenes
    w, cam, depth = scenes.csg_mesh_random(4)
    cams = [cam, worlds.camera(rt, (3.0, 2.0, -5.0), (0, 0, 0.5), 24, 16), worlds.camera(rt, (-4.0, 3.5, -3.0), (0, 0, 0.5), 24, 16)]
    bufs = [torch.full((16, 24, 3), -1.0, dtype=torch.float64, device="cuda") for _ in cams]
    torch.cuda.synchronize()
    rt.render_frames_device(w, cams, depth, 8, 0, 1, [b.data_ptr() for b in bufs], torch.cuda.current_stream().cuda_stream,
                            False, 1)
    torch.cuda.synchronize()
    w.check()
    ref = csg_tri_ref.CsgTriRef.from_world(w)
    for c, b in zip(cams, bufs):
        assert b.cpu().numpy().tobytes() == ref.render(c.desc_bytes(), depth)[0].tobytes()
    assert ref.csg_ties == 0


def test_csg_mesh_random_ray_batch(rt):
    from rtamd import scenes
    w, cam, depth = scenes.csg_mesh_random(5)
    ref = csg_tri_ref.CsgTriRef.from_world(w)
    rng = np.random.default_rng(13)
    o = np.tile([0.0, 1.5, -6.0], (300, 1))
    d = rng.normal([0, -0.25, 1], [0.35, 0.15, 0.05], size=(300, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.hstack([o, d])
    want = ref.color_at_batch(rays, depth)
    for exhaustive in (False, True):
        got, st = w.color_at_batch(rays, depth, True, exhaustive)
        assert np.asarray(got).tobytes() == want.tobytes(), np.abs(np.asarray(got) - want).max()
        for k in COUNTS:
            assert st[k] == ref.counts[k], (k, exhaustive)
    assert ref.csg_ties == 0 and ref.counts["rays_reflect"] > 50


# ---------------------------------------------------------------- 8: the caps
@pytest.mark.parametrize("make,word", [(worlds.too_many_primitives, "RT_CSG_MAX_LEAVES"), (worlds.too_many_nodes, "RT_CSG_MAX_NODES"),
                                       (worlds.too_deep, "RT_CSG_MAX_DEPTH"), (worlds.equal_triangles, "structurally equal"),
                                       (worlds.lone_triangle, "put it in a Group")],
                         ids=["primitives", "nodes", "depth", "equal_triangles", "lone_triangle"])
def test_beyond_the_caps_is_refused(rt, make, word):
    w = rt.World()
    w.add_object(make(rt))
    worlds.lights(rt, w, False)
    with pytest.raises(rt.RtError) as e:
        w.upload()
    assert word in str(e.value), str(e.value)


def test_at_the_caps_creates(rt):
    for make in (worlds.narrow_at_the_caps,                          # today's caps, exactly
                 lambda r: worlds.too_many_primitives(r, 16),          # a wide unit: 16 primitives of kinds 0-4,
                 lambda r: worlds.too_many_nodes(r, 32),               # 32 Csg nodes,
                 lambda r: worlds.too_deep(r, 4)):                     # 4 levels
        w = rt.World()
        w.add_object(make(rt))
        worlds.lights(rt, w, False)
        w.upload()
        cam = worlds.camera(rt, (1.0, 1.0, -6.0), (1.0, 0.2, 0.0), 8, 6)
        exh, _ = cam.render(w, 2, True, True)
        fast, _ = cam.render(w, 2, False)
        assert fast.to_numpy().tobytes() == exh.to_numpy().tobytes()
