"""The co-resident launch shape (the `coresident` knob, rt_wf_plan.hpp) renders
the frames the usual shape renders, bit for bit.

Image under test: scenes.c3(320, 180), the headline's 1000 spheres at depth 5: the workload's own
LDS image (the four-wide hierarchy, LANE 15), every staged region of which holds more than 960
items of its stage's loop (16-byte units of nodes and sphere records), so a stage that stepped by
1024 with 960 threads would leave a tail that the walks read. Batches of 2 frames through
render_frames_device (the entry point that takes the shape) on 1 and on 4 streams, knob values 0
(off), 1 (blocks of 15 waves, the combine in one-wave blocks of at most 64 registers) and 2 (the
capped kernels, the combine at 32; the default): every frame equals the exhaustive frame and the
knob-0 frame. Scenes whose plan does not run over that image render unchanged and report the usual
shape, as does every single-frame and counted render. No timing here.
"""
import pytest

pytestmark = pytest.mark.gpu
KNOBS = (0, 1, 2)
SHAPE = {0: (1024, 0), 1: (960, 1), 2: (1024, 2)}  # knob -> (threads per block, form) where the plan grants it
W, H = 320, 180


def _settled(w, fn, tries=4):
    """fn() until no asynchronous pass of it outgrew its arenas (a workspace's first passes may: the
    pass is poisoned, reported by check() and the arenas have grown)."""
    import torch
    import rtamd
    for attempt in range(tries):
        try:
            out = fn()
            torch.cuda.synchronize()
            w.check()
            return out
        except rtamd.RtError as e:
            if "overflow" not in str(e) or attempt == tries - 1:
                raise
            torch.cuda.synchronize()


def _batches(rt, w, cam, depth, streams, h, wd):
    """One batch of 2 frames per stream, all in flight together; the frames' bytes, in order."""
    import torch
    bufs = [[torch.full((h, wd, 3), -1.0, dtype=torch.float64, device="cuda") for _ in range(2)] for _ in streams]
    torch.cuda.synchronize()
    for s, b in zip(streams, bufs):
        rt.render_frames_device(w, [cam, cam], depth, 8, 0, 1, [x.data_ptr() for x in b], s.cuda_stream)
    torch.cuda.synchronize()
    return [x.cpu().numpy().tobytes() for b in bufs for x in b]


@pytest.fixture(scope="module")
def streams(rt):
    import torch
    return [torch.cuda.current_stream()] + [rt.render_stream() for _ in range(3)]


@pytest.fixture(scope="module")
def c3(rt):
    """The world, its camera and depth, the exhaustive frame's bytes and reference counters."""
    from rtamd import scenes
    w, cam, depth = scenes.c3(W, H)
    exh, st = cam.render(w, depth, True, True)
    assert st["exhaustive"]
    yield w, cam, depth, exh.to_numpy().tobytes(), st
    w.tune("coresident", 0)


@pytest.fixture(scope="module")
def knob0(rt, c3, streams):
    """The knob-0 frames on 1 and on 4 streams (rendered once, shared)."""
    w, cam, depth, _, _ = c3
    w.tune("coresident", 0)
    return {n: _settled(w, lambda: _batches(rt, w, cam, depth, streams[:n], H, W)) for n in (1, 4)}


def test_staged_regions_are_longer_than_a_block(rt, c3):
    """The premise of the image under test: each region the fused kernel stages (nodes, sphere
    records, distances) holds more than 960 16-byte units."""
    w, cam, depth, _, _ = c3
    cam.render(w, depth, False)
    prof = rt._rtamd._wf_profile(w, -1, True)
    plan = rt._rtamd._wf_plan(w)
    assert plan["secondary"]["lane"] == 15 and plan["primary"]["lane"] == 15, plan
    assert plan["secondary"]["lds_deltas"]
    n_diag, n_wide = int(prof["n_diag"]), int(prof["n_bvh_wide"])
    assert n_diag == 1000
    assert n_wide * 128 // 16 > 960         # the four-wide nodes, 128 B each
    assert n_diag * 48 // 16 > 960          # the 48-B sphere records
    # (the metas, 4 B per sphere, and one light's distances, 2 B per sphere, are staged by loops of
    # their own over words and halfwords: 1000 of each, again more than 960 items)


@pytest.mark.parametrize("n_streams", (1, 4))
@pytest.mark.parametrize("knob", KNOBS)
def test_batches_equal_exhaustive_and_knob0(rt, c3, streams, knob0, knob, n_streams):
    w, cam, depth, exh, _ = c3
    w.tune("coresident", knob)
    try:
        frames = _settled(w, lambda: _batches(rt, w, cam, depth, streams[:n_streams], H, W))
        shape = rt._rtamd._wf_shape(w)
    finally:
        w.tune("coresident", 0)
    assert len(frames) == 2 * n_streams
    for k, f in enumerate(frames):
        assert f == exh, f"knob {knob}, {n_streams} streams: frame {k} differs from the exhaustive frame"
        assert f == knob0[n_streams][k], f"knob {knob}, {n_streams} streams: frame {k} differs from the knob-0 frame"
    for gen in ("primary", "secondary"):
        assert (shape[gen]["threads"], shape[gen]["coresident"]) == SHAPE[knob], (knob, shape)


@pytest.mark.parametrize("knob", KNOBS)
def test_counted_launch_and_single_frames_keep_the_usual_shape(rt, c3, knob):
    """One counted launch per knob value: the reference ray counts equal knob 0's (and the
    exhaustive frame's); a counted or single-frame render never takes the co-resident shape."""
    import torch
    w, cam, depth, exh, ref = c3
    w.tune("coresident", knob)
    try:
        canvas, st = cam.render(w, depth, True, False)
        shape_counted = rt._rtamd._wf_shape(w)
        buf = torch.full((H, W, 3), -1.0, dtype=torch.float64, device="cuda")
        cam.render_shard_device(w, depth, 8, 0, 1, buf.data_ptr(), torch.cuda.current_stream().cuda_stream, False)
        torch.cuda.synchronize()
        w.check()
        shape_single = rt._rtamd._wf_shape(w)
    finally:
        w.tune("coresident", 0)
    assert not st["exhaustive"]
    for k in ("rays_primary", "rays_reflect", "rays_refract", "rays_shadow"):
        assert st[k] == ref[k], (knob, k)
    assert canvas.to_numpy().tobytes() == exh and buf.cpu().numpy().tobytes() == exh
    for shape in (shape_counted, shape_single):
        for gen in ("primary", "secondary"):
            assert (shape[gen]["threads"], shape[gen]["coresident"]) == SHAPE[0], (knob, shape)


# scene, image knobs, the lane the deeper generations run over. The small sphere scene and the zoo
# frame still run over the four-wide LDS image (a small one), so the plan grants them the shape;
# the same scenes over the pair image (LANE 14) or a global-memory image (LANE 4) have no wide LDS
# image and must report the fallback shape.
OTHERS = (("c3-60", {}, 15), ("zoo", {}, 15), ("c3-60", {"lds_wide": 0}, 14), ("c3-60", {"image": 3}, 4),
          ("zoo", {"lds_wide": 0}, 14))


@pytest.mark.parametrize("which,image_knobs,lane", OTHERS, ids=[f"{n}-{'-'.join(k) or 'default'}" for n, k, _ in OTHERS])
def test_other_images_render_unchanged_and_report_the_plan(rt, streams, which, image_knobs, lane):
    """A scene whose launches do not run over the four-wide LDS image renders unchanged under
    every knob value and reports the fallback shape (1024 threads, form 0); one that does
    reports the shape its plan granted."""
    from rtamd import scenes
    (w, cam, depth), wd, h = (scenes.c3(96, 54, 60), 96, 54) if which == "c3-60" else (scenes.zoo(64, 48), 64, 48)
    exh = cam.render(w, depth, True, True)[0].to_numpy().tobytes()
    for k, v in image_knobs.items():
        w.tune(k, v)
    for knob in KNOBS:
        w.tune("coresident", knob)
        frames = _settled(w, lambda: _batches(rt, w, cam, depth, streams[:2], h, wd))
        shape, plan = rt._rtamd._wf_shape(w), rt._rtamd._wf_plan(w)
        for f in frames:
            assert f == exh, f"{which}, knob {knob}: a frame differs from the exhaustive frame"
        for gen in ("primary", "secondary"):
            assert plan[gen]["lane"] == lane, (which, image_knobs, plan)
            want = SHAPE[knob] if lane == 15 and _plain(rt, w, knob) else SHAPE[0]
            assert (shape[gen]["threads"], shape[gen]["coresident"]) == want, (which, knob, gen, shape, plan)


def _plain(rt, w, knob):
    """Form 2 has capped kernels for the plain sphere scenes only (no solids, triangles, Csg, aliases)."""
    if knob != 2:
        return True
    prof = rt._rtamd._wf_profile(w, -1, True)
    plan = rt._rtamd._wf_plan(w)
    return (prof["n_quads"] == 0 and prof["n_obvh_nodes"] == 0 and prof["n_lbvh_nodes"] == 0 and
            plan["n_tris"] == 0 and plan["n_csg_units"] == 0 and plan["n_alias_members"] == 0)
