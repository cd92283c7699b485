"""The run hierarchies inside wide and deep Csg units on the GPU (rt_bvh.cpp build_csg_run, rt_slab.hpp
csg_run_walk in csg_wide_eval / csg_deep_eval), bit for bit against the checker tests/csg_tri_ref.py: per
world (tests/csg_run_worlds.py) the plain fast frame, the counted fast frame and the exhaustive frame with
the rt_stats counters, color_at_batch fast and exhaustive, hit_batch's records, and the plan readout
_csg_run_plan (runs, triangles boxed, remainder; `ran` after the fast render, not after the exhaustive
one). Every comparison is made where no Csg node's list holds two equal t (the checker's csg_ties is 0).

Shapes: 32x24 frames at depth 5 and 256 hit rays a world; runs of 15 to 96 triangles: the threshold (15, 16,
17), one batch and more than one (the deck's 80 parallel triangles: a second walk from the watermark), a
chain that scales the ray beyond the world's bound, flat axis-aligned triangles with rays in their plane,
roots behind the origin that make containers and that decide shadow rays, a remainder, a deep unit, a
divided mesh without a run, and a caller's rays beyond the runs' bounds."""
import numpy as np
import pytest

import csg_run_worlds as worlds
import csg_tri_ref
import tie_worlds
from test_gpu_csg_hier import creation_knobs
from test_gpu_csg_mesh import COUNTS, _check_frames, _check_hits

pytestmark = pytest.mark.gpu
DEPTH = worlds.DEPTH


def _upload(w, name):
    if name in worlds.DEEP:
        w.upload(deep_csg=True)
    else:
        w.upload()


@pytest.fixture(scope="module", params=sorted(worlds.WORLDS))
def world(request, rt):
    name = request.param
    w, cam, box, fused = worlds.WORLDS[name](rt)
    ref = csg_tri_ref.CsgTriRef.from_world(w)
    _upload(w, name)
    return name, w, cam, box, fused, ref, worlds.expect(w, worlds.REFUSED.get(name, 0), ref)


def _plan_is(rt, w, want, ran):
    plan = rt._rtamd._csg_run_plan(w)
    assert (plan["runs"], plan["boxed"], plan["remainder"]) == (want["runs"], want["boxed"], want["remainder"]), (plan, want)
    assert plan["ran"] == (ran and want["runs"] > 0), plan
    assert (plan["nodes"] > 0 and 0 < plan["depth"] <= 60) if want["runs"] else (plan["nodes"] == 0 and plan["depth"] == 0), plan
    return plan


def test_frames_counters_and_plan(rt, world):
    name, w, cam, box, fused, ref, want = world
    if name == "divided":
        assert want["runs"] == 0 and max(worlds.runs_of(w, ref)) < worlds.RUN_MIN
    elif name == "threshold":
        assert sorted(worlds.runs_of(w, ref)) == [15, 16, 17] and want == dict(runs=2, boxed=33, remainder=0)
    elif name == "with_refused":
        assert want == dict(runs=1, boxed=18, remainder=2)
    else:
        assert want["runs"] == 1 and want["boxed"] >= 20
    img, rst = _check_frames(rt, w, cam, DEPTH, ref, fused=fused)  # (its last render is the exhaustive one)
    _plan_is(rt, w, want, ran=False)
    fast, _ = cam.render(w, DEPTH, False)
    _plan_is(rt, w, want, ran=True)
    assert fast.to_numpy().tobytes() == img.tobytes()
    assert ref.csg_ties == 0
    assert img.sum() > 0 and rst["rays_shadow"] > 100 and rst["other_tests"] > 1000
    assert len(np.unique(img.reshape(-1, 3), axis=0)) > 20


def test_hit_records(rt, world):
    name, w, cam, box, fused, ref, want = world
    rays = worlds.base.random_rays(box)
    assert len(rays) == 256
    got = _check_hits(w, ref, rays, 40)
    assert ref.csg_ties == 0
    assert np.isin(got[:, 0], list(ref.under_csg)).sum() >= 10  # hits on the triangles under the Csg


def test_color_at_batch_fast_and_exhaustive(rt, world):
    name, w, cam, box, fused, ref, want = world
    rays = worlds.base.random_rays(box, n=96, seed=9)
    if name == "flat_grid":
        rays = np.vstack([rays[:32], worlds.grid_plane_rays()])
    if name == "deck_one_run":
        rays = np.vstack([rays[:32], worlds.base.deck_rays()])
    ref.counts = dict.fromkeys(csg_tri_ref.COUNTERS, 0)
    colors = ref.color_at_batch(rays, DEPTH)
    for exhaustive in (False, True):
        got, st = w.color_at_batch(rays, DEPTH, True, exhaustive)
        assert np.asarray(got).tobytes() == colors.tobytes(), (exhaustive, np.abs(np.asarray(got) - colors).max())
        for k in COUNTS:
            assert st[k] == ref.counts[k], (k, exhaustive, st[k], ref.counts[k])
        _plan_is(rt, w, want, ran=not exhaustive)
    assert ref.csg_ties == 0 and ref.counts["rays_shadow"] > 50


def _one(rt, name):
    w, cam, box, fused = worlds.WORLDS[name](rt)
    return w, cam, box, csg_tri_ref.CsgTriRef.from_world(w)


def test_deck_needs_a_second_walk(rt):
    """More than 64 roots on one ray in the run: the second walk's interval starts at the watermark."""
    w, cam, box, ref = _one(rt, "deck_one_run")
    rays = worlds.base.deck_rays()
    ref.keep_roots = True
    ref.hit_batch(rays)
    ref.keep_roots = False
    assert max(len(r) for r in ref.unit_roots) > 64
    w.upload()
    colors = ref.color_at_batch(rays, DEPTH)
    got, _ = w.color_at_batch(rays, DEPTH, False, False)
    assert rt._rtamd._csg_run_plan(w)["ran"]
    assert np.asarray(got).tobytes() == colors.tobytes() and ref.csg_ties == 0


class _NoRootsBehind(csg_tri_ref.CsgTriRef):
    """The checker with every root t < 0 under a Csg left out: what a walk over [0, distance) would see."""

    def _shape(self, i, o, d):
        xs = csg_tri_ref.CsgTriRef._shape(self, i, o, d)
        return [x for x in xs if not x[0] < 0.0] if self.shape_node[i] >= 0 else xs


def test_shadow_rays_that_roots_behind_the_origin_decide(rt):
    """A light inside Difference(closed mesh, sphere): among the shadow rays of the frame's first hits, at least 20
    are blocked only because a root BEHIND their origin set a filter bit: culling a shadow ray's walk to
    [0, distance), as the triangle hierarchy of the world does, would light those points."""
    w, cam, box, ref = _one(rt, "light_inside")
    rays = tie_worlds.pixel_rays(ref, cam)
    want = ref.hit_batch(rays)
    pts = want[want[:, 0] >= 0][:, 5:8]  # the hits' over points
    blind = _NoRootsBehind.from_world(w)
    such = sum(1 for p in pts for light in (0, 1) if ref.is_shadowed(p, light) and not blind.is_shadowed(p, light))
    assert such >= 20, such
    w.upload()
    ref.counts = dict.fromkeys(csg_tri_ref.COUNTERS, 0)
    colors = ref.color_at_batch(rays, 1)  # (one level: the first hits' own shadow rays)
    got, st = w.color_at_batch(rays, 1, True, False)
    assert rt._rtamd._csg_run_plan(w)["ran"]
    assert np.asarray(got).tobytes() == colors.tobytes() and st["rays_shadow"] == ref.counts["rays_shadow"]


def test_callers_rays_beyond_the_bounds_take_the_ops_one_by_one(rt):
    """|d|_inf beyond the run's dmax, origins beyond its omax, a NaN component: the fast color_at_batch gives the
    exhaustive one's bits (such a chained ray falls through to the one-by-one ops)."""
    w, cam, box, ref = _one(rt, "torus_minus_sphere")
    w.upload()
    base = worlds.base.random_rays(box, n=48, seed=21)
    long = base.copy()
    long[:, 3:] *= 1000.0  # (the run sits under no Csg transform: dmax is the world's 2)
    far = base.copy()
    far[:, :3] = far[:, :3] - 1.0e6 * far[:, 3:]  # from a million units back along the same line: beyond omax = 16384
    nan = base[:12].copy()
    nan[np.arange(12), np.arange(12) % 6] = np.nan
    for rays in (base, long, far, nan):
        fast, _ = w.color_at_batch(rays, DEPTH, False, False)
        assert rt._rtamd._csg_run_plan(w)["ran"]
        exh, _ = w.color_at_batch(rays, DEPTH, False, True)
        assert np.asarray(fast).tobytes() == np.asarray(exh).tobytes()
    assert np.abs(np.asarray(w.color_at_batch(far, DEPTH, False, False)[0])).sum() > 0.0  # (the far rays do reach the world)


def test_knob_off_gives_the_same_bytes(rt):
    frames = []
    for off in (False, True):
        w, cam, box, fused = worlds.torus_minus_sphere(rt)
        if off:
            with creation_knobs(rt, csg_run_min=65536):  # above this world's one run of 96: off
                w.upload()
        else:
            w.upload()
        fast, st = cam.render(w, DEPTH, True, False)
        plan = rt._rtamd._csg_run_plan(w)
        assert plan["runs"] == (0 if off else 1) and plan["ran"] == (not off), plan
        frames.append((fast.to_numpy().tobytes(), {k: st[k] for k in COUNTS}))
    assert frames[0] == frames[1]
    # the threshold itself: a run of 96 is held at 96 and not at 97
    for n, runs in ((96, 1), (97, 0)):
        w, cam, box, fused = worlds.torus_minus_sphere(rt)
        with creation_knobs(rt, csg_run_min=n):
            w.upload()
        assert rt._rtamd._csg_run_plan(w)["runs"] == runs


def test_knob_out_of_range_is_refused(rt):
    for bad in (-1, 65537):
        with pytest.raises(rt.RtError):
            rt._rtamd._tuning_set("csg_run_min", bad)
    rt._rtamd._tuning_set("csg_run_min", 0)
