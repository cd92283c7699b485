"""Shading at the edges of the material domain, on the GPU: the cases of tests/test_shading_edges.py through
color_at_batch, hit_batch, render and render_multithreaded.

Every case runs four ways: the fast path, the fast path counting, the exhaustive pipeline, and the fast path with
no shadow ray skipped (tune("skip_shadow", 0)). All four and the checker of tests/csg_ref.py agree bit for bit on
the colours; the counted runs agree with the checker on the counters in COUNTS; hit_batch's n1, n2 and Schlick
columns agree with the checker's hit records bit for bit. The one relaxation: a NaN matches a NaN whatever its sign
and payload (Rust defines neither), and never a number. The fast runs are fused launches (_wf_profile) of the
kernel class the case names (_wf_plan: plain, TRIS, or TRIS, CSG). The conditions each case is named for are held
again on the rays it sends, and the counting fast run leaves out exactly the shadow rays that the checker's events
say shadow_irrelevant may (light behind the surface, no pattern, no -0 or NaN ambient component).
"""
import numpy as np
import pytest

import csg_ref
import test_shading_edges as se
from test_gpu_other_edges import COUNTS

pytestmark = pytest.mark.gpu


def _assert_class(rt, w, klass, st=None):
    assert rt._rtamd._wf_profile(w, -1, True)["fused"]
    plan = rt._rtamd._wf_plan(w)
    # launch_fused (rt_wavefront.hip): the TRIS, CSG kernels where there is a Csg unit, else the TRIS ones where there is a triangle
    ran = "csg" if plan["n_csg_units"] > 0 else "tris" if plan["n_tris"] > 0 else "plain"
    assert ran == klass, plan
    if st is not None:
        assert not st["exhaustive"]


def _four_ways(rt, w, klass, run):
    """run(want_stats, exhaustive) -> (array, stats), the four ways; the fast ones checked to be fused launches."""
    out = {}
    out["fast"] = run(False, False)
    _assert_class(rt, w, klass)
    out["counted"] = run(True, False)
    _assert_class(rt, w, klass, out["counted"][1])
    out["exhaustive"] = run(True, True)
    assert out["exhaustive"][1]["exhaustive"]
    w.tune("skip_shadow", 0)
    try:
        out["every_shadow_ray"] = run(True, False)
        _assert_class(rt, w, klass, out["every_shadow_ray"][1])
    finally:
        w.tune("skip_shadow", 1)
    return out


def _hold(out, want, counts, skipped=None):
    for how, (got, st) in out.items():
        bad = np.flatnonzero([not se.same(g, x) for g, x in zip(got.reshape(-1, 3), want.reshape(-1, 3))])
        assert len(bad) == 0, (how, len(bad), bad[:5], got.reshape(-1, 3)[bad[0]], want.reshape(-1, 3)[bad[0]])
        if how != "fast":
            for k in COUNTS:
                assert st[k] == counts[k], (how, k, st[k], counts[k])
    assert out["every_shadow_ray"][1]["rays_shadow_traced"] == counts["rays_shadow"]
    if skipped is not None:  # shadow_irrelevant left out exactly the shadow rays the checker's events say it may
        traced = out["counted"][1]["rays_shadow_traced"]
        assert traced == counts["rays_shadow"] - skipped, (traced, counts["rays_shadow"], skipped)


@pytest.mark.parametrize("name", sorted(se.CASES))
def test_four_ways_equal_the_checker(rt, name):
    case = se.CASES[name](rt)
    w, rays, depth = case["w"], case["rays"], case["depth"]
    ref = csg_ref.CsgRef.from_world(w)
    want, counts, t = se.check_inputs(case, ref)  # the conditions of the case, on the rays sent
    out = _four_ways(rt, w, case["klass"],
                     lambda stats, exh: (lambda r: (np.asarray(r[0]), r[1]))(w.color_at_batch(rays, depth, stats, exh)))
    # (a counted run of a world with groups or Csg nodes traces every shadow ray: Wavefront::render, rt_wavefront.hip)
    _hold(out, want, counts, t["shadow_skipped"] if len(ref.nodes) == 0 else 0)
    got = np.asarray(w.hit_batch(rays))
    with np.errstate(all="ignore"):
        rec = ref.hit_batch(rays)
    assert np.array_equal(got[:, 0], rec[:, 0])
    for col in (21, 22, 23):
        g, r = got[:, col], rec[:, col]
        assert se.same(g, r), (col, np.flatnonzero(~((g == r) | (np.isnan(g) & np.isnan(r)))))


@pytest.mark.parametrize("name", se.FRAMES)
def test_frames_four_ways_and_x4(rt, name):
    """The tile-ordered generation 0 and wf_combine_parents' per-object reflective / transparency table, through the
    same materials; render_multithreaded X4 against the checker's mean in Color::average's order."""
    case = se.CASES[name](rt)
    w, cam = case["w"], case["cam"]
    img, rst, aa = se.render_checker(csg_ref.CsgRef.from_world(w), cam)
    out = _four_ways(rt, w, case["klass"],
                     lambda stats, exh: (lambda r: (r[0].to_numpy(), r[1]))(cam.render(w, se.FRAME_DEPTH, stats, exh)))
    _hold(out, img, rst)
    cam.render_opts.aa_samples(rt.AASamples.X4)
    try:
        fast, _ = cam.render_multithreaded(w, se.FRAME_DEPTH, False)
        _assert_class(rt, w, case["klass"])
        exh, _ = cam.render_multithreaded(w, se.FRAME_DEPTH, True, True)
    finally:
        cam.render_opts.aa_samples(rt.AASamples.X1)
    for how, got in (("fast", fast.to_numpy()), ("exhaustive", exh.to_numpy())):
        bad = np.flatnonzero([not se.same(g, x) for g, x in zip(got.reshape(-1, 3), aa.reshape(-1, 3))])
        assert len(bad) == 0, (how, len(bad), bad[:5], got.reshape(-1, 3)[bad[0]], aa.reshape(-1, 3)[bad[0]])
