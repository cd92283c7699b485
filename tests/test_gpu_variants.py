"""Every fast-path kernel variant and every outcome of the LDS plan, on the GPU.

Per generation the fast path launches one instantiation of
wf_trace_fused<PRIMARY, QUADS, LANE, TALLY, CAM, TRIS, CSG> (launch_fused_q in
rt_wavefront.hip, launch_glb_lane in rt_wavefront_glb.hip), 88 in all, in three
classes that launch_fused chooses from the scene:
  TRIS = CSG = false (no triangle, no Csg): 4 for LANE 0 (the wave traversal:
    QUADS x TALLY, always camera rays) and 8 for each of LANE 15, 14, 4, 3 and
    1 (QUADS x TALLY x CAM), 44;
  TRIS (triangles, no Csg): the QUADS kernels with the triangle loop and walk,
    2 for LANE 0 and 4 for each other LANE (TALLY x CAM), 22;
  TRIS, CSG (a Csg node anywhere): the triangle kernels with the Csg units'
    loop, 22 again.
LANE 4, 3 and 1 live in rt_wavefront_glb.o, built with other compiler flags
than the rest. wf_plan_image
(rt_wf_plan.hpp) chooses the LANE and what the block stages in LDS: the
kLdsSpheres / kLdsDeltas flags and a treelet of n_top nodes. `_wf_plan(world)`
reads back the plan that ran, so every case below asserts the lane, the flags
and n_top it was written for and fails if it did not reach them; its n_tris and
n_csg_units are what launch_fused chooses the class by, held to the world's own
records (_tris_csg).

Part 1 (test_variants_*): scenes x knob settings x modes. The scenes: six
rtamd.scenes.fuzz seeds (diagonal ellipsoids, general-transform spheres, cubes,
closed cylinders, open tubes, cones, divided groups, patterns, shadowless
spheres, nested glass, two and three lights, up to three planes), a cluster of
spheres and ellipsoids without any solid (QUADS = false), a scene of solids
only (n_diag = 0: generation 0 of a camera render runs the per-lane kernels
with CAM = true on LANE 3 and 1; it also holds the unbounded cylinder, which
scenes.fuzz never keeps, and enough open cones for the line hierarchy) and a
scene of two planes only (no hierarchy at all, so no fused launch: asserted).
The knob settings are ROWS x shadow_lb x prim_lane; the modes the fast camera
render, the counted fast render, render_multithreaded X4 and color_at_batch on
2000 random rays at depth 0 and at the scene's depth. Every result is bitwise
the exhaustive GPU result of the same call, counters included; once per scene
the exhaustive frame is bitwise the CPU oracle's, with equal counters and PPM
bytes. No tolerance anywhere.

The TRIS and CSG classes run the same variants and modes over five scenes built
here (24x16, depth 3, two lights, 400 batch rays): `mesh` (two diagonal glass
spheres, a divided smooth 72-triangle torus, a loose shadowless triangle, a
cube, a patterned triangle group), `mesh_nodiag` (a floor, a flat torus and a
cone: the triangle hierarchy alone opens the fused generations, so generation 0
runs LANE 3 and 1 with CAM = true), `csg` (test_gpu_csg.py's scene (a) with a
checkers pattern on one leaf of the die), `csg_nodiag` (its scene (b): a
transformed Csg, a Csg in a divided group, grouped spheres only) and `mixed` (a
die, a divided 32-triangle mesh in one group with a second Csg, two diagonal
spheres, a patterned floor, a closed cylinder). The oracle refuses these
worlds; their yardstick is the checker of tests/csg_ref.py (pinned by
tests/test_csg_ref.py): once per scene the exhaustive GPU frame and counters
equal the checker's bit for bit, with csg_ties == 0.

test_every_reachable_kernel_variant_ran shows from the asserted readouts that
the sweep launched every (LANE, QUADS, TALLY, CAM, TRIS, CSG) tuple of
LAUNCH_TABLE that the public calls can reach, class by class.

Part 2 (test_size_*): the plan outcomes that need size, on 64x36 to 64x64
frames. Measured on an MI355X (SIZE_TABLE, asserted by the tests): the plan of
the deeper generations' launch unless the case says primary.

  case                                          lane  staged     n_top of nodes   dyn (B)
  C5 9996 spheres, 2 lights, defaults             4   distances  1183 of 4967     162800
  C5, treelet_deltas=0                            4   -          1808 of 4967     162816
  C5, treelet=0                                   4   distances     0             87088
  C3 3000 spheres, image=3 wide=0                 3   distances  1426 of 2764      97264
  C3 3000, image=3 wide=0 treelet_deltas=0        3   -          1520 of 2764      97280
  C3 3000, image=3 wide=0 shadow_lb=0             3   -          1520 of 2764      97280
  C3 3000, prim_lane=0 (primary)                  0   distances     0 (no sphere records)  6000
  light field 1000 spheres x 16 lights           14   distances     0             146400
  light field 1200 spheres x 16 lights           14   -             0             162240
  light field 1000 spheres x 17 lights        15/14/4/3  no light buffer (lb_res == 0)

The light field's 16 lights: at 800 spheres the four-wide LDS image still fits
beside the distances (LANE 15, 151168 B), from 900 on it does not (LANE 14);
at 1200 the pair image alone takes 162240 B and the distances (38400 B) stay in
global memory; from 1300 on the pair image does not fit either (LANE 4). Both
large C3 trees (seeds 0x5EED0003 and 99) and C5's are 14 to 16 levels deep, so
none lands on LANE 1 by depth (kLaneLdsDepth = 16): LANE 1 runs only through
image=1.
"""
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
PI = math.pi
NTHREADS = max(1, min(16, os.cpu_count() or 1))
# exhaustive GPU render against the oracle (test_gpu_fuzz.py's comparison)
COUNTERS = ("rays_primary", "rays_reflect", "rays_refract", "rays_shadow", "sphere_tests", "plane_tests",
            "sphere_disc_ge0", "other_tests")
# the counted fast path against the exhaustive render (test_gpu_fastpath.py's)
RAY_KEYS = ("rays_primary", "rays_reflect", "rays_refract", "rays_shadow", "sphere_tests", "plane_tests",
            "other_tests")
DEFAULTS = {"image": 0, "treelet": 1, "wide": 1, "lds_wide": 1, "treelet_deltas": 1, "prim_lane": 1, "shadow_lb": 1,
            "own_sphere": 2}
K_FUSED_LDS_LIMIT = 160 * 1024 - 1024  # rt_wf_plan.hpp kFusedLdsLimit
K_LANE_LDS_DEPTH = 16                  # rt_layout.hpp kLaneLdsDepth


def _static_lds(lane):  # rt_wf_plan.hpp lane_static_lds_bytes
    return {3: K_LANE_LDS_DEPTH * 1024 * 4, 0: 16 * 64 * 4}.get(lane, 0)


# ---------------------------------------------------------------- the launch table
# (LANE, QUADS, TALLY, CAM, TRIS, CSG) -> None (reachable) or why no public call reaches it.
CLASSES = ((False, False, False), (True, False, False), (True, True, False), (True, True, True))  # (QUADS, TRIS, CSG)


def _launch_table():
    t = {}
    for quads, tris, csg in CLASSES:  # (launch_fused: TRIS and CSG force QUADS, CSG forces TRIS)
        for tally in (False, True):
            t[(0, quads, tally, True, tris, csg)] = None  # the wave traversal only ever takes camera rays
            for lane in (15, 14, 4, 3, 1):
                for cam in (False, True):
                    # (LANE 3 and 1 with CAM and TRIS or CSG: a scene without diagonal spheres whose fused
                    # generations the triangles' or the grouped spheres' hierarchy opens: mesh_nodiag, csg_nodiag)
                    t[(lane, quads, tally, cam, tris, csg)] = None
    for tally in (False, True):
        for lane in (3, 1):
            t[(lane, False, tally, True, False, False)] = (
                "generation 0 of a camera render takes LANE 3 or 1 only in a scene without diagonal spheres "
                "(with them wf_plan_image sends it to LANE 0: lane_prim needs an LDS or four-wide image); such a "
                "scene is fused only through the other records' or the lines' hierarchy, which sets QUADS")
    return t


LAUNCH_TABLE = _launch_table()
# launch_fused_q: 4 + 2 x 8, launch_glb_lane: 3 x 8 (44); with TRIS 2 + 2 x 4 and 3 x 4 (22); with TRIS, CSG as many
assert len(LAUNCH_TABLE) == 88
assert [sum(1 for t in LAUNCH_TABLE if (t[1], t[4], t[5]) == c) for c in CLASSES] == [22, 22, 22, 22]

# ---------------------------------------------------------------- the knob rows
# name, knobs, lane of the deeper generations, n_top ("wide": n_bvh_wide, "bin": n_bvh_nodes, 0), distances staged
ROWS = (
    ("default", {}, 15, 0, True),
    ("pair", {"lds_wide": 0}, 14, 0, True),
    ("wide16", {"image": 3}, 4, "wide", True),
    ("wide16-no-treelet", {"image": 3, "treelet": 0}, 4, 0, True),
    ("wide16-no-deltas", {"image": 3, "treelet_deltas": 0}, 4, "wide", False),
    ("binary", {"image": 3, "wide": 0}, 3, "bin", True),
    ("binary-no-treelet", {"image": 3, "wide": 0, "treelet": 0}, 3, 0, True),
    ("binary-no-deltas", {"image": 3, "wide": 0, "treelet_deltas": 0}, 3, "bin", False),
    ("scratch", {"image": 1}, 1, 0, True),
)


def _variants():
    for name, knobs, lane, n_top, deltas in ROWS:
        for lb in (1, 0):
            yield f"{name}/lb{lb}", dict(knobs, shadow_lb=lb), lane, n_top, deltas
            if lane in (15, 4):
                yield f"{name}/lb{lb}/prim0", dict(knobs, shadow_lb=lb, prim_lane=0), lane, n_top, deltas


def _tune(w, knobs):
    for k, v in knobs.items():
        w.tune(k, v)


def _restore(w, knobs):
    for k in knobs:
        w.tune(k, DEFAULTS[k])


def _expected(prof, knobs, lane, n_top, deltas, camera):
    """wf_plan_image restated for scenes far below every LDS limit: the plan of
    generation 0 and of the deeper generations, as (lane, n_top, lds_deltas,
    lds_spheres) each."""
    lb = bool(knobs.get("shadow_lb", 1)) and prof["lb_res"] > 0
    if prof["n_diag"] == 0:
        # no sphere hierarchy, so no LDS image and no four-wide nodes: the binary walk's kernels,
        # with nothing to stage; generation 0 is no primary launch (no shared-origin records)
        sec = (1 if knobs.get("image", 0) == 1 else 3, 0, False, False)
        return sec, sec
    nt = {"wide": prof["n_bvh_wide"], "bin": prof["n_bvh_nodes"], 0: 0}[n_top]
    sec = (lane, nt, deltas and lb, False)
    wave = camera and (knobs.get("prim_lane", 1) == 0 or lane not in (15, 14, 4))
    return ((0, 0, lb, True) if wave else sec), sec


# ---------------------------------------------------------------- scenes
DESC = np.dtype([("kind", "i4"), ("casts_shadow", "i4"), ("transform", "f8", 16), ("inverse", "f8", 16),
                 ("color", "f8", 3), ("mat", "f8", 7), ("pattern_kind", "i4"), ("_pad", "i4"),
                 ("pattern_a", "f8", 3), ("pattern_b", "f8", 3), ("pattern_transform", "f8", 16),
                 ("pattern_inverse", "f8", 16), ("minimum", "f8"), ("maximum", "f8"), ("closed", "i4"),
                 ("_pad2", "i4")])  # rt_shape_desc (include/rt_render.h)


def _features(w):
    """What a world holds, from its flattened shape and group records."""
    d = np.frombuffer(w.descs_bytes(), dtype=DESC)
    sg = np.asarray(w.shape_groups())
    inv = d["inverse"].reshape(-1, 4, 4)
    off = np.abs(inv[:, :3, :3] * (1 - np.eye(3))).max(axis=(1, 2)) > 0
    sph = d["kind"] == 0
    diag = sph & ~off & (sg < 0)
    ell = diag & ((inv[:, 0, 0] != inv[:, 1, 1]) | (inv[:, 1, 1] != inv[:, 2, 2]))
    bounded = np.isfinite(d["minimum"]) & np.isfinite(d["maximum"])
    full_glass = sph & (d["mat"][:, 5] == 1.0)  # glass_sphere(): fuzz's shells and cores
    return dict(diag=int(diag.sum()), ellipsoids=int(ell.sum()), general=int((sph & ~diag).sum()),
                planes=int((d["kind"] == 1).sum()), cubes=int((d["kind"] == 2).sum()),
                closed_cyl=int(((d["kind"] == 3) & (d["closed"] != 0)).sum()),
                tubes=int(((d["kind"] == 3) & (d["closed"] == 0) & bounded).sum()),
                cones=int((d["kind"] == 4).sum()), unbounded=int(((d["kind"] >= 3) & ~bounded).sum()),
                groups=len(w.groups_bytes()) // 56, patterns=int((d["pattern_kind"] >= 0).sum()),
                shadowless_spheres=int((sph & (d["casts_shadow"] == 0)).sum()),
                nested_glass=int((full_glass[1:] & full_glass[:-1]).sum()), lights=w.n_lights())


FUZZ_SEEDS = (0, 42, 48, 59, 62, 75)


def _ellipsoid_cluster(rt, n=250, seed=31):
    """_glass_cluster's kind (test_gpu_bvh.py) with what its spheres lack:
    non-uniform scales, shadowless spheres and a second light. No solid and no
    general-transform sphere, so QUADS = false."""
    rng = np.random.default_rng(seed)
    w = rt.World()
    floor = rt.Plane()
    floor.material.reflective = 0.3
    w.add_object(floor)
    for i in range(n):
        s = rt.glass_sphere() if i % 3 == 1 else rt.Sphere()
        r = rng.uniform(0.2, 0.8, 3)
        if i % 2:
            r[:] = r[0]
        c = rng.uniform([-3, 0.8, -3], [3, 3, 3])
        s.set_transform(rt.translation(*c) * rt.scaling(*r))
        s.material.refractive_index = 1.0 + rng.uniform(0, 1.5)
        s.material.reflective = rng.uniform(0, 0.9) if i % 3 else 0.0
        s.material.color = rt.Color(*rng.uniform(0, 1, 3))
        if i % 11 == 5:
            s.no_shadow()
        w.add_object(s)
    w.add_light(rt.PointLight(rt.Point(-10, 10, -10), rt.Color(0.9, 0.9, 0.9)))
    w.add_light(rt.PointLight(rt.Point(6, 7, -8), rt.Color(0.3, 0.35, 0.4)))
    cam = rt.Camera(64, 48, PI / 2.5)
    cam.set_transform(rt.view_transform(rt.Point(0, 2, -8), rt.Point(0, 1.2, 1), rt.Vector(0, 1, 0)))
    return w, cam, 5


def _solids_only(rt, seed=41):
    """No diagonal sphere (n_diag = 0): cubes, closed cylinders and cones and
    rotated spheres behind the other records' hierarchy, 20 open cones and
    tubes behind the lines' hierarchy, an unbounded cylinder and an unbounded
    cone outside both, glass and mirrors among them, two lights."""
    rng = np.random.default_rng(seed)
    w = rt.World()
    floor = rt.Plane()
    floor.material.set_pattern(rt.checkers_pattern(rt.Color(0.9, 0.9, 0.9), rt.Color(0.2, 0.2, 0.3)))
    floor.material.reflective = 0.2
    w.add_object(floor)
    for i in range(44):
        c = rng.uniform([-4, 0.4, -2], [4, 2.8, 6])
        r = rng.uniform(0.25, 0.6, 3)
        kind = i % 5
        if kind == 0:
            s = rt.Cube()
        elif kind == 1:
            s = rt.Cylinder(-1.0, rng.uniform(0.2, 1.0), True)
        elif kind == 2:
            s = rt.Cone(-1.0, rng.uniform(-0.2, 0.8), True)
        elif kind == 3:
            s = rt.Sphere()
        else:  # the lines' records: open, finite bounds
            s = rt.Cone(rng.uniform(-1.0, -0.3), rng.uniform(0.2, 1.0), False) if i % 10 == 4 else \
                rt.Cylinder(rng.uniform(-1.0, 0.0), rng.uniform(0.2, 1.0), False)
        s.set_transform(rt.translation(*c) * rt.rotation_y(rng.uniform(0.1, 3.0)) * rt.rotation_x(rng.uniform(0.1, 3.0))
                        * rt.scaling(*r))
        s.material.color = rt.Color(*rng.uniform(0, 1, 3))
        if i % 4 == 1:
            s.material.transparency = 0.85
            s.material.refractive_index = rng.uniform(1.1, 2.0)
            s.material.reflective = 0.4
            s.material.diffuse = 0.2
        elif i % 4 == 2:
            s.material.reflective = rng.uniform(0.2, 0.9)
        if i % 13 == 7:
            s.no_shadow()
        w.add_object(s)
    for k in range(12):  # more open cones and tubes: past the line hierarchy's threshold of 16 records
        s = rt.Cone(-1.0, rng.uniform(-0.5, 0.0), False) if k % 2 else rt.Cylinder(0.0, rng.uniform(0.5, 1.5), False)
        s.set_transform(rt.translation(*rng.uniform([-4, 0.5, -2], [4, 2.5, 6])) * rt.rotation_z(rng.uniform(-1, 1))
                        * rt.scaling(0.3, rng.uniform(0.4, 0.7), 0.3))
        s.material.color = rt.Color(*rng.uniform(0, 1, 3))
        s.material.reflective = 0.3 if k % 3 == 0 else 0.0
        w.add_object(s)
    pole = rt.Cylinder()
    pole.set_transform(rt.translation(2.4, 0.0, 2.5) * rt.scaling(0.1, 1.0, 0.1))
    pole.material.color = rt.Color(0.6, 0.6, 0.6)
    w.add_object(pole)
    hourglass = rt.Cone()
    hourglass.set_transform(rt.translation(-3.0, 1.5, 5.0) * rt.rotation_z(0.3) * rt.scaling(0.15, 1.0, 0.15))
    hourglass.material.reflective = 0.5
    w.add_object(hourglass)
    w.add_light(rt.PointLight(rt.Point(-6, 8, -8), rt.Color(1.0, 1.0, 1.0)))
    w.add_light(rt.PointLight(rt.Point(5.0, 6.0, -4.0), rt.Color(0.3, 0.3, 0.3)))
    cam = rt.Camera(64, 48, PI / 3.0)
    cam.set_transform(rt.view_transform(rt.Point(0.0, 2.5, -7.5), rt.Point(0, 1.2, 1), rt.Vector(0, 1, 0)))
    return w, cam, 4


def _two_planes(rt):
    w = rt.World()
    floor = rt.Plane()
    floor.material.set_pattern(rt.checkers_pattern(rt.Color(0.9, 0.9, 0.9), rt.Color(0.1, 0.3, 0.2)))
    floor.material.reflective = 0.4
    w.add_object(floor)
    back = rt.Plane()
    back.set_transform(rt.translation(0, 0, 6) * rt.rotation_x(PI / 2.0))
    back.material.color = rt.Color(0.6, 0.7, 0.9)
    back.material.reflective = 0.5
    w.add_object(back)
    w.add_light(rt.PointLight(rt.Point(-6, 8, -8), rt.Color(1.0, 1.0, 1.0)))
    w.add_light(rt.PointLight(rt.Point(5.0, 6.0, -4.0), rt.Color(0.3, 0.3, 0.3)))
    cam = rt.Camera(64, 48, PI / 3.0)
    cam.set_transform(rt.view_transform(rt.Point(0.0, 2.0, -6.0), rt.Point(0, 1, 0), rt.Vector(0, 1, 0)))
    return w, cam, 3


def _light_field(rt, n, n_lights, seed=53):
    """n uniform and ellipsoid spheres over a floor under a ring of lights."""
    rng = np.random.default_rng(seed)
    w = rt.World()
    floor = rt.Plane()
    floor.material.reflective = 0.2
    w.add_object(floor)
    for i in range(n):
        s = rt.glass_sphere() if i % 5 == 2 else rt.Sphere()
        r = rng.uniform(0.15, 0.5, 3)
        if i % 2:
            r[:] = r[0]
        c = rng.uniform([-8, 0.5, -2], [8, 3.5, 14])
        s.set_transform(rt.translation(*c) * rt.scaling(*r))
        s.material.color = rt.Color(*rng.uniform(0.1, 1, 3))
        s.material.reflective = 0.6 if i % 5 == 1 else 0.0
        w.add_object(s)
    for k in range(n_lights):
        a = 2 * PI * k / n_lights
        w.add_light(rt.PointLight(rt.Point(14 * math.cos(a), 9 + 0.25 * k, 6 + 14 * math.sin(a)),
                                  rt.Color(*(rng.uniform(0.5, 1.0, 3) / n_lights * 2.0))))
    cam = rt.Camera(64, 36, PI / 3.0)
    cam.set_transform(rt.view_transform(rt.Point(0, 3, -11), rt.Point(0, 1, 5), rt.Vector(0, 1, 0)))
    return w, cam, 2


# ---- the scenes of the TRIS and CSG classes: 24x16, depth 3, two lights (one off the camera's axis)
W2, H2, DEPTH2 = 24, 16, 3


def _two_lights(rt, w):
    w.add_light(rt.PointLight(rt.Point(-6, 8, -8), rt.Color(1, 1, 1)))
    w.add_light(rt.PointLight(rt.Point(5, 6, -4), rt.Color(0.35, 0.35, 0.35)))


def _camera2(rt, frm=(0.0, 2.0, -6.0), to=(0.0, 0.6, 0.0)):
    cam = rt.Camera(W2, H2, PI / 3)
    cam.set_transform(rt.view_transform(rt.Point(*frm), rt.Point(*to), rt.Vector(0, 1, 0)))
    return cam


def _diag_spheres(rt, w, xs=(-2.1, 2.1)):
    """Two diagonal glass spheres: what makes test_gpu_csg.py's scene (a) reach all five images."""
    for x, idx in zip(xs, (1.5, 1.33)):
        s = rt.glass_sphere()
        s.set_transform(rt.translation(x, 0.7, 0.4) * rt.scaling(0.7, 0.7, 0.7))
        s.material.refractive_index = idx
        s.material.reflective = 0.4
        w.add_object(s)


def _torus(rt, n, smooth, place, transparent=False):
    """scenes.mesh_torus(n, n) as one group (2 n n triangles), divided, then rotated and scaled non-uniformly."""
    from rtamd import scenes
    g = rt.parse_obj_string(scenes.mesh_torus(n, n, smooth)).as_group()
    m = rt.Material()
    m.color = rt.Color(0.9, 0.45, 0.2)
    m.reflective = 0.15
    if transparent:
        m.transparency = 0.3
        m.refractive_index = 1.3
    g.set_material(m)
    g.divide(4)
    g.set_transform(place * rt.rotation_x(0.6) * rt.rotation_z(0.3) * rt.scaling(1.2, 0.9, 1.0))
    return g


def _floor(rt, patterned=False):
    floor = rt.Plane()
    floor.material.reflective = 0.3
    floor.material.color = rt.Color(0.8, 0.8, 0.7)
    if patterned:
        p = rt.ring_pattern(rt.Color(0.8, 0.8, 0.7), rt.Color(0.3, 0.4, 0.5))
        p.set_transform(rt.translation(0.2, 0.0, 0.3) * rt.scaling(0.8, 1.0, 0.6))
        floor.material.set_pattern(p)
    return floor


def _die(rt, place, color, patterned):
    """scenes.csg_die's tree, (cube & sphere) - (three cylinders), with a checkers pattern on the cube leaf."""
    m = rt.Material()
    m.color = rt.Color(*color)
    m.reflective = 0.2
    cube = rt.Cube()
    cube.set_transform(place)
    cube.set_material(m)
    if patterned:
        p = rt.checkers_pattern(rt.Color(0.9, 0.9, 0.9), rt.Color(0.2, 0.1, 0.5))
        p.set_transform(rt.scaling(0.5, 0.5, 0.5))
        cube.material.set_pattern(p)
    ball = rt.Sphere()
    ball.set_transform(place * rt.scaling(1.38, 1.38, 1.38))
    ball.set_material(m)
    body = rt.Csg(rt.Operation.Intersection, cube, ball)
    drills = []
    for turn in (rt.rotation_z(PI / 2.0), None, rt.rotation_x(PI / 2.0)):
        c = rt.Cylinder(-1.5, 1.5, True)
        c.set_transform((place * turn if turn is not None else place) * rt.scaling(0.35, 1.0, 0.35))
        c.set_material(m)
        drills.append(c)
    holes = rt.Csg(rt.Operation.Union, drills[0], rt.Csg(rt.Operation.Union, drills[1], drills[2]))
    return rt.Csg(rt.Operation.Difference, body, holes)


def _mesh(rt):
    w = rt.World()
    w.add_object(_floor(rt))
    _diag_spheres(rt, w)
    w.add_object(_torus(rt, 6, True, rt.translation(0.0, 1.1, 0.0), transparent=True))
    fin = rt.Triangle(rt.Point(-2.6, 0.0, -0.5), rt.Point(-1.6, 0.0, -1.4), rt.Point(-2.0, 1.8, -0.8))
    fin.material.color = rt.Color(0.2, 0.6, 0.9)
    fin.no_shadow()
    w.add_object(fin)
    cube = rt.Cube()
    cube.set_transform(rt.translation(1.3, 0.4, -1.6) * rt.rotation_y(0.5) * rt.scaling(0.4, 0.4, 0.4))
    cube.material.color = rt.Color(0.3, 0.8, 0.3)
    cube.material.reflective = 0.3
    w.add_object(cube)
    g = rt.Group()  # a patterned triangle group: a flat and a smooth triangle under one striped material
    g.add_child(rt.Triangle(rt.Point(-1.2, 0.0, -2.0), rt.Point(-0.2, 0.0, -2.2), rt.Point(-0.7, 1.0, -1.9)))
    g.add_child(rt.SmoothTriangle(rt.Point(-0.2, 0.0, -2.2), rt.Point(0.6, 0.0, -1.8), rt.Point(0.2, 0.9, -2.0),
                                  rt.Vector(-0.3, 0.1, -1.0), rt.Vector(0.3, 0.1, -1.0), rt.Vector(0.0, 0.5, -1.0)))
    m = rt.Material()
    p = rt.stripe_pattern(rt.Color(0.9, 0.9, 0.2), rt.Color(0.2, 0.2, 0.9))
    p.set_transform(rt.rotation_z(0.5) * rt.scaling(0.15, 0.15, 0.15))
    m.set_pattern(p)
    g.set_material(m)
    w.add_object(g)
    _two_lights(rt, w)
    return w, _camera2(rt), DEPTH2


def _mesh_nodiag(rt):
    w = rt.World()
    w.add_object(_floor(rt))
    w.add_object(_torus(rt, 6, False, rt.translation(-0.3, 1.1, 0.0)))
    cone = rt.Cone()  # unbounded: outside every hierarchy, so the triangles' is the only one
    cone.set_transform(rt.translation(2.2, 1.2, 0.3) * rt.rotation_z(0.3) * rt.scaling(0.15, 1.0, 0.15))
    cone.material.color = rt.Color(0.2, 0.5, 0.9)
    cone.material.reflective = 0.4
    w.add_object(cone)
    _two_lights(rt, w)
    return w, _camera2(rt), DEPTH2


def _csg(rt):
    w = rt.World()
    w.add_object(_floor(rt))
    w.add_object(_die(rt, rt.translation(0.0, 0.8, 0.0) * rt.rotation_y(0.6) * rt.scaling(0.8, 0.8, 0.8), (0.9, 0.3, 0.2), True))
    _diag_spheres(rt, w)
    _two_lights(rt, w)
    return w, _camera2(rt, to=(0.0, 0.5, 0.0)), DEPTH2


def _csg_nodiag(rt):
    import test_gpu_csg
    w, _, _ = test_gpu_csg._scene_b(rt)  # a transformed Csg, a Csg in a divided group, a group in a Csg; two lights
    return w, _camera2(rt, (0.0, 2.5, -7.0), (0.0, 0.5, 0.0)), DEPTH2


def _mixed(rt):
    w = rt.World()
    w.add_object(_floor(rt, patterned=True))
    w.add_object(_die(rt, rt.translation(-1.9, 0.7, -0.6) * rt.rotation_y(0.4) * rt.scaling(0.6, 0.6, 0.6), (0.9, 0.3, 0.2), False))
    g = rt.Group()  # a divided 32-triangle mesh in one group with a second Csg
    g.add_child(_torus(rt, 4, True, rt.translation(0.2, 1.2, 0.4), transparent=True))
    a = rt.Sphere()
    a.set_transform(rt.translation(1.4, 0.6, -0.9) * rt.scaling(0.6, 0.6, 0.6))
    a.material.color = rt.Color(0.2, 0.8, 0.3)
    b = rt.Cube()
    b.set_transform(rt.translation(1.7, 0.8, -1.1) * rt.rotation_y(0.3) * rt.scaling(0.4, 0.4, 0.4))
    b.material.transparency = 0.8
    b.material.refractive_index = 1.4
    b.material.reflective = 0.3
    g.add_child(rt.Csg(rt.Operation.Difference, a, b))
    w.add_object(g)
    _diag_spheres(rt, w, xs=(-0.4, 2.9))
    can = rt.Cylinder(0.0, 1.0, True)
    can.set_transform(rt.translation(-3.2, 0.0, 1.2) * rt.scaling(0.5, 1.3, 0.5))
    can.material.color = rt.Color(0.7, 0.7, 0.2)
    can.material.reflective = 0.3
    w.add_object(can)
    _two_lights(rt, w)
    return w, _camera2(rt, (0.0, 2.4, -6.5)), DEPTH2


NEW_SCENES = ("mesh", "mesh_nodiag", "csg", "csg_nodiag", "mixed")  # the checker of tests/csg_ref.py is their yardstick
SCENES = {f"fuzz{s}": s for s in FUZZ_SEEDS}
SCENES.update(cluster=_ellipsoid_cluster, solids=_solids_only, planes=_two_planes)
SCENES.update(mesh=_mesh, mesh_nodiag=_mesh_nodiag, csg=_csg, csg_nodiag=_csg_nodiag, mixed=_mixed)
# What the profile must show of each scene: n_quads, n_other_culled, n_line_culled, n_gen, n_lights, n_planes
# (the fuzz generator makes at most 13 solids, below the line hierarchy's 16 records: n_line_culled
# is 0 there, and it replaces every unbounded cylinder or cone; `solids` has both).
SCENE_PROFILE = {
    "fuzz0": dict(n_other_culled=34, n_quads=2, n_gen=33, n_lights=3, n_planes=3),
    "fuzz42": dict(n_other_culled=56, n_quads=9, n_gen=50, n_lights=2, n_planes=2),
    "fuzz48": dict(n_other_culled=57, n_quads=8, n_gen=52, n_lights=3, n_planes=3),
    "fuzz59": dict(n_quads=0, n_gen=7, n_lights=2, n_planes=2, n_other_culled=0),
    "fuzz62": dict(n_other_culled=58, n_quads=13, n_gen=52, n_lights=2, n_planes=1),
    "fuzz75": dict(n_other_culled=59, n_quads=12, n_gen=54, n_lights=3, n_planes=3),
    "cluster": dict(n_quads=0, n_lights=2, n_planes=1, n_gen=0, n_other_culled=0, n_line_culled=0, n_diag=250),
    "solids": dict(n_lights=2, n_planes=1, n_diag=0),
    "planes": dict(n_quads=0, n_lights=2, n_planes=2, n_diag=0, n_gen=0),
    "mesh": dict(n_lights=2, n_planes=1, n_diag=2, n_gen=0, n_quads=1, n_bvh_nodes=1, n_obvh_nodes=0, n_lbvh_nodes=0),
    # (no hierarchy but the triangles': theirs alone opens the fused generations)
    "mesh_nodiag": dict(n_lights=2, n_planes=1, n_diag=0, n_gen=0, n_quads=1, n_bvh_nodes=0, n_obvh_nodes=0, n_lbvh_nodes=0),
    "csg": dict(n_lights=2, n_planes=1, n_diag=2, n_gen=0, n_quads=0, n_bvh_nodes=1),
    # (the four grouped spheres' hierarchy opens the fused generations)
    "csg_nodiag": dict(n_lights=2, n_planes=1, n_diag=0, n_gen=4, n_other_culled=4, n_bvh_nodes=0, n_obvh_nodes=1),
    "mixed": dict(n_lights=2, n_planes=1, n_diag=2, n_gen=0, n_quads=1, n_bvh_nodes=1),
}


def _prof(rt, w):
    return rt._rtamd._wf_profile(w, -1, True)


def _quads(prof):
    """launch_fused's QUADS: solids outside the hierarchies, or either of the
    other hierarchies. A solid is in one of the two or outside both, so any
    solid sets it; without solids only 16 general spheres (n_obvh) do."""
    return prof["n_quads"] > 0 or prof["n_obvh_nodes"] > 0 or prof["n_lbvh_nodes"] > 0


def _tris_csg(w):
    """launch_fused's TRIS and CSG restated from the world's own records: CSG, the world
    holds a Csg node; TRIS, it holds triangles and no Csg."""
    import csg_ref
    csg = bool((np.frombuffer(w.nodes_bytes(), dtype=csg_ref.NODE)["kind"] == csg_ref.NODE_CSG).any())
    tris = len(w.triangles_bytes()) > 0 and not csg
    return tris or csg, csg  # (the Csg kernels are triangle kernels: wf_trace_fused<.., TRIS = true, CSG = true>)


def _rays(seed, n=2000):
    rng = np.random.default_rng(seed)
    o = rng.uniform([-4.5, -0.2, -2.5], [4.5, 3.5, 6.5], size=(n, 3))  # test_gpu_fuzz.py's volume: many inside shapes
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.hstack([o, d])


class _Sweep:
    """One scene through every variant and mode; the failures as text, the
    (LANE, QUADS, TALLY, CAM, TRIS, CSG) tuples the asserted readouts show were launched."""

    def __init__(self, rt, oracle, name):
        from rtamd import scenes
        self.rt, self.name = rt, name
        self.failures, self.reached = [], set()
        mk = SCENES[name]
        self.w, self.cam, self.depth = scenes.fuzz(mk, 64, 48) if isinstance(mk, int) else mk(rt)
        w, cam, depth = self.w, self.cam, self.depth
        # the references, once: the exhaustive results of each call, and the oracle's frame
        exh, self.st = cam.render(w, depth)
        self.frame = exh.to_numpy()
        self.prof = _prof(rt, w)
        self.tris, self.csg = _tris_csg(w)
        self.tri_plan = rt._rtamd._wf_plan(w)["triangles"]  # (of the scene: the hierarchy's records, depth, nodes)
        self.quads = _quads(self.prof) or self.tris  # (TRIS and CSG force QUADS)
        self.check(self.prof["bvh_depth"] <= K_LANE_LDS_DEPTH, "a tree too deep for LANE 3")  # (else LANE 1)
        if name in NEW_SCENES:  # the oracle refuses triangles and Csg
            import csg_ref
            checker = csg_ref.CsgRef.from_world(w)
            ref, rst = checker.render(cam.desc_bytes(), depth)
            self.check(checker.csg_ties == 0, f"{checker.csg_ties} equal-t pairs in a Csg node's list")
            self.check(self.tris, "neither a triangle nor a Csg")
        else:
            ref, rst = oracle.OracleWorld.from_world(w).render(cam.desc_bytes(), depth, nthreads=NTHREADS)
            self.check(not self.tris and not self.csg, "a triangle or a Csg")
        self.check(np.isfinite(self.frame).all(), "exhaustive frame not finite")
        self.check(self.frame.tobytes() == ref.tobytes(), f"exhaustive != oracle in {int((self.frame != ref).sum())} channels")
        self.check(rt.canvas_to_ppm(self.frame) == oracle.canvas_to_ppm(ref), "PPM bytes differ from the oracle's")
        for k in COUNTERS:
            self.check(self.st[k] == rst[k], f"oracle counter {k}: {self.st[k]} != {rst[k]}")
        self.aa_cam = (scenes.fuzz(mk, 64, 48) if isinstance(mk, int) else mk(rt))[1]
        self.aa_cam.render_opts.aa_samples(rt.AASamples.X4)
        self.frame4 = self.aa_cam.render_multithreaded(w, depth)[0].to_numpy().tobytes()
        self.rays = _rays(len(name) + 7 * depth, 400 if name in NEW_SCENES else 2000)
        self.batch0 = w.color_at_batch(self.rays, 0, True, True)
        self.batch = w.color_at_batch(self.rays, depth, True, True)
        self.frame = self.frame.tobytes()
        self.fused = self.prof["n_bvh_nodes"] > 0 or self.prof["n_obvh_nodes"] > 0 or self.prof["n_lbvh_nodes"] > 0 or \
            self.tri_plan["nodes"] > 0
        for vname, knobs, lane, n_top, deltas in _variants():
            try:
                _tune(w, knobs)
                self.variant(vname, knobs, lane, n_top, deltas)
            finally:
                _restore(w, knobs)
        w.check()

    def check(self, ok, what):
        if not ok and len(self.failures) < 20:
            self.failures.append(f"{self.name}: {what}")

    def plan(self, what, knobs, lane, n_top, deltas, camera, tally, deeper):
        """Asserts the plan readout of the render just made and records its launches."""
        p = self.rt._rtamd._wf_plan(self.w)
        # what launch_fused chooses the class by, against the world's own records
        self.check((p["n_csg_units"] > 0) == self.csg and (p["n_tris"] > 0 or self.csg) == self.tris,
                   f"{what}: n_tris {p['n_tris']}, n_csg_units {p['n_csg_units']} for TRIS {self.tris} CSG {self.csg}")
        self.check(p["triangles"]["ran"] == (self.fused and self.tri_plan["nodes"] > 0), f"{what}: triangles {p['triangles']}")
        if not self.fused:
            self.check(p["primary"]["lane"] == -1 and p["secondary"]["lane"] == -1, f"{what}: a fused launch {p}")
            return
        want = _expected(self.prof, knobs, lane, n_top, deltas, camera)
        for which, (wl, wt, wd, ws), cam_rays in (("primary", want[0], camera), ("secondary", want[1], False)):
            got = p[which]
            if which == "secondary" and not deeper:
                self.check(got["lane"] == -1, f"{what}: a deeper launch at depth 0: {got}")
                continue
            ok = (got["lane"], got["n_top"], got["lds_deltas"], got["lds_spheres"]) == (wl, wt, wd, ws)
            ok = ok and got["dyn"] + _static_lds(wl) <= K_FUSED_LDS_LIMIT and (got["dyn"] > 0 or wl in (3, 1))
            self.check(ok, f"{what}: {which} plan {got}, expected lane {wl} n_top {wt} deltas {wd} spheres {ws}")
            if ok:
                self.reached.add((wl, self.quads, tally, cam_rays or wl == 0, self.tris, self.csg))

    def variant(self, vname, knobs, lane, n_top, deltas):
        w, cam, depth = self.w, self.cam, self.depth
        args = (knobs, lane, n_top, deltas)
        fast, _ = cam.render(w, depth, want_stats=False)
        self.plan(f"{vname} render", *args, camera=True, tally=False, deeper=depth > 0)
        self.check(fast.to_numpy().tobytes() == self.frame, f"{vname}: fast frame != exhaustive")
        cnt, st = cam.render(w, depth, want_stats=True, exhaustive=False)
        self.plan(f"{vname} counted render", *args, camera=True, tally=True, deeper=depth > 0)
        self.check(cnt.to_numpy().tobytes() == self.frame, f"{vname}: counted fast frame != exhaustive")
        for k in RAY_KEYS:
            self.check(st[k] == self.st[k], f"{vname}: counted fast render {k}: {st[k]} != {self.st[k]}")
        aa, _ = self.aa_cam.render_multithreaded(w, depth, want_stats=False)
        self.plan(f"{vname} X4", *args, camera=True, tally=False, deeper=depth > 0)
        self.check(aa.to_numpy().tobytes() == self.frame4, f"{vname}: X4 frame != exhaustive X4")
        for d, ref in ((0, self.batch0), (depth, self.batch)):
            col, _ = w.color_at_batch(self.rays, d, False, False)
            self.plan(f"{vname} batch depth {d}", *args, camera=False, tally=False, deeper=d > 0)
            self.check(col.tobytes() == ref[0].tobytes(), f"{vname}: batch depth {d} != exhaustive")
        col, st = w.color_at_batch(self.rays, depth, True, False)
        self.plan(f"{vname} counted batch", *args, camera=False, tally=True, deeper=depth > 0)
        self.check(col.tobytes() == self.batch[0].tobytes(), f"{vname}: counted batch != exhaustive")
        for k in RAY_KEYS:
            self.check(st[k] == self.batch[1][k], f"{vname}: counted batch {k}: {st[k]} != {self.batch[1][k]}")


@pytest.fixture(scope="module")
def sweep(rt, oracle):
    done = {}

    def run(name):
        if name not in done:
            done[name] = _Sweep(rt, oracle, name)
        return done[name]
    return run


@pytest.mark.parametrize("name", sorted(SCENES))
def test_variants_bitwise(sweep, name):
    """Every variant x mode of one scene equals the exhaustive result of the
    same call bit for bit, with the plan readout each variant was written for;
    the exhaustive frame equals the oracle's."""
    s = sweep(name)
    assert not s.failures, "\n".join(s.failures)
    for k, v in SCENE_PROFILE[name].items():
        assert s.prof[k] == v, (name, k, s.prof[k])
    if name == "planes":  # no hierarchy of any kind: the generation pipeline, no fused launch
        assert not s.fused and not s.reached
        return
    assert s.fused and s.prof["n_lights"] >= 2 and s.depth >= 3
    if name in NEW_SCENES:
        assert (s.tris, s.csg) == {"mesh": (True, False), "mesh_nodiag": (True, False)}.get(name, (True, True))
        assert (s.cam.hsize, s.cam.vsize, s.depth, len(s.rays)) == (W2, H2, DEPTH2, 400)
        n_tri = len(s.w.triangles_bytes()) // 144
        assert n_tri == {"mesh": 75, "mesh_nodiag": 72, "mixed": 32}.get(name, 0)
        # every mesh: at least 16 boxed triangles, so the walk (tri_trace) ran, not the remainder's loop
        assert s.tri_plan["records"] == n_tri and (n_tri == 0 or (s.tri_plan["nodes"] > 0 and 0 < s.tri_plan["depth"] <= 60))
        assert s.st["rays_reflect"] > 20 and s.st["rays_refract"] > (-1 if name == "mesh_nodiag" else 20)
        assert s.st["other_tests"] > 0 and _features(s.w)["patterns"] == {"mesh": 2, "csg": 1, "mixed": 1}.get(name, 0)
    elif name == "solids":
        assert s.quads and s.prof["n_other_culled"] >= 16 and s.prof["n_line_culled"] >= 16
        assert s.prof["n_quads"] > s.prof["n_other_culled"] + s.prof["n_line_culled"] - s.prof["n_gen"]  # unbounded ones
        f = _features(s.w)
        assert f["unbounded"] == 2 and f["diag"] == 0 and f["general"] > 0
    elif name == "cluster":
        assert not s.quads
        f = _features(s.w)
        assert f["ellipsoids"] > 100 and f["shadowless_spheres"] > 10
    else:
        assert s.prof["n_diag"] > 0 and s.prof["n_gen"] > 0 and s.prof["n_line_culled"] == 0
        assert s.quads == (name != "fuzz59")  # 7 general spheres and no solid: no other hierarchy


@pytest.mark.parametrize("seed", [0, 62])
def test_counted_group_gates_behind_own_sphere(rt, seed):
    """Regression (found by the sweep above on fuzz seeds 0, 42, 48 and 62): a
    shadow ray from inside a sphere record that this sphere answers
    (own_sphere >= 1, shadow_trace's `first`) ended before the loop over the
    records outside the hierarchies, so a counted fast render did not subtract
    the grouped solids that the ray's group boxes would have kept out:
    other_tests came out too high (seed 0: 35408 for the reference's 33222).
    The frame was never affected."""
    from rtamd import scenes
    w, cam, depth = scenes.fuzz(seed, 64, 48)
    exact, se = cam.render(w, depth)
    for own in (0, 1, 2):
        w.tune("own_sphere", own)
        try:
            fast, sf = cam.render(w, depth, want_stats=True, exhaustive=False)
        finally:
            w.tune("own_sphere", DEFAULTS["own_sphere"])
        assert fast.to_numpy().tobytes() == exact.to_numpy().tobytes()
        for k in RAY_KEYS:
            assert sf[k] == se[k], (own, k, sf[k], se[k])


def test_fuzz_seeds_hold_every_feature(rt):
    """The chosen seeds together hold what the sweep is meant to cross with
    every image (read from the worlds' own records)."""
    from rtamd import scenes
    tot = {}
    for seed in FUZZ_SEEDS:
        f = _features(scenes.fuzz(seed, 64, 48)[0])
        assert f["ellipsoids"] > 0 and f["general"] > 0 and f["patterns"] > 0
        for k, v in f.items():
            tot.setdefault(k, []).append(v)
    for k in ("cubes", "closed_cyl", "tubes", "cones", "shadowless_spheres", "nested_glass"):
        assert sum(tot[k]) > 0, k
    assert max(tot["groups"]) > 1  # a divided group: subgroups
    assert {2, 3} <= set(tot["lights"]) and max(tot["planes"]) == 3
    assert sum(tot["unbounded"]) == 0  # (scenes.fuzz keeps none: the `solids` scene has them)


@pytest.mark.parametrize("quads,tris,csg", CLASSES, ids=["plain", "quads", "tris", "csg"])
def test_every_reachable_kernel_variant_ran(sweep, quads, tris, csg):
    """Completeness: the asserted plan readouts of the sweep cover every
    (LANE, QUADS, TALLY, CAM, TRIS, CSG) instantiation the launch switch can
    produce, except those LAUNCH_TABLE explains as unreachable."""
    reached = set()
    for name in sorted(SCENES):
        reached |= sweep(name).reached
    assert reached <= set(LAUNCH_TABLE), reached - set(LAUNCH_TABLE)
    mine = lambda t: (t[1], t[4], t[5]) == (quads, tris, csg)
    want = {t for t, why in LAUNCH_TABLE.items() if mine(t) and why is None}
    assert len(want) == (22 if quads else 18)
    missing = want - reached
    assert not missing, sorted(missing)
    unreachable = {t for t, why in LAUNCH_TABLE.items() if mine(t) and why is not None}
    assert not (unreachable & reached), sorted(unreachable & reached)


# ---------------------------------------------------------------- plan outcomes that need size
N_BIG = 3000          # C3 spheres: past LANE 0's LDS sphere records and LANE 3's treelet
N_WIDE_OUT = 1000     # light field, 16 lights: the four-wide LDS image + distances pass the limit -> LANE 14
N_DELTAS_OUT = 1200   # ... the pair image still fits, its distances do not
SIZE_TABLE = {        # case -> (lane, lds_flags, n_top, dyn) as measured; asserted below
    "c5": (4, 2, 1183, 162800),
    "c5 treelet_deltas=0": (4, 0, 1808, 162816),
    "c5 treelet=0": (4, 2, 0, 87088),
    "c3 big image=3 wide=0": (3, 2, 1426, 97264),
    "c3 big image=3 wide=0 treelet_deltas=0": (3, 0, 1520, 97280),
    "c3 big image=3 wide=0 shadow_lb=0": (3, 0, 1520, 97280),
    "c3 big prim_lane=0 (primary)": (0, 2, 0, 6000),
    "lights16 wide out": (14, 2, 0, 146400),
    "lights16 deltas out": (14, 0, 0, 162240),
}


def _plan(rt, w, which="secondary"):
    p = rt._rtamd._wf_plan(w)[which]
    return p["lane"], p["lds_flags"], p["n_top"], p["dyn"]


def _reference(rt, oracle, w, cam, depth):
    """The exhaustive frame, checked bitwise against the oracle (counters and PPM too)."""
    exh, st = cam.render(w, depth)
    e = exh.to_numpy()
    ref, rst = oracle.OracleWorld.from_world(w).render(cam.desc_bytes(), depth, nthreads=NTHREADS)
    assert e.tobytes() == ref.tobytes(), int((e != ref).sum())
    assert rt.canvas_to_ppm(e) == oracle.canvas_to_ppm(ref)
    for k in COUNTERS:
        assert st[k] == rst[k], k
    return e.tobytes(), st


def _fast(cam, w, depth, exact, knobs):
    """The fast frame and the counted fast frame under `knobs`: bitwise `exact`."""
    _tune(w, knobs)
    try:
        fast, _ = cam.render(w, depth, want_stats=False)
        cnt, st = cam.render(w, depth, want_stats=True, exhaustive=False)
    finally:
        _restore(w, knobs)
    assert fast.to_numpy().tobytes() == exact[0], knobs
    assert cnt.to_numpy().tobytes() == exact[0], knobs
    for k in RAY_KEYS:
        assert st[k] == exact[1][k], (knobs, k)


def test_size_c5_partial_treelet_lane4(rt, oracle):
    """C5's 9996 spheres on a 64x64 frame: the four-wide global image (LANE 4)
    with a treelet that holds only the top of the hierarchy, after the staged
    distances; without the distances (a larger treelet); without a treelet."""
    from rtamd import scenes
    w, cam, depth = scenes.c5(64, 64)
    exact = _reference(rt, oracle, w, cam, depth)
    n_wide = _prof(rt, w)["n_bvh_wide"]
    _fast(cam, w, depth, exact, {})
    assert _plan(rt, w) == SIZE_TABLE["c5"] and _plan(rt, w, "primary") == SIZE_TABLE["c5"]
    lane, flags, n_top, dyn = _plan(rt, w)
    assert lane == 4 and flags == 2 and 0 < n_top < n_wide and dyn <= K_FUSED_LDS_LIMIT < dyn + 64
    _fast(cam, w, depth, exact, {"treelet_deltas": 0})
    assert _plan(rt, w) == SIZE_TABLE["c5 treelet_deltas=0"]
    lane, flags, n_top2, dyn = _plan(rt, w)
    assert lane == 4 and flags == 0 and n_top < n_top2 < n_wide and dyn <= K_FUSED_LDS_LIMIT < dyn + 64
    _fast(cam, w, depth, exact, {"treelet": 0})
    assert _plan(rt, w) == SIZE_TABLE["c5 treelet=0"]
    lane, flags, n_top, _ = _plan(rt, w)
    assert lane == 4 and flags == 2 and n_top == 0
    for lb in (1, 0):  # the wave traversal for generation 0, shadows through the light buffer or the treelet walk
        _fast(cam, w, depth, exact, {"prim_lane": 0, "shadow_lb": lb})
        assert _plan(rt, w, "primary")[:2] == (0, 0 if lb == 0 else 2)  # 9996 sphere records do not fit LDS
        assert _plan(rt, w)[0] == 4 and 0 < _plan(rt, w)[2] < n_wide


@pytest.fixture(scope="module")
def big_c3(rt, oracle):
    from rtamd import scenes
    w, cam, depth = scenes.c3(64, 36, n_spheres=N_BIG)
    return w, cam, depth, _reference(rt, oracle, w, cam, depth)


def test_size_lane3_partial_treelet(rt, big_c3):
    """3000 spheres over the binary global image: LANE 3's treelet takes what
    its 64-KB static stack leaves, the top of the hierarchy only, so the walk
    crosses from LDS nodes to global ones (lane_trace's e < n_top split)."""
    w, cam, depth, exact = big_c3
    p = _prof(rt, w)
    assert p["n_diag"] == N_BIG and p["bvh_depth"] <= K_LANE_LDS_DEPTH
    for knobs, case in (({"image": 3, "wide": 0}, "c3 big image=3 wide=0"),
                        ({"image": 3, "wide": 0, "treelet_deltas": 0}, "c3 big image=3 wide=0 treelet_deltas=0"),
                        ({"image": 3, "wide": 0, "shadow_lb": 0}, "c3 big image=3 wide=0 shadow_lb=0")):
        _fast(cam, w, depth, exact, knobs)
        assert _plan(rt, w) == SIZE_TABLE[case], (case, _plan(rt, w))
        lane, flags, n_top, dyn = _plan(rt, w)
        assert lane == 3 and 0 < n_top < p["n_bvh_nodes"]
        assert flags == (2 if case.endswith("wide=0") else 0)
        assert dyn + _static_lds(3) <= K_FUSED_LDS_LIMIT < dyn + _static_lds(3) + 64
        assert _plan(rt, w, "primary")[0] == 0  # (LANE 3 never takes a camera's generation 0 here)


def test_size_lane0_without_lds_sphere_records(rt, oracle, big_c3):
    """prim_lane=0 on 3000 spheres: the wave traversal reads the sphere records
    from global memory (kLdsSpheres clear: 3000 x 64 B pass the limit); the
    1000-sphere scene stages them."""
    from rtamd import scenes
    w, cam, depth, exact = big_c3
    for knobs in ({"prim_lane": 0}, {"prim_lane": 0, "image": 3}, {"prim_lane": 0, "shadow_lb": 0}):
        _fast(cam, w, depth, exact, knobs)
        lane, flags, n_top, dyn = _plan(rt, w, "primary")
        assert lane == 0 and not (flags & 1) and n_top == 0, (knobs, lane, flags)
        assert bool(flags & 2) == bool(knobs.get("shadow_lb", 1))
    _fast(cam, w, depth, exact, {"prim_lane": 0})
    assert _plan(rt, w, "primary") == SIZE_TABLE["c3 big prim_lane=0 (primary)"]
    w1, cam1, depth1 = scenes.c3(64, 36)
    _fast(cam1, w1, depth1, _reference(rt, oracle, w1, cam1, depth1), {"prim_lane": 0})
    lane, flags, _, dyn = _plan(rt, w1, "primary")
    assert lane == 0 and flags == 3 and dyn >= 1000 * 64


def test_size_distances_that_do_not_fit(rt, oracle):
    """16 lights make the light buffer's distances large (2 B x lights x spheres):
    first the four-wide LDS image no longer fits beside them and the plan falls
    to the pair image (LANE 14, distances staged); with more spheres the pair
    image fits but its distances stay in global memory (lb_walk's binary32
    arm)."""
    for n, case, flags_want in ((N_WIDE_OUT, "lights16 wide out", 2), (N_DELTAS_OUT, "lights16 deltas out", 0)):
        w, cam, depth = _light_field(rt, n, 16)
        exact = _reference(rt, oracle, w, cam, depth)
        p = _prof(rt, w)
        assert p["lb_res"] > 0 and p["n_lights"] == 16 and p["n_diag"] == n and p["n_bvh_wide"] > 0
        _fast(cam, w, depth, exact, {})  # lds_wide = 1, and still LANE 14
        assert _plan(rt, w) == SIZE_TABLE[case], (case, _plan(rt, w))
        lane, flags, n_top, dyn = _plan(rt, w)
        assert lane == 14 and flags == flags_want and n_top == 0 and dyn <= K_FUSED_LDS_LIMIT
        assert _plan(rt, w, "primary")[:2] == (14, flags_want)
        _fast(cam, w, depth, exact, {"shadow_lb": 0})  # no distances asked for: the wide image fits again
        assert _plan(rt, w)[:2] == ((15, 0) if n == N_WIDE_OUT else (14, 0))
        for knobs in ({"image": 3}, {"image": 3, "wide": 0}, {"image": 1}, {"prim_lane": 0}):
            _fast(cam, w, depth, exact, knobs)  # 16 lights through the global-memory images and the wave traversal
            assert _plan(rt, w)[0] == {3: 4 if knobs.get("wide", 1) else 3, 1: 1, 0: 14}[knobs.get("image", 0)]


def test_size_17_lights_no_light_buffer(rt, oracle):
    """One light past kLbMaxLights: the scene has no light buffer, so every
    shadow ray walks the image's own hierarchy, on LANE 15, 14, 4 and 3."""
    w, cam, depth = _light_field(rt, N_WIDE_OUT, 17)
    exact = _reference(rt, oracle, w, cam, depth)
    p = _prof(rt, w)
    assert p["lb_res"] == 0 and p["n_lights"] == 17
    for knobs, lane in (({}, 15), ({"lds_wide": 0}, 14), ({"image": 3}, 4), ({"image": 3, "wide": 0}, 3)):
        _fast(cam, w, depth, exact, knobs)
        got = _plan(rt, w)
        assert got[0] == lane and not (got[1] & 2), (knobs, got)


def test_size_own_sphere_rules_across_images(rt, sweep):
    """own_sphere 0, 1 and 2 (the shadow rays of a hit on a sphere record: that
    sphere tested first from inside, left out from outside) on the ellipsoid
    cluster under LANE 14, 4 and 3, with the light buffer and without: the
    frame and the reference's counters do not move."""
    s = sweep("cluster")
    assert not s.failures, "\n".join(s.failures)
    for knobs, lane in (({"lds_wide": 0}, 14), ({"image": 3}, 4), ({"image": 3, "wide": 0}, 3)):
        for own in (0, 1, 2):
            for lb in (1, 0):
                _fast(s.cam, s.w, s.depth, (s.frame, s.st), dict(knobs, own_sphere=own, shadow_lb=lb))
                assert _plan(rt, s.w)[0] == lane
                _tune(s.w, dict(knobs, own_sphere=own, shadow_lb=lb))
                try:
                    col, _ = s.w.color_at_batch(s.rays, s.depth, False, False)
                finally:
                    _restore(s.w, dict(knobs, own_sphere=own, shadow_lb=lb))
                assert col.tobytes() == s.batch[0].tobytes(), (knobs, own, lb)
