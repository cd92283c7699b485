"""The hierarchy over the other bounded records (other_trace, rt_bvh.cpp other_box: general spheres,
cubes, closed cylinders) at the edges its culling rule was argued for (DESIGN.md 5.2 "The other
records"): Cube::check_axis's parallel band (an object-space |d| < EPSILON on an axis: the roots leave
the cube by up to |t| EPSILON), Cylinder::local_intersect's cap-only band (dx^2 + dz^2 < EPSILON: one cap
root behind an origin outside the box), the EPSILON thresholds themselves, exact zeros, tangents, the
condition-number limit of a box, and rays outside the domain the cubes' boxes are widened for (kOtherDirMin,
kOtherOriginMax: farther origins walk with grown boxes, shorter or non-finite rays test every record).

The instrument: cam.render(w, depth, True, exhaustive) and w.color_at_batch(rays, depth, True,
exhaustive), fast against exhaustive against the checker of tests/csg_ref.py (pinned to the oracle by
tests/test_csg_ref.py), colours and the counters in COUNTS bit for bit, with the hit records and the
shadow answers of the same rays against the checker. Every case asserts from the profile readout that
the hierarchy exists and how many records it holds. Two regimes build it: a world of one to three boxed
records and no diagonal sphere, and a world of diagonal spheres with at least 16 boxed solids.

Each case's conditions on its own inputs come from the checker alone; the unmarked test_inputs_* hold
them without a GPU, and the GPU tests hold them again on the rays they send.
"""
import itertools
import math

import numpy as np
import pytest

import csg_ref

COUNTS = ("rays_primary", "rays_reflect", "rays_refract", "rays_shadow", "sphere_tests", "plane_tests", "other_tests")
EPS = 0.00001  # lib.rs:18
K_OTHER_DIR_MIN, K_OTHER_ORIGIN_MAX = 0.5, 1024.0  # rt_layout.hpp kOtherDirMin, kOtherOriginMax
W, H = 24, 16


# ---------------------------------------------------------------- helpers
def _transform(ref, i):
    return np.array(ref.s["transform"][i], dtype=np.float64).reshape(4, 4)


def _parent_box(T, lo=(-1.0, -1.0, -1.0), hi=(1.0, 1.0, 1.0)):
    """The box this hierarchy gave a record before its cubes were widened: the region's corners through the
    transform, then 1e-6 of size and position (pad_axis). Returns lo, hi (padded) and the padding."""
    c = np.array([[x, y, z, 1.0] for x, y, z in itertools.product(*zip(lo, hi))]) @ T.T
    mn, mx = c[:, :3].min(axis=0), c[:, :3].max(axis=0)
    pad = 1e-6 * ((mx - mn) + np.abs(mn) + np.abs(mx)) + 1e-9
    return mn - pad, mx + pad, pad


def _world_rays(T, o_obj, d_obj):
    """Object-space origins and directions as world rays (unit directions)."""
    o = np.asarray(o_obj, dtype=np.float64) @ T[:3, :3].T + T[:3, 3]
    d = np.asarray(d_obj, dtype=np.float64) @ T[:3, :3].T
    return np.hstack([o, d / np.linalg.norm(d, axis=1, keepdims=True)])


def _scaled(T, main, small):
    """Object-space directions `main` + `small`, with `small` scaled so that the OBJECT-space direction of the
    unit world ray has exactly these small components (the reference normalises in world space)."""
    main, small = np.asarray(main, dtype=np.float64), np.asarray(small, dtype=np.float64)
    v = main.copy()
    for _ in range(4):
        n = np.linalg.norm(v @ T[:3, :3].T, axis=1, keepdims=True)
        v = main + small * n
    return v


def _local(ref, i, ray):
    return csg_ref.ray_transform(ref.s["inverse"][i], tuple(ray[:3]), tuple(ray[3:]))


def _outside_parent_box(ref, i, rays):
    """How many rays the checker lands on object i (as a hit, or as the blocker of a shadow ray) at a point
    outside the parent's box of i by more than 100 times that box's padding."""
    lo, hi, pad = _parent_box(_transform(ref, i))
    n = 0
    for r in rays:
        xs = [x for x in ref.intersect(r[:3], r[3:]) if x[0] >= 0.0]
        if not xs or xs[0][1] != i:
            continue
        p = r[:3] + xs[0][0] * r[3:6]
        n += bool((np.maximum(p - hi, lo - p) > 100.0 * pad).any())
    return n


def _light(rt, w, at=(-300.0, 400.0, -500.0), i=1.0):
    w.add_light(rt.PointLight(rt.Point(*at), rt.Color(i, i, i)))


def _general_sphere(rt, at, r=0.5, glass=None, turn=0.4):
    s = rt.glass_sphere() if glass else rt.Sphere()
    s.set_transform(rt.translation(*at) * rt.rotation_y(turn) * rt.rotation_z(0.3) * rt.scaling(r, 0.8 * r, r))
    if glass:
        s.material.refractive_index = glass
        s.material.reflective = 0.3
    else:
        s.material.color = rt.Color(0.9, 0.3, 0.2)
    return s


def _cube(rt, transform, color=(0.3, 0.6, 0.9)):
    c = rt.Cube()
    c.set_transform(transform)
    c.material.color = rt.Color(*color)
    c.material.reflective = 0.2
    return c


def _field(rt, w, n=16, at=(0.0, -300.0, 0.0)):
    """The second regime: two diagonal glass spheres (a sphere hierarchy) and n small boxed solids, far from the case's rays."""
    for k in range(2):
        s = rt.glass_sphere()
        s.set_transform(rt.translation(at[0] + 3.0 * k, at[1], at[2] - 4.0) * rt.scaling(0.8, 0.8, 0.8))
        w.add_object(s)
    for k in range(n):
        x, z = at[0] + 2.5 * (k % 4), at[2] + 2.5 * (k // 4)
        if k % 3 == 0:
            s = rt.Cylinder(-0.5, 0.7, True)
        elif k % 3 == 1:
            s = rt.Cube()
        else:
            s = rt.Sphere()
        s.set_transform(rt.translation(x, at[1], z) * rt.rotation_x(0.2 * k) * rt.scaling(0.6, 0.5, 0.7))
        s.material.color = rt.Color(0.2 + 0.04 * k, 0.5, 0.9 - 0.04 * k)
        w.add_object(s)


def _band_rays(T, rng, n, two, dist=600.0):
    """Rays along an object axis of the cube under T from `dist` (world units) away, towards either face, with one
    or two other object-space components inside (0, EPSILON), of both signs, starting inside those slabs just under
    the face the component points at: the reference's roots leave the cube by |t| EPSILON."""
    ax = rng.integers(0, 3, size=n)
    par = (ax + 1 + rng.integers(0, 2, size=n)) % 3
    oth = 3 - ax - par
    step = np.linalg.norm(T[:3, :3], axis=0)  # world length of an object-space step on each axis
    face = rng.choice([-1.0, 1.0], size=n)
    sgn = rng.choice([-1.0, 1.0], size=(n, 2))
    main, small, o = np.zeros((n, 3)), np.zeros((n, 3)), rng.uniform(-0.8, 0.8, size=(n, 3))
    k = np.arange(n)
    main[k, ax] = -face
    small[k, par] = sgn[:, 0] * rng.uniform(0.5, 0.95, size=n) * EPS
    o[k, par] = sgn[:, 0] * (1.0 - rng.uniform(1e-4, 2e-3, size=n))
    if two:
        small[k, oth] = sgn[:, 1] * rng.uniform(0.5, 0.95, size=n) * EPS
        o[k, oth] = sgn[:, 1] * (1.0 - rng.uniform(1e-4, 2e-3, size=n))
    o[k, ax] = face * (1.0 + dist / step[ax])
    return _world_rays(T, o, _scaled(T, main, small))


# ---------------------------------------------------------------- cases: (world, rays, depth, boxed records, condition)
def _case_cube_band(rt, scale, two, grouped=False, field=False):
    """1. The cube's parallel band, seen from 600 away: the scale-50 cube and the unit cube, one and two small
    components, top level or inside a transformed, divided group (the gate at the leaf), alone or with the field."""
    w = rt.World()
    if grouped:
        g = rt.Group()
        g.add_child(_cube(rt, rt.scaling(1.0, 1.0, 1.0)))
        for k in range(4):
            g.add_child(_general_sphere(rt, (-0.5 + 0.3 * k, 1.3, 0.2 * k), 0.2))
        g.set_transform(rt.scaling(scale, scale, scale))
        g.divide(2)
        w.add_object(g)
    else:
        w.add_object(_cube(rt, rt.scaling(scale, scale, scale)))
        w.add_object(_general_sphere(rt, (0.0, 3.0 * scale, 0.0), 0.5 * scale))
    if field:
        _field(rt, w)
    _light(rt, w)
    rng = np.random.default_rng(int(scale) + 2 * two + 4 * grouped)
    T = np.diag([scale, scale, scale, 1.0])
    rays = _band_rays(T, rng, 48, two)
    boxed = (5 if grouped else 2) + (16 if field else 0)

    def cond(ref):
        cube = int(np.flatnonzero(ref.s["kind"] == 2)[0])
        assert np.allclose(_transform(ref, cube), T)
        assert _outside_parent_box(ref, cube, rays) >= 16
        small = [sum(0.0 < abs(c) < EPS for c in _local(ref, cube, r)[1]) for r in rays]
        assert small.count(2 if two else 1) >= 40, small
    return w, rays, 3, boxed, cond


def _case_cube_sheared(rt):
    """1b. A rotated and sheared cube: the small component shows only in object space."""
    w = rt.World()
    m = rt.translation(3.0, -2.0, 1.0) * rt.rotation_z(0.4) * rt.rotation_y(-0.7) * rt.shearing(0.3, 0.0, 0.0, 0.2, 0.1, 0.0) \
        * rt.scaling(20.0, 10.0, 30.0)
    w.add_object(_cube(rt, m))
    w.add_object(_general_sphere(rt, (0.0, 60.0, 0.0), 8.0))
    _light(rt, w)
    T = _transform(csg_ref.CsgRef.from_world(w), 0)
    rays = np.vstack([_band_rays(T, np.random.default_rng(21), 32, False, 500.0),
                      _band_rays(T, np.random.default_rng(22), 32, True, 500.0)])

    def cond(ref):
        assert _outside_parent_box(ref, 0, rays) >= 16
        assert (np.abs(rays[:, 3:]).min(axis=1) > 1e-3).sum() >= 48  # no small component in world space
    return w, rays, 3, 2, cond


def _cylinder_world(rt, length, general, target_y=None, field=False):
    """A closed glass cylinder (index 1.5) of `length` radii, upright or under a general transform; with `target_y`,
    beside its wall at that object-space height a second glass solid (index 1.3) before a checkered wall. Returns the
    world and the cylinder's transform."""
    w = rt.World()
    cyl = rt.Cylinder(0.0, length, True)
    m = rt.translation(0.5, -1.0, 2.0) * rt.rotation_z(0.5) * rt.rotation_x(-0.3) * rt.scaling(0.6, 0.05 if length > 10 else 0.9, 0.8) \
        if general else rt.scaling(1.0, 1.0, 1.0)
    cyl.set_transform(m)
    cyl.material.transparency, cyl.material.refractive_index = 0.9, 1.5
    cyl.material.reflective, cyl.material.diffuse = 0.3, 0.2
    w.add_object(cyl)
    T = _transform(csg_ref.CsgRef.from_world(w), 0)
    if target_y is None:
        return w, T
    r = 1.5 * float(np.linalg.norm(T[:3, 0]))
    gap = 3.0 + 2.5 * r / float(np.linalg.norm(T[:3, 1]))
    at = T[:3, :3] @ np.array([1.01, target_y + gap, 0.0]) + T[:3, 3]
    w.add_object(_general_sphere(rt, tuple(at), r, glass=1.3))
    up = T[:3, 1] / np.linalg.norm(T[:3, 1])
    wall = rt.Plane()  # what the refracted rays land on: their direction depends on n1 / n2
    far = at + (6.0 * r) * up
    # a plane through `far` with normal `up`: y turned onto `up` about x, then about z
    b = math.asin(max(-1.0, min(1.0, up[2])))
    a = math.atan2(-up[0], up[1])
    wall.set_transform(rt.translation(*far) * rt.rotation_z(a) * rt.rotation_x(b))
    pattern = rt.checkers_pattern(rt.Color(0.9, 0.9, 0.9), rt.Color(0.1, 0.1, 0.4))
    pattern.set_transform(rt.scaling(0.2 * r, 0.2 * r, 0.2 * r))
    wall.material.set_pattern(pattern)
    w.add_object(wall)
    if field:
        _field(rt, w)
    _light(rt, w, (-30.0, 40.0, -50.0))
    return w, T


def _case_cylinder(rt, length, general, mode, field=False):
    """4. The closed cylinder's cap-only band. In object space the line x = x0 + s y, x0 just under 1, crosses the cap
    y = 0 inside the disc and leaves through the wall without a root while dx^2 + dz^2 < EPSILON. A ray along +y from
    where the line is 0.006 beyond the wall, outside the box, has exactly one root, behind it: the cylinder is a
    container at the glass sphere ahead. `mode`: "behind" (that ray), "front" (the same line backwards from the same
    point: the single root ahead), "above" (a just above EPSILON: a wall root too, an even count, no container)."""
    _, T = _cylinder_world(rt, length, general)
    rng = np.random.default_rng(int(length) + 7 * general + {"behind": 0, "front": 1, "above": 2}[mode])
    n = 40
    x0 = 0.9995 - rng.uniform(0.0, 2e-4, size=n)
    ang = rng.uniform(-0.02, 0.02, size=n)  # the plane of the line, through the axis, turned a little about it
    a = np.full(n, 1.15 * EPS) if mode == "above" else rng.uniform(0.5, 0.95, size=n) * EPS
    sign = -1.0 if mode == "front" else 1.0
    main = np.tile([0.0, sign, 0.0], (n, 1))
    small = sign * np.sqrt(a)[:, None] * np.column_stack([np.cos(ang), np.zeros(n), np.sin(ang)])
    v = _scaled(T, main, small)
    s = np.hypot(v[:, 0], v[:, 2])  # the line's slope: x per unit of y
    y0 = 0.006 / s
    assert length <= 10 or y0.max() < length
    origins = lambda y: np.column_stack([(x0 + s * y) * np.cos(ang), y, (x0 + s * y) * np.sin(ang)])
    if general and length > 10:  # a turned tube's world box holds the points beside its wall: start above the far cap
        lo, hi, _ = _parent_box(T, (-1.0, 0.0, -1.0), (1.0, float(length), 1.0))
        above = 1.0
        while True:
            y0 = np.full(n, length + above)
            o = _world_rays(T, origins(y0), v)[:, :3]
            if ((o > hi) | (o < lo)).any(axis=1).all():
                break
            above *= 2.0
    rays = _world_rays(T, origins(y0), v)
    w, _ = _cylinder_world(rt, length, general, float(y0.max()), field)
    boxed = 2 + (16 if field else 0)

    def cond(ref):
        lo, hi, _ = _parent_box(_transform(ref, 0), (-1.0, 0.0, -1.0), (1.0, float(length), 1.0))
        outside = ((rays[:, :3] > hi) | (rays[:, :3] < lo)).any(axis=1)
        rec = ref.hit_batch(rays)
        roots = [[x[0] for x in ref.intersect(r[:3], r[3:]) if x[1] == 0] for r in rays]
        aa = np.array([(lambda d: d[0] * d[0] + d[2] * d[2])(_local(ref, 0, r)[1]) for r in rays])
        if mode == "behind":  # a container at the hit on the sphere, from an origin outside the cylinder's box
            assert (aa < EPS).all()
            ok = outside & (rec[:, 0] == 1) & (rec[:, 21] == 1.5) & np.array([len(t) == 1 and t[0] < 0 for t in roots])
        elif mode == "front":  # the single root ahead: the hit is the cylinder's cap, and it is all there is
            assert (aa < EPS).all()
            ok = outside & (rec[:, 0] == 0) & np.array([len(t) == 1 and t[0] > 0 for t in roots])
        else:  # both roots behind: no container
            assert (aa > EPS).all() and (aa < 1.3 * EPS).all()
            ok = outside & (rec[:, 0] == 1) & (rec[:, 21] == 1.0) & np.array([len(t) == 2 and max(t) < 0 for t in roots])
        assert ok.sum() >= 16, (int(ok.sum()), int(outside.sum()), rec[:4, [0, 21]], roots[:4])
    return w, rays, 4, boxed, cond


def _case_thresholds(rt):
    """5. The thresholds: a = EPSILON (1 -+ 1e-9) on a cylinder, |d| = EPSILON (1 -+ 1e-9) on a cube's axis, dy = 0
    exactly (the caps divide by zero), zero direction components, tangents of a general sphere."""
    w = rt.World()
    w.add_object(_cube(rt, rt.translation(-6.0, 0.0, 0.0) * rt.scaling(2.0, 1.0, 1.5)))
    cyl = rt.Cylinder(-1.0, 1.0, True)
    cyl.set_transform(rt.translation(0.0, 0.0, 0.0) * rt.scaling(1.5, 2.0, 1.5))
    cyl.material.color = rt.Color(0.8, 0.7, 0.2)
    w.add_object(cyl)
    w.add_object(_general_sphere(rt, (6.0, 0.0, 0.0), 1.5))
    _light(rt, w, (-30.0, 40.0, -50.0))
    ref = csg_ref.CsgRef.from_world(w)
    rng = np.random.default_rng(31)
    n = 20
    tags, rays = [], []
    for side in (-1.0, 1.0):
        # the cube: travel along +x from 40 away, dy at the threshold, starting just under the top face
        T = _transform(ref, 0)
        o = np.column_stack([np.full(n, -(1.0 + 40.0 / 2.0)), 1.0 - rng.uniform(1e-5, 1e-4, size=n), rng.uniform(-0.9, 0.9, size=n)])
        v = _scaled(T, np.tile([1.0, 0.0, 0.0], (n, 1)), np.tile([0.0, EPS * (1.0 + side * 1e-9), 0.0], (n, 1)))
        rays.append(_world_rays(T, o, v))
        tags += ["cube_below" if side < 0 else "cube_above"] * n
        # the cylinder: travel along +y from below, a at the threshold, over the rim
        T = _transform(ref, 1)
        ang = rng.uniform(0.0, 2.0 * math.pi, size=n)
        sa = math.sqrt(EPS * (1.0 + side * 1e-9))
        v = _scaled(T, np.tile([0.0, 1.0, 0.0], (n, 1)), sa * np.column_stack([np.cos(ang), np.zeros(n), np.sin(ang)]))
        rad = 1.0 - rng.uniform(0.0, 2e-3, size=n)
        o = np.column_stack([rad * np.cos(ang), np.full(n, -6.0), rad * np.sin(ang)])
        rays.append(_world_rays(T, o, v))
        tags += ["cyl_below" if side < 0 else "cyl_above"] * n
    # dy = 0 exactly, through and beside the cylinder and the cube; exact zeros in two components
    z = rng.uniform(-1.6, 1.6, size=n)
    rays.append(np.column_stack([np.full(n, -20.0), rng.uniform(-2.2, 2.2, size=n), z, np.ones(n), np.zeros(n), np.zeros(n)]))
    tags += ["zeros"] * n
    d = np.column_stack([np.ones(n), np.zeros(n), rng.uniform(-0.05, 0.05, size=n)])
    rays.append(np.hstack([np.column_stack([np.full(n, -20.0), rng.uniform(-2.2, 2.2, size=n), z]),
                           d / np.linalg.norm(d, axis=1, keepdims=True)]))
    tags += ["dy0"] * n
    # tangents of the general sphere: through a surface point, perpendicular to the object-space normal there
    T = _transform(ref, 2)
    p = rng.normal(size=(n, 3))
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    t = np.cross(p, rng.normal(size=(n, 3)))
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    rays.append(_world_rays(T, p - 8.0 * t, t))
    tags += ["tangent"] * n
    rays, tags = np.vstack(rays), np.array(tags)

    def cond(ref):
        ld = np.array([[_local(ref, i, r)[1] for i in range(3)] for r in rays])  # ray, object, component
        lo = np.array([[_local(ref, i, r)[0] for i in range(3)] for r in rays])
        dy = np.abs(ld[:, 0, 1])
        assert ((dy < EPS) & (dy > EPS * (1 - 1e-8)))[tags == "cube_below"].sum() >= 16
        assert ((dy >= EPS) & (dy < EPS * (1 + 1e-8)))[tags == "cube_above"].sum() >= 16
        a = ld[:, 1, 0] ** 2 + ld[:, 1, 2] ** 2
        assert ((a < EPS) & (a > EPS * (1 - 1e-8)))[tags == "cyl_below"].sum() >= 16
        assert ((a >= EPS) & (a < EPS * (1 + 1e-8)))[tags == "cyl_above"].sum() >= 16
        assert (ld[tags == "dy0", 1, 1] == 0.0).sum() >= 16 and (ld[tags == "zeros", 0, 1:] == 0.0).all()
        # tangent: the discriminant of sphere.rs:47-62 within rounding of zero, relative to its two terms
        o3, d3 = lo[tags == "tangent", 2], ld[tags == "tangent", 2]
        aa, bb, cc = (d3 * d3).sum(axis=1), 2.0 * (d3 * o3).sum(axis=1), (o3 * o3).sum(axis=1) - 1.0
        assert (np.abs(bb * bb - 4.0 * aa * cc) <= 1e-9 * bb * bb).sum() >= 16
        hit = ref.hit_batch(rays)[:, 0]
        assert (hit == 0).sum() >= 30 and (hit == 1).sum() >= 30 and (hit == 2).sum() >= 5
    return w, rays, 3, 3, cond


def _case_condition(rt):
    """6. A plate of condition just below 1e6 is boxed and culled; one just above stays in the exhaustive remainder."""
    w = rt.World()
    w.add_object(_cube(rt, rt.translation(0.0, 1.0, 0.0) * rt.scaling(1000.0, 1.1e-3, 1.0), (0.9, 0.2, 0.2)))   # 9.1e5
    w.add_object(_cube(rt, rt.translation(0.0, -1.0, 0.0) * rt.scaling(1000.0, 0.9e-3, 1.0), (0.2, 0.9, 0.2)))  # 1.1e6
    w.add_object(_general_sphere(rt, (0.0, 0.0, 3.0), 0.7))
    _light(rt, w, (-30.0, 40.0, -50.0))
    rng = np.random.default_rng(41)
    n = 96
    o = rng.uniform([-30.0, 3.0, -8.0], [30.0, 9.0, -4.0], size=(n, 3))
    o[::2, 1] *= -1.0
    aim = np.column_stack([rng.uniform(-40.0, 40.0, size=n), np.where(rng.random(n) < 0.5, 1.0, -1.0), rng.uniform(-1.2, 1.2, size=n)])
    d = aim - o
    rays = np.hstack([o, d / np.linalg.norm(d, axis=1, keepdims=True)])

    def cond(ref):
        hit = ref.hit_batch(rays)[:, 0]
        assert (hit == 0).sum() >= 16 and (hit == 1).sum() >= 16, np.bincount(hit.astype(int) + 1)
    return w, rays, 3, 2, cond


CASES = {
    "cube50_one": lambda rt: _case_cube_band(rt, 50.0, False),
    "cube50_two": lambda rt: _case_cube_band(rt, 50.0, True),
    "cube1_one": lambda rt: _case_cube_band(rt, 1.0, False),
    "cube1_two": lambda rt: _case_cube_band(rt, 1.0, True),
    "cube50_grouped": lambda rt: _case_cube_band(rt, 50.0, False, grouped=True),
    "cube50_field": lambda rt: _case_cube_band(rt, 50.0, True, field=True),
    "cube_sheared": _case_cube_sheared,
    "cyl1_behind": lambda rt: _case_cylinder(rt, 1.0, False, "behind"),
    "cyl1000_behind": lambda rt: _case_cylinder(rt, 1000.0, False, "behind"),
    "cyl1_general_behind": lambda rt: _case_cylinder(rt, 1.0, True, "behind"),
    "cyl1000_general_behind": lambda rt: _case_cylinder(rt, 1000.0, True, "behind"),
    "cyl1_behind_field": lambda rt: _case_cylinder(rt, 1.0, False, "behind", field=True),
    "cyl1_front": lambda rt: _case_cylinder(rt, 1.0, False, "front"),
    "cyl1_above": lambda rt: _case_cylinder(rt, 1.0, False, "above"),
    "thresholds": _case_thresholds,
    "condition": _case_condition,
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_inputs_meet_the_conditions_of_their_case(rt, name):
    """The conditions on each case's inputs, from the checker alone (no GPU)."""
    w, rays, depth, boxed, cond = CASES[name](rt)
    assert len(rays) <= 400 and depth <= 4
    dom = (np.abs(rays[:, :3]).max(axis=1) <= K_OTHER_ORIGIN_MAX) & (np.abs(rays[:, 3:]).max(axis=1) >= K_OTHER_DIR_MIN)
    assert dom.all()  # inside the walk's domain: these rays are culled, not looped
    cond(csg_ref.CsgRef.from_world(w))


def _upload(rt, w, boxed):
    """Creates the scene: a small world with leaves of one record (the default leaf of two would put a case's record
    and its neighbour behind one box, and the neighbour's box would let the rays in); a field world as it comes."""
    try:
        rt._rtamd._tuning_set("bvh_leaf", 1 if boxed < 16 else 0)
        w.upload()
    finally:
        rt._rtamd._tuning_set("bvh_leaf", 0)


def _readout(rt, w, boxed):
    p = rt._rtamd._wf_profile(w, -1, True)
    assert p["n_obvh_nodes"] > 0 and p["n_other_culled"] == boxed, (p["n_obvh_nodes"], p["n_other_culled"], boxed)


def _hold(rt, w, rays, depth, boxed, ref, shadow_pts=None):
    exh, est = w.color_at_batch(rays, depth, True, True)
    fast, fst = w.color_at_batch(rays, depth, True, False)
    _readout(rt, w, boxed)
    ref.counts = dict.fromkeys(csg_ref.COUNTERS, 0)
    want = ref.color_at_batch(rays, depth)
    exh, fast = np.asarray(exh), np.asarray(fast)
    assert exh.tobytes() == want.tobytes(), (int((exh != want).any(axis=1).sum()), np.abs(exh - want).max())
    assert fast.tobytes() == want.tobytes(), (int((fast != want).any(axis=1).sum()), np.abs(fast - want).max())
    for k in COUNTS:
        assert est[k] == ref.counts[k] and fst[k] == ref.counts[k], (k, est[k], fst[k], ref.counts[k])
    assert est["exhaustive"] and not fst["exhaustive"]
    got, rec = w.hit_batch(rays), ref.hit_batch(rays)
    assert np.array_equal(got[:, 0], rec[:, 0])
    assert got[:, 1:23].tobytes() == rec[:, 1:23].tobytes(), np.abs(got[:, 1:23] - rec[:, 1:23]).max()
    pts = rays[:, :3] if shadow_pts is None else shadow_pts
    shadowed = w.is_shadowed_batch(pts, 0).astype(bool)
    assert np.array_equal(shadowed, np.array([ref.is_shadowed(p, 0) for p in pts]))
    assert ref.csg_ties == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_fast_equals_exhaustive_equals_checker(rt, name):
    w, rays, depth, boxed, cond = CASES[name](rt)
    ref = csg_ref.CsgRef.from_world(w)
    cond(ref)
    _upload(rt, w, boxed)
    _hold(rt, w, rays, depth, boxed, ref)


# ---------------------------------------------------------------- 2: the band as a frame
def _pixel_rays(ref, cam):
    c = np.frombuffer(cam.desc_bytes(), dtype=csg_ref.CAMERA)[0]
    return np.array([list(o) + list(d) for o, d in (ref.ray_for_pixel(c, x, y) for y in range(H) for x in range(W))])


def _band_frame(rt):
    """A camera 600 from the scale-50 cube, level with its top edge, 1.2 mrad wide: 5e-5 rad a pixel, so every
    row's object-space dy is inside the band, and the rows looking up land on the cube above its top face."""
    w = rt.World()
    w.add_object(_cube(rt, rt.scaling(50.0, 50.0, 50.0)))
    w.add_object(_general_sphere(rt, (0.0, 150.0, 0.0), 25.0))
    _light(rt, w)
    cam = rt.Camera(W, H, 1.2e-3)
    cam.set_transform(rt.view_transform(rt.Point(-600.0, 49.99, 3.0), rt.Point(0.0, 49.99, 3.0), rt.Vector(0, 1, 0)))
    return w, cam, 3, 2


def _band_frame_cond(ref, cam):
    rays = _pixel_rays(ref, cam)
    lo, hi, pad = _parent_box(_transform(ref, 0))
    rows = 0
    for y in range(H):
        row = rays[y * W:(y + 1) * W]
        assert all(0.0 < abs(_local(ref, 0, r)[1][1]) < EPS for r in row)
        rows += _outside_parent_box(ref, 0, row) == W
    assert rows >= 1, rows
    return rays


def _shadow_frame(rt):
    """3. Shadow rays in the band: a floor strip at z just under the cube's face z = 50, far on the -x side, and a
    light far on the +x side a little beyond that face: the shadow rays cross the cube's x range with an object-space
    dz inside the band, outside the cube, and the reference has the cube block them."""
    w = rt.World()
    w.add_object(_cube(rt, rt.scaling(50.0, 50.0, 50.0)))
    floor = rt.Plane()
    floor.set_transform(rt.translation(0.0, -40.0, 0.0))
    floor.material.color = rt.Color(0.9, 0.9, 0.8)
    w.add_object(floor)
    w.add_object(_general_sphere(rt, (0.0, 150.0, 0.0), 25.0))
    _light(rt, w, (600.0, -30.0, 50.4))
    cam = rt.Camera(W, H, 8e-3)  # looking straight down on the strip from 10 above: 0.08 wide
    cam.set_transform(rt.view_transform(rt.Point(-600.0, -30.0, 49.95), rt.Point(-600.0, -40.0, 49.95), rt.Vector(1, 0, 0)))
    rng = np.random.default_rng(51)
    pts = np.column_stack([rng.uniform(-700.0, -500.0, size=64), np.full(64, -40.0 + EPS), rng.uniform(49.9, 49.99, size=64)])
    return w, cam, 2, 2, pts


def _shadow_cond(ref, pts):
    L = ref.lights[0][:3]
    d = L - pts
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.hstack([pts, d])
    assert all(0.0 < abs(_local(ref, 0, r)[1][2]) < EPS for r in rays)
    blocked = np.array([ref.is_shadowed(p, 0) for p in pts])
    assert _outside_parent_box(ref, 0, rays[blocked]) >= 16 and blocked.sum() >= 16


def test_inputs_of_the_frames_meet_their_conditions(rt):
    w, cam, _, _ = _band_frame(rt)
    _band_frame_cond(csg_ref.CsgRef.from_world(w), cam)
    w, cam, _, _, pts = _shadow_frame(rt)
    ref = csg_ref.CsgRef.from_world(w)
    _shadow_cond(ref, pts)
    hit = ref.hit_batch(_pixel_rays(ref, cam))
    assert (hit[:, 0] == 1).all() and (np.abs(hit[:, 4] - 49.95) < 0.05).all()  # every pixel on the strip


def _hold_frame(rt, w, cam, depth, boxed, ref):
    fast, fst = cam.render(w, depth, True, False)
    _readout(rt, w, boxed)
    plain, _ = cam.render(w, depth, False, False)
    exh, est = cam.render(w, depth, True, True)
    ref.counts = dict.fromkeys(csg_ref.COUNTERS, 0)
    img, rst = ref.render(cam.desc_bytes(), depth)
    fast, plain, exh = fast.to_numpy(), plain.to_numpy(), exh.to_numpy()
    assert exh.tobytes() == img.tobytes(), np.abs(exh - img).max()
    assert fast.tobytes() == img.tobytes(), (int((fast != img).any(axis=2).sum()), np.abs(fast - img).max())
    assert plain.tobytes() == img.tobytes(), np.abs(plain - img).max()
    for k in COUNTS:
        assert fst[k] == rst[k] and est[k] == rst[k], (k, fst[k], est[k], rst[k])
    assert not fst["exhaustive"] and est["exhaustive"] and img.sum() > 0 and ref.csg_ties == 0


@pytest.mark.gpu
def test_band_frame(rt):
    w, cam, depth, boxed = _band_frame(rt)
    ref = csg_ref.CsgRef.from_world(w)
    rays = _band_frame_cond(ref, cam)
    _upload(rt, w, boxed)
    _hold_frame(rt, w, cam, depth, boxed, ref)
    _hold(rt, w, rays[::4], depth, boxed, ref)


@pytest.mark.gpu
def test_shadow_rays_in_the_band(rt):
    w, cam, depth, boxed, pts = _shadow_frame(rt)
    ref = csg_ref.CsgRef.from_world(w)
    _shadow_cond(ref, pts)
    _upload(rt, w, boxed)
    _hold_frame(rt, w, cam, depth, boxed, ref)
    _hold(rt, w, _pixel_rays(ref, cam)[::4], depth, boxed, ref, shadow_pts=pts)


# ---------------------------------------------------------------- 7: rays outside the walk's domain
def _domain_world(rt):
    w = rt.World()
    w.add_object(_cube(rt, rt.translation(-2.5, 0.0, 0.0) * rt.rotation_y(0.3) * rt.scaling(0.8, 0.8, 0.8)))
    cyl = rt.Cylinder(-1.0, 1.0, True)
    cyl.set_transform(rt.translation(0.0, 0.0, 0.0) * rt.rotation_z(0.2))
    cyl.material.transparency, cyl.material.refractive_index, cyl.material.diffuse = 0.8, 1.5, 0.3
    w.add_object(cyl)
    w.add_object(_general_sphere(rt, (2.5, 0.0, 0.0), 1.0, glass=1.3))
    _light(rt, w, (-30.0, 40.0, -50.0))
    return w


def _domain_rays(seed=61, n=90):
    rng = np.random.default_rng(seed)
    aim = np.array([[-2.5, 0.0, 0.0], [0.0, 0.0, 0.0], [2.5, 0.0, 0.0]])[rng.integers(0, 3, size=n)] + rng.uniform(-0.7, 0.7, size=(n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    k = np.arange(n)
    dist = np.where(k % 3 == 0, np.where(k % 2 == 0, 1100.0, 9000.0), 6.0)[:, None]  # a third from beyond the origin bound
    o = aim - dist * d
    d[1::6] *= 0.25   # |d|_inf below the direction bound
    d[4::6] *= 1e-3   # short
    d[2::9] *= 1e6    # huge
    return np.hstack([o, d])


def test_inputs_of_the_domain_rays():
    rays = _domain_rays()
    assert (np.abs(rays[:, :3]).max(axis=1) > K_OTHER_ORIGIN_MAX).sum() >= 16
    assert (np.abs(rays[:, 3:]).max(axis=1) < K_OTHER_DIR_MIN).sum() >= 16
    inside = (np.abs(rays[:, :3]).max(axis=1) <= K_OTHER_ORIGIN_MAX) & (np.abs(rays[:, 3:]).max(axis=1) >= K_OTHER_DIR_MIN)
    assert inside.sum() >= 16 and (np.abs(rays[:, 3:]).max(axis=1) > 1e5).sum() >= 5


def _far_band_rays(ref):
    """The parallel band from 5000 away, past kOtherOriginMax: the roots leave the cube by 0.03 to 0.05 of its size."""
    return _band_rays(_transform(ref, 0), np.random.default_rng(63), 32, False, 5000.0)


def test_inputs_of_the_far_band_rays(rt):
    ref = csg_ref.CsgRef.from_world(_domain_world(rt))
    rays = _far_band_rays(ref)
    assert (np.abs(rays[:, :3]).max(axis=1) > 2.0 * K_OTHER_ORIGIN_MAX).all()
    assert _outside_parent_box(ref, 0, rays) >= 16


@pytest.mark.gpu
def test_rays_outside_the_walks_domain(rt):
    """The cubes' widening is argued for rays with |d|_inf >= kOtherDirMin from |o|_inf <= kOtherOriginMax. A ray from
    farther off walks the hierarchy with every box grown by what a cube's root can add from there (other_far_pad),
    and a caller's ray shorter than kOtherDirMin tests every record instead of walking. Far origins (the cube's
    parallel band from 5000 away among them), short, huge and non-unit directions beside ordinary rays, against the
    checker."""
    w = _domain_world(rt)
    ref = csg_ref.CsgRef.from_world(w)
    far = _far_band_rays(ref)
    assert _outside_parent_box(ref, 0, far) >= 16
    rays = np.vstack([_domain_rays(), far])
    assert (ref.hit_batch(rays)[:, 0] >= 0).sum() >= 30
    _upload(rt, w, 3)
    _hold(rt, w, rays, 3, 3, ref)


@pytest.mark.gpu
def test_non_finite_rays(rt):
    """An infinite and a NaN direction or origin component, mixed with ordinary rays: fast equals exhaustive bit for
    bit, counters included, and both equal the checker on every ray the reference itself survives (its sort
    panics on a NaN t, so such a ray has no reference answer)."""
    w = _domain_world(rt)
    rays = _domain_rays(62, 60)
    rays[0::6, 3] = np.inf
    rays[1::6, 4] = np.nan
    rays[2::12, 1] = np.nan
    rays[3::12, 5] = -np.inf
    depth = 2
    _upload(rt, w, 3)
    exh, est = w.color_at_batch(rays, depth, True, True)
    fast, fst = w.color_at_batch(rays, depth, True, False)
    _readout(rt, w, 3)
    exh, fast = np.asarray(exh), np.asarray(fast)

    def same(a, b):  # bit for bit, but for which NaN it is
        nan = np.isnan(a)
        return np.array_equal(nan, np.isnan(b)) and a[~nan].tobytes() == b[~nan].tobytes()
    assert same(fast, exh), np.flatnonzero((fast != exh).any(axis=1))
    for k in COUNTS:
        assert est[k] == fst[k], (k, est[k], fst[k])
    ref = csg_ref.CsgRef.from_world(w)
    held = 0
    for i, r in enumerate(rays):
        try:
            with np.errstate(all="ignore"):
                want = np.array(ref.color_at(r[:3], r[3:], depth), dtype=np.float64)
        except (ValueError, ZeroDivisionError, OverflowError):
            continue
        held += 1
        assert same(fast[i], want), (i, r, fast[i], want)
    assert held >= 20
