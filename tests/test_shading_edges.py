"""Shading at the edges of the material domain: the cases, their conditions, and the checker against the oracle.

The code held: pattern_color, lighting and schlick (rt_device.hpp), the spawn rules of prep_one and shade_fused
(rt_wf_device.hpp), shadow_irrelevant and shade_color_rt (rt_trace.hpp) and the two combines (rt_wf_combine.hip).
Each has branches that only an edge input reaches: fmod2_is_zero's integer conversion below 2^53, its "every such
value is even" at and above, its rule for non-finite values; the four branches for Rust's saturating `f64 as isize`
in checkers; the six-clause no_spec shortcut around pow; shadow_irrelevant's -0 and NaN ambient; `equal(x, 0.0)`
(|x| < EPSILON) for the spawn rules against `x > 0.0` for the Schlick gate.

The yardstick is the checker of tests/csg_ref.py. This file holds, without a GPU, that every ray of every case is
inside the reference's domain (the checker finishes it: no NaN root, intersection.rs:113), that each case reaches
the branch it is named for at least 8 times by the checker's own count (`events`), and that the checker equals the
C oracle bit for bit on every case of kinds 0-4. tests/test_gpu_shading_edges.py sends the same cases to the GPU.

What the reference's own domain forced on the cases:
  * Matrix::inverse asserts |det| >= EPSILON (matrix.rs:134-139), so scaling(s, s, s) has s >= 0.0216 and a uniform
    pattern scale cannot multiply by more than 46. The magnitude cases take s = 2^-5 (pattern point = 32 x, exact)
    and rays at x up to 2^59; 1e300 and the inf entry need a non-uniform scale of determinant >= EPSILON. Each of
    these worlds holds a sphere beside the plane whose pattern is scaled the non-uniform way (two coordinates by
    2^64, one by 1e300, or the inf entry), so the branches are reached through a transformed shape's inverse too.
  * A world coordinate above 1.3e154 squares to inf, and a sphere's discriminant is then NaN (a NaN root), so
    1e300 is reached in pattern space only: x = 1e150 under scaling(1e-150, 1, 1e150).
  * On a plane the middle floor of checkers is floor(32 * 1e-5) = 0 or, from below, -1: the cancelling sum is
    2^63 + 0 + (-2^63) = 0 and 2^63 + (-1) + (-2^63), which binary64 also makes 0 (even) where integers make -1.
"""
import math

import numpy as np
import pytest

import csg_ref
import mesh_ref

EPS = 0.00001  # lib.rs:18
W, H = 24, 16
NEAR_EPS = float(np.nextafter(EPS, 0.0))
P53, P63 = 2.0 ** 53, 2.0 ** 63
INF = float("inf")


# ---------------------------------------------------------------- worlds
def _side(rt, w, at=(-40.0, 30.0, 40.0)):
    """Four diagonal spheres and a cube off to the side: the fast path is fused and builds its hierarchies."""
    for k in range(4):
        s = rt.glass_sphere() if k % 2 else rt.Sphere()
        s.set_transform(rt.translation(at[0] + 3.0 * k, at[1], at[2] + 2.0 * k) * rt.scaling(0.8, 0.8, 0.8))
        s.material.color = rt.Color(0.9, 0.4 + 0.1 * k, 0.2)
        w.add_object(s)
    c = rt.Cube()
    c.set_transform(rt.translation(at[0], at[1] + 4.0, at[2]) * rt.rotation_y(0.3) * rt.scaling(0.7, 0.5, 0.6))
    c.material.color = rt.Color(0.3, 0.6, 0.9)
    c.material.reflective = 0.2
    w.add_object(c)


def _light(rt, w, at=(-30.0, 40.0, -50.0), i=(1.0, 1.0, 1.0)):
    w.add_light(rt.PointLight(rt.Point(*at), rt.Color(*i)))


def _camera(rt, frm=(0.0, 6.0, -12.0), to=(0.0, 0.5, 0.0), fov=0.9):
    cam = rt.Camera(W, H, fov)
    cam.set_transform(rt.view_transform(rt.Point(*frm), rt.Point(*to), rt.Vector(0, 1, 0)))
    return cam


PATTERNS = {"test": 0, "stripe": 1, "gradient": 2, "ring": 3, "checkers": 4}
A_COL, B_COL = (0.9, 0.2, 0.1), (0.1, 0.3, 0.8)


def _pattern(rt, kind, transform=None):
    a, b = rt.Color(*A_COL), rt.Color(*B_COL)
    p = rt.test_pattern() if kind == "test" else getattr(rt, kind + "_pattern")(a, b)
    if transform is not None:
        p.set_transform(transform)
    return p


def _zero_like(v):  # a zero direction component with the sign of a zero origin: -0.0 + 0.0 * t would be +0.0
    return -0.0 if v == 0.0 and math.copysign(1.0, v) < 0 else 0.0


def _down(x, z, y=1.0, s=1.0):
    return [x, y, z, _zero_like(x), -s, _zero_like(z)]


def _up(x, z):
    return [x, -1.0, z, _zero_like(x), 1.0, _zero_like(z)]


def _around(vals):
    out = []
    for v in vals:
        for u in (v, float(np.nextafter(v, -INF)), float(np.nextafter(v, INF))):
            if not any(u == o and math.copysign(1.0, u) == math.copysign(1.0, o) for o in out):
                out.append(u)
    return out


LATTICE = _around([0.0, -0.0, 1.0, -1.0, 2.0, -2.0, 0.5, -0.5, -2.0 ** -60, -1e-300, 2.0 ** 31 - 1.0, 2.0 ** 31 + 1.0,
                   2.0 ** 52 + 1.0, P53, P53 + 2.0, -P53])
RING_POINTS = [(3.0, 4.0), (5.0, 12.0), (8.0, 15.0), (-3.0, 4.0), (5.0, -12.0), (-8.0, -15.0)]


# ---------------------------------------------------------------- what the checker saw
def _odd(f):  # of an integer-valued double below 2^53
    return math.fmod(f, 2.0) != 0.0


def tally_patterns(events, obj=None):
    """Counts over the pattern events (of object `obj` alone, if given)."""
    t = dict.fromkeys(("neg_odd_floor", "neg_zero", "ge_2p53", "fraction_one", "ring_exact", "ring_odd", "ring_ge_2p53",
                       "isize_max", "isize_below_min", "isize_min", "isize_nan", "cancel", "non_finite", "underside", "ring_inf", "xy_large",
                       "small_int"), 0)
    for e in events:
        if e[0] != "pattern" or (obj is not None and e[3] != obj):
            continue
        p = e[2]
        with np.errstate(all="ignore"):
            fx, fy, fz = (mesh_ref.floor(c) for c in p)
            t["non_finite"] += not all(math.isfinite(c) for c in p)
            t["neg_zero"] += any(c == 0.0 and math.copysign(1.0, c) < 0 for c in p)
            if math.isfinite(fx):
                t["neg_odd_floor"] += fx < 0.0 and abs(fx) < P53 and _odd(fx)
                t["small_int"] += abs(fx) < P53
                t["ge_2p53"] += abs(fx) >= P53
                t["fraction_one"] += (p[0] - fx) == 1.0
            t["underside"] += fy == -1.0
            d = math.sqrt(p[0] * p[0] + p[2] * p[2])
            t["ring_inf"] += d == INF
            if math.isfinite(d):
                t["ring_exact"] += d == mesh_ref.floor(d) and d > 0.0 and p[0] != 0.0 and p[2] != 0.0 and d * d == p[0] * p[0] + p[2] * p[2]
                t["ring_odd"] += d < P53 and _odd(mesh_ref.floor(d))
                t["ring_ge_2p53"] += d >= P53
            s = fx + fy + fz
            t["isize_nan"] += s != s
            t["isize_max"] += s >= P63
            t["isize_below_min"] += s < -P63
            t["isize_min"] += s == -P63
            t["cancel"] += abs(fx) >= P63 and abs(fz) >= P63 and abs(s) < P53
            t["xy_large"] += 2.0 ** 62 <= abs(fx) < INF and 2.0 ** 62 <= abs(fy) < INF
    return t


def no_spec_clauses(e):
    """The six clauses of lighting()'s no_spec (rt_device.hpp), in its order, on one lighting event; the intensity
    clause counts once per component."""
    i = e["intensity"]
    return {"specular_zero": e["specular"] == 0.0, "rde_le_1": e["reflect_dot_eye"] <= 1.0,
            "shininess_ge_0": e["shininess"] >= 0.0, "shininess_finite": e["shininess"] < INF,
            "intensity_x": abs(i[0]) < INF, "intensity_y": abs(i[1]) < INF, "intensity_z": abs(i[2]) < INF}


def no_spec(e):
    return all(no_spec_clauses(e).values())


def _plain(x):
    return x == x and not (x == 0.0 and math.copysign(1.0, x) < 0)


def tally_lighting(events):
    t = dict.fromkeys(("spec_branch", "no_spec", "ldn_zero", "spec0_rde_pos", "diffuse_neg_zero", "diffuse_pos_zero",
                       "shadow_skipped", "shadow_neg_zero", "shadow_nan", "shadow_patterned", "specular_nan"), 0)
    for k in ("specular_zero", "rde_le_1", "shininess_ge_0", "shininess_finite", "intensity_x", "intensity_y", "intensity_z"):
        t["only_" + k] = 0
    for e in events:
        if e[0] != "lighting":
            continue
        e = e[1]
        if e["light_dot_normal"] < 0.0:  # shadow_irrelevant's question (rt_trace.hpp)
            if e["patterned"]:
                t["shadow_patterned"] += 1
            elif any(c != c for c in e["ambient"]):
                t["shadow_nan"] += 1
            elif not all(_plain(c) for c in e["ambient"]):
                t["shadow_neg_zero"] += 1
            else:
                t["shadow_skipped"] += 1
        if e["in_shadow"]:
            continue
        t["ldn_zero"] += e["light_dot_normal"] == 0.0
        if e["diffuse_term"] is not None:
            t["diffuse_neg_zero"] += any(c == 0.0 and math.copysign(1.0, c) < 0 for c in e["diffuse_term"])
            t["diffuse_pos_zero"] += any(c == 0.0 and math.copysign(1.0, c) > 0 for c in e["diffuse_term"])
        if e["reflect_dot_eye"] is None or e["reflect_dot_eye"] <= 0.0:
            continue
        t["spec_branch"] += 1
        t["spec0_rde_pos"] += e["specular"] == 0.0
        t["specular_nan"] += any(c != c for c in e["specular_term"])
        cl = no_spec_clauses(e)
        t["no_spec"] += all(cl.values())
        for k, ok in cl.items():
            t["only_" + k] += (not ok) and all(v for j, v in cl.items() if j != k)
    return t


def tally_shade(events):
    t = dict.fromkeys(("schlick_black_reflection", "negative_reflection_sum", "refl_at_eps", "refl_below_eps", "transp_at_eps",
                       "transp_below_eps", "remaining_0", "cos_one", "grazing", "tir", "sin2_le_1_near", "sin2_gt_1_near",
                       "schlick_non_finite", "same_index", "negative_index", "refl_neg_zero"), 0)
    for e in events:
        if e[0] != "shade":
            continue
        e = e[1]
        r, tr, live = e["reflective"], e["transparency"], e["remaining"] > 0
        t["remaining_0"] += not live and (r != 0.0 or tr != 0.0)
        t["schlick_black_reflection"] += live and 0.0 < r < EPS and tr > 0.0 and not e["reflect"] and e["schlick"] is not None
        t["negative_reflection_sum"] += live and r <= -EPS and tr > 0.0 and e["reflect"] and e["schlick"] is None
        t["refl_at_eps"] += live and abs(r) == EPS and e["reflect"]
        t["refl_below_eps"] += live and 0.0 < abs(r) < EPS and not e["reflect"]
        t["transp_at_eps"] += live and abs(tr) == EPS and e["sin2_t"] is not None
        t["transp_below_eps"] += live and 0.0 < abs(tr) < EPS and e["sin2_t"] is None
        t["refl_neg_zero"] += r == 0.0 and math.copysign(1.0, r) < 0
        if e["sin2_t"] is not None:
            s2 = e["sin2_t"]
            t["cos_one"] += e["cos_i"] == 1.0
            t["grazing"] += abs(e["cos_i"]) < 0.05
            t["tir"] += s2 > 1.0
            t["sin2_le_1_near"] += 1.0 - 1e-12 < s2 <= 1.0
            t["sin2_gt_1_near"] += 1.0 < s2 < 1.0 + 1e-12
            t["same_index"] += e["n1"] == e["n2"] and e["n1"] != 1.0
            t["negative_index"] += e["n1"] < 0.0 or e["n2"] < 0.0
        t["schlick_non_finite"] += e["schlick"] is not None and not math.isfinite(e["schlick"])
    return t


def tally(events):
    t = tally_patterns(events)
    t.update(tally_lighting(events))
    t.update(tally_shade(events))
    return t


def run_checker(ref, rays, depth):
    """The checker's colours, counters and events for a batch; a ray outside the domain raises (a NaN root)."""
    ref.counts = dict.fromkeys(csg_ref.COUNTERS, 0)
    ref.events = []
    try:
        with np.errstate(all="ignore"):
            want = ref.color_at_batch(rays, depth)
        return want, dict(ref.counts), ref.events
    finally:
        ref.events = None


# ---------------------------------------------------------------- cases: dict(w, rays, depth, klass, need, cam)
def _case(w, rays, depth, need, klass="plain", cam=None, need_on=None):
    """`need`: the least counts over all events; `need_on`: {object: least counts over that object's pattern events}."""
    return dict(w=w, rays=np.array(rays, dtype=np.float64), depth=depth, klass=klass, need=need, cam=cam, need_on=need_on or {})


def _lattice_rays():
    n, rays = len(LATTICE), []
    for i, v in enumerate(LATTICE):
        rays += [_down(v, LATTICE[(5 * i + 7) % n]), _up(v, LATTICE[(7 * i + 3) % n]), _down(LATTICE[(3 * i + 1) % n], v)]
    return rays


LATTICE_NEED = {
    "test": {"underside": 8, "small_int": 8},
    "stripe": {"neg_odd_floor": 8, "ge_2p53": 8, "small_int": 8},
    "gradient": {"fraction_one": 8, "ge_2p53": 8},
    "ring": {"ring_odd": 8, "ring_ge_2p53": 8, "ring_exact": 8},
    "checkers": {"neg_odd_floor": 8, "underside": 8, "ge_2p53": 8},
}


def _case_lattice_plane(rt, kind):
    """Exact pattern points: o = (x, 1, z), d = (0, -1, 0) onto the plane y = 0 gives t = 1, the point (x, 0, z) and the
    over point (x, 1e-5, z) exactly; from below, (x, -1e-5, z). x and z from LATTICE. (Its -0.0 reaches the hit point,
    with a -0.0 direction component, but not the pattern: over = point + normal * EPSILON adds the normal's +0.0.)"""
    w = rt.World()
    p = rt.Plane()
    p.material.set_pattern(_pattern(rt, kind))
    p.material.specular = 0.0
    w.add_object(p)
    _side(rt, w)
    _light(rt, w)
    _light(rt, w, (20.0, -35.0, 10.0), (0.5, 1.0, 0.25))
    return _case(w, _lattice_rays(), 2, LATTICE_NEED[kind], cam=_camera(rt))


def _case_lattice_sphere(rt, kind):
    """The same lattice under a sphere of radius 4 whose pattern undoes the scale (object point = world / 4, pattern
    point = object * 4, both exact): vertical rays at the lattice values inside the disc. (A sphere that the values
    from 2^31 up could land on would have to hold the whole world inside it; they are held on the planes, and on the
    magnitude cases' spheres through the pattern's scale.) -0.0 reaches the pattern point here, from a -0.0 origin
    and direction component where the other coordinate is negative or -0.0 and the ray comes from above: every
    product the two matrices add to it is then -0.0 too (the inverses' zero entries carry signs). Test passes it on
    as a colour component, gradient takes -0 - floor(-0), the others fmod2_is_zero(-0.0)."""
    w = rt.World()
    s = rt.Sphere()
    s.set_transform(rt.scaling(4.0, 4.0, 4.0))
    s.material.set_pattern(_pattern(rt, kind, rt.scaling(0.25, 0.25, 0.25)))
    w.add_object(s)
    _side(rt, w)
    _light(rt, w)
    small = [v for v in LATTICE if abs(v) <= 2.5]
    rays = []
    for i, v in enumerate(small):
        rays += [_down(v, small[(5 * i + 3) % len(small)], 9.0), _down(small[(3 * i + 1) % len(small)], v, 9.0),
                 [v, -9.0, small[(7 * i + 2) % len(small)], 0.0, 1.0, 0.0]]
    for v in (-0.5, -1.0, -2.0, -0.25, -1.5, -2.5, -0.0, 0.5):
        rays += [_down(-0.0, v, 9.0), _down(v, -0.0, 9.0)]
    need = {"test": {"small_int": 8}, "stripe": {"neg_odd_floor": 8}, "gradient": {"neg_odd_floor": 8}, "ring": {"ring_odd": 8},
            "checkers": {"neg_odd_floor": 8}}[kind]
    return _case(w, rays, 2, dict(need, neg_zero=8), cam=_camera(rt))


def _case_underside(rt):
    """Checkers from below: over.y = -1e-5, floor -1, the parity of every square flips against the upper side."""
    w = rt.World()
    p = rt.Plane()
    p.material.set_pattern(_pattern(rt, "checkers"))
    w.add_object(p)
    _side(rt, w)
    _light(rt, w, (10.0, -40.0, -20.0))
    _light(rt, w)
    vals = [v for v in LATTICE if abs(v) < 4.0]
    rays = []
    for i, v in enumerate(vals):
        z = vals[(5 * i + 2) % len(vals)]
        rays += [_up(v, z), _down(v, z)]
    return _case(w, rays, 2, {"underside": 30, "neg_odd_floor": 8}, cam=_camera(rt, (0.0, -5.0, -10.0)))


def _case_ring_integers(rt):
    """Ring at radii that are exact integers (3-4-5, 5-12-13, 8-15-17), their neighbours, and (0, +-n)."""
    w = rt.World()
    p = rt.Plane()
    p.material.set_pattern(_pattern(rt, "ring"))
    w.add_object(p)
    _side(rt, w)
    _light(rt, w)
    rays = []
    for x, z in RING_POINTS:
        for xx in _around([x]):
            for zz in _around([z]):
                rays.append(_down(xx, zz))
    for n in range(1, 9):
        rays += [_down(0.0, float(n)), _down(0.0, -float(n)), _down(-0.0, float(np.nextafter(float(n), 0.0))), _up(float(n), -0.0)]
    return _case(w, rays, 2, {"ring_exact": 8, "ring_odd": 8}, cam=_camera(rt))


SPHERE_AT = (100.0, 6.0, 0.0)


def _scaled_sphere(rt, w, pattern):
    """The sphere of the magnitude cases (object 1, radius 4, beside the rays onto the plane) and vertical rays onto
    it from above and from below: object coordinates of 1/8 to 3/4 in x and z and of either sign in y, none 0."""
    s = rt.Sphere()
    s.set_transform(rt.translation(*SPHERE_AT) * rt.scaling(4.0, 4.0, 4.0))
    s.material.set_pattern(pattern)
    w.add_object(s)
    rays = []
    for dx in (-3.0, -1.5, -0.5, 0.5, 1.5, 3.0):
        for dz in (-2.0, -0.5, 0.5, 2.0):
            rays += [_down(SPHERE_AT[0] + dx, dz, 12.0), [SPHERE_AT[0] + dx, 0.5, dz, 0.0, 1.0, 0.0]]
    return rays


def _sphere_camera(rt):
    return _camera(rt, (SPHERE_AT[0] - 3.0, 9.0, -18.0), (SPHERE_AT[0], 3.0, 0.0), 0.8)


def _case_magnitude(rt, kind):
    """Pattern scaling(2^-5, 2^-5, 2^-5): the pattern point is 32 times the over point, exactly; x and z at +-2^57,
    2^58, 2^59 put it at 2^62, 2^63, 2^64 (checkers: sums >= 2^63, < -2^63, exactly -2^63, and cancelling). The sphere's
    pattern multiplies two coordinates by 2^64 and the third by 2^-132 (determinant 16; for ring x and z, else x and y):
    checkers sums two large floors of either sign there, through the sphere's own inverse. (A sum of exactly -2^63
    needs exact points: the plane alone has them.)"""
    w = rt.World()
    p = rt.Plane()
    p.material.set_pattern(_pattern(rt, kind, rt.scaling(2.0 ** -5, 2.0 ** -5, 2.0 ** -5)))
    w.add_object(p)
    on_sphere = _scaled_sphere(rt, w, _pattern(rt, kind, rt.scaling(2.0 ** -64, 2.0 ** 132, 2.0 ** -64) if kind == "ring"
                                               else rt.scaling(2.0 ** -64, 2.0 ** -64, 2.0 ** 132)))
    _side(rt, w)
    _light(rt, w)
    big = _around([2.0 ** 57, 2.0 ** 58, 2.0 ** 59, -2.0 ** 57, -2.0 ** 58, -2.0 ** 59])
    near = [0.0, 0.01, -0.01, 0.5, -0.5, 1.0 / 64.0, -1.0 / 64.0, 3.0 / 32.0]
    rays = []
    for i, v in enumerate(big):
        rays += [_down(v, near[i % 8]), _up(v, near[(i + 3) % 8]), _down(near[(i + 5) % 8], v), _down(v, -v), _up(v, -v),
                 _down(v, big[(5 * i + 1) % len(big)])]
    rays += [_down(-2.0 ** 58, k / 512.0) for k in range(12)]  # -2^63 + 0 + 0
    need = {"stripe": {"ge_2p53": 60}, "ring": {"ring_ge_2p53": 60},
            "checkers": {"isize_max": 8, "isize_below_min": 8, "isize_min": 8, "cancel": 8}}[kind]
    there = {"stripe": {"ge_2p53": 40}, "ring": {"ring_ge_2p53": 40},
             "checkers": {"isize_max": 8, "isize_below_min": 8, "xy_large": 8}}[kind]
    return _case(w, rays + on_sphere, 2, need, cam=_sphere_camera(rt), need_on={0: need, 1: there})


def _case_magnitude_1e300(rt, kind):
    """1e300 in pattern space: x = +-1e150 (its square is finite: a larger world coordinate makes a NaN root) under
    the pattern scaling(1e-150, 1, 1e150), of determinant 1; on the sphere, object x times 1e300 under
    scaling(1e-300, 1e150, 1e150)."""
    w = rt.World()
    p = rt.Plane()
    p.material.set_pattern(_pattern(rt, kind, rt.scaling(1e-150, 1.0, 1e150)))
    w.add_object(p)
    on_sphere = _scaled_sphere(rt, w, _pattern(rt, kind, rt.scaling(1e-300, 1e150, 1e150)))
    _side(rt, w)
    _light(rt, w)
    rays = []
    for i, v in enumerate(_around([1e150, -1e150, 1e149, -1e149])):
        rays += [_down(v, 0.5 * i), _up(v, -0.5 * i)]
    need = {"checkers": {"isize_max": 8, "isize_below_min": 8}, "stripe": {"ge_2p53": 16},
            "ring": {"ring_inf": 16}}[kind]  # (1e300 squared: ring's distance is inf, its non-finite rule)
    return _case(w, rays + on_sphere, 2, need, cam=_sphere_camera(rt), need_on={0: need, 1: need})


def _case_pattern_inf(rt, kind):
    """A pattern transform of determinant 1e-4 whose inverse holds +inf and -inf (scaling(1e-310, 1e153, 1e153) times
    a shear of y by x), on the plane and on the sphere: the pattern point is (+-inf, -+inf, tiny), or NaN at x = 0. Stripe and ring take their
    non-finite rule (inf % 2 is NaN: colour b), checkers sums inf - inf to NaN (`as isize` 0: colour a). Inside the
    domain: a colour enters no root."""
    w = rt.World()
    p = rt.Plane()
    p.material.set_pattern(_pattern(rt, kind, rt.scaling(1e-310, 1e153, 1e153) * rt.shearing(0.0, 0.0, 1.0, 0.0, 0.0, 0.0)))
    w.add_object(p)
    on_sphere = _scaled_sphere(rt, w, _pattern(rt, kind, rt.scaling(1e-310, 1e153, 1e153) * rt.shearing(0.0, 0.0, 1.0, 0.0, 0.0, 0.0)))
    _side(rt, w)
    _light(rt, w)
    inv = p.material.pattern.transform_inverse.to_list()
    assert inv[0] == INF and inv[4] == -INF and not any(v != v for v in inv)
    rays = []
    for i, v in enumerate([0.5, -0.5, 3.0, -3.0, 1e-300, -1e-300, 2.0 ** 31, -2.0 ** 31, 0.0, -0.0, 7.25, -7.25]):
        rays += [_down(v, 0.25 * i), _up(v, -0.25 * i)]
    need = {"non_finite": 24, "isize_nan": 24} if kind == "checkers" else {"non_finite": 24}
    return _case(w, rays + on_sphere, 2, need, cam=_sphere_camera(rt), need_on={0: need, 1: need})


def _case_parent_group(rt):
    """A striped, a checkered and a ringed sphere inside a rotated, scaled group: the leaf's own baked inverse takes
    the world point to the pattern (pattern/mod.rs:39-49)."""
    w = rt.World()
    g = rt.Group()
    for k, kind in enumerate(("stripe", "checkers", "ring", "gradient")):
        s = rt.Sphere()
        s.set_transform(rt.translation(-3.0 + 2.0 * k, 0.0, 0.3 * k) * rt.scaling(0.9, 0.8, 0.9))
        s.material.set_pattern(_pattern(rt, kind, rt.rotation_z(0.4) * rt.scaling(0.11, 0.13, 0.12)))
        g.add_child(s)
    g.set_transform(rt.translation(0.5, 1.0, 0.0) * rt.rotation_y(0.5) * rt.rotation_x(-0.3) * rt.scaling(1.5, 1.2, 1.1))
    w.add_object(g)
    _side(rt, w)
    _light(rt, w)
    rng = np.random.default_rng(5)
    o = np.tile([0.0, 3.0, -12.0], (240, 1))
    d = rng.uniform([-6.0, -0.5, 0.0], [6.0, 2.5, 0.0], size=(240, 3)) - o
    rays = np.hstack([o, d / np.linalg.norm(d, axis=1, keepdims=True)])
    return _case(w, rays, 2, {"neg_odd_floor": 8, "small_int": 30}, cam=_camera(rt, (0.0, 3.0, -12.0), (0.0, 1.0, 0.0), 0.8))


def _case_parent_triangle(rt):
    """A checkered triangle and a striped smooth triangle: the TRIS kernels' pattern_color."""
    w = rt.World()
    t = rt.Triangle(rt.Point(-4.0, 0.0, 3.0), rt.Point(4.0, 0.5, 3.0), rt.Point(0.0, 5.0, 2.0))
    t.material.set_pattern(_pattern(rt, "checkers", rt.scaling(0.3, 0.3, 0.3)))
    w.add_object(t)
    t = rt.SmoothTriangle(rt.Point(-4.0, 0.0, 1.0), rt.Point(4.0, 0.0, 1.0), rt.Point(0.0, -5.0, 2.0), rt.Vector(-0.3, 0.0, -1.0),
                          rt.Vector(0.3, 0.0, -1.0), rt.Vector(0.0, -0.3, -1.0))
    t.material.set_pattern(_pattern(rt, "stripe", rt.rotation_z(0.7) * rt.scaling(0.2, 0.2, 0.2)))
    w.add_object(t)
    _side(rt, w)
    _light(rt, w)
    rng = np.random.default_rng(6)
    o = np.tile([0.0, 0.5, -12.0], (120, 1))
    d = rng.uniform([-4.0, -5.0, 2.0], [4.0, 5.0, 2.0], size=(120, 3)) - o
    rays = np.hstack([o, d / np.linalg.norm(d, axis=1, keepdims=True)])
    return _case(w, rays, 2, {"neg_odd_floor": 8, "small_int": 30}, "tris", _camera(rt, (0.0, 0.5, -12.0), (0.0, 0.0, 2.0), 0.8))


# ---- the material table: a covering set
SHININESS = (0.0, 0.5, 1.0, 1e9, -3.0, INF)
SPECULAR = (0.0, -0.0, 1.0, -1.0)
AMBIENT = (0.0, -0.0, 1.0, 2.0)
DIFFUSE = (0.0, 1.0, -1.0)
COMPONENT = (0.0, -0.0, 1.0, 3.0, -1.0)
N_TABLE = 48


def _table_material(rt, m, k):
    """Material k of the covering set: shininess x specular in full (24), twice, over rotating ambient, diffuse and
    colour components."""
    m.shininess = SHININESS[k % 6]
    m.specular = SPECULAR[(k // 6) % 4]
    m.ambient = AMBIENT[(k + k // 24) % 4]
    m.diffuse = DIFFUSE[(k + k // 6) % 3]
    m.color = rt.Color(COMPONENT[k % 5], COMPONENT[(2 * k + 1) % 5], COMPONENT[(3 * k + 2) % 5])


def _case_table(rt, extra=None, inf_axis=0):  # inf_axis None: every intensity finite
    """48 spheres, one material each, on a plane, under three lights: in front (above), behind the surface (below the
    plane), and in the plane's tangent plane (light.y == over.y == 1e-5: light_dot_normal is 0.0 exactly), whose
    intensity holds +inf in one component (that channel is then inf or NaN on every ray, so each world comes a second
    time with a finite tangent light, which holds all three channels of every material). Vertical rays onto each sphere, off its axis both ways, one of them with
    a direction of length 8 (reflect_dot_eye above 1); vertical rays onto the plane between them. `extra` adds a
    triangle or a Csg unit: the TRIS and the TRIS, CSG kernels."""
    w = rt.World()
    p = rt.Plane()
    p.material.specular, p.material.shininess, p.material.color = 0.0, 0.5, rt.Color(1.0, -1.0, -0.0)
    w.add_object(p)
    rays = []
    for k in range(N_TABLE):
        cx, cz = 3.0 * (k % 8) - 10.5, 3.0 * (k // 8) - 7.5
        s = rt.Sphere()
        s.set_transform(rt.translation(cx, 1.0, cz))
        _table_material(rt, s.material, k)
        if k % 12 == 11:
            s.material.set_pattern(_pattern(rt, "stripe", rt.scaling(0.3, 0.3, 0.3)))
        w.add_object(s)
        for dx, dz, sc in ((0.0, 0.0, 1.0), (0.05, 0.05, 8.0), (0.55, 0.5, 1.0), (-0.6, -0.45, 1.0), (0.5, -0.62, 1.0),
                           (-0.58, 0.52, 8.0), (0.62, -0.4, 1.0)):
            rays.append(_down(cx + dx, cz + dz, 4.0, sc))
        rays.append(_down(cx + 1.5, cz + 1.5))
    if extra == "tri":
        t = rt.Triangle(rt.Point(-14.0, 0.5, -9.0), rt.Point(-13.0, 0.5, -9.0), rt.Point(-13.5, 0.5, -8.0))
        _table_material(rt, t.material, 7)
        w.add_object(t)
        rays += [_down(-13.5 + 0.02 * i, -8.7 + 0.01 * i, 4.0) for i in range(8)]
    if extra == "csg":
        a, b = rt.Sphere(), rt.Cube()
        b.set_transform(rt.translation(0.5, 0.5, 0.0) * rt.scaling(0.7, 0.7, 0.7))
        _table_material(rt, a.material, 13)
        _table_material(rt, b.material, 30)
        c = rt.Csg(rt.Operation.Difference, a, b)
        c.set_transform(rt.translation(-13.5, 1.0, -5.0))
        w.add_object(c)
        rays += [_down(-13.9 + 0.1 * i, -5.3 + 0.07 * i, 4.0) for i in range(8)]
    _side(rt, w)
    _light(rt, w, (-20.0, 30.0, -25.0), (1.0, 5.0, -1.0))
    _light(rt, w, (15.0, -30.0, 10.0), (1.0, 0.0, 5.0))
    tangent = [1.0, 1.0, 1.0]
    if inf_axis is not None:
        tangent[inf_axis] = INF
    _light(rt, w, (60.0, EPS, -45.0), tuple(tangent))
    need = {"no_spec": 8, "only_specular_zero": 8, "only_rde_le_1": 8, "only_shininess_ge_0": 8, "only_shininess_finite": 8,
            "ldn_zero": 8, "spec0_rde_pos": 8, "diffuse_neg_zero": 8,
            "diffuse_pos_zero": 8, "shadow_skipped": 8, "shadow_neg_zero": 8, "shadow_nan": 8, "shadow_patterned": 8,
            "specular_nan": 8}
    if inf_axis is None:
        del need["shadow_nan"]  # (a NaN ambient is 0 * inf)
    else:
        need["only_intensity_" + "xyz"[inf_axis]] = 8
    klass = {None: "plain", "tri": "tris", "csg": "csg"}[extra]
    return _case(w, rays, 1, need, klass, _camera(rt, (-2.0, 9.0, -22.0), (0.0, 0.5, 0.0), 0.8))


def _case_nospec_negative_shininess(rt):
    """Where the `shininess >= 0` clause of no_spec decides the colour: specular 0, shininess -3 and a
    reflect_dot_eye of 1e-120. The plane lies at y = -EPSILON and the rays start at y = EPSILON, so over.y is 0.0
    exactly; the light is 1e-120 above it, and reflect_dot_eye = lightv.y. pow gives inf, the specular term
    (I * 0) * inf is NaN; without the clause it would be 0."""
    w = rt.World()
    p = rt.Plane()
    p.set_transform(rt.translation(0.0, -EPS, 0.0))
    p.material.specular, p.material.shininess = 0.0, -3.0
    w.add_object(p)
    _side(rt, w)
    _light(rt, w, (0.0, 1e-120, 0.0), (1.0, 5.0, -1.0))
    rays = [_down(0.5 + 0.25 * i, -1.0 + 0.3 * j, EPS) for i in range(4) for j in range(4)]
    return _case(w, rays, 1, {"only_shininess_ge_0": 16, "specular_nan": 16}, cam=_camera(rt))


# ---- spawn thresholds
SPAWN = (0.0, -0.0, 5e-6, NEAR_EPS, EPS, -5e-6, -EPS, -0.5, 1.0, 1.5)


def _case_spawn(rt, depth):
    """reflective x transparency over SPAWN in full, one glass sphere each above a checkered floor, one ray each just
    off the axis. `equal(x, 0.0)` is |x| < EPSILON (world.rs:108, 117), the Schlick gate is x > 0.0 (world.rs:62)."""
    w = rt.World()
    f = rt.Plane()
    f.set_transform(rt.translation(0.0, -1.5, 0.0))
    f.material.set_pattern(_pattern(rt, "checkers", rt.scaling(0.7, 0.7, 0.7)))
    w.add_object(f)
    rays = []
    for i, r in enumerate(SPAWN):
        for j, t in enumerate(SPAWN):
            s = rt.glass_sphere()
            s.set_transform(rt.translation(3.0 * i - 13.5, 0.0, 3.0 * j - 13.5))
            s.material.reflective, s.material.transparency = r, t
            s.material.diffuse, s.material.ambient, s.material.color = 0.3, 0.1, rt.Color(0.2 + 0.08 * i, 0.9 - 0.08 * j, 0.5)
            w.add_object(s)
            rays.append(_down(3.0 * i - 13.5 + 0.31, 3.0 * j - 13.5 - 0.23, 4.0))
    _side(rt, w)
    _light(rt, w)
    need = {"remaining_0": 90} if depth == 0 else \
        {"schlick_black_reflection": 8, "negative_reflection_sum": 8, "refl_at_eps": 8, "refl_below_eps": 8, "transp_at_eps": 8,
         "transp_below_eps": 8, "refl_neg_zero": 8}
    return _case(w, rays, depth, need, cam=_camera(rt, (-1.0, 12.0, -30.0), (0.0, 0.0, 0.0), 0.9) if depth == 3 else None)


# ---- Schlick and refraction
NESTED = ((1.5, 1.5), (0.5, 1.5), (1.5, -1.5), (1e-3, 1e3), (1e3, 1e-3), (1.0, 0.5), (-1.5, 1.0), (1.5, 1.0))


def _case_schlick(rt):
    """Nested glass (an outer sphere of radius 2 around an inner one of radius 1) over NESTED's index pairs: vertical
    rays through the centre (cos_i = 1 exactly), off the axis, and grazing both spheres. Index -1.5 against 1.5 makes
    Schlick's (n1 - n2) / (n1 + n2) a division by zero (inf, then a NaN colour)."""
    w = rt.World()
    f = rt.Plane()
    f.set_transform(rt.translation(0.0, -3.0, 0.0))
    f.material.set_pattern(_pattern(rt, "checkers"))
    w.add_object(f)
    rays = []
    for k, (no, ni) in enumerate(NESTED):
        cx = 6.0 * k - 21.0
        for r, n in ((2.0, no), (1.0, ni)):
            s = rt.glass_sphere()
            s.set_transform(rt.translation(cx, 0.0, 0.0) * rt.scaling(r, r, r))
            s.material.refractive_index, s.material.reflective, s.material.diffuse = n, 0.6, 0.2
            w.add_object(s)
        for dx in (0.0, 0.0, 0.4, -0.7, 0.97, 0.9999, -0.99999, 1.3, 1.9, -1.9995, 1.99999):
            rays.append(_down(cx + dx, 0.0, 5.0))
        rays[-10][2] = -0.0
    _side(rt, w)
    _light(rt, w)
    need = {"cos_one": 8, "grazing": 8, "tir": 8, "schlick_non_finite": 8, "same_index": 8, "negative_index": 8}
    return _case(w, rays, 4, need, cam=_camera(rt, (0.0, 7.0, -32.0), (0.0, 0.0, 0.0), 1.2))


def _case_critical(rt):
    """sin2_t at 1.0: rays from inside a unit glass sphere of index 1.5, from (a, 0, 0) along +y, meet the surface
    with sin^2 = a^2, and sin2_t = 2.25 a^2 crosses 1.0 at a = 2/3. Forty neighbours of 2/3, one ulp apart: the
    checker says which land on which side of the `> 1.0` test."""
    w = rt.World()
    s = rt.glass_sphere()
    s.material.reflective = 0.4
    w.add_object(s)
    f = rt.Plane()
    f.set_transform(rt.translation(0.0, 5.0, 0.0))
    f.material.set_pattern(_pattern(rt, "stripe", rt.scaling(0.05, 0.05, 0.05)))
    w.add_object(f)
    _side(rt, w)
    _light(rt, w, (3.0, 2.0, -8.0))
    a, rays = 2.0 / 3.0, []
    for _ in range(20):
        a = float(np.nextafter(a, 0.0))
    for _ in range(40):
        rays.append([a, 0.0, 0.0, 0.0, 1.0, 0.0])
        a = float(np.nextafter(a, 1.0))
    return _case(w, rays, 2, {"sin2_le_1_near": 8, "sin2_gt_1_near": 8, "tir": 8}, cam=_camera(rt, (0.0, 2.0, -6.0), (0.0, 0.5, 0.0)))


CASES = {
    "table_plain": lambda rt: _case_table(rt, None, 0),
    "table_tris": lambda rt: _case_table(rt, "tri", 1),
    "table_csg": lambda rt: _case_table(rt, "csg", 2),
    "table_plain_finite": lambda rt: _case_table(rt, None, None),
    "table_tris_finite": lambda rt: _case_table(rt, "tri", None),
    "table_csg_finite": lambda rt: _case_table(rt, "csg", None),
    "nospec_negative_shininess": _case_nospec_negative_shininess,
    "spawn_remaining_0": lambda rt: _case_spawn(rt, 0),
    "spawn_remaining_1": lambda rt: _case_spawn(rt, 1),
    "spawn_remaining_3": lambda rt: _case_spawn(rt, 3),
    "schlick_nested": _case_schlick,
    "schlick_critical": _case_critical,
    "underside_checkers": _case_underside,
    "ring_integers": _case_ring_integers,
    "parent_group": _case_parent_group,
    "parent_triangle": _case_parent_triangle,
}
for _k in PATTERNS:
    CASES["lattice_plane_" + _k] = lambda rt, k=_k: _case_lattice_plane(rt, k)
    CASES["lattice_sphere_" + _k] = lambda rt, k=_k: _case_lattice_sphere(rt, k)
for _k in ("stripe", "ring", "checkers"):
    CASES["magnitude_" + _k] = lambda rt, k=_k: _case_magnitude(rt, k)
    CASES["magnitude_1e300_" + _k] = lambda rt, k=_k: _case_magnitude_1e300(rt, k)
    CASES["pattern_inf_" + _k] = lambda rt, k=_k: _case_pattern_inf(rt, k)


def check_inputs(case, ref):
    """Every ray inside the domain (the checker finishes it; its intersect raises on a NaN root), no material field
    NaN, no refractive index 0, and the named branches reached by the checker's count. Returns the checker's answer."""
    assert len(case["rays"]) <= 400 and case["depth"] <= 4
    s = ref.s
    for f in ("ambient", "diffuse", "specular", "shininess", "reflective", "transparency", "refractive_index", "color"):
        assert not np.isnan(s[f]).any(), f
    assert (s["refractive_index"] != 0.0).all()
    want, counts, events = run_checker(ref, case["rays"], case["depth"])
    t = tally(events)
    for k, n in case["need"].items():
        assert t[k] >= n, (k, t[k], n)
    for obj, need in case["need_on"].items():
        on = tally_patterns(events, obj)
        for k, n in need.items():
            assert on[k] >= n, (obj, k, on[k], n)
    return want, counts, t


@pytest.mark.parametrize("name", sorted(CASES))
def test_inputs_meet_the_conditions_of_their_case(rt, name):
    case = CASES[name](rt)
    check_inputs(case, csg_ref.CsgRef.from_world(case["w"]))


def test_the_cases_together_reach_every_outcome(rt):
    """Every outcome of no_spec (all six clauses, and each one as the only one that fails, the intensity clause per
    component) and of shadow_irrelevant over the three table worlds together."""
    total = {}
    for name in ("table_plain", "table_tris", "table_csg"):
        case = CASES[name](rt)
        _, _, t = check_inputs(case, csg_ref.CsgRef.from_world(case["w"]))
        for k, v in t.items():
            total[k] = total.get(k, 0) + v
    for k in ("no_spec", "only_specular_zero", "only_rde_le_1", "only_shininess_ge_0", "only_shininess_finite", "only_intensity_x",
              "only_intensity_y", "only_intensity_z", "shadow_skipped", "shadow_neg_zero", "shadow_nan", "shadow_patterned"):
        assert total[k] >= 8, (k, total[k])


def render_x4(ref, camera_desc, depth):
    """render_multithreaded with AASamples.X4 by the checker: the four sample rays of camera.rs:71-126, folded from
    black and scaled by 1 / 4 (Color::average, color.rs:26-33)."""
    c = np.frombuffer(camera_desc, dtype=csg_ref.CAMERA)[0]
    inv = [float(v) for v in c["inverse"]]
    out = np.zeros((int(c["vsize"]), int(c["hsize"]), 3))
    origin = csg_ref.mat_point(inv, (0.0, 0.0, 0.0))
    with np.errstate(all="ignore"):
        for y in range(out.shape[0]):
            for x in range(out.shape[1]):
                total = (0.0, 0.0, 0.0)
                for ox, oy in ((0.25, 0.25), (0.75, 0.25), (0.25, 0.75), (0.75, 0.75)):
                    world_x = float(c["half_width"]) - (float(x) + ox) * float(c["pixel_size"])
                    world_y = float(c["half_height"]) - (float(y) + oy) * float(c["pixel_size"])
                    pixel = csg_ref.mat_point(inv, (world_x, world_y, -1.0))
                    col = ref.color_at(origin, csg_ref.normalize(csg_ref.sub(pixel, origin)), depth)
                    total = (total[0] + col[0], total[1] + col[1], total[2] + col[2])
                out[y, x] = (total[0] * (1.0 / 4.0), total[1] * (1.0 / 4.0), total[2] * (1.0 / 4.0))
    return out


FRAME_DEPTH = 3
# one frame per world (the three spawn cases share one world: its frame comes with spawn_remaining_3)
FRAMES = sorted(k for k in CASES if k not in ("spawn_remaining_0", "spawn_remaining_1"))


def render_checker(ref, cam):
    """The checker's frame, its counters and its X4 frame; a pixel outside the domain raises."""
    with np.errstate(all="ignore"):
        img, rst = ref.render(cam.desc_bytes(), FRAME_DEPTH)
    return img, rst, render_x4(ref, cam.desc_bytes(), FRAME_DEPTH)


@pytest.mark.parametrize("name", FRAMES)
def test_frames_are_inside_the_domain(rt, name):
    case = CASES[name](rt)
    img, rst, aa = render_checker(csg_ref.CsgRef.from_world(case["w"]), case["cam"])
    assert rst["rays_primary"] == W * H and rst["rays_shadow"] > 32 and len(np.unique(img.reshape(-1, 3), axis=0)) > 8


def same(a, b):
    """Bit for bit, but for which NaN it is (Rust defines neither its sign nor its payload)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and a[~nan].tobytes() == b[~nan].tobytes()


@pytest.mark.parametrize("name", sorted(CASES))
def test_no_spec_shortcut_is_exact_on_every_event(rt, name):
    """lighting()'s shortcut, restated: where no_spec holds the specular term is intensity * specular, and that must
    be the reference's (intensity * specular) * pow(...) bit for bit on every event of every case."""
    case = CASES[name](rt)
    _, _, events = run_checker(csg_ref.CsgRef.from_world(case["w"]), case["rays"], case["depth"])
    n = 0
    for e in events:
        if e[0] != "lighting" or e[1]["reflect_dot_eye"] is None or e[1]["reflect_dot_eye"] <= 0.0:
            continue
        e = e[1]
        if no_spec(e):
            n += 1
            assert same(mesh_ref.scale(e["intensity"], e["specular"]), e["specular_term"]), e
    assert n > 0 or "table" not in name


def _kinds_0_to_4(ref):
    return bool((ref.s["kind"] <= 4).all()) and not (ref.nodes["kind"] == csg_ref.NODE_CSG).any()


NOT_FOR_THE_ORACLE = ("parent_triangle", "table_csg", "table_tris", "table_csg_finite", "table_tris_finite")  # a triangle or a Csg: the C oracle has neither


def test_the_oracle_is_spared_only_what_it_cannot_hold(rt):
    for name in NOT_FOR_THE_ORACLE:
        case = CASES[name](rt)
        assert not _kinds_0_to_4(csg_ref.CsgRef.from_world(case["w"])) and case["klass"] != "plain"


@pytest.mark.parametrize("name", sorted(set(CASES) - set(NOT_FOR_THE_ORACLE)))
def test_checker_equals_oracle(rt, oracle, name):
    """Two independent restatements of the reference, one in Python and one in C, bit for bit (NaN ~ NaN) on colours
    and counters, on every case made of kinds 0-4."""
    case = CASES[name](rt)
    ref = csg_ref.CsgRef.from_world(case["w"])
    assert _kinds_0_to_4(ref) and case["klass"] == "plain"
    want, counts, _ = run_checker(ref, case["rays"], case["depth"])
    got, st = oracle.OracleWorld.from_world(case["w"]).color_at_batch(case["rays"], case["depth"])
    bad = [i for i in range(len(want)) if not same(got[i], want[i])]
    assert not bad, (bad[:5], got[bad[0]], want[bad[0]], case["rays"][bad[0]])
    for k in csg_ref.COUNTERS:
        assert st[k] == counts[k], (k, st[k], counts[k])
