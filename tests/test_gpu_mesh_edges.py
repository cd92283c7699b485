"""The triangle hierarchy (tri_trace, rt_bvh.cpp tri_box) at the edges its box
padding was argued for (DESIGN.md 5.2 "Triangles"): axis-aligned triangles
(boxes of zero thickness) and exact ties, rays the slab test cannot divide for,
roots at |det| just above EPSILON that the reference accepts outside the exact
vertex box, origins and directions at and past kTriOriginMax / kTriDirMax (the
every-record loop), the 16-record threshold, records without a box, and
triangles as containers and as blockers of shadow rays.

The instrument: w.color_at_batch(rays, depth, True, exhaustive), fast against
exhaustive against the checker of tests/csg_ref.py (pinned by
tests/test_csg_ref.py), colours and the counters in COUNTS bit for bit, at
depths 0 and 2 (3 for the glass octahedron). Every world has two diagonal glass
spheres (so a fused render does not depend on the triangles) and a floor unless
the case says otherwise, and every case asserts the plan["triangles"] readout of
the fast call, so it fails if it did not reach the walk it was written for.

What the cases can and cannot show (mutations tried on an MI355X, not kept):
forcing t_lo = 0 for radiance rays in tri_trace fails `containers` (and
test_gpu_mesh.py's frames). Dropping the kTriOriginMax fallback, and replacing
tri_box's widening and pad_axis with the bare vertex box, fail nothing here:
the binary32 slab test widens every plane by 2^-20 (M + |o|) / |d| on its own
(slab_ray), a thousand times the padding bound of DESIGN.md 5.2 at these sizes
and 10^6 times the 1.8e-12 by which the roots of `grazing16000` leave the exact
box, and a ray that meets a box anywhere before t_hi enters it. The double
padding is generous; these cases pin the results it must keep, not its size.

Each case's conditions on its own inputs (how many rays tie, how many roots
fall outside the exact box, how many rays an unboxed triangle wins, how many
refract) are computed from the checker alone; the unmarked test_inputs_* hold
them without a GPU, and the GPU tests hold them again on the rays they send.
"""
import math

import numpy as np
import pytest

import csg_ref

COUNTS = ("rays_primary", "rays_reflect", "rays_refract", "rays_shadow", "sphere_tests", "plane_tests", "other_tests")
EYE = (1.3, 2.1, -5.0)
K_TRI_ORIGIN_MAX, K_TRI_DIR_MAX = 16384.0, 2.0  # rt_layout.hpp kTriOriginMax, kTriDirMax


# ---------------------------------------------------------------- worlds
def _world(rt, spheres=True, lights=((-6, 8, -8, 1.0), (5, 6, -4, 0.35))):
    w = rt.World()
    floor = rt.Plane()
    floor.set_transform(rt.translation(0, -2.0, 0))
    floor.material.reflective = 0.3
    floor.material.color = rt.Color(0.8, 0.8, 0.7)
    w.add_object(floor)
    if spheres:
        for c, r, idx in (((6.5, 0.0, 1.5), 0.8, 1.5), ((-3.0, 0.5, 2.5), 0.7, 1.33)):
            s = rt.glass_sphere()
            s.set_transform(rt.translation(*c) * rt.scaling(r, r, r))
            s.material.refractive_index = idx
            s.material.reflective = 0.4
            w.add_object(s)
    for x, y, z, i in lights:
        w.add_light(rt.PointLight(rt.Point(x, y, z), rt.Color(i, i, i)))
    return w


def _tri(rt, p1, p2, p3, color, k=0):
    t = rt.Triangle(rt.Point(*p1), rt.Point(*p2), rt.Point(*p3))
    t.material.color = rt.Color(*color)
    if k % 5 == 3:
        t.material.reflective = 0.4
    return t


def _grid(rt, w, plane, nx=4, ny=4):
    """nx x ny unit quads with corners at the integers, in the plane z = 0 (over x, y) or x = 0 (over y, z):
    2 nx ny loose triangles, each with its own colour, so the winner of a tie shows."""
    at = (lambda a, b: (float(a), float(b), 0.0)) if plane == "z" else (lambda a, b: (0.0, float(a), float(b)))
    k = 0
    for i in range(nx):
        for j in range(ny):
            for corners in (((i, j), (i + 1, j), (i + 1, j + 1)), ((i, j), (i + 1, j + 1), (i, j + 1))):
                col = (0.1 + 0.8 * ((k * 7) % 32) / 31.0, 0.1 + 0.8 * ((k * 11) % 32) / 31.0, 0.9 if plane == "z" else 0.2)
                w.add_object(_tri(rt, *(at(*c) for c in corners), col, k))
                k += 1


def _lattice():
    """The half-integer lattice of grid 1: its vertices, edge midpoints and diagonal midpoints (81 points)."""
    return [(0.5 * i, 0.5 * j, 0.0) for i in range(9) for j in range(9)]


def _toward(origin, targets, normalised):
    o = np.tile(np.asarray(origin, dtype=np.float64), (len(targets), 1))
    d = np.asarray(targets, dtype=np.float64) - o
    if normalised:
        d = d / np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])[:, None]
    return np.hstack([o, d])


def _tied(ref, rays):
    """Rays that meet two or more triangles at a bit-equal t; the largest number of triangles that accept one ray."""
    kinds, n, most = ref.s["kind"], 0, 0
    for r in rays:
        ts = [x[0] for x in ref.intersect(r[:3], r[3:]) if kinds[x[1]] >= 5]
        most = max(most, len(ts))
        n += len(set(ts)) < len(ts)
    return n, most


def _winners(ref, rays):
    """The object each ray's hit lands on (-1: none), from the checker."""
    out = []
    for r in rays:
        h = next((x for x in ref.intersect(r[:3], r[3:]) if x[0] >= 0.0), None)
        out.append(-1 if h is None else h[1])
    return np.array(out)


# ---------------------------------------------------------------- the cases: (world, rays, depths, readout, conditions)
def _case_ties(rt):
    """1. Zero-thickness boxes and exact ties."""
    w = _world(rt)
    _grid(rt, w, "z")
    _grid(rt, w, "x")
    rays = np.vstack([_toward(EYE, _lattice(), False), _toward(EYE, _lattice(), True)])
    assert len(rays) == 162

    def cond(ref):
        n, most = _tied(ref, rays)
        assert n >= 60 and most >= 6, (n, most)  # (measured: 106 rays, up to six triangles on one ray)
    return w, rays, (0, 2), dict(records=64, ran=True), cond


def _case_no_division(rt):
    """2. Rays the slab test cannot divide for: directions with one or two components exactly 0 toward both
    grids, origins on a grid line's coordinate, rays lying in the plane z = 0 (every |det| < EPSILON there:
    grid 1 vanishes), origins on a triangle (the root is t == 0)."""
    w = _world(rt)
    _grid(rt, w, "z")
    _grid(rt, w, "x")
    rays = []
    for a in np.arange(0.0, 4.01, 0.25):  # (every other one on a grid line's coordinate)
        for b in (0.0, 0.7, 2.0, 3.25, 4.0):
            rays.append((a, b, -5.0, 0.0, 0.0, 1.0))      # two zero components, toward grid 1
            rays.append((b, a, 3.0, 0.0, 0.0, -2.0))
            rays.append((5.0, a, b, -1.0, 0.0, 0.0))      # ... toward grid 2
            rays.append((a, b - 1.5, -5.0, 0.0, 0.3, 1.0))  # one zero component
            rays.append((a - 2.0, b, -5.0, 0.4, 0.0, 1.0))
            rays.append((5.0, a, b - 0.6, -1.0, 0.0, 0.12))
            rays.append((5.0, a - 1.0, b, -1.0, 0.2, 0.0))
    n_plane0 = len(rays)
    for y0 in (-0.5, 0.0, 0.5, 1.0, 2.25, 4.0):  # in the plane z = 0
        for s in (0.0, 0.25, -0.5, 1.0):
            rays.append((-2.0, y0, 0.0, 1.0, s, 0.0))
            rays.append((6.0, y0, 0.0, -0.6, 0.8 * s, 0.0))
    n_plane1 = len(rays)
    for x, y, z in _lattice()[::3]:  # origins on a triangle of grid 1
        for d in ((0.3, 0.2, 1.0), (0.0, 0.0, 1.0), (0.0, 0.0, -1.0), (-0.4, 0.1, -0.9)):
            rays.append((x, y, z) + d)
    rays = np.array(rays, dtype=np.float64)

    def cond(ref):
        kinds = ref.s["kind"]
        grid1 = {int(i) for i in np.flatnonzero(kinds >= 5)[:32]}
        for r in rays[n_plane0:n_plane1]:  # the mesh vanishes: no root on grid 1 at all
            assert not [x for x in ref.intersect(r[:3], r[3:]) if x[1] in grid1]
        zero = sum(1 for r in rays[n_plane1:] if any(x[0] == 0.0 and x[1] in grid1 for x in ref.intersect(r[:3], r[3:])))
        assert zero >= 80, zero
        win = _winners(ref, rays[:n_plane0])
        assert (kinds[win[win >= 0]] >= 5).sum() >= 300
    return w, rays, (0, 2), dict(records=64, ran=True), cond


KAT = ((0.0, 1.0, 0.0), (-1.0, 0.0, 0.0), (1.0, 0.0, 0.0))  # triangle.rs:105-120


def _case_grazing(rt, R):
    """3. Roots the reference accepts outside the exact box: rays aimed at points on an edge, and at a vertex,
    of the KAT triangle among 16 boxed triangles, |det| = 2 |d.z| in [1e-5, 4e-5], from 0.5 R to R away."""
    w = _world(rt)
    w.add_object(_tri(rt, *KAT, (0.9, 0.2, 0.2)))
    rng = np.random.default_rng(int(R))
    for k in range(15):
        c = rng.uniform([-4, 2.5, -3], [4, 5, 3])
        p = [tuple(c + rng.uniform(-0.6, 0.6, 3)) for _ in range(3)]
        w.add_object(_tri(rt, *p, tuple(rng.uniform(0.1, 0.9, 3)), k))
    n = 2000
    v = np.array(KAT)
    # (the exact box is [-1, 1] x [0, 1] x {0}: the edge p2-p3 and the three vertices lie on its faces, so a root
    # there can fall outside it in x or y; one in four rays goes to the other two edges, inside the box)
    e = np.where(rng.uniform(0, 1, n) < 0.75, 1, rng.integers(0, 3, n))
    s = rng.uniform(0, 1, n)
    s[: n // 8] = 0.0  # at a vertex
    e[: n // 8] = rng.integers(0, 3, n // 8)
    target = v[e] * (1 - s)[:, None] + v[(e + 1) % 3] * s[:, None]
    a = rng.uniform(0, 2 * math.pi, n)
    dz = rng.uniform(0.5e-5, 2e-5, n) * rng.choice([-1.0, 1.0], n)
    d = np.stack([np.cos(a), np.sin(a), dz], axis=1)
    d = d / np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])[:, None]
    o = target - d * rng.uniform(0.5 * R, R, n)[:, None]
    rays = np.hstack([o, d])
    assert np.abs(o).max() <= K_TRI_ORIGIN_MAX and ((1e-5 <= 2 * np.abs(d[:, 2])) & (2 * np.abs(d[:, 2]) <= 4e-5)).all()

    def cond(ref):
        kat = int(np.flatnonzero(ref.s["kind"] >= 5)[0])
        outside = accepted = 0
        for r in rays:
            for x in ref.intersect(r[:3], r[3:]):
                if x[1] == kat:
                    accepted += 1
                    px, py = r[0] + x[0] * r[3], r[1] + x[0] * r[4]  # (z: the exact box has no thickness at all)
                    outside += not (-1.0 <= px <= 1.0 and 0.0 <= py <= 1.0)
        # measured: R = 8: 91 of 1197 accepted roots outside, by up to 8.9e-16; R = 1000: 80 of 1005, 1.1e-13;
        # R = 16000: 75 of 1024, 1.8e-12
        assert accepted >= 500 and outside >= 50, (accepted, outside)
    return w, rays, (0, 2), dict(records=16, ran=True), cond


def _case_limits(rt):
    """4. The walk's limits: the rays of case 1 to grid 1 from |o|_inf in {16383, 16384, 16385, 1e6} and with
    |d|_inf in {1.9, 2.0, 2.1, 50}; past kTriOriginMax and kTriDirMax they take the every-record loop."""
    w = _world(rt)
    _grid(rt, w, "z")
    rays = []
    for far in (16383.0, 16384.0, 16385.0, 1e6):
        r = _toward((EYE[0], EYE[1], -far), _lattice(), True)
        assert np.abs(r[:, :3]).max() == far
        rays.append(r)
    for big in (1.9, 2.0, 2.1, 50.0):
        r = _toward(EYE, _lattice(), True)
        r[:, 3:] = r[:, 3:] / r[:, 5:6] * big  # (z is every direction's largest component: exactly `big`)
        assert (np.abs(r[:, 3:]).max(axis=1) == big).all()
        rays.append(r)
    rays = np.vstack(rays)
    om, dm = np.abs(rays[:, :3]).max(axis=1), np.abs(rays[:, 3:]).max(axis=1)
    assert ((om > K_TRI_ORIGIN_MAX) | (dm > K_TRI_DIR_MAX)).sum() == 4 * 81 and len(rays) == 8 * 81

    def cond(ref):
        win = _winners(ref, rays)
        assert (ref.s["kind"][win[win >= 0]] >= 5).sum() >= 500
    return w, rays, (0, 2), dict(records=32, ran=True), cond


def _random_triangles(rt, w, n, seed):
    """n random triangles around the square [0, 4]^2 of the plane z = 0; their vertices."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        c = rng.uniform([0, 0, -0.5], [4, 4, 0.5])
        p = [tuple(c + rng.uniform(-0.9, 0.9, 3)) for _ in range(3)]
        w.add_object(_tri(rt, *p, tuple(rng.uniform(0.1, 0.9, 3)), k))
        out.append(p)
    return np.array(out)


def _fan_rays(n, seed, tris):
    """n unit rays from in front of the triangles `tris`, each toward a point near a random one of them."""
    rng = np.random.default_rng(seed)
    o = rng.uniform([-3, -1, -7], [5, 5, -4], size=(n, 3))
    b = rng.dirichlet((1.0, 1.0, 1.0), n)
    t = tris[rng.integers(0, len(tris), n)]
    target = t[:, 0] * b[:, :1] + t[:, 1] * b[:, 1:2] + t[:, 2] * b[:, 2:] + rng.uniform(-0.3, 0.3, size=(n, 3))
    return _toward_each(o, target)


def _toward_each(o, targets):
    d = targets - o
    d = d / np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])[:, None]
    return np.hstack([o, d])


def _case_threshold(rt, n_tri, spheres=True):
    """5. The thresholds: n_tri boxed triangles beside the two spheres (fewer than 16 stay in the exhaustive
    remainder), or alone with the floor (theirs is the only hierarchy)."""
    w = _world(rt, spheres)
    rays = _fan_rays(300, n_tri, _random_triangles(rt, w, n_tri, n_tri))
    records = n_tri if (n_tri >= 16 or not spheres) else 0

    def cond(ref):
        win = _winners(ref, rays)
        assert (ref.s["kind"][win[win >= 0]] >= 5).sum() >= (100 if n_tri >= 15 else 25)
    return w, rays, (0, 2), dict(records=records, ran=records > 0), cond


def _unboxed_world(rt):
    w = _world(rt)
    tris = _random_triangles(rt, w, 17, 6)
    thin = _tri(rt, (-2000.0, 0.5, 0.0), (2000.0, 0.5, 1e-4), (0.0, 1.5, 2e-4), (0.2, 0.9, 0.9))  # x 1e-4, z 1e4
    thin.set_transform(rt.translation(-2.2, 2.0, 1.0) * rt.scaling(1e-4, 1.0, 1e4))  # cond 1e8: no box
    w.add_object(thin)
    w.add_object(_tri(rt, (-1500.0, -1.5, 6.0), (1500.0, -1.5, 6.0), (0.0, 2598.0, 6.0), (0.9, 0.9, 0.3)))  # edges of 3000
    return w, tris


def _case_unboxed(rt):
    """6. Records without a box: a triangle whose inverse fails cond <= 1e6 and one whose kappa bound passes
    1e12 (edges of 3000 units) stay in the exhaustive remainder beside 17 boxed ones."""
    w, tris = _unboxed_world(rt)
    rng = np.random.default_rng(66)
    o = rng.uniform([-3, 0, -7], [5, 4, -4], size=(400, 3))
    t = rng.uniform([-2.4, 2.5, 1.0], [-2.0, 3.5, 3.0], size=(400, 3))  # the thin one
    t[200:] = rng.uniform([-9, -1, 6], [9, 8, 6], size=(200, 3))        # the wall-sized one
    rays = np.vstack([_fan_rays(200, 66, tris), _toward_each(o, t)])

    def cond(ref):
        win = _winners(ref, rays)
        tri = np.flatnonzero(ref.s["kind"] >= 5)
        assert (win == tri[17]).sum() >= 10 and (win == tri[18]).sum() >= 10, ((win == tri[17]).sum(), (win == tri[18]).sum())
        assert np.isin(win, tri[:17]).sum() >= 60
    return w, rays, (0, 2), dict(records=17, ran=True), cond


OCTA_C, OCTA_R = (1.0, 1.0, -1.5), 0.8


def _case_containers(rt):
    """7. Containers and blockers: a closed glass octahedron (8 triangles, index 1.5) in a group beside a
    16-triangle mesh in the plane z = 0; half the origins inside it, so triangles behind the origin set n1 and
    n2. One light lies in that plane and one between the origins and the octahedron: [0, distance)."""
    w = _world(rt, lights=((9.0, 5.0, 0.0, 0.9), (0.6, 1.2, -3.2, 0.4)))
    g = rt.Group()
    c = np.array(OCTA_C)
    for sx in (-1, 1):
        for sy in (-1, 1):
            for sz in (-1, 1):
                p = [tuple(c + OCTA_R * np.array(v)) for v in ((sx, 0, 0), (0, sy, 0), (0, 0, sz))]
                t = rt.Triangle(*(rt.Point(*q) for q in p))
                t.material.color = rt.Color(0.1, 0.1, 0.15)
                t.material.diffuse, t.material.transparency, t.material.reflective = 0.2, 0.9, 0.3
                t.material.refractive_index = 1.5
                g.add_child(t)
    k = 0
    for i in range(4):
        for j in range(2):
            for corners in (((i, j), (i + 1, j), (i + 1, j + 1)), ((i, j), (i + 1, j + 1), (i, j + 1))):
                g.add_child(_tri(rt, *((float(a), float(b), 0.0) for a, b in corners),
                                 (0.2 + 0.1 * (k % 8), 0.9 - 0.1 * (k % 7), 0.5), k))
                k += 1
    w.add_object(g)
    rng = np.random.default_rng(77)
    n = 400
    o = rng.uniform([-2, 0, -6], [4, 3, -3.5], size=(n, 3))
    inside = rng.uniform(-1, 1, size=(n // 2, 3))
    inside = inside / np.abs(inside).sum(axis=1, keepdims=True) * rng.uniform(0.05, 0.9, size=(n // 2, 1))
    o[: n // 2] = c + OCTA_R * inside
    t = c + rng.uniform(-0.9, 0.9, size=(n, 3))
    t[: n // 2] = rng.uniform([-0.5, -0.5, -0.5], [4.5, 2.5, 0.5], size=(n // 2, 3))
    rays = _toward_each(o, t)

    def cond(ref):
        ref.counts = dict.fromkeys(csg_ref.COUNTERS, 0)
        ref.color_at_batch(rays, 3)
        assert ref.counts["rays_refract"] >= 100, ref.counts
        rec = ref.hit_batch(rays[: n // 2])
        hit = rec[rec[:, 0] >= 0]
        assert (hit[:, 21] == 1.5).sum() >= 100  # n1: the octahedron's triangles behind the origin are containers
    return w, rays, (0, 3), dict(records=24, ran=True), cond


CASES = {"ties": _case_ties, "no_division": _case_no_division, "grazing8": lambda rt: _case_grazing(rt, 8.0),
         "grazing1000": lambda rt: _case_grazing(rt, 1000.0), "grazing16000": lambda rt: _case_grazing(rt, 16000.0),
         "limits": _case_limits, "threshold15": lambda rt: _case_threshold(rt, 15),
         "threshold16": lambda rt: _case_threshold(rt, 16), "threshold17": lambda rt: _case_threshold(rt, 17),
         "alone3": lambda rt: _case_threshold(rt, 3, spheres=False), "unboxed": _case_unboxed,
         "containers": _case_containers}


@pytest.mark.parametrize("name", sorted(CASES))
def test_inputs_meet_the_conditions_of_their_case(rt, name):
    """The conditions on each case's inputs, from the checker alone (no GPU)."""
    w, rays, depths, readout, cond = CASES[name](rt)
    assert len(rays) <= 2000 and max(depths) <= 3
    cond(csg_ref.CsgRef.from_world(w))


def _hold(rt, w, rays, depths, readout, ref):
    for depth in depths:
        exh, est = w.color_at_batch(rays, depth, True, True)
        fast, fst = w.color_at_batch(rays, depth, True, False)
        plan = rt._rtamd._wf_plan(w)
        ref.counts = dict.fromkeys(csg_ref.COUNTERS, 0)
        want = ref.color_at_batch(rays, depth)
        exh, fast = np.asarray(exh), np.asarray(fast)
        assert exh.tobytes() == want.tobytes(), (depth, int((exh != want).any(axis=1).sum()), np.abs(exh - want).max())
        assert fast.tobytes() == want.tobytes(), (depth, int((fast != want).any(axis=1).sum()), np.abs(fast - want).max())
        for k in COUNTS:
            assert est[k] == ref.counts[k] and fst[k] == ref.counts[k], (depth, k, est[k], fst[k], ref.counts[k])
        assert est["exhaustive"] and not fst["exhaustive"]
        got = plan["triangles"]
        assert (got["records"], got["ran"]) == (readout["records"], readout["ran"]), (depth, got)
        assert plan["primary"]["lane"] >= 0  # a fused call
    assert ref.csg_ties == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_fast_equals_exhaustive_equals_checker(rt, name):
    w, rays, depths, readout, cond = CASES[name](rt)
    ref = csg_ref.CsgRef.from_world(w)
    cond(ref)
    _hold(rt, w, rays, depths, readout, ref)


def _unboxed_frame(rt):
    """Case 6 as a 24x16 frame; its condition: every kind of record wins pixels (from the checker)."""
    w, _ = _unboxed_world(rt)
    cam = rt.Camera(24, 16, math.pi / 2.5)  # (from the side the thin triangle faces)
    cam.set_transform(rt.view_transform(rt.Point(-6.0, 2.0, 0.5), rt.Point(0.0, 2.6, 1.8), rt.Vector(0, 1, 0)))
    ref = csg_ref.CsgRef.from_world(w)
    c = np.frombuffer(cam.desc_bytes(), dtype=csg_ref.CAMERA)[0]
    rays = np.array([list(o) + list(d) for o, d in (ref.ray_for_pixel(c, x, y) for y in range(16) for x in range(24))])
    win = _winners(ref, rays)
    tri = np.flatnonzero(ref.s["kind"] >= 5)
    assert (win == tri[17]).sum() >= 5 and (win == tri[18]).sum() >= 5 and np.isin(win, tri[:17]).sum() >= 15
    return w, cam, ref


def test_inputs_unboxed_frame_sees_every_kind_of_record(rt):
    _unboxed_frame(rt)


@pytest.mark.gpu
def test_unboxed_frame(rt):
    """Case 6 as a 24x16 frame through all three kinds of record: fast = exhaustive = checker."""
    w, cam, ref = _unboxed_frame(rt)
    img, rst = ref.render(cam.desc_bytes(), 2)
    fast, fst = cam.render(w, 2, True, False)
    plan = rt._rtamd._wf_plan(w)
    exh, est = cam.render(w, 2, True, True)
    assert exh.to_numpy().tobytes() == img.tobytes(), np.abs(exh.to_numpy() - img).max()
    assert fast.to_numpy().tobytes() == img.tobytes()
    for k in COUNTS:
        assert fst[k] == rst[k] and est[k] == rst[k], (k, fst[k], est[k], rst[k])
    assert plan["triangles"]["records"] == 17 and plan["triangles"]["ran"] and ref.csg_ties == 0
