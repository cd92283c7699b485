"""A small restatement of the reference's algorithm for scenes with triangles
(test infrastructure; the C oracle under oracle/ has no triangle).

Input: the bytes the library itself consumes (World.descs_bytes, groups_bytes,
shape_groups, triangles_bytes, lights_bytes; Camera.desc_bytes). Output: per
ray the 24 doubles of rt_hit_batch; per frame the canvas and the reference's
rays_* / *_tests counts. Spheres, planes, Triangle, SmoothTriangle, group
gates and the five patterns (Pattern::color_at_shape in `lighting`); any other
kind of shape is refused.

How it computes: Python floats, or element-wise numpy over the shapes of one
kind (both IEEE binary64, never fused); no dot / matmul / einsum / sum;
math.pow and math.sqrt / numpy.sqrt only; where Python deviates from IEEE it
is wrapped (`floor`, `fmod`, `as_isize`, `div`). Every ray builds the reference's
full intersection list (World::intersect, world.rs:31-38), sorts it stably
(intersection.rs:108-116, as the oracle does) and runs the `containers` walk
of prepare_computations literally (intersection.rs:63-90); none of the
library's shortcuts (top-2 containers, culling, skipped shadow rays).

Pinned at both ends by tests/test_mesh_ref.py: bit for bit against liboracle
on triangle-free scenes (patterned ones included), and the reference's
triangle and pattern KATs.
"""
import math

import numpy as np

EPSILON = 0.00001
INF = float("inf")

SHAPE = np.dtype([("kind", "<i4"), ("casts_shadow", "<i4"), ("transform", "<f8", 16), ("inverse", "<f8", 16),
                  ("color", "<f8", 3), ("ambient", "<f8"), ("diffuse", "<f8"), ("specular", "<f8"),
                  ("shininess", "<f8"), ("reflective", "<f8"), ("transparency", "<f8"), ("refractive_index", "<f8"),
                  ("pattern_kind", "<i4"), ("_pad", "<i4"), ("pattern_a", "<f8", 3), ("pattern_b", "<f8", 3),
                  ("pattern_transform", "<f8", 16), ("pattern_inverse", "<f8", 16), ("minimum", "<f8"),
                  ("maximum", "<f8"), ("closed", "<i4"), ("_pad2", "<i4")])
GROUP = np.dtype([("min", "<f8", 3), ("max", "<f8", 3), ("parent", "<i4"), ("_pad", "<i4")])
TRI = np.dtype([("p1", "<f8", 3), ("p2", "<f8", 3), ("p3", "<f8", 3), ("n1", "<f8", 3), ("n2", "<f8", 3),
                ("n3", "<f8", 3)])
CAMERA = np.dtype([("hsize", "<u4"), ("vsize", "<u4"), ("pixel_size", "<f8"), ("half_width", "<f8"),
                   ("half_height", "<f8"), ("inverse", "<f8", 16)])
assert SHAPE.itemsize == 680 and GROUP.itemsize == 56 and TRI.itemsize == 144 and CAMERA.itemsize == 160

SPHERE, PLANE, TRIANGLE, SMOOTH = 0, 1, 5, 6
COUNTERS = ("rays_primary", "rays_reflect", "rays_refract", "rays_shadow", "sphere_tests", "plane_tests",
            "sphere_disc_ge0", "other_tests")


# ---- vector.rs, on 3-tuples of floats or of equally shaped arrays
def sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def add(a, b):
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2])


def scale(a, s):
    return (a[0] * s, a[1] * s, a[2] * s)


def neg(a):
    return (-a[0], -a[1], -a[2])


def dot(a, b):  # vector.rs:99-101
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def cross(a, b):  # vector.rs:103-109
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def div(a, b):  # `/` on an f64 (Python raises where IEEE gives an inf or a NaN: a zero divisor)
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0.0:
            return float("nan")
        return math.copysign(INF, a) * math.copysign(1.0, b)


def normalize(a):  # vector.rs:21-28
    m = math.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])
    return (div(a[0], m), div(a[1], m), div(a[2], m))


def reflect(v, n):  # vector.rs:30-32: self - normal * 2.0 * dot(self, normal)
    return sub(v, scale(scale(n, 2.0), dot(v, n)))


def mat_point(m, p):  # matrix.rs:232-245 (rows 0..2 of a row-major 4x4)
    return (m[0] * p[0] + m[1] * p[1] + m[2] * p[2] + m[3], m[4] * p[0] + m[5] * p[1] + m[6] * p[2] + m[7],
            m[8] * p[0] + m[9] * p[1] + m[10] * p[2] + m[11])


def mat_vector(m, v):  # matrix.rs:247-260
    return (m[0] * v[0] + m[1] * v[1] + m[2] * v[2], m[4] * v[0] + m[5] * v[1] + m[6] * v[2],
            m[8] * v[0] + m[9] * v[1] + m[10] * v[2])


# ---- Triangle / SmoothTriangle (triangle.rs, smooth_triangle.rs)
def triangle_new(p1, p2, p3):
    """Triangle::new (triangle.rs:24-44): e1, e2, normal and the box of the three points."""
    e1, e2 = sub(p2, p1), sub(p3, p1)
    lo = tuple(min(p1[a], p2[a], p3[a]) for a in range(3))
    hi = tuple(max(p1[a], p2[a], p3[a]) for a in range(3))
    return {"p1": p1, "p2": p2, "p3": p3, "e1": e1, "e2": e2, "normal": normalize(cross(e2, e1)), "min": lo, "max": hi}


def triangle_solve(p1, e1, e2, o, d):
    """local_intersect (triangle.rs:63-90) on floats or arrays: (accepted, t, u, v).
    `accepted` is the reference's chain of early returns; t, u, v are only
    meaningful where it holds."""
    with np.errstate(all="ignore"):
        dir_cross_e2 = cross(d, e2)
        det = dot(e1, dir_cross_e2)
        ok = ~(np.abs(det) < EPSILON)
        f = 1.0 / det
        p1_to_origin = sub(o, p1)
        u = f * dot(p1_to_origin, dir_cross_e2)
        ok = ok & (0.0 <= u) & (u <= 1.0)  # RangeInclusive::contains: false for a NaN
        origin_cross_e1 = cross(p1_to_origin, e1)
        v = f * dot(d, origin_cross_e1)
        ok = ok & ~((v < 0.0) | ((u + v) > 1.0))
        t = f * dot(e2, origin_cross_e1)
    return ok, t, u, v


def triangle_local_intersect(tri, o, d):
    """The list of (t, u, v) of one triangle for a local ray (KATs)."""
    ok, t, u, v = triangle_solve(tuple(np.float64(x) for x in tri["p1"]), tuple(np.float64(x) for x in tri["e1"]),
                                 tuple(np.float64(x) for x in tri["e2"]), tuple(np.float64(x) for x in o),
                                 tuple(np.float64(x) for x in d))
    return [(float(t), float(u), float(v))] if bool(ok) else []


def smooth_normal(n1, n2, n3, u, v):  # smooth_triangle.rs:103-105
    return add(add(scale(n2, u), scale(n3, v)), scale(n1, 1.0 - u - v))


def schlick(eyev, normalv, n1, n2):  # intersection.rs:147-162
    cos = dot(eyev, normalv)
    if n1 > n2:
        n = div(n1, n2)
        sin2_t = n * n * (1.0 - cos * cos)
        if sin2_t > 1.0:
            return 1.0
        cos = math.sqrt(1.0 - sin2_t)
    q = div(n1 - n2, n1 + n2)
    r0 = q * q  # powi(2)
    x = 1.0 - cos
    return r0 + (1.0 - r0) * (x * ((x * x) * (x * x)))  # powi(5): x * (x^2)^2


# ---- pattern/{test_pattern,stripe,gradient,ring,checkers}.rs; `%` on an f64 is fmod
PATTERN_NONE, PATTERN_TEST, PATTERN_STRIPE, PATTERN_GRADIENT, PATTERN_RING, PATTERN_CHECKERS = -1, 0, 1, 2, 3, 4


def floor(x):  # f64::floor (math.floor makes an int and refuses inf and NaN)
    return float(np.floor(x))


def fmod(x, y):  # `%` on an f64 (math.fmod raises where C's fmod gives a NaN: an infinite x)
    try:
        return math.fmod(x, y)
    except ValueError:
        return float("nan")


def as_isize(x):  # `f64 as isize`: saturating, a NaN goes to 0
    if x != x:
        return 0
    if x >= 9223372036854775807.0:
        return 9223372036854775807
    if x <= -9223372036854775808.0:
        return -9223372036854775808
    return int(x)


def pattern_color_at(kind, a, b, p):
    """<Kind>Pattern::color_at on floats: `a`, `b` the pattern's colours, `p` the pattern point."""
    if kind == PATTERN_TEST:  # test_pattern.rs:7-9
        return (p[0], p[1], p[2])
    if kind == PATTERN_STRIPE:  # stripe.rs:14-20
        return a if fmod(floor(p[0]), 2.0) == 0.0 else b
    if kind == PATTERN_GRADIENT:  # gradient.rs:14-18: a + (b - a) * fraction
        fraction = p[0] - floor(p[0])
        return add(a, scale(sub(b, a), fraction))
    if kind == PATTERN_RING:  # ring.rs:14-21
        distance = floor(math.sqrt(p[0] * p[0] + p[2] * p[2]))
        return a if fmod(distance, 2.0) == 0.0 else b
    if kind == PATTERN_CHECKERS:  # checkers.rs:14-21: an integer `%`; its sign rule does not matter to `== 0`
        distance = floor(p[0]) + floor(p[1]) + floor(p[2])
        return a if as_isize(distance) % 2 == 0 else b
    raise ValueError("mesh_ref: bad pattern kind")


def pattern_color_at_shape(kind, a, b, pattern_inverse, shape_inverse, world_point, events=None, tag=None):  # pattern/mod.rs:39-49
    object_point = mat_point(shape_inverse, world_point)
    pattern_point = mat_point(pattern_inverse, object_point)
    if events is not None:
        events.append(("pattern", kind, pattern_point, tag))
    return pattern_color_at(kind, a, b, pattern_point)


class MeshRef:
    # a list to record in, or None: ("pattern", kind, pattern point, object) per Pattern::color_at_shape, ("lighting", {...})
    # per Material::lighting, ("shade", {...}) per World::shade_hit (what tests/test_shading_edges.py counts)
    events = None

    def __init__(self, descs_bytes, groups_bytes=b"", shape_groups=None, triangles_bytes=b"", lights_bytes=b""):
        self.s = np.frombuffer(descs_bytes, dtype=SHAPE)
        self.g = np.frombuffer(groups_bytes, dtype=GROUP)
        n = len(self.s)
        self.shape_group = np.asarray(shape_groups if shape_groups is not None and len(self.g) else [-1] * n,
                                      dtype=np.int64)
        tris = np.frombuffer(triangles_bytes, dtype=TRI)
        self.lights = np.frombuffer(lights_bytes, dtype=np.float64).reshape(-1, 6)
        kind = self.s["kind"]
        if not np.isin(kind, (SPHERE, PLANE, TRIANGLE, SMOOTH)).all():
            raise ValueError("mesh_ref: spheres, planes and triangles only")
        self.idx = {k: np.flatnonzero(kind == k) for k in (SPHERE, PLANE)}
        self.idx["tri"] = np.flatnonzero(kind >= TRIANGLE)
        if len(self.idx["tri"]) != len(tris):
            raise ValueError("mesh_ref: triangles_bytes does not match the shapes")
        self.tri_of = {int(i): j for j, i in enumerate(self.idx["tri"])}
        self.tris = tris
        # per kind: the inverse's entries as columns (element-wise over the shapes)
        self.inv = {k: [self.s["inverse"][ix, e].copy() for e in range(12)] for k, ix in self.idx.items()}
        col = lambda a: (a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy())
        self.tp1 = col(tris["p1"])
        self.te1 = sub(col(tris["p2"]), self.tp1)  # Triangle::new: e1 = p2 - p1, e2 = p3 - p1
        self.te2 = sub(col(tris["p3"]), self.tp1)
        self.smooth = {int(i): bool(kind[i] == SMOOTH) for i in self.idx["tri"]}
        self.counts = dict.fromkeys(COUNTERS, 0)

    @classmethod
    def from_world(cls, w):
        return cls(w.descs_bytes(), w.groups_bytes(), w.shape_groups(), w.triangles_bytes(), w.lights_bytes())

    # ---- Group::intersect's gates (group.rs:49-58, bounding_box.rs:95-136)
    def _gates(self, o, d):
        """Per shape: the ray meets the box of every group around it."""
        n_g = len(self.g)
        if n_g == 0:
            return None
        with np.errstate(all="ignore"):
            t0, t1 = [], []
            for a in range(3):
                n0, n1 = self.g["min"][:, a] - o[a], self.g["max"][:, a] - o[a]
                if abs(d[a]) >= EPSILON:
                    lo, hi = n0 / d[a], n1 / d[a]
                else:
                    lo, hi = n0 * INF, n1 * INF
                swap = lo > hi
                t0.append(np.where(swap, hi, lo))
                t1.append(np.where(swap, lo, hi))
            tmin = np.fmax(np.fmax(t0[0], t0[1]), t0[2])  # f64::max / min ignore a NaN operand
            tmax = np.fmin(np.fmin(t1[0], t1[1]), t1[2])
            hit = tmin <= tmax
        ok = np.zeros(n_g + 1, dtype=bool)
        ok[n_g] = True  # index -1: no group
        parent = self.g["parent"]
        for g in range(n_g):  # parents first
            ok[g] = hit[g] and ok[parent[g]]
        return ok[self.shape_group]

    # ---- World::intersect (world.rs:31-38): the sorted list of (t, object, u, v)
    def intersect(self, o, d):
        o = tuple(float(x) for x in o)
        d = tuple(float(x) for x in d)
        gate = self._gates(o, d)
        xs = []  # (object, position in its list, t, u, v)
        c = self.counts
        with np.errstate(all="ignore"):
            for k in (SPHERE, PLANE, "tri"):
                ix = self.idx[k]
                if len(ix) == 0:
                    continue
                on = np.ones(len(ix), dtype=bool) if gate is None else gate[ix]
                m = self.inv[k]
                lo, ld = mat_point(m, o), mat_vector(m, d)  # Ray::transform (ray.rs:26-28)
                if k == SPHERE:  # sphere.rs:47-62
                    a = dot(ld, ld)
                    b = 2.0 * dot(ld, lo)
                    cc = dot(lo, lo) - 1.0
                    disc = b * b - 4.0 * a * cc
                    ok = on & ~(disc < 0.0)
                    sq = np.sqrt(disc)
                    t1, t2 = (-b - sq) / (2.0 * a), (-b + sq) / (2.0 * a)
                    c["sphere_tests"] += int(on.sum())
                    c["sphere_disc_ge0"] += int(ok.sum())
                    for j in np.flatnonzero(ok):
                        xs.append((int(ix[j]), 0, float(t1[j]), None, None))
                        xs.append((int(ix[j]), 1, float(t2[j]), None, None))
                elif k == PLANE:  # plane.rs:53-60
                    ok = on & ~(np.abs(ld[1]) < EPSILON)
                    t = -lo[1] / ld[1]
                    c["plane_tests"] += int(on.sum())
                    for j in np.flatnonzero(ok):
                        xs.append((int(ix[j]), 0, float(t[j]), None, None))
                else:
                    ok, t, u, v = triangle_solve(self.tp1, self.te1, self.te2, lo, ld)
                    ok = ok & on
                    c["other_tests"] += int(on.sum())
                    for j in np.flatnonzero(ok):
                        i = int(ix[j])
                        uv = (float(u[j]), float(v[j])) if self.smooth[i] else (None, None)  # new / new_with_uv
                        xs.append((i, 0, float(t[j]), uv[0], uv[1]))
        if any(x[2] != x[2] for x in xs):
            raise ValueError("mesh_ref: a NaN t (the reference's sort panics)")
        xs.sort(key=lambda x: (x[0], x[1]))  # the flat_map order: objects in order, each list in push order
        xs.sort(key=lambda x: x[2])          # stable by t
        return [(x[2], x[0], x[3], x[4]) for x in xs]

    def normal_at(self, i, point, hit):  # geometry/mod.rs:51-56
        inv = self.s["inverse"][i]
        lp = mat_point(inv, point)
        kind = int(self.s["kind"][i])
        if kind == SPHERE:
            ln = sub(lp, (0.0, 0.0, 0.0))
        elif kind == PLANE:
            ln = (0.0, 1.0, 0.0)
        else:
            t = self.tris[self.tri_of[i]]
            if kind == TRIANGLE:
                p1 = tuple(float(x) for x in t["p1"])
                ln = triangle_new(p1, tuple(float(x) for x in t["p2"]), tuple(float(x) for x in t["p3"]))["normal"]
            else:
                ln = smooth_normal(tuple(float(x) for x in t["n1"]), tuple(float(x) for x in t["n2"]),
                                   tuple(float(x) for x in t["n3"]), hit[2], hit[3])
        # transform_inverse_transpose * local_normal (the upper 3x3 of the transpose)
        wn = (inv[0] * ln[0] + inv[4] * ln[1] + inv[8] * ln[2], inv[1] * ln[0] + inv[5] * ln[1] + inv[9] * ln[2],
              inv[2] * ln[0] + inv[6] * ln[1] + inv[10] * ln[2])
        return normalize(tuple(float(x) for x in wn))

    def prepare(self, hit, o, d, xs):  # intersection.rs:53-105
        t, obj = hit[0], hit[1]
        point = add(o, scale(d, t))
        eyev = neg(d)
        normalv = self.normal_at(obj, point, hit)
        inside = False
        if dot(normalv, eyev) < 0.0:
            inside = True
            normalv = neg(normalv)
        ri = self.s["refractive_index"]
        containers = []
        n1 = n2 = -1.0
        for i in xs:
            if i == hit:
                n1 = 1.0 if not containers else float(ri[containers[-1]])
            if i[1] in containers:
                containers.remove(i[1])
            else:
                containers.append(i[1])
            if i == hit:
                n2 = 1.0 if not containers else float(ri[containers[-1]])
                break
        return {"object": obj, "t": t, "point": point, "over": add(point, scale(normalv, EPSILON)),
                "under": sub(point, scale(normalv, EPSILON)), "eyev": eyev, "normalv": normalv, "inside": inside,
                "reflectv": reflect(d, normalv), "n1": n1, "n2": n2}

    def hit_record(self, o, d):
        """The 24 doubles of rt_hit_batch for one ray."""
        o = tuple(float(x) for x in o)
        d = tuple(float(x) for x in d)
        xs = self.intersect(o, d)
        out = [0.0] * 24
        out[0] = -1.0
        h = next((x for x in xs if x[0] >= 0.0), None)
        if h is None:
            return out
        c = self.prepare(h, o, d, xs)
        out[0:2] = [float(c["object"]), c["t"]]
        out[2:5], out[5:8], out[8:11] = c["point"], c["over"], c["under"]
        out[11:14], out[14:17] = c["eyev"], c["normalv"]
        out[17] = 1.0 if c["inside"] else 0.0
        out[18:21] = c["reflectv"]
        out[21], out[22] = c["n1"], c["n2"]
        out[23] = schlick(c["eyev"], c["normalv"], c["n1"], c["n2"])
        return out

    def hit_batch(self, rays):
        return np.array([self.hit_record(r[:3], r[3:]) for r in np.asarray(rays, dtype=np.float64)])

    def is_shadowed(self, point, light):  # world.rs:95-105
        point = tuple(float(x) for x in point)
        L = self.lights[light]
        v = sub(tuple(float(x) for x in L[:3]), point)
        distance = math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
        direction = normalize(v)
        self.counts["rays_shadow"] += 1
        xs = self.intersect(point, direction)
        h = next((x for x in xs if x[0] >= 0.0 and self.s["casts_shadow"][x[1]] != 0), None)
        return h is not None and h[0] < distance

    def lighting(self, i, L, point, eyev, normalv, in_shadow):  # material.rs:38-82
        s = self.s[i]
        if int(s["pattern_kind"]) != PATTERN_NONE:  # material.rs:47-51
            color = pattern_color_at_shape(int(s["pattern_kind"]), tuple(float(x) for x in s["pattern_a"]),
                                           tuple(float(x) for x in s["pattern_b"]),
                                           [float(x) for x in s["pattern_inverse"]], [float(x) for x in s["inverse"]],
                                           point, self.events, i)
        else:
            color = tuple(float(x) for x in s["color"])
        intensity = tuple(float(x) for x in L[3:])
        effective = (color[0] * intensity[0], color[1] * intensity[1], color[2] * intensity[2])
        lightv = normalize(sub(tuple(float(x) for x in L[:3]), point))
        ambient = scale(effective, float(s["ambient"]))
        ev = None
        if self.events is not None:
            ev = {"object": i, "in_shadow": bool(in_shadow), "patterned": int(s["pattern_kind"]) != PATTERN_NONE,
                  "ambient": ambient, "intensity": intensity, "specular": float(s["specular"]),
                  "shininess": float(s["shininess"]), "light_dot_normal": dot(lightv, normalv),
                  "reflect_dot_eye": None, "diffuse_term": None, "specular_term": None}
            self.events.append(("lighting", ev))
        if in_shadow:
            return ambient
        light_dot_normal = dot(lightv, normalv)
        if light_dot_normal < 0.0:
            diffuse = specular = (0.0, 0.0, 0.0)
        else:
            diffuse = scale(scale(effective, float(s["diffuse"])), light_dot_normal)
            reflect_dot_eye = dot(reflect(neg(lightv), normalv), eyev)
            if reflect_dot_eye <= 0.0:
                specular = (0.0, 0.0, 0.0)
            else:
                try:
                    factor = math.pow(reflect_dot_eye, float(s["shininess"]))
                except OverflowError:  # f64::powf gives inf (an unnormalised eye vector)
                    factor = INF
                specular = scale(scale(intensity, float(s["specular"])), factor)
            if ev is not None:
                ev["reflect_dot_eye"], ev["diffuse_term"], ev["specular_term"] = reflect_dot_eye, diffuse, specular
        return add(add(ambient, diffuse), specular)

    def color_at(self, o, d, remaining, kind="rays_primary"):  # world.rs:70-81
        o = tuple(float(x) for x in o)
        d = tuple(float(x) for x in d)
        self.counts[kind] += 1
        xs = self.intersect(o, d)
        h = next((x for x in xs if x[0] >= 0.0), None)
        if h is None:
            return (0.0, 0.0, 0.0)
        c = self.prepare(h, o, d, xs)
        i = c["object"]
        s = self.s[i]
        surface = (0.0, 0.0, 0.0)  # Sum for Color: a fold from black
        for li in range(len(self.lights)):
            shadowed = self.is_shadowed(c["over"], li)
            surface = add(surface, self.lighting(i, self.lights[li], c["over"], c["eyev"], c["normalv"], shadowed))
        refl_m, transp = float(s["reflective"]), float(s["transparency"])
        ev = None
        if self.events is not None:
            ev = {"object": i, "remaining": remaining, "reflective": refl_m, "transparency": transp, "n1": c["n1"],
                  "n2": c["n2"], "cos_i": dot(c["eyev"], c["normalv"]), "reflect": False, "refract": False,
                  "sin2_t": None, "schlick": None}
            self.events.append(("shade", ev))
        if abs(refl_m - 0.0) < EPSILON or remaining == 0:  # world.rs:107-114
            reflected = (0.0, 0.0, 0.0)
        else:
            if ev is not None:
                ev["reflect"] = True
            reflected = scale(self.color_at(c["over"], c["reflectv"], remaining - 1, "rays_reflect"), refl_m)
        refracted = (0.0, 0.0, 0.0)  # world.rs:116-134
        if not (abs(transp - 0.0) < EPSILON or remaining == 0):
            n_ratio = div(c["n1"], c["n2"])
            cos_i = dot(c["eyev"], c["normalv"])
            sin2_t = n_ratio * n_ratio * (1.0 - cos_i * cos_i)
            if ev is not None:
                ev["sin2_t"], ev["refract"] = sin2_t, not sin2_t > 1.0
            if not sin2_t > 1.0:
                cos_t = math.sqrt(1.0 - sin2_t)
                direction = sub(scale(c["normalv"], n_ratio * cos_i - cos_t), scale(c["eyev"], n_ratio))
                refracted = scale(self.color_at(c["under"], direction, remaining - 1, "rays_refract"), transp)
        if refl_m > 0.0 and transp > 0.0:  # world.rs:58-67
            r = schlick(c["eyev"], c["normalv"], c["n1"], c["n2"])
            if ev is not None:
                ev["schlick"] = r
            return add(add(surface, scale(reflected, r)), scale(refracted, 1.0 - r))
        return add(add(surface, reflected), refracted)

    def color_at_batch(self, rays, remaining):
        return np.array([self.color_at(r[:3], r[3:], remaining) for r in np.asarray(rays, dtype=np.float64)])

    def ray_for_pixel(self, cam, px, py):  # camera.rs:57-69
        xoffset = (float(px) + 0.5) * float(cam["pixel_size"])
        yoffset = (float(py) + 0.5) * float(cam["pixel_size"])
        world_x = float(cam["half_width"]) - xoffset
        world_y = float(cam["half_height"]) - yoffset
        inv = [float(x) for x in cam["inverse"]]
        pixel = mat_point(inv, (world_x, world_y, -1.0))
        origin = mat_point(inv, (0.0, 0.0, 0.0))
        return origin, normalize(sub(pixel, origin))

    def render(self, camera_desc, max_depth):
        """Camera::render (camera.rs:133-148): (rgb[vsize, hsize, 3], the counters of this frame)."""
        cam = np.frombuffer(camera_desc, dtype=CAMERA)[0]
        self.counts = dict.fromkeys(COUNTERS, 0)
        out = np.zeros((int(cam["vsize"]), int(cam["hsize"]), 3))
        for y in range(out.shape[0]):
            for x in range(out.shape[1]):
                o, d = self.ray_for_pixel(cam, x, y)
                out[y, x] = self.color_at(o, d, max_depth)
        return out, dict(self.counts)
