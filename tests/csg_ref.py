"""A literal restatement of the reference's algorithm for worlds with `Csg`
(geometry/shape/csg.rs): test infrastructure, the yardstick of the CSG tests
(the C oracle under oracle/ has no Csg).

Input: the bytes the library itself consumes (World.descs_bytes, nodes_bytes,
shape_nodes, shape_sides, lights_bytes, triangles_bytes; for a world without a
Csg groups_bytes and shape_groups). Output as tests/mesh_ref.py: per ray the 24
doubles of rt_hit_batch, per frame the canvas and the reference's counters.
Every world the library accepts: kinds 0-4 (sphere, plane, cube, cylinder,
cone), Triangle and SmoothTriangle (kinds 5 and 6) at the top level or under
groups, groups, Csg nodes and the five patterns (mesh_ref's `lighting`). A
triangle under a Csg is refused, as the library refuses it.

How it computes (the rules of mesh_ref.py): IEEE binary64 scalars, never fused,
no dot / matmul / sum. Every ray builds the reference's lists as the reference
does: Shape::intersect transforms the ray by the shape's own inverse (one
matrix after another down a Csg chain, never a product), Group::intersect and
Csg::local_intersect gate on their boxes, a Csg sorts left ++ right stably and
runs filter_intersections as written (csg.rs:71-91), `includes` is membership
in the left subtree, World::intersect sorts everything again; then the full
`containers` walk (mesh_ref.MeshRef.prepare). A triangle's Shape::intersect is
ray_transform by its own inverse, then mesh_ref.triangle_solve; all triangles
of a world are solved in one element-wise numpy call per world ray (no group
changes the ray, and no triangle lies under a Csg), and each one's answer is
taken, and counted, where the tree walk reaches it.

`csg_ties`: the number of adjacent equal-t pairs met in any Csg node's sorted
list since the object was made (the reference's sort is unstable there).
"""
import numpy as np

from mesh_ref import (CAMERA, COUNTERS, EPSILON, GROUP, INF, SHAPE, TRI, MeshRef, mat_point, mat_vector,  # noqa: F401
                      normalize, sub, triangle_solve)

NODE = np.dtype([("kind", "<i4"), ("parent", "<i4"), ("side", "<i4"), ("operation", "<i4"), ("min", "<f8", 3),
                 ("max", "<f8", 3), ("inverse", "<f8", 16)])
assert NODE.itemsize == 192

SPHERE, PLANE, CUBE, CYLINDER, CONE, TRIANGLE, SMOOTH = 0, 1, 2, 3, 4, 5, 6
NODE_GROUP, NODE_CSG = 0, 1
UNION, INTERSECTION, DIFFERENCE = 0, 1, 2
F = np.float64


def intersection_allowed(op, lhit, inl, inr):  # csg.rs:22-41
    if op == UNION:
        return (lhit and not inr) or (not lhit and not inl)
    if op == INTERSECTION:
        return (lhit and inr) or (not lhit and inl)
    if op == DIFFERENCE:
        return (lhit and not inr) or (not lhit and inl)
    raise ValueError("csg_ref: bad operation")


def filter_intersections(op, in_left, xs):
    """Csg::filter_intersections (csg.rs:71-91); `in_left(x)`: left.includes(x's object)."""
    inl = inr = False
    result = []
    for x in xs:
        lhit = in_left(x)
        if intersection_allowed(op, lhit, inl, inr):
            result.append(x)
        if lhit:
            inl = not inl
        else:
            inr = not inr
    return result


def box_intersects(mn, mx, o, d):  # bounding_box.rs:95-136
    t0s, t1s = [], []
    for a in range(3):
        n0, n1 = F(mn[a]) - o[a], F(mx[a]) - o[a]
        if abs(d[a]) >= EPSILON:
            t0, t1 = n0 / d[a], n1 / d[a]
        else:
            t0, t1 = n0 * F(INF), n1 * F(INF)
        if t0 > t1:
            t0, t1 = t1, t0
        t0s.append(t0)
        t1s.append(t1)
    tmin = np.fmax(np.fmax(t0s[0], t0s[1]), t0s[2])  # f64::max / min ignore a NaN operand
    tmax = np.fmin(np.fmin(t1s[0], t1s[1]), t1s[2])
    return bool(tmin <= tmax)


def ray_transform(m, o, d):  # ray.rs:26-28, matrix.rs:232-260
    lo = (m[0] * o[0] + m[1] * o[1] + m[2] * o[2] + m[3], m[4] * o[0] + m[5] * o[1] + m[6] * o[2] + m[7],
          m[8] * o[0] + m[9] * o[1] + m[10] * o[2] + m[11])
    ld = (m[0] * d[0] + m[1] * d[1] + m[2] * d[2], m[4] * d[0] + m[5] * d[1] + m[6] * d[2],
          m[8] * d[0] + m[9] * d[1] + m[10] * d[2])
    return lo, ld


def cube_check_axis(origin, direction):  # cube.rs:30-47
    n0, n1 = F(-1.0) - origin, F(1.0) - origin
    if abs(direction) >= EPSILON:
        t0, t1 = n0 / direction, n1 / direction
    else:
        t0, t1 = n0 * F(INF), n1 * F(INF)
    return (t1, t0) if t0 > t1 else (t0, t1)


def caps(kind, mn, mx, closed, o, d):  # cylinder.rs:42-65, cone.rs:48-71
    xs = []
    if not closed:
        return xs
    for y in (mn, mx):
        t = (y - o[1]) / d[1]
        x = o[0] + t * d[0]
        z = o[2] + t * d[2]
        radius2 = F(1.0) if kind == CYLINDER else y * y
        if (x * x + z * z) <= radius2:
            xs.append(t)
    return xs


def local_intersect(kind, mn, mx, closed, o, d):
    """The t values of <kind>::local_intersect in push order, and whether a sphere's disc was >= 0."""
    if kind == SPHERE:  # sphere.rs:47-62
        a = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
        b = F(2.0) * (d[0] * o[0] + d[1] * o[1] + d[2] * o[2])
        c = o[0] * o[0] + o[1] * o[1] + o[2] * o[2] - F(1.0)
        disc = b * b - F(4.0) * a * c
        if disc < 0.0:
            return [], False
        return [(-b - np.sqrt(disc)) / (F(2.0) * a), (-b + np.sqrt(disc)) / (F(2.0) * a)], True
    if kind == PLANE:  # plane.rs:53-60
        if abs(d[1]) < EPSILON:
            return [], False
        return [-o[1] / d[1]], False
    if kind == CUBE:  # cube.rs:71-93
        xt, yt, zt = cube_check_axis(o[0], d[0]), cube_check_axis(o[1], d[1]), cube_check_axis(o[2], d[2])
        tmin = np.fmax(np.fmax(xt[0], yt[0]), zt[0])
        tmax = np.fmin(np.fmin(xt[1], yt[1]), zt[1])
        if tmin > tmax:
            return [], False
        return [tmin, tmax], False
    xs = []
    if kind == CYLINDER:  # cylinder.rs:88-119
        a = d[0] * d[0] + d[2] * d[2]
        if abs(a) < EPSILON:
            return caps(kind, mn, mx, closed, o, d), False
        b = F(2.0) * o[0] * d[0] + F(2.0) * o[2] * d[2]
        c = o[0] * o[0] + o[2] * o[2] - F(1.0)
    else:  # cone.rs:94-134
        a = d[0] * d[0] - d[1] * d[1] + d[2] * d[2]
        b = F(2.0) * o[0] * d[0] - F(2.0) * o[1] * d[1] + F(2.0) * o[2] * d[2]
        c = o[0] * o[0] - o[1] * o[1] + o[2] * o[2]
        if abs(a) < EPSILON:
            if abs(b) < EPSILON:
                return caps(kind, mn, mx, closed, o, d), False
            return [-c / F(2.0) * b] + caps(kind, mn, mx, closed, o, d), False
    disc = b * b - F(4.0) * a * c
    if disc < 0.0:
        return [], False
    t0 = (-b - np.sqrt(disc)) / (F(2.0) * a)
    t1 = (-b + np.sqrt(disc)) / (F(2.0) * a)
    y0 = o[1] + t0 * d[1]
    if mn < y0 and y0 < mx:
        xs.append(t0)
    y1 = o[1] + t1 * d[1]
    if mn < y1 and y1 < mx:
        xs.append(t1)
    return xs + caps(kind, mn, mx, closed, o, d), False


class CsgRef(MeshRef):
    def __init__(self, descs_bytes, nodes_bytes=b"", shape_nodes=None, shape_sides=None, lights_bytes=b"",
                 groups_bytes=b"", shape_groups=None, triangles_bytes=b""):
        self.s = np.frombuffer(descs_bytes, dtype=SHAPE)
        n = len(self.s)
        nodes = np.frombuffer(nodes_bytes, dtype=NODE)
        if len(nodes) == 0:  # a world without a Csg: its groups
            g = np.frombuffer(groups_bytes, dtype=GROUP)
            nodes = np.zeros(len(g), dtype=NODE)
            nodes["parent"], nodes["min"], nodes["max"] = g["parent"], g["min"], g["max"]
            shape_nodes = shape_groups
        self.nodes = nodes
        self.shape_node = list(shape_nodes) if shape_nodes is not None and len(nodes) else [-1] * n
        self.shape_side = list(shape_sides) if shape_sides is not None and len(shape_sides) else [0] * n
        self.lights = np.frombuffer(lights_bytes, dtype=np.float64).reshape(-1, 6)
        if not np.isin(self.s["kind"], (SPHERE, PLANE, CUBE, CYLINDER, CONE, TRIANGLE, SMOOTH)).all():
            raise ValueError("csg_ref: kinds 0-6 only")
        # the triangles, as MeshRef holds them: columns, for one element-wise solve per world ray
        self.tris = np.frombuffer(triangles_bytes, dtype=TRI)
        tri_idx = np.flatnonzero(self.s["kind"] >= TRIANGLE)
        if len(tri_idx) != len(self.tris):
            raise ValueError("csg_ref: triangles_bytes does not match the shapes")
        self.tri_of = {int(i): j for j, i in enumerate(tri_idx)}
        for i in tri_idx:
            g = self.shape_node[int(i)]
            while g >= 0:
                if int(nodes["kind"][g]) == NODE_CSG:
                    raise ValueError("csg_ref: a triangle under a Csg (the library refuses it)")
                g = int(nodes["parent"][g])
        self.tri_inv = [self.s["inverse"][tri_idx, e].copy() for e in range(12)]
        col = lambda a: (a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy())
        self.tp1 = col(self.tris["p1"])
        self.te1 = sub(col(self.tris["p2"]), self.tp1)  # Triangle::new: e1 = p2 - p1, e2 = p3 - p1
        self.te2 = sub(col(self.tris["p3"]), self.tp1)
        self._solved = None
        self.counts = dict.fromkeys(COUNTERS, 0)
        self.csg_ties = 0
        # the tree: each node's children in the reference's order (the shapes come depth first)
        first = [n] * len(nodes)
        for i in range(n - 1, -1, -1):
            g = self.shape_node[i]
            while g >= 0:
                first[g] = i
                g = int(nodes["parent"][g])
        kids = {g: [] for g in range(-1, len(nodes))}
        for i in range(n):
            kids[self.shape_node[i]].append((i, self.shape_side[i], "shape", i))
        for g in range(len(nodes)):
            kids[int(nodes["parent"][g])].append((first[g], int(nodes["side"][g]), "node", g))
        for k in kids.values():
            k.sort(key=lambda c: c[0])
        self.kids = kids
        self.leaves = {}  # node -> the shapes below it (Shape::includes down the tree)
        for g in range(len(nodes) - 1, -1, -1):
            below = set()
            for c in kids[g]:
                below |= {c[3]} if c[2] == "shape" else self.leaves[c[3]]
            self.leaves[g] = below

    @classmethod
    def from_world(cls, w):
        return cls(w.descs_bytes(), w.nodes_bytes(), w.shape_nodes(), w.shape_sides(), w.lights_bytes(),
                   w.groups_bytes(), w.shape_groups(), w.triangles_bytes())

    # ---- Shape::intersect (geometry/mod.rs:46-49) of a primitive: [(t, object, u, v)]
    def _shape(self, i, o, d):
        s = self.s[i]
        kind = int(s["kind"])
        if kind >= TRIANGLE:  # triangle.rs:63-90, smooth_triangle.rs:74-101: solved with all the others
            ok, t, u, v = self._solved
            j = self.tri_of[i]
            self.counts["other_tests"] += 1
            if not ok[j]:
                return []
            return [(t[j], i, float(u[j]), float(v[j]))] if kind == SMOOTH else [(t[j], i, None, None)]
        lo, ld = ray_transform(s["inverse"], o, d)
        ts, disc = local_intersect(kind, s["minimum"], s["maximum"], bool(s["closed"]), lo, ld)
        c = self.counts
        c["sphere_tests" if kind == SPHERE else "plane_tests" if kind == PLANE else "other_tests"] += 1
        if disc:
            c["sphere_disc_ge0"] += 1
        return [(t, i, None, None) for t in ts]

    def _child(self, c, o, d):
        return self._shape(c[3], o, d) if c[2] == "shape" else self._node(c[3], o, d)

    def _node(self, g, o, d):
        nd = self.nodes[g]
        if int(nd["kind"]) == NODE_GROUP:  # Group::intersect (group.rs:49-58)
            if not box_intersects(nd["min"], nd["max"], o, d):
                return []
            xs = []
            for c in self.kids[g]:
                xs.extend(self._child(c, o, d))
            return xs
        lo, ld = ray_transform(nd["inverse"], o, d)  # Shape::intersect of the Csg (geometry/mod.rs:46-49)
        if not box_intersects(nd["min"], nd["max"], lo, ld):  # csg.rs:115-118
            return []
        left = [c for c in self.kids[g] if c[1] == 0]
        right = [c for c in self.kids[g] if c[1] == 1]
        if len(left) != 1 or len(right) != 1:
            raise ValueError("csg_ref: a Csg needs one left and one right child")
        xs = self._child(left[0], lo, ld)
        xs.extend(self._child(right[0], lo, ld))  # csg.rs:120-123
        if any(x[0] != x[0] for x in xs):
            raise ValueError("csg_ref: a NaN t (the reference's sort panics)")
        xs.sort(key=lambda x: x[0])  # intersections(): stable here
        self.csg_ties += sum(1 for a, b in zip(xs, xs[1:]) if a[0] == b[0])
        in_left = self.leaves[left[0][3]] if left[0][2] == "node" else {left[0][3]}
        return filter_intersections(int(nd["operation"]), lambda x: x[1] in in_left, xs)  # csg.rs:124-125

    # ---- World::intersect (world.rs:31-38): the sorted list of (t, object, None, None)
    def intersect(self, o, d):
        o = tuple(F(x) for x in o)
        d = tuple(F(x) for x in d)
        xs = []
        with np.errstate(all="ignore"):
            if len(self.tris):  # Ray::transform by each triangle's own inverse, then local_intersect
                self._solved = triangle_solve(self.tp1, self.te1, self.te2, mat_point(self.tri_inv, o),
                                              mat_vector(self.tri_inv, d))
            for c in self.kids[-1]:
                xs.extend(self._child(c, o, d))
        if any(x[0] != x[0] for x in xs):
            raise ValueError("csg_ref: a NaN t (the reference's sort panics)")
        xs.sort(key=lambda x: x[0])
        return [(float(x[0]), x[1], x[2], x[3]) for x in xs]

    def normal_at(self, i, point, hit):  # geometry/mod.rs:51-56: the leaf's own matrices on the world point
        s = self.s[i]
        if int(s["kind"]) >= TRIANGLE:
            return MeshRef.normal_at(self, i, point, hit)
        inv = [float(x) for x in s["inverse"]]
        p = (inv[0] * point[0] + inv[1] * point[1] + inv[2] * point[2] + inv[3],
             inv[4] * point[0] + inv[5] * point[1] + inv[6] * point[2] + inv[7],
             inv[8] * point[0] + inv[9] * point[1] + inv[10] * point[2] + inv[11])
        kind = int(s["kind"])
        if kind == SPHERE:  # sphere.rs:64-67
            ln = (p[0] - 0.0, p[1] - 0.0, p[2] - 0.0)
        elif kind == PLANE:  # plane.rs:62-64
            ln = (0.0, 1.0, 0.0)
        elif kind == CUBE:  # cube.rs:95-106
            maxc = max(max(abs(p[0]), abs(p[1])), abs(p[2]))
            if abs(maxc - abs(p[0])) < EPSILON:
                ln = (p[0], 0.0, 0.0)
            elif abs(maxc - abs(p[1])) < EPSILON:
                ln = (0.0, p[1], 0.0)
            else:
                ln = (0.0, 0.0, p[2])
        else:  # cylinder.rs:121-130, cone.rs:136-149
            dist = p[0] * p[0] + p[2] * p[2]
            if dist < 1.0 and p[1] >= float(s["maximum"]) - EPSILON:
                ln = (0.0, 1.0, 0.0)
            elif dist < 1.0 and p[1] <= float(s["minimum"]) + EPSILON:
                ln = (0.0, -1.0, 0.0)
            elif kind == CYLINDER:
                ln = (p[0], 0.0, p[2])
            else:
                y = float(np.sqrt(F(p[0] * p[0] + p[2] * p[2])))
                if p[1] > 0.0:
                    y = -y
                ln = (p[0], y, p[2])
        wn = (inv[0] * ln[0] + inv[4] * ln[1] + inv[8] * ln[2], inv[1] * ln[0] + inv[5] * ln[1] + inv[9] * ln[2],
              inv[2] * ln[0] + inv[6] * ln[1] + inv[10] * ln[2])
        return normalize(wn)
