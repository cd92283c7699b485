"""The checker of tests/csg_ref.py for worlds with a Triangle or SmoothTriangle
under a `Csg` (test infrastructure; csg_ref.py itself refuses them, as the
library once did, and stays as it is).

What differs from CsgRef, and nothing else:
  - the constructor accepts a triangle below a Csg node;
  - `_shape` solves a triangle below a Csg with the ray it is handed, the world
    ray through the inverse of every Csg above it, one rounded transform after
    another (geometry/mod.rs:46-49, csg.rs:115-125), then through its own:
    `triangle_solve` on that record with that ray (the triangles that share
    their innermost Csg are handed the same ray, so they are solved in one
    element-wise call when the first of them is reached: per record the same
    scalar operations). A triangle with no Csg above it still takes its answer
    from the one element-wise solve per world ray;
  - the tuple carries that solve's u and v, so MeshRef.normal_at gives a
    SmoothTriangle the reference's normal (smooth_triangle.rs:103-105: the
    intersection's own u and v, those of the chained ray).

`unit_roots`: per ray handed to a Csg that no Csg encloses, the t of every
intersection its leaves returned before any filter (what the library's wide
evaluator has to stream), kept while `keep_roots` is set.
"""
import numpy as np

import csg_ref
from csg_ref import (COUNTERS, GROUP, NODE, NODE_CSG, SHAPE, SMOOTH, TRI, TRIANGLE, CsgRef, mat_point,  # noqa: F401
                     mat_vector, sub, triangle_solve)


class CsgTriRef(CsgRef):
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
        if not np.isin(self.s["kind"], (0, 1, 2, 3, 4, TRIANGLE, SMOOTH)).all():
            raise ValueError("csg_tri_ref: kinds 0-6 only")
        self.tris = np.frombuffer(triangles_bytes, dtype=TRI)
        tri_idx = np.flatnonzero(self.s["kind"] >= TRIANGLE)
        if len(tri_idx) != len(self.tris):
            raise ValueError("csg_tri_ref: triangles_bytes does not match the shapes")
        self.tri_of = {int(i): j for j, i in enumerate(tri_idx)}
        self.under_csg = {}  # a triangle with a Csg above it -> the innermost one
        for i in tri_idx:
            g = self.shape_node[int(i)]
            while g >= 0:
                if int(nodes["kind"][g]) == NODE_CSG:
                    self.under_csg[int(i)] = g
                    break
                g = int(nodes["parent"][g])
        # per such Csg: its triangles' records as columns (the groups between hand the ray on unchanged, so all
        # of them are handed the same ray: one element-wise solve, each lane the single record's own operations)
        self._below = {}
        for g in set(self.under_csg.values()):
            js = np.array([self.tri_of[i] for i, gg in sorted(self.under_csg.items()) if gg == g])
            self._below[g] = {"place": {int(j): k for k, j in enumerate(js)}, "js": js, "ray": (None, None), "solved": None}
        self.tri_inv = [self.s["inverse"][tri_idx, e].copy() for e in range(12)]
        col = lambda a: (a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy())
        self.tp1 = col(self.tris["p1"])
        self.te1 = sub(col(self.tris["p2"]), self.tp1)  # Triangle::new: e1 = p2 - p1, e2 = p3 - p1
        self.te2 = sub(col(self.tris["p3"]), self.tp1)
        self._solved = None
        self.counts = dict.fromkeys(COUNTERS, 0)
        self.csg_ties = 0
        self.keep_roots = False
        self.unit_roots = []
        self._depth = 0
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

    def _shape(self, i, o, d):
        if i not in self.under_csg:
            xs = CsgRef._shape(self, i, o, d)
        else:  # triangle.rs:63-90, smooth_triangle.rs:74-101 with the ray this shape was handed
            b = self._below[self.under_csg[i]]
            if b["ray"][0] is not o or b["ray"][1] is not d:  # the first of them this ray reaches
                js = b["js"]
                inv = [c[js] for c in self.tri_inv]
                cut = lambda cols: tuple(c[js] for c in cols)
                b["solved"] = triangle_solve(cut(self.tp1), cut(self.te1), cut(self.te2), mat_point(inv, o), mat_vector(inv, d))
                b["ray"] = (o, d)
            ok, t, u, v = b["solved"]
            k = b["place"][self.tri_of[i]]
            self.counts["other_tests"] += 1
            if not bool(ok[k]):
                xs = []
            elif int(self.s["kind"][i]) == SMOOTH:
                xs = [(t[k], i, float(u[k]), float(v[k]))]
            else:
                xs = [(t[k], i, None, None)]
        if self.keep_roots and self._depth > 0:
            self.unit_roots[-1].extend(float(x[0]) for x in xs)
        return xs

    def _node(self, g, o, d):
        if int(self.nodes["kind"][g]) != NODE_CSG:
            return CsgRef._node(self, g, o, d)
        if self.keep_roots and self._depth == 0:
            self.unit_roots.append([])
        self._depth += 1
        try:
            return CsgRef._node(self, g, o, d)
        finally:
            self._depth -= 1
