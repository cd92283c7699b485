"""Worlds whose intersections tie bit for bit, and what the checker says of them:
test infrastructure (a plain helper module like csg_ref.py).

The rule they hold (world.rs:31-38, intersection.rs:53-105): where two roots of
World::intersect's list have a bit-equal t, the one that comes first in the
traversal order (world order, a group's children in order, t1 before t2 of one
object) is the hit, and `containers` meets them in that order. The checker
(csg_ref.py) and the C oracle restate it with a stable sort; the GPU never
builds the list and must reach the same winner from its keys.

How the ties are made exact: every transform is a product of translations and
scalings by dyadic rationals (scalings by powers of two along the axis whose
roots must match), so the inverse's entries and the local origin of a dyadic
world origin are exact, and (face - o) / d rounds once, to the same double for
every object that shares the face, whatever the direction. Twins (two objects
at one transform) tie for every ray at all. No rotation anywhere; every camera
looks along an axis from a dyadic point, so primary origins are exact.

Objects that tie differ in colour (role A warm: red > blue; role B cool) and in
refractive_index, and in every pair the B member casts no shadow where the
world says so. Each world holds every tying pair in both insertion orders
(seeded, or mirrored copies side by side), so both roles win somewhere.

`build(rt, name)` gives a TieWorld: the world, its 24x16 camera, the authored
batch rays and the tie classes it was written for. `classify` counts, from the
checker alone:
  H   rays whose first t >= 0 is shared by two different objects,
  T0  H at t == 0,
  C   rays with a hit whose last negative root is shared by two different
      objects that are both in `containers` there,
  C3  ... by three.
`Reversed` is the checker with every run of equal t in the world's list turned
round: what a walk that took the last instead of the first would compute.
"""
import math
import random

import numpy as np

import csg_ref

W, H, DEPTH = 24, 16, 3
WARM, COOL = (0.9, 0.35, 0.15), (0.15, 0.45, 0.9)
ORACLE_WORLDS = ("twins", "flush", "lattice", "lattice_divided", "lattice_twins", "nested", "lines")
WORLDS = ORACLE_WORLDS + ("mesh", "csg")


class TieWorld:
    def __init__(self, name, w, cam, rays, classes):
        self.name, self.w, self.cam, self.classes = name, w, cam, classes
        self.rays = np.ascontiguousarray(rays, dtype=np.float64)
        self.depth = DEPTH


# ---------------------------------------------------------------- parts
def _paint(s, role, k=0, glass=True, shadow=True):
    """Role A (0) or B (1): colour and refractive_index apart, so the winner of a tie shows."""
    base = WARM if role == 0 else COOL
    s.material.color = rt_color(base[0], base[1] + 0.05 * (k % 4), base[2])
    s.material.refractive_index = (1.5 + 0.0625 * (k % 3)) if role == 0 else (1.125 + 0.0625 * (k % 2))
    if glass:
        s.material.transparency = 0.8
        s.material.reflective = 0.3
        s.material.diffuse = 0.3
    if not shadow:
        s.no_shadow()
    return s


rt_color = None  # (set by build(): the package's Color)


def _lights(rt, w):
    w.add_light(rt.PointLight(rt.Point(-6, 8, -8), rt.Color(1, 1, 1)))
    w.add_light(rt.PointLight(rt.Point(5, 6, -4), rt.Color(0.35, 0.35, 0.35)))


def _camera(rt, frm, axis, up=(0, 1, 0), fov=math.pi / 3):
    """A camera at the dyadic point `frm` looking along `axis`: an orientation of 0 and +-1 only."""
    cam = rt.Camera(W, H, fov)
    to = tuple(f + a for f, a in zip(frm, axis))
    cam.set_transform(rt.view_transform(rt.Point(*frm), rt.Point(*to), rt.Vector(*up)))
    return cam


def _floor(rt, w, y=0.0, glass=False):
    floor = rt.Plane()
    if y != 0.0:
        floor.set_transform(rt.translation(0, y, 0))
    p = rt.checkers_pattern(rt.Color(0.85, 0.85, 0.8), rt.Color(0.25, 0.3, 0.25))
    floor.material.set_pattern(p)
    floor.material.reflective = 0.2
    floor.material.refractive_index = 1.25
    if glass:
        floor.material.transparency = 0.7
    w.add_object(floor)
    return floor


def _diag_spheres(rt, w, centres, r=0.5):
    for c, idx in zip(centres, (1.5, 1.33)):
        s = rt.glass_sphere()
        s.set_transform(rt.translation(*c) * rt.scaling(r, r, r))
        s.material.refractive_index = idx
        s.material.reflective = 0.4
        w.add_object(s)


def _box(rt, c, h):
    s = rt.Cube()
    s.set_transform(rt.translation(*c) * rt.scaling(*h))
    return s


AXES = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))


def _aim(origins, target, axis_dir, spread, seed):
    """Rays from each dyadic origin: one along the exact unit axis direction `axis_dir`, one toward a
    seeded point within `spread` of `target`, normalised."""
    rng = np.random.default_rng(seed)
    out = []
    for o in origins:
        out.append(tuple(o) + tuple(float(x) for x in axis_dir))
        p = np.asarray(target, dtype=np.float64) + rng.uniform(-1, 1, 3) * np.asarray(spread, dtype=np.float64)
        d = p - np.asarray(o, dtype=np.float64)
        if not d.any():
            d = np.asarray(axis_dir, dtype=np.float64) + 0.25
        d = d / np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
        out.append(tuple(o) + tuple(d))
    return out


# ---------------------------------------------------------------- twins
N_PAIRS, N_SINGLES = 48, 32


def _twins(rt, seed=5):
    """48 coincident pairs among 32 single diagonal spheres over a floor: every ray that meets a pair ties
    twice. A pair is glass A against opaque B or glass against glass; its B casts no shadow; half the pairs
    lie next to each other in the world's list, the others' second members come after every other sphere;
    which member comes first is seeded."""
    rnd = random.Random(seed)
    w = rt.World()
    _floor(rt, w)
    later, centres = [], []
    for s in range(N_PAIRS + N_SINGLES):
        i, j = s % 10, s // 10
        c = (-4.5 + i, 0.5 + 0.75 * j, 0.5 * ((3 * i + 5 * j) % 4))
        r = (0.3125, 0.3125, 0.3125) if s % 3 else (0.375, 0.25, 0.3125)  # (every third an ellipsoid)
        place = rt.translation(*c) * rt.scaling(*r)
        if s % 5 >= 3:  # a single
            one = rt.Sphere()
            one.set_transform(place)
            one.material.color = rt.Color(0.3 + 0.05 * i, 0.8 - 0.05 * j, 0.3)
            one.material.reflective = 0.2 * (s % 2)
            w.add_object(one)
            continue
        k = len(centres)
        centres.append((c, r))
        a = _paint(rt.Sphere(), 0, k, glass=True)
        b = _paint(rt.Sphere(), 1, k, glass=(k % 2 == 1), shadow=False)
        a.set_transform(place)
        b.set_transform(place)
        first, second = (a, b) if rnd.random() < 0.5 else (b, a)
        w.add_object(first)
        if k % 2:
            later.append(second)
        else:
            w.add_object(second)
    for s in later:
        w.add_object(s)
    assert len(centres) == N_PAIRS
    _lights(rt, w)
    cam = _camera(rt, (0.0, 2.5, -8.0), (0, 0, 1))
    rays = []
    for k, (c, r) in enumerate(centres):
        if k % 3 == 2:  # (32 of the 48 pairs, of both kinds of placement in the list: the checker's time)
            continue
        outside = (c[0] + 0.125 * (k % 3 - 1), c[1] + 0.125, -4.0)
        inside = (c[0] + 0.0625, c[1], c[2] - 0.125)
        on = (c[0], c[1], c[2] - r[2])  # c = 0 exactly in the sphere's space: a root at t == 0
        rays += _aim([outside, inside, on], c, (0, 0, 1), (r[0] / 2, r[1] / 2, 0), 100 + k)
    return TieWorld("twins", w, cam, rays, ("H", "C", "T0"))


# ---------------------------------------------------------------- flush
def _flush(rt):
    """Coplanar faces seen from outside, by a camera that looks straight down: in each of two mirrored rows
    (the second with every pair inserted the other way round) a glass cube inside a larger one sharing its
    top, a capped cylinder and a capped cone inside cubes with the cap in the cube's top, and a slab whose
    bottom lies in the glass floor's plane (the batch rays look at it from under the floor). The inner
    cube and the cylinder are members of a translated group, their partners top-level objects."""
    w = rt.World()
    slabs = [_paint(_box(rt, (-2.5 + 5.0 * row, 0.125, 3.0), (1, 0.125, 0.5)), 1, row + 3, shadow=False) for row in range(2)]
    w.add_object(slabs[0])  # one slab before the floor in the world's list, one after it
    _floor(rt, w, glass=True)
    w.add_object(slabs[1])
    _diag_spheres(rt, w, ((-1.25, 0.5, 0.0), (1.25, 0.5, 0.0)), r=0.1875)  # (the sphere images; 14 solids: no hierarchy)
    tops = []
    for row, z in enumerate((1.25, -1.25)):
        pairs = []
        g = rt.Group()
        g.set_transform(rt.translation(0.0, 0.25, 0.0))
        outer = _paint(_box(rt, (-2.5, 1.25, z), (1, 1, 1)), 0, row)
        inner = _paint(_box(rt, (-2.5, 1.5, z), (0.75, 0.5, 0.75)), 1, row, shadow=False)  # (in the group: y + 0.25)
        g.add_child(inner)
        pairs.append((outer, None))
        tops.append(((-2.5, 2.25, z), (-2.5, 1.75, z)))
        box2 = _paint(_box(rt, (0.0, 1.25, z), (1, 1, 1)), 0, row + 1)
        can = _paint(rt.Cylinder(-1.0, 1.0, True), 1, row + 1, glass=(row == 0), shadow=False)
        can.set_transform(rt.translation(0.0, 1.5, z) * rt.scaling(0.75, 0.5, 0.75))
        g.add_child(can)
        pairs.append((box2, None))
        tops.append(((0.0, 2.25, z), (0.0, 1.75, z)))
        box3 = _paint(_box(rt, (2.5, 1.25, z), (1, 1, 1)), 0, row + 2)
        cone = _paint(rt.Cone(0.0, 1.0, True), 1, row + 2, shadow=False)
        cone.set_transform(rt.translation(2.5, 1.75, z) * rt.scaling(0.75, 0.5, 0.75))
        pairs.append((box3, cone))
        tops.append(((2.5, 2.25, z), (2.5, 2.125, z)))
        if row == 0:  # this row: the group's members first, then the top-level partners
            w.add_object(g)
            for a, b in pairs:
                if b is not None:
                    w.add_object(b)
                w.add_object(a)
        else:
            for a, b in pairs:
                w.add_object(a)
                if b is not None:
                    w.add_object(b)
            w.add_object(g)
    _lights(rt, w)
    cam = _camera(rt, (0.0, 9.0, 0.0), (0, -1, 0), up=(0, 0, 1))
    rays = []
    for k, (top, inside) in enumerate(tops):
        above = [(top[0] + 0.25 * (j - 1), 5.0, top[2] + 0.125 * j) for j in range(3)]
        rays += _aim(above, top, (0, -1, 0), (0.25, 0, 0.25), 200 + k)
        within = [(inside[0] + 0.125 * (j - 1), inside[1], inside[2] + 0.0625 * j) for j in range(3)]
        rays += _aim(within, (top[0], 0.5, top[2]), (0, -1, 0), (0.25, 0, 0.25), 220 + k)  # away from the top: C
        rays += _aim(within[:2], top, (0, 1, 0), (0.25, 0, 0.25), 240 + k)                  # out through the top: H
        on = [(top[0] + 0.125 * j, top[1], top[2] - 0.125 * j) for j in range(3)]
        rays += _aim(on, (top[0], 0.5, top[2]), (0, -1, 0), (0.25, 0, 0.25), 260 + k)       # on the top: t == 0
    for row in range(2):
        x = -2.5 + 5.0 * row
        under = [(x + 0.25 * (j - 2), -2.0, 3.0 + 0.125 * (j - 2)) for j in range(5)]
        rays += _aim(under, (x, 0.0, 3.0), (0, 1, 0), (0.5, 0, 0.25), 280 + row)            # floor and slab bottom: H
        within = [(x + 0.25 * (j - 2), 0.125, 3.0) for j in range(5)]
        rays += _aim(within, (x, 2.0, 3.0), (0, 1, 0), (0.5, 0, 0.25), 290 + row)           # both behind: C
        on = [(x + 0.25 * (j - 2), 0.0, 3.0) for j in range(5)]
        rays += _aim(on, (x, 2.0, 3.0), (0, 1, 0), (0.5, 0, 0.25), 300 + row)               # t == 0
    return TieWorld("flush", w, cam, rays, ("H", "C", "T0"))


# ---------------------------------------------------------------- lattice
def _lattice_cells():
    return [(i, j, k) for i in range(3) for j in range(2) for k in range(3)]


def _lattice_cube(rt, cell):
    i, j, k = cell
    role = (i + j + k) % 2  # neighbours across a face are of the other role
    s = _paint(_box(rt, (i - 1.0, j + 0.75, float(k)), (0.5, 0.5, 0.5)), role, 0, shadow=(role == 0 or k != 1))
    n = i + 3 * j + 6 * k  # every cell its own colour and index: cells that meet in an edge or a corner tie too
    s.material.color = rt_color(*(WARM if role == 0 else COOL)[:2], 0.1 + 0.04 * n if role == 0 else 0.95 - 0.02 * n)
    s.material.refractive_index = (1.5 if role == 0 else 1.125) + 0.015625 * n
    return s


def _lattice(rt, form, seed=9):
    """3 x 2 x 3 glass unit cubes sharing faces (18 boxed solids: the other records' hierarchy) beside two
    diagonal spheres, inserted in a seeded order, so each shared face has either neighbour first.
    form "top": top-level objects; "divided": children of one group, divided at a threshold that splits
    it; "twins": four cubes replaced by twin spheres under a dyadic shear (general-transform spheres)."""
    rnd = random.Random(seed)
    cells = _lattice_cells()
    rnd.shuffle(cells)
    w = rt.World()
    _floor(rt, w)
    _diag_spheres(rt, w, ((-2.5, 0.5, 0.5), (2.5, 0.5, 1.5)))
    holder = rt.Group() if form == "divided" else w
    add = holder.add_child if form == "divided" else w.add_object
    swapped = ((0, 0, 0), (2, 1, 0), (1, 0, 2), (1, 1, 1)) if form == "twins" else ()
    for n, cell in enumerate(cells):
        if cell in swapped:
            place = rt.translation(cell[0] - 1.0, cell[1] + 0.75, float(cell[2])) * \
                rt.shearing(0.5, 0, 0, 0, 0, 0.25) * rt.scaling(0.5, 0.5, 0.5)
            pair = [_paint(rt.Sphere(), 0, n), _paint(rt.Sphere(), 1, n, glass=(n % 2 == 0), shadow=False)]
            if n % 2:
                pair.reverse()
            for s in pair:
                s.set_transform(place)
                add(s)
        else:
            add(_lattice_cube(rt, cell))
    if form == "divided":
        holder.divide(4)
        w.add_object(holder)
    _lights(rt, w)
    cam = _camera(rt, (0.25, 1.5, -6.0), (0, 0, 1))
    rays = []
    n = 0
    for i, j, k in _lattice_cells():
        c = (i - 1.0, j + 0.75, float(k))
        for axis, idx in ((0, i), (2, k)):  # the faces shared along x and z (3 cells each way)
            if idx == 2:
                continue
            e = AXES[axis]
            face = tuple(c[a] + 0.5 * e[a] for a in range(3))
            inside = tuple(c[a] + 0.125 * (1 - e[a]) for a in range(3))          # in this cell, toward the face: H
            beyond = tuple(face[a] + 0.25 * e[a] + 0.0625 * (1 - e[a]) for a in range(3))  # in the next cell: C-like
            on = [tuple(face[a] + 0.125 * (m - 1) * (1 - e[a]) for a in range(3)) for m in range(3)]  # on the face: t == 0
            spread = tuple(0.25 * (1 - e[a]) for a in range(3))
            rays += _aim([inside], face, e, spread, 400 + n)
            rays += _aim(on, tuple(face[a] + e[a] for a in range(3)), e, spread, 450 + n)
            rays += _aim([beyond], tuple(face[a] + 1.0 * e[a] for a in range(3)), e, spread, 500 + n)
            n += 1
    for j in range(2):  # from outside, through three cells each
        for i in range(3):
            o = (i - 1.0 + 0.125, j + 0.75 - 0.125, -3.0)
            rays += _aim([o], (i - 1.0, j + 0.75, 0.0), (0, 0, 1), (0.25, 0.25, 0), 600 + 3 * j + i)
    name = {"top": "lattice", "divided": "lattice_divided", "twins": "lattice_twins"}[form]
    return TieWorld(name, w, cam, rays, ("H", "T0"))


# ---------------------------------------------------------------- nested
NESTED_ORDERS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))


def _nested(rt):
    """Six triples of glass boxes x in [-1, 1], [-1, 3], [-1, 7] around one axis, sharing the face x = -1, one
    triple per insertion order: an origin inside all three has three bit-equal roots behind it, of which
    `containers` keeps the order. The camera looks along +x at the six shared faces."""
    w = rt.World()
    _floor(rt, w)
    _diag_spheres(rt, w, ((-3.0, 2.5, -1.25), (-3.0, 2.5, 1.25)), r=0.1875)
    sizes = ((0.0, (1, 0.5, 0.5)), (1.0, (2, 0.75, 0.75)), (3.0, (4, 1, 1)))
    centres = []
    for n, order in enumerate(NESTED_ORDERS):
        y, z = 1.25 + 2.5 * (n // 3), -2.5 + 2.5 * (n % 3)
        centres.append((y, z))
        boxes = []
        for m, (cx, h) in enumerate(sizes):
            b = _paint(_box(rt, (cx, y, z), h), 0 if m != 1 else 1, m + n, shadow=(m != 1))
            b.material.refractive_index = (1.5, 1.125, 1.875)[m] + 0.03125 * n
            b.material.color = rt.Color(*((0.9, 0.3, 0.1), (0.1, 0.4, 0.9), (0.8, 0.7, 0.45))[m])
            boxes.append(b)
        for m in order:
            w.add_object(boxes[m])
    _lights(rt, w)
    cam = _camera(rt, (-9.0, 2.5, 0.0), (1, 0, 0))
    rays = []
    for n, (y, z) in enumerate(centres):
        inside = [(-0.5 + 0.25 * j, y + 0.125 * (j - 1), z + 0.0625 * j) for j in range(3)]
        rays += _aim(inside, (1.0, y, z), (1, 0, 0), (0, 0.25, 0.25), 700 + n)    # three roots behind: C3
        rays += _aim(inside[:2], (-1.0, y, z), (-1, 0, 0), (0, 0.25, 0.25), 720 + n)  # three exits at once: H
        outside = [(-4.0, y + 0.125 * j, z - 0.125 * j) for j in range(2)]
        rays += _aim(outside, (-1.0, y, z), (1, 0, 0), (0, 0.25, 0.25), 740 + n)  # three entries at once: H
        on = [(-1.0, y + 0.125 * j, z + 0.125 * (1 - j)) for j in range(3)]
        rays += _aim(on, (1.0, y, z), (1, 0, 0), (0, 0.25, 0.25), 760 + n)        # on the face: t == 0
    return TieWorld("nested", w, cam, rays, ("H", "C", "C3", "T0"))


# ---------------------------------------------------------------- lines
def _lines(rt):
    """Coaxial twin open tubes (6 pairs) and twin open cones (4 pairs), one transform per pair and two
    materials: 20 records, past the line hierarchy's 16. The pairs alternate their insertion order. Some
    batch rays take the cones' |a| < EPSILON branch (d.x^2 + d.z^2 == d.y^2 in the cone's space)."""
    w = rt.World()
    _floor(rt, w)
    _diag_spheres(rt, w, ((-4.0, 0.5, -1.0), (4.0, 0.5, -1.0)))
    spots = []
    for k in range(10):
        cone = k >= 6
        c = (-3.375 + 0.75 * k, 1.25 + 0.25 * (k % 3), 0.5 * (k % 2))
        sc = (0.25, 0.5, 0.25) if not cone else (0.5, 0.5, 0.5)
        if cone:
            c = (-3.0 + 2.0 * (k - 6), 3.0, 1.0)
        place = rt.translation(*c) * rt.scaling(*sc)
        pair = []
        for role in (0, 1):
            s = rt.Cone(-1.0, -0.25, False) if cone else rt.Cylinder(-1.0, 1.0, False)
            _paint(s, role, k, glass=(role == 0 or k % 2 == 0), shadow=(role == 0))
            s.set_transform(place)
            pair.append(s)
        if k % 2:
            pair.reverse()
        for s in pair:
            w.add_object(s)
        spots.append((c, sc, cone))
    _lights(rt, w)
    cam = _camera(rt, (0.0, 2.0, -7.0), (0, 0, 1))
    rays = []
    for k, (c, sc, cone) in enumerate(spots):
        mid = (c[0], c[1] - 0.25, c[2]) if cone else c  # (cone: local y = -0.5, radius 0.5)
        outside = [(mid[0] + 0.0625 * j, mid[1] + 0.0625, -3.0) for j in range(2)]
        rays += _aim(outside, mid, (0, 0, 1), (sc[0] / 4, 0.125, 0), 800 + k)
        inside = [(mid[0] + 0.03125, mid[1] + 0.0625 * j, mid[2] + 0.03125) for j in range(2)]
        rays += _aim(inside, (mid[0], mid[1], mid[2] + 2.0), (0, 0, 1), (sc[0] / 4, 0.125, 0), 820 + k)
        r = sc[0] * (0.5 if cone else 1.0)
        on = [(mid[0], mid[1], mid[2] - r), (mid[0], mid[1] + 0.0625, mid[2] + r)]  # on the wall: c == 0 exactly, a root at t == 0
        rays += _aim(on, (mid[0], mid[1], mid[2] + 2.0), (0, 0, 1), (sc[0] / 4, 0.0625, 0), 840 + k)
        if cone:  # |a| < EPSILON: unit diagonals of the x-y and the z-y planes, and unnormalised ones
            h = math.sqrt(0.5)
            for j, d in enumerate(((h, h, 0.0), (0.0, h, h), (1.0, 1.0, 0.0), (0.0, -1.0, 1.0), (-h, -h, 0.0), (h, -h, 0.0))):
                o = (mid[0] - 0.125 * (j % 3), mid[1] - 0.5 + 0.0625 * j, mid[2] - 0.25)
                rays.append(o + d)
    return TieWorld("lines", w, cam, rays, ("H", "C", "T0"))


# ---------------------------------------------------------------- mesh
def _mesh(rt, cubes=True):
    """test_gpu_mesh_edges.py's tie case (two axis-aligned grids of 32 loose triangles each, corners at the
    integers) and two glass cubes with a face in the first grid's plane z = 0 over one of its quads, one
    added before the triangles and one after. A cube's root and a triangle's come from different formulas:
    whether they tie the checker decides; the triangles among themselves do."""
    import test_gpu_mesh_edges as edges
    w = edges._world(rt)
    if cubes:
        w.add_object(_paint(_box(rt, (1.5, 1.5, 0.5), (0.5, 0.5, 0.5)), 1, 0, shadow=False))
    edges._grid(rt, w, "z")
    edges._grid(rt, w, "x")
    if cubes:
        w.add_object(_paint(_box(rt, (2.5, 2.5, -0.5), (0.5, 0.5, 0.5)), 1, 1, shadow=False))
    cam = _camera(rt, (2.0, 2.0, -5.0), (0, 0, 1))
    rays = [tuple(r) for r in np.vstack([edges._toward(edges.EYE, edges._lattice(), False),
                                         edges._toward(edges.EYE, edges._lattice(), True)])]
    eye = (2.0, 2.0, -5.0)
    pts = [(1.0 + 0.25 * i, 1.0 + 0.25 * j, 0.0) for i in range(9) for j in range(9)]  # both cubes' quads
    rays += [tuple(r) for r in edges._toward(eye, pts, False)] + [tuple(r) for r in edges._toward(eye, pts, True)]
    for i in range(5):  # inside each cube, toward its face in the grid's plane, and on that face
        for c, e in (((1.5, 1.5, 0.5), (0, 0, -1)), ((2.5, 2.5, -0.5), (0, 0, 1))):
            inside = (c[0] - 0.25 + 0.125 * i, c[1] + 0.125, c[2])
            on = (c[0] - 0.25 + 0.125 * i, c[1] - 0.125, 0.0)
            rays += _aim([inside, on], (c[0], c[1], 0.0), e, (0.25, 0.25, 0), 900 + i)
    return TieWorld("mesh" if cubes else "mesh_bare", w, cam, rays, ("H",))


# ---------------------------------------------------------------- csg
N_UNITS = 16


def _csg(rt):
    """16 Csg units, each a glass cube minus a ball at its centre (the cutter stays away from every face),
    each sharing the face z = 0.5 or z = -0.5 with a glass cube that is a top-level object or a member of
    a group, in either insertion order: the unit's surviving root ties with the solid's in the world's
    list. No tie inside any Csg node's own list. 16 units: the units' hierarchy at its default threshold."""
    w = rt.World()
    _floor(rt, w)
    _diag_spheres(rt, w, ((-4.0, 0.5, 0.0), (4.0, 0.5, 0.0)))
    g = rt.Group()
    g.set_transform(rt.translation(0.0, 0.0, 0.5))
    spots, after_group = [], []
    for k in range(N_UNITS):
        i, j = k % 4, k // 4
        c = (-2.25 + 1.5 * i, 0.75 + 1.25 * j, 0.0)
        pz = -1.0 if (k // 2) % 2 == 0 else 1.0  # the partner before the unit along +z, or behind it
        spots.append((c, pz))
        cube = _paint(_box(rt, c, (0.5, 0.5, 0.5)), 0, k)
        ball = _paint(rt.Sphere(), 0, k + 1)
        # (off the centre by no dyadic number: a ray mirrored by the ball grazes no cube's edge exactly)
        ball.set_transform(rt.translation(c[0] + 0.03, c[1] - 0.02, 0.01) * rt.scaling(0.25, 0.25, 0.25))
        unit = rt.Csg(rt.Operation.Difference, cube, ball)
        grouped = j % 2 == 1
        partner = _paint(_box(rt, (c[0], c[1], pz - (0.5 if grouped else 0.0)), (0.5, 0.5, 0.5)), 1, k, shadow=False)
        if grouped:  # the group stands in the middle of the world's list: units before it and after it
            g.add_child(partner)
            (after_group.append if k % 2 else w.add_object)(unit)
        else:
            for s in ((partner, unit) if k % 2 else (unit, partner)):
                w.add_object(s)
    w.add_object(g)
    for unit in after_group:
        w.add_object(unit)
    _lights(rt, w)
    cam = _camera(rt, (0.0, 2.625, -9.0), (0, 0, 1))
    rays = []
    for k, (c, pz) in enumerate(spots):
        face = (c[0], c[1], 0.5 * pz)
        e = (0, 0, pz)
        inside = (c[0] + 0.375, c[1] - 0.375 + 0.0625 * (k % 4), 0.0)   # in the unit's glass, beside the ball
        partner = (c[0] + 0.125, c[1] + 0.0625 * (k % 4), pz)           # in the partner, toward the unit
        on = [(c[0] + 0.25, c[1] - 0.125, 0.5 * pz), (c[0] - 0.3125, c[1] + 0.1875, 0.5 * pz)]
        outside = (c[0] + 0.375, c[1] + 0.375, -4.0)
        rays += _aim([inside] + on, (face[0] + 0.25, face[1] - 0.25, face[2]), e, (0.125, 0.125, 0), 1000 + k)
        rays += _aim([partner], (face[0] + 0.25, face[1] - 0.25, face[2]), (0, 0, -pz), (0.125, 0.125, 0), 1100 + k)
        rays += _aim([outside], (c[0] + 0.375, c[1] + 0.375, 0.0), (0, 0, 1), (0.0625, 0.0625, 0), 1200 + k)
    return TieWorld("csg", w, cam, rays, ("H", "T0"))


BUILDERS = {"twins": _twins, "flush": _flush, "lattice": lambda rt: _lattice(rt, "top"),
            "lattice_divided": lambda rt: _lattice(rt, "divided"), "lattice_twins": lambda rt: _lattice(rt, "twins"),
            "nested": _nested, "lines": _lines, "mesh": _mesh, "csg": _csg,
            # (the mesh world without its cubes: what tests/mesh_ref.py accepts, for the pin of the two checkers)
            "mesh_bare": lambda rt: _mesh(rt, cubes=False)}


def build(rt, name):
    global rt_color
    rt_color = rt.Color
    return BUILDERS[name](rt)


# ---------------------------------------------------------------- what the checker says
class Reversed(csg_ref.CsgRef):
    """The checker with every run of bit-equal t in World::intersect's list turned round."""

    def intersect(self, o, d):
        xs = csg_ref.CsgRef.intersect(self, o, d)
        out, i = [], 0
        while i < len(xs):
            j = i
            while j < len(xs) and xs[j][0] == xs[i][0]:
                j += 1
            out.extend(reversed(xs[i:j]))
            i = j
        return out


def pixel_rays(ref, cam):
    c = np.frombuffer(cam.desc_bytes(), dtype=csg_ref.CAMERA)[0]
    return np.array([list(o) + list(d) for o, d in (ref.ray_for_pixel(c, x, y) for y in range(H) for x in range(W))])


def classify(ref, rays):
    """Per ray, from the checker's list alone: the masks H, T0, C, C3, the winner (-1: no hit) and the
    objects that share the hit's t."""
    n = len(rays)
    out = {k: np.zeros(n, dtype=bool) for k in ("H", "T0", "C", "C3")}
    winner, sharing = np.full(n, -1), [()] * n
    for r, ray in enumerate(rays):
        xs = ref.intersect(ray[:3], ray[3:])
        pos = [x for x in xs if x[0] >= 0.0]
        if not pos:
            continue
        winner[r] = pos[0][1]
        tied = []
        for x in pos:
            if x[0] != pos[0][0]:
                break
            if x[1] not in tied:
                tied.append(x[1])
        sharing[r] = tuple(tied)
        out["H"][r] = len(tied) >= 2
        out["T0"][r] = len(tied) >= 2 and pos[0][0] == 0.0
        neg = xs[:len(xs) - len(pos)]
        if neg:
            containers = []
            for x in neg:
                if x[1] in containers:
                    containers.remove(x[1])
                else:
                    containers.append(x[1])
            at_last = {x[1] for x in neg if x[0] == neg[-1][0]}
            c = sum(1 for i in containers if i in at_last)
            out["C"][r] = c >= 2
            out["C3"][r] = c >= 3
    out["winner"], out["sharing"] = winner, sharing
    return out


def roles(ref):
    """Role A (0) or B (1) of every object, from its colour (WARM: red > blue); a triangle is of role A
    (the mesh world's pairs are a triangle and a cube)."""
    col = ref.s["color"]
    return np.where((col[:, 0] > col[:, 2]) | (ref.s["kind"] >= csg_ref.TRIANGLE), 0, 1)
