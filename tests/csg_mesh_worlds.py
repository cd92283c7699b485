"""Worlds with triangles under a `Csg` (test infrastructure, shared by tests/test_csg_tri_ref.py
and tests/test_gpu_csg_mesh.py): the known-answer slab, the small worlds, the deck of more roots
than one batch holds, and the worlds beyond the caps. Frames are 32x24 at depth 5."""
import math
import os

import numpy as np

W, H, DEPTH = 32, 24, 5
OBJ = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "obj")


def camera(rt, frm, to, w=W, h=H, fov=math.pi / 3):
    cam = rt.Camera(w, h, fov)
    cam.set_transform(rt.view_transform(rt.Point(*frm), rt.Point(*to), rt.Vector(0, 1, 0)))
    return cam


def lights(rt, w, two=True):
    w.add_light(rt.PointLight(rt.Point(-6, 8, -8), rt.Color(1, 1, 1)))
    if two:
        w.add_light(rt.PointLight(rt.Point(5, 6, -4), rt.Color(0.35, 0.35, 0.35)))


def glass(m, index, transparency=0.9):
    m.transparency = transparency
    m.refractive_index = index
    m.reflective = 0.3
    m.diffuse = 0.2
    return m


def material(rt, color, index=None, reflective=0.0):
    m = rt.Material()
    m.color = rt.Color(*color)
    m.reflective = reflective
    if index is not None:
        glass(m, index)
    return m


def beads(rt, w):
    """Two small diagonal glass spheres: the sphere hierarchy that opens the fused generations."""
    for x, idx in ((-2.6, 1.5), (2.7, 1.33)):
        s = rt.glass_sphere()
        s.set_transform(rt.translation(x, 0.4, 1.2) * rt.scaling(0.4, 0.4, 0.4))
        s.material.refractive_index = idx
        s.material.reflective = 0.4
        w.add_object(s)


def tetrahedron(rt, centre, size, mat, smooth=False):
    """A closed mesh of four triangles in a Group (no two vertices share a coordinate)."""
    v = [(1.0, 1.03, 0.98), (1.02, -1.0, -0.97), (-0.99, 1.01, -1.0), (-1.0, -0.98, 1.02)]
    p = [rt.Point(centre[0] + size * a, centre[1] + size * b, centre[2] + size * c) for a, b, c in v]
    n = [rt.Vector(a, b, c) for a, b, c in v]  # (outward at each vertex, not normalised: as an OBJ file may give them)
    g = rt.Group()
    for a, b, c in ((0, 1, 2), (0, 3, 1), (0, 2, 3), (1, 3, 2)):
        t = rt.SmoothTriangle(p[a], p[b], p[c], n[a], n[b], n[c]) if smooth else rt.Triangle(p[a], p[b], p[c])
        t.set_material(mat)
        g.add_child(t)
    return g


def torus(rt, nu, nv, mat, smooth=False, seed=0x5EED0007):
    from rtamd import scenes
    g = rt.parse_obj_string(scenes.mesh_torus(nu, nv, smooth, seed)).as_group()
    g.set_material(mat)
    return g


# ---------------------------------------------------------------- the known answers
KNOWN_RAY = (0.1, 0.1, -5.0, 0.0, 0.0, 1.0)
KNOWN_INSIDE = (0.1, 0.1, 1.0, 0.0, 0.0, 1.0)
KNOWN_T = {"Union": [5.0, 7.0], "Intersection": [5.5, 6.5], "Difference": [5.0, 5.5, 6.5, 7.0]}
# from KNOWN_INSIDE the roots are -1 (triangle 0), -0.5 and 0.5 (the sphere, object 2), 1 (triangle 1):
# (object hit, t, hin as `inside`-independent n1 and n2) worked by hand from csg.rs:22-41 and intersection.rs:63-90
KNOWN_INSIDE_HIT = {"Union": (1, 1.0, 1.1, 1.2),          # survivors -1, 1: container [tri 0], then tri 1 enters
                    "Intersection": (2, 0.5, 1.5, 1.0),   # survivors -0.5, 0.5: container [sphere], the sphere leaves
                    "Difference": (2, 0.5, 1.5, 1.1)}     # all four: containers [tri 0, sphere], the sphere leaves


def known_answer(rt, op):
    """A slab of two triangles at z = 0 and z = 2 (indices 1.1 and 1.2), each far wider than the ray's
    path, and a sphere of radius 0.5 about (0.1, 0.1, 1) (index 1.5): every coordinate the ray meets is
    a small dyadic number, so every t below is exact."""
    slab = rt.Group()
    for z, idx in ((0.0, 1.1), (2.0, 1.2)):
        t = rt.Triangle(rt.Point(-4, -4, z), rt.Point(4, -4, z), rt.Point(0, 4, z))
        t.set_material(material(rt, (0.8, 0.3, 0.2), idx))
        slab.add_child(t)
    ball = rt.Sphere()
    ball.set_transform(rt.translation(0.1, 0.1, 1.0) * rt.scaling(0.5, 0.5, 0.5))
    ball.set_material(material(rt, (0.2, 0.3, 0.8), 1.5))
    w = rt.World()
    w.add_object(rt.Csg(getattr(rt.Operation, op), slab, ball))
    lights(rt, w, False)
    return w


# ---------------------------------------------------------------- the small worlds
def _floor(rt, w, y=-1.2):
    floor = rt.Plane()
    floor.set_transform(rt.translation(0, y, 0))
    floor.material.color = rt.Color(0.8, 0.8, 0.7)
    floor.material.reflective = 0.2
    w.add_object(floor)


def tetra_minus_sphere(rt):
    w = rt.World()
    _floor(rt, w)
    beads(rt, w)
    ball = rt.Sphere()
    ball.set_transform(rt.translation(0.35, 0.3, -0.5) * rt.scaling(0.8, 0.8, 0.8))
    ball.set_material(material(rt, (0.2, 0.7, 0.3), reflective=0.3))
    w.add_object(rt.Csg(rt.Operation.Difference, tetrahedron(rt, (0, 0.1, 0), 1.1, material(rt, (0.9, 0.4, 0.2))), ball))
    lights(rt, w)
    return w, camera(rt, (0.7, 1.6, -5.0), (0, 0, 0)), ((-1.2, -1.1, -1.2), (1.2, 1.3, 1.2))


def cube_and_torus(rt):
    w = rt.World()
    _floor(rt, w)
    beads(rt, w)
    cube = rt.Cube()
    cube.set_transform(rt.translation(0.5, 0.0, 0.0) * rt.rotation_y(0.3) * rt.scaling(0.9, 0.6, 0.9))
    cube.set_material(material(rt, (0.3, 0.4, 0.9), 1.4))
    w.add_object(rt.Csg(rt.Operation.Intersection, cube, torus(rt, 8, 6, material(rt, (0.9, 0.8, 0.2), reflective=0.2))))
    lights(rt, w)
    return w, camera(rt, (0.4, 2.4, -4.0), (0.3, 0, 0)), ((-0.5, -0.6, -1.0), (1.5, 0.6, 1.0))


def smooth_nested(rt):
    """A smooth torus union a sphere under two nested Csgs, each rotated and scaled unevenly: the ray the
    triangles are handed is the world ray through both inverses, and so are the hit's u and v."""
    ball = rt.Sphere()
    ball.set_transform(rt.translation(0.9, 0.1, 0.0) * rt.scaling(0.5, 0.5, 0.5))
    ball.set_material(material(rt, (0.8, 0.2, 0.2)))
    inner = rt.Csg(rt.Operation.Union, torus(rt, 8, 6, material(rt, (0.3, 0.8, 0.5), reflective=0.25), smooth=True), ball)
    inner.set_transform(rt.rotation_z(0.25) * rt.scaling(1.05, 0.9, 1.1))
    plug = rt.Cylinder(-1.0, 1.0, True)
    plug.set_transform(rt.translation(-1.0, 0.0, 0.1) * rt.scaling(0.35, 1.0, 0.35))
    plug.set_material(material(rt, (0.3, 0.3, 0.9), 1.3))
    outer = rt.Csg(rt.Operation.Difference, inner, plug)
    outer.set_transform(rt.rotation_x(-0.3) * rt.rotation_y(0.4) * rt.scaling(0.95, 1.15, 0.9))
    w = rt.World()
    _floor(rt, w)
    beads(rt, w)
    w.add_object(outer)
    lights(rt, w)
    return w, camera(rt, (0.3, 2.6, -3.6), (0, 0, 0)), ((-1.5, -0.6, -1.5), (1.5, 0.6, 1.5))


def divided_mesh(rt):
    """A mesh in a Group in a Csg, divided: subgroup gates inside the unit."""
    ball = rt.Sphere()
    ball.set_transform(rt.translation(1.0, 0.2, -0.2) * rt.scaling(0.7, 0.7, 0.7))
    ball.set_material(material(rt, (0.9, 0.3, 0.6), reflective=0.2))
    c = rt.Csg(rt.Operation.Difference, torus(rt, 6, 4, material(rt, (0.4, 0.7, 0.9))), ball)
    c.divide(4)
    assert c.left.n_children() < 48  # (divided: subgroups, not the 48 triangles)
    w = rt.World()
    _floor(rt, w)
    beads(rt, w)
    w.add_object(c)
    lights(rt, w)
    return w, camera(rt, (-0.5, 2.8, -3.4), (0, 0, 0)), ((-1.5, -0.5, -1.5), (1.5, 0.5, 1.5))


def in_moved_group(rt):
    """A wide unit inside a transformed top-level group (the Csg's own transform takes the product)."""
    cube = rt.Cube()
    cube.set_transform(rt.translation(0.6, 0.2, 0.3) * rt.scaling(0.6, 0.6, 0.6))
    cube.set_material(material(rt, (0.2, 0.5, 0.9), 1.25))
    g = rt.Group()
    g.add_child(rt.Csg(rt.Operation.Union, tetrahedron(rt, (0, 0, 0), 0.9, material(rt, (0.9, 0.6, 0.1)), smooth=True), cube))
    extra = rt.Sphere()
    extra.set_transform(rt.translation(-1.8, 0.1, 0.5) * rt.scaling(0.5, 0.5, 0.5))
    g.add_child(extra)
    g.set_transform(rt.translation(0.3, 0.1, 0.2) * rt.rotation_y(0.5) * rt.scaling(1.1, 0.9, 1.0))
    w = rt.World()
    _floor(rt, w)
    beads(rt, w)
    w.add_object(g)
    lights(rt, w)
    return w, camera(rt, (0.5, 1.8, -4.6), (0, 0, 0)), ((-1.0, -1.0, -1.0), (1.4, 1.0, 1.2))


def glass_from_inside(rt):
    """A glass Difference with the camera inside it: survivors behind the origin on triangle leaves."""
    ball = rt.Sphere()
    ball.set_transform(rt.translation(0.2, 0.1, 1.3) * rt.scaling(0.7, 0.7, 0.7))
    clear = material(rt, (0.1, 0.2, 0.1), 1.6)
    clear.reflective = 0.0  # (refraction only: the ray tree stays a chain at depth 5)
    ball.set_material(clear)
    pane = material(rt, (0.1, 0.1, 0.2), 1.45)
    pane.reflective = 0.0
    w = rt.World()
    _floor(rt, w, -3.5)
    beads(rt, w)
    w.add_object(rt.Csg(rt.Operation.Difference, tetrahedron(rt, (0, 0, 0), 2.4, pane), ball))
    lights(rt, w)
    return w, camera(rt, (0.15, 0.1, -0.4), (0.2, 0.0, 2.0), fov=1.4), ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.6))


def obj_minus_sphere(rt):
    """tests/golden/obj/triangles.obj (two named groups of one triangle each) as the left of a Difference."""
    g = rt.parse_obj_file(os.path.join(OBJ, "triangles.obj")).as_group()
    g.set_material(material(rt, (0.9, 0.5, 0.2), reflective=0.2))
    ball = rt.Sphere()
    ball.set_transform(rt.translation(0.15, 0.45, 0.05) * rt.scaling(0.4, 0.4, 0.4))
    ball.set_material(material(rt, (0.3, 0.3, 0.9)))
    w = rt.World()
    _floor(rt, w, -0.6)
    beads(rt, w)
    w.add_object(rt.Csg(rt.Operation.Difference, g, ball))
    lights(rt, w)
    return w, camera(rt, (0.6, 0.9, -2.6), (0, 0.4, 0)), ((-1.0, 0.0, -0.4), (1.0, 1.0, 0.4))


SMALL = {"tetra_minus_sphere": tetra_minus_sphere, "cube_and_torus": cube_and_torus, "smooth_nested": smooth_nested,
         "divided_mesh": divided_mesh, "in_moved_group": in_moved_group, "glass_from_inside": glass_from_inside,
         "obj_minus_sphere": obj_minus_sphere}


def random_rays(box, n=256, seed=5):
    """n rays, a third of them from inside `box` (the unit's), the others aimed at it from around it."""
    rng = np.random.default_rng(seed)
    lo, hi = np.array(box[0]), np.array(box[1])
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    o = mid + rng.normal(size=(n, 3)) * 3.0 * (half.max() + 1.0)
    d = mid + rng.uniform(-1, 1, size=(n, 3)) * half - o
    inside = n // 3
    o[:inside] = rng.uniform(lo, hi, size=(inside, 3))
    d[:inside] = rng.normal(size=(inside, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.hstack([o, d])


# ---------------------------------------------------------------- more roots than one batch
DECK = 80


def deck_minus_sphere(rt):
    """80 parallel glass triangles 0.05 apart (z = 0 .. 3.95) minus a glass sphere through the middle."""
    deck = rt.Group()
    for k in range(DECK):
        z = 0.05 * k
        t = rt.Triangle(rt.Point(-3.0 - 0.001 * k, -2.5, z), rt.Point(3.0, -2.4 - 0.001 * k, z), rt.Point(0.1, 3.0 + 0.001 * k, z))
        t.set_material(material(rt, (0.1, 0.15, 0.2), 1.02 + 0.002 * k, ))
        deck.add_child(t)
    ball = rt.Sphere()
    ball.set_transform(rt.translation(0.05, 0.1, 2.0) * rt.scaling(0.6, 0.6, 0.6))
    ball.set_material(material(rt, (0.2, 0.1, 0.1), 1.5))
    w = rt.World()
    beads(rt, w)
    w.add_object(rt.Csg(rt.Operation.Difference, deck, ball))
    lights(rt, w, False)
    return w


def deck_rays():
    """Along the deck's normal: from in front, from behind, and from the middle both ways (beside and through the sphere)."""
    rays = []
    for x, y in ((0.05, 0.1), (0.3, -0.2), (1.4, 0.6), (-1.1, -0.9)):
        rays += [(x, y, -2.0, 0.011, 0.007, 1.0), (x, y, 6.0, -0.009, 0.006, -1.0),
                 (x, y, 3.321, 0.004, -0.003, 1.0), (x, y, 3.321, 0.002, 0.005, -1.0), (x, y, 3.987, -0.003, 0.002, -1.0)]
    r = np.array(rays, dtype=np.float64)
    r[:, 3:] /= np.linalg.norm(r[:, 3:], axis=1, keepdims=True)
    return r


# ---------------------------------------------------------------- beyond the caps
def _tri(rt, k, z=0.0, lone=False):
    """A mesh of one face: the triangle in a Group (a lone triangle as a Csg's own child stays refused)."""
    t = rt.Triangle(rt.Point(0.3 * k, 0.0, z), rt.Point(0.3 * k + 0.25, 0.01 * k, z), rt.Point(0.3 * k + 0.1, 0.3, z + 0.001 * k))
    if lone:
        return t
    g = rt.Group()
    g.add_child(t)
    return g


def too_many_primitives(rt, n=17):
    """n primitives of kinds 0-4 and one triangle in one unit."""
    g = rt.Group()
    for k in range(n):
        s = rt.Sphere()
        s.set_transform(rt.translation(0.25 * k, 1.0, 0.0) * rt.scaling(0.1, 0.1, 0.1))
        g.add_child(s)
    return rt.Csg(rt.Operation.Union, g, _tri(rt, 0))


def too_many_nodes(rt, n=33):
    """n Csg nodes in one unit, two levels deep: a group of n - 1 Csgs of two triangles each under one Csg."""
    g = rt.Group()
    for k in range(n - 1):
        g.add_child(rt.Csg(rt.Operation.Union, _tri(rt, 2 * k), _tri(rt, 2 * k + 1, 0.5)))
    return rt.Csg(rt.Operation.Union, g, _tri(rt, 2 * n, 1.0))


def too_deep(rt, levels=5):
    node = _tri(rt, 0)
    for k in range(levels):
        node = rt.Csg(rt.Operation.Union, node, _tri(rt, k + 1, 0.2 * k))
    return node


def equal_triangles(rt):
    return rt.Csg(rt.Operation.Union, _tri(rt, 3), _tri(rt, 3))


def lone_triangle(rt):
    """A triangle as a Csg's own child, outside any Group: the refusal that is kept."""
    return rt.Csg(rt.Operation.Difference, rt.Sphere(), _tri(rt, 1, lone=True))


def narrow_at_the_caps(rt):
    """16 spheres under 4 levels of Csg nodes: today's caps exactly."""
    items = []
    for k in range(16):
        s = rt.Sphere()
        s.set_transform(rt.translation(0.25 * k - 2.0, 0.1 * (k % 3), 0.05 * k) * rt.scaling(0.3, 0.3, 0.3))
        items.append(s)
    while len(items) > 1:
        items = [rt.Csg(rt.Operation.Union, items[i], items[i + 1]) for i in range(0, len(items), 2)]
    return items[0]
