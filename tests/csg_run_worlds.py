"""Worlds whose wide or deep Csg units hold long runs of triangle leaves (test infrastructure of
tests/test_gpu_csg_run.py): the run hierarchies' ground. Frames are 32x24 at depth 5. Each maker
returns (world, camera, the unit's box for random rays, fused) and `runs_of(world)` gives what the
plan readout must report, counted from the world itself: a run is a maximal stretch of consecutive
triangle shapes with the same innermost node."""
import math

import numpy as np

import csg_mesh_worlds as base
from csg_mesh_worlds import DEPTH, H, W, beads, camera, glass, lights, material, torus  # noqa: F401

RUN_MIN = 16  # the default csg_run_min (the other hierarchies' kMinHierRecords)


def runs_of(w, under=None):
    """The lengths of the world's runs of triangles under a Csg, in program order."""
    import csg_ref
    import csg_tri_ref
    ref = under if under is not None else csg_tri_ref.CsgTriRef.from_world(w)
    kinds = ref.s["kind"]
    out, prev = [], None
    for i in range(len(kinds)):
        if int(kinds[i]) >= csg_ref.TRIANGLE and i in ref.under_csg:
            node = ref.shape_node[i]
            if prev == node:
                out[-1] += 1
            else:
                out.append(1)
            prev = node
        else:
            prev = None
    return out


def expect(w, refused=0, ref=None):
    """The plan of the world's run hierarchies: every run of RUN_MIN boxed triangles has one."""
    long = [n for n in runs_of(w, ref) if n >= RUN_MIN]
    return dict(runs=len(long), boxed=sum(long) - refused, remainder=refused)


def _floor(rt, w, y=-1.2):
    floor = rt.Plane()
    floor.set_transform(rt.translation(0, y, 0))
    floor.material.color = rt.Color(0.8, 0.8, 0.7)
    floor.material.reflective = 0.2
    w.add_object(floor)


def torus_minus_sphere(rt):
    """An undivided torus of 96 triangles minus a sphere, beside the beads that open the fused generations."""
    w = rt.World()
    _floor(rt, w)
    beads(rt, w)
    ball = rt.Sphere()
    ball.set_transform(rt.translation(1.0, 0.2, -0.2) * rt.scaling(0.7, 0.7, 0.7))
    ball.set_material(material(rt, (0.9, 0.3, 0.6), reflective=0.2))
    w.add_object(rt.Csg(rt.Operation.Difference, torus(rt, 8, 6, material(rt, (0.4, 0.7, 0.9), reflective=0.15)), ball))
    lights(rt, w)
    return w, camera(rt, (-0.5, 2.8, -3.4), (0, 0, 0)), ((-1.5, -0.5, -1.5), (1.5, 0.5, 1.5)), True


def smooth_scaled_nested(rt):
    """The same torus, smooth, under a rotated Csg scaled (0.25, 2, 1) nested in a second, translated Csg: the chained
    ray's |d|_inf reaches 4 and more, and the hit's u and v are the chained ray's."""
    ball = rt.Sphere()
    ball.set_transform(rt.translation(1.0, 0.2, -0.2) * rt.scaling(0.7, 0.7, 0.7))
    ball.set_material(material(rt, (0.9, 0.3, 0.6), reflective=0.2))
    inner = rt.Csg(rt.Operation.Difference, torus(rt, 8, 6, material(rt, (0.3, 0.8, 0.5), reflective=0.25), smooth=True), ball)
    inner.set_transform(rt.rotation_z(0.25) * rt.scaling(0.25, 2.0, 1.0))
    plug = rt.Cylinder(-1.0, 1.0, True)
    plug.set_transform(rt.translation(0.9, 0.0, 0.8) * rt.scaling(0.3, 0.6, 0.3))
    plug.set_material(material(rt, (0.3, 0.3, 0.9), 1.3))
    outer = rt.Csg(rt.Operation.Union, inner, plug)
    outer.set_transform(rt.translation(0.15, 0.1, 0.05))
    w = rt.World()
    _floor(rt, w)
    beads(rt, w)
    w.add_object(outer)
    lights(rt, w)
    return w, camera(rt, (0.3, 1.2, -3.6), (0.1, 0, 0)), ((-0.5, -1.0, -1.5), (1.3, 1.2, 1.5)), True


def _fan(rt, n, x, mat, z=0.0):
    """n triangles about (x, 0.1, z): a jittered fan, open (no two share a coordinate)."""
    g = rt.Group()
    for k in range(n):
        a0, a1 = 2.0 * math.pi * k / n, 2.0 * math.pi * (k + 0.93) / n
        r0, r1 = 0.8 + 0.01 * k, 0.78 + 0.013 * k
        t = rt.Triangle(rt.Point(x + 0.01 * k, 0.1 + 0.004 * k, z + 0.003 * k),
                        rt.Point(x + r0 * math.cos(a0), 0.12 + r0 * math.sin(a0), z + 0.1 + 0.01 * k),
                        rt.Point(x + r1 * math.cos(a1), 0.11 + r1 * math.sin(a1), z - 0.1 - 0.01 * k))
        t.set_material(mat)
        g.add_child(t)
    return g


def threshold(rt):
    """Runs of 15, 16 and 17 triangles, each minus a sphere: the first stays one by one. A floor and wide units
    only: the fast path runs the exhaustive pipeline's kernels, and walks the two hierarchies all the same."""
    w = rt.World()
    _floor(rt, w)
    for j, n in enumerate((15, 16, 17)):
        x = 2.1 * (j - 1)
        ball = rt.Sphere()
        ball.set_transform(rt.translation(x + 0.3, 0.3, 0.0) * rt.scaling(0.45, 0.45, 0.45))
        ball.set_material(material(rt, (0.9, 0.8, 0.2), reflective=0.2))
        w.add_object(rt.Csg(rt.Operation.Difference, _fan(rt, n, x, material(rt, (0.3 + 0.2 * j, 0.5, 0.8 - 0.2 * j))), ball))
    lights(rt, w)
    return w, camera(rt, (0.2, 1.0, -5.5), (0, 0, 0)), ((-3.0, -0.9, -0.4), (3.0, 1.1, 0.4)), False


GRID_Y = 0.25


def flat_grid(rt, light_in_plane=True):
    """32 axis-aligned triangles in the plane y = GRID_Y (a 4 x 4 grid of squares, two each) united with a
    sphere; the camera and one light in that plane."""
    g = rt.Group()
    m = material(rt, (0.8, 0.5, 0.3), reflective=0.2)
    for i in range(4):
        for j in range(4):
            x0, z0 = -1.0 + 0.5 * i, -1.0 + 0.5 * j
            for a, b, c in (((x0, z0), (x0 + 0.5, z0), (x0, z0 + 0.5)), ((x0 + 0.5, z0 + 0.5), (x0, z0 + 0.5), (x0 + 0.5, z0))):
                t = rt.Triangle(rt.Point(a[0], GRID_Y, a[1]), rt.Point(b[0], GRID_Y, b[1]), rt.Point(c[0], GRID_Y, c[1]))
                t.set_material(m)
                g.add_child(t)
    ball = rt.Sphere()
    ball.set_transform(rt.translation(0.2, 0.3, 0.1) * rt.scaling(0.5, 0.5, 0.5))
    ball.set_material(material(rt, (0.2, 0.3, 0.9), 1.4))
    w = rt.World()
    _floor(rt, w)
    beads(rt, w)
    w.add_object(rt.Csg(rt.Operation.Union, g, ball))
    w.add_light(rt.PointLight(rt.Point(-6, 8, -8), rt.Color(1, 1, 1)))
    w.add_light(rt.PointLight(rt.Point(3.0, GRID_Y, -2.0), rt.Color(0.4, 0.4, 0.4)))
    return w, camera(rt, (0.1, GRID_Y, -4.0), (0.0, GRID_Y, 0.0)), ((-1.0, -0.3, -1.0), (1.0, 0.9, 1.0)), True


def grid_plane_rays(n=64, seed=3):
    """Rays in the grid's own plane (origin and direction: y = GRID_Y and 0 exactly), and just off it."""
    rng = np.random.default_rng(seed)
    o = np.column_stack([rng.uniform(-3, 3, n), np.full(n, GRID_Y), rng.uniform(-4, -2, n)])
    aim = np.column_stack([rng.uniform(-1, 1, n), np.full(n, GRID_Y), rng.uniform(-1, 1, n)])
    d = aim - o
    d[n // 2:, 1] = rng.uniform(-2e-5, 2e-5, n - n // 2)  # (grazing: |det| around EPSILON)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[: n // 2, 1] = 0.0
    return np.hstack([o, d])


def drum(rt, n, r, h, mat, centre=(0.0, 0.0, 0.0)):
    """A closed mesh of 4 n triangles: an n-gon prism with fan caps, jittered so that no two vertices share a coordinate."""
    cx, cy, cz = centre
    ring = lambda y, s: [rt.Point(cx + (r + 0.003 * k) * math.cos(2 * math.pi * (k + s) / n), cy + y + 0.002 * k,
                                  cz + (r + 0.002 * k) * math.sin(2 * math.pi * (k + s) / n)) for k in range(n)]
    top, bot = ring(h, 0.07), ring(-h, 0.03)
    ct, cb = rt.Point(cx + 0.011, cy + h + 0.05, cz + 0.007), rt.Point(cx - 0.009, cy - h - 0.04, cz + 0.013)
    g = rt.Group()
    for k in range(n):
        k1 = (k + 1) % n
        for tri in ((ct, top[k1], top[k]), (cb, bot[k], bot[k1]), (top[k], top[k1], bot[k]), (bot[k], top[k1], bot[k1])):
            t = rt.Triangle(*tri)
            t.set_material(mat)
            g.add_child(t)
    return g


def glass_drum_from_inside(rt):
    """A closed glass mesh of 24 triangles minus a glass sphere, the camera inside the mesh: the survivors behind the
    origin on triangle leaves are the hit's containers."""
    ball = rt.Sphere()
    ball.set_transform(rt.translation(0.2, 0.1, 1.5) * rt.scaling(0.8, 0.8, 0.8))
    clear = material(rt, (0.1, 0.2, 0.1), 1.6)
    clear.reflective = 0.0  # (refraction only: the ray tree stays a chain at depth 5)
    ball.set_material(clear)
    pane = material(rt, (0.1, 0.1, 0.2), 1.45)
    pane.reflective = 0.0
    w = rt.World()
    _floor(rt, w, -3.5)
    beads(rt, w)
    w.add_object(rt.Csg(rt.Operation.Difference, drum(rt, 6, 2.0, 1.6, pane), ball))
    lights(rt, w)
    return w, camera(rt, (0.15, 0.1, -0.4), (0.2, 0.0, 2.0), fov=1.4), ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.6)), True


def light_inside(rt):
    """Difference(closed mesh, sphere) with a light inside the mesh: a shadow ray that starts inside the mesh too is
    blocked by the sphere only because the mesh's root BEHIND its origin set the left filter bit."""
    ball = rt.Sphere()
    ball.set_transform(rt.translation(0.1, -0.1, 0.3) * rt.scaling(0.6, 0.6, 0.6))
    ball.set_material(material(rt, (0.9, 0.5, 0.2), reflective=0.1))
    pane = material(rt, (0.1, 0.1, 0.2), 1.2, )
    pane.reflective = 0.0
    w = rt.World()
    _floor(rt, w, -2.5)
    beads(rt, w)
    w.add_object(rt.Csg(rt.Operation.Difference, drum(rt, 5, 2.0, 1.5, pane), ball))
    w.add_light(rt.PointLight(rt.Point(-0.9, 0.6, 0.9), rt.Color(1, 1, 1)))
    w.add_light(rt.PointLight(rt.Point(0.3, 0.4, -1.2), rt.Color(0.4, 0.4, 0.4)))
    return w, camera(rt, (0.3, 0.5, -1.5), (0.1, -0.1, 0.3), fov=1.2), ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.2)), True


def deck_one_run(rt):
    """csg_mesh_worlds.deck_minus_sphere: its 80 parallel triangles are one run (more roots than a batch holds, so a
    second walk from the watermark)."""
    w = base.deck_minus_sphere(rt)
    return w, camera(rt, (1.0, 0.6, -11.0), (0.0, 0.0, 2.0)), ((-1.5, -1.5, -0.5), (1.5, 1.5, 4.5)), True


def with_refused(rt):
    """A run of 20 triangles, two of them under a transform of condition 4e6: tri_box refuses those two."""
    g = _fan(rt, 18, 0.0, material(rt, (0.4, 0.8, 0.4), reflective=0.2))
    for k in range(2):
        x = (-0.9 + 1.2 * k) / 2000.0
        t = rt.Triangle(rt.Point(x, 400.0 + 200.0 * k, 0.6), rt.Point(x + 0.7 / 2000.0, 1000.0, 0.65 + 0.01 * k),
                        rt.Point(x + 0.3 / 2000.0, 1800.0 - 200.0 * k, -0.7))
        t.set_transform(rt.scaling(2000.0, 5.0e-4, 1.0))  # (world x as above times 2000, y = 0.2 .. 0.9)
        t.set_material(material(rt, (0.9, 0.3, 0.3)))
        g.add_child(t)
    ball = rt.Sphere()
    ball.set_transform(rt.translation(0.3, 0.3, 0.0) * rt.scaling(0.45, 0.45, 0.45))
    ball.set_material(material(rt, (0.9, 0.8, 0.2), 1.3))
    w = rt.World()
    _floor(rt, w)
    beads(rt, w)
    w.add_object(rt.Csg(rt.Operation.Difference, g, ball))
    lights(rt, w)
    return w, camera(rt, (0.2, 1.4, -4.0), (0, 0.2, 0)), ((-1.0, -0.9, -0.8), (1.0, 1.1, 0.8)), True


def divided(rt):
    """A torus of 36 triangles divided at threshold 8 (runs of 6 and 12: the triangles no half holds stay in the
    group itself): no run reaches the threshold."""
    ball = rt.Sphere()
    ball.set_transform(rt.translation(1.0, 0.2, -0.2) * rt.scaling(0.7, 0.7, 0.7))
    ball.set_material(material(rt, (0.9, 0.3, 0.6), reflective=0.2))
    c = rt.Csg(rt.Operation.Difference, torus(rt, 6, 3, material(rt, (0.4, 0.7, 0.9))), ball)
    c.divide(8)
    w = rt.World()
    _floor(rt, w)
    beads(rt, w)
    w.add_object(c)
    lights(rt, w)
    return w, camera(rt, (-0.5, 2.8, -3.4), (0, 0, 0)), ((-1.5, -0.5, -1.5), (1.5, 0.5, 1.5)), True


def deep_mesh(rt):
    """A mesh of 64 triangles under 36 Csg nodes (35 unions of thin cubes cut from it): a deep unit (deep_csg=True)."""
    from rtamd import scenes
    w = rt.World()
    _floor(rt, w, -1.0)
    m = material(rt, (0.9, 0.5, 0.2), reflective=0.2)
    ring = scenes._mesh_group(scenes.mesh_torus(8, 4), m, 0)
    cuts = None
    for k in range(36):
        a = 2.0 * math.pi * k / 36.0
        c = rt.Cube()
        c.set_transform(rt.translation(math.cos(a), 0.0, math.sin(a)) * rt.rotation_y(-a) * rt.scaling(0.55, 0.55, 0.03))
        c.material.color = rt.Color(0.2, 0.3 + 0.015 * k, 0.8)
        if k % 4 == 1:
            glass(c.material, 1.3 + 0.01 * k)
        cuts = c if cuts is None else rt.Csg(rt.Operation.Union, cuts, c)
    w.add_object(rt.Csg(rt.Operation.Difference, ring, cuts))
    lights(rt, w)
    return w, camera(rt, (0.3, 2.6, -3.6), (0, 0, 0)), ((-1.5, -0.5, -1.5), (1.5, 0.5, 1.5)), False


WORLDS = {"torus_minus_sphere": torus_minus_sphere, "smooth_scaled_nested": smooth_scaled_nested, "threshold": threshold,
          "flat_grid": flat_grid, "glass_drum_from_inside": glass_drum_from_inside, "light_inside": light_inside,
          "deck_one_run": deck_one_run, "with_refused": with_refused, "divided": divided, "deep_mesh": deep_mesh}
REFUSED = {"with_refused": 2}
DEEP = {"deep_mesh"}
