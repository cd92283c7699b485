"""Worlds in which shapes are structurally equal (rt_scene_create_aliased): the reference renders them with equal
shapes aliasing in the `containers` walk of prepare_computations (intersection.rs:63-90). Shared by
tests/test_alias_worlds.py (CPU: aliasing changes every one of these frames) and tests/test_gpu_alias.py (GPU: the
library's frames equal the oracle's).

Every world holds a light, a checkered floor, a striped back wall and four diagonal spheres and a cube in view behind
the glass (so the fast path is fused and builds its hierarchies); what is named is added to that. The frames are
32x24 at depth 5. The oracle (oracle/rt_oracle.c) walks by structural equality; the checker of tests/csg_ref.py walks
by object identity, which is what a renderer does that takes equal shapes for distinct ones.
"""
import math

W, H, DEPTH = 32, 24, 5
NUDGE = 5e-6  # below EPSILON = 1e-5 (lib.rs:18): the nudged twin is still `==`


def _camera(rt, frm, to, fov=0.9):
    cam = rt.Camera(W, H, fov)
    cam.set_transform(rt.view_transform(rt.Point(*frm), rt.Point(*to), rt.Vector(0, 1, 0)))
    return cam


def _backdrop(rt, floor_y=-3.0):
    w = rt.World()
    w.add_light(rt.PointLight(rt.Point(-8.0, 12.0, -14.0), rt.Color(1.0, 1.0, 1.0)))
    floor = rt.Plane()
    floor.set_transform(rt.translation(0, floor_y, 0))
    floor.material.set_pattern(rt.checkers_pattern(rt.Color(0.85, 0.85, 0.85), rt.Color(0.15, 0.2, 0.3)))
    floor.material.specular = 0.0
    w.add_object(floor)
    wall = rt.Plane()
    wall.set_transform(rt.translation(0, 0, 14.0) * rt.rotation_x(math.pi / 2))
    p = rt.stripe_pattern(rt.Color(0.9, 0.3, 0.2), rt.Color(0.2, 0.5, 0.9))
    p.set_transform(rt.scaling(0.7, 0.7, 0.7) * rt.rotation_y(0.5))
    wall.material.set_pattern(p)
    wall.material.specular = 0.0
    w.add_object(wall)
    for k, (x, y, z) in enumerate(((-2.6, -1.0, 6.0), (-0.9, 1.4, 7.0), (1.1, -0.6, 6.5), (2.7, 1.2, 7.5))):
        s = rt.Sphere()
        s.set_transform(rt.translation(x, y, z) * rt.scaling(0.8, 0.8 + 0.1 * k, 0.8))
        s.material.color = rt.Color(0.9 - 0.2 * k, 0.2 + 0.2 * k, 0.3 + 0.1 * k)
        w.add_object(s)
    c = rt.Cube()
    c.set_transform(rt.translation(0.2, 2.6, 8.0) * rt.rotation_y(0.4) * rt.scaling(0.6, 0.4, 0.6))
    c.material.color = rt.Color(0.3, 0.7, 0.4)
    c.material.reflective = 0.2
    w.add_object(c)
    return w


def _glass(shape, index=1.5, color=(1.0, 1.0, 1.0)):
    m = shape.material
    m.transparency = 1.0
    m.refractive_index = index
    m.diffuse = 0.1
    m.ambient = 0.05
    m.color = type(m.color)(*color)
    return shape


def _twins(rt, make, place, nudges):
    """`make()` placed by `place`, once per nudge: the first unmoved, the others nudged along x."""
    out = []
    for dx in nudges:
        s = make()
        s.set_transform(rt.translation(dx, 0, 0) * place if dx else place)
        out.append(s)
    return out


def concentric_outside(rt):
    w = _backdrop(rt)
    for s in _twins(rt, lambda: _glass(rt.Sphere()), rt.scaling(1.6, 1.6, 1.6), (0.0, 0.0)):
        w.add_object(s)
    return w, _camera(rt, (0.0, 0.3, -6.0), (0.0, 0.0, 0.0))


def concentric_inside(rt):
    w = _backdrop(rt)
    for s in _twins(rt, lambda: _glass(rt.Sphere()), rt.scaling(1.6, 1.6, 1.6), (0.0, 0.0)):
        w.add_object(s)
    return w, _camera(rt, (0.2, 0.1, -0.4), (0.0, 0.2, 6.0), fov=1.3)


def near_pair(rt):
    w = _backdrop(rt)
    for s in _twins(rt, lambda: _glass(rt.Sphere(), 1.7), rt.translation(0.3, 0.2, 0.5) * rt.scaling(1.5, 1.3, 1.5), (0.0, NUDGE)):
        w.add_object(s)
    return w, _camera(rt, (0.0, 0.3, -6.0), (0.0, 0.0, 0.0))


def clique_of_three(rt):
    w = _backdrop(rt)
    for s in _twins(rt, lambda: _glass(rt.Sphere(), 1.4), rt.translation(-0.2, 0.0, 0.0) * rt.scaling(1.5, 1.5, 1.5),
                    (0.0, 3e-6, 6e-6)):
        w.add_object(s)
    return w, _camera(rt, (0.0, 0.3, -6.0), (0.0, 0.0, 0.0))


def enclosing(rt):
    """A different glass sphere around a duplicated pair: the pair is the second container from the top."""
    w = _backdrop(rt)
    outer = _glass(rt.Sphere(), 2.0)
    outer.set_transform(rt.scaling(2.2, 2.2, 2.2))
    w.add_object(outer)
    for s in _twins(rt, lambda: _glass(rt.Sphere(), 1.3), rt.scaling(1.2, 1.2, 1.2), (0.0, 0.0)):
        w.add_object(s)
    return w, _camera(rt, (0.0, 0.3, -6.5), (0.0, 0.0, 0.0))


def enclosed(rt):
    """A different glass sphere inside a duplicated pair, listed between the twins."""
    w = _backdrop(rt)
    a, b = _twins(rt, lambda: _glass(rt.Sphere(), 1.3), rt.scaling(2.0, 2.0, 2.0), (0.0, NUDGE))
    inner = _glass(rt.Sphere(), 2.0)
    inner.set_transform(rt.translation(0.2, 0.0, 0.0) * rt.scaling(0.9, 0.9, 0.9))
    w.add_object(a)
    w.add_object(inner)
    w.add_object(b)
    return w, _camera(rt, (0.0, 0.3, -6.5), (0.0, 0.0, 0.0))


def planes_behind(rt):
    """Two coincident glass planes behind the camera (each ray has one root t < 0 on each: they cancel), a glass
    sphere ahead."""
    w = _backdrop(rt)
    for s in _twins(rt, lambda: _glass(rt.Plane(), 2.0), rt.translation(0, 0, -9.0) * rt.rotation_x(math.pi / 2), (0.0, 0.0)):
        w.add_object(s)
    ball = _glass(rt.Sphere(), 1.5)
    ball.set_transform(rt.scaling(1.5, 1.5, 1.5))
    w.add_object(ball)
    return w, _camera(rt, (0.0, 0.3, -6.0), (0.0, 0.0, 0.0))


def _inside_solid(rt, make, place, frm):
    w = _backdrop(rt, floor_y=-7.0)
    for s in _twins(rt, lambda: _glass(make(), 1.5), place, (0.0, NUDGE)):
        w.add_object(s)
    return w, _camera(rt, frm, (0.0, 0.2, 6.0), fov=1.2)


def cubes_inside(rt):
    return _inside_solid(rt, rt.Cube, rt.rotation_y(0.3) * rt.scaling(2.5, 2.0, 2.5), (0.1, 0.2, -0.5))


def cylinders_inside(rt):
    return _inside_solid(rt, lambda: rt.Cylinder(-1.0, 1.0, True), rt.rotation_x(0.4) * rt.scaling(2.5, 2.0, 2.5), (0.1, 0.2, -0.5))


def cones_inside(rt):
    # a closed single cone, apex up: the camera sits below the apex, inside
    return _inside_solid(rt, lambda: rt.Cone(-1.0, 0.0, True), rt.translation(0, 2.0, 0) * rt.scaling(3.5, 4.0, 3.5), (0.1, -0.8, -0.3))


def grouped_twin(rt):
    """One member inside a group (with a small sphere; rays past the group's box skip both), its twin at the top level."""
    w = _backdrop(rt)
    place = rt.translation(0.9, 0.4, 0.0) * rt.scaling(1.3, 1.3, 1.3)
    inside, twin = _twins(rt, lambda: _glass(rt.Sphere(), 1.6), place, (0.0, 0.0))
    g = rt.Group()
    g.add_child(inside)
    small = rt.Sphere()
    small.set_transform(rt.translation(0.9, 2.0, 0.0) * rt.scaling(0.3, 0.3, 0.3))
    small.material.color = rt.Color(0.9, 0.8, 0.1)
    g.add_child(small)
    w.add_object(g)
    w.add_object(twin)
    return w, _camera(rt, (0.0, 0.3, -6.0), (0.0, 0.0, 0.0))


def opaque_pair(rt):
    """An opaque duplicated pair (refractive index 2) around the camera and a glass sphere: by identity the glass is
    entered from index 2, by equality from 1."""
    w = _backdrop(rt)

    def shell():
        s = rt.Sphere()
        s.material.refractive_index = 2.0
        s.material.color = rt.Color(0.6, 0.7, 0.9)
        s.material.ambient = 0.4
        return s
    for s in _twins(rt, shell, rt.scaling(5.0, 5.0, 5.0), (0.0, 0.0)):
        w.add_object(s)
    ball = _glass(rt.Sphere(), 1.5)
    ball.material.reflective = 0.6
    ball.set_transform(rt.translation(0, 0, 1.5) * rt.scaling(1.2, 1.2, 1.2))
    w.add_object(ball)
    w.add_light(rt.PointLight(rt.Point(-1.0, 2.5, -3.0), rt.Color(0.8, 0.8, 0.8)))
    return w, _camera(rt, (0.0, 0.3, -3.5), (0.0, 0.0, 1.5))


from mesh_ref import SHAPE  # noqa: E402  (rt_shape_desc as a numpy record)

SHAPE_DESC_BYTES = SHAPE.itemsize


def librtamd():
    import ctypes
    import os

    from conftest import PKG
    lib = ctypes.CDLL(os.path.join(PKG, "lib", "librtamd.so"))
    lib.rt_last_error.restype = ctypes.c_char_p
    return lib


def equal_pairs(descs_bytes, lib=None):
    """rt_shapes_equal_pairs over rt_shape_desc bytes: [(i, j), ...], sorted (the two-call protocol of the header)."""
    import ctypes

    import numpy as np
    lib = lib or librtamd()
    n = len(descs_bytes) // SHAPE_DESC_BYTES
    assert n * SHAPE_DESC_BYTES == len(descs_bytes)
    found = ctypes.c_size_t(0)
    rc = lib.rt_shapes_equal_pairs(descs_bytes, ctypes.c_size_t(n), None, ctypes.c_size_t(0), ctypes.byref(found))
    assert rc in (0, -7), (rc, lib.rt_last_error())  # RT_ERR_BUFFER_TOO_SMALL: the pairs did not fit in cap = 0
    assert (rc == 0) == (found.value == 0)
    out = np.zeros((found.value, 2), dtype=np.int32)
    if found.value:
        rc = lib.rt_shapes_equal_pairs(descs_bytes, ctypes.c_size_t(n), out.ctypes.data_as(ctypes.c_void_p),
                                       ctypes.c_size_t(found.value), ctypes.byref(found))
        assert rc == 0 and found.value == len(out), (rc, lib.rt_last_error())
    return [(int(a), int(b)) for a, b in out]


WORLDS = {
    "concentric_outside": concentric_outside,
    "concentric_inside": concentric_inside,
    "near_pair": near_pair,
    "clique_of_three": clique_of_three,
    "enclosing": enclosing,
    "enclosed": enclosed,
    "planes_behind": planes_behind,
    "cubes_inside": cubes_inside,
    "cylinders_inside": cylinders_inside,
    "cones_inside": cones_inside,
    "grouped_twin": grouped_twin,
    "opaque_pair": opaque_pair,
}
# name -> (members of alias classes, classes), as rt_shapes_equal_pairs must find them
CLASSES = {name: (3, 1) if name == "clique_of_three" else (2, 1) for name in WORLDS}

# A scene file that places a glass sphere and a cube twice (the reference's render_scene renders such files).
TWICE_YAML = """
- add: camera
  width: 16
  height: 12
  field-of-view: 0.9
  from: [0, 1, -6]
  to: [0, 0, 0]
  up: [0, 1, 0]
- add: light
  at: [-5, 8, -8]
  intensity: [1, 1, 1]
- define: glass
  value:
    transparency: 1.0
    refractive-index: 1.5
    diffuse: 0.1
- add: plane
  transform:
    - [translate, 0, -2, 0]
  material:
    pattern:
      type: checkers
      colors: [[1, 1, 1], [0.2, 0.2, 0.2]]
- add: sphere
  material: glass
  transform:
    - [scale, 1.5, 1.5, 1.5]
- add: sphere
  material: glass
  transform:
    - [scale, 1.5, 1.5, 1.5]
- add: cube
  transform:
    - [translate, 3, 0, 2]
- add: cube
  transform:
    - [translate, 3, 0, 2]
"""
