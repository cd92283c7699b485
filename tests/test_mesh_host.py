"""Triangle, SmoothTriangle and the OBJ parser on the host (CPU only): the
reference's constructor, bounding-box and parser KATs (triangle.rs:105-210,
smooth_triangle.rs:113-200, obj_parser/mod.rs:203-340 on its own seven data
files under tests/golden/obj/), groups of triangles, and the validation of
rt_scene_create_mesh that needs no device."""
import ctypes
import os
import time

import numpy as np
import pytest

from conftest import PKG, REPO

import mesh_ref

OBJ = os.path.join(REPO, "tests", "golden", "obj")
LIB = os.path.join(PKG, "lib", "librtamd.so")
RT_ERR_INVALID_ARGUMENT, RT_ERR_UNSUPPORTED_SHAPE, RT_ERR_DUPLICATE_SHAPES = -1, -2, -5


def _tri(rt):
    return rt.Triangle(rt.Point(0, 1, 0), rt.Point(-1, 0, 0), rt.Point(1, 0, 0))


def _smooth(rt):
    return rt.SmoothTriangle(rt.Point(0, 1, 0), rt.Point(-1, 0, 0), rt.Point(1, 0, 0), rt.Vector(0, 1, 0),
                             rt.Vector(-1, 0, 0), rt.Vector(1, 0, 0))


def test_construct_triangle(rt):  # triangle.rs:105-120
    t = _tri(rt)
    assert t.kind == 5
    assert t.p1 == rt.Point(0, 1, 0) and t.p2 == rt.Point(-1, 0, 0) and t.p3 == rt.Point(1, 0, 0)
    assert t.e1 == rt.Vector(-1, -1, 0) and t.e2 == rt.Vector(1, -1, 0) and t.normal == rt.Vector(0, 0, -1)


def test_construct_smooth_triangle(rt):  # smooth_triangle.rs:113-131
    t = _smooth(rt)
    assert t.kind == 6
    assert t.p1 == rt.Point(0, 1, 0) and t.p2 == rt.Point(-1, 0, 0) and t.p3 == rt.Point(1, 0, 0)
    assert t.n1 == rt.Vector(0, 1, 0) and t.n2 == rt.Vector(-1, 0, 0) and t.n3 == rt.Vector(1, 0, 0)
    assert t.e1 == rt.Vector(-1, -1, 0) and t.e2 == rt.Vector(1, -1, 0) and t.normal == rt.Vector(0, 0, -1)


@pytest.mark.parametrize("smooth", [False, True])
def test_triangle_bounding_box(rt, smooth):  # triangle.rs:199-209, smooth_triangle.rs:186-199
    p = (rt.Point(-3, 7, 2), rt.Point(6, 2, -4), rt.Point(2, -1, -1))
    s = rt.SmoothTriangle(*p, rt.Vector(0, 1, 0), rt.Vector(-1, 0, 0), rt.Vector(1, 0, 0)) if smooth else rt.Triangle(*p)
    bb = s.get_bounds()
    assert bb.min == rt.Point(-3, -1, -4) and bb.max == rt.Point(6, 7, 2)


# ---- obj_parser/mod.rs:203-340
def test_obj_ignores_unrecognized_lines(rt):
    assert rt.parse_obj_file(os.path.join(OBJ, "gibberish.obj")).ignored == 5


def test_obj_vertex_records(rt):
    p = rt.parse_obj_file(os.path.join(OBJ, "vertex_records.obj"))
    assert len(p.vertices) == 5
    assert p.vertices[1] == rt.Point(-1, 1, 0) and p.vertices[2] == rt.Point(-1.0, 0.5, 0.0)
    assert p.vertices[3] == rt.Point(1, 0, 0) and p.vertices[4] == rt.Point(1, 1, 0)


def test_obj_triangle_faces(rt):
    p = rt.parse_obj_file(os.path.join(OBJ, "triangle_faces.obj"))
    g = p.group("default")
    t1, t2 = g.child(0), g.child(1)
    assert t1.kind == 5 and t2.kind == 5
    assert (t1.p1, t1.p2, t1.p3) == (p.vertices[1], p.vertices[2], p.vertices[3])
    assert (t2.p1, t2.p2, t2.p3) == (p.vertices[1], p.vertices[3], p.vertices[4])


def test_obj_polygon_is_fan_triangulated(rt):
    p = rt.parse_obj_file(os.path.join(OBJ, "triangulate_polygons.obj"))
    g = p.group("default")
    assert g.n_children() == 3
    for k, (a, b, c) in enumerate([(1, 2, 3), (1, 3, 4), (1, 4, 5)]):
        t = g.child(k)
        assert (t.p1, t.p2, t.p3) == (p.vertices[a], p.vertices[b], p.vertices[c])


def test_obj_triangles_in_groups(rt):
    p = rt.parse_obj_file(os.path.join(OBJ, "triangles.obj"))
    t1, t2 = p.group("FirstGroup").child(0), p.group("SecondGroup").child(0)
    assert (t1.p1, t1.p2, t1.p3) == (p.vertices[1], p.vertices[2], p.vertices[3])
    assert (t2.p1, t2.p2, t2.p3) == (p.vertices[1], p.vertices[3], p.vertices[4])


def test_obj_as_group(rt):
    """convert_obj_file_to_group; the children come in the order of the `g` lines
    (the reference's HashMap order is unspecified, its KAT accepts either)."""
    p = rt.parse_obj_file(os.path.join(OBJ, "triangles.obj"))
    v = list(p.vertices)
    g = p.as_group()
    assert g.n_children() == 2  # the empty default group is left out
    t1, t2 = g.child(0).child(0), g.child(1).child(0)
    assert (t1.p1, t1.p2, t1.p3) == (v[1], v[2], v[3])
    assert (t2.p1, t2.p2, t2.p3) == (v[1], v[3], v[4])
    # a file without `g` lines: the default group itself
    q = rt.parse_obj_file(os.path.join(OBJ, "triangle_faces.obj"))
    assert q.as_group().n_children() == 2


def test_obj_vertex_normals(rt):
    p = rt.parse_obj_file(os.path.join(OBJ, "vertex_normals.obj"))
    assert p.normals[1] == rt.Vector(0, 0, 1) and p.normals[2] == rt.Vector(0.707, 0.0, -0.707)
    assert p.normals[3] == rt.Vector(1, 2, 3)


def test_obj_faces_with_normals(rt):
    p = rt.parse_obj_file(os.path.join(OBJ, "faces_with_normals.obj"))
    g = p.group("default")
    t1, t2 = g.child(0), g.child(1)
    assert t1.kind == 6 and t2.kind == 6
    assert (t1.p1, t1.p2, t1.p3) == (p.vertices[1], p.vertices[2], p.vertices[3])
    assert (t1.n1, t1.n2, t1.n3) == (p.normals[3], p.normals[1], p.normals[2])
    assert t1.desc_bytes() == t2.desc_bytes()
    assert all(getattr(t1, k) == getattr(t2, k) for k in ("p1", "p2", "p3", "n1", "n2", "n3"))


def test_obj_parse_line_and_string(rt):  # test_parse_line, and the string entry point
    p = rt.ObjParser()
    p.parse_line("v  7.0000 0.0000 12.0000")
    assert p.vertices[1] == rt.Point(7, 0, 12)
    q = rt.parse_obj_string("v 0 0 0\r\nv 1 0 0\nv 0 1 0\n\nf 1 2 3\nsomething else\n")
    assert q.ignored == 1 and q.group("default").n_children() == 1


@pytest.mark.parametrize("text", ["v 1 2\n", "v 1 x 3\n", "v 0 0 0\nf 1 2 3\n", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 -1\n",
                                  "vn 0 1\n", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1//1 2//1 3//1\n", "g\n"])
def test_obj_malformed_input_raises(rt, text):
    with pytest.raises(rt.RtError):
        rt.parse_obj_string(text)


# ---- groups of triangles
def test_group_of_triangles_divides_and_flattens(rt):
    from rtamd import scenes
    g = rt.parse_obj_string(scenes.mesh_torus(6, 6)).as_group()
    assert g.n_children() == 72 and all(g.child(k).kind == 5 for k in range(72))
    m = rt.Material()
    m.color = rt.Color(0.1, 0.2, 0.3)
    g.set_material(m)
    g.set_transform(rt.translation(1, 2, 3) * rt.scaling(2, 2, 2))
    g.divide(4)
    w = rt.World()
    w.add_object(g)
    shapes = np.frombuffer(w.descs_bytes(), dtype=mesh_ref.SHAPE)
    groups = np.frombuffer(w.groups_bytes(), dtype=mesh_ref.GROUP)
    tris = np.frombuffer(w.triangles_bytes(), dtype=mesh_ref.TRI)
    sg = np.array(w.shape_groups())
    assert len(shapes) == len(tris) == 72 and (shapes["kind"] == 5).all()
    assert len(groups) > 3 and groups["parent"][0] == -1 and (groups["parent"][1:] >= 0).all()
    assert (groups["parent"] < np.arange(len(groups))).all()  # parents first
    assert (sg >= 0).all()
    # baked transform and material on every triangle; the vertices stay in object space
    assert np.allclose(shapes["transform"][:, [0, 3, 7, 11]], [2.0, 1.0, 2.0, 3.0])
    assert np.allclose(shapes["color"], [0.1, 0.2, 0.3])
    # every triangle's world vertices lie in the box of its innermost group
    for i in range(72):
        M = shapes["transform"][i].reshape(4, 4)
        for k in ("p1", "p2", "p3"):
            p = M[:3, :3] @ tris[k][i] + M[:3, 3]
            gr = groups[sg[i]]
            assert (p >= gr["min"] - 1e-9).all() and (p <= gr["max"] + 1e-9).all()
    # the same vertices as the parser's faces, as a set (divide reorders the children)
    v = np.array([[float(x) for x in ln.split()[1:]] for ln in scenes.mesh_torus(6, 6).splitlines() if ln.startswith("v ")])
    assert {tuple(p) for p in tris["p1"]} <= {tuple(p) for p in v}


# ---- rt_scene_create_mesh: validation that needs no device
def _lib():
    lib = ctypes.CDLL(LIB)
    lib.rt_last_error.restype = ctypes.c_char_p
    P, S = ctypes.c_void_p, ctypes.c_size_t
    lib.rt_scene_create_mesh.argtypes = [P, S, P, P, S, P, S, P, S, ctypes.c_int, ctypes.POINTER(P)]
    lib.rt_scene_create_groups.argtypes = [P, S, P, P, S, P, S, ctypes.c_int, ctypes.POINTER(P)]
    lib.rt_scene_create.argtypes = [P, S, P, S, ctypes.c_int, ctypes.POINTER(P)]
    return lib


def _descs(n, kind):
    s = np.zeros(n, dtype=mesh_ref.SHAPE)
    s["kind"] = kind
    s["casts_shadow"] = 1
    s["transform"] = s["inverse"] = s["pattern_transform"] = s["pattern_inverse"] = np.eye(4).ravel()
    s["color"] = 1.0
    s["ambient"], s["diffuse"], s["specular"], s["shininess"], s["refractive_index"] = 0.1, 0.9, 0.9, 200.0, 1.0
    s["pattern_kind"] = -1
    return s


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


# an ordinal no machine has: the call ends right after validation, with RT_ERR_NO_DEVICE (no
# GPU) or RT_ERR_INVALID_ARGUMENT "bad device ordinal" (a GPU), and never uploads anything
NO_SUCH_DEVICE = 1 << 20


def _create_mesh(lib, shapes, tris, n_tris=None):
    out = ctypes.c_void_p()
    rc = lib.rt_scene_create_mesh(_ptr(shapes), len(shapes), None, None, 0, _ptr(tris), len(tris) if n_tris is None else n_tris,
                                  None, 0, NO_SUCH_DEVICE, ctypes.byref(out))
    assert not out.value
    return rc, lib.rt_last_error().decode()


def _passed_validation(rc, msg):
    return rc in (-1, -8) and ("bad device ordinal" in msg or "no HIP device" in msg)


def _two_triangles():
    t = np.zeros(2, dtype=mesh_ref.TRI)
    t["p1"], t["p2"], t["p3"] = [0, 1, 0], [-1, 0, 0], [1, 0, 0]
    return t


def test_create_mesh_n_tris_mismatch():
    lib = _lib()
    rc, msg = _create_mesh(lib, _descs(2, 5), _two_triangles(), n_tris=1)
    assert rc == RT_ERR_INVALID_ARGUMENT and "n_tris" in msg
    s = _descs(2, 5)
    s["kind"][1] = 0
    rc, msg = _create_mesh(lib, s, _two_triangles())
    assert rc == RT_ERR_INVALID_ARGUMENT and "n_tris" in msg


def test_create_mesh_duplicate_face_is_refused():
    rc, msg = _create_mesh(_lib(), _descs(2, 5), _two_triangles())
    assert rc == RT_ERR_DUPLICATE_SHAPES and "structurally equal" in msg


@pytest.mark.parametrize("kind", [5, 6])
def test_create_mesh_triangles_differing_in_one_field_are_not_duplicates(kind):
    lib = _lib()
    t = _two_triangles()
    t["p3"][1] = [1, 0, 0.5]  # only p3 differs
    rc, msg = _create_mesh(lib, _descs(2, kind), t)
    assert _passed_validation(rc, msg), (rc, msg)
    t = _two_triangles()
    t["n2"][1] = [0, 0, 1]  # only a normal differs: equal as Triangles, distinct as SmoothTriangles
    rc, msg = _create_mesh(lib, _descs(2, kind), t)
    if kind == 5:
        assert rc == RT_ERR_DUPLICATE_SHAPES
    else:
        assert _passed_validation(rc, msg), (rc, msg)


def test_create_without_vertices_still_refuses_triangles():
    lib = _lib()
    s = _descs(1, 5)
    out = ctypes.c_void_p()
    want = "shape 0: supported kinds are Sphere, Plane, Cube, Cylinder, Cone"
    assert lib.rt_scene_create(_ptr(s), 1, None, 0, 0, ctypes.byref(out)) == RT_ERR_UNSUPPORTED_SHAPE
    assert lib.rt_last_error().decode() == want
    assert lib.rt_scene_create_groups(_ptr(s), 1, None, None, 0, None, 0, 0, ctypes.byref(out)) == RT_ERR_UNSUPPORTED_SHAPE
    assert lib.rt_last_error().decode() == want
    assert lib.rt_scene_create_mesh(_ptr(s), 1, None, None, 0, None, 0, None, 0, 0, ctypes.byref(out)) == RT_ERR_UNSUPPORTED_SHAPE
    assert lib.rt_last_error().decode() == want
    s["kind"] = 7
    rc, msg = _create_mesh(lib, s, _two_triangles()[:1])
    assert rc == RT_ERR_UNSUPPORTED_SHAPE and "SmoothTriangle" in msg


def test_duplicate_sweep_of_a_large_mesh_is_fast():
    """100 000 triangles of a regular grid (one transform and one material, as the
    faces of an OBJ file) pass the duplicate sweep in less time than the parent
    commit takes for 100 000 spheres spread on x, the case its sweep was written
    for. Measured on the build machine, best of five calls that end right after
    validation:
      parent, 100 000 spheres at x = 3 k in shuffled order (as a scene's random
        spheres come)                                              0.023 s
      parent, the same spheres listed in ascending x               0.006 s
      this sweep, the grid below                                   0.014 s
      this sweep, the spheres: shuffled 0.011 s, ascending         0.003 s
    The bound is the parent's shuffled figure: the grid's keys come unsorted too.
    (Listed in ascending x the parent's sort has nothing to do, and the grid does
    not beat that 0.006 s.) The parent's key, the translation alone, would put all
    5e9 pairs of the grid into one window."""
    lib = _lib()
    n = 100_000
    side = 224  # 224 x 224 cells, two triangles each: 100 352
    ij = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2).astype(np.float64)
    t = np.zeros(2 * len(ij), dtype=mesh_ref.TRI)
    z = np.zeros(len(ij))
    a = np.column_stack([ij[:, 0], z, ij[:, 1]])
    t["p1"][0::2], t["p2"][0::2], t["p3"][0::2] = a, a + [1, 0, 0], a + [1, 0, 1]
    t["p1"][1::2], t["p2"][1::2], t["p3"][1::2] = a, a + [1, 0, 1], a + [0, 0, 1]
    t = t[:n].copy()
    s = _descs(n, 5)
    best = float("inf")
    for _ in range(5):
        t0 = time.perf_counter()
        rc, msg = _create_mesh(lib, s, t)
        best = min(best, time.perf_counter() - t0)
        assert _passed_validation(rc, msg), (rc, msg)
    print(f"duplicate sweep, 100 000 grid triangles: {best:.3f} s")
    assert best < PARENT_SPHERES_ON_X_S
    # a face listed twice is still found in it
    t[n - 1] = t[12345]
    rc, msg = _create_mesh(lib, s, t)
    assert rc == RT_ERR_DUPLICATE_SHAPES and "12345" in msg


PARENT_SPHERES_ON_X_S = 0.023
