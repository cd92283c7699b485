"""Host side of alias classes (CPU only; nothing here reaches a device).

rt_shapes_equal_pairs must give exactly the oracle's or_shape_equals (oracle/rt_oracle.c:410, the derived PartialEq
of the reference's shapes, bounding box included) on descs built by a constructor and at most one set_transform: a
table of pairs, each asked of both. rt_scene_create_aliased's validation: bad pairs are RT_ERR_INVALID_ARGUMENT; a
component that is no clique, an aliased triangle and an aliased primitive under a Csg are RT_ERR_DUPLICATE_SHAPES with
a message that says which. Every call names a device ordinal no machine has (tests/test_mesh_host.py): a call that
passes validation ends with "no HIP device" or "bad device ordinal", before any upload. tests/cpp/alias_check.cpp
runs the component / clique split and the pair helper under the address and undefined-behaviour sanitizers.
"""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import alias_worlds as aw
import csg_ref
import mesh_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "raytracer-challenge-rs_amd", "csrc")
RT_ERR_INVALID_ARGUMENT, RT_ERR_DUPLICATE_SHAPES = -1, -5
NO_SUCH_DEVICE = 1 << 20
NAN = float("nan")


# ---- the oracle's shapes (oracle/rt_oracle.h), to ask or_shape_equals
class _T3(ctypes.Structure):
    _fields_ = [("x", ctypes.c_double), ("y", ctypes.c_double), ("z", ctypes.c_double)]


class _Mat(ctypes.Structure):
    _fields_ = [("rows", ctypes.c_int), ("cols", ctypes.c_int), ("e", ctypes.c_double * 16)]


class _Box(ctypes.Structure):
    _fields_ = [("min", _T3), ("max", _T3)]


class _Pattern(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int), ("a", _T3), ("b", _T3), ("transform", _Mat), ("inverse", _Mat)]


class _Material(ctypes.Structure):
    _fields_ = [("color", _T3)] + [(n, ctypes.c_double) for n in (
        "ambient", "diffuse", "specular", "shininess", "reflective", "transparency", "refractive_index")] + [
        ("has_pattern", ctypes.c_int), ("pattern", _Pattern)]


class _Shape(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int), ("transform", _Mat), ("inverse", _Mat), ("inverse_t", _Mat),
                ("material", _Material), ("bbox", _Box), ("shadow", ctypes.c_int), ("minimum", ctypes.c_double),
                ("maximum", ctypes.c_double), ("closed", ctypes.c_int), ("gate", ctypes.c_int)]


class _World(ctypes.Structure):
    _fields_ = [("objects", ctypes.POINTER(_Shape)), ("n", ctypes.c_int), ("cap", ctypes.c_int)]


def oracle_equals(oracle, descs):
    """or_shape_equals(objects[0], objects[1]) of the oracle's world built from the two descs."""
    ow = oracle.OracleWorld(descs.tobytes())
    wp = ctypes.cast(ctypes.c_void_p(ow._w), ctypes.POINTER(_World)).contents
    assert wp.n == 2
    # the mirror above is the oracle's layout: the fields it rebuilt read back as the descs'
    for k in range(2):
        o = wp.objects[k]
        assert o.kind == descs["kind"][k] and o.shadow == (1 if descs["casts_shadow"][k] else 0)
        assert list(o.transform.e) == list(descs["transform"][k]) and o.transform.rows == 4
        ri = descs["refractive_index"][k]
        assert o.material.refractive_index == ri or (math.isnan(ri) and math.isnan(o.material.refractive_index))
        assert o.closed == descs["closed"][k] and o.gate == 0
    f = oracle.lib().or_shape_equals
    f.restype = ctypes.c_int
    return bool(f(ctypes.byref(wp.objects[0]), ctypes.byref(wp.objects[1])))


def _desc(rt, shape, transform=None, **fields):
    if transform is not None:
        shape.set_transform(transform)
    d = np.frombuffer(shape.desc_bytes(), dtype=mesh_ref.SHAPE).copy()
    for k, v in fields.items():
        d[k] = v
    return d


def _pair(a, b):
    return np.concatenate([a, b])


def _patterned(rt, kind="stripe", b=(0.1, 0.3, 0.8), transform=None):
    s = rt.Sphere()
    p = getattr(rt, kind + "_pattern")(rt.Color(0.9, 0.2, 0.1), rt.Color(*b)) if kind != "test" else rt.test_pattern()
    if transform is not None:
        p.set_transform(transform)
    s.material.set_pattern(p)
    return s


def _table(rt):
    """name -> (the two descs, what the reference's `==` gives, None where only agreement with the oracle is asked)."""
    T = rt.translation
    place = T(1.0, 2.0, 3.0) * rt.rotation_y(0.4) * rt.scaling(1.5, 0.7, 1.2)
    t = {}
    t["identical_default"] = (_pair(_desc(rt, rt.Sphere()), _desc(rt, rt.Sphere())), True)
    t["identical_placed"] = (_pair(_desc(rt, rt.Sphere(), place), _desc(rt, rt.Sphere(), place)), True)
    t["nudged_5e-6"] = (_pair(_desc(rt, rt.Sphere(), place), _desc(rt, rt.Sphere(), T(5e-6, 0, 0) * place)), True)
    t["nudged_2e-5"] = (_pair(_desc(rt, rt.Sphere(), place), _desc(rt, rt.Sphere(), T(2e-5, 0, 0) * place)), False)
    t["default_and_nudged"] = (_pair(_desc(rt, rt.Sphere()), _desc(rt, rt.Sphere(), T(5e-6, 0, 0))), True)
    t["casts_shadow"] = (_pair(_desc(rt, rt.Sphere()), _desc(rt, rt.Sphere(), casts_shadow=0)), False)
    t["other_kind"] = (_pair(_desc(rt, rt.Sphere()), _desc(rt, rt.Cube())), False)
    t["cubes"] = (_pair(_desc(rt, rt.Cube(), place), _desc(rt, rt.Cube(), T(0, -5e-6, 0) * place)), True)
    t["cylinders"] = (_pair(_desc(rt, rt.Cylinder(-1, 2, True), place), _desc(rt, rt.Cylinder(-1, 2, True), place)), True)
    t["cylinder_bound"] = (_pair(_desc(rt, rt.Cylinder(-1, 2, True)), _desc(rt, rt.Cylinder(-1, 2.000001, True))), False)
    t["cylinder_closed"] = (_pair(_desc(rt, rt.Cylinder(-1, 2, True)), _desc(rt, rt.Cylinder(-1, 2, False))), False)
    t["cones"] = (_pair(_desc(rt, rt.Cone(-1, 0.5, True), place), _desc(rt, rt.Cone(-1, 0.5, True), T(0, 0, 5e-6) * place)), True)
    t["cone_bound"] = (_pair(_desc(rt, rt.Cone(-1, 0.5, True)), _desc(rt, rt.Cone(-1.000001, 0.5, True))), False)
    for field in ("ambient", "diffuse", "specular", "shininess", "reflective", "transparency", "refractive_index"):
        a = _desc(rt, rt.glass_sphere(), place)
        b = a.copy()
        b[field] = np.nextafter(a[field], 10.0)  # one ulp: Material's f64 fields compare exactly
        t["material_" + field] = (_pair(a, b), False)
    a = _desc(rt, rt.Sphere())
    t["colour_5e-6"] = (_pair(a, _desc(rt, rt.Sphere(), color=a["color"] + [0, 5e-6, 0])), True)
    t["colour_2e-5"] = (_pair(a, _desc(rt, rt.Sphere(), color=a["color"] + [0, 2e-5, 0])), False)
    t["nan_index"] = (_pair(_desc(rt, rt.Sphere(), refractive_index=NAN), _desc(rt, rt.Sphere(), refractive_index=NAN)), False)
    t["nan_colour"] = (_pair(_desc(rt, rt.Sphere(), color=[1, NAN, 1]), _desc(rt, rt.Sphere(), color=[1, NAN, 1])), False)
    t["nan_bound"] = (_pair(_desc(rt, rt.Cylinder(-1, 2, True), maximum=NAN), _desc(rt, rt.Cylinder(-1, 2, True), maximum=NAN)), False)
    pt = rt.scaling(0.5, 0.5, 0.5) * rt.rotation_z(0.3)
    t["patterned"] = (_pair(_desc(rt, _patterned(rt, transform=pt), place), _desc(rt, _patterned(rt, transform=pt), place)), True)
    t["patterned_test"] = (_pair(_desc(rt, _patterned(rt, "test")), _desc(rt, _patterned(rt, "test"))), True)
    t["pattern_colour"] = (_pair(_desc(rt, _patterned(rt)), _desc(rt, _patterned(rt, b=(0.1, 0.3, 0.80002)))), False)
    t["pattern_colour_near"] = (_pair(_desc(rt, _patterned(rt)), _desc(rt, _patterned(rt, b=(0.1, 0.3, 0.800005)))), True)
    t["pattern_kind"] = (_pair(_desc(rt, _patterned(rt)), _desc(rt, _patterned(rt, "ring"))), False)
    t["pattern_transform"] = (_pair(_desc(rt, _patterned(rt, transform=pt)), _desc(rt, _patterned(rt, transform=rt.scaling(0.5, 0.5, 0.51)))), False)
    t["pattern_and_none"] = (_pair(_desc(rt, _patterned(rt)), _desc(rt, rt.Sphere())), False)
    # every matrix entry within EPSILON, the boxes' corners not (three entries add up): equal descs, unequal shapes
    t["box_only"] = (_pair(_desc(rt, rt.Cube(), T(0, 0, 1)), _desc(rt, rt.Cube(), T(0, 0, 1) * rt.shearing(6e-6, 6e-6, 0, 0, 0, 0))), False)
    # boxes with infinite and (after set_transform's 0 * inf) empty sides: whatever the reference's rules give
    t["planes_default"] = (_pair(_desc(rt, rt.Plane()), _desc(rt, rt.Plane())), True)
    t["planes_placed"] = (_pair(_desc(rt, rt.Plane(), T(0, 1, 0)), _desc(rt, rt.Plane(), T(0, 1, 0))), None)
    t["plane_default_and_nudged"] = (_pair(_desc(rt, rt.Plane()), _desc(rt, rt.Plane(), T(0, 5e-6, 0))), None)
    t["tubes_default"] = (_pair(_desc(rt, rt.Cylinder()), _desc(rt, rt.Cylinder())), True)
    t["tubes_placed"] = (_pair(_desc(rt, rt.Cylinder(), place), _desc(rt, rt.Cylinder(), place)), None)
    t["tube_default_and_nudged"] = (_pair(_desc(rt, rt.Cylinder()), _desc(rt, rt.Cylinder(), T(5e-6, 0, 0))), None)
    return t


TABLE_NAMES = ["identical_default", "identical_placed", "nudged_5e-6", "nudged_2e-5", "default_and_nudged", "casts_shadow",
               "other_kind", "cubes", "cylinders", "cylinder_bound", "cylinder_closed", "cones", "cone_bound",
               "material_ambient", "material_diffuse", "material_specular", "material_shininess", "material_reflective",
               "material_transparency", "material_refractive_index", "colour_5e-6", "colour_2e-5", "nan_index",
               "nan_colour", "nan_bound", "patterned", "patterned_test", "pattern_colour", "pattern_colour_near",
               "pattern_kind", "pattern_transform", "pattern_and_none", "box_only", "planes_default", "planes_placed",
               "plane_default_and_nudged", "tubes_default", "tubes_placed", "tube_default_and_nudged"]


@pytest.fixture(scope="module")
def table(rt):
    t = _table(rt)
    assert sorted(t) == sorted(TABLE_NAMES)
    return t


@pytest.mark.parametrize("name", TABLE_NAMES)
def test_equal_pairs_is_the_oracles_relation(oracle, table, name):
    descs, want = table[name]
    got = aw.equal_pairs(descs.tobytes())
    assert got in ([], [(0, 1)])
    ref = oracle_equals(oracle, descs)
    assert (got == [(0, 1)]) == ref, (name, got, ref)
    if want is not None:
        assert ref == want, (name, ref)


# ---- rt_scene_create_aliased: validation
def _lib():
    lib = aw.librtamd()
    P, S = ctypes.c_void_p, ctypes.c_size_t
    lib.rt_scene_create_aliased.argtypes = [P, S, P, P, P, S, P, S, P, S, P, S, ctypes.c_int, ctypes.POINTER(P)]
    return lib


def _ptr(a):
    return None if a is None or len(a) == 0 else a.ctypes.data_as(ctypes.c_void_p)


def _create(descs, pairs, tris=None, nodes=None, shape_node=None, shape_side=None):
    lib = _lib()
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    sn = None if shape_node is None else np.ascontiguousarray(shape_node, dtype=np.int32)
    ss = None if shape_side is None else np.ascontiguousarray(shape_side, dtype=np.int32)
    out = ctypes.c_void_p()
    rc = lib.rt_scene_create_aliased(_ptr(descs), len(descs), _ptr(sn), _ptr(ss), _ptr(nodes), 0 if nodes is None else len(nodes),
                                     _ptr(tris), 0 if tris is None else len(tris), None, 0, _ptr(pairs), len(pairs),
                                     NO_SUCH_DEVICE, ctypes.byref(out))
    assert not out.value
    return rc, lib.rt_last_error().decode()


def _passed_validation(rc, msg):
    return rc in (-1, -8) and ("bad device ordinal" in msg or "no HIP device" in msg)


def _spheres(rt, xs):
    return np.concatenate([_desc(rt, rt.Sphere(), rt.translation(x, 0, 0) if x else None) for x in xs])


def test_good_pairs_pass_validation(rt):
    three = _spheres(rt, (0.0, 3e-6, 6e-6))
    for pairs in ([(0, 1), (0, 2), (1, 2)], [(0, 1)], [(1, 2)], []):  # (an unlisted pair is distinct: no refusal)
        rc, msg = _create(three, pairs)
        assert _passed_validation(rc, msg), (pairs, rc, msg)
    assert aw.equal_pairs(three.tobytes()) == [(0, 1), (0, 2), (1, 2)]


@pytest.mark.parametrize("pairs,what", [
    ([(0, 3)], "needs 0 <= i < j"), ([(-1, 1)], "needs 0 <= i < j"), ([(1, 0)], "needs 0 <= i < j"), ([(1, 1)], "needs 0 <= i < j"),
    ([(1, 2), (0, 1)], "sorted"), ([(0, 2), (0, 1)], "sorted"), ([(0, 1), (0, 1)], "sorted"),
])
def test_bad_pairs_are_invalid_arguments(rt, pairs, what):
    rc, msg = _create(_spheres(rt, (0.0, 0.0, 0.0)), pairs)
    assert rc == RT_ERR_INVALID_ARGUMENT and what in msg, (rc, msg)


def test_a_pair_that_cannot_be_equal_is_an_invalid_argument(rt):
    descs = np.concatenate([_desc(rt, rt.Sphere()), _desc(rt, rt.Cube()), _desc(rt, rt.Sphere(), rt.translation(2e-5, 0, 0))])
    for pair in ((0, 1), (0, 2)):
        rc, msg = _create(descs, [pair])
        assert rc == RT_ERR_INVALID_ARGUMENT and "differ in a field" in msg, (pair, rc, msg)


def test_a_chain_is_refused(rt):
    """Translations 0, 6e-6 and 1.2e-5: A == B, B == C, A != C (`equal()` is |a - b| < EPSILON)."""
    chain = _spheres(rt, (0.0, 6e-6, 1.2e-5))
    pairs = aw.equal_pairs(chain.tobytes())
    assert pairs == [(0, 1), (1, 2)]
    rc, msg = _create(chain, pairs)
    assert rc == RT_ERR_DUPLICATE_SHAPES and "not transitive" in msg and "shapes 0 and 2" in msg, (rc, msg)


def test_an_aliased_triangle_is_refused():
    s = np.zeros(2, dtype=mesh_ref.SHAPE)
    s["kind"], s["casts_shadow"], s["color"], s["pattern_kind"] = 5, 1, 1.0, -1
    s["transform"] = s["inverse"] = s["pattern_transform"] = s["pattern_inverse"] = np.eye(4).ravel()
    s["ambient"], s["diffuse"], s["specular"], s["shininess"], s["refractive_index"] = 0.1, 0.9, 0.9, 200.0, 1.0
    t = np.zeros(2, dtype=mesh_ref.TRI)
    t["p1"], t["p2"], t["p3"] = [0, 1, 0], [-1, 0, 0], [1, 0, 0]
    rc, msg = _create(s, [(0, 1)], tris=t)
    assert rc == RT_ERR_DUPLICATE_SHAPES and "triangles" in msg, (rc, msg)
    assert aw.equal_pairs(s.tobytes()) == []  # the helper never lists a triangle
    t["p3"][1] = [1, 0, 0.5]  # not the same triangle: the pair cannot be equal
    rc, msg = _create(s, [(0, 1)], tris=t)
    assert rc == RT_ERR_INVALID_ARGUMENT and "differ in a field" in msg, (rc, msg)
    rc, msg = _create(s, [], tris=t)
    assert _passed_validation(rc, msg), (rc, msg)


def test_an_aliased_csg_leaf_is_refused(rt):
    w = rt.World()
    w.add_object(rt.Csg(rt.Operation.Union, rt.Sphere(), rt.Cube()))
    w.add_object(rt.Sphere())  # the left leaf's twin
    descs = np.frombuffer(w.descs_bytes(), dtype=mesh_ref.SHAPE)
    nodes = np.frombuffer(w.nodes_bytes(), dtype=csg_ref.NODE)
    pairs = aw.equal_pairs(w.descs_bytes())
    assert pairs == [(0, 2)]
    rc, msg = _create(descs, pairs, nodes=nodes, shape_node=w.shape_nodes(), shape_side=w.shape_sides())
    assert rc == RT_ERR_DUPLICATE_SHAPES and "under a Csg" in msg, (rc, msg)
    rc, msg = _create(descs, [], nodes=nodes, shape_node=w.shape_nodes(), shape_side=w.shape_sides())
    assert _passed_validation(rc, msg), (rc, msg)
    with pytest.raises(rt.RtError, match="under a Csg"):  # the mirror's opt-in: the helper, then the same refusal
        w.upload(aliases=True)


def test_the_existing_entry_points_still_refuse(rt):
    two = _spheres(rt, (0.0, 0.0))
    lib = _lib()
    out = ctypes.c_void_p()
    lib.rt_scene_create.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int,
                                    ctypes.POINTER(ctypes.c_void_p)]
    assert lib.rt_scene_create(_ptr(two), 2, None, 0, NO_SUCH_DEVICE, ctypes.byref(out)) == RT_ERR_DUPLICATE_SHAPES
    assert "may be structurally equal" in lib.rt_last_error().decode()


def _best(descs_bytes, runs=5):
    import time
    best, pairs = float("inf"), None
    for _ in range(runs):
        t0 = time.perf_counter()
        pairs = aw.equal_pairs(descs_bytes)
        best = min(best, time.perf_counter() - t0)
    return best, pairs


def _spread_spheres(rt, n, dup):
    d = np.repeat(_desc(rt, rt.Sphere()), n)
    x = np.random.default_rng(5).permutation(n).astype(np.float64) * 3.0
    x[n - dup:] = x[:dup]
    d["transform"][:, 3] = x
    d["inverse"][:, 3] = -x
    return d


def test_the_helper_is_not_quadratic(rt):
    """Spheres spread on x with 200 exact duplicates among them: all found, and eight times the shapes cost far
    less than the 64 times of a scan of every pair (the bound is relative: the best of five runs of each size,
    40 000 against 5 000 shapes, under 24 times; n log n is about 10)."""
    small, _ = _best(_spread_spheres(rt, 5_000, 200).tobytes())
    n = 40_000
    large, pairs = _best(_spread_spheres(rt, n, 200).tobytes())
    print(f"rt_shapes_equal_pairs: 5 000 spheres {small:.4f} s, 40 000 spheres {large:.4f} s")
    assert pairs == sorted((i, n - 200 + i) for i in range(200))
    assert large < 24 * small


def _mesh_descs(n):
    """`n` triangle descs of one mesh: one transform, one material (what an OBJ file's faces are)."""
    s = np.zeros(n, dtype=mesh_ref.SHAPE)
    s["kind"], s["casts_shadow"], s["color"], s["pattern_kind"] = 5, 1, 1.0, -1
    s["transform"] = s["inverse"] = s["pattern_transform"] = s["pattern_inverse"] = np.eye(4).ravel()
    s["ambient"], s["diffuse"], s["specular"], s["shininess"], s["refractive_index"] = 0.1, 0.9, 0.9, 200.0, 1.0
    return s


def test_the_helper_is_not_quadratic_on_a_mesh(rt):
    """The triangles of a mesh share their transform, so a key of the translation alone puts every pair of them
    into one window. The helper never lists a triangle and leaves them out of its sweep: 40 000 faces beside two
    equal spheres cost their sort (a scan of their pairs took 6.7 s at 20 000 faces). Relative bound as above;
    tests/cpp/alias_check.cpp counts the candidate pairs of such a mesh: none."""
    two = np.concatenate([_desc(rt, rt.Sphere()), _desc(rt, rt.Sphere())])
    small, pairs = _best(np.concatenate([_mesh_descs(5_000), two]).tobytes())
    assert pairs == [(5_000, 5_001)]
    large, pairs = _best(np.concatenate([_mesh_descs(40_000), two]).tobytes())
    print(f"rt_shapes_equal_pairs: 5 000 faces {small:.4f} s, 40 000 faces {large:.4f} s")
    assert pairs == [(40_000, 40_001)]
    assert large < 24 * small


# ---- triangles on the opt-in path: two that may be equal are refused, listed or not
def test_equal_triangles_are_refused_though_unlisted():
    s = _mesh_descs(3)
    t = np.zeros(3, dtype=mesh_ref.TRI)
    t["p1"], t["p2"], t["p3"] = [0, 1, 0], [-1, 0, 0], [1, 0, 0]
    t["p1"][1] = [5, 1, 0]  # faces 0 and 2 are the same triangle
    rc, msg = _create(s, [], tris=t)
    assert rc == RT_ERR_DUPLICATE_SHAPES and "shapes 0 and 2" in msg and "triangles" in msg, (rc, msg)
    t["p3"][2] = [1, 0, 0.5]
    rc, msg = _create(s, [], tris=t)
    assert _passed_validation(rc, msg), (rc, msg)


def test_upload_with_aliases_refuses_a_mesh_with_a_repeated_face(rt):
    """The mirror's opt-in (rt_shapes_equal_pairs, then rt_scene_create_aliased): the reference would alias the two
    faces in the containers walk, so the world is refused, as without the opt-in; a duplicated sphere beside the
    mesh does not change that, and without the repeated face the same world passes validation."""
    def world(repeat):
        w = rt.World()
        g = rt.Group()
        g.add_child(rt.Triangle(rt.Point(0, 1, 0), rt.Point(-1, 0, 0), rt.Point(1, 0, 0)))
        g.add_child(rt.Triangle(rt.Point(0, 1, 0), rt.Point(-1, 0, 0), rt.Point(1, 0, 0 if repeat else 2)))
        w.add_object(g)
        w.add_object(rt.glass_sphere())
        w.add_object(rt.glass_sphere())
        return w
    with pytest.raises(rt.RtError, match="aliased triangles are not supported"):
        world(True).upload(aliases=True)
    with pytest.raises(rt.RtError, match="may be structurally equal"):
        world(True).upload()
    if rt.device_count() == 0:
        with pytest.raises(rt.RtError, match="no HIP device"):
            world(False).upload(aliases=True)
    else:
        world(False).upload(aliases=True)


# ---- the opt-in is the world's: upload() without the argument leaves it alone
def _try_upload(rt, w, **kw):
    try:
        w.upload(**kw)
    except rt.RtError as e:
        assert "no HIP device" in str(e) or "structurally equal" in str(e), str(e)


def test_upload_without_the_argument_keeps_the_opt_in(rt):
    w = rt.World()
    w.add_object(rt.Sphere())
    assert not w.aliases
    _try_upload(rt, w)
    assert not w.aliases  # the default stays the refusal
    _try_upload(rt, w, aliases=True)
    assert w.aliases
    _try_upload(rt, w, device=0)
    _try_upload(rt, w)
    assert w.aliases
    _try_upload(rt, w, aliases=False)
    assert not w.aliases


def test_the_scene_parser_always_opts_in(rt):
    """A scene file that places a sphere and a cube twice (the reference's binary renders it): the parser's world is
    opted in, its upload gets past validation, and a plain re-upload keeps the opt-in."""
    p = rt.SceneParser()
    p.load_str(aw.TWICE_YAML)
    w = p.build_world()
    assert w.aliases and aw.equal_pairs(w.descs_bytes()) == [(1, 2), (3, 4)]
    if rt.device_count() == 0:
        with pytest.raises(rt.RtError, match="no HIP device"):
            p.render(5)
        with pytest.raises(rt.RtError, match="no HIP device"):
            w.upload()
    else:
        p.render(5)
        w.upload()
    assert w.aliases
    plain = rt.World()
    for i in range(1, 5):
        plain.add_object(w.child(i))
    with pytest.raises(rt.RtError, match="may be structurally equal"):
        plain.upload()


# ---- the split and the helper under the sanitizers
@pytest.fixture(scope="module")
def alias_check(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("alias")
    exes = []
    for name, flags in (("alias_check", ["-O2"]),
                        ("alias_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(d / name)
        subprocess.run(["g++", "-std=c++17", "-Wall", "-ffp-contract=off", *flags, "-I", CSRC,
                        os.path.join(REPO, "tests", "cpp", "alias_check.cpp"), "-o", exe], check=True)
        exes.append(exe)
    return exes


def test_split_and_helper_under_the_sanitizers(alias_check):
    for exe in alias_check:
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), r.stdout + r.stderr
