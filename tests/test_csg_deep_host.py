"""Host side of the deep Csg units (rt_scene_create_ex with RT_SCENE_DEEP_CSG; CPU only, nothing here reaches a device).

Without the flag the three caps keep their refusals word for word, through rt_scene_create_ex with flags 0 and
through every older entry point that can express the world; with it the same three worlds pass validation (every
call names a device ordinal no machine has, tests/test_alias_host.py: a call that passes validation ends with "no HIP
device" or "bad device ordinal", before any upload). What the flag does not lift stays refused with it. The mirror's
opt-in (World.upload(deep_csg=...)) is sticky. tests/cpp/csg_deep_check.cpp drives the deep evaluator's stream
functions against a literally nested evaluation under the address and undefined-behaviour sanitizers.
"""
import ctypes
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
RT_ERR_INVALID_ARGUMENT, RT_ERR_UNSUPPORTED_SHAPE, RT_ERR_DUPLICATE_SHAPES = -1, -2, -5
RT_SCENE_ALIASED, RT_SCENE_DEEP_CSG = 1, 2
NO_SUCH_DEVICE = 1 << 20
MAX_LEAVES, MAX_DEPTH, MAX_NODES = 16, 4, 32  # RT_CSG_MAX_* (include/rt_render.h)
P, S, I, U = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint32


def _lib():
    lib = aw.librtamd()
    lib.rt_scene_create_ex.argtypes = [P, S, P, P, P, S, P, S, P, S, P, S, U, I, ctypes.POINTER(P)]
    lib.rt_scene_create_aliased.argtypes = [P, S, P, P, P, S, P, S, P, S, P, S, I, ctypes.POINTER(P)]
    lib.rt_scene_create_tree.argtypes = [P, S, P, P, P, S, P, S, P, S, I, ctypes.POINTER(P)]
    return lib


def _ptr(a):
    return None if a is None or len(a) == 0 else a.ctypes.data_as(ctypes.c_void_p)


class _Flat:
    """A world's flattened arrays, as the mirror hands them to rt_scene_create_*."""

    def __init__(self, w):
        self.descs = np.frombuffer(w.descs_bytes(), dtype=mesh_ref.SHAPE)
        self.nodes = np.frombuffer(w.nodes_bytes(), dtype=csg_ref.NODE)
        self.sn = np.ascontiguousarray(w.shape_nodes(), dtype=np.int32)
        self.ss = np.ascontiguousarray(w.shape_sides(), dtype=np.int32)
        self.tris = np.frombuffer(w.triangles_bytes(), dtype=mesh_ref.TRI)


def _create(f, flags, pairs=None, call="ex"):
    lib = _lib()
    out = ctypes.c_void_p()
    head = (_ptr(f.descs), len(f.descs), _ptr(f.sn), _ptr(f.ss), _ptr(f.nodes), len(f.nodes), _ptr(f.tris), len(f.tris), None, 0)
    pairs = None if pairs is None else np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    n_pairs = 0 if pairs is None else len(pairs)
    if call == "ex":
        rc = lib.rt_scene_create_ex(*head, _ptr(pairs), n_pairs, flags, NO_SUCH_DEVICE, ctypes.byref(out))
    elif call == "aliased":
        rc = lib.rt_scene_create_aliased(*head, _ptr(pairs), n_pairs, NO_SUCH_DEVICE, ctypes.byref(out))
    else:
        rc = lib.rt_scene_create_tree(*head, NO_SUCH_DEVICE, ctypes.byref(out))
    assert not out.value
    return rc, lib.rt_last_error().decode()


def _passed_validation(rc, msg):
    return rc in (-1, -8) and ("bad device ordinal" in msg or "no HIP device" in msg)


# ---- the smallest worlds beyond one cap each
def grouped(rt, n):
    """tests/test_gpu_csg.py's: a union of two groups of spheres, n leaves on one level."""
    halves = []
    for lo, hi in ((0, n // 2), (n // 2, n)):
        g = rt.Group()
        for k in range(lo, hi):
            s = rt.Sphere()
            s.set_transform(rt.translation(0.25 * k, 0.0, 0.0) * rt.scaling(0.3, 0.3, 0.3))
            g.add_child(s)
        halves.append(g)
    return rt.Csg(rt.Operation.Union, halves[0], halves[1])


def nest(rt, levels):
    from test_gpu_csg import _nest
    return _nest(rt, levels)


def mesh_under(rt, n_nodes):
    """A tetrahedron (a group of four triangles) under a left chain of n_nodes unions with small spheres."""
    p = [rt.Point(1, 1, 1), rt.Point(1, -1, -1), rt.Point(-1, 1, -1), rt.Point(-1, -1, 1)]
    g = rt.Group()
    for a, b, c in ((0, 1, 2), (0, 3, 1), (0, 2, 3), (1, 3, 2)):
        g.add_child(rt.Triangle(p[a], p[b], p[c]))
    node = g
    for k in range(n_nodes):
        s = rt.Sphere()
        s.set_transform(rt.translation(0.9 * np.cos(0.7 * k), 0.9 * np.sin(0.7 * k), 0.03 * k) * rt.scaling(0.3, 0.3, 0.3))
        node = rt.Csg(rt.Operation.Union, node, s)
    return node


BEYOND = {
    "leaves": (lambda rt: grouped(rt, MAX_LEAVES + 1), "more than RT_CSG_MAX_LEAVES = 16 primitives under one Csg "
               "(Sphere, Plane, Cube, Cylinder, Cone; triangles are not counted)"),
    "depth": (lambda rt: nest(rt, MAX_DEPTH + 1), "more than RT_CSG_MAX_DEPTH = 4 nested Csg nodes"),
}


def _world(rt, shape):
    w = rt.World()
    w.add_object(shape)
    return w


def nodes_world(rt):
    """A mesh under 33 Csg nodes within the other two caps: groups between Csg nodes are free, so the outermost Csg's
    two sides are groups of 16 Csgs each, every one the union or difference of two small sheets of two triangles
    (one of them cut by a sphere instead). 33 nodes, 2 levels, 1 leaf of kinds 0-4, 126 triangles."""
    def sheet(k, dz):
        x, y = 0.45 * (k % 8) - 1.6, 0.5 * (k // 8) - 0.9
        a, b = rt.Point(x, y, dz + 0.01 * k), rt.Point(x + 0.4, y + 0.02, dz + 0.02 * k)
        c, d = rt.Point(x + 0.03, y + 0.42, dz - 0.01 * k), rt.Point(x + 0.41, y + 0.4, dz + 0.03)
        g = rt.Group()
        g.add_child(rt.Triangle(a, b, c))
        g.add_child(rt.Triangle(b, d, c))
        return g
    sides = []
    for s in range(2):
        g = rt.Group()
        for k in range(16 * s, 16 * s + 16):
            right = sheet(k, 0.3)
            if k == 5:
                right = rt.Sphere()
                right.set_transform(rt.translation(0.45 * 5 - 1.4, -0.7, 0.0) * rt.scaling(0.15, 0.15, 0.15))
            g.add_child(rt.Csg(rt.Operation.Difference if k % 3 == 0 else rt.Operation.Union, sheet(k, 0.0), right))
        sides.append(g)
    return _world(rt, rt.Csg(rt.Operation.Union, sides[0], sides[1]))


def test_the_three_refusals_keep_their_words(rt):
    for name, (make, words) in BEYOND.items():
        f = _Flat(_world(rt, make(rt)))
        for call, pairs in (("ex", None), ("tree", None), ("aliased", [])):
            rc, msg = _create(f, 0, pairs, call)
            assert rc == RT_ERR_UNSUPPORTED_SHAPE and msg.endswith(words) and msg.startswith("node "), (name, call, rc, msg)
        rc, msg = _create(f, RT_SCENE_ALIASED, [])  # the other flag lifts nothing
        assert rc == RT_ERR_UNSUPPORTED_SHAPE and msg.endswith(words), (name, rc, msg)
    # the third cap: leaves beyond 16 come first in a world of kinds 0-4, so this one is held by a mesh with few spheres
    f = _Flat(_world(rt, mesh_under(rt, MAX_DEPTH)))  # (within every cap: 4 nodes, 4 levels, 4 leaves of kinds 0-4)
    assert _passed_validation(*_create(f, 0))
    # the older calls that cannot express a Csg refuse none of this: they never see one (groups only)
    lib = _lib()
    lib.rt_scene_create.argtypes = [P, S, P, S, I, ctypes.POINTER(P)]
    out = ctypes.c_void_p()
    one = np.frombuffer(_world(rt, rt.Sphere()).descs_bytes(), dtype=mesh_ref.SHAPE)
    rc = lib.rt_scene_create(_ptr(one), 1, None, 0, NO_SUCH_DEVICE, ctypes.byref(out))
    assert _passed_validation(rc, lib.rt_last_error().decode())


def test_the_node_cap_keeps_its_words(rt):
    w = nodes_world(rt)
    f = _Flat(w)
    assert (f.nodes["kind"] == csg_ref.NODE_CSG).sum() == MAX_NODES + 1
    words = "more than RT_CSG_MAX_NODES = 32 Csg nodes in one Csg with triangles below it"
    for call, pairs in (("ex", None), ("tree", None), ("aliased", [])):
        rc, msg = _create(f, 0, pairs, call)
        assert rc == RT_ERR_UNSUPPORTED_SHAPE and msg.endswith(words), (call, rc, msg)
    assert _passed_validation(*_create(f, RT_SCENE_DEEP_CSG))
    with pytest.raises(rt.RtError, match="RT_CSG_MAX_NODES"):
        w.upload()


def test_with_the_flag_the_same_worlds_pass_validation(rt):
    for name, (make, _) in BEYOND.items():
        f = _Flat(_world(rt, make(rt)))
        for flags, pairs in ((RT_SCENE_DEEP_CSG, None), (RT_SCENE_DEEP_CSG | RT_SCENE_ALIASED, [])):
            rc, msg = _create(f, flags, pairs)
            assert _passed_validation(rc, msg), (name, flags, rc, msg)
    f = _Flat(_world(rt, mesh_under(rt, MAX_NODES + 1)))  # 33 nodes and levels over a mesh
    rc, msg = _create(f, 0)
    assert rc == RT_ERR_UNSUPPORTED_SHAPE and "RT_CSG_MAX_DEPTH" in msg
    assert _passed_validation(*_create(f, RT_SCENE_DEEP_CSG))


def test_what_the_flag_does_not_lift_stays_refused(rt):
    # a lone triangle as a Csg's own child
    w = _world(rt, rt.Csg(rt.Operation.Union, rt.Triangle(rt.Point(0, 1, 0), rt.Point(-1, 0, 0), rt.Point(1, 0, 0)), rt.Sphere()))
    rc, msg = _create(_Flat(w), RT_SCENE_DEEP_CSG)
    assert rc == RT_ERR_UNSUPPORTED_SHAPE and "a Triangle under a Csg as its own left or right child is not supported" in msg
    # an unknown bit
    f = _Flat(_world(rt, rt.Sphere()))
    for flags in (4, 8 | RT_SCENE_DEEP_CSG, 1 << 31):
        rc, msg = _create(f, flags)
        assert rc == RT_ERR_INVALID_ARGUMENT and "unknown flag" in msg, (flags, rc, msg)
    # pairs without RT_SCENE_ALIASED
    two = _world(rt, rt.Sphere())
    two.add_object(rt.Sphere())
    for flags in (0, RT_SCENE_DEEP_CSG):
        rc, msg = _create(_Flat(two), flags, [(0, 1)])
        assert rc == RT_ERR_INVALID_ARGUMENT and "without RT_SCENE_ALIASED" in msg, (flags, rc, msg)
    # duplicates without RT_SCENE_ALIASED
    rc, msg = _create(_Flat(two), RT_SCENE_DEEP_CSG)
    assert rc == RT_ERR_DUPLICATE_SHAPES and "may be structurally equal" in msg
    assert _passed_validation(*_create(_Flat(two), RT_SCENE_DEEP_CSG | RT_SCENE_ALIASED, [(0, 1)]))
    # an aliased leaf under a (deep) Csg, both flags set
    w = _world(rt, nest(rt, MAX_DEPTH + 1))
    twin = rt.Sphere()
    twin.set_transform(rt.translation(0.0, 0.0, 0.0) * rt.scaling(1.2, 1.2, 1.2))
    twin.material.color = rt.Color(0.9, 0.5, 0.1)
    w.add_object(twin)  # the chain's first leaf again
    pairs = aw.equal_pairs(w.descs_bytes())
    assert pairs == [(0, MAX_DEPTH + 2)]
    rc, msg = _create(_Flat(w), RT_SCENE_DEEP_CSG | RT_SCENE_ALIASED, pairs)
    assert rc == RT_ERR_DUPLICATE_SHAPES and "an aliased primitive under a Csg is not supported" in msg, (rc, msg)
    # flags 0 is rt_scene_create_tree: a plain world passes
    assert _passed_validation(*_create(f, 0))


def test_the_mirror_opt_in_is_sticky(rt):
    w = _world(rt, nest(rt, MAX_DEPTH + 1))
    assert not w.deep_csg
    with pytest.raises(rt.RtError, match="RT_CSG_MAX_DEPTH"):
        w.upload()
    assert not w.deep_csg

    def reaches_the_device(**kw):
        if rt.device_count() == 0:
            with pytest.raises(rt.RtError, match="no HIP device"):
                w.upload(**kw)
        else:
            w.upload(**kw)
    reaches_the_device(deep_csg=True)
    assert w.deep_csg
    reaches_the_device()  # None leaves it as it is
    reaches_the_device(device=0, aliases=False)
    assert w.deep_csg and not w.aliases
    with pytest.raises(rt.RtError, match="RT_CSG_MAX_DEPTH"):
        w.upload(deep_csg=False)
    assert not w.deep_csg
    with pytest.raises(rt.RtError, match="RT_CSG_MAX_DEPTH"):
        w.upload()


def test_the_knob_exists(rt):
    rt._rtamd._tuning_set("csg_deep_all", 1)
    rt._rtamd._tuning_set("csg_deep_all", 0)
    with pytest.raises(rt.RtError):
        rt._rtamd._tuning_set("csg_deep_all", 2)


# ---- the deep evaluator's stream functions under the sanitizers
@pytest.fixture(scope="module")
def deep_check(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("csg_deep") / "csg_deep_check_san")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(REPO, "tests", "cpp", "csg_deep_check.cpp"), "-o", exe], check=True)
    return exe


def test_deep_stream_equals_nested(deep_check):
    r = subprocess.run([deep_check], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
    fields = {k: int(v) for k, v in (f.split("=") for f in r.stdout.split()[1:])}
    assert fields["cases"] >= 1000
    assert fields["multi_batch"] * 5 >= fields["cases"]  # more roots than one batch of 64 holds
    assert fields["three_odd"] * 5 >= fields["cases"]  # three or more odd leaves behind the origin: the top-2 rule chooses
    assert fields["max_roots"] > 192 and fields["levels40"] > 0 and fields["leaves150"] > 0
