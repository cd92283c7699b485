"""Host side of Csg (CPU only): the host mirror (host/rt_world.hpp Csg: bounds,
divide, the default set_transform / set_material through a Group, the flattening
into rt_node_desc) against the reference's KATs and rules (csg.rs, group.rs,
geometry/mod.rs), and tests/cpp/csg_check.cpp, a stand-alone program that drives
the kernels' filter header rt_csg.hpp against a literal restatement."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import csg_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "raytracer-challenge-rs_amd", "csrc")


def test_csg_bounding_box_contains_its_children(rt):  # csg.rs:278-302
    right = rt.Sphere()
    right.set_transform(rt.translation(2, 3, 4))
    c = rt.Csg(rt.Operation.Difference, rt.Sphere(), right)
    assert c.operation == rt.Operation.Difference
    assert c.left.kind == 0 and c.right.transform == rt.translation(2, 3, 4)
    b = c.get_bounds()
    assert b.min == rt.Point(-1, -1, -1) and b.max == rt.Point(3, 4, 5)


def test_subdividing_a_csg_subdivides_its_children(rt):  # csg.rs:304-358
    def pair(a, b):
        g = rt.Group()
        for t in (a, b):
            s = rt.Sphere()
            s.set_transform(rt.translation(*t))
            g.add_child(s)
        return g
    shape = rt.Csg(rt.Operation.Difference, pair((-1.5, 0, 0), (1.5, 0, 0)), pair((0, 0, -1.5), (0, 0, 1.5)))
    shape.divide(1)
    left, right = shape.left, shape.right
    assert left.n_children() == 2 and right.n_children() == 2
    assert left.child(0).child(0).transform == rt.translation(-1.5, 0, 0)
    assert left.child(1).child(0).transform == rt.translation(1.5, 0, 0)
    assert right.child(0).child(0).transform == rt.translation(0, 0, -1.5)
    assert right.child(1).child(0).transform == rt.translation(0, 0, 1.5)


def test_csg_in_a_transformed_group(rt):
    """add_child / Group::set_transform call the Csg's default set_transform with the product
    (group.rs:71-94,128-133): its own transform changes, its leaves keep theirs; Group::set_material
    reaches only the Csg's own material (geometry/mod.rs:66-68)."""
    leaf = rt.Cube()
    leaf.set_transform(rt.translation(0, 1, 0))
    leaf.material.color = rt.Color(0.1, 0.2, 0.3)
    c = rt.Csg(rt.Operation.Union, leaf, rt.Sphere())
    c.set_transform(rt.scaling(2, 2, 2))
    g = rt.Group()
    g.set_transform(rt.translation(5, 0, 0))
    g.add_child(c)
    inside = g.child(0)
    assert inside.transform == rt.translation(5, 0, 0) * rt.scaling(2, 2, 2)
    assert inside.left.transform == rt.translation(0, 1, 0) and inside.right.transform == rt.Sphere().transform
    g.set_transform(rt.translation(0, 0, 7))
    inside = g.child(0)
    assert inside.transform == rt.translation(0, 0, 7) * rt.scaling(2, 2, 2)
    assert inside.left.transform == rt.translation(0, 1, 0)
    m = rt.Material()
    m.color = rt.Color(1, 0, 0)
    g.set_material(m)
    inside = g.child(0)
    assert inside.material.color == rt.Color(1, 0, 0)
    assert inside.left.material.color == rt.Color(0.1, 0.2, 0.3) and inside.right.material.color == rt.Color(1, 1, 1)
    # the box follows the default set_transform (geometry/mod.rs:74-85): the children's union, moved
    b = inside.get_bounds()
    assert abs(b.min.z - (7 - 2)) < 1e-9 and abs(b.max.y - 4) < 1e-9


def test_flattening_order_and_bytes(rt):
    """Depth first, a Csg's left before its right; nodes parents first, with side, operation,
    box and the Csg's own inverse."""
    w = rt.World()
    w.add_object(rt.Plane())
    a, b, c = rt.Sphere(), rt.Cube(), rt.Cylinder(-1, 1, True)
    a.material.ambient, b.material.ambient, c.material.ambient = 0.11, 0.22, 0.33
    inner = rt.Csg(rt.Operation.Intersection, b, c)
    outer = rt.Csg(rt.Operation.Difference, inner, a)
    outer.set_transform(rt.translation(1, 2, 3))
    g = rt.Group()
    g.add_child(outer)
    tail = rt.Cone(-1, 0, True)
    g.add_child(tail)
    w.add_object(g)
    shapes = np.frombuffer(w.descs_bytes(), dtype=csg_ref.SHAPE)
    nodes = np.frombuffer(w.nodes_bytes(), dtype=csg_ref.NODE)
    assert list(shapes["kind"]) == [1, 2, 3, 0, 4]
    assert [round(float(x), 2) for x in shapes["ambient"][1:4]] == [0.22, 0.33, 0.11]
    assert list(nodes["kind"]) == [0, 1, 1] and list(nodes["parent"]) == [-1, 0, 1]
    assert list(nodes["operation"][1:]) == [csg_ref.DIFFERENCE, csg_ref.INTERSECTION]
    assert list(nodes["side"][1:]) == [0, 0]
    assert w.shape_nodes() == [-1, 2, 2, 1, 0] and w.shape_sides()[1:4] == [0, 1, 1]
    inv = nodes["inverse"][1].reshape(4, 4)
    assert np.array_equal(inv[:3, 3], [-1, -2, -3]) and np.array_equal(inv[:3, :3], np.eye(3))
    assert np.array_equal(nodes["inverse"][2].reshape(4, 4), np.eye(4))
    assert list(nodes["min"][1]) == [0, 1, 2] and list(nodes["max"][1]) == [2, 3, 4]  # the outer Csg's box, moved
    assert list(nodes["min"][2]) == [-1, -1, -1] and list(nodes["max"][2]) == [1, 1, 1]
    with pytest.raises(ValueError, match="is a Group"):
        w.object(1)
    w.add_object(inner)
    with pytest.raises(ValueError, match="is a Csg"):
        w.object(2)
    assert w.child(2).operation == rt.Operation.Intersection and w.object(0).kind == 1
    # a world without a Csg keeps the rt_group_desc arrays
    w2 = rt.World()
    g2 = rt.Group()
    g2.add_child(rt.Sphere())
    w2.add_object(g2)
    assert w2.nodes_bytes() == b"" and len(w2.groups_bytes()) == 56 and w2.shape_groups() == [0]


@pytest.fixture(scope="module")
def csg_check(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("csg")
    exes = []
    for name, flags in (("csg_check", ["-O2"]),
                        ("csg_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(d / name)
        subprocess.run(["g++", "-std=c++17", "-Wall", *flags, "-I", CSRC,
                        os.path.join(REPO, "tests", "cpp", "csg_check.cpp"), "-o", exe], check=True)
        exes.append(exe)
    return exes


def test_csg_filter_header(csg_check):
    for exe in csg_check:  # the plain build, then the same program under the address and undefined sanitizers
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
