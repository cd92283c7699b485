"""The checker for triangles under a Csg (tests/csg_tri_ref.py) pinned (CPU only).

Pin 1: where the old checker (tests/csg_ref.py, itself pinned by tests/test_csg_ref.py) accepts the
world it is the old checker: rtamd.scenes.csg_random seeds 0-15 (24x16) and csg_dice(4) at 32x18,
hit records, frames and counters bit for bit.
Pin 2: a world with answers worked by hand (csg_mesh_worlds.known_answer): a slab of two triangles
and a sphere between them under each operation, a ray from outside and one from inside.
Pin 3: the union of two disjoint closed meshes under identity Csg transforms is the same two meshes
as plain top-level groups under the old checker: hit records and frame.
csg_ties is asserted 0 on every world."""
import numpy as np
import pytest

import csg_mesh_worlds as worlds
import csg_ref
import csg_tri_ref

COUNTS = csg_ref.COUNTERS


def _pixel_rays(ref, cam):
    c = np.frombuffer(cam.desc_bytes(), dtype=csg_ref.CAMERA)[0]
    return np.array([list(o) + list(d) for y in range(int(c["vsize"])) for x in range(int(c["hsize"]))
                     for o, d in [ref.ray_for_pixel(c, x, y)]])


def _same_as_old(w, cam, depth):
    old, new = csg_ref.CsgRef.from_world(w), csg_tri_ref.CsgTriRef.from_world(w)
    img_old, st_old = old.render(cam.desc_bytes(), depth)
    img_new, st_new = new.render(cam.desc_bytes(), depth)
    assert img_new.tobytes() == img_old.tobytes()
    assert st_new == st_old and st_old["rays_shadow"] > 100
    rays = _pixel_rays(old, cam)[::3]
    assert new.hit_batch(rays).tobytes() == old.hit_batch(rays).tobytes()
    assert old.csg_ties == 0 and new.csg_ties == 0


@pytest.mark.parametrize("seed", range(16))
def test_equals_the_old_checker_on_csg_random(rt, seed):
    from rtamd import scenes
    _same_as_old(*scenes.csg_random(seed))


def test_equals_the_old_checker_on_four_dice(rt):
    from rtamd import scenes
    _same_as_old(*scenes.csg_dice(4, 32, 18))


@pytest.mark.parametrize("op", sorted(worlds.KNOWN_T))
def test_known_answers(rt, op):
    w = worlds.known_answer(rt, op)
    ref = csg_tri_ref.CsgTriRef.from_world(w)
    assert list(ref.s["kind"]) == [5, 5, 0]
    xs = ref.intersect(worlds.KNOWN_RAY[:3], worlds.KNOWN_RAY[3:])
    assert [x[0] for x in xs] == pytest.approx(worlds.KNOWN_T[op], abs=1e-9)
    tri_ts = [x[0] for x in xs if x[1] < 2]
    assert all(t in (5.0, 7.0) for t in tri_ts)  # the triangles' roots are exact
    rec = ref.hit_record(worlds.KNOWN_RAY[:3], worlds.KNOWN_RAY[3:])
    assert rec[0] == (2 if op == "Intersection" else 0) and rec[1] == pytest.approx(worlds.KNOWN_T[op][0], abs=1e-9)
    assert (rec[21], rec[22]) == (1.0, 1.5 if op == "Intersection" else 1.1)
    # from inside the sphere, between the triangles
    obj, t, n1, n2 = worlds.KNOWN_INSIDE_HIT[op]
    rec = ref.hit_record(worlds.KNOWN_INSIDE[:3], worlds.KNOWN_INSIDE[3:])
    assert rec[0] == obj and rec[1] == pytest.approx(t, abs=1e-9) and (rec[21], rec[22]) == (n1, n2)
    assert ref.csg_ties == 0
    # the reference's counts: every ray tests the two triangles and the sphere (the Csg's box is met)
    assert ref.counts["other_tests"] == 2 * 3 and ref.counts["sphere_tests"] == 3 and ref.counts["sphere_disc_ge0"] == 3


def _two_meshes(rt, as_union):
    a = worlds.tetrahedron(rt, (-1.3, 0.2, 0.1), 0.8, worlds.material(rt, (0.9, 0.4, 0.2), 1.3))
    b = worlds.tetrahedron(rt, (1.2, -0.1, 0.4), 0.7, worlds.material(rt, (0.2, 0.5, 0.9), reflective=0.3), smooth=True)
    w = rt.World()
    floor = rt.Plane()
    floor.set_transform(rt.translation(0, -1.4, 0))
    w.add_object(floor)
    if as_union:
        w.add_object(rt.Csg(rt.Operation.Union, a, b))
    else:
        w.add_object(a)
        w.add_object(b)
    worlds.lights(rt, w)
    return w


def test_union_of_disjoint_meshes_is_the_plain_groups(rt):
    cam = worlds.camera(rt, (0.4, 1.7, -5.2), (0.1, 0.05, 0.2))
    union, plain = _two_meshes(rt, True), _two_meshes(rt, False)
    assert union.descs_bytes() == plain.descs_bytes()  # the same shapes in the same order
    new, old = csg_tri_ref.CsgTriRef.from_world(union), csg_ref.CsgRef.from_world(plain)
    rays = np.vstack([_pixel_rays(old, cam)[::2], worlds.random_rays(((-2.2, -0.8, -0.8), (2.0, 1.1, 1.2)), 128, 3)])
    assert (rays != 0.0).all()  # an identity transform turns -0.0 into +0.0
    got, want = new.hit_batch(rays), old.hit_batch(rays)
    assert got.tobytes() == want.tobytes()
    on_mesh = want[:, 0] >= 1
    assert on_mesh.sum() > 60 and len(set(want[on_mesh, 0])) >= 6 and (want[on_mesh, 17] == 1.0).sum() > 5
    img_new, st_new = new.render(cam.desc_bytes(), worlds.DEPTH)
    img_old, st_old = old.render(cam.desc_bytes(), worlds.DEPTH)
    assert img_new.tobytes() == img_old.tobytes() and img_old.sum() > 0
    for k in ("rays_primary", "rays_reflect", "rays_refract", "rays_shadow"):
        assert st_new[k] == st_old[k]
    assert st_old["rays_refract"] > 10 and new.csg_ties == 0
