"""The tie worlds (tests/tie_worlds.py) hold what they were written for, and
would show a wrong order (CPU only; the GPU holds them in test_gpu_ties.py).

test_inputs_*: per world, from the checker alone (tests/csg_ref.py), over the
authored batch rays and the pixels of the 24x16 frame: the rays of each tie
class (H, T0, C, C3: tie_worlds.classify). The floors are conditions on the
inputs: at least 32 batch rays in every class a world is written for, at least
24 of the 384 pixels of `twins` and `flush` with a tied primary hit, both roles
(so both insertion orders) among the winners, tying objects that differ in
colour and in refractive_index, no equal-t pair inside a Csg node's own list.

test_reversed_order_shows: the checker with every run of equal t turned round
(tie_worlds.Reversed) gives another colour at depth 3 on at least half the rays
of every class, and on at least half the tied pixels of `twins` and `flush`: a
walk that took the wrong one of two tied roots would not pass for right.

The counts (batch rays / pixels, in brackets how many the reversed order
changes), as the checker gave them:

  world            rays  H          T0    C          C3       pixels H
  twins            192   192 (192)  48    80 (80)    -        82 (82)
  flush            192   136 (136)  56    56 (50)    -        106 (106)
  lattice          252   216 (216)  144   [0]        -        0
  lattice_divided  252   216 (216)  144   [0]        -        0
  lattice_twins    252   156 (156)  100   [55 (55)]  -        18
  nested           120   84 (84)    36    36 (36)    36 (36)  80
  lines            144   125 (125)  32    64 (64)    -        40
  mesh             364   201 (134)  [10]  -          -        21
  csg              160   128 (128)  32    [32 (32)]  -        0

(in square brackets: counted, but no class the world is written for; T0 is a
part of H. In a lattice a ray from one cell into the next has the first cell's
exit and the second's entry at one t behind it, but only one of the two is a
container there: no C. `mesh`: 88 of its 201 tied rays tie a cube's face with a
triangle in its plane, the others triangles with each other.)
"""
import numpy as np
import pytest

import csg_ref
import tie_worlds

FLOOR_RAYS, FLOOR_PIXELS = 32, 24
FRAME_WORLDS = ("twins", "flush")  # whose frames must hold tied primary hits
_cache = {}


def _analysed(rt, name):
    """One world's checker, its classes over the batch rays and over the frame's primary rays; once."""
    if name not in _cache:
        tw = tie_worlds.build(rt, name)
        ref = csg_ref.CsgRef.from_world(tw.w)
        pix = tie_worlds.pixel_rays(ref, tw.cam)
        _cache[name] = dict(tw=tw, ref=ref, pix=pix, batch=tie_worlds.classify(ref, tw.rays),
                            frame=tie_worlds.classify(ref, pix))
    return _cache[name]


@pytest.mark.parametrize("name", tie_worlds.WORLDS)
def test_inputs_meet_the_floors(rt, name):
    a = _analysed(rt, name)
    tw, ref, batch, frame = a["tw"], a["ref"], a["batch"], a["frame"]
    counts = {k: int(batch[k].sum()) for k in ("H", "T0", "C", "C3")}
    print(name, len(tw.rays), counts, "pixels H", int(frame["H"].sum()))
    assert (tw.cam.hsize, tw.cam.vsize, tw.depth) == (24, 16, 3) and len(tw.rays) <= 400 and tw.w.n_lights() == 2
    for k in tw.classes:
        assert counts[k] >= FLOOR_RAYS, (name, k, counts)
    if name in FRAME_WORLDS:
        assert frame["H"].sum() >= FLOOR_PIXELS, (name, int(frame["H"].sum()))
    role = tie_worlds.roles(ref)
    for cls in (batch, frame) if name in FRAME_WORLDS else (batch,):
        winners = cls["winner"][cls["H"]]
        assert set(role[winners]) == {0, 1}, name  # both insertion orders win somewhere
    # half the directions are exact unit axis directions, every origin is dyadic (a multiple of 2^-10)
    if name != "mesh":  # (324 of its rays are test_gpu_mesh_edges.py's tie case, from one eye at 1.3, 2.1, -5)
        axis = (np.abs(tw.rays[:, 3:]) == 1.0).sum(axis=1) == 1
        assert axis.sum() >= len(tw.rays) // 3 and (~axis).sum() >= len(tw.rays) // 3
        assert (tw.rays[:, :3] * 1024 == np.round(tw.rays[:, :3] * 1024)).all()
    # tying objects differ in colour and in refractive_index, so the winner shows
    s = ref.s
    pairs = {(i, j) for tied in batch["sharing"] + frame["sharing"] for i in tied for j in tied if i < j}
    assert pairs
    for i, j in pairs:
        assert s["refractive_index"][i] != s["refractive_index"][j] or min(s["kind"][i], s["kind"][j]) >= 5, (i, j)
        assert tuple(s["color"][i]) != tuple(s["color"][j]), (i, j)
    if name in ("twins", "flush", "csg"):  # a shadowless member in each pair
        assert all(s["casts_shadow"][i] != s["casts_shadow"][j] for i, j in pairs if 1 not in (s["kind"][i], s["kind"][j]))
    assert ref.csg_ties == 0
    n_groups = len(tw.w.groups_bytes()) // 56
    if name == "lattice_divided":
        assert n_groups >= 4  # the threshold did split the group
    if name == "flush":  # grouped members against top-level partners
        sg = np.asarray(tw.w.shape_groups())
        assert sum(1 for i, j in pairs if (sg[i] < 0) != (sg[j] < 0)) >= 2
    if name == "csg":
        nodes = np.frombuffer(tw.w.nodes_bytes(), dtype=csg_ref.NODE)
        assert (nodes["kind"] == csg_ref.NODE_CSG).sum() == tie_worlds.N_UNITS
        sn = np.asarray(tw.w.shape_nodes())
        in_unit = np.array([n >= 0 and nodes["kind"][n] == csg_ref.NODE_CSG for n in sn])
        assert all(in_unit[i] != in_unit[j] for i, j in pairs)  # every tie: a unit's root against a solid's
    if name == "twins":
        assert tie_worlds.N_PAIRS >= 48 and tie_worlds.N_SINGLES >= 32 and len(s) == 2 * 48 + 32 + 1
    if name == "mesh":
        mixed = sum(1 for t in batch["sharing"] if len(t) >= 2 and len({bool(s["kind"][i] >= 5) for i in t}) == 2)
        print("mesh: rays that tie a cube with a triangle:", mixed)  # (counted: 88)


@pytest.mark.parametrize("name", tie_worlds.WORLDS)
def test_reversed_order_shows(rt, name):
    a = _analysed(rt, name)
    tw, ref = a["tw"], a["ref"]
    rev = tie_worlds.Reversed.from_world(tw.w)
    for label, rays, cls in (("batch", tw.rays, a["batch"]), ("pixels", a["pix"], a["frame"])):
        if label == "pixels" and name not in FRAME_WORLDS:
            continue
        tied = np.flatnonzero(cls["H"] | cls["C"] | cls["C3"])
        changed = np.zeros(len(rays), dtype=bool)
        changed[tied] = (ref.color_at_batch(rays[tied], tw.depth) != rev.color_at_batch(rays[tied], tw.depth)).any(axis=1)
        for k in ("H", "C", "C3"):
            n, c = int(cls[k].sum()), int((cls[k] & changed).sum())
            print(name, label, k, n, c)
            if k in tw.classes and (label == "batch" or k == "H"):
                assert n > 0 and 2 * c >= n, (name, label, k, n, c)
