"""Roots that tie bit for bit, on the GPU: every walk takes the one that comes
first in the reference's traversal order.

The reference sorts World::intersect's list stably, so of two roots with a
bit-equal t the first in world order (a group's children in order, also after
divide; t1 before t2 of one object) is the hit, and `containers` meets them in
that order: it decides which material is shaded and what n1 and n2 are. The GPU
never builds the list: better(t, key) and push_container order by (t, key) with
key = (object << kKeyShift) | list position, in every leaf test of every walk.

The worlds are those of tests/tie_worlds.py (what ties in each, how many rays,
and that a reversed order would show: tests/test_tie_worlds.py, without a GPU).
Each runs through the knob rows and modes of tests/test_gpu_variants.py (its
_variants table and its _Sweep's plan and variant checks, not a copy): the fast
camera render, the counted fast render, render_multithreaded X4 and
color_at_batch on the authored rays at depths 0 and 3 equal the exhaustive call
bit for bit under every variant, with the plan readout the variant was written
for. Once per world the exhaustive frame, its counters and the exhaustive
color_at_batch at depths 0 and 3 equal the C oracle's (the checker's of
tests/csg_ref.py for `mesh` and `csg`, which the oracle refuses), hit_batch
equals the checker over all 24 doubles (the winner, n1, n2) and
is_shadowed_batch equals it from every authored origin to both lights. No
tolerance anywhere.

Which walk each world is for, asserted from _wf_profile / _wf_plan / _csg_plan:
  twins            128 diagonal spheres: the wave traversal and every LDS and global sphere image
  flush            14 solids outside every hierarchy (the every-record loop of the fused kernels), grouped members
  lattice (x3)     18 boxed solids: the other records' hierarchy; a divided group; general-transform spheres
  nested           18 boxed solids: the other records' hierarchy, three roots at one t
  lines            20 open tubes and cones: the lines' hierarchy
  mesh             64 triangles: the triangles' hierarchy (TRIS kernels)
  csg              16 units: the units' hierarchy (CSG kernels)
"""
import numpy as np
import pytest

import csg_ref
import tie_worlds
from test_gpu_variants import COUNTERS, NTHREADS, _Sweep, _prof, _quads, _restore, _tris_csg, _tune, _variants

pytestmark = pytest.mark.gpu


class _TieSweep(_Sweep):
    """One tie world through test_gpu_variants._Sweep's variants and modes, with the authored rays."""

    def __init__(self, rt, oracle, name):
        self.rt, self.name = rt, name
        self.failures, self.reached = [], set()
        tw = tie_worlds.build(rt, name)
        self.tw, self.w, self.cam, self.depth, self.rays = tw, tw.w, tw.cam, tw.depth, tw.rays
        w, cam, depth, rays = self.w, self.cam, self.depth, self.rays
        exh, self.st = cam.render(w, depth)
        self.frame = exh.to_numpy()
        self.prof = _prof(rt, w)
        self.tris, self.csg = _tris_csg(w)
        self.tri_plan = rt._rtamd._wf_plan(w)["triangles"]
        self.quads = _quads(self.prof) or self.tris
        self.batch0 = w.color_at_batch(rays, 0, True, True)
        self.batch = w.color_at_batch(rays, depth, True, True)
        # the yardsticks, once: the oracle where it takes the world, the checker for the hit records and shadows
        checker = csg_ref.CsgRef.from_world(w)
        if name in tie_worlds.ORACLE_WORLDS:
            ow = oracle.OracleWorld.from_world(w)
            ref, rst = ow.render(cam.desc_bytes(), depth, nthreads=NTHREADS)
            want = [ow.color_at_batch(rays, d) for d in (0, depth)]
        else:
            ref, rst = checker.render(cam.desc_bytes(), depth)
            want = []
            for d in (0, depth):
                checker.counts = dict.fromkeys(csg_ref.COUNTERS, 0)
                want.append((checker.color_at_batch(rays, d), dict(checker.counts)))
        self.check(self.frame.tobytes() == ref.tobytes(), f"exhaustive frame != yardstick in {int((self.frame != ref).sum())} channels")
        for k in COUNTERS:
            self.check(self.st[k] == rst[k], f"frame counter {k}: {self.st[k]} != {rst[k]}")
        for d, got, (col, cst) in ((0, self.batch0, want[0]), (depth, self.batch, want[1])):
            bad = int((np.asarray(got[0]) != col).any(axis=1).sum())
            self.check(bad == 0, f"exhaustive batch depth {d} != yardstick on {bad} rays")
            for k in COUNTERS:
                self.check(got[1][k] == cst[k], f"batch depth {d} counter {k}: {got[1][k]} != {cst[k]}")
        rec, rec_want = np.ascontiguousarray(w.hit_batch(rays)), np.ascontiguousarray(checker.hit_batch(rays))
        bad = np.flatnonzero((rec.view(np.uint64) != rec_want.view(np.uint64)).any(axis=1))
        self.check(len(bad) == 0, f"hit_batch != checker on {len(bad)} rays, first {bad[:1]}: "
                   f"{rec[bad[:1], [0, 1, 21, 22]] if len(bad) else ''} for {rec_want[bad[:1], [0, 1, 21, 22]] if len(bad) else ''}")
        pts = np.ascontiguousarray(rays[:, :3])
        for light in range(w.n_lights()):
            got = np.asarray(w.is_shadowed_batch(pts, light)).astype(bool)
            sh = np.array([checker.is_shadowed(p, light) for p in pts])
            self.check((got == sh).all(), f"is_shadowed_batch light {light}: {int((got != sh).sum())} differ")
        self.shadowed = int(sh.sum())
        self.check(checker.csg_ties == 0, f"{checker.csg_ties} equal-t pairs in a Csg node's list")
        self.aa_cam = tie_worlds.build(rt, name).cam
        self.aa_cam.render_opts.aa_samples(rt.AASamples.X4)
        self.frame4 = self.aa_cam.render_multithreaded(w, depth)[0].to_numpy().tobytes()
        self.frame = self.frame.tobytes()
        self.fused = self.prof["n_bvh_nodes"] > 0 or self.prof["n_obvh_nodes"] > 0 or self.prof["n_lbvh_nodes"] > 0 or \
            self.tri_plan["nodes"] > 0
        self.csg_ran = True
        for vname, knobs, lane, n_top, deltas in _variants():
            try:
                _tune(w, knobs)
                self.variant(vname, knobs, lane, n_top, deltas)
                if self.csg:
                    self.csg_ran = self.csg_ran and rt._rtamd._csg_plan(w)["ran"]
            finally:
                _restore(w, knobs)
        w.check()


@pytest.fixture(scope="module")
def sweep(rt, oracle):
    done = {}

    def run(name):
        if name not in done:
            done[name] = _TieSweep(rt, oracle, name)
        return done[name]
    return run


# What the profile must show of each world beside the walk it was written for (asserted below).
PROFILE = {
    "twins": dict(n_diag=128, n_gen=0, n_quads=0, n_obvh_nodes=0, n_lbvh_nodes=0),
    "flush": dict(n_diag=2, n_gen=0, n_obvh_nodes=0, n_lbvh_nodes=0, n_other_culled=0, n_line_culled=0),
    "lattice": dict(n_diag=2, n_gen=0, n_other_culled=18, n_lbvh_nodes=0),
    "lattice_divided": dict(n_diag=2, n_gen=0, n_other_culled=18, n_lbvh_nodes=0),
    "lattice_twins": dict(n_diag=2, n_gen=8, n_other_culled=22, n_lbvh_nodes=0),
    "nested": dict(n_diag=2, n_gen=0, n_other_culled=18, n_lbvh_nodes=0),
    "lines": dict(n_diag=2, n_gen=0, n_line_culled=20, n_obvh_nodes=0),
    "mesh": dict(n_diag=2, n_gen=0, n_obvh_nodes=0, n_lbvh_nodes=0),
    "csg": dict(n_diag=2),
}


@pytest.mark.parametrize("name", tie_worlds.WORLDS)
def test_tie_world_bitwise(rt, sweep, name):
    """Every variant x mode of one tie world equals the exhaustive call, and the exhaustive call the
    yardstick, bit for bit; the walk the world was written for ran."""
    s = sweep(name)
    assert not s.failures, "\n".join(s.failures)
    for k, v in dict(PROFILE[name], n_planes=1, n_lights=2).items():
        assert s.prof[k] == v, (name, k, s.prof[k])
    assert s.fused and s.prof["n_bvh_nodes"] > 0
    assert (s.cam.hsize, s.cam.vsize, s.depth) == (24, 16, 3) and len(s.rays) <= 400
    assert s.st["rays_reflect"] > 20 and s.st["rays_refract"] > 20 and s.shadowed > 0
    # every image of the sphere walks ran on this world: the wave traversal (0), the four-wide and pair LDS
    # images (15, 14), the global walks with a treelet (4, 3) and the scratch stack (1), plain and counted
    lanes = {(t[0], t[2]) for t in s.reached}
    assert lanes == {(lane, tally) for lane in (0, 15, 14, 4, 3, 1) for tally in (False, True)}, sorted(lanes)
    assert {(t[1], t[4], t[5]) for t in s.reached} == {(s.quads, s.tris, s.csg)}
    if name == "twins":
        assert not s.quads  # spheres only: every tie is decided inside the sphere walks
    elif name == "flush":
        assert s.quads and s.prof["n_other_culled"] == 0  # the fused kernels' loop over the records outside the hierarchies
    elif name in ("lattice", "lattice_divided", "lattice_twins", "nested"):
        assert s.prof["n_obvh_nodes"] > 0  # other_trace
        if name == "lattice_divided":
            assert len(s.w.groups_bytes()) // 56 >= 4
    elif name == "lines":
        assert s.prof["n_lbvh_nodes"] > 0  # line_trace
    elif name == "mesh":
        assert (s.tris, s.csg) == (True, False)
        assert s.tri_plan["records"] == 64 and s.tri_plan["nodes"] > 0  # tri_trace (`ran`: held per call by the sweep)
    elif name == "csg":
        assert (s.tris, s.csg) == (True, True)
        cp = rt._rtamd._csg_plan(s.w)
        assert cp["units"] == tie_worlds.N_UNITS and cp["records"] == tie_worlds.N_UNITS and cp["remainder"] == 0, cp
        assert cp["nodes"] >= 1 and s.csg_ran  # unit_trace, in every variant
