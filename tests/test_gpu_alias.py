"""Worlds with structurally equal shapes on the GPU (World.upload(aliases=True): rt_shapes_equal_pairs, then
rt_scene_create_aliased), bit for bit against the oracle, whose `containers` walk goes by structural equality as the
reference's does (oracle/rt_oracle.c:640-661).

The worlds of tests/alias_worlds.py (tests/test_alias_worlds.py shows that aliasing changes each of their frames),
each rendered on the fast path, its counting run, the exhaustive pipeline and the run that skips no shadow ray, as
frames, X4 frames and ray batches (hit records, shadows and colours); a sweep of every reachable instantiation of the
ALIAS kernel class with the plan that ran asserted (the pattern of tests/test_gpu_variants.py); 24 seeded fuzz worlds
with one to three shapes duplicated exactly or nudged by less than EPSILON / 3, some of them members of groups; and a
world without aliases, which renders the same bytes through either entry point. No tolerance anywhere.
"""
import os
import random

import numpy as np
import pytest

import alias_worlds as aw
import test_gpu_variants as gv

pytestmark = pytest.mark.gpu
NTHREADS = max(1, min(16, os.cpu_count() or 1))
COUNTS = ("rays_primary", "rays_reflect", "rays_refract", "rays_shadow", "sphere_tests", "plane_tests", "other_tests")
EXACT = COUNTS + ("sphere_disc_ge0",)  # the exhaustive pipeline's, as tests/test_gpu_fuzz.py holds them
EPS = 0.00001


def _uploaded(rt, name):
    w, cam = aw.WORLDS[name](rt)
    w.upload(aliases=True)
    return w, cam


def _alias_plan(rt, w, members, classes, fused=True):
    """The last render ran the ALIAS kernels (launch_fused chooses them by the scene's alias members), fused or not."""
    assert bool(rt._rtamd._wf_profile(w, -1, True)["fused"]) == fused
    plan = rt._rtamd._wf_plan(w)
    assert (plan["n_alias_members"], plan["n_alias_classes"]) == (members, classes), plan
    return plan


def _four_ways(rt, w, run, members, classes):
    """run(want_stats, exhaustive) -> (array, stats): the fast path, its counting run, the exhaustive pipeline and the
    fast path with no shadow ray skipped."""
    out = {"fast": run(False, False)}
    _alias_plan(rt, w, members, classes)
    out["counted"] = run(True, False)
    _alias_plan(rt, w, members, classes)
    assert not out["counted"][1]["exhaustive"]
    out["exhaustive"] = run(True, True)
    assert out["exhaustive"][1]["exhaustive"]
    w.tune("skip_shadow", 0)
    try:
        out["every_shadow_ray"] = run(True, False)
        _alias_plan(rt, w, members, classes)
    finally:
        w.tune("skip_shadow", 1)
    return out


def _hold(out, want, counts):
    for how, (got, st) in out.items():
        got = np.asarray(got)
        assert got.shape == want.shape
        bad = np.flatnonzero((got != want).reshape(-1, 3).any(axis=1))
        assert len(bad) == 0, (how, len(bad), bad[:5], got.reshape(-1, 3)[bad[0]], want.reshape(-1, 3)[bad[0]])
        if how != "fast":
            for k in (EXACT if how == "exhaustive" else COUNTS):
                assert st[k] == counts[k], (how, k, st[k], counts[k])
    assert out["every_shadow_ray"][1]["rays_shadow_traced"] == counts["rays_shadow"]


_REF = {}


def _reference(oracle, name, w, cam):
    """The oracle's frame, X4 frame, and hit records / shadows / colours of the world's batch rays, once per world."""
    if name not in _REF:
        ow = oracle.OracleWorld.from_world(w)
        frame, fst = ow.render(cam.desc_bytes(), aw.DEPTH, nthreads=NTHREADS)
        x4, _ = ow.render_rows(cam.desc_bytes(), aw.DEPTH, list(range(aw.H)), NTHREADS, aa_samples=4)
        rng = np.random.default_rng(len(name) + 11)
        n = 600
        o = rng.uniform([-3.5, -2.5, -4.0], [3.5, 3.5, 5.0], size=(n, 3))  # many origins inside the aliased shapes
        d = rng.normal(size=(n, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        rays = np.hstack([o, d])
        hits = np.array([ow.hit(r[:3], r[3:]) for r in rays])
        shadows = [np.array([ow.is_shadowed(p, light) for p in o]) for light in range(w.n_lights())]
        colours, cst = ow.color_at_batch(rays, aw.DEPTH)
        for a in (frame, x4, rays, hits, colours):
            a.setflags(write=False)
        _REF[name] = dict(frame=frame, fst=fst, x4=x4, rays=rays, hits=hits, shadows=shadows, colours=colours, cst=cst)
    return _REF[name]


@pytest.mark.parametrize("name", sorted(aw.WORLDS))
def test_frames_four_ways_and_x4(rt, oracle, name):
    w, cam = _uploaded(rt, name)
    ref = _reference(oracle, name, w, cam)
    members, classes = aw.CLASSES[name]
    out = _four_ways(rt, w, lambda stats, exh: (lambda r: (r[0].to_numpy(), r[1]))(cam.render(w, aw.DEPTH, stats, exh)),
                     members, classes)
    _hold(out, ref["frame"], ref["fst"])
    assert rt.canvas_to_ppm(out["fast"][0]) == oracle.canvas_to_ppm(ref["frame"])
    cam.render_opts.aa_samples(rt.AASamples.X4)
    try:
        fast, _ = cam.render_multithreaded(w, aw.DEPTH, False)
        _alias_plan(rt, w, members, classes)
        exh, _ = cam.render_multithreaded(w, aw.DEPTH, True, True)
    finally:
        cam.render_opts.aa_samples(rt.AASamples.X1)
    for how, got in (("fast", fast.to_numpy()), ("exhaustive", exh.to_numpy())):
        assert got.tobytes() == ref["x4"].tobytes(), (how, int((got != ref["x4"]).sum()))
    w.check()


@pytest.mark.parametrize("name", sorted(aw.WORLDS))
def test_ray_batches(rt, oracle, name):
    w, cam = _uploaded(rt, name)
    ref = _reference(oracle, name, w, cam)
    rays, want = ref["rays"], ref["hits"]
    got = np.asarray(w.hit_batch(rays))
    assert np.array_equal(got[:, 0], want[:, 0])
    hit = want[:, 0] >= 0
    assert hit.sum() > 100
    bad = np.flatnonzero((got[hit] != want[hit]).any(axis=1))  # every column: geometry, n1, n2, Schlick
    assert len(bad) == 0, (len(bad), got[hit][bad[0]], want[hit][bad[0]])
    for light, rs in enumerate(ref["shadows"]):
        assert np.array_equal(np.asarray(w.is_shadowed_batch(rays[:, :3], light)).astype(bool), rs), light
    members, classes = aw.CLASSES[name]
    out = _four_ways(rt, w, lambda stats, exh: (lambda r: (np.asarray(r[0]), r[1]))(w.color_at_batch(rays, aw.DEPTH, stats, exh)),
                     members, classes)
    _hold(out, ref["colours"], ref["cst"])
    w.check()


# ---------------------------------------------------------------- every instantiation of the ALIAS class
# (LANE, TALLY, CAM) of wf_trace_fused<.., QUADS = TRIS = CSG = ALIAS = true>: launch_fused_q's 2 + 2 x 4 and
# launch_glb_lane's 3 x 4. LANE 0 only ever takes camera rays; LANE 3 and 1 take them only in a world without
# diagonal spheres (tests/test_gpu_variants.py LAUNCH_TABLE), here `nodiag`.
ALIAS_TABLE = {(0, tally, True) for tally in (False, True)} | {
    (lane, tally, cam) for lane in (15, 14, 4, 3, 1) for tally in (False, True) for cam in (False, True)}
assert len(ALIAS_TABLE) == 22


def _nodiag(rt):
    """No diagonal sphere: turned spheres and cubes (their hierarchy opens the fused generations), a floor, and a
    duplicated glass cylinder around a turned sphere."""
    w = rt.World()
    w.add_light(rt.PointLight(rt.Point(-8.0, 12.0, -14.0), rt.Color(1.0, 1.0, 1.0)))
    w.add_light(rt.PointLight(rt.Point(6.0, 9.0, -10.0), rt.Color(0.4, 0.4, 0.5)))
    floor = rt.Plane()
    floor.set_transform(rt.translation(0, -2.0, 0))
    floor.material.set_pattern(rt.checkers_pattern(rt.Color(0.8, 0.8, 0.8), rt.Color(0.2, 0.2, 0.3)))
    floor.material.reflective = 0.2
    w.add_object(floor)
    rnd = random.Random(7)
    for k in range(18):
        s = rt.Sphere() if k % 3 else rt.Cube()
        s.set_transform(rt.translation(rnd.uniform(-4, 4), rnd.uniform(-1, 3), rnd.uniform(3, 9)) * rt.rotation_z(0.3 + 0.1 * k) *
                        rt.scaling(0.6, 0.4, 0.5))
        s.material.color = rt.Color(rnd.random(), rnd.random(), rnd.random())
        if k % 5 == 0:
            s.material.reflective = 0.4
        w.add_object(s)
    for dx in (0.0, aw.NUDGE):
        c = rt.Cylinder(-1.0, 1.0, True)
        c.set_transform(rt.translation(dx, 0.2, 1.0) * rt.rotation_x(0.5) * rt.scaling(1.4, 1.2, 1.4))
        m = c.material
        m.transparency, m.refractive_index, m.diffuse, m.ambient, m.reflective = 1.0, 1.5, 0.1, 0.05, 0.3
        w.add_object(c)
    return w, aw._camera(rt, (0.0, 0.5, -5.0), (0.0, 0.2, 2.0))


SWEEP_SCENES = {"near_pair": aw.near_pair, "grouped_twin": aw.grouped_twin, "nodiag": _nodiag}


class _Sweep:
    def __init__(self, rt, oracle, name):
        self.rt, self.name, self.failures, self.reached = rt, name, [], set()
        self.w, self.cam = SWEEP_SCENES[name](rt)
        w, cam = self.w, self.cam
        w.upload(aliases=True)
        self.depth = 3
        exh, self.st = cam.render(w, self.depth)
        frame = exh.to_numpy()
        ref, rst = oracle.OracleWorld.from_world(w).render(cam.desc_bytes(), self.depth, nthreads=NTHREADS)
        self.check(frame.tobytes() == ref.tobytes(), f"exhaustive != oracle in {int((frame != ref).sum())} channels")
        for k in EXACT:
            self.check(self.st[k] == rst[k], f"oracle counter {k}: {self.st[k]} != {rst[k]}")
        self.frame = frame.tobytes()
        self.prof = gv._prof(rt, w)
        self.check((self.prof["n_diag"] == 0) == (name == "nodiag"), f"n_diag {self.prof['n_diag']}")
        self.check(rt._rtamd._wf_plan(w)["n_alias_members"] == 2, "no alias members")
        self.rays = gv._rays(17, 400)
        self.batch = w.color_at_batch(self.rays, self.depth, True, True)
        for vname, knobs, lane, n_top, deltas in gv._variants():
            try:
                gv._tune(w, knobs)
                self.variant(vname, knobs, lane, n_top, deltas)
            finally:
                gv._restore(w, knobs)
        w.check()

    def check(self, ok, what):
        if not ok and len(self.failures) < 20:
            self.failures.append(f"{self.name}: {what}")

    def plan(self, what, knobs, lane, n_top, deltas, camera, tally):
        p = self.rt._rtamd._wf_plan(self.w)
        self.check(p["n_alias_members"] == 2 and p["n_alias_classes"] == 1, f"{what}: {p}")
        want = gv._expected(self.prof, knobs, lane, n_top, deltas, camera)
        for which, (wl, wt, wd, ws), cam_rays in (("primary", want[0], camera), ("secondary", want[1], False)):
            got = p[which]
            ok = (got["lane"], got["n_top"], got["lds_deltas"], got["lds_spheres"]) == (wl, wt, wd, ws)
            self.check(ok, f"{what}: {which} plan {got}, expected lane {wl} n_top {wt} deltas {wd} spheres {ws}")
            if ok:
                self.reached.add((wl, tally, cam_rays or wl == 0))

    def variant(self, vname, knobs, lane, n_top, deltas):
        w, cam, depth = self.w, self.cam, self.depth
        args = (knobs, lane, n_top, deltas)
        fast, _ = cam.render(w, depth, want_stats=False)
        self.plan(f"{vname} render", *args, camera=True, tally=False)
        self.check(fast.to_numpy().tobytes() == self.frame, f"{vname}: fast frame != exhaustive")
        cnt, st = cam.render(w, depth, want_stats=True, exhaustive=False)
        self.plan(f"{vname} counted render", *args, camera=True, tally=True)
        self.check(cnt.to_numpy().tobytes() == self.frame, f"{vname}: counted fast frame != exhaustive")
        for k in COUNTS:
            self.check(st[k] == self.st[k], f"{vname}: counted fast render {k}: {st[k]} != {self.st[k]}")
        col, _ = w.color_at_batch(self.rays, depth, False, False)
        self.plan(f"{vname} batch", *args, camera=False, tally=False)
        self.check(col.tobytes() == self.batch[0].tobytes(), f"{vname}: batch != exhaustive")
        col, st = w.color_at_batch(self.rays, depth, True, False)
        self.plan(f"{vname} counted batch", *args, camera=False, tally=True)
        self.check(col.tobytes() == self.batch[0].tobytes(), f"{vname}: counted batch != exhaustive")
        for k in COUNTS:
            self.check(st[k] == self.batch[1][k], f"{vname}: counted batch {k}: {st[k]} != {self.batch[1][k]}")


@pytest.fixture(scope="module")
def sweep(rt, oracle):
    done = {}

    def run(name):
        if name not in done:
            done[name] = _Sweep(rt, oracle, name)
        return done[name]
    return run


@pytest.mark.parametrize("name", sorted(SWEEP_SCENES))
def test_alias_variants_bitwise(sweep, name):
    s = sweep(name)
    assert not s.failures, "\n".join(s.failures)
    assert s.reached and s.st["rays_refract"] > 20 and s.st["other_tests"] > 0


def test_every_alias_kernel_ran(sweep):
    reached = set()
    for name in sorted(SWEEP_SCENES):
        reached |= sweep(name).reached
    assert reached <= ALIAS_TABLE, reached - ALIAS_TABLE
    assert not (ALIAS_TABLE - reached), sorted(ALIAS_TABLE - reached)


# ---------------------------------------------------------------- fuzz
def _path(obj, rnd):
    """The way down `obj` to one of its primitives, as child indices ([]: `obj` is one); None: there is none."""
    path = []
    while hasattr(obj, "n_children"):
        if obj.n_children() == 0:
            return None
        path.append(rnd.randrange(obj.n_children()))
        obj = obj.child(path[-1])
    return path


def _at(w, i, path):
    """A fresh copy of that primitive, with its final transform (a group's is baked into its members')."""
    obj = w.child(i)
    for k in path:
        obj = obj.child(k)
    return obj


def _cliques(pairs):
    """Every connected component of the pairs is complete."""
    near = {}
    for a, b in pairs:
        near.setdefault(a, {a}).add(b)
        near.setdefault(b, {b}).add(a)
    return all(near[b] == near[a] for a in near for b in near[a])


def _fuzz_world(rt, seed):
    """scenes.fuzz(seed) with one to three of its primitives duplicated once or twice: exactly, or nudged by less than
    EPSILON / 3 an axis; a twin goes to the top level or into a new group of its own. A small shape's inverse
    magnifies the nudge, and a family whose members are not all `==` each other is no clique (the library refuses
    it): the nudges are then shrunk until every family is one."""
    from rtamd import scenes
    for shrink in (1.0, 0.3, 0.1, 0.03, 0.01, 0.0):
        w, cam, depth = scenes.fuzz(seed, 32, 24)
        rnd = random.Random(1000 + seed)
        tally = dict(grouped=0, nudged=0, triples=0)
        n = w.n_objects()
        for i in rnd.sample(range(n), min(n, rnd.randrange(1, 4))):
            path = _path(w.child(i), rnd)
            if path is None:
                continue
            tally["grouped"] += len(path) > 0
            copies = rnd.choice((1, 1, 2))
            tally["triples"] += copies == 2
            for _ in range(copies):
                twin = _at(w, i, path)
                if rnd.random() < 0.6:
                    d = [shrink * rnd.uniform(-EPS / 3, EPS / 3) for _ in range(3)]
                    twin.set_transform(rt.translation(*d) * twin.transform)
                    tally["nudged"] += 1
                if rnd.random() < 0.4:
                    g = rt.Group()
                    g.add_child(twin)
                    w.add_object(g)
                    tally["grouped"] += 1
                else:
                    w.add_object(twin)
        pairs = aw.equal_pairs(w.descs_bytes())
        if pairs and _cliques(pairs):
            return w, cam, depth, tally
    raise AssertionError(f"seed {seed}: no family of duplicates is a clique")


FUZZ_SEEDS = tuple(range(24))


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_fuzz_worlds_with_duplicates(rt, oracle, seed):
    w, cam, depth, _ = _fuzz_world(rt, seed)
    pairs = aw.equal_pairs(w.descs_bytes())
    assert pairs, "no duplicate survived"
    w.upload(aliases=True)
    fast, _ = cam.render(w, depth, want_stats=False)
    plan = rt._rtamd._wf_plan(w)
    assert plan["n_alias_members"] == len({i for p in pairs for i in p}) and plan["n_alias_classes"] >= 1
    exh, st = cam.render(w, depth)
    ref, rst = oracle.OracleWorld.from_world(w).render(cam.desc_bytes(), depth, nthreads=NTHREADS)
    e = exh.to_numpy()
    assert e.tobytes() == ref.tobytes(), f"seed {seed}: {int((e != ref).sum())} channels differ from the oracle"
    assert fast.to_numpy().tobytes() == e.tobytes(), f"seed {seed}: fast path differs from the exhaustive frame"
    for k in EXACT:
        assert st[k] == rst[k], (seed, k, st[k], rst[k])
    cnt, cst = cam.render(w, depth, want_stats=True, exhaustive=False)
    assert cnt.to_numpy().tobytes() == e.tobytes()
    for k in COUNTS:
        assert cst[k] == rst[k], (seed, k, cst[k], rst[k])
    w.check()


def test_the_fuzz_worlds_hold_what_they_are_for(rt):
    tot = dict(grouped=0, nudged=0, triples=0)
    for seed in FUZZ_SEEDS:
        for k, v in _fuzz_world(rt, seed)[3].items():
            tot[k] += v
    assert tot["grouped"] >= 3 and tot["nudged"] >= 8 and tot["triples"] >= 3, tot


# ---------------------------------------------------------------- the scene parser (always opted in)
def test_a_scene_file_with_a_shape_placed_twice(rt, oracle, tmp_path):
    p = rt.SceneParser()
    p.load_str(aw.TWICE_YAML)
    canvas, st = p.render(5)
    w = p.build_world()
    ref, rst = oracle.OracleWorld.from_world(w).render(p.camera.desc_bytes(), 5, nthreads=NTHREADS)
    got = canvas.to_numpy()
    assert got.tobytes() == ref.tobytes(), int((got != ref).sum())
    for k in COUNTS:  # (SceneParser.render counts on the fast path: sphere_disc_ge0 is the exhaustive pipeline's)
        assert st[k] == rst[k], (k, st[k], rst[k])
    exh, est = p.camera.render(w, 5, True, True)
    assert exh.to_numpy().tobytes() == ref.tobytes()
    for k in EXACT:
        assert est[k] == rst[k], (k, est[k], rst[k])
    fast, _ = p.camera.render(w, 5, want_stats=False)
    assert fast.to_numpy().tobytes() == ref.tobytes()
    assert rt._rtamd._wf_plan(w)["n_alias_members"] == 4 and rt._rtamd._wf_plan(w)["n_alias_classes"] == 2
    out = tmp_path / "twice.ppm"
    p.render_to(str(out), 5)  # what bin/render_scene calls
    assert out.read_bytes() == oracle.canvas_to_ppm(ref)


# ---------------------------------------------------------------- a world without aliases
@pytest.mark.parametrize("seed", [3, 62])
def test_no_aliases_same_bytes_through_either_entry_point(rt, seed):
    from rtamd import scenes
    w, cam, depth = scenes.fuzz(seed, 32, 24)
    assert aw.equal_pairs(w.descs_bytes()) == []
    plain_fast, _ = cam.render(w, depth, want_stats=False)
    plain_exh, plain_st = cam.render(w, depth)
    before = rt._rtamd._wf_plan(w)
    w.upload(aliases=True)  # rt_scene_create_aliased with n_pairs = 0
    assert w.aliases
    fast, _ = cam.render(w, depth, want_stats=False)
    after = rt._rtamd._wf_plan(w)
    assert after["n_alias_members"] == 0 and after["n_alias_classes"] == 0
    exh, st = cam.render(w, depth)
    assert fast.to_numpy().tobytes() == plain_fast.to_numpy().tobytes()
    assert exh.to_numpy().tobytes() == plain_exh.to_numpy().tobytes()
    for k in EXACT:
        assert st[k] == plain_st[k], (k, st[k], plain_st[k])
    assert before["n_alias_members"] == 0
