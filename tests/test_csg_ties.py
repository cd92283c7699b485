"""The condition of the Csg GPU comparisons, held on the CPU: in every fixed
scene of tests/test_gpu_csg.py, over its hit-record rays, and in the twelve
random seeds, no Csg node's sorted list holds two equal t (the checker's
csg_ties is 0), so the reference's unstable sort decides nothing there. A tie
is a rule, not a measurement: a later change of scene or seed that brings one
in fails here, without a GPU. The one deliberate tie is checked to be one."""
import numpy as np
import pytest

import csg_ref
import test_gpu_csg as scenes_under_test


@pytest.mark.parametrize("name", sorted(scenes_under_test.FIXED))
def test_fixed_scene_has_no_tie(rt, name):
    w, cam, depth = scenes_under_test.FIXED[name](rt)
    ref = csg_ref.CsgRef.from_world(w)
    img, st = ref.render(cam.desc_bytes(), depth)
    assert ref.csg_ties == 0 and img.sum() > 0 and st["rays_shadow"] > 100


@pytest.mark.parametrize("seed", range(12))
def test_random_scene_has_no_tie(rt, seed):
    from rtamd import scenes
    w, cam, depth = scenes.csg_random(seed, scenes_under_test.W, scenes_under_test.H)
    ref = csg_ref.CsgRef.from_world(w)
    ref.render(cam.desc_bytes(), depth)
    assert ref.csg_ties == 0


def test_hit_record_rays_have_no_tie_and_the_deliberate_one_has(rt):
    w = scenes_under_test._three_ops(rt)
    ref = csg_ref.CsgRef.from_world(w)
    ref.hit_batch(scenes_under_test._three_ops_rays())
    assert ref.csg_ties == 0
    w, rays = scenes_under_test._tie_case(rt)
    ref = csg_ref.CsgRef.from_world(w)
    ref.hit_batch(rays)
    assert ref.csg_ties > 0
