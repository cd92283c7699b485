"""The worlds of tests/alias_worlds.py on the CPU: aliasing changes each of their frames.

The oracle (oracle/rt_oracle.c) walks `containers` by structural equality, as the reference does; the checker of
tests/csg_ref.py walks by object identity. A world whose two frames are equal would prove nothing about aliasing on the
GPU, so each world must differ in at least one pixel. Also held here: rt_shapes_equal_pairs finds exactly the classes
each world is named for (from the descs the library itself is given), and the default upload still refuses them.
"""
import numpy as np
import pytest

import alias_worlds as aw
import csg_ref


@pytest.mark.parametrize("name", sorted(aw.WORLDS))
def test_aliasing_changes_the_frame(rt, oracle, name):
    w, cam = aw.WORLDS[name](rt)
    by_equality, _ = oracle.OracleWorld.from_world(w).render(cam.desc_bytes(), aw.DEPTH, nthreads=4)
    with np.errstate(all="ignore"):
        by_identity, _ = csg_ref.CsgRef.from_world(w).render(cam.desc_bytes(), aw.DEPTH)
    assert by_equality.shape == (aw.H, aw.W, 3) and np.isfinite(by_equality).all()
    changed = int((by_equality != by_identity).any(axis=2).sum())
    print(f"{name}: {changed} of {aw.W * aw.H} pixels differ between the walk by equality and the walk by identity")
    assert changed >= 1


@pytest.mark.parametrize("name", sorted(aw.WORLDS))
def test_the_helper_finds_the_classes(rt, name):
    w, _ = aw.WORLDS[name](rt)
    pairs = aw.equal_pairs(w.descs_bytes())
    members = sorted({i for p in pairs for i in p})
    n_members, n_classes = aw.CLASSES[name]
    assert len(members) == n_members and len(pairs) == n_members * (n_members - 1) // 2 * n_classes, pairs


def test_the_default_upload_still_refuses(rt):
    w, _ = aw.WORLDS["near_pair"](rt)
    assert not w.aliases
    with pytest.raises(rt.RtError, match="structurally equal"):
        w.upload()
