"""Far-origin and tangent rays (tests/far_rays.py), host side: the rays' power on the oracle alone, the
re-bounded trees against the caller's tree with every differing ray judged in extended precision, and the
tight Rotate culling box against the reference's (tests/test_gpu_far_rays.py runs the same rays on the
device)."""
import numpy as np
import pytest

import far_rays as F
import pyoracle
import rtamd


@pytest.mark.parametrize("name", F.WORLDS)
def test_rays_have_power(name):
    """On the oracle alone: every (family, rung) hits something with at least a quarter of its rays, and
    every leaf kind of the world is the closest hit of at least 100 rays."""
    rays, fam, rung = F.rays(name)
    ref = F.oracle_hits(name)
    assert len(rays) == len(F.FAMILIES) * len(F.RUNGS) * F.PER
    share = [[float(ref[(fam == fi) & (rung == ri), 0].mean()) for ri in range(len(F.RUNGS))]
             for fi in range(len(F.FAMILIES))]
    counts = F.kind_counts(F.world(name), ref)
    print(f"{name}: hit share per family and rung {np.round(share, 3).tolist()}; fewest hits of a kind "
          f"{min(counts.values())}")
    share = np.array(share)
    if name == "lattice":
        # One cell cannot be hit at all, by the reference's own arithmetic: an axis ray (a = d.d exact, b = oc.d
        # one product) from 2^44 away has c = fl(oc.oc - r^2) = fl(b^2), since r^2 + |offset|^2 <= 1e6 + 2^6 is
        # below half an ulp of 2^88 (2^35), so disc = b^2 - a c is exactly 0 and `disc > 0` fails for every
        # sphere, and this world holds spheres only. Pinned as such, not waived.
        fi, ri = F.FAMILIES.index("axis"), len(F.RUNGS) - 1
        assert share[fi, ri] == 0.0
        share[fi, ri] = 1.0
    assert np.min(share) >= 0.25, share
    assert min(counts.values()) >= 100, counts


def test_exact_judge_on_plain_cases():
    """The judge on rays whose answer is known: through a leaf's middle (meets), past it by a leaf's size
    (misses), starting beyond it (t < t_min: misses), for a leaf of every kind and chain of `chains`."""
    sc = F.world("chains").scene
    paths = F.leaf_paths(sc)
    c0, _, half, _ = F._targets("chains")
    assert {p.kind for p in paths} == set(F._PRIMS) - {rtamd.RT_NODE_MOVING_SPHERE}
    d = np.array([0.3, -0.8, 0.52])
    for p, c, h in zip(paths, c0, half):
        far = 3.0 * max(h.max(), 1.0)
        assert F.exact_judge(sc, np.concatenate([c - 50.0 * d, d, [0.5]]), p)
        assert not F.exact_judge(sc, np.concatenate([c + far * np.array([0.8, 0.52, 0.3]) - 50.0 * d, d, [0.5]]), p)
        assert not F.exact_judge(sc, np.concatenate([c + 50.0 * d, d, [0.5]]), p)
    import zoo_worlds
    with pytest.raises(ValueError):  # (a kind these worlds do not hold)
        F.leaf_paths(zoo_worlds.build("media").scene)


@pytest.mark.parametrize("name", F.WORLDS)
def test_rebuilt_tree_differs_only_by_artefacts(name):
    """test_bvh's comparison on far and tangent rays: the oracle over the tree the device walks
    (rtamd.rebuilt_scene: SAH order, tight Rotate boxes, re-bounded frames) against the oracle over the caller's
    tree. Both use the reference's per-axis box test, so they differ where a box of one tree excludes a hit
    that the other's boxes admit. Every differing ray must be an artefact of rounding (far_rays.artefacts): the
    exact ray misses one of the leaves reported, or a reported hit is not where the exact ray meets its leaf
    (far_rays.genuine); or else the rebuilt tree has the nearer genuine hit, which the reference's own box test
    lost on the caller's tree."""
    rays, fam, rung = F.rays(name)
    a = F.oracle_hits(name)
    rb, paths = F._rebuilt(F.world(name).scene)
    b = pyoracle.closest_hits(rb, rays, F.T_MIN, np.inf, seed=3)
    diff = F.trees_differ(name)
    print(f"{name}: rays that differ between the two trees, per family and rung "
          f"{F.cull_table(diff, fam, rung)}")
    real, ref_lost = F.artefacts(rb, paths, rays, a, b, np.flatnonzero(diff))
    print(f"{name}: of {int(diff.sum())} differing rays {len(ref_lost)} are genuine hits that the caller's tree lost, "
          f"{len(real)} genuine hits that the rebuilt tree lost")
    assert not real, f"{len(real)} differing rays whose hits are all genuine, first {real[:8]}"


ROTATE_RUNGS = 5  # asserted through 2^36 (far_rays.RUNGS[:5]); beyond it no static pad holds


@pytest.mark.parametrize("name", ["rot_grid", "chains"])
def test_tight_rotate_boxes_add_no_predicted_cull(name):
    """The host model of the default walk (far_rays.predicted_culls: the device's joint box test on every
    ancestor box of the reference's hit leaf) with the shipped tight Rotate boxes against the same model in a
    fresh process with RTAMD_TIGHT_ROTATE=0 (the reference's 27-point boxes; the switch is read once per
    process). On every ray whose reference hit lies on a rect or cuboid below a Rotate, through 2^36: no
    hit is predicted lost with the tight boxes that is kept with the reference's. The comparison is one-sided
    and per leaf class because the two builds are different trees: sphere artefacts fall differently in them,
    and the reference's box, exact on its lower sides, culls corner hits that a padded box keeps. With
    the former pad of 2^-30 this failed at 2^28 and 2^36 (rot_grid: 1 and 10 rays, chains: 1 and 3)."""
    rays, fam, rung = F.rays(name)
    tight, cls = F.predicted(name)
    loose = F.predicted_in_child(name, {"RTAMD_TIGHT_ROTATE": "0"})
    rotated = cls == F.ROTATED
    assert (rotated & (rung < ROTATE_RUNGS)).sum() >= 5000  # (the oracle alone: the class is exercised)
    added = tight & ~loose & rotated
    print(f"{name}: hits on rotated leaves predicted lost, tight {F.cull_table(tight & rotated, fam, rung)}, "
          f"reference boxes {F.cull_table(loose & rotated, fam, rung)}, added {F.cull_table(added, fam, rung)}")
    assert not (added & (rung < ROTATE_RUNGS)).any(), F.cull_table(added, fam, rung)
