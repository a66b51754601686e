"""Far-origin and tangent rays (tests/far_rays.py) on the device against the CPU oracle: origins 2^4 .. 2^44 away
from what they aim at, on every culling path. The terms that exist only for distant origins are the K = max|o *
(1/d)| slack of the fp32 child-box test (set_ray32, wide_keys2) and of the pop cull (rt_wkey_beyond), the 2^-48
band of the fp64 joint slab filter (box_hit) and the pad of the tight Rotate culling box (flat_box).

  (a) the reference's tree with the reference's cull: the oracle's hits on every ray, no allowance;
  (b) the default upload, every walk: the oracle's hits on every ray of each (family, rung) in which the host
      model (far_rays.predicted_culls) predicts no lost hit and the oracle agrees with itself over both trees;
  (c) everywhere else every differing ray is an artefact of rounding by the extended-precision judge
      (far_rays.artefacts), or a genuine hit that the reference's own box test lost;
  (d) tier-B renders through telephoto cameras 2^12 and 2^20 away: the production kernels on far first segments.
"""
import math
import os

import numpy as np
import pytest

import far_rays as F
import pyoracle
import rtamd
from conftest import parity

pytestmark = pytest.mark.gpu

WALK_NAMES = {0: "recursive", rtamd.RT_FLAG_REFERENCE_CULL: "reference_cull", rtamd.RT_DEBUG_RESUMABLE: "resumable",
              rtamd.RT_DEBUG_WIDE: "wide", rtamd.RT_DEBUG_QNODE: "qnode"}
WALKS = [(n, f) for n in F.WORLDS for f in (0, rtamd.RT_FLAG_REFERENCE_CULL, rtamd.RT_DEBUG_RESUMABLE)]
WALKS += [(n, rtamd.RT_DEBUG_WIDE) for n in ("chains", "rot_grid", "lattice")] + [("lattice", rtamd.RT_DEBUG_QNODE)]


def _field_rules(got, ref, rows):
    """test_closest_hits_per_kind's rules on `rows`: exact columns equal, surface t and p bit-identical (NaN
    where the oracle has NaN), sphere u, v within 4e-16. Returns the rows that break them."""
    g, r = got[rows], ref[rows]
    both_nan = np.isnan(g) & np.isnan(r)
    bad = ~np.all((g[:, F.EXACT_COLS] == r[:, F.EXACT_COLS]) | both_nan[:, F.EXACT_COLS], axis=1)
    bad |= ~np.all((g[:, 1:5] == r[:, 1:5]) | both_nan[:, 1:5], axis=1)
    with np.errstate(invalid="ignore"):
        du = np.abs(g[:, 8:10] - r[:, 8:10])
    du[both_nan[:, 8:10]] = 0
    bad |= ~np.all(du <= 4e-16, axis=1)  # (a NaN against a number compares false: bad)
    return rows[bad]


def _save(name, walk, rays, got, ref, rows):
    os.makedirs("out", exist_ok=True)  # (kept out of git)
    np.savez(f"out/far_{name}_{walk}.npz", rows=rows, rays=rays[rows], got=got[rows], ref=ref[rows])


@pytest.mark.parametrize("name", F.WORLDS)
def test_anchor_reference_tree_and_cull(gpu_ctx, name):
    """(a) The caller's tree uploaded as it is, walked recursively with the reference's per-axis cull: the
    oracle's closest hit on every ray of every family and rung. This pins the leaf tests, rotate_point /
    unrotate_point, the guarded quotients' trusted range and the frame records at magnitudes up to 2^44."""
    rays = F.rays(name)[0]
    ref = F.oracle_hits(name)
    gpu_ctx.upload(F.world(name).scene, reference_bvh=True)
    got = gpu_ctx.closest_hits(rays, F.T_MIN, np.inf, seed=3, flags=rtamd.RT_FLAG_REFERENCE_CULL)
    bad = _field_rules(got, ref, np.arange(len(rays)))
    print(f"far {name} anchor: {len(bad)} of {len(rays)} rays differ; bit-identical in every field "
          f"{np.all((got == ref) | (np.isnan(got) & np.isnan(ref)), axis=1).mean():.5f}")
    if len(bad):
        _save(name, "anchor", rays, got, ref, bad)
    assert not len(bad), f"{len(bad)} rays differ, first {bad[:8].tolist()}"


@pytest.mark.parametrize("name,flags", WALKS)
def test_default_upload_every_walk(gpu_ctx, name, flags, monkeypatch):
    """(b) and (c): one closest_hits call over all rungs and families per (world, walk) on the default upload
    (SAH tree, tight Rotate boxes, joint filter unless RT_FLAG_REFERENCE_CULL). In each (family, rung) where the
    host model predicts no lost hit and the oracle finds the same hits in the device's tree as in the caller's
    (both conditions are the host's alone), every ray equals the oracle; this holds for the fp32 walks too,
    whose test accepts every box whose exact interval meets [t_min, t_max] (the proof at wide_keys2). Elsewhere every differing ray is an
    artefact of rounding, or a genuine nearer hit that the reference's own box test lost on the caller's tree.

    The resumable walk found one product fault here, since mended: on one ray of 49 152 in rot_grid (tangent,
    2^36) and one in frames (corner, 2^44) several spheres reported one and the same t far outside themselves,
    the walk flagged the tie, and the tie redo bounded by nextafter(t*) over the caller's tree, whose boxes cull
    such hits, ended with no hit at all where the reference has a genuine one beyond t*. A bounded redo that
    finds nothing is now redone in full (rt_trace.h redo_again)."""
    if flags == rtamd.RT_DEBUG_QNODE:
        monkeypatch.setenv("RTAMD_QNODE", "1")  # (read at upload)
    rays, fam, rung = F.rays(name)
    ref = F.oracle_hits(name)
    sc = F.world(name).scene
    lost = F.predicted(name)[0]
    table = np.array(F.cull_table(lost | F.trees_differ(name), fam, rung))
    clean = table[fam, rung] == 0
    gpu_ctx.upload(sc)
    got = gpu_ctx.closest_hits(rays, F.T_MIN, np.inf, seed=3, flags=flags)
    walk = WALK_NAMES[flags]
    bad = _field_rules(got, ref, np.arange(len(rays)))
    is_bad = np.zeros(len(rays), dtype=bool)
    is_bad[bad] = True
    share = np.array(F.cull_table(is_bad, fam, rung)) / F.PER
    print(f"far {name} {walk}: predicted lost or tree-dependent per family and rung {table.tolist()}; differing share "
          f"{np.round(share, 4).tolist()}")
    if len(bad):
        _save(name, walk, rays, got, ref, bad)
    assert clean.sum() >= 8 * F.PER  # (the oracle and the model alone: the low rungs)
    in_clean = bad[clean[bad]]
    assert not len(in_clean), (f"{len(in_clean)} rays differ where no lost hit is predicted, first "
                               f"{in_clean[:8].tolist()}: family, rung "
                               f"{sorted(set(zip(fam[in_clean].tolist(), rung[in_clean].tolist())))}")
    rb, paths = F._rebuilt(sc)
    real, ref_lost = F.artefacts(rb, paths, rays, ref, got, bad)
    print(f"far {name} {walk}: of {len(bad)} differing rays {len(ref_lost)} genuine hits lost by the reference's "
          f"tree, {len(real)} not explained by rounding")
    assert not real, f"{len(real)} differing rays are no artefacts, first {real[:8]}"


# ----------------------------------------------------------------------------- (d) telephoto renders
F_MIXW, F_ALL = 1024, 63 | 512
TELE = {"random_book_one": ((13.0, 2.0, 3.0), (0.0, 0.0, 0.0), 20.0, 0), "chains": None, "frames": None}
TELE_VARIANT = {"random_book_one": 0, "chains": 21, "frames": 1599}  # rt_layout.h: kVarSpheres, kVarCornell, kVarFull
W, H = 48, 32


def _telephoto(name, dist):
    """The world's usual view from `dist` away along the same line of sight, the field of view narrowed so that
    the same extent fills the frame; no aperture."""
    if TELE[name] is None:
        import zoo_worlds
        lf, la, vfov = zoo_worlds.CAMERAS[name][:3]
    else:
        lf, la, vfov = TELE[name][:3]
    lf, la = np.array(lf), np.array(la)
    d0 = float(np.linalg.norm(lf - la))
    frm = la + (lf - la) / d0 * dist
    fov = 2.0 * math.degrees(math.atan(math.tan(math.radians(vfov) / 2.0) * d0 / dist))
    return rtamd.newCamera(tuple(frm), tuple(la), (0.0, 1.0, 0.0), fov, W / H, 0.0, dist, 0.0, 1.0)


def _scene(name):
    if name == "random_book_one":
        return rtamd.make_scene(name, rtamd.randGen(1024))[0]
    return F.world(name).scene


@pytest.mark.parametrize("dist", [2.0 ** 12, 2.0 ** 20])
@pytest.mark.parametrize("name", list(TELE))
def test_telephoto_renders(gpu_ctx, name, dist):
    """(d) Tier B at 48x32, 4 spp, depth 12, seed 1024, flags 0 and RT_FLAG_NAN_ZERO, from 2^12 and 2^20 away:
    every primary ray is a far first segment through the production kernels (packed keys, pop cull, the mixed
    walk). Against the oracle by the project's thresholds (>= 99.9 % of channels within 1e-3, >= 99.9 % of bytes
    equal); on the oracle alone, the view is lit in at least 0.3 of its pixels."""
    sc = _scene(name)
    cam = _telephoto(name, dist)
    gpu_ctx.upload(sc)
    for flags in (0, rtamd.RT_FLAG_NAN_ZERO):
        p = rtamd.make_params(W, H, 4, 12, rtamd.RT_RNG_PHILOX, seed=1024, flags=flags)
        rgb_o, lin_o, _, _ = pyoracle.render(sc, cam, p)
        if flags:
            bg = np.array([pyoracle.lib().oracle_scale_color(float(x)) for x in sc.desc.background], dtype=np.uint8)
            lit = np.any(rgb_o != bg, axis=2).mean()
            assert lit >= 0.3, lit
        rgb_g, lin_g, _ = gpu_ctx.render(cam, p, linear=True)
        launch = gpu_ctx.last_launch()
        ok, eq, dmax = parity(lin_g, lin_o, rgb_g, rgb_o)
        print(f"far telephoto {name} 2^{int(math.log2(dist))} flags {flags}: channels within 1e-3 {ok:.6f}, bytes "
              f"equal {eq:.6f}, max |d| {dmax:.3g}; launch variant {launch['variant']} loop {launch['loop']}")
        assert ok >= 0.999, f"only {ok:.5f} of channels within 1e-3 (max |d| {dmax:.3g})"
        assert eq >= 0.999, f"only {eq:.5f} of bytes equal"
        assert launch["variant"] & (F_ALL | F_MIXW) == TELE_VARIANT[name] and launch["loop"] >= 1, launch
