"""Builder-made worlds (tests/zoo_worlds.py) on the device against the CPU oracle: what the named scenes never
run. Rotations about X and Z (rotate_point / unrotate_point's other arms, the fused frame records' second
axis), every leaf kind under Translate / Rotate chains and inside instance frames, moving spheres under
chains, a medium inside a frame, and lights trees of three and four items whose leaves include kinds
htblRandom / htblPdfValue do not sample. Each kind of object has its own material, so each test can count
the closest hits per kind; the conditions on those counts are checked on the oracle's output alone."""
import functools

import numpy as np
import pytest

import pyoracle
import rtamd
import zoo_worlds
from conftest import parity

pytestmark = pytest.mark.gpu

F_WIDE, F_MIXW, F_ALL = 256, 1024, 63 | 512
VARIANT = {"chains": 21, "moving": 1583, "frames": 1599, "media": 1583}  # rt_layout.h: kVarCornell, kVarFull(Dark)
WALKS = [(n, f) for n in zoo_worlds.NAMES for f in (0, rtamd.RT_FLAG_REFERENCE_CULL, rtamd.RT_DEBUG_RESUMABLE)]
WALKS += [("chains", rtamd.RT_DEBUG_WIDE), ("moving", rtamd.RT_DEBUG_WIDE)]


@functools.lru_cache(maxsize=None)
def _oracle_hits(name):
    z = zoo_worlds.build(name)
    rays = zoo_worlds.rays(z)
    ref = pyoracle.closest_hits(z.scene, rays, 1e-4, np.inf, seed=3)
    ref.setflags(write=False)
    return rays, ref


def _ulp_close(a, b, ulps):
    return np.abs(a - b) <= ulps * np.spacing(np.maximum(np.abs(a), np.abs(b)))


@pytest.mark.parametrize("name,flags", WALKS)
def test_closest_hits_per_kind(gpu_ctx, name, flags):
    """2^14 rays per world (from outside, from among the frames' contents, axis-aligned, at times 0, 1 and
    nextafter(1, 0)) through the recursive walk (flags 0 / reference cull), the render loop's resumable walk
    and, where the world has no media or frames, the 4-wide walk. test_closest_hits_bit_exact's assertions:
    hit, normal, front face and material equal; surface t and p bit-identical; medium hits t within 4 ulps and
    p within 1e-13 of the scale (t goes through log: OCML against glibc); sphere u, v within 4e-16 (atan2 /
    asin), NaN where the oracle has NaN. And every kind of object is the closest hit of as many rays as in
    the oracle, at least 100."""
    z = zoo_worlds.build(name)
    rays, ref = _oracle_hits(name)
    want = zoo_worlds.kind_counts(z, ref)
    assert min(want.values()) >= 100, want  # (a condition on the rays: the oracle alone)
    gpu_ctx.upload(z.scene)
    got = gpu_ctx.closest_hits(rays, 1e-4, np.inf, seed=3, flags=flags)
    have = zoo_worlds.kind_counts(z, got)
    mats = z.scene.materials
    medium = (ref[:, 0] == 1) & (mats["type"][ref[:, 11].astype(int)] == 4)  # Isotropic phase = medium hit
    exact_cols = [0, 5, 6, 7, 10, 11]
    bad = ~np.all(got[:, exact_cols] == ref[:, exact_cols], axis=1)
    bad |= ~medium & ~np.all(got[:, 1:5] == ref[:, 1:5], axis=1)
    print(f"zoo {name} flags {flags}: hits per kind {have}; media hits {int(medium.sum())}; "
          f"{int(bad.sum())} rays differ; bit-identical in every field {np.all(got == ref, axis=1).mean():.5f}")
    assert np.array_equal(got[:, exact_cols], ref[:, exact_cols]), f"{int(bad.sum())} rays differ"
    surf = ~medium
    assert np.array_equal(got[surf][:, 1:5], ref[surf][:, 1:5]), "surface t/p not bit-identical"
    gm, rm, ray_m = got[medium], ref[medium], rays[medium]
    assert _ulp_close(gm[:, 1], rm[:, 1], 4).all()
    scale = np.abs(ray_m[:, 0:3]) + np.abs(rm[:, 1:2] * ray_m[:, 3:6])  # p = o + t*d may cancel
    assert (np.abs(gm[:, 2:5] - rm[:, 2:5]) <= 1e-13 * scale).all()
    du = np.abs(got[:, 8:10] - ref[:, 8:10])
    du[np.isnan(got[:, 8:10]) & np.isnan(ref[:, 8:10])] = 0
    assert np.all(du <= 4e-16), f"u/v max |d| {np.nanmax(du):.3g}"
    assert have == want


@pytest.mark.parametrize("name", ["frames", "media"])
def test_wide_walks_refuse_frame_and_media_worlds(gpu_ctx, name):
    """A world walked in the reference's order (media or instance frames) has 4-wide trees too: the mixed
    walk's, over its re-bounded subtrees. The plain 4-wide walk must not be started over them from the binary
    world root: RT_DEBUG_WIDE and RT_DEBUG_QNODE return RT_E_UNSUPPORTED (rt.h) before anything is launched,
    and the scene renders afterwards as before."""
    z = zoo_worlds.build(name)
    gpu_ctx.upload(z.scene)
    p = rtamd.make_params(32, 24, 2, 12, rtamd.RT_RNG_PHILOX, seed=7)
    before = gpu_ctx.render(z.camera, p, linear=True)
    rays, _ = _oracle_hits(name)
    for walk in (rtamd.RT_DEBUG_WIDE, rtamd.RT_DEBUG_QNODE):
        with pytest.raises(rtamd.RTError, match=r"\(-4\)") as e:
            gpu_ctx.closest_hits(rays[:256], 1e-4, np.inf, seed=3, flags=walk)
        print(f"zoo {name} walk {walk}: {e.value}")
    after = gpu_ctx.render(z.camera, p, linear=True)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1], equal_nan=True)


SEED = 77


def _light_points(z):
    """World-space centres of the lights tree's leaves."""
    nodes = z.scene.nodes
    ids = []

    def go(i):
        if nodes[i]["type"] == rtamd.RT_NODE_BVH:
            for ch in sorted({int(nodes[i]["a"]), int(nodes[i]["b"])}):
                go(ch)
        else:
            m = i
            while nodes[m]["type"] in (rtamd.RT_NODE_TRANSLATE, rtamd.RT_NODE_ROTATE):
                m = int(nodes[m]["a"])
            ids.append(int(nodes[m]["a"]))
    go(z.scene.desc.lights_root)
    return np.array([lf[1] for lf in z.leaves if lf[0] in ids]), len(ids)


@pytest.mark.parametrize("name", ["chains", "frames"])
def test_lights_tree_probes(gpu_ctx, name):
    """htblRandom / htblPdfValue (src/Lib.hs:673-724) on lights trees the named scenes do not have: makeBVH of
    three items (weights 1/3 and 2/3) and of four (two levels), with an XY rect and a translate(XZ rect) among
    the leaves, which neither function samples: direction (1, 0, 0), pdf 0. 384 records each, half of the pdf
    directions aimed at the lights. Philox words consumed exact, htbl_pdf bit-exact (sqrt and IEEE divisions
    only), htbl_random within 1e-12 relative (sin / cos of the sphere-light sample)."""
    z = zoo_worlds.build(name)
    rng = np.random.default_rng(31)
    n = 384
    lights, n_lights = _light_points(z)
    assert len(lights) == n_lights == {"chains": 3, "frames": 4}[name]
    org = np.array([lf[1] for lf in z.leaves])[rng.integers(0, len(z.leaves), n)] + rng.normal(0, 2.0, (n, 3))
    v = rng.normal(0, 1, (n, 3))
    aim = lights[rng.integers(0, len(lights), n // 2)] + rng.uniform(-0.5, 0.5, (n // 2, 3))
    v[: n // 2] = aim - org[: n // 2]
    pdf_in = np.concatenate([org, v], axis=1)
    ref_r = pyoracle.probe(z.scene, "htbl_random", org, seed=SEED)
    ref_p = pyoracle.probe(z.scene, "htbl_pdf", pdf_in, seed=SEED)
    unsampled = np.all(ref_r[:, :3] == [1.0, 0.0, 0.0], axis=1).mean()
    positive = (ref_p[:, 0] > 0).mean()
    assert unsampled >= 0.1 and positive >= 0.1, (unsampled, positive)  # (conditions on the inputs: the oracle alone)
    gpu_ctx.upload(z.scene)
    got_r = gpu_ctx.probe("htbl_random", org, seed=SEED)
    got_p = gpu_ctx.probe("htbl_pdf", pdf_in, seed=SEED)
    with np.errstate(invalid="ignore", divide="ignore"):
        close = np.isclose(got_r[:, :3], ref_r[:, :3], rtol=1e-12, atol=1e-300, equal_nan=True)
        rel = np.nanmax(np.abs(got_r[:, :3] - ref_r[:, :3]) / np.abs(ref_r[:, :3]))
    exact_p = (got_p == ref_p) | (np.isnan(got_p) & np.isnan(ref_p))
    print(f"zoo {name} lights tree: htbl_random (1,0,0) in {unsampled:.4f} of records, bit-exact "
          f"{np.all(got_r == ref_r, axis=1).mean():.4f}, max relative error {rel:.3g}; htbl_pdf positive in "
          f"{positive:.4f}, bit-exact {exact_p.all(axis=1).mean():.4f}")
    assert np.array_equal(got_r[:, 3], ref_r[:, 3]) and np.array_equal(got_p[:, 1], ref_p[:, 1]), "words consumed"
    assert exact_p.all(), f"{int((~exact_p.all(axis=1)).sum())} htbl_pdf records not bit-exact"
    assert close.all(), f"{int((~close.all(axis=1)).sum())} htbl_random records beyond 1e-12 relative"


@pytest.mark.parametrize("name", ["chains", "frames", "moving"])
def test_scatter_probe_every_material(gpu_ctx, name):
    """scatter (src/Lib.hs:822-885) for every material of the world, 48 records each: Lambertian with these
    lights trees' mixture (or the Unhittable lights' quirk), Metal, Dielectric, DiffuseLight. The contract of
    test_function_goldens.py: scattered / specular flags and Philox words exact, doubles within 1e-12 relative,
    at most 1 record in 500 flipped by a libm ulp."""
    z = zoo_worlds.build(name)
    rng = np.random.default_rng(37)
    centres = np.array([lf[1] for lf in z.leaves])
    recs = []
    for m in range(z.scene.desc.n_materials):
        n = 48
        o = centres[rng.integers(0, len(centres), n)] + rng.normal(0, 3.0, (n, 3))
        d = rng.normal(0, 1, (n, 3)) * rng.uniform(0.2, 3.0, (n, 1))
        tm = rng.uniform(0, 1, (n, 1))
        t = rng.uniform(0.01, 10.0, (n, 1))
        p = centres[rng.integers(0, len(centres), n)] + rng.normal(0, 1.0, (n, 3))
        nn = rng.normal(0, 1, (n, 3))
        nn /= np.linalg.norm(nn, axis=1, keepdims=True)
        nn[: n // 8] = np.eye(3)[rng.integers(0, 3, n // 8)] * rng.choice([-1.0, 1.0], (n // 8, 1))  # axis normals
        uv = rng.uniform(0, 1, (n, 2))
        ff = rng.integers(0, 2, (n, 1)).astype(np.float64)
        recs.append(np.concatenate([o, d, tm, t, p, nn, uv, ff, np.full((n, 1), float(m))], axis=1))
    x = np.concatenate(recs)
    ref = pyoracle.probe(z.scene, "scatter", x, seed=SEED, cam=z.camera)
    gpu_ctx.upload(z.scene)
    got = gpu_ctx.probe("scatter", x, seed=SEED, cam=z.camera)
    same_int = np.all(got[:, [0, 12, 13]] == ref[:, [0, 12, 13]], axis=1)
    exact = np.all((got == ref) | (np.isnan(got) & np.isnan(ref)), axis=1)
    with np.errstate(invalid="ignore"):
        close = np.all(np.isclose(got, ref, rtol=1e-12, atol=1e-300, equal_nan=True), axis=1)
    flips = ~(same_int & close)
    print(f"zoo {name} scatter: {len(ref)} records over {z.scene.desc.n_materials} materials, bit-exact "
          f"{exact.mean():.4f}, within 1e-12 {close.mean():.4f}, flips {int(flips.sum())}")
    assert flips.mean() <= 0.002, f"{int(flips.sum())} of {len(ref)} records differ beyond 1e-12 / in words"


def _background_bytes(z):
    return np.array([pyoracle.lib().oracle_scale_color(float(x)) for x in z.scene.desc.background], dtype=np.uint8)


@pytest.mark.parametrize("name", zoo_worlds.NAMES)
def test_images_tier_b(gpu_ctx, name, monkeypatch):
    """Tier B at 64x48, 8 spp, depth 12, with flags 0 and RT_FLAG_NAN_ZERO, against the oracle by the project's
    thresholds (>= 99.9 % of channels within 1e-3 on the displayed float, >= 99.9 % of bytes equal); then the
    same bytes from the one-sample-per-lane loop (RTAMD_REPLACE=0) and, for the world without frames or media
    in the Cornell variant, from the binary and the 4-wide replacement walks."""
    z = zoo_worlds.build(name)
    gpu_ctx.upload(z.scene)
    for flags in (0, rtamd.RT_FLAG_NAN_ZERO):
        p = rtamd.make_params(64, 48, 8, 12, rtamd.RT_RNG_PHILOX, seed=1024, flags=flags)
        rgb_o, lin_o, _, _ = pyoracle.render(z.scene, z.camera, p)
        if flags:
            lit = np.any(rgb_o != _background_bytes(z), axis=2).mean()
            assert lit >= 0.3, lit  # (the camera frames the world: the oracle alone)
        rgb_g, lin_g, _ = gpu_ctx.render(z.camera, p, linear=True)
        launch = gpu_ctx.last_launch()
        ok, eq, dmax = parity(lin_g, lin_o, rgb_g, rgb_o)
        print(f"zoo {name} tier B flags {flags} 64x48x8: channels within 1e-3 {ok:.6f}, bytes equal {eq:.6f}, "
              f"max |d| {dmax:.3g}, NaN channels {np.isnan(lin_o).mean():.4f}; launch variant {launch['variant']} "
              f"loop {launch['loop']}")
        assert ok >= 0.999, f"only {ok:.5f} of channels within 1e-3 (max |d| {dmax:.3g})"
        assert eq >= 0.999, f"only {eq:.5f} of bytes equal"
        assert launch["variant"] & (F_ALL | F_MIXW) == VARIANT[name] and launch["loop"] >= 1, launch
        monkeypatch.setenv("RTAMD_REPLACE", "0")
        rgb_s, lin_s, _ = gpu_ctx.render(z.camera, p, linear=True)
        assert gpu_ctx.last_launch()["loop"] == 0
        monkeypatch.delenv("RTAMD_REPLACE")
        assert np.array_equal(rgb_s, rgb_g) and np.array_equal(lin_s, lin_g, equal_nan=True)
        if name == "chains":
            for wide in ("0", "1"):
                monkeypatch.setenv("RTAMD_WIDE", wide)
                rgb_w, lin_w, _ = gpu_ctx.render(z.camera, p, linear=True)
                assert bool(gpu_ctx.last_launch()["variant"] & F_WIDE) == (wide == "1"), gpu_ctx.last_launch()
                assert np.array_equal(rgb_w, rgb_g) and np.array_equal(lin_w, lin_g, equal_nan=True)
            monkeypatch.delenv("RTAMD_WIDE")


@pytest.mark.parametrize("name", zoo_worlds.NAMES)
def test_images_tier_a(gpu_ctx, name):
    """Tier A (the reference's per-column SplitMix streams) at 32x24, 2 spp, depth 12. With
    RT_FLAG_SHARED_LIBM: bytes and every column's end generator equal the oracle's. With each side's own libm:
    the 1e-3 / 99.9 % contract and equal end generators in at least 95 % of columns
    (test_tier_a_rng_consuming_features' bound: a libm ulp may flip a branch of a column's serial stream)."""
    z = zoo_worlds.build(name)
    gpu_ctx.upload(z.scene)
    gens = rtamd.column_gens(z.g1, 32)
    p = rtamd.make_params(32, 24, 2, 12, rtamd.RT_RNG_EXACT, flags=rtamd.RT_FLAG_SHARED_LIBM)
    rgb_g, lin_g, gens_g = gpu_ctx.render(z.camera, p, gens, linear=True, want_gens=True)
    rgb_o, lin_o, gens_o, _ = pyoracle.render(z.scene, z.camera, p, col_gens=gens)
    ok, eq, dmax = parity(lin_g, lin_o, rgb_g, rgb_o)
    print(f"zoo {name} tier A, shared libm: bytes equal {eq:.6f}, channels within 1e-3 {ok:.6f}, max |d| {dmax:.3g}, "
          f"end generators equal {float((gens_g == gens_o).all(axis=1).mean()):.6f}")
    assert np.array_equal(gens_g, gens_o) and np.array_equal(rgb_g, rgb_o)
    p = rtamd.make_params(32, 24, 2, 12, rtamd.RT_RNG_EXACT)
    rgb_g, lin_g, gens_g = gpu_ctx.render(z.camera, p, gens, linear=True, want_gens=True)
    rgb_o, lin_o, gens_o, _ = pyoracle.render(z.scene, z.camera, p, col_gens=gens)
    ok, eq, dmax = parity(lin_g, lin_o, rgb_g, rgb_o)
    same_cols = (gens_g == gens_o).all(axis=1)
    print(f"zoo {name} tier A, device libm vs glibc: channels within 1e-3 {ok:.6f}, bytes equal {eq:.6f}, max |d| "
          f"{dmax:.3g}, end generators equal in {same_cols.mean():.6f} of columns")
    assert ok >= 0.999 and eq >= 0.999 and same_cols.mean() >= 0.95
