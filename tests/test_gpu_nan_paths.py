"""Tier B ends a path once its throughput is NaN in all three channels (rt_kernels.h: philox_loop2 and
philox_loop). The sample's colour is decided there — thr * background, thr * emitted and
thr * 0 are all (NaN, NaN, NaN) — and a tier-B sample draws from its own (pixel, sample) stream, so the
image is what the full paths give: checked per sample against the oracle (which traces every path to its
end), by the counting build's segments per sample, and on chunk sums through the progressive frames.

NaNs are compared by mask (np.isnan, equal_nan=True), never by bit pattern."""
import os

import numpy as np
import pytest

import pyoracle
import rtamd
from conftest import parity

pytestmark = pytest.mark.gpu

SEED, DEPTH = 1024, 50
CAMERAS = {"random_book_one": "random_scene", "three_spheres": "random_scene", "next_week_final": "next_week",
           "cornell": "cornell", "cornell_smoke": "cornell"}
_scenes, _oracle = {}, {}


def _frames_scene(depth):
    """Ground + a BVH of small spheres under `depth` alternating Translate / Rotate frames, as
    tests/test_gpu_scenes.py::test_nested_frames builds it (6 deep: more than RT_MAX_FRAMES, so the
    per-sample loop renders it)."""
    b = rtamd.Builder(rtamd.randGen(77))
    white = b.lambertian(b.constantColor(0.73, 0.73, 0.73))
    red = b.lambertian(b.constantColor(0.65, 0.05, 0.05))
    glass = b.dielectric(1.5)
    metal = b.metal(b.constantColor(0.8, 0.8, 0.9), 0.1)
    rng = np.random.default_rng(3)
    items = []
    for i in range(24):
        c = (float(rng.uniform(-2, 2)), float(rng.uniform(0.2, 2)), float(rng.uniform(-2, 2)))
        items.append(b.sphere(c, float(rng.uniform(0.1, 0.4)), [white, red, glass, metal][i % 4]))
    inner = b.makeBVH((0.0, 1.0), items)
    for k in range(depth):
        inner = b.translate((0.3, 0.0, -0.2), inner) if k % 2 == 0 else b.rotate(rtamd.YAxis, 17.0, inner)
    ground = b.sphere((0.0, -1000.0, 0.0), 1000.0, white)
    return b.finish(b.makeBVH((0.0, 1.0), [ground, inner]), -1, (0.7, 0.8, 1.0))


def scene_of(name):
    if name not in _scenes:
        if name == "frames6":
            _scenes[name] = _frames_scene(6)
        else:
            earth = None
            if name == "next_week_final":
                earth = np.load(os.path.join(os.path.dirname(__file__), "golden", "earthmap_rgb8.npz"))["rgb"]
            _scenes[name] = rtamd.make_scene(name, rtamd.randGen(1024), earth=earth)[0]
    return _scenes[name]


def setup(ctx, name, w, h, spp, flags=0):
    ctx.upload(scene_of(name))
    cam = rtamd.camera(CAMERAS.get(name, "random_scene"), w, h)
    return cam, rtamd.make_params(w, h, spp, DEPTH, rtamd.RT_RNG_PHILOX, seed=SEED, flags=flags)


def oracle(name, cam, p, counters=False):
    """The oracle's render of (scene, params), computed once and left unchanged."""
    key = (name, p.width, p.height, p.spp, p.flags)
    if key not in _oracle:
        rgb, lin, _, cnt = pyoracle.render(scene_of(name), cam, p, counters=True)
        rgb.setflags(write=False)
        lin.setflags(write=False)
        _oracle[key] = (rgb, lin, cnt)
    return _oracle[key]


# scene, W, H, the loop that renders it (rt_launch_info.loop: 2 the 4-wide replacement loop, 1 the binary /
# mixed replacement loop, 0 the per-sample loop), the least share of NaN pixels (None: not asserted)
IDENTITY = [
    ("random_book_one", 96, 64, 2, 0.05),   # 4-wide walk, spheres kernel; the CPU figure is 14 %
    ("three_spheres", 64, 32, 1, None),     # binary walk
    ("next_week_final", 64, 64, 1, 0.05),   # mixed walk, media; the CPU figure is 25 %
    ("cornell", 64, 64, 1, None),           # lights: the quirk's 0 / 0 does not occur, nothing is cut
    ("frames6", 64, 40, 0, None),           # frames nested 6 deep: the per-sample loop
]


@pytest.mark.parametrize("name, w, h, loop, min_nan", IDENTITY, ids=[c[0] for c in IDENTITY])
def test_each_sample_equals_the_oracles(gpu_ctx, name, w, h, loop, min_nan):
    """At 1 spp a pixel is one sample: its NaN mask equals the oracle's and its finite channels agree
    (the parity helper's thresholds: 0.999 of the channels within 1e-3 on the displayed value, a channel
    that is NaN on one side only counts as a miss; 0.999 of the bytes equal)."""
    cam, p = setup(gpu_ctx, name, w, h, 1)
    rgb, lin, _ = gpu_ctx.render(cam, p, linear=True)
    assert gpu_ctx.last_launch()["loop"] == loop
    rgb_o, lin_o, _ = oracle(name, cam, p)
    ok, eq, dmax = parity(lin, lin_o, rgb, rgb_o)
    masks = float((np.isnan(lin) == np.isnan(lin_o)).mean())
    nan_px = float(np.isnan(lin).all(axis=2).mean())
    part_px = float((np.isnan(lin).any(axis=2) & ~np.isnan(lin).all(axis=2)).mean())
    print(f"{name} {w}x{h}x1: within 1e-3 {ok:.6f}, bytes equal {eq:.6f}, max |d| {dmax:.3g}, NaN masks equal "
          f"{masks:.6f}, NaN pixels {nan_px:.4f} (oracle {float(np.isnan(lin_o).all(axis=2).mean()):.4f}), "
          f"partly NaN {part_px:.4f}")
    assert ok >= 0.999 and eq >= 0.999 and masks >= 0.999, (ok, eq, masks, dmax)
    if min_nan is not None:
        assert nan_px > min_nan, nan_px


# Segments per sample: the counting build's `segments / samples` over the oracle's `world_queries /
# samples` for the same parameters. (oracle segments / sample, after the cut, ratio)
RATIOS = [
    ("random_book_one", 96, 64, 8, (3.093, 2.322, 0.751)),
    ("next_week_final", 64, 64, 4, (5.687, 3.754, 0.660)),
    ("cornell_smoke", 64, 64, 4, (2.966, 2.966, 1.000)),
]


@pytest.mark.parametrize("name, w, h, spp, expect", RATIOS, ids=[c[0] for c in RATIOS])
def test_paths_end_where_the_throughput_goes_nan(gpu_ctx, name, w, h, spp, expect):
    """The cut happens, and only where it should: the device traces `ratio` times the oracle's segments,
    within +-0.01 (the slack covers the rare path that flips on a libm ulp between OCML and glibc; the
    samples are the same on both sides), and every sample is still started and counted.

    The expected figures come from an instrumented copy of oracle/oracle.c (not committed): tier-B
    streams, seed 1024, depth 50, this scene, camera and frame; it flags a sample when scatteringPdf / pdf
    is NaN at a non-specular scatter and counts the world queries traced after that ("after the cut" =
    world_queries minus those, per sample). To regenerate them, add the flag and the second counter to
    ray_color's scatter branch in such a copy and run it with the parameters below. A world with lights
    (cornell_smoke) never takes the quirk's 0 / 0: nothing is cut."""
    cam, p = setup(gpu_ctx, name, w, h, spp)
    work = gpu_ctx.render_work(cam, p)
    _, _, cnt = oracle(name, cam, p)
    assert work["samples"] == w * h * spp and cnt["samples"] == w * h * spp
    dev = work["segments"] / work["samples"]
    ref = cnt["world_queries"] / cnt["samples"]
    print(f"{name} {w}x{h}x{spp}: device segments / sample {dev:.4f}, oracle {ref:.4f}, ratio {dev / ref:.4f} "
          f"(expected {expect[1]} / {expect[0]} = {expect[2]})")
    assert abs(dev / ref - expect[2]) <= 0.01, (dev, ref, dev / ref)


S = (48, 32, 24)  # 24 chunks of one sample each


def test_progressive_frame_equals_rt_render(gpu_ctx):
    """Chunk sums: a progressive frame advanced in 3 steps ends equal to rt_render bit for bit (NaNs by
    mask), on a frame where a seventh of the samples is cut."""
    w, h, spp = S
    assert rtamd.frame_chunking(w * h, spp) == (1, 24)
    cam, p = setup(gpu_ctx, "random_book_one", w, h, spp)
    rgb, lin, _ = gpu_ctx.render(cam, p, linear=True)
    assert np.isnan(lin).any()
    with gpu_ctx.open_frame(cam, p) as fr:
        assert [fr.advance(3), fr.advance(7), fr.advance(1000)] == [3, 7, 14] and fr.complete
        rgb_f, lin_f, st = fr.resolve()
    assert st["samples_done"] == spp
    assert np.array_equal(rgb_f, rgb) and np.array_equal(lin_f, lin, equal_nan=True)


def test_nan_zero_adds_zero_for_a_cut_sample(gpu_ctx):
    """RT_FLAG_NAN_ZERO: a cut sample's thr * 0 is NaN in every channel and adds 0, as the full path's
    colour would. Here a chunk is one sample, so the flagged image is what nan_to_num of the unflagged
    chunk sums gives: no NaN is left, a channel with no NaN sample is bit for bit the unflagged one, the
    whole image is the oracle's under the same flag (which traces the full paths), and a progressive
    frame in 3 steps equals rt_render."""
    w, h, spp = S
    assert rtamd.frame_chunking(w * h, spp) == (1, 24)
    cam, p = setup(gpu_ctx, "random_book_one", w, h, spp)
    _, lin, _ = gpu_ctx.render(cam, p, linear=True)
    cam, pz = setup(gpu_ctx, "random_book_one", w, h, spp, flags=rtamd.RT_FLAG_NAN_ZERO)
    rgb_z, lin_z, _ = gpu_ctx.render(cam, pz, linear=True)
    finite = ~np.isnan(lin)
    assert not np.isnan(lin_z).any() and 0.05 < 1.0 - finite.mean()
    assert np.array_equal(lin_z[finite], lin[finite])
    rgb_o, lin_o, _ = oracle("random_book_one", cam, pz)
    ok, eq, dmax = parity(lin_z, lin_o, rgb_z, rgb_o)
    print(f"NaN-zero 48x32x24 vs the oracle: within 1e-3 {ok:.6f}, bytes equal {eq:.6f}, max |d| {dmax:.3g}")
    assert ok >= 0.999 and eq >= 0.999, (ok, eq, dmax)
    with gpu_ctx.open_frame(cam, pz) as fr:
        assert [fr.advance(3), fr.advance(7), fr.advance(1000)] == [3, 7, 14]
        rgb_f, lin_f, _ = fr.resolve()
    assert np.array_equal(rgb_f, rgb_z) and np.array_equal(lin_f, lin_z)
