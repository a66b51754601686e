"""The feature-guided denoiser on the GPU (include/rt.h, rt_denoise*): the device's image, bytes and counts are
rt_denoise_host's bit for bit on the smallest shapes at which the tile halo, the residue-class mapping and the
edge clipping can go wrong; the async call composes with the feature pass; a progressive frame's denoised
preview is the host filter of its resolve and error map and leaves the frame alone; NaN-quirk frames; renders
around a denoise; error codes; and the filter does reduce the error of a noisy Cornell preview.

Frame shape as in tests/test_gpu_frame_error.py: 96x64, spp 40, CH 1, 40 chunks (asserted)."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import rtamd
from test_denoise_host import ALL_FLAGS, DEMOD, FILL, counts, synthetic
from test_error_host import same_bits

pytestmark = pytest.mark.gpu

W, H, SPP, DEPTH = 96, 64, 40, 10
E_STATE, E_INVALID = r"\(-5\)", r"\(-1\)"
CAMERAS = {"cornell": "cornell", "random_book_one": "random_scene"}
_scenes = {}


def scene_of(name):
    if name not in _scenes:
        _scenes[name] = rtamd.make_scene(name, rtamd.randGen(1024))[0]
    return _scenes[name]


def setup(ctx, name, spp=SPP, seed=77, flags=0):
    assert rtamd.frame_chunking(W * H, SPP) == (1, 40)
    ctx.upload(scene_of(name))
    return rtamd.camera(CAMERAS[name], W, H), rtamd.make_params(W, H, spp, DEPTH, rtamd.RT_RNG_PHILOX, seed=seed,
                                                                flags=flags)


def same_result(got, want):
    """(rgb8, linear, stats) of two denoise calls: the same bits, bytes and counts."""
    return same_bits(got[1], want[1]) and np.array_equal(got[0], want[0]) and counts(got[2]) == counts(want[2])


@pytest.mark.parametrize("iterations", [1, 5])
@pytest.mark.parametrize("shape", [(1, 1), (37, 21), (65, 33)])
def test_device_equals_host_bit_for_bit(gpu_ctx, shape, iterations):
    """65x33 is one past a tile multiple (32x8) in both axes; five iterations reach stride 16, where an image of
    37x21 has more residue classes than pixels per class. Every flag combination, with and without se."""
    w, h = shape
    color, se, feat = synthetic(w, h, seed=7 * w + iterations)
    for e, flags in itertools.product((se, None), ALL_FLAGS):
        p = rtamd.make_denoise_params(w, h, 4, iterations=iterations, flags=flags)
        got = gpu_ctx.denoise(p, color, e, feat)
        assert same_result(got, rtamd.denoise_host(p, color, e, feat)), (flags, e is None)
        assert got[2]["kernel_ms"] > 0.0
        assert gpu_ctx.last_denoise()["launches"] == iterations + 2


def test_eight_iterations_on_a_wide_and_a_tall_strip(gpu_ctx):
    """Stride 128 on images one pixel high or wide: classes limited by min(s, W) and min(s, H)."""
    for w, h in ((300, 1), (1, 70)):
        color, se, feat = synthetic(w, h, seed=w + h)
        p = rtamd.make_denoise_params(w, h, 4, iterations=8, flags=FILL)
        assert same_result(gpu_ctx.denoise(p, color, se, feat), rtamd.denoise_host(p, color, se, feat))


def test_async_equals_the_blocking_call(gpu_ctx):
    """Device tensors on a caller's stream, the feature sums straight from render_features_async."""
    cam, rp = setup(gpu_ctx, "cornell")
    n = 6
    color, se, _ = synthetic(W, H, seed=2)
    d_feat = torch.zeros((H, W, 8), dtype=torch.float64, device="cuda:0")
    d_color, d_se = torch.from_numpy(color).to("cuda:0"), torch.from_numpy(se).to("cuda:0")
    d_out = torch.full((H, W, 3), -1.0, dtype=torch.float64, device="cuda:0")
    d_rgb = torch.full((H, W, 3), 9, dtype=torch.uint8, device="cuda:0")
    p = rtamd.make_denoise_params(W, H, n, flags=DEMOD | FILL)
    st = torch.cuda.Stream(device=0)
    with torch.cuda.stream(st):
        gpu_ctx.render_features_async(cam, rp, d_feat.data_ptr(), 0, n, stream=st.cuda_stream)
        gpu_ctx.denoise_async(p, d_color.data_ptr(), d_se.data_ptr(), d_feat.data_ptr(), d_out.data_ptr(),
                              d_rgb.data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    feat = gpu_ctx.render_features(cam, rp, n_samples=n)
    assert np.array_equal(d_feat.cpu().numpy(), feat)
    want = gpu_ctx.denoise(p, color, se, feat)
    assert same_bits(d_out.cpu().numpy(), want[1]) and np.array_equal(d_rgb.cpu().numpy(), want[0])
    assert same_result(want, rtamd.denoise_host(p, color, se, feat))
    # without se and without bytes
    d_out.fill_(-1.0)
    with torch.cuda.stream(st):
        gpu_ctx.denoise_async(p, d_color.data_ptr(), 0, d_feat.data_ptr(), d_out.data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    assert same_bits(d_out.cpu().numpy(), rtamd.denoise_host(p, color, None, feat)[1])


def test_tracked_frame_preview_is_the_host_filter_and_the_frame_is_left_alone(gpu_ctx):
    cam, rp = setup(gpu_ctx, "cornell")
    n = 8
    feat = gpu_ctx.render_features(cam, rp, n_samples=n)
    d_feat = torch.from_numpy(feat).to("cuda:0")
    kw = dict(flags=DEMOD)
    p = rtamd.make_denoise_params(W, H, n, **kw)
    keys = ("chunks_done", "samples_done", "nan_pixels", "bytes_changed")
    with gpu_ctx.open_frame(cam, rp, moments=True) as fr, gpu_ctx.open_frame(cam, rp, moments=True) as twin:
        for target in (10, 40):
            fr.advance(target - fr.chunks_done)
            twin.advance(target - twin.chunks_done)
            got = fr.denoise(d_feat, n, **kw)
            rgb, lin, st = twin.resolve()
            se, _ = twin.error()
            assert same_result(got, rtamd.denoise_host(p, lin, se, feat))
            assert same_result(fr.denoise(feat, n, **kw), got)  # (a host array of sums, and a repeat)
            # the denoised frame resolves as its untouched twin does, counts included
            rgb2, lin2, st2 = fr.resolve()
            assert np.array_equal(rgb2, rgb) and same_bits(lin2, lin) and [st2[k] for k in keys] == [st[k] for k in keys]
            assert same_bits(fr.error()[0], se)
        assert fr.complete and fr.save() == twin.save() and fr.checkpoint() == twin.checkpoint()
        assert not same_bits(got[1], lin)  # (the filter did something)
    # one chunk: no error map yet, the filter runs without se; an untracked frame never has one
    with gpu_ctx.open_frame(cam, rp, moments=True) as fr, gpu_ctx.open_frame(cam, rp) as plain:
        fr.advance(1)
        plain.advance(12)
        for f in (fr, plain):
            assert same_result(f.denoise(d_feat, n, **kw), rtamd.denoise_host(p, f.resolve()[1], None, feat))


def test_nan_quirk_frame(gpu_ctx):
    """random_book_one: the Lambertian-mixture quirk leaves NaN pixels. Without RT_DENOISE_FILL they stay, with it
    they are filled; either way the host's bytes and counts, and no finite pixel becomes non-finite."""
    cam, rp = setup(gpu_ctx, "random_book_one")
    _, lin, _ = gpu_ctx.render(cam, rp, linear=True)
    bad = ~np.isfinite(lin).all(-1)
    assert 0 < bad.sum() < W * H
    n = 4
    feat = gpu_ctx.render_features(cam, rp, n_samples=n)
    for flags in (0, FILL, DEMOD, DEMOD | FILL):
        p = rtamd.make_denoise_params(W, H, n, flags=flags)
        got = gpu_ctx.denoise(p, lin, None, feat)
        assert same_result(got, rtamd.denoise_host(p, lin, None, feat))
        bad_out = ~np.isfinite(got[1]).all(-1)
        assert not (bad_out & ~bad).any()
        assert got[2]["invalid_in"] == int(bad.sum()) and got[2]["invalid_out"] == int(bad_out.sum())
        if flags & FILL:
            assert got[2]["filled"] == int((bad & ~bad_out).sum()) > 0
        else:
            assert np.array_equal(bad_out, bad) and got[2]["filled"] == 0 and same_bits(got[1][bad], lin[bad])


def test_renders_around_a_denoise_are_unchanged_and_a_repeat_allocates_nothing():
    ctx = rtamd.Context(0)  # (its own ctx: the first denoise of a size must allocate, the second must not)
    try:
        cam, rp = setup(ctx, "cornell", spp=8)
        before = ctx.render(cam, rp, linear=True)
        feat = ctx.render_features(cam, rp, n_samples=4)
        p = rtamd.make_denoise_params(W, H, 4, flags=DEMOD)
        first = ctx.denoise(p, before[1], None, feat)
        assert ctx.last_denoise()["device_allocs"] > 0
        after = ctx.render(cam, rp, linear=True)
        assert np.array_equal(after[0], before[0]) and same_bits(after[1], before[1])
        second = ctx.denoise(p, before[1], None, feat)
        info = ctx.last_denoise()
        assert info["device_allocs"] == 0 and info["launches"] == 7 and 0 < info["lds_bytes"] <= 64 * 1024
        assert same_result(second, first)
        assert ctx.frame_timing()["device_allocs"] == 0  # (the second render of one size, as before)
        with ctx.open_frame(cam, rp) as fr:
            fr.advance(4)
            fr.denoise(feat, 4)
            fr.denoise(feat, 4)
            assert ctx.last_denoise()["device_allocs"] == 0
    finally:
        ctx.close()


def test_error_codes(gpu_ctx):
    cam, rp = setup(gpu_ctx, "cornell")
    color, se, feat = synthetic(W, H, seed=9, sprinkle=False)
    d_feat = torch.from_numpy(feat).to("cuda:0")
    good = rtamd.make_denoise_params(W, H, 4)
    for change in (dict(iterations=0), dict(iterations=9), dict(feature_samples=0), dict(flags=8),
                   dict(sigma_color=0.0), dict(sigma_depth=float("nan")), dict(color_floor=float("inf"))):
        p = rtamd.make_denoise_params(W, H, 4)
        for k, v in change.items():
            setattr(p, k, v)
        with pytest.raises(rtamd.RTError, match=E_INVALID):
            gpu_ctx.denoise(p, color, se, feat)
        with pytest.raises(rtamd.RTError, match=E_INVALID):
            gpu_ctx.denoise_async(p, d_feat.data_ptr(), 0, d_feat.data_ptr(), d_feat.data_ptr())
    with pytest.raises(rtamd.RTError, match=E_INVALID):
        gpu_ctx.denoise_async(good, 0, 0, d_feat.data_ptr(), d_feat.data_ptr())
    with gpu_ctx.open_frame(cam, rp) as fr:
        with pytest.raises(rtamd.RTError, match=E_STATE):  # (no chunk rendered yet)
            fr.denoise(d_feat, 4)
        fr.advance(1)
        with pytest.raises(rtamd.RTError, match=E_INVALID):
            fr.denoise(d_feat, 4, iterations=9)
        assert rtamd.lib().rt_frame_denoise(fr._h, C.byref(good), None, None, None, None) == rtamd.RT_E_INVALID
        other = rtamd.make_denoise_params(W + 1, H, 4)
        assert rtamd.lib().rt_frame_denoise(fr._h, C.byref(other), C.c_void_p(d_feat.data_ptr()), None, None,
                                            None) == rtamd.RT_E_INVALID
        assert fr.denoise(d_feat, 4, rgb=False, linear=False)[2]["pixels"] == W * H  # (stats alone)
    shard = rtamd.make_params(W, H, SPP, DEPTH, rtamd.RT_RNG_PHILOX, seed=77, shard_rank=0, shard_count=2)
    with gpu_ctx.open_shard_frame(cam, shard) as fr:
        fr.advance(2)
        with pytest.raises(rtamd.RTError, match=E_STATE) as err:
            fr.denoise(d_feat, 4)
        assert "halo" in str(err.value)
    # a ctx without a scene denoises; only the frame call needs one (and cannot exist without it)
    bare = rtamd.Context(0)
    try:
        assert same_result(bare.denoise(good, color, se, feat), rtamd.denoise_host(good, color, se, feat))
    finally:
        bare.close()


def test_denoised_preview_is_closer_to_a_converged_render_than_the_raw_one(gpu_ctx):
    """Cornell 96x64: the RMSE against a 2000-spp render (same camera, another seed) of the denoised 40-spp preview
    (default parameters, RT_DENOISE_DEMODULATE, the frame's own error map, the feature sums of the same 40 samples)
    is below the raw 40-spp image's. Over the pixels finite in all three images: at least 90 % of the frame
    (the CPU oracle renders Cornell at this shape without a NaN pixel at 40 and at 200 spp, so the renders need no
    RT_FLAG_NAN_ZERO)."""
    cam, rp = setup(gpu_ctx, "cornell")
    ref = gpu_ctx.render(cam, rtamd.make_params(W, H, 2000, DEPTH, rtamd.RT_RNG_PHILOX, seed=5), linear=True)[1]
    feat = gpu_ctx.render_features(cam, rp, n_samples=SPP)
    with gpu_ctx.open_frame(cam, rp, moments=True) as fr:
        fr.advance(fr.chunks_total)
        raw = fr.resolve()[1]
        den = fr.denoise(feat, SPP, flags=DEMOD)[1]
    ok = np.isfinite(ref).all(-1) & np.isfinite(raw).all(-1) & np.isfinite(den).all(-1)
    assert ok.mean() >= 0.9
    rmse = lambda a: float(np.sqrt(((a - ref)[ok] ** 2).mean()))
    print(f"rmse raw {rmse(raw):.5f} denoised {rmse(den):.5f} over {ok.mean():.3f} of the frame")
    assert rmse(den) < rmse(raw)
