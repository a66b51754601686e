"""Specular-chain feature buffers on the device (include/rt.h rt_render_features_chain) against the first-hit pass
(max_bounces = 0, flags = 0), the CPU composition of tests/feature_chain_ref.py (fuzz-0 chains, bit for bit), and the
device's own render (fuzzy metals). Frames of 37x21 to 64x48 pixels at 5 to 8 samples."""
import ctypes as C

import numpy as np
import pytest
import torch

import feature_chain_ref as fcr
import feature_ref
import rtamd
from test_error_host import same_bits

pytestmark = pytest.mark.gpu

KNOBS = ("RTAMD_LDS", "RTAMD_LEAF_LDS", "RTAMD_PACKED_KEYS", "RTAMD_WAVES", "RTAMD_WIDE")
DIEL, METAL = rtamd.RT_CHAIN_DIELECTRIC, rtamd.RT_CHAIN_METAL
BOTH = DIEL | METAL
COUNTS = ("samples", "ended_surface", "ended_miss", "ended_cap", "bounces")


def _params(W, H, spp, flags=0, seed=1024, depth=1):
    return rtamd.make_params(W, H, spp, depth, rtamd.RT_RNG_PHILOX, seed=seed, flags=flags)


def _chain(max_bounces, flags, max_fuzz=0.0):
    return rtamd.make_feature_chain(max_bounces, bool(flags & DIEL), bool(flags & METAL), max_fuzz)


def _clear(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _first_hit_world(name):
    if name == "deep":
        scene, cam = feature_ref.deep_world()
        return scene, lambda W, H: cam
    return feature_ref.world(name)


# one world per walk form: mixed (chains, frames), recursive (deep), staged 4-wide (random_book_one)
@pytest.mark.parametrize("name,W,H,n,walk", [("chains", 64, 48, 8, 1), ("frames", 64, 48, 8, 1), ("deep", 40, 27, 3, 0),
                                             ("random_book_one", 48, 32, 6, 2)])
def test_zero_bounces_and_no_flags_are_the_first_hit_pass(gpu_ctx, monkeypatch, name, W, H, n, walk):
    """max_bounces = 0 with every flag, and flags = 0 with max_bounces = 8: rt_render_features' bytes, and no scatter
    followed. 1.0 * x is x and 0.0 + x is x."""
    _clear(monkeypatch)
    scene, cam = _first_hit_world(name)
    gpu_ctx.upload(scene)
    c, p = cam(W, H), _params(W, H, n)
    want = gpu_ctx.render_features(c, p)
    assert gpu_ctx.last_feature_launch()["loop"] == walk
    hits = int(want[..., 7].sum())
    for mb, flags in ((0, BOTH), (8, 0)):
        got = gpu_ctx.render_features(c, p, chain=_chain(mb, flags, 0.5))
        assert gpu_ctx.last_feature_launch()["loop"] == walk
        assert same_bits(got, want), (mb, flags)
        k = gpu_ctx.last_feature_chain()
        print(name, mb, flags, k)
        assert k["samples"] == W * H * n and k["bounces"] == 0 and k["ended_miss"] == W * H * n - hits
        assert k["ended_surface"] + k["ended_cap"] == hits and (flags != 0 or k["ended_cap"] == 0)


WORLDS = [("chains", 64, 48), ("moving", 64, 48), ("specular", 64, 48), ("chains", 37, 21)]
SETTINGS = [(mb, fl) for mb in (1, 8) for fl in (DIEL, METAL, BOTH)]
FLAG_NAMES = {DIEL: "dielectric", METAL: "metal", BOTH: "both"}


@pytest.mark.parametrize("max_bounces,flags", SETTINGS, ids=[f"{mb}_{FLAG_NAMES[fl]}" for mb, fl in SETTINGS])
@pytest.mark.parametrize("name,W,H", WORLDS, ids=[f"{w[0]}_{w[1]}x{w[2]}" for w in WORLDS])
def test_worlds_against_the_composition(gpu_ctx, monkeypatch, name, W, H, max_bounces, flags):
    """8 samples, max_fuzz 0. On every pixel not left out as undecided (at most 0.1 % of them, asserted first) the
    hits, normal and depth sums are the composition's bit for bit; so is the albedo where every texture is constant
    (elsewhere tests/test_gpu_features.py's rule: >= 99.9 % of pixels within 1e-12 * (|sum| + n), a checker or noise
    lookup may flip); the five counts are the composition's when no pixel is left out. The 37x21 frame's partial 8x8
    blocks put idle lanes next to lanes in chains."""
    _clear(monkeypatch)
    n = 8
    scene, cam = fcr.world(name)
    comp = fcr.composition(name, W, H, n, max_bounces, flags)
    want, keep, kc = comp.sums(), ~comp.left_out, comp.counts()
    print(f"{name} {W}x{H}x{n} max_bounces {max_bounces} flags {flags}: composition {kc}, "
          f"left out {int(comp.left_out.sum())} pixels")
    assert comp.left_out.mean() <= 0.001
    assert kc["bounces"] > 0  # (the case follows something)
    gpu_ctx.upload(scene)
    got = gpu_ctx.render_features(cam(W, H), _params(W, H, n), chain=_chain(max_bounces, flags))
    kd = gpu_ctx.last_feature_chain()
    d_alb = np.abs(got[..., 0:3] - want[..., 0:3])[keep]
    close = (d_alb <= 1e-12 * (np.abs(want[..., 0:3][keep]) + n)).all(axis=-1)
    print(f"device {kd}; hits equal {np.array_equal(got[..., 7][keep], want[..., 7][keep])}, normal equal "
          f"{same_bits(got[..., 3:6][keep], want[..., 3:6][keep])}, depth equal "
          f"{same_bits(got[..., 6][keep], want[..., 6][keep])}, albedo equal {(d_alb == 0).all(axis=-1).mean():.5f} "
          f"within tolerance {close.mean():.5f}")
    assert np.array_equal(got[..., 7][keep], want[..., 7][keep])
    assert same_bits(got[..., 3:6][keep], want[..., 3:6][keep])
    assert same_bits(got[..., 6][keep], want[..., 6][keep])
    if feature_ref.constant_textures(scene):
        assert same_bits(got[..., 0:3][keep], want[..., 0:3][keep])
    else:
        assert close.mean() >= 0.999
    if keep.all():
        assert kd == kc
    assert kd["samples"] == kd["ended_surface"] + kd["ended_miss"] + kd["ended_cap"]
    out = rtamd.resolve_features(got, n)
    assert np.isfinite(out["albedo"]).all() and np.isfinite(out["normal"]).all() and (out["depth"] > 0).all()


def test_fuzzy_metals_against_the_devices_own_render(gpu_ctx, monkeypatch):
    """max_fuzz = 0.5 on the specular-only world with Metal spheres of fuzz 0.1 and 0.3 added (numpy cannot restate
    the device's sincos bit for bit). Every material is followed, so a sample's chain ends in the background or at
    the cap, and a pixel whose hits sum is 0 saw only misses: its albedo sum / n is the average of thr * background
    over its samples, which is what rt_render computes at max_depth = max_bounces + 1, in another summation order:
    1e-12 relative. The other pixels are left out: no more of them than ended_cap + ended_surface, itself at most
    1 % of the samples."""
    _clear(monkeypatch)
    W, H, n, mb = 64, 48, 8, 16
    scene, cam = fcr.specular_world(True)
    gpu_ctx.upload(scene)
    got = gpu_ctx.render_features(cam, _params(W, H, n), chain=_chain(mb, BOTH, 0.5))
    k = gpu_ctx.last_feature_chain()
    _, lin, _ = gpu_ctx.render(cam, _params(W, H, n, depth=mb + 1), linear=True)
    keep = got[..., 7] == 0
    left = int((~keep).sum())
    print(f"fuzzy specular world: {k}, pixels left out {left}")
    assert k["ended_surface"] == 0 and k["bounces"] > 0.2 * k["samples"]
    assert left <= k["ended_cap"] + k["ended_surface"] <= 0.01 * k["samples"]
    assert k["ended_cap"] == int(got[..., 7].sum())
    mean = got[..., 0:3] / float(n)
    assert np.isfinite(lin[keep]).all()
    err = np.abs(mean - lin)[keep]
    print(f"max relative difference {float((err / lin[keep]).max()):.3g}")
    assert (err <= 1e-12 * lin[keep]).all()
    # the fuzz-0 chain differs: the fuzzy spheres end it
    plain = gpu_ctx.render_features(cam, _params(W, H, n), chain=_chain(mb, BOTH, 0.0))
    k0 = gpu_ctx.last_feature_chain()
    assert k0["ended_surface"] > 0 and not same_bits(plain, got)


def test_sample_ranges_and_accumulate(gpu_ctx, monkeypatch):
    """[0, 3) then [3, 8) accumulated, and 8 passes of one sample, are [0, 8) bit for bit; samples 3..7 alone are
    the composition of those samples."""
    _clear(monkeypatch)
    W, H, n, mb = 37, 21, 8, 8
    scene, cam = fcr.world("chains")
    comp = fcr.composition("chains", W, H, n, mb, BOTH)
    assert not comp.left_out.any()
    gpu_ctx.upload(scene)
    c, ch = cam(W, H), _chain(mb, BOTH)
    whole = gpu_ctx.render_features(c, _params(W, H, n), chain=ch)
    assert gpu_ctx.last_feature_chain() == comp.counts()
    part = gpu_ctx.render_features(c, _params(W, H, 1000), first_sample=0, n_samples=3, chain=ch)
    assert same_bits(part, comp.sums(0, 3))
    back = gpu_ctx.render_features(c, _params(W, H, 1), first_sample=3, n_samples=5, into=part, chain=ch)
    assert back is part and same_bits(part, whole)
    assert gpu_ctx.last_feature_chain()["samples"] == W * H * 5  # (the counts are the last pass's)
    one = None
    for s in range(n):
        one = gpu_ctx.render_features(c, _params(W, H, n), first_sample=s, n_samples=1, into=one, chain=ch)
    assert same_bits(one, whole)
    alone = gpu_ctx.render_features(c, _params(W, H, n), first_sample=3, n_samples=5, chain=ch)
    assert same_bits(alone, comp.sums(3, 5))


def _plan(scene, p, ch, cu_count):
    fn = rtamd.lib().rt_internal_features_chain_plan
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    info = rtamd.rt_launch_info()
    assert fn(C.addressof(scene.desc), 0, cu_count, C.addressof(p), C.addressof(ch), C.addressof(info), None) == 0
    return {k: getattr(info, k) for k, _ in rtamd.rt_launch_info._fields_}


def test_forms_give_the_same_bytes(gpu_ctx, monkeypatch):
    """random_book_one runs the staged 4-wide form at 3 waves per SIMD; at 4 and 2 waves, from global memory,
    without the staged leaf table, with the key / reference pairs, over the binary tree and under the reference
    cull the bytes and the counts are the same, and every launch is the one rt_internal_features_chain_plan returns
    without a device."""
    _clear(monkeypatch)
    W, H, n = 48, 32, 6
    scene, cam = feature_ref.world("random_book_one")
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    gpu_ctx.upload(scene)
    c, ch = cam(W, H), _chain(8, BOTH)
    base = gpu_ctx.render_features(c, _params(W, H, n), chain=ch)
    info, counts = gpu_ctx.last_feature_launch(), gpu_ctx.last_feature_chain()
    print("default:", info, counts)
    assert info["variant"] == 256 and info["loop"] == 2 and info["lds_staged"] == 1 and info["leaf_lds"] == 1
    assert info["waves"] == 3 and info["block"] == 768
    assert info == _plan(scene, _params(W, H, n), ch, cu)
    assert counts["bounces"] > 0 and not same_bits(base, gpu_ctx.render_features(c, _params(W, H, n)))
    cases = [({"RTAMD_WAVES": "4"}, 0, dict(loop=2, lds_staged=1, block=1024)),
             ({"RTAMD_WAVES": "2"}, 0, dict(loop=2, lds_staged=1, block=512)),
             ({"RTAMD_LDS": "0"}, 0, dict(loop=2, lds_staged=0, block=128)),
             ({"RTAMD_LEAF_LDS": "0"}, 0, dict(loop=2, lds_staged=1, leaf_lds=0)),
             ({"RTAMD_PACKED_KEYS": "0"}, 0, dict(loop=2, lds_staged=1, leaf_lds=1)),
             ({"RTAMD_PACKED_KEYS": "0", "RTAMD_WAVES": "4"}, 0, dict(loop=2, lds_staged=1, block=1024)),
             ({"RTAMD_PACKED_KEYS": "0", "RTAMD_LDS": "0"}, 0, dict(loop=2, lds_staged=0)),
             ({"RTAMD_WIDE": "0"}, 0, dict(loop=1, lds_staged=0)),
             ({}, rtamd.RT_FLAG_REFERENCE_CULL, dict(loop=1, lds_staged=0))]
    for env, flags, expect in cases:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        p = _params(W, H, n, flags=flags)
        got = gpu_ctx.render_features(c, p, chain=ch)
        info = gpu_ctx.last_feature_launch()
        print(env, flags, info)
        assert {k: info[k] for k in expect} == expect
        assert info == _plan(scene, p, ch, cu)
        assert same_bits(got, base), (env, flags)
        assert gpu_ctx.last_feature_chain() == counts
        for k in env:
            monkeypatch.delenv(k)


def test_async_pass_into_device_memory(gpu_ctx, monkeypatch):
    """rt_render_features_chain_async on a caller's stream into a caller's device buffer, accumulating onto it: the
    blocking call's bytes, and rt_last_feature_chain drains the stream."""
    _clear(monkeypatch)
    W, H, n = 37, 21, 5
    scene, cam = fcr.world("chains")
    gpu_ctx.upload(scene)
    c, p, ch = cam(W, H), _params(W, H, n), _chain(8, BOTH)
    want = gpu_ctx.render_features(c, p, chain=ch)
    d = torch.full((H, W, 8), 7.0, dtype=torch.float64, device="cuda:0")
    st = torch.cuda.Stream(device=0)
    with torch.cuda.stream(st):
        gpu_ctx.render_features_async(c, p, d.data_ptr(), 0, 2, accumulate=False, stream=st.cuda_stream, chain=ch)
        gpu_ctx.render_features_async(c, p, d.data_ptr(), 2, 3, accumulate=True, stream=st.cuda_stream, chain=ch)
    k = gpu_ctx.last_feature_chain()  # (no synchronize before it)
    assert k["samples"] == W * H * 3 and k["samples"] == k["ended_surface"] + k["ended_miss"] + k["ended_cap"]
    alone = gpu_ctx.render_features(c, p, first_sample=2, n_samples=3, chain=ch)
    assert gpu_ctx.last_feature_chain() == k
    st.synchronize()
    assert same_bits(d.cpu().numpy(), want) and not same_bits(alone, want)


def test_renders_and_first_hit_passes_around_a_chain_pass(gpu_ctx, monkeypatch):
    """A chain pass between two renders, and between two first-hit passes, leaves their bytes and what rt_last_launch
    reports unchanged."""
    _clear(monkeypatch)
    W, H = 48, 32
    scene, cam = feature_ref.world("random_book_one")
    gpu_ctx.upload(scene)
    c, p, ch = cam(W, H), _params(W, H, 6, depth=8), _chain(8, BOTH)
    rgb0, lin0, _ = gpu_ctx.render(c, p, linear=True)
    launch0 = gpu_ctx.last_launch()
    f0 = gpu_ctx.render_features(c, p)
    c0 = gpu_ctx.render_features(c, p, chain=ch)
    rgb1, lin1, _ = gpu_ctx.render(c, p, linear=True)
    f1 = gpu_ctx.render_features(c, p)
    c1 = gpu_ctx.render_features(c, p, chain=ch)
    assert np.array_equal(rgb0, rgb1) and same_bits(lin0, lin1)
    assert gpu_ctx.last_launch() == launch0
    assert same_bits(f0, f1) and same_bits(c0, c1) and not same_bits(f0, c0)


def test_fog_world_with_glass_spheres(gpu_ctx, monkeypatch):
    """feature_ref.fog_world (media, glass and fuzz-0.1 metal spheres; the mixed walk): a medium's keyed draw at the
    stream position the chain has reached. Not composed (feature_ref says why): every output is finite, the counts
    add up, and the chain does follow glass."""
    _clear(monkeypatch)
    W, H, n, mb = 64, 48, 8, 8
    scene, cam = feature_ref.fog_world()
    gpu_ctx.upload(scene)
    first = gpu_ctx.render_features(cam, _params(W, H, n))
    got = gpu_ctx.render_features(cam, _params(W, H, n), chain=_chain(mb, BOTH, 0.2))
    assert gpu_ctx.last_feature_launch()["loop"] == 1
    k = gpu_ctx.last_feature_chain()
    print("fog world:", k)
    assert np.isfinite(got).all() and (got[..., 6] >= 0).all()
    assert k["samples"] == W * H * n == k["ended_surface"] + k["ended_miss"] + k["ended_cap"]
    assert 0 < k["bounces"] <= k["samples"] * mb
    assert k["ended_miss"] == W * H * n - int(got[..., 7].sum())
    assert (got[..., 7] <= first[..., 7]).all() and (got[..., 6] >= first[..., 6] - 1e-9 * first[..., 6])[got[..., 7] == first[..., 7]].all()


def test_chain_sums_go_through_the_denoiser_unchanged(gpu_ctx, monkeypatch):
    """rt_denoise and a frame's denoised preview take chain sums as they take first-hit sums: rt_denoise_host of the
    same inputs, bit for bit."""
    _clear(monkeypatch)
    W, H, n = 64, 48, 8
    scene, cam = fcr.specular_world(True)
    gpu_ctx.upload(scene)
    p = _params(W, H, n, depth=10)
    feat = gpu_ctx.render_features(cam, p, chain=_chain(8, BOTH, 0.5))
    dp = rtamd.make_denoise_params(W, H, n, flags=rtamd.RT_DENOISE_DEMODULATE)
    with gpu_ctx.open_frame(cam, p, moments=True) as fr:
        fr.advance(fr.chunks_total)
        _, lin, _ = fr.resolve()
        se, _ = fr.error()
        got = fr.denoise(feat, n, flags=rtamd.RT_DENOISE_DEMODULATE)
    want = rtamd.denoise_host(dp, lin, se, feat)
    assert same_bits(got[1], want[1]) and np.array_equal(got[0], want[0])
    dev = gpu_ctx.denoise(dp, lin, se, feat)
    assert same_bits(dev[1], want[1]) and np.array_equal(dev[0], want[0])
    assert not same_bits(want[1], lin)
