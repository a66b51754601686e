"""First-hit feature buffers on the device (include/rt.h rt_render_features) against the CPU composition of
tests/feature_ref.py: Philox streams, the UV pair and getRay restated in numpy, the oracle's closest hits and
texture values, and a left fold over the samples. Frames of 21x37 to 64x48 pixels at 3 to 8 samples."""
import ctypes as C

import numpy as np
import pytest
import torch

import feature_ref
import pyoracle
import rtamd

pytestmark = pytest.mark.gpu

F_WIDE, F_MIXW, F_UV, F_ALL = 256, 1024, 64, 63 | 512
KNOBS = ("RTAMD_LDS", "RTAMD_LEAF_LDS", "RTAMD_PACKED_KEYS", "RTAMD_WAVES", "RTAMD_WIDE")
# world, W, H, samples, the walk rt_last_feature_launch must report (2 4-wide, 1 mixed resumable)
WORLDS = [("chains", 64, 48, 8, 1), ("frames", 64, 48, 8, 1), ("moving", 64, 48, 8, 1),
          ("random_book_one", 48, 32, 6, 2), ("two_perlin_spheres", 48, 32, 4, 1), ("earth", 48, 32, 4, 1),
          ("chains", 37, 21, 5, 1)]  # (the last: a frame whose sides are no multiples of 8)
ALL_MATERIALS = {("chains", 64): 20, ("frames", 64): 26}


def _params(W, H, spp, flags=0, seed=1024, depth=1):
    return rtamd.make_params(W, H, spp, depth, rtamd.RT_RNG_PHILOX, seed=seed, flags=flags)


def _check_sums(got, want, n, scene, what):
    """hits, normal and depth sums equal (closest hits of surfaces are bit-identical by the existing contract, and
    the fold order is the same); albedo sums equal where every texture is constant, else >= 99.9 % of pixels
    within 1e-12 * (|sum| + n): sphere u, v agree to 4e-16, and a checker or raster lookup may flip."""
    d_alb = np.abs(got[..., 0:3] - want[..., 0:3])
    close = (d_alb <= 1e-12 * (np.abs(want[..., 0:3]) + n)).all(axis=-1)
    print(f"{what}: hits equal {np.array_equal(got[..., 7], want[..., 7])}, normal equal "
          f"{np.array_equal(got[..., 3:6], want[..., 3:6])}, depth equal {np.array_equal(got[..., 6], want[..., 6])}, "
          f"albedo equal {(d_alb == 0).all(axis=-1).mean():.5f} within tolerance {close.mean():.5f} "
          f"max |d| {d_alb.max():.3g}")
    assert np.array_equal(got[..., 7], want[..., 7])
    assert np.array_equal(got[..., 3:6], want[..., 3:6])
    assert np.array_equal(got[..., 6], want[..., 6])
    if feature_ref.constant_textures(scene):
        assert np.array_equal(got[..., 0:3], want[..., 0:3])
    else:
        assert close.mean() >= 0.999


@pytest.mark.parametrize("name,W,H,n,walk", WORLDS, ids=[f"{w[0]}_{w[1]}x{w[2]}" for w in WORLDS])
def test_worlds_against_the_composition(gpu_ctx, monkeypatch, name, W, H, n, walk):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    scene, cam = feature_ref.world(name)
    comp = feature_ref.composition(name, W, H, n)
    cov, partly = comp.coverage()
    print(f"{name} {W}x{H}x{n}: oracle coverage {cov:.3f}, partly covered {partly:.3f}, "
          f"materials hit {len(comp.hit_mats)} of {scene.desc.n_materials}")
    # conditions on the oracle's output alone (`moving` has a ground that fills the frame: no such condition)
    if name != "moving":
        assert 0.0 < cov < 1.0 and partly >= 0.01
    if (name, W) in ALL_MATERIALS:  # every material is some sample's hit
        assert 0.5 < cov < 0.65 and partly >= 0.02
        assert scene.desc.n_materials == ALL_MATERIALS[(name, W)] and len(comp.hit_mats) == scene.desc.n_materials
    gpu_ctx.upload(scene)
    got = gpu_ctx.render_features(cam(W, H), _params(W, H, n))
    info = gpu_ctx.last_feature_launch()
    assert got.shape == (H, W, 8) and info["loop"] == walk and info["work_items"] == ((W + 7) // 8) * ((H + 7) // 8)
    _check_sums(got, comp.sums(), n, scene, f"{name} {W}x{H}x{n}")
    # the guide images are finite and inside their ranges
    out = rtamd.resolve_features(got, n)
    assert np.isfinite(out["albedo"]).all() and np.isfinite(out["normal"]).all()
    assert ((out["coverage"] >= 0) & (out["coverage"] <= 1)).all()
    assert np.array_equal(np.isinf(out["depth"]), got[..., 7] == 0) and (out["depth"] > 0).all()


def test_sample_ranges(gpu_ctx, monkeypatch):
    """[0, 3) then [3, 5) accumulated is [0, 5) bit for bit, whatever `spp` says; samples 3 and 4 alone are the
    composition of samples 3 and 4."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    W, H = 37, 21
    scene, cam = feature_ref.world("chains")
    comp = feature_ref.composition("chains", W, H, 5)
    gpu_ctx.upload(scene)
    c = cam(W, H)
    whole = gpu_ctx.render_features(c, _params(W, H, 5))
    part = gpu_ctx.render_features(c, _params(W, H, 1000), first_sample=0, n_samples=3)
    assert np.array_equal(part, comp.sums(0, 3))
    back = gpu_ctx.render_features(c, _params(W, H, 1), first_sample=3, n_samples=2, into=part)
    assert back is part and np.array_equal(part, whole)
    alone = gpu_ctx.render_features(c, _params(W, H, 5), first_sample=3, n_samples=2)
    _check_sums(alone, comp.sums(3, 2), 2, scene, "chains samples 3, 4")
    with pytest.raises(rtamd.RTError):
        gpu_ctx.render_features(c, _params(W, H, 5), into=np.zeros((H, W, 8), dtype=np.float32))
    with pytest.raises(rtamd.RTError):
        gpu_ctx.render_features(c, _params(W, H, 5), into=np.zeros((W, H, 8)))


def test_async_pass_into_device_memory(gpu_ctx, monkeypatch):
    """rt_render_features_async on a caller's stream into a caller's device buffer, accumulating onto it: the
    blocking call's bytes."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    W, H, n = 37, 21, 5
    scene, cam = feature_ref.world("chains")
    gpu_ctx.upload(scene)
    c, p = cam(W, H), _params(W, H, n)
    want = gpu_ctx.render_features(c, p)
    d = torch.full((H, W, 8), 7.0, dtype=torch.float64, device="cuda:0")
    st = torch.cuda.Stream(device=0)
    with torch.cuda.stream(st):
        gpu_ctx.render_features_async(c, p, d.data_ptr(), 0, 2, accumulate=False, stream=st.cuda_stream)
        gpu_ctx.render_features_async(c, p, d.data_ptr(), 2, 3, accumulate=True, stream=st.cuda_stream)
    st.synchronize()
    assert np.array_equal(d.cpu().numpy(), want)


def test_media_world_coverage(gpu_ctx, monkeypatch):
    """The fog world (feature_ref.fog_world): the oracle's closest-hits entry draws a medium from another stream
    position, so albedo and depth are not composed; the hits are pinned by depth-1 renders instead, the oracle's
    and the context's own: hits == spp - rint(lin * spp) on every pixel (background 1, no emitter). The kernel form
    is the mixed walk, which `frames` checks field by field."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    W, H, n = 64, 48, 8
    scene, cam = feature_ref.fog_world()
    assert rtamd.prepare_scene(scene)["mixed_wide"] == 1
    assert tuple(scene.desc.background) == (1.0, 1.0, 1.0)
    p1 = _params(W, H, n, flags=rtamd.RT_FLAG_NAN_ZERO)
    _, lin_o, _, _ = pyoracle.render(scene, cam, p1)
    want = feature_ref.hits_from_render(lin_o, n, scene.desc.background)
    partly = float(((want > 0) & (want < n)).mean())
    print(f"fog world: oracle coverage {want.mean() / n:.3f}, partly covered {partly:.3f}")
    assert partly >= 0.10  # (on the oracle alone)
    gpu_ctx.upload(scene)
    got = gpu_ctx.render_features(cam, _params(W, H, n))
    info = gpu_ctx.last_feature_launch()
    assert info["loop"] == 1 and info["variant"] == F_ALL | F_UV | F_MIXW and info["wide_nodes"] > 0
    _, lin_g, _ = gpu_ctx.render(cam, p1, linear=True)
    own = feature_ref.hits_from_render(lin_g, n, scene.desc.background)
    print(f"fog world: hits equal the oracle's {(got[..., 7] == want).mean():.5f}, "
          f"the context's {(got[..., 7] == own).mean():.5f}")
    assert np.array_equal(got[..., 7], want)
    assert np.array_equal(got[..., 7], own)
    # a medium hit keeps the reference's fixed normal (1, 0, 0), and its albedo is the medium's texture
    assert np.isfinite(got).all() and (got[..., 6] >= 0).all()
    assert (np.abs(got[..., 3:6]).max(axis=-1) <= got[..., 7] + 1e-9).all()


def test_deep_frames_take_the_recursive_walk(gpu_ctx, monkeypatch):
    """Frames nested past RT_MAX_FRAMES: the recursive walk, against the composition (constant textures: every
    field equal)."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    W, H, n = 40, 27, 3
    scene, cam = feature_ref.deep_world()
    comp = feature_ref.Composition(scene, cam, W, H, 1024, 0, n)
    cov, partly = comp.coverage()
    print(f"deep world: oracle coverage {cov:.3f}, partly covered {partly:.3f}, materials hit {len(comp.hit_mats)}")
    assert partly >= 0.01 and len(comp.hit_mats) == 6
    gpu_ctx.upload(scene)
    got = gpu_ctx.render_features(cam, _params(W, H, n))
    assert gpu_ctx.last_feature_launch()["loop"] == 0
    _check_sums(got, comp.sums(), n, scene, "deep world")


def _plan(scene, p, cu_count):
    fn = rtamd.lib().rt_internal_features_plan
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    info = rtamd.rt_launch_info()
    assert fn(C.addressof(scene.desc), 0, cu_count, C.addressof(p), C.addressof(info), None) == 0
    return {k: getattr(info, k) for k, _ in rtamd.rt_launch_info._fields_}


def test_forms_give_the_same_bytes(gpu_ctx, monkeypatch):
    """random_book_one runs the staged 4-wide form; from global memory, without the staged leaf table, with the
    key / reference pairs, at 2 waves, over the binary tree and under the reference cull the bytes are the same,
    and every launch is the one rt_internal_features_plan returns without a device."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    W, H, n = 48, 32, 6
    scene, cam = feature_ref.world("random_book_one")
    comp = feature_ref.composition("random_book_one", W, H, n)
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    gpu_ctx.upload(scene)
    c = cam(W, H)
    base = gpu_ctx.render_features(c, _params(W, H, n))
    info = gpu_ctx.last_feature_launch()
    print("default:", info)
    assert info["variant"] == F_WIDE and info["loop"] == 2 and info["lds_staged"] == 1 and info["leaf_lds"] == 1
    assert info["waves"] == 4 and info["block"] == 1024
    assert info == _plan(scene, _params(W, H, n), cu)
    _check_sums(base, comp.sums(), n, scene, "random_book_one staged")
    cases = [({"RTAMD_LDS": "0"}, 0, dict(loop=2, lds_staged=0, block=128)),
             ({"RTAMD_LEAF_LDS": "0"}, 0, dict(loop=2, lds_staged=1, leaf_lds=0)),
             ({"RTAMD_PACKED_KEYS": "0"}, 0, dict(loop=2, lds_staged=1, leaf_lds=1)),
             ({"RTAMD_PACKED_KEYS": "0", "RTAMD_LDS": "0"}, 0, dict(loop=2, lds_staged=0)),
             ({"RTAMD_WAVES": "2"}, 0, dict(loop=2, lds_staged=1, block=512)),
             ({"RTAMD_WIDE": "0"}, 0, dict(loop=1, lds_staged=0)),
             ({}, rtamd.RT_FLAG_REFERENCE_CULL, dict(loop=1, lds_staged=0))]
    for env, flags, expect in cases:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        p = _params(W, H, n, flags=flags)
        got = gpu_ctx.render_features(c, p)
        info = gpu_ctx.last_feature_launch()
        print(env, flags, info)
        assert {k: info[k] for k in expect} == expect
        assert info == _plan(scene, p, cu)
        assert np.array_equal(got, base), (env, flags)
        for k in env:
            monkeypatch.delenv(k)


def test_renders_around_a_feature_pass(gpu_ctx, monkeypatch):
    """A feature pass between two renders leaves the renders' bytes and linear values, and what rt_last_launch
    reports, unchanged."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    W, H = 48, 32
    scene, cam = feature_ref.world("random_book_one")
    gpu_ctx.upload(scene)
    c, p = cam(W, H), _params(W, H, 6, depth=8)
    rgb0, lin0, _ = gpu_ctx.render(c, p, linear=True)
    launch0 = gpu_ctx.last_launch()
    f0 = gpu_ctx.render_features(c, p)
    rgb1, lin1, _ = gpu_ctx.render(c, p, linear=True)
    f1 = gpu_ctx.render_features(c, p)
    assert np.array_equal(rgb0, rgb1) and np.array_equal(lin0, lin1, equal_nan=True)
    assert gpu_ctx.last_launch() == launch0
    assert np.array_equal(f0, f1)
