"""The tier-B kernels' launch constants (rt_kernels.h LaunchConst: camera, table pointers, work geometry,
claim parameters) travel through a device copy that every workgroup stages in LDS. One world per kernel
form, each at 64x48, 4 spp, depth 8:

  * a context that rendered camera A renders camera B exactly as a fresh context does (a stale block would
    repeat A's camera or geometry);
  * the frame as 1 shard, as 3 shards, and through rt_frame_* in two steps gives the same bytes;
  * a second frame of the same size allocates nothing on the device.

The reference in each case is a fresh context rendering the same frame; the comparison is conftest.parity's
(tests/test_gpu_parity.py: 1e-3 on the displayed float and equal bytes for >= 99.9 % of channels), and on top
of it the bytes and the linear sums are required to be identical, as tier B defines them.
"""
import numpy as np
import pytest

import rtamd
from conftest import parity

pytestmark = pytest.mark.gpu

W, H, SPP, DEPTH = 64, 48, 4, 8
# world -> (camera, expected last_launch fields)
WORLDS = {
    "three_spheres": ("random_scene", dict(loop=1, lds_staged=1)),                  # binary walk, nodes in LDS
    "random_book_one": ("random_scene", dict(loop=2, lds_staged=1, leaf_lds=1)),    # 4-wide, leaves staged
    "stress_spheres": ("random_scene", dict(loop=2, lds_staged=0)),                 # 4-wide from global memory
    "cornell": ("cornell", dict(loop=1, lds_staged=1)),
    "cornell_smoke": ("cornell", dict(loop=1)),                                     # media: the full variant
}
_scenes, _fresh = {}, {}


def _global_kernel_param():
    """The smallest stress_spheres size of the ladder whose 64x48 frame no longer fits the LDS-staged kernel."""
    ctx = rtamd.Context(0)
    try:
        for param in (800, 1200, 1500, 2000, 3000, 5000, 20000):
            sc = rtamd.make_scene("stress_spheres", rtamd.randGen(1024), param=param)[0]
            ctx.upload(sc)
            ctx.render(rtamd.camera("random_scene", W, H), _params())
            if ctx.last_launch()["lds_staged"] == 0:
                return param, sc
    finally:
        ctx.close()
    raise AssertionError("no stress_spheres size of the ladder takes the global-memory kernel")


def _params(**kw):
    return rtamd.make_params(W, H, SPP, DEPTH, rtamd.RT_RNG_PHILOX, seed=11, **kw)


def _scene(name):
    if name not in _scenes:
        if name == "stress_spheres":
            _scenes[name] = _global_kernel_param()[1]
        else:
            _scenes[name] = rtamd.make_scene(name, rtamd.randGen(1024))[0]
    return _scenes[name]


def _cameras(name):
    """Camera A (the scene's own) and B (the same camera moved sideways and up by a tenth of its distance
    from the look-at plane's corner: another image of the same world)."""
    a = rtamd.camera(WORLDS[name][0], W, H)
    b = rtamd.camera(WORLDS[name][0], W, H)
    step = 0.1 * max(abs(a.origin[i] - a.llc[i]) for i in range(3))
    for i, d in enumerate((step, 0.5 * step, 0.0)):
        b.origin[i] += d
        b.llc[i] += d
    return a, b


def _fresh_render(name, which):
    """Camera `which` of the world rendered by a context that has rendered nothing else (computed once)."""
    key = (name, which)
    if key not in _fresh:
        ctx = rtamd.Context(0)
        try:
            ctx.upload(_scene(name))
            rgb, lin, _ = ctx.render(_cameras(name)[which], _params(), linear=True)
        finally:
            ctx.close()
        rgb.setflags(write=False)
        lin.setflags(write=False)
        _fresh[key] = (rgb, lin)
    return _fresh[key]


def _check(got, ref, what):
    ok, eq, dmax = parity(got[1], ref[1], got[0], ref[0])
    print(f"{what}: channels within 1e-3 {ok:.6f}, bytes equal {eq:.6f}, max |d| {dmax:.3g}")
    assert ok >= 0.999 and eq >= 0.999, what
    assert np.array_equal(got[0], ref[0]), f"{what}: bytes differ"
    assert np.array_equal(got[1], ref[1], equal_nan=True), f"{what}: linear sums differ"


@pytest.mark.parametrize("name", list(WORLDS))
def test_second_camera_equals_fresh_context(name):
    cam_a, cam_b = _cameras(name)
    ref_a, ref_b = _fresh_render(name, 0), _fresh_render(name, 1)
    assert not np.array_equal(ref_a[0], ref_b[0]), "the two cameras must give different images"
    ctx = rtamd.Context(0)
    try:
        ctx.upload(_scene(name))
        a = ctx.render(cam_a, _params(), linear=True)[:2]
        ll = ctx.last_launch()
        print(name, ll)
        for k, v in WORLDS[name][1].items():
            assert ll[k] == v, (k, ll)
        _check(a, ref_a, f"{name} camera A")
        b = ctx.render(cam_b, _params(), linear=True)[:2]
        assert ctx.frame_timing()["device_allocs"] == 0, "a second frame of one size allocates nothing"
        _check(b, ref_b, f"{name} camera B after A")
    finally:
        ctx.close()


@pytest.mark.parametrize("name", list(WORLDS))
def test_shards_and_frame_steps_give_the_same_bytes(gpu_ctx, name):
    import torch
    cam = _cameras(name)[1]
    ref = _fresh_render(name, 1)
    gpu_ctx.upload(_scene(name))
    one = gpu_ctx.render(cam, _params(), linear=True)[:2]
    _check(one, ref, f"{name} 1 shard")
    shards = 3
    geo = _params(shard_count=shards)
    slab = rtamd.shard_geometry(geo)[2]
    slabs = torch.zeros((shards, slab, 3), dtype=torch.uint8, device="cuda")
    for r in range(shards):
        gpu_ctx.render_shard_async(cam, _params(shard_rank=r, shard_count=shards), slabs[r].data_ptr())
    torch.cuda.synchronize()
    img = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    gpu_ctx.assemble_async(geo, slabs.data_ptr(), img.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(img.cpu().numpy(), ref[0]), f"{name}: 3 shards"
    with gpu_ctx.open_frame(cam, _params()) as fr:
        assert fr.chunks_total >= 2
        assert fr.advance(fr.chunks_total // 2) == fr.chunks_total // 2
        assert fr.advance(fr.chunks_total) == fr.chunks_total - fr.chunks_total // 2
        assert fr.complete
        rgb, lin, _ = fr.resolve()
    _check((rgb, lin), ref, f"{name} rt_frame in two steps")
