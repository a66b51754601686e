"""Sharded feature passes on the device (include/rt.h rt_render_features_shard_async, rt_assemble_records_async). The
reference of every comparison is the image-order pass of the same context (`Context.render_features`) and
rtamd.shard_pixel_map; a slab pass is never compared with another slab pass. Comparisons are of bytes
(view(np.uint64): -0.0 and NaN count) and every slab starts from the sentinel 7.0, which must survive in the padding.

Frames: 37x21 (both sides no multiple of 8; 15 tiles of 8, which 2, 4 or 8 shards do not divide; 6 overhanging tiles
of 16, of which 8 shards leave two empty), 64x48 at tile 64 (one tile, three shards, two of them empty), 48x32 for the
LDS-staged 4-wide form, 40x27 for the recursive walk."""
import numpy as np
import pytest
import torch

import feature_chain_ref as fcr
import feature_ref
import rtamd

pytestmark = pytest.mark.gpu

KNOBS = ("RTAMD_LDS", "RTAMD_LEAF_LDS", "RTAMD_PACKED_KEYS", "RTAMD_WAVES", "RTAMD_WIDE")
GEOMETRIES = [(1, 8), (2, 8), (4, 8), (3, 16), (8, 16), (3, 64), (16, 8)]  # (shards, tile)
SENTINEL = 7.0
COUNTS = ("samples", "ended_surface", "ended_miss", "ended_cap", "bounces")
BOTH = rtamd.RT_CHAIN_DIELECTRIC | rtamd.RT_CHAIN_METAL


def _clear(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _params(W, H, spp, tile=8, rank=0, shards=1, flags=0, seed=1024, depth=1):
    return rtamd.make_params(W, H, spp, depth, rtamd.RT_RNG_PHILOX, seed=seed, flags=flags, tile=tile, shard_rank=rank,
                             shard_count=shards)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _world(name):
    if name == "fog":
        scene, cam = feature_ref.fog_world()
        return scene, lambda W, H: cam
    if name == "deep":
        scene, cam = feature_ref.deep_world()
        return scene, lambda W, H: cam
    if name == "specular":
        return fcr.world(name)
    return feature_ref.world(name)


def _slab_pass(ctx, cam, W, H, n, shards, tile, chain=None, first=0, flags=0, slabs=None, accumulate=False, stream=0):
    """Every shard's slab pass into one [shards, slab, 8] tensor that starts from the sentinel (or `slabs`); returns
    the tensor, what rt_last_feature_launch reported per shard and, with a chain, the per-shard counts."""
    slab = rtamd.shard_geometry(_params(W, H, n, tile, 0, shards))[2]
    if slabs is None:
        slabs = torch.full((shards, slab, 8), SENTINEL, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
    infos, counts = [], []
    for r in range(shards):
        p = _params(W, H, n, tile, r, shards, flags=flags)
        ctx.render_features_shard_async(cam, p, slabs[r].data_ptr(), first, n, accumulate=accumulate, stream=stream,
                                        chain=chain)
        infos.append(ctx.last_feature_launch())
        if chain is not None:
            counts.append(ctx.last_feature_chain())
    torch.cuda.synchronize()
    return slabs, infos, counts


def _check_slabs(ctx, slabs, want, W, H, n, shards, tile, what):
    """Owned slots hold the image-order pass's pixels, the padding the sentinel, and the merge gives the array."""
    host = slabs.cpu().numpy()
    flat = _bits(want).reshape(W * H, 8)
    sentinel = np.float64(SENTINEL).view(np.uint64)
    owned = 0
    for r in range(shards):
        m = rtamd.shard_pixel_map(_params(W, H, n, tile, r, shards))
        ok = m >= 0
        owned += int(ok.sum())
        assert np.array_equal(_bits(host[r])[ok], flat[m[ok]]), (what, "owned slots of shard", r)
        assert (_bits(host[r])[~ok] == sentinel).all(), (what, "padding of shard", r)
    assert owned == W * H
    img = torch.full((H, W, 8), -1.0, dtype=torch.float64, device="cuda:0")
    ctx.assemble_records_async(_params(W, H, n, tile, 0, shards), slabs.data_ptr(), img.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(_bits(img.cpu().numpy()), _bits(want)), (what, "assembled")
    assert np.array_equal(_bits(rtamd.assemble_records_host(host, _params(W, H, n, tile, 0, shards))), _bits(want))


def _work_items(W, H, shards, tile, r):
    tiles = -(-W // tile) * -(-H // tile)
    return len(range(r, tiles, shards)) * (tile // 8) ** 2


FIRST_HIT = [("chains", 37, 21, 5, 1), ("random_book_one", 48, 32, 6, 2), ("deep", 40, 27, 3, 0), ("fog", 64, 48, 4, 1)]


@pytest.mark.parametrize("name,W,H,n,walk", FIRST_HIT, ids=[w[0] for w in FIRST_HIT])
def test_first_hit_slabs_are_the_image_order_pass(gpu_ctx, monkeypatch, name, W, H, n, walk):
    _clear(monkeypatch)
    scene, cam = _world(name)
    gpu_ctx.upload(scene)
    c = cam(W, H)
    want = gpu_ctx.render_features(c, _params(W, H, n))
    base = gpu_ctx.last_feature_launch()
    assert base["loop"] == walk
    for shards, tile in GEOMETRIES:
        slabs, infos, _ = _slab_pass(gpu_ctx, c, W, H, n, shards, tile)
        _check_slabs(gpu_ctx, slabs, want, W, H, n, shards, tile, (name, shards, tile))
        for r, info in enumerate(infos):
            assert info["loop"] == walk and info["work_items"] == _work_items(W, H, shards, tile, r), (shards, tile, r, info)
            for k in ("variant", "lds_staged", "leaf_lds", "waves", "block", "dyn_lds_bytes", "wide_nodes"):
                assert info[k] == base[k], (k, shards, tile, r)
        if (shards, tile) == (1, 8):
            assert infos[0]["work_items"] == base["work_items"]
        if (W, H) == (37, 21) and (shards, tile) in ((8, 16), (3, 64), (16, 8)):
            assert infos[-1]["work_items"] == 0  # (a shard that owns no tile: RT_OK, nothing written)
        if (W, H) == (64, 48) and (shards, tile) == (3, 64):  # (one tile, three shards, two of them empty; the
            assert [i["work_items"] for i in infos] == [64, 0, 0]  # tile's 16 blocks below the image are claimed and idle)


def test_chain_slabs_and_counts(gpu_ctx, monkeypatch):
    """The specular world at 48x32, 8 bounces, both flags, 3 shards of tile 16: the chain pass's bytes, and the five
    counts added over the shards are its counts. max_bounces = 0 gives the first-hit pass's bytes."""
    _clear(monkeypatch)
    W, H, n, shards, tile = 48, 32, 5, 3, 16
    scene, cam = _world("specular")
    gpu_ctx.upload(scene)
    c = cam(W, H)
    chain = rtamd.make_feature_chain(8, True, True, 0.0)
    want = gpu_ctx.render_features(c, _params(W, H, n), chain=chain)
    kw = gpu_ctx.last_feature_chain()
    assert kw["bounces"] > 0 and kw["samples"] == W * H * n
    slabs, infos, counts = _slab_pass(gpu_ctx, c, W, H, n, shards, tile, chain=chain)
    _check_slabs(gpu_ctx, slabs, want, W, H, n, shards, tile, "specular chain")
    total = {k: sum(k_r[k] for k_r in counts) for k in COUNTS}
    print("image-order", kw, "shards", counts)
    assert total == kw
    for r, k_r in enumerate(counts):
        owned = int((rtamd.shard_pixel_map(_params(W, H, n, tile, r, shards)) >= 0).sum())
        assert k_r["samples"] == owned * n == k_r["ended_surface"] + k_r["ended_miss"] + k_r["ended_cap"]
    first = gpu_ctx.render_features(c, _params(W, H, n))
    assert not np.array_equal(_bits(first), _bits(want))
    zero = rtamd.make_feature_chain(0, True, True, 0.0)
    slabs, _, counts = _slab_pass(gpu_ctx, c, W, H, n, shards, tile, chain=zero)
    _check_slabs(gpu_ctx, slabs, first, W, H, n, shards, tile, "max_bounces 0")
    assert sum(k_r["bounces"] for k_r in counts) == 0
    # an empty shard's chain pass reports zero counts
    _, infos, counts = _slab_pass(gpu_ctx, c, W, H, n, 8, 64, chain=chain)
    assert infos[-1]["work_items"] == 0 and all(counts[-1][k] == 0 for k in COUNTS)


def test_sample_ranges_accumulate_on_a_slab(gpu_ctx, monkeypatch):
    """[0, 3) then [3, 5) accumulated on the slabs is [0, 5); the padding keeps the sentinel through both."""
    _clear(monkeypatch)
    W, H, shards, tile = 37, 21, 3, 16
    scene, cam = _world("chains")
    gpu_ctx.upload(scene)
    c = cam(W, H)
    whole = gpu_ctx.render_features(c, _params(W, H, 5))
    part = gpu_ctx.render_features(c, _params(W, H, 5), first_sample=0, n_samples=3)
    slabs, _, _ = _slab_pass(gpu_ctx, c, W, H, 3, shards, tile, first=0)
    _check_slabs(gpu_ctx, slabs, part, W, H, 3, shards, tile, "[0, 3)")
    slabs, _, _ = _slab_pass(gpu_ctx, c, W, H, 2, shards, tile, first=3, slabs=slabs, accumulate=True)
    _check_slabs(gpu_ctx, slabs, whole, W, H, 2, shards, tile, "[0, 3) + [3, 5)")
    chain = rtamd.make_feature_chain(4, True, True, 0.0)
    whole = gpu_ctx.render_features(c, _params(W, H, 5), chain=chain)
    slabs, _, _ = _slab_pass(gpu_ctx, c, W, H, 3, shards, tile, first=0, chain=chain)
    slabs, _, _ = _slab_pass(gpu_ctx, c, W, H, 2, shards, tile, first=3, chain=chain, slabs=slabs, accumulate=True)
    _check_slabs(gpu_ctx, slabs, whole, W, H, 2, shards, tile, "chain [0, 3) + [3, 5)")


def test_forms_give_the_same_slab_bytes(gpu_ctx, monkeypatch):
    """random_book_one, 3 shards: every form tests/test_gpu_features.py's knob list selects gives the image-order
    pass's bytes in the slabs, first hit and chain, and the slab launch reports that form."""
    _clear(monkeypatch)
    W, H, n, shards, tile = 48, 32, 6, 3, 16
    scene, cam = _world("random_book_one")
    gpu_ctx.upload(scene)
    c = cam(W, H)
    chain = rtamd.make_feature_chain(8, True, True, 0.0)
    want = gpu_ctx.render_features(c, _params(W, H, n))
    want_chain = gpu_ctx.render_features(c, _params(W, H, n), chain=chain)
    cases = [({}, 0, dict(loop=2, lds_staged=1, leaf_lds=1, waves=4, block=1024)),
             ({"RTAMD_LDS": "0"}, 0, dict(loop=2, lds_staged=0, block=128)),
             ({"RTAMD_LEAF_LDS": "0"}, 0, dict(loop=2, lds_staged=1, leaf_lds=0)),
             ({"RTAMD_PACKED_KEYS": "0"}, 0, dict(loop=2, lds_staged=1, leaf_lds=1)),
             ({"RTAMD_PACKED_KEYS": "0", "RTAMD_LDS": "0"}, 0, dict(loop=2, lds_staged=0)),
             ({"RTAMD_WAVES": "2"}, 0, dict(loop=2, lds_staged=1, block=512)),
             ({"RTAMD_WIDE": "0"}, 0, dict(loop=1, lds_staged=0)),
             ({}, rtamd.RT_FLAG_REFERENCE_CULL, dict(loop=1, lds_staged=0))]
    for env, flags, expect in cases:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        slabs, infos, _ = _slab_pass(gpu_ctx, c, W, H, n, shards, tile, flags=flags)
        print(env, flags, infos[0])
        assert {k: infos[0][k] for k in expect} == expect, (env, flags)
        _check_slabs(gpu_ctx, slabs, want, W, H, n, shards, tile, (env, flags))
        slabs, infos, _ = _slab_pass(gpu_ctx, c, W, H, n, shards, tile, flags=flags, chain=chain)
        assert infos[0]["loop"] == expect["loop"] and infos[0]["lds_staged"] == expect["lds_staged"]
        _check_slabs(gpu_ctx, slabs, want_chain, W, H, n, shards, tile, (env, flags, "chain"))
        for k in env:
            monkeypatch.delenv(k)


def test_renders_around_a_slab_pass(gpu_ctx, monkeypatch):
    """A render, a slab pass of every shard, a render: both renders' bytes are a render's alone."""
    _clear(monkeypatch)
    W, H = 48, 32
    scene, cam = _world("random_book_one")
    gpu_ctx.upload(scene)
    c, p = cam(W, H), _params(W, H, 6, depth=8)
    rgb0, lin0, _ = gpu_ctx.render(c, p, linear=True)
    launch0 = gpu_ctx.last_launch()
    want = gpu_ctx.render_features(c, _params(W, H, 6))
    rgb1, lin1, _ = gpu_ctx.render(c, p, linear=True)
    slabs, _, _ = _slab_pass(gpu_ctx, c, W, H, 6, 3, 16)
    rgb2, lin2, _ = gpu_ctx.render(c, p, linear=True)
    assert gpu_ctx.last_launch() == launch0
    for rgb, lin in ((rgb1, lin1), (rgb2, lin2)):
        assert np.array_equal(rgb, rgb0) and np.array_equal(_bits(lin), _bits(lin0))
    _check_slabs(gpu_ctx, slabs, want, W, H, 6, 3, 16, "between renders")


def test_slab_pass_on_a_callers_stream(gpu_ctx, monkeypatch):
    _clear(monkeypatch)
    W, H, n, shards, tile = 37, 21, 5, 2, 8
    scene, cam = _world("chains")
    gpu_ctx.upload(scene)
    c = cam(W, H)
    want = gpu_ctx.render_features(c, _params(W, H, n))
    slab = rtamd.shard_geometry(_params(W, H, n, tile, 0, shards))[2]
    st = torch.cuda.Stream(device=0)
    with torch.cuda.stream(st):
        slabs = torch.full((shards, slab, 8), SENTINEL, dtype=torch.float64, device="cuda:0")
        img = torch.zeros((H, W, 8), dtype=torch.float64, device="cuda:0")
        for r in range(shards):
            p = _params(W, H, n, tile, r, shards)
            gpu_ctx.render_features_shard_async(c, p, slabs[r].data_ptr(), 0, 2, accumulate=False, stream=st.cuda_stream)
            gpu_ctx.render_features_shard_async(c, p, slabs[r].data_ptr(), 2, 3, accumulate=True, stream=st.cuda_stream)
        gpu_ctx.assemble_records_async(_params(W, H, n, tile, 0, shards), slabs.data_ptr(), img.data_ptr(),
                                       stream=st.cuda_stream)
    st.synchronize()
    assert np.array_equal(_bits(img.cpu().numpy()), _bits(want))
    _check_slabs(gpu_ctx, slabs, want, W, H, n, shards, tile, "caller's stream")


def test_error_codes_on_a_live_ctx(monkeypatch):
    """RT_E_STATE without a scene; the RT_E_INVALID cases with a live ctx; the image-order entries still reject
    shards."""
    import ctypes as C
    _clear(monkeypatch)
    ctx = rtamd.Context(0)
    try:
        L = rtamd.lib()
        cam = rtamd.camera("random_scene", 37, 21)
        buf = torch.zeros((64 * 40, 8), dtype=torch.float64, device="cuda:0")
        good = _params(37, 21, 1, 16, 1, 3)

        def call(fn, p, ptr=buf.data_ptr(), first=0, n=1):
            return fn(ctx._h, C.byref(cam), C.byref(p), None, first, n, 0, C.c_void_p(ptr), None)

        for fn in (L.rt_render_features_shard_async, L.rt_render_ids_shard_async):
            assert call(fn, good) == rtamd.RT_E_STATE and b"no scene" in L.rt_last_error()
        scene, _ = _world("chains")
        ctx.upload(scene)
        for fn in (L.rt_render_features_shard_async, L.rt_render_ids_shard_async):
            assert call(fn, good) == 0
            for bad in (_params(37, 21, 1, 12, 0, 3), _params(37, 21, 1, 264, 0, 3), _params(37, 21, 1, 16, 3, 3),
                        _params(37, 21, 1, 16, 1, 0), _params(37, 21, 1, 16, 0, -1), _params(0, 21, 1, 16, 0, 3)):
                assert call(fn, bad) == rtamd.RT_E_INVALID
            bad = _params(37, 21, 1, 16, 1, 3)
            bad.rng_mode = rtamd.RT_RNG_EXACT
            assert call(fn, bad) == rtamd.RT_E_INVALID
            assert call(fn, good, ptr=0) == rtamd.RT_E_INVALID
            assert call(fn, good, n=0) == rtamd.RT_E_INVALID and call(fn, good, first=-1) == rtamd.RT_E_INVALID
        torch.cuda.synchronize()
        with pytest.raises(rtamd.RTError):
            ctx.render_features(cam, _params(37, 21, 1, 16, 1, 3))
        with pytest.raises(rtamd.RTError):
            ctx.render_ids(cam, _params(37, 21, 1, 16, 1, 3))
    finally:
        ctx.close()
