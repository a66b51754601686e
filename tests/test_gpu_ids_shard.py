"""Sharded material-ID passes on the device (include/rt.h rt_render_ids_shard_async, rt_assemble_records_async).
The reference of every comparison is the image-order pass of the same context (`Context.render_ids`) and
rtamd.shard_pixel_map; comparisons are of bytes, every slab starts from the byte 0xAB, which must survive in the
padding. The geometries are tests/test_gpu_features_shard.py's."""
import numpy as np
import pytest
import torch

import rtamd
from test_gpu_features_shard import COUNTS, GEOMETRIES, _clear, _params, _work_items, _world
from test_ids_host import OVERFLOW

pytestmark = pytest.mark.gpu

SENTINEL = 0xAB


def _slab_pass(ctx, cam, W, H, n, shards, tile, chain=None, first=0, seed=1024, slabs=None, accumulate=False):
    """Every shard's ID pass into one [shards, slab, 64] byte tensor that starts from the sentinel (or `slabs`)."""
    slab = rtamd.shard_geometry(_params(W, H, n, tile, 0, shards))[2]
    if slabs is None:
        slabs = torch.full((shards, slab, 64), SENTINEL, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
    infos, counts = [], []
    for r in range(shards):
        p = _params(W, H, n, tile, r, shards, seed=seed)
        ctx.render_ids_shard_async(cam, p, slabs[r].data_ptr(), first, n, chain=chain, accumulate=accumulate)
        infos.append(ctx.last_feature_launch())
        if chain is not None:
            counts.append(ctx.last_feature_chain())
    torch.cuda.synchronize()
    return slabs, infos, counts


def _check_slabs(ctx, slabs, want, W, H, n, shards, tile, what):
    """Owned slots hold the image-order pass's records, the padding the sentinel, and the merge gives the array."""
    host = slabs.cpu().numpy()
    flat = np.ascontiguousarray(want).view(np.uint8).reshape(W * H, 64)
    owned = 0
    for r in range(shards):
        m = rtamd.shard_pixel_map(_params(W, H, n, tile, r, shards))
        ok = m >= 0
        owned += int(ok.sum())
        assert np.array_equal(host[r][ok], flat[m[ok]]), (what, "owned slots of shard", r)
        assert (host[r][~ok] == SENTINEL).all(), (what, "padding of shard", r)
    assert owned == W * H
    img = torch.full((H, W, 64), 0xCD, dtype=torch.uint8, device="cuda:0")
    ctx.assemble_records_async(_params(W, H, n, tile, 0, shards), slabs.data_ptr(), img.data_ptr())
    torch.cuda.synchronize()
    got = img.cpu().numpy().view(rtamd.ID_DTYPE).reshape(H, W)
    assert got.tobytes() == np.ascontiguousarray(want).tobytes(), (what, "assembled")
    on_host = rtamd.assemble_records_host(host.view(rtamd.ID_DTYPE)[..., 0], _params(W, H, n, tile, 0, shards))
    assert on_host.tobytes() == np.ascontiguousarray(want).tobytes()
    return got


WORLDS = [("chains", 37, 21, 5, 1), ("random_book_one", 48, 32, 6, 2), ("deep", 40, 27, 3, 0), ("fog", 64, 48, 4, 1)]


@pytest.mark.parametrize("name,W,H,n,walk", WORLDS, ids=[w[0] for w in WORLDS])
def test_id_slabs_are_the_image_order_pass(gpu_ctx, monkeypatch, name, W, H, n, walk):
    """First hit and chain (8 bounces, both materials) over every geometry; with a chain the counts add up."""
    _clear(monkeypatch)
    scene, cam = _world(name)
    gpu_ctx.upload(scene)
    c = cam(W, H)
    chain = rtamd.make_feature_chain(8, True, True, 0.0)
    want = gpu_ctx.render_ids(c, _params(W, H, n))
    assert gpu_ctx.last_feature_launch()["loop"] == walk
    want_chain = gpu_ctx.render_ids(c, _params(W, H, n), chain=chain)
    kw = gpu_ctx.last_feature_chain()
    for shards, tile in GEOMETRIES:
        slabs, infos, _ = _slab_pass(gpu_ctx, c, W, H, n, shards, tile)
        _check_slabs(gpu_ctx, slabs, want, W, H, n, shards, tile, (name, shards, tile))
        for r, info in enumerate(infos):
            assert info["loop"] == walk and info["work_items"] == _work_items(W, H, shards, tile, r), (shards, tile, r)
        slabs, _, counts = _slab_pass(gpu_ctx, c, W, H, n, shards, tile, chain=chain)
        _check_slabs(gpu_ctx, slabs, want_chain, W, H, n, shards, tile, (name, shards, tile, "chain"))
        assert {k: sum(k_r[k] for k_r in counts) for k in COUNTS} == kw, (shards, tile)


def test_accumulate_on_a_slab(gpu_ctx, monkeypatch):
    """[0, 3) then [3, 5) folded onto the slabs is [0, 5), first hit and chain."""
    _clear(monkeypatch)
    W, H, shards, tile = 37, 21, 3, 16
    scene, cam = _world("chains")
    gpu_ctx.upload(scene)
    c = cam(W, H)
    for chain in (None, rtamd.make_feature_chain(4, True, True, 0.0)):
        whole = gpu_ctx.render_ids(c, _params(W, H, 5), chain=chain)
        part = gpu_ctx.render_ids(c, _params(W, H, 5), first_sample=0, n_samples=3, chain=chain)
        slabs, _, _ = _slab_pass(gpu_ctx, c, W, H, 3, shards, tile, chain=chain)
        _check_slabs(gpu_ctx, slabs, part, W, H, 3, shards, tile, "[0, 3)")
        slabs, _, _ = _slab_pass(gpu_ctx, c, W, H, 2, shards, tile, chain=chain, first=3, slabs=slabs, accumulate=True)
        _check_slabs(gpu_ctx, slabs, whole, W, H, 2, shards, tile, "[0, 3) + [3, 5)")


def test_overflowing_pixels_and_the_mattes(gpu_ctx, monkeypatch):
    """The book-one cover at 16x8, 64 samples, as tests/test_gpu_ids.py's test_overflowing_pixels builds it: some
    pixel overflows its seven slots and some fills them exactly (asserted on the image-order records). The slabs
    hold those records; the matte and the preview of the assembled records are those of the image-order records."""
    _clear(monkeypatch)
    name, W, H, n, seed = OVERFLOW
    scene, cam = _world(name)
    gpu_ctx.upload(scene)
    c = cam(W, H)
    want = gpu_ctx.render_ids(c, _params(W, H, n, seed=seed))
    used = (want["count"] > 0).sum(axis=-1)
    assert (want["other"] > 0).any() and ((used == 7) & (want["other"] == 0)).any()
    ids = np.unique(want["id"][(want["count"] > 0) & (want["id"] != rtamd.RT_ID_MISS)])[::2]
    for shards, tile in ((2, 8), (3, 16)):
        slabs, infos, _ = _slab_pass(gpu_ctx, c, W, H, n, shards, tile, seed=seed)
        assert infos[0]["loop"] == 2 and infos[0]["lds_staged"] == 1
        got = _check_slabs(gpu_ctx, slabs, want, W, H, n, shards, tile, ("overflow", shards, tile))
        for a, b in zip(gpu_ctx.id_matte(got, ids), gpu_ctx.id_matte(want, ids)):
            assert a.tobytes() == b.tobytes()
        assert gpu_ctx.id_preview(got).tobytes() == gpu_ctx.id_preview(want).tobytes()
        for a, b in zip(rtamd.id_matte(got, ids), gpu_ctx.id_matte(want, ids)):
            assert a.tobytes() == b.tobytes()
