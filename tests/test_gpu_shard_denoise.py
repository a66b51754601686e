"""Guides, mattes and the denoised preview of a sharded progressive frame
(rtamd.progressive.ShardedProgressiveFrame.render_features, render_ids, denoise) in local mode (one ctx repeated for 3
shards; two contexts on one device for 2) and in distributed mode at world 1. The reference of every comparison is
the unsharded path of the same context: `Context.render_features`, `Context.render_ids` and
`ProgressiveFrame.denoise` of the same frame at the same chunks_done. Frames of 48x32 pixels."""
import numpy as np
import pytest
import torch

import rtamd
from rtamd.progressive import ShardedProgressiveFrame
from test_denoise_host import DEMOD, FILL, counts
from test_error_host import same_bits
from test_gpu_shard_frames import _free_port

pytestmark = pytest.mark.gpu

W, H = 48, 32
CAMERAS = {"cornell": "cornell", "random_book_one": "random_scene"}
_scenes = {}


def scene_of(name):
    if name not in _scenes:
        _scenes[name] = rtamd.make_scene(name, rtamd.randGen(1024))[0]
    return _scenes[name]


def setup(ctxs, name, spp, tile, depth=10, seed=77):
    for c in ctxs:
        c.upload(scene_of(name))
    return rtamd.camera(CAMERAS[name], W, H), rtamd.make_params(W, H, spp, depth, rtamd.RT_RNG_PHILOX, seed=seed,
                                                                tile=tile)


def same_result(got, want):
    return same_bits(got[1], want[1]) and np.array_equal(got[0], want[0]) and counts(got[2]) == counts(want[2])


def check_guides(frame, ctx, cam, p, n=6):
    """render_features and render_ids, with and without a chain, are the ctx's image-order passes; `into` over two
    ranges is one range. Returns the first-hit sums (the torch tensor)."""
    chain = rtamd.make_feature_chain(8, True, True, 0.0)
    for ch in (None, chain):
        want = ctx.render_features(cam, p, n_samples=n, chain=ch)
        got = frame.render_features(n_samples=n, chain=ch)
        assert got.shape == (H, W, 8) and got.dtype == torch.float64 and got.device.index == frame.root.device
        assert same_bits(got.cpu().numpy(), want), ("features", ch is not None)
        part = frame.render_features(0, 2, chain=ch)
        assert same_bits(part.cpu().numpy(), ctx.render_features(cam, p, 0, 2, chain=ch))
        both = frame.render_features(2, n - 2, chain=ch, into=part)
        assert same_bits(both.cpu().numpy(), want), ("into", ch is not None)
        recs = frame.render_ids(n_samples=n, chain=ch)
        want_recs = ctx.render_ids(cam, p, n_samples=n, chain=ch)
        assert recs.dtype == rtamd.ID_DTYPE and recs.shape == (H, W) and recs.tobytes() == want_recs.tobytes()
    return frame.render_features(n_samples=n)


def check_denoise(frame, ctx, cam, p, feats, n, moments, **kw):
    """Both frames rendered to their last chunk; the sharded denoise is the unsharded frame's, and leaves the frame's
    resolve as it was."""
    with ctx.open_frame(cam, p, moments=moments) as ref:
        while not ref.complete:
            ref.advance(4)
        while not frame.complete:
            frame.advance(3)
        assert frame.chunks_done == ref.chunks_done >= 2
        want = ref.denoise(feats, n, **kw)
        before = frame.resolve()
        got = frame.denoise(feats, n, **kw)
        assert same_result(got, want)
        assert same_result(frame.denoise(feats.cpu().numpy(), n, **kw), want)  # (host sums, and a repeat)
        after, unsharded = frame.resolve(), ref.resolve()
        keys = ("chunks_done", "samples_done", "nan_pixels", "bytes_changed")
        for a in (after, unsharded):
            assert np.array_equal(a[0], before[0]) and same_bits(a[1], before[1])
        assert [after[2][k] for k in keys] == [before[2][k] for k in keys]
        assert frame.denoise(feats, n, rgb=False, linear=False, **kw)[:2] == (None, None)
        return got, before


def test_three_shards_on_one_ctx(gpu_ctx):
    """Cornell 48x32x16 with moments, tile 16: six tiles dealt to three shard frames of one ctx."""
    cam, p = setup([gpu_ctx], "cornell", 16, 16)
    assert rtamd.frame_chunking(W * H, 16)[1] >= 2
    with ShardedProgressiveFrame([gpu_ctx] * 3, cam, p, moments=True) as frame:
        feats = check_guides(frame, gpu_ctx, cam, p)
        got, before = check_denoise(frame, gpu_ctx, cam, p, feats, 6, True, flags=DEMOD)
        assert not same_bits(got[1], before[1])  # (the filter did something)


def test_denoise_right_after_an_advance(gpu_ctx):
    """advance, denoise, resolve with no resolve between: the denoise is the unsharded frame's after the same
    calls, and the resolve that follows reports what the unsharded frame's reports (images and counts), at one
    chunk (no error map yet) and at every later one."""
    cam, p = setup([gpu_ctx], "cornell", 24, 16)
    assert rtamd.frame_chunking(W * H, 24)[1] >= 3
    feats = gpu_ctx.render_features(cam, p, n_samples=6)
    keys = ("chunks_done", "samples_done", "nan_pixels", "bytes_changed")
    with ShardedProgressiveFrame([gpu_ctx] * 3, cam, p, moments=True) as frame, \
            gpu_ctx.open_frame(cam, p, moments=True) as ref:
        while not ref.complete:
            assert frame.advance(1) == ref.advance(1) == 1
            assert same_result(frame.denoise(feats, 6, flags=DEMOD), ref.denoise(feats, 6, flags=DEMOD))
            got, want = frame.resolve(), ref.resolve()
            assert np.array_equal(got[0], want[0]) and same_bits(got[1], want[1])
            assert [got[2][k] for k in keys] == [want[2][k] for k in keys]
        assert frame.complete


def test_into_must_continue_the_kept_slabs(gpu_ctx):
    cam, p = setup([gpu_ctx], "cornell", 16, 16)
    chain = rtamd.make_feature_chain(8, True, True, 0.0)
    with ShardedProgressiveFrame([gpu_ctx] * 2, cam, p) as frame:
        with pytest.raises(rtamd.RTError):
            frame.render_features(0, 2, into=True)  # (no kept slabs)
        part = frame.render_features(0, 2)
        with pytest.raises(rtamd.RTError):
            frame.render_features(3, 2, into=part)  # (a gap)
        with pytest.raises(rtamd.RTError):
            frame.render_features(2, 2, chain=chain, into=part)  # (another chain)
        both = frame.render_features(2, 2, into=True)
        assert same_bits(both.cpu().numpy(), gpu_ctx.render_features(cam, p, 0, 4))


def test_two_contexts_on_one_device(gpu_ctx):
    """Two shards, each on its own ctx (tile 8: 24 tiles); an untracked frame: the filter runs without an error map."""
    other = rtamd.Context(0)
    try:
        cam, p = setup([gpu_ctx, other], "cornell", 16, 8)
        with ShardedProgressiveFrame([gpu_ctx, other], cam, p) as frame:
            feats = check_guides(frame, gpu_ctx, cam, p)
            check_denoise(frame, gpu_ctx, cam, p, feats, 6, False, flags=DEMOD, color_floor=0.2)
    finally:
        other.close()


def test_nan_quirk_frame_with_fill(gpu_ctx):
    """random_book_one 48x32: the Lambertian-mixture quirk leaves NaN pixels (asserted on the unsharded render);
    with RT_DENOISE_FILL the sharded denoise fills them as the unsharded frame's does."""
    cam, p = setup([gpu_ctx], "random_book_one", 40, 16)
    _, lin, _ = gpu_ctx.render(cam, p, linear=True)
    bad = ~np.isfinite(lin).all(-1)
    print("NaN pixels of the unsharded render:", int(bad.sum()))
    assert 0 < bad.sum() < W * H
    with ShardedProgressiveFrame([gpu_ctx] * 3, cam, p, moments=True) as frame:
        feats = frame.render_features(n_samples=4)
        assert same_bits(feats.cpu().numpy(), gpu_ctx.render_features(cam, p, n_samples=4))
        got, _ = check_denoise(frame, gpu_ctx, cam, p, feats, 4, True, flags=FILL)
        assert got[2]["invalid_in"] == int(bad.sum()) and got[2]["filled"] > 0


def test_distributed_mode_over_rccl_world_one(gpu_ctx):
    import torch.distributed as dist
    cam, p = setup([gpu_ctx], "cornell", 16, 16)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{_free_port()}", rank=0, world_size=1, device_id=dev)
    try:
        with ShardedProgressiveFrame(gpu_ctx, cam, p, moments=True, rank=0, world=1, backend="nccl", gather=True) as frame:
            assert frame.gather and not frame.local
            feats = check_guides(frame, gpu_ctx, cam, p)
            check_denoise(frame, gpu_ctx, cam, p, feats, 6, True, flags=DEMOD)
    finally:
        dist.destroy_process_group()
