"""Shard frames on the GPU (include/rt.h: rt_frame_open_shard, rt_frame_resolve_shard, rt_frame_error_shard,
rt_frame_shard_state, rt_frame_save_header, rt_frame_restore_shard): N progressive frames over the tile shards
of one image, open on one ctx and advanced interleaved, each shard in its own step pattern. Their slabs,
assembled by rt_assemble[_linear]_async, are the unsharded frame's previews, sums, moments, error map and K_p
bit for bit; their counts add up to its counts; header + assembled sums is its blob; a checkpoint of 3 shards
resumes on 2; and rtamd.progressive.ShardedProgressiveFrame drives all of it.

The reference in every test is an UNSHARDED frame (and rt_render) of the same parameters, computed once per
key and left unchanged.

Shapes (every test asserts its chunking first):
    P    97x61   spp 40  CH 1  40 chunks, depth 8: mostly padded tiles; tile 16, N 3: 28 tiles dealt 10/9/9;
                                tile 64, N 3: 2 tiles, the third shard owns nothing
    S2   256x192 spp 99  CH 5  20 chunks, depth 10, the last chunk of 4 samples
"""
import json
import os
import socket

import numpy as np
import pytest

import rtamd
from rtamd.progressive import ShardedProgressiveFrame, shard_params
from test_error_host import same_bits

pytestmark = pytest.mark.gpu

P, S2 = (97, 61, 40, 8), (256, 192, 99, 10)
CHUNKS = {P: (1, 40), S2: (5, 20)}
E_STATE, E_INVALID, E_UNSUPPORTED = r"\(-5\)", r"\(-1\)", r"\(-4\)"
F_SKIP = 32768
SCENES = {"random_book_one": "random_scene", "cornell": "cornell", "next_week_final": "next_week",
          "stress_spheres": "random_scene"}
# what rt_last_launch reports of a shard's launches: 4-wide walk with the tree in LDS, the Cornell box's binary walk
# in LDS, the full variant's replacement loop (media / instance frames), the 4-wide walk from global memory
FORMS = {"random_book_one": dict(loop=2, lds_staged=1), "cornell": dict(loop=1, lds_staged=1),
         "next_week_final": dict(loop=1), "stress_spheres": dict(loop=2, lds_staged=0)}
_scenes, _cache = {}, {}


def check_shape(shape):
    w, h, spp, _ = shape
    assert rtamd.frame_chunking(w * h, spp) == CHUNKS[shape]


def scene_of(name):
    if name not in _scenes:
        kw = {"param": 20000} if name == "stress_spheres" else {}
        _scenes[name] = rtamd.make_scene(name, rtamd.randGen(1024), **kw)[0]
    return _scenes[name]


def setup(ctx, name, shape, seed=77, **kw):
    w, h, spp, depth = shape
    check_shape(shape)
    if ctx._scene is not scene_of(name):  # (an upload rebuilds the BVH: once per run of tests over one scene)
        ctx.upload(scene_of(name))
    return rtamd.camera(SCENES[name], w, h), rtamd.make_params(w, h, spp, depth, rtamd.RT_RNG_PHILOX, seed=seed, **kw)


def frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


def payload(blob, p):
    return np.frombuffer(blob, dtype="<f8", offset=288).reshape(p.height, p.width, 3)


def reference(ctx, cam, p, points, key, moments=False, render=True):
    """The unsharded frame of (cam, p) at each of `points` chunks: {K: (rgb, linear, resolve stats, blob, Q)},
    and under "render" rt_render's (rgb, linear)."""
    if key not in _cache:
        out = {}
        with ctx.open_frame(cam, p, moments=moments) as fr:
            for k in points:
                assert fr.advance(k - fr.chunks_done) > 0 and fr.chunks_done == k
                rgb, lin, st = fr.resolve()
                out[k] = frozen(rgb, lin, st, fr.save(), fr.moments() if moments else None)
        if render:
            rgb, lin, _ = ctx.render(cam, p, linear=True)
            out["render"] = frozen(rgb, lin)
        _cache[key] = out
    return _cache[key]


def open_shards(ctx, cam, p, n, tile, moments=False):
    ps = shard_params(p, 0, n)
    ps.tile = tile
    return [ctx.open_shard_frame(cam, shard_params(ps, r, n), moments=moments) for r in range(n)], ps


def advance_to(frames, k, shift=0):
    """Every shard to `k` chunks, interleaved on the ctx, shard r in steps of 1 + (r + shift) % 3 chunks."""
    while any(f.chunks_done < k for f in frames):
        for r, f in enumerate(frames):
            n = min(1 + (r + shift) % 3, k - f.chunks_done)
            if n:
                assert f.advance(n) == n
    assert all(f.chunks_done == k for f in frames)


def assembled(ctx, ps, tensors):
    """The shards' [slab, 3] device slabs (uint8 or float64) through rt_assemble[_linear]_async -> numpy [H, W, 3]."""
    import torch
    slabs = torch.stack(tensors).contiguous()
    img = torch.zeros((ps.height, ps.width, 3), dtype=slabs.dtype, device=slabs.device)
    if slabs.dtype == torch.uint8:
        ctx.assemble_async(ps, slabs.data_ptr(), img.data_ptr())
    else:
        ctx.assemble_linear_async(ps, slabs.data_ptr(), img.data_ptr())
    torch.cuda.synchronize()
    return img.cpu().numpy()


def resolved(ctx, ps, frames):
    """(rgb, linear, stats dicts) of the shards' previews, assembled."""
    import torch
    rgbs, lins, stats = [], [], []
    for f in frames:
        t_rgb, t_lin = f.slab_tensor(torch.uint8), f.slab_tensor(torch.float64)
        stats.append(f.resolve_into(t_rgb, t_lin))
        rgbs.append(t_rgb)
        lins.append(t_lin)
    return assembled(ctx, ps, rgbs), assembled(ctx, ps, lins), stats


def state_images(ctx, ps, frames, moments):
    """(S[H,W,3], Q[H,W,3] | None, K_p[H,W]) of the shards' states: S and Q assembled on the device, K_p merged
    through shard_pixel_map."""
    import torch
    ss, qs, kp = [], [], np.zeros(ps.height * ps.width, np.int32)
    for r, f in enumerate(frames):
        s, k = f.slab_tensor(torch.float64), f.slab_tensor(torch.int32, 0)
        q = f.slab_tensor(torch.float64) if moments else None
        f.state_into(s, q, k)
        ss.append(s)
        qs.append(q)
        m = rtamd.shard_pixel_map(shard_params(ps, r, len(frames)))
        kp[m[m >= 0]] = k.cpu().numpy()[m >= 0]
    return (assembled(ctx, ps, ss), assembled(ctx, ps, qs) if moments else None, kp.reshape(ps.height, ps.width))


def close_all(frames):
    for f in frames:
        f.close()


def total(stats, key):
    return sum(s[key] for s in stats)


# ----------------------------------------------------------------------------- 1. bit identity
@pytest.mark.parametrize("n, tile", [(1, 8), (2, 8), (3, 8), (8, 8), (1, 16), (2, 16), (3, 16), (8, 16), (3, 64)])
@pytest.mark.parametrize("name", list(SCENES))
def test_shard_previews_and_final_image_are_the_unsharded_frames(gpu_ctx, name, n, tile):
    cam, p = setup(gpu_ctx, name, P)
    ref = reference(gpu_ctx, cam, p, (7, 19, 40), ("bits", name))
    frames, ps = open_shards(gpu_ctx, cam, p, n, tile)
    try:
        assert sum(f.owned_pixels for f in frames) == 97 * 61
        if (n, tile) == (3, 16):
            assert [rtamd.shard_geometry(f.params)[1] for f in frames] == [10] * 3 and rtamd.shard_geometry(ps)[0] == 28
        if tile == 64:
            assert frames[2].owned_pixels == 0
        for k in (7, 19, 40):  # (two consecutive resolves at intermediate counts, then the finished frame)
            advance_to(frames, k)
            launch = gpu_ctx.last_launch()  # (the scenes are here for their kernel forms)
            assert all(launch[key] == v for key, v in FORMS[name].items()), launch
            rgb, lin, stats = resolved(gpu_ctx, ps, frames)
            assert np.array_equal(rgb, ref[k][0])
            assert np.array_equal(lin, ref[k][1], equal_nan=True) and same_bits(np.nan_to_num(lin), np.nan_to_num(ref[k][1]))
            assert total(stats, "nan_pixels") == ref[k][2]["nan_pixels"]
            assert total(stats, "bytes_changed") == ref[k][2]["bytes_changed"]
            assert all(s["chunks_done"] == k and s["samples_done"] == k and s["chunks_total"] == 40 for s in stats)
        assert np.array_equal(rgb, ref["render"][0]) and np.array_equal(lin, ref["render"][1], equal_nan=True)
        # a poll with nothing new rendered repeats the stats; a complete frame advances by 0
        again = frames[0].resolve_into()
        assert {k: again[k] for k in ("nan_pixels", "bytes_changed")} == {k: stats[0][k] for k in ("nan_pixels", "bytes_changed")}
        assert frames[0].advance(3) == 0
    finally:
        close_all(frames)


def test_short_last_chunk_at_s2(gpu_ctx):
    cam, p = setup(gpu_ctx, "random_book_one", S2)
    ref = reference(gpu_ctx, cam, p, (7, 20), ("s2", "plain"), moments=True)
    frames, ps = open_shards(gpu_ctx, cam, p, 3, 16)
    try:
        for k in (7, 20):
            advance_to(frames, k)
            rgb, lin, stats = resolved(gpu_ctx, ps, frames)
            assert np.array_equal(rgb, ref[k][0]) and np.array_equal(lin, ref[k][1], equal_nan=True)
            assert all(s["samples_done"] == min(99, 5 * k) for s in stats)
            assert total(stats, "bytes_changed") == ref[k][2]["bytes_changed"]
        assert np.array_equal(rgb, ref["render"][0]) and np.array_equal(lin, ref["render"][1], equal_nan=True)
    finally:
        close_all(frames)


# ----------------------------------------------------------------------------- 2. state
@pytest.mark.parametrize("n, tile", [(2, 8), (3, 16), (8, 16), (3, 64)])
def test_shard_state_is_the_unsharded_sums_and_moments(gpu_ctx, n, tile):
    cam, p = setup(gpu_ctx, "random_book_one", P)
    ref = reference(gpu_ctx, cam, p, (7, 19), ("state", "P"), moments=True, render=False)
    for shift in (0, 1):  # (two different step patterns)
        frames, ps = open_shards(gpu_ctx, cam, p, n, tile, moments=True)
        try:
            for k in (7, 19):
                advance_to(frames, k, shift)
                s, q, kp = state_images(gpu_ctx, ps, frames, True)
                assert same_bits(s, payload(ref[k][3], p)) and same_bits(q, ref[k][4])
                assert (kp == k).all()
        finally:
            close_all(frames)


# ----------------------------------------------------------------------------- 3. error
@pytest.mark.parametrize("n, tile", [(1, 8), (3, 16), (8, 8), (3, 64)])
def test_shard_error_maps_and_stats(gpu_ctx, n, tile):
    import torch
    cam, p = setup(gpu_ctx, "cornell", P)
    tol = (0.02, 0.05)
    key = ("error", "P")
    if key not in _cache:
        with gpu_ctx.open_frame(cam, p, moments=True) as fr:
            fr.advance(9)
            se, st = fr.error(*tol)
            sums, q = payload(fr.save(), p).copy(), fr.moments()
        _cache[key] = frozen(se, st, sums, q)
    ref_se, ref_st, sums, q = _cache[key]
    host = rtamd.error_estimate(sums, q, 9, 9, *tol)[1]
    frames, ps = open_shards(gpu_ctx, cam, p, n, tile, moments=True)
    try:
        advance_to(frames, 9)
        maps, parts = [], []
        for f in frames:
            t = f.slab_tensor(torch.float64)
            parts.append(f.error_into(t, *tol))
            maps.append(t)
            assert f.error_into(None, *tol) == parts[-1] and f.error_into(t, *tol) == parts[-1]  # (repeats exactly)
            assert parts[-1]["pixels"] == f.owned_pixels
        se = assembled(gpu_ctx, ps, maps)
        assert np.array_equal(se, ref_se, equal_nan=True) and same_bits(np.nan_to_num(se), np.nan_to_num(ref_se))
        merged = rtamd.error_stats_merge(parts)
        for k in ("chunks_done", "samples_done", "pixels", "nonfinite_pixels", "unconverged_pixels", "max_se"):
            assert merged[k] == ref_st[k] == host[k], k
        print("mean_se merged", merged["mean_se"], "unsharded", ref_st["mean_se"], "host", host["mean_se"])
        assert abs(merged["mean_se"] - host["mean_se"]) <= 1e-12 * host["mean_se"]
        assert 0 < merged["unconverged_pixels"] < merged["pixels"] - merged["nonfinite_pixels"]
    finally:
        close_all(frames)


def test_mean_se_keeps_its_summation_order(gpu_ctx):
    """mean_se to the last bit (the tests above hold it to 1e-12 only): a frame's blocks, one per 256 pixels of its
    own order, and their fixed-order sum are what tests/golden/frame_mean_se.json recorded. An unsharded frame, its
    3 shard frames at tile 16, and an adapted unsharded frame with pixels stopped before two chunks."""
    with open(os.path.join(os.path.dirname(__file__), "golden", "frame_mean_se.json")) as fh:
        want = json.load(fh)
    cam, p = setup(gpu_ctx, "cornell", P)
    tol = (0.02, 0.05)
    with gpu_ctx.open_frame(cam, p, moments=True) as fr:
        fr.advance(9)
        got = fr.error(*tol, want_map=False)[1]["mean_se"].hex()
    assert got == want["cornell_97x61_40spp_depth8_seed77_9_chunks_tol_0.02_0.05"]
    frames, _ = open_shards(gpu_ctx, cam, p, 3, 16, moments=True)
    try:
        advance_to(frames, 9)
        assert [f.error_into(None, *tol)["mean_se"].hex() for f in frames] == want["the_same_on_3_shards_tile_16"]
    finally:
        close_all(frames)
    gpu_ctx.upload(scene_of("three_spheres"))
    cam = rtamd.camera("random_scene", 64, 48)
    p = rtamd.make_params(64, 48, 6, 8, rtamd.RT_RNG_PHILOX, seed=77)
    yy, xx = np.mgrid[0:48, 0:64]
    with gpu_ctx.open_frame(cam, p, moments=True) as fr:
        fr.advance(1)
        fr.stop((xx + yy) % 5 == 0)
        fr.advance(2)
        got = fr.error(want_map=False)[1]["mean_se"].hex()
    assert got == want["three_spheres_64x48_6spp_depth8_seed77_stop_mask_at_1_chunk_error_at_3"]


# ----------------------------------------------------------------------------- 4. adaptive
def test_nan_rule_on_every_shard_ends_with_rt_renders_image(gpu_ctx):
    cam, p = setup(gpu_ctx, "random_book_one", S2)
    ref = reference(gpu_ctx, cam, p, (7, 20), ("s2", "plain"), moments=True)
    key = ("s2", "nan")
    if key not in _cache:
        with gpu_ctx.open_frame(cam, p) as fr:
            nans = []
            for k in (3, 9, 20):
                fr.advance(k - fr.chunks_done)
                nans.append(fr.adapt(nan=True, converged=False)["stopped_nan"])
        _cache[key] = nans
    frames, ps = open_shards(gpu_ctx, cam, p, 3, 16)
    try:
        for k, want in zip((3, 9, 20), _cache[key]):
            advance_to(frames, k)
            stats = [f.adapt(nan=True, converged=False) for f in frames]
            assert total(stats, "stopped_nan") == want
            assert total(stats, "pixels") == 256 * 192 and all(s["pixels"] == f.owned_pixels for s, f in zip(stats, frames))
            if k < 20 and want:
                # (shard 0 one chunk ahead of the others: advance_to evens it out before the next stop call)
                assert frames[0].advance(1) == 1 and gpu_ctx.last_launch()["variant"] & F_SKIP
        assert _cache[key][-1] > 0
        rgb, lin, _ = resolved(gpu_ctx, ps, frames)
        assert np.array_equal(rgb, ref["render"][0]) and np.array_equal(lin, ref["render"][1], equal_nan=True)
    finally:
        close_all(frames)


def adapted_reference(ctx, cam, p, key, stops):
    """An unsharded tracked frame with `stops` = [(K, call)], call(frame) making the stop call at K chunks, run to
    its end: (rgb, linear, Q, K_p, [adapt stats])."""
    if key not in _cache:
        with ctx.open_frame(cam, p, moments=True) as fr:
            stats = []
            for k, call in stops:
                fr.advance(k - fr.chunks_done)
                stats.append(call(fr))
            fr.advance(p.spp)
            rgb, lin, _ = fr.resolve()
            _cache[key] = frozen(rgb, lin, fr.moments(), fr.chunk_counts()) + (stats,)
    return _cache[key]


def cut_mask(w, h):
    """A stop mask that cuts through tiles, 8x8 blocks and waves: diagonal stripes, a band 13 wide and single pixels."""
    y, x = np.mgrid[0:h, 0:w]
    return (((x + 2 * y) % 5 == 0) | (x < 13) | ((x == 40) & (y % 9 == 4))).astype(np.uint8)


@pytest.mark.parametrize("n, tile", [(2, 8), (3, 16), (8, 16), (3, 64)])
def test_adaptive_shards_equal_the_adaptive_unsharded_frame(gpu_ctx, n, tile):
    cam, p = setup(gpu_ctx, "cornell", P)
    rule = dict(abs_tol=0.02, rel_tol=0.05, min_chunks=8)
    mask = cut_mask(97, 61)
    stops = [(5, lambda f: f.stop(mask)), (8, lambda f: f.adapt(**rule)), (16, lambda f: f.adapt(**rule)),
             (24, lambda f: f.adapt(**rule))]
    ref_rgb, ref_lin, ref_q, ref_kp, ref_stats = adapted_reference(gpu_ctx, cam, p, ("adapt", "P"), stops)
    # (the reference run exercises what it should: masked pixels, converged pixels at several K, active ones)
    assert set(np.unique(ref_kp)) >= {5, 8, 40} and ref_stats[1]["stopped_now"] > 0 and ref_stats[-1]["active_pixels"] > 0
    frames, ps = open_shards(gpu_ctx, cam, p, n, tile, moments=True)
    try:
        def live():  # (a shard whose pixels are all stopped renders nothing more: advance reports 0 chunks)
            return [f for f in frames if f.active_pixels or not f.owned_pixels]

        for (k, call), want in zip(stops, ref_stats):
            advance_to(live(), k)
            stats = [call(f) for f in frames]
            for key in ("pixels", "active_pixels", "stopped_nan", "stopped_converged_or_masked", "stopped_now"):
                assert total(stats, key) == want[key], (k, key)
            owner = next(f for f in frames if f.owned_pixels and f.active_pixels)
            done = owner.chunks_done
            assert owner.advance(1) == 1 and gpu_ctx.last_launch()["variant"] & F_SKIP
            advance_to([f for f in live() if f is not owner], done + 1)
        assert all(f.advance(1) == 0 for f in frames if f not in live())
        advance_to(live(), 40)
        rgb, lin, _ = resolved(gpu_ctx, ps, frames)
        s, q, kp = state_images(gpu_ctx, ps, frames, True)
        assert np.array_equal(kp, ref_kp)
        assert np.array_equal(rgb, ref_rgb) and np.array_equal(lin, ref_lin, equal_nan=True)
        assert same_bits(q, ref_q)
        with pytest.raises(rtamd.RTError, match=E_STATE):  # (stopped pixels: no version-1 header, as save)
            next(f for f in frames if f.active_pixels < f.owned_pixels).save_header()
    finally:
        close_all(frames)


# ----------------------------------------------------------------------------- 5. checkpoint
def test_checkpoint_of_three_shards_resumes_on_two_and_unsharded(gpu_ctx):
    cam, p = setup(gpu_ctx, "random_book_one", S2)
    ref = reference(gpu_ctx, cam, p, (7, 20), ("s2", "plain"), moments=True)
    frames, ps = open_shards(gpu_ctx, cam, p, 3, 16, moments=True)
    try:
        advance_to(frames, 7)
        heads = [f.save_header() for f in frames]
        assert len(heads[0]) == 288 and heads[1] == heads[0] and heads[2] == heads[0]
        s, q, _ = state_images(gpu_ctx, ps, frames, True)
    finally:
        close_all(frames)
    blob = heads[0] + np.ascontiguousarray(s, dtype="<f8").tobytes()
    # the unsharded frame was opened at the default tile 8, the shards at 16: the tile is a header field
    want = ref[7][3]
    assert blob[288:] == want[288:] and same_bits(q, ref[7][4])
    with gpu_ctx.open_frame(cam, ps) as fr:  # (the same tile: the whole blob byte for byte)
        fr.advance(7)
        assert fr.save() == blob
        assert fr.save_header() == heads[0]  # (works on unsharded frames too)
    info = rtamd.blob_info(blob)
    assert info["chunks_done"] == 7 and info["tile"] == 16 and (info["shard_rank"], info["shard_count"]) == (0, 1)
    # M = 2 shard frames from the 3 shards' checkpoint
    two = [gpu_ctx.restore_shard_frame(blob, r, 2, q) for r in range(2)]
    try:
        assert all(f.chunks_done == 7 and f.params.tile == 16 for f in two)
        p2 = shard_params(ps, 0, 2)
        s2, q2, _ = state_images(gpu_ctx, p2, two, True)
        assert same_bits(s2, s) and same_bits(q2, q)
        advance_to(two, 20, shift=1)
        rgb, lin, _ = resolved(gpu_ctx, p2, two)
        _, q_end, _ = state_images(gpu_ctx, p2, two, True)
        assert np.array_equal(rgb, ref["render"][0]) and np.array_equal(lin, ref["render"][1], equal_nan=True)
        assert same_bits(q_end, ref[20][4])
    finally:
        close_all(two)
    # and through plain rt_frame_restore_ex with the moments
    with gpu_ctx.restore_frame(blob, q) as fr:
        assert fr.advance(99) == 13
        rgb, lin, _ = fr.resolve()
        assert np.array_equal(rgb, ref["render"][0]) and np.array_equal(lin, ref["render"][1], equal_nan=True)
        assert same_bits(fr.moments(), ref[20][4])


# ----------------------------------------------------------------------------- 6. errors
def test_errors_and_the_shard_that_owns_nothing(gpu_ctx):
    import torch
    cam, p = setup(gpu_ctx, "random_book_one", P)
    frames, ps = open_shards(gpu_ctx, cam, p, 3, 64, moments=False)
    plain = gpu_ctx.open_frame(cam, p)
    try:
        sh = frames[0]
        sh.advance(2)
        plain.advance(2)
        # image-order calls on a shard frame, _shard calls on an unsharded frame
        for call in (lambda: rtamd.ProgressiveFrame.resolve(sh), sh.save, sh.moments, sh.chunk_counts,
                     lambda: rtamd.ProgressiveFrame.error(sh)):
            with pytest.raises(rtamd.RTError, match=E_STATE + r".*_shard|" + E_STATE + r".*rt_frame_save_header"):
                call()
        L = rtamd.lib()
        st = rtamd.rt_frame_stats()
        assert L.rt_frame_resolve_shard(plain._h, None, None, st) == rtamd.RT_E_STATE
        assert b"rt_frame_resolve" in L.rt_last_error()
        assert L.rt_frame_error_shard(plain._h, None, None, None) == rtamd.RT_E_STATE
        assert L.rt_frame_shard_state(plain._h, None, None, None) == rtamd.RT_E_STATE
        # moments of an untracked shard frame
        with pytest.raises(rtamd.RTError, match=E_STATE):
            sh.state_into(None, sh.slab_tensor(torch.float64), None)
        with pytest.raises(rtamd.RTError, match=E_STATE):
            sh.error_into(None)
        # the shard that owns nothing: advances, resolves with zero counts, adapts with pixels == 0
        empty = frames[2]
        assert empty.owned_pixels == 0 and empty.advance(5) == 5 and empty.chunks_done == 5
        st = empty.resolve_into(empty.slab_tensor(torch.uint8), empty.slab_tensor(torch.float64))
        assert st["chunks_done"] == 5 and st["nan_pixels"] == 0 and st["bytes_changed"] == 0
        ad = empty.adapt(nan=True, converged=False)
        assert ad["pixels"] == 0 and ad["active_pixels"] == 0 and ad["stopped_now"] == 0
        assert empty.stop(np.ones((61, 97), np.uint8))["pixels"] == 0
        assert empty.advance(100) == 35 and empty.complete
        # bad rank / count, tier A
        for rank, count in ((3, 3), (-1, 3), (1, 1), (0, -2)):
            with pytest.raises(rtamd.RTError, match=E_INVALID):
                gpu_ctx.open_shard_frame(cam, shard_params(p, rank, count))
        exact = shard_params(p, 0, 2)
        exact.rng_mode = rtamd.RT_RNG_EXACT
        with pytest.raises(rtamd.RTError, match=E_UNSUPPORTED):
            gpu_ctx.open_shard_frame(cam, exact)
        # a blob of this scene against another scene; a re-upload invalidates shard frames
        blob = plain.save()
        with pytest.raises(rtamd.RTError, match=E_INVALID):
            gpu_ctx.restore_shard_frame(blob, 2, 2)
        gpu_ctx.upload(scene_of("cornell"))
        with pytest.raises(rtamd.RTError, match=E_STATE):
            gpu_ctx.restore_shard_frame(blob, 0, 2)
        for call in (lambda: sh.advance(1), sh.resolve_into, sh.save_header, lambda: sh.state_into(None, None, None)):
            with pytest.raises(rtamd.RTError, match=E_STATE):
                call()
    finally:
        close_all(frames + [plain])


# ----------------------------------------------------------------------------- 7. driver
def drive(frame, ref, p):
    """A ShardedProgressiveFrame through previews, an error poll, a checkpoint and the NaN rule to its end."""
    assert frame.advance(7) == 7
    rgb, lin, st = frame.resolve()
    assert np.array_equal(rgb, ref[7][0]) and np.array_equal(lin, ref[7][1], equal_nan=True)
    assert st["nan_pixels"] == ref[7][2]["nan_pixels"] and st["bytes_changed"] == ref[7][2]["bytes_changed"]
    se, est = frame.error(0.02, 0.05)
    host = rtamd.error_estimate(payload(ref[7][3], p), ref[7][4], 7, 35, 0.02, 0.05)
    assert np.array_equal(se, host[0], equal_nan=True)
    assert all(est[k] == host[1][k] for k in ("pixels", "nonfinite_pixels", "unconverged_pixels", "max_se"))
    assert abs(est["mean_se"] - host[1]["mean_se"]) <= 1e-12 * host[1]["mean_se"]
    blob, q = frame.save()
    assert blob[288:] == ref[7][3][288:] and same_bits(q, ref[7][4])
    assert (frame.chunk_counts() == 7).all()
    return blob, q


def finish(frame, ref):
    ad = frame.adapt(nan=True, converged=False)
    assert ad["pixels"] == 256 * 192 and ad["active_pixels"] + ad["stopped_nan"] == ad["pixels"]
    while not frame.complete:
        assert frame.advance(6) > 0
    rgb, lin, _ = frame.resolve()
    assert np.array_equal(rgb, ref["render"][0]) and np.array_equal(lin, ref["render"][1], equal_nan=True)
    kp = frame.chunk_counts()
    assert ((kp == 20) | (kp == 7)).all() and (kp == 7).sum() == ad["stopped_nan"]
    assert same_bits(np.where(kp[..., None] == 20, frame.moments(), 0.0), np.where(kp[..., None] == 20, ref[20][4], 0.0))


def test_driver_local_mode_one_context_three_shards(gpu_ctx):
    cam, p = setup(gpu_ctx, "random_book_one", S2)
    ref = reference(gpu_ctx, cam, p, (7, 20), ("s2", "plain"), moments=True)
    with ShardedProgressiveFrame([gpu_ctx] * 3, cam, p, moments=True) as frame:
        blob, q = drive(frame, ref, p)
    with ShardedProgressiveFrame.restore([gpu_ctx] * 2, blob, q) as frame:  # (3 shards' checkpoint on 2)
        assert frame.chunks_done == 7 and frame.world == 2
        finish(frame, ref)


def test_driver_local_mode_two_contexts_on_one_device(gpu_ctx):
    cam, p = setup(gpu_ctx, "random_book_one", S2)
    ref = reference(gpu_ctx, cam, p, (7, 20), ("s2", "plain"), moments=True)
    other = rtamd.Context(0)
    try:
        other.upload(scene_of("random_book_one"))
        with ShardedProgressiveFrame([gpu_ctx, other], cam, p, moments=True) as frame:
            drive(frame, ref, p)
            finish(frame, ref)
    finally:
        other.close()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_driver_distributed_mode_over_rccl_world_one(gpu_ctx):
    import torch
    import torch.distributed as dist
    cam, p = setup(gpu_ctx, "random_book_one", S2)
    ref = reference(gpu_ctx, cam, p, (7, 20), ("s2", "plain"), moments=True)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{_free_port()}", rank=0, world_size=1, device_id=dev)
    try:
        assert dist.get_backend() == "nccl"
        with ShardedProgressiveFrame(gpu_ctx, cam, p, moments=True, rank=0, world=1, backend="nccl", gather=True) as frame:
            assert frame.gather and not frame.local
            drive(frame, ref, p)
            finish(frame, ref)
    finally:
        dist.destroy_process_group()
