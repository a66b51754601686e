"""Checkpoints of progressive frames on the GPU (include/rt.h: rt_frame_checkpoint, rt_frame_resume[_shard],
rt_frame_shard_stops, rt_frame_checkpoint_header): a resumed frame is the saved frame. Whatever calls follow, it
gives bit for bit and count for count what the uninterrupted frame gives (the first resolve's bytes_changed
apart, which every restored frame takes against zero); the shards' assembled checkpoint is the unsharded
frame's byte for byte and resumes on any shard count; the host-only preview and error map of a checkpoint are
the resumed frame's first resolve and error.

The reference in every test is the UNINTERRUPTED frame of the same calls. Shapes (each test asserts its
chunking first; tests/test_gpu_adaptive.py):
    S2   256x192 spp 99  CH 5  20 chunks, the last of 4 samples
    T    64x48   spp 6   CH 1   6 chunks, depth 8
    P    97x61   spp 12  CH 1  12 chunks, tile 16: 28 tiles, 3 shards; tile 64: 2 tiles, the third shard owns nothing
"""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import rtamd
import test_gpu_adaptive as ga
from rtamd.progressive import shard_params
from test_error_host import same_bits

pytestmark = pytest.mark.gpu

S1, S2, T, P = ga.S1, ga.S2, ga.T, ga.P
E_STATE, E_INVALID = ga.E_STATE, ga.E_INVALID
F_SKIP = ga.F_SKIP
HEADER = 320
MOMENTS, STOPS = rtamd.RT_CKPT_MOMENTS, rtamd.RT_CKPT_STOPS
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def no_ms(stats):
    return {k: v for k, v in stats.items() if k != "kernel_ms"}


def same_preview(a, b):
    """Two resolves: bytes, linear bits and every count but kernel_ms."""
    return np.array_equal(a[0], b[0]) and same_bits(a[1], b[1]) and no_ms(a[2]) == no_ms(b[2])


def same_error(a, b):
    return same_bits(a[0], b[0]) and a[1] == b[1]


# ------------------------------------------------------------------ 1. a plain frame
def test_a_plain_frames_checkpoint_is_its_save(gpu_ctx):
    ga.check_shape(T)
    cam, p = ga.setup(gpu_ctx, "three_spheres", T, depth=8)
    ref_rgb, ref_lin, _ = gpu_ctx.render(cam, p, linear=True)
    with gpu_ctx.open_frame(cam, p) as fr:
        assert fr.advance(3) == 3
        ck, v1 = fr.checkpoint(), fr.save()
    info = rtamd.checkpoint_info(ck)
    assert info["version"] == 2 and info["sections"] == 0 and info["chunks_done"] == 3 and info["active_pixels"] == 64 * 48
    assert len(ck) == HEADER + 64 * 48 * 24 and ck[HEADER:] == v1[288:]
    assert ck[:8] == v1[:8] and struct.unpack_from("<I", ck, 8)[0] == 2 and ck[12:288] == v1[12:288]
    assert ck[288:HEADER] == bytes(32)
    for blob in (ck, v1):  # rt_frame_resume takes both versions
        with gpu_ctx.resume_frame(blob) as fr:
            assert fr.chunks_done == 3 and not fr.tracks_moments and fr.active_pixels == 64 * 48
            assert fr.advance(100) == 3 and fr.complete
            rgb, lin, st = fr.resolve()
            assert fr.checkpoint()[HEADER:] == fr.save()[288:]
        assert np.array_equal(rgb, ref_rgb) and np.array_equal(lin, ref_lin, equal_nan=True)
        assert st["bytes_changed"] == int((ref_rgb != 0).sum())  # (a restored frame's first resolve: against zero)


def golden_frame(ctx):
    """The frame of tests/golden/checkpoint_v2_three_spheres.bin: (checkpoint, the frame's preview bytes)."""
    ga.check_shape(T)
    cam, p = ga.setup(ctx, "three_spheres", T, depth=8)
    yy, xx = np.mgrid[0:48, 0:64]
    with ctx.open_frame(cam, p, moments=True) as fr:
        fr.advance(2)
        fr.stop((7 * xx + 13 * yy) % 3 == 0)
        fr.advance(2)
        return fr.checkpoint(), fr.resolve(linear=False)[0]


def test_the_committed_checkpoint_is_this_frames(gpu_ctx):
    ck, rgb = golden_frame(gpu_ctx)
    assert len(ck) == 160064
    assert ck == open(os.path.join(GOLDEN, "checkpoint_v2_three_spheres.bin"), "rb").read()
    assert rgb.tobytes() == open(os.path.join(GOLDEN, "checkpoint_v2_three_spheres_preview.bin"), "rb").read()


# ------------------------------------------------------------------ 2. a tracked, adapted frame
POINTS = [8, 11, 16, 20]  # stop calls at 8 and 16 (tests/test_gpu_adaptive.py), checkpoints at 8 and 11


def cornell_states(fr, abs_tol, first=None):
    """Drives `fr` (at 0, 8 or 11 chunks) through POINTS: a resolve at every point, NAN | CONVERGED at 8 and 16, a
    checkpoint after the stop call at 8 and at 11. Returns {point: state}; `first`: the resumed frame's state at
    the point it was saved at (no stop call is repeated there)."""
    out = {}
    if first is not None:
        out[first] = dict(resolve=fr.resolve(), error=fr.error(abs_tol, 0.0), ck=fr.checkpoint())
    for k in [q for q in POINTS if q > fr.chunks_done]:
        n = k - fr.chunks_done
        assert fr.advance(n) == n
        st = dict(resolve=fr.resolve())
        if k in (8, 16):
            st["adapt"] = fr.adapt(abs_tol, 0.0, 2)
        st["error"] = fr.error(abs_tol, 0.0)
        st["kp"], st["q"] = fr.chunk_counts(), fr.moments()
        st["ck"] = fr.checkpoint()  # (S, Q and K in one: equal bytes are equal sums, moments and stops)
        out[k] = st
    return out


def test_a_resumed_adaptive_frame_is_the_uninterrupted_one(gpu_ctx, monkeypatch):
    ga.check_shape(S2)
    monkeypatch.delenv("RTAMD_PARTIAL_CAP", raising=False)
    cam, p, _, abs_tol, want_kp = ga.cornell_reference(gpu_ctx)
    with gpu_ctx.open_frame(cam, p, moments=True) as fr:
        ref = cornell_states(fr, abs_tol)
    assert np.array_equal(ref[20]["kp"], want_kp)  # (the frame of tests/test_gpu_adaptive.py)
    i8 = rtamd.checkpoint_info(ref[8]["ck"])
    shares = (i8["stopped_pixels"] / i8["pixels"], i8["active_pixels"] / i8["pixels"], float((i8["K"] == 8).mean()))
    print("at the first checkpoint: stopped %.3f, active %.3f, K_p == chunks_done %.3f" % shares)
    assert shares[0] >= 0.05 and shares[1] >= 0.05 and (i8["K"] == 8).any()
    assert i8["sections"] == MOMENTS | STOPS and i8["chunks_done"] == 8 and i8["samples_done"] == 40
    assert i8["stopped_pixels"] == ref[8]["adapt"]["stopped_nan"] + ref[8]["adapt"]["stopped_converged_or_masked"]
    assert len(ref[8]["ck"]) == HEADER + 256 * 192 * 52
    for at in (8, 11):
        ck = ref[at]["ck"]
        with gpu_ctx.resume_frame(ck) as fr:
            assert fr.chunks_done == at and fr.tracks_moments
            assert fr.active_pixels == rtamd.checkpoint_info(ck)["active_pixels"] == ref[8]["adapt"]["active_pixels"]
            got = cornell_states(fr, abs_tol, first=at)
            assert gpu_ctx.last_launch()["variant"] & F_SKIP
        # the saved state itself: the checkpoint again, the error map, and the preview but for bytes_changed
        first = got[at]
        assert first["ck"] == ck
        assert same_error(first["error"], ref[at]["error"])
        assert np.array_equal(first["resolve"][0], ref[at]["resolve"][0]) and same_bits(first["resolve"][1], ref[at]["resolve"][1])
        assert first["resolve"][2]["nan_pixels"] == ref[at]["resolve"][2]["nan_pixels"]
        assert first["resolve"][2]["bytes_changed"] == int((ref[at]["resolve"][0] != 0).sum())
        # the host-only preview and error map of the blob are the resumed frame's first resolve and error
        off = rtamd.checkpoint_resolve(ck)
        assert np.array_equal(off[0], first["resolve"][0]) and no_ms(off[2]) == no_ms(first["resolve"][2])
        fin = np.isfinite(off[1])  # (finite values bit for bit; a NaN is a NaN, whatever its payload)
        assert np.array_equal(off[1], first["resolve"][1], equal_nan=True) and same_bits(off[1][fin], first["resolve"][1][fin])
        assert off[2]["kernel_ms"] == 0.0
        se, est = rtamd.checkpoint_error(ck, abs_tol, 0.0)
        assert np.array_equal(se, first["error"][0], equal_nan=True)
        fin = np.isfinite(se)
        assert same_bits(se[fin], first["error"][0][fin])
        for key in ("chunks_done", "samples_done", "pixels", "nonfinite_pixels", "unconverged_pixels", "max_se"):
            assert est[key] == first["error"][1][key], key
        assert abs(est["mean_se"] - first["error"][1]["mean_se"]) <= 1e-12 * est["mean_se"]  # (rt.h's bound)
        # everything after it: K_p, S, Q, bytes, linear image, adapt stats, the error map and its stats
        for k in [q for q in POINTS if q > at]:
            g, r = got[k], ref[k]
            assert g["ck"] == r["ck"], (at, k)
            assert np.array_equal(g["kp"], r["kp"]) and same_bits(g["q"], r["q"])
            assert same_error(g["error"], r["error"]), (at, k)
            assert g.get("adapt") == r.get("adapt"), (at, k)
            assert same_preview(g["resolve"], r["resolve"]), (at, k)  # (bytes_changed: against the same preview)


def test_resumed_resolves_count_changes_like_the_uninterrupted_frame(gpu_ctx):
    """bytes_changed after the first resolve of a resumed frame: taken against the resumed frame's own previous
    preview, which is the uninterrupted frame's."""
    ga.check_shape(T)
    cam, p = ga.setup(gpu_ctx, "cornell", T, depth=8)
    with gpu_ctx.open_frame(cam, p, moments=True) as fr:
        fr.advance(2)
        fr.resolve()
        fr.adapt(converged=False)
        ck = fr.checkpoint()
        fr.advance(2)
        want = fr.resolve()
    with gpu_ctx.resume_frame(ck) as fr:
        fr.resolve()
        fr.advance(2)
        assert same_preview(fr.resolve(), want)


# ------------------------------------------------------------------ 3. the NaN rule
def test_nan_rule_checkpoint_resumes_to_rt_render(gpu_ctx):
    ga.check_shape(S2)
    cam, p = ga.setup(gpu_ctx, "random_book_one", S2)
    ref_rgb, ref_lin, _ = gpu_ctx.render(cam, p, linear=True)

    def steps(fr, upto):
        out = []
        while fr.chunks_done < upto:
            assert fr.advance(4) == 4
            out.append(fr.adapt(converged=False))
        return out

    with gpu_ctx.open_frame(cam, p) as fr:  # (untracked: the NaN rule needs only S)
        head = steps(fr, 8)
        ck = fr.checkpoint()
        rest = steps(fr, 20)
        end = fr.resolve()
    info = rtamd.checkpoint_info(ck)
    assert info["sections"] == STOPS and info["chunks_done"] == 8 and info["Q"] is None
    assert info["stopped_pixels"] == info["stopped_nan"] == head[-1]["stopped_nan"] > 0.3 * 256 * 192
    assert info["stopped_nan"] == rtamd.checkpoint_resolve(ck, rgb=False, linear=False)[2]["nan_pixels"]
    with gpu_ctx.resume_frame(ck) as fr:
        assert not fr.tracks_moments and fr.active_pixels == info["active_pixels"]
        assert fr.resolve(rgb=False, linear=False)[2]["nan_pixels"] == info["stopped_nan"]
        got = steps(fr, 20)
        assert gpu_ctx.last_launch()["variant"] & F_SKIP
        rgb, lin, st = fr.resolve()
    assert len(got) == 3 and got == rest  # the adapt stats at 12, 16 and 20
    assert np.array_equal(rgb, ref_rgb), "bytes differ from rt_render's"
    assert np.array_equal(lin, ref_lin, equal_nan=True), "the linear image differs from rt_render's"
    assert st["nan_pixels"] == end[2]["nan_pixels"] == got[-1]["stopped_nan"]


# ------------------------------------------------------------------ 4. shards
def owned_mask(p, rank, count):
    m = rtamd.shard_pixel_map(shard_params(p, rank, count))
    out = np.zeros(p.width * p.height, bool)
    out[m[m >= 0]] = True
    return out.reshape(p.height, p.width)


def shard_script(fr, mask, abs_tol, upto):
    """The stop calls of the shard test on any kind of frame at 0 chunks: the mask at 2, both rules at 4, then on
    to `upto`."""
    assert fr.advance(2) == 2
    fr.stop(mask)
    fr.advance(2)
    st = fr.adapt(abs_tol, 0.0, 2)
    fr.advance(upto - 4)
    return st


def finish(fr, abs_tol):
    """From 5 chunks: both rules again at 8, then to the end. Returns the final (resolve, error, checkpoint, K_p)."""
    fr.advance(8 - fr.chunks_done)
    st = fr.adapt(abs_tol, 0.0, 2)
    fr.advance(100)
    rgb, lin, rs = fr.resolve()
    se, es = fr.error(abs_tol, 0.0)
    return dict(rgb=rgb, lin=lin, nan=rs["nan_pixels"], se=se, es=es, ck=fr.checkpoint(), kp=fr.chunk_counts(), adapt=st)


def same_end(a, b):
    return (a["ck"] == b["ck"] and np.array_equal(a["rgb"], b["rgb"]) and same_bits(a["lin"], b["lin"]) and
            a["nan"] == b["nan"] and same_bits(a["se"], b["se"]) and np.array_equal(a["kp"], b["kp"]) and
            a["adapt"] == b["adapt"] and all(a["es"][k] == b["es"][k] for k in a["es"] if k != "mean_se") and
            abs(a["es"]["mean_se"] - b["es"]["mean_se"]) <= 1e-12 * a["es"]["mean_se"])


def test_a_checkpoint_of_three_shards_resumes_on_two_and_unsharded(gpu_ctx):
    ga.check_shape(P)
    cam, p = ga.setup(gpu_ctx, "cornell", P, depth=8, tile=16)
    assert rtamd.shard_geometry(shard_params(p, 0, 3))[:2] == (28, 10)
    yy, xx = np.mgrid[0:61, 0:97]
    # cuts through tiles, 8x8 blocks and waves, and holds every pixel of shard 1
    mask = ((5 * xx + 3 * yy) % 7 == 0) | (xx == 21) | owned_mask(p, 1, 3)
    assert not mask.all() and not mask[:, :16].all() and mask[:8, 16:32].all()
    with gpu_ctx.open_frame(cam, p, moments=True) as fr:
        fr.advance(4)
        se = fr.error()[0].max(axis=2)
    abs_tol = float(np.median(se[se > 0]))
    # the unsharded adaptive frame: checkpoint at 5, then to the end
    with gpu_ctx.open_frame(cam, p, moments=True) as fr:
        ust = shard_script(fr, mask, abs_tol, 5)
        uck = fr.checkpoint()
        uend = finish(fr, abs_tol)
    info = rtamd.checkpoint_info(uck)
    assert info["sections"] == MOMENTS | STOPS and info["chunks_done"] == 5
    assert ust["stopped_now"] > 0 and info["active_pixels"] == ust["active_pixels"] > 0
    assert set(np.unique(info["K"])) == {0, 2, 4}
    # three shard frames on one ctx
    with rtamd.ShardedProgressiveFrame([gpu_ctx] * 3, cam, p, moments=True) as sh:
        sst = shard_script(sh, mask, abs_tol, 5)
        assert sst == ust
        lag = sh.frames[1]
        assert lag.active_pixels == 0 and lag.chunks_done == 2 < sh.frames[0].chunks_done == sh.chunks_done == 5
        assert (lag.stops()[rtamd.shard_pixel_map(lag.params) >= 0] == 2).all()
        sck = sh.checkpoint()
        assert sck == uck, "the assembled checkpoint differs from the unsharded frame's"
        # every shard writes the same header; a shard that still has active pixels cannot be ahead of itself
        heads = [f.checkpoint_header(MOMENTS | STOPS, 5) for f in sh.frames]
        assert heads[0] == heads[1] == heads[2] == uck[:HEADER]
        assert sh.frames[0].checkpoint_header(MOMENTS | STOPS) == uck[:HEADER]  # (-1: its own count)
        assert struct.unpack_from("<i", lag.checkpoint_header(STOPS), 260)[0] == 2
        with pytest.raises(rtamd.RTError, match=E_STATE):
            sh.frames[0].checkpoint_header(MOMENTS | STOPS, 6)
        assert len(lag.checkpoint_header(MOMENTS | STOPS, 12)) == HEADER
        for bad in (13, 1, -2):
            with pytest.raises(rtamd.RTError, match=E_INVALID):
                lag.checkpoint_header(MOMENTS | STOPS, bad)
        with pytest.raises(rtamd.RTError, match=E_INVALID):
            lag.checkpoint_header(4)
        send = finish(sh, abs_tol)
    assert same_end(send, uend)
    # ... resumed on two shards, and unsharded
    with rtamd.ShardedProgressiveFrame.resume([gpu_ctx] * 2, sck) as sh2:
        assert sh2.chunks_done == 5 and sh2.tracks_moments and sh2.active_pixels == info["active_pixels"]
        assert sum(f.active_pixels for f in sh2.frames) == info["active_pixels"]
        assert sh2.checkpoint() == sck
        assert same_end(finish(sh2, abs_tol), uend)
    with gpu_ctx.resume_frame(sck) as fr:
        assert same_end(finish(fr, abs_tol), uend)
    # an untracked shard frame has no Q to give
    with gpu_ctx.open_shard_frame(cam, shard_params(p, 0, 3)) as fr:
        with pytest.raises(rtamd.RTError, match=E_STATE):
            fr.checkpoint_header(MOMENTS)
        assert (fr.stops() == 0).all()  # (no stop call yet)


def test_a_shard_that_owns_nothing(gpu_ctx):
    ga.check_shape(P)
    cam, p = ga.setup(gpu_ctx, "cornell", P, depth=8, tile=64)
    assert rtamd.shard_geometry(shard_params(p, 0, 3))[0] == 2 and not owned_mask(p, 2, 3).any()
    yy, xx = np.mgrid[0:61, 0:97]
    mask = (5 * xx + 3 * yy) % 7 == 0
    with gpu_ctx.open_frame(cam, p, moments=True) as fr:
        fr.advance(2)
        fr.stop(mask)
        fr.advance(1)
        uck = fr.checkpoint()
        fr.advance(100)
        uend = fr.resolve()[:2] + (fr.checkpoint(),)
    with rtamd.ShardedProgressiveFrame([gpu_ctx] * 3, cam, p, moments=True) as sh:
        sh.advance(2)
        sh.stop(mask)
        sh.advance(1)
        assert sh.checkpoint() == uck
    with rtamd.ShardedProgressiveFrame.resume([gpu_ctx] * 3, uck) as sh:
        assert sh.frames[2].owned_pixels == 0 and sh.frames[2].active_pixels == 0
        sh.advance(100)
        rgb, lin, _ = sh.resolve()
        assert np.array_equal(rgb, uend[0]) and same_bits(lin, uend[1]) and sh.checkpoint() == uend[2]


def test_sharded_checkpoint_in_distributed_mode_over_rccl_world_one(gpu_ctx):
    """The driver as one rank of a torch.distributed group of one, the nccl gather forced on: K_p goes through
    all_gather_into_tensor like the other slabs."""
    import socket

    import torch
    import torch.distributed as dist
    ga.check_shape(T)
    cam, p = ga.setup(gpu_ctx, "three_spheres", T, depth=8)
    first, _ = ga.wave_cutting_masks()
    with gpu_ctx.open_frame(cam, p, moments=True) as fr:
        fr.advance(2)
        fr.stop(first)
        fr.advance(1)
        want = fr.checkpoint()
        fr.advance(100)
        end = fr.checkpoint()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=dev)
    try:
        kw = dict(rank=0, world=1, backend="nccl", gather=True)
        with rtamd.ShardedProgressiveFrame(gpu_ctx, cam, p, moments=True, **kw) as f:
            assert f.gather and not f.local
            f.advance(2)
            f.stop(first)
            f.advance(1)
            assert f.checkpoint() == want
        with rtamd.ShardedProgressiveFrame.resume(gpu_ctx, want, **kw) as f:
            assert f.gather and not f.local and f.chunks_done == 3 and f.tracks_moments
            assert f.active_pixels == 64 * 48 - int(first.sum())
            f.advance(100)
            assert f.checkpoint() == end
    finally:
        dist.destroy_process_group()


# ------------------------------------------------------------------ 5. the kernel forms after a resume with stops
@pytest.mark.parametrize("name", ["three_spheres", "stress_spheres"])
def test_launches_after_a_resume_with_stops_read_the_mask(gpu_ctx, name, monkeypatch):
    ga.check_shape(T)
    monkeypatch.delenv("RTAMD_PARTIAL_CAP", raising=False)
    if name not in ga._scenes:
        ga._scenes[name] = rtamd.make_scene(name, rtamd.randGen(1024), **(dict(param=20000) if name == "stress_spheres" else {}))[0]
    gpu_ctx.upload(ga._scenes[name])
    cam = rtamd.camera("random_scene", 64, 48)
    p = rtamd.make_params(64, 48, 6, 8, rtamd.RT_RNG_PHILOX, seed=11)
    first, second = ga.wave_cutting_masks()
    with gpu_ctx.open_frame(cam, p) as fr:
        fr.advance(2)
        plain = gpu_ctx.last_launch()
        assert plain["lds_staged"] == (1 if name == "three_spheres" else 0) and plain["variant"] & F_SKIP == 0
        fr.stop(first)
        ck = fr.checkpoint()
        fr.advance(2)
        skipping = gpu_ctx.last_launch()
        fr.stop(second)
        fr.advance(2)
        want = fr.resolve() + (fr.chunk_counts(),)
    with gpu_ctx.resume_frame(ck) as fr:
        assert fr.active_pixels == 64 * 48 - int(first.sum())
        assert fr.advance(2) == 2
        ll = gpu_ctx.last_launch()
        assert ll["variant"] == plain["variant"] | F_SKIP == skipping["variant"]
        assert all(ll[k] == skipping[k] for k in ("loop", "lds_staged", "leaf_lds", "waves", "grid", "block", "dyn_lds_bytes"))
        fr.stop(second)
        fr.advance(2)
        got = fr.resolve() + (fr.chunk_counts(),)
    assert np.array_equal(got[0], want[0]) and same_bits(got[1], want[1]) and np.array_equal(got[3], want[3])
    assert got[2]["nan_pixels"] == want[2]["nan_pixels"]


# ------------------------------------------------------------------ 6. errors
def test_errors(gpu_ctx):
    ga.check_shape(T)
    cam, p = ga.setup(gpu_ctx, "three_spheres", T, depth=8)
    L = rtamd.lib()
    h = C.c_void_p()
    with gpu_ctx.open_frame(cam, p, moments=True) as fr:
        fr.advance(2)
        fr.stop(np.eye(48, 64, dtype=bool))
        ck = fr.checkpoint()
        n = C.c_size_t(0)  # the buffer protocol of rt_frame_save: a short cap is a size query
        small = C.create_string_buffer(16)
        assert L.rt_frame_checkpoint(fr._h, small, 16, C.byref(n)) == 0 and n.value == len(ck) and small.raw == bytes(16)
        assert L.rt_frame_shard_stops(fr._h, None) == rtamd.RT_E_STATE  # an unsharded frame has no slab
        assert b"rt_frame_checkpoint" in L.rt_last_error()
    assert rtamd.checkpoint_info(ck)["sections"] == MOMENTS | STOPS
    # a version-2 blob into the version-1 calls
    assert L.rt_frame_restore(gpu_ctx._h, ck, len(ck), C.byref(h)) == rtamd.RT_E_INVALID and not h.value
    assert L.rt_frame_restore_shard(gpu_ctx._h, ck, len(ck), None, 0, 2, C.byref(h)) == rtamd.RT_E_INVALID
    for bad in (ck[:-1], ck[:288] + struct.pack("<I", 7) + ck[292:]):
        assert L.rt_frame_resume(gpu_ctx._h, bad, len(bad), C.byref(h)) == rtamd.RT_E_INVALID and not h.value
    assert L.rt_frame_resume_shard(gpu_ctx._h, ck, len(ck), 2, 2, C.byref(h)) == rtamd.RT_E_INVALID and not h.value
    # a shard frame: the image-order call names the shard calls
    with gpu_ctx.resume_shard_frame(ck, 1, 2) as sf:
        assert sf.chunks_done == 2 and sf.tracks_moments and sf.active_pixels < sf.owned_pixels
        with pytest.raises(rtamd.RTError, match=E_STATE) as e:
            sf.checkpoint()
        for call in ("rt_frame_checkpoint_header", "rt_frame_shard_state", "rt_frame_shard_stops"):
            assert call in str(e.value)
        with pytest.raises(rtamd.RTError, match=E_STATE):
            sf.save_header()  # (stopped pixels: the version-1 header still refuses)
        # the ctx's scene is replaced: the frame is over
        gpu_ctx.upload(ga.scene_of("three_spheres"))
        for call in (sf.stops, lambda: sf.checkpoint_header(STOPS)):
            with pytest.raises(rtamd.RTError, match=E_STATE):
                call()
    with gpu_ctx.resume_frame(ck) as fr:
        gpu_ctx.upload(ga.scene_of("three_spheres"))
        with pytest.raises(rtamd.RTError, match=E_STATE):
            fr.checkpoint()
    # another scene
    gpu_ctx.upload(ga.scene_of("cornell"))
    for call in (lambda: gpu_ctx.resume_frame(ck), lambda: gpu_ctx.resume_shard_frame(ck, 0, 2)):
        with pytest.raises(rtamd.RTError, match=E_STATE):
            call()
    fresh = rtamd.Context(0)  # no scene at all
    try:
        with pytest.raises(rtamd.RTError, match=E_STATE):
            fresh.resume_frame(ck)
    finally:
        fresh.close()


# ------------------------------------------------------------------ 7. render_progressive(resume=, checkpoint=)
def test_render_progressive_resumes_from_its_checkpoints(gpu_ctx):
    ga.check_shape(S1)
    cam, p = ga.setup(gpu_ctx, "cornell", S1)
    with gpu_ctx.open_frame(cam, p, moments=True) as fr:
        fr.advance(8)
        se = fr.error()[0].max(axis=2)
    kw = dict(adaptive=True, abs_tol=float(np.median(se[se > 0])), rel_tol=0.01, min_chunks=4)
    whole = list(rtamd.render_progressive(gpu_ctx, cam, p, 4, **kw))
    print([s["active_pixels"] for _, s in whole])
    assert len(whole) >= 4 and 0 < whole[1][1]["active_pixels"] < 96 * 64  # (at least two steps after the resume)
    blobs = []
    gen = rtamd.render_progressive(gpu_ctx, cam, p, 4, checkpoint=blobs.append, **kw)
    head = [next(gen), next(gen)]
    gen.close()  # interrupted after 2 steps
    assert len(blobs) == 2 and rtamd.checkpoint_info(blobs[1])["chunks_done"] == 8
    assert rtamd.checkpoint_info(blobs[1])["active_pixels"] == whole[1][1]["active_pixels"]
    later = []
    rest = list(rtamd.render_progressive(gpu_ctx, None, None, 4, resume=blobs[1], checkpoint=later.append, **kw))
    got = head + rest
    assert len(got) == len(whole) and len(later) == len(rest)
    for i, ((rgb, st), (rgb_w, st_w)) in enumerate(zip(got, whole)):
        a, b = no_ms(st), no_ms(st_w)
        if i == 2:  # the first resolve of the resumed frame counts its changes against zero
            assert a.pop("bytes_changed") == int((rgb_w != 0).sum()) and b.pop("bytes_changed") >= 0
        assert np.array_equal(rgb, rgb_w) and a == b, i
    assert rtamd.checkpoint_info(later[-1])["chunks_done"] == whole[-1][1]["chunks_done"]
