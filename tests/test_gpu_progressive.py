"""Progressive tier-B frames on the GPU (include/rt.h, rt_frame_*): a frame advanced in any step pattern
ends bit-identical to rt_render of the same params, a preview equals rt_render at that sample count, the
stats are exact, other calls on the ctx interleave freely, and a saved frame continues on another ctx.

"Equal" is np.array_equal on the bytes and np.array_equal(..., equal_nan=True) on the linear image.
Shapes (chunk sizes from rt_sample_chunk; every test asserts them first, so that a change of the chunk
rule fails loudly instead of hollowing the tests):
    S1  96x64   spp 40  CH 1  40 chunks
    S2  256x192 spp 99  CH 5  20 chunks, the last of 4 samples
    S3  640x480 spp 60  CH 8   8 chunks, the last of 4 samples
"""
import numpy as np
import pytest

import pyoracle
import rtamd
from conftest import parity

pytestmark = pytest.mark.gpu

S1, S2, S3 = (96, 64, 40), (256, 192, 99), (640, 480, 60)
CHUNKS = {S1: (1, 40), S2: (5, 20), S3: (8, 8)}
DEPTH = 10
E_UNSUPPORTED, E_STATE, E_INVALID = r"\(-4\)", r"\(-5\)", r"\(-1\)"

# scene -> (camera, param); stress_spheres with 20000 spheres does not fit the LDS-staged kernels
SCENES = {"random_book_one": ("random_scene", 0), "cornell": ("cornell", 0), "cornell_smoke": ("cornell", 0),
          "next_week_final": ("next_week", 0), "stress_spheres": ("random_scene", 20000)}
_scenes, _refs = {}, {}


def check_shape(shape):
    """The chunk rule the tests are built on (first line of every test), asked of the library: rt.h's own
    rt_sample_chunk through rt_frame_chunking, not a copy of the rule."""
    w, h, spp = shape
    assert rtamd.frame_chunking(w * h, spp) == CHUNKS[shape]


def scene_of(name):
    if name not in _scenes:
        _scenes[name] = rtamd.make_scene(name, rtamd.randGen(1024), param=SCENES[name][1])[0]
    return _scenes[name]


def setup(ctx, name, shape, spp=None, flags=0, seed=77):
    w, h, full = shape
    ctx.upload(scene_of(name))
    cam = rtamd.camera(SCENES[name][0], w, h)
    return cam, rtamd.make_params(w, h, full if spp is None else spp, DEPTH, rtamd.RT_RNG_PHILOX, seed=seed, flags=flags)


def reference(ctx, name, shape, spp=None, flags=0):
    """rt_render of the frame (the scene is uploaded), computed once per (scene, shape, spp, flags)."""
    key = (name, shape, spp, flags)
    if key not in _refs:
        cam, p = setup(ctx, name, shape, spp, flags)
        rgb, lin, _ = ctx.render(cam, p, linear=True)
        rgb.setflags(write=False)
        lin.setflags(write=False)
        _refs[key] = (rgb, lin)
    return _refs[key]


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1], equal_nan=True)


def run_steps(frame, steps):
    """Advance by each of `steps` ("rest": what remains); returns the chunks each call reported."""
    done = []
    for s in steps:
        done.append(frame.advance(frame.chunks_total - frame.chunks_done if s == "rest" else s))
    return done


PATTERNS = {"all": ["rest"], "one": None, "3-7-rest": [3, 7, "rest"], "over": [5, 1000]}


@pytest.mark.parametrize("name, pattern", [
    ("random_book_one", "all"), ("random_book_one", "one"), ("random_book_one", "3-7-rest"), ("random_book_one", "over"),
    ("cornell", "all"), ("cornell", "3-7-rest"), ("cornell", "over"),
    ("cornell_smoke", "all"), ("cornell_smoke", "one"), ("cornell_smoke", "3-7-rest"), ("cornell_smoke", "over"),
    ("next_week_final", "all"), ("next_week_final", "3-7-rest"), ("next_week_final", "over"),
    ("stress_spheres", "all"), ("stress_spheres", "3-7-rest"), ("stress_spheres", "over"),
])
def test_complete_frame_equals_rt_render(gpu_ctx, name, pattern):
    check_shape(S2)
    ref = reference(gpu_ctx, name, S2)
    cam, p = setup(gpu_ctx, name, S2)
    if name == "stress_spheres":  # the global-memory kernel family, in rt_render and in the frame's launches
        gpu_ctx.render(cam, p)
        assert gpu_ctx.last_launch()["lds_staged"] == 0
    steps = PATTERNS[pattern] or [1] * 20
    with gpu_ctx.open_frame(cam, p) as fr:
        assert (fr.chunk, fr.chunks_total) == CHUNKS[S2]
        done = run_steps(fr, steps)
        assert sum(done) == 20 and fr.complete
        if pattern == "over":
            assert done == [5, 15]
        if name == "stress_spheres":
            assert gpu_ctx.last_launch()["lds_staged"] == 0
        rgb, lin, st = fr.resolve()
        assert st["chunks_done"] == 20 and st["samples_done"] == 99
        assert same((rgb, lin), ref)


@pytest.mark.parametrize("shape, pattern", [(S3, "all"), (S3, "one"), (S3, "3-7-rest"), (S3, "over"), (S1, "all"),
                                            (S1, "one"), (S1, "3-7-rest"), (S1, "over")])
def test_complete_frame_other_shapes(gpu_ctx, shape, pattern):
    check_shape(shape)
    ref = reference(gpu_ctx, "random_book_one", shape)
    cam, p = setup(gpu_ctx, "random_book_one", shape)
    total = CHUNKS[shape][1]
    steps = PATTERNS[pattern] or [1] * total
    with gpu_ctx.open_frame(cam, p) as fr:
        done = run_steps(fr, steps)
        assert sum(done) == total and fr.complete
        if shape == S3 and pattern == "3-7-rest":  # (8 chunks: the 7 over-asks, and nothing is left for the rest)
            assert done == [3, 5, 0]
        if pattern == "over":
            assert done == ([5, 3] if shape == S3 else [5, 35])
        assert same(fr.resolve()[:2], ref)


@pytest.mark.parametrize("flag", [rtamd.RT_FLAG_NAN_ZERO, rtamd.RT_FLAG_NAN_CULL])
def test_complete_frame_with_nan_flags(gpu_ctx, flag):
    check_shape(S2)
    ref = reference(gpu_ctx, "cornell", S2, flags=flag)
    cam, p = setup(gpu_ctx, "cornell", S2, flags=flag)
    with gpu_ctx.open_frame(cam, p) as fr:
        run_steps(fr, [3, 7, "rest"])
        assert same(fr.resolve()[:2], ref)


@pytest.mark.parametrize("shape, ks", [(S1, (1, 2, 7, 39, 40)), (S2, (18, 19)), (S3, (3, 5, 7))])
def test_preview_equals_rt_render_at_that_sample_count(gpu_ctx, shape, ks):
    check_shape(shape)
    w, h, _ = shape
    ch = CHUNKS[shape][0]
    for k in ks:  # rt_render at k * CH samples sums the same chunks only if its chunk size is the frame's
        assert rtamd.sample_chunk(w * h, k * ch) == ch
    refs = {k: reference(gpu_ctx, "random_book_one", shape, spp=k * ch) for k in ks}
    cam, p = setup(gpu_ctx, "random_book_one", shape)
    with gpu_ctx.open_frame(cam, p) as fr:
        for k in ks:
            fr.advance(k - fr.chunks_done)
            rgb, lin, st = fr.resolve()
            assert st["chunks_done"] == k and st["samples_done"] == k * ch
            assert same((rgb, lin), refs[k]), k


def test_preview_against_the_oracle(gpu_ctx):
    check_shape(S1)
    assert rtamd.sample_chunk(96 * 64, 7) == 1
    cam, p = setup(gpu_ctx, "cornell", S1)
    with gpu_ctx.open_frame(cam, p) as fr:
        fr.advance(7)
        rgb, lin, _ = fr.resolve()
    _, p7 = setup(gpu_ctx, "cornell", S1, spp=7)
    rgb_o, lin_o, _, _ = pyoracle.render(scene_of("cornell"), cam, p7)
    ok, eq, dmax = parity(lin, lin_o, rgb, rgb_o)
    print(f"preview at 7 of 40 samples vs the oracle at 7 spp: within 1e-3 {ok:.6f}, bytes equal {eq:.6f}, max |d| {dmax:.3g}")
    assert ok >= 0.999 and eq >= 0.999


def test_stats(gpu_ctx):
    check_shape(S2)
    cam, p = setup(gpu_ctx, "cornell", S2)
    with gpu_ctx.open_frame(cam, p) as fr:
        prev = np.zeros((192, 256, 3), np.uint8)
        for step, chunks, samples in [(3, 3, 15), (16, 19, 95), (1, 20, 99)]:  # (the last chunk is short)
            assert fr.advance(step) == step
            polled = fr.stats()  # null image pointers: the same stats as the resolve that fetches the images
            rgb, lin, st = fr.resolve()
            assert polled == st
            assert (st["chunk"], st["chunks_total"], st["chunks_done"], st["samples_done"]) == (5, 20, chunks, samples)
            assert st["nan_pixels"] == int(np.isnan(lin).any(axis=2).sum())
            assert st["bytes_changed"] == int((prev != rgb).sum())
            assert st["kernel_ms"] > 0
            # NaN pixels are permanent and their bytes are 0
            assert (rgb[np.isnan(lin)] == 0).all()
            prev = rgb
        assert fr.advance(1) == 0
    # a scene without NaN pixels counts none
    cam, p = setup(gpu_ctx, "random_book_one", S1)
    with gpu_ctx.open_frame(cam, p) as fr:
        fr.advance(2)
        rgb, lin, st = fr.resolve()
        assert st["nan_pixels"] == int(np.isnan(lin).any(axis=2).sum())
        assert st["bytes_changed"] == int((rgb != 0).sum())


def test_interleaved_calls_leave_the_frame_alone(gpu_ctx, monkeypatch):
    check_shape(S2)
    monkeypatch.delenv("RTAMD_PARTIAL_CAP", raising=False)
    ref = reference(gpu_ctx, "random_book_one", S2)
    cam, p = setup(gpu_ctx, "random_book_one", S2)
    # the other render: 128x96 at 24 spp is 24 chunks of 1 sample; with the chunk sums capped at two
    # chunks' bytes it takes rt_render's own multi-batch path (12 launches folded through the ctx's sums)
    assert rtamd.sample_chunk(128 * 96, 24) == 1
    ocam = rtamd.camera("random_scene", 128, 96)
    op = rtamd.make_params(128, 96, 24, DEPTH, rtamd.RT_RNG_PHILOX, seed=5)
    alone = gpu_ctx.render(ocam, op, linear=True)
    assert gpu_ctx.last_launch()["chunk_batches"] == 1
    rays = np.zeros((256, 7))
    rays[:, :3] = (13.0, 2.0, 3.0)
    rays[:, 3:6] = np.random.default_rng(3).normal(size=(256, 3)) - np.array([13.0, 2.0, 3.0])
    hits_alone = gpu_ctx.closest_hits(rays, 1e-3, 1e30)
    with gpu_ctx.open_frame(cam, p) as fr:
        fr.advance(3)
        monkeypatch.setenv("RTAMD_PARTIAL_CAP", str(2 * 128 * 96 * 24))
        between = gpu_ctx.render(ocam, op, linear=True)
        assert gpu_ctx.last_launch()["chunk_batches"] == 12
        monkeypatch.delenv("RTAMD_PARTIAL_CAP")
        hits = gpu_ctx.closest_hits(rays, 1e-3, 1e30)
        fr.advance(1000)
        assert same(fr.resolve()[:2], ref)
    assert same(between[:2], alone[:2])
    assert np.array_equal(hits, hits_alone, equal_nan=True)


def test_a_step_is_split_into_launches(gpu_ctx, monkeypatch):
    check_shape(S2)
    monkeypatch.delenv("RTAMD_PARTIAL_CAP", raising=False)
    ref = reference(gpu_ctx, "cornell_smoke", S2)
    cam, p = setup(gpu_ctx, "cornell_smoke", S2)
    monkeypatch.setenv("RTAMD_PARTIAL_CAP", str(2 * 256 * 192 * 24))  # two chunks' sums per launch
    with gpu_ctx.open_frame(cam, p) as fr:
        assert fr.advance(5) == 5
        assert gpu_ctx.last_launch()["chunk_batches"] == 3
        assert fr.advance(1000) == 15
        assert gpu_ctx.last_launch()["chunk_batches"] == 8
        assert same(fr.resolve()[:2], ref)


def test_two_frames_open_at_once(gpu_ctx):
    check_shape(S2)
    check_shape(S1)
    ref2, ref1 = reference(gpu_ctx, "random_book_one", S2), reference(gpu_ctx, "random_book_one", S1)
    cam2, p2 = setup(gpu_ctx, "random_book_one", S2)
    cam1, p1 = setup(gpu_ctx, "random_book_one", S1)
    with gpu_ctx.open_frame(cam2, p2) as a, gpu_ctx.open_frame(cam1, p1) as b:
        while not (a.complete and b.complete):
            a.advance(3)
            b.advance(7)
        assert same(b.resolve()[:2], ref1)
        assert same(a.resolve()[:2], ref2)


def test_save_and_restore(gpu_ctx):
    check_shape(S2)
    ref = reference(gpu_ctx, "cornell_smoke", S2)
    cam, p = setup(gpu_ctx, "cornell_smoke", S2)
    with gpu_ctx.open_frame(cam, p) as fr:
        fr.advance(7)
        part = fr.resolve()
        blob = fr.save()
    info = rtamd.blob_info(blob)
    assert len(blob) == 288 + 256 * 192 * 24 and info["chunks_done"] == 7 and info["samples_done"] == 35
    assert (info["width"], info["height"], info["spp"], info["max_depth"], info["seed"]) == (256, 192, 99, DEPTH, 77)
    assert info["chunk"] == 5 and info["chunks_total"] == 20
    assert info["scene_fingerprint"] == rtamd.scene_fingerprint(scene_of("cornell_smoke"))
    assert bytes(info["camera"]) == bytes(cam)
    other = rtamd.Context(0)
    try:
        with pytest.raises(rtamd.RTError, match=E_STATE):  # no scene yet
            other.restore_frame(blob)
        other.upload(scene_of("cornell"))
        with pytest.raises(rtamd.RTError, match=E_STATE):  # another scene
            other.restore_frame(blob)
        other.upload(scene_of("cornell_smoke"))
        with pytest.raises(rtamd.RTError, match=E_INVALID):
            other.restore_frame(blob[:-1])
        with pytest.raises(rtamd.RTError, match=E_INVALID):
            other.restore_frame(blob[:200])
        with other.restore_frame(blob) as fr:
            assert fr.chunks_done == 7 and not fr.complete
            rgb, lin, st = fr.resolve()  # the saved preview again; a restored frame's first resolve compares with zeros
            assert same((rgb, lin), part[:2]) and st["bytes_changed"] == int((rgb != 0).sum())
            assert fr.advance(1000) == 13
            assert same(fr.resolve()[:2], ref)
    finally:
        other.close()


def test_state_errors(gpu_ctx):
    check_shape(S1)
    cam, p = setup(gpu_ctx, "random_book_one", S1)
    tier_a = rtamd.make_params(96, 64, 40, DEPTH, rtamd.RT_RNG_EXACT)
    with pytest.raises(rtamd.RTError, match=E_UNSUPPORTED):
        gpu_ctx.open_frame(cam, tier_a)
    fr = gpu_ctx.open_frame(cam, p)
    with pytest.raises(rtamd.RTError, match=E_STATE):
        fr.resolve()
    assert fr.advance(40) == 40 and fr.advance(1) == 0 and fr.advance(0) == 0
    fr.resolve()
    gpu_ctx.upload(scene_of("random_book_one"))  # any upload ends the ctx's open frames
    for call in (lambda: fr.advance(1), fr.resolve, fr.save):
        with pytest.raises(rtamd.RTError, match=E_STATE):
            call()
    fr.close()
    fr.close()


@pytest.mark.parametrize("w, h", [(1, 1), (17, 13)])
def test_edge_sizes(gpu_ctx, w, h):
    assert rtamd.sample_chunk(w * h, 3) == 1
    gpu_ctx.upload(scene_of("random_book_one"))
    cam = rtamd.camera("random_scene", w, h)
    p = rtamd.make_params(w, h, 3, DEPTH, rtamd.RT_RNG_PHILOX, seed=3)
    ref = gpu_ctx.render(cam, p, linear=True)
    with gpu_ctx.open_frame(cam, p) as fr:
        assert fr.chunks_total == 3
        assert [fr.advance(1), fr.advance(1), fr.advance(1), fr.advance(1)] == [1, 1, 1, 0]
        assert same(fr.resolve()[:2], ref[:2])


def test_reopen_after_close(gpu_ctx):
    check_shape(S1)
    ref = reference(gpu_ctx, "random_book_one", S1)
    cam, p = setup(gpu_ctx, "random_book_one", S1)
    before = rtamd.lib().rt_last_error()  # (the thread's last failure, if any: nothing below may add one)
    gpu_ctx.open_frame(cam, p).close()
    with gpu_ctx.open_frame(cam, p) as fr:
        fr.advance(40)
        out = fr.resolve()
    with gpu_ctx.open_frame(cam, p) as fr:
        fr.advance(40)
        assert same(fr.resolve()[:2], out[:2]) and same(out[:2], ref)
    assert rtamd.lib().rt_last_error() == before


def test_render_progressive_runs_to_completion_or_stops(gpu_ctx):
    check_shape(S2)
    ref = reference(gpu_ctx, "random_book_one", S2)
    cam, p = setup(gpu_ctx, "random_book_one", S2)
    steps = list(rtamd.render_progressive(gpu_ctx, cam, p, 8))
    assert [s["chunks_done"] for _, s in steps] == [8, 16, 20]
    assert np.array_equal(steps[-1][0], ref[0])
    # every byte counts as changed at most once per step: a fraction of 1 stops after the first step
    assert len(list(rtamd.render_progressive(gpu_ctx, cam, p, 8, stop_changed_fraction=1.0))) == 1
