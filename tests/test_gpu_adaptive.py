"""Adaptive progressive tier-B frames on the GPU (include/rt.h: rt_frame_adapt, rt_frame_stop,
rt_frame_chunk_counts): a stopped pixel keeps the sums of its first K_p chunks bit for bit, the NaN rule loses
nothing of rt_render's image, steps / batching / interleaved calls do not matter, every kernel form reads the
skip mask, the error estimate runs per pixel at (K_p, N_p), and render_progressive(adaptive=True).

The reference in every test is an UNADAPTED frame of the same parameters, with previews, sums and moments
taken at the stop points; the expected K_p maps come from rt_adapt_decide (host) over those.

Shapes (every test asserts its chunking first):
    S2   256x192 spp 99  CH 5  20 chunks, the last of 4 samples
    T    64x48   spp 6   CH 1   6 chunks, depth 8 (the five worlds of tests/test_gpu_launch_const.py)
    P    97x61   spp 12  CH 1  12 chunks, tile 16: 28 tiles of 256 slab pixels for 5917 image pixels
(S1 96x64x40, CH 1, is the shape of the early-end run of render_progressive.)
"""
import numpy as np
import pytest

import rtamd
import test_gpu_launch_const as lc
from test_error_host import same_bits

pytestmark = pytest.mark.gpu

S1, S2, T, P = (96, 64, 40), (256, 192, 99), (64, 48, 6), (97, 61, 12)
CHUNKS = {S1: (1, 40), S2: (5, 20), T: (1, 6), P: (1, 12)}
E_STATE, E_INVALID = r"\(-5\)", r"\(-1\)"
F_SKIP = 32768  # rt_launch_info.variant: the launch ran a kernel that tests an adaptive frame's skip mask
SCENES = {"random_book_one": "random_scene", "cornell": "cornell", "next_week_final": "next_week",
          "three_spheres": "random_scene"}
_scenes, _cache = {}, {}


def check_shape(shape):
    w, h, spp = shape
    assert rtamd.frame_chunking(w * h, spp) == CHUNKS[shape]


def scene_of(name):
    if name not in _scenes:
        _scenes[name] = rtamd.make_scene(name, rtamd.randGen(1024))[0]
    return _scenes[name]


def setup(ctx, name, shape, depth=10, seed=77, **kw):
    w, h, spp = shape
    ctx.upload(scene_of(name))
    return rtamd.camera(SCENES[name], w, h), rtamd.make_params(w, h, spp, depth, rtamd.RT_RNG_PHILOX, seed=seed, **kw)


def frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


def reference_at(ctx, cam, p, points, moments, key):
    """An unadapted frame of (cam, p) advanced to each of `points` (chunks done): {K: (rgb, linear, resolve
    stats, sums, Q | None)}. Computed once per key and left unchanged."""
    if key not in _cache:
        out = {}
        with ctx.open_frame(cam, p, moments=moments) as fr:
            for k in points:
                n = k - fr.chunks_done
                assert n > 0 and fr.advance(n) == n
                rgb, lin, st = fr.resolve()
                sums = np.frombuffer(fr.save(), dtype="<f8", offset=288).reshape(p.height, p.width, 3).copy()
                out[k] = frozen(rgb, lin, st, sums, fr.moments() if moments else None)
        _cache[key] = out
    return _cache[key]


def expected_at(ref, kp, field):
    """Per pixel, the reference's `field` (0 rgb, 1 linear, 3 sums, 4 Q) at that pixel's K_p."""
    out = np.zeros_like(ref[int(kp.flat[0])][field])
    seen = np.zeros(kp.shape, bool)
    for k in np.unique(kp):
        out[kp == k] = ref[int(k)][field][kp == k]
        seen |= kp == k
    assert seen.all()
    return out


def same_image(rgb, lin, ref, kp):
    return (np.array_equal(rgb, expected_at(ref, kp, 0)) and
            np.array_equal(lin.view(np.uint64), expected_at(ref, kp, 1).view(np.uint64)))


# ------------------------------------------------------------------ 1. the NaN rule loses nothing
@pytest.mark.parametrize("name", ["random_book_one", "next_week_final"])
def test_the_nan_rule_loses_nothing(gpu_ctx, name):
    check_shape(S2)
    cam, p = setup(gpu_ctx, name, S2)
    points = [4, 8, 12, 16, 20]
    ref = reference_at(gpu_ctx, cam, p, points, False, (name, "nan"))
    ref_rgb, ref_lin, _ = gpu_ctx.render(cam, p, linear=True)
    share = np.isnan(ref_lin).any(axis=2).mean()
    print(f"{name}: {share:.3f} of the pixels are NaN at the end")
    assert 0.40 <= share <= 0.99  # (the input condition: the rule has most of the frame to stop, not all)
    with gpu_ctx.open_frame(cam, p) as fr:  # (untracked: the NaN rule needs only S)
        for k in points:
            assert fr.advance(4) == 4
            st = fr.adapt(converged=False)
            print(k, st)
            assert st["stopped_nan"] == ref[k][2]["nan_pixels"] and st["stopped_converged_or_masked"] == 0
            assert st["active_pixels"] == 256 * 192 - st["stopped_nan"] == fr.active_pixels
        assert fr.complete
        rgb, lin, rst = fr.resolve()
        kp = fr.chunk_counts()
    assert np.array_equal(rgb, ref_rgb), "bytes differ from rt_render's"
    assert np.array_equal(lin, ref_lin, equal_nan=True), "the linear image differs from rt_render's"
    assert rst["nan_pixels"] == ref[20][2]["nan_pixels"]
    # a pixel stopped at point k is NaN in the reference preview at k and was not at the point before
    nan_at = {k: np.isnan(ref[k][1]).any(axis=2) for k in points}
    first = np.full(kp.shape, 20, np.int32)
    for k in reversed(points):
        first[nan_at[k]] = k
    assert np.array_equal(kp, first)


# ------------------------------------------------------------------ 2, 3, 6. a stopped pixel is the prefix
POINTS2 = [8, 16, 20]


def cornell_reference(ctx):
    cam, p = setup(ctx, "cornell", S2)
    ref = reference_at(ctx, cam, p, POINTS2, True, ("cornell", "prefix"))
    if ("cornell", "plan") not in _cache:
        se8 = rtamd.error_estimate(ref[8][3], ref[8][4], 8, 40)[0].max(axis=2)
        # abs_tol: the median, over pixels with a positive se, of the max-channel se at 8 chunks
        abs_tol = float(np.median(se8[se8 > 0]))
        k1, _ = rtamd.adapt_decide(ref[8][3], ref[8][4], None, 8, 5, 99, abs_tol, 0.0, 2)
        k2, _ = rtamd.adapt_decide(ref[16][3], ref[16][4], k1, 16, 5, 99, abs_tol, 0.0, 2)
        kp = np.where(k2 == 0, 20, k2).astype(np.int32)
        shares = [(kp == k).mean() for k in POINTS2]
        print(f"abs_tol {abs_tol:.6g}; stopped at 8: {shares[0]:.3f}, at 16: {shares[1]:.3f}, active: {shares[2]:.3f}")
        assert min(shares) >= 0.05  # (the input condition, on the reference-derived map)
        _cache[("cornell", "plan")] = (abs_tol, frozen(kp)[0])
    return (cam, p, ref) + _cache[("cornell", "plan")]


def adaptive_cornell(ctx, cam, p, abs_tol, step, between=None):
    """Test 2's frame: NAN | CONVERGED at 8 and 16 chunks, advanced `step` chunks at a time."""
    with ctx.open_frame(cam, p, moments=True) as fr:
        stats = []
        while not fr.complete:
            fr.advance(min(step, [k for k in POINTS2 if k > fr.chunks_done][0] - fr.chunks_done))
            if between:
                between(fr)
            if fr.chunks_done in (8, 16):
                stats.append(fr.adapt(abs_tol, 0.0, 2))
        rgb, lin, _ = fr.resolve()
        return frozen(fr.chunk_counts(), fr.moments(), rgb, lin, fr.error(abs_tol, 0.0)) + (stats,)


def cornell_run(ctx):
    cam, p, ref, abs_tol, _ = cornell_reference(ctx)
    if ("cornell", "run") not in _cache:
        _cache[("cornell", "run")] = adaptive_cornell(ctx, cam, p, abs_tol, 8)
    return _cache[("cornell", "run")]


def test_a_stopped_pixel_is_the_prefix(gpu_ctx, monkeypatch):
    check_shape(S2)
    monkeypatch.delenv("RTAMD_PARTIAL_CAP", raising=False)
    cam, p, ref, abs_tol, want_kp = cornell_reference(gpu_ctx)
    kp, q, rgb, lin, _, stats = cornell_run(gpu_ctx)
    assert np.array_equal(kp, want_kp)
    assert same_image(rgb, lin, ref, kp)
    assert same_bits(q, expected_at(ref, kp, 4))
    n8, n16 = int((want_kp == 8).sum()), int((want_kp == 16).sum())
    assert [s["stopped_now"] for s in stats] == [n8, n16]
    assert stats[1]["active_pixels"] == 256 * 192 - n8 - n16 and stats[1]["stopped_nan"] == 0
    assert stats[1]["stopped_converged_or_masked"] == n8 + n16


def test_steps_and_batching_do_not_matter(gpu_ctx, monkeypatch):
    check_shape(S2)
    monkeypatch.delenv("RTAMD_PARTIAL_CAP", raising=False)
    cam, p, ref, abs_tol, _ = cornell_reference(gpu_ctx)
    want = cornell_run(gpu_ctx)

    def same_run(got):
        return (np.array_equal(got[0], want[0]) and same_bits(got[1], want[1]) and np.array_equal(got[2], want[2])
                and same_bits(got[3], want[3]) and same_bits(got[4][0], want[4][0]) and got[4][1] == want[4][1]
                and got[5] == want[5])

    assert same_run(adaptive_cornell(gpu_ctx, cam, p, abs_tol, 1)), "one chunk at a time"
    # several launches per step: the chunk sums capped at two chunks' bytes, 4 batches per 8-chunk step
    monkeypatch.setenv("RTAMD_PARTIAL_CAP", str(2 * 256 * 192 * 24))
    batches = []
    got = adaptive_cornell(gpu_ctx, cam, p, abs_tol, 8, lambda fr: batches.append(gpu_ctx.last_launch()["chunk_batches"]))
    monkeypatch.delenv("RTAMD_PARTIAL_CAP")
    assert batches == [4, 4, 2] and same_run(got), "chunk batches"
    # an rt_render and a second open frame interleaved on the ctx
    ocam = rtamd.camera("cornell", 128, 96)
    op = rtamd.make_params(128, 96, 24, 10, rtamd.RT_RNG_PHILOX, seed=5)
    alone = gpu_ctx.render(ocam, op, linear=True)
    with gpu_ctx.open_frame(ocam, op) as other:
        def between(fr):
            other.advance(3)
            mid = gpu_ctx.render(ocam, op, linear=True)
            assert np.array_equal(mid[0], alone[0]) and np.array_equal(mid[1], alone[1], equal_nan=True)
        got = adaptive_cornell(gpu_ctx, cam, p, abs_tol, 3, between)
        other.advance(1000)
        assert other.complete and np.array_equal(other.resolve()[0], alone[0])
    assert same_run(got), "interleaved calls"


def test_frame_error_on_an_adapted_frame(gpu_ctx, monkeypatch):
    check_shape(S2)
    monkeypatch.delenv("RTAMD_PARTIAL_CAP", raising=False)
    cam, p, ref, abs_tol, want_kp = cornell_reference(gpu_ctx)
    kp, _, _, _, (se, st), _ = cornell_run(gpu_ctx)
    assert np.array_equal(kp, want_kp)
    want_se = np.zeros_like(se)
    nonfinite = unconverged = 0
    for k in POINTS2:  # rt_error_estimate on the host per group of equal K_p, over the reference's sums and Q at K_p
        n = min(99, 5 * k)
        m = kp == k
        g_se, g_st = rtamd.error_estimate(ref[k][3][m], ref[k][4][m], k, n, abs_tol, 0.0)
        want_se[m] = g_se
        nonfinite += g_st["nonfinite_pixels"]
        unconverged += g_st["unconverged_pixels"]
    assert same_bits(se, want_se)
    assert st["pixels"] == 256 * 192 and st["nonfinite_pixels"] == nonfinite and st["unconverged_pixels"] == unconverged
    assert st["chunks_done"] == 20 and st["samples_done"] == 99
    fin = np.isfinite(want_se).all(axis=2)
    total = 0.0
    for v in want_se[fin].reshape(-1):
        total = total + float(v)
    mean = total / (3 * int(fin.sum()))
    print(f"mean_se {st['mean_se']!r} vs sequential {mean!r}; max_se {st['max_se']!r}")
    assert st["max_se"] == want_se[fin].max()
    assert abs(st["mean_se"] - mean) <= 1e-12 * mean  # (rt.h's bound)
    # the pixels stopped at 8 and 16 are converged by construction; none of them counts as unconverged
    assert unconverged <= int((kp == 20).sum())


def test_frame_error_of_a_pixel_stopped_before_two_chunks(gpu_ctx):
    check_shape(T)
    cam, p = setup(gpu_ctx, "three_spheres", T, depth=8)
    ref = reference_at(gpu_ctx, cam, p, [1, 3], True, ("three_spheres", "k1"))
    yy, xx = np.mgrid[0:48, 0:64]
    mask = (xx + yy) % 5 == 0
    with gpu_ctx.open_frame(cam, p, moments=True) as fr:
        fr.advance(1)
        assert fr.stop(mask)["stopped_now"] == int(mask.sum())
        fr.advance(2)
        se, st = fr.error()
        kp = fr.chunk_counts()
    assert np.array_equal(kp, np.where(mask, 1, 3))
    assert np.isnan(se[mask]).all()  # K_p < 2: non-finite
    g_se, g_st = rtamd.error_estimate(ref[3][3][~mask], ref[3][4][~mask], 3, 3)
    assert same_bits(se[~mask], g_se)
    assert st["nonfinite_pixels"] == int(mask.sum()) + g_st["nonfinite_pixels"]
    assert st["unconverged_pixels"] == g_st["unconverged_pixels"] and st["max_se"] == g_st["max_se"]


# ------------------------------------------------------------------ 4. every kernel form reads the mask
def wave_cutting_masks():
    yy, xx = np.mgrid[0:48, 0:64]
    first = (7 * xx + 13 * yy) % 3 == 0
    second = np.zeros((48, 64), bool)
    second[16:24, 40:48] = True  # one whole 8x8 block (one wave of work-items, one word of the mask)
    second[5, 3] = True          # and a single pixel
    return first, second


@pytest.mark.parametrize("name", list(lc.WORLDS))
def test_every_kernel_form_reads_the_mask(gpu_ctx, name, monkeypatch):
    check_shape(T)
    monkeypatch.delenv("RTAMD_PARTIAL_CAP", raising=False)
    gpu_ctx.upload(lc._scene(name))
    cam = lc._cameras(name)[0]
    p = rtamd.make_params(64, 48, 6, lc.DEPTH, rtamd.RT_RNG_PHILOX, seed=11)
    ref = reference_at(gpu_ctx, cam, p, [2, 4, 5], False, (name, "forms"))
    first, second = wave_cutting_masks()
    assert not first[5, 3] and not first[16:24, 40:48].all()
    want_kp = np.where(first, 2, np.where(second, 4, 5)).astype(np.int32)
    with gpu_ctx.open_frame(cam, p) as fr:
        assert fr.advance(2) == 2
        ll = gpu_ctx.last_launch()
        print(name, ll)
        for k, v in lc.WORLDS[name][1].items():
            assert ll[k] == v, (k, ll)
        assert ll["variant"] & F_SKIP == 0  # no stop call yet: the kernel rt_render runs
        st = fr.stop(first)
        assert st["stopped_now"] == int(first.sum()) and st["active_pixels"] == 64 * 48 - int(first.sum())
        assert fr.advance(2) == 2
        l2 = gpu_ctx.last_launch()  # the same kernel form, in its instantiation that reads the mask
        assert l2["variant"] == ll["variant"] | F_SKIP
        assert all(l2[k] == ll[k] for k in ("loop", "lds_staged", "leaf_lds", "waves", "grid", "block", "dyn_lds_bytes"))
        st = fr.stop(second | first)  # (a pixel already stopped stays as it is and is not counted again)
        assert st["stopped_now"] == int((second & ~first).sum())
        assert fr.advance(1) == 1
        rgb, lin, _ = fr.resolve()
        kp = fr.chunk_counts()
        assert np.array_equal(kp, want_kp)
        assert same_image(rgb, lin, ref, kp)
        nan = np.isnan(expected_at(ref, kp, 3)).any(axis=2) & (kp < 5)
        assert st["stopped_nan"] == int(nan.sum())
        # everything stopped: nothing is rendered, the frame stays where it is
        st = fr.stop(np.ones((48, 64), bool))
        assert st["active_pixels"] == 0 and fr.active_pixels == 0
        assert st["stopped_nan"] + st["stopped_converged_or_masked"] == 64 * 48
        assert fr.advance(1) == 0 and fr.chunks_done == 5 and not fr.complete
        rgb2, lin2, _ = fr.resolve()
        assert np.array_equal(rgb2, rgb) and same_bits(lin2, lin)
        assert np.array_equal(fr.chunk_counts(), want_kp)


# ------------------------------------------------------------------ 5. padding
def test_an_image_smaller_than_its_padded_slab(gpu_ctx):
    check_shape(P)
    cam, p = setup(gpu_ctx, "random_book_one", P, depth=8, tile=16)
    assert rtamd.shard_geometry(p)[2] == 28 * 256 > 97 * 61
    ref = reference_at(gpu_ctx, cam, p, [2, 4], True, ("random_book_one", "padding"))
    all_but_one = np.ones((61, 97), bool)
    all_but_one[60, 96] = False  # the image's last pixel, in a tile that is mostly padding
    with gpu_ctx.open_frame(cam, p, moments=True) as fr:
        fr.advance(2)
        st = fr.stop(all_but_one)
        assert st["stopped_now"] == 97 * 61 - 1 and st["active_pixels"] == 1 and st["pixels"] == 97 * 61
        assert fr.advance(2) == 2
        st = fr.stop(~all_but_one)
        assert st["stopped_now"] == 1 and st["active_pixels"] == 0
        assert fr.advance(5) == 0 and fr.chunks_done == 4
        rgb, lin, rst = fr.resolve()
        kp, q = fr.chunk_counts(), fr.moments()
    assert np.array_equal(kp, np.where(all_but_one, 2, 4))
    assert same_image(rgb, lin, ref, kp) and same_bits(q, expected_at(ref, kp, 4))
    assert st["stopped_nan"] == int(np.isnan(expected_at(ref, kp, 3)).any(axis=2).sum()) == rst["nan_pixels"]


# ------------------------------------------------------------------ 7. errors
def test_errors(gpu_ctx):
    check_shape(T)
    cam, p = setup(gpu_ctx, "three_spheres", T, depth=8)
    L = rtamd.lib()
    import ctypes as C
    h = C.c_void_p()
    assert L.rt_frame_open_ex(gpu_ctx._h, C.byref(cam), C.byref(p), 2, C.byref(h)) == rtamd.RT_E_INVALID
    with gpu_ctx.open_frame(cam, p) as fr:
        for call in (lambda: fr.adapt(converged=False), lambda: fr.stop(np.ones((48, 64), bool))):
            with pytest.raises(rtamd.RTError, match=E_STATE):  # no chunk rendered yet
                call()
        fr.advance(2)
        with pytest.raises(rtamd.RTError, match=E_STATE):  # RT_ADAPT_CONVERGED on a frame without moments
            fr.adapt(1.0)
        for kw in [dict(nan=False, converged=False), dict(abs_tol=-1.0), dict(rel_tol=float("nan")),
                   dict(abs_tol=float("nan"), converged=False)]:
            with pytest.raises(rtamd.RTError, match=E_INVALID):
                fr.adapt(**kw)
        rule = rtamd.rt_adapt_rule(0.0, 0.0, 2, 4)  # an unknown flag bit
        assert L.rt_frame_adapt(fr._h, C.byref(rule), None) == rtamd.RT_E_INVALID
        assert L.rt_frame_adapt(fr._h, None, None) == rtamd.RT_E_INVALID
        assert L.rt_frame_stop(fr._h, None, None) == rtamd.RT_E_INVALID
        assert L.rt_frame_chunk_counts(fr._h, None) == rtamd.RT_E_INVALID
        with pytest.raises(ValueError):
            fr.stop(np.ones((64, 48), bool))
        assert (fr.chunk_counts() == 2).all()  # (no stop call yet: every pixel is active)
        assert len(fr.save()) == 288 + 64 * 48 * 24
        # RT_ADAPT_NAN alone and rt_frame_stop work on an untracked frame; a stop that stops nothing still
        # leaves the frame saveable
        st = fr.adapt(converged=False)
        if st["stopped_now"] == 0:
            assert len(fr.save()) == 288 + 64 * 48 * 24
        one = np.zeros((48, 64), bool)
        one[0, 0] = True
        st = fr.stop(one)
        assert st["stopped_now"] in (0, 1) and st["active_pixels"] < 64 * 48
        with pytest.raises(rtamd.RTError, match=E_STATE):  # the version-1 blob has no room for K_p
            fr.save()
    with gpu_ctx.open_frame(cam, p, moments=True) as fr:
        fr.advance(2)
        for mc in (1, 0, -3):
            with pytest.raises(rtamd.RTError, match=E_INVALID):  # min_chunks < 2 with RT_ADAPT_CONVERGED
                fr.adapt(1.0, min_chunks=mc)
        assert fr.adapt(0.0, min_chunks=1, converged=False)["chunks_done"] == 2  # (not looked at without it)
        q_before = fr.moments()
        assert fr.adapt(1e6)["active_pixels"] == 0
        assert same_bits(fr.moments(), q_before)  # rt_frame_moments still works on an adapted frame
        with pytest.raises(rtamd.RTError, match=E_STATE):
            fr.save()
        gpu_ctx.upload(scene_of("three_spheres"))  # the ctx's scene is replaced: the frame is over
        for call in (lambda: fr.adapt(converged=False), lambda: fr.stop(np.ones((48, 64), bool)), fr.chunk_counts):
            with pytest.raises(rtamd.RTError, match=E_STATE):
                call()


# ------------------------------------------------------------------ 8. render_progressive(adaptive=True)
def test_render_progressive_adaptive(gpu_ctx):
    check_shape(S1)
    cam, p = setup(gpu_ctx, "cornell", S1)
    with gpu_ctx.open_frame(cam, p, moments=True) as fr:
        fr.advance(8)
        se = fr.error()[0].max(axis=2)
    abs_tol = float(np.median(se[se > 0]))
    by_hand = []
    with gpu_ctx.open_frame(cam, p, moments=True) as fr:
        while not fr.complete:
            fr.advance(8)
            rgb, _, st = fr.resolve(linear=False)
            st.update(fr.adapt(abs_tol, 0.01, 4))
            by_hand.append((rgb, st))
            if st["active_pixels"] == 0:
                break
    out = list(rtamd.render_progressive(gpu_ctx, cam, p, 8, adaptive=True, abs_tol=abs_tol, rel_tol=0.01, min_chunks=4))
    assert len(out) == len(by_hand) >= 2
    for (rgb, st), (rgb_h, st_h) in zip(out, by_hand):
        st.pop("kernel_ms"), st_h.pop("kernel_ms")
        assert np.array_equal(rgb, rgb_h) and st == st_h
    print([s["active_pixels"] for _, s in out])
    assert out[0][1]["stopped_now"] > 0
    # every pixel stops at the first step under a large tolerance: the loop ends early
    out = list(rtamd.render_progressive(gpu_ctx, cam, p, 8, adaptive=True, abs_tol=1e6))
    assert len(out) == 1 and out[0][1]["active_pixels"] == 0 and out[0][1]["chunks_done"] == 8
    assert out[0][1]["stopped_now"] == 96 * 64
