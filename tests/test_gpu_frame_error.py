"""Per-pixel error estimates of progressive tier-B frames on the GPU (include/rt.h, RT_FRAME_MOMENTS):
tracking the second moments Q changes no sum, Q is a fixed function of the frame whatever the steps, the
error map and its summary are the host function's bit for bit, the estimate is calibrated against two
independent renders, a tracked frame continues from a blob plus its saved moments, and the error stop rule
of render_progressive runs on the device.

Shapes as in tests/test_gpu_progressive.py (every test asserts the chunking first):
    S1  96x64   spp 40  CH 1  40 chunks
    S2  256x192 spp 99  CH 5  20 chunks, the last of 4 samples (the n_k weighting)
    S3  640x480 spp 60  CH 8   8 chunks, the last of 4 samples
"""
import ctypes as C

import numpy as np
import pytest

import rtamd
from test_error_host import reference as numpy_estimate
from test_error_host import same_bits

pytestmark = pytest.mark.gpu

S1, S2, S3 = (96, 64, 40), (256, 192, 99), (640, 480, 60)
CHUNKS = {S1: (1, 40), S2: (5, 20), S3: (8, 8)}
DEPTH = 10
E_UNSUPPORTED, E_STATE, E_INVALID = r"\(-4\)", r"\(-5\)", r"\(-1\)"
SCENES = {"random_book_one": "random_scene", "cornell": "cornell", "next_week_final": "next_week"}
PATTERNS = {"all": ["rest"], "one": None, "3-7-rest": [3, 7, "rest"]}
_scenes, _cache = {}, {}


def check_shape(shape):
    w, h, spp = shape
    assert rtamd.frame_chunking(w * h, spp) == CHUNKS[shape]


def scene_of(name):
    if name not in _scenes:
        _scenes[name] = rtamd.make_scene(name, rtamd.randGen(1024))[0]
    return _scenes[name]


def setup(ctx, name, shape, seed=77):
    w, h, spp = shape
    ctx.upload(scene_of(name))
    return rtamd.camera(SCENES[name], w, h), rtamd.make_params(w, h, spp, DEPTH, rtamd.RT_RNG_PHILOX, seed=seed)


def run_steps(frame, steps):
    for s in steps or [1] * frame.chunks_total:
        frame.advance(frame.chunks_total - frame.chunks_done if s == "rest" else s)
    assert frame.complete


def sums_of(blob, shape):
    """The running sums a blob holds (rt.h: 288 bytes of header, then 3 f64 per pixel in image order)."""
    w, h, _ = shape
    return np.frombuffer(blob, dtype="<f8", offset=288).reshape(h, w, 3)


def complete_tracked(ctx, name, shape, seed=77):
    """One tracked frame of (scene, shape, seed) advanced in one step, computed once and left unchanged:
    (rgb, linear, resolve stats, blob, moments, error map, error stats)."""
    key = (name, shape, seed)
    if key not in _cache:
        cam, p = setup(ctx, name, shape, seed)
        with ctx.open_frame(cam, p, moments=True) as fr:
            assert fr.tracks_moments
            run_steps(fr, ["rest"])
            rgb, lin, st = fr.resolve()
            out = (rgb, lin, st, fr.save(), fr.moments(), *fr.error())
        for a in out:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


@pytest.mark.parametrize("name", ["cornell", "random_book_one", "next_week_final"])
def test_tracking_does_not_change_the_image(gpu_ctx, name):
    check_shape(S2)
    rgb, lin, st, blob, q, _, _ = complete_tracked(gpu_ctx, name, S2)
    cam, p = setup(gpu_ctx, name, S2)
    ref_rgb, ref_lin, _ = gpu_ctx.render(cam, p, linear=True)
    assert np.array_equal(rgb, ref_rgb) and np.array_equal(lin, ref_lin, equal_nan=True)
    with gpu_ctx.open_frame(cam, p) as fr:
        assert not fr.tracks_moments
        run_steps(fr, ["rest"])
        assert fr.save() == blob
    assert q.shape == (192, 256, 3) and st["samples_done"] == 99


@pytest.mark.parametrize("name, shape, pattern", [
    ("cornell", S2, "one"), ("cornell", S2, "3-7-rest"),
    ("random_book_one", S2, "one"), ("random_book_one", S2, "3-7-rest"),
    ("next_week_final", S2, "one"), ("next_week_final", S2, "3-7-rest"),
    ("random_book_one", S1, "one"), ("random_book_one", S1, "3-7-rest"),
    ("random_book_one", S3, "one"), ("random_book_one", S3, "3-7-rest"),
])
def test_moments_do_not_depend_on_the_steps(gpu_ctx, name, shape, pattern):
    check_shape(shape)
    q_all = complete_tracked(gpu_ctx, name, shape)[4]  # the "all" pattern: one step
    cam, p = setup(gpu_ctx, name, shape)
    with gpu_ctx.open_frame(cam, p, moments=True) as fr:
        run_steps(fr, PATTERNS[pattern])
        assert np.array_equal(fr.moments(), q_all, equal_nan=True)
        assert fr.save() == complete_tracked(gpu_ctx, name, shape)[3]


def test_interleaved_calls_leave_the_moments_alone(gpu_ctx):
    check_shape(S2)
    _, _, _, blob, q_all, se_all, est_all = complete_tracked(gpu_ctx, "random_book_one", S2)
    cam, p = setup(gpu_ctx, "random_book_one", S2)
    ocam = rtamd.camera("random_scene", 128, 96)
    op = rtamd.make_params(128, 96, 24, DEPTH, rtamd.RT_RNG_PHILOX, seed=5)
    rays = np.zeros((256, 7))
    rays[:, :3] = (13.0, 2.0, 3.0)
    rays[:, 3:6] = np.random.default_rng(3).normal(size=(256, 3)) - np.array([13.0, 2.0, 3.0])
    with gpu_ctx.open_frame(cam, p, moments=True) as fr:
        fr.advance(3)
        gpu_ctx.render(ocam, op, linear=True)
        fr.advance(4)
        gpu_ctx.closest_hits(rays, 1e-3, 1e30)
        fr.error()  # (an estimate in the middle changes nothing either)
        fr.advance(1000)
        assert np.array_equal(fr.moments(), q_all, equal_nan=True) and fr.save() == blob
        se, est = fr.error()
        assert np.array_equal(se, se_all, equal_nan=True) and est == est_all


def test_first_chunk_is_exact(gpu_ctx):
    check_shape(S2)
    cam, p = setup(gpu_ctx, "random_book_one", S2)
    with gpu_ctx.open_frame(cam, p, moments=True) as fr:
        fr.advance(1)
        s = sums_of(fr.save(), S2)
        q = fr.moments()
    with np.errstate(invalid="ignore"):
        want = (s * s) / np.float64(5)
    assert np.isfinite(s).any() and (s > 0).any()
    assert np.array_equal(q, want, equal_nan=True)
    finite = np.isfinite(want)
    assert same_bits(q[finite], want[finite])


def test_moments_against_the_running_sums(gpu_ctx):
    """Q against its definition evaluated from the saved running sums R_k after every chunk: the chunk sums
    are recovered as S_k ~ R_k - R_(k-1), and Q_ref = sum_k S_k^2 / n_k in numpy.

    Bound. The radiance is non-negative, so 0 <= R_(k-1) <= R_k <= R_K. The frame computed
    R_k = fl(R_(k-1) + S_k), so R_k - R_(k-1) (exact by Sterbenz or rounded once more) differs from the true
    S_k by at most about ulp(R_k) <= 2^-52 R_K. That moves S_k^2 / n_k by at most 2 |S_k| 2^-52 R_K / n_k,
    over all chunks 2 * 2^-52 * R_K * sum_k |S_k| / n_k. Each of the two K-term evaluations of Q rounds a
    multiply, a divide and K additions of non-negative terms: at most (K + 2) * 2^-53 relative each, together
    (K + 2) * 2^-52 * Q_ref. Both parts are below (K + 2) * 2^-52 * (R_K * sum_k |S_k| / n_k + Q_ref); the
    test allows 4 times that."""
    check_shape(S2)
    cam, p = setup(gpu_ctx, "cornell", S2)
    K = 20
    n_k = [5] * 19 + [4]
    prev = np.zeros((192, 256, 3))
    q_ref, weight = np.zeros_like(prev), np.zeros_like(prev)
    with gpu_ctx.open_frame(cam, p, moments=True) as fr:
        for k in range(K):
            fr.advance(1)
            r = sums_of(fr.save(), S2)
            with np.errstate(invalid="ignore"):
                s_k = r - prev
                q_ref = q_ref + (s_k * s_k) / np.float64(n_k[k])
                weight = weight + np.abs(s_k) / np.float64(n_k[k])
            prev = r
        q = fr.moments()
    assert np.array_equal(np.isnan(q), np.isnan(q_ref))
    ok = np.isfinite(q_ref)
    assert ok.mean() > 0.5 and (q_ref[ok] > 0).any()
    bound = 4 * (K + 2) * 2.0 ** -52 * (np.abs(prev[ok]) * weight[ok] + q_ref[ok])
    err = np.abs(q[ok] - q_ref[ok])
    worst = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0)))
    print(f"|Q - Q_ref| over its bound: worst {worst:.3g}; nonzero errors where the bound is 0: {int((err[bound == 0] != 0).sum())}")
    assert (err <= bound).all()


@pytest.mark.parametrize("name", ["cornell", "random_book_one"])
def test_error_map_and_stats(gpu_ctx, name):
    check_shape(S2)
    cam, p = setup(gpu_ctx, name, S2)
    tol = (0.01, 0.05)
    with gpu_ctx.open_frame(cam, p, moments=True) as fr:
        for chunks, samples in [(7, 35), (20, 99)]:
            fr.advance(chunks - fr.chunks_done)
            se, st = fr.error(*tol)
            again = fr.error(*tol, want_map=False)
            s, q = sums_of(fr.save(), S2), fr.moments()
            host_se, host = rtamd.error_estimate(s, q, chunks, samples, *tol)
            np_se, np_st = numpy_estimate(s, q, chunks, samples, *tol)
            assert se.shape == (192, 256, 3) and again[0] is None
            assert np.array_equal(se, host_se, equal_nan=True) and same_bits(se[np.isfinite(se)], host_se[np.isfinite(se)])
            assert np.array_equal(se, np_se.reshape(se.shape), equal_nan=True)
            for key in ("chunks_done", "samples_done", "pixels", "nonfinite_pixels", "unconverged_pixels", "max_se"):
                assert st[key] == host[key] == np_st[key], key
            assert (st["chunks_done"], st["samples_done"], st["pixels"]) == (chunks, samples, 256 * 192)
            print(f"{name} at {chunks} chunks: mean_se device {st['mean_se']!r} host {host['mean_se']!r}, max_se {st['max_se']!r}, "
                  f"non-finite {st['nonfinite_pixels']}, unconverged {st['unconverged_pixels']}")
            assert abs(st["mean_se"] - host["mean_se"]) <= 1e-12 * host["mean_se"] and host["mean_se"] > 0
            assert again[1] == st  # (mean_se included: the same value on every call)
            assert 0 < st["unconverged_pixels"] < st["pixels"] - st["nonfinite_pixels"]
            # the default tolerance {0, 0}: every finite pixel with any spread is unconverged
            st0 = fr.error(want_map=False)[1]
            assert st0["unconverged_pixels"] == int((np.isfinite(se).all(axis=2) & (se > 0).any(axis=2)).sum())
        nan_pixels = fr.resolve()[2]["nan_pixels"]
        assert st["nonfinite_pixels"] == int((~np.isfinite(se).all(axis=2)).sum())
        if name == "random_book_one":
            assert st["nonfinite_pixels"] >= nan_pixels > 0


def test_error_leaves_the_preview_alone(gpu_ctx):
    check_shape(S2)
    cam, p = setup(gpu_ctx, "cornell", S2)
    results = []
    for ask in (True, False):
        with gpu_ctx.open_frame(cam, p, moments=True) as fr:
            fr.advance(7)
            first = fr.resolve()
            if ask:
                fr.error()
                assert fr.resolve()[2] == first[2]  # (nothing rendered since: the same stats, kernel_ms too)
            fr.advance(1000)
            if ask:
                fr.error(0.01, 0.01)
            rgb, lin, st = fr.resolve()
            results.append((first[2]["bytes_changed"], st["bytes_changed"], rgb, lin))
    assert results[0][:2] == results[1][:2] and results[0][1] > 0
    assert np.array_equal(results[0][2], results[1][2]) and np.array_equal(results[0][3], results[1][3], equal_nan=True)


def test_calibration(gpu_ctx):
    """Two independent renders of one frame (seeds 77 and 78): z^2 = (m_A - m_B)^2 / (se_A^2 + se_B^2) per
    channel is chi-square(1) distributed if se is the standard error of the mean m = S / N; its median is
    0.455. A normalisation wrong by CH = 5 either way moves the median to 0.11 or 2.8: the band is the
    geometric midpoint on each side. Channels with a zero or non-finite denominator (the black surround of
    the box) are left out, at most 40 % of them (the CPU oracle's emulation: 31.4 % left out, median 0.559)."""
    check_shape(S2)
    a = complete_tracked(gpu_ctx, "cornell", S2, seed=77)
    b = complete_tracked(gpu_ctx, "cornell", S2, seed=78)
    m_a, m_b = sums_of(a[3], S2) / 99.0, sums_of(b[3], S2) / 99.0
    with np.errstate(invalid="ignore"):
        den = a[5] * a[5] + b[5] * b[5]
        use = np.isfinite(den) & (den > 0)
        z2 = (m_a[use] - m_b[use]) ** 2 / den[use]
    excluded = 1.0 - use.mean()
    median = float(np.median(z2))
    print(f"calibration: median z^2 {median:.4f} over {int(use.sum())} channels, {excluded:.3%} excluded")
    assert excluded <= 0.40
    assert 0.455 / np.sqrt(5) <= median <= 0.455 * np.sqrt(5)


def test_restore_with_moments(gpu_ctx):
    check_shape(S2)
    rgb, lin, _, blob_end, q_end, se_end, est_end = complete_tracked(gpu_ctx, "random_book_one", S2)
    cam, p = setup(gpu_ctx, "random_book_one", S2)
    with gpu_ctx.open_frame(cam, p, moments=True) as fr:
        fr.advance(7)
        blob, q7 = fr.save(), fr.moments()
        se7, est7 = fr.error(0.01, 0.05)
    other = rtamd.Context(0)
    try:
        other.upload(scene_of("random_book_one"))
        with other.restore_frame(blob, q7) as fr:
            assert fr.tracks_moments and fr.chunks_done == 7
            assert np.array_equal(fr.moments(), q7, equal_nan=True)
            se, est = fr.error(0.01, 0.05)
            assert np.array_equal(se, se7, equal_nan=True) and est == est7
            assert fr.advance(1000) == 13
            assert np.array_equal(fr.moments(), q_end, equal_nan=True) and fr.save() == blob_end
            se, est = fr.error()
            assert np.array_equal(se, se_end, equal_nan=True) and est == est_end
            out = fr.resolve()
            assert np.array_equal(out[0], rgb) and np.array_equal(out[1], lin, equal_nan=True)
        with other.restore_frame(blob) as fr:  # without moments: an untracked frame
            assert not fr.tracks_moments and fr.chunks_done == 7
            for call in (fr.moments, fr.error):
                with pytest.raises(rtamd.RTError, match=E_STATE):
                    call()
            fr.advance(1000)
            assert fr.save() == blob_end
        with pytest.raises(ValueError):
            other.restore_frame(blob, q7[:-1])
    finally:
        other.close()


def test_errors(gpu_ctx):
    check_shape(S1)
    cam, p = setup(gpu_ctx, "random_book_one", S1)
    with gpu_ctx.open_frame(cam, p) as fr:  # untracked
        fr.advance(5)
        for call in (fr.moments, fr.error):
            with pytest.raises(rtamd.RTError, match=E_STATE):
                call()
    with pytest.raises(rtamd.RTError, match=E_UNSUPPORTED):
        gpu_ctx.open_frame(cam, rtamd.make_params(96, 64, 40, DEPTH, rtamd.RT_RNG_EXACT), moments=True)
    h = C.c_void_p()
    L = rtamd.lib()
    for flags in (2, 3, 0x80000000):
        assert L.rt_frame_open_ex(gpu_ctx._h, C.byref(cam), C.byref(p), flags, C.byref(h)) == rtamd.RT_E_INVALID and not h.value
    fr = gpu_ctx.open_frame(cam, p, moments=True)
    with pytest.raises(rtamd.RTError, match=E_STATE):
        fr.moments()  # no chunk yet
    with pytest.raises(rtamd.RTError, match=E_STATE):
        fr.error()
    fr.advance(1)
    fr.moments()
    with pytest.raises(rtamd.RTError, match=E_STATE):
        fr.error()  # one chunk has no spread
    fr.advance(1)
    fr.error()
    for tol in [(-1.0, 0.0), (0.0, float("nan"))]:
        with pytest.raises(rtamd.RTError, match=E_INVALID):
            fr.error(*tol)
    gpu_ctx.upload(scene_of("random_book_one"))  # any upload ends the ctx's open frames
    for call in (fr.moments, fr.error):
        with pytest.raises(rtamd.RTError, match=E_STATE):
            call()
    fr.close()
    fr.close()


def test_stop_rule_on_the_device(gpu_ctx):
    check_shape(S2)
    rgb_end = complete_tracked(gpu_ctx, "cornell", S2)[0]
    cam, p = setup(gpu_ctx, "cornell", S2)
    steps = list(rtamd.render_progressive(gpu_ctx, cam, p, 4, stop_unconverged_fraction=0.5, abs_tol=0.05))
    # the same rule by hand
    want = []
    with gpu_ctx.open_frame(cam, p, moments=True) as fr:
        while not fr.complete:
            fr.advance(4)
            rgb, _, st = fr.resolve(linear=False)
            err = fr.error(0.05, 0.0, want_map=False)[1]
            st.update(err)
            want.append((rgb, st))
            if err["unconverged_pixels"] <= 0.5 * (err["pixels"] - err["nonfinite_pixels"]):
                break
    print("stop rule: chunks_done / unconverged per step", [(s["chunks_done"], s["unconverged_pixels"]) for _, s in steps])
    assert len(steps) == len(want) and 1 <= len(steps) < 5  # (met before completion: 5 steps of 4 chunks)
    for (rgb, st), (rgb_w, st_w) in zip(steps, want):
        assert np.array_equal(rgb, rgb_w)
        assert {k: v for k, v in st.items() if k != "kernel_ms"} == {k: v for k, v in st_w.items() if k != "kernel_ms"}
    last = steps[-1][1]
    assert last["unconverged_pixels"] <= 0.5 * (last["pixels"] - last["nonfinite_pixels"])
    # abs_tol 0: no pixel with any spread converges, the frame runs to its end
    steps = list(rtamd.render_progressive(gpu_ctx, cam, p, 4, stop_unconverged_fraction=0.5))
    assert [s["chunks_done"] for _, s in steps] == [4, 8, 12, 16, 20]
    assert np.array_equal(steps[-1][0], rgb_end)
