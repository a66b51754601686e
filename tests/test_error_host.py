"""Per-pixel error estimates of progressive frames without a GPU (include/rt.h, RT_FRAME_MOMENTS): the
bindings, rt_error_estimate against a numpy transcription of rt.h's definition bit for bit, its edge
cases, the error stop rule of rtamd.render_progressive over a stub frame, and the host function under
AddressSanitizer + UBSan in a stand-alone C program (tests/c/error_estimate_check.c)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rtamd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def reference(S, Q, K, N, abs_tol=0.0, rel_tol=0.0):
    """rt.h's definition in numpy, operation by operation (IEEE fp64, no contraction): the map, and the
    stats with mean_se as the sequential sum in pixel and channel order."""
    S, Q = np.asarray(S, np.float64).reshape(-1, 3), np.asarray(Q, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        t = (S * S) / np.float64(N)
        d = Q - t
        d = np.where(d < 0, 0.0, d)
        se = np.sqrt((d / np.float64(K - 1)) / np.float64(N))
        finite = np.isfinite(se).all(axis=1)
        conv = (se <= abs_tol + rel_tol * np.abs(S / np.float64(N))).all(axis=1)
    total = 0.0
    for v in se[finite].reshape(-1):
        total = total + float(v)
    n = int(finite.sum())
    return se, {"chunks_done": K, "samples_done": N, "pixels": len(S), "nonfinite_pixels": len(S) - n,
                "unconverged_pixels": int((finite & ~conv).sum()),
                "max_se": float(se[finite].max()) if n else 0.0, "mean_se": total / (3 * n) if n else 0.0}


def folded(chunk_sums, n_k):
    """(S, Q, N) from chunk sums [K, pixels, 3] and sample counts n_k, added in chunk order as rt.h adds them."""
    S, Q = np.zeros(chunk_sums.shape[1:]), np.zeros(chunk_sums.shape[1:])
    with np.errstate(all="ignore"):
        for x, n in zip(chunk_sums, n_k):
            S = S + x
            Q = Q + (x * x) / np.float64(n)
    return S, Q, int(sum(n_k))


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def test_bindings_sizes_and_null_handles():
    L = rtamd.lib()
    assert L.rt_abi_version() == 1
    for name in ("rt_frame_open_ex", "rt_frame_moments", "rt_frame_restore_ex", "rt_frame_error", "rt_error_estimate"):
        assert hasattr(L, name) and name in rtamd.EXPORTED
    assert C.sizeof(rtamd.rt_error_tol) == 16 and C.sizeof(rtamd.rt_error_stats) == 48
    assert C.sizeof(rtamd.rt_frame_stats) == 40 and C.sizeof(rtamd.rt_frame_blob_desc) == 288
    assert rtamd.RT_FRAME_MOMENTS == 1
    for attr in ("moments", "error"):
        assert hasattr(rtamd.ProgressiveFrame, attr)
    assert callable(rtamd.error_estimate)
    # null handles are argument errors, not crashes
    h = C.c_void_p()
    assert L.rt_frame_open_ex(None, None, None, rtamd.RT_FRAME_MOMENTS, C.byref(h)) == rtamd.RT_E_INVALID
    assert L.rt_frame_open_ex(None, None, None, 0, None) == rtamd.RT_E_INVALID
    assert L.rt_frame_moments(None, None) == rtamd.RT_E_INVALID
    assert L.rt_frame_error(None, None, None, None) == rtamd.RT_E_INVALID
    assert L.rt_frame_restore_ex(None, None, 0, None, None) == rtamd.RT_E_INVALID
    assert L.rt_error_estimate(None, None, 1, 2, 2, None, None, None) == rtamd.RT_E_INVALID


def test_bad_arguments_are_invalid():
    s = np.ones((4, 3))
    for tol in [(-1.0, 0.0), (0.0, -1e-300), (float("nan"), 0.0), (0.0, float("nan"))]:
        with pytest.raises(rtamd.RTError, match=r"\(-1\)"):
            rtamd.error_estimate(s, s, 2, 8, *tol)
    for k, n in [(0, 8), (1, 8), (-3, 8), (3, 2)]:
        with pytest.raises(rtamd.RTError, match=r"\(-1\)"):
            rtamd.error_estimate(s, s, k, n)
    L = rtamd.lib()
    P = C.POINTER(C.c_double)
    for pixels in (0, -1):
        assert L.rt_error_estimate(s.ctypes.data_as(P), s.ctypes.data_as(P), pixels, 2, 8, None, None, None) == rtamd.RT_E_INVALID
    assert b"rt_error_estimate" in L.rt_last_error()
    # a null tolerance is {0, 0}; null outputs are allowed
    st = rtamd.rt_error_stats()
    assert L.rt_error_estimate(s.ctypes.data_as(P), s.ctypes.data_as(P), 4, 2, 8, None, None, C.byref(st)) == rtamd.RT_OK
    assert st.pixels == 4 and st.chunks_done == 2 and st.samples_done == 8


@pytest.mark.parametrize("pixels, n_k, tol", [
    (1, [5, 4], (0.0, 0.0)),
    (257, [5] * 19 + [4], (0.0, 0.0)),
    (1000, [8, 8, 8, 3], (0.05, 0.0)),
    (777, [1] * 40, (0.0, 0.1)),
    (4099, [5] * 6 + [2], (0.01, 0.02)),
])
def test_estimate_equals_the_numpy_transcription_bit_for_bit(pixels, n_k, tol):
    rng = np.random.default_rng(pixels)
    # per-sample means differ per pixel by orders of magnitude; each chunk's sum scales with its n_k
    scale = 10.0 ** rng.uniform(-3, 2, size=(1, pixels, 3))
    x = rng.random((len(n_k), pixels, 3)) * scale * np.asarray(n_k, np.float64).reshape(-1, 1, 1)
    S, Q, N = folded(x, n_k)
    se, st = rtamd.error_estimate(S, Q, len(n_k), N, *tol)
    ref_se, ref_st = reference(S, Q, len(n_k), N, *tol)
    assert same_bits(se, ref_se)
    assert st == ref_st  # the counts exactly; max_se and the sequential mean_se bit for bit
    assert st["nonfinite_pixels"] == 0 and st["max_se"] > 0
    if tol != (0.0, 0.0) and pixels > 1:
        assert 0 < st["unconverged_pixels"] < pixels  # (the tolerance splits the pixels: both sides are exercised)
    # image-shaped input gives an image-shaped map
    if pixels == 1000:
        se2, st2 = rtamd.error_estimate(S.reshape(25, 40, 3), Q.reshape(25, 40, 3), len(n_k), N, *tol)
        assert se2.shape == (25, 40, 3) and same_bits(se2.reshape(-1, 3), se) and st2 == st


def test_edge_cases():
    n_k = [5, 5, 5, 4]
    # a constant pixel: every sample the same value, so every chunk sum is value * n_k and d is exactly 0
    x = np.array([0.25, 1.0, 3.0]).reshape(1, 1, 3) * np.asarray(n_k, np.float64).reshape(-1, 1, 1)
    S, Q, N = folded(x, n_k)
    se, st = rtamd.error_estimate(S, Q, 4, N)
    assert (se == 0).all() and st["max_se"] == 0 and st["mean_se"] == 0 and st["unconverged_pixels"] == 0
    # d slightly negative (Q one ulp below S*S/N) clamps to se = 0 instead of NaN
    t = (3.0 * 3.0) / 7.0
    se, st = rtamd.error_estimate([[3.0, 3.0, 3.0]], [[np.nextafter(t, 0), t, np.nextafter(t, 10)]], 2, 7)
    assert se[0, 0] == 0 and se[0, 1] == 0 and se[0, 2] > 0 and st["nonfinite_pixels"] == 0
    # a NaN or inf channel makes its pixel non-finite: out of max, mean and the unconverged count
    S = np.array([[4.0, 4, 4], [np.nan, 4, 4], [4, np.inf, 4], [4, 4, 4]])
    Q = np.array([[10.0, 10, 10], [np.nan, 10, 10], [10, np.inf, 10], [10, 10, np.inf]])
    se, st = rtamd.error_estimate(S, Q, 2, 2)
    ref_se, ref_st = reference(S, Q, 2, 2)
    assert np.array_equal(se, ref_se, equal_nan=True) and st == ref_st
    assert (se[0] == 1.0).all() and np.isnan(se[1, 0]) and se[1, 1] == 1.0 and np.isnan(se[2, 1]) and np.isinf(se[3, 2])
    assert st["nonfinite_pixels"] == 3 and st["unconverged_pixels"] == 1 and st["max_se"] == 1.0 and st["mean_se"] == 1.0
    # convergence is <=: se = 1 against abs_tol 1, rel_tol 0.5 * |mean 2|, and 0.5 + 0.25 * 2
    for tol, open_pixels in [((1.0, 0.0), 0), ((float(np.nextafter(1.0, 0)), 0.0), 1), ((0.0, 0.5), 0),
                             ((0.0, float(np.nextafter(0.5, 0))), 1), ((0.5, 0.25), 0)]:
        st = rtamd.error_estimate(S, Q, 2, 2, *tol)[1]
        assert st["unconverged_pixels"] == open_pixels and st["nonfinite_pixels"] == 3, tol
    # no finite pixel at all: both summaries are 0
    st = rtamd.error_estimate(S[1:], Q[1:], 2, 2)[1]
    assert st["nonfinite_pixels"] == 3 and st["unconverged_pixels"] == 0 and st["max_se"] == 0 and st["mean_se"] == 0


class StubFrame:
    """A frame whose error stats per step are scripted: render_progressive's error rule without a device."""

    def __init__(self, total, unconverged, pixels=16, nonfinite=4, changed=48):
        self.total, self.done, self.unconverged, self.steps, self.closed = total, 0, list(unconverged), [], False
        self.pixels, self.nonfinite, self.changed, self.error_calls = pixels, nonfinite, changed, []

    @property
    def complete(self):
        return self.done >= self.total

    def advance(self, n):
        n = min(n, self.total - self.done)
        self.done += n
        self.steps.append(n)
        return n

    def resolve(self, rgb=True, linear=True):
        assert not linear
        return np.full((4, 4, 3), self.done, np.uint8), None, {"chunks_done": self.done, "bytes_changed": self.changed}

    def error(self, abs_tol=0.0, rel_tol=0.0, want_map=True):
        assert self.done >= 2 and not want_map
        self.error_calls.append((self.done, abs_tol, rel_tol))
        return None, {"chunks_done": self.done, "samples_done": self.done, "pixels": self.pixels,
                      "nonfinite_pixels": self.nonfinite, "unconverged_pixels": self.unconverged[len(self.steps) - 1],
                      "max_se": 0.5, "mean_se": 0.25}

    def close(self):
        self.closed = True


class TrackedCtx:
    def __init__(self, frame):
        self.frame, self.opened = frame, []

    def open_frame(self, cam, params, moments=False):
        self.opened.append(moments)
        return self.frame


class TwoArgumentCtx:
    def __init__(self, frame):
        self.frame = frame

    def open_frame(self, cam, params):
        return self.frame


def test_render_progressive_error_stop_rule():
    p = rtamd.make_params(4, 4, 40, 5)  # 16 pixels, 4 of them non-finite in the stub: 12 finite
    # stops at the first step at the bound (3 <= 0.25 * 12), yielding it, with the error stats merged in
    fr = StubFrame(20, [12, 9, 3, 0, 0])
    ctx = TrackedCtx(fr)
    out = list(rtamd.render_progressive(ctx, None, p, 2, stop_unconverged_fraction=0.25, abs_tol=0.05, rel_tol=0.01))
    assert ctx.opened == [True] and fr.steps == [2, 2, 2] and len(out) == 3 and fr.closed
    assert fr.error_calls == [(2, 0.05, 0.01), (4, 0.05, 0.01), (6, 0.05, 0.01)]
    assert out[2][1]["unconverged_pixels"] == 3 and out[2][1]["bytes_changed"] == 48 and out[2][1]["mean_se"] == 0.25
    assert out[0][1]["pixels"] == 16 and out[0][1]["nonfinite_pixels"] == 4
    # just above the bound (4 > 3): goes on to completion
    fr = StubFrame(6, [12, 4, 4])
    assert len(list(rtamd.render_progressive(TrackedCtx(fr), None, p, 2, stop_unconverged_fraction=0.25))) == 3
    # not before chunks_done >= 2: single-chunk steps ask for no estimate after the first, which cannot stop
    fr = StubFrame(10, [0] * 10)
    out = list(rtamd.render_progressive(TrackedCtx(fr), None, p, 1, stop_unconverged_fraction=1.0))
    assert fr.steps == [1, 1] and fr.error_calls == [(2, 0.0, 0.0)]
    assert "unconverged_pixels" not in out[0][1] and out[1][1]["unconverged_pixels"] == 0
    # fraction 0: only when no finite pixel is left unconverged
    fr = StubFrame(100, [5, 1, 0, 7])
    assert len(list(rtamd.render_progressive(TrackedCtx(fr), None, p, 2, stop_unconverged_fraction=0.0))) == 3
    # both rules given: either one stops (here the bytes, at the first step)
    fr = StubFrame(10, [12] * 5, changed=0)
    out = list(rtamd.render_progressive(TrackedCtx(fr), None, p, 2, stop_changed_fraction=0.0, stop_unconverged_fraction=0.0))
    assert len(out) == 1 and fr.closed
    fr = StubFrame(10, [12, 0, 0, 0, 0])
    out = list(rtamd.render_progressive(TrackedCtx(fr), None, p, 2, stop_changed_fraction=0.0, stop_unconverged_fraction=0.0))
    assert len(out) == 2
    # the new keywords are keyword-only
    with pytest.raises(TypeError):
        list(rtamd.render_progressive(TrackedCtx(StubFrame(4, [0] * 4)), None, p, 2, None, 0.5))


def test_render_progressive_without_the_keyword_opens_an_untracked_frame():
    p = rtamd.make_params(4, 4, 40, 5)
    fr = StubFrame(6, [0] * 3)
    out = list(rtamd.render_progressive(TwoArgumentCtx(fr), None, p, 2))  # open_frame(cam, params), nothing else
    assert fr.steps == [2, 2, 2] and fr.error_calls == [] and len(out) == 3
    assert all("unconverged_pixels" not in s for _, s in out)
    # abs_tol / rel_tol alone select nothing
    fr = StubFrame(4, [0] * 2)
    assert len(list(rtamd.render_progressive(TwoArgumentCtx(fr), None, p, 2, abs_tol=1.0, rel_tol=1.0))) == 2
    assert fr.error_calls == []


def test_error_estimate_is_sanitizer_clean(tmp_path):
    """tests/c/error_estimate_check.c with the host-only unit under ASan + UBSan, as a child process: the edge
    cases above and every pixel count up to 64 over heap blocks of exactly pixels * 3 doubles."""
    csrc = os.path.join(ROOT, "ray-tracing_amd", "csrc")
    exe = str(tmp_path / "error_estimate_check")
    obj = str(tmp_path / "error_estimate_check.o")
    # (the sanitizer runtimes linked into the program itself: it needs nothing from its environment)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1",
           "-static-libasan", "-static-libubsan"]
    fp = ["-ffp-contract=off", "-fno-fast-math"]
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + csrc]
    subprocess.run(["gcc", "-std=c11", "-Wall", *san, *fp, *inc, "-c",
                    os.path.join(ROOT, "tests", "c", "error_estimate_check.c"), "-o", obj], check=True, timeout=300)
    # (rt_scene.cpp: rt_last_error / set_error; both units are C++, so the link goes through g++'s runtime)
    subprocess.run(["gcc", "-std=c++17", "-Wall", *san, *fp, *inc, obj, os.path.join(csrc, "rt_frame_error.cpp"),
                    os.path.join(csrc, "rt_scene.cpp"), "-lstdc++", "-lm", "-o", exe], check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    print(r.stdout[-4000:], r.stderr[-4000:])
    assert r.returncode == 0, r.stderr[-2000:]
    assert "error_estimate_check: clean (0 failures)" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
