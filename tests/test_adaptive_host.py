"""Adaptive progressive frames without a GPU (include/rt.h, rt_frame_adapt / rt_frame_stop): the bindings,
rt_adapt_decide against a numpy restatement of rt.h's rule, its argument checks,
rtamd.render_progressive(adaptive=True) over a stub frame, and the host function under AddressSanitizer +
UBSan in a stand-alone C program (tests/c/adapt_decide_check.c)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rtamd
from test_error_host import folded
from test_error_host import reference as numpy_estimate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = r"\(-1\)"


def numpy_decide(S, Q, chunks_in, K, chunk, spp, abs_tol, rel_tol, min_chunks, nan, converged):
    """rt.h's rule in numpy: an active pixel with a NaN sum channel stops under `nan`; otherwise, under
    `converged`, one with K >= max(2, min_chunks) that the error estimate (test_error_host.reference, rt.h's
    definition operation by operation) calls finite and converged. Returns (K_p map, stats)."""
    S = np.asarray(S, np.float64).reshape(-1, 3)
    kin = np.zeros(len(S), np.int32) if chunks_in is None else np.asarray(chunks_in, np.int32).reshape(-1)
    N = min(spp, K * chunk)
    is_nan = np.isnan(S).any(axis=1)
    stop = is_nan if nan else np.zeros(len(S), bool)
    if converged and K >= max(2, min_chunks):
        Qa = np.asarray(Q, np.float64).reshape(-1, 3)
        with np.errstate(all="ignore"):
            se = numpy_estimate(S, Qa, K, N)[0]
            ok = np.isfinite(se).all(axis=1) & (se <= abs_tol + rel_tol * np.abs(S / np.float64(N))).all(axis=1)
        stop = stop | (ok & ~(is_nan & nan))
    now = stop & (kin == 0)
    out = np.where(kin != 0, kin, np.where(now, K, 0)).astype(np.int32)
    stopped = out != 0
    return out, {"chunks_done": K, "pixels": len(S), "active_pixels": int((~stopped).sum()),
                 "stopped_nan": int((stopped & is_nan).sum()),
                 "stopped_converged_or_masked": int((stopped & ~is_nan).sum()), "stopped_now": int(now.sum())}


def test_bindings_sizes_and_null_handles():
    L = rtamd.lib()
    for name in ("rt_frame_adapt", "rt_frame_stop", "rt_frame_chunk_counts", "rt_adapt_decide"):
        assert hasattr(L, name) and name in rtamd.EXPORTED
    assert C.sizeof(rtamd.rt_adapt_rule) == 24 and C.sizeof(rtamd.rt_adapt_stats) == 48
    assert rtamd.RT_ADAPT_NAN == 1 and rtamd.RT_ADAPT_CONVERGED == 2
    for attr in ("adapt", "stop", "chunk_counts"):
        assert hasattr(rtamd.ProgressiveFrame, attr)
    assert callable(rtamd.adapt_decide)
    # null handles are argument errors, not crashes
    rule = rtamd.rt_adapt_rule(0.0, 0.0, 2, rtamd.RT_ADAPT_NAN)
    mask = (C.c_uint8 * 4)()
    assert L.rt_frame_adapt(None, C.byref(rule), None) == rtamd.RT_E_INVALID
    assert L.rt_frame_adapt(None, None, None) == rtamd.RT_E_INVALID
    assert L.rt_frame_stop(None, mask, None) == rtamd.RT_E_INVALID
    assert L.rt_frame_stop(None, None, None) == rtamd.RT_E_INVALID
    assert L.rt_frame_chunk_counts(None, None) == rtamd.RT_E_INVALID
    assert L.rt_adapt_decide(None, None, None, 1, 2, 1, 8, C.byref(rule), None, None) == rtamd.RT_E_INVALID


def test_bad_arguments_are_invalid():
    s = np.ones((4, 3))
    good = dict(chunks_done=2, chunk=1, spp=8)
    for kw in [dict(abs_tol=-1.0), dict(rel_tol=-1e-300), dict(abs_tol=float("nan")), dict(rel_tol=float("nan")),
               dict(min_chunks=1), dict(min_chunks=0), dict(nan=False, converged=False)]:
        with pytest.raises(rtamd.RTError, match=E_INVALID):
            rtamd.adapt_decide(s, s, None, **good, **kw)
    for kw in [dict(chunks_done=0, chunk=1, spp=8), dict(chunks_done=2, chunk=0, spp=8),
               dict(chunks_done=2, chunk=1, spp=0), dict(chunks_done=4, chunk=5, spp=12)]:
        with pytest.raises(rtamd.RTError, match=E_INVALID):
            rtamd.adapt_decide(s, s, None, **kw)
    with pytest.raises(rtamd.RTError, match=E_INVALID):  # RT_ADAPT_CONVERGED needs the moments
        rtamd.adapt_decide(s, None, None, **good)
    for bad in ([0, 0, 3, 0], [0, -1, 0, 0]):  # a count outside [0, chunks_done]
        with pytest.raises(rtamd.RTError, match=E_INVALID):
            rtamd.adapt_decide(s, s, bad, **good)
    L = rtamd.lib()
    assert b"rt_adapt_decide" in L.rt_last_error()
    rule = rtamd.rt_adapt_rule(0.0, 0.0, 2, 4)  # an unknown flag bit
    out = np.zeros(4, np.int32)
    PD, PI = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    assert L.rt_adapt_decide(s.ctypes.data_as(PD), s.ctypes.data_as(PD), None, 4, 2, 1, 8, C.byref(rule),
                             out.ctypes.data_as(PI), None) == rtamd.RT_E_INVALID
    # min_chunks is not looked at without RT_ADAPT_CONVERGED; moments and chunks_in may then be None
    k, st = rtamd.adapt_decide(s, None, None, **good, min_chunks=0, converged=False)
    assert (k == 0).all() and st["active_pixels"] == 4 and st["stopped_now"] == 0


@pytest.mark.parametrize("pixels, n_k, spp, chunk, tol, min_chunks, flags", [
    (1, [5, 4], 9, 5, (0.0, 0.0), 2, (True, True)),
    (257, [5] * 8, 99, 5, (0.3, 0.0), 2, (True, True)),
    (1000, [8, 8, 8, 3], 27, 8, (0.05, 0.01), 3, (True, True)),
    (777, [1] * 6, 40, 1, (0.0, 0.2), 2, (False, True)),
    (4099, [5] * 3, 99, 5, (0.2, 0.02), 4, (True, True)),   # K < min_chunks: only the NaN rule can stop
    (513, [5] * 4, 99, 5, (0.0, 0.0), 0, (True, False)),
])
def test_decide_equals_the_numpy_restatement(pixels, n_k, spp, chunk, tol, min_chunks, flags):
    rng = np.random.default_rng(pixels)
    scale = 10.0 ** rng.uniform(-3, 1, size=(1, pixels, 3))
    x = rng.random((len(n_k), pixels, 3)) * scale * np.asarray(n_k, np.float64).reshape(-1, 1, 1)
    kinds = rng.integers(0, 8, size=pixels)
    x[:, kinds == 0, :] = x[:1, kinds == 0, :]                    # zero variance: every chunk sum the same
    x[-1, kinds == 1, rng.integers(0, 3)] = np.nan                # a NaN channel
    x[0, kinds == 2, rng.integers(0, 3)] = np.inf                 # an infinite channel
    S, Q, _ = folded(x, n_k)
    K = len(n_k)
    kin = np.where(kinds == 3, rng.integers(1, K + 1, size=pixels), 0).astype(np.int32)  # already stopped
    nan, conv = flags
    for chunks_in in (None, kin):
        got, st = rtamd.adapt_decide(S, Q if conv else None, chunks_in, K, chunk, spp, *tol, min_chunks, nan, conv)
        want, want_st = numpy_decide(S, Q, chunks_in, K, chunk, spp, *tol, min_chunks, nan, conv)
        assert got.dtype == np.int32 and np.array_equal(got, want)
        assert st == want_st
        if pixels > 1:
            assert (got == 0).any()  # (some pixel stays active: the inputs exercise both sides)
            if nan or K >= max(2, min_chunks):
                assert st["stopped_now"] > 0
    # infinite sums never stop, whatever the tolerance
    if pixels > 1:
        big, _ = rtamd.adapt_decide(S, Q, None, K, chunk, spp, 1e300, 1e300, 2, True, True)
        assert (big[np.isinf(S).any(axis=1) & ~np.isnan(S).any(axis=1)] == 0).all()
        assert (big[np.isfinite(S).all(axis=1)] == K).all()
    # image-shaped input gives an image-shaped map
    if pixels == 1000:
        got2, st2 = rtamd.adapt_decide(S.reshape(25, 40, 3), Q.reshape(25, 40, 3), kin.reshape(25, 40), K, chunk, spp,
                                       *tol, min_chunks, nan, conv)
        assert got2.shape == (25, 40) and np.array_equal(got2.reshape(-1), got) and st2 == st


class StubFrame:
    """A frame whose adapt stats per step are scripted: render_progressive's adaptive loop without a device."""

    def __init__(self, total, active, pixels=16):
        self.total, self.done, self.active, self.pixels = total, 0, list(active), pixels
        self.steps, self.adapt_calls, self.closed = [], [], False

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
        return np.full((4, 4, 3), self.done, np.uint8), None, {"chunks_done": self.done, "bytes_changed": 48}

    def adapt(self, abs_tol=0.0, rel_tol=0.0, min_chunks=2, nan=True, converged=True):
        self.adapt_calls.append((self.done, abs_tol, rel_tol, min_chunks, nan, converged))
        a = self.active[len(self.steps) - 1]
        return {"chunks_done": self.done, "pixels": self.pixels, "active_pixels": a, "stopped_nan": 1,
                "stopped_converged_or_masked": self.pixels - a - 1, "stopped_now": 0}

    def close(self):
        self.closed = True


class TrackedCtx:
    def __init__(self, frame):
        self.frame, self.opened = frame, []

    def open_frame(self, cam, params, moments=False):
        self.opened.append(moments)
        return self.frame


def test_render_progressive_adaptive_over_a_stub():
    p = rtamd.make_params(4, 4, 40, 5)
    # ends at the step that leaves no pixel active, yielding it, with the adapt stats merged in
    fr = StubFrame(20, [12, 5, 0, 0])
    ctx = TrackedCtx(fr)
    out = list(rtamd.render_progressive(ctx, None, p, 2, adaptive=True, abs_tol=0.05, rel_tol=0.01, min_chunks=4))
    assert ctx.opened == [True] and fr.steps == [2, 2, 2] and len(out) == 3 and fr.closed
    assert fr.adapt_calls == [(2, 0.05, 0.01, 4, True, True), (4, 0.05, 0.01, 4, True, True),
                              (6, 0.05, 0.01, 4, True, True)]
    assert [s["active_pixels"] for _, s in out] == [12, 5, 0]
    assert out[1][1]["stopped_converged_or_masked"] == 10 and out[1][1]["bytes_changed"] == 48
    # pixels still active: goes on to completion
    fr = StubFrame(6, [12, 4, 4])
    assert len(list(rtamd.render_progressive(TrackedCtx(fr), None, p, 2, adaptive=True))) == 3 and fr.complete
    # without the keyword no adapt call is made
    fr = StubFrame(4, [0, 0])
    assert len(list(rtamd.render_progressive(TrackedCtx(fr), None, p, 2))) == 2 and fr.adapt_calls == []
    # keyword-only
    with pytest.raises(TypeError):
        list(rtamd.render_progressive(TrackedCtx(StubFrame(4, [0] * 4)), None, p, 2, None, None, 0.0, 0.0, True))


def test_adapt_decide_is_sanitizer_clean(tmp_path):
    """tests/c/adapt_decide_check.c with the host-only unit under ASan + UBSan, as a child process: the null
    arguments it must refuse, the NULL moments and chunks_in it must accept, and every pixel count up to 64
    over heap blocks of exactly that many pixels."""
    csrc = os.path.join(ROOT, "ray-tracing_amd", "csrc")
    exe = str(tmp_path / "adapt_decide_check")
    obj = str(tmp_path / "adapt_decide_check.o")
    # (the sanitizer runtimes linked into the program itself: it needs nothing from its environment)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1",
           "-static-libasan", "-static-libubsan"]
    fp = ["-ffp-contract=off", "-fno-fast-math"]
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + csrc]
    subprocess.run(["gcc", "-std=c11", "-Wall", *san, *fp, *inc, "-c",
                    os.path.join(ROOT, "tests", "c", "adapt_decide_check.c"), "-o", obj], check=True, timeout=300)
    subprocess.run(["gcc", "-std=c++17", "-Wall", *san, *fp, *inc, obj, os.path.join(csrc, "rt_frame_error.cpp"),
                    os.path.join(csrc, "rt_scene.cpp"), "-lstdc++", "-lm", "-o", exe], check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    print(r.stdout[-4000:], r.stderr[-4000:])
    assert r.returncode == 0, r.stderr[-2000:]
    assert "adapt_decide_check: clean (0 failures)" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
