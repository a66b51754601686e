"""Progressive tier-B frames over the C ABI (include/rt.h, rt_frame_*): render a frame a few sample
chunks at a time, look at previews while it converges, stop when the bytes stop moving, or save the
running sums and finish later. A frame advanced to its end resolves to `Context.render`'s output bit
for bit, whatever the steps.

    with ctx.open_frame(cam, params) as fr:
        while not fr.complete:
            fr.advance(8)
            rgb, lin, stats = fr.resolve()

`render_progressive` wraps that loop as a generator with the 8-bit stopping rule.

A frame opened with `moments=True` also keeps the second moments of its chunk sums (rt.h, RT_FRAME_MOMENTS):
`fr.error(abs_tol, rel_tol)` is the per-pixel standard error of the mean and its summary at any point
after two chunks, and `render_progressive(..., stop_unconverged_fraction=...)` stops on it.

Adaptive frames (rt.h): `fr.adapt(...)` stops the pixels whose sum is NaN (nothing is lost: their bytes stay 0)
and those already converged under a tolerance, `fr.stop(mask)` the caller's own choice; later `advance` calls
render the active pixels only. `render_progressive(..., adaptive=True)` calls `adapt` after every step.
"""
from __future__ import annotations

import ctypes as C
from typing import Iterator, Optional, Tuple

import numpy as np

import rtamd as _rt

STATS_FIELDS = ("chunk", "chunks_total", "chunks_done", "samples_done", "kernel_ms", "nan_pixels", "bytes_changed")
BLOB_HEADER = 288  # RT_FRAME_BLOB_HEADER
BLOB_VERSION = 1   # RT_FRAME_BLOB_VERSION
BLOB_MAGIC = b"RTFRAME\0"
PARAM_FIELDS = ("width", "height", "spp", "max_depth", "rng_mode", "flags", "seed", "tile", "shard_rank",
                "shard_count")


ADAPT_FIELDS = ("chunks_done", "pixels", "active_pixels", "stopped_nan", "stopped_converged_or_masked", "stopped_now")
ERROR_FIELDS = ("chunks_done", "samples_done", "pixels", "nonfinite_pixels", "unconverged_pixels", "max_se", "mean_se")


def _stats_dict(s) -> dict:
    return {k: getattr(s, k) for k in STATS_FIELDS}


def _error_dict(s) -> dict:
    return {k: getattr(s, k) for k in ERROR_FIELDS}


def _adapt_dict(s) -> dict:
    return {k: getattr(s, k) for k in ADAPT_FIELDS}


def _adapt_rule(abs_tol, rel_tol, min_chunks, nan, converged):
    flags = (_rt.RT_ADAPT_NAN if nan else 0) | (_rt.RT_ADAPT_CONVERGED if converged else 0)
    return _rt.rt_adapt_rule(abs_tol, rel_tol, int(min_chunks), flags)


def _doubles(a, shape=None) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None and a.shape != shape:
        raise ValueError(f"expected an array of shape {shape}, got {a.shape}")
    return a


class ProgressiveFrame:
    """One open frame of a Context (rt_frame_open / rt_frame_restore). Also a context manager."""

    def __init__(self, ctx, handle, params, tracks_moments: bool = False):
        self._ctx = ctx
        self._h = handle
        self.width, self.height, self.spp = params.width, params.height, params.spp
        self.chunk, self.chunks_total = _rt.frame_chunking(self.width * self.height, self.spp)
        self.chunks_done = 0
        self.tracks_moments = bool(tracks_moments)
        self.active_pixels = self.width * self.height  # (pixels no stop call has stopped)

    @classmethod
    def open(cls, ctx, cam, params, moments: bool = False) -> "ProgressiveFrame":
        h = C.c_void_p()
        if moments:
            _rt._check(_rt.lib().rt_frame_open_ex(ctx._h, C.byref(cam), C.byref(params), _rt.RT_FRAME_MOMENTS,
                                                  C.byref(h)), "rt_frame_open_ex")
        else:
            _rt._check(_rt.lib().rt_frame_open(ctx._h, C.byref(cam), C.byref(params), C.byref(h)), "rt_frame_open")
        return cls(ctx, h, params, moments)

    @property
    def complete(self) -> bool:
        return self.chunks_done >= self.chunks_total

    def advance(self, max_chunks: int = 1) -> int:
        """Queue the next min(max_chunks, remaining) chunks; returns how many (0 on a complete frame)."""
        n = C.c_int(0)
        _rt._check(_rt.lib().rt_frame_advance(self._handle(), int(max_chunks), C.byref(n)), "rt_frame_advance")
        self.chunks_done += n.value
        return n.value

    def resolve(self, rgb: bool = True, linear: bool = True):
        """(rgb8[H,W,3] | None, linear[H,W,3] | None, stats dict) over the samples rendered so far."""
        W, H = self.width, self.height
        out_rgb = np.zeros((H, W, 3), dtype=np.uint8) if rgb else None
        out_lin = np.zeros((H, W, 3), dtype=np.float64) if linear else None
        s = _rt.rt_frame_stats()
        P = C.POINTER
        _rt._check(_rt.lib().rt_frame_resolve(
            self._handle(), out_rgb.ctypes.data_as(P(C.c_uint8)) if rgb else None,
            out_lin.ctypes.data_as(P(C.c_double)) if linear else None, C.byref(s)), "rt_frame_resolve")
        return out_rgb, out_lin, _stats_dict(s)

    def stats(self) -> dict:
        """The stats of `resolve` without the image copies."""
        return self.resolve(rgb=False, linear=False)[2]

    def save(self) -> bytes:
        """The frame as a blob (rt.h layout) for `Context.restore_frame`."""
        n = C.c_size_t(0)
        _rt._check(_rt.lib().rt_frame_save(self._handle(), None, 0, C.byref(n)), "rt_frame_save")
        buf = C.create_string_buffer(n.value)
        _rt._check(_rt.lib().rt_frame_save(self._handle(), buf, n.value, C.byref(n)), "rt_frame_save")
        return buf.raw[:n.value]

    def moments(self) -> np.ndarray:
        """rt_frame_moments: Q[H,W,3], the second moments of the chunk sums (rt.h), for `restore_frame` and
        `error_estimate`. RTError (RT_E_STATE) on a frame that does not track them."""
        q = np.zeros((self.height, self.width, 3), dtype=np.float64)
        _rt._check(_rt.lib().rt_frame_moments(self._handle(), q.ctypes.data_as(C.POINTER(C.c_double))), "rt_frame_moments")
        return q

    def error(self, abs_tol: float = 0.0, rel_tol: float = 0.0, want_map: bool = True):
        """rt_frame_error: (se[H,W,3] | None, stats dict) after at least two chunks: the standard error of
        each pixel's mean, and pixels / nonfinite_pixels / unconverged_pixels (under abs_tol + rel_tol * |mean|)
        / max_se / mean_se."""
        se = np.zeros((self.height, self.width, 3), dtype=np.float64) if want_map else None
        tol = _rt.rt_error_tol(abs_tol, rel_tol)
        s = _rt.rt_error_stats()
        _rt._check(_rt.lib().rt_frame_error(self._handle(), C.byref(tol),
                                            se.ctypes.data_as(C.POINTER(C.c_double)) if want_map else None,
                                            C.byref(s)), "rt_frame_error")
        return se, _error_dict(s)

    def adapt(self, abs_tol: float = 0.0, rel_tol: float = 0.0, min_chunks: int = 2, nan: bool = True,
              converged: bool = True) -> dict:
        """rt_frame_adapt: stops, for good, the active pixels whose running sum has a NaN channel (`nan`) and
        those with chunks_done >= max(2, min_chunks) that `error`'s rule calls converged under (abs_tol,
        rel_tol) (`converged`; needs a frame opened with moments). Returns the stats dict: pixels /
        active_pixels / stopped_nan / stopped_converged_or_masked / stopped_now."""
        rule = _adapt_rule(abs_tol, rel_tol, min_chunks, nan, converged)
        s = _rt.rt_adapt_stats()
        _rt._check(_rt.lib().rt_frame_adapt(self._handle(), C.byref(rule), C.byref(s)), "rt_frame_adapt")
        self.active_pixels = s.active_pixels
        return _adapt_dict(s)

    def stop(self, mask) -> dict:
        """rt_frame_stop: stops the pixels where mask[H,W] is nonzero (the caller's own rule). Stats as `adapt`."""
        m = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
        if m.shape != (self.height, self.width):
            raise ValueError(f"expected a mask of shape {(self.height, self.width)}, got {m.shape}")
        s = _rt.rt_adapt_stats()
        _rt._check(_rt.lib().rt_frame_stop(self._handle(), m.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(s)),
                   "rt_frame_stop")
        self.active_pixels = s.active_pixels
        return _adapt_dict(s)

    def chunk_counts(self) -> np.ndarray:
        """rt_frame_chunk_counts: K_p[H,W] (int32), the chunks each pixel's sums hold: where it was stopped,
        else chunks_done."""
        k = np.zeros((self.height, self.width), dtype=np.int32)
        _rt._check(_rt.lib().rt_frame_chunk_counts(self._handle(), k.ctypes.data_as(C.POINTER(C.c_int32))),
                   "rt_frame_chunk_counts")
        return k

    def close(self):
        # (rt_destroy closes the ctx's open frames itself: after Context.close the handle is dead)
        if self._h is not None and self._ctx._h is not None:
            _rt.lib().rt_frame_close(self._h)
        self._h = None

    def _handle(self):
        if self._h is None or self._ctx._h is None:
            raise _rt.RTError("the frame (or its context) is closed")
        return self._h

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def restore_frame(ctx, blob: bytes, moments: Optional[np.ndarray] = None) -> ProgressiveFrame:
    """rt_frame_restore, or with `moments` (the saved frame's `moments()` at that save; pairing the two is
    the caller's business) rt_frame_restore_ex: a tracked frame."""
    info = blob_info(blob)
    h = C.c_void_p()
    if moments is None:
        _rt._check(_rt.lib().rt_frame_restore(ctx._h, blob, len(blob), C.byref(h)), "rt_frame_restore")
    else:
        q = _doubles(moments, (info["height"], info["width"], 3))
        _rt._check(_rt.lib().rt_frame_restore_ex(ctx._h, blob, len(blob), q.ctypes.data_as(C.POINTER(C.c_double)),
                                                 C.byref(h)), "rt_frame_restore_ex")
    fr = ProgressiveFrame(ctx, h, info["params"], moments is not None)
    fr.chunks_done = info["chunks_done"]
    return fr


def error_estimate(sums, moments, chunks_done: int, samples_done: int, abs_tol: float = 0.0, rel_tol: float = 0.0):
    """rt_error_estimate (host only): (se, stats dict) from image-order sums (a blob's payload) and moments
    of the same shape [..., 3], by the per-pixel function `ProgressiveFrame.error` runs on the device."""
    s = _doubles(sums)
    q = _doubles(moments, s.shape)
    if s.ndim < 1 or s.shape[-1] != 3:
        raise ValueError("sums and moments must have 3 channels in their last axis")
    se = np.zeros_like(s)
    tol = _rt.rt_error_tol(abs_tol, rel_tol)
    st = _rt.rt_error_stats()
    P = C.POINTER(C.c_double)
    _rt._check(_rt.lib().rt_error_estimate(s.ctypes.data_as(P), q.ctypes.data_as(P), s.size // 3, int(chunks_done),
                                           int(samples_done), C.byref(tol), se.ctypes.data_as(P), C.byref(st)),
               "rt_error_estimate")
    return se, _error_dict(st)


def adapt_decide(sums, moments, chunks_in, chunks_done: int, chunk: int, spp: int, abs_tol: float = 0.0,
                 rel_tol: float = 0.0, min_chunks: int = 2, nan: bool = True, converged: bool = True):
    """rt_adapt_decide (host only): (chunks_out, stats dict) by the rule `ProgressiveFrame.adapt` runs on the
    device, from image-order sums [..., 3] at `chunks_done` chunks. `moments` may be None without
    `converged`; `chunks_in` (the K_p map so far, 0 = active) may be None."""
    s = _doubles(sums)
    if s.ndim < 1 or s.shape[-1] != 3:
        raise ValueError("sums must have 3 channels in their last axis")
    q = None if moments is None else _doubles(moments, s.shape)
    kin = None if chunks_in is None else np.ascontiguousarray(chunks_in, dtype=np.int32)
    if kin is not None and kin.shape != s.shape[:-1]:
        raise ValueError(f"expected chunks_in of shape {s.shape[:-1]}, got {kin.shape}")
    out = np.zeros(s.shape[:-1], dtype=np.int32)
    rule = _adapt_rule(abs_tol, rel_tol, min_chunks, nan, converged)
    st = _rt.rt_adapt_stats()
    PD, PI = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    _rt._check(_rt.lib().rt_adapt_decide(s.ctypes.data_as(PD), None if q is None else q.ctypes.data_as(PD),
                                         None if kin is None else kin.ctypes.data_as(PI), s.size // 3,
                                         int(chunks_done), int(chunk), int(spp), C.byref(rule), out.ctypes.data_as(PI),
                                         C.byref(st)), "rt_adapt_decide")
    return out, _adapt_dict(st)


def blob_info(blob: bytes) -> dict:
    """rt_frame_blob_info: a saved frame's header, validated on the host (no device). Raises RTError
    (RT_E_INVALID) for a malformed blob."""
    d = _rt.rt_frame_blob_desc()
    _rt._check(_rt.lib().rt_frame_blob_info(blob, len(blob), C.byref(d)), "rt_frame_blob_info")
    p = _rt.rt_render_params()
    C.memmove(C.byref(p), C.byref(d.params), C.sizeof(p))
    cam = _rt.rt_camera()
    C.memmove(C.byref(cam), C.byref(d.camera), C.sizeof(cam))
    out = {k: getattr(d, k) for k in ("version", "upload_flags", "chunk", "chunks_total", "chunks_done", "samples_done",
                                      "pixels", "scene_fingerprint", "payload_bytes")}
    out.update({k: getattr(p, k) for k in PARAM_FIELDS})
    out["params"], out["camera"] = p, cam
    return out


def render_progressive(ctx, cam, params, step_chunks: int,
                       stop_changed_fraction: Optional[float] = None, *,
                       stop_unconverged_fraction: Optional[float] = None, abs_tol: float = 0.0,
                       rel_tol: float = 0.0, adaptive: bool = False,
                       min_chunks: int = 2) -> Iterator[Tuple[np.ndarray, dict]]:
    """Yields (rgb, stats) after each step of `step_chunks` chunks. Stops at completion, or once
    bytes_changed / (3*W*H) of a step is at most `stop_changed_fraction` (the 8-bit stopping rule: the
    bytes stopped moving). `ctx` needs `open_frame(cam, params)` returning a frame with `advance`,
    `resolve(linear=False)`, `complete` and `close`.

    With `stop_unconverged_fraction` the frame is opened with `moments=True`, every step that leaves
    chunks_done >= 2 merges `frame.error(abs_tol, rel_tol, want_map=False)`'s stats into the yielded
    dict, and the loop also stops once unconverged_pixels <= fraction * (pixels - nonfinite_pixels): the
    standard error of all but that share of the finite pixels is within abs_tol + rel_tol * |mean|.
    Either rule stops the loop.

    With `adaptive` the frame is opened with `moments=True` and after each step's resolve
    `frame.adapt(abs_tol, rel_tol, min_chunks)` stops the NaN pixels and the pixels converged under the
    tolerances (its stats are merged into the yielded dict; the yielded image is the one before that call,
    which a stop does not change); the loop also ends once no pixel is active."""
    if step_chunks < 1:
        raise ValueError("step_chunks must be at least 1")
    channels = 3 * params.width * params.height
    by_error = stop_unconverged_fraction is not None
    tracked = by_error or adaptive
    frame = ctx.open_frame(cam, params, moments=True) if tracked else ctx.open_frame(cam, params)
    try:
        while not frame.complete:
            frame.advance(step_chunks)
            rgb, _, stats = frame.resolve(linear=False)
            met = False
            if by_error and stats["chunks_done"] >= 2:
                err = frame.error(abs_tol, rel_tol, want_map=False)[1]
                stats.update(err)
                met = err["unconverged_pixels"] <= stop_unconverged_fraction * (err["pixels"] - err["nonfinite_pixels"])
            if adaptive:
                ad = frame.adapt(abs_tol, rel_tol, min_chunks)
                stats.update(ad)
                met = met or ad["active_pixels"] == 0
            yield rgb, stats
            if met or (stop_changed_fraction is not None and stats["bytes_changed"] <= stop_changed_fraction * channels):
                break
    finally:
        frame.close()
