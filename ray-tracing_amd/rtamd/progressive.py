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

Shard frames (rt.h): `ctx.open_shard_frame(cam, params)` is the same frame over the slab of one tile shard
(params.tile, shard_rank, shard_count), its previews, error map and state left in slab order in device memory
(`ShardFrame`); `ShardedProgressiveFrame` drives `world` of them, in one process or as one rank of a
torch.distributed group, and gives the unsharded frame's results bit for bit.

Checkpoints (rt.h, the version-2 blob): `fr.checkpoint()` is one blob with the sums, a tracked frame's moments
and an adapted frame's K_p; `ctx.resume_frame(blob)` / `ctx.resume_shard_frame(blob, rank, count)` continue it
bit for bit, on any shard count; `checkpoint_info`, `checkpoint_resolve` and `checkpoint_error` parse, preview
and estimate a checkpoint on the host alone; `render_progressive(..., resume=blob, checkpoint=callable)`.
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
CKPT_HEADER = 320  # RT_FRAME_CKPT_HEADER
CKPT_VERSION = 2   # RT_FRAME_CKPT_VERSION
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

    def save_header(self) -> bytes:
        """rt_frame_save_header: the 288-byte header of the whole image's version-1 blob (`save()`'s first 288 bytes;
        on a shard frame the whole image's, the same on every shard)."""
        buf = C.create_string_buffer(BLOB_HEADER)
        _rt._check(_rt.lib().rt_frame_save_header(self._handle(), buf, BLOB_HEADER), "rt_frame_save_header")
        return buf.raw

    def checkpoint(self) -> bytes:
        """rt_frame_checkpoint: the frame as a version-2 blob (rt.h) with its moments when it tracks them and its
        K_p when a pixel is stopped, for `Context.resume_frame`, `Context.resume_shard_frame` and the host-only
        `checkpoint_info` / `checkpoint_resolve` / `checkpoint_error`."""
        n = C.c_size_t(0)
        _rt._check(_rt.lib().rt_frame_checkpoint(self._handle(), None, 0, C.byref(n)), "rt_frame_checkpoint")
        buf = C.create_string_buffer(n.value)
        _rt._check(_rt.lib().rt_frame_checkpoint(self._handle(), buf, n.value, C.byref(n)), "rt_frame_checkpoint")
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

    def denoise(self, feature_sums, feature_samples: int, rgb: bool = True, linear: bool = True, **params):
        """rt_frame_denoise: (rgb8[H,W,3] | None, linear[H,W,3] | None, stats dict) of the frame's current preview
        through the feature-guided denoiser (rt.h), on the device: the preview is `resolve`'s, its error map
        `error`'s when the frame tracks moments and has two chunks (else none), and only the result is copied
        back. `feature_sums`: a feature pass's sums of `feature_samples` samples, [H, W, 8], as a torch tensor on
        the frame's device (e.g. what `Context.render_features_async` filled), a device address, or a numpy array
        (copied to the device through torch). `params`: `rtamd.make_denoise_params`' keywords (iterations, flags,
        sigma_color, color_floor, sigma_normal, sigma_depth). The frame itself is left as it is: its next
        `resolve` reports the bytes_changed it would have reported. RTError (RT_E_STATE) on a shard frame."""
        p = _rt.make_denoise_params(self.width, self.height, int(feature_samples), **params)
        if isinstance(feature_sums, np.ndarray):
            import torch
            feature_sums = torch.from_numpy(_doubles(feature_sums, (self.height, self.width, _rt.RT_FEATURE_DOUBLES))
                                            ).to(f"cuda:{self._ctx.device}")
        out_rgb = np.zeros((self.height, self.width, 3), dtype=np.uint8) if rgb else None
        out_lin = np.zeros((self.height, self.width, 3), dtype=np.float64) if linear else None
        s = _rt.rt_denoise_stats()
        P = C.POINTER
        _rt._check(_rt.lib().rt_frame_denoise(
            self._handle(), C.byref(p), _dev_ptr(feature_sums), out_rgb.ctypes.data_as(P(C.c_uint8)) if rgb else None,
            out_lin.ctypes.data_as(P(C.c_double)) if linear else None, C.byref(s)), "rt_frame_denoise")
        return out_rgb, out_lin, _rt._denoise_stats_dict(s)

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


def resume_frame(ctx, blob: bytes) -> ProgressiveFrame:
    """rt_frame_resume: the frame a version-1 or version-2 blob holds (see Context.resume_frame)."""
    info = checkpoint_info(blob)
    h = C.c_void_p()
    _rt._check(_rt.lib().rt_frame_resume(ctx._h, blob, len(blob), C.byref(h)), "rt_frame_resume")
    fr = ProgressiveFrame(ctx, h, info["params"], info["Q"] is not None)
    fr.chunks_done, fr.active_pixels = info["chunks_done"], info["active_pixels"]
    return fr


def checkpoint_info(blob: bytes) -> dict:
    """rt_frame_checkpoint_info (host only): `blob_info`'s dict of a version-1 or version-2 blob, plus `sections`,
    the byte offsets `sums_offset` / `moments_offset` / `stops_offset`, the counts `stopped_pixels` /
    `stopped_nan` / `active_pixels`, and read-only numpy views of the payload: `S` [H,W,3] float64, `Q` [H,W,3]
    float64 or None, `K` [H,W] int32 (0 = active) or None. Raises RTError (RT_E_INVALID) for a malformed blob."""
    d = _rt.rt_frame_ckpt_desc()
    _rt._check(_rt.lib().rt_frame_checkpoint_info(blob, len(blob), C.byref(d)), "rt_frame_checkpoint_info")
    b = d.blob
    p = _rt.rt_render_params()
    C.memmove(C.byref(p), C.byref(b.params), C.sizeof(p))
    cam = _rt.rt_camera()
    C.memmove(C.byref(cam), C.byref(b.camera), C.sizeof(cam))
    out = {k: getattr(b, k) for k in ("version", "upload_flags", "chunk", "chunks_total", "chunks_done", "samples_done",
                                      "pixels", "scene_fingerprint", "payload_bytes")}
    out.update({k: getattr(p, k) for k in PARAM_FIELDS})
    out.update({k: getattr(d, k) for k in ("sections", "sums_offset", "moments_offset", "stops_offset",
                                           "stopped_pixels", "stopped_nan", "active_pixels")})
    out["params"], out["camera"] = p, cam
    H, W = p.height, p.width
    out["S"] = np.frombuffer(blob, dtype="<f8", count=3 * W * H, offset=d.sums_offset).reshape(H, W, 3)
    out["Q"] = (np.frombuffer(blob, dtype="<f8", count=3 * W * H, offset=d.moments_offset).reshape(H, W, 3)
                if d.moments_offset else None)
    out["K"] = np.frombuffer(blob, dtype="<i4", count=W * H, offset=d.stops_offset).reshape(H, W) if d.stops_offset else None
    return out


def checkpoint_resolve(blob: bytes, rgb: bool = True, linear: bool = True):
    """rt_checkpoint_resolve (host only, no scene needed): (rgb8[H,W,3] | None, linear[H,W,3] | None, stats dict),
    the preview `resolve` gives of a resumed frame; bytes_changed is taken against an all-zero image."""
    info = checkpoint_info(blob)
    H, W = info["height"], info["width"]
    out_rgb = np.zeros((H, W, 3), dtype=np.uint8) if rgb else None
    out_lin = np.zeros((H, W, 3), dtype=np.float64) if linear else None
    s = _rt.rt_frame_stats()
    P = C.POINTER
    _rt._check(_rt.lib().rt_checkpoint_resolve(blob, len(blob), out_rgb.ctypes.data_as(P(C.c_uint8)) if rgb else None,
                                               out_lin.ctypes.data_as(P(C.c_double)) if linear else None, C.byref(s)),
               "rt_checkpoint_resolve")
    return out_rgb, out_lin, _stats_dict(s)


def checkpoint_error(blob: bytes, abs_tol: float = 0.0, rel_tol: float = 0.0, want_map: bool = True):
    """rt_checkpoint_error (host only): (se[H,W,3] | None, stats dict), `ProgressiveFrame.error` of a checkpoint
    with moments and at least two chunks, each stopped pixel at its own (K_p, N_p)."""
    info = checkpoint_info(blob)
    se = np.zeros((info["height"], info["width"], 3), dtype=np.float64) if want_map else None
    tol = _rt.rt_error_tol(abs_tol, rel_tol)
    s = _rt.rt_error_stats()
    _rt._check(_rt.lib().rt_checkpoint_error(blob, len(blob), C.byref(tol),
                                             se.ctypes.data_as(C.POINTER(C.c_double)) if want_map else None,
                                             C.byref(s)), "rt_checkpoint_error")
    return se, _error_dict(s)


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
                       min_chunks: int = 2, resume: Optional[bytes] = None,
                       checkpoint=None) -> Iterator[Tuple[np.ndarray, dict]]:
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
    which a stop does not change); the loop also ends once no pixel is active.

    With `resume` (a blob of `ProgressiveFrame.checkpoint`, or a version-1 blob) the loop starts from
    `ctx.resume_frame(resume)` instead of opening a frame: `cam` and `params` are then the blob's and the
    arguments are not looked at. With `checkpoint` (a callable) every step hands it `frame.checkpoint()` after
    the step's stop call (after the resolve when the run is not adaptive) and before the step is yielded, so a
    run interrupted at any step continues from the last blob to the same image and stats."""
    if step_chunks < 1:
        raise ValueError("step_chunks must be at least 1")
    by_error = stop_unconverged_fraction is not None
    tracked = by_error or adaptive
    if resume is not None:
        frame = ctx.resume_frame(resume)
    else:
        frame = ctx.open_frame(cam, params, moments=True) if tracked else ctx.open_frame(cam, params)
    channels = 3 * params.width * params.height if resume is None else 3 * frame.width * frame.height
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
            if checkpoint is not None:
                checkpoint(frame.checkpoint())
            yield rgb, stats
            if met or (stop_changed_fraction is not None and stats["bytes_changed"] <= stop_changed_fraction * channels):
                break
    finally:
        frame.close()


# ----------------------------------------------------------------------------- shard frames (rt.h)
def error_stats_merge(parts) -> dict:
    """rt_error_stats_merge (host only): the error stats of N shard frames (dicts with ERROR_FIELDS, or
    rt_error_stats) as one: counts added, max_se the maximum, mean_se weighted by finite pixels."""
    parts = list(parts)
    arr = (_rt.rt_error_stats * max(1, len(parts)))()
    for i, p in enumerate(parts):
        for k in ERROR_FIELDS:
            setattr(arr[i], k, p[k] if isinstance(p, dict) else getattr(p, k))
    out = _rt.rt_error_stats()
    _rt._check(_rt.lib().rt_error_stats_merge(arr, len(parts), C.byref(out)), "rt_error_stats_merge")
    return _error_dict(out)


def _dev_ptr(x):
    """A device pointer argument: None, an integer address, or a torch tensor (contiguous, on the frame's device)."""
    if x is None:
        return None
    if hasattr(x, "data_ptr"):
        if not x.is_contiguous():
            raise ValueError("device buffers must be contiguous")
        return C.c_void_p(x.data_ptr())
    return C.c_void_p(int(x))


def shard_params(params, rank: int, count: int):
    """A copy of `params` for shard `rank` of `count`."""
    p = _rt.rt_render_params()
    C.memmove(C.byref(p), C.byref(params), C.sizeof(p))
    p.shard_rank, p.shard_count = int(rank), int(count)
    return p


class ShardFrame(ProgressiveFrame):
    """One shard frame of a Context (rt_frame_open_shard / rt_frame_restore_shard): `advance`, `adapt`, `stop`
    and `close` as ProgressiveFrame; previews, error map and state are slabs of `slab_pixels` pixels in the
    layout of rt_render_shard_async, written into device memory (`*_into`: device pointers or torch tensors
    on the ctx's device) or, by the host conveniences `resolve`, `error` and `state`, returned as numpy slabs.
    The image-order calls (`save`, `moments`, `chunk_counts`) raise RTError (RT_E_STATE) on it."""

    def __init__(self, ctx, handle, params, tracks_moments: bool = False):
        super().__init__(ctx, handle, params, tracks_moments)
        self.params = shard_params(params, params.shard_rank, max(1, params.shard_count))
        self.rank, self.count = self.params.shard_rank, self.params.shard_count
        self.slab_pixels = _rt.shard_geometry(self.params)[2]
        self.owned_pixels = int((_rt.shard_pixel_map(self.params) >= 0).sum())
        self.active_pixels = self.owned_pixels

    @classmethod
    def open(cls, ctx, cam, params, moments: bool = False) -> "ShardFrame":
        h = C.c_void_p()
        _rt._check(_rt.lib().rt_frame_open_shard(ctx._h, C.byref(cam), C.byref(params),
                                                 _rt.RT_FRAME_MOMENTS if moments else 0, C.byref(h)),
                   "rt_frame_open_shard")
        return cls(ctx, h, params, moments)

    # ---- device outputs
    def resolve_into(self, rgb=None, linear=None) -> dict:
        """rt_frame_resolve_shard: the preview into device slabs (uint8 [slab, 3] / float64 [slab, 3]; None:
        skipped); returns the stats dict, whose counts are over this shard's pixels."""
        s = _rt.rt_frame_stats()
        _rt._check(_rt.lib().rt_frame_resolve_shard(self._handle(), _dev_ptr(rgb), _dev_ptr(linear), C.byref(s)),
                   "rt_frame_resolve_shard")
        return _stats_dict(s)

    def error_into(self, se=None, abs_tol: float = 0.0, rel_tol: float = 0.0) -> dict:
        """rt_frame_error_shard: the error map into a device slab (float64 [slab, 3]; None: skipped); returns
        the stats dict over this shard's pixels (merge them with `error_stats_merge`)."""
        tol = _rt.rt_error_tol(abs_tol, rel_tol)
        s = _rt.rt_error_stats()
        _rt._check(_rt.lib().rt_frame_error_shard(self._handle(), C.byref(tol), _dev_ptr(se), C.byref(s)),
                   "rt_frame_error_shard")
        return _error_dict(s)

    def state_into(self, sums=None, moments=None, chunks=None) -> None:
        """rt_frame_shard_state: device copies of S, Q (float64 [slab, 3]) and K_p (int32 [slab]), slab order."""
        _rt._check(_rt.lib().rt_frame_shard_state(self._handle(), _dev_ptr(sums), _dev_ptr(moments), _dev_ptr(chunks)),
                   "rt_frame_shard_state")

    def stops_into(self, stops) -> None:
        """rt_frame_shard_stops: the raw K_p (int32 [slab], 0 = active) in slab order into device memory."""
        _rt._check(_rt.lib().rt_frame_shard_stops(self._handle(), _dev_ptr(stops)), "rt_frame_shard_stops")

    def checkpoint_header(self, sections: int, chunks_done: int = -1) -> bytes:
        """rt_frame_checkpoint_header: the 320 header bytes of the whole image's checkpoint; `sections` is the OR
        over the image's shards, `chunks_done` the image's (-1: this frame's own)."""
        buf = C.create_string_buffer(CKPT_HEADER)
        _rt._check(_rt.lib().rt_frame_checkpoint_header(self._handle(), int(sections), int(chunks_done), buf,
                                                        CKPT_HEADER), "rt_frame_checkpoint_header")
        return buf.raw

    # ---- host conveniences (numpy slabs, staged through torch tensors on the ctx's device)
    def slab_tensor(self, dtype, channels: int = 3):
        """A zeroed torch tensor of one slab on the ctx's device: [slab_pixels, channels] (channels 0: [slab_pixels])."""
        import torch
        shape = (self.slab_pixels, channels) if channels else (self.slab_pixels,)
        t = torch.zeros(shape, dtype=dtype, device=f"cuda:{self._ctx.device}")
        torch.cuda.current_stream(t.device).synchronize()  # (the ctx writes it on its own, non-blocking stream)
        return t

    def resolve(self, rgb: bool = True, linear: bool = True):
        """(rgb8[slab,3] | None, linear[slab,3] | None, stats dict): `ProgressiveFrame.resolve` in slab order."""
        import torch
        t_rgb = self.slab_tensor(torch.uint8) if rgb else None
        t_lin = self.slab_tensor(torch.float64) if linear else None
        st = self.resolve_into(t_rgb, t_lin)
        return (t_rgb.cpu().numpy() if rgb else None, t_lin.cpu().numpy() if linear else None, st)

    def error(self, abs_tol: float = 0.0, rel_tol: float = 0.0, want_map: bool = True):
        """(se[slab,3] | None, stats dict): `ProgressiveFrame.error` in slab order over this shard's pixels."""
        import torch
        t = self.slab_tensor(torch.float64) if want_map else None
        st = self.error_into(t, abs_tol, rel_tol)
        return (t.cpu().numpy() if want_map else None), st

    def state(self, moments: Optional[bool] = None):
        """(S[slab,3], Q[slab,3] | None, K_p[slab]) as numpy slabs; `moments` defaults to whether the frame tracks them."""
        import torch
        want_q = self.tracks_moments if moments is None else moments
        s, k = self.slab_tensor(torch.float64), self.slab_tensor(torch.int32, 0)
        q = self.slab_tensor(torch.float64) if want_q else None
        self.state_into(s, q, k)
        return s.cpu().numpy(), (q.cpu().numpy() if want_q else None), k.cpu().numpy()

    def stops(self) -> np.ndarray:
        """The raw K_p[slab] (int32, 0 = active) as a numpy slab."""
        import torch
        k = self.slab_tensor(torch.int32, 0)
        self.stops_into(k)
        return k.cpu().numpy()


def restore_shard_frame(ctx, blob: bytes, rank: int, count: int, moments: Optional[np.ndarray] = None) -> ShardFrame:
    """rt_frame_restore_shard: shard `rank` of `count` of a whole-image blob's frame (see Context.restore_shard_frame)."""
    info = blob_info(blob)
    h = C.c_void_p()
    q = None if moments is None else _doubles(moments, (info["height"], info["width"], 3))
    _rt._check(_rt.lib().rt_frame_restore_shard(ctx._h, blob, len(blob),
                                                None if q is None else q.ctypes.data_as(C.POINTER(C.c_double)),
                                                int(rank), int(count), C.byref(h)), "rt_frame_restore_shard")
    fr = ShardFrame(ctx, h, shard_params(info["params"], rank, count), moments is not None)
    fr.chunks_done = info["chunks_done"]
    return fr


def resume_shard_frame(ctx, blob: bytes, rank: int, count: int) -> ShardFrame:
    """rt_frame_resume_shard: shard `rank` of `count` of a whole-image checkpoint's frame (see
    Context.resume_shard_frame)."""
    info = checkpoint_info(blob)
    h = C.c_void_p()
    _rt._check(_rt.lib().rt_frame_resume_shard(ctx._h, blob, len(blob), int(rank), int(count), C.byref(h)),
               "rt_frame_resume_shard")
    fr = ShardFrame(ctx, h, shard_params(info["params"], rank, count), info["Q"] is not None)
    fr.chunks_done = info["chunks_done"]
    if info["K"] is not None:
        m = _rt.shard_pixel_map(fr.params)
        fr.active_pixels = fr.owned_pixels - int((info["K"].reshape(-1)[m[m >= 0]] != 0).sum())
    return fr


class ShardedProgressiveFrame:
    """One progressive frame over `world` shard frames, with ProgressiveFrame's surface: `advance`, `resolve`
    (image, linear, merged stats), `error`, `adapt`, `stop`, `chunk_counts`, `save` (blob, moments), the
    `restore(..., world=M)` classmethod, `checkpoint` (the version-2 blob, adapted frames too) with the
    `resume(..., world=M)` classmethod, and `close`. The result is the unsharded frame's, bit for bit.

    Local mode: `ctxs` is a list of Contexts, one per shard, in this process (the same Context may repeat; each
    needs the scene uploaded). The shards' slabs are copied to the first context's device and assembled there by
    rt_assemble[_linear]_async; K_p is merged on the host through `shard_pixel_map`.

    Distributed mode: `ctxs` is one Context and (`rank`, `world`) this process's place in the default
    torch.distributed group, after ShardedFrame's pattern: with the nccl backend the slabs go through
    all_gather_into_tensor, with gloo they are staged through the host; counts go through all_reduce; rank 0
    assembles, and the image-returning calls give None arrays on the other ranks. `gather` forces the
    collective at world 1.

    Every rank (every shard) must make the same calls in the same order."""

    def __init__(self, ctxs, cam, params, moments: bool = False, *, rank: Optional[int] = None,
                 world: Optional[int] = None, backend: str = "nccl", gather: Optional[bool] = None, _frames=None):
        self.local = isinstance(ctxs, (list, tuple))
        if self.local:
            self.ctxs, self.world, self.rank = list(ctxs), len(ctxs), 0
            ranks = list(range(self.world))
        else:
            if rank is None or world is None:
                raise ValueError("distributed mode needs rank and world")
            self.ctxs, self.world, self.rank = [ctxs], int(world), int(rank)
            ranks = [self.rank]
        if self.world < 1:
            raise ValueError("at least one shard")
        self.backend = backend
        self.gather = (not self.local and self.world > 1) if gather is None else bool(gather)
        if not self.local and self.world > 1 and not self.gather:
            raise ValueError("a distributed frame of more than one shard needs the gather (rank 0 assembles every slab)")
        self.p = shard_params(params, 0, self.world)
        self.width, self.height, self.spp = params.width, params.height, params.spp
        self.chunk, self.chunks_total = _rt.frame_chunking(self.width * self.height, self.spp)
        self.tracks_moments = bool(moments)
        self.frames = _frames if _frames is not None else [
            c.open_shard_frame(cam, shard_params(params, r, self.world), moments=moments)
            for c, r in zip(self.ctxs, ranks)]
        self.chunks_done = max(f.chunks_done for f in self.frames)
        self.slab_pixels = self.frames[0].slab_pixels
        self.root = self.ctxs[0]  # (assembles: local mode's first context, or rank 0's)
        self.active_pixels = self.width * self.height
        self.cam = cam
        self._feature_slabs = None  # (render_features: one [slab, 8] float64 tensor per local shard, kept for `into`)
        self._feature_kept = None   # (... and (their chain, the end of their sample range))

    @classmethod
    def restore(cls, ctxs, blob: bytes, moments: Optional[np.ndarray] = None, *, world: Optional[int] = None,
                rank: Optional[int] = None, backend: str = "nccl", gather: Optional[bool] = None):
        """The frame a whole-image blob (`save`'s, or ProgressiveFrame.save's) holds, over `world` shards: the
        shard count of the saved frame does not matter. Local mode: world defaults to len(ctxs)."""
        info = blob_info(blob)
        local = isinstance(ctxs, (list, tuple))
        m = len(ctxs) if local and world is None else world
        if m is None or (local and m != len(ctxs)):
            raise ValueError("world must be given (local mode: one context per shard)")
        pairs = list(zip(ctxs, range(m))) if local else [(ctxs, rank)]
        frames = [restore_shard_frame(c, blob, r, m, moments) for c, r in pairs]
        return cls(ctxs, info["camera"], info["params"], moments is not None, rank=rank, world=m, backend=backend,
                   gather=gather, _frames=frames)

    @property
    def complete(self) -> bool:
        return self.chunks_done >= self.chunks_total

    # ---- plumbing
    def _torch(self):
        import torch
        return torch

    def _root_device(self):
        return f"cuda:{self.root.device}"

    def _all_slabs(self, slabs):
        """The shards' slabs (this process's, one torch tensor per local frame) as one [world, slab, ...] tensor
        on the root device; None on a distributed rank other than 0 when nothing is gathered."""
        torch = self._torch()
        if self.local:
            out = torch.zeros((self.world,) + tuple(slabs[0].shape), dtype=slabs[0].dtype, device=self._root_device())
            for r, t in enumerate(slabs):
                out[r].copy_(t)  # (device to device, across devices when the contexts differ)
            return out
        slab = slabs[0]
        if not self.gather:
            return slab.unsqueeze(0)
        import torch.distributed as dist
        if self.backend == "nccl":
            out = torch.zeros((self.world,) + tuple(slab.shape), dtype=slab.dtype, device=slab.device)
            dist.all_gather_into_tensor(out, slab)
            return out
        host = slab.cpu()
        parts = [torch.empty_like(host) for _ in range(self.world)]
        dist.all_gather(parts, host)
        return torch.stack(parts).to(slab.device)

    def _assemble_device(self, slabs):
        """[world, slab, 3] uint8 or float64 slabs -> a [H, W, 3] tensor on the root device (None off the root)."""
        torch = self._torch()
        if self.rank != 0:
            return None
        slabs = slabs.contiguous()
        img = torch.zeros((self.height, self.width, 3), dtype=slabs.dtype, device=slabs.device)
        if slabs.dtype == torch.uint8:
            self.root.assemble_async(self.p, slabs.data_ptr(), img.data_ptr())
        else:
            self.root.assemble_linear_async(self.p, slabs.data_ptr(), img.data_ptr())
        torch.cuda.synchronize(slabs.device)
        return img

    def _assemble(self, slabs):
        """[world, slab, 3] uint8 or float64 slabs -> numpy [H, W, 3] on the root (None elsewhere)."""
        img = self._assemble_device(slabs)
        return None if img is None else img.cpu().numpy()

    def _sum_counts(self, dicts, keys) -> dict:
        """The shards' exact counts added (rt.h: frame and adapt stats merge by plain addition)."""
        tot = [int(sum(d[k] for d in dicts)) for k in keys]
        if not self.local and self.world > 1:
            import torch.distributed as dist
            torch = self._torch()
            t = torch.tensor(tot, dtype=torch.int64, device=self._root_device() if self.backend == "nccl" else "cpu")
            dist.all_reduce(t)
            tot = [int(x) for x in t.cpu()]
        return dict(zip(keys, tot))

    def _slabs_of(self, make, fill):
        ts = []
        for f in self.frames:
            t = make(f)
            fill(f, t)
            ts.append(t)
        return ts

    # ---- ProgressiveFrame's surface
    def advance(self, max_chunks: int = 1) -> int:
        n = max(f.advance(max_chunks) for f in self.frames)
        if not self.local and self.world > 1:
            n = self._max_int(n)
        self.chunks_done += n
        return n

    def _max_int(self, n: int) -> int:
        import torch.distributed as dist
        torch = self._torch()
        t = torch.tensor([n], dtype=torch.int64, device=self._root_device() if self.backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return int(t.cpu()[0])

    def resolve(self, rgb: bool = True, linear: bool = True):
        """(rgb8[H,W,3] | None, linear[H,W,3] | None, stats dict): the shards' previews assembled; nan_pixels and
        bytes_changed added over the shards, kernel_ms the slowest local shard's."""
        torch = self._torch()
        stats, rgbs, lins = [], [], []
        for f in self.frames:
            t_rgb = f.slab_tensor(torch.uint8) if rgb else None
            t_lin = f.slab_tensor(torch.float64) if linear else None
            stats.append(f.resolve_into(t_rgb, t_lin))
            rgbs.append(t_rgb)
            lins.append(t_lin)
        out = dict(stats[0])
        out["chunks_done"] = max(s["chunks_done"] for s in stats)
        out["samples_done"] = max(s["samples_done"] for s in stats)
        out["kernel_ms"] = max(s["kernel_ms"] for s in stats)
        out.update(self._sum_counts(stats, ("nan_pixels", "bytes_changed")))
        img = self._assemble(self._all_slabs(rgbs)) if rgb else None
        lin = self._assemble(self._all_slabs(lins)) if linear else None
        return img, lin, out

    def stats(self) -> dict:
        return self.resolve(rgb=False, linear=False)[2]

    def error(self, abs_tol: float = 0.0, rel_tol: float = 0.0, want_map: bool = True):
        """(se[H,W,3] | None, stats dict): the shards' error maps assembled, their stats merged by
        rt_error_stats_merge (a shard whose pixels are all stopped may lag in chunks_done: its stats are
        per pixel at (K_p, N_p) anyway and are merged at the frame's)."""
        torch = self._torch()
        parts, maps = [], []
        for f in self.frames:
            t = f.slab_tensor(torch.float64) if want_map else None
            parts.append(f.error_into(t, abs_tol, rel_tol))
            maps.append(t)
        if not self.local and self.world > 1:
            import torch.distributed as dist
            row = torch.tensor([float(parts[0][k]) for k in ERROR_FIELDS], dtype=torch.float64,
                               device=self._root_device() if self.backend == "nccl" else "cpu")
            rows = [torch.empty_like(row) for _ in range(self.world)]
            dist.all_gather(rows, row)
            parts = [{k: (float(v) if k in ("max_se", "mean_se") else int(v)) for k, v in zip(ERROR_FIELDS, r.cpu().tolist())}
                     for r in rows]
        k_done = max(p["chunks_done"] for p in parts)
        n_done = max(p["samples_done"] for p in parts)
        parts = [dict(p, chunks_done=k_done, samples_done=n_done) for p in parts]
        se = self._assemble(self._all_slabs(maps)) if want_map else None
        return se, error_stats_merge(parts)

    def _adapt_merge(self, stats) -> dict:
        out = self._sum_counts(stats, ("pixels", "active_pixels", "stopped_nan", "stopped_converged_or_masked",
                                       "stopped_now"))
        out["chunks_done"] = max(s["chunks_done"] for s in stats)
        self.active_pixels = out["active_pixels"]
        return out

    def adapt(self, abs_tol: float = 0.0, rel_tol: float = 0.0, min_chunks: int = 2, nan: bool = True,
              converged: bool = True) -> dict:
        return self._adapt_merge([f.adapt(abs_tol, rel_tol, min_chunks, nan, converged) for f in self.frames])

    def stop(self, mask) -> dict:
        """The same image-order mask[H,W] to every shard (each reads its own pixels)."""
        return self._adapt_merge([f.stop(mask) for f in self.frames])

    def _merge_host(self, slabs: np.ndarray) -> np.ndarray:
        """[world, slab] slabs -> [H, W] through shard_pixel_map (the host's statement of the slab layout)."""
        out = np.zeros(self.height * self.width, dtype=slabs.dtype)
        for r in range(self.world):
            m = _rt.shard_pixel_map(shard_params(self.p, r, self.world))
            ok = m >= 0
            out[m[ok]] = slabs[r][ok]
        return out.reshape(self.height, self.width)

    def chunk_counts(self) -> Optional[np.ndarray]:
        """K_p[H,W] (int32): the shards' slab-order counts merged on the host (None off the root)."""
        torch = self._torch()
        ks = self._slabs_of(lambda f: f.slab_tensor(torch.int32, 0), lambda f, t: f.state_into(None, None, t))
        allk = self._all_slabs(ks)
        return self._merge_host(allk.cpu().numpy()) if self.rank == 0 else None

    def _state_image(self, which: str) -> Optional[np.ndarray]:
        torch = self._torch()
        fill = (lambda f, t: f.state_into(t, None, None)) if which == "sums" else (lambda f, t: f.state_into(None, t, None))
        return self._assemble(self._all_slabs(self._slabs_of(lambda f: f.slab_tensor(torch.float64), fill)))

    def moments(self) -> Optional[np.ndarray]:
        """Q[H,W,3] in image order, as ProgressiveFrame.moments."""
        return self._state_image("moments")

    def save(self):
        """(blob, moments | None): the whole image's version-1 blob, header (rt_frame_save_header) plus the
        assembled sums, byte for byte the unsharded frame's `save()`, and with a tracked frame its moments
        in image order: what `restore` and `Context.restore_frame` take. (None, None) off the root."""
        head = self.frames[0].save_header()
        sums = self._state_image("sums")
        q = self.moments() if self.tracks_moments else None
        if self.rank != 0:
            return None, None
        return head + np.ascontiguousarray(sums, dtype="<f8").tobytes(), q

    def checkpoint(self) -> Optional[bytes]:
        """The whole image's version-2 checkpoint, byte for byte the unsharded frame's `checkpoint()`: the header
        (rt_frame_checkpoint_header; sections and chunks_done reduced over the shards), the assembled sums, the
        assembled moments of a tracked frame, and, when a pixel is stopped, the shards' raw K_p merged through
        `shard_pixel_map`. What `resume` and `Context.resume_frame` take. None off the root."""
        torch = self._torch()
        stops = int(any(f.active_pixels < f.owned_pixels for f in self.frames))
        if not self.local and self.world > 1:
            stops = self._max_int(stops)
        sections = (_rt.RT_CKPT_MOMENTS if self.tracks_moments else 0) | (_rt.RT_CKPT_STOPS if stops else 0)
        head = self.frames[0].checkpoint_header(sections, self.chunks_done)
        sums = self._state_image("sums")
        q = self.moments() if self.tracks_moments else None
        k = None
        if stops:
            ks = self._slabs_of(lambda f: f.slab_tensor(torch.int32, 0), lambda f, t: f.stops_into(t))
            allk = self._all_slabs(ks)
            k = self._merge_host(allk.cpu().numpy()) if self.rank == 0 else None
        if self.rank != 0:
            return None
        parts = [head, np.ascontiguousarray(sums, dtype="<f8").tobytes()]
        if q is not None:
            parts.append(np.ascontiguousarray(q, dtype="<f8").tobytes())
        if k is not None:
            parts.append(np.ascontiguousarray(k, dtype="<i4").tobytes())
        return b"".join(parts)

    # ---- guides, mattes and the denoised preview (rt.h: sharded feature and ID passes)
    def _record_pass(self, slabs, accumulate: bool, first_sample: int, n_samples: Optional[int], chain, ids: bool):
        """One slab pass per local shard into `slabs` (zeroed [slab, ...] tensors of 64-byte records on the shards'
        devices), the gather, and rt_assemble_records_async at the root: the [H, W, ...] tensor there, None elsewhere."""
        torch = self._torch()
        n = self.spp if n_samples is None else int(n_samples)
        for f, t in zip(self.frames, slabs):
            st = torch.cuda.current_stream(t.device).cuda_stream  # (after the tensor's fill, before the copies below)
            call = f._ctx.render_ids_shard_async if ids else f._ctx.render_features_shard_async
            call(self.cam, f.params, t.data_ptr(), first_sample, n, chain=chain, accumulate=accumulate, stream=st)
        for t in slabs:
            torch.cuda.current_stream(t.device).synchronize()
        gathered = self._all_slabs(slabs)
        if self.rank != 0:
            return None
        gathered = gathered.contiguous()
        img = torch.zeros((self.height, self.width) + tuple(gathered.shape[2:]), dtype=gathered.dtype,
                          device=gathered.device)
        self.root.assemble_records_async(self.p, gathered.data_ptr(), img.data_ptr(),
                                         stream=torch.cuda.current_stream(gathered.device).cuda_stream)
        torch.cuda.current_stream(gathered.device).synchronize()
        return img

    def render_features(self, first_sample: int = 0, n_samples: Optional[int] = None, chain=None, into=None):
        """The feature sums of samples first_sample .. first_sample + n_samples - 1 (default: the frame's spp), every
        shard rendering its slab (`Context.render_features_shard_async`; with `chain`, the specular-chain pass), as
        a [H, W, 8] float64 torch tensor on the root device (None on the other ranks): byte for byte what
        `Context.render_features` gives for the whole image. The object keeps the shards' slabs; `into` (the
        tensor an earlier call returned, or True) accumulates this range onto them, so a progressive caller adds
        [k0, k1) without rendering or gathering the earlier samples again. Without `into` the slabs start from 0.
        `into` is a request, not a buffer: the sums are the kept slabs', whatever tensor is passed. It needs kept
        slabs of the same chain whose samples end where this range begins; anything else raises RTError, since
        the sum would be of no sample range."""
        torch = self._torch()
        accumulate = into is not None and into is not False
        n = self.spp if n_samples is None else int(n_samples)
        key = None if chain is None else (chain.max_bounces, chain.flags, chain.max_fuzz)
        if accumulate:
            if self._feature_slabs is None:
                raise _rt.RTError("render_features: `into` without an earlier call whose slabs it could add to")
            if self._feature_kept != (key, int(first_sample)):
                raise _rt.RTError("render_features: `into` must continue the kept slabs: the same chain, and "
                                  f"first_sample = {self._feature_kept[1]}, where their samples end")
        else:
            self._feature_slabs = [torch.zeros((f.slab_pixels, _rt.RT_FEATURE_DOUBLES), dtype=torch.float64,
                                               device=f"cuda:{f._ctx.device}") for f in self.frames]
        self._feature_kept = (key, int(first_sample) + n)  # (the kept slabs' chain and the end of their samples)
        return self._record_pass(self._feature_slabs, accumulate, int(first_sample), n, chain, ids=False)

    def render_ids(self, first_sample: int = 0, n_samples: Optional[int] = None, chain=None):
        """The material-ID records of the same samples, every shard rendering its slab, as an (H, W) numpy array of
        ID_DTYPE (None off the root): byte for byte what `Context.render_ids` gives for the whole image."""
        torch = self._torch()
        slabs = [torch.zeros((f.slab_pixels, 64), dtype=torch.uint8, device=f"cuda:{f._ctx.device}")
                 for f in self.frames]
        img = self._record_pass(slabs, False, int(first_sample), n_samples, chain, ids=True)
        if img is None:
            return None
        return img.cpu().numpy().view(_rt.ID_DTYPE).reshape(self.height, self.width)

    def denoise(self, feature_sums, feature_samples: int, rgb: bool = True, linear: bool = True, **params):
        """(rgb8[H,W,3] | None, linear[H,W,3] | None, stats dict) of the frame's current preview through the
        feature-guided denoiser, what `ProgressiveFrame.denoise` returns for the unsharded frame at the same
        chunks_done: the shards' previews are assembled on the root device, and their error maps when the frame
        tracks moments and has two chunks, and rt_denoise_async filters the assembled image there (no halo
        exchange between shards); only the result is copied back. `feature_sums`: [H, W, 8], e.g. what
        `render_features` returned (a torch tensor, moved to the root device if it is elsewhere, or a numpy array).
        The counts rt_denoise_async does not report are taken on the device, by rt.h's rule: a pixel is valid when
        its three channels are finite; kernel_ms is the filter's time by device events. The frame is left as it
        is: a `resolve` after it reports what it would have reported. (None, None, {}) on a rank other than 0."""
        torch = self._torch()
        p = _rt.make_denoise_params(self.width, self.height, int(feature_samples), **params)
        with_se = self.tracks_moments and self.chunks_done >= 2
        lins = self._slabs_of(lambda f: f.slab_tensor(torch.float64), lambda f, t: f.resolve_into(None, t))
        d_lin = self._assemble_device(self._all_slabs(lins))
        d_se = None
        if with_se:
            ses = self._slabs_of(lambda f: f.slab_tensor(torch.float64), lambda f, t: f.error_into(t))
            d_se = self._assemble_device(self._all_slabs(ses))
        if self.rank != 0:
            return None, None, {}
        dev = d_lin.device
        if isinstance(feature_sums, np.ndarray):
            feature_sums = torch.from_numpy(_doubles(feature_sums, (self.height, self.width, _rt.RT_FEATURE_DOUBLES)))
        d_feat = feature_sums.to(dev).contiguous()
        d_out = torch.zeros((self.height, self.width, 3), dtype=torch.float64, device=dev)
        d_rgb = torch.zeros((self.height, self.width, 3), dtype=torch.uint8, device=dev) if rgb else None
        st = torch.cuda.current_stream(dev)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(st)
        self.root.denoise_async(p, d_lin.data_ptr(), d_se.data_ptr() if with_se else 0, d_feat.data_ptr(),
                                d_out.data_ptr(), d_rgb.data_ptr() if rgb else 0, stream=st.cuda_stream)
        t1.record(st)
        was, now = torch.isfinite(d_lin).all(dim=-1), torch.isfinite(d_out).all(dim=-1)
        n_in, n_out, n_fill = (int(x) for x in torch.stack([(~was).sum(), (~now).sum(), (~was & now).sum()]).cpu())
        stats = {"pixels": self.width * self.height, "invalid_in": n_in, "invalid_out": n_out, "filled": n_fill,
                 "kernel_ms": t0.elapsed_time(t1)}
        return (d_rgb.cpu().numpy() if rgb else None), (d_out.cpu().numpy() if linear else None), stats

    @classmethod
    def resume(cls, ctxs, blob: bytes, *, world: Optional[int] = None, rank: Optional[int] = None,
               backend: str = "nccl", gather: Optional[bool] = None):
        """The frame a whole-image checkpoint (`checkpoint`'s, or ProgressiveFrame.checkpoint's; a version-1 blob
        too) holds, over `world` shards, with its moments and stopped pixels: the shard count of the saved frame
        does not matter. Local mode: world defaults to len(ctxs)."""
        info = checkpoint_info(blob)
        local = isinstance(ctxs, (list, tuple))
        m = len(ctxs) if local and world is None else world
        if m is None or (local and m != len(ctxs)):
            raise ValueError("world must be given (local mode: one context per shard)")
        pairs = list(zip(ctxs, range(m))) if local else [(ctxs, rank)]
        frames = [resume_shard_frame(c, blob, r, m) for c, r in pairs]
        fr = cls(ctxs, info["camera"], info["params"], info["Q"] is not None, rank=rank, world=m, backend=backend,
                 gather=gather, _frames=frames)
        fr.active_pixels = info["active_pixels"]
        return fr

    def close(self):
        for f in self.frames:
            f.close()
        self.frames = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
