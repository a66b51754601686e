"""Progressive tier-B frames over the C ABI (include/rt.h, rt_frame_*): render a frame a few sample
chunks at a time, look at previews while it converges, stop when the bytes stop moving, or save the
running sums and finish later. A frame advanced to its end resolves to `Context.render`'s output bit
for bit, whatever the steps.

    with ctx.open_frame(cam, params) as fr:
        while not fr.complete:
            fr.advance(8)
            rgb, lin, stats = fr.resolve()

`render_progressive` wraps that loop as a generator with the 8-bit stopping rule.
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


def _stats_dict(s) -> dict:
    return {k: getattr(s, k) for k in STATS_FIELDS}


class ProgressiveFrame:
    """One open frame of a Context (rt_frame_open / rt_frame_restore). Also a context manager."""

    def __init__(self, ctx, handle, params):
        self._ctx = ctx
        self._h = handle
        self.width, self.height, self.spp = params.width, params.height, params.spp
        self.chunk, self.chunks_total = _rt.frame_chunking(self.width * self.height, self.spp)
        self.chunks_done = 0

    @classmethod
    def open(cls, ctx, cam, params) -> "ProgressiveFrame":
        h = C.c_void_p()
        _rt._check(_rt.lib().rt_frame_open(ctx._h, C.byref(cam), C.byref(params), C.byref(h)), "rt_frame_open")
        return cls(ctx, h, params)

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


def restore_frame(ctx, blob: bytes) -> ProgressiveFrame:
    info = blob_info(blob)
    h = C.c_void_p()
    _rt._check(_rt.lib().rt_frame_restore(ctx._h, blob, len(blob), C.byref(h)), "rt_frame_restore")
    fr = ProgressiveFrame(ctx, h, info["params"])
    fr.chunks_done = info["chunks_done"]
    return fr


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
                       stop_changed_fraction: Optional[float] = None) -> Iterator[Tuple[np.ndarray, dict]]:
    """Yields (rgb, stats) after each step of `step_chunks` chunks. Stops at completion, or once
    bytes_changed / (3*W*H) of a step is at most `stop_changed_fraction` (the 8-bit stopping rule: the
    bytes stopped moving). `ctx` needs `open_frame(cam, params)` returning a frame with `advance`,
    `resolve(linear=False)`, `complete` and `close`."""
    if step_chunks < 1:
        raise ValueError("step_chunks must be at least 1")
    channels = 3 * params.width * params.height
    frame = ctx.open_frame(cam, params)
    try:
        while not frame.complete:
            frame.advance(step_chunks)
            rgb, _, stats = frame.resolve(linear=False)
            yield rgb, stats
            if stop_changed_fraction is not None and stats["bytes_changed"] <= stop_changed_fraction * channels:
                break
    finally:
        frame.close()
