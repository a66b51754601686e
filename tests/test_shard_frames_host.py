"""Shard frames without a GPU (include/rt.h, rt_frame_*_shard): the seven new symbols load, null arguments
are argument errors and not crashes, and rt_error_stats_merge puts the error stats of the shards of an image
together into rt_error_estimate's over the whole image (counts and max_se exactly, mean_se to the 1e-12
relative that rt.h states for the device sum)."""
import ctypes as C

import numpy as np
import pytest

import rtamd
from test_error_host import folded

NEW = ("rt_frame_open_shard", "rt_frame_resolve_shard", "rt_frame_error_shard", "rt_error_stats_merge",
       "rt_frame_shard_state", "rt_frame_save_header", "rt_frame_restore_shard")
W, H = 97, 61


def test_symbols_load_and_null_arguments_are_invalid():
    L = rtamd.lib()
    assert L.rt_abi_version() == 1
    for name in NEW:
        assert hasattr(L, name) and name in rtamd.EXPORTED
    for attr in ("resolve_into", "error_into", "state_into", "resolve", "error", "state", "adapt", "stop",
                 "save_header"):
        assert hasattr(rtamd.ShardFrame, attr)
    for attr in ("advance", "resolve", "error", "adapt", "stop", "chunk_counts", "save", "restore", "close"):
        assert hasattr(rtamd.ShardedProgressiveFrame, attr)
    assert hasattr(rtamd.Context, "open_shard_frame") and hasattr(rtamd.Context, "restore_shard_frame")
    h = C.c_void_p()
    buf = C.create_string_buffer(288)
    assert L.rt_frame_open_shard(None, None, None, 0, C.byref(h)) == rtamd.RT_E_INVALID
    assert L.rt_frame_open_shard(None, None, None, 0, None) == rtamd.RT_E_INVALID
    assert L.rt_frame_resolve_shard(None, None, None, None) == rtamd.RT_E_INVALID
    assert L.rt_frame_error_shard(None, None, None, None) == rtamd.RT_E_INVALID
    assert L.rt_frame_shard_state(None, None, None, None) == rtamd.RT_E_INVALID
    assert L.rt_frame_save_header(None, buf, 288) == rtamd.RT_E_INVALID
    assert L.rt_frame_restore_shard(None, None, 0, None, 0, 1, C.byref(h)) == rtamd.RT_E_INVALID
    assert L.rt_frame_restore_shard(None, None, 0, None, 0, 1, None) == rtamd.RT_E_INVALID
    st = rtamd.rt_error_stats()
    assert L.rt_error_stats_merge(None, 1, C.byref(st)) == rtamd.RT_E_INVALID
    assert L.rt_error_stats_merge(C.byref(st), 1, None) == rtamd.RT_E_INVALID
    assert L.rt_error_stats_merge(C.byref(st), 0, C.byref(st)) == rtamd.RT_E_INVALID
    assert b"rt_error_stats_merge" in L.rt_last_error()


def planted():
    """Image-order (S, Q, K, N) of a 97x61 frame of 7 chunks (5 samples, the last 2) with pixels of very
    different scales, and NaN and infinite sums planted across tiles."""
    n_k = [5] * 6 + [2]
    rng = np.random.default_rng(9761)
    scale = 10.0 ** rng.uniform(-3, 2, size=(1, W * H, 3))
    x = rng.random((len(n_k), W * H, 3)) * scale * np.asarray(n_k, np.float64).reshape(-1, 1, 1)
    S, Q, N = folded(x, n_k)
    bad = rng.choice(W * H, size=200, replace=False)
    S[bad[:120], rng.integers(0, 3, 120)] = np.nan
    S[bad[120:160], 0] = Q[bad[120:160], 0] = np.inf  # (an infinite chunk sum makes both infinite)
    Q[bad[160:], 2] = np.inf
    return S, Q, len(n_k), N


@pytest.mark.parametrize("tile, shards, empty", [(16, 3, 0), (64, 3, 1)])
def test_merged_shard_stats_equal_the_whole_image_estimate(tile, shards, empty):
    S, Q, K, N = planted()
    tol = (0.01, 0.02)
    _, whole = rtamd.error_estimate(S, Q, K, N, *tol)
    assert whole["nonfinite_pixels"] == 200 and 0 < whole["unconverged_pixels"] < whole["pixels"] - 200
    parts, seen = [], np.zeros(W * H, int)
    for r in range(shards):
        m = rtamd.shard_pixel_map(rtamd.make_params(W, H, N, 8, tile=tile, shard_rank=r, shard_count=shards))
        own = m[m >= 0]
        seen[own] += 1
        if len(own):
            parts.append(rtamd.error_estimate(S[own], Q[own], K, N, *tol)[1])
        else:  # (a shard without pixels: what rt_frame_error_shard reports for it; the estimate needs a pixel)
            parts.append({"chunks_done": K, "samples_done": N, "pixels": 0, "nonfinite_pixels": 0,
                          "unconverged_pixels": 0, "max_se": 0.0, "mean_se": 0.0})
    assert (seen == 1).all()  # (the shards partition the image)
    assert sum(p["pixels"] == 0 for p in parts) == empty
    merged = rtamd.error_stats_merge(parts)
    for k in ("chunks_done", "samples_done", "pixels", "nonfinite_pixels", "unconverged_pixels", "max_se"):
        assert merged[k] == whole[k], k
    print("mean_se merged", merged["mean_se"], "whole", whole["mean_se"])
    assert abs(merged["mean_se"] - whole["mean_se"]) <= 1e-12 * whole["mean_se"]
    # one part merges to itself; parts whose pixels are all non-finite have mean 0 and do not weigh in
    assert rtamd.error_stats_merge([whole]) == whole
    nothing = dict(parts[0], pixels=5, nonfinite_pixels=5, unconverged_pixels=0, max_se=0.0, mean_se=0.0)
    again = rtamd.error_stats_merge(parts + [nothing])
    assert again["mean_se"] == merged["mean_se"] and again["nonfinite_pixels"] == merged["nonfinite_pixels"] + 5
    assert rtamd.error_stats_merge([nothing])["mean_se"] == 0.0


def test_parts_that_disagree_are_invalid():
    a = {"chunks_done": 4, "samples_done": 20, "pixels": 10, "nonfinite_pixels": 1, "unconverged_pixels": 2,
         "max_se": 0.5, "mean_se": 0.1}
    assert rtamd.error_stats_merge([a, a])["pixels"] == 20
    for other in (dict(a, chunks_done=5), dict(a, samples_done=19)):
        with pytest.raises(rtamd.RTError, match=r"\(-1\)"):
            rtamd.error_stats_merge([a, other])
    with pytest.raises(rtamd.RTError, match=r"\(-1\)"):
        rtamd.error_stats_merge([])
