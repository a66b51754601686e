"""Checkpoints of progressive frames without a GPU (include/rt.h, the version-2 blob): the bindings, the
layout as rt.h documents it (built here byte by byte with struct, not with the library's writer) for all four
section combinations, its validation, rt_checkpoint_resolve and rt_checkpoint_error against a numpy
restatement, a committed checkpoint of a real frame (tests/golden/checkpoint_v2_three_spheres.bin), and the
host-only unit under AddressSanitizer + UBSan in a stand-alone C program (tests/c/checkpoint_check.c)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import rtamd
from test_progressive_host import make_blob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
HEADER = 320
MOMENTS, STOPS = 1, 2
E_INVALID = r"\(-1\)"


def make_ckpt(sections, S=None, Q=None, K=None, w=8, h=8, spp=40, chunks_done=7, reserved=bytes(28), **over):
    """A version-2 checkpoint in rt.h's layout: the version-1 header of make_blob with version 2 and the payload
    size of `sections`, the sections word, the reserved bytes, then S, Q and K (zeros when not given)."""
    n = w * h
    payload = n * (24 + (24 if sections & MOMENTS else 0) + (4 if sections & STOPS else 0))
    f = dict(version=2, payload_bytes=payload)
    f.update(over)
    head = make_blob(w, h, spp, chunks_done, **f)[:288] + struct.pack("<I", sections) + reserved
    assert len(head) == HEADER
    body = np.zeros((n, 3)) if S is None else np.asarray(S, np.float64).reshape(n, 3)
    out = head + body.astype("<f8").tobytes()
    if sections & MOMENTS:
        out += (np.zeros((n, 3)) if Q is None else np.asarray(Q, np.float64).reshape(n, 3)).astype("<f8").tobytes()
    if sections & STOPS:
        out += (np.zeros(n, np.int32) if K is None else np.asarray(K).reshape(n)).astype("<i4").tobytes()
    return out


def test_bindings_sizes_and_null_arguments():
    L = rtamd.lib()
    assert L.rt_abi_version() == 1
    for name in ("rt_frame_checkpoint_info", "rt_checkpoint_resolve", "rt_checkpoint_error", "rt_frame_checkpoint",
                 "rt_frame_resume", "rt_frame_resume_shard", "rt_frame_shard_stops", "rt_frame_checkpoint_header"):
        assert hasattr(L, name) and name in rtamd.EXPORTED
    assert C.sizeof(rtamd.rt_frame_ckpt_desc) == 344 and C.sizeof(rtamd.rt_frame_blob_desc) == 288
    assert rtamd.rt_frame_ckpt_desc.sections.offset == 288 and rtamd.rt_frame_ckpt_desc.sums_offset.offset == 296
    assert rtamd.RT_CKPT_MOMENTS == 1 and rtamd.RT_CKPT_STOPS == 2
    assert hasattr(rtamd.ProgressiveFrame, "checkpoint")
    assert hasattr(rtamd.Context, "resume_frame") and hasattr(rtamd.Context, "resume_shard_frame")
    for attr in ("stops_into", "stops", "checkpoint_header"):
        assert hasattr(rtamd.ShardFrame, attr)
    assert hasattr(rtamd.ShardedProgressiveFrame, "checkpoint") and hasattr(rtamd.ShardedProgressiveFrame, "resume")
    assert callable(rtamd.checkpoint_info) and callable(rtamd.checkpoint_resolve) and callable(rtamd.checkpoint_error)
    # null arguments are argument errors, not crashes
    h = C.c_void_p()
    buf = C.create_string_buffer(HEADER)
    n = C.c_size_t(0)
    assert L.rt_frame_checkpoint_info(None, 0, None) == rtamd.RT_E_INVALID
    assert L.rt_checkpoint_resolve(None, 0, None, None, None) == rtamd.RT_E_INVALID
    assert L.rt_checkpoint_error(None, 0, None, None, None) == rtamd.RT_E_INVALID
    assert L.rt_frame_checkpoint(None, buf, HEADER, C.byref(n)) == rtamd.RT_E_INVALID
    assert L.rt_frame_resume(None, buf, HEADER, C.byref(h)) == rtamd.RT_E_INVALID
    assert L.rt_frame_resume(None, buf, HEADER, None) == rtamd.RT_E_INVALID
    assert L.rt_frame_resume_shard(None, buf, HEADER, 0, 1, C.byref(h)) == rtamd.RT_E_INVALID
    assert L.rt_frame_shard_stops(None, None) == rtamd.RT_E_INVALID
    assert L.rt_frame_checkpoint_header(None, 0, -1, buf, HEADER) == rtamd.RT_E_INVALID


@pytest.mark.parametrize("sections", [0, MOMENTS, STOPS, MOMENTS | STOPS])
def test_checkpoint_info_reads_the_documented_layout(sections):
    rng = np.random.default_rng(sections)
    S, Q = rng.random((8, 8, 3)), rng.random((8, 8, 3))
    S[1, 2, 0] = S[5, 5, 2] = S[7, 0, 1] = np.nan
    K = np.zeros((8, 8), np.int32)
    K[1, 2], K[3, 3], K[4, :] = 7, 1, 5  # (1, 2) is a stopped NaN pixel; (5, 5) and (7, 0) are active ones
    blob = make_ckpt(sections, S, Q, K)
    info = rtamd.checkpoint_info(blob)
    assert info["version"] == 2 and info["sections"] == sections
    assert info["width"] == 8 and info["height"] == 8 and info["spp"] == 40 and info["max_depth"] == 10
    assert info["seed"] == 1024 and info["tile"] == 8 and info["scene_fingerprint"] == 0x0123456789ABCDEF
    assert info["chunk"] == 1 and info["chunks_total"] == 40 and info["chunks_done"] == 7 and info["samples_done"] == 7
    assert info["camera"].lens_radius == 21.5
    n_sec = 1 + bool(sections & MOMENTS)
    assert info["pixels"] == 64 and info["payload_bytes"] == len(blob) - HEADER == 64 * (24 * n_sec + 4 * bool(sections & STOPS))
    assert info["sums_offset"] == HEADER
    assert info["moments_offset"] == (HEADER + 64 * 24 if sections & MOMENTS else 0)
    assert info["stops_offset"] == (HEADER + 64 * 24 * n_sec if sections & STOPS else 0)
    assert np.array_equal(info["S"], S, equal_nan=True) and info["S"].shape == (8, 8, 3)
    if sections & MOMENTS:
        assert np.array_equal(info["Q"], Q)
    else:
        assert info["Q"] is None
    if sections & STOPS:
        assert np.array_equal(info["K"], K) and info["K"].dtype == np.int32
        assert (info["stopped_pixels"], info["stopped_nan"], info["active_pixels"]) == (10, 1, 54)
    else:
        assert info["K"] is None
        assert (info["stopped_pixels"], info["stopped_nan"], info["active_pixels"]) == (0, 0, 64)


def test_a_version_1_blob_passes_checkpoint_info():
    blob = make_blob(256, 192, 99, 19)
    info = rtamd.checkpoint_info(blob)
    assert info["version"] == 1 and info["sections"] == 0 and info["sums_offset"] == 288
    assert info["moments_offset"] == 0 and info["stops_offset"] == 0
    assert info["payload_bytes"] == 256 * 192 * 24 and info["samples_done"] == 95 and info["chunks_total"] == 20
    assert (info["stopped_pixels"], info["stopped_nan"], info["active_pixels"]) == (0, 0, 256 * 192)
    assert info["S"].shape == (192, 256, 3) and info["Q"] is None and info["K"] is None
    # rt_frame_blob_info keeps rejecting version 2
    with pytest.raises(rtamd.RTError, match=E_INVALID):
        rtamd.blob_info(make_ckpt(0))


def _k(value):
    k = np.zeros(64, np.int32)
    k[63] = value
    return k


BOTH = MOMENTS | STOPS
V1_CASES = [  # the version-1 table's cases (tests/test_progressive_host.py) with version = 2
    ("magic", dict(magic=b"RTFRAMF\0")), ("chunks_done above the total", dict(chunks_done=41)),
    ("chunks_done negative", dict(chunks_done=-1)), ("width zero", dict(width=0)), ("width negative", dict(width=-8)),
    ("tier A", dict(rng_mode=rtamd.RT_RNG_EXACT)), ("chunk size", dict(chunk=2)), ("pixel count", dict(pixels=65)),
    ("payload bytes", dict(payload_bytes=64 * 52 - 8)),
]


@pytest.mark.parametrize("what, blob", [
    ("an unknown section bit", make_ckpt(BOTH)[:288] + struct.pack("<I", BOTH | 4) + make_ckpt(BOTH)[292:]),
    ("only an unknown section bit", make_ckpt(0)[:288] + struct.pack("<I", 4) + make_ckpt(0)[292:]),
    ("a reserved byte set", make_ckpt(BOTH, reserved=bytes(27) + b"\1")),
    ("the first reserved byte set", make_ckpt(0, reserved=b"\x80" + bytes(27))),
    ("K = -1", make_ckpt(BOTH, K=_k(-1))),
    ("K = chunks_done + 1", make_ckpt(STOPS, K=_k(8))),
    ("one byte short", make_ckpt(BOTH)[:-1]),
    ("one byte long", make_ckpt(BOTH) + b"\0"),
    ("a Q section flagged but absent", make_ckpt(STOPS)[:288] + struct.pack("<I", BOTH) + make_ckpt(STOPS)[292:]),
    ("a Q section flagged, payload size adjusted, but absent", make_ckpt(MOMENTS)[:HEADER + 64 * 24]),
    ("header only", make_ckpt(BOTH)[:HEADER]),
    ("a version-1 header's length", make_ckpt(0)[:288]),
    ("half a header", make_ckpt(0)[:HEADER // 2]),
    ("version 3", make_ckpt(0, version=3)),
    ("version 0", make_ckpt(0, version=0)),
] + [(what + " (version 2)", make_ckpt(BOTH, **kw)) for what, kw in V1_CASES])
def test_checkpoint_corruptions_are_invalid(what, blob):
    L = rtamd.lib()
    d = rtamd.rt_frame_ckpt_desc()
    assert L.rt_frame_checkpoint_info(blob, len(blob), C.byref(d)) == rtamd.RT_E_INVALID, what
    assert b"frame blob:" in L.rt_last_error()
    assert L.rt_checkpoint_resolve(blob, len(blob), None, None, None) == rtamd.RT_E_INVALID
    assert L.rt_checkpoint_error(blob, len(blob), None, None, None) == rtamd.RT_E_INVALID
    with pytest.raises(rtamd.RTError, match=E_INVALID):
        rtamd.checkpoint_info(blob)


def test_k_at_the_ends_of_its_range_is_valid():
    assert rtamd.checkpoint_info(make_ckpt(STOPS, K=_k(7)))["stopped_pixels"] == 1
    assert rtamd.checkpoint_info(make_ckpt(STOPS, K=_k(0)))["stopped_pixels"] == 0
    assert rtamd.checkpoint_info(make_ckpt(STOPS, chunks_done=0))["active_pixels"] == 64


# ------------------------------------------------------------------ the offline preview and error map
def numpy_resolve(S, K, chunk, spp, samples_done):
    """rt.h in numpy: per pixel S / N_p, then scaleColor (sqrt, clamp to [0, 0.999], floor(256 x); NaN -> 0)."""
    S = np.asarray(S, np.float64)
    N = np.where(K != 0, np.minimum(spp, K.astype(np.int64) * chunk), samples_done).astype(np.float64)[..., None]
    with np.errstate(all="ignore"):
        lin = S / N
        s = np.sqrt(lin)
        cl = np.where(s < 0.0, 0.0, np.where(s > 0.999, 0.999, s))
        f = np.floor(256 * cl)
        rgb = np.where(np.isnan(f), 0.0, f).astype(np.uint8)
    return rgb, lin, int(np.isnan(S).any(axis=-1).sum()), int((rgb != 0).sum())


def numpy_error(S, Q, K, chunk, spp, chunks_done, samples_done, abs_tol, rel_tol):
    """rt.h's estimate in numpy, operation by operation, per pixel at (K_p, N_p); K_p < 2: NaN, non-finite."""
    S, Q = np.asarray(S, np.float64).reshape(-1, 3), np.asarray(Q, np.float64).reshape(-1, 3)
    K = np.asarray(K).reshape(-1)
    Kp = np.where(K != 0, K, chunks_done).astype(np.int64)
    Np = np.where(K != 0, np.minimum(spp, Kp * chunk), samples_done).astype(np.float64)[:, None]
    with np.errstate(all="ignore"):
        t = (S * S) / Np
        d = Q - t
        d = np.where(d < 0, 0.0, d)
        se = np.sqrt((d / (Kp - 1).astype(np.float64)[:, None]) / Np)
        se[Kp < 2] = np.nan
        finite = np.isfinite(se).all(axis=1)
        conv = (se <= abs_tol + rel_tol * np.abs(S / Np)).all(axis=1)
    total = 0.0
    for v in se[finite].reshape(-1):
        total = total + float(v)
    n = int(finite.sum())
    return se, {"chunks_done": chunks_done, "samples_done": samples_done, "pixels": len(S), "nonfinite_pixels": len(S) - n,
                "unconverged_pixels": int((finite & ~conv).sum()),
                "max_se": float(se[finite].max()) if n else 0.0, "mean_se": total / (3 * n) if n else 0.0}


def offline_case():
    """An 8x8 frame at 40000 spp: CH = 3, 13334 chunks, the last of one sample; all chunks done, so both the frame's
    samples_done and a pixel stopped at the last chunk meet min(spp, K * CH). NaN and infinite sums, pixels
    stopped after one chunk (K_p = 1: no estimate), in between, and at the end."""
    w = h = 8
    spp, chunk, total = 40000, 3, 13334
    assert rtamd.frame_chunking(w * h, spp) == (chunk, total) and total * chunk > spp
    rng = np.random.default_rng(7)
    K = np.zeros((h, w), np.int32)
    K[0, :], K[1, :4], K[2, ::2], K[7, 7] = 1, total, rng.integers(2, total, 4), 2
    Kp = np.where(K != 0, K, total)
    N = np.minimum(spp, Kp * chunk).astype(np.float64)[..., None]
    mean = 10.0 ** rng.uniform(-3, 1, size=(h, w, 3))
    S = mean * N
    Q = S * S / N * (1.0 + 10.0 ** rng.uniform(-6, -1, size=(h, w, 3)))
    Q[3, 3] = S[3, 3] * S[3, 3] / N[3, 3] * 0.5  # d < 0: clamped to 0, se 0
    S[0, 1, 0] = S[1, 1, 2] = S[4, 4, 1] = np.nan   # stopped at 1, stopped at the end, active
    S[2, 0, 1] = S[5, 5, 0] = np.inf                # stopped in between, active
    Q[2, 0, 1] = Q[5, 5, 0] = np.inf                # (an infinite chunk sum's square)
    S[6, 6] = 0.0
    S[6, 7] = -1e-3                                 # a negative mean: sqrt gives NaN, the byte 0
    return S, Q, K, spp, chunk, total


@pytest.mark.parametrize("sections", [BOTH, MOMENTS, STOPS, 0])
def test_offline_resolve_and_error_equal_the_numpy_restatement(sections):
    S, Q, K, spp, chunk, total = offline_case()
    blob = make_ckpt(sections, S, Q, K, spp=spp, chunks_done=total)
    k = K if sections & STOPS else np.zeros_like(K)
    rgb, lin, st = rtamd.checkpoint_resolve(blob)
    want_rgb, want_lin, nan_pixels, nonzero = numpy_resolve(S, k, chunk, spp, spp)
    assert np.array_equal(rgb, want_rgb)
    assert np.array_equal(lin, want_lin, equal_nan=True)
    fin = np.isfinite(want_lin)
    assert np.array_equal(lin[fin].view(np.uint64), want_lin[fin].view(np.uint64))
    assert st == {"chunk": chunk, "chunks_total": total, "chunks_done": total, "samples_done": spp, "kernel_ms": 0.0,
                  "nan_pixels": nan_pixels, "bytes_changed": nonzero}
    assert nan_pixels == 3 and rgb[5, 5, 0] == 255 and (rgb[6, 7] == 0).all() and 0 < nonzero < 192
    assert rtamd.checkpoint_resolve(blob, rgb=False, linear=False)[2] == st
    if not sections & MOMENTS:
        with pytest.raises(rtamd.RTError, match=E_INVALID):
            rtamd.checkpoint_error(blob)
        return
    for tol in [(0.0, 0.0), (0.0, 1e-3)]:
        se, est = rtamd.checkpoint_error(blob, *tol)
        want_se, want_st = numpy_error(S, Q, k, chunk, spp, total, spp, *tol)
        want_se = want_se.reshape(8, 8, 3)
        assert np.array_equal(se, want_se, equal_nan=True)
        fin = np.isfinite(want_se)
        assert np.array_equal(se[fin].view(np.uint64), want_se[fin].view(np.uint64))
        for key in ("chunks_done", "samples_done", "pixels", "nonfinite_pixels", "unconverged_pixels", "max_se"):
            assert est[key] == want_st[key], key
        assert abs(est["mean_se"] - want_st["mean_se"]) <= 1e-12 * want_st["mean_se"]
        assert se[3, 3].tolist() == [0.0, 0.0, 0.0]
        if sections & STOPS:
            assert np.isnan(se[0]).all() and est["nonfinite_pixels"] >= 8 + 4
        if tol != (0.0, 0.0):
            assert 0 < est["unconverged_pixels"] < 64 - est["nonfinite_pixels"]
        assert rtamd.checkpoint_error(blob, *tol, want_map=False)[1] == est


def test_offline_calls_check_their_arguments():
    S, Q, K, spp, chunk, total = offline_case()
    with pytest.raises(rtamd.RTError, match=E_INVALID):  # no chunk rendered yet
        rtamd.checkpoint_resolve(make_ckpt(MOMENTS, chunks_done=0))
    with pytest.raises(rtamd.RTError, match=E_INVALID):  # the estimate needs two chunks
        rtamd.checkpoint_error(make_ckpt(MOMENTS, chunks_done=1))
    assert rtamd.checkpoint_error(make_ckpt(MOMENTS, chunks_done=2))[1]["pixels"] == 64
    for tol in [(-1.0, 0.0), (0.0, float("nan"))]:
        with pytest.raises(rtamd.RTError, match=E_INVALID):
            rtamd.checkpoint_error(make_ckpt(BOTH, S, Q, K, spp=spp, chunks_done=total), *tol)
    # a version-1 blob resolves (sections 0) and has no error map
    v1 = make_blob(8, 8, 40, 7)
    rgb, lin, st = rtamd.checkpoint_resolve(v1)
    assert (rgb == 0).all() and (lin == 0).all() and st["samples_done"] == 7 and st["bytes_changed"] == 0
    with pytest.raises(rtamd.RTError, match=E_INVALID):
        rtamd.checkpoint_error(v1)


# ------------------------------------------------------------------ a real frame's checkpoint
def test_the_committed_checkpoint_parses_and_previews():
    """tests/golden/checkpoint_v2_three_spheres.bin: 64x48x6, three_spheres, depth 8, tracked, stopped by a mask
    after 2 chunks, saved after 4 (tests/test_gpu_checkpoint.py writes the same bytes); beside it the bytes of the
    frame's own preview at that point."""
    blob = open(os.path.join(GOLDEN, "checkpoint_v2_three_spheres.bin"), "rb").read()
    assert len(blob) == 160064 == HEADER + 64 * 48 * 52
    assert blob[:8] == b"RTFRAME\0" and struct.unpack_from("<II", blob, 8) == (2, 0)
    assert struct.unpack_from("<I", blob, 288)[0] == BOTH and blob[292:320] == bytes(28)
    info = rtamd.checkpoint_info(blob)
    assert (info["width"], info["height"], info["spp"], info["max_depth"], info["tile"]) == (64, 48, 6, 8, 8)
    assert (info["chunk"], info["chunks_total"], info["chunks_done"], info["samples_done"]) == (1, 6, 4, 4)
    assert info["sections"] == BOTH and info["shard_rank"] == 0 and info["shard_count"] == 1
    yy, xx = np.mgrid[0:48, 0:64]
    mask = (7 * xx + 13 * yy) % 3 == 0
    assert np.array_equal(info["K"], np.where(mask, 2, 0))
    assert info["stopped_pixels"] == int(mask.sum()) and info["active_pixels"] == 64 * 48 - int(mask.sum())
    scene = rtamd.make_scene("three_spheres", rtamd.randGen(1024))[0]
    assert info["scene_fingerprint"] == rtamd.scene_fingerprint(scene)
    rgb, lin, st = rtamd.checkpoint_resolve(blob)
    want = np.fromfile(os.path.join(GOLDEN, "checkpoint_v2_three_spheres_preview.bin"), dtype=np.uint8)
    assert np.array_equal(rgb.reshape(-1), want)
    assert st["nan_pixels"] == int(np.isnan(info["S"]).any(axis=2).sum())
    k = info["K"]
    assert np.array_equal(lin, info["S"] / np.where(k != 0, k, 4)[..., None].astype(np.float64), equal_nan=True)
    se, est = rtamd.checkpoint_error(blob)
    assert est["pixels"] == 64 * 48 and est["chunks_done"] == 4 and np.isfinite(se[~np.isnan(info["S"]).any(axis=2)]).all()


def test_checkpoint_unit_is_sanitizer_clean(tmp_path):
    """tests/c/checkpoint_check.c with the host-only unit under ASan + UBSan, as a child process: every header
    byte of each section combination changed, every length from 0 to the full blob, each in a heap block of
    exactly that length, and the two offline calls on whatever parses."""
    csrc = os.path.join(ROOT, "ray-tracing_amd", "csrc")
    exe = str(tmp_path / "checkpoint_check")
    obj = str(tmp_path / "checkpoint_check.o")
    # (the sanitizer runtimes linked into the program itself: it needs nothing from its environment)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1",
           "-static-libasan", "-static-libubsan"]
    fp = ["-ffp-contract=off", "-fno-fast-math"]
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + csrc]
    subprocess.run(["gcc", "-std=c11", "-Wall", *san, *fp, *inc, "-c",
                    os.path.join(ROOT, "tests", "c", "checkpoint_check.c"), "-o", obj], check=True, timeout=300)
    subprocess.run(["gcc", "-std=c++17", "-Wall", *san, *fp, *inc, obj, os.path.join(csrc, "rt_frame_blob.cpp"),
                    os.path.join(csrc, "rt_scene.cpp"), "-lstdc++", "-lm", "-o", exe], check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    print(r.stdout[-4000:], r.stderr[-4000:])
    assert r.returncode == 0, r.stderr[-2000:]
    assert "checkpoint_check: clean (0 failures)" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
