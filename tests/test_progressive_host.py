"""Progressive frames without a GPU (include/rt.h, rt_frame_*): the bindings, the saved frame's header
as rt.h documents it (built here byte by byte, not with the library's writer), its validation, the
stopping rule of rtamd.render_progressive, and the blob parser under AddressSanitizer + UBSan in a
stand-alone C program (tests/c/frame_blob_check.c)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import rtamd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = 288


def make_blob(w=8, h=8, spp=40, chunks_done=7, **over):
    """A blob in rt.h's layout with a zero payload; `over` replaces single fields."""
    f = dict(magic=b"RTFRAME\0", version=1, upload_flags=0, width=w, height=h, spp=spp, max_depth=10,
             rng_mode=rtamd.RT_RNG_PHILOX, flags=0, seed=1024, tile=8, shard_rank=0, shard_count=1, pad=0,
             camera=[0.5 + i for i in range(24)], chunk=rtamd.sample_chunk(w * h, spp),
             chunks_done=chunks_done, pixels=w * h, fingerprint=0x0123456789ABCDEF,
             payload_bytes=w * h * 24)
    f.update(over)
    head = f["magic"] + struct.pack("<II", f["version"], f["upload_flags"])
    head += struct.pack("<iiiiiIQiiii", f["width"], f["height"], f["spp"], f["max_depth"], f["rng_mode"], f["flags"],
                        f["seed"], f["tile"], f["shard_rank"], f["shard_count"], f["pad"])
    head += struct.pack("<24d", *f["camera"])
    head += struct.pack("<iiqQQ", f["chunk"], f["chunks_done"], f["pixels"], f["fingerprint"], f["payload_bytes"])
    assert len(head) == HEADER
    return head + bytes(w * h * 24)


def test_bindings_exist_and_abi_version_stays_1():
    L = rtamd.lib()
    assert L.rt_abi_version() == 1
    for name in ("rt_frame_open", "rt_frame_advance", "rt_frame_resolve", "rt_frame_save", "rt_frame_restore",
                 "rt_frame_blob_info", "rt_frame_close", "rt_scene_fingerprint", "rt_frame_chunking"):
        assert hasattr(L, name) and name in rtamd.EXPORTED
    assert C.sizeof(rtamd.rt_frame_stats) == 40 and C.sizeof(rtamd.rt_frame_blob_desc) == HEADER
    for attr in ("open", "advance", "resolve", "save", "close", "__enter__", "__exit__"):
        assert hasattr(rtamd.ProgressiveFrame, attr)
    assert hasattr(rtamd.Context, "open_frame") and hasattr(rtamd.Context, "restore_frame")
    # null handles are argument errors, not crashes
    assert L.rt_frame_advance(None, 1, None) == rtamd.RT_E_INVALID
    assert L.rt_frame_resolve(None, None, None, None) == rtamd.RT_E_INVALID
    assert L.rt_frame_save(None, None, 0, None) == rtamd.RT_E_INVALID
    assert L.rt_frame_open(None, None, None, None) == rtamd.RT_E_INVALID
    L.rt_frame_close(None)


def test_frame_chunking_is_the_headers_rule():
    """rt_frame_chunking evaluates rt.h's rt_sample_chunk in C (rtamd.sample_chunk and ProgressiveFrame ask
    it): the values the GPU tests' shapes and the bench frames are built on, and bench.py's own mirror."""
    import bench
    for px, spp, ch in [(96 * 64, 40, 1), (256 * 192, 99, 5), (640 * 480, 60, 8), (1200 * 800, 500, 8),
                        (1200 * 800, 2000, 16), (1, 3, 1), (17 * 13, 3, 1), (200 * 100, 10, 1), (500 * 500, 1000, 8)]:
        assert rtamd.frame_chunking(px, spp) == (ch, -(-spp // ch))
        assert rtamd.sample_chunk(px, spp) == ch == bench.sample_chunk(px, spp)
    L = rtamd.lib()
    a, b = C.c_int(), C.c_int()
    for px, spp in [(0, 1), (1, 0), (1 << 32, 1), (1, 2 ** 31 - 1)]:
        assert L.rt_frame_chunking(px, spp, C.byref(a), C.byref(b)) == rtamd.RT_E_INVALID
    assert L.rt_frame_chunking(64, 8, None, None) == rtamd.RT_E_INVALID


def test_blob_info_reads_the_documented_layout():
    info = rtamd.blob_info(make_blob())
    assert info["version"] == 1 and info["width"] == 8 and info["height"] == 8 and info["spp"] == 40
    assert info["max_depth"] == 10 and info["seed"] == 1024 and info["tile"] == 8 and info["flags"] == 0
    assert info["chunk"] == 1 and info["chunks_total"] == 40 and info["chunks_done"] == 7 and info["samples_done"] == 7
    assert info["pixels"] == 64 and info["payload_bytes"] == 64 * 24 and info["scene_fingerprint"] == 0x0123456789ABCDEF
    cam = info["camera"]
    assert list(cam.origin) == [0.5, 1.5, 2.5] and cam.lens_radius == 21.5 and cam.t1 == 23.5
    # a short last chunk: 256x192 at 99 spp is 20 chunks of 5, the last of 4 samples
    info = rtamd.blob_info(make_blob(256, 192, 99, 20))
    assert info["chunk"] == 5 and info["chunks_total"] == 20 and info["samples_done"] == 99
    assert rtamd.blob_info(make_blob(256, 192, 99, 19))["samples_done"] == 95
    assert rtamd.blob_info(make_blob(chunks_done=0))["samples_done"] == 0


@pytest.mark.parametrize("what, blob", [
    ("magic", make_blob(magic=b"RTFRAMF\0")),
    ("version", make_blob(version=2)),
    ("one byte short", make_blob()[:-1]),
    ("one byte long", make_blob() + b"\0"),
    ("header only", make_blob()[:HEADER]),
    ("half a header", make_blob()[:HEADER // 2]),
    ("empty", b""),
    ("chunks_done above the total", make_blob(chunks_done=41)),
    ("chunks_done negative", make_blob(chunks_done=-1)),
    ("width zero", make_blob(width=0)),
    ("width negative", make_blob(width=-8)),
    ("tier A", make_blob(rng_mode=rtamd.RT_RNG_EXACT)),
    ("chunk size", make_blob(chunk=2)),
    ("pixel count", make_blob(pixels=65)),
    ("payload bytes", make_blob(payload_bytes=64 * 24 - 8)),
])
def test_blob_corruptions_are_invalid(what, blob):
    d = rtamd.rt_frame_blob_desc()
    assert rtamd.lib().rt_frame_blob_info(blob, len(blob), C.byref(d)) == rtamd.RT_E_INVALID, what
    assert b"frame blob" in rtamd.lib().rt_last_error()
    with pytest.raises(rtamd.RTError, match=r"\(-1\)"):
        rtamd.blob_info(blob)


def test_scene_fingerprint_tells_scenes_apart():
    a, _ = rtamd.make_scene("three_spheres", rtamd.randGen(1024))
    b, _ = rtamd.make_scene("three_spheres", rtamd.randGen(1024))
    c, _ = rtamd.make_scene("cornell", rtamd.randGen(1024))
    assert rtamd.scene_fingerprint(a) == rtamd.scene_fingerprint(b) != rtamd.scene_fingerprint(c)
    # FNV-1a over the arrays in rt.h's order, recomputed here
    h = 0xCBF29CE484222325
    d = a.desc
    parts = [(d.nodes, d.n_nodes, rtamd.rt_node), (d.materials, d.n_materials, rtamd.rt_material),
             (d.textures, d.n_textures, rtamd.rt_texture), (d.perlins, d.n_perlins, rtamd.rt_perlin),
             (d.images, d.n_images, rtamd.rt_image), (d.image_pool, d.image_pool_bytes, C.c_uint8)]
    data = b"".join(C.string_at(p, n * C.sizeof(t)) for p, n, t in parts if p and n > 0)
    data += struct.pack("<ii3d", d.world_root, d.lights_root, *d.background)
    for byte in data:
        h = ((h ^ byte) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    assert rtamd.scene_fingerprint(a) == h


class StubFrame:
    """A frame whose bytes_changed per step is scripted: render_progressive's loop without a device."""

    def __init__(self, total, changed):
        self.total, self.done, self.changed, self.steps, self.closed = total, 0, list(changed), [], False

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
        return np.full((4, 4, 3), self.done, np.uint8), None, {"chunks_done": self.done,
                                                                "bytes_changed": self.changed[len(self.steps) - 1]}

    def close(self):
        self.closed = True


class StubCtx:
    def __init__(self, frame):
        self.frame = frame

    def open_frame(self, cam, params):
        return self.frame


def test_render_progressive_stop_rule():
    p = rtamd.make_params(4, 4, 40, 5)  # 48 channels
    # no stop fraction: runs to completion, the last step short
    fr = StubFrame(10, [48] * 4)
    out = list(rtamd.render_progressive(StubCtx(fr), None, p, 3))
    assert fr.steps == [3, 3, 3, 1] and [s["chunks_done"] for _, s in out] == [3, 6, 9, 10] and fr.closed
    assert out[1][0][0, 0, 0] == 6
    # stops at the first step whose changed fraction falls to the bound (12 / 48 = 0.25), yielding it
    fr = StubFrame(10, [48, 30, 12, 0, 0])
    out = list(rtamd.render_progressive(StubCtx(fr), None, p, 2, stop_changed_fraction=0.25))
    assert fr.steps == [2, 2, 2] and len(out) == 3 and fr.closed
    # just above the bound: goes on
    fr = StubFrame(6, [48, 13, 13])
    assert len(list(rtamd.render_progressive(StubCtx(fr), None, p, 2, stop_changed_fraction=0.25))) == 3
    # fraction 0: only when no byte moved
    fr = StubFrame(100, [5, 1, 0, 7])
    assert len(list(rtamd.render_progressive(StubCtx(fr), None, p, 1, stop_changed_fraction=0.0))) == 3
    # a consumer that walks away closes the frame too
    fr = StubFrame(10, [48] * 10)
    gen = rtamd.render_progressive(StubCtx(fr), None, p, 1)
    next(gen)
    gen.close()
    assert fr.closed and fr.steps == [1]
    with pytest.raises(ValueError):
        next(rtamd.render_progressive(StubCtx(StubFrame(1, [0])), None, p, 0))


def test_blob_parser_is_sanitizer_clean(tmp_path):
    """tests/c/frame_blob_check.c with the host-only blob unit under ASan + UBSan, as a child process: the
    corruptions above plus every truncation length, each in a heap block of exactly that length."""
    csrc = os.path.join(ROOT, "ray-tracing_amd", "csrc")
    exe = str(tmp_path / "frame_blob_check")
    obj = str(tmp_path / "frame_blob_check.o")
    # (the sanitizer runtimes linked into the program itself: it needs nothing from its environment)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1",
           "-static-libasan", "-static-libubsan"]
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + csrc]
    subprocess.run(["gcc", "-std=c11", "-Wall", *san, *inc, "-c", os.path.join(ROOT, "tests", "c", "frame_blob_check.c"),
                    "-o", obj], check=True, timeout=300)
    # (rt_scene.cpp: rt_last_error / set_error; both units are C++, so the link goes through g++'s runtime)
    subprocess.run(["gcc", "-std=c++17", "-Wall", *san, *inc, obj, os.path.join(csrc, "rt_frame_blob.cpp"),
                    os.path.join(csrc, "rt_scene.cpp"), "-lstdc++", "-lm", "-o", exe], check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    print(r.stdout[-4000:], r.stderr[-4000:])
    assert r.returncode == 0, r.stderr[-2000:]
    assert "frame_blob_check: clean (0 failures)" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
