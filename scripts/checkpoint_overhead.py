"""What a checkpoint costs (the protocol of profiles/frame_helper_calls.jsonl): C2's 1200x800
frame, tracked, 8 chunks rendered, both stop rules applied once at (0.002, 0.02), so that the checkpoint has
all three sections (a 50 MB blob). 2 warm-up calls then 10 timed, host clock around the C call, the blob in a
buffer allocated once. One JSON line per call on stdout.

    python scripts/checkpoint_overhead.py [label]
"""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(os.path.join(ROOT, "ray-tracing_amd"))

import rtamd  # noqa: E402

WARMUP, REPS = 2, 10


def timed(label, call, fn, **more):
    ms = []
    for i in range(WARMUP + REPS):
        t0 = time.perf_counter()
        fn()
        if i >= WARMUP:
            ms.append((time.perf_counter() - t0) * 1e3)
    out = {"label": label, "call": call, "median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
           "max_ms": round(max(ms), 4), "all_ms": [round(x, 4) for x in ms]}
    out.update(more)
    print(json.dumps(out), flush=True)


def main():
    label = sys.argv[1] if len(sys.argv) > 1 else "checkpoint"
    L = rtamd.lib()
    scene, _ = rtamd.make_scene("random_book_one", rtamd.randGen(1024))
    cam = rtamd.camera("random_scene", 1200, 800)
    p = rtamd.make_params(1200, 800, 500, 50, rtamd.RT_RNG_PHILOX, seed=1024)
    ctx = rtamd.Context(0)
    ctx.upload(scene)
    with ctx.open_frame(cam, p, moments=True) as fr:
        fr.advance(8)
        st = fr.adapt(0.002, 0.02)
        n = C.c_size_t(0)
        rtamd._check(L.rt_frame_checkpoint(fr._h, None, 0, C.byref(n)), "rt_frame_checkpoint")
        buf = C.create_string_buffer(n.value)
        more = dict(blob_bytes=n.value, active_pixels=st["active_pixels"], stopped_nan=st["stopped_nan"],
                    stopped_converged=st["stopped_converged_or_masked"])
        timed(label, "rt_frame_checkpoint (S, Q, K)",
              lambda: rtamd._check(L.rt_frame_checkpoint(fr._h, buf, n.value, C.byref(n)), "rt_frame_checkpoint"), **more)
        v1 = C.create_string_buffer(288 + 1200 * 800 * 24)
        with ctx.open_frame(cam, p) as plain:
            plain.advance(1)
            m = C.c_size_t(0)
            timed(label, "rt_frame_save (S alone, for scale)",
                  lambda: rtamd._check(L.rt_frame_save(plain._h, v1, len(v1), C.byref(m)), "rt_frame_save"),
                  blob_bytes=len(v1))

    def resume():
        h = C.c_void_p()
        rtamd._check(L.rt_frame_resume(ctx._h, buf, n.value, C.byref(h)), "rt_frame_resume")
        L.rt_frame_close(h)

    timed(label, "rt_frame_resume + rt_frame_close (S, Q, K)", resume, **more)
    d = rtamd.rt_frame_ckpt_desc()
    timed(label, "rt_frame_checkpoint_info (host: the scan of K and S)",
          lambda: rtamd._check(L.rt_frame_checkpoint_info(buf, n.value, C.byref(d)), "rt_frame_checkpoint_info"), **more)
    ctx.close()


if __name__ == "__main__":
    main()
