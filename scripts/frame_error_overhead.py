"""Overhead of progressive frames' error estimates on C2's bench frame (DESIGN.md §3.7's protocol): one
process per row, 2 warm-up frames then 10 timed, host clock around calls that end in a stream synchronise,
RGB8 download included, no linear image. One JSON line per run on stdout.

    python scripts/frame_error_overhead.py render            # rt_render (RTAMD_LIB selects the library)
    python scripts/frame_error_overhead.py frame 63          # untracked frame, steps of 63 chunks + 1 resolve
    python scripts/frame_error_overhead.py tracked 63        # tracked frame, the same steps
    python scripts/frame_error_overhead.py tracked 8         # tracked frame, steps of 8 chunks
    python scripts/frame_error_overhead.py error             # one rt_frame_error: stats only, and with the map
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(os.path.join(ROOT, "ray-tracing_amd"))  # (after PYTHONPATH: another commit's package goes there)

import rtamd  # noqa: E402

W, H, SPP, DEPTH = 1200, 800, 500, 50
WARMUP, REPS = 2, 10


def summary(mode, ms, **more):
    out = {"mode": mode, "reps": len(ms), "median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms),
           "all_ms": [round(x, 3) for x in ms]}
    out.update(more)
    print(json.dumps(out), flush=True)


def main():
    mode = sys.argv[1]
    step = int(sys.argv[2]) if len(sys.argv) > 2 else 63
    label = sys.argv[3] if len(sys.argv) > 3 else ""
    scene, _ = rtamd.make_scene("random_book_one", rtamd.randGen(1024))
    cam = rtamd.camera("random_scene", W, H)
    p = rtamd.make_params(W, H, SPP, DEPTH, rtamd.RT_RNG_PHILOX, seed=1024)
    ctx = rtamd.Context(0)
    ctx.upload(scene)
    ms, kernel = [], []
    if mode == "render":
        for i in range(WARMUP + REPS):
            t0 = time.perf_counter()
            ctx.render(cam, p)
            t = (time.perf_counter() - t0) * 1e3
            if i >= WARMUP:
                ms.append(t)
                kernel.append(ctx.frame_timing()["kernel_ms"][0])
        summary(f"{label}rt_render (wall)", ms, kernel_ms_median=statistics.median(kernel))
    elif mode in ("frame", "tracked"):
        launches = 0
        for i in range(WARMUP + REPS):
            t0 = time.perf_counter()
            fr = ctx.open_frame(cam, p, moments=True) if mode == "tracked" else ctx.open_frame(cam, p)
            launches = 0
            while not fr.complete:
                fr.advance(step)
                launches += 1
            _, _, st = fr.resolve(linear=False)
            fr.close()
            t = (time.perf_counter() - t0) * 1e3
            if i >= WARMUP:
                ms.append(t)
                kernel.append(st["kernel_ms"])
        kind = "tracked frame" if mode == "tracked" else "frame"
        summary(f"{label}{kind}, steps of {step} chunks + 1 resolve (wall, open and close included)", ms,
                kernel_ms_median=statistics.median(kernel), launches=launches)
    elif mode == "error":
        with ctx.open_frame(cam, p, moments=True) as fr:
            fr.advance(1000)
            fr.resolve(linear=False)  # (the render is drained)
            for want_map, what in [(False, "stats only"), (True, "with the map downloaded")]:
                ms = []
                for i in range(WARMUP + 2 * REPS):
                    t0 = time.perf_counter()
                    _, st = fr.error(0.01, 0.05, want_map=want_map)
                    t = (time.perf_counter() - t0) * 1e3
                    if i >= WARMUP:
                        ms.append(t)
                summary(f"one rt_frame_error, {what} (wall, render drained before)", ms, stats=st)
    else:
        raise SystemExit(f"unknown mode {mode}")
    ctx.close()


if __name__ == "__main__":
    main()
