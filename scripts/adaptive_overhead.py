"""What adaptive progressive frames cost and gain (DESIGN.md §3.7's protocol): one process per row, 2 warm-up
frames then 10 timed, host clock around calls that end in a stream synchronise, RGB8 download included, no
linear image. One JSON line per run on stdout.

    python scripts/adaptive_overhead.py render c3 [spp]   # rt_render of a bench.py config (RTAMD_LIB selects the
                                                          # library; spp: a sampled run of the big configs);
                                                          # the line carries rt_last_launch's selection
    python scripts/adaptive_overhead.py tracked           # C2, tracked frame, steps of 8 chunks, no stop calls
    python scripts/adaptive_overhead.py nan               # ... with adapt(NaN rule) after every step
    python scripts/adaptive_overhead.py both 0.002 0.02   # ... with adapt(NaN | converged) at (abs_tol, rel_tol)

The frame rows resolve once, at the end, and report per step the wall ms, the render ms (HIP events around
the step's render launches, from a stats-only resolve outside the timed window of a further frame) and the
active pixels after the step's adapt call.
"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(os.path.join(ROOT, "ray-tracing_amd"))  # (after PYTHONPATH: another commit's package goes there)

import rtamd  # noqa: E402

# bench.py's configs (its CONFIGS table; importing bench.py would parse its command line's module state)
CONFIGS = {
    "c1": dict(scene="three_spheres", camera="random_scene", W=200, H=100, spp=10, depth=10),
    "c2": dict(scene="random_book_one", camera="random_scene", W=1200, H=800, spp=500, depth=50),
    "c3": dict(scene="cornell", camera="cornell", W=600, H=600, spp=1000, depth=50),
    "c4": dict(scene="next_week_final", camera="next_week", W=800, H=800, spp=1000, depth=50, earth=True),
    "c5": dict(scene="stress_spheres", camera="random_scene", W=3840, H=2160, spp=2000, depth=50, param=100000),
}
WARMUP, REPS, STEP = 2, 10, 8


def setup(name, spp=0):
    cfg = CONFIGS[name]
    earth = None
    if cfg.get("earth"):
        earth = np.load(os.path.join(ROOT, "tests", "golden", "earthmap_rgb8.npz"))["rgb"]
    scene, _ = rtamd.make_scene(cfg["scene"], rtamd.randGen(1024), param=cfg.get("param", 0), earth=earth)
    cam = rtamd.camera(cfg["camera"], cfg["W"], cfg["H"])
    p = rtamd.make_params(cfg["W"], cfg["H"], spp or cfg["spp"], cfg["depth"], rtamd.RT_RNG_PHILOX, seed=1024)
    ctx = rtamd.Context(0)
    ctx.upload(scene)
    return ctx, cam, p


def summary(mode, ms, **more):
    out = {"mode": mode, "reps": len(ms), "median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms),
           "all_ms": [round(x, 3) for x in ms]}
    out.update(more)
    print(json.dumps(out), flush=True)


def adaptive_frame(ctx, cam, p, mode, tol, per_step_render=False):
    """One frame in steps of STEP chunks with the row's stop calls; returns (wall ms per step, active pixels per
    step, render ms per step | total render ms, final stats)."""
    fr = ctx.open_frame(cam, p, moments=True)
    walls, active, render = [], [], []
    while not fr.complete:
        t0 = time.perf_counter()
        if fr.advance(STEP) == 0:
            break
        if mode == "nan":
            fr.adapt(converged=False)
        elif mode == "both":
            fr.adapt(tol[0], tol[1], 2)
        walls.append((time.perf_counter() - t0) * 1e3)  # (tracked: the step is only queued; the frame's wall counts)
        active.append(fr.active_pixels)
        if per_step_render:
            render.append(fr.stats()["kernel_ms"])
    _, _, st = fr.resolve(linear=False)
    fr.close()
    return walls, active, render if per_step_render else st["kernel_ms"], st


def main():
    mode = sys.argv[1]
    label = os.environ.get("ROW_LABEL", "")
    if mode == "render":
        name = sys.argv[2]
        spp = int(sys.argv[3]) if len(sys.argv) > 3 else 0
        ctx, cam, p = setup(name, spp)
        ms, kernel = [], []
        for i in range(WARMUP + REPS):
            t0 = time.perf_counter()
            ctx.render(cam, p)
            t = (time.perf_counter() - t0) * 1e3
            if i >= WARMUP:
                ms.append(t)
                kernel.append(ctx.frame_timing()["kernel_ms"][0])
        ll = ctx.last_launch()
        summary(f"{label}rt_render {name} at {p.spp} spp (wall)", ms, kernel_ms_median=statistics.median(kernel),
                launch={k: ll[k] for k in ("variant", "loop", "lds_staged", "leaf_lds", "waves", "grid", "block",
                                           "dyn_lds_bytes")})
    elif mode in ("tracked", "nan", "both"):
        tol = (float(sys.argv[2]), float(sys.argv[3])) if mode == "both" else (0.0, 0.0)
        ctx, cam, p = setup("c2")
        ms, kernel, walls, active = [], [], [], []
        for i in range(WARMUP + REPS):
            t0 = time.perf_counter()
            w, a, k, st = adaptive_frame(ctx, cam, p, mode, tol)
            t = (time.perf_counter() - t0) * 1e3
            if i >= WARMUP:
                ms.append(t)
                kernel.append(k)
                walls.append(w)
                active = a
        # per-step render ms: one further frame, polled after every step (the polls drain the stream, so this
        # frame is outside the timed ones)
        _, _, step_render, st = adaptive_frame(ctx, cam, p, mode, tol, per_step_render=True)
        what = {"tracked": "no stop calls", "nan": "adapt(NaN) after every step",
                "both": f"adapt(NaN | converged, abs_tol {tol[0]}, rel_tol {tol[1]}) after every step"}[mode]
        summary(f"{label}tracked C2 frame, steps of {STEP} chunks, {what} + 1 resolve (wall, open and close included)",
                ms, kernel_ms_median=statistics.median(kernel), steps=len(active), active_pixels=active,
                step_wall_ms_median=[round(statistics.median(x), 3) for x in zip(*walls)],
                step_render_ms=[round(x, 3) for x in step_render], chunks_done=st["chunks_done"],
                nan_pixels=st["nan_pixels"])
    else:
        raise SystemExit(f"unknown mode {mode}")
    ctx.close()


if __name__ == "__main__":
    main()
