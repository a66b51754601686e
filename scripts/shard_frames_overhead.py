"""What a shard frame's step costs on one GPU: C2 as N shard frames open on one ctx, tracked,
each advanced in steps of 8 chunks, next to the unsharded tracked frame's step / N. One process, 2 warm-up
frames then 10 timed; per-step render ms are the HIP-event times around each step's render launches (a
stats-only resolve after every step of a further, polled frame). One JSON line per row on stdout.

    python scripts/shard_frames_overhead.py [N]      # default 8

The shards share the GPU one after another, so a shard's step is the one-GPU prediction of a step on N GPUs
less everything N devices add (gather, host threads); nothing here runs on more than one device.
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(os.path.join(ROOT, "ray-tracing_amd"))
sys.path.append(os.path.join(ROOT, "scripts"))

import rtamd  # noqa: E402
from adaptive_overhead import REPS, STEP, WARMUP, setup  # noqa: E402
from rtamd.progressive import shard_params  # noqa: E402


def run_frames(frames, poll):
    """The frames to their end in steps of STEP chunks, interleaved; returns the wall ms and, with `poll`, per
    frame the render ms of each step."""
    steps = [[] for _ in frames]
    t0 = time.perf_counter()
    while not all(f.complete for f in frames):
        for i, f in enumerate(frames):
            if f.advance(STEP) and poll:
                steps[i].append(f.resolve_into()["kernel_ms"] if hasattr(f, "resolve_into") else f.stats()["kernel_ms"])
    for f in frames:  # (drains each frame's queued work)
        f.resolve_into() if hasattr(f, "resolve_into") else f.stats()
    return (time.perf_counter() - t0) * 1e3, steps


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    ctx, cam, p = setup("c2")
    rows = {"unsharded": lambda: [ctx.open_frame(cam, p, moments=True)],
            f"{n} shard frames": lambda: [ctx.open_shard_frame(cam, shard_params(p, r, n), moments=True) for r in range(n)]}
    out = {}
    for name, make in rows.items():
        walls = []
        for i in range(WARMUP + REPS):
            frames = make()
            wall, _ = run_frames(frames, False)
            for f in frames:
                f.close()
            if i >= WARMUP:
                walls.append(wall)
        frames = make()
        _, steps = run_frames(frames, True)
        for f in frames:
            f.close()
        out[name] = steps
        print(json.dumps({"mode": f"tracked C2 frame as {name} on one GPU, steps of {STEP} chunks (wall: all frames to "
                                  "their end, one stats poll each)", "reps": len(walls),
                          "median_ms": statistics.median(walls), "min_ms": min(walls), "max_ms": max(walls),
                          "step_render_ms": [[round(x, 3) for x in s] for s in steps]}), flush=True)
    whole = out["unsharded"][0]
    shard = out[f"{n} shard frames"]
    per_step = [statistics.median(s[k] for s in shard) for k in range(len(whole))]
    print(json.dumps({"mode": f"per-shard render ms per step (median over the {n} shards) next to the unsharded step / {n}",
                      "shard_step_ms": [round(x, 3) for x in per_step],
                      "slowest_shard_step_ms": [round(max(s[k] for s in shard), 3) for k in range(len(whole))],
                      "unsharded_step_over_n_ms": [round(x / n, 3) for x in whole],
                      "difference_ms": [round(a - b / n, 3) for a, b in zip(per_step, whole)]}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
