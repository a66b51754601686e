"""What a first-hit feature pass costs next to its yardstick, the same frame's rt_render at
max_depth = 1 (the same primary walks plus one scatter and the chunk sums): config 2 (1200x800, 500 samples) and
config 4's scene (800x800) at 100 samples. The two alternate in one process, one warm-up each and then five legs
each, timed by device events on one stream around the queued launches (the render's include its launch set-up
and chunk fold, into device slabs; the feature pass's its counter reset, into a device buffer). One JSON line per
config on stdout: minimum, spread and every leg, and what each launch ran.

    python scripts/features_probe.py [c2] [c4]
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(os.path.join(ROOT, "ray-tracing_amd"))  # (after PYTHONPATH: another commit's package goes there)

import rtamd  # noqa: E402

# bench.py's configs 2 and 4 (its CONFIGS table), config 4 at 100 samples
CONFIGS = {
    "c2": dict(scene="random_book_one", camera="random_scene", W=1200, H=800, spp=500),
    "c4": dict(scene="next_week_final", camera="next_week", W=800, H=800, spp=100, earth=True),
}
LEGS = 5
LAUNCH_KEYS = ("variant", "loop", "lds_staged", "leaf_lds", "waves", "grid", "block", "dyn_lds_bytes")


def timed(st, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(st)
    fn()
    b.record(st)
    b.synchronize()
    return a.elapsed_time(b)


def probe(name):
    cfg = CONFIGS[name]
    earth = np.load(os.path.join(ROOT, "tests", "golden", "earthmap_rgb8.npz"))["rgb"] if cfg.get("earth") else None
    scene, _ = rtamd.make_scene(cfg["scene"], rtamd.randGen(1024), earth=earth)
    W, H, spp = cfg["W"], cfg["H"], cfg["spp"]
    cam = rtamd.camera(cfg["camera"], W, H)
    p = rtamd.make_params(W, H, spp, 1, rtamd.RT_RNG_PHILOX, seed=1024)
    ctx = rtamd.Context(0)
    ctx.upload(scene)
    slab = rtamd.shard_geometry(p)[2]
    d_rgb = torch.zeros(slab * 3, dtype=torch.uint8, device="cuda:0")
    d_sums = torch.zeros((H, W, rtamd.RT_FEATURE_DOUBLES), dtype=torch.float64, device="cuda:0")
    st = torch.cuda.Stream(device=0)
    legs = {"features": [], "render_depth1": []}
    kernel = []
    with torch.cuda.stream(st):
        for i in range(1 + LEGS):
            f = timed(st, lambda: ctx.render_features_async(cam, p, d_sums.data_ptr(), stream=st.cuda_stream))
            r = timed(st, lambda: ctx.render_shard_async(cam, p, d_rgb.data_ptr(), stream=st.cuda_stream))
            if i:  # (the first pair warms both up)
                legs["features"].append(f)
                legs["render_depth1"].append(r)
                kernel.append(ctx.last_kernel_ms())
    out = {"config": name, "width": W, "height": H, "samples": spp, "legs": LEGS}
    for k, ms in legs.items():
        out[k] = {"min_ms": round(min(ms), 3), "spread_ms": round(max(ms) - min(ms), 3), "all_ms": [round(x, 3) for x in ms]}
    out["render_depth1"]["render_kernel_min_ms"] = round(min(kernel), 3)  # (rt_last_kernel_ms: the render kernel alone)
    out["features_over_render"] = round(min(legs["features"]) / min(legs["render_depth1"]), 4)
    fl, rl = ctx.last_feature_launch(), ctx.last_launch()
    out["features_launch"] = {k: fl[k] for k in LAUNCH_KEYS}
    out["render_launch"] = {k: rl[k] for k in LAUNCH_KEYS}
    sums = d_sums.cpu().numpy()
    out["coverage"] = round(float(sums[..., rtamd.RT_FEAT_HITS].mean() / spp), 4)
    out["finite"] = bool(np.isfinite(sums).all())
    print(json.dumps(out), flush=True)
    ctx.close()


if __name__ == "__main__":
    for name in (sys.argv[1:] or ["c2", "c4"]):
        probe(name)
