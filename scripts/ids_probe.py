"""What a material-ID pass costs next to the feature passes of the same frame.

Config 2 (1200x800, 500 samples) and config 4's scene (800x800) at 100 samples. Legs alternate in one process, one
warm-up round and then five rounds, each timed by device events on one stream: the id pass without a chain and at
max_bounces 8, the first-hit and chain (8) feature passes, and the chain feature pass at max_bounces 0 (the id pass
without a chain runs that kernel form); on config 2 also the id pass without a chain at
RTAMD_WAVES=4, the staged kernel that spills, at the first-hit feature pass's block size. Minimum, spread and every
leg, what each launch ran, the chain's counts, and how many pixels overflowed their seven slots.

    python scripts/ids_probe.py [c2] [c4]      (one JSON line each on stdout)
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(os.path.join(ROOT, "ray-tracing_amd"))  # (after PYTHONPATH: another commit's package goes there)

import rtamd  # noqa: E402

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


def cost(name):
    cfg = CONFIGS[name]
    earth = np.load(os.path.join(ROOT, "tests", "golden", "earthmap_rgb8.npz"))["rgb"] if cfg.get("earth") else None
    scene, _ = rtamd.make_scene(cfg["scene"], rtamd.randGen(1024), earth=earth)
    W, H, spp = cfg["W"], cfg["H"], cfg["spp"]
    cam = rtamd.camera(cfg["camera"], W, H)
    p = rtamd.make_params(W, H, spp, 1, rtamd.RT_RNG_PHILOX, seed=1024)
    ctx = rtamd.Context(0)
    ctx.upload(scene)
    d_sums = torch.zeros((H, W, rtamd.RT_FEATURE_DOUBLES), dtype=torch.float64, device="cuda:0")
    d_recs = {k: torch.zeros((H, W, 64), dtype=torch.uint8, device="cuda:0") for k in ("ids_first_hit", "ids_chain_8")}
    st = torch.cuda.Stream(device=0)
    chain8, chain0 = rtamd.make_feature_chain(8), rtamd.make_feature_chain(0)
    legs, launches, counts = {}, {}, {}

    def leg(key, fn, chain):
        legs.setdefault(key, []).append(timed(st, fn))
        launches[key] = {k: ctx.last_feature_launch()[k] for k in LAUNCH_KEYS}
        if chain:
            counts[key] = ctx.last_feature_chain()

    with torch.cuda.stream(st):
        for i in range(1 + LEGS):
            leg("ids_first_hit", lambda: ctx.render_ids_async(cam, p, d_recs["ids_first_hit"].data_ptr(),
                                                              stream=st.cuda_stream), False)
            leg("features_first_hit", lambda: ctx.render_features_async(cam, p, d_sums.data_ptr(), stream=st.cuda_stream),
                False)
            leg("ids_chain_8", lambda: ctx.render_ids_async(cam, p, d_recs["ids_chain_8"].data_ptr(), chain=chain8,
                                                            stream=st.cuda_stream), True)
            leg("features_chain_8", lambda: ctx.render_features_async(cam, p, d_sums.data_ptr(), stream=st.cuda_stream,
                                                                      chain=chain8), True)
            leg("features_chain_0", lambda: ctx.render_features_async(cam, p, d_sums.data_ptr(), stream=st.cuda_stream,
                                                                      chain=chain0), True)
            if name == "c2":
                def waves4():
                    os.environ["RTAMD_WAVES"] = "4"
                    ctx.render_ids_async(cam, p, d_recs["ids_first_hit"].data_ptr(), stream=st.cuda_stream)
                    os.environ.pop("RTAMD_WAVES", None)
                leg("ids_first_hit_waves4", waves4, False)
            if i == 0:  # (the first round warms everything up)
                legs.clear()
    out = {"config": name, "width": W, "height": H, "samples": spp, "legs": LEGS}
    for k, ms in legs.items():
        out[k] = {"min_ms": round(min(ms), 3), "spread_ms": round(max(ms) - min(ms), 3), "all_ms": [round(x, 3) for x in ms],
                  "launch": launches[k]}
        if k in counts:
            out[k]["counts"] = counts[k]
    for a, b in (("ids_first_hit", "features_first_hit"), ("ids_chain_8", "features_chain_8")):
        out[a]["over_features"] = round(out[a]["min_ms"] / out[b]["min_ms"], 4)
    out["ids_first_hit"]["over_features_chain_0"] = round(out["ids_first_hit"]["min_ms"] / out["features_chain_0"]["min_ms"], 4)
    for k, d in d_recs.items():
        recs = d.cpu().numpy().reshape(H, W, 64).view(rtamd.ID_DTYPE).reshape(H, W)
        out[k]["pixels_with_other"] = int((recs["other"] > 0).sum())
        out[k]["samples_in_other"] = int(recs["other"].sum(dtype=np.int64))
        out[k]["samples_ok"] = bool((recs["samples"] == spp).all())
    print(json.dumps(out), flush=True)
    ctx.close()


if __name__ == "__main__":
    for name in (sys.argv[1:] or ["c2", "c4"]):
        cost(name)
