"""What a specular-chain feature pass costs and what its guides buy the denoiser.

Cost: config 2 (1200x800, 500 samples) and config 4's scene (800x800) at 100 samples. Legs alternate in one
process, one warm-up round and then five rounds, each timed by device events on one stream: the unchanged first-hit
pass, the chain pass at max_bounces 0, 4 and 8 (on config 2 also 8 at RTAMD_WAVES=4, the staged kernel that spills),
and rt_render at max_depth = max_bounces + 1 (the same walks plus diffuse scatters and the chunk sums). Minimum,
spread and every leg, what each launch ran, and the chain's counts (ended_cap / samples: the evidence for the
Python default of 8).

Quality: a 96x64 frame, a glass and a fuzz-0 mirror sphere over a checker floor, 40 samples of a tracked frame with
its own error map, default denoise parameters with RT_DENOISE_DEMODULATE, renders with RT_FLAG_NAN_ZERO: RMSE against
a 2000-sample render of another seed of the raw image, of the image denoised with first-hit guides and with chain
guides, over the whole frame and over the pixels whose first hit is followed in at least half of the samples.

    python scripts/features_chain_probe.py [c2] [c4] [quality]      (one JSON line each on stdout)
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
BOUNCES = (0, 4, 8)
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
    slab = rtamd.shard_geometry(p)[2]
    d_rgb = torch.zeros(slab * 3, dtype=torch.uint8, device="cuda:0")
    d_sums = torch.zeros((H, W, rtamd.RT_FEATURE_DOUBLES), dtype=torch.float64, device="cuda:0")
    st = torch.cuda.Stream(device=0)
    legs, launches, counts = {}, {}, {}

    def features(key, chain, waves=None):
        def run():
            if waves:
                os.environ["RTAMD_WAVES"] = waves
            ctx.render_features_async(cam, p, d_sums.data_ptr(), stream=st.cuda_stream, chain=chain)
            os.environ.pop("RTAMD_WAVES", None)
        legs.setdefault(key, []).append(timed(st, run))
        launches[key] = {k: ctx.last_feature_launch()[k] for k in LAUNCH_KEYS}
        if chain is not None:
            counts[key] = ctx.last_feature_chain()

    def render(key, depth):
        pd = rtamd.make_params(W, H, spp, depth, rtamd.RT_RNG_PHILOX, seed=1024)
        legs.setdefault(key, []).append(timed(st, lambda: ctx.render_shard_async(cam, pd, d_rgb.data_ptr(),
                                                                                   stream=st.cuda_stream)))
        launches[key] = {k: ctx.last_launch()[k] for k in LAUNCH_KEYS}

    with torch.cuda.stream(st):
        for i in range(1 + LEGS):
            features("first_hit", None)
            for mb in BOUNCES:
                features(f"chain_{mb}", rtamd.make_feature_chain(mb))
                render(f"render_depth{mb + 1}", mb + 1)
            if name == "c2":
                features("chain_8_waves4", rtamd.make_feature_chain(8), waves="4")
            if i == 0:  # (the first round warms everything up)
                legs.clear()
    out = {"config": name, "width": W, "height": H, "samples": spp, "legs": LEGS}
    for k, ms in legs.items():
        out[k] = {"min_ms": round(min(ms), 3), "spread_ms": round(max(ms) - min(ms), 3), "all_ms": [round(x, 3) for x in ms],
                  "launch": launches[k]}
        if k in counts:
            c = counts[k]
            out[k]["counts"] = c
            out[k]["capped_fraction"] = round(c["ended_cap"] / c["samples"], 6)
            out[k]["bounces_per_sample"] = round(c["bounces"] / c["samples"], 4)
    for mb in BOUNCES:
        out[f"chain_{mb}"]["over_render"] = round(out[f"chain_{mb}"]["min_ms"] / out[f"render_depth{mb + 1}"]["min_ms"], 4)
        out[f"chain_{mb}"]["over_first_hit"] = round(out[f"chain_{mb}"]["min_ms"] / out["first_hit"]["min_ms"], 4)
    out["finite"] = bool(np.isfinite(d_sums.cpu().numpy()).all())
    print(json.dumps(out), flush=True)
    ctx.close()


def quality_world():
    """A glass sphere and a fuzz-0 mirror sphere over a checker floor, small diffuse spheres behind and between."""
    b = rtamd.Builder(rtamd.randGen(3))
    floor = b.lambertian(b.checkerTexture(b.constantColor(0.2, 0.3, 0.1), b.constantColor(0.9, 0.9, 0.9)))
    items = [b.sphere((0.0, -1000.0, 0.0), 1000.0, floor),
             b.sphere((-1.3, 1.0, 0.0), 1.0, b.dielectric(1.5)),
             b.sphere((1.3, 1.0, 0.0), 1.0, b.metal(b.constantColor(0.8, 0.8, 0.9), 0.0))]
    for i in range(14):
        col = b.constantColor(0.2 + 0.05 * i, 0.8 - 0.04 * i, 0.3 + 0.03 * (i % 5))
        items.append(b.sphere((-3.9 + 0.6 * i, 0.3, 2.0 + 0.9 * (i % 3)), 0.3, b.lambertian(col)))
    scene = b.finish(b.makeBVH((0.0, 1.0), items), -1, (0.7, 0.8, 1.0))
    cam = rtamd.newCamera((0.0, 2.0, -7.0), (0.0, 0.8, 0.0), (0.0, 1.0, 0.0), 35.0, 1.5, 0.0, 7.0, 0.0, 1.0)
    return scene, cam


def quality():
    sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
    import feature_chain_ref as fcr
    W, H, spp, depth = 96, 64, 40, 10
    scene, cam = quality_world()
    ctx = rtamd.Context(0)
    ctx.upload(scene)
    # (RT_FLAG_NAN_ZERO on both: the world has no emitter, and without the flag the Lambertian mixture's NaN samples
    # leave 62 % of the pixels of the 2000-sample render non-finite, which the denoiser never taps)
    nz = rtamd.RT_FLAG_NAN_ZERO
    p = rtamd.make_params(W, H, spp, depth, rtamd.RT_RNG_PHILOX, seed=77, flags=nz)
    ref = ctx.render(cam, rtamd.make_params(W, H, 2000, depth, rtamd.RT_RNG_PHILOX, seed=5, flags=nz), linear=True)[1]
    first = ctx.render_features(cam, p, n_samples=spp)
    chain = ctx.render_features(cam, p, n_samples=spp, chain=rtamd.make_feature_chain())
    counts = ctx.last_feature_chain()
    with ctx.open_frame(cam, p, moments=True) as fr:
        fr.advance(fr.chunks_total)
        raw = fr.resolve()[1]
        den_first = fr.denoise(first, spp, flags=rtamd.RT_DENOISE_DEMODULATE)[1]
        den_chain = fr.denoise(chain, spp, flags=rtamd.RT_DENOISE_DEMODULATE)[1]
    # the mask, from the CPU composition at max_bounces 0: a capped sample is one whose first hit is followed
    comp = fcr.Chain(scene, cam, W, H, 77, 0, spp, 0, 3, 0.0)
    mask = (comp.kind == fcr.CAP).mean(axis=0) >= 0.5
    ok = np.isfinite(ref).all(-1) & np.isfinite(raw).all(-1) & np.isfinite(den_first).all(-1) & np.isfinite(den_chain).all(-1)
    rmse = lambda a, m: round(float(np.sqrt(((a - ref)[m] ** 2).mean())), 6)
    out = {"quality": f"{W}x{H} at {spp} samples against 2000 samples of another seed", "finite_fraction": round(float(ok.mean()), 4),
           "mask_fraction": round(float(mask.mean()), 4), "chain_counts": counts}
    for key, m in (("whole_frame", ok), ("followed_first_hit_mask", ok & mask)):
        out[key] = {"rmse_raw": rmse(raw, m), "rmse_denoised_first_hit_guides": rmse(den_first, m),
                    "rmse_denoised_chain_guides": rmse(den_chain, m)}
    print(json.dumps(out), flush=True)
    ctx.close()


if __name__ == "__main__":
    for name in (sys.argv[1:] or ["c2", "c4", "quality"]):
        quality() if name == "quality" else cost(name)
