"""What the sharded feature passes cost, on ONE GPU: config 2 (1200x800, 500 samples) and config 4's
scene (800x800, 100 samples), first-hit pass and chain pass (8 bounces, both materials).

  unsharded   the image-order pass (rt_render_features_async, rt_render_features_chain_async) alternating with the
              one-shard slab pass (rt_render_features_shard_async, shard_count 1) in one process: what slab-order
              stores are worth, and the figure to compare with another commit's run of this script (--unsharded-only
              runs on a commit without the slab entries).
  shards      every shard r of N in turn, N in 1, 2, 4, 8: the slowest shard's time x N over the one-shard slab pass
              is the N-device pass's efficiency per shard ("of ideal"), a one-GPU prediction as shard_probe.py's.
  merge       rt_assemble_records_async over config 2's 8 slabs of records next to rt_assemble_linear_async over its
              8 linear slabs (64 against 24 bytes per pixel).

Legs alternate in one process, one warm-up then five legs each, timed by device events on one stream around the
queued launches; minimum and spread. One JSON line per measurement on stdout.

    python scripts/features_shard_probe.py [c2] [c4] [--unsharded-only] [--tile 16]
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
SHARDS = (1, 2, 4, 8)


def timed(st, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(st)
    fn()
    b.record(st)
    b.synchronize()
    return a.elapsed_time(b)


def summary(ms):
    return {"min_ms": round(min(ms), 3), "spread_ms": round(max(ms) - min(ms), 3), "all_ms": [round(x, 3) for x in ms]}


def alternate(st, fns):
    """One warm-up of every leg, then LEGS rounds of them in turn: {name: [ms]}."""
    legs = {k: [] for k in fns}
    for i in range(1 + LEGS):
        for k, fn in fns.items():
            ms = timed(st, fn)
            if i:
                legs[k].append(ms)
    return legs


def probe(name, tile, unsharded_only):
    cfg = CONFIGS[name]
    earth = np.load(os.path.join(ROOT, "tests", "golden", "earthmap_rgb8.npz"))["rgb"] if cfg.get("earth") else None
    scene, _ = rtamd.make_scene(cfg["scene"], rtamd.randGen(1024), earth=earth)
    W, H, spp = cfg["W"], cfg["H"], cfg["spp"]
    cam = rtamd.camera(cfg["camera"], W, H)

    def params(rank=0, shards=1):
        return rtamd.make_params(W, H, spp, 1, rtamd.RT_RNG_PHILOX, seed=1024, tile=tile, shard_rank=rank, shard_count=shards)

    ctx = rtamd.Context(0)
    ctx.upload(scene)
    chain = rtamd.make_feature_chain(8, True, True, 0.0)
    d_img = torch.zeros((H, W, 8), dtype=torch.float64, device="cuda:0")
    st = torch.cuda.Stream(device=0)
    s = st.cuda_stream
    head = {"config": name, "width": W, "height": H, "samples": spp, "tile": tile, "legs": LEGS}
    with torch.cuda.stream(st):
        p1 = params()
        fns = {"first_hit": lambda: ctx.render_features_async(cam, p1, d_img.data_ptr(), stream=s),
               "chain": lambda: ctx.render_features_async(cam, p1, d_img.data_ptr(), stream=s, chain=chain)}
        if not unsharded_only:
            d_one = torch.zeros((rtamd.shard_geometry(p1)[2], 8), dtype=torch.float64, device="cuda:0")
            fns["first_hit_slab"] = lambda: ctx.render_features_shard_async(cam, p1, d_one.data_ptr(), stream=s)
            fns["chain_slab"] = lambda: ctx.render_features_shard_async(cam, p1, d_one.data_ptr(), stream=s, chain=chain)
        legs = alternate(st, fns)
        out = dict(head, measure="unsharded", **{k: summary(v) for k, v in legs.items()})
        if not unsharded_only:
            for k in ("first_hit", "chain"):
                out[k + "_slab_over_image_order"] = round(min(legs[k + "_slab"]) / min(legs[k]), 4)
        print(json.dumps(out), flush=True)
        if unsharded_only:
            ctx.close()
            return
        one = {"first_hit": min(legs["first_hit_slab"]), "chain": min(legs["chain_slab"])}
        for n in SHARDS:
            slab = rtamd.shard_geometry(params(0, n))[2]
            d_slabs = torch.zeros((n, slab, 8), dtype=torch.float64, device="cuda:0")
            fns = {}
            for r in range(n):
                pr = params(r, n)
                fns[("first_hit", r)] = lambda pr=pr, r=r: ctx.render_features_shard_async(cam, pr, d_slabs[r].data_ptr(), stream=s)
                fns[("chain", r)] = lambda pr=pr, r=r: ctx.render_features_shard_async(cam, pr, d_slabs[r].data_ptr(), stream=s,
                                                                                    chain=chain)
            legs = alternate(st, fns)
            out = dict(head, measure="shards", shards=n)
            for k in ("first_hit", "chain"):
                per = [min(legs[(k, r)]) for r in range(n)]
                out[k] = {"slowest_shard_ms": round(max(per), 3), "mean_shard_ms": round(float(np.mean(per)), 3),
                          "spread_of_slowest_ms": round(max(max(legs[(k, r)]) - min(legs[(k, r)]) for r in range(n)), 3),
                          "shard_ms": [round(x, 3) for x in per],
                          "of_ideal": round(one[k] / (max(per) * n), 4)}
            print(json.dumps(out), flush=True)
            if name == "c2" and n == SHARDS[-1]:
                d_lin = torch.zeros((n, slab, 3), dtype=torch.float64, device="cuda:0")
                d_lin_img = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")
                pn = params(0, n)
                legs = alternate(st, {
                    "assemble_records": lambda: ctx.assemble_records_async(pn, d_slabs.data_ptr(), d_img.data_ptr(), stream=s),
                    "assemble_linear": lambda: ctx.assemble_linear_async(pn, d_lin.data_ptr(), d_lin_img.data_ptr(), stream=s)})
                out = dict(head, measure="merge", shards=n, **{k: summary(v) for k, v in legs.items()})
                out["records_over_linear"] = round(min(legs["assemble_records"]) / min(legs["assemble_linear"]), 3)
                out["bytes_ratio"] = round(64 / 24, 3)
                out["records_gb_per_s"] = round(2 * 64 * W * H / (min(legs["assemble_records"]) * 1e-3) / 1e9, 1)
                print(json.dumps(out), flush=True)
    ctx.close()


if __name__ == "__main__":
    args = sys.argv[1:]
    only = "--unsharded-only" in args
    tile = int(args[args.index("--tile") + 1]) if "--tile" in args else 16
    names = [a for a in args if a in CONFIGS] or ["c2", "c4"]
    for name in names:
        probe(name, tile, only)
