#!/usr/bin/env python3
"""Records which tier-B launch the library makes for a table of cases, one per branch of the launch decision
(kernel form, waves, LDS staging, batches, tail, counting build, progressive and adaptive spans).

For each case: upload the world and render once at the case's size (or advance a frame, or run the counting
build) under the case's environment, then write the case, rt_last_launch() and wide_keys(). The output is
tests/golden/launch_plans.json, the record tests/test_launch_plan_host.py and tests/test_gpu_launch_plan.py
compare against. It uses the public Python API only, so it runs on any commit.

    python scripts/launch_table.py [-o tests/golden/launch_plans.json]
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "ray-tracing_amd"))

import numpy as np  # noqa: E402
import rtamd  # noqa: E402

DEPTH, SEED = 8, 11
STRESS_LADDER = (800, 1200, 1500, 2000, 3000, 5000, 20000)  # tests/test_gpu_launch_const.py


def case(name, world, camera, size=(64, 48, 4), env=None, flags=0, mode="render", param=0):
    """mode: render | frame (one advance of one chunk) | adaptive (the same after a stop call) | work."""
    w, h, spp = size
    return dict(name=name, world=world, camera=camera, param=param, width=w, height=h, spp=spp, depth=DEPTH,
                seed=SEED, flags=flags, env=dict(env or {}), mode=mode)


def cases(cu_count):
    rb = ("random_book_one", "random_scene")
    out = [
        case("three_spheres", "three_spheres", "random_scene"),
        case("random_book_one", *rb),
        case("stress_spheres", "stress_spheres", "random_scene", param=-1),  # (the ladder size, found below)
        case("cornell", "cornell", "cornell"),
        case("cornell_smoke", "cornell_smoke", "cornell"),
        case("next_week_final", "next_week_final", "next_week"),
    ]
    for k, v in (("WIDE", "0"), ("LDS", "0"), ("LEAF_LDS", "0"), ("PACKED_KEYS", "0"), ("REPLACE", "0"),
                 ("WAVES", "2")):
        out.append(case(f"random_book_one {k}={v}", *rb, env={f"RTAMD_{k}": v}))
    out.append(case("random_book_one QNODE=1 LDS=0", *rb, env={"RTAMD_QNODE": "1", "RTAMD_LDS": "0"}))
    out.append(case("random_book_one reference cull", *rb, flags=rtamd.RT_FLAG_REFERENCE_CULL))
    # the 4th-wave threshold, work_total >= cu_count * 1024, at 1 spp: 512 x 2*cu pixels reach it, 8 rows less do not
    hi = 2 * cu_count
    out.append(case("random_book_one at the 4th-wave threshold", *rb, size=(512, hi, 1)))
    out.append(case("random_book_one below the 4th-wave threshold", *rb, size=(512, hi - 8, 1)))
    out.append(case("cornell WIDE=1", "cornell", "cornell", env={"RTAMD_WIDE": "1"}))
    out.append(case("cornell_smoke TAIL=0", "cornell_smoke", "cornell", env={"RTAMD_TAIL": "0"}))
    out.append(case("random_book_one PARTIAL_CAP=1", *rb, env={"RTAMD_PARTIAL_CAP": "1"}))
    out.append(case("random_book_one frame advance", *rb, size=(512, 512, 4), mode="frame"))
    out.append(case("random_book_one adaptive advance", *rb, size=(512, 512, 4), mode="adaptive"))
    out.append(case("random_book_one counting build", *rb, mode="work"))
    out.append(case("cornell counting build", "cornell", "cornell", mode="work"))
    return out


def params_of(c):
    return rtamd.make_params(c["width"], c["height"], c["spp"], c["depth"], rtamd.RT_RNG_PHILOX, seed=c["seed"],
                             flags=c["flags"])


def scene_of(c):
    return rtamd.make_scene(c["world"], rtamd.randGen(1024), param=max(0, c["param"]))[0]


class case_env:
    """The case's RTAMD_* settings for the duration of its upload and launch."""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def launch(ctx, c):
    """Runs the case on `ctx` (upload included) and returns (rt_last_launch(), wide_keys())."""
    cam, p = rtamd.camera(c["camera"], c["width"], c["height"]), params_of(c)
    with case_env(c["env"]):
        ctx.upload(scene_of(c))
        if c["mode"] == "render":
            ctx.render(cam, p)
        elif c["mode"] == "work":
            ctx.render_work(cam, p)
        else:
            with ctx.open_frame(cam, p) as fr:
                assert fr.chunks_total >= 2, "the span cases need a frame of several chunks"
                fr.advance(1)
                if c["mode"] == "adaptive":
                    mask = np.zeros((c["height"], c["width"]), dtype=np.uint8)
                    mask[: c["height"] // 2] = 1
                    fr.stop(mask)
                    fr.advance(1)
                fr.stats()  # (drains the frame's launches)
        return ctx.last_launch(), ctx.wide_keys()


def stress_param(ctx):
    """The smallest stress_spheres size of the ladder whose 64x48 frame takes the global-memory kernel."""
    for param in STRESS_LADDER:
        c = case("stress_spheres", "stress_spheres", "random_scene", param=param)
        if launch(ctx, c)[0]["lds_staged"] == 0:
            return param
    raise SystemExit("no stress_spheres size of the ladder takes the global-memory kernel")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-o", "--out", default=os.path.join(HERE, "..", "tests", "golden", "launch_plans.json"))
    args = ap.parse_args()
    import torch
    cu_count = torch.cuda.get_device_properties(0).multi_processor_count
    ctx = rtamd.Context(0)
    rows = []
    try:
        ladder = stress_param(ctx)
        for c in cases(cu_count):
            if c["param"] < 0:
                c["param"] = ladder
            c["launch"], c["wide_keys"] = launch(ctx, c)
            print(c["name"], c["launch"], c["wide_keys"], flush=True)
            rows.append(c)
    finally:
        ctx.close()
    with open(args.out, "w") as f:
        json.dump({"cu_count": cu_count, "cases": rows}, f, indent=1)
        f.write("\n")
    print(f"wrote {len(rows)} cases to {args.out}")


if __name__ == "__main__":
    main()
