"""What a denoise costs next to its yardstick: a 5-iteration rt_denoise_async of 1200x800 and of
3840x2160 against a device-to-device copy of the bytes its iterations must move. An iteration reads a pixel's
guide record (32 B) and (colour, V) record (32 B) and writes one record (32 B): 96 B per pixel, the traffic of a copy
of 48 B per pixel (48 read, 48 written); the yardstick is `iterations` such copies. Both run in one process on one
stream, alternating: one warm-up each, then five legs each, timed by device events around the queued work. No time
is asserted. The 1200x800 result is also compared with rt_denoise_host bit for bit. One JSON line per size on
stdout.

    python scripts/denoise_probe.py [1200x800] [3840x2160]
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(os.path.join(ROOT, "ray-tracing_amd"))  # (after PYTHONPATH: another commit's package goes there)

import rtamd  # noqa: E402

LEGS = 5
ITERATIONS = 5
N = 8  # feature samples
CHECK_PIXELS = 1200 * 800  # sizes up to this are compared with the host function


def timed(st, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(st)
    fn()
    b.record(st)
    b.synchronize()
    return a.elapsed_time(b)


def inputs(W, H, seed):
    """Seeded device inputs of a plausible frame: noisy colour around a smooth image, an se map, feature sums with
    three planes of constant normal and slowly varying depth, some NaN pixels."""
    g = torch.Generator(device="cuda:0").manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64, device="cuda:0")
    y, x = torch.meshgrid(torch.arange(H, device="cuda:0", dtype=torch.float64) / H,
                          torch.arange(W, device="cuda:0", dtype=torch.float64) / W, indexing="ij")
    smooth = torch.stack([0.2 + 0.6 * x, 0.2 + 0.6 * y, 0.5 + 0.3 * x * y], -1)
    se = 0.02 + 0.08 * rnd(H, W, 3)
    color = smooth + se * (rnd(H, W, 3) - 0.5) * 3.46
    color[rnd(H, W) < 0.01] = float("nan")
    feat = torch.zeros((H, W, 8), dtype=torch.float64, device="cuda:0")
    feat[..., 0:3] = N * (0.3 + 0.5 * smooth)
    plane = (3 * x).floor().long().clamp(0, 2)
    feat[..., 3:6] = N * torch.nn.functional.one_hot(plane, 3).to(torch.float64)
    feat[..., 6] = N * (2.0 + x + 0.5 * y)
    feat[..., 7] = N
    return color.contiguous(), se.contiguous(), feat.contiguous()


def probe(W, H):
    ctx = rtamd.Context(0)
    color, se, feat = inputs(W, H, seed=W + H)
    out = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")
    rgb = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda:0")
    p = rtamd.make_denoise_params(W, H, N, iterations=ITERATIONS, flags=rtamd.RT_DENOISE_DEMODULATE)
    src = torch.zeros(W * H * 48, dtype=torch.uint8, device="cuda:0")
    dst = torch.zeros_like(src)
    st = torch.cuda.Stream(device=0)
    legs = {"denoise": [], "copies": []}

    def denoise():
        ctx.denoise_async(p, color.data_ptr(), se.data_ptr(), feat.data_ptr(), out.data_ptr(), rgb.data_ptr(),
                          stream=st.cuda_stream)

    def copies():
        for _ in range(ITERATIONS):
            dst.copy_(src)

    with torch.cuda.stream(st):
        for i in range(1 + LEGS):
            d, c = timed(st, denoise), timed(st, copies)
            if i:  # (the first pair warms both up)
                legs["denoise"].append(d)
                legs["copies"].append(c)
    res = {"width": W, "height": H, "iterations": ITERATIONS, "legs": LEGS, "flags": int(p.flags),
           "bytes_per_iteration": W * H * 96}
    for k, ms in legs.items():
        res[k] = {"min_ms": round(min(ms), 4), "spread_ms": round(max(ms) - min(ms), 4), "all_ms": [round(x, 4) for x in ms]}
    res["denoise_over_copies"] = round(min(legs["denoise"]) / min(legs["copies"]), 3)
    res["copy_GBps"] = round(ITERATIONS * W * H * 96 / (min(legs["copies"]) * 1e-3) / 1e9, 1)
    res["last_denoise"] = ctx.last_denoise()
    got = out.cpu().numpy()
    res["finite_out"] = round(float(np.isfinite(got).all(-1).mean()), 4)
    if W * H <= CHECK_PIXELS:
        want = rtamd.denoise_host(p, color.cpu().numpy(), se.cpu().numpy(), feat.cpu().numpy())
        res["equals_host_bits"] = bool(np.array_equal(got.view(np.uint64), want[1].view(np.uint64))
                                       and np.array_equal(rgb.cpu().numpy(), want[0]))
    print(json.dumps(res), flush=True)
    ctx.close()


if __name__ == "__main__":
    for size in (sys.argv[1:] or ["1200x800", "3840x2160"]):
        w, h = size.split("x")
        probe(int(w), int(h))
