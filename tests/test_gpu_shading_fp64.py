"""The packed spheres unit's fused sincos (RT_FUSED_SINCOS: rt_device.h) against the plain sin and cos, on the device:
OCML's sincos gives the bits of its sin and of its cos, and images rendered by the packed unit (one sincos call per
scatter) equal the spheres unit's (cos, then sin; RTAMD_WIDE=0), bytes and fp64 linear averages."""
import math

import numpy as np
import pytest

import rtamd

pytestmark = pytest.mark.gpu

N = 1 << 20


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(a, b):
    return (_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))


def _make(rng, n, elo, ehi):
    """Random sign and mantissa, biased exponent uniform in [elo, ehi]."""
    e = rng.integers(elo, ehi + 1, n, dtype=np.int64)
    m = rng.integers(0, 2 ** 52, n, dtype=np.int64)
    s = rng.integers(0, 2, n, dtype=np.int64) << 63
    return ((e << 52) | m | s).view(np.float64)


def _angles(rng):
    """The production domain 2 pi a, a = word_to_draw(random word) (rt_device.h), its ends, neighbours of multiples
    of pi / 4, and a sweep of large, negative, zero, infinite and NaN arguments."""
    w = rng.integers(0, 2 ** 64, N, dtype=np.uint64)
    w[:3] = [0, 2 ** 64 - 1, 2 ** 64 - 2048]  # a = 1, a = 0 and a = 2^-53, the smallest nonzero draw
    a = 1.0 - w.astype(np.float64) / 18446744073709551616.0
    assert a[0] == 1.0 and a[1] == 0.0 and a[2] == 2.0 ** -53
    prod = 2.0 * math.pi * a
    m = np.arange(-64, 65, dtype=np.float64) * (math.pi / 4)
    near = (_bits(m)[:, None] + np.arange(-8, 9)[None, :]).view(np.float64).reshape(-1)
    big = np.concatenate([rng.uniform(-1e6, 1e6, 1 << 14), 10.0 ** rng.uniform(0, 300, 1 << 14) * rng.choice([-1, 1], 1 << 14),
                          10.0 ** rng.uniform(-320, 0, 1 << 14), _make(rng, 1 << 14, 0, 2047)])
    odd = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, -5e-324, 2.0 ** -27, 2.0 ** 30, 2.0 ** 31, 1.7e308, -1.7e308])
    return np.concatenate([prod, near, big, odd])


@pytest.mark.parametrize("half,plain", [("sincos_sin", "sin"), ("sincos_cos", "cos")])
def test_sincos_halves_are_sin_and_cos(gpu_ctx, half, plain):
    x = _angles(np.random.default_rng(34))
    ref = gpu_ctx.math(plain, x)
    got = gpu_ctx.math(half, x)
    bad = ~_same(got, ref)
    assert not bad.any(), (f"{int(bad.sum())} of {x.size} differ, e.g. x = {[v.hex() for v in x[bad][:3]]}: "
                           f"got {got[bad][:3].tolist()} want {ref[bad][:3].tolist()}")


@pytest.mark.parametrize("world,w,h,spp,depth", [("random_book_one", 96, 64, 16, 50), ("three_spheres", 64, 32, 10, 50)])
def test_packed_unit_image_equals_plain_unit(gpu_ctx, monkeypatch, world, w, h, spp, depth):
    """The default launch (the packed spheres unit: fused sincos) against RTAMD_WIDE=0 (the
    spheres unit's binary walk, cos and then sin): the same bytes and the same fp64 averages, from different kernels.
    (three_spheres, below the 16 leaves from which a world's default launch is the 4-wide walk, would run the
    spheres unit's kernel both times: its first launch asks for the packed unit's with RTAMD_WIDE=1.)"""
    sc = rtamd.make_scene(world, rtamd.randGen(1024))[0]
    cam = rtamd.camera("random_scene", w, h)
    p = rtamd.make_params(w, h, spp, depth, rtamd.RT_RNG_PHILOX, seed=1024)
    gpu_ctx.upload(sc)
    monkeypatch.delenv("RTAMD_WIDE", raising=False)
    if world == "three_spheres":
        monkeypatch.setenv("RTAMD_WIDE", "1")
    new = gpu_ctx.render(cam, p, linear=True)[:2]
    launch_new, keys = gpu_ctx.last_launch(), gpu_ctx.wide_keys()
    monkeypatch.setenv("RTAMD_WIDE", "0")
    old = gpu_ctx.render(cam, p, linear=True)[:2]
    launch_old = gpu_ctx.last_launch()
    print(world, launch_new, keys, launch_old)
    assert launch_new["loop"] == 2 and launch_new["lds_staged"] == 1 and keys["packed"] == 1, "not the packed unit's kernel"
    assert launch_old["loop"] == 1, "not the spheres unit's binary-walk kernel"
    assert np.array_equal(new[0], old[0]), "bytes differ"
    assert np.array_equal(new[1], old[1], equal_nan=True), "linear averages differ"
