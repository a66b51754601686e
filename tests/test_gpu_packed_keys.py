"""The 4-wide walk's packed sort keys (wide_node<F, true>, include/rt_wide.h) and the spheres-only kernels' fp32
ray set-up from the direction itself (set_ray32<true>): closest hits bit for bit against the oracle on a world
built to produce equal and nearly equal child entry distances, and 4-wide images equal to the binary walk's on
both sides of the LDS-staging threshold (the packed form below it, the key / reference pairs above)."""
import numpy as np
import pytest

import pyoracle
import rtamd

pytestmark = pytest.mark.gpu

W, H = 64, 48
LADDER = (800, 1200, 1500, 2000, 3000, 5000, 20000)  # tests/test_gpu_launch_const.py's stress_spheres sizes
COLS = [0, 1, 2, 3, 4, 5, 6, 7, 10, 11]              # hit, t, p, normal, front face, material


def _lattice_world():
    """6 x 6 x 6 equal spheres on a regular lattice (many children of a node are entered at equal or nearly equal
    distances: exact ties and ties in the truncated keys) over one huge ground sphere."""
    b = rtamd.Builder(rtamd.randGen(7))
    mat = b.lambertian(b.constantColor(0.4, 0.5, 0.6))
    centers = np.array([(x, y, z) for x in range(6) for y in range(6) for z in range(6)], dtype=np.float64)
    ids = [b.sphere(tuple(c), 0.375, mat) for c in centers]
    ids.append(b.sphere((2.5, -1000.5, 2.5), 1000.0, b.lambertian(b.constantColor(0.5, 0.5, 0.5))))
    return b.finish(b.makeBVH((0.0, 1.0), ids), -1, (0.7, 0.8, 0.9)), centers, 0.375


def _rays(centers, rad, rng):
    """4096 rays, 512 of each kind; returns (rays, slice of the NaN-direction rays)."""
    n = 512
    unit = np.eye(3)

    def toward(o):  # a direction from o towards a random lattice point, jittered
        return centers[rng.integers(0, len(centers), len(o))] + rng.normal(0, 0.3, o.shape) - o

    def outside(m):
        return np.array([2.5, 2.5, 2.5]) + rng.normal(0, 1, (m, 3)) * 6.0

    def on_surface(m):  # points on sphere surfaces (exactly on a box plane where the offset is axis-aligned)
        k = rng.integers(0, len(centers), m)
        return centers[k] + rad * unit[rng.integers(0, 3, m)] * rng.choice([-1.0, 1.0], (m, 1))

    kinds = []
    o = outside(n)
    kinds.append((o, toward(o)))                                                       # random
    o = np.concatenate([outside(n // 2), on_surface(n // 2)])
    d = unit[rng.integers(0, 3, n)] * rng.choice([-1.0, 1.0], (n, 1))
    d[n // 2:] = np.array([1.0, 0.0, 0.0])                                             # (1,0,0) from sphere surfaces
    kinds.append((o, d))                                                               # axis-aligned
    o = on_surface(n)
    o[:, 1] += rng.choice([0.0, 1.0, -2.0], n)                                         # (still on a box plane of a row)
    kinds.append((o, toward(o)))                                                       # origins on box planes
    o = outside(n)
    d = toward(o)
    d[np.arange(n), rng.integers(0, 3, n)] = rng.choice([0.0, -0.0], n)                # one zero component
    two = np.arange(n) >= n // 2
    ax = rng.integers(0, 3, n)
    d[two] = unit[ax[two]] * rng.choice([-1.0, 1.0, 0.5, -3.0], (int(two.sum()), 1))   # two zero components
    d[two] *= rng.choice([-1.0, 1.0], (int(two.sum()), 3))                             # (zeros of both signs)
    kinds.append((o, d))
    for scale in (1e-30, 1e30, 1e-300):                                                # 1e-300: beyond fp32, `bad`
        o = outside(n)
        kinds.append((o, toward(o) * scale))
    o = outside(n)
    d = toward(o)
    d[np.arange(n), rng.integers(0, 3, n)] = np.nan                                    # hits nothing
    kinds.append((o, d))
    o = np.concatenate([k[0] for k in kinds])
    d = np.concatenate([k[1] for k in kinds])
    rays = np.concatenate([o, d, rng.uniform(0, 1, (len(o), 1))], axis=1)
    return rays, slice(7 * n, 8 * n)


def test_closest_hits_packed_lattice(gpu_ctx):
    """The packed-key walk finds the oracle's hits, bit for bit, where sort keys tie."""
    sc, centers, rad = _lattice_world()
    rays, nan_rows = _rays(centers, rad, np.random.default_rng(23))
    assert len(rays) == 4096
    gpu_ctx.upload(sc)
    got = gpu_ctx.closest_hits(rays, 1e-4, np.inf, seed=3, flags=rtamd.RT_DEBUG_WIDE)
    wk = gpu_ctx.wide_keys()
    assert wk["fits"] == 1 and wk["packed"] == 1, wk
    ref = pyoracle.closest_hits(sc, rays, 1e-4, np.inf, seed=3)
    hits = got[:, 0].reshape(8, -1).sum(axis=1)
    print("hits per ray kind:", hits.astype(int).tolist())
    assert got[:, 0].sum() > len(rays) // 8
    assert hits[0] > 0 and hits[1] > 0 and hits[2] > 0 and hits[3] > 0 and hits[4] > 0  # (each kind is exercised)
    assert not got[nan_rows, 0].any(), "a ray with a NaN direction hit something"
    bad = ~np.all(got[:, COLS] == ref[:, COLS], axis=1)
    assert not bad.any(), f"{int(bad.sum())} of {len(rays)} rays differ, first {np.flatnonzero(bad)[:8].tolist()}"


_images = {}


def _wide_and_binary(ctx, sc, monkeypatch):
    """(4-wide image, its launch, its sort form, binary-walk image) at 64x48, 4 spp, depth 50, seed 5."""
    cam = rtamd.camera("random_scene", W, H)
    p = rtamd.make_params(W, H, 4, 50, rtamd.RT_RNG_PHILOX, seed=5)
    ctx.upload(sc)
    monkeypatch.setenv("RTAMD_WIDE", "1")
    wide = ctx.render(cam, p, linear=True)[:2]
    launch, keys = ctx.last_launch(), ctx.wide_keys()
    monkeypatch.setenv("RTAMD_WIDE", "0")
    binary = ctx.render(cam, p, linear=True)[:2]
    assert ctx.last_launch()["loop"] == 1
    return wide, launch, keys, binary


def _stress_pair(ctx, monkeypatch):
    """The ladder's largest stress_spheres world whose 4-wide tree is still LDS-staged and the first that is not
    (found once: one 4-wide launch per size up to the threshold)."""
    if "pair" not in _images:
        cam = rtamd.camera("random_scene", W, H)
        p = rtamd.make_params(W, H, 4, 50, rtamd.RT_RNG_PHILOX, seed=5)
        monkeypatch.setenv("RTAMD_WIDE", "1")
        staged = None
        for param in LADDER:
            sc = rtamd.make_scene("stress_spheres", rtamd.randGen(1024), param=param)[0]
            ctx.upload(sc)
            ctx.render(cam, p)
            if ctx.last_launch()["lds_staged"] == 0:
                _images["pair"] = (staged, sc)
                break
            staged = sc
        monkeypatch.delenv("RTAMD_WIDE")
    assert "pair" in _images and _images["pair"][0] is not None, "the ladder does not straddle the LDS threshold"
    return _images["pair"]


@pytest.mark.parametrize("world", ["random_book_one", "stress_staged", "stress_global"])
def test_wide_image_equals_binary(gpu_ctx, world, monkeypatch):
    """The 4-wide walk's image (packed keys when LDS-staged, key / reference pairs from global memory) is the
    binary walk's, bytes and linear averages."""
    if world == "random_book_one":
        sc = rtamd.make_scene(world, rtamd.randGen(1024))[0]
    else:
        sc = _stress_pair(gpu_ctx, monkeypatch)[0 if world == "stress_staged" else 1]
    wide, launch, keys, binary = _wide_and_binary(gpu_ctx, sc, monkeypatch)
    print(world, launch, keys)
    assert launch["loop"] == 2
    if world == "stress_global":
        assert launch["lds_staged"] == 0 and keys["packed"] == 0
    else:
        assert launch["lds_staged"] == 1 and keys["packed"] == 1
    assert np.array_equal(wide[0], binary[0]), "bytes differ"
    assert np.array_equal(wide[1], binary[1], equal_nan=True), "linear averages differ"


def test_lds_fit_implies_the_id_bound(gpu_ctx):
    """No LDS-staged world can exceed the packed keys' id bound: at every waves-per-SIMD value the 160 KiB
    left by the lanes' stacks (at least wide_node's 3 slots of headroom and one entry, 4 bytes each) hold fewer
    128-byte wide nodes — and 4 leaf slots per node — than a packed word's reference field addresses."""
    wk = gpu_ctx.wide_keys()
    ids = 1 << (wk["ref_bits"] - 1)  # references -ids .. ids - 1
    assert wk["lds_max_wide_nodes"] * 128 <= 160 * 1024
    for waves in (1, 2, 3, 4):
        n_max = (160 * 1024 - waves * 256 * 4 * 4) // 128
        assert n_max <= wk["lds_max_wide_nodes"]
        assert n_max <= ids and 4 * n_max <= ids
    assert 4 * wk["lds_max_wide_nodes"] <= ids
