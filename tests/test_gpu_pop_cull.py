"""The stack cull of the 4-wide walk's packed form (wide_leaf<F, true>, rt_wkey_beyond in include/rt_wide.h): stacked
children whose boxes the ray enters beyond a new hit are dropped when the hit is taken. It changes no result: closest
hits bit for bit against the oracle on a world where stale stack entries are the rule, images equal to the binary
walk's and to the key / reference pairs form's (which does not cull), and less work in the counting build."""
import numpy as np
import pytest

import pyoracle
import rtamd

pytestmark = pytest.mark.gpu

W, H = 64, 48
COLS = [0, 1, 2, 3, 4, 5, 6, 7, 10, 11]  # hit, t, p, normal, front face, material
RAD = 0.375
PAIR = np.array([[10.0, 2.0, 2.0], [12.0, 2.0, 2.0]])  # two unit spheres touching at (11, 2, 2)

_cache = {}


def _lattice_world(twin=False):
    """6 x 6 x 6 equal spheres on a regular lattice over one huge ground sphere (a ray along a row hits the first
    sphere and leaves the row's other boxes on its stack), and a pair of touching unit spheres (exact ties).
    `twin`: the pair's second sphere is there twice, as two leaves, so that every ray that hits it first ties."""
    key = "twin" if twin else "world"
    if key not in _cache:
        b = rtamd.Builder(rtamd.randGen(7))
        mat = b.lambertian(b.constantColor(0.4, 0.5, 0.6))
        centers = np.array([(x, y, z) for x in range(6) for y in range(6) for z in range(6)], dtype=np.float64)
        ids = [b.sphere(tuple(c), RAD, mat) for c in centers]
        ids.append(b.sphere((2.5, -1000.5, 2.5), 1000.0, b.lambertian(b.constantColor(0.5, 0.5, 0.5))))
        ids += [b.sphere(tuple(c), 1.0, b.lambertian(b.constantColor(0.7, 0.3, 0.3))) for c in PAIR]
        if twin:
            ids.append(b.sphere(tuple(PAIR[1]), 1.0, b.lambertian(b.constantColor(0.3, 0.7, 0.3))))
        _cache[key] = (b.finish(b.makeBVH((0.0, 1.0), ids), -1, (0.7, 0.8, 0.9)), centers)
    return _cache[key]


def _rays(centers, rng):
    """4096 rays, 512 of each kind; returns (rays, names of the kinds)."""
    n = 512
    unit = np.eye(3)

    def toward(o):  # a direction from o towards a random lattice point, jittered
        return centers[rng.integers(0, len(centers), len(o))] + rng.normal(0, 0.3, o.shape) - o

    def outside(m):
        return np.array([2.5, 2.5, 2.5]) + rng.normal(0, 1, (m, 3)) * 6.0

    kinds = []
    # along lattice rows (256) and diagonals (192) from outside, both ways; the first sphere hit leaves the rest of
    # the row stacked. Then 64 rays through the touching point of the pair from inside one of the two, along the line
    # of centres with dyadic coordinates: the sphere left and the sphere entered are hit at exactly the same t.
    axis = rng.integers(0, 3, 256)
    sign = rng.choice([-1.0, 1.0], 256)
    o = rng.integers(0, 6, (256, 3)).astype(np.float64) + rng.choice([0.0, 0.0, 0.1, -0.25], (256, 3))
    o[np.arange(256), axis] = np.where(sign > 0, -4.0, 9.0)
    rows = (o, unit[axis] * sign[:, None])
    dd = np.array([(1, 1, 0), (1, 0, 1), (0, 1, 1), (1, -1, 0), (1, 1, 1), (1, -1, 1), (-1, -1, -1)], dtype=np.float64)
    d = dd[rng.integers(0, len(dd), 192)]
    p = rng.integers(0, 6, (192, 3)).astype(np.float64)  # a lattice point the diagonal passes through
    diag = (p - 7.0 * d, d)
    s = rng.choice([-0.75, -0.5, -0.25, 0.0, 0.25, 0.5, 0.75], 64)
    side = rng.choice([-1.0, 1.0], 64)  # from inside the first sphere along +x, or the second along -x
    o = np.stack([11.0 - side * (1.0 - s), np.full(64, 2.0), np.full(64, 2.0)], axis=1)
    tang = (o, np.stack([side * rng.choice([0.5, 1.0, 2.0, 4.0], 64), np.zeros(64), np.zeros(64)], axis=1))
    kinds.append(("rows, diagonals, touching point", np.concatenate([rows[0], diag[0], tang[0]]),
                  np.concatenate([rows[1], diag[1], tang[1]])))
    k = rng.integers(0, len(centers), n)                                               # on sphere surfaces (and so
    o = centers[k] + RAD * unit[rng.integers(0, 3, n)] * rng.choice([-1.0, 1.0], (n, 1))  # on a box plane), +x
    kinds.append(("from surfaces along +x", o, np.tile([1.0, 0.0, 0.0], (n, 1))))
    o = outside(n)
    d = toward(o)
    d[np.arange(n), rng.integers(0, 3, n)] = rng.choice([0.0, -0.0], n)                # one zero component
    two = np.arange(n) >= n // 2
    o[two] = rng.integers(0, 6, (int(two.sum()), 3)) + rng.normal(0, 0.1, (int(two.sum()), 3))
    ax = rng.integers(0, 3, n)
    o[two, ax[two]] = rng.choice([-5.0, 11.0], int(two.sum()))
    d[two] = unit[ax[two]] * np.where(o[two, ax[two]] < 0, 1.0, -1.0)[:, None] * rng.choice([1.0, 0.5, 3.0], (int(two.sum()), 1))
    d[two] = np.where(d[two] == 0, rng.choice([0.0, -0.0], (int(two.sum()), 3)), d[two])  # (zeros of both signs)
    kinds.append(("zero components", o, d))
    for scale in (1e-30, 1e30, 1e-300):                                                # 1e-300: beyond fp32, `bad`
        o = outside(n)
        kinds.append((f"scaled {scale:g}", o, toward(o) * scale))
    o = centers[rng.integers(0, len(centers), n)] + rng.uniform(-0.2, 0.2, (n, 3))     # inside a sphere
    kinds.append(("from inside", o, rng.normal(0, 1, (n, 3))))
    o = outside(n)
    d = toward(o)
    d[np.arange(n), rng.integers(0, 3, n)] = np.nan                                    # hits nothing
    kinds.append(("NaN direction", o, d))
    o = np.concatenate([k[1] for k in kinds])
    d = np.concatenate([k[2] for k in kinds])
    rays = np.concatenate([o, d, rng.uniform(0, 1, (len(o), 1))], axis=1)
    return rays, [k[0] for k in kinds]


def test_closest_hits_with_stale_entries(gpu_ctx):
    """The culling walk finds the oracle's hits, bit for bit, where a hit leaves stacked boxes behind it."""
    sc, centers = _lattice_world()
    rays, names = _rays(centers, np.random.default_rng(41))
    assert len(rays) == 4096 and len(names) == 8
    gpu_ctx.upload(sc)
    got = gpu_ctx.closest_hits(rays, 1e-4, np.inf, seed=3, flags=rtamd.RT_DEBUG_WIDE)
    wk = gpu_ctx.wide_keys()
    assert wk["fits"] == 1 and wk["packed"] == 1, wk
    ref = pyoracle.closest_hits(sc, rays, 1e-4, np.inf, seed=3)
    hits = got[:, 0].reshape(8, -1).sum(axis=1).astype(int)
    print("hits per ray kind:", dict(zip(names, hits.tolist())))
    # (scaled 1e30: every t is below tmin; scaled 1e-300: |d|^2 underflows; NaN: nothing may be hit)
    for k in (0, 1, 2, 3, 6):
        assert hits[k] > 0, f"ray kind '{names[k]}' is not exercised: {hits[k]} hits"
    tie_t = (11.0 - rays[448:512, 0]) / rays[448:512, 3]
    assert got[448:512, 0].all() and np.all(got[448:512, 1] == tie_t), "no exact tie at the touching point"
    assert not got[7 * 512:, 0].any(), "a ray with a NaN direction hit something"
    bad = ~np.all(got[:, COLS] == ref[:, COLS], axis=1)
    assert not bad.any(), f"{int(bad.sum())} of {len(rays)} rays differ, first {np.flatnonzero(bad)[:8].tolist()}"


def _render(ctx, monkeypatch, env):
    """(bytes, linear averages), the launch and the sort form at 64x48, 4 spp, depth 50, seed 5 under `env`."""
    cam = rtamd.camera("random_scene", W, H)
    p = rtamd.make_params(W, H, 4, 50, rtamd.RT_RNG_PHILOX, seed=5)
    for k in ("RTAMD_WIDE", "RTAMD_PACKED_KEYS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    img = ctx.render(cam, p, linear=True)[:2]
    return img, ctx.last_launch(), ctx.wide_keys()


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1], equal_nan=True)


@pytest.mark.parametrize("world", ["random_book_one", "lattice", "lattice_twin"])
def test_image_equals_binary_and_pairs(gpu_ctx, world, monkeypatch):
    """The culling walk's image is the binary walk's, bytes and linear averages; on book one (the glass sphere
    resting on the ground: exact ties) also the image of the pairs form, which does not cull. The twin world's
    image is made of tie redos (test_tie_redos_equal_on_touching_spheres counts them)."""
    sc = (rtamd.make_scene(world, rtamd.randGen(1024))[0] if world == "random_book_one"
          else _lattice_world(world == "lattice_twin")[0])
    gpu_ctx.upload(sc)
    wide, launch, keys = _render(gpu_ctx, monkeypatch, {"RTAMD_WIDE": "1"})
    print(world, launch, keys)
    assert launch["loop"] == 2 and launch["lds_staged"] == 1 and keys["packed"] == 1
    binary, launch_b, _ = _render(gpu_ctx, monkeypatch, {"RTAMD_WIDE": "0"})
    assert launch_b["loop"] == 1
    assert _same(wide, binary), "the 4-wide image differs from the binary walk's"
    if world == "random_book_one":
        pairs, launch_p, keys_p = _render(gpu_ctx, monkeypatch, {"RTAMD_WIDE": "1", "RTAMD_PACKED_KEYS": "0"})
        assert launch_p["loop"] == 2 and keys_p["packed"] == 0
        assert _same(wide, pairs), "the culling walk's image differs from the pairs form's"


def _work(ctx, monkeypatch, packed):
    cam = rtamd.camera("random_scene", W, H)
    p = rtamd.make_params(W, H, 4, 50, rtamd.RT_RNG_PHILOX, seed=5)
    monkeypatch.setenv("RTAMD_WIDE", "1")
    monkeypatch.setenv("RTAMD_PACKED_KEYS", "1" if packed else "0")
    w = ctx.render_work(cam, p)
    assert ctx.wide_keys()["packed"] == int(packed), "the counting build does not walk in the timed kernel's form"
    assert ctx.last_launch()["loop"] == 2
    return w


def test_the_work_fell(gpu_ctx, monkeypatch):
    """The counting build walks as the timed kernel does: the same samples and segments as the pairs form, fewer
    leaf tests. (Wide-node visits are reported only: the truncated sort order moves single visits either way.)"""
    gpu_ctx.upload(rtamd.make_scene("random_book_one", rtamd.randGen(1024))[0])
    cull, pairs = _work(gpu_ctx, monkeypatch, True), _work(gpu_ctx, monkeypatch, False)
    for name, w in (("packed, stack cull", cull), ("pairs", pairs)):
        print(f"{name}: wide nodes / segment {w['wide_nodes'] / w['segments']:.4f}, "
              f"leaf tests / segment {w['prim_tests'] / w['segments']:.4f}, tie redos {w['tie_redos']}")
    assert cull["samples"] == pairs["samples"] == W * H * 4
    assert cull["segments"] == pairs["segments"]
    assert cull["prim_tests"] < pairs["prim_tests"]


@pytest.mark.parametrize("twin", [False, True])
def test_tie_redos_equal_on_touching_spheres(gpu_ctx, monkeypatch, twin):
    """A tie at the closest hit is seen whether or not stale entries are culled: the same redos in both forms. The
    camera's random rays do not pass through the one touching point, so the plain world may report no redo at all;
    with the twin of the sphere that fills most of this camera's view, primary rays tie by the thousand, behind a
    stack that the lattice has filled."""
    gpu_ctx.upload(_lattice_world(twin)[0])
    cull, pairs = _work(gpu_ctx, monkeypatch, True), _work(gpu_ctx, monkeypatch, False)
    print("tie redos:", cull["tie_redos"], pairs["tie_redos"])
    assert cull["samples"] == pairs["samples"] and cull["segments"] == pairs["segments"]
    assert cull["tie_redos"] == pairs["tie_redos"]
    if twin:
        assert cull["tie_redos"] > 0, "no tie occurred: the test shows nothing about ties under the cull"
