"""The packed 4-wide walk's lean step loop (rt_trace.h, kLeanWalk: lane predicates read off Trav's registers, the tie
redo run where it is set up instead of as steps of the loop, the leaf step's sweep and postpone as selects over the top
of the stack). It changes no result: closest hits bit for bit against the oracle at every occupancy target, images
equal between the packed form, the key / reference pairs form and the binary walk, the same samples and segments in
the counting build, and tie redos behind a filled stack where a world has a sphere twice."""
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
    """6 x 6 x 6 equal spheres on a regular lattice over one huge ground sphere (rays along rows fill the stack),
    and a pair of touching unit spheres (exact ties). `twin`: the pair's second sphere is there twice, as two
    leaves, so that every ray that hits it first ties and its walk is redone."""
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
    """4096 rays in 8 kinds of 512; returns (rays, names of the kinds)."""
    n = 512
    unit = np.eye(3)
    mid = np.array([2.5, 2.5, 2.5])

    def toward(o):  # from o towards a random lattice point, jittered
        return centers[rng.integers(0, len(centers), len(o))] + rng.normal(0, 0.3, o.shape) - o

    def outside(m):
        return mid + rng.normal(0, 1, (m, 3)) * 6.0

    kinds = []
    # lattice rows from outside, both ways: the first sphere hit leaves the rest of the row stacked
    axis = rng.integers(0, 3, n)
    sign = rng.choice([-1.0, 1.0], n)
    o = rng.integers(0, 6, (n, 3)).astype(np.float64) + rng.choice([0.0, 0.0, 0.1, -0.25], (n, 3))
    o[np.arange(n), axis] = np.where(sign > 0, -4.0, 9.0)
    kinds.append(("rows", o, unit[axis] * sign[:, None]))
    # diagonals through lattice points (448), and 64 rays through the pair's touching point from inside one of
    # the two, along the line of centres with dyadic coordinates: both spheres are hit at exactly the same t
    dd = np.array([(1, 1, 0), (1, 0, 1), (0, 1, 1), (1, -1, 0), (1, 1, 1), (1, -1, 1), (-1, -1, -1)], dtype=np.float64)
    d = dd[rng.integers(0, len(dd), n - 64)]
    p = rng.integers(0, 6, (n - 64, 3)).astype(np.float64)
    s = rng.choice([-0.75, -0.5, -0.25, 0.0, 0.25, 0.5, 0.75], 64)
    side = rng.choice([-1.0, 1.0], 64)
    to = np.stack([11.0 - side * (1.0 - s), np.full(64, 2.0), np.full(64, 2.0)], axis=1)
    td = np.stack([side * rng.choice([0.5, 1.0, 2.0, 4.0], 64), np.zeros(64), np.zeros(64)], axis=1)
    kinds.append(("diagonals, touching point", np.concatenate([p - 7.0 * d, to]), np.concatenate([d, td])))
    # one zero direction component, of either sign
    o = outside(n)
    d = toward(o)
    d[np.arange(n), rng.integers(0, 3, n)] = rng.choice([0.0, -0.0], n)
    kinds.append(("one zero component", o, d))
    # two zero components: axis-parallel rays off the lattice lines
    o = rng.integers(0, 6, (n, 3)) + rng.normal(0, 0.1, (n, 3))
    ax = rng.integers(0, 3, n)
    o[np.arange(n), ax] = rng.choice([-5.0, 11.0], n)
    d = unit[ax] * np.where(o[np.arange(n), ax] < 0, 1.0, -1.0)[:, None] * rng.choice([1.0, 0.5, 3.0], (n, 1))
    d = np.where(d == 0, rng.choice([0.0, -0.0], (n, 3)), d)
    kinds.append(("two zero components", o, d))
    # starts inside a sphere, and on a sphere's surface (and so on a box plane) along +x
    o = centers[rng.integers(0, len(centers), n)] + rng.uniform(-0.2, 0.2, (n, 3))
    kinds.append(("from inside", o, rng.normal(0, 1, (n, 3))))
    o = centers[rng.integers(0, len(centers), n)] + RAD * unit[rng.integers(0, 3, n)] * rng.choice([-1.0, 1.0], (n, 1))
    kinds.append(("from surfaces along +x", o, np.tile([1.0, 0.0, 0.0], (n, 1))))
    # general rays
    o = outside(n)
    kinds.append(("general", o, toward(o)))
    # a NaN direction component: hits nothing
    o = outside(n)
    d = toward(o)
    d[np.arange(n), rng.integers(0, 3, n)] = np.nan
    kinds.append(("NaN direction", o, d))
    o = np.concatenate([k[1] for k in kinds])
    d = np.concatenate([k[2] for k in kinds])
    return np.concatenate([o, d, rng.uniform(0, 1, (len(o), 1))], axis=1), [k[0] for k in kinds]


def _probe_case():
    """The lattice world, its 4096 rays and the oracle's closest hits, computed once."""
    if "probe" not in _cache:
        sc, centers = _lattice_world()
        rays, names = _rays(centers, np.random.default_rng(43))
        _cache["probe"] = (sc, rays, names, pyoracle.closest_hits(sc, rays, 1e-4, np.inf, seed=3))
    return _cache["probe"]


@pytest.mark.parametrize("waves", [1, 2, 3, 4])
def test_closest_hits_bit_for_bit(gpu_ctx, monkeypatch, waves):
    """The lean walk finds the oracle's hits, bit for bit: rows, diagonals, zero direction components, inside
    starts, NaN directions, the touching pair's exact ties."""
    sc, rays, names, ref = _probe_case()
    assert len(rays) == 4096 and len(names) == 8
    monkeypatch.setenv("RTAMD_WAVES", str(waves))
    for k in ("RTAMD_WIDE", "RTAMD_PACKED_KEYS"):
        monkeypatch.delenv(k, raising=False)
    gpu_ctx.upload(sc)
    got = gpu_ctx.closest_hits(rays, 1e-4, np.inf, seed=3, flags=rtamd.RT_DEBUG_WIDE)
    wk = gpu_ctx.wide_keys()
    assert wk["fits"] == 1 and wk["packed"] == 1, wk
    hits = got[:, 0].reshape(8, -1).sum(axis=1).astype(int)
    print("hits per ray kind:", dict(zip(names, hits.tolist())))
    for k in range(7):
        assert hits[k] > 0, f"ray kind '{names[k]}' is not exercised: {hits[k]} hits"
    tie = slice(2 * 512 - 64, 2 * 512)
    tie_t = (11.0 - rays[tie, 0]) / rays[tie, 3]
    assert got[tie, 0].all() and np.all(got[tie, 1] == tie_t), "no exact tie at the touching point"
    assert not got[7 * 512:, 0].any(), "a ray with a NaN direction hit something"
    bad = ~np.all(got[:, COLS] == ref[:, COLS], axis=1)
    assert not bad.any(), f"{int(bad.sum())} of {len(rays)} rays differ, first {np.flatnonzero(bad)[:8].tolist()}"


def _env(monkeypatch, env):
    for k in ("RTAMD_WIDE", "RTAMD_PACKED_KEYS", "RTAMD_WAVES"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _render(ctx, monkeypatch, env):
    """(bytes, linear averages), the launch and the sort form at 64x48, 4 spp, depth 50, seed 5 under `env`."""
    cam = rtamd.camera("random_scene", W, H)
    p = rtamd.make_params(W, H, 4, 50, rtamd.RT_RNG_PHILOX, seed=5)
    _env(monkeypatch, env)
    img = ctx.render(cam, p, linear=True)[:2]
    return img, ctx.last_launch(), ctx.wide_keys()


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1], equal_nan=True)


def _work(ctx, monkeypatch, packed):
    cam = rtamd.camera("random_scene", W, H)
    p = rtamd.make_params(W, H, 4, 50, rtamd.RT_RNG_PHILOX, seed=5)
    _env(monkeypatch, {"RTAMD_WIDE": "1", "RTAMD_PACKED_KEYS": "1" if packed else "0"})
    w = ctx.render_work(cam, p)
    assert ctx.wide_keys()["packed"] == int(packed), "the counting build does not walk in the timed kernel's form"
    assert ctx.last_launch()["loop"] == 2
    return w


def _scene(world):
    if world == "random_book_one":
        return rtamd.make_scene(world, rtamd.randGen(1024))[0]
    return _lattice_world(world == "lattice_twin")[0]


@pytest.mark.parametrize("world", ["random_book_one", "lattice", "lattice_twin"])
def test_images_equal_between_the_forms(gpu_ctx, world, monkeypatch):
    """The packed 4-wide kernel's image, bytes and linear averages, is the pairs form's and the binary walk's."""
    gpu_ctx.upload(_scene(world))
    packed, launch, keys = _render(gpu_ctx, monkeypatch, {"RTAMD_WIDE": "1"})
    print(world, launch, keys)
    assert launch["loop"] == 2 and launch["lds_staged"] == 1 and keys["packed"] == 1
    pairs, launch_p, keys_p = _render(gpu_ctx, monkeypatch, {"RTAMD_WIDE": "1", "RTAMD_PACKED_KEYS": "0"})
    assert launch_p["loop"] == 2 and keys_p["packed"] == 0
    binary, launch_b, _ = _render(gpu_ctx, monkeypatch, {"RTAMD_WIDE": "0"})
    assert launch_b["loop"] == 1
    assert _same(packed, pairs), "the packed form's image differs from the pairs form's"
    assert _same(packed, binary), "the packed form's image differs from the binary walk's"


@pytest.mark.parametrize("waves", [1, 2, 3, 4])
def test_twin_image_at_every_occupancy_target(gpu_ctx, monkeypatch, waves):
    """Each of the packed kernel's four instantiations renders the twin world, whose image is made of tie redos
    behind a filled stack, as the binary walk does."""
    gpu_ctx.upload(_scene("lattice_twin"))
    if "twin_binary" not in _cache:
        _cache["twin_binary"] = _render(gpu_ctx, monkeypatch, {"RTAMD_WIDE": "0"})[0]
    packed, launch, keys = _render(gpu_ctx, monkeypatch, {"RTAMD_WIDE": "1", "RTAMD_WAVES": str(waves)})
    assert launch["loop"] == 2 and launch["lds_staged"] == 1 and launch["waves"] == waves and keys["packed"] == 1, launch
    assert _same(packed, _cache["twin_binary"]), f"the {waves}-wave packed kernel's image differs from the binary walk's"


@pytest.mark.parametrize("world", ["random_book_one", "lattice", "lattice_twin"])
def test_samples_and_segments_equal_between_the_forms(gpu_ctx, world, monkeypatch):
    """The counting build walks as the timed kernel does: the same samples, segments and tie redos as the pairs
    form. Wide nodes and leaf tests are reported only (they depend on which items share a wave). The twin world
    must redo walks, so that the relocated redo is exercised."""
    gpu_ctx.upload(_scene(world))
    lean, pairs = _work(gpu_ctx, monkeypatch, True), _work(gpu_ctx, monkeypatch, False)
    for name, w in (("packed", lean), ("pairs", pairs)):
        print(f"{world} {name}: wide nodes / segment {w['wide_nodes'] / w['segments']:.4f}, "
              f"leaf tests / segment {w['prim_tests'] / w['segments']:.4f}, tie redos {w['tie_redos']}")
    assert lean["samples"] == pairs["samples"] == W * H * 4
    assert lean["segments"] == pairs["segments"]
    assert lean["tie_redos"] == pairs["tie_redos"]
    if world == "lattice_twin":
        assert lean["tie_redos"] > 0, "no tie occurred: the relocated redo is not exercised"
