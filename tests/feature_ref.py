"""The expected first-hit feature sums (include/rt.h rt_render_features), composed on the CPU from oracle pieces:
a numpy Philox4x32-10 (checked against pyoracle.philox in tests/test_features_host.py) and the word -> draw
conversion (checked there against oracle_word_to_draw), a numpy restatement of the UV pair and getRay (the disk
rejection loop and the time draw, in oracle/oracle.c's operation order), pyoracle.closest_hits(scene, rays, 1e-4,
inf) for the hits, pyoracle.probe(scene, "texture", ...) for the albedo, and a left fold over the samples.

The oracle's closest-hits entry draws a ConstantMedium from the stream position 0 of (key, ray index), not from
the sample's position after getRay: worlds with media are not composed here (tests/test_gpu_features.py checks
their coverage against depth-1 renders instead).

Shared by the host and the GPU tests; compositions are cached and must be left unchanged."""
import functools
import os

import numpy as np

import pyoracle
import rtamd

RT_MAT_DIELECTRIC = 2
RT_TEX_CONSTANT = 0
HERE = os.path.dirname(os.path.abspath(__file__))
M32 = np.uint64(0xFFFFFFFF)


def philox(ctr, key):
    """Philox4x32-10 (Salmon et al. 2011) on (N, 4) uint32 counters with one key (k0, k1): (N, 4) uint32."""
    c = [np.ascontiguousarray(ctr[:, i]).astype(np.uint64) for i in range(4)]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return np.stack(c, axis=1).astype(np.uint32)


def word_to_draw(w):
    """random-1.2.0's `random :: Double` = 1 - word64 / 2^64 (uint64 -> double rounds to nearest, as C's cast)."""
    return 1.0 - w.astype(np.float64) / 18446744073709551616.0


class Streams:
    """The tier-B streams of N (pixel, sample) pairs: key = seed, counter {pair, sample, pid, 0}; word i of a
    stream is half i % 2 of block i // 2. `draw()` returns each stream's next draw for the streams in `mask`."""

    def __init__(self, seed, pid, sample):
        self.key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
        self.pid = pid.astype(np.uint32)
        self.sample = sample.astype(np.uint32)
        self.pos = np.zeros(len(pid), dtype=np.int64)

    def draw(self, mask=None):
        idx = np.arange(len(self.pid)) if mask is None else np.flatnonzero(mask)
        ctr = np.zeros((len(idx), 4), dtype=np.uint32)
        ctr[:, 0] = self.pos[idx] // 2
        ctr[:, 1] = self.sample[idx]
        ctr[:, 2] = self.pid[idx]
        o = philox(ctr, self.key).astype(np.uint64)
        odd = (self.pos[idx] % 2).astype(bool)
        lo = np.where(odd, o[:, 2], o[:, 0])
        hi = np.where(odd, o[:, 3], o[:, 1])
        self.pos[idx] += 1
        return word_to_draw(lo | (hi << np.uint64(32)))


def primary_rays(cam, W, H, seed, samples):
    """The primary rays rt_render traces for every pixel (image order) and every sample index in `samples`:
    (len(samples), H*W, 7) rays (o, d, time). uniformRandomUVs' pair, then getRay (src/Lib.hs:1253-1267) with its
    own draws: disk rejection pairs, then the time."""
    n_s = len(samples)
    pid = np.tile(np.arange(W * H, dtype=np.int64), n_s)
    smp = np.repeat(np.asarray(samples, dtype=np.int64), W * H)
    px, row = (pid % W).astype(np.float64), pid // W
    g = Streams(seed, pid, smp)
    ru, rv = g.draw(), g.draw()
    u = (px + ru) / float(W)
    v = ((H - 1 - row).astype(np.float64) + rv) / float(H)
    # randomInUnitDisk: p = 2 * (x, y, 0) - (1, 1, 0) until |p|^2 < 1
    dx, dy = np.zeros(len(pid)), np.zeros(len(pid))
    todo = np.ones(len(pid), dtype=bool)
    while todo.any():
        x, y = g.draw(todo), g.draw(todo)
        qx, qy, qz = 2.0 * x - 1.0, 2.0 * y - 1.0, 2.0 * 0.0 - 0.0
        ok = qx * qx + qy * qy + qz * qz < 1.0
        idx = np.flatnonzero(todo)
        dx[idx[ok]], dy[idx[ok]] = qx[ok], qy[ok]
        todo[idx[ok]] = False
    lr = cam.lens_radius
    rdx, rdy = lr * dx, lr * dy
    cu, cv = np.array(cam.u), np.array(cam.v)
    offset = rdx[:, None] * cu[None, :] + rdy[:, None] * cv[None, :]
    rd = g.draw()
    tm = cam.t0 + (cam.t1 - cam.t0) * rd
    origin, llc = np.array(cam.origin), np.array(cam.llc)
    horiz, vert = np.array(cam.horiz), np.array(cam.vert)
    o = origin[None, :] + offset
    d = (((llc[None, :] + u[:, None] * horiz[None, :]) + v[:, None] * vert[None, :]) - origin[None, :]) - offset
    return np.concatenate([o, d, tm[:, None]], axis=1).reshape(n_s, W * H, 7)


def constant_textures(scene):
    """Every texture of the descriptor is constant (then the albedo sums are exact)."""
    return all(scene.desc.textures[i].type == RT_TEX_CONSTANT for i in range(scene.desc.n_textures))


def sample_features(scene, rays):
    """The feature vectors (N, 8) of N primary rays, and the oracle's closest-hit records (N, 12)."""
    hits = pyoracle.closest_hits(scene, rays, 1e-4, float("inf"))
    got = hits[:, 0] == 1
    f = np.zeros((len(rays), 8))
    f[:, 0:3] = np.array(scene.desc.background)[None, :]
    idx = np.flatnonzero(got)
    mats = hits[idx, 11].astype(np.int64)
    mtype = np.array([scene.desc.materials[int(m)].type for m in range(scene.desc.n_materials)])
    mtex = np.array([scene.desc.materials[int(m)].texture for m in range(scene.desc.n_materials)])
    albedo = np.ones((len(idx), 3))
    tex = mtype[mats] != RT_MAT_DIELECTRIC
    if tex.any():
        rec = np.concatenate([mtex[mats[tex]][:, None].astype(np.float64), hits[idx[tex], 8:10], hits[idx[tex], 2:5]],
                             axis=1)
        albedo[tex] = pyoracle.probe(scene, "texture", rec)
    f[idx, 0:3] = albedo
    f[idx, 3:6] = hits[idx, 5:8]
    d = rays[idx, 3:6]
    f[idx, 6] = hits[idx, 1] * np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    f[idx, 7] = 1.0
    return f, hits


class Composition:
    """per_sample[s] (H, W, 8): the feature vectors of sample first + s; hit_mats: the materials some sample hit."""

    def __init__(self, scene, cam, W, H, seed, first, n):
        rays = primary_rays(cam, W, H, seed, range(first, first + n))
        f, hits = sample_features(scene, rays.reshape(-1, 7))
        self.W, self.H, self.first, self.n = W, H, first, n
        self.per_sample = f.reshape(n, H, W, 8)
        self.hit_mats = set(int(m) for m in np.unique(hits[hits[:, 0] == 1][:, 11]))
        self.per_sample.setflags(write=False)

    def sums(self, first=None, n=None, start=None):
        """The left fold, in sample order, of samples first .. first + n - 1 (default: all), from 0 or `start`."""
        first = self.first if first is None else first
        n = self.n - (first - self.first) if n is None else n
        acc = np.zeros((self.H, self.W, 8)) if start is None else start.copy()
        for s in range(first - self.first, first - self.first + n):
            acc = acc + self.per_sample[s]
        return acc

    def coverage(self):
        hits = self.sums()[..., 7]
        return float(hits.mean() / self.n), float(((hits > 0) & (hits < self.n)).mean())


@functools.lru_cache(maxsize=None)
def named_scene(name):
    earth = np.load(os.path.join(HERE, "golden", "earthmap_rgb8.npz"))["rgb"] if name == "earth" else None
    return rtamd.make_scene(name, rtamd.randGen(1024), earth=earth)[0]


NAMED_CAMERAS = {"random_book_one": "random_scene", "two_perlin_spheres": "two_spheres", "earth": "two_spheres"}


@functools.lru_cache(maxsize=None)
def world(name):
    """(scene, camera factory (W, H) -> rt_camera) of a zoo world (tests/zoo_worlds.py) or a named scene."""
    import zoo_worlds
    if name in zoo_worlds.NAMES:
        z = zoo_worlds.build(name)
        return z.scene, lambda W, H: z.camera
    return named_scene(name), lambda W, H: rtamd.camera(NAMED_CAMERAS[name], W, H)


@functools.lru_cache(maxsize=None)
def composition(name, W, H, n, seed=1024, first=0):
    scene, cam = world(name)
    return Composition(scene, cam(W, H), W, H, seed, first, n)


@functools.lru_cache(maxsize=None)
def fog_world():
    """(scene, camera) of a media world made with rtamd.Builder: 24 small spheres, two world-level ConstantMediums
    (a cuboid and a sphere boundary), a third medium inside translate(rotateZ(BVH)), no emitter, background
    (1, 1, 1). The device walks it with the mixed walk over 4-wide trees (rt_prepare_scene: mixed_wide = 1)."""
    b = rtamd.Builder(rtamd.randGen(21))
    mats = [b.lambertian(b.constantColor(0.8, 0.3, 0.3)), b.metal(b.constantColor(0.7, 0.7, 0.8), 0.1),
            b.dielectric(1.5)]
    fog = [b.constantColor(0.9 - 0.1 * i, 0.8, 0.7 + 0.1 * i) for i in range(3)]
    items = [b.sphere(((i - 2.5) * 3.0, 0.0, (j - 1.5) * 3.0), 0.6, mats[(i + j) % 3])
             for j in range(4) for i in range(6)]
    items.append(b.constantMedium(0.4, fog[0], b.cuboid((-9.0, 1.5, -6.0), (-1.0, 4.5, 0.0), mats[2])))
    items.append(b.constantMedium(0.5, fog[1], b.sphere((5.0, 3.0, 2.0), 2.5, mats[2])))
    inner = [b.sphere(((i - 1.5) * 2.0, 0.0, (j - 0.5) * 2.0), 0.5, mats[(i + j) % 3])
             for j in range(2) for i in range(4)]
    inner.append(b.constantMedium(0.6, fog[2], b.sphere((0.0, 1.5, 0.0), 1.2, mats[2])))
    items.append(b.translate((0.0, 5.0, 8.0), b.rotate(2, 25.0, b.makeBVH((0.0, 1.0), inner))))
    scene = b.finish(b.makeBVH((0.0, 1.0), items), -1, (1.0, 1.0, 1.0))
    cam = rtamd.newCamera((0.0, 14.0, -24.0), (0.0, 2.0, 2.0), (0.0, 1.0, 0.0), 40.0, 4.0 / 3.0, 0.1, 28.0, 0.0, 1.0)
    return scene, cam


@functools.lru_cache(maxsize=None)
def deep_world():
    """(scene, camera) of a world whose instance frames nest five deep, past RT_MAX_FRAMES: the device walks it
    with the recursive walk (rt_prepare_scene: replace_ok = 0). Constant textures, one material per level."""
    b = rtamd.Builder(rtamd.randGen(5))
    mat = [b.lambertian(b.constantColor(0.2 + 0.1 * i, 0.5, 0.9 - 0.1 * i)) for i in range(6)]
    h = b.makeBVH((0.0, 1.0), [b.sphere((i - 1.0, 0.0, 0.0), 0.45, mat[5]) for i in range(3)])
    for i in range(5):
        h = b.makeBVH((0.0, 1.0), [b.translate((0.15, 0.0, 0.0), h), b.sphere((0.3 * i - 0.6, 1.0 + i, 0.0), 0.45, mat[i])])
    scene = b.finish(h, -1, (0.6, 0.7, 0.9))
    cam = rtamd.newCamera((0.0, 2.5, -12.0), (0.0, 2.5, 0.0), (0.0, 1.0, 0.0), 40.0, 4.0 / 3.0, 0.05, 12.0, 0.0, 1.0)
    return scene, cam


def hits_from_render(lin, spp, background):
    """Samples that hit something, per pixel, from a max_depth = 1, RT_FLAG_NAN_ZERO render of a world without
    emitters: a hit's colour is black (depth 0 after one scatter; an emitter's front face aside), a miss's the
    background, so hits = spp - rint(lin * spp / background), channel 0."""
    return spp - np.rint(lin[..., 0] * spp / background[0])
