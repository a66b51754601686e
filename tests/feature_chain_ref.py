"""The expected specular-chain feature sums (include/rt.h rt_render_features_chain), composed on the CPU.

tests/feature_ref.py's Philox streams and worlds; the UV pair and getRay restated once more, this time keeping
every stream's position (feature_ref.primary_rays does not return it); pyoracle.closest_hits per segment;
Dielectric scatter and Metal reflect restated in numpy in oracle/oracle.c's operation order (scatter, reflect,
refract, schlick, random_unit_vector, unit); pyoracle.probe(scene, "texture", ...) for the texture values; and the
left fold over the samples. Worlds without media only, for the reason feature_ref gives.

A sample is *undecided* when a Dielectric decision is within 1e-9 of its threshold (|rd - schlick| or
|eta sin_theta - 1|): the oracle takes x^5 with pow(x, 5), the device with pow5, numpy with its own power, which
may differ in the last bit. A pixel with such a sample is left out (`Chain.left_out`); the tests assert that at
most 0.1 % of pixels are.

Shared by the host and the GPU tests; compositions are cached and must be left unchanged."""
import functools

import numpy as np

import feature_ref
import pyoracle
import rtamd

RT_MAT_METAL, RT_MAT_DIELECTRIC = 1, 2
RT_CHAIN_DIELECTRIC, RT_CHAIN_METAL = 1, 2
SURFACE, MISS, CAP = 0, 1, 2  # how a sample's chain ended
UNDECIDED = 1e-9
PI = 3.141592653589793


def primary_rays_and_streams(cam, W, H, seed, samples):
    """feature_ref.primary_rays (uniformRandomUVs' pair, then getRay with its disk pairs and its time draw) for
    every pixel and every sample index in `samples`, sample-major: (rays (N, 7), the streams after getRay)."""
    n_s = len(samples)
    pid = np.tile(np.arange(W * H, dtype=np.int64), n_s)
    smp = np.repeat(np.asarray(samples, dtype=np.int64), W * H)
    px, row = (pid % W).astype(np.float64), pid // W
    g = feature_ref.Streams(seed, pid, smp)
    ru, rv = g.draw(), g.draw()
    u = (px + ru) / float(W)
    v = ((H - 1 - row).astype(np.float64) + rv) / float(H)
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
    return np.concatenate([o, d, tm[:, None]], axis=1), g


def _dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def _unit(a):
    return a / np.sqrt(_dot(a, a))[:, None]


def _reflect(v, n):
    return v - n * (2.0 * _dot(v, n))[:, None]


def _refract(v, n, eta):
    uv = _unit(v)
    cos_theta = _dot(-uv, n)
    par = (uv + n * cos_theta[:, None]) * eta[:, None]
    with np.errstate(invalid="ignore"):
        perp = n * (-np.sqrt(1.0 - _dot(par, par)))[:, None]
    return par + perp


def _schlick(cosine, ref_idx):
    r0 = (1.0 - ref_idx) / (1.0 + ref_idx)
    r1 = r0 * r0
    return r1 + (1.0 - r1) * np.power(1 - cosine, 5.0)


def scatter_metal(d, n, fuzz, aa, zz):
    """oracle.c scatter, RT_MAT_METAL: reflect(unit(d), n) + fuzz * random_unit_vector, the term added at fuzz 0
    too. (Bit for bit with the device at fuzz 0 only: cos and sin are numpy's.)"""
    a = aa * 2.0 * PI
    z = (zz * 2.0) - 1.0
    r = np.sqrt(1.0 - z * z)
    r_unit = np.stack([r * np.cos(a), r * np.sin(a), z], axis=1)
    return _reflect(_unit(d), n) + r_unit * fuzz[:, None]


def scatter_dielectric(d, n, ff, ref_idx, rd):
    """oracle.c scatter, RT_MAT_DIELECTRIC: (direction, how close the decision was to either threshold)."""
    eta = np.where(ff != 0, 1.0 / ref_idx, ref_idx)
    ud = _unit(d)
    c = _dot(-ud, n)
    cos_theta = np.where(c <= 1.0, c, 1.0)
    sin_theta = np.sqrt(1.0 - cos_theta * cos_theta)
    sch = _schlick(cos_theta, eta)
    tir = eta * sin_theta > 1.0
    refl = tir | (rd < sch)
    out = np.where(refl[:, None], _reflect(ud, n), _refract(ud, n, eta))
    # (past total internal reflection the draw decides nothing)
    margin = np.minimum(np.abs(eta * sin_theta - 1.0), np.where(tir, np.inf, np.abs(rd - sch)))
    return out, margin


class Chain:
    """per_sample[s] (H, W, 8): the chain feature vectors of sample first + s; kind[s], bounces[s] (H, W): how that
    sample's chain ended (SURFACE, MISS, CAP) and the scatters it followed; left_out (H, W): pixels with an
    undecided sample; words[s] (H, W): stream words the sample consumed in all."""

    def __init__(self, scene, cam, W, H, seed, first, n, max_bounces, flags, max_fuzz):
        d = scene.desc
        assert not any(d.nodes[i].type == rtamd.RT_NODE_CONSTANT_MEDIUM for i in range(d.n_nodes)), "no media here"
        mtype = np.array([d.materials[m].type for m in range(d.n_materials)])
        mtex = np.array([d.materials[m].texture for m in range(d.n_materials)])
        mparam = np.array([d.materials[m].param for m in range(d.n_materials)])
        bg = np.array(d.background)
        rays, g = primary_rays_and_streams(cam, W, H, seed, range(first, first + n))
        N = len(rays)
        thr, length = np.ones((N, 3)), np.zeros(N)
        f = np.zeros((N, 8))
        kind, b = np.full(N, -1), np.zeros(N, dtype=np.int64)
        undecided = np.zeros(N, dtype=bool)
        active = np.ones(N, dtype=bool)
        self.scatters = 0
        while active.any():
            idx = np.flatnonzero(active)
            hits = pyoracle.closest_hits(scene, rays[idx], 1e-4, float("inf"))
            got = hits[:, 0] == 1
            miss = idx[~got]
            f[miss, 0:3] = thr[miss] * bg[None, :]
            kind[miss] = MISS
            active[miss] = False
            idx, hits = idx[got], hits[got]
            dd = rays[idx, 3:6]
            length[idx] = length[idx] + hits[:, 1] * np.sqrt(_dot(dd, dd))
            mats = hits[:, 11].astype(np.int64)
            diel, metal = mtype[mats] == RT_MAT_DIELECTRIC, mtype[mats] == RT_MAT_METAL
            could = (diel & bool(flags & RT_CHAIN_DIELECTRIC)) | (metal & bool(flags & RT_CHAIN_METAL) &
                                                                   (mparam[mats] <= max_fuzz))
            follow = could & (b[idx] < max_bounces)
            a = np.ones((len(idx), 3))
            if (~diel).any():
                rec = np.concatenate([mtex[mats[~diel]][:, None].astype(np.float64), hits[~diel, 8:10], hits[~diel, 2:5]],
                                     axis=1)
                a[~diel] = pyoracle.probe(scene, "texture", rec)
            end = idx[~follow]
            f[end, 0:3] = thr[end] * a[~follow]
            f[end, 3:6] = hits[~follow, 5:8]
            f[end, 6] = length[end]
            f[end, 7] = 1.0
            kind[end] = np.where(could[~follow], CAP, SURFACE)
            active[end] = False
            # the followed: Metal draws two words, Dielectric one
            new_d = np.zeros((len(idx), 3))
            m_sel, d_sel = follow & metal, follow & diel
            if m_sel.any():
                mask = np.zeros(N, dtype=bool)
                mask[idx[m_sel]] = True
                aa, zz = g.draw(mask), g.draw(mask)
                new_d[m_sel] = scatter_metal(dd[m_sel], hits[m_sel, 5:8], mparam[mats[m_sel]], aa, zz)
            if d_sel.any():
                mask = np.zeros(N, dtype=bool)
                mask[idx[d_sel]] = True
                rd = g.draw(mask)
                new_d[d_sel], margin = scatter_dielectric(dd[d_sel], hits[d_sel, 5:8], hits[d_sel, 10],
                                                          mparam[mats[d_sel]], rd)
                undecided[idx[d_sel]] |= margin < UNDECIDED
            go = idx[follow]
            thr[go] = thr[go] * a[follow]
            rays[go, 0:3] = hits[follow, 2:5]
            rays[go, 3:6] = new_d[follow]
            b[go] += 1
            self.scatters += len(go)
        self.W, self.H, self.first, self.n = W, H, first, n
        self.per_sample = f.reshape(n, H, W, 8)
        self.kind, self.bounces = kind.reshape(n, H, W), b.reshape(n, H, W)
        self.words = g.pos.reshape(n, H, W).copy()
        self.left_out = undecided.reshape(n, H, W).any(axis=0)
        for a in (self.per_sample, self.kind, self.bounces, self.words, self.left_out):
            a.setflags(write=False)

    def sums(self, first=None, n=None, start=None, only=None):
        """The left fold, in sample order, of samples first .. first + n - 1 (default: all), from 0 or `start`;
        `only`: of the samples whose chain ended that way, the others adding 0."""
        first = self.first if first is None else first
        n = self.n - (first - self.first) if n is None else n
        acc = np.zeros((self.H, self.W, 8)) if start is None else start.copy()
        for s in range(first - self.first, first - self.first + n):
            v = self.per_sample[s]
            acc = acc + (v if only is None else v * (self.kind[s] == only)[..., None])
        return acc

    def counts(self):
        """rt_feature_chain_stats of the whole composition."""
        return dict(samples=int(self.kind.size), ended_surface=int((self.kind == SURFACE).sum()),
                    ended_miss=int((self.kind == MISS).sum()), ended_cap=int((self.kind == CAP).sum()),
                    bounces=int(self.bounces.sum()))


@functools.lru_cache(maxsize=None)
def specular_world(fuzzy=False):
    """(scene, camera) of a specular-only world: a 5 x 4 grid of well-separated spheres, Dielectric and fuzz-0 Metal
    in turn, constant textures, no emitter, a constant background. `fuzzy`: a second row of Metal spheres of fuzz 0.1
    and 0.3 above it. 20 leaves or more, so the device walks it 4-wide."""
    b = rtamd.Builder(rtamd.randGen(7))
    items = []
    for j in range(4):
        for i in range(5):
            k = 5 * j + i
            if (i + j) % 2:
                m = b.metal(b.constantColor(0.55 + 0.02 * k, 0.9 - 0.02 * k, 0.6 + 0.01 * k), 0.0)
            else:
                m = b.dielectric(1.3 + 0.02 * k)
            items.append(b.sphere(((i - 2.0) * 3.2, 0.0, (j - 1.5) * 3.2), 0.8, m))
    if fuzzy:
        for i, fz in enumerate((0.1, 0.3, 0.1, 0.3)):
            m = b.metal(b.constantColor(0.8, 0.7 + 0.05 * i, 0.5), fz)
            items.append(b.sphere(((i - 1.5) * 3.2, 2.6, 0.0), 0.8, m))
    scene = b.finish(b.makeBVH((0.0, 1.0), items), -1, (0.6, 0.7, 0.9))
    cam = rtamd.newCamera((0.0, 11.0, -15.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 40.0, 4.0 / 3.0, 0.05, 18.0, 0.0, 1.0)
    return scene, cam


def world(name):
    """(scene, camera factory): "specular", "specular_fuzzy", or a world of feature_ref.world."""
    if name.startswith("specular"):
        scene, cam = specular_world(name == "specular_fuzzy")
        return scene, lambda W, H: cam
    return feature_ref.world(name)


@functools.lru_cache(maxsize=None)
def composition(name, W, H, n, max_bounces, flags, max_fuzz=0.0, seed=1024, first=0):
    scene, cam = world(name)
    return Chain(scene, cam(W, H), W, H, seed, first, n, max_bounces, flags, max_fuzz)
