"""Four small worlds made through rtamd.Builder (the rt_obj_* constructor surface), aimed at what the
named scenes leave out: rotations about X and Z, every leaf kind under Translate/Rotate chains, moving
spheres under chains, instance frames whose second axis is not Y, media inside frames, and lights trees of
three and four items with leaves htblRandom / htblPdfValue do not sample (src/Lib.hs:673-724).

Every world is one recipe run twice: against rtamd.Builder (the product's C++ constructors) and against
oracle/scenes_ref.py's constructors (the independent restatement), with the same numbers in the same order,
so the two can be compared structurally (tests/test_zoo_host.py). Every labelled kind of object has a
material of its own: column 11 of a closest-hits record tells which kind was hit. Only nodes that the world
or its lights tree references are created (rt_prepare_scene derives the kernel variant from every node of
the descriptor).

  chains  Cornell-like variant: spheres, rects in all three planes, a cuboid, and for each axis
          translate(rotate(cuboid)), rotate(translate(rotate'(cuboid))) and rotate(rect); lights = makeBVH of
          an XZ rect, a sphere and an XY rect (three items: unequal htblSize weights, one unsampled kind)
  moving  spheres and moving spheres over (0, 1): still, far-moving, under translate, under rotate per axis
  frames  translate(rotateX(BVH)) and translate(rotateZ(translate(BVH))), 16 leaves each; lights = makeBVH of
          four items (depth 2), one a translate(XZ rect)
  media   frames plus a medium inside a frame (boundary rotateX(cuboid)) and two at world level
"""
import functools
import math

import numpy as np

import rtamd
import scenes_ref as R

NAMES = ("chains", "moving", "frames", "media")
SEEDS = {"chains": 11, "moving": 12, "frames": 13, "media": 14}
XY, XZ, YZ = rtamd.XYPlane, rtamd.XZPlane, rtamd.YZPlane


# ----------------------------------------------------------------------------- the two constructor sets
class _Product:
    """rtamd.Builder: ids."""

    def __init__(self, gen):
        self.b = rtamd.Builder(gen)

    def const(self, r, g, b):
        return self.b.constantColor(r, g, b)

    def checker(self, odd, even):
        return self.b.checkerTexture(odd, even)

    def lambertian(self, tex):
        return self.b.lambertian(tex)

    def metal(self, tex, fuzz):
        return self.b.metal(tex, fuzz)

    def dielectric(self, ri):
        return self.b.dielectric(ri)

    def light(self, tex):
        return self.b.diffuseLight(tex)

    def sphere(self, c, r, m):
        return self.b.sphere(c, r, m)

    def msphere(self, c0, c1, r, m):
        return self.b.movingSphere(c0, c1, 0.0, 1.0, r, m)

    def rect(self, plane, a0, a1, b0, b1, k, m):
        return self.b.rect(plane, a0, a1, b0, b1, k, m)

    def cuboid(self, lo, hi, m):
        return self.b.cuboid(lo, hi, m)

    def translate(self, off, h):
        return self.b.translate(off, h)

    def rotate(self, axis, angle, h):
        return self.b.rotate(axis, angle, h)

    def medium(self, density, tex, h):
        return self.b.constantMedium(density, tex, h)

    def bvh(self, items):
        return self.b.makeBVH((0.0, 1.0), items)


class _Restated:
    """oracle/scenes_ref.py: dicts and tuples."""

    def __init__(self, gen):
        self.g = R.Gen(gen)

    def const(self, r, g, b):
        return R.const(r, g, b)

    def checker(self, odd, even):
        return ("checker", odd, even)

    def lambertian(self, tex):
        return R.lam(tex)

    def metal(self, tex, fuzz):
        return ("metal", tex, fuzz)

    def dielectric(self, ri):
        return ("dielectric", ri)

    def light(self, tex):
        return ("diffuse_light", tex)

    def sphere(self, c, r, m):
        return R.sphere(c, r, m)

    def msphere(self, c0, c1, r, m):
        return R.moving_sphere(c0, c1, 0.0, 1.0, r, m)

    def rect(self, plane, a0, a1, b0, b1, k, m):
        return R.rect(plane, a0, a1, b0, b1, k, m)

    def cuboid(self, lo, hi, m):
        return R.cuboid(lo, hi, m)

    def translate(self, off, h):
        return R.translate(off, h)

    def rotate(self, axis, angle, h):
        return R.rotate(axis, angle, h)

    def medium(self, density, tex, h):
        return R.constant_medium(density, tex, h)

    def bvh(self, items):
        return R.make_bvh(self.g, items)


class _Recipe:
    """A constructor set plus the labelled materials: `mats` label -> material (one per kind of object),
    `media` label -> ConstantMedium (whose Isotropic material the constructor makes)."""

    def __init__(self, k):
        self.k = k
        self.mats = {}
        self.media = {}

    def mat(self, label, kind=None, tex=None):
        i = len(self.mats)
        col = tuple(0.2 + 0.6 * ((i * f) % 1.0) for f in (0.37, 0.61, 0.83))
        kind = kind or ("lambertian", "metal", "dielectric")[i % 3]
        k = self.k
        if kind == "dielectric":
            m = k.dielectric(1.3 + 0.01 * i)
        elif kind == "metal":
            m = k.metal(k.const(*col), 0.05 * (i % 5))
        elif kind == "diffuse_light":
            m = k.light(k.const(4.0 + col[0], 4.0 + col[1], 4.0 + col[2]))
        else:
            m = k.lambertian(k.const(*col) if tex is None else tex)
        assert label not in self.mats
        self.mats[label] = m
        return m

    def medium(self, label, density, boundary):
        i = len(self.media)
        h = self.k.medium(density, self.k.const(0.9 - 0.1 * i, 0.8, 0.7 + 0.1 * i), boundary)
        self.media[label] = h
        return h


# ----------------------------------------------------------------------------- geometry helpers
def _cells(n, pitch, y):
    """Centres of an n x n grid in the xz plane, row by row."""
    h = (n - 1) / 2.0
    return iter([((i - h) * pitch, y, (j - h) * pitch) for j in range(n) for i in range(n)])


def _add(p, d):
    return (p[0] + d[0], p[1] + d[1], p[2] + d[2])


def _unrot(axis, angle, p):
    """The point that rotate(axis, angle, .) carries to p (to place an object under a rotation)."""
    rad = angle * R.PI / 180.0
    return R.rotate_point(axis, -math.sin(rad), math.cos(rad), p)


def _rect_at(k, plane, c, h, m):
    if plane == XY:
        return k.rect(XY, c[0] - h, c[0] + h, c[1] - h, c[1] + h, c[2], m)
    if plane == XZ:
        return k.rect(XZ, c[0] - h, c[0] + h, c[2] - h, c[2] + h, c[1], m)
    return k.rect(YZ, c[1] - h, c[1] + h, c[2] - h, c[2] + h, c[0], m)


def _box_at(k, c, half, m):
    return k.cuboid((c[0] - half[0], c[1] - half[1], c[2] - half[2]), (c[0] + half[0], c[1] + half[1], c[2] + half[2]), m)


ORIGIN = (0.0, 0.0, 0.0)
AX = "xyz"


# ----------------------------------------------------------------------------- the recipes
def _chains(q):
    k = q.k
    at = _cells(5, 4.0, 1.0)
    items = [k.rect(XZ, -14.0, 14.0, -14.0, 14.0, -4.0, q.mat("rect_xz_floor", "lambertian"))]
    for lab, kind in (("sphere_lam", "lambertian"), ("sphere_metal", "metal"), ("sphere_glass", "dielectric")):
        items.append(k.sphere(next(at), 1.0, q.mat(lab, kind)))
    l_sphere = k.sphere(_add(next(at), (0.0, 0.5, 0.0)), 0.8, q.mat("light_sphere", "diffuse_light"))
    items.append(_rect_at(k, XY, next(at), 1.0, q.mat("rect_xy")))
    l_xy = _rect_at(k, XY, next(at), 1.0, q.mat("light_rect_xy", "diffuse_light"))
    l_xz = _rect_at(k, XZ, _add(next(at), (0.0, 2.0, 0.0)), 1.2, q.mat("light_rect_xz", "diffuse_light"))
    items += [l_sphere, l_xy, l_xz]
    items.append(_rect_at(k, YZ, next(at), 1.0, q.mat("rect_yz_a")))
    items.append(_rect_at(k, YZ, next(at), 0.8, q.mat("rect_yz_b")))
    items.append(_box_at(k, next(at), (1.0, 1.1, 0.9), q.mat("cuboid")))
    for ax, ang in enumerate((25.0, -35.0, 50.0)):
        box = _box_at(k, ORIGIN, (1.0, 0.8, 0.6), q.mat(f"t_r{AX[ax]}_cuboid"))
        items.append(k.translate(next(at), k.rotate(ax, ang, box)))
    for ax, (ang, ang2) in enumerate(((40.0, -15.0), (-20.0, 30.0), (15.0, 65.0))):
        nx = (ax + 1) % 3
        inner = k.rotate(nx, ang2, _box_at(k, ORIGIN, (0.9, 0.7, 1.0), q.mat(f"r{AX[ax]}_t_r{AX[nx]}_cuboid")))
        items.append(k.rotate(ax, ang, k.translate(_unrot(ax, ang, next(at)), inner)))
    for ax, ang in enumerate((-30.0, 55.0, 20.0)):
        r = _rect_at(k, (XZ, XY, YZ)[ax], _unrot(ax, ang, next(at)), 1.0, q.mat(f"r{AX[ax]}_rect"))
        items.append(k.rotate(ax, ang, r))
    world = k.bvh(items)
    lights = k.bvh([l_xz, l_sphere, l_xy])
    return world, lights, (0.05, 0.05, 0.08)


def _moving(q):
    k = q.k
    at = _cells(5, 4.0, 0.0)
    chk = k.checker(k.const(0.2, 0.3, 0.1), k.const(0.9, 0.9, 0.9))
    items = [k.sphere((0.0, -1003.0, 0.0), 1000.0, q.mat("ground", "lambertian", tex=chk))]
    still = [q.mat("sphere_lam", "lambertian"), q.mat("sphere_metal", "metal"), q.mat("sphere_glass", "dielectric")]
    for i in range(9):
        items.append(k.sphere(next(at), 0.7 + 0.05 * i, still[i % 3]))
    m = q.mat("moving")
    for d in ((0.6, 0.3, -0.4), (-0.5, 0.0, 0.5), (0.0, 0.8, 0.0)):
        c = next(at)
        items.append(k.msphere(c, _add(c, d), 0.8, m))
    c = next(at)
    items.append(k.msphere(c, c, 0.9, q.mat("moving_still")))
    c = next(at)
    next(at)  # (the cell it moves into)
    items.append(k.msphere(c, _add(c, (3.5, 0.0, 0.0)), 0.5, q.mat("moving_far")))
    items.append(k.translate(next(at), k.msphere(ORIGIN, (0.5, 0.5, 0.0), 0.8, q.mat("t_moving"))))
    for ax, ang in enumerate((35.0, -50.0, 25.0)):
        c = next(at)
        c1 = _add(c, (0.4, 0.5, -0.6))
        ms = k.msphere(_unrot(ax, ang, c), _unrot(ax, ang, c1), 0.8, q.mat(f"r{AX[ax]}_moving"))
        items.append(k.rotate(ax, ang, ms))
    return k.bvh(items), None, (0.7, 0.8, 0.9)


def _inner(q, tag, chain_ax, medium):
    """The 16 leaves inside a frame (local coordinates), 17 with the medium."""
    k = q.k
    at = _cells(4, 3.0, 0.0)
    ms = [q.mat(f"{tag}_sphere_lam", "lambertian"), q.mat(f"{tag}_sphere_metal", "metal"),
          q.mat(f"{tag}_sphere_glass", "dielectric")]
    items = [k.sphere(next(at), 0.9, ms[i % 3]) for i in range(12)]
    c = next(at)
    items.append(k.msphere(c, _add(c, (0.5, 0.4, 0.3)), 0.8, q.mat(f"{tag}_moving")))
    items.append(_rect_at(k, XY, next(at), 1.0, q.mat(f"{tag}_rect_xy")))
    items.append(_box_at(k, next(at), (0.9, 1.0, 0.8), q.mat(f"{tag}_cuboid")))
    box = _box_at(k, ORIGIN, (0.9, 0.7, 0.8), q.mat(f"{tag}_t_r{AX[chain_ax]}_cuboid"))
    items.append(k.translate(next(at), k.rotate(chain_ax, 30.0, box)))
    if medium:
        bound = k.rotate(0, 30.0, _box_at(k, _unrot(0, 30.0, (0.0, 3.0, 0.0)), (1.2, 1.0, 1.1), ms[2]))
        items.append(q.medium(f"{tag}_medium_rx_cuboid", 0.9, bound))
    return items


def _frames(q, media):
    k = q.k
    frame_a = k.translate((-8.0, 1.0, -4.0), k.rotate(0, 20.0, k.bvh(_inner(q, "A", 2, media))))
    frame_b = k.translate((8.0, 1.5, -4.0),
                          k.rotate(2, -20.0, k.translate((0.5, 0.25, -0.5), k.bvh(_inner(q, "B", 1, False)))))
    items = [frame_a, frame_b, k.rect(XZ, -22.0, 22.0, -22.0, 22.0, -5.0, q.mat("rect_xz_floor", "lambertian"))]
    row1 = iter([(x, 0.0, 8.0) for x in (-12.0, -8.0, -4.0, 0.0, 4.0, 8.0, 12.0)])
    row2 = iter([(x, 0.0, 13.0) for x in (-12.0, -8.0, -4.0, 0.0, 4.0, 8.0, 12.0)])
    l_xz = _rect_at(k, XZ, _add(next(row1), (0.0, 2.5, 0.0)), 1.2, q.mat("light_rect_xz", "diffuse_light"))
    l_s1 = k.sphere(next(row1), 0.9, q.mat("light_sphere_a", "diffuse_light"))
    l_t = k.translate(_add(next(row1), (0.0, 2.0, 0.0)),
                      _rect_at(k, XZ, ORIGIN, 1.1, q.mat("light_t_rect_xz", "diffuse_light")))
    l_s2 = k.sphere(next(row1), 0.7, q.mat("light_sphere_b", "diffuse_light"))
    items += [l_xz, l_s1, l_t, l_s2]
    ms = [q.mat("sphere_lam", "lambertian"), q.mat("sphere_metal", "metal"), q.mat("sphere_glass", "dielectric")]
    for i in range(3):
        items.append(k.sphere(next(row1), 1.0, ms[i]))
    for i in range(3):
        items.append(k.sphere(next(row2), 0.8, ms[i]))
    c = next(row2)
    items.append(k.msphere(c, _add(c, (0.7, 0.6, 0.0)), 0.8, q.mat("moving")))
    items.append(_box_at(k, next(row2), (1.0, 0.9, 0.8), q.mat("cuboid")))
    items.append(_rect_at(k, YZ, next(row2), 1.0, q.mat("rect_yz")))
    items.append(k.rotate(1, 35.0, _rect_at(k, XY, _unrot(1, 35.0, next(row2)), 1.0, q.mat("ry_rect_xy"))))
    if media:
        items.append(q.medium("medium_sphere", 0.8, k.sphere((-4.0, 3.5, 13.0), 1.3, ms[2])))
        bound = k.translate((4.0, 3.5, 13.0), _box_at(k, ORIGIN, (1.2, 1.0, 1.1), ms[2]))
        items.append(q.medium("medium_t_cuboid", 0.8, bound))
    world = k.bvh(items)
    lights = None if media else k.bvh([l_xz, l_s1, l_t, l_s2])
    return world, lights, ((0.6, 0.7, 0.9) if media else (0.05, 0.06, 0.1))


RECIPES = {"chains": _chains, "moving": _moving, "frames": lambda q: _frames(q, False),
           "media": lambda q: _frames(q, True)}
CAMERAS = {  # lookfrom, lookat, vfov, aperture, focus distance (aspect 4:3, shutter 0..1)
    "chains": ((0.0, 17.0, -25.0), (0.0, 0.0, 0.0), 40.0, 0.1, 30.0),
    "moving": ((3.0, 16.0, -25.0), (0.0, 0.0, 0.0), 40.0, 0.1, 30.0),
    "frames": ((0.0, 26.0, -34.0), (0.0, 0.0, 3.0), 42.0, 0.1, 43.0),
    "media": ((0.0, 26.0, -34.0), (0.0, 0.0, 3.0), 42.0, 0.1, 43.0),
}


# ----------------------------------------------------------------------------- the worlds
class Zoo:
    """A built world: `scene`, `g1` (the generator after construction), `kinds` (label -> material id, one per
    kind of object, media included), `leaves` (world-space targets for rays), `camera`."""


def restate(name):
    """(world, lights or None, background, g1) by oracle/scenes_ref.py's constructors."""
    k = _Restated(rtamd.randGen(SEEDS[name]))
    world, lights, bg = RECIPES[name](_Recipe(k))
    return world, lights, bg, k.g.state


@functools.lru_cache(maxsize=None)
def build(name):
    """The world by rtamd.Builder. Cached: tests share one instance and leave it unchanged."""
    k = _Product(rtamd.randGen(SEEDS[name]))
    q = _Recipe(k)
    world, lights, bg = RECIPES[name](q)
    z = Zoo()
    z.name = name
    z.scene = k.b.finish(world, -1 if lights is None else lights, bg)
    z.g1 = k.b.gen
    nodes = z.scene.nodes
    z.kinds = dict(q.mats)
    for label, h in q.media.items():
        z.kinds[label] = int(nodes[h]["b"])
    assert len(set(z.kinds.values())) == len(z.kinds)
    z.leaves = _leaves(z.scene)
    lf, la, vfov, ap, fd = CAMERAS[name]
    z.camera = rtamd.newCamera(lf, la, (0.0, 1.0, 0.0), vfov, 4.0 / 3.0, ap, fd, 0.0, 1.0)
    return z


def camera_restated(name):
    lf, la, vfov, ap, fd = CAMERAS[name]
    return R.new_camera(lf, la, (0.0, 1.0, 0.0), vfov, 4.0 / 3.0, ap, fd, 0.0, 1.0)


def frame_roots(scene):
    """Ids of the BVH nodes inside the instance frames reachable from the scene's world root."""
    nodes = scene.nodes
    out = []

    def go(i, inst):
        t = int(nodes[i]["type"])
        if t == rtamd.RT_NODE_BVH:
            if inst:
                out.append(i)
            for ch in {int(nodes[i]["a"]), int(nodes[i]["b"])}:
                go(ch, False)
        elif t in (rtamd.RT_NODE_TRANSLATE, rtamd.RT_NODE_ROTATE):
            go(int(nodes[i]["a"]), True)
    go(scene.desc.world_root, False)
    return sorted(set(out))


def _leaves(scene):
    """Every primitive and medium of the world as (material id, centre at time 0, centre at time 1, half
    extents, inside a frame) in world coordinates: where to aim rays."""
    nodes = scene.nodes
    out = []

    def to_world(p, chain):
        for t, nd in reversed(chain):
            f = nd["f"]
            if t == rtamd.RT_NODE_TRANSLATE:
                p = (p[0] + f[0], p[1] + f[1], p[2] + f[2])
            else:
                p = R.rotate_point(int(nd["b"]), float(f[0]), float(f[1]), p)
        return np.array(p, dtype=np.float64)

    def go(i, chain, framed, mat):
        nd = nodes[i]
        t = int(nd["type"])
        f = [float(x) for x in nd["f"]]
        if t == rtamd.RT_NODE_BVH:
            for ch in sorted({int(nd["a"]), int(nd["b"])}):
                go(ch, chain, framed or bool(chain), mat)
            return
        if t in (rtamd.RT_NODE_TRANSLATE, rtamd.RT_NODE_ROTATE):
            return go(int(nd["a"]), chain + [(t, nd)], framed, mat)
        if t == rtamd.RT_NODE_CONSTANT_MEDIUM:
            return go(int(nd["a"]), chain, framed, int(nd["b"]))
        m = int(nd["a"]) if mat is None else mat
        if t == rtamd.RT_NODE_SPHERE:
            c0 = c1 = f[0:3]
            half = [f[3]] * 3
        elif t == rtamd.RT_NODE_MOVING_SPHERE:
            c0, c1 = f[0:3], f[3:6]
            half = [float(nodes[i + 1]["f"][3])] * 3
        elif t == rtamd.RT_NODE_CUBOID:
            c0 = c1 = [(f[a] + f[3 + a]) / 2 for a in range(3)]
            half = [(f[3 + a] - f[a]) / 2 for a in range(3)]
        else:
            ca, cb, ha, hb = (f[0] + f[1]) / 2, (f[2] + f[3]) / 2, (f[1] - f[0]) / 2, (f[3] - f[2]) / 2
            c0 = c1 = {rtamd.RT_NODE_RECT_XY: [ca, cb, f[4]], rtamd.RT_NODE_RECT_XZ: [ca, f[4], cb],
                       rtamd.RT_NODE_RECT_YZ: [f[4], ca, cb]}[t]
            half = {rtamd.RT_NODE_RECT_XY: [ha, hb, 0.0], rtamd.RT_NODE_RECT_XZ: [ha, 0.0, hb],
                    rtamd.RT_NODE_RECT_YZ: [0.0, ha, hb]}[t]
        out.append((m, to_world(tuple(c0), chain), to_world(tuple(c1), chain), min(2.0, max(half)), framed))
    go(scene.desc.world_root, [], False, None)
    return out


def rays(z, n=1 << 14, seed=5):
    """n rays (origin, direction, time) for closest-hit comparisons over world `z`. Every ray is aimed at a
    leaf of a kind drawn uniformly (where the leaf is at the ray's time), jittered within the leaf's size:
      * one eighth axis-aligned (exact zeros in two components), both signs, from 30 units away;
      * one quarter from origins among the frames' contents (among the leaves, in worlds without frames),
        half of those in a random direction instead;
      * the rest from 40 units outside, from above the floor, with direction lengths in [0.5, 2).
    Times: exactly 0.0, exactly 1.0 and nextafter(1, 0), one eighth each, else uniform in [0, 1). Never outside
    [0, 1]: there a moving sphere leaves its boundingBox and the reference's own tree culls it."""
    rng = np.random.default_rng(seed)
    idx = np.arange(n)
    tm = rng.uniform(0.0, 1.0, n)
    sel = (idx // 8) % 8
    tm[sel == 0] = 0.0
    tm[sel == 1] = 1.0
    tm[sel == 2] = np.nextafter(1.0, 0.0)
    by_kind = {}
    for j, lf in enumerate(z.leaves):
        by_kind.setdefault(lf[0], []).append(j)
    kinds = sorted(by_kind)
    pick = np.array([by_kind[kinds[a]][b % len(by_kind[kinds[a]])]
                     for a, b in zip(rng.integers(0, len(kinds), n), rng.integers(0, 1 << 20, n))])
    c0 = np.array([lf[1] for lf in z.leaves])[pick]
    c1 = np.array([lf[2] for lf in z.leaves])[pick]
    half = np.array([lf[3] for lf in z.leaves])[pick]
    target = c0 + tm[:, None] * (c1 - c0) + rng.uniform(-0.6, 0.6, (n, 3)) * half[:, None]
    # from outside, above the floor
    u = rng.normal(0, 1, (n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    u[:, 1] = np.abs(u[:, 1]) + 0.35
    o = target + 40.0 * u
    d = (target - o) * rng.uniform(0.5, 2.0, (n, 1)) / 40.0
    # from inside
    inside = np.array([lf[1] for lf in z.leaves if lf[4]] or [lf[1] for lf in z.leaves])
    m = np.flatnonzero(idx % 8 >= 6)
    o[m] = inside[rng.integers(0, len(inside), len(m))] + rng.normal(0, 1.5, (len(m), 3))
    d[m] = target[m] - o[m]
    free = m[::2]
    d[free] = rng.normal(0, 1, (len(free), 3))
    # axis-aligned
    m = np.flatnonzero(idx % 8 == 0)
    ax = rng.integers(0, 3, len(m))
    sg = rng.choice([-1.0, 1.0], len(m))
    o[m] = target[m]
    o[m, ax] -= 30.0 * sg
    d[m] = 0.0
    d[m, ax] = sg
    return np.ascontiguousarray(np.concatenate([o, d, tm[:, None]], axis=1))


def kind_counts(z, hits):
    """Closest hits per kind: {label: rays whose closest hit has that kind's material}."""
    got = hits[hits[:, 0] == 1][:, 11].astype(np.int64)
    cnt = np.bincount(got, minlength=int(z.scene.desc.n_materials))
    return {label: int(cnt[m]) for label, m in z.kinds.items()}
