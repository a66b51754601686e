"""Far-origin and tangent rays: worlds, ray families, the host model of the default walk's box culls and an
extended-precision judge of single ray / leaf pairs (tests/test_far_rays_host.py, tests/test_gpu_far_rays.py).

Every other closest-hit test starts its rays within a few dozen units of what they hit. Here every ray is
o = target - S * d^ with S on the rungs 2^4 .. 2^44, so the terms that exist only for distant origins are
exercised: the K = max|o * (1/d)| slack of the fp32 child-box test and of the pop cull, the 2^-48 band of the
fp64 joint slab filter, and the pad of the tight Rotate culling box (flat_box, rt_bvh.cpp).

A *path* describes one leaf of a tree: the Translate / Rotate records of the instance frames above it
(outermost first), the leaf's own top node (a primitive or a Translate / Rotate chain over one), the primitive,
and every BVH box above it with the number of frame records that apply to a ray before that box is tested.
"""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import mpmath
import numpy as np

import pyoracle
import rtamd
import test_box_fastpath as bf

RUNGS = tuple(2.0 ** k for k in (4, 12, 20, 28, 36, 44))
FAMILIES = ("aimed", "corner", "tangent", "axis")
PER = 2048           # rays per (family, rung)
T_MIN = 1e-4
WORLDS = ("chains", "frames", "lattice", "rot_grid")
EXACT_COLS = [0, 5, 6, 7, 10, 11]  # hit, normal, front face, material
_XFORM = (rtamd.RT_NODE_TRANSLATE, rtamd.RT_NODE_ROTATE)
_SPHERES = (rtamd.RT_NODE_SPHERE, rtamd.RT_NODE_MOVING_SPHERE)
_RECTS = (rtamd.RT_NODE_RECT_XY, rtamd.RT_NODE_RECT_XZ, rtamd.RT_NODE_RECT_YZ)
_PRIMS = _SPHERES + _RECTS + (rtamd.RT_NODE_CUBOID,)


# ----------------------------------------------------------------------------- worlds
class World:
    """`scene`, `name`, `kinds` (label -> material id: the leaf kinds whose hits are counted)."""


def _rot_grid():
    """20 leaves translate(c, rotate(ax, 10 + 7k degrees, cuboid +-(1, .8, .6))) on a 5 x 4 grid, ax cycling
    X, Y, Z, then four plain spheres and four plain cuboids; every leaf has a material of its own."""
    b = rtamd.Builder(rtamd.randGen(29))
    kinds, items = {}, []

    def mat(label):
        i = len(kinds)
        kinds[label] = b.lambertian(b.constantColor(0.2 + 0.03 * i, 0.5, 0.9 - 0.03 * i))
        return kinds[label]

    for k in range(20):
        c = (4.0 * (k % 5) - 8.0, 0.0, 4.0 * (k // 5) - 6.0)
        box = b.cuboid((-1.0, -0.8, -0.6), (1.0, 0.8, 0.6), mat(f"t_r{'xyz'[k % 3]}_cuboid_{k}"))
        items.append(b.translate(c, b.rotate(k % 3, 10.0 + 7.0 * k, box)))
    for k in range(4):
        items.append(b.sphere((4.0 * k - 6.0, 0.0, 10.0), 1.0, mat(f"sphere_{k}")))
        c = (4.0 * k - 6.0, 0.0, -10.0)
        items.append(b.cuboid((c[0] - 1.0, -0.8, c[2] - 0.6), (c[0] + 1.0, 0.8, c[2] + 0.6), mat(f"cuboid_{k}")))
    return b.finish(b.makeBVH((0.0, 1.0), items), -1, (0.7, 0.8, 0.9)), kinds


@functools.lru_cache(maxsize=None)
def world(name):
    """The named world. Cached: tests share one instance and leave it unchanged."""
    w = World()
    w.name = name
    if name in ("chains", "frames"):
        import zoo_worlds
        z = zoo_worlds.build(name)
        w.scene, w.kinds = z.scene, dict(z.kinds)
    elif name == "lattice":
        import test_gpu_packed_keys
        w.scene = test_gpu_packed_keys._lattice_world()[0]
        nodes = w.scene.nodes
        sph = nodes[nodes["type"] == rtamd.RT_NODE_SPHERE]
        w.kinds = {"lattice_sphere": int(sph["a"][sph["f"][:, 3] < 1.0][0]),
                   "ground_sphere": int(sph["a"][sph["f"][:, 3] > 1.0][0])}
    elif name == "rot_grid":
        w.scene, w.kinds = _rot_grid()
    else:
        raise KeyError(name)
    return w


def kind_counts(w, hits):
    got = hits[hits[:, 0] == 1][:, 11].astype(np.int64)
    cnt = np.bincount(got, minlength=int(w.scene.desc.n_materials))
    return {label: int(cnt[m]) for label, m in w.kinds.items()}


# ----------------------------------------------------------------------------- paths
class Path:
    """One leaf: `frames` (Translate / Rotate records above it, outermost first), `top` (node id of the
    leaf in its tree), `chain` (the leaf's own Translate / Rotate records, outermost first), `prim` (node
    id), `mat`, `boxes` ([(six doubles, frame records applied before it)], root first)."""


def _rec(nd):
    return (int(nd["type"]), [float(x) for x in nd["f"][:3]], int(nd["b"]))


def leaf_paths(scene):
    nodes = scene.nodes
    out = []

    def go(i, frames, boxes):
        t = int(nodes[i]["type"])
        if t == rtamd.RT_NODE_BVH:
            mine = boxes + [(np.array(nodes[i]["f"][:6], dtype=np.float64), len(frames))]
            for ch in sorted({int(nodes[i]["a"]), int(nodes[i]["b"])}):
                go(ch, frames, mine)
            return
        chain, j = [], i
        while int(nodes[j]["type"]) in _XFORM:
            chain.append(_rec(nodes[j]))
            j = int(nodes[j]["a"])
        tj = int(nodes[j]["type"])
        if tj == rtamd.RT_NODE_BVH:  # an instance frame
            return go(j, frames + chain, boxes)
        if tj not in _PRIMS:
            raise ValueError(f"node {j}: kind {tj} is not handled")
        p = Path()
        p.frames, p.top, p.chain, p.prim, p.mat, p.boxes = frames, i, chain, j, int(nodes[j]["a"]), boxes
        p.kind = tj
        out.append(p)
    go(scene.desc.world_root, [], [])
    return out


def _unrot(ax, s, c, p):
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    if ax == 0:
        return np.stack([x, c * y + s * z, -s * y + c * z], axis=-1)
    if ax == 1:
        return np.stack([c * x - s * z, y, s * x + c * z], axis=-1)
    return np.stack([c * x + s * y, -s * x + c * y, z], axis=-1)


def _rot(ax, s, c, p):
    return _unrot(ax, -s, c, p)


def into(records, o, d):
    """The ray carried into the coordinates below `records` in fp64, as hit does (oracle.c: vsub,
    unrotate_point of origin and direction; no contraction)."""
    for t, f, ax in records:
        if t == rtamd.RT_NODE_TRANSLATE:
            o = o - np.array(f)
        else:
            o, d = _unrot(ax, f[0], f[1], o), _unrot(ax, f[0], f[1], d)
    return o, d


def _out_of(records, p):
    for t, f, ax in records[::-1]:
        p = p + np.array(f) if t == rtamd.RT_NODE_TRANSLATE else _rot(ax, f[0], f[1], p)
    return p


def _with_root(scene, root):
    d = rtamd.rt_scene_desc()
    C.pointer(d)[0] = scene.desc
    d.world_root = root
    s = rtamd.Scene(scene._builder, d)
    s._keep = scene
    return s


def hit_leaves(scene, paths, rays, hits):
    """Index into `paths` of the leaf each hit came from (-1: no hit): the leaf with the hit's material
    that, walked alone by the oracle with the ray carried into its frame, returns the same t and, carried
    back out of the frame, the same normal."""
    out = np.full(len(rays), -1)
    for k, p in enumerate(paths):
        m = np.flatnonzero((hits[:, 0] == 1) & (hits[:, 11] == p.mat) & (out < 0))
        if not len(m):
            continue
        o, d = into(p.frames, rays[m, 0:3], rays[m, 3:6])
        sub = np.ascontiguousarray(np.concatenate([o, d, rays[m, 6:7]], axis=1))
        h = pyoracle.closest_hits(_with_root(scene, p.top), sub, T_MIN, np.inf, seed=3)
        same = (h[:, 0] == 1) & (h[:, 1] == hits[m, 1])
        nrm = h[:, 5:8]  # (two spheres can report one t for a far origin: the normal tells them apart)
        for t, f, ax in p.frames[::-1]:
            if t == rtamd.RT_NODE_ROTATE:
                nrm = _rot(ax, f[0], f[1], nrm)
        same &= np.all(nrm == hits[m, 5:8], axis=1)
        out[m[same]] = k
    assert np.all((out >= 0) == (hits[:, 0] == 1)), "a hit whose leaf was not found"
    return out


@functools.lru_cache(maxsize=None)
def _rebuilt(scene):
    rb = rtamd.rebuilt_scene(scene)
    return rb, leaf_paths(rb)


def predicted_culls(scene, rays, ref_hits):
    """The host model of the default upload's walk: True for every ray whose reference hit lies in a leaf
    with an ancestor box, in the tree the device walks (rtamd.rebuilt_scene), that the device's joint box
    test (test_box_fastpath.exact) rejects. Such a hit is one the default walk is predicted to lose."""
    rb, paths = _rebuilt(scene)
    leaf = hit_leaves(rb, paths, rays, ref_hits)
    lost = np.zeros(len(rays), dtype=bool)
    for k, p in enumerate(paths):
        m = np.flatnonzero(leaf == k)
        if not len(m):
            continue
        for box, depth in p.boxes:
            o, d = into(p.frames[:depth], rays[m, 0:3], rays[m, 3:6])
            n = len(m)
            ok = bf.exact(np.tile(box[:3], (n, 1)), np.tile(box[3:], (n, 1)), o, d, np.full(n, T_MIN),
                          np.full(n, np.inf))
            lost[m[~ok]] = True
    return lost


# ----------------------------------------------------------------------------- the exact judge
PREC = 200
RIM = 2.0 ** -50  # of the largest origin coordinate in the leaf's frame: 4 ulps of it


def _mp3(v):
    return [mpmath.mpf(float(x)) for x in v]


def exact_judge(scene, ray, path):
    """Does the exact ray meet the exact primitive of `path` at some t >= T_MIN? 200-bit arithmetic on the
    stored doubles taken as exact (a Rotate's stored sine and cosine included), the ray carried exactly
    through the frames and the leaf's chain."""
    return exact_t(scene, ray, path) is not None


def exact_t(scene, ray, path):
    """exact_judge's answer as the parameter of the meeting that the leaf test reports when it computes
    exactly (a sphere's first root beyond T_MIN, the nearest face of a cuboid), or None. A meeting within RIM
    of the leaf's rim (a rect's edges, a sphere's silhouette) does not count: the leaf test forms o + t d with
    an error of a few ulps of |o|, so whether it takes such a hit is decided by rounding, and the joint slab
    filter, which intersects the same slabs in another order, may decide otherwise (rt_trace.h box_hit_exact:
    it prunes hits on a box face)."""
    nodes = scene.nodes
    with mpmath.workprec(PREC):
        o, d, tm = _mp3(ray[0:3]), _mp3(ray[3:6]), mpmath.mpf(float(ray[6]))
        for t, f, ax in path.frames + path.chain:
            g = _mp3(f)
            if t == rtamd.RT_NODE_TRANSLATE:
                o = [o[a] - g[a] for a in range(3)]
            else:
                s, c = g[0], g[1]
                i, j = [(1, 2), (2, 0), (0, 1)][ax]  # the rotated pair, in the order of unrotate_point
                for v in (o, d):
                    v[i], v[j] = c * v[i] + s * v[j], -s * v[i] + c * v[j]
        rim = RIM * max(abs(x) for x in o)
        nd = nodes[path.prim]
        f = _mp3(nd["f"])
        kind = int(nd["type"])
        tmin = mpmath.mpf(T_MIN)
        if kind in _SPHERES:
            if kind == rtamd.RT_NODE_SPHERE:
                cen, rad = f[0:3], f[3]
            else:
                e = _mp3(nodes[path.prim + 1]["f"][:4])
                cen, rad = [f[a] + (tm - e[0]) / e[2] * (f[3 + a] - f[a]) for a in range(3)], e[3]
            oc = [o[a] - cen[a] for a in range(3)]
            aa = sum(x * x for x in d)
            bb = sum(x * y for x, y in zip(oc, d))
            cc = sum(x * x for x in oc) - rad * rad
            disc = bb * bb - aa * cc
            if disc < 0 or (-bb + mpmath.sqrt(disc)) / aa < tmin:
                return None
            if rad - mpmath.sqrt(max(0, cc + rad * rad - bb * bb / aa)) < rim:  # (grazing within the rim)
                return None
            t1 = (-bb - mpmath.sqrt(disc)) / aa
            return t1 if t1 >= tmin else (-bb + mpmath.sqrt(disc)) / aa
        if kind in _RECTS:
            faces = [(kind - rtamd.RT_NODE_RECT_XY, f[0], f[1], f[2], f[3], f[4])]
        elif kind == rtamd.RT_NODE_CUBOID:
            faces = [(0, f[0], f[3], f[1], f[4], f[5]), (0, f[0], f[3], f[1], f[4], f[2]),
                     (1, f[0], f[3], f[2], f[5], f[4]), (1, f[0], f[3], f[2], f[5], f[1]),
                     (2, f[1], f[4], f[2], f[5], f[3]), (2, f[1], f[4], f[2], f[5], f[0])]
        else:
            raise ValueError(f"kind {kind} is not handled")
        best = None
        for plane, i0, i1, j0, j1, k in faces:
            ia, ja, ka = [(0, 1, 2), (0, 2, 1), (1, 2, 0)][plane]
            if d[ka] == 0:
                if o[ka] == k:
                    raise ValueError("ray inside a rect's plane")
                continue
            t = (k - o[ka]) / d[ka]
            if t >= tmin and i0 + rim <= o[ia] + t * d[ia] <= i1 - rim and j0 + rim <= o[ja] + t * d[ja] <= j1 - rim:
                best = t if best is None or t < best else best
        return best


PLACED = 2.0 ** -40  # relative; a leaf test's own rounding on a well-conditioned hit is a few 2^-52


def genuine(scene, ray, path, t):
    """Is the hit that a walk reports on this leaf at parameter t one that exact arithmetic makes too? The
    exact ray meets the exact leaf (exact_judge), and t is within PLACED of where it does. For a far origin
    the sphere test's c = |o - c|^2 - r^2 loses r^2 and its discriminant cancels, so it reports hits on
    spheres the exact ray misses (by up to |o - c|^2 * 2^-52 / r) and, on spheres it meets, at points
    hundreds of radii away from them; either is a hit made by rounding."""
    te = exact_t(scene, ray, path)
    if te is None:
        return False
    with mpmath.workprec(PREC):
        return bool(abs(mpmath.mpf(float(t)) - te) <= PLACED * abs(te))


def artefacts(scene, paths, rays, a, b, rows):
    """The rays `rows`, whose closest hits a (the reference side: the oracle over the caller's tree) and b
    (the side under test), over trees with the leaves of `paths`, differ, sorted into
      artefacts       a hit that either side reports is not genuine: made or placed by rounding;
      reference_lost  every reported hit is genuine and b's is the nearer (or a has none): the reference's own
                      box test dropped a hit, as it does beyond |o| = 2^40, where the +-1e-4 box of a rect
                      collapses to one quotient and `tmax > tmin` fails;
      real            every reported hit is genuine and b reports the farther one, none, or the same leaf
                      with other numbers: b lost or changed a hit that exact arithmetic makes.
    Returns (real, reference_lost) as lists of row numbers."""
    la = hit_leaves(scene, paths, rays[rows], a[rows])
    lb = hit_leaves(scene, paths, rays[rows], b[rows])
    real, ref_lost = [], []
    for r, i, j in zip(rows, la, lb):
        sides = [(int(k), h[r, 1]) for k, h in ((i, a), (j, b)) if k >= 0]
        if i != j and not all(genuine(scene, rays[r], paths[k], t) for k, t in sides):
            continue
        if i != j and j >= 0 and (i < 0 or b[r, 1] < a[r, 1]):
            ref_lost.append(int(r))
        else:
            real.append(int(r))
    return real, ref_lost


def differing(got, ref):
    """Rows that differ by test_closest_hits_per_kind's rules for surface hits: the exact columns equal, t and
    p bit-identical (u, v are compared apart: 4e-16, NaN where the oracle has NaN)."""
    return ~np.all(got[:, EXACT_COLS] == ref[:, EXACT_COLS], axis=1) | ~np.all(got[:, 1:5] == ref[:, 1:5], axis=1)


# ----------------------------------------------------------------------------- rays
def _targets(name):
    """Per leaf of the world: centre at times 0 and 1 and half extents of its world-space box (spheres: centre
    +- r, so the box's face centres are the sphere's extremal points), and its material."""
    sc = world(name).scene
    nodes = sc.nodes
    c0, c1, half, mats = [], [], [], []
    for p in leaf_paths(sc):
        f = np.array(nodes[p.prim]["f"], dtype=np.float64)
        recs = p.frames + p.chain
        if p.kind in _SPHERES:
            a, b = f[0:3], (f[3:6] if p.kind == rtamd.RT_NODE_MOVING_SPHERE else f[0:3])
            r = float(nodes[p.prim + 1]["f"][3]) if p.kind == rtamd.RT_NODE_MOVING_SPHERE else f[3]
            c0.append(_out_of(recs, a))
            c1.append(_out_of(recs, b))
            half.append(np.full(3, r))
        else:
            if p.kind == rtamd.RT_NODE_CUBOID:
                lo, hi = f[0:3], f[3:6]
            else:
                ia, ja, ka = [(0, 1, 2), (0, 2, 1), (1, 2, 0)][p.kind - rtamd.RT_NODE_RECT_XY]
                lo, hi = np.zeros(3), np.zeros(3)
                lo[ia], hi[ia], lo[ja], hi[ja], lo[ka], hi[ka] = f[0], f[1], f[2], f[3], f[4], f[4]
            corners = np.array([[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[k][2]] for i in (0, 1) for j in (0, 1)
                                for k in (0, 1)])
            q = _out_of(recs, corners)
            c0.append((q.min(0) + q.max(0)) / 2)
            c1.append(c0[-1])
            half.append((q.max(0) - q.min(0)) / 2)
        mats.append(p.mat)
    return np.array(c0), np.array(c1), np.array(half), np.array(mats)


def _unit(rng, n):
    u = rng.normal(0, 1, (n, 3))
    return u / np.linalg.norm(u, axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def rays(name):
    """(rays, family index, rung index) for the world: PER rays per (family, rung), family-major, from a fixed
    seed. Every ray is o = target - S * d^, its direction then scaled by 2^-20 (a quarter) or 2^20 (another).
    Leaves are drawn uniformly by material, then uniformly among that material's leaves.
      aimed    target = a jittered leaf centre, random direction
      corner   target within +-10^U(-13, -3) per component of a corner or a face centre (a sphere's extremal
               point) of the leaf's world-space box, random direction
      tangent  target as corner's, on the +-a face of the box and offset along a only; d[a] in {0, -0, +-1e-12,
               +-1e-9} before normalisation, the other two components random: all three axes, both sides
      axis     two exact zero components (zeros of both signs), both directions, at a jittered leaf centre"""
    c0, c1, half, mats = _targets(name)
    rng = np.random.default_rng(4404)
    by_mat = {}
    for j, m in enumerate(mats):
        by_mat.setdefault(int(m), []).append(j)
    keys = sorted(by_mat)
    out, fam, rung = [], [], []
    for fi, family in enumerate(FAMILIES):
        for ri, S in enumerate(RUNGS):
            n = PER
            pick = np.array([by_mat[keys[a]][b % len(by_mat[keys[a]])]
                             for a, b in zip(rng.integers(0, len(keys), n), rng.integers(0, 1 << 20, n))])
            tm = rng.uniform(0.0, 1.0, n)
            cen = c0[pick] + tm[:, None] * (c1[pick] - c0[pick])
            h = half[pick]
            hj = np.maximum(h, 0.05)  # (off a rect's own plane: a ray inside it has t = 0 / 0)
            d = _unit(rng, n)
            eps = rng.choice([-1.0, 1.0], (n, 3)) * 10.0 ** rng.uniform(-13, -3, (n, 3))
            if family == "aimed":
                target = cen + rng.uniform(-0.6, 0.6, (n, 3)) * hj
            elif family == "corner":
                sg = rng.choice([-1.0, 1.0], (n, 3))
                face = rng.random(n) < 0.5          # a face centre: one axis at its extreme, the others central
                keep = rng.integers(0, 3, n)
                sg[face] *= np.eye(3)[keep[face]]
                target = cen + sg * h + eps
            elif family == "tangent":
                a = np.arange(n) % 3
                sg = rng.choice([-1.0, 1.0], (n, 3))
                face = rng.random(n) < 0.5
                sg[face] *= np.eye(3)[a[face]]
                sg[np.arange(n), a] = np.where((np.arange(n) // 3) % 2 == 0, 1.0, -1.0)
                target = cen + sg * h
                target[np.arange(n), a] += eps[np.arange(n), a]
                d[np.arange(n), a] = rng.choice([0.0, -0.0, 1e-12, -1e-12, 1e-9, -1e-9], n)
                d /= np.linalg.norm(d, axis=1, keepdims=True)
            else:
                target = cen + rng.uniform(-0.6, 0.6, (n, 3)) * hj
                ax = rng.integers(0, 3, n)
                d = rng.choice([0.0, -0.0], (n, 3))
                d[np.arange(n), ax] = rng.choice([-1.0, 1.0], n)
            o = target - S * d
            sc = np.ones(n)
            sc[0::4] = 2.0 ** -20
            sc[1::4] = 2.0 ** 20
            out.append(np.concatenate([o, d * sc[:, None], tm[:, None]], axis=1))
            fam.append(np.full(n, fi))
            rung.append(np.full(n, ri))
    r = np.ascontiguousarray(np.concatenate(out))
    r.setflags(write=False)
    return r, np.concatenate(fam), np.concatenate(rung)


@functools.lru_cache(maxsize=None)
def oracle_hits(name):
    """The oracle's closest hits over the caller's tree. Cached and read-only."""
    ref = pyoracle.closest_hits(world(name).scene, rays(name)[0], T_MIN, np.inf, seed=3)
    ref.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def trees_differ(name):
    """Rays on which the oracle over the tree the device walks differs from the oracle over the caller's tree:
    with the reference's own box test on both, the two trees do not hold the same closest hit."""
    a = oracle_hits(name)
    b = pyoracle.closest_hits(_rebuilt(world(name).scene)[0], rays(name)[0], T_MIN, np.inf, seed=3)
    return ~np.all((a == b) | (np.isnan(a) & np.isnan(b)), axis=1)


@functools.lru_cache(maxsize=None)
def predicted(name):
    """predicted_culls per ray, and the hit leaf's class per ray (hit_classes)."""
    r = rays(name)[0]
    sc = world(name).scene
    return predicted_culls(sc, r, oracle_hits(name)), hit_classes(sc, r, oracle_hits(name))


NO_HIT, SPHERE, ROTATED, PLAIN = 0, 1, 2, 3


def hit_classes(scene, rays, hits):
    """Per ray, what its hit's leaf is: a sphere (moving or not: the leaf test that loses r^2 against |o - c|^2
    for a far origin), a rect or cuboid below a Rotate (its own chain's or an instance frame's: a tight
    Rotate box bounds it), or a plain rect or cuboid."""
    rb, paths = _rebuilt(scene)
    leaf = hit_leaves(rb, paths, rays, hits)
    cls = np.array([SPHERE if p.kind in _SPHERES else
                    ROTATED if any(t == rtamd.RT_NODE_ROTATE for t, _, _ in p.frames + p.chain) else PLAIN
                    for p in paths] + [NO_HIT])
    return cls[leaf]


def cull_table(mask, fam, rung):
    return [[int(mask[(fam == fi) & (rung == ri)].sum()) for ri in range(len(RUNGS))] for fi in range(len(FAMILIES))]


def predicted_in_child(name, env):
    """predicted(name)'s mask from a fresh process with `env` added (RTAMD_TIGHT_ROTATE is read once per
    process)."""
    e = dict(os.environ)
    e.update(env)
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    e["PYTHONPATH"] = os.pathsep.join([here, os.path.join(root, "ray-tracing_amd"), os.path.join(root, "oracle")]
                                      + ([e["PYTHONPATH"]] if e.get("PYTHONPATH") else []))
    code = f"import far_rays, json; print(json.dumps(far_rays.predicted({name!r})[0].nonzero()[0].tolist()))"
    out = subprocess.run([sys.executable, "-c", code], env=e, check=True, capture_output=True, text=True).stdout
    mask = np.zeros(len(rays(name)[0]), dtype=bool)
    mask[json.loads(out.strip().splitlines()[-1])] = True
    return mask
