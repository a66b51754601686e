"""Builder-made worlds (tests/zoo_worlds.py), host side: the C++ constructors against the restatement on X / Z
rotations and nested chains, the kernels each world was designed to select, the SAH rebuild against the
caller's tree on every leaf kind, and the 4-wide trees' fp32 boxes against the leaves' surfaces in extended
precision (tests/test_gpu_zoo.py runs the same worlds on the device)."""
import functools

import mpmath
import numpy as np
import pytest

import pyoracle
import rtamd
import scenes_ref
import zoo_worlds

F_RECT, F_MOVING, F_INST, F_MEDIA, F_LIGHTS, F_TEX, F_FRAMES = 1, 2, 4, 8, 16, 32, 512
# rt_layout.h: kVarCornell = F_RECT | F_INST | F_LIGHTS, kVarFullDark = (F_ALL & ~F_LIGHTS) | F_MIXW, kVarFull
K_VAR_CORNELL, K_VAR_FULL_DARK, K_VAR_FULL = 21, 1583, 1599
# (a MovingSphere's payload record counts as "anything needing the full dispatch": F_RECT)
DESIGN = {
    "chains": dict(features=F_RECT | F_INST | F_LIGHTS, variant=K_VAR_CORNELL, rebuilt_bvh=1, mixed_wide=0,
                   ref_walk=0, replace_ok=1),
    "moving": dict(features=F_RECT | F_MOVING | F_INST | F_TEX, variant=K_VAR_FULL_DARK, rebuilt_bvh=1, mixed_wide=0,
                   ref_walk=0, replace_ok=1),
    "frames": dict(features=F_RECT | F_MOVING | F_INST | F_LIGHTS | F_FRAMES, variant=K_VAR_FULL, rebuilt_bvh=1,
                   mixed_wide=1, ref_walk=1, replace_ok=1),
    "media": dict(features=F_RECT | F_MOVING | F_INST | F_MEDIA | F_FRAMES, variant=K_VAR_FULL_DARK, rebuilt_bvh=1,
                  mixed_wide=1, ref_walk=1, replace_ok=1),
}


@pytest.mark.parametrize("name", zoo_worlds.NAMES)
def test_builder_matches_restatement(name):
    """rt_obj_* against oracle/scenes_ref.py's constructors: the world, the lights tree, the generator after
    construction and the camera, bit for bit (test_scenes.py's contract, on rotations about every axis,
    rotate(translate(rotate(.))) chains, moving spheres under chains and nested frames)."""
    z = zoo_worlds.build(name)
    world, lights, bg, g1 = zoo_worlds.restate(name)
    assert z.g1 == g1, "generator after construction differs"
    assert scenes_ref.canon_desc(z.scene) == scenes_ref.canon(world)
    if lights is None:
        assert z.scene.desc.lights_root == -1
    else:
        assert scenes_ref.canon_desc(z.scene, z.scene.desc.lights_root) == scenes_ref.canon(lights)
    assert tuple(z.scene.desc.background) == tuple(float(x) for x in bg)
    ref = zoo_worlds.camera_restated(name)
    for k in ("origin", "llc", "horiz", "vert", "u", "v", "w"):
        assert tuple(getattr(z.camera, k)) == tuple(float(x) for x in ref[k]), k
    assert z.camera.lens_radius == ref["lens_radius"]
    root = z.scene.nodes[z.scene.desc.world_root]
    assert root["type"] == rtamd.RT_NODE_BVH and root["c"] >= 16  # (the SAH rebuild applies)


@pytest.mark.parametrize("name", zoo_worlds.NAMES)
def test_worlds_select_the_intended_kernels(name):
    info = rtamd.prepare_scene(zoo_worlds.build(name).scene)
    assert {k: info[k] for k in DESIGN[name]} == DESIGN[name]


def test_worlds_hold_every_axis():
    """What the worlds are for: Rotate nodes about each axis over a primitive (chains) and over a BVH
    (frames), and every leaf kind below a chain."""
    def rotations(name, over_bvh):
        nodes = zoo_worlds.build(name).scene.nodes
        out = set()
        for nd in nodes[nodes["type"] == rtamd.RT_NODE_ROTATE]:
            ch = int(nd["a"])
            while nodes[ch]["type"] in (rtamd.RT_NODE_TRANSLATE, rtamd.RT_NODE_ROTATE):
                ch = int(nodes[ch]["a"])
            if (nodes[ch]["type"] == rtamd.RT_NODE_BVH) == over_bvh:
                out.add((int(nd["b"]), int(nodes[ch]["type"])))
        return out
    ch = rotations("chains", False)
    assert {(a, rtamd.RT_NODE_CUBOID) for a in range(3)} <= ch
    assert {(0, rtamd.RT_NODE_RECT_XZ), (1, rtamd.RT_NODE_RECT_XY), (2, rtamd.RT_NODE_RECT_YZ)} <= ch
    assert {(a, rtamd.RT_NODE_MOVING_SPHERE) for a in range(3)} <= rotations("moving", False)
    assert {a for a, _ in rotations("frames", True)} == {0, 2}


@functools.lru_cache(maxsize=None)
def _oracle_hits(name):
    z = zoo_worlds.build(name)
    rays = zoo_worlds.rays(z)
    return rays, pyoracle.closest_hits(z.scene, rays, 1e-4, np.inf, seed=3)


@pytest.mark.parametrize("name", zoo_worlds.NAMES)
def test_rebuilt_tree_gives_identical_closest_hits(name):
    """The oracle's closest hits over the caller's tree and over the tree the device walks (rt_rebuild_bvh:
    tight rotated boxes, re-bounded frames, hoisted media) on 2^14 rays; every kind of object is the closest
    hit of at least 100 of them."""
    z = zoo_worlds.build(name)
    rays, a = _oracle_hits(name)
    assert len(rays) == 1 << 14 and rays[:, 6].min() == 0.0 and rays[:, 6].max() == 1.0
    counts = zoo_worlds.kind_counts(z, a)
    print(f"{name}: oracle closest hits per kind {counts}")
    assert min(counts.values()) >= 100, counts
    rb = rtamd.rebuilt_scene(z.scene)
    assert rb.desc.world_root != z.scene.desc.world_root
    b = pyoracle.closest_hits(rb, rays, 1e-4, np.inf, seed=3)
    assert np.array_equal(a, b, equal_nan=True)


# ----------------------------------------------------------------------------- containment
PREC = 256  # bits (products and sums of a few doubles: exact)
_DIRS = np.random.default_rng(23).normal(0, 1, (24, 3))
_DIRS /= np.linalg.norm(_DIRS, axis=1, keepdims=True) * (1 + 2.0 ** -40)  # (inside the unit sphere)
_TIMES = (0.0, 1.0, 0.5, 0.123, float(np.nextafter(1.0, 0.0)))
_PRIMS = (rtamd.RT_NODE_SPHERE, rtamd.RT_NODE_MOVING_SPHERE, rtamd.RT_NODE_RECT_XY, rtamd.RT_NODE_RECT_XZ,
          rtamd.RT_NODE_RECT_YZ, rtamd.RT_NODE_CUBOID, rtamd.RT_NODE_BVH)


def _mp(v):
    return [mpmath.mpf(float(x)) for x in v]


def _surface_points(nodes, leaf):
    """Points of the leaf's surface in the coordinates of the tree that holds it, in extended precision.
    Sphere: 24 sampled directions and the six axis extremes; moving sphere: the same at five times; rect: its
    corners; cuboid (and the BVH inside an instance frame: its box): its corners; a medium: its boundary's.
    Carried through the leaf's Translate / Rotate chain, innermost first."""
    chain = []
    i = leaf
    while True:
        nd = nodes[i]
        t = int(nd["type"])
        if t == rtamd.RT_NODE_CONSTANT_MEDIUM:
            i = int(nd["a"])
        elif t in (rtamd.RT_NODE_TRANSLATE, rtamd.RT_NODE_ROTATE):
            chain.append(nd)
            i = int(nd["a"])
        else:
            break
    assert t in _PRIMS, t
    f = _mp(nd["f"])
    pts = []
    if t in (rtamd.RT_NODE_SPHERE, rtamd.RT_NODE_MOVING_SPHERE):
        if t == rtamd.RT_NODE_SPHERE:
            centres, rad = [f[0:3]], f[3]
        else:
            t0, t1, _, rad = _mp(nodes[i + 1]["f"][:4])
            centres = [[f[a] + (mpmath.mpf(tm) - t0) / (t1 - t0) * (f[3 + a] - f[a]) for a in range(3)] for tm in _TIMES]
        dirs = [_mp(d) for d in _DIRS] + [_mp(s * e) for e in np.eye(3) for s in (-1.0, 1.0)]
        pts = [[c[a] + rad * d[a] for a in range(3)] for c in centres for d in dirs]
    elif t in (rtamd.RT_NODE_CUBOID, rtamd.RT_NODE_BVH):
        pts = [[f[3 * i0], f[1 + 3 * i1], f[2 + 3 * i2]] for i0 in (0, 1) for i1 in (0, 1) for i2 in (0, 1)]
    else:
        for a in (f[0], f[1]):
            for b in (f[2], f[3]):
                pts.append({rtamd.RT_NODE_RECT_XY: [a, b, f[4]], rtamd.RT_NODE_RECT_XZ: [a, f[4], b],
                            rtamd.RT_NODE_RECT_YZ: [f[4], a, b]}[t])
    for nd in chain[::-1]:
        g = _mp(nd["f"])
        if int(nd["type"]) == rtamd.RT_NODE_TRANSLATE:
            pts = [[p[a] + g[a] for a in range(3)] for p in pts]
        else:
            s, c, ax = g[0], g[1], int(nd["b"])
            if ax == 0:
                pts = [[x, c * y - s * z, s * y + c * z] for x, y, z in pts]
            elif ax == 1:
                pts = [[c * x + s * z, y, -s * x + c * z] for x, y, z in pts]
            else:
                pts = [[c * x - s * y, s * x + c * y, z] for x, y, z in pts]
    return t, pts


def _check_containment(scene, root=None):
    """Every leaf of the 4-wide tree at `root`: its surface inside its own fp32 box and inside every
    ancestor's. Returns (leaves by primitive type, smallest slack)."""
    nodes = scene.nodes
    wide, _ = rtamd.wide_bvh(scene, root)
    seen = {}
    slack = [mpmath.inf]
    with mpmath.workprec(PREC):
        _walk_wide(nodes, wide, 0, [], seen, slack)
    return seen, slack[0]


def _walk_wide(nodes, wide, w, boxes, seen, slack):
    for k in range(4):
        lo, hi = wide[w]["lo"][:, k], wide[w]["hi"][:, k]
        if np.any(lo > hi):
            continue
        mine = boxes + [(_mp(lo), _mp(hi))]
        c = int(wide[w]["child"][k])
        if c >= 0:
            _walk_wide(nodes, wide, c, mine, seen, slack)
            continue
        t, pts = _surface_points(nodes, ~c)
        seen[t] = seen.get(t, 0) + 1
        for blo, bhi in mine:
            for p in pts:
                s = min(min(p[a] - blo[a], bhi[a] - p[a]) for a in range(3))
                slack[0] = min(slack[0], s)
                assert s >= 0, f"leaf {~c} (type {t}) leaves an fp32 box by {mpmath.nstr(-s, 5)}"


@pytest.mark.parametrize("name", ["chains", "moving", "frames", "media", "cornell", "random"])
def test_wide_boxes_contain_every_leaf_kind(name):
    """rt_wide_bvh over the rebuilt tree (flat_box's tight rotated box, f32_down / f32_up): spheres, moving
    spheres at five times, rects, cuboids and Translate / Rotate chains on all three axes lie inside their
    leaf's fp32 box and every ancestor's (test_bvh.py checks this for bare spheres only). Worlds with frames:
    the world's tree (a frame's leaf box against the corners of the box inside it) and each frame's own."""
    if name in zoo_worlds.NAMES:
        scene = zoo_worlds.build(name).scene
    else:
        scene, _ = rtamd.make_scene(name, rtamd.randGen(1024))
    rb = rtamd.rebuilt_scene(scene)
    seen, slack = _check_containment(rb)
    roots = zoo_worlds.frame_roots(rb)
    for r in roots:
        s2, sl2 = _check_containment(rb, r)
        slack = min(slack, sl2)
        for t, n in s2.items():
            seen[t] = seen.get(t, 0) + n
    print(f"{name}: leaves by primitive type {dict(sorted(seen.items()))}, {len(roots)} frame trees, smallest slack "
          f"{mpmath.nstr(slack, 5)}")
    want = {"chains": {rtamd.RT_NODE_SPHERE, rtamd.RT_NODE_RECT_XY, rtamd.RT_NODE_RECT_XZ, rtamd.RT_NODE_RECT_YZ,
                       rtamd.RT_NODE_CUBOID},
            "moving": {rtamd.RT_NODE_SPHERE, rtamd.RT_NODE_MOVING_SPHERE},
            "frames": {rtamd.RT_NODE_SPHERE, rtamd.RT_NODE_MOVING_SPHERE, rtamd.RT_NODE_RECT_XY, rtamd.RT_NODE_RECT_XZ,
                       rtamd.RT_NODE_RECT_YZ, rtamd.RT_NODE_CUBOID, rtamd.RT_NODE_BVH},
            "cornell": {rtamd.RT_NODE_SPHERE, rtamd.RT_NODE_RECT_XY, rtamd.RT_NODE_RECT_XZ, rtamd.RT_NODE_RECT_YZ,
                        rtamd.RT_NODE_CUBOID},
            "random": {rtamd.RT_NODE_SPHERE, rtamd.RT_NODE_MOVING_SPHERE, rtamd.RT_NODE_CUBOID}}
    want["media"] = want["frames"]
    assert want[name] <= set(seen)
    assert len(roots) == (2 if name in ("frames", "media") else 0)


# ----------------------------------------------------------------------------- lights validation
def _lights_world(n_lights):
    b = rtamd.Builder(rtamd.randGen(3))
    lam = b.lambertian(b.constantColor(0.5, 0.5, 0.5))
    lit = b.diffuseLight(b.constantColor(4.0, 4.0, 4.0))
    lights = [b.sphere((3.0 * i, 5.0, 0.0), 0.5, lit) for i in range(n_lights)]
    items = [b.sphere((3.0 * i, 0.0, 0.0), 1.0, lam) for i in range(4)] + lights
    return b.finish(b.makeBVH((0.0, 1.0), items), b.makeBVH((0.0, 1.0), lights), (0.0, 0.0, 0.0))


def test_lights_tree_depth_is_validated():
    """makeBVH of up to four lights is two levels deep (RT_LIGHT_DEPTH, the depth htbl_pdf_value unrolls);
    five give a third level, which the upload refuses."""
    for n in (1, 2, 3, 4):
        assert rtamd.prepare_scene(_lights_world(n))["features"] & F_LIGHTS
    with pytest.raises(rtamd.RTError, match=r"\(-4\).*RT_LIGHT_DEPTH"):
        rtamd.prepare_scene(_lights_world(5))
    assert rtamd.RT_E_UNSUPPORTED == -4
