"""Specular-chain feature buffers without a device (include/rt.h rt_render_features_chain): every RT_E_INVALID case
of the two render calls, the device-free plan entry, and the CPU composition the GPU tests compare against
(tests/feature_chain_ref.py) pinned to the oracle's own renderer by a specular-only world."""
import ctypes as C

import numpy as np
import pytest

import feature_chain_ref as fcr
import feature_ref
import pyoracle
import rtamd

CU_COUNT = 256
F_WIDE = 256
BOTH = rtamd.RT_CHAIN_DIELECTRIC | rtamd.RT_CHAIN_METAL


def _call(fn_async, ctx, cam, p, chain, first, n, sums):
    L = rtamd.lib()
    ref = lambda x: C.byref(x) if x is not None else None
    if fn_async:
        rc = L.rt_render_features_chain_async(ctx, ref(cam), ref(p), ref(chain), first, n, 0,
                                              sums.ctypes.data if sums is not None else None, None)
    else:
        rc = L.rt_render_features_chain(ctx, ref(cam), ref(p), ref(chain), first, n, 0,
                                        sums.ctypes.data_as(C.POINTER(C.c_double)) if sums is not None else None)
    return rc, L.rt_last_error().decode()


@pytest.mark.parametrize("fn_async", [False, True], ids=["blocking", "async"])
def test_invalid_arguments_without_a_device(fn_async):
    """Every RT_E_INVALID case is returned before any HIP call: there is no device here and the ctx is null. The
    ctx is checked last, so each case is told by its message, and valid arguments reach that check."""
    cam = rtamd.camera("random_scene", 16, 8)
    sums = np.zeros((8, 16, 8))

    def params(**kw):
        a = dict(width=16, height=8, spp=1, max_depth=1, rng_mode=rtamd.RT_RNG_PHILOX, seed=1, flags=0)
        a.update({k: v for k, v in kw.items() if k in a})
        p = rtamd.make_params(a["width"], a["height"], a["spp"], a["max_depth"], a["rng_mode"], a["seed"], a["flags"])
        p.shard_count = kw.get("shard_count", 1)
        return p

    def chain(max_bounces=8, flags=BOTH, max_fuzz=0.0):
        ch = rtamd.rt_feature_chain()
        ch.max_bounces, ch.flags, ch.max_fuzz = max_bounces, flags, max_fuzz
        return ch

    imax = 2**31 - 1
    ok = chain()
    cases = [
        # the chain's own cases
        ("null argument", (cam, params(), None, 0, 1, sums)),
        ("max_bounces", (cam, params(), chain(max_bounces=-1), 0, 1, sums)),
        ("max_bounces", (cam, params(), chain(max_bounces=65), 0, 1, sums)),
        ("unknown flag bits", (cam, params(), chain(flags=4), 0, 1, sums)),
        ("unknown flag bits", (cam, params(), chain(flags=BOTH | 0x80000000), 0, 1, sums)),
        ("max_fuzz", (cam, params(), chain(max_fuzz=-1e-300), 0, 1, sums)),
        ("max_fuzz", (cam, params(), chain(max_fuzz=float("inf")), 0, 1, sums)),
        ("max_fuzz", (cam, params(), chain(max_fuzz=float("nan")), 0, 1, sums)),
        # everything the first-hit pass rejects
        ("null argument", (None, params(), ok, 0, 1, sums)),
        ("null argument", (cam, None, ok, 0, 1, sums)),
        ("null argument", (cam, params(), ok, 0, 1, None)),
        ("RT_RNG_PHILOX", (cam, params(rng_mode=rtamd.RT_RNG_EXACT), ok, 0, 1, sums)),
        ("RT_FLAG_SHARED_LIBM", (cam, params(flags=rtamd.RT_FLAG_SHARED_LIBM), ok, 0, 1, sums)),
        ("shard_count", (cam, params(shard_count=2), ok, 0, 1, sums)),
        ("first_sample", (cam, params(), ok, -1, 1, sums)),
        ("first_sample", (cam, params(), ok, 0, 0, sums)),
        ("first_sample", (cam, params(), ok, imax, 1, sums)),
        ("2^32 pixels", (cam, params(width=65536, height=65536), ok, 0, 1, sums)),
        ("width and height", (cam, params(width=0), ok, 0, 1, sums)),
        # valid chains reach the ctx check: the ends of every range, no flags, max_depth not read
        ("null ctx", (cam, params(max_depth=-1), chain(0, 0, 0.0), 0, imax, sums)),
        ("null ctx", (cam, params(), chain(64, BOTH, 1e300), 0, 1, sums)),
        ("null ctx", (cam, params(), chain(8, rtamd.RT_CHAIN_METAL, -0.0), 0, 1, sums)),
    ]
    for word, (c, p, ch, first, n, s) in cases:
        rc, msg = _call(fn_async, None, c, p, ch, first, n, s)
        assert rc == rtamd.RT_E_INVALID and word in msg, (word, rc, msg)
    st = rtamd.rt_feature_chain_stats()
    assert rtamd.lib().rt_last_feature_chain(None, C.byref(st)) == rtamd.RT_E_INVALID


def test_make_feature_chain():
    ch = rtamd.make_feature_chain()
    assert (ch.max_bounces, ch.flags, ch.max_fuzz) == (8, BOTH, 0.0)
    ch = rtamd.make_feature_chain(3, dielectric=False, max_fuzz=0.25)
    assert (ch.max_bounces, ch.flags, ch.max_fuzz) == (3, rtamd.RT_CHAIN_METAL, 0.25)
    assert rtamd.make_feature_chain(0, metal=False).flags == rtamd.RT_CHAIN_DIELECTRIC


def _plan(scene, W, H, chain, flags=0):
    p = rtamd.make_params(W, H, 1, 1, rtamd.RT_RNG_PHILOX, seed=1, flags=flags)
    info = rtamd.rt_launch_info()
    extra = np.zeros(5, dtype=np.int32)
    if chain is None:
        fn = rtamd.lib().rt_internal_features_plan
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        rc = fn(C.addressof(scene.desc), 0, CU_COUNT, C.addressof(p), C.addressof(info), extra.ctypes.data)
    else:
        fn = rtamd.lib().rt_internal_features_chain_plan
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        rc = fn(C.addressof(scene.desc), 0, CU_COUNT, C.addressof(p), C.addressof(chain), C.addressof(info),
                extra.ctypes.data)
    if rc:
        return rc, None
    return ({k: getattr(info, k) for k, _ in rtamd.rt_launch_info._fields_},
            dict(zip(("n_items", "entries", "n_leaves", "wide_packed", "leaf_stop"), (int(x) for x in extra))))


def test_plan_without_a_device(monkeypatch):
    """A chain pass takes the first-hit pass's walk forms. The staged 4-wide form runs at 3 waves per SIMD (its
    kernels hold the chain's state in registers there) where the first-hit pass runs at 4, and RTAMD_WAVES still
    decides; every other field, and every other form, is the first-hit plan's. A chain the pass rejects is
    RT_E_INVALID here too."""
    for k in ("RTAMD_LDS", "RTAMD_LEAF_LDS", "RTAMD_PACKED_KEYS", "RTAMD_WAVES", "RTAMD_WIDE"):
        monkeypatch.delenv(k, raising=False)
    ch = rtamd.make_feature_chain()
    scene, _ = feature_ref.world("random_book_one")
    first, fx = _plan(scene, 1200, 800, None)
    info, extra = _plan(scene, 1200, 800, ch)
    print(info, extra)
    assert first["waves"] == 4 and first["block"] == 1024
    assert info["variant"] == F_WIDE and info["loop"] == 2 and info["lds_staged"] == 1 and info["leaf_lds"] == 1
    assert info["waves"] == 3 and info["block"] == 768 and info["grid"] == CU_COUNT
    assert info["dyn_lds_bytes"] == 128 * extra["n_items"] + 64 * extra["n_leaves"] + 4 * 768 * extra["entries"]
    assert extra == fx
    same = ("variant", "loop", "lds_staged", "leaf_lds", "work_items", "wide_nodes", "chunk", "chunk_batches")
    assert {k: info[k] for k in same} == {k: first[k] for k in same}
    monkeypatch.setenv("RTAMD_WAVES", "4")
    assert _plan(scene, 1200, 800, ch) == _plan(scene, 1200, 800, None)
    monkeypatch.delenv("RTAMD_WAVES")
    monkeypatch.setenv("RTAMD_LDS", "0")
    assert _plan(scene, 1200, 800, ch) == _plan(scene, 1200, 800, None)
    monkeypatch.delenv("RTAMD_LDS")
    assert _plan(scene, 64, 48, ch, rtamd.RT_FLAG_REFERENCE_CULL) == _plan(scene, 64, 48, None, rtamd.RT_FLAG_REFERENCE_CULL)
    for other in (feature_ref.fog_world()[0], feature_ref.deep_world()[0], feature_ref.world("chains")[0]):
        assert _plan(other, 64, 48, ch) == _plan(other, 64, 48, None)
    spec, _ = fcr.specular_world()
    assert _plan(spec, 64, 48, ch)[0]["loop"] == 2
    bad = rtamd.make_feature_chain(65)
    assert _plan(scene, 64, 48, bad) == (rtamd.RT_E_INVALID, None)


def test_composition_matches_the_oracles_render():
    """The specular-only world at 64x48, 8 samples, max_bounces 16. Every path of the oracle's max_depth = 17
    render is a specular chain that ends in the background (thr * background) or runs out of depth (black), so the
    image is, per pixel, the sum of thr * background over the samples whose chain ended in a miss, over spp: the
    composition's albedo sums restricted to those samples. The two differ in summation order (the image's chunk
    sums) and one division: at most 63 additions of non-negative terms and a division, each within 2^-53
    relative, about 1.4e-14; the bound asserted is 1e-12. Conditions on the composition itself, first: at most
    0.1 % of pixels left out as undecided, at most 1 % of samples capped."""
    W, H, n, mb = 64, 48, 8, 16
    scene, cam = fcr.specular_world()
    comp = fcr.composition("specular", W, H, n, mb, BOTH)
    k = comp.counts()
    print(f"specular world: {k}, scatters {comp.scatters}, left out {int(comp.left_out.sum())} pixels")
    assert comp.left_out.mean() <= 0.001
    assert k["ended_surface"] == 0 and k["samples"] == W * H * n == k["ended_miss"] + k["ended_cap"]
    assert k["ended_cap"] <= 0.01 * k["samples"]
    assert k["bounces"] == comp.scatters > 0.2 * k["samples"]  # (the spheres fill a good part of the frame)
    assert comp.bounces.max() >= 4  # (chains through glass: in, bounces inside, out, and on to a neighbour)
    p = rtamd.make_params(W, H, n, mb + 1, rtamd.RT_RNG_PHILOX, seed=1024)
    _, lin, _, _ = pyoracle.render(scene, cam, p)
    want = comp.sums(only=fcr.MISS)[..., 0:3] / float(n)
    keep = ~comp.left_out
    err = np.abs(lin - want)[keep]
    print(f"max relative difference {float((err / np.maximum(want[keep], 1e-300)).max()):.3g}")
    assert (err <= 1e-12 * want[keep]).all()


def test_zero_bounces_and_no_flags_are_the_first_hit_composition():
    """max_bounces = 0, and flags = 0, compose to feature_ref's first-hit sums bit for bit (chains, 37x21x5)."""
    W, H, n = 37, 21, 5
    want = feature_ref.composition("chains", W, H, n).sums()
    for mb, flags in ((0, BOTH), (8, 0)):
        comp = fcr.composition("chains", W, H, n, mb, flags)
        assert np.array_equal(comp.sums(), want)
        k = comp.counts()
        assert k["bounces"] == 0 and k["samples"] == W * H * n
        assert (k["ended_cap"] > 0) == (flags != 0)


def test_words_consumed_per_scatter_match_the_oracle():
    """pyoracle.probe(scene, "scatter", ...) consumes one word for a Dielectric and two for a Metal, even at fuzz 0:
    the composition's streams advance by exactly that per followed scatter."""
    scene, cam = fcr.specular_world(True)
    d = scene.desc
    rec = np.zeros((d.n_materials, 18))
    rec[:, 0:3], rec[:, 3:6] = (0.0, 3.0, -4.0), (0.1, -0.7, 0.6)
    rec[:, 7], rec[:, 8:11], rec[:, 11:14], rec[:, 16] = 1.0, (0.1, 2.3, -3.4), (0.0, 1.0, 0.0), 1.0
    rec[:, 17] = np.arange(d.n_materials)
    out = pyoracle.probe(scene, "scatter", rec, seed=9)
    per_type = {fcr.RT_MAT_METAL: 2, fcr.RT_MAT_DIELECTRIC: 1}
    kinds = set()
    for m in range(d.n_materials):
        assert out[m, 12] == 1 and out[m, 13] == per_type[d.materials[m].type]
        kinds.add((d.materials[m].type, d.materials[m].param > 0))
    assert len(kinds) == 3  # Dielectric, Metal at fuzz 0, fuzzy Metal
    # the composition: words after getRay + 2 per Metal scatter + 1 per Dielectric scatter
    W, H, n = 64, 48, 2
    for flags, per in ((rtamd.RT_CHAIN_DIELECTRIC, 1), (rtamd.RT_CHAIN_METAL, 2)):
        comp = fcr.Chain(scene, cam, W, H, 1024, 0, n, 8, flags, 0.5)
        none = fcr.Chain(scene, cam, W, H, 1024, 0, n, 0, flags, 0.5)
        assert comp.bounces.sum() > 500
        assert np.array_equal(comp.words - none.words, per * comp.bounces)


def test_chain_depth_is_a_path_length():
    """chains at 37x21x8, max_bounces 8: a sample that followed a scatter and ended on a hit has a depth strictly
    beyond its first segment's (feature_ref's first-hit depth of the same sample: the same primary ray), and a sample
    that followed none has exactly that depth."""
    W, H, n = 37, 21, 8
    first = feature_ref.composition("chains", W, H, n).per_sample
    comp = fcr.composition("chains", W, H, n, 8, BOTH)
    hit = comp.per_sample[..., 7] == 1
    went = hit & (comp.bounces > 0)
    assert went.sum() > 50 and (first[..., 7][went] == 1).all()
    assert (comp.per_sample[..., 6][went] > first[..., 6][went]).all()
    stayed = comp.bounces == 0
    assert np.array_equal(comp.per_sample[stayed], first[stayed])
