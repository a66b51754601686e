"""Material-ID coverage buffers without a device (include/rt.h rt_render_ids, rt_ids_*): the shared fold against a
Python restatement (tests/id_ref.py fold), the rank resolve, the matte and the preview against numpy restatements
byte for byte, every RT_E_INVALID case of the calls, the device-free plan, and the CPU composition the GPU tests
compare against (tests/id_ref.py), chosen here so that it leaves out at most 0.1 % of pixels."""
import ctypes as C

import numpy as np
import pytest

import feature_chain_ref as fcr
import feature_ref
import id_ref
import rtamd

MISS = rtamd.RT_ID_MISS
BOTH = rtamd.RT_CHAIN_DIELECTRIC | rtamd.RT_CHAIN_METAL
CU_COUNT = 256


def _tuple(rec):
    return tuple(map(lambda v: v if isinstance(v, int) else tuple(v), id_ref.as_tuple(rec)))


def _ref_tuple(t):
    return (tuple(t[0]), tuple(t[1]), t[2], t[3])


def test_record_layout():
    assert rtamd.ID_DTYPE == id_ref.ID_DTYPE and rtamd.ID_DTYPE.itemsize == 64 == C.sizeof(rtamd.rt_id_record)
    assert (rtamd.RT_ID_SLOTS, rtamd.RT_ID_MISS, rtamd.RT_ID_MATTE_MAX) == (7, 0xFFFFFFFF, 1024)
    f = rtamd.ID_DTYPE.fields
    assert (f["id"][1], f["count"][1], f["other"][1], f["samples"][1]) == (0, 28, 56, 60)


@pytest.mark.parametrize("distinct", [1, 3, 7, 8, 20])
def test_fold_against_the_restatement(distinct):
    """Random streams of 1..200 samples over `distinct` ids (RT_ID_MISS among them, an ordinary id): the record is
    the restatement's; slots are in order of first appearance; `other` counts exactly the samples of the eighth and
    later ids; while other == 0 the slots are the histogram."""
    rng = np.random.default_rng(100 + distinct)
    pool = np.concatenate([[MISS], rng.choice(5000, size=distinct - 1, replace=False)]).astype(np.uint32)
    for n in (1, 2, 7, 8, 9, 40, 200):
        ids = rng.choice(pool, size=n)
        got = rtamd.fold_ids(None, ids)
        assert _tuple(got) == _ref_tuple(id_ref.fold(ids.tolist()))
        seen = list(dict.fromkeys(int(x) for x in ids))  # (first-appearance order)
        used = int((got["count"] > 0).sum())
        assert used == min(len(seen), 7) and [int(x) for x in got["id"][:used]] == seen[:7]
        assert (got["count"][used:] == 0).all() and (got["id"][used:] == 0).all()
        assert int(got["samples"]) == n == int(got["count"].sum()) + int(got["other"])
        assert int(got["other"]) == sum(1 for x in ids if int(x) in seen[7:])
        if got["other"] == 0:
            assert {int(i): int(c) for i, c in zip(got["id"][:used], got["count"][:used])} == \
                   {v: int((ids == v).sum()) for v in seen}
        else:
            assert distinct > 7


def test_fold_split_invariance_and_saturation():
    """One 40-sample stream over 9 ids split at every point: folding [0, k) and then [k, 40) onto it is the fold of
    [0, 40) byte for byte. A record at UINT32_MAX samples is left as it is. A free slot before a used one with the
    id: the used slot counts (the rule looks for the id first)."""
    rng = np.random.default_rng(7)
    ids = rng.choice(np.array([3, 9, MISS, 0, 17, 4, 250, 8, 11], dtype=np.uint32), size=40)
    whole = rtamd.fold_ids(None, ids)
    assert whole["other"] > 0
    for k in range(41):
        part = rtamd.fold_ids(None, ids[:k])
        assert rtamd.fold_ids(part, ids[k:]).tobytes() == whole.tobytes(), k
    full = np.zeros((), dtype=rtamd.ID_DTYPE)
    full["id"][0], full["count"][0], full["samples"] = 5, 0xFFFFFFFF, 0xFFFFFFFF
    assert rtamd.fold_ids(full, [5, 6, MISS]).tobytes() == full.tobytes()
    near = full.copy()
    near["count"][0], near["samples"] = 0xFFFFFFFE, 0xFFFFFFFE
    assert rtamd.fold_ids(near, [5, 6]).tobytes() == full.tobytes()
    gap = np.zeros((), dtype=rtamd.ID_DTYPE)
    gap["id"][2], gap["count"][2], gap["samples"] = 12, 4, 4
    got = rtamd.fold_ids(gap, [12, 13])
    assert _tuple(got) == _ref_tuple(id_ref.fold([12, 13], id_ref.as_tuple(gap)))
    assert [int(x) for x in got["count"]] == [1, 0, 5, 0, 0, 0, 0] and int(got["id"][0]) == 13
    L = rtamd.lib()
    assert L.rt_ids_fold_host(None, None, 0) == rtamd.RT_E_INVALID
    assert L.rt_ids_fold_host(C.c_void_p(gap.ctypes.data), None, 1) == rtamd.RT_E_INVALID
    assert L.rt_ids_fold_host(C.c_void_p(gap.ctypes.data), None, -1) == rtamd.RT_E_INVALID
    assert L.rt_ids_fold_host(C.c_void_p(gap.ctypes.data), None, 0) == rtamd.RT_OK


def _random_records(rng, shape):
    """Folded records of random streams (0 to 60 samples over 1 to 12 ids, RT_ID_MISS among them), a zero record
    and hand-made ties among them."""
    recs = np.zeros(shape, dtype=rtamd.ID_DTYPE)
    flat = recs.reshape(-1)
    for i in range(flat.size):
        pool = np.concatenate([[MISS], rng.choice(3000, size=rng.integers(0, 12), replace=False)]).astype(np.uint32)
        flat[i] = rtamd.fold_ids(None, rng.choice(pool, size=rng.integers(0, 61)))[()]
    return recs


def _np_fmix32(h):
    h = h.astype(np.uint64)
    m = np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & m
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & m
    h ^= h >> np.uint64(16)
    return h.astype(np.uint32)


def np_matte(recs, ids):
    inlist = np.isin(recs["id"], np.asarray(ids, dtype=np.uint32)) & (recs["count"] > 0)
    total = np.where(inlist, recs["count"].astype(np.uint64), np.uint64(0)).sum(axis=-1)
    n = recs["samples"].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        cov = np.where(recs["samples"] > 0, total.astype(np.float64) / n, 0.0)
    return cov, (cov * 255.0 + 0.5).astype(np.uint8)


def np_preview(recs):
    n = recs["samples"].astype(np.float64)[..., None]
    with np.errstate(invalid="ignore", divide="ignore"):
        cov = np.where(n > 0, recs["count"].astype(np.float64) / n, 0.0)
    h = _np_fmix32(recs["id"])
    acc = np.zeros(recs.shape + (3,))
    for k in range(7):
        for c in range(3):
            col = np.where(recs["id"][..., k] == MISS, 0.0, ((h[..., k] >> np.uint32(8 * c)) & np.uint32(255)) / 255.0)
            acc[..., c] = acc[..., c] + cov[..., k] * col
    return (acc * 255.0 + 0.5).astype(np.uint8)


def np_resolve(recs):
    flat = recs.reshape(-1)
    ids, cov = np.full((flat.size, 7), MISS, dtype=np.uint32), np.zeros((flat.size, 7))
    other = np.zeros(flat.size)
    for i, r in enumerate(flat):
        order = sorted(range(7), key=lambda k: (-int(r["count"][k]), int(r["id"][k])))
        for j, k in enumerate(order):
            if r["count"][k] > 0:
                ids[i, j] = r["id"][k]
            if r["samples"] > 0:
                cov[i, j] = float(r["count"][k]) / float(r["samples"])
        if r["samples"] > 0:
            other[i] = float(r["other"]) / float(r["samples"])
    return ids.reshape(recs.shape + (7,)), cov.reshape(recs.shape + (7,)), other.reshape(recs.shape)


def test_fmix32_is_murmur3s_finaliser():
    """Known values of MurmurHash3's fmix32: 0 -> 0, and the published avalanche of 1."""
    assert int(_np_fmix32(np.array([0], dtype=np.uint32))[0]) == 0
    assert int(_np_fmix32(np.array([1], dtype=np.uint32))[0]) == 0x514E28B7
    one = np.zeros(1, dtype=rtamd.ID_DTYPE)
    one["id"][0, 0], one["count"][0, 0], one["samples"] = 1, 3, 3
    assert rtamd.id_preview(one)[0].tolist() == [0xB7, 0x28, 0x4E]


def test_resolve_matte_and_preview_against_numpy():
    rng = np.random.default_rng(11)
    recs = _random_records(rng, (9, 13))
    recs[0, 0] = np.zeros((), dtype=rtamd.ID_DTYPE)[()]  # samples == 0
    tie = np.zeros((), dtype=rtamd.ID_DTYPE)  # ties broken by id, a free slot between used ones, the sky
    tie["id"][:5], tie["count"][:5], tie["other"], tie["samples"] = (40, MISS, 7, 0, 9), (3, 3, 3, 0, 5), 2, 16
    recs[0, 1] = tie[()]
    assert (recs["other"] > 0).any() and (recs["samples"] == 0).sum() >= 1
    out = rtamd.resolve_ids(recs)
    ids, cov, other = np_resolve(recs)
    assert np.array_equal(out["rank_ids"], ids) and out["rank_coverage"].tobytes() == cov.tobytes()
    assert out["other_coverage"].tobytes() == other.tobytes() and np.array_equal(out["samples"], recs["samples"])
    assert out["rank_ids"][0, 1].tolist() == [9, 7, 40, MISS, MISS, MISS, MISS]
    assert out["rank_coverage"][0, 1].tolist() == [5 / 16, 3 / 16, 3 / 16, 3 / 16, 0, 0, 0] and out["other_coverage"][0, 1] == 2 / 16
    assert (out["rank_ids"][0, 0] == MISS).all() and (out["rank_coverage"][0, 0] == 0).all() and out["other_coverage"][0, 0] == 0
    assert (np.diff(out["rank_coverage"], axis=-1) <= 0).all()
    # any output may be null
    L = rtamd.lib()
    only = np.zeros(recs.shape)
    assert L.rt_ids_resolve(C.c_void_p(recs.ctypes.data), recs.size, None, None, only.ctypes.data_as(C.POINTER(C.c_double))) == 0
    assert only.tobytes() == other.tobytes()
    assert L.rt_ids_resolve(None, 1, None, None, None) == rtamd.RT_E_INVALID
    assert L.rt_ids_resolve(C.c_void_p(recs.ctypes.data), 0, None, None, None) == rtamd.RT_E_INVALID
    present = np.unique(recs["id"][recs["count"] > 0])
    lists = [[int(present[0])], [MISS], sorted(set(int(x) for x in present[::3]) | {MISS}),
             sorted(set(int(x) for x in rng.choice(3000, size=1023, replace=False)) | {MISS})[:1024]]
    for lst in lists:
        cov_g, u8_g = rtamd.id_matte(recs, lst)
        cov_w, u8_w = np_matte(recs, lst)
        assert cov_g.tobytes() == cov_w.tobytes() and np.array_equal(u8_g, u8_w), len(lst)
    assert rtamd.id_matte(recs, [MISS])[0][0, 1] == 3 / 16
    every = sorted(int(x) for x in present)
    assert len(every) <= 1024
    full = rtamd.id_matte(recs, every)
    want = np.where(recs["samples"] > 0, 1.0 - out["other_coverage"], 0.0)
    assert np.allclose(full[0], want, rtol=0, atol=1e-15)
    assert (full[1][(recs["other"] == 0) & (recs["samples"] > 0)] == 255).all()
    assert np.array_equal(rtamd.id_preview(recs), np_preview(recs))
    assert (rtamd.id_preview(recs)[0, 0] == 0).all()


def test_invalid_lists_and_arguments():
    recs = np.zeros(4, dtype=rtamd.ID_DTYPE)
    for bad in ([], [3, 2], [1, 1], [0, 5, 5, 9], list(range(1025))):
        with pytest.raises(rtamd.RTError):
            rtamd.id_matte(recs, bad)
    L = rtamd.lib()
    lst = np.arange(1025, dtype=np.uint32)
    lp = lst.ctypes.data_as(C.POINTER(C.c_uint32))
    cov, u8 = np.zeros(4), np.zeros(12, dtype=np.uint8)
    cp, up, rp = cov.ctypes.data_as(C.POINTER(C.c_double)), u8.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_void_p(recs.ctypes.data)
    for n_ids in (0, -1, 1025):
        assert L.rt_ids_matte_host(rp, 4, lp, n_ids, cp, up) == rtamd.RT_E_INVALID
        assert L.rt_ids_matte(None, rp, 4, lp, n_ids, cp, up) == rtamd.RT_E_INVALID
        assert "n_ids" in L.rt_last_error().decode()
        assert L.rt_ids_matte_async(None, rp, 4, lp, n_ids, cp, up, None) == rtamd.RT_E_INVALID
    assert L.rt_ids_matte_host(rp, 4, lp, 1024, cp, up) == rtamd.RT_OK
    assert L.rt_ids_matte_host(rp, 4, lp, 1, None, up) == rtamd.RT_OK and L.rt_ids_matte_host(rp, 4, lp, 1, cp, None) == rtamd.RT_OK
    for args in ((None, 4, lp, 1, cp, up), (rp, 0, lp, 1, cp, up), (rp, 4, None, 1, cp, up), (rp, 4, lp, 1, None, None)):
        assert L.rt_ids_matte_host(*args) == rtamd.RT_E_INVALID
    desc = np.array([2, 1], dtype=np.uint32).ctypes.data_as(C.POINTER(C.c_uint32))
    for fn, tail in ((L.rt_ids_matte, ()), (L.rt_ids_matte_async, (None,))):
        assert fn(None, rp, 4, desc, 2, cp, up, *tail) == rtamd.RT_E_INVALID and "ascending" in L.rt_last_error().decode()
        assert fn(None, None, 4, lp, 1, cp, up, *tail) == rtamd.RT_E_INVALID
        assert fn(None, rp, 4, lp, 1, None, None, *tail) == rtamd.RT_E_INVALID
        assert fn(None, rp, 0, lp, 1, cp, up, *tail) == rtamd.RT_E_INVALID
        assert fn(None, rp, 2**32, lp, 1, cp, up, *tail) == rtamd.RT_E_INVALID
        assert fn(None, rp, 4, lp, 1, cp, up, *tail) == rtamd.RT_E_INVALID and "null ctx" in L.rt_last_error().decode()
    assert L.rt_ids_preview_host(None, 4, up) == rtamd.RT_E_INVALID and L.rt_ids_preview_host(rp, 4, None) == rtamd.RT_E_INVALID
    assert L.rt_ids_preview_host(rp, 0, up) == rtamd.RT_E_INVALID and L.rt_ids_preview_host(rp, 4, up) == rtamd.RT_OK
    for fn, tail in ((L.rt_ids_preview, ()), (L.rt_ids_preview_async, (None,))):
        assert fn(None, None, 4, up, *tail) == rtamd.RT_E_INVALID and fn(None, rp, 4, None, *tail) == rtamd.RT_E_INVALID
        assert fn(None, rp, 0, up, *tail) == rtamd.RT_E_INVALID
        assert fn(None, rp, 4, up, *tail) == rtamd.RT_E_INVALID and "null ctx" in L.rt_last_error().decode()


def _call(fn_async, ctx, cam, p, chain, first, n, recs):
    L = rtamd.lib()
    ref = lambda x: C.byref(x) if x is not None else None
    rp = C.c_void_p(recs.ctypes.data) if recs is not None else None
    if fn_async:
        rc = L.rt_render_ids_async(ctx, ref(cam), ref(p), ref(chain), first, n, 0, rp, None)
    else:
        rc = L.rt_render_ids(ctx, ref(cam), ref(p), ref(chain), first, n, 0, rp)
    return rc, L.rt_last_error().decode()


@pytest.mark.parametrize("fn_async", [False, True], ids=["blocking", "async"])
def test_invalid_arguments_without_a_device(fn_async):
    """Every RT_E_INVALID case of the pass is returned before any HIP call: there is no device here and the ctx is
    null. The ctx is checked last, so each case is told by its message, and valid arguments reach that check."""
    cam = rtamd.camera("random_scene", 16, 8)
    recs = np.zeros((8, 16), dtype=rtamd.ID_DTYPE)

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
    cases = []
    for ok in (None, chain()):  # everything the first-hit pass rejects, without and with a chain
        cases += [
            ("null argument", (None, params(), ok, 0, 1, recs)),
            ("null argument", (cam, None, ok, 0, 1, recs)),
            ("null argument", (cam, params(), ok, 0, 1, None)),
            ("RT_RNG_PHILOX", (cam, params(rng_mode=rtamd.RT_RNG_EXACT), ok, 0, 1, recs)),
            ("RT_FLAG_SHARED_LIBM", (cam, params(flags=rtamd.RT_FLAG_SHARED_LIBM), ok, 0, 1, recs)),
            ("shard_count", (cam, params(shard_count=2), ok, 0, 1, recs)),
            ("first_sample", (cam, params(), ok, -1, 1, recs)),
            ("first_sample", (cam, params(), ok, 0, 0, recs)),
            ("first_sample", (cam, params(), ok, imax, 1, recs)),
            ("2^32 pixels", (cam, params(width=65536, height=65536), ok, 0, 1, recs)),
            ("width and height", (cam, params(width=0), ok, 0, 1, recs)),
            ("null ctx", (cam, params(max_depth=-1), ok, 0, imax, recs)),
        ]
    cases += [  # the chain's own cases
        ("max_bounces", (cam, params(), chain(max_bounces=-1), 0, 1, recs)),
        ("max_bounces", (cam, params(), chain(max_bounces=65), 0, 1, recs)),
        ("unknown flag bits", (cam, params(), chain(flags=4), 0, 1, recs)),
        ("max_fuzz", (cam, params(), chain(max_fuzz=-1e-300), 0, 1, recs)),
        ("max_fuzz", (cam, params(), chain(max_fuzz=float("inf")), 0, 1, recs)),
        ("max_fuzz", (cam, params(), chain(max_fuzz=float("nan")), 0, 1, recs)),
        ("null ctx", (cam, params(), chain(0, 0, 0.0), 0, 1, recs)),
        ("null ctx", (cam, params(), chain(64, BOTH, 1e300), 0, 1, recs)),
    ]
    for word, (c, p, ch, first, n, r) in cases:
        rc, msg = _call(fn_async, None, c, p, ch, first, n, r)
        assert rc == rtamd.RT_E_INVALID and word in msg and msg.startswith("rt_render_ids: "), (word, rc, msg)


def _plan(scene, W, H, chain, flags=0, which="ids", cu_count=CU_COUNT):
    p = rtamd.make_params(W, H, 1, 1, rtamd.RT_RNG_PHILOX, seed=1, flags=flags)
    info = rtamd.rt_launch_info()
    extra = np.zeros(5, dtype=np.int32)
    fn = getattr(rtamd.lib(), "rt_internal_ids_plan" if which == "ids" else "rt_internal_features_chain_plan")
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    rc = fn(C.addressof(scene.desc), 0, cu_count, C.addressof(p), C.addressof(chain) if chain is not None else None,
            C.addressof(info), extra.ctypes.data)
    if rc:
        return rc, None
    return ({k: getattr(info, k) for k, _ in rtamd.rt_launch_info._fields_},
            dict(zip(("n_items", "entries", "n_leaves", "wide_packed", "leaf_stop"), (int(x) for x in extra))))


def test_plan_without_a_device(monkeypatch):
    """An id pass, with or without a chain, launches with the chain feature pass's plan: on the book-one cover
    (C2-like: spheres only) the staged 4-wide form at 3 waves per SIMD, where RTAMD_WAVES still decides; the mixed
    walk on worlds with frames or media; the recursive walk on the deep world."""
    for k in ("RTAMD_LDS", "RTAMD_LEAF_LDS", "RTAMD_PACKED_KEYS", "RTAMD_WAVES", "RTAMD_WIDE"):
        monkeypatch.delenv(k, raising=False)
    ch = rtamd.make_feature_chain()
    scene, _ = feature_ref.world("random_book_one")
    info, extra = _plan(scene, 1200, 800, None)
    print(info, extra)
    assert info["variant"] == 256 and info["loop"] == 2 and info["lds_staged"] == 1 and info["leaf_lds"] == 1
    assert info["waves"] == 3 and info["block"] == 768 and info["grid"] == CU_COUNT
    assert info["work_items"] == 150 * 100
    assert info["dyn_lds_bytes"] == 128 * extra["n_items"] + 64 * extra["n_leaves"] + 4 * 768 * extra["entries"]
    assert _plan(scene, 1200, 800, ch) == (info, extra) == _plan(scene, 1200, 800, ch, which="chain")
    monkeypatch.setenv("RTAMD_WAVES", "4")
    assert _plan(scene, 1200, 800, None)[0]["block"] == 1024
    monkeypatch.delenv("RTAMD_WAVES")
    monkeypatch.setenv("RTAMD_LDS", "0")
    assert _plan(scene, 1200, 800, None)[0]["lds_staged"] == 0
    monkeypatch.delenv("RTAMD_LDS")
    assert _plan(scene, 64, 48, None, rtamd.RT_FLAG_REFERENCE_CULL)[0]["loop"] == 1
    for other, loop in ((feature_ref.fog_world()[0], 1), (feature_ref.world("chains")[0], 1),
                        (feature_ref.world("frames")[0], 1), (feature_ref.deep_world()[0], 0),
                        (fcr.specular_world()[0], 2)):
        for c in (None, ch):
            assert _plan(other, 64, 48, c)[0]["loop"] == loop
            assert _plan(other, 64, 48, c) == _plan(other, 64, 48, ch, which="chain")
    assert _plan(scene, 64, 48, rtamd.make_feature_chain(65)) == (rtamd.RT_E_INVALID, None)


# The GPU tests' chain cases (tests/test_gpu_ids.py): world, W, H
CHAIN_WORLDS = [("chains", 64, 48), ("specular", 64, 48), ("chains", 37, 21)]
CHAIN_SETTINGS = [(mb, fl) for mb in (1, 8) for fl in (rtamd.RT_CHAIN_DIELECTRIC, rtamd.RT_CHAIN_METAL, BOTH)]


@pytest.mark.parametrize("name,W,H", CHAIN_WORLDS, ids=[f"{w[0]}_{w[1]}x{w[2]}" for w in CHAIN_WORLDS])
def test_chain_composition_on_the_gpu_tests_cases(name, W, H):
    """For every case the GPU tests compose: at most 0.1 % of pixels are left out, the restated stepping ends every
    sample as feature_chain_ref's Chain does (how, and after how many scatters), a sample that ends on a hit has a
    material id below n_materials, and max_bounces = 0 or flags = 0 give the first-hit ids."""
    n = 8
    scene, _ = fcr.world(name)
    first = id_ref.first_hit_ids(name, W, H, n)
    for mb, fl in CHAIN_SETTINGS:
        comp, ref = id_ref.chain_ids(name, W, H, n, mb, fl), fcr.composition(name, W, H, n, mb, fl)
        assert comp.left_out.mean() <= 0.001, (mb, fl)
        assert np.array_equal(comp.kind, ref.kind) and np.array_equal(comp.bounces, ref.bounces)
        assert np.array_equal(comp.left_out, ref.left_out) and comp.counts() == ref.counts()
        assert np.array_equal(comp.ids == MISS, comp.kind == fcr.MISS)
        assert (comp.ids[comp.ids != MISS] < scene.desc.n_materials).all()
        assert np.array_equal(comp.ids[comp.bounces == 0], first[comp.bounces == 0])
    for mb, fl in ((0, BOTH), (8, 0)):
        assert np.array_equal(id_ref.chain_ids(name, W, H, n, mb, fl).ids, first)


def test_first_hit_composition_agrees_with_the_feature_composition():
    """The ids' hit / miss split is feature_ref's hits feature, sample for sample (chains, 37x21x8), and the folded
    records count them: samples - count[RT_ID_MISS] = the hits sum wherever other == 0."""
    W, H, n = 37, 21, 8
    ids = id_ref.first_hit_ids("chains", W, H, n)
    feat = feature_ref.composition("chains", W, H, n)
    assert np.array_equal(ids != MISS, feat.per_sample[..., 7] == 1)
    recs = id_ref.first_hit_records("chains", W, H, n)
    miss = np.where((recs["id"] == MISS) & (recs["count"] > 0), recs["count"], 0).sum(axis=-1)
    keep = recs["other"] == 0
    assert keep.any() and np.array_equal((recs["samples"] - miss)[keep], feat.sums()[..., 7][keep])
    assert (recs["samples"] == n).all()


# The overflow case of the GPU tests: the book-one cover at 16x8, 64 samples
OVERFLOW = ("random_book_one", 16, 8, 64, 1024)


def test_overflow_case_has_full_and_overflowing_pixels():
    name, W, H, n, seed = OVERFLOW
    recs = id_ref.first_hit_records(name, W, H, n, seed)
    used = (recs["count"] > 0).sum(axis=-1)
    print("used slots histogram", np.bincount(used.reshape(-1), minlength=8), "pixels with other > 0", int((recs["other"] > 0).sum()))
    assert (recs["other"] > 0).any() and ((used == 7) & (recs["other"] == 0)).any()
