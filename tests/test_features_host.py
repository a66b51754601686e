"""First-hit feature buffers without a device (include/rt.h rt_render_features): the CPU composition the GPU tests
compare against (tests/feature_ref.py) checked against the oracle's own depth-1 render, rt_features_resolve
against numpy, every RT_E_INVALID case of the render calls, and the device-free launch plan
(rt_internal_features_plan) of a staged spheres world, the same from global memory, and a fog world."""
import ctypes as C

import numpy as np
import pytest

import feature_ref
import pyoracle
import rtamd

CU_COUNT = 256
K_LDS_BUDGET = 160 * 1024 - 16 * 8  # rt_launch_plan.h kLdsBudget
F_WIDE, F_MIXW, F_UV, F_ALL = 256, 1024, 64, 63 | 512


def test_numpy_philox_and_draws_match_the_oracle():
    """1000 random counters and keys against pyoracle.philox, and the word -> draw conversion against
    oracle_word_to_draw on the words they make and on the edge words."""
    rng = np.random.default_rng(3)
    ctr = rng.integers(0, 1 << 32, (1000, 4), dtype=np.uint64).astype(np.uint32)
    key = [int(x) for x in rng.integers(0, 1 << 32, 2, dtype=np.uint64)]
    got = feature_ref.philox(ctr, key)
    want = np.array([pyoracle.philox([int(x) for x in c], key) for c in ctr], dtype=np.uint32)
    assert np.array_equal(got, want)
    words = np.concatenate([got[:, 0].astype(np.uint64) | (got[:, 1].astype(np.uint64) << np.uint64(32)),
                            np.array([0, 1, (1 << 64) - 1, 1 << 63, (1 << 53) + 1], dtype=np.uint64)])
    L = pyoracle.lib()
    assert np.array_equal(feature_ref.word_to_draw(words), np.array([L.oracle_word_to_draw(int(w)) for w in words]))


def test_composition_matches_the_oracles_depth_one_render():
    """random_book_one at 48x32x6: a depth-1 RT_FLAG_NAN_ZERO render is background for a miss and black for a
    hit, so hits == spp - rint(lin * spp / background) on every pixel pins the helper's streams, rays and
    closest hits to the oracle's renderer. Condition, on the oracle alone: >= 1 % of pixels partly covered."""
    W, H, spp = 48, 32, 6
    scene, cam = feature_ref.world("random_book_one")
    p = rtamd.make_params(W, H, spp, 1, rtamd.RT_RNG_PHILOX, seed=1024, flags=rtamd.RT_FLAG_NAN_ZERO)
    _, lin, _, _ = pyoracle.render(scene, cam(W, H), p)
    want = feature_ref.hits_from_render(lin, spp, scene.desc.background)
    partly = float(((want > 0) & (want < spp)).mean())
    print(f"oracle depth-1 render: coverage {want.mean() / spp:.3f}, partly covered {partly:.3f}")
    assert partly >= 0.01
    comp = feature_ref.composition("random_book_one", W, H, spp)
    assert np.array_equal(comp.sums()[..., 7], want)
    assert comp.coverage() == (float(want.mean() / spp), partly)
    # the fold splits: [0, 2) then [2, 6) onto it is the whole fold
    assert np.array_equal(comp.sums(2, 4, start=comp.sums(0, 2)), comp.sums())


def test_resolve_against_numpy():
    """rt_features_resolve on random sums, with pixels nothing hit (depth +inf), NaN sums, and the albedo's
    bytes against oracle_scale_color."""
    rng = np.random.default_rng(5)
    n = 7
    sums = rng.uniform(0.0, 2.0 * n, (33, 9, 8))
    sums[..., 3:6] = rng.uniform(-n, n, (33, 9, 3))
    sums[..., 7] = rng.integers(0, n + 1, (33, 9)).astype(np.float64)
    sums[0, 0, 7] = 0.0
    sums[sums[..., 7] == 0, 6] = 0.0
    sums[1, 2, 0] = np.nan
    sums[2, 3, 6] = np.nan
    sums[3, 4, 1] = np.inf
    sums[4, 5, 2] = -1.0
    out = rtamd.resolve_features(sums, n)
    assert np.array_equal(out["albedo"], sums[..., 0:3] / float(n), equal_nan=True)
    assert np.array_equal(out["normal"], sums[..., 3:6] / float(n))
    with np.errstate(invalid="ignore", divide="ignore"):
        depth = np.where(sums[..., 7] == 0, np.inf, sums[..., 6] / sums[..., 7])
    assert (sums[..., 7] == 0).sum() >= 2 and np.isinf(out["depth"][0, 0]) and np.isnan(out["depth"][2, 3])
    assert np.array_equal(out["depth"], depth, equal_nan=True)
    assert np.array_equal(out["coverage"], sums[..., 7] / float(n))
    L = pyoracle.lib()
    want = np.array([L.oracle_scale_color(float(x)) for x in out["albedo"].reshape(-1)], dtype=np.uint8)
    assert np.array_equal(out["albedo_rgb8"].reshape(-1), want)
    assert out["albedo_rgb8"][1, 2, 0] == 0 and out["albedo_rgb8"][3, 4, 1] == 255 and out["albedo_rgb8"][4, 5, 2] == 0
    # NULL outputs are skipped; bad arguments are RT_E_INVALID
    P = C.POINTER
    s = np.ascontiguousarray(sums)
    cov = np.zeros(33 * 9)
    fn = rtamd.lib().rt_features_resolve
    assert fn(s.ctypes.data_as(P(C.c_double)), 33 * 9, n, None, None, None, cov.ctypes.data_as(P(C.c_double)), None) == 0
    assert np.array_equal(cov.reshape(33, 9), out["coverage"])
    for args in ((None, 1, 1), (s.ctypes.data_as(P(C.c_double)), 0, 1), (s.ctypes.data_as(P(C.c_double)), 1, 0)):
        assert fn(*args, None, None, None, None, None) == rtamd.RT_E_INVALID


def _call(fn_async, ctx, cam, p, first, n, sums):
    L = rtamd.lib()
    P = C.POINTER
    if fn_async:
        rc = L.rt_render_features_async(ctx, C.byref(cam) if cam is not None else None,
                                        C.byref(p) if p is not None else None, first, n, 0,
                                        sums.ctypes.data if sums is not None else None, None)
    else:
        rc = L.rt_render_features(ctx, C.byref(cam) if cam is not None else None,
                                  C.byref(p) if p is not None else None, first, n, 0,
                                  sums.ctypes.data_as(P(C.c_double)) if sums is not None else None)
    return rc, L.rt_last_error().decode()


@pytest.mark.parametrize("fn_async", [False, True], ids=["blocking", "async"])
def test_invalid_arguments_without_a_device(fn_async):
    """Every RT_E_INVALID case of rt.h is returned before any HIP call: there is no device here and the ctx is
    null. The ctx is checked last, so each case is told by its message, and valid arguments reach that check."""
    cam = rtamd.camera("random_scene", 16, 8)
    sums = np.zeros((8, 16, 8))

    def params(**kw):
        a = dict(width=16, height=8, spp=1, max_depth=1, rng_mode=rtamd.RT_RNG_PHILOX, seed=1, flags=0)
        a.update({k: v for k, v in kw.items() if k in a})
        p = rtamd.make_params(a["width"], a["height"], a["spp"], a["max_depth"], a["rng_mode"], a["seed"], a["flags"])
        p.shard_count = kw.get("shard_count", 1)
        return p

    imax = 2**31 - 1
    cases = [
        ("null argument", (None, params(), 0, 1, sums)),
        ("null argument", (cam, None, 0, 1, sums)),
        ("null argument", (cam, params(), 0, 1, None)),
        ("RT_RNG_PHILOX", (cam, params(rng_mode=rtamd.RT_RNG_EXACT), 0, 1, sums)),
        ("RT_FLAG_SHARED_LIBM", (cam, params(flags=rtamd.RT_FLAG_SHARED_LIBM), 0, 1, sums)),
        ("shard_count", (cam, params(shard_count=2), 0, 1, sums)),
        ("first_sample", (cam, params(), -1, 1, sums)),
        ("first_sample", (cam, params(), 0, 0, sums)),
        ("first_sample", (cam, params(), 0, -3, sums)),
        ("first_sample", (cam, params(), imax, 1, sums)),
        ("first_sample", (cam, params(), 1, imax, sums)),
        ("2^32 pixels", (cam, params(width=65536, height=65536), 0, 1, sums)),
        ("width and height", (cam, params(width=0), 0, 1, sums)),
        # spp, max_depth and the NaN flags are not read; a sample range that ends at INT32_MAX is allowed
        ("null ctx", (cam, params(spp=0, max_depth=-1, flags=rtamd.RT_FLAG_NAN_ZERO | rtamd.RT_FLAG_NAN_CULL),
                      0, imax, sums)),
        ("null ctx", (cam, params(shard_count=0), imax - 1, 1, sums)),
        ("null ctx", (cam, params(width=65535, height=65536), 0, 1, sums)),
    ]
    for word, (c, p, first, n, s) in cases:
        rc, msg = _call(fn_async, None, c, p, first, n, s)
        assert rc == rtamd.RT_E_INVALID and word in msg, (word, rc, msg)
    info = rtamd.rt_launch_info()
    assert rtamd.lib().rt_last_feature_launch(None, C.byref(info)) == rtamd.RT_E_INVALID


def _plan(scene, W, H, flags=0, cu_count=CU_COUNT):
    fn = rtamd.lib().rt_internal_features_plan
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    p = rtamd.make_params(W, H, 1, 1, rtamd.RT_RNG_PHILOX, seed=1, flags=flags)
    info = rtamd.rt_launch_info()
    extra = np.zeros(5, dtype=np.int32)
    rc = fn(C.addressof(scene.desc), 0, cu_count, C.addressof(p), C.addressof(info), extra.ctypes.data)
    assert rc == 0, rtamd.lib().rt_last_error()
    return ({k: getattr(info, k) for k, _ in rtamd.rt_launch_info._fields_},
            dict(zip(("n_items", "entries", "n_leaves", "wide_packed", "leaf_stop"), (int(x) for x in extra))))


def test_plan_of_a_staged_spheres_world(monkeypatch):
    """random_book_one at 256 CUs: the 4-wide form with packed keys, nodes and leaves staged, within kLdsBudget;
    one wave per 8x8 block at most. RTAMD_LDS=0: from global memory. The other knobs, and the reference cull."""
    for k in ("RTAMD_LDS", "RTAMD_LEAF_LDS", "RTAMD_PACKED_KEYS", "RTAMD_WAVES", "RTAMD_WIDE"):
        monkeypatch.delenv(k, raising=False)
    scene, _ = feature_ref.world("random_book_one")
    shape = rtamd.prepare_scene(scene)
    info, extra = _plan(scene, 1200, 800)
    print(info, extra)
    assert info["variant"] == F_WIDE and info["loop"] == 2 and info["lds_staged"] == 1 and info["leaf_lds"] == 1
    assert extra["wide_packed"] == 1 and extra["n_items"] == shape["n_wide_nodes"] and extra["n_leaves"] == shape["n_leaves"]
    assert extra["entries"] == shape["wide_stack_need"] + 3 and extra["leaf_stop"] == 8  # (the render's schedule)
    assert info["waves"] == 4 and info["block"] == 1024 and info["grid"] == CU_COUNT
    assert info["dyn_lds_bytes"] == 128 * extra["n_items"] + 64 * extra["n_leaves"] + 4 * 1024 * extra["entries"]
    assert 0 < info["dyn_lds_bytes"] <= K_LDS_BUDGET
    assert info["work_items"] == 150 * 100 and info["wide_nodes"] == shape["n_wide_nodes"]
    assert info["chunk"] == 0 and info["chunk_batches"] == 1
    small, _ = _plan(scene, 37, 21)  # 5 x 3 blocks: one workgroup of 16 waves holds them
    assert small["work_items"] == 15 and small["grid"] == 1
    monkeypatch.setenv("RTAMD_LDS", "0")
    info, extra = _plan(scene, 1200, 800)
    assert info["loop"] == 2 and info["lds_staged"] == 0 and info["leaf_lds"] == 0 and info["dyn_lds_bytes"] == 0
    assert info["block"] == 128 and info["grid"] == 8 * CU_COUNT and extra["wide_packed"] == 1
    assert _plan(scene, 37, 21)[0]["grid"] == 8  # 15 blocks, two waves per workgroup
    monkeypatch.delenv("RTAMD_LDS")
    monkeypatch.setenv("RTAMD_LEAF_LDS", "0")
    info, extra = _plan(scene, 1200, 800)
    assert info["lds_staged"] == 1 and info["leaf_lds"] == 0 and extra["n_leaves"] == 0
    assert info["dyn_lds_bytes"] == 128 * extra["n_items"] + 4 * 1024 * extra["entries"]
    monkeypatch.delenv("RTAMD_LEAF_LDS")
    monkeypatch.setenv("RTAMD_PACKED_KEYS", "0")
    info, extra = _plan(scene, 1200, 800)
    assert info["lds_staged"] == 1 and info["leaf_lds"] == 1 and extra["wide_packed"] == 0
    monkeypatch.delenv("RTAMD_PACKED_KEYS")
    monkeypatch.setenv("RTAMD_WAVES", "2")
    info, _ = _plan(scene, 1200, 800)
    assert info["lds_staged"] == 1 and info["waves"] == 2 and info["block"] == 512
    monkeypatch.delenv("RTAMD_WAVES")
    # the reference cull asks for the binary tree's exact box test: the resumable walk over it
    info, extra = _plan(scene, 1200, 800, flags=rtamd.RT_FLAG_REFERENCE_CULL)
    assert info["variant"] == F_ALL | F_UV | F_MIXW and info["loop"] == 1 and info["lds_staged"] == 0
    assert info["wide_nodes"] == 0 and extra["wide_packed"] == 0


def test_plan_of_a_fog_world_and_of_deep_frames(monkeypatch):
    """A media world takes the mixed-walk form (over its re-bounded subtrees' 4-wide trees); a world whose frames
    nest deeper than RT_MAX_FRAMES the recursive walk."""
    for k in ("RTAMD_LDS", "RTAMD_LEAF_LDS", "RTAMD_PACKED_KEYS", "RTAMD_WAVES", "RTAMD_WIDE"):
        monkeypatch.delenv(k, raising=False)
    scene, _ = feature_ref.fog_world()
    shape = rtamd.prepare_scene(scene)
    assert shape["mixed_wide"] == 1 and shape["replace_ok"] == 1 and shape["ref_walk"] == 1
    info, extra = _plan(scene, 64, 48)
    print(info, extra)
    assert info["variant"] == F_ALL | F_UV | F_MIXW and info["loop"] == 1 and info["lds_staged"] == 0
    assert info["wide_nodes"] == shape["n_wide_nodes"] > 0 and info["block"] == 128 and info["grid"] == 24
    assert info["work_items"] == 48 and info["dyn_lds_bytes"] == 0 and extra["leaf_stop"] == 4
    deep, _ = feature_ref.deep_world()
    assert rtamd.prepare_scene(deep)["replace_ok"] == 0
    info, _ = _plan(deep, 64, 48)
    assert info["variant"] == F_ALL | F_UV | F_MIXW and info["loop"] == 0 and info["wide_nodes"] == 0
