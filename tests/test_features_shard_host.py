"""Sharded feature and ID passes without a device (include/rt.h rt_render_features_shard_async,
rt_render_ids_shard_async, rt_assemble_records_async, rt_assemble_records_host): every RT_E_INVALID case of the
three device entries with a null ctx (the ctx is checked last, so each case is told by its message),
rt_assemble_records_host against rtamd.shard_pixel_map with poisoned padding, and the device-free plan of a slab
pass (rt_internal_features_shard_plan) against the image-order pass's."""
import ctypes as C

import numpy as np
import pytest

import feature_ref
import rtamd

CU_COUNT = 256
IMAX = 2**31 - 1


def _params(**kw):
    a = dict(width=37, height=21, spp=1, max_depth=1, rng_mode=rtamd.RT_RNG_PHILOX, seed=1, flags=0, tile=8,
             shard_rank=0, shard_count=3)
    a.update(kw)
    return rtamd.make_params(a["width"], a["height"], a["spp"], a["max_depth"], a["rng_mode"], a["seed"], a["flags"],
                             a["tile"], a["shard_rank"], a["shard_count"])


def _chain(max_bounces=8, flags=3, max_fuzz=0.0):
    ch = rtamd.rt_feature_chain()
    ch.max_bounces, ch.flags, ch.max_fuzz = max_bounces, flags, max_fuzz
    return ch


def _call(entry, cam, p, chain, first, n, slab):
    L = rtamd.lib()
    fn = L.rt_render_ids_shard_async if entry == "ids" else L.rt_render_features_shard_async
    rc = fn(None, C.byref(cam) if cam is not None else None, C.byref(p) if p is not None else None,
            C.byref(chain) if chain is not None else None, first, n, 0, slab, None)
    return rc, L.rt_last_error().decode()


@pytest.mark.parametrize("entry", ["features", "ids"])
def test_invalid_arguments_of_the_slab_passes_without_a_device(entry):
    cam = rtamd.camera("random_scene", 37, 21)
    buf = np.zeros(64 * 64, dtype=np.uint8)
    slab = buf.ctypes.data
    name = "rt_render_ids_shard_async" if entry == "ids" else "rt_render_features_shard_async"
    cases = [
        ("null argument", (None, _params(), None, 0, 1, slab)),
        ("null argument", (cam, None, None, 0, 1, slab)),
        ("null argument", (cam, _params(), None, 0, 1, None)),  # a null slab
        # the shard geometry: what rt_shard_geometry rejects
        ("tile must be", (cam, _params(tile=12), None, 0, 1, slab)),
        ("tile must be", (cam, _params(tile=264), None, 0, 1, slab)),
        ("tile must be", (cam, _params(tile=-8), None, 0, 1, slab)),
        ("shard_rank/shard_count", (cam, _params(shard_rank=3, shard_count=3), None, 0, 1, slab)),
        ("shard_rank/shard_count", (cam, _params(shard_rank=-1), None, 0, 1, slab)),
        ("shard_rank/shard_count", (cam, _params(shard_count=-2), None, 0, 1, slab)),
        ("shard_rank/shard_count", (cam, _params(shard_rank=1, shard_count=0), None, 0, 1, slab)),
        ("shard_rank/shard_count", (cam, _params(shard_rank=1, shard_count=1), None, 0, 1, slab)),
        # what the image-order entries reject
        ("RT_RNG_PHILOX", (cam, _params(rng_mode=rtamd.RT_RNG_EXACT), None, 0, 1, slab)),
        ("RT_FLAG_SHARED_LIBM", (cam, _params(flags=rtamd.RT_FLAG_SHARED_LIBM), None, 0, 1, slab)),
        ("first_sample", (cam, _params(), None, -1, 1, slab)),
        ("first_sample", (cam, _params(), None, 0, 0, slab)),
        ("first_sample", (cam, _params(), None, IMAX, 1, slab)),
        ("first_sample", (cam, _params(), None, 1, IMAX, slab)),
        ("2^32 pixels", (cam, _params(width=65536, height=65536), None, 0, 1, slab)),
        ("2^32 slots", (cam, _params(width=65535, height=65536, tile=256, shard_count=1), None, 0, 1, slab)),
        ("width and height", (cam, _params(width=0), None, 0, 1, slab)),
        ("width and height", (cam, _params(height=-1), None, 0, 1, slab)),
        # the chain's
        ("max_bounces", (cam, _params(), _chain(max_bounces=-1), 0, 1, slab)),
        ("max_bounces", (cam, _params(), _chain(max_bounces=65), 0, 1, slab)),
        ("unknown flag bits", (cam, _params(), _chain(flags=4), 0, 1, slab)),
        ("max_fuzz", (cam, _params(), _chain(max_fuzz=float("nan")), 0, 1, slab)),
        ("max_fuzz", (cam, _params(), _chain(max_fuzz=-1.0), 0, 1, slab)),
        # valid arguments reach the ctx check: tile 0 is the default, shard_count 0 and 1 are one shard, more
        # shards than tiles, spp / max_depth / the NaN flags are not read, a range that ends at INT32_MAX
        ("null ctx", (cam, _params(tile=0), None, 0, 1, slab)),
        ("null ctx", (cam, _params(shard_count=0), None, 0, 1, slab)),
        ("null ctx", (cam, _params(shard_count=1), _chain(), 0, 1, slab)),
        ("null ctx", (cam, _params(tile=64, shard_rank=15, shard_count=16), None, 0, 1, slab)),
        ("null ctx", (cam, _params(tile=256, spp=0, max_depth=-1, flags=rtamd.RT_FLAG_NAN_ZERO), _chain(0, 0), 0, IMAX, slab)),
        ("null ctx", (cam, _params(), None, IMAX - 1, 1, slab)),
    ]
    for word, args in cases:
        rc, msg = _call(entry, *args)
        assert rc == rtamd.RT_E_INVALID and word in msg and msg.startswith(name), (word, rc, msg)


def test_invalid_arguments_of_the_merge_without_a_device():
    L = rtamd.lib()
    buf = np.zeros(64 * 64, dtype=np.uint8)
    a = buf.ctypes.data
    cases = [
        ("null argument", (None, a, a)),
        ("null argument", (_params(), None, a)),
        ("null argument", (_params(), a, None)),
        ("tile must be", (_params(tile=12), a, a)),
        ("tile must be", (_params(tile=264), a, a)),
        ("shard_rank/shard_count", (_params(shard_rank=3), a, a)),
        ("shard_rank/shard_count", (_params(shard_count=-1), a, a)),
        ("width and height", (_params(width=0), a, a)),
    ]
    for word, (p, s, i) in cases:
        rc = L.rt_assemble_records_async(None, C.byref(p) if p is not None else None, s, i, None)
        msg = L.rt_last_error().decode()
        assert rc == rtamd.RT_E_INVALID and word in msg and msg.startswith("rt_assemble_records_async"), (word, msg)
        rc = L.rt_assemble_records_host(C.byref(p) if p is not None else None, s, i)
        msg = L.rt_last_error().decode()
        assert rc == rtamd.RT_E_INVALID and word in msg and msg.startswith("rt_assemble_records_host"), (word, msg)
    assert L.rt_assemble_records_async(None, C.byref(_params()), a, a, None) == rtamd.RT_E_INVALID
    assert "null ctx" in L.rt_last_error().decode()
    with pytest.raises(rtamd.RTError):
        rtamd.assemble_records_host(np.zeros((3, 5, 8)), _params())  # (not the slab's shape)
    with pytest.raises(rtamd.RTError):
        rtamd.assemble_records_host(np.zeros((3, 320, 8), dtype=np.float32), _params())


@pytest.mark.parametrize("tile", [8, 16, 64, 256])
@pytest.mark.parametrize("size", [(1, 1), (8, 8), (37, 21), (65, 33)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_assemble_records_host_against_the_pixel_map(size, tile):
    """Slabs whose owned slots (rtamd.shard_pixel_map) hold a value made of the pixel id and whose padding holds a
    poison: every image record arrives, and the poison never appears. Doubles and ID records."""
    W, H = size
    for shards in (1, 2, 3, 5, 8, 16):
        p = _params(width=W, height=H, tile=tile, shard_count=shards)
        slab = rtamd.shard_geometry(p)[2]
        words = np.full((shards, slab, 8), 0xABABABABABABABAB, dtype=np.uint64)
        owned = 0
        for r in range(shards):
            m = rtamd.shard_pixel_map(_params(width=W, height=H, tile=tile, shard_rank=r, shard_count=shards))
            ok = m >= 0
            owned += int(ok.sum())
            words[r][ok] = (m[ok].astype(np.uint64) * np.uint64(8))[:, None] + np.arange(1, 9, dtype=np.uint64)[None, :]
        assert owned == W * H
        want = (np.arange(W * H, dtype=np.uint64) * np.uint64(8))[:, None] + np.arange(1, 9, dtype=np.uint64)[None, :]
        got = rtamd.assemble_records_host(words.view(np.float64), p)
        assert got.shape == (H, W, 8) and np.array_equal(got.view(np.uint64).reshape(-1, 8), want)
        recs = rtamd.assemble_records_host(words.view(np.uint8).reshape(shards, slab, 64).view(rtamd.ID_DTYPE)[..., 0], p)
        assert recs.shape == (H, W) and recs.dtype == rtamd.ID_DTYPE
        assert np.array_equal(recs.view(np.uint64).reshape(-1, 8), want)


def _plan(fn_name, scene, p, *mid):
    fn = getattr(rtamd.lib(), fn_name)
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p] + [C.c_int] * len(mid) + [C.c_void_p, C.c_void_p]
    info = rtamd.rt_launch_info()
    extra = np.zeros(5, dtype=np.int32)
    rc = fn(C.addressof(scene.desc), 0, CU_COUNT, C.addressof(p), *mid, C.addressof(info), extra.ctypes.data)
    assert rc == 0, rtamd.lib().rt_last_error()
    return {k: getattr(info, k) for k, _ in rtamd.rt_launch_info._fields_}, [int(x) for x in extra]


FORM_FIELDS = ("variant", "loop", "lds_staged", "leaf_lds", "waves", "block", "dyn_lds_bytes", "chunk", "wide_nodes",
               "chunk_batches")


@pytest.mark.parametrize("world", ["random_book_one", "fog", "deep"])
def test_plan_of_a_slab_pass(world, monkeypatch):
    """The slab pass takes the image-order pass's form for the same world (every field of the launch but the grid and
    the work), for the first-hit and the chain plan; work_items = the shard's tiles inside the image x (tile/8)^2:
    at one shard and tile 8 the image-order count, 0 for a shard that owns no tile."""
    for k in ("RTAMD_LDS", "RTAMD_LEAF_LDS", "RTAMD_PACKED_KEYS", "RTAMD_WAVES", "RTAMD_WIDE"):
        monkeypatch.delenv(k, raising=False)
    scene = {"fog": lambda: feature_ref.fog_world()[0], "deep": lambda: feature_ref.deep_world()[0]}.get(
        world, lambda: feature_ref.world(world)[0])()
    W, H = 37, 21
    for chain in (0, 1):
        base_p = rtamd.make_params(W, H, 1, 1, rtamd.RT_RNG_PHILOX, seed=1)
        base, base_extra = _plan_chain(scene, base_p) if chain else _plan("rt_internal_features_plan", scene, base_p)
        assert base["work_items"] == 15
        for shards, tile in ((1, 8), (2, 8), (4, 8), (3, 16), (8, 16), (3, 64), (16, 8)):
            tiles = -(-W // tile) * -(-H // tile)
            total = 0
            for r in range(shards):
                p = _params(width=W, height=H, tile=tile, shard_rank=r, shard_count=shards)
                info, extra = _plan("rt_internal_features_shard_plan", scene, p, chain)
                assert {k: info[k] for k in FORM_FIELDS} == {k: base[k] for k in FORM_FIELDS}, (shards, tile, r)
                assert extra == base_extra
                owned = len(range(r, tiles, shards))
                assert info["work_items"] == owned * (tile // 8) ** 2, (shards, tile, r, info)
                assert info["grid"] >= 1
                total += info["work_items"]
            assert total == tiles * (tile // 8) ** 2
            if (shards, tile) == (1, 8):
                assert info["work_items"] == base["work_items"] and info["grid"] == base["grid"]
            if (shards, tile) in ((8, 16), (3, 64), (16, 8)):
                assert info["work_items"] == 0  # (the last shard owns no tile)


def _plan_chain(scene, p):
    fn = rtamd.lib().rt_internal_features_chain_plan
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    ch = _chain()
    info = rtamd.rt_launch_info()
    extra = np.zeros(5, dtype=np.int32)
    rc = fn(C.addressof(scene.desc), 0, CU_COUNT, C.addressof(p), C.addressof(ch), C.addressof(info), extra.ctypes.data)
    assert rc == 0, rtamd.lib().rt_last_error()
    return {k: getattr(info, k) for k, _ in rtamd.rt_launch_info._fields_}, [int(x) for x in extra]
