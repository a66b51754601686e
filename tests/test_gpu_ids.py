"""Material-ID coverage buffers on the device (include/rt.h rt_render_ids, rt_ids_matte*, rt_ids_preview*) against
the CPU composition of tests/id_ref.py (the oracle's closest hits per segment, the chain stepping of
tests/feature_chain_ref.py, rt.h's fold restated), the device's own feature passes, and the host functions. The
outputs are integers: every comparison is of bytes. Frames of 16x8 to 65x33 pixels at 5 to 64 samples."""
import numpy as np
import pytest
import torch

import feature_chain_ref as fcr
import feature_ref
import id_ref
import rtamd
from test_error_host import same_bits
from test_ids_host import CHAIN_SETTINGS, CHAIN_WORLDS, OVERFLOW, _plan, _random_records

pytestmark = pytest.mark.gpu

KNOBS = ("RTAMD_LDS", "RTAMD_LEAF_LDS", "RTAMD_PACKED_KEYS", "RTAMD_WAVES", "RTAMD_WIDE")
MISS = rtamd.RT_ID_MISS
DIEL, METAL = rtamd.RT_CHAIN_DIELECTRIC, rtamd.RT_CHAIN_METAL
BOTH = DIEL | METAL
FLAG_NAMES = {DIEL: "dielectric", METAL: "metal", BOTH: "both"}
# every form the feature tests select through their knobs (environment, render flags)
FORMS = [({}, 0), ({"RTAMD_LDS": "0"}, 0), ({"RTAMD_LEAF_LDS": "0"}, 0), ({"RTAMD_PACKED_KEYS": "0"}, 0),
         ({"RTAMD_PACKED_KEYS": "0", "RTAMD_LDS": "0"}, 0), ({"RTAMD_WAVES": "2"}, 0), ({"RTAMD_WAVES": "4"}, 0),
         ({"RTAMD_WIDE": "0"}, 0), ({}, rtamd.RT_FLAG_REFERENCE_CULL)]


def _params(W, H, spp, flags=0, seed=1024, depth=1):
    return rtamd.make_params(W, H, spp, depth, rtamd.RT_RNG_PHILOX, seed=seed, flags=flags)


def _chain(max_bounces, flags, max_fuzz=0.0):
    return rtamd.make_feature_chain(max_bounces, bool(flags & DIEL), bool(flags & METAL), max_fuzz)


def _clear(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _miss_count(recs):
    return np.where((recs["id"] == MISS) & (recs["count"] > 0), recs["count"], 0).sum(axis=-1)


def _each_form(monkeypatch):
    for env, flags in FORMS:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        yield env, flags
        for k in env:
            monkeypatch.delenv(k)


FIRST_WORLDS = [("chains", 64, 48), ("frames", 64, 48), ("moving", 64, 48), ("chains", 37, 21)]


@pytest.mark.parametrize("name,W,H", FIRST_WORLDS, ids=[f"{w[0]}_{w[1]}x{w[2]}" for w in FIRST_WORLDS])
def test_first_hit_against_the_composition(gpu_ctx, monkeypatch, name, W, H):
    """8 samples, no chain, under every knob setting of FORMS: the records are the composition's byte for byte. On
    the same frame samples - count[RT_ID_MISS] is the first-hit feature pass's hits sum wherever other == 0 (no
    oracle in that), and on these worlds every pixel's slots hold a material of the scene."""
    _clear(monkeypatch)
    n = 8
    scene, cam = feature_ref.world(name)
    want = id_ref.first_hit_records(name, W, H, n)
    gpu_ctx.upload(scene)
    c = cam(W, H)
    hits = gpu_ctx.render_features(c, _params(W, H, n))[..., 7]
    for env, flags in _each_form(monkeypatch):
        got = gpu_ctx.render_ids(c, _params(W, H, n, flags=flags))
        info = gpu_ctx.last_feature_launch()
        print(name, env, flags, info["loop"], "records equal", _same(got, want))
        assert info["loop"] == 1 and info["work_items"] == ((W + 7) // 8) * ((H + 7) // 8)
        assert _same(got, want), (env, flags)
    keep = got["other"] == 0
    assert keep.mean() > 0.9 and np.array_equal((got["samples"] - _miss_count(got))[keep], hits[keep])
    used = got["id"][got["count"] > 0]
    assert ((used < scene.desc.n_materials) | (used == MISS)).all() and (got["samples"] == n).all()
    out = rtamd.resolve_ids(got)
    assert (out["rank_coverage"].sum(axis=-1) + out["other_coverage"] == 1.0).all()


def test_overflowing_pixels(gpu_ctx, monkeypatch):
    """The book-one cover at 16x8, 64 samples (seed 1024): a pixel spans many one-material spheres. From the
    composition alone: some pixel has other > 0 and some has exactly 7 used slots and other == 0. Then the bytes,
    in the staged 4-wide form."""
    _clear(monkeypatch)
    name, W, H, n, seed = OVERFLOW
    want = id_ref.first_hit_records(name, W, H, n, seed)
    used = (want["count"] > 0).sum(axis=-1)
    assert (want["other"] > 0).any() and ((used == 7) & (want["other"] == 0)).any()
    scene, cam = feature_ref.world(name)
    gpu_ctx.upload(scene)
    got = gpu_ctx.render_ids(cam(W, H), _params(W, H, n, seed=seed))
    assert gpu_ctx.last_feature_launch()["loop"] == 2 and gpu_ctx.last_feature_launch()["lds_staged"] == 1
    assert _same(got, want)
    hits = gpu_ctx.render_features(cam(W, H), _params(W, H, n, seed=seed))[..., 7]
    keep = got["other"] == 0
    assert np.array_equal((got["samples"] - _miss_count(got))[keep], hits[keep])


@pytest.mark.parametrize("max_bounces,flags", CHAIN_SETTINGS, ids=[f"{mb}_{FLAG_NAMES[fl]}" for mb, fl in CHAIN_SETTINGS])
@pytest.mark.parametrize("name,W,H", CHAIN_WORLDS, ids=[f"{w[0]}_{w[1]}x{w[2]}" for w in CHAIN_WORLDS])
def test_chain_against_the_composition(gpu_ctx, monkeypatch, name, W, H, max_bounces, flags):
    """8 samples, max_fuzz 0. At most 0.1 % of pixels are left out as undecided (asserted first); on every other
    pixel the records are the composition's byte for byte, and when none is left out rt_last_feature_chain's five
    counts are the composition's. The 37x21 frame's partial 8x8 blocks put idle lanes next to lanes in chains."""
    _clear(monkeypatch)
    n = 8
    scene, cam = fcr.world(name)
    comp = id_ref.chain_ids(name, W, H, n, max_bounces, flags)
    want, keep, kc = id_ref.chain_records(name, W, H, n, max_bounces, flags), ~comp.left_out, comp.counts()
    assert comp.left_out.mean() <= 0.001
    assert kc["bounces"] > 0  # (the case follows something)
    gpu_ctx.upload(scene)
    got = gpu_ctx.render_ids(cam(W, H), _params(W, H, n), chain=_chain(max_bounces, flags))
    kd = gpu_ctx.last_feature_chain()
    print(f"{name} {W}x{H} max_bounces {max_bounces} flags {flags}: composition {kc}, device {kd}, left out "
          f"{int(comp.left_out.sum())}, records equal {float((got[keep] == want[keep]).mean()):.5f}")
    assert _same(got[keep], want[keep])
    if keep.all():
        assert kd == kc
    assert kd["samples"] == W * H * n == kd["ended_surface"] + kd["ended_miss"] + kd["ended_cap"]
    assert kd["ended_miss"] == int(_miss_count(got).sum())
    assert not _same(got, id_ref.first_hit_records(name, W, H, n))


@pytest.mark.parametrize("name,W,H,n,walk", [("chains", 64, 48, 8, 1), ("deep", 40, 27, 3, 0), ("random_book_one", 48, 32, 6, 2)])
def test_zero_bounces_no_flags_and_no_chain_are_one(gpu_ctx, monkeypatch, name, W, H, n, walk):
    """max_bounces = 0 with every flag, flags = 0 with max_bounces = 8, and chain = NULL: identical bytes, on one
    world per walk form; the chain counts follow no scatter."""
    _clear(monkeypatch)
    if name == "deep":
        scene, c = feature_ref.deep_world()
    else:
        scene, cam = feature_ref.world(name)
        c = cam(W, H)
    gpu_ctx.upload(scene)
    want = gpu_ctx.render_ids(c, _params(W, H, n))
    assert gpu_ctx.last_feature_launch()["loop"] == walk
    hits = int((want["samples"] - _miss_count(want)).sum())
    assert (want["other"] == 0).all() or name == "random_book_one"
    for mb, flags in ((0, BOTH), (8, 0)):
        got = gpu_ctx.render_ids(c, _params(W, H, n), chain=_chain(mb, flags, 0.5))
        assert gpu_ctx.last_feature_launch()["loop"] == walk
        assert _same(got, want), (mb, flags)
        k = gpu_ctx.last_feature_chain()
        assert k["samples"] == W * H * n and k["bounces"] == 0
        if (want["other"] == 0).all():
            assert k["ended_miss"] == W * H * n - hits


def test_sample_ranges_and_accumulate(gpu_ctx, monkeypatch):
    """[0, 3) then [3, 8) with `accumulate` is [0, 8) byte for byte, with a chain and without; so are 8 passes of
    one sample; samples 3..7 alone are the composition's fold of those samples."""
    _clear(monkeypatch)
    W, H, n, mb = 37, 21, 8, 8
    scene, cam = fcr.world("chains")
    comp = id_ref.chain_ids("chains", W, H, n, mb, BOTH)
    assert not comp.left_out.any()
    gpu_ctx.upload(scene)
    c = cam(W, H)
    for ch, ids in ((None, id_ref.first_hit_ids("chains", W, H, n)), (_chain(mb, BOTH), comp.ids)):
        whole = gpu_ctx.render_ids(c, _params(W, H, n), chain=ch)
        assert _same(whole, id_ref.records(ids))
        part = gpu_ctx.render_ids(c, _params(W, H, 1000), first_sample=0, n_samples=3, chain=ch)
        assert _same(part, id_ref.records(ids, 0, 3))
        back = gpu_ctx.render_ids(c, _params(W, H, 1), first_sample=3, n_samples=5, chain=ch, accumulate=part)
        assert back is part and _same(part, whole)
        one = None
        for s in range(n):
            one = gpu_ctx.render_ids(c, _params(W, H, n), first_sample=s, n_samples=1, chain=ch, accumulate=one)
        assert _same(one, whole)
        alone = gpu_ctx.render_ids(c, _params(W, H, n), first_sample=3, n_samples=5, chain=ch)
        assert _same(alone, id_ref.records(ids, 3, 5))
    assert gpu_ctx.last_feature_chain()["samples"] == W * H * 5  # (the counts are the last chain pass's)
    with pytest.raises(rtamd.RTError):
        gpu_ctx.render_ids(c, _params(W, H, n), accumulate=np.zeros((W, H), dtype=rtamd.ID_DTYPE))
    with pytest.raises(rtamd.RTError):
        gpu_ctx.render_ids(c, _params(W, H, n), accumulate=np.zeros((H, W, 8)))


def test_forms_give_the_same_bytes(gpu_ctx, monkeypatch):
    """random_book_one runs the staged 4-wide form at 3 waves per SIMD; at 4 and 2 waves, from global memory, without
    the staged leaf table, with the key / reference pairs, over the binary tree and under the reference cull the
    bytes and the chain counts are the same, without a chain (the composition's bytes) and with one, and every
    launch is the one rt_internal_ids_plan returns without a device."""
    _clear(monkeypatch)
    W, H, n = 48, 32, 6
    scene, cam = feature_ref.world("random_book_one")
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    gpu_ctx.upload(scene)
    c, ch = cam(W, H), _chain(8, BOTH)
    base0 = gpu_ctx.render_ids(c, _params(W, H, n))
    info = gpu_ctx.last_feature_launch()
    print("default:", info)
    assert info["variant"] == 256 and info["loop"] == 2 and info["lds_staged"] == 1 and info["leaf_lds"] == 1
    assert info["waves"] == 3 and info["block"] == 768
    assert _same(base0, id_ref.first_hit_records("random_book_one", W, H, n))
    base8 = gpu_ctx.render_ids(c, _params(W, H, n), chain=ch)
    counts = gpu_ctx.last_feature_chain()
    assert counts["bounces"] > 0 and not _same(base0, base8)
    expect = [dict(loop=2, lds_staged=1, block=768), dict(loop=2, lds_staged=0, block=128),
              dict(loop=2, lds_staged=1, leaf_lds=0), dict(loop=2, lds_staged=1, leaf_lds=1),
              dict(loop=2, lds_staged=0), dict(loop=2, lds_staged=1, block=512), dict(loop=2, lds_staged=1, block=1024),
              dict(loop=1, lds_staged=0), dict(loop=1, lds_staged=0)]
    for (env, flags), exp in zip(_each_form(monkeypatch), expect):
        p = _params(W, H, n, flags=flags)
        got0 = gpu_ctx.render_ids(c, p)
        info = gpu_ctx.last_feature_launch()
        print(env, flags, info)
        assert {k: info[k] for k in exp} == exp
        assert info == _plan_on(scene, W, H, None, flags, cu)
        got8 = gpu_ctx.render_ids(c, p, chain=ch)
        assert gpu_ctx.last_feature_launch() == info == _plan_on(scene, W, H, ch, flags, cu)
        assert _same(got0, base0) and _same(got8, base8), (env, flags)
        assert gpu_ctx.last_feature_chain() == counts


def _plan_on(scene, W, H, ch, flags, cu):
    return _plan(scene, W, H, ch, flags, cu_count=cu)[0]


def test_async_pass_into_device_memory(gpu_ctx, monkeypatch):
    """rt_render_ids_async on a caller's stream into a torch tensor, accumulating onto it: the blocking call's
    bytes; rt_last_feature_chain drains the stream; the matte and the preview queued behind it on the same stream
    are the host functions' bytes."""
    _clear(monkeypatch)
    W, H, n = 37, 21, 5
    scene, cam = fcr.world("chains")
    gpu_ctx.upload(scene)
    c, p, ch = cam(W, H), _params(W, H, n), _chain(8, BOTH)
    want = gpu_ctx.render_ids(c, p, chain=ch)
    want0 = gpu_ctx.render_ids(c, p)
    d = torch.full((H, W, 64), 7, dtype=torch.uint8, device="cuda:0")
    d0 = torch.zeros((H, W, 64), dtype=torch.uint8, device="cuda:0")
    cov = torch.zeros((H, W), dtype=torch.float64, device="cuda:0")
    u8 = torch.zeros((H, W), dtype=torch.uint8, device="cuda:0")
    rgb = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda:0")
    mats = [0, 3, 5, MISS]
    st = torch.cuda.Stream(device=0)
    with torch.cuda.stream(st):
        gpu_ctx.render_ids_async(c, p, d0.data_ptr(), stream=st.cuda_stream)
        gpu_ctx.render_ids_async(c, p, d.data_ptr(), 0, 2, chain=ch, accumulate=False, stream=st.cuda_stream)
        gpu_ctx.render_ids_async(c, p, d.data_ptr(), 2, 3, chain=ch, accumulate=True, stream=st.cuda_stream)
        gpu_ctx.id_matte(d.data_ptr(), mats, pixels=W * H, d_out_cov=cov.data_ptr(), d_out_u8=u8.data_ptr(),
                         stream=st.cuda_stream)
        gpu_ctx.id_preview(d.data_ptr(), pixels=W * H, d_out_rgb8=rgb.data_ptr(), stream=st.cuda_stream)
    k = gpu_ctx.last_feature_chain()  # (no synchronize before it)
    assert k["samples"] == W * H * 3 and k["samples"] == k["ended_surface"] + k["ended_miss"] + k["ended_cap"]
    st.synchronize()
    got = d.cpu().numpy().reshape(H, W, 64).view(rtamd.ID_DTYPE).reshape(H, W)
    got0 = d0.cpu().numpy().reshape(H, W, 64).view(rtamd.ID_DTYPE).reshape(H, W)
    assert _same(got, want) and _same(got0, want0) and not _same(want, want0)
    cov_w, u8_w = rtamd.id_matte(want, mats)
    assert cov.cpu().numpy().tobytes() == cov_w.tobytes() and np.array_equal(u8.cpu().numpy(), u8_w)
    assert 0 < cov_w.mean() < 1
    assert np.array_equal(rgb.cpu().numpy(), rtamd.id_preview(want))


def test_renders_and_feature_passes_around_an_id_pass(gpu_ctx, monkeypatch):
    """An id pass (without and with a chain) between two renders, two first-hit passes and two chain feature passes
    leaves their bytes, what rt_last_launch reports and the chain counts of the feature pass unchanged. A second id
    pass, matte and preview of one size allocate nothing."""
    _clear(monkeypatch)
    W, H = 48, 32
    scene, cam = feature_ref.world("random_book_one")
    gpu_ctx.upload(scene)
    c, p, ch = cam(W, H), _params(W, H, 6, depth=8), _chain(8, BOTH)
    rgb0, lin0, _ = gpu_ctx.render(c, p, linear=True)
    launch0 = gpu_ctx.last_launch()
    f0 = gpu_ctx.render_features(c, p)
    c0 = gpu_ctx.render_features(c, p, chain=ch)
    k0 = gpu_ctx.last_feature_chain()
    i0 = gpu_ctx.render_ids(c, p)
    assert gpu_ctx.last_feature_chain() == k0  # (a pass without a chain leaves the last chain pass's counts)
    i8 = gpu_ctx.render_ids(c, p, chain=ch)
    k8 = gpu_ctx.last_feature_chain()
    assert k8 == k0  # (the same chains)
    rgb1, lin1, _ = gpu_ctx.render(c, p, linear=True)
    f1 = gpu_ctx.render_features(c, p)
    c1 = gpu_ctx.render_features(c, p, chain=ch)
    assert np.array_equal(rgb0, rgb1) and same_bits(lin0, lin1)
    assert gpu_ctx.last_launch() == launch0 and gpu_ctx.last_feature_chain() == k0
    assert same_bits(f0, f1) and same_bits(c0, c1)
    assert _same(gpu_ctx.render_ids(c, p), i0) and gpu_ctx.last_id_allocs() == 0
    assert _same(gpu_ctx.render_ids(c, p, chain=ch), i8) and gpu_ctx.last_id_allocs() == 0
    ids = [1, 2, MISS]
    first = gpu_ctx.id_matte(i0, ids)
    again = gpu_ctx.id_matte(i0, [4])
    assert gpu_ctx.last_id_allocs() == 0 and first[0].tobytes() == rtamd.id_matte(i0, ids)[0].tobytes()
    assert again[0].tobytes() == rtamd.id_matte(i0, [4])[0].tobytes()
    gpu_ctx.id_preview(i0)
    assert np.array_equal(gpu_ctx.id_preview(i0), rtamd.id_preview(i0)) and gpu_ctx.last_id_allocs() == 0


def test_fog_world(gpu_ctx, monkeypatch):
    """feature_ref.fog_world (media; the mixed walk) has no oracle composition, as for features: per pixel
    samples - miss count is the feature pass's hits (no slot overflows there), every medium's phase material
    appears as an id, and with a chain the counts add up and the misses are the records' RT_ID_MISS counts."""
    _clear(monkeypatch)
    W, H, n = 64, 48, 8
    scene, cam = feature_ref.fog_world()
    d = scene.desc
    phase = {int(d.nodes[i].b) for i in range(d.n_nodes) if d.nodes[i].type == rtamd.RT_NODE_CONSTANT_MEDIUM}
    assert len(phase) == 3
    gpu_ctx.upload(scene)
    hits = gpu_ctx.render_features(cam, _params(W, H, n))[..., 7]
    got = gpu_ctx.render_ids(cam, _params(W, H, n))
    assert gpu_ctx.last_feature_launch()["loop"] == 1
    assert (got["other"] == 0).all() and np.array_equal(got["samples"] - _miss_count(got), hits)
    seen = {int(x) for x in np.unique(got["id"][got["count"] > 0])}
    print("fog world: ids seen", sorted(seen), "phase materials", sorted(phase))
    assert phase <= seen and seen - {MISS} <= set(range(d.n_materials))
    chained = gpu_ctx.render_ids(cam, _params(W, H, n), chain=_chain(8, BOTH, 0.2))
    k = gpu_ctx.last_feature_chain()
    assert k["samples"] == W * H * n == k["ended_surface"] + k["ended_miss"] + k["ended_cap"] and k["bounces"] > 0
    assert k["ended_miss"] == int(_miss_count(chained).sum()) and not _same(chained, got)
    feat = gpu_ctx.render_features(cam, _params(W, H, n), chain=_chain(8, BOTH, 0.2))
    assert gpu_ctx.last_feature_chain() == k
    assert np.array_equal((chained["samples"] - _miss_count(chained))[chained["other"] == 0], feat[..., 7][chained["other"] == 0])


@pytest.mark.parametrize("W,H", [(1, 1), (37, 21), (65, 33)])
def test_device_matte_and_preview_are_the_hosts(gpu_ctx, W, H):
    """rt_ids_matte and rt_ids_preview (through the device) against the host functions, bit for bit, over random
    folded records (a zero record among them) with lists of 1, 3 and 1024 ids."""
    rng = np.random.default_rng(W * 100 + H)
    recs = _random_records(rng, (H, W))
    if W > 1:
        recs[0, 0] = np.zeros((), dtype=rtamd.ID_DTYPE)[()]
    present = np.unique(recs["id"][recs["count"] > 0]) if (recs["count"] > 0).any() else np.array([5], dtype=np.uint32)
    big = sorted(set(int(x) for x in rng.choice(3000, size=1023, replace=False)) | {MISS} | {int(present[0])})[-1024:]
    three = sorted(([int(present[0])] + [x for x in (1, 2, MISS) if x != int(present[0])])[:3])
    lists = [[int(present[0])], three, big]
    assert [len(x) for x in lists] == [1, 3, 1024]
    for lst in lists:
        cov_g, u8_g = gpu_ctx.id_matte(recs, lst)
        cov_w, u8_w = rtamd.id_matte(recs, lst)
        assert cov_g.tobytes() == cov_w.tobytes() and np.array_equal(u8_g, u8_w), len(lst)
    assert np.array_equal(gpu_ctx.id_preview(recs), rtamd.id_preview(recs))


def test_error_codes(gpu_ctx):
    """With a live ctx: RT_E_INVALID for the cases test_ids_host.py makes with a null one, RT_E_STATE without a
    scene (a fresh ctx), and the Python wrappers raise."""
    import ctypes as C
    L = rtamd.lib()
    cam, p = rtamd.camera("random_scene", 16, 8), _params(16, 8, 1)
    recs = np.zeros((8, 16), dtype=rtamd.ID_DTYPE)
    rp = C.c_void_p(recs.ctypes.data)
    fresh = rtamd.Context(0)
    try:
        assert L.rt_render_ids(fresh._h, C.byref(cam), C.byref(p), None, 0, 1, 0, rp) == rtamd.RT_E_STATE
        assert L.rt_render_ids_async(fresh._h, C.byref(cam), C.byref(p), None, 0, 1, 0, rp, None) == rtamd.RT_E_STATE
        assert "rt_render_ids" in L.rt_last_error().decode()
        cov, u8 = fresh.id_matte(recs, [0])  # (the resolve calls need no scene)
        assert (cov == 0).all() and (u8 == 0).all() and (fresh.id_preview(recs) == 0).all()
    finally:
        fresh.close()
    h = gpu_ctx._h
    bad = rtamd.make_feature_chain(65)
    assert L.rt_render_ids(h, C.byref(cam), C.byref(p), C.byref(bad), 0, 1, 0, rp) == rtamd.RT_E_INVALID
    assert L.rt_render_ids(h, C.byref(cam), C.byref(p), None, 0, 0, 0, rp) == rtamd.RT_E_INVALID
    assert L.rt_render_ids(h, C.byref(cam), C.byref(p), None, 0, 1, 0, None) == rtamd.RT_E_INVALID
    p2 = _params(16, 8, 1)
    p2.shard_count = 2
    assert L.rt_render_ids(h, C.byref(cam), C.byref(p2), None, 0, 1, 0, rp) == rtamd.RT_E_INVALID
    for lst in ([], [2, 1], [1, 1], list(range(1025))):
        with pytest.raises(rtamd.RTError):
            gpu_ctx.id_matte(recs, lst)
    with pytest.raises(rtamd.RTError):
        gpu_ctx.id_matte(0x1000, [1], pixels=0, d_out_u8=0x1000)
    with pytest.raises(rtamd.RTError):
        gpu_ctx.id_preview(0x1000, pixels=4, d_out_rgb8=0)
