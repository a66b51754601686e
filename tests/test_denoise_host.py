"""The feature-guided denoiser without a GPU (include/rt.h, rt_denoise_host): the bindings, the host function
against a numpy restatement of rt.h's text bit for bit (one vectorised pass per tap, in the stated tap order), and
the properties the definition implies: constants and hard edges are preserved exactly, one guides-only iteration
is the separable B3 convolution, invalid pixels neither spread nor move unless RT_DENOISE_FILL asks for it."""
import ctypes as C
import itertools

import numpy as np
import pytest

import rtamd
from test_error_host import same_bits

DEMOD, GUIDES, FILL = rtamd.RT_DENOISE_DEMODULATE, rtamd.RT_DENOISE_GUIDES_ONLY, rtamd.RT_DENOISE_FILL
ALL_FLAGS = tuple(range(8))
B3 = (0.375, 0.25, 0.0625)  # k[|d|]


def synthetic(W, H, seed, n=4, sprinkle=True):
    """Seeded inputs of a W x H image: colour, an se map and the feature sums of n samples (pixels without a hit
    among them), with NaN and +inf colour pixels and non-finite se channels sprinkled in."""
    rng = np.random.default_rng(seed)
    color = rng.random((H, W, 3))
    se = 0.1 * rng.random((H, W, 3))
    feat = np.zeros((H, W, 8))
    feat[..., 0:3] = n * rng.random((H, W, 3))
    feat[..., 0:3][rng.random((H, W)) < 0.1] = 0.0  # (black albedo: the 1e-3 floor)
    feat[..., 0:3][rng.random((H, W)) < 0.1] *= 9.0  # (an emitter's radiance: the cap at 1)
    nrm = rng.normal(size=(H, W, 3))
    feat[..., 3:6] = n * np.round(nrm / np.linalg.norm(nrm, axis=-1, keepdims=True) * 2) / 2  # (few distinct normals)
    hits = rng.integers(0, n + 1, (H, W)).astype(np.float64)
    feat[..., 7] = hits
    feat[..., 6] = hits * (1.0 + np.round(rng.random((H, W)) * 4) / 16)  # (depths that cluster)
    if sprinkle:
        color[rng.random((H, W)) < 0.08] = np.nan
        color[rng.random((H, W)) < 0.04, 1] = np.inf
        color[rng.random((H, W)) < 0.04, 2] = np.nan
        se[rng.random((H, W)) < 0.05, 0] = np.nan
        se[rng.random((H, W)) < 0.03] = np.inf
    return color, se, feat


def falloff(x):
    return np.where(x < 1.0, (1.0 - x) * (1.0 - x), 0.0)


def luma(c):
    return (0.2126 * c[..., 0] + 0.7152 * c[..., 1]) + 0.0722 * c[..., 2]


def scale_color(x):
    """scaleColor as rt.h's outputs take it: NaN -> 0, +inf -> 255."""
    with np.errstate(all="ignore"):
        s = np.sqrt(x)
        cl = np.where(s < 0.0, 0.0, np.where(s > 0.999, 0.999, s))
        f = np.floor(256 * cl)
    return np.where(f == f, np.nan_to_num(f), 0.0).astype(np.uint8)


def restate(p, color, se, feat):
    """rt.h's definition in numpy, operation by operation (IEEE fp64, no contraction): (linear, rgb8, variance,
    stats)."""
    H, W = p.height, p.width
    color, feat = np.asarray(color, np.float64), np.asarray(feat, np.float64)
    n = np.float64(p.feature_samples)
    with np.errstate(all="ignore"):
        N = feat[..., 3:6] / n
        hits = feat[..., 7]
        Z = np.where(hits == 0.0, 0.0, feat[..., 6] / hits)
        A = feat[..., 0:3] / n
        a = np.where(A > 1e-3, np.where(A < 1.0, A, 1.0), 1e-3)
        valid_in = np.isfinite(color).all(-1)
        demod = valid_in[..., None] & bool(p.flags & DEMOD)
        c = np.where(demod, color / a, color)
        V = np.zeros((H, W))
        if se is not None:
            se = np.asarray(se, np.float64)
            e = np.where(demod, se / a, se)
            t0, t1, t2 = 0.2126 * e[..., 0], 0.7152 * e[..., 1], 0.0722 * e[..., 2]
            v = (t0 * t0 + t1 * t1) + t2 * t2
            V = np.where(np.isfinite(se).all(-1) & np.isfinite(v), v, 0.0)
        rn = np.float64(1.0) / (np.float64(p.sigma_normal) * np.float64(p.sigma_normal))
        for it in range(p.iterations):
            s = 1 << it
            valid = np.isfinite(c).all(-1)
            L = luma(c)
            rz = 1.0 / (p.sigma_depth * Z + 1e-12)
            rc = 1.0 / (p.sigma_color * np.sqrt(V) + p.color_floor)
            acc, wsum, vacc = np.zeros((H, W, 3)), np.zeros((H, W)), np.zeros((H, W))
            centre = valid | bool(p.flags & FILL)
            use_c = valid & (not p.flags & GUIDES)
            for dy, dx in itertools.product(range(-2, 3), repeat=2):  # dy outer, dx inner
                y0, y1, x0, x1 = max(0, -s * dy), min(H, H - s * dy), max(0, -s * dx), min(W, W - s * dx)
                if y0 >= y1 or x0 >= x1:
                    continue
                P = (slice(y0, y1), slice(x0, x1))
                Q = (slice(y0 + s * dy, y1 + s * dy), slice(x0 + s * dx, x1 + s * dx))
                h = np.float64(B3[abs(dx)]) * np.float64(B3[abs(dy)])
                d = N[P] - N[Q]
                wn = falloff(((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) * rn)
                wz = falloff(np.abs(Z[P] - Z[Q]) * rz[P])
                wc = np.where(use_c[P], falloff(np.abs(L[P] - L[Q]) * rc[P]), 1.0)
                w = ((h * wn) * wz) * wc
                take = centre[P] & valid[Q]
                acc[P] = np.where(take[..., None], acc[P] + w[..., None] * c[Q], acc[P])
                wsum[P] = np.where(take, wsum[P] + w, wsum[P])
                vacc[P] = np.where(take, vacc[P] + (w * w) * V[Q], vacc[P])
            upd = wsum > 0.0
            c = np.where(upd[..., None], acc / wsum[..., None], c)
            V = np.where(upd, vacc / (wsum * wsum), V)
        valid_end = np.isfinite(c).all(-1)
        out = np.where(valid_end[..., None], c * a, c) if p.flags & DEMOD else c
    valid_out = np.isfinite(out).all(-1)
    stats = {"pixels": H * W, "invalid_in": int((~valid_in).sum()), "invalid_out": int((~valid_out).sum()),
             "filled": int((~valid_in & valid_out).sum())}
    return out, scale_color(out), V, stats


def counts(stats):
    return {k: stats[k] for k in ("pixels", "invalid_in", "invalid_out", "filled")}


def flat_features(W, H, n=2, albedo=0.5):
    """One plane seen head-on: the same albedo, normal and depth in every pixel."""
    feat = np.zeros((H, W, 8))
    feat[..., 0:3] = n * albedo
    feat[..., 5] = n
    feat[..., 6] = n * 3.0
    feat[..., 7] = n
    return feat


def test_bindings_and_struct_sizes():
    L = rtamd.lib()
    assert L.rt_abi_version() == 1
    for name in ("rt_denoise_host", "rt_denoise", "rt_denoise_async", "rt_frame_denoise", "rt_last_denoise"):
        assert hasattr(L, name) and name in rtamd.EXPORTED
    assert C.sizeof(rtamd.rt_denoise_params) == 56 and rtamd.rt_denoise_params.sigma_color.offset == 24
    assert C.sizeof(rtamd.rt_denoise_stats) == 40 and rtamd.rt_denoise_stats.kernel_ms.offset == 32
    assert C.sizeof(rtamd.rt_denoise_info) == 16
    assert (DEMOD, GUIDES, FILL) == (1, 2, 4)
    assert hasattr(rtamd.ProgressiveFrame, "denoise") and hasattr(rtamd.Context, "denoise")
    assert hasattr(rtamd.Context, "denoise_async")
    p = rtamd.make_denoise_params(8, 4, 3)
    assert (p.width, p.height, p.feature_samples, p.iterations, p.flags) == (8, 4, 3, 5, 0)
    assert min(p.sigma_color, p.color_floor, p.sigma_normal, p.sigma_depth) > 0


@pytest.mark.parametrize("iterations", [1, 5])
@pytest.mark.parametrize("shape", [(1, 1), (5, 3), (37, 21)])
def test_host_equals_the_restatement_bit_for_bit(shape, iterations):
    """Every flag combination, with and without se, NaN and +inf pixels sprinkled in; at 37x21 the fifth
    iteration's stride of 16 puts most taps outside the image."""
    W, H = shape
    color, se, feat = synthetic(W, H, seed=100 * W + iterations)
    if (W, H) == (1, 1):
        color[0, 0] = (0.25, 0.5, 0.125)  # (the lone pixel valid here, invalid below)
    cases = [(color, e) for e in (se, None)]
    if (W, H) == (1, 1):
        cases.append((np.full((1, 1, 3), np.nan), se))
    for (col, e), flags in itertools.product(cases, ALL_FLAGS):
        p = rtamd.make_denoise_params(W, H, 4, iterations=iterations, flags=flags)
        rgb, lin, stats = rtamd.denoise_host(p, col, e, feat)
        lin_v, var = rtamd.denoise_host_variance(p, col, e, feat)
        want_lin, want_rgb, want_var, want_stats = restate(p, col, e, feat)
        assert same_bits(lin, want_lin), (flags, e is None)
        assert same_bits(lin_v, want_lin) and same_bits(var, want_var), (flags, e is None)
        assert np.array_equal(rgb, want_rgb)
        assert counts(stats) == want_stats and stats["kernel_ms"] == 0.0


def test_sprinkled_inputs_exercise_what_they_claim():
    """The synthetic inputs hold what the restatement test says they cover."""
    color, se, feat = synthetic(37, 21, seed=3705)
    assert np.isnan(color).any() and np.isposinf(color).any() and np.isfinite(color).all(-1).mean() > 0.7
    assert (~np.isfinite(se)).any() and (feat[..., 7] == 0).any() and (feat[..., 0:3] == 0).any()
    assert (feat[..., 0:3] > 4.0).any()  # (n = 4: an albedo above 1)
    p = rtamd.make_denoise_params(37, 21, 4)
    out = rtamd.denoise_host(p, color, se, feat)[1]
    ok = np.isfinite(color).all(-1)
    assert not same_bits(out[ok], color[ok])  # (the filter does move pixels on this data)


@pytest.mark.parametrize("flags", [0, DEMOD, GUIDES | FILL])
def test_constant_image_is_returned_exactly(flags):
    W, H = 23, 11
    color = np.full((H, W, 3), 0.5)
    se = np.full((H, W, 3), 0.01)
    p = rtamd.make_denoise_params(W, H, 2, flags=flags)
    rgb, lin, stats = rtamd.denoise_host(p, color, se, flat_features(W, H))
    assert same_bits(lin, color) and (rgb == scale_color(np.float64(0.5))).all()
    assert counts(stats) == {"pixels": W * H, "invalid_in": 0, "invalid_out": 0, "filled": 0}


def test_two_half_planes_keep_their_edge_exactly():
    """Orthogonal unit normals and sigma_normal = 1: |N_p - N_q|^2 = 2, so no weight crosses the edge and each
    half, being constant, is returned exactly."""
    W, H, n = 24, 13, 2
    color = np.zeros((H, W, 3))
    color[:, :11], color[:, 11:] = 0.25, 0.75
    feat = flat_features(W, H, n)
    feat[..., 3:6] = 0.0
    feat[:, :11, 3] = n
    feat[:, 11:, 4] = n
    for flags in (0, GUIDES):
        p = rtamd.make_denoise_params(W, H, n, flags=flags, sigma_normal=1.0)
        assert same_bits(rtamd.denoise_host(p, color, None, feat)[1], color)
    # (with a wide normal falloff the same call does blur the edge: the test above is not vacuous)
    p = rtamd.make_denoise_params(W, H, n, flags=GUIDES, sigma_normal=4.0)
    assert not same_bits(rtamd.denoise_host(p, color, None, feat)[1], color)


def test_one_guides_only_iteration_is_the_b3_convolution():
    """Flat guides, RT_DENOISE_GUIDES_ONLY, one iteration: every weight is h, they add up to 1 exactly, and an
    interior pixel is the separable B3 convolution of the input to 1e-14 relative (25 products and sums at 2^-53
    each); its variance is V * sum(h^2) = V * 0.2734375^2 to the same bound."""
    W, H = 19, 14
    rng = np.random.default_rng(7)
    color = 0.1 + rng.random((H, W, 3))
    se = np.full((H, W, 3), 0.03)
    p = rtamd.make_denoise_params(W, H, 2, iterations=1, flags=GUIDES)
    lin, var = rtamd.denoise_host_variance(p, color, se, flat_features(W, H))
    k = np.array([0.0625, 0.25, 0.375, 0.25, 0.0625])
    rows = sum(k[i] * color[:, i:W - 4 + i] for i in range(5))
    want = sum(k[j] * rows[j:H - 4 + j] for j in range(5))
    got = lin[2:H - 2, 2:W - 2]
    assert np.all(np.abs(got - want) <= 1e-14 * np.abs(want))
    v = (0.2126 * 0.03) ** 2 + (0.7152 * 0.03) ** 2 + (0.0722 * 0.03) ** 2
    want_v = v * 0.2734375 ** 2
    assert np.all(np.abs(var[2:H - 2, 2:W - 2] - want_v) <= 1e-14 * want_v)


def test_nan_pixels_stay_put_without_fill():
    W, H = 37, 21
    color, se, feat = synthetic(W, H, seed=11)
    bad = ~np.isfinite(color).all(-1)
    assert bad.any()
    for flags in (0, DEMOD, GUIDES, DEMOD | GUIDES):
        p = rtamd.make_denoise_params(W, H, 4, flags=flags)
        _, lin, stats = rtamd.denoise_host(p, color, se, feat)
        assert np.array_equal(~np.isfinite(lin).all(-1), bad)
        assert same_bits(lin[bad], color[bad])  # (passed through bit for bit)
        assert stats["invalid_in"] == stats["invalid_out"] == int(bad.sum()) and stats["filled"] == 0
        # a NaN pixel's payload does not matter to anyone else: +inf in its place changes no other pixel's bits
        other = color.copy()
        other[np.isnan(color).any(-1)] = np.inf
        lin2 = rtamd.denoise_host(p, other, se, feat)[1]
        assert same_bits(lin2[~bad], lin[~bad])


@pytest.mark.parametrize("flags", [FILL, FILL | DEMOD, FILL | GUIDES])
def test_fill_replaces_every_invalid_pixel_on_flat_guides(flags):
    """Flat guides and at least one valid pixel in every 5x5 neighbourhood: one iteration fills every hole."""
    W, H = 21, 17
    rng = np.random.default_rng(5)
    color = 0.2 + rng.random((H, W, 3))
    holes = rng.random((H, W)) < 0.3
    holes[::3, ::3] = False  # (a valid pixel within two pixels of everyone)
    color[holes] = np.nan
    color[holes & (rng.random((H, W)) < 0.5), 0] = np.inf
    for iterations in (1, 3):
        p = rtamd.make_denoise_params(W, H, 2, iterations=iterations, flags=flags)
        _, lin, stats = rtamd.denoise_host(p, color, None, flat_features(W, H))
        assert np.isfinite(lin).all()
        assert stats["invalid_in"] == int(holes.sum()) == stats["filled"] and stats["invalid_out"] == 0
        assert lin.min() >= 0.2 - 1e-12 and lin.max() <= 1.2 + 1e-12  # (a weighted mean of valid pixels)


def test_invalid_arguments():
    L = rtamd.lib()
    W, H = 4, 3
    color, _, feat = synthetic(W, H, seed=1, sprinkle=False)
    out = np.zeros((H, W, 3))
    P = C.POINTER
    ptr = lambda a: a.ctypes.data_as(P(C.c_double))

    def call(p, c=color, f=feat, o=out):
        return L.rt_denoise_host(C.byref(p) if p is not None else None, ptr(c) if c is not None else None, None,
                                 ptr(f) if f is not None else None, ptr(o) if o is not None else None, None, None)

    good = rtamd.make_denoise_params(W, H, 2)
    assert call(good) == rtamd.RT_OK
    assert call(None) == rtamd.RT_E_INVALID
    assert call(good, c=None) == call(good, f=None) == call(good, o=None) == rtamd.RT_E_INVALID
    bad = [dict(width=0), dict(width=-1), dict(height=0), dict(iterations=0), dict(iterations=9),
           dict(feature_samples=0), dict(flags=8), dict(flags=1 << 31), dict(width=65536, height=32768)]
    for name in ("sigma_color", "color_floor", "sigma_normal", "sigma_depth"):
        bad += [{name: v} for v in (0.0, -1.0, float("nan"), float("inf"))]
    for change in bad:
        p = rtamd.make_denoise_params(W, H, 2)
        for k, v in change.items():
            setattr(p, k, v)
        assert call(p) == rtamd.RT_E_INVALID, change
        assert b"rt_denoise_host" in L.rt_last_error()
    # the device calls check the same things before they touch a device or a ctx
    for change in bad[:8]:
        p = rtamd.make_denoise_params(W, H, 2)
        for k, v in change.items():
            setattr(p, k, v)
        assert L.rt_denoise(None, C.byref(p), ptr(color), None, ptr(feat), ptr(out), None, None) == rtamd.RT_E_INVALID
        assert L.rt_denoise_async(None, C.byref(p), 8, None, 8, 8, None, None) == rtamd.RT_E_INVALID
    assert L.rt_denoise(None, C.byref(good), ptr(color), None, ptr(feat), ptr(out), None, None) == rtamd.RT_E_INVALID
    assert L.rt_denoise_async(None, C.byref(good), None, None, 8, 8, None, None) == rtamd.RT_E_INVALID
    assert L.rt_frame_denoise(None, C.byref(good), 8, None, None, None) == rtamd.RT_E_INVALID
    assert L.rt_last_denoise(None, None) == rtamd.RT_E_INVALID
    # the Python layer checks shapes
    with pytest.raises(rtamd.RTError):
        rtamd.denoise_host(good, color[:2], None, feat)
    with pytest.raises(rtamd.RTError):
        rtamd.denoise_host(good, color, None, feat[..., :7])
