"""fp64 restatement in numpy of stages 2 to 5 of pseg_augment_batch_blend (include/pseg_amd.h) and of its mask sampler, on top
of the restatements the other augment tests hold their kernels to (test_augment_gpu._oracle for the warp stage,
test_augment_nbhd_gpu.correlate / reflect101 / ms_index).  The median is numpy.sort over the reflected window.  Shared by
tests/test_augment_blend_cpu.py (which shows, without a GPU, how many pixels each comparison excludes) and
tests/test_augment_blend_gpu.py; it also holds the rows and inputs of those comparisons, so that both see the same ones.

Margins (distance of a pre-rounding value from a half-integer below which the fp32 kernel may round the other way):
  * a filter's output: test_augment_nbhd_gpu's accumulation bound delta = K^2 sum|w| 255 2^-23;
  * a mask blend fmaf(m, a - b, b) of two 8-bit integers: the fp32 sample m differs from the fp64 one by the rounding of
    16 / W in gx (below 1e-6 at gx <= 15, times a table slope of at most 1 per cell, on two axes) and six roundings of
    values up to 1: below 3e-6, times |a - b| <= 255: below 1e-3.  BLEND_MARGIN = 2e-3.  Where the issue sets 0.01 (the mask
    sampler's own test, hue / saturation) that is used;
  * the colour matrices of the comparisons are dyadic (multiples of 1/4, integer offsets): their products with 8-bit integers
    are exact in fp32 and fp64 alike, ties included."""
import numpy as np

from pytorch_segmentation_amd.utils import augment as aug

import test_augment_nbhd_gpu as G
from test_augment_gpu import _batch, _half_distance, _oracle, _round8

B = G.B
GRIDS = G.GRIDS
TINY = [(1, 1), (5, 1)]
BLEND_MARGIN = 2e-3
SAMPLER_MARGIN = 0.01                     # set by the issue: mask sampler and hue / saturation
SAMPLER_CAP = 0.05
FILTER_CAP = 0.02                         # test_augment_nbhd_gpu.excluded_cap of every filter used here
MEDIANS = (3, 5, 7, 9, 11)
HUE_V = (-20, -7, 0, 1, 20)
HUE_BEYOND = (7.3, 0.05)                  # a dh beyond a full turn


# ------------------------------------------------------------------ the stages
def mask_sample(T, H, W):
    """[H, W] fp64: the bilinear sample of the 16 x 16 table at every working-grid pixel, clamped to [0, 1], NaN -> 0"""
    T = np.asarray(T, dtype=np.float64).reshape(16, 16)
    gx = np.clip((np.arange(W) + 0.5) * 16.0 / W - 0.5, 0.0, 15.0)
    gy = np.clip((np.arange(H) + 0.5) * 16.0 / H - 0.5, 0.0, 15.0)
    i0, j0 = np.minimum(gx.astype(np.int64), 14), np.minimum(gy.astype(np.int64), 14)
    fu, fv = (gx - i0)[None], (gy - j0)[:, None]
    t = T[j0][:, i0] + fu * (T[j0][:, i0 + 1] - T[j0][:, i0])
    b = T[j0 + 1][:, i0] + fu * (T[j0 + 1][:, i0 + 1] - T[j0 + 1][:, i0])
    m = t + fv * (b - t)
    return np.where(np.isnan(m), 0.0, np.clip(m, 0.0, 1.0))


def median(q, k):
    """q [3,H,W] -> per plane element (k^2 - 1) / 2 of the sorted k x k window, indices reflected (repeatedly if need be)"""
    H, W = q.shape[1:]
    ys, xs = G.reflect101(np.arange(-(k // 2), H + k // 2), H), G.reflect101(np.arange(-(k // 2), W + k // 2), W)
    padded = q[:, ys][:, :, xs]
    taps = np.stack([padded[:, j:j + H, i:i + W] for j in range(k) for i in range(k)], axis=-1)
    return np.sort(taps, axis=-1)[..., (k * k - 1) // 2]


def hue_sat(q, dh, ds):
    """stage 5 on 8-bit values q [3, ...] in fp64 -> the three values BEFORE the 8-bit rounding"""
    r, g, b = (np.asarray(c, dtype=np.float64) for c in q)
    mx, mn = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    d = mx - mn
    safe_d, safe_mx = np.where(d == 0, 1.0, d), np.where(mx > 0, mx, 1.0)
    s = np.where(mx > 0, d / safe_mx, 0.0)
    hr = (g - b) / safe_d
    h = np.where(d == 0, 0.0, np.where(mx == r, np.where(hr < 0, hr + 6.0, hr),
                                       np.where(mx == g, 2.0 + (b - r) / safe_d, 4.0 + (r - g) / safe_d)))
    hp = h + dh
    hp = hp - 6.0 * np.floor(hp / 6.0)
    hp = np.where(hp == 6.0, 0.0, hp)
    sp = np.clip(s + ds, 0.0, 1.0)
    i = np.minimum(hp.astype(np.int64), 5)
    f = hp - i
    p, qq, t = mx * (1.0 - sp), mx * (1.0 - sp * f), mx * (1.0 - sp * (1.0 - f))
    pick = lambda six: np.choose(i, six)
    return np.stack([pick([mx, qq, p, p, t, mx]), pick([t, mx, mx, qq, p, p]), pick([p, p, t, mx, mx, qq])])


def quarters(m):
    """every entry is a multiple of 1/4 and small: m . [r, g, b, 1] on 8-bit integers is exact in fp32, in any order"""
    return bool((m * 4 == np.rint(m * 4)).all() and np.abs(m).max() <= 1024)


def filter_delta(w):
    return w.size * np.abs(w).sum() * 255 * 2.0 ** -23


def restate(imgs, segs, rows, out_hw=None):
    """rows [B, BLEND_ROW] whose coordinate map is the plain affine of [0..5] (no warp field), without noise or dropout ->
    {'q': the 8-bit result [B,3,oh,ow], 'ok': bool, the same shape: every pre-rounding value behind the pixel is decided,
    'med', 'label', and per stage the pre-rounding values 'filt', 'edge', 'blend1', 'blend2', 'hue' where the stage ran}"""
    Bn, _, H, W = imgs.shape
    base = _oracle(imgs, segs, np.ascontiguousarray(rows[:, :aug.ROW]))
    iy, ix = (np.arange(H), np.arange(W)) if out_hw is None else (G.ms_index(out_hw[0], H), G.ms_index(out_hw[1], W))
    res = {}
    for b in range(Bn):
        row = rows[b]
        assert row[aug.NBHD_NOISE] == 0 and row[aug.NBHD_DROP] == 0 and row[aug.WARP_ALPHA] == 0 and row[aug.WARP_GRID_ON] == 0
        assert list(row[aug.WARP_H2:aug.WARP_H2 + 3]) == [0, 0, 1]
        x = _round8(base['warp'][b])
        ok = np.ones(x.shape, dtype=bool)
        one = {}
        kmed, K, K2 = int(row[aug.BLEND_KMED]), int(row[aug.NBHD_K]), int(row[aug.BLEND_K2])
        if kmed:
            x = median(x, kmed)
        one['med'] = x
        y = x
        if K > 1:
            w = row[aug.NBHD_WEIGHTS:aug.NBHD_WEIGHTS + K * K].astype(np.float64).reshape(K, K)
            one['filt'] = G.correlate(x, w)
            exact = G.is_dyadic(w)
            d = _half_distance(one['filt'])
            ok &= (d > filter_delta(w)) | ((d == 0.0) & exact)
            y = _round8(one['filt'])
        if K2:
            w2 = row[aug.BLEND_WEIGHTS2:aug.BLEND_WEIGHTS2 + K2 * K2].astype(np.float64).reshape(K2, K2)
            one['edge'] = G.correlate(x, w2)
            d = _half_distance(one['edge'])
            ok &= (d > filter_delta(w2)) | ((d == 0.0) & G.is_dyadic(w2))
            e = _round8(one['edge'])
            one['blend1'] = y + mask_sample(row[aug.BLEND_T1:aug.BLEND_T1 + 256], H, W)[None] * (e - y)
            ok &= _half_distance(one['blend1']) > BLEND_MARGIN
            y = _round8(one['blend1'])
        M = row[6:18].astype(np.float64).reshape(3, 4)
        assert quarters(M)                                                                  # exact products, ties included
        q = _round8(np.einsum('ck,khw->chw', M[:, :3], y) + M[:, 3][:, None, None])
        if row[aug.BLEND_COLOUR_ON] != 0:
            Mb = row[aug.BLEND_MB:aug.BLEND_MB + 12].astype(np.float64).reshape(3, 4)
            assert quarters(Mb)
            qb = _round8(np.einsum('ck,khw->chw', Mb[:, :3], y) + Mb[:, 3][:, None, None])
            one['blend2'] = qb + mask_sample(row[aug.BLEND_T2:aug.BLEND_T2 + 256], H, W)[None] * (q - qb)
            ok &= _half_distance(one['blend2']) > BLEND_MARGIN
            q = _round8(one['blend2'])
        dh, ds = float(row[aug.BLEND_HUE]), float(row[aug.BLEND_HUE + 1])
        if np.isfinite(dh) and np.isfinite(ds) and (dh != 0 or ds != 0):
            one['hue'] = hue_sat(q, dh, ds)
            ok &= _half_distance(one['hue']) > SAMPLER_MARGIN
            q = _round8(one['hue'])
        one['q'], one['ok'] = q, ok
        for k, v in one.items():
            res.setdefault(k, []).append(v[:, iy][:, :, ix])
    out = {k: np.stack(v) for k, v in res.items()}
    out['label'] = base['label']
    return out


# ------------------------------------------------------------------ rows and inputs of the comparisons
def blend_table(warp_rows, **kw):
    return np.stack([aug.make_blend_row(r, **kw) for r in warp_rows])


def warp_rows(H, W, warped=True, kernel=None, colour=None):
    """[B] make_warp_row rows over G.exact_warps (or the identity), without a warp field"""
    if warped:
        bases = [aug.make_row(inv, colour, G.CVAL, order, mode) for inv, order, mode in G.exact_warps(H, W)]
    else:
        bases = [aug.make_row(None, colour, G.CVAL, 0, 0) for _ in range(B)]
    return [aug.make_warp_row(r) for r in G.nbhd_table(bases, kernel)]


def random_table(seed):
    """a smooth mask with the whole range: what value_noise_table draws (linear octaves)"""
    rng = np.random.default_rng(seed)
    return aug._unit_range(sum(aug.resize_to_table(rng.random((g, g)), True) for g in (3, 5, 9)), False)


MA = aug.colour_matrix([('multiply', [1.5, 0.5, 1.25]), ('add', [-10.0, 4.0, 9.0])])
MB = aug.colour_matrix([('contrast', [0.5, 2.0, 0.75]), ('add', [3.0, 0.0, -5.0])])       # 127 * (1 - a): multiples of 1/4


def sampler_rows(H, W, seed=3):
    """M = 0 with offset 0, Mb = 0 with offset 255, a random T2: the output is round(255 (1 - m2))"""
    zero, full = np.zeros((3, 4)), np.zeros((3, 4))
    full[:, 3] = 255.0
    return blend_table(warp_rows(H, W, False, colour=zero), colour2=full, t2=random_table(seed))


# (F, alpha, direction): dyadic weights; general ones.  E sums to 1 - alpha: with alpha = 0.5 every odd value of a flat region
# (the fill value's) would be an exact tie
EDGE_CASES = [('average 2', 0.75, None), ('average 3', 0.625, 0.3)]


def edge_rows(H, W, name, alpha, direction):
    """F = a mild filter, G = E * F with E = EdgeDetect / DirectedEdgeDetect (mild: delta grows with sum|w|, and what it
    excludes has to stay below the 2 % cap), a random T1, exact warps"""
    F = G.filter_of(name)
    G2 = aug.compose_filters([F, aug.edge_kernel(alpha, direction)])
    return blend_table(warp_rows(H, W, True, kernel=F), kernel2=G2, t1=random_table(4))


def colour_rows(H, W):
    return blend_table(warp_rows(H, W, True, colour=MA), colour2=MB, t2=random_table(5))


def median_rows(H, W, k, warped=True, kernel=None):
    return blend_table(warp_rows(H, W, warped, kernel=kernel), kmed=k)


def hue_batch():
    """uint8 [B, 3, 37, 83]: black, white, greys, the six primaries and secondaries, ties of two channels above or below the
    third, then random colours; and all-zero labels"""
    H, W = GRIDS[0]
    rng = np.random.default_rng(11)
    fixed = [(0, 0, 0), (255, 255, 255), (1, 1, 1), (77, 77, 77), (128, 128, 128), (254, 254, 254),
             (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255),
             (200, 200, 50), (50, 200, 200), (200, 50, 200), (200, 50, 50), (50, 200, 50), (50, 50, 200),
             (1, 0, 0), (0, 1, 0), (0, 0, 1), (255, 254, 0), (254, 255, 255), (130, 129, 129)]
    imgs = rng.integers(0, 256, (B, 3, H, W)).astype(np.uint8)
    flat = imgs.reshape(B, 3, -1)
    for b in range(B):
        flat[b, :, :len(fixed)] = np.array(fixed, dtype=np.uint8).T
        flat[b, :, len(fixed):2 * len(fixed)] = np.roll(np.array(fixed, dtype=np.uint8).T, b + 1, axis=0)
    return imgs, np.zeros((B, H, W), dtype=np.uint8)


def hue_shifts():
    return [aug.hue_sat_shift(v) for v in HUE_V] + [HUE_BEYOND]


def hue_rows(H, W, dh_ds):
    return blend_table(warp_rows(H, W, False), hue_sat=dh_ds)


def excluded(r, b):
    return 1.0 - r['ok'][b].mean()


def photos(H, W):
    return _batch(B, H, W)
