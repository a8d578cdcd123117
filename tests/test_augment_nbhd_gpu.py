"""The neighbourhood augmentation kernel (pseg_augment_batch_nbhd, ops.augment_batch_nbhd, DeviceAugment.full) on the GPU:
rows without a filter, noise or dropout against pseg_augment_batch (bit for bit), filters, noise and dropout against an
fp64 restatement of the pipeline in numpy (Philox4x32-10 included), the reflecting border, sentinel-guarded outputs under
hostile rows, the entry point's refusals, and one training epoch with DeviceAugment.full().

Measured on one MI355X -- the largest excluded share of a row, which is a property of the restatement and the photos (the
CPU test test_restatement_stays_inside_the_caps finds the same), and the device's distance on the excluded pixels:
  filters (cap 2 %; average k=6: 5 %): Gaussian sigma 0.4 / 1.7 / 2.99: 0.0024 / 0.0018 / 0.0056; composed K=13: 0.0189;
    average k=6: 0.0334; average k=3, 5, 7: 0; the dyadic ones (average k=2, 4, sharpen, emboss): 0 excluded, with 94790
    + 23993 + 278785 exact ties compared over the cases; every compared pixel equal, no excluded pixel off by more than 1;
  noise (cap 1 %): 0.0026 at 37x83, 0.0022 at 70x131; every compared pixel equal and, as it happened, the excluded ones too."""
import os

import numpy as np
import pytest
import torch

from pytorch_segmentation_amd.utils import augment as aug
from pytorch_segmentation_amd.utils.augment import DeviceAugment
from pytorch_segmentation_amd.utils.datasets import MEAN, STD

from test_augment_gpu import _batch, _dev, _device_q, _half_distance, _normalise32, _oracle, _round8

pytestmark = pytest.mark.gpu
DEV = 'cuda'
B = 3
GRIDS = [(37, 83), (70, 131)]
MULTI = [(32, 64), (96, 160)]             # from 70 x 131: a reduction by more than 2 and an enlargement
CVAL = 77.0
SEEDS = [0x0123456789ABCDEF, 0xFFC00001_7FA00001, 3]     # (the second one's halves are NaN patterns when read as floats)


# ------------------------------------------------------------------ rows
def exact_warps(H, W):
    """(inverse 2x3, order, mode) of three warps whose coordinates and interpolation weights are exact in fp32, so that the
    warp stage of the restatement equals the device's on every pixel: both flips with a shift (partly outside: cval), a
    shift by (-3, 2) pixels (edge mode), and a shift by (1/2, -1/4) pixel (bilinear, dyadic weights).  The part of the grid that lies outside
    the image is kept small: where an edge pixel is replicated the image is not noise-like, window sums repeat, and the
    exact ties of a box filter stop being the 1/36 of the pixels that the cap for average k=6 counts on."""
    return [(np.array([[-1., 0, W - 1 - 5], [0, -1., H - 1 + 3]]), 0, 0),
            (np.array([[1., 0, -3], [0, 1., 2]]), 0, 1),
            (np.array([[1., 0, 0.5], [0, 1., -0.25]]), 1, 0)]


def base_rows(H, W, warped):
    if not warped:
        return [aug.make_row(None, None, CVAL, 0, 0) for _ in range(B)]
    return [aug.make_row(inv, None, CVAL, order, mode) for inv, order, mode in exact_warps(H, W)]


def nbhd_table(bases, kernel=None, noise=None, dropout=None, seeds=SEEDS):
    return np.stack([aug.make_nbhd_row(base, kernel, noise, dropout, seed) for base, seed in zip(bases, seeds)])


FILTERS = {
    'gaussian 0.4': [('gaussian', 0.4)], 'gaussian 1.7': [('gaussian', 1.7)], 'gaussian 2.99': [('gaussian', 2.99)],
    'average 2': [('average', 2)], 'average 3': [('average', 3)], 'average 4': [('average', 4)], 'average 5': [('average', 5)],
    'average 6': [('average', 6)], 'average 7': [('average', 7)],
    'sharpen light': [('sharpen', 1.0, 1.5)], 'sharpen dark': [('sharpen', 1.0, 0.75)],
    'emboss strong': [('emboss', 1.0, 2.0)], 'emboss flat': [('emboss', 1.0, 0.0)],
    # (mild blends: delta grows with sum|w|, and 2 * delta, the share it excludes, has to stay below the 2 % cap: sum|w| < 1.9)
    'composed 13': [('gaussian', 2.99), ('sharpen', 0.25, 1.25), ('emboss', 0.25, 0.5)],
}


def filter_of(name):
    return aug.compose_filters([aug.filter_kernel(*f) for f in FILTERS[name]])


def excluded_cap(name):
    # average k=6: a window sum = 18 (mod 36) is an exact tie, 1/36 of the pixels by counting, and fl32(1/36) is inexact
    return 0.05 if name == 'average 6' else 0.02


# ------------------------------------------------------------------ fp64 restatement of the pipeline
def ms_index(n_out, n_in):
    """ATen's nearest source index, in fp32 as the kernel"""
    i = np.floor(np.arange(n_out, dtype=np.float32) * (np.float32(n_in) / np.float32(n_out))).astype(np.int64)
    return np.minimum(i, n_in - 1)


def reflect101(i, n):
    """-1 -> 1, n -> n - 2 (cv2's default border), repeated while needed; the only pixel when n == 1"""
    i = np.array(i, dtype=np.int64)
    if n == 1:
        return np.zeros_like(i)
    while ((i < 0) | (i >= n)).any():
        i = np.where(i < 0, -i, i)
        i = np.where(i >= n, 2 * n - 2 - i, i)
    return i


def philox4x32_10(n, stream, seed):
    """counter (n, stream, 0, 0), key = the 64-bit seed -> four uint64 arrays holding 32-bit words"""
    m0, m1, lo = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0xFFFFFFFF)
    s = np.uint64(32)
    c = [np.asarray(n, dtype=np.uint64), np.full(np.shape(n), stream, dtype=np.uint64), np.zeros(np.shape(n), dtype=np.uint64),
         np.zeros(np.shape(n), dtype=np.uint64)]
    k0, k1 = np.uint64(int(seed) & 0xFFFFFFFF), np.uint64(int(seed) >> 32)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]                      # 32 x 32 -> 64 bits: no overflow
        c = [(p1 >> s) ^ c[1] ^ k0, p1 & lo, (p0 >> s) ^ c[3] ^ k1, p0 & lo]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & lo, (k1 + np.uint64(0xBB67AE85)) & lo
    return c


def uniform24(bits):
    return (bits >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def correlate(q, w):
    """q [3,H,W] (fp64), w [K,K] -> sum_j sum_i w[j][i] q(y + j - K/2, x + i - K/2) with the reflecting border"""
    K, (H, W) = w.shape[0], q.shape[1:]
    ys, xs = reflect101(np.arange(-(K // 2), H + K // 2), H), reflect101(np.arange(-(K // 2), W + K // 2), W)
    padded = q[:, ys][:, :, xs]
    out = np.zeros_like(q)
    for j in range(K):
        for i in range(K):
            out += w[j, i] * padded[:, j:j + H, i:i + W]
    return out


def row_seed(row):
    lo, hi = row.view(np.uint32)[aug.NBHD_SEED:aug.NBHD_SEED + 2]
    return int(lo) | (int(hi) << 32)


def restate(imgs, segs, rows, out_hw=None):
    """-> dict of [B,3,oh,ow] arrays: q (8-bit result), filt / noise (the pre-rounding values of those stages), delta
    ([B]: the filter's fp32 accumulation bound K^2 sum|w| 255 2^-23), keep (bool); and label [B,H,W]"""
    Bn, _, H, W = imgs.shape
    base = _oracle(imgs, segs, np.ascontiguousarray(rows[:, :aug.ROW]))
    iy, ix = (np.arange(H), np.arange(W)) if out_hw is None else (ms_index(out_hw[0], H), ms_index(out_hw[1], W))
    yy, xx = np.meshgrid(np.arange(H, dtype=np.uint64), np.arange(W, dtype=np.uint64), indexing='ij')
    pix = yy * np.uint64(W) + xx
    res = {k: [] for k in ('q', 'filt', 'noise', 'delta', 'keep')}
    for b in range(Bn):
        row = rows[b]
        q = _round8(base['warp'][b])
        K, delta = int(row[aug.NBHD_K]), 0.0
        filt = q
        if K > 1:
            w = row[aug.NBHD_WEIGHTS:aug.NBHD_WEIGHTS + K * K].astype(np.float64).reshape(K, K)     # the fp32-rounded weights
            filt, delta = correlate(q, w), K * K * np.abs(w).sum() * 255 * 2.0 ** -23
            q = _round8(filt)
        M = row[6:18].astype(np.float64).reshape(3, 4)
        q = _round8(np.einsum('ck,khw->chw', M[:, :3], q) + M[:, 3][:, None, None])
        seed, noise = row_seed(row), q
        scale, noise_pc = float(row[aug.NBHD_NOISE]), row[aug.NBHD_NOISE + 1] != 0
        if scale > 0:
            n = []
            for c in range(3):
                r = philox4x32_10(pix, c if noise_pc else 0, seed)
                u1, u2 = ((r[0] >> np.uint64(8)).astype(np.float64) + 1.0) * 2.0 ** -24, uniform24(r[1])
                n.append(np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2))
            noise = q + scale * np.stack(n)
            q = _round8(noise)
        p, drop_pc = np.float32(row[aug.NBHD_DROP]), row[aug.NBHD_DROP + 1] != 0
        mh, mw = np.uint64(row[aug.NBHD_DROP + 2]), np.uint64(row[aug.NBHD_DROP + 3])
        keep = np.ones((3, H, W), dtype=bool)
        if p > 0:
            cell = (yy * mh // np.uint64(H)) * mw + xx * mw // np.uint64(W) if mh else pix
            keep = np.stack([uniform24(philox4x32_10(cell, 4 + (c if drop_pc else 0), seed)[0]) >= np.float64(p) for c in range(3)])
            q = np.where(keep, q, 0.0)
        for k, v in (('q', q), ('filt', filt), ('noise', noise), ('keep', keep)):
            res[k].append(v[:, iy][:, :, ix])
        res['delta'].append(delta)
    out = {k: np.stack(v) for k, v in res.items()}
    out['label'] = base['label']
    return out


def is_dyadic(w):
    """every weight is a multiple of 1/64 and small: the fp32 accumulation of 8-bit values is then exact in any order"""
    w = np.asarray(w, dtype=np.float64) * 64
    return bool((w == np.rint(w)).all() and np.abs(w).sum() < 2 ** 12)


def filter_ok(r, b, exact):
    """the pixels of sample b that are compared exactly: further than delta from a half-integer before rounding, and for
    dyadic weights (exact arithmetic) also the exact ties, which round half up"""
    d = _half_distance(r['filt'][b])
    return (d > r['delta'][b]) | (d == 0.0) if exact else d > r['delta'][b]


# ------------------------------------------------------------------ device call
def run(imgs, segs, rows, out_hw=None):
    out, tgt = DeviceAugment.identity().apply(_dev(imgs), _dev(segs), rows, out_hw)
    assert out.dtype == torch.float32 and tgt.dtype == torch.int64 and out.is_contiguous() and tgt.is_contiguous()
    return out.cpu().numpy(), tgt.cpu().numpy()


def flat(H, W, value=128):
    imgs = np.full((B, 3, H, W), value, dtype=np.uint8)
    return imgs, np.zeros((B, H, W), dtype=np.uint8)


def out_sizes(H, W):
    return [None] + (MULTI if (H, W) == (70, 131) else [])


# ------------------------------------------------------------------ 1. no-op rows == pseg_augment_batch
@pytest.mark.parametrize('order', [0, 1])
@pytest.mark.parametrize('H,W', GRIDS)
def test_rows_without_neighbourhood_fields_equal_augment_batch(H, W, order):
    from pytorch_segmentation_amd import ops
    imgs, segs = (_dev(a) for a in _batch(B, H, W))
    shapes = torch.zeros(B, 3, dtype=torch.int32)
    warped = 0
    for seed in range(4):
        narrow = DeviceAugment.reference(seed=seed).sample(B, H, W)
        assert narrow.shape == (B, aug.ROW)
        narrow[:, 19] = order
        warped += int((narrow[:, 0:6] != aug.make_row()[0:6]).any(axis=1).sum())
        wide = np.stack([aug.make_nbhd_row(r) for r in narrow])
        for out_hw in out_sizes(H, W):
            oh, ow = out_hw or (H, W)
            want_img, want_lab = ops.augment_batch(imgs, segs, _dev(narrow), oh, ow, MEAN, STD)
            got_img, got_lab = ops.augment_batch_nbhd(imgs, segs, _dev(wide), shapes, oh, ow, MEAN, STD)
            assert torch.equal(got_img, want_img) and torch.equal(got_lab, want_lab), (seed, out_hw)
    assert warped >= 6                                       # the drawn rows do warp


# ------------------------------------------------------------------ 2. filters vs fp64
@pytest.mark.parametrize('warped', [False, True])
@pytest.mark.parametrize('H,W', GRIDS)
@pytest.mark.parametrize('name', sorted(FILTERS))
def test_filters_against_fp64(name, H, W, warped):
    imgs, segs = _batch(B, H, W)
    kernel = filter_of(name)
    assert kernel.shape[0] == {'composed 13': 13, 'gaussian 2.99': 9, 'average 6': 7}.get(name, kernel.shape[0])
    rows = nbhd_table(base_rows(H, W, warped), kernel)
    exact = is_dyadic(rows[0, aug.NBHD_WEIGHTS:])
    assert exact == (name in ('average 2', 'average 4', 'sharpen light', 'sharpen dark', 'emboss strong', 'emboss flat'))
    for out_hw in out_sizes(H, W) if not warped else [None]:
        got_img, got_lab = run(imgs, segs, rows, out_hw)
        r = restate(imgs, segs, rows, out_hw)
        q = _device_q(got_img)
        assert np.array_equal(got_lab, r['label'])
        for b in range(B):
            ok = filter_ok(r, b, exact)
            excluded, worst = 1.0 - ok.mean(), np.abs(q[b] - r['q'][b]).max()
            print('filter %s %dx%d -> %s warped=%d b=%d: delta %.3g, excluded %.4f, ties checked %d, max |dq| %g'
                  % (name, H, W, out_hw, warped, b, r['delta'][b], excluded, (_half_distance(r['filt'][b]) == 0).sum() * exact, worst))
            assert excluded <= excluded_cap(name)
            assert np.array_equal(q[b][ok], r['q'][b][ok])
            assert worst <= 1.0
        if warped:
            assert (r['filt'] != restate(imgs, segs, nbhd_table(base_rows(H, W, False), kernel))['filt']).mean() > 0.5


# ------------------------------------------------------------------ 3. the border
@pytest.mark.parametrize('H,W', GRIDS)
def test_box_filter_reflects_without_repeating_the_edge(H, W):
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    ramp = (xx + (3 * yy) // 2).astype(np.uint8)                          # at most 130 + 103
    imgs = np.ascontiguousarray(np.broadcast_to(ramp, (B, 3, H, W)))
    segs = np.zeros((B, H, W), dtype=np.uint8)
    rows = nbhd_table(base_rows(H, W, False), np.full((7, 7), 1.0 / 49))
    q = _device_q(run(imgs, segs, rows)[0])
    r = restate(imgs, segs, rows)
    border = np.zeros((H, W), dtype=bool)
    border[:3], border[-3:], border[:, :3], border[:, -3:] = True, True, True, True
    ok = filter_ok(r, 0, False)[0] & border
    print('border %dx%d: compared %d of %d border pixels' % (H, W, ok.sum(), border.sum()))
    assert ok.sum() >= 0.95 * border.sum()
    for b in range(B):
        assert np.array_equal(q[b][:, ok], r['q'][b][:, ok])
        assert np.abs(q[b] - r['q'][b]).max() <= 1.0
    # and the check tells the borders apart: repeating the edge pixel (reflect with edge) or replicating it gives other values
    f = imgs[0].astype(np.float64)
    for mode in ('symmetric', 'edge'):
        padded = np.pad(f, ((0, 0), (3, 3), (3, 3)), mode=mode)
        other = _round8(sum(padded[:, j:j + H, i:i + W] for j in range(7) for i in range(7)) / 49.0)
        assert (other[0][ok] != r['q'][0][0][ok]).mean() > 0.1, mode


# ------------------------------------------------------------------ 4. dropout
@pytest.mark.parametrize('per_channel', [False, True])
@pytest.mark.parametrize('mask', [(0, 0), (5, 9)])
@pytest.mark.parametrize('H,W', GRIDS)
def test_dropout_pattern_equals_the_restatement(H, W, mask, per_channel):
    imgs, segs = flat(H, W)
    p = 0.1 if mask == (0, 0) else 0.3
    rows = nbhd_table(base_rows(H, W, False), dropout=(p, per_channel) + mask)
    for out_hw in out_sizes(H, W):
        q = _device_q(run(imgs, segs, rows, out_hw)[0])
        r = restate(imgs, segs, rows, out_hw)
        assert set(np.unique(q)) <= {0.0, 128.0}
        assert np.array_equal(q == 128.0, r['keep'])                   # bit for bit
        assert np.array_equal(q, r['q'])
        if out_hw is not None:                                          # the nearest resize of the working-grid mask
            full = restate(imgs, segs, rows)['keep']
            assert np.array_equal(q == 128.0, full[:, :, ms_index(out_hw[0], H)][:, :, :, ms_index(out_hw[1], W)])
        kept = q == 128.0
        assert per_channel == bool((kept[:, 0] != kept[:, 1]).any())
        assert not np.array_equal(kept[0], kept[1])                     # the samples of a batch have their own seeds
        if out_hw is None and mask == (0, 0):
            n = kept.size if per_channel else kept[:, 0].size           # independent draws
            dropped = (~kept).sum() if per_channel else (~kept[:, 0]).sum()
            print('dropout %dx%d per_channel=%d: dropped %d of %d' % (H, W, per_channel, dropped, n))
            assert abs(dropped - n * p) <= 5.0 * np.sqrt(n * p * (1 - p))
        if out_hw is None and mask != (0, 0):
            cy, cx = np.arange(H) * mask[0] // H, np.arange(W) * mask[1] // W
            seen = 0
            for j in range(mask[0]):
                for i in range(mask[1]):
                    cell = kept[:, :, cy == j][:, :, :, cx == i]
                    assert cell.size and (cell == cell[:, :, :1, :1]).all()
                    seen += 1
            assert seen == 45 and 0 < (~kept).sum() < kept.size


# ------------------------------------------------------------------ 5. noise
@pytest.mark.parametrize('H,W', GRIDS)
def test_noise_against_fp64(H, W):
    imgs, segs = flat(H, W)
    scale = 10.0
    shared = nbhd_table(base_rows(H, W, False), noise=(scale, False))
    q = _device_q(run(imgs, segs, shared)[0])
    r = restate(imgs, segs, shared)
    # |q + scale n| < 512: fp32 ulp 6e-5, a few ulp for logf / cosf / the product
    ok = _half_distance(r['noise']) > 1e-3
    print('noise %dx%d: excluded %.4f, max |dq| %g' % (H, W, 1.0 - ok.mean(), np.abs(q - r['q']).max()))
    assert 1.0 - ok.mean() <= 0.01
    assert np.array_equal(q[ok], r['q'][ok]) and np.abs(q - r['q']).max() <= 1.0
    assert np.array_equal(q[:, 0], q[:, 1]) and np.array_equal(q[:, 0], q[:, 2])            # one normal per pixel
    n = q[:, 0].size
    sigma = np.sqrt(scale ** 2 + 1.0 / 12)                                                   # rounding adds 1/12
    mean, std = (q[:, 0] - 128.0).mean(), q[:, 0].std()
    print('noise %dx%d: mean %.4f std %.4f over %d draws' % (H, W, mean, std, n))
    assert abs(mean) <= 5.0 * sigma / np.sqrt(n) and abs(std - sigma) <= 5.0 * sigma / np.sqrt(2 * n)
    assert np.array_equal(q, _device_q(run(imgs, segs, shared)[0]))                         # the same seeds: the same output
    assert not np.array_equal(q[0], q[1]) and not np.array_equal(q[1], q[2])                # the samples' seeds differ
    other = _device_q(run(imgs, segs, nbhd_table(base_rows(H, W, False), noise=(scale, False), seeds=[11, 12, 13]))[0])
    assert (other != q).mean() > 0.5

    per = nbhd_table(base_rows(H, W, False), noise=(scale, True))
    for out_hw in out_sizes(H, W):
        qp = _device_q(run(imgs, segs, per, out_hw)[0])
        rp = restate(imgs, segs, per, out_hw)
        ok = _half_distance(rp['noise']) > 1e-3
        assert np.array_equal(qp[ok], rp['q'][ok]) and np.abs(qp - rp['q']).max() <= 1.0
        assert (qp[:, 0] != qp[:, 1]).mean() > 0.5 and (qp[:, 1] != qp[:, 2]).mean() > 0.5  # a normal per plane
        if out_hw is None:
            assert np.array_equal(qp[:, 0], q[:, 0])                                        # plane 0 is the shared stream


def test_all_stages_together_against_fp64():
    """warp, K=5 filter, colour matrix, noise and coarse dropout in one row, multi-scale: the stage order of the contract"""
    H, W = GRIDS[1]
    imgs, segs = _batch(B, H, W)
    colour = aug.colour_matrix([('multiply', [1.5, 0.5, 1.25]), ('add', [-10.0, 4.0, 9.0])])
    bases = [aug.make_row(inv, colour, CVAL, order, mode) for inv, order, mode in exact_warps(H, W)]
    rows = nbhd_table(bases, filter_of('average 4'), noise=(12.75, True), dropout=(0.15, False, 7, 11))
    for out_hw in out_sizes(H, W):
        got_img, got_lab = run(imgs, segs, rows, out_hw)
        q, r = _device_q(got_img), restate(imgs, segs, rows, out_hw)
        ok = _half_distance(r['noise']) > 1e-3                          # (the filter and the colour matrix are dyadic)
        assert 1.0 - ok.mean() <= 0.01 and np.array_equal(q[ok], r['q'][ok]) and np.abs(q - r['q']).max() <= 1.0
        assert np.array_equal(got_lab, r['label']) and not r['keep'].all() and (q == 255).any()


# ------------------------------------------------------------------ 6. footprint, hostile rows, refusals
@pytest.mark.parametrize('order', [0, 1])
@pytest.mark.parametrize('H,W,out_hw', [(37, 83, None), (70, 131, (32, 64)), (70, 131, (96, 160))])
def test_hostile_rows_and_output_footprint(H, W, out_hw, order):
    from pytorch_segmentation_amd import ops
    imgs, segs = _batch(B, H, W)
    rng = np.random.default_rng(5)
    kernel = rng.uniform(-1, 1, (13, 13))
    kernel /= np.abs(kernel).sum()
    masks = [(1, 1), (H, W), (0, 0)]
    for hostile in ([(2, 1e6), (5, -1e6), (2, -1e6)], [(2, np.nan), (5, np.inf), (0, -np.inf)], [(2, 1e30), (4, np.nan), (2, 3e38)]):
        bases = [aug.make_row(None, None, CVAL, order, mode) for mode in (0, 1, 1)]
        for base, (at, value) in zip(bases, hostile):
            base[at] = value
        rows = np.stack([aug.make_nbhd_row(base, kernel, (12.75, True), (0.1, True) + m, seed)
                         for base, m, seed in zip(bases, masks, SEEDS)])
        oh, ow = out_hw or (H, W)
        pad = 4099
        n_out, n_tgt = B * 3 * oh * ow, B * H * W
        big_out = torch.full((n_out + 2 * pad,), -12345.0, dtype=torch.float32, device=DEV)
        big_tgt = torch.full((n_tgt + 2 * pad,), -987654321, dtype=torch.int64, device=DEV)
        out, tgt = ops.augment_batch_nbhd(_dev(imgs), _dev(segs), _dev(rows), torch.from_numpy(aug.row_shapes(rows)), oh, ow, MEAN,
                                          STD, out=big_out[pad:pad + n_out].view(B, 3, oh, ow),
                                          target=big_tgt[pad:pad + n_tgt].view(B, H, W))
        torch.cuda.synchronize()
        assert (big_out[:pad] == -12345.0).all() and (big_out[pad + n_out:] == -12345.0).all()
        assert (big_tgt[:pad] == -987654321).all() and (big_tgt[pad + n_tgt:] == -987654321).all()
        assert torch.isfinite(out).all() and (out != -12345.0).all() and (tgt != -987654321).all()
        q = _device_q(out.cpu().numpy())                                # every value is a normalised 8-bit value
        assert (tgt.cpu().numpy() == 0).all()                           # every label lies outside
        assert len(np.unique(q)) > 16                                   # and noise ran on the fill values


def test_refusals_launch_nothing():
    from pytorch_segmentation_amd import _lib, ops
    H, W = GRIDS[0]
    imgs, segs = (_dev(a) for a in _batch(B, H, W))
    rows = _dev(nbhd_table(base_rows(H, W, False), filter_of('average 3')))
    out = torch.full((B, 3, H, W), -12345.0, dtype=torch.float32, device=DEV)
    tgt = torch.full((B, H, W), -987654321, dtype=torch.int64, device=DEV)
    for bad, what in (([3, 4, 3], 'filter size 4'), ([3, 3, 15], 'filter size 15'), ([-1, 3, 3], 'filter size -1')):
        shapes = torch.tensor([[k, 0, 0] for k in bad], dtype=torch.int32)
        with pytest.raises(_lib.PsegError, match=what):
            ops.augment_batch_nbhd(imgs, segs, rows, shapes, H, W, MEAN, STD, out=out, target=tgt)
    for mask in ((-1, 4), (4, -1), (0, 4), (70000, 4)):
        shapes = torch.tensor([[3, 0, 0], [3, 0, 0], [3, mask[0], mask[1]]], dtype=torch.int32)
        with pytest.raises(_lib.PsegError, match='sample 2: dropout mask'):
            ops.augment_batch_nbhd(imgs, segs, rows, shapes, H, W, MEAN, STD, out=out, target=tgt)
    # LDS: a 13-tap halo around the span of a 32 x 8 output tile of a 40-fold reduction does not fit
    big = torch.zeros(1, 3, 1300, 1300, dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.PsegError, match='bytes of LDS'):
        ops.augment_batch_nbhd(big, big[:, 0].contiguous(), _dev(nbhd_table(base_rows(8, 8, False)[:1], np.full((13, 13), 1 / 169.))),
                               torch.tensor([[13, 0, 0]], dtype=torch.int32), 32, 32, MEAN, STD)
    torch.cuda.synchronize()
    assert (out == -12345.0).all() and (tgt == -987654321).all()
    ops.augment_batch_nbhd(imgs, segs, rows, torch.tensor([[3, 0, 0]] * 3, dtype=torch.int32), H, W, MEAN, STD, out=out, target=tgt)
    assert (out != -12345.0).all() and (tgt != -987654321).all()      # and the valid call does launch


# ------------------------------------------------------------------ 7. end to end
def test_train_with_full_augment(tmp_path, monkeypatch):
    from pytorch_segmentation_amd import ops
    from pytorch_segmentation_amd.utils.datasets import make_synthetic_coco
    root = make_synthetic_coco(str(tmp_path / 'data'), n_train=4, n_val=2, n_classes=1)
    monkeypatch.chdir(tmp_path)
    import train as train_mod

    made, calls = [], {'nbhd': 0, 'plain': 0}

    class Recorded(train_mod.CocoInstance):
        def __init__(self, path, *a, **kw):
            super().__init__(path, *a, **kw)
            made.append((os.path.basename(path), self))

    def counted(name, fn):
        def call(*a, **kw):
            calls[name] += 1
            return fn(*a, **kw)
        return call

    monkeypatch.setattr(train_mod, 'CocoInstance', Recorded)
    monkeypatch.setattr(ops, 'augment_batch_nbhd', counted('nbhd', ops.augment_batch_nbhd))
    monkeypatch.setattr(ops, 'augment_batch', counted('plain', ops.augment_batch))
    full = DeviceAugment.full(seed=0)
    torch.manual_seed(0)
    _, loss = train_mod.train(root, epochs=1, img_size=[64, 64], batch_size=4, accumulate=1, lr=1e-2, num_workers=0,
                              notest=False, nosave=True, model_name='unet', augment=full)
    print('loss with the full augmentation:', loss, calls)
    assert np.isfinite(loss)
    assert [name for name, _ in made] == ['train.json', 'val.json']
    assert made[0][1].augments is full and made[1][1].augments is None          # validation is not augmented
    assert calls['nbhd'] >= 1                                                   # (seed 0: the first batch draws a filter)
