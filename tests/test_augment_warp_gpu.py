"""The warp augmentation kernel (pseg_augment_batch_warp, ops.augment_batch_warp, DeviceAugment.warps) on the GPU: rows
without a warp field against pseg_augment_batch_nbhd (bit for bit), a uniform displacement grid against the same
translation folded into the matrix (bit for bit), perspective / grid / elastic against an fp64 restatement of the
coordinate map in numpy (Philox included), image and mask moving together, the jitter of the filter's halo, sentinel-guarded
outputs under hostile rows, the entry point's refusals, and one training epoch with DeviceAugment.warps().

The comparison rules are those of test_augment_gpu.py: a nearest sample is compared where s + 0.5 lies more than 1e-3 from
an integer on both axes (at most 2 % of a row excluded), a bilinear value where its pre-rounding value lies more than 0.05
from a half-integer (at most 15 %), every pixel within one 8-bit step.  The caps are properties of the restatement and
the photos; tests/test_augment_warp_cpu.py::test_restatement_stays_inside_the_caps finds them without a GPU.  On the grids
of one or five pixels (the W == 1 guard) a single undecided pixel is 20 % of a row, so their rows are chosen from the
restatement alone (tiny_rows) such that NO pixel is undecided: there nothing is excluded and every pixel is compared."""
import os

import numpy as np
import pytest
import torch

from pytorch_segmentation_amd.utils import augment as aug
from pytorch_segmentation_amd.utils.augment import DeviceAugment
from pytorch_segmentation_amd.utils.datasets import MEAN, STD

import test_augment_nbhd_gpu as G
from test_augment_gpu import _batch, _dev, _device_q, _half_distance, _round8

pytestmark = pytest.mark.gpu
DEV = 'cuda'
B = G.B
GRIDS = G.GRIDS                           # (37, 83), (70, 131); the latter also at G.MULTI = (32, 64), (96, 160)
TINY = [(1, 1), (5, 1)]
CVAL = G.CVAL
SEEDS = G.SEEDS
CASES = ('perspective', 'grid', 'elastic', 'all')
ELASTIC_FILTER_CAP = 0.06                 # nine pixels of a 3 x 3 window at about 0.4 % undecided each: about 3.5 % expected


# ------------------------------------------------------------------ rows
def recipe(order, mode, **kw):
    r = {'fliplr': False, 'flipud': False, 'crop_pad': None, 'affine': None, 'order': order, 'cval': CVAL, 'mode': mode, 'colour': []}
    r.update(kw)
    return r


def case_rows(case, H, W, order, mode, cval=CVAL, alpha=3.5, draw=7):
    """[B, WARP_ROW] through DeviceAugment.rows: perspective (|N(0, 0.1)| per corner, behind a mild affine), a displacement grid
    (nodes ~ N(0, 0.05) of the size), elastic (alpha 3.5), or all three; a different draw per sample"""
    rng = np.random.default_rng(draw)
    recipes = []
    for b in range(B):
        kw = {}
        if case in ('perspective', 'all'):
            kw['perspective'] = np.minimum(np.abs(rng.normal(0.0, 0.1, (4, 2))), aug.PERSPECTIVE_CLIP)
            kw['affine'] = {'rotate': 10.0 * (b - 1), 'scale': (1.1, 0.95), 'shear': 3.0, 'translate': tuple(rng.uniform(-0.05, 0.05, 2))}
        if case in ('grid', 'all'):
            kw['piecewise'] = rng.normal(0.0, 0.05, (4, 4, 2))
        if case in ('elastic', 'all'):
            kw['elastic'], kw['seed'] = alpha, (SEEDS[b] + draw - 7) % 2 ** 64
        recipes.append(recipe(order, mode, cval=cval, **kw))
    rows = DeviceAugment.rows(recipes, H, W)
    assert rows.shape == (B, aug.WARP_ROW)
    return rows


def tiny_rows(case, H, W, order, mode):
    """case_rows for a grid of a few pixels: the first draw (7, 8, ...) for which the restatement decides every label, every
    nearest sample and every bilinear value of the photos, so that the comparison excludes nothing.  The grid's nodes are
    then N(0, 0.5) of the size and alpha is 0.75 (a pixel of a one-pixel-wide image otherwise mostly reads outside it).
    Chosen from the fp64 restatement alone; the CPU test checks that the choice exists and reads inside the image."""
    imgs, segs = _batch(B, H, W)
    for draw in range(7, 2007):
        rows = case_rows(case, H, W, order, mode, alpha=0.75, draw=draw)
        if case in ('grid', 'all'):
            rows[:, aug.WARP_GRID:] *= 10.0
        o = oracle(imgs, segs, rows)
        if o['label_ok'].all() and o['img_ok'].all():
            return rows
    raise AssertionError('no draw without an undecided pixel')


def warp_table(nbhd_rows, **kw):
    return np.stack([aug.make_warp_row(r, **kw) for r in nbhd_rows])


def uniform_grid(dx, dy):
    return np.broadcast_to(np.array([dx, dy], dtype=np.float64), (4, 4, 2))


def fold_translation(rows, dx, dy):
    """the rows whose matrix reads (x + dx, y + dy): exact in fp32 for the dyadic matrices of G.exact_warps"""
    out = rows.copy()
    out[:, 2] = rows[:, 2] + rows[:, 0] * np.float32(dx) + rows[:, 1] * np.float32(dy)
    out[:, 5] = rows[:, 5] + rows[:, 3] * np.float32(dx) + rows[:, 4] * np.float32(dy)
    return out


# ------------------------------------------------------------------ fp64 restatement of the coordinate map
def source_coords(row, ys, xs, H, W):
    """working-grid pixels (ys x xs) -> (sx, sy, inside-capable): the contract of include/pseg_amd.h in fp64 on the row's
    fp32-rounded numbers: elastic jitter -> displacement grid -> homography; not inside where den <= 0 or not finite"""
    with np.errstate(invalid='ignore'):                     # (the seed's halves may be NaN patterns)
        r64 = row.astype(np.float64)
    gy, gx = np.meshgrid(np.asarray(ys, dtype=np.int64), np.asarray(xs, dtype=np.int64), indexing='ij')
    px, py = gx.astype(np.float64), gy.astype(np.float64)
    alpha = float(row[aug.WARP_ALPHA])
    if 0.0 < alpha <= 3.0e38:
        r = G.philox4x32_10((gy * W + gx).astype(np.uint64), 8, G.row_seed(row))
        px = px + alpha * (2.0 * G.uniform24(r[0]) - 1.0)
        py = py + alpha * (2.0 * G.uniform24(r[1]) - 1.0)
    if row[aug.WARP_GRID_ON] != 0:
        nodes = r64[aug.WARP_GRID:aug.WARP_GRID + 32].reshape(4, 4, 2)
        gu = np.clip(px * 3.0 / (W - 1), 0.0, 3.0) if W > 1 else np.zeros_like(px)
        gv = np.clip(py * 3.0 / (H - 1), 0.0, 3.0) if H > 1 else np.zeros_like(py)
        i0, j0 = np.minimum(gu.astype(np.int64), 2), np.minimum(gv.astype(np.int64), 2)
        fu, fv = (gu - i0)[..., None], (gv - j0)[..., None]
        top = nodes[j0, i0] + fu * (nodes[j0, i0 + 1] - nodes[j0, i0])
        bot = nodes[j0 + 1, i0] + fu * (nodes[j0 + 1, i0 + 1] - nodes[j0 + 1, i0])
        d = top + fv * (bot - top)
        px, py = px + d[..., 0], py + d[..., 1]
    h2 = r64[aug.WARP_H2:aug.WARP_H2 + 3]
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        den = h2[0] * px + h2[1] * py + h2[2]
        sx, sy = (r64[0] * px + r64[1] * py + r64[2]) / den, (r64[3] * px + r64[4] * py + r64[5]) / den
    finite = np.isfinite(sx) & np.isfinite(sy) & (den > 0)
    return np.where(finite, sx, -1.0), np.where(finite, sy, -1.0), finite


def oracle(imgs, segs, rows, out_hw=None):
    """test_augment_gpu._oracle with the warp kernel's coordinate map; also decided [B,H,W]: the nearest sample of the
    working-grid pixel is decided"""
    Bn, _, H, W = imgs.shape
    f = imgs.astype(np.float64)
    iy, ix = (np.arange(H), np.arange(W)) if out_hw is None else (G.ms_index(out_hw[0], H), G.ms_index(out_hw[1], W))
    res = {k: [] for k in ('warp', 'stage', 'q', 'img_ok', 'label', 'label_ok')}
    for b in range(Bn):
        row = rows[b]
        M = row[6:18].astype(np.float64).reshape(3, 4)
        cval, bilinear, edge = float(row[18]), row[19] != 0, row[20] != 0
        sx, sy, finite = source_coords(row, np.arange(H), np.arange(W), H, W)
        cx, cy = np.clip(sx, -1.0, W), np.clip(sy, -1.0, H)
        decided = (np.abs(sx + 0.5 - np.round(sx + 0.5)) > 1e-3) & (np.abs(sy + 0.5 - np.round(sy + 0.5)) > 1e-3)
        nx, ny = np.floor(cx + 0.5).astype(np.int64), np.floor(cy + 0.5).astype(np.int64)
        inside = finite & (nx >= 0) & (nx < W) & (ny >= 0) & (ny < H)
        res['label'].append(np.where(inside, segs[b][np.clip(ny, 0, H - 1), np.clip(nx, 0, W - 1)], 0).astype(np.int64))
        res['label_ok'].append(decided)

        def tap(y, x):
            ok = (edge & finite) | (finite & (y >= 0) & (y < H) & (x >= 0) & (x < W))
            return np.where(ok[None], f[b][:, np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)], cval)

        if not bilinear:
            v = tap(ny, nx)
            ok = np.broadcast_to(decided[None], v.shape)
        else:
            x0, y0 = np.floor(cx).astype(np.int64), np.floor(cy).astype(np.int64)
            lx, ly = (cx - x0)[None], (cy - y0)[None]
            v = (1 - ly) * ((1 - lx) * tap(y0, x0) + lx * tap(y0, x0 + 1)) + ly * ((1 - lx) * tap(y0 + 1, x0) + lx * tap(y0 + 1, x0 + 1))
            ok = _half_distance(v) > 0.05
        stage = np.einsum('ck,khw->chw', M[:, :3], _round8(v)) + M[:, 3][:, None, None]
        for k, a in (('warp', v), ('stage', stage), ('q', _round8(stage)), ('img_ok', ok)):
            res[k].append(a[:, iy][:, :, ix])
    return {k: np.stack(v) for k, v in res.items()}


def restate_filtered(imgs, segs, rows, out_hw=None):
    """oracle() followed by the row's K x K correlation (reflecting border) and the colour matrix, each rounded to 8 bits:
    {'q': [B,3,oh,ow], 'label': [B,H,W]} of rows without noise or dropout"""
    Bn, _, H, W = imgs.shape
    o = oracle(imgs, segs, rows)
    iy, ix = (np.arange(H), np.arange(W)) if out_hw is None else (G.ms_index(out_hw[0], H), G.ms_index(out_hw[1], W))
    q = []
    for b in range(Bn):
        row = rows[b]
        K = int(row[aug.NBHD_K])
        assert K > 1 and row[aug.NBHD_NOISE] == 0 and row[aug.NBHD_DROP] == 0
        w = row[aug.NBHD_WEIGHTS:aug.NBHD_WEIGHTS + K * K].astype(np.float64).reshape(K, K)
        M = row[6:18].astype(np.float64).reshape(3, 4)
        f = _round8(G.correlate(_round8(o['warp'][b]), w))
        q.append(_round8(np.einsum('ck,khw->chw', M[:, :3], f) + M[:, 3][:, None, None])[:, iy][:, :, ix])
    return {'q': np.stack(q), 'label': o['label']}


def window_decided(decided, K):
    """[H, W] bool: every pixel of the K x K window (reflecting border) is decided"""
    H, W = decided.shape
    ys, xs = G.reflect101(np.arange(-(K // 2), H + K // 2), H), G.reflect101(np.arange(-(K // 2), W + K // 2), W)
    padded = decided[ys][:, xs]
    out = np.ones((H, W), dtype=bool)
    for j in range(K):
        for i in range(K):
            out &= padded[j:j + H, i:i + W]
    return out


def elastic_filter_rows(H, W):
    """identity matrix, order 0, sharpen (alpha 1: dyadic weights, exact fp32 sums) and elastic alpha 3.5"""
    nb = G.nbhd_table(G.base_rows(H, W, False), aug.sharpen_kernel(1.0, 1.5))
    return warp_table(nb, alpha=3.5)


def out_sizes(H, W):
    return G.out_sizes(H, W)


def check_against_fp64(imgs, segs, rows, out_hw, nothing_excluded=False):
    got_img, got_lab = G.run(imgs, segs, rows, out_hw)
    o = oracle(imgs, segs, rows, out_hw)
    q = _device_q(got_img)
    bilinear = rows[0, 19] != 0
    for b in range(imgs.shape[0]):
        lab_ok, img_ok = o['label_ok'][b], o['img_ok'][b]
        excl_lab, excl_img = 1.0 - lab_ok.mean(), 1.0 - img_ok.mean()
        print('warp %s -> %s b=%d order=%d mode=%d: labels excluded %.4f, image excluded %.4f, max |dq| %g'
              % (imgs.shape, out_hw, b, rows[b, 19], rows[b, 20], excl_lab, excl_img, np.abs(q[b] - o['q'][b]).max()))
        assert excl_lab <= 0.02 and excl_img <= (0.15 if bilinear else 0.02)
        assert not nothing_excluded or (excl_lab == 0.0 and excl_img == 0.0)
        assert np.array_equal(got_lab[b][lab_ok], o['label'][b][lab_ok])
        assert np.array_equal(q[b][img_ok], o['q'][b][img_ok])
        if bilinear:
            assert np.abs(q[b] - o['q'][b]).max() <= 1.0     # every pixel within one 8-bit step
    return o


# ------------------------------------------------------------------ 1. rows without a warp field == pseg_augment_batch_nbhd
@pytest.mark.parametrize('filtered', [False, True])
@pytest.mark.parametrize('order', [0, 1])
@pytest.mark.parametrize('H,W', GRIDS + TINY)
def test_rows_without_warp_fields_equal_augment_batch_nbhd(H, W, order, filtered):
    from pytorch_segmentation_amd import ops
    imgs, segs = (_dev(a) for a in _batch(B, H, W))
    for seed in range(3):
        narrow = DeviceAugment.reference(seed=seed).sample(B, H, W)
        narrow[:, 19] = order
        if filtered:
            nb = np.stack([aug.make_nbhd_row(r, G.filter_of('gaussian 1.7'), (10.0, True), (0.1, False, 5, 9), s) for r, s in zip(narrow, SEEDS)])
        else:
            nb = np.stack([aug.make_nbhd_row(r) for r in narrow])
        wide = warp_table(nb)
        assert wide.shape == (B, aug.WARP_ROW) and np.array_equal(wide[:, aug.WARP_H2:], np.tile(aug.make_warp_row()[aug.WARP_H2:], (B, 1)))
        shapes = torch.from_numpy(aug.row_shapes(nb))
        for out_hw in out_sizes(H, W):
            oh, ow = out_hw or (H, W)
            want_img, want_lab = ops.augment_batch_nbhd(imgs, segs, _dev(nb), shapes, oh, ow, MEAN, STD)
            got_img, got_lab = ops.augment_batch_warp(imgs, segs, _dev(wide), shapes, oh, ow, MEAN, STD)
            assert torch.equal(got_img, want_img) and torch.equal(got_lab, want_lab), (seed, out_hw)


# ------------------------------------------------------------------ 2. a uniform grid is a translation
@pytest.mark.parametrize('filtered', [False, True])
@pytest.mark.parametrize('H,W', GRIDS)
def test_uniform_grid_equals_the_folded_translation(H, W, filtered):
    from pytorch_segmentation_amd import ops
    imgs, segs = (_dev(a) for a in _batch(B, H, W))
    nb = G.nbhd_table(G.base_rows(H, W, True), G.filter_of('average 3') if filtered else None)
    wide, folded = warp_table(nb, grid=uniform_grid(3.0, -2.0)), fold_translation(nb, 3.0, -2.0)
    assert (folded[:, [2, 5]] != nb[:, [2, 5]]).all() and wide[0, aug.WARP_GRID_ON] == 1
    shapes = torch.from_numpy(aug.row_shapes(nb))
    for out_hw in out_sizes(H, W):
        oh, ow = out_hw or (H, W)
        want_img, want_lab = ops.augment_batch_nbhd(imgs, segs, _dev(folded), shapes, oh, ow, MEAN, STD)
        got_img, got_lab = ops.augment_batch_warp(imgs, segs, _dev(wide), shapes, oh, ow, MEAN, STD)
        assert torch.equal(got_img, want_img) and torch.equal(got_lab, want_lab), out_hw
        plain = ops.augment_batch_nbhd(imgs, segs, _dev(nb), shapes, oh, ow, MEAN, STD)
        assert not torch.equal(plain[0], want_img) and not torch.equal(plain[1], want_lab)     # the translation does move them


# ------------------------------------------------------------------ 3. perspective, grid, elastic vs fp64
@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('order', [0, 1])
@pytest.mark.parametrize('H,W', GRIDS + TINY)
@pytest.mark.parametrize('case', CASES)
def test_warps_against_fp64(case, H, W, order, mode):
    imgs, segs = _batch(B, H, W)
    tiny = (H, W) in TINY
    rows = tiny_rows(case, H, W, order, mode) if tiny else case_rows(case, H, W, order, mode)
    for out_hw in out_sizes(H, W):
        o = check_against_fp64(imgs, segs, rows, out_hw, nothing_excluded=tiny)
        if out_hw is None and (H, W) in GRIDS:                                 # and the warp is one: it moves most pixels
            still = oracle(imgs, segs, warp_table(np.stack([aug.make_nbhd_row(aug.make_row(None, None, CVAL, order, mode))] * B)))
            assert (o['label'] != still['label']).mean() > 0.5


# ------------------------------------------------------------------ 4. image and mask move together
@pytest.mark.parametrize('H,W', GRIDS)
def test_image_and_mask_move_together(H, W):
    _, segs = _batch(B, H, W)
    imgs = np.ascontiguousarray(np.broadcast_to(segs[:, None], (B, 3, H, W)))
    rows = case_rows('all', H, W, order=0, mode=0, cval=0.0)
    got_img, got_lab = G.run(imgs, segs, rows)
    q = _device_q(got_img)
    assert np.array_equal(q, np.broadcast_to(got_lab[:, None], q.shape).astype(np.float64))      # every pixel, no exclusions
    assert (got_lab != segs).mean() > 0.5 and (got_lab != 0).mean() > 0.5


# ------------------------------------------------------------------ 5. the halo's jitter is the reflected pixel's
@pytest.mark.parametrize('H,W', GRIDS)
def test_elastic_with_filter_against_fp64(H, W):
    imgs, segs = _batch(B, H, W)
    rows = elastic_filter_rows(H, W)
    assert G.is_dyadic(rows[0, aug.NBHD_WEIGHTS:aug.NBHD_WEIGHTS + 9]) and rows[0, aug.NBHD_K] == 3
    decided = oracle(imgs, segs, rows)['label_ok']
    for out_hw in out_sizes(H, W):
        got_img, got_lab = G.run(imgs, segs, rows, out_hw)
        r, q = restate_filtered(imgs, segs, rows, out_hw), _device_q(got_img)
        iy, ix = (np.arange(H), np.arange(W)) if out_hw is None else (G.ms_index(out_hw[0], H), G.ms_index(out_hw[1], W))
        for b in range(B):
            ok = window_decided(decided[b], 3)[iy][:, ix]
            print('elastic + sharpen %dx%d -> %s b=%d: excluded %.4f, max |dq| %g' % (H, W, out_hw, b, 1.0 - ok.mean(), np.abs(q[b] - r['q'][b]).max()))
            assert 1.0 - ok.mean() <= ELASTIC_FILTER_CAP
            assert np.array_equal(q[b][:, ok], r['q'][b][:, ok])
            assert np.array_equal(got_lab[b][decided[b]], r['label'][b][decided[b]])


def restate_with_unreflected_halo(imgs, rows):
    """what a halo filled with the jitter of index -1 / H (and the reflected pixel's matrix) would give: [B,3,H,W]"""
    Bn, _, H, W = imgs.shape
    f, out = imgs.astype(np.float64), []
    for b in range(Bn):
        ys, xs = np.arange(-1, H + 1), np.arange(-1, W + 1)
        # jitter drawn at the unreflected index, added to the reflected pixel's position
        jx, jy, _ = source_coords(rows[b], ys, xs, H, W)
        gy, gx = np.meshgrid(ys, xs, indexing='ij')
        sx, sy = jx - gx + G.reflect101(gx, W), jy - gy + G.reflect101(gy, H)
        nx, ny = np.floor(np.clip(sx, -1.0, W) + 0.5).astype(np.int64), np.floor(np.clip(sy, -1.0, H) + 0.5).astype(np.int64)
        inside = (nx >= 0) & (nx < W) & (ny >= 0) & (ny < H)
        padded = np.where(inside[None], f[b][:, np.clip(ny, 0, H - 1), np.clip(nx, 0, W - 1)], float(rows[b, 18]))
        w = rows[b, aug.NBHD_WEIGHTS:aug.NBHD_WEIGHTS + 9].astype(np.float64).reshape(3, 3)
        out.append(_round8(sum(w[j, i] * padded[:, j:j + H, i:i + W] for j in range(3) for i in range(3))))
    return np.stack(out)


# ------------------------------------------------------------------ 6. seeds
def test_same_seed_same_output_and_samples_differ():
    H, W = GRIDS[0]
    imgs, segs = _batch(B, H, W)
    imgs, segs = np.ascontiguousarray(np.broadcast_to(imgs[:1], imgs.shape)), np.ascontiguousarray(np.broadcast_to(segs[:1], segs.shape))
    rows = warp_table(G.nbhd_table(G.base_rows(H, W, False)), alpha=3.5)
    a_img, a_lab = G.run(imgs, segs, rows)
    b_img, b_lab = G.run(imgs, segs, rows)
    assert np.array_equal(a_img, b_img) and np.array_equal(a_lab, b_lab)
    for i, j in ((0, 1), (1, 2), (0, 2)):                                  # one photo, three seeds
        assert (a_img[i] != a_img[j]).mean() > 0.5 and (a_lab[i] != a_lab[j]).mean() > 0.5
    other = warp_table(G.nbhd_table(G.base_rows(H, W, False), seeds=[11, 12, 13]), alpha=3.5)
    assert (G.run(imgs, segs, other)[0] != a_img).mean() > 0.5


# ------------------------------------------------------------------ 7. footprint and hostile rows
def hostile_tables(H, W, order):
    """[(rows, den or None)]: NaN / inf / 1e30 in h2, in grid nodes and in alpha, and an h2 whose den = 8 - x / 4 (exact in fp32)
    is <= 0 from x = 32 on; every row also carries a 13 x 13 filter, noise and dropout, as the nbhd test's"""
    rng = np.random.default_rng(5)
    kernel = rng.uniform(-1, 1, (13, 13))
    kernel /= np.abs(kernel).sum()
    masks = [(1, 1), (H, W), (0, 0)]
    nb = np.stack([aug.make_nbhd_row(aug.make_row(None, None, CVAL, order, mode), kernel, (12.75, True), (0.1, True) + m, seed)
                   for mode, m, seed in zip((0, 1, 1), masks, SEEDS)])
    tables = []
    for bad in (np.nan, np.inf, -np.inf, 1e30, -1e30):
        grid = rng.normal(0.0, 3.0, (4, 4, 2))
        grid[1, 2, 0], grid[2, 1, 1], grid[3, 3, 0] = bad, -bad, bad
        tables.append((np.stack([aug.make_warp_row(nb[0], h2=(bad, 0.0, 1.0)), aug.make_warp_row(nb[1], grid=grid),
                                 aug.make_warp_row(nb[2], alpha=bad)]), None))
        tables.append((np.stack([aug.make_warp_row(nb[0], h2=(0.0, 0.0, bad), alpha=3.5), aug.make_warp_row(nb[1], h2=(0.0, bad, bad), grid=grid),
                                 aug.make_warp_row(nb[2], alpha=3e38, grid=np.full((4, 4, 2), bad))]), None))
    den = np.broadcast_to(8.0 - np.arange(W) / 4.0, (H, W))
    tables.append((warp_table(nb, h2=(-0.25, 0.0, 8.0)), den))
    return tables


@pytest.mark.parametrize('order', [0, 1])
@pytest.mark.parametrize('H,W,out_hw', [(37, 83, None), (70, 131, (32, 64)), (70, 131, (96, 160))])
def test_hostile_rows_and_output_footprint(H, W, out_hw, order):
    from pytorch_segmentation_amd import ops
    imgs, segs = _batch(B, H, W)
    segs = np.maximum(segs, 1)                                              # no label is 0 by itself
    for rows, den in hostile_tables(H, W, order):
        oh, ow = out_hw or (H, W)
        pad = 4099
        n_out, n_tgt = B * 3 * oh * ow, B * H * W
        big_out = torch.full((n_out + 2 * pad,), -12345.0, dtype=torch.float32, device=DEV)
        big_tgt = torch.full((n_tgt + 2 * pad,), -987654321, dtype=torch.int64, device=DEV)
        out, tgt = ops.augment_batch_warp(_dev(imgs), _dev(segs), _dev(rows), torch.from_numpy(aug.row_shapes(rows)), oh, ow, MEAN,
                                          STD, out=big_out[pad:pad + n_out].view(B, 3, oh, ow),
                                          target=big_tgt[pad:pad + n_tgt].view(B, H, W))
        torch.cuda.synchronize()
        assert (big_out[:pad] == -12345.0).all() and (big_out[pad + n_out:] == -12345.0).all()
        assert (big_tgt[:pad] == -987654321).all() and (big_tgt[pad + n_tgt:] == -987654321).all()
        assert torch.isfinite(out).all() and (out != -12345.0).all() and (tgt != -987654321).all()
        _device_q(out.cpu().numpy())                                        # every value is a normalised 8-bit value
        tgt = tgt.cpu().numpy()
        assert tgt.min() >= 0 and tgt.max() <= 255
        if den is not None:
            assert (den <= 0).any() and (den > 0).any()
            assert (tgt[:, den <= 0] == 0).all() and (tgt[:, den > 0] != 0).mean() > 0.5


def test_refusals_launch_nothing():
    from pytorch_segmentation_amd import _lib, ops
    H, W = GRIDS[0]
    imgs, segs = (_dev(a) for a in _batch(B, H, W))
    rows = _dev(warp_table(G.nbhd_table(G.base_rows(H, W, False), G.filter_of('average 3')), alpha=3.5))
    out = torch.full((B, 3, H, W), -12345.0, dtype=torch.float32, device=DEV)
    tgt = torch.full((B, H, W), -987654321, dtype=torch.int64, device=DEV)
    for bad, what in (([3, 4, 3], 'filter size 4'), ([3, 3, 15], 'filter size 15'), ([-1, 3, 3], 'filter size -1')):
        shapes = torch.tensor([[k, 0, 0] for k in bad], dtype=torch.int32)
        with pytest.raises(_lib.PsegError, match='augment_batch_warp: .*' + what):
            ops.augment_batch_warp(imgs, segs, rows, shapes, H, W, MEAN, STD, out=out, target=tgt)
    for mask in ((-1, 4), (4, -1), (0, 4), (70000, 4)):
        shapes = torch.tensor([[3, 0, 0], [3, 0, 0], [3, mask[0], mask[1]]], dtype=torch.int32)
        with pytest.raises(_lib.PsegError, match='sample 2: dropout mask'):
            ops.augment_batch_warp(imgs, segs, rows, shapes, H, W, MEAN, STD, out=out, target=tgt)
    big = torch.zeros(1, 3, 1300, 1300, dtype=torch.uint8, device=DEV)
    big_rows = warp_table(G.nbhd_table(G.base_rows(8, 8, False)[:1], np.full((13, 13), 1 / 169.)), alpha=3.5)
    with pytest.raises(_lib.PsegError, match='bytes of LDS'):
        ops.augment_batch_warp(big, big[:, 0].contiguous(), _dev(big_rows), torch.tensor([[13, 0, 0]], dtype=torch.int32), 32, 32, MEAN, STD)
    torch.cuda.synchronize()
    assert (out == -12345.0).all() and (tgt == -987654321).all()
    ops.augment_batch_warp(imgs, segs, rows, torch.tensor([[3, 0, 0]] * 3, dtype=torch.int32), H, W, MEAN, STD, out=out, target=tgt)
    assert (out != -12345.0).all() and (tgt != -987654321).all()          # and the valid call does launch


# ------------------------------------------------------------------ 8. end to end
TRAIN_SET = {'n_train': 12, 'batch_size': 12}    # one batch: the first 12 recipes of warps(seed=0) hold a warp (the CPU test checks)


def test_train_with_warps_augment(tmp_path, monkeypatch):
    from pytorch_segmentation_amd import ops
    from pytorch_segmentation_amd.utils.datasets import make_synthetic_coco
    root = make_synthetic_coco(str(tmp_path / 'data'), n_train=TRAIN_SET['n_train'], n_val=2, n_classes=1)
    monkeypatch.chdir(tmp_path)
    import train as train_mod

    made, calls = [], {'warp': 0, 'nbhd': 0, 'plain': 0}

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
    monkeypatch.setattr(ops, 'augment_batch_warp', counted('warp', ops.augment_batch_warp))
    monkeypatch.setattr(ops, 'augment_batch_nbhd', counted('nbhd', ops.augment_batch_nbhd))
    monkeypatch.setattr(ops, 'augment_batch', counted('plain', ops.augment_batch))
    warps = DeviceAugment.warps(seed=0)
    torch.manual_seed(0)
    _, loss = train_mod.train(root, epochs=1, img_size=[64, 64], batch_size=TRAIN_SET['batch_size'], accumulate=1, lr=1e-2,
                              num_workers=0, notest=False, nosave=True, model_name='unet', augment=warps)
    print('loss with the warps augmentation:', loss, calls)
    assert np.isfinite(loss)
    assert [name for name, _ in made] == ['train.json', 'val.json']
    assert made[0][1].augments is warps and made[1][1].augments is None         # validation is not augmented
    assert calls['warp'] >= 1 and sum(calls.values()) == TRAIN_SET['n_train'] // TRAIN_SET['batch_size']
