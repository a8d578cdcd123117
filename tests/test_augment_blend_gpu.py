"""The blend augmentation kernel (pseg_augment_batch_blend, ops.augment_batch_blend, DeviceAugment.blends) on the GPU: the
five bit-for-bit identities of the contract, the median at every window against numpy.sort (every pixel, the grids of one
and five pixels included), median then filter, the mask sampler, the edge and colour blends and hue / saturation against the
fp64 restatement of tests/augment_blend_ref.py, all stages behind a general warp, sentinel-guarded outputs under hostile
rows, the entry point's refusals, and one training epoch with DeviceAugment.blends().

Comparison rule wherever pixels are excluded: every pixel within one 8-bit step of the restatement, equal where every
pre-rounding value behind it lies further from a half-integer than the stage's margin (augment_blend_ref: the filters'
accumulation bound, 2e-3 for a mask blend, 0.01 for the mask sampler alone and for hue / saturation), and the excluded share
below the cap (2 % with filters, 5 % for the sampler and hue / saturation).  The caps are properties of the restatement and
the inputs; tests/test_augment_blend_cpu.py::test_restatement_stays_inside_the_caps finds them without a GPU.

Measured on one MI355X -- the largest excluded share of a sample and the device's largest distance from the restatement on
any pixel, excluded ones included: median 5 then Gaussian 1.7 / composed K=13: 0.0024 / 0.0161, 1 step; the mask sampler:
0.022, 0; edge blend over average 2 (dyadic) / average 3: 0.0052 / 0.0073, 0 / 1 step; colour blend: 0.0046, 0; hue /
saturation: 0.0259, 1 step; every compared pixel equal; the medians, the identities and the labels equal on every pixel."""
import os

import numpy as np
import pytest
import torch

from pytorch_segmentation_amd.utils import augment as aug
from pytorch_segmentation_amd.utils.augment import DeviceAugment
from pytorch_segmentation_amd.utils.datasets import MEAN, STD

import augment_blend_ref as R
import test_augment_nbhd_gpu as G
import test_augment_warp_gpu as Wp
from test_augment_gpu import _batch, _dev, _device_q

pytestmark = pytest.mark.gpu
DEV = 'cuda'
B = G.B
GRIDS = G.GRIDS
TINY = R.TINY


def run_blend(imgs, segs, rows, out_hw=None):
    assert rows.shape == (B, aug.BLEND_ROW)
    return G.run(imgs, segs, rows, out_hw)


def same_bits(imgs, segs, a, b, out_hw=None):
    """the outputs of two tables (any of the wide kernels) are equal bit for bit"""
    ia, la = G.run(imgs, segs, a, out_hw)
    ib, lb = G.run(imgs, segs, b, out_hw)
    assert np.array_equal(ia.view(np.uint32), ib.view(np.uint32)) and np.array_equal(la, lb)
    return ia


def compare(q, r, cap, what):
    for b in range(B):
        excl, worst = R.excluded(r, b), np.abs(q[b] - r['q'][b]).max()
        print('%s b=%d: excluded %.4f, max |dq| %g' % (what, b, excl, worst))
        assert excl <= cap
        assert np.array_equal(q[b][r['ok'][b]], r['q'][b][r['ok'][b]])
        assert worst <= 1.0


# ------------------------------------------------------------------ 1. the five identities, bit for bit
@pytest.mark.parametrize('H,W', GRIDS + TINY)
def test_rows_without_blend_fields_equal_augment_batch_warp(H, W):
    imgs, segs = _batch(B, H, W)
    for order in (0, 1):
        for case in ('all', 'plain'):
            warp = Wp.case_rows('all', H, W, order, 1) if case == 'all' else np.stack(R.warp_rows(H, W, True, G.filter_of('gaussian 1.7')))
            if case == 'all':                                   # and a filter, noise and dropout on top
                for b in range(B):
                    nb = aug.make_nbhd_row(warp[b, :aug.ROW], G.filter_of('composed 13'), (10.0, True), (0.1, False, 5, 9), G.SEEDS[b])
                    warp[b].view(np.uint32)[aug.ROW:aug.NBHD_ROW] = nb.view(np.uint32)[aug.ROW:]
            wide = R.blend_table(warp)
            assert not wide[:, aug.BLEND_KMED:aug.BLEND_MB].any() and aug.row_shapes(wide).shape == (B, 5)
            for out_hw in G.out_sizes(H, W):
                same_bits(imgs, segs, wide, warp, out_hw)


@pytest.mark.parametrize('H,W', GRIDS)
def test_constant_tables_select_one_branch(H, W):
    imgs, segs = _batch(B, H, W)
    zeros, ones = np.zeros((16, 16), dtype=np.float32), np.ones((16, 16), dtype=np.float32)
    F, G2 = G.filter_of('gaussian 1.7'), aug.compose_filters([G.filter_of('gaussian 1.7'), aug.edge_kernel(0.75, 0.3)])
    assert G2.shape == (7, 7)
    with_f, with_g, no_f = R.warp_rows(H, W, True, F), R.warp_rows(H, W, True, G2), R.warp_rows(H, W, True)
    for out_hw in G.out_sizes(H, W):
        # T1 all 0: the row with K2 = 0;  T1 all 1: the row whose F is G, no blend (also without an F of its own)
        a = same_bits(imgs, segs, R.blend_table(with_f, kernel2=G2, t1=zeros), R.blend_table(with_f), out_hw)
        b = same_bits(imgs, segs, R.blend_table(with_f, kernel2=G2, t1=ones), R.blend_table(with_g), out_hw)
        same_bits(imgs, segs, R.blend_table(no_f, kernel2=G2, t1=ones), np.stack(with_g), out_hw)
        assert (a != b).mean() > 0.5
        # T2 all 1: M alone;  T2 all 0: Mb in M's place
        with_ma, with_mb = R.warp_rows(H, W, True, F, colour=R.MA), R.warp_rows(H, W, True, F, colour=R.MB)
        a = same_bits(imgs, segs, R.blend_table(with_ma, colour2=R.MB, t2=ones), np.stack(with_ma), out_hw)
        b = same_bits(imgs, segs, R.blend_table(with_ma, colour2=R.MB, t2=zeros), np.stack(with_mb), out_hw)
        assert (a != b).mean() > 0.5


# ------------------------------------------------------------------ 2. the median
@pytest.mark.parametrize('H,W', GRIDS + TINY)
@pytest.mark.parametrize('k', R.MEDIANS)
def test_median_equals_numpy_sort(k, H, W):
    imgs, segs = _batch(B, H, W)
    rows = R.median_rows(H, W, k)
    for out_hw in G.out_sizes(H, W):
        got_img, got_lab = run_blend(imgs, segs, rows, out_hw)
        r = R.restate(imgs, segs, rows, out_hw)
        assert r['ok'].all()                                      # nothing is excluded
        assert np.array_equal(_device_q(got_img), r['q']) and np.array_equal(got_lab, r['label'])
    if (H, W) in GRIDS:                                           # and the median is one: it changes most pixels
        assert (R.restate(imgs, segs, rows)['q'] != R.restate(imgs, segs, R.median_rows(H, W, 0))['q']).mean() > 0.5


@pytest.mark.parametrize('H,W', GRIDS)
@pytest.mark.parametrize('name', ['gaussian 1.7', 'composed 13'])
def test_median_then_filter_against_fp64(name, H, W):
    imgs, segs = _batch(B, H, W)
    kernel = G.filter_of(name)
    assert kernel.shape[0] == (13 if name == 'composed 13' else 5)
    rows = R.median_rows(H, W, 5, True, kernel)
    for out_hw in G.out_sizes(H, W):
        got_img, got_lab = run_blend(imgs, segs, rows, out_hw)
        r = R.restate(imgs, segs, rows, out_hw)
        assert np.array_equal(got_lab, r['label'])
        compare(_device_q(got_img), r, G.excluded_cap(name), 'median 5 + %s %dx%d -> %s' % (name, H, W, out_hw))


# ------------------------------------------------------------------ 3. masks
@pytest.mark.parametrize('H,W', GRIDS + TINY)
def test_mask_sampler_against_fp64(H, W):
    imgs, segs = _batch(B, H, W)
    rows = R.sampler_rows(H, W)
    for out_hw in G.out_sizes(H, W):
        q = _device_q(run_blend(imgs, segs, rows, out_hw)[0])
        iy, ix = (np.arange(H), np.arange(W)) if out_hw is None else (G.ms_index(out_hw[0], H), G.ms_index(out_hw[1], W))
        want = 255.0 * (1.0 - R.mask_sample(rows[0, aug.BLEND_T2:aug.BLEND_T2 + 256], H, W))[iy][:, ix]
        ok = R._half_distance(want) > R.SAMPLER_MARGIN
        print('sampler %dx%d -> %s: excluded %.4f, max |dq| %g' % (H, W, out_hw, 1.0 - ok.mean(), np.abs(q - R._round8(want)).max()))
        assert 1.0 - ok.mean() <= R.SAMPLER_CAP
        assert np.abs(q - R._round8(want)).max() <= 1.0
        assert np.array_equal(q[:, :, ok], np.broadcast_to(R._round8(want)[ok], q[:, :, ok].shape))
        if (H, W) in GRIDS:
            assert len(np.unique(q)) > 64                         # the table's whole range is there


@pytest.mark.parametrize('H,W', GRIDS)
@pytest.mark.parametrize('case', range(len(R.EDGE_CASES)))
def test_edge_blend_against_fp64(case, H, W):
    imgs, segs = _batch(B, H, W)
    rows = R.edge_rows(H, W, *R.EDGE_CASES[case])
    for out_hw in G.out_sizes(H, W):
        got_img, got_lab = run_blend(imgs, segs, rows, out_hw)
        r = R.restate(imgs, segs, rows, out_hw)
        assert np.array_equal(got_lab, r['label'])
        compare(_device_q(got_img), r, R.FILTER_CAP, 'edge blend %s %dx%d -> %s' % (R.EDGE_CASES[case], H, W, out_hw))


@pytest.mark.parametrize('H,W', GRIDS)
def test_colour_blend_against_fp64(H, W):
    imgs, segs = _batch(B, H, W)
    rows = R.colour_rows(H, W)
    for out_hw in G.out_sizes(H, W):
        got_img, got_lab = run_blend(imgs, segs, rows, out_hw)
        r = R.restate(imgs, segs, rows, out_hw)
        assert np.array_equal(got_lab, r['label'])
        compare(_device_q(got_img), r, R.FILTER_CAP, 'colour blend %dx%d -> %s' % (H, W, out_hw))


# ------------------------------------------------------------------ 4. hue and saturation
@pytest.mark.parametrize('shift', range(len(R.HUE_V) + 1))
def test_hue_saturation_against_fp64(shift):
    H, W = GRIDS[0]
    imgs, segs = R.hue_batch()
    dh_ds = R.hue_shifts()[shift]
    rows = R.hue_rows(H, W, dh_ds)
    q = _device_q(run_blend(imgs, segs, rows)[0])
    r = R.restate(imgs, segs, rows)
    compare(q, r, R.SAMPLER_CAP, 'hue / saturation dh %.4f ds %.4f' % dh_ds)
    if dh_ds == (0.0, 0.0):                                       # v = 0 is the identity, bit for bit
        assert np.array_equal(q, imgs.astype(np.float64))
        same_bits(imgs, segs, rows, np.stack(R.warp_rows(H, W, False)))
    else:
        assert (q != imgs).mean() > 0.5


# ------------------------------------------------------------------ 5. everything behind a general warp
def all_rows(H, W, order=1, mode=1):
    """Wp.case_rows('all') with a median, F and G, both colour matrices, hue / saturation, noise and coarse dropout on top"""
    warp = Wp.case_rows('all', H, W, order, mode)
    F = G.filter_of('gaussian 1.7')
    G2 = aug.compose_filters([F, aug.edge_kernel(0.75, None)])
    out = []
    for b in range(B):
        base = aug.make_row(None, R.MA, G.CVAL, order, mode)
        base[0:6] = warp[b, 0:6]
        nb = aug.make_nbhd_row(base, F, (10.0, True), (0.1, False, 5, 9), Wp.SEEDS[b])
        wr = warp[b].copy()
        wr.view(np.uint32)[:aug.NBHD_ROW] = nb.view(np.uint32)
        out.append(aug.make_blend_row(wr, 3 + 4 * b, G2, R.MB, R.random_table(20 + b), R.random_table(30 + b), aug.hue_sat_shift(20 - 13 * b)))
    return np.stack(out), warp


@pytest.mark.parametrize('H,W', GRIDS)
def test_all_stages_behind_a_general_warp(H, W):
    imgs, segs = _batch(B, H, W)
    rows, warp = all_rows(H, W)
    assert aug.row_shapes(rows).tolist() == [[5, 5, 9, 3 + 4 * b, 7] for b in range(B)]
    for out_hw in G.out_sizes(H, W):
        a_img, a_lab = run_blend(imgs, segs, rows, out_hw)
        b_img, b_lab = run_blend(imgs, segs, rows, out_hw)
        assert np.isfinite(a_img).all()
        _device_q(a_img)                                          # every value is a normalised 8-bit value
        assert np.array_equal(a_img.view(np.uint32), b_img.view(np.uint32)) and np.array_equal(a_lab, b_lab)
        assert np.array_equal(a_lab, G.run(imgs, segs, warp, out_hw)[1])      # the new stages never touch labels
        assert (a_img != G.run(imgs, segs, warp, out_hw)[0]).mean() > 0.5


# ------------------------------------------------------------------ 6. footprint and hostile rows
def hostile_tables(H, W, order):
    """honest shape_host, hostile device rows: kmed, K2, the tables, dh and ds NaN, infinite, huge or negative"""
    rows, _ = all_rows(H, W, order)
    shapes = aug.row_shapes(rows)
    tables = []
    for bad in (np.nan, np.inf, -np.inf, 1e30, -1e30, -5.0, 1e6):
        t = rows.copy()
        t[0, aug.BLEND_KMED], t[1, aug.BLEND_K2], t[2, aug.BLEND_KMED], t[2, aug.BLEND_K2] = bad, bad, -bad, bad
        t[0, aug.BLEND_T1:aug.BLEND_T1 + 256:3], t[1, aug.BLEND_T2:aug.BLEND_T2 + 256:5], t[2, aug.BLEND_T1:aug.BLEND_T2 + 256] = bad, -bad, bad
        t[0, aug.BLEND_HUE], t[1, aug.BLEND_HUE + 1], t[2, aug.BLEND_HUE:aug.BLEND_HUE + 2] = bad, bad, (-bad, bad)
        tables.append((t, shapes))
    # and rows whose windows are LARGER than shape_host says: the kernel must fall back, not write past its LDS
    small = shapes.copy()
    small[:, 0], small[:, 3], small[:, 4] = 0, 0, 3
    tables.append((rows.copy(), small))
    return tables


@pytest.mark.parametrize('order', [0, 1])
@pytest.mark.parametrize('H,W,out_hw', [(37, 83, None), (70, 131, (32, 64)), (70, 131, (96, 160))])
def test_hostile_rows_and_output_footprint(H, W, out_hw, order):
    from pytorch_segmentation_amd import ops
    imgs, segs = _batch(B, H, W)
    for rows, shapes in hostile_tables(H, W, order):
        oh, ow = out_hw or (H, W)
        pad = 4099
        n_out, n_tgt = B * 3 * oh * ow, B * H * W
        big_out = torch.full((n_out + 2 * pad,), -12345.0, dtype=torch.float32, device=DEV)
        big_tgt = torch.full((n_tgt + 2 * pad,), -987654321, dtype=torch.int64, device=DEV)
        out, tgt = ops.augment_batch_blend(_dev(imgs), _dev(segs), _dev(rows), torch.from_numpy(shapes), oh, ow, MEAN, STD,
                                           out=big_out[pad:pad + n_out].view(B, 3, oh, ow), target=big_tgt[pad:pad + n_tgt].view(B, H, W))
        torch.cuda.synchronize()
        assert (big_out[:pad] == -12345.0).all() and (big_out[pad + n_out:] == -12345.0).all()
        assert (big_tgt[:pad] == -987654321).all() and (big_tgt[pad + n_tgt:] == -987654321).all()
        assert torch.isfinite(out).all() and (out != -12345.0).all() and (tgt != -987654321).all()
        _device_q(out.cpu().numpy())                                # every value is a normalised 8-bit value
        tgt = tgt.cpu().numpy()
        assert tgt.min() >= 0 and tgt.max() <= 255


def test_refusals_launch_nothing():
    from pytorch_segmentation_amd import _lib, ops
    H, W = GRIDS[0]
    imgs, segs = (_dev(a) for a in _batch(B, H, W))
    rows = _dev(R.median_rows(H, W, 3, False, G.filter_of('average 3')))
    out = torch.full((B, 3, H, W), -12345.0, dtype=torch.float32, device=DEV)
    tgt = torch.full((B, H, W), -987654321, dtype=torch.int64, device=DEV)

    def call(shapes, **kw):
        a = dict(imgs=imgs, segs=segs, params=rows, out=out, target=tgt)
        a.update(kw)
        return ops.augment_batch_blend(a['imgs'], a['segs'], a['params'], torch.tensor(shapes, dtype=torch.int32), H, W, MEAN, STD,
                                       out=a['out'], target=a['target'])
    good = [3, 0, 0, 3, 0]
    for bad, what in (([3, 0, 0, 4, 0], 'median window 4'), ([3, 0, 0, 13, 0], 'median window 13'), ([3, 0, 0, 1, 0], 'median window 1'),
                      ([3, 0, 0, -3, 0], 'median window -3'), ([3, 0, 0, 3, 4], 'second filter size 4'), ([3, 0, 0, 3, 17], 'second filter size 17'),
                      ([3, 0, 0, 3, 1], 'second filter size 1'), ([3, 0, 0, 3, -1], 'second filter size -1'), ([4, 0, 0, 3, 0], 'filter size 4'),
                      ([15, 0, 0, 3, 0], 'filter size 15'), ([3, 0, 4, 3, 0], 'dropout mask'), ([3, 70000, 4, 3, 0], 'dropout mask')):
        with pytest.raises(_lib.PsegError, match='augment_batch_blend: sample 2: .*' + what):
            call([good, good, bad])
    with pytest.raises(_lib.PsegError, match='augment_batch_blend: null pointer'):
        _lib.call('pseg_augment_batch_blend', imgs.data_ptr(), segs.data_ptr(), None, torch.tensor([good] * 3, dtype=torch.int32).data_ptr(),
                  B, H, W, *MEAN, *STD, out.data_ptr(), H, W, tgt.data_ptr(), None)
    with pytest.raises(_lib.PsegError, match='augment_batch_blend: null pointer'):
        _lib.call('pseg_augment_batch_blend', imgs.data_ptr(), segs.data_ptr(), rows.data_ptr(), None, B, H, W, *MEAN, *STD, out.data_ptr(),
                  H, W, tgt.data_ptr(), None)
    # LDS: two tiles around the span of a 32 x 8 output tile of a 40-fold reduction do not fit
    big = torch.zeros(1, 3, 1300, 1300, dtype=torch.uint8, device=DEV)
    big_rows = _dev(R.blend_table(R.warp_rows(8, 8, False, np.full((13, 13), 1 / 169.))[:1], kmed=11))
    with pytest.raises(_lib.PsegError, match='kmed = 11, K = 13, K2 = 0 needs .* bytes of LDS'):
        ops.augment_batch_blend(big, big[:, 0].contiguous(), big_rows, torch.tensor([[13, 0, 0, 11, 0]], dtype=torch.int32), 32, 32, MEAN, STD)
    torch.cuda.synchronize()
    assert (out == -12345.0).all() and (tgt == -987654321).all()
    call([good] * 3)
    assert (out != -12345.0).all() and (tgt != -987654321).all()          # and the valid call does launch


# ------------------------------------------------------------------ 7. end to end
TRAIN_SET = {'n_train': 12, 'batch_size': 12}    # one batch: the first 12 recipes of blends(seed=0) hold a blend (the CPU test checks)


def test_train_with_blends_augment(tmp_path, monkeypatch):
    from pytorch_segmentation_amd import ops
    from pytorch_segmentation_amd.utils.datasets import make_synthetic_coco
    root = make_synthetic_coco(str(tmp_path / 'data'), n_train=TRAIN_SET['n_train'], n_val=2, n_classes=1)
    monkeypatch.chdir(tmp_path)
    import train as train_mod

    made, calls = [], {'blend': 0, 'warp': 0, 'nbhd': 0, 'plain': 0}

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
    for name, attr in (('blend', 'augment_batch_blend'), ('warp', 'augment_batch_warp'), ('nbhd', 'augment_batch_nbhd'), ('plain', 'augment_batch')):
        monkeypatch.setattr(ops, attr, counted(name, getattr(ops, attr)))
    blends = DeviceAugment.blends(seed=0)
    torch.manual_seed(0)
    _, loss = train_mod.train(root, epochs=1, img_size=[64, 64], batch_size=TRAIN_SET['batch_size'], accumulate=1, lr=1e-2,
                              num_workers=0, notest=False, nosave=True, model_name='unet', augment=blends)
    print('loss with the blends augmentation:', loss, calls)
    assert np.isfinite(loss)
    assert [name for name, _ in made] == ['train.json', 'val.json']
    assert made[0][1].augments is blends and made[1][1].augments is None        # validation is not augmented
    assert calls['blend'] >= 1 and sum(calls.values()) == TRAIN_SET['n_train'] // TRAIN_SET['batch_size']
