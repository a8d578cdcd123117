"""The augmentation kernel (csrc/augment.hip, ops.augment_batch, utils/augment.py) on the GPU: identity rows against the
loader's own post_fetch_fn (bit for bit), warps and colour matrices against an fp64 restatement in numpy, far and
non-finite coordinates with sentinel-guarded outputs, and one training epoch through train.py --augment."""
import json
import os
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pytorch_segmentation_amd.utils import augment as aug
from pytorch_segmentation_amd.utils.augment import DeviceAugment
from pytorch_segmentation_amd.utils.datasets import MEAN, STD

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SHAPES = [(1, 1), (37, 53), (48, 80), (64, 96)]
BATCHES = [1, 6]
# (rotate deg, scale x, scale y, shear deg, translate x, translate y, fliplr, flipud) about the image centre
WARPS = [(30, .8, 1.2, 16, .1, -.2, 1, 0), (-90, 1, 1, 0, 0, 0, 0, 0), (45, 1.2, .8, -16, -.2, .2, 0, 1),
         (7.3, 1.1, .9, 5, .03, .07, 1, 1), (0, 1, 1, 0, 0, 0, 1, 0), (-61, .93, 1.17, -9, .11, .05, 0, 0)]
CVAL = 77.0


# ------------------------------------------------------------------ inputs
def _photo(H, W, seed):
    """the content of tests/test_inference_gpu.py::_photos: smooth sinusoids plus N(0, 30) noise, here planar [3,H,W]"""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.linspace(0, 6, H), np.linspace(0, 9, W), indexing='ij')
    base = 127.5 + 100 * np.sin(yy[..., None] + xx[..., None] * np.array([1.0, 0.7, 1.3]))
    return np.clip(base + rng.normal(0, 30, (H, W, 3)), 0, 255).astype(np.uint8).transpose(2, 0, 1).copy()


_BATCH = {}


def _batch(B, H, W):
    """(imgs uint8 [B,3,H,W], segs uint8 [B,H,W]) numpy, made once per shape and never modified"""
    key = (B, H, W)
    if key not in _BATCH:
        rng = np.random.default_rng(1000 + H)
        imgs = np.stack([_photo(H, W, i) for i in range(B)])
        segs = rng.integers(0, 21, (B, H, W)).astype(np.uint8)
        segs[:, 0, 0] = 255                      # the widest label value must survive the widening
        imgs.setflags(write=False)
        segs.setflags(write=False)
        _BATCH[key] = (imgs, segs)
    return _BATCH[key]


def _warp_inverse(H, W, rot, sx, sy, sh, tx, ty, fl, fu):
    """output index -> source index of: flip, scale, shear, rotate about the centre, translate by fractions of the size"""
    c = np.array([[1, 0, (W - 1) / 2], [0, 1, (H - 1) / 2], [0, 0, 1.]])
    r, s = np.deg2rad(rot), np.deg2rad(sh)
    R = np.array([[np.cos(r), -np.sin(r), 0], [np.sin(r), np.cos(r), 0], [0, 0, 1]])
    S, Sh = np.diag([sx, sy, 1.]), np.array([[1, -np.tan(s), 0], [0, 1, 0], [0, 0, 1.]])
    Fl = np.diag([-1. if fl else 1., -1. if fu else 1., 1.])
    T = np.array([[1, 0, tx * W], [0, 1, ty * H], [0, 0, 1.]])
    return np.linalg.inv(T @ c @ R @ Sh @ S @ Fl @ np.linalg.inv(c))


# ------------------------------------------------------------------ device call
def _dev(a):
    return torch.tensor(a, device=DEV)              # a copy: the shared inputs are read-only arrays


def _run(imgs, segs, rows, out_hw=None):
    """numpy in, numpy out: (out fp32 [B,3,oh,ow], target int64 [B,H,W])"""
    out, tgt = DeviceAugment.identity().apply(_dev(imgs), _dev(segs), rows, out_hw)
    assert out.dtype == torch.float32 and tgt.dtype == torch.int64 and out.is_contiguous() and tgt.is_contiguous()
    return out.cpu().numpy(), tgt.cpu().numpy()


# ------------------------------------------------------------------ fp64 restatement (operation order of the kernel)
def _normalise32(q):
    """the kernel's last step on 8-bit values q [B,3,h,w]: fp32 subtraction, correctly rounded fp32 division"""
    m = np.asarray(MEAN, dtype=np.float32).reshape(1, 3, 1, 1)
    s = np.asarray(STD, dtype=np.float32).reshape(1, 3, 1, 1)
    return (q.astype(np.float32) - m) / s


def _round8(v):
    return np.clip(np.floor(v + 0.5), 0, 255)


def _half_distance(v):
    """distance of v from the nearest half-integer"""
    return np.abs(v - np.floor(v) - 0.5)


def _oracle(imgs, segs, rows, out_hw=None):
    B, _, H, W = imgs.shape
    oh, ow = (H, W) if out_hw is None else out_hw
    f = imgs.astype(np.float64)
    res = {k: [] for k in ('warp', 'stage', 'q', 'img_ok', 'label', 'label_ok')}
    for b in range(B):
        row = rows[b].astype(np.float64)
        A, M = row[0:6].reshape(2, 3), row[6:18].reshape(3, 4)
        cval, bilinear, edge = row[18], row[19] != 0, row[20] != 0

        def coords(ys, xs):
            gy, gx = np.meshgrid(ys.astype(np.float64), xs.astype(np.float64), indexing='ij')
            with np.errstate(invalid='ignore', over='ignore'):
                sx, sy = A[0, 0] * gx + A[0, 1] * gy + A[0, 2], A[1, 0] * gx + A[1, 1] * gy + A[1, 2]
            finite = np.isfinite(sx) & np.isfinite(sy)
            return np.where(finite, sx, -1.0), np.where(finite, sy, -1.0), finite

        def near(sx, sy):
            return np.floor(np.clip(sx, -1.0, W) + 0.5).astype(np.int64), np.floor(np.clip(sy, -1.0, H) + 0.5).astype(np.int64)

        def decided(sx, sy):
            """the nearest sample is decided: s + 0.5 lies more than 1e-3 from an integer on both axes"""
            dx, dy = np.abs(sx + 0.5 - np.round(sx + 0.5)), np.abs(sy + 0.5 - np.round(sy + 0.5))
            return (dx > 1e-3) & (dy > 1e-3)

        # labels: [H, W], nearest, 0 outside
        sx, sy, finite = coords(np.arange(H), np.arange(W))
        x, y = near(sx, sy)
        inside = finite & (x >= 0) & (x < W) & (y >= 0) & (y < H)
        res['label'].append(np.where(inside, segs[b][np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)], 0).astype(np.int64))
        res['label_ok'].append(decided(sx, sy))

        # image: multi-scale index as ATen's nearest, in fp32
        ix = np.minimum(np.floor(np.arange(ow, dtype=np.float32) * (np.float32(W) / np.float32(ow))).astype(np.int64), W - 1)
        iy = np.minimum(np.floor(np.arange(oh, dtype=np.float32) * (np.float32(H) / np.float32(oh))).astype(np.int64), H - 1)
        sx, sy, finite = coords(iy, ix)
        use_edge = edge & finite

        def tap(y, x):
            ok = use_edge | (finite & (y >= 0) & (y < H) & (x >= 0) & (x < W))
            return np.where(ok[None], f[b][:, np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)], cval)

        if not bilinear:
            x, y = near(sx, sy)
            v = tap(y, x)
            ok = np.broadcast_to(decided(sx, sy)[None], v.shape)
        else:
            cx, cy = np.clip(sx, -1.0, W), np.clip(sy, -1.0, H)
            x0, y0 = np.floor(cx).astype(np.int64), np.floor(cy).astype(np.int64)
            lx, ly = (cx - x0)[None], (cy - y0)[None]
            v = (1 - ly) * ((1 - lx) * tap(y0, x0) + lx * tap(y0, x0 + 1)) + ly * ((1 - lx) * tap(y0 + 1, x0) + lx * tap(y0 + 1, x0 + 1))
            ok = _half_distance(v) > 0.05            # per element: each channel has its own pre-rounding value
        w8 = _round8(v)
        stage = np.einsum('ck,khw->chw', M[:, :3], w8) + M[:, 3][:, None, None]
        res['warp'].append(v)
        res['stage'].append(stage)
        res['q'].append(_round8(stage))
        res['img_ok'].append(ok)
    return {k: np.stack(v) for k, v in res.items()}


def _device_q(out):
    """the kernel's 8-bit values, recovered from its normalised output -- and the output is exactly their normalisation"""
    m = np.asarray(MEAN, dtype=np.float64).reshape(1, 3, 1, 1)
    s = np.asarray(STD, dtype=np.float64).reshape(1, 3, 1, 1)
    q = np.rint(out.astype(np.float64) * s + m)
    assert q.min() >= 0 and q.max() <= 255
    assert np.array_equal(out, _normalise32(q)), 'the output is not the fp32 normalisation of an 8-bit value'
    return q


# ------------------------------------------------------------------ 1. identity == the loader
@pytest.fixture(scope='module')
def loader(tmp_path_factory):
    from pytorch_segmentation_amd.utils.datasets import CocoDataset
    path = tmp_path_factory.mktemp('coco') / 'train.json'
    path.write_text(json.dumps({'categories': [{'name': 'a'}], 'images': [], 'annotations': []}))
    return lambda **kw: CocoDataset(str(path), **kw)


@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('H,W', SHAPES)
def test_identity_rows_equal_post_fetch_fn(loader, H, W, B):
    imgs, segs = (_dev(a) for a in _batch(B, H, W))
    want_img, want_seg = loader().post_fetch_fn((imgs, segs))
    hws = [None] + ([(32, 64), (96, 128)] if (H, W) == (64, 96) else [])
    for order in (0, 1):
        a = DeviceAugment.identity(order=order, seed=0)
        for out_hw in hws:
            got_img, got_seg = a(imgs, segs, out_hw)
            want = want_img if out_hw is None else F.interpolate(want_img, out_hw)
            assert got_img.shape == want.shape and got_img.dtype == want.dtype
            assert torch.equal(got_img, want), (order, out_hw)
            assert got_seg.dtype == torch.int64 and torch.equal(got_seg, want_seg)


def test_dataset_with_identity_augment_equals_dataset_without(loader):
    """through CocoDataset.post_fetch_fn, multi-scale draw included: the same seed gives the same size and the same tensors"""
    imgs, segs = (_dev(a) for a in _batch(6, 64, 96))
    plain, fused = loader(multi_scale=True), loader(multi_scale=True, augments=DeviceAugment.identity(seed=0))
    sizes = set()
    for seed in range(4):
        random.seed(seed)
        a_img, a_seg = plain.post_fetch_fn((imgs, segs))
        random.seed(seed)
        b_img, b_seg = fused.post_fetch_fn((imgs, segs))
        assert torch.equal(a_img, b_img) and torch.equal(a_seg, b_seg)
        sizes.add(tuple(a_img.shape[2:]))
    assert len(sizes) > 1


# ------------------------------------------------------------------ 2. warp vs fp64
def _check_warp(imgs, segs, rows, out_hw, stats_required):
    got_img, got_lab = _run(imgs, segs, rows, out_hw)
    o = _oracle(imgs, segs, rows, out_hw)
    q = _device_q(got_img)
    bilinear = rows[0, 19] != 0
    for b in range(imgs.shape[0]):
        lab_ok, img_ok = o['label_ok'][b], o['img_ok'][b]
        excl_lab, excl_img = 1.0 - lab_ok.mean(), 1.0 - img_ok.mean()
        print('warp %s b=%d order=%d mode=%d: labels excluded %.4f, image excluded %.4f, max |dq| %g'
              % (imgs.shape, b, rows[b, 19], rows[b, 20], excl_lab, excl_img, np.abs(q[b] - o['q'][b]).max()))
        if stats_required:
            assert excl_lab <= 0.02 and excl_img <= (0.15 if bilinear else 0.02)
        assert np.array_equal(got_lab[b][lab_ok], o['label'][b][lab_ok])
        assert np.array_equal(q[b][img_ok], o['q'][b][img_ok])
        if bilinear:
            assert np.abs(q[b] - o['q'][b]).max() <= 1.0     # every pixel within one 8-bit step


@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('H,W', SHAPES)
def test_warp_against_fp64(H, W, B):
    imgs, segs = _batch(B, H, W)
    inverses = [_warp_inverse(H, W, *w) for w in WARPS]
    for mode in (0, 1):
        for order in (0, 1):
            table = np.stack([aug.make_row(inv, None, CVAL, order, mode) for inv in inverses])
            if B == 6:
                _check_warp(imgs, segs, table, None, stats_required=(H, W) != (1, 1))     # a different row per sample
            else:
                for i in range(len(WARPS)):
                    _check_warp(imgs, segs, table[i:i + 1], None, stats_required=(H, W) != (1, 1))


def test_warp_with_multi_scale_against_fp64():
    imgs, segs = _batch(6, 64, 96)
    for out_hw in ((32, 64), (96, 128)):
        for order in (0, 1):
            table = np.stack([aug.make_row(_warp_inverse(64, 96, *w), None, CVAL, order, order) for w in WARPS])
            _check_warp(imgs, segs, table, out_hw, stats_required=False)


# ------------------------------------------------------------------ 3. colour
# (factors such as 1.3 or 1.1 put every tenth 8-bit value within rounding error of a half-integer: 1.3 * 5 = 6.5; the
# third channel's factors are chosen off that grid so that few values are undecided)
COLOURS = {
    'add': [('add', [7.0, -10.0, 3.0])],
    'multiply 1.5': [('multiply', [1.5, 1.5, 1.5])],
    'multiply per channel': [('multiply', [0.5, 1.5, 1.1371])],
    'contrast': [('contrast', [0.5, 2.0, 1.3141])],
    'invert': [('invert', [True, True, True])],
    'invert two': [('invert', [True, False, True])],
    'grayscale': [('grayscale', 0.6)],
    'composed': [('add', [-10.0, 4.0, 9.0]), ('contrast', [1.7, 1.7, 1.7]), ('grayscale', 0.35), ('invert', [False, True, False]),
                 ('multiply', [1.5, 0.8, 1.2])],
}


@pytest.mark.parametrize('name', sorted(COLOURS))
def test_colour_matrix_against_fp64(name):
    imgs, segs = _batch(6, 48, 80)
    row = aug.make_row(None, aug.colour_matrix(COLOURS[name]), 0.0, 0, 0)
    table = np.stack([row] * 6)
    got_img, got_lab = _run(imgs, segs, table)
    o = _oracle(imgs, segs, table)
    q = _device_q(got_img)
    assert np.array_equal(got_lab, segs.astype(np.int64))            # colour never touches the labels
    # A stage value EXACTLY on a half-integer (Multiply 1.5 of an odd value, contrast 0.5 of an even one) is checked, not
    # excluded: such ties only arise from dyadic coefficients, for which the kernel's fp32 arithmetic is exact, and then
    # they round half up.  Excluded: values within 1e-3 of a half-integer but not on it.
    d = _half_distance(o['stage'])
    ok = (d > 1e-3) | (d == 0.0)
    print('colour %s: excluded %.4f, saturated low %d high %d' % (name, 1.0 - ok.mean(), (o['stage'] < 0).sum(), (o['stage'] > 255).sum()))
    assert 1.0 - ok.mean() <= 0.02
    assert np.array_equal(q[ok], o['q'][ok])
    if name in ('multiply 1.5', 'composed'):
        assert (o['stage'] > 255.5).any() and q.max() == 255         # saturation above
    if name in ('add', 'contrast', 'composed'):
        assert (o['stage'] < -0.5).any() and q.min() == 0            # and below
    if name == 'invert':
        assert np.array_equal(q, 255.0 - imgs)


# ------------------------------------------------------------------ 4. far and non-finite coordinates, guarded outputs
@pytest.mark.parametrize('order', [0, 1])
@pytest.mark.parametrize('mode', [0, 1])
def test_far_translation_and_output_footprint(mode, order):
    B, H, W = 6, 37, 53
    imgs, segs = _batch(B, H, W)
    table = np.stack([aug.make_row(None, None, CVAL, order, mode) for _ in range(B)])
    table[0, 2] = 1e6                       # far right: the source lies a million pixels past the right edge
    table[1, 2] = -1e6
    table[2, 5] = 1e6
    table[3, 2], table[3, 5] = -1e6, -1e6
    table[4, 2] = np.nan                    # non-finite coordinates count as outside, in either mode
    table[5, 5] = np.inf
    pad = 4099
    n_out, n_tgt = B * 3 * H * W, B * H * W
    big_out = torch.full((n_out + 2 * pad,), -12345.0, dtype=torch.float32, device=DEV)
    big_tgt = torch.full((n_tgt + 2 * pad,), -987654321, dtype=torch.int64, device=DEV)
    from pytorch_segmentation_amd import ops
    out, tgt = ops.augment_batch(_dev(imgs), _dev(segs), _dev(table),
                                 H, W, MEAN, STD, out=big_out[pad:pad + n_out].view(B, 3, H, W),
                                 target=big_tgt[pad:pad + n_tgt].view(B, H, W))
    torch.cuda.synchronize()
    assert (big_out[:pad] == -12345.0).all() and (big_out[pad + n_out:] == -12345.0).all()
    assert (big_tgt[:pad] == -987654321).all() and (big_tgt[pad + n_tgt:] == -987654321).all()
    out, tgt = out.cpu().numpy(), tgt.cpu().numpy()
    assert (tgt == 0).all()
    fill = _normalise32(np.full((1, 3, 1, 1), CVAL))
    q = _device_q(out)
    if mode == 0:
        assert np.array_equal(out, np.broadcast_to(fill, out.shape))
    else:
        f = imgs.astype(np.float64)
        assert np.array_equal(q[0], np.broadcast_to(f[0][:, :, W - 1:W], q[0].shape))        # each row's last pixel
        assert np.array_equal(q[1], np.broadcast_to(f[1][:, :, 0:1], q[1].shape))
        assert np.array_equal(q[2], np.broadcast_to(f[2][:, H - 1:H, :], q[2].shape))        # each column's last pixel
        assert np.array_equal(q[3], np.broadcast_to(f[3][:, 0:1, 0:1], q[3].shape))          # the corner
        assert np.array_equal(out[4:], np.broadcast_to(fill, out[4:].shape))
    assert np.array_equal(q, _oracle(imgs, segs, table)['q'])


# ------------------------------------------------------------------ 5. end to end
def test_train_with_augment(tmp_path, monkeypatch):
    from pytorch_segmentation_amd.utils import Fetcher
    from pytorch_segmentation_amd.utils.datasets import CocoInstance, make_synthetic_coco
    root = make_synthetic_coco(str(tmp_path / 'data'), n_train=4, n_val=2, n_classes=1)
    monkeypatch.chdir(tmp_path)
    import train as train_mod

    def first_batch(seed):
        ds = CocoInstance(os.path.join(root, 'train.json'), img_size=[64, 64], augments=DeviceAugment.reference(seed=seed))
        fetcher = Fetcher(train_mod._loader(ds, 4, 0, train=False), ds.post_fetch_fn)
        return next(iter(fetcher))

    a, b, c = first_batch(7), first_batch(7), first_batch(8)
    assert a[0].shape == (4, 3, 64, 64) and a[0].dtype == torch.float32 and a[1].shape == (4, 64, 64) and a[1].dtype == torch.int64
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not torch.equal(a[0], c[0])

    losses = {}
    for augment in (False, True):
        torch.manual_seed(0)
        _, losses[augment] = train_mod.train(root, epochs=1, img_size=[64, 64], batch_size=4, accumulate=1, lr=1e-2,
                                             num_workers=0, notest=True, nosave=True, model_name='unet', augment=augment)
    print('loss without / with augmentation:', losses[False], losses[True])
    assert np.isfinite(losses[False]) and np.isfinite(losses[True])
    assert losses[True] != losses[False]
