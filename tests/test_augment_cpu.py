"""Host side of the on-device augmentation (pytorch_segmentation_amd/utils/augment.py): what the sampler draws, how a
recipe becomes a row of the kernel's parameter table, and the wiring into CocoDataset and train.py.  No GPU."""
import inspect
import json
import warnings

import numpy as np
import pytest

from pytorch_segmentation_amd.utils import augment as aug
from pytorch_segmentation_amd.utils.augment import DeviceAugment

H, W = 37, 53


def _inverse(row):
    return np.vstack([row[0:6].astype(np.float64).reshape(2, 3), [0.0, 0.0, 1.0]])


def _forward_point(row, x, y):
    """where the source pixel index (x, y) lands in the output, by the row's (inverse) matrix"""
    p = np.linalg.inv(_inverse(row)) @ np.array([x, y, 1.0])
    return p[0], p[1]


def test_row_layout_matches_the_header():
    import re
    from pytorch_segmentation_amd import _lib, ops
    m = re.search(r'#define\s+PSEG_AUGMENT_ROW\s+(\d+)', open(_lib.HEADER_PATH).read())
    assert int(m.group(1)) == aug.ROW == ops.AUGMENT_ROW
    assert 'pseg_augment_batch' in _lib.parse_header()


@pytest.mark.parametrize('order', [0, 1])
def test_identity_rows_are_exactly_identity(order):
    t = DeviceAugment.identity(order=order, seed=1).sample(6, H, W)
    assert t.shape == (6, aug.ROW) and t.dtype == np.float32
    for row in t:
        assert np.array_equal(row[0:6], np.array([1, 0, 0, 0, 1, 0], dtype=np.float32))
        assert np.array_equal(row[6:18].reshape(3, 4), np.eye(4, dtype=np.float32)[:3])
        assert row[19] == order and row[20] == 0


def test_fliplr_only_row_mirrors_x():
    a = DeviceAugment.identity(seed=0)
    a.fliplr = 1.0
    row = a.sample(1, H, W)[0]
    for x, y in [(0, 0), (W - 1, 0), (17, 30), (W - 1, H - 1)]:
        sx, sy = _inverse(row)[:2] @ np.array([x, y, 1.0])
        assert sx == W - 1 - x and sy == y
    a.fliplr, a.flipud = 0.0, 1.0
    row = a.sample(1, H, W)[0]
    sx, sy = _inverse(row)[:2] @ np.array([5.0, 7.0, 1.0])
    assert sx == 5 and sy == H - 1 - 7


def test_rotation_about_the_centre_fixes_the_centre():
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    for deg in (-90.0, 30.0, 61.5):
        row = DeviceAugment.rows([{'affine': {'rotate': deg}}], H, W)[0]
        sx, sy = _inverse(row)[:2] @ np.array([cx, cy, 1.0])
        assert abs(sx - cx) < 1e-4 and abs(sy - cy) < 1e-4
        # and it is a rotation: a unit step in the output is a unit step in the source
        lin = _inverse(row)[:2, :2]
        assert np.allclose(lin @ lin.T, np.eye(2), atol=1e-6)
    # +90 degrees about the centre of a square image sends the corner (0, 0) to (N-1, 0)
    row = DeviceAugment.rows([{'affine': {'rotate': 90.0}}], 41, 41)[0]
    x, y = _forward_point(row, 0.0, 0.0)
    assert abs(x - 40.0) < 1e-4 and abs(y) < 1e-4


def test_affine_scale_and_translate_map_points():
    row = DeviceAugment.rows([{'affine': {'scale': (1.2, 0.8), 'translate': (0.1, -0.2)}}], H, W)[0]
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    x, y = _forward_point(row, cx + 10.0, cy + 10.0)
    assert abs(x - (cx + 12.0 + 0.1 * W)) < 1e-4 and abs(y - (cy + 8.0 - 0.2 * H)) < 1e-4


def test_crop_and_pad_moves_the_corners_by_the_drawn_fractions():
    a = DeviceAugment.identity(seed=3)
    a.crop_pad, a.crop_pad_p = (-0.05, 0.1), 1.0
    for r in a.draw(8):
        top, right, bottom, left = r['crop_pad']
        assert all(-0.05 <= v <= 0.1 for v in r['crop_pad']) and r['order'] == 1
        row = DeviceAugment.rows([r], H, W)[0]
        # the image's corners in edge coordinates (pixel i covers [i - 0.5, i + 0.5]): padded by the fractions of the image
        # size, then the grown (or cropped) canvas is resized back to W x H
        kx, ky = W / (W * (1 + left + right)), H / (H * (1 + top + bottom))
        x0, y0 = _forward_point(row, -0.5, -0.5)
        x1, y1 = _forward_point(row, W - 0.5, H - 0.5)
        assert abs((x0 + 0.5) - left * W * kx) < 1e-3 and abs((y0 + 0.5) - top * H * ky) < 1e-3
        assert abs((W - 0.5 - x1) - right * W * kx) < 1e-3 and abs((H - 0.5 - y1) - bottom * H * ky) < 1e-3


def test_same_seed_same_table_and_ranks_differ():
    t0 = DeviceAugment.reference(seed=11, rank=0).sample(16, H, W)
    t1 = DeviceAugment.reference(seed=11, rank=0).sample(16, H, W)
    t2 = DeviceAugment.reference(seed=11, rank=1).sample(16, H, W)
    assert np.array_equal(t0, t1)
    assert not np.array_equal(t0, t2)
    a = DeviceAugment.reference(seed=11)                  # no process group: rank 0
    assert np.array_equal(a.sample(16, H, W), t0)
    assert not np.array_equal(a.sample(16, H, W), t0)     # the generator moves on from batch to batch


def test_flip_frequencies():
    n = 4000
    recipes = DeviceAugment.reference(seed=5).draw(n)
    for key, p in (('fliplr', 0.5), ('flipud', 0.2)):
        k = sum(r[key] for r in recipes)
        assert abs(k - n * p) <= 4.0 * np.sqrt(n * p * (1 - p)), (key, k)
    # the other draws stay in their ranges
    for r in recipes:
        assert r['order'] in (0, 1) and r['mode'] in (0, 1) and 0 <= r['cval'] <= 255 and len(r['colour']) <= 5
        if r['affine'] is not None:
            f = r['affine']
            assert all(0.8 <= s <= 1.2 for s in f['scale']) and all(-0.2 <= t <= 0.2 for t in f['translate'])
            assert -90 <= f['rotate'] <= 90 and -16 <= f['shear'] <= 16
    assert 0.4 < np.mean([r['affine'] is not None for r in recipes]) < 0.6
    assert 0.4 < np.mean([r['crop_pad'] is not None for r in recipes]) < 0.6


def _apply_named(name, value, rgb):
    """fp64 restatement of one named operation on an [N, 3] array of 0..255 values"""
    if name == 'add':
        return rgb + np.asarray(value)[None, :]
    if name == 'multiply':
        return rgb * np.asarray(value)[None, :]
    if name == 'contrast':
        return 127.0 + np.asarray(value)[None, :] * (rgb - 127.0)
    if name == 'invert':
        return np.where(np.asarray(value, dtype=bool)[None, :], 255.0 - rgb, rgb)
    if name == 'grayscale':
        gray = rgb @ np.array([0.299, 0.587, 0.114])
        return (1.0 - value) * rgb + value * gray[:, None]
    raise AssertionError(name)


def test_colour_matrices_equal_the_composition_of_their_named_ops():
    v = np.arange(256, dtype=np.float64)
    rgb = np.stack([v, v[::-1], (v * 7) % 256], axis=1)
    a = DeviceAugment.reference(seed=2)
    recipes = a.draw(600)
    seen = set()
    for r in recipes:
        want = rgb
        for name, value in r['colour']:
            seen.add(name)
            want = _apply_named(name, value, want)
        row = DeviceAugment.rows([r], H, W)[0]
        m = row[6:18].astype(np.float64).reshape(3, 4)
        got = rgb @ m[:, :3].T + m[:, 3][None, :]
        # the table is fp32: 2^-24 relative on coefficients of at most a few, times 255, per composed operation
        assert np.abs(got - want).max() < 2e-3, r['colour']
    assert seen == {'add', 'multiply', 'contrast', 'invert', 'grayscale'}
    counts = [len(r['colour']) for r in recipes]
    assert min(counts) == 0 and max(counts) >= 2


def _empty_coco(tmp_path):
    path = tmp_path / 'train.json'
    path.write_text(json.dumps({'categories': [{'name': 'a'}], 'images': [], 'annotations': []}))
    return str(path)


def test_dataset_takes_a_device_augment_silently(tmp_path):
    from pytorch_segmentation_amd.utils import datasets as ds
    path = _empty_coco(tmp_path)
    ds._WARNED.clear()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        a = DeviceAugment.reference()
        d = ds.CocoDataset(path, augments=a)
        assert d.augments is a
        assert ds.CocoInstance(path, augments=a).augments is a
        assert not [x for x in w if issubclass(x.category, RuntimeWarning)]
        d = ds.CocoDataset(path, augments=[object()])
        assert d.augments is None
        assert ds.CocoDataset(path).augments is None
    msgs = [str(x.message) for x in w if issubclass(x.category, RuntimeWarning)]
    assert len(msgs) == 1 and msgs[0].startswith('augments') and 'IGNORED' in msgs[0]
    ds._WARNED.clear()


def test_train_flag_and_signature():
    import train
    ap = train.build_parser()
    assert ap.parse_args(['data/x']).augment is False
    assert ap.parse_args(['data/x', '--augment']).augment is True
    names = list(inspect.signature(train.train).parameters)
    assert names == ['data_dir', 'epochs', 'img_size', 'batch_size', 'accumulate', 'lr', 'adam', 'resume', 'weights',
                     'num_workers', 'multi_scale', 'rect', 'mixed_precision', 'notest', 'nosave', 'model_name', 'augment']
    assert inspect.signature(train.train).parameters['augment'].default is False
