"""Host side of the neighbourhood augmentation (utils/augment.py: filters, noise, dropout; pseg_augment_batch_nbhd's row):
the row layout against the header, the untouched default tables, the filter formulas, what DeviceAugment.full() draws, the
train.py flag, and the fp64 restatement that tests/test_augment_nbhd_gpu.py holds the kernel to, on its own.  No GPU."""
import re
import sys

import numpy as np
import pytest
import scipy.signal
import torch

from pytorch_segmentation_amd.utils import augment as aug
from pytorch_segmentation_amd.utils.augment import DeviceAugment

import test_augment_nbhd_gpu as G
from test_augment_gpu import _batch, _half_distance

GOLDEN = __file__.rsplit('/', 1)[0] + '/golden/augment_tables_abi13.npz'


# ------------------------------------------------------------------ layout
def test_nbhd_row_layout_matches_the_header():
    from pytorch_segmentation_amd import _lib, ops
    src = open(_lib.HEADER_PATH).read()
    d = {k: int(v) for k, v in re.findall(r'#define\s+PSEG_AUGMENT_NBHD_(\w+)\s+(\d+)', src)}
    assert d == {'ROW': aug.NBHD_ROW, 'KMAX': aug.NBHD_KMAX, 'K': aug.NBHD_K, 'NOISE': aug.NBHD_NOISE, 'DROP': aug.NBHD_DROP,
                 'SEED': aug.NBHD_SEED, 'WEIGHTS': aug.NBHD_WEIGHTS}
    assert ops.AUGMENT_NBHD_ROW == aug.NBHD_ROW and ops.AUGMENT_NBHD_KMAX == aug.NBHD_KMAX
    assert aug.NBHD_WEIGHTS + aug.NBHD_KMAX ** 2 <= aug.NBHD_ROW and aug.NBHD_SEED + 2 <= aug.NBHD_WEIGHTS
    assert _lib.abi_version_of_header() == 14
    protos = _lib.parse_header()
    a, b = protos['pseg_augment_batch'][2], protos['pseg_augment_batch_nbhd'][2]
    assert [n for n in b if n != 'shape_host'] == a and b.index('shape_host') == 3


def test_nbhd_row_keeps_the_plain_row_and_the_seed_bits():
    base = aug.make_row(np.array([[0.5, 0.1, 3], [0.2, 1.5, -4.]]), aug.colour_matrix([('add', [1., 2., 3.])]), 9.0, 1, 1)
    kernel = np.arange(25, dtype=np.float64).reshape(5, 5)
    for seed in (0, 1, 2 ** 64 - 1, 0xFFC00001_7FA00001, 0x7F800000_FF800000):       # NaN and infinity patterns as floats
        row = aug.make_nbhd_row(base, kernel, (3.5, True), (0.25, False, 4, 7), seed)
        assert row.dtype == np.float32 and row.shape == (aug.NBHD_ROW,)
        assert row[:aug.ROW].tobytes() == base.tobytes()
        assert row[aug.NBHD_K] == 5 and np.array_equal(row[aug.NBHD_WEIGHTS:aug.NBHD_WEIGHTS + 25], np.arange(25, dtype=np.float32))
        assert list(row[aug.NBHD_NOISE:aug.NBHD_NOISE + 2]) == [3.5, 1.0] and list(row[aug.NBHD_DROP:aug.NBHD_DROP + 4]) == [0.25, 0, 4, 7]
        # the bits survive the way DeviceAugment.apply takes a table to the device
        t = torch.from_numpy(np.ascontiguousarray(np.stack([row, row]), dtype=np.float32)).clone().numpy()
        assert G.row_seed(t[1]) == seed
    assert np.array_equal(aug.row_shapes(np.stack([row])), np.array([[5, 4, 7]], dtype=np.int32))
    for bad in (np.ones((4, 4)), np.ones((15, 15)), np.ones((3, 5))):
        with pytest.raises(ValueError):
            aug.make_nbhd_row(base, bad)


def test_default_tables_are_those_of_the_previous_sampler():
    """DeviceAugment() and .reference() draw, byte for byte, the tables captured before the neighbourhood augmenters
    existed (tests/golden/augment_tables_abi13.npz: 16 rows at 37 x 83, then 5 at 70 x 131, seeds 0..3)"""
    golden = np.load(GOLDEN)
    for seed in range(4):
        for name, make in (('default', DeviceAugment), ('reference', DeviceAugment.reference)):
            a = make(seed=seed, rank=0)
            got = np.concatenate([a.sample(16, 37, 83), a.sample(5, 70, 131)])
            want = golden['%s_seed%d' % (name, seed)]
            assert got.dtype == want.dtype and got.shape == want.shape == (21, aug.ROW) and got.tobytes() == want.tobytes()


# ------------------------------------------------------------------ filters
def test_gaussian_kernel():
    for sigma, k in ((0.4, 5), (1.5, 5), (1.7, 5), (1.9, 7), (2.5, 9), (2.99, 9), (0.001, 5)):
        g = aug.gaussian_kernel(sigma)
        assert g.shape == (k, k) and k == (lambda v: v + 1 - v % 2)(int(max(3.3 * sigma, 5)))
        d = np.arange(k) - k // 2
        one = np.exp(-d.astype(np.float64) ** 2 / (2 * sigma ** 2))
        assert np.allclose(g, np.outer(one, one) / np.outer(one, one).sum(), rtol=1e-13, atol=0)
        assert abs(g.sum() - 1) < 1e-14 and np.array_equal(g, g.T) and np.array_equal(g, g[::-1, ::-1])
    assert aug.gaussian_kernel(0.0009) is None and aug.gaussian_kernel(0.0) is None


def test_average_kernel_window():
    for k in range(2, 8):
        m = aug.average_kernel(k)
        K = m.shape[0]
        assert K % 2 == 1 and K in (k, k + 1) and abs(m.sum() - 1) < 1e-14
        # tap (j, i) reads offset (j - K//2, i - K//2): the window is [-(k//2), -(k//2) + k - 1] on both axes
        offsets = np.nonzero(m[K // 2])[0] - K // 2
        assert list(offsets) == list(range(-(k // 2), -(k // 2) + k))
        assert np.array_equal(m != 0, np.outer(m[K // 2] != 0, m[K // 2] != 0)) and set(np.unique(m)) <= {0.0, 1.0 / (k * k)}


def test_sharpen_and_emboss_kernels():
    for a, l in ((0.0, 1.0), (1.0, 1.5), (1.0, 0.75), (0.3, 1.2)):
        m = aug.sharpen_kernel(a, l)
        want = (1 - a) * np.array([[0, 0, 0], [0, 1., 0], [0, 0, 0]]) + a * np.array([[-1, -1, -1], [-1, 8 + l, -1], [-1, -1, -1]])
        assert np.allclose(m, want, rtol=0, atol=1e-15) and abs(m.sum() - (1 - a + a * l)) < 1e-14
    for a, s in ((0.0, 1.0), (1.0, 2.0), (1.0, 0.0), (0.6, 0.7)):
        m = aug.emboss_kernel(a, s)
        want = (1 - a) * np.array([[0, 0, 0], [0, 1., 0], [0, 0, 0]]) + a * np.array([[-1 - s, -s, 0], [-s, 1, s], [0, s, 1 + s]])
        assert np.allclose(m, want, rtol=0, atol=1e-15) and abs(m.sum() - 1) < 1e-14


def test_composed_filter_is_the_full_convolution_of_its_parts():
    parts = [aug.gaussian_kernel(2.99), aug.sharpen_kernel(0.6, 1.2), aug.emboss_kernel(0.7, 1.4), aug.average_kernel(2)]
    for picked in ([0], [1, 2], [0, 1, 2], [2, 0, 1], [3, 2], [3, 1, 2]):
        want = np.ones((1, 1))
        for i in picked:
            want = scipy.signal.convolve2d(want, parts[i], mode='full')
        got = aug.compose_filters([parts[i] for i in picked])
        assert got.shape == want.shape and np.abs(got - want).max() < 1e-13
    assert aug.compose_filters(parts[:3]).shape == (13, 13)
    # and it stands for applying the correlations one after the other (away from the border)
    rng = np.random.default_rng(0)
    x = rng.uniform(0, 255, (1, 40, 40))
    one = G.correlate(G.correlate(x, parts[3]), parts[2])
    both = G.correlate(x, aug.compose_filters([parts[3], parts[2]]))
    assert np.abs(one - both)[:, 4:-4, 4:-4].max() < 1e-9 and np.abs(parts[2] - parts[2][::-1, ::-1]).max() > 0     # (a filter that tells correlation from convolution)


# ------------------------------------------------------------------ what full() draws
def _within(k, n, p):
    return abs(k - n * p) <= 4.0 * np.sqrt(n * p * (1 - p))


def test_full_draws_ranges_and_frequencies():
    n, H, W = 20000, 512, 384
    a = DeviceAugment.full(seed=9)
    recipes = a.draw(n)
    slot = 2.5 / aug.COLOUR_SLOTS                              # SomeOf((0, 5)) of 16: a slot is picked 2.5 / 16 of the time
    names = [[f[0] for f in r.get('filters', ())] for r in recipes]
    count = {k: sum(k in f for f in names) for k in ('gaussian', 'average', 'sharpen', 'emboss')}
    assert _within(count['gaussian'], n, slot / 3 * (1 - 0.001 / 3)) and _within(count['average'], n, slot / 3)
    assert _within(count['sharpen'], n, slot) and _within(count['emboss'], n, slot)
    assert all(len(f) == len(set(f)) and len(set(f) & {'gaussian', 'average'}) <= 1 for f in names)
    noise = [r['noise'] for r in recipes if 'noise' in r]
    assert _within(len(noise), n, slot) and _within(sum(pc for _, pc in noise), len(noise), 0.5)
    assert all(0 <= s <= 12.75 for s, _ in noise) and max(s for s, _ in noise) > 12 and min(s for s, _ in noise) < 0.75
    drops = [r['dropout'] for r in recipes if 'dropout' in r]
    fine, coarse = [d for d in drops if d['size'] is None], [d for d in drops if d['size'] is not None]
    assert _within(len(fine), n, slot / 2) and _within(len(coarse), n, slot / 2)
    assert _within(sum(d['per_channel'] for d in fine), len(fine), 0.5) and _within(sum(d['per_channel'] for d in coarse), len(coarse), 0.2)
    assert all(0.01 <= d['p'] <= 0.1 for d in fine) and all(0.03 <= d['p'] <= 0.15 and 0.02 <= d['size'] <= 0.05 for d in coarse)
    for r in recipes:
        for f in r.get('filters', ()):
            if f[0] == 'gaussian':
                assert 0.001 <= f[1] < 3.0
            elif f[0] == 'average':
                assert f[1] in range(2, 8)
            elif f[0] == 'sharpen':
                assert 0 <= f[1] <= 1 and 0.75 <= f[2] <= 1.5
            else:
                assert 0 <= f[1] <= 1 and 0 <= f[2] <= 2
        assert ('seed' in r) == ('noise' in r or 'dropout' in r)
    seeds = [r['seed'] for r in recipes if 'seed' in r]
    assert len(set(seeds)) == len(seeds) and max(seeds) >= 2 ** 63 and all(0 <= s < 2 ** 64 for s in seeds)
    assert _within(sum(k == 2 for k in (f[1] for r in recipes for f in r.get('filters', ()) if f[0] == 'average')), count['average'], 1 / 6)

    # the rows: K, scale, p and the mask sizes as the kernel gets them
    wide = [r for r in recipes if r.get('filters') or 'noise' in r or 'dropout' in r]
    table = DeviceAugment.rows(wide, H, W)
    assert table.shape == (len(wide), aug.NBHD_ROW)
    shapes = aug.row_shapes(table)
    K, seen = shapes[:, 0], set(shapes[:, 0])
    assert seen == {0, 3, 5, 7, 9, 11, 13} and ((K == 0) == np.array([not r.get('filters') for r in wide])).all()
    for r, row, (k, mh, mw) in zip(wide, table, shapes):
        w = row[aug.NBHD_WEIGHTS:aug.NBHD_WEIGHTS + k * k]
        assert not row[aug.NBHD_WEIGHTS + k * k:].any()
        if k:
            lift = np.prod([1 - f[1] + f[1] * f[2] for f in r['filters'] if f[0] == 'sharpen'])
            assert abs(w.astype(np.float64).sum() - lift) < 1e-5
        assert row[aug.NBHD_NOISE] == np.float32(r['noise'][0] if 'noise' in r else 0)
        d = r.get('dropout')
        assert row[aug.NBHD_DROP] == np.float32(d['p'] if d else 0)
        if d and d['size'] is not None:
            assert (mh, mw) == (max(4, int(H * d['size'])), max(4, int(W * d['size']))) and 10 <= mh <= 25 and 7 <= mw <= 19
        else:
            assert (mh, mw) == (0, 0)
        assert G.row_seed(row) == r.get('seed', 0)
    # a batch in which nothing of the kind was drawn keeps the plain rows, and so the plain kernel
    plain = [r for r in recipes if not (r.get('filters') or 'noise' in r or 'dropout' in r)][:8]
    assert DeviceAugment.rows(plain, H, W).shape == (8, aug.ROW)
    assert DeviceAugment.rows(plain + wide[:1], H, W).shape == (9, aug.NBHD_ROW)
    assert np.array_equal(DeviceAugment.rows(plain + wide[:1], H, W)[:8, :aug.ROW], DeviceAugment.rows(plain, H, W))


def test_full_is_reference_plus_the_seven_and_all_are_off_by_default():
    off = ('gaussian_blur', 'average_blur', 'sharpen_alpha', 'emboss_alpha', 'noise_scale', 'dropout_p', 'coarse_p')
    ref, full = DeviceAugment.reference(seed=1), DeviceAugment.full(seed=1)
    assert all(getattr(ref, k) is None for k in off) and all(getattr(full, k) is not None for k in off)
    assert {k: v for k, v in vars(ref).items() if k not in off} == {k: v for k, v in vars(full).items() if k not in off}
    assert full.noise_scale == (0.0, 12.75) and full.gaussian_blur == (0.0, 3.0) and full.average_blur == (2.0, 7.0)
    assert DeviceAugment.full(noise_scale=None, seed=1).noise_scale is None
    assert all(r.keys() == {'fliplr', 'flipud', 'crop_pad', 'affine', 'order', 'cval', 'mode', 'colour'} for r in ref.draw(500))


def test_augment_full_flag_reaches_train(monkeypatch):
    import train
    ap = train.build_parser()
    assert ap.parse_args(['data/x']).augment_full is False and ap.parse_args(['data/x', '--augment-full']).augment_full is True
    seen = {}

    def fake_train(*args, **kw):
        seen['args'] = args

    monkeypatch.setattr(train, 'train', fake_train)
    monkeypatch.setattr(train.torch.cuda, 'set_device', lambda i: None)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    for argv, check in ((['--augment-full'], lambda a: isinstance(a, DeviceAugment) and a.noise_scale == (0.0, 12.75)),
                        (['--augment', '--augment-full'], lambda a: isinstance(a, DeviceAugment) and a.coarse_p == (0.03, 0.15)),
                        (['--augment'], lambda a: a is True), ([], lambda a: a is False)):
        monkeypatch.setattr(sys, 'argv', ['train.py', 'data/x'] + argv)
        train.main()
        assert check(seen['args'][-1]), argv


# ------------------------------------------------------------------ the restatement on its own
def test_philox_known_answers():
    """Random123's known-answer vectors for philox4x32-10 whose counter words 2 and 3 are zero, as this kernel's are"""
    got = G.philox4x32_10(np.array([0]), 0, 0)
    assert [int(v[0]) for v in got] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    a = G.philox4x32_10(np.arange(4), 1, 5)
    assert len({tuple(int(v[i]) for v in a) for i in range(4)}) == 4 and all(int(v.max()) < 2 ** 32 for v in a)
    assert [int(v[1]) for v in a] != [int(v[1]) for v in G.philox4x32_10(np.arange(4), 2, 5)]
    assert [int(v[1]) for v in a] != [int(v[1]) for v in G.philox4x32_10(np.arange(4), 1, 5 + 2 ** 32)]


def test_reflect_and_multi_scale_index():
    assert list(G.reflect101(np.arange(-3, 8), 5)) == [3, 2, 1, 0, 1, 2, 3, 4, 3, 2, 1]
    assert list(G.reflect101(np.arange(-6, 9), 3)) == [2, 1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1, 0]
    assert list(G.reflect101(np.arange(-2, 3), 1)) == [0] * 5
    x = np.arange(12, dtype=np.float64).reshape(1, 3, 4)
    assert np.array_equal(G.correlate(x, np.pad([[1.]], 1)), x)
    want = np.pad(x, ((0, 0), (1, 1), (1, 1)), mode='reflect')
    w = np.arange(9, dtype=np.float64).reshape(3, 3)
    assert np.array_equal(G.correlate(x, w), sum(w[j, i] * want[:, j:j + 3, i:i + 4] for j in range(3) for i in range(3)))
    import torch.nn.functional as F
    for n_in, n_out in ((70, 32), (131, 64), (70, 96), (131, 160), (37, 37)):
        t = F.interpolate(torch.arange(n_in, dtype=torch.float32).view(1, 1, 1, n_in), (1, n_out)).view(-1).numpy()
        assert np.array_equal(G.ms_index(n_out, n_in), t.astype(np.int64))


@pytest.mark.parametrize('H,W', G.GRIDS)
def test_restatement_stays_inside_the_caps(H, W):
    """what the GPU tests rely on: on the photos they use, few pixels of the restatement lie within delta of a half-integer
    (2 %; 5 % for the average of 6 x 6), and for the dyadic filters every exact tie is compared, none excluded"""
    imgs, segs = _batch(G.B, H, W)
    for name in sorted(G.FILTERS):
        for warped in (False, True):
            rows = G.nbhd_table(G.base_rows(H, W, warped), G.filter_of(name))
            r = G.restate(imgs, segs, rows)
            exact = G.is_dyadic(rows[0, aug.NBHD_WEIGHTS:])
            shares = [1.0 - G.filter_ok(r, b, exact).mean() for b in range(G.B)]
            print('%s %dx%d warped=%d: delta %.3g, excluded' % (name, H, W, warped, r['delta'][0]), ['%.4f' % s for s in shares])
            assert max(shares) <= G.excluded_cap(name)
            if exact:
                assert max(shares) == 0.0 and (_half_distance(r['filt']) == 0).any() == (not name.startswith('emboss'))
    # noise at scale 10 on a flat image: about 2 * delta of the pixels
    flat = G.flat(H, W)
    r = G.restate(*flat, G.nbhd_table(G.base_rows(H, W, False), noise=(10.0, True)))
    share = (_half_distance(r['noise']) <= 1e-3).mean()
    print('noise %dx%d: excluded %.4f' % (H, W, share))
    assert share <= 0.01
    n = r['noise'] - 128.0
    assert abs(n.mean()) < 5 * 10 / np.sqrt(n.size) and abs(n.std() - 10) < 5 * 10 / np.sqrt(2 * n.size)
