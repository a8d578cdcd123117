"""Host side of the blend augmentation (utils/augment.py: median blur, edge-detect blend, hue / saturation, frequency-noise
blend; pseg_augment_batch_blend's row): the row layout against the header, the untouched tables of the existing
constructors, what DeviceAugment.blends() draws and at which rates, the composed second filter, the mask tables, rows()'
refusals, the dispatch by row width, the train.py flag, and the fp64 restatement that tests/test_augment_blend_gpu.py holds
the kernel to, on its own: the share of pixels each of its comparisons excludes.  No GPU."""
import re
import sys

import numpy as np
import pytest
import torch

from pytorch_segmentation_amd.utils import augment as aug
from pytorch_segmentation_amd.utils.augment import DeviceAugment

import augment_blend_ref as R
import test_augment_nbhd_gpu as G
from test_augment_gpu import _batch, _half_distance, _round8

GOLDEN = __file__.rsplit('/', 1)[0] + '/golden/augment_tables_abi13.npz'
NEW = ('median_blur', 'edge_blend', 'hue_sat', 'frequency_blend')
OFF = dict(median_blur=None, edge_blend=None, hue_sat=None, frequency_blend=False)


# ------------------------------------------------------------------ layout
def test_blend_row_layout_matches_the_header():
    from pytorch_segmentation_amd import _lib, ops
    src = open(_lib.HEADER_PATH).read()
    d = {k: int(v) for k, v in re.findall(r'#define\s+PSEG_AUGMENT_BLEND_(\w+)\s+(\d+)', src)}
    assert d == {'ROW': aug.BLEND_ROW, 'KMEDMAX': aug.BLEND_KMEDMAX, 'K2MAX': aug.BLEND_K2MAX, 'KMED': aug.BLEND_KMED, 'K2': aug.BLEND_K2,
                 'COLOUR_ON': aug.BLEND_COLOUR_ON, 'HUE': aug.BLEND_HUE, 'MB': aug.BLEND_MB, 'WEIGHTS2': aug.BLEND_WEIGHTS2,
                 'T1': aug.BLEND_T1, 'T2': aug.BLEND_T2, 'TABLE': aug.BLEND_TABLE}
    assert ops.AUGMENT_BLEND_ROW == aug.BLEND_ROW and ops.AUGMENT_BLEND_KMEDMAX == 11 and ops.AUGMENT_BLEND_K2MAX == 15
    assert aug.BLEND_KMED == aug.WARP_ROW and aug.BLEND_HUE + 2 <= aug.BLEND_MB and aug.BLEND_MB + 12 <= aug.BLEND_WEIGHTS2
    assert aug.BLEND_WEIGHTS2 + aug.BLEND_K2MAX ** 2 <= aug.BLEND_T1 and aug.BLEND_T1 + 256 == aug.BLEND_T2
    assert aug.BLEND_T2 + 256 == aug.BLEND_ROW
    assert _lib.abi_version_of_header() == 14                     # additive: the version does not move
    protos = _lib.parse_header()
    assert protos['pseg_augment_batch_blend'][1:] == protos['pseg_augment_batch_warp'][1:]
    assert 'pseg_augment_batch_blend' in _lib.prototypes()


def test_blend_row_keeps_the_warp_row_and_refuses_what_is_out_of_range():
    nb = aug.make_nbhd_row(aug.make_row(np.array([[0.5, 0.1, 3], [0.2, 1.5, -4.]]), None, 9.0, 1, 1), np.arange(9.).reshape(3, 3),
                           (3.5, True), (0.25, False, 4, 7), 0xFFC00001_7FA00001)
    wr = aug.make_warp_row(nb, (1e-3, -2e-3, 1.0), 2.5, np.arange(32.).reshape(4, 4, 2))
    t1, t2 = R.random_table(1), R.random_table(2)
    row = aug.make_blend_row(wr, 7, np.arange(25.).reshape(5, 5), R.MB, t1, t2, (0.5, -0.25))
    assert row.dtype == np.float32 and row.shape == (aug.BLEND_ROW,) and row[:aug.WARP_ROW].tobytes() == wr.tobytes()
    assert G.row_seed(row) == 0xFFC00001_7FA00001
    assert row[aug.BLEND_KMED] == 7 and row[aug.BLEND_K2] == 5 and row[aug.BLEND_COLOUR_ON] == 1
    assert list(row[aug.BLEND_HUE:aug.BLEND_HUE + 2]) == [0.5, -0.25] and not row[aug.BLEND_HUE + 2:aug.BLEND_MB].any()
    assert np.array_equal(row[aug.BLEND_MB:aug.BLEND_MB + 12], R.MB.astype(np.float32).reshape(-1))
    assert np.array_equal(row[aug.BLEND_WEIGHTS2:aug.BLEND_WEIGHTS2 + 25], np.arange(25, dtype=np.float32))
    assert np.array_equal(row[aug.BLEND_T1:aug.BLEND_T2].reshape(16, 16), t1) and np.array_equal(row[aug.BLEND_T2:].reshape(16, 16), t2)
    assert np.array_equal(aug.row_shapes(np.stack([row])), np.array([[3, 4, 7, 7, 5]], dtype=np.int32))
    assert aug.row_shapes(np.stack([wr])).shape == (1, 3) and aug.row_shapes(np.stack([nb])).shape == (1, 3)
    off = aug.make_blend_row()
    assert off[:aug.WARP_ROW].tobytes() == aug.make_warp_row().tobytes() and not off[aug.BLEND_KMED:aug.BLEND_MB].any()
    assert np.array_equal(off[aug.BLEND_MB:aug.BLEND_MB + 12], np.eye(4, dtype=np.float32)[:3].reshape(-1)) and not off[aug.BLEND_WEIGHTS2:].any()
    for kw in (dict(kmed=4), dict(kmed=13), dict(kmed=1), dict(kmed=-3), dict(kernel2=np.ones((4, 4))), dict(kernel2=np.ones((17, 17))),
               dict(kernel2=np.ones((1, 1))), dict(kernel2=np.ones((3, 5))), dict(t1=np.full((16, 16), 1.5)), dict(t2=np.full((16, 16), -0.1)),
               dict(t1=np.full((16, 16), np.nan)), dict(t2=np.zeros((8, 8))), dict(hue_sat=(np.inf, 0.0)), dict(hue_sat=(0.0, np.nan))):
        with pytest.raises(ValueError):
            aug.make_blend_row(wr, **kw)


# ------------------------------------------------------------------ the existing constructors draw what they drew
def test_existing_constructors_tables_are_unchanged():
    golden = np.load(GOLDEN)
    for seed in range(4):
        for name, make in (('default', DeviceAugment), ('reference', DeviceAugment.reference)):
            a = make(seed=seed, rank=0)
            got = np.concatenate([a.sample(16, 37, 83), a.sample(5, 70, 131)])
            assert got.tobytes() == golden['%s_seed%d' % (name, seed)].tobytes()
    ref, full, warps, blends = (make(seed=1) for make in (DeviceAugment.reference, DeviceAugment.full, DeviceAugment.warps, DeviceAugment.blends))
    for a in (ref, full, warps):
        assert all(not getattr(a, k) for k in NEW)
    assert (blends.median_blur, blends.edge_blend, blends.hue_sat, blends.frequency_blend) == ((3.0, 11.0), (0.5, 1.0), (-20.0, 20.0), True)
    assert {k: v for k, v in vars(warps).items() if k not in NEW} == {k: v for k, v in vars(blends).items() if k not in NEW}
    # full() and warps(): no recipe holds a new key, and a blends() sampler with the four off consumes the generator identically
    no_warps = dict(elastic_alpha=None, piecewise_scale=None, perspective_scale=None)
    for make, more in ((DeviceAugment.full, no_warps), (DeviceAugment.warps, {})):
        old, dead = make(seed=3, rank=0), DeviceAugment.blends(seed=3, rank=0, **dict(OFF, **more))
        a, b = old.draw(400), dead.draw(400)
        assert not any(k in r for r in a for k in aug._BLEND_KEYS + ('edge_mask',)) and not any(n == 'blend' for r in a for n, _ in r['colour'])
        ta, tb = DeviceAugment.rows(a, 37, 83), DeviceAugment.rows(b, 37, 83)
        assert ta.shape[1] in (aug.NBHD_ROW, aug.WARP_ROW) and ta.view(np.uint32).tobytes() == tb.view(np.uint32).tobytes()
        assert old.rng.random() == dead.rng.random()


# ------------------------------------------------------------------ what blends() draws
def _within(k, n, p):
    return abs(k - n * p) <= 4.0 * np.sqrt(n * p * (1 - p))


def test_blends_draws_rates_ranges_and_row_widths():
    n, H, W = 20000, 96, 64
    recipes = DeviceAugment.blends(seed=9).draw(n)
    slot = 2.5 / aug.COLOUR_SLOTS
    blended = [any(name == 'blend' for name, _ in r['colour']) for r in recipes]
    assert _within(sum('edge' in r for r in recipes), n, slot) and _within(sum('hue_sat' in r for r in recipes), n, slot)
    assert _within(sum('median' in r for r in recipes), n, slot / 3) and _within(sum(blended), n, slot / 2)
    assert _within(sum(any(name == 'multiply' for name, _ in r['colour']) for r in recipes), n, slot / 2)
    ks = [r['median'] for r in recipes if 'median' in r]
    assert set(ks) == {3, 5, 7, 9, 11} and abs(ks.count(3) / len(ks) - 1 / 9) < 0.04 and abs(ks.count(11) / len(ks) - 2 / 9) < 0.05
    assert not any('median' in r and any(f[0] in ('gaussian', 'average') for f in r.get('filters', ())) for r in recipes)
    assert any('median' in r and r.get('filters') for r in recipes)       # a sharpen / emboss still composes into F
    edges = [r['edge'] for r in recipes if 'edge' in r]
    assert all(0.5 <= e['alpha'] <= 1.0 and (e['direction'] is None or 0.0 <= e['direction'] < 1.0) for e in edges)
    assert _within(sum(e['direction'] is None for e in edges), len(edges), 0.5)
    vs = [r['hue_sat'] for r in recipes if 'hue_sat' in r]
    assert min(vs) == -20 and max(vs) == 20 and all(isinstance(v, int) for v in vs)
    for r in recipes:
        assert ('edge' in r) == ('edge_mask' in r) and ('colour_mask' in r) == any(name == 'blend' for name, _ in r['colour'])
        for k in ('edge_mask', 'colour_mask'):
            if k in r:
                t = r[k]
                assert t.dtype == np.float32 and t.shape == (16, 16) and np.isfinite(t).all() and t.min() >= 0 and t.max() <= 1
                assert t.max() - t.min() > 0.5                   # normalised: the mask does blend
    # reproducible by seed, and the tables differ between samples
    again = DeviceAugment.blends(seed=9).draw(300)
    masks = [r['edge_mask'] for r in again if 'edge_mask' in r]
    assert all(np.array_equal(a, b['edge_mask']) for a, b in zip(masks, (r for r in recipes[:300] if 'edge_mask' in r)))
    assert len(masks) > 20 and not np.array_equal(masks[0], masks[1])
    assert DeviceAugment.rows(again, H, W).tobytes() == DeviceAugment.rows(recipes[:300], H, W).tobytes()

    # rows: width by content, fields by recipe
    is_blend = [any(k in r for k in aug._BLEND_KEYS) for r in recipes]
    some = [r for r, w in zip(recipes, is_blend) if w][:200]
    none = [r for r, w in zip(recipes, is_blend) if not w][:16]
    assert DeviceAugment.rows(none, H, W).shape[1] == aug.WARP_ROW and DeviceAugment.rows(none + some[:1], H, W).shape == (17, aug.BLEND_ROW)
    table = DeviceAugment.rows(none + some[:1], H, W)
    assert table[:16, :aug.WARP_ROW].view(np.uint32).tobytes() == DeviceAugment.rows(none, H, W).view(np.uint32).tobytes()
    assert np.array_equal(table[:16, aug.WARP_ROW:], np.tile(aug.make_blend_row()[aug.WARP_ROW:], (16, 1)))
    shapes = aug.row_shapes(DeviceAugment.rows(some, H, W))
    assert shapes.shape == (len(some), 5) and shapes[:, 0].max() <= aug.NBHD_KMAX and shapes[:, 4].max() <= aug.BLEND_K2MAX
    for r, row, sh in zip(some, DeviceAugment.rows(some, H, W), shapes):
        assert sh[3] == r.get('median', 0) and (sh[4] > 0) == ('edge' in r) and (sh[4] == 0 or sh[4] == max(sh[0], 1) + 2)
        want = aug.hue_sat_shift(r['hue_sat']) if 'hue_sat' in r else (0.0, 0.0)
        assert list(row[aug.BLEND_HUE:aug.BLEND_HUE + 2]) == [np.float32(want[0]), np.float32(want[1])]
        assert (row[aug.BLEND_COLOUR_ON] == 1) == ('colour_mask' in r)
        if 'colour_mask' in r:                                    # (M, Mb): the two branches in the blend's place, the other ops around
            mul, con = next(v for name, v in r['colour'] if name == 'blend')
            assert mul.shape == (3,) and 0.5 <= mul.min() and mul.max() <= 1.5 and 0.5 <= con <= 2.0
            for at, op in ((6, ('multiply', mul)), (aug.BLEND_MB, ('contrast', np.full(3, con)))):
                ops_ = [op if name == 'blend' else (name, v) for name, v in r['colour']]
                assert np.array_equal(row[at:at + 12], aug.colour_matrix(ops_).astype(np.float32).reshape(-1))
            assert np.array_equal(row[aug.BLEND_T2:].reshape(16, 16), r['colour_mask'])
    assert aug.hue_sat_shift(20) == (6 * 20 / 255, 20 / 255)
    # the first batch of the end-to-end GPU test holds a blend
    import test_augment_blend_gpu as Bg
    first = DeviceAugment.blends(seed=0, rank=0).sample(Bg.TRAIN_SET['batch_size'], 64, 64)
    assert first.shape == (Bg.TRAIN_SET['batch_size'], aug.BLEND_ROW)


def test_rows_refuses_hand_made_recipes_outside_the_ranges():
    base = {'fliplr': False, 'flipud': False, 'crop_pad': None, 'affine': None, 'order': 0, 'cval': 0.0, 'mode': 0, 'colour': []}
    ok = np.full((16, 16), 0.5, dtype=np.float32)
    assert DeviceAugment.rows([dict(base, median=11)], 8, 8).shape == (1, aug.BLEND_ROW)
    for bad in (dict(median=4), dict(median=13), dict(median=2), dict(edge={'alpha': 0.5, 'direction': None}, edge_mask=ok * 3),
                dict(edge={'alpha': 0.5, 'direction': None}, edge_mask=np.full((16, 16), np.nan)),
                dict(edge={'alpha': 0.5, 'direction': None}, edge_mask=np.zeros((4, 4))),
                dict(colour=[('blend', (np.ones(3), 1.0))], colour_mask=-ok), dict(hue_sat=float('inf'))):
        with pytest.raises(ValueError):
            DeviceAugment.rows([dict(base, **bad)], 8, 8)
    # K2 <= 15 by construction: the widest F (K = 13) under an edge filter
    r = dict(base, filters=[('gaussian', 2.99), ('sharpen', 0.5, 1.0), ('emboss', 0.5, 1.0)], edge={'alpha': 0.7, 'direction': 0.2}, edge_mask=ok)
    assert aug.row_shapes(DeviceAugment.rows([r], 8, 8)).tolist() == [[13, 0, 0, 0, 15]]


# ------------------------------------------------------------------ the second filter
def test_composed_edge_filter_is_the_edge_filter_after_f():
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (1, 40, 40)).astype(np.float64)
    for direction in (None, 0.0, 0.3, 0.875):
        E = aug.edge_kernel(0.7, direction)
        assert E.shape == (3, 3) and abs(E.sum() - 0.3) < 1e-12          # the edge part sums to 0
        if direction is not None:
            assert abs((E - 0.3 * np.eye(3)[1][:, None] * np.eye(3)[1][None]).sum()) < 1e-12 and E[1, 1] == 1.0
        for F in (G.filter_of('gaussian 1.7'), G.filter_of('composed 13'), aug.emboss_kernel(0.6, 1.3)):
            G2 = aug.compose_filters([F, E])
            assert G2.shape[0] == F.shape[0] + 2
            two = G.correlate(G.correlate(img, F), E)                      # F, then E, no rounding in between
            one = G.correlate(img, G2)
            m = G2.shape[0]                                                # interior: the border handling of each on its own differs
            assert np.abs(one - two)[:, m:-m, m:-m].max() < 1e-9
    # the directed kernel: direction 0 looks up, a quarter turn looks right; the neighbours' weights sum to -1
    up, right = aug.directed_edge_kernel(1.0, 0.0), aug.directed_edge_kernel(1.0, 0.25)
    assert up[0, 1] < up[0, 0] < 0 and np.allclose(up[1:, [0, 2]], 0, atol=1e-12) and abs(up[2, 1]) < 1e-12
    assert np.allclose(right, np.rot90(up, -1), atol=1e-12) and abs(up.sum()) < 1e-12
    assert aug.edge_kernel(1.0).tolist() == [[0, 1, 0], [1, -4, 1], [0, 1, 0]]


def test_mask_tables_and_their_sampler():
    for seed in range(20):
        for make in (aug.value_noise_table, aug.frequency_noise_table):
            t = make(np.random.default_rng(seed))
            assert t.dtype == np.float32 and t.shape == (16, 16) and np.isfinite(t).all() and 0 <= t.min() and t.max() <= 1
            assert np.array_equal(t, make(np.random.default_rng(seed)))
    # resize: constant grids stay constant, the nearest one repeats cells, the linear one interpolates between the same centres
    g = np.arange(16.).reshape(4, 4)
    near, lin = aug.resize_to_table(g, False), aug.resize_to_table(g, True)
    assert np.array_equal(near, np.kron(g, np.ones((4, 4)))) and lin.min() == 0 and lin.max() == 15 and len(np.unique(lin)) > 16
    assert np.array_equal(aug.resize_to_table(np.full((2, 2), 3.0), True), np.full((16, 16), 3.0))
    assert np.array_equal(aug.resize_to_table(g[:2, :2].repeat(8, 0).repeat(8, 1), True), g[:2, :2].repeat(8, 0).repeat(8, 1))
    # the sampler: at 16 x 16 it is the table itself; constant tables give constants; NaN counts as 0, values are clamped
    t = R.random_table(0)
    assert np.array_equal(R.mask_sample(t, 16, 16), t.astype(np.float64))
    assert (R.mask_sample(np.ones((16, 16)), 37, 83) == 1).all() and (R.mask_sample(np.full((16, 16), np.nan), 5, 1) == 0).all()
    assert (R.mask_sample(np.full((16, 16), 7.0), 5, 7) == 1).all() and (R.mask_sample(np.full((16, 16), -7.0), 5, 7) == 0).all()
    m = R.mask_sample(t, 70, 131)
    assert m.shape == (70, 131) and m.min() >= t.min() and m.max() <= t.max() and m[0, 0] == t[0, 0] and m[-1, -1] == t[-1, -1]


# ------------------------------------------------------------------ dispatch and flag
def test_apply_dispatches_blend_rows_to_the_blend_kernel(monkeypatch):
    from pytorch_segmentation_amd import ops
    calls = []
    for name in ('augment_batch', 'augment_batch_nbhd', 'augment_batch_warp', 'augment_batch_blend'):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **kw: calls.append((_n, a[2].shape[1], None if _n == 'augment_batch' else tuple(a[3].shape))) or (None, None))
    monkeypatch.setattr(torch.Tensor, 'pin_memory', lambda self: self)
    a = DeviceAugment.identity()
    imgs, segs = torch.zeros(2, 3, 8, 8, dtype=torch.uint8), torch.zeros(2, 8, 8, dtype=torch.uint8)
    wr = np.stack([aug.make_warp_row()] * 2)
    for table in (np.stack([aug.make_row()] * 2), wr[:, :aug.NBHD_ROW].copy(), wr, R.blend_table(wr, kmed=3)):
        a.apply(imgs, segs, table)
    assert calls == [('augment_batch', aug.ROW, None), ('augment_batch_nbhd', aug.NBHD_ROW, (2, 3)), ('augment_batch_warp', aug.WARP_ROW, (2, 3)),
                     ('augment_batch_blend', aug.BLEND_ROW, (2, 5))]


def test_augment_blends_flag_reaches_train(monkeypatch):
    import train
    ap = train.build_parser()
    assert ap.parse_args(['data/x']).augment_blends is False and ap.parse_args(['data/x', '--augment-blends']).augment_blends is True
    seen = {}
    monkeypatch.setattr(train, 'train', lambda *args, **kw: seen.update(args=args))
    monkeypatch.setattr(train.torch.cuda, 'set_device', lambda i: None)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    for argv, check in ((['--augment-blends'], lambda a: isinstance(a, DeviceAugment) and a.hue_sat == (-20.0, 20.0) and a.elastic_alpha == (0.5, 3.5)),
                        (['--augment-warps', '--augment-blends'], lambda a: isinstance(a, DeviceAugment) and a.frequency_blend),
                        (['--augment-warps'], lambda a: isinstance(a, DeviceAugment) and a.hue_sat is None and not a.frequency_blend),
                        (['--augment'], lambda a: a is True), ([], lambda a: a is False)):
        monkeypatch.setattr(sys, 'argv', ['train.py', 'data/x'] + argv)
        train.main()
        assert check(seen['args'][-1]), argv


# ------------------------------------------------------------------ the restatement on its own
def test_median_and_hue_restatements():
    rng = np.random.default_rng(3)
    q = rng.integers(0, 256, (3, 6, 9)).astype(np.float64)
    for k in R.MEDIANS:                                           # against a plain loop; windows wider than the grid included
        m = R.median(q, k)
        for (c, y, x) in ((0, 0, 0), (1, 5, 8), (2, 3, 4), (0, 2, 0)):
            ys, xs = G.reflect101(np.arange(y - k // 2, y + k // 2 + 1), 6), G.reflect101(np.arange(x - k // 2, x + k // 2 + 1), 9)
            assert m[c, y, x] == sorted(q[c][ys][:, xs].ravel())[(k * k - 1) // 2]
        # the window of a pixel beyond the grid, taken at unreflected indices, holds the taps of the reflected pixel's window
        for p in (-1, -4, 9, 13):
            a = np.sort(q[0][3, G.reflect101(np.arange(p - k // 2, p + k // 2 + 1), 9)])
            b = np.sort(q[0][3, G.reflect101(G.reflect101([p], 9)[0] + np.arange(-(k // 2), k // 2 + 1), 9)])
            assert np.array_equal(a, b)
    assert np.array_equal(R.median(q[:, :1, :1], 11), q[:, :1, :1])
    # hue / saturation: a grey stays grey under a hue shift or a desaturation (a positive ds colours it: s' = ds at hue dh), a
    # sixth of a turn permutes the primaries and secondaries, desaturation pulls towards the maximum
    grey = np.array([[10.0], [10.0], [10.0]])
    assert np.array_equal(R.hue_sat(grey, 1.7, 0.0), grey) and np.array_equal(R.hue_sat(grey, 1.7, -0.3), grey)
    assert np.allclose(R.hue_sat(grey, 0.0, 0.3), [[10.0], [7.0], [7.0]], atol=1e-12)
    wheel = np.array([[255, 255, 0, 0, 0, 255], [0, 255, 255, 255, 0, 0], [0, 0, 0, 255, 255, 255]], dtype=np.float64)
    assert np.array_equal(R.hue_sat(wheel, 1.0, 0.0), np.roll(wheel, -1, axis=1)) and np.array_equal(R.hue_sat(wheel, 6.0, 0.0), wheel)
    assert np.array_equal(R.hue_sat(wheel, -1.0, 0.0), np.roll(wheel, 1, axis=1))
    assert np.array_equal(R.hue_sat(wheel, 0.0, -1.0), np.full((3, 6), 255.0))
    c = rng.integers(0, 256, (3, 500)).astype(np.float64)
    assert np.abs(R.hue_sat(c, 0.0, 0.0) - c).max() < 1e-9 and np.abs(R.hue_sat(c, 12.0, 0.0) - c).max() < 1e-9
    # continuity across the sector boundaries and the wrap: a small dh moves every value by little
    step = np.abs(R.hue_sat(c, 1e-6, 0.0) - c).max()
    assert step < 1e-3, step


@pytest.mark.parametrize('H,W', R.GRIDS)
def test_restatement_stays_inside_the_caps(H, W):
    """what the GPU comparisons rely on, at their shapes, rows and inputs: the share of pixels each of them excludes, from the
    restatement alone"""
    imgs, segs = _batch(R.B, H, W)
    for k in R.MEDIANS:
        for out_hw in G.out_sizes(H, W):
            assert R.restate(imgs, segs, R.median_rows(H, W, k), out_hw)['ok'].all()
    for name in ('gaussian 1.7', 'composed 13'):
        r = R.restate(imgs, segs, R.median_rows(H, W, 5, True, G.filter_of(name)))
        shares = [R.excluded(r, b) for b in range(R.B)]
        print('median 5 + %s %dx%d: excluded' % (name, H, W), ['%.4f' % s for s in shares])
        assert max(shares) <= G.excluded_cap(name)
        assert (r['q'] != R.restate(imgs, segs, R.blend_table(R.warp_rows(H, W, True, G.filter_of(name))))['q']).mean() > 0.3
    for out_hw in G.out_sizes(H, W):
        iy, ix = (np.arange(H), np.arange(W)) if out_hw is None else (G.ms_index(out_hw[0], H), G.ms_index(out_hw[1], W))
        rows = R.sampler_rows(H, W)
        want = 255.0 * (1.0 - R.mask_sample(rows[0, aug.BLEND_T2:aug.BLEND_T2 + 256], H, W))[iy][:, ix]
        share = 1.0 - (_half_distance(want) > R.SAMPLER_MARGIN).mean()
        print('sampler %dx%d -> %s: excluded %.4f' % (H, W, out_hw, share))
        assert share <= R.SAMPLER_CAP and want.max() - want.min() > 200
        assert np.array_equal(R.restate(imgs, segs, rows, out_hw)['q'], np.broadcast_to(_round8(want), (R.B, 3) + want.shape))
        for what, rows in [('edge %s' % (c,), R.edge_rows(H, W, *c)) for c in R.EDGE_CASES] + [('colour', R.colour_rows(H, W))]:
            r = R.restate(imgs, segs, rows, out_hw)
            shares = [R.excluded(r, b) for b in range(R.B)]
            print('%s %dx%d -> %s: excluded' % (what, H, W, out_hw), ['%.4f' % s for s in shares])
            assert max(shares) <= R.FILTER_CAP
    # the blends do blend: neither branch alone gives the result
    r = R.restate(imgs, segs, R.colour_rows(H, W))
    for M in (R.MA, R.MB):
        assert (r['q'] != R.restate(imgs, segs, R.blend_table(R.warp_rows(H, W, True, colour=M)))['q']).mean() > 0.3


def test_hue_inputs_stay_inside_the_cap_and_tiny_grids_exclude_little():
    imgs, segs = R.hue_batch()
    H, W = R.GRIDS[0]
    px = set(map(tuple, imgs[0].reshape(3, -1).T.tolist()))
    assert {(0, 0, 0), (255, 255, 255), (77, 77, 77), (255, 0, 0), (0, 255, 255), (200, 200, 50), (50, 200, 200)} <= px
    for dh_ds in R.hue_shifts():
        r = R.restate(imgs, segs, R.hue_rows(H, W, dh_ds))
        shares = [R.excluded(r, b) for b in range(R.B)]
        print('hue / saturation dh %.4f ds %.4f: excluded' % dh_ds, ['%.4f' % s for s in shares])
        assert max(shares) <= R.SAMPLER_CAP
    assert R.HUE_BEYOND[0] > 6 and R.hue_shifts()[2] == (0.0, 0.0)
    for H, W in R.TINY:                                           # a sample far from a half-integer at every pixel
        rows = R.sampler_rows(H, W)
        want = 255.0 * (1.0 - R.mask_sample(rows[0, aug.BLEND_T2:aug.BLEND_T2 + 256], H, W))
        assert (_half_distance(want) > R.SAMPLER_MARGIN).all()
        for k in R.MEDIANS:
            assert R.restate(*_batch(R.B, H, W), R.median_rows(H, W, k))['ok'].all()
