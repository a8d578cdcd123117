"""Host side of the warp augmentation (utils/augment.py: elastic, piecewise-affine, perspective; pseg_augment_batch_warp's
row): the row layout against the header, the untouched default and full() tables, the perspective matrix and its refusals,
what DeviceAugment.warps() draws, the dispatch by row width, the train.py flag, and the fp64 restatement that
tests/test_augment_warp_gpu.py holds the kernel to, on its own.  No GPU."""
import re
import sys

import numpy as np
import pytest
import torch

from pytorch_segmentation_amd.utils import augment as aug
from pytorch_segmentation_amd.utils.augment import DeviceAugment

import test_augment_nbhd_gpu as G
import test_augment_warp_gpu as Wp
from test_augment_gpu import _batch

GOLDEN = __file__.rsplit('/', 1)[0] + '/golden/augment_tables_abi13.npz'
WARP_KEYS = ('elastic', 'piecewise', 'perspective')


# ------------------------------------------------------------------ layout
def test_warp_row_layout_matches_the_header():
    from pytorch_segmentation_amd import _lib, ops
    src = open(_lib.HEADER_PATH).read()
    d = {k: int(v) for k, v in re.findall(r'#define\s+PSEG_AUGMENT_WARP_(\w+)\s+(\d+)', src)}
    assert d == {'ROW': aug.WARP_ROW, 'H2': aug.WARP_H2, 'ALPHA': aug.WARP_ALPHA, 'GRID_ON': aug.WARP_GRID_ON, 'GRID': aug.WARP_GRID}
    assert ops.AUGMENT_WARP_ROW == aug.WARP_ROW == 252
    assert aug.WARP_H2 == aug.NBHD_ROW and aug.WARP_H2 + 3 <= aug.WARP_ALPHA < aug.WARP_GRID_ON < aug.WARP_GRID
    assert aug.WARP_GRID + 2 * aug.WARP_NODES ** 2 == aug.WARP_ROW
    assert _lib.abi_version_of_header() == 14
    protos = _lib.parse_header()
    assert protos['pseg_augment_batch_warp'][1:] == protos['pseg_augment_batch_nbhd'][1:]
    assert 'pseg_augment_batch_warp' in _lib.prototypes()


def test_warp_row_keeps_the_nbhd_row_and_the_seed_bits():
    base = aug.make_row(np.array([[0.5, 0.1, 3], [0.2, 1.5, -4.]]), None, 9.0, 1, 1)
    grid = np.arange(32, dtype=np.float64).reshape(4, 4, 2) - 7
    for seed in (0, 2 ** 64 - 1, 0xFFC00001_7FA00001, 0x7F800000_FF800000):          # NaN and infinity patterns as floats
        nb = aug.make_nbhd_row(base, np.arange(9.).reshape(3, 3), (3.5, True), (0.25, False, 4, 7), seed)
        row = aug.make_warp_row(nb, (1e-3, -2e-3, 1.0), 2.5, grid)
        assert row.dtype == np.float32 and row.shape == (aug.WARP_ROW,)
        assert row[:aug.NBHD_ROW].tobytes() == nb.tobytes() and G.row_seed(row) == seed
        assert list(row[aug.WARP_H2:aug.WARP_H2 + 3]) == [np.float32(1e-3), np.float32(-2e-3), 1.0]
        assert row[aug.WARP_ALPHA] == 2.5 and row[aug.WARP_GRID_ON] == 1 and not row[aug.WARP_GRID_ON + 1:aug.WARP_GRID].any()
        # node (j, i) at 220 + 2 (4 j + i): dx, dy
        assert row[aug.WARP_GRID + 2 * (4 * 2 + 1)] == grid[2, 1, 0] and row[aug.WARP_GRID + 2 * (4 * 2 + 1) + 1] == grid[2, 1, 1]
        assert np.array_equal(aug.row_shapes(np.stack([row])), np.array([[3, 4, 7]], dtype=np.int32))
    off = aug.make_warp_row()
    assert list(off[aug.WARP_H2:]) == [0, 0, 1] + [0] * 37 and off[:aug.NBHD_ROW].tobytes() == aug.make_nbhd_row().tobytes()
    with pytest.raises(ValueError):
        aug.make_warp_row(nb, grid=np.zeros((3, 3, 2)))


def test_reference_and_full_tables_are_unchanged():
    """the new arguments are off by default and an augmenter that is off draws nothing: reference() draws the golden tables
    byte for byte, and full() draws what a sampler without slots 10..12 draws (the same generator state after every sample)"""
    golden = np.load(GOLDEN)
    for seed in range(4):
        a = DeviceAugment.reference(seed=seed, rank=0)
        got = np.concatenate([a.sample(16, 37, 83), a.sample(5, 70, 131)])
        assert got.tobytes() == golden['reference_seed%d' % seed].tobytes()
    new = ('elastic_alpha', 'elastic_p', 'piecewise_scale', 'piecewise_p', 'perspective_scale', 'perspective_p')
    ref, full, warps = DeviceAugment.reference(seed=1), DeviceAugment.full(seed=1), DeviceAugment.warps(seed=1)
    assert all(getattr(ref, k) is None and getattr(full, k) is None and getattr(warps, k) is not None for k in new)
    assert {k: v for k, v in vars(full).items() if k not in new} == {k: v for k, v in vars(warps).items() if k not in new}
    assert (warps.elastic_alpha, warps.piecewise_scale, warps.perspective_scale) == ((0.5, 3.5), (0.01, 0.05), (0.01, 0.1))
    assert (warps.elastic_p, warps.piecewise_p, warps.perspective_p) == (0.5, 0.5, 0.5)
    assert DeviceAugment.warps(elastic_alpha=None, seed=1).elastic_alpha is None
    # full(): no recipe holds a warp key, and a sampler whose slots 10..12 are dead (p = 0 draws one number, so compare with
    # ranges of None) consumes the generator identically
    full, dead = DeviceAugment.full(seed=3, rank=0), DeviceAugment.warps(seed=3, rank=0, elastic_alpha=None, piecewise_scale=None,
                                                                        perspective_scale=None)
    fr, dr = full.draw(300), dead.draw(300)
    assert not any(k in r for r in fr for k in WARP_KEYS)
    assert DeviceAugment.rows(fr, 37, 83).tobytes() == DeviceAugment.rows(dr, 37, 83).tobytes()
    assert full.rng.random() == dead.rng.random()


# ------------------------------------------------------------------ perspective
def moved_quad(H, W, f):
    w, h = W - 1.0, H - 1.0
    return np.array([[f[0, 0] * w, f[0, 1] * h], [w - f[1, 0] * w, f[1, 1] * h], [w - f[2, 0] * w, h - f[2, 1] * h], [f[3, 0] * w, h - f[3, 1] * h]])


def test_perspective_matrix_sends_the_moved_quad_to_the_corners():
    rng = np.random.default_rng(0)
    for H, W in ((37, 83), (70, 131), (512, 384)):
        for _ in range(20):
            f = np.minimum(np.abs(rng.normal(0, 0.2, (4, 2))), aug.PERSPECTIVE_CLIP)
            m = aug.perspective_matrix(H, W, f)
            assert m.shape == (3, 3) and m[2, 2] == 1.0
            p = m @ np.vstack([moved_quad(H, W, f).T, np.ones(4)])
            assert np.abs(p[:2] / p[2] - np.array([[0, W - 1, W - 1, 0], [0, 0, H - 1, H - 1]])).max() < 1e-9 * max(H, W)
            # forward_matrix multiplies it in after the affine
            r = {'affine': {'rotate': 20.0, 'scale': (1.1, 0.9), 'shear': 4.0, 'translate': (0.1, 0.0)}, 'perspective': f}
            assert np.allclose(aug.forward_matrix(r, H, W), m @ aug.affine_matrix(H, W, **r['affine']), rtol=0, atol=1e-12)
    assert np.array_equal(aug.perspective_matrix(37, 83, np.zeros((4, 2))).round(12), np.eye(3))
    assert np.array_equal(aug.perspective_matrix(5, 1, np.full((4, 2), 0.2)), np.eye(3))      # a line has no perspective


def _corner_dens(row, H, W):
    h2 = row[aug.WARP_H2:aug.WARP_H2 + 3].astype(np.float64)
    assert h2[2] == 1.0
    return h2[0] * np.array([0, W - 1, 0, W - 1]) + h2[1] * np.array([0, 0, H - 1, H - 1]) + 1.0


def test_clip_keeps_the_denominator_positive_and_a_degenerate_quad_raises():
    H, W = 70, 131
    # what the sampler draws at the upper end of the range, |N(0, 0.1)| clipped to 0.4, every sample: rows() takes them all
    a = DeviceAugment.warps(seed=4, rank=0, perspective_scale=(0.1, 0.1), perspective_p=1.0, some_of=(16, 16))
    recipes = [r for r in a.draw(3000) if 'perspective' in r]
    assert len(recipes) >= 2990 and max(r['perspective'].max() for r in recipes) == aug.PERSPECTIVE_CLIP
    for row, r in zip(DeviceAugment.rows(recipes, H, W), recipes):
        assert (_corner_dens(row, H, W) > 0).all() and aug.quad_is_convex(r['perspective'])
    # corners AT the clip: each stays in its own quadrant, which alone does not make the quad convex.  A convex quad has
    # den > 0 on the grid and the row is its inverse (the image corners read the moved quad); any other raises, and the
    # sampler drops such a draw
    rng = np.random.default_rng(1)
    seen = {True: 0, False: 0}
    for _ in range(300):
        f = np.where(rng.random((4, 2)) < 0.5, aug.PERSPECTIVE_CLIP, rng.uniform(0, aug.PERSPECTIVE_CLIP, (4, 2)))
        convex = aug.quad_is_convex(f)
        seen[convex] += 1
        if not convex:
            with pytest.raises(ValueError):
                DeviceAugment.rows([Wp.recipe(0, 0, perspective=f)], H, W)
            continue
        row = DeviceAugment.rows([Wp.recipe(0, 0, perspective=f)], H, W)[0]
        assert (_corner_dens(row, H, W) > 0).all()
        hm = np.vstack([row[0:6].astype(np.float64).reshape(2, 3), row[aug.WARP_H2:aug.WARP_H2 + 3].astype(np.float64)])
        p = hm @ np.array([[0, W - 1, W - 1, 0], [0, 0, H - 1, H - 1], [1, 1, 1, 1.]])
        assert np.abs(p[:2] / p[2] - moved_quad(H, W, f).T).max() < 1e-5 * W / p[2].min()     # fp32 rows; a thin quad has a small den
    assert seen[True] > 50 and seen[False] > 5
    for bad in (np.array([[0.9, 0.0], [0.9, 0.0], [0.0, 0.0], [0.0, 0.0]]),       # the top edge's corners cross: a bow tie
                np.array([[0.5, 0.5]] * 4),                                        # all four corners in one point
                np.array([[0.0, 0.0], [0.0, 0.0], [0.7, 0.7], [0.0, 0.0]])):       # not convex
        assert not aug.quad_is_convex(bad)
        with pytest.raises(ValueError):
            DeviceAugment.rows([Wp.recipe(0, 0, perspective=bad)], H, W)


# ------------------------------------------------------------------ the grid
def test_uniform_grid_folds_to_a_translation():
    H, W = 37, 83
    nb = G.nbhd_table(G.base_rows(H, W, True))
    wide, folded = Wp.warp_table(nb, grid=Wp.uniform_grid(3.0, -2.0)), Wp.warp_table(Wp.fold_translation(nb, 3.0, -2.0))
    for b in range(G.B):
        a, c = Wp.source_coords(wide[b], np.arange(H), np.arange(W), H, W), Wp.source_coords(folded[b], np.arange(H), np.arange(W), H, W)
        assert all(np.array_equal(u, v) for u, v in zip(a, c))
        still = Wp.source_coords(Wp.warp_table(nb)[b], np.arange(H), np.arange(W), H, W)
        assert not np.array_equal(a[0], still[0]) and not np.array_equal(a[1], still[1])
    # a node's displacement is what the pixel at the node gets, and a pixel beyond the image takes the border's
    grid = np.random.default_rng(2).normal(0, 2, (4, 4, 2))
    row = aug.make_warp_row(None, grid=grid)
    g32 = grid.astype(np.float32).astype(np.float64)
    sx, sy, _ = Wp.source_coords(row, np.array([0, 12, 24, 36]), np.array([0, 82]), H, W)      # rows at the nodes: j (H - 1) / 3
    assert np.allclose(sx - np.array([0, 82]), g32[:, [0, 3], 0], atol=1e-12) and np.allclose(sy - np.array([[0], [12], [24], [36]]), g32[:, [0, 3], 1], atol=1e-12)
    out, edge = Wp.source_coords(row, np.array([-5, 40]), np.array([-9, 90]), H, W), Wp.source_coords(row, np.array([0, 36]), np.array([0, 82]), H, W)
    assert np.allclose(out[0] - np.array([-9, 90]), edge[0] - np.array([0, 82])) and np.allclose(out[1] - np.array([[-5], [40]]), edge[1] - np.array([[0], [36]]))


# ------------------------------------------------------------------ what warps() draws
def _within(k, n, p):
    return abs(k - n * p) <= 4.0 * np.sqrt(n * p * (1 - p))


def test_warps_draws_ranges_frequencies_and_row_widths():
    n, H, W = 20000, 512, 384
    recipes = DeviceAugment.warps(seed=9).draw(n)
    slot = 2.5 / aug.COLOUR_SLOTS * 0.5                        # a slot is picked 2.5 / 16 of the time, Sometimes(0.5)
    for k in WARP_KEYS:
        assert _within(sum(k in r for r in recipes), n, slot), k
    el = [r['elastic'] for r in recipes if 'elastic' in r]
    assert all(isinstance(a, float) and 0.5 <= a <= 3.5 for a in el) and min(el) < 0.7 and max(el) > 3.3
    pw = np.stack([r['piecewise'] for r in recipes if 'piecewise' in r])
    assert pw.shape[1:] == (4, 4, 2)
    s = pw.reshape(len(pw), -1).std(axis=1)                    # 32 draws of N(0, s), s ~ U(0.01, 0.05)
    assert 0.005 < s.min() < 0.02 and 0.04 < s.max() < 0.08 and abs(pw.mean()) < 1e-3
    ps = np.stack([r['perspective'] for r in recipes if 'perspective' in r])
    assert ps.shape[1:] == (4, 2) and ps.min() >= 0 and ps.max() <= aug.PERSPECTIVE_CLIP and 0.02 < ps.mean() < 0.06
    assert (ps.max(axis=(1, 2)) > 0.2).any()                   # |N(0, 0.1)| does reach far
    for r in recipes:
        assert ('seed' in r) == ('noise' in r or 'dropout' in r or 'elastic' in r)
    seeds = [r['seed'] for r in recipes if 'seed' in r]
    assert len(set(seeds)) == len(seeds)

    # row width by recipe content
    is_warp = [any(k in r for k in WARP_KEYS) for r in recipes]
    is_nbhd = [bool(r.get('filters') or 'noise' in r or 'dropout' in r) for r in recipes]
    warp = [r for r, w in zip(recipes, is_warp) if w][:40]
    nbhd = [r for r, w, m in zip(recipes, is_warp, is_nbhd) if m and not w][:8]
    plain = [r for r, w, m in zip(recipes, is_warp, is_nbhd) if not m and not w][:8]
    assert DeviceAugment.rows(plain, H, W).shape == (8, aug.ROW) and DeviceAugment.rows(nbhd + plain, H, W).shape == (16, aug.NBHD_ROW)
    table = DeviceAugment.rows(plain + nbhd + warp[:1], H, W)
    assert table.shape == (17, aug.WARP_ROW)
    assert np.array_equal(table[:16, :aug.NBHD_ROW].view(np.uint32), DeviceAugment.rows(nbhd + plain, H, W)[[8, 9, 10, 11, 12, 13, 14, 15, 0, 1, 2, 3, 4, 5, 6, 7]].view(np.uint32))
    assert np.array_equal(table[:16, aug.WARP_H2:], np.tile(aug.make_warp_row()[aug.WARP_H2:], (16, 1)))
    for r, row in zip(warp, DeviceAugment.rows(warp, H, W)):
        assert row[aug.WARP_ALPHA] == np.float32(r.get('elastic', 0.0)) and G.row_seed(row) == r.get('seed', 0)
        assert (row[aug.WARP_GRID_ON] == 1) == ('piecewise' in r)
        if 'piecewise' in r:                                   # minus the jitter times (W, H)
            assert np.array_equal(row[aug.WARP_GRID:].reshape(4, 4, 2), (-r['piecewise'] * (W, H)).astype(np.float32))
        else:
            assert not row[aug.WARP_GRID:].any()
        assert ('perspective' in r) == bool(row[aug.WARP_H2] != 0 or row[aug.WARP_H2 + 1] != 0) and row[aug.WARP_H2 + 2] == 1.0
    # the first batch of the end-to-end GPU test holds a warp
    first = DeviceAugment.warps(seed=0, rank=0).sample(Wp.TRAIN_SET['batch_size'], 64, 64)
    assert first.shape == (Wp.TRAIN_SET['batch_size'], aug.WARP_ROW)


def test_apply_dispatches_on_the_row_width(monkeypatch):
    """a batch that drew no warp never reaches the warp kernel: its cost cannot change"""
    from pytorch_segmentation_amd import ops
    calls = []
    for name in ('augment_batch', 'augment_batch_nbhd', 'augment_batch_warp'):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **kw: calls.append((_n, a[2].shape[1])) or (None, None))
    monkeypatch.setattr(torch.Tensor, 'pin_memory', lambda self: self)
    a = DeviceAugment.identity()
    imgs, segs = torch.zeros(2, 3, 8, 8, dtype=torch.uint8), torch.zeros(2, 8, 8, dtype=torch.uint8)
    narrow = np.stack([aug.make_row()] * 2)
    nb = np.stack([aug.make_nbhd_row(r) for r in narrow])
    for table in (narrow, nb, np.stack([aug.make_warp_row(r) for r in nb])):
        a.apply(imgs, segs, table)
    assert calls == [('augment_batch', aug.ROW), ('augment_batch_nbhd', aug.NBHD_ROW), ('augment_batch_warp', aug.WARP_ROW)]


def test_augment_warps_flag_reaches_train(monkeypatch):
    import train
    ap = train.build_parser()
    assert ap.parse_args(['data/x']).augment_warps is False and ap.parse_args(['data/x', '--augment-warps']).augment_warps is True
    seen = {}

    def fake_train(*args, **kw):
        seen['args'] = args

    monkeypatch.setattr(train, 'train', fake_train)
    monkeypatch.setattr(train.torch.cuda, 'set_device', lambda i: None)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    for argv, check in ((['--augment-warps'], lambda a: isinstance(a, DeviceAugment) and a.elastic_alpha == (0.5, 3.5) and a.noise_scale == (0.0, 12.75)),
                        (['--augment-full', '--augment-warps'], lambda a: isinstance(a, DeviceAugment) and a.perspective_scale == (0.01, 0.1)),
                        (['--augment-full'], lambda a: isinstance(a, DeviceAugment) and a.elastic_alpha is None),
                        (['--augment'], lambda a: a is True), ([], lambda a: a is False)):
        monkeypatch.setattr(sys, 'argv', ['train.py', 'data/x'] + argv)
        train.main()
        assert check(seen['args'][-1]), argv


# ------------------------------------------------------------------ the restatement on its own
def test_elastic_stream_is_new_and_uniform():
    row = aug.make_warp_row(aug.make_nbhd_row(seed=G.SEEDS[0]), alpha=2.0)
    H, W = 70, 131
    sx, sy, ok = Wp.source_coords(row, np.arange(H), np.arange(W), H, W)
    jx, jy = (sx - np.arange(W)) / 2.0, (sy - np.arange(H)[:, None]) / 2.0
    n = jx.size
    assert ok.all() and jx.min() >= -1 and jx.max() < 1 and jy.min() >= -1 and jy.max() < 1
    for j in (jx, jy):                                         # U(-1, 1): mean 0, variance 1/3
        assert abs(j.mean()) < 5 / np.sqrt(3 * n) and abs(j.var() - 1 / 3) < 5 * np.sqrt(4 / 45 / n)
    assert abs(np.corrcoef(jx.ravel(), jy.ravel())[0, 1]) < 5 / np.sqrt(n)
    pix = np.arange(H * W, dtype=np.uint64).reshape(H, W)
    assert np.array_equal(jx, 2.0 * G.uniform24(G.philox4x32_10(pix, 8, G.SEEDS[0])[0]) - 1.0)
    for stream in range(7):                                    # not one of the noise / dropout streams
        assert not np.array_equal(jx, 2.0 * G.uniform24(G.philox4x32_10(pix, stream, G.SEEDS[0])[0]) - 1.0)


@pytest.mark.parametrize('H,W', Wp.GRIDS)
def test_restatement_stays_inside_the_caps(H, W):
    """what the GPU tests rely on, at their shapes and rows: few nearest samples of the restatement are undecided (2 %), few
    bilinear values lie within 0.05 of a half-integer (15 %), and few 3 x 3 windows under elastic jitter hold an
    undecided pixel (6 %)"""
    imgs, segs = _batch(Wp.B, H, W)
    for case in Wp.CASES:
        for order in (0, 1):
            for mode in (0, 1):
                o = Wp.oracle(imgs, segs, Wp.case_rows(case, H, W, order, mode))
                lab = [1.0 - o['label_ok'][b].mean() for b in range(Wp.B)]
                img = [1.0 - o['img_ok'][b].mean() for b in range(Wp.B)]
                print('%s %dx%d order=%d mode=%d: labels excluded' % (case, H, W, order, mode), ['%.4f' % s for s in lab],
                      'image excluded', ['%.4f' % s for s in img])
                assert max(lab) <= 0.02 and max(img) <= (0.15 if order else 0.02)
    rows = Wp.elastic_filter_rows(H, W)
    decided = Wp.oracle(imgs, segs, rows)['label_ok']
    shares = [1.0 - Wp.window_decided(decided[b], 3).mean() for b in range(Wp.B)]
    print('elastic + sharpen %dx%d: excluded' % (H, W), ['%.4f' % s for s in shares])
    assert max(shares) <= Wp.ELASTIC_FILTER_CAP
    # and that check tells the halo's jitter apart: filled with the jitter of the unreflected index the border differs
    border = np.zeros((H, W), dtype=bool)
    border[0], border[-1], border[:, 0], border[:, -1] = True, True, True, True
    right, wrong = Wp.restate_filtered(imgs, segs, rows)['q'], Wp.restate_with_unreflected_halo(imgs, rows)
    assert (wrong[:, :, border] != right[:, :, border]).mean() > 0.2
    inner = ~border
    assert np.array_equal(wrong[:, :, inner], right[:, :, inner])
    # restate_filtered's filter and colour stages are test_augment_nbhd_gpu.restate's (there behind an affine warp)
    nb = G.nbhd_table(G.base_rows(H, W, True), G.filter_of('emboss strong'))
    assert np.array_equal(Wp.restate_filtered(imgs, segs, Wp.warp_table(nb))['q'], G.restate(imgs, segs, nb)['q'])
    # image == mask in the restatement too
    imgs3 = np.ascontiguousarray(np.broadcast_to(segs[:, None], imgs.shape))
    o = Wp.oracle(imgs3, segs, Wp.case_rows('all', H, W, 0, 0, cval=0.0))
    assert np.array_equal(o['q'], np.broadcast_to(o['label'][:, None], o['q'].shape).astype(np.float64))


@pytest.mark.parametrize('H,W', Wp.TINY)
def test_tiny_grid_rows_leave_nothing_undecided(H, W):
    """the rows of the one- and five-pixel grids (the W == 1 guard of the displacement grid): a draw exists for every case
    in which the restatement excludes nothing, the grid and the jitter do move the coordinates, and pixels read inside"""
    imgs, segs = _batch(Wp.B, H, W)
    inside = 0
    for case in Wp.CASES:
        for order in (0, 1):
            for mode in (0, 1):
                rows = Wp.tiny_rows(case, H, W, order, mode)
                o = Wp.oracle(imgs, segs, rows)
                assert o['label_ok'].all() and o['img_ok'].all()
                for b in range(Wp.B):
                    sx, sy, ok = Wp.source_coords(rows[b], np.arange(H), np.arange(W), H, W)
                    inside += int((ok & (np.abs(sx) < W - 0.5) & (sy > -0.5) & (sy < H - 0.5)).sum())
                    if case in ('grid', 'elastic'):                          # identity matrix: the displacement itself
                        assert (sx != np.arange(W)).all() and (sy != np.arange(H)[:, None]).all()
    assert inside >= 0.4 * len(Wp.CASES) * 4 * Wp.B * H * W
