"""Connected regions on the device (csrc/regions.hip) against the plain reference (tests/regions_ref.py): labels, records
and cleaned masks must be EQUAL, element for element, for 4- and 8-connectivity.  The shapes are the smallest at which
each stage can go wrong, written in terms of the kernel's tile edge T (ops.REGIONS_TILE): inside one tile, across tile
borders and corners, long equivalence chains through the border merge, labels that must travel back up."""
import numpy as np
import pytest
import torch

import regions_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    from pytorch_segmentation_amd import ops
    return ops


def T():
    from pytorch_segmentation_amd import ops
    return ops.REGIONS_TILE


def _serpentine(t):
    """a one-pixel-wide path (class 1 on 0) that runs right across > 3 tiles, down, back left, down, ... over > 3 tile rows"""
    H, W = 3 * t + 5, 3 * t + 7
    m = np.zeros((H, W), np.uint8)
    for k, y in enumerate(range(1, H - 1, 2)):
        m[y, 1:W - 1] = 1
        if y + 2 < H - 1:
            m[y + 1, W - 2 if k % 2 == 0 else 1] = 1
    return m


def _arms(t, n):
    """n vertical arms (class 1) from the top row down, joined only by the last row: 2 arms = U, 3 arms = W"""
    H, W = 2 * t + 3, 2 * t + 5
    m = np.zeros((H, W), np.uint8)
    for x in np.linspace(1, W - 2, n).astype(int):
        m[:, x] = 1
    m[H - 1, 1:W - 1] = 1
    return m


def _staircase(t):
    """a diagonal of single pixels through the tile corner at (T, T): connected under 8 only"""
    n = t + 6
    m = np.zeros((n, n), np.uint8)
    m[np.arange(n), np.arange(n)] = 1
    return m


def _rings(t):
    n = 2 * t + 3
    yy, xx = np.mgrid[:n, :n]
    d = np.minimum(np.minimum(yy, xx), np.minimum(n - 1 - yy, n - 1 - xx))
    return ((d // 2) % 2).astype(np.uint8) * 3          # square rings two pixels thick, classes 0 / 3: holes within holes


def _checker(h, w):
    yy, xx = np.mgrid[:h, :w]
    return ((yy + xx) % 2).astype(np.uint8)


def _cases():
    t = T()
    rng = np.random.RandomState(5)
    edge = np.zeros((t + 1, 2 * t + 3), np.uint8)
    edge[:, ::3] = 2
    edge[t, :] = 2                                        # columns joined by the one row past the tile border
    side = np.zeros((t + 2, t + 2), np.uint8)
    side[:, :t] = 255                                     # class values 0 and 255 side by side, the border one tile in
    return {
        '1x1': np.full((1, 1), 7, np.uint8),
        '1xN': (np.arange(2 * t + 3) // 5 % 2).astype(np.uint8).reshape(1, -1),
        'Nx1': (np.arange(2 * t + 3) // 5 % 2).astype(np.uint8).reshape(-1, 1),
        'not_a_multiple': edge,
        'uniform': np.full((2 * t + 1, 3 * t + 2), 4, np.uint8),
        'checker': _checker(t + 3, t + 5),
        'serpentine': _serpentine(t),
        'U': _arms(t, 2),
        'W': _arms(t, 3),
        'staircase': _staircase(t),
        'rings': _rings(t),
        '0_and_255': side,
        'random3': rng.randint(0, 3, (40, 50)).astype(np.uint8),
    }


_REF = {}


def _ref_label(name, m, conn):
    """the reference labelling, computed once per (case, connectivity) and shared"""
    key = (name, conn)
    if key not in _REF:
        lab = ref.label(m, conn)
        lab.setflags(write=False)
        _REF[key] = lab
    return _REF[key]


def _pack(ops_mod, masks):
    """-> (device mask, device table, numpy table, npix, max_hw)"""
    from pytorch_segmentation_amd.utils.regions import packed_table
    table, npix, max_hw = packed_table([m.shape for m in masks])
    flat = np.concatenate([m.reshape(-1) for m in masks])
    return torch.from_numpy(flat).cuda(), torch.from_numpy(table).cuda(), table, npix, max_hw


def _split(flat, table):
    return [flat[o:o + h * w].reshape(h, w) for o, h, w in table.tolist()]


CASE_NAMES = ['1x1', '1xN', 'Nx1', 'not_a_multiple', 'uniform', 'checker', 'serpentine', 'U', 'W', 'staircase', 'rings',
              '0_and_255', 'random3']


@pytest.mark.parametrize('conn', [4, 8])
@pytest.mark.parametrize('name', CASE_NAMES)
def test_label_records_clean_equal_reference(ops, name, conn):
    m = _cases()[name]
    want = _ref_label(name, m, conn)
    dmask, dtable, table, npix, max_hw = _pack(ops, [m])
    labels = ops.mask_label(dmask, dtable, npix, max_hw, conn)
    got = labels.cpu().numpy().reshape(m.shape)
    assert np.array_equal(got, want), name
    # what the shape is there to show
    ncomp = len(np.unique(want))
    if name == 'checker':
        assert ncomp == (m.size if conn == 4 else 2)
    if name in ('uniform', '1x1'):
        assert ncomp == 1
    if name == 'staircase':
        assert ncomp == (m.shape[0] + 2 if conn == 4 else 2)
    if name in ('serpentine', 'U', 'W'):
        assert (want[m == 1] == want[m == 1].min()).all()          # one path: one label, however far it travels
    # records: full capacity, in label order
    wrec = ref.records(m, want)
    rec, count = ops.mask_regions(dmask, labels, dtable, npix, max_hw, len(wrec))
    assert int(count.item()) == len(wrec)
    assert rec.cpu().numpy().tolist() == wrec, name
    # cleanup, with and without largest_only
    lut = torch.from_numpy(np.random.RandomState(1).randint(0, 256, (256, 3)).astype(np.uint8)).cuda()
    for min_area, largest in ((3, False), (0, True), (12, True)):
        wclean = ref.clean(m, want, min_area, largest)
        out, rgb = ops.mask_clean(dmask, labels, dtable, npix, max_hw, min_area, largest, lut)
        assert np.array_equal(out.cpu().numpy().reshape(m.shape), wclean), (name, min_area, largest)
        assert torch.equal(rgb, lut[out.long()])
    assert np.array_equal(dmask.cpu().numpy().reshape(m.shape), m)     # out of place: the input is untouched


@pytest.mark.parametrize('conn', [4, 8])
def test_ragged_batch_and_bad_record(ops, conn):
    """three photos of different sizes, one smaller than a tile; then the same batch with the middle record's extent
    leaving the buffer: that photo's labels, records and cleaned pixels are untouched and the others are correct"""
    t = T()
    rng = np.random.RandomState(9)
    masks = [rng.randint(0, 3, (t + 5, 2 * t + 1)).astype(np.uint8), rng.randint(0, 2, (5, 7)).astype(np.uint8),
             rng.randint(0, 4, (2 * t + 2, t - 3)).astype(np.uint8)]
    wlab = [ref.label(m, conn) for m in masks]
    dmask, dtable, table, npix, max_hw = _pack(ops, masks)
    labels = ops.mask_label(dmask, dtable, npix, max_hw, conn)
    for got, want in zip(_split(labels.cpu().numpy(), table), wlab):
        assert np.array_equal(got, want)
    wrec = sum([ref.records(m, l, b) for b, (m, l) in enumerate(zip(masks, wlab))], [])
    rec, count = ops.mask_regions(dmask, labels, dtable, npix, max_hw, len(wrec))
    assert int(count.item()) == len(wrec) and rec.cpu().numpy().tolist() == wrec
    out, _ = ops.mask_clean(dmask, labels, dtable, npix, max_hw, 4, True)
    for got, m, l in zip(_split(out.cpu().numpy(), table), masks, wlab):
        assert np.array_equal(got, ref.clean(m, l, 4, True))

    bad = table.copy()
    bad[1, 0] = npix - 3                                       # 5 x 7 pixels from there: the extent leaves the buffer
    dbad = torch.from_numpy(bad).cuda()
    sentinel = torch.full((npix,), -7, dtype=torch.int32, device='cuda')
    labels = ops.mask_label(dmask, dbad, npix, max_hw, conn, out=sentinel)
    got = _split(labels.cpu().numpy(), table)
    assert np.array_equal(got[0], wlab[0]) and np.array_equal(got[2], wlab[2]) and (got[1] == -7).all()
    wrec = ref.records(masks[0], wlab[0], 0) + ref.records(masks[2], wlab[2], 2)
    rec, count = ops.mask_regions(dmask, labels, dbad, npix, max_hw, len(wrec) + 3)
    assert int(count.item()) == len(wrec) and rec[:len(wrec)].cpu().numpy().tolist() == wrec
    out = torch.full((npix,), 99, dtype=torch.uint8, device='cuda')
    ops.mask_clean(dmask, labels, dbad, npix, max_hw, 4, True, out=out)
    got = _split(out.cpu().numpy(), table)
    assert (got[1] == 99).all()
    assert np.array_equal(got[0], ref.clean(masks[0], wlab[0], 4, True))
    assert np.array_equal(got[2], ref.clean(masks[2], wlab[2], 4, True))


def test_regions_capacity_and_guard_band(ops):
    """max_regions below the count: count is full, the prefix is right, nothing is written past it"""
    m = _cases()['random3']
    want = _ref_label('random3', m, 8)
    wrec = ref.records(m, want)
    dmask, dtable, table, npix, max_hw = _pack(ops, [m])
    labels = ops.mask_label(dmask, dtable, npix, max_hw, 8)
    W = ops.REGION_WORDS
    for cap in (0, 1, len(wrec) // 2):
        buf = torch.full(((cap + 4) * W,), -12345, dtype=torch.int64, device='cuda')
        rec, count = ops.mask_regions(dmask, labels, dtable, npix, max_hw, cap, records=buf)
        assert int(count.item()) == len(wrec) > cap
        host = buf.cpu().numpy()
        assert host[:cap * W].reshape(cap, W).tolist() == wrec[:cap]
        assert (host[cap * W:] == -12345).all()
    # capacity above the count: the words past the count stay as they were
    buf = torch.full(((len(wrec) + 4) * W,), -12345, dtype=torch.int64, device='cuda')
    ops.mask_regions(dmask, labels, dtable, npix, max_hw, len(wrec) + 4, records=buf)
    host = buf.cpu().numpy()
    assert host[:len(wrec) * W].reshape(-1, W).tolist() == wrec and (host[len(wrec) * W:] == -12345).all()


def test_clean_copy_in_place_colours_and_ties(ops):
    t = T()
    m = _cases()['random3']
    want = _ref_label('random3', m, 4)
    dmask, dtable, table, npix, max_hw = _pack(ops, [m])
    labels = ops.mask_label(dmask, dtable, npix, max_hw, 4)
    lut = torch.from_numpy(np.random.RandomState(2).randint(0, 256, (256, 3)).astype(np.uint8)).cuda()
    for k in (0, 1):                                           # min_area 0 / 1 copies the mask
        out, rgb = ops.mask_clean(dmask, labels, dtable, npix, max_hw, k, False, lut)
        assert torch.equal(out, dmask) and torch.equal(rgb, lut[dmask.long()])
    # in place and out of place agree, colours equal lut[mask_out], and a guard band after the buffer stays
    out, rgb = ops.mask_clean(dmask, labels, dtable, npix, max_hw, 5, False, lut)
    assert np.array_equal(out.cpu().numpy().reshape(m.shape), ref.clean(m, want, 5))
    assert torch.equal(rgb, lut[out.long()])
    big = torch.full((4 * npix + 64,), 201, dtype=torch.uint8, device='cuda')
    big[:npix] = dmask
    out2, rgb2 = ops.mask_clean(big[:npix], labels, dtable, npix, max_hw, 5, False, lut, out=big[:4 * npix])
    assert out2.data_ptr() == big.data_ptr()
    assert torch.equal(out2, out) and torch.equal(rgb2, rgb) and (big[4 * npix:] == 201).all()
    # largest_only, two equal-area components of one class in different tiles: the smaller label stays
    tie = np.zeros((t + 6, t + 6), np.uint8)
    tie[1:3, 1:4] = 1
    tie[t + 2:t + 4, t + 1:t + 4] = 1
    tie[5, 5] = 2
    dmask, dtable, table, npix, max_hw = _pack(ops, [tie])
    labels = ops.mask_label(dmask, dtable, npix, max_hw, 8)
    out, _ = ops.mask_clean(dmask, labels, dtable, npix, max_hw, 0, True)
    wclean = ref.clean(tie, ref.label(tie, 8), 0, True)
    got = out.cpu().numpy().reshape(tie.shape)
    assert np.array_equal(got, wclean)
    assert (got[1:3, 1:4] == 1).all() and (got[t + 2:t + 4, t + 1:t + 4] == 0).all() and got[5, 5] == 2


def test_argument_checks(ops):
    from pytorch_segmentation_amd._lib import PsegError
    m = np.zeros((3, 3), np.uint8)
    dmask, dtable, table, npix, max_hw = _pack(ops, [m])
    with pytest.raises(PsegError, match='connectivity'):
        ops.mask_label(dmask, dtable, npix, max_hw, 6)
    with pytest.raises(PsegError, match='2\\^31'):
        ops.mask_label(dmask, dtable, npix, (65535, 65535), 8)


def test_clean_predictions_for_evaluation(ops):
    """test.py's route: int64 [B,H,W] predictions in, the reference cleaning of each out"""
    from pytorch_segmentation_amd.utils.regions import clean_predictions
    rng = np.random.RandomState(6)
    pred = rng.randint(0, 3, (2, 37, 41))
    got = clean_predictions(torch.from_numpy(pred).cuda(), 5, 4, True).cpu().numpy()
    assert got.dtype == np.int64
    for g, p in zip(got, pred.astype(np.uint8)):
        assert np.array_equal(g, ref.clean(p, ref.label(p, 4), 5, True))


def _tiny_model():
    from pytorch_segmentation_amd import models
    torch.manual_seed(3)
    return models.UNet(3).cuda().eval()


@pytest.mark.parametrize('flip', [False, True])
def test_inference_end_to_end(ops, flip):
    """inference(..., min_area=k) equals the reference cleaning of inference(...)'s own mask; regions=True returns what the
    reference records of that cleaned mask give; the colours are the cleaned mask's"""
    from pytorch_segmentation_amd.utils import VOC_COLORMAP, inference
    from pytorch_segmentation_amd.utils.regions import region_geometry
    rng = np.random.RandomState(4)
    photos = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in ((50, 70), (64, 64))]
    m = _tiny_model()
    kw = {'flip': True} if flip else {}
    raw = inference(m, photos, (64, 64), **kw)
    for conn, k, largest in ((8, 6, False), (4, 3, True)):
        masks, colored, regions = inference(m, photos, (64, 64), colors=VOC_COLORMAP, min_area=k, connectivity=conn,
                                            largest_only=largest, regions=True, **kw)
        for b, (r, got, col, regs) in enumerate(zip(raw, masks, colored, regions)):
            r8 = r.astype(np.uint8)
            want = ref.clean(r8, ref.label(r8, conn), k, largest)
            assert got.dtype == np.int64 and np.array_equal(got, want)
            assert np.array_equal(col, VOC_COLORMAP[got])
            wrec = ref.records(want, ref.label(want, conn), b)
            assert [(d['class'], d['label'], d['area'], d['bbox']) for d in regs] == \
                [(w[0] & 255, w[1], w[2], w[3:7]) for w in wrec]
            for d, w in zip(regs, wrec):
                g = region_geometry(w)
                assert d['centroid'] == list(g['centroid']) and d['angle'] == g['angle'] and d['sides'] == list(g['sides'])
        print('flip %s, connectivity %d: %s regions after cleaning' % (flip, conn, [len(r) for r in regions]))
    only = inference(m, photos, (64, 64), min_area=6, **kw)
    assert isinstance(only, list) and all(np.array_equal(a, ref.clean(r.astype(np.uint8), ref.label(r.astype(np.uint8), 8), 6))
                                          for a, r in zip(only, raw))
