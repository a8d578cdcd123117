"""Outlines of mask regions on the device (csrc/polygons.hip) against the sequential tracer (tests/rings_ref.py): ring
records, vertices and counts must be EQUAL, word for word, for 4- and 8-connectivity, on the fixtures of
tests/rings_cases.py; then what holds without any reference -- the rings rasterise back to the components, their signed
areas add up to pseg_mask_regions' area word, and there is one ring per hole plus one."""
import numpy as np
import pytest
import torch

import rings_cases as cases
import rings_ref

pytestmark = pytest.mark.gpu

SENTINEL = -12345


@pytest.fixture(scope='module')
def ops():
    from pytorch_segmentation_amd import ops
    return ops


def _pack(masks):
    from pytorch_segmentation_amd.utils.regions import packed_table
    table, npix, max_hw = packed_table([m.shape for m in masks])
    flat = np.concatenate([m.reshape(-1) for m in masks])
    return torch.from_numpy(flat).cuda(), torch.from_numpy(table).cuda(), table, npix, max_hw


def _buffers(cap, guard=8):
    rings = torch.full((cap // 4 + guard, 6), SENTINEL, dtype=torch.int64, device='cuda')
    verts = torch.full((cap + guard, 2), SENTINEL, dtype=torch.int32, device='cuda')
    return rings, verts


def _run(ops, dmask, labels, dtable, npix, max_hw, conn, cap):
    """one call into sentinel-filled buffers -> (records, vertices, counts) as lists, after checking that nothing past the
    counts was written"""
    rings, verts = _buffers(cap)
    _, _, counts = ops.mask_rings(dmask, labels, dtable, npix, max_hw, conn, cap, rings=rings, vertices=verts)
    n = counts.cpu().tolist()
    rings, verts = rings.cpu().numpy(), verts.cpu().numpy()
    nr, nv = (n[1], n[2]) if n[0] <= cap else (0, 0)
    assert (rings[nr:] == SENTINEL).all() and (verts[nv:] == SENTINEL).all()
    return rings[:nr].tolist(), verts[:nv].tolist(), n


@pytest.mark.parametrize('conn', [4, 8])
@pytest.mark.parametrize('name', cases.NAMES)
def test_rings_equal_reference(ops, name, conn):
    masks, labs, (wrec, wverts, wcounts) = cases.reference(name, conn)
    dmask, dtable, table, npix, max_hw = _pack(masks)
    labels = ops.mask_label(dmask, dtable, npix, max_hw, conn)
    assert np.array_equal(labels.cpu().numpy(), np.concatenate([l.reshape(-1) for l in labs]))
    rec, verts, counts = _run(ops, dmask, labels, dtable, npix, max_hw, conn, wcounts[0])      # the exact need succeeds
    print('%s, connectivity %d: %s edges, rings, vertices' % (name, conn, counts))
    assert counts == wcounts
    assert rec == wrec, name
    assert verts == wverts, name
    # without the reference: round trip, holes, and the areas of the records call
    cases.check_invariants(masks, labs, conn, rec, verts)
    regions, count = ops.mask_regions(dmask, labels, dtable, npix, max_hw, len({(r[0] >> 8, r[1]) for r in rec}))
    area2 = {}
    for head, label, start, first, n, hole in rec:
        area2[(head >> 8, label)] = area2.get((head >> 8, label), 0) + rings_ref.area2(verts[first:first + n])
    regions = regions.cpu().numpy().tolist()
    assert int(count.item()) == len(area2)
    assert [(r[0] >> 8, r[1], 2 * r[2]) for r in regions] == [(b, l, a) for (b, l), a in sorted(area2.items())]
    # a larger capacity gives the same words (and leaves the rest alone: _run checks)
    assert _run(ops, dmask, labels, dtable, npix, max_hw, conn, min(4 * npix, wcounts[0] + 37)) == (rec, verts, counts)
    # what the shape is there to show
    if name == 'serpentine':
        path = [r for r in rec if r[0] & 255 == 1]
        assert len(path) == 1 and counts[0] > 2 * int(masks[0].sum())     # one ring, about twice as long as the area
    if name == 'checker6' and conn == 4:
        assert counts == [144, 36, 144]
    if name == 'uniform33x65':
        assert counts == [2 * (33 + 65), 1, 4] and verts == [[0, 0], [65, 0], [65, 33], [0, 33]]


@pytest.mark.parametrize('conn', [4, 8])
def test_capacity_one_below_the_need(ops, conn):
    """max_edges one below the need: counts = [need, -1, -1] and the sentinel-filled buffers are untouched; max_edges 0
    takes no buffers at all"""
    masks, labs, (wrec, wverts, wcounts) = cases.reference('ragged', conn)
    dmask, dtable, table, npix, max_hw = _pack(masks)
    labels = ops.mask_label(dmask, dtable, npix, max_hw, conn)
    rec, verts, counts = _run(ops, dmask, labels, dtable, npix, max_hw, conn, wcounts[0] - 1)
    assert counts == [wcounts[0], -1, -1] and rec == [] and verts == []
    _, _, c0 = ops.mask_rings(dmask, labels, dtable, npix, max_hw, conn, 0)
    assert c0.cpu().tolist() == [wcounts[0], -1, -1]
    rec, verts, counts = _run(ops, dmask, labels, dtable, npix, max_hw, conn, wcounts[0])
    assert (rec, verts, counts) == (wrec, wverts, wcounts)


@pytest.mark.parametrize('conn', [4, 8])
def test_bad_record_is_skipped(ops, conn):
    """the ragged batch with the 7 x 3 photo's extent leaving the buffer: no ring of that photo, the others' rings as
    before (their vertex offsets moved up), labels of the bad photo never read (they hold a sentinel), nothing written
    past the counts"""
    masks, labs, (wrec, wverts, wcounts) = cases.reference('ragged', conn)
    dmask, dtable, table, npix, max_hw = _pack(masks)
    bad = table.copy()
    bad[1, 0] = npix - 3
    dbad = torch.from_numpy(bad).cuda()
    labels = ops.mask_label(dmask, dbad, npix, max_hw, conn, out=torch.full((npix,), -7, dtype=torch.int32, device='cuda'))
    assert (labels[1:22] == -7).all()
    before = labels.clone()
    rec, verts, counts = _run(ops, dmask, labels, dbad, npix, max_hw, conn, wcounts[0])
    want_rec, want_verts = [], []
    for r in wrec:
        if r[0] >> 8 != 1:
            want_rec.append(r[:3] + [len(want_verts)] + r[4:])
            want_verts += wverts[r[3]:r[3] + r[4]]
    gone = len(rings_ref.edges(labs[1]))
    assert counts == [wcounts[0] - gone, len(want_rec), len(want_verts)]
    assert rec == want_rec and verts == want_verts
    assert torch.equal(labels, before) and np.array_equal(dmask.cpu().numpy(), np.concatenate([m.reshape(-1) for m in masks]))


def test_two_calls_give_identical_bytes(ops):
    masks, labs, (wrec, wverts, wcounts) = cases.reference('ragged', 8)
    dmask, dtable, table, npix, max_hw = _pack(masks)
    labels = ops.mask_label(dmask, dtable, npix, max_hw, 8)
    outs = []
    for _ in range(2):
        rings, verts = _buffers(wcounts[0])
        _, _, counts = ops.mask_rings(dmask, labels, dtable, npix, max_hw, 8, wcounts[0], rings=rings, vertices=verts)
        outs.append((rings.cpu().numpy().tobytes(), verts.cpu().numpy().tobytes(), counts.cpu().numpy().tobytes()))
    assert outs[0] == outs[1]


def test_argument_checks(ops):
    from pytorch_segmentation_amd._lib import PsegError
    dmask, dtable, table, npix, max_hw = _pack([np.zeros((3, 3), np.uint8)])
    labels = ops.mask_label(dmask, dtable, npix, max_hw, 8)
    with pytest.raises(PsegError, match='connectivity'):
        ops.mask_rings(dmask, labels, dtable, npix, max_hw, 6, 12)
    with pytest.raises(PsegError, match='2\\^31'):
        ops.mask_rings(dmask, labels, dtable, npix, (65535, 65535), 8, 12)
    with pytest.raises(AssertionError):
        ops.mask_rings(dmask, labels, dtable, npix, max_hw, 8, 4 * npix + 1)
    with pytest.raises(AssertionError):
        ops.mask_rings(dmask, labels.long(), dtable, npix, max_hw, 8, 12)


@pytest.mark.parametrize('conn', [4, 8])
def test_mask_polygons_groups_rings_and_repeats_once(ops, conn, monkeypatch):
    """utils.regions.mask_polygons: outer ring first, then the holes, per photo in label order; a first capacity that is too
    small costs exactly one more rings call"""
    from pytorch_segmentation_amd.utils import regions as R
    masks, labs, (wrec, wverts, wcounts) = cases.reference('ragged', conn)
    dmask, dtable, table, npix, max_hw = _pack(masks)
    calls = []
    real = ops.mask_rings
    monkeypatch.setattr(ops, 'mask_rings', lambda *a, **k: calls.append(a[6]) or real(*a, **k))
    for capacity, ncalls in ((16, [16, wcounts[0]]), (None, None), (wcounts[0], [wcounts[0]])):
        del calls[:]
        got = R.mask_polygons(dmask, dtable, max_hw, conn, capacity)
        assert ncalls is None or calls == ncalls
        assert len(calls) <= 2
        want = [{} for _ in masks]
        for head, label, start, first, n, hole in wrec:
            e = want[head >> 8].setdefault(label, {'label': label, 'class': head & 255, 'rings': []})
            e['rings'].append(wverts[first:first + n])
        for g, w in zip(got, want):
            assert [(p['label'], p['class'], [r.tolist() for r in p['rings']]) for p in g] == \
                [(w[k]['label'], w[k]['class'], w[k]['rings']) for k in sorted(w)]
            assert all(r.dtype == np.int32 and r.ndim == 2 and r.shape[1] == 2 for p in g for r in p['rings'])


def _tiny_model():
    from pytorch_segmentation_amd import models
    torch.manual_seed(3)
    return models.UNet(3).cuda().eval()


@pytest.mark.parametrize('route', ['single', 'flip', 'slide'])
def test_inference_end_to_end(ops, route):
    """inference(..., regions=True, polygons=True) on all three routes: every region's polygon rasterises back to exactly
    the pixels of its label in the returned mask; without polygons the call returns what it returned before, and the
    polygon call's dicts are those plus three keys"""
    import regions_ref
    from pytorch_segmentation_amd.utils import inference
    rng = np.random.RandomState(4)
    photos = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in ((50, 70), (64, 64))]
    m = _tiny_model()
    kw = {'single': {}, 'flip': {'flip': True}, 'slide': {'slide': True}}[route]
    for conn, k in ((8, 6), (4, 0)):
        plain_masks, plain = inference(m, photos, (64, 64), min_area=k, connectivity=conn, regions=True, **kw)
        masks, regions = inference(m, photos, (64, 64), min_area=k, connectivity=conn, regions=True, polygons=True, **kw)
        for b, (mask, regs, mask0, regs0) in enumerate(zip(masks, regions, plain_masks, plain)):
            assert np.array_equal(mask, mask0)
            m8 = mask.astype(np.uint8)
            lab = regions_ref.label(m8, conn)
            assert regs0 == [{key: d[key] for key in d0} for d, d0 in zip(regs, regs0)] and len(regs) == len(regs0)
            wrec = regions_ref.records(m8, lab, b)
            assert [(d['class'], d['label'], d['area'], d['bbox']) for d in regs0] == [(w[0] & 255, w[1], w[2], w[3:7]) for w in wrec]
            covered = np.zeros(mask.shape, np.int64)
            for d in regs:
                rings = [np.array(f).reshape(-1, 2) for f in d['polygon']]
                inside = rings_ref.rasterise(rings, *mask.shape)
                assert np.array_equal(inside, lab == d['label']) and (mask[inside] == d['class']).all()
                assert sum(rings_ref.area2(r) for r in rings) == 2 * d['area']
                assert len(rings) == 1 + rings_ref.holes(inside, conn)
                covered += inside
            assert (covered == 1).all()
        print('%s, connectivity %d: %s regions' % (route, conn, [len(r) for r in regions]))
