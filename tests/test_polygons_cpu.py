"""Outlines of mask regions, host side: the yardstick itself (tests/rings_ref.py must satisfy what the header's definition
implies, on every fixture of tests/rings_cases.py and both connectivities) and the host code of utils/regions.py -- ring
measures, the minimum-area rectangle, the region dicts with polygons, the COCO layout and the command line."""
import json
import math
import os
import sys

import numpy as np
import pytest

import rings_cases as cases
import rings_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('conn', [4, 8])
@pytest.mark.parametrize('name', cases.NAMES)
def test_reference_rings_satisfy_the_definition(name, conn):
    masks, labs, (records, vertices, counts) = cases.reference(name, conn)
    cases.check_invariants(masks, labs, conn, records, vertices)
    assert counts == [sum(len(rings_ref.edges(lab)) for lab in labs), len(records), len(vertices)]
    starts = [(r[0] >> 8, r[2]) for r in records]
    assert starts == sorted(starts)                                       # photo first, then raster
    for (head, label, start, first, count, hole), nxt in zip(records, records[1:] + [None]):
        assert first + count == (nxt[3] if nxt else len(vertices))       # contiguous, no gaps
    # the start is the smallest corner edge: re-derive the corner edges of every ring from the successor function alone
    for b, lab in enumerate(labs):
        W = lab.shape[1]
        pred = {rings_ref.successor(lab, e, conn): e for e in rings_ref.edges(lab)}
        assert len(pred) == len(rings_ref.edges(lab))                     # one successor, one predecessor
        for head, label, start, first, count, hole in records:
            if head >> 8 != b:
                continue
            ring, e = [], start
            while not ring or e != start:
                ring.append(e)
                e = rings_ref.successor(lab, e, conn)
            corners = [e for e in ring if pred[e] & 3 != e & 3]
            assert min(corners) == start and len(corners) == count
            y, x = divmod(start >> 2, W)
            assert list(vertices[first]) == [x + rings_ref.TAIL[start & 3][0], y + rings_ref.TAIL[start & 3][1]]


def test_reference_saddles_and_known_rings():
    two = cases.CASES['checker2'][0]                                      # [[0, 1], [1, 0]]
    _, _, (rec4, v4, n4) = cases.reference('checker2', 4)
    _, _, (rec8, v8, n8) = cases.reference('checker2', 8)
    assert n4 == [16, 4, 16] and [r[4] for r in rec4] == [4, 4, 4, 4]    # four unit squares
    assert n8 == [16, 2, 16] and [r[4] for r in rec8] == [8, 8]          # two rings through the centre vertex twice
    assert v8[:8] == [[0, 0], [1, 0], [1, 1], [2, 1], [2, 2], [1, 2], [1, 1], [0, 1]]
    # the 2-wide hole: its ring starts at a corner edge that is not its smallest edge
    _, labs, (rec, v, n) = cases.reference('hole2', 8)
    hole = [r for r in rec if r[5] == 1]
    assert len(hole) == 1 and hole[0][1] == 0
    smallest = min(e for e in rings_ref.edges(labs[0]) if e >> 2 in (1 * 6 + 2, 1 * 6 + 3) and e & 3 == 2)
    assert smallest == 4 * 8 + 2 and hole[0][2] > smallest
    assert hole[0][2] == 4 * 9 + 2                                        # pixel (3, 1), side S: where the ring turns west
    assert two.shape == (2, 2)


def test_ring_measures():
    from pytorch_segmentation_amd.utils.regions import ring_area2, ring_perimeter
    sq = np.array([[2, 3], [7, 3], [7, 6], [2, 6]], np.int32)
    assert ring_area2(sq) == 30 and ring_area2(sq[::-1]) == -30 and isinstance(ring_area2(sq), int)
    assert ring_perimeter(sq) == 16 and isinstance(ring_perimeter(sq), int)
    big = np.array([[0, 0], [65535, 0], [65535, 65535], [0, 65535]], np.int32)
    assert ring_area2(big) == 2 * 65535 * 65535                           # beyond int32: Python integers
    for name in ('nested', 'ragged'):
        _, _, (records, vertices, _) = cases.reference(name, 8)
        for r in records:
            v = vertices[r[3]:r[3] + r[4]]
            assert ring_area2(v) == rings_ref.area2(v)


def _inside(rect, pts, tol=1e-9):
    (cx, cy), (a, b), t = rect['center'], rect['size'], rect['angle']
    u, v = (math.cos(t), math.sin(t)), (-math.sin(t), math.cos(t))
    for x, y in pts:
        du, dv = (x - cx) * u[0] + (y - cy) * u[1], (x - cx) * v[0] + (y - cy) * v[1]
        assert abs(du) <= a / 2 + tol and abs(dv) <= b / 2 + tol, (x, y)


@pytest.mark.parametrize('a,b', [(1, 1), (7, 3), (3, 7), (301, 2)])
def test_min_area_rect_of_a_rectangle(a, b):
    from pytorch_segmentation_amd.utils.regions import min_area_rect
    pts = [(10, 20), (10 + a, 20), (10 + a, 20 + b), (10, 20 + b), (10 + a // 2, 20)]
    r = min_area_rect(pts)
    assert abs(r['size'][0] * r['size'][1] - a * b) < 1e-9
    assert abs(r['center'][0] - (10 + a / 2)) < 1e-9 and abs(r['center'][1] - (20 + b / 2)) < 1e-9
    assert -math.pi / 2 < r['angle'] <= math.pi / 2
    _inside(r, pts)


def test_min_area_rect_of_a_staircase_diamond():
    """the 45-degree diamond of pixels |x| + |y| <= n: its outline is a staircase whose hull is an octagon with four long
    diagonal edges; the best rectangle lies on one of them, so its angle is +-45 degrees, it contains every vertex, and it
    beats the bounding box"""
    from pytorch_segmentation_amd.utils.regions import convex_hull, min_area_rect
    import regions_ref
    n = 6
    yy, xx = np.mgrid[-n:n + 1, -n:n + 1]
    m = (abs(yy) + abs(xx) <= n).astype(np.uint8)
    lab = regions_ref.label(m, 4)
    ring = [r for r in rings_ref.trace(lab, 4) if m.reshape(-1)[r['label']] == 1][0]['vertices']
    r = min_area_rect(ring)
    hull = convex_hull(ring)
    assert abs(abs(r['angle']) - math.pi / 4) < 1e-12
    _inside(r, ring)
    # a side on a hull edge: some hull edge is parallel to the angle and lies on the rectangle's border
    u, v = (math.cos(r['angle']), math.sin(r['angle'])), (-math.sin(r['angle']), math.cos(r['angle']))
    on_border = False
    for p, q in zip(hull, hull[1:] + hull[:1]):
        d = [((pt[0] - r['center'][0]) * v[0] + (pt[1] - r['center'][1]) * v[1]) for pt in (p, q)]
        par = abs((q[0] - p[0]) * v[0] + (q[1] - p[1]) * v[1]) < 1e-9
        on_border |= par and abs(abs(d[0]) - r['size'][1] / 2) < 1e-9 and abs(abs(d[1]) - r['size'][1] / 2) < 1e-9
    assert on_border
    xs, ys = [p[0] for p in ring], [p[1] for p in ring]
    box = (max(xs) - min(xs)) * (max(ys) - min(ys))
    assert r['size'][0] * r['size'][1] <= box + 1e-9 and r['size'][0] * r['size'][1] < 0.75 * box
    # exact value: the staircase's corners reach |x'| + |y'| = n + 1 around the centre of the diamond
    assert abs(r['size'][0] * r['size'][1] - 2.0 * (n + 1) ** 2) < 1e-9


def test_min_area_rect_hull_is_exact_and_degenerate_inputs():
    from pytorch_segmentation_amd.utils.regions import convex_hull, min_area_rect
    k = 3037000499                                                         # cross products beyond 2^63: Python integers
    assert convex_hull([(0, 0), (k, k), (2 * k, 2 * k), (2 * k, 2 * k + 1)]) == [(0, 0), (2 * k, 2 * k), (2 * k, 2 * k + 1)]
    assert convex_hull([(0, 0), (2, 2), (4, 4), (1, 1)]) == [(0, 0), (4, 4)]
    r = min_area_rect([(0, 0), (2, 2), (4, 4)])
    assert abs(r['size'][0] - math.hypot(4, 4)) < 1e-12 and r['size'][1] == 0.0
    assert min_area_rect([(5, 6)]) == {'center': (5.0, 6.0), 'size': (0.0, 0.0), 'angle': 0.0}
    # ties go to the first hull edge: a square's four rectangles are equal; the first edge leaves (0, 0)
    sq = min_area_rect([(0, 0), (4, 0), (4, 4), (0, 4)])
    hull = convex_hull([(0, 0), (4, 0), (4, 4), (0, 4)])
    first = math.atan2(hull[1][1] - hull[0][1], hull[1][0] - hull[0][0])
    first = first - math.pi if first > math.pi / 2 else first + math.pi if first <= -math.pi / 2 else first
    assert sq['angle'] == first


def _records_and_polygons(name, conn):
    """host-side stand-ins for mask_regions / mask_polygons, from the references"""
    import regions_ref
    masks, labs, (rec, verts, _) = cases.reference(name, conn)
    records = sum([regions_ref.records(m, l, b) for b, (m, l) in enumerate(zip(masks, labs))], [])
    polys = [{} for _ in masks]
    for head, label, start, first, count, hole in rec:
        e = polys[head >> 8].setdefault(label, {'label': label, 'class': head & 255, 'rings': []})
        e['rings'].append(np.array(verts[first:first + count], np.int32))
    return masks, records, [[p[k] for k in sorted(p)] for p in polys]


def test_region_dicts_with_and_without_polygons():
    from pytorch_segmentation_amd.utils.regions import min_area_rect, region_dicts, region_geometry
    masks, records, polys = _records_and_polygons('ragged', 8)
    plain = region_dicts(np.array(records, np.int64), len(masks))
    # without polygons: today's output, key for key
    for b, regs in enumerate(plain):
        mine = [r for r in records if r[0] >> 8 == b]
        assert len(regs) == len(mine)
        for d, r in zip(regs, mine):
            g = region_geometry(r)
            assert d == {'class': r[0] & 255, 'area': r[2], 'bbox': r[3:7], 'centroid': list(g['centroid']), 'angle': g['angle'],
                         'sides': list(g['sides']), 'label': r[1]}
            assert list(d) == ['class', 'area', 'bbox', 'centroid', 'angle', 'sides', 'label']
    full = region_dicts(np.array(records, np.int64), len(masks), polys)
    json.dumps(full)                                                       # plain Python numbers
    for b, (regs, base) in enumerate(zip(full, plain)):
        for d, d0, p in zip(regs, base, polys[b]):
            assert {k: d[k] for k in d0} == d0 and set(d) - set(d0) == {'polygon', 'perimeter', 'min_rect'}
            assert d['label'] == p['label'] and d['class'] == p['class']
            assert d['polygon'] == [ring.reshape(-1).tolist() for ring in p['rings']]
            assert sum(rings_ref.area2(np.array(f).reshape(-1, 2)) for f in d['polygon']) == 2 * d['area']
            rect = min_area_rect(p['rings'][0])
            assert d['min_rect'] == {'center': list(rect['center']), 'size': list(rect['size']), 'angle': rect['angle']}
            x0, y0, x1, y1 = d['bbox']
            assert d['min_rect']['size'][0] * d['min_rect']['size'][1] <= (x1 - x0 + 1) * (y1 - y0 + 1) + 1e-9
            assert d['perimeter'] >= 2 * ((x1 - x0 + 1) + (y1 - y0 + 1))


def test_coco_layout_loads_through_the_dataset(tmp_path):
    from PIL import Image
    from pytorch_segmentation_amd.utils.datasets import CocoDataset
    from pytorch_segmentation_amd.utils.regions import coco_annotations, region_dicts
    masks, records, polys = _records_and_polygons('ragged', 8)
    dicts = region_dicts(np.array(records, np.int64), len(masks), polys)
    names = ['p%d.png' % b for b in range(len(masks))]
    found, sizes = dict(zip(names, dicts)), {n: m.shape for n, m in zip(names, masks)}
    coco = coco_annotations(found, sizes, 3)
    assert [c['id'] for c in coco['categories']] == [0, 1]
    assert [(i['file_name'], i['height'], i['width']) for i in coco['images']] == [(n, m.shape[0], m.shape[1]) for n, m in zip(names, masks)]
    want = [(b, d) for b, regs in enumerate(dicts) for d in regs if d['class'] >= 1]
    assert len(coco['annotations']) == len(want)
    for ann, (b, d) in zip(coco['annotations'], want):
        x0, y0, x1, y1 = d['bbox']
        assert ann == {'id': ann['id'], 'image_id': b, 'category_id': d['class'] - 1, 'segmentation': [d['polygon'][0]],
                       'area': d['area'], 'bbox': [x0, y0, x1 - x0 + 1, y1 - y0 + 1], 'iscrowd': 0}
    for n, m in zip(names, masks):
        Image.fromarray(np.zeros(m.shape + (3,), np.uint8)).save(str(tmp_path / n))
    path = tmp_path / 'pred.json'
    path.write_text(json.dumps(coco))
    ds = CocoDataset(str(path), img_size=[70, 37])
    assert ds.classes == ['background', 'class1', 'class2'] and len(ds) == len(masks)
    per_image = [len(anns) for _, anns in ds.data]
    assert per_image == [sum(1 for d in regs if d['class'] >= 1) for regs in dicts]
    img, seg = ds[3]                                                       # the 37 x 70 photo at its own size: it draws
    assert tuple(seg.shape) == (37, 70) and set(np.unique(seg.numpy()).tolist()) <= {0, 1, 2}


def test_cli_refuses_polygons_alone(capsys):
    sys.path.insert(0, REPO)
    import inference as cli
    with pytest.raises(SystemExit) as e:
        cli.main(['in', 'out', '--polygons'])
    assert e.value.code == 2
    assert '--polygons needs --regions or --coco' in capsys.readouterr().err
    with pytest.raises(ValueError, match='--polygons needs'):
        cli.run('in', 'out', [64, 64], 2, 'w.pt', polygons=True)


def test_inference_refuses_polygons_without_regions():
    import torch
    from pytorch_segmentation_amd.utils import inference
    with pytest.raises(ValueError, match='polygons'):
        inference(torch.nn.Conv2d(3, 2, 1), [np.zeros((4, 4, 3), np.uint8)], polygons=True)
