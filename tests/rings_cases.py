"""The fixture masks of the outline tests (tests/test_polygons_cpu.py, tests/test_polygons_gpu.py): the smallest shapes at
which tracing rings can go wrong, and their reference labels and rings, computed once per (case, connectivity) and shared."""
import numpy as np

import regions_ref
import rings_ref


def _checker(h, w):
    yy, xx = np.mgrid[:h, :w]
    return ((yy + xx) % 2).astype(np.uint8)


def _serpentine(H, W):
    """a one-pixel-wide path (class 1 on 0) that runs right, down, back left, down, ...: one ring about twice its area"""
    m = np.zeros((H, W), np.uint8)
    for k, y in enumerate(range(1, H - 1, 2)):
        m[y, 1:W - 1] = 1
        if y + 2 < H - 1:
            m[y + 1, W - 2 if k % 2 == 0 else 1] = 1
    return m


def _nested(n):
    yy, xx = np.mgrid[:n, :n]
    d = np.minimum(np.minimum(yy, xx), np.minimum(n - 1 - yy, n - 1 - xx))
    return ((d // 2) % 2).astype(np.uint8) * 3          # square rings two pixels thick: a ring inside a hole inside a ring


def _build():
    diag = np.zeros((4, 4), np.uint8)
    diag[1, 1] = diag[2, 2] = 1
    hole2 = np.ones((5, 6), np.uint8)
    hole2[2, 2:4] = 0                                   # the hole ring's smallest edge lies mid-way along a straight run
    c255 = np.zeros((5, 5), np.uint8)
    c255[1:4, 1:4] = 255
    c255[2, 2] = 0
    ragged = [np.random.RandomState(seed).randint(0, 3, hw).astype(np.uint8)
              for seed, hw in ((11, (1, 1)), (12, (7, 3)), (13, (33, 65)), (14, (37, 70)))]
    return {
        '1x1': [np.full((1, 1), 7, np.uint8)],
        '1x7': [np.array([[0, 0, 1, 1, 1, 0, 2]], np.uint8)],
        '5x1': [np.array([[1], [1], [0], [1], [1]], np.uint8)],
        'checker2': [_checker(2, 2)],
        'checker6': [_checker(6, 6)],
        'diagonal': [diag],
        'hole2': [hole2],
        'nested': [_nested(11)],
        'uniform33x65': [np.full((33, 65), 4, np.uint8)],
        'serpentine': [_serpentine(64, 96)],
        'class255': [c255],
        'ragged': ragged,
    }


CASES = _build()
NAMES = list(CASES)
_REF = {}


def reference(name, conn):
    """-> (masks, labels, (records, vertices, counts)) of a case; read-only, computed once"""
    key = (name, conn)
    if key not in _REF:
        masks = CASES[name]
        labs = [regions_ref.label(m, conn) for m in masks]
        for a in masks + labs:
            a.setflags(write=False)
        _REF[key] = (masks, labs, rings_ref.device_arrays(masks, labs, conn))
    return _REF[key]


def check_invariants(masks, labs, conn, records, vertices):
    """the definition's own consequences, for rings in the device's format (ref-independent: only labels are used): every
    component's rings rasterise back to its pixel set, their signed areas add up to its area, it has 1 + holes rings, the
    outer ring comes first and alone has hole = 0, segments alternate, counts are even and >= 4"""
    by = {}
    for head, label, start, first, count, hole in records:
        assert count >= 4 and count % 2 == 0
        v = vertices[first:first + count]
        horiz = [v[i][1] == v[(i + 1) % count][1] for i in range(count)]
        assert all((v[i][0] == v[(i + 1) % count][0]) != horiz[i] for i in range(count)), 'a segment is horizontal or vertical'
        assert all(horiz[i] != horiz[(i + 1) % count] for i in range(count)), 'segments alternate'
        assert (rings_ref.area2(v) > 0) == (hole == 0)
        assert (start == 4 * label) == (hole == 0)
        by.setdefault((head >> 8, label), []).append((hole, v, head & 255))
    seen = 0
    for b, (m, lab) in enumerate(zip(masks, labs)):
        H, W = m.shape
        for label in np.unique(lab).tolist():
            rings = by[(b, label)]
            comp = lab == label
            assert [r[0] for r in rings] == [0] + [1] * (len(rings) - 1)
            assert all(r[2] == int(m[label // W, label % W]) for r in rings)
            assert np.array_equal(rings_ref.rasterise([r[1] for r in rings], H, W), comp)
            assert sum(rings_ref.area2(r[1]) for r in rings) == 2 * int(comp.sum())
            assert len(rings) == 1 + rings_ref.holes(comp, conn)
            seen += len(rings)
    assert seen == len(records)
