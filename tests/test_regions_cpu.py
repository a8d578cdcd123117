"""Connected regions, host side: the plain reference (tests/regions_ref.py) against hand-written expectations,
region_geometry on the integer sums of analytic shapes, the command line's flag checks, and that inference()'s defaults
stay clear of the new code.  No GPU needed."""
import math
import os
import sys

import numpy as np
import pytest

import regions_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _m(rows):
    return np.array([[int(ch) for ch in r] for r in rows], dtype=np.uint8)


def test_reference_labels_by_hand():
    m = _m(['1100',
            '0010',
            '0011'])
    # 4-connectivity: {0, 1}; the zeros {2, 3, 7}; the zeros {4, 5, 8, 9}; the ones {6, 10, 11}
    assert ref.label(m, 4).tolist() == [[0, 0, 2, 2], [4, 4, 6, 2], [4, 4, 6, 6]]
    # 8-connectivity: the ones join diagonally (1 - 6 - 11), and so do the zeros (2 - 5 across the 1/6 diagonal)
    assert ref.label(m, 8).tolist() == [[0, 0, 2, 2], [2, 2, 0, 2], [2, 2, 0, 0]]


def test_reference_records_by_hand():
    m = _m(['22',
            '02',
            '00'])
    lab = ref.label(m, 4)
    assert lab.tolist() == [[0, 0], [2, 0], [2, 2]]
    # class 2: pixels (x, y) = (0,0), (1,0), (1,1); class 0: (0,1), (0,2), (1,2)
    assert ref.records(m, lab, photo=3) == [[3 * 256 + 2, 0, 3, 0, 0, 1, 1, 2, 1, 2, 1, 1],
                                            [3 * 256 + 0, 2, 3, 0, 1, 1, 2, 1, 5, 1, 2, 9]]


def test_reference_clean_hole_speck_and_cascade():
    # a hole (the 0 inside the 1s) takes the object's class; a speck (the 2) its surroundings'
    m = _m(['00000',
            '01110',
            '01010',
            '01110',
            '00002'])
    want = _m(['00000',
               '01110',
               '01110',
               '01110',
               '00000'])
    assert np.array_equal(ref.clean(m, ref.label(m, 4), min_area=2), want)
    # a cluster of specks: 3 sits under 2 sits under the large 1-region; 3 -> (2 is small too) -> 1
    m = _m(['1111',
            '1211',
            '1311',
            '1111'])
    assert np.array_equal(ref.clean(m, ref.label(m, 4), min_area=2), np.ones((4, 4), np.uint8))
    # min_area 0 and 1 change nothing
    for k in (0, 1):
        assert np.array_equal(ref.clean(m, ref.label(m, 4), min_area=k), m)


def test_reference_clean_corner_keeps_its_class_and_top_row_steps_left():
    # the corner component (one pixel of class 5) is small and keeps its class; the speck 7 in the top row has no pixel
    # above: it steps left, into the small corner component, which keeps 5 -- so 7 becomes 5
    m = _m(['5700',
            '0000'])
    want = _m(['5500',
               '0000'])
    assert np.array_equal(ref.clean(m, ref.label(m, 4), min_area=2), want)


def test_reference_largest_only_ties_and_background():
    # two 1-regions of equal area: the first in raster order stays; background regions (class 0) are never dropped by
    # largest_only; the dropped region takes the class above its first pixel (0)
    m = _m(['11000',
            '00000',
            '00011',
            '22000'])
    want = _m(['11000',
               '00000',
               '00000',
               '22000'])
    assert np.array_equal(ref.clean(m, ref.label(m, 8), min_area=0, largest_only=True), want)


@pytest.mark.parametrize('a,b', [(1, 1), (7, 3), (20, 20), (301, 2), (5, 64)])
def test_region_geometry_of_pixel_rectangles(a, b):
    """An axis-aligned a x b pixel rectangle (a wide, b high) at an offset: exact integer sums in, sides a and b out, to
    1e-9.  With a >= b the principal axis is x: angle 0.  A tall rectangle is the same box told from its long side: angle
    pi/2 and the sides swapped."""
    from pytorch_segmentation_amd.utils.regions import region_geometry
    x0, y0 = 40000, 123
    xs, ys = range(x0, x0 + a), range(y0, y0 + b)
    sx, sy = b * sum(xs), a * sum(ys)
    rec = [0, 0, a * b, x0, y0, x0 + a - 1, y0 + b - 1, sx, sy, b * sum(x * x for x in xs), sum(xs) * sum(ys),
           a * sum(y * y for y in ys)]
    g = region_geometry(rec)
    assert abs(g['centroid'][0] - (x0 + (a - 1) / 2)) < 1e-9 and abs(g['centroid'][1] - (y0 + (b - 1) / 2)) < 1e-9
    if a >= b:
        assert abs(g['angle']) < 1e-9
        assert abs(g['sides'][0] - a) < 1e-9 and abs(g['sides'][1] - b) < 1e-9
    else:
        assert abs(abs(g['angle']) - math.pi / 2) < 1e-9
        assert abs(g['sides'][0] - b) < 1e-9 and abs(g['sides'][1] - a) < 1e-9


def test_region_geometry_of_a_diagonal():
    """n pixels on the main diagonal: mu20 = mu02 = mu11 = (n^2 - 1) / 12, so the axis is at 45 degrees, the long side is
    sqrt(2 n^2 - 1) and the short side 1."""
    from pytorch_segmentation_amd.utils.regions import region_geometry
    n = 9
    s1, s2 = sum(range(n)), sum(i * i for i in range(n))
    g = region_geometry([0, 0, n, 0, 0, n - 1, n - 1, s1, s1, s2, s2, s2])
    assert abs(g['angle'] - math.pi / 4) < 1e-9
    assert abs(g['sides'][0] - math.sqrt(2 * n * n - 1)) < 1e-9 and abs(g['sides'][1] - 1) < 1e-9


def test_cli_rejects_bad_flags(capsys):
    sys.path.insert(0, REPO)
    import inference as cli
    for argv in (['in', 'out', '--min-area', '-1'], ['in', 'out', '--connectivity', '6'], ['in', 'out', '--min-area', 'x'],
                 ['in', 'out', '--regions']):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2, argv
    capsys.readouterr()
    with pytest.raises(ValueError, match='min-area'):
        cli.run('in', 'out', [64, 64], 2, 'w.pt', min_area=-1)
    with pytest.raises(ValueError, match='connectivity'):
        cli.run('in', 'out', [64, 64], 2, 'w.pt', connectivity=6)


def test_inference_rejects_bad_region_arguments():
    import torch
    from pytorch_segmentation_amd.utils import inference
    model = torch.nn.Conv2d(3, 2, 1)
    with pytest.raises(ValueError, match='min_area'):
        inference(model, [np.zeros((4, 4, 3), np.uint8)], min_area=-1)
    with pytest.raises(ValueError, match='connectivity'):
        inference(model, [np.zeros((4, 4, 3), np.uint8)], connectivity=6)


def test_inference_defaults_stay_clear_of_the_region_ops(monkeypatch):
    """With min_area, connectivity, largest_only and regions at their defaults inference() neither imports utils/regions.py
    nor calls a region op: the ops are patched to raise, the module is taken out of sys.modules, and the stubbed decode
    route runs to its end."""
    import torch
    from pytorch_segmentation_amd import ops
    from pytorch_segmentation_amd.utils import inference as infer_mod_fn
    infer_mod = sys.modules['pytorch_segmentation_amd.utils.inference']     # the attribute of that name is the function

    def boom(*a, **k):
        raise AssertionError('a region op ran on the default route')

    for name in ('mask_label', 'mask_regions', 'mask_clean'):
        monkeypatch.setattr(ops, name, boom)
    monkeypatch.delitem(sys.modules, 'pytorch_segmentation_amd.utils.regions', raising=False)
    monkeypatch.setattr(infer_mod, '_postprocess', boom)

    class Stop(Exception):
        pass

    seen = {}

    def fake_decode(logits, table, npix_total, lut=None, out=None):
        seen['decode'] = (lut is not None, out.numel(), npix_total)
        raise Stop

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(1))

    # the device route, stubbed: the parameter claims a GPU, staging and kernels are replaced
    monkeypatch.setattr(infer_mod, '_forward', lambda model, x, half: torch.zeros(1, 2, 4, 4))
    monkeypatch.setattr(ops, 'image_preprocess', lambda *a, **k: torch.zeros(1, 3, 4, 4))
    monkeypatch.setattr(ops, 'seg_decode', fake_decode)
    real_empty = torch.empty

    def cpu_empty(*a, **k):
        k.pop('pin_memory', None)
        k.pop('device', None)
        return real_empty(*a, **k)

    class FakeDevice:
        type = 'cuda'

    class P:
        device = FakeDevice()

    monkeypatch.setattr(Model, 'parameters', lambda self: iter([P()]))
    monkeypatch.setattr(torch, 'empty', cpu_empty)
    monkeypatch.setattr(torch.Tensor, 'to', lambda self, *a, **k: self)
    with pytest.raises(Stop):
        infer_mod_fn(Model(), [np.zeros((5, 6, 3), np.uint8)], (4, 4), colors=np.zeros((2, 3), np.uint8))
    assert seen['decode'] == (True, 4 * 30, 30)         # the palette went to the decode: the default route, unchanged
    assert 'pytorch_segmentation_amd.utils.regions' not in sys.modules
