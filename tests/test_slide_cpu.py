"""Sliding-window inference, host side: the two entry points are declared and exported, the window grid and the working
size against a walked restatement (tests/slide_ref.py), the host-side refusals of both entry points and of
inference(slide=True), and the two command lines.  No GPU needed."""
import importlib.util
import os
import sys
import warnings

import numpy as np
import pytest

import slide_ref
from pytorch_segmentation_amd import _lib
from pytorch_segmentation_amd.csrc import build as csrc_build

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('pseg_image_preprocess_windows', 'pseg_seg_decode_windows')


@pytest.fixture(scope='module')
def lib():
    csrc_build.build(verbose=False)
    return _lib.load()


def test_entry_points_declared_and_exported(lib):
    protos = _lib.parse_header()
    for name in NEW:
        assert name in protos, name
        assert hasattr(lib, name), name
    assert _lib.abi_version_of_header() == 14 == lib.pseg_abi_version()


# window 32 x 48, stride 22 x 32 (the GPU tests' grid) and the default stride of a 64 x 64 window
GRID_CASES = [
    # (Hs, Ws, h, w, sy, sx)
    (20, 30, 32, 48, 22, 32),        # smaller than the window along both axes: one window
    (32, 48, 32, 48, 22, 32),        # equal
    (33, 49, 32, 48, 22, 32),        # one pixel larger: a second window shifted back by all but one pixel
    (1, 1, 32, 48, 22, 32),
    (32 + 22, 48 + 2 * 32, 32, 48, 22, 32),     # exact multiples of the stride beyond the window
    (75, 100, 32, 48, 22, 32),       # Hs - h = 43, Ws - w = 52: not multiples, the last window is shifted
    (77, 117, 32, 48, 22, 32),       # three covering windows along each axis
    (97, 61, 32, 48, 22, 32),
    (20, 117, 32, 48, 22, 32),       # smaller along one axis only
    (100, 130, 64, 64, 43, 43),
    (64, 64, 64, 64, 43, 43),
    (40, 150, 64, 64, 43, 43),
    (200, 200, 64, 64, 32, 32),      # the smallest stride: half the window
    (200, 200, 64, 64, 64, 64),      # the largest: no overlap but the shifted last window's
    (65535, 70, 512, 64, 342, 43),
]


@pytest.mark.parametrize('case', GRID_CASES)
def test_window_grid_against_the_walk(case):
    from pytorch_segmentation_amd.utils.inference import window_grid
    Hs, Ws, h, w, sy, sx = case
    origins, (ny, nx) = window_grid(Hs, Ws, h, w, sy, sx)
    want, (wny, wnx) = slide_ref.grid(Hs, Ws, h, w, sy, sx)
    assert origins == want and (ny, nx) == (wny, wnx) and len(origins) == ny * nx
    assert ny == -(-max(Hs - h, 0) // sy) + 1 and nx == -(-max(Ws - w, 0) // sx) + 1
    for y0, x0 in origins:                                   # never hung over the edge of an image that holds a window
        assert 0 <= y0 <= max(Hs - h, 0) and 0 <= x0 <= max(Ws - w, 0)
    for size, win, st in ((Hs, h, sy), (Ws, w, sx)):         # every pixel covered by between 1 and 3 windows per axis
        cov = slide_ref.coverage(size, win, st)
        assert min(cov) >= 1 and max(cov) <= 3, (size, win, st, min(cov), max(cov))
    assert max(slide_ref.coverage(77, 32, 22)) == 3 and max(slide_ref.coverage(117, 48, 32)) == 3


def test_work_size_and_stride_rule():
    from pytorch_segmentation_amd import ops
    from pytorch_segmentation_amd.utils.inference import slide_strides, work_size
    for H, W in ((1, 1), (37, 53), (75, 100), (1024, 2048), (3, 65535)):
        for s in (0.01, 0.25, 0.5, 0.75, 1.0, 1.25, 1.5):
            assert work_size(H, W, s) == slide_ref.work_size(H, W, s)
        assert work_size(H, W, 1.0) == (H, W)
    assert work_size(75, 100, 0.5) == (38, 50) and work_size(1, 1, 0.1) == (1, 1) and work_size(5, 5, 0.5) == (3, 3)
    for win in (1, 2, 3, 32, 48, 64, 511, 512):
        lo, hi, default = ops.window_stride_limits(win)
        assert (lo, hi, default) == (-(-win // 2), win, -(-2 * win // 3)) and lo <= default <= hi
    assert slide_strides(64, 96) == (43, 64)                 # (sy, sx) of a window h = 64, w = 96
    assert slide_strides(64, 96, (48, 32)) == (32, 48)       # stride is given as (sw, sh)
    for bad in ((47, 32), (48, 31), (97, 64), (96, 65)):
        with pytest.raises(ValueError, match='stride'):
            slide_strides(64, 96, bad)


def test_scales_merge_only_when_every_photo_agrees():
    from pytorch_segmentation_amd.utils.inference import slide_scales
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        assert slide_scales([(10, 10), (100, 100)], (1.0, 0.5)) == [[(10, 10), (100, 100)], [(5, 5), (50, 50)]]
        # 1.0 and 1.04 give the 10 x 10 photo one size but not the 100 x 100 one: kept
        assert len(slide_scales([(10, 10), (100, 100)], (1.0, 1.04))) == 2
    with pytest.warns(RuntimeWarning, match='merged'):
        assert slide_scales([(10, 10), (12, 12)], (1.0, 1.04)) == [[(10, 10), (12, 12)]]
    with pytest.raises(ValueError, match='65535'):
        slide_scales([(40000, 10)], (2.0,))


@pytest.mark.skipif(__import__('torch').cuda.is_available(), reason='uses made-up device addresses: host-side checks only')
def test_host_side_refusals(lib):
    """Every case is refused before any launch, so the made-up addresses are never dereferenced."""
    A, MIS = 0x7f0000000000, 0x7f0000000004

    def refused(name, *args, match):
        with pytest.raises(_lib.PsegError, match=match):
            _lib.call(name, *args)

    def dec(S=2, C=21, h=32, w=48, sy=22, sx=32, rgb=None, lut=None, prob=A, groups=A, table=A, mask=A, Hmax=64, Wmax=64):
        return ('pseg_seg_decode_windows', prob, 1 << 20, groups, S, 2, C, h, w, sy, sx, table, 4096, Hmax, Wmax, mask, rgb, lut,
                None)

    for null in ('prob', 'groups', 'table', 'mask'):
        refused(*dec(**{null: None}), match='seg_decode_windows: null pointer')
    refused(*dec(S=0), match='seg_decode_windows: 0 scales')
    refused(*dec(S=9), match='seg_decode_windows: 9 scales')
    refused(*dec(C=0), match='seg_decode_windows: 0 classes')
    refused(*dec(C=257), match='seg_decode_windows: 257 classes')
    refused(*dec(sy=15), match='seg_decode_windows: stride 15x32')         # below ceil(32 / 2)
    refused(*dec(sy=33), match='seg_decode_windows: stride 33x32')         # above the window
    refused(*dec(sx=23), match='seg_decode_windows: stride 22x23')
    refused(*dec(sx=49), match='seg_decode_windows: stride 22x49')
    refused(*dec(h=33, sy=16), match='seg_decode_windows: stride 16x32')   # ceil(33 / 2) = 17
    refused(*dec(sy=0), match='seg_decode_windows: stride')
    refused(*dec(h=0), match='seg_decode_windows: window size 0x48')
    refused(*dec(w=-1), match='seg_decode_windows: window size')
    refused(*dec(Hmax=0), match='seg_decode_windows: largest image')
    refused(*dec(rgb=A), match='rgb and lut come together')
    refused(*dec(lut=A), match='rgb and lut come together')
    refused(*dec(prob=MIS), match='16-byte aligned')
    # the limits themselves pass the stride check and reach the next one
    refused(*dec(sy=16, sx=24, Hmax=0), match='largest image')
    refused(*dec(sy=32, sx=48, Hmax=0), match='largest image')

    def pre(mask=1, rows=2, oh=8, ow=8, src=A, table=A, out=A, nbytes=4096):
        return ('pseg_image_preprocess_windows', src, nbytes, table, rows, mask, 1, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, out, oh, ow, None)

    for null in ('src', 'table', 'out'):
        refused(*pre(**{null: None}), match='image_preprocess_windows: null pointer')
    refused(*pre(mask=2), match='image_preprocess_windows: unknown flag bits')
    refused(*pre(rows=0), match='image_preprocess_windows: 0 table rows')
    refused(*pre(rows=65536), match='image_preprocess_windows: 65536 table rows')
    refused(*pre(oh=0), match='image_preprocess_windows: window size')
    refused(*pre(ow=65536), match='image_preprocess_windows: window size')
    refused(*pre(nbytes=2), match='holds no pixel')


def test_inference_argument_checks():
    import torch
    from pytorch_segmentation_amd.utils import inference
    model = torch.nn.Conv2d(3, 2, 1)
    photo = [np.zeros((40, 50, 3), np.uint8)]
    with pytest.raises(ValueError, match='multiples of 32'):
        inference(model, photo, (64, 48), slide=True)
    with pytest.raises(ValueError, match='multiples of 32'):
        inference(model, photo, (0, 64), slide=True)
    with pytest.raises(ValueError, match='stride'):
        inference(model, photo, (64, 64), slide=True, stride=(31, 32))
    with pytest.raises(ValueError, match='stride'):
        inference(model, photo, (64, 64), slide=True, stride=(64, 65))
    with pytest.raises(ValueError, match='at most 8'):
        inference(model, photo, (64, 64), slide=True, scales=[0.5 + 0.25 * k for k in range(9)])
    with pytest.raises(ValueError, match='finite and > 0'):
        inference(model, photo, (64, 64), slide=True, scales=[0.0])
    with pytest.raises(ValueError, match='empty'):
        inference(model, photo, (64, 64), slide=True, scales=[])
    with pytest.raises(ValueError, match='window_batch'):
        inference(model, photo, (64, 64), slide=True, window_batch=0)
    with pytest.raises(ValueError, match='slide=True'):
        inference(model, photo, (64, 64), stride=(43, 43))
    with pytest.raises(ValueError, match='slide=True'):
        inference(model, photo, (64, 64), window_batch=4)
    # valid arguments (the limits of the stride, eight scales) reach the device check
    for kw in ({}, {'stride': (32, 32)}, {'stride': (64, 64)}, {'scales': [0.5 + 0.25 * k for k in range(8)], 'flip': True},
               {'window_batch': 1}):
        with pytest.raises(RuntimeError, match='HIP path'):
            inference(model, photo, (64, 64), slide=True, **kw)
    assert inference(model, [], (64, 64), slide=True) == []


def test_predict_mask_windows_is_exported():
    import pytorch_segmentation_amd.utils as u
    assert callable(u.predict_mask_windows) and 'predict_mask_windows' in u.__all__


def _script(name):
    spec = importlib.util.spec_from_file_location('pseg_slide_cli_' + name, os.path.join(REPO, name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_evaluation_cli_parser(capsys):
    cli = _script('test')
    opt = cli.parse_args(['val.json'])
    assert opt.window is None and opt.stride is None
    opt = cli.parse_args(['val.json', '-s', '128', '96', '--window', '64', '32', '--stride', '43', '22', '--flip'])
    assert opt.window == [64, 32] and opt.stride == [43, 22] and opt.img_size == [128, 96] and opt.flip
    assert cli.parse_args(['val.json', '--window', '64', '64']).stride is None
    for bad in (['val.json', '--stride', '43', '43'], ['val.json', '--window', '64'], ['val.json', '--window', '64', 'x']):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)
    assert '--stride needs --window' in capsys.readouterr().err
    with pytest.raises(ValueError, match='stride belongs to window'):
        cli.test(__import__('torch').nn.Identity(), None, stride=(43, 43))


def test_inference_cli_passes_the_keywords_only_when_given(tmp_path, monkeypatch, capsys):
    import torch
    from PIL import Image
    cli = _script('inference')
    img_dir, out_dir = tmp_path / 'in', tmp_path / 'out'
    img_dir.mkdir()
    Image.fromarray(np.zeros((5, 7, 3), np.uint8)).save(str(img_dir / 'a.png'))
    calls = []

    class Stub(torch.nn.Module):
        def __init__(self, nc):
            super().__init__()

        def load_state_dict(self, sd):
            pass

        def cuda(self):
            return self

    def fake_inference(model, imgs, img_size, **kw):
        calls.append(kw)
        masks = [np.ones(im.shape[:2], np.int64) for im in imgs]
        return masks, [kw['colors'][m] for m in masks]

    monkeypatch.setitem(cli.MODELS, 'unet', Stub)
    monkeypatch.setattr(cli, 'inference', fake_inference)
    monkeypatch.setattr(cli.torch, 'load', lambda path, map_location=None: {'model': {}})
    base = [str(img_dir), str(out_dir), '-s', '64', '64', '--weights', 'w.pt', '--model', 'unet']
    cli.main(base)
    assert sorted(calls[-1]) == ['bgr', 'colors', 'half', 'norm']            # exactly the old keywords
    cli.main(base + ['--slide'])
    assert calls[-1]['slide'] is True and calls[-1]['stride'] is None and calls[-1]['window_batch'] is None
    assert 'scales' not in calls[-1] and 'flip' not in calls[-1]
    cli.main(base + ['--slide', '--stride', '43', '32', '--window-batch', '6', '--scales', '0.5', '1.0', '--flip'])
    assert calls[-1]['stride'] == (43, 32) and calls[-1]['window_batch'] == 6
    assert calls[-1]['flip'] is True and list(calls[-1]['scales']) == [0.5, 1.0]
    n = len(calls)
    for bad in (['--stride', '43', '43'], ['--window-batch', '4'], ['--slide', '--window-batch', '0'], ['--slide', '--stride', '43']):
        with pytest.raises(SystemExit):
            cli.main(base + bad)
    assert len(calls) == n
    assert 'need --slide' in capsys.readouterr().err
    with pytest.raises(ValueError, match='need --slide'):
        cli.run(str(img_dir), str(out_dir), [64, 64], 2, 'w.pt', model_name='unet', stride=(43, 43))
