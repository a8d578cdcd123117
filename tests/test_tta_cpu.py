"""Test-time ensembling, host side: the three entry points are declared and exported, their host-side refusals, the scale
rule, the validation of inference(scales=, flip=) and the two command lines.  No GPU needed."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

from pytorch_segmentation_amd import _lib
from pytorch_segmentation_amd.csrc import build as csrc_build

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('pseg_image_preprocess_views', 'pseg_softmax_views', 'pseg_seg_decode_ensemble')


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


@pytest.mark.skipif(__import__('torch').cuda.is_available(), reason='uses made-up device addresses: host-side checks only')
def test_host_side_refusals(lib):
    """Every case is refused before any launch, so the made-up addresses are never dereferenced."""
    A, MIS = 0x7f0000000000, 0x7f0000000004

    def refused(name, *args, match):
        with pytest.raises(_lib.PsegError, match=match):
            _lib.call(name, *args)

    soft = lambda C=21, pairs=0, prob=A, off=0, cap=1 << 30: ('pseg_softmax_views', A, 2, pairs, C, 8, 8, prob, off, cap, None)
    refused(*soft(C=257), match='softmax.*257')
    refused(*soft(C=0), match='softmax.*0 classes')
    refused(*soft(pairs=2), match='unknown flag bits')
    refused(*soft(prob=MIS), match='16-byte aligned')
    refused(*soft(off=6), match='16-byte aligned')
    refused(*soft(cap=2 * 8 * 8 * 24 - 1), match='leaves the buffer')

    ens = lambda S=3, C=21, rgb=None, lut=None, prob=A: ('pseg_seg_decode_ensemble', prob, 1 << 20, A, S, 2, C, A, 4096, 64, 64,
                                                           A, rgb, lut, None)
    refused(*ens(S=0), match='seg.*0 maps')
    refused(*ens(S=9), match='seg.*9 maps')
    refused(*ens(C=257), match='seg.*257')
    refused(*ens(rgb=A), match='rgb and lut come together')
    refused(*ens(lut=A), match='rgb and lut come together')
    refused(*ens(prob=MIS), match='16-byte aligned')

    pre = lambda mask=1, rows=2: ('pseg_image_preprocess_views', A, 4096, A, rows, mask, 1, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, A, 8, 8,
                                  None)
    refused(*pre(mask=2), match='image.*unknown flag bits')
    refused(*pre(mask=3), match='image.*unknown flag bits')
    refused(*pre(rows=0), match='image.*rows')
    refused(*pre(rows=65536), match='image.*rows')


def test_scale_rule_and_merging():
    from pytorch_segmentation_amd.utils.inference import tta_sizes
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        assert tta_sizes(64, 64, (0.5, 1, 1.5)) == [(32, 32), (64, 64), (96, 96)]
        assert tta_sizes(64, 96, (0.1,)) == [(32, 32)]                  # never below 32
        assert tta_sizes(320, 512, (0.75, 1.25)) == [(224, 384), (384, 640)]
    with pytest.warns(RuntimeWarning, match='merged'):
        assert tta_sizes(64, 64, (1.0, 1.01)) == [(64, 64)]


def test_inference_rejects_bad_scales():
    import torch
    from pytorch_segmentation_amd.utils import inference
    model = torch.nn.Conv2d(3, 2, 1)
    photo = [np.zeros((4, 4, 3), np.uint8)]
    with pytest.raises(ValueError, match='finite and > 0'):
        inference(model, photo, scales=[0])
    with pytest.raises(ValueError, match='finite and > 0'):
        inference(model, photo, scales=[float('nan')])
    with pytest.raises(ValueError, match='finite and > 0'):
        inference(model, photo, scales=[1.0, float('inf')])
    with pytest.raises(ValueError, match='at most 8'):
        inference(model, photo, (64, 64), scales=[0.5 * k for k in range(1, 10)])
    with pytest.raises(ValueError, match='empty'):
        inference(model, photo, scales=[])
    # eight distinct sizes pass the validation and reach the device check
    with pytest.raises(RuntimeError, match='HIP path'):
        inference(model, photo, (64, 64), scales=[0.5 * k for k in range(1, 9)], flip=True)
    assert inference(model, [], scales=(0.5, 1.0), flip=True) == []


def test_predict_mask_ensemble_is_exported():
    import pytorch_segmentation_amd.utils as u
    assert callable(u.predict_mask_ensemble) and 'predict_mask_ensemble' in u.__all__


def test_cli_help_lists_the_flags():
    for script in ('inference.py', 'test.py'):
        out = subprocess.check_output([sys.executable, script, '--help'], cwd=REPO).decode()
        assert '--scales' in out and '--flip' in out, script


def test_cli_passes_the_keywords_only_when_given(tmp_path, monkeypatch):
    import torch
    sys.path.insert(0, REPO)
    import inference as cli
    from PIL import Image
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
    cli.main(base + ['--flip'])
    assert calls[-1]['flip'] is True and calls[-1]['scales'] is None
    cli.main(base + ['--scales', '0.5', '1.0'])
    assert calls[-1]['flip'] is False and list(calls[-1]['scales']) == [0.5, 1.0]
