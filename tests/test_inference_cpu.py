"""Batched inference, host side: the VOC palette as the reference builds it, the inference.py command line and its file
selection (the decoder stubbed out), the reference's import paths.  No GPU needed."""
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_voc_palette_as_decoded_rgb():
    """VOC_COLORMAP rows are [b, g, r] (the reference writes them with cv2.imwrite), so row[::-1] is the RGB a decoded
    PNG shows: the standard VOC colours."""
    from pytorch_segmentation_amd.utils import VOC_COLORMAP, voc_colormap
    assert VOC_COLORMAP.shape == (32, 3) and VOC_COLORMAP.dtype == np.uint8
    rgb = VOC_COLORMAP[:, ::-1]
    assert tuple(rgb[0]) == (0, 0, 0)
    assert tuple(rgb[1]) == (128, 0, 0)
    assert tuple(rgb[2]) == (0, 128, 0)
    assert tuple(rgb[15]) == (192, 128, 128)
    assert np.array_equal(voc_colormap(256)[:32], VOC_COLORMAP)


def test_lut_classes_beyond_palette_are_black():
    from pytorch_segmentation_amd.utils import VOC_COLORMAP
    from pytorch_segmentation_amd.utils.inference import lut_of
    lut = lut_of(VOC_COLORMAP)
    assert lut.shape == (256, 3) and np.array_equal(lut[:32], VOC_COLORMAP) and not lut[32:].any()


def test_reference_import_paths():
    from utils.datasets import VOC_COLORMAP
    from utils.inference import inference
    import pytorch_segmentation_amd.utils as u
    assert inference is u.inference and VOC_COLORMAP is u.VOC_COLORMAP


def test_inference_rejects_bad_photos_and_norm():
    import torch
    from pytorch_segmentation_amd.utils import inference
    model = torch.nn.Conv2d(3, 2, 1)
    with pytest.raises(ValueError, match='norm'):
        inference(model, [np.zeros((4, 4, 3), np.uint8)], norm='imagenet')
    with pytest.raises(ValueError, match='uint8'):
        inference(model, [np.zeros((4, 4, 3), np.float32)])
    with pytest.raises(ValueError, match='uint8'):
        inference(model, [np.zeros((4, 4), np.uint8)])
    assert inference(model, []) == []


def test_cli_help():
    out = subprocess.check_output([sys.executable, 'inference.py', '--help'], cwd=REPO).decode()
    for flag in ('img_dir', 'output_dir', '--img_size', '--num-classes', '--weights', '--show', '--model', '--batch-size',
                 '-mp', '--norm'):
        assert flag in out, flag


def test_cli_file_selection_and_names(tmp_path, monkeypatch):
    """IMG_EXT matches, case-sensitive as the reference, sorted by name; outputs are <stem>.png; the output directory is
    created and never emptied; --show warns once and is ignored."""
    sys.path.insert(0, REPO)
    import inference as cli
    img_dir, out_dir = tmp_path / 'in', tmp_path / 'out'
    img_dir.mkdir()
    out_dir.mkdir()
    (out_dir / 'keep.txt').write_text('x')
    from PIL import Image
    names = ['b.jpg', 'a.png', 'c.bmp', 'd.JPG', 'notes.txt', 'e.tif', 'f.jpeg']
    for i, n in enumerate(names):
        if n.endswith('.txt'):
            (img_dir / n).write_text('not an image')
        else:
            Image.fromarray(np.full((5 + i, 7, 3), i, np.uint8)).save(str(img_dir / n), format='PNG')
    assert cli.list_images(str(img_dir)) == ['a.png', 'b.jpg', 'c.bmp', 'e.tif', 'f.jpeg']

    calls = []

    class Stub(torch_module()):
        def __init__(self, nc):
            super().__init__()

        def load_state_dict(self, sd):
            assert sd == {'w': 1}

        def cuda(self):
            return self

    def fake_inference(model, imgs, img_size, norm, bgr, half, colors):
        calls.append(([im.shape for im in imgs], img_size, norm, bgr, half))
        masks = [np.ones(im.shape[:2], np.int64) for im in imgs]
        return masks, [colors[m] for m in masks]

    monkeypatch.setitem(cli.MODELS, 'unet', Stub)
    monkeypatch.setattr(cli, 'inference', fake_inference)
    monkeypatch.setattr(cli.torch, 'load', lambda path, map_location=None: {'model': {'w': 1}})
    with pytest.warns(RuntimeWarning, match='--show'):
        done = cli.run(str(img_dir), str(out_dir), [32, 16], 2, 'w.pt', show=True, model_name='unet', batch_size=2)
    assert done == ['a.png', 'b.jpg', 'c.bmp', 'e.tif', 'f.jpeg']
    assert [len(c[0]) for c in calls] == [2, 2, 1]
    assert all(c[1] == (32, 16) and c[2] == 'dataset' and c[3] is False and c[4] is False for c in calls)
    written = sorted(os.listdir(out_dir))
    assert written == ['a.png', 'b.png', 'c.png', 'e.png', 'f.png', 'keep.txt']
    px = np.asarray(Image.open(str(out_dir / 'c.png')))
    assert px.shape == (5 + 2, 7, 3) and (px == (128, 0, 0)).all()


def torch_module():
    import torch
    return torch.nn.Module


@pytest.mark.parametrize('route', ['plain', 'ensemble', 'slide'])
def test_pack_staging_layout(route):
    """The staging buffer of every route: the head tables' bytes in order, then the photos back to back at head + 3 *
    pix_off; offsets and totals against an independent cumulative sum."""
    from pytorch_segmentation_amd.utils.inference import pack_staging
    rng = np.random.default_rng(4)
    shapes = [(5, 7), (1, 1), (4, 3)]
    imgs = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for H, W in shapes]
    imgs[2] = imgs[2][:, ::-1]                                   # a view that is not contiguous
    photos = [(im, im.shape[0], im.shape[1]) for im in imgs]
    B, V, S, N = len(photos), 2, 2, 5
    dims = {'plain': [(2, B, 3)], 'ensemble': [(V * B, 4), (B, 3), (S, 3)], 'slide': [(N, 8), (B, 3), (S, B, 3)]}[route]
    heads = [rng.integers(-2 ** 40, 2 ** 40, d, dtype=np.int64) for d in dims]
    want_off, o = [], 0
    for H, W in shapes:
        want_off.append(o)
        o += H * W
    want_head = sum(8 * int(np.prod(d)) for d in dims)
    head, pix_off, total_pix, sizes = pack_staging(photos, heads)        # the layout alone
    assert head == want_head and list(pix_off) == want_off and total_pix == o == 35 + 1 + 12
    assert sizes.dtype == np.int64 and sizes.tolist() == [list(s) for s in shapes]
    buf = np.full(head + 3 * total_pix + 16, 0xAB, dtype=np.uint8)
    assert pack_staging(photos, heads, buf[:head + 3 * total_pix])[0] == head
    assert buf[:head].tobytes() == b''.join(t.tobytes() for t in heads)
    for im, po in zip(imgs, want_off):
        assert buf[head + 3 * po:head + 3 * po + im.size].tobytes() == np.ascontiguousarray(im).tobytes()
    assert (buf[head + 3 * total_pix:] == 0xAB).all()
