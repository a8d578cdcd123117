"""Batched inference on the device (csrc/infer.hip, utils/inference.py, inference.py) against float64 restatements of
the reference's host passes (reference utils/inference.py:10-22): resize + normalise before the model, softmax -> bilinear
resize -> argmax after it."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import fill
from oracle import margins
from oracle import models as omodels

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda'


@pytest.fixture(scope='module')
def pkg():
    assert torch.cuda.is_available()
    import pytorch_segmentation_amd as p
    return p


def _rng(seed):
    return np.random.default_rng(seed)


def _photos(sizes, seed):
    rng = _rng(seed)
    out = []
    for (H, W) in sizes:
        # smooth content plus noise: bilinear values land everywhere between the 8-bit steps
        yy, xx = np.meshgrid(np.linspace(0, 6, H), np.linspace(0, 9, W), indexing='ij')
        base = 127.5 + 100 * np.sin(yy[..., None] + xx[..., None] * np.array([1.0, 0.7, 1.3]))
        out.append(np.clip(base + rng.normal(0, 30, (H, W, 3)), 0, 255).astype(np.uint8))
    return out


def _pack(photos, per_px):
    """flat device buffer + int64 device table {offset, H, W} (offset in elements of per_px each)"""
    offs, o = [], 0
    for p in photos:
        offs.append(o)
        o += p.shape[0] * p.shape[1]
    table = torch.tensor([[per_px * of, p.shape[0], p.shape[1]] for of, p in zip(offs, photos)], dtype=torch.int64)
    return offs, o, table.to(DEV)


def _preprocess(photos, oh, ow, mean, std, bgr):
    from pytorch_segmentation_amd import ops
    _, total, table = _pack(photos, 3)
    src = torch.from_numpy(np.concatenate([p.reshape(-1) for p in photos])).to(DEV)
    return ops.image_preprocess(src, table, oh, ow, mean, std, bgr)


def _pre_oracle(photo, oh, ow, bgr):
    """float64: INTER_LINEAR resample (value before rounding) and the 8-bit result, RGB order, [3, oh, ow]"""
    x = torch.from_numpy(photo.astype(np.float64)).permute(2, 0, 1)
    if bgr:
        x = x.flip(0)
    v = F.interpolate(x[None], (oh, ow), mode='bilinear', align_corners=False)[0]
    return v, torch.clamp(torch.floor(v + 0.5), 0, 255)


SIZES = [(1, 1), (37, 53), (320, 320), (480, 640), (1080, 1920)]


@pytest.mark.parametrize('norm', ['dataset', 'reference'])
@pytest.mark.parametrize('bgr', [True, False])
@pytest.mark.parametrize('oh,ow', [(320, 320), (256, 384)])
def test_preprocess_vs_float64(pkg, norm, bgr, oh, ow):
    from pytorch_segmentation_amd.utils.datasets import CocoDataset
    from pytorch_segmentation_amd.utils.inference import NORMS
    mean, std = NORMS[norm]
    photos = _photos(SIZES, 1 + oh + int(bgr))
    got = _preprocess(photos, oh, ow, mean, std, bgr).cpu()
    assert got.shape == (len(photos), 3, oh, ow)
    m32 = torch.tensor(mean, dtype=torch.float32).view(3, 1, 1)
    s32 = torch.tensor(std, dtype=torch.float32).view(3, 1, 1)
    for i, p in enumerate(photos):
        v, q = _pre_oracle(p, oh, ow, bgr)
        ref64 = (q - m32.double()) / s32.double()
        step = 1.0 / s32.double()
        assert ((got[i].double() - ref64).abs() <= step * 1.0001 + 1e-6).all(), i
        exact = ((v - torch.floor(v)) - 0.5).abs() > 1e-3
        want32 = (q.float() - m32) / s32                  # the same fp32 operations on the oracle's 8-bit value
        assert torch.equal(got[i][exact], want32[exact]), (i, (got[i][exact] != want32[exact]).sum().item())
        assert exact.float().mean() > 0.5                 # (x2 down-scaling lands on exact half-integers)
        if (p.shape[0], p.shape[1]) == (oh, ow) and norm == 'dataset':
            rgb = p[..., ::-1] if bgr else p
            chw = torch.from_numpy(np.ascontiguousarray(rgb.transpose(2, 0, 1)))[None]
            loader, _ = CocoDataset.post_fetch_fn(SimpleNamespace(multi_scale=False), (chw, torch.zeros(1, oh, ow)))
            assert torch.equal(got[i], loader[0])          # bit-identical to the training loader's input


def _decode_oracle(logits64, H, W):
    """float64: softmax over classes, bilinear to (H, W), -> (argmax mask, top-2 probability margin)"""
    p = torch.softmax(logits64, dim=0)[None]
    r = F.interpolate(p, (H, W), mode='bilinear', align_corners=False)[0]
    if r.shape[0] == 1:
        return torch.zeros(H, W, dtype=torch.int64), torch.full((H, W), float('inf'), dtype=torch.float64)
    t = r.topk(2, dim=0).values
    return r.argmax(0), t[0] - t[1]


def _decode(logits, sizes, lut=None):
    from pytorch_segmentation_amd import ops
    offs, total, table = _pack([np.empty((H, W, 0)) for H, W in sizes], 1)
    mask, rgb = ops.seg_decode(logits.contiguous(), table, total, lut)
    mask = mask.cpu()
    masks = [mask[o:o + H * W].view(H, W).long() for o, (H, W) in zip(offs, sizes)]
    rgbs = None if rgb is None else [rgb.cpu()[o:o + H * W].view(H, W, 3) for o, (H, W) in zip(offs, sizes)]
    return masks, rgbs


@pytest.mark.parametrize('C', [1, 2, 21, 150, 256])
def test_decode_vs_float64(pkg, C):
    h, w = 64, 96
    sizes = [(150, 200), (h, w), (h // 8, w // 8), (1, 1), (203, 97)]   # larger, equal, x1/8, 1x1, mixed ratios
    g = torch.Generator().manual_seed(C)
    logits = torch.randn(len(sizes), C, h, w, generator=g) * 3
    lut = torch.randint(0, 256, (256, 3), dtype=torch.uint8, generator=g)
    masks, rgbs = _decode(logits.to(DEV), sizes, lut.to(DEV))
    n_safe = n_all = 0
    for i, (H, W) in enumerate(sizes):
        want, margin = _decode_oracle(logits[i].double(), H, W)
        safe = margin > 1e-6
        assert torch.equal(masks[i][safe], want[safe]), (i, (masks[i][safe] != want[safe]).sum().item())
        assert torch.equal(rgbs[i], lut[masks[i]])
        n_safe += safe.sum().item()
        n_all += H * W
    assert n_safe >= 0.99 * n_all, (n_safe, n_all)


def test_decode_constant_logits_and_limits(pkg):
    from pytorch_segmentation_amd import _lib
    masks, _ = _decode(torch.zeros(2, 21, 9, 13, device=DEV), [(40, 50), (3, 2)])
    assert all((m == 0).all() for m in masks)
    masks, _ = _decode(torch.full((1, 256, 5, 5), 7.0, device=DEV), [(17, 4)])
    assert (masks[0] == 0).all()
    with pytest.raises(_lib.PsegError, match='256'):
        _decode(torch.zeros(1, 257, 4, 4, device=DEV), [(8, 8)])


def _rows_oracle(P64, H, W, rows):
    """float64 bilinear (align_corners=False) of probabilities P64 [C, h, w] at output rows `rows`, all columns"""
    C, h, w = P64.shape

    def taps(n_in, n_out, o):
        s = np.maximum((o + 0.5) * (n_in / n_out) - 0.5, 0.0)
        i0 = np.minimum(np.floor(s).astype(np.int64), n_in - 1)
        i1 = np.minimum(i0 + 1, n_in - 1)
        l1 = s - i0
        return i0, i1, 1 - l1, l1

    x0, x1, lx0, lx1 = taps(w, W, np.arange(W))
    out = []
    for oy in rows:
        y0, y1, ly0, ly1 = taps(h, H, np.array(oy))
        r = ly0 * (lx0 * P64[:, y0, x0] + lx1 * P64[:, y0, x1]) + ly1 * (lx0 * P64[:, y1, x0] + lx1 * P64[:, y1, x1])
        out.append(r)
    return np.stack(out, 1)            # [C, len(rows), W]


def test_decode_full_size_batch(pkg):
    """B = 16, C = 21, 512^2 logits -> 1024 x 2048 masks (the measured configuration), float64 on a sample of rows."""
    B, C, h, w, H, W = 16, 21, 512, 512, 1024, 2048
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(B, C, h, w, generator=g) * 3
    masks, _ = _decode(logits.to(DEV), [(H, W)] * B)
    rows = [0, 1, 2, 511, 512, 777, 1022, 1023]
    n_safe = n_all = 0
    for b in (0, 7, 15):
        P = torch.softmax(logits[b].double(), 0).numpy()
        r = _rows_oracle(P, H, W, rows)
        srt = np.sort(r, 0)
        margin, want = srt[-1] - srt[-2], r.argmax(0)
        safe = margin > 1e-6
        got = masks[b][rows].numpy()
        assert np.array_equal(got[safe], want[safe]), b
        n_safe += safe.sum()
        n_all += safe.size
    assert n_safe >= 0.99 * n_all


# ------------------------------------------------------------------ end to end
E2E_SIZES = [(100, 130), (64, 64), (77, 50), (90, 120), (33, 200)]
LOGIT_TOL = 1e-3          # fp32 path vs fp64 oracle, relative to the peak logit (tests/test_models_gpu.py)
HALF_LOGIT_TOL = 2e-2     # half policy (tests/test_half_models_gpu.py)


def _models(name, nc, S):
    from pytorch_segmentation_amd import models
    hip = {'deeplabv3plus': models.DeepLabV3Plus, 'unet': models.UNet}[name]
    ref = {'deeplabv3plus': omodels.DeepLabV3Plus, 'unet': omodels.UNet}[name](nc)
    key = 'infer_%s' % name
    fill.fill_module_(ref, key)
    if name == 'deeplabv3plus':           # residual gain of a trained network (see tests/test_half_models_gpu.py)
        with torch.no_grad():
            for mn, mod in ref.named_modules():
                if mn.endswith('bn3'):
                    mod.weight.mul_(0.25)
    margins.freeze_stats(ref, fill.images(key + '/x', (4, 3, S, S)))
    ref.eval()
    m = hip(nc)
    m.load_state_dict({k: v.clone() for k, v in ref.state_dict().items()})
    return m.cuda().eval(), ref


@pytest.mark.parametrize('name,nc', [('deeplabv3plus', 21), ('unet', 2)])
def test_inference_end_to_end(pkg, name, nc):
    import copy
    from pytorch_segmentation_amd.utils import inference
    from pytorch_segmentation_amd.utils.datasets import MEAN, STD
    S = 64
    m, ref = _models(name, nc, S)
    photos = _photos(E2E_SIZES, 11)
    masks4 = inference(m, photos, (S, S))
    masks1 = [inference(m, [p], (S, S))[0] for p in photos]
    masks_h = inference(m, photos, (S, S), half=True)
    x = _preprocess(photos, S, S, MEAN, STD, True).cpu()
    ref64 = copy.deepcopy(ref).double()
    with torch.no_grad():
        logits64 = ref64(x.double())
    peak = logits64.abs().max().item()
    fracs = []
    for i, (H, W) in enumerate(E2E_SIZES):
        assert masks4[i].shape == (H, W) and masks4[i].dtype == np.int64
        want, margin = _decode_oracle(logits64[i], H, W)
        safe = (margin > 2 * LOGIT_TOL * peak).numpy()
        assert np.array_equal(masks4[i][safe], want.numpy()[safe]), i
        assert np.array_equal(masks1[i][safe], masks4[i][safe]), i
        hsafe = (margin > 2 * HALF_LOGIT_TOL * peak).numpy()
        assert np.array_equal(masks_h[i][hsafe], masks4[i][hsafe]), i
        fracs.append((safe.mean(), hsafe.mean()))
    print('%s: safe-margin fraction fp32 %.3f, half %.3f' % (name, np.mean([f[0] for f in fracs]), np.mean([f[1] for f in fracs])))
    assert np.mean([f[0] for f in fracs]) > 0.5
    assert np.mean([f[1] for f in fracs]) > 0.2
    # the half forward left no Env behind: a plain call afterwards is the fp32 path again
    assert all(np.array_equal(a, b) for a, b in zip(inference(m, photos, (S, S)), masks4))


def test_inference_device_tensors_and_colors(pkg):
    from pytorch_segmentation_amd.utils import VOC_COLORMAP, inference
    m, _ = _models('unet', 2, 64)
    photos = _photos([(50, 70), (64, 64)], 3)
    masks = inference(m, photos, (64, 64), norm='reference', bgr=False)
    mixed = [torch.from_numpy(photos[0]).cuda(), torch.from_numpy(photos[1])]
    masks2, colored = inference(m, mixed, (64, 64), norm='reference', bgr=False, colors=VOC_COLORMAP)
    for a, b, c in zip(masks, masks2, colored):
        assert np.array_equal(a, b)
        assert np.array_equal(c, VOC_COLORMAP[a])


def test_cli_writes_palette_pngs(pkg, tmp_path):
    from PIL import Image
    from pytorch_segmentation_amd.utils import inference
    from pytorch_segmentation_amd.utils.datasets import VOC_COLORMAP, make_synthetic_coco
    root = make_synthetic_coco(str(tmp_path / 'data'), n_train=3, n_val=0, size=(160, 128))
    img_dir = os.path.join(root, 'images')
    Image.fromarray(_photos([(45, 97)], 9)[0]).save(os.path.join(img_dir, 'odd.jpg'), quality=95)
    with open(os.path.join(img_dir, 'readme.txt'), 'w') as f:
        f.write('not an image')
    m, _ = _models('unet', 2, 64)
    ckpt = str(tmp_path / 'w.pt')
    torch.save({'model': {k: v.cpu() for k, v in m.state_dict().items()}}, ckpt)
    out_dir = tmp_path / 'out'
    out_dir.mkdir()
    (out_dir / 'keep.txt').write_text('mine')
    cmd = [sys.executable, 'inference.py', img_dir, str(out_dir), '-s', '64', '64', '-nc', '2', '--weights', ckpt,
           '--model', 'unet', '-bs', '2']
    subprocess.run(cmd, cwd=REPO, check=True, timeout=600)
    names = sorted(n for n in os.listdir(img_dir) if n.endswith(('.png', '.jpg')))
    assert sorted(os.listdir(out_dir)) == sorted([os.path.splitext(n)[0] + '.png' for n in names] + ['keep.txt'])
    assert (out_dir / 'keep.txt').read_text() == 'mine'
    imgs = [np.asarray(Image.open(os.path.join(img_dir, n)).convert('RGB')) for n in names]
    masks = []
    for i in range(0, len(imgs), 2):
        masks += inference(m, imgs[i:i + 2], (64, 64), bgr=False)
    for n, im, mk in zip(names, imgs, masks):
        px = np.asarray(Image.open(str(out_dir / (os.path.splitext(n)[0] + '.png'))).convert('RGB'))
        assert px.shape == im.shape, n
        assert np.array_equal(px, VOC_COLORMAP[:, ::-1][mk]), n


def test_infer_bits_match_recorded(pkg, golden_dir):
    """every entry point of csrc/infer.hip (tests/infer_bits.py: the three preprocess routes at 32 x 48 with bgr and both
    normalisations, the three decodes at C in {2, 8, 9, 21, 150} with and without mirrored twins, softmax_views) writes the
    bytes recorded in tests/golden/infer_bits.json from the kernels as they stood before their shared parts were folded"""
    import json

    import infer_bits
    from optim_bits import compiler_line
    from pytorch_segmentation_amd import ops
    with open(os.path.join(golden_dir, 'infer_bits.json')) as f:
        rec = json.load(f)
    got = infer_bits.digests(ops)
    assert sorted(got) == sorted(rec['digests'])
    for name, tensors in got.items():
        assert sorted(tensors) == sorted(rec['digests'][name]), name
        for k, h in tensors.items():
            assert h == rec['digests'][name][k], \
                'case %s, tensor %s: sha256 %s, recorded %s (recorded from %s under "%s", installed "%s")' % (
                    name, k, h, rec['digests'][name][k], rec['commit'], rec['compiler'], compiler_line())
