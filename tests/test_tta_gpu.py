"""Test-time ensembling on the device (csrc/infer.hip: image_preprocess_views, softmax_views, seg_decode_ensemble;
utils/inference.py, utils/loss.py, test.py) against float64 restatements of its definition: for every view (scale x
plain / mirrored) softmax -> un-mirror -> bilinear resize (align_corners=False) to the photo's size, unweighted sum,
argmax with the first index winning ties."""
import copy
import importlib.util
import os

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


# ------------------------------------------------------------------ helpers (the idiom of tests/test_inference_gpu.py)
def _photos(sizes, seed):
    rng = np.random.default_rng(seed)
    out = []
    for (H, W) in sizes:
        yy, xx = np.meshgrid(np.linspace(0, 6, H), np.linspace(0, 9, W), indexing='ij')
        base = 127.5 + 100 * np.sin(yy[..., None] + xx[..., None] * np.array([1.0, 0.7, 1.3]))
        out.append(np.clip(base + rng.normal(0, 30, (H, W, 3)), 0, 255).astype(np.uint8))
    return out


def _pack(photos, per_px):
    """flat size + int64 host table {offset, H, W} (offset in elements of per_px each)"""
    offs, o = [], 0
    for p in photos:
        offs.append(o)
        o += p.shape[0] * p.shape[1]
    table = torch.tensor([[per_px * of, p.shape[0], p.shape[1]] for of, p in zip(offs, photos)], dtype=torch.int64)
    return offs, o, table


def _views(photos, oh, ow, mean, std, bgr, flip=True):
    """-> (ops.image_preprocess_views of every photo plain, then every photo flagged; ops.image_preprocess)"""
    from pytorch_segmentation_amd import ops
    _, _, table = _pack(photos, 3)
    src = torch.from_numpy(np.concatenate([p.reshape(-1) for p in photos])).to(DEV)
    rows = [torch.cat([table, torch.zeros(len(photos), 1, dtype=torch.int64)], 1)]
    if flip:
        rows.append(torch.cat([table, torch.full((len(photos), 1), ops.VIEW_MIRROR, dtype=torch.int64)], 1))
    got = ops.image_preprocess_views(src, torch.cat(rows).contiguous().to(DEV), oh, ow, mean, std, bgr)
    return got, ops.image_preprocess(src, table.to(DEV), oh, ow, mean, std, bgr)


def _maps(logit_list, pairs):
    """ops.softmax_views of each tensor into one packed buffer -> (prob, device map table, [views of the maps])"""
    from pytorch_segmentation_amd import ops
    n, C = logit_list[0].shape[:2]
    B, CP = (n // 2 if pairs else n), ops.class_pad(C)
    offs, o = [], 0
    for lg in logit_list:
        offs.append(o)
        o += B * lg.shape[2] * lg.shape[3] * CP
    prob = torch.full((o,), float('nan'), device=DEV)
    views = [ops.softmax_views(lg.to(DEV).contiguous(), prob, of, pairs) for lg, of in zip(logit_list, offs)]
    table = torch.tensor([[of, lg.shape[2], lg.shape[3]] for of, lg in zip(offs, logit_list)], dtype=torch.int64).to(DEV)
    return prob, table, views


def _prob64(logits, pairs):
    """float64 [B,C,h,w]: softmax, plus the un-mirrored softmax of the mirrored twin"""
    p = torch.softmax(logits.double(), 1)
    if not pairs:
        return p
    B = logits.shape[0] // 2
    return p[:B] + p[B:].flip(3)


def _ensemble_oracle(p64s, i, H, W):
    """float64: sum over the maps of bilinear(map[i], (H, W)) -> (argmax mask, top-2 margin of the summed probabilities)"""
    r = sum(F.interpolate(p[i:i + 1], (H, W), mode='bilinear', align_corners=False)[0] for p in p64s)
    if r.shape[0] == 1:
        return torch.zeros(H, W, dtype=torch.int64), torch.full((H, W), float('inf'), dtype=torch.float64)
    t = r.topk(2, dim=0).values
    return r.argmax(0), t[0] - t[1]


def _decode(prob, maps, sizes, C, lut=None):
    from pytorch_segmentation_amd import ops
    offs, total, table = _pack([np.empty((H, W, 0)) for H, W in sizes], 1)
    max_hw = (max(H for H, _ in sizes), max(W for _, W in sizes))
    mask, rgb = ops.seg_decode_ensemble(prob, maps, len(sizes), C, table.to(DEV), total, max_hw, lut)
    mask = mask.cpu()
    masks = [mask[o:o + H * W].view(H, W).long() for o, (H, W) in zip(offs, sizes)]
    rgbs = None if rgb is None else [rgb.cpu()[o:o + H * W].view(H, W, 3) for o, (H, W) in zip(offs, sizes)]
    return masks, rgbs


# ------------------------------------------------------------------ preprocess views
@pytest.mark.parametrize('bgr', [True, False])
def test_preprocess_views_plain_and_mirrored(pkg, bgr):
    from pytorch_segmentation_amd.utils.datasets import MEAN, STD
    photos = _photos([(1, 1), (37, 53), (64, 64), (90, 120)], 5 + int(bgr))
    got, plain = _views(photos, 64, 96, MEAN, STD, bgr)
    B = len(photos)
    assert got.shape == (2 * B, 3, 64, 96)
    assert torch.equal(got[:B], plain)                       # flags 0: image_preprocess bit for bit
    assert torch.equal(got[B:], got[:B].flip(3))             # flagged: the unflagged result mirrored, bit for bit
    assert not torch.equal(got[B + 1], got[1])


def test_preprocess_views_skips_rows_with_undeclared_flags(pkg):
    from pytorch_segmentation_amd import ops
    from pytorch_segmentation_amd.utils.datasets import MEAN, STD
    photo = _photos([(20, 30)], 2)[0]
    src = torch.from_numpy(photo.reshape(-1)).to(DEV)
    table = torch.tensor([[0, 20, 30, 0], [0, 20, 30, 2], [0, 20, 30, 1]], dtype=torch.int64, device=DEV)
    out = torch.empty(3, 3, 32, 32, device=DEV)
    keep = torch.full_like(out, -7.0)
    from pytorch_segmentation_amd import _lib
    out.copy_(keep)
    _lib.call('pseg_image_preprocess_views', src.data_ptr(), src.numel(), table.data_ptr(), 3, 1, 1, *MEAN, *STD, out.data_ptr(),
              32, 32, torch.cuda.current_stream().cuda_stream)
    assert torch.equal(out[1], keep[1])                      # bit 1 is not in flag_mask: nothing written
    assert torch.equal(out[2], out[0].flip(2)) and (out[0] != -7.0).all()
    with pytest.raises(_lib.PsegError, match='unknown flag bits'):
        ops.image_preprocess_views(src, table, 32, 32, MEAN, STD, True, flag_mask=3)


# ------------------------------------------------------------------ softmax views
@pytest.mark.parametrize('pairs', [0, 1])
@pytest.mark.parametrize('C', [1, 2, 21, 150, 256])
def test_softmax_views_vs_float64(pkg, C, pairs):
    """Bound: 4 ulp of the map's value range, the error of an fp32 exp / sum / divide on values <= 1."""
    from pytorch_segmentation_amd import ops
    B, h, w = 3, 17, 23                                      # odd width: the mirror's centre column maps to itself
    g = torch.Generator().manual_seed(100 + C)
    logits = torch.randn(B * (2 if pairs else 1), C, h, w, generator=g) * 3
    _, _, (got,) = _maps([logits], pairs)
    CP = ops.class_pad(C)
    assert got.shape == (B, h, w, CP) and CP % 4 == 0 and CP >= max(C, 8) and CP - C < 8
    got = got.cpu()
    want = _prob64(logits, pairs).permute(0, 2, 3, 1)
    err = (got[..., :C].double() - want).abs().max().item()
    bound = 4 * 2.0 ** -23 * (2 if pairs else 1)
    print('softmax_views C=%d pairs=%d: max abs error %.3g (bound %.3g)' % (C, pairs, err, bound))
    assert err <= bound
    assert (got[..., C:] == 0).all()                         # pad lanes are written, as exact zeros


# ------------------------------------------------------------------ ensemble decode
MAP_SIZES = [(32, 48), (64, 96), (96, 144)]
IMG_SIZES = [(150, 200), (64, 96), (8, 12), (1, 1), (203, 97)]   # larger, equal, x1/8, 1x1, mixed ratios


@pytest.mark.parametrize('pairs', [0, 1])
@pytest.mark.parametrize('C', [1, 2, 21, 150, 256])
def test_ensemble_vs_float64(pkg, C, pairs):
    g = torch.Generator().manual_seed(C)
    n = len(IMG_SIZES) * (2 if pairs else 1)
    logits = [torch.randn(n, C, h, w, generator=g) * 3 for h, w in MAP_SIZES]
    lut = torch.randint(0, 256, (256, 3), dtype=torch.uint8, generator=g)
    prob, maps, _ = _maps(logits, pairs)
    masks, rgbs = _decode(prob, maps, IMG_SIZES, C, lut.to(DEV))
    p64s = [_prob64(lg, pairs) for lg in logits]
    K = len(MAP_SIZES) * (2 if pairs else 1)
    n_safe = n_all = 0
    for i, (H, W) in enumerate(IMG_SIZES):
        want, margin = _ensemble_oracle(p64s, i, H, W)
        safe = margin > 1e-6 * K                             # 1e-6 per unit of probability mass
        assert torch.equal(masks[i][safe], want[safe]), (i, (masks[i][safe] != want[safe]).sum().item())
        assert torch.equal(rgbs[i], lut[masks[i]])
        n_safe += safe.sum().item()
        n_all += H * W
    assert n_safe >= 0.99 * n_all, (n_safe, n_all)


def test_single_map_equals_plain_decode(pkg):
    from pytorch_segmentation_amd import ops
    C, (h, w) = 21, (64, 96)
    g = torch.Generator().manual_seed(7)
    logits = torch.randn(len(IMG_SIZES), C, h, w, generator=g) * 3
    prob, maps, _ = _maps([logits], 0)
    masks, _ = _decode(prob, maps, IMG_SIZES, C)
    offs, total, table = _pack([np.empty((H, W, 0)) for H, W in IMG_SIZES], 1)
    plain = ops.seg_decode(logits.to(DEV), table.to(DEV), total)[0].cpu()
    p64 = [_prob64(logits, 0)]
    for i, (H, W) in enumerate(IMG_SIZES):
        _, margin = _ensemble_oracle(p64, i, H, W)
        safe = margin > 1e-6
        assert torch.equal(masks[i][safe], plain[offs[i]:offs[i] + H * W].view(H, W).long()[safe]), i
        assert safe.float().mean() > 0.99 or H * W < 200


def test_ragged_batch_and_bad_rows(pkg):
    """Images from 203 x 97 down to 1 x 1 with gaps between them, one record whose extent leaves the mask buffer, and an
    image larger than the stated maximum: every valid image is right, and no byte outside a valid image's range changes."""
    from pytorch_segmentation_amd import ops
    C = 21
    sizes = [(203, 97), (1, 1), (8, 12), (64, 96), (150, 40)]
    g = torch.Generator().manual_seed(3)
    logits = [torch.randn(len(sizes) + 2, C, h, w, generator=g) * 3 for h, w in MAP_SIZES[:2]]
    lut = torch.randint(0, 256, (256, 3), dtype=torch.uint8, generator=g)
    prob, maps, _ = _maps(logits, 0)
    rows, o = [], 5
    for H, W in sizes:
        rows.append([o, H, W])
        o += H * W + 7                                       # a gap after every image
    total = o + 50
    rows.append([o, 8, 12])                                  # 96 pixels into the 50 bytes that are left: leaves the buffer
    rows.append([0, 300, 97])                                # taller than Hmax: skipped, although it fits the buffer
    table = torch.tensor(rows, dtype=torch.int64, device=DEV)
    guard = 64
    big = torch.full((guard + 4 * total + guard,), 0xAB, dtype=torch.uint8, device=DEV)
    ops.seg_decode_ensemble(prob, maps, len(rows), C, table, total, (203, 97), lut.to(DEV), out=big[guard:guard + 4 * total])
    big = big.cpu()
    mask, rgb = big[guard:guard + total], big[guard + total:guard + 4 * total].view(total, 3)
    touched = torch.zeros(total, dtype=torch.bool)
    p64s = [_prob64(lg, 0) for lg in logits]
    for i, (H, W) in enumerate(sizes):
        of = rows[i][0]
        got = mask[of:of + H * W].view(H, W).long()
        want, margin = _ensemble_oracle(p64s, i, H, W)
        safe = margin > 1e-6 * 2
        assert torch.equal(got[safe], want[safe]), i
        assert torch.equal(rgb[of:of + H * W].view(H, W, 3), lut[got]), i
        touched[of:of + H * W] = True
    assert (mask[~touched] == 0xAB).all() and (rgb[~touched] == 0xAB).all()
    assert (big[:guard] == 0xAB).all() and (big[-guard:] == 0xAB).all()

    # a map record that leaves the packed buffer: no image is written at all
    bad_maps = maps.clone()
    bad_maps[1, 0] += 4
    out = torch.full((4 * total,), 0xAB, dtype=torch.uint8, device=DEV)
    ops.seg_decode_ensemble(prob, bad_maps, len(rows), C, table, total, (203, 97), lut.to(DEV), out=out)
    assert (out == 0xAB).all()


# ------------------------------------------------------------------ end to end
E2E_SIZES = [(100, 130), (64, 64), (77, 50)]
LOGIT_TOL = 1e-3          # fp32 path vs fp64 oracle, relative to the peak logit (tests/test_inference_gpu.py)
HALF_LOGIT_TOL = 2e-2     # half policy


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
def test_inference_ensemble_end_to_end(pkg, name, nc):
    from pytorch_segmentation_amd.utils import inference
    from pytorch_segmentation_amd.utils.datasets import MEAN, STD
    from pytorch_segmentation_amd.utils.inference import tta_sizes
    S, scales = 64, (1.0, 1.5)
    m, ref = _models(name, nc, S)
    photos = _photos(E2E_SIZES, 11)
    B = len(photos)
    plain = inference(m, photos, (S, S))
    same = inference(m, photos, (S, S), scales=(1.0,), flip=False)
    assert all(np.array_equal(a, b) for a, b in zip(plain, same))          # the existing path, bit-identical masks
    masks = inference(m, photos, (S, S), scales=scales, flip=True)
    masks_h = inference(m, photos, (S, S), scales=scales, flip=True, half=True)

    ref64 = copy.deepcopy(ref).double()
    p64s, peak = [], 0.0
    for hs, ws in tta_sizes(S, S, scales):
        x, x_plain = _views(photos, hs, ws, MEAN, STD, True)
        assert torch.equal(x[:B], x_plain) and torch.equal(x[B:], x[:B].flip(3))
        with torch.no_grad():
            logits64 = ref64(x.cpu().double())
        peak = max(peak, logits64.abs().max().item())
        p64s.append(_prob64(logits64, 1))
    K = 2 * len(p64s)
    fracs = []
    for i, (H, W) in enumerate(E2E_SIZES):
        assert masks[i].shape == (H, W) and masks[i].dtype == np.int64
        want, margin = _ensemble_oracle(p64s, i, H, W)
        safe = (margin > 2 * LOGIT_TOL * peak * K).numpy()
        assert np.array_equal(masks[i][safe], want.numpy()[safe]), i
        hsafe = (margin > 2 * HALF_LOGIT_TOL * peak * K).numpy()
        assert np.array_equal(masks_h[i][hsafe], want.numpy()[hsafe]), i
        fracs.append((safe.mean(), hsafe.mean()))
    print('%s: safe-margin fraction fp32 %.3f, half %.3f' % (name, np.mean([f[0] for f in fracs]), np.mean([f[1] for f in fracs])))
    assert np.mean([f[0] for f in fracs]) > 0.5
    assert np.mean([f[1] for f in fracs]) > 0.2
    # the views are really used: the ensemble is not the single-view prediction
    assert any((a != b).any() for a, b in zip(masks, plain))
    # colours ride along as in the single-view call
    from pytorch_segmentation_amd.utils import VOC_COLORMAP
    masks2, colored = inference(m, photos, (S, S), scales=scales, flip=True, colors=VOC_COLORMAP)
    for a, b, c in zip(masks, masks2, colored):
        assert np.array_equal(a, b) and np.array_equal(c, VOC_COLORMAP[a])


# ------------------------------------------------------------------ evaluation
def test_predict_mask_ensemble_is_the_ops_composition(pkg):
    from pytorch_segmentation_amd import ops
    from pytorch_segmentation_amd.utils import predict_mask_ensemble
    m, _ = _models('unet', 2, 64)
    x = fill.images('tta/eval', (2, 3, 64, 64)).to(DEV)
    got = predict_mask_ensemble(m, x, (80, 72), (1.0, 1.5), True)
    assert got.shape == (2, 80, 72) and got.dtype == torch.int64
    logits = []
    with torch.no_grad():
        for hw in [(64, 64), (96, 96)]:
            v = x if hw == (64, 64) else F.interpolate(x, hw, mode='bilinear', align_corners=False)
            logits.append(m(torch.cat([v, v.flip(3)]).contiguous()).float())
    prob, maps, _ = _maps(logits, 1)
    masks, _ = _decode(prob, maps, [(80, 72)] * 2, 2)
    assert torch.equal(got.cpu(), torch.stack(masks))
    single = predict_mask_ensemble(m, x, (80, 72), (1.0,), False)
    assert (single != got).any()


def test_evaluation_with_the_flags(pkg, tmp_path, monkeypatch):
    from torch.utils.data import DataLoader
    from pytorch_segmentation_amd.utils import Fetcher
    from pytorch_segmentation_amd.utils.datasets import CocoDataset, make_synthetic_coco
    spec = importlib.util.spec_from_file_location('pseg_eval_cli', os.path.join(REPO, 'test.py'))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    root = make_synthetic_coco(str(tmp_path / 'data'), n_train=1, n_val=4, n_classes=1)
    data = CocoDataset(os.path.join(root, 'val.json'), img_size=[64, 64], augments=None)
    fetcher = Fetcher(DataLoader(data, batch_size=2, num_workers=0), post_fetch_fn=data.post_fetch_fn)
    m, _ = _models('unet', 2, 64)
    seen = []
    monkeypatch.setattr(cli, 'all_reduce_counters', lambda c: seen.append(c.clone()))
    miou = cli.test(m, fetcher, scales=(1.5, 2.0), flip=True)           # (no scale 1.0: the loss takes its own forward)
    assert isinstance(miou, float) and 0.0 <= miou <= 1.0
    tp, fn, _ = seen[-1].cpu()
    assert int((tp + fn).sum()) == 4 * 64 * 64
    miou_1 = cli.test(m, fetcher, scales=(1.0, 1.5), flip=True)
    assert 0.0 <= miou_1 <= 1.0 and int(seen[-1][:2].sum()) == 4 * 64 * 64
    plain = cli.test(m, fetcher)
    assert 0.0 <= plain <= 1.0 and int(seen[-1][:2].sum()) == 4 * 64 * 64
