"""Sliding-window inference on the device (csrc/infer.hip: image_preprocess_windows, seg_decode_windows;
utils/inference.py, utils/loss.py, test.py) against the float64 restatement of its definition in tests/slide_ref.py:
per working pixel the mean of the covering windows' softmaxes, resized bilinearly (align_corners=False) to the photo's
size, summed over the scales, argmax with the first index winning ties."""
import copy
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import regions_ref
import slide_ref
from oracle import fill
from test_tta_gpu import HALF_LOGIT_TOL, LOGIT_TOL, _decode, _maps, _models, _photos, _prob64, _ensemble_oracle

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda'
WIN, STRIDE = (32, 48), (22, 32)         # (h, w), (sy, sx): both strides strictly between half the window and the window


@pytest.fixture(scope='module')
def pkg():
    assert torch.cuda.is_available()
    import pytorch_segmentation_amd as p
    return p


def _src(photos):
    """-> (flat uint8 device tensor of the photos back to back, byte offset of each)"""
    offs = np.concatenate([[0], np.cumsum([p.size for p in photos])[:-1]]).tolist()
    return torch.from_numpy(np.concatenate([p.reshape(-1) for p in photos])).to(DEV), offs


def _rows(rows):
    return torch.tensor(rows, dtype=torch.int64, device=DEV).view(-1, 8)


# ------------------------------------------------------------------ preprocess windows
PRE_SIZES = [(1, 1), (37, 53), (64, 64), (90, 120)]


@pytest.mark.parametrize('bgr', [True, False])
def test_preprocess_row_without_origin_equals_views(pkg, bgr):
    from pytorch_segmentation_amd import ops
    from pytorch_segmentation_amd.utils.datasets import MEAN, STD
    photos = _photos(PRE_SIZES, 5 + int(bgr))
    src, offs = _src(photos)
    h, w = WIN
    views = [[o, p.shape[0], p.shape[1], f] for f in (0, ops.VIEW_MIRROR) for o, p in zip(offs, photos)]
    want = ops.image_preprocess_views(src, torch.tensor(views, dtype=torch.int64, device=DEV), h, w, MEAN, STD, bgr)
    got = ops.image_preprocess_windows(src, _rows([v + [h, w, 0, 0] for v in views]), h, w, MEAN, STD, bgr)
    assert got.shape == (2 * len(photos), 3, h, w)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))        # bit for bit, plain and mirrored
    assert not torch.equal(got[len(photos) + 1], got[1])


@pytest.mark.parametrize('bgr', [True, False])
def test_preprocess_windows_are_crops_of_the_working_image(pkg, bgr):
    from pytorch_segmentation_amd import ops
    from pytorch_segmentation_amd.utils.datasets import MEAN, STD
    from pytorch_segmentation_amd.utils.inference import window_grid, work_size
    photos = _photos(PRE_SIZES, 7 + int(bgr))
    src, offs = _src(photos)
    h, w = WIN
    m32, s32 = torch.tensor(MEAN).view(3, 1, 1), torch.tensor(STD).view(3, 1, 1)
    windows = 0
    for s in (1.0, 0.5):
        for o, p in zip(offs, photos):
            H, W = p.shape[:2]
            Hs, Ws = work_size(H, W, s)
            head = [o, H, W]
            full = ops.image_preprocess_windows(src, _rows([head + [0, Hs, Ws, 0, 0]]), Hs, Ws, MEAN, STD, bgr)
            views = ops.image_preprocess_views(src, torch.tensor([head + [0]], dtype=torch.int64, device=DEV), Hs, Ws, MEAN, STD, bgr)
            assert torch.equal(full.view(torch.int32), views.view(torch.int32))
            if s == 1.0:                                     # the photo itself: the taps degenerate to weights 1 / 0
                rgb = p[..., ::-1] if bgr else p
                q = torch.from_numpy(np.ascontiguousarray(rgb.transpose(2, 0, 1))).float()
                assert torch.equal(full[0].cpu(), (q - m32) / s32)
            origins, _ = window_grid(Hs, Ws, h, w, *STRIDE)
            rows = [head + [f, Hs, Ws, y0, x0] for f in (0, ops.VIEW_MIRROR) for y0, x0 in origins]
            got = ops.image_preprocess_windows(src, _rows(rows), h, w, MEAN, STD, bgr)
            n = len(origins)
            for k, (y0, x0) in enumerate(origins):
                want = torch.zeros(3, h, w, device=DEV)
                hh, ww = min(h, Hs - y0), min(w, Ws - x0)
                want[:, :hh, :ww] = full[0, :, y0:y0 + hh, x0:x0 + ww]
                assert torch.equal(got[k].view(torch.int32), want.view(torch.int32)), (s, H, W, k)   # +0.0 beyond the image
                assert torch.equal(got[n + k].view(torch.int32), want.flip(2).view(torch.int32)), (s, H, W, k)
            windows += n
    assert windows == (1 + 2 * 2 + 3 * 2 + 4 * 4) + (1 + 1 + 1 * 1 + 2 * 2)


def test_preprocess_skips_bad_rows(pkg):
    from pytorch_segmentation_amd import _lib
    from pytorch_segmentation_amd.utils.datasets import MEAN, STD
    photo = _photos([(40, 60)], 2)[0]
    src = torch.from_numpy(photo.reshape(-1)).to(DEV)
    h, w = WIN
    good = [0, 40, 60, 0, 40, 60, 8, 12]
    rows = [good,
            [0, 40, 60, 2, 40, 60, 8, 12],                   # a flag bit that flag_mask does not declare
            [0, 40, 60, 0, 40, 60, -1, 12],                  # negative origin
            [0, 40, 60, 0, 40, 60, 8, -1],
            [0, 40, 60, 0, 40, 60, 40, 12],                  # origin at / beyond the working image
            [0, 40, 60, 0, 40, 60, 8, 60],
            [0, 40, 60, 0, 20, 30, 20, 12],                  # ... of a scaled working image
            [3, 40, 60, 0, 40, 60, 8, 12],                   # the photo leaves src by three bytes
            [0, 40, 60, 0, 0, 60, 0, 0],                     # working size outside [1, 65535]
            [0, 40, 60, 0, 40, 65536, 0, 0],
            [0, 40, 60, 1, 20, 30, 19, 29]]                  # good again: mirrored, the working image's last pixel
    per, guard = 3 * h * w, 256
    big = torch.full((guard + len(rows) * per + guard,), -7.0, device=DEV)
    _lib.call('pseg_image_preprocess_windows', src.data_ptr(), src.numel(), _rows(rows).data_ptr(), len(rows), 1, 1, *MEAN, *STD,
              big[guard:].data_ptr(), h, w, torch.cuda.current_stream().cuda_stream)
    out = big[guard:guard + len(rows) * per].view(len(rows), 3, h, w)
    assert (out[0] != -7.0).all() and (out[-1] != -7.0).all()
    assert (out[1:-1] == -7.0).all()                         # nothing written for a skipped row
    assert (big[:guard] == -7.0).all() and (big[-guard:] == -7.0).all()
    assert (out[-1, :, 0, w - 1] != 0).any() and (out[-1, :, 0, :w - 1] == 0).all() and (out[-1, :, 1:] == 0).all()


# ------------------------------------------------------------------ decode against float64
DEC_SIZES = [(75, 100), (32, 48), (20, 30), (33, 49), (1, 1), (97, 61), (77, 117)]   # the last: 3 x 3 covering windows
DEC_SCALES = (1.0, 0.5)


@functools.lru_cache(maxsize=2)
def _case(C, pairs):
    """Seeded per-window logits for every (scale, photo) group of DEC_SIZES and the float64 prediction from them ->
    (logits[s][b], work sizes[s][b], [(mask, margin) per photo], largest number of windows covering a working pixel)"""
    h, w = WIN
    g = torch.Generator().manual_seed(C)
    logits, work = [], []
    for s in DEC_SCALES:
        work.append([slide_ref.work_size(H, W, s) for H, W in DEC_SIZES])
        logits.append([torch.randn(len(slide_ref.grid(Hs, Ws, h, w, *STRIDE)[0]) * (2 if pairs else 1), C, h, w, generator=g) * 3
                       for Hs, Ws in work[-1]])
    oracle, cover = [], 0
    for b, (H, W) in enumerate(DEC_SIZES):
        probs = []
        for s in range(len(DEC_SCALES)):
            p, cnt = slide_ref.working_prob64(slide_ref.window_prob64(logits[s][b], pairs), *work[s][b], h, w, *STRIDE)
            probs.append(p)
            cover = max(cover, int(cnt.max()))
        oracle.append(slide_ref.slide_oracle(probs, H, W))
    return logits, work, oracle, cover


def _pack_groups(logits, work, pairs):
    """ops.softmax_views of every group into one packed buffer -> (prob, device group table [S,B,3])"""
    from pytorch_segmentation_amd import ops
    h, w = WIN
    CP = ops.class_pad(logits[0][0].shape[1])
    V = 2 if pairs else 1
    total = sum(lg.shape[0] // V for row in logits for lg in row) * h * w * CP
    prob = torch.full((total,), float('nan'), device=DEV)
    groups, off = [], 0
    for row, sizes in zip(logits, work):
        for lg, (Hs, Ws) in zip(row, sizes):
            ops.softmax_views(lg.to(DEV).contiguous(), prob, off, pairs)
            groups.append([off, Hs, Ws])
            off += lg.shape[0] // V * h * w * CP
    assert off == total
    return prob, torch.tensor(groups, dtype=torch.int64, device=DEV).view(len(logits), len(logits[0]), 3)


def _packed_table(sizes, start=0, gap=0):
    rows, o = [], start
    for H, W in sizes:
        rows.append([o, H, W])
        o += H * W + gap
    return rows, o


@pytest.mark.parametrize('pairs', [0, 1])
@pytest.mark.parametrize('C', [1, 2, 21, 150, 256])
def test_decode_windows_vs_float64(pkg, C, pairs):
    from pytorch_segmentation_amd import ops
    logits, work, oracle, cover = _case(C, pairs)
    assert cover == 9
    g = torch.Generator().manual_seed(1000 + C)
    lut = torch.randint(0, 256, (256, 3), dtype=torch.uint8, generator=g)
    prob, groups = _pack_groups(logits, work, pairs)
    rows, total = _packed_table(DEC_SIZES)
    table = torch.tensor(rows, dtype=torch.int64, device=DEV)
    max_hw = (max(H for H, _ in DEC_SIZES), max(W for _, W in DEC_SIZES))
    mask, rgb = ops.seg_decode_windows(prob, groups, len(DEC_SIZES), C, WIN, STRIDE, table, total, max_hw, lut.to(DEV))
    assert mask.dtype == torch.uint8
    mask, rgb = mask.cpu(), rgb.cpu()
    K = len(DEC_SCALES) * (2 if pairs else 1)
    n_safe = n_all = 0
    for (o, H, W), (want, margin) in zip(rows, oracle):
        got = mask[o:o + H * W].view(H, W).long()
        safe = margin > 1e-6 * K                             # 1e-6 per unit of probability mass (tests/test_tta_gpu.py)
        assert torch.equal(got[safe], want[safe]), ((H, W), (got[safe] != want[safe]).sum().item())
        assert torch.equal(rgb[o:o + H * W].view(H, W, 3), lut[got])
        n_safe += safe.sum().item()
        n_all += H * W
    print('decode windows C=%d pairs=%d: safe share %.5f' % (C, pairs, n_safe / n_all))
    assert n_safe >= 0.99 * n_all, (n_safe, n_all)


def test_one_window_per_photo_is_the_ensemble(pkg):
    """Every working size equal to the window: group (s, b) is row b of map s, and the prediction is seg_decode_ensemble's
    on the same packed buffer.  The two kernels blend the four taps in different association (the windows kernel folds the
    row and column weights), so equality is asserted where the float64 margin is safe, and the rest is printed."""
    from pytorch_segmentation_amd import ops
    C, (h, w) = 21, WIN
    sizes = [(150, 200), (32, 48), (8, 12), (1, 1), (203, 97)]
    g = torch.Generator().manual_seed(7)
    logits = [torch.randn(len(sizes), C, h, w, generator=g) * 3 for _ in range(2)]
    prob, maps, _ = _maps(logits, 0)
    ens, _ = _decode(prob, maps, sizes, C)
    CP = ops.class_pad(C)
    groups = torch.tensor([[[int(maps[s, 0]) + b * h * w * CP, h, w] for b in range(len(sizes))] for s in range(2)],
                          dtype=torch.int64, device=DEV)
    rows, total = _packed_table(sizes)
    mask, _ = ops.seg_decode_windows(prob, groups, len(sizes), C, WIN, STRIDE, torch.tensor(rows, dtype=torch.int64, device=DEV),
                                     total, (203, 200))
    mask = mask.cpu()
    p64s = [_prob64(lg, 0) for lg in logits]
    differ = 0
    for i, (o, H, W) in enumerate(rows):
        got = mask[o:o + H * W].view(H, W).long()
        _, margin = _ensemble_oracle(p64s, i, H, W)
        safe = margin > 1e-6 * 2
        assert torch.equal(got[safe], ens[i][safe]), i
        assert safe.float().mean() > 0.99 or H * W < 200
        differ += (got != ens[i]).sum().item()
    print('one window per photo: %d of %d pixels differ from seg_decode_ensemble' % (differ, total))


def test_ragged_batch_and_bad_records(pkg):
    """Photos with gaps between them, a record whose extent leaves the mask buffer, a photo above Hmax, and one photo with
    one bad group record: every valid photo is right, and no byte outside a valid photo's range changes."""
    from pytorch_segmentation_amd import ops
    C = 21
    logits, work, oracle, _ = _case(C, 0)
    g = torch.Generator().manual_seed(3)
    lut = torch.randint(0, 256, (256, 3), dtype=torch.uint8, generator=g)
    prob, groups = _pack_groups(logits, work, 0)
    rows, o = _packed_table(DEC_SIZES, start=5, gap=7)
    total = o + 50
    nb = len(DEC_SIZES)
    rows.append([o, 8, 12])                                  # 96 pixels into the 50 bytes that are left: leaves the buffer
    rows.append([0, 300, 61])                                # taller than Hmax: skipped, although it fits the buffer
    groups = torch.cat([groups, groups[:, :2]], 1).contiguous()      # the two extra photos have valid groups of their own
    table = torch.tensor(rows, dtype=torch.int64, device=DEV)
    guard = 64
    bad_photo = 3
    bads = {'none': None,
            'misaligned offset': (1, 0, int(groups[1, bad_photo, 0]) + 2),
            'leaves prob': (0, 0, prob.numel() - 8),
            'size 0': (1, 1, 0),
            'size 65536': (0, 2, 65536)}
    for what, bad in bads.items():
        gr = groups.clone()
        if bad is not None:
            gr[bad[0], bad_photo, bad[1]] = bad[2]
        big = torch.full((guard + 4 * total + guard,), 0xAB, dtype=torch.uint8, device=DEV)
        ops.seg_decode_windows(prob, gr, len(rows), C, WIN, STRIDE, table, total, (97, 117), lut.to(DEV),
                               out=big[guard:guard + 4 * total])
        big = big.cpu()
        mask, rgb = big[guard:guard + total], big[guard + total:guard + 4 * total].view(total, 3)
        touched = torch.zeros(total, dtype=torch.bool)
        for i, ((of, H, W), (want, margin)) in enumerate(zip(rows[:nb], oracle)):
            if bad is not None and i == bad_photo:
                continue                                     # only this photo is unwritten
            got = mask[of:of + H * W].view(H, W).long()
            safe = margin > 1e-6 * 2
            assert torch.equal(got[safe], want[safe]), (what, i)
            assert torch.equal(rgb[of:of + H * W].view(H, W, 3), lut[got]), (what, i)
            touched[of:of + H * W] = True
        assert (mask[~touched] == 0xAB).all() and (rgb[~touched] == 0xAB).all(), what
        assert (big[:guard] == 0xAB).all() and (big[-guard:] == 0xAB).all(), what


# ------------------------------------------------------------------ end to end
E2E_SIZES = [(100, 130), (64, 64), (77, 50), (40, 150)]
E2E_SCALES = (1.0, 0.5)


def _slide_oracle_of_model(ref64, photos, S, scales, flip):
    """float64 restatement of inference(slide=True) around the float64 oracle model: the working images are the device
    preprocess's (held bit for bit above), the windows slices of them, zero beyond -> ([(mask, margin)], peak |logit|).
    The peak is the one LOGIT_TOL is relative to: the largest |logit| that enters the prediction.  In tests/test_tta_gpu.py
    that is every logit of every view; here the logits at window positions outside the working image are never sampled
    (the contract says so), so they do not count -- a smaller peak, hence a smaller margin threshold and MORE pixels on
    which the masks must agree."""
    from pytorch_segmentation_amd import ops
    from pytorch_segmentation_amd.utils.datasets import MEAN, STD
    from pytorch_segmentation_amd.utils.inference import slide_strides
    sy, sx = slide_strides(S, S)
    src, offs = _src(photos)
    out, peak = [], 0.0
    for o, p in zip(offs, photos):
        H, W = p.shape[:2]
        probs = []
        for s in scales:
            Hs, Ws = slide_ref.work_size(H, W, s)
            img = ops.image_preprocess_windows(src, _rows([[o, H, W, 0, Hs, Ws, 0, 0]]), Hs, Ws, MEAN, STD, True)[0].cpu().double()
            img = F.pad(img, (0, max(S - Ws, 0), 0, max(S - Hs, 0)))
            origins = slide_ref.grid(Hs, Ws, S, S, sy, sx)[0]
            wins = torch.stack([img[:, y0:y0 + S, x0:x0 + S] for y0, x0 in origins])
            if flip:
                wins = torch.cat([wins, wins.flip(3)])
            with torch.no_grad():
                logits64 = ref64(wins)
            for k, (y0, x0) in enumerate(origins):           # the peak of the logits that enter the prediction
                hh, ww = min(S, Hs - y0), min(S, Ws - x0)
                peak = max(peak, logits64[k, :, :hh, :ww].abs().max().item())
                if flip:
                    peak = max(peak, logits64[len(origins) + k, :, :hh, S - ww:].abs().max().item())
            probs.append(slide_ref.working_prob64(slide_ref.window_prob64(logits64, flip), Hs, Ws, S, S, sy, sx)[0])
        out.append(slide_ref.slide_oracle(probs, H, W))
    return out, peak


@pytest.mark.parametrize('name,nc', [('deeplabv3plus', 21), ('unet', 2)])
def test_inference_slide_end_to_end(pkg, name, nc):
    """Masks of inference(slide=True, scales=(1.0, 0.5), flip=True), fp32 and half, against the float64 restatement on the
    pixels whose margin is safe, with LOGIT_TOL / HALF_LOGIT_TOL and the safe-share floors (0.5 / 0.2) of
    tests/test_tta_gpu.py.

    The peak logit is taken over the logits the decode samples (_slide_oracle_of_model).  DeepLabV3+'s largest logits, up
    to 22.8, lie in the zero-padded part of the 0.5-scale windows, outside the working image; the largest sampled one is
    17.1.  With 22.8 the half threshold 2 * HALF_LOGIT_TOL * peak * K would be 3.65 of the K = 4 units of summed probability
    and the float64 oracle's own half safe share 0.077, under the 0.2 floor, whatever the device computes; with 17.1 the
    oracle's share is 0.48 and the masks are held to it on six times as many pixels."""
    from pytorch_segmentation_amd.utils import VOC_COLORMAP, inference
    S = 64
    m, ref = _models(name, nc, S)
    photos = _photos(E2E_SIZES, 11)
    kw = dict(slide=True, scales=E2E_SCALES, flip=True)
    masks = inference(m, photos, (S, S), **kw)
    masks_h = inference(m, photos, (S, S), half=True, **kw)
    masks_1 = inference(m, photos, (S, S), window_batch=1, **kw)
    masks_7 = inference(m, photos, (S, S), window_batch=7, **kw)     # chunks that cross photo and scale boundaries
    oracle, peak = _slide_oracle_of_model(copy.deepcopy(ref).double(), photos, S, E2E_SCALES, True)
    K = 2 * len(E2E_SCALES)
    fracs = []
    for i, ((H, W), (want, margin)) in enumerate(zip(E2E_SIZES, oracle)):
        assert masks[i].shape == (H, W) and masks[i].dtype == np.int64
        safe = (margin > 2 * LOGIT_TOL * peak * K).numpy()
        assert np.array_equal(masks[i][safe], want.numpy()[safe]), i
        assert np.array_equal(masks_1[i][safe], masks[i][safe]) and np.array_equal(masks_7[i][safe], masks[i][safe]), i
        hsafe = (margin > 2 * HALF_LOGIT_TOL * peak * K).numpy()
        assert np.array_equal(masks_h[i][hsafe], want.numpy()[hsafe]), i
        fracs.append((safe.mean(), hsafe.mean()))
    print('%s: safe-margin fraction fp32 %.3f, half %.3f' % (name, np.mean([f[0] for f in fracs]), np.mean([f[1] for f in fracs])))
    # the windows are really used: not the whole photo squeezed into the input
    plain = inference(m, photos, (S, S))
    assert any((a != b).any() for a, b in zip(masks, plain))
    # colours ride along as in the single-view call
    masks2, colored = inference(m, photos, (S, S), colors=VOC_COLORMAP, **kw)
    for a, b, c in zip(masks, masks2, colored):
        assert np.array_equal(a, b) and np.array_equal(c, VOC_COLORMAP[a])
    # the safe-share floors of tests/test_tta_gpu.py, last: they are a condition on the float64 oracle alone
    assert np.mean([f[0] for f in fracs]) > 0.5
    assert np.mean([f[1] for f in fracs]) > 0.2


def test_inference_slide_with_regions(pkg):
    """the region pass runs on the decoded slide mask as on the other routes: records and cleaned mask are those of
    tests/regions_ref.py applied to inference(slide=True)'s own mask"""
    from pytorch_segmentation_amd.utils import VOC_COLORMAP, inference
    m, _ = _models('unet', 2, 64)
    photos = _photos(E2E_SIZES[:2], 12)
    kw = dict(slide=True, flip=True)
    raw = inference(m, photos, (64, 64), **kw)
    masks, colored, regions = inference(m, photos, (64, 64), colors=VOC_COLORMAP, min_area=6, connectivity=8, regions=True, **kw)
    for b, (r, got, col, regs) in enumerate(zip(raw, masks, colored, regions)):
        r8 = r.astype(np.uint8)
        want = regions_ref.clean(r8, regions_ref.label(r8, 8), 6, False)
        assert np.array_equal(got, want) and np.array_equal(col, VOC_COLORMAP[got])
        wrec = regions_ref.records(want, regions_ref.label(want, 8), b)
        assert [(d['class'], d['label'], d['area'], d['bbox']) for d in regs] == [(w[0] & 255, w[1], w[2], w[3:7]) for w in wrec]


# ------------------------------------------------------------------ evaluation
def test_predict_mask_windows_is_the_ops_composition(pkg):
    from pytorch_segmentation_amd import ops
    from pytorch_segmentation_amd.utils import predict_mask_windows
    m, _ = _models('unet', 2, 64)
    x = fill.images('slide/eval', (2, 3, 96, 128)).to(DEV)
    S, (sy, sx), out_hw = 64, (43, 43), (100, 90)
    got = predict_mask_windows(m, x, out_hw, (S, S), None, (1.0, 0.5), True)
    assert got.shape == (2, 100, 90) and got.dtype == torch.int64
    logits, work = [], []
    with torch.no_grad():
        for hw in [(96, 128), (48, 64)]:                      # 0.5: lower than the window, zero-padded
            v = x if hw == (96, 128) else F.interpolate(x, hw, mode='bilinear', align_corners=False)
            v = F.pad(v, (0, max(S - hw[1], 0), 0, max(S - hw[0], 0)))
            row = []
            for b in range(2):
                wins = torch.stack([v[b, :, y0:y0 + S, x0:x0 + S] for y0, x0 in slide_ref.grid(hw[0], hw[1], S, S, sy, sx)[0]])
                row.append(m(torch.cat([wins, wins.flip(3)]).contiguous()).float())
            logits.append(row)
            work.append([hw, hw])
    CP = ops.class_pad(2)
    total = sum(lg.shape[0] // 2 for row in logits for lg in row) * S * S * CP
    prob, groups, off = torch.empty(total, device=DEV), [], 0
    for row, sizes in zip(logits, work):
        for lg, (Hs, Ws) in zip(row, sizes):
            ops.softmax_views(lg.contiguous(), prob, off, True)
            groups.append([off, Hs, Ws])
            off += lg.shape[0] // 2 * S * S * CP
    rows, npix = _packed_table([out_hw] * 2)
    mask, _ = ops.seg_decode_windows(prob, torch.tensor(groups, dtype=torch.int64, device=DEV).view(2, 2, 3), 2, 2, (S, S), (sy, sx),
                                     torch.tensor(rows, dtype=torch.int64, device=DEV), npix, out_hw)
    assert torch.equal(got, mask.view(2, 100, 90).long())
    whole = m(x).float().argmax(1)
    single = predict_mask_windows(m, x, (96, 128), (S, S))
    assert single.shape == whole.shape and (single != whole).any()


def test_evaluation_with_windows(pkg, tmp_path, monkeypatch):
    from torch.utils.data import DataLoader
    from pytorch_segmentation_amd.utils import Fetcher, predict_mask, predict_mask_windows
    from pytorch_segmentation_amd.utils.datasets import CocoDataset, make_synthetic_coco
    spec = importlib.util.spec_from_file_location('pseg_slide_eval_cli', os.path.join(REPO, 'test.py'))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    root = make_synthetic_coco(str(tmp_path / 'data'), n_train=1, n_val=4, n_classes=1)
    data = CocoDataset(os.path.join(root, 'val.json'), img_size=[96, 96], augments=None)
    fetcher = Fetcher(DataLoader(data, batch_size=2, num_workers=0), post_fetch_fn=data.post_fetch_fn)
    m, _ = _models('unet', 2, 64)
    seen = []
    monkeypatch.setattr(cli, 'all_reduce_counters', lambda c: seen.append(c.clone()))

    def counted(predict):
        c = torch.zeros(3, 2, dtype=torch.int64)
        for inputs, targets in fetcher:
            p, t = predict(inputs, targets).cpu(), targets.cpu().long()
            for k in range(2):
                c[0, k] += ((p == k) & (t == k)).sum()
                c[1, k] += ((p != k) & (t == k)).sum()
                c[2, k] += ((p == k) & (t != k)).sum()
        return c

    miou = cli.test(m, fetcher, window=(64, 64), stride=(32, 48), scales=(1.0, 0.5), flip=True)
    assert isinstance(miou, float) and 0.0 <= miou <= 1.0
    want = counted(lambda x, t: predict_mask_windows(m, x, t.shape[1:], (64, 64), (48, 32), (1.0, 0.5), True))
    assert torch.equal(seen[-1].cpu(), want) and int(want[:2].sum()) == 4 * 96 * 96
    cli.test(m, fetcher, window=(64, 64))
    want_default = counted(lambda x, t: predict_mask_windows(m, x, t.shape[1:], (64, 64)))
    assert torch.equal(seen[-1].cpu(), want_default)
    # window=None: test()'s numbers as they are
    plain = cli.test(m, fetcher)
    want_plain = counted(lambda x, t: predict_mask(m(x)))
    assert torch.equal(seen[-1].cpu(), want_plain) and 0.0 <= plain <= 1.0
    assert not torch.equal(want_plain, want_default)
