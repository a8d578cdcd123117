"""Timing of test-time ensembling (csrc/infer.hip: image_preprocess_views, softmax_views, seg_decode_ensemble;
utils/inference.py) with HIP events.

    python tools/time_tta.py [--out FILE.json] [--iters N] [--skip-model]

B = 16, C = 21, 512 x 512 model input, scales (0.5, 1.0, 1.5) with flipping (6 views), photos of 1024 x 2048.
1. the three kernels, each launch between two events on one stream: median of `iters` (>= 20) runs after warm-up.
   Algorithmic bytes: preprocess = every photo byte once per scale + the fp32 output; softmax = the logits once + the map;
   decode = the three maps once + 1 (mask) or 4 (mask + RGB) bytes per photo pixel.
2. the same ensemble composed from torch ops on the device (softmax, flip, add, interpolate, sum, argmax, palette gather),
   four photos at a time: it materialises a C-channel probability tensor at photo size for every scale.
3. inference(): DeepLabV3+ (ResNet-50), 21 classes, -s 512 512, 16 photos of 1024 x 2048, images/s with and without the
   ensemble.
Fractions of the roof are over 6.3 TB/s HBM.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_segmentation_amd import ops  # noqa: E402
from pytorch_segmentation_amd.utils.datasets import MEAN, STD  # noqa: E402
from pytorch_segmentation_amd.utils.inference import map_offsets, tta_sizes  # noqa: E402

HBM = 6.3e12
B, C, BASE, H, W = 16, 21, (512, 512), 1024, 2048
SCALES = (0.5, 1.0, 1.5)


def timed(fn, iters, warmup=3):
    """median ms of `iters` calls, each between its own pair of events (after warm-up)"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def row(name, ms, nbytes=None):
    r = {'name': name, 'ms': round(ms, 4)}
    if nbytes:
        r['alg_bytes'] = int(nbytes)
        r['bytes_per_s'] = round(nbytes / (ms * 1e-3), -9)
        r['roof_fraction'] = round(nbytes / HBM / (ms * 1e-3), 3)
    print(json.dumps(r), flush=True)
    return r


def kernel_rows(iters):
    sizes = tta_sizes(BASE[0], BASE[1], SCALES)
    CP = ops.class_pad(C)
    out = []
    # preprocess: plain + mirrored rows of every photo
    src = torch.randint(0, 256, (B * H * W * 3,), dtype=torch.uint8, device='cuda')
    views = torch.tensor([[(i % B) * H * W * 3, H, W, i // B] for i in range(2 * B)], dtype=torch.int64, device='cuda')
    total = 0.0
    for hs, ws in sizes:
        ms = timed(lambda: ops.image_preprocess_views(src, views, hs, ws, MEAN, STD, True), iters)
        out.append(row('preprocess_views %dx%d (32 rows)' % (hs, ws), ms, src.numel() + 2 * B * 3 * hs * ws * 4))
        total += ms
    del src
    # softmax: both views of a pair into one map
    offs, cells = map_offsets(B, sizes)
    prob = torch.empty(cells * CP, device='cuda')
    logits = [torch.randn(2 * B, C, hs, ws, device='cuda') * 3 for hs, ws in sizes]
    for lg, of in zip(logits, offs):
        ms = timed(lambda: ops.softmax_views(lg, prob, of * CP, True), iters)
        out.append(row('softmax_views %dx%d (pairs)' % tuple(lg.shape[2:]), ms, lg.numel() * 4 + B * lg.shape[2] * lg.shape[3] * CP * 4))
        total += ms
    # decode
    maps = torch.tensor([[of * CP, hs, ws] for of, (hs, ws) in zip(offs, sizes)], dtype=torch.int64, device='cuda')
    table = torch.tensor([[i * H * W, H, W] for i in range(B)], dtype=torch.int64, device='cuda')
    lut = torch.randint(0, 256, (256, 3), dtype=torch.uint8, device='cuda')
    npix = B * H * W
    ms = timed(lambda: ops.seg_decode_ensemble(prob, maps, B, C, table, npix, (H, W)), iters)
    out.append(row('seg_decode_ensemble mask', ms, prob.numel() * 4 + npix))
    total += ms
    ms_rgb = timed(lambda: ops.seg_decode_ensemble(prob, maps, B, C, table, npix, (H, W), lut), iters)
    out.append(row('seg_decode_ensemble mask+rgb', ms_rgb, prob.numel() * 4 + 4 * npix))
    out.append(row('three kernels, all scales (mask only)', total))

    def composed(chunk=4):
        masks = []
        for i in range(0, B, chunk):
            acc = None
            for lg in logits:
                p = lg[i:i + chunk].softmax(1) + lg[B + i:B + i + chunk].softmax(1).flip(3)
                r = F.interpolate(p, (H, W), mode='bilinear', align_corners=False)
                acc = r if acc is None else acc.add_(r)
            masks.append(acc.argmax(1))
        m = torch.cat(masks)
        return m.to(torch.uint8), lut[m]

    def composed_hip():
        for lg, of in zip(logits, offs):
            ops.softmax_views(lg, prob, of * CP, True)
        return ops.seg_decode_ensemble(prob, maps, B, C, table, npix, (H, W), lut)

    t_hip = timed(composed_hip, iters)
    t_torch = timed(composed, max(5, iters // 4), warmup=2)
    out.append(row('softmax_views x3 + seg_decode_ensemble mask+rgb', t_hip))
    out.append(row('torch softmax-flip-add-interpolate-sum-argmax-gather (4 photos at a time)', t_torch))
    m1, _ = composed_hip()
    m2, _ = composed()
    out.append({'name': 'HIP vs torch composition: equal pixels', 'fraction': (m1.view(B, H, W) == m2).float().mean().item(),
                'speedup': round(t_torch / t_hip, 2)})
    print(json.dumps(out[-1]), flush=True)
    return out


def inference_rows(iters):
    from pytorch_segmentation_amd.models import DeepLabV3Plus
    from pytorch_segmentation_amd.utils import inference
    model = DeepLabV3Plus(C).cuda().eval()
    rng = np.random.default_rng(0)
    photos = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(B)]
    out = []
    for name, kw in (('single view', {}), ('scales %s + flip' % (SCALES,), {'scales': SCALES, 'flip': True})):
        for _ in range(2):
            inference(model, photos, BASE, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            inference(model, photos, BASE, **kw)
        wall = (time.perf_counter() - t0) / iters
        out.append({'name': 'inference() DeepLabV3+ R50 C=21 -s 512 512 B=16 from 1024x2048, ' + name,
                    'wall_ms': round(wall * 1e3, 2), 'images_per_s': round(B / wall, 1)})
        print(json.dumps(out[-1]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--skip-model', action='store_true')
    opt = ap.parse_args()
    assert torch.cuda.is_available(), 'time_tta.py measures on the GPU'
    rows = kernel_rows(max(20, opt.iters))
    if not opt.skip_model:
        rows += inference_rows(max(3, opt.iters // 4))
    if opt.out:
        with open(opt.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
