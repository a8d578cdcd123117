"""Timing of batched inference (csrc/infer.hip, utils/inference.py) with HIP events.

    python tools/time_inference.py [--out FILE.json] [--iters N]

1. decode: B = 16, C = 21, 512^2 logits -> 1024 x 2048 masks, mask only and mask + RGB, against the torch composition
   softmax -> interpolate -> argmax -> palette gather.  Algorithmic bytes = logits read once + 1 (mask) or 4 (mask + RGB)
   bytes per output pixel.
2. preprocess: 16 photos of 1024 x 2048 x 3 uint8 -> [16, 3, 512, 512] fp32, against interpolate -> round -> normalise in
   torch.  Algorithmic bytes = every photo byte read once + the fp32 output.
3. inference(): DeepLabV3+ (ResNet-50), 21 classes, -s 512 512, B = 16 photos of 1024 x 2048: images/s end to end, and the
   device time apart from the host-to-device copy.
Fractions of the roof are over 6.3 TB/s HBM.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_segmentation_amd import ops  # noqa: E402
from pytorch_segmentation_amd.utils.datasets import MEAN, STD  # noqa: E402

HBM = 6.3e12


def timed(fn, iters, warmup=3):
    """mean ms per call over `iters` calls between two events (after warm-up)"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def row(name, ms, nbytes=None):
    r = {'name': name, 'ms': round(ms, 4)}
    if nbytes:
        r['alg_bytes'] = int(nbytes)
        r['roof_fraction'] = round(nbytes / HBM / (ms * 1e-3), 3)
    print(json.dumps(r), flush=True)
    return r


def decode_rows(iters):
    B, C, h, w, H, W = 16, 21, 512, 512, 1024, 2048
    logits = torch.randn(B, C, h, w, device='cuda') * 3
    table = torch.tensor([[i * H * W, H, W] for i in range(B)], dtype=torch.int64, device='cuda')
    lut = torch.randint(0, 256, (256, 3), dtype=torch.uint8, device='cuda')
    npix = B * H * W
    out = []
    out.append(row('decode mask', timed(lambda: ops.seg_decode(logits, table, npix), iters), logits.numel() * 4 + npix))
    out.append(row('decode mask+rgb', timed(lambda: ops.seg_decode(logits, table, npix, lut), iters),
                   logits.numel() * 4 + 4 * npix))

    def composed():
        p = F.interpolate(logits.softmax(1), (H, W), mode='bilinear', align_corners=False)
        m = p.argmax(1)
        return m.to(torch.uint8), lut[m]
    out.append(row('torch softmax-interpolate-argmax-gather', timed(composed, max(1, iters // 4)), logits.numel() * 4 + 4 * npix))
    m1, _ = ops.seg_decode(logits, table, npix)
    m2, _ = composed()
    out.append({'name': 'decode vs torch fp32 composition: equal pixels', 'fraction': (m1.view(B, H, W) == m2).float().mean().item()})
    print(json.dumps(out[-1]), flush=True)
    return out


def preprocess_rows(iters):
    B, Hs, Ws, oh, ow = 16, 1024, 2048, 512, 512
    src = torch.randint(0, 256, (B * Hs * Ws * 3,), dtype=torch.uint8, device='cuda')
    table = torch.tensor([[i * Hs * Ws * 3, Hs, Ws] for i in range(B)], dtype=torch.int64, device='cuda')
    nbytes = src.numel() + B * 3 * oh * ow * 4
    out = [row('preprocess', timed(lambda: ops.image_preprocess(src, table, oh, ow, MEAN, STD, True), iters), nbytes)]
    mean = torch.tensor(MEAN, device='cuda').view(1, 3, 1, 1)
    std = torch.tensor(STD, device='cuda').view(1, 3, 1, 1)

    def composed():
        x = src.view(B, Hs, Ws, 3).permute(0, 3, 1, 2).flip(1).float()
        v = F.interpolate(x, (oh, ow), mode='bilinear', align_corners=False)
        return (torch.floor(v + 0.5).clamp(0, 255) - mean) / std
    out.append(row('torch interpolate-round-normalise', timed(composed, iters), nbytes))
    return out


def inference_rows(iters):
    from pytorch_segmentation_amd.models import DeepLabV3Plus
    from pytorch_segmentation_amd.utils import inference
    model = DeepLabV3Plus(21).cuda().eval()
    rng = np.random.default_rng(0)
    photos = [rng.integers(0, 256, (1024, 2048, 3), dtype=np.uint8) for _ in range(16)]
    for _ in range(2):
        inference(model, photos, (512, 512))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        inference(model, photos, (512, 512))
    wall = (time.perf_counter() - t0) / iters
    staging = torch.empty(16 * 1024 * 2048 * 3, dtype=torch.uint8, pin_memory=True)
    h2d = timed(lambda: staging.to('cuda', non_blocking=True), iters)
    x = torch.randn(16, 3, 512, 512, device='cuda')
    with torch.no_grad():
        fwd = timed(lambda: model(x), iters, warmup=1)
    out = [{'name': 'inference() DeepLabV3+ R50 C=21 -s 512 512 B=16 from 1024x2048', 'wall_ms': round(wall * 1e3, 2),
            'images_per_s': round(16 / wall, 1), 'h2d_ms': round(h2d, 3), 'model_forward_ms': round(fwd, 3),
            'device_ms_excl_h2d_approx': round(wall * 1e3 - h2d, 2)}]
    print(json.dumps(out[-1]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--skip-model', action='store_true')
    opt = ap.parse_args()
    assert torch.cuda.is_available(), 'time_inference.py measures on the GPU'
    rows = decode_rows(opt.iters) + preprocess_rows(opt.iters)
    if not opt.skip_model:
        rows += inference_rows(max(1, opt.iters // 4))
    if opt.out:
        with open(opt.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
