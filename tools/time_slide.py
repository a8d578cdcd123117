"""Timing of sliding-window inference (csrc/infer.hip: image_preprocess_windows, softmax_views, seg_decode_windows;
utils/inference.py) with HIP events.

    python tools/time_slide.py [--out FILE.json] [--iters N] [--skip-model]

B = 16 photos of 1024 x 2048, window 512 x 512, C = 21, default stride (342); two configurations: one scale without flip,
and scales 0.75 / 1.0 / 1.25 with flip.
1. the launches, each between two events on one stream, median of `iters` runs after warm-up: one preprocess launch and
   one softmax launch for a chunk of 16 windows (32 rows with flip), and the ONE decode of the whole batch.  Algorithmic
   bytes: preprocess = the fp32 windows written + the photo bytes under them; softmax = the logits once + the maps;
   decode = the packed probability buffer once + one byte per photo pixel.
2. the same prediction from torch ops on the device, photo by photo: slice, softmax (+ flipped twin), accumulate into a
   per-scale C-channel canvas, divide by the count, F.interpolate to the photo's size, sum, argmax.  Both read the same
   random logits (window k of the batch takes row k % 16 of one chunk), and the share of equal pixels is reported.
3. inference(): DeepLabV3+ (ResNet-50), 21 classes, the same 16 photos: single view (-s 512 512), slide=True at one scale,
   slide=True at the three scales with flip.
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
from pytorch_segmentation_amd.utils.inference import slide_strides, window_grid, work_size  # noqa: E402

HBM = 6.3e12
B, C, WIN, H, W = 16, 21, (512, 512), 1024, 2048
CONFIGS = (('one scale', (1.0,), False), ('scales 0.75 / 1.0 / 1.25 + flip', (0.75, 1.0, 1.25), True))


def timed(fn, iters, warmup=2):
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


def kernel_rows(label, scales, flip, iters):
    h, w = WIN
    sy, sx = slide_strides(h, w)
    CP, V = ops.class_pad(C), 2 if flip else 1
    out = []
    # the windows of every (scale, photo) group, scale-major, as inference(slide=True) lays them out
    rows, groups = [], []
    for s in scales:
        Hs, Ws = work_size(H, W, s)
        origins, _ = window_grid(Hs, Ws, h, w, sy, sx)
        for b in range(B):
            groups.append([len(rows) * h * w * CP, Hs, Ws])
            rows += [[b * H * W * 3, H, W, 0, Hs, Ws, y0, x0] for y0, x0 in origins]
    N = len(rows)
    # preprocess: one chunk of B windows (the largest scale's first ones), plain + mirrored rows with flip
    src = torch.randint(0, 256, (B * H * W * 3,), dtype=torch.uint8, device='cuda')
    chunk = rows[-B:]
    table = torch.tensor(chunk + [r[:3] + [ops.VIEW_MIRROR] + r[4:] for r in chunk] * (V - 1), dtype=torch.int64, device='cuda')
    under = sum(3 * h * w * (H / r[4]) * (W / r[5]) for r in chunk)
    ms = timed(lambda: ops.image_preprocess_windows(src, table, h, w, MEAN, STD, True), iters)
    out.append(row('%s: preprocess_windows, %d rows' % (label, len(table)), ms, under + len(table) * 3 * h * w * 4))
    del src
    # softmax: one chunk into the packed buffer
    prob = torch.empty(N * h * w * CP, device='cuda')
    logits = torch.randn(V * B, C, h, w, device='cuda') * 3
    ms = timed(lambda: ops.softmax_views(logits, prob, 0, flip), iters)
    out.append(row('%s: softmax_views, %d windows%s' % (label, B, ' (pairs)' if flip else ''), ms,
                   logits.numel() * 4 + B * h * w * CP * 4))
    assert N % B == 0
    for a in range(0, N, B):                                  # window k of the batch: row k % B of the one chunk
        ops.softmax_views(logits, prob, a * h * w * CP, flip)
    out.append({'name': '%s: %d windows, %d softmax launches for the batch' % (label, N, N // B), 'prob_bytes': prob.numel() * 4})
    print(json.dumps(out[-1]), flush=True)
    # decode
    dgroups = torch.tensor(groups, dtype=torch.int64, device='cuda').view(len(scales), B, 3)
    dtable = torch.tensor([[i * H * W, H, W] for i in range(B)], dtype=torch.int64, device='cuda')
    npix = B * H * W
    t_dec = timed(lambda: ops.seg_decode_windows(prob, dgroups, B, C, WIN, (sy, sx), dtable, npix, (H, W)), iters)
    out.append(row('%s: seg_decode_windows mask' % label, t_dec, prob.numel() * 4 + npix))

    def composed():
        masks = []
        p = logits.softmax(1)
        p = p[:B] + p[B:].flip(3) if flip else p              # the B distinct window maps, once
        for b in range(B):
            acc, k = None, 0
            for si, s in enumerate(scales):
                Hs, Ws = work_size(H, W, s)
                origins, _ = window_grid(Hs, Ws, h, w, sy, sx)
                k = groups[si * B + b][0] // (h * w * CP)
                canvas = torch.zeros(C, Hs, Ws, device='cuda')
                cnt = torch.zeros(1, Hs, Ws, device='cuda')
                for j, (y0, x0) in enumerate(origins):
                    canvas[:, y0:y0 + h, x0:x0 + w] += p[(k + j) % B]
                    cnt[:, y0:y0 + h, x0:x0 + w] += 1
                r = F.interpolate((canvas / cnt)[None], (H, W), mode='bilinear', align_corners=False)
                acc = r if acc is None else acc.add_(r)
            masks.append(acc.argmax(1))
        return torch.cat(masks).to(torch.uint8)

    t_torch = timed(composed, max(3, iters // 4), warmup=1)
    out.append(row('%s: torch softmax-accumulate-divide-interpolate-sum-argmax (softmax of the %d distinct maps once)' % (label, B),
                   t_torch))
    m1, _ = ops.seg_decode_windows(prob, dgroups, B, C, WIN, (sy, sx), dtable, npix, (H, W))
    out.append({'name': '%s: decode vs torch composition' % label, 'equal_pixels': (m1.view(B, H, W) == composed()).float().mean().item(),
                'torch_over_decode': round(t_torch / t_dec, 2)})
    print(json.dumps(out[-1]), flush=True)
    return out


def inference_rows(iters):
    from pytorch_segmentation_amd.models import DeepLabV3Plus
    from pytorch_segmentation_amd.utils import inference
    model = DeepLabV3Plus(C).cuda().eval()
    rng = np.random.default_rng(0)
    photos = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(B)]
    out = []
    cases = [('single view', {}, iters)] + [('slide, ' + label, {'slide': True, 'scales': sc, 'flip': fl}, max(1, iters // (4 if fl else 1)))
                                            for label, sc, fl in CONFIGS]
    for name, kw, n in cases:
        inference(model, photos, WIN, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            inference(model, photos, WIN, **kw)
        wall = (time.perf_counter() - t0) / n
        out.append({'name': 'inference() DeepLabV3+ R50 C=21 -s 512 512 B=16 of 1024x2048, ' + name, 'runs': n,
                    'wall_ms': round(wall * 1e3, 2), 'images_per_s': round(B / wall, 1)})
        print(json.dumps(out[-1]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--skip-model', action='store_true')
    opt = ap.parse_args()
    assert torch.cuda.is_available(), 'time_slide.py measures on the GPU'
    rows = []
    for label, scales, flip in CONFIGS:
        rows += kernel_rows(label, scales, flip, max(10, opt.iters))
        torch.cuda.empty_cache()
    if not opt.skip_model:
        rows += inference_rows(max(2, opt.iters // 5))
    if opt.out:
        with open(opt.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
