"""Timing of the contour measures (csrc/boundary.hip) with HIP events, at 16 x 512 x 512 (C = 21, d = 14: the headline
evaluation size at the default ratio 0.02) and 16 x 1024 x 2048 (d = 46: Cityscapes-sized).

    python tools/time_boundary.py [--out FILE.json] [--iters N] [--shape B H W C d ...]

Labels are blob maps (nearest of 24 random seeds per image, classes at random) with 0.02 % void specks; the prediction is the
target moved by (2, 3) pixels with 0.5 % of its pixels set to random classes.  Per shape, on the same maps:
  * `pseg_label_depth`: the depth map of the target alone (uint8 out);
  * `pseg_boundary_counts`: the six counter rows of (prediction, target);
  * `pseg_confusion`: the plain tp / fn / fp counters evaluation already takes, on the same pixels;
  * `torch ops`: the same six rows from torch ops on the same GPU -- one-hot fp16 [B, C, H, W], d rounds of
    -max_pool2d(-x, 3, 1) over the zero-padded masks for the bands (and d more, padded with ones, for the trimap), masked sums.
The kernel's counters and the torch ops' must be EQUAL before anything is timed.  Each figure is the median over --iters single
calls, each between its own pair of events, after warm-up; the variants alternate inside one loop so that they see the same
machine.  `bytes` is what a call must move -- each int64 label once, plus the depth bytes written -- and `tb_per_s` is that
over the median: a rate over the required bytes, not a measured traffic."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_segmentation_amd import ops  # noqa: E402

SHAPES = [[16, 512, 512, 21, 14], [16, 1024, 2048, 21, 46]]


def timed_median(fns, iters, warmup=3):
    """{name: fn} -> {name: (median, min, max) ms of `iters` single calls}; the functions alternate call by call"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)] for k in fns}
    for i in range(iters):
        for k, fn in fns.items():
            a, b = ev[k][i]
            a.record()
            fn()
            b.record()
    torch.cuda.synchronize()
    out = {}
    for k in fns:
        ms = [a.elapsed_time(b) for a, b in ev[k]]
        out[k] = (statistics.median(ms), min(ms), max(ms))
    return out


def blob_maps(B, H, W, C, seeds=24, seed=0):
    """(pred, target) int64 [B, H, W] on the GPU"""
    g = torch.Generator(device='cuda').manual_seed(seed)
    y = torch.arange(H, device='cuda').view(H, 1, 1).float()
    x = torch.arange(W, device='cuda').view(1, W, 1).float()
    target = torch.empty(B, H, W, dtype=torch.int64, device='cuda')
    for b in range(B):
        sy = torch.rand(seeds, generator=g, device='cuda') * H
        sx = torch.rand(seeds, generator=g, device='cuda') * W
        cls = torch.randint(0, C, (seeds,), generator=g, device='cuda')
        target[b] = cls[((y - sy) ** 2 + (x - sx) ** 2).argmin(2)]
    pred = torch.roll(target, (2, 3), (1, 2)).contiguous()
    noise = torch.rand(B, H, W, generator=g, device='cuda') < 0.005
    pred[noise] = torch.randint(0, C, (int(noise.sum().item()),), generator=g, device='cuda')
    target[torch.rand(B, H, W, generator=g, device='cuda') < 0.0002] = 255
    return pred, target


def torch_counts(pred, target, C, d):
    """the six counter rows from torch ops: one-hot masks, iterated 3 x 3 erosion, masked sums"""
    valid = (target >= 0) & (target < C)
    pp = torch.where(valid, pred, torch.full_like(pred, -1))
    classes = torch.arange(C, device=pred.device).view(1, C, 1, 1)
    mt, mp = (target.unsqueeze(1) == classes).half(), (pp.unsqueeze(1) == classes).half()

    def erode(m, border):
        for _ in range(d):
            m = -F.max_pool2d(-F.pad(m, (1, 1, 1, 1), value=border), 3, 1)
        return m

    bt, bp = mt * (1 - erode(mt, 0.0)), mp * (1 - erode(mp, 0.0))
    near = mt * (1 - erode(mt, 1.0))                       # the trimap: the image border is no contour
    near_any = near.sum(1, keepdim=True)
    rows = [bt * bp, bt, bp, near * mp, near * (1 - mp), near_any * mp * (1 - mt)]
    return torch.stack([r.sum((0, 2, 3), dtype=torch.float64) for r in rows]).to(torch.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--shape', type=int, nargs='+', default=sum(SHAPES, []), help='B H W C d, repeated')
    opt = ap.parse_args()
    assert torch.cuda.is_available(), 'time_boundary.py measures on the GPU'
    assert opt.iters >= 10, 'a median over fewer than 10 calls is not reported'
    assert len(opt.shape) % 5 == 0, '--shape takes B H W C d, repeated'
    rows = []
    for shape in [opt.shape[i:i + 5] for i in range(0, len(opt.shape), 5)]:
        B, H, W, C, d = shape
        pred, target = blob_maps(B, H, W, C)
        cnt = torch.zeros(6, C, dtype=torch.int64, device='cuda')
        ops.boundary_counts(pred, target, cnt, d)
        ref = torch_counts(pred, target, C, d)
        depth = ops.label_depth(target, C, d, True)
        torch.cuda.synchronize()
        check = {'name': 'agreement', 'shape': shape, 'equal': bool(torch.equal(cnt, ref)),
                 'inter': int(cnt[0].sum()), 'gband': int(cnt[1].sum()), 'pband': int(cnt[2].sum()),
                 'trimap_pixels': int((cnt[3] + cnt[4]).sum()), 'pixels': B * H * W,
                 'share_at_d_plus_1': round((ops.label_depth(target, C, d) == d + 1).float().mean().item(), 4)}
        print(json.dumps(check), flush=True)
        assert check['equal'], 'the kernel and the torch ops disagree: %s vs %s' % (cnt.tolist(), ref.tolist())
        del ref, depth
        rows.append(check)

        conf = torch.zeros(3, C, dtype=torch.int64, device='cuda')
        npix = B * H * W
        moved = {'pseg_label_depth': 9 * npix, 'pseg_boundary_counts': 16 * npix, 'pseg_confusion': 16 * npix}
        fns = {
            'pseg_label_depth': lambda: ops.label_depth(target, C, d, True),
            'pseg_boundary_counts': lambda: ops.boundary_counts(pred, target, cnt, d),
            'pseg_confusion': lambda: ops.confusion(pred.view(-1), target.view(-1), conf),
            'torch ops': lambda: torch_counts(pred, target, C, d),
        }
        for k, (med, lo, hi) in timed_median(fns, opt.iters).items():
            r = {'name': k, 'shape': shape, 'median_ms': round(med, 4), 'min_ms': round(lo, 4), 'max_ms': round(hi, 4),
                 'iters': opt.iters}
            if k in moved:
                r['bytes'] = moved[k]
                r['tb_per_s'] = round(moved[k] / (med * 1e-3) / 1e12, 3)
            print(json.dumps(r), flush=True)
            rows.append(r)
        del pred, target, cnt, conf
        torch.cuda.empty_cache()
    if opt.out:
        with open(opt.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
