"""Timing of the local dense-CRF refinement (csrc/crf.hip: ops.crf_refine) with HIP events, at 16 x 21 x 512 x 512 (a
DeepLabV3+ batch) and 8 x 2 x 256 x 256 (a small binary-foreground batch), with the defaults of utils/crf.py.

    python tools/time_crf.py [--out FILE.json] [--iters N] [--shape B C H W ...]

On the same logits (4 x N(0, 1)) and guide (a smooth 8-bit pattern plus noise, normalised with MEAN / STD), per shape:
  * `pseg_softmax_views`: the launch that forms Q^0 (the README's softmax figure at this shape);
  * `pseg_crf_refine, T = 1`: Q^0 and the last iteration (which writes NCHW logits, no softmax);
  * `pseg_crf_refine, T = 5`: the default call; `per inner iteration` = (T = 5 minus T = 1) / 4 -- an iteration that also
    writes Q^t and turns it into the softmax in place;
  * `torch ops, T = 5`: the same iterations from torch ops on the same GPU (shifted slices with in-image masks; the pair
    weights are computed once and kept, 48 maps per image, which the kernel never stores).
Each figure is the median over --iters single calls, each between its own pair of events, after warm-up.  The kernel's and
the torch ops' masks are compared first: they must agree on all but 1e-4 of the pixels (both are fp32; the few are near
ties).  `bytes` is what an inner iteration must move -- Q read once and written once, the logits and the guide read once --
and `tb_per_s` that over the time: a rate over the required bytes, not a measured traffic."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_segmentation_amd import ops  # noqa: E402
from pytorch_segmentation_amd.utils.crf import CRF  # noqa: E402
from pytorch_segmentation_amd.utils.datasets import MEAN, STD  # noqa: E402

SHAPES = [[16, 21, 512, 512], [8, 2, 256, 256]]


def timed(fn, iters, warmup=3):
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
    return statistics.median(ms), min(ms), max(ms)


def shifted(a, oy, ox):
    """a[..., y + oy, x + ox] inside the image, 0 outside"""
    h, w = a.shape[-2:]
    out = torch.zeros_like(a)
    ys, ye, xs, xe = max(0, -oy), min(h, h - oy), max(0, -ox), min(w, w - ox)
    if ys < ye and xs < xe:
        out[..., ys:ye, xs:xe] = a[..., ys + oy:ye + oy, xs + ox:xe + ox]
    return out


def torch_weights(guide, o):
    """-> (offsets, ka [K,B,1,h,w], ks [K,1,1,h,w]) normalised over K: what the iterations reuse"""
    G = guide * torch.tensor(STD, device=guide.device).view(1, 3, 1, 1)
    offs = [(dy * o.dilation, dx * o.dilation) for dy in range(-o.radius, o.radius + 1) for dx in range(-o.radius, o.radius + 1)
            if dy or dx]
    one = torch.ones(1, 1, *guide.shape[2:], device=guide.device)
    ta, tb, tg = o.theta
    ka = torch.stack([shifted(one, oy, ox) * torch.exp(-(oy * oy + ox * ox) / (2 * ta * ta)
                                                        - ((G - shifted(G, oy, ox)) ** 2).sum(1, keepdim=True) / (2 * tb * tb))
                      for oy, ox in offs])
    ks = torch.stack([shifted(one, oy, ox) * torch.exp(torch.tensor(-(oy * oy + ox * ox) / (2 * tg * tg))) for oy, ox in offs])
    return offs, ka / ka.sum(0, keepdim=True), ks / ks.sum(0, keepdim=True)


def torch_refine(logits, weights, o):
    offs, ka, ks = weights
    Q, L = torch.softmax(logits, 1), logits
    for _ in range(o.iters):
        m = torch.zeros_like(logits)
        for k, (oy, ox) in enumerate(offs):
            m += (o.weights[0] * ka[k] + o.weights[1] * ks[k]) * shifted(Q, oy, ox)
        L = logits + m
        Q = torch.softmax(L, 1)
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--shape', type=int, nargs='+', default=sum(SHAPES, []), help='B C H W, repeated')
    opt = ap.parse_args()
    assert torch.cuda.is_available(), 'time_crf.py measures on the GPU'
    iters = max(20, opt.iters)
    assert len(opt.shape) % 4 == 0, '--shape takes B C H W, repeated'
    o = CRF()
    args = (o.radius, o.dilation, o.iters) + o.theta + o.weights
    rows = []

    def row(**r):
        print(json.dumps(r), flush=True)
        rows.append(r)

    for shape in [opt.shape[i:i + 4] for i in range(0, len(opt.shape), 4)]:
        B, C, H, W = shape
        g = torch.Generator().manual_seed(0)
        logits = (torch.randn(B, C, H, W, generator=g) * 4).cuda()
        yy = torch.linspace(0, 6, H).view(1, 1, H, 1)
        xx = torch.linspace(0, 9, W).view(1, 1, 1, W)
        photo = 127.5 + 100 * torch.sin(yy + xx * torch.tensor([1.0, 0.7, 1.3]).view(1, 3, 1, 1)) + 30 * torch.randn(B, 3, H, W, generator=g)
        photo = photo.clamp(0, 255).floor()
        guide = ((photo - torch.tensor(MEAN).view(1, 3, 1, 1)) / torch.tensor(STD).view(1, 3, 1, 1)).cuda().contiguous()
        out = torch.empty_like(logits)

        weights = torch_weights(guide, o)
        got = ops.crf_refine(logits, guide, STD, *args, out=out).argmax(1)
        want = torch_refine(logits, weights, o).argmax(1)
        differ = (got != want).float().mean().item()
        changed = (got != logits.argmax(1)).float().mean().item()
        row(name='agreement', shape=shape, masks_differ=differ, changed_by_refinement=changed)
        assert differ <= 1e-4, 'the kernel and the torch ops disagree on %g of the pixels' % differ
        del got, want

        CP = ops.class_pad(C)
        prob = torch.empty(B * H * W * CP, device='cuda')
        q_bytes, u_bytes, g_bytes = prob.numel() * 4, logits.numel() * 4, guide.numel() * 4
        med, lo, hi = timed(lambda: ops.softmax_views(logits, prob, 0), iters)
        row(name='pseg_softmax_views', shape=shape, median_ms=round(med, 4), min_ms=round(lo, 4), max_ms=round(hi, 4), iters=iters,
            bytes=u_bytes + q_bytes, tb_per_s=round((u_bytes + q_bytes) / (med * 1e-3) / 1e12, 3))
        del prob
        t1 = timed(lambda: ops.crf_refine(logits, guide, STD, o.radius, o.dilation, 1, *o.theta, *o.weights, out=out), iters)
        row(name='pseg_crf_refine, T = 1', shape=shape, median_ms=round(t1[0], 4), min_ms=round(t1[1], 4), max_ms=round(t1[2], 4),
            iters=iters)
        t5 = timed(lambda: ops.crf_refine(logits, guide, STD, *args, out=out), iters)
        row(name='pseg_crf_refine, T = %d' % o.iters, shape=shape, median_ms=round(t5[0], 4), min_ms=round(t5[1], 4),
            max_ms=round(t5[2], 4), iters=iters)
        inner = (t5[0] - t1[0]) / (o.iters - 1)
        moved = 2 * q_bytes + u_bytes + g_bytes
        row(name='per inner iteration', shape=shape, median_ms=round(inner, 4), bytes=moved,
            tb_per_s=round(moved / (inner * 1e-3) / 1e12, 3))
        tt = timed(lambda: torch_refine(logits, weights, o), iters)
        row(name='torch ops, T = %d' % o.iters, shape=shape, median_ms=round(tt[0], 4), min_ms=round(tt[1], 4), max_ms=round(tt[2], 4),
            iters=iters, ratio_to_kernel=round(tt[0] / t5[0], 1))
        del logits, guide, out, weights
        torch.cuda.empty_cache()
    if opt.out:
        with open(opt.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
