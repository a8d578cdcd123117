"""Timing of the outline call (csrc/polygons.hip: mask_rings) with HIP events, next to the label and records calls it
follows on the same buffer, and of the copy back of its result.

    python tools/time_polygons.py [--out FILE.json] [--iters N]

B = 16 photos of 1024 x 2048 -- the batch of tools/time_regions.py.  Two kinds of mask, 8-connectivity:
  smooth   low-resolution (32 x 64) random logits through ops.seg_decode: large blobs, what a model gives;
  voronoi  48 random sites per photo, every pixel takes the class of its nearest site: straight oblique borders, which
           on the lattice are staircases -- many corners per edge.
Each call sits between two events on one stream: median of `iters` (>= 20) runs after warm-up.  The rings call is timed
three times: with max_edges 0 (the per-pixel part alone: crack bits and their scan, 4 launches), with the exact edge count
as capacity, and with the first capacity utils.regions.mask_polygons would use.  R is the number of doubling rounds of
each of the two passes; a round reads 8 bytes per edge in order, gathers 8 bytes per edge and writes 8 per edge.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_segmentation_amd import ops  # noqa: E402

B, C, H, W = 16, 21, 1024, 2048
SITES = 48


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
    return statistics.median(ms)


def row(name, ms, **extra):
    r = {'name': name, 'ms': round(ms, 4)}
    r.update(extra)
    print(json.dumps(r), flush=True)
    return r


def voronoi():
    g = torch.Generator(device='cuda').manual_seed(1)
    yy = torch.arange(H, device='cuda', dtype=torch.float32).view(1, H, 1)
    xx = torch.arange(W, device='cuda', dtype=torch.float32).view(1, 1, W)
    out = torch.empty(B, H, W, dtype=torch.uint8, device='cuda')
    for b in range(B):
        sy = torch.rand(SITES, generator=g, device='cuda').view(-1, 1, 1) * H
        sx = torch.rand(SITES, generator=g, device='cuda').view(-1, 1, 1) * W
        cls = torch.randint(0, C, (SITES,), generator=g, device='cuda', dtype=torch.uint8)
        out[b] = cls[((yy - sy) ** 2 + (xx - sx) ** 2).argmin(0)]
    return out.reshape(-1)


def rounds(cap):
    longest, r = min(cap, 4 * H * W), 0
    while (1 << r) < longest:
        r += 1
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='')
    ap.add_argument('--iters', type=int, default=20)
    opt = ap.parse_args()
    assert torch.cuda.is_available(), 'time_polygons.py measures on the GPU'
    iters = max(20, opt.iters)
    npix = B * H * W
    table = torch.tensor([[i * H * W, H, W] for i in range(B)], dtype=torch.int64, device='cuda')
    torch.manual_seed(0)
    rows = []
    low = torch.randn(B, C, 32, 64, device='cuda') * 3
    masks = {'smooth': ops.seg_decode(low, table, npix)[0].clone(), 'voronoi': voronoi()}
    for name, mask in masks.items():
        labels = torch.empty(npix, dtype=torch.int32, device='cuda')
        ms_l = timed(lambda: ops.mask_label(mask, table, npix, (H, W), 8, out=labels), iters)
        _, count = ops.mask_regions(mask, labels, table, npix, (H, W), 0)
        n = int(count.item())
        rows.append(row('%s: mask_label' % name, ms_l, components=n))
        records = torch.empty(max(n, 1), ops.REGION_WORDS, dtype=torch.int64, device='cuda')
        ms_r = timed(lambda: ops.mask_regions(mask, labels, table, npix, (H, W), n, records=records, count=count), iters)
        rows.append(row('%s: mask_regions (capacity %d)' % (name, n), ms_r))

        counts = torch.empty(3, dtype=torch.int64, device='cuda')
        ms_0 = timed(lambda: ops.mask_rings(mask, labels, table, npix, (H, W), 8, 0, counts=counts), iters)
        edges = int(counts[0].item())
        rows.append(row('%s: mask_rings, max_edges 0 (cracks + scan)' % name, ms_0, edges=edges))
        first = min(4 * npix, 4096 * B + npix // 4)
        for what, cap in (('exact', edges), ('first capacity of mask_polygons', first)):
            if cap < edges:
                rows.append(row('%s: mask_rings, %s: capacity %d below the %d edges' % (name, what, cap, edges), 0.0))
                continue
            rings = torch.empty(cap // 4, ops.RING_WORDS, dtype=torch.int64, device='cuda')
            verts = torch.empty(cap, 2, dtype=torch.int32, device='cuda')
            ms_p = timed(lambda: ops.mask_rings(mask, labels, table, npix, (H, W), 8, cap, rings, verts, counts), iters)
            c = counts.tolist()
            R = rounds(cap)
            rows.append(row('%s: mask_rings, %s (capacity %d)' % (name, what, cap), ms_p, edges=c[0], rings=c[1], vertices=c[2],
                            rounds_per_pass=R, launches=11 + 2 * R, bytes_per_round=24 * c[0],
                            ms_per_round=round((ms_p - ms_0) / (2 * R + 6), 4),
                            ratio_to_label_plus_records=round(ms_p / (ms_l + ms_r), 3)))
            if what == 'exact':
                ms_c = timed(lambda: (rings[:c[1]].cpu(), verts[:c[2]].cpu()), iters)
                rows.append(row('%s: copy back of rings and vertices' % name, ms_c, bytes=48 * c[1] + 8 * c[2]))
            del rings, verts
        del records, labels
    if opt.out:
        with open(opt.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
