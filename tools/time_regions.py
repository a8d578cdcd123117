"""Timing of the connected-region calls (csrc/regions.hip: mask_label, mask_regions, mask_clean) with HIP events, next
to the decode they are appended to.

    python tools/time_regions.py [--out FILE.json] [--iters N]

B = 16 photos of 1024 x 2048, C = 21 -- the batch of tools/time_tta.py.  Three kinds of mask:
  smooth     low-resolution (32 x 64) random logits through ops.seg_decode: large blobs, what a model gives;
  speckled   an independent random class per pixel: the worst case for the number of unions and of records;
  serpentine one one-pixel-wide path winding over the whole photo: the longest equivalence chain through the border merge.
Each call sits between two events on one stream: median of `iters` (>= 10) runs after warm-up (the serpentine, whose
label call is slow, a third of that, 8-connectivity only).  Algorithmic bytes per
pixel: label = 1 (mask) + 4 (labels); records = 1 + 4 read (+ 96 bytes per record written); clean = 1 + 4 read + 1 (mask)
+ 3 (colours) written.  Every stage in fact touches more: the workspace arrays, and labels that are read more than once.
pseg_seg_decode (single view, 512 x 512 logits, mask + colours) is timed on the same batch for comparison.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_segmentation_amd import ops  # noqa: E402

HBM = 6.3e12
B, C, H, W = 16, 21, 1024, 2048
MIN_AREA = 64


def timed(fn, iters, warmup=2):
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


def row(name, ms, nbytes=None, **extra):
    r = {'name': name, 'ms': round(ms, 4)}
    if nbytes:
        r['alg_bytes'] = int(nbytes)
        r['GB_per_s'] = round(nbytes / (ms * 1e-3) / 1e9, 1)
        r['roof_fraction'] = round(nbytes / HBM / (ms * 1e-3), 4)
    r.update(extra)
    print(json.dumps(r), flush=True)
    return r


def serpentine():
    m = np.zeros((H, W), np.uint8)
    for k, y in enumerate(range(1, H - 1, 2)):
        m[y, 1:W - 1] = 1
        if y + 2 < H - 1:
            m[y + 1, W - 2 if k % 2 == 0 else 1] = 1
    return torch.from_numpy(np.tile(m.reshape(-1), B)).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='')
    ap.add_argument('--iters', type=int, default=10)
    opt = ap.parse_args()
    assert torch.cuda.is_available(), 'time_regions.py measures on the GPU'
    iters = max(10, opt.iters)
    npix = B * H * W
    table = torch.tensor([[i * H * W, H, W] for i in range(B)], dtype=torch.int64, device='cuda')
    lut = torch.randint(0, 256, (256, 3), dtype=torch.uint8, device='cuda')
    torch.manual_seed(0)
    rows = []

    logits = torch.randn(B, C, 512, 512, device='cuda') * 3
    out4 = torch.empty(4 * npix, dtype=torch.uint8, device='cuda')
    ms_dec = timed(lambda: ops.seg_decode(logits, table, npix, lut, out=out4), iters)
    rows.append(row('seg_decode 512x512 -> 1024x2048 mask+rgb', ms_dec, logits.numel() * 4 + 4 * npix))
    del logits

    low = torch.randn(B, C, 32, 64, device='cuda') * 3
    smooth = ops.seg_decode(low, table, npix)[0].clone()
    masks = {'smooth': smooth, 'speckled': torch.randint(0, C, (npix,), dtype=torch.uint8, device='cuda'),
             'serpentine': serpentine()}
    full_iters = iters
    for name, mask in masks.items():
        iters = full_iters if name != 'serpentine' else max(3, full_iters // 3)
        for conn in ((8, 4) if name != 'serpentine' else (8,)):
            labels = torch.empty(npix, dtype=torch.int32, device='cuda')
            ms_l = timed(lambda: ops.mask_label(mask, table, npix, (H, W), conn, out=labels), iters)
            _, count = ops.mask_regions(mask, labels, table, npix, (H, W), 0)
            n = int(count.item())
            rows.append(row('%s: mask_label, connectivity %d' % (name, conn), ms_l, 5 * npix, components=n))
            if conn == 4:
                continue
            cap = min(n, 1 << 22)
            records = torch.empty(max(cap, 1), ops.REGION_WORDS, dtype=torch.int64, device='cuda')
            ms_r = timed(lambda: ops.mask_regions(mask, labels, table, npix, (H, W), cap, records=records, count=count), iters)
            rows.append(row('%s: mask_regions (capacity %d)' % (name, cap), ms_r, 5 * npix + 96 * cap))
            ms_c = timed(lambda: ops.mask_clean(mask, labels, table, npix, (H, W), MIN_AREA, False, lut, out=out4), iters)
            rows.append(row('%s: mask_clean min_area %d, mask+rgb' % (name, MIN_AREA), ms_c, 9 * npix))
            ms_cl = timed(lambda: ops.mask_clean(mask, labels, table, npix, (H, W), MIN_AREA, True, lut, out=out4), iters)
            rows.append(row('%s: mask_clean min_area %d + largest_only, mask+rgb' % (name, MIN_AREA), ms_cl, 9 * npix))
            rows.append(row('%s: label + clean + relabel + records' % name, 2 * ms_l + ms_c + ms_r, None,
                            times_decode=round((2 * ms_l + ms_c + ms_r) / ms_dec, 2)))
            del records
    if opt.out:
        with open(opt.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
