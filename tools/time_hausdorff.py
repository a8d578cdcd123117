"""Timing of the surface-distance records (csrc/hausdorff.hip) with HIP events, at 16 x 21 x 512 x 512 (the headline
evaluation batch) and 8 x 2 x 256 x 256 (a small binary-foreground batch).

    python tools/time_hausdorff.py [--out FILE.json] [--iters N] [--shape B C H W ...] [--no-cpu]

The target is the Voronoi label map of tools/time_surface.py (24 random sites per image, a void outline between the cells);
the prediction is the target moved by (3, 2) pixels with the outline closed by class 0.  Per shape:
  * `pseg_hausdorff_stats`: the whole call, two label maps in, the [B, C] records out;
  * `pseg_class_sdist`: the signed distance map of the same targets -- the transform the surface loss uses and the only other
    on-device distance transform there is (one map, every class, a [B, C, H, W] result);
  * `update_surface_stats`: the call and the torch ops that fold its records into the [7, C] accumulator;
  * `scipy, CPU`: the same records from scipy.ndimage (binary_erosion, distance_transform_edt) on the host, the label maps
    already there: one run, wall clock.
The device figures are the median over --iters single calls, each between its own pair of events, after warm-up; the variants
alternate inside one loop so that they see the same machine.  The records are compared with scipy's first (integer fields
equal).  The split of the call over its kernels (the row pass against the column pass) is read from a kernel trace of this
script, in a run of its own."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, 'tests'))
from pytorch_segmentation_amd import ops  # noqa: E402
from pytorch_segmentation_amd.utils import update_surface_stats  # noqa: E402
from time_surface import voronoi_labels  # noqa: E402
from time_tversky import timed_median  # noqa: E402

SHAPES = [[16, 21, 512, 512], [8, 2, 256, 256]]


def perturbed(target):
    """the target moved by (3, 2) pixels, its void outline closed by class 0: what a prediction a few pixels off looks like"""
    pred = torch.roll(target, (3, 2), (1, 2))
    pred[pred < 0] = 0
    return pred


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--shape', type=int, nargs='+', default=sum(SHAPES, []), help='B C H W, repeated')
    ap.add_argument('--no-cpu', action='store_true', help='leave the scipy run and the comparison out (kernel traces)')
    opt = ap.parse_args()
    assert torch.cuda.is_available(), 'time_hausdorff.py measures on the GPU'
    assert opt.iters >= 10, 'a median over fewer than 10 calls is not reported'
    assert len(opt.shape) % 4 == 0, '--shape takes B C H W, repeated'
    rows = []
    for shape in [opt.shape[i:i + 4] for i in range(0, len(opt.shape), 4)]:
        B, C, H, W = shape
        t_host = voronoi_labels(B, C, H, W)
        p_host = perturbed(t_host)
        target, pred = t_host.cuda(), p_host.cuda()
        stats, sums = ops.hausdorff_stats(pred, target, C)
        torch.cuda.synchronize()
        active = ((stats[..., 0] > 0) & (stats[..., 1] > 0)).sum().item()
        check = {'name': 'records', 'shape': shape, 'defined': int(active), 'of': B * C,
                 'border_pixels': int(stats[..., :2].sum().item()),
                 'hd_max': float(stats[..., 2:4].max().clamp(min=0).double().sqrt().item())}
        if not opt.no_cpu:
            import hausdorff_ref
            t0 = time.perf_counter()
            ref_stats, ref_sums = hausdorff_ref.stats_scipy(p_host.numpy(), t_host.numpy(), C)
            cpu_ms = (time.perf_counter() - t0) * 1e3
            assert np.array_equal(stats.cpu().numpy(), ref_stats), 'the kernels and scipy disagree'
            np.testing.assert_allclose(sums.cpu().numpy(), ref_sums, rtol=1e-9)
            check['equal_to_scipy'] = True
            rows.append({'name': 'scipy, CPU', 'shape': shape, 'ms': round(cpu_ms, 1), 'runs': 1})
            print(json.dumps(rows[-1]), flush=True)
        print(json.dumps(check), flush=True)
        rows.append(check)
        acc = torch.zeros(7, C, dtype=torch.float64, device='cuda')
        fns = {
            'pseg_hausdorff_stats': lambda: ops.hausdorff_stats(pred, target, C),
            'pseg_class_sdist': lambda: ops.class_sdist(target, C),
            'update_surface_stats': lambda: update_surface_stats(acc, pred, target),
        }
        for k, (med, lo, hi) in timed_median(fns, opt.iters).items():
            r = {'name': k, 'shape': shape, 'median_ms': round(med, 4), 'min_ms': round(lo, 4), 'max_ms': round(hi, 4),
                 'iters': opt.iters}
            print(json.dumps(r), flush=True)
            rows.append(r)
        del target, pred, stats, sums, acc
        torch.cuda.empty_cache()
    if opt.out:
        with open(opt.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
