"""Timing of the surface (boundary-distance) loss (csrc/surface.hip) with HIP events, at 16 x 21 x 512 x 512 (the headline
training size) and 8 x 2 x 256 x 256 (a small binary-foreground batch).

    python tools/time_surface.py [--out FILE.json] [--iters N] [--shape B C H W ...]

On the same logits (N(0, 2)) and labels (Voronoi cells of 24 random sites per image with a void outline between them), per
shape:
  * `pseg_tversky_fwd_bwd`: the region loss the term sits beside (two reads of the logits, one write): the yardstick;
  * `pseg_class_sdist`: the distance map of the targets (labels in, 4 C bytes per pixel out);
  * `pseg_surface_fwd_bwd`: the loss call given the map, loss + dlogits;
  * `pseg_surface_fwd_bwd, no gradient`: dlogits = NULL;
  * `pseg_class_sdist + pseg_surface_fwd_bwd`: what a training step pays;
  * `torch ops given phi, forward + backward`: the same loss from torch ops on the same GPU given the fp32 phi -- softmax,
    multiply, masked mean, autograd's backward to the logits.
Each figure is the median over --iters single calls, each between its own pair of events, after warm-up; the variants
alternate inside one loop so that they see the same machine.  The two losses are compared first (the values to 1e-5 of
max(1, max|phi|), the gradients to 1e-4 of the largest).  `bytes` is what the call must move and `tb_per_s` is that over
the median: a rate over the required bytes, not a measured traffic."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_segmentation_amd import ops  # noqa: E402
from pytorch_segmentation_amd.utils import signed_distance  # noqa: E402
from time_tversky import timed_median  # noqa: E402

SHAPES = [[16, 21, 512, 512], [8, 2, 256, 256]]
SITES = 24


def voronoi_labels(B, C, H, W, seed=0, ignore_index=-100):
    """int64 [B,H,W]: the class of the nearest of SITES random sites; pixels whose right or lower neighbour lies in another
    cell are ignore_index"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.int32)
    t = np.empty((B, H, W), dtype=np.int64)
    for b in range(B):
        sy, sx, sc = rng.randint(0, H, SITES), rng.randint(0, W, SITES), rng.randint(0, C, SITES)
        best = np.full((H, W), np.iinfo(np.int32).max, dtype=np.int32)
        for y, x, c in zip(sy, sx, sc):
            d = (yy - y) ** 2 + (xx - x) ** 2
            t[b][d < best] = c
            best = np.minimum(best, d)
    edge = np.zeros_like(t, dtype=bool)
    edge[:, :, :-1] |= t[:, :, :-1] != t[:, :, 1:]
    edge[:, :-1, :] |= t[:, :-1, :] != t[:, 1:, :]
    t[edge] = ignore_index
    return torch.from_numpy(t)


def torch_surface(logits, target, phi, ignore_index=-100, backward=True):
    x = logits.detach().requires_grad_(backward)
    C = x.shape[1]
    valid = (target != ignore_index) & (target >= 0) & (target < C)
    loss = ((torch.softmax(x, 1) * phi).sum(1) * valid).sum() / valid.sum().clamp(min=1)
    if backward:
        loss.backward()
        return loss.detach(), x.grad
    return loss, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--shape', type=int, nargs='+', default=sum(SHAPES, []), help='B C H W, repeated')
    opt = ap.parse_args()
    assert torch.cuda.is_available(), 'time_surface.py measures on the GPU'
    assert opt.iters >= 10, 'a median over fewer than 10 calls is not reported'
    assert len(opt.shape) % 4 == 0, '--shape takes B C H W, repeated'
    rows = []
    for shape in [opt.shape[i:i + 4] for i in range(0, len(opt.shape), 4)]:
        B, C, H, W = shape
        g = torch.Generator().manual_seed(0)
        logits = (torch.randn(B, C, H, W, generator=g) * 2).cuda()
        target = voronoi_labels(B, C, H, W).cuda()

        sdist = ops.class_sdist(target, C)
        phi = signed_distance(target, C)
        out, dl = ops.surface_fwd_bwd(logits, target, sdist)
        ref, dref = torch_surface(logits, target, phi)
        torch.cuda.synchronize()
        check = {'name': 'agreement', 'shape': shape, 'loss_hip': out[0].item(), 'loss_torch': ref.item(),
                 'n_valid': int(out[1].item()), 'phi_max': phi.abs().max().item(), 'phi_min': phi.min().item(),
                 'planes_without_contour': int((sdist.view(B, C, -1) == 0).all(2).sum().item()),
                 'grad_max_abs_diff': (dl - dref).abs().max().item(), 'grad_max_abs': dref.abs().max().item()}
        print(json.dumps(check), flush=True)
        assert abs(check['loss_hip'] - check['loss_torch']) <= 1e-5 * max(1.0, check['phi_max']), 'the kernel and the torch ops disagree'
        assert check['grad_max_abs_diff'] <= 1e-4 * check['grad_max_abs'], 'the gradients disagree'
        del dl, dref
        rows.append(check)

        logit_bytes, target_bytes = logits.numel() * 4, target.numel() * 8
        moved = {'pseg_tversky_fwd_bwd': 3 * logit_bytes + 2 * target_bytes,
                 'pseg_class_sdist': target_bytes + logit_bytes,
                 'pseg_surface_fwd_bwd': 5 * logit_bytes + 2 * target_bytes,
                 'pseg_surface_fwd_bwd, no gradient': 2 * logit_bytes + target_bytes}
        fns = {
            'pseg_tversky_fwd_bwd': lambda: ops.tversky_fwd_bwd(logits, target),
            'pseg_class_sdist': lambda: ops.class_sdist(target, C),
            'pseg_surface_fwd_bwd': lambda: ops.surface_fwd_bwd(logits, target, sdist),
            'pseg_surface_fwd_bwd, no gradient': lambda: ops.surface_fwd_bwd(logits, target, sdist, want_grad=False),
            'pseg_class_sdist + pseg_surface_fwd_bwd': lambda: ops.surface_fwd_bwd(logits, target, ops.class_sdist(target, C)),
            'torch ops given phi, forward + backward': lambda: torch_surface(logits, target, phi),
        }
        for k, (med, lo, hi) in timed_median(fns, opt.iters).items():
            r = {'name': k, 'shape': shape, 'median_ms': round(med, 4), 'min_ms': round(lo, 4), 'max_ms': round(hi, 4),
                 'iters': opt.iters}
            if k in moved:
                r['bytes'] = moved[k]
                r['tb_per_s'] = round(moved[k] / (med * 1e-3) / 1e12, 3)
            print(json.dumps(r), flush=True)
            rows.append(r)
        del logits, target, sdist, phi
        torch.cuda.empty_cache()
    if opt.out:
        with open(opt.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
