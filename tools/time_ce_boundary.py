"""Timing of the boundary-weighted cross-entropy (pseg_ce_opts_binned_fwd_bwd, csrc/ce_opts.hip) with HIP events, at
16 x 21 x 512 x 512 and 8 x 2 x 256 x 256.

    python tools/time_ce_boundary.py [--out FILE.json] [--iters N]

Per shape, on the same logits (N(0, 2)), labels (Voronoi cells of 24 random sites per image, classes cycling, 5 % of the
pixels ignored in square patches), class weights (linspace(0.25, 2, C)), eps = 0.1, gamma = 2, and the 'gaussian' table with
boost 2 at the width the evaluation's rule gives (boundary_width(hw, 0.02): 14 and 7 pixels):
  * `pseg_label_depth`: the depth map of the target alone (two launches, uint8 out);
  * `pseg_ce_opts_binned_fwd_bwd` (loss + dlogits; the depth map already there) at keep_ratio 1 and 0.25;
  * `pseg_ce_opts_fwd_bwd` with the same options on the same inputs, at keep_ratio 1 and 0.25: the binned call's yardstick --
    the derived expectation is the extra byte per pixel, about 1 % of the bytes moved at C = 21;
  * `boundary loss, HIP`: pseg_label_depth + the binned call, what a training step pays;
  * `torch ops`: the same loss from torch ops on the same GPU, forward + backward.  The formulation timed: the depth as
    1 + sum_{k=1..d} [max_k == min_k] with max_k / min_k the k-times iterated 3 x 3 F.max_pool2d(padding=1) of the labels
    as fp32 and of their negation (2 d poolings; -inf padding makes the image border no contour), u = table[depth], then
    F.cross_entropy(weight=, label_smoothing=, reduction='none') times (1 - p_t)^2 times u, torch.topk over the detached
    values for keep 0.25, and sum / sum of u w_t.
Each figure is the median over --iters single calls, each between its own pair of events, after warm-up; the variants
alternate inside one loop so that they see the same machine.  Before timing, the torch depth must equal
pseg_label_depth's bytes and the losses must agree to 1e-4 relative.
"""
import argparse
import json
import math
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_segmentation_amd import ops  # noqa: E402
from pytorch_segmentation_amd.utils import boundary_weight_table, boundary_width  # noqa: E402
from tools.time_lovasz import timed_median  # noqa: E402

EPS, GAMMA, BOOST = 0.1, 2.0, 2.0
SHAPES = [(16, 21, 512, 512), (8, 2, 256, 256)]


def make_target(B, C, H, W, g):
    """Voronoi cells on the CPU generator's sites, built on the device; 5 % ignored in 16 x 16 patches"""
    sites = 24
    sy = torch.randint(0, H, (B, sites), generator=g).cuda().view(B, sites, 1, 1)
    sx = torch.randint(0, W, (B, sites), generator=g).cuda().view(B, sites, 1, 1)
    y = torch.arange(H, device='cuda').view(1, 1, H, 1)
    x = torch.arange(W, device='cuda').view(1, 1, 1, W)
    cell = ((y - sy) ** 2 + (x - sx) ** 2).argmin(1)
    target = (cell + torch.arange(B, device='cuda').view(B, 1, 1)) % C
    patches = (torch.rand(B, H // 16, W // 16, generator=g) < 0.05).cuda()
    target[patches.repeat_interleave(16, 1).repeat_interleave(16, 2)] = -100
    return target.contiguous()


def torch_depth(target, d):
    hi = target.float().unsqueeze(1)
    lo = -hi
    depth = torch.ones_like(hi)
    for _ in range(d):
        hi = F.max_pool2d(hi, 3, 1, 1)
        lo = F.max_pool2d(lo, 3, 1, 1)
        depth += (hi == -lo)
    return depth.squeeze(1).long()


def torch_boundary_ce(logits, target, w, table, d, keep, k):
    """forward + backward of the boundary-weighted loss from torch ops -> (loss, dlogits, depth)"""
    x = logits.detach().requires_grad_(True)
    depth = torch_depth(target, d)
    u = table[depth]
    ell = F.cross_entropy(x, target, weight=w, label_smoothing=EPS, reduction='none')
    pt = torch.exp(-F.cross_entropy(x, target, reduction='none'))
    valid = target != -100
    gq = u * (1 - pt) ** GAMMA * ell
    uw = u * w[target.clamp(min=0)] * valid
    if keep != 1:
        gv = torch.where(valid, gq.detach(), gq.new_full((), -1.0)).reshape(-1)
        # (the count of valid pixels is known to this script: no host synchronisation inside the timed region)
        kept = valid & (gq.detach() >= torch.topk(gv, k).values[-1])
        loss = (gq * kept).sum() / (uw * kept).sum()
    else:
        loss = (gq * valid).sum() / uw.sum()
    loss.backward()
    return loss.detach(), x.grad, depth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'time_ce_boundary.json'))
    ap.add_argument('--iters', type=int, default=20)
    opt = ap.parse_args()
    assert torch.cuda.is_available(), 'time_ce_boundary.py measures on the GPU'
    assert opt.iters >= 10, 'a median over fewer than 10 calls is not reported'
    rows = []
    for B, C, H, W in SHAPES:
        shape = [B, C, H, W]
        g = torch.Generator().manual_seed(0)
        logits = (torch.randn(B, C, H, W, generator=g) * 2).cuda()
        target = make_target(B, C, H, W, g)
        n_valid = int((target != -100).sum())
        k = min(max(int(math.ceil(0.25 * n_valid)), 1), n_valid)
        w = torch.linspace(0.25, 2.0, C).cuda()
        d = boundary_width((H, W), 0.02)
        table = ops.bin_weight_table(boundary_weight_table(d, BOOST, 'gaussian'), 'cuda')
        depth = ops.label_depth(target, C, d, False)
        hist = torch.bincount(depth.reshape(-1).long(), minlength=d + 2)
        rows.append({'name': 'inputs', 'shape': shape, 'd': d, 'n_valid': n_valid,
                     'share_in_band': round(1.0 - hist[d + 1].item() / depth.numel(), 4), 'share_at_depth_1': round(hist[1].item() / depth.numel(), 4)})
        print(json.dumps(rows[-1]), flush=True)

        for keep in (1.0, 0.25):
            out, dl = ops.ce_opts_binned_fwd_bwd(logits, target, depth, table, w, EPS, GAMMA, keep)
            ref, dref, tdepth = torch_boundary_ce(logits, target, w, table, d, keep, k)
            torch.cuda.synchronize()
            assert torch.equal(tdepth, depth.long()), 'the pooled depth and pseg_label_depth disagree'
            check = {'name': 'agreement: keep %g' % keep, 'shape': shape, 'loss_hip': out[0].item(), 'loss_torch': ref.item(),
                     'n_valid': int(out[1].item()), 'n_kept': int(out[3].item()), 'tau': out[4].item(),
                     'grad_max_abs_diff': (dl - dref).abs().max().item(), 'grad_max_abs': dref.abs().max().item()}
            print(json.dumps(check), flush=True)
            assert abs(check['loss_hip'] - check['loss_torch']) <= 1e-4 * abs(check['loss_torch']), 'the kernel and torch disagree'
            rows.append(check)
            del dl, dref, tdepth

        def whole(keep):
            return ops.ce_opts_binned_fwd_bwd(logits, target, ops.label_depth(target, C, d, False), table, w, EPS, GAMMA, keep)

        fns = {'pseg_label_depth': lambda: ops.label_depth(target, C, d, False)}
        for keep in (1.0, 0.25):
            tag = 'keep %g' % keep
            fns['pseg_ce_opts_fwd_bwd, ' + tag] = lambda keep=keep: ops.ce_opts_fwd_bwd(logits, target, w, EPS, GAMMA, keep)
            fns['pseg_ce_opts_binned_fwd_bwd, ' + tag] = lambda keep=keep: ops.ce_opts_binned_fwd_bwd(logits, target, depth, table, w,
                                                                                                    EPS, GAMMA, keep)
            fns['boundary loss, HIP, ' + tag] = lambda keep=keep: whole(keep)
            fns['torch ops, ' + tag] = lambda keep=keep: torch_boundary_ce(logits, target, w, table, d, keep, k)
        med = timed_median(fns, opt.iters)
        for name, (m, lo, hi) in med.items():
            r = {'name': name, 'shape': shape, 'median_ms': round(m, 4), 'min_ms': round(lo, 4), 'max_ms': round(hi, 4),
                 'iters': opt.iters}
            if ', ' in name:
                tag = name.rsplit(', ', 1)[1]
                plain = med['pseg_ce_opts_fwd_bwd, ' + tag][0]
                if name.startswith('pseg_ce_opts_binned'):
                    r['ratio_to_pseg_ce_opts_fwd_bwd'] = round(m / plain, 4)
                    r['extra_ms'] = round(m - plain, 4)
                    # bytes moved per pixel by the unbinned call at keep 1: logits + dlogits + two reads of the target
                    r['derived_extra_bytes_share'] = round(2.0 / (8.0 * C + 16.0), 4) if keep_of(tag) == 1.0 else None
                if name.startswith('boundary loss'):
                    r['torch_over_hip'] = round(med['torch ops, ' + tag][0] / m, 2)
                    r['ratio_to_pseg_ce_opts_fwd_bwd'] = round(m / plain, 4)
            print(json.dumps(r), flush=True)
            rows.append(r)
        del logits, target, depth
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, 'w') as f:
            json.dump(rows, f, indent=1)


def keep_of(tag):
    return float(tag.split(' ')[1])


if __name__ == '__main__':
    main()
