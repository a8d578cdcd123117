"""Timing of the configured cross-entropy (csrc/ce_opts.hip) with HIP events, at the headline size 16 x 21 x 512 x 512.

    python tools/time_ce_opts.py [--out FILE.json] [--iters N] [--shape B C H W]

On the same logits (N(0, 2)), labels (uniform over the classes, 5 % ignored) and class weights (linspace(0.25, 2, C)):
  * `pseg_ce_fwd_bwd`: the plain cross-entropy call (loss + dlogits);
  * `pseg_ce_opts_fwd_bwd` (loss + dlogits) in three configurations: `weights + smoothing` (eps = 0.1), `+ gamma 2`, and
    `+ gamma 2, keep 0.25` (the hard-pixel selection: park, four-round radix select, kept sums, gradient pass);
  * `torch ops`: the same three computations from torch ops on the same GPU, forward + backward -- F.cross_entropy(weight=,
    label_smoothing=); that per pixel times (1 - p_t)^2; that with torch.topk over the detached per-pixel values.
Each figure is the median over --iters single calls, each between its own pair of events, after warm-up; the variants
alternate inside one loop so that they see the same machine.  The losses are compared first (1e-4 relative).  The ratios
to `pseg_ce_fwd_bwd` and to the torch form of the same computation are part of each row.
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
from tools.time_lovasz import timed_median  # noqa: E402

EPS = 0.1


def torch_ce_opts(logits, target, w, eps, gamma, keep):
    """forward + backward of the configured loss from torch ops -> (loss, dlogits)"""
    x = logits.detach().requires_grad_(True)
    if gamma == 0 and keep == 1:
        loss = F.cross_entropy(x, target, weight=w, label_smoothing=eps)
    else:
        ell = F.cross_entropy(x, target, weight=w, label_smoothing=eps, reduction='none')
        pt = torch.exp(-F.cross_entropy(x, target, reduction='none'))
        f = (1 - pt) ** gamma * ell
        valid = target != -100
        wt = w[target.clamp(min=0)] * valid
        if keep != 1:
            fv = torch.where(valid, f.detach(), f.new_full((), -1.0)).reshape(-1)
            # (the count of valid pixels is known to this script: no host synchronisation inside the timed region)
            kept = valid & (f.detach() >= torch.topk(fv, torch_ce_opts.k).values[-1])
            loss = (f * kept).sum() / (wt * kept).sum()
        else:
            loss = (f * valid).sum() / wt.sum()
    loss.backward()
    return loss.detach(), x.grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--shape', type=int, nargs=4, default=[16, 21, 512, 512])
    opt = ap.parse_args()
    assert torch.cuda.is_available(), 'time_ce_opts.py measures on the GPU'
    assert opt.iters >= 10, 'a median over fewer than 10 calls is not reported'
    B, C, H, W = opt.shape
    g = torch.Generator().manual_seed(0)
    logits = (torch.randn(B, C, H, W, generator=g) * 2).cuda()
    target = torch.randint(0, C, (B, H, W), generator=g)
    target[torch.rand(B, H, W, generator=g) < 0.05] = -100
    n_valid = int((target != -100).sum())
    target = target.cuda()
    w = torch.linspace(0.25, 2.0, C).cuda()
    configs = {'weights + smoothing': (0.0, 1.0), '+ gamma 2': (2.0, 1.0), '+ gamma 2, keep 0.25': (2.0, 0.25)}
    torch_ce_opts.k = min(max(int(math.ceil(0.25 * n_valid)), 1), n_valid)

    rows = []
    for name, (gamma, keep) in configs.items():
        out, dl = ops.ce_opts_fwd_bwd(logits, target, w, EPS, gamma, keep)
        ref, dref = torch_ce_opts(logits, target, w, EPS, gamma, keep)
        torch.cuda.synchronize()
        check = {'name': 'agreement: ' + name, 'shape': opt.shape, 'loss_hip': out[0].item(), 'loss_torch': ref.item(),
                 'n_valid': int(out[1].item()), 'n_kept': int(out[3].item()), 'tau': out[4].item(),
                 'grad_max_abs_diff': (dl - dref).abs().max().item(), 'grad_max_abs': dref.abs().max().item()}
        print(json.dumps(check), flush=True)
        assert abs(check['loss_hip'] - check['loss_torch']) <= 1e-4 * abs(check['loss_torch']), 'the kernel and torch disagree'
        rows.append(check)
        del dl, dref

    fns = {'pseg_ce_fwd_bwd': lambda: ops.ce_fwd_bwd(logits, target)}
    for name, (gamma, keep) in configs.items():
        fns['pseg_ce_opts_fwd_bwd, ' + name] = lambda gamma=gamma, keep=keep: ops.ce_opts_fwd_bwd(logits, target, w, EPS, gamma, keep)
        fns['torch ops, ' + name] = lambda gamma=gamma, keep=keep: torch_ce_opts(logits, target, w, EPS, gamma, keep)
    med = timed_median(fns, opt.iters)
    base = med['pseg_ce_fwd_bwd'][0]
    for k, (m, lo, hi) in med.items():
        r = {'name': k, 'shape': opt.shape, 'median_ms': round(m, 3), 'min_ms': round(lo, 3), 'max_ms': round(hi, 3),
             'iters': opt.iters, 'ratio_to_pseg_ce_fwd_bwd': round(m / base, 2)}
        if k.startswith('pseg_ce_opts'):
            r['torch_over_hip'] = round(med['torch ops, ' + k.split(', ', 1)[1]][0] / m, 2)
        print(json.dumps(r), flush=True)
        rows.append(r)
    if opt.out:
        with open(opt.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
