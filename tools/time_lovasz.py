"""Timing of the Lovasz-softmax loss (csrc/lovasz.hip) with HIP events, at the headline size 16 x 21 x 512 x 512.

    python tools/time_lovasz.py [--out FILE.json] [--iters N] [--shape B C H W]

On the same logits (N(0, 2)) and labels (uniform over the classes, 5 % ignored):
  * `pseg_ce_fwd_bwd`: the cross-entropy call the loss sits beside (loss + dlogits);
  * `pseg_lovasz_softmax_fwd_bwd`: the whole call, loss + dlogits;
  * `pseg_lovasz_softmax_fwd_bwd, no gradient`: dlogits = NULL (no scatter, no softmax backward);
  * `torch ops, forward`: the same loss from torch ops on the same GPU -- softmax, one torch.sort (stable, descending) per
    class, cumsum, the subtracted Jaccard differences -- without a gradient;
  * `torch ops, forward + backward`: that with autograd's backward to the logits.
Each figure is the median over --iters single calls, each between its own pair of events, after warm-up; the variants
alternate inside one loop so that they see the same machine.  The two losses are compared first (they must agree to 1e-4:
the torch form subtracts Jaccard values near 1 in fp32).  `share_of_step` is over the 42.9 ms DeepLabV3+ training step.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_segmentation_amd import ops  # noqa: E402

STEP_MS = 42.9


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


def torch_lovasz(logits, target, ignore_index=-100, backward=False):
    """The loss from torch ops (present classes, whole batch, stable descending sort)."""
    x = logits.detach().requires_grad_(backward)
    C = x.shape[1]
    probs = torch.softmax(x, 1).permute(0, 2, 3, 1).reshape(-1, C)
    t = target.reshape(-1)
    keep = (t != ignore_index) & (t >= 0) & (t < C)
    probs, t = probs[keep], t[keep]
    total, present = x.new_zeros(()), x.new_zeros(())
    for c in range(C):
        fg = (t == c).float()
        n = fg.sum()
        err, perm = torch.sort((fg - probs[:, c]).abs(), descending=True, stable=True)
        fgs = fg[perm]
        inter = n - fgs.cumsum(0)
        union = n + (1 - fgs).cumsum(0)
        jac = 1 - inter / union
        jac = torch.cat([jac[:1], jac[1:] - jac[:-1]])
        has = (n > 0).float()                      # (no host synchronisation: an absent class is weighted by zero)
        total = total + has * (err * jac).sum()
        present = present + has
    loss = total / present.clamp(min=1)
    if backward:
        loss.backward()
        return loss.detach(), x.grad
    return loss, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--shape', type=int, nargs=4, default=[16, 21, 512, 512])
    opt = ap.parse_args()
    assert torch.cuda.is_available(), 'time_lovasz.py measures on the GPU'
    assert opt.iters >= 10, 'a median over fewer than 10 calls is not reported'
    B, C, H, W = opt.shape
    g = torch.Generator().manual_seed(0)
    logits = (torch.randn(B, C, H, W, generator=g) * 2).cuda()
    target = torch.randint(0, C, (B, H, W), generator=g)
    target[torch.rand(B, H, W, generator=g) < 0.05] = -100
    target = target.cuda()

    out, dl = ops.lovasz_softmax_fwd_bwd(logits, target)
    ref, dref = torch_lovasz(logits, target, backward=True)
    torch.cuda.synchronize()
    check = {'name': 'agreement', 'shape': opt.shape, 'loss_hip': out[0].item(), 'loss_torch': ref.item(),
             'n_valid': int(out[1].item()), 'n_present': int(out[3].item()),
             'grad_max_abs_diff': (dl - dref).abs().max().item(), 'grad_max_abs': dref.abs().max().item()}
    print(json.dumps(check), flush=True)
    assert abs(check['loss_hip'] - check['loss_torch']) <= 1e-4, 'the kernel and the torch ops disagree'
    del dl, dref

    fns = {
        'pseg_ce_fwd_bwd': lambda: ops.ce_fwd_bwd(logits, target),
        'pseg_lovasz_softmax_fwd_bwd': lambda: ops.lovasz_softmax_fwd_bwd(logits, target),
        'pseg_lovasz_softmax_fwd_bwd, no gradient': lambda: ops.lovasz_softmax_fwd_bwd(logits, target, want_grad=False),
        'torch ops, forward': lambda: torch_lovasz(logits, target),
        'torch ops, forward + backward': lambda: torch_lovasz(logits, target, backward=True),
    }
    rows = [check]
    for k, (med, lo, hi) in timed_median(fns, opt.iters).items():
        r = {'name': k, 'shape': opt.shape, 'median_ms': round(med, 3), 'min_ms': round(lo, 3), 'max_ms': round(hi, 3),
             'iters': opt.iters, 'share_of_step': round(med / STEP_MS, 3)}
        print(json.dumps(r), flush=True)
        rows.append(r)
    if opt.out:
        with open(opt.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
