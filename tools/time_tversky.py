"""Timing of the Dice / Tversky loss (csrc/tversky.hip) with HIP events, at 16 x 21 x 512 x 512 (the headline training
size) and 8 x 2 x 256 x 256 (a small binary-foreground batch).

    python tools/time_tversky.py [--out FILE.json] [--iters N] [--shape B C H W ...]

On the same logits (N(0, 2)) and labels (uniform over the classes, 5 % ignored), per shape:
  * `pseg_ce_fwd_bwd`: the cross-entropy call the loss sits beside (loss + dlogits: one read, one write);
  * `pseg_tversky_fwd_bwd`: the whole call, loss + dlogits (two reads of the logits, one write);
  * `pseg_tversky_fwd_bwd, no gradient`: dlogits = NULL (one read);
  * `torch ops, forward`: the same loss from torch ops on the same GPU -- softmax, one-hot, masked sums -- without a gradient;
  * `torch ops, forward + backward`: that with autograd's backward to the logits.
Each figure is the median over --iters single calls, each between its own pair of events, after warm-up; the variants
alternate inside one loop so that they see the same machine.  The two losses are compared first (they must agree to 1e-5,
the gradients to 1e-4 of the largest).  `bytes` is what the call must move -- logits once per read and dlogits once, plus the
targets per pass -- and `tb_per_s` is that over the median: a rate over the required bytes, not a measured traffic."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_segmentation_amd import ops  # noqa: E402

SHAPES = [[16, 21, 512, 512], [8, 2, 256, 256]]


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


def torch_dice(logits, target, ignore_index=-100, smooth=1.0, backward=False):
    """Soft Dice over the classes present in the batch from torch ops (no host synchronisation: an absent class is
    weighted by zero)."""
    x = logits.detach().requires_grad_(backward)
    C = x.shape[1]
    p = torch.softmax(x, 1)
    valid = ((target != ignore_index) & (target >= 0) & (target < C)).unsqueeze(1)
    onehot = torch.zeros_like(p).scatter_(1, target.clamp(0, C - 1).unsqueeze(1), 1.0) * valid
    pm = p * valid
    n, S, TP = onehot.sum((0, 2, 3)), pm.sum((0, 2, 3)), (pm * onehot).sum((0, 2, 3))
    term = 1 - (TP + smooth) / (TP + 0.5 * (S - TP) + 0.5 * (n - TP) + smooth)
    has = (n > 0).float()
    loss = (term * has).sum() / has.sum().clamp(min=1)
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
    assert torch.cuda.is_available(), 'time_tversky.py measures on the GPU'
    assert opt.iters >= 10, 'a median over fewer than 10 calls is not reported'
    assert len(opt.shape) % 4 == 0, '--shape takes B C H W, repeated'
    rows = []
    for shape in [opt.shape[i:i + 4] for i in range(0, len(opt.shape), 4)]:
        B, C, H, W = shape
        g = torch.Generator().manual_seed(0)
        logits = (torch.randn(B, C, H, W, generator=g) * 2).cuda()
        target = torch.randint(0, C, (B, H, W), generator=g)
        target[torch.rand(B, H, W, generator=g) < 0.05] = -100
        target = target.cuda()

        out, dl = ops.tversky_fwd_bwd(logits, target)
        ref, dref = torch_dice(logits, target, backward=True)
        torch.cuda.synchronize()
        check = {'name': 'agreement', 'shape': shape, 'loss_hip': out[0].item(), 'loss_torch': ref.item(),
                 'n_valid': int(out[1].item()), 'n_terms': int(out[3].item()),
                 'grad_max_abs_diff': (dl - dref).abs().max().item(), 'grad_max_abs': dref.abs().max().item()}
        print(json.dumps(check), flush=True)
        assert abs(check['loss_hip'] - check['loss_torch']) <= 1e-5, 'the kernel and the torch ops disagree'
        assert check['grad_max_abs_diff'] <= 1e-4 * check['grad_max_abs'], 'the gradients disagree'
        del dl, dref
        rows.append(check)

        logit_bytes, target_bytes = logits.numel() * 4, target.numel() * 8
        moved = {'pseg_ce_fwd_bwd': 2 * logit_bytes + target_bytes,
                 'pseg_tversky_fwd_bwd': 3 * logit_bytes + 2 * target_bytes,
                 'pseg_tversky_fwd_bwd, no gradient': logit_bytes + target_bytes}
        fns = {
            'pseg_ce_fwd_bwd': lambda: ops.ce_fwd_bwd(logits, target),
            'pseg_tversky_fwd_bwd': lambda: ops.tversky_fwd_bwd(logits, target),
            'pseg_tversky_fwd_bwd, no gradient': lambda: ops.tversky_fwd_bwd(logits, target, want_grad=False),
            'torch ops, forward': lambda: torch_dice(logits, target),
            'torch ops, forward + backward': lambda: torch_dice(logits, target, backward=True),
        }
        for k, (med, lo, hi) in timed_median(fns, opt.iters).items():
            r = {'name': k, 'shape': shape, 'median_ms': round(med, 4), 'min_ms': round(lo, 4), 'max_ms': round(hi, 4),
                 'iters': opt.iters}
            if k in moved:
                r['bytes'] = moved[k]
                r['tb_per_s'] = round(moved[k] / (med * 1e-3) / 1e12, 3)
            print(json.dumps(r), flush=True)
            rows.append(r)
        del logits, target
        torch.cuda.empty_cache()
    if opt.out:
        with open(opt.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
