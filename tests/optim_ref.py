"""fp64 restatement of ONE grouped optimiser step (csrc/optim.hip), and the same recipe through torch.optim.

grouped_step(): runs with their own learning-rate factor and weight decay, the global-norm clip of
torch.nn.utils.clip_grad_norm_, SGD (momentum, Nesterov) or Adam / AdamW, the weight EMA and the `-mp` skip, written out
on fp64 tensors.  torch_recipe(): the same thing as a user would write it -- one param group per run, clip_grad_norm_,
optimizer.step(), a hand-written EMA -- in a dtype of the caller's choice: in fp64 it pins the restatement
(tests/test_optim_groups_cpu.py), in fp32 its distance from the restatement is the yardstick of the GPU tests.

    python tests/optim_ref.py          # prints that distance per tensor for the cases of tests/test_optim_groups_gpu.py
"""
import math

import numpy as np
import torch

SPAN, BLOCK_CAP = 1024, 1024        # floats per block and trip; blocks per run (arena.RUN_SPAN, arena.RUN_BLOCK_CAP)


def f32(v):
    """a hyper-parameter as the C ABI receives it (float)"""
    return float(np.float32(v))


def grouped_step(st, g, runs, adam, lr, momentum=0.0, nesterov=False, betas=(0.9, 0.999), eps=1e-8, decoupled=False,
                 grad_scale=1.0, step=1, max_norm=0.0, ema_decay=0.0, mp=None):
    """One step, in place on the fp64 tensors of `st`: 'p', 'm' (momentum buffer / exp_avg, None without momentum), 'v'
    (exp_avg_sq, Adam), 'ema' (None: no EMA), and the clip record 'coef', 'norm', 'clipped'.
    g: the gradients as they lie in the arena (fp64; under `-mp` still multiplied by the loss scale).
    runs: rows of (offset, count, first_block, lr_mult, weight_decay).  step: 1-based number of this applied step.
    mp: None or dict(inv_scale=1/S, found=bool).  -> False when the step was skipped."""
    gs = grad_scale
    if mp is not None:
        if mp['found']:
            return False
        gs = f32(f32(grad_scale) * f32(mp['inv_scale']))
    coef = 1.0
    if max_norm > 0:
        eff = math.sqrt(float((g * g).sum())) * abs(gs)
        coef = min(1.0, max_norm / (eff + 1e-6))
        st['coef'], st['norm'] = coef, eff
        st['clipped'] = st.get('clipped', 0) + (1 if coef < 1.0 else 0)
    for off, cnt, _, lm, wd in runs:
        s = slice(off, off + cnt)
        lr_r = lr * lm
        w = st['p'][s]
        d = g[s] * gs * coef
        if wd != 0:
            if decoupled:
                w.mul_(1 - lr_r * wd)
            else:
                d = d + wd * w
        if adam:
            b1, b2 = betas
            m, v = st['m'][s], st['v'][s]
            m.mul_(b1).add_((1 - b1) * d)
            v.mul_(b2).add_((1 - b2) * d * d)
            bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
            w.sub_((lr_r / bc1) * m / (v.sqrt() / bc2 ** 0.5 + eps))
        else:
            if momentum != 0:
                buf = st['m'][s]
                if step == 1:
                    buf.copy_(d)
                else:
                    buf.mul_(momentum).add_(d)
                d = d + momentum * buf if nesterov else buf
            w.sub_(lr_r * d)
        if st.get('ema') is not None:
            st['ema'][s].mul_(ema_decay).add_((1 - ema_decay) * w)
    return True


def new_state(p0, adam, momentum, ema):
    p = p0.double().clone()
    return {'p': p, 'm': torch.zeros_like(p) if (adam or momentum != 0) else None, 'v': torch.zeros_like(p) if adam else None,
            'ema': p.clone() if ema else None}


def torch_recipe(p0, grads, runs, adam, lr, momentum=0.0, nesterov=False, betas=(0.9, 0.999), eps=1e-8, decoupled=False,
                 grad_scale=1.0, max_norm=0.0, ema_decay=0.0, dtype=torch.float64):
    """The recipe with torch's own tools, from zero optimiser state, one step per entry of `grads` (unscaled-by-loss-scale
    gradients; grad_scale is applied here): -> dict of flat tensors p, m, v, ema in `dtype` (None where absent)."""
    params = [p0[o:o + c].to(dtype).clone().requires_grad_() for o, c, _, _, _ in runs]
    groups = [{'params': [p], 'lr': lr * lm, 'weight_decay': wd} for p, (_, _, _, lm, wd) in zip(params, runs)]
    if adam:
        opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)(groups, lr=lr, betas=betas, eps=eps)
    else:
        assert not decoupled, 'torch.optim.SGD has no decoupled decay'
        opt = torch.optim.SGD(groups, lr=lr, momentum=momentum, nesterov=nesterov)
    ema = [p.detach().clone() for p in params] if ema_decay > 0 else None
    for g in grads:
        for p, (o, c, _, _, _) in zip(params, runs):
            p.grad = g[o:o + c].to(dtype) * grad_scale
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_(params, max_norm, error_if_nonfinite=False)
        opt.step()
        if ema is not None:
            for e, p in zip(ema, params):
                e.mul_(ema_decay).add_((1 - ema_decay) * p.detach())

    def flat(key):
        parts = [opt.state[p].get(key) for p in params]
        return None if parts[0] is None else torch.cat([t.detach() for t in parts])
    return {'p': torch.cat([p.detach() for p in params]), 'm': flat('exp_avg' if adam else 'momentum_buffer'),
            'v': flat('exp_avg_sq') if adam else None, 'ema': torch.cat(ema) if ema is not None else None}


def restatement_run(p0, grads, runs, adam, ema_decay=0.0, momentum=0.0, **kw):
    """grouped_step over `grads` from zero state -> the state dict"""
    st = new_state(p0, adam, momentum, ema_decay > 0)
    for i, g in enumerate(grads):
        grouped_step(st, g.double(), runs, adam, momentum=momentum, ema_decay=ema_decay, step=i + 1, **kw)
    return st


# ---------------------------------------------------------------------------------------- the cases of the GPU tests
# Five runs (tests/test_optim_groups_gpu.py): 4 floats; 8 floats; 1020 floats, less than one block's span of 1024; 5000
# floats, five blocks and no multiple of the span; 2 * BLOCK_CAP * SPAN = 2 097 152 floats, the shortest run whose blocks
# (capped at BLOCK_CAP = 1024 per run) send every thread through its loop twice.  Distinct lr_mult (one 0) and decay (one 0).
RUN_COUNTS = [4, 8, 1020, 5000, 2 * BLOCK_CAP * SPAN]
RUN_LR_MULT = [0.5, 0.0, 2.0, 0.1, 1.0]
RUN_DECAY = [1e-2, 5e-3, 0.0, 2e-2, 1e-3]


def five_runs():
    rows, off, blocks = [], 0, 0
    for c, lm, wd in zip(RUN_COUNTS, RUN_LR_MULT, RUN_DECAY):
        rows.append((off, c, blocks, f32(lm), f32(wd)))
        off += c
        blocks += max(1, min(BLOCK_CAP, -(-c // SPAN)))
    return rows, off, blocks


# name, adam, decoupled, momentum, nesterov, grad_scale
VARIANTS = [('sgd', False, False, 0.9, True, 0.5), ('adam', True, False, 0.0, False, 0.5), ('adamw', True, True, 0.0, False, 0.5)]
HYPER = {'sgd': dict(lr=f32(0.1)), 'adam': dict(lr=f32(1e-2), betas=(f32(0.9), f32(0.999)), eps=f32(1e-8)),
         'adamw': dict(lr=f32(1e-2), betas=(f32(0.9), f32(0.999)), eps=f32(1e-8))}
EMA_DECAY = f32(0.99)
# the gradients are uniform in [-1, 1): their norm over 2.1 M floats is ~836, ~418 after grad_scale 0.5; this clips every step
MAX_NORM = f32(100.0)


def case_inputs():
    from oracle import fill
    _, n, _ = five_runs()
    p0 = fill.uniform('optg/p', (n,))
    grads = [fill.uniform('optg/g%d' % i, (n,)) for i in range(3)]
    return p0, grads


def elem_fig(got, ref):
    """tests/test_support_ops_gpu.py's per-element figure: max_i |got_i - ref_i| / max(|ref_i|, 1e-2 * peak)"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    peak = ref.abs().max().item()
    return ((got - ref).abs() / (ref.abs().clamp(min=1e-2 * peak) + 1e-300)).max().item()


def measure():
    """distance of torch's fp32 CPU run of the recipe from the restatement, per variant and tensor (elem_fig)"""
    runs, _, _ = five_runs()
    p0, grads = case_inputs()
    out = {}
    for name, adam, decoupled, mu, nesterov, gscale in VARIANTS:
        kw = dict(HYPER[name], nesterov=nesterov, decoupled=decoupled, grad_scale=f32(gscale), max_norm=MAX_NORM)
        ref = restatement_run(p0, grads, runs, adam, ema_decay=EMA_DECAY, momentum=f32(mu), **kw)
        t32 = torch_recipe(p0, grads, runs, adam, momentum=f32(mu), ema_decay=EMA_DECAY, dtype=torch.float32, **kw)
        out[name] = {k: elem_fig(t32[k], ref[k]) for k in ('p', 'm', 'v', 'ema') if ref[k] is not None}
    return out


if __name__ == '__main__':
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    for name, figs in measure().items():
        print(name, ' '.join('%s %.2e' % kv for kv in figs.items()))
