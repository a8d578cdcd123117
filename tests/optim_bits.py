"""The optimiser steps on the device, as the tests call them, and sha256 digests of what they leave behind.

digests(): every step entry point on CPU-generated inputs (optim_ref.case_inputs), three steps each, -> the sha256 of the raw
bytes of every state tensor after the third step.  tests/golden/optim_step_bits.json holds those digests as the kernels
produced them before the six step kernels became one per rule; test_step_bits_match_recorded (tests/test_optim_groups_gpu.py)
recomputes them, so a change to the update arithmetic -- a moved contraction, a multiply that is not by exactly 1.0f --
shows as a changed digest.  The file also names the compiler it was recorded under: another hipcc may contract differently.

    python tests/optim_bits.py --record        # on a GPU: rewrites the fixture (only when the arithmetic is MEANT to change)

Flat entry points (pseg_sgd_step, pseg_adam_step and their _mp forms) at n = 3 (a scalar tail only, n / 4 == 0), 1027 (one
block and a 3-float tail) and 2 098 179 = 2048 * 1024 + 1024 + 3 (the 2048-block grid cap, a second trip over part of the
grid, and a tail).  The _mp cases use loss scale 1024 and gradients multiplied by it, with pseg_mp_check and pseg_mp_update
around the step as the trainer issues them.  Grouped entry points: every row of optim_ref.VARIANTS over the five-run table
with clip and EMA on, with and without mp_state; clip_state is digested too (pseg_grad_sumsq is bit-reproducible).
"""
import hashlib
import json
import os
import shutil
import subprocess
import sys

import torch

import optim_ref as R
from optim_ref import f32

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'optim_step_bits.json')
LOSS_SCALE = 1024.0
MP_UPDATE = (2.0, 0.5, 2000, 1.0, float(2 ** 24))      # growth, backoff, interval, min and max scale: the trainer's
FLAT_SIZES = (3, 1027, 2048 * 1024 + 1024 + 3)
# name, momentum, weight decay, nesterov, grad_scale
FLAT_SGD = [('plain-null-buffer', 0.0, 0.0, False, 1.0), ('momentum-wd', 0.9, 1e-2, False, 1.0),
            ('nesterov-wd-gscale', 0.9, 1e-2, True, 0.25)]
# name, weight decay, decoupled, grad_scale
FLAT_ADAM = [('plain', 0.0, False, 1.0), ('wd-gscale', 1e-2, False, 0.5), ('adamw', 1e-2, True, 1.0)]


class Table:
    """a run table on the host and on the device (both kept alive for the launches)"""

    def __init__(self, rows, blocks):
        from pytorch_segmentation_amd.arena import pack_runs
        self.rows, self.blocks = rows, blocks
        self.host, _ = pack_runs(rows)
        self.dev = torch.from_numpy(self.host.view('uint8').copy()).cuda()

    def args(self, n):
        return (n, self.dev.data_ptr(), self.host.ctypes.data, len(self.rows), self.blocks)


def opt_sgd(lib, ops, tab, p, g, buf, ema, lr, mu, nesterov, decoupled, gscale, first, max_norm=0.0, decay=0.0, clip=None,
            mp=None):
    lib.call('pseg_opt_step_sgd', p.data_ptr(), g.data_ptr(), ops._ptr(buf), ops._ptr(ema), *tab.args(p.numel()), lr, mu,
             int(nesterov), int(decoupled), gscale, int(first), max_norm, decay, ops._ptr(clip), ops._ptr(mp), ops._stream())


def opt_adam(lib, ops, tab, p, g, m, v, ema, lr, betas, eps, decoupled, gscale, step, max_norm=0.0, decay=0.0, clip=None,
             mp=None):
    lib.call('pseg_opt_step_adam', p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), ops._ptr(ema), *tab.args(p.numel()),
             lr, betas[0], betas[1], eps, int(decoupled), gscale, int(step), max_norm, decay, ops._ptr(clip), ops._ptr(mp),
             ops._stream())


def sumsq(lib, ops, g, clip):
    nbytes = lib.query('pseg_grad_sumsq_workspace_bytes', g.numel())
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device='cuda')
    lib.call('pseg_grad_sumsq', g.data_ptr(), g.numel(), ws.data_ptr(), nbytes, clip.data_ptr(), ops._stream())
    return ws


def five_run_case():
    """the five-run table and its CPU-generated inputs"""
    runs, n, blocks = R.five_runs()
    p0, grads = R.case_inputs()
    return {'runs': runs, 'n': n, 'blocks': blocks, 'p0': p0, 'grads': grads}


def run_five(ops, lib, case, name, mp, max_norm=R.MAX_NORM, steps=3, ema=True):
    """the five-run table through the device calls the optimiser issues: [mp_check] sumsq step [mp_update] -> state dict"""
    _, adam, decoupled, mu, nesterov, gscale = next(v for v in R.VARIANTS if v[0] == name)
    mu, gscale, n, S = f32(mu), f32(gscale), case['n'], LOSS_SCALE
    tab = Table(case['runs'], case['blocks'])
    p = case['p0'].cuda()
    m = torch.zeros(n, device='cuda') if (adam or mu != 0) else None
    v = torch.zeros(n, device='cuda') if adam else None
    e = p.clone() if ema else None
    clip = torch.zeros(4, device='cuda')
    state = None
    if mp:
        state = torch.zeros(8, device='cuda')
        lib.call('pseg_mp_state_init', state.data_ptr(), S, ops._stream())
    h = R.HYPER[name]
    for i, g in enumerate(case['grads'][:steps]):
        gd = (g * S).cuda() if mp else g.cuda()       # (-mp: the gradients arrive multiplied by the loss scale, exactly)
        if mp:
            lib.call('pseg_mp_check', gd.data_ptr(), n, state.data_ptr(), ops._stream())
        if max_norm > 0:
            sumsq(lib, ops, gd, clip)
        decay = R.EMA_DECAY if ema else 0.0
        if adam:
            opt_adam(lib, ops, tab, p, gd, m, v, e, h['lr'], h['betas'], h['eps'], decoupled, gscale, i + 1, max_norm, decay,
                     clip, state)
        else:
            opt_sgd(lib, ops, tab, p, gd, m, e, h['lr'], mu, nesterov, decoupled, gscale, i == 0, max_norm, decay, clip, state)
        if mp:
            lib.call('pseg_mp_update', state.data_ptr(), *MP_UPDATE, ops._stream())
    out = {'p': p, 'm': m, 'v': v, 'ema': e}
    return {k: t for k, t in out.items() if t is not None}, clip.cpu(), (state.cpu() if mp else None)


def run_flat(ops, lib, case, n, adam, cfg, mp):
    """three steps of a flat entry point over the first n floats of the case's inputs -> state dict"""
    p = case['p0'][:n].cuda()
    state = None
    if mp:
        state = torch.zeros(8, device='cuda')
        lib.call('pseg_mp_state_init', state.data_ptr(), LOSS_SCALE, ops._stream())
    if adam:
        _, wd, decoupled, gscale = cfg
        h = R.HYPER['adam']
        m, v = torch.zeros(n, device='cuda'), torch.zeros(n, device='cuda')
        head = (m.data_ptr(), v.data_ptr(), n, h['lr'], h['betas'][0], h['betas'][1], h['eps'], f32(wd), int(decoupled), f32(gscale))
    else:
        _, mu, wd, nesterov, gscale = cfg
        m, v = (torch.zeros(n, device='cuda') if mu != 0 else None), None
        head = (ops._ptr(m), n, R.HYPER['sgd']['lr'], f32(mu), f32(wd), int(nesterov), f32(gscale))
    entry = 'pseg_adam_step' if adam else 'pseg_sgd_step'
    for i, g in enumerate(case['grads']):
        gd = (g[:n] * LOSS_SCALE).cuda() if mp else g[:n].cuda()
        if mp:
            lib.call('pseg_mp_check', gd.data_ptr(), n, state.data_ptr(), ops._stream())
            lib.call(entry + '_mp', p.data_ptr(), gd.data_ptr(), *head, state.data_ptr(), ops._stream())
            lib.call('pseg_mp_update', state.data_ptr(), *MP_UPDATE, ops._stream())
        else:
            # (the host's step argument: first_step for SGD, the 1-based step number for Adam)
            lib.call(entry, p.data_ptr(), gd.data_ptr(), *head, (i + 1) if adam else int(i == 0), ops._stream())
    out = {'p': p, 'm': m, 'v': v, 'mp_state': state}
    return {k: t for k, t in out.items() if t is not None}


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def digests(lib, ops):
    """{case: {tensor: sha256 of its bytes after the third step}} over every step entry point"""
    case = five_run_case()
    out = {}
    for adam, configs in ((False, FLAT_SGD), (True, FLAT_ADAM)):
        for mp in (False, True):
            entry = 'pseg_%s_step%s' % ('adam' if adam else 'sgd', '_mp' if mp else '')
            for cfg in configs:
                for n in FLAT_SIZES:
                    got = run_flat(ops, lib, case, n, adam, cfg, mp)
                    out['%s/%s/n=%d' % (entry, cfg[0], n)] = {k: sha(t) for k, t in got.items()}
    for name, adam, *_ in R.VARIANTS:
        for mp in (False, True):
            got, clip, state = run_five(ops, lib, case, name, mp)
            d = {k: sha(t) for k, t in got.items()}
            d['clip_state'] = sha(clip)
            if mp:
                d['mp_state'] = sha(state)
            out['pseg_opt_step_%s/%s/five-runs%s' % ('adam' if adam else 'sgd', name, '/mp' if mp else '')] = d
    return out


def compiler_line():
    """the version line of the installed hipcc's compiler ('not found' without one: the line only labels a mismatch)"""
    hipcc = os.environ.get('HIPCC') or shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    try:
        text = subprocess.run([hipcc, '--version'], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60).stdout.decode()
    except (OSError, subprocess.SubprocessError):
        return 'hipcc not found'
    lines = [ln.strip() for ln in text.splitlines() if ln.strip()]
    return next((ln for ln in lines if 'clang version' in ln), lines[0] if lines else 'hipcc not found')


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert '--record' in sys.argv, 'python tests/optim_bits.py --record'
    assert torch.cuda.is_available(), 'the digests are those of the GPU kernels'
    from pytorch_segmentation_amd import _lib, ops as _ops
    rec = {'compiler': compiler_line(), 'digests': digests(_lib, _ops)}
    with open(FIXTURE, 'w') as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write('\n')
    print('recorded %d cases under %s' % (len(rec['digests']), rec['compiler']))
