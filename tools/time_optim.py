"""Timing of the optimiser launches with HIP events on the DeepLabV3+ (ResNet-50, 21 classes) parameter arena.

    python tools/time_optim.py [--out profiles/time_optim.json] [--iters N]

On random gradients, one FlatOptimizer.step() per call:
  * `pseg_sgd_step` (momentum 0.9) and `pseg_adam_step` as they stand: the baseline;
  * `pseg_sgd_step_mp` / `pseg_adam_step_mp`: the baseline under the half-precision policy, FlatOptimizer.step(mp_state=...),
    three launches (`pseg_mp_check`, the step, `pseg_mp_update`);
  * the grouped step (`pseg_opt_step_sgd` / `pseg_opt_step_adam`) with a ONE-run table, the configuration that reproduces the
    baseline bit for bit;
  * the grouped step with the model's real run table (no decay on BatchNorm parameters and biases, 0.1 on `backbone.`);
  * that with the weight EMA added;
  * that with the norm pass (`pseg_grad_sumsq`, two launches) and the clip added.
Each figure is the median over --iters single calls, each between its own pair of events, after warm-up; the variants
alternate inside one loop so that they see the same machine.  Every row carries the bytes the call moves by count (SGD
20 B / element: parameter and momentum read and written, gradient read; Adam 28; the EMA adds 8, the norm pass and the
`-mp` check 4 each) and that
over the time against 6.3 TB/s.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_segmentation_amd import _lib, ops  # noqa: E402
from pytorch_segmentation_amd.arena import ParamArena, make_runs  # noqa: E402
from pytorch_segmentation_amd.models import DeepLabV3Plus  # noqa: E402
from pytorch_segmentation_amd.utils import FlatOptimizer  # noqa: E402
from tools.time_lovasz import timed_median  # noqa: E402

PEAK = 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join('profiles', 'time_optim.json'))
    ap.add_argument('--iters', type=int, default=30)
    opt = ap.parse_args()
    assert torch.cuda.is_available(), 'time_optim.py measures on the GPU'
    assert opt.iters >= 10, 'a median over fewer than 10 calls is not reported'
    model = DeepLabV3Plus(21)
    arena = ParamArena(model, torch.device('cuda', torch.cuda.current_device()))
    n = arena.numel
    arena.grads.copy_(torch.randn(n, generator=torch.Generator().manual_seed(0)) * 1e-3)

    def rule(key, module, name):
        wd = 0.0 if (isinstance(module, torch.nn.BatchNorm2d) or name == 'bias') else 1e-4
        return (0.1 if key.startswith('backbone.') else 1.0), wd
    real = arena.runs(rule)
    one = make_runs([(0, n, 1.0, 1e-4)])
    mp_state = torch.zeros(8, dtype=torch.float32, device=arena.device)
    _lib.call('pseg_mp_state_init', mp_state.data_ptr(), 2.0 ** 16, ops._stream())
    variants = {}
    for adam, tag, base_bytes in ((False, 'sgd', 20), (True, 'adam', 28)):
        kw = dict(adam=adam, lr=1e-3, weight_decay=1e-4)
        variants['pseg_%s_step' % tag] = (FlatOptimizer(arena, **kw), base_bytes, 1)
        variants['pseg_%s_step_mp' % tag] = (FlatOptimizer(arena, **kw), base_bytes + 4, 3)
        variants['pseg_opt_step_%s, one run' % tag] = (FlatOptimizer(arena, runs=one, **kw), base_bytes, 1)
        variants['pseg_opt_step_%s, %d runs' % (tag, len(real))] = (FlatOptimizer(arena, runs=real, **kw), base_bytes, 1)
        variants['pseg_opt_step_%s, %d runs + ema' % (tag, len(real))] = \
            (FlatOptimizer(arena, runs=real, ema_decay=0.999, **kw), base_bytes + 8, 1)
        variants['pseg_opt_step_%s, %d runs + ema + norm' % (tag, len(real))] = \
            (FlatOptimizer(arena, runs=real, ema_decay=0.999, max_grad_norm=1.0, **kw), base_bytes + 12, 3)
    med = timed_median({k: (lambda o=v[0]: o.step(mp_state=mp_state)) if k.endswith('_mp') else v[0].step
                        for k, v in variants.items()}, opt.iters)
    rows = []
    for k, (m, lo, hi) in med.items():
        _, bpe, launches = variants[k]
        base = med['pseg_%s_step' % ('adam' if 'adam' in k else 'sgd')][0]
        r = {'name': k, 'elements': n, 'launches': launches, 'median_ms': round(m, 4), 'min_ms': round(lo, 4), 'max_ms': round(hi, 4),
             'iters': opt.iters, 'bytes_per_element': bpe, 'TB_per_s': round(bpe * n / (m * 1e-3) / 1e12, 2),
             'of_6.3_TB_per_s': round(bpe * n / (m * 1e-3) / PEAK, 3), 'ratio_to_baseline': round(m / base, 3)}
        print(json.dumps(r), flush=True)
        rows.append(r)
    if opt.out:
        os.makedirs(os.path.dirname(opt.out) or '.', exist_ok=True)
        with open(opt.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
