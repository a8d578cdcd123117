"""Timing of the augmentation kernel (csrc/augment.hip, utils/augment.py) with HIP events.

    python tools/time_augment.py [--out FILE.json] [--iters N]

At B = 16, 3 x 512 x 512 and at B = 8, 3 x 256 x 256, on the same uint8 tensors:
  * `post_fetch_fn`: the five torch ops the kernel replaces (CocoDataset.post_fetch_fn without augments: float, subtract,
    divide, labels to int64; at the multi-scale size additionally the nearest interpolate);
  * `augment identity`: ops.augment_batch with identity rows already on the device (the kernel alone);
  * `augment reference`: ops.augment_batch with DeviceAugment.reference() rows already on the device (rotated / bilinear
    gathers, colour matrices);
  * `DeviceAugment()`: the whole call as the loader makes it -- host sampling, the pinned copy of the table, the launch.
At B = 16, 3 x 512 x 512 also the neighbourhood kernel (ops.augment_batch_nbhd: filter, noise, dropout), tables on the device:
  * `nbhd identity rows`: identity rows without a filter, noise or dropout (next to `augment identity rows` of the same loop);
  * `nbhd full(seed=0) rows`: the first batch that DeviceAugment.full(seed=0) draws;
  * `nbhd K=13 every sample`: identity rows with a dense 13 x 13 filter on every sample, the upper end;
and the warp kernel (ops.augment_batch_warp: elastic jitter, displacement grid, homography) on the last two tables:
  * `warp ..., fields off`: the same rows with h2 = (0, 0, 1), no jitter, no grid (the output is the nbhd kernel's);
  * `warp ..., all three on`: the same rows with a mild perspective, a grid of N(0, 0.05) of the size and alpha = 3.5 on
    every sample.
and the blend kernel (ops.augment_batch_blend: median, edge and colour blends, hue / saturation) on the first batch of
DeviceAugment.blends(seed=0), tables on the device:
  * `blend batch: warp kernel (baseline)`: the batch's rows without the four new stages, through ops.augment_batch_warp;
  * `blend kernel, fields off`: the same rows through the blend kernel (the output is the warp kernel's);
  * `blend kernel, median k=11` / `edge blend` / `colour blend` / `hue / saturation`: one new stage on every sample;
  * `blend kernel, all on`: the four together; each with its ratio to the baseline of the same loop.
Each figure is the median over --iters (>= 50) single calls, each between its own pair of events, after warm-up; the
variants alternate inside one loop so that they see the same machine.  Algorithmic bytes = every input byte once + the fp32
output + the int64 targets; fractions of the roof are over 6.3 TB/s HBM.
"""
import argparse
import json
import os
import random
import statistics
import sys
import tempfile

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_segmentation_amd import ops  # noqa: E402
from pytorch_segmentation_amd.utils.augment import DeviceAugment  # noqa: E402
from pytorch_segmentation_amd.utils.datasets import MEAN, STD, CocoDataset  # noqa: E402

HBM = 6.3e12


def timed_median(fns, iters, warmup=10):
    """{name: fn} -> {name: median ms of `iters` single calls}; the functions alternate call by call"""
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
    return {k: statistics.median(a.elapsed_time(b) for a, b in ev[k]) for k in fns}


def rows_for(B, H, W, out_hw, iters):
    g = torch.Generator().manual_seed(B * H)
    imgs = torch.randint(0, 256, (B, 3, H, W), dtype=torch.uint8, generator=g).cuda()
    segs = torch.randint(0, 21, (B, H, W), dtype=torch.uint8, generator=g).cuda()
    oh, ow = out_hw or (H, W)
    with tempfile.TemporaryDirectory() as d:             # post_fetch_fn of a loader without augments: an empty dataset will do
        with open(os.path.join(d, 'train.json'), 'w') as f:
            json.dump({'categories': [{'name': 'a'}], 'images': [], 'annotations': []}, f)
        loader = CocoDataset(os.path.join(d, 'train.json'))
    ident = torch.from_numpy(DeviceAugment.identity(seed=0).sample(B, H, W)).cuda()
    ref_aug = DeviceAugment.reference(seed=0)
    ref = torch.from_numpy(ref_aug.sample(B, H, W)).cuda()

    def torch_path():
        x, t = loader.post_fetch_fn((imgs, segs))
        if out_hw:
            x = torch.nn.functional.interpolate(x, out_hw)
        return x, t
    fns = {
        'post_fetch_fn (torch ops)': torch_path,
        'augment identity rows': lambda: ops.augment_batch(imgs, segs, ident, oh, ow, MEAN, STD),
        'augment reference rows': lambda: ops.augment_batch(imgs, segs, ref, oh, ow, MEAN, STD),
        'DeviceAugment() sample + copy + launch': lambda: ref_aug(imgs, segs, out_hw),
    }
    a, b = torch_path(), ops.augment_batch(imgs, segs, ident, oh, ow, MEAN, STD)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), 'identity rows must reproduce post_fetch_fn'
    ms = timed_median(fns, iters)
    nbytes = imgs.numel() + segs.numel() + B * 3 * oh * ow * 4 + segs.numel() * 8
    out = []
    for k, v in ms.items():
        r = {'name': k, 'B': B, 'in': [H, W], 'out': [oh, ow], 'median_ms': round(v, 4), 'iters': iters, 'alg_bytes': nbytes,
             'roof_fraction': round(nbytes / HBM / (v * 1e-3), 3)}
        print(json.dumps(r), flush=True)
        out.append(r)
    return out


def nbhd_rows_for(B, H, W, iters):
    import numpy as np
    from pytorch_segmentation_amd.utils import augment as aug
    g = torch.Generator().manual_seed(B * H)
    imgs = torch.randint(0, 256, (B, 3, H, W), dtype=torch.uint8, generator=g).cuda()
    segs = torch.randint(0, 21, (B, H, W), dtype=torch.uint8, generator=g).cuda()
    narrow = DeviceAugment.identity(seed=0).sample(B, H, W)
    full = DeviceAugment.full(seed=0).sample(B, H, W)
    assert full.shape[1] == aug.NBHD_ROW, 'the first batch of full(seed=0) draws a filter'
    tables = {
        'nbhd identity rows': np.stack([aug.make_nbhd_row(r) for r in narrow]),
        'nbhd full(seed=0) rows': full,
        'nbhd K=13 every sample': np.stack([aug.make_nbhd_row(r, np.full((13, 13), 1.0 / 169)) for r in narrow]),
    }
    grid = np.random.default_rng(0).normal(0.0, 0.05, (4, 4, 2)) * (W, H)
    for name in ('full(seed=0) rows', 'K=13 every sample'):
        t = tables['nbhd ' + name]
        tables['warp %s, fields off' % name] = np.stack([aug.make_warp_row(r) for r in t])
        tables['warp %s, all three on' % name] = np.stack([aug.make_warp_row(r, (1e-4, -5e-5, 1.0), 3.5, grid) for r in t])
    ident = torch.from_numpy(narrow).cuda()
    fns = {'augment identity rows': lambda: ops.augment_batch(imgs, segs, ident, H, W, MEAN, STD)}
    for name, t in tables.items():
        dev, shapes = torch.from_numpy(t).cuda(), torch.from_numpy(aug.row_shapes(t))
        kernel = ops.augment_batch_warp if name.startswith('warp') else ops.augment_batch_nbhd
        fns[name] = lambda kernel=kernel, dev=dev, shapes=shapes: kernel(imgs, segs, dev, shapes, H, W, MEAN, STD)
    a, b = fns['augment identity rows'](), fns['nbhd identity rows']()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), 'rows without neighbourhood fields must reproduce augment_batch'
    a, b = fns['nbhd full(seed=0) rows'](), fns['warp full(seed=0) rows, fields off']()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), 'rows without warp fields must reproduce augment_batch_nbhd'
    ms = timed_median(fns, iters)
    shapes = aug.row_shapes(full)
    out = []
    for k, v in ms.items():
        r = {'name': k, 'B': B, 'in': [H, W], 'out': [H, W], 'median_ms': round(v, 4), 'iters': iters, 'section': 'nbhd'}
        if k.startswith('nbhd full'):
            r['K'] = shapes[:, 0].tolist()
            r['noise'] = int((full[:, aug.NBHD_NOISE] > 0).sum())
            r['dropout'] = int((full[:, aug.NBHD_DROP] > 0).sum())
        print(json.dumps(r), flush=True)
        out.append(r)
    return out


def blend_rows_for(B, H, W, iters):
    """the blend kernel (ops.augment_batch_blend) on the first batch of DeviceAugment.blends(seed=0): the batch's own warp rows
    through pseg_augment_batch_warp (the baseline: that kernel is the parent commit's), then the same rows through the blend
    kernel with the new fields off, with each of the four on alone on every sample (the median at k = 11), and with all on"""
    import numpy as np
    from pytorch_segmentation_amd.utils import augment as aug
    g = torch.Generator().manual_seed(B * H)
    imgs = torch.randint(0, 256, (B, 3, H, W), dtype=torch.uint8, generator=g).cuda()
    segs = torch.randint(0, 21, (B, H, W), dtype=torch.uint8, generator=g).cuda()
    recipes = DeviceAugment.blends(seed=0).draw(B)
    plain = [dict({k: v for k, v in r.items() if k not in aug._BLEND_KEYS + ('edge_mask',)},
                  colour=[('multiply', v[0]) if n == 'blend' else (n, v) for n, v in r['colour']]) for r in recipes]
    base = DeviceAugment.rows(plain, H, W)
    if base.shape[1] == aug.ROW:
        base = np.stack([aug.make_nbhd_row(r) for r in base])
    if base.shape[1] == aug.NBHD_ROW:
        base = np.stack([aug.make_warp_row(r) for r in base])
    rng = np.random.default_rng(0)
    t1, t2 = aug.value_noise_table(rng), aug.frequency_noise_table(rng)
    mb = aug.colour_matrix([('contrast', np.full(3, 1.5))])

    def second(row):                                        # G = E * F of the sample's own F
        K = int(row[aug.NBHD_K])
        F = row[aug.NBHD_WEIGHTS:aug.NBHD_WEIGHTS + K * K].astype(np.float64).reshape(K, K) if K > 1 else np.ones((1, 1))
        return aug.compose_filters([F, aug.edge_kernel(0.75)])
    on = {'median k=11': lambda r: dict(kmed=11), 'edge blend': lambda r: dict(kernel2=second(r), t1=t1),
          'colour blend': lambda r: dict(colour2=mb, t2=t2), 'hue / saturation': lambda r: dict(hue_sat=aug.hue_sat_shift(20))}
    tables = {'blend batch: warp kernel (baseline)': base, 'blend kernel, fields off': np.stack([aug.make_blend_row(r) for r in base])}
    for name, kw in on.items():
        tables['blend kernel, %s' % name] = np.stack([aug.make_blend_row(r, **kw(r)) for r in base])
    tables['blend kernel, all on'] = np.stack([aug.make_blend_row(r, **{k: v for kw in on.values() for k, v in kw(r).items()}) for r in base])
    fns = {}
    for name, t in tables.items():
        dev, shapes = torch.from_numpy(t).cuda(), torch.from_numpy(aug.row_shapes(t))
        kernel = ops.augment_batch_blend if t.shape[1] == aug.BLEND_ROW else ops.augment_batch_warp
        fns[name] = lambda kernel=kernel, dev=dev, shapes=shapes: kernel(imgs, segs, dev, shapes, H, W, MEAN, STD)
    a, b = fns['blend batch: warp kernel (baseline)'](), fns['blend kernel, fields off']()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), 'rows without blend fields must reproduce augment_batch_warp'
    ms = timed_median(fns, iters)
    ref = ms['blend batch: warp kernel (baseline)']
    out = []
    for k, v in ms.items():
        r = {'name': k, 'B': B, 'in': [H, W], 'out': [H, W], 'median_ms': round(v, 4), 'iters': iters, 'section': 'blend',
             'ratio_to_warp': round(v / ref, 3)}
        if k.endswith('(baseline)'):
            r['K'] = aug.row_shapes(base)[:, 0].tolist()
        print(json.dumps(r), flush=True)
        out.append(r)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='')
    ap.add_argument('--iters', type=int, default=100)
    opt = ap.parse_args()
    assert torch.cuda.is_available(), 'time_augment.py measures on the GPU'
    assert opt.iters >= 50, 'a median over fewer than 50 calls is not reported'
    random.seed(0)
    rows = rows_for(16, 512, 512, None, opt.iters) + rows_for(8, 256, 256, None, opt.iters)
    rows += rows_for(16, 512, 512, (384, 384), opt.iters)          # one multi-scale size: the torch path adds its interpolate
    rows += nbhd_rows_for(16, 512, 512, opt.iters)
    rows += blend_rows_for(16, 512, 512, opt.iters)
    if opt.out:
        with open(opt.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
