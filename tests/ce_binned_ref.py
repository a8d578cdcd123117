"""numpy float64 restatement of the contract of pseg_ce_opts_binned_fwd_bwd (include/pseg_amd.h) -- the configured
cross-entropy with a per-pixel weight u = bin_weight[pixel_bin] -- of boundary_weight_table, and the cases the CPU and GPU
tests share.

The per-pixel value f and its derivative are test_ce_opts_cpu.ce_opts_ref's, re-stated (that file is not touched);
test_ce_boundary_cpu.py pins this restatement to ce_opts_ref (table of ones: equal), to a separate band formula ('flat') and
to float64 autograd.  Here g = u f is what is summed, ranked and kept; the divisor is sum_kept u w_t.
"""
import collections
import math

import numpy as np
import torch

import boundary_ref as BR
from test_ce_opts_cpu import EPS, MIN_GAP, SHAPES, weights

CeBinnedRef = collections.namedtuple('CeBinnedRef', 'loss grad n_kept tau gap den info')

D = 3              # the band's width in every shared case
BOOST = 2.0


# ------------------------------------------------------------------ the table, from the formulas alone
def weight_table(width, boost, falloff='gaussian', sigma=None):
    """float64 [256]: 1 + boost * shape(k) for depth k in 1 .. width, 1 everywhere else"""
    if sigma is None:
        sigma = width / 3.0
    t = np.ones(256)
    for k in range(1, width + 1):
        if falloff == 'flat':
            s = 1.0
        elif falloff == 'linear':
            s = (width + 1 - k) / width
        elif falloff == 'gaussian':
            s = math.exp(-(k - 1) ** 2 / (2.0 * sigma ** 2))
        else:
            raise ValueError(falloff)
        t[k] = 1.0 + boost * s
    return t


# ------------------------------------------------------------------ the contract
def per_pixel(z, t, wv, eps, gamma):
    """rows of valid pixels: logits z [n, C], labels t [n] -> (f [n], df/dz [n, C], w_t [n]); ce_opts_ref's arithmetic"""
    n, C = z.shape
    rows = np.arange(n)
    zs = z - z.max(1, keepdims=True)
    ex = np.exp(zs)
    s = ex.sum(1, keepdims=True)
    p = ex / s
    nlogp = np.log(s) - zs
    onehot = np.zeros_like(p)
    onehot[rows, t] = 1.0
    wt = wv[t]
    ell = (1 - eps) * wt * nlogp[rows, t] + (eps / C) * (nlogp * wv).sum(1)
    q = (p * (1 - onehot)).sum(1)
    pt = p[rows, t]
    m = q ** gamma if gamma != 0 else np.ones(n)
    dl = (1 - eps) * wt[:, None] * (p - onehot) + (eps / C) * (p * wv.sum() - wv[None, :])
    dq = gamma * q ** (gamma - 1) if gamma != 0 else np.zeros(n)
    return m * ell, m[:, None] * dl - (ell * dq * pt)[:, None] * (onehot - p), wt


def ce_binned_ref(logits, target, pixel_bin, table, w=None, eps=0.0, gamma=0.0, keep=1.0, ignore_index=-100):
    """logits [B,C,H,W], target [B,H,W], pixel_bin [B,H,W] (0 .. 255), table [256] -> CeBinnedRef.  u = table[pixel_bin],
    g = u f; keep == 1 keeps every valid pixel (tau = 0), else k = clamp(ceil(float32(keep) * n_valid), 1, n_valid), tau =
    the k-th largest g, kept = g >= tau.  loss = sum_kept g / sum_kept (u w_t), NaN (and a zero gradient) when that divisor
    is 0; gradient = u df/dz / divisor on kept pixels.  gap: relative distance from tau to the nearest different g."""
    x = np.asarray(logits, dtype=np.float64)
    B, C, H, W = x.shape
    t = np.asarray(target).reshape(-1).astype(np.int64)
    z = x.transpose(0, 2, 3, 1).reshape(-1, C)
    wv = np.ones(C) if w is None else np.asarray(w, dtype=np.float64)
    u_all = np.asarray(table, dtype=np.float64)[np.asarray(pixel_bin).reshape(-1).astype(np.int64)]
    in_range = (t >= 0) & (t < C)
    valid = (t != ignore_index) & in_range
    n = int(valid.sum())
    info = {'n_valid': n, 'n_bad': int(((t != ignore_index) & ~in_range).sum()), 'valid': valid}
    f, df, wt = per_pixel(z[valid], t[valid], wv, eps, gamma) if n else (np.zeros(0), np.zeros((0, C)), np.zeros(0))
    u = u_all[valid]
    g = u * f
    tau, gap, k = 0.0, math.inf, n
    kept = np.ones(n, dtype=bool)
    if keep != 1.0 and n > 0:
        k = min(max(int(math.ceil(float(np.float32(keep)) * n)), 1), n)
        tau = float(np.sort(g)[::-1][k - 1])
        kept = g >= tau
        other = g[g != tau]
        gap = float(np.abs(other - tau).min() / abs(tau)) if len(other) and tau != 0 else math.inf
    den = float((u * wt)[kept].sum())
    kept_all = np.zeros(len(t), dtype=bool)
    kept_all[np.flatnonzero(valid)[kept]] = True
    info.update(k=k, f=f, g=g, u=u, wt=wt, kept_valid=kept, kept=kept_all.reshape(B, H, W))
    dz = np.zeros_like(z)
    if den > 0:
        loss = float(g[kept].sum() / den)
        gr = u[:, None] * df
        gr[~kept] = 0.0
        dz[valid] = gr / den
    else:
        loss = math.nan
    return CeBinnedRef(loss, dz.reshape(B, H, W, C).transpose(0, 3, 1, 2).copy(), int(kept.sum()), tau, gap, den, info)


# ------------------------------------------------------------------ cases
#            weights?, eps, gamma, keep
OPTIONS = {'off': (False, 0.0, 0.0, 1.0), 'w+eps+g2': (True, EPS, 2.0, 1.0), 'off,keep.25': (False, 0.0, 0.0, 0.25),
           'w+eps+g2,keep.25': (True, EPS, 2.0, 0.25), 'w+eps+g2,keep.75': (True, EPS, 2.0, 0.75)}
TABLES = ('gaussian', 'flat')
# seed 0 everywhere, except where a condition of test_ce_boundary_cpu.py fails at seed 0 (the seed changes, never the bound)
SEEDS = {}


def case_seed(name, falloff, opt):
    return SEEDS.get((name, falloff, opt), SEEDS.get(name, 0))


_CASES = {}


def make_case(name, seed=0):
    """(logits fp32 [B,C,H,W], target int64 [B,H,W]) torch tensors, depth int64 numpy [B,H,W] at width D.  Targets are
    Voronoi cells (pixel-random labels would have depth 1 everywhere) with a patch of ignore_index and a patch of an
    out-of-range label in the first image; the depth is boundary_ref's, where void labels compare by value."""
    if (name, seed) not in _CASES:
        B, C, H, W, std = SHAPES[name]
        g = torch.Generator().manual_seed(seed)
        logits = (torch.randn(B, C, H, W, generator=g, dtype=torch.float64) * std).float()
        rng = np.random.default_rng([seed, B, C, H, W])
        cells = 2 if H * W <= 128 else 3      # small images: two cells, so that some pixel is deeper than D
        T = np.stack([BR.voronoi(rng, H, W, C, cells + b % 2, first=b) for b in range(B)])
        T[0, 1:3, 2:5] = -100
        T[0, H - 3:H - 1, W - 3:W - 1] = C + 3
        if B > 1:
            T[B - 1, H // 2, W // 2] = -100      # a void speck: its neighbours are at depth 1
        _CASES[(name, seed)] = (logits, torch.from_numpy(T), BR.label_depth(T, D))
    return _CASES[(name, seed)]


_REFS = {}


def reference(name, falloff, opt):
    """(logits, target, depth, w, table float64, CeBinnedRef) of one shared case, computed once and left unchanged"""
    key = (name, falloff, opt)
    if key not in _REFS:
        C = SHAPES[name][1]
        use_w, eps, gamma, keep = OPTIONS[opt]
        logits, target, depth = make_case(name, case_seed(name, falloff, opt))
        w = weights(C) if use_w else None
        table = weight_table(D, BOOST, falloff)
        # the kernel reads the table in fp32: the reference uses those values
        table = table.astype(np.float32).astype(np.float64)
        _REFS[key] = (logits, target, depth, w, table, ce_binned_ref(logits, target, depth, table, w, eps, gamma, keep))
    return _REFS[key]


__all__ = ['BOOST', 'D', 'EPS', 'MIN_GAP', 'OPTIONS', 'SHAPES', 'TABLES', 'ce_binned_ref', 'make_case', 'reference',
           'weight_table', 'weights']
