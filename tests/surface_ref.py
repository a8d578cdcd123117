"""The contracts of pseg_class_sdist and pseg_surface_fwd_bwd (include/pseg_amd.h) restated in numpy: the signed squared
Euclidean distance map by all pairs (sdist_brute) and by column distances and a broadcast row minimum (sdist_separable), the
signed distance phi, and the loss with its gradient in float64 (surface_ref).  tests/test_surface_cpu.py holds the two
distance maps to each other; tests/test_surface_gpu.py holds the kernels to them."""
import numpy as np
import torch

_FAR = 1 << 20      # "no such pixel in this column": its square is beyond every real distance and fits int64


def sdist_brute(labels, C):
    """labels [B,H,W] int -> int64 [B,C,H,W] by definition: every pair of pixels of an image (small maps only)"""
    t = np.asarray(labels).astype(np.int64)
    B, H, W = t.shape
    yy, xx = np.mgrid[0:H, 0:W]
    y, x = yy.reshape(-1), xx.reshape(-1)
    d2 = (y[:, None] - y[None, :]) ** 2 + (x[:, None] - x[None, :]) ** 2          # [HW, HW]
    out = np.zeros((B, C, H, W), dtype=np.int64)
    for b in range(B):
        for c in range(C):
            m = (t[b] == c).reshape(-1)
            if not m.any() or m.all():
                continue
            plane = np.empty(H * W, dtype=np.int64)
            plane[~m] = d2[~m][:, m].min(1)
            plane[m] = -d2[m][:, ~m].min(1)
            out[b, c] = plane.reshape(H, W)
    return out


def _col_dist(mask):
    """distance along axis 0 to the nearest True of mask [H,W] (0 on it; >= _FAR where the column has none)"""
    H = mask.shape[0]
    idx = np.arange(H, dtype=np.int64)[:, None]
    above = np.maximum.accumulate(np.where(mask, idx, -_FAR), 0)
    below = np.minimum.accumulate(np.where(mask, idx, _FAR + H)[::-1], 0)[::-1]
    return np.minimum(idx - above, below - idx)


def _sq_dist_to(mask):
    """squared Euclidean distance of every pixel to the nearest True of mask [H,W] (which has one): columns, then rows"""
    W = mask.shape[1]
    col2 = _col_dist(mask) ** 2                                                   # [H, W']
    x = np.arange(W, dtype=np.int64)
    dx2 = (x[:, None] - x[None, :]) ** 2                                          # [W, W']
    return (dx2[None, :, :] + col2[:, None, :]).min(2)                            # [H, W]


def sdist_separable(labels, C):
    """labels [B,H,W] int -> int64 [B,C,H,W]: O(H W^2) per class"""
    t = np.asarray(labels).astype(np.int64)
    B, H, W = t.shape
    out = np.zeros((B, C, H, W), dtype=np.int64)
    for b in range(B):
        for c in np.unique(t[b]):
            if not 0 <= c < C:
                continue
            m = t[b] == c
            if m.all():
                continue
            out[b, c] = np.where(m, -_sq_dist_to(~m), _sq_dist_to(m))
    return out


def phi(sdist, clip=0.0):
    """signed squared distances -> float64 phi: sqrt outside, -(sqrt - 1) inside, 0 at 0; limited to [-clip, clip] if clip > 0"""
    sd = np.asarray(sdist).astype(np.float64)
    f = np.where(sd > 0, np.sqrt(np.abs(sd)), np.where(sd < 0, 1.0 - np.sqrt(np.abs(sd)), 0.0))
    return np.clip(f, -clip, clip) if clip > 0 else f


def surface_ref(logits, target, clip=0.0, ignore_index=-100, sdist=None):
    """logits [B,C,H,W] (any float), target [B,H,W] int -> (loss, dlogits [B,C,H,W] float64, info).
    info: n_valid, n_bad (out[1:]), valid [B,H,W], sdist int64 [B,C,H,W], phi_max.  sdist: the map, when it is at hand."""
    x = np.asarray(logits, dtype=np.float64)
    B, C, H, W = x.shape
    t = np.asarray(target).astype(np.int64)
    sd = sdist_separable(t, C) if sdist is None else np.asarray(sdist).astype(np.int64)
    f = phi(sd, clip)
    in_range = (t >= 0) & (t < C)
    valid = (t != ignore_index) & in_range
    ex = np.exp(x - x.max(1, keepdims=True))
    p = ex / ex.sum(1, keepdims=True)
    n = int(valid.sum())
    dot = (f * p).sum(1)                                                          # [B,H,W]
    info = {'n_valid': n, 'n_bad': int(((t != ignore_index) & ~in_range).sum()), 'valid': valid, 'sdist': sd,
            'phi_max': float(np.abs(f).max())}
    if n == 0:
        return 0.0, np.zeros_like(x), info
    loss = float(dot[valid].sum() / n)
    grad = p * (f - dot[:, None]) / n * valid[:, None]
    return loss, grad, info


def make_labels(B, C, H, W, seed, outline=True, ignore_frac=0.02, n_bad=3, ignore_index=-100):
    """int64 [B,H,W]: Voronoi cells of a few random sites per image, a class each; with `outline` the pixels whose right or
    lower neighbour lies in another cell are ignore_index (a void outline, like VOC's); about ignore_frac further pixels are
    ignore_index and n_bad (as far as there are pixels) out of range: C, -1, 1000, ...  With B >= 2 the class of image 0's
    first cell is removed from image 1: absent from one image only."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    t = np.empty((B, H, W), dtype=np.int64)
    for b in range(B):
        k = int(min(max(2, H * W // 40), 12))
        sy, sx, sc = rng.randint(0, H, k), rng.randint(0, W, k), rng.randint(0, C, k)
        if C > 1:
            sc[1] = (sc[0] + 1) % C                                               # at least two classes per image
        near = ((yy[None] - sy[:, None, None]) ** 2 + (xx[None] - sx[:, None, None]) ** 2).argmin(0)
        t[b] = sc[near]
    if B >= 2 and C > 1:
        c0 = t[0, 0, 0]
        t[1][t[1] == c0] = (c0 + 1) % C
    cells = t.copy()
    if outline:
        edge = np.zeros_like(t, dtype=bool)
        edge[:, :, :-1] |= cells[:, :, :-1] != cells[:, :, 1:]
        edge[:, :-1, :] |= cells[:, :-1, :] != cells[:, 1:, :]
        t[edge] = ignore_index
    t[rng.rand(B, H, W) < ignore_frac] = ignore_index
    flat = t.reshape(-1)
    where = rng.permutation(flat.size)[:min(n_bad, flat.size // 8)]
    flat[where] = np.array([C, -1, 1000, C + 7, -5])[:len(where)]
    return torch.from_numpy(t)


def make_case(B, C, H, W, std, seed, ignore_index=-100):
    """(fp32 logits N(0, std), make_labels(B, C, H, W, seed))"""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, C, H, W, generator=g, dtype=torch.float64) * std
    return logits.float(), make_labels(B, C, H, W, seed, ignore_index=ignore_index)
