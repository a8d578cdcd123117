"""numpy restatement of the local dense-CRF refinement (include/pseg_amd.h, "local dense-CRF refinement of logits"):
shifted slices with explicit in-image masks, every array in `dtype` (float64 for the reference, float32 to measure what
the number format alone costs).

Only the ratios k / sum k of the definition enter the message, so -- as the header states -- each kernel's weights are
taken relative to the pixel's largest one, exp(e - max e): the same ratios in exact arithmetic, and no 0 / 0 in float32
where every neighbour of a pixel is far in colour.  `crf_refine_plain` is the definition without that shift, for the
test that the two agree in float64.
"""
import numpy as np

DEFAULTS = dict(radius=3, dilation=2, iters=5, theta_alpha=8.0, theta_beta=13.0, theta_gamma=3.0, w_appearance=4.0, w_smooth=3.0)


def softmax(x, axis=1):
    e = np.exp(x - x.max(axis=axis, keepdims=True))
    return e / e.sum(axis=axis, keepdims=True)


def _shift(a, oy, ox):
    """a[..., y + oy, x + ox] where that lies inside the image, 0 elsewhere"""
    h, w = a.shape[-2:]
    out = np.zeros_like(a)
    ys, ye = max(0, -oy), min(h, h - oy)
    xs, xe = max(0, -ox), min(w, w - ox)
    if ys < ye and xs < xe:
        out[..., ys:ye, xs:xe] = a[..., ys + oy:ye + oy, xs + ox:xe + ox]
    return out


def _offsets(radius, dilation):
    return [(dy * dilation, dx * dilation) for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1)
            if dy or dx]


def _exponents(guide, guide_scale, radius, dilation, theta_alpha, theta_beta, theta_gamma, dtype):
    """-> (offsets, in-image masks [K,1,1,h,w], appearance exponents [K,B,1,h,w], smoothness exponents [K])"""
    G = np.asarray(guide, dtype=dtype) * np.asarray(guide_scale, dtype=dtype).reshape(1, 3, 1, 1)
    B, _, h, w = G.shape
    offs = _offsets(radius, dilation)
    one = np.ones((1, 1, h, w), dtype=dtype)
    inside = np.stack([_shift(one, oy, ox) for oy, ox in offs])
    d2 = np.array([oy * oy + ox * ox for oy, ox in offs], dtype=dtype)
    two = dtype(2)
    col = np.stack([((G - _shift(G, oy, ox)) ** 2).sum(1, keepdims=True) for oy, ox in offs])
    ea = -d2.reshape(-1, 1, 1, 1, 1) / (two * dtype(theta_alpha) ** 2) - col / (two * dtype(theta_beta) ** 2)
    es = -d2 / (two * dtype(theta_gamma) ** 2)
    return offs, inside, ea, es


def _iterate(U, offs, ka, ks, iters, w_appearance, w_smooth, dtype):
    """ka, ks: [K,B|1,1,h,w] weights, zero outside the image"""
    na, ns = ka.sum(0), ks.sum(0)
    na_safe, ns_safe = np.where(na > 0, na, 1), np.where(ns > 0, ns, 1)      # no in-image neighbour: no message
    Q = softmax(U)
    L = U
    for _ in range(iters):
        ma, ms = np.zeros_like(U), np.zeros_like(U)
        for k, (oy, ox) in enumerate(offs):
            Qs = _shift(Q, oy, ox)
            ma += ka[k] * Qs
            ms += ks[k] * Qs
        L = U + (dtype(w_appearance) * (ma / na_safe) + dtype(w_smooth) * (ms / ns_safe))
        Q = softmax(L)
    return L


def crf_refine(logits, guide, guide_scale, radius=3, dilation=2, iters=5, theta_alpha=8.0, theta_beta=13.0, theta_gamma=3.0,
               w_appearance=4.0, w_smooth=3.0, dtype=np.float64):
    """logits [B,C,h,w], guide [B,3,h,w], guide_scale (3) -> L^T [B,C,h,w] in `dtype`"""
    dtype = np.dtype(dtype).type
    U = np.asarray(logits, dtype=dtype)
    if w_appearance == 0 and w_smooth == 0:
        return U.copy()
    offs, inside, ea, es = _exponents(guide, guide_scale, radius, dilation, theta_alpha, theta_beta, theta_gamma, dtype)
    neg = dtype(-np.inf)
    ea = np.where(inside > 0, ea, neg)
    es = np.where(inside > 0, es.reshape(-1, 1, 1, 1, 1), neg)
    ma, ms = ea.max(0, keepdims=True), es.max(0, keepdims=True)
    with np.errstate(invalid='ignore'):                        # -inf - -inf where a pixel has no in-image neighbour
        ka = np.where(inside > 0, np.exp(ea - ma), 0).astype(dtype)
        ks = np.where(inside > 0, np.exp(es - ms), 0).astype(dtype)
    return _iterate(U, offs, ka, ks, iters, w_appearance, w_smooth, dtype)


def crf_refine_plain(logits, guide, guide_scale, radius=3, dilation=2, iters=5, theta_alpha=8.0, theta_beta=13.0,
                     theta_gamma=3.0, w_appearance=4.0, w_smooth=3.0, dtype=np.float64):
    """the definition word for word: weights exp(e), no shift by the largest exponent"""
    dtype = np.dtype(dtype).type
    U = np.asarray(logits, dtype=dtype)
    offs, inside, ea, es = _exponents(guide, guide_scale, radius, dilation, theta_alpha, theta_beta, theta_gamma, dtype)
    ka = np.exp(ea) * inside
    ks = np.exp(es).reshape(-1, 1, 1, 1, 1) * inside
    return _iterate(U, offs, ka, ks, iters, w_appearance, w_smooth, dtype)


def top_two_gap(L):
    """[B,h,w]: the largest minus the second largest value over the classes (inf with one class)"""
    if L.shape[1] == 1:
        return np.full((L.shape[0],) + L.shape[2:], np.inf)
    s = np.sort(L, axis=1)
    return s[:, -1] - s[:, -2]


# the parity cases of tests/test_crf_gpu.py: (B, C, h, w, options)
CASES = [
    (3, 21, 37, 45, {}),
    (2, 2, 5, 70, dict(radius=5, dilation=4)),
    (1, 37, 33, 19, dict(radius=1, dilation=1, iters=10)),
    (2, 8, 64, 64, dict(radius=2, dilation=3, iters=1)),
    (1, 9, 21, 50, dict(radius=3, dilation=4, iters=2)),      # the narrow class chunk with more than one chunk
]
NORMS = {'dataset': ((123.675, 116.28, 103.53), (58.395, 57.12, 57.375)), 'reference': ((0.0, 0.0, 0.0), (255.0, 255.0, 255.0))}


def case_inputs(B, C, h, w, norm, seed):
    """logits = 4 x standard normal; the guide = random 8-bit values normalised as `norm` does, in float32 as the
    preprocess kernel delivers it -> (logits fp32, guide fp32, guide_scale)"""
    rng = np.random.RandomState(seed)
    logits = (4 * rng.standard_normal((B, C, h, w))).astype(np.float32)
    mean, std = NORMS[norm]
    raw = rng.randint(0, 256, (B, 3, h, w)).astype(np.float32)
    guide = (raw - np.float32(mean).reshape(1, 3, 1, 1)) / np.float32(std).reshape(1, 3, 1, 1)
    return logits, guide.astype(np.float32), std
