"""Plain CPU reference of bilinear resize and max-pooling (numpy / torch, independent of the library), and the case lists
that tests/test_resize_ref_cpu.py (the reference against torch, on the CPU) and tests/test_pool_resize_gpu.py (the kernels
against the reference) share.

  axis_matrix(n_in, n_out, align_corners) -> float64 [n_out, n_in]: one axis of F.interpolate(mode='bilinear') as a matrix.
      The source coordinate is computed in FLOAT32 as csrc/pool_resize.hip promises (ATen's
      area_pixel_compute_source_index), the two weights are taken in float32 and then widened.
  resize_fwd(x, Ho, Wo, align)  = Wh @ x @ Ww^T          in fp64
  resize_bwd(gy, Hi, Wi, align) = Wh^T @ gy @ Ww         in fp64 (the gradient of the above)
  maxpool_ref(x, k, stride, pad) -> (y, arg): explicit loops over the window; arg is the window-local index r*k + s
  maxpool_bwd_ref(gy, arg, H, W, k, stride, pad): gradients routed by arg
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

TOL = 1e-4          # tests/test_ops_gpu.py
BOUND_FACTOR = 4.0  # a kernel may contract the coordinate arithmetic into an FMA and sums its taps in another order: each is
                    # worth about one of torch's own fp32 roundings
BOUND_FLOOR = 1e-6


def rel(got, ref):
    """tests/opcheck.py's tensor-wide figure (restated so that this module needs nothing of the library;
    tests/test_resize_ref_cpu.py holds the two pairs equal)"""
    return ((got - ref).abs().max() / (ref.abs().max() + 1e-30)).item()


def rel_ch(got, ref, dim=1):
    """tests/opcheck.py's per-channel figure: max over channels c of max|err_c| / max(max|ref_c|, 1e-2 * peak)"""
    n = ref.shape[dim]
    g = got.movedim(dim, 0).reshape(n, -1)
    r = ref.movedim(dim, 0).reshape(n, -1)
    ra = r.abs().amax(1)
    den = torch.clamp(ra, min=1e-2 * ra.max().item()) + 1e-30
    return ((g - r).abs().amax(1) / den).max().item()


def axis_matrix(n_in, n_out, align_corners):
    f = np.float32
    o = np.arange(n_out, dtype=np.float32)
    if align_corners:
        scale = f(n_in - 1) / f(n_out - 1) if n_out > 1 else f(0.0)
        s = scale * o
    else:
        scale = f(n_in) / f(n_out)
        s = scale * (o + f(0.5)) - f(0.5)
        s = np.maximum(s, f(0.0))
    assert s.dtype == np.float32
    i0 = np.minimum(s.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = s - i0.astype(np.float32)
    l0 = f(1.0) - l1
    assert l0.dtype == np.float32 and l1.dtype == np.float32
    m = np.zeros((n_out, n_in), dtype=np.float64)
    rows = np.arange(n_out)
    np.add.at(m, (rows, i0), l0.astype(np.float64))
    np.add.at(m, (rows, i1), l1.astype(np.float64))
    return m


def resize_fwd(x, Ho, Wo, align_corners):
    """x [B,C,Hi,Wi] -> fp64 [B,C,Ho,Wo]"""
    x = x.detach().double()
    wh = torch.from_numpy(axis_matrix(x.shape[2], Ho, align_corners))
    ww = torch.from_numpy(axis_matrix(x.shape[3], Wo, align_corners))
    return wh @ x @ ww.t()


def resize_bwd(gy, Hi, Wi, align_corners):
    """gy [B,C,Ho,Wo] -> fp64 [B,C,Hi,Wi]"""
    gy = gy.detach().double()
    wh = torch.from_numpy(axis_matrix(Hi, gy.shape[2], align_corners))
    ww = torch.from_numpy(axis_matrix(Wi, gy.shape[3], align_corners))
    return wh.t() @ gy @ ww


def torch_fp32_error(x, gy, align_corners):
    """How far torch's own fp32 CPU F.interpolate (+ autograd) is from the fp64 reference on these inputs:
    (forward, backward), each the larger of opcheck's rel and rel_ch."""
    Hi, Wi, Ho, Wo = x.shape[2], x.shape[3], gy.shape[2], gy.shape[3]
    xr = x.detach().float().clone().requires_grad_()
    y = F.interpolate(xr, size=(Ho, Wo), mode='bilinear', align_corners=bool(align_corners))
    y.backward(gy.float())
    fwd_ref, bwd_ref = resize_fwd(x, Ho, Wo, align_corners), resize_bwd(gy, Hi, Wi, align_corners)
    fwd, bwd = y.detach().double(), xr.grad.double()
    return (max(rel(fwd, fwd_ref), rel_ch(fwd, fwd_ref)), max(rel(bwd, bwd_ref), rel_ch(bwd, bwd_ref)))


def bound_from(err):
    """the bound a kernel is held to, given torch's fp32 error on the same case"""
    return min(TOL, max(BOUND_FLOOR, BOUND_FACTOR * err))


def maxpool_ref(x, k, stride, pad):
    """x [B,C,H,W] (any float dtype) -> (y fp64 [B,C,Ho,Wo], arg uint8 [B,C,Ho,Wo]).  Window taps are visited row-major; taps
    outside the map are skipped.  A tap is taken when it is the first one in the map, when it is greater than the best so
    far, or when it is a NaN (ATen: `val > maxval || isnan(val)`): the first maximum wins, any NaN makes the output NaN with
    arg on a NaN tap (the last one), and a window of -inf keeps its first in-map tap."""
    x = np.asarray(x.detach().double() if torch.is_tensor(x) else x, dtype=np.float64)
    B, C, H, W = x.shape
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    y = np.zeros((B, C, Ho, Wo), dtype=np.float64)
    arg = np.zeros((B, C, Ho, Wo), dtype=np.uint8)
    for b in range(B):
        for c in range(C):
            for ho in range(Ho):
                for wo in range(Wo):
                    best, pos, seen = 0.0, 0, False
                    for r in range(k):
                        hi = ho * stride - pad + r
                        if hi < 0 or hi >= H:
                            continue
                        for s in range(k):
                            wi = wo * stride - pad + s
                            if wi < 0 or wi >= W:
                                continue
                            v = x[b, c, hi, wi]
                            if not seen or v > best or v != v:
                                best, pos, seen = v, r * k + s, True
                    assert seen
                    y[b, c, ho, wo] = best
                    arg[b, c, ho, wo] = pos
    return torch.from_numpy(y), torch.from_numpy(arg)


def maxpool_bwd_ref(gy, arg, H, W, k, stride, pad):
    """gy [B,C,Ho,Wo], arg as maxpool_ref gives it -> fp64 dx [B,C,H,W]"""
    gy = np.asarray(gy.detach().double() if torch.is_tensor(gy) else gy, dtype=np.float64)
    arg = np.asarray(arg)
    B, C, Ho, Wo = gy.shape
    dx = np.zeros((B, C, H, W), dtype=np.float64)
    for b in range(B):
        for c in range(C):
            for ho in range(Ho):
                for wo in range(Wo):
                    r, s = divmod(int(arg[b, c, ho, wo]), k)
                    hi, wi = ho * stride - pad + r, wo * stride - pad + s
                    assert 0 <= hi < H and 0 <= wi < W
                    dx[b, c, hi, wi] += gy[b, c, ho, wo]
    return torch.from_numpy(dx)


# ---------------------------------------------------------------------------------------------- shared cases
# (B, C, Hi, Wi, Ho, Wo, align): the NCHW backward, each with the launch path it must take in pseg_bilinear_bwd
NCHW_BWD_CASES = [
    (2, 5, 3, 4, 7, 20, 1),         # LDS W pass exactly on the tap gate (11 by 2*ceil(Wo/Wi)+1, 12 real); C off the 4-grid
    (1, 2, 2, 1, 5, 4, 1),          # Wi = 1: wi_pad = 1, all-ones weights
    (1, 3, 4, 256, 8, 1024, 0),     # Wi = 256 (rstep = 1); RB = 8; nrows = 24 is no multiple of RB * kChunks
    (1, 1, 3, 100, 3, 400, 0),      # wi_pad = 128 > Wi: idle threads; nrows = 3 < RB
    (2, 4, 2, 512, 4, 2048, 1),     # Wo = 2048, the last LDS width -- but Wi > 256: register W pass
    (1, 2, 2, 257, 3, 1028, 0),     # Wi = 257: the first register-pass width
    (1, 2, 2, 513, 3, 2052, 0),     # Wo > 2048
    (2, 21, 9, 7, 19, 15, 0),       # Wo % 4 != 0
    (1, 4, 5, 3, 11, 40, 1),        # > kMaxTaps taps: in-place fallback (register W pass / single gather pass)
    (1, 4, 1, 1, 6, 17, 0),         # ... from a single pixel
    (2, 4, 9, 12, 5, 4, 1),         # downsampling
    (1, 4, 16, 6, 4, 24, 0),        # down in H, up in W
    (1, 4, 6, 6, 6, 6, 0),          # identity
]
WIDE = 100                          # cases with Wi >= WIDE exist for the NCHW backward's launch logic only
# the NHWC kernels and bilinear_fwd_nchw: the non-wide cases above (C rounded up to 4 / 8 by the test), plus
NHWC_EXTRA_CASES = [
    (1, 4, 4, 5, 32, 40, 1),        # scale 8 up (HRNet's largest)
    (2, 4, 3, 3, 24, 24, 0),        # ... without align_corners
    (2, 8, 1, 1, 5, 7, 1),          # 1x1 -> HxW
    (2, 8, 64, 64, 384, 384, 0),    # B*Ho*Wo*C/4 = 589 824 > 2048 blocks x 256 lanes: a second trip of the grid-stride loop
]
NHWC_CASES = [c for c in NCHW_BWD_CASES if c[3] < WIDE] + NHWC_EXTRA_CASES
RESIZE_CASES = NCHW_BWD_CASES + NHWC_EXTRA_CASES

# (B, C, H, W, k, stride, pad)
MAXPOOL_CASES = [
    (2, 8, 9, 7, 3, 2, 1),          # the stem's geometry on a small odd map
    (2, 8, 12, 10, 3, 2, 1),        # ... and an even one
    (1, 4, 8, 8, 2, 2, 0),
    (2, 12, 7, 9, 3, 1, 1),         # overlapping windows: up to 9 outputs per input in the backward
    (1, 4, 10, 11, 3, 3, 0),        # floor mode: the last row / column is in no window and gets zero gradient
    (1, 8, 11, 9, 5, 2, 2),
    (1, 4, 9, 9, 15, 1, 7),         # window larger than the map; arg up to 224
]


def case_id(case):
    return 'x'.join(map(str, case))


@functools.lru_cache(maxsize=None)
def resize_inputs(case, Cq=1, half=False):
    """(x, gy) of a resize case, drawn with oracle.fill; C rounded up to a multiple of Cq; half: quantised to fp16."""
    from oracle import fill
    B, C, Hi, Wi, Ho, Wo, align = case
    C = (C + Cq - 1) // Cq * Cq
    key = 'poolresize/%s/%d' % (case_id(case), C)
    x = fill.uniform(key + '/x', (B, C, Hi, Wi))
    gy = fill.uniform(key + '/g', (B, C, Ho, Wo))
    if half:
        x, gy = x.half().float(), gy.half().float()
    return x, gy


@functools.lru_cache(maxsize=None)
def resize_reference(case, Cq=1, half=False):
    """-> (x, gy, fwd_ref, bwd_ref, fwd_bound, bwd_bound): computed once per case and shared (treat as read-only)"""
    B, C, Hi, Wi, Ho, Wo, align = case
    x, gy = resize_inputs(case, Cq, half)
    e_fwd, e_bwd = torch_fp32_error(x, gy, align)
    return (x, gy, resize_fwd(x, Ho, Wo, align), resize_bwd(gy, Hi, Wi, align), bound_from(e_fwd), bound_from(e_bwd))
