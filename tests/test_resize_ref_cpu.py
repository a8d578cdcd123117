"""tests/resize_ref.py against torch in fp64, on the CPU, for every case tests/test_pool_resize_gpu.py runs -- so that what the
kernels are compared with there is known to be F.interpolate(mode='bilinear') / F.max_pool2d and their autograd -- and the
error of torch's own fp32 CPU result on each resize case, from which the GPU file takes its bounds (4 x, never above TOL)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resize_ref as R


def test_metrics_are_those_of_opcheck():
    """resize_ref restates opcheck.rel / rel_ch (it imports nothing of the library); the two pairs agree"""
    import opcheck
    from oracle import fill
    ref = fill.uniform('resizeref/m/r', (2, 5, 4, 3)).double() * torch.tensor([1.0, 1e-3, 0.5, 2.0, 1e-5]).view(1, 5, 1, 1)
    got = ref + 1e-6 * fill.uniform('resizeref/m/e', (2, 5, 4, 3)).double()
    assert R.rel(got, ref) == opcheck.rel(got, ref) and R.rel_ch(got, ref) == opcheck.rel_ch(got, ref)
    assert R.rel_ch(got, ref, 3) == opcheck.rel_ch(got, ref, 3)
    assert R.TOL == 1e-4


def test_axis_matrix_by_hand():
    """2 -> 4 without align_corners: s = 0.5*(o+0.5)-0.5 clamped = 0, 0.25, 0.75, 1.25 (the last one reads pixel 1 twice);
    3 -> 5 with it: s = o/2; 1 -> n: all ones; n -> 1: the first pixel"""
    assert np.array_equal(R.axis_matrix(2, 4, 0), np.array([[1, 0], [0.75, 0.25], [0.25, 0.75], [0, 1]]))
    assert np.array_equal(R.axis_matrix(3, 5, 1), np.array([[1, 0, 0], [.5, .5, 0], [0, 1, 0], [0, .5, .5], [0, 0, 1]]))
    assert np.array_equal(R.axis_matrix(1, 3, 0), np.ones((3, 1))) and np.array_equal(R.axis_matrix(1, 3, 1), np.ones((3, 1)))
    assert np.array_equal(R.axis_matrix(4, 1, 1), np.array([[1, 0, 0, 0]]))
    assert np.array_equal(R.axis_matrix(4, 1, 0), np.array([[0, 0.5, 0.5, 0]]))       # s = 4 * 0.5 - 0.5 = 1.5


@pytest.mark.parametrize('case', R.RESIZE_CASES, ids=R.case_id)
def test_resize_reference_is_torch_fp64_and_bounds_stay_below_tol(case):
    """Wh @ x @ Ww^T == F.interpolate(bilinear) in fp64 and Wh^T @ gy @ Ww == its autograd, up to the fp32 coordinates: the
    reference takes its coordinates in fp32 as the kernels do, torch's fp64 path takes them in fp64.  A coordinate s <= n_in
    carries three fp32 roundings (the scale, the product, the subtraction): |ds| <= 3 * 2^-24 * n_in, which moves the two
    weights by ds and a value by at most 2 * peak * |ds| per axis -- to first order 6 * 2^-24 * (Hi + Wi) of the peak.  The
    assert holds the two to 4 * 2^-24 * max(Hi, Wi), below that (9.5e-7 at a 4-wide source, 1.2e-4 at the 513-wide one;
    measured: at most 2.3 * 2^-24 * max(Hi, Wi), at 64 -> 384).  Then the figure the GPU bounds come from: torch's fp32 CPU
    result against the reference, rel and rel_ch, times 4, below TOL."""
    B, C, Hi, Wi, Ho, Wo, align = case
    for Cq, half in ((1, False), (4, False), (8, True)):
        x, gy, fwd_ref, bwd_ref, fwd_bound, bwd_bound = R.resize_reference(case, Cq, half)
        xr = x.double().requires_grad_()
        y = F.interpolate(xr, size=(Ho, Wo), mode='bilinear', align_corners=bool(align))
        y.backward(gy.double())
        coord = 2.0 ** -24 * max(Hi, Wi) * 4 + 1e-12
        e_f, e_b = R.rel(fwd_ref, y.detach()), R.rel(bwd_ref, xr.grad)
        assert e_f < coord and e_b < coord, (case, e_f, e_b, coord)
        e_fwd, e_bwd = R.torch_fp32_error(x, gy, align)
        print('%s C%%%d: torch fp32 fwd %.2e bwd %.2e -> bounds %.2e %.2e' % (R.case_id(case), Cq, e_fwd, e_bwd, fwd_bound, bwd_bound))
        assert R.BOUND_FACTOR * e_fwd < R.TOL and R.BOUND_FACTOR * e_bwd < R.TOL, (case, e_fwd, e_bwd)
        assert R.BOUND_FLOOR <= fwd_bound <= R.TOL and R.BOUND_FLOOR <= bwd_bound <= R.TOL


def _pool_input(case):
    from oracle import fill
    B, C, H, W, k, stride, pad = case
    return fill.uniform('resizeref/pool/%s' % R.case_id(case), (B, C, H, W)).double()


@pytest.mark.parametrize('case', R.MAXPOOL_CASES, ids=R.case_id)
def test_maxpool_reference_is_torch_fp64(case):
    """on tie-free inputs: values, the arg bytes (against return_indices, converted to window-local r*k+s) and the gradient"""
    B, C, H, W, k, stride, pad = case
    x = _pool_input(case)
    assert x.unique().numel() == x.numel(), 'inputs must be tie-free'
    y, arg = R.maxpool_ref(x, k, stride, pad)
    xr = x.clone().requires_grad_()
    yt, idx = F.max_pool2d(xr, k, stride, pad, return_indices=True)
    assert torch.equal(y, yt.detach())
    Ho, Wo = y.shape[2:]
    hi, wi = idx // W, idx % W
    r = hi - (torch.arange(Ho).view(1, 1, Ho, 1) * stride - pad)
    s = wi - (torch.arange(Wo).view(1, 1, 1, Wo) * stride - pad)
    assert torch.equal(arg.long(), r * k + s)
    from oracle import fill
    gy = fill.uniform('resizeref/poolg/%s' % R.case_id(case), tuple(y.shape)).double()
    yt.backward(gy)
    assert torch.equal(R.maxpool_bwd_ref(gy, arg, H, W, k, stride, pad), xr.grad)


def test_maxpool_reference_ties_nan_and_minus_inf():
    """first maximum in row-major window order; any NaN tap -> NaN with arg on a NaN tap; all -inf -> first in-map tap;
    torch's CPU max_pool2d agrees on all three"""
    x = torch.zeros(1, 1, 4, 4, dtype=torch.float64)
    y, arg = R.maxpool_ref(x, 3, 2, 1)                           # all equal: the first in-map tap of each window
    assert arg.view(-1).tolist() == [4, 3, 1, 0]
    x = torch.full((1, 1, 4, 4), float('-inf'), dtype=torch.float64)
    y, arg = R.maxpool_ref(x, 3, 2, 1)
    assert torch.isinf(y).all() and (y < 0).all() and arg.view(-1).tolist() == [4, 3, 1, 0]
    x = torch.arange(16, dtype=torch.float64).view(1, 1, 4, 4)
    x[0, 0, 1, 1] = float('nan')     # last tap of window (0,0), first of (1,1), tap 2 of (1,0), tap 6 of (0,1)
    y, arg = R.maxpool_ref(x, 3, 2, 1)
    assert torch.isnan(y).all() and arg.view(-1).tolist() == [8, 6, 2, 0]
    yt, idx = F.max_pool2d(x, 3, 2, 1, return_indices=True)
    assert torch.isnan(yt).all() and (idx == 5).all()
    x[0, 0, 1, 1] = 5.0
    x[0, 0, 3, 3] = float('nan')     # only window (1,1) sees it, as its last tap
    y, arg = R.maxpool_ref(x, 3, 2, 1)
    assert torch.isnan(y).view(-1).tolist() == [False, False, False, True] and int(arg[0, 0, 1, 1]) == 8


def test_tap_count_of_every_width_the_lds_pass_accepts():
    """pseg_bilinear_bwd sends a NCHW gradient to the LDS-staged W pass when Wi <= 256, Wo <= 2048, Wo % 4 == 0 and
    2*ceil(Wo/Wi)+1 <= 12; that kernel keeps 12 column weights per source column and has no fallback.  Over every such
    (Wi, Wo), both align modes, the fp32 weights (coordinates rounded as written and as one FMA) of a source column never
    span more than 12 destination columns; the span of 12 is reached at Wi = 4, Wo = 20 with align_corners, where the
    estimate says 11 -- the first case of the GPU file."""
    f = np.float32
    worst = {0: (0, 0, 0), 1: (0, 0, 0)}
    for align in (1, 0):
        for Wi in range(1, 257):
            for Wo in range(4, min(5 * Wi, 2048) + 1, 4):
                assert 2 * ((Wo + Wi - 1) // Wi) + 1 <= 12
                o = np.arange(Wo, dtype=np.float32)
                if align:
                    forms = [(f(Wi - 1) / f(Wo - 1)) * o]
                else:
                    scale = f(Wi) / f(Wo)
                    forms = [scale * (o + f(0.5)) - f(0.5),
                             (np.float64(scale) * (o + f(0.5)).astype(np.float64) - 0.5).astype(np.float32)]
                for s in forms:
                    s = np.maximum(s, f(0.0))
                    i0 = np.minimum(s.astype(np.int64), Wi - 1)
                    i1 = i0 + (i0 < Wi - 1)
                    l1 = s - i0.astype(np.float32)
                    l0 = f(1.0) - l1
                    # i0 and i1 do not decrease with o: the span of source column i is (last o that reads i with a non-zero
                    # weight) - (first such o) + 1
                    idx = np.concatenate([i0[l0 != 0], i1[l1 != 0]])
                    pos = np.concatenate([np.nonzero(l0 != 0)[0], np.nonzero(l1 != 0)[0]])
                    first = np.full(Wi, Wo)
                    last = np.full(Wi, -1)
                    np.minimum.at(first, idx, pos)
                    np.maximum.at(last, idx, pos)
                    span = int((last - first + 1).max())
                    if span > worst[align][0]:
                        worst[align] = (span, Wi, Wo)
    print('widest span: align %s, no align %s' % (worst[1], worst[0]))
    assert worst[1] == (12, 4, 20) and worst[0][0] <= 12


def test_dst_range_lower_end_is_margin():
    """csrc/pool_resize.hip's dst_range starts the backward's gather at floor(flo) - 1, flo = (i - 1) / scale with
    align_corners and (i - 0.5) / scale - 0.5 without.  Destination index o reads source column i only when its coordinate
    s(o) is ABOVE i - 1, that is o > flo, and an o that is exactly flo has weight 0: floor(flo) already holds a whole column
    of margin, and the fp32 rounding of flo (2^-24 * flo) is far below 1 at any size the entry points accept.  So dropping
    that `- 1` changes no result, and no test of values can see it; this enumeration is the evidence: sizes 1..69 -> 1..139
    and the wide shapes of the GPU file, both align modes, s and flo each rounded as written and as one FMA -- the first
    destination index with a non-zero fp32 weight is never below floor(flo)."""
    f = np.float32
    checked = dropped = 0
    for align in (1, 0):
        for n_in in list(range(1, 70)) + [100, 256, 257, 512, 513]:
            for n_out in list(range(1, 140)) + [400, 1024, 1028, 2048, 2052]:
                scale = (f(n_in - 1) / f(n_out - 1) if n_out > 1 else f(0.0)) if align else f(n_in) / f(n_out)
                if scale <= 0:
                    continue                                     # dst_range returns the whole axis
                o = np.arange(n_out, dtype=np.float32)
                i = np.arange(n_in, dtype=np.float32)
                inv = f(1.0) / scale
                if align:
                    coords, flos = [scale * o], [(i - f(1.0)) * inv]
                else:
                    coords = [scale * (o + f(0.5)) - f(0.5),
                              (np.float64(scale) * (o + f(0.5)).astype(np.float64) - 0.5).astype(np.float32)]
                    flos = [(i - f(0.5)) * inv - f(0.5),
                            ((i - f(0.5)).astype(np.float64) * np.float64(inv) - 0.5).astype(np.float32)]
                for s in coords:
                    s = np.maximum(s, f(0.0))
                    i0 = np.minimum(s.astype(np.int64), n_in - 1)
                    i1 = i0 + (i0 < n_in - 1)
                    l1 = s - i0.astype(np.float32)
                    l0 = f(1.0) - l1
                    first = np.full(n_in, n_out)
                    np.minimum.at(first, i0[l0 != 0], np.nonzero(l0 != 0)[0])
                    np.minimum.at(first, i1[l1 != 0], np.nonzero(l1 != 0)[0])
                    fed = first < n_out
                    for flo in flos:
                        lo = np.maximum(np.floor(flo).astype(np.int64), 0)
                        checked += int(fed.sum())
                        dropped += int((lo[fed] > first[fed]).sum())
    print('source columns checked: %d, first taps below floor(flo): %d' % (checked, dropped))
    assert checked > 2000000 and dropped == 0
