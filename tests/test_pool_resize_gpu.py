"""The kernels of csrc/pool_resize.hip -- bilinear resize (NHWC forward / backward in fp32 and fp16, NHWC -> NCHW forward, the
three forms of the NCHW backward), pool_sum / broadcast and max-pooling -- against tests/resize_ref.py at the edges of their
launch logic.  tests/test_resize_ref_cpu.py holds that reference equal to torch in fp64 on the same cases.

Conventions: inputs come from oracle.fill; an output is NaN before a call that overwrites it (a NaN left counts as unwritten)
and holds a known non-zero value before a call that accumulates; NHWC operands are channel slices of wider buffers whose
other channels hold a sentinel (outputs: must still be there) or 3e4 (inputs: a read of a neighbour shows); fp32 results are
held, in opcheck's `rel` AND `rel_ch`, to max(1e-6, 4 x the error of torch's fp32 CPU result on the same case) <= TOL; fp16
results to one fp16 rounding of the fp64 value computed from the fp16-quantised inputs (assert_half_rounded); max-pool and
broadcast bit for bit.  Every measured figure is printed as `FIG <kernel> <case> rel rel_ch bound`."""
import numpy as np
import pytest
import torch

import resize_ref as R
from oracle import fill
from test_half_gpu import assert_half_rounded
from test_support_ops_gpu import SENTINEL, _nchw64, _outside_untouched, _wide

pytestmark = pytest.mark.gpu

NAN = float('nan')


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    from pytorch_segmentation_amd import ops as _ops
    return _ops


@pytest.fixture(scope='module')
def lib():
    from pytorch_segmentation_amd import _lib
    return _lib


def _check(kernel, what, got, ref, bound, half):
    """got, ref: fp64 cpu, channels in dimension 1"""
    unwritten = int(torch.isnan(got).sum())
    assert unwritten == 0, '%s %s: %d elements left unwritten' % (kernel, what, unwritten)
    if half:
        assert_half_rounded(got, ref, '%s %s' % (kernel, what))
        return
    e, ech = R.rel(got, ref), R.rel_ch(got, ref)
    print('FIG %s %s %.2e %.2e %.2e' % (kernel, what, e, ech, bound))
    assert e < bound and ech < bound, (kernel, what, e, ech, bound)


def _prev(key, shape, half):
    p = fill.uniform(key, shape, 2.0)
    return p.half().float() if half else p


# ---------------------------------------------------------------------------------------------- NCHW backward
# the launch each case of R.NCHW_BWD_CASES must reach when scratch is given.  _nchw_bwd_path is a COPY of the host gate in
# pseg_bilinear_bwd (csrc/pool_resize.hip), not a query of the library: whoever changes that gate updates this copy and
# re-reads the case table, or the cases quietly leave their edges.
NCHW_BWD_PATHS = ['lds', 'lds', 'lds', 'lds', 'reg', 'reg', 'reg', 'reg', 'reg-inplace', 'reg-inplace', 'lds', 'lds', 'reg']
K_MAX_TAPS = 12


def _w_span(Wi, Wo, align):
    """widest run of destination columns one source column feeds with a non-zero fp32 weight"""
    m = R.axis_matrix(Wi, Wo, align)
    return max(int(np.nonzero(m[:, i])[0][-1] - np.nonzero(m[:, i])[0][0]) + 1 for i in range(Wi))


def _nchw_bwd_path(case, aligned):
    B, C, Hi, Wi, Ho, Wo, align = case
    if Wi <= 256 and Wo <= 2048 and Wo % 4 == 0 and aligned and 2 * ((Wo + Wi - 1) // Wi) + 1 <= K_MAX_TAPS:
        return 'lds'
    return 'reg-inplace' if _w_span(Wi, Wo, align) > K_MAX_TAPS else 'reg'


def test_nchw_bwd_cases_sit_on_their_edges():
    """(no kernel runs) the case table still describes the launch logic it was written for"""
    assert [_nchw_bwd_path(c, True) for c in R.NCHW_BWD_CASES] == NCHW_BWD_PATHS
    first = R.NCHW_BWD_CASES[0]
    assert 2 * ((first[5] + first[3] - 1) // first[3]) + 1 == 11 and _w_span(first[3], first[5], 1) == K_MAX_TAPS
    assert _nchw_bwd_path(first, False) == 'reg' and (first[0] * first[1] * first[4]) % 16 != 0      # ragged last row group
    B, C, Hi, Wi, Ho, Wo, align = R.NCHW_BWD_CASES[2]
    assert Wi == 256 and (B * C * Ho) % ((8192 // Wo) * 4) != 0


def _nchw_bwd(ops, lib, case, unaligned):
    B, C, Hi, Wi, Ho, Wo, align = case
    _, gy, _, ref, _, bound = R.resize_reference(case)
    Cp = (C + 3) // 4 * 4
    what = R.case_id(case) + ('+4B' if unaligned else '')
    n = gy.numel()
    if unaligned:          # the gradient starts 4 bytes into a larger tensor
        store = torch.full((n + 8,), 3.0e4, device='cuda')
        gyc = store[1:1 + n]
        gyc.copy_(gy.reshape(-1))
        assert gyc.data_ptr() % 16 == 4
    else:
        gyc = gy.cuda().reshape(-1)
        assert gyc.data_ptr() % 16 == 0
    nbytes = lib.query('pseg_bilinear_bwd_workspace_bytes', B, Hi, Wi, C, Ho, Wo, 1)
    assert nbytes == B * C * Ho * Wi * 4
    ld, c0 = Cp + 8, 4
    key = 'poolresize/prev/' + R.case_id(case)
    prev = _prev(key, (B, Cp, Hi, Wi), False)
    for scratch in (True, False):
        for accumulate in (0, 1):
            ws = torch.full((nbytes // 4 + 16,), NAN, device='cuda')
            ws[nbytes // 4:] = SENTINEL
            start = prev if accumulate else torch.full((B, Cp, Hi, Wi), NAN)
            dxa, whole = _wide(ops, start, c0, ld, torch.float32)
            lib.call('pseg_bilinear_bwd', gyc.data_ptr(), 0, B, Hi, Wi, C, dxa.ptr, dxa.ld, Ho, Wo, align, 1, accumulate,
                     ws.data_ptr() if scratch else 0, nbytes if scratch else 0, ops._stream())
            got = _nchw64(dxa)
            tag = '%s scratch=%d acc=%d' % (what, scratch, accumulate)
            want = ref + prev[:, :C].double() if accumulate else ref
            _check('bilinear_bwd_nchw', tag, got[:, :C], want, bound, False)
            if Cp > C:     # the pad channels of the last group are written as zeros (accumulate: left as they were)
                pad_want = prev[:, C:].double() if accumulate else torch.zeros(B, Cp - C, Hi, Wi, dtype=torch.float64)
                assert torch.equal(got[:, C:], pad_want), tag + ': pad channels'
            _outside_untouched(whole, c0, Cp, 'bilinear_bwd_nchw ' + tag)
            assert (ws[nbytes // 4:] == SENTINEL).all(), tag + ': wrote behind the scratch'
            if not scratch:
                assert torch.isnan(ws[:nbytes // 4]).all()


@pytest.mark.parametrize('case', R.NCHW_BWD_CASES, ids=R.case_id)
def test_bilinear_bwd_nchw_launch_edges(ops, lib, case):
    """pseg_bilinear_bwd(dy_nchw=1) on every branch of its launch logic (R.NCHW_BWD_CASES / NCHW_BWD_PATHS), with scratch
    (W pass + H pass) and without (single gather pass), overwrite then accumulate on a non-zero gradient."""
    _nchw_bwd(ops, lib, case, unaligned=False)


def test_bilinear_bwd_nchw_unaligned_gradient(ops, lib):
    """the LDS-gate case again with dy 4 bytes off a 16-byte boundary: the register W pass, whose 70 rows leave a ragged last
    group of kRowsPerThread = 16"""
    _nchw_bwd(ops, lib, R.NCHW_BWD_CASES[0], unaligned=True)


# ---------------------------------------------------------------------------------------------- NHWC forward / backward
@pytest.mark.parametrize('half', [False, True], ids=['fp32', 'fp16'])
@pytest.mark.parametrize('case', R.NHWC_CASES, ids=R.case_id)
def test_bilinear_nhwc_fwd_bwd(ops, lib, case, half):
    """bilinear_fwd_nhwc_kernel / bilinear_bwd_nhwc_kernel (both storage types) and bilinear_fwd_nchw_kernel on channel
    slices (ld = C + 2 quads): up- and down-sampling, identity, 1x1 sources, scale 8, tap counts far above kMaxTaps, and
    589 824 work items on 2048 x 256 lanes."""
    B, C0, Hi, Wi, Ho, Wo, align = case
    q = 8 if half else 4
    dtype = torch.float16 if half else torch.float32
    x, gy, fwd_ref, bwd_ref, fwd_bound, bwd_bound = R.resize_reference(case, q, half)
    C = x.shape[1]
    ld, c0 = C + 2 * q, q
    what = R.case_id(case)
    sfx = '_h' if half else ''

    xa, _ = _wide(ops, x, c0, ld, dtype, fill_value=3.0e4)
    ya, ywhole = _wide(ops, torch.full((B, C, Ho, Wo), NAN), c0, ld, dtype)
    ops.bilinear_fwd(xa, ya, align)
    _check('bilinear_fwd_nhwc' + sfx, what, _nchw64(ya), fwd_ref, fwd_bound, half)
    _outside_untouched(ywhole, c0, C, 'bilinear_fwd ' + what)

    gya, _ = _wide(ops, gy, c0, ld, dtype, fill_value=3.0e4)
    prev = _prev('poolresize/prevn/' + what, (B, C, Hi, Wi), half)
    for accumulate in (False, True):
        start = prev if accumulate else torch.full((B, C, Hi, Wi), NAN)
        dxa, dxwhole = _wide(ops, start, c0, ld, dtype)
        ops.bilinear_bwd(gya, dxa, align, accumulate=accumulate)
        want = bwd_ref + prev.double() if accumulate else bwd_ref
        _check('bilinear_bwd_nhwc' + sfx, '%s acc=%d' % (what, accumulate), _nchw64(dxa), want, bwd_bound, half)
        _outside_untouched(dxwhole, c0, C, 'bilinear_bwd ' + what)

    if not half:
        n = B * C * Ho * Wo
        out = torch.full((n + 16,), NAN, device='cuda')
        out[n:] = SENTINEL
        lib.call('pseg_bilinear_fwd', xa.ptr, xa.ld, B, Hi, Wi, C, out.data_ptr(), 0, Ho, Wo, align, 1, ops._stream())
        _check('bilinear_fwd_nchw', what, out[:n].view(B, C, Ho, Wo).double().cpu(), fwd_ref, fwd_bound, False)
        assert (out[n:] == SENTINEL).all(), what + ': bilinear_fwd_nchw wrote behind its output'


def test_bilinear_fwd_nchw_21_channels_in_24(ops, lib):
    """21 logit channels in a 24-wide buffer whose last three channels hold 3e4: the last quad is read whole, and only its
    first channel may reach the output"""
    case = R.NCHW_BWD_CASES[7]
    B, C, Hi, Wi, Ho, Wo, align = case
    assert C == 21
    x, _, fwd_ref, _, fwd_bound, _ = R.resize_reference(case)
    xa, _ = _wide(ops, x, 0, 24, torch.float32, fill_value=3.0e4)
    n = B * C * Ho * Wo
    out = torch.full((n + 16,), NAN, device='cuda')
    out[n:] = SENTINEL
    lib.call('pseg_bilinear_fwd', xa.ptr, xa.ld, B, Hi, Wi, C, out.data_ptr(), 0, Ho, Wo, align, 1, ops._stream())
    _check('bilinear_fwd_nchw', R.case_id(case) + ' ld=24', out[:n].view(B, C, Ho, Wo).double().cpu(), fwd_ref, fwd_bound, False)
    assert (out[n:] == SENTINEL).all()


# ---------------------------------------------------------------------------------------------- pool_sum / broadcast
# (B, C, HW).  pool_sum_impl halves tx from 64 while tx > 16 and B * cdiv(C/4, tx) < 512; TY = 256 / tx
POOL_CASES = [
    (1, 4, 1),            # single pixel, single chunk (tx = 16, fifteen columns idle)
    (3, 20, 7),           # HW < TY
    (2, 132, 4099),       # long prime-length column; 33 chunks on tx = 16: three column blocks, the last with one chunk
    (40, 256, 33),        # 64 chunks: 40 x cdiv(64, tx) stays below 512 down to tx = 16 (four column blocks)
    (300, 132, 9),        # 300 x cdiv(33, 32) = 600 >= 512: tx = 32, TY = 8
    (256, 260, 5),        # 256 x cdiv(65, 64) = 512: tx = 64, TY = 4; the second column block holds one chunk
]


@pytest.mark.parametrize('half', [False, True], ids=['fp32', 'fp16'])
@pytest.mark.parametrize('case', POOL_CASES, ids=R.case_id)
def test_pool_sum_and_broadcast(ops, lib, case, half):
    """pool_sum against an fp64 sum; broadcast bit for bit against scale * x rounded to the storage type.

    fp32 pool_sum is held, in `rel` and `rel_ch`, to the bound of every fp32 case of this file: max(1e-6, 4 x the error of
    torch's fp32 CPU `x.sum() * scale` on the same inputs), never above TOL.  Beside it, per element, the first-order bound
    of its summation order: a thread adds at most ceil(HW / 4) terms in sequence (TY = 256 / tx >= 4), thread 0 adds at
    most 16 partial sums (tx >= 16), one product with scale -- at most (ceil(HW/4) + 16 + 1) * 2^-24 * scale * sum_p |x_p|."""
    B, C, HW = case
    q = 8 if half else 4
    C = (C + q - 1) // q * q
    dtype = torch.float16 if half else torch.float32
    what = R.case_id(case)
    x = fill.uniform('poolresize/gap/' + what, (B, C, HW, 1))
    if half:
        x = x.half().float()
    scale = float(np.float32(1.0 / HW))
    ld, c0 = C + 2 * q, q
    xa, _ = _wide(ops, x, c0, ld, dtype, fill_value=3.0e4)
    oa, owhole = _wide(ops, torch.full((B, C, 1, 1), NAN), c0, ld, dtype)
    ops.pool_sum(xa, oa, scale)
    got = _nchw64(oa)
    ref = x.double().sum((2, 3), keepdim=True) * scale
    assert not torch.isnan(got).any(), 'pool_sum %s: elements left unwritten' % what
    if half:
        assert_half_rounded(got, ref, 'pool_sum_h ' + what)
    else:
        t32 = (x.sum((2, 3), keepdim=True) * scale).double()                                  # torch's own fp32 CPU result
        bound = R.bound_from(max(R.rel(t32, ref), R.rel_ch(t32, ref)))
        e, ech = R.rel(got, ref), R.rel_ch(got, ref)
        band = ((HW + 3) // 4 + 17) * 2.0 ** -24 * scale * x.double().abs().sum((2, 3), keepdim=True)
        worst = ((got - ref).abs() / band).max().item()
        print('FIG pool_sum %s %.2e %.2e %.2e (torch fp32: %.2e %.2e; worst error / its summation bound: %.3f)' % (
            what, e, ech, bound, R.rel(t32, ref), R.rel_ch(t32, ref), worst))
        assert e < bound and ech < bound, (what, e, ech, bound)
        assert worst < 1.0, (what, worst)
    _outside_untouched(owhole, c0, C, 'pool_sum ' + what)

    # broadcast: the pooled row of every image over its HW pixels
    src = fill.uniform('poolresize/bc/' + what, (B, C, 1, 1))
    if half:
        src = src.half().float()
    sa, _ = _wide(ops, src, c0, ld, dtype, fill_value=3.0e4)
    prev = torch.round(fill.uniform('poolresize/bcp/' + what, (B, C, HW, 1)) * 8.0)            # integers -8 .. 8
    for bscale, accumulate in ((0.37, False), (1.0, False), (0.25, True)):
        start = prev if accumulate else torch.full((B, C, HW, 1), NAN)
        ya, ywhole = _wide(ops, start, c0, ld, dtype)
        ops.broadcast(sa, ya, bscale, accumulate=accumulate)
        v = src * float(np.float32(bscale))                      # one fp32 product ...
        if accumulate:
            v = prev + v                                         # ... 0.25 * x is exact, so the sum is rounded once however it is fused
        want = v.to(dtype).expand(B, C, HW, 1)                   # ... rounded once more to the storage type
        got = ya.view4().detach().cpu().permute(0, 3, 1, 2)
        assert torch.equal(got, want), 'broadcast %s scale=%g acc=%d: %d elements differ' % (
            what, bscale, accumulate, int((got != want).sum()))
        _outside_untouched(ywhole, c0, C, 'broadcast ' + what)


# ---------------------------------------------------------------------------------------------- max-pool
def _same_bits(a, b):
    """equal, NaN in the same places"""
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(a[~na], b[~nb])


def _pool_input(case, C, special):
    """five distinct values (nearly every window has ties), exact in fp16; special 'inf': whole regions of -inf, so that
    windows see nothing else; 'nan': NaNs that are the first, a middle and the last in-map tap of some window"""
    B, _, H, W, k, stride, pad = case
    x = torch.round(fill.uniform('poolresize/mp/%s/%d' % (R.case_id(case), C), (B, C, H, W)) * 2.0) / 2.0
    assert x.unique().numel() == 5
    if k > H:              # a lone maximum near the far corner: the window of output (0, 0) finds it at its last row and column
        x[0, 0, H - 2, W - 2] = 1.5
    if special == 'inf':
        x[0, 1, :4, :4] = float('-inf')
        x[B - 1, C - 1, H - 3:, W - 3:] = float('-inf')
        x[0, 2] = float('-inf')
    elif special == 'nan':
        for i, (h, w) in enumerate(((1, 1), (2, 2), (0, 0), (H - 1, W - 1), (3, 4), (4, 3))):
            x[i % B, i % C, h, w] = NAN
        x[B - 1, C - 1, 2:5, 2:5] = NAN
        x[0, 3, :4, :4] = float('-inf')
    return x


_POOL_REF = {}


def _pool_reference(case, half, special):
    """inputs + explicit-loop reference, computed once per (case, storage type, special) and shared"""
    key = (case, half, special)
    if key not in _POOL_REF:
        B, C, H, W, k, stride, pad = case
        q = 8 if half else 4
        C = (C + q - 1) // q * q
        x = _pool_input(case, C, special)
        y, arg = R.maxpool_ref(x, k, stride, pad)
        gy = torch.round(fill.uniform('poolresize/mpg/%s/%d' % (R.case_id(case), C), tuple(y.shape)) * 4.0)   # integers -4 .. 4
        dx = R.maxpool_bwd_ref(gy, arg, H, W, k, stride, pad)
        _POOL_REF[key] = (x, y, arg, gy, dx)
    return _POOL_REF[key]


def _maxpool_case(ops, lib, case, half, special):
    B, _, H, W, k, stride, pad = case
    x, y_ref, arg_ref, gy, dx_ref = _pool_reference(case, half, special)
    C = x.shape[1]
    Ho, Wo = y_ref.shape[2:]
    q = 8 if half else 4
    dtype = torch.float16 if half else torch.float32
    sfx = '_h' if half else ''
    what = 'maxpool%s %s %s' % (sfx, R.case_id(case), special)
    ld, c0 = C + 2 * q, q
    if k > H:
        assert int(arg_ref.max()) == k * k - 1
    if special == 'inf':
        assert (y_ref == float('-inf')).any(), 'no window of -inf'
    if special == 'nan':
        taps = set(arg_ref[torch.isnan(y_ref)].tolist())
        assert {0, k * k // 2, k * k - 1} <= taps, 'NaN is not a first, a middle and a last tap'

    xa, _ = _wide(ops, x, c0, ld, dtype, fill_value=3.0e4)
    n = B * Ho * Wo * C
    for want_arg in (True, False):
        ya, ywhole = _wide(ops, torch.full((B, C, Ho, Wo), 12345.0), c0, ld, dtype)          # NaN is a legal result here
        arg = torch.full((n + 16,), 0xFF, dtype=torch.uint8, device='cuda')                   # no window has a tap 255
        lib.call('pseg_maxpool_fwd' + sfx, xa.ptr, xa.ld, B, H, W, C, ya.ptr, ya.ld, arg.data_ptr() if want_arg else 0, Ho, Wo,
                 k, stride, pad, ops._stream())
        got = _nchw64(ya)
        assert _same_bits(got, y_ref), '%s: %d values differ from the reference' % (
            what, int(((got != y_ref) & ~(torch.isnan(got) & torch.isnan(y_ref))).sum()))
        _outside_untouched(ywhole, c0, C, what)
        if want_arg:
            got_arg = arg[:n].view(B, Ho, Wo, C).permute(0, 3, 1, 2).cpu()
            assert torch.equal(got_arg, arg_ref), '%s: %d window positions differ' % (what, int((got_arg != arg_ref).sum()))
            assert (arg[n:] == 0xFF).all(), what + ': wrote behind arg'
        else:
            assert (arg == 0xFF).all()

    # backward, routed by the REFERENCE's positions (independent of the forward above)
    argd = arg_ref.permute(0, 2, 3, 1).contiguous().view(-1).cuda()
    gya, _ = _wide(ops, gy, c0, ld, dtype, fill_value=3.0e4)
    prev = torch.round(fill.uniform('poolresize/mpp/%s' % R.case_id(case), (B, C, H, W)) * 8.0)
    for accumulate in (False, True):
        start = prev if accumulate else torch.full((B, C, H, W), NAN)
        dxa, dxwhole = _wide(ops, start, c0, ld, dtype)
        ops.maxpool_bwd(gya, argd, dxa, k, stride, pad, accumulate=accumulate)
        got = _nchw64(dxa)
        want = dx_ref + prev.double() if accumulate else dx_ref
        assert want.abs().max().item() <= 2048                                                 # exact in fp16
        assert torch.equal(got, want), '%s bwd acc=%d: %d elements differ' % (what, accumulate, int((got != want).sum()))
        _outside_untouched(dxwhole, c0, C, what + ' bwd')
    if (H + 2 * pad - k) % stride != 0 and pad == 0:
        assert (dx_ref[:, :, -1] == 0).all() and (dx_ref[:, :, :, -1] == 0).all()              # floor mode: in no window


@pytest.mark.parametrize('half', [False, True], ids=['fp32', 'fp16'])
@pytest.mark.parametrize('case', R.MAXPOOL_CASES, ids=R.case_id)
def test_maxpool_fwd_bwd_bit_exact(ops, lib, case, half):
    """values, window positions and routed gradients bit for bit on inputs full of ties: k = 2 / 3 / 5 / 15, strides 1 / 2 / 3,
    pad 0 .. 7, floor mode, windows larger than the map; want_argmax on and off; accumulate"""
    _maxpool_case(ops, lib, case, half, 'ties')


@pytest.mark.parametrize('half', [False, True], ids=['fp32', 'fp16'])
@pytest.mark.parametrize('special', ['inf', 'nan'])
def test_maxpool_minus_inf_and_nan(ops, lib, special, half):
    """a window of nothing but -inf gives -inf at its first in-map tap; a NaN that is the first, a middle or the last tap of
    its window gives NaN with arg on a NaN tap (ATen's `val > maxval || isnan(val)`)"""
    _maxpool_case(ops, lib, R.MAXPOOL_CASES[0], half, special)


@pytest.mark.parametrize('half', [False, True], ids=['fp32', 'fp16'])
@pytest.mark.parametrize('act', [0, 1, 2], ids=['none', 'relu', 'relu6'])
@pytest.mark.parametrize('which', [(0, 'nan'), (5, 'ties')], ids=['3x3s2-nan', '5x5s2'])
def test_bn_act_maxpool_equals_the_two_passes(ops, lib, which, act, half):
    """bn_act_maxpool_fwd == bn_act_fwd followed by maxpool_fwd, values and window positions bit for bit, on tie-rich input,
    with NaN and -inf in it, for every activation"""
    case, special = R.MAXPOOL_CASES[which[0]], which[1]
    B, _, H, W, k, stride, pad = case
    x = _pool_reference(case, half, special)[0] * 2.0            # -2 .. 2: ReLU6 has something to clip after scaling
    C = x.shape[1]
    dtype = torch.float16 if half else torch.float32
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    co = torch.stack([fill.uniform('poolresize/bn/mean', (C,), 0.5), torch.ones(C),
                      3.0 + fill.uniform('poolresize/bn/scale', (C,), 1.0), fill.uniform('poolresize/bn/shift', (C,), 0.5)]).cuda()
    xa, _ = _wide(ops, x, 0, C, dtype)
    z = xa.like()
    ops.bn_act_fwd(xa, co, act, z)
    p0, p1, p2 = (ops.Act.empty(B, Ho, Wo, C, 'cuda', zero=True, dtype=dtype) for _ in range(3))
    a0 = ops.maxpool_fwd(z, p0, k, stride, pad)
    a1 = ops.bn_act_maxpool_fwd(xa, co, act, p1, k, stride, pad)
    assert _same_bits(p0.t.float().cpu(), p1.t.float().cpu()) and torch.equal(a0, a1)
    if special == 'nan' and act == 0:
        assert torch.isnan(p1.t).any(), 'no NaN reached the pooled map'
    assert ops.bn_act_maxpool_fwd(xa, co, act, p2, k, stride, pad, want_argmax=False) is None
    assert _same_bits(p0.t.float().cpu(), p2.t.float().cpu())
