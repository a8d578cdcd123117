"""The support kernels of every training step against plain fp64 / bit-exact CPU references, at the sizes where their
launch caps, tails and strides matter.

The conv / BatchNorm / resize / loss calls are recomputed call by call by tests/opcheck.py; what is checked HERE is the rest of
the library -- depthwise convs, the amax reductions, the bf16 limb split, the layout copies, the optimiser and loss-scaler
kernels, argmax and the confusion counters.  Every expected value is built on the CPU from the test's own inputs (drawn with
oracle.fill), never from an entry point of the library, and the inputs reach the device as plain torch tensors (the layout
kernels are under test themselves).

Launch caps, and the case of this file that takes more than one trip through each grid-stride loop:
  dw_fwd_kernel / dw_dgrad_kernel   2048 blocks x 256 lanes = 524 288 items    DW_BIG: 1 048 576 / 786 432 (fwd), 1 048 576 / 3 145 728 (dgrad)
  sgd / adam / mp_check kernels     2048 x 256 lanes x 4 floats = 2 097 152    n = 5 000 000 .. 5 000 003 (three trips)
  amax_kernel                       1024 x 256 lanes = 262 144                 4099 x 1027 = 4 209 673 elements (17 trips)
  amax_batch_kernel                 64 blocks x 256 lanes per job (the arena's table)   3 000 001 elements (184 trips)
  split_planes_kernel               8192 x 256 lanes = 2 097 152 8-column groups    450 001 rows x 5 groups = 2 250 005
  nchw_to_nhwc4 / nchw_to_nhwc8h    2048 x 256 lanes = 524 288 pixels          16 x 512 x 512 = 4 194 304 pixels (eight trips)
  transpose_kernel                  no loop: one 32x32 tile per block          4 x 70 x (131 x 129): 529 x 3 x 4 blocks, ragged both ways
  argmax_kernel / confusion_kernel  4096 / 1024 blocks x 256 lanes             16 x 512 x 512 = 4 194 304 pixels (1 048 576 groups of 4)
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from opcheck import rel_ch
from oracle import fill
from test_half_gpu import TOL32, assert_half_rounded
from test_ops_gpu import TOL

pytestmark = pytest.mark.gpu

SENTINEL = 777.0      # what the memory around an output holds before a call (exact in fp16 too)


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    from pytorch_segmentation_amd import ops as _ops
    return _ops


@pytest.fixture(scope='module')
def lib():
    from pytorch_segmentation_amd import _lib
    return _lib


def rel(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


# ---------------------------------------------------------------------------------------------- depthwise convolution
def _wide(ops, x, c0, ld, dtype, fill_value=SENTINEL):
    """NCHW cpu tensor -> (Act over channels [c0, c0 + C) of a [B,H,W,ld] device buffer, the buffer's Act); the other
    channels hold `fill_value`.  Plain torch copies only."""
    B, C, H, W = x.shape
    buf = torch.full((B, H, W, ld), fill_value, dtype=torch.float32)
    buf[..., c0:c0 + C] = x.permute(0, 2, 3, 1)
    t = buf.to(dtype).reshape(-1).cuda()
    whole = ops.Act(t, B, H, W, ld, ld)
    return (whole.slice(c0, c0 + C) if (c0, C) != (0, ld) else whole), whole


def _nchw64(a):
    return a.view4().detach().cpu().double().permute(0, 3, 1, 2).contiguous()


def _outside_untouched(whole, c0, C, what):
    v = whole.view4().detach().cpu().float()
    keep = torch.ones(whole.ld, dtype=torch.bool)
    keep[c0:c0 + C] = False
    assert (v[..., keep] == SENTINEL).all(), '%s: channels beside the slice were written' % what


# B, C, H, W, k, stride, pad -- with the reason each shape is here (work items = pixels x C/4)
DW_EDGE = [
    (2, 4, 9, 11, 1, 1, 0),       # k = 1, pad 0; one 4-channel chunk (dw_tx = 8 holds seven idle columns); 198 pixels
    (2, 20, 10, 9, 2, 1, 0),      # k = 2; 5 chunks in a column group of 8
    (1, 36, 13, 11, 3, 1, 0),     # k = 3 with pad 0; 9 chunks -> dw_tx = 16, TY = 16: 99 output pixels, not a multiple of 32
    (2, 132, 9, 7, 3, 2, 1),      # stride 2 on odd H and W; 33 chunks -> dw_tx = 64, one column idle... and TY = 4
    (3, 20, 7, 5, 3, 2, 1),       # stride 2, odd, tiny map
    (2, 36, 12, 10, 3, 2, 1),     # stride 2 on even H and W (the last input row / column has no tap)
]
DW_BIG = [
    (8, 32, 128, 128, 3, 1, 1),   # fwd 1 048 576 items, dgrad 1 048 576: two trips each
    (8, 96, 128, 128, 3, 2, 1),   # fwd 786 432 items (two trips), dgrad 3 145 728 (six trips)
]


def _dw_reference(key, B, C, H, W, k, stride, pad, half):
    """inputs + fp64 F.conv2d(groups=C) through autograd, computed ONCE per case"""
    x = fill.uniform(key + '/x', (B, C, H, W))
    w = fill.uniform(key + '/w', (C, 1, k, k), 0.5)
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    gy = fill.uniform(key + '/g', (B, C, Ho, Wo))
    if half:
        x, gy = x.half().float(), gy.half().float()          # the values the fp16 kernels see; the filter stays fp32
    xr, wr = x.double().requires_grad_(), w.double().requires_grad_()
    ref = F.conv2d(xr, wr, None, stride, pad, 1, groups=C)
    ref.backward(gy.double())
    return x, w, gy, ref.detach(), xr.grad, wr.grad, Ho, Wo


def _dw_case(ops, lib, case, half, sliced):
    B, C, H, W, k, stride, pad = case
    q = 8 if half else 4
    if half:
        C = (C + 7) // 8 * 8                                   # fp16 activations carry multiples of 8 channels
    dtype = torch.float16 if half else torch.float32
    key = 'sup/dw/%d_%d_%d_%d_%d_%d' % (C, H, W, k, stride, int(half))
    x, w, gy, ref, dx_ref, dw_ref, Ho, Wo = _dw_reference(key, B, C, H, W, k, stride, pad, half)
    # sliced: every operand is a channel slice of a wider buffer.  The INPUT slices end where their buffer ends (c0 + C == ld),
    # so the last byte the weight gradient's buffer descriptors may reach, (rows - 1) * ld + C, is the buffer's last byte
    ld = C + 3 * q if sliced else C
    c_in = ld - C if sliced else 0
    c_out = q if sliced else 0
    w_raw = w[:, 0].permute(1, 2, 0).contiguous().cuda()      # [k][k][C]
    what = 'dw %s half=%d sliced=%d' % (case, half, sliced)

    def check(got, want, name, dim=1):
        assert not torch.isnan(got).any(), '%s %s: elements left unwritten' % (what, name)
        if half:
            assert_half_rounded(got, want, what + ' ' + name)
        else:
            e, ech = rel(got, want), rel_ch(got, want, dim)
            print('%s %s: %.2e (per channel %.2e)' % (what, name, e, ech))
            assert e < TOL and ech < TOL, (what, name, e, ech)

    xa, _ = _wide(ops, x, c_in, ld, dtype, fill_value=3.0e4)    # a read of a neighbouring channel would be seen
    ya, ywhole = _wide(ops, torch.full((B, C, Ho, Wo), float('nan')), c_out, ld, dtype)
    ops.dwconv_fwd(xa, w_raw, ya, k, stride, pad)
    check(_nchw64(ya), ref, 'fwd')
    _outside_untouched(ywhole, c_out, C, what + ' fwd')

    gya, _ = _wide(ops, gy, c_in, ld, dtype, fill_value=3.0e4)
    dxa, dxwhole = _wide(ops, torch.full((B, C, H, W), float('nan')), c_out, ld, dtype)
    ops.dwconv_dgrad(gya, w_raw, dxa, k, stride, pad)
    check(_nchw64(dxa), dx_ref, 'dgrad')
    _outside_untouched(dxwhole, c_out, C, what + ' dgrad')

    # weight gradient: fp32 always; NaN before the call, a sentinel tail behind it
    n = k * k * C
    dw = torch.full((n + 16,), float('nan'), device='cuda')
    dw[n:] = SENTINEL
    ops.dwconv_wgrad(xa, gya, dw[:n], k, stride, pad)
    want = dw_ref[:, 0].permute(1, 2, 0).contiguous()          # [k][k][C]
    got = dw[:n].view(k, k, C)
    e, ech = rel(got, want), rel_ch(got.double().cpu(), want, 2)
    print('%s wgrad: %.2e (per channel %.2e)' % (what, e, ech))
    tol = TOL32 if half else TOL
    assert e < tol and ech < tol, (what, 'wgrad', e, ech)
    assert (dw[n:] == SENTINEL).all(), what + ': wgrad wrote behind the gradient'
    # fixed-order reduction: a second call gives the same bits, and accumulate adds exactly those bits once more
    first = dw[:n].clone()
    dw2 = torch.full((n,), float('nan'), device='cuda')
    ops.dwconv_wgrad(xa, gya, dw2, k, stride, pad)
    assert torch.equal(dw2, first), what + ': two identical weight-gradient calls differ'
    ops.dwconv_wgrad(xa, gya, dw2, k, stride, pad, accumulate=True)
    assert torch.equal(dw2, first * 2), what + ': accumulate=True is not first + first'

    # a workspace one byte short is refused before anything is launched
    need = lib.query('pseg_dwconv_wgrad_workspace_bytes', B, Ho, Wo, C, k)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    keep = dw2.clone()
    with pytest.raises(lib.PsegError, match=r'\(-3\)'):          # PSEG_ERR_WORKSPACE
        lib.call('pseg_dwconv_wgrad_h' if half else 'pseg_dwconv_wgrad', xa.ptr, xa.ld, gya.ptr, gya.ld, dw2.data_ptr(), B, H,
                 W, C, Ho, Wo, k, stride, pad, 0, ws.data_ptr(), need - 1, ops._stream())
    torch.cuda.synchronize()
    assert torch.equal(dw2, keep)


@pytest.mark.parametrize('half', [False, True], ids=['fp32', 'fp16'])
@pytest.mark.parametrize('case', DW_EDGE, ids=lambda c: 'x'.join(map(str, c)))
def test_depthwise_edges(ops, lib, case, half):
    """Depthwise fwd / dgrad / wgrad on channel slices of wider buffers (ld > C, neighbours untouched), k = 1 / 2 / 3, pad 0,
    stride 2 on odd maps, channel counts that leave dw_tx columns idle (C = 4, 20, 36, 132; fp16: the next multiple of 8),
    pixel counts off the 2 * TY grid; bit-reproducible weight gradient, accumulate, the workspace refusal."""
    _dw_case(ops, lib, case, half, sliced=True)


@pytest.mark.parametrize('half', [False, True], ids=['fp32', 'fp16'])
@pytest.mark.parametrize('case', DW_BIG, ids=lambda c: 'x'.join(map(str, c)))
def test_depthwise_above_the_launch_cap(ops, lib, case, half):
    """More work items than the 2048 x 256 lanes of dw_fwd_kernel / dw_dgrad_kernel (see DW_BIG): the grid-stride loop takes
    2 to 6 trips.  Dense operands (ld == C), one fp64 reference for the three passes."""
    _dw_case(ops, lib, case, half, sliced=False)


# ---------------------------------------------------------------------------------------------- amax
def _amax(ops, lib, t, ld, M, C, out):
    lib.call('pseg_amax', t.data_ptr(), ld, M, C, out.data_ptr(), ops._stream())


@pytest.mark.parametrize('M,C,ld', [(37, 20, 20), (37, 20, 24), (4099, 1027, 1027), (4099, 1027, 1032)],
                         ids=['small', 'small-strided', 'big', 'big-strided'])
def test_amax_is_exactly_abs_max(ops, lib, M, C, ld):
    """pseg_amax == abs().max() of the logical [M][C] block, bit for bit (max and abs are exact).  Below the grid cap
    (740 elements: one block) and above it (4099 x 1027 = 4 209 673 elements on 1024 x 256 lanes: 17 sweeps); contiguous and
    ld > C; the maximum at the first element, at the last, negative, in a padding column (ignored); zeros; in/out."""
    base = torch.full((M, ld), 1.0e30)                          # the padding columns hold a value that must never win
    base[:, :C] = fill.uniform('sup/amax/%d_%d' % (M, ld), (M, C))

    def run(x, out=None):
        out = torch.zeros(1, device='cuda') if out is None else out
        _amax(ops, lib, x.reshape(-1).cuda(), ld, M, C, out)
        return out

    assert torch.equal(run(base).cpu(), base[:, :C].abs().max().reshape(1))
    for m, c, v in ((0, 0, 5.0), (M - 1, C - 1, 7.0), (M // 2, C - 1, -9.0), (M - 1, 0, -3.4028234663852886e38)):
        x = base.clone()
        x[m, c] = v
        want = x[:, :C].abs().max().reshape(1)
        assert want.item() == abs(np.float32(v))
        assert torch.equal(run(x).cpu(), want), (m, c, v)
    zero = base.clone()
    zero[:, :C] = 0.0
    zero[0, 0] = -0.0
    assert torch.equal(run(zero).cpu(), torch.zeros(1))
    # in/out: a running maximum -- a smaller tensor does not lower it, a larger one raises it
    x = base.clone()
    x[M // 3, C // 2] = 11.0
    out = run(x)
    run(base, out)
    assert out.item() == 11.0
    x[M - 1, 1] = -12.5
    run(x, out)
    assert out.item() == 12.5


def _amax_jobs(counts):
    """the job table as ParamArena.filter_amax builds it (arena.py): {address, element count, first block}, 1 to 64 blocks of
    4096 elements per job -- here as (offset, count, first block) rows + the block total"""
    rows, off, blocks = [], 0, 0
    for n in counts:
        rows.append([off, n, blocks])
        blocks += max(1, min(64, (n + 4095) // 4096))
        off += n
    return rows, off, blocks


@pytest.mark.parametrize('counts', [[1], [255], [256], [257], [3000001], [1, 255, 256, 257, 3000001, 5, 4096, 4097],
                                    [1 + (i * 7919) % 70001 for i in range(131)]],
                         ids=['1', '255', '256', '257', '3M', 'mixed', '131-jobs'])
def test_amax_batch_is_exactly_abs_max_per_job(ops, lib, counts):
    """pseg_amax_batch: out[j] == abs().max() of job j, bit for bit.  Jobs of 1 / 255 / 256 / 257 elements (one block, its
    lanes partly idle) and of 3 000 001 (64 blocks x 256 lanes: 184 sweeps); tables of one record and of 131 (the binary
    search over first-block indices); the outputs start as 1e30 and must be overwritten, not raised."""
    rows, total, blocks = _amax_jobs(counts)
    x = fill.uniform('sup/amaxb/%d_%d' % (len(counts), total), (total,), 3.0)
    for j, (off, n, _) in enumerate(rows):                      # every job its own peak, at a position that moves with j
        x[off + (j * 2654435761) % n] = (-1.0) ** j * (4.0 + j)
    xd = x.cuda()
    table = torch.tensor([[xd.data_ptr() + 4 * off, n, first] for off, n, first in rows], dtype=torch.int64, device='cuda')
    out = torch.full((len(rows),), 1.0e30, device='cuda')
    lib.call('pseg_amax_batch', table.data_ptr(), len(rows), blocks, out.data_ptr(), ops._stream())
    want = torch.stack([x[off:off + n].abs().max() for off, n, _ in rows])
    assert torch.equal(out.cpu(), want), (out.cpu() - want).abs().max()
    assert want[-1].item() == 4.0 + len(rows) - 1


# ---------------------------------------------------------------------------------------------- bf16 limb planes
def split_planes_contract(x):
    """include/pseg_amd.h: hi = bf16(x), lo = bf16(x - hi), as uint16 bit patterns (int16 storage).

    The kernel converts with `(__bf16)value` (pack_bf16 in csrc/conv_limb.h: v_cvt_pk_bf16_f32), which rounds to nearest,
    ties to even -- the rounding of torch's `.bfloat16()`; x - hi is exact in fp32 (hi carries the leading 8 bits of x).
    Hand-checked on the CPU (value -> hi, lo):
        1.0                  -> 0x3F80, 0x0000      (zero low limb)
        1 + 2^-8   (a tie)   -> 0x3F80, 0x3B80      (to the even mantissa, DOWN; lo = +2^-8)
        1 + 3*2^-8 (a tie)   -> 0x3F82, 0xBB80      (to the even mantissa, UP; lo = -2^-8)
        -0.0                 -> 0x8000, 0x0000      (-0 - -0 = +0)
        1e-40 (denormal)     -> 0x0001, 0x0000      (71362 * 2^-149: one bf16 denormal step of 2^-133 = 65536 * 2^-149, and a
                                                     residual of 5826 * 2^-149 that rounds to zero)
    """
    hi = x.bfloat16()
    lo = (x - hi.float()).bfloat16()
    return hi.view(torch.int16), lo.view(torch.int16)


SPLIT_SPECIALS = [0.0, -0.0, 1.0, -2.0, 0.5, 1.5, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), 1.0e38, -1.0e38,
                  2.0 ** -126, 1.01 * 2.0 ** -126, -1.5 * 2.0 ** -120, 1.0e-40, -1.0e-40, 2.0 ** -149, -3 * 2.0 ** -149,
                  3.0e-39, 65504.0, 1.0 / 3.0, -1.0e-30]


def test_split_planes_contract_on_known_values():
    """(runs on the CPU) the reference above on the hand-checked handful"""
    x = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -0.0, 1.0e-40])
    hi, lo = split_planes_contract(x)
    u = lambda t: [int(v) & 0xFFFF for v in t.tolist()]
    assert u(hi)[:4] == [0x3F80, 0x3F80, 0x3F82, 0x8000] and u(lo)[:4] == [0x0000, 0x3B80, 0xBB80, 0x0000]
    # 1e-40 = 71362 * 2^-149; bf16's denormal step is 2^-133 = 65536 * 2^-149: hi = 1 step, the rest 5826 * 2^-149 rounds to 0
    assert u(hi)[4] == 0x0001 and u(lo)[4] == 0x0000


@pytest.mark.parametrize('M,C,ldx,ldp', [(450001, 36, 44, 40), (1000, 8, 8, 8), (513, 4, 12, 8), (77, 132, 132, 136)],
                         ids=['above-cap', 'dense', 'C4', 'C132'])
def test_split_planes_matches_the_header_contract(ops, lib, M, C, ldx, ldp):
    """pseg_split_planes against the contract of include/pseg_amd.h computed on the CPU from x (split_planes_contract: RNE, the
    rounding of the kernel's conversion), both planes compared as uint16 bit for bit; columns [C, ldp) zero; the source read
    with ldx > C (its padding columns hold 1e30, which would show in a limb).  450 001 rows x 5 eight-column groups =
    2 250 005 work items on 8192 x 256 = 2 097 152 lanes: a second sweep.  Values with a zero low limb, rounding ties,
    denormal inputs and denormal residuals, both zeros."""
    x = torch.full((M, ldx), 1.0e30)
    x[:, :C] = fill.uniform('sup/split/%d_%d' % (M, C), (M, C))
    x[:, :C] *= 2.0 ** ((torch.arange(M) % 41) - 20).float().view(M, 1)       # a spread of exponents
    sp = torch.tensor(SPLIT_SPECIALS)
    flat = x[:, :C].reshape(-1).clone()
    flat[:sp.numel()] = sp                                     # the first rows ...
    flat[-sp.numel():] = sp.flip(0)                            # ... and the last (second sweep in the large case)
    x[:, :C] = flat.view(M, C)
    hi_ref, lo_ref = split_planes_contract(x[:, :C].contiguous())
    xd = x.reshape(-1).cuda()
    hi = torch.full((M * ldp,), 0x5555, dtype=torch.int16, device='cuda')
    lo = torch.full((M * ldp,), 0x5555, dtype=torch.int16, device='cuda')
    lib.call('pseg_split_planes', xd.data_ptr(), ldx, M, C, hi.data_ptr(), lo.data_ptr(), ldp, ops._stream())
    hi, lo = hi.cpu().view(M, ldp), lo.cpu().view(M, ldp)
    for name, got, want in (('hi', hi, hi_ref), ('lo', lo, lo_ref)):
        bad = got[:, :C] != want
        if bad.any():
            r, c = [int(v[0]) for v in torch.nonzero(bad, as_tuple=True)]
            raise AssertionError('%s plane: %d of %d wrong; first at (%d, %d): x = %r, got 0x%04x, contract 0x%04x' % (
                name, int(bad.sum()), bad.numel(), r, c, x[r, c].item(), int(got[r, c]) & 0xFFFF, int(want[r, c]) & 0xFFFF))
        assert (got[:, C:] == 0).all(), name + ': columns [C, ldp) are not zero'


# ---------------------------------------------------------------------------------------------- layout copies
# B, C, H, W, Cpad, ld
NHWC_CASES = [
    (16, 3, 512, 512, 4, 4),      # C <= 4 into 4-wide pixels: 4 194 304 pixels on 524 288 lanes (eight trips)
    (2, 1, 7, 5, 4, 8),           # ... ld > Cpad
    (3, 4, 9, 9, 4, 4),
    (2, 2, 33, 31, 4, 12),
    (2, 3, 16, 20, 8, 8),         # C <= 4 but Cpad = 8: the tiled transpose
    (2, 21, 17, 19, 24, 28),      # tiled transpose, C and HW off the 32-grid, Cpad > C, ld > Cpad
    (4, 70, 131, 129, 72, 76),    # 529 x 3 x 4 tiles
    (1, 64, 32, 32, 64, 64),      # everything on the grid
]


@pytest.mark.parametrize('B,C,H,W,Cpad,ld', NHWC_CASES, ids=lambda v: str(v))
def test_nchw_to_nhwc_bit_exact(ops, lib, B, C, H, W, Cpad, ld):
    """pseg_nchw_to_nhwc == permute, bit for bit, on both of its kernels; channels [C, Cpad) zero, [Cpad, ld) untouched."""
    x = fill.images('sup/nhwc/%d_%d_%d' % (B, C, H), (B, 3, H, W))[:, :C].contiguous() if C <= 3 else \
        fill.uniform('sup/nhwc/%d_%d_%d' % (B, C, H), (B, C, H, W), 3.0)
    y = torch.full((B, H * W, ld), SENTINEL, device='cuda')
    lib.call('pseg_nchw_to_nhwc', x.cuda().data_ptr(), y.data_ptr(), ld, B, C, H * W, Cpad, ops._stream())
    y = y.cpu()
    assert torch.equal(y[..., :C], x.permute(0, 2, 3, 1).reshape(B, H * W, C))
    assert (y[..., C:Cpad] == 0).all() and (y[..., Cpad:] == SENTINEL).all()


@pytest.mark.parametrize('B,C,H,W,ld', [(2, 21, 17, 19, 28), (4, 70, 131, 129, 76), (1, 64, 32, 32, 64), (3, 2, 9, 7, 4),
                                        (16, 2, 512, 512, 4)], ids=lambda v: str(v))
def test_nhwc_to_nchw_bit_exact(ops, lib, B, C, H, W, ld):
    """pseg_nhwc_to_nchw == permute of the first C channels of a ld > C source, bit for bit (the padding columns hold a value
    that must not appear); the result starts as NaN."""
    src = torch.full((B, H * W, ld), SENTINEL)
    src[..., :C] = fill.uniform('sup/nchw/%d_%d_%d' % (B, C, H), (B, H * W, C), 3.0)
    y = torch.full((B, C, H * W), float('nan'), device='cuda')
    lib.call('pseg_nhwc_to_nchw', src.cuda().data_ptr(), ld, y.data_ptr(), B, C, H * W, ops._stream())
    assert torch.equal(y.cpu(), src[..., :C].permute(0, 2, 1).contiguous())


@pytest.mark.parametrize('B,C,H,W,ld', [(16, 3, 512, 512, 8), (2, 1, 7, 5, 8), (3, 8, 9, 9, 8), (2, 3, 33, 31, 16),
                                        (2, 5, 20, 13, 8)], ids=lambda v: str(v))
def test_nchw_to_nhwc_h_bit_exact(ops, lib, B, C, H, W, ld):
    """pseg_nchw_to_nhwc_h == permute + one rounding to fp16, bit for bit; channels [C, 8) zero, [8, ld) untouched.
    16 x 512 x 512 = 4 194 304 pixels on 524 288 lanes: eight trips."""
    x = fill.images('sup/nhwch/%d_%d_%d' % (B, C, H), (B, 3, H, W))[:, :C].contiguous() if C <= 3 else \
        fill.uniform('sup/nhwch/%d_%d_%d' % (B, C, H), (B, C, H, W), 3.0)
    y = torch.full((B, H * W, ld), SENTINEL, dtype=torch.float16, device='cuda')
    lib.call('pseg_nchw_to_nhwc_h', x.cuda().data_ptr(), y.data_ptr(), ld, B, C, H * W, ops._stream())
    y = y.cpu()
    want = x.permute(0, 2, 3, 1).reshape(B, H * W, C).half()
    assert torch.equal(y[..., :C].contiguous().view(torch.int16), want.view(torch.int16))
    assert (y[..., C:8] == 0).all() and (y[..., 8:] == SENTINEL).all()


# ---------------------------------------------------------------------------------------------- optimisers
def f32(v):
    """a hyper-parameter as the C ABI receives it (float)"""
    return float(np.float32(v))


def sgd_formula(p, g, buf, lr, mu, wd, nesterov, gscale, first):
    """torch.optim.SGD written out, fp64 tensors in place (buf None when mu == 0)"""
    d = g * gscale
    if wd != 0:
        d = d + wd * p
    if mu != 0:
        if first:
            buf.copy_(d)
        else:
            buf.mul_(mu).add_(d)
        d = d + mu * buf if nesterov else buf
    p.sub_(lr * d)


def adam_formula(p, g, m, v, lr, b1, b2, eps, wd, decoupled, gscale, step):
    """torch.optim.Adam / AdamW written out, fp64 tensors in place"""
    d = g * gscale
    if wd != 0:
        if decoupled:
            p.mul_(1 - lr * wd)
        else:
            d = d + wd * p
    m.mul_(b1).add_((1 - b1) * d)
    v.mul_(b2).add_((1 - b2) * d * d)
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    p.sub_((lr / bc1) * m / (v.sqrt() / bc2 ** 0.5 + eps))


def elem_fig(got, ref):
    """per-element figure: max_i |got_i - ref_i| / max(|ref_i|, 1e-2 * peak) -- the convention of opcheck.rel_ch with every
    element its own channel: an error on a small element is not diluted by the largest one"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    peak = ref.abs().max().item()
    return ((got - ref).abs() / (ref.abs().clamp(min=1e-2 * peak) + 1e-300)).max().item()


# name, momentum, weight decay, nesterov, grad_scale, start with first_step
SGD_VARIANTS = [('plain', 0.0, 0.0, False, 1.0, True), ('momentum-wd', 0.9, 1e-2, False, 0.5, True),
                ('nesterov', 0.9, 0.0, True, 0.5, True), ('running', 0.9, 1e-2, True, 0.25, False)]
# name, weight decay, decoupled, grad_scale, first step number
ADAM_VARIANTS = [('plain', 0.0, False, 1.0, 1), ('wd', 1e-2, False, 1.0, 1), ('adamw', 1e-2, True, 0.5, 1),
                 ('running', 1e-2, True, 0.5, 5)]
OPT_NS = [3, 4, 5000000, 5000001, 5000003]
# Distance of torch's own fp32 CPU optimiser from the fp64 formula, measured on the CPU with the inputs of these tests
# (n = 5 000 003, three steps from zero state, elem_fig, worst over the variants above that torch.optim can express):
#     SGD:   parameters 2.44e-06   momentum buffer 6.67e-06
#     Adam:  parameters 8.15e-07   exp_avg 6.03e-06   exp_avg_sq 3.36e-07
# (an absolute error of one fp32 rounding of a value near 1, seen from an element of 1e-2: elem_fig's floor).  The fp64
# formulas themselves agree with torch.optim run in fp64 to 1.4e-14 in the same figure.
# The HIP kernels are fp32 evaluations of the same formula in another operation order: they get four times that.
D_SGD = {'param': 2.44e-06, 'momentum': 6.67e-06}
D_ADAM = {'param': 8.15e-07, 'exp_avg': 6.03e-06, 'exp_avg_sq': 3.36e-07}
BOUND_FACTOR = 4.0


def _opt_inputs(n, running):
    p0 = fill.uniform('sup/opt/p%d' % n, (n,))
    gs = [fill.uniform('sup/opt/g%d_%d' % (n, i), (n,)) for i in range(3)]
    m0 = fill.uniform('sup/opt/m%d' % n, (n,), 0.5) if running else torch.zeros(n)
    v0 = fill.uniform('sup/opt/v%d' % n, (n,), 0.3).abs() if running else torch.zeros(n)
    return p0, gs, m0, v0


def _check_elements(tag, pairs, measured, n):
    """every tensor per element (elem_fig) + the first, last and tail elements on their own; bound = 4 x the measured
    distance of torch's fp32 optimiser for that tensor"""
    edge = sorted(set([0, n - 1] + list(range(n // 4 * 4, n)) + ([n // 4 * 4 - 1] if n >= 4 else [])))
    for name, got, ref in pairs:
        got, ref = got.detach().cpu(), ref.detach().cpu()
        bound = BOUND_FACTOR * measured[name]
        e = elem_fig(got, ref)
        peak = ref.abs().max().item()
        e_edge = max(abs(got[i].item() - ref[i].item()) / max(abs(ref[i].item()), 1e-2 * peak, 1e-300) for i in edge)
        print('%s %s: per-element %.2e, edges %.2e (bound %.2e)' % (tag, name, e, e_edge, bound))
        assert e < bound and e_edge < bound, (tag, name, e, e_edge, bound)


def sgd_torch(p0, gs, lr, mu, wd, nesterov, gscale, dtype):
    pr = p0.to(dtype).clone().requires_grad_()
    opt = torch.optim.SGD([pr], lr=lr, momentum=mu, weight_decay=wd, nesterov=nesterov)
    for g in gs:
        pr.grad = (g.to(dtype) * gscale)
        opt.step()
    return pr.detach(), (opt.state[pr].get('momentum_buffer') if mu != 0 else None)


def adam_torch(p0, gs, lr, b1, b2, eps, wd, decoupled, gscale, dtype):
    pr = p0.to(dtype).clone().requires_grad_()
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)([pr], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    for g in gs:
        pr.grad = (g.to(dtype) * gscale)
        opt.step()
    return pr.detach(), opt.state[pr]['exp_avg'], opt.state[pr]['exp_avg_sq']


def sgd_formula_run(p0, gs, m0, lr, mu, wd, nesterov, gscale, first):
    p, buf = p0.double().clone(), (m0.double().clone() if mu != 0 else None)
    for i, g in enumerate(gs):
        sgd_formula(p, g.double(), buf, lr, mu, wd, nesterov, gscale, first and i == 0)
    return p, buf


def adam_formula_run(p0, gs, m0, v0, lr, b1, b2, eps, wd, decoupled, gscale, step0):
    p, m, v = p0.double().clone(), m0.double().clone(), v0.double().clone()
    for i, g in enumerate(gs):
        adam_formula(p, g.double(), m, v, lr, b1, b2, eps, wd, decoupled, gscale, step0 + i)
    return p, m, v


@pytest.mark.parametrize('n', OPT_NS)
def test_sgd_steps_per_element(ops, lib, n):
    """pseg_sgd_step / pseg_sgd_step_mp, three steps, against torch.optim.SGD's formula written out in fp64 (sgd_formula; on the
    CPU it agrees with torch.optim.SGD run in fp64 to 1e-15 -- asserted here too), per element, parameters and momentum
    buffer.  n = 3 and 4 (tail only / one vector), 5 000 000 / 5 000 001 / 5 000 003 (n % 4 = 0, 1, 3; 1 250 000 vectors on
    524 288 lanes: three trips).  Momentum 0 with a NULL buffer, weight decay, Nesterov, grad_scale != 1, first_step on and
    off.  Bound per tensor: four times the measured distance of torch's fp32 CPU SGD from the same formula (D_SGD:
    parameters 4 x 2.44e-06, momentum buffer 4 x 6.67e-06)."""
    lr = f32(0.1)
    for name, mu, wd, nesterov, gscale, first in SGD_VARIANTS:
        mu, wd, gscale = f32(mu), f32(wd), f32(gscale)
        p0, gs, m0, _ = _opt_inputs(n, running=not first)
        p_ref, b_ref = sgd_formula_run(p0, gs, m0, lr, mu, wd, nesterov, gscale, first)
        if first:      # the formula itself against torch.optim in fp64
            pt, bt = sgd_torch(p0, gs, lr, mu, wd, nesterov, gscale, torch.float64)
            assert elem_fig(pt, p_ref) < 1e-13 and (bt is None or elem_fig(bt, b_ref) < 1e-13)
        for mp in (False, True):
            p = p0.clone().cuda()
            buf = m0.clone().cuda() if mu != 0 else None
            S = 1024.0
            state = torch.zeros(8, device='cuda')
            if mp:
                lib.call('pseg_mp_state_init', state.data_ptr(), S, ops._stream())
                if not first:
                    state[4] = 7.0                              # steps already applied: no first-step form
            for i, g in enumerate(gs):
                if mp:
                    gd = (g * S).cuda()                          # the gradients arrive multiplied by the loss scale (exact)
                    lib.call('pseg_sgd_step_mp', p.data_ptr(), gd.data_ptr(), ops._ptr(buf), n, lr, mu, wd, int(nesterov),
                             gscale, state.data_ptr(), ops._stream())
                    state[4] += 1.0
                else:
                    lib.call('pseg_sgd_step', p.data_ptr(), g.cuda().data_ptr(), ops._ptr(buf), n, lr, mu, wd, int(nesterov),
                             gscale, int(first and i == 0), ops._stream())
            pairs = [('param', p, p_ref)] + ([('momentum', buf, b_ref)] if mu != 0 else [])
            _check_elements('sgd%s[%s] n=%d' % ('_mp' if mp else '', name, n), pairs, D_SGD, n)


@pytest.mark.parametrize('n', OPT_NS)
def test_adam_steps_per_element(ops, lib, n):
    """pseg_adam_step / pseg_adam_step_mp, three steps, against torch.optim.Adam / AdamW's formula written out in fp64
    (adam_formula; agrees with torch.optim in fp64 to 1e-13, asserted here), per element: parameters, exp_avg, exp_avg_sq.
    Sizes as for SGD.  Weight decay 0 / coupled / decoupled, grad_scale != 1, step numbers 1-3 and 5-7 (on running state).
    Bound per tensor: four times the measured distance of torch's fp32 CPU Adam from the same formula (D_ADAM: parameters
    4 x 8.15e-07, exp_avg 4 x 6.03e-06, exp_avg_sq 4 x 3.36e-07)."""
    lr, b1, b2, eps = f32(1e-2), f32(0.9), f32(0.999), f32(1e-8)
    for name, wd, decoupled, gscale, step0 in ADAM_VARIANTS:
        wd, gscale = f32(wd), f32(gscale)
        p0, gs, m0, v0 = _opt_inputs(n, running=step0 > 1)
        p_ref, m_ref, v_ref = adam_formula_run(p0, gs, m0, v0, lr, b1, b2, eps, wd, decoupled, gscale, step0)
        if step0 == 1:
            pt, mt, vt = adam_torch(p0, gs, lr, b1, b2, eps, wd, decoupled, gscale, torch.float64)
            assert elem_fig(pt, p_ref) < 1e-11 and elem_fig(mt, m_ref) < 1e-13 and elem_fig(vt, v_ref) < 1e-13
        for mp in (False, True):
            p, m, v = p0.clone().cuda(), m0.clone().cuda(), v0.clone().cuda()
            S = 1024.0
            state = torch.zeros(8, device='cuda')
            if mp:
                lib.call('pseg_mp_state_init', state.data_ptr(), S, ops._stream())
                state[4] = float(step0 - 1)
            for i, g in enumerate(gs):
                if mp:
                    gd = (g * S).cuda()
                    lib.call('pseg_adam_step_mp', p.data_ptr(), gd.data_ptr(), m.data_ptr(), v.data_ptr(), n, lr, b1, b2, eps,
                             wd, int(decoupled), gscale, state.data_ptr(), ops._stream())
                    state[4] += 1.0
                else:
                    lib.call('pseg_adam_step', p.data_ptr(), g.cuda().data_ptr(), m.data_ptr(), v.data_ptr(), n, lr, b1, b2,
                             eps, wd, int(decoupled), gscale, step0 + i, ops._stream())
            _check_elements('adam%s[%s] n=%d' % ('_mp' if mp else '', name, n),
                            [('param', p, p_ref), ('exp_avg', m, m_ref), ('exp_avg_sq', v, v_ref)], D_ADAM, n)


# ---------------------------------------------------------------------------------------------- loss scaler
FLT_MAX = 3.4028234663852886e38


def _flag(ops, lib, g, n):
    state = torch.zeros(8, device='cuda')
    lib.call('pseg_mp_state_init', state.data_ptr(), 1024.0, ops._stream())
    lib.call('pseg_mp_check', g.data_ptr(), n, state.data_ptr(), ops._stream())
    return state


@pytest.mark.parametrize('n', [5000003, 5000002, 4099, 3])
def test_mp_check_sees_one_bad_value_anywhere(ops, lib, n):
    """pseg_mp_check raises the flag for ONE inf, -inf or NaN at index 0, in the last full vector, at every scalar tail
    position and (n > 2 097 152 = one sweep of 2048 x 256 lanes x 4 floats) beyond the first sweep; not for the largest finite
    float or denormals."""
    g = fill.uniform('sup/mpc/%d' % n, (n,)).cuda()
    n4 = n // 4 * 4
    g[n // 2] = FLT_MAX
    g[n - 1] = -FLT_MAX
    g[0] = 1.0e-40
    g[n // 3] = -2.0 ** -149
    assert _flag(ops, lib, g, n)[3].item() == 0.0, 'finite gradients raised the overflow flag'
    pos = set([0, n - 1] + list(range(n4, n)))
    if n4:
        pos |= {n4 - 1, n4 - 4}
    if n > 2097152:
        pos |= {2097152, 2097152 + 1027, 3000001, 4194304 + 5, n4 - 8}
    for i in sorted(pos):
        for bad in (float('inf'), float('-inf'), float('nan')):
            keep = g[i].item()
            g[i] = bad
            st = _flag(ops, lib, g, n).cpu()
            g[i] = keep
            assert st[3].item() == 1.0, 'a single %r at index %d of %d was not seen' % (bad, i, n)
            assert st[0].item() == 1024.0 and st[4].item() == 0.0 and st[5].item() == 0.0


@pytest.mark.parametrize('adam', [False, True], ids=['sgd', 'adam'])
def test_flagged_mp_step_changes_nothing_at_arena_size(ops, lib, adam):
    """a flagged _mp step leaves parameters and state buffers bit-identical at n = 5 000 003 (three sweeps + a 3-element tail);
    the same step unflagged changes every element"""
    n = 5000003
    p0, gs, m0, v0 = _opt_inputs(n, running=True)
    p, m, v = p0.clone().cuda(), m0.clone().cuda(), v0.clone().cuda()
    g = (gs[0] * 1024.0).cuda()
    g[n - 2] = float('inf')
    state = _flag(ops, lib, g, n)
    assert state[3].item() == 1.0

    def step():
        if adam:
            lib.call('pseg_adam_step_mp', p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, 1e-2, 0.9, 0.999, 1e-8,
                     1e-2, 0, 1.0, state.data_ptr(), ops._stream())
        else:
            lib.call('pseg_sgd_step_mp', p.data_ptr(), g.data_ptr(), m.data_ptr(), n, 1e-2, 0.9, 1e-2, 0, 1.0, state.data_ptr(),
                     ops._stream())
    step()
    assert torch.equal(p.cpu(), p0) and torch.equal(m.cpu(), m0) and torch.equal(v.cpu(), v0)
    g[n - 2] = 1.0
    state[3] = 0.0
    step()
    pc, mc = p.cpu(), m.cpu()
    assert (pc != p0).float().mean().item() > 0.999 and (mc != m0).float().mean().item() > 0.999
    assert (pc[-3:] != p0[-3:]).any() and (pc[:4] != p0[:4]).any()


def test_mp_update_clamps_and_counters(ops, lib):
    """pseg_mp_update: backoff stops at min_scale, growth at max_scale, the tracker restarts on both events, applied / skipped
    steps are counted, and state[1] is exactly 1 / state[0] in fp32."""
    g_ok = torch.ones(8, device='cuda')
    g_bad = g_ok.clone()
    g_bad[5] = float('nan')
    state = torch.zeros(8, device='cuda')

    def step(bad, growth, backoff, interval, lo, hi):
        lib.call('pseg_mp_check', (g_bad if bad else g_ok).data_ptr(), 8, state.data_ptr(), ops._stream())
        assert state[3].item() == (1.0 if bad else 0.0)
        lib.call('pseg_mp_update', state.data_ptr(), growth, backoff, interval, lo, hi, ops._stream())
        s = state.cpu().numpy()
        assert s[3] == 0.0, 'the flag is cleared'
        assert s[1] == np.float32(1.0) / s[0], 'state[1] == 1 / state[0]'
        return [float(v) for v in s[:6]]

    lib.call('pseg_mp_state_init', state.data_ptr(), 4.0, ops._stream())
    assert [float(v) for v in state.cpu()[:6]] == [4.0, 0.25, 0.0, 0.0, 0.0, 0.0]
    # clean steps with growth_interval 2, max_scale 12: 4 -(2 clean)-> 8 -(2 clean)-> min(16, 12) = 12 -> stays 12
    assert step(False, 2.0, 0.5, 2, 3.0, 12.0)[::2] == [4.0, 1.0, 1.0]
    assert step(False, 2.0, 0.5, 2, 3.0, 12.0)[::2] == [8.0, 0.0, 2.0]          # grown, tracker restarted
    assert step(False, 2.0, 0.5, 2, 3.0, 12.0)[::2] == [8.0, 1.0, 3.0]
    assert step(False, 2.0, 0.5, 2, 3.0, 12.0)[::2] == [12.0, 0.0, 4.0]         # clamped at max_scale
    assert step(False, 2.0, 0.5, 2, 3.0, 12.0)[::2] == [12.0, 1.0, 5.0]
    # a flagged step: backoff, tracker restarted (it stood at 1), counted as skipped, not as applied
    s = step(True, 2.0, 0.5, 2, 3.0, 12.0)
    assert s == [6.0, float(np.float32(1.0) / np.float32(6.0)), 0.0, 0.0, 5.0, 1.0]
    s = step(True, 2.0, 0.5, 2, 3.5, 12.0)
    assert s[0] == 3.5 and s[2] == 0.0 and s[4] == 5.0 and s[5] == 2.0          # max(3, min_scale 3.5)
    s = step(True, 2.0, 0.5, 2, 3.5, 12.0)
    assert s[0] == 3.5 and s[5] == 3.0                                          # stays at min_scale
    assert step(False, 2.0, 0.5, 2, 3.5, 12.0)[::2] == [3.5, 1.0, 6.0]
    assert step(False, 2.0, 0.5, 2, 3.5, 12.0)[::2] == [7.0, 0.0, 7.0]


# ---------------------------------------------------------------------------------------------- argmax / confusion
def test_argmax_and_confusion_at_full_size(ops):
    """pseg_argmax at 16 x 21 x 512 x 512 (4 194 304 pixels: 1 048 576 groups of four on 4096 x 256 lanes) == max(1)[1] with the
    first index on ties (ties planted over whole regions, their answer also stated outright); pseg_confusion over the same
    4 194 304 pixels (1024 x 256 lanes: 16 trips) == bincount-based tp / fn / fp as reference test.py:34-46 counts them
    (include/pseg_amd.h; the kernel in csrc/loss.hip): a target outside [0, C) -- the ignore labels -100 and 255, or 21, -1 --
    is in no class's tp / fn, but its prediction still counts as a false positive of the predicted class; a prediction outside
    [0, C) counts nowhere except as the target class's fn.  The counters accumulate."""
    B, C, S = 16, 21, 512
    lg = fill.uniform('sup/am', (B, C, S, S), 3.0)
    lg[0, 5, :64] = 10.0
    lg[0, 9, :64] = 10.0                       # tie 5 / 9 -> 5
    lg[3, 0, 100:200, 7] = 10.0
    lg[3, 20, 100:200, 7] = 10.0               # tie 0 / 20 -> 0
    lg[15, :, 511, 508:] = -1.0                # all equal in the last vector group -> 0
    lg[7, 20, 300, :] = 11.0                   # the last class wins outright
    want = lg.max(1)[1]
    assert (want[0, :64] == 5).all() and (want[3, 100:200, 7] == 0).all() and (want[15, 511, 508:] == 0).all()
    assert (want[7, 300] == 20).all()
    got = ops.argmax(lg.cuda())
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), want)
    del lg

    tg = fill.labels('sup/am/t', (B, S, S), C, block=16)
    tg[1, :40] = 255
    tg[2, 17:90, 300:] = -100
    tg[4, 5, :] = C
    tg[5, :, 3] = -1
    pred = want.clone()
    pred[6, 9, :100] = -1                      # out-of-range predictions (never produced by argmax; the kernel guards them)
    pred[4, 5, :50] = C
    pred[1, :20] = 255
    p, t = pred.reshape(-1), tg.reshape(-1)
    tin, pin = (t >= 0) & (t < C), (p >= 0) & (p < C)
    tp = torch.bincount(t[tin & (p == t)], minlength=C)
    fn = torch.bincount(t[tin], minlength=C) - tp
    fp = torch.bincount(p[pin], minlength=C) - tp
    start = torch.arange(3 * C, dtype=torch.int64).view(3, C) * 1000003
    cnt = start.clone().cuda()
    ops.confusion(pred.cuda(), tg.cuda(), cnt)
    assert torch.equal(cnt.cpu(), start + torch.stack([tp, fn, fp]))
    ops.confusion(pred.cuda(), tg.cuda(), cnt)
    assert torch.equal(cnt.cpu(), start + 2 * torch.stack([tp, fn, fp]))
    assert int(tp.sum() + fn.sum()) == int(tin.sum()) and int(fp.sum()) == int((pin & (p != t)).sum())
