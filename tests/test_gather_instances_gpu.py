"""Every instantiation of the exact-fp32 / limb gather convolution (csrc/conv_gather.hip: 74 kernels), one at a time, against fp64.

tests/test_ops_gpu.py runs its cases wherever the default plan sends them and compares kernel families with each other; here every
row of tests/gather_cases.py FORCES one instantiation with the documented planning switches, asserts through
pseg_debug_last_gather that this instantiation is the one that ran (tests/test_gather_instances_cpu.py shows without a GPU that the
rows reach all 74), and only then compares: with stock torch conv2d / autograd in fp64 on oracle.fill operands, computed once per
problem and never written to.

Per row, the modes it names: the forward plain, with bias, accumulated onto a filled tensor and with the fused BatchNorm statistics
(finalised mean / invstd against the fp64 statistics); the data gradient plain, accumulating, from pre-split limb planes and with
the fused BatchNorm-backward sums (against fp64 sums over the same operands).  Every result tensor starts as NaN, so an element the
kernel did not write fails the comparison; the padding channels must come out zero.  Tap-skipping rows are bit-identical to the same
tile with PSEG_CONV_NOSKIP=1 (a skipped tap contributes exact zeros and each element still sums its live K-steps in ascending
order, whatever the row order), the persistent pointwise kernel to the ring kernel on the same tile (the same products in the same
order per element: test_conv2d_persistent_pointwise_kernel).  One row per tile and kernel family also runs with operands that are
channel slices of wider tensors, whose other columns must keep their bit pattern.

Bounds, relative to the peak of the fp64 result: exact fp32 1e-5 (TOL32: the project's figure for fp32 accumulation, the halo
test's); bf16x3 PREC_TOL['bf16x3'] = 2e-4; bf16x6 and fp16x3 carry (nearly) the whole fp32 significand in their limbs and sum in
fp32, so they are held to what fp32 arithmetic itself achieves: four times the worst error of stock torch's fp32 CPU conv against fp64
on the very problems these rows run.  That error is 2.5e-7 .. 4.7e-7 per problem and its worst 4.2e-7 or 4.7e-7 with the CPU (the conv's
summation order is the CPU library's choice), so the bound is a constant from the smaller measurement, 4 x 4.19e-7 = 1.68e-6, well
under the 1e-4 of test_ops_gpu.py; the references still measure the figure and the last test prints it beside the constant.  The factor allows for another accumulation order and the limb split; nothing here is derived from the kernels
under test.  The statistics use test_conv2d_fwd's formulas with the row's own bound, the sums 1e-5 of the sum of magnitudes
(test_dgrad_with_fused_batchnorm_backward_sums)."""
import contextlib
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

import gather_cases as gc
from oracle import fill

pytestmark = pytest.mark.gpu

TOL32 = 1e-5                   # tests/test_half_gpu.py TOL32, test_conv2d_halo_staged_narrow_3x3
TOL_BF16X3 = 2e-4              # tests/test_ops_gpu.py PREC_TOL['bf16x3']
TOL_LOOSE = 1e-4               # ... PREC_TOL['bf16x6'] / ['fp16x3']: the ceiling of the measured bound
FP32_CPU_ERROR = 4.19e-7       # torch's fp32 CPU conv against fp64, worst over the bf16x6 / fp16x3 problems (fp32_cpu_error(): 4.19e-7, 4.65e-7)
FP32_MARGIN = 4.0
NAN = float('nan')
WORST = {}                     # arithmetic -> (worst error, row id, mode), for the report at the end of the file


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    from pytorch_segmentation_amd import ops as _ops
    return _ops


@contextlib.contextmanager
def switches(monkeypatch, env):
    """the planner overrides, set for the body and undone (and re-read) after it"""
    from pytorch_segmentation_amd import _lib
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    _lib.clear_query_cache()
    try:
        yield
    finally:
        for k in env:
            monkeypatch.delenv(k, raising=False)
        _lib.clear_query_cache()


def ran(launched=True):
    """the record of this thread's last exact-fp32 / limb gather launch (launched: that was the thread's last conv call, so the
    kernel code is pseg_debug_last_conv_kernel's too; a refused call may have moved that code, never the record)"""
    from pytorch_segmentation_amd import _lib
    lib = _lib.load()
    rec = (ctypes.c_int * 13)()
    assert lib.pseg_debug_last_gather(rec) == 0
    assert not launched or rec[gc.KERNEL] == lib.pseg_debug_last_conv_kernel()
    return tuple(rec)


def expect(row, mode, env_note=''):
    got, want = ran(), gc.expected(row, mode)
    assert got == want, '%s (%s%s)\n  ran    %s\n  meant  %s' % (row.id, mode, env_note, gc.describe(got), gc.describe(want))


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()      # (NaN if an element was never written: every bound fails)


@functools.lru_cache(maxsize=None)
def reference(case):
    """operands of a conv problem, its fp64 results, and the error of stock torch's fp32 CPU conv on them; once per module"""
    B, Cin, H, W, Cout, k, stride, pad, dil = case
    key = 'ginst/' + '_'.join(map(str, case))
    x = fill.uniform(key + '/x', (B, Cin, H, W))
    w = fill.uniform(key + '/w', (Cout, Cin, k, k), (6.0 / (Cin * k * k)) ** 0.5)
    b = fill.uniform(key + '/b', (Cout,), 0.5)
    xr, wr = x.double().requires_grad_(), w.double().requires_grad_()
    y = F.conv2d(xr, wr, None, stride, pad, dil)
    gy = fill.uniform(key + '/gy', tuple(y.shape))
    y.backward(gy.double())
    x32 = x.clone().requires_grad_()
    y32 = F.conv2d(x32, w, None, stride, pad, dil)
    y32.backward(gy)
    return dict(x=x, w=w, b=b, gy=gy, y=y.detach(), dx=xr.grad, ybase=fill.uniform(key + '/ybase', tuple(y.shape)),
                xbase=fill.uniform(key + '/xbase', (B, Cin, H, W)), e32=max(rel(y32, y), rel(x32.grad, xr.grad)))


@functools.lru_cache(maxsize=None)
def fp32_cpu_error():
    """the worst error of torch's fp32 CPU conv (forward and data gradient) over the problems the bf16x6 / fp16x3 rows run"""
    return max(reference(case)['e32'] for case in sorted({r.case for r in gc.ROWS if r.prec in (gc.BF16X6, gc.FP16X3)}))


def bound(prec):
    if prec == gc.FP32:
        return TOL32
    if prec == gc.BF16X3:
        return TOL_BF16X3
    return min(TOL_LOOSE, FP32_MARGIN * FP32_CPU_ERROR)


def check(got, want, row, mode, what=''):
    """the comparison with fp64, at the bound of the arithmetic that RAN (the LDS-DMA kernels run exact fp32 whatever was asked)"""
    prec = row.record[gc.PREC]
    e = rel(got, want)
    name = gc.PREC_NAMES[prec]
    print('%-44s %-10s %-8s %.3e (bound %.1e)' % (row.id, mode + what, name, e, bound(prec)))
    if not WORST.get(name, (-1.0,))[0] >= e:
        WORST[name] = (e, row.id, mode + what)
    assert e < bound(prec), '%s (%s%s): %.3e of the peak, bound %.1e' % (row.id, mode, what, e, bound(prec))


_DEVICE = {}


def operands(ops, case):
    """... and their device copies: NHWC activations padded to 4 channels, the filter and its transpose, the padded bias"""
    if case not in _DEVICE:
        B, Cin, H, W, Cout, k, stride, pad, dil = case
        r = reference(case)
        cin_p, cout_p = gc.r4(Cin), gc.r4(Cout)
        w_raw = torch.zeros(cout_p, k, k, cin_p)
        w_raw[:Cout, :, :, :Cin] = r['w'].permute(0, 2, 3, 1)
        w_raw = w_raw.contiguous().cuda()
        b_raw = torch.zeros(cout_p)
        b_raw[:Cout] = r['b']
        xa, gya = ops.Act.from_nchw(r['x'].cuda(), cin_p), ops.Act.from_nchw(r['gy'].cuda(), cout_p)
        wT = ops.filter_transpose(w_raw, cout_p, k * k, cin_p)
        assert torch.equal(wT.view(cin_p, k * k, cout_p), w_raw.view(cout_p, k * k, cin_p).permute(2, 1, 0).contiguous())
        _DEVICE[case] = dict(xa=xa, gya=gya, w_raw=w_raw, wT=wT, b_raw=b_raw.cuda(), Ho=r['y'].shape[2], Wo=r['y'].shape[3],
                             cin_p=cin_p, cout_p=cout_p, amax_x=ops.amax_of(xa), amax_gy=ops.amax_of(gya), amax_w=ops.amax_of(w_raw),
                             amax_wT=ops.amax_of(wT))
    return _DEVICE[case]


def geom(case):
    k, stride, pad, dil = case[5:]
    return k, k, stride, pad, dil


def nan_act(ops, B, H, W, C):
    a = ops.Act.empty(B, H, W, C, 'cuda')
    a.t.fill_(NAN)
    return a


def bn_layer(ops, case):
    """the BatchNorm + ReLU layer in front of a case's conv (its saved y, finalised coefficients) and the fp64 ingredients of
    its backward sums"""
    key = ('bn', case)
    if key not in _DEVICE:
        B, C, H, W = case[:4]
        name = 'ginst/bn/' + '_'.join(map(str, case))
        y = fill.uniform(name + '/y', (B, C, H, W), 2.0) + fill.uniform(name + '/off', (1, C, 1, 1), 1.0)
        g, b = 1.0 + fill.uniform(name + '/g', (C,), 0.3), fill.uniform(name + '/b', (C,), 0.3)
        Cp = gc.r4(C)
        gp, bp = torch.ones(Cp), torch.zeros(Cp)
        gp[:C], bp[:C] = g, b
        ya = ops.Act.from_nchw(y.cuda(), Cp)
        co = ops.bn_finalize(ops.col_stats(ya), ya.M, gp.cuda(), bp.cuda(), torch.zeros(Cp).cuda(), torch.ones(Cp).cuda(), 0.1, 1e-5)
        pre = (y.cuda() - co[0][:C].view(1, C, 1, 1)) * co[2][:C].view(1, C, 1, 1) + co[3][:C].view(1, C, 1, 1)    # fp32, as the kernels decide
        mu, istd = (co[i][:C].double().cpu().view(1, C, 1, 1) for i in range(2))
        _DEVICE[key] = dict(ya=ya, co=co, on=(pre > 0).cpu().double(), xh=(y.double() - mu) * istd)
    return _DEVICE[key]


def check_stats(ops, stats, M, ref, Cout, row, tol):
    """the finalised mean / invstd of fused statistics against those of the fp64 result: test_conv2d_fwd's formulas"""
    st, rows, group = stats
    tile = (row.record[gc.BM], row.record[gc.BN])
    assert rows == -(-M // tile[0]) * gc.WAVE_ROWS[tile] and group == tile[0] // gc.WAVE_ROWS[tile], (row.id, rows, group)
    co = ops.bn_finalize(stats, M, None, None, None, None, 0.0, 1e-5)
    mu, var = ref.mean((0, 2, 3)), ref.var((0, 2, 3), unbiased=False)
    e_mu, e_is = rel(co[0][:Cout], mu), rel(co[1][:Cout], 1.0 / (var + 1e-5).sqrt())
    assert e_mu < tol * max(1.0, (var.sqrt().max() / (mu.abs().max() + 1e-30)).item()) and e_is < tol, (row.id, e_mu, e_is)


def run_fwd(ops, row, mode, xa=None, into=None, note=''):
    """one forward launch of a row -> the result Act (dense, or the slice `into` of a wider buffer)"""
    B, Cin, H, W, Cout = row.case[:5]
    r, d = reference(row.case), operands(ops, row.case)
    acc = mode in ('acc', 'bias+acc')
    want = r['y']
    if into is not None:
        y = into
        ops.copy2d(ops.Act.from_nchw((r['ybase'] if acc else torch.full_like(r['ybase'], NAN)).cuda(), d['cout_p']), y)
    else:
        y = ops.Act.from_nchw(r['ybase'].cuda(), d['cout_p']) if acc else nan_act(ops, B, d['Ho'], d['Wo'], d['cout_p'])
    if acc:
        want = want + r['ybase'].double()
    if mode in ('bias', 'bias+acc'):
        want = want + r['b'].double().view(1, -1, 1, 1)
    am = dict(amax_x=d['amax_x'], amax_w=d['amax_w']) if row.prec == gc.FP16X3 else {}
    stats = ops.conv2d_fwd(d['xa'] if xa is None else xa, d['w_raw'], d['b_raw'] if 'bias' in mode else None, y, *geom(row.case),
                           accumulate=acc, want_stats=mode == 'stats', precision=row.prec, **am)
    expect(row, mode, note)
    check(y.to_nchw(Cout), want, row, mode, note)
    if d['cout_p'] > Cout:       # the padding channels: zero (plus the zero padding of what was accumulated onto)
        assert y.view4()[..., Cout:].abs().max().item() == 0.0, row.id
    if mode == 'stats':
        check_stats(ops, stats, y.M, r['y'], Cout, row, bound(row.record[gc.PREC]))
    return y


def run_dgrad(ops, row, mode, gya=None, into=None, note='', dy_planes=None):
    """one data-gradient launch of a row -> the result Act (gya / dy_planes: dy, or its limb planes, out of a wider tensor)"""
    B, Cin, H, W, Cout = row.case[:5]
    r, d = reference(row.case), operands(ops, row.case)
    acc = mode in ('acc', 'planes+acc')
    want = r['dx'] + r['xbase'].double() if acc else r['dx']
    if into is not None:
        dx = into
        ops.copy2d(ops.Act.from_nchw((r['xbase'] if acc else torch.full_like(r['xbase'], NAN)).cuda(), d['cin_p']), dx)
    else:
        dx = ops.Act.from_nchw(r['xbase'].cuda(), d['cin_p']) if acc else nan_act(ops, B, H, W, d['cin_p'])
    gya = d['gya'] if gya is None else gya
    if mode.startswith('planes'):
        if 'planes' not in d:
            d['planes'] = (ops.split_planes(d['gya']), ops.split_planes(d['wT'].view(d['cin_p'], -1)))
        ops.conv2d_dgrad_planes(d['planes'][0] if dy_planes is None else dy_planes, d['gya'], d['planes'][1], dx, *geom(row.case),
                                accumulate=acc)
    elif mode == 'bns':
        s = bn_layer(ops, row.case)
        ops.conv2d_dgrad(gya, d['wT'], dx, *geom(row.case), precision=row.prec, bn=(s['ya'], s['co'], 1))
    else:
        am = dict(amax_dy=d['amax_gy'], amax_w=d['amax_wT']) if row.prec == gc.FP16X3 else {}
        ops.conv2d_dgrad(gya, d['wT'], dx, *geom(row.case), accumulate=acc, precision=row.prec, **am)
    expect(row, mode, note)
    check(dx.to_nchw(Cin), want, row, mode, note)
    if d['cin_p'] > Cin:
        assert dx.view4()[..., Cin:].abs().max().item() == 0.0, row.id
    if mode == 'bns':
        # the sums against fp64 sums over the fp64 data gradient and the layer's own y: dbeta = sum(dz act'), dgamma = sum(dz act' xhat)
        tile = (row.record[gc.BM], row.record[gc.BN])
        assert dx.bnpart is not None and dx.bnpart.rows == -(-dx.M // tile[0]) * gc.WAVE_ROWS[tile], row.id
        gm = r['dx'] * s['on']
        part = dx.bnpart.part.double().cpu()[:, :, :Cin]
        e_b = (part[0].sum(0) - gm.sum((0, 2, 3))).abs().max().item() / (gm.abs().sum((0, 2, 3)).max().item() + 1e-30)
        e_g = (part[1].sum(0) - (gm * s['xh']).sum((0, 2, 3))).abs().max().item() / ((gm * s['xh']).abs().sum((0, 2, 3)).max().item() + 1e-30)
        assert e_b < 1e-5 and e_g < 1e-5, (row.id, e_b, e_g)
    else:
        assert dx.bnpart is None
    return dx


def run(ops, row, mode, **kw):
    return (run_dgrad if row.dgrad else run_fwd)(ops, row, mode, **kw)


# ------------------------------------------------------------------------------------------------------ every row
@pytest.mark.parametrize('row', gc.ROWS, ids=[r.id for r in gc.ROWS])
def test_row_against_fp64(ops, row, monkeypatch):
    monkeypatch.setattr(ops, 'FUSE_BN_BWD', True)
    with switches(monkeypatch, row.env):
        got = {mode: run(ops, row, mode).t.clone() for mode in row.modes}
    if 'bns' in got:         # the sums ride on the same data gradient
        assert torch.equal(got['bns'], got['plain']), row.id
    for tag, env, flip in (('skip', {'PSEG_CONV_NOSKIP': 1}, lambda rec: rec[gc.SKIP] == 0 and rec[gc.PERM] in (0, 3)),
                           ('pw', {'PSEG_CONV_PW': 0}, lambda rec: rec[gc.KERNEL] == gc.RING)):
        if tag not in row.tags:
            continue
        # the same tile without tap skipping (rows in the dense order) / on the tile-per-block ring kernel: bit-identical tensors
        with switches(monkeypatch, dict(row.env, **env)):
            for mode in row.modes:
                other = (_plain_dgrad if row.dgrad else _plain_fwd)(ops, row, mode)
                rec = ran()
                assert flip(rec) and rec[gc.BM:gc.SKIP] == row.record[gc.BM:gc.SKIP], (row.id, mode, gc.describe(rec))
                assert torch.equal(other.t, got[mode]), '%s (%s): differs from the run with %r' % (row.id, mode, env)


def _plain_fwd(ops, row, mode):
    """the launch of run_fwd without its checks (the comparison runs of the 'skip' and 'pw' tags)"""
    B, Cin, H, W, Cout = row.case[:5]
    r, d = reference(row.case), operands(ops, row.case)
    acc = mode in ('acc', 'bias+acc')
    y = ops.Act.from_nchw(r['ybase'].cuda(), d['cout_p']) if acc else nan_act(ops, B, d['Ho'], d['Wo'], d['cout_p'])
    am = dict(amax_x=d['amax_x'], amax_w=d['amax_w']) if row.prec == gc.FP16X3 else {}
    ops.conv2d_fwd(d['xa'], d['w_raw'], d['b_raw'] if 'bias' in mode else None, y, *geom(row.case), accumulate=acc,
                   want_stats=mode == 'stats', precision=row.prec, **am)
    return y


def _plain_dgrad(ops, row, mode):
    B, Cin, H, W, Cout = row.case[:5]
    r, d = reference(row.case), operands(ops, row.case)
    acc = mode in ('acc', 'planes+acc')
    dx = ops.Act.from_nchw(r['xbase'].cuda(), d['cin_p']) if acc else nan_act(ops, B, H, W, d['cin_p'])
    if mode.startswith('planes'):
        ops.conv2d_dgrad_planes(d['planes'][0], d['gya'], d['planes'][1], dx, *geom(row.case), accumulate=acc)
    elif mode == 'bns':
        s = bn_layer(ops, row.case)
        ops.conv2d_dgrad(d['gya'], d['wT'], dx, *geom(row.case), precision=row.prec, bn=(s['ya'], s['co'], 1))
    else:
        am = dict(amax_dy=d['amax_gy'], amax_w=d['amax_wT']) if row.prec == gc.FP16X3 else {}
        ops.conv2d_dgrad(d['gya'], d['wT'], dx, *geom(row.case), accumulate=acc, precision=row.prec, **am)
    return dx


# ------------------------------------------------------------------------------------------------------ sliced operands
PATTERN = 0x5A5A5A5A           # (a finite float)
SLICE_PAD, SLICE_C0 = 12, 8    # row stride C + 12, the slice 32 bytes into the row


def wide_buffer(ops, like, content=None):
    """a [M][C + 12] buffer filled with a bit pattern, and the `like.C`-channel slice at column 8 of it (holding `content`)"""
    wide = ops.Act.empty(like.B, like.H, like.W, like.C + SLICE_PAD, 'cuda')
    wide.t.view(torch.int32).fill_(PATTERN)
    part = wide.slice(SLICE_C0, SLICE_C0 + like.C)
    if content is not None:
        ops.copy2d(content, part)
    return wide, part


def assert_outside_untouched(wide, C):
    bits = wide.t.view(torch.int32).view(wide.M, wide.ld)
    assert bool((bits[:, :SLICE_C0] == PATTERN).all()) and bool((bits[:, SLICE_C0 + C:] == PATTERN).all()), 'wrote outside its channel slice'


PLANE_PATTERN = 0x5A5A
PLANE_PAD, PLANE_C0 = 16, 8    # plane row stride ldp + 16 halves, the slice 16 bytes into the row


def sliced_planes(ops, pl):
    """the hi / lo planes of `pl` as column slices of pattern-filled [M][ldp + 16] int16 tensors -> (the wide tensors, the argument
    of run_dgrad: Planes with the wider row stride whose pointers start 16 bytes into a row)"""
    ld = pl.ldp + PLANE_PAD
    wide = []
    for src in (pl.hi, pl.lo):
        w = torch.full((pl.M * ld,), PLANE_PATTERN, dtype=torch.int16, device=src.device)
        w.view(pl.M, ld)[:, PLANE_C0:PLANE_C0 + pl.ldp] = src.view(pl.M, pl.ldp)
        wide.append(w)
    return wide, {'dy_planes': ops.Planes(wide[0][PLANE_C0:], wide[1][PLANE_C0:], ld, pl.M, pl.C)}


def assert_planes_untouched(wide, pl):
    for w, src in zip(wide, (pl.hi, pl.lo)):
        bits = w.view(pl.M, -1)
        assert bool((bits[:, :PLANE_C0] == PLANE_PATTERN).all()) and bool((bits[:, PLANE_C0 + pl.ldp:] == PLANE_PATTERN).all())
        assert torch.equal(bits[:, PLANE_C0:PLANE_C0 + pl.ldp], src.view(pl.M, pl.ldp))


SLICED = [r for r in gc.ROWS if 'sliced' in r.tags]


@pytest.mark.parametrize('row', SLICED, ids=[r.id for r in SLICED])
def test_sliced_operands(ops, row, monkeypatch):
    """the gathered operand read out of a channel slice of a wider tensor (ldx > C, a non-zero channel offset; for the pre-split limb
    kernel the hi / lo planes of dy out of wider int16 tensors, ldp + 16 halves a row, 16 bytes in) and the result written
    into one, plain and accumulating (and, forward, with the fused statistics: those of the slice): the instantiation of the row,
    the fp64 result at the row's bound, bit-identical to the dense run, every column outside the slices untouched bit for bit"""
    d = operands(ops, row.case)
    limb = row.record[gc.KERNEL] == gc.LIMB_DMA
    with switches(monkeypatch, row.env):
        src = d['gya'] if row.dgrad else d['xa']
        swide, spart = wide_buffer(ops, src, content=src)
        feed = {'gya': spart} if row.dgrad else {'xa': spart}
        if limb:        # the gathered operand of the pre-split kernel is the pair of planes: those out of wider int16 tensors
            run(ops, row, row.modes[0])                           # (splits the dense planes)
            pwide, feed = sliced_planes(ops, d['planes'][0])
        out_like = ops.Act.empty(src.B, *((row.case[2], row.case[3], d['cin_p']) if row.dgrad else (d['Ho'], d['Wo'], d['cout_p'])), 'cuda')
        for mode in [m for m in row.modes if m in ('plain', 'acc', 'stats', 'planes', 'planes+acc')]:
            dense = run(ops, row, mode)
            owide, opart = wide_buffer(ops, out_like)
            sliced = run(ops, row, mode, into=opart, note=' sliced', **feed)
            assert torch.equal(sliced.view4(), dense.view4()), (row.id, mode)
            assert_outside_untouched(owide, out_like.C)
        assert_outside_untouched(swide, src.C)
        if limb:
            assert_planes_untouched(pwide, d['planes'][0])


# ------------------------------------------------------------------------------------------------------ refusals
def test_refusals_write_nothing(ops, monkeypatch):
    """a forced tile without an instantiation, the sums where no kernel carries them, planes on an uncovered problem, fused statistics
    of a split plan, fp16x3 without amax: an error, the sentinel-filled output and the debug record exactly as they were"""
    from pytorch_segmentation_amd import _lib
    monkeypatch.setattr(ops, 'FUSE_BN_BWD', True)
    refusals = {r[0]: r for r in gc.REFUSALS}

    def refused(name, call, out, match):
        before, rec = out.t.clone(), ran(False)
        with pytest.raises(_lib.PsegError, match=match):
            call()
        torch.cuda.synchronize()
        assert torch.equal(out.t.view(torch.int32), before.view(torch.int32)) and ran(False) == rec, name

    def sentinel(B, H, W, C):
        a = ops.Act.empty(B, H, W, C, 'cuda')
        a.t.view(torch.int32).fill_(PATTERN)
        return a

    d, dT = operands(ops, gc.GRID), operands(ops, gc.GRID_T)
    g, gT = geom(gc.GRID), geom(gc.GRID_T)
    y = sentinel(1, 13, 13, 136)
    dx = sentinel(1, 13, 13, 136)
    ops.conv2d_fwd(d['xa'], d['w_raw'], None, nan_act(ops, 1, 13, 13, 136), *g, precision=gc.FP32)      # (a record to leave alone)
    assert ran()[gc.KERNEL] == gc.RING
    with switches(monkeypatch, refusals['fp32-on-256x128'][5]):
        refused('fp32-on-256x128', lambda: ops.conv2d_fwd(d['xa'], d['w_raw'], None, y, *g, precision=gc.FP32), y, 'no kernel for tile')
    with switches(monkeypatch, refusals['bf16x6-on-256x128'][5]):
        refused('bf16x6-on-256x128', lambda: ops.conv2d_dgrad(dT['gya'], dT['wT'], dx, *gT, precision=gc.BF16X6), dx, 'no kernel for tile')
    s = bn_layer(ops, gc.GRID_T)
    part = torch.zeros(2, 4, 136, device='cuda')
    co = s['co']
    with switches(monkeypatch, refusals['sums-on-the-register-kernel'][5]):
        assert ops._lib.query('pseg_conv2d_dgrad_bnstat_rows', 1, 13, 13, 136, 13, 13, 64, 3, 3, 1, 1, 1) == 0
        refused('sums-on-the-register-kernel',
                lambda: _lib.call('pseg_conv2d_dgrad_bnstat', dT['gya'].ptr, dT['gya'].ld, dT['wT'].data_ptr(), dx.ptr, dx.ld, 1, 13, 13, 136,
                                  13, 13, 64, 3, 3, 1, 1, 1, s['ya'].ptr, s['ya'].ld, co[0].data_ptr(), co[1].data_ptr(), co[2].data_ptr(),
                                  co[3].data_ptr(), 1, part[0].data_ptr(), part[1].data_ptr(), 4, 0), dx, 'part_rows')
        assert part.abs().max().item() == 0.0
    with switches(monkeypatch, refusals['sums-with-accumulate'][5]):
        # the C ABI has no accumulating form of the sums: ops runs the plain accumulating data gradient, no kernel carries sums
        acc = ops.Act.from_nchw(reference(gc.GRID_T)['xbase'].cuda(), 136)
        ops.conv2d_dgrad(dT['gya'], dT['wT'], acc, *gT, accumulate=True, bn=(s['ya'], s['co'], 1))
        assert acc.bnpart is None and ran()[gc.BNS] == 0 and ran()[gc.KERNEL] == gc.RING
        assert rel(acc.to_nchw(), reference(gc.GRID_T)['dx'] + reference(gc.GRID_T)['xbase'].double()) < TOL32
    dl = operands(ops, gc.LIMB)
    planes = (ops.split_planes(dl['gya']), ops.split_planes(dl['wT'].view(dl['cin_p'], -1)))
    with switches(monkeypatch, refusals['planes-uncovered'][5]):
        assert not ops.dgrad_planes_ok(dl['gya'], dx, *geom(gc.LIMB))
        refused('planes-uncovered', lambda: ops.conv2d_dgrad_planes(planes[0], dl['gya'], planes[1], dx, *geom(gc.LIMB)), dx, 'does not cover')
    ws = torch.empty(1 << 20, dtype=torch.uint8, device='cuda')
    stat = torch.zeros(3, 8, 136, device='cuda')

    def fwd_call(precision, stat_ptr):
        return lambda: _lib.call('pseg_conv2d_fwd', d['xa'].ptr, d['xa'].ld, d['w_raw'].data_ptr(), None, y.ptr, y.ld, 1, 13, 13, 64, 13, 13,
                                 136, 3, 3, 1, 1, 1, 0, precision, None, None, stat_ptr, ws.data_ptr(), ws.numel(), None)

    with switches(monkeypatch, refusals['statistics-of-a-split-plan'][5]):
        refused('statistics-of-a-split-plan', fwd_call(gc.FP32, stat.data_ptr()), y, 'splits K')
        assert stat.abs().max().item() == 0.0
    refused('fp16x3-without-amax', fwd_call(gc.FP16X3, None), y, 'amax')


def test_zz_worst_errors():
    """the figures of this run (profiles/EXPERIMENTS.md section 18 quotes them): the fp32 CPU conv's own error, the bound it gives
    the bf16x6 / fp16x3 rows, the worst error per arithmetic"""
    print('\ntorch fp32 CPU conv against fp64, worst over the bf16x6 / fp16x3 problems: %.3e here (constant %.3e -> bound %.3e)'
          % (fp32_cpu_error(), FP32_CPU_ERROR, bound(gc.BF16X6)))
    for name, (e, rid, mode) in sorted(WORST.items()):
        print('worst %-7s %.3e  (%s, %s)' % (name, e, rid, mode))
    # the constant is a measurement of this quantity: a torch whose fp32 conv is far off it means the bound wants measuring again
    assert FP32_CPU_ERROR / 2 < fp32_cpu_error() < FP32_CPU_ERROR * 2 and FP32_CPU_ERROR * FP32_MARGIN < TOL_LOOSE
