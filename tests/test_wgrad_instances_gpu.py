"""Every reachable instantiation and pixel order of the fp16 weight gradient (wgrad_h_kernel, csrc/conv_half_wgrad.hip) and of the
exact-fp32 LDS-DMA weight gradient (wgrad_f32_dma_kernel, csrc/conv_wgrad.hip), one launch at a time, against fp64.

The rows are tests/wgrad_cases.py's (tests/test_wgrad_instances_cpu.py shows without a GPU that each reaches what it names, and
that together they reach everything that can be reached).  Every row sets its switches, runs, asserts through
pseg_debug_last_wgrad that the launch was the one the table names, and compares with stock torch conv2d + autograd in fp64 on the
same operands (half-rounded for fp16): the plain gradient, the gradient accumulated onto a FILLED tensor, exact zeros in the padded
filter rows / channels, two runs bit-equal; split plans also through a SlabPool.  The bounds are the project's: test_half_gpu.TOL32
(fp16 operands: exact products, fp32 sums) and test_ops_gpu.PREC_TOL['fp32'].  Each case prints its error before it asserts."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

import wgrad_cases as wc
from oracle import fill
from test_half_gpu import CONV_CASES, TOL32, h, r8, rel, to_act_h
from test_half_instances_gpu import assert_outside_untouched, switches, wide_buffer
from test_ops_gpu import PREC_TOL, to_act

pytestmark = pytest.mark.gpu

TOL = {'h': TOL32, 'f': PREC_TOL['fp32']}


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    from pytorch_segmentation_amd import ops as _ops
    return _ops


def ran():
    """the record of this thread's last weight-gradient launch (its kernel code is pseg_debug_last_conv_kernel's answer too)"""
    from pytorch_segmentation_amd import _lib
    lib = _lib.load()
    rec = (ctypes.c_int * 11)()
    assert lib.pseg_debug_last_wgrad(rec) == 0
    assert lib.pseg_debug_last_conv_kernel() == rec[0]
    return tuple(rec)


def expect(row_id, record):
    got = ran()
    assert got == record, 'meant to test %s:\n  %s\nran\n  %s' % (row_id, wc.describe(record), wc.describe(got))


def padded(fmt, c):
    return r8(c) if fmt == 'h' else (c + 3) // 4 * 4


@functools.lru_cache(maxsize=None)
def reference(fmt, case):
    """operands of a weight gradient (half-rounded for fp16), its fp64 result and a filled base to accumulate onto: once per
    module, never written to afterwards"""
    B, Cin, H, W, Cout, k, stride, pad, dil = case
    key = 'wginst/%s/' % fmt + '_'.join(map(str, case))
    rnd = h if fmt == 'h' else (lambda t: t)
    x = rnd(fill.uniform(key + '/x', (B, Cin, H, W)))
    gy = rnd(fill.uniform(key + '/gy', (B, Cout, wc.out_size(H, k, stride, pad, dil), wc.out_size(W, k, stride, pad, dil))))
    wr = torch.zeros(Cout, Cin, k, k, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), wr, None, stride, pad, dil).backward(gy.double())
    base = fill.uniform(key + '/base', (padded(fmt, Cout), k, k, padded(fmt, Cin)))
    return dict(x=x, gy=gy, dw=wr.grad, base=base)


_DEVICE = {}


def operands(ops, fmt, case):
    if (fmt, case) not in _DEVICE:
        r = reference(fmt, case)
        cin_p, cout_p = padded(fmt, case[1]), padded(fmt, case[4])
        if fmt == 'h':
            xa, gya = to_act_h(ops, r['x'], cin_p), to_act_h(ops, r['gy'], cout_p)
        else:
            xa, gya = to_act(ops, r['x'], cin_p), to_act(ops, r['gy'], cout_p)
        _DEVICE[(fmt, case)] = dict(xa=xa, gya=gya, base=r['base'].cuda(), cin_p=cin_p, cout_p=cout_p)
    return _DEVICE[(fmt, case)]


def launch(ops, fmt, case, xa, gya, dw, **kw):
    k, stride, pad, dil = case[5:]
    if fmt == 'f':
        kw['precision'] = ops.PREC_FP32
    ops.conv2d_wgrad(xa, gya, dw, k, k, stride, pad, dil, **kw)


def filled(d, case, value):
    """a gradient tensor holding a value no result has: an element the launch leaves out shows"""
    return torch.full((d['cout_p'], case[5], case[5], d['cin_p']), value, device='cuda')


def live(case, dw):
    """[Cout][Cin][k][k] of a raw [Cout_p][k][k][Cin_p] gradient"""
    return dw[:case[4], :, :, :case[1]].permute(0, 3, 1, 2)


def check_row(ops, row, monkeypatch):
    fmt, case = row.fmt, row.case
    B, Cin, H, W, Cout, k, stride, pad, dil = case
    r, d = reference(fmt, case), operands(ops, fmt, case)
    tol = TOL[fmt]
    base64 = live(case, r['base']).double()
    with switches(monkeypatch, **row.env):
        # plain
        dw = filled(d, case, 7.0)
        launch(ops, fmt, case, d['xa'], d['gya'], dw)
        expect(row.id, row.record)
        err = rel(live(case, dw), r['dw'])
        print('\n%s: rel %.3e (bound %.0e)' % (row.id, err, tol), end='')
        assert err < tol
        # padded filter rows / channels: exact zeros
        if d['cout_p'] > Cout:
            assert dw[Cout:].abs().max().item() == 0.0
        if d['cin_p'] > Cin:
            assert dw[..., Cin:].abs().max().item() == 0.0
        # accumulated onto a filled tensor
        acc = d['base'].clone()
        launch(ops, fmt, case, d['xa'], d['gya'], acc, accumulate=True)
        expect(row.id, row.record)
        err = rel(live(case, acc), base64 + r['dw'])
        print(', accumulate %.3e' % err, end='')
        assert err < tol
        if d['cout_p'] > Cout:
            assert torch.equal(acc[Cout:], d['base'][Cout:])
        if d['cin_p'] > Cin:
            assert torch.equal(acc[..., Cin:], d['base'][..., Cin:])
        # bit-reproducible
        again = filled(d, case, -3.0)
        launch(ops, fmt, case, d['xa'], d['gya'], again)
        assert torch.equal(again, dw)
        if 'centre_only' in row.flags:
            # every tap but the centre one reads padding alone: exact zeros, and the base bit-identical under accumulation
            side = [t for t in range(k * k) if t != (k * k) // 2]
            assert r['dw'].reshape(Cout, Cin, k * k)[:, :, side].abs().max().item() == 0.0
            assert dw.view(d['cout_p'], k * k, d['cin_p'])[:, side].abs().max().item() == 0.0
            assert torch.equal(acc.view(d['cout_p'], k * k, d['cin_p'])[:, side], d['base'].view(d['cout_p'], k * k, d['cin_p'])[:, side])
        if 'deferred' in row.flags:
            # the slabs parked in a pool: dw untouched until the pool folds them, then base + gradient
            assert row.record[9] > 1
            pool = ops.SlabPool(d['base'].device)
            parked = d['base'].clone()
            launch(ops, fmt, case, d['xa'], d['gya'], parked, pool=pool)
            expect(row.id, row.record)
            assert torch.equal(parked, d['base'])
            pool.reduce(accumulate=True)
            err = rel(live(case, parked), base64 + r['dw'])
            print(', deferred %.3e' % err, end='')
            assert err < tol
            assert torch.equal(parked, acc)         # the same slabs in the same order, by either reduction
    return dw


def _ids(rows):
    return [r.id for r in rows]


@pytest.mark.parametrize('row', wc.H_DENSE, ids=_ids(wc.H_DENSE))
def test_half_dense_grid(ops, row, monkeypatch):
    """wgrad_h_kernel<tile, SKIP = false, 32 | 64 pixels per K-step> on maps in 4x8, 2x16 and 1x32 patch order and row-major (63
    and 25 pixels, three sub-steps), and the stem's geometry"""
    check_row(ops, row, monkeypatch)


@pytest.mark.parametrize('row', wc.H_SKIP, ids=_ids(wc.H_SKIP))
def test_half_skipping(ops, row, monkeypatch):
    """wgrad_h_kernel<tile, SKIP = true> with dead patches and with dead image rows skipped (at 64 pixels per K-step a K-step is fed
    from two live sub-steps that need not be neighbours), a problem whose side taps are padding alone, a strided one; and the
    first of them dense under PSEG_CONV_NOSKIP=1"""
    check_row(ops, row, monkeypatch)


@pytest.mark.parametrize('row', wc.H_SPLIT, ids=_ids(wc.H_SPLIT))
def test_half_splits_slabs_remap(ops, row, monkeypatch):
    """forced pixel splits: a last split of one sub-step, a split boundary inside a 64-pixel K-step, splits whose steps are all
    dead, 18 blocks (a remapped head and a tail in wgrad_block) and 16 (no tail); each also through a SlabPool"""
    check_row(ops, row, monkeypatch)


SLICES = [pytest.param((24, 16), (8, 8), id='x-ld+24-dy-last-columns'), pytest.param((8, 8), (24, 8), id='x-last-columns-dy-ld+24')]


@pytest.mark.parametrize('xs,gs', SLICES)
@pytest.mark.parametrize('bkp', wc.BKPS)
@pytest.mark.parametrize('tile,case,patch', wc.H_SLICED,
                         ids=['%dx%d-%s' % (t[0], t[1], 'patches' if p[0] else 'row-major') for t, _, p in wc.H_SLICED])
def test_half_sliced_operands(ops, tile, case, patch, bkp, xs, gs, monkeypatch):
    """x and dy read out of channel slices of wider buffers (row strides + 8 and + 24; one of the two slices is the LAST columns of
    its buffer, where the buffer resource's byte limit is the buffer's end): bit-equal to the dense-operand result, which meets
    fp64, and the pattern around the slices intact"""
    r, d = reference('h', case), operands(ops, 'h', case)
    with switches(monkeypatch, PSEG_HWGRAD_BKP=bkp):
        dense = filled(d, case, 7.0)
        launch(ops, 'h', case, d['xa'], d['gya'], dense)
        rec = ran()
        assert rec[:5] == (wc.WGRAD_H,) + tile + (bkp, 0) and rec[6:9] == patch, wc.describe(rec)
        assert rel(live(case, dense), r['dw']) < TOL32
        xwide, xpart = wide_buffer(ops, d['xa'], d['cin_p'] + xs[0], xs[1], content=d['xa'])
        gwide, gpart = wide_buffer(ops, d['gya'], d['cout_p'] + gs[0], gs[1], content=d['gya'])
        dw = filled(d, case, -3.0)
        launch(ops, 'h', case, xpart, gpart, dw)
        assert ran() == rec
        assert torch.equal(dw, dense)
        assert_outside_untouched(xwide, xs[1], xs[1] + d['cin_p'])
        assert_outside_untouched(gwide, gs[1], gs[1] + d['cout_p'])


@pytest.mark.parametrize('row', wc.F_ROWS, ids=_ids(wc.F_ROWS))
def test_fp32_dma_instances(ops, row, monkeypatch):
    """wgrad_f32_dma_kernel<tile, skip> for every reachable entry of kWgradDmaTiles, in patch order, row-major, packed and with dead
    patches skipped (strided), and the two skipping orders of the register-staged kernel"""
    check_row(ops, row, monkeypatch)


def test_default_plan_of_the_small_half_cases(ops):
    """Which weight-gradient launch the DEFAULT selection gives every CONV_CASES entry of test_half_gpu.py (where
    test_conv2d_dgrad_wgrad_half checks it against fp64), printed and held against tests/wgrad_cases.py's table: a planner change
    that moves the small cases shows here."""
    from pytorch_segmentation_amd import _lib
    _lib.clear_query_cache()
    table = []
    for case in CONV_CASES:
        B, Cin, H, W, Cout, k, stride, pad, dil = case
        g = wc.geometry(case, 'h')
        x = ops.Act.empty(B, H, W, g[3], 'cuda', zero=True, dtype=torch.float16)
        dy = ops.Act.empty(B, g[4], g[5], g[6], 'cuda', zero=True, dtype=torch.float16)
        dw = torch.empty(g[6], k, k, g[3], device='cuda')
        ops.conv2d_wgrad(x, dy, dw, k, k, stride, pad, dil)
        table.append((case, ran()))
    torch.cuda.synchronize()
    print('\ncase, tile, pixels per K-step, SKIP, order, patch_mode, patch, splits, pixels per split')
    for case, rec in table:
        print('%-36s %3dx%-3d  %2d  %d  %d  %d  %dx%-2d  %3d  %d' % ((str(case),) + rec[1:]))
    moved = [(case, rec) for case, rec in table if rec != (wc.WGRAD_H,) + wc.DEFAULT_PLAN_H[case]]
    assert not moved, moved
    assert {wc.instance_h(rec) for _, rec in table} == wc.DEFAULT_REACH_H
