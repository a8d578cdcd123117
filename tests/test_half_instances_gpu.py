"""Every instantiation of the fp16 gather convolution (csrc/conv_half_gather.hip), one at a time, against fp64.

gather_h_kernel (ring) and gather_hp_kernel (persistent) are instantiated over four tiles x two K-steps x ring depths 2..4 x the
plain / tap-skipping / GENERIC variants (+ the siblings with the fused BatchNorm-backward sums).  tests/test_half_gpu.py runs its
cases wherever the default selection sends them; here every case FORCES one instantiation with the documented switches
(PSEG_CONV_BM / _BN, PSEG_HCONV_KB, PSEG_HCONV_STAGES, PSEG_HCONV_PERSIST, PSEG_CONV_NOSKIP) and asserts, through
pseg_debug_last_conv_kernel / pseg_debug_last_gather_h, that this instantiation is the one that ran.  The reference is stock torch
conv2d / autograd in fp64 on the same half-rounded operands, computed once per shape; the bounds are those of test_half_gpu.py
(1e-5 of the peak for fp32 results, one fp16 rounding for fp16 results, 1e-4 for the finalised statistics).

The ring-grid problem is 3x3, pad 1, 1 x 64 x 13 x 13 -> 136 channels: M = 169 (two ragged 128-row tiles / three 64-row ones),
N = 136 (ragged 128-, 64- and 32-column tiles), K = 576 (9 or 18 K-steps: every ring wraps at least twice).  Its own data gradient
gathers 136 channels, which is off both K-step grids (the GENERIC variant; asserted as such), so the plain data gradient is taken
on the mirrored problem 136 -> 64 channels: the same M x N x K.

What is cut from the cross product, and why: the persistent kernel and the fused sums share the epilogue modes with nothing (they
exist for fp16 results without bias / accumulation only); the tap-skipping cases run at the default ring depth (skipping changes
which K-steps enter the ring, not the ring); the sliced-operand cases run one forced (K-step, depth) per tile and kernel (the row
stride enters the epilogue only).  The ring grid itself runs every epilogue mode on every (tile, K-step, depth): it is cheap."""
import contextlib
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import fill
from test_half_gpu import (BNSTAT_CASES_H, CONV_CASES, TOL32, assert_half_rounded, h, krsc, r8, rel, to_act_h)

pytestmark = pytest.mark.gpu

RING, PERSISTENT = 21, 22                               # PSEG_KERNEL_GATHER_H, PSEG_KERNEL_GATHER_H_PERSISTENT
TILES = [(128, 128), (128, 64), (64, 128), (128, 32)]   # kHTiles (conv_half_gather.hip)
WAVE_ROWS = {(128, 128): 2, (128, 64): 2, (64, 128): 2, (128, 32): 4}      # HTile::wm
KBS = [32, 64]
DEPTHS = [2, 3, 4]

# B, Cin, H, W, Cout, k, stride, pad, dil
CASE_A = (1, 64, 13, 13, 136, 3, 1, 1, 1)         # the ring-grid problem
CASE_AT = (1, 136, 13, 13, 64, 3, 1, 1, 1)        # ... mirrored: its data gradient is the same GEMM with a plain gather
CASE_A200 = (1, 64, 13, 13, 200, 3, 1, 1, 1)      # 2 x 7 = 14 tiles of 128x32
CASE_AT200 = (1, 200, 13, 13, 64, 3, 1, 1, 1)
CASE_1X1 = (1, 64, 13, 13, 136, 1, 1, 0, 1)       # one or two K-steps: fewer than any ring is deep
CASE_ONE = (1, 64, 8, 8, 32, 3, 1, 1, 1)          # a single tile on every tile shape
CASE_ONET = (1, 32, 8, 8, 64, 3, 1, 1, 1)
CASE_GEN = (1, 40, 13, 13, 136, 3, 1, 1, 1)       # 40 (and, in its data gradient, 136) channels: off both K-step grids
CASE_STEM = (1, 3, 30, 30, 20, 7, 2, 3, 1)        # the stem: 3 -> 8 padded input channels, 7x7 stride 2 (20 -> 24 output channels)
CASE_DIL = (2, 64, 24, 24, 64, 3, 1, 12, 12)      # CONV_CASES' rate-12 conv on a 24 x 24 map with 64 output channels (so that its
                                                  # data gradient stays on the K-step grid with either K-step): whole (tile, tap)
                                                  # pairs are padding
CASE_S2 = (2, 64, 32, 32, 64, 3, 2, 1, 1)         # stride-2 data gradient: parity-class row order


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    from pytorch_segmentation_amd import ops as _ops
    return _ops


@contextlib.contextmanager
def switches(monkeypatch, **env):
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


def force(tile=None, kb=None, depth=None, persist=None, noskip=None):
    env = {}
    if tile is not None:
        env['PSEG_CONV_BM'], env['PSEG_CONV_BN'] = tile
    if kb is not None:
        env['PSEG_HCONV_KB'] = kb
    if depth is not None:
        env['PSEG_HCONV_STAGES'] = depth
    if persist is not None:
        env['PSEG_HCONV_PERSIST'] = persist
    if noskip is not None:
        env['PSEG_CONV_NOSKIP'] = noskip
    return env


def ran():
    """(kernel id, (bm, bn, K-step, ring depth, variant, fused sums)) of this thread's last fp16 gather launch"""
    from pytorch_segmentation_amd import _lib
    lib = _lib.load()
    rec = (ctypes.c_int * 6)()
    assert lib.pseg_debug_last_gather_h(rec) == 0
    return lib.pseg_debug_last_conv_kernel(), tuple(rec)


def expect(kernel, tile, kb, depth, variant, bns=0):
    assert ran() == (kernel, (tile[0], tile[1], kb, depth, variant, bns)), \
        'meant to test %s on tile %dx%d, K-step %d, depth %d, variant %d, sums %d; ran %r' % (
            kernel, tile[0], tile[1], kb, depth, variant, bns, ran())


@functools.lru_cache(maxsize=None)
def reference(case):
    """half-rounded operands of a conv problem and its fp64 results, once per module: never written to afterwards"""
    B, Cin, H, W, Cout, k, stride, pad, dil = case
    key = 'hinst/' + '_'.join(map(str, case))
    x = h(fill.uniform(key + '/x', (B, Cin, H, W)))
    w = h(fill.uniform(key + '/w', (Cout, Cin, k, k), (6.0 / (Cin * k * k)) ** 0.5))
    b = fill.uniform(key + '/b', (Cout,), 0.5)
    xr, wr = x.double().requires_grad_(), w.double().requires_grad_()
    y = F.conv2d(xr, wr, None, stride, pad, dil)
    gy = h(fill.uniform(key + '/gy', tuple(y.shape)))
    y.backward(gy.double())
    return dict(x=x, w=w, b=b, gy=gy, y=y.detach(), dx=xr.grad, dw=wr.grad)


_DEVICE = {}


def operands(ops, case):
    """... and their device copies (fp16 NHWC activations, the filter and its transpose, the padded fp32 bias)"""
    if case not in _DEVICE:
        B, Cin, H, W, Cout, k, stride, pad, dil = case
        r = reference(case)
        cin_p, cout_p = r8(Cin), r8(Cout)
        w_h = krsc(r['w'], cout_p, cin_p).half().cuda()
        b_raw = torch.zeros(cout_p)
        b_raw[:Cout] = r['b']
        _DEVICE[case] = dict(xa=to_act_h(ops, r['x'], cin_p), gya=to_act_h(ops, r['gy'], cout_p), w_h=w_h,
                             wT_h=w_h.view(cout_p, k * k, cin_p).permute(2, 1, 0).contiguous(), b_raw=b_raw.cuda(),
                             Ho=r['y'].shape[2], Wo=r['y'].shape[3], cin_p=cin_p, cout_p=cout_p)
    return _DEVICE[case]


def conv_args(case):
    k, stride, pad, dil = case[5:]
    return k, k, stride, pad, dil


def check_stats(ops, stats, M, ref, Cout):
    """the finalised mean / invstd of fused statistics against those of `ref` (fp64 NCHW): test_conv2d_fwd_half's bounds"""
    co = ops.bn_finalize(stats, M, None, None, None, None, 0.0, 1e-5)
    mu, var = ref.mean((0, 2, 3)), ref.var((0, 2, 3), unbiased=False)
    assert rel(co[0][:Cout], mu) < 1e-4 * max(1.0, (var.sqrt().max() / (mu.abs().max() + 1e-30)).item())
    assert rel(co[1][:Cout], 1.0 / (var + 1e-5).sqrt()) < 1e-4
    return co


def fwd_half_stats(ops, case):
    """forward, fp16 result + fused statistics -> (y, finalised coefficients): the result against fp64, the statistics against
    the fp64 statistics of the result AS STORED (the kernels round to fp16 before they sum, so that the layer normalises the
    values it reads back; on a map of 64 pixels the statistics of the unrounded result are 1.1e-4 away)"""
    B, Cin, H, W, Cout = case[:5]
    r, d = reference(case), operands(ops, case)
    y = ops.Act.empty(B, d['Ho'], d['Wo'], d['cout_p'], 'cuda', dtype=torch.float16)
    stats = ops.conv2d_fwd(d['xa'], d['w_h'], None, y, *conv_args(case), want_stats=True)
    look = ran()
    stored = y.to_nchw(Cout).double().cpu()
    assert_half_rounded(stored, r['y'], 'fwd f16')
    co = check_stats(ops, stats, y.M, stored, Cout)
    return y, co, look


def dgrad_half(ops, case, accumulate_too=False):
    B, Cin, H, W, Cout = case[:5]
    r, d = reference(case), operands(ops, case)
    dx = ops.Act.empty(B, H, W, d['cin_p'], 'cuda', dtype=torch.float16)
    ops.conv2d_dgrad(d['gya'], d['wT_h'], dx, *conv_args(case))
    look = ran()
    assert_half_rounded(dx.to_nchw(Cin), r['dx'], 'dgrad')
    if accumulate_too:
        keep = dx.t.clone()
        before = dx.to_nchw(Cin).double().cpu()
        ops.conv2d_dgrad(d['gya'], d['wT_h'], dx, *conv_args(case), accumulate=True)
        assert ran() == look
        assert_half_rounded(dx.to_nchw(Cin), before + r['dx'], 'dgrad accumulate')
        dx = ops.Act(keep, dx.B, dx.H, dx.W, dx.C, dx.ld)
    return dx, look


def grid_ids(tiles=TILES, kbs=KBS, depths=DEPTHS):
    return [pytest.param(t, kb, st, id='%dx%d-kb%d-depth%d' % (t[0], t[1], kb, st)) for t in tiles for kb in kbs for st in depths]


# ------------------------------------------------------------------------------------------------------ a. the ring grid
@pytest.mark.parametrize('tile,kb,depth', grid_ids())
def test_ring_grid_plain(ops, tile, kb, depth, monkeypatch):
    """gather_h_kernel<tile, plain, K-step, depth>: every epilogue mode of the forward, the data gradient, and a contraction
    shorter than the ring (the depth is clamped to the K loop's length, two at the least)."""
    B, Cin, H, W, Cout = CASE_A[:5]
    r, d = reference(CASE_A), operands(ops, CASE_A)
    with switches(monkeypatch, **force(tile, kb, depth, persist=0)):
        want = (RING, tile + (kb, depth, 0, 0))
        # fp16 result with the fused statistics
        y16, _, look = fwd_half_stats(ops, CASE_A)
        assert look == want, (look, want)
        # fp32 result with bias
        y32 = ops.Act.empty(B, d['Ho'], d['Wo'], d['cout_p'], 'cuda')
        assert ops.conv2d_fwd(d['xa'], d['w_h'], d['b_raw'], y32, *conv_args(CASE_A)) is None
        expect(RING, tile, kb, depth, 0)
        assert rel(y32.to_nchw(Cout), r['y'] + r['b'].double().view(1, -1, 1, 1)) < TOL32
        # accumulate onto a non-zero fp16 result: y = half(float(y) + conv)
        before = y16.to_nchw(Cout).double().cpu()
        ops.conv2d_fwd(d['xa'], d['w_h'], None, y16, *conv_args(CASE_A), accumulate=True)
        expect(RING, tile, kb, depth, 0)
        assert_half_rounded(y16.to_nchw(Cout), before + r['y'], 'fwd accumulate')
        # data gradient of the mirrored problem (plain gather), overwriting and accumulating
        _, look = dgrad_half(ops, CASE_AT, accumulate_too=True)
        assert look == want, (look, want)
        # ... and of the problem itself: 136 gathered channels are off the K-step grid -> the GENERIC instantiation
        _, look = dgrad_half(ops, CASE_A)
        assert look == (RING, tile + (kb, depth, 2, 0)), look
        # 1x1 on 64 channels: two K-steps of 32 or one of 64 -> a ring two deep whatever was asked for
        _, _, look = fwd_half_stats(ops, CASE_1X1)
        assert look == (RING, tile + (kb, 2, 0, 0)), look


# ------------------------------------------------------------------------------------------------------ b. GENERIC
@pytest.mark.parametrize('kb', [None, 64], ids=['kb-by-rule', 'kb64'])
@pytest.mark.parametrize('tile,depth', [pytest.param(t, st, id='%dx%d-depth%d' % (t[0], t[1], st)) for t in TILES for st in DEPTHS])
def test_ring_grid_generic(ops, tile, depth, kb, monkeypatch):
    """gather_h_kernel<tile, GENERIC, K-step, depth> on 40 input channels: K-steps that straddle taps, per-lane (tap, channel)
    addressing.  Unforced, the K-step is 32 (Cin % 64 != 0)."""
    with switches(monkeypatch, **force(tile, kb, depth, persist=0)):
        want = (RING, tile + (kb or 32, depth, 2, 0))
        _, _, look = fwd_half_stats(ops, CASE_GEN)
        assert look == want, (look, want)
        _, look = dgrad_half(ops, CASE_GEN, accumulate_too=True)
        assert look == want, (look, want)


@pytest.mark.parametrize('tile', [None] + TILES, ids=['default'] + ['%dx%d' % t for t in TILES])
def test_generic_stem(ops, tile, monkeypatch):
    """the stem (3 -> 8 padded input channels, 7x7, stride 2; 20 -> 24 output channels): the padded input channels contribute
    exact zeros, the padded output channels and the padded channels of dx receive exact zeros"""
    B, Cin, H, W, Cout = CASE_STEM[:5]
    r, d = reference(CASE_STEM), operands(ops, CASE_STEM)
    assert d['cin_p'] == 8 and d['cout_p'] == 24
    with switches(monkeypatch, **force(tile, persist=0)):
        y32 = ops.Act.empty(B, d['Ho'], d['Wo'], d['cout_p'], 'cuda')
        stats = ops.conv2d_fwd(d['xa'], d['w_h'], None, y32, *conv_args(CASE_STEM), want_stats=True)
        kernel, rec = ran()
        assert kernel == RING and rec[4] == 2 and rec[2] == 32 and (tile is None or rec[:2] == tile), rec
        assert rel(y32.to_nchw(Cout), r['y']) < TOL32
        assert y32.view4()[..., Cout:].abs().max().item() == 0.0
        check_stats(ops, stats, y32.M, r['y'], Cout)
        y16, _, _ = fwd_half_stats(ops, CASE_STEM)
        assert y16.view4()[..., Cout:].abs().max().item() == 0.0
        dx, (kernel, rec) = dgrad_half(ops, CASE_STEM)         # (gathers 24 channels: GENERIC as well)
        assert kernel == RING and rec[4] == 2 and (tile is None or rec[:2] == tile), rec
        assert dx.view4()[..., Cin:].abs().max().item() == 0.0


# ------------------------------------------------------------------------------------------------------ c. tap skipping
def _skip_pair(ops, monkeypatch, tile, kb, run):
    """run() under the tap-skipping selection and under PSEG_CONV_NOSKIP=1 on the same (tile, K-step) -> both results"""
    out = []
    for noskip in (None, 1):
        with switches(monkeypatch, **force(tile, kb, persist=0, noskip=noskip)):
            out.append(run())
    return out


@pytest.mark.parametrize('kb', KBS, ids=['kb32', 'kb64'])
@pytest.mark.parametrize('tile', TILES, ids=['%dx%d' % t for t in TILES])
def test_tap_skipping_dilated(ops, tile, kb, monkeypatch):
    """rate-12 3x3 on a 24 x 24 map: gather_h_kernel<tile, tap-skipping> on the three 4-wave tiles -- never on 128x128, which runs
    the plain instantiation (select_gather_h: dense is faster there).  A skipped tap contributes exact zeros and the live K-steps
    keep their order, so the skipping and the dense (PSEG_CONV_NOSKIP=1) result of one instantiation are BIT-identical."""
    variant = 0 if tile == (128, 128) else 1
    depth = 3 if kb == 32 else 2        # K = 576: select_gather_h's own depth for either K-step

    def run():
        y, co, look_f = fwd_half_stats(ops, CASE_DIL)
        dx, look_d = dgrad_half(ops, CASE_DIL)
        return y.t, dx.t, co, look_f, look_d

    skip, dense = _skip_pair(ops, monkeypatch, tile, kb, run)
    assert skip[3] == skip[4] == (RING, tile + (kb, depth, variant, 0)), skip[3:]
    assert dense[3] == dense[4] == (RING, tile + (kb, depth, 0, 0)), dense[3:]
    assert torch.equal(skip[0], dense[0]) and torch.equal(skip[1], dense[1])
    assert rel(skip[2][0], dense[2][0]) < 1e-5 and rel(skip[2][1], dense[2][1]) < 1e-5


@pytest.mark.parametrize('kb', KBS, ids=['kb32', 'kb64'])
@pytest.mark.parametrize('tile', TILES, ids=['%dx%d' % t for t in TILES])
def test_tap_skipping_stride2_dgrad(ops, tile, kb, monkeypatch):
    """the stride-2 data gradient: parity-homogeneous tiles, three taps in four skipped -- on EVERY tile shape, 128x128 included
    (gather_row_order's parity order is granted to every fp16 tile; only the dilated skip is kept off the 8-wave tile).  The
    class-sorted row order moves rows between tiles, not K-steps within a row: each element still sums its live K-steps in
    ascending order, so the dense row-major result (PSEG_CONV_NOSKIP=1) is bit-identical."""
    depth = 3 if kb == 32 else 2        # K = 576
    skip, dense = _skip_pair(ops, monkeypatch, tile, kb, lambda: dgrad_half(ops, CASE_S2, accumulate_too=True))
    assert skip[1] == (RING, tile + (kb, depth, 1, 0)), skip[1]
    assert dense[1] == (RING, tile + (kb, depth, 0, 0)), dense[1]
    assert torch.equal(skip[0].t, dense[0].t)


# ------------------------------------------------------------------------------------------------------ d. persistent kernel
_RING_RESULT = {}


def _fwd_dgrad(ops, fcase, dcase):
    y, co, look_f = fwd_half_stats(ops, fcase)
    dx, look_d = dgrad_half(ops, dcase)
    return y.t, dx.t, co, look_f, look_d


def _ring_result(ops, monkeypatch, fcase, dcase, tile, kb):
    """gather_h_kernel on (tile, K-step) at its default depth, once per module (the ring grid checks every depth against fp64)"""
    key = (fcase, dcase, tile, kb)
    if key not in _RING_RESULT:
        with switches(monkeypatch, **force(tile, kb, persist=0)):
            _RING_RESULT[key] = _fwd_dgrad(ops, fcase, dcase)
        assert _RING_RESULT[key][3][0] == _RING_RESULT[key][4][0] == RING
    return _RING_RESULT[key]


def _persistent_against_ring(ops, monkeypatch, fcase, dcase, tile, kb, depth):
    ring = _ring_result(ops, monkeypatch, fcase, dcase, tile, kb)
    with switches(monkeypatch, **force(tile, kb, depth, persist=2)):
        got = _fwd_dgrad(ops, fcase, dcase)
    want = (PERSISTENT, tile + (kb, min(depth, 3), 0, 0))       # (its ring is two or three deep: pstages)
    assert got[3] == got[4] == want, (got[3:], want)
    # same K-step order, same fp32 accumulation, one rounding: bit-identical; statistics: the same values, summed per wave row
    assert torch.equal(got[0], ring[0]) and torch.equal(got[1], ring[1])
    assert rel(got[2][0], ring[2][0]) < 1e-5 and rel(got[2][1], ring[2][1]) < 1e-5


@pytest.mark.parametrize('tile,kb,depth', grid_ids())
def test_persistent_grid(ops, tile, kb, depth, monkeypatch):
    """gather_hp_kernel<tile, K-step, depth 2 | 3> (PSEG_HCONV_PERSIST=2; a request for depth 4 runs depth 3) on the ring-grid
    problem (4 / 6 / 6 / 10 ragged tiles), forward with statistics and data gradient: against fp64, and bit-identical to
    gather_h_kernel on the same (tile, K-step)."""
    _persistent_against_ring(ops, monkeypatch, CASE_A, CASE_AT, tile, kb, depth)


@pytest.mark.parametrize('tile,kb,depth', grid_ids(depths=[2, 3]))
def test_persistent_single_tile(ops, tile, kb, depth, monkeypatch):
    """one tile: the persistent loop's first tile is its last (no next-tile prefetch at all)"""
    _persistent_against_ring(ops, monkeypatch, CASE_ONE, CASE_ONET, tile, kb, depth)


@pytest.mark.parametrize('tile,kb,depth', grid_ids(tiles=[(128, 32)], depths=[2, 3]))
def test_persistent_fourteen_narrow_tiles(ops, tile, kb, depth, monkeypatch):
    """200 output channels on 128x32: 2 x 7 = 14 tiles, the last column tile 8 channels wide"""
    _persistent_against_ring(ops, monkeypatch, CASE_A200, CASE_AT200, tile, kb, depth)


@pytest.mark.parametrize('tile', TILES, ids=['%dx%d' % t for t in TILES])
def test_persistent_not_offered(ops, tile, monkeypatch):
    """with a bias, an fp32 result or accumulation the persistent kernel is not offered, even when forced: gather_h_kernel runs"""
    B, Cin, H, W, Cout = CASE_A[:5]
    r, d = reference(CASE_A), operands(ops, CASE_A)
    with switches(monkeypatch, **force(tile, persist=2)):
        y16 = ops.Act.empty(B, d['Ho'], d['Wo'], d['cout_p'], 'cuda', dtype=torch.float16)
        ops.conv2d_fwd(d['xa'], d['w_h'], None, y16, *conv_args(CASE_A))
        assert ran()[0] == PERSISTENT
        ops.conv2d_fwd(d['xa'], d['w_h'], d['b_raw'], y16, *conv_args(CASE_A))
        assert ran()[0] == RING
        assert_half_rounded(y16.to_nchw(Cout), r['y'] + r['b'].double().view(1, -1, 1, 1), 'fwd bias')
        y32 = ops.Act.empty(B, d['Ho'], d['Wo'], d['cout_p'], 'cuda')
        ops.conv2d_fwd(d['xa'], d['w_h'], None, y32, *conv_args(CASE_A))
        assert ran()[0] == RING
        assert rel(y32.to_nchw(Cout), r['y']) < TOL32
        before = y16.to_nchw(Cout).double().cpu()
        ops.conv2d_fwd(d['xa'], d['w_h'], None, y16, *conv_args(CASE_A), accumulate=True)
        assert ran()[0] == RING
        assert_half_rounded(y16.to_nchw(Cout), before + r['y'], 'fwd accumulate')
        dx, look = dgrad_half(ops, CASE_AT)
        assert look[0] == PERSISTENT
        dT = operands(ops, CASE_AT)
        before = dx.to_nchw().double().cpu()
        ops.conv2d_dgrad(dT['gya'], dT['wT_h'], dx, *conv_args(CASE_AT), accumulate=True)
        assert ran()[0] == RING
        assert_half_rounded(dx.to_nchw(), before + reference(CASE_AT)['dx'], 'dgrad accumulate')


# ------------------------------------------------------------------------------------------------------ e. fused sums
# The instantiations with BNS = true, restated from the two predicates of conv_half_gather.hip: HTile::bns_kb (the K-steps a
# tile carries the sums with: 128x128 and 128x64 both, 64x128 none, 128x32 the short one) and h_bns_steps (ring: 32/3, 64/2,
# 64/3; persistent: 32/3, 64/2).
BNS_KB = {(128, 128): (32, 64), (128, 64): (32, 64), (64, 128): (), (128, 32): (32,)}
BNS_STEPS = {RING: [(32, 3), (64, 2), (64, 3)], PERSISTENT: [(32, 3), (64, 2)]}
BNS_TABLE = [(t, kb, st, kern) for t in TILES for kern in (RING, PERSISTENT) for kb, st in BNS_STEPS[kern] if kb in BNS_KB[t]]
# forced combinations outside the table: -> None where no kernel carries the sums (rows == 0, the entry point refuses), or the
# instantiation inside the table the selection falls to (a ring depth the persistent kernel does not have: its depth-3 / the
# ring's instantiation takes the problem)
BNS_OUTSIDE = [
    ((64, 128), 32, 3, 0, None), ((64, 128), 64, 2, 2, None), ((128, 32), 64, 2, 0, None), ((128, 64), 32, 2, 0, None),
    ((128, 64), 32, 4, 0, None), ((128, 128), 64, 4, 2, None), ((128, 128), 32, 2, 2, None),
    ((128, 64), 64, 3, 2, (RING, 64, 3)), ((128, 64), 32, 4, 2, (PERSISTENT, 32, 3)), ((128, 32), 32, 4, 2, (PERSISTENT, 32, 3)),
]
CASE_BNS = (1, 136, 13, 13, 64, 3, 1, 1, 1)       # B, C (the BatchNorm layer = dx), H, W, C2 (dy), k, ...: the mirrored problem
BNS_ACT = 1


def _bns_setup(ops):
    """the BatchNorm layer in front of CASE_BNS' conv: its saved y, finalised coefficients and the fp64 sums' ingredients"""
    if 'bns' not in _DEVICE:
        B, C, H, W = CASE_BNS[:4]
        key = 'hinst/bns'
        y = h(fill.uniform(key + '/y', (B, C, H, W), 2.0) + fill.uniform(key + '/off', (1, C, 1, 1), 1.0))
        g, b = 1.0 + fill.uniform(key + '/g', (C,), 0.3), fill.uniform(key + '/b', (C,), 0.3)
        ya = to_act_h(ops, y, C)
        co = ops.bn_finalize(ops.col_stats(ya), ya.M, g.cuda(), b.cuda(), torch.zeros(C).cuda(), torch.ones(C).cuda(), 0.1, 1e-5)
        pre = (y.cuda() - co[0].view(1, C, 1, 1)) * co[2].view(1, C, 1, 1) + co[3].view(1, C, 1, 1)      # fp32, as the kernels decide
        mu, istd = (co[i].double().cpu().view(1, C, 1, 1) for i in range(2))
        _DEVICE['bns'] = dict(ya=ya, co=co, on=(pre > 0).cpu().double(), xh=(y.double() - mu) * istd)
    return _DEVICE['bns']


def _bns_rows(ops):
    B, C, H, W, C2, k, stride, pad, dil = CASE_BNS
    return ops._lib.query('pseg_conv2d_dgrad_bnstat_rows_h', B, H, W, C, H, W, C2, k, k, stride, pad, dil)


def _bns_check(ops, kernel, tile, kb, depth):
    B, C, H, W = CASE_BNS[:4]
    r, d, s = reference(CASE_BNS), operands(ops, CASE_BNS), _bns_setup(ops)
    rows = _bns_rows(ops)
    assert rows == -(-B * H * W // tile[0]) * WAVE_ROWS[tile]           # row tiles x wave rows (HGatherChoice::stat_rows)
    dx = ops.Act.empty(B, H, W, C, 'cuda', dtype=torch.float16)
    ops.conv2d_dgrad(d['gya'], d['wT_h'], dx, *conv_args(CASE_BNS), bn=(s['ya'], s['co'], BNS_ACT))
    expect(kernel, tile, kb, depth, 0, bns=1)
    assert dx.bnpart is not None and dx.bnpart.rows == rows
    assert_half_rounded(dx.to_nchw(C), r['dx'], 'dgrad with sums')
    gm = dx.to_nchw(C).double().cpu() * s['on']                         # the sums are taken over dx AS STORED
    db_ref, dg_ref = gm.sum((0, 2, 3)), (gm * s['xh']).sum((0, 2, 3))
    part = dx.bnpart.part.double().cpu()
    assert (part[0].sum(0) - db_ref).abs().max().item() < 1e-5 * (gm.abs().sum((0, 2, 3)).max().item() + 1e-30)
    assert (part[1].sum(0) - dg_ref).abs().max().item() < 1e-5 * ((gm * s['xh']).abs().sum((0, 2, 3)).max().item() + 1e-30)
    return dx


@pytest.mark.parametrize('tile,kb,depth,kernel', BNS_TABLE,
                         ids=['%dx%d-kb%d-depth%d-%s' % (t[0], t[1], kb, st, 'ring' if kern == RING else 'persistent')
                              for t, kb, st, kern in BNS_TABLE])
def test_fused_sums_instances(ops, tile, kb, depth, kernel, monkeypatch):
    """every BNS = true instantiation: dx within one rounding of fp64 (and bit-identical to the plain data gradient of the same
    instantiation), the partial sums equal to the fp64 sums over dx as stored"""
    monkeypatch.setattr(ops, 'FUSE_BN_BWD_H', True)
    with switches(monkeypatch, **force(tile, kb, depth, persist=2 if kernel == PERSISTENT else 0)):
        dx = _bns_check(ops, kernel, tile, kb, depth)
        plain, look = dgrad_half(ops, CASE_BNS)
        assert look == (kernel, tile + (kb, depth, 0, 0)), look
        assert plain.bnpart is None and torch.equal(plain.t, dx.t)


@pytest.mark.parametrize('tile,kb,depth,persist,falls_to', BNS_OUTSIDE,
                         ids=['%dx%d-kb%d-depth%d-persist%d' % (t[0], t[1], kb, st, p) for t, kb, st, p, _ in BNS_OUTSIDE])
def test_fused_sums_outside_the_table(ops, tile, kb, depth, persist, falls_to, monkeypatch):
    """a forced combination without a BNS instantiation never launches without the sums: either another kernel of the table takes
    the problem, or the rows query is 0, ops.conv2d_dgrad runs the plain data gradient and the entry point itself refuses"""
    monkeypatch.setattr(ops, 'FUSE_BN_BWD_H', True)
    B, C, H, W, C2, k, stride, pad, dil = CASE_BNS
    r, d, s = reference(CASE_BNS), operands(ops, CASE_BNS), _bns_setup(ops)
    with switches(monkeypatch, **force(tile, kb, depth, persist=persist)):
        if falls_to is not None:
            _bns_check(ops, falls_to[0], tile, falls_to[1], falls_to[2])
            return
        assert _bns_rows(ops) == 0
        dx = ops.Act.empty(B, H, W, C, 'cuda', dtype=torch.float16)
        ops.conv2d_dgrad(d['gya'], d['wT_h'], dx, *conv_args(CASE_BNS), bn=(s['ya'], s['co'], BNS_ACT))
        assert dx.bnpart is None and ran()[1][5] == 0
        assert_half_rounded(dx.to_nchw(C), r['dx'], 'dgrad')
        part = torch.empty(2, 8, C, device='cuda')
        co = s['co']
        with pytest.raises(ops._lib.PsegError):
            ops._lib.call('pseg_conv2d_dgrad_bnstat_h', d['gya'].ptr, d['gya'].ld, d['wT_h'].data_ptr(), dx.ptr, dx.ld, B, H, W, C, H, W,
                          C2, k, k, stride, pad, dil, s['ya'].ptr, s['ya'].ld, co[0].data_ptr(), co[1].data_ptr(), co[2].data_ptr(),
                          co[3].data_ptr(), BNS_ACT, part.data_ptr(), part[1].data_ptr(), 8, 0)


# ------------------------------------------------------------------------------------------------------ f. sliced operands
PATTERN = {torch.float16: (torch.int16, 0x5A5A), torch.float32: (torch.int32, 0x5A5A5A5A)}     # (finite in either format)


def wide_buffer(ops, like, ld, c0, dtype=None, content=None):
    """a [M][ld] buffer filled with a bit pattern, and the `like.C`-channel slice at column c0 of it (holding `content`)"""
    dtype = like.dtype if dtype is None else dtype
    wide = ops.Act.empty(like.B, like.H, like.W, ld, 'cuda', dtype=dtype)
    ity, word = PATTERN[dtype]
    wide.t.view(ity).fill_(word)
    part = wide.slice(c0, c0 + like.C)
    if content is not None:
        ops.copy2d(content, part)
    return wide, part


def assert_outside_untouched(wide, c0, c1):
    """the concat contract: the columns of the wide buffer beside the slice still hold the pattern"""
    ity, word = PATTERN[wide.dtype]
    bits = wide.t.view(ity).view(wide.M, wide.ld)
    assert bool((bits[:, :c0] == word).all()) and bool((bits[:, c1:] == word).all()), 'wrote outside its channel slice'


SLICE_CASES = [pytest.param(None, None, None, RING, id='default-ring'), pytest.param(None, None, None, PERSISTENT, id='default-persistent')]
for _t, _kb, _st in [((128, 128), 64, 2), ((128, 64), 32, 3), ((64, 128), 64, 3), ((128, 32), 32, 2)]:
    for _k in (RING, PERSISTENT):
        SLICE_CASES.append(pytest.param(_t, _kb, _st, _k, id='%dx%d-kb%d-depth%d-%s' % (_t[0], _t[1], _kb, _st, 'ring' if _k == RING else 'persistent')))


@pytest.mark.parametrize('pad_cols,c0', [(24, 16), (8, 8)], ids=['ld+24', 'ld+8'])
@pytest.mark.parametrize('tile,kb,depth,kernel', SLICE_CASES)
def test_sliced_operands(ops, tile, kb, depth, kernel, pad_cols, c0, monkeypatch):
    """results written into channel slices of wider buffers (ldy > N: the ASPP / UNet / HRNet joins) and operands read out of them
    (ldx > Cin: their backward passes), through both epilogues: the ring kernel's 32-row patch and the persistent kernel's
    transposed patch.  Row strides N + 24 and N + 8, the slice 16 bytes or more into the row."""
    B, Cin, H, W, Cout = CASE_A[:5]
    r, d = reference(CASE_A), operands(ops, CASE_A)
    rT, dT = reference(CASE_AT), operands(ops, CASE_AT)
    with switches(monkeypatch, **force(tile, kb, depth, persist=2 if kernel == PERSISTENT else 0)):
        def check_ran(k=kernel):
            kern, rec = ran()
            assert kern == k and rec[4] == 0 and (tile is None or rec[:4] == tile + (kb, depth)), (kern, rec)
            assert rec[:2] in TILES

        dense = ops.Act.empty(B, d['Ho'], d['Wo'], Cout, 'cuda', dtype=torch.float16)
        # forward into a slice, fp16, with the fused statistics: those of the slice's values
        wide, part = wide_buffer(ops, dense, Cout + pad_cols, c0)
        stats = ops.conv2d_fwd(d['xa'], d['w_h'], None, part, *conv_args(CASE_A), want_stats=True)
        check_ran()
        assert_half_rounded(part.to_nchw(), r['y'], 'fwd into a slice')
        assert_outside_untouched(wide, c0, c0 + Cout)
        check_stats(ops, stats, part.M, part.to_nchw().double().cpu(), Cout)
        # forward out of a slice of a wider input (and into a slice)
        xwide, xpart = wide_buffer(ops, d['xa'], Cin + pad_cols, c0, content=d['xa'])
        wide2, part2 = wide_buffer(ops, dense, Cout + pad_cols, c0)
        ops.conv2d_fwd(xpart, d['w_h'], None, part2, *conv_args(CASE_A))
        check_ran()
        assert torch.equal(wide2.t, wide.t)
        # data gradient: dy out of a slice, dx into a slice
        gwide, gpart = wide_buffer(ops, dT['gya'], dT['gya'].C + pad_cols, c0, content=dT['gya'])
        dxd = ops.Act.empty(B, H, W, dT['cin_p'], 'cuda', dtype=torch.float16)
        dwide, dpart = wide_buffer(ops, dxd, dxd.C + pad_cols, c0)
        ops.conv2d_dgrad(gpart, dT['wT_h'], dpart, *conv_args(CASE_AT))
        check_ran()
        assert_half_rounded(dpart.to_nchw(), rT['dx'], 'dgrad between slices')
        assert_outside_untouched(dwide, c0, c0 + dxd.C)
        assert_outside_untouched(gwide, c0, c0 + gpart.C)
        assert_outside_untouched(xwide, c0, c0 + Cin)
        if kernel == PERSISTENT:
            return          # (the epilogue modes below are gather_h_kernel's alone)
        # accumulate onto the slice: y = half(float(y) + conv)
        before = part.to_nchw().double().cpu()
        ops.conv2d_fwd(d['xa'], d['w_h'], None, part, *conv_args(CASE_A), accumulate=True)
        check_ran()
        assert_half_rounded(part.to_nchw(), before + r['y'], 'fwd accumulate into a slice')
        assert_outside_untouched(wide, c0, c0 + Cout)
        dbefore = dpart.to_nchw().double().cpu()
        ops.conv2d_dgrad(gpart, dT['wT_h'], dpart, *conv_args(CASE_AT), accumulate=True)
        check_ran()
        assert_half_rounded(dpart.to_nchw(), dbefore + rT['dx'], 'dgrad accumulate between slices')
        assert_outside_untouched(dwide, c0, c0 + dxd.C)
        # fp32 wide buffer with bias
        wide32, part32 = wide_buffer(ops, dense, Cout + pad_cols, c0, dtype=torch.float32)
        ops.conv2d_fwd(xpart, d['w_h'], d['b_raw'], part32, *conv_args(CASE_A))
        check_ran()
        assert rel(part32.to_nchw(), r['y'] + r['b'].double().view(1, -1, 1, 1)) < TOL32
        assert_outside_untouched(wide32, c0, c0 + Cout)


@pytest.mark.parametrize('bkp', [32, 64])
def test_sliced_operands_wgrad(ops, bkp, monkeypatch):
    """pseg_conv2d_wgrad_h with x and dy both read out of channel slices, one launch family per K-step pixel count"""
    B, Cin, H, W, Cout = CASE_A[:5]
    r, d = reference(CASE_A), operands(ops, CASE_A)
    with switches(monkeypatch, PSEG_HWGRAD_BKP=bkp):
        xwide, xpart = wide_buffer(ops, d['xa'], Cin + 24, 16, content=d['xa'])
        gwide, gpart = wide_buffer(ops, d['gya'], Cout + 8, 8, content=d['gya'])
        dw = torch.empty(Cout, 3, 3, Cin, device='cuda')
        ops.conv2d_wgrad(xpart, gpart, dw, *conv_args(CASE_A))
        assert rel(dw.permute(0, 3, 1, 2), r['dw']) < TOL32
        ops.conv2d_wgrad(xpart, gpart, dw, *conv_args(CASE_A), accumulate=True)
        assert rel(dw.permute(0, 3, 1, 2), 2 * r['dw']) < TOL32
        dense = torch.empty_like(dw)
        ops.conv2d_wgrad(d['xa'], d['gya'], dense, *conv_args(CASE_A))
        ops.conv2d_wgrad(xpart, gpart, dw, *conv_args(CASE_A))
        assert torch.equal(dw, dense)
        assert_outside_untouched(xwide, 16, 16 + Cin)
        assert_outside_untouched(gwide, 8, 8 + Cout)


# ------------------------------------------------------------------------------------------------------ 3. the default plan
def _default_rule(kernel, tile, Cg, K):
    """(K-step, ring depth) as the comments of hconv_kb / select_gather_h state the heuristic, for Cg gathered channels and a
    contraction of K: 32 / 3 off the 64-channel grid or with K <= 576, else 64 / 2 -- 64 / 4 on 128x32 and 64 / 3 on 128x64 with
    K >= 2048; never deeper than the K loop is long (two at the least); the persistent kernel runs its ring 2 or 3 deep"""
    kb = 32 if (Cg % 64 != 0 or K <= 576) else 64
    depth = 3 if kb == 32 else (4 if tile[1] == 32 and K >= 2048 else (3 if tile == (128, 64) and K >= 2048 else 2))
    steps = -(-K // kb)
    if steps < depth:
        depth = max(2, steps)
    return kb, (min(depth, 3) if kernel == PERSISTENT else depth)


def test_default_plan_reaches_every_small_tile(ops):
    """Which instantiations the DEFAULT selection gives the small cases of test_half_gpu.py (CONV_CASES, BNSTAT_CASES_H; forward
    and data gradient): every tile of kHTiles but 128x128 must be reached by one of them, and every (K-step, depth) must be the
    heuristic's.  A planner change that moves the small cases off a tile fails here, with the table below in the output."""
    from pytorch_segmentation_amd import _lib
    _lib.clear_query_cache()
    table, reached, pairs = [], set(), set()
    for case in CONV_CASES + sorted(set(c[:9] for c in BNSTAT_CASES_H)):
        B, Cin, H, W, Cout, k, stride, pad, dil = case
        cin_p, cout_p = r8(Cin), r8(Cout)
        Ho, Wo = ops.conv_out_size(H, k, stride, pad, dil), ops.conv_out_size(W, k, stride, pad, dil)
        x = ops.Act.empty(B, H, W, cin_p, 'cuda', zero=True, dtype=torch.float16)
        y = ops.Act.empty(B, Ho, Wo, cout_p, 'cuda', zero=True, dtype=torch.float16)
        w = torch.zeros(cout_p * k * k * cin_p, dtype=torch.float16, device='cuda')
        for what, Cg in (('fwd', cin_p), ('dgrad', cout_p)):
            if what == 'fwd':
                ops.conv2d_fwd(x, w, None, y, k, k, stride, pad, dil)
            else:
                ops.conv2d_dgrad(y, w, x, k, k, stride, pad, dil)
            kernel, (bm, bn, kb, depth, variant, bns) = ran()
            table.append((case, what, kernel, bm, bn, kb, depth, variant))
            assert kernel in (RING, PERSISTENT) and (bm, bn) in TILES and bns == 0, table[-1]
            assert (kb, depth) == _default_rule(kernel, (bm, bn), Cg, k * k * Cg), (table[-1], _default_rule(kernel, (bm, bn), Cg, k * k * Cg))
            reached.add((bm, bn))
            pairs.add((kb, depth) + ((bm, bn) if (kb, depth) in ((64, 3), (64, 4)) and kernel == RING else ()))
    torch.cuda.synchronize()
    print('\ncase, pass, kernel, tile, K-step, depth, variant')
    for row in table:
        print('%-36s %-5s %d  %3dx%-3d  %2d  %d  %d' % ((str(row[0]), row[1], row[2]) + row[3:]))
    missing = [t for t in TILES if t != (128, 128) and t not in reached]
    assert not missing, 'no small default case runs on tile(s) %r any more: they are tested only where forced' % missing
    # the pairs the heuristic's comments describe, each reached by some small case: 32/3, 64/2, the deeper rings of the narrow
    # tiles on deep contractions (a gather_h_kernel launch: the persistent kernel stops at 3), the short-K clamp
    for pair in ((32, 3), (64, 2), (32, 2), (64, 3, 128, 64), (64, 4, 128, 32)):
        assert pair in pairs, ('the default plan no longer reaches', pair, sorted(pairs))
    assert pairs <= {(32, 3), (64, 2), (32, 2), (64, 3), (64, 3, 128, 64), (64, 4, 128, 32)}, sorted(pairs)
