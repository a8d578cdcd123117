"""Every compiled instance and every host branch of the BatchNorm / activation launches (csrc/norm_act.hip), one row of
tests/norm_cases.py at a time: the row's entry points are called directly through the C ABI, pseg_debug_last_norm must answer the
record the row names (kernel, storage type, lane width, mode, block and grid shape), and every output is compared element by
element with fp64 (tests/test_norm_instances_cpu.py shows without a GPU that the rows reach every instance).

Tolerances, derived (u = 2^-24, the unit roundoff of fp32):
  element-wise passes  the header's formula in fp64 with the kernel's own fp32 coefficient vectors, so that only the pass's rounding
                       is left: fp32 outputs |out - ref| <= 4 u A, A the formula with every term replaced by its absolute value;
                       fp16 outputs the fp64 value rounded once (test_half_gpu.assert_half_rounded)
  sums                 per channel |sum - ref| <= n u sum|term|, n = R, the rows of a statistics group (the terms that pass through
                       fp32; sums across groups are taken in double)
  coefficients         pseg_bn_finalize against Chan's merge in fp64 of the same fp32 partials: mean to 4 u (|mean| + std), invstd to
                       4 u relative, the running statistics alike
  masks                z-fed and mask-fed modes read their mask from an input, exactly; a mask recomputed from y (MODE 3) is left out
                       of the comparison within a margin of a kink (fp32: 1e-5 of the peak; fp16: that at 0 and 2^-8, one fp16 ulp, at
                       6), at most 0.5 % of a row, and there the output must be one of the two values the mask allows
  mode equivalence     partials, dgamma, dbeta, dy and dres bit-identical between the mask-fed and the z-fed mode (both storage types)
                       and between MODE 3 and the z-fed mode without a residual in fp32.  Not asserted for fp16: the stored z is
                       rounded, so an fp32 pre-activation just under 6 is stored as 6 and the two masks part there by design; each
                       mode is still held to fp64 on its own
Operands outside a row's channel slices hold NaN: a read from there reaches a result, and the raw bits must be unchanged after."""
import ctypes
import functools

import pytest
import torch

import norm_cases as nc
from oracle import fill
from test_half_gpu import assert_half_rounded

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
NAN = float('nan')
EPS, MOMENTUM = 1e-5, 0.1
EPS32 = float(torch.tensor(EPS, dtype=torch.float32))            # as the library sees them: float arguments
MOM32 = float(torch.tensor(MOMENTUM, dtype=torch.float32))
MAX_LEFT_OUT = 5e-3


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    from pytorch_segmentation_amd import ops as _ops
    return _ops


def call(name, *args):
    from pytorch_segmentation_amd import _lib
    _lib.call(name, *args, torch.cuda.current_stream().cuda_stream)


def ran():
    from pytorch_segmentation_amd import _lib
    rec = (ctypes.c_int * 12)()
    assert _lib.load().pseg_debug_last_norm(rec) == 0
    return tuple(rec)


def expect(row, record):
    got = ran()
    assert got == record, 'meant to test %s:\n  %s\nran\n  %s' % (row.id, nc.describe(record), nc.describe(got))


def sfx(row, name):
    return name + '_h' if row.dtype == 'h' else name


def tdt(row):
    return torch.float16 if row.dtype == 'h' else torch.float32


def ptr(t):
    return 0 if t is None else t.data_ptr()


def dev(t):
    return t.cuda()


def vec(key, C, centre=0.0, scale=1.0, fillv=None):
    """a per-channel fp32 vector on the device"""
    if fillv is not None:
        return torch.full((C,), fillv, dtype=torch.float32, device='cuda')
    return dev(centre + fill.uniform(key, (C,), scale))


class Op:
    """an [M][C] operand: channels [c0, c0 + C) of an [M][ld] device buffer.  Everything else in the buffer -- and the slice itself
    when the operand is a pure output -- holds NaN."""

    def __init__(self, row, name, values=None):
        q = 8 if row.dtype == 'h' else 4
        self.M, self.C = row.M, row.C
        self.ld, self.c0 = row.ld[name] if row.ld and name in row.ld else (nc.cdiv(row.C, q) * q, 0)
        self.buf = torch.full((row.M, self.ld), NAN, dtype=tdt(row), device='cuda')
        if values is not None:
            self.buf[:, self.c0:self.c0 + self.C] = values.to('cuda', tdt(row))
        self.before = self.buf.clone() if self.ld > self.C else None
        self.name = name

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.c0 * self.buf.element_size()

    @property
    def pl(self):
        return self.ptr, self.ld

    def get(self):
        return self.buf[:, self.c0:self.c0 + self.C]

    def f64(self):
        return self.get().double()

    def assert_outside_untouched(self):
        if self.before is None:
            return
        ity = torch.int16 if self.buf.dtype == torch.float16 else torch.int32
        a, b = self.buf.view(ity), self.before.view(ity)
        assert torch.equal(a[:, :self.c0], b[:, :self.c0]) and torch.equal(a[:, self.c0 + self.C:], b[:, self.c0 + self.C:]), \
            '%s: bytes outside the channel slice changed' % self.name


NOPL = (0, 0)


def untouched(*operands):
    for o in operands:
        if o is not None:
            o.assert_outside_untouched()


def act_f(v, act):
    if act == nc.RELU:
        return v.clamp(min=0.0)
    if act == nc.RELU6:
        return v.clamp(min=0.0, max=6.0)
    return v


def mask_f(z, act):
    """act'(z), of fp64 values"""
    if act == nc.RELU:
        return (z > 0).double()
    if act == nc.RELU6:
        return ((z > 0) & (z < 6)).double()
    return torch.ones_like(z)


def near_kink(pre, act, dtype):
    """elements whose fp64 pre-activation lies within the margin of a kink"""
    if act == nc.NONE:
        return torch.zeros_like(pre, dtype=torch.bool)
    m0 = 1e-5 * pre.abs().max().item()
    near = pre.abs() <= m0
    if act == nc.RELU6:
        near |= (pre - 6.0).abs() <= (2.0 ** -8 if dtype == 'h' else m0)
    return near


def check_ew(row, what, got, ref, A, near=None, alt=None):
    """an element-wise output against fp64.  near / alt: the elements left out of the plain comparison and the other value the
    mask allows there -- the output must be one of the two."""
    got64 = got.double()
    if near is not None and bool(near.any()):
        frac = near.double().mean().item()
        assert frac <= MAX_LEFT_OUT, '%s %s: %.2e of the elements lie within the margin of a kink' % (row.id, what, frac)
        closer_alt = near & ((got64 - alt).abs() < (got64 - ref).abs())
        ref = torch.where(closer_alt, alt, ref)
    if row.dtype == 'h':
        # (assert_half_rounded compares with >, which a NaN passes: an element the kernel never wrote still holds one)
        assert not bool(torch.isnan(got64).any()), '%s %s: %d elements were never written' % (row.id, what, int(torch.isnan(got64).sum()))
        assert_half_rounded(got64, ref, '%s %s' % (row.id, what))
        return
    bound = 4.0 * U * A + 1e-45
    bad = ~((got64 - ref).abs() <= bound)
    if bool(bad.any()):
        i = int(bad.reshape(-1).nonzero()[0])
        g, r, b = got64.reshape(-1)[i].item(), ref.reshape(-1)[i].item(), bound.reshape(-1)[i].item()
        raise AssertionError('%s %s: %d of %d elements outside 4 u A; element %d: got %.9g, fp64 %.9g, |diff| %.3e, bound %.3e'
                             % (row.id, what, int(bad.sum()), bad.numel(), i, g, r, abs(g - r), b))


def check_sum(row, what, got, ref, absum, n, extra=None):
    """per-channel sums: |sum - ref| <= n u sum|term| (+ the ambiguous terms of a recomputed mask)"""
    bound = n * U * absum + 1e-45
    if extra is not None:
        bound = bound + extra
    err = (got.double() - ref).abs()
    bad = ~(err <= bound)
    if bool(bad.any()):
        i = int(bad.reshape(-1).nonzero()[0])
        raise AssertionError('%s %s: %d of %d sums outside %d u sum|term|; entry %d: got %.9g, fp64 %.9g, |diff| %.3e, bound %.3e'
                             % (row.id, what, int(bad.sum()), bad.numel(), n, i, got.reshape(-1)[i].item(), ref.reshape(-1)[i].item(),
                                err.reshape(-1)[i].item(), bound.reshape(-1)[i].item()))


def group_sums(v, group, rows):
    """[M][C] fp64 -> [rows][C]: sums over consecutive groups of `group` rows"""
    M, C = v.shape
    g = torch.arange(M, device=v.device) // group
    return torch.zeros(rows, C, dtype=torch.float64, device=v.device).index_add_(0, g, v)


def inputs(row, with_res, y_scale=1.0):
    return _inputs(row.dtype, row.M, row.C, with_res, y_scale)


@functools.lru_cache(maxsize=64)
def _inputs(dtype, M, C, with_res, y_scale):
    """(computed once per shape and never written to: Op copies)  y = y_scale * (uniform(2) + a per-channel offset); with the coefficients below 28 % of the pre-activations lie below 0
    and 28 % above 6"""
    key = 'norminst/%s/%d_%d' % (dtype, M, C)
    y = y_scale * (fill.uniform(key + '/y', (M, C), 2.0) + fill.uniform(key + '/off', (1, C), 1.0))
    res = fill.uniform(key + '/res', (M, C), 1.0) if with_res else None
    return key, y, res


def coefficients(key, C):
    """synthetic coefficient vectors near the batch statistics of inputs(): mean = the offset, invstd = 1 / std of uniform(2),
    gamma = 4 +- 0.3, beta = 3 +- 0.3"""
    mean = dev(fill.uniform(key + '/off', (1, C), 1.0).reshape(C).contiguous())
    invstd = vec(key + '/is', C, (4.0 / 3.0 + EPS) ** -0.5, 0.02)
    gamma = vec(key + '/g', C, 4.0, 0.3)
    scale = gamma * invstd
    shift = vec(key + '/b', C, 3.0, 0.3)
    return mean, invstd, scale, shift


def pack_bits(m):
    """[M][C] of 0 / 1 -> [M][C / 32] words as int64"""
    M, C = m.shape
    w = (1 << torch.arange(32, device=m.device, dtype=torch.int64))
    return (m.to(torch.int64).view(M, C // 32, 32) * w).sum(-1)


def check_mask_words(row, mask, z, act):
    want = pack_bits(mask_f(z.f64(), act))
    got = mask.view(row.M, row.C // 32).to(torch.int64) & 0xFFFFFFFF
    assert torch.equal(got, want), '%s: activation bitmask differs from act\'(z as stored) in %d words' % (row.id, int((got != want).sum()))


# ------------------------------------------------------------------------------------------------ statistics and column sums
def run_col_stats(ops, row, yo=None, record=None):
    """pseg_col_stats(_h)"""
    M, C = row.M, row.C
    if yo is None:
        yo = Op(row, 'y', inputs(row, False)[1])
    R, rows = nc.stat_group(M, C), nc.stat_rows(M, C)
    stat = torch.full((3, rows, C), NAN, dtype=torch.float32, device='cuda')
    call(sfx(row, 'pseg_col_stats'), *yo.pl, M, C, stat.data_ptr())
    expect(row, record or row.record)
    y64 = yo.f64()
    K = y64[::R]
    assert K.shape[0] == rows and torch.equal(stat[0].double(), K), '%s: pivots are not the first row of each group' % row.id
    d = y64 - K.repeat_interleave(R, 0)[:M]
    check_sum(row, 'S1', stat[1], group_sums(d, R, rows), group_sums(d.abs(), R, rows), R)
    check_sum(row, 'S2', stat[2], group_sums(d * d, R, rows), group_sums(d * d, R, rows), R)
    untouched(yo)


def run_col_both(ops, row):
    """pseg_col_stats(_h), then pseg_col_sum(_h), on one operand"""
    yo = Op(row, 'y', inputs(row, False)[1])
    run_col_stats(ops, row, yo, row.flags['records'][0])
    run_col_sum(ops, row, yo)


def run_col_sum(ops, row, yo=None):
    """pseg_col_sum(_h): col_stats_kernel<false> + col_reduce_kernel"""
    M, C = row.M, row.C
    if yo is None:
        yo = Op(row, 'y', inputs(row, False)[1])
    R, rows = nc.stat_group(M, C), nc.stat_rows(M, C)
    init = vec('norminst/colsum/init/%d' % C, C, 0.0, 50.0)
    out = init.clone()
    ws = torch.full((rows * C + 4,), NAN, dtype=torch.float32, device='cuda')
    call(sfx(row, 'pseg_col_sum'), *yo.pl, M, C, out.data_ptr(), int(row.flags['accumulate']), ws.data_ptr(), rows * C * 4)
    expect(row, row.record)
    y64 = yo.f64()
    base = init.double() if row.flags['accumulate'] else torch.zeros(C, dtype=torch.float64, device='cuda')
    check_sum(row, 'col_sum', out, base + y64.sum(0), y64.abs().sum(0) + base.abs(), R)
    assert bool(torch.isnan(ws[rows * C:]).all()), '%s: wrote past the workspace it asked for' % row.id
    untouched(yo)


# ------------------------------------------------------------------------------------------------ forward
def run_fwd(ops, row):
    """pseg_bn_act_fwd(_h): bn_act_fwd_kernel, bn_act_fwd_rows_kernel"""
    M, C, f = row.M, row.C, row.flags
    key, y, res = inputs(row, f['residual'], 1.0 if f['coeffs'] else 3.0)
    yo, zo = Op(row, 'y', y), Op(row, 'z')
    ro = Op(row, 'residual', res) if f['residual'] else None
    mean, invstd, scale, shift = coefficients(key, C) if f['coeffs'] else (None,) * 4
    amax = torch.full((1,), 0.5, dtype=torch.float32, device='cuda') if f['amax'] else None
    mask = torch.full((M * (C // 32),), 0x5A5A5A5A, dtype=torch.int32, device='cuda') if f['mask'] else None
    args = (*yo.pl, ptr(mean), ptr(scale), ptr(shift), *(ro.pl if ro else NOPL), f['act'], *zo.pl, M, C)
    if row.dtype == 'h':
        call('pseg_bn_act_fwd_h', *args, ptr(mask))
    else:
        call('pseg_bn_act_fwd', *args, ptr(amax), ptr(mask))
    expect(row, row.record)
    check_fwd_result(row, yo, ro, zo, mean, scale, shift, f['act'], 'z')
    if mask is not None:
        check_mask_words(row, mask, zo, f['act'])
    if amax is not None:
        want = max(0.5, zo.get().abs().max().item())
        assert amax.item() == want, '%s: amax_z %.9g, max(initial, max|z|) %.9g' % (row.id, amax.item(), want)
    untouched(yo, ro, zo)


def check_fwd_result(row, yo, ro, zo, mean, scale, shift, act, what):
    y64 = yo.f64()
    if mean is not None:
        pre = (y64 - mean.double()) * scale.double() + shift.double()
        A = (y64 - mean.double()).abs() * scale.double().abs() + shift.double().abs()
    else:
        pre, A = y64, y64.abs()
    if ro is not None:
        pre = pre + ro.f64()
        A = A + ro.f64().abs()
    if act == nc.RELU6 and row.M * row.C >= 3600:
        lo, hi = (pre < 0).double().mean().item(), (pre > 6).double().mean().item()
        floor = 0.1 if mean is not None else 0.02
        assert lo > floor and hi > floor, '%s: the kinks are not crossed (%.2f below 0, %.2f above 6)' % (row.id, lo, hi)
    check_ew(row, what, zo.get(), act_f(pre, act), A)
    return pre


# ------------------------------------------------------------------------------------------------ backward, two passes
def launch_reduce(row, dzo, zo, yo, co, act, part, mask):
    rows = part.shape[1]
    call(sfx(row, 'pseg_bn_act_bwd_reduce'), *dzo.pl, *(zo.pl if zo else NOPL), *yo.pl, *[c.data_ptr() for c in co], act, row.M, row.C,
         part[0].data_ptr(), part[1].data_ptr(), ptr(mask))
    assert rows == nc.stat_rows(row.M, row.C)


def launch_apply(row, dzo, zo, yo, co, c1, c2, act, dyo, dro, res_acc, mask, hi=None, lo=None):
    args = (*dzo.pl, *(zo.pl if zo else NOPL), *yo.pl, *[c.data_ptr() for c in co], c1.data_ptr(), c2.data_ptr(), act, *dyo.pl,
            *(dro.pl if dro else NOPL), int(res_acc), row.M, row.C, ptr(mask))
    if row.dtype == 'h':
        call('pseg_bn_act_bwd_apply_h', *args)
    else:
        call('pseg_bn_act_bwd_apply', *args, ptr(hi), ptr(lo), row.C)


def backward_reference(row, dzo, zo, yo, co, act, mode):
    """-> dyh = dz * act'(.), xhat, the elements left out (MODE 3 near a kink) and dyh with their mask flipped"""
    mean, invstd, scale, shift = [c.double() for c in co]
    y64, dz64 = yo.f64(), dzo.f64()
    xhat = (y64 - mean) * invstd
    near = alt = None
    if mode == 0:
        msk = torch.ones_like(y64)
    elif mode in (1, 2):
        msk = mask_f(zo.f64(), act)                  # (the bitmask of MODE 1 is held equal to this, bit for bit)
    else:
        pre = (y64 - mean) * scale + shift
        msk = mask_f(pre, act)
        near = near_kink(pre, act, row.dtype)
        alt = dz64 * (1.0 - msk)
    return dz64 * msk, xhat, near, alt, dz64


def run_bwd(ops, row):
    """pseg_bn_act_bwd_reduce(_h) -> pseg_bn_bwd_finalize -> pseg_bn_act_bwd_apply(_h); the mask of MODE 1 / 2 comes from
    pseg_bn_act_fwd(_h) in the same test"""
    M, C, f = row.M, row.C, row.flags
    mode, act, only_apply = f['mode'], f['act'], row.entry == 'apply_only'
    with_res = mode in (1, 2)
    key, y, res = inputs(row, with_res)
    co = coefficients(key, C)
    yo = Op(row, 'y', y)
    dzo = Op(row, 'dz', fill.uniform(key + '/dz', (M, C), 1.0))
    zo = mask = ro = None
    if with_res:
        zo, ro = Op(row, 'z'), Op(row, 'residual', res)
        if C % 32 == 0:
            mask = torch.zeros(M * (C // 32), dtype=torch.int32, device='cuda')
        fa = (*yo.pl, co[0].data_ptr(), co[2].data_ptr(), co[3].data_ptr(), *ro.pl, act, *zo.pl, M, C)
        if row.dtype == 'h':
            call('pseg_bn_act_fwd_h', *fa, ptr(mask))
        else:
            call('pseg_bn_act_fwd', *fa, 0, ptr(mask))
        if mask is not None:
            check_mask_words(row, mask, zo, act)
        assert mode == 2 or mask is not None
    dyh, xhat, near, alt, dz64 = backward_reference(row, dzo, zo, yo, co, act, mode)
    R, rows = nc.stat_group(M, C), nc.stat_rows(M, C)
    z_arg, m_arg = (zo if mode == 2 else None), (mask if mode == 1 else None)

    if not only_apply:
        part = torch.full((2, rows, C), NAN, dtype=torch.float32, device='cuda')
        launch_reduce(row, dzo, z_arg, yo, co, act, part, m_arg)
        expect(row, f['records'][0])
        amb = group_sums(dz64.abs() * near.double(), R, rows) if near is not None else None
        check_sum(row, 'part_db', part[0], group_sums(dyh, R, rows), group_sums(dyh.abs(), R, rows), R, amb)
        amb = group_sums((dz64 * xhat).abs() * near.double(), R, rows) if near is not None else None
        check_sum(row, 'part_dg', part[1], group_sums(dyh * xhat, R, rows), group_sums((dyh * xhat).abs(), R, rows), R, amb)
        # finalize: dgamma / dbeta (+=), c1, c2 from the kernel's own partials
        ginit, binit = vec(key + '/ginit', C, 0.0, 30.0), vec(key + '/binit', C, 0.0, 30.0)
        dgamma, dbeta = (ginit.clone(), binit.clone()) if f['accumulate'] else (vec(None, C, fillv=NAN), vec(None, C, fillv=NAN))
        c1, c2 = vec(None, C, fillv=NAN), vec(None, C, fillv=NAN)
        call('pseg_bn_bwd_finalize', part[0].data_ptr(), part[1].data_ptr(), rows, M, C, dgamma.data_ptr(), dbeta.data_ptr(),
             int(f['accumulate']), int(f['frozen']), c1.data_ptr(), c2.data_ptr())
        expect(row, f['records'][1])
        check_bwd_finalize(row, part, M, dgamma, dbeta, ginit if f['accumulate'] else None, binit if f['accumulate'] else None, c1, c2,
                           f['frozen'])
    else:
        c1, c2 = vec(key + '/c1', C, 0.0, 0.05), vec(key + '/c2', C, 0.0, 0.05)

    dyo = Op(row, 'dy')
    rinit = fill.uniform(key + '/dres', (M, C), 1.0) if f['dres'] and f['res_accumulate'] else None
    dro = Op(row, 'dres', rinit) if f['dres'] else None
    hi = lo = None
    if f.get('planes'):
        hi = torch.full((M * C,), 0x7FFF, dtype=torch.int16, device='cuda')
        lo = torch.full((M * C,), 0x7FFF, dtype=torch.int16, device='cuda')
    rinit64 = dro.f64().clone() if rinit is not None else None
    launch_apply(row, dzo, z_arg, yo, co, c1, c2, act, dyo, dro, f['res_accumulate'], m_arg, hi, lo)
    expect(row, row.record)
    check_apply_result(row, 'dy', dyo, dro, rinit64, dyh, alt, near, xhat, co, c1, c2)
    if hi is not None:
        p = ops.split_planes(dyo.get().contiguous())
        assert torch.equal(hi, p.hi) and torch.equal(lo, p.lo), '%s: limb planes differ from split_planes(dy)' % row.id
    untouched(yo, dzo, zo, ro, dyo, dro)
    if only_apply:
        return

    # the mask sources agree bit for bit: mask-fed == z-fed; recomputed from y == z-fed when there was no residual (fp32: the
    # same arithmetic on the same values; under fp16 storage the stored z is rounded and the two part within an ulp of 6)
    other = None
    if mode == 1:
        other = zo
    elif mode == 3 and row.dtype == 'f':
        other = Op(row, 'z')
        call('pseg_bn_act_fwd', *yo.pl, co[0].data_ptr(), co[2].data_ptr(), co[3].data_ptr(), 0, 0, act, *other.pl, M, C, 0, 0)
    if other is not None:
        part2 = torch.full((2, rows, C), NAN, dtype=torch.float32, device='cuda')
        launch_reduce(row, dzo, other, yo, co, act, part2, None)
        assert ran()[4] == 2
        assert torch.equal(part2, part), '%s: partials differ between MODE %d and the z-fed mode' % (row.id, mode)
        dg2, db2 = (ginit.clone(), binit.clone()) if f['accumulate'] else (vec(None, C, fillv=NAN), vec(None, C, fillv=NAN))
        k1, k2 = vec(None, C, fillv=NAN), vec(None, C, fillv=NAN)
        call('pseg_bn_bwd_finalize', part2[0].data_ptr(), part2[1].data_ptr(), rows, M, C, dg2.data_ptr(), db2.data_ptr(),
             int(f['accumulate']), int(f['frozen']), k1.data_ptr(), k2.data_ptr())
        assert torch.equal(dg2, dgamma) and torch.equal(db2, dbeta) and torch.equal(k1, c1) and torch.equal(k2, c2), \
            '%s: dgamma / dbeta / c1 / c2 differ between MODE %d and the z-fed mode' % (row.id, mode)
        dy2 = Op(row, 'dy')
        dr2 = Op(row, 'dres', rinit) if f['dres'] else None
        launch_apply(row, dzo, other, yo, co, c1, c2, act, dy2, dr2, f['res_accumulate'], None)
        assert ran()[4] == 2
        assert torch.equal(dy2.get(), dyo.get()), '%s: dy differs between MODE %d and the z-fed mode' % (row.id, mode)
        if dr2 is not None:
            assert torch.equal(dr2.get(), dro.get()), '%s: dres differs between MODE %d and the z-fed mode' % (row.id, mode)


def check_bwd_finalize(row, part, count, dgamma, dbeta, ginit, binit, c1, c2, frozen):
    """dbeta / dgamma = the sum over the partial rows (+ the initial value), one fp32 rounding each; c1 / c2 = that sum / count"""
    for name, p, got, init, c in (('dbeta', part[0], dbeta, binit, c1), ('dgamma', part[1], dgamma, ginit, c2)):
        s = p.double().sum(0)
        if got is not None:
            base = init.double() if init is not None else torch.zeros_like(s)
            check_sum(row, name, got, base + s, p.double().abs().sum(0) + base.abs(), 2)
        if frozen:
            assert bool((c == 0).all()), '%s: frozen statistics need c1 = c2 = 0' % row.id
        else:
            # (one fp32 rounding of a double that may differ from this one by the order of its additions)
            check_sum(row, 'c of ' + name, c, s / count, (s / count).abs(), 1.01, 1e-15 * p.double().abs().sum(0) / count)


def check_apply_result(row, what, dyo, dro, rinit64, dyh, alt, near, xhat, co, c1, c2):
    scale = co[2].double()
    k1, k2 = c1.double(), c2.double()
    ref = scale * (dyh - k1 - xhat * k2)
    A = scale.abs() * (dyh.abs() + k1.abs() + xhat.abs() * k2.abs())
    ref_alt = scale * (alt - k1 - xhat * k2) if alt is not None else None
    check_ew(row, what, dyo.get(), ref, A, near, ref_alt)
    if dro is not None:
        base = rinit64 if rinit64 is not None else torch.zeros_like(dyh)
        check_ew(row, what + ' dres', dro.get(), base + dyh, base.abs() + dyh.abs(), near, base + alt if alt is not None else None)


# ------------------------------------------------------------------------------------------------ the fused small-tensor kernels
def group_stats(y64, group, rows):
    """[3][rows][C] fp32 statistics of fp64 rows, as a producer would leave them: pivot = the group's first row, the shifted sums
    rounded to fp32; groups past the last row hold NaN"""
    M, C = y64.shape
    used = nc.cdiv(M, group)
    stat = torch.full((3, rows, C), NAN, dtype=torch.float32, device=y64.device)
    K = y64[::group].float()
    d = y64 - K.double().repeat_interleave(group, 0)[:M]
    stat[0, :used] = K
    stat[1, :used] = group_sums(d, group, used).float()
    stat[2, :used] = group_sums(d * d, group, used).float()
    return stat


def chan_merge(stat, group, count):
    """Chan's parallel merge of the fp32 group statistics, in fp64 -> (mean, M2)"""
    rows = stat.shape[1]
    n = (count - torch.arange(rows, device=stat.device, dtype=torch.float64) * group).clamp(min=0.0, max=float(group))
    live = n > 0
    n = n[live].unsqueeze(1)
    K, S1, S2 = [stat[i][live].double() for i in range(3)]
    mg = K + S1 / n
    M2g = S2 - S1 * S1 / n
    mean = (n * mg).sum(0) / count
    M2 = M2g.sum(0) + (n * (mg - mean) ** 2).sum(0)
    return mean, M2.clamp(min=0.0)


def check_coefficients(row, stat, group, count, gamma, beta, co, rm0, rv0, rm, rv):
    mean64, M2 = chan_merge(stat, group, count)
    var = M2 / count
    std = var.sqrt()
    mean, invstd, scale, shift = co
    check_sum(row, 'mean', mean, mean64, mean64.abs() + std, 4)
    is64 = 1.0 / (var + EPS32).sqrt()
    check_sum(row, 'invstd', invstd, is64, is64, 4)
    g64 = gamma.double() if gamma is not None else torch.ones_like(is64)
    check_sum(row, 'scale', scale, g64 * invstd.double(), (g64 * invstd.double()).abs(), 1.01)
    assert torch.equal(shift, beta if beta is not None else torch.zeros_like(shift)), '%s: shift is not beta' % row.id
    if rm is not None:
        unbiased = M2 / (count - 1) if count > 1 else var
        want_m = (1.0 - MOM32) * rm0.double() + MOM32 * mean64
        want_v = (1.0 - MOM32) * rv0.double() + MOM32 * unbiased
        check_sum(row, 'running_mean', rm, want_m, rm0.double().abs() + mean64.abs() + std, 4)
        check_sum(row, 'running_var', rv, want_v, rv0.double().abs() + unbiased, 4)


def run_fused(ops, row):
    """pseg_bn_fwd_fused(_h) and pseg_bn_bwd_fused(_h), each beside the two-launch chain (pseg_bn_finalize + pseg_bn_act_fwd;
    pseg_bn_bwd_finalize + pseg_bn_act_bwd_apply) on the same inputs: bit-identical coefficients, both against fp64"""
    M, C, f = row.M, row.C, row.flags
    rows, act = f['rows'], f['act']
    group = nc.cdiv(M, rows)
    lanes_ok = row.dtype == 'f' or C % 8 == 0                # (the fp16 two-pass kernels work in 8-channel lanes)
    key, y, res = inputs(row, f['residual'])
    yo, zo = Op(row, 'y', y), Op(row, 'z')
    ro = Op(row, 'residual', res) if f['residual'] else None
    stat = group_stats(yo.f64(), group, rows)
    gamma, beta = vec(key + '/g', C, 4.0, 0.3), vec(key + '/b', C, 3.0, 0.3)
    rm0, rv0 = vec(key + '/rm', C, 0.0, 0.8), vec(key + '/rv', C, 1.0, 0.4)
    rm, rv = (rm0.clone(), rv0.clone()) if f['running'] else (None, None)
    co = torch.full((4, C), NAN, dtype=torch.float32, device='cuda')
    amax = torch.full((1,), 0.5, dtype=torch.float32, device='cuda') if f['amax'] else None
    head = lambda co_, rm_, rv_: (stat.data_ptr(), rows, group, M, C, gamma.data_ptr(), beta.data_ptr(), ptr(rm_), ptr(rv_), MOMENTUM, EPS,
                                  *[co_[i].data_ptr() for i in range(4)])
    tail = (*yo.pl, *(ro.pl if ro else NOPL), act, *zo.pl, M)
    if row.dtype == 'h':
        call('pseg_bn_fwd_fused_h', *head(co, rm, rv), *tail)
    else:
        call('pseg_bn_fwd_fused', *head(co, rm, rv), *tail, ptr(amax))
    expect(row, f['records'][0])
    check_coefficients(row, stat, group, M, gamma, beta, co, rm0, rv0, rm, rv)
    pre = check_fwd_result(row, yo, ro, zo, co[0], co[2], co[3], act, 'fused z')
    if amax is not None:
        want = max(0.5, zo.get().abs().max().item())
        assert amax.item() == want, '%s: amax_z %.9g, max(initial, max|z|) %.9g' % (row.id, amax.item(), want)
    # the two-launch chain
    co2 = torch.full((4, C), NAN, dtype=torch.float32, device='cuda')
    rm2, rv2 = (rm0.clone(), rv0.clone()) if f['running'] else (None, None)
    call('pseg_bn_finalize', *head(co2, rm2, rv2), 0, 0)
    assert ran() == nc.rec_finalize(rows, C), nc.describe(ran())
    assert torch.equal(co2, co), '%s: coefficients of the fused kernel and of pseg_bn_finalize differ' % row.id
    if rm is not None:
        assert torch.equal(rm2, rm) and torch.equal(rv2, rv), '%s: running statistics differ between the two chains' % row.id
    if lanes_ok:
        z2 = Op(row, 'z')
        fa = (*yo.pl, co2[0].data_ptr(), co2[2].data_ptr(), co2[3].data_ptr(), *(ro.pl if ro else NOPL), act, *z2.pl, M, C)
        if row.dtype == 'h':
            call('pseg_bn_act_fwd_h', *fa, 0)
        else:
            call('pseg_bn_act_fwd', *fa, 0, 0)
        check_fwd_result(row, yo, ro, z2, co2[0], co2[2], co2[3], act, 'chain z')
        untouched(z2)

    # backward
    mode = f['mode']
    z_arg = zo if mode == 2 else None
    dzo = Op(row, 'dz', fill.uniform(key + '/dz', (M, C), 1.0))
    cov = [co[i] for i in range(4)]
    dyh, xhat, near, alt, dz64 = backward_reference(row, dzo, zo, yo, cov, act, mode)
    part = torch.zeros(2, rows, C, dtype=torch.float32, device='cuda')
    used = nc.cdiv(M, group)
    part[0, :used] = group_sums(dyh, group, used).float()
    part[1, :used] = group_sums(dyh * xhat, group, used).float()
    ginit, binit = vec(key + '/ginit', C, 0.0, 30.0), vec(key + '/binit', C, 0.0, 30.0)
    fresh = lambda: (ginit.clone(), binit.clone()) if f['accumulate'] else (vec(None, C, fillv=NAN), vec(None, C, fillv=NAN))
    dgamma, dbeta = fresh()
    dyo = Op(row, 'dy')
    rinit = fill.uniform(key + '/dres', (M, C), 1.0) if f['dres'] and f['res_accumulate'] else None
    dro = Op(row, 'dres', rinit) if f['dres'] else None
    rinit64 = dro.f64().clone() if rinit is not None else None
    call(sfx(row, 'pseg_bn_bwd_fused'), part[0].data_ptr(), part[1].data_ptr(), rows, M, C, dgamma.data_ptr(), dbeta.data_ptr(),
         int(f['accumulate']), int(f['frozen']), *dzo.pl, *(z_arg.pl if z_arg else NOPL), *yo.pl, *[c.data_ptr() for c in cov], act,
         *dyo.pl, *(dro.pl if dro else NOPL), int(f['res_accumulate']), M)
    expect(row, row.record)
    dg2, db2 = fresh()
    c1, c2 = vec(None, C, fillv=NAN), vec(None, C, fillv=NAN)
    call('pseg_bn_bwd_finalize', part[0].data_ptr(), part[1].data_ptr(), rows, M, C, dg2.data_ptr(), db2.data_ptr(), int(f['accumulate']),
         int(f['frozen']), c1.data_ptr(), c2.data_ptr())
    assert ran() == nc.rec_bwd_finalize(rows, C), nc.describe(ran())
    assert torch.equal(dg2, dgamma) and torch.equal(db2, dbeta), '%s: dgamma / dbeta differ between the two chains' % row.id
    check_bwd_finalize(row, part, M, dgamma, dbeta, ginit if f['accumulate'] else None, binit if f['accumulate'] else None, c1, c2,
                       f['frozen'])
    check_apply_result(row, 'fused dy', dyo, dro, rinit64, dyh, alt, near, xhat, cov, c1, c2)
    if lanes_ok:
        dy2 = Op(row, 'dy')
        dr2 = Op(row, 'dres', rinit) if f['dres'] else None
        launch_apply(row, dzo, z_arg, yo, cov, c1, c2, act, dy2, dr2, f['res_accumulate'], None)
        assert ran() == nc.rec_apply(row.dtype, M, C, mode), nc.describe(ran())
        check_apply_result(row, 'chain dy', dy2, dr2, rinit64, dyh, alt, near, xhat, cov, c1, c2)
        untouched(dy2, dr2)
    untouched(yo, zo, ro, dzo, dyo, dro)


# ------------------------------------------------------------------------------------------------ the finalize kernels alone
def run_finalize(ops, row):
    """pseg_bn_finalize on partials built without the library: bn_finalize_kernel<32 | 128>, stat_merge_kernel"""
    count, C, f = row.M, row.C, row.flags
    rows, group = f['rows'], f['group']
    key = 'norminst/finalize/%d' % rows
    y = dev(fill.uniform(key + '/y', (count, C), 2.0) + fill.uniform(key + '/off', (1, C), 1.0)).double()
    stat = group_stats(y, group, rows)
    assert not bool(torch.isnan(stat).any())
    gamma, beta = (vec(key + '/g', C, 4.0, 0.3), vec(key + '/b', C, 3.0, 0.3)) if f['affine'] else (None, None)
    rm0, rv0 = vec(key + '/rm', C, 0.0, 0.8), vec(key + '/rv', C, 1.0, 0.4)
    rm, rv = (rm0.clone(), rv0.clone()) if f['running'] else (None, None)
    co = torch.full((4, C), NAN, dtype=torch.float32, device='cuda')
    nbytes = nc.finalize_workspace_bytes(rows, C)
    ws = torch.full((nbytes // 4 + 4,), NAN, dtype=torch.float32, device='cuda')
    before = stat.clone()
    call('pseg_bn_finalize', stat.data_ptr(), rows, group, count, C, ptr(gamma), ptr(beta), ptr(rm), ptr(rv), MOMENTUM, EPS,
         *[co[i].data_ptr() for i in range(4)], ws.data_ptr() if nbytes else 0, nbytes)
    expect(row, row.record)
    check_coefficients(row, stat, group, count, gamma, beta, [co[i] for i in range(4)], rm0, rv0, rm, rv)
    assert torch.equal(stat, before) and bool(torch.isnan(ws[nbytes // 4:]).all())
    if count == 1:           # one value: it is the mean, the variance is 0 (and so is the unbiased one)
        assert torch.equal(co[0], stat[0, 0]) and bool(((co[1].double() - EPS32 ** -0.5).abs() <= 4 * U * EPS32 ** -0.5).all())


def run_bwd_finalize(ops, row):
    """pseg_bn_bwd_finalize on synthetic partials: bn_bwd_finalize_kernel<32 | 128>"""
    count, C, f = row.M, row.C, row.flags
    rows = f['rows']
    key = 'norminst/bwdfin/%d' % rows
    part = dev(fill.uniform(key + '/p', (2, rows, C), 8.0))
    ginit, binit = vec(key + '/ginit', C, 0.0, 30.0), vec(key + '/binit', C, 0.0, 30.0)
    dgamma = dbeta = None
    if f['grads']:
        dgamma, dbeta = (ginit.clone(), binit.clone()) if f['accumulate'] else (vec(None, C, fillv=NAN), vec(None, C, fillv=NAN))
    c1, c2 = vec(None, C, fillv=NAN), vec(None, C, fillv=NAN)
    call('pseg_bn_bwd_finalize', part[0].data_ptr(), part[1].data_ptr(), rows, count, C, ptr(dgamma), ptr(dbeta), int(f['accumulate']),
         int(f['frozen']), c1.data_ptr(), c2.data_ptr())
    expect(row, row.record)
    check_bwd_finalize(row, part, count, dgamma, dbeta, ginit if f['accumulate'] else None, binit if f['accumulate'] else None, c1, c2,
                       f['frozen'])


def run_eval_coeffs(ops, row):
    """pseg_bn_eval_coeffs"""
    C = row.C
    gamma, beta = vec('norminst/eval/g', C, 4.0, 0.3), vec('norminst/eval/b', C, 3.0, 0.3)
    rm, rv = vec('norminst/eval/rm', C, 0.0, 0.8), vec('norminst/eval/rv', C, 1.0, 0.4)
    co = torch.full((4, C), NAN, dtype=torch.float32, device='cuda')
    call('pseg_bn_eval_coeffs', gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(), rv.data_ptr(), EPS, C, *[co[i].data_ptr() for i in range(4)])
    expect(row, row.record)
    is64 = 1.0 / (rv.double() + EPS32).sqrt()
    assert torch.equal(co[0], rm) and torch.equal(co[3], beta)
    check_sum(row, 'invstd', co[1], is64, is64, 4)                      # (an fp32 add, square root and division)
    check_sum(row, 'scale', co[2], gamma.double() * co[1].double(), (gamma.double() * co[1].double()).abs(), 1.01)


# ------------------------------------------------------------------------------------------------ activation backward, copy
def run_act_bwd(ops, row):
    """pseg_act_bwd(_h)"""
    M, C, f = row.M, row.C, row.flags
    act = f['act']
    key = 'norminst/actbwd/%s/%d_%d' % (row.dtype, M, C)
    zo = Op(row, 'z', act_f(fill.uniform(key + '/z', (M, C), 9.0), act)) if act != nc.NONE else None      # (zeros and sixes, exactly)
    dzo = Op(row, 'dz', fill.uniform(key + '/dz', (M, C), 1.0))
    scale = vec(key + '/s', C, 3.0, 1.0) if f['scale'] else None
    dyo = Op(row, 'dy') if f['dy'] else None
    rinit = fill.uniform(key + '/dres', (M, C), 1.0) if f['dres'] and f['res_accumulate'] else None
    dro = Op(row, 'dres', rinit) if f['dres'] else None
    rinit64 = dro.f64().clone() if rinit is not None else None
    call(sfx(row, 'pseg_act_bwd'), *dzo.pl, *(zo.pl if zo else NOPL), ptr(scale), act, *(dyo.pl if dyo else NOPL), *(dro.pl if dro else NOPL),
         int(f['res_accumulate']), M, C)
    expect(row, row.record)
    g = dzo.f64() * (mask_f(zo.f64(), act) if zo is not None else 1.0)
    if act == nc.RELU6:
        z64 = zo.f64()
        assert bool((z64 == 0).any()) and bool((z64 == 6).any())
    if dyo is not None:
        ref = g * scale.double() if scale is not None else g
        check_ew(row, 'dy', dyo.get(), ref, ref.abs())
    if dro is not None:
        base = rinit64 if rinit64 is not None else torch.zeros_like(g)
        check_ew(row, 'dres', dro.get(), base + g, base.abs() + g.abs())
    untouched(zo, dzo, dyo, dro)


def run_copy2d(ops, row):
    """pseg_copy2d(_h)"""
    M, C, f = row.M, row.C, row.flags
    key = 'norminst/copy/%s/%d_%d' % (row.dtype, M, C)
    xo = Op(row, 'x', fill.uniform(key + '/x', (M, C), 2.0))
    yo = Op(row, 'y', fill.uniform(key + '/y', (M, C), 2.0) if f['accumulate'] else None)
    y0 = yo.f64().clone()
    call(sfx(row, 'pseg_copy2d'), *xo.pl, *yo.pl, M, C, int(f['accumulate']))
    expect(row, row.record)
    if f['accumulate']:
        check_ew(row, 'y += x', yo.get(), y0 + xo.f64(), y0.abs() + xo.f64().abs())
    else:
        assert torch.equal(yo.get(), xo.get()), '%s: the copy is not exact' % row.id
    untouched(xo, yo)


RUNNERS = {'col_both': run_col_both, 'col_stats': run_col_stats, 'col_sum': run_col_sum, 'fwd': run_fwd, 'bwd': run_bwd, 'apply_only': run_bwd, 'fused': run_fused,
           'finalize': run_finalize, 'bwd_finalize': run_bwd_finalize, 'eval_coeffs': run_eval_coeffs, 'act_bwd': run_act_bwd,
           'copy2d': run_copy2d}


@pytest.mark.parametrize('row', nc.ROWS, ids=[r.id for r in nc.ROWS])
def test_row(ops, row):
    RUNNERS[row.entry](ops, row)


def test_every_row_has_a_runner():
    assert {r.entry for r in nc.ROWS} == set(RUNNERS)
