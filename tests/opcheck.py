"""Teacher-forced per-call checker (test infrastructure).

Inside ``with OpCheck() as oc:`` every ``pytorch_segmentation_amd.ops`` call of a real model step -- with the real
shapes, pixel strides, concat slices, accumulate flags and precision policy of that model -- is recomputed on the CPU
in fp64 *from the call's own device inputs* and compared in max-norm.  Because each call is judged on its actual
inputs, the check is independent of how ill-conditioned the whole graph is: a ReLU mask that flips between two fp32
implementations of a 50-layer network (which moves late whole-model gradients by percents in ANY fp32 implementation,
the CPU reference included -- see DESIGN.md section 4) cannot hide or fake an error here, while a 1 % systematic error
in any one mid-network data / weight gradient is a 100x violation.  Composition (which tensor feeds which call) is
what the whole-model tests check; together they pin the backward pass.

What keeps a wrong kernel from passing:
  * poisoned outputs: before a call that overwrites an output, the output's logical region (channels [:C] of the Act
    view, the whole weight gradient) is filled with NaN -- a tile the kernel skips cannot "match" with the values the
    caching allocator left there from the previous identical pass.  NaN left after the call is ``<op>.unwritten``
    (a count: zero tolerance).  Outputs that share storage with an input (in-place calls) are not poisoned;
  * a per-channel figure ``<op>.ch`` beside the tensor-wide one: max over channels of max|err_c| /
    max(max|ref_c|, 1e-2 * peak), so an error confined to low-magnitude channels is not diluted by the largest one;
  * deferred slab reductions: a weight gradient that only parks its slabs in a SlabPool is compared after the
    SlabPool.reduce that completes it; a parked call never compared fails the ``with`` block;
  * a launch census: every ``pseg_*`` entry point launched outside a checking wrapper is counted (``oc.unchecked()``);
    the every-call tests hold that set equal to an allowlist of this module (UNCHECKED_WHY).

``oc.calls`` = list of (op name, error, description); errors are relative max-norm figures, ``.unwritten`` and the
bit-exact checks (``act_to``, ``filter_transpose``, ``transpose_filters``, ``prepare_half``, counts) report the number
of wrong elements.
"""
import math

import torch
import torch.nn.functional as F

from pytorch_segmentation_amd import _lib, ops
from pytorch_segmentation_amd.arena import ParamArena

NAN = float('nan')

# Entry points a real step may launch outside every checking wrapper, and why that is sound.  The every-call tests assert
# that oc.unchecked() EQUALS the subset named for their path (allowlist(...)), so an entry point that stops being launched
# has to leave its test's list as well.
UNCHECKED_WHY = {
    'pseg_nchw_to_nhwc': 'layout copy of the fp32 NCHW input into the network; every consumer is checked on what it read',
    'pseg_nchw_to_nhwc_h': 'layout copy of the image into 8-channel fp16 pixels; every consumer is checked on what it read',
    'pseg_nhwc_to_nchw': 'layout copy of a result out of the network; the whole-model tests compare what leaves',
    'pseg_amax': 'per-tensor max|x| bound that scales fp16-limb operands; a wrong bound shows as limb error in the convs',
    'pseg_amax_batch': 'max|w| of every filter (fp16-limb scaling); a wrong bound shows as limb error in the forward convs',
    'pseg_split_planes': 'bf16 limbs of a transposed filter; the pre-split data gradient is checked against these limbs',
}


def allowlist(*names):
    """The explicit set of unchecked entry points one every-call test expects (each must be in UNCHECKED_WHY)."""
    unknown = [n for n in names if n not in UNCHECKED_WHY]
    assert not unknown, 'not in opcheck.UNCHECKED_WHY: %s' % unknown
    return set(names)


# what each every-call path launches unchecked
ALLOW_BRIDGE = {           # model(x) + compute_loss + backward through the autograd bridge, per conv policy
    'fp32': allowlist('pseg_nchw_to_nhwc'),
    'mixed': allowlist('pseg_nchw_to_nhwc'),
    'limb': allowlist('pseg_nchw_to_nhwc', 'pseg_amax'),
}
ALLOW_TRAINER_HALF = allowlist('pseg_nchw_to_nhwc_h')      # Trainer(mixed_precision=True)._fwd_loss_bwd


def nchw(a, C=None):
    """Act -> cpu fp64 NCHW"""
    v = a.view4().detach().cpu().double().permute(0, 3, 1, 2).contiguous()
    return v if C is None else v[:, :C]


def rel(got, ref):
    return ((got - ref).abs().max() / (ref.abs().max() + 1e-30)).item()


def rel_ch(got, ref, dim=1):
    """max over channels c (dimension `dim`) of max|err_c| / max(max|ref_c|, 1e-2 * peak)"""
    n = ref.shape[dim]
    g = got.movedim(dim, 0).reshape(n, -1)
    r = ref.movedim(dim, 0).reshape(n, -1)
    ra = r.abs().amax(1)
    den = torch.clamp(ra, min=1e-2 * ra.max().item()) + 1e-30
    return ((g - r).abs().amax(1) / den).max().item()


def _vec(t):
    return t.detach().cpu().double().view(1, -1, 1, 1)


def _w_oihw(w_raw, Cout, kh, kw, Cin):
    return w_raw.detach().cpu().double().view(Cout, kh, kw, Cin).permute(0, 3, 1, 2).contiguous()


def _act(t, act):
    return F.relu(t) if act == 1 else (F.relu6(t) if act == 2 else t)


def _mask(g, zz, act):
    if act == 1:
        return g * (zz > 0)
    if act == 2:
        return g * ((zz > 0) & (zz < 6))
    return g


def _span(t):
    """(device, first byte, end byte) of an Act or a tensor"""
    if isinstance(t, ops.Act):
        n = ((t.M - 1) * t.ld + t.C) if t.M > 0 else 0
        return t.t.device, t.ptr, t.ptr + n * t.t.element_size()
    return t.device, t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()


def _overlaps(out, inputs):
    d0, a0, a1 = _span(out)
    for i in inputs:
        if i is None:
            continue
        d1, b0, b1 = _span(i)
        if d0 == d1 and a0 < b1 and b0 < a1:
            return True
    return False


def _is_conv_filter(seg):
    mod = seg.module
    return seg.name == 'weight' and getattr(mod, 'kernel_size', None) and not getattr(mod, 'depthwise', True)


def _stats_err(st_rows_group, M, sref):
    """the (pivot, shifted sum, shifted sum of squares) row groups of a column-statistics result against fp64 sums"""
    st, rows, group = st_rows_group
    st = st.double().cpu()
    # group g covers rows [g*group, min(M, (g+1)*group)) -- possibly none (tiny maps under a big tile)
    cnt = (M - group * torch.arange(rows, dtype=torch.float64)).clamp(min=0.0, max=float(group))
    K, S1, S2 = st[0], st[1], st[2]
    colsum = (S1 + K * cnt[:, None]).sum(0)
    colsq = (S2 + 2 * K * S1 + K * K * cnt[:, None]).sum(0)
    return max(rel(colsum, sref.sum((0, 2, 3))), rel(colsq, (sref * sref).sum((0, 2, 3))))


def _pool_route(arg, shape, Ho, Wo, k, stride, pad):
    """the recorded argmax of a max-pool ([B][Ho][Wo][C] window-local index r * k + s, what the backward kernel routes by)
    -> (flat NCHW input index per output [B][C][Ho][Wo], mask of indices that point inside the window and the map)"""
    B, C, H, W = shape
    a = arg.detach().cpu().to(torch.int64).view(B, Ho, Wo, C).permute(0, 3, 1, 2)
    hi = torch.arange(Ho).view(1, 1, Ho, 1) * stride - pad + a // k
    wi = torch.arange(Wo).view(1, 1, 1, Wo) * stride - pad + a % k
    ok = (a < k * k) & (hi >= 0) & (hi < H) & (wi >= 0) & (wi < W)
    bc = torch.arange(B).view(B, 1, 1, 1) * C + torch.arange(C).view(1, C, 1, 1)
    return ((bc * H + hi.clamp(0, H - 1)) * W + wi.clamp(0, W - 1)), ok


class OpCheck:
    def __init__(self, verbose=False):
        self.calls = []
        self.verbose = verbose
        self._orig = {}
        self._batch_co = {}     # id(co tensor) -> (eps) for coefficient sets produced by bn_finalize (batch statistics)
        self.census = {}        # entry point -> launches outside every checking wrapper
        self.checked = {}       # entry point -> launches inside one
        self._depth = 0
        self._patched = []      # (owner, attribute, original) restored on exit
        self._parked = {}       # (id(pool), pending key) -> (fp64 gradient, description, Cout) of a call that parked slabs
        self._reduces = 0
        self._after_reduce = {}  # gradient address -> host copy after the last wrapped SlabPool.reduce

    def report(self, name, err, info=''):
        self.calls.append((name, err, info))
        if self.verbose:
            print('%-18s err %.2e  %s' % (name, err, info), flush=True)

    def worst(self, prefix=''):
        sel = [c for c in self.calls if c[0].startswith(prefix)]
        return max(sel, key=lambda c: c[1]) if sel else None

    def unchecked(self):
        """set of pseg_* entry points launched outside every checking wrapper while the check was active"""
        return set(self.census)

    # ------------------------------------------------------------------------------------------ helpers
    def _cmp(self, name, got, ref, info='', dim=1):
        """tensor-wide figure, and the per-channel one along `dim` (None: none)"""
        self.report(name, rel(got, ref), info)
        if dim is not None:
            self.report(name + '.ch', rel_ch(got, ref, dim), info)

    def _poison(self, out, C=None, inputs=()):
        """NaN into channels [:C] of the Act `out` (or all of a tensor) unless it shares storage with an input.
        -> True when poisoned"""
        if out is None or _overlaps(out, inputs):
            return False
        if isinstance(out, ops.Act):
            out.view4()[..., :(out.C if C is None else C)].fill_(NAN)
        else:
            out.view(-1)[:(out.numel() if C is None else C)].fill_(NAN)
        return True

    def _unwritten(self, name, got, info=''):
        self.report(name + '.unwritten', float(torch.isnan(got).sum().item()), info)

    def _pool_arg_check(self, name, arg, zin, got, k, stride, pad, info):
        """the recorded argmax points inside its window, at a value equal to the pooled output (to the forward's yardstick)"""
        if arg is None:
            return
        flat, ok = _pool_route(arg, tuple(zin.shape), got.shape[2], got.shape[3], k, stride, pad)
        self.report(name + '.arg_invalid', float((~ok).sum().item()), info)
        self.report(name + '.arg', rel(zin.reshape(-1)[flat], got), info)

    def _guard(self, fn):
        def guarded(*a, **k):
            self._depth += 1
            try:
                return fn(*a, **k)
            finally:
                self._depth -= 1
        return guarded

    def _patch(self, owner, attr, new):
        self._patched.append((owner, attr, owner.__dict__[attr] if isinstance(owner, type) else getattr(owner, attr)))
        setattr(owner, attr, new)

    class _PoisonNew:
        """while active, every Act that ops.Act.empty hands out (without zero=True) starts as NaN in channels [:C]: the
        outputs a call allocates for itself (Act.to, ce_upsampled_fwd_bwd's gradient)"""

        def __init__(self):
            self.orig = ops.Act.__dict__['empty']

        def __enter__(self):
            f = self.orig.__func__

            def empty(*a, **k):
                act = f(*a, **k)
                if not k.get('zero', False) and act.M > 0:
                    act.view4().fill_(NAN)
                return act
            ops.Act.empty = staticmethod(empty)

        def __exit__(self, *exc):
            ops.Act.empty = self.orig

    # ------------------------------------------------------------------------------------------ wrappers
    def __enter__(self):
        o = self._orig
        rep = self.report
        cmp = self._cmp
        poison = self._poison
        unwritten = self._unwritten

        def wrap(name, fn):
            o[name] = getattr(ops, name)
            setattr(ops, name, self._guard(fn))

        def conv2d_fwd(x, w_raw, bias_raw, y, kh, kw, stride, pad, dil, accumulate=False, want_stats=False, **kx):
            prev = nchw(y) if accumulate else None
            xin = nchw(x)
            pz = not accumulate and poison(y, inputs=(x,))
            r = o['conv2d_fwd'](x, w_raw, bias_raw, y, kh, kw, stride, pad, dil, accumulate=accumulate,
                                want_stats=want_stats, **kx)
            ref = F.conv2d(xin, _w_oihw(w_raw, y.C, kh, kw, x.C),
                           bias_raw.detach().cpu().double() if bias_raw is not None else None, stride, pad, dil)
            if accumulate:
                ref = ref + prev
            info = 'x%s -> y%s k%d s%d p%d d%d ldx%d ldy%d' % ((x.B, x.C, x.H, x.W), (y.B, y.C, y.H, y.W), kh, stride, pad, dil,
                                                             x.ld, y.ld)
            if getattr(x, 'half', False) and not getattr(y, 'half', False):
                info += ' fp32-out'         # fp16 operands, result written in fp32 (the class logits under the half policy)
            got = nchw(y)
            if pz:
                unwritten('conv2d_fwd', got, info)
            cmp('conv2d_fwd', got, ref, info)
            if want_stats and r is not None:
                # fp16 results: the statistics are those of the values AS STORED (rounded to fp16) -- what the layer
                # normalises and what its backward pass reads -- so that is what they are checked against
                sref = got if getattr(y, 'half', False) else ref
                rep('conv2d_fwd.stats', _stats_err(r, y.M, sref), 'rows %d' % r[1])
            return r

        def col_stats(y):
            r = o['col_stats'](y)
            rep('col_stats', _stats_err(r, y.M, nchw(y)), 'y%s rows %d' % ((y.B, y.C, y.H, y.W), r[1]))
            return r

        def conv2d_dgrad(dy, wT_raw, dx, kh, kw, stride, pad, dil, accumulate=False, **kx):
            prev = nchw(dx) if accumulate else None
            g = nchw(dy)
            pz = not accumulate and poison(dx, inputs=(dy,))
            o['conv2d_dgrad'](dy, wT_raw, dx, kh, kw, stride, pad, dil, accumulate=accumulate, **kx)
            Cout, Cin = dy.C, dx.C
            w = wT_raw.detach().cpu().double().view(Cin, kh * kw, Cout).permute(2, 0, 1).reshape(Cout, Cin, kh, kw)
            ref = torch.nn.grad.conv2d_input((dx.B, Cin, dx.H, dx.W), w, g, stride, pad, dil)
            if accumulate:
                ref = ref + prev
            info = 'dy%s -> dx%s k%d s%d p%d d%d acc%d' % ((dy.B, dy.C, dy.H, dy.W), (dx.B, dx.C, dx.H, dx.W), kh, stride, pad,
                                                           dil, accumulate)
            got = nchw(dx)
            if pz:
                unwritten('conv2d_dgrad', got, info)
            cmp('conv2d_dgrad', got, ref, info)

        def conv2d_dgrad_planes(dy_planes, dy, wT_planes, dx, kh, kw, stride, pad, dil, accumulate=False):
            prev = nchw(dx) if accumulate else None
            g = nchw(dy)
            # the planes handed over are the limbs of dy itself (bn_act_bwd(want_planes=True)): bit-exact
            want = ops.split_planes(dy)
            same = torch.equal(want.hi, dy_planes.hi) and torch.equal(want.lo, dy_planes.lo)
            rep('dgrad_planes.limbs', 0.0 if same else 1.0)
            pz = not accumulate and poison(dx, inputs=(dy,))
            o['conv2d_dgrad_planes'](dy_planes, dy, wT_planes, dx, kh, kw, stride, pad, dil, accumulate=accumulate)
            Cout, Cin = dy.C, dx.C

            def f32(p):
                return (p.to(torch.int32) << 16).view(torch.float32).cpu().double()
            w = (f32(wT_planes.hi) + f32(wT_planes.lo)).view(Cin, -1)[:, :kh * kw * Cout]
            w = w.reshape(Cin, kh * kw, Cout).permute(2, 0, 1).reshape(Cout, Cin, kh, kw)
            ref = torch.nn.grad.conv2d_input((dx.B, Cin, dx.H, dx.W), w, g, stride, pad, dil)
            if accumulate:
                ref = ref + prev
            info = 'planes dy%s -> dx%s k%d s%d p%d d%d acc%d' % ((dy.B, dy.C, dy.H, dy.W), (dx.B, dx.C, dx.H, dx.W), kh, stride,
                                                                  pad, dil, accumulate)
            got = nchw(dx)
            if pz:
                unwritten('conv2d_dgrad', got, info)
            cmp('conv2d_dgrad', got, ref, info)

        def conv2d_wgrad(x, dy, dw_raw, kh, kw, stride, pad, dil, accumulate=False, pool=None, **kx):
            prev = dw_raw.detach().cpu().double().clone().reshape(-1) if accumulate else None
            xin, g = nchw(x), nchw(dy)
            # (a call that parks its slabs leaves dw alone until pool.reduce(accumulate) -- with this call's own flag, so the
            # NaN of a non-accumulating call is overwritten there)
            pz = not accumulate and poison(dw_raw, inputs=(x, dy))
            n0 = len(pool.pending) if pool is not None else 0
            red0 = self._reduces
            o['conv2d_wgrad'](x, dy, dw_raw, kh, kw, stride, pad, dil, accumulate=accumulate, pool=pool, **kx)
            Cout = dy.C
            ref = torch.nn.grad.conv2d_weight(xin, (Cout, x.C, kh, kw), g, stride, pad, dil).permute(0, 2, 3, 1).reshape(-1)
            info = 'x%s dy%s k%d s%d p%d d%d acc%d' % ((x.B, x.C, x.H, x.W), (dy.B, dy.C, dy.H, dy.W), kh, stride, pad, dil,
                                                      accumulate)
            if pool is not None and len(pool.pending) == n0 + 1 and pool.pending[-1][0] == dw_raw.data_ptr():
                # slabs parked: dw_raw is complete only after the pool's reduce -- compared there
                self._parked[(id(pool), pool.pending[-1])] = (ref, info + ' slabs', Cout)
                return
            if self._reduces != red0 and dw_raw.data_ptr() in self._after_reduce:
                # a second gradient of the same filter in one pass: the pool folded what was parked, then this call added
                ref = ref + self._after_reduce[dw_raw.data_ptr()].double()
            elif accumulate:
                ref = ref + prev
            got = dw_raw.detach().cpu().double().reshape(-1)
            if pz and self._reduces == red0:
                unwritten('conv2d_wgrad', got, info)
            cmp('conv2d_wgrad', got.view(Cout, -1), ref.view(Cout, -1), info, dim=0)

        def bn_finalize(stats, count, gamma, beta, running_mean, running_var, momentum, eps):
            co = o['bn_finalize'](stats, count, gamma, beta, running_mean, running_var, momentum, eps)
            self._batch_co[id(co)] = (co, eps, gamma, beta)
            return co

        def bn_act_fwd(y, co, act, z, residual=None, want_mask=False):
            yin = nchw(y)
            rin = nchw(residual) if residual is not None else None
            pz = poison(z, inputs=(y, residual))
            mask = o['bn_act_fwd'](y, co, act, z, residual=residual, want_mask=want_mask)
            if mask is not None:      # the activation bitmask must be exactly act'(z) of the z just written
                zz = z.view4()[..., :y.C].reshape(y.M, y.C)
                on = (zz > 0) if act == 1 else ((zz > 0) & (zz < 6))
                w = (on.view(y.M, y.C // 32, 32).to(torch.int64) << torch.arange(32, device=on.device)).sum(-1)
                w = torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)
                rep('bn_act_fwd.mask', float((w.reshape(-1) != mask).sum().item()), 'y%s' % ((y.B, y.C, y.H, y.W),))
                self.bn_masks = getattr(self, 'bn_masks', 0) + 1
            t = yin
            if co is not None:
                if id(co) in self._batch_co:      # batch statistics: mean / invstd / scale must be those of THIS y
                    _, eps, gamma, beta = self._batch_co[id(co)]
                    mu = yin.mean((0, 2, 3))
                    var = yin.var((0, 2, 3), unbiased=False)
                    is_ = 1.0 / (var + eps).sqrt()
                    gm = gamma.detach().cpu().double() if gamma is not None else torch.ones_like(mu)
                    e_mu = ((co[0].detach().cpu().double() - mu).abs().max() / (mu.abs().max() + var.sqrt().max() + 1e-30)).item()
                    rep('bn_finalize', max(e_mu, rel(co[1].detach().cpu().double(), is_),
                                           rel(co[2].detach().cpu().double(), gm * is_)), 'C%d M%d' % (y.C, y.M))
                t = (t - _vec(co[0])) * _vec(co[2]) + _vec(co[3])
            if rin is not None:
                t = t + rin
            info = 'y%s act%d res%d' % ((y.B, y.C, y.H, y.W), act, residual is not None)
            got = nchw(z)
            if pz:
                unwritten('bn_act_fwd', got, info)
            cmp('bn_act_fwd', got, _act(t, act), info)
            return mask

        def bn_fwd_fused(stats, count, gamma, beta, running_mean, running_var, momentum, eps, y, act, z, residual=None):
            yin = nchw(y)
            rin = nchw(residual) if residual is not None else None
            rm0 = running_mean.detach().cpu().double().clone() if running_mean is not None else None
            rv0 = running_var.detach().cpu().double().clone() if running_var is not None else None
            pz = poison(z, inputs=(y, residual))
            co = o['bn_fwd_fused'](stats, count, gamma, beta, running_mean, running_var, momentum, eps, y, act, z,
                                   residual=residual)
            mu = yin.mean((0, 2, 3))
            var = yin.var((0, 2, 3), unbiased=False)
            is_ = 1.0 / (var + eps).sqrt()
            gm = gamma.detach().cpu().double() if gamma is not None else torch.ones_like(mu)
            bt = beta.detach().cpu().double() if beta is not None else torch.zeros_like(mu)
            e_mu = ((co[0].detach().cpu().double() - mu).abs().max() / (mu.abs().max() + var.sqrt().max() + 1e-30)).item()
            rep('bn_finalize', max(e_mu, rel(co[1].detach().cpu().double(), is_), rel(co[2].detach().cpu().double(), gm * is_)),
                'fused C%d M%d' % (y.C, y.M))
            if rm0 is not None:
                n = float(y.M)
                rep('bn_running_stats', max(rel(running_mean.detach().cpu().double(), (1 - momentum) * rm0 + momentum * mu),
                                            rel(running_var.detach().cpu().double(), (1 - momentum) * rv0 + momentum * var * n / max(n - 1, 1))))
            t = (yin - mu.view(1, -1, 1, 1)) * (gm * is_).view(1, -1, 1, 1) + bt.view(1, -1, 1, 1)
            if rin is not None:
                t = t + rin
            info = 'fused y%s act%d res%d' % ((y.B, y.C, y.H, y.W), act, residual is not None)
            got = nchw(z)
            if pz:
                unwritten('bn_act_fwd', got, info)
            cmp('bn_act_fwd', got, _act(t, act), info)
            return co

        def bn_act_bwd(dz, z, y, co, act, dy, gamma_grad, beta_grad, accumulate=False, dres=None, res_accumulate=False,
                       frozen=False, mask=None, want_planes=False, part=None):
            g, yy = nchw(dz), nchw(y)
            zz = nchw(z) if z is not None else (yy - _vec(co[0])) * _vec(co[2]) + _vec(co[3])
            pg = gamma_grad.detach().cpu().double().clone() if gamma_grad is not None else None
            pb = beta_grad.detach().cpu().double().clone() if beta_grad is not None else None
            pres = nchw(dres) if (dres is not None and res_accumulate) else None
            ins = (dz, z, y)
            pz = poison(dy, inputs=ins)
            pr = dres is not None and not res_accumulate and poison(dres, inputs=ins)
            if not accumulate:
                poison(gamma_grad)
                poison(beta_grad)
            o['bn_act_bwd'](dz, z, y, co, act, dy, gamma_grad, beta_grad, accumulate=accumulate, dres=dres,
                            res_accumulate=res_accumulate, frozen=frozen, mask=mask, want_planes=want_planes, part=part)
            g = _mask(g, zz, act)
            xh = (yy - _vec(co[0])) * _vec(co[1])
            M = y.M
            db = g.sum((0, 2, 3))
            dg = (g * xh).sum((0, 2, 3))
            # yardstick of a column sum: the largest sum of |terms| (a BatchNorm bias that feeds conv + BatchNorm has
            # dbeta == 0 in exact arithmetic: sum / max|sum| would compare rounding noise with rounding noise)
            db_scale = g.abs().sum((0, 2, 3)).max().item() + 1e-30
            dg_scale = (g * xh).abs().sum((0, 2, 3)).max().item() + 1e-30
            ref = _vec(co[2]) * (g if frozen else (g - db.view(1, -1, 1, 1) / M - xh * dg.view(1, -1, 1, 1) / M))
            info = 'y%s act%d frozen%d' % ((y.B, y.C, y.H, y.W), act, frozen)
            got = nchw(dy)
            if pz:
                unwritten('bn_act_bwd.dy', got, info)
            cmp('bn_act_bwd.dy', got, ref, info)
            if gamma_grad is not None:
                gg, bg = gamma_grad.detach().cpu().double(), beta_grad.detach().cpu().double()
                if not accumulate:
                    unwritten('bn_act_bwd.dgamma', gg, info)
                    unwritten('bn_act_bwd.dbeta', bg, info)
                rep('bn_act_bwd.dgamma', (gg - dg - (pg if accumulate else 0)).abs().max().item()
                    / (dg_scale + (pg.abs().max().item() if accumulate else 0.0)))
                rep('bn_act_bwd.dbeta', (bg - db - (pb if accumulate else 0)).abs().max().item()
                    / (db_scale + (pb.abs().max().item() if accumulate else 0.0)))
            if dres is not None:
                got = nchw(dres)
                if pr:
                    unwritten('bn_act_bwd.dres', got, info)
                rep('bn_act_bwd.dres', rel(got, g + (pres if pres is not None else 0)))

        def act_bwd(dz, z, act, dy, scale=None, dres=None, res_accumulate=False):
            g = nchw(dz)
            zz = nchw(z) if z is not None else None
            pres = nchw(dres) if (dres is not None and res_accumulate) else None
            pz = dy is not None and poison(dy, inputs=(dz, z))
            pr = dres is not None and not res_accumulate and poison(dres, inputs=(dz, z))
            o['act_bwd'](dz, z, act, dy, scale=scale, dres=dres, res_accumulate=res_accumulate)
            g = _mask(g, zz, act) if act else g
            if dy is not None:
                got = nchw(dy)
                if pz:
                    unwritten('act_bwd.dy', got)
                rep('act_bwd.dy', rel(got, g * _vec(scale) if scale is not None else g))
            if dres is not None:
                got = nchw(dres)
                if pr:
                    unwritten('act_bwd.dres', got)
                rep('act_bwd.dres', rel(got, g + (pres if pres is not None else 0)))

        def bilinear_fwd(x, y, align_corners):
            xin = nchw(x)
            pz = poison(y, inputs=(x,))
            o['bilinear_fwd'](x, y, align_corners)
            ref = F.interpolate(xin, size=(y.H, y.W), mode='bilinear', align_corners=bool(align_corners))
            info = 'x%s -> %dx%d' % ((x.B, x.C, x.H, x.W), y.H, y.W)
            got = nchw(y)
            if pz:
                unwritten('bilinear_fwd', got, info)
            rep('bilinear_fwd', rel(got, ref), info)

        def bilinear_fwd_nchw(x, C, Ho, Wo, align_corners):
            xin = nchw(x, C)
            out = o['bilinear_fwd_nchw'](x, C, Ho, Wo, align_corners)
            ref = F.interpolate(xin, size=(Ho, Wo), mode='bilinear', align_corners=bool(align_corners))
            rep('bilinear_fwd_nchw', rel(out.detach().cpu().double(), ref), 'x%s -> %dx%d' % ((x.B, C, x.H, x.W), Ho, Wo))
            return out

        def _bil_grad(g, shape, align_corners):
            with torch.enable_grad():
                xin = torch.zeros(*shape, dtype=torch.float64, requires_grad=True)
                F.interpolate(xin, size=tuple(g.shape[2:]), mode='bilinear', align_corners=bool(align_corners)).backward(g)
            return xin.grad

        def bilinear_bwd(dy, dx, align_corners, accumulate=False):
            g = nchw(dy)
            prev = nchw(dx) if accumulate else 0
            pz = not accumulate and poison(dx, inputs=(dy,))
            o['bilinear_bwd'](dy, dx, align_corners, accumulate=accumulate)
            info = 'dy%s acc%d' % ((dy.B, dy.C, dy.H, dy.W), accumulate)
            got = nchw(dx)
            if pz:
                unwritten('bilinear_bwd', got, info)
            rep('bilinear_bwd', rel(got, _bil_grad(g, (dx.B, dx.C, dx.H, dx.W), align_corners) + prev), info)

        def bilinear_bwd_nchw(dy_nchw, dx, C, align_corners, accumulate=False):
            g = dy_nchw.detach().cpu().double()
            prev = nchw(dx, C) if accumulate else 0
            pz = not accumulate and poison(dx, C, inputs=(dy_nchw,))
            o['bilinear_bwd_nchw'](dy_nchw, dx, C, align_corners, accumulate=accumulate)
            info = 'dy%s' % (tuple(dy_nchw.shape),)
            got = nchw(dx, C)
            if pz:
                unwritten('bilinear_bwd_nchw', got, info)
            rep('bilinear_bwd_nchw', rel(got, _bil_grad(g, (dx.B, C, dx.H, dx.W), align_corners) + prev), info)

        def copy2d(x, y, accumulate=False):
            prev = nchw(y) if accumulate else 0
            xin = nchw(x)
            pz = not accumulate and poison(y, inputs=(x,))
            o['copy2d'](x, y, accumulate=accumulate)
            info = 'x%s acc%d' % ((x.B, x.C, x.H, x.W), accumulate)
            got = nchw(y)
            if pz:
                unwritten('copy2d', got, info)
            rep('copy2d', rel(got, xin + prev), info)

        def pool_sum(x, out, scale):
            xin = nchw(x)
            pz = poison(out, inputs=(x,))
            o['pool_sum'](x, out, scale)
            info = 'x%s' % ((x.B, x.C, x.H, x.W),)
            got = nchw(out)
            if pz:
                unwritten('pool_sum', got, info)
            rep('pool_sum', rel(got, scale * xin.sum((2, 3), keepdim=True)), info)

        def broadcast(x, y, scale=1.0, accumulate=False):
            prev = nchw(y) if accumulate else 0
            xin = nchw(x)
            pz = not accumulate and poison(y, inputs=(x,))
            o['broadcast'](x, y, scale=scale, accumulate=accumulate)
            got = nchw(y)
            if pz:
                unwritten('broadcast', got)
            rep('broadcast', rel(got, scale * xin.expand(-1, -1, y.H, y.W) + prev), 'acc%d' % accumulate)

        def maxpool_fwd(x, y, k, stride, pad, want_argmax=True):
            xin = nchw(x)
            pz = poison(y, inputs=(x,))
            arg = o['maxpool_fwd'](x, y, k, stride, pad, want_argmax=want_argmax)
            info = 'x%s' % ((x.B, x.C, x.H, x.W),)
            got = nchw(y)
            if pz:
                unwritten('maxpool_fwd', got, info)
            rep('maxpool_fwd', rel(got, F.max_pool2d(xin, k, stride, pad)), info)
            self._pool_arg_check('maxpool_fwd', arg, xin, got, k, stride, pad, info)
            return arg

        def bn_act_maxpool_fwd(x, co, act, y, k, stride, pad, want_argmax=True):
            # the ResNet stem without its activated map: BatchNorm (coefficients checked against THIS x) + activation + max-pool
            xin = nchw(x)
            pz = poison(y, inputs=(x,))
            arg = o['bn_act_maxpool_fwd'](x, co, act, y, k, stride, pad, want_argmax=want_argmax)
            if id(co) in self._batch_co:
                _, eps, gamma, beta = self._batch_co[id(co)]
                mu = xin.mean((0, 2, 3))
                var = xin.var((0, 2, 3), unbiased=False)
                is_ = 1.0 / (var + eps).sqrt()
                gm = gamma.detach().cpu().double() if gamma is not None else torch.ones_like(mu)
                e_mu = ((co[0].detach().cpu().double() - mu).abs().max() / (mu.abs().max() + var.sqrt().max() + 1e-30)).item()
                rep('bn_finalize', max(e_mu, rel(co[1].detach().cpu().double(), is_), rel(co[2].detach().cpu().double(), gm * is_)),
                    'C%d M%d' % (x.C, x.M))
            z = _act((xin - _vec(co[0])) * _vec(co[2]) + _vec(co[3]), act)
            if x.half:      # the pooling compares the values as the separate pass would have STORED them (ties after rounding)
                z = z.half().double()
            info = 'x%s act%d' % ((x.B, x.C, x.H, x.W), act)
            got = nchw(y)
            if pz:
                unwritten('bn_act_maxpool_fwd', got, info)
            rep('bn_act_maxpool_fwd', rel(got, F.max_pool2d(z, k, stride, pad)), info)
            self._pool_arg_check('bn_act_maxpool_fwd', arg, z, got, k, stride, pad, info)
            return arg

        def maxpool_bwd(dy, arg, dx, k, stride, pad, accumulate=False):
            g = nchw(dy)
            prev = nchw(dx) if accumulate else 0
            pz = not accumulate and poison(dx, inputs=(dy,))
            o['maxpool_bwd'](dy, arg, dx, k, stride, pad, accumulate=accumulate)
            # dy goes where the forward pass recorded the maximum (its argmax is checked there: a position holding the
            # window's maximum).  Not re-derived from fp64 inputs: under the half policy two window values within one fp16
            # rounding of each other can trade places, and either is a correct argmax.
            flat, ok = _pool_route(arg, (dx.B, dx.C, dx.H, dx.W), dy.H, dy.W, k, stride, pad)
            ref = torch.zeros(dx.B * dx.C * dx.H * dx.W, dtype=torch.float64)
            ref.index_add_(0, flat[ok], g[ok])
            info = 'dy%s' % ((dy.B, dy.C, dy.H, dy.W),)
            got = nchw(dx)
            if pz:
                unwritten('maxpool_bwd', got, info)
            rep('maxpool_bwd', rel(got, ref.view(dx.B, dx.C, dx.H, dx.W) + prev), info)

        def dwconv_fwd(x, w_raw, y, k, stride, pad):
            xin = nchw(x)
            pz = poison(y, inputs=(x,))
            o['dwconv_fwd'](x, w_raw, y, k, stride, pad)
            w = w_raw.detach().cpu().double().view(k, k, x.C).permute(2, 0, 1).unsqueeze(1)
            info = 'x%s s%d' % ((x.B, x.C, x.H, x.W), stride)
            got = nchw(y)
            if pz:
                unwritten('dwconv_fwd', got, info)
            cmp('dwconv_fwd', got, F.conv2d(xin, w, None, stride, pad, 1, groups=x.C), info)

        def dwconv_dgrad(dy, w_raw, dx, k, stride, pad):
            g = nchw(dy)
            pz = poison(dx, inputs=(dy,))
            o['dwconv_dgrad'](dy, w_raw, dx, k, stride, pad)
            w = w_raw.detach().cpu().double().view(k, k, dx.C).permute(2, 0, 1).unsqueeze(1)
            ref = torch.nn.grad.conv2d_input((dx.B, dx.C, dx.H, dx.W), w, g, stride, pad, 1, groups=dx.C)
            info = 'dx%s s%d' % ((dx.B, dx.C, dx.H, dx.W), stride)
            got = nchw(dx)
            if pz:
                unwritten('dwconv_dgrad', got, info)
            cmp('dwconv_dgrad', got, ref, info)

        def dwconv_wgrad(x, dy, dw_raw, k, stride, pad, accumulate=False):
            prev = dw_raw.detach().cpu().double().clone().view(-1)[:k * k * x.C].view(k, k, x.C) if accumulate else 0
            xin, g = nchw(x), nchw(dy)
            pz = not accumulate and poison(dw_raw, k * k * x.C, inputs=(x, dy))
            o['dwconv_wgrad'](x, dy, dw_raw, k, stride, pad, accumulate=accumulate)
            ref = torch.nn.grad.conv2d_weight(xin, (x.C, 1, k, k), g, stride, pad, 1, groups=x.C)[:, 0].permute(1, 2, 0) + prev
            info = 'x%s s%d acc%d' % ((x.B, x.C, x.H, x.W), stride, accumulate)
            got = dw_raw.detach().cpu().double().view(-1)[:k * k * x.C].view(k, k, x.C)
            if pz:
                unwritten('dwconv_wgrad', got, info)
            cmp('dwconv_wgrad', got, ref, info, dim=2)

        def col_sum(dy, out, accumulate=False, C=None):
            Cc = dy.C if C is None else C
            prev = out.detach().cpu().double().clone() if accumulate else 0
            g = nchw(dy, Cc)
            pz = not accumulate and poison(out, Cc, inputs=(dy,))
            o['col_sum'](dy, out, accumulate=accumulate, C=C)
            got = out.detach().cpu().double()[:Cc]
            if pz:
                unwritten('col_sum', got, 'C%d' % Cc)
            rep('col_sum', rel(got, (g.sum((0, 2, 3)) + (prev[:Cc] if accumulate else 0))), 'C%d' % Cc)

        def ce_fwd_bwd(logits, target, want_grad=True, ignore_index=-100):
            out, dl = o['ce_fwd_bwd'](logits, target, want_grad=want_grad, ignore_index=ignore_index)
            with torch.enable_grad():
                lg = logits.detach().cpu().double().requires_grad_()
                ref = F.cross_entropy(lg, target.cpu(), ignore_index=ignore_index)
                ref.backward()
            rep('ce.loss', abs(out[0].item() - ref.item()) / abs(ref.item()))
            if dl is not None:
                rep('ce.dlogits', rel(dl.detach().cpu().double(), lg.grad))
            return out, dl

        def ce_upsampled_fwd_bwd(lr, C, target, align_corners, want_grad=True, ignore_index=-100):
            # the fused low-resolution loss: fp64 interpolate + cross_entropy, labels outside [0, C) that are not
            # ignore_index are ignored AND counted (torch would raise on them)
            with self._PoisonNew():
                out, dlr = o['ce_upsampled_fwd_bwd'](lr, C, target, align_corners, want_grad=want_grad,
                                                     ignore_index=ignore_index)
            t = target.detach().cpu()
            bad = (t != ignore_index) & ((t < 0) | (t >= C))
            tt = torch.where(bad, torch.full_like(t, ignore_index), t)
            n_valid = int((tt != ignore_index).sum().item())
            info = 'lr%s C%d -> %dx%d ac%d' % ((lr.B, lr.C, lr.H, lr.W), C, t.shape[1], t.shape[2], int(bool(align_corners)))
            with torch.enable_grad():
                xr = nchw(lr, C).clone().requires_grad_()
                up = F.interpolate(xr, size=(int(t.shape[1]), int(t.shape[2])), mode='bilinear',
                                   align_corners=bool(align_corners))
                ref = F.cross_entropy(up, tt, ignore_index=ignore_index)
                if n_valid:
                    ref.backward()
            res = out.detach().cpu().double()
            rep('ce_upsampled.loss', abs(res[0].item() - ref.item()) / abs(ref.item()) if n_valid else abs(res[0].item()), info)
            rep('ce_upsampled.count', abs(res[1].item() - n_valid), info)
            rep('ce_upsampled.bad', abs(res[2].item() - int(bad.sum().item())), info)
            if dlr is not None:
                got = nchw(dlr)
                unwritten('ce_upsampled.dlogits', got, info)
                g = xr.grad if n_valid else torch.zeros_like(xr)
                rep('ce_upsampled.dlogits', rel(got[:, :C], g), info)
                # padded channels are written as zero (the class logits' padding reads zero downstream)
                rep('ce_upsampled.dlogits.pad', float(torch.count_nonzero(got[:, C:]).item()), info)
            return out, dlr

        def scale_inplace(x, gscale):
            x0 = x.detach().cpu().double().clone()
            s = gscale.detach().cpu().double().reshape(-1)[0]
            o['scale_inplace'](x, gscale)
            rep('scale_inplace', rel(x.detach().cpu().double(), x0 * s), 'n%d' % x.numel())

        def filter_transpose(w_raw, Cout, taps, Cin):
            wT = o['filter_transpose'](w_raw, Cout, taps, Cin)
            ref = w_raw.detach().cpu().view(Cout, taps, Cin).permute(2, 1, 0)
            got = wT.detach().cpu().view(Cin, taps, Cout)
            rep('filter_transpose', float((got != ref).sum().item()), 'Cout%d taps%d Cin%d' % (Cout, taps, Cin))
            return wT

        for name, fn in list(locals().items()):
            if callable(fn) and hasattr(ops, name) and name not in ('wrap',):
                wrap(name, fn)

        # ---- methods: Act.to (fp32 <-> fp16 with the loss scale), SlabPool.reduce, the arena's batched filter copies
        act_to0 = ops.Act.to

        def act_to(a, dtype, scale=None):
            with self._PoisonNew():
                out = act_to0(a, dtype, scale=scale)
            S = 1.0 if scale is None else float(scale.detach().cpu().reshape(-1)[0].item())
            info = '%s -> %s M%d C%d S %g' % (a.dtype, dtype, a.M, a.C, S)
            # the loss scale is a power of two: x * S is exact, the single rounding is the conversion
            rep('act_to.scale_pow2', 0.0 if S > 0 and math.frexp(S)[0] == 0.5 else 1.0, info)
            ref = (a.view4().detach().cpu().float() * S).to(dtype)
            got = out.view4().detach().cpu()
            unwritten('act_to', got.float(), info)
            rep('act_to', float((got.float() != ref.float()).sum().item()), info)
            return out
        self._patch(ops.Act, 'to', self._guard(act_to))

        reduce0 = ops.SlabPool.reduce

        def reduce(pool, accumulate=False):
            keys = list(pool.pending)
            prevs = {}
            for k in keys:
                dw = pool.regions[k][3]
                if accumulate:
                    prevs[k] = dw.detach().cpu().double().reshape(-1).clone()
                else:
                    poison(dw)      # dw = sum of slabs: every element is written here
            reduce0(pool, accumulate)
            self._reduces += 1
            self._after_reduce = {}
            for k in keys:
                dw = pool.regions[k][3]
                got = dw.detach().cpu().double().reshape(-1)
                self._after_reduce[dw.data_ptr()] = got
                hit = self._parked.pop((id(pool), k), None)
                if hit is None:
                    continue
                ref, info, Cout = hit
                if accumulate:
                    ref = ref + prevs[k]
                else:
                    unwritten('conv2d_wgrad', got, info)
                cmp('conv2d_wgrad', got.view(Cout, -1), ref.view(Cout, -1), info, dim=0)
        self._patch(ops.SlabPool, 'reduce', self._guard(reduce))

        transpose0 = ParamArena.transpose_filters

        def transpose_filters(ar):
            transpose0(ar)
            bad = n = 0
            for seg in ar.segments:
                mod = seg.module
                if not _is_conv_filter(seg) or getattr(mod, '_wT_view', None) is None:
                    continue
                cop, kh, kw, cip = seg.raw_shape
                w = ar.params[seg.offset:seg.offset + cop * kh * kw * cip].detach().cpu().view(cop, kh * kw, cip)
                ref = torch.zeros(cip, kh * kw, cop)
                co, ci = mod.out_channels, mod.in_channels
                ref[:ci, :, :co] = w[:co, :, :ci].permute(2, 1, 0)
                bad += int((mod._wT_view.detach().cpu().view(cip, kh * kw, cop) != ref).sum().item())
                n += 1
            rep('transpose_filters', float(bad), '%d filters' % n)
        self._patch(ParamArena, 'transpose_filters', self._guard(transpose_filters))

        prepare0 = ParamArena.prepare_half

        def prepare_half(ar, transposed=True):
            prepare0(ar, transposed=transposed)
            bad = n = 0
            for seg in ar.segments:
                mod = seg.module
                if not _is_conv_filter(seg) or getattr(mod, '_w_h_view', None) is None:
                    continue
                cop, kh, kw, cip = seg.raw_shape
                w = ar.params[seg.offset:seg.offset + cop * kh * kw * cip].detach().cpu().view(cop, kh * kw, cip)
                co, ci = mod.out_channels, mod.in_channels
                co8, ci8 = (cop + 7) // 8 * 8, (cip + 7) // 8 * 8
                ref = torch.zeros(co8, kh * kw, ci8, dtype=torch.float16)
                ref[:co, :, :ci] = w[:co, :, :ci].half()       # rounded to fp16 once; zero in the padding
                bad += int((mod._w_h_view.detach().cpu().view(co8, kh * kw, ci8) != ref).sum().item())
                if transposed:
                    bad += int((mod._wT_h_view.detach().cpu().view(ci8, kh * kw, co8) != ref.permute(2, 1, 0)).sum().item())
                n += 1
            rep('prepare_half', float(bad), '%d filters transposed%d' % (n, int(transposed)))
        self._patch(ParamArena, 'prepare_half', self._guard(prepare_half))

        # ---- census: every library launch outside a checking wrapper
        call0 = _lib.call

        def call(name, *args):
            d = self.checked if self._depth else self.census
            d[name] = d.get(name, 0) + 1
            return call0(name, *args)
        self._patch(_lib, 'call', call)
        return self

    def __exit__(self, *exc):
        for k, v in self._orig.items():
            setattr(ops, k, v)
        self._orig.clear()
        for owner, attr, v in reversed(self._patched):
            setattr(owner, attr, v)
        self._patched = []
        self._batch_co.clear()
        parked, self._parked = self._parked, {}
        if parked and exc[0] is None:
            raise AssertionError('OpCheck: %d weight gradients parked their slabs and no SlabPool.reduce completed them: %s'
                                 % (len(parked), [v[1] for v in parked.values()][:4]))
