"""Every compiled instance and every host branch of the loss / mask / metric launches (csrc/loss.hip), one row of
tests/loss_cases.py at a time: the row's entry point is called directly through the C ABI, pseg_debug_last_loss must answer the
record the row names (kernel, CMAX, VEC, grid, block, form of the up-sampled loss, partials handed to the finish kernel, gradient
asked for), and every output is compared element by element with fp64 on the CPU (tests/test_loss_instances_cpu.py shows without a
GPU that the rows reach every instance and that a plain fp32 evaluation stays inside the bounds below).

Bounds, derived (u = 2^-24, the unit roundoff of fp32; they are computed in tests/loss_cases.py from the fp64 reference alone).

Gradient of the plain loss, every element: |got - ref| <= K u A, A = (p_c + [t == c]) / n_valid.  With D the row's largest
|z - max z| the kernel forms g = e_c * (inv_n / s) - [t == c] * inv_n, e_c = __expf(z_c - m) = exp2((z_c - m) * log2 e):
  z_c - m                one rounding, D u absolute, so D u relative on e_c
  (z_c - m) * log2 e     the rounding of the product and of the constant: 2 D u relative on e_c
  exp2                   V_EXP_F32: 1 ulp = 2 u ("AMD Instinct MI300 / CDNA3 Instruction Set Architecture", V_EXP_F32 and V_LOG_F32:
                         1 ULP accuracy; the CDNA4 document restates it)
  s = sum e_c            C - 1 additions of positive terms, (C - 1) u, on top of the (3 D + 2) u of its terms
  inv_n, inv_n / s, e_c * scale   u each (correctly rounded division: hipcc's default), and u A for the final multiply-subtract
=> K = (3 D + 2) + (C - 1 + 3 D + 2) + 3 + 1, rounded up to K = 6 D + C + 8; the term [t == c] inv_n carries u, inside it.
ce_generic_kernel goes through lse = m + logf(s) and expf(z - lse) with the library functions (1 ulp): the argument z - lse carries
u (|lse| + 2 ln s + C + D + 1) from lse and u (D + ln C) of its own: K = 2 D + max|z| + 4 ln C + C + 8.

Loss: |loss - ref| <= K_l u mean|term|, term = 1 + |m| + ln s + |z_t| over the valid pixels (the 1: the relative error of s enters
ln s absolutely).  ln s = log2(s) * ln 2 carries 4 u ln s (V_LOG_F32 1 ulp, constant, product) and the (C + 3 D + 1) u of s; m + ln s
and - z_t one rounding each of at most the term; the partials are summed in double, the mean is rounded once: K_l = 3 D + C + 8.

Up-sampled loss: the same with z the interpolated logits, plus
  the four taps          three products / additions per axis and 1 - l1: 6 u max|x| absolute on a logit
  the weights            s = scale * o: two roundings of a value below the source size n, and 1 - l1: (2 n + 1) u absolute on a weight
                         (none at ratio 1 with align_corners, where scale == 1 and s == o exactly), which moves a logit by that times
                         the largest difference between neighbouring source logits along the axis.  A first tap that lands on the
                         other side of an integer is the same error: the interpolation is continuous
=> E_v absolute on a logit (in u), 4 E_v relative on p (2 E_v on z - m, as much on s): K = 4 E_v + (6 D + C + 8) + n_y + n_x + 8, n_y,
n_x the destination indices that touch one source index (the separable fixed-order sums; 8: two weight products, three patch
additions, inv_n, the last multiply).  The gradient also takes the weights' own error, dw_y w_x + w_y dw_x on every pixel of the
support: folded into K as the row's largest ratio of that sum to A.  A = sum_{Y,X} w_y w_x (p_c + [t == c]) / n_valid.
K_l = 2 E_v + 3 D + C + 8.  This is why the rows keep h, w <= 16 apart from the finish-loop and grid-stride rows, whose K grows.

Counts are exact; the gradient is exactly 0 at invalid pixels and in channels [C, ldd); no NaN is left in a written gradient (the
gradient buffers start as NaN, the padded logit channels hold NaN); bytes around the operands are unchanged; two calls give the same
bits; loss-only gives the bits of the full call's loss; the gather form matches the scatter form within 2 K (each within K of fp64:
different summation orders)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import loss_cases as lc
from oracle import fill

pytestmark = pytest.mark.gpu

NAN = float('nan')
WORST = {}                                   # entry -> the largest error / (u A) seen (printed by the last test)


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
    rec = (ctypes.c_int * 8)()
    assert _lib.load().pseg_debug_last_loss(rec) == 0
    return tuple(rec)


def expect(row, record):
    got = ran()
    assert got == record, 'meant to test %s:\n  %s\nran\n  %s' % (row.id, lc.describe(record), lc.describe(got))


def note(row, what, value, K):
    key = '%s %s' % (row.entry, what)
    WORST[key] = max(WORST.get(key, (0.0, 0.0, '')), (value, K, row.id))
    print('%s %s: worst error %.2f u, K %.0f' % (row.id, what, value, K))


class Framed:
    """n elements inside a larger device buffer: `front` elements before and 4 after hold a canary (NaN for floats) whose bits
    must not change.  front = 4: the operand is 16-byte aligned; front = 1 (floats): four bytes off."""

    def __init__(self, n, dtype=torch.float32, front=4, values=None, canary=NAN):
        self.n, self.front = n, front
        self.buf = torch.full((front + n + 4,), canary, dtype=dtype, device='cuda')
        assert self.buf.data_ptr() % 16 == 0
        if values is not None:
            self.buf[front:front + n] = values.reshape(-1).to('cuda', dtype)
        self.before = self.buf.clone()

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.front * self.buf.element_size()

    def get(self):
        return self.buf[self.front:self.front + self.n]

    def assert_frame_untouched(self, what):
        ity = {4: torch.int32, 8: torch.int64}[self.buf.element_size()]
        a, b = self.buf.view(ity), self.before.view(ity)
        assert torch.equal(a[:self.front], b[:self.front]) and torch.equal(a[self.front + self.n:], b[self.front + self.n:]), \
            '%s: bytes outside the operand changed' % what

    def assert_unchanged(self, what):
        ity = {4: torch.int32, 8: torch.int64}[self.buf.element_size()]
        assert torch.equal(self.buf.view(ity), self.before.view(ity)), '%s: an input changed' % what


def bits(t):
    return t.view(torch.int32)


def workspace(nbytes):
    """the workspace a call asks for, and 64 canary bytes behind it"""
    ws = torch.full((nbytes + 64,), 0x5A, dtype=torch.uint8, device='cuda')
    assert ws.data_ptr() % 16 == 0
    return ws


def assert_workspace_kept(row, ws, nbytes):
    assert bool((ws[nbytes:] == 0x5A).all()), '%s: wrote past the workspace it asked for' % row.id


# ------------------------------------------------------------------------------------------------ plain cross-entropy
def launch_ce(row, lg, tg, ign, dl, out):
    B, C, H, W = row.shape
    nbytes = lc.ce_workspace_bytes()
    ws = workspace(nbytes)
    call('pseg_ce_fwd_bwd', lg.ptr, tg.data_ptr(), B, C, H * W, ign, dl.ptr if dl is not None else 0, out.data_ptr(), ws.data_ptr(), nbytes)
    assert_workspace_kept(row, ws, nbytes)


def run_ce(row):
    """pseg_ce_fwd_bwd: ce_count_kernel, ce_fused_kernel<CMAX, VEC> | ce_generic_kernel, ce_finish_kernel"""
    B, C, H, W = row.shape
    x, t, ign = lc.ce_inputs(row)
    ref = lc.ce_reference(row)
    mis = row.flags.get('mis')
    lg = Framed(x.numel(), front=1 if mis == 'logits' else 4, values=x)
    tg = t.cuda()
    outs, grads = [], []
    for rep in range(2):                                              # two calls: the same bits
        dl = Framed(x.numel(), front=1 if mis == 'dlogits' else 4)
        out = torch.full((3,), NAN, dtype=torch.float32, device='cuda')
        launch_ce(row, lg, tg, ign, dl, out)
        expect(row, row.record)
        dl.assert_frame_untouched(row.id + ' dlogits')
        outs.append(out)
        grads.append(dl.get().clone())
    lg.assert_unchanged(row.id + ' logits')
    assert torch.equal(tg.cpu(), t)
    assert torch.equal(bits(outs[0]), bits(outs[1])) and torch.equal(bits(grads[0]), bits(grads[1])), '%s: two calls differ' % row.id
    loss, n_valid, n_bad = outs[0].tolist()
    assert (n_valid, n_bad) == (ref.n_valid, ref.n_bad), '%s: counts (%r, %r), fp64 (%d, %d)' % (row.id, n_valid, n_bad, ref.n_valid, ref.n_bad)
    note(row, 'loss', lc.check_loss(row, 'loss', loss, ref), ref.K_loss)
    got = grads[0].cpu().view(B, C, H, W)
    note(row, 'dlogits', lc.check_grad(row, 'dlogits', got, ref), ref.K)
    invalid = (lc.map_labels(t, C, ign) == ign).unsqueeze(1).expand(B, C, H, W)
    assert bool((got[invalid] == 0).all()), '%s: the gradient is not 0 at %d invalid pixels' % (row.id, int((got[invalid] != 0).sum()))
    if row.flags.get('only_class'):
        assert loss == 0.0 and bool((got == 0).all()), '%s: one class: loss 0, gradient 0' % row.id
    if row.flags.get('nograd'):
        out = torch.full((3,), NAN, dtype=torch.float32, device='cuda')
        launch_ce(row, lg, tg, ign, None, out)
        # (a NULL gradient is not a misaligned one: the loss-only call of such a row may take the vector instance)
        expect(row, lc.rec_ce(B, C, H * W, logits_aligned=mis != 'logits', grad=False))
        if mis is None:
            assert torch.equal(bits(out), bits(outs[0])), '%s: loss-only differs from the loss of the full call' % row.id
        else:
            assert out[1:].tolist() == [ref.n_valid, ref.n_bad]
            lc.check_loss(row, 'loss-only', out[0].item(), ref)


# ------------------------------------------------------------------------------------------------ up-sampled cross-entropy
def launch_up(row, L, tg, dL, out):
    B, C, h, w, H, W, ac, ld, ldd = row.shape
    from pytorch_segmentation_amd import _lib
    nbytes = _lib.query('pseg_ce_upsampled_workspace_bytes', B, h, w)
    assert nbytes == lc.ce_upsampled_workspace_bytes(B, h, w)
    ws = workspace(nbytes)
    call('pseg_ce_upsampled_fwd_bwd', L.data_ptr(), ld, B, h, w, C, tg.data_ptr(), H, W, ac, -100, dL.data_ptr() if dL is not None else 0,
         ldd, out.data_ptr(), ws.data_ptr(), nbytes)
    assert_workspace_kept(row, ws, nbytes)


def up_once(row, L, tg, grad=True):
    """one call -> (loss_out, dlogits_lr [B h w + 2][ldd] | None); the gradient buffer starts as NaN, two rows longer than the operand"""
    B, C, h, w, H, W, ac, ld, ldd = row.shape
    dL = torch.full((B * h * w + 2, ldd), NAN, dtype=torch.float32, device='cuda') if grad else None
    out = torch.full((3,), NAN, dtype=torch.float32, device='cuda')
    launch_up(row, L, tg, dL, out)
    return out, dL


def run_ce_up(row, monkeypatch):
    """pseg_ce_upsampled_fwd_bwd: ce_up_scatter_kernel + ce_up_finish_kernel + ce_up_combine_kernel | ce_count_kernel +
    ce_up_fused_kernel + ce_finish_kernel"""
    B, C, h, w, H, W, ac, ld, ldd = row.shape
    env = row.flags['env']
    if env is None:
        monkeypatch.delenv('PSEG_CE_SCATTER', raising=False)
    else:
        monkeypatch.setenv('PSEG_CE_SCATTER', env)
    x, t = lc.up_inputs(row)
    ref = lc.up_reference(row)
    n = B * h * w
    L = torch.full((n + 2, ld), NAN, dtype=torch.float32, device='cuda')          # NaN in the padded channels and past the operand
    L[:n, :C] = x.permute(0, 2, 3, 1).reshape(n, C).cuda()
    L0 = L.clone()
    tg = t.cuda()
    out, dL = up_once(row, L, tg)
    expect(row, row.record)
    out2, dL2 = up_once(row, L, tg)
    assert torch.equal(bits(out), bits(out2)) and torch.equal(bits(dL), bits(dL2)), '%s: two calls differ' % row.id
    assert torch.equal(bits(L), bits(L0)) and torch.equal(tg.cpu(), t), '%s: an input changed' % row.id
    loss, n_valid, n_bad = out.tolist()
    assert (n_valid, n_bad) == (ref.n_valid, ref.n_bad), '%s: counts (%r, %r), fp64 (%d, %d)' % (row.id, n_valid, n_bad, ref.n_valid, ref.n_bad)
    note(row, 'loss', lc.check_loss(row, 'loss', loss, ref), ref.K_loss)
    d = dL.cpu()
    assert bool(torch.isnan(d[n:]).all()), '%s: rows past B h w were written' % row.id
    assert not bool(torch.isnan(d[:n]).any()), '%s: %d elements of the gradient were never written (channels %s)' % (
        row.id, int(torch.isnan(d[:n]).sum()), sorted(set(torch.isnan(d[:n]).nonzero()[:, 1].tolist())))
    assert bool((d[:n, C:] == 0).all()), '%s: channels [C, ldd) are not 0' % row.id
    got = d[:n, :C].view(B, h, w, C).permute(0, 3, 1, 2)
    note(row, 'dlogits_lr', lc.check_grad(row, 'dlogits_lr', got, ref), ref.K)
    if ref.n_valid == 0:
        assert bool((d[:n] == 0).all()), '%s: no valid pixel: the gradient is 0' % row.id
    if row.flags.get('nograd'):
        out3, none = up_once(row, L, tg, grad=False)
        expect(row, lc.without_gradient(row.record))
        assert torch.equal(bits(out3), bits(out)), '%s: loss-only differs from the loss of the full call' % row.id
    if env == '0' and lc.scatter_eligible(h, w, H, W, ac) and not row.flags.get('big'):
        # the two forms side by side: each within K of fp64, so within 2 K of each other (not bit-equal: other summation orders)
        monkeypatch.delenv('PSEG_CE_SCATTER')
        out4, dL4 = up_once(row, L, tg)
        expect(row, lc.rec_ce_up(B, h, w, H, W, ac, None))
        assert ran()[5] == lc.SCATTER
        assert out4[1:].tolist() == [ref.n_valid, ref.n_bad]
        lc.check_loss(row, 'scatter loss', out4[0].item(), ref)
        diff = (dL4.cpu()[:n, :C].double() - d[:n, :C].double()).abs().view(B, h, w, C).permute(0, 3, 1, 2)
        assert bool((diff <= 2.0 * ref.K * lc.U * ref.A).all()), '%s: gather and scatter forms differ beyond 2 K u A' % row.id
        assert torch.equal(bits(dL4[n:]), bits(dL[n:])) and bool((dL4[:n, C:] == 0).all())


# ------------------------------------------------------------------------------------------------ argmax
def run_argmax(row):
    """pseg_argmax: argmax_kernel<4 | 1> == torch.max(1)[1] on the same fp32 values (first index on ties; no NaN inputs)"""
    B, C, HW = row.shape
    x = fill.uniform('lossinst/argmax/%d_%d_%d' % row.shape, (B, C, HW), 3.0)
    if not row.flags.get('big'):
        if C > 1:
            x[0, 1] = -math.inf                             # a whole plane of -inf (the pixels planted below apart)
        x[:, 0, 0] = x[:, C - 1, 0] = 10.0                  # the first and the last class tie: the first
        x[:, C // 2, 1] = x[:, C - 1, 1] = 10.0             # the middle and the last class tie: the middle
        x[:, C - 1, 2] = 10.0                               # the last class alone
        x[:, :, 3] = 1.5                                    # every class ties: the first
        x[:, :, 4] = -math.inf                              # ... at -inf too
    else:
        x[0, 1, ::7] = x[0, 0, ::7]                         # ties over a seventh of the pixels
    want = x.max(1)[1]
    if not row.flags.get('big'):
        assert want[:, :5].tolist() == [[0, C // 2, C - 1, 0, 0]] * B                  # (stated outright)
    lg = Framed(x.numel(), front=1 if row.flags.get('mis') else 4, values=x)
    mask = Framed(B * HW, dtype=torch.int64, canary=-12345)
    call('pseg_argmax', lg.ptr, B, C, HW, mask.ptr)
    expect(row, row.record)
    got = mask.get().cpu().view(B, HW)
    assert torch.equal(got, want), '%s: %d of %d pixels differ from torch.max(1)[1]' % (row.id, int((got != want).sum()), got.numel())
    mask.assert_frame_untouched(row.id + ' mask')
    lg.assert_unchanged(row.id + ' logits')


# ------------------------------------------------------------------------------------------------ confusion
def run_confusion(row):
    """pseg_confusion: confusion_kernel; the call accumulates into counters that already hold something"""
    n, C = row.shape
    key = 'lossinst/confusion/%d_%d' % row.shape
    pred = fill.labels(key + '/p', (n,), C + 4) - 2                    # [-2, C + 2): outside [0, C) on both sides
    target = fill.labels(key + '/t', (n,), C + 4) - 2
    match = fill.labels(key + '/m', (n,), 2) == 1                      # half the predictions hit
    pred = torch.where(match, target, pred)
    for i, v in enumerate((-100, 255, -100, 255)):
        if n > 8:
            (pred if i < 2 else target)[3 + 2 * i] = v
    before = torch.arange(3 * C, dtype=torch.int64).view(3, C) * 7 + 5
    cnt = Framed(3 * C, dtype=torch.int64, values=before, canary=-12345)
    p, t = pred.cuda(), target.cuda()
    call('pseg_confusion', p.data_ptr(), t.data_ptr(), n, C, cnt.ptr)
    expect(row, row.record)
    pn, tn = pred.numpy(), target.numpy()
    tin, pin = (tn >= 0) & (tn < C), (pn >= 0) & (pn < C)
    want = before.numpy().copy()
    want[0] += np.bincount(tn[tin & (pn == tn)], minlength=C)
    want[1] += np.bincount(tn[tin & (pn != tn)], minlength=C)
    want[2] += np.bincount(pn[pin & (pn != tn)], minlength=C)
    got = cnt.get().cpu().view(3, C).numpy()
    assert np.array_equal(got, want), '%s: %d of %d counters differ' % (row.id, int((got != want).sum()), got.size)
    cnt.assert_frame_untouched(row.id + ' counters')
    assert torch.equal(p.cpu(), pred) and torch.equal(t.cpu(), target)


# ------------------------------------------------------------------------------------------------ scale_inplace
def run_scale(row):
    """pseg_scale_inplace: scale_inplace_kernel; g = 2.5: the fp32 product exactly; g = 1: the bits unchanged"""
    (n,) = row.shape
    x = fill.uniform('lossinst/scale/%d' % n, (n,), 3.0)
    buf = Framed(n, values=x)
    call('pseg_scale_inplace', buf.ptr, n, torch.tensor([2.5], device='cuda').data_ptr())
    expect(row, row.record)
    want = x * torch.tensor(2.5)                                        # one fp32 multiplication: IEEE, the same on the host
    got = buf.get().cpu()
    assert torch.equal(bits(got), bits(want)), '%s: %d of %d elements are not the fp32 product (first at %d)' % (
        row.id, int((bits(got) != bits(want)).sum()), n, int((bits(got) != bits(want)).nonzero()[0]))
    buf.assert_frame_untouched(row.id)
    call('pseg_scale_inplace', buf.ptr, n, torch.ones(1, device='cuda').data_ptr())
    expect(row, row.record)
    assert torch.equal(bits(buf.get().cpu()), bits(want)), '%s: g = 1 changed bits' % row.id
    buf.assert_frame_untouched(row.id)


RUNNERS = {'ce': run_ce, 'ce_up': run_ce_up, 'argmax': run_argmax, 'confusion': run_confusion, 'scale': run_scale}


@pytest.mark.parametrize('row', lc.ROWS, ids=[r.id for r in lc.ROWS])
def test_row(ops, row, monkeypatch):
    if row.entry == 'ce_up':
        run_ce_up(row, monkeypatch)
    else:
        RUNNERS[row.entry](row)


def test_every_row_has_a_runner():
    assert {r.entry for r in lc.ROWS} == set(RUNNERS)


def test_worst_errors_are_reported():
    """the head-room: per entry and output the largest error in units of u A (u mean|term| for the loss), beside its K"""
    for key in sorted(WORST):
        value, K, id = WORST[key]
        print('worst %s: %.2f u at K = %.0f (%s)' % (key, value, K, id))
        assert value <= K
