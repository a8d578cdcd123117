"""Self-tests of the per-call checker (tests/opcheck.py), one per way a wrong kernel could slip through it.

No GPU and no library: the "kernels" here are Python fakes monkeypatched over the ops entry points BEFORE the checker
wraps them, writing into host-memory Acts; `_lib.call` / `_lib.query` are stubbed.  Each test first shows that a correct
fake passes, then that the broken one is caught."""
import pytest
import torch
import torch.nn.functional as F

import opcheck
from opcheck import OpCheck
from pytorch_segmentation_amd import _lib, ops

TOL = 1e-4      # the fp32 every-call bound


def act_of(x_nchw, ld=None):
    """fp32 NCHW host tensor -> host Act (pixel stride ld)"""
    B, C, H, W = x_nchw.shape
    ld = ld or (C + 3) // 4 * 4
    t = torch.zeros(B * H * W * ld, dtype=torch.float32)
    a = ops.Act(t, B, H, W, C, ld)
    a.view4().copy_(x_nchw.permute(0, 2, 3, 1))
    return a


def failures(oc, tol=TOL):
    return [c for c in oc.calls if not c[1] < tol]


@pytest.fixture()
def no_lib(monkeypatch):
    """_lib.call records launches instead of making them; _lib.query answers a constant"""
    launched = []
    monkeypatch.setattr(_lib, 'call', lambda name, *a: launched.append(name))
    monkeypatch.setattr(_lib, 'query', lambda name, *a: 64)
    return launched


def _conv_case(seed=0, Cin=4, Cout=8, quiet=None):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, Cin, 6, 6, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g)
    if quiet is not None:
        w[quiet] *= 1e-2        # one output channel at 1/100 of the peak
    w_raw = w.permute(0, 2, 3, 1).contiguous().view(-1)      # [Cout][kh][kw][Cin]
    ref = F.conv2d(x.double(), w.double(), None, 1, 1)
    return act_of(x), w_raw, act_of(torch.zeros(2, Cout, 6, 6)), ref


def _fake_conv_fwd(write=True, bump=None):
    def conv2d_fwd(x, w_raw, bias_raw, y, kh, kw, stride, pad, dil, accumulate=False, want_stats=False, **kx):
        if write:
            xn = x.view4().permute(0, 3, 1, 2).double()
            w = w_raw.double().view(y.C, kh, kw, x.C).permute(0, 3, 1, 2)
            r = F.conv2d(xn, w, None, stride, pad, dil)
            if bump is not None:                # (channel, absolute error) added to one element
                r[0, bump[0], 0, 0] += bump[1]
            y.view4().copy_(r.permute(0, 2, 3, 1))
        return None
    return conv2d_fwd


def test_stale_output_is_caught(no_lib, monkeypatch):
    """An output that already holds the right answer (the caching allocator hands back the block of the previous
    identical pass) and a kernel that never writes it: the poisoned output stays NaN."""
    x, w_raw, y, ref = _conv_case()
    monkeypatch.setattr(ops, 'conv2d_fwd', _fake_conv_fwd(write=True))
    with OpCheck() as oc:
        ops.conv2d_fwd(x, w_raw, None, y, 3, 3, 1, 1, 1)
    assert not failures(oc) and oc.worst('conv2d_fwd')[1] < 1e-6
    y.view4().copy_(ref.permute(0, 2, 3, 1))        # the stale block: exactly the right values
    monkeypatch.setattr(ops, 'conv2d_fwd', _fake_conv_fwd(write=False))
    with OpCheck() as oc:
        ops.conv2d_fwd(x, w_raw, None, y, 3, 3, 1, 1, 1)
    bad = failures(oc)
    assert bad and any(op == 'conv2d_fwd.unwritten' and err == 2 * 8 * 6 * 6 for op, err, _ in bad), oc.calls


def test_error_in_a_quiet_channel_is_caught(no_lib, monkeypatch):
    """One output channel at 1/100 of the tensor's peak, off by 5x the bound in that channel: the tensor-wide figure is
    1/20 of the bound and passes, the per-channel figure must not."""
    x, w_raw, y, ref = _conv_case(quiet=3)
    peak3 = ref[:, 3].abs().max().item()
    assert peak3 < 0.05 * ref.abs().max().item()
    monkeypatch.setattr(ops, 'conv2d_fwd', _fake_conv_fwd(bump=(3, 5 * TOL * peak3)))
    with OpCheck() as oc:
        ops.conv2d_fwd(x, w_raw, None, y, 3, 3, 1, 1, 1)
    glob = [err for op, err, _ in oc.calls if op == 'conv2d_fwd']
    assert glob and max(glob) < TOL / 4           # the tensor-wide max-norm dilutes it
    bad = failures(oc)
    assert bad and all(op == 'conv2d_fwd.ch' for op, _, _ in bad), oc.calls
    # (5x the bound when the channel's peak is above the 1e-2 * peak floor of the figure, less where the floor applies)
    assert TOL < max(err for _, err, _ in bad) < 5.5 * TOL


def _wgrad_case():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 4, 5, 5, generator=g)
    dy = torch.randn(2, 8, 5, 5, generator=g)
    ref = torch.nn.grad.conv2d_weight(x.double(), (8, 4, 1, 1), dy.double(), 1, 0, 1).permute(0, 2, 3, 1).reshape(-1)
    return act_of(x), act_of(dy), ref


def _fake_parking_wgrad():
    """a split weight gradient under a SlabPool: two slabs (images 0 and 1) parked, dw untouched"""
    def conv2d_wgrad(x, dy, dw_raw, kh, kw, stride, pad, dil, accumulate=False, precision=None, pool=None, concurrent=False):
        slabs = pool.region(dw_raw, ('geom',), 2)
        n = dw_raw.numel()
        for b in range(2):
            xb = x.view4()[b:b + 1].permute(0, 3, 1, 2).double()
            gb = dy.view4()[b:b + 1].permute(0, 3, 1, 2).double()
            part = torch.nn.grad.conv2d_weight(xb, (dy.C, x.C, kh, kw), gb, stride, pad, dil).permute(0, 2, 3, 1)
            slabs[b * n:(b + 1) * n] = part.reshape(-1).float()
    return conv2d_wgrad


def _fake_reduce(wrong=False):
    def reduce(pool, accumulate=False):
        for key in pool.pending:
            slabs, elems, splits, dw = pool.regions[key]
            s = slabs.view(splits, elems)
            tot = s[0] if wrong else s.sum(0)           # wrong: the last slab is dropped
            dw.copy_(dw + tot if accumulate else tot)
        pool.pending = []
    return reduce


def test_parked_weight_gradient_without_reduce_is_caught(no_lib, monkeypatch):
    """A weight gradient that only parks its slabs is complete after SlabPool.reduce: compared at call time, a gradient
    that still holds last pass's (right) values would pass.  A check that ends with the call never compared fails."""
    x, dy, ref = _wgrad_case()
    monkeypatch.setattr(ops, 'conv2d_wgrad', _fake_parking_wgrad())
    monkeypatch.setattr(ops.SlabPool, 'reduce', _fake_reduce())
    pool = ops.SlabPool(torch.device('cpu'))
    dw = ref.float().clone()            # last pass's gradient, the right answer
    with OpCheck() as oc:
        ops.conv2d_wgrad(x, dy, dw, 1, 1, 1, 0, 1, pool=pool)
        pool.reduce()
    assert not failures(oc) and any(op == 'conv2d_wgrad' for op, _, _ in oc.calls)
    with pytest.raises(AssertionError, match='parked'):
        with OpCheck():
            ops.conv2d_wgrad(x, dy, dw, 1, 1, 1, 0, 1, pool=pool)
    pool.pending = []


def test_wrong_slab_reduction_is_caught(no_lib, monkeypatch):
    """The deferred reduction itself is checked, honouring reduce(accumulate)."""
    x, dy, ref = _wgrad_case()
    monkeypatch.setattr(ops, 'conv2d_wgrad', _fake_parking_wgrad())
    monkeypatch.setattr(ops.SlabPool, 'reduce', _fake_reduce())
    pool = ops.SlabPool(torch.device('cpu'))
    dw = torch.full((ref.numel(),), 0.25)
    with OpCheck() as oc:                               # correct reduction, accumulating into what is there
        ops.conv2d_wgrad(x, dy, dw, 1, 1, 1, 0, 1, accumulate=True, pool=pool)
        pool.reduce(accumulate=True)
    assert not failures(oc) and torch.allclose(dw.double(), ref + 0.25, atol=1e-5)
    dw.copy_(ref.float())
    monkeypatch.setattr(ops.SlabPool, 'reduce', _fake_reduce(wrong=True))
    with OpCheck() as oc:
        ops.conv2d_wgrad(x, dy, dw, 1, 1, 1, 0, 1, pool=pool)
        pool.reduce()
    bad = failures(oc)
    assert bad and any(op == 'conv2d_wgrad' and err > 0.1 for op, err, _ in bad), oc.calls


def test_unchecked_launch_is_counted(no_lib, monkeypatch):
    """A library launch outside every checking wrapper shows in the census; one inside a wrapper does not."""
    def copy2d(x, y, accumulate=False):
        _lib.call('pseg_copy2d', 0)
        y.view4().copy_(x.view4())
    monkeypatch.setattr(ops, 'copy2d', copy2d)
    x = act_of(torch.randn(1, 4, 3, 3))
    y = act_of(torch.zeros(1, 4, 3, 3))
    with OpCheck() as oc:
        ops.copy2d(x, y)
        _lib.call('pseg_nhwc_to_nchw', 0)
        _lib.call('pseg_nhwc_to_nchw', 0)
    assert no_lib == ['pseg_copy2d', 'pseg_nhwc_to_nchw', 'pseg_nhwc_to_nchw']
    assert not failures(oc)
    assert oc.unchecked() == opcheck.allowlist('pseg_nhwc_to_nchw')
    assert oc.census == {'pseg_nhwc_to_nchw': 2} and oc.checked == {'pseg_copy2d': 1}
    with pytest.raises(AssertionError):
        opcheck.allowlist('pseg_not_an_entry_point')
