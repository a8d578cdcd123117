"""pseg_ce_opts_binned_fwd_bwd (csrc/ce_opts.hip) and the boundary-weighted cross-entropy above it against the fp64
restatement in tests/ce_binned_ref.py, with the bins from the device's own ops.label_depth.

Counts, n_kept and the kept mask equal the restatement's exactly (tests/test_ce_boundary_cpu.py::test_case_conditions is
what allows that: around tau the per-pixel values are at least 1e-4 apart, relative).  Loss, gradient and tau: the bounds
tests/test_ce_opts_gpu.py holds this kernel family to -- loss 1e-5 relative, gradient max|d - d64| / max|d64| < 1e-4, tau
1e-5 relative.  Measured on an MI355X over the 40 parity cases: loss at most 8.8e-8, gradient 5.3e-7, tau 2.8e-7
(profiles/EXPERIMENTS.md section 25).  With a table of ones every output equals ops.ce_opts_fwd_bwd's bit for bit."""
import math

import numpy as np
import pytest
import torch

import ce_binned_ref as R

pytestmark = pytest.mark.gpu

LOSS_RTOL = 1e-5      # tests/test_ce_opts_gpu.py
GRAD_TOL = 1e-4       # on rel() below
TAU_RTOL = 1e-5


def rel(a, b):
    """tests/test_ops_gpu.py's rel()"""
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def _table(values):
    from pytorch_segmentation_amd import ops
    return ops.bin_weight_table(np.asarray(values, dtype=np.float64), 'cuda')


def _depth(target, C):
    from pytorch_segmentation_amd import ops
    return ops.label_depth(target.cuda().contiguous(), C, R.D, edge=False)


def _run(logits, target, bins, table, w=None, eps=0.0, gamma=0.0, keep=1.0, want_grad=True, ignore_index=-100):
    """bins: uint8 device tensor (any storage offset); table: fp32 [256] device tensor"""
    from pytorch_segmentation_amd import ops
    wd = None if w is None else torch.as_tensor(np.asarray(w), dtype=torch.float32).cuda()
    out, dl = ops.ce_opts_binned_fwd_bwd(logits.cuda().contiguous(), target.cuda().contiguous(), bins, table, wd, eps, gamma, keep,
                                         want_grad=want_grad, ignore_index=ignore_index)
    torch.cuda.synchronize()
    return out.cpu(), (None if dl is None else dl.cpu())


def _plain(logits, target, w=None, eps=0.0, gamma=0.0, keep=1.0, want_grad=True):
    from pytorch_segmentation_amd import ops
    wd = None if w is None else torch.as_tensor(np.asarray(w), dtype=torch.float32).cuda()
    out, dl = ops.ce_opts_fwd_bwd(logits.cuda().contiguous(), target.cuda().contiguous(), wd, eps, gamma, keep, want_grad=want_grad)
    torch.cuda.synchronize()
    return out.cpu(), (None if dl is None else dl.cpu())


# ------------------------------------------------------------------ parity
@pytest.mark.parametrize('opt', list(R.OPTIONS))
@pytest.mark.parametrize('falloff', list(R.TABLES))
@pytest.mark.parametrize('name', list(R.SHAPES))
def test_parity_with_the_restatement(name, falloff, opt):
    logits, target, depth, w, table, ref = R.reference(name, falloff, opt)
    use_w, eps, gamma, keep = R.OPTIONS[opt]
    C = R.SHAPES[name][1]
    bins = _depth(target, C)
    np.testing.assert_array_equal(bins.cpu().numpy().astype(np.int64), depth)      # ops.label_depth's bytes are the reference's
    out, dl = _run(logits, target, bins, _table(table), w, eps, gamma, keep)
    info = ref.info
    mask = (dl != 0).any(1).numpy()
    g = rel(dl, ref.grad)
    lerr = abs(out[0].item() - ref.loss) / abs(ref.loss)
    terr = abs(out[4].item() - ref.tau) / abs(ref.tau) if keep != 1.0 else abs(out[4].item())
    print('%s %s %s: loss %.9f vs %.9f (rel %.3e), grad rel %.3e, tau %.9g vs %.9g (rel %.3e), n_kept %d vs %d, mask diff %d'
          % (name, falloff, opt, out[0].item(), ref.loss, lerr, g, out[4].item(), ref.tau, terr, int(out[3].item()), ref.n_kept,
             int((mask != info['kept']).sum())))
    assert out[1:4].tolist() == [info['n_valid'], info['n_bad'], ref.n_kept]
    assert np.array_equal(mask, info['kept'])
    assert terr <= TAU_RTOL
    assert abs(out[5].item() - ref.den) <= 1e-6 * ref.den
    assert lerr <= LOSS_RTOL
    assert g < GRAD_TOL
    assert torch.isfinite(dl).all()


# ------------------------------------------------------------------ bit identity
@pytest.mark.parametrize('name', list(R.SHAPES))
def test_table_of_ones_gives_the_unbinned_bits(name):
    """1.0f * x is exact: loss, counts, tau, divisor and every gradient element are pseg_ce_opts_fwd_bwd's.  Two binned calls
    give the same bits; want_grad=False gives the same loss bits."""
    logits, target, _ = R.make_case(name)
    C = R.SHAPES[name][1]
    bins = _depth(target, C)
    ones = _table(np.ones(256))
    for w, eps, gamma in ((None, 0.0, 0.0), (R.weights(C), R.EPS, 2.0)):
        for keep in (1.0, 0.25):
            a, da = _run(logits, target, bins, ones, w, eps, gamma, keep)
            b, db = _plain(logits, target, w, eps, gamma, keep)
            assert torch.equal(a, b) and torch.equal(da, db), (name, keep)
            assert a[3].item() > 0 and da.any()
    table = _table(R.weight_table(R.D, R.BOOST, 'gaussian'))
    for keep in (1.0, 0.25):
        a, da = _run(logits, target, bins, table, R.weights(C), R.EPS, 2.0, keep)
        b, db = _run(logits, target, bins, table, R.weights(C), R.EPS, 2.0, keep)
        assert torch.equal(a, b) and torch.equal(da, db)
        c, none = _run(logits, target, bins, table, R.weights(C), R.EPS, 2.0, keep, want_grad=False)
        assert none is None and torch.equal(c, a)


# ------------------------------------------------------------------ misaligned bins
@pytest.mark.parametrize('keep', [1.0, 0.25])
def test_misaligned_bins(keep):
    """pixel_bin as a slice starting at byte 1, 2 and 3 of a larger buffer, on the vector-path shape: the same bits as the
    aligned call.  The bytes around the slice are 255 and the table's entry 255 is huge, so a wrong offset would show."""
    name = '2x5x24x40'
    logits, target, _ = R.make_case(name)
    B, C, H, W, _ = R.SHAPES[name]
    bins = _depth(target, C)
    values = R.weight_table(R.D, R.BOOST, 'gaussian')
    values[255] = 1e6
    table = _table(values)
    assert bins.data_ptr() % 4 == 0
    want, dwant = _run(logits, target, bins, table, R.weights(C), R.EPS, 2.0, keep)
    assert torch.isfinite(want).all() and want[0].item() < 100
    n = B * H * W
    for off in (1, 2, 3):
        buf = torch.full((n + 16,), 255, dtype=torch.uint8, device='cuda')
        assert buf.data_ptr() % 4 == 0
        view = buf[off:off + n].view(B, H, W)
        view.copy_(bins)
        assert view.data_ptr() % 4 == off and view.is_contiguous()
        got, dgot = _run(logits, target, view, table, R.weights(C), R.EPS, 2.0, keep)
        assert torch.equal(got, want) and torch.equal(dgot, dwant), off
        assert (buf[:off] == 255).all() and (buf[off + n:] == 255).all()


# ------------------------------------------------------------------ edge cases
@pytest.mark.parametrize('keep', [1.0, 0.25])
def test_nothing_to_average(keep):
    logits, target, _ = R.make_case('3x21x17x23')
    C = 21
    bins = _depth(target, C)
    table = _table(R.weight_table(R.D, R.BOOST, 'gaussian'))
    out, dl = _run(logits, torch.full_like(target, -100), bins, table, R.weights(C), R.EPS, 2.0, keep)
    assert math.isnan(out[0].item()) and out[1:].tolist() == [0.0] * 5 and not dl.any()
    # a table that is zero on the only bin present: the pixels are counted, the divisor is zero
    seven = torch.full_like(bins, 7)
    zero7 = _table(np.where(np.arange(256) == 7, 0.0, 1.0))
    out, dl = _run(logits, target, seven, zero7, R.weights(C), R.EPS, 2.0, keep)
    n_valid = int(((target >= 0) & (target < C)).sum())
    assert math.isnan(out[0].item()) and out[1].item() == n_valid > 0 and out[5].item() == 0 and not dl.any()


@pytest.mark.parametrize('name', ['2x5x24x40', '1x40x9x11'])
def test_a_zero_weight_bin_among_others(name):
    """u = 0 on depth 2: those pixels stay valid (n_valid counts them) and their gradient rows are exactly zero; out-of-range
    labels are counted in out[2]"""
    logits, target, depth = R.make_case(name)
    C = R.SHAPES[name][1]
    values = R.weight_table(R.D, R.BOOST, 'gaussian')
    values[2] = 0.0
    bins = _depth(target, C)
    ref = R.ce_binned_ref(logits, target, depth, values.astype(np.float32).astype(np.float64), R.weights(C), R.EPS, 2.0, 1.0)
    out, dl = _run(logits, target, bins, _table(values), R.weights(C), R.EPS, 2.0, 1.0)
    valid = ref.info['valid'].reshape(depth.shape)
    assert out[1].item() == ref.info['n_valid'] == int(valid.sum()) and (valid & (depth == 2)).any()
    assert out[2].item() == ref.info['n_bad'] > 0
    rows = dl.permute(0, 2, 3, 1).numpy()
    assert not rows[depth == 2].any() and rows[valid & (depth != 2)].any(1).all()
    assert abs(out[0].item() - ref.loss) <= LOSS_RTOL * ref.loss and rel(dl, ref.grad) < GRAD_TOL


def test_wrapper_refusals():
    from pytorch_segmentation_amd import ops
    logits, target, _ = R.make_case('2x5x24x40')
    x, t = logits.cuda(), target.cuda()
    bins, table = _depth(target, 5), _table(np.ones(256))
    with pytest.raises(ValueError, match='come together'):
        ops.ce_opts_binned_fwd_bwd(x, t, bins, None)
    with pytest.raises(ValueError, match='come together'):
        ops.ce_opts_binned_fwd_bwd(x, t, None, table)
    with pytest.raises(AssertionError, match='pixel_bin'):
        ops.ce_opts_binned_fwd_bwd(x, t, bins.int(), table)
    with pytest.raises(AssertionError, match='pixel_bin'):
        ops.ce_opts_binned_fwd_bwd(x, t, bins.cpu(), table)
    with pytest.raises(AssertionError, match='bin_weight'):
        ops.ce_opts_binned_fwd_bwd(x, t, bins, table[:255])


# ------------------------------------------------------------------ through the public interface
def test_resize_path_fp16_logits_and_backward():
    """fp16 logits at half the target size: the loss is the restatement's on the library's own resized fp32 logits, the
    backward runs through _ResizeFn, and an incoming factor of 0.5 halves the gradient."""
    from pytorch_segmentation_amd.utils import boundary_weighted_cross_entropy_loss
    from pytorch_segmentation_amd.utils.loss import _ResizeFn
    _, target, depth = R.make_case('2x5x24x40')
    g = torch.Generator().manual_seed(6)
    small = (torch.randn(2, 5, 12, 20, generator=g) * 2).half()
    w = R.weights(5)
    x = small.cuda().requires_grad_(True)
    loss = boundary_weighted_cross_entropy_loss(x, target.cuda(), R.BOOST, boundary_width=R.D, class_weight=w,
                                                label_smoothing=R.EPS, focal_gamma=2.0)
    loss.backward()
    up = _ResizeFn.apply(small.float().cuda(), 24, 40)
    table = R.weight_table(R.D, R.BOOST, 'gaussian').astype(np.float32).astype(np.float64)
    ref = R.ce_binned_ref(up.cpu(), target, depth, table, w, R.EPS, 2.0, 1.0)
    print('loss %.9f vs %.9f' % (loss.item(), ref.loss))
    assert abs(loss.item() - ref.loss) <= LOSS_RTOL * ref.loss
    assert x.grad.dtype == torch.float16 and torch.isfinite(x.grad).all() and x.grad.any()
    # the gradient: the restatement's, taken back through the library's resize
    x32 = small.float().cuda().requires_grad_(True)
    _ResizeFn.apply(x32, 24, 40).backward(torch.from_numpy(ref.grad).float().cuda())
    # (bound: the kernel family's GRAD_TOL, plus the rounding of the result to fp16 -- 2^-11 relative, 2^-24 absolute)
    top = x32.grad.abs().max().item()
    assert (x.grad.float() - x32.grad).abs().max().item() <= (GRAD_TOL + 2.0 ** -11) * top + 2.0 ** -24
    y = small.cuda().requires_grad_(True)
    (0.5 * boundary_weighted_cross_entropy_loss(y, target.cuda(), R.BOOST, boundary_width=R.D, class_weight=w,
                                                label_smoothing=R.EPS, focal_gamma=2.0)).backward()
    # (halving is exact in fp32 and in fp16 above its subnormals: at most one fp16 step of the largest element apart)
    assert (y.grad.float() - 0.5 * x.grad.float()).abs().max().item() <= 2.0 ** -10 * x.grad.float().abs().max().item() + 2.0 ** -24
    assert y.grad.any()
    # the width from the ratio is the evaluation's rule
    from pytorch_segmentation_amd.utils import boundary_width
    assert boundary_width((24, 40), 0.065) == R.D
    by_ratio = boundary_weighted_cross_entropy_loss(small.cuda(), target.cuda(), R.BOOST, boundary_ratio=0.065, class_weight=w,
                                                    label_smoothing=R.EPS, focal_gamma=2.0)
    assert by_ratio.item() == loss.item()


def test_trainer_step_with_a_boundary_weighted_loss(tmp_path):
    """One Trainer epoch (fp32) of UNet at 2 x 3 x 64 x 64 with the boundary-weighted cross-entropy plus Tversky through the
    Trainer's custom-loss route.  The loss is finite and every parameter moves."""
    import os
    from torch.utils.data import DataLoader
    from pytorch_segmentation_amd.models import UNet
    from pytorch_segmentation_amd.utils import Fetcher, Trainer, make_loss
    from pytorch_segmentation_amd.utils.datasets import CocoInstance, make_synthetic_coco
    root = make_synthetic_coco(str(tmp_path / 'data'), n_train=2, n_val=0, n_classes=1)
    ds = CocoInstance(os.path.join(root, 'train.json'), img_size=[64, 64])
    fetcher = Fetcher(DataLoader(ds, batch_size=2, shuffle=False, num_workers=0, drop_last=True), ds.post_fetch_fn)
    torch.manual_seed(0)
    C = len(ds.classes)
    loss_fn = make_loss('ce+tversky', boundary_boost=1.0, boundary_width=2)
    tr = Trainer(UNet(C), fetcher, loss_fn=loss_fn, workdir=str(tmp_path / 'weights'), lr=1e-2)
    before = [p.detach().clone() for p in tr.model.parameters()]
    loss = tr.step()
    assert np.isfinite(loss) and loss > 0, loss
    moved = [not torch.equal(a, b.detach()) for a, b in zip(before, tr.model.parameters())]
    assert all(moved), '%d of %d parameters did not move' % (moved.count(False), len(moved))


# ------------------------------------------------------------------ the loss family's recorded bits
def test_loss_bits_match_recorded(golden_dir):
    """every make_loss configuration of tests/loss_bits.py at its five shapes, the resize and fp16 cases and the five direct
    ops.*_fwd_bwd calls give the loss bytes, the gradient bytes and the sequence of C entry points recorded in
    tests/golden/loss_bits.json from the code as it stood before the loss Functions, closures and kernel helpers were folded"""
    import json
    import os

    import loss_bits
    from optim_bits import compiler_line
    from pytorch_segmentation_amd import ops
    with open(os.path.join(golden_dir, 'loss_bits.json')) as f:
        rec = json.load(f)
    got = loss_bits.digests(ops)
    assert sorted(got) == sorted(rec['digests'])
    for name, fields in got.items():
        assert sorted(fields) == sorted(rec['digests'][name]), name
        for k, v in fields.items():
            assert v == rec['digests'][name][k], \
                'case %s, %s: %s, recorded %s (recorded from %s under "%s", installed "%s")' % (
                    name, k, v, rec['digests'][name][k], rec['commit'], rec['compiler'], compiler_line())
