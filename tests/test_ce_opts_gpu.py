"""pseg_ce_opts_fwd_bwd (csrc/ce_opts.hip) and its host wrappers against the fp64 restatement of the contract in
tests/test_ce_opts_cpu.py.

Counts, n_kept and the kept mask equal the restatement's exactly (tests/test_ce_opts_cpu.py::test_tau_is_well_separated is
what allows that: around tau the per-pixel values are at least 1e-4 apart, relative).  tau: 1e-5 relative.  Loss and
gradient: the bounds tests/test_ops_gpu.py::test_cross_entropy holds this arithmetic to -- loss 1e-5 relative, gradient
max|d - d64| / max|d64| < 1e-4 -- for every option set, gamma = 2 included.  Measured on an MI355X over all comparisons of
this file: loss at most 8.6e-8, gradient 6.3e-7, tau 2.4e-7 (profiles/EXPERIMENTS.md section 10)."""
import math

import numpy as np
import pytest
import torch

import test_ce_opts_cpu as R
from test_lovasz_cpu import make_case

pytestmark = pytest.mark.gpu

LOSS_RTOL = 1e-5      # tests/test_ops_gpu.py::test_cross_entropy
GRAD_TOL = 1e-4       # TOL of tests/test_ops_gpu.py, on rel() below
TAU_RTOL = 1e-5

#            weights?, eps, gamma, keep
OPTIONS = {'w': (True, 0.0, 0.0, 1.0), 'eps': (False, R.EPS, 0.0, 1.0), 'w+eps': (True, R.EPS, 0.0, 1.0),
           'g2': (False, 0.0, 2.0, 1.0), 'g2+w+eps': (True, R.EPS, 2.0, 1.0),
           'g2,keep.25': (False, 0.0, 2.0, 0.25), 'g2,keep.75': (False, 0.0, 2.0, 0.75),
           'g2+w+eps,keep.25': (True, R.EPS, 2.0, 0.25), 'g2+w+eps,keep.75': (True, R.EPS, 2.0, 0.75),
           'w+eps,keep.0625': (True, R.EPS, 0.0, 0.0625)}
_REF = {}


def rel(a, b):
    """tests/test_ops_gpu.py's rel()"""
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def _case(name, opt):
    """(logits, target, w, reference), computed once per case and shared"""
    if (name, opt) not in _REF:
        B, C, H, W, std = R.SHAPES[name]
        use_w, eps, gamma, keep = OPTIONS[opt]
        logits, target = make_case(B, C, H, W, std, seed=R.case_seed(name, use_w, eps, gamma, keep))
        w = R.weights(C) if use_w else None
        _REF[(name, opt)] = (logits, target, w, R.ce_opts_ref(logits, target, w, eps, gamma, keep))
    return _REF[(name, opt)]


def _run(logits, target, w=None, eps=0.0, gamma=0.0, keep=1.0, want_grad=True, ignore_index=-100):
    from pytorch_segmentation_amd import ops
    wd = None if w is None else torch.as_tensor(np.asarray(w), dtype=torch.float32).cuda()
    out, dl = ops.ce_opts_fwd_bwd(logits.cuda().contiguous(), target.cuda().contiguous(), wd, eps, gamma, keep,
                                  want_grad=want_grad, ignore_index=ignore_index)
    torch.cuda.synchronize()
    return out.cpu(), (None if dl is None else dl.cpu())


def _check(out, dl, ref, keep, tag=''):
    """the whole comparison of one call with the restatement; figures are printed before they are asserted"""
    info = ref.info
    mask = (dl != 0).any(1).numpy()
    g = rel(dl, ref.grad)
    lerr = abs(out[0].item() - ref.loss) / abs(ref.loss)
    terr = abs(out[4].item() - ref.tau) / abs(ref.tau) if keep != 1.0 else abs(out[4].item())
    print('%s: loss %.9f vs %.9f (rel %.3e), grad rel %.3e, tau %.9g vs %.9g (rel %.3e), n_kept %d vs %d, mask diff %d'
          % (tag, out[0].item(), ref.loss, lerr, g, out[4].item(), ref.tau, terr, int(out[3].item()), ref.n_kept,
             int((mask != info['kept']).sum())))
    assert out[1:4].tolist() == [info['n_valid'], info['n_bad'], ref.n_kept]
    assert np.array_equal(mask, info['kept'])
    assert terr <= TAU_RTOL
    assert abs(out[5].item() - info['den']) <= 1e-6 * info['den']
    assert lerr <= LOSS_RTOL
    assert g < GRAD_TOL
    assert torch.isfinite(dl).all()


@pytest.mark.parametrize('opt', list(OPTIONS))
@pytest.mark.parametrize('name', list(R.SHAPES))
def test_parity_with_the_restatement(name, opt):
    logits, target, w, ref = _case(name, opt)
    use_w, eps, gamma, keep = OPTIONS[opt]
    out, dl = _run(logits, target, w, eps, gamma, keep)
    _check(out, dl, ref, keep, '%s %s' % (name, opt))


# ------------------------------------------------------------------ equivalences
@pytest.mark.parametrize('name', list(R.SHAPES))
def test_all_options_off_is_the_plain_cross_entropy(name):
    from pytorch_segmentation_amd import ops
    B, C, H, W, std = R.SHAPES[name]
    logits, target = make_case(B, C, H, W, std, seed=0)
    out, dl = _run(logits, target)
    ce, dce = ops.ce_fwd_bwd(logits.cuda(), target.cuda())
    print('%s: loss %.9f vs %.9f, grad rel %.3e' % (name, out[0].item(), ce[0].item(), rel(dl, dce)))
    assert abs(out[0].item() - ce[0].item()) <= 1e-6 * abs(ce[0].item())
    assert rel(dl, dce) <= 1e-6
    assert out[1:4].tolist() == [ce[1].item(), ce[2].item(), ce[1].item()] and out[4].item() == 0


@pytest.mark.parametrize('name', list(R.SHAPES))
def test_no_selection_at_keep_one_loss_only_and_determinism(name):
    """keep_ratio == 1 never enters the selection: tau stays 0 and every valid pixel is kept.  want_grad=False gives the
    same loss bits (with and without selection); two identical calls give identical bits."""
    logits, target, w, ref = _case(name, 'g2+w+eps')
    out, dl = _run(logits, target, w, R.EPS, 2.0, 1.0)
    assert out[4].item() == 0 and out[3].item() == out[1].item() == ref.info['n_valid']
    out_w, _ = _run(logits, target, w)
    assert out_w[4].item() == 0 and out_w[3].item() == out_w[1].item()
    for keep in (1.0, 0.25):
        a, da = _run(logits, target, w, R.EPS, 2.0, keep)
        b, db = _run(logits, target, w, R.EPS, 2.0, keep)
        assert torch.equal(a, b) and torch.equal(da, db)
        c, none = _run(logits, target, w, R.EPS, 2.0, keep, want_grad=False)
        assert none is None and torch.equal(c, a)


# ------------------------------------------------------------------ ties
@pytest.mark.parametrize('C,std', [(5, 2.0), (21, 3.0), (40, 2.0)])
def test_ties_at_tau_share_one_fate(C, std):
    """One 1 x C x 6 x 10 block tiled 2 x 2 in space: every valid pixel has three exact copies, so every per-pixel value
    occurs four times (or a multiple), bit for bit.  k = ceil(0.25 n) need not be a multiple of 4: the copies of tau are all
    kept, n_kept is a multiple of 4 and at least k, and the result is the restatement's on the same tiled input."""
    logits, target = make_case(1, C, 6, 10, std, seed=0)
    logits, target = logits.repeat(1, 1, 2, 2), target.repeat(1, 2, 2)
    w = R.weights(C)
    for gamma in (0.0, 2.0):
        ref = R.ce_opts_ref(logits, target, w, R.EPS, gamma, 0.25)
        out, dl = _run(logits, target, w, R.EPS, gamma, 0.25)
        n_kept = int(out[3].item())
        assert ref.gap >= R.MIN_GAP      # (the condition of test_tau_is_well_separated, on this input)
        assert n_kept % 4 == 0 and n_kept >= ref.info['k'] and ref.n_kept % 4 == 0
        _check(out, dl, ref, 0.25, 'ties C=%d gamma=%g' % (C, gamma))
        mask = (dl != 0).any(1)[0]
        assert torch.equal(mask[:6, :10], mask[6:, :10]) and torch.equal(mask[:6, :10], mask[:6, 10:]) and \
            torch.equal(mask[:6, :10], mask[6:, 10:])


# ------------------------------------------------------------------ labels
@pytest.mark.parametrize('keep', [1.0, 0.25])
def test_out_of_range_labels_are_ignored_and_reported(keep):
    logits, target, w, _ = _case('2x5x24x40', 'g2+w+eps')
    bad = target.clone()
    bad.view(-1)[[3, 50, 77, 1000]] = torch.tensor([255, -7, 255, 5])
    as_ignored = bad.clone()
    as_ignored.view(-1)[[3, 50, 77, 1000]] = -100
    a, da = _run(logits, bad, w, R.EPS, 2.0, keep)
    b, db = _run(logits, as_ignored, w, R.EPS, 2.0, keep)
    assert a[2].item() == 4 and b[2].item() == 0
    assert torch.equal(a[[0, 1, 3, 4, 5]], b[[0, 1, 3, 4, 5]]) and torch.equal(da, db)
    ref = R.ce_opts_ref(logits, bad, w, R.EPS, 2.0, keep)
    assert ref.info['n_bad'] == 4
    assert abs(a[0].item() - ref.loss) <= LOSS_RTOL * ref.loss and a[3].item() == ref.n_kept
    # another ignore_index: the same pixels ignored under another name
    other = as_ignored.clone()
    other[other == -100] = 255
    c, dc = _run(logits, other, w, R.EPS, 2.0, keep, ignore_index=255)
    assert torch.equal(c, b) and torch.equal(dc, db)


@pytest.mark.parametrize('keep', [1.0, 0.25])
def test_every_pixel_ignored(keep):
    logits, target, w, _ = _case('3x21x17x23', 'g2+w+eps')
    out, dl = _run(logits, torch.full_like(target, -100), w, R.EPS, 2.0, keep)
    assert math.isnan(out[0].item()) and out[1:].tolist() == [0.0] * 5 and not dl.any()
    # every kept weight zero: the same answer, with the pixels counted
    one = target.clone()
    one[one >= 0] = 2
    w0 = w.copy()
    w0[2] = 0.0
    out, dl = _run(logits, one, w0, 0.0, 0.0, keep)
    assert math.isnan(out[0].item()) and out[1].item() == int((target >= 0).sum()) and out[5].item() == 0 and not dl.any()


# ------------------------------------------------------------------ through the public interface
def test_resize_path_fp16_logits_and_the_sum_with_lovasz():
    """Targets larger than the logits: the loss equals the direct call on the library's own resized logits, and the gradient
    is that call's gradient taken back through the resize, bit for bit.  fp16 logits (what -mp hands a custom loss) are
    accepted.  'ce+lovasz' with options is the sum of its parts."""
    from pytorch_segmentation_amd.utils import compute_loss, make_loss, weighted_cross_entropy_loss
    from pytorch_segmentation_amd.utils.loss import _ResizeFn
    g = torch.Generator().manual_seed(6)
    small = torch.randn(2, 5, 12, 20, generator=g) * 2
    _, target = make_case(2, 5, 24, 40, 2.0, seed=0)
    w = R.weights(5)
    x = small.cuda().requires_grad_(True)
    loss = weighted_cross_entropy_loss(x, target.cuda(), w, R.EPS, 2.0, 0.5)
    loss.backward()
    x2 = small.cuda().requires_grad_(True)
    up = _ResizeFn.apply(x2, 24, 40)
    out, dl = _run(up.detach(), target, w, R.EPS, 2.0, 0.5)
    up.backward(dl.cuda())
    assert loss.item() == out[0].item() and torch.equal(x.grad, x2.grad)
    ref = R.ce_opts_ref(up.detach().cpu(), target, w, R.EPS, 2.0, 0.5)
    assert abs(out[0].item() - ref.loss) <= LOSS_RTOL * ref.loss
    # fp16 logits: the loss of their fp32 values
    h = small.half().cuda().requires_grad_(True)
    loss_h = weighted_cross_entropy_loss(h, target.cuda(), w, R.EPS, 2.0, 0.5)
    loss_h.backward()
    loss_f = weighted_cross_entropy_loss(small.half().float().cuda(), target.cuda(), w, R.EPS, 2.0, 0.5)
    assert loss_h.item() == loss_f.item() and h.grad.dtype == torch.float16 and torch.isfinite(h.grad).all() and h.grad.any()
    # the sum: one fp32 addition of the two losses; the gradients are added before the resize's backward instead of after it
    res = {}
    for name, fn in (('ce', make_loss('ce', focal_gamma=2.0)), ('lovasz', make_loss('lovasz')),
                     ('ce+lovasz', make_loss('ce+lovasz', focal_gamma=2.0))):
        assert fn is not compute_loss
        x = small.cuda().requires_grad_(True)
        loss = fn(x, target.cuda(), None)
        loss.backward()
        res[name] = (loss.item(), x.grad.cpu())
    assert res['ce+lovasz'][0] == np.float32(res['ce'][0]) + np.float32(res['lovasz'][0])
    want = res['ce'][1] + res['lovasz'][1]
    assert (res['ce+lovasz'][1] - want).abs().max() <= 1e-6 * want.abs().max()
    ref = R.ce_opts_ref(up.detach().cpu(), target, None, 0.0, 2.0, 1.0)
    assert abs(res['ce'][0] - ref.loss) <= LOSS_RTOL * ref.loss
    with pytest.raises(ValueError, match='class_weight has 3 values for 5 classes'):
        weighted_cross_entropy_loss(small.cuda(), target.cuda(), [1.0, 2.0, 3.0])


def test_trainer_step_with_a_configured_loss(tmp_path):
    """One Trainer epoch (fp32) with class weights, the focal factor and hard-pixel selection through the Trainer's
    custom-loss route: UNet, 64 x 64, batch 2, synthetic COCO data.  The loss is finite and every parameter moves."""
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
    loss_fn = make_loss('ce', class_weight=[0.5 + c for c in range(C)], focal_gamma=2.0, keep_ratio=0.5)
    tr = Trainer(UNet(C), fetcher, loss_fn=loss_fn, workdir=str(tmp_path / 'weights'), lr=1e-2)
    before = [p.detach().clone() for p in tr.model.parameters()]
    loss = tr.step()
    assert np.isfinite(loss) and loss > 0, loss
    moved = [not torch.equal(a, b.detach()) for a, b in zip(before, tr.model.parameters())]
    assert all(moved), '%d of %d parameters did not move' % (moved.count(False), len(moved))
