"""pseg_tversky_fwd_bwd (csrc/tversky.hip) and its host wrappers against the fp64 restatement of the contract in
tests/tversky_ref.py, on the same fp32 logits.

Counts (out[1:], class_sums[..., 0]) are exact.  Loss: |loss - loss64| <= 2e-5; gradient: elementwise within
2e-5 * max|dlogits64|, nothing left out; class_sums S and TP within 2e-5 * max(1, value) -- 2e-5 is the project's per-call fp64
bound (README, Oracle paragraph).  The measured maxima are printed by every case.

Measured on an MI355X (worst over all cases of test_loss_gradient_and_sums and test_edge_cases): |loss - loss64| 2.9e-8,
gradient error 9.0e-7 of max|dlogits64|, class_sums 2.3e-7 (profiles/EXPERIMENTS.md section 23)."""
import numpy as np
import pytest
import torch

import tversky_ref as T

pytestmark = pytest.mark.gpu

TOL = 2e-5

#          B, C, H, W, std
CASES = {'2x5x24x40': (2, 5, 24, 40, 2.0),          # the aligned vector path
         '3x21x17x23': (3, 21, 17, 23, 3.0),        # HW = 391: ragged and odd; three images for per_image
         '1x2x1x70': (1, 2, 1, 70, 2.0),            # two classes; less than one block
         '2x3x97x131': (2, 3, 97, 131, 2.0),        # 13 blocks per image: the cross-block partials; HW % 4 != 0
         '1x70x8x9': (1, 70, 8, 9, 2.0),            # more classes than a wave has lanes
         '1x1024x4x4': (1, 1024, 4, 4, 2.0)}        # the class limit
#          alpha, beta, smooth, power, per_image, all_classes
OPTIONS = {'dice': (0.5, 0.5, 1.0, 1.0, False, False), 'tversky_0.3_0.7': (0.3, 0.7, 1.0, 1.0, False, False),
           'power_0.75': (0.5, 0.5, 1.0, 0.75, False, False), 'power_2': (0.5, 0.5, 1.0, 2.0, False, False),
           'per_image': (0.5, 0.5, 1.0, 1.0, True, False), 'all_classes': (0.5, 0.5, 1.0, 1.0, False, True),
           'smooth_0': (0.5, 0.5, 0.0, 1.0, False, False)}
RUNS = [(c, 'dice') for c in CASES] + [(c, o) for c in ('2x5x24x40', '3x21x17x23') for o in OPTIONS if o != 'dice']
_INPUT, _REF = {}, {}


def _case(name, opt='dice'):
    """(logits, target, loss64, grad64, info): inputs once per case, the reference once per (case, options), shared"""
    if name not in _INPUT:
        _INPUT[name] = T.make_case(*CASES[name], seed=0)
    if (name, opt) not in _REF:
        _REF[name, opt] = T.tversky_ref(*_INPUT[name], *OPTIONS[opt])
    return _INPUT[name] + _REF[name, opt]


def _run(logits, target, opts=OPTIONS['dice'], want_grad=True, ignore_index=-100, want_sums=True):
    from pytorch_segmentation_amd import ops
    res = ops.tversky_fwd_bwd(logits.cuda().contiguous(), target.cuda().contiguous(), *opts, want_grad=want_grad,
                              ignore_index=ignore_index, want_sums=want_sums)
    torch.cuda.synchronize()
    return tuple(None if r is None else r.cpu() for r in res)


def _check(tag, out, dl, sums, loss64, grad64, info, target):
    counts = [info['n_valid'], info['n_bad'], info['n_terms'], info['n_groups']]
    ref = info['class_sums']
    s = sums.numpy()
    grad_err = np.abs(dl.double().numpy() - grad64).max()
    grad_max = np.abs(grad64).max()
    sum_err = (np.abs(s[..., 1:] - ref[..., 1:]) / np.maximum(1.0, ref[..., 1:])).max()
    print('%s: loss %.9f vs %.9f (diff %.3e); grad max err %.3e = %.3e of max|grad| %.3e; sums rel err %.3e'
          % (tag, out[0].item(), loss64, out[0].item() - loss64, grad_err, grad_err / max(grad_max, 1e-300), grad_max, sum_err))
    assert out[1:].tolist() == counts
    assert np.array_equal(s[..., 0], ref[..., 0])
    assert abs(out[0].item() - loss64) <= TOL
    assert grad_err <= TOL * grad_max
    assert sum_err <= TOL
    bad = ~torch.from_numpy(info['valid'])
    assert torch.isfinite(dl).all() and not dl.permute(0, 2, 3, 1)[bad].any()


@pytest.mark.parametrize('name,opt', RUNS)
def test_loss_gradient_and_sums(name, opt):
    logits, target, loss64, grad64, info = _case(name, opt)
    out, dl, sums = _run(logits, target, OPTIONS[opt])
    assert info['n_bad'] > 0 and grad64.any()
    _check('%s %s' % (name, opt), out, dl, sums, loss64, grad64, info, target)


def test_edge_cases():
    logits, target = T.make_case(3, 5, 9, 11, 2.0, seed=4)
    # all ignored: loss 0, gradient 0, nothing counted
    out, dl, sums = _run(logits, torch.full_like(target, -100))
    assert out.tolist() == [0.0] * 5 and not dl.any() and not sums.any()
    # per image, one image fully ignored: it is no group
    t = target.clone()
    t[1] = -100
    opts = OPTIONS['per_image']
    ref = T.tversky_ref(logits, t, *opts)
    out, dl, sums = _run(logits, t, opts)
    assert ref[2]['n_groups'] == 2 and out[4].item() == 2 and not dl[1].any()
    _check('one image ignored', out, dl, sums, *ref, t)
    # a class absent from the batch: not counted when present-only, counted with all_classes; another ignore_index
    t = target.clone()
    t[t == 3] = 1
    t[t == -100] = 255
    for opt, n_terms in (('dice', 4), ('all_classes', 5), ('smooth_0', 4)):
        ref = T.tversky_ref(logits, t, *OPTIONS[opt], ignore_index=255)
        out, dl, sums = _run(logits, t, OPTIONS[opt], ignore_index=255)
        assert out[3].item() == n_terms and out[2].item() == ref[2]['n_bad'] > 0
        _check('absent class, %s' % opt, out, dl, sums, *ref, t)
    # saturated logits on the labels (p is exactly 0 / 1), smooth = 0, power = 0.75: TI = 1, loss 0, gradient finite and 0
    t = target.clone()
    t[(t < 0) | (t >= 5)] = 0
    sat = torch.full((3, 5, 9, 11), -80.0).scatter_(1, t.unsqueeze(1), 80.0)
    for per_image in (False, True):
        out, dl, sums = _run(sat, t, (0.5, 0.5, 0.0, 0.75, per_image, False))
        assert out[0].item() == 0.0 and out[1].item() == t.numel() and torch.isfinite(dl).all() and not dl.any()
        assert torch.equal(sums[..., 1], sums[..., 0]) and torch.equal(sums[..., 2], sums[..., 0])


def test_without_gradient_and_determinism():
    for name, opt in (('2x3x97x131', 'dice'), ('3x21x17x23', 'per_image'), ('2x5x24x40', 'power_0.75')):
        logits, target, loss64, _, _ = _case(name, opt)
        out, dl, sums = _run(logits, target, OPTIONS[opt])
        out2, dl2, sums2 = _run(logits, target, OPTIONS[opt])
        assert torch.equal(out, out2) and torch.equal(dl, dl2) and torch.equal(sums, sums2)      # bit-identical
        out3, none, sums3 = _run(logits, target, OPTIONS[opt], want_grad=False)
        out4, none4 = _run(logits, target, OPTIONS[opt], want_grad=False, want_sums=False)
        assert none is None and none4 is None and torch.equal(out3, out) and torch.equal(out4, out) and torch.equal(sums3, sums)
        assert abs(out[0].item() - loss64) <= TOL


def test_workspace_one_byte_short_is_refused():
    from pytorch_segmentation_amd import _lib
    logits, target = (t.cuda() for t in _case('2x5x24x40')[:2])
    need = _lib.query('pseg_tversky_workspace_bytes', 2, 5, 24 * 40)
    ws = torch.zeros(need, dtype=torch.uint8, device='cuda')
    out = torch.full((5,), -7.0, device='cuda')
    dl = torch.full_like(logits, -7.0)
    args = (logits.data_ptr(), target.data_ptr(), 2, 5, 24 * 40, -100, 0.5, 0.5, 1.0, 1.0, 0, 0, dl.data_ptr(), out.data_ptr(),
            None, ws.data_ptr())
    with pytest.raises(_lib.PsegError, match='workspace too small'):
        _lib.call('pseg_tversky_fwd_bwd', *args, need - 1, None)
    torch.cuda.synchronize()
    assert (out == -7).all() and (dl == -7).all() and not ws.any()      # nothing was launched
    _lib.call('pseg_tversky_fwd_bwd', *args, need, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert abs(out[0].item() - _case('2x5x24x40')[2]) <= TOL


# ------------------------------------------------------------------ host wrappers
def test_autograd_wrapper_matches_the_direct_call():
    from pytorch_segmentation_amd.utils import tversky_loss
    logits, target, loss64, _, _ = _case('2x5x24x40', 'tversky_0.3_0.7')
    out, dl = _run(logits, target, OPTIONS['tversky_0.3_0.7'], want_sums=False)
    x = logits.cuda().requires_grad_(True)
    loss = tversky_loss(x, target.cuda(), alpha=0.3, beta=0.7)
    (3 * loss).backward()
    assert loss.item() == out[0].item()
    assert torch.allclose(x.grad.cpu(), 3.0 * dl, rtol=1e-6, atol=0)
    with torch.no_grad():
        assert tversky_loss(logits.cuda(), target.cuda(), alpha=0.3, beta=0.7).item() == out[0].item()


def test_resize_path_and_sum_of_losses():
    """Targets larger than the logits: the logits are resized (bilinear, align_corners=True) exactly as compute_loss does,
    so the loss equals the direct call on the library's own resized logits and the gradient is that call's gradient taken
    back through the resize; 'ce+tversky' with tversky_weight = 0.5 is ce + 0.5 * tversky in loss and gradient."""
    import torch.nn.functional as F
    from pytorch_segmentation_amd.utils import compute_loss, make_loss
    from pytorch_segmentation_amd.utils.loss import _ResizeFn
    g = torch.Generator().manual_seed(6)
    small = torch.randn(2, 5, 12, 20, generator=g) * 2
    target = _case('2x5x24x40')[1]
    fns = {'ce': make_loss('ce'), 'tversky': make_loss('tversky'), 'ce+tversky': make_loss('ce+tversky', tversky_weight=0.5)}
    res = {}
    for name, fn in fns.items():
        x = small.cuda().requires_grad_(True)
        loss = fn(x, target.cuda(), None)
        loss.backward()
        res[name] = (loss.item(), x.grad.cpu())
    assert fns['ce'] is compute_loss
    # the same composition by hand, from the library's own pieces: bit-identical
    x = small.cuda().requires_grad_(True)
    up = _ResizeFn.apply(x, 24, 40)
    out, dl = _run(up.detach(), target, want_sums=False)
    up.backward(dl.cuda())
    assert res['tversky'][0] == out[0].item() and torch.equal(res['tversky'][1], x.grad.cpu())
    # and it is the resize compute_loss takes: against fp64 interpolation + the restatement.  The resize kernel (held to its
    # own bound in test_ops_gpu.py) leaves d = max|up - up64|; a probability moves by at most d / 2 when every logit moves by
    # at most d, TI_c is a quotient of sums of probabilities over a denominator that is at least the class's share of them,
    # so a term moves by at most about d and the mean of the terms with it: the kernel's 2e-5 + d
    up64 = F.interpolate(small.double(), size=(24, 40), mode='bilinear', align_corners=True)
    d = (up.detach().cpu().double() - up64).abs().max().item()
    loss64 = T.tversky_ref(up64, target)[0]
    print('resize: d = %.3e, loss %.9f vs %.9f' % (d, out[0].item(), loss64))
    assert d <= 1e-4
    assert abs(out[0].item() - loss64) <= TOL + d
    # the sum: one fp32 multiplication by 0.5 (exact) and one fp32 addition; the gradients are added before the resize's
    # backward instead of after it (linear, so equal up to fp32 rounding of sums of at most four products per element)
    assert res['ce+tversky'][0] == np.float32(res['ce'][0]) + np.float32(0.5) * np.float32(res['tversky'][0])
    want = res['ce'][1] + 0.5 * res['tversky'][1]
    assert (res['ce+tversky'][1] - want).abs().max() <= 1e-6 * want.abs().max()


@pytest.mark.parametrize('mixed_precision', [False, True])
def test_trainer_step_with_the_tversky_loss(tmp_path, mixed_precision):
    """One Trainer epoch with loss_fn=make_loss('tversky') through the Trainer's custom-loss route, fp32 and -mp (fp16
    logits reach the loss): UNet, 64 x 64, batch 2, synthetic COCO data.  The fp32 epoch is one batch.  The -mp epoch is
    eight: the dynamic loss scale starts at 65536 and the optimiser skips a step whose fp16 gradients overflow, halving the
    scale -- on this data the first three steps of a fresh UNet are skipped with this loss (and as many with a configured
    cross-entropy through the same route), so an epoch of one batch leaves the weights where they were by design."""
    import os
    from torch.utils.data import DataLoader
    from pytorch_segmentation_amd.models import UNet
    from pytorch_segmentation_amd.utils import Fetcher, Trainer, make_loss
    from pytorch_segmentation_amd.utils.datasets import CocoInstance, make_synthetic_coco
    root = make_synthetic_coco(str(tmp_path / 'data'), n_train=16 if mixed_precision else 2, n_val=0, n_classes=1)
    ds = CocoInstance(os.path.join(root, 'train.json'), img_size=[64, 64])
    fetcher = Fetcher(DataLoader(ds, batch_size=2, shuffle=False, num_workers=0, drop_last=True), ds.post_fetch_fn)
    torch.manual_seed(0)
    tr = Trainer(UNet(len(ds.classes)), fetcher, loss_fn=make_loss('tversky'), workdir=str(tmp_path / 'weights'), lr=1e-2,
                 mixed_precision=mixed_precision)
    before = [p.detach().clone() for p in tr.model.parameters()]
    loss = tr.step()
    print('mixed_precision=%s: loss %.6f, loss scale state %s' % (mixed_precision, loss, tr.loss_scale_state()))
    assert np.isfinite(loss) and 0 < loss <= 1, loss
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, tr.model.parameters()))
