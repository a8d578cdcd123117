"""pseg_lovasz_softmax_fwd_bwd (csrc/lovasz.hip) and its host wrappers against the fp64 restatement of the contract in
tests/test_lovasz_cpu.py.

Loss: |loss - loss64| <= 2e-6 (the loss lies in [0, 1]; the differences of the Jaccard loss have total variation 1 per class,
so an fp32 error of about 1e-7 in each error bounds the loss error near 1e-7; the margin covers the accumulation).
Gradient: elementwise, atol = 1e-5 * max|dlogits64|.  The fp32 and fp64 orders can differ only between near-equal errors;
a swap of two neighbours of the same label moves the gradient by O(1 / n^2), a swap of opposite labels is visible, so pixels
whose fp64 error is within 1e-6 of an opposite-label pixel's error in some class are left out -- at most 1 % of the valid
pixels, asserted -- and nothing else is."""
import numpy as np
import pytest
import torch

import test_lovasz_cpu as L

pytestmark = pytest.mark.gpu

LOSS_TOL = 2e-6
GRAD_RTOL = 1e-5

#          B, C, H, W, std         (2,3,97,131: 25414 pixels = 6.2 sort tiles of 4096, a multiple of no tile or vector size)
CASES = {'2x5x24x40': (2, 5, 24, 40, 2.0), '3x21x17x23': (3, 21, 17, 23, 3.0), '1x2x1x70': (1, 2, 1, 70, 2.0),
         '2x3x97x131': (2, 3, 97, 131, 2.0)}
_REF = {}


def _case(name):
    """(logits, target, loss64, grad64, info), the reference computed once per case and shared"""
    if name not in _REF:
        logits, target = L.make_case(*CASES[name], seed=0)
        _REF[name] = (logits, target) + L.lovasz_softmax_ref(logits, target)
    return _REF[name]


def _run(logits, target, want_grad=True, ignore_index=-100):
    from pytorch_segmentation_amd import ops
    out, dl = ops.lovasz_softmax_fwd_bwd(logits.cuda().contiguous(), target.cuda().contiguous(), want_grad=want_grad,
                                         ignore_index=ignore_index)
    torch.cuda.synchronize()
    return out.cpu(), (None if dl is None else dl.cpu())


def _check_grad(dl, grad64, info, leave_out=True):
    """elementwise against the restatement; returns the share of valid pixels left out"""
    B, C, H, W = grad64.shape
    keep = np.ones(B * H * W, dtype=bool)
    share = 0.0
    if leave_out:
        near = L.near_opposite_label(info)
        share = float(near.mean()) if len(near) else 0.0
        assert share <= 0.01, share
        keep[np.flatnonzero(info['valid'])[near]] = False
    err = np.abs(dl.double().numpy() - grad64).transpose(0, 2, 3, 1).reshape(-1, C)
    atol = GRAD_RTOL * np.abs(grad64).max()
    print('grad: max err %.3e (kept pixels) / %.3e (all), atol %.3e, left out %.4f'
          % (err[keep].max(), err.max(), atol, share))
    assert err[keep].max() <= atol
    return share


# the gradient is held to fp64 where the fp64 reference alone leaves out at most 1 % of the pixels.  At 2x3x97x131 (22.9 k
# valid pixels, mean spacing of the errors 4e-5) 6 % of the pixels have an opposite-label error within 1e-6, so random
# logits cannot be judged there: the gradient across several sort tiles is held, with nothing left out, by
# test_stated_tie_order on the same shape.
GRAD_CASES = ('2x5x24x40', '3x21x17x23', '1x2x1x70')


@pytest.mark.parametrize('name', list(CASES))
def test_loss_and_gradient(name):
    logits, target, loss64, grad64, info = _case(name)
    out, dl = _run(logits, target)
    print('%s: loss %.9f vs %.9f (diff %.3e)' % (name, out[0].item(), loss64, out[0].item() - loss64))
    assert out[1:].tolist() == [info['n_valid'], info['n_bad'], info['n_present']]
    assert abs(out[0].item() - loss64) <= LOSS_TOL
    if name in GRAD_CASES:
        _check_grad(dl, grad64, info)
    assert not dl.permute(0, 2, 3, 1)[target == -100].any() and torch.isfinite(dl).all()


def test_class_groups_give_the_same_bits(monkeypatch):
    """PSEG_LOVASZ_GROUP caps the classes sorted at a time (what the 512 MiB budget does at training sizes: 21 classes in
    three groups of 7): 21 classes in groups of 4 and of 1 give the loss and gradient of the single group."""
    logits, target, loss64, _, _ = _case('3x21x17x23')
    out, dl = _run(logits, target)
    for g in ('4', '1'):
        monkeypatch.setenv('PSEG_LOVASZ_GROUP', g)
        out_g, dl_g = _run(logits, target)
        assert torch.equal(out_g, out) and torch.equal(dl_g, dl)
    assert abs(out[0].item() - loss64) <= LOSS_TOL


def tie_case():
    """2x3x97x131 (6.2 sort tiles), rows in five bands of constant logits, labels mixed: every error of a class is one of
    ten values, at least 9e-4 apart, each shared by hundreds to thousands of pixels of both kinds."""
    B, C, H, W = 2, 3, 97, 131
    levels = torch.tensor([[0.25, -1.0, 0.5], [1.5, 0.0, -0.75], [-0.5, 2.0, 0.125], [0.0, 0.375, 3.0], [-2.0, -0.25, 1.0]])
    g = torch.Generator().manual_seed(5)
    logits = levels[torch.arange(H) % 5].t().reshape(1, C, H, 1).expand(B, C, H, W).contiguous()
    target = torch.randint(0, C, (B, H, W), generator=g)
    target[torch.rand(B, H, W, generator=g) < 0.1] = -100
    return logits, target


def test_stated_tie_order():
    """Logits constant over many pixels of mixed labels: exact ties in fp32, broken by ascending pixel index.  Nothing
    is left out of the comparison (and nothing would be: distinct errors are far apart)."""
    logits, target = tie_case()
    loss64, grad64, info = L.lovasz_softmax_ref(logits, target)
    out, dl = _run(logits, target)
    print('ties: loss %.9f vs %.9f' % (out[0].item(), loss64))
    assert abs(out[0].item() - loss64) <= LOSS_TOL
    _check_grad(dl, grad64, info, leave_out=False)
    # the order is visible: the tied pixels of one label do not all get the same gradient
    tied = dl[0, 0, 0::5][target[0, 0::5] == 0]
    assert tied.unique().numel() > 100


def test_edge_cases():
    logits, target = L.make_case(2, 5, 9, 11, 2.0, seed=4)
    # all ignored: loss 0, gradient 0, nothing present
    out, dl = _run(logits, torch.full_like(target, -100))
    assert out.tolist() == [0.0, 0.0, 0.0, 0.0] and not dl.any()
    # a single present class; a class without pixels; out-of-range labels counted and treated as ignored;
    # another ignore_index
    one = target.clone()
    one[one >= 0] = 2
    absent = target.clone()
    absent[absent == 3] = 1
    bad = target.clone()
    bad.view(-1)[[3, 50, 77]] = torch.tensor([5, -1, 1000])
    other = target.clone()
    other[other == -100] = 255
    for t, ign, n_bad in ((one, -100, 0), (absent, -100, 0), (bad, -100, 3), (other, 255, 0)):
        loss64, grad64, info = L.lovasz_softmax_ref(logits, t, ignore_index=ign)
        out, dl = _run(logits, t, ignore_index=ign)
        assert out[1:].tolist() == [info['n_valid'], n_bad, info['n_present']] and info['n_bad'] == n_bad
        assert abs(out[0].item() - loss64) <= LOSS_TOL
        _check_grad(dl, grad64, info)


def test_without_gradient_and_determinism():
    logits, target, loss64, _, _ = _case('2x3x97x131')
    out, dl = _run(logits, target)
    out2, dl2 = _run(logits, target)
    assert torch.equal(out, out2) and torch.equal(dl, dl2)            # bit-identical
    out3, none = _run(logits, target, want_grad=False)
    assert none is None and torch.equal(out3, out)


def test_workspace_one_byte_short_is_refused():
    from pytorch_segmentation_amd import _lib
    logits, target = (t.cuda() for t in L.make_case(2, 5, 24, 40, 2.0, seed=0))
    need = _lib.query('pseg_lovasz_workspace_bytes', 2, 5, 24 * 40)
    ws = torch.zeros(need, dtype=torch.uint8, device='cuda')
    out = torch.full((4,), -7.0, device='cuda')
    dl = torch.full_like(logits, -7.0)
    with pytest.raises(_lib.PsegError, match='workspace too small'):
        _lib.call('pseg_lovasz_softmax_fwd_bwd', logits.data_ptr(), target.data_ptr(), 2, 5, 24 * 40, -100, dl.data_ptr(),
                  out.data_ptr(), ws.data_ptr(), need - 1, None)
    torch.cuda.synchronize()
    assert (out == -7).all() and (dl == -7).all() and not ws.any()      # nothing was launched
    _lib.call('pseg_lovasz_softmax_fwd_bwd', logits.data_ptr(), target.data_ptr(), 2, 5, 24 * 40, -100, dl.data_ptr(),
              out.data_ptr(), ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert abs(out[0].item() - _case('2x5x24x40')[2]) <= LOSS_TOL


# ------------------------------------------------------------------ host wrappers
def test_autograd_wrapper_matches_the_direct_call():
    from pytorch_segmentation_amd.utils.loss import lovasz_softmax_loss
    logits, target, loss64, _, _ = _case('2x5x24x40')
    out, dl = _run(logits, target)
    x = logits.cuda().requires_grad_(True)
    loss = lovasz_softmax_loss(x, target.cuda())
    (loss * 3.0).backward()
    assert loss.item() == out[0].item()
    assert torch.allclose(x.grad.cpu(), 3.0 * dl, rtol=1e-6, atol=0)
    with torch.no_grad():
        assert lovasz_softmax_loss(logits.cuda(), target.cuda()).item() == out[0].item()


def test_resize_path_and_sum_of_losses():
    """Targets larger than the logits: the logits are resized (bilinear, align_corners=True) exactly as compute_loss does,
    so the loss equals the direct call on the library's own resized logits and the gradient is that call's gradient taken
    back through the resize; 'ce+lovasz' is the plain sum of the two losses and of their gradients."""
    import torch.nn.functional as F
    from pytorch_segmentation_amd.utils import compute_loss, make_loss
    from pytorch_segmentation_amd.utils.loss import _ResizeFn
    g = torch.Generator().manual_seed(6)
    small = torch.randn(2, 5, 12, 20, generator=g) * 2
    _, target = L.make_case(2, 5, 24, 40, 2.0, seed=0)
    res = {}
    for name in ('ce', 'lovasz', 'ce+lovasz'):
        x = small.cuda().requires_grad_(True)
        loss = make_loss(name)(x, target.cuda(), None)
        loss.backward()
        res[name] = (loss.item(), x.grad.cpu())
    assert make_loss('ce') is compute_loss
    # the same composition by hand, from the library's own pieces: bit-identical
    x = small.cuda().requires_grad_(True)
    up = _ResizeFn.apply(x, 24, 40)
    out, dl = _run(up.detach(), target)
    up.backward(dl.cuda())
    assert res['lovasz'][0] == out[0].item() and torch.equal(res['lovasz'][1], x.grad.cpu())
    # and it is the resize compute_loss takes: against fp64 interpolation.  The resize kernel (held to its own bound in
    # test_ops_gpu.py) leaves d = max|up - up64|; a probability moves by at most d / 2 when every logit moves by at most d
    # (|dp_c / dz_j| <= 1 / 4, two signs), and the loss is 1-Lipschitz in the largest error change: the kernel's 2e-6 + d
    up64 = F.interpolate(small.double(), size=(24, 40), mode='bilinear', align_corners=True)
    d = (up.detach().cpu().double() - up64).abs().max().item()
    loss64 = L.lovasz_softmax_ref(up64, target)[0]
    print('resize: d = %.3e, loss %.9f vs %.9f' % (d, out[0].item(), loss64))
    assert d <= 1e-4
    assert abs(out[0].item() - loss64) <= LOSS_TOL + d
    # the sum: one fp32 addition of the two losses; the gradients are added before the resize's backward instead of after
    # it (linear, so equal up to fp32 rounding of sums of at most four products per element)
    assert res['ce+lovasz'][0] == np.float32(res['ce'][0]) + np.float32(res['lovasz'][0])
    want = res['ce'][1] + res['lovasz'][1]
    assert (res['ce+lovasz'][1] - want).abs().max() <= 1e-6 * want.abs().max()


def test_trainer_step_with_the_lovasz_loss(tmp_path):
    """One Trainer epoch (fp32) with loss_fn=make_loss('lovasz') through the Trainer's custom-loss route: UNet, 64 x 64,
    batch 2, synthetic COCO data."""
    import os
    from torch.utils.data import DataLoader
    from pytorch_segmentation_amd.models import UNet
    from pytorch_segmentation_amd.utils import Fetcher, Trainer, make_loss
    from pytorch_segmentation_amd.utils.datasets import CocoInstance, make_synthetic_coco
    root = make_synthetic_coco(str(tmp_path / 'data'), n_train=2, n_val=0, n_classes=1)
    ds = CocoInstance(os.path.join(root, 'train.json'), img_size=[64, 64])
    fetcher = Fetcher(DataLoader(ds, batch_size=2, shuffle=False, num_workers=0, drop_last=True), ds.post_fetch_fn)
    torch.manual_seed(0)
    tr = Trainer(UNet(len(ds.classes)), fetcher, loss_fn=make_loss('lovasz'), workdir=str(tmp_path / 'weights'), lr=1e-2)
    before = [p.detach().clone() for p in tr.model.parameters()]
    loss = tr.step()
    assert np.isfinite(loss) and 0 < loss <= 1, loss
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, tr.model.parameters()))
