"""pseg_class_sdist and pseg_surface_fwd_bwd (csrc/surface.hip) and their host wrappers against the numpy restatements of
their contracts in tests/surface_ref.py.

Distance map: exact equality, element for element.  Loss, on the same fp32 logits: counts exact, |loss - loss64| <=
2e-5 * max(1, max|phi|) (the loss is a mean of distances, so it is scaled by the case's largest one), every gradient element
within 2e-5 * max|dlogits64|, nothing left out -- 2e-5 is the project's per-call fp64 bound (README, Oracle paragraph).  The
measured maxima are printed by every case.

Measured on an MI355X (worst over all cases of test_loss_and_gradient and test_edge_cases): |loss - loss64| 1.9e-7, that is
9.9e-9 of max(1, max|phi|); gradient error 1.45e-6 of max|dlogits64|; no element of any distance map differs
(profiles/EXPERIMENTS.md section 28)."""
import numpy as np
import pytest
import torch

import surface_ref as S

pytestmark = pytest.mark.gpu

TOL = 2e-5


def _pattern(kind, H=64, W=200):
    t = torch.zeros(1, H, W, dtype=torch.int64)
    if kind == 'checkerboard':
        t[0] = (torch.arange(H)[:, None] + torch.arange(W)[None, :]) & 1
    elif kind == 'corner':
        t[0, H - 1, W - 1] = 1
    elif kind == 'uniform':
        t[:] = 1
    return t


#               C, labels
def _maps():
    return {'1x2x1x70': (2, S.make_labels(1, 2, 1, 70, seed=0)),                  # one row
            '1x3x70x1': (3, S.make_labels(1, 3, 70, 1, seed=0)),                  # one column
            '2x5x24x40': (5, S.make_labels(2, 5, 24, 40, seed=0)),                # aligned
            '3x21x17x23': (21, S.make_labels(3, 21, 17, 23, seed=0)),             # ragged, void outline, out of range, absent in one
            '1x2x97x300': (2, S.make_labels(1, 2, 97, 300, seed=0)),              # a row above 256 pixels, more rows than a wave
            '1x70x8x9': (70, S.make_labels(1, 70, 8, 9, seed=0)),                 # more classes than lanes
            '1x1024x4x4': (1024, S.make_labels(1, 1024, 4, 4, seed=0)),           # the class limit
            'checkerboard': (2, _pattern('checkerboard')),                        # every distance 1
            'corner': (2, _pattern('corner')),                                    # the longest search, the largest values
            'uniform': (2, _pattern('uniform'))}                                  # an image of one label: zeros


_MAPS, _SDIST = {}, {}


def _map(name):
    """(C, labels, int64 reference [B,C,H,W]): once per case, shared"""
    if not _MAPS:
        _MAPS.update(_maps())
    if name not in _SDIST:
        C, t = _MAPS[name]
        _SDIST[name] = S.sdist_separable(t.numpy(), C)
    return _MAPS[name] + (_SDIST[name],)


def _sdist(t, C):
    from pytorch_segmentation_amd import ops
    out = ops.class_sdist(t.cuda().contiguous(), C)
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize('name', ['1x2x1x70', '1x3x70x1', '2x5x24x40', '3x21x17x23', '1x2x97x300', '1x70x8x9', '1x1024x4x4',
                                  'checkerboard', 'corner', 'uniform'])
def test_distance_map_is_exact(name):
    C, t, want = _map(name)
    got = _sdist(t, C)
    assert got.dtype == torch.int32 and tuple(got.shape) == want.shape
    g = got.numpy().astype(np.int64)
    print('%s: max |sdist| %d, %d planes without a contour, %d differing elements'
          % (name, np.abs(want).max(), sum(not want[b, c].any() for b in range(want.shape[0]) for c in range(C)), (g != want).sum()))
    assert np.array_equal(g, want)
    if name == 'checkerboard':
        assert (np.abs(g) == 1).all()
    elif name == 'corner':
        assert g.max() == 63 ** 2 + 199 ** 2 and g[0, 1, 0, 0] == g.max() and g[0, 1, 63, 199] == -1
    elif name == 'uniform':
        assert not g.any()
    elif name == '3x21x17x23':
        c0 = t[0, 0, 0].item()
        assert g[0, c0].any() and not g[1, c0].any() and ((t < 0) | (t >= C)).any()
    if want.shape[2] * want.shape[3] <= 2000:
        assert np.array_equal(g, S.sdist_brute(t.numpy(), C))


def test_distance_map_is_bit_identical_and_leaves_its_input():
    for name in ('3x21x17x23', '1x2x97x300'):
        C, t, _ = _map(name)
        keep = t.clone()
        assert torch.equal(_sdist(t, C), _sdist(t, C)) and torch.equal(t, keep)


def test_distance_map_against_the_label_depth():
    """Where the Chebyshev depth of a pixel of class c is k <= d, the nearest pixel of another label is at Chebyshev distance
    k, so its Euclidean distance squared lies in [k^2, 2 k^2]"""
    from pytorch_segmentation_amd import ops
    d = 6
    for name in ('2x5x24x40', '3x21x17x23', '1x2x97x300'):
        C, t, _ = _map(name)
        depth = ops.label_depth(t.cuda(), C, d, edge=False).cpu().long()
        sd = _sdist(t, C).long()
        valid = (t >= 0) & (t < C)
        own = sd.gather(1, t.clamp(0, C - 1).unsqueeze(1)).squeeze(1)
        sel = valid & (depth <= d)
        k2 = depth[sel] ** 2
        assert sel.sum() > 50 and (k2 <= -own[sel]).all() and (-own[sel] <= 2 * k2).all()


def test_distance_map_refusals():
    from pytorch_segmentation_amd import _lib, ops
    t = _map('2x5x24x40')[1].cuda()
    with pytest.raises(AssertionError, match='int64'):
        ops.class_sdist(t.int(), 5)
    with pytest.raises(ValueError, match='class_sdist'):
        ops.class_sdist(t, 1025)
    with pytest.raises(RuntimeError, match='HIP path only'):
        ops.class_sdist(t.cpu(), 5)
    # H or W above 16384, made-up sizes with null pointers only: refused by the host-side checks, which look at the sizes
    # first; nothing is launched and there is no memory to touch
    for H, W in ((16385, 8), (8, 16385)):
        with pytest.raises(_lib.PsegError, match='pseg_class_sdist: H, W = %d, %d above 16384' % (H, W)):
            _lib.call('pseg_class_sdist', None, 1, H, W, 2, None, None, 0, None)
        assert _lib.query('pseg_class_sdist_workspace_bytes', 1, 2, H, W) == 0
    with pytest.raises(_lib.PsegError, match='pseg_class_sdist: .*null pointer'):
        _lib.call('pseg_class_sdist', None, 1, 8, 8, 2, None, None, 0, None)


# ------------------------------------------------------------------ the loss
#          B, C, H, W, std
CASES = {'2x5x24x40': (2, 5, 24, 40, 2.0),          # the aligned vector path
         '3x21x17x23': (3, 21, 17, 23, 3.0),        # HW = 391: ragged and odd
         '1x2x1x70': (1, 2, 1, 70, 2.0),            # two classes; less than one block
         '2x3x97x131': (2, 3, 97, 131, 2.0),        # 13 blocks per image: the cross-block partials; HW % 4 != 0
         '1x70x8x9': (1, 70, 8, 9, 2.0)}            # more classes than a wave has lanes
CLIPS = (0.0, 3.0)
_INPUT, _REF = {}, {}


def _case(name, clip=0.0):
    """(logits, target, loss64, grad64, info): inputs once per case, the reference once per (case, clip), shared"""
    if name not in _INPUT:
        _INPUT[name] = S.make_case(*CASES[name], seed=0)
    if (name, clip) not in _REF:
        sd = _REF[name, CLIPS[0]][2]['sdist'] if (name, CLIPS[0]) in _REF else None
        _REF[name, clip] = S.surface_ref(*_INPUT[name], clip, sdist=sd)
    return _INPUT[name] + _REF[name, clip]


def _run(logits, target, clip=0.0, want_grad=True, ignore_index=-100):
    from pytorch_segmentation_amd import ops
    x, t = logits.cuda().contiguous(), target.cuda().contiguous()
    sd = ops.class_sdist(t, x.shape[1])
    out, dl = ops.surface_fwd_bwd(x, t, sd, clip, want_grad=want_grad, ignore_index=ignore_index)
    torch.cuda.synchronize()
    return out.cpu(), None if dl is None else dl.cpu(), sd.cpu()


def _check(tag, out, dl, loss64, grad64, info):
    grad_err = np.abs(dl.double().numpy() - grad64).max()
    grad_max = np.abs(grad64).max()
    scale = max(1.0, info['phi_max'])
    print('%s: loss %.9f vs %.9f (diff %.3e = %.3e of max(1, max|phi| %.3f)); grad max err %.3e = %.3e of max|grad| %.3e'
          % (tag, out[0].item(), loss64, out[0].item() - loss64, abs(out[0].item() - loss64) / scale, info['phi_max'], grad_err,
             grad_err / max(grad_max, 1e-300), grad_max))
    assert out[1:].tolist() == [info['n_valid'], info['n_bad']]
    assert abs(out[0].item() - loss64) <= TOL * scale
    assert grad_err <= TOL * grad_max
    bad = ~torch.from_numpy(info['valid'])
    assert torch.isfinite(dl).all() and not dl.permute(0, 2, 3, 1)[bad].any()


@pytest.mark.parametrize('clip', CLIPS)
@pytest.mark.parametrize('name', list(CASES))
def test_loss_and_gradient(name, clip):
    logits, target, loss64, grad64, info = _case(name, clip)
    out, dl, sd = _run(logits, target, clip)
    assert info['n_bad'] > 0 and 0 < info['n_valid'] < target.numel() and grad64.any()
    assert np.array_equal(sd.numpy().astype(np.int64), info['sdist'])
    if clip:
        assert info['phi_max'] <= clip
    _check('%s clip %g' % (name, clip), out, dl, loss64, grad64, info)


def test_edge_cases():
    logits, target, _, _, _ = _case('3x21x17x23')
    # all ignored: [0, 0, 0] and a zero gradient
    out, dl, _ = _run(logits, torch.full_like(target, -100))
    assert out.tolist() == [0.0, 0.0, 0.0] and not dl.any()
    # another ignore_index: the void outline is now out of range and counted
    t = target.clone()
    t[t == -100] = 255
    ref = S.surface_ref(logits, t, 0.0, ignore_index=255)
    out, dl, _ = _run(logits, t, ignore_index=255)
    _check('ignore_index 255', out, dl, *ref)
    ref = S.surface_ref(logits, t, 0.0, ignore_index=-100)
    out, dl, _ = _run(logits, t, ignore_index=-100)
    assert out[2].item() == ref[2]['n_bad'] > 100
    _check('void counted as out of range', out, dl, *ref)


def test_without_gradient_and_determinism():
    for name, clip in (('2x3x97x131', 0.0), ('3x21x17x23', 3.0), ('2x5x24x40', 0.0)):
        logits, target, loss64, _, info = _case(name, clip)
        out, dl, _ = _run(logits, target, clip)
        out2, dl2, _ = _run(logits, target, clip)
        assert torch.equal(out, out2) and torch.equal(dl, dl2)                  # bit-identical
        out3, none, _ = _run(logits, target, clip, want_grad=False)
        assert none is None and torch.equal(out3, out)                          # the same bits without dlogits
        assert abs(out[0].item() - loss64) <= TOL * max(1.0, info['phi_max'])


def test_aliasing_gradient_is_refused():
    from pytorch_segmentation_amd import _lib, ops
    logits, target = (t.cuda() for t in _case('2x5x24x40')[:2])
    sd = ops.class_sdist(target, 5)
    need = _lib.query('pseg_surface_workspace_bytes', 2, 5, 24 * 40)
    ws = torch.zeros(need, dtype=torch.uint8, device='cuda')
    out = torch.full((3,), -7.0, device='cuda')
    keep = logits.clone()
    head = (logits.data_ptr(), target.data_ptr(), sd.data_ptr(), 2, 5, 24 * 40, -100, 0.0)
    with pytest.raises(_lib.PsegError, match='must not alias logits'):
        _lib.call('pseg_surface_fwd_bwd', *head, logits.data_ptr(), out.data_ptr(), ws.data_ptr(), need, None)
    with pytest.raises(_lib.PsegError, match='must not alias sdist'):
        _lib.call('pseg_surface_fwd_bwd', *head, sd.data_ptr(), out.data_ptr(), ws.data_ptr(), need, None)
    with pytest.raises(_lib.PsegError, match='workspace too small'):
        _lib.call('pseg_surface_fwd_bwd', *head, None, out.data_ptr(), ws.data_ptr(), need - 1, None)
    with pytest.raises(_lib.PsegError, match='clip'):
        _lib.call('pseg_surface_fwd_bwd', *head[:-1], -1.0, None, out.data_ptr(), ws.data_ptr(), need, None)
    torch.cuda.synchronize()
    assert (out == -7).all() and torch.equal(logits, keep) and not ws.any()      # nothing was launched


# ------------------------------------------------------------------ host wrappers
def test_autograd_wrapper_and_signed_distance():
    from pytorch_segmentation_amd.utils import signed_distance, surface_loss
    logits, target, loss64, _, info = _case('2x5x24x40', 3.0)
    out, dl, _ = _run(logits, target, 3.0)
    x = logits.cuda().requires_grad_(True)
    loss = surface_loss(x, target.cuda(), clip=3.0)
    loss.backward()
    assert loss.item() == out[0].item() and torch.equal(x.grad.cpu(), dl)
    x = logits.cuda().requires_grad_(True)
    (3 * surface_loss(x, target.cuda(), clip=3.0)).backward()
    assert torch.allclose(x.grad.cpu(), 3.0 * dl, rtol=1e-6, atol=0)
    with torch.no_grad():
        assert surface_loss(logits.cuda(), target.cuda(), clip=3.0).item() == out[0].item()
    for clip in CLIPS:
        phi = signed_distance(target.cuda(), 5, clip)
        assert phi.dtype == torch.float32 and phi.is_cuda and tuple(phi.shape) == (2, 5, 24, 40)
        want = S.phi(info['sdist'], clip)
        assert np.abs(phi.cpu().double().numpy() - want).max() <= 1e-6 * np.abs(want).max()


def test_sum_of_losses_callable_weight_and_resize():
    """'ce+surface' with surface_weight = 0.5 is compute_loss + 0.5 * surface_loss in value and gradient; a callable weight
    is read at every call; logits at half the target size go through the resize compute_loss takes."""
    from pytorch_segmentation_amd.utils import compute_loss, make_loss, surface_loss
    from pytorch_segmentation_amd.utils.loss import _ResizeFn
    logits, target = _case('2x5x24x40')[:2]
    res = {}
    for name, fn in (('ce', compute_loss), ('surface', surface_loss),
                     ('ce+surface', make_loss('ce+surface', surface_weight=0.5))):
        x = logits.cuda().requires_grad_(True)
        loss = fn(x, target.cuda())
        loss.backward()
        res[name] = (loss.item(), x.grad.cpu())
    # one fp32 multiplication by 0.5 (exact) and one fp32 addition, in value and per gradient element
    assert res['ce+surface'][0] == np.float32(res['ce'][0]) + np.float32(0.5) * np.float32(res['surface'][0])
    want = res['ce'][1] + 0.5 * res['surface'][1]
    assert (res['ce+surface'][1] - want).abs().max() <= 1e-6 * want.abs().max()
    # a schedule needs no rebuild
    weights = iter([0.5, 0.0])
    fn = make_loss('ce+surface', surface_weight=lambda: next(weights))
    with torch.no_grad():
        first, second = fn(logits.cuda(), target.cuda()).item(), fn(logits.cuda(), target.cuda()).item()
    assert first == res['ce+surface'][0] and second == res['ce'][0] and first != second
    # half-size logits: the loss of the library's own resized logits, the gradient taken back through the resize
    g = torch.Generator().manual_seed(6)
    small = torch.randn(2, 5, 12, 20, generator=g) * 2
    x = small.cuda().requires_grad_(True)
    loss = surface_loss(x, target.cuda())
    loss.backward()
    x2 = small.cuda().requires_grad_(True)
    up = _ResizeFn.apply(x2, 24, 40)
    out, dl, _ = _run(up.detach().cpu(), target)
    up.backward(dl.cuda())
    assert loss.item() == out[0].item() and torch.equal(x.grad.cpu(), x2.grad.cpu())
    ref = S.surface_ref(up.detach().cpu(), target)
    assert abs(out[0].item() - ref[0]) <= TOL * max(1.0, ref[2]['phi_max'])


def test_trainer_steps_with_the_tversky_surface_loss(tmp_path):
    """Two Trainer epochs of one batch with loss_fn=make_loss('tversky+surface') through the Trainer's custom-loss route:
    UNet, 64 x 64, batch 2, synthetic COCO data (the configuration of the Tversky test)."""
    import os
    from torch.utils.data import DataLoader
    from pytorch_segmentation_amd.models import UNet
    from pytorch_segmentation_amd.utils import Fetcher, Trainer, make_loss
    from pytorch_segmentation_amd.utils.datasets import CocoInstance, make_synthetic_coco
    root = make_synthetic_coco(str(tmp_path / 'data'), n_train=2, n_val=0, n_classes=1)
    ds = CocoInstance(os.path.join(root, 'train.json'), img_size=[64, 64])
    fetcher = Fetcher(DataLoader(ds, batch_size=2, shuffle=False, num_workers=0, drop_last=True), ds.post_fetch_fn)
    torch.manual_seed(0)
    tr = Trainer(UNet(len(ds.classes)), fetcher, loss_fn=make_loss('tversky+surface'), workdir=str(tmp_path / 'weights'), lr=1e-2)
    before = [p.detach().clone() for p in tr.model.parameters()]
    losses = [tr.step(), tr.step()]
    print('losses %s' % (losses,))
    assert all(np.isfinite(l) for l in losses) and tr.epoch == 2
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, tr.model.parameters()))
