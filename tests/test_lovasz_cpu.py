"""Lovasz-softmax loss without a GPU: the fp64 restatement of the contract of pseg_lovasz_softmax_fwd_bwd (include/pseg_amd.h)
that tests/test_lovasz_gpu.py holds the kernels to, checked here against an independent formulation (torch.autograd in
float64 over torch.sort(stable=True) and cumsum, with SUBTRACTED Jaccard differences), its edge cases, and the host
interface: header, prototypes, make_loss, train.py's --loss."""
import inspect

import numpy as np
import pytest
import torch


# ------------------------------------------------------------------ the contract, restated in numpy float64
def lovasz_softmax_ref(logits, target, ignore_index=-100):
    """logits [B,C,H,W] (any float), target [B,H,W] int -> (loss, dlogits [B,C,H,W] float64, info).
    Valid pixels: t != ignore_index and 0 <= t < C.  Per present class: errors |[t == c] - p_c| sorted descending, ties by
    ascending flat pixel index (stable argsort of -e over pixels in index order), closed-form differences of the Jaccard
    loss from the integer counts, mean over present classes; the gradient goes through e and the softmax."""
    x = np.asarray(logits, dtype=np.float64)
    B, C, H, W = x.shape
    t = np.asarray(target).reshape(-1).astype(np.int64)
    z = x.transpose(0, 2, 3, 1).reshape(-1, C)
    in_range = (t >= 0) & (t < C)
    valid = (t != ignore_index) & in_range
    info = {'n_valid': int(valid.sum()), 'n_bad': int(((t != ignore_index) & ~in_range).sum())}
    zv, tv = z[valid], t[valid]
    n = len(tv)
    ex = np.exp(zv - zv.max(1, keepdims=True)) if n else zv
    p = ex / ex.sum(1, keepdims=True) if n else zv
    present = [c for c in range(C) if (tv == c).any()]
    info['n_present'] = len(present)
    info['p'], info['tv'], info['valid'], info['present'] = p, tv, valid, present
    loss, dp = 0.0, np.zeros_like(p)
    for c in present:
        fg = tv == c
        e = np.abs(fg.astype(np.float64) - p[:, c])
        order = np.argsort(-e, kind='stable')
        fgs = fg[order].astype(np.int64)
        P = int(fgs.sum())
        F = np.cumsum(fgs)
        k = np.arange(n, dtype=np.int64)
        I, U = P - F, P + (k + 1 - F)
        d = np.where(fgs == 1, 1.0 / U, I / (np.maximum(U - 1, 1).astype(np.float64) * U))
        loss += float((e[order] * d).sum())
        g = np.empty(n)
        g[order] = d
        dp[:, c] = np.where(fg, -g, g) / len(present)
    if present:
        loss /= len(present)
    dz = np.zeros_like(z)
    if n:
        dz[valid] = p * (dp - (dp * p).sum(1, keepdims=True))
    return loss, dz.reshape(B, H, W, C).transpose(0, 3, 1, 2).copy(), info


def near_opposite_label(info, eps=1e-6):
    """Valid pixels (bool over the valid ones) that, in some present class, have an fp64 error within eps of the error of a
    pixel of the opposite label: the only ones whose rank an fp32 evaluation may legitimately swap visibly."""
    p, tv = info['p'], info['tv']
    out = np.zeros(len(tv), dtype=bool)
    for c in info['present']:
        fg = tv == c
        e = np.abs(fg.astype(np.float64) - p[:, c])
        for a, b in ((fg, ~fg), (~fg, fg)):
            if not a.any() or not b.any():
                continue
            other = np.sort(e[b])
            pos = np.searchsorted(other, e[a])
            lo = other[np.clip(pos - 1, 0, len(other) - 1)]
            hi = other[np.clip(pos, 0, len(other) - 1)]
            out[np.flatnonzero(a)] |= np.minimum(np.abs(e[a] - lo), np.abs(e[a] - hi)) <= eps
    return out


def make_case(B, C, H, W, std, seed, ignore_frac=0.1, ignore_index=-100):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, C, H, W, generator=g, dtype=torch.float64) * std
    target = torch.randint(0, C, (B, H, W), generator=g)
    target[torch.rand(B, H, W, generator=g) < ignore_frac] = ignore_index
    return logits.float(), target


# ------------------------------------------------------------------ the independent formulation
def lovasz_softmax_torch64(logits, target, ignore_index=-100):
    x = logits.detach().double().requires_grad_(True)
    C = x.shape[1]
    probs = torch.softmax(x, 1).permute(0, 2, 3, 1).reshape(-1, C)
    t = target.reshape(-1)
    keep = (t != ignore_index) & (t >= 0) & (t < C)
    probs, t = probs[keep], t[keep]
    losses = []
    for c in range(C):
        fg = (t == c).double()
        if fg.sum() == 0:
            continue
        err, perm = torch.sort((fg - probs[:, c]).abs(), descending=True, stable=True)
        fgs = fg[perm]
        inter = fgs.sum() - fgs.cumsum(0)
        union = fgs.sum() + (1 - fgs).cumsum(0)
        jac = 1 - inter / union
        losses.append((err * torch.diff(jac, prepend=jac.new_zeros(1))).sum())
    if not losses:
        return 0.0, torch.zeros_like(x).numpy()
    loss = torch.stack(losses).mean()
    loss.backward()
    return loss.item(), x.grad.numpy()


@pytest.mark.parametrize('shape,std', [((2, 5, 24, 40), 2.0), ((3, 21, 17, 23), 3.0)])
def test_restatement_matches_the_independent_formulation(shape, std):
    logits, target = make_case(*shape, std, seed=0)
    loss, grad, info = lovasz_softmax_ref(logits, target)
    loss_t, grad_t = lovasz_softmax_torch64(logits, target)
    print('loss %.15f vs %.15f, max |dgrad| %.3e' % (loss, loss_t, np.abs(grad - grad_t).max()))
    assert 0 < loss <= 1 and info['n_present'] == shape[1]
    assert abs(loss - loss_t) <= 1e-12
    assert np.abs(grad - grad_t).max() <= 1e-12
    assert (grad.transpose(0, 2, 3, 1)[target.numpy() == -100] == 0).all()


def test_share_of_pixels_near_an_opposite_label_is_small():
    """What the GPU gradient test leaves out stays far inside its 1 % bound, in the fp64 reference alone."""
    for shape, std in (((2, 5, 24, 40), 2.0), ((3, 21, 17, 23), 3.0)):
        _, _, info = lovasz_softmax_ref(*make_case(*shape, std, seed=0))
        share = near_opposite_label(info).mean()
        print(shape, 'share left out %.4f' % share)
        assert share <= 0.01


# ------------------------------------------------------------------ edge cases of the contract
def test_all_pixels_ignored():
    logits, target = make_case(2, 4, 6, 7, 2.0, seed=1)
    target[:] = -100
    loss, grad, info = lovasz_softmax_ref(logits, target)
    assert loss == 0.0 and not grad.any() and info['n_valid'] == 0 and info['n_present'] == 0
    loss_t, grad_t = lovasz_softmax_torch64(logits, target)
    assert loss_t == 0.0 and not grad_t.any()


def test_single_present_class():
    logits, target = make_case(2, 4, 6, 7, 2.0, seed=2, ignore_frac=0.2)
    target[target >= 0] = 2
    loss, grad, info = lovasz_softmax_ref(logits, target)
    loss_t, grad_t = lovasz_softmax_torch64(logits, target)
    # every valid pixel is foreground: the differences are 1 / P each, so the loss is the mean error of class 2
    assert info['n_present'] == 1 and abs(loss - (1 - info['p'][:, 2]).mean()) <= 1e-14
    assert abs(loss - loss_t) <= 1e-12 and np.abs(grad - grad_t).max() <= 1e-12


def test_absent_class_adds_nothing():
    logits, target = make_case(2, 5, 9, 11, 2.0, seed=3)
    target[target == 3] = 1
    loss, grad, info = lovasz_softmax_ref(logits, target)
    loss_t, grad_t = lovasz_softmax_torch64(logits, target)
    assert info['n_present'] == 4 and 3 not in info['present']
    assert abs(loss - loss_t) <= 1e-12 and np.abs(grad - grad_t).max() <= 1e-12


def test_out_of_range_labels_are_counted_and_ignored():
    logits, target = make_case(2, 5, 9, 11, 2.0, seed=4)
    bad = target.clone()
    flat = bad.view(-1)
    flat[3], flat[50], flat[77] = 5, -1, 1000
    as_ignored = bad.clone()
    as_ignored.view(-1)[[3, 50, 77]] = -100
    loss, grad, info = lovasz_softmax_ref(logits, bad)
    loss_i, grad_i, info_i = lovasz_softmax_ref(logits, as_ignored)
    assert info['n_bad'] == 3 and info_i['n_bad'] == 0 and info['n_valid'] == info_i['n_valid']
    assert loss == loss_i and np.array_equal(grad, grad_i)


def test_ties_are_ordered_by_pixel_index():
    """Constant logits: every error of a class is one of two values, the order inside each is the pixel order, and the
    gradient differs from pixel to pixel only through that order."""
    logits = torch.zeros(1, 2, 1, 6)
    target = torch.tensor([[[0, 1, 0, 1, 1, 0]]])
    loss, grad, _ = lovasz_softmax_ref(logits, target)
    loss_t, grad_t = lovasz_softmax_torch64(logits, target)
    assert abs(loss - loss_t) <= 1e-15 and np.abs(grad - grad_t).max() <= 1e-15
    # class 0, all errors 0.5, order = pixel order 0..5 with labels f b f b b f, P = 3:
    # U = 3 4 4 5 6 6, I = 2 2 1 1 1 0 -> differences 1/3, 2/12, 1/4, 1/20, 1/30, 1/6 (they sum to 1)
    d = np.array([1 / 3, 2 / 12, 1 / 4, 1 / 20, 1 / 30, 1 / 6])
    assert abs(d.sum() - 1) < 1e-15 and abs(loss - 0.5) <= 1e-15


# ------------------------------------------------------------------ interface
def test_header_declares_the_entry_points():
    from pytorch_segmentation_amd import _lib
    protos = _lib.parse_header()
    assert _lib.abi_version_of_header() == 14
    rt, args, names = protos['pseg_lovasz_softmax_fwd_bwd']
    assert names == ['logits', 'target', 'B', 'C', 'HW', 'ignore_index', 'dlogits', 'out', 'workspace', 'workspace_bytes',
                     'stream']
    assert protos['pseg_lovasz_workspace_bytes'][2] == ['B', 'C', 'HW']
    # same argument types as the cross-entropy call it sits beside
    assert args == protos['pseg_ce_fwd_bwd'][1]


def test_library_exports_the_entry_points_and_sizes_the_workspace():
    from pytorch_segmentation_amd import _lib
    from pytorch_segmentation_amd.csrc import build as csrc_build
    csrc_build.build(verbose=False)
    assert {'pseg_lovasz_softmax_fwd_bwd', 'pseg_lovasz_workspace_bytes'} <= set(_lib.prototypes())
    small = _lib.query('pseg_lovasz_workspace_bytes', 2, 5, 24 * 40)
    assert small >= 16 * 5 * 2 * 24 * 40
    # the headline shape is processed in class groups of at most 8: far below 16 bytes per class and pixel, and four times
    # the classes still fit the same budget
    head = _lib.query('pseg_lovasz_workspace_bytes', 16, 21, 512 * 512)
    assert 16 * 7 * (16 << 18) <= head < 16 * 9 * (16 << 18)
    assert _lib.query('pseg_lovasz_workspace_bytes', 16, 84, 512 * 512) < 16 * 9 * (16 << 18)
    # operands above 2 GiB are refused: no size, and the call says why before anything is launched
    assert _lib.query('pseg_lovasz_workspace_bytes', 64, 21, 1024 * 1024) == 0
    A = 0x7f0000000000
    with pytest.raises(_lib.PsegError, match='2 GiB'):
        _lib.call('pseg_lovasz_softmax_fwd_bwd', A, A, 64, 21, 1024 * 1024, -100, A, A, A, 1 << 40, None)
    with pytest.raises(_lib.PsegError, match='workspace too small'):
        _lib.call('pseg_lovasz_softmax_fwd_bwd', A, A, 2, 5, 960, -100, A, A, A, small - 1, None)


def test_make_loss_names():
    from pytorch_segmentation_amd.utils import compute_loss, loss, make_loss
    assert make_loss('ce') is compute_loss
    assert make_loss('lovasz') is not compute_loss and make_loss('ce+lovasz') is not make_loss('lovasz')
    for name in ('lovasz', 'ce+lovasz'):
        assert list(inspect.signature(make_loss(name)).parameters) == ['outputs', 'targets', 'model']
    with pytest.raises(ValueError, match='unknown loss'):
        make_loss('dice')
    assert list(inspect.signature(loss.lovasz_softmax_loss).parameters) == ['outputs', 'targets', 'ignore_index']
    with pytest.raises(RuntimeError, match='HIP path only'):
        make_loss('lovasz')(torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64))


def test_train_loss_flag_and_signature():
    import train
    from pytorch_segmentation_amd.utils import compute_loss
    ap = train.build_parser()
    assert ap.parse_args(['data/x']).loss == 'ce'
    assert ap.parse_args(['data/x', '--loss', 'lovasz']).loss == 'lovasz'
    assert ap.parse_args(['data/x', '--loss', 'ce+lovasz']).loss == 'ce+lovasz'
    with pytest.raises(SystemExit):
        ap.parse_args(['data/x', '--loss', 'dice'])
    assert train.LOSS_FN is compute_loss
    names = list(inspect.signature(train.train).parameters)
    assert names == ['data_dir', 'epochs', 'img_size', 'batch_size', 'accumulate', 'lr', 'adam', 'resume', 'weights',
                     'num_workers', 'multi_scale', 'rect', 'mixed_precision', 'notest', 'nosave', 'model_name', 'augment']
