"""Dice / Tversky / focal-Tversky loss without a GPU: the fp64 restatement of the contract of pseg_tversky_fwd_bwd
(tests/tversky_ref.py) that tests/test_tversky_gpu.py holds the kernels to, checked here against central finite differences
and against torch autograd over an independent float64 formulation, and the host interface: header, prototypes, host-side
refusals, make_loss names and options, train.py's flags."""
import inspect
import math

import numpy as np
import pytest
import torch

from tversky_ref import make_case, tversky_ref

#          alpha, beta, smooth, power, per_image, all_classes
OPTIONS = {'dice': (0.5, 0.5, 1.0, 1.0, False, False), 'tversky_0.3_0.7': (0.3, 0.7, 1.0, 1.0, False, False),
           'power_0.75': (0.5, 0.5, 1.0, 0.75, False, False), 'power_2': (0.5, 0.5, 1.0, 2.0, False, False),
           'per_image': (0.5, 0.5, 1.0, 1.0, True, False), 'all_classes': (0.5, 0.5, 1.0, 1.0, False, True),
           'smooth_0': (0.5, 0.5, 0.0, 1.0, False, False)}


# ------------------------------------------------------------------ the independent formulation
def tversky_torch64(logits, target, alpha, beta, smooth, power, per_image, all_classes, ignore_index=-100):
    """float64 autograd over masked one-hot tensors: TI from S - TP and n - TP, 1 - TI by subtraction"""
    x = logits.detach().double().requires_grad_(True)
    B, C = x.shape[:2]
    p = torch.softmax(x, 1)
    valid = (target != ignore_index) & (target >= 0) & (target < C)
    onehot = torch.zeros_like(p).scatter_(1, target.clamp(0, C - 1).unsqueeze(1), 1.0) * valid.unsqueeze(1)
    pm = p * valid.unsqueeze(1)
    dims = (2, 3) if per_image else (0, 2, 3)
    n, S, TP = onehot.sum(dims), pm.sum(dims), (pm * onehot).sum(dims)
    TI = (TP + smooth) / (TP + alpha * (S - TP) + beta * (n - TP) + smooth)
    term = ((1 - TI) ** power).reshape(-1, C)
    n, has = n.reshape(-1, C), valid.sum((1, 2) if per_image else (0, 1, 2)).reshape(-1) > 0
    counted = (torch.ones_like(n, dtype=torch.bool) if all_classes else n > 0) & has[:, None]
    groups = [term[g][counted[g]].mean() for g in range(term.shape[0]) if counted[g].any()]
    if not groups:
        return 0.0, torch.zeros_like(x).numpy()
    loss = torch.stack(groups).mean()
    loss.backward()
    return loss.item(), x.grad.numpy()


@pytest.mark.parametrize('name', list(OPTIONS))
def test_restatement_gradient_matches_central_differences(name):
    logits, target = make_case(2, 3, 4, 5, 2.0, seed=0)
    x = logits.double().numpy()
    loss, grad, info = tversky_ref(x, target, *OPTIONS[name])
    assert info['n_bad'] > 0 and 0 < info['n_valid'] < target.numel()
    h, worst = 1e-6, 0.0
    for idx in np.ndindex(*x.shape):
        xp, xm = x.copy(), x.copy()
        xp[idx] += h
        xm[idx] -= h
        fd = (tversky_ref(xp, target, *OPTIONS[name])[0] - tversky_ref(xm, target, *OPTIONS[name])[0]) / (2 * h)
        worst = max(worst, abs(fd - grad[idx]))
    print('%s: loss %.12f, max |fd - grad| %.3e, max |grad| %.3e' % (name, loss, worst, np.abs(grad).max()))
    assert worst <= 1e-8
    assert not grad.transpose(0, 2, 3, 1)[~info['valid']].any()


@pytest.mark.parametrize('name', list(OPTIONS))
@pytest.mark.parametrize('shape,std', [((2, 5, 24, 40), 2.0), ((3, 21, 17, 23), 3.0)])
def test_restatement_matches_the_independent_formulation(shape, std, name):
    logits, target = make_case(*shape, std, seed=0)
    loss, grad, info = tversky_ref(logits, target, *OPTIONS[name])
    loss_t, grad_t = tversky_torch64(logits, target, *OPTIONS[name])
    print('%s %s: loss %.15f vs %.15f, max |dgrad| %.3e' % (shape, name, loss, loss_t, np.abs(grad - grad_t).max()))
    assert 0 < loss < 1 and abs(loss - loss_t) <= 1e-12
    assert np.abs(grad - grad_t).max() <= 1e-12
    G = shape[0] if OPTIONS[name][4] else 1
    assert info['n_groups'] == G and info['n_terms'] == G * shape[1] and info['class_sums'].shape == (G, shape[1], 3)
    assert info['class_sums'][..., 0].sum() == info['n_valid']


def test_dice_term_in_closed_form():
    """alpha = beta = 0.5, power = 1, smooth = 0: the present-class term is 1 - 2 TP / (S + n)"""
    logits, target = make_case(2, 5, 9, 11, 2.0, seed=3)
    target[target == 3] = 1                          # class 3 absent
    loss, _, info = tversky_ref(logits, target, 0.5, 0.5, 0.0, 1.0)
    n, S, TP = info['class_sums'][0].T
    present = n > 0
    assert present.tolist() == [True, True, True, False, True] and info['n_terms'] == 4
    assert np.abs(info['terms'][0][present] - (1 - 2 * TP[present] / (S[present] + n[present]))).max() <= 1e-14
    assert np.isnan(info['terms'][0][3])
    assert abs(loss - (1 - 2 * TP[present] / (S[present] + n[present])).mean()) <= 1e-14


def test_edge_cases_of_the_contract():
    logits, target = make_case(3, 4, 6, 7, 2.0, seed=1)
    # nothing valid: loss 0, gradient 0, no group
    loss, grad, info = tversky_ref(logits, torch.full_like(target, -100))
    assert loss == 0.0 and not grad.any() and (info['n_valid'], info['n_terms'], info['n_groups']) == (0, 0, 0)
    # per image, one image ignored: that image is no group
    t = target.clone()
    t[1] = -100
    loss, grad, info = tversky_ref(logits, t, per_image=True)
    assert info['n_groups'] == 2 and not grad[1].any() and grad[0].any() and grad[2].any()
    assert abs(loss - tversky_torch64(logits, t, 0.5, 0.5, 1.0, 1.0, True, False)[0]) <= 1e-12
    # an absent class is counted only with all_classes (its term: everything the model puts there is a false positive)
    t = target.clone()
    t[t == 2] = 0
    present = tversky_ref(logits, t)[2]
    every = tversky_ref(logits, t, all_classes=True)[2]
    assert present['n_terms'] == 3 and every['n_terms'] == 4 and every['terms'][0][2] > 0
    # saturated logits on the labels, smooth = 0: TI = 1 exactly, the loss and (power < 1) the gradient are 0
    t = target.clone()
    t[t < 0] = 0
    t[t >= 4] = 0
    sat = torch.full((3, 4, 6, 7), -80.0).scatter_(1, t.unsqueeze(1), 80.0)
    loss, grad, _ = tversky_ref(sat.float(), t, 0.5, 0.5, 0.0, 0.75)
    assert loss == 0.0 and np.isfinite(grad).all() and not grad.any()


# ------------------------------------------------------------------ interface
def test_header_declares_the_entry_points():
    from pytorch_segmentation_amd import _lib
    protos = _lib.parse_header()
    assert _lib.abi_version_of_header() == 14
    assert protos['pseg_tversky_workspace_bytes'][2] == ['B', 'C', 'HW']
    assert protos['pseg_tversky_fwd_bwd'][2] == ['logits', 'target', 'B', 'C', 'HW', 'ignore_index', 'alpha', 'beta', 'smooth',
                                                 'power', 'per_image', 'all_classes', 'dlogits', 'out', 'class_sums',
                                                 'workspace', 'workspace_bytes', 'stream']
    # the cross-entropy call's arguments around the six options and class_sums
    ce = protos['pseg_ce_fwd_bwd'][1]
    import ctypes
    assert protos['pseg_tversky_fwd_bwd'][1] == ce[:6] + [ctypes.c_float] * 4 + [ctypes.c_int] * 2 + ce[6:8] + \
        [ctypes.c_void_p] + ce[8:]


@pytest.fixture(scope='module')
def lib():
    from pytorch_segmentation_amd import _lib
    from pytorch_segmentation_amd.csrc import build as csrc_build
    csrc_build.build(verbose=False)
    _lib.load()
    return _lib


def test_library_exports_the_entry_points_and_sizes_the_workspace(lib):
    assert {'pseg_tversky_fwd_bwd', 'pseg_tversky_workspace_bytes'} <= set(lib.prototypes())
    # 24 bytes per class and block of 1024 pixels, 40 per (image, class): small beside the logits (4 bytes per class and pixel)
    head = lib.query('pseg_tversky_workspace_bytes', 16, 21, 512 * 512)
    assert 24 * 21 * 16 * 256 <= head <= 24 * 21 * 16 * 256 + (1 << 16)
    assert 0 < lib.query('pseg_tversky_workspace_bytes', 1, 1024, 16) < (1 << 20)
    assert lib.query('pseg_tversky_workspace_bytes', 0, 21, 64) == 0
    assert lib.query('pseg_tversky_workspace_bytes', 1, 1025, 64) == 0
    assert lib.query('pseg_tversky_workspace_bytes', 64, 21, 1024 * 1024) == 0      # logits above 2 GiB
    rc = lib.load().pseg_tversky_fwd_bwd(None, None, 0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0, 0, None, None, None, None, 0, None)
    assert rc == -1 and lib.load().pseg_last_error().startswith(b'pseg_tversky_fwd_bwd:')


@pytest.mark.skipif(torch.cuda.is_available(), reason='uses made-up device addresses: host-side checks only')
def test_argument_refusals(lib):
    """Every refusal the header lists, by the host-side checks alone: the pointers are made-up addresses and nothing is
    dereferenced or launched."""
    A, A2, MIS = 0x7f0000000000, 0x7f0000100000, 0x7f0000000004
    need = lib.query('pseg_tversky_workspace_bytes', 2, 5, 960)
    assert need > 0

    def call(logits=A, target=A, B=2, C=5, HW=960, alpha=0.5, beta=0.5, smooth=1.0, power=1.0, dl=A2, out=A, sums=None, ws=A,
             nbytes=need):
        lib.call('pseg_tversky_fwd_bwd', logits, target, B, C, HW, -100, alpha, beta, smooth, power, 0, 0, dl, out, sums, ws,
                 nbytes, None)

    def refused(match, **kw):
        with pytest.raises(lib.PsegError, match='pseg_tversky_fwd_bwd: .*' + match):
            call(**kw)

    for name in ('logits', 'target', 'out', 'ws'):
        refused('null pointer', **{name: None})
    for name in ('B', 'C', 'HW'):
        refused('bad sizes', **{name: 0})
        refused('bad sizes', **{name: -1})
    refused('at most 1024 classes', C=1025, HW=16)
    refused('above 2 GiB', B=64, C=21, HW=1024 * 1024, nbytes=1 << 40)        # the logits
    refused('above 2 GiB', B=1, C=1, HW=1 << 28, nbytes=1 << 40)              # the targets: 2^28 * 8 bytes = 2 GiB
    refused('must not alias', dl=A)
    refused('workspace too small', nbytes=need - 1)
    refused('workspace too small', nbytes=0)
    refused('workspace must be 16-byte aligned', ws=MIS)
    refused('alpha and beta', alpha=-0.1)
    refused('alpha and beta', beta=-0.1)
    refused('alpha and beta', alpha=0.0, beta=0.0)
    refused('smooth', smooth=-1e-3)
    for power in (0.49, 4.01, 0.0, -1.0):
        refused('power', power=power)
    for name in ('alpha', 'beta', 'smooth', 'power'):
        for bad in (math.nan, math.inf, -math.inf):
            refused('must be finite', **{name: bad})


def test_make_loss_names_and_options():
    from pytorch_segmentation_amd import ops, utils
    from pytorch_segmentation_amd.utils import compute_loss, loss, make_loss
    # what was there stays what it was
    assert make_loss('ce') is compute_loss
    assert make_loss('lovasz') is loss._lovasz_loss_fn and make_loss('ce+lovasz') is loss._ce_lovasz_loss_fn
    with pytest.raises(ValueError, match='unknown loss'):
        make_loss('dice')
    with pytest.raises(ValueError, match='unknown loss'):
        make_loss('dice', tversky_alpha=0.3, bogus=1)             # the name is refused first
    with pytest.raises(TypeError, match='unknown cross-entropy option'):
        make_loss('tversky', alpha=0.3)
    with pytest.raises(TypeError, match='unknown cross-entropy option'):
        make_loss('ce', gamma=2.0)
    # the new names; an option left at its default is not an option
    assert make_loss('tversky') is loss.LOSSES['tversky'] and make_loss('ce+tversky') is loss.LOSSES['ce+tversky']
    assert make_loss('tversky') is not make_loss('ce+tversky') and make_loss('tversky') is not compute_loss
    defaults = dict(tversky_alpha=0.5, tversky_beta=0.5, tversky_smooth=1.0, tversky_power=1.0, tversky_per_image=False,
                    tversky_all_classes=False, tversky_weight=1.0)
    assert set(defaults) == set(loss.TVERSKY_OPTIONS)
    for name in ('ce', 'lovasz', 'ce+lovasz', 'tversky', 'ce+tversky'):
        assert make_loss(name, keep_ratio=1.0, **defaults) is make_loss(name)
    for opts in ({'tversky_alpha': 0.3, 'tversky_beta': 0.7}, {'tversky_smooth': 0.0}, {'tversky_power': 0.75},
                 {'tversky_per_image': True}, {'tversky_all_classes': True}, {'tversky_weight': 0.5}):
        for name in ('tversky', 'ce+tversky'):
            fn = make_loss(name, **opts)
            assert fn is not make_loss(name) and list(inspect.signature(fn).parameters) == ['outputs', 'targets', 'model']
        for name in ('ce', 'lovasz', 'ce+lovasz'):                # no Tversky term to configure
            with pytest.raises(ValueError, match='Tversky options'):
                make_loss(name, **opts)
    # cross-entropy options: refused on the plain losses, the cross-entropy term's on the sums
    with pytest.raises(ValueError, match='lovasz'):
        make_loss('lovasz', label_smoothing=0.1)
    with pytest.raises(ValueError, match='tversky'):
        make_loss('tversky', focal_gamma=2.0)
    for opts in ({'focal_gamma': 2.0}, {'class_weight': [1.0, 2.0]}, {'label_smoothing': 0.1, 'tversky_weight': 0.5}):
        fn = make_loss('ce+tversky', **opts)
        assert fn is not make_loss('ce+tversky') and list(inspect.signature(fn).parameters) == ['outputs', 'targets', 'model']
    # the public surface
    assert utils.tversky_loss is loss.tversky_loss and 'tversky_loss' in utils.__all__
    assert list(inspect.signature(loss.tversky_loss).parameters) == [
        'outputs', 'targets', 'alpha', 'beta', 'smooth', 'power', 'per_image', 'all_classes', 'ignore_index']
    sig = inspect.signature(ops.tversky_fwd_bwd)
    assert list(sig.parameters) == ['logits', 'target', 'alpha', 'beta', 'smooth', 'power', 'per_image', 'all_classes',
                                    'want_grad', 'ignore_index', 'want_sums']
    assert [p.default for p in sig.parameters.values()][2:] == [0.5, 0.5, 1.0, 1.0, False, False, True, -100, False]


def test_wrappers_refuse_cpu_tensors():
    from pytorch_segmentation_amd.utils import loss, make_loss
    cpu = torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64)
    for fn in (make_loss('tversky'), make_loss('ce+tversky'), make_loss('tversky', tversky_power=0.75),
               make_loss('ce+tversky', tversky_weight=0.5, focal_gamma=2.0), loss.tversky_loss):
        with pytest.raises(RuntimeError, match='HIP path only'):
            fn(*cpu)


def test_train_flags():
    import train
    from pytorch_segmentation_amd.utils import compute_loss, make_loss
    ap = train.build_parser()
    opt = ap.parse_args(['data/x'])
    assert (opt.tversky_alpha, opt.tversky_beta, opt.tversky_smooth, opt.tversky_power, opt.tversky_per_image,
            opt.tversky_all_classes, opt.tversky_weight) == (0.5, 0.5, 1.0, 1.0, False, False, 1.0)
    assert train.loss_from_options(opt) == (compute_loss, None) and train.LOSS_FN is compute_loss
    for name in ('lovasz', 'ce+lovasz', 'tversky', 'ce+tversky'):
        assert train.loss_from_options(ap.parse_args(['data/x', '--loss', name])) == (make_loss(name), None)
    with pytest.raises(SystemExit):
        ap.parse_args(['data/x', '--loss', 'dice'])
    opt = ap.parse_args(['data/x', '--loss', 'ce+tversky', '--tversky-alpha', '0.3', '--tversky-beta', '0.7', '--tversky-smooth',
                         '0', '--tversky-power', '0.75', '--tversky-per-image', '--tversky-all-classes', '--tversky-weight',
                         '0.5', '--class-weights', '1', '2', '--focal-gamma', '2'])
    assert (opt.tversky_alpha, opt.tversky_beta, opt.tversky_smooth, opt.tversky_power, opt.tversky_per_image,
            opt.tversky_all_classes, opt.tversky_weight) == (0.3, 0.7, 0.0, 0.75, True, True, 0.5)
    fn, w = train.loss_from_options(opt)
    assert fn is not make_loss('ce+tversky') and w == [1.0, 2.0]
    assert list(inspect.signature(fn).parameters) == ['outputs', 'targets', 'model']
    with pytest.raises(ValueError, match='Tversky options'):
        train.loss_from_options(ap.parse_args(['data/x', '--loss', 'ce', '--tversky-power', '2']))
    with pytest.raises(ValueError, match='tversky'):
        train.loss_from_options(ap.parse_args(['data/x', '--loss', 'tversky', '--label-smoothing', '0.1']))
    for flag in ('--tversky-alpha', '--tversky-weight', '--loss ce|lovasz|ce+lovasz|tversky|ce+tversky'):
        assert flag in train.__doc__
    names = list(inspect.signature(train.train).parameters)
    assert names == ['data_dir', 'epochs', 'img_size', 'batch_size', 'accumulate', 'lr', 'adam', 'resume', 'weights',
                     'num_workers', 'multi_scale', 'rect', 'mixed_precision', 'notest', 'nosave', 'model_name', 'augment']
