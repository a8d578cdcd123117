"""Class-weighted, label-smoothed, focal, hard-pixel cross-entropy without a GPU: the fp64 restatement of the contract of
pseg_ce_opts_fwd_bwd (include/pseg_amd.h) that tests/test_ce_opts_gpu.py holds the kernels to, checked here against
F.cross_entropy(weight=, label_smoothing=) and an independent float64 autograd formulation (torch.topk for the selection),
the condition on the inputs that lets the GPU test take the kept set from the restatement, the edge cases, and the host
interface: header, prototypes, host-side refusals, make_loss options, train.py's flags."""
import collections
import inspect
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_lovasz_cpu import make_case

#          B, C, H, W, std of the logits: vector loads C <= 8 | odd HW, C <= 24 | C <= 32 | generic
SHAPES = {'2x5x24x40': (2, 5, 24, 40, 2.0), '3x21x17x23': (3, 21, 17, 23, 3.0), '2x30x8x8': (2, 30, 8, 8, 2.0),
          '1x40x9x11': (1, 40, 9, 11, 2.0)}
EPS = 0.1
MIN_GAP = 1e-4

CeOptsRef = collections.namedtuple('CeOptsRef', 'loss grad n_kept tau gap info')


def weights(C):
    return np.linspace(0.25, 2.0, C)


# ------------------------------------------------------------------ the contract, restated in numpy float64
def ce_opts_ref(logits, target, w=None, eps=0.0, gamma=0.0, keep=1.0, ignore_index=-100):
    """logits [B,C,H,W], target [B,H,W] -> CeOptsRef(loss, dlogits [B,C,H,W] float64, n_kept, tau, gap, info).
    Valid pixels: t != ignore_index and 0 <= t < C.  Per valid pixel l = (1 - eps) w_t (-log p_t) + (eps / C) sum_c w_c
    (-log p_c), f = (1 - p_t)^gamma l with 1 - p_t the sum of the other classes' probabilities.  keep == 1: every valid pixel
    is kept (tau = 0); else k = clamp(ceil(float32(keep) * n_valid), 1, n_valid), tau = the k-th largest f, kept = f >= tau.
    loss = sum_kept f / sum_kept w_t (NaN when that divisor is 0, the gradient then all zeros); the gradient is that of
    the quotient with the kept set fixed.  gap: the relative distance from tau to the nearest different f."""
    x = np.asarray(logits, dtype=np.float64)
    B, C, H, W = x.shape
    t = np.asarray(target).reshape(-1).astype(np.int64)
    z = x.transpose(0, 2, 3, 1).reshape(-1, C)
    wv = np.ones(C) if w is None else np.asarray(w, dtype=np.float64)
    in_range = (t >= 0) & (t < C)
    valid = (t != ignore_index) & in_range
    n = int(valid.sum())
    info = {'n_valid': n, 'n_bad': int(((t != ignore_index) & ~in_range).sum()), 'valid': valid}
    zv, tv = z[valid], t[valid]
    rows = np.arange(n)
    zs = zv - zv.max(1, keepdims=True) if n else zv
    ex = np.exp(zs)
    s = ex.sum(1, keepdims=True) if n else ex
    p = ex / s if n else ex
    nlogp = np.log(s) - zs if n else ex                                  # -log p_c
    onehot = np.zeros_like(p)
    onehot[rows, tv] = 1.0
    wt = wv[tv]
    ell = (1 - eps) * wt * nlogp[rows, tv] + (eps / C) * (nlogp * wv).sum(1)
    q = (p * (1 - onehot)).sum(1)                                        # 1 - p_t from the other classes
    pt = p[rows, tv]
    m = q ** gamma if gamma != 0 else np.ones(n)
    f = m * ell
    tau, gap, k = 0.0, math.inf, n
    kept = np.ones(n, dtype=bool)
    if keep != 1.0 and n > 0:
        k = min(max(int(math.ceil(float(np.float32(keep)) * n)), 1), n)
        tau = float(np.sort(f)[::-1][k - 1])
        kept = f >= tau
        other = f[f != tau]
        gap = float(np.abs(other - tau).min() / abs(tau)) if len(other) and tau != 0 else math.inf
    den = float(wt[kept].sum())
    info.update(k=k, den=den, f=f, kept_valid=kept)
    kept_all = np.zeros(len(t), dtype=bool)
    kept_all[np.flatnonzero(valid)[kept]] = True
    info['kept'] = kept_all.reshape(B, H, W)
    dz = np.zeros_like(z)
    if den > 0:
        loss = float(f[kept].sum() / den)
        dl = (1 - eps) * wt[:, None] * (p - onehot) + (eps / C) * (p * wv.sum() - wv[None, :])
        dq = gamma * q ** (gamma - 1) if gamma != 0 else np.zeros(n)    # d m / d (1 - p_t)
        g = m[:, None] * dl - (ell * dq * pt)[:, None] * (onehot - p)
        g[~kept] = 0.0
        dz[valid] = g / den
    else:
        loss = math.nan
    return CeOptsRef(loss, dz.reshape(B, H, W, C).transpose(0, 3, 1, 2).copy(), int(kept.sum()), tau, gap, info)


# ------------------------------------------------------------------ the independent formulation
def ce_opts_torch64(logits, target, w=None, eps=0.0, gamma=0.0, keep=1.0, ignore_index=-100):
    """float64 autograd: F.cross_entropy(reduction='none') for l and for p_t, torch.topk on the detached per-pixel values"""
    x = logits.detach().double().requires_grad_(True)
    C = x.shape[1]
    t = target.clone()
    t[(t < 0) | (t >= C)] = ignore_index
    wt = None if w is None else torch.as_tensor(np.asarray(w), dtype=torch.float64)
    ell = F.cross_entropy(x, t, weight=wt, label_smoothing=eps, ignore_index=ignore_index, reduction='none')
    pt = torch.exp(-F.cross_entropy(x, t, ignore_index=ignore_index, reduction='none'))
    f = (1 - pt) ** gamma * ell if gamma != 0 else ell
    valid = t != ignore_index
    fv = f[valid]
    wv = torch.ones_like(fv) if wt is None else wt[t[valid]]
    kept = torch.ones_like(fv, dtype=torch.bool)
    if keep != 1.0:
        n = fv.numel()
        k = min(max(int(math.ceil(float(np.float32(keep)) * n)), 1), n)
        kept = fv.detach() >= torch.topk(fv.detach(), k).values[-1]
    loss = fv[kept].sum() / wv[kept].sum()
    loss.backward()
    return loss.item(), x.grad.numpy(), int(kept.sum())


@pytest.mark.parametrize('name', list(SHAPES))
def test_restatement_matches_torch_cross_entropy(name):
    B, C, H, W, std = SHAPES[name]
    logits, target = make_case(B, C, H, W, std, seed=0)
    ref = ce_opts_ref(logits, target, weights(C), EPS)
    x = logits.double().requires_grad_(True)
    loss = F.cross_entropy(x, target, weight=torch.from_numpy(weights(C)), label_smoothing=EPS)
    loss.backward()
    print('%s: loss %.15f vs %.15f, max |dgrad| %.3e' % (name, ref.loss, loss.item(), np.abs(ref.grad - x.grad.numpy()).max()))
    assert abs(ref.loss - loss.item()) <= 1e-12
    assert np.abs(ref.grad - x.grad.numpy()).max() <= 1e-12
    assert ref.n_kept == ref.info['n_valid'] == int((target != -100).sum()) and ref.tau == 0.0
    # nothing set: nn.CrossEntropyLoss()
    plain = ce_opts_ref(logits, target)
    assert abs(plain.loss - F.cross_entropy(logits.double(), target).item()) <= 1e-12


@pytest.mark.parametrize('keep', [1.0, 0.75, 0.25, 0.0625])
@pytest.mark.parametrize('name', list(SHAPES))
def test_restatement_matches_the_independent_formulation(name, keep):
    B, C, H, W, std = SHAPES[name]
    logits, target = make_case(B, C, H, W, std, seed=0)
    for w, eps, gamma in ((weights(C), EPS, 2.0), (None, 0.0, 2.0), (weights(C), EPS, 0.0), (weights(C), EPS, 3.0)):
        ref = ce_opts_ref(logits, target, w, eps, gamma, keep)
        loss_t, grad_t, kept_t = ce_opts_torch64(logits, target, w, eps, gamma, keep)
        assert abs(ref.loss - loss_t) <= 1e-12
        assert np.abs(ref.grad - grad_t).max() <= 1e-12
        assert ref.n_kept == kept_t >= ref.info['k']
        assert not ref.grad.transpose(0, 2, 3, 1)[~ref.info['kept']].any()


# every selection the GPU test runs: (weights?, eps, gamma, keep)
SELECTIONS = [(True, EPS, g, k) for g in (0.0, 2.0) for k in (0.0625, 0.25, 0.75)] + \
             [(False, 0.0, 2.0, 0.25), (False, 0.0, 2.0, 0.75)]
# seed 0 everywhere, except where the condition below fails at seed 0 (gap 2.3e-5: the seed changes, never the bound)
SEEDS = {('2x5x24x40', False, 0.0, 2.0, 0.75): 2}


def case_seed(name, use_w, eps, gamma, keep):
    return SEEDS.get((name, use_w, eps, gamma, keep), 0)


@pytest.mark.parametrize('name', list(SHAPES))
def test_tau_is_well_separated(name):
    """A condition on the INPUTS, in the reference alone: around tau the per-pixel values are at least 1e-4 (relative)
    apart -- about a hundred times their fp32 rounding -- so the fp32 kernel keeps exactly the reference's pixels and the
    GPU test compares kept masks for equality.  If a case ever fails this, change the seed, never the bound."""
    B, C, H, W, std = SHAPES[name]
    for use_w, eps, gamma, keep in SELECTIONS:
        logits, target = make_case(B, C, H, W, std, seed=case_seed(name, use_w, eps, gamma, keep))
        ref = ce_opts_ref(logits, target, weights(C) if use_w else None, eps, gamma, keep)
        print('%s w=%d eps=%g gamma=%g keep=%g: k=%d n_kept=%d tau=%.6g gap=%.3e'
              % (name, use_w, eps, gamma, keep, ref.info['k'], ref.n_kept, ref.tau, ref.gap))
        assert ref.n_kept == ref.info['k'] and ref.gap >= MIN_GAP


# ------------------------------------------------------------------ edge cases of the contract
def test_all_pixels_ignored():
    logits, target = make_case(2, 4, 6, 7, 2.0, seed=1)
    target[:] = -100
    for keep in (1.0, 0.5):
        ref = ce_opts_ref(logits, target, weights(4), EPS, 2.0, keep)
        assert math.isnan(ref.loss) and not ref.grad.any() and ref.n_kept == 0 and ref.info['n_valid'] == 0


def test_zero_weight_class():
    logits, target = make_case(2, 5, 9, 11, 2.0, seed=3)
    w = weights(5)
    w[2] = 0.0
    ref = ce_opts_ref(logits, target, w, 0.0, 2.0, 0.5)
    loss_t, grad_t, kept_t = ce_opts_torch64(logits, target, w, 0.0, 2.0, 0.5)
    assert abs(ref.loss - loss_t) <= 1e-12 and np.abs(ref.grad - grad_t).max() <= 1e-12 and ref.n_kept == kept_t
    # without smoothing a pixel of the zero-weight class has f = 0 and no gradient
    assert not ref.grad.transpose(0, 2, 3, 1)[target.numpy() == 2].any()
    # every kept weight zero: NaN loss, zero gradient (one class, weight 0)
    only = target.clone()
    only[only >= 0] = 2
    ref = ce_opts_ref(logits, only, w, 0.0, 0.0, 1.0)
    assert math.isnan(ref.loss) and not ref.grad.any() and ref.info['den'] == 0.0 and ref.n_kept == ref.info['n_valid'] > 0


def test_k_of_one():
    logits, target = make_case(1, 4, 3, 5, 2.0, seed=2, ignore_frac=0.0)
    ref = ce_opts_ref(logits, target, None, 0.0, 0.0, 0.01)       # ceil(0.01 * 15) = 1
    assert ref.info['k'] == 1 and ref.n_kept == 1 and ref.tau == ref.info['f'].max()
    assert ref.loss == pytest.approx(ref.tau, rel=1e-15)
    assert int(ref.grad.any(axis=1).sum()) == 1


def test_out_of_range_labels_are_counted_and_ignored():
    logits, target = make_case(2, 5, 9, 11, 2.0, seed=4)
    bad = target.clone()
    bad.view(-1)[[3, 50, 77]] = torch.tensor([255, -7, 5])
    as_ignored = bad.clone()
    as_ignored.view(-1)[[3, 50, 77]] = -100
    a = ce_opts_ref(logits, bad, weights(5), EPS, 2.0, 0.25)
    b = ce_opts_ref(logits, as_ignored, weights(5), EPS, 2.0, 0.25)
    assert a.info['n_bad'] == 3 and b.info['n_bad'] == 0 and a.info['n_valid'] == b.info['n_valid']
    assert a.loss == b.loss and np.array_equal(a.grad, b.grad) and a.n_kept == b.n_kept


# ------------------------------------------------------------------ interface
def test_header_declares_the_entry_points():
    from pytorch_segmentation_amd import _lib
    protos = _lib.parse_header()
    assert _lib.abi_version_of_header() == 14
    assert protos['pseg_ce_opts_workspace_bytes'][2] == ['B', 'C', 'HW']
    assert protos['pseg_ce_opts_fwd_bwd'][2] == ['logits', 'target', 'B', 'C', 'HW', 'ignore_index', 'class_weight',
                                                 'label_smoothing', 'focal_gamma', 'keep_ratio', 'dlogits', 'loss_out',
                                                 'workspace', 'workspace_bytes', 'stream']


def test_make_loss_options():
    from pytorch_segmentation_amd import utils
    from pytorch_segmentation_amd.utils import compute_loss, loss, make_loss
    assert make_loss('ce') is compute_loss
    assert make_loss('ce', class_weight=None, label_smoothing=0.0, focal_gamma=0.0, keep_ratio=1.0) is compute_loss
    assert make_loss('lovasz', keep_ratio=1.0) is make_loss('lovasz')
    for name in ('ce', 'ce+lovasz'):
        for opts in ({'focal_gamma': 2.0}, {'class_weight': [1.0, 2.0]}, {'label_smoothing': 0.1}, {'keep_ratio': 0.5}):
            fn = make_loss(name, **opts)
            assert fn is not compute_loss and fn is not make_loss(name)
            assert list(inspect.signature(fn).parameters) == ['outputs', 'targets', 'model']
    with pytest.raises(ValueError, match='lovasz'):
        make_loss('lovasz', label_smoothing=0.1)
    with pytest.raises(ValueError, match='unknown loss'):
        make_loss('dice', focal_gamma=2.0)
    with pytest.raises(TypeError, match='unknown cross-entropy option'):
        make_loss('ce', gamma=2.0)
    assert utils.weighted_cross_entropy_loss is loss.weighted_cross_entropy_loss
    assert list(inspect.signature(loss.weighted_cross_entropy_loss).parameters) == [
        'outputs', 'targets', 'class_weight', 'label_smoothing', 'focal_gamma', 'keep_ratio', 'ignore_index']
    from pytorch_segmentation_amd import ops
    assert list(inspect.signature(ops.ce_opts_fwd_bwd).parameters) == [
        'logits', 'target', 'class_weight', 'label_smoothing', 'focal_gamma', 'keep_ratio', 'want_grad', 'ignore_index']
    cpu = torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match='HIP path only'):
        make_loss('ce', focal_gamma=2.0)(*cpu)
    with pytest.raises(RuntimeError, match='HIP path only'):
        make_loss('ce+lovasz', class_weight=[1.0, 2.0])(*cpu)
    with pytest.raises(RuntimeError, match='HIP path only'):
        loss.weighted_cross_entropy_loss(*cpu, label_smoothing=0.1)


def test_train_flags():
    import train
    from pytorch_segmentation_amd.utils import compute_loss
    ap = train.build_parser()
    opt = ap.parse_args(['data/x'])
    assert (opt.class_weights, opt.label_smoothing, opt.focal_gamma, opt.ohem_keep) == (None, 0.0, 0.0, 1.0)
    assert train.loss_from_options(opt) == (compute_loss, None)
    assert train.LOSS_FN is compute_loss and train.CLASS_WEIGHTS is None
    opt = ap.parse_args(['data/x', '--class-weights', '0.5', '2', '1', '--label-smoothing', '0.1', '--focal-gamma', '2',
                         '--ohem-keep', '0.25', '--loss', 'ce+lovasz'])
    assert (opt.class_weights, opt.label_smoothing, opt.focal_gamma, opt.ohem_keep) == ([0.5, 2.0, 1.0], 0.1, 2.0, 0.25)
    fn, w = train.loss_from_options(opt)
    assert fn is not compute_loss and w == [0.5, 2.0, 1.0]
    assert list(inspect.signature(fn).parameters) == ['outputs', 'targets', 'model']
    with pytest.raises(ValueError, match='lovasz'):
        train.loss_from_options(ap.parse_args(['data/x', '--loss', 'lovasz', '--focal-gamma', '2']))
    names = list(inspect.signature(train.train).parameters)
    assert names == ['data_dir', 'epochs', 'img_size', 'batch_size', 'accumulate', 'lr', 'adam', 'resume', 'weights',
                     'num_workers', 'multi_scale', 'rect', 'mixed_precision', 'notest', 'nosave', 'model_name', 'augment']


# ------------------------------------------------------------------ host-side refusals
@pytest.fixture(scope='module')
def lib():
    from pytorch_segmentation_amd import _lib
    from pytorch_segmentation_amd.csrc import build as csrc_build
    csrc_build.build(verbose=False)
    _lib.load()
    return _lib


def test_library_exports_the_entry_points_and_sizes_the_workspace(lib):
    assert {'pseg_ce_opts_fwd_bwd', 'pseg_ce_opts_workspace_bytes'} <= set(lib.prototypes())
    # the parked values: 4 bytes per pixel, plus the header, the histograms and the partials
    npix = 16 * 512 * 512
    assert 4 * npix <= lib.query('pseg_ce_opts_workspace_bytes', 16, 21, 512 * 512) <= 4 * npix + (1 << 17)
    assert lib.query('pseg_ce_opts_workspace_bytes', 16, 84, 512 * 512) == lib.query('pseg_ce_opts_workspace_bytes', 16, 21, 512 * 512)
    assert lib.query('pseg_ce_opts_workspace_bytes', 0, 21, 64) == 0
    assert lib.query('pseg_ce_opts_workspace_bytes', 2, 21, 1 << 30) == 0      # 2^31 pixels: 32-bit counts
    # the existing sweep's call: all null, all zero
    rc = lib.load().pseg_ce_opts_fwd_bwd(None, None, 0, 0, 0, 0, None, 0.0, 0.0, 0.0, None, None, None, 0, None)
    assert rc == -1 and lib.load().pseg_last_error().startswith(b'ce_opts:')


@pytest.mark.skipif(torch.cuda.is_available(), reason='uses made-up device addresses: host-side checks only')
def test_argument_refusals(lib):
    """Every refusal the header lists, by the host-side checks alone: the pointers are made-up addresses and nothing is
    dereferenced or launched."""
    A, MIS = 0x7f0000000000, 0x7f0000000004
    need = lib.query('pseg_ce_opts_workspace_bytes', 2, 5, 960)

    def call(logits=A, target=A, B=2, C=5, HW=960, w=None, eps=0.0, gamma=0.0, keep=1.0, dl=A, out=A, ws=A, nbytes=need):
        lib.call('pseg_ce_opts_fwd_bwd', logits, target, B, C, HW, -100, w, eps, gamma, keep, dl, out, ws, nbytes, None)

    def refused(match, **kw):
        with pytest.raises(lib.PsegError, match='ce_opts: ' + match):
            call(**kw)

    for name in ('logits', 'target', 'out', 'ws'):
        refused('null pointer', **{name: None})
    for name in ('B', 'C', 'HW'):
        refused('bad sizes', **{name: 0})
        refused('bad sizes', **{name: -1})
    refused('more than 2\\^31 - 1 pixels', B=2, HW=1 << 30, nbytes=1 << 40)
    refused('workspace too small', nbytes=need - 1)
    refused('workspace must be 16-byte aligned', ws=MIS)
    for eps in (-0.1, 1.0, 1.5, math.nan):
        refused('label_smoothing', eps=eps)
    for keep in (0.0, -0.5, 1.0001, math.nan):
        refused('keep_ratio', keep=keep)
    for gamma in (-1.0, 0.5, 0.999, 8.5, math.nan):
        refused('focal_gamma', gamma=gamma)
