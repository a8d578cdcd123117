"""Boundary-weighted cross-entropy without a GPU: the restatement of pseg_ce_opts_binned_fwd_bwd's contract
(tests/ce_binned_ref.py) against test_ce_opts_cpu.ce_opts_ref (table of ones), a separately computed band formula ('flat')
and float64 autograd; the conditions on the shared inputs that let the GPU test compare kept masks for equality;
boundary_weight_table; make_loss's boundary options; train.py's flags; header, export and host-side refusals."""
import inspect
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import boundary_ref as BR
import ce_binned_ref as R
from test_ce_opts_cpu import ce_opts_ref

ONES = np.ones(256)


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize('keep', [1.0, 0.25])
@pytest.mark.parametrize('name', list(R.SHAPES))
def test_table_of_ones_is_the_unweighted_restatement(name, keep):
    logits, target, depth = R.make_case(name)
    C = R.SHAPES[name][1]
    for w, eps, gamma in ((None, 0.0, 0.0), (R.weights(C), R.EPS, 2.0)):
        a = R.ce_binned_ref(logits, target, depth, ONES, w, eps, gamma, keep)
        b = ce_opts_ref(logits, target, w, eps, gamma, keep)
        assert a.loss == b.loss and np.array_equal(a.grad, b.grad)
        assert (a.n_kept, a.tau, a.gap, a.den) == (b.n_kept, b.tau, b.gap, b.info['den'])
        assert a.info['n_valid'] == b.info['n_valid'] and a.info['n_bad'] == b.info['n_bad'] > 0
        assert np.array_equal(a.info['kept'], b.info['kept'])


@pytest.mark.parametrize('name', list(R.SHAPES))
def test_flat_table_is_the_band_formula(name):
    """'flat': loss = (sum_all f + A sum_band f) / (sum_all w + A sum_band w), band = depth <= d, from ce_opts_ref's own f and
    boundary_ref.label_depth -- nothing of ce_binned_ref is used on the right-hand side"""
    logits, target, _ = R.make_case(name)
    C = R.SHAPES[name][1]
    w = R.weights(C)
    plain = ce_opts_ref(logits, target, w, R.EPS, 2.0, 1.0)
    valid = plain.info['valid']
    f = plain.info['f']
    wt = w[target.numpy().reshape(-1)[valid]]
    band = (BR.label_depth(target.numpy(), R.D) <= R.D).reshape(-1)[valid]
    want = (f.sum() + R.BOOST * f[band].sum()) / (wt.sum() + R.BOOST * wt[band].sum())
    got = R.ce_binned_ref(logits, target, BR.label_depth(target.numpy(), R.D), R.weight_table(R.D, R.BOOST, 'flat'), w, R.EPS,
                          2.0, 1.0)
    print('%s: %.15f vs %.15f, band share %.3f' % (name, got.loss, want, band.mean()))
    assert abs(got.loss - want) <= 1e-12 * want and 0 < band.sum() < band.size


def binned_torch64(logits, target, depth, table, w, eps, gamma, keep):
    """float64 autograd of the same expression: F.cross_entropy per pixel, u from the table, torch.topk on u f"""
    x = logits.detach().double().requires_grad_(True)
    C = x.shape[1]
    t = target.clone()
    t[(t < 0) | (t >= C)] = -100
    wt = None if w is None else torch.as_tensor(np.asarray(w), dtype=torch.float64)
    ell = F.cross_entropy(x, t, weight=wt, label_smoothing=eps, reduction='none')
    pt = torch.exp(-F.cross_entropy(x, t, reduction='none'))
    f = (1 - pt) ** gamma * ell if gamma != 0 else ell
    u = torch.as_tensor(np.asarray(table), dtype=torch.float64)[torch.as_tensor(depth)]
    valid = t != -100
    gv, uv = (u * f)[valid], u[valid]
    wv = torch.ones_like(gv) if wt is None else wt[t[valid]]
    kept = torch.ones_like(gv, dtype=torch.bool)
    if keep != 1.0:
        k = min(max(int(math.ceil(float(np.float32(keep)) * gv.numel())), 1), gv.numel())
        kept = gv.detach() >= torch.topk(gv.detach(), k).values[-1]
    loss = gv[kept].sum() / (uv * wv)[kept].sum()
    loss.backward()
    return loss.item(), x.grad.numpy(), int(kept.sum())


@pytest.mark.parametrize('falloff', ['gaussian', 'linear', 'flat'])
@pytest.mark.parametrize('name', list(R.SHAPES))
def test_restatement_matches_float64_autograd(name, falloff):
    logits, target, depth = R.make_case(name)
    C = R.SHAPES[name][1]
    table = R.weight_table(R.D, R.BOOST, falloff)
    for w, eps, gamma, keep in ((None, 0.0, 0.0, 1.0), (R.weights(C), R.EPS, 2.0, 1.0), (R.weights(C), R.EPS, 2.0, 0.25),
                                (None, 0.0, 3.0, 0.75)):
        ref = R.ce_binned_ref(logits, target, depth, table, w, eps, gamma, keep)
        loss_t, grad_t, kept_t = binned_torch64(logits, target, depth, table, w, eps, gamma, keep)
        assert abs(ref.loss - loss_t) <= 1e-12
        assert np.abs(ref.grad - grad_t).max() <= 1e-12
        assert ref.n_kept == kept_t >= ref.info['k']
        assert not ref.grad.transpose(0, 2, 3, 1)[~ref.info['kept']].any()


def test_zero_weight_bins():
    """u = 0: the pixel is valid and counted, may be kept, contributes nothing; every present bin at 0: NaN, zero gradient"""
    logits, target, depth = R.make_case('2x5x24x40')
    table = R.weight_table(R.D, R.BOOST, 'gaussian')
    table[2] = 0.0
    ref = R.ce_binned_ref(logits, target, depth, table, R.weights(5), R.EPS, 2.0, 1.0)
    plain = ce_opts_ref(logits, target, R.weights(5), R.EPS, 2.0, 1.0)
    assert ref.info['n_valid'] == plain.info['n_valid'] == ref.n_kept
    assert not ref.grad.transpose(0, 2, 3, 1)[depth == 2].any() and ref.grad.any()
    ref = R.ce_binned_ref(logits, target, np.full_like(depth, 7), np.where(np.arange(256) == 7, 0.0, 1.0), None, 0.0, 0.0, 0.5)
    assert math.isnan(ref.loss) and not ref.grad.any() and ref.den == 0.0 and ref.n_kept == ref.info['n_valid'] > 0


# ------------------------------------------------------------------ conditions on the shared inputs (the reference alone)
@pytest.mark.parametrize('name', list(R.SHAPES))
def test_case_conditions(name):
    """Every case's depth map holds depth 1, depth d + 1 and a value between (else the table would not be exercised); the
    void patches are there.  For every selection the GPU test runs, n_kept == k and the values around tau are at least
    MIN_GAP (1e-4, relative) apart -- about a hundred times their fp32 rounding -- so the fp32 kernel keeps exactly the
    restatement's pixels.  If a seed fails this, change the seed (ce_binned_ref.SEEDS), never the bound."""
    for falloff in R.TABLES:
        for opt, (use_w, eps, gamma, keep) in R.OPTIONS.items():
            logits, target, depth, w, table, ref = R.reference(name, falloff, opt)
            vals = set(np.unique(depth[ref.info['valid'].reshape(depth.shape)]).tolist())      # (among the pixels that count)
            assert 1 in vals and R.D + 1 in vals and vals & set(range(2, R.D + 1)), vals
            assert set(np.unique(depth).tolist()) <= set(range(1, R.D + 2))
            assert ref.info['n_bad'] > 0 and (target == -100).any()
            if keep != 1.0:
                print('%s %s %s: k=%d n_kept=%d tau=%.6g gap=%.3e' % (name, falloff, opt, ref.info['k'], ref.n_kept, ref.tau, ref.gap))
                assert ref.n_kept == ref.info['k'] and ref.gap >= R.MIN_GAP


# ------------------------------------------------------------------ boundary_weight_table
def test_boundary_weight_table():
    from pytorch_segmentation_amd import ops
    from pytorch_segmentation_amd.utils import boundary_weight_table
    for width, boost, falloff, sigma in ((3, 2.0, 'gaussian', None), (3, 2.0, 'flat', None), (3, 2.0, 'linear', None),
                                         (1, 0.5, 'gaussian', None), (7, 4.0, 'gaussian', 1.5), (254, 1.0, 'linear', None),
                                         (254, 3.0, 'gaussian', None), (5, 0.0, 'flat', None)):
        got = boundary_weight_table(width, boost, falloff, sigma)
        want = R.weight_table(width, boost, falloff, sigma)
        assert got.dtype == torch.float32 and tuple(got.shape) == (256,) and got.device.type == 'cpu'
        assert np.abs(got.double().numpy() - want).max() <= 1e-6 * (1 + boost)
        assert got[0].item() == 1.0 and (got[width + 1:] == 1.0).all() and (got[1:width + 1] >= 1.0).all()
        assert got[1].item() == pytest.approx(1.0 + boost, rel=1e-7)
    assert inspect.signature(boundary_weight_table).parameters['falloff'].default == 'gaussian'
    for bad in (dict(width=0), dict(width=ops.BOUNDARY_MAX_WIDTH + 1), dict(width=2.5), dict(boost=-0.1), dict(boost=math.nan),
                dict(boost=math.inf), dict(falloff='cosine'), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=math.inf),
                dict(sigma=math.nan)):
        with pytest.raises(ValueError, match='boundary_weight_table'):
            boundary_weight_table(**dict(dict(width=3, boost=1.0), **bad))
    # the upload's check of the C call's precondition
    for bad in ([1.0] * 255, [1.0] * 255 + [-1.0], [1.0] * 255 + [math.nan], [math.inf] + [1.0] * 255):
        with pytest.raises(ValueError, match='bin_weight'):
            ops.bin_weight_table(bad, 'cpu')
    assert torch.equal(ops.bin_weight_table(boundary_weight_table(3, 1.0), 'cpu'), boundary_weight_table(3, 1.0))


# ------------------------------------------------------------------ make_loss, train.py
def test_make_loss_boundary_options():
    from pytorch_segmentation_amd import ops, utils
    from pytorch_segmentation_amd.utils import compute_loss, loss, make_loss
    assert loss.BOUNDARY_OPTIONS == {'boundary_boost': 0.0, 'boundary_width': 0, 'boundary_ratio': 0.02,
                                     'boundary_falloff': 'gaussian', 'boundary_sigma': 0.0}
    # an option left at its default is not an option
    assert make_loss('ce') is compute_loss and make_loss('ce', **loss.BOUNDARY_OPTIONS) is compute_loss
    for name in loss.LOSSES:
        assert make_loss(name, **loss.BOUNDARY_OPTIONS) is loss.LOSSES[name]
    for name in ('ce', 'ce+lovasz', 'ce+tversky'):
        for extra in ({}, {'boundary_width': 2}, {'boundary_ratio': 0.05, 'boundary_falloff': 'linear'}, {'focal_gamma': 2.0},
                      {'boundary_sigma': 1.5, 'keep_ratio': 0.5, 'class_weight': [1.0, 2.0]}):
            fn = make_loss(name, boundary_boost=0.5, **extra)
            assert fn is not loss.LOSSES[name] and fn is not make_loss(name, focal_gamma=2.0)
            assert list(inspect.signature(fn).parameters) == ['outputs', 'targets', 'model']
    for name in ('lovasz', 'tversky'):
        with pytest.raises(ValueError, match=name):
            make_loss(name, boundary_boost=0.5)
    for opts in ({'boundary_width': 3}, {'boundary_ratio': 0.05}, {'boundary_falloff': 'flat'}, {'boundary_sigma': 2.0}):
        with pytest.raises(ValueError, match='boundary_boost'):
            make_loss('ce', **opts)
    with pytest.raises(ValueError, match='boundary_boost'):
        make_loss('ce', boundary_boost=-1.0)
    with pytest.raises(ValueError, match='exclude'):
        make_loss('ce', boundary_boost=1.0, boundary_width=3, boundary_ratio=0.05)
    with pytest.raises(ValueError, match='falloff'):
        make_loss('ce', boundary_boost=1.0, boundary_falloff='cosine')
    with pytest.raises(TypeError, match='unknown cross-entropy option'):
        make_loss('ce', boundary_boost=1.0, boundary=3)
    with pytest.raises(ValueError, match='unknown loss'):
        make_loss('dice', boundary_boost=1.0)
    with pytest.raises(ValueError, match='Tversky options'):
        make_loss('ce', boundary_boost=1.0, tversky_power=2.0)
    # the public surface
    assert utils.boundary_weighted_cross_entropy_loss is loss.boundary_weighted_cross_entropy_loss
    assert utils.boundary_weight_table is loss.boundary_weight_table
    assert {'boundary_weighted_cross_entropy_loss', 'boundary_weight_table'} <= set(utils.__all__)
    assert list(inspect.signature(loss.boundary_weighted_cross_entropy_loss).parameters) == [
        'outputs', 'targets', 'boundary_boost', 'boundary_width', 'boundary_ratio', 'boundary_falloff', 'boundary_sigma',
        'class_weight', 'label_smoothing', 'focal_gamma', 'keep_ratio', 'ignore_index']
    assert list(inspect.signature(ops.ce_opts_binned_fwd_bwd).parameters) == [
        'logits', 'target', 'pixel_bin', 'bin_weight', 'class_weight', 'label_smoothing', 'focal_gamma', 'keep_ratio',
        'want_grad', 'ignore_index']
    cpu = torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64)
    for fn in (make_loss('ce', boundary_boost=1.0), make_loss('ce+tversky', boundary_boost=1.0, boundary_width=2),
               lambda o, t: loss.boundary_weighted_cross_entropy_loss(o, t, 1.0)):
        with pytest.raises(RuntimeError, match='HIP path only'):
            fn(*cpu)


def test_train_flags():
    import train
    from pytorch_segmentation_amd.utils import compute_loss, make_loss
    ap = train.build_parser()
    opt = ap.parse_args(['data/x'])
    assert (opt.boundary_boost, opt.boundary_loss_ratio, opt.boundary_loss_width, opt.boundary_falloff, opt.boundary_sigma) == \
        (0.0, None, None, 'gaussian', None)
    assert train.loss_from_options(opt) == (compute_loss, None)
    for name in ('ce', 'ce+lovasz', 'ce+tversky'):
        opt = ap.parse_args(['data/x', '--loss', name, '--boundary-boost', '1', '--boundary-loss-width', '4', '--boundary-falloff',
                             'linear', '--focal-gamma', '2'])
        assert (opt.boundary_boost, opt.boundary_loss_width, opt.boundary_falloff) == (1.0, 4, 'linear')
        fn, w = train.loss_from_options(opt)
        assert fn is not make_loss(name) and w is None
        assert list(inspect.signature(fn).parameters) == ['outputs', 'targets', 'model']
    opt = ap.parse_args(['data/x', '--boundary-boost', '0.5', '--boundary-loss-ratio', '0.05', '--boundary-sigma', '2'])
    assert (opt.boundary_loss_ratio, opt.boundary_sigma) == (0.05, 2.0) and train.loss_from_options(opt)[0] is not compute_loss
    with pytest.raises(SystemExit):
        ap.parse_args(['data/x', '--boundary-boost', '1', '--boundary-loss-width', '4', '--boundary-loss-ratio', '0.05'])
    with pytest.raises(SystemExit):
        ap.parse_args(['data/x', '--boundary-boost', '1', '--boundary-falloff', 'cosine'])
    with pytest.raises(ValueError, match='lovasz'):
        train.loss_from_options(ap.parse_args(['data/x', '--loss', 'lovasz', '--boundary-boost', '1']))
    with pytest.raises(ValueError, match='boundary_boost'):
        train.loss_from_options(ap.parse_args(['data/x', '--boundary-loss-width', '4']))
    for flag in ('--boundary-boost', '--boundary-loss-ratio', '--boundary-loss-width', '--boundary-falloff', '--boundary-sigma'):
        assert flag in train.__doc__


# ------------------------------------------------------------------ header, export, host-side refusals
@pytest.fixture(scope='module')
def lib():
    from pytorch_segmentation_amd import _lib
    from pytorch_segmentation_amd.csrc import build as csrc_build
    csrc_build.build(verbose=False)
    _lib.load()
    return _lib


def test_header_declares_and_library_exports_the_entry_point(lib):
    protos = lib.parse_header()
    assert lib.abi_version_of_header() == 14      # additive: the version does not move
    assert protos['pseg_ce_opts_binned_fwd_bwd'][2] == [
        'logits', 'target', 'pixel_bin', 'bin_weight', 'B', 'C', 'HW', 'ignore_index', 'class_weight', 'label_smoothing',
        'focal_gamma', 'keep_ratio', 'dlogits', 'loss_out', 'workspace', 'workspace_bytes', 'stream']
    assert 'pseg_ce_opts_binned_fwd_bwd' in lib.prototypes() and hasattr(lib.load(), 'pseg_ce_opts_binned_fwd_bwd')
    rc = lib.load().pseg_ce_opts_binned_fwd_bwd(None, None, None, None, 0, 0, 0, 0, None, 0.0, 0.0, 0.0, None, None, None, 0, None)
    assert rc == -1 and lib.load().pseg_last_error().startswith(b'pseg_ce_opts_binned_fwd_bwd:')


@pytest.mark.skipif(torch.cuda.is_available(), reason='uses made-up device addresses: host-side checks only')
def test_argument_refusals(lib):
    """Every refusal by the host-side checks alone: the pointers are made-up addresses, nothing is dereferenced or launched"""
    A, MIS = 0x7f0000000000, 0x7f0000000004
    need = lib.query('pseg_ce_opts_workspace_bytes', 2, 5, 960)

    def call(logits=A, target=A, bins=A + 1, table=A, B=2, C=5, HW=960, w=None, eps=0.0, gamma=0.0, keep=1.0, dl=A, out=A, ws=A,
             nbytes=need):
        lib.call('pseg_ce_opts_binned_fwd_bwd', logits, target, bins, table, B, C, HW, -100, w, eps, gamma, keep, dl, out, ws,
                 nbytes, None)

    def refused(match, **kw):
        with pytest.raises(lib.PsegError, match='\\): pseg_ce_opts_binned_fwd_bwd: ' + match):
            call(**kw)

    for name in ('logits', 'target', 'out', 'ws'):
        refused('null pointer', **{name: None})
    refused('null pixel_bin or bin_weight', bins=None)
    refused('null pixel_bin or bin_weight', table=None)
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
