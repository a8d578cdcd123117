"""The surface (boundary-distance) loss without a GPU: the two numpy restatements of pseg_class_sdist's contract
(tests/surface_ref.py) against each other, phi against Kervadec's one_hot2dist formula, and the host interface: header,
make_loss names and options (the term stubbed, so no device is needed), train.py's flags."""
import ctypes
import inspect
import math
import re

import numpy as np
import pytest
import torch

import surface_ref as S

#          B, C, H, W: every one at most about 2000 pixels per image, so all pairs are affordable
SMALL = [(1, 2, 1, 70), (1, 3, 70, 1), (2, 5, 24, 40), (3, 21, 17, 23), (1, 70, 8, 9), (1, 1024, 4, 4), (2, 4, 31, 64)]


def _special(kind, H=12, W=30):
    t = np.zeros((1, H, W), dtype=np.int64)
    if kind == 'checkerboard':
        t[0] = (np.add.outer(np.arange(H), np.arange(W)) & 1)
    elif kind == 'corner':
        t[0, 0, 0] = 1
    elif kind == 'uniform':
        t[:] = 1
    return t


# ------------------------------------------------------------------ the distance map's two restatements
@pytest.mark.parametrize('shape', SMALL, ids=lambda s: 'x'.join(map(str, s)))
def test_separable_equals_all_pairs(shape):
    B, C, H, W = shape
    t = S.make_labels(B, C, H, W, seed=1).numpy()
    brute, sep = S.sdist_brute(t, C), S.sdist_separable(t, C)
    assert sep.dtype == np.int64 and sep.shape == (B, C, H, W)
    assert np.array_equal(sep, brute)
    # the sign is the membership, 0 only on the planes without a contour, and every magnitude is a sum of two squares
    for b in range(B):
        for c in range(C):
            m = t[b] == c
            if not m.any() or m.all():
                assert not sep[b, c].any()
            else:
                assert (sep[b, c][m] <= -1).all() and (sep[b, c][~m] >= 1).all()
    assert np.abs(sep).max() <= (H - 1) ** 2 + (W - 1) ** 2


@pytest.mark.parametrize('kind', ['checkerboard', 'corner', 'uniform'])
def test_special_maps(kind):
    t = _special(kind)
    H, W = t.shape[1:]
    sep = S.sdist_separable(t, 2)
    assert np.array_equal(sep, S.sdist_brute(t, 2))
    if kind == 'checkerboard':
        assert np.array_equal(np.abs(sep), np.ones_like(sep))
    elif kind == 'corner':
        yy, xx = np.mgrid[0:H, 0:W]
        want = yy ** 2 + xx ** 2
        want[0, 0] = -1
        assert np.array_equal(sep[0, 1], want) and np.array_equal(sep[0, 0], -want)
        assert sep.max() == (H - 1) ** 2 + (W - 1) ** 2
    else:
        assert not sep.any()


def test_two_classes_without_void_mirror_each_other():
    t = S.make_labels(2, 2, 19, 27, seed=3, outline=False, ignore_frac=0.0, n_bad=0).numpy()
    sd = S.sdist_separable(t, 2)
    assert sd.any() and np.array_equal(sd[:, 0], -sd[:, 1])
    # with a void outline they no longer do: a void pixel is outside both
    tv = S.make_labels(1, 2, 19, 27, seed=3).numpy()
    sv = S.sdist_separable(tv, 2)
    void = (tv < 0) | (tv >= 2)
    assert void.any() and (sv[:, 0][void] > 0).all() and (sv[:, 1][void] > 0).all()
    assert not np.array_equal(sv[:, 0], -sv[:, 1])


def test_absent_and_full_classes_give_zero_maps():
    t = S.make_labels(3, 21, 17, 23, seed=0).numpy()
    sd = S.sdist_separable(t, 21)
    c0 = t[0, 0, 0]
    assert (t[0] == c0).any() and not (t[1] == c0).any()         # make_labels: absent from image 1 only
    assert sd[0, c0].any() and not sd[1, c0].any()
    absent = [c for c in range(21) if not (t == c).any()]
    assert absent and not sd[:, absent].any()
    full = np.full((1, 5, 6), 2, dtype=np.int64)
    assert not S.sdist_separable(full, 4).any() and not S.sdist_brute(full, 4).any()
    full[0, 2, 3] = -100                                          # one void pixel: now class 2 has a contour around it
    sd = S.sdist_separable(full, 4)
    assert sd[0, 2, 2, 3] == 1 and sd[0, 2, 2, 4] == -1 and not sd[0, [0, 1, 3]].any()


def test_phi_is_one_hot2dist():
    """Kervadec's one_hot2dist: edt(neg) * neg - (edt(pos) - 1) * pos, edt(mask) the distance of the mask's pixels to its
    complement -- restated from unsigned distances"""
    t = S.make_labels(2, 5, 24, 40, seed=2).numpy()
    sd = S.sdist_separable(t, 5)
    for b in range(2):
        for c in range(5):
            pos = t[b] == c
            if not pos.any() or pos.all():
                assert not S.phi(sd[b, c]).any()
                continue
            neg = ~pos
            edt_neg = np.sqrt(np.where(neg, np.abs(sd[b, c]), 0).astype(np.float64))       # outside: distance to the class
            edt_pos = np.sqrt(np.where(pos, np.abs(sd[b, c]), 0).astype(np.float64))       # inside: distance to the outside
            want = edt_neg * neg - (edt_pos - 1) * pos
            assert np.array_equal(S.phi(sd[b, c]), want)
    f = S.phi(sd)
    assert f.max() > 3 and f.min() < -1
    clipped = S.phi(sd, 3.0)
    assert clipped.max() == 3.0 and clipped.min() >= -3.0 and np.array_equal(clipped, np.clip(f, -3, 3))
    assert np.array_equal(S.phi(np.array([4, -4, -1, 0, 1])), np.array([2.0, -1.0, 0.0, 0.0, 1.0]))


def test_restatement_gradient_matches_central_differences():
    logits, target = S.make_case(2, 3, 5, 6, 2.0, seed=0)
    x = logits.double().numpy()
    for clip in (0.0, 1.5):
        loss, grad, info = S.surface_ref(x, target, clip)
        assert info['n_bad'] > 0 and 0 < info['n_valid'] < target.numel()
        h, worst = 1e-6, 0.0
        for idx in np.ndindex(*x.shape):
            xp, xm = x.copy(), x.copy()
            xp[idx] += h
            xm[idx] -= h
            fd = (S.surface_ref(xp, target, clip, sdist=info['sdist'])[0] - S.surface_ref(xm, target, clip, sdist=info['sdist'])[0]) / (2 * h)
            worst = max(worst, abs(fd - grad[idx]))
        print('clip %g: loss %.12f, max |fd - grad| %.3e, max |grad| %.3e' % (clip, loss, worst, np.abs(grad).max()))
        assert worst <= 1e-8
        assert not grad.transpose(0, 2, 3, 1)[~info['valid']].any()
    loss, grad, info = S.surface_ref(x, torch.full_like(target, -100))
    assert loss == 0.0 and not grad.any() and info['n_valid'] == 0


# ------------------------------------------------------------------ header
def test_header_declares_the_entry_points():
    from pytorch_segmentation_amd import _lib
    protos = _lib.parse_header()
    assert _lib.abi_version_of_header() == 14
    assert protos['pseg_class_sdist_workspace_bytes'][2] == ['B', 'C', 'H', 'W']
    assert protos['pseg_class_sdist'][2] == ['labels', 'B', 'H', 'W', 'C', 'sdist', 'workspace', 'workspace_bytes', 'stream']
    assert protos['pseg_surface_workspace_bytes'][2] == ['B', 'C', 'HW']
    assert protos['pseg_surface_fwd_bwd'][2] == ['logits', 'target', 'sdist', 'B', 'C', 'HW', 'ignore_index', 'clip', 'dlogits',
                                                 'out', 'workspace', 'workspace_bytes', 'stream']
    assert protos['pseg_surface_workspace_bytes'][0] is ctypes.c_int64 and protos['pseg_class_sdist_workspace_bytes'][0] is ctypes.c_int64
    # the cross-entropy call's arguments around sdist and clip
    ce = protos['pseg_ce_fwd_bwd'][1]
    assert protos['pseg_surface_fwd_bwd'][1] == ce[:2] + [ctypes.c_void_p] + ce[2:6] + [ctypes.c_float] + ce[6:]
    header = open(_lib.HEADER_PATH).read()
    additive = header.split('#define PSEG_ABI_VERSION')[0]
    for name in ('pseg_class_sdist_workspace_bytes', 'pseg_class_sdist', 'pseg_surface_workspace_bytes', 'pseg_surface_fwd_bwd'):
        assert name in additive, name


@pytest.fixture(scope='module')
def lib():
    from pytorch_segmentation_amd import _lib
    from pytorch_segmentation_amd.csrc import build as csrc_build
    csrc_build.build(verbose=False)
    _lib.load()
    return _lib


def test_library_exports_the_entry_points_and_sizes_the_workspaces(lib):
    assert {'pseg_class_sdist', 'pseg_class_sdist_workspace_bytes', 'pseg_surface_fwd_bwd',
            'pseg_surface_workspace_bytes'} <= set(lib.prototypes())
    # 4 bytes per (image, class) and 2 per pixel
    need = lib.query('pseg_class_sdist_workspace_bytes', 16, 21, 512, 512)
    assert 16 * 512 * 512 * 2 <= need <= 16 * 512 * 512 * 2 + (1 << 16)
    assert 0 < lib.query('pseg_class_sdist_workspace_bytes', 1, 1024, 4, 4) < (1 << 20)
    for refused in ((0, 2, 8, 8), (1, 0, 8, 8), (1, 1025, 8, 8), (1, 2, 16385, 8), (1, 2, 8, 16385), (1, 2, 0, 8),
                    (32, 21, 1024, 1024), (2, 1, 16384, 16384)):
        assert lib.query('pseg_class_sdist_workspace_bytes', *refused) == 0, refused
    assert lib.query('pseg_class_sdist_workspace_bytes', 1, 1, 16384, 16384) > 0        # 1 GiB of int32: the largest side fits
    # 24 bytes per block of 1024 pixels
    need = lib.query('pseg_surface_workspace_bytes', 16, 21, 512 * 512)
    assert 24 * 16 * 256 <= need <= 24 * 16 * 256 + (1 << 12)
    assert lib.query('pseg_surface_workspace_bytes', 0, 21, 64) == 0 and lib.query('pseg_surface_workspace_bytes', 1, 1025, 64) == 0
    assert lib.query('pseg_surface_workspace_bytes', 64, 21, 1024 * 1024) == 0
    raw = lib.load()
    assert raw.pseg_class_sdist(None, 0, 0, 0, 0, None, None, 0, None) == -1
    assert raw.pseg_last_error().startswith(b'pseg_class_sdist:')
    assert raw.pseg_surface_fwd_bwd(None, None, None, 0, 0, 0, 0, 0.0, None, None, None, 0, None) == -1
    assert raw.pseg_last_error().startswith(b'pseg_surface_fwd_bwd:')


@pytest.mark.skipif(torch.cuda.is_available(), reason='uses made-up device addresses: host-side checks only')
def test_argument_refusals(lib):
    """Every refusal the header lists, by the host-side checks alone: the pointers are made-up addresses and nothing is
    dereferenced or launched."""
    A, A2, A3, MIS = 0x7f0000000000, 0x7f0000100000, 0x7f0000200000, 0x7f0000000004

    def sdist(labels=A, B=2, H=24, W=40, C=5, out=A2, ws=A3, nbytes=None):
        need = lib.query('pseg_class_sdist_workspace_bytes', B, C, H, W)
        lib.call('pseg_class_sdist', labels, B, H, W, C, out, ws, need if nbytes is None else nbytes, None)

    def refused(fn, match, **kw):
        entry = {'sdist': 'pseg_class_sdist', 'surface': 'pseg_surface_fwd_bwd'}[fn.__name__]
        with pytest.raises(lib.PsegError, match=entry + ': .*' + match):
            fn(**kw)

    for name in ('labels', 'out', 'ws'):
        refused(sdist, 'null pointer', **{name: None})
    for name in ('B', 'H', 'W'):
        refused(sdist, 'must be >= 1', **{name: 0}, nbytes=1 << 30)
    refused(sdist, 'H, W = 16385, 8', H=16385, W=8, nbytes=1 << 40)
    refused(sdist, 'H, W = 8, 16385', H=8, W=16385, nbytes=1 << 40)
    refused(sdist, 'class count C = 0', C=0, nbytes=1 << 30)
    refused(sdist, 'class count C = 1025', C=1025, nbytes=1 << 30)
    refused(sdist, 'above 2 GiB', B=32, C=21, H=1024, W=1024, nbytes=1 << 40)
    refused(sdist, 'workspace too small', nbytes=lib.query('pseg_class_sdist_workspace_bytes', 2, 5, 24, 40) - 1)
    refused(sdist, 'workspace too small', nbytes=0)
    refused(sdist, '16-byte aligned', ws=MIS)

    need = lib.query('pseg_surface_workspace_bytes', 2, 5, 960)

    def surface(logits=A, target=A, sd=A3, B=2, C=5, HW=960, clip=0.0, dl=A2, out=A, ws=A, nbytes=need):
        lib.call('pseg_surface_fwd_bwd', logits, target, sd, B, C, HW, -100, clip, dl, out, ws, nbytes, None)

    for name in ('logits', 'target', 'sd', 'out', 'ws'):
        refused(surface, 'null pointer', **{name: None})
    for name in ('B', 'C', 'HW'):
        refused(surface, 'bad sizes', **{name: 0})
    refused(surface, 'at most 1024 classes', C=1025, HW=16)
    refused(surface, 'above 2 GiB', B=64, C=21, HW=1024 * 1024, nbytes=1 << 40)
    for clip in (-1.0, math.nan, math.inf, -math.inf):
        refused(surface, 'clip', clip=clip)
    refused(surface, 'must not alias logits', dl=A)
    refused(surface, 'must not alias sdist', dl=A3)
    refused(surface, 'workspace too small', nbytes=need - 1)
    refused(surface, '16-byte aligned', ws=MIS)


# ------------------------------------------------------------------ make_loss
def test_make_loss_names_and_options(monkeypatch):
    from pytorch_segmentation_amd import ops, utils
    from pytorch_segmentation_amd.utils import compute_loss, loss, make_loss
    new = ('ce+surface', 'tversky+surface', 'ce+tversky+surface')
    assert loss.TERMS['ce+surface'] == ('ce', 'surface') and loss.TERMS['tversky+surface'] == ('tversky', 'surface')
    assert loss.TERMS['ce+tversky+surface'] == ('ce', 'tversky', 'surface') and 'surface' not in loss.TERMS
    assert set(loss.LOSSES) == set(loss.TERMS) and all(kinds[-1] == 'surface' for n, kinds in loss.TERMS.items() if 'surface' in n)
    assert loss.SURFACE_OPTIONS == {'surface_weight': 0.01, 'surface_clip': 0.0}
    # what was there stays what it was
    assert make_loss('ce') is compute_loss and make_loss('tversky') is loss.LOSSES['tversky']
    assert loss.TVERSKY_OPTIONS['tversky_weight'] == 1.0 and loss.BOUNDARY_OPTIONS['boundary_boost'] == 0.0
    with pytest.raises(ValueError, match='unknown loss'):
        make_loss('surface')                                      # no bare name
    with pytest.raises(ValueError, match='unknown loss'):
        make_loss('surface', surface_weight=0.5, bogus=1)         # the name is refused first
    with pytest.raises(TypeError, match='unknown cross-entropy option'):
        make_loss('ce+surface', weight=0.5)
    # an option left at its default is not an option
    for name in loss.LOSSES:
        assert make_loss(name) is loss.LOSSES[name]
        assert make_loss(name, **loss.BOUNDARY_OPTIONS) is loss.LOSSES[name]
        assert make_loss(name, **loss.SURFACE_OPTIONS, **loss.TVERSKY_OPTIONS, **loss.CE_OPTIONS) is loss.LOSSES[name]
        assert make_loss(name, surface_weight=None, surface_clip=None) is loss.LOSSES[name]
    assert len({id(make_loss(n)) for n in loss.LOSSES}) == len(loss.LOSSES)
    # the surface options: on a name with a surface term only
    for opts in ({'surface_weight': 0.5}, {'surface_clip': 3.0}, {'surface_weight': lambda: 0.01}, {'surface_weight': 0.0}):
        for name in new:
            fn = make_loss(name, **opts)
            assert fn is not make_loss(name) and list(inspect.signature(fn).parameters) == ['outputs', 'targets', 'model']
        for name in ('ce', 'lovasz', 'ce+lovasz', 'tversky', 'ce+tversky'):
            with pytest.raises(ValueError, match=re.escape('the surface options do not apply to %r' % name)):
                make_loss(name, **opts)
    for bad in ({'surface_weight': -0.1}, {'surface_weight': math.nan}, {'surface_weight': math.inf}):
        with pytest.raises(ValueError, match='surface_weight must be finite and >= 0'):
            make_loss('ce+surface', **bad)
    for bad in ({'surface_clip': -1.0}, {'surface_clip': math.nan}, {'surface_clip': math.inf}):
        with pytest.raises(ValueError, match='surface_clip must be finite and >= 0'):
            make_loss('ce+surface', **bad)
    # the cross-entropy and boundary options need a 'ce' term, the Tversky options a 'tversky' term: the same messages
    with pytest.raises(ValueError, match="the cross-entropy options do not apply to 'tversky\\+surface'"):
        make_loss('tversky+surface', focal_gamma=2.0)
    with pytest.raises(ValueError, match="the boundary options do not apply to 'tversky\\+surface'"):
        make_loss('tversky+surface', boundary_boost=1.0)
    with pytest.raises(ValueError, match="the Tversky options do not apply to 'ce\\+surface'"):
        make_loss('ce+surface', tversky_power=2.0)
    with pytest.raises(ValueError, match="the cross-entropy options do not apply to 'lovasz'"):
        make_loss('lovasz', label_smoothing=0.1)
    with pytest.raises(ValueError, match="the boundary options do not apply to 'tversky'"):
        make_loss('tversky', boundary_boost=1.0)
    for name, opts in (('ce+surface', {'focal_gamma': 2.0}), ('ce+surface', {'boundary_boost': 1.0, 'boundary_width': 3}),
                       ('tversky+surface', {'tversky_power': 0.75}), ('ce+tversky+surface', {'tversky_weight': 0.5}),
                       ('ce+tversky+surface', {'label_smoothing': 0.1, 'tversky_alpha': 0.3, 'tversky_beta': 0.7,
                                               'surface_clip': 5.0})):
        fn = make_loss(name, **opts)
        assert fn is not make_loss(name) and list(inspect.signature(fn).parameters) == ['outputs', 'targets', 'model']
    # which terms a configured name builds, in table order, and launch_last_first only for 'ce+tversky'
    seen = []
    real = loss._compose
    monkeypatch.setattr(loss, '_compose', lambda name, term_of, launch_last_first=False:
                        seen.append((name, term_of, launch_last_first)) or real(name, term_of, launch_last_first))
    made = []
    monkeypatch.setattr(loss, '_surface_term', lambda weight=1.0, clip=0.0, ignore_index=-100:
                        made.append((weight, clip)) or (lambda logits, targets: None))
    ramp = lambda: 0.25
    for name in list(loss.LOSSES):
        make_loss(name, **({'surface_weight': ramp, 'surface_clip': 4} if 'surface' in name else {'keep_ratio': 0.5} if
                           'ce' in loss.TERMS[name] else {'tversky_power': 2.0} if 'tversky' in name else {}))
    assert [s[0] for s in seen] == [n for n in loss.LOSSES if n != 'lovasz']
    assert [s[0] for s in seen if s[2]] == ['ce+tversky']
    assert made == [(ramp, 4)] * 3                                # the callable itself reaches the term: no float() of it
    for name, term_of, _ in seen:
        if 'surface' not in name:
            assert term_of['surface'] is loss._DEFAULT_TERMS['surface']
    # the public surface
    assert utils.surface_loss is loss.surface_loss and utils.signed_distance is loss.signed_distance
    assert {'surface_loss', 'signed_distance'} <= set(utils.__all__)
    assert list(inspect.signature(loss.surface_loss).parameters) == ['outputs', 'targets', 'clip', 'ignore_index']
    assert list(inspect.signature(loss.signed_distance).parameters) == ['targets', 'num_classes', 'clip']
    assert list(inspect.signature(ops.class_sdist).parameters) == ['labels', 'num_classes']
    sig = inspect.signature(ops.surface_fwd_bwd)
    assert list(sig.parameters) == ['logits', 'target', 'sdist', 'clip', 'want_grad', 'ignore_index']
    assert [p.default for p in sig.parameters.values()][3:] == [0.0, True, -100]


def test_callable_weight_is_read_on_every_call(monkeypatch):
    """The term with the two device calls stubbed: a zero-argument callable is read once per call of the term, after the
    kernel call, and a weight of exactly 1 returns the kernel's scalar itself."""
    from pytorch_segmentation_amd import ops
    from pytorch_segmentation_amd.utils import loss
    calls = []
    monkeypatch.setattr(ops, 'class_sdist', lambda t, C: calls.append(('sdist', C)) or torch.zeros(t.shape[0], C, *t.shape[1:],
                                                                                                  dtype=torch.int32))
    monkeypatch.setattr(ops, 'surface_fwd_bwd', lambda logits, target, sdist, clip=0.0, want_grad=True, ignore_index=-100:
                        calls.append(('loss', clip, want_grad, ignore_index)) or (torch.tensor([2.0, 16.0, 0.0]), None))
    logits, target = torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64)
    schedule = iter([0.5, 0.25, 1.0])
    reads = []
    term = loss._surface_term(lambda: reads.append(1) or next(schedule), clip=3.0, ignore_index=255)
    assert term(logits, target).item() == 1.0 and len(reads) == 1
    assert term(logits, target).item() == 0.5 and len(reads) == 2
    assert term(logits, target).item() == 2.0 and len(reads) == 3
    assert calls == [('sdist', 3), ('loss', 3.0, False, 255)] * 3
    assert loss._surface_term(0.125)(logits, target).item() == 0.25
    assert loss._surface_term(0.0)(logits, target).item() == 0.0


def test_wrappers_refuse_cpu_tensors():
    from pytorch_segmentation_amd.utils import loss, make_loss
    cpu = torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64)
    for fn in (make_loss('ce+surface'), make_loss('tversky+surface'), make_loss('ce+tversky+surface', surface_weight=0.5),
               loss.surface_loss):
        with pytest.raises(RuntimeError, match='HIP path only'):
            fn(*cpu)
    with pytest.raises(RuntimeError, match='HIP path only'):
        loss.signed_distance(cpu[1], 2)


# ------------------------------------------------------------------ train.py
def test_train_flags():
    import train
    from pytorch_segmentation_amd.utils import compute_loss, loss, make_loss
    ap = train.build_parser()
    opt = ap.parse_args(['data/x'])
    assert (opt.surface_weight, opt.surface_clip, opt.surface_ramp_epochs) == (None, None, None)
    assert train.loss_from_options(opt) == (compute_loss, None) and train.SURFACE_RAMP is None
    for name in ('ce+surface', 'tversky+surface', 'ce+tversky+surface'):
        assert train.loss_from_options(ap.parse_args(['data/x', '--loss', name])) == (make_loss(name), None)
        opt = ap.parse_args(['data/x', '--loss', name, '--surface-weight', '0.05', '--surface-clip', '20'])
        assert (opt.surface_weight, opt.surface_clip, opt.surface_ramp_epochs) == (0.05, 20.0, None)
        fn, w = train.loss_from_options(opt)
        assert fn is not make_loss(name) and w is None and train.SURFACE_RAMP is None
        assert list(inspect.signature(fn).parameters) == ['outputs', 'targets', 'model']
        # flags at their defaults are no options
        opt = ap.parse_args(['data/x', '--loss', name, '--surface-weight', '0.01', '--surface-clip', '0', '--surface-ramp-epochs', '0'])
        assert train.loss_from_options(opt)[0] is make_loss(name) and train.SURFACE_RAMP is None
    with pytest.raises(SystemExit):
        ap.parse_args(['data/x', '--loss', 'surface'])
    with pytest.raises(SystemExit):
        ap.parse_args(['data/x', '--loss', 'ce+surface', '--surface-ramp-epochs', '1.5'])
    # the ramp: W * min(1, (epoch + 1) / E), read from the trainer's epoch at every call
    opt = ap.parse_args(['data/x', '--loss', 'ce+surface', '--surface-weight', '0.08', '--surface-ramp-epochs', '4'])
    fn, _ = train.loss_from_options(opt)
    ramp = train.SURFACE_RAMP
    assert fn is not make_loss('ce+surface') and isinstance(ramp, train.SurfaceRamp) and ramp() == 0.08

    class FakeTrainer:
        epoch = 0
    ramp.trainer = FakeTrainer()
    got = []
    for e in range(6):
        ramp.trainer.epoch = e
        got.append(ramp())
    assert got == pytest.approx([0.02, 0.04, 0.06, 0.08, 0.08, 0.08], rel=1e-12)
    fn, _ = train.loss_from_options(ap.parse_args(['data/x', '--loss', 'tversky+surface', '--surface-ramp-epochs', '2']))
    assert train.SURFACE_RAMP.weight == loss.SURFACE_OPTIONS['surface_weight'] and train.SURFACE_RAMP.epochs == 2
    train.loss_from_options(ap.parse_args(['data/x']))
    assert train.SURFACE_RAMP is None                             # a later call without the flag drops the ramp
    # refusals: any of the three flags without a surface term, and values out of range
    for name in ('ce', 'lovasz', 'ce+lovasz', 'tversky', 'ce+tversky'):
        for flags in (['--surface-weight', '0.5'], ['--surface-clip', '3'], ['--surface-ramp-epochs', '2'],
                      ['--surface-ramp-epochs', '0']):
            with pytest.raises(ValueError, match='the surface options do not apply'):
                train.loss_from_options(ap.parse_args(['data/x', '--loss', name] + flags))
    for flags, match in ((['--surface-weight', '-1'], '--surface-weight must be >= 0'),
                         (['--surface-clip', '-1'], '--surface-clip must be >= 0'),
                         (['--surface-ramp-epochs', '-1'], '--surface-ramp-epochs must be >= 0')):
        with pytest.raises(ValueError, match=match):
            train.loss_from_options(ap.parse_args(['data/x', '--loss', 'ce+surface'] + flags))
    with pytest.raises(ValueError, match='tversky\\+surface'):
        train.loss_from_options(ap.parse_args(['data/x', '--loss', 'tversky+surface', '--label-smoothing', '0.1']))
    for flag in ('--surface-weight', '--surface-clip', '--surface-ramp-epochs',
                 '--loss ce|lovasz|ce+lovasz|tversky|ce+tversky|ce+surface|tversky+surface|ce+tversky+surface'):
        assert flag in train.__doc__
    names = list(inspect.signature(train.train).parameters)
    assert names == ['data_dir', 'epochs', 'img_size', 'batch_size', 'accumulate', 'lr', 'adam', 'resume', 'weights',
                     'num_workers', 'multi_scale', 'rect', 'mixed_precision', 'notest', 'nosave', 'model_name', 'augment']
