"""The local dense-CRF refinement without a GPU: the numpy restatement of its definition (tests/crf_ref.py) checked against
properties that follow from the definition, the float32-versus-float64 error the GPU test's tolerance is built on, and the
host layer -- options, command-line flags, entry-point refusals, and that nothing of it is loaded when it is not asked for."""
import ctypes
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import crf_ref
from test_crf_gpu import F32_VS_F64, MAX_EXCLUDED, PARITY, TOL

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = (1.0, 1.0, 1.0)


# ------------------------------------------------------------------ the restatement
def test_zero_weights_return_the_logits():
    U, G, gs = crf_ref.case_inputs(2, 5, 9, 11, 'dataset', 1)
    assert np.array_equal(crf_ref.crf_refine(U, G, gs, w_appearance=0.0, w_smooth=0.0), U.astype(np.float64))
    assert np.array_equal(crf_ref.crf_refine_plain(U, G, gs, w_appearance=0.0, w_smooth=0.0), U.astype(np.float64))


def test_shifted_weights_are_the_definition():
    """exp(e - max e) against the definition's exp(e), in float64 where neither underflows"""
    for ci, (B, C, h, w, opts) in enumerate(crf_ref.CASES):
        U, G, gs = crf_ref.case_inputs(B, C, h, w, 'dataset', 40 + ci)
        assert np.abs(crf_ref.crf_refine(U, G, gs, **opts) - crf_ref.crf_refine_plain(U, G, gs, **opts)).max() < 1e-12


@pytest.mark.parametrize('radius,dilation', [(3, 2), (5, 4), (1, 1)])
def test_uniform_field_gets_the_full_weights_at_every_pixel(radius, dilation):
    """a constant guide and spatially uniform Q: both normalised messages are Q itself, the border included"""
    rng = np.random.RandomState(2)
    u = rng.standard_normal(6) * 3
    U = np.broadcast_to(u.reshape(1, 6, 1, 1), (2, 6, 7, 23)).copy()
    G = np.full((2, 3, 7, 23), 0.3)
    q = crf_ref.softmax(u.reshape(1, 6), 1).reshape(1, 6, 1, 1)
    L = crf_ref.crf_refine(U, G, ONE, radius=radius, dilation=dilation, iters=1, w_appearance=4.0, w_smooth=3.0)
    assert np.abs(L - (U + 7.0 * q)).max() < 1e-12
    L3 = crf_ref.crf_refine(U, G, ONE, radius=radius, dilation=dilation, iters=3, w_appearance=4.0, w_smooth=3.0)
    for _ in range(2):
        q = crf_ref.softmax(u.reshape(1, 6) + 7.0 * q.reshape(1, 6), 1).reshape(1, 6, 1, 1)
    assert np.abs(L3 - (U + 7.0 * q)).max() < 1e-12


def test_a_single_mislabelled_pixel_is_flipped_by_the_defaults():
    U = np.zeros((1, 3, 21, 21))
    U[:, 1] = 3.0                                              # class 1 everywhere ...
    U[0, :, 10, 10] = (0.0, 0.0, 3.0)                          # ... but one pixel says class 2
    G = np.full((1, 3, 21, 21), 90.0)
    assert U.argmax(1)[0, 10, 10] == 2
    L = crf_ref.crf_refine(U, G, ONE)
    assert (L.argmax(1) == 1).all()


def test_a_label_edge_on_a_colour_edge_stays_without_smoothness():
    h, w = 16, 24
    G = np.zeros((1, 3, h, w))
    G[..., 12:] = 200.0
    U = np.zeros((1, 2, h, w))
    U[0, 0, :, :12] = 2.0
    U[0, 1, :, 12:] = 2.0
    L = crf_ref.crf_refine(U, G, ONE, w_smooth=0.0)
    assert np.array_equal(L.argmax(1), U.argmax(1))
    # and every pixel's own class gained: its like-coloured neighbours all vote for it
    assert ((L.max(1) - L.min(1)) > 2.0 + 2.0).all()


def test_mirrored_input_gives_the_mirrored_output():
    for ci, (B, C, h, w, opts) in enumerate(crf_ref.CASES[:3]):
        U, G, gs = crf_ref.case_inputs(1, min(C, 5), h, w, 'reference', 60 + ci)
        L = crf_ref.crf_refine(U, G, gs, **opts)
        Lm = crf_ref.crf_refine(U[..., ::-1], G[..., ::-1], gs, **opts)
        assert np.abs(Lm[..., ::-1] - L).max() < 1e-12


def test_no_neighbour_inside_the_image_means_no_message():
    U, G, gs = crf_ref.case_inputs(1, 4, 2, 2, 'dataset', 3)
    assert np.array_equal(crf_ref.crf_refine(U, G, gs, dilation=2), U.astype(np.float64))
    assert not np.array_equal(crf_ref.crf_refine(U, G, gs, dilation=1), U.astype(np.float64))


def test_float32_reference_error():
    """What the GPU test's tolerance stands on: the float32 run of the restatement differs from the float64 run by at most
    F32_VS_F64 on the parity cases, agrees with it on every pixel whose float64 top-two gap exceeds TOL, and at most
    MAX_EXCLUDED of the pixels of any case lie within TOL."""
    worst = 0.0
    for ci, norm in PARITY:
        B, C, h, w, opts = crf_ref.CASES[ci]
        U, G, gs = crf_ref.case_inputs(B, C, h, w, norm, 100 + 2 * ci + ('dataset', 'reference').index(norm))
        L64 = crf_ref.crf_refine(U, G, gs, dtype=np.float64, **opts)
        L32 = crf_ref.crf_refine(U, G, gs, dtype=np.float32, **opts)
        assert L32.dtype == np.float32 and np.isfinite(L32).all()
        worst = max(worst, float(np.abs(L32 - L64).max()))
        decided = crf_ref.top_two_gap(L64) > TOL
        assert 1.0 - decided.mean() <= MAX_EXCLUDED, (ci, norm)
        assert np.array_equal(L32.argmax(1)[decided], L64.argmax(1)[decided])
    print('largest |float32 - float64| over the parity cases: %.4e' % worst)
    # the constant is this measurement, rounded up (1.0196e-5 where it was made; another libm's float32 exp may move it a little)
    assert 0.5 * F32_VS_F64 <= worst <= 1.1 * F32_VS_F64


# ------------------------------------------------------------------ options and flags
def test_crf_options():
    from pytorch_segmentation_amd.utils.crf import CRF, from_flags
    d = CRF()
    assert (d.radius, d.dilation, d.iters, d.theta, d.weights) == (3, 2, 5, (8.0, 13.0, 3.0), (4.0, 3.0))
    ref = crf_ref.DEFAULTS
    assert (d.radius, d.dilation, d.iters) == (ref['radius'], ref['dilation'], ref['iters'])
    assert d.theta == (ref['theta_alpha'], ref['theta_beta'], ref['theta_gamma']) and d.weights == (ref['w_appearance'], ref['w_smooth'])
    assert CRF.of(True).__dict__ == d.__dict__ and CRF.of(d) is d and CRF.of({'radius': 5, 'iters': 10}).radius == 5
    for ok in (dict(radius=1), dict(radius=5), dict(dilation=1), dict(dilation=4), dict(iters=1), dict(iters=10),
               dict(weights=(0, 0)), dict(theta=(0.5, 1e3, 2))):
        CRF(**ok)
    for bad in (dict(radius=0), dict(radius=6), dict(radius=2.5), dict(radius=True), dict(dilation=0), dict(dilation=5),
                dict(iters=0), dict(iters=11), dict(theta=(0, 1, 1)), dict(theta=(1, -1, 1)), dict(theta=(1, 1, float('nan'))),
                dict(theta=(1, 1, float('inf'))), dict(theta=(1, 1)), dict(weights=(-1, 0)), dict(weights=(0, float('inf'))),
                dict(weights=(1, 2, 3))):
        with pytest.raises(ValueError, match='crf'):
            CRF(**bad)
    for bad in (1, 'yes', [3]):
        with pytest.raises(TypeError):
            CRF.of(bad)
    assert from_flags(False) is None
    got = from_flags(True, 2, None, 7, [1.0, 2.0, 3.0], None)
    assert (got.radius, got.dilation, got.iters, got.theta, got.weights) == (2, 2, 7, (1.0, 2.0, 3.0), (4.0, 3.0))
    for lone in (dict(radius=2), dict(dilation=1), dict(iters=3), dict(theta=[1, 2, 3]), dict(weights=[1, 2])):
        with pytest.raises(ValueError, match='need --crf'):
            from_flags(False, **lone)


def _script(name):
    spec = importlib.util.spec_from_file_location('pseg_crf_cli_' + name.replace('.', '_'), os.path.join(REPO, name))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


LONE_FLAGS = (['--crf-radius', '2'], ['--crf-dilation', '1'], ['--crf-iters', '3'], ['--crf-theta', '1', '2', '3'],
              ['--crf-weights', '1', '2'])


def test_evaluation_flags(capsys):
    cli = _script('test.py')
    opt = cli.parse_args(['val.json'])
    assert opt.crf is False and opt.crf_options is None
    opt = cli.parse_args(['val.json', '--crf'])
    assert opt.crf_options.radius == 3 and opt.crf_options.weights == (4.0, 3.0)
    opt = cli.parse_args(['val.json', '--crf', '--crf-radius', '5', '--crf-dilation', '4', '--crf-iters', '10', '--crf-theta', '1',
                          '2', '3', '--crf-weights', '0.5', '0'])
    o = opt.crf_options
    assert (o.radius, o.dilation, o.iters, o.theta, o.weights) == (5, 4, 10, (1.0, 2.0, 3.0), (0.5, 0.0))
    for lone in LONE_FLAGS:
        with pytest.raises(SystemExit):
            cli.parse_args(['val.json'] + lone)
        assert 'need --crf' in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.parse_args(['val.json', '--crf', '--crf-radius', '6'])
    assert 'radius' in capsys.readouterr().err
    with pytest.raises(ValueError, match='crf radius'):
        cli.test(None, None, crf=dict(radius=9))               # refused before the model or the data is touched


def test_inference_flags(capsys, monkeypatch, tmp_path):
    cli = _script('inference.py')
    seen = []
    monkeypatch.setattr(cli, 'run', lambda *a: seen.append(a))
    base = [str(tmp_path), str(tmp_path / 'out')]
    cli.main(base)
    printed = capsys.readouterr().out
    assert seen[-1][-1] is None and 'crf' not in printed        # the options line is what it was
    cli.main(base + ['--crf'])
    assert seen[-1][-1].radius == 3 and 'crf=True' in capsys.readouterr().out
    cli.main(base + ['--crf', '--crf-iters', '2', '--crf-weights', '1', '0'])
    assert (seen[-1][-1].iters, seen[-1][-1].weights) == (2, (1.0, 0.0))
    for lone in LONE_FLAGS:
        with pytest.raises(SystemExit):
            cli.main(base + lone)
        assert 'need --crf' in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.main(base + ['--crf', '--crf-dilation', '9'])
    assert 'dilation' in capsys.readouterr().err
    monkeypatch.undo()
    with pytest.raises(ValueError, match='crf iters'):
        cli.run(str(tmp_path), str(tmp_path / 'out'), (64, 64), 2, 'nowhere.pth', crf=dict(iters=0))
    with pytest.raises(ValueError, match='crf radius'):
        from pytorch_segmentation_amd.utils import inference
        inference(None, [], crf=dict(radius=0))


def test_nothing_is_imported_without_crf():
    """inference(..., crf=None) and test(..., crf=None) never load utils/crf.py; with crf= they do"""
    code = '''
import importlib.util, sys, types
import torch
from pytorch_segmentation_amd.utils import inference
spec = importlib.util.spec_from_file_location('pseg_cli', 'test.py')
cli = importlib.util.module_from_spec(spec)
spec.loader.exec_module(cli)
name = 'pytorch_segmentation_amd.utils.crf'
fetcher = types.SimpleNamespace(loader=types.SimpleNamespace(dataset=types.SimpleNamespace(classes=['a', 'b'])))
fetcher = type('F', (), {'loader': fetcher.loader, '__iter__': lambda self: iter(())})()
assert inference(None, [], crf=None) == [] and inference(None, [], scales=(0.5, 1.0), flip=True, crf=None) == []
assert inference(None, [], (64, 64), slide=True) == []
assert cli.test(torch.nn.Linear(1, 1), fetcher, crf=None) == 0.0 and cli.test(torch.nn.Linear(1, 1), fetcher) == 0.0
assert name not in sys.modules, 'utils/crf.py was imported without crf='
assert inference(None, [], crf=True) == [] and name in sys.modules
del sys.modules[name]
assert cli.test(torch.nn.Linear(1, 1), fetcher, crf={'iters': 2}) == 0.0 and name in sys.modules
print('ok')
'''
    out = subprocess.check_output([sys.executable, '-c', code], cwd=REPO)
    assert out.decode().strip().endswith('ok')


# ------------------------------------------------------------------ the entry points, host side
def test_entry_points_refuse_on_the_host():
    from pytorch_segmentation_amd import _lib
    from pytorch_segmentation_amd.csrc import build as csrc_build
    csrc_build.build(verbose=False)
    protos = _lib.prototypes()
    assert protos['pseg_crf_workspace_bytes'][0] is ctypes.c_int64 and len(protos['pseg_crf_workspace_bytes'][1]) == 4
    assert protos['pseg_crf_refine'][2] == ['logits', 'guide', 'B', 'C', 'h', 'w', 'g0', 'g1', 'g2', 'R', 'D', 'T', 'theta_alpha',
                                            'theta_beta', 'theta_gamma', 'w_a', 'w_s', 'out', 'workspace', 'workspace_bytes', 'stream']
    q = lambda *a: _lib.query('pseg_crf_workspace_bytes', *a)
    assert q(16, 21, 512, 512) == 2 * 16 * 512 * 512 * 24 * 4 and q(1, 8, 1, 2) == 2 * 64 and q(1, 9, 3, 3) == 2 * 432
    assert q(1, 3, 1, 3) == 2 * 96 and q(3, 256, 7, 5) == 2 * 3 * 35 * 1024
    for bad in ((0, 4, 8, 8), (65536, 4, 8, 8), (1, 0, 8, 8), (1, 257, 8, 8), (1, 4, 0, 8), (1, 4, 8, 65536), (1, 4, 1, 1),
                (64, 21, 1024, 1024)):
        assert q(*bad) == -1, bad
    # made-up addresses: every case is refused by the host-side checks, nothing is dereferenced or launched
    A = 0x7f0000000000
    good = dict(logits=A, guide=A + (1 << 30), B=1, C=4, h=6, w=7, g0=1.0, g1=1.0, g2=1.0, R=3, D=2, T=5, theta_alpha=8.0,
                theta_beta=13.0, theta_gamma=3.0, w_a=4.0, w_s=3.0, out=A, workspace=A + (2 << 30), workspace_bytes=1 << 20,
                stream=None)
    cases = [(dict(logits=None), 'null'), (dict(guide=None), 'null'), (dict(out=None), 'null'), (dict(workspace=None), 'null'),
             (dict(B=0), '65535'), (dict(h=65536), '65535'), (dict(h=1, w=1), '1 x 1'), (dict(C=0), 'classes'),
             (dict(C=257), 'classes'), (dict(R=0), 'radius'), (dict(R=6), 'radius'), (dict(D=0), 'dilation'), (dict(D=5), 'dilation'),
             (dict(T=0), 'iterations'), (dict(T=11), 'iterations'), (dict(theta_alpha=0.0), 'theta'),
             (dict(theta_beta=float('nan')), 'theta'), (dict(theta_gamma=float('inf')), 'theta'), (dict(theta_gamma=1e-25), 'overflows'),
             (dict(w_a=-0.5), 'weights'), (dict(w_s=float('nan')), 'weights'), (dict(g1=-1.0), 'guide scales'),
             (dict(g2=float('inf')), 'guide scales'), (dict(B=16, C=256, h=512, w=512), '2 GiB'), (dict(B=64, C=4, h=2048, w=2048), '2 GiB'),
             (dict(workspace=A + (2 << 30) + 8), 'aligned'), (dict(workspace_bytes=2 * 6 * 7 * 8 * 4 - 1), 'too small'),
             (dict(out=A + (2 << 30) + 64), 'inside the workspace'), (dict(out=A + (1 << 30)), 'guide')]
    for change, match in cases:
        with pytest.raises(_lib.PsegError, match=match):
            _lib.call('pseg_crf_refine', *dict(good, **change).values())
