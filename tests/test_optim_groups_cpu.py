"""Host side of the grouped optimiser step: the fp64 restatement against torch.optim, the learning-rate schedules, the run
tables of ParamArena.runs, the command-line flags, and the refusals of the entry points (csrc/optim.hip).  No GPU."""
import math

import numpy as np
import pytest
import torch

import optim_ref
from optim_ref import f32
from pytorch_segmentation_amd import _lib
from pytorch_segmentation_amd.arena import RUN_BLOCK_CAP, RUN_SPAN, ParamArena, make_runs, pack_runs, run_blocks
from pytorch_segmentation_amd.csrc import build as csrc_build
from pytorch_segmentation_amd.utils.schedule import lr_at


@pytest.fixture(scope='module')
def lib():
    csrc_build.build(verbose=False)
    return _lib.load()


# ------------------------------------------------------------------------------------------------ the restatement
SMALL_RUNS = [(0, 8, 0, 0.5, 1e-2), (8, 4, 1, 0.0, 5e-3), (12, 1020, 2, 2.0, 0.0), (1032, 2000, 3, 0.1, 2e-2)]


@pytest.mark.parametrize('name,adam,decoupled,mu,nesterov', [
    ('sgd', False, False, 0.0, False), ('sgd-momentum', False, False, 0.9, False), ('sgd-nesterov', False, False, 0.9, True),
    ('adam', True, False, 0.0, False), ('adamw', True, True, 0.0, False)])
@pytest.mark.parametrize('max_norm', [0.0, 1e9, 3.0])
def test_restatement_is_torch_optim_in_fp64(name, adam, decoupled, mu, nesterov, max_norm):
    """grouped_step == torch.optim.SGD / Adam / AdamW on one param group per run + clip_grad_norm_ + a hand-written EMA, all in
    fp64, three steps: 1e-12 absolute on values of order 1.  max_norm 3.0 clips (the norm is ~16), 1e9 does not."""
    n = SMALL_RUNS[-1][0] + SMALL_RUNS[-1][1]
    g0 = torch.Generator().manual_seed(5)
    p0 = torch.rand(n, generator=g0, dtype=torch.float64) * 2 - 1
    grads = [torch.rand(n, generator=g0, dtype=torch.float64) * 2 - 1 for _ in range(3)]
    kw = dict(lr=0.1 if not adam else 1e-2, nesterov=nesterov, decoupled=decoupled, grad_scale=0.5, max_norm=max_norm)
    ref = optim_ref.restatement_run(p0, grads, SMALL_RUNS, adam, ema_decay=0.9, momentum=mu, **kw)
    tor = optim_ref.torch_recipe(p0, grads, SMALL_RUNS, adam, momentum=mu, ema_decay=0.9, dtype=torch.float64, **kw)
    for k in ('p', 'm', 'v', 'ema'):
        assert (ref[k] is None) == (tor[k] is None), k
        if ref[k] is not None:
            assert (ref[k] - tor[k]).abs().max().item() < 1e-12, (name, k)
    if max_norm == 3.0:
        assert ref['clipped'] == 3 and ref['coef'] < 1.0
    if max_norm == 1e9:
        assert ref['clipped'] == 0 and ref['coef'] == 1.0
    # the run with lr_mult 0 keeps its parameters, its moments move
    assert torch.equal(ref['p'][8:12], p0[8:12])
    if ref['m'] is not None:
        assert ref['m'][8:12].abs().min().item() > 0


def test_restatement_mp_skip_changes_nothing():
    p0 = torch.linspace(-1, 1, 16, dtype=torch.float64)
    st = optim_ref.new_state(p0, True, 0.0, True)
    before = {k: v.clone() for k, v in st.items() if torch.is_tensor(v)}
    runs = [(0, 16, 0, 1.0, 1e-2)]
    assert optim_ref.grouped_step(st, torch.ones(16, dtype=torch.float64), runs, True, 1e-2, max_norm=1.0, ema_decay=0.9,
                                  mp={'inv_scale': 1 / 1024.0, 'found': True}) is False
    assert all(torch.equal(st[k], v) for k, v in before.items()) and 'coef' not in st
    assert optim_ref.grouped_step(st, torch.ones(16, dtype=torch.float64) * 1024, runs, True, 1e-2, max_norm=1.0, ema_decay=0.9,
                                  mp={'inv_scale': 1 / 1024.0, 'found': False}) is True
    assert abs(st['norm'] - 4.0) < 1e-12 and abs(st['coef'] - 1.0 / (4.0 + 1e-6)) < 1e-12


# ------------------------------------------------------------------------------------------------ schedules
def test_lr_at_formulas():
    base, total, warm, power, lo = 0.1, 50, 5, 0.9, 1e-4
    for t in range(0, 60):
        for sched in ('poly', 'cosine'):
            got = lr_at(t, base, sched, total, warm, power, lo)
            if t >= total:
                want = lo
            elif t < warm:
                want = base * (t + 1) / warm
            else:
                u = (t - warm) / (total - warm)
                want = max(lo, base * (1 - u) ** power) if sched == 'poly' else lo + (base - lo) * (1 + math.cos(math.pi * u)) / 2
            assert got == pytest.approx(want, rel=1e-15, abs=0), (sched, t)
        assert lr_at(t, base) == base and lr_at(t, base, None, total, warm) == base
    for bad in (dict(schedule='step', total_steps=10), dict(schedule='poly'), dict(schedule='poly', total_steps=10, warmup_steps=10)):
        with pytest.raises(ValueError):
            lr_at(0, base, **bad)


def test_lr_at_poly_is_torch_polynomial_lr_step_for_step():
    base, total, power = 0.1, 40, 0.9
    p = torch.zeros(1, requires_grad=True)
    opt = torch.optim.SGD([p], lr=base)
    sched = torch.optim.lr_scheduler.PolynomialLR(opt, total_iters=total, power=power)
    for t in range(total + 3):
        # (torch's chained form multiplies a ratio into the rate every step: a few roundings per step)
        assert opt.param_groups[0]['lr'] == pytest.approx(lr_at(t, base, 'poly', total, 0, power, 0.0), rel=1e-12, abs=1e-17), t
        opt.step()
        sched.step()


@pytest.mark.parametrize('sched', ['poly', 'cosine'])
def test_lr_at_shape(sched):
    base, total, warm, lo = 0.05, 100, 10, 1e-5
    lrs = [lr_at(t, base, sched, total, warm, 0.9, lo) for t in range(total + 5)]
    assert lrs[warm - 1] == base and lrs[warm] == base            # the warm-up ends on base_lr, the curve starts from it
    assert all(a < b for a, b in zip(lrs[:warm - 1], lrs[1:warm]))
    assert all(a >= b for a, b in zip(lrs[warm:], lrs[warm + 1:]))  # monotone afterwards
    assert lrs[total] == lo and lrs[-1] == lo and min(lrs[warm:]) >= lo
    assert lrs[total - 1] > lo


# ------------------------------------------------------------------------------------------------ run tables
def _per_float(arena, runs):
    lm, wd = np.full(arena.numel, np.nan), np.full(arena.numel, np.nan)
    for off, cnt, _, a, b in runs:
        assert np.isnan(lm[off:off + cnt]).all(), 'overlap'
        lm[off:off + cnt], wd[off:off + cnt] = a, b
    assert not np.isnan(lm).any(), 'gap'
    return lm, wd


def _check_table(arena, runs):
    assert runs[0][0] == 0 and runs[-1][0] + runs[-1][1] == arena.numel
    blocks = 0
    for i, (off, cnt, first, lm, wd) in enumerate(runs):
        assert off % 4 == 0 and cnt % 4 == 0 and cnt > 0
        assert first == blocks
        blocks += run_blocks(cnt)
        if i:
            prev = runs[i - 1]
            assert prev[0] + prev[1] == off                       # no gap, no overlap
            assert (prev[3], prev[4]) != (lm, wd)                 # equal neighbours are merged
    arr, total = pack_runs(runs)
    assert total == blocks and arr.dtype.itemsize == 32 and len(arr) == len(runs)
    assert run_blocks(1) == 1 and run_blocks(RUN_SPAN + 1) == 2 and run_blocks(10 ** 9) == RUN_BLOCK_CAP


@pytest.fixture(scope='module', params=['unet', 'deeplabv3plus'])
def cpu_arena(request):
    from pytorch_segmentation_amd.models import DeepLabV3Plus, UNet
    model = UNet(3) if request.param == 'unet' else DeepLabV3Plus(21)
    return model, ParamArena(model, 'cpu')


def test_runs_cover_the_arena_and_merge(cpu_arena):
    model, arena = cpu_arena
    one = arena.runs(lambda key, module, name: (1.0, 1e-4))
    assert one == [(0, arena.numel, 0, 1.0, f32(1e-4))]
    keys = []
    alternating = arena.runs(lambda key, module, name: (keys.append(key) or 1.0, float(len(keys) % 2)))
    assert len(alternating) == len(arena.segments)
    _check_table(arena, alternating)
    assert sorted(keys) == sorted(k for k, _ in model.named_parameters())


def test_runs_no_decay_on_norm_and_bias(cpu_arena):
    model, arena = cpu_arena
    wd0 = 1e-4

    def rule(key, module, name):
        return 1.0, (0.0 if isinstance(module, torch.nn.BatchNorm2d) or name == 'bias' else wd0)
    runs = arena.runs(rule)
    _check_table(arena, runs)
    assert 1 < len(runs) < len(arena.segments)
    _, wd = _per_float(arena, runs)
    seen = {'norm': 0, 'bias': 0, 'weight': 0}
    for seg in arena.segments:
        got = wd[seg.offset:seg.offset + seg.numel]
        if isinstance(seg.module, torch.nn.BatchNorm2d) or seg.name == 'bias':
            assert (got == 0).all(), arena.key_of(seg)
            seen['norm' if isinstance(seg.module, torch.nn.BatchNorm2d) else 'bias'] += 1
        else:
            assert isinstance(seg.module, torch.nn.Conv2d) and seg.name == 'weight', arena.key_of(seg)
            assert (got == f32(wd0)).all(), arena.key_of(seg)
            seen['weight'] += 1
    assert seen['norm'] > 0 and seen['weight'] > 0


def test_runs_backbone_factor_lands_on_the_backbone(cpu_arena):
    model, arena = cpu_arena
    factors = {'backbone.': 0.1}
    runs = arena.runs(lambda key, module, name: (next((f for p, f in factors.items() if key.startswith(p)), 1.0), 0.0))
    _check_table(arena, runs)
    lm, _ = _per_float(arena, runs)
    b, e = arena.range_of(model.backbone)
    want = np.ones(arena.numel)
    want[b:e] = f32(0.1)
    assert (lm == want).all() and e - b > 0 and e - b < arena.numel
    own = set(id(p) for p in model.backbone.parameters())
    assert all((id(s.param) in own) == (b <= s.offset < e) for s in arena.segments)


def test_make_runs_merges_only_touching_equal_rows():
    t = make_runs([(0, 8, 1.0, 0.1), (8, 4, 1.0, 0.1), (12, 4, 1.0, 0.2), (20, 4, 1.0, 0.2), (24, 4096, 0.5, 0.2)])
    a, b = f32(0.1), f32(0.2)
    assert t == [(0, 12, 0, 1.0, a), (12, 4, 1, 1.0, b), (20, 4, 2, 1.0, b), (24, 4096, 3, 0.5, b)]
    assert pack_runs(t)[1] == 3 + 4


# ------------------------------------------------------------------------------------------------ command line
def test_train_flags_reach_the_trainer(monkeypatch):
    import train
    ap = train.build_parser()
    assert train.optim_from_options(ap.parse_args(['data/x'])) == {}
    opt = ap.parse_args(['data/x', '--weight-decay', '1e-4', '--momentum', '0.8', '--adamw', '--no-decay-norm-bias',
                         '--backbone-lr-mult', '0.1', '--clip-grad', '5', '--ema-decay', '0.999', '--schedule', 'poly',
                         '--warmup-steps', '7', '--min-lr', '1e-6'])
    kw = train.optim_from_options(opt)
    assert kw == dict(weight_decay=1e-4, momentum=0.8, adamw=True, no_decay_norm_bias=True, lr_mult={'backbone.': 0.1},
                      max_grad_norm=5.0, ema_decay=0.999, schedule='poly', warmup_steps=7, min_lr=1e-6)
    assert ap.parse_args(['data/x', '--schedule', 'cosine']).schedule == 'cosine'
    with pytest.raises(SystemExit):
        ap.parse_args(['data/x', '--schedule', 'step'])
    for bad in (['--ema-decay', '1'], ['--clip-grad', '-1'], ['--warmup-steps', '3']):
        with pytest.raises(ValueError):
            train.optim_from_options(ap.parse_args(['data/x'] + bad))

    class Data:
        classes = ['a', 'b', 'c']
        post_fetch_fn = None
    seen = {}

    class FakeTrainer:
        def __init__(self, model, fetcher, **kwargs):
            seen.update(kwargs)
            self.epoch = 10 ** 9
    monkeypatch.setattr(train, 'CocoInstance', lambda *a, **k: Data())
    monkeypatch.setattr(train, '_loader', lambda *a, **k: list(range(11)))
    monkeypatch.setattr(train, 'Fetcher', lambda loader, *a, **k: loader)
    monkeypatch.setattr(train, 'MODELS', {'unet': lambda nc: 'model'})
    monkeypatch.setattr(train, 'Trainer', FakeTrainer)
    monkeypatch.setattr(train, 'OPTIM', kw)
    train.train('data/x', epochs=6, accumulate=2, notest=True)
    for k, v in kw.items():
        assert seen[k] == v, k
    assert seen['total_steps'] == 6 * (11 // 2)
    seen.clear()
    monkeypatch.setattr(train, 'OPTIM', {})
    train.train('data/x', epochs=6, accumulate=2, notest=True)
    assert sorted(seen) == ['accumulate', 'adam', 'loss_fn', 'lr', 'mixed_precision', 'resume', 'weights', 'workdir']


def test_trainer_keywords_come_last():
    import inspect
    from pytorch_segmentation_amd.utils import FlatOptimizer, Trainer
    names = list(inspect.signature(Trainer.__init__).parameters)
    assert names[-10:] == ['no_decay_norm_bias', 'lr_mult', 'max_grad_norm', 'ema_decay', 'adamw', 'schedule', 'warmup_steps',
                           'total_steps', 'poly_power', 'min_lr']
    assert names[names.index('no_decay_norm_bias') - 1] == 'max_graphs'
    assert list(inspect.signature(FlatOptimizer.__init__).parameters)[-4:] == ['runs', 'max_grad_norm', 'ema_decay', 'decoupled']


def test_ema_flag_of_test_and_inference(tmp_path):
    import inference
    import test as test_cli
    assert test_cli.parse_args(['val.json']).ema is False and test_cli.parse_args(['val.json', '--ema']).ema is True
    ck = {'model': {'w': 1}, 'model_ema': {'w': 2}}
    assert test_cli.checkpoint_weights(ck) == {'w': 1} and test_cli.checkpoint_weights(ck, ema=True) == {'w': 2}
    with pytest.raises(KeyError, match="holds no 'model_ema'"):
        test_cli.checkpoint_weights({'model': {}}, ema=True, path='old.pt')
    path = tmp_path / 'old.pt'
    torch.save({'model': {}}, path)
    (tmp_path / 'in').mkdir()
    with pytest.raises(KeyError, match="holds no 'model_ema'"):
        inference.run(str(tmp_path / 'in'), str(tmp_path / 'out'), (64, 64), 2, str(path), model_name='unet', ema=True)


# ------------------------------------------------------------------------------------------------ refusals
A, MIS = 0x7f0000000000, 0x7f0000000004            # 16-byte aligned / misaligned made-up device addresses


def _sgd_args(table, total, n, param=A, ema=None, max_norm=0.0, decay=0.0, clip=A, host=None):
    host = table if host is None else host
    return ('pseg_opt_step_sgd', param, A, A, ema, n, A, host.ctypes.data, len(host), total, 0.1, 0.9, 0, 0, 1.0, 1,
            max_norm, decay, clip, None, None)


def _adam_args(table, total, n, param=A, ema=None, max_norm=0.0, decay=0.0, clip=A):
    return ('pseg_opt_step_adam', param, A, A, A, ema, n, A, table.ctypes.data, len(table), total, 1e-3, 0.9, 0.999, 1e-8, 0,
            1.0, 1, max_norm, decay, clip, None, None)


@pytest.mark.skipif(torch.cuda.is_available(), reason='uses made-up device addresses: host-side checks only')
def test_refusals_say_which_check_failed(lib):
    """every case is refused by the host-side checks, so nothing is launched and no address is dereferenced"""
    def refused(args, match):
        with pytest.raises(_lib.PsegError, match=match):
            _lib.call(*args)
    good, total = pack_runs(make_runs([(0, 8, 1.0, 0.0), (8, 2048, 0.5, 1e-2)]))
    n = 2056
    for mk in (_sgd_args, _adam_args):
        refused(mk(good, total, n, param=MIS), 'alignment')
        refused(mk(good, total, n, ema=MIS, decay=0.5), 'alignment')
        refused(mk(good, total, n, decay=1.0), r'decay must be in \[0, 1\)')
        refused(mk(good, total, n, max_norm=-1.0), 'max_norm must be >= 0')
        refused(mk(good, total, n, max_norm=1.0, clip=None), 'needs clip_state')
        refused(mk(good, total, n - 4), 'the arena holds')
        refused(mk(good, total + 1, n), 'blocks')
        overlap, _ = pack_runs([(0, 8, 0, 1.0, 0.0), (4, 2048, 1, 1.0, 0.0)])
        refused(mk(overlap, 3, n), 'overlap')
        odd, _ = pack_runs([(0, 6, 0, 1.0, 0.0), (8, 2048, 1, 1.0, 0.0)])
        refused(mk(odd, 3, n), 'multiples of 4')
        odd_off, _ = pack_runs([(0, 4, 0, 1.0, 0.0), (6, 2048, 1, 1.0, 0.0)])
        refused(mk(odd_off, 3, n), 'multiples of 4')
        fat, _ = pack_runs([(0, 8, 0, 1.0, 0.0), (8, 2048, 2, 1.0, 0.0)])       # two blocks for a run of 8 floats
        refused(mk(fat, 4, n), 'blocks for')
    refused(('pseg_opt_step_sgd', A, A, None, None, n, A, good.ctypes.data, len(good), total, 0.1, 0.9, 0, 0, 1.0, 1, 0.0, 0.0,
             None, None, None), 'momentum needs a buffer')
    refused(('pseg_grad_sumsq', MIS, 1024, A, 8192, A, None), 'alignment')
    refused(('pseg_grad_sumsq', A, 1022, A, 8192, A, None), 'multiple of 4')
    refused(('pseg_grad_sumsq', A, 1 << 20, A, 8, A, None), 'workspace')


def test_sumsq_workspace_query(lib):
    q = lambda n: _lib.query('pseg_grad_sumsq_workspace_bytes', n)
    assert q(4) == 8 and q(1024) == 8 and q(1028) == 16 and q(1 << 20) == 8 * 1024 and q(1 << 30) == 8 * 1024 and q(0) == 0
