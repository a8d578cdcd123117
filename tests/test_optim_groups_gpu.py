"""The grouped optimiser step on the device (csrc/optim.hip): pseg_grad_sumsq, pseg_opt_step_sgd / pseg_opt_step_adam,
and the Trainer / command-line options built on them, against the fp64 restatement of tests/optim_ref.py.

Sizes (optim_ref.five_runs): runs of 4, 8, 1020 (less than a block's span of 1024), 5000 (five blocks, no multiple of the
span) and 2 097 152 floats -- blocks per run are capped at 1024 (arena.RUN_BLOCK_CAP), 1024 blocks x 1024 floats cover
1 048 576 per trip, so every thread of the last run's blocks makes exactly two trips.  2 103 184 floats in all.

Bounds of the per-element checks: four times the distance of torch's own fp32 CPU run of the same recipe (one param group
per run, clip_grad_norm_, optimizer.step(), hand-written EMA) from the fp64 restatement, in elem_fig, per tensor.  Measured on
the CPU with the inputs of these tests by

    python tests/optim_ref.py
    sgd   p 2.68e-04 m 4.33e-04 ema 6.05e-06
    adam  p 9.45e-03 m 4.30e-04 v 1.17e-04 ema 2.64e-04
    adamw p 2.94e-06 m 1.34e-04 v 5.30e-05 ema 2.85e-07

(torch's fp32 norm of the 2.1 M gradients is 2.5e-5 off, which every clipped gradient inherits; coupled Adam divides a
gradient by its own magnitude, so an element whose clipped gradient and decay term cancel carries that error at full size.)
"""
import json
import os

import pytest
import torch

import optim_bits
import optim_ref as R
from optim_bits import Table, opt_adam, opt_sgd, run_five, sumsq
from optim_ref import f32
from oracle import fill

pytestmark = pytest.mark.gpu

D = {'sgd': {'p': 2.68e-04, 'm': 4.33e-04, 'ema': 6.05e-06},
     'adam': {'p': 9.45e-03, 'm': 4.30e-04, 'v': 1.17e-04, 'ema': 2.64e-04},
     'adamw': {'p': 2.94e-06, 'm': 1.34e-04, 'v': 5.30e-05, 'ema': 2.85e-07}}
BOUND_FACTOR = 4.0
ADAM_HYPER = dict(lr=f32(1e-2), betas=(f32(0.9), f32(0.999)), eps=f32(1e-8))


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    from pytorch_segmentation_amd import ops as _ops
    return _ops


@pytest.fixture(scope='module')
def lib():
    from pytorch_segmentation_amd import _lib
    return _lib


@pytest.fixture(scope='module')
def case():
    """inputs and fp64 references of the five-run table, computed once: {variant: [state after step 1, 2, 3]}"""
    c = optim_bits.five_run_case()
    runs, p0, grads = c['runs'], c['p0'], c['grads']
    refs = {}
    for name, adam, decoupled, mu, nesterov, gscale in R.VARIANTS:
        st = R.new_state(p0, adam, f32(mu), True)
        for i, g in enumerate(grads):
            R.grouped_step(st, g.double(), runs, adam, momentum=f32(mu), nesterov=nesterov, decoupled=decoupled,
                           grad_scale=f32(gscale), step=i + 1, max_norm=R.MAX_NORM, ema_decay=R.EMA_DECAY, **R.HYPER[name])
        refs[name] = st
    return dict(c, refs=refs)


def one_run(n):
    from pytorch_segmentation_amd.arena import run_blocks
    return Table([(0, n, 0, 1.0, 0.0)], run_blocks(n))


def with_wd(tab_rows, wd):
    return [(o, c, b, lm, f32(wd)) for o, c, b, lm, _ in tab_rows]


# ------------------------------------------------------------------------------------------------ 1. bit identity
def test_step_bits_match_recorded(ops, lib, golden_dir):
    """every step entry point (tests/optim_bits.py: the four flat ones at n = 3, 1027 and 2 098 179, the grouped ones over the
    five-run table with clip and EMA, fp32 and -mp) leaves, after three steps, the bytes recorded in
    tests/golden/optim_step_bits.json from the kernels as they stood before they were merged into one per rule"""
    with open(os.path.join(golden_dir, 'optim_step_bits.json')) as f:
        rec = json.load(f)
    got = optim_bits.digests(lib, ops)
    assert sorted(got) == sorted(rec['digests'])
    for name, tensors in got.items():
        assert sorted(tensors) == sorted(rec['digests'][name]), name
        for k, h in tensors.items():
            assert h == rec['digests'][name][k], \
                'case %s, tensor %s: sha256 %s, recorded %s (recorded under "%s", installed "%s")' % (
                    name, k, h, rec['digests'][name][k], rec['compiler'], optim_bits.compiler_line())


# (a one-run table and a flat entry point reach the same kernel: these pin the two host paths to it against each other)
# name, momentum, weight decay, nesterov, grad_scale
SGD_ID = [('plain-null-buffer', 0.0, 0.0, False, 1.0), ('momentum-wd', 0.9, 1e-2, False, 0.5), ('nesterov-wd', 0.9, 1e-2, True, 0.25)]
# name, weight decay, decoupled, grad_scale
ADAM_ID = [('plain', 0.0, False, 1.0), ('wd', 1e-2, False, 0.5), ('adamw', 1e-2, True, 0.5)]


@pytest.mark.parametrize('mp', [False, True])
def test_one_run_reproduces_sgd_step_bit_for_bit(ops, lib, case, mp):
    """a one-run table with lr_mult 1, no clip and no EMA against pseg_sgd_step / pseg_sgd_step_mp, three steps, torch.equal on
    parameters and momentum buffer: momentum 0 with a NULL buffer, coupled decay, Nesterov, grad_scale != 1"""
    n, lr, S = case['n'], f32(0.1), 1024.0
    for name, mu, wd, nesterov, gscale in SGD_ID:
        mu, wd, gscale = f32(mu), f32(wd), f32(gscale)
        tab = one_run(n)
        tab = Table(with_wd(tab.rows, wd), tab.blocks)
        pa, pb = case['p0'].cuda(), case['p0'].cuda()
        ba, bb = (torch.zeros(n, device='cuda'), torch.zeros(n, device='cuda')) if mu != 0 else (None, None)
        sa, sb = torch.zeros(8, device='cuda'), torch.zeros(8, device='cuda')
        for s in (sa, sb):
            lib.call('pseg_mp_state_init', s.data_ptr(), S, ops._stream())
        for i, g in enumerate(case['grads']):
            gd = (g * S).cuda() if mp else g.cuda()
            if mp:
                lib.call('pseg_sgd_step_mp', pa.data_ptr(), gd.data_ptr(), ops._ptr(ba), n, lr, mu, wd, int(nesterov), gscale,
                         sa.data_ptr(), ops._stream())
                opt_sgd(lib, ops, tab, pb, gd, bb, None, lr, mu, nesterov, False, gscale, 0, mp=sb)
                sa[4] += 1.0
                sb[4] += 1.0
            else:
                lib.call('pseg_sgd_step', pa.data_ptr(), gd.data_ptr(), ops._ptr(ba), n, lr, mu, wd, int(nesterov), gscale,
                         int(i == 0), ops._stream())
                opt_sgd(lib, ops, tab, pb, gd, bb, None, lr, mu, nesterov, False, gscale, i == 0)
            assert torch.equal(pa, pb), (name, i)
            assert ba is None or torch.equal(ba, bb), (name, i)
        assert not torch.equal(pa.cpu(), case['p0'])


@pytest.mark.parametrize('mp', [False, True])
def test_one_run_reproduces_adam_step_bit_for_bit(ops, lib, case, mp):
    """the same against pseg_adam_step / pseg_adam_step_mp: no decay, coupled and decoupled decay, grad_scale != 1; torch.equal
    on parameters, exp_avg and exp_avg_sq after each of three steps"""
    n, S = case['n'], 1024.0
    lr, (b1, b2), eps = ADAM_HYPER['lr'], ADAM_HYPER['betas'], ADAM_HYPER['eps']
    for name, wd, decoupled, gscale in ADAM_ID:
        wd, gscale = f32(wd), f32(gscale)
        tab = one_run(n)
        tab = Table(with_wd(tab.rows, wd), tab.blocks)
        A = [case['p0'].cuda(), torch.zeros(n, device='cuda'), torch.zeros(n, device='cuda')]
        B = [t.clone() for t in A]
        sa, sb = torch.zeros(8, device='cuda'), torch.zeros(8, device='cuda')
        for s in (sa, sb):
            lib.call('pseg_mp_state_init', s.data_ptr(), S, ops._stream())
        for i, g in enumerate(case['grads']):
            gd = (g * S).cuda() if mp else g.cuda()
            if mp:
                lib.call('pseg_adam_step_mp', A[0].data_ptr(), gd.data_ptr(), A[1].data_ptr(), A[2].data_ptr(), n, lr, b1, b2,
                         eps, wd, int(decoupled), gscale, sa.data_ptr(), ops._stream())
                opt_adam(lib, ops, tab, B[0], gd, B[1], B[2], None, lr, (b1, b2), eps, decoupled, gscale, 0, mp=sb)
                sa[4] += 1.0
                sb[4] += 1.0
            else:
                lib.call('pseg_adam_step', A[0].data_ptr(), gd.data_ptr(), A[1].data_ptr(), A[2].data_ptr(), n, lr, b1, b2, eps,
                         wd, int(decoupled), gscale, i + 1, ops._stream())
                opt_adam(lib, ops, tab, B[0], gd, B[1], B[2], None, lr, (b1, b2), eps, decoupled, gscale, i + 1)
            for a, b, what in zip(A, B, ('param', 'exp_avg', 'exp_avg_sq')):
                assert torch.equal(a, b), (name, i, what)
        assert not torch.equal(A[0].cpu(), case['p0'])


# ------------------------------------------------------------------------------------------------ 2. per element
def check_elements(tag, name, got, ref, runs):
    """every tensor per element (elem_fig) and the first and last element of every run on their own"""
    edges = sorted(set(i for o, c, _, _, _ in runs for i in (o, o + c - 1)))
    for k, t in got.items():
        g, r = t.detach().cpu().double(), ref[k]
        bound = BOUND_FACTOR * D[name][k]
        e = R.elem_fig(g, r)
        peak = r.abs().max().item()
        e_edge = max(abs(g[i].item() - r[i].item()) / max(abs(r[i].item()), 1e-2 * peak, 1e-300) for i in edges)
        print('%s %s: per-element %.2e, run edges %.2e (bound %.2e)' % (tag, k, e, e_edge, bound))
        assert e < bound and e_edge < bound, (tag, k, e, e_edge, bound)


@pytest.mark.parametrize('mp', [False, True])
@pytest.mark.parametrize('name', [v[0] for v in R.VARIANTS])
def test_five_runs_per_element(ops, lib, case, name, mp):
    """SGD (Nesterov), Adam and AdamW over the five-run table (distinct lr_mult, one 0; distinct decay, one 0), three steps, clip
    and EMA on, fp32 and -mp, against the restatement: parameters, moments and EMA per element and at every run's first and last
    element, bound 4 x D (module docstring).  The run with lr_mult 0 keeps its parameters bit for bit while its moments move.
    clip_state holds the coefficient and the norm of the last step (four fp32 roundings: 2^-21) and counts three clipped steps."""
    got, clip, state = run_five(ops, lib, case, name, mp)
    ref = case['refs'][name]
    check_elements('%s%s' % (name, '-mp' if mp else ''), name, got, ref, case['runs'])
    o, c = case['runs'][1][0], case['runs'][1][1]
    assert case['runs'][1][3] == 0.0
    assert torch.equal(got['p'][o:o + c].cpu(), case['p0'][o:o + c])
    assert (got['m'][o:o + c] != 0).all()
    assert clip[3].item() == 3.0
    assert abs(clip[1].item() - ref['coef']) < 2.0 ** -21 * ref['coef'], (clip[1].item(), ref['coef'])
    assert abs(clip[2].item() - ref['norm']) < 2.0 ** -21 * ref['norm'], (clip[2].item(), ref['norm'])
    if mp:
        assert state[4].item() == 3.0 and state[5].item() == 0.0 and state[0].item() == 1024.0


# ------------------------------------------------------------------------------------------------ 3. clipping
def test_grad_norm_is_fp64_accurate_and_reproducible(ops, lib, case):
    """clip_state[0] is the fp64 norm rounded once to fp32 (2^-23 relative is asserted), the same bits from call to call, at
    n = 4 (one vector), 1028 (two blocks, the second with one vector) and 2 103 184 (the 1024-block cap, three trips); entries
    of 1e30 give a finite norm because the squares are fp64."""
    for n in (4, 1028, case['n']):
        g = case['grads'][0][:n].cuda()
        want = float((g.double() ** 2).sum().sqrt().item())
        c1, c2 = torch.zeros(4, device='cuda'), torch.zeros(4, device='cuda')
        sumsq(lib, ops, g, c1)
        sumsq(lib, ops, g, c2)
        got = c1.cpu()
        print('n=%d norm %.9g fp64 %.17g rel %.2e' % (n, got[0].item(), want, abs(got[0].item() - want) / want))
        assert abs(got[0].item() - want) <= 2.0 ** -23 * want
        assert torch.equal(c1, c2) and (got[1:] == 0).all()
    big = torch.zeros(4096, device='cuda')
    big[5], big[4095] = 1e30, -1e30
    c = torch.zeros(4, device='cuda')
    sumsq(lib, ops, big, c)
    want = 1e30 * 2 ** 0.5
    assert torch.isfinite(c[0]).item() and abs(c[0].item() - want) <= 2.0 ** -23 * want


@pytest.mark.parametrize('name', ['sgd', 'adam'])
def test_max_norm_above_the_norm_changes_nothing(ops, lib, case, name):
    """max_norm above the norm: the coefficient is exactly 1, nothing is counted, and the step is bit-identical to the unclipped
    one (the norm of the gradients is ~837 x grad_scale 0.5)"""
    loose, clip, _ = run_five(ops, lib, case, name, False, max_norm=f32(1e4), steps=2)
    free, clip0, _ = run_five(ops, lib, case, name, False, max_norm=0.0, steps=2)
    assert clip[1].item() == 1.0 and clip[3].item() == 0.0 and 400 < clip[2].item() < 440
    assert (clip0 == 0).all()
    for k in free:
        assert torch.equal(loose[k], free[k]), k


# ------------------------------------------------------------------------------------------------ 4. -mp skip
@pytest.mark.parametrize('name', ['sgd', 'adamw'])
def test_mp_skip_leaves_everything_unchanged(ops, lib, case, name):
    """one inf among the gradients: after pseg_mp_check the grouped step writes nothing -- parameters, moments, EMA and
    clip_state[1..3] keep their bits -- and pseg_mp_update backs the scale off and counts the skip"""
    got, clip, state = run_five(ops, lib, case, name, True, steps=1)
    _, adam, decoupled, mu, nesterov, gscale = next(v for v in R.VARIANTS if v[0] == name)
    before = {k: t.clone() for k, t in got.items()}
    n, h = case['n'], R.HYPER[name]
    tab = Table(case['runs'], case['blocks'])
    sd = state.cuda()
    cd = clip.cuda()
    g = (case['grads'][1] * 1024.0).cuda()
    g[case['runs'][3][0] + 17] = float('inf')
    lib.call('pseg_mp_check', g.data_ptr(), n, sd.data_ptr(), ops._stream())
    assert sd[3].item() == 1.0
    sumsq(lib, ops, g, cd)
    if adam:
        opt_adam(lib, ops, tab, got['p'], g, got['m'], got['v'], got['ema'], h['lr'], h['betas'], h['eps'], decoupled, f32(gscale),
                 2, R.MAX_NORM, R.EMA_DECAY, cd, sd)
    else:
        opt_sgd(lib, ops, tab, got['p'], g, got['m'], got['ema'], h['lr'], f32(mu), nesterov, decoupled, f32(gscale), False,
                R.MAX_NORM, R.EMA_DECAY, cd, sd)
    for k in before:
        assert torch.equal(got[k], before[k]), k
    assert torch.equal(cd.cpu()[1:], clip[1:]) and torch.isinf(cd[0]).item()
    lib.call('pseg_mp_update', sd.data_ptr(), 2.0, 0.5, 2000, 1.0, float(2 ** 24), ops._stream())
    s = sd.cpu().tolist()
    assert s[0] == 512.0 and s[1] == 1.0 / 512.0 and s[3] == 0.0 and s[4] == 1.0 and s[5] == 1.0


# ------------------------------------------------------------------------------------------------ 5. Trainer
OPTIONS = dict(adam=True, lr=1e-2, weight_decay=1e-2, no_decay_norm_bias=True, lr_mult={'backbone.': 0.1}, max_grad_norm=0.5,
               ema_decay=0.9, adamw=True, schedule='poly', warmup_steps=2, total_steps=10, poly_power=0.9, min_lr=1e-5)
OPT_CALLS = {'pseg_sgd_step', 'pseg_adam_step', 'pseg_sgd_step_mp', 'pseg_adam_step_mp', 'pseg_mp_check', 'pseg_mp_update',
             'pseg_grad_sumsq', 'pseg_opt_step_sgd', 'pseg_opt_step_adam'}


def _batch(i):
    return (fill.images('optg/x%d' % i, (2, 3, 64, 64)).cuda(), fill.labels('optg/t%d' % i, (2, 64, 64), 3, block=8).cuda())


def _snapshot(tr):
    o = tr.optimizer
    return {'p': tr.arena.params.detach().cpu().clone(), 'm': o.m.cpu().clone(), 'v': o.v.cpu().clone(), 'ema': o.ema.cpu().clone()}


@pytest.mark.parametrize('mp', [False, True])
def test_trainer_with_every_option(ops, lib, tmp_path, monkeypatch, mp):
    """UNet(3) at 2 x 3 x 64 x 64, AdamW with no decay on norm parameters and biases, a backbone factor, clip, EMA and a poly
    schedule with warm-up, fp32 and -mp.  After each of three steps (five under -mp, whose first two overflow at the initial loss scale and are skipped) the arena, moments and EMA are the restatement applied to
    the state before the step and the gradients the step left in the arena (bounds: 'adamw' of the module docstring), with the
    scheduled learning rate; graph=True (eager, captured, replayed, replayed) equals graph=False bit for bit after one more step;
    save() + Trainer(resume=True) takes that step bit-identically at the scheduled rate; 'model_ema' is the state dict under
    ema_weights() and (fp32) gives the same eval logits in a fresh model; leaving ema_weights() restores the parameters."""
    from pytorch_segmentation_amd import _lib, models
    from pytorch_segmentation_amd.utils import Trainer, compute_loss
    from pytorch_segmentation_amd.utils.schedule import lr_at
    torch.manual_seed(0)
    init = {k: v.clone() for k, v in models.UNet(3).state_dict().items()}
    sched = dict(schedule='poly', total_steps=10, warmup_steps=2, poly_power=0.9, min_lr=1e-5)

    def make(graph, resume=False):
        m = models.UNet(3)
        m.load_state_dict(init)
        tr = Trainer(m, None, loss_fn=compute_loss, workdir=str(tmp_path / 'w'), mixed_precision=mp, graph=graph, resume=resume,
                     **OPTIONS)
        m.train()
        return tr

    log = []
    real_call = _lib.call
    monkeypatch.setattr(_lib, 'call', lambda name, *a: (log.append(name) if name in OPT_CALLS else None, real_call(name, *a))[1])
    tr = make(False)
    assert torch.equal(tr.optimizer.ema, tr.arena.params)
    runs = tr.optimizer.runs
    assert len(runs) > 2 and {r[3] for r in runs} == {f32(0.1), 1.0} and {r[4] for r in runs} == {0.0, f32(1e-2)}
    nsteps = 5 if mp else 3          # (-mp: the initial loss scale of 65536 overflows twice; those steps are skipped)
    for i in range(nsteps):
        before = {k: v.double() for k, v in _snapshot(tr).items()}
        s0 = tr.mp_state.cpu().tolist() if mp else None
        del log[:]
        tr.train_batch(*_batch(i))
        assert log == (['pseg_mp_check'] if mp else []) + ['pseg_grad_sumsq', 'pseg_opt_step_adam'] + (['pseg_mp_update'] if mp else [])
        assert tr.optimizer.lr == lr_at(i, 1e-2, **sched)
        s1 = tr.mp_state.cpu().tolist() if mp else None
        skipped = mp and s1[5] > s0[5]
        R.grouped_step(before, tr.arena.grads.cpu().double(), runs, True, f32(tr.optimizer.lr), betas=(f32(0.9), f32(0.999)),
                       eps=f32(1e-8), decoupled=True, grad_scale=1.0, step=int(s0[4]) + 1 if mp else i + 1, max_norm=f32(0.5),
                       ema_decay=f32(0.9), mp={'inv_scale': s0[1], 'found': skipped} if mp else None)
        check_elements('trainer%s step %d' % ('-mp' if mp else '', i), 'adamw', _snapshot(tr), before, runs)
        if not skipped:
            st = tr.optimizer.clip_stats()
            assert abs(st['coef'] - before['coef']) < 2.0 ** -21 * before['coef'] and abs(st['norm'] - before['norm']) < 2.0 ** -21 * before['norm']
    assert not torch.equal(tr.optimizer.ema, tr.arena.params)
    # checkpoint after three steps; the averaged weights in it
    tr.save()
    ck = torch.load(tmp_path / 'w' / 'last.pt', map_location='cpu')
    assert set(ck['model_ema']) == set(ck['model']) and ck['optimizer']['sched_steps'] == nsteps
    if mp:
        assert tr.loss_scale_state()['steps_applied'] >= 3 and ck['optimizer']['steps'] == tr.loss_scale_state()['steps_applied']
    assert torch.equal(ck['optimizer']['ema'].cpu(), tr.optimizer.ema.cpu())
    live = tr.arena.params.clone()
    x = _batch(7)[0]
    tr.model.eval()
    with torch.no_grad():
        with tr.ema_weights():
            assert torch.equal(tr.arena.params, ck['optimizer']['ema'].cuda()) and torch.equal(tr.optimizer.ema, live)
            sd = tr.model.state_dict()
            assert all(torch.equal(sd[k].cpu(), ck['model_ema'][k]) for k in sd)
            logits_ema = tr.model(x).float().cpu()
        assert torch.equal(tr.arena.params, live)                        # restored bit for bit
        logits_live = tr.model(x).float().cpu()
    assert not torch.equal(logits_ema, logits_live)                      # (under -mp: the fp16 filter copies followed the swap)
    if not mp:
        fresh = models.UNet(3)
        fresh.load_state_dict(ck['model_ema'])
        fresh.cuda().eval()
        with torch.no_grad():
            assert torch.equal(fresh(x).cpu(), logits_ema)
    tr.model.train()
    # fourth step: the live trainer, a resumed one, and a graph=True run from the start
    tr.train_batch(*_batch(nsteps))
    four = _snapshot(tr)
    tr2 = make(False, resume=True)
    assert tr2.optimizer.sched_steps == nsteps and torch.equal(tr2.optimizer.ema.cpu(), ck['optimizer']['ema'].cpu())
    tr2.train_batch(*_batch(nsteps))
    assert tr2.optimizer.lr == lr_at(nsteps, 1e-2, **sched) == tr.optimizer.lr
    for k, t in _snapshot(tr2).items():
        assert torch.equal(t, four[k]), ('resume', k)
    trg = make(True)
    for i in range(nsteps + 1):
        trg.train_batch(*_batch(i))
    assert trg.step_mode() == 'replayed'
    for k, t in _snapshot(trg).items():
        assert torch.equal(t, four[k]), ('graph', k)
    # an older checkpoint (no averaged weights) starts the average from the weights it holds
    old = {k: v for k, v in ck.items() if k != 'model_ema'}
    old['optimizer'] = {k: v for k, v in ck['optimizer'].items() if k not in ('ema', 'clip_state', 'sched_steps')}
    torch.save(old, tmp_path / 'w' / 'last.pt')
    tr3 = make(False, resume=True)
    assert torch.equal(tr3.optimizer.ema, tr3.arena.params) and torch.equal(tr3.arena.params.cpu(), live.cpu())


@pytest.mark.parametrize('mp', [False, True])
@pytest.mark.parametrize('adam', [False, True])
def test_default_trainer_issues_the_old_calls(ops, monkeypatch, mp, adam):
    """without the new options the optimiser calls are the four old entry points, in the old order"""
    from pytorch_segmentation_amd import _lib, models
    from pytorch_segmentation_amd.utils import Trainer, compute_loss
    log = []
    real_call = _lib.call
    monkeypatch.setattr(_lib, 'call', lambda name, *a: (log.append(name) if name in OPT_CALLS else None, real_call(name, *a))[1])
    torch.manual_seed(0)
    m = models.UNet(3)
    tr = Trainer(m, None, loss_fn=compute_loss, adam=adam, lr=1e-2, mixed_precision=mp, graph=False)
    m.train()
    assert not tr.optimizer.grouped and tr.optimizer.ema is None and tr.schedule is None
    for i in range(2):
        tr.train_batch(*_batch(i))
    step = 'pseg_adam_step' if adam else 'pseg_sgd_step'
    assert log == (['pseg_mp_check', step + '_mp', 'pseg_mp_update'] if mp else [step]) * 2
    with pytest.raises(RuntimeError, match='ema_decay'):
        with tr.ema_weights():
            pass


# ------------------------------------------------------------------------------------------------ 6. command line
def test_command_line_with_every_flag(tmp_path, monkeypatch):
    """two epochs of train.py's train() with the new flags on synthetic data write last.pt with 'model_ema'; test.py --ema
    scores it; test.py --ema on a checkpoint without averaged weights says so"""
    from pytorch_segmentation_amd.utils.datasets import make_synthetic_coco
    import test as test_cli
    import train as train_mod
    root = make_synthetic_coco(str(tmp_path / 'data'), n_train=4, n_val=2, n_classes=1)
    monkeypatch.chdir(tmp_path)
    opt = train_mod.build_parser().parse_args([root, '--weight-decay', '1e-4', '--momentum', '0.8', '--adamw', '--no-decay-norm-bias',
                                               '--backbone-lr-mult', '0.1', '--clip-grad', '1.0', '--ema-decay', '0.9',
                                               '--schedule', 'cosine', '--warmup-steps', '1', '--min-lr', '1e-5'])
    monkeypatch.setattr(train_mod, 'OPTIM', train_mod.optim_from_options(opt))
    trainer, loss = train_mod.train(root, epochs=2, img_size=[64, 64], batch_size=2, accumulate=1, lr=1e-2, num_workers=0,
                                    notest=False, nosave=False, model_name='unet')
    assert trainer.epoch == 2 and loss == loss and trainer.optimizer.grouped and trainer.optimizer.decoupled
    assert trainer.schedule['total_steps'] == 4 and trainer.optimizer.sched_steps == 4
    assert trainer.optimizer.momentum == 0.8 and trainer.optimizer.max_grad_norm == 1.0
    last = str(tmp_path / 'weights' / 'last.pt')
    ck = torch.load(last, map_location='cpu')
    assert set(ck['model_ema']) == set(ck['model']) and any(not torch.equal(ck['model_ema'][k], ck['model'][k]) for k in ck['model'])
    val = os.path.join(root, 'val.json')
    common = [val, '--weights', last, '--model', 'unet', '-s', '64', '64', '-bs', '2', '--num-workers', '0']
    miou = test_cli.main(common + ['--ema'])
    assert isinstance(miou, float) and 0.0 <= miou <= 1.0
    plain = str(tmp_path / 'plain.pt')
    torch.save({'model': ck['model']}, plain)
    with pytest.raises(KeyError, match="holds no 'model_ema'"):
        test_cli.main([val, '--weights', plain, '--model', 'unet', '-s', '64', '64', '-bs', '2', '--num-workers', '0', '--ema'])
