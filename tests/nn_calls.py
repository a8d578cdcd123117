"""The library calls behind nn.Conv2d, nn.BatchNorm2d, nn.ConvNormAct and the ResNet bottleneck, recorded without a GPU (shared
by tests/test_nn_calls_cpu.py and tools/nn_call_log.py).  `_lib.call` is replaced by a recorder and `ops._stream` by a constant,
so the layers run on CPU tensors; the size and plan queries go to the real library, which loads without a device.  A log is the
ordered list of entry points with every argument: integers and floats as they are, a pointer as 0 when null and otherwise as the
ordinal of that address's first appearance in the case's log -- the same tensor feeding two calls, and a slice of it, show."""
import contextlib

import torch

from pytorch_segmentation_amd import _lib, arena, ops
from pytorch_segmentation_amd import nn as pnn
from pytorch_segmentation_amd.backbones import resnet
from pytorch_segmentation_amd.ops import ACT_RELU, Act

CPU = torch.device('cpu')
POLICIES = ('fp32', 'mixed', 'limb', 'half')
# every module-level switch the layers read, at its default: a case names the ones it turns
SWITCHES = {'ops.CAPTURING': 0, 'ops.OVERLAP_WGRAD': True, 'ops.DY_PLANES': True, 'ops.BN_MASK': True, 'ops.WGRAD_AFTER_DGRAD': False,
            'ops.FUSE_BN_BWD': True, 'ops.FUSE_BN_BWD_H': False, 'ops.BN_SMALL_IN_GRAPH': False, 'ops.EVER_CAPTURED': False,
            'nn.FUSE_STEM_POOL': True, 'nn.LIMB_MIN_CHANNELS': 0}
_MODS = {'ops': ops, 'nn': pnn}


class Recorder:
    def __init__(self):
        self.log, self.addr, self.keep = [], {}, []
        self.protos = _lib.parse_header()

    def ordinal(self, p):
        return 0 if not p else self.addr.setdefault(p, len(self.addr) + 1)

    def call(self, name, *args):
        types = self.protos[name][1]
        assert len(args) == len(types), '%s takes %d arguments, got %d' % (name, len(types), len(args))
        row = [name]
        for a, t in zip(args, types):
            if t is _lib.ctypes.c_void_p:
                row.append(self.ordinal(a))
            else:
                row.append(float(a) if t is _lib.ctypes.c_float else int(a))
        self.log.append(row)

    # what a case adds about the values the layers hand back
    def acts(self, *acts):
        self.log.append(['acts'] + [None if a is None else [a.B, a.H, a.W, a.C, a.ld, 'f16' if a.half else 'f32'] for a in acts])

    def none_slots(self, what, state):
        self.log.append([what, None if state is None else [int(v is None) for v in state]])

    def has(self, what, value):
        self.log.append(['has', what, int(value is not None)])


@contextlib.contextmanager
def recording(switches=None):
    """Everything the layers do inside goes to the returned Recorder; every tensor allocated inside stays alive until the end, so
    the allocator hands no address out twice."""
    rec = Recorder()

    def keeping(fn):
        def wrapped(*a, **k):
            t = fn(*a, **k)
            rec.keep.append(t)
            return t
        return wrapped

    @contextlib.contextmanager
    def side_stream(stream):
        rec.log.append(['enter'])
        try:
            yield
        finally:
            rec.log.append(['exit'])

    def fork_aux(device):
        rec.log.append(['fork'])
        return 'side'

    def record_stream(tensor, stream):
        rec.log.append(['record', rec.ordinal(tensor.data_ptr())])

    want = dict(SWITCHES)
    want.update(switches or {})
    patches = [(_lib, 'call', rec.call), (ops, '_stream', lambda: 0), (ops, 'workspace', ops._Workspace()),
               (ops, 'fork_aux', fork_aux), (torch.cuda, 'stream', side_stream), (torch.Tensor, 'record_stream', record_stream),
               (torch, 'empty', keeping(torch.empty)), (torch, 'zeros', keeping(torch.zeros)),
               (torch, 'empty_like', keeping(torch.empty_like))]
    patches += [(_MODS[k.split('.')[0]], k.split('.')[1], v) for k, v in want.items()]
    old = [(o, n, getattr(o, n)) for o, n, _ in patches]
    for o, n, v in patches:
        setattr(o, n, v)
    try:
        yield rec
    finally:
        for o, n, v in old:
            setattr(o, n, v)


def arm(model, half):
    """Zero CPU tensors where the arena would put kernel-native storage (and the fp16 filter copies of the half policy)."""
    for mod in model.modules():
        for name, p in mod._parameters.items():
            if p is None:
                continue
            shape = arena._layout(mod, name, p)[0]
            if '_raw' not in mod.__dict__:
                mod._raw, mod._raw_grad = {}, {}
            mod._raw[name], mod._raw_grad[name] = torch.zeros(shape), torch.zeros(shape)
        if half and isinstance(mod, pnn.Conv2d) and not mod.depthwise:
            n = mod.cout_h * mod.kernel_size[0] * mod.kernel_size[1] * mod.cin_h
            mod._w_h_view, mod._wT_h_view = torch.zeros(n, dtype=torch.float16), torch.zeros(n, dtype=torch.float16)
    return model


def make_env(rec, policy, pool=False, ready=False, **kw):
    env = pnn.Env(policy=policy, **kw)
    if pool:
        env.slab_pool = ops.SlabPool(CPU)
    if ready:
        env.grad_ready = lambda m: rec.log.append(['grad_ready', type(m).__name__])
    return env


def act_in(env, B, H, W, C):
    return Act.empty(B, H, W, C, CPU, dtype=env.act_dtype)


def cin_of(conv, env):
    return conv.cin_h if env.half else conv.cin_p


# ------------------------------------------------------------------------------------------------------------- runners
def run_conv(rec, policy, cin, cout, k, s=1, pad=None, d=1, groups=1, bias=False, H=8, out_f32=False, env=None, pool=False,
             ready=False, dx=None, reps=1, **bwd_kw):
    """Conv2d.fwd, then Conv2d.bwd `reps` times with one Env (a filter used twice in one pass), then the pool's reduction."""
    env = make_env(rec, policy, pool, ready, **(env or {}))
    conv = arm(pnn.Conv2d(cin, cout, k, s, (k - 1) // 2 * d if pad is None else pad, d, groups, bias=bias), env.half)
    x = act_in(env, 2, H, H, cin_of(conv, env))
    try:
        y, stats, saved = conv.fwd(x, env, want_stats=True, out_f32=out_f32)
    except NotImplementedError as e:
        rec.log.append(['raises', 'NotImplementedError', str(e)])
        return
    rec.acts(y)
    rec.has('stats', stats)
    rec.has('saved', saved)
    dy = act_in(env, y.B, y.H, y.W, y.C)
    for _ in range(reps):
        got = conv.bwd(dy, x, env, dx_out=act_in(env, x.B, x.H, x.W, x.C) if dx == 'given' else None, **bwd_kw)
        rec.acts(got)
    if env.slab_pool is not None:
        env.slab_pool.reduce(env.accumulate)


def run_cna(rec, policy, cin, cout, k=3, s=1, d=1, groups=1, H=8, env=None, pool=False, ready=False, dx=None, **bwd_kw):
    """ConvNormAct.fwd and .bwd."""
    env = make_env(rec, policy, pool, ready, **(env or {}))
    m = arm(pnn.ConvNormAct(cin, cout, k, s, groups, d), env.half).train()
    x = act_in(env, 2, H, H, cin_of(m.conv, env))
    z, (sc, sb) = m.fwd(x, env)
    rec.acts(z)
    rec.has('saved', sc)
    rec.none_slots('bn_saved', sb)
    if not env.save:
        return
    dz = z.like()
    got = m.bwd(dz, (sc, sb), env, dx_out=act_in(env, x.B, x.H, x.W, x.C) if dx == 'given' else None, **bwd_kw)
    rec.acts(got)
    if got is not None:
        rec.has('bnpart', got.bnpart)
    if env.slab_pool is not None:
        env.slab_pool.reduce(env.accumulate)


def run_chain(rec, policy, cin, mid, cout, k=3, H=8, dx_accumulate=False):
    """Two layers chained as the ResNet bottleneck chains them: the second conv's data gradient is the first layer's dz."""
    env = make_env(rec, policy)
    a, b = arm(pnn.ConvNormAct(cin, mid, 1), env.half).train(), arm(pnn.ConvNormAct(mid, cout, k), env.half).train()
    x = act_in(env, 2, H, H, cin_of(a.conv, env))
    za, (sca, sba) = a.fwd(x, env)
    zb, (scb, sbb) = b.fwd(za, env)
    rec.acts(za, zb)
    rec.none_slots('bn_saved', sba)
    dyb = b.bn.bwd(zb.like(), sbb, env, want_planes=b.conv.wants_dy_planes(scb, env))
    rec.has('planes', dyb.planes)
    dza = b.conv.bwd(dyb, scb, env, bn_prev=sba, dx_out=za.like() if dx_accumulate else None, dx_accumulate=dx_accumulate)
    rec.acts(dza)
    rec.has('bnpart', dza.bnpart)
    dya = a.bn.bwd(dza, sba, env)
    rec.acts(a.conv.bwd(dya, sca, env))


def run_bn(rec, policy, C=16, H=8, train=True, stats='given', residual=False, save=True, pooled=False, bwd=None, **ctor):
    """BatchNorm2d.fwd (or .fwd_pooled) and, with `bwd` (its keyword switches), .bwd."""
    env = make_env(rec, policy, save=save)
    bn = arm(pnn.BatchNorm2d(C, **ctor), env.half).train(train)
    y = act_in(env, 2, H, H, C)
    st = ops.col_stats(y) if stats == 'given' else None
    if pooled:
        got = bn.fwd_pooled(y, st, env, ACT_RELU, 3, 2, 1)
        rec.has('pooled', got)
        if got is None:
            return
        z, arg, saved = got
        rec.has('argmax', arg)
    else:
        z, saved = bn.fwd(y, st, env, act=ACT_RELU, residual=y.like() if residual else None)
        rec.has('amax', z.amax)
    rec.acts(z)
    rec.none_slots('bn_saved', saved)
    if bwd is None or saved is None:
        return
    kw = dict(bwd)
    if kw.pop('dres', False):
        kw['dres'] = z.like()
    dy = bn.bwd(z.like(), saved, env, **kw)
    rec.acts(dy)
    rec.has('planes', dy.planes)


def run_bottleneck(rec, policy, inplanes, planes, stride=1, H=8):
    env = make_env(rec, policy)
    down = None
    if stride != 1 or inplanes != planes * 4:
        down = torch.nn.Sequential(pnn.Conv2d(inplanes, planes * 4, 1, stride=stride, bias=False), pnn.BatchNorm2d(planes * 4))
    blk = arm(resnet.Bottleneck(inplanes, planes, stride, down), env.half).train()
    x = act_in(env, 2, H, H, inplanes)
    out, saved = blk.fwd(x, env)
    rec.acts(out)
    for b in saved[1::2]:
        rec.none_slots('bn_saved', b)
    rec.acts(blk.bwd(out.like(), saved, env))


# --------------------------------------------------------------------------------------------------------------- cases
def cases():
    """-> [(name, runner, args, kwargs, switches, entry points that must appear, entry points that must not)]"""
    out = []

    def add(name, fn, *args, switches=None, present=(), absent=(), **kw):
        out.append((name, fn, args, kw, switches or {}, tuple(present), tuple(absent)))

    dense = {'3x3s1': dict(k=3), '3x3s2': dict(k=3, s=2), '1x1': dict(k=1), '3x3d2': dict(k=3, d=2)}
    for pol in POLICIES:
        h = '_h' if pol == 'half' else ''
        plain = ['pseg_conv2d_fwd' + h, 'pseg_conv2d_wgrad' + h]
        for name, geo in dense.items():
            add('dense/%s/%s' % (name, pol), run_cna, pol, 16, 32, present=plain + ['pseg_conv2d_dgrad' + h], **geo)
        add('dense/3x3s1/%s/no_dx' % pol, run_cna, pol, 16, 32, need_dx=False, present=plain, absent=['pseg_conv2d_dgrad' + h])
        add('dense/3x3s1/%s/dx_accumulate' % pol, run_cna, pol, 16, 32, dx='given', dx_accumulate=True)
        add('dense/3x3s1/%s/no_save' % pol, run_cna, pol, 16, 32, env=dict(save=False))
        # channel counts the fp16 kernels pad further than the arena does: the stem (3 -> 4 / 8), the two-class classifier (2 -> 4 / 8)
        padded = ['pseg_copy2d'] if pol == 'half' else []
        for acc in (False, True):
            tag = '%s/accumulate%d' % (pol, acc)
            add('padded/stem/' + tag, run_conv, pol, 3, 16, 7, s=2, H=16, env=dict(accumulate=acc), need_dx=False, present=plain + padded)
            add('padded/cls21/' + tag, run_conv, pol, 32, 21, 1, bias=True, out_f32=True, env=dict(accumulate=acc),
                present=plain + ['pseg_col_sum' + h])
            add('padded/cls2/' + tag, run_conv, pol, 32, 2, 1, bias=True, out_f32=True, env=dict(accumulate=acc),
                present=plain + padded + ['pseg_col_sum' + h])
        # where the weight gradient goes
        wide = dict(k=3, H=16)
        add('wgrad/pool/' + pol, run_conv, pol, 64, 64, pool=True, present=['pseg_conv2d_wgrad_slabs' + h, 'pseg_slab_reduce_batch'], **wide)
        add('wgrad/pool_accumulate/' + pol, run_conv, pol, 64, 64, pool=True, env=dict(accumulate=True),
            present=['pseg_conv2d_wgrad_slabs' + h], **wide)
        add('wgrad/pool_twice/' + pol, run_conv, pol, 64, 64, pool=True, reps=2,
            present=['pseg_conv2d_wgrad_slabs' + h, 'pseg_slab_reduce_batch', 'pseg_conv2d_wgrad' + h], **wide)
        add('wgrad/pool_small/' + pol, run_conv, pol, 16, 32, 3, pool=True, present=['pseg_conv2d_wgrad' + h])
        add('wgrad/pool_forked/' + pol, run_conv, pol, 64, 64, pool=True, env=dict(overlap_wgrad=True), present=['fork'], **wide)
        add('wgrad/grad_ready/' + pol, run_cna, pol, 64, 64, pool=True, ready=True, present=['grad_ready', 'pseg_conv2d_wgrad' + h],
            absent=['pseg_conv2d_wgrad_slabs' + h], **wide)
        for tag, kw in (('plain', {}), ('on_main', dict(wgrad_on_main=True)), ('concurrent_true', dict(wgrad_concurrent=True)),
                        ('concurrent_false', dict(wgrad_concurrent=False)), ('concurrent_none', dict(wgrad_concurrent=None)),
                        ('on_main_concurrent', dict(wgrad_on_main=True, wgrad_concurrent=True))):
            forks = 'on_main' not in tag
            add('wgrad/overlap/%s/%s' % (tag, pol), run_conv, pol, 64, 64, env=dict(overlap_wgrad=True),
                present=['fork', 'enter', 'exit', 'record'] if forks else [], absent=[] if forks else ['fork'], **dict(wide, **kw))
        add('wgrad/overlap/bias/' + pol, run_conv, pol, 32, 21, 1, bias=True, env=dict(overlap_wgrad=True), present=['fork'])
        add('wgrad/overlap/off/' + pol, run_conv, pol, 16, 32, 3, env=dict(overlap_wgrad=True), switches={'ops.OVERLAP_WGRAD': False},
            absent=['fork'])
        add('wgrad/after_dgrad/' + pol, run_conv, pol, 16, 32, 3, switches={'ops.WGRAD_AFTER_DGRAD': True})
        add('wgrad/after_dgrad/no_dx/' + pol, run_conv, pol, 16, 32, 3, need_dx=False, switches={'ops.WGRAD_AFTER_DGRAD': True})
        add('wgrad/after_dgrad/forked/' + pol, run_conv, pol, 16, 32, 3, env=dict(overlap_wgrad=True),
            switches={'ops.WGRAD_AFTER_DGRAD': True}, present=['fork'])
        # the data gradient that carries the BatchNorm backward sums of the layer below
        fused = ['pseg_conv2d_dgrad_bnstat'] if pol == 'fp32' else []
        add('bnstat/chain/' + pol, run_chain, pol, 32, 64, 64, H=16, present=fused, absent=['pseg_conv2d_dgrad_bnstat_h'])
        add('bnstat/chain_dx_accumulate/' + pol, run_chain, pol, 32, 64, 64, H=16, dx_accumulate=True,
            absent=['pseg_conv2d_dgrad_bnstat', 'pseg_conv2d_dgrad_bnstat_h'])
        add('bnstat/chain_capturing/' + pol, run_chain, pol, 32, 64, 64, H=16, switches={'ops.CAPTURING': 1}, present=fused)
        add('bottleneck/identity/' + pol, run_bottleneck, pol, 64, 16)
        add('bottleneck/projection/' + pol, run_bottleneck, pol, 32, 16, stride=2, H=16)
    add('bnstat/chain_fused_h/half', run_chain, 'half', 32, 64, 64, H=16, switches={'ops.FUSE_BN_BWD_H': True},
        present=['pseg_conv2d_dgrad_bnstat_h'])
    add('bnstat/chain_fused_h_dx_accumulate/half', run_chain, 'half', 32, 64, 64, H=16, dx_accumulate=True,
        switches={'ops.FUSE_BN_BWD_H': True}, absent=['pseg_conv2d_dgrad_bnstat_h'])
    add('bnstat/chain_off/fp32', run_chain, 'fp32', 32, 64, 64, H=16, switches={'ops.FUSE_BN_BWD': False},
        absent=['pseg_conv2d_dgrad_bnstat'])
    # limb planes: BatchNorm backward writes dy pre-split, the data gradient reads the planes
    planes = ['pseg_split_planes', 'pseg_conv2d_dgrad_planes']
    # (the smallest problem the pre-split kernel takes at batch 2: 192 input channels on a 128 x 128 map; nothing is computed)
    add('planes/cna/limb', run_cna, 'limb', 192, 128, H=128, present=planes)
    add('planes/cna_capturing/limb', run_cna, 'limb', 192, 128, H=128, switches={'ops.CAPTURING': 1}, present=planes)
    add('planes/cna_dx_accumulate/limb', run_cna, 'limb', 192, 128, H=128, dx='given', dx_accumulate=True, present=planes)
    add('planes/chain/limb', run_chain, 'limb', 32, 192, 128, H=128, present=planes)
    add('planes/off/limb', run_cna, 'limb', 192, 128, H=128, switches={'ops.DY_PLANES': False}, absent=planes)
    add('planes/small_map/limb', run_cna, 'limb', 64, 128, H=16, switches={'ops.CAPTURING': 1}, absent=planes)
    # depthwise
    for pol in ('fp32', 'half'):
        h = '_h' if pol == 'half' else ''
        for s in (1, 2):
            for tag, kw in (('plain', {}), ('dx_given', dict(dx='given')), ('dx_accumulate_given', dict(dx='given', dx_accumulate=True)),
                            ('dx_accumulate', dict(dx_accumulate=True)), ('no_dx', dict(need_dx=False))):
                add('depthwise/s%d/%s/%s' % (s, tag, pol), run_cna, pol, 16, 16, 3, s, groups=16, H=8 * s,
                    present=['pseg_dwconv_fwd' + h, 'pseg_dwconv_wgrad' + h] + (['pseg_copy2d' + h] if 'accumulate' in tag else []), **kw)
        add('depthwise/forked/' + pol, run_cna, pol, 16, 16, 3, 1, groups=16, env=dict(overlap_wgrad=True), present=['fork'])
        add('depthwise/after_dgrad/' + pol, run_cna, pol, 16, 16, 3, 1, groups=16, switches={'ops.WGRAD_AFTER_DGRAD': True})
        add('depthwise/c12/' + pol, run_conv, pol, 12, 12, 3, groups=12, present=['raises'] if pol == 'half' else ['pseg_dwconv_fwd'])
    # BatchNorm2d
    back = dict(bwd={})
    for pol in ('fp32', 'half'):
        h = '_h' if pol == 'half' else ''
        for cap in (0, 1):
            sw = {'ops.CAPTURING': cap}
            tag = '%s/capturing%d' % (pol, cap)
            path = ['pseg_bn_fwd_fused' + h] if cap == 0 else ['pseg_bn_finalize', 'pseg_bn_act_fwd' + h]
            add('bn/train/stats_given/' + tag, run_bn, pol, switches=sw, present=path, **back)
            add('bn/train/stats_none/' + tag, run_bn, pol, stats=None, switches=sw, present=path + ['pseg_col_stats' + h], **back)
            add('bn/eval/' + tag, run_bn, pol, train=False, switches=sw, present=['pseg_bn_eval_coeffs', 'pseg_bn_act_fwd' + h], **back)
            add('bn/momentum_none/' + tag, run_bn, pol, momentum=None, switches=sw, **back)
            add('bn/no_running_stats/' + tag, run_bn, pol, track_running_stats=False, switches=sw, **back)
            add('bn/no_running_stats_eval/' + tag, run_bn, pol, train=False, track_running_stats=False, switches=sw, **back)
            add('bn/no_affine/' + tag, run_bn, pol, affine=False, switches=sw, **back)
            add('bn/no_save/' + tag, run_bn, pol, save=False, switches=sw)
            for mask in (True, False):
                add('bn/residual_c32/mask%d/%s' % (mask, tag), run_bn, pol, C=32, residual=True,
                    switches=dict(sw, **{'ops.BN_MASK': mask}), bwd=dict(dres=True))
            add('bn/residual_c32/no_save/' + tag, run_bn, pol, C=32, residual=True, save=False, switches=sw)
            add('bn/residual_c16/' + tag, run_bn, pol, residual=True, switches=sw, bwd=dict(dres=True, res_accumulate=True))
            add('bn/bwd_switches/' + tag, run_bn, pol, switches=sw, bwd=dict(dres=True, res_accumulate=True, want_planes=True))
            add('bn/pooled/' + tag, run_bn, pol, pooled=True, switches=sw,
                present=['pseg_bn_finalize', 'pseg_bn_act_maxpool_fwd' + h], **back)
        add('bn/pooled/stats_none/' + pol, run_bn, pol, pooled=True, stats=None, present=['pseg_col_stats' + h], **back)
        add('bn/pooled/momentum_none/' + pol, run_bn, pol, pooled=True, momentum=None, **back)
        add('bn/pooled/no_running_stats/' + pol, run_bn, pol, pooled=True, track_running_stats=False, **back)
        add('bn/pooled/no_save/' + pol, run_bn, pol, pooled=True, save=False)
        add('bn/pooled/eval/' + pol, run_bn, pol, pooled=True, train=False, absent=['pseg_bn_finalize'])
        add('bn/pooled/off/' + pol, run_bn, pol, pooled=True, switches={'nn.FUSE_STEM_POOL': False}, absent=['pseg_bn_finalize'])
    for cap in (0, 1):
        sw = {'ops.CAPTURING': cap}
        add('bn/track_amax/limb/capturing%d' % cap, run_bn, 'limb', switches=sw, **back)
        add('bn/track_amax_eval/limb/capturing%d' % cap, run_bn, 'limb', train=False, switches=sw, **back)
        add('bn/want_planes/limb/capturing%d' % cap, run_bn, 'limb', C=64, switches=sw, bwd=dict(want_planes=True))
    add('bn/pooled/limb', run_bn, 'limb', pooled=True, absent=['pseg_bn_finalize'])
    return out


def run_case(case):
    """-> the log of one case"""
    name, fn, args, kw, switches, present, absent = case
    with recording(switches) as rec:
        fn(rec, *args, **kw)
        return rec.log


def check_presence(case, log):
    """A case that stops exercising its branch must fail, not pass on another path's log."""
    name, _, _, _, _, present, absent = case
    seen = {row[0] for row in log}
    assert not set(present) - seen, '%s: no %s in its log' % (name, sorted(set(present) - seen))
    assert not set(absent) & seen, '%s: %s in its log' % (name, sorted(set(absent) & seen))
