"""The case table of the cross-entropy / mask / metric instance tests (csrc/loss.hip), importable without a GPU.  Shared by
tests/test_loss_instances_cpu.py (the table reaches every compiled instance and host branch; the refusals; the mirror against the
library's own query; a plain fp32 evaluation stays inside the bounds) and tests/test_loss_instances_gpu.py (every row launched,
its record read back, every output against fp64).

Four parts:
  * a mirror of the host rules that choose a launch: capped_blocks, the dispatch ladder of pseg_ce_fwd_bwd, pseg_ce_upsampled_ok,
    up_src_index and max_owned in numpy float32, the scatter / gather decision -- written from the source, not read back;
  * the compiled instances (CE_COMPILED, ARGMAX_COMPILED), written out from the dispatch code;
  * the rows.  A row is (id, entry, shape, flags, record):
      entry   'ce' (pseg_ce_fwd_bwd), 'ce_up' (pseg_ce_upsampled_fwd_bwd), 'argmax', 'confusion', 'scale' (pseg_scale_inplace)
      shape   ce: (B, C, H, W); ce_up: (B, C, h, w, H, W, align_corners, ld, ldd); argmax: (B, C, HW); confusion: (n, C); scale: (n,)
      flags   dict of what the row sets (mis, ignore_index, nograd, all_ignored, env, ...)
      record  what pseg_debug_last_loss must answer after the row's launch WITH a gradient (pseg_amd.h); rows with flags['nograd']
              are launched a second time without one, and then the last field is 0
  * the inputs, the fp64 reference and the bounds of the 'ce' and 'ce_up' rows (torch on the CPU), computed once per row and shared.

The bounds are derived in the docstring of tests/test_loss_instances_gpu.py."""
import collections
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import fill

Row = collections.namedtuple('Row', 'id entry shape flags record')
Refusal = collections.namedtuple('Refusal', 'id name args rc match')

ERR_ARG = -1
FIELDS = ('kernel', 'CMAX', 'VEC', 'grid x', 'block x', 'form', 'finish blocks', 'gradient')
# kernel codes of pseg_debug_last_loss (enum LossKernel)
CE_FUSED, CE_GENERIC, CE_UP_FUSED, CE_UP_SCATTER, ARGMAX, CONFUSION, SCALE_INPLACE = range(1, 8)
KERNEL_NAMES = {CE_FUSED: 'ce_fused_kernel', CE_GENERIC: 'ce_generic_kernel', CE_UP_FUSED: 'ce_up_fused_kernel',
                CE_UP_SCATTER: 'ce_up_scatter_kernel', ARGMAX: 'argmax_kernel', CONFUSION: 'confusion_kernel',
                SCALE_INPLACE: 'scale_inplace_kernel'}
# the __global__ functions that run beside the one a record names
HELPER_KERNELS = ('ce_count_kernel', 'ce_finish_kernel', 'ce_up_finish_kernel', 'ce_up_combine_kernel')
NONE, GATHER, SCATTER = 0, 1, 2                                       # form of the up-sampled loss
FORM_NAMES = {NONE: '-', GATHER: 'gather', SCATTER: 'scatter'}


def describe(rec):
    return '%s: ' % KERNEL_NAMES.get(rec[0], '?') + ', '.join('%s %s' % (n, FORM_NAMES[v] if n == 'form' else v)
                                                              for n, v in zip(FIELDS[1:], rec[1:]))


# ------------------------------------------------------------------------------------------------ the mirror of the host rules
kCeMaxBlocks = 4096
kCountMaxBlocks, kScaleMaxBlocks, kArgmaxMaxBlocks, kConfusionMaxBlocks, kCombineMaxBlocks = 2048, 2048, 4096, 1024, 4096
kMaxConfusionClasses = 1024
kUpTY, kUpTX, kUpCP, kUpThreads, kUpRY, kUpRX = 2, 8, 24, 512, 16, 42
kSY, kSX, kSThreads = 2, 8, 256
kSPY, kSPX = kSY + 1, kSX + 1
kSRY, kSRX = 4 * kSY + 2, 4 * kSX + 2
kFinishUnroll, kUpFinishUnroll = 8 * 256, 4 * 256                    # the unrolled loops run while i + 7 * 256 (3 * 256) < nblocks
CE_HEADER_BYTES = 16
f32 = np.float32


def cdiv(a, b):
    return -(-a // b)


def capped_blocks(items, cap):
    return max(1, min(cdiv(items, 256), cap))


def ce_dispatch(C, HW, logits_aligned=True, dlogits_aligned=True):
    """the ladder of pseg_ce_fwd_bwd -> (kernel, CMAX, VEC); dlogits_aligned is True for a NULL dlogits"""
    vec4 = HW % 4 == 0 and logits_aligned and dlogits_aligned
    for cmax, vec in ((4, 4), (8, 4), (24, 4), (32, 2)):
        if C <= cmax:
            return (CE_FUSED, cmax, vec if vec4 else 1)
    return (CE_GENERIC, 0, 1)


def ce_workspace_bytes():
    return CE_HEADER_BYTES + kCeMaxBlocks * 8


def ce_upsampled_ok(h, w, C, H, W, ac):
    if h <= 0 or w <= 0 or H < h or W < w or C <= 0 or C > kUpCP:
        return 0
    sy = ((h - 1) / (H - 1) if H > 1 else 0.0) if ac else h / H
    sx = ((w - 1) / (W - 1) if W > 1 else 0.0) if ac else w / W
    if sy <= 0.0 or sx <= 0.0:
        return 0
    ry, rx = min((kUpTY + 1) / sy + 2.5, H), min((kUpTX + 1) / sx + 2.5, W)
    return int(ry <= kUpRY and rx <= kUpRX)


def ce_upsampled_workspace_bytes(B, h, w):
    blocks = B * cdiv(h, kUpTY) * cdiv(w, kUpTX)
    partial = cdiv(CE_HEADER_BYTES + blocks * 3 * 8, 256) * 256
    return partial + B * cdiv(h, kSY) * cdiv(w, kSX) * (kSPY * kSPX * kUpCP) * 4


def up_scale(n_in, n_out, ac):
    if ac:
        return f32(n_in - 1) / f32(n_out - 1) if n_out > 1 else f32(0)
    return f32(n_in) / f32(n_out)


def up_src_index(n_in, n_out, ac, o=None):
    """up_src_index of loss.hip over the destination indices o (all of them by default), in float32 -> (i0, i1, l0, l1)"""
    o = np.arange(n_out) if o is None else np.asarray(o)
    sc, of = up_scale(n_in, n_out, ac), o.astype(f32)
    if ac:
        s = sc * of
    else:
        s = np.maximum(sc * (of + f32(0.5)) - f32(0.5), f32(0))
    assert s.dtype == f32
    i0 = np.minimum(s.astype(np.int32), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = s - i0.astype(f32)
    return i0, i1, f32(1) - l1, l1


def max_owned(n_in, n_out, ac, tile):
    """the largest number of destination indices whose first tap falls into one tile of source indices, + 2 for align_corners = 0"""
    i0 = up_src_index(n_in, n_out, ac)[0]
    return int(np.bincount(i0 // tile).max()) + (0 if ac else 2)


def scatter_eligible(h, w, H, W, ac):
    return max_owned(h, H, ac, kSY) <= kSRY and max_owned(w, W, ac, kSX) <= kSRX


def up_form(h, w, H, W, ac, env=None):
    """env: the value of PSEG_CE_SCATTER (None: unset)"""
    on = env is None or int(env) != 0
    return SCATTER if on and scatter_eligible(h, w, H, W, ac) else GATHER


# ------------------------------------------------------------------------------------------------ records
def rec_ce(B, C, HW, logits_aligned=True, dlogits_aligned=True, grad=True):
    k, cmax, vec = ce_dispatch(C, HW, logits_aligned, dlogits_aligned or not grad)
    blocks = capped_blocks(B * HW // vec, kCeMaxBlocks)
    return (k, cmax, vec, blocks, 256, NONE, blocks, int(grad))


def rec_ce_up(B, h, w, H, W, ac, env=None, grad=True):
    blocks = B * cdiv(h, kUpTY) * cdiv(w, kUpTX)                       # (kSY x kSX is the same tile)
    if up_form(h, w, H, W, ac, env) == SCATTER:
        return (CE_UP_SCATTER, kUpCP, 1, blocks, kSThreads, SCATTER, blocks, int(grad))
    return (CE_UP_FUSED, kUpCP, 1, blocks, kUpThreads, GATHER, blocks, int(grad))


def rec_argmax(B, HW, aligned=True):
    vec = 4 if HW % 4 == 0 and aligned else 1
    return (ARGMAX, 0, vec, capped_blocks(B * HW // vec, kArgmaxMaxBlocks), 256, NONE, 0, 0)


def rec_confusion(n):
    return (CONFUSION, 0, 1, capped_blocks(n, kConfusionMaxBlocks), 256, NONE, 0, 0)


def rec_scale(n):
    return (SCALE_INPLACE, 0, 4, capped_blocks(max(n // 4, 1), kScaleMaxBlocks), 256, NONE, 0, 0)


def without_gradient(rec):
    return rec[:7] + (0,)


# ------------------------------------------------------------------------------------------------ what is compiled
GENERIC = 'generic'
CE_COMPILED = {(4, 4), (4, 1), (8, 4), (8, 1), (24, 4), (24, 1), (32, 2), (32, 1), GENERIC}   # CE_LAUNCH(CMAX, VEC) + ce_generic_kernel
ARGMAX_COMPILED = {4, 1}                                                                       # argmax_kernel<VEC>


def instance(rec):
    if rec[0] == CE_FUSED:
        return (rec[1], rec[2])
    if rec[0] == CE_GENERIC:
        return GENERIC
    if rec[0] == ARGMAX:
        return rec[2]
    return ()


# ------------------------------------------------------------------------------------------------ the rows
ROWS = []


def _add(id, entry, shape, record, **flags):
    ROWS.append(Row(id, entry, tuple(shape), flags, record))


# ---- plain cross-entropy: pseg_ce_fwd_bwd.  One row per compiled instance, at the smallest shapes that take it
CE_INSTANCE_SHAPES = [((2, 3, 5, 7), (4, 1)), ((2, 2, 4, 6), (4, 4)), ((1, 5, 7, 9), (8, 1)), ((2, 8, 4, 4), (8, 4)),
                      ((2, 21, 3, 3), (24, 1)), ((2, 24, 4, 8), (24, 4)), ((1, 32, 3, 5), (32, 1)), ((2, 25, 4, 4), (32, 2)),
                      ((1, 33, 3, 5), GENERIC)]
for (_B, _C, _H, _W), _inst in CE_INSTANCE_SHAPES:
    _add('ce-%dx%dx%dx%d' % (_B, _C, _H, _W), 'ce', (_B, _C, _H, _W), rec_ce(_B, _C, _H * _W),
         nograd=_inst in ((24, 4), GENERIC))                        # loss-only on one vector row and on the generic row
_add('ce-only-class', 'ce', (1, 1, 3, 5), rec_ce(1, 1, 15), only_class=True)
# HW % 4 == 0 but an operand four bytes off a 16-byte boundary inside a larger buffer: VEC = 1
_add('ce-misaligned-logits', 'ce', (2, 2, 4, 6), rec_ce(2, 2, 24, logits_aligned=False), mis='logits')
_add('ce-misaligned-dlogits', 'ce', (2, 8, 4, 4), rec_ce(2, 8, 16, dlogits_aligned=False), mis='dlogits', nograd=True)
_add('ce-misaligned-logits-C21', 'ce', (2, 21, 2, 4), rec_ce(2, 21, 8, logits_aligned=False), mis='logits')
_add('ce-misaligned-dlogits-C25', 'ce', (2, 25, 2, 4), rec_ce(2, 25, 8, dlogits_aligned=False), mis='dlogits')
# three images of 12 pixels under VEC = 4: three groups per image, the groups of a wave cross image boundaries
_add('ce-B3-HW12', 'ce', (3, 3, 3, 4), rec_ce(3, 3, 12))
# grid stride: more pixels than 4096 blocks hold, an odd count (VEC = 1), 4096 partials for the finish kernel
BIG_CE_HW = 4096 * 256 + 259
_add('ce-grid-stride', 'ce', (1, 2, 1, BIG_CE_HW), rec_ce(1, 2, BIG_CE_HW), big=True)
_add('ce-all-ignored', 'ce', (2, 5, 4, 4), rec_ce(2, 5, 16), all_ignored=True)
_add('ce-all-ignored-generic', 'ce', (1, 33, 3, 5), rec_ce(1, 33, 15), all_ignored=True)
_add('ce-ignore255', 'ce', (2, 21, 4, 6), rec_ce(2, 21, 24), ignore_index=255)

# ---- cross-entropy on up-sampled logits: pseg_ce_upsampled_fwd_bwd.  Every shape with PSEG_CE_SCATTER unset and with
#  PSEG_CE_SCATTER=0; the form in the record is the mirror's (tests/test_loss_instances_cpu.py holds it to the forms stated there)
UP_SHAPES = [(8, 8, 32, 32, 1), (8, 8, 32, 32, 0), (9, 13, 33, 49, 1), (9, 13, 33, 49, 0), (5, 9, 15, 27, 0), (5, 9, 13, 20, 0),
             (6, 10, 9, 15, 1), (7, 11, 7, 11, 0), (7, 11, 7, 11, 1), (16, 16, 65, 65, 1), (1, 1, 4, 4, 0), (8, 1, 32, 1, 0),
             (2, 2, 2, 2, 1)]
UP_CLASSES = (21, 5, 24, 1)


def _up_id(B, C, h, w, H, W, ac, ld, ldd, env):
    return 'ce_up-%dx%dx%dx%d-%dx%d-ac%d-ld%d-ldd%d-%s' % (B, C, h, w, H, W, ac, ld, ldd, 'env0' if env == '0' else 'default')


def _add_up(B, C, h, w, H, W, ac, ld, ldd, env, **flags):
    _add(_up_id(B, C, h, w, H, W, ac, ld, ldd, env) + ''.join('-' + k for k in sorted(flags)), 'ce_up', (B, C, h, w, H, W, ac, ld, ldd),
         rec_ce_up(B, h, w, H, W, ac, env), env=env, **flags)


for _i, (_h, _w, _H, _W, _ac) in enumerate(UP_SHAPES):
    for _j, _env in enumerate((None, '0')):
        # C and the two leading dimensions cycle independently: every (ld, ldd) pair with both forms, every C with both forms
        _add_up(2, UP_CLASSES[(_i + _j) % 4], _h, _w, _H, _W, _ac, (24, 32)[_i % 2], (24, 32)[(_i // 2 + _j) % 2], _env)
for _env in (None, '0'):
    _add_up(2, 21, 9, 13, 33, 49, 1, 32, 32, _env, nograd=True)      # loss only: dlogits_lr NULL
    _add_up(2, 5, 9, 13, 33, 49, 1, 24, 32, _env, all_ignored=True)
# the unrolled loops of the finish kernels: 1024 blocks > 768 behind the scatter kernel, 2048 > 1792 behind the gather kernel
_add_up(4, 3, 64, 64, 256, 256, 1, 24, 24, None, big=True)
_add_up(8, 3, 64, 64, 256, 256, 1, 24, 32, '0', big=True)
# the grid-stride loop of ce_up_combine_kernel: more (pixel, lane) items than 4096 blocks hold, at ratio 1
_add_up(1, 3, 420, 420, 420, 420, 1, 24, 32, None, big=True)

# ---- argmax: pseg_argmax.  (B, C, HW)
BIG_ARGMAX_HW = 4096 * 256 * 4 + 8
_add('argmax-vec4', 'argmax', (2, 21, 24), rec_argmax(2, 24))
_add('argmax-odd-HW', 'argmax', (2, 21, 35), rec_argmax(2, 35))
_add('argmax-misaligned', 'argmax', (2, 5, 24), rec_argmax(2, 24, aligned=False), mis=True)
_add('argmax-only-class', 'argmax', (2, 1, 12), rec_argmax(2, 12))
_add('argmax-B3-HW12', 'argmax', (3, 3, 12), rec_argmax(3, 12))
_add('argmax-grid-stride', 'argmax', (1, 2, BIG_ARGMAX_HW), rec_argmax(1, BIG_ARGMAX_HW), big=True)

# ---- confusion: pseg_confusion.  (n, C)
BIG_CONFUSION_N = 1024 * 256 + 3
for _n, _C in ((1, 1), (257, 1), (1, 21), (255, 21), (257, 21), (BIG_CONFUSION_N, 21), (255, 1024), (BIG_CONFUSION_N, 1024)):
    _add('confusion-n%d-C%d' % (_n, _C), 'confusion', (_n, _C), rec_confusion(_n))

# ---- scale_inplace: pseg_scale_inplace.  (n,)
BIG_SCALE_N = 2048 * 256 * 4 + 5
for _n in (1, 3, 4, 7, 1027, BIG_SCALE_N):
    _add('scale-n%d' % _n, 'scale', (_n,), rec_scale(_n))

BY_ID = {r.id: r for r in ROWS}

# ------------------------------------------------------------------------------------------------ refusals
# argument checks run before any launch: these need no device.  'A' stands for a 16-byte aligned made-up device address.
A = 'A'
UP_NOT_OK = [(8, 8, 25, 32, 32, 1), (8, 8, 21, 7, 32, 1), (8, 8, 21, 33, 33, 1), (16, 16, 21, 68, 68, 1), (1, 8, 21, 4, 32, 1)]   # (h, w, C, H, W, ac)


def _up_call(B, h, w, C, H, W, ac, ld=32, ldd=32, ws_bytes=1 << 24):
    return (A, ld, B, h, w, C, A, H, W, ac, -100, A, ldd, A, A, ws_bytes, None)


REFUSALS = [Refusal('ce_up-not-covered-%dx%dx%d-%dx%d' % (h, w, C, H, W), 'pseg_ce_upsampled_fwd_bwd', _up_call(1, h, w, C, H, W, ac),
                    ERR_ARG, 'not covered') for h, w, C, H, W, ac in UP_NOT_OK] + [
    Refusal('confusion-C1025', 'pseg_confusion', (A, A, 64, 1025, A, None), ERR_ARG, 'class count'),
    Refusal('ce-short-workspace', 'pseg_ce_fwd_bwd', (A, A, 2, 5, 16, -100, A, A, A, ce_workspace_bytes() - 1, None), ERR_ARG,
            'workspace too small'),
    Refusal('ce_up-short-workspace', 'pseg_ce_upsampled_fwd_bwd',
            _up_call(2, 8, 8, 21, 32, 32, 1, ws_bytes=ce_upsampled_workspace_bytes(2, 8, 8) - 1), ERR_ARG, 'workspace too small'),
    Refusal('ce_up-ldd22', 'pseg_ce_upsampled_fwd_bwd', _up_call(2, 8, 8, 21, 32, 32, 1, ldd=22), ERR_ARG, 'ldd % 4'),
    Refusal('ce_up-ldd-below-C', 'pseg_ce_upsampled_fwd_bwd', _up_call(2, 8, 8, 21, 32, 32, 1, ldd=20), ERR_ARG, 'ldd >= C'),
]

# ------------------------------------------------------------------------------------------------ inputs, fp64 reference, bounds
U = 2.0 ** -24
CE_SCALE, UP_SCALE = 5.0, 3.0            # the logits are uniform in [-5, 5) and [-3, 3)

Ref = collections.namedtuple('Ref', 'loss n_valid n_bad grad A K K_loss term')


def ce_inputs(row):
    """-> (logits [B][C][H][W] fp32, target [B][H][W] int64, ignore_index); computed once per row, never written to"""
    return _ce_inputs(row.id)


@functools.lru_cache(maxsize=None)
def _ce_inputs(id):
    row = BY_ID[id]
    B, C, H, W = row.shape
    ign = row.flags.get('ignore_index', -100)
    key = 'lossinst/ce/%d_%d_%d_%d' % row.shape
    x = fill.uniform(key, (B, C, H, W), CE_SCALE)
    t = fill.labels(key + '/t', (B, H, W), C, block=2)
    if row.flags.get('all_ignored'):
        t[:] = ign
        return x, t, ign
    t[0, 0, :3] = ign                                 # ignored
    t[-1, -1, -1] = C + 2                             # out of range on both sides: ignored and counted
    t[-1, -1, 0] = -7
    if ign != -100:
        t[0, 1, :2] = -100                            # (then an out-of-range label like any other)
        t[0, 2, 1] = ign
    return x, t, ign


def map_labels(t, C, ign):
    """out-of-range labels -> the ignore value (what the kernels do with them; torch raises)"""
    t = t.clone()
    t[(t < 0) | (t >= C)] = ign
    return t


def softmax_parts(z, t, C, ign):
    """z [B][C][...] fp64, t the mapped labels -> (p, onehot, valid [B][1][...], m, log s, z_t)"""
    m = z.max(1, keepdim=True)[0]
    s = (z - m).exp().sum(1, keepdim=True)
    valid = (t != ign).unsqueeze(1)
    tc = torch.where(t != ign, t, torch.zeros_like(t)).unsqueeze(1)
    onehot = torch.zeros_like(z).scatter_(1, tc, 1.0) * valid
    return (z - m).exp() / s, onehot, valid, m, s.log(), z.gather(1, tc)


def ce_K(C, D, generic=False, zmax=0.0):
    """the gradient bound's K of a softmax over C classes whose largest |z - max z| is D (derivation: test_loss_instances_gpu.py)"""
    if generic:
        return 2.0 * D + zmax + 4.0 * math.log(C) + C + 8.0
    return 6.0 * D + C + 8.0


def ce_K_loss(C, D):
    return 3.0 * D + C + 8.0


def ce_reference(row):
    return _ce_reference(row.id)


@functools.lru_cache(maxsize=None)
def _ce_reference(id):
    row = BY_ID[id]
    B, C, H, W = row.shape
    x, t, ign = ce_inputs(row)
    tt = map_labels(t, C, ign)
    z = x.double().requires_grad_()
    p, onehot, valid, m, logs, zt = softmax_parts(z.detach(), tt, C, ign)
    n = int(valid.sum())
    n_bad = int(((t != ign) & ((t < 0) | (t >= C))).sum())
    D = float((m - z.detach()).max())
    K = ce_K(C, D, row.record[0] == CE_GENERIC, float(z.detach().abs().max()))
    if n == 0:
        return Ref(float('nan'), 0, n_bad, torch.zeros_like(z.detach()), torch.zeros_like(z.detach()), K, ce_K_loss(C, D), 0.0)
    loss = F.cross_entropy(z, tt, ignore_index=ign)
    loss.backward()
    Aabs = (p + onehot) * valid / n
    term = float(((1.0 + m.abs() + logs + zt.abs()) * valid).sum() / n)
    return Ref(loss.item(), n, n_bad, z.grad, Aabs, K, ce_K_loss(C, D), term)


def up_inputs(row):
    """-> (logits [B][C][h][w] fp32, target [B][H][W] int64); computed once per shape and label recipe, never written to"""
    B, C, h, w, H, W, ac, ld, ldd = row.shape
    return _up_inputs(B, C, h, w, H, W, ac, bool(row.flags.get('all_ignored')))


@functools.lru_cache(maxsize=None)
def _up_inputs(B, C, h, w, H, W, ac, all_ignored):
    key = 'lossinst/up/%d_%d_%d_%d_%d_%d_%d' % (B, C, h, w, H, W, ac)
    x = fill.uniform(key, (B, C, h, w), UP_SCALE)
    t = fill.labels(key + '/t', (B, H, W), C, block=2)
    if all_ignored:
        t[:] = -100
        t[0, 0, 0] = C                                # (one out of range: counted, still no valid pixel)
        return x, t
    t[0, :max(1, H // 4), :max(1, W // 3)] = -100     # a block of ignored pixels
    t[-1, (H - 1) // 2:(H - 1) // 2 + 2, (W - 1) // 2:(W - 1) // 2 + 3] = C + 3     # a block out of range above ...
    t[-1, (H - 1) // 2:(H - 1) // 2 + 2, :W // 4] = -7                 # ... and below (empty on the narrowest shapes)
    # an ignored pixel on a seam of the 2 x 8 tiles (the first destination row / column whose first tap is source row 2 / column 8,
    # where there is one) and one in the last, ragged tile
    i0y, i0x = up_src_index(h, H, ac)[0], up_src_index(w, W, ac)[0]
    Ys, Xs = np.nonzero(i0y >= kSY)[0], np.nonzero(i0x >= kSX)[0]
    t[0, int(Ys[0]) if len(Ys) else H - 1, int(Xs[0]) if len(Xs) else W - 1] = -100
    t[-1, H - 1, W - 1] = -100
    return x, t


def interp_matrix(n_in, n_out, ac):
    """[n_out][n_in] fp64: the bilinear weights of one axis, as torch takes them for a double tensor"""
    o = torch.arange(n_out, dtype=torch.float64)
    if ac:
        s = o * ((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0)
    else:
        s = ((o + 0.5) * (n_in / n_out) - 0.5).clamp(min=0.0)
    i0 = s.floor().long().clamp(max=n_in - 1)
    i1 = (i0 + 1).clamp(max=n_in - 1)
    l1 = s - i0
    M = torch.zeros(n_out, n_in, dtype=torch.float64)
    M[torch.arange(n_out), i0] += 1.0 - l1
    M[torch.arange(n_out), i1] += l1
    return M


def support_count(n_in, n_out):
    """an upper bound on the destination indices that touch one source index: 2 * ceil(n_out / n_in) + 1"""
    return 2 * cdiv(n_out, n_in) + 1


def up_reference(row):
    B, C, h, w, H, W, ac, ld, ldd = row.shape
    return _up_reference(B, C, h, w, H, W, ac, bool(row.flags.get('all_ignored')))


@functools.lru_cache(maxsize=None)
def _up_reference(B, C, h, w, H, W, ac, all_ignored):
    x, t = _up_inputs(B, C, h, w, H, W, ac, all_ignored)
    tt = map_labels(t, C, -100)
    n_bad = int(((t != -100) & ((t < 0) | (t >= C))).sum())
    xr = x.double().requires_grad_()
    up = F.interpolate(xr, size=(H, W), mode='bilinear', align_corners=bool(ac))
    z = up.detach()
    p, onehot, valid, m, logs, zt = softmax_parts(z, tt, C, -100)
    n = int(valid.sum())
    My, Mx = interp_matrix(h, H, ac), interp_matrix(w, W, ac)
    assert float((torch.einsum('Yi,bcij,Xj->bcYX', My, x.double(), Mx) - z).abs().max()) <= 1e-12       # the matrices are torch's weights
    D = float((m - z).max())
    zmax = float(x.abs().max())
    # the largest difference between two neighbouring low-resolution logits, per axis
    dy = float((x[:, :, 1:] - x[:, :, :-1]).abs().max()) if h > 1 else 0.0
    dx = float((x[:, :, :, 1:] - x[:, :, :, :-1]).abs().max()) if w > 1 else 0.0
    # absolute error of an interpolation weight in units of u: s = scale * o (2 roundings of a value below n_in) and 1 - l1;
    # none at ratio 1 with align_corners, where scale == 1 and s == o exactly
    wy = 0.0 if (ac and H == h) else 2.0 * h + 1.0
    wx = 0.0 if (ac and W == w) else 2.0 * w + 1.0
    Ev = 6.0 * zmax + wy * dy + wx * dx                                # absolute error of an interpolated logit, in units of u
    K = 4.0 * Ev + ce_K(C, D) + support_count(h, H) + support_count(w, W) + 8.0
    K_loss = 2.0 * Ev + ce_K_loss(C, D)
    if n == 0:
        zero = torch.zeros(B, C, h, w, dtype=torch.float64)
        return Ref(float('nan'), 0, n_bad, zero, zero, K, K_loss, 0.0)
    loss = F.cross_entropy(up, tt, ignore_index=-100)
    loss.backward()
    G = (p + onehot) * valid / n
    Aabs = torch.einsum('Yi,bcYX,Xj->bcij', My, G, Mx)
    # the gradient also takes the weights' own error: |d(w_y w_x)| <= dw_y w_x + w_y dw_x on every pixel of the support.  Folded
    # into K through the row's largest ratio of that sum to A (both from the fp64 reference alone)
    Sy, Sx = (My > 0).double(), (Mx > 0).double()
    A1 = wy * torch.einsum('Yi,bcYX,Xj->bcij', Sy, G, Mx) + wx * torch.einsum('Yi,bcYX,Xj->bcij', My, G, Sx)
    K += float((A1 / Aabs.clamp(min=1e-300)).max())
    term = float(((1.0 + m.abs() + logs + zt.abs()) * valid).sum() / n)
    return Ref(loss.item(), n, n_bad, xr.grad, Aabs, K, K_loss, term)


def check_grad(row, what, got, ref, K=None):
    """every element: |got - ref| <= K u A -> the largest error / (u A) (0 / 0 counts as 0)"""
    K = ref.K if K is None else K
    got64 = got.double()
    assert not bool(torch.isnan(got64).any()), '%s %s: %d elements are NaN (never written?)' % (row.id, what, int(torch.isnan(got64).sum()))
    err = (got64 - ref.grad).abs()
    bound = K * U * ref.A
    bad = ~(err <= bound)
    if bool(bad.any()):
        i = int(bad.reshape(-1).nonzero()[0])
        raise AssertionError('%s %s: %d of %d elements outside %.0f u A; element %d: got %.9g, fp64 %.9g, |diff| %.3e, bound %.3e'
                             % (row.id, what, int(bad.sum()), bad.numel(), K, i, got64.reshape(-1)[i].item(), ref.grad.reshape(-1)[i].item(),
                                err.reshape(-1)[i].item(), bound.reshape(-1)[i].item()))
    live = ref.A > 0
    return float((err[live] / (U * ref.A[live])).max()) if bool(live.any()) else 0.0


def check_loss(row, what, loss, ref):
    """|loss - ref| <= K_loss u mean|term| -> error / (u mean|term|); NaN exactly when no pixel is valid"""
    if ref.n_valid == 0:
        assert math.isnan(loss), '%s %s: loss %r with no valid pixel, NaN promised' % (row.id, what, loss)
        return 0.0
    err = abs(loss - ref.loss)
    assert err <= ref.K_loss * U * ref.term, '%s %s: loss %.9g, fp64 %.9g, |diff| %.3e, bound %.0f u x %.4g = %.3e' % (
        row.id, what, loss, ref.loss, err, ref.K_loss, ref.term, ref.K_loss * U * ref.term)
    return err / (U * ref.term)
