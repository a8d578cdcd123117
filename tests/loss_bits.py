"""The training losses on the device, through make_loss and the five ops.*_fwd_bwd calls, and sha256 digests of what they give.

digests(): every configuration of CONFIGS on seeded CPU-generated inputs at SHAPES, through the public surface only
(loss_fn = make_loss(name, **options); loss = loss_fn(logits, targets, None); (3 * loss).backward()) -> the sha256 of the raw
bytes of the loss and of logits.grad, and the names of the C entry points that reached _lib.call on the way, in order.
tests/golden/loss_bits.json holds them as the code produced them before the five autograd Functions became one, the loss
closures one composer over a term table, and the loss kernels' reduction helpers one header;
test_loss_bits_match_recorded (tests/test_ce_boundary_gpu.py) recomputes them, so a changed launch sequence, a moved
contraction or a changed summation order shows as a changed entry.  The file names the commit and the compiler it was
recorded under.

    python tests/loss_bits.py --record        # on a GPU: rewrites the fixture (only when the arithmetic is MEANT to change)

SHAPES are the smallest that reach each kernel form of csrc/loss.hip and csrc/ce_opts.hip: 2x3x8x8 (C <= 4, 16-byte vector
path), 1x5x7x9 (C <= 8, scalar path, HW % 4 != 0), 2x21x12x16 (C <= 24, vector path), 1x25x4x4 (C <= 32, two-wide) and
1x40x9x11 (the generic kernels; Tversky and Lovasz at a class count above one lane's registers).  Every target holds a block
of -100 labels and one label outside [0, C).  The incoming scalar of backward is 3, so pseg_scale_inplace does work.  Two
more groups at 2x21x12x16: logits at half the targets' size (the resize path) and fp16 logits.  'ops/...': the out vectors
(and gradients, and Tversky's class sums) of direct calls to the five ops.*_fwd_bwd functions at 2x21x12x16.
"""
import contextlib
import hashlib
import json
import os
import subprocess
import sys

import torch

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'loss_bits.json')
SHAPES = ((2, 3, 8, 8), (1, 5, 7, 9), (2, 21, 12, 16), (1, 25, 4, 4), (1, 40, 9, 11))
OPS_SHAPE = (2, 21, 12, 16)
BACKWARD_SCALE = 3
CE_OPTS = dict(label_smoothing=0.1, focal_gamma=2.0)        # plus class_weight=class_weights(C)
TVERSKY_OPTS = dict(tversky_alpha=0.3, tversky_beta=0.7, tversky_power=1.5, tversky_per_image=True, tversky_weight=0.5)
BOUNDARY = dict(boundary_boost=2.0, boundary_width=2)


def class_weights(C):
    return [0.5 + 0.25 * (c % 5) for c in range(C)]


def configs(C):
    """[(tag, loss name, options)]: what test_loss_bits_match_recorded runs at every shape"""
    w = class_weights(C)
    rows = [(name, name, {}) for name in ('ce', 'lovasz', 'ce+lovasz', 'tversky', 'ce+tversky')]
    rows += [('ce/weighted-smoothed-focal', 'ce', dict(CE_OPTS, class_weight=w)),
             ('ce/weighted-smoothed-focal-keep', 'ce', dict(CE_OPTS, class_weight=w, keep_ratio=0.25)),
             ('ce+lovasz/focal', 'ce+lovasz', dict(focal_gamma=2.0)),
             ('tversky/configured', 'tversky', dict(TVERSKY_OPTS)),
             ('ce+tversky/weight-keep', 'ce+tversky', dict(tversky_weight=0.5, keep_ratio=0.25))]
    rows += [('ce/boundary-' + f, 'ce', dict(BOUNDARY, boundary_falloff=f)) for f in ('flat', 'linear', 'gaussian')]
    rows += [('ce+tversky/boundary-smoothed-keep', 'ce+tversky', dict(BOUNDARY, label_smoothing=0.1, keep_ratio=0.25))]
    return rows


def make_case(shape, logits_hw=None):
    """seeded CPU logits [B, C, *logits_hw or H, W] and int64 targets [B, H, W] with a -100 block and one label C + 1"""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(7000 + 101 * C + H * W)
    h, w = logits_hw or (H, W)
    logits = torch.randn(B, C, h, w, generator=g) * 3
    target = torch.randint(0, C, (B, H, W), generator=g)
    target[:, :2, 1:4] = -100
    target[B - 1, H - 1, W - 1] = C + 1
    return logits, target


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


@contextlib.contextmanager
def recorded_calls(names):
    """inside: every _lib.call appends its entry point's name to `names`"""
    from pytorch_segmentation_amd import _lib
    call = _lib.call

    def recording(name, *args):
        names.append(name)
        return call(name, *args)

    _lib.call = recording
    try:
        yield names
    finally:
        _lib.call = call


def evaluate(loss_fn, logits, target):
    x = logits.cuda().requires_grad_(True)
    t = target.cuda()
    with recorded_calls([]) as names:
        loss = loss_fn(x, t, None)
        (BACKWARD_SCALE * loss).backward()
    torch.cuda.synchronize()
    return {'loss': sha(loss), 'grad': sha(x.grad), 'calls': list(names)}


def ops_digests(ops, out):
    from pytorch_segmentation_amd.utils.loss import boundary_weight_table
    B, C, H, W = OPS_SHAPE
    logits, target = make_case(OPS_SHAPE)
    x, t = logits.cuda().contiguous(), target.cuda().contiguous()
    w = torch.tensor(class_weights(C), dtype=torch.float32).cuda()
    depth = ops.label_depth(t, C, BOUNDARY['boundary_width'], edge=False)
    table = ops.bin_weight_table(boundary_weight_table(BOUNDARY['boundary_width'], BOUNDARY['boundary_boost']), 'cuda')
    runs = {'ce_fwd_bwd': lambda g: ops.ce_fwd_bwd(x, t, want_grad=g),
            'ce_opts_fwd_bwd': lambda g: ops.ce_opts_fwd_bwd(x, t, w, 0.1, 2.0, 0.25, want_grad=g),
            'ce_opts_binned_fwd_bwd': lambda g: ops.ce_opts_binned_fwd_bwd(x, t, depth, table, w, 0.1, 2.0, 0.25, want_grad=g),
            'lovasz_softmax_fwd_bwd': lambda g: ops.lovasz_softmax_fwd_bwd(x, t, want_grad=g),
            'tversky_fwd_bwd': lambda g: ops.tversky_fwd_bwd(x, t, 0.3, 0.7, 1.0, 1.5, True, False, want_grad=g, want_sums=True)}
    for name, run in runs.items():
        for want_grad in (True, False):
            with recorded_calls([]) as names:
                got = run(want_grad)
            torch.cuda.synchronize()
            assert (got[1] is None) == (not want_grad)
            d = {'out': sha(got[0]), 'calls': list(names)}
            if want_grad:
                d['grad'] = sha(got[1])
            if len(got) == 3:
                d['sums'] = sha(got[2])
            out['ops/%s/want_grad=%d' % (name, want_grad)] = d


def digests(ops):
    """{case: {'loss': sha256, 'grad': sha256, 'calls': [entry points]}} over CONFIGS x SHAPES, the resize and fp16 cases,
    and {'out': ..., 'calls': ...} of the direct ops calls"""
    from pytorch_segmentation_amd.utils import loss as L
    check, L.CHECK_LABELS = L.CHECK_LABELS, False      # (every target holds a label outside [0, C))
    try:
        out = {}
        for shape in SHAPES:
            logits, target = make_case(shape)
            for tag, name, options in configs(shape[1]):
                out['%dx%dx%dx%d/%s' % (shape + (tag,))] = evaluate(L.make_loss(name, **options), logits, target)
        B, C, H, W = OPS_SHAPE
        rows = {r[0]: r for r in configs(C)}
        logits, target = make_case(OPS_SHAPE, (H // 2, W // 2))
        for tag in ('ce', 'ce+lovasz', 'ce+tversky/weight-keep', 'ce/boundary-gaussian'):
            out['resize/' + tag] = evaluate(L.make_loss(rows[tag][1], **rows[tag][2]), logits, target)
        logits, target = make_case(OPS_SHAPE)
        for tag in ('ce+lovasz', 'tversky', 'ce/weighted-smoothed-focal', 'ce+tversky/boundary-smoothed-keep'):
            out['fp16/' + tag] = evaluate(L.make_loss(rows[tag][1], **rows[tag][2]), logits.half(), target)
        ops_digests(ops, out)
        return out
    finally:
        L.CHECK_LABELS = check


if __name__ == '__main__':
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, repo)
    assert '--record' in sys.argv, 'python tests/loss_bits.py --record'
    assert torch.cuda.is_available(), 'the digests are those of the GPU kernels'
    from optim_bits import compiler_line
    from pytorch_segmentation_amd import ops as _ops
    commit = subprocess.run(['git', '-C', repo, 'rev-parse', 'HEAD'], stdout=subprocess.PIPE,
                            stderr=subprocess.DEVNULL).stdout.decode().strip()
    commit = next((a.split('=', 1)[1] for a in sys.argv if a.startswith('--commit=')), commit)
    rec = {'commit': commit, 'compiler': compiler_line(), 'digests': digests(_ops)}
    with open(next((a.split('=', 1)[1] for a in sys.argv if a.startswith('--out=')), FIXTURE), 'w') as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write('\n')
    print('recorded %d cases from %s under %s' % (len(rec['digests']), rec['commit'], rec['compiler']))
