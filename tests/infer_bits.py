"""The inference kernels on the device, as the tests call them, and sha256 digests of what they write.

digests(): the six public entry points of csrc/infer.hip plus softmax_views, through ops, on seeded inputs at the shapes of
tests/test_tta_gpu.py and tests/test_slide_gpu.py -> the sha256 of the raw bytes of every output tensor.
tests/golden/infer_bits.json holds those digests as the kernels produced them before the three preprocess kernels became one
template and the three decode kernels took their class scan and pixel store from shared helpers;
test_infer_bits_match_recorded (tests/test_inference_gpu.py) recomputes them, so a moved contraction or a changed
accumulation order shows as a changed digest.  The file names the commit and the compiler it was recorded under.

    python tests/infer_bits.py --record        # on a GPU: rewrites the fixture (only when the arithmetic is MEANT to change)

image_preprocess / _views / _windows: photos PRE_SIZES -> 32 x 48, bgr both ways, both NORMS; views plain + mirrored;
windows at working scales 1.0 and 0.5, every window of window_grid at WIN / STRIDE (those hanging over the working image
included), plain + mirrored.  seg_decode, seg_decode_ensemble (2 maps) and seg_decode_windows (scales 1.0 and 0.5) over
DEC_SIZES at C in {2, 8, 9, 21, 150} -- 8 and 9 are the two sides of the class-padding switch, 150 takes more than one
32-class chunk -- the latter two with pairs 0 and 1; the mask, and at C = 21 also the colours.
"""
import hashlib
import json
import os
import subprocess
import sys

import torch

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'infer_bits.json')
PRE_OUT = (32, 48)
WORK_SCALES = (1.0, 0.5)
CLASSES = (2, 8, 9, 21, 150)
ENS_MAPS = [(32, 48), (64, 96)]


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def preprocess_digests(ops, out):
    from pytorch_segmentation_amd.utils.inference import NORMS, window_grid, work_size
    from test_slide_gpu import PRE_SIZES, STRIDE, _rows, _src
    from test_tta_gpu import _photos
    oh, ow = PRE_OUT
    photos = _photos(PRE_SIZES, 11)
    src, offs = _src(photos)
    heads = [[o, p.shape[0], p.shape[1]] for o, p in zip(offs, photos)]
    plain = torch.tensor(heads, dtype=torch.int64, device=src.device)
    views = torch.tensor([hd + [f] for f in (0, ops.VIEW_MIRROR) for hd in heads], dtype=torch.int64, device=src.device)
    windows = {}
    for s in WORK_SCALES:
        rows = []
        for hd in heads:
            Hs, Ws = work_size(hd[1], hd[2], s)
            origins, _ = window_grid(Hs, Ws, oh, ow, *STRIDE)
            rows += [hd + [f, Hs, Ws, y0, x0] for f in (0, ops.VIEW_MIRROR) for y0, x0 in origins]
        windows[s] = _rows(rows)
    for norm in sorted(NORMS):
        mean, std = NORMS[norm]
        for bgr in (0, 1):
            tag = 'bgr=%d/norm=%s' % (bgr, norm)
            out['image_preprocess/' + tag] = {'out': sha(ops.image_preprocess(src, plain, oh, ow, mean, std, bgr))}
            out['image_preprocess_views/' + tag] = {'out': sha(ops.image_preprocess_views(src, views, oh, ow, mean, std, bgr))}
            for s in WORK_SCALES:
                got = ops.image_preprocess_windows(src, windows[s], oh, ow, mean, std, bgr)
                out['image_preprocess_windows/scale=%g/%s' % (s, tag)] = {'out': sha(got)}


def _named(mask, rgb, C):
    d = {'mask': sha(mask)}
    if rgb is not None:
        assert C == 21
        d['rgb'] = sha(rgb)
    return d


def decode_digests(ops, out):
    import slide_ref
    from test_slide_gpu import DEC_SIZES, STRIDE, WIN, _pack_groups, _packed_table
    from test_tta_gpu import DEV, _maps
    h, w = WIN
    B = len(DEC_SIZES)
    rows, total = _packed_table(DEC_SIZES)
    table = torch.tensor(rows, dtype=torch.int64, device=DEV)
    max_hw = (max(H for H, _ in DEC_SIZES), max(W for _, W in DEC_SIZES))
    work = [[slide_ref.work_size(H, W, s) for H, W in DEC_SIZES] for s in WORK_SCALES]
    for C in CLASSES:
        g = torch.Generator().manual_seed(500 + C)
        lut = torch.randint(0, 256, (256, 3), dtype=torch.uint8, generator=g).to(DEV) if C == 21 else None
        logits = torch.randn(B, C, h, w, generator=g) * 3
        out['seg_decode/C=%d' % C] = _named(*ops.seg_decode(logits.to(DEV), table, total, lut), C)
        for pairs in (0, 1):
            V = 2 if pairs else 1
            tag = 'C=%d/pairs=%d' % (C, pairs)
            maps_in = [torch.randn(V * B, C, hs, ws, generator=g) * 3 for hs, ws in ENS_MAPS]
            prob, maps, _ = _maps(maps_in, pairs)
            out['softmax_views/maps/' + tag] = {'prob': sha(prob)}
            out['seg_decode_ensemble/' + tag] = _named(*ops.seg_decode_ensemble(prob, maps, B, C, table, total, max_hw, lut), C)
            win_in = [[torch.randn(len(slide_ref.grid(Hs, Ws, h, w, *STRIDE)[0]) * V, C, h, w, generator=g) * 3
                       for Hs, Ws in sizes] for sizes in work]
            prob, groups = _pack_groups(win_in, work, pairs)
            out['softmax_views/windows/' + tag] = {'prob': sha(prob)}
            out['seg_decode_windows/' + tag] = _named(
                *ops.seg_decode_windows(prob, groups, B, C, WIN, STRIDE, table, total, max_hw, lut), C)


def digests(ops):
    """{case: {tensor: sha256 of its bytes}} over every entry point of csrc/infer.hip"""
    out = {}
    preprocess_digests(ops, out)
    decode_digests(ops, out)
    return out


if __name__ == '__main__':
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, repo)
    assert '--record' in sys.argv, 'python tests/infer_bits.py --record'
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
