"""pseg_label_depth / pseg_boundary_counts and everything above them on the GPU.  Every comparison is exact equality against
tests/boundary_ref.py: the kernels are integer arithmetic, there is no tolerance and nothing is left out."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import boundary_ref as R

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_cache = {}


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from pytorch_segmentation_amd import ops as _ops
    return _ops


def _case(case):
    """(target, pred, expected counters) of a case, built once and left unchanged"""
    if case not in _cache:
        T = R.make_target(case)
        P = R.make_pred(case, T)
        for a in (T, P):
            a.setflags(write=False)
        _cache[case] = (T, P, R.boundary_counts(P, T, case[3], case[4]))
    return _cache[case]


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a)).cuda()          # (a copy: the cached arrays are read-only)


# ------------------------------------------------------------------ pseg_label_depth
@pytest.mark.parametrize('edge', [False, True], ids=['depth', 'depth_edge'])
@pytest.mark.parametrize('case', R.CASES, ids=R.case_id)
def test_label_depth(ops, case, edge):
    B, H, W, C, d = case
    T, P, _ = _case(case)
    for L in (T, P):                                     # the prediction carries the shifted void specks as well
        got = ops.label_depth(_dev(L), C, d, edge)
        assert got.dtype == torch.uint8 and got.shape == (B, H, W)
        np.testing.assert_array_equal(got.cpu().numpy().astype(np.int64), R.label_depth(L, d, edge))


def test_label_depth_of_one_pixel_and_of_a_uniform_image(ops):
    for value in (1, -100):                              # a valid and a void pixel: nothing differs, the edge is 1 away
        L = torch.full((1, 1, 1), value, dtype=torch.int64, device='cuda')
        assert ops.label_depth(L, 2, 1).item() == 2 and ops.label_depth(L, 2, 1, edge=True).item() == 1
    (B, H, W, C, d), L = R.uniform_case()
    got = ops.label_depth(_dev(L), C, d)
    assert (got == d + 1).all()
    np.testing.assert_array_equal(ops.label_depth(_dev(L), C, d, edge=True).cpu().numpy(), np.minimum(d + 1, R.edge_distance(H, W))[None].repeat(B, 0))


def test_void_values_compare_by_value(ops):
    """two different void values next to each other are a label change; equal ones are not"""
    L = torch.full((1, 9, 9), -100, dtype=torch.int64)
    assert (ops.label_depth(L.cuda(), 3, 2) == 3).all()
    L[0, :, 5:] = 255
    got = ops.label_depth(L.cuda(), 3, 2).cpu()
    assert got[0, :, 4].eq(1).all() and got[0, :, 5].eq(1).all() and got[0, :, 3].eq(2).all() and got[0, :, 0].eq(3).all()
    np.testing.assert_array_equal(got.numpy(), R.label_depth(L.numpy(), 2))


# ------------------------------------------------------------------ pseg_boundary_counts
@pytest.mark.parametrize('case', R.CASES, ids=R.case_id)
def test_boundary_counts(ops, case):
    B, H, W, C, d = case
    T, P, want = _case(case)
    cnt = torch.zeros(6, C, dtype=torch.int64, device='cuda')
    ops.boundary_counts(_dev(P), _dev(T), cnt, d)
    np.testing.assert_array_equal(cnt.cpu().numpy(), want)
    ops.boundary_counts(_dev(P), _dev(T), cnt, d)        # a second call accumulates
    np.testing.assert_array_equal(cnt.cpu().numpy(), 2 * want)
    if case in R.RICH:
        assert 0 < want[0].sum() < want[1].sum()         # the intersection lies strictly between nothing and the band


def test_boundary_counts_of_one_pixel(ops):
    one = lambda v: torch.full((1, 1, 1), v, dtype=torch.int64, device='cuda')
    cnt = torch.zeros(6, 2, dtype=torch.int64, device='cuda')
    ops.boundary_counts(one(1), one(1), cnt, 1)          # right: in both bands through the edge, not in the trimap
    assert cnt.cpu().tolist() == [[0, 1], [0, 1], [0, 1], [0, 0], [0, 0], [0, 0]]
    ops.boundary_counts(one(0), one(-100), cnt, 1)       # a void target counts nowhere
    assert cnt.cpu().tolist() == [[0, 1], [0, 1], [0, 1], [0, 0], [0, 0], [0, 0]]


@pytest.mark.parametrize('case', [R.CASES[0], R.CASES[4]], ids=R.case_id)
def test_trimap_rows_over_the_whole_image_are_the_confusion_counts(ops, case):
    """with d large enough to reach every contour from every pixel, rows 3-5 are pseg_confusion on the valid-target pixels"""
    B, H, W, C, _ = case
    T, P, _ = _case(case)
    d = max(H, W)
    assert (R.label_depth(T, d) <= d).all()
    cnt = torch.zeros(6, C, dtype=torch.int64, device='cuda')
    ops.boundary_counts(_dev(P), _dev(T), cnt, d)
    valid = (T >= 0) & (T < C)
    conf = torch.zeros(3, C, dtype=torch.int64, device='cuda')
    ops.confusion(_dev(P[valid]), _dev(T[valid]), conf)
    assert torch.equal(cnt[3:], conf)
    np.testing.assert_array_equal(cnt.cpu().numpy(), R.boundary_counts(P, T, C, d))


def test_prediction_values_outside_the_classes(ops):
    """a prediction outside [0, C) on a valid target: a miss of the target's class, no false alarm, not in pband; and it is a
    label of its own for the prediction's contours"""
    C, d = 3, 2
    T = np.zeros((1, 12, 12), dtype=np.int64)
    T[0, :, 6:] = 1
    P = T.copy()
    P[0, 2:5, 3:6] = 7
    P[0, 8, 7] = -5
    want = R.boundary_counts(P, T, C, d)
    cnt = torch.zeros(6, C, dtype=torch.int64, device='cuda')
    ops.boundary_counts(_dev(P), _dev(T), cnt, d)
    np.testing.assert_array_equal(cnt.cpu().numpy(), want)
    assert want[5].sum() == 0 and want[4].sum() > 0 and want[2].sum() < (R.label_depth(P, d, True) <= d).sum()


def test_counts_on_a_side_stream(ops):
    case = R.CASES[4]
    B, H, W, C, d = case
    T, P, want = _case(case)
    t, p = _dev(T), _dev(P)
    cnt = torch.zeros(6, C, dtype=torch.int64, device='cuda')
    busy = torch.randn(2048, 2048, device='cuda')
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    for _ in range(8):                                   # keep the default stream busy meanwhile
        busy = busy @ busy * 1e-3
    with torch.cuda.stream(side):
        ops.boundary_counts(p, t, cnt, d)
        depth = ops.label_depth(t, C, d, True)
    side.synchronize()
    np.testing.assert_array_equal(cnt.cpu().numpy(), want)
    np.testing.assert_array_equal(depth.cpu().numpy().astype(np.int64), R.label_depth(T, d, True))
    torch.cuda.synchronize()


def test_wrappers_check_their_arguments(ops):
    t = torch.zeros(2, 8, 8, dtype=torch.int64, device='cuda')
    cnt = torch.zeros(6, 3, dtype=torch.int64, device='cuda')
    with pytest.raises(AssertionError):
        ops.label_depth(t.int(), 3, 2)
    with pytest.raises(AssertionError):
        ops.label_depth(t[:, :, ::2], 3, 2)
    with pytest.raises(RuntimeError, match='HIP path only'):
        ops.label_depth(t.cpu(), 3, 2)
    with pytest.raises(AssertionError):
        ops.boundary_counts(t, t[:1], cnt, 2)
    with pytest.raises(AssertionError):
        ops.boundary_counts(t, t, cnt[:3], 2)
    with pytest.raises(ValueError, match='out of range'):
        ops.boundary_counts(t, t, cnt, 255)
    assert not cnt.any()


# ------------------------------------------------------------------ utils and test.py
def test_update_and_metrics_against_the_reference(ops):
    from pytorch_segmentation_amd.utils import compute_boundary_metrics, update_boundary_counts
    case = R.CASES[0]
    T, P, want = _case(case)
    cnt = torch.zeros(6, case[3], dtype=torch.int64, device='cuda')
    assert update_boundary_counts(cnt, _dev(P), _dev(T).int(), case[4]) is cnt          # (targets of another integer type)
    np.testing.assert_array_equal(cnt.cpu().numpy(), want)
    biou, tiou = compute_boundary_metrics(cnt)
    rb, rt = R.metrics(want)
    np.testing.assert_array_equal(biou.numpy(), rb)
    np.testing.assert_array_equal(tiou.numpy(), rt)
    assert 0 < rb.min() and rb.max() < 1


class _Stub(torch.nn.Module):
    """returns the fixed logits of the batches in turn"""

    def __init__(self, logits):
        super().__init__()
        self.logits, self.i = logits, 0

    def forward(self, x):
        out = self.logits[self.i % len(self.logits)]
        self.i += 1
        return out


class _Batches:
    def __init__(self, batches, classes):
        self.batches = batches
        self.loader = type('L', (), {'dataset': type('D', (), {'classes': classes})()})()

    def __iter__(self):
        return iter(self.batches)


def _evaluation():
    spec = importlib.util.spec_from_file_location('pseg_eval_cli_boundary_gpu', os.path.join(REPO, 'test.py'))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    C, sizes = 4, [(2, 64, 96), (2, 40, 40)]             # two batches of different size: the width follows each (2 and 1)
    logits, batches, maps = [], [], []
    for i, (B, H, W) in enumerate(sizes):
        case = (B, H, W, C, 1 + i)
        T = R.make_target(case, seed=5)
        P = R.make_pred(case, T, seed=5)
        P = np.where((P >= 0) & (P < C), P, 0)               # what an argmax can say
        onehot = torch.nn.functional.one_hot(torch.from_numpy(P), C).permute(0, 3, 1, 2).float() * 8
        logits.append(onehot.contiguous().cuda())
        batches.append((torch.zeros(B, 3, H, W, device='cuda'), torch.from_numpy(T).cuda()))
        maps.append((T, P))
    return cli, C, logits, batches, maps


def test_evaluation_with_and_without_the_flags(ops, capsys):
    from pytorch_segmentation_amd.utils import compute_metrics, update_class_counts
    cli, C, logits, batches, maps = _evaluation()
    classes = ['c%d' % c for c in range(C)]
    # what the evaluation printed before the flags existed, from the counters it is defined by
    conf = torch.zeros(3, C, dtype=torch.int64, device='cuda')
    for (T, P) in maps:
        update_class_counts(conf, _dev(P), _dev(T))
    tp, fn, fp = (c.float() for c in conf.cpu())
    Tn, Pr, Rc, miou, F1 = compute_metrics(tp, fn, fp)
    rows = ['cls: %8s, targets: %8d, pre: %8g, rec: %8g, iou: %8g, F1: %8g' % (classes[c], Tn[c], Pr[c], Rc[c], miou[c], F1[c])
            for c in range(C)]
    capsys.readouterr()
    got = cli.test(_Stub(logits), _Batches(batches, classes))
    out = capsys.readouterr().out.splitlines()
    assert got == miou.mean().item()
    assert out[0].startswith('loss: ') and out[0].endswith('mAP: %8g, F1: %8g, miou: %8g' % (Pr.mean(), F1.mean(), miou.mean()))
    assert out[1:] == rows and 'boundary' not in '\n'.join(out)
    plain_first = out[0]

    results = {}
    got = cli.test(_Stub(logits), _Batches(batches, classes), boundary=0.02, results=results)
    out = capsys.readouterr().out.splitlines()
    widths = [R.width(T.shape[1:]) for T, _ in maps]
    assert widths == [2, 1]
    want = sum(R.boundary_counts(P, T, C, w) for (T, P), w in zip(maps, widths))
    rb, rt = R.metrics(want)
    assert got == miou.mean().item()                     # the return value stays the mean IoU
    np.testing.assert_array_equal(results['boundary_counters'].numpy(), want)
    np.testing.assert_array_equal(results['boundary_iou'].numpy(), rb)
    np.testing.assert_array_equal(results['trimap_iou'].numpy(), rt)
    assert results['boundary_widths'] == sorted(set(widths))
    assert out[0] == plain_first
    assert out[1] == 'boundary iou: %8g, trimap iou: %8g, width: %s' % (torch.from_numpy(rb).mean(), torch.from_numpy(rt).mean(), '1 2')
    assert out[2:] == [r + ', biou: %8g, trimap: %8g' % (rb[c], rt[c]) for c, r in enumerate(rows)]

    results = {}
    cli.test(_Stub(logits), _Batches(batches, classes), boundary_width=3, results=results)
    capsys.readouterr()
    np.testing.assert_array_equal(results['boundary_counters'].numpy(), sum(R.boundary_counts(P, T, C, 3) for T, P in maps))
    assert results['boundary_widths'] == [3]
