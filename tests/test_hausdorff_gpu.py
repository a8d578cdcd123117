"""pseg_hausdorff_stats and everything above it on the GPU, against tests/hausdorff_ref.py.  The integer fields must be equal.
The two sums must agree to a relative 1e-12: the terms are positive and a test has fewer than 10^4 of them, so a double
summation in any fixed order stays below n * 2^-53 of the sum."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import hausdorff_ref as R

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-12
_cache = {}


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from pytorch_segmentation_amd import ops as _ops
    return _ops


def _case(shape):
    """(target, pred, (stats, sums)) of a generated case, built once and left unchanged"""
    if shape not in _cache:
        t, p = R.make_case(*shape, seed=R.SEED)
        for a in (t, p):
            a.setflags(write=False)
        _cache[shape] = (t, p, R.stats_brute(p, t, shape[1]))
    return _cache[shape]


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a)).cuda()          # (a copy: the cached arrays are read-only)


def _same(got, want, what=''):
    stats, sums = got
    assert stats.dtype == torch.int64 and sums.dtype == torch.float64
    assert tuple(stats.shape) == want[0].shape and tuple(sums.shape) == want[1].shape
    np.testing.assert_array_equal(stats.cpu().numpy(), want[0], err_msg=what)
    np.testing.assert_allclose(sums.cpu().numpy(), want[1], rtol=RTOL, atol=0.0, err_msg=what)


@pytest.mark.parametrize('shape', R.SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_records_of_the_generated_cases(ops, shape):
    t, p, want = _case(shape)
    assert want[0][..., :2].sum() < 10 ** 4                      # the terms of the sums: what RTOL is worked out for
    _same(ops.hausdorff_stats(_dev(p), _dev(t), shape[1]), want)


@pytest.mark.parametrize('kind', R.SPECIAL)
def test_records_of_the_hand_made_maps(ops, kind):
    t, p, C = R.special(kind)
    _same(ops.hausdorff_stats(_dev(p), _dev(t), C), R.stats_brute(p, t, C))


@pytest.mark.parametrize('shape', [(1, 2, 3, 9000), (1, 2, 2, 16384)], ids=lambda s: 'x'.join(map(str, s)))
def test_rows_wider_than_the_shared_tile(ops, shape):
    """a row of more than 8192 pixels has a block of the row pass to itself, and the widest takes all 64 KiB of LDS"""
    t, p = R.make_case(*shape, seed=2)
    want = R.stats_scipy(p, t, shape[1])
    assert (want[0][..., 2:4] > 255 ** 2).any()                  # distances beyond every band width
    stats, sums = ops.hausdorff_stats(_dev(p), _dev(t), shape[1])
    np.testing.assert_array_equal(stats.cpu().numpy(), want[0])
    # up to 20000 positive terms per sum here: either summation is within n * 2^-53 of the exact sum
    n = int(want[0][..., :2].max())
    assert 10 ** 4 < n <= 20000
    np.testing.assert_allclose(sums.cpu().numpy(), want[1], rtol=2 * n * 2.0 ** -53, atol=0.0)


def test_quantiles_and_tolerances(ops):
    shape = (2, 5, 24, 40)
    t, p, _ = _case(shape)
    dt, dp = _dev(t), _dev(p)
    seen = set()
    for permille in (500, 950, 1000):
        for tol in (0, 2, 255):
            want = R.stats_brute(p, t, shape[1], permille, tol)
            _same(ops.hausdorff_stats(dp, dt, shape[1], permille, tol), want, 'permille %d tol %d' % (permille, tol))
            seen.add(want[0][..., 4:].tobytes())
    assert len(seen) == 9                                        # every setting changes the record
    with pytest.raises(ValueError, match='permille'):
        ops.hausdorff_stats(dp, dt, 5, permille=0)
    with pytest.raises(ValueError, match='tol'):
        ops.hausdorff_stats(dp, dt, 5, tol=256)


def test_views_at_an_address_that_is_not_16_byte_aligned(ops):
    shape = (2, 4, 31, 64)
    t, p, want = _case(shape)
    n = t.size
    bt, bp = torch.zeros(n + 1, dtype=torch.int64, device='cuda'), torch.zeros(n + 1, dtype=torch.int64, device='cuda')
    vt, vp = bt[1:].view(t.shape), bp[1:].view(p.shape)
    vt.copy_(_dev(t))
    vp.copy_(_dev(p))
    assert vt.data_ptr() % 16 == 8 and vp.data_ptr() % 16 == 8 and vt.is_contiguous()
    _same(ops.hausdorff_stats(vp, vt, shape[1]), want)


def test_two_calls_give_the_same_bytes(ops):
    shape = (3, 21, 17, 23)
    t, p, want = _case(shape)
    dt, dp = _dev(t), _dev(p)
    a = ops.hausdorff_stats(dp, dt, shape[1])
    b = ops.hausdorff_stats(dp, dt, shape[1])
    assert torch.equal(a[0], b[0]) and a[1].cpu().numpy().tobytes() == b[1].cpu().numpy().tobytes()
    _same(b, want)


def test_a_batch_walked_in_chunks(ops, monkeypatch):
    from pytorch_segmentation_amd import _lib
    shape = (3, 21, 17, 23)
    t, p, want = _case(shape)
    dt, dp = _dev(t), _dev(p)
    whole = ops.hausdorff_stats(dp, dt, shape[1])
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, 'call', lambda name, *a: calls.append((name, a[2])) or real(name, *a))
    monkeypatch.setattr(ops, 'HAUSDORFF_MAX_IMAGES', 2)
    chunked = ops.hausdorff_stats(dp, dt, shape[1])
    assert calls == [('pseg_hausdorff_stats', 2), ('pseg_hausdorff_stats', 1)]
    assert torch.equal(whole[0], chunked[0]) and whole[1].cpu().numpy().tobytes() == chunked[1].cpu().numpy().tobytes()
    _same(chunked, want)


def test_update_surface_stats_over_two_batches(ops):
    from pytorch_segmentation_amd.utils import compute_surface_metrics, update_surface_stats
    C = 5
    acc = torch.zeros(7, C, dtype=torch.float64, device='cuda')
    ref = np.zeros((7, C))
    for shape, seed in (((2, C, 24, 40), R.SEED), ((3, C, 17, 23), 11)):
        t, p = R.make_case(*shape, seed=seed)
        assert update_surface_stats(acc, _dev(p), _dev(t).int(), 900, 1) is acc          # (targets of another integer type)
        R.accumulate(ref, *R.stats_brute(p, t, C, 900, 1))
    got = acc.cpu().numpy()
    np.testing.assert_array_equal(got[[0, 4, 6]], ref[[0, 4, 6]])                        # the counts
    np.testing.assert_allclose(got, ref, rtol=RTOL, atol=0.0)
    assert (ref[0] >= 2).sum() >= 3 and ref[6].sum() >= 1        # classes defined in several images, and misses
    for a, b in zip(compute_surface_metrics(acc), R.metrics(ref)):
        np.testing.assert_allclose(a.numpy(), b, rtol=RTOL, atol=0.0, equal_nan=True)


# ------------------------------------------------------------------ test.py
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


def test_evaluation_with_and_without_the_flag(ops, capsys, monkeypatch):
    from pytorch_segmentation_amd import _lib
    spec = importlib.util.spec_from_file_location('pseg_eval_cli_hausdorff_gpu', os.path.join(REPO, 'test.py'))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    C = 4
    classes = ['c%d' % c for c in range(C)]
    logits, batches, maps = [], [], []
    for shape, seed in (((2, C, 24, 40), 5), ((2, C, 17, 23), 6)):         # two batches of different size
        t, p = R.make_case(*shape, seed=seed)
        p = np.where((p >= 0) & (p < C), p, 0)                             # what an argmax can say
        logits.append((torch.nn.functional.one_hot(torch.from_numpy(p), C).permute(0, 3, 1, 2).float() * 8).contiguous().cuda())
        batches.append((torch.zeros(shape[0], 3, *shape[2:], device='cuda'), torch.from_numpy(t).cuda()))
        maps.append((t, p))
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, 'call', lambda name, *a: calls.append(name) or real(name, *a))

    capsys.readouterr()
    plain = cli.test(_Stub(logits), _Batches(batches, classes))
    plain_out = capsys.readouterr().out.splitlines()
    assert calls and not [n for n in calls if n.startswith('pseg_hausdorff')]
    assert 'hd' not in '\n'.join(plain_out)

    del calls[:]
    results = {}
    got = cli.test(_Stub(logits), _Batches(batches, classes), surface_distance=True, hd_percentile=90.0, surface_tolerance=1,
                   results=results)
    out = capsys.readouterr().out.splitlines()
    assert got == plain                                                    # the return value stays the mean IoU
    assert calls.count('pseg_hausdorff_stats') == 2
    ref = np.zeros((7, C))
    for t, p in maps:
        R.accumulate(ref, *R.stats_brute(p, t, C, 900, 1))
    np.testing.assert_allclose(results['surface_stats'].numpy(), ref, rtol=RTOL, atol=0.0)
    hd, hd95, assd, nsd, misses = R.metrics(ref)
    for key, want in (('hd', hd), ('hd95', hd95), ('assd', assd), ('nsd', nsd), ('surface_misses', misses)):
        assert results[key].dtype == torch.float64 and tuple(results[key].shape) == (C,)
        np.testing.assert_allclose(results[key].numpy(), want, rtol=RTOL, atol=0.0, equal_nan=True)
    assert (~np.isnan(hd)).sum() >= 3 and np.nanmax(hd) > 1
    assert out[0] == plain_out[0]
    assert out[1] == 'hd: %8g, hd90: %8g, assd: %8g, nsd@1: %8g, misses: %d' % (np.nanmean(hd), np.nanmean(hd95), np.nanmean(assd),
                                                                                  np.nanmean(nsd), misses.sum())
    assert out[2:] == [r + ', hd: %8g, hd90: %8g, assd: %8g, nsd: %8g' % (hd[c], hd95[c], assd[c], nsd[c])
                       for c, r in enumerate(plain_out[1:])]

    # it composes with --boundary: both summary lines and both sets of columns
    results = {}
    cli.test(_Stub(logits), _Batches(batches, classes), boundary_width=2, surface_distance=True, results=results)
    out = capsys.readouterr().out.splitlines()
    assert out[1].startswith('boundary iou: ') and out[2].startswith('hd: ') and ', hd95: ' in out[2]
    assert all(', biou: ' in r and r.index(', biou: ') < r.index(', hd: ') for r in out[3:]) and len(out) == 3 + C
    assert {'boundary_iou', 'hd', 'hd95', 'assd', 'nsd', 'surface_misses', 'surface_stats'} <= set(results)
