"""Surface-distance evaluation without a GPU: the two numpy restatements of pseg_hausdorff_stats' contract
(tests/hausdorff_ref.py) against each other and on hand-made maps, the coverage of the generated cases, and the host
interface: header, library exports and refusals, compute_surface_metrics, test.py's flags, the CPU-tensor refusals."""
import ctypes
import importlib.util
import inspect
import math
import os

import numpy as np
import pytest
import torch

import hausdorff_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_cache = {}


def _case(shape):
    if shape not in _cache:
        t, p = R.make_case(*shape, seed=R.SEED)
        _cache[shape] = (t, p, R.stats_brute(p, t, shape[1]))
    return _cache[shape]


# ------------------------------------------------------------------ the two restatements
@pytest.mark.parametrize('shape', R.SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_scipy_equals_all_pairs(shape):
    B, C, H, W = shape
    t, p, (stats, sums) = _case(shape)
    s2, f2 = R.stats_scipy(p, t, C)
    assert stats.dtype == np.int64 and stats.shape == (B, C, 8) and sums.shape == (B, C, 2)
    np.testing.assert_array_equal(stats, s2)
    np.testing.assert_array_equal(sums, f2)
    for permille, tol in ((500, 0), (1000, 255), (1, 1)):
        a, b = R.stats_brute(p, t, C, permille, tol), R.stats_scipy(p, t, C, permille, tol)
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])
    assert stats[..., 2:6].max() <= (H - 1) ** 2 + (W - 1) ** 2


def test_quantile_is_the_kth_of_the_sorted_list_and_permille_1000_the_maximum():
    shape = (2, 5, 24, 40)
    t, p, _ = _case(shape)
    P, G = R.masks(p, t, 5)
    seen = 0
    for permille in (1, 500, 950, 999, 1000):
        stats, _ = R.stats_brute(p, t, 5, permille, 2)
        for b in range(2):
            for c in range(5):
                bp, bg = np.argwhere(R.border(P[b, c])), np.argwhere(R.border(G[b, c]))
                if not len(bp) or not len(bg):
                    assert (stats[b, c, 2:6] == -1).all()
                    continue
                d2 = ((bp[:, None] - bg[None]) ** 2).sum(2)
                for i, d in enumerate((sorted(d2.min(1).tolist()), sorted(d2.min(0).tolist()))):
                    k = (len(d) * permille + 999) // 1000
                    assert 1 <= k <= len(d) and stats[b, c, 4 + i] == d[k - 1]
                    if permille == 1000:
                        assert stats[b, c, 4 + i] == stats[b, c, 2 + i] == d[-1]
                    seen += 1
    assert seen >= 20


def test_hand_made_maps():
    t, p, C = R.special('pixels')                         # one pixel against one pixel at offset (3, 4)
    stats, sums = R.stats_brute(p, t, C)
    assert stats[0, 1].tolist() == [1, 1, 25, 25, 25, 25, 0, 0] and sums[0, 1].tolist() == [5.0, 5.0]
    assert R.stats_brute(p, t, C, tol=5)[0][0, 1, 6:].tolist() == [1, 1]
    acc = R.accumulate(np.zeros((7, C)), stats, sums)
    hd, hd95, assd, nsd, misses = R.metrics(acc)
    assert hd[1] == hd95[1] == assd[1] == 5.0 and nsd[1] == 0.0 and not misses.any()

    t, p, C = R.special('identical')
    stats, sums = R.stats_brute(p, t, C)
    assert (stats[..., 0] == stats[..., 1]).all() and (stats[..., 0] > 0).any()
    assert not stats[..., 2:6][stats[..., 0] > 0].any() and not sums.any()
    assert (stats[..., 6] == stats[..., 0]).all() and (stats[..., 7] == stats[..., 1]).all()
    nsd = R.metrics(R.accumulate(np.zeros((7, C)), stats, sums))[3]
    assert (nsd[~np.isnan(nsd)] == 1.0).all() and (~np.isnan(nsd)).any()

    t, p, C = R.special('full')                           # the target's class 1 fills the image: its border is the frame
    H, W = t.shape[1:]
    assert R.border(t[0] == 1).sum() == 2 * H + 2 * W - 4 and not R.border(t[0] == 1)[1:-1, 1:-1].any()
    stats, _ = R.stats_brute(p, t, C)
    assert stats[0, 1, 1] == 2 * H + 2 * W - 4 and stats[0, 1, 0] == 2 * H + 2 * W - 4 + 10      # the frame and the hole's rim
    assert stats[0, 0, 1] == 0 and (stats[0, 0, 2:6] == -1).all()

    t, p, C = R.special('checkerboard')                   # every pixel is a border pixel; the nearest of the other colour is 1 away
    stats, sums = R.stats_brute(p, t, C)
    n0, n1 = int((t == 0).sum()), int((t == 1).sum())
    assert stats[0, 0].tolist() == [n1, n0, 1, 1, 1, 1, n1, n0] and sums[0, 0].tolist() == [float(n1), float(n0)]

    t, p, C = R.special('one_map_only')
    stats, sums = R.stats_brute(p, t, C)
    assert stats[0, 1].tolist() == [0, 4, -1, -1, -1, -1, 0, 0] and stats[0, 2].tolist() == [6, 0, -1, -1, -1, -1, 0, 0]
    assert not sums[0, 1:].any() and R.kinds(stats)[0].tolist() == [3, 2, 1]
    hd, hd95, assd, nsd, misses = R.metrics(R.accumulate(np.zeros((7, C)), stats, sums))
    assert misses.tolist() == [0, 1, 1] and nsd[1:].tolist() == [0.0, 0.0] and np.isnan(hd[1:]).all() and not np.isnan(hd[0])

    t, p, C = R.special('all_void')
    stats, sums = R.stats_brute(p, t, C)
    assert not stats[..., :2].any() and (stats[..., 2:6] == -1).all() and not stats[..., 6:].any() and not sums.any()
    out = R.metrics(R.accumulate(np.zeros((7, C)), stats, sums))
    assert all(np.isnan(v).all() for v in out[:4]) and not out[4].any()
    for kind in R.SPECIAL:
        t, p, C = R.special(kind)
        a, b = R.stats_brute(p, t, C), R.stats_scipy(p, t, C)
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])


def test_void_rules():
    """a void target pixel is in neither mask, whatever the prediction says; a prediction out of range is in no mask"""
    t = np.zeros((1, 6, 6), dtype=np.int64)
    p = np.zeros((1, 6, 6), dtype=np.int64)
    t[0, 2, 2] = 255
    p[0, 2, 2] = 1                                        # predicted under a void target: not a pixel of class 1
    p[0, 4, 4] = 7                                        # out of range: a hole in class 0's prediction only
    P, G = R.masks(p, t, 2)
    assert not P[0, 1].any() and not P[0, 0, 2, 2] and not G[0, 0, 2, 2] and not P[0, 0, 4, 4] and G[0, 0, 4, 4]
    stats, _ = R.stats_brute(p, t, 2)
    assert stats[0, 1].tolist() == [0, 0, -1, -1, -1, -1, 0, 0]
    assert stats[0, 0, 1] == 20 + 4                       # the frame and the four neighbours of the void pixel
    assert stats[0, 0, 0] == stats[0, 0, 1] + 2           # the hole's neighbours; two of the four are on the frame already


def test_generated_cases_cover_every_kind_of_record():
    """a condition on the case list, shown by the reference alone: over the cases with C <= 5 at least half of the records are
    defined, and the list holds records of all four kinds"""
    small = np.concatenate([R.kinds(_case(s)[2][0]).reshape(-1) for s in R.SHAPES if s[1] <= 5])
    every = np.concatenate([R.kinds(_case(s)[2][0]).reshape(-1) for s in R.SHAPES])
    print('C <= 5: %d of %d records defined; kinds over all cases: %s' % ((small == 3).sum(), small.size,
                                                                           np.bincount(every, minlength=4).tolist()))
    assert 2 * (small == 3).sum() >= small.size
    assert (np.bincount(every, minlength=4) > 0).all()


# ------------------------------------------------------------------ header and library
def test_header_declares_the_entry_points():
    from pytorch_segmentation_amd import _lib
    protos = _lib.parse_header()
    assert _lib.abi_version_of_header() == 14
    assert protos['pseg_hausdorff_workspace_bytes'][2] == ['B', 'C', 'H', 'W']
    assert protos['pseg_hausdorff_workspace_bytes'][0] is ctypes.c_int64
    assert protos['pseg_hausdorff_stats'][2] == ['pred', 'target', 'B', 'H', 'W', 'C', 'permille', 'tol', 'stats', 'sums',
                                                 'workspace', 'workspace_bytes', 'stream']
    V, I = ctypes.c_void_p, ctypes.c_int
    assert protos['pseg_hausdorff_stats'][:2] == (I, [V, V, I, I, I, I, I, I, V, V, V, ctypes.c_int64, V])
    additive = open(_lib.HEADER_PATH).read().split('#define PSEG_ABI_VERSION')[0]
    assert 'pseg_hausdorff_workspace_bytes' in additive and 'pseg_hausdorff_stats' in additive
    # pseg_class_sdist is as it was
    assert protos['pseg_class_sdist'][2] == ['labels', 'B', 'H', 'W', 'C', 'sdist', 'workspace', 'workspace_bytes', 'stream']


@pytest.fixture(scope='module')
def lib():
    from pytorch_segmentation_amd import _lib
    from pytorch_segmentation_amd.csrc import build as csrc_build
    assert 'hausdorff.hip' in csrc_build.SOURCES
    csrc_build.build(verbose=False)
    _lib.load()
    return _lib


def test_library_exports_the_entry_points_and_sizes_the_workspace(lib):
    assert {'pseg_hausdorff_stats', 'pseg_hausdorff_workspace_bytes'} <= set(lib.prototypes())
    assert lib.load().pseg_abi_version() == 14
    # an int16 plane per class and map, and 12 bytes per pixel
    need = lib.query('pseg_hausdorff_workspace_bytes', 16, 21, 512, 512)
    px = 16 * 512 * 512
    assert px * (4 * 21 + 12) <= need <= px * (4 * 21 + 12) + (4 << 20)
    assert 0 < lib.query('pseg_hausdorff_workspace_bytes', 1, 1024, 4, 4) < (8 << 20)
    for refused in ((0, 2, 8, 8), (1, 0, 8, 8), (1, 1025, 8, 8), (1, 2, 16385, 8), (1, 2, 8, 16385), (1, 2, 0, 8), (1, 2, 8, 0),
                    (32, 21, 1024, 1024), (2, 1, 16384, 16384), (-1, 2, 8, 8), (1 << 11, 1 << 10, 1, 1)):
        assert lib.query('pseg_hausdorff_workspace_bytes', *refused) == 0, refused
    assert lib.query('pseg_hausdorff_workspace_bytes', 1, 1, 16384, 16384) > 0         # the largest side fits
    raw = lib.load()
    assert raw.pseg_hausdorff_stats(None, None, 0, 0, 0, 0, 0, 0, None, None, None, 0, None) == -1
    assert raw.pseg_last_error().startswith(b'pseg_hausdorff_stats:')


@pytest.mark.skipif(torch.cuda.is_available(), reason='uses made-up device addresses: host-side checks only')
def test_argument_refusals(lib):
    """Every refusal the header lists, by the host-side checks alone: the pointers are made-up addresses and nothing is
    dereferenced or launched."""
    A, A2, A3, A4, A5, MIS = 0x7f0000000000, 0x7f0000100000, 0x7f0000200000, 0x7f0000300000, 0x7f0000400000, 0x7f0000400008

    def stats(pred=A, target=A2, B=2, H=24, W=40, C=5, permille=950, tol=2, out=A3, sums=A4, ws=A5, nbytes=None):
        need = lib.query('pseg_hausdorff_workspace_bytes', B, C, H, W)
        lib.call('pseg_hausdorff_stats', pred, target, B, H, W, C, permille, tol, out, sums, ws, need if nbytes is None else nbytes,
                 None)

    def refused(match, **kw):
        with pytest.raises(lib.PsegError, match=r'\): pseg_hausdorff_stats: .*' + match):
            stats(**kw)

    for name in ('pred', 'target', 'out', 'sums', 'ws'):
        refused('null pointer', **{name: None})
    for name in ('B', 'H', 'W'):
        refused('must be >= 1', **{name: 0}, nbytes=1 << 30)
        refused('must be >= 1', **{name: -3}, nbytes=1 << 30)
    refused('H, W = 16385, 8', H=16385, W=8, nbytes=1 << 40)
    refused('H, W = 8, 16385', H=8, W=16385, nbytes=1 << 40)
    refused('class count C = 0', C=0, nbytes=1 << 30)
    refused('class count C = 1025', C=1025, nbytes=1 << 30)
    refused('above 2 GiB', B=32, C=21, H=1024, W=1024, nbytes=1 << 40)
    refused('above 2 GiB', B=1 << 11, C=1 << 10, H=1, W=1, nbytes=1 << 40)
    for bad in (0, -1, 1001):
        refused('permille = %d' % bad, permille=bad)
    for bad in (-1, 256):
        refused('tol = %d' % bad, tol=bad)
    refused('workspace too small', nbytes=lib.query('pseg_hausdorff_workspace_bytes', 2, 5, 24, 40) - 1)
    refused('workspace too small', nbytes=0)
    refused('16-byte aligned', ws=MIS)


# ------------------------------------------------------------------ host interface
def test_compute_surface_metrics_on_hand_written_accumulators():
    from pytorch_segmentation_amd import utils
    from pytorch_segmentation_amd.utils import compute_surface_metrics, loss, update_surface_stats
    assert utils.update_surface_stats is loss.update_surface_stats and utils.compute_surface_metrics is loss.compute_surface_metrics
    assert {'update_surface_stats', 'compute_surface_metrics'} <= set(utils.__all__)
    assert list(inspect.signature(update_surface_stats).parameters) == ['acc', 'predicted', 'targets', 'permille', 'tol']
    assert [p.default for p in inspect.signature(update_surface_stats).parameters.values()][3:] == [950, 2]
    #                     defined  sum HD  sum HD95  sum ASSD  with NSD  sum NSD  misses
    acc = torch.tensor([[4.0, 10.0, 8.0, 3.0, 5.0, 2.5, 1.0],           # four defined images and one miss
                        [0.0, 0.0, 0.0, 0.0, 2.0, 0.0, 2.0],            # two misses: an NSD of 0 and no distance
                        [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0],            # never seen
                        [1.0, math.sqrt(2.0), 1.0, 0.75, 1.0, 1.0, 0.0]], dtype=torch.float64).t().contiguous()
    hd, hd95, assd, nsd, misses = compute_surface_metrics(acc)
    for v in (hd, hd95, assd, nsd, misses):
        assert v.dtype == torch.float64 and v.shape == (4,) and v.device.type == 'cpu'
    assert hd[[0, 3]].tolist() == [2.5, math.sqrt(2.0)] and torch.isnan(hd[[1, 2]]).all()
    assert hd95[[0, 3]].tolist() == [2.0, 1.0] and torch.isnan(hd95[[1, 2]]).all()
    assert assd[[0, 3]].tolist() == [0.75, 0.75] and torch.isnan(assd[[1, 2]]).all()
    assert nsd[[0, 1, 3]].tolist() == [0.5, 0.0, 1.0] and torch.isnan(nsd[2])
    assert misses.tolist() == [1.0, 2.0, 0.0, 0.0]
    ref = R.metrics(acc.numpy())
    for got, want in zip((hd, hd95, assd, nsd, misses), ref):
        np.testing.assert_array_equal(got.numpy(), want)


def _cli():
    spec = importlib.util.spec_from_file_location('pseg_eval_cli_hausdorff_cpu', os.path.join(REPO, 'test.py'))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def test_evaluation_flags(capsys):
    cli = _cli()
    opt = cli.parse_args(['val.json'])
    assert (opt.surface_distance, opt.hd_percentile, opt.surface_tolerance) == (False, 95.0, 2)
    opt = cli.parse_args(['val.json', '--surface-distance'])
    assert (opt.surface_distance, opt.hd_percentile, opt.surface_tolerance) == (True, 95.0, 2)
    opt = cli.parse_args(['val.json', '--surface-distance', '--hd-percentile', '99.5', '--surface-tolerance', '0', '--boundary'])
    assert (opt.surface_distance, opt.hd_percentile, opt.surface_tolerance, opt.boundary) == (True, 99.5, 0, 0.02)
    assert cli.hd_permille(99.5) == 995 and cli.hd_permille(95) == 950 and cli.hd_permille(100) == 1000 and cli.hd_permille(0.1) == 1
    for bad in (['--hd-percentile', '90'], ['--surface-tolerance', '3'], ['--hd-percentile', '95', '--surface-tolerance', '2'],
                ['--surface-distance', '--hd-percentile', '95.25'], ['--surface-distance', '--hd-percentile', '0'],
                ['--surface-distance', '--hd-percentile', '100.1'], ['--surface-distance', '--surface-tolerance', '256'],
                ['--surface-distance', '--surface-tolerance', '-1'], ['--surface-distance', '--surface-tolerance', '1.5']):
        with pytest.raises(SystemExit):
            cli.parse_args(['val.json'] + bad)
    assert 'need --surface-distance' in capsys.readouterr().err
    names = list(inspect.signature(cli.test).parameters)
    assert names == ['model', 'fetcher', 'scales', 'flip', 'min_area', 'connectivity', 'largest_only', 'window', 'stride',
                     'boundary', 'boundary_width', 'results', 'crf', 'surface_distance', 'hd_percentile', 'surface_tolerance']
    assert [p.default for p in inspect.signature(cli.test).parameters.values()][-3:] == [False, 95.0, 2]
    for flag in ('--surface-distance', '--hd-percentile', '--surface-tolerance'):
        assert flag in cli.__doc__


def test_wrappers_refuse_cpu_tensors():
    from pytorch_segmentation_amd import ops
    from pytorch_segmentation_amd.utils import update_surface_stats
    t = torch.zeros(1, 4, 4, dtype=torch.int64)
    assert list(inspect.signature(ops.hausdorff_stats).parameters) == ['pred', 'target', 'num_classes', 'permille', 'tol']
    assert [p.default for p in inspect.signature(ops.hausdorff_stats).parameters.values()][3:] == [950, 2]
    with pytest.raises(RuntimeError, match='hausdorff_stats runs on the HIP path only'):
        ops.hausdorff_stats(t, t, 2)
    with pytest.raises(RuntimeError, match='HIP path only'):
        update_surface_stats(torch.zeros(7, 2, dtype=torch.float64), t, t)
