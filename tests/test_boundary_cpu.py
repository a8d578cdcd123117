"""Contour measures without a GPU: the numpy restatement (tests/boundary_ref.py) against the published algorithm and against
itself, the conditions of the cases the GPU test runs, the host helpers, the command line and the argument checks of the two
entry points."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import boundary_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cli():
    spec = importlib.util.spec_from_file_location('pseg_eval_cli_boundary', os.path.join(REPO, 'test.py'))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize('H,W,d', [(37, 53, 5), (3, 40, 5), (20, 20, 1)])
def test_band_is_the_published_erosion_band(H, W, d):
    """for every class c, M = (L == c): M & (depth_edge <= d) == M & ~erode^d(M), the boundary region of the Boundary IoU code"""
    C = 4
    L = R.make_target((1, H, W, C, d), seed=3)[0]
    assert ((L < 0) | (L >= C)).any()                   # void specks are part of the claim
    band = R.label_depth(L, d, edge=True) <= d
    for c in range(C):
        M = L == c
        assert M.any()
        np.testing.assert_array_equal(M & band, M & ~R.erode_reference(M, d))


@pytest.mark.parametrize('case', R.CASES, ids=R.case_id)
def test_depth_edge_is_depth_cut_by_the_edge_distance(case):
    B, H, W, C, d = case
    L = R.make_target(case)
    y, x = np.arange(H)[:, None], np.arange(W)[None, :]
    to_edge = np.minimum(np.minimum(x, W - 1 - x), np.minimum(y, H - 1 - y))
    np.testing.assert_array_equal(R.label_depth(L, d, edge=True), np.minimum(R.label_depth(L, d), to_edge + 1))


@pytest.mark.parametrize('case', R.CASES, ids=R.case_id)
def test_separable_recurrence_equals_the_windowed_definition(case):
    d = case[4]
    T = R.make_target(case)
    for L in (T, R.make_pred(case, T)):
        want = R.depth_windowed(L, d)
        assert want.min() >= 1 and want.max() <= d + 1
        np.testing.assert_array_equal(R.depth_separable(L, d), want)


def test_images_of_a_batch_are_separate():
    case = R.CASES[0]
    T = R.make_target(case)
    assert (T[0, -1] != T[1, 0]).any() and (T[1, -1] != T[2, 0]).any()          # neighbouring rows in memory differ
    whole = R.label_depth(T, case[4])
    for b in range(case[0]):
        np.testing.assert_array_equal(whole[b], R.depth_windowed(T[b], case[4]))


@pytest.mark.parametrize('case', R.CASES, ids=R.case_id)
def test_case_conditions(case):
    """What the generator promises for the cases test_boundary_gpu.py runs.  The RICH cases meet all four conditions.  The
    others are the degenerate shapes of the list, where some conditions cannot hold, for these reasons:
      - one pixel (1x1x1): a void pixel counts nowhere and a valid one has no neighbour, so the GPU test runs it once each way;
      - 3 x 40, 40 x 3 (thinner than d), 16 x 16 at d = 3 with specks, 24 x 24 with one class: too few pixels far from every
        contour and speck for 5 % at d + 1 or for every depth value; d = 254 on 40 x 300 has no pixel 254 away from anything.
    They still have a void pixel, both labels' contours, and -- where a second class exists -- a counted intersection."""
    B, H, W, C, d = case
    T = R.make_target(case)
    P = R.make_pred(case, T)
    void_t = (T < 0) | (T >= C)
    cnt = R.boundary_counts(P, T, C, d)
    if H * W > 1:
        assert void_t.any()
    if H * W >= 8:
        present = set(T[void_t].tolist())
        assert present == set(R.void_values(C))                                  # all four void values
        a, b = R.void_values(C)[0], R.void_values(C)[3]
        assert ((T[:, :, :-1] == a) & (T[:, :, 1:] == b)).any() or ((T[:, :-1] == a) & (T[:, 1:] == b)).any()
        assert ((P < 0) | (P >= C))[~void_t].any()                               # a prediction outside [0, C) on a valid target
        assert cnt[1].any() and cnt[2].any() and cnt[3].any()
    if case in R.RICH:
        Pp = np.where(void_t, R.VOID, P)
        for L in (T, Pp):
            dep = R.label_depth(L, d)
            assert set(np.unique(dep).tolist()) == set(range(1, d + 2))
            assert (dep == d + 1).mean() >= 0.05
        assert all(cnt[r].any() for r in range(6))
        assert (0 < cnt[0].sum() < cnt[1].sum())                                 # contours near but not on the target's


def test_counts_against_the_definition_spelled_out():
    """boundary_counts against per-class loops over the erosion bands (Boundary IoU) and over the trimap"""
    case = R.CASES[0]
    B, H, W, C, d = case
    T = R.make_target(case)
    P = R.make_pred(case, T)
    valid = (T >= 0) & (T < C)
    Pp = np.where(valid, P, R.VOID)
    want = np.zeros((6, C), dtype=np.int64)
    for b in range(B):
        near = R.depth_windowed(T[b], d) <= d
        for c in range(C):
            G, Q = T[b] == c, Pp[b] == c
            gb, qb = G & ~R.erode_reference(G, d), Q & ~R.erode_reference(Q, d)
            want[0, c] += (gb & qb).sum()
            want[1, c] += gb.sum()
            want[2, c] += qb.sum()
            want[3, c] += (near & G & (P[b] == c)).sum()
            want[4, c] += (near & G & (P[b] != c)).sum()
            want[5, c] += (near & valid[b] & ~G & (P[b] == c)).sum()
    np.testing.assert_array_equal(R.boundary_counts(P, T, C, d), want)


# ------------------------------------------------------------------ host helpers
def test_boundary_width():
    from pytorch_segmentation_amd.utils import boundary_width
    assert boundary_width((512, 512)) == 14 == R.width((512, 512))               # 14.48
    assert boundary_width((1024, 2048)) == 46                                    # 45.79
    assert boundary_width((3, 4), 0.1) == 1 and boundary_width((3, 4), 0.3) == 2     # 0.5 rounds up to 1, 1.5 up to 2
    assert boundary_width((30, 40), 0.05) == 3                                   # 2.5 rounds up
    assert boundary_width((30, 40), 0.0499) == 2
    assert boundary_width((1, 1)) == 1                                           # never below one pixel
    assert boundary_width((6000, 8000), 0.0254) == 254
    with pytest.raises(ValueError, match='exceeds 254'):
        boundary_width((6000, 8000), 0.0255)
    for ratio in (0.0, -0.1, 0.51):
        with pytest.raises(ValueError, match='ratio'):
            boundary_width((64, 64), ratio)
    from utils.utils import boundary_width as shim, compute_boundary_metrics, update_boundary_counts     # noqa: F401
    assert shim is boundary_width


def test_compute_boundary_metrics_with_zero_denominators():
    from pytorch_segmentation_amd.utils import compute_boundary_metrics
    cnt = torch.tensor([[3, 0, 0], [4, 0, 5], [5, 0, 0], [7, 0, 0], [1, 0, 2], [2, 0, 0]])
    biou, tiou = compute_boundary_metrics(cnt)
    assert biou.dtype == torch.float32 and biou.tolist() == [0.5, 0.0, 0.0]      # 3 / (4 + 5 - 3); 0 / 1; 0 / 5
    assert torch.equal(tiou, torch.tensor([7.0, 0.0, 0.0]) / torch.tensor([10.0, 1.0, 2.0]))
    rb, rt = R.metrics(cnt.numpy())
    np.testing.assert_array_equal(biou.numpy(), rb)
    np.testing.assert_array_equal(tiou.numpy(), rt)
    assert torch.equal(cnt, torch.tensor([[3, 0, 0], [4, 0, 5], [5, 0, 0], [7, 0, 0], [1, 0, 2], [2, 0, 0]]))    # not modified


def test_update_boundary_counts_checks_the_width_on_the_host():
    from pytorch_segmentation_amd.utils import update_boundary_counts
    z = torch.zeros(1, 4, 4, dtype=torch.int64)
    for w in (0, 255):
        with pytest.raises(ValueError, match='width'):
            update_boundary_counts(torch.zeros(6, 2, dtype=torch.int64), z, z, w)


# ------------------------------------------------------------------ command line
def test_evaluation_cli_parser(capsys):
    cli = _cli()
    opt = cli.parse_args(['val.json'])
    assert opt.boundary is None and opt.boundary_width is None
    assert cli.parse_args(['val.json', '--boundary']).boundary == 0.02
    assert cli.parse_args(['--boundary', '0.05', 'val.json']).boundary == 0.05
    assert cli.parse_args(['val.json', '--boundary', '0.5']).boundary == 0.5
    opt = cli.parse_args(['val.json', '--boundary-width', '3'])
    assert opt.boundary_width == 3 and opt.boundary is None
    for bad, msg in ((['--boundary', '0.02', '--boundary-width', '3'], 'not allowed with'),
                     (['--boundary', '0'], '--boundary must be in'), (['--boundary', '0.6'], '--boundary must be in'),
                     (['--boundary-width', '0'], '--boundary-width must be in'),
                     (['--boundary-width', '255'], '--boundary-width must be in')):
        with pytest.raises(SystemExit):
            cli.parse_args(['val.json'] + bad)
        assert msg in capsys.readouterr().err


def test_evaluation_refuses_both_keywords():
    cli = _cli()
    model = torch.nn.Identity()
    with pytest.raises(ValueError, match='exclude each other'):
        cli.test(model, None, boundary=0.02, boundary_width=3)
    with pytest.raises(ValueError, match='boundary must be in'):
        cli.test(model, None, boundary=0.7)
    with pytest.raises(ValueError, match='boundary_width must be in'):
        cli.test(model, None, boundary_width=255)


# ------------------------------------------------------------------ the entry points' argument checks
@pytest.mark.skipif(torch.cuda.is_available(), reason='uses made-up device addresses: host-side checks only')
def test_entry_points_refuse_bad_arguments():
    from pytorch_segmentation_amd import _lib
    from pytorch_segmentation_amd.csrc import build as csrc_build
    csrc_build.build(verbose=False)
    A = 0x7f0000000000                                  # a made-up aligned address: every case is refused before any launch

    def refused(name, *args, match):
        with pytest.raises(_lib.PsegError, match=match):
            _lib.call(name, *args)

    depth = lambda B, H, W, C, d: ('pseg_label_depth', A, B, H, W, C, d, 0, A, None)
    need = _lib.query('pseg_boundary_counts_workspace_bytes', 2, 8, 8, 3)
    assert need == 2 * 128
    counts = lambda B, H, W, C, d, ws=need: ('pseg_boundary_counts', A, A, B, H, W, C, d, A, A, ws, None)
    for call in (depth, counts):
        fn = 'label_depth' if call is depth else 'boundary_counts'
        refused(*call(2, 8, 8, 0, 3), match=fn + '.*class count C = 0')
        refused(*call(2, 8, 8, 1025, 3), match=fn + '.*class count C = 1025')
        refused(*call(2, 8, 8, 4, 0), match=fn + '.*width d = 0')
        refused(*call(2, 8, 8, 4, 255), match=fn + '.*width d = 255')
        refused(*call(0, 8, 8, 4, 3), match=fn + '.*sizes B, H, W')
        refused(*call(2, 8, 0, 4, 3), match=fn + '.*sizes B, H, W')
        refused(*call(1 << 20, 1 << 20, 1 << 20, 4, 3), match=fn + '.*exceeds 2\\^40')
    refused(*counts(2, 8, 8, 4, 3, need - 1), match='boundary_counts: workspace too small')
    refused('pseg_label_depth', None, 2, 8, 8, 4, 3, 0, A, None, match='label_depth: null pointer')
    refused('pseg_boundary_counts', A, A, 2, 8, 8, 4, 3, A, None, need, None, match='boundary_counts: null pointer')
    assert _lib.query('pseg_boundary_counts_workspace_bytes', 2, 8, 8, 255) == -1
    assert _lib.query('pseg_boundary_counts_workspace_bytes', 0, 8, 8, 3) == -1
    assert _lib.query('pseg_boundary_counts_workspace_bytes', 1, 3, 5, 1) == 32
