"""The integer-only planning queries of the conv entry points over a grid of conv problems (shared by tests/test_plan_cpu.py and
tools/plan_table.py).  A problem is (B, H, W, Cin, Cout, k, stride, pad, dil): a square k x k conv on a B x H x W x Cin input."""


def _up(c, m):
    return (c + m - 1) // m * m


def answers(lib, prob):
    """-> the answers of every query for one problem, in a fixed order (see NAMES)."""
    B, H, W, Cin, Cout, k, s, p, d = prob
    Ho, Wo = (H + 2 * p - d * (k - 1) - 1) // s + 1, (W + 2 * p - d * (k - 1) - 1) // s + 1
    ci, co = _up(Cin, 4), _up(Cout, 4)          # the fp32 kernels take channels in fours, the fp16 ones in eights
    ci8, co8 = _up(Cin, 8), _up(Cout, 8)
    fwd, fwd8 = (B, Ho, Wo, ci, co, k, k, s, p, d), (B, Ho, Wo, ci8, co8, k, k, s, p, d)
    dg, dg8 = (B, H, W, ci, Ho, Wo, co, k, k, s, p, d), (B, H, W, ci8, Ho, Wo, co8, k, k, s, p, d)
    out = [lib.pseg_conv2d_stat_rows(*fwd), lib.pseg_conv2d_stat_group(*fwd),
           lib.pseg_conv2d_fwd_workspace_bytes(B, Ho, Wo, ci, co, k, k),
           lib.pseg_conv2d_fwd_workspace_bytes(B, H, W, co, ci, k, k),      # (as the data gradient asks)
           lib.pseg_conv2d_dgrad_bnstat_rows(*dg), lib.pseg_conv2d_dgrad_planes_ok(*dg),
           lib.pseg_conv2d_wgrad_workspace_bytes(B, Ho, Wo, ci, co, k, k)]
    out += [lib.pseg_conv2d_wgrad_splits(B, Ho, Wo, ci, co, k, k, prec, conc) for prec in (0, 1, 2) for conc in (0, 1)]
    out += [lib.pseg_conv2d_stat_rows_h(*fwd8), lib.pseg_conv2d_stat_group_h(*fwd8), lib.pseg_conv2d_dgrad_bnstat_rows_h(*dg8),
            lib.pseg_conv2d_wgrad_workspace_bytes_h(B, Ho, Wo, ci8, co8, k, k), lib.pseg_conv2d_wgrad_splits_h(B, Ho, Wo, ci8, co8, k, k)]
    return out


NAMES = (['stat_rows', 'stat_group', 'fwd_workspace_bytes', 'fwd_workspace_bytes(dgrad)', 'dgrad_bnstat_rows', 'dgrad_planes_ok',
          'wgrad_workspace_bytes'] + ['wgrad_splits(prec %d, concurrent %d)' % (p, c) for p in (0, 1, 2) for c in (0, 1)] +
         ['stat_rows_h', 'stat_group_h', 'dgrad_bnstat_rows_h', 'wgrad_workspace_bytes_h', 'wgrad_splits_h'])


def model_convs():
    """(Cin, Cout, k, stride, pad, dil) of every dense conv of the three models, 21 classes."""
    import warnings
    from pytorch_segmentation_amd import models
    from pytorch_segmentation_amd.nn import Conv2d
    convs = set()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for make in (models.DeepLabV3Plus, models.UNet, models.HRNet):
            for m in make(21).modules():
                if isinstance(m, Conv2d) and m.groups == 1 and m.kernel_size[0] == m.kernel_size[1]:
                    convs.add((m.in_channels, m.out_channels, m.kernel_size[0], m.stride[0], m.padding[0], m.dilation[0]))
    return sorted(convs)


def grid():
    """Every conv of DeepLabV3+, UNet and HRNet at every map size a 512 x 512 input passes through and batch 1 / 2 / 16, and a
    synthetic grid: 1x1 / 3x3 / 7x7 (49 taps: above the 32 of the tap masks), strides 1 / 2, dilations 1 / 2 / 6 / 12 / 18, channel
    counts on and off the 32-grid, even and odd maps."""
    probs, convs = [], model_convs()
    for B in (1, 2, 16):
        for (ci, co, k, s, p, d) in convs:
            for H in (512, 256, 128, 64, 32, 16):
                if H + 2 * p >= d * (k - 1) + 1:
                    probs.append((B, H, H, ci, co, k, s, p, d))
        chans = (3, 21, 24, 32, 48, 64, 96, 144, 256, 2048)
        shapes = [(1, 1, 1), (1, 2, 1), (7, 1, 1), (7, 2, 1), (3, 2, 1), (3, 2, 2)] + [(3, 1, d) for d in (1, 2, 6, 12, 18)]
        for H in (16, 32, 33, 64, 65, 128):
            for ci in chans:
                for co in chans:
                    for (k, s, d) in shapes:
                        probs.append((B, H, H, ci, co, k, s, d * (k - 1) // 2, d))
    return probs


def pinned(step=97):
    """A few hundred problems of the grid: every `step`-th, and the convs around DeepLabV3+'s ASPP at the bench size by name."""
    named = [(16, 32, 32, 2048, 256, 3, 1, d, d) for d in (6, 12, 18)] + \
            [(16, 32, 32, 2048, 256, 1, 1, 0, 1), (16, 128, 128, 384, 21, 3, 1, 1, 1), (16, 512, 512, 3, 64, 7, 2, 3, 1),
             (16, 128, 128, 64, 64, 3, 1, 1, 1), (16, 64, 64, 512, 128, 3, 2, 1, 1), (2, 65, 65, 256, 256, 3, 1, 12, 12)]
    return named + grid()[::step]

