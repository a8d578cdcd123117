"""The case tables of the weight-gradient instantiation tests (shared by tests/test_wgrad_instances_cpu.py, which proves through
the pure queries pseg_conv2d_wgrad_choice(_h) that every row reaches the launch it claims, and tests/test_wgrad_instances_gpu.py,
which runs every row against fp64).

A row is (id, fmt, case, env, record, flags):
  fmt     'h' (fp16 operands, wgrad_h_kernel) or 'f' (exact fp32: wgrad_f32_dma_kernel and, two rows, wgrad_kernel)
  case    (B, Cin, H, W, Cout, k, stride, pad, dil), a square k x k conv; channel counts as the model has them (the kernels see
          them padded to 8 -- fp16 -- or 4)
  env     the planning switches of the row (PSEG_HWGRAD_BKP, PSEG_WGRAD_SPLITS, PSEG_CONV_NOSKIP, PSEG_WGRAD_F32DMA,
          PSEG_WGRAD_HALO and nothing else)
  record  what pseg_debug_last_wgrad / pseg_conv2d_wgrad_choice(_h) must answer (pseg_amd.h): kernel code, tile rows, tile columns,
          pixels per K-step, SKIP flag, pixel order, patch_mode, patch rows, patch columns, pixel splits, pixels per split
  flags   'deferred': the split plan is also run through a SlabPool; 'centre_only': every tap but the centre one is padding

The expectations are written from the selection's rules (pick_tile, plan_wgrad, wgrad_pixel_order, select_wgrad(_h)), not read
back from the library: the tile from (Cout, K), the patch shape from the map (dense: the widest of 1x32 / 2x16 / 4x8 that tiles
it, else row-major; dilated at unit stride: the shape with the fewest live (patch, tap) pairs), one split for maps of fewer than
16 K-steps unless PSEG_WGRAD_SPLITS forces more."""
import collections

Row = collections.namedtuple('Row', 'id fmt case env record flags')

WGRAD_REGISTER, WGRAD_LIMB, WGRAD_DMA, WGRAD_HALO, WGRAD_H = 11, 12, 13, 14, 23      # PSEG_KERNEL_WGRAD_*
DENSE, SKIP_ROWS, SKIP_PATCHES, PACKED, ROW_MAJOR_DMA = 0, 1, 2, 3, 4                # kWgDense .. kWgRowMajorDma
SWITCHES = ('PSEG_HWGRAD_BKP', 'PSEG_WGRAD_SPLITS', 'PSEG_CONV_NOSKIP', 'PSEG_WGRAD_F32DMA', 'PSEG_WGRAD_HALO')
FIELDS = ('kernel', 'tile rows', 'tile columns', 'pixels per K-step', 'SKIP', 'pixel order', 'patch_mode', 'patch_h', 'patch_w',
          'splits', 'pix_per_split')
ROW_MAJOR = (0, 1, 32)                 # (patch_mode, patch_h, patch_w) of a map that does not tile into 32-pixel patches


def out_size(n, k, stride, pad, dil):
    return (n + 2 * pad - dil * (k - 1) - 1) // stride + 1


def geometry(case, fmt):
    """-> (B, H, W, Cin, Ho, Wo, Cout, kh, kw, stride, pad, dil) with the channel counts padded as the kernels take them"""
    B, Cin, H, W, Cout, k, stride, pad, dil = case
    q = 8 if fmt == 'h' else 4
    up = lambda c: (c + q - 1) // q * q
    return B, H, W, up(Cin), out_size(H, k, stride, pad, dil), out_size(W, k, stride, pad, dil), up(Cout), k, k, stride, pad, dil


def pixels(case):
    B, Cin, H, W, Cout, k, stride, pad, dil = case
    return B * out_size(H, k, stride, pad, dil) * out_size(W, k, stride, pad, dil)


def one_split(case):
    """(splits, pix_per_split) of a plan that does not split: the pixels rounded up to whole 32-pixel K-steps"""
    return 1, (pixels(case) + 31) // 32 * 32


def forced_splits(case, n):
    """... and under PSEG_WGRAD_SPLITS=n (plan_wgrad): ceil(K-steps / n) K-steps per split, as many splits as that leaves"""
    steps = (pixels(case) + 31) // 32
    per = -(-steps // min(n, steps)) * 32
    return -(-pixels(case) // per), per


def record(kernel, tile, kstep, skip, mode, patch, split):
    return (kernel, tile[0], tile[1], kstep, int(skip), mode) + tuple(patch) + tuple(split)


def choice(lib, row):
    """the record of the launch that WOULD run for a row (its switches must be set): the pure query"""
    import ctypes
    out = (ctypes.c_int * 11)()
    g = geometry(row.case, row.fmt)
    rc = lib.pseg_conv2d_wgrad_choice_h(*g, out) if row.fmt == 'h' else lib.pseg_conv2d_wgrad_choice(*g, 0, 0, out)
    assert rc == 0, lib.pseg_last_error()
    return tuple(out)


def describe(rec):
    return ', '.join('%s %d' % (n, v) for n, v in zip(FIELDS, rec))


BKPS = (32, 64)

# ------------------------------------------------------------------------------------------------ fp16: the dense grid
# One problem per tile of kHWgradTiles (Cin, Cout, k); pick_tile(Cout, K): rows 128 / 64 / 32 for Cout > 64 / > 32 / <= 32, columns
# 128 / 64 / 32 for K > 64 / > 32 / <= 32.
#   136 filters: two row tiles, the second with 8 live rows; K = 288: three column tiles, the last 32 columns wide
#   128x32 at 32 pixels per K-step: fewer DMA pieces (2) than waves for the x operand; 32x128 has that on the dy side
H_TILE_PROBLEMS = [((128, 128), (32, 136, 3)), ((64, 128), (32, 40, 3)), ((32, 128), (32, 24, 3)), ((128, 64), (48, 136, 1)),
                   ((128, 32), (24, 136, 1))]
# name, B, H, W, (patch_mode, patch_h, patch_w)
H_MAPS = [('8x8', 1, 8, 8, (1, 4, 8)),           # 4x8 patches, two sub-steps
          ('16x16', 1, 16, 16, (1, 2, 16)),
          ('8x32', 1, 8, 32, (1, 1, 32)),
          ('7x9', 1, 7, 9, ROW_MAJOR),           # 63 pixels: row-major, ragged last sub-step
          ('5x5', 1, 5, 5, ROW_MAJOR),           # 25 pixels: one partial sub-step (the second half of a 64-pixel K-step: the zero dummy)
          ('3of4x8', 3, 4, 8, (1, 4, 8))]        # three sub-steps: an odd count at 64 pixels per K-step
PATCH_MAP, ROW_MAJOR_MAP = H_MAPS[0], H_MAPS[3]


def _tile_case(problem, B, H, W):
    Cin, Cout, k = problem
    return (B, Cin, H, W, Cout, k, 1, k // 2, 1)


H_DENSE = []
for _tile, _prob in H_TILE_PROBLEMS:
    for _name, _B, _H, _W, _patch in H_MAPS:
        for _bkp in BKPS:
            _case = _tile_case(_prob, _B, _H, _W)
            H_DENSE.append(Row('h-%dx%d-%s-bkp%d' % (_tile + (_name, _bkp)), 'h', _case, {'PSEG_HWGRAD_BKP': _bkp},
                               record(WGRAD_H, _tile, _bkp, False, DENSE, _patch, one_split(_case)), ()))
# the stem: 3 -> 8 padded input channels, 7x7 stride 2, 20 -> 24 filters; K = 392: column tiles that straddle taps; 15 x 15 pixels
STEM = (1, 3, 30, 30, 20, 7, 2, 3, 1)
for _bkp in BKPS:
    H_DENSE.append(Row('h-stem-bkp%d' % _bkp, 'h', STEM, {'PSEG_HWGRAD_BKP': _bkp},
                       record(WGRAD_H, (32, 128), _bkp, False, DENSE, ROW_MAJOR, one_split(STEM)), ()))

# ------------------------------------------------------------------------------------------------ fp16: skipping
# 128 input channels, 3x3, dilation >= 4: a 128-column tile is one tap, the dead-step test is block-uniform.
# (name, geometry without the filter count, pixel order, patch, (splits, pix_per_split) or None for one split, flags)
#   rate 6 on 16 x 16: no 1x32 patch (32 > 16 columns); 2x16 -> rows: 8 patches x 3 taps at offsets -6 / 0 / +6, (5 + 8 + 5) / 24
#     live, columns: one patch, 3 / 3 -> 0.75; 4x8 -> rows (3 + 4 + 3) / 12, columns (2 + 2 + 2) / 6 -> 0.83: 2x16
#   rate 12 on 24 x 24: neither 32 nor 16 columns tile 24: 4x8.  1152 pixels = 36 K-steps: a split holds eight or more, so up to
#     four, and pick_splits takes every split a launch this far from filling the chip can get: 4 x 288 pixels
#   rate 6 on 13 x 13: 169 pixels, no patches: row-major with dead image rows skipped
#   rate 18 on 16 x 16: 2x16 and 4x8 tie at 1 / 9 live, the wider one (tried first) stays; only the centre tap has a live pixel
#   stride 2, rate 4, 32 x 32 -> 16 x 16 outputs: live_fraction is for unit stride only, so the widest patch that tiles the map
#   rate 12 on 16 x 16: 2x16 -> rows (2 + 8 + 2) / 24, columns 3 / 3 -> 0.5; 4x8 -> rows (1 + 4 + 1) / 12, columns (1 + 2 + 1) / 6 -> 0.33:
#     4x8, two patches per patch row of which a side tap has ONE live -- its live sub-steps are 1, 3, 5, 7 or 0, 2, 4, 6: at 64
#     pixels per K-step every K-step is fed from two live sub-steps that are NOT neighbours.  (In every other geometry here the dead
#     sub-steps of a tap lie in front of, behind or between whole PAIRS of live ones, so that the second sub-step of a K-step is
#     always the one after the first: a kernel that took "first + 32" for it passes them all, and fails this one.)
H_SKIP_GEOMETRIES = [('rate6-16x16', (1, 128, 16, 16, None, 3, 1, 6, 6), SKIP_PATCHES, (1, 2, 16), None, ()),
                     ('rate12-16x16', (1, 128, 16, 16, None, 3, 1, 12, 12), SKIP_PATCHES, (1, 4, 8), None, ()),
                     ('rate12-2of24x24', (2, 128, 24, 24, None, 3, 1, 12, 12), SKIP_PATCHES, (1, 4, 8), (4, 288), ()),
                     ('rate6-13x13', (1, 128, 13, 13, None, 3, 1, 6, 6), SKIP_ROWS, ROW_MAJOR, None, ()),
                     ('rate18-16x16', (1, 128, 16, 16, None, 3, 1, 18, 18), SKIP_PATCHES, (1, 2, 16), None, ('centre_only',)),
                     ('stride2-rate4-32x32', (1, 128, 32, 32, None, 3, 2, 4, 4), SKIP_PATCHES, (1, 2, 16), None, ())]
H_SKIP_TILES = [((128, 128), 136), ((64, 128), 40), ((32, 128), 24)]


def _with_cout(case, cout):
    return case[:4] + (cout,) + case[5:]


H_SKIP = []
for _name, _geom, _mode, _patch, _split, _flags in H_SKIP_GEOMETRIES:
    for _tile, _cout in H_SKIP_TILES:
        for _bkp in BKPS:
            _case = _with_cout(_geom, _cout)
            H_SKIP.append(Row('h-%dx%d-%s-bkp%d' % (_tile + (_name, _bkp)), 'h', _case, {'PSEG_HWGRAD_BKP': _bkp},
                              record(WGRAD_H, _tile, _bkp, True, _mode, _patch, _split or one_split(_case)), _flags))
# the first geometry with PSEG_CONV_NOSKIP=1: no skipping and no patch order either -- dense, row-major
for _tile, _cout in H_SKIP_TILES:
    for _bkp in BKPS:
        _case = _with_cout(H_SKIP_GEOMETRIES[0][1], _cout)
        H_SKIP.append(Row('h-%dx%d-rate6-16x16-noskip-bkp%d' % (_tile + (_bkp,)), 'h', _case, {'PSEG_HWGRAD_BKP': _bkp, 'PSEG_CONV_NOSKIP': 1},
                          record(WGRAD_H, _tile, _bkp, False, DENSE, ROW_MAJOR, one_split(_case)), ()))

# ------------------------------------------------------------------------------------------------ fp16: splits, slabs, the XCD remap
# Five images of 4 x 8 (160 pixels, five K-steps of 32; one 4x8 patch per image), 136 filters (two row tiles):
#   PSEG_WGRAD_SPLITS=3 -> 64 + 64 + 32 pixels: the last split holds one sub-step
#   PSEG_WGRAD_SPLITS=2 -> 96 + 64: at 64 pixels per K-step a split ends, and the next begins, in the middle of a K-step
# dense (32 channels, K = 288: 6 tiles -> 18 / 12 blocks: wgrad_block remaps the first 16 / 8 and leaves a tail of 2 / 4) and at rate
# 6 (128 channels: on a 4 x 8 map the taps of the upper and the lower filter row have no live pixel at all -- every K-step of every
# split of theirs is dead, the blocks store zeros -- and the middle row's side taps two live columns)
H_SPLIT_PROBLEMS = [('dense', (5, 32, 4, 8, 136, 3, 1, 1, 1), False, DENSE), ('rate6', (5, 128, 4, 8, 136, 3, 1, 6, 6), True, SKIP_PATCHES)]
H_SPLIT = []
for _name, _case, _skip, _mode in H_SPLIT_PROBLEMS:
    for _n in (3, 2):
        for _bkp in BKPS:
            H_SPLIT.append(Row('h-%s-5of4x8-splits%d-bkp%d' % (_name, _n, _bkp), 'h', _case, {'PSEG_HWGRAD_BKP': _bkp, 'PSEG_WGRAD_SPLITS': _n},
                               record(WGRAD_H, (128, 128), _bkp, _skip, _mode, (1, 4, 8), forced_splits(_case, _n)), ('deferred',)))
# 56 channels, K = 504: 2 x 4 tiles x 2 splits = 16 blocks, all of them remapped (no tail)
REMAP16 = (5, 56, 4, 8, 136, 3, 1, 1, 1)
for _bkp in BKPS:
    H_SPLIT.append(Row('h-dense-16-blocks-bkp%d' % _bkp, 'h', REMAP16, {'PSEG_HWGRAD_BKP': _bkp, 'PSEG_WGRAD_SPLITS': 2},
                       record(WGRAD_H, (128, 128), _bkp, False, DENSE, (1, 4, 8), forced_splits(REMAP16, 2)), ('deferred',)))
# (blocks of a row's launch: row tiles x column tiles x splits)
BLOCKS = {'h-dense-5of4x8-splits3-bkp32': 18, 'h-dense-5of4x8-splits3-bkp64': 18, 'h-dense-16-blocks-bkp32': 16,
          'h-dense-16-blocks-bkp64': 16}

# ------------------------------------------------------------------------------------------------ fp16: sliced operands
# every tile problem on one patch-order and one row-major map; (tile, case, patch)
H_SLICED = [(_tile, _tile_case(_prob, _m[1], _m[2], _m[3]), _m[4]) for _tile, _prob in H_TILE_PROBLEMS for _m in (PATCH_MAP, ROW_MAJOR_MAP)]

H_ROWS = H_DENSE + H_SKIP + H_SPLIT

# ------------------------------------------------------------------------------------------------ exact fp32
# wgrad_f32_dma_kernel: kWgradDmaTiles x skip, and its pixel orders -- dense patches, row-major (a map without 32-pixel patches: every
# lane derives its pixel), packed live rectangles (dilated, unit stride, patches), dead patches skipped (dilated, strided).  Tiles as
# pick_tile says, but 32 rows: 256 columns where they pad K by at most 5 % more than 128 (K = 504 = 9 x 56, K = 2304), and K = 288
# as one 32 x 288 tile.  PSEG_WGRAD_HALO=0 on the one row the halo kernel would otherwise take.
#   (id, case, env, kernel, tile, skip, order, patch)
_F = [('f-128x128-dense', (1, 32, 8, 8, 136, 3, 1, 1, 1), {}, WGRAD_DMA, (128, 128), False, DENSE, (1, 4, 8)),
      ('f-128x128-packed', (1, 128, 16, 16, 136, 3, 1, 6, 6), {}, WGRAD_DMA, (128, 128), True, PACKED, (1, 2, 16)),
      ('f-128x128-stride2-rate4', (1, 128, 32, 32, 136, 3, 2, 4, 4), {}, WGRAD_DMA, (128, 128), True, SKIP_PATCHES, (1, 2, 16)),
      ('f-128x128-row-major', (1, 32, 7, 9, 136, 3, 1, 1, 1), {}, WGRAD_DMA, (128, 128), False, ROW_MAJOR_DMA, ROW_MAJOR),
      ('f-128x64-dense', (1, 48, 8, 8, 136, 1, 1, 0, 1), {}, WGRAD_DMA, (128, 64), False, DENSE, (1, 4, 8)),
      ('f-128x64-row-major', (1, 48, 7, 9, 136, 1, 1, 0, 1), {}, WGRAD_DMA, (128, 64), False, ROW_MAJOR_DMA, ROW_MAJOR),
      ('f-64x128-dense', (1, 32, 8, 8, 40, 3, 1, 1, 1), {}, WGRAD_DMA, (64, 128), False, DENSE, (1, 4, 8)),
      ('f-64x128-packed', (1, 128, 16, 16, 40, 3, 1, 6, 6), {}, WGRAD_DMA, (64, 128), True, PACKED, (1, 2, 16)),
      ('f-64x128-row-major', (1, 32, 7, 9, 40, 3, 1, 1, 1), {}, WGRAD_DMA, (64, 128), False, ROW_MAJOR_DMA, ROW_MAJOR),
      ('f-32x256-dense', (1, 56, 8, 8, 24, 3, 1, 1, 1), {}, WGRAD_DMA, (32, 256), False, DENSE, (1, 4, 8)),
      ('f-32x256-packed', (1, 256, 16, 16, 24, 3, 1, 6, 6), {}, WGRAD_DMA, (32, 256), True, PACKED, (1, 2, 16)),
      ('f-32x256-row-major', (1, 56, 7, 9, 24, 3, 1, 1, 1), {}, WGRAD_DMA, (32, 256), False, ROW_MAJOR_DMA, ROW_MAJOR),
      ('f-32x288-dense', (1, 32, 8, 8, 24, 3, 1, 1, 1), {}, WGRAD_DMA, (32, 288), False, DENSE, (1, 4, 8)),
      ('f-32x288-row-major', (1, 32, 7, 9, 24, 3, 1, 1, 1), {}, WGRAD_DMA, (32, 288), False, ROW_MAJOR_DMA, ROW_MAJOR),
      ('f-32x288-16x16-no-halo', (1, 32, 16, 16, 24, 3, 1, 1, 1), {'PSEG_WGRAD_HALO': 0}, WGRAD_DMA, (32, 288), False, DENSE, (1, 2, 16)),
      # the register-staged kernel runs the shared orders as wgrad_pixel_order gives them: dead rows / dead patches skipped
      ('f-register-skip-rows', (1, 128, 13, 13, 136, 3, 1, 6, 6), {'PSEG_WGRAD_F32DMA': 0}, WGRAD_REGISTER, (128, 128), True, SKIP_ROWS, ROW_MAJOR),
      ('f-register-skip-patches', (1, 128, 16, 16, 136, 3, 1, 6, 6), {'PSEG_WGRAD_F32DMA': 0}, WGRAD_REGISTER, (128, 128), True, SKIP_PATCHES, (1, 2, 16))]
F_ROWS = [Row(_id, 'f', _case, _env, record(_kernel, _tile, 32, _skip, _mode, _patch, one_split(_case)), ())
          for _id, _case, _env, _kernel, _tile, _skip, _mode, _patch in _F]

# tests/test_ops_gpu.py::WGRAD_FAMILY_CASES by id: (tile, SKIP, pixel order) of the launch beside its kernel code.  With
# PSEG_CONV_NOSKIP=1 the dilated problem loses the patch order with the skipping and runs row-major on the LDS-DMA kernel.
FAMILY_RECORDS = {
    'patch_order_dma': ((64, 128), 0, DENSE), 'row_major_dma': ((64, 128), 0, ROW_MAJOR_DMA), 'packed_dilated': ((64, 128), 1, PACKED),
    'packed_dilated_noskip': ((64, 128), 0, ROW_MAJOR_DMA), 'tile_32x288': ((32, 288), 0, DENSE), 'halo': ((32, 288), 0, DENSE),
    'register_32_to_21': ((32, 128), 0, DENSE), 'register_32x256': ((32, 256), 0, DENSE), 'limb_bf16x3': ((64, 128), 0, DENSE),
    'limb_bf16x6': ((64, 128), 0, DENSE), 'forced_split_2x8x8': ((64, 128), 0, DENSE), 'forced_split_3x8x8': ((64, 128), 0, DENSE),
}

# ------------------------------------------------------------------------------------------------ what can be reached
# wgrad_h_kernel is instantiated for kHWgradTiles x SKIP x 32 | 64 pixels per K-step = 20.  SKIP needs more than one tap and
# Cin % tile columns == 0, so K >= 4 Cin >= 4 x the tile's columns; the 64- and 32-column tiles are picked for K <= 64 and K <= 32:
# SKIP = true on 128x64 and 128x32 (four instantiations) is compiled and cannot be selected.
H_TILES = [(128, 128), (128, 64), (128, 32), (64, 128), (32, 128)]
H_REACHABLE = {(t, skip, bkp) for t in H_TILES for skip in (0, 1) for bkp in BKPS if not (skip and t[1] < 128)}
H_UNREACHABLE = {((128, 64), 1, 32), ((128, 64), 1, 64), ((128, 32), 1, 32), ((128, 32), 1, 64)}
# wgrad_f32_dma_kernel: kWgradDmaTiles x skip where the table has a SKIP instantiation = 9; 128x64 with SKIP by the same argument
F_DMA_REACHABLE = {((128, 128), 0), ((128, 128), 1), ((128, 64), 0), ((64, 128), 0), ((64, 128), 1), ((32, 256), 0), ((32, 256), 1),
                   ((32, 288), 0)}
F_DMA_UNREACHABLE = {((128, 64), 1)}
# the pixel orders each exact-fp32 family can run
F_ORDERS = {WGRAD_DMA: {DENSE, SKIP_PATCHES, PACKED, ROW_MAJOR_DMA}, WGRAD_REGISTER: {DENSE, SKIP_ROWS, SKIP_PATCHES}}


def instance_h(rec):
    return (rec[1], rec[2]), rec[4], rec[3]


def instance_f(rec):
    return (rec[1], rec[2]), rec[4]


# ------------------------------------------------------------------------------------------------ the default plan
# What select_wgrad_h gives every CONV_CASES entry of tests/test_half_gpu.py with no switch set (case -> record without the kernel
# code), pinned: a planner change that moves the small cases shows up in both instance tests.
DEFAULT_PLAN_H = {
    (2, 64, 16, 16, 128, 1, 1, 0, 1): (128, 64, 64, 0, 0, 1, 2, 16, 2, 256),
    (2, 32, 20, 20, 64, 3, 1, 1, 1): (64, 128, 64, 0, 0, 0, 1, 32, 3, 288),
    (2, 64, 24, 24, 32, 3, 1, 6, 6): (32, 128, 64, 0, 0, 1, 4, 8, 4, 288),            # (64 channels: a column tile spans two taps)
    (2, 64, 24, 24, 32, 3, 1, 12, 12): (32, 128, 64, 0, 0, 1, 4, 8, 4, 288),
    (2, 64, 24, 24, 32, 3, 1, 18, 18): (32, 128, 64, 0, 0, 1, 4, 8, 4, 288),
    (2, 32, 33, 35, 64, 3, 2, 1, 1): (64, 128, 64, 0, 0, 0, 1, 32, 2, 320),
    (2, 64, 16, 16, 128, 1, 2, 0, 1): (128, 64, 64, 0, 0, 1, 4, 8, 1, 128),
    (2, 3, 64, 64, 64, 7, 2, 3, 1): (64, 128, 64, 0, 0, 1, 1, 32, 8, 256),
    (2, 384, 32, 32, 21, 3, 1, 1, 1): (32, 128, 64, 0, 0, 1, 1, 32, 8, 256),
    (2, 2048, 8, 8, 256, 3, 1, 6, 6): (128, 128, 32, 1, 2, 1, 4, 8, 1, 128),
    (2, 1280, 4, 4, 256, 3, 1, 1, 1): (128, 128, 32, 0, 0, 0, 1, 32, 1, 32),
    (4, 256, 1, 1, 64, 1, 1, 0, 1): (64, 128, 64, 0, 0, 0, 1, 32, 1, 32),
    (2, 88, 16, 16, 2, 3, 1, 1, 1): (32, 128, 64, 0, 0, 1, 2, 16, 2, 256),
    (1, 160, 9, 9, 64, 3, 1, 1, 1): (64, 128, 64, 0, 0, 0, 1, 32, 1, 96),
    (2, 512, 8, 8, 512, 3, 1, 2, 2): (128, 128, 32, 0, 0, 1, 4, 8, 1, 128),
    (1, 16, 130, 130, 16, 3, 1, 1, 1): (32, 128, 64, 0, 0, 0, 1, 32, 59, 288),
    (4, 256, 32, 32, 128, 1, 1, 0, 1): (128, 128, 64, 0, 0, 1, 1, 32, 16, 256),
    (4, 320, 4, 4, 1280, 1, 1, 0, 1): (128, 128, 64, 0, 0, 0, 1, 32, 1, 64),
    (4, 256, 8, 8, 1024, 1, 1, 0, 1): (128, 128, 64, 0, 0, 1, 4, 8, 1, 256),
    (2, 128, 48, 48, 128, 3, 1, 1, 1): (128, 128, 64, 0, 0, 1, 2, 16, 18, 256),
    (4, 16, 128, 128, 32, 3, 1, 1, 1): (32, 128, 64, 0, 0, 1, 1, 32, 128, 512),
    (2, 128, 32, 32, 64, 3, 1, 18, 18): (64, 128, 64, 1, 2, 1, 2, 16, 8, 256),
    (2, 128, 32, 32, 64, 3, 1, 12, 12): (64, 128, 64, 1, 2, 1, 4, 8, 8, 256),
    (3, 256, 16, 16, 128, 3, 1, 6, 6): (128, 128, 64, 1, 2, 1, 2, 16, 3, 256),
    (2, 64, 32, 32, 64, 3, 2, 1, 1): (64, 128, 64, 0, 0, 1, 2, 16, 2, 256),
    (2, 64, 32, 32, 128, 1, 2, 0, 1): (128, 64, 64, 0, 0, 1, 2, 16, 2, 256),
    (1, 32, 64, 48, 96, 3, 2, 1, 1): (128, 128, 64, 0, 0, 1, 4, 8, 3, 256),
    (2, 24, 40, 40, 144, 1, 1, 0, 1): (128, 32, 64, 0, 0, 1, 4, 8, 12, 288),
    (2, 144, 40, 40, 24, 1, 1, 0, 1): (32, 128, 64, 0, 0, 1, 4, 8, 12, 288),
    (8, 32, 64, 64, 32, 3, 1, 1, 1): (32, 128, 64, 0, 0, 1, 1, 32, 79, 416),
    (8, 64, 32, 32, 64, 3, 1, 1, 1): (64, 128, 64, 0, 0, 1, 1, 32, 32, 256),
    (8, 32, 64, 64, 64, 3, 2, 1, 1): (64, 128, 64, 0, 0, 1, 1, 32, 32, 256),
}
# ... which is nine of the sixteen reachable instantiations: the 32-pixel K-step only on 128x128 (it needs 128 filters or more and
# K >= 4096), skipping never on 32x128; the forced rows above reach the rest
DEFAULT_REACH_H = {((32, 128), 0, 64), ((64, 128), 0, 64), ((64, 128), 1, 64), ((128, 32), 0, 64), ((128, 64), 0, 64),
                   ((128, 128), 0, 32), ((128, 128), 0, 64), ((128, 128), 1, 32), ((128, 128), 1, 64)}

