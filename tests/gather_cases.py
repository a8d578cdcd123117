"""The case tables of the exact-fp32 / limb gather-conv instantiation tests (csrc/conv_gather.hip), shared by
tests/test_gather_instances_cpu.py, which proves through the pure query pseg_conv2d_gather_choice that every row reaches the launch
it claims, and tests/test_gather_instances_gpu.py, which runs every row against fp64.

A row is (id, case, dgrad, prec, modes, env, record, tags):
  case    (B, Cin, H, W, Cout, k, stride, pad, dil), a square k x k conv; channel counts as the model has them (the kernels see them
          padded to 4)
  dgrad   0: the forward conv of the case, 1: its data gradient (GEMM rows = input pixels, N = Cin, gathers dy's Cout channels)
  prec    PSEG_PREC_*: 0 fp32, 1 bf16x3, 2 bf16x6, 3 fp16x3 -- the caller's request
  modes   what the GPU file runs: forward 'plain', 'bias', 'acc' (accumulated onto a filled tensor), 'bias+acc', 'stats' (fused
          BatchNorm statistics); data gradient 'plain', 'acc', 'bns' (fused BatchNorm-backward sums), 'planes' / 'planes+acc'
          (pre-split limb planes: pseg_conv2d_dgrad_planes).  Every mode of a row must select the row's record (the sums' flag
          apart): a mode that changes the selection -- fused statistics take the 256x128 tile away -- is not in the row.
  env     the planning switches of the row: those documented in conv_common.h (SWITCHES) and nothing else
  record  what pseg_debug_last_gather must answer after the launch (pseg_amd.h): kernel code, tile rows, tile columns, arithmetic
          as run, SKIP flag, ring depth, GENERIC flag, row_perm, patch rows, patch columns, K splits, fused sums, offered to the
          persistent kernel.  pseg_conv2d_gather_choice answers the same, except that it names the tile-per-block kernel where the
          persistent one is tried first (as_query).
  tags    'skip': also run with PSEG_CONV_NOSKIP=1 on the same tile, bit-identical; 'pw': also run with PSEG_CONV_PW=0 (the ring
          kernel), bit-identical; 'sliced': also run with operands that are channel slices of wider tensors

The expectations are written from the selection's rules (plan_gather, gather_row_order, select_gather), not read back from the
library:
  * a forced tile (PSEG_CONV_BM / _BN) is taken as it is and switches the patch and class-sorted searches off; PSEG_CONV_FORCEBIG
    gives the two-limb arithmetics (bf16x3, fp16x3) the 256x128 tile unless fused statistics are asked for
  * K splits: PSEG_CONV_SPLITK=n gives cdiv(K-steps, cdiv(K-steps, n)) splits; the problems here have fewer than 32 K-steps, so
    pick_splits (16 K-steps per split at the least) leaves them whole; a split plan runs on the register-staged kernel
  * exact fp32, one split, a tile of kF32Tiles: gathered channels % 32 == 0 -> the ring kernel (PSEG_CONV_F32DMA 3 -> two stages,
    1 -> three, 0 -> the register-staged kernel); % 4 only -> its GENERIC form, two stages; a 3x3 at unit stride and rate on a map
    of whole 8 x 16 patches with a 128x64 / 128x32 tile -> the halo kernel; a 1x1 (row_perm 3) of at most 32 K-steps on a tile
    marked pw -> offered to the persistent kernel, which takes it when there are more tiles than PSEG_CONV_PW_RESIDENT blocks
  * SKIP: more than one tap, rate >= 4, gathered channels % 32 == 0, not PSEG_CONV_NOSKIP; the stride-2 data gradient of a map
    whose parity classes are whole tiles runs in parity order (row_perm 1) with SKIP
  * every other arithmetic runs on the register-staged kernel; the pre-split planes on gather_limb_dma_kernel (256x128) or nowhere"""
import collections

Row = collections.namedtuple('Row', 'id case dgrad prec modes env record tags')

REGISTER, LIMB_DMA, RING, RING_GENERIC, POINTWISE, HALO = 1, 2, 3, 4, 5, 6       # PSEG_KERNEL_GATHER_*
FP32, BF16X3, BF16X6, FP16X3 = 0, 1, 2, 3                                         # PSEG_PREC_*
PREC_NAMES = ['fp32', 'bf16x3', 'bf16x6', 'fp16x3']
SWITCHES = ('PSEG_CONV_BM', 'PSEG_CONV_BN', 'PSEG_CONV_SPLITK', 'PSEG_CONV_NOSKIP', 'PSEG_CONV_NOBAND', 'PSEG_CONV_NOBIG',
            'PSEG_CONV_FORCEBIG', 'PSEG_CONV_F32DMA', 'PSEG_CONV_PW', 'PSEG_CONV_PW_RESIDENT', 'PSEG_CONV_HALO')
FIELDS = ('kernel', 'tile rows', 'tile columns', 'arithmetic', 'SKIP', 'ring depth', 'GENERIC', 'row_perm', 'patch rows',
          'patch columns', 'K splits', 'fused sums', 'offered to the persistent kernel')
KERNEL, BM, BN, PREC, SKIP, STAGES, GENERIC, PERM, PATCH_H, PATCH_W, SPLITS, BNS, TRY_PW = range(13)

REG_TILES = [(128, 128), (128, 64), (128, 32), (64, 128), (32, 128)]      # gather_conv_kernel (launch_tiles' slots 0 .. 4)
BIG = (256, 128)                                                          # ... and slot 5, bf16x3 and fp16x3 only
F32_TILES = [(128, 128), (128, 64), (64, 128), (128, 32)]                 # kF32Tiles, in the table's order
PW_TILES = [(128, 128), (128, 64), (64, 128)]                             # ... those marked pw
HALO_TILES = [(128, 64), (128, 32)]                                       # ... those with a halo instantiation
WAVE_ROWS = {(128, 128): 2, (128, 64): 2, (64, 128): 2, (128, 32): 4, (32, 128): 1, (256, 128): 4}     # waves_m

FWD_MODES = ('plain', 'bias', 'acc', 'stats')
DGRAD_MODES = ('plain', 'acc')

# B, Cin, H, W, Cout, k, stride, pad, dil
GRID = (1, 64, 13, 13, 136, 3, 1, 1, 1)       # M = 169: ragged 128-, 64- and 32-row tiles; N = 136: ragged 128-, 64-, 32-column tiles;
                                              # K = 576: 18 K-steps, every ring wraps
GRID_T = (1, 136, 13, 13, 64, 3, 1, 1, 1)     # mirrored: its data gradient is the same M x N x K with a plain gather (GRID's own data
                                              # gradient gathers 136 channels, off the K-step grid: GENERIC)
DIL24 = (2, 64, 24, 24, 32, 3, 1, 12, 12)     # CONV_CASES' rate-12 conv: whole (tile, tap) pairs are padding
DIL16 = (1, 64, 16, 16, 32, 3, 1, 12, 12)     # rate 12 on 16 x 16: a side tap is live on 4 of 16 columns / rows -- the live K-steps
                                              # of a tile do not come in adjacent pairs
S2 = (2, 64, 32, 32, 64, 3, 2, 1, 1)          # stride-2 data gradient: parity classes of 16 x 16 = 256 rows, whole tiles of every shape
ONE = (1, 32, 13, 13, 136, 1, 1, 0, 1)        # 1x1 on 32 channels: ONE K-step, shorter than either ring
ONE_T = (1, 136, 13, 13, 32, 1, 1, 0, 1)
GEN = (1, 40, 13, 13, 136, 3, 1, 1, 1)        # 40 channels: K = 360, K-steps straddle taps, the last one is a quarter full
STEM = (1, 3, 30, 30, 20, 7, 2, 3, 1)         # 3 -> 4 padded channels, 7x7 stride 2: 49 taps, K = 196; 15 x 15 outputs
HALO_MAP = (1, 32, 16, 32, 40, 3, 1, 1, 1)    # 2 x 2 patches of 8 x 16 pixels; 40 filters: ragged 32- and 64-column tiles
HALO_MAP_T = (1, 40, 16, 32, 32, 3, 1, 1, 1)
PW = (2, 64, 13, 13, 136, 1, 1, 0, 1)         # M = 338: 3 x 2 / 3 x 3 / 6 x 2 tiles of 128x128 / 128x64 / 64x128
PW_T = (2, 136, 13, 13, 64, 1, 1, 0, 1)
PW_RESIDENT = 5                               # blocks: 6, 9, 12 tiles over 5 blocks -> 2+1+1+1+1, 2+2+2+2+1, 3+3+2+2+2
LIMB = (1, 136, 13, 13, 32, 3, 1, 1, 1)       # the pre-split limb kernel wants N = Cin >= 128 and gathered channels % 32 == 0: one
                                              # ragged 256-row tile x two column tiles (the second 8 wide)
LIMB_SKIP = (1, 136, 16, 16, 32, 3, 1, 12, 12)


def out_size(n, k, stride, pad, dil):
    return (n + 2 * pad - dil * (k - 1) - 1) // stride + 1


def r4(c):
    return (c + 3) // 4 * 4


def geometry(case):
    """-> (B, H, W, Cin, Ho, Wo, Cout, kh, kw, stride, pad, dil) with the channel counts padded as the kernels take them"""
    B, Cin, H, W, Cout, k, stride, pad, dil = case
    return B, H, W, r4(Cin), out_size(H, k, stride, pad, dil), out_size(W, k, stride, pad, dil), r4(Cout), k, k, stride, pad, dil


def record(kernel, tile, prec=FP32, skip=0, stages=0, generic=0, perm=0, patch=(0, 0), splits=1, bns=0, try_pw=0):
    return (kernel, tile[0], tile[1], prec, skip, stages, generic, perm, patch[0], patch[1], splits, bns, try_pw)


def with_sums(rec):
    return rec[:BNS] + (1,) + rec[BNS + 1:]


def expected(row, mode):
    """the record of a row's launch in one of its modes"""
    return with_sums(row.record) if mode == 'bns' else row.record


def as_query(rec):
    """... as pseg_conv2d_gather_choice states it: where the persistent kernel is tried first the kernel code and the ring depth
    are those of the tile-per-block launch it may fall back to"""
    if rec[KERNEL] == POINTWISE:
        return (RING,) + rec[1:STAGES] + (2,) + rec[STAGES + 1:]
    return rec


MODE_FLAGS = {            # (stats, bias, planes, bns, accumulate) of pseg_conv2d_gather_choice
    'plain': (0, 0, 0, 0, 0), 'bias': (0, 1, 0, 0, 0), 'acc': (0, 0, 0, 0, 1), 'bias+acc': (0, 1, 0, 0, 1), 'stats': (1, 0, 0, 0, 0),
    'bns': (0, 0, 0, 1, 0), 'planes': (0, 0, 1, 0, 0), 'planes+acc': (0, 0, 1, 0, 1),
}


def choice(lib, case, dgrad, prec, mode='plain'):
    """the record of the launch that WOULD run (the switches must be set): the pure query, or the library's message"""
    import ctypes
    out = (ctypes.c_int * 13)()
    rc = lib.pseg_conv2d_gather_choice(*geometry(case), dgrad, prec, *MODE_FLAGS[mode], out)
    assert rc == 0, lib.pseg_last_error()
    return tuple(out)


def describe(rec):
    return ', '.join('%s %d' % (n, v) for n, v in zip(FIELDS, rec))


def forced(tile, **more):
    env = {'PSEG_CONV_BM': tile[0], 'PSEG_CONV_BN': tile[1]}
    env.update(('PSEG_CONV_' + k, v) for k, v in more.items())
    return env


def _t(tile):
    return '%dx%d' % tile


ROWS = []


def add(id, case, dgrad, prec, modes, env, rec, *tags):
    ROWS.append(Row(id, case, dgrad, prec, tuple(modes), env, rec, tuple(tags)))


# ------------------------------------------------------------------------------------------------ the register-staged kernel
# gather_conv_kernel<tile, SKIP, arithmetic>: 5 tiles x SKIP x 4 arithmetics, + 256x128 x SKIP x {bf16x3, fp16x3}
for _tile in REG_TILES:
    for _p in (FP32, BF16X3, BF16X6, FP16X3):
        _id = 'reg-%s-%s' % (_t(_tile), PREC_NAMES[_p])
        _env = forced(_tile, F32DMA=0)
        _sl = ('sliced',) if _p == FP32 else ()
        add(_id + '-fwd', GRID, 0, _p, FWD_MODES, _env, record(REGISTER, _tile, _p), *_sl)
        add(_id + '-dgrad', GRID_T, 1, _p, DGRAD_MODES, _env, record(REGISTER, _tile, _p), *_sl)
        # the SKIP siblings: the dilated problems, and the stride-2 data gradient in parity order
        add(_id + '-rate12-24x24-fwd', DIL24, 0, _p, FWD_MODES, _env, record(REGISTER, _tile, _p, skip=1), 'skip')
        add(_id + '-rate12-24x24-dgrad', DIL24, 1, _p, DGRAD_MODES, _env, record(REGISTER, _tile, _p, skip=1), 'skip')
        add(_id + '-rate12-16x16-fwd', DIL16, 0, _p, ('plain', 'bias', 'acc'), _env, record(REGISTER, _tile, _p, skip=1), 'skip')
        add(_id + '-stride2-dgrad', S2, 1, _p, DGRAD_MODES, _env, record(REGISTER, _tile, _p, skip=1, perm=1), 'skip')
    # a 1x1 at unit stride: the 1 x M image (row_perm 3) on the register-staged kernel
    add('reg-%s-fp32-1x1-fwd' % _t(_tile), ONE, 0, FP32, FWD_MODES, forced(_tile, F32DMA=0), record(REGISTER, _tile, perm=3))
# 256x128 (PSEG_CONV_FORCEBIG; fused statistics would take the tile away: not among the modes).  No tile is forced, so the planner's
# searches run: on DIL24 the rows sorted by liveness class win (row_perm 4), on the 16 x 16 map (one 256-row tile) nothing does
for _p in (BF16X3, FP16X3):
    _id = 'reg-256x128-%s' % PREC_NAMES[_p]
    _env = {'PSEG_CONV_FORCEBIG': 1}
    _sl = ('sliced',) if _p == BF16X3 else ()       # (the eight-wave 4 x 2 layout: an epilogue and a gather of its own)
    add(_id + '-fwd', GRID, 0, _p, ('plain', 'bias', 'acc'), _env, record(REGISTER, BIG, _p), *_sl)
    add(_id + '-dgrad', GRID_T, 1, _p, DGRAD_MODES, _env, record(REGISTER, BIG, _p), *_sl)
    add(_id + '-rate12-24x24-fwd', DIL24, 0, _p, ('plain', 'bias', 'acc'), _env, record(REGISTER, BIG, _p, skip=1, perm=4), 'skip')
    add(_id + '-rate12-24x24-dgrad', DIL24, 1, _p, DGRAD_MODES, _env, record(REGISTER, BIG, _p, skip=1, perm=4), 'skip')
    add(_id + '-rate12-16x16-fwd', DIL16, 0, _p, ('plain', 'bias', 'acc'), _env, record(REGISTER, BIG, _p, skip=1), 'skip')
    add(_id + '-stride2-dgrad', S2, 1, _p, DGRAD_MODES, _env, record(REGISTER, BIG, _p, skip=1, perm=1), 'skip')
# split K, one tile per arithmetic: 18 K-steps in 2 x 9, and in 5 + 5 + 5 + 3 (PSEG_CONV_SPLITK=4: cdiv(18, 4) = 5 per split, a ragged
# last one); bias and accumulation go through launch_slab_reduce
SPLIT_TILES = {FP32: (128, 128), BF16X3: (128, 64), BF16X6: (64, 128), FP16X3: (32, 128)}
for _p, _tile in SPLIT_TILES.items():
    for _n in (2, 4):
        _id = 'reg-%s-%s-splits%d' % (_t(_tile), PREC_NAMES[_p], _n)
        _env = forced(_tile, SPLITK=_n)
        add(_id + '-fwd', GRID, 0, _p, ('plain', 'bias', 'acc', 'bias+acc'), _env, record(REGISTER, _tile, _p, splits=_n))
        add(_id + '-dgrad', GRID_T, 1, _p, DGRAD_MODES, _env, record(REGISTER, _tile, _p, splits=_n))

# ------------------------------------------------------------------------------------------------ the ring kernel
# gather_f32_dma_kernel<tile, SKIP, stages, GENERIC = false>: kF32Tiles x {plain, SKIP} x {2, 3}.  PSEG_CONV_SPLITK=1 throughout
# (harmless where the plan would not split)
for _tile in F32_TILES:
    for _stages, _mode in ((2, 3), (3, 1)):
        _id = 'ring-%s-depth%d' % (_t(_tile), _stages)
        _env = forced(_tile, SPLITK=1, F32DMA=_mode)
        _sl = ('sliced',) if _stages == 2 else ()
        add(_id + '-fwd', GRID, 0, FP32, FWD_MODES, _env, record(RING, _tile, stages=_stages), *_sl)
        add(_id + '-dgrad', GRID_T, 1, FP32, DGRAD_MODES + ('bns',), _env, record(RING, _tile, stages=_stages), *_sl)
        add(_id + '-rate12-24x24-fwd', DIL24, 0, FP32, FWD_MODES, _env, record(RING, _tile, skip=1, stages=_stages), 'skip')
        add(_id + '-rate12-24x24-dgrad', DIL24, 1, FP32, DGRAD_MODES + ('bns',), _env, record(RING, _tile, skip=1, stages=_stages), 'skip')
        add(_id + '-rate12-16x16-fwd', DIL16, 0, FP32, ('plain', 'bias', 'acc'), _env, record(RING, _tile, skip=1, stages=_stages), 'skip')
        add(_id + '-stride2-dgrad', S2, 1, FP32, DGRAD_MODES + ('bns',), _env, record(RING, _tile, skip=1, stages=_stages, perm=1), 'skip')
        # one K-step: the contraction is shorter than the ring (PSEG_CONV_PW=0: a 1x1 would be offered to the persistent kernel)
        _env1 = dict(_env, PSEG_CONV_PW=0)
        add(_id + '-1x1-fwd', ONE, 0, FP32, FWD_MODES, _env1, record(RING, _tile, stages=_stages, perm=3))
        add(_id + '-1x1-dgrad', ONE_T, 1, FP32, DGRAD_MODES, _env1, record(RING, _tile, stages=_stages, perm=3))
# GENERIC: two stages whatever PSEG_CONV_F32DMA says
for _tile in F32_TILES:
    _id = 'generic-%s' % _t(_tile)
    _env = forced(_tile, SPLITK=1)
    _rec = record(RING_GENERIC, _tile, stages=2, generic=1)
    add(_id + '-40ch-fwd', GEN, 0, FP32, FWD_MODES, _env, _rec, 'sliced')
    add(_id + '-136ch-dgrad', GRID, 1, FP32, DGRAD_MODES, _env, _rec, 'sliced')
    add(_id + '-stem-fwd', STEM, 0, FP32, FWD_MODES, _env, _rec)
    add(_id + '-stem-dgrad', STEM, 1, FP32, DGRAD_MODES, _env, _rec)
# ... and a 1x1 off the K-step grid: GENERIC on the 1 x M image (row_perm 3), two K-steps of which the second holds 8 channels
GEN_1X1 = (1, 40, 13, 13, 136, 1, 1, 0, 1)
add('generic-128x128-40ch-1x1-fwd', GEN_1X1, 0, FP32, FWD_MODES, forced((128, 128), SPLITK=1), record(RING_GENERIC, (128, 128), stages=2, generic=1, perm=3))
# (that PSEG_CONV_F32DMA=1 leaves GENERIC at two stages, and that the default plan runs the stem on 128x32, are statements about
# the selection: tests/test_gather_instances_cpu.py asks the query; the instantiations are those of the rows above)

# ------------------------------------------------------------------------------------------------ the halo kernel
for _tile in HALO_TILES:
    _env = forced(_tile, SPLITK=1)
    _rec = record(HALO, _tile, perm=2, patch=(8, 16))
    add('halo-%s-fwd' % _t(_tile), HALO_MAP, 0, FP32, FWD_MODES, _env, _rec, 'sliced')
    add('halo-%s-dgrad' % _t(_tile), HALO_MAP_T, 1, FP32, DGRAD_MODES + ('bns',), _env, _rec, 'sliced')

# ------------------------------------------------------------------------------------------------ the persistent pointwise kernel
# gather_f32_pw_kernel<tile, BNS>: three tiles x {plain, fused sums}
for _tile in PW_TILES:
    _env = forced(_tile, PW_RESIDENT=PW_RESIDENT)
    _rec = record(POINTWISE, _tile, perm=3, try_pw=1)
    add('pw-%s-fwd' % _t(_tile), PW, 0, FP32, FWD_MODES, _env, _rec, 'pw', 'sliced')
    add('pw-%s-dgrad' % _t(_tile), PW_T, 1, FP32, DGRAD_MODES + ('bns',), _env, _rec, 'pw', 'sliced')

# ------------------------------------------------------------------------------------------------ the pre-split limb kernel
# gather_limb_dma_kernel<SKIP>.  PSEG_CONV_NOBAND=1 on the dilated row is not needed: one 256-row tile has nothing to sort
_env = {'PSEG_CONV_FORCEBIG': 1}
add('limb-dma-dgrad', LIMB, 1, BF16X3, ('planes', 'planes+acc'), _env, record(LIMB_DMA, BIG, BF16X3), 'sliced')
add('limb-dma-rate12-16x16-dgrad', LIMB_SKIP, 1, BF16X3, ('planes', 'planes+acc'), _env, record(LIMB_DMA, BIG, BF16X3, skip=1), 'skip')
# ... in parity order (stride 2: four classes of 16 x 16 = 256 rows, one tile each) and with class-sorted rows (DIL24's map, 136 wide)
LIMB_S2 = (1, 128, 32, 32, 32, 3, 2, 1, 1)
LIMB_BAND = (2, 136, 24, 24, 32, 3, 1, 12, 12)
add('limb-dma-stride2-dgrad', LIMB_S2, 1, BF16X3, ('planes', 'planes+acc'), _env, record(LIMB_DMA, BIG, BF16X3, skip=1, perm=1), 'skip')
add('limb-dma-rate12-24x24-dgrad', LIMB_BAND, 1, BF16X3, ('planes',), _env, record(LIMB_DMA, BIG, BF16X3, skip=1, perm=4), 'skip')
# ... in 16 x 16 patches (rate 18 on a 32 x 32 map: the corner patches keep four taps of nine) and as a 1x1's 1 x M image
LIMB_PATCH = (1, 128, 32, 32, 32, 3, 1, 18, 18)
LIMB_1X1 = (1, 136, 13, 13, 32, 1, 1, 0, 1)
add('limb-dma-rate18-32x32-dgrad', LIMB_PATCH, 1, BF16X3, ('planes',), _env, record(LIMB_DMA, BIG, BF16X3, skip=1, perm=2, patch=(16, 16)), 'skip')
add('limb-dma-1x1-dgrad', LIMB_1X1, 1, BF16X3, ('planes', 'planes+acc'), _env, record(LIMB_DMA, BIG, BF16X3, perm=3))

# ------------------------------------------------------------------------------------------------ row orders at the default plan
# No tile forced (a forced tile switches both searches off).  The cheapest problems of a search over the query -- maps 8 .. 64,
# batches 1 .. 16, channels 32 .. 2048, rates 4 / 6 / 12 / 18, both directions -- that select
#   class-sorted rows (row_perm 4): rate 4 on an 8 x 8 map, 32 -> 32 channels -- the 64 pixels fall into 3 x 3 liveness classes of one
#     128x32 tile (rate 6 on the same map selects them too, from 64 channels on);
#   the patch order (row_perm 2): rate 18 on a 32 x 32 map, 32 -> 64 channels, 16 x 8 patches on 128x64.  Maps under 32 x 32 select
#     it too, but only from 24 x 24 with a batch of 4 and 2048 -> 256 channels on (a 22-GFLOP reference in fp64): the 32 x 32 map
#     is the smallest WORK that does.
# Each on the ring kernel and, with PSEG_CONV_F32DMA=0 or another arithmetic, on the register-staged one.
BAND = (1, 32, 8, 8, 32, 3, 1, 4, 4)
PATCH = (1, 32, 32, 32, 64, 3, 1, 18, 18)
add('default-class-sorted-ring-fwd', BAND, 0, FP32, ('plain', 'stats'), {}, record(RING, (128, 32), skip=1, stages=2, perm=4), 'skip')
add('default-class-sorted-register-fwd', BAND, 0, FP32, ('plain', 'stats'), {'PSEG_CONV_F32DMA': 0}, record(REGISTER, (128, 32), skip=1, perm=4), 'skip')
add('default-class-sorted-bf16x3-fwd', BAND, 0, BF16X3, ('plain',), {}, record(REGISTER, (128, 32), BF16X3, skip=1, perm=4), 'skip')
add('default-patches-ring-fwd', PATCH, 0, FP32, ('plain', 'stats'), {}, record(RING, (128, 64), skip=1, stages=2, perm=2, patch=(16, 8)), 'skip')
add('default-patches-register-fwd', PATCH, 0, FP32, ('plain', 'stats'), {'PSEG_CONV_F32DMA': 0},
    record(REGISTER, (128, 64), skip=1, perm=2, patch=(16, 8)), 'skip')
add('default-patches-bf16x6-fwd', PATCH, 0, BF16X6, ('plain',), {}, record(REGISTER, (128, 64), BF16X6, skip=1, perm=2, patch=(16, 8)), 'skip')

# ------------------------------------------------------------------------------------------------ refusals
# (id, case, dgrad, prec, mode, env): pseg_conv2d_gather_choice answers kernel 0 and the entry point returns an error without a
# launch.  The C ABI cannot ask for the fused sums AND accumulation (pseg_conv2d_dgrad_bnstat has no accumulate argument; ops takes
# the plain data gradient): that combination is a refusal of the choice only; the launch-side case of the sums is a problem no
# LDS-DMA kernel takes (PSEG_CONV_F32DMA=0), where pseg_conv2d_dgrad_bnstat_rows is 0 and the entry point refuses any part_rows.
# fp16x3 without the operands' amax is refused by the entry point alone (the query has no such argument).
REFUSALS = [
    ('fp32-on-256x128', GRID, 0, FP32, 'plain', forced(BIG)),
    ('bf16x6-on-256x128', GRID_T, 1, BF16X6, 'plain', forced(BIG)),
    ('sums-with-accumulate', GRID_T, 1, FP32, 'bns+acc', forced((128, 64), SPLITK=1)),
    ('sums-on-the-register-kernel', GRID_T, 1, FP32, 'bns', forced((128, 64), F32DMA=0)),
    ('planes-uncovered', LIMB, 1, BF16X3, 'planes', {}),
    ('statistics-of-a-split-plan', GRID, 0, FP32, 'stats', forced((128, 128), SPLITK=2)),
]
MODE_FLAGS['bns+acc'] = (0, 0, 0, 1, 1)

# ------------------------------------------------------------------------------------------------ what is compiled, what can be reached
REGISTER_COMPILED = {(t, s, p) for t in REG_TILES for s in (0, 1) for p in range(4)} | {(BIG, s, p) for s in (0, 1) for p in (BF16X3, FP16X3)}
RING_COMPILED = {(t, s, st, 0) for t in F32_TILES for s in (0, 1) for st in (2, 3)} | {(t, 0, 2, 1) for t in F32_TILES}
HALO_COMPILED = set(HALO_TILES)
PW_COMPILED = {(t, b) for t in PW_TILES for b in (0, 1)}
LIMB_COMPILED = {0, 1}
UNREACHABLE = set()       # every one of the 74 can be selected: the rows above do


def instance(rec):
    """(kernel family, instantiation) of a record"""
    tile = (rec[BM], rec[BN])
    if rec[KERNEL] == REGISTER:
        return 'register', (tile, rec[SKIP], rec[PREC])
    if rec[KERNEL] in (RING, RING_GENERIC):
        return 'ring', (tile, rec[SKIP], rec[STAGES], rec[GENERIC])
    if rec[KERNEL] == HALO:
        return 'halo', tile
    if rec[KERNEL] == POINTWISE:
        return 'pw', (tile, rec[BNS])
    if rec[KERNEL] == LIMB_DMA:
        return 'limb', rec[SKIP]
    return 'refused', None


def instances_hit(rows=None):
    hit = collections.defaultdict(set)
    for row in ROWS if rows is None else rows:
        for mode in row.modes:
            fam, inst = instance(expected(row, mode))
            hit[fam].add(inst)
    return hit


# the row orders each kernel family accepts (gather_row_order + select_gather): the register-staged and ring kernels all five, the
# GENERIC form 0 and 3, the halo kernel its own patches, the persistent kernel the 1 x M image, the limb kernel all five
ROW_ORDERS = {REGISTER: {0, 1, 2, 3, 4}, RING: {0, 1, 2, 3, 4}, RING_GENERIC: {0, 3}, HALO: {2}, POINTWISE: {3}, LIMB_DMA: {0, 1, 2, 3, 4}}


def row_key(row):
    """what a row is in the table for: (kernel family, instantiation of its plain mode, problem, direction, row order, K splits)"""
    return instance(row.record) + (row.case, row.dgrad, row.record[PERM], row.record[SPLITS])


def required():
    """The (instantiation, problem) pairs the table must hold, stated per instantiation and apart from the loops that build ROWS:
    every row must be one of them, none may be missing, and no two rows may stand for the same one -- so a row taken out of the
    table is a pair missing here (tests/test_gather_instances_cpu.py)."""
    need = set()

    def want(fam, inst, problems, perm=0, splits=1):
        for case, dgrad in problems:
            need.add((fam, inst, case, dgrad, perm, splits))

    dense, one = [(GRID, 0), (GRID_T, 1)], [(ONE, 0), (ONE_T, 1)]
    dilated, strided = [(DIL24, 0), (DIL24, 1), (DIL16, 0)], [(S2, 1)]
    for p in range(4):                                            # gather_conv_kernel
        for t in REG_TILES:
            want('register', (t, 0, p), dense)
            want('register', (t, 1, p), dilated)
            want('register', (t, 1, p), strided, perm=1)
        for n in (2, 4):
            want('register', (SPLIT_TILES[p], 0, p), dense, splits=n)
    for t in REG_TILES:
        want('register', (t, 0, FP32), one[:1], perm=3)
    for p in (BF16X3, FP16X3):
        want('register', (BIG, 0, p), dense)
        want('register', (BIG, 1, p), dilated[:2], perm=4)        # (no forced tile: the class-sorted rows win on DIL24)
        want('register', (BIG, 1, p), dilated[2:])
        want('register', (BIG, 1, p), strided, perm=1)
    for t in F32_TILES:                                           # gather_f32_dma_kernel
        for st in (2, 3):
            want('ring', (t, 0, st, 0), dense)
            want('ring', (t, 0, st, 0), one, perm=3)
            want('ring', (t, 1, st, 0), dilated)
            want('ring', (t, 1, st, 0), strided, perm=1)
        want('ring', (t, 0, 2, 1), [(GEN, 0), (GRID, 1), (STEM, 0), (STEM, 1)])
    want('ring', ((128, 128), 0, 2, 1), [(GEN_1X1, 0)], perm=3)
    for t in HALO_TILES:                                          # gather_f32_halo_kernel
        want('halo', t, [(HALO_MAP, 0), (HALO_MAP_T, 1)], perm=2)
    for t in PW_TILES:                                            # gather_f32_pw_kernel (the BNS sibling: the 'bns' mode of the dgrad row)
        want('pw', (t, 0), [(PW, 0), (PW_T, 1)], perm=3)
    want('limb', 0, [(LIMB, 1)])                                  # gather_limb_dma_kernel
    want('limb', 0, [(LIMB_1X1, 1)], perm=3)
    want('limb', 1, [(LIMB_SKIP, 1)])
    want('limb', 1, [(LIMB_S2, 1)], perm=1)
    want('limb', 1, [(LIMB_PATCH, 1)], perm=2)
    want('limb', 1, [(LIMB_BAND, 1)], perm=4)
    # the row orders of the default plan, on the ring and on the register-staged kernel
    want('ring', ((128, 32), 1, 2, 0), [(BAND, 0)], perm=4)
    want('ring', ((128, 64), 1, 2, 0), [(PATCH, 0)], perm=2)
    want('register', ((128, 32), 1, FP32), [(BAND, 0)], perm=4)
    want('register', ((128, 32), 1, BF16X3), [(BAND, 0)], perm=4)
    want('register', ((128, 64), 1, FP32), [(PATCH, 0)], perm=2)
    want('register', ((128, 64), 1, BF16X6), [(PATCH, 0)], perm=2)
    return need
