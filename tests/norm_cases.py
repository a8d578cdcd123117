"""The case table of the BatchNorm / activation instance tests (csrc/norm_act.hip), importable without a GPU.  Shared by
tests/test_norm_instances_cpu.py (the table reaches every compiled instance; the refusals; the mirror against the library's own
queries) and tests/test_norm_instances_gpu.py (every row launched, its record read back, every output against fp64).

Three parts:
  * a mirror of the host rules that choose a launch: stat_group, stat_block, ew_grid, the row-block (RB) sweep sizing of the apply
    and fp16 forward-rows kernels, pseg_bn_small_path's rule and the finalize thresholds -- written from the source, not read back;
  * the compiled instances of every __global__ function of the file (*_COMPILED), written out from the dispatch code;
  * the rows.  A row is (id, entry, dtype, M, C, ld, flags, record):
      entry   which runner of the GPU test takes it (the C entry points it calls are listed beside the runner)
      dtype   'f' (fp32 storage) or 'h' (fp16)
      ld      None: every operand dense (ld == C); else {operand: (ld, first channel)}: the operand is a channel slice of a wider
              buffer whose other channels hold a NaN canary
      flags   dict of the arguments the row sets (act, mode, residual, dres, res_accumulate, accumulate, frozen, planes, ...)
      record  what pseg_debug_last_norm must answer after the row's LAST launch (pseg_amd.h); rows that chain launches carry the
              records of the earlier ones in flags['records']

Outside this table: PSEG_BN_FWD_ROWS and PSEG_BN_SMALL are read once per process, so the rows-kernel-with-residual form
(PSEG_BN_FWD_ROWS=2) and PSEG_BN_SMALL=0 (pseg_bn_small_path answering 0 everywhere) cannot be reached without a child process and
are not run here; the fused kernels are called through their own entry points, whatever pseg_bn_small_path recommends."""
import collections

Row = collections.namedtuple('Row', 'id entry dtype M C ld flags record')
Refusal = collections.namedtuple('Refusal', 'id name args rc match')

NONE, RELU, RELU6 = 0, 1, 2                                             # PSEG_ACT_*
ERR_ARG, ERR_WORKSPACE = -1, -3                                         # PSEG_ERR_*
FIELDS = ('kernel', 'fp16', 'V', 'NR', 'MODE', 'LANES', 'block x', 'block y', 'grid x', 'grid y', 'rows', 'two-stage')
# kernel codes of pseg_debug_last_norm (enum NormKernel)
(COL_STATS, BWD_REDUCE, STAT_MERGE, FINALIZE, BWD_FINALIZE, COL_REDUCE, EVAL_COEFFS, ACT_FWD, ACT_FWD_ROWS, BWD_APPLY, ACT_BWD,
 COPY2D, FWD_SMALL, BWD_SMALL) = range(1, 15)
KERNEL_NAMES = {COL_STATS: 'col_stats_kernel', BWD_REDUCE: 'bn_bwd_reduce_kernel', STAT_MERGE: 'stat_merge_kernel',
                FINALIZE: 'bn_finalize_kernel', BWD_FINALIZE: 'bn_bwd_finalize_kernel', COL_REDUCE: 'col_reduce_kernel',
                EVAL_COEFFS: 'bn_eval_coeffs_kernel', ACT_FWD: 'bn_act_fwd_kernel', ACT_FWD_ROWS: 'bn_act_fwd_rows_kernel',
                BWD_APPLY: 'bn_act_bwd_apply_kernel', ACT_BWD: 'act_bwd_kernel', COPY2D: 'copy2d_kernel',
                FWD_SMALL: 'bn_fwd_small_kernel', BWD_SMALL: 'bn_bwd_small_kernel'}


def describe(rec):
    return '%s: ' % KERNEL_NAMES.get(rec[0], '?') + ', '.join('%s %d' % (n, v) for n, v in zip(FIELDS[1:], rec[1:]))


# ------------------------------------------------------------------------------------------------ the mirror of the host rules
kMaxStatRows = 512
kFinCh, kFinLanes, kFinLanesWide, kFinWideRows = 8, 32, 128, 128
kMergePer, kTwoStageRows = 64, 2048
kSmallCh, kSmallRowsPerBlock, kSmallMaxPartials = 64, 64, 64
kSmallMaxElements = 8 << 20
kEwMaxBlocks = 256 * 8


def cdiv(a, b):
    return -(-a // b)


def stat_group(M, C):
    """rows per statistics group (always from C / 4, also for the 8-channel lanes)"""
    c4 = C // 4
    tx = 64 if c4 >= 64 else (32 if c4 > 16 else 16)
    colblocks = cdiv(c4, tx)
    r = kMaxStatRows
    while r > 32 and cdiv(M, r) * colblocks < 1024:
        r >>= 1
    return r


def stat_rows(M, C):
    return cdiv(M, stat_group(M, C))


def lane_channels(dtype):
    return 8 if dtype == 'h' else 4


def stat_block(C, V):
    """-> (block x, block y, column blocks)"""
    cv = C // V
    tx = 64 if cv >= 64 else (32 if cv > 16 else (16 if cv > 8 else 8))
    return tx, 256 // tx, cdiv(cv, tx)


def ew_grid(total):
    return max(1, min(cdiv(total, 256), kEwMaxBlocks))


def row_block(M, C, V, NR):
    """the apply / forward-rows launches -> (block x, block y, grid x, grid y, RB, sweeps)"""
    tx, ty, gy = stat_block(C, V)
    sweep = NR * ty
    sweeps = max(1, min(16, (M * gy) // (sweep * 2048)))
    RB = sweeps * sweep
    return tx, ty, cdiv(M, RB), gy, RB, sweeps


def small_path(rows, M, C):
    return int(0 < rows <= kSmallMaxPartials and M * C <= kSmallMaxElements)


def fin_lanes(rows):
    return kFinLanesWide if rows >= kFinWideRows else kFinLanes


def finalize_workspace_bytes(rows, C):
    return 3 * cdiv(rows, kMergePer) * C * 4 if rows > kTwoStageRows else 0


def bwd_nr(dtype):
    return 2 if dtype == 'h' else 4


def bwd_mode(act, mask, z):
    return 0 if act == NONE else (1 if mask else (2 if z else 3))


# ------------------------------------------------------------------------------------------------ records
def _h(dtype):
    return int(dtype == 'h')


def rec_col_stats(dtype, M, C, shifted=1, lanes=0):
    R = stat_group(M, C)
    tx, ty, gy = stat_block(C, 4)
    return (COL_STATS, _h(dtype), 4, 4, shifted, lanes, tx, ty, cdiv(M, R), gy, R, 0)


def rec_col_sum(dtype, M, C):
    return rec_col_stats(dtype, M, C, 0, fin_lanes(stat_rows(M, C)))


def rec_reduce(dtype, M, C, mode):
    V, R = lane_channels(dtype), stat_group(M, C)
    tx, ty, gy = stat_block(C, V)
    return (BWD_REDUCE, _h(dtype), V, bwd_nr(dtype), mode, 0, tx, ty, cdiv(M, R), gy, R, 0)


def rec_apply(dtype, M, C, mode):
    V = lane_channels(dtype)
    tx, ty, gx, gy, RB, _ = row_block(M, C, V, bwd_nr(dtype))
    return (BWD_APPLY, _h(dtype), V, bwd_nr(dtype), mode, 0, tx, ty, gx, gy, RB, 0)


def fwd_takes_rows_kernel(dtype, M, coeffs, residual):
    return dtype == 'h' and coeffs and M >= 256 and not residual


def rec_act_fwd(dtype, M, C, coeffs=True, residual=False):
    V = lane_channels(dtype)
    if fwd_takes_rows_kernel(dtype, M, coeffs, residual):
        tx, ty, gx, gy, RB, _ = row_block(M, C, V, 4)
        return (ACT_FWD_ROWS, 1, V, 4, 0, 0, tx, ty, gx, gy, RB, 0)
    return (ACT_FWD, _h(dtype), V, 1, 0, 0, 256, 1, ew_grid(M * (C // V)), 1, 0, 0)


def rec_act_bwd(dtype, M, C, act):
    return (ACT_BWD, _h(dtype), 4, 1, 0 if act == NONE else 2, 0, 256, 1, ew_grid(M * (C // 4)), 1, 0, 0)


def rec_copy2d(dtype, M, C):
    return (COPY2D, _h(dtype), 4, 1, 0, 0, 256, 1, ew_grid(M * (C // 4)), 1, 0, 0)


def rec_fwd_small(dtype, M, C):
    return (FWD_SMALL, _h(dtype), 4, 1, 0, kFinLanes, 256, 1, cdiv(M, kSmallRowsPerBlock), cdiv(C, kSmallCh), kSmallRowsPerBlock, 0)


def rec_bwd_small(dtype, M, C, mode):
    return (BWD_SMALL, _h(dtype), 4, 1, mode, kFinLanes, 256, 1, cdiv(M, kSmallRowsPerBlock), cdiv(C, kSmallCh), kSmallRowsPerBlock, 0)


def rec_finalize(rows, C):
    two = int(rows > kTwoStageRows)
    r = cdiv(rows, kMergePer) if two else rows
    lanes = fin_lanes(r)
    return (FINALIZE, 0, 1, 4, 0, lanes, kFinCh * lanes, 1, cdiv(C, kFinCh), 1, r, two)


def rec_bwd_finalize(rows, C):
    lanes = fin_lanes(rows)
    return (BWD_FINALIZE, 0, 1, 4, 0, lanes, kFinCh * lanes, 1, cdiv(C, kFinCh), 1, rows, 0)


def rec_eval_coeffs(C):
    return (EVAL_COEFFS, 0, 1, 1, 0, 0, 256, 1, cdiv(C, 256), 1, 0, 0)


# ------------------------------------------------------------------------------------------------ what is compiled
# written out from the dispatch code of norm_act.hip; an instance is the tuple of template arguments, the storage type as 0 / 1
COL_STATS_COMPILED = {(shifted, half) for shifted in (0, 1) for half in (0, 1)}                  # <SHIFTED, T>
# PSEG_BWD_REDUCE(MODE): <MODE, V == 8 ? 2 : 4, T, V>; PSEG_BWD_APPLY(MODE): <MODE, kNR, T, V> with the same NR
BWD_REDUCE_COMPILED = {(mode, 4, 0, 4) for mode in range(4)} | {(mode, 2, 1, 8) for mode in range(4)}
BWD_APPLY_COMPILED = set(BWD_REDUCE_COMPILED)
FINALIZE_COMPILED = {kFinLanes, kFinLanesWide}                                                    # <LANES>
BWD_FINALIZE_COMPILED = {kFinLanes, kFinLanesWide}
COL_REDUCE_COMPILED = {kFinLanes, kFinLanesWide}
ACT_FWD_COMPILED = {(0, 4), (1, 8)}                                                               # <T, V>
ACT_FWD_ROWS_COMPILED = {(4, 1, 8)}                                                               # <kNR, T, V>: fp16 only
ACT_BWD_COMPILED = {0, 1}                                                                         # <T>
COPY2D_COMPILED = {0, 1}
FWD_SMALL_COMPILED = {0, 1}
BWD_SMALL_COMPILED = {0, 1}
STAT_MERGE_COMPILED = {()}                                                                        # not a template
EVAL_COEFFS_COMPILED = {()}
COMPILED = {COL_STATS: COL_STATS_COMPILED, BWD_REDUCE: BWD_REDUCE_COMPILED, STAT_MERGE: STAT_MERGE_COMPILED,
            FINALIZE: FINALIZE_COMPILED, BWD_FINALIZE: BWD_FINALIZE_COMPILED, COL_REDUCE: COL_REDUCE_COMPILED,
            EVAL_COEFFS: EVAL_COEFFS_COMPILED, ACT_FWD: ACT_FWD_COMPILED, ACT_FWD_ROWS: ACT_FWD_ROWS_COMPILED,
            BWD_APPLY: BWD_APPLY_COMPILED, ACT_BWD: ACT_BWD_COMPILED, COPY2D: COPY2D_COMPILED, FWD_SMALL: FWD_SMALL_COMPILED,
            BWD_SMALL: BWD_SMALL_COMPILED}
BLOCK_SHAPES = {(8, 32), (16, 16), (32, 8), (64, 4)}


def instance(rec):
    """the compiled instance a record names"""
    k, half, V, NR, mode, lanes = rec[:6]
    if k == COL_STATS:
        return (mode, half)
    if k in (BWD_REDUCE, BWD_APPLY):
        return (mode, NR, half, V)
    if k in (FINALIZE, BWD_FINALIZE, COL_REDUCE):
        return lanes
    if k == ACT_FWD:
        return (half, V)
    if k == ACT_FWD_ROWS:
        return (NR, half, V)
    if k in (ACT_BWD, COPY2D, FWD_SMALL, BWD_SMALL):
        return half
    return ()


def launches(row):
    """every record a row asserts: those of its chained launches and the last one; a two-stage finalize and a column sum also ran
    the kernel their record points to (stat_merge_kernel; col_reduce_kernel with the record's LANES)"""
    recs = list(row.flags.get('records', ())) + [row.record]
    out = []
    for r in recs:
        out.append((r[0], instance(r)))
        if r[0] == FINALIZE and r[11]:
            out.append((STAT_MERGE, ()))
        if r[0] == COL_STATS and r[4] == 0:
            out.append((COL_REDUCE, r[5]))
    return out


# ------------------------------------------------------------------------------------------------ the rows
# Channel counts that take each block shape of stat_block (cv = C / V: <= 8 -> 8x32, <= 16 -> 16x16, < 64 -> 32x8, else 64x4), each
# off a multiple of tx * V so that the last column block is ragged; M = 300: a ragged last row group at R = 32 and a ragged last
# NR x TY sweep.
BLOCK_C = {'f': (12, 36, 68, 260), 'h': (24, 72, 136, 520)}
MASK_C = (32, 288)                       # C % 32 == 0: one mask word per row, and nine
STAT_M = (1, 31, 33, 300, 1581)
M0 = 300
DTYPES = ('f', 'h')

ROWS = []


def _add(id, entry, dtype, M, C, record, ld=None, **flags):
    ROWS.append(Row(id, entry, dtype, M, C, ld, flags, record))


# ---- col_stats / col_sum: pseg_col_stats(_h), pseg_col_sum(_h).  The statistics kernel works in 4-channel lanes for both types.
for _t in DTYPES:
    for _C in BLOCK_C[_t] + ((40,) if _t == 'h' else ()):           # (fp16 at V = 4: 40 channels for the 16x16 block, at 300 and 1581 rows)
        for _i, _M in enumerate(STAT_M if _C != 40 else STAT_M[3:]):            # (both entry points on one operand: the statistics first, the column sum last)
            _add('col-%s-M%d-C%d' % (_t, _M, _C), 'col_both', _t, _M, _C, rec_col_sum(_t, _M, _C), accumulate=(_i + _C // 4) % 2,
                 records=(rec_col_stats(_t, _M, _C),))
# col_reduce_kernel at 1, 127, 128, 131 and 2048 partial rows; the last group short.  stat_group shrinks the groups until there are
# 1024 of them, so 2048 partial rows need groups of kMaxStatRows: 2^20 pixels, here of 4 channels
for _i, (_rows, _R, _C) in enumerate(((1, 32, 12), (127, 32, 12), (128, 32, 12), (131, 32, 12), (2048, 512, 4))):
    _M = _rows * _R - 5
    _add('col_sum-f-rows%d-C%d' % (_rows, _C), 'col_sum', 'f', _M, _C, rec_col_sum('f', _M, _C), accumulate=_i % 2, rows=_rows)

# ---- forward: pseg_bn_act_fwd(_h)
#  fp32: bn_act_fwd_kernel with / without residual, with / without coefficients, with amax_z, with mask_out
#  fp16: bn_act_fwd_rows_kernel (M >= 256, coefficients, no residual), else the streaming kernel (residual; M = 255; no coefficients)
_FWD = [  # (suffix, coeffs, residual, act, amax, mask)
    ('bn-relu6', True, False, RELU6, False, False), ('bn-res-relu', True, True, RELU, False, False),
    ('bn-none-amax', True, False, NONE, True, False), ('act-only-relu6', False, False, RELU6, False, False),
    ('res-add-only', False, True, NONE, False, False), ('bn-res-relu6-amax', True, True, RELU6, True, False)]
for _t in DTYPES:
    for _j, _C in enumerate(BLOCK_C[_t]):
        for _k, (_sfx, _co, _res, _act, _amax, _mask) in enumerate(_FWD):
            if _t == 'h' and _amax:
                continue                                              # (no amax_z argument on the fp16 entry point)
            # three of the six forms per block shape in fp32; in fp16 the rows-kernel form on every shape and one of the others
            if (_k not in ((0, 1, 2), (3, 4, 5), (0, 2, 4), (1, 3, 5))[_j]) if _t == 'f' else (_k != 0 and _k != (1, 3, 4)[_j % 3]):
                continue
            _add('fwd-%s-C%d-%s' % (_t, _C, _sfx), 'fwd', _t, M0, _C, rec_act_fwd(_t, M0, _C, _co, _res), coeffs=_co, residual=_res,
                 act=_act, amax=_amax, mask=_mask)
    for _C in MASK_C:
        for _res, _act in ((False, RELU6), (True, RELU)):
            _add('fwd-%s-C%d-mask%s' % (_t, _C, '-res' if _res else ''), 'fwd', _t, M0, _C, rec_act_fwd(_t, M0, _C, True, _res),
                 coeffs=True, residual=_res, act=_act, amax=_t == 'f', mask=True)
_add('fwd-h-M255-C72', 'fwd', 'h', 255, 72, rec_act_fwd('h', 255, 72), coeffs=True, residual=False, act=RELU6, amax=False, mask=False)
_add('fwd-h-M256-C72', 'fwd', 'h', 256, 72, rec_act_fwd('h', 256, 72), coeffs=True, residual=False, act=RELU6, amax=False, mask=False)

# ---- backward, the two-pass chain: pseg_bn_act_bwd_reduce(_h) -> pseg_bn_bwd_finalize -> pseg_bn_act_bwd_apply(_h)
#  MODE 0 no activation, 1 the bitmask bn_act_fwd wrote in the same test (C % 32 == 0; with a residual), 2 the stored z (with a
#  residual), 3 recomputed from y (no residual).  dres / res_accumulate / dgamma-dbeta accumulate / frozen / limb planes cycle over
#  the rows; tests/test_norm_instances_cpu.py holds that every one of them is set and cleared somewhere on every mode.
def _bwd_flags(i, dtype, C):
    dres = i % 3 != 0
    return dict(dres=dres, res_accumulate=dres and i % 2 == 1, accumulate=i % 4 >= 2, frozen=i % 5 == 4,
                planes=dtype == 'f' and C % 8 == 0 and i % 2 == 0)


_i = 0
for _t in DTYPES:
    for _mode in range(4):
        # (MODE 1 on the 64x4 block: 288 channels in 4-channel lanes, 544 in 8-channel ones)
        for _C in (MASK_C + ((544,) if _t == 'h' else (64,)) if _mode == 1 else BLOCK_C[_t] + (MASK_C[1],)):
            # (ReLU and ReLU6 on the mask rows and on the widest block; elsewhere they alternate)
            for _act in ((NONE,) if _mode == 0 else (RELU, RELU6) if _C % 32 == 0 else ((RELU6, RELU)[(_C // 4) % 2],)):
                _add('bwd-%s-mode%d-C%d-act%d' % (_t, _mode, _C, _act), 'bwd', _t, M0, _C, rec_apply(_t, M0, _C, _mode), mode=_mode,
                     act=_act, records=(rec_reduce(_t, M0, _C, _mode), rec_bwd_finalize(stat_rows(M0, _C), _C)),
                     **_bwd_flags(_i, _t, _C))
                _i += 1

# ---- the fused small-tensor kernels, called directly: pseg_bn_fwd_fused(_h), pseg_bn_bwd_fused(_h), each beside the two-launch
#  chain on the same inputs.  C = 12 and 68 (ragged against kSmallCh = 64), 1 and 64 partial rows (the cap; groups past the last
#  pixel row are empty and hold NaN), M on both sides of kSmallRowsPerBlock.
_i = 0
for _t in DTYPES:
    for _M in (1, 63, 65, 300):
        for _C in (12, 68):
            for _rows in (1, 64):
                _act = (RELU6, RELU, NONE)[_i % 3]
                _z = _i % 2 == 0                                     # z given (with a residual) or the mask recomputed from y
                _mode = bwd_mode(_act, False, _z)
                _add('fused-%s-M%d-C%d-rows%d' % (_t, _M, _C, _rows), 'fused', _t, _M, _C, rec_bwd_small(_t, _M, _C, _mode), rows=_rows,
                     act=_act, residual=_z, running=_i % 4 < 2, frozen=_i % 8 == 5, accumulate=_i % 4 in (1, 2), dres=_i % 3 != 2,
                     res_accumulate=_i % 3 == 1, amax=_t == 'f' and _i % 2 == 1, mode=_mode,
                     records=(rec_fwd_small(_t, _M, _C),))
                _i += 1

# fp16 at 72 channels: C % 8 == 0, so that the two-pass fp16 kernels (8-channel lanes) run beside the fused ones, still ragged against
# kSmallCh
for _M, _rows, _act, _z in ((300, 64, RELU6, True), (65, 1, RELU, False)):
    _mode = bwd_mode(_act, False, _z)
    _add('fused-h-M%d-C72-rows%d' % (_M, _rows), 'fused', 'h', _M, 72, rec_bwd_small('h', _M, 72, _mode), rows=_rows, act=_act, residual=_z,
         running=True, frozen=False, accumulate=_z, dres=True, res_accumulate=_z, amax=False, mode=_mode,
         records=(rec_fwd_small('h', _M, 72),))

# ---- the finalize kernels on synthetic partials: pseg_bn_finalize, pseg_bn_bwd_finalize.  C = 12 (ragged against kFinCh = 8),
#  groups of 32 rows, the last one short by 7; 2049 and 2049 + 64 * 3 + 5 partial rows: two stages, the last merge block ragged.
for _i, _rows in enumerate((1, 127, 128, 131, 2048, 2049, 2049 + 64 * 3 + 5)):
    _add('finalize-rows%d' % _rows, 'finalize', 'f', _rows * 32 - 7, 12, rec_finalize(_rows, 12), rows=_rows, group=32,
         running=_i % 2 == 0, affine=_i % 3 != 1)
_add('finalize-count1', 'finalize', 'f', 1, 12, rec_finalize(1, 12), rows=1, group=32, running=True, affine=True)
for _i, _rows in enumerate((1, 127, 128, 131, 2048)):
    _add('bwd_finalize-rows%d' % _rows, 'bwd_finalize', 'f', _rows * 32 - 7, 12, rec_bwd_finalize(_rows, 12), rows=_rows,
         accumulate=_i % 2 == 1, frozen=_i == 2, grads=_i != 3)
_add('eval_coeffs-C300', 'eval_coeffs', 'f', 1, 300, rec_eval_coeffs(300))

# ---- plain activation backward and the strided copy: pseg_act_bwd(_h), pseg_copy2d(_h)
_ACT_BWD = [  # (suffix, act, scale, dy, dres, res_accumulate)
    ('relu6-scale-dres', RELU6, True, True, True, False), ('relu-dres-acc', RELU, False, True, True, True),
    ('none-scale', NONE, True, True, False, False), ('relu6-dres-only-acc', RELU6, False, False, True, True),
    ('relu', RELU, False, True, False, False)]
for _t in DTYPES:
    for _sfx, _act, _scale, _dy, _dres, _racc in _ACT_BWD:
        _C = 36 if _t == 'f' else 44                                   # (fp16 in 4-channel lanes: C % 8 == 4 is within the contract)
        _add('act_bwd-%s-%s' % (_t, _sfx), 'act_bwd', _t, M0, _C, rec_act_bwd(_t, M0, _C, _act), act=_act, scale=_scale, dy=_dy,
             dres=_dres, res_accumulate=_racc)
    for _M, _C, _acc in ((M0, 12, False), (M0, 12, True), (1, 260, True), (1581, 36, False)):
        _add('copy2d-%s-M%d-C%d%s' % (_t, _M, _C, '-acc' if _acc else ''), 'copy2d', _t, _M, _C, rec_copy2d(_t, _M, _C), accumulate=_acc)

# ---- grid-stride and multi-sweep: one fp32 row each, the largest of the table (fp64 reference with torch on the device)
BIG_EW_M = 65537                          # x 32 channels: 524 296 four-channel lane items, eight past the 2048 x 256 a launch holds
BIG_APPLY_M = 2 * 128 * 2048 + 37         # x 32 channels in an 8 x 32 block: sweeps = 2 of 128 rows, a ragged last block of 37 rows
_add('fwd-f-grid-stride', 'fwd', 'f', BIG_EW_M, 32, rec_act_fwd('f', BIG_EW_M, 32, True, True), coeffs=True, residual=True, act=RELU6,
     amax=True, mask=True, big=True)
_add('act_bwd-f-grid-stride', 'act_bwd', 'f', BIG_EW_M, 32, rec_act_bwd('f', BIG_EW_M, 32, RELU6), act=RELU6, scale=True, dy=True,
     dres=True, res_accumulate=True, big=True)
_add('copy2d-f-grid-stride', 'copy2d', 'f', BIG_EW_M, 32, rec_copy2d('f', BIG_EW_M, 32), accumulate=True, big=True)
# the fp16 forward-rows kernel sizes its row blocks the same way: 8 channels (one lane column of the 8 x 32 block), sweeps = 2
_add('fwd-h-rows-two-sweeps', 'fwd', 'h', BIG_APPLY_M, 8, rec_act_fwd('h', BIG_APPLY_M, 8), coeffs=True, residual=False, act=RELU6,
     amax=False, mask=False, big=True)
_add('apply-f-two-sweeps', 'apply_only', 'f', BIG_APPLY_M, 32, rec_apply('f', BIG_APPLY_M, 32, 3), mode=3, act=RELU, dres=True,
     res_accumulate=False, big=True)

# ---- sliced operands: every activation operand a channel slice of a wider buffer, a different ld per operand (multiples of 4 /
#  8 elements, slices 16-byte aligned), NaN around the slices.  The second operand's slice is the LAST columns of its buffer (the
#  byte range of a buffer resource ends where the buffer does), the fourth's the first.
def _lds(dtype, C, names):
    q = 8 if dtype == 'h' else 4
    first = (1, 4, 3, 0, 2, 2)
    Cq = cdiv(C, q) * q
    return {n: (Cq + q * (2 * i + 2), q * first[i]) for i, n in enumerate(names)}


for _t in DTYPES:
    _C = 36 if _t == 'f' else 72
    _Cm = 32
    _add('sliced-col_stats-%s' % _t, 'col_stats', _t, M0, _C, rec_col_stats(_t, M0, _C), _lds(_t, _C, ('y',)))
    _add('sliced-col_sum-%s' % _t, 'col_sum', _t, M0, _C, rec_col_sum(_t, M0, _C), _lds(_t, _C, ('y',)), accumulate=1)
    _add('sliced-fwd-%s' % _t, 'fwd', _t, M0, _Cm, rec_act_fwd(_t, M0, _Cm, True, True), _lds(_t, _Cm, ('y', 'residual', 'z')), coeffs=True,
         residual=True, act=RELU6, amax=False, mask=True)
    if _t == 'h':
        _add('sliced-fwd-rows-h', 'fwd', 'h', M0, _C, rec_act_fwd('h', M0, _C), _lds('h', _C, ('y', 'residual', 'z')), coeffs=True,
             residual=False, act=RELU6, amax=False, mask=False)
    for _mode, _Cb in ((2, _C), (1, _Cm), (3, _C)):
        _add('sliced-bwd-%s-mode%d' % (_t, _mode), 'bwd', _t, M0, _Cb, rec_apply(_t, M0, _Cb, _mode),
             _lds(_t, _Cb, ('y', 'residual', 'z', 'dz', 'dy', 'dres')), mode=_mode, act=RELU6, dres=True, res_accumulate=_mode == 2,
             accumulate=False, frozen=False, planes=False,
             records=(rec_reduce(_t, M0, _Cb, _mode), rec_bwd_finalize(stat_rows(M0, _Cb), _Cb)))
    _add('sliced-fused-%s' % _t, 'fused', _t, M0, 68, rec_bwd_small(_t, M0, 68, 2), _lds(_t, 68, ('y', 'residual', 'z', 'dz', 'dy', 'dres')),
         rows=10, act=RELU6, residual=True, running=True, frozen=False, accumulate=True, dres=True, res_accumulate=True, amax=False,
         mode=2, records=(rec_fwd_small(_t, M0, 68),))
    _add('sliced-act_bwd-%s' % _t, 'act_bwd', _t, M0, _C, rec_act_bwd(_t, M0, _C, RELU6), _lds(_t, _C, ('dz', 'z', 'dy', 'dres')), act=RELU6,
         scale=True, dy=True, dres=True, res_accumulate=True)
    _add('sliced-copy2d-%s' % _t, 'copy2d', _t, M0, _C, rec_copy2d(_t, M0, _C), _lds(_t, _C, ('x', 'y')), accumulate=True)

BY_ID = {r.id: r for r in ROWS}

# ------------------------------------------------------------------------------------------------ refusals
# argument checks run before any launch: these need no device.  'A' stands for a 16-byte aligned made-up device address.
A = 'A'
REFUSALS = [
    # C % 8 == 4 on the fp16 entry points whose kernels work in 8-channel lanes (the last lane would run four channels past C)
    Refusal('fwd_h-C12', 'pseg_bn_act_fwd_h', (A, 16, A, A, A, None, 0, RELU, A, 16, 64, 12, None, None), ERR_ARG, 'C % 8 == 0'),
    Refusal('reduce_h-C12', 'pseg_bn_act_bwd_reduce_h', (A, 16, None, 0, A, 16, A, A, A, A, RELU, 64, 12, A, A, None, None), ERR_ARG,
            'C % 8 == 0'),
    Refusal('apply_h-C12', 'pseg_bn_act_bwd_apply_h', (A, 16, None, 0, A, 16, A, A, A, A, A, A, RELU, A, 16, None, 0, 0, 64, 12, None, None),
            ERR_ARG, 'C % 8 == 0'),
    # the fused kernels take at most kSmallMaxPartials partial rows
    Refusal('fwd_fused-rows65', 'pseg_bn_fwd_fused', (A, 65, 32, 65 * 32, 12, A, A, None, None, 0.1, 1e-5, A, A, A, A, A, 12, None, 0, RELU,
                                                      A, 12, 65 * 32, None, None), ERR_ARG, 'rows 65'),
    Refusal('fwd_fused_h-rows65', 'pseg_bn_fwd_fused_h', (A, 65, 32, 65 * 32, 16, A, A, None, None, 0.1, 1e-5, A, A, A, A, A, 16, None, 0, RELU,
                                                          A, 16, 65 * 32, None), ERR_ARG, 'rows 65'),
    Refusal('fwd_fused-uncovered', 'pseg_bn_fwd_fused', (A, 4, 32, 129, 12, A, A, None, None, 0.1, 1e-5, A, A, A, A, A, 12, None, 0, RELU,
                                                         A, 12, 129, None, None), ERR_ARG, 'do not cover'),
    # workspaces one float short
    Refusal('finalize-short-workspace', 'pseg_bn_finalize', (A, 2049, 32, 2049 * 32 - 7, 12, None, None, None, None, 0.1, 1e-5, A, A, A, A, A,
                                                             finalize_workspace_bytes(2049, 12) - 4, None), ERR_WORKSPACE, 'workspace'),
    Refusal('finalize-no-workspace', 'pseg_bn_finalize', (A, 2049, 32, 2049 * 32 - 7, 12, None, None, None, None, 0.1, 1e-5, A, A, A, A, None,
                                                          0, None), ERR_WORKSPACE, 'workspace'),
    Refusal('col_sum-short-workspace', 'pseg_col_sum', (A, 12, M0, 12, A, 0, A, stat_rows(M0, 12) * 12 * 4 - 4, None), ERR_WORKSPACE,
            'workspace'),
    Refusal('col_sum_h-short-workspace', 'pseg_col_sum_h', (A, 24, M0, 24, A, 0, A, stat_rows(M0, 24) * 24 * 4 - 4, None), ERR_WORKSPACE,
            'workspace'),
    # masks need whole words; limb planes a dense dy; ld a multiple of 8 for fp16
    Refusal('reduce-mask-C36', 'pseg_bn_act_bwd_reduce', (A, 36, None, 0, A, 36, A, A, A, A, RELU, 64, 36, A, A, A, None), ERR_ARG, 'C % 32'),
    Refusal('copy2d_h-ld12', 'pseg_copy2d_h', (A, 12, A, 16, 64, 8, 0, None), ERR_ARG, 'alignment'),
    Refusal('act_bwd-no-z', 'pseg_act_bwd', (A, 12, None, 0, None, RELU, A, 12, None, 0, 0, 64, 12, None), ERR_ARG, 'needs z'),
]
