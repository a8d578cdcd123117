"""The case table of tests/test_norm_instances_gpu.py reaches what it claims -- shown without a GPU.

Over tests/norm_cases.py:
(a) every compiled instance of every __global__ function of csrc/norm_act.hip (the *_COMPILED sets, written out from the dispatch
    code and held against the source here) is launched by at least one row, and no row names an instance that is not compiled;
(b) every block shape of stat_block is taken by the reduce and the apply kernel in both storage types and by the statistics
    kernel, and the host branches the issue names are reached: two-stage merge, grid stride, sweeps > 1, both finalize widths;
(c) every refusal row is refused by the entry point's argument checks, which run before any launch;
(d) pseg_debug_last_norm answers zeros on a thread that has launched nothing and refuses a null pointer;
(e) the Python mirror of stat_group and pseg_bn_small_path agrees with the library's own queries over a sweep of (M, C)."""
import ctypes
import os
import re
import threading

import pytest

import norm_cases as nc
from pytorch_segmentation_amd import _lib
from pytorch_segmentation_amd.csrc import build as csrc_build

HERE = os.path.dirname(os.path.abspath(__file__))
FAKE = 0x7f0000000000                       # a 16-byte aligned made-up device address: never dereferenced by an argument check


@pytest.fixture(scope='module')
def lib():
    csrc_build.build(verbose=False)
    return _lib.load()


def hit_instances(rows):
    hit = {}
    for row in rows:
        for kernel, inst in nc.launches(row):
            hit.setdefault(kernel, set()).add(inst)
    return hit


def test_rows_are_well_formed():
    ids = [r.id for r in nc.ROWS]
    assert len(set(ids)) == len(ids)
    for row in nc.ROWS:
        q = 8 if row.dtype == 'h' else 4
        assert len(row.record) == len(nc.FIELDS) == 12, row.id
        assert row.dtype in nc.DTYPES and row.M > 0 and row.C % 4 == 0, row.id
        for rec in list(row.flags.get('records', ())) + [row.record]:
            assert len(rec) == 12 and rec[1] in (0, 1), row.id
        if row.ld:
            for name, (ld, c0) in row.ld.items():
                assert ld % q == 0 and c0 % q == 0 and c0 + row.C <= ld and ld > row.C, (row.id, name)
            assert len({ld for ld, _ in row.ld.values()}) == len(row.ld), row.id          # a different ld per operand


def test_every_compiled_instance_is_hit():
    """(a), and that the check has teeth: without its only row an instance goes missing"""
    hit = hit_instances(nc.ROWS)
    for kernel, compiled in nc.COMPILED.items():
        got = hit.get(kernel, set())
        assert got <= compiled, '%s: rows name instances that are not compiled: %s' % (nc.KERNEL_NAMES[kernel], sorted(got - compiled))
        assert got == compiled, '%s: no row reaches %s' % (nc.KERNEL_NAMES[kernel], sorted(compiled - got, key=str))
    two_stage = [r for r in nc.ROWS if r.record[0] == nc.FINALIZE and r.record[11]]
    assert len(two_stage) == 2
    thinned = [r for r in nc.ROWS if r not in two_stage]
    assert nc.STAT_MERGE not in hit_instances(thinned)
    only_rows_kernel = [r for r in nc.ROWS if r.record[0] != nc.ACT_FWD_ROWS]
    assert nc.ACT_FWD_ROWS not in hit_instances(only_rows_kernel)


def test_compiled_sets_restate_the_source():
    src = open(os.path.join(os.path.dirname(HERE), 'pytorch_segmentation_amd', 'csrc', 'norm_act.hip')).read()
    globals_ = re.findall(r'__global__[^\n]*?void (\w+)\(', src)
    assert sorted(globals_) == sorted(nc.KERNEL_NAMES.values()), globals_
    # the enum of the record, in order
    enum = re.search(r'enum NormKernel \{(.*?)\};', src, re.S).group(1)
    names = [n.strip().split(' ')[0] for n in enum.replace('\n', ' ').split(',')]
    assert names == ['kNormColStats', 'kNormBwdReduce', 'kNormStatMerge', 'kNormFinalize', 'kNormBwdFinalize', 'kNormColReduce',
                     'kNormEvalCoeffs', 'kNormActFwd', 'kNormActFwdRows', 'kNormBwdApply', 'kNormActBwd', 'kNormCopy2d', 'kNormFwdSmall',
                     'kNormBwdSmall'] and 'kNormColStats = 1' in enum
    # the dispatch: four modes of reduce and apply, NR by lane width; two finalize widths; constants
    assert [int(m) for m in re.findall(r'PSEG_BWD_REDUCE\(\s*(\d)\s*\)\s*;', src)] == [0, 1, 2, 3]
    assert [int(m) for m in re.findall(r'PSEG_BWD_APPLY\(\s*(\d)\s*\)\s*;', src)] == [0, 1, 2, 3]
    flat = re.sub(r'\s+', '', src)           # (spacing and line breaks of the source are free)
    assert 'bn_bwd_reduce_kernel<MODE,(V==8?2:4),T,V>' in flat and re.search(r'constexprintkNR=V==8\?2:4;', flat)
    assert re.search(r'lane_channels\(\)\{returnsizeof\(T\)==2\?8:4;\}', flat)
    for name in ('kMaxStatRows', 'kFinCh', 'kFinLanes', 'kFinLanesWide', 'kFinWideRows', 'kMergePer', 'kTwoStageRows', 'kSmallCh',
                 'kSmallRowsPerBlock', 'kSmallMaxPartials'):
        assert re.search(r'\b%s\s*=\s*%d\b' % (name, getattr(nc, name)), src), name
    assert '<=(int64_t)(8<<20)' in flat and nc.kSmallMaxElements == 8 << 20
    assert re.search(r'if\(b>256\*8\)b=256\*8;', flat) and nc.kEwMaxBlocks == 2048
    header = open(os.path.join(os.path.dirname(HERE), 'include', 'pseg_amd.h')).read()
    assert re.search(r'int\s+pseg_debug_last_norm\(\s*int\s*\*\s*out12\s*\)\s*;', header)
    for code, name in nc.KERNEL_NAMES.items():
        assert re.search(r'\b%d %s\b' % (code, name), header), name


def test_block_shapes_and_host_branches_are_reached():
    """(b)"""
    for kernel in (nc.BWD_REDUCE, nc.BWD_APPLY):
        for half in (0, 1):
            seen = {rec[6:8] for row in nc.ROWS for rec in list(row.flags.get('records', ())) + [row.record]
                    if rec[0] == kernel and rec[1] == half}
            assert seen == nc.BLOCK_SHAPES, (nc.KERNEL_NAMES[kernel], half, seen)
            for mode in range(4):
                assert any(rec[0] == kernel and rec[1] == half and rec[4] == mode and rec[6:8] == (64, 4)
                           for row in nc.ROWS for rec in list(row.flags.get('records', ())) + [row.record]), (kernel, half, mode)
    for half in (0, 1):
        for shifted in (0, 1):
            seen = {rec[6:8] for r in nc.ROWS for rec in list(r.flags.get('records', ())) + [r.record]
                    if rec[0] == nc.COL_STATS and rec[1] == half and rec[4] == shifted}
            assert seen == nc.BLOCK_SHAPES, (half, shifted, seen)
    assert {r.record[6:8] for r in nc.ROWS if r.record[0] == nc.ACT_FWD_ROWS} == nc.BLOCK_SHAPES
    # the fp16 statistics kernel: 4-channel lanes
    assert all(r.record[2] == 4 for r in nc.ROWS if r.record[0] == nc.COL_STATS)
    # ragged against the block: the last column block and the last row group / sweep of the M = 300 rows
    for t in nc.DTYPES:
        V = nc.lane_channels(t)
        for C in nc.BLOCK_C[t]:
            tx, ty, _ = nc.stat_block(C, V)
            assert (C // V) % tx != 0 and nc.M0 % nc.stat_group(nc.M0, C) != 0 and nc.M0 % (nc.bwd_nr(t) * ty) != 0, (t, C)
    # grid stride: more lane items than a launch holds; sweeps > 1 with a ragged tail
    for id in ('fwd-f-grid-stride', 'act_bwd-f-grid-stride', 'copy2d-f-grid-stride'):
        row = nc.BY_ID[id]
        assert row.M * (row.C // 4) == nc.kEwMaxBlocks * 256 + 8 and row.record[8] == nc.kEwMaxBlocks
    row = nc.BY_ID['apply-f-two-sweeps']
    tx, ty, gx, gy, RB, sweeps = nc.row_block(row.M, row.C, 4, 4)
    assert sweeps == 2 and RB == 256 and row.M % RB == 37 and row.record[10] == 256
    row = nc.BY_ID['fwd-h-rows-two-sweeps']
    tx, ty, gx, gy, RB, sweeps = nc.row_block(row.M, row.C, 8, 4)
    assert row.record[0] == nc.ACT_FWD_ROWS and sweeps == 2 and RB == 256 and row.M % RB == 37 and row.record[10] == 256
    # finalize: both widths on each kernel, 131 rows on the wide one (not a multiple of 128), and the two-stage merge twice, the
    # second with a ragged last merge block
    for kernel in (nc.FINALIZE, nc.BWD_FINALIZE):
        assert {(r.record[5], r.record[10]) for r in nc.ROWS if r.record[0] == kernel and r.entry in ('finalize', 'bwd_finalize')
                and not r.record[11]} >= {(32, 1), (32, 127), (128, 128), (128, 131), (128, 2048)}
    assert [(r.flags['rows'], r.record[10]) for r in nc.ROWS if r.record[0] == nc.FINALIZE and r.record[11]] == [(2049, 33), (2246, 36)]
    assert 2246 % nc.kMergePer == 6 and nc.finalize_workspace_bytes(2048, 12) == 0 and nc.finalize_workspace_bytes(2049, 12) == 3 * 33 * 48
    assert {r.record[5] for r in nc.ROWS if r.entry == 'col_sum' and 'rows' in r.flags} == {32, 128}
    for r in nc.ROWS:
        if r.entry == 'col_sum' and 'rows' in r.flags:
            assert nc.stat_rows(r.M, r.C) == r.flags['rows'], r.id
    # the arguments no operator test set: each both ways on the kernels that take it
    bwd = [r for r in nc.ROWS if r.entry == 'bwd' and not r.ld]
    for mode in range(4):
        rows = [r for r in bwd if r.flags['mode'] == mode]
        for flag in ('dres', 'res_accumulate', 'accumulate'):
            assert {bool(r.flags[flag]) for r in rows} == {False, True}, (mode, flag)
    assert {bool(r.flags['planes']) for r in bwd if r.dtype == 'f'} == {False, True} and any(r.flags['frozen'] for r in bwd)
    fused = [r for r in nc.ROWS if r.entry == 'fused']
    for flag in ('running', 'frozen', 'accumulate', 'res_accumulate', 'dres', 'residual', 'amax'):
        assert {bool(r.flags[flag]) for r in fused} == {False, True}, flag
    assert {r.flags['mode'] for r in fused} == {0, 2, 3} and {r.flags['rows'] for r in fused if not r.ld} == {1, 64}
    # both chains in full for fp16 too: C % 8 == 0 and still ragged against kSmallCh
    assert any(r.dtype == 'h' and r.C % 8 == 0 and r.C % nc.kSmallCh != 0 for r in fused)
    assert any(r.flags['res_accumulate'] and r.flags['dres'] for r in fused)
    act_bwd = [r for r in nc.ROWS if r.entry == 'act_bwd']
    assert {(r.dtype, bool(r.flags['scale']), bool(r.flags['dres'])) for r in act_bwd} >= {(t, s, d) for t in nc.DTYPES for s in (False, True)
                                                                                              for d in (False, True)}
    # every kernel that takes activations has a sliced row per storage type
    for t in nc.DTYPES:
        assert {r.entry for r in nc.ROWS if r.ld and r.dtype == t} == {'col_stats', 'col_sum', 'fwd', 'bwd', 'fused', 'act_bwd', 'copy2d'}


NO_GPU = pytest.mark.skipif(__import__('torch').cuda.is_available(), reason='uses made-up device addresses: host-side checks only')


@NO_GPU
@pytest.mark.parametrize('ref', nc.REFUSALS, ids=[r.id for r in nc.REFUSALS])
def test_refusals(lib, ref):
    """(c): refused on the arguments alone, with the code and the message the row names.  The pointers are made-up addresses, so
    this runs only where no device could be reached should a check ever let a call through."""
    args = [FAKE if a == nc.A else a for a in ref.args]
    _, argtypes, _ = _lib.prototypes()[ref.name]
    assert len(args) == len(argtypes), ref.id
    rc = getattr(lib, ref.name)(*args)
    msg = lib.pseg_last_error().decode()
    assert rc == ref.rc and ref.match in msg, (rc, msg)


def on_fresh_thread(body):
    failures = []

    def run():
        try:
            body()
        except BaseException as e:      # (re-raised in the test's own thread)
            failures.append(e)

    t = threading.Thread(target=run)
    t.start()
    t.join()
    if failures:
        raise failures[0]


def test_record_is_zero_before_any_launch(lib):
    """(d): the record is the calling thread's: zeros on a thread that has launched nothing; a null pointer is refused"""
    def body():
        rec = (ctypes.c_int * 12)(*[7] * 12)
        assert lib.pseg_debug_last_norm(rec) == 0 and list(rec) == [0] * 12
        assert lib.pseg_debug_last_norm(None) == -1 and b'debug_last_norm' in lib.pseg_last_error()
        assert lib.pseg_debug_last_norm(rec) == 0 and list(rec) == [0] * 12

    on_fresh_thread(body)


@NO_GPU
def test_a_refused_call_leaves_the_record_alone(lib):
    def body():
        ref = nc.REFUSALS[0]
        assert getattr(lib, ref.name)(*[FAKE if a == nc.A else a for a in ref.args]) == ref.rc
        rec = (ctypes.c_int * 12)(*[7] * 12)
        assert lib.pseg_debug_last_norm(rec) == 0 and list(rec) == [0] * 12

    on_fresh_thread(body)


def test_mirror_agrees_with_the_library(lib):
    """(e): stat_group / stat_rows and the small-path rule against pseg_col_stats_group / _rows and pseg_bn_small_path"""
    Ms = [1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 300, 1023, 1024, 1581, 4096, 16383, 16384, 32769, 65536, 65537, 131072, 262144, 524288,
          524325, 1 << 20, (1 << 22) + 3]
    Cs = [4, 8, 12, 24, 32, 36, 64, 68, 72, 128, 136, 256, 260, 288, 512, 520, 1024, 2048]
    for M in Ms:
        for C in Cs:
            assert lib.pseg_col_stats_group(M, C) == nc.stat_group(M, C), (M, C)
            assert lib.pseg_col_stats_rows(M, C) == nc.stat_rows(M, C), (M, C)
            for rows in (0, 1, 63, 64, 65, nc.stat_rows(M, C)):
                assert lib.pseg_bn_small_path(rows, M, C) == nc.small_path(rows, M, C), (rows, M, C)
    assert nc.small_path(64, 1 << 20, 8) == 1 and nc.small_path(64, (1 << 20) + 1, 8) == 0
    for rows in (1, 2048, 2049, 2246, 16384):
        assert lib.pseg_bn_finalize_workspace_bytes(rows, 12) == nc.finalize_workspace_bytes(rows, 12)
