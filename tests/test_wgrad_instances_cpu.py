"""The case tables of tests/test_wgrad_instances_gpu.py reach what they claim -- shown without a GPU, through the pure queries
pseg_conv2d_wgrad_choice / pseg_conv2d_wgrad_choice_h, which read the selection the launches read (select_wgrad, select_wgrad_h).

Every row of tests/wgrad_cases.py must select the (kernel, tile, pixels per K-step, SKIP, pixel order, patch shape, splits) it
names, and over the whole table:

(a) every REACHABLE instantiation of wgrad_h_kernel is hit.  It is instantiated 20 times (kHWgradTiles x SKIP x 32 | 64 pixels per
    K-step).  SKIP needs kh * kw > 1 and Cin % tile columns == 0 (wgrad_pixel_order), hence K >= 4 * tile columns, while pick_tile
    gives the 64-column tile to K <= 64 and the 32-column tile to K <= 32 only: wgrad_h_kernel<128, 64, ..., SKIP = true> and
    <128, 32, ..., SKIP = true>, each with 32 and with 64 pixels per K-step, are compiled and cannot be selected by any shape.
    Sixteen remain, and the table hits exactly those.
(b) every reachable instantiation of wgrad_f32_dma_kernel is hit: kWgradDmaTiles x skip is nine, <128, 64, ..., SKIP = true> is
    unreachable by the same argument, eight remain; and every pixel order appears on each exact-fp32 kernel family that can run
    it (LDS-DMA: dense, dead patches skipped, packed, row-major; register-staged: dense, dead rows skipped, dead patches skipped).

The evidence for "unreachable" is a brute-force grid -- 33 x 33 channel counts, 1x1 / 3x3 / 7x7, dilation 1 / 6, three maps --
over which no shape selects an instantiation outside the expected sets."""
import ctypes
import itertools
import os
import re

import pytest

import wgrad_cases as wc
from pytorch_segmentation_amd import _lib
from pytorch_segmentation_amd.csrc import build as csrc_build

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def lib():
    csrc_build.build(verbose=False)
    return _lib.load()


@pytest.fixture
def plain_env(monkeypatch):
    """none of the rows' switches set from outside; the library re-reads them before and after"""
    for name in wc.SWITCHES:
        monkeypatch.delenv(name, raising=False)
    _lib.clear_query_cache()
    yield monkeypatch
    monkeypatch.undo()
    _lib.clear_query_cache()


def chosen(lib, row, monkeypatch):
    for k, v in row.env.items():
        monkeypatch.setenv(k, str(v))
    _lib.clear_query_cache()
    try:
        return wc.choice(lib, row)
    finally:
        for k in row.env:
            monkeypatch.delenv(k, raising=False)
        _lib.clear_query_cache()


def test_rows_use_the_documented_switches_only():
    ids = [r.id for r in wc.H_ROWS + wc.F_ROWS]
    assert len(set(ids)) == len(ids)
    for row in wc.H_ROWS + wc.F_ROWS:
        assert set(row.env) <= set(wc.SWITCHES), row.id
        assert len(row.record) == len(wc.FIELDS) == 11


@pytest.mark.parametrize('row', wc.H_ROWS + wc.F_ROWS, ids=[r.id for r in wc.H_ROWS + wc.F_ROWS])
def test_row_selects_what_it_names(lib, row, plain_env):
    got = chosen(lib, row, plain_env)
    assert got == row.record, '%s\n  selects %s\n  table   %s' % (row.id, wc.describe(got), wc.describe(row.record))


def test_record_is_zero_before_any_launch(lib):
    """pseg_debug_last_wgrad on a thread that has launched no weight gradient (a fresh one: the record is the calling thread's):
    zeros; the queries refuse a null record and a bad geometry with a message and leave the record alone"""
    import threading
    failures = []

    def body():
        try:
            _fresh_thread(lib)
        except BaseException as e:      # (re-raised in the test's own thread)
            failures.append(e)

    t = threading.Thread(target=body)
    t.start()
    t.join()
    if failures:
        raise failures[0]


def _fresh_thread(lib):
    rec = (ctypes.c_int * 11)(*[7] * 11)
    assert lib.pseg_debug_last_wgrad(rec) == 0 and list(rec) == [0] * 11
    rec = (ctypes.c_int * 11)(*[7] * 11)
    assert lib.pseg_conv2d_wgrad_choice(1, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, 1, 7, 0, rec) == -1 and b'precision' in lib.pseg_last_error()
    assert lib.pseg_conv2d_wgrad_choice_h(0, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, 1, rec) == -1 and b'geometry' in lib.pseg_last_error()
    assert list(rec) == [7] * 11
    assert lib.pseg_debug_last_wgrad(None) == -1 and lib.pseg_conv2d_wgrad_choice_h(1, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, 1, None) == -1
    # the queries are not launches: the record of the thread's last launch stays as it was
    rec = (ctypes.c_int * 11)()
    assert lib.pseg_conv2d_wgrad_choice_h(1, 8, 8, 32, 8, 8, 64, 3, 3, 1, 1, 1, rec) == 0 and rec[0] == wc.WGRAD_H
    last = (ctypes.c_int * 11)(*[7] * 11)
    assert lib.pseg_debug_last_wgrad(last) == 0 and list(last) == [0] * 11


def test_tables_restate_the_sources():
    """the tile tables and kernel codes this file argues from are those of the sources"""
    csrc = os.path.join(os.path.dirname(HERE), 'pytorch_segmentation_amd', 'csrc')
    half = open(os.path.join(csrc, 'conv_half_wgrad.hip')).read()
    line = re.search(r'constexpr HWgradTile kHWgradTiles\[\] = \{(.*)\};', half).group(1)
    assert [tuple(map(int, t[:2])) for t in re.findall(r'\{(\d+), (\d+), \d+, \d+\}', line)] == wc.H_TILES
    fp32 = open(os.path.join(csrc, 'conv_wgrad.hip')).read()
    table = fp32[fp32.index('constexpr WgradDmaTile kWgradDmaTiles[] = {'):fp32.index('constexpr int kNumWgradDmaTiles')]
    dma = [((int(a), int(b)), s == 'true') for a, b, s in re.findall(r'\{(\d+), (\d+), \d+, \d+, (true|false)\}', table)]
    compiled = {(t, skip) for t, has_skip in dma for skip in ((0, 1) if has_skip else (0,))}
    assert len(compiled) == 9 and compiled == wc.F_DMA_REACHABLE | wc.F_DMA_UNREACHABLE
    assert len(wc.H_REACHABLE) == 16 and len(wc.H_UNREACHABLE) == 4 and not (wc.H_REACHABLE & wc.H_UNREACHABLE)
    assert wc.H_REACHABLE | wc.H_UNREACHABLE == {(t, s, b) for t in wc.H_TILES for s in (0, 1) for b in wc.BKPS}
    header = open(os.path.join(os.path.dirname(HERE), 'include', 'pseg_amd.h')).read()
    for name, code in (('REGISTER', wc.WGRAD_REGISTER), ('LIMB', wc.WGRAD_LIMB), ('DMA', wc.WGRAD_DMA), ('HALO', wc.WGRAD_HALO), ('H', wc.WGRAD_H)):
        assert re.search(r'#define PSEG_KERNEL_WGRAD_%s %d\b' % (name, code), header), name
    common = open(os.path.join(csrc, 'conv_common.h')).read()
    for name, code in (('kWgDense', wc.DENSE), ('kWgSkipRows', wc.SKIP_ROWS), ('kWgSkipPatches', wc.SKIP_PATCHES), ('kWgPacked', wc.PACKED),
                       ('kWgRowMajorDma', wc.ROW_MAJOR_DMA)):
        assert re.search(r'constexpr int %s = %d;' % (name, code), common), name


def test_every_reachable_half_instantiation_is_hit():
    """(a): the fp16 rows hit the sixteen reachable instantiations of wgrad_h_kernel, every one of them with every pixel order it
    can run (dense in patch order and row-major; SKIP: dead rows and dead patches), and none of the four unreachable ones"""
    hit = {wc.instance_h(r.record) for r in wc.H_ROWS}
    assert hit == wc.H_REACHABLE, (sorted(hit ^ wc.H_REACHABLE))
    orders = {}
    for r in wc.H_ROWS:
        orders.setdefault(wc.instance_h(r.record), set()).add((r.record[5], r.record[6]))
    for inst, seen in sorted(orders.items()):
        want = {(wc.SKIP_ROWS, 0), (wc.SKIP_PATCHES, 1)} if inst[1] else {(wc.DENSE, 0), (wc.DENSE, 1)}
        assert seen == want, (inst, seen)
    patches = {r.record[6:9] for r in wc.H_ROWS}
    assert patches == {(1, 1, 32), (1, 2, 16), (1, 4, 8), wc.ROW_MAJOR}
    # the sliced-operand cases: every tile, in patch order and row-major
    assert {(t, p[0]) for t, _, p in wc.H_SLICED} == {(t, m) for t in wc.H_TILES for m in (0, 1)}
    # the XCD remap: a launch with a remapped head and a tail (18 blocks), one without a tail (16)
    for row in wc.H_ROWS:
        if row.id in wc.BLOCKS:
            g = wc.geometry(row.case, 'h')
            tiles = -(-g[6] // row.record[1]) * -(-g[7] * g[8] * g[3] // row.record[2])
            assert tiles * row.record[9] == wc.BLOCKS[row.id], row.id
    assert sorted(set(wc.BLOCKS.values())) == [16, 18]


def test_every_reachable_fp32_dma_instantiation_is_hit():
    """(b): the exact-fp32 rows (and the family cases of tests/test_ops_gpu.py they extend) hit the eight reachable instantiations
    of wgrad_f32_dma_kernel, and every pixel order 0 .. 4 on each kernel family that can run it"""
    dma = [r for r in wc.F_ROWS if r.record[0] == wc.WGRAD_DMA]
    hit = {wc.instance_f(r.record) for r in dma}
    assert hit == wc.F_DMA_REACHABLE, sorted(hit ^ wc.F_DMA_REACHABLE)
    for kernel, want in wc.F_ORDERS.items():
        seen = {r.record[5] for r in wc.F_ROWS if r.record[0] == kernel}
        if kernel == wc.WGRAD_REGISTER:
            seen |= {wc.FAMILY_RECORDS['register_32_to_21'][2]}      # (dense on the register-staged kernel: the family cases)
        assert seen == want, (kernel, seen)
    assert set().union(*wc.F_ORDERS.values()) == {0, 1, 2, 3, 4}
    # a row-major row per tile
    assert {(r.record[1], r.record[2]) for r in dma if r.record[5] == wc.ROW_MAJOR_DMA} == {t for t, _ in wc.F_DMA_REACHABLE}


GRID_CHANNELS = range(8, 265, 8)
GRID_MAPS = [(8, 8), (7, 9), (16, 16)]


def test_no_shape_of_the_grid_selects_anything_else(lib, plain_env):
    """Cout, Cin in 8 .. 264 by 8, k in 1 / 3 / 7, dilation 1 / 6 ("same" padding), maps 8x8, 7x9, 16x16 -- and, for the fp16 kernel,
    both K-steps forced beside its own choice: every selection lies inside the expected sets, and the grid itself reaches all of
    them but the forced K-steps' (it is the table that must be complete; the grid is the evidence for what cannot be reached)"""
    rec = (ctypes.c_int * 11)()
    hit_h, hit_f, kernels_f = set(), set(), set()
    for (H, W), k, dil, Cin, Cout in itertools.product(GRID_MAPS, (1, 3, 7), (1, 6), GRID_CHANNELS, GRID_CHANNELS):
        pad = dil * (k - 1) // 2
        g = (1, H, W, Cin, H, W, Cout, k, k, 1, pad, dil)
        assert lib.pseg_conv2d_wgrad_choice_h(*g, rec) == 0
        r = tuple(rec)
        assert r[0] == wc.WGRAD_H and r[3] in wc.BKPS
        hit_h.add(wc.instance_h(r)[:2])
        assert lib.pseg_conv2d_wgrad_choice(*g, 0, 0, rec) == 0
        r = tuple(rec)
        kernels_f.add(r[0])
        if r[0] == wc.WGRAD_DMA:
            hit_f.add(wc.instance_f(r))
            assert r[5] in wc.F_ORDERS[wc.WGRAD_DMA], r
    reachable_h = {i[:2] for i in wc.H_REACHABLE}
    assert hit_h == reachable_h, sorted(hit_h ^ reachable_h)
    assert not hit_h & {i[:2] for i in wc.H_UNREACHABLE}
    assert hit_f == wc.F_DMA_REACHABLE, sorted(hit_f ^ wc.F_DMA_REACHABLE)
    assert kernels_f <= {wc.WGRAD_DMA, wc.WGRAD_HALO, wc.WGRAD_REGISTER}
    # the K-step is chosen apart from tile and SKIP (PSEG_HWGRAD_BKP or the rule on kh * kw, Cout and K): forcing it moves nothing else
    for bkp in wc.BKPS:
        plain_env.setenv('PSEG_HWGRAD_BKP', str(bkp))
        _lib.clear_query_cache()
        for (H, W), k, dil, Cin, Cout in itertools.product(GRID_MAPS, (1, 3), (1, 6), (8, 32, 128, 264), (8, 40, 136, 264)):
            g = (1, H, W, Cin, H, W, Cout, k, k, 1, dil * (k - 1) // 2, dil)
            assert lib.pseg_conv2d_wgrad_choice_h(*g, rec) == 0
            assert rec[3] == bkp and wc.instance_h(tuple(rec)) in wc.H_REACHABLE, tuple(rec)


def test_default_plan_of_the_small_half_cases(lib, plain_env):
    """which instantiation the default selection gives every CONV_CASES entry of tests/test_half_gpu.py, against the pinned table"""
    from test_half_gpu import CONV_CASES
    assert list(wc.DEFAULT_PLAN_H) == CONV_CASES
    moved = []
    for case, want in wc.DEFAULT_PLAN_H.items():
        got = wc.choice(lib, wc.Row('default', 'h', case, {}, None, ()))
        if got != (wc.WGRAD_H,) + want:
            moved.append('%r\n  selects %s\n  pinned  %s' % (case, wc.describe(got), wc.describe((wc.WGRAD_H,) + want)))
    assert not moved, '\n'.join(moved)
    assert {wc.instance_h((wc.WGRAD_H,) + r) for r in wc.DEFAULT_PLAN_H.values()} == wc.DEFAULT_REACH_H
    assert wc.DEFAULT_REACH_H < wc.H_REACHABLE
