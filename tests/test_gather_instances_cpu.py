"""The case tables of tests/test_gather_instances_gpu.py reach what they claim -- shown without a GPU, through the pure query
pseg_conv2d_gather_choice, which reads the selection the launches read (select_gather in csrc/conv_gather.hip).

Every row of tests/gather_cases.py must select, in every mode it runs, the (kernel, tile, arithmetic, SKIP, ring depth, GENERIC, row
order, patch, K splits, fused sums) it names, and over the whole table the rows hit every instantiation conv_gather.hip compiles:

  gather_conv_kernel      5 tiles x SKIP x 4 arithmetics = 40, + 256x128 x SKIP x {bf16x3, fp16x3} = 4
  gather_f32_dma_kernel   kF32Tiles x {plain, SKIP} x {2, 3} stages = 16, + GENERIC (two stages) x 4 tiles = 4
  gather_f32_halo_kernel  2 (128x64, 128x32)
  gather_f32_pw_kernel    3 tiles x {plain, fused BatchNorm-backward sums} = 6
  gather_limb_dma_kernel  2 (SKIP)

74 in all, and none of them is unreachable: unlike the weight gradients, whose tile follows from (Cout, K), the gather tile can be
forced (PSEG_CONV_BM / _BN), SKIP depends on the gathered channels and the rate alone, and the ring depth is a switch.  The brute-force
grid below -- channel counts on and off the 32-grid, 1x1 / 3x3 / 7x7, strides 1 / 2, dilations 1 / 6 / 12, four maps, both directions,
the switch settings of the table -- is the evidence for the converse: no shape selects anything OUTSIDE the 74 (a kernel code, tile,
ring depth or flag combination without an instantiation), and every row order a family reports is one the table exercises on it."""
import ctypes
import itertools
import os
import re
import threading

import pytest

import gather_cases as gc
from pytorch_segmentation_amd import _lib
from pytorch_segmentation_amd.csrc import build as csrc_build

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope='module')
def lib():
    csrc_build.build(verbose=False)
    return _lib.load()


@pytest.fixture
def plain_env(monkeypatch):
    """none of the rows' switches set from outside; the library re-reads them before and after"""
    for name in gc.SWITCHES:
        monkeypatch.delenv(name, raising=False)
    _lib.clear_query_cache()
    yield monkeypatch
    monkeypatch.undo()
    _lib.clear_query_cache()


class switches:
    def __init__(self, monkeypatch, env):
        self.mp, self.env = monkeypatch, env

    def __enter__(self):
        for k, v in self.env.items():
            self.mp.setenv(k, str(v))
        _lib.clear_query_cache()

    def __exit__(self, *exc):
        for k in self.env:
            self.mp.delenv(k, raising=False)
        _lib.clear_query_cache()


def test_rows_use_the_documented_switches_only():
    ids = [r.id for r in gc.ROWS] + [r[0] for r in gc.REFUSALS]
    assert len(set(ids)) == len(ids)
    common = open(os.path.join(ROOT, 'pytorch_segmentation_amd', 'csrc', 'conv_common.h')).read()
    for name in gc.SWITCHES:
        assert 'env_int("%s"' % name in common, name
    for row in gc.ROWS:
        assert set(row.env) <= set(gc.SWITCHES), row.id
        assert len(row.record) == len(gc.FIELDS) == 13 and row.modes, row.id
        assert set(row.modes) <= set(gc.MODE_FLAGS) and set(row.tags) <= {'skip', 'pw', 'sliced'}, row.id
        assert ('skip' in row.tags) == bool(row.record[gc.SKIP]), row.id          # every SKIP row is compared with its dense run
        assert ('pw' in row.tags) == (row.record[gc.KERNEL] == gc.POINTWISE), row.id
    for _, _, _, _, mode, env in gc.REFUSALS:
        assert set(env) <= set(gc.SWITCHES) and mode in gc.MODE_FLAGS


@pytest.mark.parametrize('row', gc.ROWS, ids=[r.id for r in gc.ROWS])
def test_row_selects_what_it_names(lib, row, plain_env):
    with switches(plain_env, row.env):
        for mode in row.modes:
            got, want = gc.choice(lib, row.case, row.dgrad, row.prec, mode), gc.as_query(gc.expected(row, mode))
            assert got == want, '%s (%s)\n  selects %s\n  table   %s' % (row.id, mode, gc.describe(got), gc.describe(want))
    if 'skip' in row.tags:      # the dense run it is compared with: the same instantiation but for SKIP, rows in the dense order
        with switches(plain_env, dict(row.env, PSEG_CONV_NOSKIP=1)):
            got = gc.choice(lib, row.case, row.dgrad, row.prec, row.modes[0])
            dense_perm = 3 if row.record[gc.PERM] == 3 else 0
            want = row.record[:gc.SKIP] + (0,) + row.record[gc.SKIP + 1:gc.PERM] + (dense_perm, 0, 0) + row.record[gc.SPLITS:]
            assert got == want, '%s with PSEG_CONV_NOSKIP=1\n  selects %s\n  wanted  %s' % (row.id, gc.describe(got), gc.describe(want))
    if 'pw' in row.tags:        # ... and the ring kernel the persistent one is compared with
        with switches(plain_env, dict(row.env, PSEG_CONV_PW=0)):
            got = gc.choice(lib, row.case, row.dgrad, row.prec, row.modes[0])
            want = gc.as_query(row.record)[:gc.TRY_PW] + (0,)
            assert got == want, (row.id, gc.describe(got))


@pytest.mark.parametrize('refusal', gc.REFUSALS, ids=[r[0] for r in gc.REFUSALS])
def test_refusals_select_no_kernel(lib, refusal, plain_env):
    _, case, dgrad, prec, mode, env = refusal
    with switches(plain_env, env):
        rec = gc.choice(lib, case, dgrad, prec, mode)
    assert rec[gc.KERNEL] == 0 and rec[gc.BNS] == 0, gc.describe(rec)


def test_record_is_zero_before_any_launch(lib):
    """pseg_debug_last_gather on a thread that has launched nothing (a fresh one: the record is the calling thread's): zeros; the
    query refuses a null record and a bad geometry with a message and leaves the record alone; the query is not a launch"""
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
    rec = (ctypes.c_int * 13)(*[7] * 13)
    assert lib.pseg_debug_last_gather(rec) == 0 and list(rec) == [0] * 13
    rec = (ctypes.c_int * 13)(*[7] * 13)
    g = gc.geometry(gc.GRID)
    flags = (0, 0, 0, 0, 0)
    assert lib.pseg_conv2d_gather_choice(*g, 0, 7, *flags, rec) == -1 and b'precision' in lib.pseg_last_error()
    assert lib.pseg_conv2d_gather_choice(0, *g[1:], 0, 0, *flags, rec) == -1 and b'geometry' in lib.pseg_last_error()
    assert lib.pseg_conv2d_gather_choice(*g[:3], 62, *g[4:], 0, 0, *flags, rec) == -1 and b'fours' in lib.pseg_last_error()
    assert lib.pseg_conv2d_gather_choice(*g[:4], 12, *g[5:], 0, 0, *flags, rec) == -1 and b'inconsistent' in lib.pseg_last_error()
    assert list(rec) == [7] * 13
    assert lib.pseg_debug_last_gather(None) == -1 and lib.pseg_conv2d_gather_choice(*g, 0, 0, *flags, None) == -1
    rec = (ctypes.c_int * 13)()
    assert lib.pseg_conv2d_gather_choice(*g, 0, 0, *flags, rec) == 0 and rec[gc.KERNEL] == gc.RING
    last = (ctypes.c_int * 13)(*[7] * 13)
    assert lib.pseg_debug_last_gather(last) == 0 and list(last) == [0] * 13


def test_tables_restate_the_sources():
    """the tile tables and kernel codes this file argues from are those of the sources"""
    src = open(os.path.join(ROOT, 'pytorch_segmentation_amd', 'csrc', 'conv_gather.hip')).read()
    table = src[src.index('constexpr F32Tile kF32Tiles[] = {'):src.index('constexpr int kNumF32Tiles')]
    tiles = [(int(a), int(b), p == 'true', int(h)) for a, b, p, h in re.findall(r'\{(\d+), (\d+), \d+, \d+, (true|false), (\d)\}', table)]
    assert [t[:2] for t in tiles] == gc.F32_TILES
    assert [t[:2] for t in tiles if t[2]] == gc.PW_TILES and [t[:2] for t in tiles if t[3]] == gc.HALO_TILES
    # the register-staged kernel's table: the five tiles of PSEG_GATHER_ROW in launch_tiles' slot order, 256x128 for two arithmetics
    row = src[src.index('#define PSEG_GATHER_ROW'):src.index('static const GatherFnTable fns32')]
    assert [tuple(map(int, t)) for t in re.findall(r'gather_conv_kernel<(\d+), (\d+), \d, \d, SK, PR>', row)] == gc.REG_TILES
    big = re.findall(r'gather_conv_kernel<256, 128, 4, 2, (true|false), (\d)>', src)
    assert sorted(big) == [('false', '1'), ('false', '3'), ('true', '1'), ('true', '3')]
    assert len(re.findall(r'PSEG_GATHER_ROW\((?:true|false), \d,', src)) == 8
    assert 'launch_ring_as<I, false, 2, true>' in src and len(re.findall(r'launch_ring_as<I, (?:true|false), [23], false>', src)) == 4
    assert len(re.findall(r'gather_limb_dma_kernel<(?:true|false)>, grid', src)) == 2
    header = open(os.path.join(ROOT, 'include', 'pseg_amd.h')).read()
    for name, code in (('REGISTER', gc.REGISTER), ('LIMB_DMA', gc.LIMB_DMA), ('RING', gc.RING), ('RING_GENERIC', gc.RING_GENERIC),
                       ('POINTWISE', gc.POINTWISE), ('HALO', gc.HALO)):
        assert re.search(r'#define PSEG_KERNEL_GATHER_%s %d\b' % (name, code), header), name
    for name, code in (('FP32', gc.FP32), ('BF16X3', gc.BF16X3), ('BF16X6', gc.BF16X6), ('FP16X3', gc.FP16X3)):
        assert re.search(r'#define PSEG_PREC_%s %d\b' % (name, code), header), name
    common = open(os.path.join(ROOT, 'pytorch_segmentation_amd', 'csrc', 'conv_common.h')).read()
    waves = re.search(r'static int waves_m\(TileCfg t\) \{ return (.*); \}', common).group(1)
    assert waves == 't.bm == 256 ? 4 : (t.bn == 32 ? 4 : (t.bm == 32 ? 1 : 2))'
    assert all(gc.WAVE_ROWS[t] == (4 if t[0] == 256 else 4 if t[1] == 32 else 1 if t[0] == 32 else 2) for t in gc.WAVE_ROWS)
    compiled = len(gc.REGISTER_COMPILED) + len(gc.RING_COMPILED) + len(gc.HALO_COMPILED) + len(gc.PW_COMPILED) + len(gc.LIMB_COMPILED)
    assert (len(gc.REGISTER_COMPILED), len(gc.RING_COMPILED), compiled) == (44, 20, 74)


COMPILED = {'register': gc.REGISTER_COMPILED, 'ring': gc.RING_COMPILED, 'halo': gc.HALO_COMPILED, 'pw': gc.PW_COMPILED,
            'limb': gc.LIMB_COMPILED}


def test_every_instantiation_is_hit():
    """taken together the rows hit all 74 instantiations (none is unreachable), every row order on each kernel that accepts it, and a
    sliced-operand row per tile and kernel family"""
    hit = gc.instances_hit()
    assert not gc.UNREACHABLE
    for fam, want in COMPILED.items():
        assert hit[fam] == want, (fam, sorted(hit[fam] ^ want, key=repr))
    orders = {}
    for row in gc.ROWS:
        orders.setdefault(row.record[gc.KERNEL], set()).add(row.record[gc.PERM])
    assert orders == gc.ROW_ORDERS, orders
    # K splits: two, and a ragged four, on one tile per arithmetic
    assert {(r.prec, r.record[gc.SPLITS]) for r in gc.ROWS if r.record[gc.SPLITS] > 1} == {(p, n) for p in range(4) for n in (2, 4)}
    sliced = {(r.record[gc.KERNEL], r.record[gc.BM], r.record[gc.BN]) for r in gc.ROWS if 'sliced' in r.tags}
    want = {(gc.REGISTER,) + t for t in gc.REG_TILES + [gc.BIG]} | {(k,) + t for k in (gc.RING, gc.RING_GENERIC) for t in gc.F32_TILES}
    want |= {(gc.HALO,) + t for t in gc.HALO_TILES} | {(gc.POINTWISE,) + t for t in gc.PW_TILES} | {(gc.LIMB_DMA,) + gc.BIG}
    assert sliced == want, sorted(sliced ^ want)
    # ... and the table holds exactly the (instantiation, problem) pairs gc.required() states, one row each: a row taken out is a
    # pair missing, a row added must be stated there
    keys = [gc.row_key(r) for r in gc.ROWS]
    assert len(set(keys)) == len(keys), sorted((k for k in keys if keys.count(k) > 1), key=repr)
    assert set(keys) == gc.required(), sorted(set(keys) ^ gc.required(), key=repr)


def test_selection_facts_that_need_no_launch(lib, plain_env):
    """GENERIC stays at two stages when three are asked for (PSEG_CONV_F32DMA=1); the default plan runs the stem on 128x32"""
    with switches(plain_env, gc.forced((128, 64), SPLITK=1, F32DMA=1)):
        assert gc.choice(lib, gc.GEN, 0, gc.FP32) == gc.record(gc.RING_GENERIC, (128, 64), stages=2, generic=1)
    for mode in gc.FWD_MODES:
        assert gc.choice(lib, gc.STEM, 0, gc.FP32, mode) == gc.record(gc.RING_GENERIC, (128, 32), stages=2, generic=1)


GRID_CHANNELS = (4, 20, 32, 40, 64, 136, 256)
GRID_MAPS = [(8, 8), (13, 13), (16, 32), (32, 32)]
GRID_ENVS = [{}, {'PSEG_CONV_SPLITK': 1}, {'PSEG_CONV_F32DMA': 0}, {'PSEG_CONV_SPLITK': 1, 'PSEG_CONV_F32DMA': 1}, {'PSEG_CONV_FORCEBIG': 1},
             {'PSEG_CONV_SPLITK': 4}, {'PSEG_CONV_NOSKIP': 1}, {'PSEG_CONV_NOBAND': 1}, {'PSEG_CONV_PW': 0}, {'PSEG_CONV_HALO': 0},
             {'PSEG_CONV_NOBIG': 1, 'PSEG_CONV_FORCEBIG': 1}, {'PSEG_CONV_PW_RESIDENT': gc.PW_RESIDENT}] + \
            [gc.forced(t, SPLITK=1) for t in gc.REG_TILES + [gc.BIG]]


def test_no_shape_of_the_grid_selects_anything_else(lib, plain_env):
    """Cin, Cout in 4 .. 256 on and off the 32-grid, k in 1 / 3 / 7, stride 1 / 2, dilation 1 / 6 / 12 ("same" padding), maps 8x8, 13x13,
    16x32, 32x32, forward and data gradient, every arithmetic, the switch settings of the table, with and without the fused sums and
    the planes: every selection is a compiled instantiation (or a refusal), in a row order the table exercises on that kernel"""
    rec = (ctypes.c_int * 13)()
    seen = {fam: set() for fam in COMPILED}
    n = 0
    for env in GRID_ENVS:
        with switches(plain_env, env):
            for (H, W), k, stride, dil, Cin, Cout, dgrad in itertools.product(GRID_MAPS, (1, 3, 7), (1, 2), (1, 6, 12), GRID_CHANNELS,
                                                                              GRID_CHANNELS, (0, 1)):
                if k == 1 and dil > 1:
                    continue
                pad = dil * (k - 1) // 2
                g = (1, H, W, Cin, gc.out_size(H, k, stride, pad, dil), gc.out_size(W, k, stride, pad, dil), Cout, k, k, stride, pad, dil)
                for prec, mode in ((0, 'plain'), (0, 'stats'), (0, 'bns'), (1, 'plain'), (1, 'planes'), (2, 'plain'), (3, 'plain')):
                    if (mode == 'stats' and dgrad) or (mode in ('bns', 'planes') and not dgrad):
                        continue
                    assert lib.pseg_conv2d_gather_choice(*g, dgrad, prec, *gc.MODE_FLAGS[mode], rec) == 0, lib.pseg_last_error()
                    r = tuple(rec)
                    n += 1
                    fam, inst = gc.instance(r)
                    if fam == 'refused':
                        continue
                    if fam == 'ring' and r[gc.TRY_PW]:       # (the persistent kernel may take it: its instantiation must exist too)
                        assert ((r[gc.BM], r[gc.BN]), r[gc.BNS]) in gc.PW_COMPILED, r
                        seen['pw'].add(((r[gc.BM], r[gc.BN]), r[gc.BNS]))
                    assert inst in COMPILED[fam], (g, dgrad, prec, mode, env, gc.describe(r))
                    assert r[gc.PERM] in gc.ROW_ORDERS[r[gc.KERNEL]], (g, dgrad, prec, mode, env, gc.describe(r))
                    assert r[gc.PREC] == (prec if fam == 'register' else 1 if fam == 'limb' else 0)
                    seen[fam].add(inst)
    assert n > 100000
    # the grid alone reaches most of them; what it misses the table forces (asserted above, per row)
    for fam in seen:
        assert seen[fam] <= COMPILED[fam]
    assert seen['halo'] == gc.HALO_COMPILED and seen['limb'] == gc.LIMB_COMPILED and seen['pw'] == gc.PW_COMPILED
