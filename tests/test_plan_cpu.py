"""The planning decisions behind the integer-only conv queries are pinned: tests/golden/plan_table.json holds the answers of every
query (tests/plan_queries.py) for a few hundred conv problems, under the default environment, PSEG_CONV_NOSKIP=1,
PSEG_HCONV_PERSIST=0 / 2 and PSEG_WGRAD_F32DMA=0 / PSEG_WGRAD_NARROW256=0 / PSEG_WGRAD_BPC=2, written by tools/plan_table.py with
the library of the commit BEFORE the kernel selection was gathered into select_gather / select_wgrad (conv_gather.hip, conv_wgrad.hip) and
select_gather_h / select_wgrad_h (conv_half_gather.hip, conv_half_wgrad.hip): the PSEG_WGRAD_* tables with the commit before the
weight gradient's was.
A selection that moves changes the statistics layout, the fused-sum rows, a split count or a workspace size, and shows here
without a GPU."""
import json
import os
import re

import pytest

import plan_queries
from pytorch_segmentation_amd import _lib
from pytorch_segmentation_amd.csrc import build as csrc_build

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE = json.load(open(os.path.join(HERE, 'golden', 'plan_table.json')))


@pytest.fixture(scope='module')
def lib():
    csrc_build.build(verbose=False)
    return _lib.load()


@pytest.mark.parametrize('setting', sorted(TABLE))
def test_queries_answer_as_pinned(lib, setting, monkeypatch):
    rows = TABLE[setting]
    assert len(rows) >= 200
    for kv in filter(None, setting.split(',')):
        monkeypatch.setenv(*kv.split('='))
    _lib.clear_query_cache()          # the library re-reads its PSEG_* switches
    try:
        bad = []
        for prob, want in rows:
            got = plan_queries.answers(lib, tuple(prob))
            bad += ['%s %s: %d, pinned %d' % (prob, n, g, w) for n, g, w in zip(plan_queries.NAMES, got, want) if g != w]
            assert len(got) == len(want) == len(plan_queries.NAMES)
        assert not bad, '%d answers moved:\n%s' % (len(bad), '\n'.join(bad[:40]))
    finally:
        monkeypatch.undo()
        _lib.clear_query_cache()


def test_pinned_problems_cover_the_cases():
    probs = [tuple(p) for p, _ in TABLE['']]
    assert {p[5] for p in probs} >= {1, 3, 7} and {p[6] for p in probs} >= {1, 2} and {p[8] for p in probs} >= {1, 2, 6, 12, 18}
    assert {p[0] for p in probs} >= {1, 2, 16} and {p[1] for p in probs} & {33, 65}
    assert {p[3] for p in probs} & {3, 21} and {p[3] for p in probs} & {48, 144}


def _csrc(name):
    return open(os.path.join(os.path.dirname(HERE), 'pytorch_segmentation_amd', 'csrc', name)).read()


FP32_UNITS = ('conv_gather.hip', 'conv_wgrad.hip', 'core.hip')     # the fp32 / limb conv units and the library's core
HALF_UNITS = ('conv_half_gather.hip', 'conv_half_wgrad.hip', 'conv_half.h')     # the fp16 conv units and what they share


def _half():
    return ''.join(map(_csrc, HALF_UNITS))


def test_gather_selection_is_written_once():
    """The fp32 conv units decide tap skipping nowhere themselves (gather_row_order, conv_common.h, does, for fp32 and fp16) and
    the rows query has no plan of its own."""
    gather = _csrc('conv_gather.hip')
    host = gather[gather.index('static GatherChoice select_gather('):]
    for src in map(_csrc, FP32_UNITS):
        assert 'dgrad_bnstat_plan' not in src and 'plan_fwd_stats' not in src and 'plan_dgrad' not in src
    # the gather side's host code, and all of the other two units (kernels included)
    for text in (host, _csrc('conv_wgrad.hip'), _csrc('core.hip')):
        assert not re.search(r'skip_taps\s*=[^=]', text)
    common = _csrc('conv_common.h')
    assert len(re.findall(r'\.skip_taps = \(', common)) == 1


def test_half_gather_selection_is_written_once():
    """The fp16 gather side (conv_half_gather.hip) has one selection, select_gather_h, and the other fp16 files none: no dry run
    of the launch path behind the fused-sums query, no second or third derivation of the statistics layout, no launch ladders
    anywhere in them -- and the selection asks the device nothing."""
    for gone in ('bns_query', 'plan_fwd_stats_h', 'plan_run_h', 'PSEG_H_LAUNCH', 'PSEG_HP_LAUNCH'):
        assert gone not in _half(), gone
    src = _csrc('conv_half_gather.hip')
    assert 'select_gather_h(' not in _csrc('conv_half_wgrad.hip') + _csrc('conv_half.h')
    start = src.index('static HGatherChoice select_gather_h(')
    body = src[start:src.index('\n}\n', start)]
    assert 'return c;' in body and len(body.splitlines()) > 40
    assert not re.search(r'\bhip[A-Z]\w*', body), re.findall(r'\bhip[A-Z]\w*', body)


def _body(src, head):
    start = src.index(head)
    return src[start:src.index('\n}\n', start)]


@pytest.mark.parametrize('name,head', [('conv_wgrad.hip', 'static WgradChoice select_wgrad('),
                                       ('conv_half_wgrad.hip', 'static HWgradChoice select_wgrad_h(')])
def test_wgrad_selection_is_pure(name, head):
    """The weight gradient's kernel is picked in one function per number format, which launches nothing and asks the device
    nothing; the launch path and the queries (_splits, _slabs, _workspace_bytes) all go through it."""
    src = _csrc(name)
    body = _body(src, head)
    assert 'return c;' in body and len(body.splitlines()) > 20
    assert not re.search(r'\bhip[A-Z]\w*', body), re.findall(r'\bhip[A-Z]\w*', body)
    fn = head[head.index('select_wgrad'):-1]
    assert len(re.findall(r'\b%s\(' % fn, src)) >= 4                   # its definition, the launch path, both queries
    assert not re.search(r'\bplan_wgrad(_h)?\(', src.replace(body, ''))  # no plan of anyone's own beside it
    # ... nor a selection or a plan in the other fp32 units, the fp16 gather unit or the fp16 units' header
    for other in ('conv_gather.hip', 'core.hip', 'conv_half_gather.hip', 'conv_half.h'):
        assert not re.search(r'\b(select|plan)_wgrad(_h)?\(', _csrc(other)), other


def test_wgrad_launches_are_written_once():
    """No launch macros in the fp16 conv units; the slab reduction is launched from launch_slab_reduce alone (the batch kernel is
    another kernel); WgradParams::skip_rows is assigned by set_wgrad_geometry (conv_common.h) and nowhere else."""
    fp32, half, common = ''.join(map(_csrc, FP32_UNITS)), _half(), _csrc('conv_common.h')
    assert 'PSEG_HW_LAUNCH' not in half
    launches = [m.start() for m in re.finditer(r'hipLaunchKernelGGL\(\s*\(?slab_reduce_kernel\b', fp32 + half + common)]
    assert len(launches) == 1
    reduce_fn = _body(_csrc('conv_wgrad.hip'), 'int launch_slab_reduce(')
    assert 'hipLaunchKernelGGL(slab_reduce_kernel,' in reduce_fn
    assign = r'skip_rows\s*=[^=]'
    assert not re.search(assign, fp32) and not re.search(assign, half)
    assert len(re.findall(assign, common)) == 1 and re.search(assign, _body(common, 'static void set_wgrad_geometry('))


def test_switches_are_read_in_one_place():
    """cfg_load (conv_common.h) is the only reader of the conv planning switches: env_int( occurs in its own definition and in
    cfg_load's body, nowhere else in conv_common.h and nowhere in conv_gather.hip / conv_wgrad.hip / core.hip / the fp16 units
    (conv_half_gather.hip, conv_half_wgrad.hip, conv_half.h), which do not call getenv( either -- so pseg_config_reload() reaches every switch and no plan, selection or launch helper keeps a
    per-process copy of one."""
    fp32, half, common = ''.join(map(_csrc, FP32_UNITS)), _half(), _csrc('conv_common.h')
    assert 'env_int(' not in fp32 and 'env_int(' not in half
    assert 'getenv(' not in fp32 and 'getenv(' not in half
    definition = _body(common, 'static int env_int(')
    load = _body(common, 'inline void cfg_load(')
    assert load.count('env_int(') >= 20
    rest = common.replace(definition, '').replace(load, '')
    assert 'env_int(' not in rest and 'getenv(' not in rest
    assert common.count('getenv(') == 1 and 'getenv(' in definition


def test_lab_build_is_gone():
    """The fp16 conv lab build (measured-and-rejected kernels, ablation bits) is in no source under csrc/."""
    csrc = os.path.join(os.path.dirname(HERE), 'pytorch_segmentation_amd', 'csrc')
    names = [n for n in sorted(os.listdir(csrc)) if n.endswith(('.hip', '.h', '.py'))]
    assert 'conv_half.hip' not in names and 'build.py' in names and set(FP32_UNITS + HALF_UNITS) <= set(names)
    assert sorted(n for n in names if n.endswith('.hip')) == sorted(csrc_build.SOURCES)     # every unit is built, none is left behind
    # ... and every header is a dependency of the build
    assert sorted(n for n in names if n.endswith('.h')) == sorted(h for h in csrc_build.HEADERS if os.sep not in h)
    for n in names:
        src = _csrc(n)
        for gone in ('PSEG_LAB', 'PSEG_ABLATE', 'gather_hh_kernel', 'gather_hr_kernel'):
            assert gone not in src, (n, gone)
