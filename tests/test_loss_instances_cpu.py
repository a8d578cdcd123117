"""The case table of tests/test_loss_instances_gpu.py reaches what it claims, and its bounds are sound -- shown without a GPU.

Over tests/loss_cases.py:
(a) every compiled instance of ce_fused_kernel / ce_generic_kernel / argmax_kernel (CE_COMPILED, ARGMAX_COMPILED, written out from
    the dispatch code and held against the source here) is launched by at least one row, and no row names one that is not compiled;
(b) both forms of the up-sampled loss run at both align_corners values, with the forms stated below shape by shape; both unrolled
    finish loops, the over-the-cap grid of the grid-stride kernels, the misaligned-base fallbacks, a NULL gradient, no valid pixel
    and a non-default ignore_index are reached;
(c) the mirror's pseg_ce_upsampled_ok equals the library's query for every row and every refusal; the refusals are refused by the
    entry point's argument checks, which run before any launch;
(d) pseg_debug_last_loss answers zeros on a thread that has launched nothing, refuses a null pointer, and a refused call leaves it;
(e) the tolerance is not vacuous: a plain torch fp32 evaluation of the same formula on the CPU stays inside the GPU test's bound
    against fp64, row by row (the grid-stride rows left out).

Not reached, and why: the over-the-cap grid of ce_generic_kernel needs more than 4096 x 256 pixels of more than 32 classes (138 MB
of logits), beyond what a quick test can hold against fp64 on the CPU."""
import ctypes
import os
import re
import threading

import pytest
import torch
import torch.nn.functional as F

import loss_cases as lc
from pytorch_segmentation_amd import _lib
from pytorch_segmentation_amd.csrc import build as csrc_build

HERE = os.path.dirname(os.path.abspath(__file__))
FAKE = 0x7f0000000000                       # a 16-byte aligned made-up device address: never dereferenced by an argument check


@pytest.fixture(scope='module')
def lib():
    csrc_build.build(verbose=False)
    return _lib.load()


def rows_of(entry):
    return [r for r in lc.ROWS if r.entry == entry]


def test_rows_are_well_formed():
    ids = [r.id for r in lc.ROWS]
    assert len(set(ids)) == len(ids)
    for row in lc.ROWS:
        assert len(row.record) == len(lc.FIELDS) == 8 and row.record[0] in lc.KERNEL_NAMES, row.id
    for row in rows_of('ce_up'):
        B, C, h, w, H, W, ac, ld, ldd = row.shape
        assert ld % 4 == 0 and ldd % 4 == 0 and ld >= C and ldd >= C and lc.ce_upsampled_ok(h, w, C, H, W, ac), row.id
        if not row.flags.get('big'):
            assert h <= 16 and w <= 16, row.id                   # (the bound grows with max(h, w))
    for row in rows_of('ce'):
        _, t, ign = lc.ce_inputs(row) if not row.flags.get('big') else (None, None, None)
        if t is not None and not row.flags.get('all_ignored'):
            C = row.shape[1]
            assert bool((t == ign).any()) and bool((t >= C).any()) and bool(((t < 0) & (t != ign)).any()), row.id


def test_every_compiled_instance_is_hit():
    """(a), and that the check has teeth: without its only row an instance goes missing"""
    hit = {lc.instance(r.record) for r in rows_of('ce')}
    assert hit <= lc.CE_COMPILED, 'rows name instances that are not compiled: %s' % sorted(hit - lc.CE_COMPILED, key=str)
    assert hit == lc.CE_COMPILED, 'no row reaches %s' % sorted(lc.CE_COMPILED - hit, key=str)
    assert {lc.instance(r.record) for r in rows_of('argmax')} == lc.ARGMAX_COMPILED
    assert {r.record[0] for r in lc.ROWS} == set(lc.KERNEL_NAMES)
    for (shape, inst) in lc.CE_INSTANCE_SHAPES:
        assert lc.instance(lc.BY_ID['ce-%dx%dx%dx%d' % shape].record) == inst, shape
    thinned = [r for r in rows_of('ce') if lc.instance(r.record) != (32, 2) or r.id != 'ce-2x25x4x4']
    assert (32, 2) not in {lc.instance(r.record) for r in thinned}


def test_compiled_sets_restate_the_source():
    src = open(os.path.join(os.path.dirname(HERE), 'pytorch_segmentation_amd', 'csrc', 'loss.hip')).read()
    globals_ = re.findall(r'__global__[^\n]*?void (\w+)\(', src)
    assert sorted(globals_) == sorted(list(lc.KERNEL_NAMES.values()) + list(lc.HELPER_KERNELS)) and len(globals_) == 11, globals_
    launched = {(int(a), int(b)) for a, b in re.findall(r'CE_LAUNCH\(\s*(\d+)\s*,\s*(\d+)\s*\)\s*;', src)}
    assert launched | {lc.GENERIC} == lc.CE_COMPILED
    assert {int(v) for v in re.findall(r'argmax_kernel<(\d)>', src)} == lc.ARGMAX_COMPILED
    enum = re.search(r'enum LossKernel \{(.*?)\};', src, re.S).group(1)
    names = [n.strip().split(' ')[0] for n in enum.replace('\n', ' ').split(',')]
    assert names == ['kLossCeFused', 'kLossCeGeneric', 'kLossCeUpFused', 'kLossCeUpScatter', 'kLossArgmax', 'kLossConfusion',
                     'kLossScaleInplace'] and 'kLossCeFused = 1' in enum
    for name in ('kCeMaxBlocks', 'kUpTY', 'kUpTX', 'kUpCP', 'kUpThreads', 'kUpRY', 'kUpRX', 'kSY', 'kSX', 'kSThreads', 'kMaxConfusionClasses'):
        assert re.search(r'\b%s\s*=\s*%d\b' % (name, getattr(lc, name)), src), name
    flat = re.sub(r'\s+', '', src)           # (spacing and line breaks of the source are free)
    assert 'kSRY=4*kSY+2,kSRX=4*kSX+2' in flat and 'kSPY=kSY+1,kSPX=kSX+1' in flat
    # the caps of the grid-stride launches
    assert 'ce_count_kernel,dim3(capped_blocks(npix,%d))' % lc.kCountMaxBlocks in flat
    assert 'capped_blocks(n4?n4:1,%d)' % lc.kScaleMaxBlocks in flat and 'capped_blocks(n,%d)' % lc.kConfusionMaxBlocks in flat
    assert 'capped_blocks(npix/4,%d)' % lc.kArgmaxMaxBlocks in flat and 'capped_blocks(npix,%d)' % lc.kArgmaxMaxBlocks in flat
    assert 'capped_blocks(total,%d)' % lc.kCombineMaxBlocks in flat
    # the unrolled loops of the finish kernels (ce_finish_kernel's is the loss family's shared one, in loss_common.h)
    shared = re.sub(r'\s+', '', open(os.path.join(os.path.dirname(HERE), 'pytorch_segmentation_amd', 'csrc', 'loss_common.h')).read())
    assert 'for(;i+7*256<nblocks;i+=8*256)' in flat + shared and 'for(;i+3*256<nblocks;i+=4*256)' in flat
    assert 'block_sum_d(thread_sum_partials(partial,nblocks),sh)' in flat
    assert 'returnbest+(a.align?0:2);' in flat
    header = open(os.path.join(os.path.dirname(HERE), 'include', 'pseg_amd.h')).read()
    assert re.search(r'int\s+pseg_debug_last_loss\(\s*int\s*\*\s*out8\s*\)\s*;', header)
    for code, name in lc.KERNEL_NAMES.items():
        assert re.search(r'\b%d %s\b' % (code, name), header), name


# the forms the table was planned with, shape by shape ((h, w, H, W, align_corners) -> form with PSEG_CE_SCATTER unset)
PLANNED_FORMS = {(8, 8, 32, 32, 1): lc.SCATTER, (8, 8, 32, 32, 0): lc.GATHER, (9, 13, 33, 49, 1): lc.SCATTER, (9, 13, 33, 49, 0): lc.GATHER,
                 (5, 9, 15, 27, 0): lc.SCATTER, (5, 9, 13, 20, 0): lc.SCATTER, (6, 10, 9, 15, 1): lc.SCATTER, (7, 11, 7, 11, 0): lc.SCATTER,
                 (7, 11, 7, 11, 1): lc.SCATTER, (16, 16, 65, 65, 1): lc.GATHER, (1, 1, 4, 4, 0): lc.SCATTER, (8, 1, 32, 1, 0): lc.GATHER,
                 (2, 2, 2, 2, 1): lc.SCATTER}


def test_upsampled_forms_and_shapes_are_reached():
    """(b) for the up-sampled loss"""
    assert set(PLANNED_FORMS) == set(lc.UP_SHAPES)
    for shape, form in PLANNED_FORMS.items():
        assert lc.up_form(*shape) == form, shape
        assert lc.up_form(*shape, env='0') == lc.GATHER and lc.up_form(*shape, env='1') == form
    # why x4 with align_corners = 0 falls back: the first tile owns 6 + 4 destination rows, + 2 of slack > kSRY
    assert lc.max_owned(8, 32, 0, lc.kSY) == 12 > lc.kSRY and lc.max_owned(16, 64, 0, lc.kSY) == 12 and lc.max_owned(5, 15, 0, lc.kSY) == 4 + 3 + 2 <= lc.kSRY
    assert lc.max_owned(16, 65, 1, lc.kSX) > lc.kSRX >= lc.max_owned(16, 64, 1, lc.kSX)
    up = rows_of('ce_up')
    small = [r for r in up if not r.flags.get('big')]
    for ac in (0, 1):
        assert {r.record[5] for r in small if r.shape[6] == ac} == {lc.GATHER, lc.SCATTER}, ac
    for form in (lc.GATHER, lc.SCATTER):
        mine = [r for r in small if r.record[5] == form]
        assert {r.shape[1] for r in mine} == set(lc.UP_CLASSES) == {1, 5, 21, 24}, form
        assert {(r.shape[7], r.shape[8]) for r in mine} == {(24, 24), (24, 32), (32, 24), (32, 32)}, form
        assert any(r.flags.get('nograd') for r in mine) and any(r.flags.get('all_ignored') for r in mine), form
        assert any(r.shape[2] % 2 == 1 and r.shape[3] % 8 != 0 for r in mine), form            # both ragged edges
    # a gather launch on a scatter-eligible shape (the two forms side by side) and on one that is not
    assert any(r.record[5] == lc.GATHER and lc.scatter_eligible(*r.shape[2:7]) for r in small)
    assert any(r.record[5] == lc.GATHER and not lc.scatter_eligible(*r.shape[2:7]) and r.flags['env'] is None for r in small)
    # ratios: non-integer, unequal per axis, 1, x3, just above 4; h or w of 1
    ratios = {(r.shape[4] / r.shape[2], r.shape[5] / r.shape[3]) for r in small}
    assert (1.0, 1.0) in ratios and (3.0, 3.0) in ratios and (4.0, 4.0) in ratios and any(a != b and a % 1 and b % 1 for a, b in ratios)
    assert any(4 < a < 4.1 for a, _ in ratios) and any(r.shape[2] == 1 and r.shape[3] == 1 for r in small) and any(r.shape[3] == 1 for r in small)
    # the unrolled loops of the finish kernels, each behind its own form; the grid-stride loop of the combine kernel
    assert any(r.record[5] == lc.SCATTER and r.record[6] > 3 * 256 and r.record[6] % lc.kUpFinishUnroll == 0 for r in up)
    assert any(r.record[5] == lc.GATHER and r.record[6] > 7 * 256 and r.record[6] % lc.kFinishUnroll == 0 for r in up)
    assert any(r.record[5] == lc.SCATTER and r.record[6] > 3 * 256 and r.record[6] % lc.kUpFinishUnroll != 0 for r in up)      # ... and its tail after it
    assert any(r.record[5] == lc.SCATTER and r.shape[0] * r.shape[2] * r.shape[3] * (lc.kUpCP // 4) > lc.kCombineMaxBlocks * 256
               and r.shape[8] > lc.kUpCP for r in up)
    # the labels: ignored and out-of-range blocks everywhere, an ignored pixel on a tile seam where there is one
    for r in small:
        if r.flags.get('all_ignored'):
            continue
        B, C, h, w, H, W, ac, ld, ldd = r.shape
        _, t = lc.up_inputs(r)
        assert bool((t == -100).any()) and bool((t >= C).any()) and t[-1, H - 1, W - 1] == -100, r.id
        assert bool((t < -100).any() | ((t < 0) & (t != -100)).any()) or W < 4, r.id
        assert bool(((t >= 0) & (t < C)).any()), r.id


def test_host_branches_are_reached():
    """(b) for the other entries: the grid-stride loops on the mirror, the fallbacks, the label cases"""
    ce = rows_of('ce')
    big = lc.BY_ID['ce-grid-stride']
    B, C, H, W = big.shape
    assert H * W % 2 == 1 and lc.cdiv(B * H * W, 256) > lc.kCeMaxBlocks == big.record[3] == big.record[6] and big.record[2] == 1
    assert lc.cdiv(B * H * W, 256) > lc.kCountMaxBlocks                                   # ce_count_kernel too
    assert big.record[6] > 7 * 256 and B * C * H * W * 4 < 9 << 20
    # VEC = 1 by a misaligned base, HW % 4 == 0, on each operand
    for which in ('logits', 'dlogits'):
        rows = [r for r in ce if r.flags.get('mis') == which]
        assert rows and all(r.shape[2] * r.shape[3] % 4 == 0 and r.record[2] == 1 for r in rows)
    assert lc.rec_ce(2, 8, 16, dlogits_aligned=False, grad=False)[2] == 4                 # (a NULL gradient is not misaligned)
    assert any(r.shape[0] == 3 and r.shape[2] * r.shape[3] == 12 and r.record[2] == 4 for r in ce)
    assert {lc.instance(r.record) for r in ce if r.flags.get('nograd')} >= {(24, 4), lc.GENERIC}
    assert {r.record[0] for r in ce if r.flags.get('all_ignored')} == {lc.CE_FUSED, lc.CE_GENERIC}
    assert any(r.flags.get('ignore_index') == 255 for r in ce) and any(r.shape[1] == 1 for r in ce)
    am = rows_of('argmax')
    big = lc.BY_ID['argmax-grid-stride']
    assert big.shape[1] == 2 and big.shape[0] * big.shape[2] > 4096 * 256 * 4 and big.record[2:4] == (4, lc.kArgmaxMaxBlocks)
    assert any(r.record[2] == 1 and r.shape[2] % 4 for r in am) and any(r.record[2] == 1 and r.flags.get('mis') and r.shape[2] % 4 == 0 for r in am)
    assert any(r.shape[1] == 1 for r in am)
    cf = rows_of('confusion')
    assert {r.shape[1] for r in cf} == {1, 21, 1024} and {r.shape[0] for r in cf} == {1, 255, 257, 1024 * 256 + 3}
    assert any(lc.cdiv(r.shape[0], 256) > lc.kConfusionMaxBlocks == r.record[3] for r in cf)
    sc = rows_of('scale')
    assert {r.shape[0] for r in sc} == {1, 3, 4, 7, 1027, 2048 * 256 * 4 + 5}
    assert any(lc.cdiv(r.shape[0] // 4, 256) > lc.kScaleMaxBlocks == r.record[3] and r.shape[0] % 4 for r in sc)


def test_mirror_agrees_with_the_library(lib):
    """(c): pseg_ce_upsampled_ok and the workspace queries, for every row, every refusal and a sweep of shapes"""
    for r in rows_of('ce_up'):
        B, C, h, w, H, W, ac, ld, ldd = r.shape
        assert lib.pseg_ce_upsampled_ok(h, w, C, H, W, ac) == lc.ce_upsampled_ok(h, w, C, H, W, ac) == 1, r.id
        assert lib.pseg_ce_upsampled_workspace_bytes(B, h, w) == lc.ce_upsampled_workspace_bytes(B, h, w), r.id
    for h, w, C, H, W, ac in lc.UP_NOT_OK:
        assert lib.pseg_ce_upsampled_ok(h, w, C, H, W, ac) == lc.ce_upsampled_ok(h, w, C, H, W, ac) == 0, (h, w, C, H, W, ac)
    for h in (1, 2, 3, 7, 8, 16, 33, 128):
        for w in (1, 5, 8, 16, 31, 128):
            for ry in (1, 1.5, 2, 3, 3.9, 4, 4.07, 4.3, 5):
                for rx in (1, 2.5, 4, 4.07, 4.3):
                    for ac in (0, 1):
                        for C in (1, 24, 25):
                            H, W = int(h * ry), int(w * rx)
                            assert lib.pseg_ce_upsampled_ok(h, w, C, H, W, ac) == lc.ce_upsampled_ok(h, w, C, H, W, ac), (h, w, C, H, W, ac)
    assert lib.pseg_ce_workspace_bytes(12345) == lc.ce_workspace_bytes()


NO_GPU = pytest.mark.skipif(torch.cuda.is_available(), reason='uses made-up device addresses: host-side checks only')


def _args(ref):
    return [FAKE if a == lc.A else a for a in ref.args]


@NO_GPU
@pytest.mark.parametrize('ref', lc.REFUSALS, ids=[r.id for r in lc.REFUSALS])
def test_refusals(lib, ref):
    """(c): refused on the arguments alone, with the code and the message the row names.  The pointers are made-up addresses, so
    this runs only where no device could be reached should a check ever let a call through."""
    _, argtypes, _ = _lib.prototypes()[ref.name]
    assert len(ref.args) == len(argtypes), ref.id
    rc = getattr(lib, ref.name)(*_args(ref))
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
        rec = (ctypes.c_int * 8)(*[7] * 8)
        assert lib.pseg_debug_last_loss(rec) == 0 and list(rec) == [0] * 8
        assert lib.pseg_debug_last_loss(None) == -1 and b'debug_last_loss' in lib.pseg_last_error()
        assert lib.pseg_debug_last_loss(rec) == 0 and list(rec) == [0] * 8

    on_fresh_thread(body)


@NO_GPU
def test_a_refused_call_leaves_the_record_alone(lib):
    def body():
        for ref in lc.REFUSALS:
            assert getattr(lib, ref.name)(*_args(ref)) == ref.rc
        rec = (ctypes.c_int * 8)(*[7] * 8)
        assert lib.pseg_debug_last_loss(rec) == 0 and list(rec) == [0] * 8

    on_fresh_thread(body)


# ------------------------------------------------------------------------------------------------ (e)
CE_SMALL = [r for r in lc.ROWS if r.entry == 'ce' and not r.flags.get('big')]
UP_ALL = [r for r in lc.ROWS if r.entry == 'ce_up' and r.flags.get('env') is None]        # (the inputs do not depend on the form)


@pytest.mark.parametrize('row', CE_SMALL, ids=[r.id for r in CE_SMALL])
def test_fp32_evaluation_stays_inside_the_bound_ce(row):
    """a plain fp32 evaluation on the CPU -- F.cross_entropy and autograd -- against the fp64 reference, under the GPU test's bound"""
    x, t, ign = lc.ce_inputs(row)
    ref = lc.ce_reference(row)
    C = row.shape[1]
    assert ref.K < 200 and ref.K_loss < 100, (ref.K, ref.K_loss)              # a bound, not a blank cheque
    if ref.n_valid == 0:
        assert bool((ref.A == 0).all()) and ref.loss != ref.loss
        return
    z = x.clone().requires_grad_()
    loss = F.cross_entropy(z, lc.map_labels(t, C, ign), ignore_index=ign)
    loss.backward()
    assert lc.check_grad(row, 'fp32 on the CPU', z.grad, ref) <= ref.K
    assert lc.check_loss(row, 'fp32 on the CPU', loss.item(), ref) <= ref.K_loss
    invalid = (lc.map_labels(t, C, ign) == ign).unsqueeze(1).expand_as(ref.A)
    assert bool((ref.A[invalid] == 0).all()) and bool((ref.A[~invalid] > 0).all())
    assert lc.U * ref.K < 2e-5, ref.K                    # relative to A: far below any wrong or missing term


@pytest.mark.parametrize('row', UP_ALL, ids=[r.id for r in UP_ALL])
def test_fp32_evaluation_stays_inside_the_bound_ce_up(row):
    """F.interpolate + F.cross_entropy and autograd in fp32 on the CPU against the fp64 reference, under the GPU test's bound"""
    B, C, h, w, H, W, ac, ld, ldd = row.shape
    x, t = lc.up_inputs(row)
    ref = lc.up_reference(row)
    if ref.n_valid == 0:
        assert bool((ref.A == 0).all()) and ref.loss != ref.loss
        return
    z = x.clone().requires_grad_()
    loss = F.cross_entropy(F.interpolate(z, size=(H, W), mode='bilinear', align_corners=bool(ac)), lc.map_labels(t, C, -100), ignore_index=-100)
    loss.backward()
    assert lc.check_grad(row, 'fp32 on the CPU', z.grad, ref) <= ref.K
    assert lc.check_loss(row, 'fp32 on the CPU', loss.item(), ref) <= ref.K_loss
    assert lc.U * ref.K < (1e-2 if row.flags.get('big') else 1e-3), ref.K      # relative to A: far below any wrong or missing term
