"""The library calls behind nn.Conv2d, nn.BatchNorm2d, nn.ConvNormAct and the ResNet bottleneck are pinned:
tests/golden/nn_calls.json holds, for every case of tests/nn_calls.py, the ordered list of pseg_* entry points with every argument
(pointers as ordinals of first appearance), the fork / enter / exit / record markers of the weight-gradient stream, the grad_ready
callbacks and the shapes and optional parts of what the layers return -- written by tools/nn_call_log.py with nn.py, ops.py and
the backbones of the commit BEFORE the fp32 and fp16 forms of Conv2d.fwd / .bwd were merged and BatchNorm2d's saved state was
named.  A launch that moves, goes missing, changes an argument or changes sides of the fork shows here without a GPU."""
import json
import os

import pytest

import nn_calls
from pytorch_segmentation_amd import _lib
from pytorch_segmentation_amd.csrc import build as csrc_build

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE = json.load(open(os.path.join(HERE, 'golden', 'nn_calls.json')))
CASES = {c[0]: c for c in nn_calls.cases()}


@pytest.fixture(scope='module')
def lib():
    csrc_build.build(verbose=False)
    _lib.clear_query_cache()
    return _lib.load()


def test_every_case_is_pinned():
    assert sorted(CASES) == sorted(TABLE) and len(CASES) >= 200


@pytest.mark.parametrize('name', sorted(CASES))
def test_calls_as_pinned(lib, name):
    got = json.loads(json.dumps(nn_calls.run_case(CASES[name])))
    want = TABLE[name]
    nn_calls.check_presence(CASES[name], got)
    nn_calls.check_presence(CASES[name], want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, '%s: entry %d differs\n  now    %s\n  pinned %s' % (name, i, g, w)
    n = min(len(got), len(want))
    assert len(got) == len(want), '%s: %d entries, pinned %d; first unmatched: %s' % (name, len(got), len(want), (got[n:] + want[n:])[0])


def test_recorder_leaves_nothing_behind(lib):
    """Outside a recording the package calls the library and torch as before."""
    import torch
    from pytorch_segmentation_amd import ops
    before = (_lib.call, ops._stream, ops.fork_aux, torch.empty, torch.cuda.stream, torch.Tensor.record_stream, ops.CAPTURING)
    nn_calls.run_case(CASES['dense/3x3s1/fp32'])
    assert before == (_lib.call, ops._stream, ops.fork_aux, torch.empty, torch.cuda.stream, torch.Tensor.record_stream, ops.CAPTURING)
