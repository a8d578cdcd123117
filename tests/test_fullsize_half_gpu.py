"""Every kernel call of one half-precision (`-mp`) training step at full size, against fp64.

BASELINE.json configs[2] (DeepLabV3+ R50, 21 classes, 512x512, batch 16), configs[4] (HRNet, 21 classes, 512x512, batch 8) and
configs[1] (UNet on MobileNetV2, 2 classes, 256x256, batch 8: the depthwise kernels above their launch cap, ReLU6)
under Trainer(mixed_precision=True): the explicit step `bench.py` and `train.py -mp` run (Trainer._fwd_loss_bwd), with the fp16
filter copies, the loss-scaled entry into the fp16 network and, for DeepLabV3+, the fused low-resolution loss.  At 128x128 the
planner picks other kernels and tiles than here (256x128 tiles on eight waves, the XCD remap of 2048-block grids, the
persistent-kernel cut-offs, weight-gradient pixel splits with their slab reduction); this is the per-call net under the -mp
kernels at the shapes they are benchmarked at.

Every call is recomputed on the CPU in fp64 from its own device inputs (tests/opcheck.py: poisoned outputs, per-channel
figures, deferred slab reductions compared after the reduce, launch census).  The bounds are those of the half-policy
every-call test at 128x128 (tests/test_half_models_gpu.py), imported, not restated:
  * CALL_TOL for every fp16 result, tensor-wide and per channel (one fp16 rounding of the result + fp32 accumulation);
  * F32_CALL_TOL for what the kernels write in fp32: weight gradients, BatchNorm coefficients, dgamma / dbeta, the class
    logits of the classifier conv;
  * the fused loss as at op level (tests/test_ops_gpu.py): loss 1e-5 relative, pixel counts exact, gradient 2e-5;
  * bit-exact results (fp16 filter copies, the loss-scaled conversion, counts of unwritten elements): zero.
HRNet runs with PSEG_DEFER_SLABS=1, so its split weight gradients park their slabs and one pseg_slab_reduce_batch folds them
(compared after that reduce); DeepLabV3+ runs with the default settings."""
import time

import pytest
import torch

from oracle import fill
from oracle import models as omodels
from test_half_models_gpu import CALL_TOL, F32_CALL_TOL

pytestmark = pytest.mark.gpu

CASES = [('deeplabv3plus', 21, 512, 16, 'cfg2h'), ('hrnet', 21, 512, 8, 'cfg4h'), ('unet', 2, 256, 8, 'cfg1h')]
# UNet's every-call run at 128x128, batch 4 (tests/test_half_models_gpu.py) records 1260 figures, 47 of them 'bn_running_stats'
# (reported only by the fused small-tensor BatchNorm launch: 35 at 256x256); the other 1213 are the same at every size
UNET_CALLS_128 = 1260 - 47
F32_OPS = ('conv2d_wgrad', 'conv2d_wgrad.ch', 'dwconv_wgrad', 'dwconv_wgrad.ch', 'bn_finalize', 'bn_act_bwd.dgamma',
           'bn_act_bwd.dbeta')
CE_UP_TOL = {'ce_upsampled.loss': 1e-5, 'ce_upsampled.count': 0.5, 'ce_upsampled.bad': 0.5, 'ce_upsampled.dlogits': 2e-5}


def _bound(op, info):
    if op in CE_UP_TOL:
        return CE_UP_TOL[op]
    if op in F32_OPS or (op in ('conv2d_fwd', 'conv2d_fwd.ch') and 'fp32-out' in info):
        return F32_CALL_TOL
    return CALL_TOL


@pytest.mark.parametrize('name,nc,S,B,key', CASES)
def test_fullsize_half_step_every_call(monkeypatch, name, nc, S, B, key):
    from opcheck import ALLOW_TRAINER_HALF, OpCheck
    from pytorch_segmentation_amd import models
    from pytorch_segmentation_amd.utils import Trainer
    if name == 'hrnet':
        monkeypatch.setenv('PSEG_DEFER_SLABS', '1')         # read when the Trainer is built
    hip_cls = {'deeplabv3plus': models.DeepLabV3Plus, 'hrnet': models.HRNet, 'unet': models.UNet}[name]
    ref = {'deeplabv3plus': omodels.DeepLabV3Plus, 'hrnet': omodels.HRNet, 'unet': omodels.UNet}[name](nc)
    fill.fill_module_(ref, key)
    m = hip_cls(nc)
    m.load_state_dict(ref.state_dict())
    del ref
    tr = Trainer(m, None, lr=1e-3, mixed_precision=True, graph=False, device=torch.device('cuda', 0))
    assert tr.env.half
    assert (tr._slab_pool is not None) == (name == 'hrnet')
    m.train()
    x = fill.images(key + '/x', (B, 3, S, S)).cuda()
    tgt = fill.labels(key + '/t', (B, S, S), nc, block=16).cuda()
    t0 = time.time()
    with OpCheck() as oc:
        tr._fwd_loss_bwd(x, tgt)
        torch.cuda.synchronize()
    wall = time.time() - t0
    tr.close()

    kinds = {}
    for op, err, info in oc.calls:
        base = op[:-3] if op.endswith('.ch') else op
        k = kinds.setdefault(base, [0, 0.0, None])
        if op.endswith('.ch'):
            k[2] = max(k[2] or 0.0, err)
        else:
            k[0] += 1
            k[1] = max(k[1], err)
    print('\nfull-size -mp every-call check [%s %dx%d B=%d]: %d checks in %.0f s' % (name, S, S, B, len(oc.calls), wall))
    print('  %-28s %6s %10s %10s' % ('op', 'calls', 'worst', 'per-chan'))
    for op, (n, e, ech) in sorted(kinds.items()):
        print('  %-28s %6d %10.2e %10s' % (op, n, e, '%.2e' % ech if ech is not None else '-'))
    print('  launches checked: %s' % dict(sorted(oc.checked.items())))
    print('  launches unchecked: %s' % dict(sorted(oc.census.items())))

    if name == 'unet':
        assert sum(1 for op, _, _ in oc.calls if op != 'bn_running_stats') >= UNET_CALLS_128
    else:
        assert len(oc.calls) > 400
    need = ['conv2d_fwd', 'conv2d_dgrad', 'conv2d_wgrad', 'bn_act_fwd', 'bn_act_bwd.dy', 'bn_finalize', 'act_to',
            'prepare_half']
    if name == 'deeplabv3plus':
        need += ['ce_upsampled.loss', 'ce_upsampled.count', 'ce_upsampled.bad', 'ce_upsampled.dlogits']
    elif name == 'hrnet':
        need += ['ce.loss', 'ce.dlogits']
    else:                       # UNet: the one model on the depthwise kernels and on ReLU6 in the fused BatchNorm kernels
        need += ['dwconv_fwd', 'dwconv_dgrad', 'dwconv_wgrad']
        assert any(op.startswith('ce') for op in kinds), sorted(kinds)
        for op in ('bn_act_fwd', 'bn_act_bwd.dy'):
            assert any(o == op and ' act2 ' in info + ' ' for o, _, info in oc.calls), op + ' act2'
    for op in need:
        assert op in kinds, op
    # the fp16 filter copies every forward conv and data gradient of the step read were checked bit for bit
    assert 'pseg_filter_prepare_h' in oc.checked and 'pseg_filter_prepare_h' not in oc.census
    if name == 'hrnet':         # the deferred reduction ran, and every parked gradient was compared after it
        assert oc.checked.get('pseg_slab_reduce_batch', 0) >= 1
        assert any(op == 'conv2d_wgrad' and info.endswith(' slabs') for op, _, info in oc.calls)
    assert oc.unchecked() == ALLOW_TRAINER_HALF, oc.census
    bad = [(op, err, info) for op, err, info in oc.calls if not err < _bound(op, info)]
    assert not bad, bad[:8]
