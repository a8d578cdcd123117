#!/usr/bin/python3
"""Training entry point with the reference's flags and `train(...)` keyword surface (reference train.py:19-21,84-140)
on the MI355X HIP path.

    python3 train.py data/<custom> [--epochs N] [-s W H] [-bs N] [-a ACC] [--lr LR] [--adam] [--resume]
                     [--weights F] [--notest] [--nosave] [--model unet|deeplabv3plus] [--augment | --augment-full | --augment-warps |
                     --augment-blends]
                     [--loss ce|lovasz|ce+lovasz|tversky|ce+tversky|ce+surface|tversky+surface|ce+tversky+surface]
                     [--class-weights W0 W1 ...] [--label-smoothing E] [--focal-gamma G] [--ohem-keep R]
                     [--tversky-alpha A] [--tversky-beta B] [--tversky-smooth S] [--tversky-power P] [--tversky-per-image]
                     [--tversky-all-classes] [--tversky-weight W]
                     [--boundary-boost A] [--boundary-loss-ratio R | --boundary-loss-width D] [--boundary-falloff flat|linear|gaussian]
                     [--boundary-sigma S]
                     [--surface-weight W] [--surface-clip D] [--surface-ramp-epochs E]
                     [--weight-decay WD] [--momentum M] [--adamw] [--no-decay-norm-bias] [--backbone-lr-mult F]
                     [--clip-grad N] [--ema-decay D] [--schedule poly|cosine] [--warmup-steps N] [--min-lr LR]
    python3 -m torch.distributed.run --nproc-per-node <n> train.py data/<custom>        # RCCL data parallel

Differences from the reference that are visible here: the model is picked with --model (the reference edits
train.py:57-59; default stays UNet), `best` is initialised so --notest without --nosave no longer raises
(SURVEY.md section 3.A.8), and -mp/--mix_precision selects the `half` policy (fp16 activations / gradients / filter copies, one fp16 MFMA pass with fp32
accumulation, fp32 master weights, device-side dynamic loss scaling) instead of apex; PSEG_MP_POLICY=limb keeps fp32 storage.
"""
import argparse
import os

# multi-process GPU work on this ROCm host: only dmabuf IPC is supported (RCCL / tensor sharing fail on the legacy mode)
os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
import os.path as osp
import sys

import torch
import torch.distributed as dist
from torch.utils.data import DataLoader, DistributedSampler

from pytorch_segmentation_amd.models import DeepLabV3Plus, HRNet, UNet
from pytorch_segmentation_amd.utils import Fetcher, Trainer, compute_loss, make_loss
from pytorch_segmentation_amd.utils.augment import DeviceAugment
from pytorch_segmentation_amd.utils.datasets import CocoInstance
from test import test

MODELS = {'deeplabv3plus': DeepLabV3Plus, 'unet': UNet, 'hrnet': HRNet}
# what train() minimises: main() sets it from --loss (train()'s keyword surface is the reference's and stays as it is);
# the validation loss test.py reports is cross-entropy whatever is chosen here
LOSS_FN = compute_loss
# --surface-ramp-epochs: the schedule behind the surface term's weight (SurfaceRamp), or None; train() hands it the Trainer
SURFACE_RAMP = None
# --class-weights as given, or None: train() checks their number against the data set's classes
CLASS_WEIGHTS = None
# optimiser recipe: Trainer keywords main() fills from --weight-decay ... --min-lr (optim_from_options); empty = the
# Trainer's defaults, as before.  'total_steps' is worked out in train() once the loader's length is known.
OPTIM = {}


class SurfaceRamp:
    """The surface term's weight as a zero-argument callable: W * min(1, (epoch + 1) / E) during the 0-based epoch of
    `trainer` (Kervadec's rebalancing in its simplest form), W before a trainer is attached."""

    def __init__(self, weight, epochs):
        self.weight, self.epochs, self.trainer = float(weight), int(epochs), None

    def __call__(self):
        if self.trainer is None:
            return self.weight
        return self.weight * min(1.0, (self.trainer.epoch + 1) / self.epochs)


def _loader(dataset, batch_size, num_workers, train=True):
    distributed = dist.is_available() and dist.is_initialized()
    sampler = DistributedSampler(dataset, dist.get_world_size(), dist.get_rank(), shuffle=train) if distributed else None
    # training: drop the short last batch (train-mode BatchNorm needs more than one sample per step).  Evaluation uses
    # the running statistics, so EVERY validation image is scored, as in the reference (train.py:45-53).
    return DataLoader(dataset, batch_size=batch_size, shuffle=train and sampler is None, sampler=sampler, pin_memory=True,
                      num_workers=num_workers, drop_last=train)


def train(data_dir, epochs=100, img_size=(320, 320), batch_size=32, accumulate=2, lr=1e-3, adam=False, resume=False,
          weights='', num_workers=4, multi_scale=False, rect=False, mixed_precision=False, notest=False, nosave=False,
          model_name='unet', augment=False):
    # --augment: the training batches (never the validation ones) go through the on-device augmentation kernel; True =
    # the reference's values, or a DeviceAugment of the caller's own (seeded, other ranges; --augment-full: DeviceAugment.full(),
    # --augment-warps: DeviceAugment.warps(), --augment-blends: DeviceAugment.blends())
    if augment and not isinstance(augment, DeviceAugment):
        augment = DeviceAugment.reference()
    train_data = CocoInstance(osp.join(data_dir, 'train.json'), img_size=list(img_size), multi_scale=multi_scale,
                              rect=rect, augments=augment or None)
    train_fetcher = Fetcher(_loader(train_data, batch_size, num_workers), train_data.post_fetch_fn)
    val_fetcher = None
    if not notest:
        val_data = CocoInstance(osp.join(data_dir, 'val.json'), img_size=list(img_size), augments=None, rect=rect)
        val_fetcher = Fetcher(_loader(val_data, batch_size, num_workers, train=False), post_fetch_fn=val_data.post_fetch_fn)
    if CLASS_WEIGHTS is not None and len(CLASS_WEIGHTS) != len(train_data.classes):
        raise ValueError('--class-weights has %d values, the data set has %d classes' % (len(CLASS_WEIGHTS), len(train_data.classes)))
    model = MODELS[model_name](len(train_data.classes))
    optim = dict(OPTIM)
    if optim.get('schedule') is not None:
        optim['total_steps'] = epochs * (len(train_fetcher) // max(1, accumulate))
    trainer = Trainer(model, train_fetcher, loss_fn=LOSS_FN, workdir='weights', accumulate=accumulate, adam=adam,
                      lr=lr, weights=weights, resume=resume, mixed_precision=mixed_precision, **optim)
    if SURFACE_RAMP is not None:
        SURFACE_RAMP.trainer = trainer
    use_ema = optim.get('ema_decay', 0.0) > 0
    last_loss = None
    while trainer.epoch < epochs:
        last_loss = trainer.step()
        print('epoch %d: loss %g' % (trainer.epoch, last_loss))
        best = False
        if val_fetcher is not None:
            if use_ema:         # the averaged weights are the ones scored, and the ones best.pt is chosen by
                with trainer.ema_weights():
                    metrics = test(trainer.model, val_fetcher)
            else:
                metrics = test(trainer.model, val_fetcher)
            if metrics > trainer.metrics:
                best = True
                print('save best, miou: %g' % metrics)
                trainer.metrics = metrics
        if not nosave:
            trainer.save(best)
    return trainer, last_loss


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument('data', type=str, default='data/voc')
    ap.add_argument('--epochs', type=int, default=100)
    ap.add_argument('-s', '--img_size', type=int, nargs=2, default=[320, 320])
    ap.add_argument('-bs', '--batch-size', type=int, default=32)
    ap.add_argument('-a', '--accumulate', type=int, default=2)
    ap.add_argument('--lr', type=float, default=1e-3)
    ap.add_argument('--adam', action='store_true')
    ap.add_argument('--resume', action='store_true')
    ap.add_argument('--weights', type=str, default='')
    ap.add_argument('--num-workers', type=int, default=4)
    ap.add_argument('--multi-scale', action='store_true')
    ap.add_argument('--rect', action='store_true')
    ap.add_argument('-mp', '--mix_precision', action='store_true', help='mixed precision')
    ap.add_argument('--notest', action='store_true')
    ap.add_argument('--nosave', action='store_true')
    ap.add_argument('--backend', type=str, default='nccl')
    ap.add_argument('--local-rank', '--local_rank', type=int, default=int(os.environ.get('LOCAL_RANK', 0)))
    ap.add_argument('--model', choices=sorted(MODELS), default='unet')
    ap.add_argument('--augment', action='store_true',
                    help='on-device training augmentation (flips, crop-and-pad, affine, colour): the affine part of the '
                         "reference's TRAIN_AUGS, utils/augment.py")
    ap.add_argument('--augment-full', action='store_true',
                    help='--augment plus blur, sharpen, emboss, Gaussian noise and (coarse) dropout: DeviceAugment.full()')
    ap.add_argument('--augment-warps', action='store_true',
                    help='--augment-full plus elastic, piecewise-affine and perspective warps of images and labels: '
                         'DeviceAugment.warps()')
    ap.add_argument('--augment-blends', action='store_true',
                    help='--augment-warps plus the median blur, the edge-detect and frequency-noise blends and hue / saturation: '
                         'DeviceAugment.blends()')
    ap.add_argument('--loss', choices=['ce', 'lovasz', 'ce+lovasz', 'tversky', 'ce+tversky', 'ce+surface', 'tversky+surface',
                                       'ce+tversky+surface'], default='ce',
                    help='training objective: per-pixel cross-entropy, the Lovasz-softmax surrogate of the mean IoU '
                         '(classes present in the batch), or their sum; the soft Dice / Tversky / focal-Tversky '
                         'region-overlap loss, or cross-entropy plus --tversky-weight times it; ...+surface adds '
                         "--surface-weight times Kervadec's surface (boundary-distance) loss to any of these")
    ap.add_argument('--class-weights', type=float, nargs='+', default=None, metavar='W',
                    help='per-class weights of the cross-entropy, one value per class (ce and ce+lovasz)')
    ap.add_argument('--label-smoothing', type=float, default=0.0, metavar='E', help='label smoothing of the cross-entropy, in [0, 1)')
    ap.add_argument('--focal-gamma', type=float, default=0.0, metavar='G',
                    help='focal modulation (1 - p_t)^G of the cross-entropy: 0 (off) or a value in [1, 8]')
    ap.add_argument('--ohem-keep', type=float, default=1.0, metavar='R',
                    help='online hard-example mining: average the cross-entropy over the share R in (0, 1] of the valid '
                         'pixels of a batch with the largest loss')
    ap.add_argument('--tversky-alpha', type=float, default=0.5, metavar='A',
                    help='weight of the soft false positives in the Tversky index (0.5 with --tversky-beta 0.5: soft Dice)')
    ap.add_argument('--tversky-beta', type=float, default=0.5, metavar='B',
                    help='weight of the soft false negatives (above --tversky-alpha: misses cost more than false alarms)')
    ap.add_argument('--tversky-smooth', type=float, default=1.0, metavar='S', help='added to numerator and denominator, >= 0')
    ap.add_argument('--tversky-power', type=float, default=1.0, metavar='P',
                    help='focal-Tversky exponent on 1 - index, in [0.5, 4] (Abraham & Khan: 1 / gamma = 0.75)')
    ap.add_argument('--tversky-per-image', action='store_true', help='one index per image and class, not per batch and class')
    ap.add_argument('--tversky-all-classes', action='store_true',
                    help='average over every class, not only over the classes present in the batch (image)')
    ap.add_argument('--tversky-weight', type=float, default=1.0, metavar='W', help='ce+tversky: ce + W * tversky')
    ap.add_argument('--boundary-boost', type=float, default=0.0, metavar='A',
                    help='weight the cross-entropy of ce, ce+lovasz and ce+tversky by 1 + A * falloff(distance to the nearest '
                         "label change of the target) inside a band along the target's contours (0: off)")
    band = ap.add_mutually_exclusive_group()
    band.add_argument('--boundary-loss-ratio', type=float, default=None, metavar='R',
                      help="width of that band as a share of the target's diagonal (default 0.02, the evaluation's rule)")
    band.add_argument('--boundary-loss-width', type=int, default=None, metavar='D', help='width of that band in pixels')
    ap.add_argument('--boundary-falloff', choices=['flat', 'linear', 'gaussian'], default='gaussian',
                    help='how the extra weight decays from the contour to the edge of the band')
    ap.add_argument('--boundary-sigma', type=float, default=None, metavar='S',
                    help='sigma of the gaussian falloff in pixels (default: a third of the width)')
    ap.add_argument('--surface-weight', type=float, default=None, metavar='W',
                    help='...+surface: weight of the surface term, >= 0 (default 0.01)')
    ap.add_argument('--surface-clip', type=float, default=None, metavar='D',
                    help='limit the signed distance of the surface term to [-D, D] pixels (default 0: no limit)')
    ap.add_argument('--surface-ramp-epochs', type=int, default=None, metavar='E',
                    help='raise the surface weight linearly to W over the first E epochs: W * min(1, (epoch + 1) / E) (default 0: off)')
    ap.add_argument('--weight-decay', type=float, default=None, metavar='WD', help='weight decay (default 0)')
    ap.add_argument('--momentum', type=float, default=None, metavar='M', help='SGD momentum (default 0.9)')
    ap.add_argument('--adamw', action='store_true', help='decoupled weight decay (AdamW with --adam, SGDW without)')
    ap.add_argument('--no-decay-norm-bias', action='store_true', help='no weight decay on BatchNorm parameters and biases')
    ap.add_argument('--backbone-lr-mult', type=float, default=None, metavar='F',
                    help="factor on the learning rate of the parameters under 'backbone.' (e.g. 0.1 for a pretrained one)")
    ap.add_argument('--clip-grad', type=float, default=0.0, metavar='N', help='clip the global gradient norm to N (0: off)')
    ap.add_argument('--ema-decay', type=float, default=0.0, metavar='D',
                    help='exponential moving average of the weights with decay D in [0, 1): validated, chosen as best.pt by, '
                         "and saved as 'model_ema' (0: off)")
    ap.add_argument('--schedule', choices=['poly', 'cosine'], default=None, help='learning-rate schedule over all epochs')
    ap.add_argument('--warmup-steps', type=int, default=0, metavar='N', help='linear warm-up over the first N optimiser steps')
    ap.add_argument('--min-lr', type=float, default=0.0, help='floor of the schedule')
    return ap


def optim_from_options(opt):
    """Trainer keywords of the parsed optimiser flags; {} when none is given"""
    kw = {}
    if opt.weight_decay is not None:
        kw['weight_decay'] = opt.weight_decay
    if opt.momentum is not None:
        kw['momentum'] = opt.momentum
    if opt.adamw:
        kw['adamw'] = True
    if opt.no_decay_norm_bias:
        kw['no_decay_norm_bias'] = True
    if opt.backbone_lr_mult is not None:
        kw['lr_mult'] = {'backbone.': opt.backbone_lr_mult}
    if opt.clip_grad < 0:
        raise ValueError('--clip-grad must be >= 0; got %g' % opt.clip_grad)
    if opt.clip_grad > 0:
        kw['max_grad_norm'] = opt.clip_grad
    if not 0.0 <= opt.ema_decay < 1.0:
        raise ValueError('--ema-decay must be in [0, 1); got %g' % opt.ema_decay)
    if opt.ema_decay > 0:
        kw['ema_decay'] = opt.ema_decay
    if opt.schedule is not None:
        kw.update(schedule=opt.schedule, warmup_steps=opt.warmup_steps, min_lr=opt.min_lr)
    elif opt.warmup_steps or opt.min_lr:
        raise ValueError('--warmup-steps and --min-lr belong to --schedule')
    return kw


def loss_from_options(opt):
    """(loss_fn, class weights or None) of the parsed --loss / --class-weights / --label-smoothing / --focal-gamma /
    --ohem-keep / --tversky-* / --boundary-* / --surface-*; with none of them given this is make_loss(opt.loss), as before.
    With --surface-ramp-epochs the surface weight is a SurfaceRamp, kept in SURFACE_RAMP for train() to attach the Trainer."""
    global SURFACE_RAMP
    SURFACE_RAMP = None
    surface = {}
    given = [flag for flag, v in (('--surface-weight', opt.surface_weight), ('--surface-clip', opt.surface_clip),
                                  ('--surface-ramp-epochs', opt.surface_ramp_epochs)) if v is not None]
    if given and 'surface' not in opt.loss:
        raise ValueError("%s: the surface options do not apply to --loss %s (use 'ce+surface', 'tversky+surface' or "
                         "'ce+tversky+surface')" % (', '.join(given), opt.loss))
    if opt.surface_weight is not None:
        if not opt.surface_weight >= 0:
            raise ValueError('--surface-weight must be >= 0; got %g' % opt.surface_weight)
        surface['surface_weight'] = opt.surface_weight
    if opt.surface_clip is not None:
        if not opt.surface_clip >= 0:
            raise ValueError('--surface-clip must be >= 0; got %g' % opt.surface_clip)
        surface['surface_clip'] = opt.surface_clip
    if opt.surface_ramp_epochs is not None:
        if opt.surface_ramp_epochs < 0:
            raise ValueError('--surface-ramp-epochs must be >= 0; got %d' % opt.surface_ramp_epochs)
        if opt.surface_ramp_epochs > 0:
            SURFACE_RAMP = SurfaceRamp(surface.get('surface_weight', 0.01), opt.surface_ramp_epochs)
            surface['surface_weight'] = SURFACE_RAMP
    boundary = {'boundary_boost': opt.boundary_boost, 'boundary_falloff': opt.boundary_falloff}
    if opt.boundary_loss_ratio is not None:
        boundary['boundary_ratio'] = opt.boundary_loss_ratio
    if opt.boundary_loss_width is not None:
        if not 1 <= opt.boundary_loss_width <= 254:
            raise ValueError('--boundary-loss-width must be in [1, 254]; got %d' % opt.boundary_loss_width)
        boundary['boundary_width'] = opt.boundary_loss_width
    if opt.boundary_sigma is not None:
        if not opt.boundary_sigma > 0:
            raise ValueError('--boundary-sigma must be > 0; got %g' % opt.boundary_sigma)
        boundary['boundary_sigma'] = opt.boundary_sigma
    return make_loss(opt.loss, class_weight=opt.class_weights, label_smoothing=opt.label_smoothing,
                     focal_gamma=opt.focal_gamma, keep_ratio=opt.ohem_keep, tversky_alpha=opt.tversky_alpha,
                     tversky_beta=opt.tversky_beta, tversky_smooth=opt.tversky_smooth, tversky_power=opt.tversky_power,
                     tversky_per_image=opt.tversky_per_image, tversky_all_classes=opt.tversky_all_classes,
                     tversky_weight=opt.tversky_weight, **boundary, **surface), opt.class_weights


def main():
    global LOSS_FN, CLASS_WEIGHTS, OPTIM
    opt = build_parser().parse_args()
    LOSS_FN, CLASS_WEIGHTS = loss_from_options(opt)
    OPTIM = optim_from_options(opt)

    if os.environ.get('WORLD_SIZE'):
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        dist.init_process_group(backend=opt.backend, init_method='env://', world_size=int(os.environ['WORLD_SIZE']),
                                rank=int(os.environ['RANK']))
    torch.cuda.set_device(opt.local_rank)
    os.environ.setdefault('LOCAL_RANK', str(opt.local_rank))
    if opt.local_rank > 0:
        sys.stdout = open(os.devnull, 'w')
    print(opt)
    train(opt.data, opt.epochs, opt.img_size, opt.batch_size, opt.accumulate, opt.lr, opt.adam, opt.resume, opt.weights,
          opt.num_workers, opt.multi_scale, opt.rect, opt.mix_precision, opt.notest, opt.nosave, opt.model,
          DeviceAugment.blends() if opt.augment_blends else DeviceAugment.warps() if opt.augment_warps else DeviceAugment.full() if opt.augment_full else opt.augment)
    if dist.is_available() and dist.is_initialized():
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
