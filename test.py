#!/usr/bin/python3
"""Evaluation entry point with the reference's flags (reference test.py:76-105) on the MI355X HIP path.

    python3 test.py data/<custom>/val.json --weights weights/best.pt [-s W H] [-bs N] [--model deeplabv3plus|unet]
                    [--scales S [S ...]] [--flip] [--min-area N] [--connectivity {4,8}] [--largest-only]
                    [--window W H [--stride SW SH]] [--ema] [--boundary [RATIO] | --boundary-width D]
                    [--crf [--crf-radius R] [--crf-dilation D] [--crf-iters T] [--crf-theta A B G] [--crf-weights WA WS]]
                    [--surface-distance [--hd-percentile P] [--surface-tolerance T]]

`test(model, fetcher)` keeps the reference's contract: evaluates in eval mode without gradients, prints per-class
(or the five worst classes') targets / precision / recall / IoU / F1 and returns the mean IoU.  The per-class
tp/fn/fp bookkeeping runs as one device kernel per batch instead of 3 host synchronisations per class, and the
distributed reduction is a single [3, num_classes] all-reduce.  With --scales / --flip the counted prediction is the
test-time ensemble (utils.predict_mask_ensemble: summed class probabilities of every scale and mirrored view at the target
size); the printed loss stays that of the plain forward.  With --min-area / --largest-only the counted prediction is the
cleaned mask (utils/regions.py: small connected regions dropped) of either route, so the effect of a threshold on the mIoU
can be read off; the loss again stays as it is.  With --window W H the counted prediction is the sliding-window one
(utils.predict_mask_windows: W x H windows at --stride over the images -s delivers, the probabilities of the windows covering
a pixel averaged; --scales then scale the image, --flip adds every window's mirrored twin).
With --boundary [RATIO] or --boundary-width D the counted prediction -- whichever route made it -- is also scored near the
contours: Boundary IoU (Cheng et al. 2021) and the trimap IoU of the DeepLabV3+ paper, in a band of RATIO times the target's
diagonal (default 0.02) or of D pixels (utils.update_boundary_counts: two launches per batch, any class count).  One more
summary line and two more columns per class row are printed; everything else, the returned mean IoU included, stays.
With --crf the logits of every forward of the route in use -- plain, --scales / --flip, --window -- are refined by the local
dense CRF (utils/crf.py, csrc/crf.hip), guided by that forward's inputs, before the prediction is made; --boundary shows what
it does to the contours.  The printed loss stays that of the unrefined plain forward.
With --surface-distance the counted prediction -- whichever route made it -- is also scored by the distances between its
contours and the target's, per image and class (utils.update_surface_stats, csrc/hausdorff.hip): the Hausdorff distance, its
--hd-percentile (default 95), the average symmetric surface distance and the surface Dice within --surface-tolerance pixels
(default 2), each class's value the mean over the images that define it.  One more summary line and four more columns per
class row are printed; it composes with --boundary, and everything else, the returned mean IoU included, stays.
"""
import argparse

import torch
from torch.utils.data import DataLoader

from pytorch_segmentation_amd.models import DeepLabV3Plus, HRNet, UNet
from pytorch_segmentation_amd.utils import (Fetcher, all_reduce_counters, broadcast_buffers,
                                            compute_boundary_metrics, compute_loss, compute_metrics, predict_mask,
                                            predict_mask_ensemble, predict_mask_windows, update_boundary_counts,
                                            update_class_counts)
from pytorch_segmentation_amd.utils import boundary_width as band_width      # (test() has an argument of that name)
from pytorch_segmentation_amd.utils.datasets import CocoDataset

MODELS = {'deeplabv3plus': DeepLabV3Plus, 'unet': UNet, 'hrnet': HRNet}


@torch.no_grad()
def test(model, fetcher, scales=None, flip=False, min_area=0, connectivity=8, largest_only=False, window=None, stride=None,
         boundary=None, boundary_width=None, results=None, crf=None, surface_distance=False, hd_percentile=95.0,
         surface_tolerance=2):
    """boundary (a ratio of the target's diagonal) or boundary_width (pixels): also count Boundary IoU and trimap IoU on the
    prediction that is scored.  results: a dict that receives 'boundary_iou' and 'trimap_iou' ([C] tensors),
    'boundary_counters' (int64 [6][C], summed over the ranks) and 'boundary_widths' (the sorted widths used).
    crf (None, True, a utils.crf.CRF or a dict of its options): the counted prediction of every route is made from logits
    refined by the local dense CRF, guided by the inputs of the forward that gave them; the loss stays the plain forward's.
    surface_distance: also score the counted prediction by HD, HD at hd_percentile (percent, one decimal at most), ASSD and
    the surface Dice within surface_tolerance pixels; results receives 'hd', 'hd95', 'assd', 'nsd', 'surface_misses' (float64
    [C], NaN where no image defines the value) and 'surface_stats' (the float64 [7][C] accumulator, summed over the ranks)."""
    permille = None
    if surface_distance:
        from pytorch_segmentation_amd.utils import compute_surface_metrics, update_surface_stats
        permille = hd_permille(hd_percentile)
        if not 0 <= surface_tolerance <= 255 or int(surface_tolerance) != surface_tolerance:
            raise ValueError('surface_tolerance must be an integer in [0, 255]; got %r' % (surface_tolerance,))
    refine = None
    if crf is not None and crf is not False:
        from pytorch_segmentation_amd.utils.crf import CRF
        from pytorch_segmentation_amd.utils.datasets import STD
        crf = CRF.of(crf)
        refine = lambda logits, x: crf.refine(logits, x, STD)   # the loader normalises with MEAN / STD
    model.eval()
    if boundary is not None and boundary_width is not None:
        raise ValueError('boundary= (a ratio) and boundary_width= (pixels) exclude each other')
    if boundary is not None and not 0.0 < boundary <= 0.5:
        raise ValueError('boundary must be in (0, 0.5]; got %r' % (boundary,))
    if boundary_width is not None and not 1 <= boundary_width <= 254:
        raise ValueError('boundary_width must be in [1, 254]; got %r' % (boundary_width,))
    contours = boundary is not None or boundary_width is not None
    if window is None and stride is not None:
        raise ValueError('stride belongs to window=')
    if min_area < 0:
        raise ValueError('min_area must be >= 0; got %d' % min_area)
    if connectivity not in (4, 8):
        raise ValueError('connectivity must be 4 or 8; got %r' % (connectivity,))
    clean = min_area > 1 or largest_only
    tta = scales is not None or flip
    scales = (1.0,) if scales is None else tuple(scales)
    # distributed evaluation sums per-class counters over the ranks (reference test.py:51-58): they must all come from ONE
    # model, so every replica takes rank 0's BatchNorm running statistics first (DistributedDataParallel's broadcast_buffers)
    broadcast_buffers(model, 0)
    classes = fetcher.loader.dataset.classes
    nc = len(classes)
    if clean and nc > 256:
        raise ValueError('mask cleanup handles at most 256 classes; the dataset has %d' % nc)
    counters = None
    bcounters, widths = None, set()
    sacc = None
    loss_sum, batches = None, 0
    for inputs, targets in fetcher:
        if window is not None:                                 # sliding windows of (w, h) over the delivered batch
            predicted = predict_mask_windows(model, inputs, targets.shape[1:], (window[1], window[0]),
                                             None if stride is None else (stride[1], stride[0]), scales, flip, refine)
            outputs = model(inputs)                            # the loss stays that of the plain forward
        elif tta:
            view_logits = {}
            predicted = predict_mask_ensemble(model, inputs, targets.shape[1:], scales, flip, view_logits, refine)
            # the loss of the plain forward: the scale-1.0 unmirrored view, or one extra forward without scale 1.0
            outputs = view_logits.get(tuple(inputs.shape[2:]))
            del view_logits
            outputs = model(inputs) if outputs is None else outputs[:inputs.shape[0]]
        else:
            outputs = model(inputs)
            predicted = None
        loss = compute_loss(outputs, targets, model)
        loss_sum = loss if loss_sum is None else loss_sum + loss
        batches += 1
        if counters is None:
            counters = torch.zeros(3, nc, dtype=torch.int64, device=outputs.device)
        if predicted is None:
            predicted = predict_mask(outputs if refine is None else refine(outputs, inputs))
        if clean:
            from pytorch_segmentation_amd.utils.regions import clean_predictions
            predicted = clean_predictions(predicted, min_area, connectivity, largest_only)
        update_class_counts(counters, predicted, targets)
        if contours:
            if bcounters is None:
                bcounters = torch.zeros(6, nc, dtype=torch.int64, device=outputs.device)
            # the width follows the target size of the batch (--rect delivers more than one)
            width = band_width(targets.shape[1:], boundary) if boundary_width is None else boundary_width
            widths.add(width)
            update_boundary_counts(bcounters, predicted, targets, width)
        if surface_distance:
            if sacc is None:
                sacc = torch.zeros(7, nc, dtype=torch.float64, device=outputs.device)
            update_surface_stats(sacc, predicted, targets, permille, int(surface_tolerance))
    if counters is None:
        return 0.0
    all_reduce_counters(counters)
    tp, fn, fp = (c.float() for c in counters.cpu())
    T, P, R, miou, F1 = compute_metrics(tp, fn, fp)
    print('loss: %8g, mAP: %8g, F1: %8g, miou: %8g' % (loss_sum.item() / batches, P.mean(), F1.mean(), miou.mean()))
    row = 'cls: %8s, targets: %8d, pre: %8g, rec: %8g, iou: %8g, F1: %8g'
    if contours:
        all_reduce_counters(bcounters)
        biou, tiou = compute_boundary_metrics(bcounters)
        print('boundary iou: %8g, trimap iou: %8g, width: %s' % (biou.mean(), tiou.mean(), ' '.join(map(str, sorted(widths)))))
        if results is not None:
            results.update(boundary_iou=biou, trimap_iou=tiou, boundary_counters=bcounters.cpu(), boundary_widths=sorted(widths))
    if surface_distance:
        all_reduce_counters(sacc)
        hd, hd95, assd, nsd, misses = compute_surface_metrics(sacc)
        print('hd: %8g, hd%g: %8g, assd: %8g, nsd@%d: %8g, misses: %d'
              % (nanmean(hd), permille / 10, nanmean(hd95), nanmean(assd), surface_tolerance, nanmean(nsd), misses.sum()))
        if results is not None:
            results.update(hd=hd, hd95=hd95, assd=assd, nsd=nsd, surface_misses=misses, surface_stats=sacc.cpu())
    if nc < 10:
        order = range(nc)
    else:
        print('top error 5')
        order = torch.argsort(miou)[:5].tolist()
    for c in order:
        line = row % (classes[c], T[c], P[c], R[c], miou[c], F1[c])
        line = line + ', biou: %8g, trimap: %8g' % (biou[c], tiou[c]) if contours else line
        print(line + ', hd: %8g, hd%g: %8g, assd: %8g, nsd: %8g' % (hd[c], permille / 10, hd95[c], assd[c], nsd[c])
              if surface_distance else line)
    return miou.mean().item()


def hd_permille(percent):
    """--hd-percentile in percent, one decimal at most -> thousandths in [1, 1000]"""
    permille = int(round(float(percent) * 10))
    if abs(float(percent) * 10 - permille) > 1e-6 or not 1 <= permille <= 1000:
        raise ValueError('hd_percentile must be in [0.1, 100] with at most one decimal; got %r' % (percent,))
    return permille


def nanmean(v):
    """the mean over the classes that have a value; NaN when none has"""
    have = ~torch.isnan(v)
    return (v[have].mean() if have.any() else torch.tensor(float('nan'))).item()


def checkpoint_weights(checkpoint, ema=False, path='the checkpoint'):
    """the state dict to evaluate: 'model', or with ema the averaged weights train.py --ema-decay saved as 'model_ema'"""
    if not ema:
        return checkpoint['model']
    if 'model_ema' not in checkpoint:
        raise KeyError("--ema: %s holds no 'model_ema' (it was not trained with --ema-decay)" % path)
    return checkpoint['model_ema']


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('val', type=str)
    ap.add_argument('--weights', type=str, default='')
    ap.add_argument('--rect', action='store_true')
    ap.add_argument('-s', '--img_size', type=int, nargs=2, default=[320, 320])
    ap.add_argument('-bs', '--batch-size', type=int, default=32)
    ap.add_argument('--num-workers', type=int, default=4)
    ap.add_argument('--model', choices=sorted(MODELS), default='deeplabv3plus')
    ap.add_argument('--scales', type=float, nargs='+', default=None, metavar='S',
                    help='test-time ensembling: factors on the input size (sizes in multiples of 32), e.g. 0.5 1.0 1.5')
    ap.add_argument('--flip', action='store_true', help='test-time ensembling: add the left-right mirrored view')
    ap.add_argument('--min-area', type=int, default=0, metavar='N',
                    help='evaluate the masks with connected regions of fewer than N pixels dropped')
    ap.add_argument('--connectivity', type=int, choices=[4, 8], default=8, help='neighbours that connect a region')
    ap.add_argument('--largest-only', action='store_true', help='keep only the largest region of every class >= 1')
    ap.add_argument('--window', type=int, nargs=2, default=None, metavar=('W', 'H'),
                    help='sliding-window evaluation: W x H windows over the images the loader delivers (-s); --scales then '
                         'scale the image')
    ap.add_argument('--stride', type=int, nargs=2, default=None, metavar=('SW', 'SH'),
                    help='with --window: the window stride, between half the window and the window (default: 2/3 of it)')
    ap.add_argument('--ema', action='store_true', help="evaluate the averaged weights ('model_ema') of the checkpoint")
    contour = ap.add_mutually_exclusive_group()
    contour.add_argument('--boundary', type=float, nargs='?', const=0.02, default=None, metavar='RATIO',
                         help='also report Boundary IoU and trimap IoU in a band of RATIO (default 0.02, in (0, 0.5]) times '
                              "the target's diagonal")
    contour.add_argument('--boundary-width', type=int, default=None, metavar='D',
                         help='the same with a band of D pixels (1 .. 254)')
    ap.add_argument('--crf', action='store_true',
                    help='refine the logits of every forward by the local dense CRF (utils/crf.py) before the prediction is made')
    ap.add_argument('--crf-radius', type=int, default=None, metavar='R', help='with --crf: window radius in taps, 1 .. 5 (default 3)')
    ap.add_argument('--crf-dilation', type=int, default=None, metavar='D', help='with --crf: pixels between taps, 1 .. 4 (default 2)')
    ap.add_argument('--crf-iters', type=int, default=None, metavar='T', help='with --crf: mean-field iterations, 1 .. 10 (default 5)')
    ap.add_argument('--crf-theta', type=float, nargs=3, default=None, metavar=('A', 'B', 'G'),
                    help='with --crf: theta_alpha, theta_beta, theta_gamma (default 8 13 3)')
    ap.add_argument('--crf-weights', type=float, nargs=2, default=None, metavar=('WA', 'WS'),
                    help='with --crf: appearance and smoothness weights in logit units (default 4 3)')
    ap.add_argument('--surface-distance', action='store_true',
                    help='also report the Hausdorff distance, its percentile, the average symmetric surface distance and the '
                         'surface Dice of the counted prediction, per image and class')
    ap.add_argument('--hd-percentile', type=float, default=None, metavar='P',
                    help='with --surface-distance: the percentile of the Hausdorff distance, in (0, 100] with one decimal at '
                         'most (default 95)')
    ap.add_argument('--surface-tolerance', type=int, default=None, metavar='T',
                    help='with --surface-distance: the surface Dice tolerance in pixels, 0 .. 255 (default 2)')
    opt = ap.parse_args(argv)
    if not opt.surface_distance and (opt.hd_percentile is not None or opt.surface_tolerance is not None):
        ap.error('--hd-percentile and --surface-tolerance need --surface-distance')
    opt.hd_percentile = 95.0 if opt.hd_percentile is None else opt.hd_percentile
    opt.surface_tolerance = 2 if opt.surface_tolerance is None else opt.surface_tolerance
    try:
        hd_permille(opt.hd_percentile)
    except ValueError:
        ap.error('--hd-percentile must be in [0.1, 100] with at most one decimal')
    if not 0 <= opt.surface_tolerance <= 255:
        ap.error('--surface-tolerance must be in [0, 255]')
    crf_flags = (opt.crf_radius, opt.crf_dilation, opt.crf_iters, opt.crf_theta, opt.crf_weights)
    if not opt.crf and any(v is not None for v in crf_flags):
        ap.error('--crf-radius, --crf-dilation, --crf-iters, --crf-theta and --crf-weights need --crf')
    opt.crf_options = None
    if opt.crf:
        from pytorch_segmentation_amd.utils.crf import from_flags
        try:
            opt.crf_options = from_flags(True, *crf_flags)
        except ValueError as e:
            ap.error(str(e))
    if opt.boundary is not None and not 0.0 < opt.boundary <= 0.5:
        ap.error('--boundary must be in (0, 0.5]')
    if opt.boundary_width is not None and not 1 <= opt.boundary_width <= 254:
        ap.error('--boundary-width must be in [1, 254]')
    if opt.min_area < 0:
        ap.error('--min-area must be >= 0')
    if opt.stride is not None and opt.window is None:
        ap.error('--stride needs --window')
    return opt


def main(argv=None):
    opt = parse_args(argv)
    data = CocoDataset(opt.val, img_size=opt.img_size, augments=None, rect=opt.rect)
    loader = DataLoader(data, batch_size=opt.batch_size, pin_memory=True, num_workers=opt.num_workers)
    fetcher = Fetcher(loader, post_fetch_fn=data.post_fetch_fn)
    model = MODELS[opt.model](len(data.classes))
    if opt.weights:
        model.load_state_dict(checkpoint_weights(torch.load(opt.weights, map_location='cpu'), opt.ema, opt.weights))
    elif opt.ema:
        raise ValueError('--ema needs --weights')
    metrics = test(model.cuda(), fetcher, opt.scales, opt.flip, opt.min_area, opt.connectivity,
                   opt.largest_only, opt.window, opt.stride, opt.boundary, opt.boundary_width, crf=opt.crf_options,
                   surface_distance=opt.surface_distance, hd_percentile=opt.hd_percentile,
                   surface_tolerance=opt.surface_tolerance)
    print('metrics: %8g' % metrics)
    return metrics


if __name__ == '__main__':
    main()
