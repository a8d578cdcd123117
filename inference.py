#!/usr/bin/python3
"""Inference entry point with the reference's flags (reference inference.py:41-58) on the MI355X HIP path.

    python3 inference.py data/samples outputs --weights weights.pth [-s W H] [-nc N] [-bs N] [--model ...] [-mp]
                         [--norm dataset|reference] [--scales S [S ...]] [--flip]
                         [--min-area N] [--connectivity {4,8}] [--largest-only] [--regions FILE.json]
                         [--polygons] [--coco FILE.json]
                         [--slide [--stride SW SH] [--window-batch N]] [--ema]
                         [--crf [--crf-radius R] [--crf-dilation D] [--crf-iters T] [--crf-theta A B G] [--crf-weights WA WS]]

Every file of img_dir whose extension is in IMG_EXT (case-sensitive, as the reference) is segmented, in name order, and
written to output_dir as <name>.png in VOC colours.  Photos are decoded with PIL (RGB); resizing, normalisation, softmax,
the resize of the probabilities to each photo's size and the argmax run on the device (utils/inference.py), -bs photos
per batch.  Unlike the reference, output_dir is created but never emptied: deleting a directory the user names is not
something an inference tool should do.  --show is accepted and ignored (the reference never used it either).
--scales and --flip turn on test-time ensembling: the class probabilities of every scale of the model input (sizes in
multiples of 32), and with --flip of the left-right mirrored photo as well, are summed at the photo's size before the argmax.
--min-area N drops connected regions of fewer than N pixels (specks take their surroundings' class, holes are filled),
--largest-only keeps the largest region of every class but background, --connectivity chooses 4- or 8-neighbour regions
(utils/regions.py); the PNGs show the cleaned masks.  --regions FILE.json writes {file name: [region, ...]} for the whole
folder: class, area, bbox, centroid, angle, sides and label of every region of the (cleaned) mask.
--polygons adds every region's outline to that file: polygon (flat [x0, y0, x1, y1, ...] rings on the pixel lattice, the
outer ring first, then the holes), perimeter and min_rect (the minimum-area enclosing rectangle).  --coco FILE.json writes
the regions of every class but background as COCO annotations in the layout utils/datasets.py reads; a COCO polygon
cannot express holes, so only the outer ring goes there (--regions keeps them).
--slide does not squeeze a photo into -s W H: the model runs on overlapping W x H windows (multiples of 32) laid over the
photo at its own size -- with --scales over the photo scaled by each factor -- at --stride SW SH (default 2/3 of the
window), the class probabilities of the windows covering a pixel are averaged and the argmax is taken; --window-batch N
windows go through the model at a time (default: the photos of a batch).
--crf refines the logits of every forward -- on any of the routes above -- by a local dense CRF guided by the model input
(utils/crf.py, csrc/crf.hip) before the softmax and the decode: label changes snap to colour edges, specks go.  --crf-radius
R (1 .. 5, default 3) and --crf-dilation D (1 .. 4, default 2) set the window, (2R+1) x (2R+1) taps D pixels apart at the
model input's resolution; --crf-iters T (1 .. 10, default 5) the mean-field iterations; --crf-theta A B G (default 8 13 3) the
appearance kernel's spatial and colour widths and the smoothness kernel's spatial width; --crf-weights WA WS (default 4 3)
the two kernels' weights in logit units.
"""
import argparse
import json
import os
import os.path as osp

import numpy as np
import torch
from PIL import Image

from pytorch_modules.utils import IMG_EXT
from pytorch_segmentation_amd.models import DeepLabV3Plus, HRNet, UNet
from pytorch_segmentation_amd.utils.datasets import VOC_COLORMAP, _warn_ignored
from pytorch_segmentation_amd.utils.inference import NORMS, inference

MODELS = {'deeplabv3plus': DeepLabV3Plus, 'unet': UNet, 'hrnet': HRNet}
# VOC_COLORMAP rows are [b, g, r] for cv2.imwrite (reference inference.py:35-37); PIL writes RGB
PALETTE_RGB = np.ascontiguousarray(VOC_COLORMAP[:, ::-1])


def list_images(img_dir):
    return sorted(n for n in os.listdir(img_dir) if osp.splitext(n)[1] in IMG_EXT)


def load_image(path):
    return np.asarray(Image.open(path).convert('RGB'), dtype=np.uint8)


def run(img_dir, output_dir, img_size, num_classes, weights, show=False, model_name='deeplabv3plus', batch_size=1,
        half=False, norm='dataset', scales=None, flip=False, min_area=0, connectivity=8, largest_only=False, regions=None,
        slide=False, stride=None, window_batch=None, ema=False, polygons=False, coco=None, crf=None):
    if not slide and (stride is not None or window_batch is not None):
        raise ValueError('--stride and --window-batch need --slide')
    if min_area < 0:
        raise ValueError('--min-area must be >= 0; got %d' % min_area)
    if connectivity not in (4, 8):
        raise ValueError('--connectivity must be 4 or 8; got %r' % (connectivity,))
    if polygons and not (regions or coco):
        raise ValueError('--polygons needs --regions or --coco')
    polygons = bool(polygons or coco)
    if crf is not None and crf is not False:
        from pytorch_segmentation_amd.utils.crf import CRF
        crf = CRF.of(crf)                                      # bad options are refused before the weights are read
    if show:
        _warn_ignored('--show', 'the reference accepts it and never displays anything either')
    os.makedirs(output_dir, exist_ok=True)
    model = MODELS[model_name](num_classes)
    state_dict = torch.load(weights, map_location='cpu')
    if ema and 'model_ema' not in state_dict:
        raise KeyError("--ema: %s holds no 'model_ema' (it was not trained with --ema-decay)" % weights)
    model.load_state_dict(state_dict['model_ema' if ema else 'model'])
    model = model.cuda()
    model.eval()
    names = list_images(img_dir)
    tta = {} if scales is None and not flip else {'scales': scales, 'flip': bool(flip)}
    if slide:
        tta.update(slide=True, stride=None if stride is None else tuple(stride), window_batch=window_batch)
    if min_area > 1 or largest_only or regions or coco:
        tta.update(min_area=min_area, connectivity=connectivity, largest_only=bool(largest_only), regions=bool(regions or coco))
    if polygons:
        tta.update(polygons=True)
    if crf:
        tta.update(crf=crf)
    found, sizes = {}, {}
    for i in range(0, len(names), max(1, batch_size)):
        batch = names[i:i + max(1, batch_size)]
        imgs = [load_image(osp.join(img_dir, n)) for n in batch]
        result = inference(model, imgs, tuple(img_size), norm=norm, bgr=False, half=half, colors=PALETTE_RGB, **tta)
        colored = result[1]
        if regions or coco:
            found.update(zip(batch, result[2]))
            sizes.update((n, im.shape[:2]) for n, im in zip(batch, imgs))
        for name, seg in zip(batch, colored):
            Image.fromarray(seg).save(osp.join(output_dir, osp.splitext(name)[0] + '.png'))
        print('%d/%d' % (min(i + batch_size, len(names)), len(names)), flush=True)
    if regions:
        with open(regions, 'w') as f:
            json.dump(found, f)
    if coco:
        from pytorch_segmentation_amd.utils.regions import coco_annotations
        with open(coco, 'w') as f:
            json.dump(coco_annotations(found, sizes, num_classes), f)
    return names


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('img_dir', type=str)
    parser.add_argument('output_dir', type=str)
    parser.add_argument('-s', '--img_size', type=int, nargs=2, default=[320, 320])
    parser.add_argument('-nc', '--num-classes', type=int, default=2)
    parser.add_argument('--weights', type=str, default='weights/best.pt')
    parser.add_argument('--show', action='store_true', help='accepted and ignored')
    parser.add_argument('--model', choices=sorted(MODELS), default='deeplabv3plus')
    parser.add_argument('-bs', '--batch-size', type=int, default=1)
    parser.add_argument('-mp', '--mix_precision', action='store_true', help='half-precision forward')
    parser.add_argument('--norm', choices=sorted(NORMS), default='dataset',
                        help="'dataset': the training loader's mean/std (default); 'reference': /255 as the reference")
    parser.add_argument('--scales', type=float, nargs='+', default=None, metavar='S',
                        help='test-time ensembling: factors on --img_size (sizes in multiples of 32), e.g. 0.5 1.0 1.5')
    parser.add_argument('--flip', action='store_true', help='test-time ensembling: add the left-right mirrored view')
    parser.add_argument('--min-area', type=int, default=0, metavar='N',
                        help='drop connected regions of fewer than N pixels (they take the class of the region above them)')
    parser.add_argument('--connectivity', type=int, choices=[4, 8], default=8, help='neighbours that connect a region')
    parser.add_argument('--largest-only', action='store_true', help='keep only the largest region of every class >= 1')
    parser.add_argument('--regions', type=str, default=None, metavar='FILE.json',
                        help='write {file name: [region, ...]} (class, area, bbox, centroid, angle, sides, label)')
    parser.add_argument('--polygons', action='store_true',
                        help='with --regions or --coco: add polygon, perimeter and min_rect to every region')
    parser.add_argument('--coco', type=str, default=None, metavar='FILE.json',
                        help='write the regions of every class >= 1 as COCO polygon annotations (outer rings; holes are dropped)')
    parser.add_argument('--slide', action='store_true',
                        help='sliding-window inference: -s W H is the window (multiples of 32) laid over the photo at its own '
                             'size; --scales then scale the photo')
    parser.add_argument('--stride', type=int, nargs=2, default=None, metavar=('SW', 'SH'),
                        help='with --slide: the window stride, between half the window and the window (default: 2/3 of it)')
    parser.add_argument('--window-batch', type=int, default=None, metavar='N',
                        help='with --slide: windows per forward (default: -bs)')
    parser.add_argument('--ema', action='store_true', help="use the averaged weights ('model_ema') of the checkpoint")
    # (argparse.SUPPRESS: without the flags the options printed below are what they were)
    parser.add_argument('--crf', action='store_true', default=argparse.SUPPRESS,
                        help='refine the logits of every forward by the local dense CRF (utils/crf.py) before the decode')
    parser.add_argument('--crf-radius', type=int, default=argparse.SUPPRESS, metavar='R',
                        help='with --crf: window radius in taps, 1 .. 5 (default 3)')
    parser.add_argument('--crf-dilation', type=int, default=argparse.SUPPRESS, metavar='D',
                        help='with --crf: pixels between taps, 1 .. 4 (default 2)')
    parser.add_argument('--crf-iters', type=int, default=argparse.SUPPRESS, metavar='T',
                        help='with --crf: mean-field iterations, 1 .. 10 (default 5)')
    parser.add_argument('--crf-theta', type=float, nargs=3, default=argparse.SUPPRESS, metavar=('A', 'B', 'G'),
                        help='with --crf: theta_alpha, theta_beta, theta_gamma (default 8 13 3)')
    parser.add_argument('--crf-weights', type=float, nargs=2, default=argparse.SUPPRESS, metavar=('WA', 'WS'),
                        help='with --crf: appearance and smoothness weights in logit units (default 4 3)')
    opt = parser.parse_args(argv)
    if opt.min_area < 0:
        parser.error('--min-area must be >= 0')
    if not opt.slide and (opt.stride is not None or opt.window_batch is not None):
        parser.error('--stride and --window-batch need --slide')
    if opt.window_batch is not None and opt.window_batch < 1:
        parser.error('--window-batch must be >= 1')
    if opt.polygons and not (opt.regions or opt.coco):
        parser.error('--polygons needs --regions or --coco')
    crf = None
    crf_flags = [getattr(opt, 'crf_' + k, None) for k in ('radius', 'dilation', 'iters', 'theta', 'weights')]
    if getattr(opt, 'crf', False) or any(v is not None for v in crf_flags):
        from pytorch_segmentation_amd.utils.crf import from_flags
        try:
            crf = from_flags(getattr(opt, 'crf', False), *crf_flags)
        except ValueError as e:
            parser.error(str(e))
    print(opt)
    run(opt.img_dir, opt.output_dir, opt.img_size, opt.num_classes, opt.weights, opt.show, opt.model, opt.batch_size,
        opt.mix_precision, opt.norm, opt.scales, opt.flip, opt.min_area, opt.connectivity, opt.largest_only, opt.regions,
        opt.slide, opt.stride, opt.window_batch, opt.ema, opt.polygons, opt.coco, crf)


if __name__ == '__main__':
    main()
