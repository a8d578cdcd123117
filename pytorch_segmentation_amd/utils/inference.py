"""Batched inference: a list of photos in, one segmentation mask per photo out (reference utils/inference.py).

The reference resizes every photo with cv2 on the host, runs the model, then -- again on the host, per photo -- takes
the softmax at model resolution, resizes the C-channel probability map to the photo's own size and takes the argmax.
Here both ends are device kernels (csrc/infer.hip): ``ops.image_preprocess`` turns the ragged batch of uint8 photos into
the model input, ``ops.seg_decode`` reads the logits once and writes one byte per photo pixel (plus three colour bytes
if a palette is given).  The host packs the photos and both size tables into ONE pinned buffer (one host-to-device
copy) and receives masks and colours in ONE device-to-host copy.

Normalisation is a decision, not a copy: ``norm='dataset'`` (default) applies the loader's MEAN / STD -- what weights
trained with train.py expect; ``norm='reference'`` divides by 255 only, as the reference's inference does although its
own training normalised with mean / std.

Test-time ensembling (``scales=``, ``flip=``): the class probabilities of several scales, each optionally with its
left-right mirrored twin, are summed at the photo's size before the argmax -- the evaluation protocol DeepLabV3+ and HRNet
figures are published with.  The size at scale s of a model input (h, w) is ``(max(32, int(h*s/32)*32), max(32,
int(w*s/32)*32))``, the training loader's multi-scale rule (``tta_sizes``); scales that give the same size are merged.  Per
scale one ``ops.image_preprocess_views`` launch makes the plain and the mirrored inputs, one forward runs, and
``ops.softmax_views`` adds a pair's two softmaxes (the twin un-mirrored) into one map of a packed buffer; one
``ops.seg_decode_ensemble`` then sums the bilinear samples of all maps per photo pixel and takes the argmax, first index
on ties.  The sum is unweighted.
"""
import math
import warnings

import numpy as np
import torch

from .. import ops
from .datasets import MEAN, STD

NORMS = {'dataset': (MEAN, STD), 'reference': ((0.0, 0.0, 0.0), (255.0, 255.0, 255.0))}


def _photo(img):
    """-> (host numpy array or device tensor, H, W) of one uint8 HWC 3-channel photo"""
    if isinstance(img, torch.Tensor):
        if not img.is_cuda:
            img = img.numpy()
    else:
        img = np.asarray(img)
    if img.ndim != 3 or img.shape[2] != 3 or img.dtype != (torch.uint8 if isinstance(img, torch.Tensor) else np.uint8):
        raise ValueError('inference() takes uint8 H x W x 3 photos; got %s %s' % (tuple(img.shape), img.dtype))
    if not 1 <= img.shape[0] <= 65535 or not 1 <= img.shape[1] <= 65535:
        raise ValueError('photo size %dx%d outside [1, 65535]' % (img.shape[0], img.shape[1]))
    return img, int(img.shape[0]), int(img.shape[1])


def lut_of(colors):
    """[N, 3] uint8 palette -> the decode kernel's 256-entry table; classes >= N are black (reference inference.py:33-35)"""
    lut = np.zeros((256, 3), dtype=np.uint8)
    colors = np.asarray(colors, dtype=np.uint8).reshape(-1, 3)[:256]
    lut[:len(colors)] = colors
    return lut


def tta_sizes(h, w, scales):
    """The distinct (h_s, w_s) of a model input (h, w) at `scales`, in first-seen order: the training loader's multi-scale
    rule, sizes in multiples of 32.  Scales must be finite and > 0; scales that give the same size are merged with a
    warning; at most ops.ENSEMBLE_MAX_MAPS sizes."""
    scales = [float(s) for s in scales]
    if not scales:
        raise ValueError('scales is empty')
    sizes = []
    for s in scales:
        if not math.isfinite(s) or s <= 0:
            raise ValueError('scales must be finite and > 0; got %r' % (s,))
        hw = (max(32, int(h * s / 32) * 32), max(32, int(w * s / 32) * 32))
        if hw in sizes:
            warnings.warn('scale %g gives the model input size %dx%d of an earlier scale; merged' % (s, hw[0], hw[1]),
                          RuntimeWarning, stacklevel=3)
        else:
            sizes.append(hw)
    if len(sizes) > ops.ENSEMBLE_MAX_MAPS:
        raise ValueError('%d distinct sizes; at most %d scales are ensembled' % (len(sizes), ops.ENSEMBLE_MAX_MAPS))
    return sizes


def map_offsets(B, sizes):
    """-> (pixel offset of each scale's [B,h_s,w_s] map in the packed buffer, pixels in all); times ops.class_pad(C) = floats"""
    cells = [B * hs * ws for hs, ws in sizes]
    return [sum(cells[:i]) for i in range(len(cells))], sum(cells)


class Ensemble:
    """The packed probability maps of one batch: ``add`` each scale's logits in the order of `sizes`, then ``decode``.
    dmaps (optional): int64 device tensor [S,3] of {PIXEL offset (map_offsets), h_s, w_s} that travelled with the caller's
    own host-to-device copy; it is turned into float offsets in place once the class count is known.  Without it the
    table is built and copied at the first ``add``.  The buffer is sized once, at the first ``add``."""

    def __init__(self, B, sizes, pairs, dmaps=None):
        assert 1 <= len(sizes) <= ops.ENSEMBLE_MAX_MAPS
        self.B, self.sizes, self.pairs, self.dmaps = B, list(sizes), bool(pairs), dmaps
        self.offsets, self.cells = map_offsets(B, self.sizes)
        self.prob, self.C, self.CP, self.n = None, None, None, 0

    def add(self, logits):
        n, C, hs, ws = logits.shape
        assert self.n < len(self.sizes) and (hs, ws) == self.sizes[self.n] and n == self.B * (2 if self.pairs else 1)
        if self.prob is None:
            self.C, self.CP = C, ops.class_pad(C)
            self.prob = torch.empty(self.cells * self.CP, dtype=torch.float32, device=logits.device)
            if self.dmaps is None:
                rows = [[o * self.CP, hs_, ws_] for o, (hs_, ws_) in zip(self.offsets, self.sizes)]
                self.dmaps = torch.tensor(rows, dtype=torch.int64).to(logits.device)
            else:
                self.dmaps[:, 0] *= self.CP         # device arithmetic on S numbers: no host round trip
        assert C == self.C
        ops.softmax_views(logits.contiguous(), self.prob, self.offsets[self.n] * self.CP, self.pairs)
        self.n += 1

    def decode(self, table, npix_total, max_hw, lut=None, out=None):
        assert self.n == len(self.sizes)
        return ops.seg_decode_ensemble(self.prob, self.dmaps, self.B, self.C, table, npix_total, max_hw, lut, out)


@torch.no_grad()
def inference(model, imgs, img_size=(64, 64), norm='dataset', bgr=True, half=False, colors=None, scales=None, flip=False,
              min_area=0, connectivity=8, largest_only=False, regions=False, slide=False, stride=None, window_batch=None,
              polygons=False, crf=None):
    """The reference's contract: ``imgs`` is a list of uint8 H x W x 3 photos (numpy arrays, or CPU or device tensors),
    ``img_size`` = (w, h) of the model input as cv2.resize takes it; returns one int64 numpy H x W mask per photo, at
    that photo's own size.  ``bgr=True``: the photos are cv2.imread output (B, G, R).  ``half=True``: the forward runs
    under the half-precision policy.  ``colors``: an [N, 3] uint8 palette -- then returns (masks, images) with images[i]
    = colors[masks[i]] as uint8 H x W x 3 (classes >= N black).

    ``scales`` (a sequence of factors on the model input size, see ``tta_sizes``) and ``flip`` (add every scale's
    left-right mirrored view) turn on test-time ensembling: mask = argmax_c of the unweighted sum, over all views, of the
    un-mirrored softmax resized bilinearly (align_corners=False) to the photo's size; first index on ties.  ``scales`` None
    or (1.0,) without ``flip`` is the single forward above, bit for bit.

    ``min_area`` (> 1), ``largest_only`` and ``regions`` turn on the connected-region post-processing (utils/regions.py) on
    the device mask, after the decode of either route and before the single copy back: regions of fewer than ``min_area``
    pixels -- with ``largest_only`` also every region of a class >= 1 but its class's largest in the photo -- take the
    class of the region above their first pixel (``connectivity`` 4 or 8); the colours are those of the cleaned mask.
    ``regions=True`` appends one more result: per photo, a list of dicts {class, area, bbox, centroid, angle, sides, label}
    of the regions of the cleaned mask (utils.regions.region_dicts).  With all four at their defaults none of this runs.
    ``polygons=True`` (with ``regions=True``) traces every region's outline on the cleaned device mask before the copy
    back (utils.regions.mask_polygons) and adds {polygon, perimeter, min_rect} to each region's dict; without it nothing
    of that is launched or allocated.

    ``slide=True`` turns on sliding-window inference for photos larger than the model input: ``img_size`` is then the
    WINDOW (both sides multiples of 32), laid over the photo at ``stride`` = (sw, sh) in ``img_size``'s order (between
    half the window, rounded up, and the window; default ceil(2/3 of the window)) -- ``window_grid``; ``scales`` scale the
    PHOTO (``work_size``), not the input.  mask = argmax_c of the sum, over the scales, of the bilinearly resized
    (align_corners=False) working probability, which is the unweighted mean of the softmaxes (with ``flip``: softmax plus
    un-mirrored softmax of the mirrored window) of the windows covering a working-image pixel.  Windows go through the
    model at most ``window_batch`` at a time (default: the number of photos).  ``colors``, ``half`` and the region
    options compose as on the other routes.  Without ``slide`` neither ``stride`` nor ``window_batch`` may be given.

    ``crf`` (None, True for the defaults, a ``utils.crf.CRF`` or a dict of its options) refines the logits of every forward
    -- the single one, each scale's (mirrored rows with their mirrored inputs), each chunk of windows -- by the local dense
    CRF of ops.crf_refine, guided by that forward's own input, before the softmax and decode of the route; in fp32 also
    under ``half``.  With None nothing of it is imported, launched or allocated."""
    slide = bool(slide)
    if not slide and (stride is not None or window_batch is not None):
        raise ValueError('stride and window_batch belong to slide=True')
    if window_batch is not None and int(window_batch) < 1:
        raise ValueError('window_batch must be >= 1; got %r' % (window_batch,))
    min_area = int(min_area)
    if min_area < 0:
        raise ValueError('min_area must be >= 0; got %d' % min_area)
    if connectivity not in (4, 8):
        raise ValueError('connectivity must be 4 or 8; got %r' % (connectivity,))
    if polygons and not regions:
        raise ValueError('polygons=True adds to the region dicts: it needs regions=True')
    post = (min_area, int(connectivity), bool(largest_only), bool(regions), bool(polygons)) \
        if min_area > 1 or largest_only or regions else None
    if norm not in NORMS:
        raise ValueError('norm must be one of %s' % sorted(NORMS))
    mean, std = NORMS[norm]
    refine = _refiner(crf, std)
    w, h = int(img_size[0]), int(img_size[1])
    flip = bool(flip)
    if scales is not None:
        scales = tuple(float(s) for s in scales)
    tta = not slide and (flip or (scales is not None and scales != (1.0,)))
    sizes = tta_sizes(h, w, scales if scales is not None else (1.0,)) if tta else None
    if slide:
        if h < 32 or w < 32 or h % 32 or w % 32:
            raise ValueError('slide=True takes a window whose sides are multiples of 32; got img_size (%d, %d)' % (w, h))
        sy, sx = slide_strides(h, w, stride)
        scales = scales if scales is not None else (1.0,)
        slide_scales([], scales)                               # the scales alone: finite, > 0, at most 8
    photos = [_photo(im) for im in imgs]
    if not photos:
        return _result([], None if colors is None else [], None, post)
    device = next(model.parameters()).device
    if device.type != 'cuda':
        raise RuntimeError('inference() runs on the HIP path: move the model to the GPU first')
    B = len(photos)
    if slide:
        return _inference_slide(model, photos, h, w, sy, sx, scales, flip, window_batch, mean, std, bgr, half, colors, device,
                                post, refine)
    if tta:
        if B * (2 if flip else 1) > 65535:
            raise ValueError('%d photos x %d views exceed 65535 rows per launch' % (B, 2 if flip else 1))
        return _inference_ensemble(model, photos, h, w, sizes, flip, mean, std, bgr, half, colors, device, post, refine)
    lay = photo_layout(photos)
    tables = np.stack([_table(lay, 3), _table(lay, 1)])           # preprocess: byte offsets; decode: pixel offsets
    (dtables,), src = _stage(photos, lay, [tables], device)
    x = ops.image_preprocess(src, dtables[0], h, w, mean, std, bgr)
    logits = _forward(model, x, half).contiguous()
    if refine is not None:
        logits = refine(logits, x)
    return _finish(lambda lut, out: ops.seg_decode(logits, dtables[1], lay[2], lut, out=out), dtables[1], lay, colors, post,
                   device)


def photo_layout(photos):
    """[(photo, H, W)] -> (int64 sizes [B,2], pixel offset of each photo in the back-to-back packing, pixels in all)"""
    sizes = np.array([(H, W) for _, H, W in photos], dtype=np.int64).reshape(-1, 2)
    npix = sizes[:, 0] * sizes[:, 1]
    return sizes, np.concatenate([[0], np.cumsum(npix)[:-1]]).astype(np.int64), int(npix.sum())


def pack_staging(photos, heads, buf=None):
    """The byte layout of the staging buffer -- the int64 head tables back to back, in order, then the photos back to back
    (photo i at byte head + 3 * pix_off[i]) -> (head bytes, pix_off, total_pix, sizes).  buf (a uint8 numpy view of head +
    3 * total_pix bytes, or None for the layout alone) receives the tables and every photo that is a numpy array; photos
    that live on the device are left for the caller.  numpy only."""
    sizes, pix_off, total_pix = photo_layout(photos)
    head = 8 * sum(t.size for t in heads)
    if buf is not None:
        buf[:head] = np.concatenate([np.ascontiguousarray(t, dtype=np.int64).reshape(-1) for t in heads]).view(np.uint8)
        for (img, H, W), o in zip(photos, pix_off):
            if isinstance(img, np.ndarray):
                buf[head + 3 * o:head + 3 * (o + H * W)] = np.ascontiguousarray(img).reshape(-1)
    return head, pix_off, total_pix, sizes


def _table(lay, per_px):
    """int64 [B,3] of {per_px * pixel offset, H, W}: per_px = 3 the preprocess kernels' byte offsets, 1 the decode table"""
    sizes, pix_off, _ = lay
    return np.concatenate([per_px * pix_off[:, None], sizes], 1)


def _stage(photos, lay, heads, device):
    """One pinned buffer = the head tables + every host photo, one host-to-device copy; photos already on the device are
    copied in behind it -> ([each head table as an int64 device view of its own shape], the photo bytes on the device)"""
    head = pack_staging(photos, heads)[0]
    staging = torch.empty(head + 3 * lay[2], dtype=torch.uint8, pin_memory=True)
    pack_staging(photos, heads, staging.numpy())
    dbuf = staging.to(device, non_blocking=True)
    for (img, H, W), o in zip(photos, lay[1]):
        if isinstance(img, torch.Tensor):
            dbuf[head + 3 * o:head + 3 * (o + H * W)].copy_(img.to(device).reshape(-1))
    words, views, at = dbuf[:head].view(torch.int64), [], 0
    for t in heads:
        views.append(words[at:at + t.size].view(t.shape))
        at += t.size
    return views, dbuf[head:]


def _finish(decode, dtable, lay, colors, post, device):
    """What follows the forward passes on every route: decode(lut, out) writes the packed masks (and with a lut the
    colours) of the photos of the device decode table dtable; then the region pass if asked for, the single device-to-host
    copy and the results in inference()'s shape."""
    sizes, pix_off, total_pix = lay
    lut = None if colors is None else torch.from_numpy(lut_of(colors)).to(device)
    out = torch.empty(total_pix * (1 if lut is None else 4), dtype=torch.uint8, device=device)
    if post is None:
        decode(lut, out)
        records = None
    else:                                                       # decode without the palette: mask_clean writes the colours
        decode(None, out[:total_pix])
        records = _postprocess(out, dtable, total_pix, sizes, lut, post)
    host = torch.empty(out.numel(), dtype=torch.uint8, pin_memory=True)
    host.copy_(out, non_blocking=True)
    torch.cuda.current_stream(device).synchronize()
    hv = host.numpy()
    masks = [hv[o:o + H * W].reshape(H, W).astype(np.int64) for o, (H, W) in zip(pix_off, sizes)]
    images = None
    if colors is not None:
        rgb = hv[total_pix:]
        images = [rgb[3 * o:3 * (o + H * W)].reshape(H, W, 3).copy() for o, (H, W) in zip(pix_off, sizes)]
    return _result(masks, images, records, post)


def _postprocess(out, table, total_pix, sizes, lut, post):
    """the connected-region pass on the decoded device mask (imported here: the default route never loads it)"""
    from .regions import postprocess
    min_area, connectivity, largest_only, want_regions, want_polygons = post
    return postprocess(out, table, total_pix, (int(sizes[:, 0].max()), int(sizes[:, 1].max())), lut, min_area, connectivity,
                       largest_only, want_regions, want_polygons)


def _result(masks, images, records, post):
    """inference()'s four result shapes: masks, or (masks, images) with a palette, each with the per-photo region lists
    appended when regions=True asked for them (records: postprocess's result, with polygons=True the pair it returns)"""
    result = masks if images is None else (masks, images)
    if post is None or not post[3]:
        return result
    lists = []
    if masks:
        from .regions import region_dicts
        lists = region_dicts(records[0], len(masks), records[1]) if post[4] else region_dicts(records, len(masks))
    return result + (lists,) if images is not None else (result, lists)


def _refiner(crf, std):
    """inference()'s ``crf=`` -> None, or the call (logits, model input) -> refined logits (utils/crf.py is imported only here)"""
    if crf is None or crf is False:
        return None
    from .crf import CRF
    opts = CRF.of(crf)
    return lambda logits, x: opts.refine(logits, x, std)


def _inference_ensemble(model, photos, h, w, view_sizes, flip, mean, std, bgr, half, colors, device, post=None, refine=None):
    """inference() with several views: the same single staging buffer (now also carrying the view table and the map
    table) and the same single copy back; per scale one preprocess launch, one forward, one softmax launch."""
    B, S, V = len(photos), len(view_sizes), 2 if flip else 1
    lay = photo_layout(photos)
    views = np.concatenate([np.tile(_table(lay, 3), (V, 1)), np.zeros((V * B, 1), dtype=np.int64)], 1)
    views[B:, 3] = ops.VIEW_MIRROR                             # rows 0..B-1 plain, rows B..2B-1 mirrored
    maps = np.zeros((S, 3), dtype=np.int64)                    # pixel offsets: Ensemble scales them by the class padding
    maps[:, 0], maps[:, 1:] = map_offsets(B, view_sizes)[0], np.array(view_sizes, dtype=np.int64)
    (dviews, ddecode, dmaps), src = _stage(photos, lay, [views, _table(lay, 1), maps], device)

    ens = Ensemble(B, view_sizes, flip, dmaps)
    for hs, ws in view_sizes:
        x = ops.image_preprocess_views(src, dviews, hs, ws, mean, std, bgr)
        logits = _forward(model, x, half)
        if refine is not None:
            logits = refine(logits, x)
        del x
        ens.add(logits)
        del logits                                             # released before the next scale's forward
    max_hw = (int(lay[0][:, 0].max()), int(lay[0][:, 1].max()))
    return _finish(lambda lut, out: ens.decode(ddecode, lay[2], max_hw, lut, out=out), ddecode, lay, colors, post, device)


def work_size(H, W, s):
    """(Hs, Ws) of an H x W photo at scale s for sliding-window inference: the photo's own size at 1.0"""
    return max(1, int(H * s + 0.5)), max(1, int(W * s + 0.5))


def window_grid(Hs, Ws, h, w, sy, sx):
    """The windows of h x w at stride (sy, sx) over a working image of Hs x Ws -> ([(y0, x0), ...] in (i, j) order, (ny,
    nx)): n = ceil(max(size - window, 0) / stride) + 1 per axis, window i at min(i * stride, max(size - window, 0)) -- the
    last one is shifted back inside the image, and an image smaller than the window has one window along that axis."""
    my, mx = max(Hs - h, 0), max(Ws - w, 0)
    ny, nx = -(-my // sy) + 1, -(-mx // sx) + 1
    ys, xs = [min(i * sy, my) for i in range(ny)], [min(j * sx, mx) for j in range(nx)]
    return [(y0, x0) for y0 in ys for x0 in xs], (ny, nx)


def slide_strides(h, w, stride=None):
    """(sy, sx) for windows of h x w: `stride` = (sw, sh) in img_size's order, checked against ops.window_stride_limits;
    None: the default of that rule"""
    (ly, hy, dy), (lx, hx, dx) = ops.window_stride_limits(h), ops.window_stride_limits(w)
    if stride is None:
        return dy, dx
    sx, sy = int(stride[0]), int(stride[1])
    if not (ly <= sy <= hy and lx <= sx <= hx):
        raise ValueError('stride (%d, %d) outside [%d, %d] x [%d, %d]: between half the window (rounded up) and the window'
                         % (sx, sy, lx, hx, ly, hy))
    return sy, sx


def slide_scales(photo_sizes, scales):
    """-> per kept scale the list of (Hs, Ws) of every photo.  Scales must be finite and > 0 and keep every working size
    within 65535; a scale that gives EVERY photo the working size of an earlier scale is merged with a warning (as
    tta_sizes does); at most ops.ENSEMBLE_MAX_MAPS scales."""
    scales = [float(s) for s in scales]
    if not scales:
        raise ValueError('scales is empty')
    kept = []
    for s in scales:
        if not math.isfinite(s) or s <= 0:
            raise ValueError('scales must be finite and > 0; got %r' % (s,))
        sizes = [work_size(H, W, s) for H, W in photo_sizes]
        if any(Hs > 65535 or Ws > 65535 for Hs, Ws in sizes):
            raise ValueError('scale %g takes a photo beyond 65535 pixels along an axis' % s)
        if sizes and sizes in kept:
            warnings.warn('scale %g gives every photo the working size of an earlier scale; merged' % s, RuntimeWarning,
                          stacklevel=3)
        else:
            kept.append(sizes)
    if len(kept) > ops.ENSEMBLE_MAX_MAPS:
        raise ValueError('%d scales; at most %d scales are ensembled' % (len(kept), ops.ENSEMBLE_MAX_MAPS))
    return kept


def _inference_slide(model, photos, h, w, sy, sx, scales, flip, window_batch, mean, std, bgr, half, colors, device, post=None,
                     refine=None):
    """inference(slide=True): the same single staging buffer (now also carrying the window table and the group table) and
    the same single copy back; per chunk of windows one preprocess launch, one forward, one softmax launch, then ONE
    decode.  The window table is staged chunk by chunk -- with flip a chunk is [n plain; n mirrored] -- so every chunk's
    table is a slice of the staged words."""
    B, V = len(photos), 2 if flip else 1
    lay = photo_layout(photos)
    sizes, pix_off, _ = lay
    work = slide_scales([(int(H), int(W)) for H, W in sizes], scales)
    S = len(work)
    rows, groups = [], np.zeros((S, B, 3), dtype=np.int64)       # groups: window offsets, scaled to floats on the device
    for s in range(S):
        for b in range(B):
            Hs, Ws = work[s][b]
            groups[s, b] = (len(rows) * h * w, Hs, Ws)
            rows += [(3 * pix_off[b], sizes[b, 0], sizes[b, 1], 0, Hs, Ws, y0, x0)
                     for y0, x0 in window_grid(Hs, Ws, h, w, sy, sx)[0]]
    rows = np.array(rows, dtype=np.int64)
    N = len(rows)
    step = min(max(1, int(window_batch) if window_batch is not None else B), 65535 // V)
    chunks = [(a, min(a + step, N)) for a in range(0, N, step)]
    staged = []
    for a, e in chunks:
        staged.append(rows[a:e])
        if flip:
            twin = rows[a:e].copy()
            twin[:, 3] = ops.VIEW_MIRROR
            staged.append(twin)
    (dwindows, ddecode, dgroups), src = _stage(photos, lay, [np.concatenate(staged), _table(lay, 1), groups], device)

    prob = C = None
    for a, e in chunks:
        x = ops.image_preprocess_windows(src, dwindows[V * a:V * e], h, w, mean, std, bgr)
        logits = _forward(model, x, half)
        if logits.shape[2:] != (h, w):
            raise RuntimeError('the model returns %dx%d logits for a %dx%d window' % (tuple(logits.shape[2:]) + (h, w)))
        if refine is not None:
            logits = refine(logits, x)
        del x
        if prob is None:
            C = logits.shape[1]
            CP = ops.class_pad(C)
            prob = torch.empty(N * h * w * CP, dtype=torch.float32, device=device)
            dgroups[:, :, 0] *= CP                             # device arithmetic on S * B numbers: no host round trip
        ops.softmax_views(logits.contiguous(), prob, a * h * w * CP, flip)
        del logits                                             # released before the next chunk's forward
    max_hw = (int(sizes[:, 0].max()), int(sizes[:, 1].max()))
    return _finish(lambda lut, out: ops.seg_decode_windows(prob, dgroups, B, C, (h, w), (sy, sx), ddecode, lay[2], max_hw, lut,
                                                           out=out), ddecode, lay, colors, post, device)


def _forward(model, x, half):
    """eval forward; half=True binds an Env(policy='half', save=False) to the model the way Trainer.__init__ does, for
    this call only"""
    if not half:
        return model(x).float()
    from ..arena import prepare
    from ..nn import Env
    prepare(model, x.device)
    had = '_pseg_env' in model.__dict__
    prev = model.__dict__.get('_pseg_env')
    object.__setattr__(model, '_pseg_env', Env(save=False, accumulate=False, policy='half'))
    try:
        return model(x).float()
    finally:
        if had:
            object.__setattr__(model, '_pseg_env', prev)
        else:
            object.__delattr__(model, '_pseg_env')
