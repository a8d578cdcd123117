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
"""
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


@torch.no_grad()
def inference(model, imgs, img_size=(64, 64), norm='dataset', bgr=True, half=False, colors=None):
    """The reference's contract: ``imgs`` is a list of uint8 H x W x 3 photos (numpy arrays, or CPU or device tensors),
    ``img_size`` = (w, h) of the model input as cv2.resize takes it; returns one int64 numpy H x W mask per photo, at
    that photo's own size.  ``bgr=True``: the photos are cv2.imread output (B, G, R).  ``half=True``: the forward runs
    under the half-precision policy.  ``colors``: an [N, 3] uint8 palette -- then returns (masks, images) with images[i]
    = colors[masks[i]] as uint8 H x W x 3 (classes >= N black)."""
    if norm not in NORMS:
        raise ValueError('norm must be one of %s' % sorted(NORMS))
    mean, std = NORMS[norm]
    w, h = int(img_size[0]), int(img_size[1])
    photos = [_photo(im) for im in imgs]
    if not photos:
        return ([], []) if colors is not None else []
    device = next(model.parameters()).device
    if device.type != 'cuda':
        raise RuntimeError('inference() runs on the HIP path: move the model to the GPU first')
    B = len(photos)
    sizes = np.array([(H, W) for _, H, W in photos], dtype=np.int64)
    npix = sizes[:, 0] * sizes[:, 1]
    pix_off = np.concatenate([[0], np.cumsum(npix)[:-1]])
    total_pix = int(npix.sum())
    tables = np.zeros((2, B, 3), dtype=np.int64)
    tables[0, :, 0], tables[1, :, 0] = 3 * pix_off, pix_off      # preprocess: byte offsets; decode: pixel offsets
    tables[:, :, 1], tables[:, :, 2] = sizes[:, 0], sizes[:, 1]
    head = tables.nbytes

    # one pinned buffer = both tables + every host photo; one host-to-device copy
    staging = torch.empty(head + 3 * total_pix, dtype=torch.uint8, pin_memory=True)
    sv = staging.numpy()
    sv[:head] = tables.reshape(-1).view(np.uint8)
    for (img, _, _), o in zip(photos, pix_off):
        if isinstance(img, np.ndarray):
            sv[head + 3 * o:head + 3 * (o + img.shape[0] * img.shape[1])] = np.ascontiguousarray(img).reshape(-1)
    dbuf = staging.to(device, non_blocking=True)
    for (img, _, _), o in zip(photos, pix_off):
        if isinstance(img, torch.Tensor):
            dbuf[head + 3 * o:head + 3 * (o + img.shape[0] * img.shape[1])].copy_(img.to(device).reshape(-1))
    dtables = dbuf[:head].view(torch.int64).view(2, B, 3)

    x = ops.image_preprocess(dbuf[head:], dtables[0], h, w, mean, std, bgr)
    logits = _forward(model, x, half)
    lut = None if colors is None else torch.from_numpy(lut_of(colors)).to(device)
    out = torch.empty(total_pix * (1 if lut is None else 4), dtype=torch.uint8, device=device)
    ops.seg_decode(logits.contiguous(), dtables[1], total_pix, lut, out=out)

    # one device-to-host copy of masks (and colours)
    host = torch.empty(out.numel(), dtype=torch.uint8, pin_memory=True)
    host.copy_(out, non_blocking=True)
    torch.cuda.current_stream(device).synchronize()
    hv = host.numpy()
    masks = [hv[o:o + H * W].reshape(H, W).astype(np.int64) for o, (H, W) in zip(pix_off, sizes)]
    if colors is None:
        return masks
    rgb = hv[total_pix:]
    return masks, [rgb[3 * o:3 * (o + H * W)].reshape(H, W, 3).copy() for o, (H, W) in zip(pix_off, sizes)]


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
