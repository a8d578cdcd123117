"""Connected regions of segmentation masks: labelling, cleanup and region records (csrc/regions.hip).

The step after the argmax that users of a segmentation tool expect: drop regions under N pixels (specks take their
surroundings' class, pinholes are filled), keep the largest region of each class, and get the objects out as area,
bounding box, centre and orientation.  Everything up to the records runs on the device, on the layout inference already
uses: a ragged batch of uint8 masks packed in one flat buffer under an int64 table [B,3] of {pixel offset, H, W}.

``label_masks``, ``clean_masks`` and ``mask_regions`` work on such a packed device mask; ``region_geometry`` turns one
record's integer sums into centroid, principal-axis angle and the moment-equivalent rectangle, in float64 on the host.
The exact definitions (component, canonical label, replacement walk, record words) are in include/pseg_amd.h.
"""
import math

import numpy as np
import torch

from .. import ops


def packed_table(sizes):
    """[(H, W), ...] -> (int64 numpy table [B,3] of {pixel offset, H, W}, pixels in all, (largest H, largest W))"""
    sizes = np.asarray(sizes, dtype=np.int64).reshape(-1, 2)
    npix = sizes[:, 0] * sizes[:, 1]
    table = np.zeros((len(sizes), 3), dtype=np.int64)
    table[:, 0] = np.concatenate([[0], np.cumsum(npix)[:-1]])
    table[:, 1:] = sizes
    return table, int(npix.sum()), (int(sizes[:, 0].max()), int(sizes[:, 1].max()))


def label_masks(mask, table, max_hw, connectivity=8):
    """Packed uint8 device mask + device table -> int32 labels at the same offsets: y*W + x of the first pixel, in raster
    order, of each pixel's component within its own photo.  A component is a maximal 4- or 8-connected set of pixels of
    one class value; every value is a class, background included."""
    if connectivity not in (4, 8):
        raise ValueError('connectivity must be 4 or 8; got %r' % (connectivity,))
    return ops.mask_label(mask, table, mask.numel(), max_hw, connectivity)


def clean_masks(mask, table, max_hw, min_area=0, connectivity=8, largest_only=False, lut=None, out=None):
    """Label, then drop the small components: those below ``min_area`` pixels and, with ``largest_only``, every component
    of a class >= 1 that is not the largest of its class in its photo (equal areas: the first in raster order stays).  A
    small component takes the class of the region above its first pixel (left of it in the top row), followed through
    further small regions: a hole takes the object's class, a speck its surroundings', a cluster of specks the first
    large region behind it; a region at the photo's corner keeps its class.  ``out`` may be the buffer ``mask`` heads (in
    place).  -> (cleaned mask, colours or None), as ops.seg_decode returns them."""
    labels = label_masks(mask, table, max_hw, connectivity)
    return ops.mask_clean(mask, labels, table, mask.numel(), max_hw, min_area, largest_only, lut, out)


def mask_regions(mask, table, max_hw, connectivity=8, capacity=None):
    """-> int64 numpy array [count, ops.REGION_WORDS]: one record per component of the packed device mask, in (photo, label)
    order.  The records are counted and summed on the device with a first capacity (default: 1024 per photo); this
    function reads the count on the host -- it returns host data anyway -- and repeats ONLY the records call with the
    full count if the first capacity was too small."""
    labels = label_masks(mask, table, max_hw, connectivity)
    npix = mask.numel()
    cap = min(npix, 1024 * table.shape[0]) if capacity is None else int(capacity)
    records, count = ops.mask_regions(mask, labels, table, npix, max_hw, cap)
    n = int(count.item())
    if n > cap:
        records, count = ops.mask_regions(mask, labels, table, npix, max_hw, n)
    return records[:n].cpu().numpy()


def region_geometry(record):
    """One record (the ops.REGION_WORDS integers of mask_regions) -> dict with
      centroid: (cx, cy) = (Sx, Sy) / area, in pixel coordinates of the photo (pixel centres at integers);
      angle:    0.5 * atan2(2 mu11, mu20 - mu02), the direction of the principal axis of the central second moments
                (radians, x to the right, y down, in (-pi/2, pi/2]);
      sides:    (sqrt(12 l1 + 1), sqrt(12 l2 + 1)) for the eigenvalues l1 >= l2 of the pixel covariance [[mu20, mu11],
                [mu11, mu02]]: the side along ``angle`` first.
    This is the MOMENT-EQUIVALENT rectangle: the rectangle of unit pixels with the region's covariance.  It is exact for an
    axis-aligned a x b pixel rectangle, whose variances are (a^2 - 1) / 12 and (b^2 - 1) / 12 (a wide one gives angle 0 and
    sides (a, b); a tall one is the same box told as angle pi/2 and sides (b, a)).  It is NOT cv2.minAreaRect of the
    contour, which the reference's RectLoss uses: for a non-convex or ragged region the two differ.
    The central moments are formed from the integer sums in exact integer arithmetic (area * Sxx - Sx^2, ...) before the
    one division, so no cancellation of large coordinates enters."""
    r = [int(v) for v in record]
    n, sx, sy, sxx, sxy, syy = r[2], r[7], r[8], r[9], r[10], r[11]
    if n < 1:
        raise ValueError('record of an empty region')
    n2 = n * n
    mu20, mu02, mu11 = (n * sxx - sx * sx) / n2, (n * syy - sy * sy) / n2, (n * sxy - sx * sy) / n2
    half_sum, half_dif = 0.5 * (mu20 + mu02), 0.5 * (mu20 - mu02)
    root = math.hypot(half_dif, mu11)
    l1, l2 = half_sum + root, max(half_sum - root, 0.0)
    return {'centroid': (sx / n, sy / n), 'angle': 0.5 * math.atan2(2.0 * mu11, mu20 - mu02),
            'sides': (math.sqrt(12.0 * l1 + 1.0), math.sqrt(12.0 * l2 + 1.0))}


def region_dicts(records, B):
    """records (mask_regions) -> per photo, a list of {class, area, bbox [x0, y0, x1, y1] (inclusive), centroid, angle,
    sides, label}: plain Python numbers, ready for json"""
    out = [[] for _ in range(B)]
    for r in np.asarray(records).reshape(-1, ops.REGION_WORDS).tolist():
        g = region_geometry(r)
        out[r[0] >> 8].append({'class': r[0] & 255, 'area': r[2], 'bbox': r[3:7], 'centroid': list(g['centroid']),
                               'angle': g['angle'], 'sides': list(g['sides']), 'label': r[1]})
    return out


def postprocess(out, table, total_pix, max_hw, lut, min_area, connectivity, largest_only, want_regions):
    """inference()'s post-processing on the decode's own output buffer ``out`` (mask, then room for the colours when lut
    is given): cleaned in place, coloured from the cleaned mask.  -> records (numpy) of the cleaned mask, or None."""
    mask = out[:total_pix]
    clean_masks(mask, table, max_hw, min_area, connectivity, largest_only, lut, out)
    return mask_regions(mask, table, max_hw, connectivity) if want_regions else None


def clean_predictions(pred, min_area=0, connectivity=8, largest_only=False):
    """int64 device masks [B,H,W] of at most 256 classes (what predict_mask returns) -> the same, cleaned: evaluation's
    route into clean_masks"""
    B, H, W = pred.shape
    table_np, total, max_hw = packed_table([(H, W)] * B)
    mask = pred.to(torch.uint8).reshape(-1)
    table = torch.from_numpy(table_np).to(pred.device)
    cleaned, _ = clean_masks(mask, table, max_hw, min_area, connectivity, largest_only, None, mask)
    return cleaned.view(B, H, W).to(torch.int64)
