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


def mask_regions(mask, table, max_hw, connectivity=8, capacity=None, labels=None):
    """-> int64 numpy array [count, ops.REGION_WORDS]: one record per component of the packed device mask, in (photo, label)
    order.  The records are counted and summed on the device with a first capacity (default: 1024 per photo); this
    function reads the count on the host -- it returns host data anyway -- and repeats ONLY the records call with the
    full count if the first capacity was too small.  labels: label_masks' result for this mask and connectivity, if the
    caller has it."""
    if labels is None:
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


def region_dicts(records, B, polygons=None):
    """records (mask_regions) -> per photo, a list of {class, area, bbox [x0, y0, x1, y1] (inclusive), centroid, angle,
    sides, label}: plain Python numbers, ready for json.  polygons (mask_polygons of the same mask and connectivity): every
    region also gets ``polygon``, a list of flat [x0, y0, x1, y1, ...] lists in lattice coordinates (pixel (x, y) is the
    square [x, x+1] x [y, y+1]), the outer ring first, then the holes; ``perimeter``, the length of all its rings; and
    ``min_rect``, min_area_rect of the outer ring's vertices with center, size and angle as lists."""
    out = [[] for _ in range(B)]
    rings_of = None
    if polygons is not None:
        rings_of = [{p['label']: p['rings'] for p in photo} for photo in polygons]
    for r in np.asarray(records).reshape(-1, ops.REGION_WORDS).tolist():
        g = region_geometry(r)
        d = {'class': r[0] & 255, 'area': r[2], 'bbox': r[3:7], 'centroid': list(g['centroid']),
             'angle': g['angle'], 'sides': list(g['sides']), 'label': r[1]}
        if rings_of is not None:
            rings = rings_of[r[0] >> 8][r[1]]
            rect = min_area_rect(rings[0])
            d['polygon'] = [np.asarray(ring).reshape(-1).tolist() for ring in rings]
            d['perimeter'] = sum(ring_perimeter(ring) for ring in rings)
            d['min_rect'] = {'center': list(rect['center']), 'size': list(rect['size']), 'angle': rect['angle']}
        out[r[0] >> 8].append(d)
    return out


def mask_polygons(mask, table, max_hw, connectivity=8, capacity=None, labels=None):
    """-> per photo, a list of {label, class, rings} in label order: the outlines of the components of the packed device
    mask (ops.mask_rings; definitions in include/pseg_amd.h).  ``rings`` is a list of int32 numpy arrays [n, 2] of lattice
    vertices (x, y), the outer ring first, then the holes in the order of their start edges.  The rings are traced on the
    device with a first capacity of edges (default: 4096 per photo plus one per 4 pixels); this function reads the counts
    on the host -- it returns host data anyway -- and repeats ONLY the rings call, once, with the full edge count if the
    first capacity was too small.  labels: label_masks' result for this mask and connectivity, if the caller has it."""
    if labels is None:
        labels = label_masks(mask, table, max_hw, connectivity)
    elif connectivity not in (4, 8):
        raise ValueError('connectivity must be 4 or 8; got %r' % (connectivity,))
    npix, B = mask.numel(), table.shape[0]
    cap = min(4 * npix, 4096 * B + npix // 4) if capacity is None else int(capacity)
    rings, vertices, counts = ops.mask_rings(mask, labels, table, npix, max_hw, connectivity, cap)
    n = counts.tolist()
    if n[0] > cap:
        rings, vertices, counts = ops.mask_rings(mask, labels, table, npix, max_hw, connectivity, n[0])
        n = counts.tolist()
    rings, vertices = rings[:n[1]].cpu().numpy(), vertices[:n[2]].cpu().numpy()
    out = [{} for _ in range(B)]
    for head, label, _, first, count, _ in rings.tolist():
        entry = out[head >> 8].setdefault(label, {'label': label, 'class': head & 255, 'rings': []})
        entry['rings'].append(vertices[first:first + count])           # the outer ring has the smallest start edge: first
    return [[photo[label] for label in sorted(photo)] for photo in out]


def ring_area2(ring):
    """Twice the signed area of a closed ring [n, 2] of integer vertices, as an exact Python int: the shoelace sum
    sum(x_i * y_{i+1} - x_{i+1} * y_i).  With y down it is positive for outer rings, negative for holes."""
    pts = [(int(x), int(y)) for x, y in np.asarray(ring).reshape(-1, 2).tolist()]
    return sum(x0 * y1 - x1 * y0 for (x0, y0), (x1, y1) in zip(pts, pts[1:] + pts[:1]))


def ring_perimeter(ring):
    """Length of a closed ring [n, 2]: an exact Python int for the rectilinear rings of mask_polygons (every segment is
    horizontal or vertical), the sum of Euclidean lengths as a float otherwise."""
    pts = [(int(x), int(y)) for x, y in np.asarray(ring).reshape(-1, 2).tolist()]
    segs = [(x1 - x0, y1 - y0) for (x0, y0), (x1, y1) in zip(pts, pts[1:] + pts[:1])]
    if all(dx == 0 or dy == 0 for dx, dy in segs):
        return sum(abs(dx) + abs(dy) for dx, dy in segs)
    return sum(math.hypot(dx, dy) for dx, dy in segs)


def convex_hull(points):
    """Integer points [n, 2] -> the vertices of their convex hull as a list of (x, y) Python ints (Andrew's monotone chain
    with exact integer cross products): it begins at the lexicographically smallest (x, y), turns with positive cross
    products (clockwise on the screen, y down) and holds no three collinear points."""
    pts = sorted(set((int(x), int(y)) for x, y in np.asarray(points).reshape(-1, 2).tolist()))
    if len(pts) < 3:
        return pts

    def half(seq):
        h = []
        for p in seq:
            while len(h) >= 2 and (h[-1][0] - h[-2][0]) * (p[1] - h[-2][1]) - (h[-1][1] - h[-2][1]) * (p[0] - h[-2][0]) <= 0:
                h.pop()
            h.append(p)
        return h

    lower, upper = half(pts), half(pts[::-1])
    return lower[:-1] + upper[:-1]


def min_area_rect(points):
    """The minimum-area enclosing rectangle of integer points [n, 2] (what cv2.minAreaRect gives the reference's RectLoss)
    -> {center: (cx, cy), size: (along, across), angle}.  A smallest rectangle has a side on an edge of the convex hull, so
    one rectangle is formed per hull edge (convex_hull's order, the first edge leaving its first vertex), in float64, and
    the smallest area is kept; ties go to the first hull edge.  ``angle`` is the direction of that hull edge -- the side
    whose length is size[0] -- in radians, x to the right and y down, folded into (-pi/2, pi/2]; ``center`` is in the
    points' own coordinates.  Fewer than three hull vertices (one point, or all on a line) give the segment itself: size
    (length, 0.0).  This is host code on purpose: it runs over the few dozen hull vertices of a region."""
    hull = convex_hull(points)
    if not hull:
        raise ValueError('min_area_rect of no points')
    if len(hull) == 1:
        return {'center': (float(hull[0][0]), float(hull[0][1])), 'size': (0.0, 0.0), 'angle': 0.0}
    h = np.asarray(hull, dtype=np.float64)
    best = None
    for i in range(len(hull) if len(hull) > 2 else 1):
        d = h[(i + 1) % len(hull)] - h[i]
        u = d / math.hypot(d[0], d[1])
        v = np.array([-u[1], u[0]])
        a, c = h @ u, h @ v
        size = (float(a.max() - a.min()), float(c.max() - c.min()))
        if best is None or size[0] * size[1] < best[0]:
            mid = 0.5 * (a.max() + a.min()) * u + 0.5 * (c.max() + c.min()) * v
            best = (size[0] * size[1], (float(mid[0]), float(mid[1])), size, math.atan2(u[1], u[0]))
    angle = best[3]
    if angle <= -0.5 * math.pi:
        angle += math.pi
    elif angle > 0.5 * math.pi:
        angle -= math.pi
    return {'center': best[1], 'size': best[2], 'angle': angle}


def coco_annotations(found, sizes, num_classes, names=None):
    """{file name: region dicts with polygons (region_dicts)} and {file name: (H, W)} -> a COCO dict in the layout
    utils.datasets.CocoDataset reads: images {id, file_name, height, width}, categories {id = class - 1, name}, and one
    annotation per region of a class >= 1 (background regions are not written) with image_id, category_id = class - 1,
    segmentation = [outer ring] (COCO polygons cannot express holes: they are dropped here), area (pixels), bbox [x, y, w,
    h] in lattice coordinates and iscrowd 0."""
    names = list(names) if names is not None else ['class%d' % c for c in range(1, num_classes)]
    coco = {'images': [], 'categories': [{'id': i, 'name': n} for i, n in enumerate(names)], 'annotations': []}
    for image_id, name in enumerate(sorted(found)):
        H, W = sizes[name]
        coco['images'].append({'id': image_id, 'file_name': name, 'height': int(H), 'width': int(W)})
        for d in found[name]:
            if d['class'] < 1:
                continue
            x0, y0, x1, y1 = d['bbox']
            coco['annotations'].append({'id': len(coco['annotations']), 'image_id': image_id, 'category_id': d['class'] - 1,
                                        'segmentation': [list(d['polygon'][0])], 'area': d['area'],
                                        'bbox': [x0, y0, x1 - x0 + 1, y1 - y0 + 1], 'iscrowd': 0})
    return coco


def postprocess(out, table, total_pix, max_hw, lut, min_area, connectivity, largest_only, want_regions, want_polygons=False):
    """inference()'s post-processing on the decode's own output buffer ``out`` (mask, then room for the colours when lut
    is given): cleaned in place, coloured from the cleaned mask.  -> records (numpy) of the cleaned mask, or None; with
    ``want_polygons`` -> (records, polygons): mask_polygons of the cleaned mask beside them, from one labelling."""
    mask = out[:total_pix]
    clean_masks(mask, table, max_hw, min_area, connectivity, largest_only, lut, out)
    if not want_polygons:
        return mask_regions(mask, table, max_hw, connectivity) if want_regions else None
    labels = label_masks(mask, table, max_hw, connectivity)
    records = mask_regions(mask, table, max_hw, connectivity, labels=labels) if want_regions else None
    return records, mask_polygons(mask, table, max_hw, connectivity, labels=labels)


def clean_predictions(pred, min_area=0, connectivity=8, largest_only=False):
    """int64 device masks [B,H,W] of at most 256 classes (what predict_mask returns) -> the same, cleaned: evaluation's
    route into clean_masks"""
    B, H, W = pred.shape
    table_np, total, max_hw = packed_table([(H, W)] * B)
    mask = pred.to(torch.uint8).reshape(-1)
    table = torch.from_numpy(table_np).to(pred.device)
    cleaned, _ = clean_masks(mask, table, max_hw, min_area, connectivity, largest_only, None, mask)
    return cleaned.view(B, H, W).to(torch.int64)
