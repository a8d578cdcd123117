"""Plain Python reference of the outline definitions (include/pseg_amd.h, "outlines of the regions"), written from the
definitions and independent of the device code.  It only ever sees small photos.

  trace(lab, connectivity)            -> the rings of one labelled photo, ascending by start edge: dicts {label, start,
                                         hole, vertices [(x, y), ...], edges (the ring's length)}
  device_arrays(masks, labs, conn)    -> (ring records, vertices, counts) as pseg_mask_rings writes them for the packed batch
  rasterise(rings, H, W)              -> bool [H,W]: even-odd fill of rectilinear rings
  holes(component, connectivity)      -> number of holes of a bool component: the pieces of its complement (dual
                                         connectivity) that do not reach the outside
Labels come from regions_ref.label: a flood fill in raster order, canonical by construction.
"""
import numpy as np
from scipy import ndimage

# side s of a pixel: direction of travel, and the tail vertex relative to the pixel's corner (x, y)
DIR = ((1, 0), (0, 1), (-1, 0), (0, -1))
TAIL = ((0, 0), (1, 0), (1, 1), (0, 1))
ACROSS = ((0, -1), (1, 0), (0, 1), (-1, 0))


def _same(lab, x, y, l):
    H, W = lab.shape
    return 0 <= x < W and 0 <= y < H and lab[y, x] == l


def edges(lab):
    """the set of edge ids 4 * (y*W + x) + s that exist"""
    H, W = lab.shape
    return {4 * (y * W + x) + s for y in range(H) for x in range(W) for s in range(4)
            if not _same(lab, x + ACROSS[s][0], y + ACROSS[s][1], lab[y, x])}


def successor(lab, e, connectivity):
    H, W = lab.shape
    p, s = e >> 2, e & 3
    y, x = divmod(p, W)
    l = lab[y, x]
    ax, ay = x + DIR[s][0], y + DIR[s][1]
    left = DIR[(s + 3) % 4]
    bx, by = ax + left[0], ay + left[1]
    in_a, in_b = _same(lab, ax, ay, l), _same(lab, bx, by, l)
    if in_a and in_b:
        return 4 * (by * W + bx) + (s + 3) % 4
    if in_a:
        return 4 * (ay * W + ax) + s
    if in_b and connectivity == 8:
        return 4 * (by * W + bx) + (s + 3) % 4
    return 4 * p + (s + 1) % 4


def trace(lab, connectivity):
    lab = np.asarray(lab)
    H, W = lab.shape
    todo = edges(lab)
    rings = []
    for first in sorted(todo):
        if first not in todo:
            continue
        ring, e = [], first
        while True:                                   # one sequential walk per ring
            assert e in todo, 'the successor of an edge is an edge nobody else leads to'
            todo.discard(e)
            ring.append(e)
            e = successor(lab, e, connectivity)
            if e == first:
                break
        corners = [k for k in range(len(ring)) if ring[k - 1] & 3 != ring[k] & 3]
        k0 = min(corners, key=lambda k: ring[k])
        order = [k for k in corners if k >= k0] + [k for k in corners if k < k0]
        verts = []
        for k in order:
            y, x = divmod(ring[k] >> 2, W)
            verts.append((x + TAIL[ring[k] & 3][0], y + TAIL[ring[k] & 3][1]))
        start = ring[k0]
        label = int(lab[divmod(start >> 2, W)])
        rings.append({'label': label, 'start': start, 'hole': int(start != 4 * label), 'vertices': verts,
                      'edges': len(ring)})
    return sorted(rings, key=lambda r: r['start'])


def device_arrays(masks, labs, connectivity):
    """what pseg_mask_rings writes for the photos packed back to back: (records [[photo*256+class, label, start, first
    vertex, vertex count, hole], ...], vertices [[x, y], ...], [edges, rings, vertices])"""
    records, vertices, nedges = [], [], 0
    for b, (m, lab) in enumerate(zip(masks, labs)):
        W = m.shape[1]
        for r in trace(lab, connectivity):
            y, x = divmod(r['start'] >> 2, W)
            records.append([b * 256 + int(m[y, x]), r['label'], r['start'], len(vertices), len(r['vertices']), r['hole']])
            vertices += [list(v) for v in r['vertices']]
            nedges += r['edges']
    return records, vertices, [nedges, len(records), len(vertices)]


def rasterise(rings, H, W):
    """even-odd fill: pixel (x, y) is inside iff an odd number of vertical segments of the rings lie left of its centre
    (x + 0.5, y + 0.5) and span its row"""
    cross = np.zeros((H, W + 1), dtype=np.int64)
    for verts in rings:
        verts = [tuple(int(c) for c in v) for v in np.asarray(verts).reshape(-1, 2).tolist()]
        for (x0, y0), (x1, y1) in zip(verts, verts[1:] + verts[:1]):
            assert (x0 == x1) != (y0 == y1), 'rectilinear rings only'
            if x0 == x1:
                cross[min(y0, y1):max(y0, y1), x0] += 1
    return np.cumsum(cross[:, :W], axis=1) % 2 == 1


def area2(verts):
    verts = [tuple(int(c) for c in v) for v in np.asarray(verts).reshape(-1, 2).tolist()]
    return sum(x0 * y1 - x1 * y0 for (x0, y0), (x1, y1) in zip(verts, verts[1:] + verts[:1]))


def holes(component, connectivity):
    """pieces of the complement, under the dual connectivity (4 for 8, 8 for 4), of the component padded by one pixel,
    minus the one that holds the padding"""
    comp = np.pad(np.asarray(component, dtype=bool), 1)
    structure = ndimage.generate_binary_structure(2, 1 if connectivity == 8 else 2)
    return ndimage.label(~comp, structure=structure)[1] - 1
