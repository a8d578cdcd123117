"""Plain Python / numpy reference of the connected-region definitions (include/pseg_amd.h, "connected regions of the
masks"), written from the definitions and independent of the device code.  It only ever sees small photos.

  label(mask, connectivity)   -> int array [H,W]: y*W + x of the first pixel, in raster order, of each pixel's component
  records(mask, lab, photo)   -> list of 12-integer records in label order
  clean(mask, lab, min_area, largest_only) -> the cleaned mask
"""
import numpy as np

NEIGHBOURS = {4: ((-1, 0), (1, 0), (0, -1), (0, 1)),
              8: ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))}


def label(mask, connectivity):
    """Flood fill in raster order: the seed of a fill is the first pixel of its component, so its index is the label."""
    mask = np.asarray(mask)
    H, W = mask.shape
    lab = np.full((H, W), -1, dtype=np.int64)
    for y in range(H):
        for x in range(W):
            if lab[y, x] >= 0:
                continue
            seed, c = y * W + x, mask[y, x]
            lab[y, x] = seed
            stack = [(y, x)]
            while stack:
                cy, cx = stack.pop()
                for dy, dx in NEIGHBOURS[connectivity]:
                    ny, nx = cy + dy, cx + dx
                    if 0 <= ny < H and 0 <= nx < W and lab[ny, nx] < 0 and mask[ny, nx] == c:
                        lab[ny, nx] = seed
                        stack.append((ny, nx))
    return lab


def records(mask, lab, photo=0):
    """[photo * 256 + class, label, area, x0, y0, x1, y1, Sx, Sy, Sxx, Sxy, Syy] per component, ascending label; x, y from
    the photo's corner, Python integers"""
    mask = np.asarray(mask)
    H, W = mask.shape
    out = []
    for root in sorted(set(lab.reshape(-1).tolist())):
        ys, xs = np.nonzero(lab == root)
        ys, xs = [int(v) for v in ys], [int(v) for v in xs]
        out.append([photo * 256 + int(mask[root // W, root % W]), root, len(xs), min(xs), min(ys), max(xs), max(ys),
                    sum(xs), sum(ys), sum(x * x for x in xs), sum(x * y for x, y in zip(xs, ys)), sum(y * y for y in ys)])
    return out


def clean(mask, lab, min_area=0, largest_only=False):
    mask = np.asarray(mask)
    H, W = mask.shape
    roots = sorted(set(lab.reshape(-1).tolist()))
    area = {r: int((lab == r).sum()) for r in roots}
    cls = {r: int(mask[r // W, r % W]) for r in roots}
    small = {r: area[r] < min_area for r in roots}
    if largest_only:
        for c in set(cls.values()):
            if c >= 1:
                mine = [r for r in roots if cls[r] == c]
                keep = min(mine, key=lambda r: (-area[r], r))      # largest area, then the smaller label
                for r in mine:
                    if r != keep:
                        small[r] = True
    new = {}
    for r in roots:
        cur = r
        while small[cur] and cur != 0:                             # the corner component keeps its class
            y, x = cur // W, cur % W
            cur = int(lab[y - 1, x]) if y > 0 else int(lab[y, x - 1])
        new[r] = cls[cur]
    out = np.empty_like(mask)
    for r in roots:
        out[lab == r] = new[r]
    return out
