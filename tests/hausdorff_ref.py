"""The contract of pseg_hausdorff_stats (include/pseg_amd.h) restated twice in numpy: by all pairs of border pixels
(stats_brute) and with scipy's erosion and Euclidean distance transform (stats_scipy); the accumulation of
utils.update_surface_stats (accumulate) and the metrics of utils.compute_surface_metrics (metrics) in float64; the label maps
the tests run on (make_case, the hand-made maps of special).  tests/test_hausdorff_cpu.py holds the two restatements to each
other; tests/test_hausdorff_gpu.py holds the kernels to them."""
import numpy as np

#          B, C, H, W                                              why it is there
SHAPES = [(1, 2, 1, 70),                                         # one-row image
          (1, 3, 70, 1),                                         # one-column image
          (2, 5, 24, 40),                                        # several rows per block
          (3, 21, 17, 23),                                       # odd sizes, absent classes
          (1, 70, 8, 9),                                         # more classes than a wave
          (2, 4, 31, 64),                                        # W of exactly one wave
          (1, 3, 5, 300),                                        # a row longer than a block
          (1, 2, 260, 7)]                                        # a column longer than a block
SEED = 7


def masks(pred, target, C):
    """(P, G) as bool [B, C, H, W]: a void target pixel, or a prediction outside [0, C), is in no mask"""
    p, t = np.asarray(pred).astype(np.int64), np.asarray(target).astype(np.int64)
    valid = (t >= 0) & (t < C)
    cls = np.arange(C, dtype=np.int64)[None, :, None, None]
    return (p[:, None] == cls) & valid[:, None], (t[:, None] == cls)


def border(mask):
    """pixels of mask [H, W] with one of the four edge neighbours outside it; the outside of the image is outside"""
    m = np.pad(mask, 1)
    inner = m[:-2, 1:-1] & m[2:, 1:-1] & m[1:-1, :-2] & m[1:-1, 2:]
    return mask & ~inner


def _record(dp, dg, permille, tol):
    """dp, dg: the directed multisets D(P->G), D(G->P) as int64 arrays (either may be empty)"""
    stats, sums = np.zeros(8, dtype=np.int64), np.zeros(2, dtype=np.float64)
    stats[0], stats[1] = len(dp), len(dg)
    if len(dp) == 0 or len(dg) == 0:
        stats[2:6] = -1
        return stats, sums
    for i, d in enumerate((dp, dg)):
        d = np.sort(d)
        k = (len(d) * permille + 999) // 1000
        stats[2 + i] = d[-1]
        stats[4 + i] = d[k - 1]
        stats[6 + i] = int((d <= tol * tol).sum())
        sums[i] = float(np.sqrt(d.astype(np.float64)).sum())     # ascending: the terms are positive
    return stats, sums


def stats_brute(pred, target, C, permille=950, tol=2):
    """-> (stats int64 [B, C, 8], sums float64 [B, C, 2]) by definition: every pair of border pixels"""
    P, G = masks(pred, target, C)
    B = P.shape[0]
    stats, sums = np.zeros((B, C, 8), dtype=np.int64), np.zeros((B, C, 2), dtype=np.float64)
    for b in range(B):
        for c in range(C):
            bp = np.argwhere(border(P[b, c])).astype(np.int64)
            bg = np.argwhere(border(G[b, c])).astype(np.int64)
            if len(bp) and len(bg):
                d2 = ((bp[:, None, :] - bg[None, :, :]) ** 2).sum(2)
                dp, dg = d2.min(1), d2.min(0)
            else:
                dp, dg = np.zeros(len(bp), dtype=np.int64), np.zeros(len(bg), dtype=np.int64)
            stats[b, c], sums[b, c] = _record(dp, dg, permille, tol)
    return stats, sums


def stats_scipy(pred, target, C, permille=950, tol=2):
    """the same with scipy: M & ~binary_erosion(M, cross) and distance_transform_edt of the border's complement, squared and
    rounded to integers"""
    from scipy import ndimage
    P, G = masks(pred, target, C)
    B = P.shape[0]
    cross = ndimage.generate_binary_structure(2, 1)
    stats, sums = np.zeros((B, C, 8), dtype=np.int64), np.zeros((B, C, 2), dtype=np.float64)
    for b in range(B):
        for c in range(C):
            bp = P[b, c] & ~ndimage.binary_erosion(P[b, c], cross)
            bg = G[b, c] & ~ndimage.binary_erosion(G[b, c], cross)
            if bp.any() and bg.any():
                to_g = np.rint(ndimage.distance_transform_edt(~bg) ** 2).astype(np.int64)
                to_p = np.rint(ndimage.distance_transform_edt(~bp) ** 2).astype(np.int64)
                dp, dg = to_g[bp], to_p[bg]
            else:
                dp, dg = np.zeros(int(bp.sum()), dtype=np.int64), np.zeros(int(bg.sum()), dtype=np.int64)
            stats[b, c], sums[b, c] = _record(dp, dg, permille, tol)
    return stats, sums


def kinds(stats):
    """per record: 0 both borders empty, 1 only the prediction's empty, 2 only the target's empty, 3 both present"""
    return (stats[..., 0] > 0) * 1 + (stats[..., 1] > 0) * 2


def accumulate(acc, stats, sums):
    """utils.update_surface_stats on a float64 [7, C] array: images defined, sum of HD, of HD95, of ASSD, images with an NSD,
    sum of NSD, misses"""
    s = stats.astype(np.float64)
    n_p, n_g = s[..., 0], s[..., 1]
    defined = (n_p > 0) & (n_g > 0)
    has_nsd = (n_p + n_g) > 0
    one_p, one_g, one = np.where(defined, n_p, 1.0), np.where(defined, n_g, 1.0), np.where(has_nsd, n_p + n_g, 1.0)
    hd = np.where(defined, np.sqrt(np.maximum(np.maximum(s[..., 2], s[..., 3]), 0.0)), 0.0)
    hd95 = np.where(defined, np.sqrt(np.maximum(np.maximum(s[..., 4], s[..., 5]), 0.0)), 0.0)
    assd = np.where(defined, (sums[..., 0] / one_p + sums[..., 1] / one_g) / 2, 0.0)
    nsd = np.where(has_nsd, (s[..., 6] + s[..., 7]) / one, 0.0)
    acc[0] += defined.sum(0)
    acc[1] += hd.sum(0)
    acc[2] += hd95.sum(0)
    acc[3] += assd.sum(0)
    acc[4] += has_nsd.sum(0)
    acc[5] += nsd.sum(0)
    acc[6] += (has_nsd & ~defined).sum(0)
    return acc


def metrics(acc):
    """-> hd, hd95, assd, nsd, misses: float64 [C], NaN where no image defines the value"""
    acc = np.asarray(acc, dtype=np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        hd, hd95, assd = (np.where(acc[0] > 0, acc[i] / acc[0], np.nan) for i in (1, 2, 3))
        nsd = np.where(acc[4] > 0, acc[5] / acc[4], np.nan)
    return hd, hd95, assd, nsd, acc[6].copy()


def make_case(B, C, H, W, seed, n_bad=3, ignore_index=-100):
    """(target, pred) int64 [B, H, W].  The target: Voronoi cells of a few random sites per image, a class each, with a void
    outline between the cells and a few labels out of range.  The prediction: the target's cells shifted by a pixel or two
    (the outline closed by the nearest cell), a few rectangular blobs flipped to another class, and a few predictions out of
    range.  With C > 2 the last class occurs in no target and in a corner of image 0's prediction (a class of the prediction
    only), and with B >= 2 one class of image 1's target is predicted as another (a class of the target only)."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    cells = np.empty((B, H, W), dtype=np.int64)
    shifted = np.empty((B, H, W), dtype=np.int64)
    for b in range(B):
        k = int(min(max(2, H * W // 60), 8))
        sy, sx = rng.randint(0, H, k), rng.randint(0, W, k)
        free = C - 1 if C > 2 else C                     # with C > 2 the last class never occurs in a target
        sc = rng.randint(0, min(free, 5), k)
        if C > 1:
            sc[1] = (sc[0] + 1) % free
        dy, dx = rng.randint(-2, 3), rng.randint(-2, 3)
        cells[b] = sc[((yy[None] - sy[:, None, None]) ** 2 + (xx[None] - sx[:, None, None]) ** 2).argmin(0)]
        shifted[b] = sc[((yy[None] - sy[:, None, None] - dy) ** 2 + (xx[None] - sx[:, None, None] - dx) ** 2).argmin(0)]
    target, pred = cells.copy(), shifted.copy()
    edge = np.zeros_like(target, dtype=bool)
    edge[:, :, :-1] |= cells[:, :, :-1] != cells[:, :, 1:]
    edge[:, :-1, :] |= cells[:, :-1, :] != cells[:, 1:, :]
    target[edge] = ignore_index
    for b in range(B):
        for _ in range(2):
            h, w = rng.randint(1, max(2, H // 3 + 1)), rng.randint(1, max(2, W // 3 + 1))
            y, x = rng.randint(0, H - h + 1), rng.randint(0, W - w + 1)
            pred[b, y:y + h, x:x + w] = rng.randint(0, free)
    if C > 2:
        pred[0, :max(1, H // 4), :max(1, W // 4)] = C - 1
    if B >= 2 and C > 1:
        c1 = cells[1, 0, 0]
        pred[1][pred[1] == c1] = (c1 + 1) % C
    flat_t, flat_p = target.reshape(-1), pred.reshape(-1)
    where = rng.permutation(flat_t.size)[:min(n_bad, flat_t.size // 8)]
    flat_t[where] = np.array([C, -1, 1000, C + 7, -5])[:len(where)]
    where = rng.permutation(flat_p.size)[:min(n_bad, flat_p.size // 8)]
    flat_p[where] = np.array([-1, C, 255, -100, C + 1])[:len(where)]
    return target, pred


def special(kind):
    """(target, pred, C) of the hand-made maps"""
    if kind == 'pixels':                                 # one pixel against one pixel at offset (3, 4)
        t, p = np.zeros((1, 9, 11), dtype=np.int64), np.zeros((1, 9, 11), dtype=np.int64)
        t[0, 2, 3] = 1
        p[0, 5, 7] = 1
        return t, p, 2
    if kind == 'identical':
        t, _ = make_case(2, 4, 13, 17, seed=3)
        p = np.where((t >= 0) & (t < 4), t, 0)
        return t, p, 4
    if kind == 'full':                                   # a mask that fills the image: its border is the image frame
        t = np.full((1, 6, 9), 1, dtype=np.int64)
        p = t.copy()
        p[0, 2:4, 3:6] = 0
        return t, p, 2
    if kind == 'checkerboard':
        t = (np.add.outer(np.arange(10), np.arange(15)) & 1)[None].astype(np.int64)
        return t, 1 - t, 2
    if kind == 'one_map_only':                           # class 2 in the prediction only, class 1 in the target only
        t = np.zeros((1, 8, 8), dtype=np.int64)
        p = t.copy()
        t[0, 1:3, 1:3] = 1
        p[0, 5:7, 4:7] = 2
        return t, p, 3
    if kind == 'all_void':
        t = np.full((2, 5, 6), -100, dtype=np.int64)
        t[1] = 255
        p = np.zeros((2, 5, 6), dtype=np.int64)
        p[:, 2:, 3:] = 1
        return t, p, 3
    raise ValueError(kind)


SPECIAL = ['pixels', 'identical', 'full', 'checkerboard', 'one_map_only', 'all_void']
