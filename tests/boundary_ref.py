"""numpy restatement of the contour measures' definitions (include/pseg_amd.h, "contour measures of the evaluation"), and the
cases the CPU and GPU tests share.

The depth has no class loop: `depth_windowed` is the definition itself, one shifted comparison per offset of the
(2d + 1) x (2d + 1) window; `depth_separable` is the row / column decomposition over 2d + 1 offsets (rows first -- the kernels
take columns first).  `erode_reference` is deliberately separate and slow: the iterated zero-padded 3 x 3 erosion of the
published Boundary IoU code, used only to pin the restatement to that algorithm.
"""
import numpy as np

VOID = -1          # what a prediction becomes where the target is void


def _maps(L):
    L = np.asarray(L, dtype=np.int64)
    return L.reshape((-1,) + L.shape[-2:]), L.shape


def depth_windowed(L, d):
    """depth(p): smallest k >= 1 with a pixel q of the same image at Chebyshev distance k and L(q) != L(p); d + 1 if none within d"""
    M, shape = _maps(L)
    _, H, W = M.shape
    out = np.full(M.shape, d + 1, dtype=np.int64)
    for dy in range(-min(d, H - 1), min(d, H - 1) + 1):
        for dx in range(-min(d, W - 1), min(d, W - 1) + 1):
            k = max(abs(dy), abs(dx))
            if k == 0:
                continue
            p = (slice(None), slice(max(0, -dy), H - max(0, dy)), slice(max(0, -dx), W - max(0, dx)))
            q = (slice(None), slice(max(0, dy), H - max(0, -dy)), slice(max(0, dx), W - max(0, -dx)))
            out[p] = np.minimum(out[p], np.where(M[q] != M[p], k, d + 1))
    return out.reshape(shape)


def row_distance(L, d):
    """r(q): distance along q's row to the nearest different label, clipped to d + 1"""
    M, shape = _maps(L)
    W = M.shape[2]
    out = np.full(M.shape, d + 1, dtype=np.int64)
    for k in range(1, min(d, W - 1) + 1):
        diff = M[:, :, k:] != M[:, :, :-k]
        out[:, :, :-k] = np.minimum(out[:, :, :-k], np.where(diff, k, d + 1))
        out[:, :, k:] = np.minimum(out[:, :, k:], np.where(diff, k, d + 1))
    return out.reshape(shape)


def depth_separable(L, d):
    """depth(p) = min(r(p), min over the rows at vertical offset k, 1 <= |k| <= d, of (L(q) != L(p) ? |k| : max(|k|, r(q))))"""
    M, shape = _maps(L)
    H = M.shape[1]
    r = row_distance(M, d)
    out = r.copy()
    for k in range(1, min(d, H - 1) + 1):
        diff = M[:, k:] != M[:, :-k]
        out[:, :-k] = np.minimum(out[:, :-k], np.where(diff, k, np.maximum(k, r[:, k:])))
        out[:, k:] = np.minimum(out[:, k:], np.where(diff, k, np.maximum(k, r[:, :-k])))
    return out.reshape(shape)


def edge_distance(H, W):
    """min(x + 1, W - x, y + 1, H - y): distance to the nearest pixel outside the image"""
    y, x = np.arange(H)[:, None], np.arange(W)[None, :]
    return np.minimum(np.minimum(x + 1, W - x), np.minimum(y + 1, H - y))


def label_depth(L, d, edge=False):
    """what pseg_label_depth writes: the clipped depth, with edge the outside of the image counts as a different label"""
    out = depth_separable(L, d)
    if edge:
        out = np.minimum(out, edge_distance(*out.shape[-2:]))
    return out


def erode_reference(mask, d):
    """d iterations of the 3 x 3 erosion of the zero-padded mask [H, W] (cv2.copyMakeBorder(mask, 1, 1, 1, 1, 0) once is
    what the published code does; a border of zeros that is kept zero through the iterations erodes identically)"""
    m = np.asarray(mask, dtype=bool)
    H, W = m.shape
    for _ in range(d):
        pad = np.zeros((H + 2, W + 2), dtype=bool)
        pad[1:-1, 1:-1] = m
        nxt = np.ones((H, W), dtype=bool)
        for y in range(3):
            for x in range(3):
                nxt &= pad[y:y + H, x:x + W]
        m = nxt
    return m


def boundary_counts(pred, target, C, d):
    """int64 [6][C]: inter, gband, pband, trimap tp / fn / fp"""
    T = np.asarray(target, dtype=np.int64)
    P = np.asarray(pred, dtype=np.int64)
    valid = (T >= 0) & (T < C)
    Pp = np.where(valid, P, VOID)
    dT, dP = label_depth(T, d), label_depth(Pp, d)
    e = edge_distance(*T.shape[-2:])
    gt, pr = np.minimum(dT, e) <= d, np.minimum(dP, e) <= d
    pin = (Pp >= 0) & (Pp < C)

    def count(mask, cls):
        return np.bincount(cls[mask], minlength=C).astype(np.int64)

    tri = valid & (dT <= d)
    return np.stack([count(valid & gt & pr & (Pp == T), T), count(valid & gt, T), count(pin & pr, Pp),
                     count(tri & (Pp == T), T), count(tri & (Pp != T), T), count(tri & pin & (Pp != T), Pp)])


def metrics(counters):
    """(Boundary IoU [C], trimap IoU [C]) in fp32; a denominator <= 0 is replaced by 1"""
    inter, gband, pband, tp, fn, fp = (np.asarray(c).astype(np.float32) for c in counters)

    def guarded(den):
        den = den.copy()
        den[den <= 0] = 1
        return den

    return inter / guarded(gband + pband - inter), tp / guarded(tp + fn + fp)


def width(hw, ratio=0.02):
    return max(1, int(ratio * float(hw[0] * hw[0] + hw[1] * hw[1]) ** 0.5 + 0.5))


# ------------------------------------------------------------------------------------------------ cases
# (B, H, W, C, d).  RICH cases are large enough for the generator's conditions (every depth value 1 .. d + 1 in target and
# prediction, >= 5 % of the pixels at d + 1, a void pixel, every counter row non-zero); the others are the degenerate shapes
# where some of them cannot hold -- see test_boundary_cpu.test_case_conditions for which and why.
CASES = [(3, 37, 53, 4, 5), (2, 3, 40, 3, 5), (1, 40, 3, 3, 5), (1, 1, 1, 2, 1), (2, 70, 150, 5, 7), (1, 20, 20, 2, 1),
         (1, 40, 300, 3, 254), (1, 16, 16, 1024, 3), (1, 24, 24, 1, 4),
         (2, 9, 600, 3, 3)]          # (the last one: three row segments of 256 pixels, so the row pass slides twice)
RICH = [(3, 37, 53, 4, 5), (2, 70, 150, 5, 7), (1, 20, 20, 2, 1)]


def case_id(case):
    return 'B%d-%dx%d-C%d-d%d' % case


def void_values(C):
    """-100, 255, C and another negative; 255 names a class once C > 255 and is then replaced"""
    return [-100, 255 if C <= 255 else C + 255, C, -3]


def voronoi(rng, H, W, C, seeds, first=0):
    """label map of `seeds` Voronoi cells; the cells' classes cycle through [0, C) from `first`, so neighbours differ when C > 1"""
    sy, sx = rng.integers(0, H, seeds), rng.integers(0, W, seeds)
    y, x = np.arange(H)[:, None, None], np.arange(W)[None, :, None]
    cell = np.argmin((y - sy) ** 2 + (x - sx) ** 2, axis=2)
    return ((cell + first) % C).astype(np.int64)


def make_target(case, seed=0):
    B, H, W, C, d = case
    rng = np.random.default_rng([seed, B, H, W, C, d])
    T = np.empty((B, H, W), dtype=np.int64)
    for b in range(B):
        # another first class per image: the last row of image b and the first row of image b + 1 carry different labels
        T[b] = voronoi(rng, H, W, C, 5 + b % 2, first=b)
    if C > 8:                                          # the class limit: use the top of the range as well
        T[T == 1] = C - 1
    voids = void_values(C)
    n = H * W
    if n >= 8:
        for b in range(B):
            # specks: single void pixels, and one pair of DIFFERENT void values next to each other
            p = int(rng.integers(0, n - 1))
            if (p + 1) % W == 0 and W > 1:
                p -= 1
            q = p + 1 if W > 1 else p + W
            T[b].flat[p], T[b].flat[q] = voids[0], voids[3]
            rest = np.setdiff1d(np.arange(n), [p, q])
            for i, s in enumerate(rng.choice(rest, size=4, replace=False)):
                T[b].flat[s] = voids[i]
    elif n > 1:
        T[0].flat[0] = voids[0]
    return T


def make_pred(case, target, seed=0):
    """the target shifted by one or two pixels (edge pixels repeated) with small patches flipped to another class: contours
    near but not on the target's.  The shifted void specks are its values outside [0, C)."""
    B, H, W, C, d = case
    rng = np.random.default_rng([seed + 1, B, H, W, C, d])
    P = np.empty_like(target)
    for b in range(B):
        sy, sx = (1 + b % 2, 2 - b % 2)
        ys = np.clip(np.arange(H) - sy, 0, H - 1)
        xs = np.clip(np.arange(W) - sx, 0, W - 1)
        P[b] = target[b][ys][:, xs]
        for _ in range(3):
            h, w = int(rng.integers(1, max(2, H // 6 + 1))), int(rng.integers(1, max(2, W // 6 + 1)))
            y0, x0 = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
            patch = P[b, y0:y0 + h, x0:x0 + w]
            P[b, y0:y0 + h, x0:x0 + w] = np.where((patch >= 0) & (patch < C), (patch + 1) % C, patch)
    return P


def uniform_case():
    """no different label anywhere: every depth is d + 1 without the edge term"""
    return (2, 19, 70, 3, 6), np.full((2, 19, 70), 2, dtype=np.int64)
