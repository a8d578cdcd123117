"""On-device training augmentation: the geometric (affine and local), colour-affine, small-filter, noise and dropout part of
the reference's online augmentation (``TRAIN_AUGS``, reference utils/datasets.py:26-125, imgaug on the host, one sample at a time) as ONE
kernel over the collated uint8 batch (csrc/augment.hip), fused with ``CocoDataset.post_fetch_fn``'s normalisation,
multi-scale resize and label widening.

The host only draws numbers.  ``DeviceAugment.draw(B)`` draws one *recipe* per sample from a seedable
``numpy.random.Generator``; ``DeviceAugment.rows(recipes, H, W)`` folds each recipe into one row of the kernel's parameter
table (layout: include/pseg_amd.h, ``PSEG_AUGMENT_ROW`` floats): the INVERSE affine of the whole geometric chain, a 3x4
colour matrix in 0..255 units, the fill value, the interpolation order and the border mode.  A batch in which some sample
drew a filter, noise or dropout gets the wider rows of ``pseg_augment_batch_nbhd`` (``PSEG_AUGMENT_NBHD_ROW`` floats: the
same 24, then K, the noise and dropout parameters, the sample's 64-bit seed bit-cast into two floats, and the K x K
weights) and goes through that kernel; a batch in which some sample drew an elastic, piecewise-affine or perspective warp
gets the still wider rows of ``pseg_augment_batch_warp`` (``PSEG_AUGMENT_WARP_ROW`` floats: the same 212, then the third row
of an inverse homography, the elastic alpha and a 4 x 4 displacement grid); a batch in which some sample drew a median blur,
an edge-detect blend, a hue / saturation shift or a frequency-noise colour blend gets the widest rows, those of
``pseg_augment_batch_blend`` (``PSEG_AUGMENT_BLEND_ROW`` floats: the same 252, then the median window, a second filter, a
second colour matrix, the hue and saturation shifts and two 16 x 16 mask tables); every other batch goes through
``pseg_augment_batch`` as before.

Built (defaults of ``DeviceAugment.reference()`` = the reference's values):
  * ``Fliplr(0.5)``, ``Flipud(0.2)``;
  * ``Sometimes(0.5, CropAndPad(percent=(-0.05, 0.1)))``: each side drawn on its own, negative crops, positive pads, the
    result is resized back to H x W (imgaug's ``keep_size``);
  * ``Sometimes(0.5, Affine(...))`` about the image centre: scale 0.8..1.2 per axis, translate +-20 % per axis, rotate
    +-90 degrees, shear +-16 degrees, order drawn from {0, 1}, cval 0..255, mode drawn from {constant, edge};
  * of the ``SomeOf((0, 5), [...16 augmenters...], random_order=True)`` block the five that are affine in colour: ``Invert(0.05,
    per_channel=True)``, ``Add((-10, 10), per_channel=0.5)``, ``Multiply((0.5, 1.5), per_channel=0.5)`` (one of the two
    branches of its ``OneOf``), ``LinearContrast((0.5, 2.0), per_channel=0.5)`` and ``Grayscale(alpha=(0, 1))``.  As in the
    reference, 0..5 of the block's 16 slots are picked per sample; a picked slot that holds one of these five is applied,
    in a random order; the other slots do nothing here.
  * only with ``DeviceAugment.full()`` (all off by default, so ``DeviceAugment()`` / ``.reference()`` draw the tables they
    always drew): five more slots of that block, the neighbourhood and per-pixel-random augmenters -- see "Filters, noise
    and dropout" below.  With them 10 of the 16 slots are live.
  * only with ``DeviceAugment.warps()`` (= ``full()`` plus these, all off by default): the three slots that move pixels by
    something other than one matrix, ``ElasticTransformation``, ``PiecewiseAffine`` and ``PerspectiveTransform`` -- see
    "Local warps" below.  With them 13 of the 16 slots are live.
  * only with ``DeviceAugment.blends()`` (= ``warps()`` plus these, all off by default): ``AddToHueAndSaturation``, the
    edge-detect blend, the median blur and the frequency-noise blend -- see "Median, blends, hue and saturation" below.
    With them 15 of the 16 slots are live and every ``OneOf`` is complete.
Labels are warped with the same coordinate map, nearest sample, background 0, as imgaug warps segmentation maps.

Filters, noise and dropout (``full()``).  These formulas are THIS MODULE'S CONTRACT.  They were written down from imgaug's
documentation as remembered; imgaug and cv2 are not installed where this was written, so they were NOT checked against
either.  Each takes one slot of the ``SomeOf`` block (slots 5..9):
  * blur ``OneOf``: one third of the time ``GaussianBlur``: sigma ~ U(0, 3), no blur if sigma < 0.001,
    ``k = int(max(3.3 sigma, 5))`` (sigma < 3) made odd by + 1, weights ``exp(-d^2 / 2 sigma^2)`` normalised, the separable
    outer product; one third ``AverageBlur``: integer k ~ U{2..7}, window ``[x - k//2, x - k//2 + k - 1]``, weights 1/k^2,
    embedded in the next odd K; one third ``MedianBlur``: nothing happens here, ``blends()`` builds it (below);
  * ``Sharpen``: alpha ~ U(0, 1), lightness l ~ U(0.75, 1.5): ``(1 - alpha) delta + alpha [[-1,-1,-1],[-1,8+l,-1],[-1,-1,-1]]``;
  * ``Emboss``: alpha ~ U(0, 1), strength s ~ U(0, 2): ``(1 - alpha) delta + alpha [[-1-s,-s,0],[-s,1,s],[0,s,1+s]]``;
  * ``AdditiveGaussianNoise``: scale ~ U(0, 12.75), per channel with probability 0.5;
  * dropout ``OneOf``: ``Dropout``: p ~ U(0.01, 0.1), per channel 0.5; or ``CoarseDropout``: p ~ U(0.03, 0.15), size fraction
    f ~ U(0.02, 0.05), mask ``mh = max(4, int(H f))``, ``mw = max(4, int(W f))``, per channel 0.2; pixel (y, x) takes the
    draw of mask cell ``(y mh // H, x mw // W)``.
Filters are correlations (cv2 ``filter2D``, which imgaug's ``Convolve`` calls) with cv2's default border (reflect without
repeating the edge pixel).  Noise and dropout are drawn on the device: Philox4x32-10 keyed by a 64-bit seed that the host
draws per sample, counted by the working-grid pixel (include/pseg_amd.h).

Local warps (``warps()``).  Like the filters', these draws are THIS MODULE'S CONTRACT, written down from imgaug's
documentation and NOT checked against imgaug.  Each takes one slot of the ``SomeOf`` block (slots 10..12) and, when picked,
applies with its ``Sometimes`` probability (0.5 each).  The kernel's inverse coordinate map is, from the output pixel towards
the source: elastic jitter -> displacement grid -> inverse homography (include/pseg_amd.h has the arithmetic):
  * ``ElasticTransformation``: alpha ~ U(0.5, 3.5); every pixel is displaced by alpha * U(-1, 1) per axis, drawn on the device
    (Philox stream 8 of the sample's seed, counted by the pixel).  The reference smooths the displacement field with a
    Gaussian of sigma 0.25; that is NOT applied: a 3-tap Gaussian of that sigma weighs its neighbours 3e-4;
  * ``PiecewiseAffine``: s ~ U(0.01, 0.05), each of the 4 x 4 control points is moved by N(0, s) per coordinate, as a fraction
    of (W, H).  The row holds MINUS the jitter times (W, H) per node, the first-order inverse of moving the control points,
    and the kernel blends it bilinearly inside each of the 3 x 3 cells, where the reference triangulates the cells and maps
    each triangle by its own affine;
  * ``PerspectiveTransform``: s ~ U(0.01, 0.1), |N(0, s)| per corner coordinate, clipped to 0.4; each corner moves INWARD by that
    fraction of (W - 1, H - 1) and the homography that maps the moved quad onto the image corners is multiplied in after the
    affine (imgaug's ``keep_size``: a zoom onto the quad).  The clip keeps each corner in its own quadrant; that alone does
    not keep the quad convex when several corners reach it (4 sigma and more), so a draw whose quad is not strictly
    convex is dropped (the slot then does nothing, which puts the slot's rate a hair below 2.5 / 16 * 0.5: of 20000
    draws at s = 0.1, the upper end, none was dropped).  For a convex quad the inverse's denominator is positive on the whole
    grid, which ``rows()`` checks: it raises ``ValueError`` for a hand-made recipe that fails it.

Median, blends, hue and saturation (``blends()``).  Like the filters' and the warps', these draws and formulas are THIS
MODULE'S CONTRACT, written down from imgaug's documentation and NOT checked against imgaug or cv2 (include/pseg_amd.h has
the kernel's arithmetic, stage by stage):
  * ``MedianBlur``, the blur ``OneOf``'s third branch: integer k ~ U{3..11}, made odd by + 1 when even, capped at 11; per
    channel the median of the k x k window, border reflected as the filters'.  As in the ``OneOf`` that draw holds no Gaussian
    or average blur; a picked sharpen / emboss still composes into F, which runs after the median;
  * the edge-detect blend (slot 13, ``BlendAlphaSimplexNoise(OneOf([EdgeDetect, DirectedEdgeDetect]))``): alpha ~ U(0.5, 1);
    half of the time ``EdgeDetect``, ``(1 - alpha) delta + alpha [[0,1,0],[1,-4,1],[0,1,0]]``, otherwise
    ``DirectedEdgeDetect`` with direction ~ U(0, 1) of a turn: a 3 x 3 kernel with centre 1 whose eight neighbours are weighted
    by the squared clipped cosine between their direction and the drawn one and normalised to sum to -1, blended with delta
    the same way.  The picked linear filters compose to F and the edge filter E is linear too, so the blend
    ``m E(F x) + (1 - m) F x`` is two filters over the same pixels, F and G = E * F (full 2-D convolution in fp64, E itself
    without a filter; K2 <= 15 follows from K <= 13), blended per pixel by the mask m = T1.  T1 is a blobby 16 x 16 table that
    the kernel samples bilinearly over the image: the sum of 1..3 octaves, each a random g x g grid, g ~ U{2..16}, resized to
    16 x 16 with the sample's draw of nearest or linear, normalised to [0, 1] and, half of the time, passed through the
    sigmoid ``1 / (1 + exp(-10 (m - 0.5)))``.  That is VALUE noise: there is no gradient-noise library here, and it is not
    simplex noise;
  * ``AddToHueAndSaturation((-20, 20))`` (slot 14): one integer v ~ U{-20..20} serves both, dh = 6 v / 255 sixths of the colour
    circle and ds = v / 255: imgaug's one value applied to cv2's 8-bit HSV, whose hue covers the half-circle in 180 steps.
    The kernel converts the 8-bit RGB to hue / saturation / value in fp32, shifts, wraps the hue, clamps the saturation and
    converts back;
  * the frequency-noise blend, the other half of the Multiply ``OneOf``
    (``BlendAlphaFrequencyNoise(foreground=Multiply, background=LinearContrast)``): Ma is Multiply per channel, U(0.5, 1.5)
    each, Mb is LinearContrast, U(0.5, 2); both are affine, so each is composed with the sample's other colour operations on
    either side, in the order drawn, into one pair (M, Mb), and the kernel blends ``m (M v) + (1 - m) (Mb v)`` per pixel by
    the mask m = T2: a 16 x 16 random-phase spectrum weighted by ``|f|^exponent``, exponent ~ U(-4, 0), through
    ``numpy.fft.irfft2``, normalised to [0, 1], with the same sigmoid coin.
Both tables are fp32, finite and in [0, 1]; ``rows()`` checks them, the median window and K2, and raises ``ValueError`` for a
hand-made recipe outside the ranges.

OUT OF SCOPE -- the last slot of the block, Superpixels (it needs a segmentation pass); and imgaug's border modes other
than constant and edge (``ia.ALL`` also draws reflect, symmetric and wrap).

Simplifications, all on the host side: the geometric augmenters run in the fixed order flips, crop-and-pad, affine,
perspective, piecewise-affine, elastic (the reference shuffles the top-level list and the block), and the chain is ONE warp (imgaug resamples once per augmenter); one (order, cval,
mode) triple serves a sample -- crop-and-pad alone is bilinear, the affine's own draw wins when it is active; the colour
operations are composed into one matrix, so the 8-bit rounding and saturation that imgaug applies between two of them
happens once, after the last; the picked filters of a sample (blur, sharpen, emboss) are composed, in fp64, into ONE K x K
filter by full 2-D convolution (K <= 13: 9 + 2 + 2), which likewise gives up the 8-bit rounding between them (and the
border handling of each on its own), and there is no 8-bit rounding between F and the edge filter E either (G = E * F is one
filter); the masks are value noise where the reference has simplex noise; and the stages of a sample run in the fixed order
warp, median, filter / edge blend, colour matrix (or the two blended), hue-saturation, noise, dropout, whatever order the
``SomeOf`` block drew (the reference applies the picked augmenters in a random order).
"""
import numpy as np
import torch

from .datasets import MEAN, STD

ROW = 24                         # PSEG_AUGMENT_ROW
CONTRAST_CENTRE = 127.0          # imgaug LinearContrast on uint8: 127 + alpha * (v - 127)
GRAY_WEIGHTS = (0.299, 0.587, 0.114)
COLOUR_SLOTS = 16                # augmenters in the reference's SomeOf block
_COLOUR_OPS = ('invert', 'add', 'multiply', 'contrast', 'grayscale')
MODES = {'constant': 0, 'edge': 1}
NBHD_ROW = 212                   # PSEG_AUGMENT_NBHD_ROW; the offsets below are PSEG_AUGMENT_NBHD_* of include/pseg_amd.h
NBHD_KMAX = 13
NBHD_K, NBHD_NOISE, NBHD_DROP, NBHD_SEED, NBHD_WEIGHTS = 24, 25, 27, 31, 40
_NBHD_OPS = ('blur', 'sharpen', 'emboss', 'noise', 'dropout')        # slots 5..9 of the SomeOf block
WARP_ROW = 252                   # PSEG_AUGMENT_WARP_ROW; the offsets below are PSEG_AUGMENT_WARP_* of include/pseg_amd.h
WARP_H2, WARP_ALPHA, WARP_GRID_ON, WARP_GRID = 212, 215, 216, 220
WARP_NODES = 4                   # the displacement grid is 4 x 4 nodes of (dx, dy)
_WARP_OPS = ('elastic', 'piecewise', 'perspective')                  # slots 10..12
BLEND_ROW = 1012                 # PSEG_AUGMENT_BLEND_ROW; the offsets below are PSEG_AUGMENT_BLEND_* of include/pseg_amd.h
BLEND_KMEDMAX, BLEND_K2MAX = 11, 15
BLEND_KMED, BLEND_K2, BLEND_COLOUR_ON, BLEND_HUE, BLEND_MB, BLEND_WEIGHTS2 = 252, 253, 254, 255, 260, 272
BLEND_T1, BLEND_T2, BLEND_TABLE = 500, 756, 16                       # two 16 x 16 mask tables
_BLEND_OPS = ('edge_blend', 'hue_sat')                               # slots 13, 14 (slot 15, Superpixels, is not built)
_BLEND_KEYS = ('median', 'edge', 'hue_sat', 'colour_mask')           # recipe keys that send a batch to pseg_augment_batch_blend
SIGMOID_GAIN = 10.0              # the masks' optional sigmoid: 1 / (1 + exp(-10 (m - 0.5)))
PERSPECTIVE_CLIP = 0.4          # a corner moves inward by less than half a side and stays in its own quadrant (that alone
                                 # does not keep the quad convex: quad_is_convex)


def _eye3():
    return np.eye(3, dtype=np.float64)


def flip_matrix(H, W, lr, ud):
    m = _eye3()
    if lr:
        m[0, 0], m[0, 2] = -1.0, W - 1.0
    if ud:
        m[1, 1], m[1, 2] = -1.0, H - 1.0
    return m


def crop_pad_matrix(H, W, top, right, bottom, left):
    """source index -> output index of CropAndPad(percent=(top, right, bottom, left), keep_size=True): the image grows by the
    fractions on each side (negative: shrinks) and is resized back to H x W, pixel centres at index + 0.5 of the edge grid."""
    kx, ky = 1.0 / (1.0 + left + right), 1.0 / (1.0 + top + bottom)
    m = _eye3()
    m[0, 0], m[0, 2] = kx, kx * (left * W + 0.5) - 0.5
    m[1, 1], m[1, 2] = ky, ky * (top * H + 0.5) - 0.5
    return m


def affine_matrix(H, W, rotate=0.0, scale=(1.0, 1.0), shear=0.0, translate=(0.0, 0.0)):
    """source index -> output index: scale, shear, rotate about the image centre ((W-1)/2, (H-1)/2), then translate by
    fractions of the image size.  Angles in degrees."""
    c = _eye3()
    c[0, 2], c[1, 2] = (W - 1) / 2.0, (H - 1) / 2.0
    r, s = np.deg2rad(rotate), np.deg2rad(shear)
    R = np.array([[np.cos(r), -np.sin(r), 0.0], [np.sin(r), np.cos(r), 0.0], [0.0, 0.0, 1.0]])
    Sh = np.array([[1.0, -np.tan(s), 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    S = np.diag([float(scale[0]), float(scale[1]), 1.0])
    T = _eye3()
    T[0, 2], T[1, 2] = translate[0] * W, translate[1] * H
    return T @ c @ R @ Sh @ S @ np.linalg.inv(c)


def _moved_quad(corners, w=1.0, h=1.0):
    f = np.asarray(corners, dtype=np.float64).reshape(4, 2)
    return np.array([[f[0, 0] * w, f[0, 1] * h], [w - f[1, 0] * w, f[1, 1] * h], [w - f[2, 0] * w, h - f[2, 1] * h],
                     [f[3, 0] * w, h - f[3, 1] * h]])


def quad_is_convex(corners):
    """the quad that the inward corner moves leave is strictly convex (whatever the image size: scaling keeps convexity).
    Only then is its homography onto the image corners one with a positive denominator on the whole grid."""
    q = _moved_quad(corners)
    e = np.roll(q, -1, axis=0) - q
    return bool((e[:, 0] * np.roll(e, -1, axis=0)[:, 1] - e[:, 1] * np.roll(e, -1, axis=0)[:, 0] > 0).all())


def perspective_matrix(H, W, corners):
    """source index -> output index (3x3, fp64) of PerspectiveTransform(keep_size=True): corners [4, 2] = (fx, fy) of the top
    left, top right, bottom right and bottom left corner, each moved INWARD by that fraction of (W - 1, H - 1); the
    homography sends the moved quad to the image corners.  The identity where the image is a line (H or W of 1)."""
    if min(H, W) < 2:
        return _eye3()
    w, h = W - 1.0, H - 1.0
    src = _moved_quad(corners, w, h)
    dst = np.array([[0.0, 0.0], [w, 0.0], [w, h], [0.0, h]])
    A, b = np.zeros((8, 8)), np.zeros(8)
    for k, ((x, y), (u, v)) in enumerate(zip(src, dst)):      # u = (m00 x + m01 y + m02) / (m20 x + m21 y + 1), v likewise
        A[2 * k], b[2 * k] = [x, y, 1, 0, 0, 0, -u * x, -u * y], u
        A[2 * k + 1], b[2 * k + 1] = [0, 0, 0, x, y, 1, -v * x, -v * y], v
    return np.append(np.linalg.solve(A, b), 1.0).reshape(3, 3)


def colour_op_matrix(name, value):
    """4x4 homogeneous matrix (0..255 units) of one named colour operation; per-channel values are length-3."""
    m = np.eye(4, dtype=np.float64)
    if name == 'add':
        m[:3, 3] = value
    elif name == 'multiply':
        m[:3, :3] = np.diag(np.asarray(value, dtype=np.float64))
    elif name == 'contrast':
        a = np.asarray(value, dtype=np.float64)
        m[:3, :3] = np.diag(a)
        m[:3, 3] = CONTRAST_CENTRE * (1.0 - a)
    elif name == 'invert':
        for c in range(3):
            if value[c]:
                m[c, c], m[c, 3] = -1.0, 255.0
    elif name == 'grayscale':
        a = float(value)
        m[:3, :3] = (1.0 - a) * np.eye(3) + a * np.tile(np.asarray(GRAY_WEIGHTS, dtype=np.float64), (3, 1))
    else:
        raise ValueError('unknown colour operation %r' % (name,))
    return m


def colour_matrix(colour_ops):
    """3x4 matrix of a list of (name, value) operations applied first to last."""
    m = np.eye(4, dtype=np.float64)
    for name, value in colour_ops:
        m = colour_op_matrix(name, value) @ m
    return m[:3]


def forward_matrix(recipe, H, W):
    """source index -> output index of a recipe's whole geometric chain (3x3, fp64)."""
    m = flip_matrix(H, W, recipe.get('fliplr', False), False)
    m = flip_matrix(H, W, False, recipe.get('flipud', False)) @ m
    if recipe.get('crop_pad') is not None:
        m = crop_pad_matrix(H, W, *recipe['crop_pad']) @ m
    if recipe.get('affine') is not None:
        m = affine_matrix(H, W, **recipe['affine']) @ m
    if recipe.get('perspective') is not None:
        m = perspective_matrix(H, W, recipe['perspective']) @ m
    return m


def make_row(inverse=None, colour=None, cval=0.0, order=0, mode=0):
    """one parameter row from an inverse affine (2x3 or 3x3: output index -> source index), a 3x4 colour matrix, the fill
    value, the interpolation order (0 nearest, 1 bilinear) and the border mode (0 / 'constant', 1 / 'edge')."""
    row = np.zeros(ROW, dtype=np.float32)
    row[0:6] = (np.eye(3)[:2] if inverse is None else np.asarray(inverse, dtype=np.float64)[:2]).reshape(6)
    row[6:18] = (np.eye(4)[:3] if colour is None else np.asarray(colour, dtype=np.float64)).reshape(12)
    row[18], row[19], row[20] = cval, order, MODES.get(mode, mode)
    return row


def gaussian_kernel(sigma):
    """GaussianBlur(sigma) as a K x K correlation filter (fp64), None below sigma = 0.001"""
    if sigma < 0.001:
        return None
    k = int(max(3.3 * sigma, 5))
    k += 1 - k % 2
    d = np.arange(k, dtype=np.float64) - k // 2
    g = np.exp(-d * d / (2.0 * sigma * sigma))
    g /= g.sum()
    return np.outer(g, g)


def average_kernel(k):
    """AverageBlur(k): the mean over the window [x - k//2, x - k//2 + k - 1], embedded in the next odd K"""
    k = int(k)
    K = k + 1 - k % 2
    m = np.zeros((K, K), dtype=np.float64)
    m[:k, :k] = 1.0 / (k * k)
    return m


def _blend_with_identity(alpha, m):
    out = alpha * np.asarray(m, dtype=np.float64)
    out[1, 1] += 1.0 - alpha
    return out


def sharpen_kernel(alpha, lightness):
    return _blend_with_identity(alpha, [[-1, -1, -1], [-1, 8 + lightness, -1], [-1, -1, -1]])


def emboss_kernel(alpha, strength):
    s = strength
    return _blend_with_identity(alpha, [[-1 - s, -s, 0], [-s, 1, s], [0, s, 1 + s]])


def filter_kernel(name, *args):
    return {'gaussian': gaussian_kernel, 'average': average_kernel, 'sharpen': sharpen_kernel, 'emboss': emboss_kernel}[name](*args)


def compose_filters(kernels):
    """one filter that stands for the correlation filters applied one after the other: their full 2-D convolution (fp64)"""
    out = np.ones((1, 1), dtype=np.float64)
    for k in kernels:
        k = np.asarray(k, dtype=np.float64)
        acc = np.zeros((out.shape[0] + k.shape[0] - 1, out.shape[1] + k.shape[1] - 1), dtype=np.float64)
        for j in range(k.shape[0]):
            for i in range(k.shape[1]):
                acc[j:j + out.shape[0], i:i + out.shape[1]] += k[j, i] * out
        out = acc
    return out


def make_nbhd_row(base=None, kernel=None, noise=None, dropout=None, seed=0):
    """one row of pseg_augment_batch_nbhd's table from a make_row() row, a K x K filter (K odd, at most NBHD_KMAX), noise =
    (scale, per_channel), dropout = (p, per_channel[, mh, mw]) and the sample's 64-bit seed (bit-cast, not converted)"""
    row = np.zeros(NBHD_ROW, dtype=np.float32)
    row[:ROW] = make_row() if base is None else base
    if kernel is not None:
        kernel = np.asarray(kernel, dtype=np.float64)
        K = kernel.shape[0]
        if kernel.shape != (K, K) or K % 2 == 0 or K > NBHD_KMAX:
            raise ValueError('a filter is K x K with K odd and at most %d, not %s' % (NBHD_KMAX, kernel.shape))
        row[NBHD_K] = K
        row[NBHD_WEIGHTS:NBHD_WEIGHTS + K * K] = kernel.reshape(-1)
    if noise is not None:
        row[NBHD_NOISE], row[NBHD_NOISE + 1] = noise[0], bool(noise[1])
    if dropout is not None:
        row[NBHD_DROP], row[NBHD_DROP + 1] = dropout[0], bool(dropout[1])
        if len(dropout) > 2:
            row[NBHD_DROP + 2], row[NBHD_DROP + 3] = dropout[2], dropout[3]
    row.view(np.uint32)[NBHD_SEED:NBHD_SEED + 2] = (int(seed) & 0xffffffff, (int(seed) >> 32) & 0xffffffff)
    return row


def make_warp_row(base=None, h2=None, alpha=None, grid=None):
    """one row of pseg_augment_batch_warp's table from a make_nbhd_row() row (its [0..5] are the first two rows of the inverse
    homography), the third row h2 (None: 0 0 1), the elastic alpha in pixels (None: no jitter) and the [4, 4, 2]
    displacement grid of (dx, dy) in pixels, node (j, i) at [j, i] (None: off)"""
    row = np.zeros(WARP_ROW, dtype=np.float32)
    base = np.ascontiguousarray(make_nbhd_row() if base is None else base, dtype=np.float32)
    row.view(np.uint32)[:NBHD_ROW] = base.view(np.uint32)                # (the seed's bits, not its value as a float)
    row[WARP_H2:WARP_H2 + 3] = (0.0, 0.0, 1.0) if h2 is None else h2
    if alpha is not None:
        row[WARP_ALPHA] = alpha
    if grid is not None:
        grid = np.asarray(grid, dtype=np.float64)
        if grid.shape != (WARP_NODES, WARP_NODES, 2):
            raise ValueError('a displacement grid is %d x %d x 2, not %s' % (WARP_NODES, WARP_NODES, grid.shape))
        row[WARP_GRID_ON] = 1.0
        row[WARP_GRID:WARP_GRID + 2 * WARP_NODES ** 2] = grid.reshape(-1)
    return row


def edge_detect_kernel(alpha):
    """EdgeDetect(alpha): (1 - alpha) delta + alpha [[0,1,0],[1,-4,1],[0,1,0]]"""
    return _blend_with_identity(alpha, [[0, 1, 0], [1, -4, 1], [0, 1, 0]])


def directed_edge_kernel(alpha, direction):
    """DirectedEdgeDetect(alpha, direction in turns, 0 = up, clockwise): centre 1, each of the eight neighbours weighted by
    the squared clipped cosine between its direction and the drawn one, normalised to sum to -1; blended with delta"""
    a = 2.0 * np.pi * float(direction)
    d = np.array([np.sin(a), -np.cos(a)])                                 # (x, y), y down
    m = np.zeros((3, 3), dtype=np.float64)
    for j in range(3):
        for i in range(3):
            if (j, i) != (1, 1):
                c = np.array([i - 1.0, j - 1.0])
                m[j, i] = max(float(c @ d) / float(np.linalg.norm(c)), 0.0) ** 2
    m *= -1.0 / m.sum()
    m[1, 1] = 1.0
    return _blend_with_identity(alpha, m)


def edge_kernel(alpha, direction=None):
    return edge_detect_kernel(alpha) if direction is None else directed_edge_kernel(alpha, direction)


def _unit_range(m, sigmoid):
    """a mask normalised to [0, 1] (a flat one becomes 0.5), optionally through the sigmoid; fp32"""
    m = np.asarray(m, dtype=np.float64)
    span = m.max() - m.min()
    m = (m - m.min()) / span if span > 0 else np.full_like(m, 0.5)
    if sigmoid:
        m = 1.0 / (1.0 + np.exp(-SIGMOID_GAIN * (m - 0.5)))
    return np.clip(m, 0.0, 1.0).astype(np.float32)


def resize_to_table(grid, linear):
    """a g x g grid -> BLEND_TABLE x BLEND_TABLE, pixel centres aligned: nearest, or bilinear with the border clamped"""
    grid = np.asarray(grid, dtype=np.float64)
    g, n = grid.shape[0], BLEND_TABLE
    c = (np.arange(n) + 0.5) * g / n - 0.5
    if not linear:
        i = np.clip(np.floor(c + 0.5).astype(np.int64), 0, g - 1)
        return grid[i][:, i]
    c = np.clip(c, 0.0, g - 1.0)
    i0 = np.minimum(c.astype(np.int64), max(g - 2, 0))
    i1, f = np.minimum(i0 + 1, g - 1), c - i0
    rows = grid[i0] * (1.0 - f)[:, None] + grid[i1] * f[:, None]
    return rows[:, i0] * (1.0 - f)[None] + rows[:, i1] * f[None]


def value_noise_table(rng):
    """T1, the edge blend's mask: the sum of 1..3 octaves of VALUE noise (a random g x g grid, g in 2..16, resized to the table
    with the sample's draw of nearest or linear), normalised, through the sigmoid half of the time.  Not simplex noise."""
    linear = bool(rng.integers(2))
    total = np.zeros((BLEND_TABLE, BLEND_TABLE), dtype=np.float64)
    for _ in range(int(rng.integers(1, 4))):
        g = int(rng.integers(2, BLEND_TABLE + 1))
        total += resize_to_table(rng.random((g, g)), linear)
    return _unit_range(total, bool(rng.random() < 0.5))


def frequency_noise_table(rng):
    """T2, the colour blend's mask: a random-phase spectrum weighted by |f|^exponent, exponent ~ U(-4, 0) (no mean term),
    back through numpy.fft.irfft2, normalised, through the sigmoid half of the time"""
    n = BLEND_TABLE
    exponent = float(rng.uniform(-4.0, 0.0))
    f = np.hypot(np.fft.fftfreq(n)[:, None], np.fft.rfftfreq(n)[None])
    weight = np.zeros_like(f)
    weight[f > 0] = f[f > 0] ** exponent
    spectrum = weight * np.exp(2j * np.pi * rng.random(f.shape))
    return _unit_range(np.fft.irfft2(spectrum, s=(n, n)), bool(rng.random() < 0.5))


def hue_sat_shift(v):
    """AddToHueAndSaturation's one integer v -> (dh in sixths of the colour circle, ds as a fraction): imgaug applies the one
    value to cv2's 8-bit HSV, v / 255 of the hue's range and v / 255 of the saturation's: dh = 6 v / 255, ds = v / 255"""
    return 6.0 * float(v) / 255.0, float(v) / 255.0


def _check_table(name, t):
    t = np.asarray(t, dtype=np.float32)
    if t.shape != (BLEND_TABLE, BLEND_TABLE) or not np.isfinite(t).all() or t.min() < 0.0 or t.max() > 1.0:
        raise ValueError('%s is a finite %d x %d table in [0, 1]' % (name, BLEND_TABLE, BLEND_TABLE))
    return t


def make_blend_row(base=None, kmed=0, kernel2=None, colour2=None, t1=None, t2=None, hue_sat=None):
    """one row of pseg_augment_batch_blend's table from a make_warp_row() row, the median window kmed (0, or odd 3..11), the
    second filter G (K2 x K2, K2 odd, 3..15) with its mask table t1, the second colour matrix Mb (3x4) with its mask table t2
    (colour2 switches the colour blend on), and hue_sat = (dh, ds).  ValueError outside the ranges."""
    row = np.zeros(BLEND_ROW, dtype=np.float32)
    base = np.ascontiguousarray(make_warp_row() if base is None else base, dtype=np.float32)
    row.view(np.uint32)[:WARP_ROW] = base.view(np.uint32)                # (the seed's bits)
    kmed = int(kmed)
    if kmed != 0 and (kmed < 3 or kmed > BLEND_KMEDMAX or kmed % 2 == 0):
        raise ValueError('a median window is 0 or odd, 3..%d, not %d' % (BLEND_KMEDMAX, kmed))
    row[BLEND_KMED] = kmed
    if kernel2 is not None:
        kernel2 = np.asarray(kernel2, dtype=np.float64)
        K2 = kernel2.shape[0]
        if kernel2.shape != (K2, K2) or K2 % 2 == 0 or K2 < 3 or K2 > BLEND_K2MAX:
            raise ValueError('a second filter is K2 x K2 with K2 odd, 3..%d, not %s' % (BLEND_K2MAX, kernel2.shape))
        row[BLEND_K2] = K2
        row[BLEND_WEIGHTS2:BLEND_WEIGHTS2 + K2 * K2] = kernel2.reshape(-1)
    if t1 is not None:
        row[BLEND_T1:BLEND_T1 + BLEND_TABLE ** 2] = _check_table('t1', t1).reshape(-1)
    row[BLEND_MB:BLEND_MB + 12] = np.eye(4)[:3].reshape(12)
    if colour2 is not None:
        row[BLEND_COLOUR_ON] = 1.0
        row[BLEND_MB:BLEND_MB + 12] = np.asarray(colour2, dtype=np.float64).reshape(12)
    if t2 is not None:
        row[BLEND_T2:BLEND_T2 + BLEND_TABLE ** 2] = _check_table('t2', t2).reshape(-1)
    if hue_sat is not None:
        if not np.isfinite(hue_sat).all():
            raise ValueError('hue_sat = (dh, ds) is finite, not %s' % (tuple(hue_sat),))
        row[BLEND_HUE], row[BLEND_HUE + 1] = hue_sat
    return row


def row_shapes(table):
    """int32 [B, 3] = {K, mh, mw} of each row: what pseg_augment_batch_nbhd / _warp validate on the host; for rows of
    BLEND_ROW floats [B, 5] = {K, mh, mw, kmed, K2}, pseg_augment_batch_blend's"""
    table = np.asarray(table)
    cols = [NBHD_K, NBHD_DROP + 2, NBHD_DROP + 3] + ([BLEND_KMED, BLEND_K2] if table.shape[1] == BLEND_ROW else [])
    return np.ascontiguousarray(table[:, cols].astype(np.int32))


def _range(v):
    return None if v is None else (float(v[0]), float(v[1]))


class DeviceAugment:
    """See the module docstring.  A probability of 0 or a range of None switches an augmenter off."""

    def __init__(self, fliplr=0.5, flipud=0.2, crop_pad=(-0.05, 0.1), crop_pad_p=0.5, affine_p=0.5, scale=(0.8, 1.2),
                 translate=(-0.2, 0.2), rotate=(-90.0, 90.0), shear=(-16.0, 16.0), orders=(0, 1), cval=(0, 255),
                 modes=('constant', 'edge'), add=(-10, 10), multiply=(0.5, 1.5), contrast=(0.5, 2.0), invert=0.05,
                 grayscale=(0.0, 1.0), per_channel=0.5, some_of=(0, 5), seed=None, rank=None, mean=MEAN, std=STD,
                 gaussian_blur=None, average_blur=None, sharpen_alpha=None, sharpen_lightness=(0.75, 1.5), emboss_alpha=None,
                 emboss_strength=(0.0, 2.0), noise_scale=None, noise_per_channel=0.5, dropout_p=None, dropout_per_channel=0.5,
                 coarse_p=None, coarse_size=(0.02, 0.05), coarse_per_channel=0.2, elastic_alpha=None, elastic_p=None,
                 piecewise_scale=None, piecewise_p=None, perspective_scale=None, perspective_p=None, median_blur=None,
                 edge_blend=None, hue_sat=None, frequency_blend=False):
        self.fliplr, self.flipud = float(fliplr), float(flipud)
        self.crop_pad, self.crop_pad_p = _range(crop_pad), float(crop_pad_p if crop_pad is not None else 0.0)
        if self.crop_pad is not None and self.crop_pad[0] <= -0.45:
            raise ValueError('crop_pad: cropping %g of a side from both ends leaves no image' % -self.crop_pad[0])
        self.affine_p = float(affine_p)
        self.scale, self.translate, self.rotate, self.shear = _range(scale), _range(translate), _range(rotate), _range(shear)
        self.orders, self.cval, self.modes = tuple(orders), _range(cval), tuple(MODES[m] for m in modes)
        self.add, self.multiply, self.contrast = _range(add), _range(multiply), _range(contrast)
        self.invert, self.grayscale = float(invert or 0.0), _range(grayscale)
        self.per_channel, self.some_of = float(per_channel), (int(some_of[0]), int(some_of[1]))
        self.seed, self.rank = seed, rank
        self.mean, self.std = tuple(mean), tuple(std)
        # the neighbourhood and per-pixel-random augmenters: a range of None (the default) switches one off
        self.gaussian_blur, self.average_blur = _range(gaussian_blur), _range(average_blur)
        self.sharpen_alpha, self.sharpen_lightness = _range(sharpen_alpha), _range(sharpen_lightness)
        self.emboss_alpha, self.emboss_strength = _range(emboss_alpha), _range(emboss_strength)
        self.noise_scale, self.noise_per_channel = _range(noise_scale), float(noise_per_channel)
        self.dropout_p, self.dropout_per_channel = _range(dropout_p), float(dropout_per_channel)
        self.coarse_p, self.coarse_size, self.coarse_per_channel = _range(coarse_p), _range(coarse_size), float(coarse_per_channel)
        # the local warps: a range or a probability of None (the default) switches one off
        self.elastic_alpha, self.elastic_p = _range(elastic_alpha), None if elastic_p is None else float(elastic_p)
        self.piecewise_scale, self.piecewise_p = _range(piecewise_scale), None if piecewise_p is None else float(piecewise_p)
        self.perspective_scale, self.perspective_p = _range(perspective_scale), None if perspective_p is None else float(perspective_p)
        # the median blur, the two noise-masked blends and hue / saturation: None / False (the default) switches one off
        self.median_blur, self.edge_blend, self.hue_sat = _range(median_blur), _range(edge_blend), _range(hue_sat)
        self.frequency_blend = bool(frequency_blend)
        self._rng = None

    @classmethod
    def reference(cls, **kw):
        """the reference's TRAIN_AUGS values (the constructor defaults)"""
        return cls(**kw)

    @classmethod
    def full(cls, **kw):
        """reference() plus GaussianBlur / AverageBlur, Sharpen, Emboss, AdditiveGaussianNoise and Dropout / CoarseDropout at
        the reference's ranges: 10 of the 16 slots of the SomeOf block"""
        on = dict(gaussian_blur=(0.0, 3.0), average_blur=(2, 7), sharpen_alpha=(0.0, 1.0), emboss_alpha=(0.0, 1.0),
                  noise_scale=(0.0, 0.05 * 255), dropout_p=(0.01, 0.1), coarse_p=(0.03, 0.15))
        on.update(kw)
        return cls(**on)

    @classmethod
    def warps(cls, **kw):
        """full() plus ElasticTransformation, PiecewiseAffine and PerspectiveTransform at the reference's ranges, each
        Sometimes(0.5): 13 of the 16 slots of the SomeOf block"""
        on = dict(elastic_alpha=(0.5, 3.5), elastic_p=0.5, piecewise_scale=(0.01, 0.05), piecewise_p=0.5,
                  perspective_scale=(0.01, 0.1), perspective_p=0.5)
        on.update(kw)
        return cls.full(**on)

    @classmethod
    def blends(cls, **kw):
        """warps() plus MedianBlur (the blur OneOf's third branch), the edge-detect blend, AddToHueAndSaturation and the
        frequency-noise blend (the Multiply OneOf's other branch) at the reference's ranges: 15 of the 16 slots of the SomeOf
        block, every OneOf complete"""
        on = dict(median_blur=(3, 11), edge_blend=(0.5, 1.0), hue_sat=(-20, 20), frequency_blend=True)
        on.update(kw)
        return cls.warps(**on)

    @classmethod
    def identity(cls, order=0, **kw):
        """samples only identity rows (order 0 or 1): the kernel then computes exactly CocoDataset.post_fetch_fn"""
        return cls(fliplr=0.0, flipud=0.0, crop_pad=None, affine_p=0.0, orders=(order,), cval=(0, 0), modes=('constant',),
                   add=None, multiply=None, contrast=None, invert=0.0, grayscale=None, some_of=(0, 0), **kw)

    # ------------------------------------------------------------------ drawing
    @property
    def rng(self):
        if self._rng is None:            # made at the first draw: the process group exists by then
            if self.seed is None:
                self._rng = np.random.default_rng()
            else:
                rank = self.rank
                if rank is None:
                    import torch.distributed as dist
                    rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
                self._rng = np.random.default_rng(int(self.seed) + int(rank))
        return self._rng

    def _values(self, rng, lo_hi, integer=False):
        """one value for the image, or one per channel (per_channel of the time) -> length-3 array"""
        n = 3 if rng.random() < self.per_channel else 1
        v = rng.integers(int(lo_hi[0]), int(lo_hi[1]) + 1, n).astype(np.float64) if integer else rng.uniform(lo_hi[0], lo_hi[1], n)
        return np.broadcast_to(v, (3,)).copy()

    def _draw_nbhd(self, rng, name, nbhd):
        """one picked slot of the five neighbourhood / per-pixel-random augmenters -> nbhd (an augmenter that is off draws
        nothing, so the default tables are those of the colour-only sampler)"""
        if name == 'blur' and (self.gaussian_blur is not None or self.average_blur is not None or self.median_blur is not None):
            which = int(rng.integers(3))                      # Gaussian, average, median
            if which == 0 and self.gaussian_blur is not None:
                sigma = float(rng.uniform(*self.gaussian_blur))
                if sigma >= 0.001:
                    nbhd.setdefault('filters', []).append(('gaussian', sigma))
            elif which == 1 and self.average_blur is not None:
                k = int(rng.integers(int(self.average_blur[0]), int(self.average_blur[1]) + 1))
                if k > 1:
                    nbhd.setdefault('filters', []).append(('average', k))
            elif which == 2 and self.median_blur is not None:
                k = int(rng.integers(int(self.median_blur[0]), int(self.median_blur[1]) + 1))
                nbhd['median'] = min(k + 1 - k % 2, BLEND_KMEDMAX)
        elif name == 'sharpen' and self.sharpen_alpha is not None:
            nbhd.setdefault('filters', []).append(('sharpen', float(rng.uniform(*self.sharpen_alpha)),
                                                   float(rng.uniform(*self.sharpen_lightness))))
        elif name == 'emboss' and self.emboss_alpha is not None:
            nbhd.setdefault('filters', []).append(('emboss', float(rng.uniform(*self.emboss_alpha)),
                                                   float(rng.uniform(*self.emboss_strength))))
        elif name == 'noise' and self.noise_scale is not None:
            nbhd['noise'] = (float(rng.uniform(*self.noise_scale)), bool(rng.random() < self.noise_per_channel))
        elif name == 'dropout' and (self.dropout_p is not None or self.coarse_p is not None):
            which = int(rng.integers(2))                      # Dropout, CoarseDropout
            if which == 0 and self.dropout_p is not None:
                nbhd['dropout'] = {'p': float(rng.uniform(*self.dropout_p)), 'per_channel': bool(rng.random() < self.dropout_per_channel),
                                   'size': None}
            elif which == 1 and self.coarse_p is not None:
                nbhd['dropout'] = {'p': float(rng.uniform(*self.coarse_p)), 'per_channel': bool(rng.random() < self.coarse_per_channel),
                                   'size': float(rng.uniform(*self.coarse_size))}

    def _draw_warp(self, rng, name, nbhd):
        """one picked slot of the three local warps -> nbhd (one that is off draws nothing)"""
        scale, p = {'elastic': (self.elastic_alpha, self.elastic_p), 'piecewise': (self.piecewise_scale, self.piecewise_p),
                    'perspective': (self.perspective_scale, self.perspective_p)}[name]
        if scale is None or p is None or not rng.random() < p:
            return
        s = float(rng.uniform(*scale))
        if name == 'elastic':
            nbhd['elastic'] = s
        elif name == 'piecewise':
            nbhd['piecewise'] = rng.normal(0.0, s, (WARP_NODES, WARP_NODES, 2))
        else:
            f = np.minimum(np.abs(rng.normal(0.0, s, (4, 2))), PERSPECTIVE_CLIP)
            if quad_is_convex(f):                             # (several corners near the clip can fold the quad: nothing happens then)
                nbhd['perspective'] = f

    def _draw_blend(self, rng, name, nbhd):
        """one picked slot of the edge-detect blend or hue / saturation -> nbhd (one that is off draws nothing)"""
        if name == 'edge_blend' and self.edge_blend is not None:
            alpha = float(rng.uniform(*self.edge_blend))
            direction = None if rng.random() < 0.5 else float(rng.uniform(0.0, 1.0))     # EdgeDetect, DirectedEdgeDetect
            nbhd['edge'] = {'alpha': alpha, 'direction': direction}
            nbhd['edge_mask'] = value_noise_table(rng)
        elif name == 'hue_sat' and self.hue_sat is not None:
            nbhd['hue_sat'] = int(rng.integers(int(self.hue_sat[0]), int(self.hue_sat[1]) + 1))

    def _draw_colour(self, rng, nbhd=None):
        lo, hi = self.some_of
        n = int(rng.integers(lo, hi + 1)) if hi > 0 else 0
        picked = rng.permutation(COLOUR_SLOTS)[:n]            # slots 0..4 hold this module's five, in _COLOUR_OPS order
        ops = []
        for slot in picked:
            name = _COLOUR_OPS[slot] if slot < len(_COLOUR_OPS) else None
            if name == 'invert' and self.invert > 0.0:
                flags = rng.random(3) < self.invert
                if flags.any():
                    ops.append(('invert', flags))
            elif name == 'add' and self.add is not None:
                ops.append(('add', self._values(rng, self.add, integer=True)))
            elif name == 'multiply' and self.multiply is not None:
                if rng.random() < 0.5:                        # the other branch of the reference's OneOf: the frequency-noise blend
                    ops.append(('multiply', self._values(rng, self.multiply)))
                elif self.frequency_blend and nbhd is not None and self.contrast is not None:
                    ops.append(('blend', (rng.uniform(self.multiply[0], self.multiply[1], 3), float(rng.uniform(*self.contrast)))))
                    nbhd['colour_mask'] = frequency_noise_table(rng)
            elif name == 'contrast' and self.contrast is not None:
                ops.append(('contrast', self._values(rng, self.contrast)))
            elif name == 'grayscale' and self.grayscale is not None:
                ops.append(('grayscale', float(rng.uniform(*self.grayscale))))
            elif nbhd is not None and len(_COLOUR_OPS) <= slot < len(_COLOUR_OPS) + len(_NBHD_OPS):
                self._draw_nbhd(rng, _NBHD_OPS[slot - len(_COLOUR_OPS)], nbhd)
            elif nbhd is not None and 0 <= slot - len(_COLOUR_OPS) - len(_NBHD_OPS) < len(_WARP_OPS):
                self._draw_warp(rng, _WARP_OPS[slot - len(_COLOUR_OPS) - len(_NBHD_OPS)], nbhd)
            elif nbhd is not None and 0 <= slot - len(_COLOUR_OPS) - len(_NBHD_OPS) - len(_WARP_OPS) < len(_BLEND_OPS):
                self._draw_blend(rng, _BLEND_OPS[slot - len(_COLOUR_OPS) - len(_NBHD_OPS) - len(_WARP_OPS)], nbhd)
        if nbhd and ('noise' in nbhd or 'dropout' in nbhd or 'elastic' in nbhd):
            nbhd['seed'] = int(rng.integers(0, 2 ** 64, dtype=np.uint64))
        return ops

    def draw(self, B):
        """-> list of B recipes (dicts): fliplr, flipud, crop_pad (top, right, bottom, left) or None, affine (keyword
        arguments of affine_matrix) or None, order, cval, mode, colour [(name, value), ...]; and only where drawn: filters
        [(name, parameters of filter_kernel...), ...], noise (scale, per_channel), dropout {p, per_channel, size: the mask's
        fraction of the image or None}, elastic (alpha), piecewise ([4,4,2] node jitter as fractions of (W, H)), perspective
        ([4,2] inward corner moves as fractions), seed (with noise, dropout or elastic), median (the window k), edge {alpha,
        direction: turns or None for EdgeDetect} with edge_mask (T1, fp32 [16,16]), hue_sat (the integer v), and colour_mask
        (T2) next to a ('blend', (multiply[3], contrast)) entry of colour"""
        rng, out = self.rng, []
        for _ in range(B):
            r = {'fliplr': bool(rng.random() < self.fliplr), 'flipud': bool(rng.random() < self.flipud), 'crop_pad': None,
                 'affine': None}
            if self.crop_pad is not None and rng.random() < self.crop_pad_p:
                r['crop_pad'] = tuple(float(v) for v in rng.uniform(self.crop_pad[0], self.crop_pad[1], 4))
            order = 1 if r['crop_pad'] is not None else self.orders[0]
            if rng.random() < self.affine_p:
                one = (1.0, 1.0)
                r['affine'] = {
                    'scale': tuple(float(v) for v in rng.uniform(*(self.scale or one), 2)),
                    'translate': tuple(float(v) for v in rng.uniform(*(self.translate or (0.0, 0.0)), 2)),
                    'rotate': float(rng.uniform(*(self.rotate or (0.0, 0.0)))),
                    'shear': float(rng.uniform(*(self.shear or (0.0, 0.0))))}
                order = int(self.orders[int(rng.integers(len(self.orders)))])
            r['order'] = int(order)
            r['cval'] = float(rng.integers(int(self.cval[0]), int(self.cval[1]) + 1))
            r['mode'] = int(self.modes[int(rng.integers(len(self.modes)))])
            nbhd = {}
            r['colour'] = self._draw_colour(rng, nbhd)
            r.update(nbhd)
            out.append(r)
        return out

    @staticmethod
    def rows(recipes, H, W):
        """recipes -> the kernel's parameter table, numpy float32 (matrices and filters composed in fp64): [B, ROW], or
        [B, NBHD_ROW] when some recipe holds a filter, noise or dropout, or [B, WARP_ROW] when some recipe holds an elastic,
        piecewise or perspective warp, or [B, BLEND_ROW] when some recipe holds a median, an edge blend, a hue / saturation
        shift or a colour blend.  ValueError for a perspective whose inverse has no positive denominator on the grid, a median
        window or second filter outside its range, and a mask table that is not finite, 16 x 16 and in [0, 1]."""
        blend = any(r.get(k) is not None for r in recipes for k in _BLEND_KEYS)
        warp = blend or any(r.get(k) is not None for r in recipes for k in _WARP_OPS)
        wide = warp or any(r.get('filters') or r.get('noise') or r.get('dropout') for r in recipes)
        table = np.zeros((len(recipes), BLEND_ROW if blend else WARP_ROW if warp else NBHD_ROW if wide else ROW), dtype=np.float32)
        for i, r in enumerate(recipes):
            inv = np.linalg.inv(forward_matrix(r, H, W))
            if r.get('perspective') is not None:
                # den = h20 x + h21 y + h22 is linear: one sign at the four corners of the grid is one sign on all of it
                den = inv[2] @ np.array([[0.0, W - 1.0, 0.0, W - 1.0], [0.0, 0.0, H - 1.0, H - 1.0], [1.0, 1.0, 1.0, 1.0]])
                if not np.isfinite(inv).all() or not ((den > 0).all() or (den < 0).all()):
                    raise ValueError('perspective %s: the inverse homography has no positive denominator on the %d x %d grid'
                                     % (np.asarray(r['perspective']).tolist(), H, W))
                inv = inv / inv[2, 2]
            colour, colour2 = list(r.get('colour', ())), None
            if any(name == 'blend' for name, _ in colour):    # the two branches in the blend's place, the other ops on either side
                colour2 = colour_matrix([('contrast', np.full(3, v[1])) if name == 'blend' else (name, v) for name, v in colour])
                colour = [('multiply', v[0]) if name == 'blend' else (name, v) for name, v in colour]
            row = make_row(inv, colour_matrix(colour), r.get('cval', 0.0), r.get('order', 0), r.get('mode', 0))
            if wide:
                kernel = compose_filters([filter_kernel(*f) for f in r['filters']]) if r.get('filters') else None
                d = r.get('dropout')
                if d is not None:
                    mask = (0, 0) if d['size'] is None else (max(4, int(H * d['size'])), max(4, int(W * d['size'])))
                    d = (d['p'], d['per_channel']) + mask
                row = make_nbhd_row(row, kernel, r.get('noise'), d, r.get('seed', 0))
            if warp:
                grid = None if r.get('piecewise') is None else -np.asarray(r['piecewise'], dtype=np.float64) * (W, H)
                row = make_warp_row(row, inv[2] if r.get('perspective') is not None else None, r.get('elastic'), grid)
            if blend:
                kernel2 = None
                if r.get('edge') is not None:                 # G = E * F, composed in fp64 as F itself; E alone without a filter
                    kernel2 = compose_filters([filter_kernel(*f) for f in r.get('filters') or ()] + [edge_kernel(**r['edge'])])
                row = make_blend_row(row, r.get('median') or 0, kernel2, colour2, r.get('edge_mask'), r.get('colour_mask'),
                                     None if r.get('hue_sat') is None else hue_sat_shift(r['hue_sat']))
            table[i] = row
        return table

    def sample(self, B, H, W):
        """-> numpy float32 [B, ROW], [B, NBHD_ROW], [B, WARP_ROW] or [B, BLEND_ROW]: one parameter row per sample of a B x 3 x H x W batch"""
        return self.rows(self.draw(B), H, W)

    # ------------------------------------------------------------------ device side
    def apply(self, imgs, segs, params, out_hw=None, shapes=None):
        """explicit rows (numpy or tensor [B, ROW], [B, NBHD_ROW], [B, WARP_ROW] or [B, BLEND_ROW]) -> (fp32 [B,3,oh,ow], int64
        [B,H,W]); out_hw=None keeps (H, W).  Rows of NBHD_ROW floats go through pseg_augment_batch_nbhd, rows of WARP_ROW floats
        through pseg_augment_batch_warp, rows of BLEND_ROW floats through pseg_augment_batch_blend; when they already live on the device, shapes (row_shapes() of the table) has to come with
        them."""
        from .. import ops
        assert ROW == ops.AUGMENT_ROW and NBHD_ROW == ops.AUGMENT_NBHD_ROW and WARP_ROW == ops.AUGMENT_WARP_ROW
        assert BLEND_ROW == ops.AUGMENT_BLEND_ROW
        B, _, H, W = imgs.shape
        if not torch.is_tensor(params):
            params = torch.from_numpy(np.ascontiguousarray(params, dtype=np.float32))
        wide = params.shape[1] in (NBHD_ROW, WARP_ROW, BLEND_ROW)
        if wide and shapes is None:
            if params.is_cuda:
                raise ValueError('a device table of NBHD_ROW, WARP_ROW or BLEND_ROW floats needs shapes=row_shapes(table) from the host')
            shapes = row_shapes(params.numpy())
        if not params.is_cuda:
            # one pinned, non-blocking copy per batch (the pinned block stays alive until the copy ran: the caching
            # host allocator holds it back for the stream that used it)
            params = params.pin_memory().to(imgs.device, non_blocking=True)
        oh, ow = (H, W) if out_hw is None else (int(out_hw[0]), int(out_hw[1]))
        if wide:
            shapes = torch.as_tensor(shapes, dtype=torch.int32).contiguous()
            kernel = {WARP_ROW: ops.augment_batch_warp, BLEND_ROW: ops.augment_batch_blend}.get(params.shape[1], ops.augment_batch_nbhd)
            return kernel(imgs.contiguous(), segs.contiguous(), params.contiguous(), shapes, oh, ow, self.mean, self.std)
        return ops.augment_batch(imgs.contiguous(), segs.contiguous(), params.contiguous(), oh, ow, self.mean, self.std)

    def __call__(self, imgs_u8, segs_u8, out_hw=None):
        B, _, H, W = imgs_u8.shape
        return self.apply(imgs_u8, segs_u8, self.sample(B, H, W), out_hw)
