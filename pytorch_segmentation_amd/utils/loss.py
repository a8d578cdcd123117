"""compute_loss / masks / metrics on the HIP kernels (reference utils/utils.py:12-24,51-65, test.py:31-46)."""
import os

import torch

from .. import ops
from ..ops import Act


# PSEG_CHECK_LABELS=1: raise like torch on a target outside [0, C) (costs one host synchronisation per loss call).
# Without it such pixels are treated as ignored -- consistently in the divisor, the sum and the gradient -- and their
# number is available as element [2] of ops.ce_fwd_bwd's first result.
CHECK_LABELS = os.environ.get('PSEG_CHECK_LABELS', '0') == '1'


BAD_LABELS = '%d target values are outside [0, %d) and are not ignore_index'


class _FusedLossFn(torch.autograd.Function):
    """A loss whose forward and backward arithmetic happen in ONE call: run(want_grad) -> (out, dlogits | None) is one of
    the ops.*_fwd_bwd calls on `logits` (out[0] the loss, out[2] the number of out-of-range targets); everything that is
    not differentiated -- targets, weights, depth bytes, options -- reaches the kernel inside `run`.  backward only
    rescales the kept gradient by the incoming scalar (a device-side no-op when it is 1)."""

    @staticmethod
    def forward(ctx, logits, run, bad_labels):
        out, dl = run(logits.requires_grad)
        if CHECK_LABELS and out[2].item() != 0:     # (host sync: debugging aid, off by default)
            raise IndexError(bad_labels % (int(out[2].item()), logits.shape[1]))
        ctx.dl = dl
        return out[0]

    @staticmethod
    def backward(ctx, g):
        dl = ctx.dl
        ctx.dl = None
        if dl is not None:
            g = g.reshape(1) if g.dtype == torch.float32 else g.float().reshape(1)
            ops.scale_inplace(dl, g.contiguous())
        return dl, None, None


def _ce_term(logits, targets):
    """nn.CrossEntropyLoss() defaults (pseg_ce_fwd_bwd).  Like every term below: (contiguous fp32 logits at the targets'
    size, int64 targets on their device) -> the scalar."""
    return _FusedLossFn.apply(logits, lambda want_grad: ops.ce_fwd_bwd(logits, targets, want_grad=want_grad),
                              BAD_LABELS + ' (torch raises "Target ... is out of bounds" here)')


class _ResizeFn(torch.autograd.Function):
    """F.interpolate(outputs, size, mode='bilinear', align_corners=True) on NCHW logits
    (reference utils/utils.py:18-20; only taken when the sizes differ, i.e. --multi-scale)."""

    @staticmethod
    def forward(ctx, x, Ho, Wo):
        B, C, H, W = x.shape
        xa = Act.from_nchw(x)
        ctx.shape = (B, C, H, W, xa.C)
        return ops.bilinear_fwd_nchw(xa, C, Ho, Wo, True)

    @staticmethod
    def backward(ctx, g):
        B, C, H, W, Cp = ctx.shape
        dx = Act.empty(B, H, W, Cp, g.device, zero=True)
        ops.bilinear_bwd_nchw(g.contiguous(), dx, C, True)
        return dx.to_nchw(C), None, None


def compute_loss(outputs, targets, model=None):
    """Same signature and result as the reference's compute_loss(outputs, targets, model) (utils/utils.py:17-24)."""
    if not outputs.is_cuda:
        raise RuntimeError('compute_loss runs on the HIP path only (got %s)' % outputs.device)
    targets = targets.to(device=outputs.device, dtype=torch.int64).contiguous()
    th, tw = targets.size(1), targets.size(2)
    if (outputs.size(2), outputs.size(3)) != (th, tw):
        outputs = _ResizeFn.apply(outputs, th, tw)
    # equal sizes: bilinear align_corners=True is the exact identity, so nothing is launched
    return _ce_term(outputs.contiguous(), targets)


def _logits_at_target_size(outputs, targets):
    """What compute_loss does before the loss proper: int64 targets on the logits' device, logits resized to them."""
    if not outputs.is_cuda:
        raise RuntimeError('the loss runs on the HIP path only (got %s)' % outputs.device)
    targets = targets.to(device=outputs.device, dtype=torch.int64).contiguous()
    th, tw = targets.size(1), targets.size(2)
    if outputs.dtype != torch.float32:      # -mp hands fp16 logits to a custom loss: the kernels read fp32 NCHW
        outputs = outputs.float()
    if (outputs.size(2), outputs.size(3)) != (th, tw):
        outputs = _ResizeFn.apply(outputs, th, tw)
    return outputs.contiguous(), targets


def lovasz_softmax_loss(outputs, targets, ignore_index=-100):
    """Multi-class Lovasz-softmax loss of NCHW logits (classes='present', the whole batch as one image, as the reference's
    lovasz_softmax(probas, labels, ignore=...) describes it); the softmax is part of the kernel.  A direct surrogate of the
    mean IoU the trainer selects checkpoints by."""
    outputs, targets = _logits_at_target_size(outputs, targets)
    return _lovasz_term(ignore_index)(outputs, targets)


def _lovasz_term(ignore_index=-100):
    """The Lovasz-softmax term over the classes present in the batch (Berman et al.; the loss the reference names in
    utils/criterions.py): pseg_lovasz_softmax_fwd_bwd."""
    def term(logits, targets):
        return _FusedLossFn.apply(logits, lambda want_grad: ops.lovasz_softmax_fwd_bwd(
            logits, targets, want_grad=want_grad, ignore_index=ignore_index), BAD_LABELS)
    return term


def _class_weight_on(class_weight, device):
    """None, a sequence or a tensor -> None or a contiguous fp32 tensor on `device`."""
    if class_weight is None:
        return None
    return torch.as_tensor(class_weight, dtype=torch.float32).to(device).contiguous()


def _ce_opts_term(class_weight, label_smoothing, focal_gamma, keep_ratio, ignore_index=-100, boundary=None):
    """The cross-entropy term with class weights (None, a sequence or a tensor: moved to the logits' device once), label
    smoothing, the focal factor and hard-pixel selection (pseg_ce_opts_fwd_bwd; the kept set is held fixed in the
    gradient).  boundary = (boost, width in pixels or None, ratio, falloff, sigma or None): every pixel is also weighted
    by its ops.label_depth bin (pseg_ce_opts_binned_fwd_bwd)."""
    state = {'w': class_weight, 'device': None}
    ls, fg, kr = float(label_smoothing), float(focal_gamma), float(keep_ratio)

    def term(logits, targets):
        C = logits.shape[1]
        if state['w'] is not None and state['device'] != logits.device:
            state['w'], state['device'] = _class_weight_on(state['w'], logits.device), logits.device
        w = state['w']
        if w is not None and w.numel() != C:
            raise ValueError('class_weight has %d values for %d classes' % (w.numel(), C))
        if boundary is None:
            return _FusedLossFn.apply(logits, lambda want_grad: ops.ce_opts_fwd_bwd(
                logits, targets, w, ls, fg, kr, want_grad=want_grad, ignore_index=ignore_index), BAD_LABELS)
        boost, width, ratio, falloff, sigma = boundary
        d = int(width) if width else boundary_width(targets.shape[1:], ratio)
        table = _boundary_table_on(d, boost, falloff, sigma, logits.device)
        depth = ops.label_depth(targets, C, d, edge=False)
        return _FusedLossFn.apply(logits, lambda want_grad: ops.ce_opts_binned_fwd_bwd(
            logits, targets, depth, table, w, ls, fg, kr, want_grad=want_grad, ignore_index=ignore_index), BAD_LABELS)
    return term


def weighted_cross_entropy_loss(outputs, targets, class_weight=None, label_smoothing=0.0, focal_gamma=0.0, keep_ratio=1.0,
                                ignore_index=-100):
    """Cross-entropy of NCHW logits with per-class weights and label smoothing (F.cross_entropy(weight=, label_smoothing=)
    per pixel), times the focal factor (1 - p_t)^focal_gamma, averaged (weighted by the labels' class weights) over the
    keep_ratio hardest valid pixels of the batch -- all of them at keep_ratio = 1.  One HIP call (pseg_ce_opts_fwd_bwd);
    bit-reproducible."""
    outputs, targets = _logits_at_target_size(outputs, targets)
    return _ce_opts_term(class_weight, label_smoothing, focal_gamma, keep_ratio, ignore_index)(outputs, targets)


BOUNDARY_FALLOFFS = ('flat', 'linear', 'gaussian')


def boundary_weight_table(width, boost, falloff='gaussian', sigma=None):
    """The 256 pixel weights of the boundary-weighted cross-entropy, indexed by ops.label_depth's byte: fp32 [256] on the CPU.
    For a depth k in 1 .. width (k = 1: the pixel touches a different label) the weight is 1 + boost (falloff 'flat'),
    1 + boost (width + 1 - k) / width ('linear') or 1 + boost exp(-(k - 1)^2 / (2 sigma^2)) ('gaussian', sigma defaulting
    to width / 3: the UNet paper's w0 exp(-d^2 / 2 sigma^2) with the Chebyshev depth for d).  Depth width + 1 ("no contour
    within width") and the bytes the depth map cannot hold (0 and above width + 1) weigh 1."""
    import math
    if int(width) != width or not 1 <= int(width) <= ops.BOUNDARY_MAX_WIDTH:
        raise ValueError('boundary_weight_table: width must be an integer in [1, %d]; got %r' % (ops.BOUNDARY_MAX_WIDTH, width))
    width, boost = int(width), float(boost)
    if not (math.isfinite(boost) and boost >= 0.0):
        raise ValueError('boundary_weight_table: boost must be finite and >= 0; got %r' % (boost,))
    if falloff not in BOUNDARY_FALLOFFS:
        raise ValueError('boundary_weight_table: unknown falloff %r (choose from %s)' % (falloff, ', '.join(BOUNDARY_FALLOFFS)))
    if sigma is None:
        sigma = width / 3.0
    sigma = float(sigma)
    if not (math.isfinite(sigma) and sigma > 0.0):
        raise ValueError('boundary_weight_table: sigma must be finite and > 0; got %r' % (sigma,))
    table = torch.ones(256, dtype=torch.float64)
    k = torch.arange(1, width + 1, dtype=torch.float64)
    if falloff == 'flat':
        shape = torch.ones_like(k)
    elif falloff == 'linear':
        shape = (width + 1 - k) / width
    else:
        shape = torch.exp(-(k - 1) ** 2 / (2.0 * sigma * sigma))
    table[1:width + 1] = 1.0 + boost * shape
    return table.float()


_BOUNDARY_TABLES = {}      # (width, boost, falloff, sigma, device) -> the uploaded table


def _boundary_table_on(width, boost, falloff, sigma, device):
    key = (int(width), float(boost), falloff, None if sigma is None else float(sigma), str(device))
    if key not in _BOUNDARY_TABLES:
        _BOUNDARY_TABLES[key] = ops.bin_weight_table(boundary_weight_table(width, boost, falloff, sigma), device)
    return _BOUNDARY_TABLES[key]


def boundary_weighted_cross_entropy_loss(outputs, targets, boundary_boost, boundary_width=None, boundary_ratio=0.02,
                                         boundary_falloff='gaussian', boundary_sigma=None, class_weight=None,
                                         label_smoothing=0.0, focal_gamma=0.0, keep_ratio=1.0, ignore_index=-100):
    """weighted_cross_entropy_loss with every pixel weighted by its distance to the nearest label change of the target:
    u = boundary_weight_table(d, boundary_boost, boundary_falloff, boundary_sigma)[depth], depth = ops.label_depth(targets,
    C, d, edge=False), d = boundary_width or boundary_width(target size, boundary_ratio) -- the evaluation's rule, so the band
    follows multi-scale and --rect.  loss = sum_kept u f / sum_kept u w_t; with keep_ratio < 1 the hardest pixels are chosen
    by u f.  The image border is not a contour (edge=False).  Void labels compare by value in the depth map: a pixel beside
    an ignore band (VOC's 255 outline) counts as near a contour and is boosted, while the void pixels themselves stay out of
    the loss.  Two depth launches plus one HIP call (pseg_ce_opts_binned_fwd_bwd), which reads the depth byte beside the
    target; no fp32 weight map is written.  Bit-reproducible."""
    outputs, targets = _logits_at_target_size(outputs, targets)
    boundary = (boundary_boost, boundary_width, boundary_ratio, boundary_falloff, boundary_sigma)
    return _ce_opts_term(class_weight, label_smoothing, focal_gamma, keep_ratio, ignore_index, boundary)(outputs, targets)


def _tversky_term(alpha=0.5, beta=0.5, smooth=1.0, power=1.0, per_image=False, all_classes=False, ignore_index=-100, weight=1.0):
    """weight x the soft Dice / Tversky / focal-Tversky term over the softmax of the logits (Salehi et al.; Abraham & Khan):
    pseg_tversky_fwd_bwd.  A weight of 1 is no multiply."""
    args = (float(alpha), float(beta), float(smooth), float(power), bool(per_image), bool(all_classes))
    weight = float(weight)

    def term(logits, targets):
        loss = _FusedLossFn.apply(logits, lambda want_grad: ops.tversky_fwd_bwd(
            logits, targets, *args, want_grad=want_grad, ignore_index=ignore_index), BAD_LABELS)
        return loss if weight == 1.0 else weight * loss
    return term


def tversky_loss(outputs, targets, alpha=0.5, beta=0.5, smooth=1.0, power=1.0, per_image=False, all_classes=False,
                 ignore_index=-100):
    """Soft region-overlap loss of NCHW logits; the softmax is part of the kernel.  Per class, over the valid pixels of a
    group (the batch, or each image with per_image): TI = (TP + smooth) / (TP + alpha FP + beta FN + smooth) from the soft
    counts, term = (1 - TI)^power; the mean over the classes present in the group (all_classes: every class), then over the
    groups.  The defaults are soft Dice; alpha + beta = 1 is Tversky (beta > alpha weighs misses over false alarms);
    power != 1 is focal-Tversky.  One HIP call (pseg_tversky_fwd_bwd); bit-reproducible."""
    outputs, targets = _logits_at_target_size(outputs, targets)
    return _tversky_term(alpha, beta, smooth, power, per_image, all_classes, ignore_index)(outputs, targets)


def _surface_options(weight, clip):
    """the checked (weight: a float or a zero-argument callable, clip: a float) of a surface term"""
    import math
    if not callable(weight):
        weight = float(weight)
        if not (math.isfinite(weight) and weight >= 0.0):
            raise ValueError('surface_weight must be finite and >= 0 (or a zero-argument callable); got %r' % (weight,))
    clip = float(clip)
    if not (math.isfinite(clip) and clip >= 0.0):
        raise ValueError('surface_clip must be finite and >= 0 (pixels; 0: no limit); got %r' % (clip,))
    return weight, clip


def _surface_term(weight=1.0, clip=0.0, ignore_index=-100):
    """weight x Kervadec's surface term (Kervadec et al., MIDL 2019): the mean over the valid pixels of sum_c phi_c p_c, phi
    the signed Euclidean distance to the contour of class c in the target (ops.class_sdist, computed here from the targets)
    limited to [-clip, clip] when clip > 0: pseg_surface_fwd_bwd.  weight: a float, or a zero-argument callable that is
    read at every call (a schedule needs no rebuild).  A weight of 1 is no multiply."""
    weight, clip = _surface_options(weight, clip)

    def term(logits, targets):
        sdist = ops.class_sdist(targets, logits.shape[1])
        loss = _FusedLossFn.apply(logits, lambda want_grad: ops.surface_fwd_bwd(
            logits, targets, sdist, clip, want_grad=want_grad, ignore_index=ignore_index), BAD_LABELS)
        w = float(weight()) if callable(weight) else weight
        return loss if w == 1.0 else w * loss
    return term


def surface_loss(outputs, targets, clip=0.0, ignore_index=-100):
    """Kervadec's surface (boundary) loss of NCHW logits; the softmax is part of the kernel.  With phi_c the signed distance
    in pixels of a pixel to the contour of class c in the target -- positive outside the class, -(distance - 1) inside, 0 for
    a class that is absent from the image or fills it (Kervadec's one_hot2dist), limited to [-clip, clip] when clip > 0 --
    the loss is the mean over the valid pixels of sum_c phi_c p_c, over ALL classes (Kervadec's code averages over the
    selected classes too, usually the foreground only: a constant factor the weight absorbs).  The distance map is an exact
    Euclidean transform on the device (three launches and a memset), the loss one HIP call (pseg_surface_fwd_bwd);
    bit-reproducible.  Unbounded below in practice: a companion of a region loss (make_loss's '...+surface'), not an
    objective of its own."""
    outputs, targets = _logits_at_target_size(outputs, targets)
    return _surface_term(1.0, clip, ignore_index)(outputs, targets)


def signed_distance(targets, num_classes, clip=0.0):
    """phi of surface_loss as fp32 [B, num_classes, H, W] on the targets' device, from ops.class_sdist with torch ops (for
    inspection and logging; the loss reads the integer map itself)."""
    if not targets.is_cuda:
        raise RuntimeError('signed_distance runs on the HIP path only (got %s)' % targets.device)
    _, clip = _surface_options(1.0, clip)
    sd = ops.class_sdist(targets.to(torch.int64).contiguous(), num_classes).float()
    phi = torch.where(sd > 0, sd.abs().sqrt(), torch.where(sd < 0, 1.0 - sd.abs().sqrt(), torch.zeros_like(sd)))
    return phi.clamp_(-clip, clip) if clip > 0 else phi


# the one table behind every named loss: name -> its kinds of term, in the order they are added
TERMS = {'ce': ('ce',), 'lovasz': ('lovasz',), 'ce+lovasz': ('ce', 'lovasz'), 'tversky': ('tversky',),
         'ce+tversky': ('ce', 'tversky'), 'ce+surface': ('ce', 'surface'), 'tversky+surface': ('tversky', 'surface'),
         'ce+tversky+surface': ('ce', 'tversky', 'surface')}


def _compose(name, term_of, launch_last_first=False):
    """loss_fn(outputs, targets, model) of the loss `name`: the logits brought to the targets' size once, then the sum of
    TERMS[name] in table order, term_of[kind] giving each.  launch_last_first: the terms' kernels are launched in reverse
    (only the order on the stream: the sum is the same expression)."""
    terms = [term_of[kind] for kind in TERMS[name]]

    def loss_fn(outputs, targets, model=None):
        outputs, targets = _logits_at_target_size(outputs, targets)
        order = reversed(range(len(terms))) if launch_last_first else range(len(terms))
        values = {i: terms[i](outputs, targets) for i in order}
        loss = values[0]
        for i in range(1, len(terms)):
            loss = loss + values[i]
        return loss
    return loss_fn


# surface_weight: Kervadec's starting alpha (a term measured in pixels must not swamp a term of order 1); a float or a
# zero-argument callable.  surface_clip 0: the distance is not limited.
SURFACE_OPTIONS = {'surface_weight': 0.01, 'surface_clip': 0.0}
_DEFAULT_TERMS = {'ce': _ce_term, 'lovasz': _lovasz_term(), 'tversky': _tversky_term(),
                  'surface': _surface_term(SURFACE_OPTIONS['surface_weight'], SURFACE_OPTIONS['surface_clip'])}
LOSSES ={name: compute_loss if name == 'ce' else _compose(name, _DEFAULT_TERMS) for name in TERMS}
_lovasz_loss_fn, _ce_lovasz_loss_fn = LOSSES['lovasz'], LOSSES['ce+lovasz']
CE_OPTIONS = {'class_weight': None, 'label_smoothing': 0.0, 'focal_gamma': 0.0, 'keep_ratio': 1.0}
TVERSKY_OPTIONS = {'tversky_alpha': 0.5, 'tversky_beta': 0.5, 'tversky_smooth': 1.0, 'tversky_power': 1.0,
                   'tversky_per_image': False, 'tversky_all_classes': False, 'tversky_weight': 1.0}
# boundary_width 0: from boundary_ratio; boundary_sigma 0: width / 3.  On iff boundary_boost > 0.
BOUNDARY_OPTIONS = {'boundary_boost': 0.0, 'boundary_width': 0, 'boundary_ratio': 0.02, 'boundary_falloff': 'gaussian',
                    'boundary_sigma': 0.0}


def make_loss(name, **options):
    """'ce' | 'lovasz' | 'ce+lovasz' | 'tversky' | 'ce+tversky' | 'ce+surface' | 'tversky+surface' | 'ce+tversky+surface' ->
    loss_fn(outputs, targets, model) for Trainer(loss_fn=...).
    'ce' without options is compute_loss itself (the Trainer's fused fast path keys on that object); everything else goes
    through the Trainer's autograd route.  The cross-entropy options (class_weight=, label_smoothing=, focal_gamma=,
    keep_ratio=) configure the cross-entropy of 'ce', 'ce+lovasz' and 'ce+tversky' (weighted_cross_entropy_loss); the
    Tversky options (tversky_alpha=, tversky_beta=, tversky_smooth=, tversky_power=, tversky_per_image=,
    tversky_all_classes=, and tversky_weight= for ce + weight * tversky) configure the Tversky term of 'tversky' and
    'ce+tversky' (tversky_loss); the boundary options (boundary_boost= > 0 turns them on; boundary_width= in pixels or
    boundary_ratio= of the diagonal, boundary_falloff=, boundary_sigma=) weight that same cross-entropy term by the distance
    to the target's contours (boundary_weighted_cross_entropy_loss) and compose with the cross-entropy options; the surface
    options (surface_weight=, a float or a zero-argument callable read at every call, and surface_clip= in pixels)
    configure the surface term that the '...+surface' names add last (surface_loss; there is no bare 'surface': the term
    alone is unbounded below).  Every kind of option applies wherever TERMS[name] has its kind of term: the cross-entropy and
    boundary options need a 'ce', the Tversky options a 'tversky', the surface options a 'surface'.  An option left at its
    default is not an option."""
    if name not in LOSSES:
        raise ValueError('unknown loss %r (choose from %s)' % (name, ', '.join(sorted(LOSSES))))
    unknown = sorted(set(options) - set(CE_OPTIONS) - set(TVERSKY_OPTIONS) - set(BOUNDARY_OPTIONS) - set(SURFACE_OPTIONS))
    if unknown:
        raise TypeError('unknown cross-entropy option(s) %s (choose from %s; Tversky options: %s; boundary options: %s; '
                        'surface options: %s)'
                        % (', '.join(unknown), ', '.join(sorted(CE_OPTIONS)), ', '.join(sorted(TVERSKY_OPTIONS)),
                           ', '.join(sorted(BOUNDARY_OPTIONS)), ', '.join(sorted(SURFACE_OPTIONS))))
    kinds = TERMS[name]
    opts = dict(CE_OPTIONS, **{k: v for k, v in options.items() if k in CE_OPTIONS})
    tv = dict(TVERSKY_OPTIONS, **{k: v for k, v in options.items() if k in TVERSKY_OPTIONS})
    bd = dict(BOUNDARY_OPTIONS, **{k: v for k, v in options.items() if k in BOUNDARY_OPTIONS and v is not None})
    sf = dict(SURFACE_OPTIONS, **{k: v for k, v in options.items() if k in SURFACE_OPTIONS and v is not None})
    is_set = opts['class_weight'] is not None or any(float(opts[k]) != CE_OPTIONS[k] for k in
                                                      ('label_smoothing', 'focal_gamma', 'keep_ratio'))
    tv_set = any(float(tv[k]) != float(TVERSKY_OPTIONS[k]) for k in TVERSKY_OPTIONS)
    sf_set = callable(sf['surface_weight']) or any(float(sf[k]) != SURFACE_OPTIONS[k] for k in SURFACE_OPTIONS)
    bd_changed = sorted(k for k in BOUNDARY_OPTIONS if bd[k] != BOUNDARY_OPTIONS[k])
    bd_set = float(bd['boundary_boost']) > 0.0
    if float(bd['boundary_boost']) < 0.0:
        raise ValueError('boundary_boost must be >= 0; got %r' % (bd['boundary_boost'],))
    if bd_changed and not bd_set:
        raise ValueError('the boundary options (%s) need boundary_boost > 0' % ', '.join(bd_changed))
    if bd_set and 'boundary_width' in bd_changed and 'boundary_ratio' in bd_changed:
        raise ValueError('the boundary options boundary_width and boundary_ratio exclude each other')
    if tv_set and 'tversky' not in kinds:
        raise ValueError("the Tversky options do not apply to %r (use 'tversky' or 'ce+tversky')" % name)
    if sf_set and 'surface' not in kinds:
        raise ValueError("the surface options do not apply to %r (use 'ce+surface', 'tversky+surface' or 'ce+tversky+surface')"
                         % name)
    if not is_set and not tv_set and not bd_set and not sf_set:
        return LOSSES[name]
    if is_set and 'ce' not in kinds:
        raise ValueError("the cross-entropy options do not apply to %r (use 'ce', 'ce+lovasz' or 'ce+tversky')" % name)
    if bd_set and 'ce' not in kinds:
        raise ValueError("the boundary options do not apply to %r: they weight a cross-entropy term, and 'lovasz' and 'tversky' "
                         "have none (use 'ce', 'ce+lovasz' or 'ce+tversky')" % name)
    term_of = dict(_DEFAULT_TERMS)
    if 'tversky' in kinds:
        term_of['tversky'] = _tversky_term(**{k[len('tversky_'):]: v for k, v in tv.items()})
    if sf_set:
        term_of['surface'] = _surface_term(sf['surface_weight'], sf['surface_clip'])
    if is_set or bd_set:
        boundary = None
        if bd_set:
            boundary = (float(bd['boundary_boost']), int(bd['boundary_width']) or None, float(bd['boundary_ratio']),
                        bd['boundary_falloff'], float(bd['boundary_sigma']) or None)
            # bad options are refused here, not at the first batch
            boundary_weight_table(boundary[1] or 1, boundary[0], boundary[3], boundary[4])
        term_of['ce'] = _ce_opts_term(opts['class_weight'], opts['label_smoothing'], opts['focal_gamma'], opts['keep_ratio'],
                                      boundary=boundary)
    # (a configured 'ce+tversky' has always launched its Tversky kernels before its cross-entropy's)
    return _compose(name, term_of, launch_last_first=name == 'ce+tversky')


def predict_mask(outputs):
    """``outputs.max(1)[1]`` (reference test.py:31): int64 [B,H,W], first index on ties."""
    return ops.argmax(outputs.contiguous())


@torch.no_grad()
def predict_mask_ensemble(model, inputs, out_hw, scales=(1.0,), flip=False, view_logits=None, refine=None):
    """Test-time-ensembled prediction for an already normalised device batch [B,3,H,W]: int64 [B,out_h,out_w] =
    argmax_c of the unweighted sum, over the views, of the un-mirrored softmax resized bilinearly (align_corners=False) to
    out_hw; first index on ties.  Views: ``inputs`` resized (F.interpolate bilinear, align_corners=False; the identity at
    its own size) to every size of ``tta_sizes(H, W, scales)``, each also flipped along x with ``flip``.  The softmaxes
    and the resize-sum-argmax are ops.softmax_views / ops.seg_decode_ensemble.  view_logits (optional): a dict that
    receives {(h_s, w_s): that scale's logits}.  refine (optional): a call (logits, view) -> logits applied to every view's
    logits before its softmax (utils/crf.py); view_logits keeps the logits as the model gave them."""
    import torch.nn.functional as F
    from .inference import Ensemble, tta_sizes
    if not inputs.is_cuda:
        raise RuntimeError('predict_mask_ensemble runs on the HIP path only (got %s)' % inputs.device)
    B, _, H, W = inputs.shape
    oh, ow = int(out_hw[0]), int(out_hw[1])
    sizes = tta_sizes(H, W, scales)
    if B * (2 if flip else 1) > 65535:
        raise ValueError('%d images x %d views exceed 65535 rows per launch' % (B, 2 if flip else 1))
    ens = Ensemble(B, sizes, flip)
    for hs, ws in sizes:
        x = inputs if (hs, ws) == (H, W) else F.interpolate(inputs, (hs, ws), mode='bilinear', align_corners=False)
        if flip:
            x = torch.cat([x, torch.flip(x, [3])], 0)
        logits = model(x.contiguous()).float()
        if view_logits is not None:
            view_logits[(hs, ws)] = logits
        if refine is not None:
            logits = refine(logits, x)
        ens.add(logits)
        del logits, x
    table = torch.tensor([[b * oh * ow, oh, ow] for b in range(B)], dtype=torch.int64).to(inputs.device)
    mask, _ = ens.decode(table, B * oh * ow, (oh, ow))
    return mask.view(B, oh, ow).long()


@torch.no_grad()
def predict_mask_windows(model, inputs, out_hw, window_hw, stride_hw=None, scales=(1.0,), flip=False, refine=None):
    """Sliding-window prediction for an already normalised device batch [B,3,H,W]: int64 [B,out_h,out_w] = argmax_c of the
    sum, over the scales, of the bilinearly resized (align_corners=False) working probability -- the unweighted mean of the
    softmaxes (with ``flip``: plus the un-mirrored softmax of the mirrored window) of the windows covering a pixel of the
    working image; first index on ties.  The working image at scale s is ``inputs`` resized (F.interpolate bilinear,
    align_corners=False; the identity at 1.0) to ``work_size(H, W, s)``; the windows of ``window_hw`` = (h, w) at
    ``stride_hw`` = (sy, sx) (default: 2/3 of the window, ``window_grid``) are slices of it, zero-padded where it is
    smaller than the window; one forward per scale and image.  The softmaxes and the decode are ops.softmax_views /
    ops.seg_decode_windows.  refine (optional): a call (logits, windows) -> logits applied to every forward's logits before
    their softmax (utils/crf.py)."""
    import torch.nn.functional as F
    from .inference import slide_scales, slide_strides, window_grid
    if not inputs.is_cuda:
        raise RuntimeError('predict_mask_windows runs on the HIP path only (got %s)' % inputs.device)
    B, _, H, W = inputs.shape
    oh, ow = int(out_hw[0]), int(out_hw[1])
    h, w = int(window_hw[0]), int(window_hw[1])
    sy, sx = slide_strides(h, w, None if stride_hw is None else (stride_hw[1], stride_hw[0]))
    work = slide_scales([(H, W)] * B, scales)
    grids = [window_grid(sizes[0][0], sizes[0][1], h, w, sy, sx)[0] for sizes in work]
    if max(len(g) for g in grids) * (2 if flip else 1) > 65535:
        raise ValueError('more than 65535 window rows per forward')
    prob, CP, done, groups = None, None, 0, []
    for sizes, grid in zip(work, grids):
        Hs, Ws = sizes[0]
        x = inputs if (Hs, Ws) == (H, W) else F.interpolate(inputs, (Hs, Ws), mode='bilinear', align_corners=False)
        if Hs < h or Ws < w:
            x = F.pad(x, (0, max(w - Ws, 0), 0, max(h - Hs, 0)))
        for b in range(B):
            wins = torch.stack([x[b, :, y0:y0 + h, x0:x0 + w] for y0, x0 in grid])
            if flip:
                wins = torch.cat([wins, torch.flip(wins, [3])], 0)
            wins = wins.contiguous()
            logits = model(wins).float()
            if refine is not None:
                logits = refine(logits, wins)
            if prob is None:
                CP = ops.class_pad(logits.shape[1])
                prob = torch.empty(sum(len(g) for g in grids) * B * h * w * CP, dtype=torch.float32, device=inputs.device)
            groups.append([done * h * w * CP, Hs, Ws])
            ops.softmax_views(logits.contiguous(), prob, done * h * w * CP, flip)
            done += len(grid)
            C = logits.shape[1]
            del logits, wins
    dgroups = torch.tensor(groups, dtype=torch.int64).view(len(work), B, 3).to(inputs.device)
    table = torch.tensor([[b * oh * ow, oh, ow] for b in range(B)], dtype=torch.int64).to(inputs.device)
    mask, _ = ops.seg_decode_windows(prob, dgroups, B, C, (h, w), (sy, sx), table, B * oh * ow, (oh, ow))
    return mask.view(B, oh, ow).long()


def update_class_counts(counters, predicted, targets):
    """Accumulate per-class tp / fn / fp (reference test.py:34-46) into the int64 device tensor counters[3][C]
    with one kernel instead of 3*C host synchronisations."""
    ops.confusion(predicted.contiguous().view(-1), targets.to(torch.int64).contiguous().view(-1), counters)
    return counters


def _guarded(den):
    """a denominator with every entry <= 0 replaced by 1"""
    den = den.clone()
    den[den <= 0] = 1
    return den


def compute_metrics(tp, fn, fp):
    """reference utils/utils.py:51-65 -- host-side, [num_classes]-sized tensors (not on the hot path)."""
    tp, fn, fp = tp.clone().float(), fn.clone().float(), fp.clone().float()

    miou = tp / _guarded(tp + fp + fn)
    T = tp + fn
    P = tp / _guarded(tp + fp)
    R = tp / _guarded(tp + fn)
    F1 = 2 * tp / _guarded(2 * tp + fp + fn)
    return T, P, R, miou, F1


def boundary_width(hw, ratio=0.02):
    """Width in pixels of the contour band of an (H, W) label map: max(1, int(ratio * sqrt(H^2 + W^2) + 0.5)), the image
    diagonal times `ratio` rounded half up (0.02 is the Boundary IoU paper's value)."""
    h, w = int(hw[0]), int(hw[1])
    if h < 1 or w < 1:
        raise ValueError('boundary_width: size %r' % (tuple(hw),))
    if not 0.0 < float(ratio) <= 0.5:
        raise ValueError('boundary_width: ratio must be in (0, 0.5]; got %r' % (ratio,))
    d = max(1, int(float(ratio) * (h * h + w * w) ** 0.5 + 0.5))
    if d > ops.BOUNDARY_MAX_WIDTH:
        raise ValueError('boundary width %d of a %d x %d map at ratio %g exceeds %d pixels: give a smaller ratio or a fixed '
                         'width' % (d, h, w, ratio, ops.BOUNDARY_MAX_WIDTH))
    return d


def update_boundary_counts(counters, predicted, targets, width):
    """Accumulate the Boundary IoU and trimap counts of a batch into the int64 device tensor counters[6][C] (rows: inter,
    gband, pband, trimap tp / fn / fp; include/pseg_amd.h) with two launches, whatever the class count.  predicted,
    targets: [B, H, W]; width: the band's width in pixels (boundary_width)."""
    width = int(width)
    if not 1 <= width <= ops.BOUNDARY_MAX_WIDTH:
        raise ValueError('boundary width must be in [1, %d]; got %d' % (ops.BOUNDARY_MAX_WIDTH, width))
    ops.boundary_counts(predicted.to(torch.int64).contiguous(), targets.to(device=predicted.device, dtype=torch.int64).contiguous(),
                        counters, width)
    return counters


def compute_boundary_metrics(counters):
    """counters[6][C] -> (Boundary IoU [C], trimap IoU [C]) as fp32 host tensors; a denominator <= 0 is replaced by 1, as in
    compute_metrics."""
    inter, gband, pband, tp, fn, fp = (c.float() for c in counters.detach().cpu())

    return inter / _guarded(gband + pband - inter), tp / _guarded(tp + fn + fp)


SURFACE_ROWS = 7             # images defined, sum of HD, of HD95, of ASSD, images with an NSD, sum of NSD, misses


def update_surface_stats(acc, predicted, targets, permille=950, tol=2):
    """Accumulate the surface-distance metrics of a batch into the float64 device tensor acc[7][C] (rows: images where the
    class has a border in both maps, the sums of their HD, HD95 and ASSD, images where it has one in either map, the sum of
    their NSD, and the misses: images where it has one in exactly one map).  predicted, targets: [B, H, W]; permille: the
    quantile of HD95 in thousandths; tol: the NSD tolerance in pixels.  One call of ops.hausdorff_stats and torch ops on its
    [B, C] records: no host synchronisation."""
    assert acc.dtype == torch.float64 and acc.dim() == 2 and acc.shape[0] == SURFACE_ROWS, \
        'update_surface_stats: the accumulator is float64 [7][C]'
    stats, sums = ops.hausdorff_stats(predicted.to(torch.int64).contiguous(),
                                      targets.to(device=predicted.device, dtype=torch.int64).contiguous(), acc.shape[1],
                                      permille, tol)
    s = stats.double()
    n_p, n_g = s[..., 0], s[..., 1]
    defined = (n_p > 0) & (n_g > 0)
    has_nsd = (n_p + n_g) > 0
    one, zero = torch.ones_like(n_p), torch.zeros_like(n_p)
    hd = torch.where(defined, torch.maximum(s[..., 2], s[..., 3]).clamp(min=0).sqrt(), zero)
    hd95 = torch.where(defined, torch.maximum(s[..., 4], s[..., 5]).clamp(min=0).sqrt(), zero)
    assd = torch.where(defined, (sums[..., 0] / torch.where(defined, n_p, one) + sums[..., 1] / torch.where(defined, n_g, one)) / 2,
                       zero)
    nsd = torch.where(has_nsd, (s[..., 6] + s[..., 7]) / torch.where(has_nsd, n_p + n_g, one), zero)
    acc += torch.stack([defined.double().sum(0), hd.sum(0), hd95.sum(0), assd.sum(0), has_nsd.double().sum(0), nsd.sum(0),
                        (has_nsd & ~defined).double().sum(0)])
    return acc


def compute_surface_metrics(acc):
    """acc[7][C] -> (hd, hd95, assd, nsd, misses) as float64 [C] host tensors: every class's mean over the images that define
    the value (an image where only one map has the class is a miss: it enters nsd as 0 and none of the distances), NaN where
    no image does; misses is the count."""
    acc = acc.detach().cpu().double()
    nan = torch.full_like(acc[0], float('nan'))
    hd, hd95, assd = (torch.where(acc[0] > 0, acc[i] / acc[0].clamp(min=1), nan) for i in (1, 2, 3))
    nsd = torch.where(acc[4] > 0, acc[5] / acc[4].clamp(min=1), nan)
    return hd, hd95, assd, nsd, acc[6].clone()
