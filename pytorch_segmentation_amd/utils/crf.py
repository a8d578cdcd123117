"""Options of the local dense-CRF refinement (ops.crf_refine / csrc/crf.hip; definition in include/pseg_amd.h) and the one
call the inference and evaluation routes make with them.  Nothing here needs a GPU until ``refine`` is called.

The defaults are this module's own choice in the range DeepLab's dense-CRF settings are usually quoted in; they were not
tuned against trained weights.
"""
import math

RADIUS, DILATION, ITERS = (1, 5), (1, 4), (1, 10)      # inclusive ranges (pseg_crf_refine)


class CRF:
    """radius R, dilation D: the window is (2R+1) x (2R+1) taps D pixels apart; iters: mean-field iterations;
    theta = (theta_alpha, theta_beta, theta_gamma): the appearance kernel's spatial and colour (8-bit units) widths and the
    smoothness kernel's spatial width, in pixels of the model input; weights = (w_appearance, w_smooth) in logit units."""

    def __init__(self, radius=3, dilation=2, iters=5, theta=(8.0, 13.0, 3.0), weights=(4.0, 3.0)):
        for name, v, (lo, hi) in (('radius', radius, RADIUS), ('dilation', dilation, DILATION), ('iters', iters, ITERS)):
            if isinstance(v, bool) or int(v) != v or not lo <= int(v) <= hi:
                raise ValueError('crf %s must be an integer in [%d, %d]; got %r' % (name, lo, hi, v))
        theta, weights = tuple(float(t) for t in theta), tuple(float(x) for x in weights)
        if len(theta) != 3 or not all(math.isfinite(t) and t > 0 for t in theta):
            raise ValueError('crf theta takes three finite values > 0 (alpha, beta, gamma); got %r' % (theta,))
        if len(weights) != 2 or not all(math.isfinite(x) and x >= 0 for x in weights):
            raise ValueError('crf weights takes two finite values >= 0 (appearance, smoothness); got %r' % (weights,))
        self.radius, self.dilation, self.iters = int(radius), int(dilation), int(iters)
        self.theta, self.weights = theta, weights

    @classmethod
    def of(cls, crf):
        """inference() / test()'s ``crf=`` argument: True -> the defaults, a dict -> CRF(**dict), a CRF -> itself"""
        if crf is True:
            return cls()
        if isinstance(crf, cls):
            return crf
        if isinstance(crf, dict):
            return cls(**crf)
        raise TypeError('crf= takes None, True, a CRF or a dict of its options; got %r' % (crf,))

    def refine(self, logits, guide, guide_scale, out=None):
        """logits [B,C,h,w] and the model input [B,3,h,w] they came from (any float dtype; the refinement is fp32) -> the
        refined fp32 logits.  guide_scale: the std of the input's normalisation."""
        from .. import ops
        return ops.crf_refine(logits.float().contiguous(), guide.float().contiguous(), guide_scale, self.radius, self.dilation,
                              self.iters, *self.theta, *self.weights, out=out)

    def __repr__(self):
        return 'CRF(radius=%d, dilation=%d, iters=%d, theta=%r, weights=%r)' % (self.radius, self.dilation, self.iters,
                                                                                self.theta, self.weights)


def from_flags(crf, radius=None, dilation=None, iters=None, theta=None, weights=None):
    """The command-line flags --crf, --crf-radius, --crf-dilation, --crf-iters, --crf-theta, --crf-weights -> a CRF, or None
    without any of them; one of the last five without --crf is an error."""
    if not crf:
        if any(v is not None for v in (radius, dilation, iters, theta, weights)):
            raise ValueError('--crf-radius, --crf-dilation, --crf-iters, --crf-theta and --crf-weights need --crf')
        return None
    given = dict(radius=radius, dilation=dilation, iters=iters, theta=theta, weights=weights)
    return CRF(**{k: v for k, v in given.items() if v is not None})
