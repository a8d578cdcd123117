"""Tensor-level wrappers over the C-ABI (include/pseg_amd.h).

PyTorch is plumbing here: it owns device memory (caching allocator) and the HIP stream.  Every function
enqueues on ``torch.cuda.current_stream()`` and never synchronises the host.  Activations travel as
:class:`Act` handles -- fp32 NHWC with an explicit pixel stride, so a channel slice of a concat buffer is
just another handle over the same storage (the reference's ``torch.cat`` calls, models/aspp.py:36,
models/deeplabv3plus.py:38, models/unet.py:34-46, cost no copy).
"""
import os

import torch

from . import _lib

ACT_NONE, ACT_RELU, ACT_RELU6 = 0, 1, 2
PREC_FP32, PREC_BF16X3, PREC_BF16X6, PREC_FP16X3 = 0, 1, 2, 3
_PREC_NAMES = {'fp32': PREC_FP32, 'bf16x3': PREC_BF16X3, 'bf16x6': PREC_BF16X6, 'fp16x3': PREC_FP16X3}
# Conv arithmetic policy (forward convs, backward convs) used when a call does not name a precision.
#   fp32   : exact fp32 MFMA everywhere (bit-tight against the CPU oracle; the reference's own arithmetic)
#   mixed  : forward exact fp32, backward (dgrad + wgrad) split-bf16 three-product (op-level error <= 2e-4)
#   bf16x3 / bf16x6 : everything on bf16 limbs (three / six partial products)
_POLICIES = {'fp32': (PREC_FP32, PREC_FP32), 'mixed': (PREC_FP32, PREC_BF16X3),
             'bf16x3': (PREC_BF16X3, PREC_BF16X3), 'bf16x6': (PREC_BF16X6, PREC_BF16X6),
             # forward on fp16 limbs of the amax-scaled operands (~2^-22 per product), backward on bf16 limbs
             'limb': (PREC_FP16X3, PREC_BF16X3),
             # half-precision storage (`train.py -mp`): fp16 activations / gradients / filter copies, one fp16 MFMA pass with
             # fp32 accumulation, fp32 master weights and dynamic loss scaling (the precisions named here are unused: the
             # fp16 kernels have one arithmetic)
             'half': (PREC_FP32, PREC_FP32)}
# Default: 'fp32' -- the reference's arithmetic for every conv (drop-in fidelity first).  The faster reduced-product
# policies are opt-in: PSEG_PRECISION=mixed|limb, ops.set_conv_precision(...), Env(policy=...); train.py -mp selects 'half' (PSEG_MP_POLICY=limb: the fp32-storage limb policy instead).
POLICY_NAME = os.environ.get('PSEG_PRECISION', 'fp32')
FWD_PRECISION, BWD_PRECISION = _POLICIES[POLICY_NAME]


def set_conv_precision(name):
    """Select the conv arithmetic policy: 'fp32' | 'mixed' | 'bf16x3' | 'bf16x6' (see the table above)."""
    global FWD_PRECISION, BWD_PRECISION, POLICY_NAME
    FWD_PRECISION, BWD_PRECISION = _POLICIES[name]
    POLICY_NAME = name


def _prec(precision, backward=False):
    if precision is None:
        return BWD_PRECISION if backward else FWD_PRECISION
    return precision


def _round4(n):
    return (n + 3) // 4 * 4


def _round8(n):
    return (n + 7) // 8 * 8


def _stream():
    # raw handle of the current stream of the current device (0.2 us; torch.cuda.current_stream() builds a Python
    # Stream object every time, ~2 us, and this runs once per launch)
    return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())


# ---------------------------------------------------------------------------------------------- auxiliary stream
# Weight gradients have no consumer inside backward (only the optimiser / the gradient all-reduce read them), while the
# chain  BN-backward -> dgrad -> BN-backward ...  is strictly serial.  The weight-gradient kernels are bound by VALU +
# matrix work, the BatchNorm passes by HBM, the data gradients by LDS: enqueued on a second HIP stream they fill the
# same CUs side by side.  `fork_aux` orders the auxiliary stream after everything enqueued so far on the current one;
# `join_aux` makes the current stream wait for it (end of backward).
OVERLAP_WGRAD = os.environ.get('PSEG_OVERLAP_WGRAD', '1') == '1'
# limb policies: BatchNorm backward writes dy of wide 3x3 convs as bf16 limb planes too, their data gradient runs on the
# pre-split LDS-DMA kernel (nn.Conv2d.wants_dy_planes)
DY_PLANES = os.environ.get('PSEG_DY_PLANES', '1') == '1'
# residual BatchNorm layers keep their activation mask as a bitmask for backward (bn_act_fwd(want_mask=True))
BN_MASK = os.environ.get('PSEG_BN_MASK', '1') == '1'
# enqueue a conv's weight gradient after its data gradient (see nn.Conv2d.bwd)
WGRAD_AFTER_DGRAD = os.environ.get('PSEG_WGRAD_AFTER_DGRAD', '0') == '1'
_aux_streams = {}
_aux_dirty = {}


_aux_events = {}


_cur_stream_cache = {}


def _current_stream_obj(device):
    """torch.cuda.current_stream(device), memoised on the raw handle (building the Stream object costs ~3 us, and the
    backward pass asks for it once per conv)."""
    raw = _stream()
    hit = _cur_stream_cache.get(raw)
    if hit is None:
        hit = _cur_stream_cache[raw] = torch.cuda.current_stream(device)
        if len(_cur_stream_cache) > 64:
            _cur_stream_cache.clear()
    return hit


_own_stream_handles = {}       # device index -> torch stream ids of every stream this package has taken from torch's pool
OWN_STREAMS = os.environ.get('PSEG_OWN_STREAMS', '1') == '1'      # 0: torch.cuda.Stream() as it comes, torch's default capture stream


def new_stream(device):
    """A torch stream whose HIP handle differs from every stream this package already holds on the device.  torch hands out
    its 32 pool streams per device ROUND-ROBIN: in a process that has created many (a long test session; a service that builds
    Trainers over and over) a fresh ``torch.cuda.Stream()`` can BE the weight-gradient stream, the exchange stream or the
    capture stream -- a 'forked' launch then runs in line, silently (round 6: a lane-executor test saw a forked graph with one
    lane after the suite grew by two files)."""
    device = torch.device(device)
    if not OWN_STREAMS:
        return torch.cuda.Stream(device=device)
    idx = device.index if device.index is not None else torch.cuda.current_device()
    held = _own_stream_handles.setdefault(idx, set())
    s = None
    # (identity = torch's stream id, NOT the HIP handle: torch creates a pool stream's HIP stream on first access to the handle,
    # and the order in which a process's HIP streams come into being decides which hardware queue each lands on -- reading
    # `.cuda_stream` here materialised the never-used exchange stream of a one-rank Trainer ahead of the lane pool and cost the
    # replayed HRNet step 8 %: 7.19 -> 7.79 ms -mp, profiles/r06_ab_streams.txt)
    for _ in range(64):
        s = torch.cuda.Stream(device=device)
        if s.stream_id not in held:
            break
    held.add(s.stream_id)
    return s


_role_streams = {}


def role_stream(role, device=None):
    """One stream per (device, role) for the whole process, distinct from the package's other streams (new_stream): 'exchange' =
    the gradient reducer's side stream -- shared by every Trainer of the device: sharing only adds ordering, and a stream per
    Trainer would walk through torch's 32-stream pool."""
    idx = torch.cuda.current_device() if device is None or torch.device(device).index is None else torch.device(device).index
    st = _role_streams.get((idx, role))
    if st is None:
        st = _role_streams[(idx, role)] = new_stream(torch.device('cuda', idx))
    return st


def _make_aux_stream(device):
    """The auxiliary (weight-gradient) stream.  (A CU-masked stream that kept N CUs free for the main chain was measured in
    round 3 -- 44.6 -> 54.7-65.9 ms -- and is gone: profiles/EXPERIMENTS.md section 1.)"""
    return new_stream(device)


# PSEG_AUX_STREAMS: how many auxiliary streams the forked work (weight gradients) is dealt onto, round-robin.  The large
# configurations fill the chip with every weight-gradient launch and want ONE (a second would only interleave them); the
# narrow layers of the launch-bound ones (HRNet's 32 / 64-channel branches in fp32) leave it half empty, and there the
# auxiliary lane -- not the backward chain -- ends the step: two lanes overlap them.
AUX_STREAMS = max(1, min(3, int(os.environ.get('PSEG_AUX_STREAMS', '1'))))
# ... and while a step is being CAPTURED, as many as the model asks for (`capture_wgrad_lanes`, set by the Trainer around the
# capture; PSEG_AUX_STREAMS_CAPTURE forces a number).  The weight gradients are independent of one another -- only the ONE
# stream they share makes a chain of them -- and in a replayed HRNet step that chain (103 weight gradients + 104 slab
# reductions: 4.2 ms) was the longest lane of backward by a millisecond: two lanes, HRNet -mp 8.0 -> 7.5 ms, fp32 15.2 -> 14.7.
# UNet and DeepLabV3+ lose with two (3.36 -> 3.61, 14.14 -> 14.31 ms: their backward chain is the longest lane, and a second
# weight-gradient lane only takes CUs from it): they keep one.
_AUX_CAPTURE_FORCED = os.environ.get('PSEG_AUX_STREAMS_CAPTURE')
AUX_STREAMS_CAPTURE = max(1, min(3, int(_AUX_CAPTURE_FORCED))) if _AUX_CAPTURE_FORCED else 1
AUX_STREAMS_MAX = max(AUX_STREAMS, AUX_STREAMS_CAPTURE, 2)


def set_capture_wgrad_lanes(n):
    """-> the previous value.  Called by the Trainer around a capture with the model's `capture_wgrad_lanes` (default 1)."""
    global AUX_STREAMS_CAPTURE
    prev = AUX_STREAMS_CAPTURE
    if not _AUX_CAPTURE_FORCED:
        AUX_STREAMS_CAPTURE = max(1, min(AUX_STREAMS_MAX, int(n)))
    return prev


_aux_next = {}


def fork_aux(device):
    idx = device.index if device.index is not None else torch.cuda.current_device()
    pool = _aux_streams.get(idx)
    if pool is None:
        pool = _aux_streams[idx] = [_make_aux_stream(device) for _ in range(AUX_STREAMS_MAX)]
        _aux_events[idx] = [torch.cuda.Event() for _ in range(AUX_STREAMS_MAX)]
        _aux_dirty[idx] = set()
        _aux_next[idx] = 0
    n = AUX_STREAMS_CAPTURE if CAPTURING > 0 else AUX_STREAMS
    k = _aux_next[idx] % n
    _aux_next[idx] = (k + 1) % n
    aux = pool[k]
    ev = _aux_events[idx][k]       # one event object per stream, re-recorded: a wait captures the record that precedes it
    ev.record(_current_stream_obj(device))
    aux.wait_event(ev)
    _aux_dirty[idx].add(k)
    return aux


def aux_streams_in_use(device):
    """The auxiliary streams that work was forked onto since the last join (possibly none)."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    pool = _aux_streams.get(idx)
    return [pool[k] for k in sorted(_aux_dirty.get(idx, ()))] if pool else []


def join_aux(device):
    idx = device.index if device.index is not None else torch.cuda.current_device()
    dirty = _aux_dirty.get(idx)
    if dirty:
        cur = torch.cuda.current_stream(device)
        for k in sorted(dirty):
            cur.wait_stream(_aux_streams[idx][k])
        dirty.clear()
        _aux_next[idx] = 0


# ---------------------------------------------------------------------------------------------- branch lanes
# A model with independent branches (HRNet: up to four resolution branches of 8 convs each between two fusion points, then
# one independent accumulation chain per fused output) is a few hundred launches of 5-20 us on ONE stream: every small
# kernel of a low-resolution branch waits for the one before it while 200 CUs idle.  While a step is being CAPTURED the
# branches are enqueued on streams of their own (forked behind an event of the current stream, joined before the next
# fusion); the lane executor (csrc/lanes.hip) finds them in the captured graph as parallel chains and replays them on
# parallel lanes.  Eager steps stay on one stream -- they are bound by the host's enqueue rate, not by the device -- unless
# PSEG_BRANCH_EAGER=1 (tests).  Same kernels, same arguments, same order within every chain: results are bit-identical.
# PSEG_BRANCH_STREAMS=0 switches the forks off.
# Three streams (one per non-main branch of HRNet).  The HIP runtime multiplexes the streams of a process onto four hardware
# queues (GPU_MAX_HW_QUEUES), a lane that shares its queue with the main chain blocks it (head of the line), and five busy
# queues (GPU_MAX_HW_QUEUES=8) fall off a cliff -- HRNet -mp 18 ms/step against 9.1; profiles/EXPERIMENTS.md section 0.12.
# The replay itself is capped by the model (`replay_lanes`: HRNet 5 -- forward: main chain + three branch lanes; backward: six
# chains on five lanes).  Measured (branch streams, lanes): (2, 4) 7.75, (2, 5) 7.40, (3, 4) 7.21, (3, 5) 7.11-7.17, (3, 6) 7.30 ms.
BRANCH_STREAMS = max(0, min(6, int(os.environ.get('PSEG_BRANCH_STREAMS', '3'))))
BRANCH_EAGER = os.environ.get('PSEG_BRANCH_EAGER', '0') == '1'
_branch_pool = {}
_branch_depth = 0
_branch_deferred = []


def after_branches(fn):
    """Run fn() now, or -- inside a Branches region, where "everything enqueued so far" is spread over several streams --
    when the region has been joined (the gradient-bucket markers of a captured data-parallel step)."""
    if _branch_depth > 0:
        _branch_deferred.append(fn)
    else:
        fn()


def reset_branches():
    """After an exception inside a Branches region (a failed capture): forget the open region and its deferred callbacks, so
    that the next step forks again instead of running with the forks silently off."""
    global _branch_depth
    _branch_depth = 0
    del _branch_deferred[:]


class _Lane:
    __slots__ = ('ctx',)

    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        if self.ctx is not None:
            self.ctx.__enter__()

    def __exit__(self, *exc):
        if self.ctx is not None:
            return self.ctx.__exit__(*exc)
        return False


class Branches:
    """b = Branches(device, n); for i: `with b.lane(i, *inputs): ...`; b.join(*outputs).

    lane 0 is the current stream; lane i > 0 a pooled stream ordered behind everything enqueued on the current stream when
    the region opened.  `inputs`: the Acts / tensors the lane reads that were allocated elsewhere, `outputs`: what the
    code after the join reads -- both are recorded with the caching allocator for the stream that uses them (a block must
    not be handed out again on its own stream while another stream still reads it; inside a capture that defers the
    release to the end of the capture).  Off (everything on the current stream) outside a capture, inside another region,
    or for a single lane."""

    def __init__(self, device, n):
        global _branch_depth
        self.on = n > 1 and BRANCH_STREAMS > 0 and (CAPTURING > 0 or BRANCH_EAGER) and _branch_depth == 0
        if not self.on:
            return
        idx = device.index if device.index is not None else torch.cuda.current_device()
        pool = _branch_pool.get(idx)
        if pool is None:
            pool = _branch_pool[idx] = [new_stream(device) for _ in range(BRANCH_STREAMS)]
        self.pool = pool
        self.main = torch.cuda.current_stream(device)
        self.fork = torch.cuda.Event()
        self.fork.record(self.main)
        self.used = []
        _branch_depth += 1

    @staticmethod
    def _record(items, stream):
        for a in items:
            if a is None:
                continue
            t = a.t if isinstance(a, Act) else a
            t.record_stream(stream)

    def lane(self, i, *inputs):
        if not self.on or i == 0:
            return _Lane(None)
        s = self.pool[(i - 1) % len(self.pool)]
        if s not in self.used:
            s.wait_event(self.fork)
            self.used.append(s)
        self._record(inputs, s)
        return _Lane(torch.cuda.stream(s))

    def join(self, *outputs):
        global _branch_depth
        if not self.on:
            return
        for s in self.used:
            self.main.wait_stream(s)
        self._record(outputs, self.main)
        _branch_depth -= 1
        self.on = False
        if _branch_depth == 0 and _branch_deferred:
            fns = list(_branch_deferred)
            del _branch_deferred[:]
            for fn in fns:
                fn()


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _pl(a):
    """(pointer, pixel stride) of an optional Act: (0, 0) without one"""
    return (0, 0) if a is None else (a.t.data_ptr(), a.ld)


def _rows4(co):
    """The four row pointers of a [4][C] coefficient tensor (mean, invstd, scale, shift), by arithmetic: indexing a tensor costs
    ~2 us a time, and the callers run once per layer and step."""
    c0, cs = co.data_ptr(), co.shape[1] * 4
    return c0, c0 + cs, c0 + 2 * cs, c0 + 3 * cs


class Act:
    """NHWC activation [B,H,W,C] with pixel stride ``ld`` (elements); ``t`` is a 1-D tensor whose first element is
    element (0,0,0,0) and which keeps the storage alive.  fp32 everywhere except under the half-precision (`-mp`)
    policy, where activations and their gradients are fp16 (C % 8 == 0, ld % 8 == 0: 16 bytes = 8 channels)."""
    __slots__ = ('t', 'B', 'H', 'W', 'C', 'ld', 'amax', 'planes', 'bnpart')

    def __init__(self, t, B, H, W, C, ld, amax=None):
        assert t.dtype in (torch.float32, torch.float16) and t.dim() == 1
        q = 4 if t.dtype == torch.float32 else 8
        assert ld % q == 0 and ld >= C and t.data_ptr() % 16 == 0, \
            'NHWC handle must be 16-byte aligned, ld %% %d == 0' % q
        assert t.dtype == torch.float32 or C % 8 == 0, 'fp16 activations carry multiples of 8 channels'
        need = ((B * H * W - 1) * ld + C) if B * H * W > 0 else 0
        assert t.numel() >= need, 'backing tensor too small'
        self.t, self.B, self.H, self.W, self.C, self.ld = t, B, H, W, C, ld
        # optional device scalar: an upper bound of max|x| over this tensor (and every slice sharing it); the fp16-limb
        # conv kernels scale their operands by it.  Producers raise it atomically; it must start at 0.
        self.amax = amax
        # bf16 limb planes of this tensor (Planes), when its producer wrote them alongside (bn_act_bwd(want_planes=True))
        self.planes = None
        # BatchNorm-backward partial sums of this tensor seen as a layer's dz, when the data gradient that produced it
        # computed them alongside (conv2d_dgrad(bn=...)): BnPart
        self.bnpart = None

    @property
    def M(self):
        return self.B * self.H * self.W

    @property
    def ptr(self):
        return self.t.data_ptr()

    @property
    def device(self):
        return self.t.device

    @property
    def dtype(self):
        return self.t.dtype

    @property
    def half(self):
        return self.t.dtype == torch.float16

    @staticmethod
    def empty(B, H, W, C, device, zero=False, ld=None, amax=False, dtype=torch.float32):
        if ld is None:
            ld = _round4(C) if dtype == torch.float32 else _round8(C)
        n = B * H * W * ld
        t = torch.zeros(n, dtype=dtype, device=device) if zero else torch.empty(n, dtype=dtype, device=device)
        return Act(t, B, H, W, C, ld, new_amax(t.device) if amax else None)

    def new(self, B, H, W, C, zero=False, amax=False):
        """A fresh activation of this one's storage type on its device."""
        return Act.empty(B, H, W, C, self.t.device, zero=zero, amax=amax, dtype=self.t.dtype)

    def like(self, C=None, zero=False, dtype=None):
        return Act.empty(self.B, self.H, self.W, self.C if C is None else C, self.t.device, zero=zero,
                         dtype=self.t.dtype if dtype is None else dtype)

    def slice(self, c0, c1):
        """Channels [c0, c1) of this activation (no copy)."""
        q = 8 if self.half else 4
        assert 0 <= c0 < c1 <= self.ld and c0 % q == 0
        return Act(self.t[c0:], self.B, self.H, self.W, c1 - c0, self.ld, self.amax)

    def to(self, dtype, scale=None):
        """A converted copy (fp32 <-> fp16), optionally multiplied by the device scalar `scale` (the loss scale)."""
        out = self.like(dtype=dtype)
        _lib.call('pseg_convert2d', self.ptr, int(self.half), self.ld, out.ptr, int(out.half), out.ld, self.M, self.C,
                  _ptr(scale), _stream())
        return out

    def view4(self):
        """Strided torch view [B,H,W,C] in the handle's own dtype (tests / debugging / host-side glue only)."""
        return torch.as_strided(self.t, (self.B, self.H, self.W, self.C),
                                (self.H * self.W * self.ld, self.W * self.ld, self.ld, 1))

    def to_nchw(self, C=None):
        """Contiguous fp32 NCHW torch tensor with the first C channels (layout kernel, not torch.permute)."""
        C = self.C if C is None else C
        src = self.to(torch.float32) if self.half else self
        out = torch.empty(self.B, C, self.H, self.W, dtype=torch.float32, device=self.t.device)
        _lib.call('pseg_nhwc_to_nchw', src.ptr, src.ld, out.data_ptr(), self.B, C, self.H * self.W, _stream())
        return out

    @staticmethod
    def from_nchw(x, Cpad=None, dtype=torch.float32):
        """fp32 NCHW torch tensor -> NHWC handle, channels zero-padded up to Cpad (default: next multiple of 4; 8 for
        fp16 handles)."""
        assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 4
        x = x.contiguous()
        B, C, H, W = x.shape
        if dtype == torch.float16:
            Cpad = _round8(C if Cpad is None else Cpad)
        else:
            Cpad = _round4(C) if Cpad is None else Cpad
        if dtype == torch.float16 and C <= 8 and Cpad == 8:      # the image: straight into 8-channel fp16 pixels, one pass
            out = Act.empty(B, H, W, 8, x.device, dtype=torch.float16)
            _lib.call('pseg_nchw_to_nhwc_h', x.data_ptr(), out.ptr, out.ld, B, C, H * W, _stream())
            return out
        out = Act.empty(B, H, W, Cpad, x.device, ld=_round4(Cpad))
        _lib.call('pseg_nchw_to_nhwc', x.data_ptr(), out.ptr, out.ld, B, C, H * W, Cpad, _stream())
        return out.to(dtype) if dtype != torch.float32 else out


class _Workspace:
    """One growing scratch tensor per (device, stream).  Kernels on a stream run in order, so a single
    buffer per stream is race-free; torch's allocator makes growth stream-safe."""

    def __init__(self):
        self._bufs = {}
        self._retired = []

    def get(self, nbytes, device):
        key = (device.index, _stream())     # raw handle of the current stream (0.3 us; current_stream() builds objects: 5 us)
        buf = self._bufs.get(key)
        if buf is None or buf.numel() < nbytes:
            if buf is not None and EVER_CAPTURED:
                # a captured step (Trainer graph mode) has this buffer's address baked into its launches: a larger request
                # must not free it under the graph's feet -- retired buffers stay alive for the life of the process
                self._retired.append(buf)
            nbytes = max(int(nbytes), 1 << 20)
            buf = torch.empty((nbytes + 255) // 256 * 256, dtype=torch.uint8, device=device)
            self._bufs[key] = buf
        return buf


workspace = _Workspace()


def conv_out_size(n, k, stride, pad, dil):
    return (n + 2 * pad - dil * (k - 1) - 1) // stride + 1


# ---------------------------------------------------------------------------------------------- convolution
class AmaxPool:
    """Per-step pool of device scalars for the per-tensor max|x| bounds of the fp16-limb forward: one zero-fill per
    forward pass instead of one torch.zeros(1) launch per BatchNorm layer (~100 launches in HRNet)."""

    def __init__(self, device, n=2048):
        self.buf = torch.zeros(n, dtype=torch.float32, device=device)
        self.n, self.used = n, 0

    def reset(self):
        if self.used:
            self.buf[:self.used].zero_()
        self.used = 0

    def take(self):
        if self.used >= self.n:
            return torch.zeros(1, dtype=torch.float32, device=self.buf.device)
        v = self.buf[self.used:self.used + 1]
        self.used += 1
        return v


_amax_pool = None      # the pool of the forward pass in flight (Trainer._fwd_loss_bwd installs / removes it)


def new_amax(device):
    """A zeroed device scalar for an amax bound."""
    if _amax_pool is not None and _amax_pool.buf.device == device:
        return _amax_pool.take()
    return torch.zeros(1, dtype=torch.float32, device=device)


def amax_of(t_or_act):
    """Device scalar holding max|x| of a torch tensor or an Act (fresh computation with the generic kernel)."""
    out = new_amax(t_or_act.device)
    if isinstance(t_or_act, Act):
        a = t_or_act
        _lib.call('pseg_amax', a.ptr, a.ld, a.M, a.C, out.data_ptr(), _stream())
    else:
        t = t_or_act
        assert t.is_contiguous()
        _lib.call('pseg_amax', t.data_ptr(), t.numel(), 1, t.numel(), out.data_ptr(), _stream())
    return out


# ---- operands above 2 GiB (round 6) --------------------------------------------------------------------------------------
# The conv kernels read their GATHERED operand (x of a forward conv, dy of a data gradient, x and dy of a weight gradient)
# through ONE buffer descriptor with 32-bit byte offsets: the range check that makes padding and ragged edges free caps that
# tensor at 2 GiB (csrc/conv_common.h kMaxBytes; results are addressed with 64-bit pointers and are not capped).  On a 288 GB
# part that is per-GPU batch ~120 at 512x512 -- and `-s` / `-bs` are free-form in the reference (train.py:88-90).  A conv is
# independent per image, so an operand above the cap is handed to the library in equal BATCH CHUNKS (the smallest divisor of B
# whose chunk fits): forward convs and data gradients write disjoint image ranges of their result, weight gradients add chunk
# after chunk into the gradient (fp32, fixed chunk order: reproducible), fused BatchNorm statistics are the chunks' partial rows
# side by side (legal when a chunk is whole row groups -- checked).  What does not chunk (a single image above 2 GiB, B with
# no fitting divisor) keeps the library's "exceeds 2 GiB" error.
_CAP_BYTES = (1 << 31) - 64


def _span_bytes(a):
    return ((a.M - 1) * a.ld + a.C) * (2 if a.half else 4) if a.M > 0 else 0


def _batch_chunks(*acts):
    """-> images per chunk (== B when every operand fits its descriptor)"""
    B = acts[0].B
    for a in acts:          # (the common case in two comparisons per operand: this sits in front of every conv call)
        if ((a.B * a.H * a.W - 1) * a.ld + a.C) * (2 if a.t.dtype == torch.float16 else 4) >= _CAP_BYTES:
            break
    else:
        return B
    for d in range(2, B + 1):
        if B % d == 0 and all(_span_bytes(_sub(a, 0, B // d)) < _CAP_BYTES for a in acts):
            return B // d
    return B          # (no fitting divisor: the library reports the cap)


def _sub(a, b0, nb):
    """images [b0, b0 + nb) of an activation (no copy)"""
    return Act(a.t[b0 * a.H * a.W * a.ld:], nb, a.H, a.W, a.C, a.ld, a.amax)


def conv2d_fwd(x, w_raw, bias_raw, y, kh, kw, stride, pad, dil, accumulate=False, want_stats=False, precision=None,
               amax_x=None, amax_w=None):
    """y = conv(x, w) (+bias); an x above the 2 GiB descriptor cap runs in batch chunks (see above)."""
    nb = _batch_chunks(x)
    if nb == x.B:
        return _conv2d_fwd_one(x, w_raw, bias_raw, y, kh, kw, stride, pad, dil, accumulate, want_stats, precision, amax_x, amax_w)
    parts = []
    for b0 in range(0, x.B, nb):
        parts.append(_conv2d_fwd_one(_sub(x, b0, nb), w_raw, bias_raw, _sub(y, b0, nb), kh, kw, stride, pad, dil, accumulate,
                                     want_stats, precision, amax_x, amax_w))
    if not want_stats:
        return None
    rows, group = parts[0][1], parts[0][2]
    # row group g of chunk c is row group c * rows + g of the whole tensor only when a chunk is WHOLE groups
    if any(p[1] != rows or p[2] != group for p in parts) or rows * group != nb * y.H * y.W:
        raise _lib.PsegError('conv2d_fwd: a %d-image chunk of this %d-image tensor (operand above 2 GiB) is not whole '
                             'statistics groups (%d rows of %d for %d pixels)' % (nb, x.B, rows, group, nb * y.H * y.W))
    return torch.cat([p[0] for p in parts], dim=1).contiguous(), rows * len(parts), group


def _conv2d_fwd_one(x, w_raw, bias_raw, y, kh, kw, stride, pad, dil, accumulate=False, want_stats=False, precision=None,
                    amax_x=None, amax_w=None):
    """y = conv(x, w) (+bias).  w_raw is [Cout][kh][kw][Cin] with Cin == x.C, Cout == y.C.
    Returns (stat[3][rows][Cout], rows, group) when want_stats (fused into the epilogue when the plan allows,
    otherwise a separate column-statistics pass), else None."""
    Cout, Cin = y.C, x.C
    assert w_raw.numel() == Cout * kh * kw * Cin and w_raw.is_contiguous()
    assert y.B == x.B and y.H == conv_out_size(x.H, kh, stride, pad, dil) and y.W == conv_out_size(x.W, kw, stride, pad, dil)
    dev = x.device
    sfx = '_h' if x.half else ''
    # (the fp16 kernels take no workspace: their statistics are always fused)
    ws_bytes = 0 if x.half else _lib.query('pseg_conv2d_fwd_workspace_bytes', x.B, y.H, y.W, Cin, Cout, kh, kw)
    fused = want_stats and ws_bytes == 0
    st, rows, group = None, 0, 0
    if fused:
        geo = (x.B, y.H, y.W, Cin, Cout, kh, kw, stride, pad, dil)
        rows = _lib.query('pseg_conv2d_stat_rows' + sfx, *geo)
        group = _lib.query('pseg_conv2d_stat_group' + sfx, *geo)
        st = torch.empty(3, rows, Cout, dtype=torch.float32, device=dev)
    if x.half:
        # half-precision path: fp16 operands, one fp16 MFMA pass, fp32 accumulate; y fp16 (or fp32: the class logits)
        assert w_raw.dtype == torch.float16, 'fp16 activations need the fp16 filter copy (ParamArena.prepare_half)'
        _lib.call('pseg_conv2d_fwd_h', x.ptr, x.ld, w_raw.data_ptr(), _ptr(bias_raw), y.ptr, y.ld, int(not y.half), x.B,
                  x.H, x.W, Cin, y.H, y.W, Cout, kh, kw, stride, pad, dil, int(accumulate), _ptr(st), _stream())
    else:
        ws = workspace.get(ws_bytes, dev) if ws_bytes else None
        _lib.call('pseg_conv2d_fwd', x.ptr, x.ld, w_raw.data_ptr(), _ptr(bias_raw), y.ptr, y.ld, x.B, x.H, x.W, Cin,
                  y.H, y.W, Cout, kh, kw, stride, pad, dil, int(accumulate), _fwd_prec(precision, amax_x, amax_w),
                  _ptr(amax_x), _ptr(amax_w), _ptr(st), _ptr(ws), ws_bytes, _stream())
    if want_stats and not fused:
        return col_stats(y)
    return (st, rows, group) if want_stats else None


def filter_transpose(w_raw, Cout, taps, Cin):
    wT = torch.empty_like(w_raw)
    _lib.call('pseg_filter_transpose', w_raw.data_ptr(), wT.data_ptr(), Cout, taps, Cin, _stream())
    return wT


def _fwd_prec(precision, amax_a, amax_b, backward=False):
    """fp16 limbs need both per-tensor maxima; without them the call runs on the exact fp32 kernel."""
    pr = _prec(precision, backward)
    if pr == PREC_FP16X3 and (amax_a is None or amax_b is None):
        return PREC_FP32
    return pr


class BnPart:
    """[2][rows][C] partial sums (dbeta, dgamma) of a BatchNorm backward, written by the data gradient that produced dz;
    `key` names the layer they belong to (address of its saved y)."""
    __slots__ = ('part', 'rows', 'key')

    def __init__(self, part, rows, key):
        self.part, self.rows, self.key = part, rows, key


FUSE_BN_BWD = os.environ.get('PSEG_FUSE_BN_BWD', '1') == '1'
# ... under the half-precision policy: OFF by default.  Built, parity-tested (tests/test_half_gpu.py) and measured SLOWER in the
# step: DeepLabV3+ -mp 13.85-13.93 ms without, 13.96-14.04 with (32 reduction launches of ~12 us gone, the 32 data gradients that
# carry their sums instead each a few us longer -- and under -mp the data-gradient chain IS the critical path;
# profiles/EXPERIMENTS.md 5.8).  PSEG_FUSE_BN_BWD_H=1 switches it on.
FUSE_BN_BWD_H = os.environ.get('PSEG_FUSE_BN_BWD_H', '0') == '1'


def conv2d_dgrad(dy, wT_raw, dx, kh, kw, stride, pad, dil, accumulate=False, precision=None, amax_dy=None,
                 amax_w=None, bn=None):
    """dx (+)= conv_transpose(dy, w); a dy above the 2 GiB descriptor cap runs in batch chunks (without the fused
    BatchNorm-backward sums: dx.bnpart stays None and bn_act_bwd takes its own reduction pass)."""
    nb = _batch_chunks(dy)
    if nb == dy.B:
        return _conv2d_dgrad_one(dy, wT_raw, dx, kh, kw, stride, pad, dil, accumulate, precision, amax_dy, amax_w, bn)
    for b0 in range(0, dy.B, nb):
        _conv2d_dgrad_one(_sub(dy, b0, nb), wT_raw, _sub(dx, b0, nb), kh, kw, stride, pad, dil, accumulate, precision, amax_dy,
                          amax_w, None)
    dx.bnpart = None


def _conv2d_dgrad_one(dy, wT_raw, dx, kh, kw, stride, pad, dil, accumulate=False, precision=None, amax_dy=None,
                      amax_w=None, bn=None):
    """dx (+)= conv_transpose(dy, w); wT_raw is the [Cin][kh][kw][Cout] transposed filter.
    bn = (y, co, act) of the BatchNorm + activation layer that produced the conv's input, when dx is that layer's dz and
    nothing else adds to it: the kernel then also writes the layer's backward partial sums (dx.bnpart; pseg_conv2d_dgrad_bnstat /
    _bnstat_h) where the problem runs on a kernel that can (exact fp32: the LDS-DMA tiles; fp16: every gather kernel) -- bn_act_bwd
    skips its reduction pass."""
    Cout, Cin = dy.C, dx.C
    assert wT_raw.numel() == Cout * kh * kw * Cin

    def fused_sums(sfx):
        """The data gradient with the layer's partial sums, fp32 ('') or fp16 ('_h'); False where no kernel carries them."""
        y, co, act = bn
        rows = _lib.query('pseg_conv2d_dgrad_bnstat_rows' + sfx, dx.B, dx.H, dx.W, Cin, dy.H, dy.W, Cout, kh, kw, stride, pad, dil)
        if not (rows > 0 and y.C == Cin and y.M == dx.M and y.half == (sfx == '_h')):
            return False
        part = torch.empty(2, rows, Cin, dtype=torch.float32, device=dx.device)
        p0 = part.data_ptr()
        # (the rows query and the launch read one kernel choice: select_gather in conv_gather.hip, select_gather_h in
        # conv_half_gather.hip)
        _lib.call('pseg_conv2d_dgrad_bnstat' + sfx, dy.ptr, dy.ld, wT_raw.data_ptr(), dx.ptr, dx.ld, dx.B, dx.H, dx.W, Cin, dy.H,
                  dy.W, Cout, kh, kw, stride, pad, dil, y.ptr, y.ld, *_rows4(co), act, p0, p0 + rows * Cin * 4, rows, _stream())
        dx.bnpart = BnPart(part, rows, y.ptr)
        return True

    if bn is not None and FUSE_BN_BWD and not dy.half and not accumulate and _prec(precision, True) == PREC_FP32 and fused_sums(''):
        return
    if dy.half:
        assert wT_raw.dtype == torch.float16 and dx.half
        if bn is not None and FUSE_BN_BWD_H and not accumulate and fused_sums('_h'):
            return
        _lib.call('pseg_conv2d_dgrad_h', dy.ptr, dy.ld, wT_raw.data_ptr(), dx.ptr, dx.ld, dx.B, dx.H, dx.W, Cin, dy.H, dy.W,
                  Cout, kh, kw, stride, pad, dil, int(accumulate), _stream())
        return
    # the dgrad GEMM has M = input pixels, N = Cin, K = kh*kw*Cout
    ws_bytes = _lib.query('pseg_conv2d_fwd_workspace_bytes', dx.B, dx.H, dx.W, Cout, Cin, kh, kw)
    ws = workspace.get(ws_bytes, dx.device) if ws_bytes else None
    _lib.call('pseg_conv2d_dgrad', dy.ptr, dy.ld, wT_raw.data_ptr(), dx.ptr, dx.ld, dx.B, dx.H, dx.W, Cin, dy.H,
              dy.W, Cout, kh, kw, stride, pad, dil, int(accumulate), _fwd_prec(precision, amax_dy, amax_w, True),
              _ptr(amax_dy), _ptr(amax_w), _ptr(ws), ws_bytes, _stream())


class Planes:
    """bf16 limb planes of an fp32 [M][C] tensor: hi = bf16(x), lo = bf16(x - hi), each [M][ldp] (int16 storage)."""
    __slots__ = ('hi', 'lo', 'ldp', 'M', 'C')

    def __init__(self, hi, lo, ldp, M, C):
        self.hi, self.lo, self.ldp, self.M, self.C = hi, lo, ldp, M, C


def split_planes(x):
    """Act or contiguous 2-D-like torch tensor ([rows][C] fp32) -> Planes (one HBM-bound pass)."""
    if isinstance(x, Act):
        ptr, ld, M, C, dev = x.ptr, x.ld, x.M, x.C, x.device
    else:
        assert x.is_contiguous() and x.dtype == torch.float32
        M, C = x.shape[0], x.numel() // x.shape[0]
        ptr, ld, dev = x.data_ptr(), C, x.device
    ldp = (C + 7) // 8 * 8
    hi = torch.empty(M * ldp, dtype=torch.int16, device=dev)
    lo = torch.empty(M * ldp, dtype=torch.int16, device=dev)
    _lib.call('pseg_split_planes', ptr, ld, M, C, hi.data_ptr(), lo.data_ptr(), ldp, _stream())
    return Planes(hi, lo, ldp, M, C)


def dgrad_planes_ok(dy, dx, kh, kw, stride, pad, dil):
    """True when the pre-split LDS-DMA limb kernel covers this data gradient (see pseg_conv2d_dgrad_planes_ok)."""
    return bool(_lib.query('pseg_conv2d_dgrad_planes_ok', dx.B, dx.H, dx.W, dx.C, dy.H, dy.W, dy.C, kh, kw, stride, pad, dil))


def dgrad_planes_ok_shape(B, H, W, Cin, Ho, Wo, Cout, kh, kw, stride, pad, dil):
    return bool(_lib.query('pseg_conv2d_dgrad_planes_ok', B, H, W, Cin, Ho, Wo, Cout, kh, kw, stride, pad, dil))


def conv2d_dgrad_planes(dy_planes, dy, wT_planes, dx, kh, kw, stride, pad, dil, accumulate=False):
    """dx (+)= conv_transpose(dy, w) in BF16X3 arithmetic from pre-split operands (dy: Act giving the geometry)."""
    _lib.call('pseg_conv2d_dgrad_planes', dy_planes.hi.data_ptr(), dy_planes.lo.data_ptr(), dy_planes.ldp,
              wT_planes.hi.data_ptr(), wT_planes.lo.data_ptr(), dx.ptr, dx.ld, dx.B, dx.H, dx.W, dx.C, dy.H, dy.W, dy.C,
              kh, kw, stride, pad, dil, int(accumulate), _stream())


class SlabPool:
    """Deferred reduction of split weight gradients: every split conv2d_wgrad of a backward pass leaves its slabs in a
    region owned by this pool (one per (gradient tensor, geometry), allocated once and kept), and `reduce()` folds them
    all into the gradient arena with ONE launch (pseg_slab_reduce_batch) instead of one launch-bound reduction per
    layer.  The job table lives on the device and is rebuilt only when the sequence of jobs of a pass changes (first
    step), so a pass can be captured in a hipGraph."""

    def __init__(self, device):
        self.device = device
        self.regions = {}        # key -> (slab tensor, elements per slab, splits, gradient tensor)
        self.pending = []        # keys of this pass, in call order
        # device job tables, one per job sequence ever seen, NEVER freed: a captured step has its table's address (and the
        # job count / block count of that sequence) baked into its slab_reduce_batch launch
        self.tables = {}         # tuple(keys) -> (device table, blocks)
        self.block = _lib.query('pseg_slab_reduce_block')

    def region(self, dw_raw, geom, splits):
        key = (dw_raw.data_ptr(), geom, splits)
        hit = self.regions.get(key)
        if hit is None:
            hit = self.regions[key] = (torch.empty(splits * dw_raw.numel(), dtype=torch.float32, device=self.device),
                                       dw_raw.numel(), splits, dw_raw)
        if key in self.pending:      # the same gradient twice in one pass: fold what is there first
            return None
        self.pending.append(key)
        return hit[0]

    def reduce(self, accumulate=False):
        """Fold every pending slab set into its gradient (dw = or += sum of slabs); call on the stream that joined the
        weight-gradient stream, before anything reads the gradients."""
        if not self.pending:
            return
        seq = tuple(self.pending)
        hit = self.tables.get(seq)
        if hit is None:
            if CAPTURING:
                # (the upload below is a pageable host-to-device copy: it would abort the capture.  The Trainer runs the
                # first step of every shape eagerly under the capture's own configuration, so this cannot happen there)
                raise RuntimeError('SlabPool: a new job sequence inside a stream capture; run one eager pass of this '
                                   'shape with the same Env first')
            rows, first = [], 0
            for key in self.pending:
                slabs, elems, splits, dw = self.regions[key]
                assert elems % 4 == 0
                rows.append([slabs.data_ptr(), dw.data_ptr(), elems, splits, first])
                first += (elems + self.block - 1) // self.block
            hit = self.tables[seq] = (torch.tensor(rows, dtype=torch.int64).to(self.device), first)
        table, blocks = hit
        _lib.call('pseg_slab_reduce_batch', table.data_ptr(), len(self.pending), blocks, int(accumulate), _stream())
        self.pending = []


def conv2d_wgrad(x, dy, dw_raw, kh, kw, stride, pad, dil, accumulate=False, precision=None, pool=None, concurrent=False):
    """dw (+)= x^T * dy; operands above the 2 GiB descriptor cap run in batch chunks that ADD into dw in chunk order (no slab
    pool for them: every chunk reduces its own slabs)."""
    nb = _batch_chunks(x, dy)
    if nb == x.B:
        return _conv2d_wgrad_one(x, dy, dw_raw, kh, kw, stride, pad, dil, accumulate, precision, pool, concurrent)
    for b0 in range(0, x.B, nb):
        _conv2d_wgrad_one(_sub(x, b0, nb), _sub(dy, b0, nb), dw_raw, kh, kw, stride, pad, dil, accumulate or b0 > 0, precision,
                          None, concurrent)


def _conv2d_wgrad_one(x, dy, dw_raw, kh, kw, stride, pad, dil, accumulate=False, precision=None, pool=None, concurrent=False):
    """pool (SlabPool): a split plan leaves its slabs with the pool -- `accumulate` is then the POOL's business
    (pool.reduce(accumulate)), and dw_raw is complete only after that call.
    concurrent: the launch runs beside another stream's kernels (Conv2d.bwd forks it onto the weight-gradient stream): the
    exact-fp32 plan then keeps ONE resident block per CU (half the slabs); alone it is planned for two."""
    Cout, Cin = dy.C, x.C
    assert dw_raw.numel() == Cout * kh * kw * Cin and dw_raw.is_contiguous()
    if x.half:
        # fp16 operands, fp32 gradient (the master gradient arena); one arithmetic, one plan
        assert dy.half and dw_raw.dtype == torch.float32
        sfx, extra, tag = '_h', (), ('h',)
    else:
        sfx = ''
        extra = tag = (_prec(precision, True), int(bool(concurrent)))
    if pool is not None:
        splits = _lib.query('pseg_conv2d_wgrad_splits' + sfx, x.B, dy.H, dy.W, Cin, Cout, kh, kw, *extra)
        if splits > 1:
            slabs = pool.region(dw_raw, (x.B, x.H, x.W, dy.H, dy.W, kh, kw, stride, pad, dil) + tag, splits)
            if slabs is not None:
                _lib.call('pseg_conv2d_wgrad_slabs' + sfx, x.ptr, x.ld, dy.ptr, dy.ld, slabs.data_ptr(), x.B, x.H, x.W, Cin,
                          dy.H, dy.W, Cout, kh, kw, stride, pad, dil, *extra, slabs.numel() * 4, _stream())
                return
            # a second gradient for the same filter in one pass (shared weights): fold what is parked, then add
            pool.reduce(accumulate)
            accumulate = True
    ws_bytes = _lib.query('pseg_conv2d_wgrad_workspace_bytes' + sfx, x.B, dy.H, dy.W, Cin, Cout, kh, kw)
    ws = workspace.get(ws_bytes, x.device) if ws_bytes else None
    _lib.call('pseg_conv2d_wgrad' + sfx, x.ptr, x.ld, dy.ptr, dy.ld, dw_raw.data_ptr(), x.B, x.H, x.W, Cin, dy.H, dy.W,
              Cout, kh, kw, stride, pad, dil, int(accumulate), *extra, _ptr(ws), ws_bytes, _stream())


def _h(name, act):
    """entry point for the activation's storage type: the fp16 instantiation carries the suffix _h"""
    return name + '_h' if act.t.dtype == torch.float16 else name


def dwconv_fwd(x, w_raw, y, k, stride, pad):
    _lib.call(_h('pseg_dwconv_fwd', x), x.ptr, x.ld, w_raw.data_ptr(), y.ptr, y.ld, x.B, x.H, x.W, x.C, y.H, y.W, k, stride,
              pad, _stream())


def dwconv_dgrad(dy, w_raw, dx, k, stride, pad):
    _lib.call(_h('pseg_dwconv_dgrad', dy), dy.ptr, dy.ld, w_raw.data_ptr(), dx.ptr, dx.ld, dx.B, dx.H, dx.W, dx.C, dy.H, dy.W,
              k, stride, pad, _stream())


def dwconv_wgrad(x, dy, dw_raw, k, stride, pad, accumulate=False):
    ws_bytes = _lib.query('pseg_dwconv_wgrad_workspace_bytes', x.B, dy.H, dy.W, x.C, k)
    ws = workspace.get(ws_bytes, x.device)
    _lib.call(_h('pseg_dwconv_wgrad', x), x.ptr, x.ld, dy.ptr, dy.ld, dw_raw.data_ptr(), x.B, x.H, x.W, x.C, dy.H, dy.W, k,
              stride, pad, int(accumulate), ws.data_ptr(), ws_bytes, _stream())


# ---------------------------------------------------------------------------------------------- batch norm
def col_stats(y):
    """-> (stat[3][rows][C] = pivot / shifted sum / shifted sum of squares per row group, rows, group)."""
    rows = _lib.query('pseg_col_stats_rows', y.M, y.C)
    st = torch.empty(3, rows, y.C, dtype=torch.float32, device=y.device)
    _lib.call(_h('pseg_col_stats', y), y.ptr, y.ld, y.M, y.C, st.data_ptr(), _stream())
    return st, rows, _lib.query('pseg_col_stats_group', y.M, y.C)


def bn_finalize(stats, count, gamma, beta, running_mean, running_var, momentum, eps):
    """-> coeff tensor [4][C]: mean, invstd, scale = gamma*invstd, beta (and updates the running statistics)."""
    st, rows, group = stats
    C = st.shape[-1]
    co = torch.empty(4, C, dtype=torch.float32, device=st.device)
    ws_bytes = _lib.query('pseg_bn_finalize_workspace_bytes', rows, C)
    ws = workspace.get(ws_bytes, st.device) if ws_bytes else None
    _lib.call('pseg_bn_finalize', st.data_ptr(), rows, group, count, C, _ptr(gamma), _ptr(beta),
              _ptr(running_mean), _ptr(running_var), float(momentum), float(eps), *_rows4(co), _ptr(ws), ws_bytes, _stream())
    return co


BN_SMALL_IN_GRAPH = os.environ.get('PSEG_BN_SMALL_GRAPH', '0') == '1'
CAPTURING = 0     # > 0 while a Trainer step is being captured for replay (utils/trainer.py)
EVER_CAPTURED = False   # a captured step exists (or existed): device buffers whose addresses it baked in are never freed


class no_gc_capture:
    """``with no_gc_capture(graph): ...`` = ``torch.cuda.graph(graph, capture_error_mode='thread_local')`` with the garbage
    collector held off while the capture is open.  A collection that happens to run between two captured launches finalizes
    whatever cycles earlier steps left behind (trainers, graphs, streams, events); a destructor that makes a synchronising
    HIP call inside a capture aborts the process (seen in rounds 2 and 3: a `Stream` / `Event` finalizer; torch.cuda.graph
    itself collects once BEFORE the capture begins, not during).  Every capture of the package and its tests goes through
    here."""

    def __init__(self, graph, **kw):
        kw.setdefault('capture_error_mode', 'thread_local')
        self._ctx = torch.cuda.graph(graph, **kw)
        # torch's default capture stream is one of its 32 pool streams too: should it BE one of the streams this package forks onto
        # (new_stream), the capture gets a stream of its own.  Only then -- a different capture stream moves the hardware queues the
        # replay's lanes land on: HRNet replayed 14.0 -> 14.7 ms fp32, 7.2 -> 7.75 ms -mp with an own capture stream always
        # (profiles/r06_ab_streams.txt).
        cap = getattr(self._ctx, 'capture_stream', None)
        if OWN_STREAMS and 'stream' not in kw and cap is not None:
            idx = cap.device.index if cap.device.index is not None else torch.cuda.current_device()
            if cap.stream_id in _own_stream_handles.get(idx, ()):
                kw['stream'] = new_stream(cap.device)
                self._ctx = torch.cuda.graph(graph, **kw)
        self._gc_was_on = False

    def __enter__(self):
        import gc
        self._gc_was_on = gc.isenabled()
        gc.disable()
        try:
            return self._ctx.__enter__()
        except BaseException:
            if self._gc_was_on:
                gc.enable()
            raise

    def __exit__(self, *exc):
        import gc
        try:
            return self._ctx.__exit__(*exc)
        finally:
            if self._gc_was_on:
                gc.enable()


def bn_small_path(rows, M, C):
    """True when the library recommends the fused finalize + apply launches (small tensors, launch-bound regime).
    Not while a step is being captured: a replayed step pays no host time per launch, and on the device the two plain
    launches are faster than the fused one (every block of which re-derives the coefficients): UNet 5.2 -> 5.0 ms."""
    return (CAPTURING == 0 or BN_SMALL_IN_GRAPH) and bool(_lib.query('pseg_bn_small_path', rows, M, C))


def bn_fwd_fused(stats, count, gamma, beta, running_mean, running_var, momentum, eps, y, act, z, residual=None):
    """bn_finalize + bn_act_fwd in ONE launch (small tensors): -> coeff tensor [4][C]; z is written."""
    st, rows, group = stats
    C = st.shape[-1]
    co = torch.empty(4, C, dtype=torch.float32, device=st.device)
    args = (st.data_ptr(), rows, group, count, C, _ptr(gamma), _ptr(beta), _ptr(running_mean),
            _ptr(running_var), float(momentum), float(eps), *_rows4(co), y.ptr, y.ld, *_pl(residual), act, z.ptr, z.ld, y.M)
    if y.half:
        _lib.call('pseg_bn_fwd_fused_h', *args, _stream())
    else:
        _lib.call('pseg_bn_fwd_fused', *args, _ptr(z.amax), _stream())
    return co


def bn_eval_coeffs(gamma, beta, running_mean, running_var, eps):
    C = running_mean.numel()
    co = torch.empty(4, C, dtype=torch.float32, device=running_mean.device)
    _lib.call('pseg_bn_eval_coeffs', _ptr(gamma), _ptr(beta), running_mean.data_ptr(), running_var.data_ptr(),
              float(eps), C, *_rows4(co), _stream())
    return co


def track_amax():
    """True when the forward conv policy needs per-tensor maxima (fp16 limbs)."""
    return FWD_PRECISION == PREC_FP16X3


def raise_amax(dst, src):
    """dst.amax = max(dst.amax, src.amax) on the device (bound propagation through max-preserving ops)."""
    if dst.amax is not None and src.amax is not None and dst.amax is not src.amax:
        torch.maximum(dst.amax, src.amax, out=dst.amax)


def bn_act_fwd(y, co, act, z, residual=None, want_mask=False):
    """z = act((y - mean)*scale + beta (+ residual)); co None -> plain activation / residual add.
    When z carries an amax scalar the kernel raises it to max|z|.
    want_mask (C % 32 == 0, an activation): also returns the activation bitmask [M][C/32] (int32) for bn_act_bwd."""
    assert z.M == y.M and z.C == y.C
    mu = sc = sh = 0
    if co is not None:
        mu, _, sc, sh = _rows4(co)
    mask = torch.empty(y.M * (y.C // 32), dtype=torch.int32, device=y.device) \
        if (want_mask and act != ACT_NONE and y.C % 32 == 0) else None
    args = (y.ptr, y.ld, mu, sc, sh, *_pl(residual), act, z.ptr, z.ld, y.M, y.C)
    if y.half:
        _lib.call('pseg_bn_act_fwd_h', *args, _ptr(mask), _stream())
    else:
        _lib.call('pseg_bn_act_fwd', *args, _ptr(z.amax), _ptr(mask), _stream())
    return mask


def bn_act_bwd(dz, z, y, co, act, dy, gamma_grad, beta_grad, accumulate=False, dres=None, res_accumulate=False,
               frozen=False, mask=None, want_planes=False, part=None):
    """Backward through act(BN(y) (+res)).  Writes dy, (+)= dgamma/dbeta, optional dres.
    z=None (allowed when the forward had no residual): the activation mask is recomputed from y.
    mask (bn_act_fwd(want_mask=True)): the large-tensor passes read this bitmask instead of z.
    want_planes (C % 8 == 0, dense dy, large-tensor path): the apply pass also writes dy as bf16 limb planes -> dy.planes.
    frozen: eval-mode BatchNorm (co from bn_eval_coeffs) -- the statistics are constants, dy = scale * dz * act'."""
    C, M, dev = y.C, y.M, y.device
    fused = part is not None and part.key == y.ptr and z is None and mask is None and tuple(part.part.shape[::2]) == (2, C)
    if fused:       # the data gradient that produced dz left the partial sums behind (conv2d_dgrad(bn=...)): no reduction pass
        rows, part = part.rows, part.part
    else:
        rows = _lib.query('pseg_col_stats_rows', M, C)
        part = torch.empty(2, rows, C, dtype=torch.float32, device=dev)
    zp, zld = _pl(z)
    c0, c1, c2, c3 = _rows4(co)
    p0 = part.data_ptr()
    p1 = p0 + rows * C * 4
    dzp, dzl, yp, yl, dyp, dyl = dz.ptr, dz.ld, y.ptr, y.ld, dy.ptr, dy.ld
    drp, drl = _pl(dres)
    st = _stream()
    if not fused:
        _lib.call(_h('pseg_bn_act_bwd_reduce', y), dzp, dzl, zp, zld, yp, yl, c0, c1, c2, c3, act, M, C, p0, p1, _ptr(mask), st)
    if bn_small_path(rows, M, C):      # finalize folded into the apply pass: one launch fewer
        _lib.call(_h('pseg_bn_bwd_fused', y), p0, p1, rows, M, C, _ptr(gamma_grad), _ptr(beta_grad), int(accumulate),
                  int(frozen), dzp, dzl, zp, zld, yp, yl, c0, c1, c2, c3, act, dyp, dyl, drp, drl, int(res_accumulate), M,
                  st)
        return
    cc = torch.empty(2, C, dtype=torch.float32, device=dev)
    k0 = cc.data_ptr()
    k1 = k0 + C * 4
    _lib.call('pseg_bn_bwd_finalize', p0, p1, rows, M, C, _ptr(gamma_grad), _ptr(beta_grad), int(accumulate),
              int(frozen), k0, k1, st)
    if y.half:
        _lib.call('pseg_bn_act_bwd_apply_h', dzp, dzl, zp, zld, yp, yl, c0, c1, c2, c3, k0, k1, act, dyp, dyl, drp, drl,
                  int(res_accumulate), M, C, _ptr(mask), st)
        return
    hi = lo = None
    if want_planes and C % 8 == 0 and dy.ld == C:
        hi = torch.empty(M * C, dtype=torch.int16, device=dev)
        lo = torch.empty(M * C, dtype=torch.int16, device=dev)
        dy.planes = Planes(hi, lo, C, M, C)
    _lib.call('pseg_bn_act_bwd_apply', dzp, dzl, zp, zld, yp, yl, c0, c1, c2, c3, k0, k1, act, dyp, dyl, drp, drl,
              int(res_accumulate), M, C, _ptr(mask), _ptr(hi), _ptr(lo), C, st)


def act_bwd(dz, z, act, dy, scale=None, dres=None, res_accumulate=False):
    """dy = scale * dz * act'(z) (eval-mode BN / plain activation backward); optional dres = dz * act'(z)."""
    _lib.call(_h('pseg_act_bwd', dz), dz.ptr, dz.ld, *_pl(z), _ptr(scale), act, *_pl(dy), *_pl(dres), int(res_accumulate), dz.M, dz.C,
              _stream())


def col_sum(dy, out, accumulate=False, C=None):
    C = dy.C if C is None else C
    rows = _lib.query('pseg_col_stats_rows', dy.M, C)
    nbytes = rows * C * 4
    ws = workspace.get(nbytes, dy.device)
    _lib.call(_h('pseg_col_sum', dy), dy.ptr, dy.ld, dy.M, C, out.data_ptr(), int(accumulate), ws.data_ptr(), nbytes, _stream())


def copy2d(x, y, accumulate=False):
    assert x.M == y.M and x.C == y.C and x.dtype == y.dtype
    _lib.call(_h('pseg_copy2d', x), x.ptr, x.ld, y.ptr, y.ld, x.M, x.C, int(accumulate), _stream())


# ---------------------------------------------------------------------------------------------- pool / resize
def pool_sum(x, out, scale):
    """out[b,0,0,c] = scale * sum over pixels (out is an Act with H = W = 1)."""
    assert out.B == x.B and out.H == 1 and out.W == 1 and out.C == x.C
    _lib.call(_h('pseg_pool_sum', x), x.ptr, x.ld, x.B, x.H * x.W, x.C, float(scale), out.ptr, out.ld, _stream())


def broadcast(x, y, scale=1.0, accumulate=False):
    """y[b,h,w,c] (+)= scale * x[b,0,0,c]."""
    assert x.H == 1 and x.W == 1 and x.B == y.B and x.C == y.C
    _lib.call(_h('pseg_broadcast', x), x.ptr, x.ld, y.B, y.H * y.W, y.C, float(scale), y.ptr, y.ld, int(accumulate), _stream())


def bilinear_fwd(x, y, align_corners):
    assert x.B == y.B and x.C == y.C and x.dtype == y.dtype
    if x.half:
        _lib.call('pseg_bilinear_fwd_h', x.ptr, x.ld, x.B, x.H, x.W, x.C, y.ptr, y.ld, y.H, y.W, int(align_corners), _stream())
        return
    _lib.call('pseg_bilinear_fwd', x.ptr, x.ld, x.B, x.H, x.W, x.C, y.ptr, y.ld, y.H, y.W, int(align_corners), 0, _stream())


def bilinear_fwd_nchw(x, C, Ho, Wo, align_corners):
    """NHWC handle -> contiguous fp32 NCHW torch tensor [B,C,Ho,Wo] (first C channels)."""
    if x.half:
        x = x.to(torch.float32)
    out = torch.empty(x.B, C, Ho, Wo, dtype=torch.float32, device=x.device)
    _lib.call('pseg_bilinear_fwd', x.ptr, x.ld, x.B, x.H, x.W, C, out.data_ptr(), 0, Ho, Wo, int(align_corners), 1, _stream())
    return out


def bilinear_bwd(dy, dx, align_corners, accumulate=False):
    assert dx.B == dy.B and dx.C == dy.C and dx.dtype == dy.dtype
    if dy.half:
        _lib.call('pseg_bilinear_bwd_h', dy.ptr, dy.ld, dx.B, dx.H, dx.W, dx.C, dx.ptr, dx.ld, dy.H, dy.W, int(align_corners),
                  int(accumulate), _stream())
        return
    _lib.call('pseg_bilinear_bwd', dy.ptr, dy.ld, dx.B, dx.H, dx.W, dx.C, dx.ptr, dx.ld, dy.H, dy.W, int(align_corners), 0,
              int(accumulate), 0, 0, _stream())


def bilinear_bwd_nchw(dy_nchw, dx, C, align_corners, accumulate=False):
    """Gradient w.r.t. the NHWC source from a contiguous NCHW gradient [B,C,Ho,Wo]."""
    assert dy_nchw.is_contiguous() and dy_nchw.shape[0] == dx.B and dy_nchw.shape[1] == C
    Ho, Wo = dy_nchw.shape[2], dy_nchw.shape[3]
    nbytes = _lib.query('pseg_bilinear_bwd_workspace_bytes', dx.B, dx.H, dx.W, C, Ho, Wo, 1)
    ws = workspace.get(nbytes, dx.device)
    _lib.call('pseg_bilinear_bwd', dy_nchw.data_ptr(), 0, dx.B, dx.H, dx.W, C, dx.ptr, dx.ld, Ho, Wo, int(align_corners), 1,
              int(accumulate), ws.data_ptr(), nbytes, _stream())


def maxpool_fwd(x, y, k, stride, pad, want_argmax=True):
    arg = torch.empty(y.M * y.C, dtype=torch.uint8, device=x.device) if want_argmax else None
    _lib.call(_h('pseg_maxpool_fwd', x), x.ptr, x.ld, x.B, x.H, x.W, x.C, y.ptr, y.ld, _ptr(arg), y.H, y.W, k, stride, pad, _stream())
    return arg


def bn_act_maxpool_fwd(x, co, act, y, k, stride, pad, want_argmax=True):
    """y = maxpool(act(BN(x))) with BN's coefficient tensor `co` ([4][C]: mean, invstd, scale, shift) -- the activated map never exists
    (pseg_bn_act_maxpool_fwd; same values and argmax as bn_act_fwd + maxpool_fwd)."""
    arg = torch.empty(y.M * y.C, dtype=torch.uint8, device=x.device) if want_argmax else None
    mu, _, sc, sh = _rows4(co)
    _lib.call(_h('pseg_bn_act_maxpool_fwd', x), x.ptr, x.ld, mu, sc, sh, act, x.B, x.H, x.W, x.C, y.ptr, y.ld,
              _ptr(arg), y.H, y.W, k, stride, pad, _stream())
    return arg


def maxpool_bwd(dy, arg, dx, k, stride, pad, accumulate=False):
    _lib.call(_h('pseg_maxpool_bwd', dy), dy.ptr, dy.ld, arg.data_ptr(), dx.B, dx.H, dx.W, dx.C, dx.ptr, dx.ld, dy.H, dy.W, k,
              stride, pad, int(accumulate), _stream())


# ---------------------------------------------------------------------------------------------- loss / masks
def _loss_operands(logits, target):
    """the loss entry points' shared operand check -> (B, C, H, W)"""
    assert logits.is_cuda and logits.dtype == torch.float32 and logits.is_contiguous() and logits.dim() == 4
    assert target.dtype == torch.int64 and target.is_contiguous() and target.shape == (logits.shape[0],) + logits.shape[2:]
    return logits.shape


def _loss_class_weight(class_weight, logits):
    if class_weight is not None:
        C = logits.shape[1]
        assert class_weight.device == logits.device and class_weight.dtype == torch.float32 and \
            class_weight.is_contiguous() and class_weight.shape == (C,), 'class_weight: %d fp32 values on %s' % (C, logits.device)


def _loss_call(entry, head, logits, want_grad, n_out, ws_query, cache, tail=()):
    """the loss entry points' shared call shape, entry(*head, dlogits, out, *tail, workspace, workspace bytes, stream): a
    fresh gradient (want_grad) and out[n_out]; the workspace sized by the query ws_query = (name, *integers) and taken from
    `cache` -> (out, dlogits | None)"""
    dl = torch.empty_like(logits) if want_grad else None
    out = torch.empty(n_out, dtype=torch.float32, device=logits.device)
    nbytes = _lib.query(*ws_query)
    ws = cache.get(nbytes, logits.device)
    _lib.call(entry, *head, _ptr(dl), out.data_ptr(), *tail, ws.data_ptr(), nbytes, _stream())
    return out, dl


def ce_fwd_bwd(logits, target, want_grad=True, ignore_index=-100):
    """logits: contiguous NCHW fp32 cuda, target: NHW int64.
    -> (loss_out[3] = [mean loss, n_valid, n_out_of_range_targets], dlogits|None)."""
    B, C, H, W = _loss_operands(logits, target)
    return _loss_call('pseg_ce_fwd_bwd', (logits.data_ptr(), target.data_ptr(), B, C, H * W, ignore_index), logits, want_grad,
                      3, ('pseg_ce_workspace_bytes', B * H * W), workspace)


def ce_opts_fwd_bwd(logits, target, class_weight=None, label_smoothing=0.0, focal_gamma=0.0, keep_ratio=1.0, want_grad=True,
                    ignore_index=-100):
    """Cross-entropy with class weights, label smoothing, the focal factor and hard-pixel selection (pseg_ce_opts_fwd_bwd).
    logits: contiguous NCHW fp32 cuda, target: NHW int64, class_weight: [C] fp32 on the logits' device or None.
    -> (out[6] = [loss, n_valid, n_out_of_range_targets, n_kept, tau, sum of the kept pixels' weights], dlogits|None)."""
    B, C, H, W = _loss_operands(logits, target)
    _loss_class_weight(class_weight, logits)
    head = (logits.data_ptr(), target.data_ptr(), B, C, H * W, ignore_index, _ptr(class_weight), float(label_smoothing),
            float(focal_gamma), float(keep_ratio))
    return _loss_call('pseg_ce_opts_fwd_bwd', head, logits, want_grad, 6, ('pseg_ce_opts_workspace_bytes', B, C, H * W), workspace)


def bin_weight_table(values, device):
    """256 pixel weights -> the contiguous fp32 [256] tensor on `device` that ce_opts_binned_fwd_bwd takes.  The values are
    checked HERE, on the host before the upload (finite and non-negative: pseg_ce_opts_binned_fwd_bwd's precondition, which
    the C call cannot check without reading device memory)."""
    t = torch.as_tensor(values, dtype=torch.float32).detach().cpu().contiguous()
    if t.shape != (256,):
        raise ValueError('bin_weight: 256 values, one per byte value (got shape %s)' % (tuple(t.shape),))
    if not bool(torch.isfinite(t).all()) or bool((t < 0).any()):
        raise ValueError('bin_weight: the 256 values must be finite and non-negative')
    return t.to(device)


def ce_opts_binned_fwd_bwd(logits, target, pixel_bin, bin_weight, class_weight=None, label_smoothing=0.0, focal_gamma=0.0,
                           keep_ratio=1.0, want_grad=True, ignore_index=-100):
    """ce_opts_fwd_bwd with the per-pixel weight bin_weight[pixel_bin] (pseg_ce_opts_binned_fwd_bwd): the per-pixel value,
    the divisor's terms and the gradient are scaled by it, and the selection ranks the scaled values.  pixel_bin: uint8
    [B, H, W] on the logits' device, contiguous itself but at any byte offset of its storage; bin_weight: fp32 [256] on that
    device, finite and non-negative (bin_weight_table checks and uploads).  Both are required: the call without them is
    ce_opts_fwd_bwd.  -> (out[6] = [loss, n_valid, n_out_of_range_targets, n_kept, tau, sum of the kept pixels' u * w], dlogits|None)."""
    B, C, H, W = _loss_operands(logits, target)
    if pixel_bin is None or bin_weight is None:
        raise ValueError('ce_opts_binned_fwd_bwd: pixel_bin and bin_weight come together (without them: ce_opts_fwd_bwd)')
    assert pixel_bin.device == logits.device and pixel_bin.dtype == torch.uint8 and pixel_bin.is_contiguous() and \
        pixel_bin.shape == (B, H, W), 'pixel_bin: contiguous uint8 %s on %s' % ((B, H, W), logits.device)
    assert bin_weight.device == logits.device and bin_weight.dtype == torch.float32 and bin_weight.is_contiguous() and \
        bin_weight.shape == (256,), 'bin_weight: 256 fp32 values on %s' % (logits.device,)
    _loss_class_weight(class_weight, logits)
    head = (logits.data_ptr(), target.data_ptr(), pixel_bin.data_ptr(), bin_weight.data_ptr(), B, C, H * W, ignore_index,
            _ptr(class_weight), float(label_smoothing), float(focal_gamma), float(keep_ratio))
    return _loss_call('pseg_ce_opts_binned_fwd_bwd', head, logits, want_grad, 6, ('pseg_ce_opts_workspace_bytes', B, C, H * W),
                      workspace)


# the Lovasz loss's sort buffers (hundreds of MiB at training sizes) get a cache of their own: allocated once per stream,
# and the small scratch every conv shares stays small
lovasz_workspace = _Workspace()


def lovasz_softmax_fwd_bwd(logits, target, want_grad=True, ignore_index=-100):
    """Lovasz-softmax loss over the present classes of the whole batch (pseg_lovasz_softmax_fwd_bwd).
    logits: contiguous NCHW fp32 cuda, target: NHW int64.
    -> (out[4] = [loss, n_valid, n_out_of_range_targets, n_present], dlogits|None)."""
    B, C, H, W = _loss_operands(logits, target)
    return _loss_call('pseg_lovasz_softmax_fwd_bwd', (logits.data_ptr(), target.data_ptr(), B, C, H * W, ignore_index), logits,
                      want_grad, 4, ('pseg_lovasz_workspace_bytes', B, C, H * W), lovasz_workspace)


def tversky_fwd_bwd(logits, target, alpha=0.5, beta=0.5, smooth=1.0, power=1.0, per_image=False, all_classes=False,
                    want_grad=True, ignore_index=-100, want_sums=False):
    """Soft Dice / Tversky / focal-Tversky loss over the softmax of the logits (pseg_tversky_fwd_bwd).
    logits: contiguous NCHW fp32 cuda, target: NHW int64.
    -> (out[5] = [loss, n_valid, n_out_of_range_targets, n_terms, n_groups_counted], dlogits|None), and with want_sums
    also class_sums: float64 [G, C, 3] = n_c, S_c, TP_c per group (G = B with per_image, else 1)."""
    B, C, H, W = _loss_operands(logits, target)
    sums = torch.empty(B if per_image else 1, C, 3, dtype=torch.float64, device=logits.device) if want_sums else None
    head = (logits.data_ptr(), target.data_ptr(), B, C, H * W, ignore_index, float(alpha), float(beta), float(smooth),
            float(power), int(bool(per_image)), int(bool(all_classes)))
    out, dl = _loss_call('pseg_tversky_fwd_bwd', head, logits, want_grad, 5, ('pseg_tversky_workspace_bytes', B, C, H * W),
                         workspace, tail=(_ptr(sums),))
    return (out, dl, sums) if want_sums else (out, dl)


def surface_fwd_bwd(logits, target, sdist, clip=0.0, want_grad=True, ignore_index=-100):
    """Kervadec's surface loss over the softmax of the logits (pseg_surface_fwd_bwd): the mean over the valid pixels of
    sum_c phi_c p_c, phi the signed distance sqrt(sdist) / -(sqrt(-sdist) - 1) / 0 limited to [-clip, clip] when clip > 0.
    logits: contiguous NCHW fp32 cuda, target: NHW int64, sdist: int32 NCHW = class_sdist(target, C).
    -> (out[3] = [loss, n_valid, n_out_of_range_targets], dlogits|None)."""
    B, C, H, W = _loss_operands(logits, target)
    assert sdist.device == logits.device and sdist.dtype == torch.int32 and sdist.is_contiguous() and \
        sdist.shape == logits.shape, 'sdist: contiguous int32 %s on %s' % (tuple(logits.shape), logits.device)
    head = (logits.data_ptr(), target.data_ptr(), sdist.data_ptr(), B, C, H * W, ignore_index, float(clip))
    return _loss_call('pseg_surface_fwd_bwd', head, logits, want_grad, 3, ('pseg_surface_workspace_bytes', B, C, H * W), workspace)


def ce_upsampled_ok_shape(h, w, C, H, W, align_corners):
    return bool(_lib.query('pseg_ce_upsampled_ok', h, w, C, H, W, int(align_corners)))


def ce_upsampled_ok(lr, C, H, W, align_corners):
    return ce_upsampled_ok_shape(lr.H, lr.W, C, H, W, align_corners)


def ce_upsampled_fwd_bwd(lr, C, target, align_corners, want_grad=True, ignore_index=-100):
    """CrossEntropy(interpolate(logits, target.shape[1:], 'bilinear', align_corners), target) straight from the LOW-resolution
    NHWC logits `lr` (first C channels): -> (loss_out[3], dlr | None) with dlr an Act shaped like lr (gradient with respect
    to the low-resolution logits; padded channels zero).  The full-resolution logits never exist."""
    assert target.dtype == torch.int64 and target.is_contiguous() and target.dim() == 3 and target.shape[0] == lr.B
    assert not lr.half, 'the loss reads fp32 logits (the classifier conv writes them in fp32 under the half policy)'
    H, W = int(target.shape[1]), int(target.shape[2])
    dlr = Act.empty(lr.B, lr.H, lr.W, lr.C, lr.device) if want_grad else None
    out = torch.empty(3, dtype=torch.float32, device=lr.device)
    nbytes = _lib.query('pseg_ce_upsampled_workspace_bytes', lr.B, lr.H, lr.W)
    ws = workspace.get(nbytes, lr.device)
    _lib.call('pseg_ce_upsampled_fwd_bwd', lr.ptr, lr.ld, lr.B, lr.H, lr.W, C, target.data_ptr(), H, W, int(align_corners),
              ignore_index, *_pl(dlr), out.data_ptr(),
              ws.data_ptr(), nbytes, _stream())
    return out, dlr


def scale_inplace(x, gscale):
    """x *= gscale (0-dim / 1-element device tensor); a no-op on the device when gscale == 1."""
    assert x.is_contiguous() and gscale.numel() == 1 and gscale.dtype == torch.float32
    _lib.call('pseg_scale_inplace', x.data_ptr(), x.numel(), gscale.data_ptr(), _stream())


def argmax(logits):
    assert logits.is_cuda and logits.dtype == torch.float32 and logits.is_contiguous() and logits.dim() == 4
    B, C, H, W = logits.shape
    mask = torch.empty(B, H, W, dtype=torch.int64, device=logits.device)
    _lib.call('pseg_argmax', logits.data_ptr(), B, C, H * W, mask.data_ptr(), _stream())
    return mask


def _image_preprocess(entry, words, src, table, oh, ow, mean, std, bgr, flag_mask=None):
    """the three preprocess entry points: table rows of `words` int64; flag_mask None: the entry point takes no flags"""
    assert src.is_cuda and src.dtype == torch.uint8 and src.is_contiguous() and src.dim() == 1
    assert table.device == src.device and table.dtype == torch.int64 and table.is_contiguous() and table.dim() == 2
    assert table.shape[1] == words and len(mean) == 3 and len(std) == 3
    R = table.shape[0]
    out = torch.empty(R, 3, oh, ow, dtype=torch.float32, device=src.device)
    flags = () if flag_mask is None else (int(flag_mask),)
    _lib.call(entry, src.data_ptr(), src.numel(), table.data_ptr(), R, *flags, int(bool(bgr)),
              *[float(m) for m in mean], *[float(v) for v in std], out.data_ptr(), oh, ow, _stream())
    return out


def _decode_out(dev, npix_total, lut, out):
    """the decode entry points' output: validates (or allocates) out and the lut -> (out, mask, rgb or None)"""
    nbytes = npix_total * (1 if lut is None else 4)
    if out is None:
        out = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    assert out.device == dev and out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == nbytes
    mask, rgb = out[:npix_total], None
    if lut is not None:
        assert lut.device == dev and lut.dtype == torch.uint8 and lut.is_contiguous() and lut.shape == (256, 3)
        rgb = out[npix_total:].view(npix_total, 3)
    return out, mask, rgb


def image_preprocess(src, table, oh, ow, mean, std, bgr):
    """Ragged batch of uint8 HWC photos -> fp32 NCHW model input [B,3,oh,ow] (pseg_image_preprocess).  src: flat uint8
    device tensor, photos back to back; table: int64 device tensor [B,3] of {byte offset, H, W} (validated by the caller)."""
    return _image_preprocess('pseg_image_preprocess', 3, src, table, oh, ow, mean, std, bgr)


def seg_decode(logits, table, npix_total, lut=None, out=None):
    """NCHW fp32 logits [B,C,h,w] -> per-image uint8 masks argmax_c(bilinear(softmax_c(logits))) at each image's own
    size (pseg_seg_decode), packed in one flat uint8 tensor of npix_total bytes at the offsets of table (int64 device
    tensor [B,3] of {pixel offset, H, W}); with lut (uint8 [256,3] on the device) also the flat [npix_total,3] colours.
    out (optional): one uint8 device tensor of npix_total (x 4 with lut) bytes that receives the mask, then the colours.
    -> (mask, rgb or None)."""
    assert logits.is_cuda and logits.dtype == torch.float32 and logits.is_contiguous() and logits.dim() == 4
    assert table.device == logits.device and table.dtype == torch.int64 and table.is_contiguous()
    assert table.shape == (logits.shape[0], 3)
    B, C, h, w = logits.shape
    out, mask, rgb = _decode_out(logits.device, npix_total, lut, out)
    _lib.call('pseg_seg_decode', logits.data_ptr(), B, C, h, w, table.data_ptr(), npix_total, mask.data_ptr(), _ptr(rgb),
              _ptr(lut), _stream())
    return mask, rgb


VIEW_MIRROR = 1         # PSEG_VIEW_MIRROR: flag bit of image_preprocess_views' table rows
ENSEMBLE_MAX_MAPS = 8   # probability maps one seg_decode_ensemble call sums


def class_pad(C):
    """Floats per pixel of a probability map (softmax_views / seg_decode_ensemble): 8 for C <= 8, else C rounded up to 4."""
    return 8 if C <= 8 else (C + 3) // 4 * 4


def image_preprocess_views(src, table, oh, ow, mean, std, bgr, flag_mask=VIEW_MIRROR):
    """image_preprocess with one flag word per table row (pseg_image_preprocess_views): table is an int64 device tensor
    [R,4] of {byte offset, H, W, flags}, several rows may name one photo, -> fp32 [R,3,oh,ow].  A row flagged VIEW_MIRROR
    is the unflagged result flipped along x, bit for bit; a row with flags 0 is image_preprocess's, bit for bit.
    flag_mask: the flag bits the rows use -- unknown bits are refused, rows with bits outside it are skipped."""
    return _image_preprocess('pseg_image_preprocess_views', 4, src, table, oh, ow, mean, std, bgr, flag_mask)


def softmax_views(logits, prob, offset, pairs=False):
    """NCHW fp32 logits [n,C,h,w] -> the probability map [B,h,w,class_pad(C)] (pixel-major, pad lanes 0) written into the
    flat fp32 device tensor prob at float offset `offset` (a multiple of 4) (pseg_softmax_views).  pairs: n = 2B, rows
    B..2B-1 are the logits of the mirrored inputs of rows 0..B-1; each is un-mirrored and added to its twin's softmax.
    -> the map as a [B,h,w,CP] view of prob."""
    assert logits.is_cuda and logits.dtype == torch.float32 and logits.is_contiguous() and logits.dim() == 4
    assert prob.device == logits.device and prob.dtype == torch.float32 and prob.is_contiguous() and prob.dim() == 1
    n, C, h, w = logits.shape
    assert not pairs or n % 2 == 0
    B = n // 2 if pairs else n
    CP = class_pad(C)
    _lib.call('pseg_softmax_views', logits.data_ptr(), B, int(bool(pairs)), C, h, w, prob.data_ptr(), int(offset), prob.numel(),
              _stream())
    return prob[offset:offset + B * h * w * CP].view(B, h, w, CP)


def seg_decode_ensemble(prob, maps, B, C, table, npix_total, max_hw, lut=None, out=None):
    """Per-image uint8 masks argmax_c sum_s bilinear(map_s, (H, W)) (pseg_seg_decode_ensemble), first index on ties.  prob:
    the flat fp32 device tensor softmax_views filled; maps: int64 device tensor [S,3] of {float offset, h_s, w_s}, S <=
    ENSEMBLE_MAX_MAPS; table: int64 device tensor [B,3] of {pixel offset, H, W}; max_hw = (largest H, largest W) of the
    table (it sizes the grid; larger images are skipped).  npix_total, lut, out and the result are seg_decode's."""
    assert prob.is_cuda and prob.dtype == torch.float32 and prob.is_contiguous() and prob.dim() == 1
    assert maps.device == prob.device and maps.dtype == torch.int64 and maps.is_contiguous()
    assert maps.dim() == 2 and maps.shape[1] == 3
    assert table.device == prob.device and table.dtype == torch.int64 and table.is_contiguous() and table.shape == (B, 3)
    out, mask, rgb = _decode_out(prob.device, npix_total, lut, out)
    _lib.call('pseg_seg_decode_ensemble', prob.data_ptr(), prob.numel(), maps.data_ptr(), maps.shape[0], B, C, table.data_ptr(),
              npix_total, int(max_hw[0]), int(max_hw[1]), mask.data_ptr(), _ptr(rgb), _ptr(lut), _stream())
    return mask, rgb


WINDOW_STRIDE = (2, 3)  # default stride of sliding windows: ceil(2/3 of the window) along each axis


def window_stride_limits(win):
    """(smallest, largest, default) stride of sliding windows of `win` pixels along one axis: ceil(win/2) <= stride <=
    win, so that a pixel is covered by at most 3 windows per axis; default ceil(win * WINDOW_STRIDE)."""
    num, den = WINDOW_STRIDE
    return (win + 1) // 2, win, (num * win + den - 1) // den


def image_preprocess_windows(src, table, oh, ow, mean, std, bgr, flag_mask=VIEW_MIRROR):
    """image_preprocess_views whose output rows are windows (pseg_image_preprocess_windows): table is an int64 device
    tensor [R,8] of {byte offset, H, W, flags, Hs, Ws, y0, x0}, -> fp32 [R,3,oh,ow] with out[r,c,y,x] = the normalised
    value at (y0 + y, x0 + x) of the photo resampled to Hs x Ws, 0.0 beyond it.  A row {.., flags, oh, ow, 0, 0} is
    image_preprocess_views' row, bit for bit; a window is the crop of the whole working image, bit for bit.  Rows whose
    photo leaves src, with Hs / Ws outside [1, 65535], an origin outside the working image or flag bits outside flag_mask
    are skipped."""
    return _image_preprocess('pseg_image_preprocess_windows', 8, src, table, oh, ow, mean, std, bgr, flag_mask)


def seg_decode_windows(prob, groups, B, C, window_hw, stride_hw, table, npix_total, max_hw, lut=None, out=None):
    """Per-image uint8 masks argmax_c sum_s bilinear(P_s, (H, W)) (pseg_seg_decode_windows), P_s being the unweighted mean
    of the probability maps of the sliding windows that cover a working-image pixel; first index on ties.  prob: the flat
    fp32 device tensor softmax_views filled; groups: int64 device tensor [S,B,3] of {float offset, Hs, Ws}, S <=
    ENSEMBLE_MAX_MAPS, the group of photo b at scale s being [ny*nx, h, w, class_pad(C)] in window order (i*nx + j);
    window_hw = (h, w), stride_hw = (sy, sx) within window_stride_limits.  table, npix_total, max_hw, lut, out and the
    result are seg_decode_ensemble's.  A photo with a bad table or group record is not written."""
    assert prob.is_cuda and prob.dtype == torch.float32 and prob.is_contiguous() and prob.dim() == 1
    assert groups.device == prob.device and groups.dtype == torch.int64 and groups.is_contiguous()
    assert groups.dim() == 3 and groups.shape[1:] == (B, 3)
    assert table.device == prob.device and table.dtype == torch.int64 and table.is_contiguous() and table.shape == (B, 3)
    out, mask, rgb = _decode_out(prob.device, npix_total, lut, out)
    _lib.call('pseg_seg_decode_windows', prob.data_ptr(), prob.numel(), groups.data_ptr(), groups.shape[0], B, C,
              int(window_hw[0]), int(window_hw[1]), int(stride_hw[0]), int(stride_hw[1]), table.data_ptr(), npix_total,
              int(max_hw[0]), int(max_hw[1]), mask.data_ptr(), _ptr(rgb), _ptr(lut), _stream())
    return mask, rgb


REGIONS_TILE = 32       # PSEG_REGIONS_TILE: tile edge of mask_label's LDS union-find (tiles start at the photo's corner)
REGION_WORDS = 12       # PSEG_REGION_WORDS: int64 per record of mask_regions (layout: include/pseg_amd.h)
REGIONS_MAX_LARGEST_BATCH = 4096   # PSEG_REGIONS_MAX_LARGEST_BATCH: photos per mask_clean call with largest_only

# the regions calls' scratch (5 bytes per mask pixel): its own buffer, like the Lovasz loss's
regions_workspace = _Workspace()


def _regions_args(mask, table, npix_total, max_hw):
    assert mask.is_cuda and mask.dtype == torch.uint8 and mask.is_contiguous() and mask.dim() == 1
    assert mask.numel() == npix_total
    assert table.device == mask.device and table.dtype == torch.int64 and table.is_contiguous()
    assert table.dim() == 2 and table.shape[1] == 3
    Hmax, Wmax = int(max_hw[0]), int(max_hw[1])
    nbytes = _lib.query('pseg_regions_workspace_bytes', int(npix_total), 0)
    assert nbytes >= 0, 'npix_total %d out of range' % npix_total
    return table.shape[0], Hmax, Wmax, nbytes, regions_workspace.get(nbytes, mask.device)


def mask_label(mask, table, npix_total, max_hw, connectivity=8, out=None):
    """Connected-component labels of a packed batch of uint8 masks (pseg_mask_label).  mask: flat uint8 device tensor of
    npix_total pixels; table: int64 device tensor [B,3] of {pixel offset, H, W}; max_hw = (largest H, largest W) of the
    table.  -> int32 tensor [npix_total]: at each pixel, y*W + x of the first pixel (raster order) of its component, within
    its own photo.  connectivity: 4 or 8.  Words outside every valid record are left as they are (out) or undefined."""
    B, Hmax, Wmax, nbytes, ws = _regions_args(mask, table, npix_total, max_hw)
    if out is None:
        out = torch.empty(npix_total, dtype=torch.int32, device=mask.device)
    assert out.device == mask.device and out.dtype == torch.int32 and out.is_contiguous() and out.numel() == npix_total
    _lib.call('pseg_mask_label', mask.data_ptr(), table.data_ptr(), B, npix_total, Hmax, Wmax, int(connectivity),
              out.data_ptr(), ws.data_ptr(), nbytes, _stream())
    return out


def mask_regions(mask, labels, table, npix_total, max_hw, max_regions, records=None, count=None):
    """One record of REGION_WORDS int64 per component, in (photo, label) order (pseg_mask_regions; word layout in
    include/pseg_amd.h).  -> (records int64 [max_regions, REGION_WORDS], count int64 [1]): count is the full number of
    components, only the first min(count, max_regions) records are written.  No host synchronisation: read count yourself."""
    B, Hmax, Wmax, nbytes, ws = _regions_args(mask, table, npix_total, max_hw)
    assert labels.device == mask.device and labels.dtype == torch.int32 and labels.is_contiguous() and labels.numel() == npix_total
    max_regions = int(max_regions)
    assert max_regions >= 0
    if records is None:
        records = torch.empty(max_regions, REGION_WORDS, dtype=torch.int64, device=mask.device)
    if count is None:
        count = torch.empty(1, dtype=torch.int64, device=mask.device)
    assert records.device == mask.device and records.dtype == torch.int64 and records.is_contiguous()
    assert records.numel() >= max_regions * REGION_WORDS
    assert count.device == mask.device and count.dtype == torch.int64 and count.numel() >= 1
    _lib.call('pseg_mask_regions', mask.data_ptr(), labels.data_ptr(), table.data_ptr(), B, npix_total, Hmax, Wmax, max_regions,
              records.data_ptr() if max_regions else 0, count.data_ptr(), ws.data_ptr(), nbytes, _stream())
    return records, count


def mask_clean(mask, labels, table, npix_total, max_hw, min_area=0, largest_only=False, lut=None, out=None):
    """Drop the small components of a labelled packed mask (pseg_mask_clean): a component below min_area pixels -- and, with
    largest_only, every component of a class >= 1 but the largest of its class in its photo -- takes the class of the
    region above (in the top row: left of) its first pixel, followed through further small components.  out (optional):
    one uint8 device tensor of npix_total (x 4 with lut) bytes for the cleaned mask, then its colours, as seg_decode's;
    it may start at mask's own storage (in place).  -> (mask_out, rgb or None)."""
    B, Hmax, Wmax, nbytes, ws = _regions_args(mask, table, npix_total, max_hw)
    assert labels.device == mask.device and labels.dtype == torch.int32 and labels.is_contiguous() and labels.numel() == npix_total
    if int(min_area) < 0:
        raise ValueError('min_area must be >= 0; got %r' % (min_area,))
    total = npix_total * (1 if lut is None else 4)
    if out is None:
        out = torch.empty(total, dtype=torch.uint8, device=mask.device)
    assert out.device == mask.device and out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == total
    mask_out, rgb = out[:npix_total], None
    if lut is not None:
        assert lut.device == mask.device and lut.dtype == torch.uint8 and lut.is_contiguous() and lut.shape == (256, 3)
        rgb = out[npix_total:].view(npix_total, 3)
    _lib.call('pseg_mask_clean', mask.data_ptr(), labels.data_ptr(), table.data_ptr(), B, npix_total, Hmax, Wmax, int(min_area),
              int(bool(largest_only)), mask_out.data_ptr(), _ptr(rgb), _ptr(lut), ws.data_ptr(), nbytes, _stream())
    return mask_out, rgb


RING_WORDS = 6          # PSEG_RING_WORDS: int64 per record of mask_rings (layout: include/pseg_amd.h)

# the rings call's scratch (5 bytes per mask pixel, 37 per edge of capacity): its own buffer, like the regions calls'
rings_workspace = _Workspace()


def mask_rings(mask, labels, table, npix_total, max_hw, connectivity, max_edges, rings=None, vertices=None, counts=None):
    """The outlines of the components of a labelled packed mask as closed rings of lattice vertices (pseg_mask_rings;
    definitions and record layout in include/pseg_amd.h).  labels: mask_label's result for the same connectivity.
    -> (rings int64 [max_edges // 4, RING_WORDS], vertices int32 [max_edges, 2], counts int64 [3] = edges, rings,
    vertices).  If counts[0] > max_edges nothing is written and counts[1] = counts[2] = -1: repeat with max_edges =
    counts[0].  No host synchronisation: read counts yourself."""
    assert mask.is_cuda and mask.dtype == torch.uint8 and mask.is_contiguous() and mask.dim() == 1
    assert mask.numel() == npix_total
    assert table.device == mask.device and table.dtype == torch.int64 and table.is_contiguous()
    assert table.dim() == 2 and table.shape[1] == 3
    assert labels.device == mask.device and labels.dtype == torch.int32 and labels.is_contiguous() and labels.numel() == npix_total
    Hmax, Wmax = int(max_hw[0]), int(max_hw[1])
    max_edges = int(max_edges)
    nbytes = _lib.query('pseg_mask_rings_workspace_bytes', int(npix_total), max_edges)
    assert nbytes >= 0, 'npix_total %d or max_edges %d out of range' % (npix_total, max_edges)
    ws = rings_workspace.get(nbytes, mask.device)
    if rings is None:
        rings = torch.empty(max_edges // 4, RING_WORDS, dtype=torch.int64, device=mask.device)
    if vertices is None:
        vertices = torch.empty(max_edges, 2, dtype=torch.int32, device=mask.device)
    if counts is None:
        counts = torch.empty(3, dtype=torch.int64, device=mask.device)
    assert rings.device == mask.device and rings.dtype == torch.int64 and rings.is_contiguous()
    assert rings.numel() >= max_edges // 4 * RING_WORDS
    assert vertices.device == mask.device and vertices.dtype == torch.int32 and vertices.is_contiguous()
    assert vertices.numel() >= 2 * max_edges
    assert counts.device == mask.device and counts.dtype == torch.int64 and counts.is_contiguous() and counts.numel() >= 3
    _lib.call('pseg_mask_rings', mask.data_ptr(), labels.data_ptr(), table.data_ptr(), table.shape[0], npix_total, Hmax, Wmax,
              int(connectivity), max_edges, rings.data_ptr() if max_edges else 0, vertices.data_ptr() if max_edges else 0,
              counts.data_ptr(), ws.data_ptr(), nbytes, _stream())
    return rings, vertices, counts


# the CRF's two ping-pong buffers of Q (pixel-major [B,h,w,class_pad(C)]): its own buffer, kept per stream while the
# shape does not grow
crf_workspace = _Workspace()


def crf_refine(logits, guide, guide_scale, radius, dilation, iters, theta_alpha, theta_beta, theta_gamma, w_appearance, w_smooth,
               out=None):
    """Local dense-CRF refinement of logits (pseg_crf_refine; definition in include/pseg_amd.h): fp32 NCHW logits
    [B,C,h,w] and guide [B,3,h,w] (the model input; guide_scale = the std of its normalisation) -> fp32 NCHW L^T, whose
    softmax is the refined distribution.  out (optional) may be logits itself.  Every range is checked by the library
    before any launch (PsegError)."""
    assert logits.is_cuda and logits.dtype == torch.float32 and logits.is_contiguous() and logits.dim() == 4
    assert guide.device == logits.device and guide.dtype == torch.float32 and guide.is_contiguous()
    B, C, h, w = logits.shape
    assert guide.shape == (B, 3, h, w), 'crf_refine: guide %s for logits %s' % (tuple(guide.shape), tuple(logits.shape))
    assert len(guide_scale) == 3
    if out is None:
        out = torch.empty_like(logits)
    assert out.device == logits.device and out.dtype == torch.float32 and out.is_contiguous() and out.shape == logits.shape
    nbytes = _lib.query('pseg_crf_workspace_bytes', B, C, h, w)
    # (a shape the query refuses goes to the call with an empty workspace: the call names the argument that is wrong)
    ws = crf_workspace.get(max(nbytes, 0), logits.device)
    _lib.call('pseg_crf_refine', logits.data_ptr(), guide.data_ptr(), B, C, h, w, *[float(g) for g in guide_scale], int(radius),
              int(dilation), int(iters), float(theta_alpha), float(theta_beta), float(theta_gamma), float(w_appearance),
              float(w_smooth), out.data_ptr(), ws.data_ptr(), max(nbytes, 0), _stream())
    return out


AUGMENT_ROW = 24       # PSEG_AUGMENT_ROW: floats per sample of augment_batch's parameter table (layout: include/pseg_amd.h)


def augment_batch(imgs, segs, params, oh, ow, mean, std, out=None, target=None):
    """The collated uint8 batch -> (fp32 model input [B,3,oh,ow], int64 targets [B,H,W]) in one launch (pseg_augment_batch):
    per-sample inverse affine warp + 3x4 colour matrix + normalisation + multi-scale nearest resize for the images, the
    same warp with a nearest sample for the labels.  imgs: uint8 [B,3,H,W] planar RGB, segs: uint8 [B,H,W], params: fp32
    device table [B, AUGMENT_ROW].  out / target (optional): contiguous device tensors of exactly those shapes to write into."""
    assert imgs.is_cuda and imgs.dtype == torch.uint8 and imgs.is_contiguous() and imgs.dim() == 4 and imgs.shape[1] == 3
    B, _, H, W = imgs.shape
    assert segs.device == imgs.device and segs.dtype == torch.uint8 and segs.is_contiguous() and segs.shape == (B, H, W)
    assert params.device == imgs.device and params.dtype == torch.float32 and params.is_contiguous()
    assert params.shape == (B, AUGMENT_ROW) and len(mean) == 3 and len(std) == 3
    if out is None:
        out = torch.empty(B, 3, oh, ow, dtype=torch.float32, device=imgs.device)
    if target is None:
        target = torch.empty(B, H, W, dtype=torch.int64, device=imgs.device)
    assert out.device == imgs.device and out.dtype == torch.float32 and out.is_contiguous() and out.shape == (B, 3, oh, ow)
    assert target.device == imgs.device and target.dtype == torch.int64 and target.is_contiguous() and target.shape == (B, H, W)
    _lib.call('pseg_augment_batch', imgs.data_ptr(), segs.data_ptr(), params.data_ptr(), B, H, W, *[float(m) for m in mean],
              *[float(v) for v in std], out.data_ptr(), oh, ow, target.data_ptr(), _stream())
    return out, target


AUGMENT_NBHD_ROW = 212  # PSEG_AUGMENT_NBHD_ROW: floats per sample of augment_batch_nbhd's table (layout: include/pseg_amd.h)
AUGMENT_NBHD_KMAX = 13  # PSEG_AUGMENT_NBHD_KMAX


def _augment_batch_wide(entry, row, imgs, segs, params, shapes, oh, ow, mean, std, out, target, cols=3):
    assert imgs.is_cuda and imgs.dtype == torch.uint8 and imgs.is_contiguous() and imgs.dim() == 4 and imgs.shape[1] == 3
    B, _, H, W = imgs.shape
    assert segs.device == imgs.device and segs.dtype == torch.uint8 and segs.is_contiguous() and segs.shape == (B, H, W)
    assert params.device == imgs.device and params.dtype == torch.float32 and params.is_contiguous()
    assert params.shape == (B, row) and len(mean) == 3 and len(std) == 3
    assert not shapes.is_cuda and shapes.dtype == torch.int32 and shapes.is_contiguous() and shapes.shape == (B, cols)
    if out is None:
        out = torch.empty(B, 3, oh, ow, dtype=torch.float32, device=imgs.device)
    if target is None:
        target = torch.empty(B, H, W, dtype=torch.int64, device=imgs.device)
    assert out.device == imgs.device and out.dtype == torch.float32 and out.is_contiguous() and out.shape == (B, 3, oh, ow)
    assert target.device == imgs.device and target.dtype == torch.int64 and target.is_contiguous() and target.shape == (B, H, W)
    _lib.call(entry, imgs.data_ptr(), segs.data_ptr(), params.data_ptr(), shapes.data_ptr(), B, H, W,
              *[float(m) for m in mean], *[float(v) for v in std], out.data_ptr(), oh, ow, target.data_ptr(), _stream())
    return out, target


def augment_batch_nbhd(imgs, segs, params, shapes, oh, ow, mean, std, out=None, target=None):
    """augment_batch with a K x K filter, Gaussian noise and (coarse) dropout per sample, in one launch
    (pseg_augment_batch_nbhd).  params: fp32 device table [B, AUGMENT_NBHD_ROW]; shapes: HOST int32 tensor [B, 3] of each
    row's {K, mh, mw}, which the library validates and sizes its LDS tile from.  Everything else as augment_batch."""
    return _augment_batch_wide('pseg_augment_batch_nbhd', AUGMENT_NBHD_ROW, imgs, segs, params, shapes, oh, ow, mean, std, out, target)


AUGMENT_WARP_ROW = 252  # PSEG_AUGMENT_WARP_ROW: floats per sample of augment_batch_warp's table (layout: include/pseg_amd.h)


def augment_batch_warp(imgs, segs, params, shapes, oh, ow, mean, std, out=None, target=None):
    """augment_batch_nbhd with a per-sample elastic jitter, 4 x 4 displacement grid and inverse homography in the coordinate
    map of images and labels, in one launch (pseg_augment_batch_warp).  params: fp32 device table [B, AUGMENT_WARP_ROW];
    everything else as augment_batch_nbhd."""
    return _augment_batch_wide('pseg_augment_batch_warp', AUGMENT_WARP_ROW, imgs, segs, params, shapes, oh, ow, mean, std, out, target)


AUGMENT_BLEND_ROW = 1012  # PSEG_AUGMENT_BLEND_ROW: floats per sample of augment_batch_blend's table (layout: include/pseg_amd.h)
AUGMENT_BLEND_KMEDMAX = 11  # PSEG_AUGMENT_BLEND_KMEDMAX
AUGMENT_BLEND_K2MAX = 15    # PSEG_AUGMENT_BLEND_K2MAX


def augment_batch_blend(imgs, segs, params, shapes, oh, ow, mean, std, out=None, target=None):
    """augment_batch_warp with a per-sample median window, a second filter and a second colour matrix blended in by two
    16 x 16 mask tables, and a hue / saturation shift, in one launch (pseg_augment_batch_blend).  params: fp32 device table
    [B, AUGMENT_BLEND_ROW]; shapes: HOST int32 tensor [B, 5] of each row's {K, mh, mw, kmed, K2}; everything else as
    augment_batch_warp."""
    return _augment_batch_wide('pseg_augment_batch_blend', AUGMENT_BLEND_ROW, imgs, segs, params, shapes, oh, ow, mean, std, out, target,
                               cols=5)


def confusion(pred, target, counters):
    """counters: int64 [3][C] (tp, fn, fp), accumulated in place."""
    assert pred.dtype == torch.int64 and target.dtype == torch.int64 and counters.dtype == torch.int64
    assert pred.is_contiguous() and target.is_contiguous() and counters.is_contiguous() and counters.shape[0] == 3
    _lib.call('pseg_confusion', pred.data_ptr(), target.data_ptr(), pred.numel(), counters.shape[1],
              counters.data_ptr(), _stream())


BOUNDARY_MAX_WIDTH = 254     # the clipped depth d + 1 fits a byte
BOUNDARY_ROWS = 6            # inter, gband, pband, trimap tp / fn / fp (layout: include/pseg_amd.h)

# the boundary counters' scratch (one byte per pixel and map): its own buffer, like the regions calls'
boundary_workspace = _Workspace()


def _label_map(name, t):
    if not t.is_cuda:
        raise RuntimeError('%s runs on the HIP path only (got %s)' % (name, t.device))
    assert t.dtype == torch.int64 and t.is_contiguous() and t.dim() == 3, \
        '%s takes contiguous int64 [B, H, W] label maps (got %s %s)' % (name, t.dtype, tuple(t.shape))
    assert t.numel() > 0, '%s: empty label map %s' % (name, tuple(t.shape))


def label_depth(labels, num_classes, d, edge=False):
    """Clipped Chebyshev distance of every pixel to the nearest pixel of its own image that carries a different label
    (pseg_label_depth): labels int64 [B, H, W] -> uint8 [B, H, W] with values 1 .. d + 1, d + 1 standing for "none within
    d".  Labels outside [0, num_classes) are void and compare by value.  edge: the outside of the image counts as a
    different label (depth_edge)."""
    _label_map('label_depth', labels)
    B, H, W = labels.shape
    out = torch.empty(B, H, W, dtype=torch.uint8, device=labels.device)
    _lib.call('pseg_label_depth', labels.data_ptr(), B, H, W, int(num_classes), int(d), int(bool(edge)), out.data_ptr(), _stream())
    return out


def boundary_counts(pred, target, counters, d):
    """counters: int64 [6][C] (Boundary IoU's inter / gband / pband of width d, then the trimap's tp / fn / fp), accumulated
    in place (pseg_boundary_counts).  pred, target: int64 [B, H, W]; a prediction pixel counts as void where its target is."""
    _label_map('boundary_counts', pred)
    _label_map('boundary_counts', target)
    assert pred.shape == target.shape and pred.device == target.device, 'boundary_counts: pred %s / target %s' % (
        tuple(pred.shape), tuple(target.shape))
    assert counters.device == pred.device and counters.dtype == torch.int64 and counters.is_contiguous()
    assert counters.dim() == 2 and counters.shape[0] == BOUNDARY_ROWS, 'boundary_counts: counters are int64 [6][C]'
    B, H, W = pred.shape
    nbytes = _lib.query('pseg_boundary_counts_workspace_bytes', B, H, W, int(d))
    if nbytes < 0:
        raise ValueError('boundary_counts: shape %s or width d = %d out of range (1 <= d <= %d)'
                         % (tuple(pred.shape), d, BOUNDARY_MAX_WIDTH))
    ws = boundary_workspace.get(nbytes, pred.device)
    _lib.call('pseg_boundary_counts', pred.data_ptr(), target.data_ptr(), B, H, W, counters.shape[1], int(d),
              counters.data_ptr(), ws.data_ptr(), nbytes, _stream())


SDIST_MAX_SIDE = 16384       # H^2 + W^2 of class_sdist fits 2^29

# the distance transform's packed labels (two bytes per pixel): a buffer of its own, like the boundary counters'
sdist_workspace = _Workspace()


def class_sdist(labels, num_classes):
    """Exact signed squared Euclidean distance of every pixel to the contour of every class (pseg_class_sdist): labels int64
    [B, H, W] -> int32 [B, num_classes, H, W], +|p - q|^2 to the nearest pixel q of the class outside it, -|p - q|^2 to the
    nearest pixel of another label (void included) inside it, and a plane of zeros for a class that is absent from its image
    or fills it.  The image border is not a contour."""
    _label_map('class_sdist', labels)
    B, H, W = labels.shape
    C = int(num_classes)
    nbytes = _lib.query('pseg_class_sdist_workspace_bytes', B, C, H, W)
    if nbytes <= 0:
        raise ValueError('class_sdist: shape %s x %d classes out of range (H, W <= %d, 1 <= C <= 1024, the int32 result below '
                         '2 GiB)' % (tuple(labels.shape), C, SDIST_MAX_SIDE))
    out = torch.empty(B, C, H, W, dtype=torch.int32, device=labels.device)
    ws = sdist_workspace.get(nbytes, labels.device)
    _lib.call('pseg_class_sdist', labels.data_ptr(), B, H, W, C, out.data_ptr(), ws.data_ptr(), nbytes, _stream())
    return out


# the surface-distance records' planes, border maps and histograms: a buffer of its own, like the distance transform's
hausdorff_workspace = _Workspace()
HAUSDORFF_MAX_IMAGES = None  # images per call of hausdorff_stats; None: as many as the workspace query accepts (tests force chunks)


def hausdorff_stats(pred, target, num_classes, permille=950, tol=2):
    """The surface-distance record of every image and class (pseg_hausdorff_stats): pred, target int64 [B, H, W] ->
    (stats int64 [B, C, 8], sums float64 [B, C, 2]): the sizes of the two borders, the maximum, the nearest-rank permille
    quantile and the number within tol pixels of the squared border-to-border distances in either direction, and the sums of
    the distances (layout: include/pseg_amd.h).  Records are per image, so a batch that the workspace query refuses is walked
    in chunks of images; only a single image that is refused raises."""
    _label_map('hausdorff_stats', pred)
    _label_map('hausdorff_stats', target)
    assert pred.shape == target.shape and pred.device == target.device, 'hausdorff_stats: pred %s / target %s' % (
        tuple(pred.shape), tuple(target.shape))
    B, H, W = pred.shape
    C, permille, tol = int(num_classes), int(permille), int(tol)
    if not 1 <= permille <= 1000:
        raise ValueError('hausdorff_stats: permille must be in [1, 1000]; got %d' % permille)
    if not 0 <= tol <= 255:
        raise ValueError('hausdorff_stats: tol must be in [0, 255]; got %d' % tol)
    n = B if HAUSDORFF_MAX_IMAGES is None else max(1, min(B, int(HAUSDORFF_MAX_IMAGES)))
    while n > 1 and _lib.query('pseg_hausdorff_workspace_bytes', n, C, H, W) <= 0:
        n = (n + 1) // 2
    if _lib.query('pseg_hausdorff_workspace_bytes', n, C, H, W) <= 0:
        raise ValueError('hausdorff_stats: an image of %d x %d with %d classes is out of range (H, W <= %d, 1 <= C <= 1024, '
                         'the planes of one image below 2 GiB)' % (H, W, C, SDIST_MAX_SIDE))
    stats = torch.empty(B, C, 8, dtype=torch.int64, device=pred.device)
    sums = torch.empty(B, C, 2, dtype=torch.float64, device=pred.device)
    for b0 in range(0, B, n):
        nb = min(n, B - b0)
        nbytes = _lib.query('pseg_hausdorff_workspace_bytes', nb, C, H, W)
        ws = hausdorff_workspace.get(nbytes, pred.device)
        _lib.call('pseg_hausdorff_stats', pred[b0:b0 + nb].data_ptr(), target[b0:b0 + nb].data_ptr(), nb, H, W, C, permille, tol,
                  stats[b0:b0 + nb].data_ptr(), sums[b0:b0 + nb].data_ptr(), ws.data_ptr(), nbytes, _stream())
    return stats, sums


# ---------------------------------------------------------------------------------------------- optimiser
def sgd_step(param, grad, mbuf, lr, momentum, weight_decay, nesterov, grad_scale, first_step):
    _lib.call('pseg_sgd_step', param.data_ptr(), grad.data_ptr(), _ptr(mbuf), param.numel(), float(lr), float(momentum),
              float(weight_decay), int(nesterov), float(grad_scale), int(first_step), _stream())


def adam_step(param, grad, m, v, lr, beta1, beta2, eps, weight_decay, decoupled, grad_scale, step):
    _lib.call('pseg_adam_step', param.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), param.numel(), float(lr),
              float(beta1), float(beta2), float(eps), float(weight_decay), int(decoupled), float(grad_scale), int(step),
              _stream())


def fill(x, value):
    _lib.call('pseg_fill', x.data_ptr(), x.numel(), float(value), _stream())
