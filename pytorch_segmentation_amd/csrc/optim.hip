// Fused optimiser steps over the flat parameter arena (one launch for the whole model) on gfx950.
// The reference delegates the update to pytorch_modules.utils.Trainer (train.py:61-72) with torch.optim
// semantics selected by the --adam flag (train.py:94); these kernels follow torch.optim.SGD / Adam(W)
// element for element.  grad_scale folds the data-parallel mean (1/world) and 1/accumulate into the same pass.
#include "common.h"

#include <math.h>

namespace pseg {

__global__ __launch_bounds__(256) void fill_kernel(float* __restrict__ x, long long n, float value) {
  const long long n4 = n / 4;
  const f32x4 v4 = {value, value, value, value};
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256)
    *reinterpret_cast<f32x4*>(x + i * 4) = v4;
  if (blockIdx.x == 0 && threadIdx.x < n - n4 * 4) x[n4 * 4 + threadIdx.x] = value;
}

// max |x| of an [M][C] block with row stride ld, published as the bit pattern of the (non-negative) float via atomicMax
// (unsigned order == float order for non-negative values): what the fp16-limb conv kernels scale their operands by.
__global__ __launch_bounds__(256) void amax_kernel(const float* __restrict__ x, long long ld, long long M, int C,
                                                   unsigned* __restrict__ out) {
  const long long total = M * C;
  float m = 0.f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long r = i / C;
    m = fmaxf(m, fabsf(x[r * ld + (i - r * C)]));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0) publish_amax(out, m);
}

// every filter of a model in ONE launch: jobs[j] = {address of the floats, count, first block of job j}; out[j] = max|x|
// (overwritten, not accumulated: each block first reduces to one value, block 0 of a job zeroes nothing -- the outputs
// are zeroed by the same launch's predecessor memset on the host side)
__global__ __launch_bounds__(256) void amax_batch_kernel(const long long* __restrict__ jobs, int n, unsigned* __restrict__ out) {
  const long long b = blockIdx.x;
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[mid * 3 + 2] <= b) lo = mid;
    else hi = mid - 1;
  }
  const float* x = reinterpret_cast<const float*>(jobs[lo * 3]);
  const long long cnt = jobs[lo * 3 + 1];
  const long long first = jobs[lo * 3 + 2];
  const long long nblk = (lo + 1 < n ? jobs[(lo + 1) * 3 + 2] : (long long)gridDim.x) - first;
  float m = 0.f;
  for (long long i = (b - first) * 256 + threadIdx.x; i < cnt; i += nblk * 256) m = fmaxf(m, fabsf(x[i]));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0) publish_amax(out + lo, m);
}

// ------------------------------------------------------------------------------------------------ mixed precision (`-mp`)
// Dynamic loss scaling as apex / torch.cuda.amp do it (the reference's -mp, train.py:102-105), with the whole protocol on
// the device so that a step never synchronises the host and stays graph-capturable:
//   state[0] loss scale S (multiplies the loss gradient on its way into fp16, pseg_convert2d)   state[1] 1 / S
//   state[2] optimiser steps since the scale last changed                                       state[3] found-inf flag of this step
//   state[4] optimiser steps applied so far (Adam bias correction, SGD first-step)              state[5] steps skipped so far
// pseg_mp_check raises state[3] when any gradient is inf / nan; the optimiser kernels read it -- a flagged step changes
// nothing -- and fold 1 / S into grad_scale; pseg_mp_update then halves S after a flagged step, doubles it after
// growth_interval clean ones, and clears the flag.
constexpr int kMpScale = 0, kMpInv = 1, kMpTracker = 2, kMpFound = 3, kMpSteps = 4, kMpSkipped = 5;

__global__ __launch_bounds__(256) void mp_check_kernel(const float* __restrict__ g, long long n, float* __restrict__ state) {
  const long long n4 = n / 4;
  bool bad = false;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(g + i * 4);
    // (x - x is 0 for finite x and nan for inf / nan)
    const float t = (v[0] - v[0]) + (v[1] - v[1]) + (v[2] - v[2]) + (v[3] - v[3]);
    bad = bad || !(t == 0.f);
  }
  if (blockIdx.x == 0 && threadIdx.x < n - n4 * 4) {
    const float v = g[n4 * 4 + threadIdx.x];
    bad = bad || !(v - v == 0.f);
  }
  if (__any(bad) && (threadIdx.x & 63) == 0) state[kMpFound] = 1.f;     // (every writer stores the same value)
}

__global__ void mp_update_kernel(float* __restrict__ state, float growth, float backoff, int interval, float min_scale,
                                 float max_scale) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  float s = state[kMpScale];
  if (state[kMpFound] != 0.f) {
    s = fmaxf(s * backoff, min_scale);
    state[kMpTracker] = 0.f;
    state[kMpSkipped] += 1.f;
  } else {
    state[kMpSteps] += 1.f;
    float t = state[kMpTracker] + 1.f;
    if (t >= (float)interval) {
      s = fminf(s * growth, max_scale);
      t = 0.f;
    }
    state[kMpTracker] = t;
  }
  state[kMpScale] = s;
  state[kMpInv] = 1.f / s;
  state[kMpFound] = 0.f;
}

__global__ void mp_init_kernel(float* __restrict__ state, float scale) {
  if (threadIdx.x < 8) {
    float v = 0.f;
    if (threadIdx.x == kMpScale) v = scale;
    if (threadIdx.x == kMpInv) v = 1.f / scale;
    state[threadIdx.x] = v;
  }
}

// ------------------------------------------------------------------------------------------------ gradient norm
constexpr int kClipNorm = 0, kClipCoef = 1, kClipEff = 2, kClipCount = 3;

// sum of squares in fp64: every thread adds its grid-stride share in index order, the block folds 256 values through LDS
// in a fixed tree, one partial per block; a second single-block launch folds the partials the same way.  The grid depends
// on n only and no atomic is involved: the result is the same bits from call to call.
__device__ __forceinline__ double block_sum_f64(double v, double* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  return sh[0];
}

__global__ __launch_bounds__(256) void sumsq_partial_kernel(const float* __restrict__ g, long long n4,
                                                            double* __restrict__ part) {
  __shared__ double sh[256];
  double s = 0.0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(g + i * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const double x = (double)v[e];
      s += x * x;
    }
  }
  s = block_sum_f64(s, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void sumsq_final_kernel(const double* __restrict__ part, int nparts,
                                                          float* __restrict__ clip_state) {
  __shared__ double sh[256];
  double s = 0.0;
  // thread t owns the partials [t * per, (t + 1) * per): index order inside a thread, fixed tree across threads
  const int per = (nparts + 255) / 256;
  for (int k = 0; k < per; ++k) {
    const int j = (int)threadIdx.x * per + k;
    if (j < nparts) s += part[j];
  }
  s = block_sum_f64(s, sh);
  if (threadIdx.x == 0) clip_state[kClipNorm] = (float)sqrt(s);
}

static int sumsq_grid(long long n) {
  long long b = (n / 4 + 255) / 256;
  if (b > PSEG_GRAD_SUMSQ_MAX_PARTIALS) b = PSEG_GRAD_SUMSQ_MAX_PARTIALS;
  if (b < 1) b = 1;
  return (int)b;
}

// ------------------------------------------------------------------------------------------------ the step
// ONE kernel per update rule behind all six step entry points.  It steps a RUN of the arena: a range with its own
// learning-rate factor and weight decay, covered by a block range of its own.  The grouped entry points (pseg_opt_step_*)
// keep a table of runs on the device and every block looks its run up (kTable = true); the flat ones (pseg_sgd_step,
// pseg_adam_step and their _mp forms) pass the whole arena BY VALUE as the run {offset 0, count n, first_block 0, lr_mult 1,
// weight_decay}, with no table, no clip and no EMA (kTable = false, which reads none of them and alone has a scalar tail:
// table runs are multiples of 4 floats) -- lr * 1.0f is lr, so they compute what the grouped step computes for that run.
// The choice is a template parameter because made at run time it cost Adam a wave per SIMD (72 VGPRs).
// Global-norm clipping, the fused weight EMA and the `-mp` skip cost no launch and no host synchronisation: the clip
// coefficient is derived on the device from the norm pseg_grad_sumsq left there.

// (the layout of pseg_opt_run_t, include/pseg_amd.h)
struct OptRun {
  long long offset, count, first_block;
  float lr_mult, weight_decay;
};
static_assert(sizeof(OptRun) == sizeof(pseg_opt_run_t), "run record layout");

constexpr int kSpan = PSEG_OPT_RUN_SPAN;          // floats one block covers per trip: 256 threads x f32x4

// what every thread derives from the device state before it touches an element
struct StepScalars {
  bool skip;                       // `-mp`: overflow flagged, the step changes nothing
  float gscale;                    // grad_scale [* 1/S] [* clip coefficient]
  bool first;                      // SGD: no step applied so far, the momentum buffer starts as this step's gradient
  float step_size, inv_sqrt_bc2;   // Adam: lr / (1 - b1^t) and 1 / sqrt(1 - b2^t) of this, the t-th applied step
};

// With mp_state the device's count of applied steps decides `first` and the bias corrections; without it the host's
// first_host / step_size_host / inv_sqrt_bc2_host do (the last five arguments are Adam's).
__device__ __forceinline__ StepScalars step_scalars(float gscale, float max_norm, float* clip_state, const float* mp_state,
                                                    int first_host, float lr = 0.f, float b1 = 0.f, float b2 = 0.f,
                                                    float step_size_host = 0.f, float inv_sqrt_bc2_host = 0.f) {
  StepScalars r;
  r.skip = mp_state != nullptr && mp_state[kMpFound] != 0.f;   // overflow somewhere in this step's gradients: skip it
  r.gscale = gscale;
  r.first = first_host != 0;
  r.step_size = step_size_host;
  r.inv_sqrt_bc2 = inv_sqrt_bc2_host;
  if (r.skip) return r;
  if (mp_state != nullptr) {
    gscale *= mp_state[kMpInv];
    r.first = mp_state[kMpSteps] == 0.f;
    const float t = mp_state[kMpSteps] + 1.f;      // this is the t-th applied step
    // bias corrections 1 - b^t as -expm1(t * log b): in fp32 the plain difference 1.f - powf(b, t) carries powf's rounding of a
    // value next to 1 into a result of ~t * (1 - b) -- 7e-6 relative for b2 = 0.999 at t = 2, which moved every parameter by
    // 3e-6 of the step (without mp_state the host computes them in double)
    r.step_size = lr / -expm1f(t * logf(b1));
    r.inv_sqrt_bc2 = 1.f / sqrtf(-expm1f(t * logf(b2)));
  }
  r.gscale = gscale;
  if (max_norm > 0.f) {
    // torch.nn.utils.clip_grad_norm_(error_if_nonfinite=False) on the unscaled gradients
    const float eff = clip_state[kClipNorm] * fabsf(gscale);
    const float coef = fminf(1.f, max_norm / (eff + 1e-6f));
    r.gscale = gscale * coef;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      clip_state[kClipCoef] = coef;
      clip_state[kClipEff] = eff;
      if (coef < 1.f) clip_state[kClipCount] += 1.f;
    }
  }
  return r;
}

// a run as this block sees it: its 4-float groups, the scalar tail behind them (count % 4 floats, stepped by the run's
// first block; table runs have none) and this thread's place among the run's `nblk` blocks
struct RunSlice {
  long long offset, n4, first_i, stride;
  int tail;
  float lr_mult, wd;
};

__device__ __forceinline__ RunSlice slice_of(const OptRun& run, long long nblk) {
  const long long b = (long long)blockIdx.x - run.first_block;
  RunSlice s;
  s.offset = run.offset;
  s.n4 = run.count / 4;
  s.first_i = b * 256 + threadIdx.x;
  s.stride = nblk * 256;
  s.tail = b == 0 ? (int)(run.count - s.n4 * 4) : 0;
  s.lr_mult = run.lr_mult;
  s.wd = run.weight_decay;
  return s;
}

// the run of this block in the table (the search of amax_batch_kernel, once per block)
__device__ __forceinline__ RunSlice find_run(const OptRun* __restrict__ runs, int n) {
  const long long b = blockIdx.x;
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (runs[mid].first_block <= b) lo = mid;
    else hi = mid - 1;
  }
  return slice_of(runs[lo], (lo + 1 < n ? runs[lo + 1].first_block : (long long)gridDim.x) - runs[lo].first_block);
}

// the T (f32x4 in a run's body, float in its tail) at float index i
template <typename T>
__device__ __forceinline__ T& at(float* x, long long i) {
  return *reinterpret_cast<T*>(x + i);
}

template <typename T>
__device__ __forceinline__ void ema_one(T& e, T w, float decay) {
  e = decay * e + (1.f - decay) * w;
}

// torch.optim.SGD on one T; buf: its momentum (read only where mu != 0, and not on the first step)
template <typename T>
__device__ __forceinline__ void sgd_one(T& w, T gr, T* buf, float lr, float mu, float wd, int nesterov, int decoupled,
                                        float gscale, bool first) {
  T d = gr * gscale;
  if (wd != 0.f) {
    if (decoupled) w *= (1.f - lr * wd);
    else d += wd * w;
  }
  if (mu != 0.f) {
    const T b = first ? d : mu * *buf + d;
    *buf = b;
    d = nesterov ? d + mu * b : b;
  }
  w = w - lr * d;
}

template <typename T>
__device__ __forceinline__ void sgd_at(long long i, float* p, const float* g, float* mbuf, float* ema, float lr, float mu,
                                       float wd, int nesterov, int decoupled, float gscale, bool first, float decay) {
  T w = at<T>(p, i);
  sgd_one<T>(w, *reinterpret_cast<const T*>(g + i), mu != 0.f ? &at<T>(mbuf, i) : nullptr, lr, mu, wd, nesterov, decoupled,
             gscale, first);
  at<T>(p, i) = w;
  if (ema != nullptr) ema_one<T>(at<T>(ema, i), w, decay);
}

template <bool kTable>
__global__ __launch_bounds__(256) void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ mbuf,
                                                  float* __restrict__ ema, const OptRun* __restrict__ runs, int n_runs,
                                                  OptRun whole, float lr, float mu, int nesterov, int decoupled,
                                                  float gscale_in, int first_host, float max_norm, float decay,
                                                  float* clip_state, const float* __restrict__ mp_state) {
  if (!kTable) ema = nullptr, max_norm = 0.f;      // (a flat launch has neither: its instantiation carries no code for them)
  const StepScalars ss = step_scalars(gscale_in, max_norm, clip_state, mp_state, first_host);
  if (ss.skip) return;
  const RunSlice r = kTable ? find_run(runs, n_runs) : slice_of(whole, gridDim.x);
  const float lr_r = lr * r.lr_mult;
  p += r.offset;
  g += r.offset;
  if (mbuf != nullptr) mbuf += r.offset;
  if (ema != nullptr) ema += r.offset;
  for (long long i = r.first_i; i < r.n4; i += r.stride)
    sgd_at<f32x4>(i * 4, p, g, mbuf, ema, lr_r, mu, r.wd, nesterov, decoupled, ss.gscale, ss.first, decay);
  if (!kTable && (int)threadIdx.x < r.tail)
    sgd_at<float>(r.n4 * 4 + threadIdx.x, p, g, mbuf, ema, lr_r, mu, r.wd, nesterov, decoupled, ss.gscale, ss.first, decay);
}

// torch.optim.Adam / AdamW on one element
__device__ __forceinline__ void adam_one(float& w, float gr, float& m, float& v, float lr, float b1, float b2, float eps,
                                         float wd, int decoupled, float gscale, float step_size, float inv_sqrt_bc2) {
  float d = gr * gscale;
  if (wd != 0.f) {
    if (decoupled) w *= (1.f - lr * wd);
    else d += wd * w;
  }
  m = b1 * m + (1.f - b1) * d;
  v = b2 * v + (1.f - b2) * d * d;
  const float denom = sqrtf(v) * inv_sqrt_bc2 + eps;
  w -= step_size * (m / denom);
}

template <bool kTable>
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, float* __restrict__ ema,
                                                   const OptRun* __restrict__ runs, int n_runs, OptRun whole, float lr,
                                                   float b1, float b2, float eps, int decoupled, float gscale_in,
                                                   float step_size_host, float inv_sqrt_bc2_host, float max_norm, float decay,
                                                   float* clip_state, const float* __restrict__ mp_state) {
  if (!kTable) ema = nullptr, max_norm = 0.f;      // (a flat launch has neither: its instantiation carries no code for them)
  const StepScalars ss = step_scalars(gscale_in, max_norm, clip_state, mp_state, 0, lr, b1, b2, step_size_host,
                                      inv_sqrt_bc2_host);
  if (ss.skip) return;
  const RunSlice r = kTable ? find_run(runs, n_runs) : slice_of(whole, gridDim.x);
  const float lr_r = lr * r.lr_mult;
  const float step_size = ss.step_size * r.lr_mult;
  p += r.offset;
  g += r.offset;
  m += r.offset;
  v += r.offset;
  if (ema != nullptr) ema += r.offset;
  for (long long i = r.first_i; i < r.n4; i += r.stride) {
    f32x4 w = at<f32x4>(p, i * 4);
    const f32x4 gr = *reinterpret_cast<const f32x4*>(g + i * 4);
    f32x4 mm = at<f32x4>(m, i * 4);
    f32x4 vv = at<f32x4>(v, i * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float we = w[e], me = mm[e], ve = vv[e];
      adam_one(we, gr[e], me, ve, lr_r, b1, b2, eps, r.wd, decoupled, ss.gscale, step_size, ss.inv_sqrt_bc2);
      w[e] = we;
      mm[e] = me;
      vv[e] = ve;
    }
    at<f32x4>(p, i * 4) = w;
    at<f32x4>(m, i * 4) = mm;
    at<f32x4>(v, i * 4) = vv;
    if (ema != nullptr) ema_one(at<f32x4>(ema, i * 4), w, decay);
  }
  if (!kTable && (int)threadIdx.x < r.tail) {
    const long long i = r.n4 * 4 + threadIdx.x;
    adam_one(p[i], g[i], m[i], v[i], lr_r, b1, b2, eps, r.wd, decoupled, ss.gscale, step_size, ss.inv_sqrt_bc2);
    if (ema != nullptr) ema_one(ema[i], p[i], decay);
  }
}

static int grid_for(long long n) {
  long long b = (n / 4 + 255) / 256;
  if (b > 2048) b = 2048;
  if (b < 1) b = 1;
  return (int)b;
}

// Everything a launch relies on, checked against the HOST copy of the run table: rows ascending and disjoint inside
// [0, n), offsets and counts multiples of 4 (no f32x4 straddles a run), block ranges ascending from 0, every run with at
// least one block and no block without a group of its run, their sum the grid.
static int check_runs(const char* who, const pseg_opt_run_t* runs, int n_runs, int64_t total_blocks, int64_t n) {
  int64_t end = 0, blocks = 0;
  for (int r = 0; r < n_runs; ++r) {
    const pseg_opt_run_t& q = runs[r];
    PSEG_REQUIRE(q.offset >= 0 && q.count > 0, "%s: run %d: empty or negative range", who, r);
    PSEG_REQUIRE(q.offset % 4 == 0 && q.count % 4 == 0, "%s: run %d: offset %lld and count %lld must be multiples of 4", who, r,
                 (long long)q.offset, (long long)q.count);
    PSEG_REQUIRE(q.offset >= end, "%s: run %d: runs overlap or are not ascending (offset %lld, previous run ends at %lld)", who,
                 r, (long long)q.offset, (long long)end);
    end = q.offset + q.count;
    PSEG_REQUIRE(end <= n, "%s: run %d ends at %lld, the arena holds %lld floats", who, r, (long long)end, (long long)n);
    PSEG_REQUIRE(q.first_block == blocks, "%s: run %d: first_block %lld, the runs before it hold %lld blocks", who, r,
                 (long long)q.first_block, (long long)blocks);
    const int64_t nb = (r + 1 < n_runs ? runs[r + 1].first_block : total_blocks) - q.first_block;
    PSEG_REQUIRE(nb >= 1 && nb <= (q.count + kSpan - 1) / kSpan, "%s: run %d: %lld blocks for %lld floats", who, r,
                 (long long)nb, (long long)q.count);
    PSEG_REQUIRE(isfinite(q.lr_mult) && isfinite(q.weight_decay), "%s: run %d: lr_mult / weight_decay not finite", who, r);
    blocks += nb;
  }
  PSEG_REQUIRE(blocks == total_blocks, "%s: the runs hold %lld blocks, total_blocks is %lld", who, (long long)blocks,
               (long long)total_blocks);
  return PSEG_OK;
}

static int check_common(const char* who, const void* param, const void* grad, int64_t n, const pseg_opt_run_t* runs,
                        const pseg_opt_run_t* runs_host, int n_runs, int64_t total_blocks, float max_norm, float ema_decay,
                        const float* clip_state) {
  PSEG_REQUIRE(param && grad && runs && runs_host && n > 0 && n_runs > 0, "%s: bad argument (null pointer or empty table)", who);
  PSEG_REQUIRE(total_blocks > 0 && total_blocks < (1LL << 31), "%s: total_blocks out of range", who);
  PSEG_REQUIRE(((uintptr_t)runs & 7) == 0, "%s: run table not 8-byte aligned", who);
  PSEG_REQUIRE(max_norm >= 0.f, "%s: max_norm must be >= 0 (0 switches clipping off); got %g", who, (double)max_norm);
  PSEG_REQUIRE(max_norm == 0.f || clip_state, "%s: clipping needs clip_state (pseg_grad_sumsq fills it)", who);
  PSEG_REQUIRE(ema_decay >= 0.f && ema_decay < 1.f, "%s: ema decay must be in [0, 1); got %g", who, (double)ema_decay);
  PSEG_REQUIRE(((uintptr_t)clip_state & 15) == 0, "%s: clip_state 16-byte alignment", who);
  return check_runs(who, runs_host, n_runs, total_blocks, n);
}

// Adam's bias corrections of the host's 1-based `step`, in double
static void host_bias(float lr, float beta1, float beta2, int step, float* step_size, float* inv_sqrt_bc2) {
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  *step_size = (float)(lr / bc1);
  *inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
}

// The flat entry points: the whole arena as one by-value run on the grid of grid_for(n); no table, no clip, no EMA.
// mp_state: the `-mp` forms (it then replaces first_step / step).
static int flat_sgd(const char* who, float* param, const float* grad, float* momentum_buf, int64_t n, float lr, float momentum,
                    float weight_decay, int nesterov, float grad_scale, int first_step, const float* mp_state, void* stream) {
  PSEG_REQUIRE(param && grad && n > 0, "%s: bad argument", who);
  PSEG_REQUIRE(momentum == 0.f || momentum_buf, "%s: momentum needs a buffer", who);
  PSEG_REQUIRE((((uintptr_t)param | (uintptr_t)grad | (uintptr_t)momentum_buf) & 15) == 0, "%s: 16-byte alignment", who);
  hipLaunchKernelGGL(sgd_kernel<false>, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, param, grad, momentum_buf,
                     (float*)nullptr, (const OptRun*)nullptr, 0, OptRun{0, (long long)n, 0, 1.f, weight_decay}, lr, momentum,
                     nesterov, 0, grad_scale, first_step, 0.f, 0.f, (float*)nullptr, mp_state);
  PSEG_LAUNCH_CHECK();
  return PSEG_OK;
}

static int flat_adam(const char* who, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                     float beta1, float beta2, float eps, float weight_decay, int decoupled, float grad_scale, int step,
                     const float* mp_state, void* stream) {
  PSEG_REQUIRE(param && grad && exp_avg && exp_avg_sq && n > 0, "%s: bad argument", who);
  PSEG_REQUIRE((((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) == 0,
               "%s: 16-byte alignment", who);
  float step_size = 0.f, inv_sqrt_bc2 = 0.f;
  if (!mp_state) host_bias(lr, beta1, beta2, step, &step_size, &inv_sqrt_bc2);
  hipLaunchKernelGGL(adam_kernel<false>, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg, exp_avg_sq,
                     (float*)nullptr, (const OptRun*)nullptr, 0, OptRun{0, (long long)n, 0, 1.f, weight_decay}, lr, beta1, beta2,
                     eps, decoupled, grad_scale, step_size, inv_sqrt_bc2, 0.f, 0.f, (float*)nullptr, mp_state);
  PSEG_LAUNCH_CHECK();
  return PSEG_OK;
}

}  // namespace pseg

using namespace pseg;

extern "C" {

int pseg_sgd_step(float* param, const float* grad, float* momentum_buf, int64_t n, float lr, float momentum,
                  float weight_decay, int nesterov, float grad_scale, int first_step, void* stream) {
  return flat_sgd("sgd_step", param, grad, momentum_buf, n, lr, momentum, weight_decay, nesterov, grad_scale, first_step,
                  nullptr, stream);
}

int pseg_sgd_step_mp(float* param, const float* grad, float* momentum_buf, int64_t n, float lr, float momentum,
                     float weight_decay, int nesterov, float grad_scale, const float* state, void* stream) {
  PSEG_REQUIRE(state, "sgd_step_mp: bad argument");
  return flat_sgd("sgd_step_mp", param, grad, momentum_buf, n, lr, momentum, weight_decay, nesterov, grad_scale, 0, state,
                  stream);
}

int pseg_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                   float beta2, float eps, float weight_decay, int decoupled, float grad_scale, int step, void* stream) {
  PSEG_REQUIRE(step >= 1, "adam_step: bad argument");
  return flat_adam("adam_step", param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, decoupled, grad_scale,
                   step, nullptr, stream);
}

int pseg_adam_step_mp(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                      float beta2, float eps, float weight_decay, int decoupled, float grad_scale, const float* state,
                      void* stream) {
  PSEG_REQUIRE(state, "adam_step_mp: bad argument");
  return flat_adam("adam_step_mp", param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, decoupled,
                   grad_scale, 0, state, stream);
}

int pseg_mp_state_init(float* state, float init_scale, void* stream) {
  PSEG_REQUIRE(state && init_scale > 0.f, "mp_state_init: bad argument");
  hipLaunchKernelGGL(mp_init_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, init_scale);
  PSEG_LAUNCH_CHECK();
  return PSEG_OK;
}

int pseg_mp_check(const float* grad, int64_t n, float* state, void* stream) {
  PSEG_REQUIRE(grad && state && n > 0 && ((uintptr_t)grad & 15) == 0, "mp_check: bad argument");
  hipLaunchKernelGGL(mp_check_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, grad, (long long)n, state);
  PSEG_LAUNCH_CHECK();
  return PSEG_OK;
}

int pseg_mp_update(float* state, float growth_factor, float backoff_factor, int growth_interval, float min_scale,
                   float max_scale, void* stream) {
  PSEG_REQUIRE(state && growth_factor >= 1.f && backoff_factor > 0.f && backoff_factor <= 1.f && growth_interval >= 1 &&
                   min_scale > 0.f && max_scale >= min_scale,
               "mp_update: bad argument");
  hipLaunchKernelGGL(mp_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, growth_factor, backoff_factor,
                     growth_interval, min_scale, max_scale);
  PSEG_LAUNCH_CHECK();
  return PSEG_OK;
}

int64_t pseg_grad_sumsq_workspace_bytes(int64_t n) { return n > 0 ? (int64_t)sumsq_grid(n) * 8 : 0; }

int pseg_grad_sumsq(const float* grad, int64_t n, void* workspace, int64_t workspace_bytes, float* clip_state, void* stream) {
  PSEG_REQUIRE(grad && workspace && clip_state && n > 0, "grad_sumsq: bad argument");
  PSEG_REQUIRE(n % 4 == 0, "grad_sumsq: n must be a multiple of 4 (arena segments are)");
  PSEG_REQUIRE(((uintptr_t)grad & 15) == 0 && ((uintptr_t)workspace & 7) == 0, "grad_sumsq: 16-byte alignment");
  const int grid = sumsq_grid(n);
  PSEG_REQUIRE(workspace_bytes >= (int64_t)grid * 8, "grad_sumsq: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
               (long long)grid * 8);
  hipLaunchKernelGGL(sumsq_partial_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, grad, (long long)(n / 4),
                     (double*)workspace);
  PSEG_LAUNCH_CHECK();
  hipLaunchKernelGGL(sumsq_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)workspace, grid, clip_state);
  PSEG_LAUNCH_CHECK();
  return PSEG_OK;
}

int pseg_opt_step_sgd(float* param, const float* grad, float* momentum_buf, float* ema, int64_t n, const pseg_opt_run_t* runs,
                      const pseg_opt_run_t* runs_host, int n_runs, int64_t total_blocks, float lr, float momentum, int nesterov,
                      int decoupled, float grad_scale, int first_step, float max_norm, float ema_decay, float* clip_state,
                      const float* mp_state, void* stream) {
  const int rc = check_common("opt_step_sgd", param, grad, n, runs, runs_host, n_runs, total_blocks, max_norm, ema_decay,
                              clip_state);
  if (rc != PSEG_OK) return rc;
  PSEG_REQUIRE(momentum == 0.f || momentum_buf, "opt_step_sgd: momentum needs a buffer");
  PSEG_REQUIRE((((uintptr_t)param | (uintptr_t)grad | (uintptr_t)momentum_buf | (uintptr_t)ema) & 15) == 0,
               "opt_step_sgd: 16-byte alignment");
  hipLaunchKernelGGL(sgd_kernel<true>, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream, param, grad, momentum_buf,
                     ema, reinterpret_cast<const OptRun*>(runs), n_runs, OptRun{}, lr, momentum, nesterov, decoupled,
                     grad_scale, first_step, max_norm, ema_decay, clip_state, mp_state);
  PSEG_LAUNCH_CHECK();
  return PSEG_OK;
}

int pseg_opt_step_adam(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n,
                       const pseg_opt_run_t* runs, const pseg_opt_run_t* runs_host, int n_runs, int64_t total_blocks, float lr,
                       float beta1, float beta2, float eps, int decoupled, float grad_scale, int step, float max_norm,
                       float ema_decay, float* clip_state, const float* mp_state, void* stream) {
  const int rc = check_common("opt_step_adam", param, grad, n, runs, runs_host, n_runs, total_blocks, max_norm, ema_decay,
                              clip_state);
  if (rc != PSEG_OK) return rc;
  PSEG_REQUIRE(exp_avg && exp_avg_sq, "opt_step_adam: bad argument (moments)");
  PSEG_REQUIRE(mp_state || step >= 1, "opt_step_adam: step counts from 1");
  PSEG_REQUIRE((((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)ema) & 15) == 0,
               "opt_step_adam: 16-byte alignment");
  float step_size = 0.f, inv_sqrt_bc2 = 0.f;
  if (!mp_state) host_bias(lr, beta1, beta2, step, &step_size, &inv_sqrt_bc2);
  hipLaunchKernelGGL(adam_kernel<true>, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg,
                     exp_avg_sq, ema, reinterpret_cast<const OptRun*>(runs), n_runs, OptRun{}, lr, beta1, beta2, eps, decoupled,
                     grad_scale, step_size, inv_sqrt_bc2, max_norm, ema_decay, clip_state, mp_state);
  PSEG_LAUNCH_CHECK();
  return PSEG_OK;
}

int pseg_amax(const float* x, int64_t ld, int64_t M, int C, float* amax_inout, void* stream) {
  PSEG_REQUIRE(x && amax_inout && M > 0 && C > 0 && ld >= C, "amax: bad argument");
  long long b = (M * C + 1023) / 1024;
  if (b > 1024) b = 1024;
  if (b < 1) b = 1;
  hipLaunchKernelGGL(amax_kernel, dim3((unsigned)b), dim3(256), 0, (hipStream_t)stream, x, (long long)ld, (long long)M, C,
                     (unsigned*)amax_inout);
  PSEG_LAUNCH_CHECK();
  return PSEG_OK;
}

int pseg_amax_batch(const int64_t* jobs, int n, int64_t total_blocks, float* out, void* stream) {
  PSEG_REQUIRE(jobs && out && n > 0 && total_blocks > 0 && total_blocks < (1LL << 31), "amax_batch: bad argument");
  if (hipMemsetAsync(out, 0, (size_t)n * 4, (hipStream_t)stream) != hipSuccess) {
    set_error("amax_batch: hipMemsetAsync failed");
    return PSEG_ERR_HIP;
  }
  hipLaunchKernelGGL(amax_batch_kernel, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const long long*>(jobs), n, (unsigned*)out);
  PSEG_LAUNCH_CHECK();
  return PSEG_OK;
}

int pseg_fill(float* x, int64_t n, float value, void* stream) {
  PSEG_REQUIRE(x && n > 0 && ((uintptr_t)x & 15) == 0, "fill: bad argument");
  hipLaunchKernelGGL(fill_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, x, (long long)n, value);
  PSEG_LAUNCH_CHECK();
  return PSEG_OK;
}

}  // extern "C"
