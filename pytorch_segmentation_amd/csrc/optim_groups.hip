// Grouped optimiser step over the flat parameter arena on gfx950: per-run learning-rate factor and weight decay,
// global-norm gradient clipping and a fused exponential moving average of the weights -- still ONE step launch and no host
// synchronisation (the clip coefficient is derived on the device from the norm a preceding launch left there).
// The element arithmetic is that of sgd_kernel / adam_one (optim.hip) statement for statement: a one-run table with
// lr_mult = 1, no clip and no EMA reproduces pseg_sgd_step / pseg_adam_step and their _mp forms bit for bit.
#include "common.h"

#include <math.h>

namespace pseg {

// (the layout of pseg_opt_run_t, include/pseg_amd.h)
struct OptRun {
  long long offset, count, first_block;
  float lr_mult, weight_decay;
};
static_assert(sizeof(OptRun) == sizeof(pseg_opt_run_t), "run record layout");

constexpr int kSpan = PSEG_OPT_RUN_SPAN;          // floats one block covers per trip: 256 threads x f32x4
constexpr int kMpInv = 1, kMpFound = 3, kMpSteps = 4;   // (the `-mp` state words of optim.hip)
constexpr int kClipNorm = 0, kClipCoef = 1, kClipEff = 2, kClipCount = 3;

// ------------------------------------------------------------------------------------------------ gradient norm
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

// ------------------------------------------------------------------------------------------------ grouped step
// what every thread derives from the device state before it touches an element
struct StepScale {
  float scale;      // grad_scale [* 1/S] * clip coefficient
  bool skip;        // `-mp`: overflow flagged, the step changes nothing
};

__device__ __forceinline__ StepScale step_scale(float gscale, float max_norm, float* clip_state, const float* mp_state) {
  StepScale r;
  r.skip = mp_state != nullptr && mp_state[kMpFound] != 0.f;
  r.scale = gscale;
  if (r.skip) return r;
  if (mp_state != nullptr) gscale *= mp_state[kMpInv];
  r.scale = gscale;
  if (max_norm > 0.f) {
    // torch.nn.utils.clip_grad_norm_(error_if_nonfinite=False) on the unscaled gradients
    const float eff = clip_state[kClipNorm] * fabsf(gscale);
    const float coef = fminf(1.f, max_norm / (eff + 1e-6f));
    r.scale = gscale * coef;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      clip_state[kClipCoef] = coef;
      clip_state[kClipEff] = eff;
      if (coef < 1.f) clip_state[kClipCount] += 1.f;
    }
  }
  return r;
}

// the run of this block (the search of amax_batch_kernel, once per block) -> its 4-float groups and this block's place
struct RunSlice {
  long long offset, n4, first_i, stride;
  float lr_mult, wd;
};

__device__ __forceinline__ RunSlice find_run(const OptRun* __restrict__ runs, int n) {
  const long long b = blockIdx.x;
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (runs[mid].first_block <= b) lo = mid;
    else hi = mid - 1;
  }
  const long long first = runs[lo].first_block;
  const long long nblk = (lo + 1 < n ? runs[lo + 1].first_block : (long long)gridDim.x) - first;
  RunSlice s;
  s.offset = runs[lo].offset;
  s.n4 = runs[lo].count / 4;
  s.first_i = (b - first) * 256 + threadIdx.x;
  s.stride = nblk * 256;
  s.lr_mult = runs[lo].lr_mult;
  s.wd = runs[lo].weight_decay;
  return s;
}

__global__ __launch_bounds__(256) void opt_sgd_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                      float* __restrict__ mbuf, float* __restrict__ ema,
                                                      const OptRun* __restrict__ runs, int n_runs, float lr, float mu,
                                                      int nesterov, int decoupled, float gscale_in, int first_host,
                                                      float max_norm, float decay, float* clip_state,
                                                      const float* __restrict__ mp_state) {
  const StepScale ss = step_scale(gscale_in, max_norm, clip_state, mp_state);
  if (ss.skip) return;
  const float gscale = ss.scale;
  const bool first = mp_state != nullptr ? mp_state[kMpSteps] == 0.f : first_host != 0;
  const RunSlice r = find_run(runs, n_runs);
  const float wd = r.wd;
  const float lr_r = lr * r.lr_mult;
  p += r.offset;
  g += r.offset;
  if (mbuf != nullptr) mbuf += r.offset;
  if (ema != nullptr) ema += r.offset;
  for (long long i = r.first_i; i < r.n4; i += r.stride) {
    f32x4 w = *reinterpret_cast<f32x4*>(p + i * 4);
    f32x4 d = *reinterpret_cast<const f32x4*>(g + i * 4) * gscale;
    if (wd != 0.f) {
      if (decoupled) w *= (1.f - lr_r * wd);
      else d += wd * w;
    }
    if (mu != 0.f) {
      f32x4 b = first ? d : mu * *reinterpret_cast<f32x4*>(mbuf + i * 4) + d;
      *reinterpret_cast<f32x4*>(mbuf + i * 4) = b;
      d = nesterov ? d + mu * b : b;
    }
    w = w - lr_r * d;
    *reinterpret_cast<f32x4*>(p + i * 4) = w;
    if (ema != nullptr) {
      const f32x4 e = *reinterpret_cast<f32x4*>(ema + i * 4);
      *reinterpret_cast<f32x4*>(ema + i * 4) = decay * e + (1.f - decay) * w;
    }
  }
}

__device__ __forceinline__ void adam_elem(float& w, float gr, float& m, float& v, float lr, float b1, float b2, float eps,
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

__global__ __launch_bounds__(256) void opt_adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                       float* __restrict__ m, float* __restrict__ v,
                                                       float* __restrict__ ema, const OptRun* __restrict__ runs, int n_runs,
                                                       float lr, float b1, float b2, float eps, int decoupled,
                                                       float gscale_in, float step_size_host, float inv_sqrt_bc2_host,
                                                       float max_norm, float decay, float* clip_state,
                                                       const float* __restrict__ mp_state) {
  const StepScale ss = step_scale(gscale_in, max_norm, clip_state, mp_state);
  if (ss.skip) return;
  const float gscale = ss.scale;
  float step_size = step_size_host, inv_sqrt_bc2 = inv_sqrt_bc2_host;
  if (mp_state != nullptr) {
    // (bias corrections from the device's count of applied steps, in the form adam_mp_kernel gives its reasons for)
    const float t = mp_state[kMpSteps] + 1.f;
    step_size = lr / -expm1f(t * logf(b1));
    inv_sqrt_bc2 = 1.f / sqrtf(-expm1f(t * logf(b2)));
  }
  const RunSlice r = find_run(runs, n_runs);
  const float wd = r.wd;
  const float lr_r = lr * r.lr_mult;
  step_size *= r.lr_mult;
  p += r.offset;
  g += r.offset;
  m += r.offset;
  v += r.offset;
  if (ema != nullptr) ema += r.offset;
  for (long long i = r.first_i; i < r.n4; i += r.stride) {
    f32x4 w = *reinterpret_cast<f32x4*>(p + i * 4);
    const f32x4 gr = *reinterpret_cast<const f32x4*>(g + i * 4);
    f32x4 mm = *reinterpret_cast<f32x4*>(m + i * 4);
    f32x4 vv = *reinterpret_cast<f32x4*>(v + i * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float we = w[e], me = mm[e], ve = vv[e];
      adam_elem(we, gr[e], me, ve, lr_r, b1, b2, eps, wd, decoupled, gscale, step_size, inv_sqrt_bc2);
      w[e] = we;
      mm[e] = me;
      vv[e] = ve;
    }
    *reinterpret_cast<f32x4*>(p + i * 4) = w;
    *reinterpret_cast<f32x4*>(m + i * 4) = mm;
    *reinterpret_cast<f32x4*>(v + i * 4) = vv;
    if (ema != nullptr) {
      const f32x4 e = *reinterpret_cast<f32x4*>(ema + i * 4);
      *reinterpret_cast<f32x4*>(ema + i * 4) = decay * e + (1.f - decay) * w;
    }
  }
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

static int check_common(const char* who, const void* param, const void* grad, const void* ema, int64_t n,
                        const pseg_opt_run_t* runs, const pseg_opt_run_t* runs_host, int n_runs, int64_t total_blocks,
                        float max_norm, float ema_decay, const float* clip_state) {
  PSEG_REQUIRE(param && grad && runs && runs_host && n > 0 && n_runs > 0, "%s: bad argument (null pointer or empty table)", who);
  PSEG_REQUIRE(total_blocks > 0 && total_blocks < (1LL << 31), "%s: total_blocks out of range", who);
  PSEG_REQUIRE(((uintptr_t)runs & 7) == 0, "%s: run table not 8-byte aligned", who);
  PSEG_REQUIRE(max_norm >= 0.f, "%s: max_norm must be >= 0 (0 switches clipping off); got %g", who, (double)max_norm);
  PSEG_REQUIRE(max_norm == 0.f || clip_state, "%s: clipping needs clip_state (pseg_grad_sumsq fills it)", who);
  PSEG_REQUIRE(ema_decay >= 0.f && ema_decay < 1.f, "%s: ema decay must be in [0, 1); got %g", who, (double)ema_decay);
  PSEG_REQUIRE(((uintptr_t)clip_state & 15) == 0, "%s: clip_state 16-byte alignment", who);
  (void)ema;
  return check_runs(who, runs_host, n_runs, total_blocks, n);
}

}  // namespace pseg

using namespace pseg;

extern "C" {

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
  const int rc = check_common("opt_step_sgd", param, grad, ema, n, runs, runs_host, n_runs, total_blocks, max_norm, ema_decay,
                              clip_state);
  if (rc != PSEG_OK) return rc;
  PSEG_REQUIRE(momentum == 0.f || momentum_buf, "opt_step_sgd: momentum needs a buffer");
  PSEG_REQUIRE((((uintptr_t)param | (uintptr_t)grad | (uintptr_t)momentum_buf | (uintptr_t)ema) & 15) == 0,
               "opt_step_sgd: 16-byte alignment");
  hipLaunchKernelGGL(opt_sgd_kernel, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream, param, grad, momentum_buf,
                     ema, reinterpret_cast<const OptRun*>(runs), n_runs, lr, momentum, nesterov, decoupled, grad_scale,
                     first_step, max_norm, ema_decay, clip_state, mp_state);
  PSEG_LAUNCH_CHECK();
  return PSEG_OK;
}

int pseg_opt_step_adam(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n,
                       const pseg_opt_run_t* runs, const pseg_opt_run_t* runs_host, int n_runs, int64_t total_blocks, float lr,
                       float beta1, float beta2, float eps, int decoupled, float grad_scale, int step, float max_norm,
                       float ema_decay, float* clip_state, const float* mp_state, void* stream) {
  const int rc = check_common("opt_step_adam", param, grad, ema, n, runs, runs_host, n_runs, total_blocks, max_norm, ema_decay,
                              clip_state);
  if (rc != PSEG_OK) return rc;
  PSEG_REQUIRE(exp_avg && exp_avg_sq, "opt_step_adam: bad argument (moments)");
  PSEG_REQUIRE(mp_state || step >= 1, "opt_step_adam: step counts from 1");
  PSEG_REQUIRE((((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)ema) & 15) == 0,
               "opt_step_adam: 16-byte alignment");
  float step_size = 0.f, inv_sqrt_bc2 = 0.f;
  if (!mp_state) {
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    step_size = (float)(lr / bc1);
    inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
  }
  hipLaunchKernelGGL(opt_adam_kernel, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg,
                     exp_avg_sq, ema, reinterpret_cast<const OptRun*>(runs), n_runs, lr, beta1, beta2, eps, decoupled, grad_scale,
                     step_size, inv_sqrt_bc2, max_norm, ema_decay, clip_state, mp_state);
  PSEG_LAUNCH_CHECK();
  return PSEG_OK;
}

}  // extern "C"
