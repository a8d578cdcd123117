// Cross-entropy with per-class weights, label smoothing, the focal modulation and online hard-pixel selection (fused
// forward + backward) on gfx950.  The contract is in include/pseg_amd.h (pseg_ce_opts_fwd_bwd); DESIGN.md 5e has the
// derivation.  Per valid pixel, with p = softmax(z), t the label, w the class weights, W = sum_c w_c:
//     l = (1 - eps) w_t (-log p_t) + (eps / C) sum_c w_c (-log p_c)          f = (1 - p_t)^gamma l
// and loss = sum_kept f / sum_kept w_t over the kept pixels: every valid one (keep_ratio == 1), or those with f >= tau,
// tau the k-th largest f.  Two pipelines, all on the caller's stream, nothing read back by the host:
//   keep_ratio == 1:  co_count_kernel (targets only: n_valid, n_bad, partials of sum w_t) -> co_den_kernel ->
//       co_pixel_kernel<MODE 0> (ONE read of the logits, one write of dlogits, partials of sum f) -> co_finish_kernel.
//   keep_ratio < 1:   co_pixel_kernel<MODE 1> parks a 32-bit key of f per pixel (4 bytes / pixel; order-preserving map
//       of the float's bits, 0 = pixel does not count), counts the labels and takes the histogram of the keys' top byte
//       -> co_select_kernel -> three times (co_hist_kernel over the keys that match the digits chosen so far ->
//       co_select_kernel): an MSD radix select, after which hdr->prefix is the key of tau -> co_kept_kernel (keys + targets:
//       partials of sum f and sum w_t over key >= key(tau), n_kept) -> co_den_kernel -> co_finish_kernel ->
//       co_pixel_kernel<MODE 2> (recomputes the softmax, takes "kept" from the PARKED key, writes dlogits).
// The kept set, tau and the loss all come from the parked values, so they are consistent by construction; ties at tau are
// all kept.  Floating-point sums go through per-block partials added in a fixed order, in double; atomics add integers
// only (counts, histograms), so two calls give identical bits.
// pseg_ce_opts_binned_fwd_bwd is the same pipeline with a per-pixel weight u = bin_weight[pixel_bin]: the
// BINNED instantiations of the kernels that see pixels read one byte beside the target and look u up in a 256-entry table
// staged in LDS; u scales the per-pixel value BEFORE it is summed or parked (g = u f), the divisor's terms (u w_t) and the
// gradient.  1.0f * x is exact, so a table of ones gives the unbinned call's bits.
#include "loss_common.h"

#include <math.h>

namespace pseg {

constexpr int kCoMaxBlocks = 4096;

struct CoHeader {
  int n_valid, n_bad, n_kept;
  unsigned prefix;       // digits of tau's key chosen so far (after round 3: the key of tau)
  unsigned k_rem;        // rank of tau among the keys that match the prefix
  float inv_den;         // 1 / sum_kept w_t, 0 when that sum is 0
  int pad[2];
  double den;            // sum_kept w_t
  double pad2;
  unsigned hist[4][256];
};

struct CoArgs {
  const float* logits;
  const int64_t* target;
  const float* w;        // nullable: all ones
  float* dlogits;        // nullable
  CoHeader* hdr;
  double* pf;            // per-block partials of sum f (MODE 0)
  unsigned* keys;        // MODE 1 writes, MODE 2 reads
  int C;
  long long HW, groups, ignore_index;
  float eps, gamma;
  int gint;              // gamma when it is an integer, else -1
  const uint8_t* bins;   // BINNED only: [B][HW], any alignment
  const float* btab;     // BINNED only: 256 pixel weights
  int bins_aligned;      // bins is 4-byte aligned: a lane's VEC bytes are one load
};

__device__ __forceinline__ float co_wgt(const float* __restrict__ w, long long c) { return w ? w[c] : 1.f; }

// The table of pixel weights in LDS, one entry per lane of the 256-lane block (the caller's next barrier publishes it).
// Lookups are ds_read_b32 at a per-lane address: equal bins broadcast, and neighbouring pixels mostly share a depth.
__device__ __forceinline__ void co_stage_table(float* ltab, const float* __restrict__ btab) { ltab[threadIdx.x] = btab[threadIdx.x]; }

// the VEC consecutive bin bytes of a lane: one 32-bit (16-bit) load when the plane is aligned, else byte loads
template <int VEC>
__device__ __forceinline__ void co_load_bins(const uint8_t* __restrict__ bp, bool aligned, unsigned (&bin)[VEC]) {
  if (VEC == 4 && aligned) {
    const unsigned wd = *reinterpret_cast<const unsigned*>(bp);
#pragma unroll
    for (int e = 0; e < VEC; ++e) bin[e] = (wd >> (8 * e)) & 0xFFu;
  } else if (VEC == 2 && aligned) {
    const unsigned wd = *reinterpret_cast<const unsigned short*>(bp);
#pragma unroll
    for (int e = 0; e < VEC; ++e) bin[e] = (wd >> (8 * e)) & 0xFFu;
  } else {
#pragma unroll
    for (int e = 0; e < VEC; ++e) bin[e] = bp[e];
  }
}

// order-preserving map float -> unsigned (and back); valid pixels never get key 0
__device__ __forceinline__ unsigned co_key(float f) {
  const unsigned b = __builtin_bit_cast(unsigned, f);
  const unsigned k = b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
  return k ? k : 1u;
}
__device__ __forceinline__ float co_unkey(unsigned k) {
  return __builtin_bit_cast(float, k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}

// What one pixel contributes, from the pieces of its softmax: s = sum_c e_c, so = sum_{c != t} e_c, et = e_t with
// e_c = exp(z_c - max), zt = z_t - max, wz = sum_c w_c (z_c - max), wt = w_t.
struct CoTerm {
  float f;      // (1 - p_t)^gamma l
  float P;      // dz_j (j != t) = e_j * P - w_j * Q
  float Q;
  float T;      // dz_t
};

__device__ __forceinline__ CoTerm co_term(float s, float so, float et, float zt, float wz, float wt, float W, float eps,
                                          float epsC, float gamma, int gint, float ls) {
  const float rs = 1.f / s;
  // -log p_c = ls - (z_c - max): both parts are non-negative, nothing cancels
  const float ell = (1.f - eps) * wt * (ls - zt) + epsC * (W * ls - wz);
  // 1 - p_t from the OTHER classes' exponentials (1.f - p_t would lose every digit of a confident pixel)
  const float q = so * rs, pt = et * rs;
  float qg1 = 1.f, mf = 1.f;      // q^(gamma - 1), q^gamma; gamma == 0: the factor is 1 and has no derivative
  if (gamma != 0.f) {
    if (gint > 0) {
      for (int i = 1; i < gint; ++i) qg1 *= q;
    } else {
      qg1 = powf(q, gamma - 1.f);
    }
    mf = qg1 * q;
  }
  const float A = mf * (1.f - eps) * wt, D = ell * gamma * qg1 * pt, Bc = mf * epsC;
  CoTerm r;
  r.f = mf * ell + 0.f;           // (+ 0: never -0, whose key would sort below +0)
  r.P = (A + Bc * W + D) * rs;
  r.Q = Bc;
  r.T = Bc * (pt * W - wt) - (A + D) * q;
  return r;
}

// targets only (keep_ratio == 1): label counts and the partials of the divisor sum_valid w_t (BINNED: u w_t)
template <bool BINNED>
__global__ __launch_bounds__(256) void co_count_kernel(const int64_t* __restrict__ target, long long n, long long ignore_index,
                                                       int C, const float* __restrict__ w, CoHeader* __restrict__ hdr,
                                                       double* __restrict__ pw, const uint8_t* __restrict__ bins,
                                                       const float* __restrict__ btab) {
  __shared__ double shd[4];
  __shared__ int shc[2][4];
  __shared__ float ltab[BINNED ? 256 : 1];
  if (BINNED) {
    co_stage_table(ltab, btab);
    __syncthreads();
  }
  int cnt = 0, bad = 0;
  double sw = 0.0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const long long t = target[i];
    const bool v = ce_valid(t, ignore_index, C);
    cnt += v ? 1 : 0;
    bad += (!v && t != ignore_index) ? 1 : 0;
    if (v) sw += BINNED ? (double)(ltab[bins[i]] * co_wgt(w, t)) : (double)co_wgt(w, t);
  }
  block_count(cnt, bad, &hdr->n_valid, &hdr->n_bad, shc);
  const double tot = block_sum_d_again(sw, shd);
  if (threadIdx.x == 0) pw[blockIdx.x] = tot;
}

// MODE 0: loss partials + gradient, every valid pixel kept.  MODE 1: park the keys, count the labels, histogram of the
// keys' top byte.  MODE 2: gradient, kept = parked key >= key of tau.
// CMAX: compile-time bound on the class count (values live in registers); VEC consecutive pixels per lane.
template <int CMAX, int VEC, int MODE, bool BINNED>
__global__ __launch_bounds__(256) void co_pixel_kernel(const CoArgs a) {
  typedef float vecf __attribute__((ext_vector_type(VEC)));
  typedef unsigned vecu __attribute__((ext_vector_type(VEC)));
  __shared__ double shd[4];
  __shared__ int shc[2][4];
  __shared__ unsigned lh[256];
  __shared__ float ltab[BINNED ? 256 : 1];
  const int C = a.C;
  const long long HW = a.HW;
  const float* __restrict__ w = a.w;
  if (MODE == 1) lh[threadIdx.x] = 0;
  if (BINNED) co_stage_table(ltab, a.btab);
  if (MODE == 1 || BINNED) __syncthreads();
  float W = 0.f;
  for (int c = 0; c < C; ++c) W += co_wgt(w, c);
  const float epsC = a.eps / (float)C;
  const float inv_den = MODE == 1 ? 0.f : a.hdr->inv_den;
  const unsigned tau_key = MODE == 2 ? a.hdr->prefix : 0u;
  const long long gpi = HW / VEC;  // groups per image
  double lsum = 0.0;
  int cnt = 0, bad = 0;
  for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < a.groups; g += (long long)gridDim.x * 256) {
    const long long b = g / gpi;
    const long long p = (g - b * gpi) * VEC;
    const float* lp = a.logits + b * C * HW + p;
    vecf v[CMAX];
#pragma unroll
    for (int c = 0; c < CMAX; ++c)
      if (c < C) v[c] = *reinterpret_cast<const vecf*>(lp + (long long)c * HW);
    long long t[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) t[e] = a.target[b * HW + p + e];
    vecu key = 0u;
    if (MODE == 2) key = *reinterpret_cast<const vecu*>(a.keys + b * HW + p);
    vecf m = v[0];
#pragma unroll
    for (int c = 1; c < CMAX; ++c)
      if (c < C) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) m[e] = fmaxf(m[e], v[c][e]);
      }
    bool valid[VEC];
    vecf wt;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      valid[e] = ce_valid(t[e], a.ignore_index, C);
      wt[e] = valid[e] ? co_wgt(w, t[e]) : 0.f;
    }
    vecf u = 1.f;
    if (BINNED) {
      unsigned bin[VEC];
      co_load_bins<VEC>(a.bins + b * HW + p, a.bins_aligned != 0, bin);
#pragma unroll
      for (int e = 0; e < VEC; ++e) u[e] = ltab[bin[e]];
    }
    // one exponential per logit: v[c] becomes exp(v[c] - m) (__expf / __logf: the hardware exp2 / log2 paths)
    vecf s = 0.f, so = 0.f, et = 0.f, zt = 0.f, wz = 0.f;
#pragma unroll
    for (int c = 0; c < CMAX; ++c)
      if (c < C) {
        const float wc = co_wgt(w, c);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          const float d = v[c][e] - m[e];
          const float ev = __expf(d);
          const bool is_t = t[e] == c;
          zt[e] = is_t ? d : zt[e];
          et[e] = is_t ? ev : et[e];
          so[e] += is_t ? 0.f : ev;
          s[e] += ev;
          wz[e] += wc * d;
          v[c][e] = ev;
        }
      }
    vecf P, Q, T;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const CoTerm r = co_term(s[e], so[e], et[e], zt[e], wz[e], wt[e], W, a.eps, epsC, a.gamma, a.gint, __logf(s[e]));
      const float gf = BINNED ? u[e] * r.f : r.f;      // (u >= 0, f >= +0: never -0)
      bool kept = valid[e];
      if (MODE == 0 && valid[e]) lsum += (double)gf;
      if (MODE == 1) {
        key[e] = valid[e] ? co_key(gf) : 0u;
        if (valid[e]) atomicAdd(&lh[key[e] >> 24], 1u);
        cnt += valid[e] ? 1 : 0;
        bad += (!valid[e] && t[e] != a.ignore_index) ? 1 : 0;
      }
      if (MODE == 2) kept = valid[e] && key[e] >= tau_key;
      const float sc = kept ? (BINNED ? u[e] * inv_den : inv_den) : 0.f;
      P[e] = r.P * sc;
      Q[e] = r.Q * sc;
      T[e] = r.T * sc;
    }
    if (MODE == 1) *reinterpret_cast<vecu*>(a.keys + b * HW + p) = key;
    if (MODE != 1 && a.dlogits) {
#pragma unroll
      for (int c = 0; c < CMAX; ++c)
        if (c < C) {
          const float wc = co_wgt(w, c);
          vecf gvec;
#pragma unroll
          for (int e = 0; e < VEC; ++e) gvec[e] = (t[e] == c) ? T[e] : v[c][e] * P[e] - Q[e] * wc;
          *reinterpret_cast<vecf*>(a.dlogits + b * C * HW + p + (long long)c * HW) = gvec;
        }
    }
  }
  if (MODE == 0) {
    const double tot = block_sum_d_again(lsum, shd);
    if (threadIdx.x == 0) a.pf[blockIdx.x] = tot;
  }
  if (MODE == 1) {
    block_count(cnt, bad, &a.hdr->n_valid, &a.hdr->n_bad, shc);      // (barrier inside: lh is complete after it)
    if (lh[threadIdx.x]) atomicAdd(&a.hdr->hist[0][threadIdx.x], lh[threadIdx.x]);
  }
}

// any class count: one pixel per lane, sweeps over the class planes (the re-reads hit L2)
template <int MODE, bool BINNED>
__global__ __launch_bounds__(256) void co_generic_kernel(const CoArgs a) {
  __shared__ double shd[4];
  __shared__ int shc[2][4];
  __shared__ unsigned lh[256];
  __shared__ float ltab[BINNED ? 256 : 1];
  const int C = a.C;
  const long long HW = a.HW;
  const float* __restrict__ w = a.w;
  if (MODE == 1) lh[threadIdx.x] = 0;
  if (BINNED) co_stage_table(ltab, a.btab);
  if (MODE == 1 || BINNED) __syncthreads();
  float W = 0.f;
  for (int c = 0; c < C; ++c) W += co_wgt(w, c);
  const float epsC = a.eps / (float)C;
  const float inv_den = MODE == 1 ? 0.f : a.hdr->inv_den;
  const unsigned tau_key = MODE == 2 ? a.hdr->prefix : 0u;
  double lsum = 0.0;
  int cnt = 0, bad = 0;
  for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < a.groups; g += (long long)gridDim.x * 256) {
    const long long b = g / HW;
    const long long p = g - b * HW;
    const float* lp = a.logits + b * C * HW + p;
    const long long t = a.target[g];
    const bool valid = ce_valid(t, a.ignore_index, C);
    const float wt = valid ? co_wgt(w, t) : 0.f;
    float m = lp[0];
    for (int c = 1; c < C; ++c) m = fmaxf(m, lp[(long long)c * HW]);
    float s = 0.f, so = 0.f, et = 0.f, zt = 0.f, wz = 0.f;
    for (int c = 0; c < C; ++c) {
      const float d = lp[(long long)c * HW] - m;
      const float ev = expf(d);
      const bool is_t = t == c;
      zt = is_t ? d : zt;
      et = is_t ? ev : et;
      so += is_t ? 0.f : ev;
      s += ev;
      wz += co_wgt(w, c) * d;
    }
    const CoTerm r = co_term(s, so, et, zt, wz, wt, W, a.eps, epsC, a.gamma, a.gint, logf(s));
    const float u = BINNED ? ltab[a.bins[g]] : 1.f;
    const float gf = BINNED ? u * r.f : r.f;
    bool kept = valid;
    if (MODE == 0 && valid) lsum += (double)gf;
    if (MODE == 1) {
      const unsigned key = valid ? co_key(gf) : 0u;
      a.keys[g] = key;
      if (valid) atomicAdd(&lh[key >> 24], 1u);
      cnt += valid ? 1 : 0;
      bad += (!valid && t != a.ignore_index) ? 1 : 0;
    }
    if (MODE == 2) kept = valid && a.keys[g] >= tau_key;
    if (MODE != 1 && a.dlogits) {
      const float sc = kept ? (BINNED ? u * inv_den : inv_den) : 0.f;
      const float P = r.P * sc, Q = r.Q * sc, T = r.T * sc;
      float* dp = a.dlogits + b * C * HW + p;
      for (int c = 0; c < C; ++c) {
        const float ev = expf(lp[(long long)c * HW] - m);
        dp[(long long)c * HW] = (t == c) ? T : ev * P - Q * co_wgt(w, c);
      }
    }
  }
  if (MODE == 0) {
    const double tot = block_sum_d_again(lsum, shd);
    if (threadIdx.x == 0) a.pf[blockIdx.x] = tot;
  }
  if (MODE == 1) {
    block_count(cnt, bad, &a.hdr->n_valid, &a.hdr->n_bad, shc);
    if (lh[threadIdx.x]) atomicAdd(&a.hdr->hist[0][threadIdx.x], lh[threadIdx.x]);
  }
}

// round r = 1..3 of the radix select: among the keys whose top r bytes equal the prefix, the histogram of the next byte
__global__ __launch_bounds__(256) void co_hist_kernel(const unsigned* __restrict__ keys, long long n, int round,
                                                      CoHeader* __restrict__ hdr) {
  __shared__ unsigned lh[256];
  lh[threadIdx.x] = 0;
  __syncthreads();
  const int top = 32 - 8 * round, shift = 24 - 8 * round;
  const unsigned want = hdr->prefix >> top;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const unsigned k = keys[i];
    if (k != 0u && (k >> top) == want) atomicAdd(&lh[(k >> shift) & 0xFFu], 1u);
  }
  __syncthreads();
  if (lh[threadIdx.x]) atomicAdd(&hdr->hist[round][threadIdx.x], lh[threadIdx.x]);
}

// one block: the digit of this round in which the k-th largest matching key lies (digits visited from 255 down)
__global__ __launch_bounds__(256) void co_select_kernel(CoHeader* __restrict__ hdr, int round, float keep_ratio) {
  __shared__ unsigned h[256];
  const int t = threadIdx.x;
  h[t] = hdr->hist[round][t];
  unsigned k;
  if (round == 0) {
    const int n = hdr->n_valid;
    double kk = ceil((double)keep_ratio * (double)n);
    kk = kk < 1.0 ? 1.0 : kk;
    kk = kk > (double)n ? (double)n : kk;
    k = n > 0 ? (unsigned)kk : 0u;
  } else {
    k = hdr->k_rem;
  }
  const unsigned prefix = round == 0 ? 0u : hdr->prefix;
  __syncthreads();
  unsigned greater = 0;
  for (int d = t + 1; d < 256; ++d) greater += h[d];
  if (k >= 1u && greater < k && k <= greater + h[t]) {      // true for exactly one digit when k <= the matching keys
    hdr->prefix = prefix | ((unsigned)t << (24 - 8 * round));
    hdr->k_rem = k - greater;
  }
}

// keys + targets: partials of sum f and sum w_t over the kept pixels, and their number (BINNED: the parked values are
// u f already; the divisor's terms are u w_t)
template <bool BINNED>
__global__ __launch_bounds__(256) void co_kept_kernel(const unsigned* __restrict__ keys, const int64_t* __restrict__ target,
                                                      long long n, long long ignore_index, int C,
                                                      const float* __restrict__ w, CoHeader* __restrict__ hdr,
                                                      double* __restrict__ pf, double* __restrict__ pw,
                                                      const uint8_t* __restrict__ bins, const float* __restrict__ btab) {
  __shared__ double shd[4];
  __shared__ int shc[2][4];
  __shared__ float ltab[BINNED ? 256 : 1];
  if (BINNED) {
    co_stage_table(ltab, btab);
    __syncthreads();
  }
  const unsigned tau_key = hdr->prefix;
  int cnt = 0;
  double sf = 0.0, sw = 0.0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const unsigned k = keys[i];
    const long long t = target[i];
    if (ce_valid(t, ignore_index, C) && k >= tau_key) {
      sf += (double)co_unkey(k);
      sw += BINNED ? (double)(ltab[bins[i]] * co_wgt(w, t)) : (double)co_wgt(w, t);
      ++cnt;
    }
  }
  block_count(cnt, 0, &hdr->n_kept, (int*)nullptr, shc);
  const double tf = block_sum_d_again(sf, shd);
  const double tw = block_sum_d_again(sw, shd);
  if (threadIdx.x == 0) {
    pf[blockIdx.x] = tf;
    pw[blockIdx.x] = tw;
  }
}

// one block, fixed order (ce_finish_kernel's): lane t adds partials t, t + 256, ..., then waves, then lanes
__device__ __forceinline__ double co_sum_partials(const double* __restrict__ partial, int nblocks, double* sh) {
  return block_sum_d_again(thread_sum_partials(partial, nblocks), sh);
}

__global__ __launch_bounds__(256) void co_den_kernel(const double* __restrict__ pw, int nblocks, CoHeader* __restrict__ hdr) {
  __shared__ double sh[4];
  const double den = co_sum_partials(pw, nblocks, sh);
  if (threadIdx.x == 0) {
    hdr->den = den;
    hdr->inv_den = den > 0.0 ? (float)(1.0 / den) : 0.f;      // zero divisor: the gradient is all zeros
  }
}

__global__ __launch_bounds__(256) void co_finish_kernel(const double* __restrict__ pf, int nblocks, int selected,
                                                        const CoHeader* __restrict__ hdr, float* __restrict__ out) {
  __shared__ double sh[4];
  const double sf = co_sum_partials(pf, nblocks, sh);
  if (threadIdx.x == 0) {
    const double den = hdr->den;
    out[0] = den > 0.0 ? (float)(sf / den) : NAN;      // as torch and pseg_ce_fwd_bwd: nothing to average is NaN
    out[1] = (float)hdr->n_valid;
    out[2] = (float)hdr->n_bad;
    out[3] = (float)(selected ? hdr->n_kept : hdr->n_valid);
    out[4] = (selected && hdr->n_valid > 0) ? co_unkey(hdr->prefix) : 0.f;
    out[5] = (float)den;
  }
}

struct CoPlan {
  int64_t pf, pw, keys, bytes;      // byte offsets into the workspace
};

static CoPlan co_plan(int64_t npix) {
  CoPlan p;
  int64_t o = align256(sizeof(CoHeader));
  p.pf = o;   o = align256(o + (int64_t)kCoMaxBlocks * 8);
  p.pw = o;   o = align256(o + (int64_t)kCoMaxBlocks * 8);
  p.keys = o; o = align256(o + (npix + 3) / 4 * 16);      // the parked values: 4 bytes per pixel
  p.bytes = o;
  return p;
}

static bool co_sizes_ok(int B, int C, int64_t HW) {
  return B > 0 && C > 0 && HW > 0 && HW <= ((1ll << 31) - 1) / B;      // the counts and histograms are 32-bit
}

// launch the per-pixel kernel of one MODE: the register form for C <= 32 (vector loads when the planes allow), else generic
template <int MODE, bool BINNED>
static int co_launch_pixels(CoArgs a, long long npix, bool vec4, hipStream_t st) {
  int blocks;
#define CO_LAUNCH(CMAX, VEC)                                                                              \
  do {                                                                                                    \
    a.groups = npix / VEC;                                                                                \
    blocks = capped_blocks(a.groups, kCoMaxBlocks);                                                       \
    hipLaunchKernelGGL((co_pixel_kernel<CMAX, VEC, MODE, BINNED>), dim3(blocks), dim3(256), 0, st, a);            \
  } while (0)
  const int C = a.C;
  if (C <= 4 && vec4) CO_LAUNCH(4, 4);
  else if (C <= 4) CO_LAUNCH(4, 1);
  else if (C <= 8 && vec4) CO_LAUNCH(8, 4);
  else if (C <= 8) CO_LAUNCH(8, 1);
  else if (C <= 24 && vec4) CO_LAUNCH(24, 4);
  else if (C <= 24) CO_LAUNCH(24, 1);
  else if (C <= 32 && vec4) CO_LAUNCH(32, 2);
  else if (C <= 32) CO_LAUNCH(32, 1);
  else {
    a.groups = npix;
    blocks = capped_blocks(npix, kCoMaxBlocks);
    hipLaunchKernelGGL((co_generic_kernel<MODE, BINNED>), dim3(blocks), dim3(256), 0, st, a);
  }
#undef CO_LAUNCH
  return blocks;
}

// both entry points: `fn` heads the refusal messages; BINNED takes pixel_bin / bin_weight
template <bool BINNED>
static int co_run(const char* fn, const float* logits, const int64_t* target, const uint8_t* pixel_bin, const float* bin_weight,
                  int B, int C, int64_t HW, int64_t ignore_index, const float* class_weight, float label_smoothing,
                  float focal_gamma, float keep_ratio, float* dlogits, float* loss_out, void* workspace,
                  int64_t workspace_bytes, void* stream) {
  PSEG_REQUIRE(logits && target && loss_out && workspace, "%s: null pointer", fn);
  PSEG_REQUIRE(!BINNED || (pixel_bin && bin_weight), "%s: null pixel_bin or bin_weight", fn);
  PSEG_REQUIRE(B > 0 && C > 0 && HW > 0, "%s: bad sizes", fn);
  PSEG_REQUIRE(co_sizes_ok(B, C, HW), "%s: more than 2^31 - 1 pixels are not supported (B=%d HW=%lld); split the batch", fn, B,
               (long long)HW);
  const long long npix = (long long)B * HW;
  const CoPlan pl = co_plan(npix);
  PSEG_REQUIRE(workspace_bytes >= pl.bytes, "%s: workspace too small (%lld < %lld bytes)", fn, (long long)workspace_bytes,
               (long long)pl.bytes);
  PSEG_REQUIRE(((uintptr_t)workspace & 15) == 0, "%s: workspace must be 16-byte aligned", fn);
  PSEG_REQUIRE(label_smoothing >= 0.f && label_smoothing < 1.f, "%s: label_smoothing must be in [0, 1) (got %g)", fn,
               (double)label_smoothing);
  PSEG_REQUIRE(keep_ratio > 0.f && keep_ratio <= 1.f, "%s: keep_ratio must be in (0, 1] (got %g)", fn, (double)keep_ratio);
  // 0 < gamma < 1: with smoothing the derivative of (1 - p_t)^gamma is unbounded as p_t -> 1
  PSEG_REQUIRE(focal_gamma == 0.f || (focal_gamma >= 1.f && focal_gamma <= 8.f),
               "%s: focal_gamma must be 0 or in [1, 8] (got %g)", fn, (double)focal_gamma);
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  CoHeader* hdr = (CoHeader*)ws;
  double* pf = (double*)(ws + pl.pf);
  double* pw = (double*)(ws + pl.pw);
  unsigned* keys = (unsigned*)(ws + pl.keys);
  if (hipMemsetAsync(hdr, 0, sizeof(CoHeader), st) != hipSuccess) {
    set_error("%s: hipMemsetAsync failed", fn);
    return PSEG_ERR_HIP;
  }
  CoArgs a;
  a.logits = logits;
  a.target = target;
  a.w = class_weight;
  a.dlogits = dlogits;
  a.hdr = hdr;
  a.pf = pf;
  a.keys = keys;
  a.C = C;
  a.HW = (long long)HW;
  a.groups = 0;
  a.ignore_index = (long long)ignore_index;
  a.eps = label_smoothing;
  a.gamma = focal_gamma;
  a.gint = (focal_gamma == floorf(focal_gamma)) ? (int)focal_gamma : -1;
  a.bins = pixel_bin;
  a.btab = bin_weight;
  a.bins_aligned = (((uintptr_t)pixel_bin & 3) == 0) ? 1 : 0;      // (vector paths have HW % 4 == 0: every lane's bytes are then aligned)
  const bool vec4 = (HW % 4 == 0) && (((uintptr_t)logits & 15) == 0) && (!dlogits || ((uintptr_t)dlogits & 15) == 0);
  const long long ign = (long long)ignore_index;
  if (keep_ratio == 1.f) {
    const int nb = capped_blocks(npix, 2048);
    hipLaunchKernelGGL(co_count_kernel<BINNED>, dim3(nb), dim3(256), 0, st, target, npix, ign, C, class_weight, hdr, pw, pixel_bin,
                       bin_weight);
    PSEG_LAUNCH_CHECK();
    hipLaunchKernelGGL(co_den_kernel, dim3(1), dim3(256), 0, st, (const double*)pw, nb, hdr);
    PSEG_LAUNCH_CHECK();
    const int blocks = co_launch_pixels<0, BINNED>(a, npix, vec4, st);
    PSEG_LAUNCH_CHECK();
    hipLaunchKernelGGL(co_finish_kernel, dim3(1), dim3(256), 0, st, (const double*)pf, blocks, 0, (const CoHeader*)hdr,
                       loss_out);
    PSEG_LAUNCH_CHECK();
    return PSEG_OK;
  }
  co_launch_pixels<1, BINNED>(a, npix, vec4, st);
  PSEG_LAUNCH_CHECK();
  const int nb = capped_blocks(npix, 2048);
  for (int round = 0; round < 4; ++round) {
    if (round > 0) {
      hipLaunchKernelGGL(co_hist_kernel, dim3(nb), dim3(256), 0, st, (const unsigned*)keys, npix, round, hdr);
      PSEG_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(co_select_kernel, dim3(1), dim3(256), 0, st, hdr, round, keep_ratio);
    PSEG_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(co_kept_kernel<BINNED>, dim3(nb), dim3(256), 0, st, (const unsigned*)keys, target, npix, ign, C, class_weight,
                     hdr, pf, pw, pixel_bin, bin_weight);
  PSEG_LAUNCH_CHECK();
  hipLaunchKernelGGL(co_den_kernel, dim3(1), dim3(256), 0, st, (const double*)pw, nb, hdr);
  PSEG_LAUNCH_CHECK();
  hipLaunchKernelGGL(co_finish_kernel, dim3(1), dim3(256), 0, st, (const double*)pf, nb, 1, (const CoHeader*)hdr, loss_out);
  PSEG_LAUNCH_CHECK();
  if (dlogits) {
    co_launch_pixels<2, BINNED>(a, npix, vec4, st);
    PSEG_LAUNCH_CHECK();
  }
  return PSEG_OK;
}

}  // namespace pseg

using namespace pseg;

extern "C" {

int64_t pseg_ce_opts_workspace_bytes(int B, int C, int64_t HW) {
  if (!co_sizes_ok(B, C, HW)) return 0;
  return co_plan((int64_t)B * HW).bytes;
}

int pseg_ce_opts_fwd_bwd(const float* logits, const int64_t* target, int B, int C, int64_t HW, int64_t ignore_index,
                         const float* class_weight, float label_smoothing, float focal_gamma, float keep_ratio,
                         float* dlogits, float* loss_out, void* workspace, int64_t workspace_bytes, void* stream) {
  return co_run<false>("ce_opts", logits, target, nullptr, nullptr, B, C, HW, ignore_index, class_weight, label_smoothing,
                       focal_gamma, keep_ratio, dlogits, loss_out, workspace, workspace_bytes, stream);
}

int pseg_ce_opts_binned_fwd_bwd(const float* logits, const int64_t* target, const uint8_t* pixel_bin,
                                const float* bin_weight, int B, int C, int64_t HW, int64_t ignore_index,
                                const float* class_weight, float label_smoothing, float focal_gamma, float keep_ratio,
                                float* dlogits, float* loss_out, void* workspace, int64_t workspace_bytes, void* stream) {
  return co_run<true>("pseg_ce_opts_binned_fwd_bwd", logits, target, pixel_bin, bin_weight, B, C, HW, ignore_index,
                      class_weight, label_smoothing, focal_gamma, keep_ratio, dlogits, loss_out, workspace, workspace_bytes,
                      stream);
}

}  // extern "C"
