// Soft region-overlap loss (soft Dice / Tversky / focal-Tversky over the softmax of the logits) with its gradient with
// respect to the logits, on gfx950.  The contract is in include/pseg_amd.h (pseg_tversky_fwd_bwd).
//
// Geometry shared by the two passes over the logits: a block of 256 threads owns 1024 consecutive pixels of ONE image
// (so a group of per_image = 1 is a contiguous range of blocks), a lane owns four of them and sweeps the classes, whose
// planes are pixel-contiguous in NCHW.  With HW % 4 == 0 and 16-byte aligned operands the four pixels are consecutive and
// every access is 16 bytes (VEC); otherwise they are 256 apart and every access is one coalesced dword.
//   1. tversky_reduce_kernel: online max / sum of exponentials over the classes, then a second sweep (the tile's planes
//      come back from L2) forms p and reduces, per class, the lane's four pixels, then the wave (DPP adds inside a row of
//      16 lanes, four v_readlane across the rows), then the block's four waves through LDS in wave order, into
//      FP_c = sum of p_c over valid pixels of another label, TP_c = sum of p_c over pixels of label c and n_c (ballot +
//      popcount).  One double per (class, block) and quantity goes to the workspace; nothing is an atomic.
//   2. tversky_sum_kernel (one block per (group, class)): the group's block partials, added in a fixed order in double.
//      tversky_coef_kernel (one block): TI_c, the loss, out[] and the two gradient coefficients of every (group, class)
//      -- g_ic is ct_c at a pixel of label c and cn_c elsewhere -- in double.
//   3. tversky_grad_kernel (only with dlogits): the online sweep again, carrying sum_k cn_k exp(z_k - m) along with the
//      sum of exponentials, so that sum_k g_ik p_ik = (that) / s + (ct_t - cn_t) p_t is known after ONE sweep; the second
//      sweep writes p_ij (g_ij - dot) once.  p is never parked anywhere.
// No per-thread state grows with C (1024 classes cost registers for four pixels, like 2), and every floating-point sum
// has a fixed order, so two calls give identical bits.
#include "loss_common.h"

#include <math.h>

namespace pseg {

constexpr int kTvThreads = 256;
constexpr int kTvPix = 4;                               // pixels per lane
constexpr int kTvTile = kTvThreads * kTvPix;            // pixels per block
constexpr int kTvMaxClasses = 1024;

struct TvOpts {
  double alpha, beta, smooth, power;
  int per_image, all_classes;
};

// v + (v of the lane the DPP control names); every lane of the wave must be active
template <int CTRL>
__device__ __forceinline__ float tv_dpp_add(float v) {
  const int u = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true);
  return v + __builtin_bit_cast(float, u);
}

// Sum over the 64 lanes, the same bits in every lane: quads (quad_perm [1,0,3,2], [2,3,0,1]), then the four quads of a
// row of 16 (row_ror:4, row_ror:8), then the four rows through lanes 0, 16, 32, 48.
__device__ __forceinline__ float tv_wave_sum(float v) {
  v = tv_dpp_add<0xB1>(v);
  v = tv_dpp_add<0x4E>(v);
  v = tv_dpp_add<0x124>(v);
  v = tv_dpp_add<0x128>(v);
  const int i = __builtin_bit_cast(int, v);
  const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(i, 0));
  const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(i, 16));
  const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(i, 32));
  const float r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(i, 48));
  return (r0 + r1) + (r2 + r3);
}

// pixel j of a lane whose first pixel is p0
template <bool VEC>
__device__ __forceinline__ unsigned tv_pix(unsigned p0, int j) {
  return VEC ? p0 + j : p0 + j * kTvThreads;
}

// the lane's four values of one class plane; 0 past the image
template <bool VEC>
__device__ __forceinline__ void tv_load(const float* __restrict__ plane, unsigned p0, unsigned HW, float x[kTvPix]) {
  if (VEC) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p0 < HW) v = *reinterpret_cast<const float4*>(plane + p0);      // HW % 4 == 0: the whole vector is inside
    x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
  } else {
#pragma unroll
    for (int j = 0; j < kTvPix; ++j) {
      const unsigned p = tv_pix<false>(p0, j);
      x[j] = p < HW ? plane[p] : 0.f;
    }
  }
}

// the lane's four labels: tc = the class of a valid pixel, -1 otherwise; bad = in the image, not ignore_index, out of range
template <bool VEC>
__device__ __forceinline__ void tv_labels(const int64_t* __restrict__ tg, unsigned p0, unsigned HW, long long ign, int C,
                                          int tc[kTvPix], bool bad[kTvPix]) {
  long long t[kTvPix];
  bool in[kTvPix];
  if (VEC) {
    const bool inside = p0 < HW;
    longlong2 a = make_longlong2(ign, ign), b = make_longlong2(ign, ign);
    if (inside) {
      const longlong2* q = reinterpret_cast<const longlong2*>(tg + p0);
      a = q[0];
      b = q[1];
    }
    t[0] = a.x; t[1] = a.y; t[2] = b.x; t[3] = b.y;
#pragma unroll
    for (int j = 0; j < kTvPix; ++j) in[j] = inside;
  } else {
#pragma unroll
    for (int j = 0; j < kTvPix; ++j) {
      const unsigned p = tv_pix<false>(p0, j);
      in[j] = p < HW;
      t[j] = in[j] ? (long long)tg[p] : ign;
    }
  }
#pragma unroll
  for (int j = 0; j < kTvPix; ++j) {
    const bool valid = in[j] && ce_valid(t[j], ign, C);
    tc[j] = valid ? (int)t[j] : -1;
    bad[j] = in[j] && !valid && t[j] != ign;
  }
}

// One sweep over the classes: running max m and s = sum_c exp(z_c - m) of the lane's four pixels.  GRAD: also
// d = sum_c cn_c exp(z_c - m) (cf = the group's [C][2] coefficients {ct, cn}) and zt = the logit of the pixel's own label.
template <bool VEC, bool GRAD>
__device__ __forceinline__ void tv_online_sweep(const float* __restrict__ img, size_t HW, unsigned p0, int C,
                                                const float* __restrict__ cf, const int tc[kTvPix], float m[kTvPix],
                                                float s[kTvPix], float d[kTvPix], float zt[kTvPix]) {
#pragma unroll
  for (int j = 0; j < kTvPix; ++j) {
    m[j] = -INFINITY;
    s[j] = 0.f;
    d[j] = 0.f;
    zt[j] = 0.f;
  }
#pragma unroll 4
  for (int c = 0; c < C; ++c) {
    float x[kTvPix];
    tv_load<VEC>(img + (size_t)c * HW, p0, (unsigned)HW, x);
    const float cn = GRAD ? cf[2 * c + 1] : 0.f;
#pragma unroll
    for (int j = 0; j < kTvPix; ++j) {
      const float mn = fmaxf(m[j], x[j]);
      const float sc = __expf(m[j] - mn);       // exp(-inf) = 0 on the first class
      const float e = __expf(x[j] - mn);
      s[j] = s[j] * sc + e;
      if (GRAD) {
        d[j] = d[j] * sc + cn * e;
        zt[j] = tc[j] == c ? x[j] : zt[j];
      }
      m[j] = mn;
    }
  }
}

// ------------------------------------------------------------------------------------------------ pass 1
// dynamic LDS: wq[4][C], wtp[4][C] floats, wn[4][C] ints (a wave's sums of one class), wbad[4] ints
template <bool VEC>
__global__ __launch_bounds__(kTvThreads) void tversky_reduce_kernel(const float* __restrict__ logits,
                                                                    const int64_t* __restrict__ target, int C, unsigned HW,
                                                                    unsigned tiles, size_t nblk, long long ign,
                                                                    double* __restrict__ pq, double* __restrict__ ptp,
                                                                    double* __restrict__ pn, int* __restrict__ pbad) {
  extern __shared__ float tv_lds[];
  float* wq = tv_lds;
  float* wtp = wq + 4 * C;
  int* wn = reinterpret_cast<int*>(wtp + 4 * C);
  int* wbad = wn + 4 * C;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const unsigned b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
  const unsigned p0 = tile * kTvTile + (VEC ? tid * kTvPix : tid);
  const float* img = logits + (size_t)b * C * HW;
  int tc[kTvPix];
  bool bad[kTvPix];
  tv_labels<VEC>(target + (size_t)b * HW, p0, HW, ign, C, tc, bad);
  int nbad = 0;
#pragma unroll
  for (int j = 0; j < kTvPix; ++j) nbad += __popcll(__ballot(bad[j]));
  if (lane == 0) wbad[w] = nbad;
  const bool any = __ballot(tc[0] >= 0 || tc[1] >= 0 || tc[2] >= 0 || tc[3] >= 0) != 0ull;
  if (any) {                                    // (the same in every lane of the wave)
    float m[kTvPix], s[kTvPix], d[kTvPix], zt[kTvPix];
    tv_online_sweep<VEC, false>(img, HW, p0, C, nullptr, tc, m, s, d, zt);
    float inv[kTvPix];
#pragma unroll
    for (int j = 0; j < kTvPix; ++j) inv[j] = 1.f / s[j];
#pragma unroll 2
    for (int c = 0; c < C; ++c) {
      float x[kTvPix];
      tv_load<VEC>(img + (size_t)c * HW, p0, HW, x);
      float tp = 0.f, q = 0.f;
      int n = 0;
#pragma unroll
      for (int j = 0; j < kTvPix; ++j) {
        const float p = __expf(x[j] - m[j]) * inv[j];
        const bool is = tc[j] == c;
        tp += is ? p : 0.f;
        q += (!is && tc[j] >= 0) ? p : 0.f;
        n += __popcll(__ballot(is));
      }
      tp = tv_wave_sum(tp);
      q = tv_wave_sum(q);
      if (lane == 0) {
        wq[w * C + c] = q;
        wtp[w * C + c] = tp;
        wn[w * C + c] = n;
      }
    }
  } else {
    for (int c = lane; c < C; c += 64) {
      wq[w * C + c] = 0.f;
      wtp[w * C + c] = 0.f;
      wn[w * C + c] = 0;
    }
  }
  __syncthreads();
  for (int c = tid; c < C; c += kTvThreads) {     // the four waves in wave order
    const size_t o = (size_t)c * nblk + blockIdx.x;
    pq[o] = (((double)wq[c] + (double)wq[C + c]) + (double)wq[2 * C + c]) + (double)wq[3 * C + c];
    ptp[o] = (((double)wtp[c] + (double)wtp[C + c]) + (double)wtp[2 * C + c]) + (double)wtp[3 * C + c];
    pn[o] = (double)(wn[c] + wn[C + c] + wn[2 * C + c] + wn[3 * C + c]);
  }
  if (tid == 0) pbad[blockIdx.x] = wbad[0] + wbad[1] + wbad[2] + wbad[3];
}

// ------------------------------------------------------------------------------------------------ pass 2
// block (g * C + c): sums[g][c] = {n_c, S_c, TP_c, FP_c} over the group's blocks; class_sums (nullable) gets the first three
__global__ __launch_bounds__(kTvThreads) void tversky_sum_kernel(const double* __restrict__ pq, const double* __restrict__ ptp,
                                                                 const double* __restrict__ pn, int C, unsigned tiles,
                                                                 size_t nblk, int per_image, double* __restrict__ sums,
                                                                 double* __restrict__ class_sums) {
  __shared__ double sh[3][4];
  const unsigned g = blockIdx.x / (unsigned)C, c = blockIdx.x - g * (unsigned)C;
  const size_t first = per_image ? (size_t)g * tiles : 0, len = per_image ? (size_t)tiles : nblk;
  const size_t base = (size_t)c * nblk + first;
  double q = 0.0, tp = 0.0, n = 0.0;
  for (size_t i = threadIdx.x; i < len; i += kTvThreads) {
    q += pq[base + i];
    tp += ptp[base + i];
    n += pn[base + i];
  }
  q = wave_sum_d(q);
  tp = wave_sum_d(tp);
  n = wave_sum_d(n);
  if ((threadIdx.x & 63) == 0) {
    sh[0][threadIdx.x >> 6] = q;
    sh[1][threadIdx.x >> 6] = tp;
    sh[2][threadIdx.x >> 6] = n;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    q = ((sh[0][0] + sh[0][1]) + sh[0][2]) + sh[0][3];
    tp = ((sh[1][0] + sh[1][1]) + sh[1][2]) + sh[1][3];
    n = ((sh[2][0] + sh[2][1]) + sh[2][2]) + sh[2][3];
    double* o = sums + (size_t)blockIdx.x * 4;
    o[0] = n;
    o[1] = q + tp;
    o[2] = tp;
    o[3] = q;
    if (class_sums) {
      class_sums[(size_t)blockIdx.x * 3 + 0] = n;
      class_sums[(size_t)blockIdx.x * 3 + 1] = q + tp;
      class_sums[(size_t)blockIdx.x * 3 + 2] = tp;
    }
  }
}

struct TvClass {
  double one_minus, N, D, FP, FN;       // 1 - TI_c as (alpha FP + beta FN) / D; 0 when D == 0
};

__device__ __forceinline__ TvClass tv_class(const double* __restrict__ s, const TvOpts& o) {
  TvClass k;
  const double n = s[0], TP = s[2];
  k.FP = s[3];
  k.FN = fmax(n - TP, 0.0);             // (TP <= n already: a rounded sum of values <= 1 never passes their number)
  k.N = TP + o.smooth;
  k.D = TP + o.alpha * k.FP + o.beta * k.FN + o.smooth;
  k.one_minus = k.D > 0.0 ? (o.alpha * k.FP + o.beta * k.FN) / k.D : 0.0;
  return k;
}

// one block: the loss and out[], then coef[g][c] = {ct, cn}: g_ic at a pixel of label c / of another label
__global__ __launch_bounds__(kTvThreads) void tversky_coef_kernel(const double* __restrict__ sums, const int* __restrict__ pbad,
                                                                  int C, int G, size_t nblk, TvOpts o, float* __restrict__ coef,
                                                                  int* __restrict__ gcnt, float* __restrict__ out) {
  __shared__ double sh[4];
  const int tid = threadIdx.x;
  double loss_sum = 0.0, n_valid = 0.0, n_terms = 0.0, n_groups = 0.0;      // the same in every thread
  for (int g = 0; g < G; ++g) {
    const double* sg = sums + (size_t)g * C * 4;
    double nv = 0.0;
    for (int c = tid; c < C; c += kTvThreads) nv += sg[(size_t)c * 4];
    nv = block_sum_d_again(nv, sh);
    double ts = 0.0, cnt = 0.0;
    if (nv > 0.0) {
      for (int c = tid; c < C; c += kTvThreads) {
        if (!o.all_classes && !(sg[(size_t)c * 4] > 0.0)) continue;
        ts += pow(tv_class(sg + (size_t)c * 4, o).one_minus, o.power);
        cnt += 1.0;
      }
    }
    ts = block_sum_d_again(ts, sh);
    cnt = block_sum_d_again(cnt, sh);
    if (tid == 0) gcnt[g] = (int)cnt;
    if (cnt > 0.0) {
      loss_sum += ts / cnt;
      n_groups += 1.0;
      n_terms += cnt;
    }
    n_valid += nv;
  }
  double n_bad = 0.0;
  for (size_t i = tid; i < nblk; i += kTvThreads) n_bad += (double)pbad[i];
  n_bad = block_sum_d_again(n_bad, sh);      // (its barriers also order gcnt[] before the reads below)
  for (int g = 0; g < G; ++g) {
    const double* sg = sums + (size_t)g * C * 4;
    const double cnt = (double)gcnt[g];
    for (int c = tid; c < C; c += kTvThreads) {
      float ct = 0.f, cn = 0.f;
      if (cnt > 0.0 && (o.all_classes || sg[(size_t)c * 4] > 0.0)) {
        const TvClass k = tv_class(sg + (size_t)c * 4, o);
        if (k.one_minus > 0.0) {          // (then D > 0)
          const double K = -o.power * pow(k.one_minus, o.power - 1.0) / (cnt * n_groups);
          const double d2 = k.D * k.D;
          ct = (float)(K * ((o.beta * k.N + o.alpha * k.FP + o.beta * k.FN) / d2));
          cn = (float)(-K * (o.alpha * k.N / d2));
        }
      }
      coef[((size_t)g * C + c) * 2 + 0] = ct;
      coef[((size_t)g * C + c) * 2 + 1] = cn;
    }
  }
  if (tid == 0) {
    out[0] = n_groups > 0.0 ? (float)(loss_sum / n_groups) : 0.f;
    out[1] = (float)n_valid;
    out[2] = (float)n_bad;
    out[3] = (float)n_terms;
    out[4] = (float)n_groups;
  }
}

// ------------------------------------------------------------------------------------------------ pass 3
template <bool VEC>
__global__ __launch_bounds__(kTvThreads) void tversky_grad_kernel(const float* __restrict__ logits,
                                                                  const int64_t* __restrict__ target, int C, unsigned HW,
                                                                  unsigned tiles, long long ign, int per_image,
                                                                  const float* __restrict__ coef, float* __restrict__ dlogits) {
  const int tid = threadIdx.x;
  const unsigned b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
  const unsigned p0 = tile * kTvTile + (VEC ? tid * kTvPix : tid);
  const float* img = logits + (size_t)b * C * HW;
  float* dimg = dlogits + (size_t)b * C * HW;
  const float* cf = coef + (size_t)(per_image ? b : 0u) * C * 2;
  int tc[kTvPix];
  bool bad[kTvPix];
  tv_labels<VEC>(target + (size_t)b * HW, p0, HW, ign, C, tc, bad);
  const bool any = __ballot(tc[0] >= 0 || tc[1] >= 0 || tc[2] >= 0 || tc[3] >= 0) != 0ull;
  float m[kTvPix], inv[kTvPix], dot[kTvPix];
#pragma unroll
  for (int j = 0; j < kTvPix; ++j) m[j] = inv[j] = dot[j] = 0.f;
  if (any) {                                    // (the same in every lane of the wave)
    float s[kTvPix], d[kTvPix], zt[kTvPix];
    tv_online_sweep<VEC, true>(img, HW, p0, C, cf, tc, m, s, d, zt);
#pragma unroll
    for (int j = 0; j < kTvPix; ++j) {
      inv[j] = 1.f / s[j];
      const int t = tc[j] >= 0 ? tc[j] : 0;
      const float pt = __expf(zt[j] - m[j]) * inv[j];
      dot[j] = d[j] * inv[j] + (cf[2 * t] - cf[2 * t + 1]) * pt;      // sum_k g_ik p_ik
    }
  }
#pragma unroll 2
  for (int c = 0; c < C; ++c) {
    float o[kTvPix] = {0.f, 0.f, 0.f, 0.f};
    if (any) {
      float x[kTvPix];
      tv_load<VEC>(img + (size_t)c * HW, p0, HW, x);
      const float ct = cf[2 * c], cn = cf[2 * c + 1];
#pragma unroll
      for (int j = 0; j < kTvPix; ++j) {
        const float p = __expf(x[j] - m[j]) * inv[j];
        const float g = tc[j] == c ? ct : cn;
        o[j] = tc[j] >= 0 ? p * (g - dot[j]) : 0.f;
      }
    }
    float* dplane = dimg + (size_t)c * HW;
    if (VEC) {
      if (p0 < HW) *reinterpret_cast<float4*>(dplane + p0) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
      for (int j = 0; j < kTvPix; ++j) {
        const unsigned p = tv_pix<false>(p0, j);
        if (p < HW) dplane[p] = o[j];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ host
struct TvPlan {
  unsigned tiles;       // blocks per image
  int64_t nblk;         // blocks
  int G;                // groups
  int64_t pq, ptp, pn, pbad, sums, coef, gcnt, bytes;      // byte offsets into the workspace
};

static bool tv_sizes_ok(int B, int C, int64_t HW) {
  if (B <= 0 || C <= 0 || HW <= 0 || C > kTvMaxClasses) return false;
  if (HW > (1ll << 31) / 8 / B) return false;                            // targets: B * HW * 8 bytes
  return (int64_t)B * HW * C * 4 < (1ll << 31) && (int64_t)B * HW * 8 < (1ll << 31);
}

static TvPlan tv_plan(int B, int C, int64_t HW, int per_image) {
  TvPlan p;
  p.tiles = (unsigned)((HW + kTvTile - 1) / kTvTile);
  p.nblk = (int64_t)B * p.tiles;
  p.G = per_image ? B : 1;
  int64_t o = 0;
  p.pq = o;   o = align256(o + (int64_t)C * p.nblk * 8);
  p.ptp = o;  o = align256(o + (int64_t)C * p.nblk * 8);
  p.pn = o;   o = align256(o + (int64_t)C * p.nblk * 8);
  p.pbad = o; o = align256(o + p.nblk * 4);
  p.sums = o; o = align256(o + (int64_t)p.G * C * 32);
  p.coef = o; o = align256(o + (int64_t)p.G * C * 8);
  p.gcnt = o; o = align256(o + (int64_t)p.G * 4);
  p.bytes = o;
  return p;
}

}  // namespace pseg

using namespace pseg;

extern "C" {

int64_t pseg_tversky_workspace_bytes(int B, int C, int64_t HW) {
  if (!tv_sizes_ok(B, C, HW)) return 0;
  return tv_plan(B, C, HW, 1).bytes;      // the per-image plan is the larger one
}

int pseg_tversky_fwd_bwd(const float* logits, const int64_t* target, int B, int C, int64_t HW, int64_t ignore_index,
                         float alpha, float beta, float smooth, float power, int per_image, int all_classes,
                         float* dlogits, float* out, double* class_sums, void* workspace, int64_t workspace_bytes,
                         void* stream) {
  PSEG_REQUIRE(logits && target && out && workspace, "pseg_tversky_fwd_bwd: null pointer");
  PSEG_REQUIRE(B > 0 && C > 0 && HW > 0, "pseg_tversky_fwd_bwd: bad sizes");
  PSEG_REQUIRE(C <= kTvMaxClasses, "pseg_tversky_fwd_bwd: at most %d classes (got %d)", kTvMaxClasses, C);
  PSEG_REQUIRE(tv_sizes_ok(B, C, HW),
               "pseg_tversky_fwd_bwd: logits or targets at or above 2 GiB are not supported (B=%d C=%d HW=%lld); split the batch",
               B, C, (long long)HW);
  PSEG_REQUIRE(isfinite(alpha) && isfinite(beta) && isfinite(smooth) && isfinite(power),
               "pseg_tversky_fwd_bwd: alpha, beta, smooth and power must be finite");
  PSEG_REQUIRE(alpha >= 0.f && beta >= 0.f && alpha + beta > 0.f,
               "pseg_tversky_fwd_bwd: alpha and beta must be non-negative and not both zero (got %g, %g)", alpha, beta);
  PSEG_REQUIRE(smooth >= 0.f, "pseg_tversky_fwd_bwd: smooth must be non-negative (got %g)", smooth);
  PSEG_REQUIRE(power >= 0.5f && power <= 4.f, "pseg_tversky_fwd_bwd: power must lie in [0.5, 4] (got %g)", power);
  PSEG_REQUIRE(dlogits != logits, "pseg_tversky_fwd_bwd: dlogits must not alias logits");
  per_image = per_image ? 1 : 0;
  const TvPlan pl = tv_plan(B, C, HW, per_image);
  const int64_t need = pseg_tversky_workspace_bytes(B, C, HW);
  PSEG_REQUIRE(workspace_bytes >= need, "pseg_tversky_fwd_bwd: workspace too small (%lld < %lld bytes)",
               (long long)workspace_bytes, (long long)need);
  PSEG_REQUIRE(((uintptr_t)workspace & 15) == 0, "pseg_tversky_fwd_bwd: workspace must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  double* pq = (double*)(ws + pl.pq);
  double* ptp = (double*)(ws + pl.ptp);
  double* pn = (double*)(ws + pl.pn);
  int* pbad = (int*)(ws + pl.pbad);
  double* sums = (double*)(ws + pl.sums);
  float* coef = (float*)(ws + pl.coef);
  int* gcnt = (int*)(ws + pl.gcnt);
  const unsigned hw = (unsigned)HW;
  const size_t nblk = (size_t)pl.nblk;
  const long long ign = (long long)ignore_index;
  const bool vec = HW % 4 == 0 && (((uintptr_t)logits | (uintptr_t)target | (uintptr_t)dlogits) & 15) == 0;
  const size_t lds = ((size_t)12 * C + 4) * 4;
  TvOpts o;
  o.alpha = alpha;
  o.beta = beta;
  o.smooth = smooth;
  o.power = power;
  o.per_image = per_image;
  o.all_classes = all_classes ? 1 : 0;

  if (vec)
    hipLaunchKernelGGL((tversky_reduce_kernel<true>), dim3((unsigned)nblk), dim3(kTvThreads), lds, st, logits, target, C, hw,
                       pl.tiles, nblk, ign, pq, ptp, pn, pbad);
  else
    hipLaunchKernelGGL((tversky_reduce_kernel<false>), dim3((unsigned)nblk), dim3(kTvThreads), lds, st, logits, target, C, hw,
                       pl.tiles, nblk, ign, pq, ptp, pn, pbad);
  PSEG_LAUNCH_CHECK();
  hipLaunchKernelGGL(tversky_sum_kernel, dim3((unsigned)pl.G * (unsigned)C), dim3(kTvThreads), 0, st, (const double*)pq,
                     (const double*)ptp, (const double*)pn, C, pl.tiles, nblk, per_image, sums, class_sums);
  PSEG_LAUNCH_CHECK();
  hipLaunchKernelGGL(tversky_coef_kernel, dim3(1), dim3(kTvThreads), 0, st, (const double*)sums, (const int*)pbad, C, pl.G,
                     nblk, o, coef, gcnt, out);
  PSEG_LAUNCH_CHECK();
  if (dlogits) {
    if (vec)
      hipLaunchKernelGGL((tversky_grad_kernel<true>), dim3((unsigned)nblk), dim3(kTvThreads), 0, st, logits, target, C, hw,
                         pl.tiles, ign, per_image, (const float*)coef, dlogits);
    else
      hipLaunchKernelGGL((tversky_grad_kernel<false>), dim3((unsigned)nblk), dim3(kTvThreads), 0, st, logits, target, C, hw,
                         pl.tiles, ign, per_image, (const float*)coef, dlogits);
    PSEG_LAUNCH_CHECK();
  }
  return PSEG_OK;
}

}  // extern "C"
