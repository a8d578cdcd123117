// Kervadec's surface (boundary-distance) loss on gfx950: the exact signed squared Euclidean distance map of a label map,
// per image and class (pseg_class_sdist), and the loss over the softmax of the logits with its gradient
// (pseg_surface_fwd_bwd).  The contracts are in include/pseg_amd.h; the design is DESIGN.md section 5l.
//
// Distance map.  For a class c the mask is M = (L == c); the squared distance to the other side of M's contour is separable:
// with s(x, y) the signed distance along COLUMN x to the nearest pixel of the other kind (negative inside M, kSdNone in
// magnitude when the column has no such pixel),
//     |sdist(x, y)| = min over x' of (x - x')^2 + f(x'),   f(x') = 0 where (x', y) is of the other kind, else s(x', y)^2.
// Four launches, integer arithmetic only:
//  - a memset of the B * C presence counters, then sdist_pack_kernel: the int64 labels become int16 (the class, or -1 for
//    every label outside [0, C)) in the workspace and are counted per (image, class) through an LDS histogram and integer
//    atomics (order-independent).  A class with 0 or H * W pixels in an image has no contour there: its plane is zeros.
//  - sdist_cols_kernel: a lane per (image, class, column).  It sweeps down the column counting the run of equal membership
//    (the distance to the change above) into sdist itself, then walks back up through what it wrote with the distance to
//    the change below and leaves s = +-min(above, below).  A lane only reads back words it wrote itself: no barrier.
//  - sdist_rows_kernel: a block owns a span of whole rows of sdist ([B][C][H][W] is row after row) that it copies to LDS as
//    int16; a thread searches outwards from its pixel and stops once k^2 reaches the best value so far (every term at
//    offset k is >= k^2), then overwrites its own word.  A row has one owner, so the map is finished in place.
// Loss.  The geometry of tversky.hip: a block of 256 threads owns 1024 consecutive pixels of one image, a lane four of
// them, sweeping the class planes.  One online sweep gives m, s = sum_c exp(z_c - m) and d = sum_c phi_c exp(z_c - m), so
// dot = sum_c phi_c p_c = d / s without p ever being formed.  surface_reduce_kernel leaves one double per block (and the
// block's counts), surface_final_kernel adds them in a fixed order and writes out[] and 1 / n_valid, surface_grad_kernel
// (only with dlogits) repeats the sweep and writes p_c (phi_c - dot) / n_valid in a second one.  No atomics.
#include "loss_common.h"

#include <math.h>

namespace pseg {

constexpr int kSdMaxSide = 16384;         // H^2 + W^2 <= 2^29
constexpr int kSdMaxClasses = 1024;
constexpr int kSdNone = 32767;            // |s| of a column without a pixel of the other kind (a distance is <= 16383)
constexpr int kSdInf = 0x7fffffff;
constexpr int kSdThreads = 256;
constexpr int kSdPackPix = 4096;          // pixels of one image per block of sdist_pack_kernel

// ------------------------------------------------------------------------------------------------ distance map
__global__ __launch_bounds__(kSdThreads) void sdist_pack_kernel(const int64_t* __restrict__ labels, int HW, int C, int chunks,
                                                                int16_t* __restrict__ packed, int* __restrict__ cnt) {
  extern __shared__ int sd_hist[];                       // [C]
  const int b = blockIdx.x / chunks, ch = blockIdx.x - b * chunks;
  for (int c = threadIdx.x; c < C; c += kSdThreads) sd_hist[c] = 0;
  __syncthreads();
  const int p0 = ch * kSdPackPix, p1 = min(HW, p0 + kSdPackPix);
  const size_t img = (size_t)b * HW;
  for (int p = p0 + threadIdx.x; p < p1; p += kSdThreads) {
    const long long t = labels[img + p];
    const bool in = t >= 0 && t < C;
    packed[img + p] = in ? (int16_t)t : (int16_t)-1;
    if (in) atomicAdd(&sd_hist[(int)t], 1);
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += kSdThreads)
    if (sd_hist[c]) atomicAdd(&cnt[b * C + c], sd_hist[c]);
}

// a class without a contour in its image
__device__ __forceinline__ bool sd_flat(int n, int HW) { return n == 0 || n == HW; }

__global__ __launch_bounds__(kSdThreads) void sdist_cols_kernel(const int16_t* __restrict__ packed, const int* __restrict__ cnt,
                                                                int H, int W, int C, int total, int* __restrict__ sdist) {
  const int g = blockIdx.x * kSdThreads + threadIdx.x;   // (image, class, column)
  if (g >= total) return;                                // (no barrier below)
  const int bc = g / W, x = g - bc * W;
  if (sd_flat(cnt[bc], H * W)) return;                   // the row pass writes the zeros
  const int b = bc / C, c = bc - b * C;
  const int16_t* lab = packed + (size_t)b * H * W + x;
  int* out = sdist + (size_t)bc * H * W + x;
  int run = kSdNone;
  bool prev = false;
#pragma unroll 4
  for (int y = 0; y < H; ++y) {
    const bool in = lab[(size_t)y * W] == c;
    if (y > 0) run = in == prev ? (run == kSdNone ? kSdNone : run + 1) : 1;
    prev = in;
    out[(size_t)y * W] = run;
  }
  run = kSdNone;
#pragma unroll 4
  for (int y = H - 1; y >= 0; --y) {
    const bool in = lab[(size_t)y * W] == c;
    const int up = out[(size_t)y * W];
    if (y < H - 1) run = in == prev ? (run == kSdNone ? kSdNone : run + 1) : 1;
    prev = in;
    const int m = min(up, run);
    out[(size_t)y * W] = in ? -m : m;
  }
}

// what a pixel of the row with column value v adds to the squared distance of a pixel on the `inside` side
__device__ __forceinline__ int sd_cost(int v, bool inside) {
  if (inside ? v > 0 : v < 0) return 0;                  // it is of the other kind itself
  const int a = v < 0 ? -v : v;
  return a == kSdNone ? kSdInf : a * a;
}

// block: rows [blockIdx.x * R, + R) of the nrows = B * C * H rows of sdist
__global__ __launch_bounds__(kSdThreads) void sdist_rows_kernel(const int* __restrict__ cnt, int H, int W, int R, int nrows,
                                                                int* sdist) {
  extern __shared__ int16_t sd_row[];                    // [R][W]
  const int row0 = blockIdx.x * R;
  const int n = min(R, nrows - row0) * W;
  int* base = sdist + (size_t)row0 * W;
  for (int i = threadIdx.x; i < n; i += kSdThreads) {
    const int r = i / W;
    sd_row[i] = sd_flat(cnt[(row0 + r) / H], H * W) ? (int16_t)0 : (int16_t)base[i];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += kSdThreads) {
    const int r = i / W, x = i - r * W;
    const int16_t* row = sd_row + r * W;
    const int s = row[x];
    int o = 0;
    if (s != 0) {                                        // (a staged value is never 0)
      const bool inside = s < 0;
      const int a = inside ? -s : s;
      int best = a == kSdNone ? kSdInf : a * a;
      for (int k = 1; k * k < best && (k <= x || x + k < W); ++k) {
        if (k <= x) {
          const int f = sd_cost(row[x - k], inside);
          if (f != kSdInf) best = min(best, k * k + f);
        }
        if (x + k < W) {
          const int f = sd_cost(row[x + k], inside);
          if (f != kSdInf) best = min(best, k * k + f);
        }
      }
      o = best == kSdInf ? 0 : (inside ? -best : best);
    }
    base[i] = o;
  }
}

struct SdPlan {
  int HW, chunks, R, nrows;
  int64_t cols, cnt, packed, bytes;      // column lanes; byte offsets into the workspace
};

static bool sd_sizes_ok(int B, int C, int H, int W) {
  if (B < 1 || H < 1 || W < 1 || C < 1 || C > kSdMaxClasses || H > kSdMaxSide || W > kSdMaxSide) return false;
  return (int64_t)B * C <= ((1ll << 31) - 1) / 4 / ((int64_t)H * W);       // B * C * H * W * 4 < 2 GiB
}

static SdPlan sd_plan(int B, int C, int H, int W) {
  SdPlan p;
  p.HW = H * W;
  p.chunks = cdiv(p.HW, kSdPackPix);
  p.R = W >= kSdThreads ? 1 : kSdThreads / W;
  p.nrows = B * C * H;
  p.cols = (int64_t)B * C * W;
  int64_t o = 0;
  p.cnt = o;    o = align256(o + (int64_t)B * C * 4);
  p.packed = o; o = align256(o + (int64_t)B * p.HW * 2);
  p.bytes = o;
  return p;
}

// ------------------------------------------------------------------------------------------------ loss
constexpr int kSfThreads = 256;
constexpr int kSfPix = 4;                               // pixels per lane
constexpr int kSfTile = kSfThreads * kSfPix;            // pixels per block

template <bool VEC>
__device__ __forceinline__ unsigned sf_pix(unsigned p0, int j) {
  return VEC ? p0 + j : p0 + j * kSfThreads;
}

// the lane's four logits of one class plane; 0 past the image
template <bool VEC>
__device__ __forceinline__ void sf_load(const float* __restrict__ plane, unsigned p0, unsigned HW, float x[kSfPix]) {
  if (VEC) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p0 < HW) v = *reinterpret_cast<const float4*>(plane + p0);      // HW % 4 == 0: the whole vector is inside
    x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
  } else {
#pragma unroll
    for (int j = 0; j < kSfPix; ++j) {
      const unsigned p = sf_pix<false>(p0, j);
      x[j] = p < HW ? plane[p] : 0.f;
    }
  }
}

__device__ __forceinline__ float sf_phi_of(int sd, float clip) {
  float f = sd > 0 ? sqrtf((float)sd) : sd < 0 ? 1.f - sqrtf((float)-sd) : 0.f;
  if (clip > 0.f) f = fminf(fmaxf(f, -clip), clip);
  return f;
}

// ... and their phi, from the signed squared distances
template <bool VEC>
__device__ __forceinline__ void sf_phi(const int* __restrict__ plane, unsigned p0, unsigned HW, float clip, float f[kSfPix]) {
  int v[kSfPix] = {0, 0, 0, 0};
  if (VEC) {
    if (p0 < HW) {
      const int4 q = *reinterpret_cast<const int4*>(plane + p0);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    }
  } else {
#pragma unroll
    for (int j = 0; j < kSfPix; ++j) {
      const unsigned p = sf_pix<false>(p0, j);
      if (p < HW) v[j] = plane[p];
    }
  }
#pragma unroll
  for (int j = 0; j < kSfPix; ++j) f[j] = sf_phi_of(v[j], clip);
}

// the lane's four labels: valid = counted by the loss; bad = in the image, not ignore_index, out of range
template <bool VEC>
__device__ __forceinline__ void sf_labels(const int64_t* __restrict__ tg, unsigned p0, unsigned HW, long long ign, int C,
                                          bool valid[kSfPix], bool bad[kSfPix]) {
#pragma unroll
  for (int j = 0; j < kSfPix; ++j) {
    const unsigned p = sf_pix<VEC>(p0, j);
    const bool in = p < HW;
    const long long t = in ? (long long)tg[p] : ign;
    valid[j] = in && ce_valid(t, ign, C);
    bad[j] = in && !valid[j] && t != ign;
  }
}

// One sweep over the classes: running max m, s = sum_c exp(z_c - m) and d = sum_c phi_c exp(z_c - m) of the four pixels
template <bool VEC>
__device__ __forceinline__ void sf_online_sweep(const float* __restrict__ img, const int* __restrict__ simg, size_t HW,
                                                unsigned p0, int C, float clip, float m[kSfPix], float s[kSfPix],
                                                float d[kSfPix]) {
#pragma unroll
  for (int j = 0; j < kSfPix; ++j) {
    m[j] = -INFINITY;
    s[j] = 0.f;
    d[j] = 0.f;
  }
#pragma unroll 2
  for (int c = 0; c < C; ++c) {
    float x[kSfPix], f[kSfPix];
    sf_load<VEC>(img + (size_t)c * HW, p0, (unsigned)HW, x);
    sf_phi<VEC>(simg + (size_t)c * HW, p0, (unsigned)HW, clip, f);
#pragma unroll
    for (int j = 0; j < kSfPix; ++j) {
      const float mn = fmaxf(m[j], x[j]);
      const float sc = __expf(m[j] - mn);       // exp(-inf) = 0 on the first class
      const float e = __expf(x[j] - mn);
      s[j] = s[j] * sc + e;
      d[j] = d[j] * sc + f[j] * e;
      m[j] = mn;
    }
  }
}

// per block: pl = sum over its valid pixels of dot, pv = their number, pb = its out-of-range targets
template <bool VEC>
__global__ __launch_bounds__(kSfThreads) void surface_reduce_kernel(const float* __restrict__ logits,
                                                                    const int64_t* __restrict__ target,
                                                                    const int* __restrict__ sdist, int C, unsigned HW,
                                                                    unsigned tiles, long long ign, float clip,
                                                                    double* __restrict__ pl, double* __restrict__ pv,
                                                                    double* __restrict__ pb) {
  __shared__ double sh[4];
  const int tid = threadIdx.x;
  const unsigned b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
  const unsigned p0 = tile * kSfTile + (VEC ? tid * kSfPix : tid);
  bool valid[kSfPix], bad[kSfPix];
  sf_labels<VEC>(target + (size_t)b * HW, p0, HW, ign, C, valid, bad);
  double acc = 0.0, nv = 0.0, nb = 0.0;
  const bool any = __ballot(valid[0] || valid[1] || valid[2] || valid[3]) != 0ull;
  if (any) {                                    // (the same in every lane of the wave)
    float m[kSfPix], s[kSfPix], d[kSfPix];
    sf_online_sweep<VEC>(logits + (size_t)b * C * HW, sdist + (size_t)b * C * HW, HW, p0, C, clip, m, s, d);
#pragma unroll
    for (int j = 0; j < kSfPix; ++j) acc += valid[j] ? (double)(d[j] / s[j]) : 0.0;
  }
#pragma unroll
  for (int j = 0; j < kSfPix; ++j) {
    nv += valid[j] ? 1.0 : 0.0;
    nb += bad[j] ? 1.0 : 0.0;
  }
  acc = block_sum_d_again(acc, sh);
  nv = block_sum_d_again(nv, sh);
  nb = block_sum_d_again(nb, sh);
  if (tid == 0) {
    pl[blockIdx.x] = acc;
    pv[blockIdx.x] = nv;
    pb[blockIdx.x] = nb;
  }
}

// one block: out[] = [loss, n_valid, n_out_of_range], inv_n[0] = 1 / n_valid (0 without a valid pixel)
__global__ __launch_bounds__(kSfThreads) void surface_final_kernel(const double* __restrict__ pl, const double* __restrict__ pv,
                                                                   const double* __restrict__ pb, int nblk,
                                                                   float* __restrict__ inv_n, float* __restrict__ out) {
  __shared__ double sh[4];
  const double sum = block_sum_d_again(thread_sum_partials(pl, nblk), sh);
  const double nv = block_sum_d_again(thread_sum_partials(pv, nblk), sh);
  const double nb = block_sum_d_again(thread_sum_partials(pb, nblk), sh);
  if (threadIdx.x == 0) {
    out[0] = nv > 0.0 ? (float)(sum / nv) : 0.f;
    out[1] = (float)nv;
    out[2] = (float)nb;
    inv_n[0] = nv > 0.0 ? (float)(1.0 / nv) : 0.f;
  }
}

template <bool VEC>
__global__ __launch_bounds__(kSfThreads) void surface_grad_kernel(const float* __restrict__ logits,
                                                                  const int64_t* __restrict__ target,
                                                                  const int* __restrict__ sdist, int C, unsigned HW,
                                                                  unsigned tiles, long long ign, float clip,
                                                                  const float* __restrict__ inv_n, float* __restrict__ dlogits) {
  const int tid = threadIdx.x;
  const unsigned b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
  const unsigned p0 = tile * kSfTile + (VEC ? tid * kSfPix : tid);
  const float* img = logits + (size_t)b * C * HW;
  const int* simg = sdist + (size_t)b * C * HW;
  float* dimg = dlogits + (size_t)b * C * HW;
  bool valid[kSfPix], bad[kSfPix];
  sf_labels<VEC>(target + (size_t)b * HW, p0, HW, ign, C, valid, bad);
  const bool any = __ballot(valid[0] || valid[1] || valid[2] || valid[3]) != 0ull;
  const float scale = inv_n[0];
  float m[kSfPix], inv[kSfPix], dot[kSfPix];
#pragma unroll
  for (int j = 0; j < kSfPix; ++j) m[j] = inv[j] = dot[j] = 0.f;
  if (any) {                                    // (the same in every lane of the wave)
    float s[kSfPix], d[kSfPix];
    sf_online_sweep<VEC>(img, simg, HW, p0, C, clip, m, s, d);
#pragma unroll
    for (int j = 0; j < kSfPix; ++j) {
      inv[j] = 1.f / s[j];
      dot[j] = d[j] * inv[j];
    }
  }
#pragma unroll 2
  for (int c = 0; c < C; ++c) {
    float o[kSfPix] = {0.f, 0.f, 0.f, 0.f};
    if (any) {
      float x[kSfPix], f[kSfPix];
      sf_load<VEC>(img + (size_t)c * HW, p0, HW, x);
      sf_phi<VEC>(simg + (size_t)c * HW, p0, HW, clip, f);
#pragma unroll
      for (int j = 0; j < kSfPix; ++j) {
        const float p = __expf(x[j] - m[j]) * inv[j];
        o[j] = valid[j] ? p * (f[j] - dot[j]) * scale : 0.f;
      }
    }
    float* dplane = dimg + (size_t)c * HW;
    if (VEC) {
      if (p0 < HW) *reinterpret_cast<float4*>(dplane + p0) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
      for (int j = 0; j < kSfPix; ++j) {
        const unsigned p = sf_pix<false>(p0, j);
        if (p < HW) dplane[p] = o[j];
      }
    }
  }
}

struct SfPlan {
  unsigned tiles;       // blocks per image
  int64_t nblk;         // blocks
  int64_t pl, pv, pb, inv_n, bytes;      // byte offsets into the workspace
};

static bool sf_sizes_ok(int B, int C, int64_t HW) {
  if (B <= 0 || C <= 0 || HW <= 0 || C > kSdMaxClasses) return false;
  if (HW > (1ll << 31) / 8 / B) return false;                            // targets: B * HW * 8 bytes
  return (int64_t)B * HW * C * 4 < (1ll << 31) && (int64_t)B * HW * 8 < (1ll << 31);
}

static SfPlan sf_plan(int B, int64_t HW) {
  SfPlan p;
  p.tiles = (unsigned)((HW + kSfTile - 1) / kSfTile);
  p.nblk = (int64_t)B * p.tiles;
  int64_t o = 0;
  p.pl = o;    o = align256(o + p.nblk * 8);
  p.pv = o;    o = align256(o + p.nblk * 8);
  p.pb = o;    o = align256(o + p.nblk * 8);
  p.inv_n = o; o = align256(o + 4);
  p.bytes = o;
  return p;
}

}  // namespace pseg

using namespace pseg;

extern "C" {

int64_t pseg_class_sdist_workspace_bytes(int B, int C, int H, int W) {
  if (!sd_sizes_ok(B, C, H, W)) return 0;
  return sd_plan(B, C, H, W).bytes;
}

int pseg_class_sdist(const int64_t* labels, int B, int H, int W, int C, int32_t* sdist, void* workspace,
                     int64_t workspace_bytes, void* stream) {
  // (the sizes first: a call with made-up sizes and no memory behind it is told about the sizes)
  PSEG_REQUIRE(B >= 1 && H >= 1 && W >= 1, "pseg_class_sdist: sizes B, H, W = %d, %d, %d must be >= 1", B, H, W);
  PSEG_REQUIRE(H <= kSdMaxSide && W <= kSdMaxSide, "pseg_class_sdist: H, W = %d, %d above %d", H, W, kSdMaxSide);
  PSEG_REQUIRE(C >= 1 && C <= kSdMaxClasses, "pseg_class_sdist: class count C = %d outside [1, %d]", C, kSdMaxClasses);
  PSEG_REQUIRE(sd_sizes_ok(B, C, H, W),
               "pseg_class_sdist: sdist at or above 2 GiB is not supported (B=%d C=%d H=%d W=%d); split the batch", B, C, H, W);
  PSEG_REQUIRE(labels && sdist && workspace, "pseg_class_sdist: null pointer (labels, sdist or workspace)");
  const SdPlan pl = sd_plan(B, C, H, W);
  PSEG_REQUIRE(workspace_bytes >= pl.bytes, "pseg_class_sdist: workspace too small (%lld < %lld bytes)",
               (long long)workspace_bytes, (long long)pl.bytes);
  PSEG_REQUIRE(((uintptr_t)workspace & 15) == 0, "pseg_class_sdist: workspace must be 16-byte aligned");
  const hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  int* cnt = (int*)(ws + pl.cnt);
  int16_t* packed = (int16_t*)(ws + pl.packed);
  if (hipMemsetAsync(cnt, 0, (size_t)B * C * 4, st) != hipSuccess) {
    set_error("pseg_class_sdist: hipMemsetAsync failed");
    return PSEG_ERR_HIP;
  }
  hipLaunchKernelGGL(sdist_pack_kernel, dim3((unsigned)(B * pl.chunks)), dim3(kSdThreads), (size_t)C * 4, st, labels, pl.HW, C,
                     pl.chunks, packed, cnt);
  PSEG_LAUNCH_CHECK();
  hipLaunchKernelGGL(sdist_cols_kernel, dim3((unsigned)cdiv(pl.cols, kSdThreads)), dim3(kSdThreads), 0, st,
                     (const int16_t*)packed, (const int*)cnt, H, W, C, (int)pl.cols, sdist);
  PSEG_LAUNCH_CHECK();
  hipLaunchKernelGGL(sdist_rows_kernel, dim3((unsigned)cdiv(pl.nrows, pl.R)), dim3(kSdThreads), (size_t)pl.R * W * 2, st,
                     (const int*)cnt, H, W, pl.R, pl.nrows, sdist);
  PSEG_LAUNCH_CHECK();
  return PSEG_OK;
}

int64_t pseg_surface_workspace_bytes(int B, int C, int64_t HW) {
  if (!sf_sizes_ok(B, C, HW)) return 0;
  return sf_plan(B, HW).bytes;
}

int pseg_surface_fwd_bwd(const float* logits, const int64_t* target, const int32_t* sdist, int B, int C, int64_t HW,
                         int64_t ignore_index, float clip, float* dlogits, float* out, void* workspace,
                         int64_t workspace_bytes, void* stream) {
  PSEG_REQUIRE(logits && target && sdist && out && workspace, "pseg_surface_fwd_bwd: null pointer");
  PSEG_REQUIRE(B > 0 && C > 0 && HW > 0, "pseg_surface_fwd_bwd: bad sizes");
  PSEG_REQUIRE(C <= kSdMaxClasses, "pseg_surface_fwd_bwd: at most %d classes (got %d)", kSdMaxClasses, C);
  PSEG_REQUIRE(sf_sizes_ok(B, C, HW),
               "pseg_surface_fwd_bwd: logits or targets at or above 2 GiB are not supported (B=%d C=%d HW=%lld); split the batch",
               B, C, (long long)HW);
  PSEG_REQUIRE(isfinite(clip) && clip >= 0.f, "pseg_surface_fwd_bwd: clip must be finite and >= 0 (got %g)", clip);
  PSEG_REQUIRE(dlogits != logits, "pseg_surface_fwd_bwd: dlogits must not alias logits");
  PSEG_REQUIRE((const void*)dlogits != (const void*)sdist, "pseg_surface_fwd_bwd: dlogits must not alias sdist");
  const SfPlan pl = sf_plan(B, HW);
  PSEG_REQUIRE(workspace_bytes >= pl.bytes, "pseg_surface_fwd_bwd: workspace too small (%lld < %lld bytes)",
               (long long)workspace_bytes, (long long)pl.bytes);
  PSEG_REQUIRE(((uintptr_t)workspace & 15) == 0, "pseg_surface_fwd_bwd: workspace must be 16-byte aligned");
  const hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  double* ppl = (double*)(ws + pl.pl);
  double* ppv = (double*)(ws + pl.pv);
  double* ppb = (double*)(ws + pl.pb);
  float* inv_n = (float*)(ws + pl.inv_n);
  const unsigned hw = (unsigned)HW;
  const unsigned nblk = (unsigned)pl.nblk;
  const long long ign = (long long)ignore_index;
  const bool vec = HW % 4 == 0 && (((uintptr_t)logits | (uintptr_t)sdist | (uintptr_t)dlogits) & 15) == 0;

  if (vec)
    hipLaunchKernelGGL((surface_reduce_kernel<true>), dim3(nblk), dim3(kSfThreads), 0, st, logits, target, (const int*)sdist, C,
                       hw, pl.tiles, ign, clip, ppl, ppv, ppb);
  else
    hipLaunchKernelGGL((surface_reduce_kernel<false>), dim3(nblk), dim3(kSfThreads), 0, st, logits, target, (const int*)sdist, C,
                       hw, pl.tiles, ign, clip, ppl, ppv, ppb);
  PSEG_LAUNCH_CHECK();
  hipLaunchKernelGGL(surface_final_kernel, dim3(1), dim3(kSfThreads), 0, st, (const double*)ppl, (const double*)ppv,
                     (const double*)ppb, (int)nblk, inv_n, out);
  PSEG_LAUNCH_CHECK();
  if (dlogits) {
    if (vec)
      hipLaunchKernelGGL((surface_grad_kernel<true>), dim3(nblk), dim3(kSfThreads), 0, st, logits, target, (const int*)sdist, C,
                         hw, pl.tiles, ign, clip, (const float*)inv_n, dlogits);
    else
      hipLaunchKernelGGL((surface_grad_kernel<false>), dim3(nblk), dim3(kSfThreads), 0, st, logits, target, (const int*)sdist, C,
                         hw, pl.tiles, ign, clip, (const float*)inv_n, dlogits);
    PSEG_LAUNCH_CHECK();
  }
  return PSEG_OK;
}

}  // extern "C"
