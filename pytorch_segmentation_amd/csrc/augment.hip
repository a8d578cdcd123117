// Training augmentation on gfx950, fused into the batch preprocess: the geometric and colour-affine part of the reference's
// online augmentation (reference utils/datasets.py:26-125, TRAIN_AUGS, applied per sample on the host by imgaug) together
// with CocoDataset.post_fetch_fn (utils/datasets.py:199-213: float, normalise, multi-scale nearest resize, labels to int64),
// in ONE launch over the uint8 batch the loader collates.
//  - image blocks: a 64x4 tile of the fp32 output [B,3,oh,ow].  A thread owns one output pixel for the three planes: the
//    multi-scale index (ATen's nearest), the source coordinate (the sample's inverse affine, fp32) and the tap addresses
//    are computed once; 3 (nearest) or 12 (bilinear) byte loads; the warped value is rounded to 8 bits half up (imgaug
//    hands a uint8 image from one augmenter to the next), the 3x4 colour matrix is applied and rounded the same way, then
//    (q - mean[c]) / std[c] with a correctly rounded division, as image_preprocess_kernel (infer.hip).  A wave stores 64
//    consecutive floats of one output row per plane.
//  - label blocks: a 64x4 tile of the int64 target [B,H,W]: the same affine, nearest sample, 0 outside the image.
// Both ranges live in one 1-D grid (the step is launch-bound): blocks [0, n_img) are image tiles, the rest label tiles.
// Every load index is clamped into its plane and the value is replaced AFTER the load where the tap lies outside, so
// nothing outside img / seg is read whatever the table holds.  Identity rows reproduce post_fetch_fn bit for bit.
#include "common.h"

#include <math.h>

namespace pseg {

constexpr int kAugTileW = 64, kAugTileH = 4;

struct AugNorm {
  float mean[3], std[3];
};

struct AugCoord {
  float sx, sy;
  bool finite;
};

// Philox4x32-10 with counter (c0, c1, 0, 0) and key (k0, k1): the random numbers of the nbhd / warp kernels (below)
struct Philox4 {
  uint32_t v[4];
};

__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t k0, uint32_t k1) {
  uint32_t c2 = 0u, c3 = 0u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Philox4{{c0, c1, c2, c3}};
}

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

constexpr uint32_t kStreamElastic = 8;                    // streams 0..6: noise and dropout (below)

// source index coordinate of working-grid pixel (x, y): pixel centres at integers.  Clamped to [-1, size] BEFORE any
// float -> int conversion: a coordinate beyond that range behaves exactly like the bound itself (every tap outside the
// image in constant mode, the edge pixel in edge mode).  A NaN / infinite coordinate is reported and counts as outside.
// kWarp (pseg_augment_batch_warp's row): elastic jitter -> 4 x 4 displacement grid -> homography in front of that, a pure
// function of (x, y) and the row; with the three fields off, the same sx, sy bit for bit (the division is by 1.0f).
template <bool kWarp>
__device__ __forceinline__ AugCoord aug_coord(const float* __restrict__ row, int x, int y, int H, int W) {
  float px = (float)x, py = (float)y, den = 1.f;
  if constexpr (kWarp) {
    const float alpha = row[PSEG_AUGMENT_WARP_ALPHA];
    if (alpha > 0.f && alpha <= 3.0e38f) {                  // sample-uniform
      const Philox4 r = philox4x32_10((uint32_t)y * (uint32_t)W + (uint32_t)x, kStreamElastic,
                                      __float_as_uint(row[PSEG_AUGMENT_NBHD_SEED]), __float_as_uint(row[PSEG_AUGMENT_NBHD_SEED + 1]));
      px = fmaf(alpha, fmaf(2.f, (float)(r.v[0] >> 8) * 0x1p-24f, -1.f), px);
      py = fmaf(alpha, fmaf(2.f, (float)(r.v[1] >> 8) * 0x1p-24f, -1.f), py);
    }
    if (row[PSEG_AUGMENT_WARP_GRID_ON] != 0.f) {
      // clamped before the conversion: the cell lies in 0..2 and the eight loads inside the row, whatever px, py are
      const float gu = W > 1 ? fminf(fmaxf(px * (3.f / (float)(W - 1)), 0.f), 3.f) : 0.f;
      const float gv = H > 1 ? fminf(fmaxf(py * (3.f / (float)(H - 1)), 0.f), 3.f) : 0.f;
      const int i0 = clampi((int)gu, 2), j0 = clampi((int)gv, 2);
      const float fu = gu - (float)i0, fv = gv - (float)j0;
      const float* __restrict__ n = row + PSEG_AUGMENT_WARP_GRID + 2 * (4 * j0 + i0);   // nodes (j0, i0), (j0, i0 + 1); + 8: row j0 + 1
      const float tx = fmaf(fu, n[2] - n[0], n[0]), ty = fmaf(fu, n[3] - n[1], n[1]);
      const float bx = fmaf(fu, n[10] - n[8], n[8]), by = fmaf(fu, n[11] - n[9], n[9]);
      px += fmaf(fv, bx - tx, tx);
      py += fmaf(fv, by - ty, ty);
    }
    den = fmaf(row[PSEG_AUGMENT_WARP_H2], px, fmaf(row[PSEG_AUGMENT_WARP_H2 + 1], py, row[PSEG_AUGMENT_WARP_H2 + 2]));
  }
  float sx = fmaf(row[0], px, fmaf(row[1], py, row[2]));
  float sy = fmaf(row[3], px, fmaf(row[4], py, row[5]));
  if constexpr (kWarp) sx = sx / den, sy = sy / den;        // correctly rounded
  AugCoord c;
  c.finite = fabsf(sx) <= 3.0e38f && fabsf(sy) <= 3.0e38f;   // false for NaN and +-inf
  if constexpr (kWarp) c.finite = c.finite && den > 0.f;    // behind the camera, or a NaN denominator: outside
  c.sx = c.finite ? fminf(fmaxf(sx, -1.f), (float)W) : -1.f;
  c.sy = c.finite ? fminf(fmaxf(sy, -1.f), (float)H) : -1.f;
  return c;
}

__device__ __forceinline__ float round_u8(float v) {      // 8-bit result, half up, saturated
  float q = floorf(v + 0.5f);
  return q < 0.f ? 0.f : (q > 255.f ? 255.f : q);
}

__global__ __launch_bounds__(256) void augment_batch_kernel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ seg,
                                                            const float* __restrict__ params, AugNorm nm, float* __restrict__ out,
                                                            int64_t* __restrict__ target, int H, int W, int oh, int ow,
                                                            uint32_t n_img, uint32_t img_tiles_x, uint32_t img_tiles,
                                                            uint32_t lab_tiles_x, uint32_t lab_tiles) {
  const int tx = threadIdx.x & (kAugTileW - 1), ty = threadIdx.x / kAugTileW;
  const bool is_img = blockIdx.x < n_img;
  const uint32_t blk = is_img ? blockIdx.x : blockIdx.x - n_img;
  const uint32_t per = is_img ? img_tiles : lab_tiles, per_x = is_img ? img_tiles_x : lab_tiles_x;
  const uint32_t b = blk / per, t = blk - b * per;
  const uint32_t tyi = t / per_x, txi = t - tyi * per_x;
  const int ox = (int)txi * kAugTileW + tx, oy = (int)tyi * kAugTileH + ty;
  const float* __restrict__ row = params + (int64_t)b * PSEG_AUGMENT_ROW;
  const int64_t plane = (int64_t)H * W;

  if (!is_img) {                                           // ---- labels: [H, W], nearest, 0 outside
    if (ox >= W || oy >= H) return;
    const AugCoord c = aug_coord<false>(row, ox, oy, H, W);
    const int x = (int)floorf(c.sx + 0.5f), y = (int)floorf(c.sy + 0.5f);
    const bool inside = c.finite && x >= 0 && x < W && y >= 0 && y < H;
    const uint8_t v = seg[(int64_t)b * plane + (int64_t)clampi(y, H - 1) * W + clampi(x, W - 1)];
    target[(int64_t)b * plane + (int64_t)oy * W + ox] = inside ? (int64_t)v : 0;
    return;
  }

  if (ox >= ow || oy >= oh) return;
  // multi-scale: ATen's nearest source index (identity when (oh, ow) == (H, W))
  const int ix = min((int)floorf((float)ox * ((float)W / (float)ow)), W - 1);
  const int iy = min((int)floorf((float)oy * ((float)H / (float)oh)), H - 1);
  const AugCoord c = aug_coord<false>(row, ix, iy, H, W);
  const float cval = row[18];
  const bool bilinear = row[19] != 0.f, edge = row[20] != 0.f && c.finite;
  const uint8_t* __restrict__ p = img + (int64_t)b * 3 * plane;
  float v[3];
  if (!bilinear) {                                         // block-uniform branch: the row is the sample's
    const int x = (int)floorf(c.sx + 0.5f), y = (int)floorf(c.sy + 0.5f);
    const bool use = edge || (c.finite && x >= 0 && x < W && y >= 0 && y < H);
    const int64_t at = (int64_t)clampi(y, H - 1) * W + clampi(x, W - 1);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float s = (float)p[k * plane + at];
      v[k] = use ? s : cval;
    }
  } else {
    const float fx0 = floorf(c.sx), fy0 = floorf(c.sy);
    const int x0 = (int)fx0, y0 = (int)fy0, x1 = x0 + 1, y1 = y0 + 1;
    const float lx1 = c.sx - fx0, lx0 = 1.f - lx1, ly1 = c.sy - fy0, ly0 = 1.f - ly1;
    const bool in_x0 = x0 >= 0 && x0 < W, in_x1 = x1 >= 0 && x1 < W, in_y0 = y0 >= 0 && y0 < H, in_y1 = y1 >= 0 && y1 < H;
    const bool u00 = edge || (c.finite && in_y0 && in_x0), u01 = edge || (c.finite && in_y0 && in_x1);
    const bool u10 = edge || (c.finite && in_y1 && in_x0), u11 = edge || (c.finite && in_y1 && in_x1);
    const int cx0 = clampi(x0, W - 1), cx1 = clampi(x1, W - 1);
    const int64_t r0 = (int64_t)clampi(y0, H - 1) * W, r1 = (int64_t)clampi(y1, H - 1) * W;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const uint8_t* q = p + k * plane;
      const float s00 = (float)q[r0 + cx0], s01 = (float)q[r0 + cx1], s10 = (float)q[r1 + cx0], s11 = (float)q[r1 + cx1];
      const float p00 = u00 ? s00 : cval, p01 = u01 ? s01 : cval, p10 = u10 ? s10 : cval, p11 = u11 ? s11 : cval;
      v[k] = ly0 * (lx0 * p00 + lx1 * p01) + ly1 * (lx0 * p10 + lx1 * p11);
    }
  }
  const float r = round_u8(v[0]), g = round_u8(v[1]), bl = round_u8(v[2]);
  const int64_t oplane = (int64_t)oh * ow;
  float* o = out + (int64_t)b * 3 * oplane + (int64_t)oy * ow + ox;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float* m = row + 6 + 4 * k;
    const float q = round_u8(fmaf(m[0], r, fmaf(m[1], g, fmaf(m[2], bl, m[3]))));
    o[k * oplane] = (q - nm.mean[k]) / nm.std[k];
  }
}


// ---------------------------------------------------------------------------------------------------------------------
// The same preprocess with a neighbourhood stage and per-pixel random stages (pseg_augment_batch_nbhd): per sample, on
// the working grid, warp -> K x K correlation filter -> colour matrix -> Gaussian noise -> dropout -> normalise, 8-bit
// rounding after each of the first four (row layout and contract: include/pseg_amd.h).
//  - image blocks: a 32x8 tile of the output.  With a filter (K >= 3, per sample and hence block-uniform) the block first
//    evaluates the warp ONCE per working-grid pixel of the span its output pixels map to, plus a halo of K/2 (indices
//    beyond the grid reflect without repeating the edge pixel; a reflected halo pixel is evaluated again), and keeps the
//    three rounded bytes packed in one LDS dword per pixel: a tap is one ds_read_b32 for the three planes, a wave's lanes
//    read consecutive dwords (its two rows lie in different 32-lane halves, which never conflict).  Filter weights are
//    block-uniform loads from the sample's row.  Without a filter the thread evaluates its own pixel and LDS is not used.
//  - label blocks: exactly augment_batch_kernel's.
// Random numbers: Philox4x32-10, key = the row's 64-bit seed, counter = (working-grid pixel or mask cell, stream, 0, 0).
constexpr int kNbTileW = 32, kNbTileH = 8;
constexpr uint32_t kStreamNoise = 0, kStreamDrop = 4;      // + the channel where the draw is per channel

// ATen's nearest source index of output index o (fp32, as augment_batch_kernel); also evaluated on the host to size LDS
__host__ __device__ __forceinline__ int aug_ms_index(int o, int in, int on) {
  const int i = (int)floorf((float)o * ((float)in / (float)on));
  return i < in - 1 ? i : in - 1;
}

// cv2's BORDER_REFLECT_101: -1 -> 1, n -> n - 2; the only pixel when n == 1
__device__ __forceinline__ int reflect101(int i, int n) {
  if (n == 1) return 0;
  while ((unsigned)i >= (unsigned)n) i = i < 0 ? -i : 2 * n - 2 - i;
  return i;
}

// the warp of augment_batch_kernel for working-grid pixel (ix, iy): three values before the 8-bit rounding
template <bool kWarp>
__device__ __forceinline__ void aug_warp(const uint8_t* __restrict__ p, const float* __restrict__ row, int ix, int iy, int H, int W,
                                         int64_t plane, float v[3]) {
  const AugCoord c = aug_coord<kWarp>(row, ix, iy, H, W);
  const float cval = row[18];
  const bool bilinear = row[19] != 0.f, edge = row[20] != 0.f && c.finite;
  if (!bilinear) {
    const int x = (int)floorf(c.sx + 0.5f), y = (int)floorf(c.sy + 0.5f);
    const bool use = edge || (c.finite && x >= 0 && x < W && y >= 0 && y < H);
    const int64_t at = (int64_t)clampi(y, H - 1) * W + clampi(x, W - 1);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float s = (float)p[k * plane + at];
      v[k] = use ? s : cval;
    }
  } else {
    const float fx0 = floorf(c.sx), fy0 = floorf(c.sy);
    const int x0 = (int)fx0, y0 = (int)fy0, x1 = x0 + 1, y1 = y0 + 1;
    const float lx1 = c.sx - fx0, lx0 = 1.f - lx1, ly1 = c.sy - fy0, ly0 = 1.f - ly1;
    const bool in_x0 = x0 >= 0 && x0 < W, in_x1 = x1 >= 0 && x1 < W, in_y0 = y0 >= 0 && y0 < H, in_y1 = y1 >= 0 && y1 < H;
    const bool u00 = edge || (c.finite && in_y0 && in_x0), u01 = edge || (c.finite && in_y0 && in_x1);
    const bool u10 = edge || (c.finite && in_y1 && in_x0), u11 = edge || (c.finite && in_y1 && in_x1);
    const int cx0 = clampi(x0, W - 1), cx1 = clampi(x1, W - 1);
    const int64_t r0 = (int64_t)clampi(y0, H - 1) * W, r1 = (int64_t)clampi(y1, H - 1) * W;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const uint8_t* q = p + k * plane;
      const float s00 = (float)q[r0 + cx0], s01 = (float)q[r0 + cx1], s10 = (float)q[r1 + cx0], s11 = (float)q[r1 + cx1];
      const float p00 = u00 ? s00 : cval, p01 = u01 ? s01 : cval, p10 = u10 ? s10 : cval, p11 = u11 ? s11 : cval;
      v[k] = ly0 * (lx0 * p00 + lx1 * p01) + ly1 * (lx0 * p10 + lx1 * p11);
    }
  }
}

// pseg_augment_batch_blend's stages (kBlend; contract: include/pseg_amd.h).  The sample of a 16 x 16 mask table at working-grid
// pixel (x, y): the clamp comes before the float -> int conversion, so the four loads stay inside the table
__device__ __forceinline__ float aug_mask(const float* __restrict__ T, int x, int y, int H, int W) {
  const float gx = fminf(fmaxf(fmaf((float)x + 0.5f, 16.f / (float)W, -0.5f), 0.f), 15.f);
  const float gy = fminf(fmaxf(fmaf((float)y + 0.5f, 16.f / (float)H, -0.5f), 0.f), 15.f);
  const int i0 = clampi((int)gx, 14), j0 = clampi((int)gy, 14);
  const float fu = gx - (float)i0, fv = gy - (float)j0;
  const float* __restrict__ n = T + PSEG_AUGMENT_BLEND_TABLE * j0 + i0;
  const float t = fmaf(fu, n[1] - n[0], n[0]);
  const float b = fmaf(fu, n[PSEG_AUGMENT_BLEND_TABLE + 1] - n[PSEG_AUGMENT_BLEND_TABLE], n[PSEG_AUGMENT_BLEND_TABLE]);
  const float m = fmaf(fv, b - t, t);
  return m > 0.f ? (m < 1.f ? m : 1.f) : 0.f;             // NaN -> 0
}

// K x K correlation over a packed tile, the accumulation order of pseg_augment_batch_nbhd; win: the window's top-left tap
__device__ __forceinline__ void aug_correlate(const uint32_t* __restrict__ win, int stride, int K, const float* __restrict__ wt, float v[3]) {
  float a0 = 0.f, a1 = 0.f, a2 = 0.f;
  for (int j = 0; j < K; ++j) {
    for (int i = 0; i < K; ++i) {
      const float wji = wt[j * K + i];
      const uint32_t px = win[j * stride + i];
      a0 = fmaf(wji, (float)(px & 0xffu), a0);
      a1 = fmaf(wji, (float)((px >> 8) & 0xffu), a1);
      a2 = fmaf(wji, (float)((px >> 16) & 0xffu), a2);
    }
  }
  v[0] = round_u8(a0), v[1] = round_u8(a1), v[2] = round_u8(a2);
}

// the median of the k x k window of packed pixels, three planes at once: bisection on the 8-bit value, eight rounds of
// counting the taps <= mid per plane (no per-thread array, no scratch); rank = (k * k - 1) / 2
__device__ __forceinline__ uint32_t aug_median(const uint32_t* __restrict__ win, int stride, int k) {
  const int need = (k * k - 1) / 2 + 1;
  int lo0 = 0, lo1 = 0, lo2 = 0, hi0 = 255, hi1 = 255, hi2 = 255;
#pragma unroll 1
  for (int round = 0; round < 8; ++round) {
    const int m0 = (lo0 + hi0) >> 1, m1 = (lo1 + hi1) >> 1, m2 = (lo2 + hi2) >> 1;
    int c0 = 0, c1 = 0, c2 = 0;
    for (int j = 0; j < k; ++j) {
      for (int i = 0; i < k; ++i) {
        const uint32_t px = win[j * stride + i];
        c0 += (int)(px & 0xffu) <= m0;
        c1 += (int)((px >> 8) & 0xffu) <= m1;
        c2 += (int)((px >> 16) & 0xffu) <= m2;
      }
    }
    if (c0 >= need) hi0 = m0; else lo0 = m0 + 1;
    if (c1 >= need) hi1 = m1; else lo1 = m1 + 1;
    if (c2 >= need) hi2 = m2; else lo2 = m2 + 1;
  }
  return (uint32_t)lo0 | ((uint32_t)lo1 << 8) | ((uint32_t)lo2 << 16);
}

// stage 5 of pseg_augment_batch_blend on the 8-bit values q[3]
__device__ __forceinline__ void aug_hue_sat(float q[3], float dh, float ds) {
  const float r = q[0], g = q[1], b = q[2];
  const float mx = fmaxf(r, fmaxf(g, b)), mn = fminf(r, fminf(g, b)), d = mx - mn;
  const float s = mx > 0.f ? d / mx : 0.f;
  float h = 0.f;
  if (d != 0.f) {
    if (mx == r) {
      h = (g - b) / d;
      h = h < 0.f ? h + 6.f : h;
    } else if (mx == g) {
      h = 2.f + (b - r) / d;
    } else {
      h = 4.f + (r - g) / d;
    }
  }
  float hp = h + dh;
  hp -= 6.f * floorf(hp / 6.f);
  if (!(hp >= 0.f && hp < 6.f)) hp = 0.f;                  // lands on 6; or a dh so large that the wrap is all rounding error
  const float sp = fminf(fmaxf(s + ds, 0.f), 1.f);
  const int i = min((int)hp, 5);
  const float f = hp - (float)i;
  const float p = mx * (1.f - sp), qq = mx * (1.f - sp * f), t = mx * (1.f - sp * (1.f - f));
  const float nr = i == 0 || i == 5 ? mx : (i == 1 ? qq : (i == 4 ? t : p));
  const float ng = i == 1 || i == 2 ? mx : (i == 0 ? t : (i == 3 ? qq : p));
  const float nb = i == 3 || i == 4 ? mx : (i == 2 ? t : (i == 5 ? qq : p));
  q[0] = round_u8(nr), q[1] = round_u8(ng), q[2] = round_u8(nb);
}

// one kernel for pseg_augment_batch_nbhd (kWarp = false), pseg_augment_batch_warp (true) and pseg_augment_batch_blend (true,
// kBlend): the first two differ in the row length and in aug_coord, which the halo fill evaluates at the REFLECTED pixel's
// index and the label blocks on [H, W]; kBlend is the warp kernel's body plus the median, the second filter, the second
// colour matrix and the hue / saturation shift, all sample- and hence block-uniform branches.  Its LDS holds the stage-1 tile
// with a halo of kmed/2 + max(K/2, K2/2) and, behind it, with a median, the stage-2 tile with a halo of max(K/2, K2/2)
template <bool kWarp, bool kBlend>
__global__ __launch_bounds__(256) void augment_batch_nbhd_kernel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ seg,
                                                                 const float* __restrict__ params, AugNorm nm, float* __restrict__ out,
                                                                 int64_t* __restrict__ target, int H, int W, int oh, int ow,
                                                                 uint32_t n_img, uint32_t img_tiles_x, uint32_t img_tiles,
                                                                 uint32_t lab_tiles_x, uint32_t lab_tiles, int halo_max,
                                                                 uint32_t lds_elems) {
  extern __shared__ uint32_t aug_tile[];                   // [span_h][span_w] of r | g << 8 | b << 16
  const bool is_img = blockIdx.x < n_img;
  const uint32_t blk = is_img ? blockIdx.x : blockIdx.x - n_img;
  const uint32_t per = is_img ? img_tiles : lab_tiles, per_x = is_img ? img_tiles_x : lab_tiles_x;
  const uint32_t b = blk / per, t = blk - b * per;
  const uint32_t tyi = t / per_x, txi = t - tyi * per_x;
  const float* __restrict__ row = params + (int64_t)b * (kBlend ? PSEG_AUGMENT_BLEND_ROW : kWarp ? PSEG_AUGMENT_WARP_ROW : PSEG_AUGMENT_NBHD_ROW);
  const int64_t plane = (int64_t)H * W;

  if (!is_img) {                                           // ---- labels: [H, W], nearest, 0 outside
    const int ox = (int)txi * kAugTileW + (threadIdx.x & (kAugTileW - 1)), oy = (int)tyi * kAugTileH + threadIdx.x / kAugTileW;
    if (ox >= W || oy >= H) return;
    const AugCoord c = aug_coord<kWarp>(row, ox, oy, H, W);
    const int x = (int)floorf(c.sx + 0.5f), y = (int)floorf(c.sy + 0.5f);
    const bool inside = c.finite && x >= 0 && x < W && y >= 0 && y < H;
    const uint8_t v = seg[(int64_t)b * plane + (int64_t)clampi(y, H - 1) * W + clampi(x, W - 1)];
    target[(int64_t)b * plane + (int64_t)oy * W + ox] = inside ? (int64_t)v : 0;
    return;
  }

  const int ox0 = (int)txi * kNbTileW, oy0 = (int)tyi * kNbTileH;
  const int ox = ox0 + (threadIdx.x & (kNbTileW - 1)), oy = oy0 + threadIdx.x / kNbTileW;
  const bool live = ox < ow && oy < oh;
  const uint8_t* __restrict__ p = img + (int64_t)b * 3 * plane;
  // working-grid pixel of this thread (a dead thread takes the tile's first: it only helps to fill LDS)
  const int ix = aug_ms_index(live ? ox : ox0, W, ow), iy = aug_ms_index(live ? oy : oy0, H, oh);

  // K of the sample; whatever the table holds, the halo stays inside what the host sized LDS for and the weights inside the row
  const float kf = row[PSEG_AUGMENT_NBHD_K];
  int k2 = (kf >= 2.f && kf <= (float)PSEG_AUGMENT_NBHD_KMAX) ? (int)kf / 2 : 0;
  k2 = min(k2, halo_max);
  // the span of working-grid pixels the tile's outputs map to (the index is monotone in the output index)
  const int gx0 = aug_ms_index(ox0, W, ow), gx1 = aug_ms_index(min(ox0 + kNbTileW, ow) - 1, W, ow);
  const int gy0 = aug_ms_index(oy0, H, oh), gy1 = aug_ms_index(min(oy0 + kNbTileH, oh) - 1, H, oh);
  const int sw = gx1 - gx0 + 1 + 2 * k2, sh = gy1 - gy0 + 1 + 2 * k2;
  if ((uint64_t)sw * (uint64_t)sh > lds_elems) k2 = 0;              // cannot happen with the host's sizing; never write past LDS

  float v[3];
  if constexpr (kBlend) {
    // the median's halo hm and the second filter's g2, clamped like K; the two tiles must fit what the host sized
    const float kmf = row[PSEG_AUGMENT_BLEND_KMED], k2f = row[PSEG_AUGMENT_BLEND_K2];
    int hm = (kmf >= 3.f && kmf <= (float)PSEG_AUGMENT_BLEND_KMEDMAX) ? (int)kmf / 2 : 0;
    int g2 = (k2f >= 3.f && k2f <= (float)PSEG_AUGMENT_BLEND_K2MAX) ? (int)k2f / 2 : 0;
    const int span_w = gx1 - gx0 + 1, span_h = gy1 - gy0 + 1;
    {
      const uint64_t hf = (uint64_t)max(k2, g2), ht = (uint64_t)hm + hf;
      const uint64_t need = (span_w + 2 * ht) * (span_h + 2 * ht) + (hm ? (span_w + 2 * hf) * (span_h + 2 * hf) : 0);
      if (need > lds_elems) hm = 0, g2 = 0, k2 = 0;                     // cannot happen with the host's sizing; never write past LDS
    }
    const int hf = max(k2, g2), ht = hm + hf;
    if (ht == 0) {
      aug_warp<kWarp>(p, row, ix, iy, H, W, plane, v);
      v[0] = round_u8(v[0]), v[1] = round_u8(v[1]), v[2] = round_u8(v[2]);
    } else {
      // stage 1 at working-grid pixels [g0 - ht, g1 + ht]
      const int sw1 = span_w + 2 * ht, sh1 = span_h + 2 * ht;
      for (int i = threadIdx.x; i < sw1 * sh1; i += 256) {
        const int ly = i / sw1, lx = i - ly * sw1;
        float w[3];
        aug_warp<kWarp>(p, row, reflect101(gx0 - ht + lx, W), reflect101(gy0 - ht + ly, H), H, W, plane, w);
        aug_tile[i] = (uint32_t)round_u8(w[0]) | ((uint32_t)round_u8(w[1]) << 8) | ((uint32_t)round_u8(w[2]) << 16);
      }
      __syncthreads();
      const uint32_t* __restrict__ src = aug_tile;
      int stride = sw1;
      if (hm) {
        // stage 2 at [g0 - hf, g1 + hf], behind the first tile.  The window of a pixel beyond the grid, taken from the first
        // tile, is the mirror image of the window of the reflected pixel (the reflection is even about 0 and about n - 1 and
        // has the period 2 n - 2), and a median does not see the order of its taps: the value IS the reflected pixel's
        uint32_t* __restrict__ med = aug_tile + sw1 * sh1;
        const int sw2 = span_w + 2 * hf, sh2 = span_h + 2 * hf;
        for (int i = threadIdx.x; i < sw2 * sh2; i += 256) {
          const int ly = i / sw2, lx = i - ly * sw2;
          med[i] = aug_median(aug_tile + ly * sw1 + lx, sw1, 2 * hm + 1);
        }
        __syncthreads();
        src = med, stride = sw2;
      }
      if (!live) return;
      const uint32_t* __restrict__ centre = src + (iy - gy0 + hf) * stride + (ix - gx0 + hf);
      const uint32_t px = *centre;
      v[0] = (float)(px & 0xffu), v[1] = (float)((px >> 8) & 0xffu), v[2] = (float)((px >> 16) & 0xffu);
      if (k2) aug_correlate(centre - k2 * stride - k2, stride, 2 * k2 + 1, row + PSEG_AUGMENT_NBHD_WEIGHTS, v);
      if (g2) {
        float e[3];
        aug_correlate(centre - g2 * stride - g2, stride, 2 * g2 + 1, row + PSEG_AUGMENT_BLEND_WEIGHTS2, e);
        const float m1 = aug_mask(row + PSEG_AUGMENT_BLEND_T1, ix, iy, H, W);
        v[0] = round_u8(fmaf(m1, e[0] - v[0], v[0])), v[1] = round_u8(fmaf(m1, e[1] - v[1], v[1])), v[2] = round_u8(fmaf(m1, e[2] - v[2], v[2]));
      }
    }
  } else if (k2 == 0) {
    aug_warp<kWarp>(p, row, ix, iy, H, W, plane, v);
    v[0] = round_u8(v[0]), v[1] = round_u8(v[1]), v[2] = round_u8(v[2]);
  } else {
    for (int i = threadIdx.x; i < sw * sh; i += 256) {
      const int ly = i / sw, lx = i - ly * sw;
      float w[3];
      aug_warp<kWarp>(p, row, reflect101(gx0 - k2 + lx, W), reflect101(gy0 - k2 + ly, H), H, W, plane, w);
      aug_tile[i] = (uint32_t)round_u8(w[0]) | ((uint32_t)round_u8(w[1]) << 8) | ((uint32_t)round_u8(w[2]) << 16);
    }
    __syncthreads();
    if (!live) return;
    const int K = 2 * k2 + 1;
    const uint32_t* __restrict__ win = aug_tile + (iy - gy0) * sw + (ix - gx0);   // the window's top-left tap
    const float* __restrict__ wt = row + PSEG_AUGMENT_NBHD_WEIGHTS;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int j = 0; j < K; ++j) {
      for (int i = 0; i < K; ++i) {
        const float wji = wt[j * K + i];
        const uint32_t px = win[j * sw + i];
        a0 = fmaf(wji, (float)(px & 0xffu), a0);
        a1 = fmaf(wji, (float)((px >> 8) & 0xffu), a1);
        a2 = fmaf(wji, (float)((px >> 16) & 0xffu), a2);
      }
    }
    v[0] = round_u8(a0), v[1] = round_u8(a1), v[2] = round_u8(a2);
  }
  if (!live) return;

  // noise and dropout of the working-grid pixel
  const uint32_t seed_lo = __float_as_uint(row[PSEG_AUGMENT_NBHD_SEED]), seed_hi = __float_as_uint(row[PSEG_AUGMENT_NBHD_SEED + 1]);
  const uint32_t pix = (uint32_t)iy * (uint32_t)W + (uint32_t)ix;
  const float nscale = row[PSEG_AUGMENT_NBHD_NOISE];
  const bool noisy = nscale > 0.f && nscale <= 3.0e38f, noise_pc = row[PSEG_AUGMENT_NBHD_NOISE + 1] != 0.f;
  const float drop_p = row[PSEG_AUGMENT_NBHD_DROP];
  const bool dropping = drop_p > 0.f, drop_pc = row[PSEG_AUGMENT_NBHD_DROP + 1] != 0.f;
  const uint32_t mh = (uint32_t)fminf(fmaxf(row[PSEG_AUGMENT_NBHD_DROP + 2], 0.f), 65535.f);
  const uint32_t mw = (uint32_t)fminf(fmaxf(row[PSEG_AUGMENT_NBHD_DROP + 3], 0.f), 65535.f);
  const uint32_t cell = (mh && mw) ? ((uint32_t)iy * mh / (uint32_t)H) * mw + (uint32_t)ix * mw / (uint32_t)W : pix;

  const int64_t oplane = (int64_t)oh * ow;
  float* o = out + (int64_t)b * 3 * oplane + (int64_t)oy * ow + ox;
  float n_shared = 0.f;
  bool keep_shared = true;
  float qc[3];
  if constexpr (kBlend) {                                  // stages 4 and 5: the two colour matrices, hue and saturation
    const bool blend = row[PSEG_AUGMENT_BLEND_COLOUR_ON] != 0.f;
    const float m2 = blend ? aug_mask(row + PSEG_AUGMENT_BLEND_T2, ix, iy, H, W) : 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float* m = row + 6 + 4 * k;
      qc[k] = round_u8(fmaf(m[0], v[0], fmaf(m[1], v[1], fmaf(m[2], v[2], m[3]))));
      if (blend) {
        const float* mb = row + PSEG_AUGMENT_BLEND_MB + 4 * k;
        const float qb = round_u8(fmaf(mb[0], v[0], fmaf(mb[1], v[1], fmaf(mb[2], v[2], mb[3]))));
        qc[k] = round_u8(fmaf(m2, qc[k] - qb, qb));
      }
    }
    const float dh = row[PSEG_AUGMENT_BLEND_HUE], ds = row[PSEG_AUGMENT_BLEND_HUE + 1];
    if (fabsf(dh) <= 3.0e38f && fabsf(ds) <= 3.0e38f && (dh != 0.f || ds != 0.f)) aug_hue_sat(qc, dh, ds);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float* m = row + 6 + 4 * k;
    float q;
    if constexpr (kBlend) q = qc[k];
    else q = round_u8(fmaf(m[0], v[0], fmaf(m[1], v[1], fmaf(m[2], v[2], m[3]))));
    if (noisy) {
      if (k == 0 || noise_pc) {
        const Philox4 r = philox4x32_10(pix, kStreamNoise + (uint32_t)k, seed_lo, seed_hi);
        const float u1 = (float)((r.v[0] >> 8) + 1u) * 0x1p-24f, u2 = (float)(r.v[1] >> 8) * 0x1p-24f;
        n_shared = sqrtf(-2.f * logf(u1)) * cosf(6.283185307179586f * u2);
      }
      q = round_u8(fmaf(nscale, n_shared, q));
    }
    if (dropping) {
      if (k == 0 || drop_pc) {
        const Philox4 r = philox4x32_10(cell, kStreamDrop + (uint32_t)k, seed_lo, seed_hi);
        keep_shared = (float)(r.v[0] >> 8) * 0x1p-24f >= drop_p;
      }
      q = keep_shared ? q : 0.f;
    }
    o[k * oplane] = (q - nm.mean[k]) / nm.std[k];
  }
}

}  // namespace pseg

using namespace pseg;

// pseg_augment_batch_nbhd, pseg_augment_batch_warp and pseg_augment_batch_blend: the same arguments, checks, launch geometry
// and LDS sizing; cols = the columns of shape_host: 3 = {K, mh, mw}, or 5 with {kmed, K2} behind them (the blend kernel)
static int augment_nbhd_launch(const char* what, bool warp, int cols, const uint8_t* img, const uint8_t* seg, const float* params,
                               const int* shape_host, int B, int H, int W, const AugNorm& nm, float* out, int oh, int ow,
                               int64_t* target, void* stream) {
  const bool blend = cols == 5;
  PSEG_REQUIRE(img && seg && params && shape_host && out && target, "%s: null pointer", what);
  PSEG_REQUIRE(B >= 1 && B <= 65535, "%s: batch %d outside [1, 65535]", what, B);
  PSEG_REQUIRE(H >= 1 && H <= 65535 && W >= 1 && W <= 65535, "%s: input size %dx%d outside [1, 65535]", what, H, W);
  PSEG_REQUIRE(oh >= 1 && oh <= 65535 && ow >= 1 && ow <= 65535, "%s: output size %dx%d outside [1, 65535]", what, oh, ow);
  PSEG_REQUIRE(nm.std[0] != 0.f && nm.std[1] != 0.f && nm.std[2] != 0.f, "%s: std must be non-zero", what);
  int kmax = 0;
  bool any_halo = false;
  for (int b = 0; b < B; ++b) {
    const int K = shape_host[cols * b], mh = shape_host[cols * b + 1], mw = shape_host[cols * b + 2];
    PSEG_REQUIRE(K >= 0 && K <= PSEG_AUGMENT_NBHD_KMAX && (K <= 1 || (K & 1)),
                 "%s: sample %d: filter size %d is not 0, 1 or an odd number up to %d", what, b, K, PSEG_AUGMENT_NBHD_KMAX);
    PSEG_REQUIRE(mh >= 0 && mw >= 0 && mh <= 65535 && mw <= 65535 && (mh == 0) == (mw == 0),
                 "%s: sample %d: dropout mask %dx%d (0x0 = per pixel, otherwise 1..65535 each way)", what, b, mh, mw);
    kmax = K > kmax ? K : kmax;
    if (blend) {
      const int kmed = shape_host[cols * b + 3], K2 = shape_host[cols * b + 4];
      PSEG_REQUIRE(kmed == 0 || (kmed >= 3 && kmed <= PSEG_AUGMENT_BLEND_KMEDMAX && (kmed & 1)),
                   "%s: sample %d: median window %d is not 0 or an odd number from 3 to %d", what, b, kmed, PSEG_AUGMENT_BLEND_KMEDMAX);
      PSEG_REQUIRE(K2 == 0 || (K2 >= 3 && K2 <= PSEG_AUGMENT_BLEND_K2MAX && (K2 & 1)),
                   "%s: sample %d: second filter size %d is not 0 or an odd number from 3 to %d", what, b, K2, PSEG_AUGMENT_BLEND_K2MAX);
      any_halo = any_halo || kmed || K2;
    }
  }
  any_halo = any_halo || kmax > 1;
  const int halo = kmax / 2;
  const int64_t img_tiles_x = cdiv(ow, kNbTileW), img_tiles_y = cdiv(oh, kNbTileH), img_tiles = img_tiles_x * img_tiles_y;
  const int64_t lab_tiles_x = cdiv(W, kAugTileW), lab_tiles = lab_tiles_x * cdiv(H, kAugTileH);
  const int64_t n_img = (int64_t)B * img_tiles, n_lab = (int64_t)B * lab_tiles;
  PSEG_REQUIRE(n_img + n_lab <= 0xffffffLL, "%s: %lld tiles exceed one launch (batch %d of %dx%d -> %dx%d)", what,
               (long long)(n_img + n_lab), B, H, W, oh, ow);
  // LDS: the widest and the tallest working-grid span of an output tile (the kernel's own index function), plus the halo
  int64_t lds_elems = 0;
  if (any_halo) {
    int span_w = 1, span_h = 1;
    for (int64_t t = 0; t < img_tiles_x; ++t) {
      const int o0 = (int)t * kNbTileW, o1 = (o0 + kNbTileW < ow ? o0 + kNbTileW : ow) - 1;
      const int s = aug_ms_index(o1, W, ow) - aug_ms_index(o0, W, ow) + 1;
      span_w = s > span_w ? s : span_w;
    }
    for (int64_t t = 0; t < img_tiles_y; ++t) {
      const int o0 = (int)t * kNbTileH, o1 = (o0 + kNbTileH < oh ? o0 + kNbTileH : oh) - 1;
      const int s = aug_ms_index(o1, H, oh) - aug_ms_index(o0, H, oh) + 1;
      span_h = s > span_h ? s : span_h;
    }
    if (!blend) {
      lds_elems = (int64_t)(span_w + 2 * halo) * (span_h + 2 * halo);
      PSEG_REQUIRE(lds_elems * 4 <= 65536, "%s: a %dx%d output tile of %dx%d -> %dx%d with K = %d needs %lld bytes of LDS (limit 65536)", what,
                   kNbTileW, kNbTileH, H, W, oh, ow, kmax, (long long)(lds_elems * 4));
    } else {
      // two tiles (the kernel's own arithmetic): stage 1 with the whole halo, and with a median stage 2 with the filters'
      for (int b = 0; b < B; ++b) {
        const int K = shape_host[cols * b], kmed = shape_host[cols * b + 3], K2 = shape_host[cols * b + 4];
        const int hm = kmed / 2, hf = (K > K2 ? K : K2) / 2, ht = hm + hf;
        if (ht == 0) continue;
        const int64_t need = (int64_t)(span_w + 2 * ht) * (span_h + 2 * ht) + (hm ? (int64_t)(span_w + 2 * hf) * (span_h + 2 * hf) : 0);
        PSEG_REQUIRE(need * 4 <= 65536, "%s: sample %d: a %dx%d output tile of %dx%d -> %dx%d with kmed = %d, K = %d, K2 = %d needs %lld bytes of LDS (limit 65536)",
                     what, b, kNbTileW, kNbTileH, H, W, oh, ow, kmed, K, K2, (long long)(need * 4));
        lds_elems = need > lds_elems ? need : lds_elems;
      }
    }
  }
  const auto kernel = blend ? augment_batch_nbhd_kernel<true, true> : warp ? augment_batch_nbhd_kernel<true, false> : augment_batch_nbhd_kernel<false, false>;
  hipLaunchKernelGGL(kernel, dim3((uint32_t)(n_img + n_lab)), dim3(256), (size_t)lds_elems * 4, (hipStream_t)stream, img, seg, params, nm,
                     out, target, H, W, oh, ow, (uint32_t)n_img, (uint32_t)img_tiles_x, (uint32_t)img_tiles,
                     (uint32_t)lab_tiles_x, (uint32_t)lab_tiles, halo, (uint32_t)lds_elems);
  PSEG_LAUNCH_CHECK();
  return PSEG_OK;
}

extern "C" {

int pseg_augment_batch(const uint8_t* img, const uint8_t* seg, const float* params, int B, int H, int W, float mean0, float mean1,
                       float mean2, float std0, float std1, float std2, float* out, int oh, int ow, int64_t* target,
                       void* stream) {
  PSEG_REQUIRE(img && seg && params && out && target, "augment_batch: null pointer");
  PSEG_REQUIRE(B >= 1 && B <= 65535, "augment_batch: batch %d outside [1, 65535]", B);
  PSEG_REQUIRE(H >= 1 && H <= 65535 && W >= 1 && W <= 65535, "augment_batch: input size %dx%d outside [1, 65535]", H, W);
  PSEG_REQUIRE(oh >= 1 && oh <= 65535 && ow >= 1 && ow <= 65535, "augment_batch: output size %dx%d outside [1, 65535]", oh, ow);
  PSEG_REQUIRE(std0 != 0.f && std1 != 0.f && std2 != 0.f, "augment_batch: std must be non-zero");
  const int64_t img_tiles_x = cdiv(ow, kAugTileW), img_tiles = img_tiles_x * cdiv(oh, kAugTileH);
  const int64_t lab_tiles_x = cdiv(W, kAugTileW), lab_tiles = lab_tiles_x * cdiv(H, kAugTileH);
  const int64_t n_img = (int64_t)B * img_tiles, n_lab = (int64_t)B * lab_tiles;
  // (HIP bounds a launch by 2^32 threads)
  PSEG_REQUIRE(n_img + n_lab <= 0xffffffLL, "augment_batch: %lld tiles exceed one launch (batch %d of %dx%d -> %dx%d)",
               (long long)(n_img + n_lab), B, H, W, oh, ow);
  AugNorm nm{{mean0, mean1, mean2}, {std0, std1, std2}};
  hipLaunchKernelGGL(augment_batch_kernel, dim3((uint32_t)(n_img + n_lab)), dim3(256), 0, (hipStream_t)stream, img, seg, params, nm,
                     out, target, H, W, oh, ow, (uint32_t)n_img, (uint32_t)img_tiles_x, (uint32_t)img_tiles,
                     (uint32_t)lab_tiles_x, (uint32_t)lab_tiles);
  PSEG_LAUNCH_CHECK();
  return PSEG_OK;
}

int pseg_augment_batch_nbhd(const uint8_t* img, const uint8_t* seg, const float* params, const int* shape_host, int B, int H, int W,
                            float mean0, float mean1, float mean2, float std0, float std1, float std2, float* out, int oh, int ow,
                            int64_t* target, void* stream) {
  return augment_nbhd_launch("augment_batch_nbhd", false, 3, img, seg, params, shape_host, B, H, W, AugNorm{{mean0, mean1, mean2}, {std0, std1, std2}},
                             out, oh, ow, target, stream);
}

int pseg_augment_batch_warp(const uint8_t* img, const uint8_t* seg, const float* params, const int* shape_host, int B, int H, int W,
                            float mean0, float mean1, float mean2, float std0, float std1, float std2, float* out, int oh, int ow,
                            int64_t* target, void* stream) {
  return augment_nbhd_launch("augment_batch_warp", true, 3, img, seg, params, shape_host, B, H, W, AugNorm{{mean0, mean1, mean2}, {std0, std1, std2}},
                             out, oh, ow, target, stream);
}

int pseg_augment_batch_blend(const uint8_t* img, const uint8_t* seg, const float* params, const int* shape_host, int B, int H, int W,
                             float mean0, float mean1, float mean2, float std0, float std1, float std2, float* out, int oh, int ow,
                             int64_t* target, void* stream) {
  return augment_nbhd_launch("augment_batch_blend", true, 5, img, seg, params, shape_host, B, H, W, AugNorm{{mean0, mean1, mean2}, {std0, std1, std2}},
                             out, oh, ow, target, stream);
}

}  // extern "C"
