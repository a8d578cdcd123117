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

// source index coordinate of working-grid pixel (x, y): pixel centres at integers.  Clamped to [-1, size] BEFORE any
// float -> int conversion: a coordinate beyond that range behaves exactly like the bound itself (every tap outside the
// image in constant mode, the edge pixel in edge mode).  A NaN / infinite coordinate is reported and counts as outside.
__device__ __forceinline__ AugCoord aug_coord(const float* __restrict__ row, int x, int y, int H, int W) {
  const float fx = (float)x, fy = (float)y;
  const float sx = fmaf(row[0], fx, fmaf(row[1], fy, row[2]));
  const float sy = fmaf(row[3], fx, fmaf(row[4], fy, row[5]));
  AugCoord c;
  c.finite = fabsf(sx) <= 3.0e38f && fabsf(sy) <= 3.0e38f;   // false for NaN and +-inf
  c.sx = c.finite ? fminf(fmaxf(sx, -1.f), (float)W) : -1.f;
  c.sy = c.finite ? fminf(fmaxf(sy, -1.f), (float)H) : -1.f;
  return c;
}

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

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
    const AugCoord c = aug_coord(row, ox, oy, H, W);
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
  const AugCoord c = aug_coord(row, ix, iy, H, W);
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

}  // namespace pseg

using namespace pseg;

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

}  // extern "C"
