// Batched inference on gfx950: the two passes around model() that the reference runs on the host per photo
// (reference utils/inference.py:10-22: cv2.resize + /255 before the model, softmax + cv2.resize + argmax after it).
//  - image_preprocess: a ragged batch of uint8 HWC photos -> the fp32 NCHW model input [B,3,oh,ow].  INTER_LINEAR
//    geometry (= F.interpolate bilinear, align_corners=False, no antialias) in fp32, rounded to 8 bits half up as the
//    uint8 cv2.resize / PIL resize result, then (v - mean[c]) / std[c] with a correctly rounded fp32 division -- the
//    operation order of CocoDataset.post_fetch_fn, so a photo already at (oh, ow) gives the loader's input bit for bit.
//  - seg_decode: logits [B,C,h,w] -> argmax_c bilinear_resize(softmax_c(logits)) at each photo's own size, uint8 (first
//    index wins ties), optionally through a 256-entry RGB table.  A block owns a low-resolution tile (+1 halo row and
//    column): the logits are read once into LDS and turned into probabilities there, and every full-resolution pixel whose
//    upper-left tap lies in the tile is written by that block alone.  No full-resolution C-channel value is ever stored.
//    A thread walks one output column down its rows and keeps the column-lerped probabilities of the two source rows it
//    sits between in registers (C <= 32): the LDS is read 2C floats per SOURCE row it enters, not 4C per output pixel.
#include "common.h"

#include <math.h>

namespace pseg {

// ------------------------------------------------------------------ geometry (ATen area_pixel_compute_source_index, fp32)
struct InAxis {
  float scale;  // in / out
  int in, out;
};

__device__ __forceinline__ int tap0(const InAxis& a, int o) {
  float s = a.scale * ((float)o + 0.5f) - 0.5f;
  if (s < 0.f) s = 0.f;
  int i0 = (int)s;
  return i0 < a.in - 1 ? i0 : a.in - 1;
}

__device__ __forceinline__ void taps(const InAxis& a, int o, int& i0, int& i1, float& l0, float& l1) {
  float s = a.scale * ((float)o + 0.5f) - 0.5f;
  if (s < 0.f) s = 0.f;
  i0 = (int)s;
  if (i0 > a.in - 1) i0 = a.in - 1;
  i1 = i0 + ((i0 < a.in - 1) ? 1 : 0);
  l1 = s - (float)i0;
  l0 = 1.f - l1;
}

// first output index o in [0, out] whose lower tap is >= i (the lower tap is non-decreasing in o)
__device__ int first_out(const InAxis& a, int i) {
  if (i <= 0) return 0;
  if (i >= a.in) return a.out;
  int e = (int)(((float)i + 0.5f) / a.scale - 0.5f);
  e = e < 0 ? 0 : (e > a.out ? a.out : e);
  while (e > 0 && tap0(a, e - 1) >= i) --e;
  while (e < a.out && tap0(a, e) < i) ++e;
  return e;
}

__device__ __forceinline__ bool entry_ok(int64_t off, int64_t H, int64_t W, int64_t elems_per_px, int64_t cap) {
  return off >= 0 && H >= 1 && W >= 1 && H <= 65535 && W <= 65535 && off + H * W * elems_per_px <= cap;
}

// ------------------------------------------------------------------ preprocess
struct Norm {
  float mean[3], std[3];
};

__global__ __launch_bounds__(256) void image_preprocess_kernel(const uint8_t* __restrict__ src, int64_t src_bytes,
                                                               const int64_t* __restrict__ table, int bgr, Norm nm,
                                                               float* __restrict__ out, int oh, int ow) {
  const int b = blockIdx.z, oy = blockIdx.y;
  const int ox = blockIdx.x * 256 + threadIdx.x;
  if (ox >= ow) return;
  const int64_t off = table[3 * b], H = table[3 * b + 1], W = table[3 * b + 2];
  if (!entry_ok(off, H, W, 3, src_bytes)) return;        // the host wrapper validates the table; never read outside src
  const InAxis ay{(float)H / (float)oh, (int)H, oh}, ax{(float)W / (float)ow, (int)W, ow};
  int y0, y1, x0, x1;
  float ly0, ly1, lx0, lx1;
  taps(ay, oy, y0, y1, ly0, ly1);
  taps(ax, ox, x0, x1, lx0, lx1);
  const uint8_t* p = src + off;
  const uint8_t* p00 = p + ((int64_t)y0 * W + x0) * 3;
  const uint8_t* p01 = p + ((int64_t)y0 * W + x1) * 3;
  const uint8_t* p10 = p + ((int64_t)y1 * W + x0) * 3;
  const uint8_t* p11 = p + ((int64_t)y1 * W + x1) * 3;
  const int64_t plane = (int64_t)oh * ow;
  float* o = out + (int64_t)b * 3 * plane + (int64_t)oy * ow + ox;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int cs = bgr ? 2 - k : k;                      // the swap happens on load
    const float v = ly0 * (lx0 * (float)p00[cs] + lx1 * (float)p01[cs]) + ly1 * (lx0 * (float)p10[cs] + lx1 * (float)p11[cs]);
    float q = floorf(v + 0.5f);                          // 8-bit result, half up, saturated
    q = q < 0.f ? 0.f : (q > 255.f ? 255.f : q);
    o[k * plane] = (q - nm.mean[k]) / nm.std[k];
  }
}

// ------------------------------------------------------------------ decode
constexpr int kDecodeLdsFloats = 12288;   // 48 KiB of probabilities per block

template <int CR>
__global__ __launch_bounds__(256) void seg_decode_kernel(const float* __restrict__ logits, int C, int CP, int h, int w, int TH,
                                                         int TW, int tiles_x, const int64_t* __restrict__ table,
                                                         int64_t npix_cap, uint8_t* __restrict__ mask,
                                                         uint8_t* __restrict__ rgb, const uint8_t* __restrict__ lut) {
  // [tph * tpw][CP] probabilities of the tile and its halo, pixel-major, classes padded to CP (% 4 == 0) with zeros:
  // a chunk of classes of one pixel is a run of ds_read_b128 at immediate offsets
  extern __shared__ f32x4 P4[];
  float* P = reinterpret_cast<float*>(P4);
  const int b = blockIdx.y;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int ys = ty * TH, ye = min(ys + TH, h), xs = tx * TW, xe = min(xs + TW, w);
  const int64_t off = table[3 * b], H = table[3 * b + 1], W = table[3 * b + 2];
  if (!entry_ok(off, H, W, 1, npix_cap)) return;
  const InAxis ay{(float)h / (float)H, h, (int)H}, ax{(float)w / (float)W, w, (int)W};
  const int oy0 = first_out(ay, ys), oy1 = first_out(ay, ye);
  const int ox0 = first_out(ax, xs), ox1 = first_out(ax, xe);
  if (oy0 >= oy1 || ox0 >= ox1) return;   // the tile owns no output pixel (down-scaling): block-uniform exit

  const int tph = min(ye + 1, h) - ys, tpw = min(xe + 1, w) - xs, np = tph * tpw;
  const int tid = threadIdx.x;
  {
    const FastDiv dnp((uint32_t)np), dw((uint32_t)tpw);
    const float* lb = logits + (int64_t)b * C * h * w;
    // consecutive threads: consecutive x of one class row; kLoadBatch loads in flight per thread before their LDS stores
    constexpr int kLoadBatch = 16;
    const int n = C * np;
    for (int i0 = tid; i0 < n; i0 += 256 * kLoadBatch) {
      float v[kLoadBatch];
      int at[kLoadBatch];
#pragma unroll
      for (int u = 0; u < kLoadBatch; ++u) {
        const int i = i0 + u * 256;
        at[u] = -1;
        if (i < n) {
          const int c = (int)dnp.div((uint32_t)i), r = i - c * np;
          const int yy = (int)dw.div((uint32_t)r), xx = r - yy * tpw;
          v[u] = lb[((int64_t)c * h + ys + yy) * w + xs + xx];
          at[u] = r * CP + c;
        }
      }
#pragma unroll
      for (int u = 0; u < kLoadBatch; ++u)
        if (at[u] >= 0) P[at[u]] = v[u];
    }
  }
  __syncthreads();
  const int n4 = CP / 4;
  for (int p = tid; p < np; p += 256) {    // softmax over the classes, once per source pixel of the tile
    f32x4* q = P4 + p * n4;
    float m = -INFINITY;
    for (int j = 0; j < n4; ++j) {
      const f32x4 v = q[j];
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (4 * j + e < C) m = fmaxf(m, v[e]);
    }
    float s = 0.f;
    for (int j = 0; j < n4; ++j) {
      f32x4 v = q[j];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[e] = 4 * j + e < C ? expf(v[e] - m) : 0.f;
        s += v[e];
      }
      q[j] = v;
    }
    const float inv = 1.f / s;
    for (int j = 0; j < n4; ++j) q[j] *= inv;
  }
  __syncthreads();

  const int ncols = ox1 - ox0, nrows = oy1 - oy0;
  const int groups = ncols >= 256 ? 1 : 256 / ncols;
  const int rows_per = (nrows + groups - 1) / groups;
  uint8_t* mb = mask + off;
  uint8_t* rb = rgb ? rgb + 3 * off : nullptr;
  for (int j = tid; j < ncols * groups; j += 256) {
    const int g = j / ncols, col = j - g * ncols;
    const int ox = ox0 + col;
    int x0, x1;
    float lx0, lx1;
    taps(ax, ox, x0, x1, lx0, lx1);
    x0 -= xs;
    x1 -= xs;
    const int r0 = oy0 + g * rows_per, r1 = min(r0 + rows_per, oy1);
    f32x4 Qa[CR / 4], Qb[CR / 4];          // column-lerped probabilities of source rows ca and cb (kept while C <= CR)
    int ca = -1, cb = -1;
    for (int oy = r0; oy < r1; ++oy) {
      int y0, y1;
      float ly0, ly1;
      taps(ay, oy, y0, y1, ly0, ly1);
      y0 -= ys;
      y1 -= ys;
      float best = -1.f;
      int bi = 0;
      for (int c0 = 0; c0 < C; c0 += CR) {
        if (C > CR || y0 != ca || y1 != cb) {
          const bool shift = C <= CR && y0 == cb;
          const f32x4* a0 = P4 + ((y0 * tpw + x0) * CP + c0) / 4;
          const f32x4* a1 = P4 + ((y0 * tpw + x1) * CP + c0) / 4;
          const f32x4* b0 = P4 + ((y1 * tpw + x0) * CP + c0) / 4;
          const f32x4* b1 = P4 + ((y1 * tpw + x1) * CP + c0) / 4;
#pragma unroll
          for (int k = 0; k < CR / 4; ++k) {
            if (c0 + 4 * k < C) {
              Qa[k] = shift ? Qb[k] : lx0 * a0[k] + lx1 * a1[k];
              Qb[k] = lx0 * b0[k] + lx1 * b1[k];
            }
          }
          ca = y0;
          cb = y1;
        }
#pragma unroll
        for (int k = 0; k < CR / 4; ++k) {
          if (c0 + 4 * k < C) {
            const f32x4 v = ly0 * Qa[k] + ly1 * Qb[k];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              if (c0 + 4 * k + e < C && v[e] > best) {   // strict: the first index wins ties
                best = v[e];
                bi = c0 + 4 * k + e;
              }
            }
          }
        }
      }
      const int64_t o = (int64_t)oy * W + ox;
      mb[o] = (uint8_t)bi;
      if (rb) {
        rb[3 * o] = lut[3 * bi];
        rb[3 * o + 1] = lut[3 * bi + 1];
        rb[3 * o + 2] = lut[3 * bi + 2];
      }
    }
  }
}

}  // namespace pseg

using namespace pseg;

extern "C" {

int pseg_image_preprocess(const uint8_t* src, int64_t src_bytes, const int64_t* table, int B, int bgr, float mean0, float mean1,
                          float mean2, float std0, float std1, float std2, float* out, int oh, int ow, void* stream) {
  PSEG_REQUIRE(src && table && out, "image_preprocess: null pointer");
  PSEG_REQUIRE(B >= 1 && B <= 65535, "image_preprocess: batch %d outside [1, 65535]", B);
  PSEG_REQUIRE(oh >= 1 && oh <= 65535 && ow >= 1 && ow <= 65535, "image_preprocess: output size %dx%d outside [1, 65535]", oh, ow);
  PSEG_REQUIRE(src_bytes >= 3, "image_preprocess: src_bytes %lld holds no pixel", (long long)src_bytes);
  PSEG_REQUIRE(std0 != 0.f && std1 != 0.f && std2 != 0.f, "image_preprocess: std must be non-zero");
  Norm nm{{mean0, mean1, mean2}, {std0, std1, std2}};
  hipLaunchKernelGGL(image_preprocess_kernel, dim3(cdiv(ow, 256), oh, B), dim3(256), 0, (hipStream_t)stream, src, src_bytes,
                     table, bgr ? 1 : 0, nm, out, oh, ow);
  PSEG_LAUNCH_CHECK();
  return PSEG_OK;
}

int pseg_seg_decode(const float* logits, int B, int C, int h, int w, const int64_t* table, int64_t npix_total, uint8_t* mask,
                    uint8_t* rgb, const uint8_t* lut, void* stream) {
  PSEG_REQUIRE(logits && table && mask, "seg_decode: null pointer");
  PSEG_REQUIRE((rgb == nullptr) == (lut == nullptr), "seg_decode: rgb and lut come together");
  PSEG_REQUIRE(C >= 1 && C <= 256, "seg_decode: %d classes; 1 <= C <= 256 supported (the mask is uint8)", C);
  PSEG_REQUIRE(B >= 1 && B <= 65535, "seg_decode: batch %d outside [1, 65535]", B);
  PSEG_REQUIRE(h >= 1 && w >= 1 && h <= 65535 && w <= 65535, "seg_decode: logit size %dx%d outside [1, 65535]", h, w);
  PSEG_REQUIRE(npix_total >= 1, "seg_decode: npix_total %lld", (long long)npix_total);
  // tile: TW x TH source pixels (+1 halo row / column) whose CP probabilities fit kDecodeLdsFloats; as wide as possible
  const int CP = C <= 8 ? 8 : (C + 3) / 4 * 4;
  const int per_px = kDecodeLdsFloats / CP;
  int TW = 32;
  while (TW > 1 && per_px / (TW + 1) < TW / 2 + 1) TW /= 2;
  int TH = per_px / (TW + 1) - 1;
  TH = TH > 32 ? 32 : (TH < 1 ? 1 : TH);
  const int tiles_x = cdiv(w, TW), tiles_y = cdiv(h, TH);
  const size_t lds = (size_t)CP * (TH + 1) * (TW + 1) * sizeof(float);
  const hipStream_t st = (hipStream_t)stream;
  if (C <= 8)
    hipLaunchKernelGGL(seg_decode_kernel<8>, dim3(tiles_x * tiles_y, B), dim3(256), lds, st, logits, C, CP, h, w, TH, TW,
                       tiles_x, table, npix_total, mask, rgb, lut);
  else
    hipLaunchKernelGGL(seg_decode_kernel<32>, dim3(tiles_x * tiles_y, B), dim3(256), lds, st, logits, C, CP, h, w, TH, TW,
                       tiles_x, table, npix_total, mask, rgb, lut);
  PSEG_LAUNCH_CHECK();
  return PSEG_OK;
}

}  // extern "C"
