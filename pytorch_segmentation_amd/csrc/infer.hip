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
// The three preprocess entry points are one kernel template over the table's row layout (3, 4 or 8 words) around one
// sample-and-store body; a narrower row is the wider one with constants, so the plain route compiles without the others' work.
// Test-time ensembling (several scales, each optionally with its left-right mirrored twin) stands on:
//  - image_preprocess_views: image_preprocess with a flag word per table row; bit 0 mirrors the OUTPUT row, so one launch
//    gives the plain and the mirrored model input of every photo at one scale.
//  - softmax_views: logits [n,C,h,w] -> probabilities [B,h,w,CP], pixel-major, classes padded to CP with zeros; with
//    pairs the mirrored twin (batch row B + b) is un-mirrored and added, so a flip pair costs no storage of its own.
//  - seg_decode_ensemble: argmax_c of the SUM over the S maps of bilinear(map_s, (H, W)).  Ownership is by OUTPUT tile
//    (maps of different resolutions share no source tiling); a thread owns a short column of output pixels and reads the
//    four taps of each map as 16-byte vectors straight from L1/L2 -- neighbouring pixels share them -- instead of
//    staging S footprints of S different shapes in LDS (an 8x down-scaled photo's footprint would not fit anyway).
// Sliding-window inference (a photo larger than the model input is covered by overlapping windows of the input size at
// the photo's own or a scaled resolution) generalises two of them:
//  - image_preprocess_windows: image_preprocess_views whose output row is a window of the photo resampled to a working
//    size (Hs, Ws), zero (the mean colour) beyond it.
//  - seg_decode_windows: seg_decode_ensemble with, per scale, the windows' probability maps in place of one map: the value
//    of a bilinear tap is the unweighted mean of the windows that cover it.  Still a gather by output tile -- no atomics and
//    no C-channel canvas at working or photo size; the windows covering a tap depend only on its row or column, so a block
//    works them out once for its 16 rows and 64 columns into LDS.
// The two kernels that own output tiles share their table-row check and ragged-batch exit (out_tile), their class scan
// (scan_classes) and, with seg_decode, the pixel store (store_pixel); the inner loops stay each kernel's own.  The entry
// points' argument checks are written once per family and take the entry point's name for their messages.
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

// One table row in the terms of the widest layout.  kWords = 3: {byte offset, H, W}; 4: {.., flags}; 8: {.., flags, Hs, Ws,
// y0, x0}.  What a narrower row does not carry is a constant: flags 0, the working image is the output, origin (0, 0).
struct PreRow {
  int64_t off, H, W, flags, Hs, Ws, wy, wx;
};

template <int kWords>
__device__ __forceinline__ PreRow read_row(const int64_t* __restrict__ table, int b, int oh, int ow) {
  const int64_t* t = table + kWords * (int64_t)b;
  PreRow r{t[0], t[1], t[2], 0, oh, ow, 0, 0};
  if constexpr (kWords >= 4) r.flags = t[3];
  if constexpr (kWords == 8) {
    r.Hs = t[4];
    r.Ws = t[5];
    r.wy = t[6];
    r.wx = t[7];
  }
  return r;
}

// The four taps of position (Y, X) of the resampled photo p, blended, rounded to 8 bits, normalised -> o[k * plane]
__device__ __forceinline__ void sample_store(const uint8_t* __restrict__ p, int64_t W, const InAxis& ay, const InAxis& ax, int Y,
                                             int X, int bgr, const Norm& nm, float* __restrict__ o, int64_t plane) {
  int y0, y1, x0, x1;
  float ly0, ly1, lx0, lx1;
  taps(ay, Y, y0, y1, ly0, ly1);
  taps(ax, X, x0, x1, lx0, lx1);
  const uint8_t* p00 = p + ((int64_t)y0 * W + x0) * 3;
  const uint8_t* p01 = p + ((int64_t)y0 * W + x1) * 3;
  const uint8_t* p10 = p + ((int64_t)y1 * W + x0) * 3;
  const uint8_t* p11 = p + ((int64_t)y1 * W + x1) * 3;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int cs = bgr ? 2 - k : k;                      // the swap happens on load
    const float v = ly0 * (lx0 * (float)p00[cs] + lx1 * (float)p01[cs]) + ly1 * (lx0 * (float)p10[cs] + lx1 * (float)p11[cs]);
    float q = floorf(v + 0.5f);                          // 8-bit result, half up, saturated
    q = q < 0.f ? 0.f : (q > 255.f ? 255.f : q);
    o[k * plane] = (q - nm.mean[k]) / nm.std[k];
  }
}

// out[b] = the oh x ow window at the row's origin of its photo resampled to the row's working size; bit 0 of the flags
// mirrors the OUTPUT row (the resampled result, not the photo); positions beyond the working image hold 0.0f (the mean
// colour).  The layout is a template parameter: the 3-word instantiation holds no flag test, no mirror select and no
// beyond-the-image branch, the 4-word one no origin.  A bad row (the host wrapper validates the table) reads and writes
// nothing.  With Hs = oh the scale (float)H / (float)(int)Hs is (float)H / (float)oh: a 4-word row gives the 3-word
// row's bits, an 8-word row {.., oh, ow, 0, 0} the 4-word row's, and a window the bits of the crop of the working image.
template <int kWords>
__global__ __launch_bounds__(256) void image_preprocess_kernel(const uint8_t* __restrict__ src, int64_t src_bytes,
                                                               const int64_t* __restrict__ table, int flag_mask, int bgr,
                                                               Norm nm, float* __restrict__ out, int oh, int ow) {
  const int b = blockIdx.z, oy = blockIdx.y;
  const int ox = blockIdx.x * 256 + threadIdx.x;
  if (ox >= ow) return;
  const PreRow r = read_row<kWords>(table, b, oh, ow);
  if (!entry_ok(r.off, r.H, r.W, 3, src_bytes)) return;
  if constexpr (kWords >= 4)
    if ((r.flags & ~(int64_t)flag_mask) != 0) return;
  if constexpr (kWords == 8)
    if (r.Hs < 1 || r.Ws < 1 || r.Hs > 65535 || r.Ws > 65535 || r.wy < 0 || r.wx < 0 || r.wy >= r.Hs || r.wx >= r.Ws) return;
  const InAxis ay{(float)r.H / (float)(int)r.Hs, (int)r.H, (int)r.Hs}, ax{(float)r.W / (float)(int)r.Ws, (int)r.W, (int)r.Ws};
  int sx = ox;                                                       // the column of the unmirrored result
  if constexpr (kWords >= 4) sx = (r.flags & PSEG_VIEW_MIRROR) ? ow - 1 - ox : ox;
  const int Y = (int)r.wy + oy, X = (int)r.wx + sx;                  // position in the working image
  const int64_t plane = (int64_t)oh * ow;
  float* o = out + (int64_t)b * 3 * plane + (int64_t)oy * ow + ox;
  if constexpr (kWords == 8) {
    if (Y >= (int)r.Hs || X >= (int)r.Ws) {
#pragma unroll
      for (int k = 0; k < 3; ++k) o[k * plane] = 0.f;
      return;
    }
  }
  sample_store(src + r.off, r.W, ay, ax, Y, X, bgr, nm, o, plane);
}

// ------------------------------------------------------------------ decode
constexpr int kDecodeLdsFloats = 12288;   // 48 KiB of probabilities per block

// The running argmax over classes c .. c + 3 of v; classes >= C are padding
__device__ __forceinline__ void scan_classes(const f32x4& v, int c, int C, float& best, int& bi) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (c + e < C && v[e] > best) {   // strict: the first index wins ties
      best = v[e];
      bi = c + e;
    }
  }
}

// Pixel o of an image whose mask starts at mb and whose colours start at rb (null: mask only)
__device__ __forceinline__ void store_pixel(uint8_t* mb, uint8_t* rb, const uint8_t* lut, int64_t o, int bi) {
  mb[o] = (uint8_t)bi;
  if (rb) {
    rb[3 * o] = lut[3 * bi];
    rb[3 * o + 1] = lut[3 * bi + 1];
    rb[3 * o + 2] = lut[3 * bi + 2];
  }
}

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
            // scan_classes, spelt out: through the helper (in any form tried: by reference, by value, loop-free) hipcc
            // allocates 10 more VGPRs for this kernel and both instantiations lose a wave per SIMD
            const f32x4 v = ly0 * Qa[k] + ly1 * Qb[k];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              if (c0 + 4 * k + e < C && v[e] > best) {
                best = v[e];
                bi = c0 + 4 * k + e;
              }
            }
          }
        }
      }
      store_pixel(mb, rb, lut, (int64_t)oy * W + ox, bi);
    }
  }
}

// ------------------------------------------------------------------ test-time ensembling
// A block owns PX consecutive pixels of one source row (PX a power of two, 4 * PX <= 256).  The logits of the run -- and,
// with pairs, of the mirrored run of batch row B + b, stored un-mirrored -- go to LDS pixel-major (global reads: consecutive
// lanes, consecutive x of one class plane); four lanes share a pixel's softmax; the tile is then exactly the run's
// [PX][CP] stretch of the output and leaves as 16-byte vectors.
__global__ __launch_bounds__(256) void softmax_views_kernel(const float* __restrict__ logits, int B, int pairs, int C, int CP,
                                                            int h, int w, int PX, int px_shift, int runs, float* __restrict__ out) {
  extern __shared__ f32x4 T4[];
  float* T = reinterpret_cast<float*>(T4);
  const int tid = threadIdx.x;
  const int run = blockIdx.x % runs, row = blockIdx.x / runs;      // row = b * h + y
  const int b = row / h, y = row - b * h;
  const int x0 = run * PX, npx = min(PX, w - x0);
  const int64_t plane = (int64_t)h * w;
  const int views = pairs ? 2 : 1;
  for (int v = 0; v < views; ++v) {
    const float* lb = logits + ((int64_t)(v * B + b) * C) * plane + (int64_t)y * w;
    float* Tv = T + v * PX * CP;
    for (int i = tid; i < C * PX; i += 256) {
      const int c = i >> px_shift, px = i & (PX - 1);
      if (px < npx) {
        const int x = x0 + px;
        Tv[px * CP + c] = lb[c * plane + (v ? w - 1 - x : x)];
      }
    }
  }
  __syncthreads();
  const int n4 = CP / 4;
  const int px = tid >> 2, q = tid & 3;
  if (px < npx) {                                                    // whole quads take the branch together
    for (int v = 0; v < views; ++v) {
      f32x4* t = T4 + (v * PX + px) * n4;
      float m = -INFINITY;
      for (int j = q; j < n4; j += 4) {
        const f32x4 u = t[j];
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (4 * j + e < C) m = fmaxf(m, u[e]);
      }
      m = fmaxf(m, __shfl_xor(m, 1, 64));
      m = fmaxf(m, __shfl_xor(m, 2, 64));
      // sixteen partial sums per pixel (four lanes x four vector lanes), combined as a tree: at C = 256 a partial adds 16
      // terms, not 256 -- the rounding of one long running sum alone would use up the 4 ulp the map is held to
      f32x4 s4 = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int j = q; j < n4; j += 4) {
        f32x4 u = t[j];
#pragma unroll
        for (int e = 0; e < 4; ++e) u[e] = 4 * j + e < C ? expf(u[e] - m) : 0.f;
        s4 += u;
        t[j] = u;
      }
      float s = (s4[0] + s4[1]) + (s4[2] + s4[3]);
      s += __shfl_xor(s, 1, 64);
      s += __shfl_xor(s, 2, 64);
      for (int j = q; j < n4; j += 4) t[j] = t[j] / s;     // correctly rounded division: half an ulp less than * (1 / s)
    }
  }
  __syncthreads();
  f32x4* o = reinterpret_cast<f32x4*>(out) + ((int64_t)row * w + x0) * n4;
  for (int i = tid; i < npx * n4; i += 256) o[i] = pairs ? T4[i] + T4[PX * n4 + i] : T4[i];
}

constexpr int kEnsTileW = 64, kEnsTileH = 16, kEnsMaxMaps = 8;

__device__ __forceinline__ bool map_ok(int64_t off, int64_t h, int64_t w, int B, int CP, int64_t cap) {
  return off >= 0 && (off & 3) == 0 && h >= 1 && w >= 1 && h <= 65535 && w <= 65535 && off + (int64_t)B * h * w * CP <= cap;
}

// What the two kernels that own OUTPUT tiles do before their loops: image blockIdx.z's table row and the block's tile of it.
struct OutTile {
  int64_t off, H, W;
  int oy_base, ox_base, oy_end;
};

// -> false, for the whole block, when the row is bad or above the stated maximum (nothing is read or written) or the tile
// lies outside the image (ragged batch)
__device__ __forceinline__ bool out_tile(const int64_t* __restrict__ table, int64_t npix_cap, int Hmax, int Wmax, OutTile& tile) {
  const int b = blockIdx.z;
  tile.off = table[3 * b], tile.H = table[3 * b + 1], tile.W = table[3 * b + 2];
  if (!entry_ok(tile.off, tile.H, tile.W, 1, npix_cap) || tile.H > Hmax || tile.W > Wmax) return false;
  tile.oy_base = blockIdx.y * kEnsTileH, tile.ox_base = blockIdx.x * kEnsTileW;
  if (tile.oy_base >= tile.H || tile.ox_base >= tile.W) return false;
  tile.oy_end = min(tile.oy_base + kEnsTileH, (int)tile.H);
  return true;
}

// A block owns a kEnsTileW x kEnsTileH rectangle of one image's pixels; a wave owns one row of it at a time (64 mask
// bytes per store), a thread the pixels of its column in rows wave, wave + 4, ...  Per chunk of at most 32 classes the
// bilinear samples of the S maps are summed in registers, then the running best is updated: classes are independent.
__global__ __launch_bounds__(256) void seg_decode_ensemble_kernel(const float* __restrict__ prob, int64_t prob_floats,
                                                                  const int64_t* __restrict__ maps, int S, int B, int C, int CP,
                                                                  const int64_t* __restrict__ table, int64_t npix_cap,
                                                                  int Hmax, int Wmax, uint8_t* __restrict__ mask,
                                                                  uint8_t* __restrict__ rgb, const uint8_t* __restrict__ lut) {
  OutTile tile;
  if (!out_tile(table, npix_cap, Hmax, Wmax, tile)) return;
  const int b = blockIdx.z, ox = tile.ox_base + (threadIdx.x & 63);
  for (int s = 0; s < S; ++s)                                                  // one bad map: no ensemble, nothing written
    if (!map_ok(maps[3 * s], maps[3 * s + 1], maps[3 * s + 2], B, CP, prob_floats)) return;
  if (ox >= tile.W) return;
  const int n4 = CP / 4;
  uint8_t* mb = mask + tile.off;
  uint8_t* rb = rgb ? rgb + 3 * tile.off : nullptr;
  for (int oy = tile.oy_base + (threadIdx.x >> 6); oy < tile.oy_end; oy += 4) {
    float best = -1.f;
    int bi = 0;
    for (int c0 = 0; c0 < CP; c0 += 32) {
      f32x4 acc[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int s = 0; s < S; ++s) {
        const int64_t moff = maps[3 * s];
        const int h = (int)maps[3 * s + 1], w = (int)maps[3 * s + 2];
        const InAxis ay{(float)h / (float)tile.H, h, (int)tile.H}, ax{(float)w / (float)tile.W, w, (int)tile.W};
        int y0, y1, x0, x1;
        float ly0, ly1, lx0, lx1;
        taps(ay, oy, y0, y1, ly0, ly1);
        taps(ax, ox, x0, x1, lx0, lx1);
        const f32x4* mp = reinterpret_cast<const f32x4*>(prob + moff) + (int64_t)b * h * w * n4 + c0 / 4;
        const f32x4* a0 = mp + ((int64_t)y0 * w + x0) * n4;
        const f32x4* a1 = mp + ((int64_t)y0 * w + x1) * n4;
        const f32x4* b0 = mp + ((int64_t)y1 * w + x0) * n4;
        const f32x4* b1 = mp + ((int64_t)y1 * w + x1) * n4;
#pragma unroll
        for (int k = 0; k < 8; ++k)
          if (c0 + 4 * k < CP) acc[k] += ly0 * (lx0 * a0[k] + lx1 * a1[k]) + ly1 * (lx0 * b0[k] + lx1 * b1[k]);
      }
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (c0 + 4 * k < CP) scan_classes(acc[k], c0 + 4 * k, C, best, bi);
    }
    store_pixel(mb, rb, lut, (int64_t)oy * tile.W + ox, bi);
  }
}

// ------------------------------------------------------------------ sliding windows
// Along one axis a working image of `in` pixels is covered by n = ceil(max(in - win, 0) / stride) + 1 windows of `win`
// pixels; window i starts at min(i * stride, max(in - win, 0)): the last one is shifted back inside the image, and an
// image shorter than the window has one window (whose positions beyond the image are never sampled).
__device__ __forceinline__ int win_count(int in, int win, const FastDiv& st) {
  const int m = in > win ? in - win : 0;
  return (int)st.div((uint32_t)m + st.d - 1) + 1;
}

// The windows covering coordinate p (0 <= p < in), ascending, as (window index << 16 | coordinate inside the window);
// -> their number: 1..3 under the stride limits ceil(win / 2) <= stride <= win the host enforces.
__device__ __forceinline__ int win_cover(int p, int in, int win, const FastDiv& st, int n, uint32_t* out) {
  const int m = in > win ? in - win : 0;
  const int hi = p >= m ? n - 1 : (int)st.div((uint32_t)p);
  const int lo = p < win ? 0 : (int)st.div((uint32_t)(p - win)) + 1;
  const int c = min(hi - lo + 1, 3);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int i = lo + k;
    out[k] = k < c ? ((uint32_t)i << 16) | (uint32_t)(p - min(i * (int)st.d, m)) : 0u;
  }
  return c;
}

// One bilinear tap pair of an output row or column at one scale: the upper tap's weight and, for the lower and the upper
// tap, the windows that cover its working-image coordinate (win_cover); cnt = lower count | upper count << 2.
struct WinTaps {
  float l1;
  int cnt;
  uint32_t win[6];
};

// seg_decode_ensemble_kernel's tile and thread mapping, with the map of scale s replaced by the group of windows of
// photo b at that scale: the value of a tap is the sum of the covering windows' vectors over their number.  A gather: no
// atomics, no canvas.  What depends only on the tap's coordinate -- the taps of the tile's 16 rows and 64 columns at every
// scale and the windows covering them -- is worked out once per block into LDS (20 KiB), not per pixel and class chunk;
// the row entries are read wave-uniformly, the column entries by consecutive lanes.
__global__ __launch_bounds__(256) void seg_decode_windows_kernel(const float* __restrict__ prob, int64_t prob_floats,
                                                                 const int64_t* __restrict__ groups, int S, int B, int C, int CP,
                                                                 int h, int w, FastDiv dsy, FastDiv dsx,
                                                                 const int64_t* __restrict__ table, int64_t npix_cap, int Hmax,
                                                                 int Wmax, uint8_t* __restrict__ mask, uint8_t* __restrict__ rgb,
                                                                 const uint8_t* __restrict__ lut) {
  constexpr int kEnt = kEnsTileH + kEnsTileW;
  __shared__ WinTaps ent[kEnsMaxMaps * kEnt];
  __shared__ int64_t goff[kEnsMaxMaps];
  __shared__ int gnx[kEnsMaxMaps];
  OutTile tile;
  if (!out_tile(table, npix_cap, Hmax, Wmax, tile)) return;
  const int b = blockIdx.z, oy_base = tile.oy_base, ox_base = tile.ox_base;
  for (int s = 0; s < S; ++s) {                                                // one bad group: this photo is not written
    const int64_t* g = groups + 3 * ((int64_t)s * B + b);
    const int64_t go = g[0], Hs = g[1], Ws = g[2];
    if (go < 0 || (go & 3) != 0 || Hs < 1 || Ws < 1 || Hs > 65535 || Ws > 65535) return;
    const int64_t cells = (int64_t)win_count((int)Hs, h, dsy) * h * ((int64_t)win_count((int)Ws, w, dsx) * w);
    if (go + cells * CP > prob_floats) return;
  }
  const int tid = threadIdx.x;
  for (int e = tid; e < S * kEnt; e += 256) {
    const int s = e / kEnt, r = e - s * kEnt;
    const int64_t* g = groups + 3 * ((int64_t)s * B + b);
    const bool is_row = r < kEnsTileH;
    const int o = is_row ? oy_base + r : ox_base + r - kEnsTileH;
    const int in = (int)(is_row ? g[1] : g[2]), outn = (int)(is_row ? tile.H : tile.W), win = is_row ? h : w;
    const FastDiv st = is_row ? dsy : dsx;
    WinTaps wt{0.f, 0, {0, 0, 0, 0, 0, 0}};
    if (o < outn) {
      const InAxis a{(float)in / (float)outn, in, outn};
      int i0, i1;
      float l0, l1;
      taps(a, o, i0, i1, l0, l1);
      const int n = win_count(in, win, st);
      wt.l1 = l1;
      wt.cnt = win_cover(i0, in, win, st, n, wt.win) | win_cover(i1, in, win, st, n, wt.win + 3) << 2;
    }
    ent[e] = wt;
    if (r == 0) {
      goff[s] = g[0];
      gnx[s] = win_count((int)g[2], w, dsx);
    }
  }
  __syncthreads();
  const int col = tid & 63, ox = ox_base + col;
  if (ox >= tile.W) return;
  const int n4 = CP / 4;
  uint8_t* mb = mask + tile.off;
  uint8_t* rb = rgb ? rgb + 3 * tile.off : nullptr;
  for (int oy = oy_base + (tid >> 6); oy < tile.oy_end; oy += 4) {
    float best = -1.f;
    int bi = 0;
    for (int c0 = 0; c0 < CP; c0 += 32) {
      f32x4 acc[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int s = 0; s < S; ++s) {
        const WinTaps* ey = ent + s * kEnt + (oy - oy_base);
        const WinTaps* ex = ent + s * kEnt + kEnsTileH + col;
        const f32x4* gp = reinterpret_cast<const f32x4*>(prob + goff[s]) + c0 / 4;
        const int64_t nx = gnx[s];
        const float ly1 = ey->l1, ly0 = 1.f - ly1, lx1 = ex->l1, lx0 = 1.f - lx1;
        const int cy = ey->cnt, cx = ex->cnt;
#pragma unroll
        for (int ty = 0; ty < 2; ++ty) {
#pragma unroll
          for (int tx = 0; tx < 2; ++tx) {
            const int ny_ = (cy >> (2 * ty)) & 3, nx_ = (cx >> (2 * tx)) & 3;
            f32x4 t[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) t[k] = f32x4{0.f, 0.f, 0.f, 0.f};
            for (int i = 0; i < ny_; ++i) {                                    // the covering windows, in (i, j) order
              const uint32_t uy = ey->win[3 * ty + i];
              for (int j = 0; j < nx_; ++j) {
                const uint32_t ux = ex->win[3 * tx + j];
                const int64_t px = (((int64_t)(uy >> 16) * nx + (ux >> 16)) * h + (uy & 0xffffu)) * w + (ux & 0xffffu);
                const f32x4* p = gp + px * n4;
#pragma unroll
                for (int k = 0; k < 8; ++k)
                  if (c0 + 4 * k < CP) t[k] += p[k];
              }
            }
            const int n = ny_ * nx_;
            const float cnt = (float)n, wgt = (ty ? ly1 : ly0) * (tx ? lx1 : lx0);
#pragma unroll
            for (int k = 0; k < 8; ++k)
              if (c0 + 4 * k < CP) acc[k] += wgt * (n > 1 ? t[k] / cnt : t[k]);   // correctly rounded; / 1 is the identity
          }
        }
      }
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (c0 + 4 * k < CP) scan_classes(acc[k], c0 + 4 * k, C, best, bi);
    }
    store_pixel(mb, rb, lut, (int64_t)oy * tile.W + ox, bi);
  }
}

// ------------------------------------------------------------------ host checks shared by the entry points (name: theirs)
// kWords = 3: `rows` is the batch and there is no flag word; `what` names the output ("output" / "window")
template <int kWords>
static int launch_preprocess(const char* name, const char* what, const uint8_t* src, int64_t src_bytes, const int64_t* table,
                             int rows, int flag_mask, int bgr, const Norm& nm, float* out, int oh, int ow, void* stream) {
  PSEG_REQUIRE(src && table && out, "%s: null pointer", name);
  if (kWords == 3) {
    PSEG_REQUIRE(rows >= 1 && rows <= 65535, "%s: batch %d outside [1, 65535]", name, rows);
  } else {
    PSEG_REQUIRE((flag_mask & ~PSEG_VIEW_MIRROR) == 0, "%s: unknown flag bits 0x%x (known: PSEG_VIEW_MIRROR = 1)", name,
                 (unsigned)(flag_mask & ~PSEG_VIEW_MIRROR));
    PSEG_REQUIRE(rows >= 1 && rows <= 65535, "%s: %d table rows outside [1, 65535]", name, rows);
  }
  PSEG_REQUIRE(oh >= 1 && oh <= 65535 && ow >= 1 && ow <= 65535, "%s: %s size %dx%d outside [1, 65535]", name, what, oh, ow);
  PSEG_REQUIRE(src_bytes >= 3, "%s: src_bytes %lld holds no pixel", name, (long long)src_bytes);
  PSEG_REQUIRE(nm.std[0] != 0.f && nm.std[1] != 0.f && nm.std[2] != 0.f, "%s: std must be non-zero", name);
  hipLaunchKernelGGL(image_preprocess_kernel<kWords>, dim3(cdiv(ow, 256), oh, rows), dim3(256), 0, (hipStream_t)stream, src,
                     src_bytes, table, flag_mask, bgr ? 1 : 0, nm, out, oh, ow);
  PSEG_LAUNCH_CHECK();
  return PSEG_OK;
}

// The decode entry points' checks after their null-pointer test; S maps or scales (`noun`), none for the plain decode
static int check_decode(const char* name, const uint8_t* rgb, const uint8_t* lut, int S, const char* noun, int C, int B) {
  PSEG_REQUIRE((rgb == nullptr) == (lut == nullptr), "%s: rgb and lut come together", name);
  if (noun) PSEG_REQUIRE(S >= 1 && S <= kEnsMaxMaps, "%s: %d %s; 1 <= S <= %d supported", name, S, noun, kEnsMaxMaps);
  PSEG_REQUIRE(C >= 1 && C <= 256, "%s: %d classes; 1 <= C <= 256 supported (the mask is uint8)", name, C);
  PSEG_REQUIRE(B >= 1 && B <= 65535, "%s: batch %d outside [1, 65535]", name, B);
  return PSEG_OK;
}

// ... and those of the two that read the packed probability buffer and size their grid by the largest image
static int check_packed(const char* name, const float* prob, int64_t prob_floats, int64_t npix_total, int Hmax, int Wmax) {
  PSEG_REQUIRE(Hmax >= 1 && Wmax >= 1 && Hmax <= 65535 && Wmax <= 65535, "%s: largest image %dx%d outside [1, 65535]", name, Hmax,
               Wmax);
  PSEG_REQUIRE(((uintptr_t)prob & 15) == 0, "%s: the probability buffer must be 16-byte aligned", name);
  PSEG_REQUIRE(prob_floats >= 8 && npix_total >= 1, "%s: prob_floats %lld, npix_total %lld", name, (long long)prob_floats,
               (long long)npix_total);
  return PSEG_OK;
}

}  // namespace pseg

using namespace pseg;

extern "C" {

int pseg_image_preprocess(const uint8_t* src, int64_t src_bytes, const int64_t* table, int B, int bgr, float mean0, float mean1,
                          float mean2, float std0, float std1, float std2, float* out, int oh, int ow, void* stream) {
  return launch_preprocess<3>("image_preprocess", "output", src, src_bytes, table, B, 0, bgr,
                              Norm{{mean0, mean1, mean2}, {std0, std1, std2}}, out, oh, ow, stream);
}

int pseg_seg_decode(const float* logits, int B, int C, int h, int w, const int64_t* table, int64_t npix_total, uint8_t* mask,
                    uint8_t* rgb, const uint8_t* lut, void* stream) {
  PSEG_REQUIRE(logits && table && mask, "seg_decode: null pointer");
  if (int e = check_decode("seg_decode", rgb, lut, 0, nullptr, C, B)) return e;
  PSEG_REQUIRE(h >= 1 && w >= 1 && h <= 65535 && w <= 65535, "seg_decode: logit size %dx%d outside [1, 65535]", h, w);
  PSEG_REQUIRE(npix_total >= 1, "seg_decode: npix_total %lld", (long long)npix_total);
  // tile: TW x TH source pixels (+1 halo row / column) whose CP probabilities fit kDecodeLdsFloats; as wide as possible
  const int CP = class_pad(C);
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

int pseg_image_preprocess_views(const uint8_t* src, int64_t src_bytes, const int64_t* table, int rows, int flag_mask, int bgr,
                                float mean0, float mean1, float mean2, float std0, float std1, float std2, float* out, int oh,
                                int ow, void* stream) {
  return launch_preprocess<4>("image_preprocess_views", "output", src, src_bytes, table, rows, flag_mask, bgr,
                              Norm{{mean0, mean1, mean2}, {std0, std1, std2}}, out, oh, ow, stream);
}

int pseg_softmax_views(const float* logits, int B, int pairs, int C, int h, int w, float* prob, int64_t prob_offset,
                       int64_t prob_floats, void* stream) {
  PSEG_REQUIRE(logits && prob, "softmax_views: null pointer");
  PSEG_REQUIRE(pairs == 0 || pairs == 1, "softmax_views: pairs %d has unknown flag bits (0: plain rows, 1: plain + mirrored)", pairs);
  PSEG_REQUIRE(C >= 1 && C <= 256, "softmax_views: %d classes; 1 <= C <= 256 supported", C);
  PSEG_REQUIRE(B >= 1 && B <= 65535, "softmax_views: batch %d outside [1, 65535]", B);
  PSEG_REQUIRE(h >= 1 && w >= 1 && h <= 65535 && w <= 65535, "softmax_views: logit size %dx%d outside [1, 65535]", h, w);
  const int CP = class_pad(C);
  PSEG_REQUIRE(((uintptr_t)prob & 15) == 0 && prob_offset >= 0 && (prob_offset & 3) == 0,
               "softmax_views: the probability buffer and the map's offset must be 16-byte aligned");
  PSEG_REQUIRE(prob_offset + (int64_t)B * h * w * CP <= prob_floats,
               "softmax_views: map [%d,%d,%d,%d] at float offset %lld leaves the buffer of %lld floats", B, h, w, CP,
               (long long)prob_offset, (long long)prob_floats);
  // pixels per block: both views of a run fit 32 KiB of LDS
  const int PX = CP <= 64 ? 64 : (CP <= 128 ? 32 : 16), px_shift = PX == 64 ? 6 : (PX == 32 ? 5 : 4);
  const int runs = cdiv(w, PX);
  const long long blocks = (long long)B * h * runs;
  PSEG_REQUIRE(blocks <= 0x7fffffffLL, "softmax_views: %lld blocks exceed the grid", blocks);
  const size_t lds = (size_t)(pairs ? 2 : 1) * PX * CP * sizeof(float);
  hipLaunchKernelGGL(softmax_views_kernel, dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, logits, B, pairs, C, CP, h,
                     w, PX, px_shift, runs, prob + prob_offset);
  PSEG_LAUNCH_CHECK();
  return PSEG_OK;
}

int pseg_seg_decode_ensemble(const float* prob, int64_t prob_floats, const int64_t* maps, int S, int B, int C, const int64_t* table,
                             int64_t npix_total, int Hmax, int Wmax, uint8_t* mask, uint8_t* rgb, const uint8_t* lut,
                             void* stream) {
  PSEG_REQUIRE(prob && maps && table && mask, "seg_decode_ensemble: null pointer");
  if (int e = check_decode("seg_decode_ensemble", rgb, lut, S, "maps", C, B)) return e;
  if (int e = check_packed("seg_decode_ensemble", prob, prob_floats, npix_total, Hmax, Wmax)) return e;
  const int CP = class_pad(C);
  hipLaunchKernelGGL(seg_decode_ensemble_kernel, dim3(cdiv(Wmax, kEnsTileW), cdiv(Hmax, kEnsTileH), B), dim3(256), 0,
                     (hipStream_t)stream, prob, prob_floats, maps, S, B, C, CP, table, npix_total, Hmax, Wmax, mask, rgb, lut);
  PSEG_LAUNCH_CHECK();
  return PSEG_OK;
}

int pseg_image_preprocess_windows(const uint8_t* src, int64_t src_bytes, const int64_t* table, int rows, int flag_mask, int bgr,
                                  float mean0, float mean1, float mean2, float std0, float std1, float std2, float* out, int oh,
                                  int ow, void* stream) {
  return launch_preprocess<8>("image_preprocess_windows", "window", src, src_bytes, table, rows, flag_mask, bgr,
                              Norm{{mean0, mean1, mean2}, {std0, std1, std2}}, out, oh, ow, stream);
}

int pseg_seg_decode_windows(const float* prob, int64_t prob_floats, const int64_t* groups, int S, int B, int C, int h, int w, int sy,
                            int sx, const int64_t* table, int64_t npix_total, int Hmax, int Wmax, uint8_t* mask, uint8_t* rgb,
                            const uint8_t* lut, void* stream) {
  PSEG_REQUIRE(prob && groups && table && mask, "seg_decode_windows: null pointer");
  if (int e = check_decode("seg_decode_windows", rgb, lut, S, "scales", C, B)) return e;
  PSEG_REQUIRE(h >= 1 && w >= 1 && h <= 65535 && w <= 65535, "seg_decode_windows: window size %dx%d outside [1, 65535]", h, w);
  PSEG_REQUIRE(sy >= (h + 1) / 2 && sy <= h && sx >= (w + 1) / 2 && sx <= w,
               "seg_decode_windows: stride %dx%d outside [ceil(h/2), h] x [ceil(w/2), w] of the %dx%d window", sy, sx, h, w);
  if (int e = check_packed("seg_decode_windows", prob, prob_floats, npix_total, Hmax, Wmax)) return e;
  const int CP = class_pad(C);
  hipLaunchKernelGGL(seg_decode_windows_kernel, dim3(cdiv(Wmax, kEnsTileW), cdiv(Hmax, kEnsTileH), B), dim3(256), 0,
                     (hipStream_t)stream, prob, prob_floats, groups, S, B, C, CP, h, w, FastDiv((uint32_t)sy), FastDiv((uint32_t)sx),
                     table, npix_total, Hmax, Wmax, mask, rgb, lut);
  PSEG_LAUNCH_CHECK();
  return PSEG_OK;
}

}  // extern "C"
