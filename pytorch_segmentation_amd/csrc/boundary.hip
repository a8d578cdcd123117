// Contour-aware evaluation on gfx950: the label depth of a label map, and the Boundary IoU / trimap counters built on it
// (definitions: include/pseg_amd.h).  All arithmetic is integer, so every result is exact and a function of the arguments only.
//
// depth(p) -- the Chebyshev distance from p to the nearest pixel of its image with another label, clipped to d + 1 -- is
// separable: with c(q) the distance along q's COLUMN to the nearest other label (clipped),
//     depth(p) = min(c(p), min over the pixels q of p's row at 1 <= |k| <= d of (L(q) != L(p) ? |k| : max(|k|, c(q)))).
// So there are two passes, O(d) work per pixel and no pass per class:
//  - depth_cols_kernel: one wave per strip of 64 columns x TH rows, a lane per column.  It sweeps down the column from d
//    rows above the strip to d rows below it, counting the run of equal labels (that is the distance to the change above);
//    the strip's part of the counts is parked in LDS, the first change below the strip is remembered; then it walks back up
//    through the parked counts (a count of 1 marks a change) and writes min(above, below), one byte per pixel.  Every lane
//    only reads LDS bytes it wrote itself, so the kernel has no barrier.  A sweep never leaves its own image or column.
//  - depth_rows_kernel: a block owns whole rows and walks each in segments of 256 pixels.  The labels of the segment and d
//    pixels either side (never past a row end) and their column distances sit in LDS; a thread scans outwards from its pixel
//    and stops at the first k that cannot lower the minimum any more (every term at offset k is >= k).  Because a row has
//    one owner that moves left to right and keeps the column distances of the 2d pixels it still needs in LDS, the depth can
//    overwrite the plane of column distances in place: pseg_label_depth needs no workspace beyond its own result.
//    With two maps (target, prediction) nothing is written back; the six counter rows go through a per-block LDS histogram
//    and 64-bit integer atomics, as confusion_kernel does it.
// The prediction is read through the target: where the target is void it becomes kBdVoid, in both passes.
#include <algorithm>

#include "common.h"

namespace pseg {

constexpr int kBdMaxClasses = 1024;       // pseg_confusion's bound
constexpr int kBdMaxWidth = 254;          // d + 1 fits a byte
constexpr int kBdMaxSide = 1 << 30;
constexpr int kBdCols = 64;               // columns of a strip of the column pass: one wave
constexpr int kBdSeg = 256;               // pixels of a row segment = threads of the row pass
constexpr int kBdMaxStripRows = 128;
constexpr int kBdMaxDepthBlocks = 2048, kBdMaxCountBlocks = 1024;
constexpr long long kBdVoid = -1;         // what a prediction becomes where the target is void

__device__ __forceinline__ bool bd_in(long long v, int C) { return v >= 0 && v < C; }

// NM = 1: lab0 -> out0.  NM = 2: lab0 is the target and lab1 the prediction; out0 / out1 are their planes.
template <int NM>
__global__ __launch_bounds__(kBdCols) void depth_cols_kernel(const int64_t* __restrict__ lab0, const int64_t* __restrict__ lab1,
                                                             int H, int W, int C, int d, int TH, int cstrips, int rstrips,
                                                             uint8_t* __restrict__ out0, uint8_t* __restrict__ out1) {
  extern __shared__ uint8_t bd_up[];                       // [NM][TH][kBdCols]: distance to the change above
  const int cs = blockIdx.x % cstrips;
  const int rest = blockIdx.x / cstrips;
  const int rs = rest % rstrips, b = rest / rstrips;
  const int x = cs * kBdCols + threadIdx.x;
  if (x >= W) return;                                      // (no barrier below)
  const int y0 = rs * TH, y1 = min(H, y0 + TH);
  const int ya = max(0, y0 - d), yb = min(H, y1 + d);      // rows further away cannot matter: the result is clipped to d + 1
  const int64_t img = (int64_t)b * H * W + x;
  const int cap = d + 1;
  long long prev[NM];
  int up[NM], dn[NM];
#pragma unroll
  for (int m = 0; m < NM; ++m) prev[m] = 0, up[m] = cap, dn[m] = cap;
#pragma unroll 4
  for (int y = ya; y < yb; ++y) {
    long long v[NM];
    v[0] = lab0[img + (int64_t)y * W];
    if (NM == 2) {
      const long long p = lab1[img + (int64_t)y * W];
      v[NM - 1] = bd_in(v[0], C) ? p : kBdVoid;
    }
#pragma unroll
    for (int m = 0; m < NM; ++m) {
      if (y > ya) up[m] = v[m] == prev[m] ? min(up[m] + 1, cap) : 1;     // the first row of the sweep: nothing known above
      prev[m] = v[m];
      if (y < y1) {
        if (y >= y0) bd_up[(m * TH + y - y0) * kBdCols + threadIdx.x] = (uint8_t)up[m];
      } else if (up[m] == 1 && dn[m] == cap) {
        dn[m] = y - (y1 - 1);                                            // first change below the strip (<= d)
      }
    }
  }
  for (int y = y1 - 1; y >= y0; --y) {
#pragma unroll
    for (int m = 0; m < NM; ++m) {
      const int u = bd_up[(m * TH + y - y0) * kBdCols + threadIdx.x];
      (m == 0 ? out0 : out1)[img + (int64_t)y * W] = (uint8_t)min(u, dn[m]);
      dn[m] = u == 1 ? 1 : min(dn[m] + 1, cap);                          // u == 1: row y differs from row y - 1
    }
  }
}

// NM = 1: plane0 holds the column distances of lab0 and receives its depth (with `edge`: depth_edge).  NM = 2: plane0 /
// plane1 are the column distances of target / prediction, read only; counters[6][C] is added to.
template <int NM>
__global__ __launch_bounds__(kBdSeg) void depth_rows_kernel(const int64_t* __restrict__ lab0, const int64_t* __restrict__ lab1,
                                                            int64_t rows, int H, int W, int C, int d, int edge, uint8_t* plane0,
                                                            const uint8_t* plane1, unsigned long long* __restrict__ counters) {
  extern __shared__ int64_t bd_smem[];
  const int win = kBdSeg + 2 * d, winb = (win + 15) & ~15;
  int64_t* sl = bd_smem;                                   // [NM][win]  labels of the window
  uint8_t* sc = reinterpret_cast<uint8_t*>(sl + NM * win);  // [NM][winb] their column distances
  unsigned* hist = reinterpret_cast<unsigned*>(sc + NM * winb);   // [6][C], NM == 2
  const int tid = threadIdx.x, cap = d + 1;
  if (NM == 2) {
    for (int i = tid; i < 6 * C; i += kBdSeg) hist[i] = 0;
    __syncthreads();
  }
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const int y = (int)(row % H);
    const int64_t base = row * W;
    for (int xs = 0; xs < W; xs += kBdSeg) {
      const int lo = xs - d;                               // the window is [lo, lo + win), cut to [0, W) of this row
      for (int i = tid; i < win; i += kBdSeg) {
        const int x = lo + i;
        if (x < 0 || x >= W) continue;
        const long long t = lab0[base + x];
        sl[i] = t;
        if (NM == 2) sl[(NM - 1) * win + i] = bd_in(t, C) ? (long long)lab1[base + x] : kBdVoid;
      }
      if (xs == 0) {
        for (int i = tid; i < win; i += kBdSeg) {
          const int x = lo + i;
          if (x < 0 || x >= W) continue;
          sc[i] = plane0[base + x];
          if (NM == 2) sc[(NM - 1) * winb + i] = plane1[base + x];
        }
      } else {
        // slide: the last 2d entries move to the front (they may already be overwritten in plane0), the rest is new and lies
        // right of everything this block has written
        uint8_t keep[NM][2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int i = tid + j * kBdSeg;
#pragma unroll
          for (int m = 0; m < NM; ++m) keep[m][j] = i < 2 * d ? sc[m * winb + kBdSeg + i] : 0;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int i = tid + j * kBdSeg;
          if (i < 2 * d) {
#pragma unroll
            for (int m = 0; m < NM; ++m) sc[m * winb + i] = keep[m][j];
          }
        }
        for (int i = 2 * d + tid; i < win; i += kBdSeg) {
          const int x = lo + i;
          if (x >= W) continue;
          sc[i] = plane0[base + x];
          if (NM == 2) sc[(NM - 1) * winb + i] = plane1[base + x];
        }
      }
      __syncthreads();
      const int x = xs + tid;
      if (x < W) {
        const int i = tid + d;
        int dep[NM];
#pragma unroll
        for (int m = 0; m < NM; ++m) {
          const int64_t* l = sl + m * win + i;
          const uint8_t* c = sc + m * winb + i;
          const int64_t me = l[0];
          int best = c[0];
          for (int k = 1; k < best; ++k) {                 // a term at offset k is >= k: k >= best ends the search
            if (k <= x) best = min(best, l[-k] != me ? k : max(k, (int)c[-k]));
            if (x + k < W) best = min(best, l[k] != me ? k : max(k, (int)c[k]));
          }
          dep[m] = best;
        }
        const int e = min(min(x + 1, W - x), min(y + 1, H - y));
        if (NM == 1) {
          plane0[base + x] = (uint8_t)(edge ? min(dep[0], e) : dep[0]);
        } else {
          const long long t = sl[i], p = sl[(NM - 1) * win + i];
          if (bd_in(t, C)) {                               // a void target counts nowhere, and made the prediction void
            const bool gt = min(dep[0], e) <= d, pr = min(dep[NM - 1], e) <= d, pin = bd_in(p, C);
            if (gt) atomicAdd(&hist[C + (int)t], 1u);
            if (gt && pr && p == t) atomicAdd(&hist[(int)t], 1u);
            if (pr && pin) atomicAdd(&hist[2 * C + (int)p], 1u);
            if (dep[0] <= d) {                             // trimap: pseg_confusion's rules, the image border is no contour
              atomicAdd(&hist[(p == t ? 3 : 4) * C + (int)t], 1u);
              if (pin && p != t) atomicAdd(&hist[5 * C + (int)p], 1u);
            }
          }
        }
      }
      __syncthreads();
    }
  }
  if (NM == 2) {
    for (int i = tid; i < 6 * C; i += kBdSeg)
      if (hist[i]) atomicAdd(&counters[i], (unsigned long long)hist[i]);
  }
}

static inline int64_t bd_up16(int64_t v) { return (v + 15) / 16 * 16; }

struct BdPlan {
  int TH, cstrips, rstrips;
  int64_t npix, cblocks;
};

static bool bd_sizes_ok(int B, int H, int W, int d) {
  return B >= 1 && H >= 1 && W >= 1 && H <= kBdMaxSide && W <= kBdMaxSide && d >= 1 && d <= kBdMaxWidth &&
         (int64_t)B * H <= (1ll << 40) / W;
}

static BdPlan bd_plan(int B, int H, int W, int d) {
  BdPlan p;
  p.TH = std::min(std::min(std::max(4 * d, 32), kBdMaxStripRows), H);
  p.cstrips = cdiv(W, kBdCols);
  p.rstrips = cdiv(H, p.TH);
  p.npix = (int64_t)B * H * W;
  p.cblocks = (int64_t)B * p.rstrips * p.cstrips;
  return p;
}

static int bd_check(const char* fn, int B, int H, int W, int C, int d) {
  PSEG_REQUIRE(B >= 1 && H >= 1 && W >= 1, "%s: sizes B, H, W = %d, %d, %d must be >= 1", fn, B, H, W);
  PSEG_REQUIRE(H <= kBdMaxSide && W <= kBdMaxSide, "%s: H, W = %d, %d above 2^30", fn, H, W);
  PSEG_REQUIRE(C >= 1 && C <= kBdMaxClasses, "%s: class count C = %d outside [1, %d]", fn, C, kBdMaxClasses);
  PSEG_REQUIRE(d >= 1 && d <= kBdMaxWidth, "%s: width d = %d outside [1, %d]", fn, d, kBdMaxWidth);
  PSEG_REQUIRE((int64_t)B * H <= (1ll << 40) / W, "%s: B * H * W = %d * %d * %d exceeds 2^40 pixels", fn, B, H, W);
  PSEG_REQUIRE(bd_plan(B, H, W, d).cblocks < (1ll << 31), "%s: B, H, W = %d, %d, %d make more than 2^31 column strips", fn, B, H, W);
  return PSEG_OK;
}

}  // namespace pseg

using namespace pseg;

extern "C" {

int pseg_label_depth(const int64_t* labels, int B, int H, int W, int C, int d, int edge, uint8_t* depth, void* stream) {
  PSEG_REQUIRE(labels && depth, "label_depth: null pointer");
  if (int rc = bd_check("label_depth", B, H, W, C, d)) return rc;
  const hipStream_t st = (hipStream_t)stream;
  const BdPlan pl = bd_plan(B, H, W, d);
  hipLaunchKernelGGL(depth_cols_kernel<1>, dim3((unsigned)pl.cblocks), dim3(kBdCols), (size_t)pl.TH * kBdCols, st, labels,
                     (const int64_t*)nullptr, H, W, C, d, pl.TH, pl.cstrips, pl.rstrips, depth, (uint8_t*)nullptr);
  const int64_t rows = (int64_t)B * H;
  const int win = kBdSeg + 2 * d, winb = (win + 15) & ~15;
  const dim3 grid((unsigned)(rows < kBdMaxDepthBlocks ? rows : kBdMaxDepthBlocks));
  hipLaunchKernelGGL(depth_rows_kernel<1>, grid, dim3(kBdSeg), (size_t)win * 8 + winb, st, labels, (const int64_t*)nullptr, rows, H,
                     W, C, d, edge != 0, depth, (const uint8_t*)nullptr, (unsigned long long*)nullptr);
  PSEG_LAUNCH_CHECK();
  return PSEG_OK;
}

int64_t pseg_boundary_counts_workspace_bytes(int B, int H, int W, int d) {
  if (!bd_sizes_ok(B, H, W, d)) return -1;
  return 2 * bd_up16((int64_t)B * H * W);
}

int pseg_boundary_counts(const int64_t* pred, const int64_t* target, int B, int H, int W, int C, int d, int64_t* counters,
                         void* workspace, int64_t workspace_bytes, void* stream) {
  PSEG_REQUIRE(pred && target && counters && workspace, "boundary_counts: null pointer");
  if (int rc = bd_check("boundary_counts", B, H, W, C, d)) return rc;
  const BdPlan pl = bd_plan(B, H, W, d);
  const int64_t need = 2 * bd_up16(pl.npix);
  PSEG_REQUIRE(workspace_bytes >= need, "boundary_counts: workspace too small (%lld < %lld bytes)", (long long)workspace_bytes,
               (long long)need);
  const hipStream_t st = (hipStream_t)stream;
  uint8_t* ct = (uint8_t*)workspace;
  uint8_t* cp = ct + bd_up16(pl.npix);
  hipLaunchKernelGGL(depth_cols_kernel<2>, dim3((unsigned)pl.cblocks), dim3(kBdCols), (size_t)2 * pl.TH * kBdCols, st, target, pred,
                     H, W, C, d, pl.TH, pl.cstrips, pl.rstrips, ct, cp);
  const int64_t rows = (int64_t)B * H;
  const int win = kBdSeg + 2 * d, winb = (win + 15) & ~15;
  const dim3 grid((unsigned)(rows < kBdMaxCountBlocks ? rows : kBdMaxCountBlocks));
  hipLaunchKernelGGL(depth_rows_kernel<2>, grid, dim3(kBdSeg), (size_t)2 * win * 8 + 2 * winb + (size_t)6 * C * 4, st, target, pred,
                     rows, H, W, C, d, 0, ct, (const uint8_t*)cp, (unsigned long long*)counters);
  PSEG_LAUNCH_CHECK();
  return PSEG_OK;
}

}  // extern "C"
