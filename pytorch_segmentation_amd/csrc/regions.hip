// Connected regions of the inference masks on gfx950: labelling, one record per region, and cleanup (specks dropped, holes
// filled, the largest region of a class kept).  The data layout is infer.hip's: a ragged batch of uint8 masks packed in one
// buffer under a device table of {pixel offset, H, W}.  All arithmetic is integer, so every result is exact.
//  - mask_label: labels[p] = y*W + x of the first pixel, in raster order, of p's component (within its own photo).  Three
//    launches, no "repeat until nothing changes": (1) a block owns a kRegTile x kRegTile tile and runs a union-find over it
//    in LDS; (2) the pixel pairs that straddle a tile border are united in global memory; (3) every pixel is pointed at its
//    root.  A union links the LARGER root to the smaller index with an integer atomicMin, so the invariant parent[i] <= i
//    holds at every instant, a tree's root is its smallest index -- the component's first pixel -- and every walk up a tree
//    strictly decreases: that is the termination argument each loop below refers to.
//  - mask_regions: root flags labels[p] == p -> exclusive scan along the packed buffer = the record index of each root, so
//    records come in (photo, label) order without a sort; then one pass adds every pixel into its record with 64-bit
//    integer atomics, after folding runs of one region per thread and per wave.
//  - mask_clean: areas per root (integer atomics), optionally the largest region per (photo, class) (one 64-bit atomicMax
//    of area << 32 | ~label), one serial walk per ROOT to the class it takes, one pass that writes mask (and colours).
#include "common.h"

namespace pseg {

constexpr int kRegTile = PSEG_REGIONS_TILE;       // tile edge of the LDS union-find
constexpr int kRegThreads = 256;
constexpr int kRegRun = 8;                        // consecutive pixels one thread folds before it touches global atomics
constexpr int kRegScanChunk = kRegThreads * 16;   // packed positions per block of the flag scan
constexpr int kRegMaxCleanBatch = PSEG_REGIONS_MAX_LARGEST_BATCH;
typedef unsigned long long u64;

static_assert(kRegTile * kRegTile % kRegThreads == 0 && 2 * kRegTile <= kRegThreads, "tile / block shape");

__device__ __forceinline__ bool reg_ok(int64_t off, int64_t H, int64_t W, int64_t cap, int Hmax, int Wmax) {
  return off >= 0 && H >= 1 && W >= 1 && H <= Hmax && W <= Wmax && H * W <= cap && off <= cap - H * W;
}

// ---- union-find on an int array with parent[i] <= i (LDS or global)
__device__ __forceinline__ int uf_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int uf_find(const int* par, int x) {
  // ends: parent[i] <= i always, so every step either stops (parent[x] == x) or moves to a strictly smaller index >= 0
  for (;;) {
    const int p = uf_load(par + x);
    if (p == x) return x;
    x = p;
  }
}

__device__ __forceinline__ void uf_union(int* par, int a, int b) {
  // ends: each turn either returns or replaces a by `old` < a (the parent a had when the atomicMin ran, which is not a
  // itself and never larger), while find() only lowers a and b: a + b strictly decreases and is bounded below by 0.
  // A parent word only ever decreases (atomicMin), so nothing a turn has read can move back up.
  for (;;) {
    a = uf_find(par, a);
    b = uf_find(par, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(par + a, b);          // a > b: link the larger root below the smaller index
    if (old == a) return;                           // a was still a root: linked
    a = old;                                        // a had been linked meanwhile (old < a): unite its parent with b instead
  }
}

// ------------------------------------------------------------------ labelling
__global__ __launch_bounds__(kRegThreads) void label_tile_kernel(const uint8_t* __restrict__ mask,
                                                                  const int64_t* __restrict__ table, int64_t cap, int Hmax,
                                                                  int Wmax, int conn8, int* __restrict__ labels) {
  __shared__ int par[kRegTile * kRegTile];
  __shared__ uint8_t cls[kRegTile * kRegTile];
  const int b = blockIdx.z;
  const int64_t off = table[3 * b], H64 = table[3 * b + 1], W64 = table[3 * b + 2];
  if (!reg_ok(off, H64, W64, cap, Hmax, Wmax)) return;       // bad record: nothing read or written
  const int H = (int)H64, W = (int)W64;
  const int ys = blockIdx.y * kRegTile, xs = blockIdx.x * kRegTile;
  if (ys >= H || xs >= W) return;                            // ragged batch: block-uniform exit
  const int th = min(kRegTile, H - ys), tw = min(kRegTile, W - xs);
  const uint8_t* m = mask + off;
  for (int p = threadIdx.x; p < kRegTile * kRegTile; p += kRegThreads) {
    const int ly = p / kRegTile, lx = p % kRegTile;
    cls[p] = (ly < th && lx < tw) ? m[(int64_t)(ys + ly) * W + xs + lx] : 0;
    par[p] = p;
  }
  __syncthreads();
  for (int p = threadIdx.x; p < kRegTile * kRegTile; p += kRegThreads) {
    const int ly = p / kRegTile, lx = p % kRegTile;
    if (ly >= th || lx >= tw) continue;
    const uint8_t c = cls[p];
    if (lx > 0 && cls[p - 1] == c) uf_union(par, p, p - 1);
    if (ly > 0 && cls[p - kRegTile] == c) uf_union(par, p, p - kRegTile);
    if (conn8 && ly > 0) {
      if (lx > 0 && cls[p - kRegTile - 1] == c) uf_union(par, p, p - kRegTile - 1);
      if (lx + 1 < tw && cls[p - kRegTile + 1] == c) uf_union(par, p, p - kRegTile + 1);
    }
  }
  __syncthreads();
  int* lab = labels + off;
  for (int p = threadIdx.x; p < kRegTile * kRegTile; p += kRegThreads) {
    const int ly = p / kRegTile, lx = p % kRegTile;
    if (ly >= th || lx >= tw) continue;
    const int r = uf_find(par, p);     // local raster order = photo raster order inside a tile: the local minimum is the tile's first pixel
    lab[(int64_t)(ys + ly) * W + xs + lx] = (ys + r / kRegTile) * W + xs + r % kRegTile;
  }
}

// One wave per tile: lanes 0..T-1 own the tile's top row and unite across the border above (up, and with 8-connectivity
// up-left and up-right); lanes T..2T-1 own its left column and unite across the border to the left (left, and with
// 8-connectivity up-left and down-left where those stay in this tile row -- the ones that also cross a horizontal border
// are the top-row lanes' pairs).  Every pair of adjacent pixels in different tiles is one of these.
__global__ __launch_bounds__(2 * kRegTile) void label_merge_kernel(const uint8_t* __restrict__ mask,
                                                                    const int64_t* __restrict__ table, int64_t cap, int Hmax,
                                                                    int Wmax, int conn8, int* __restrict__ labels) {
  const int b = blockIdx.z;
  const int64_t off = table[3 * b], H64 = table[3 * b + 1], W64 = table[3 * b + 2];
  if (!reg_ok(off, H64, W64, cap, Hmax, Wmax)) return;
  const int H = (int)H64, W = (int)W64;
  const int ys = blockIdx.y * kRegTile, xs = blockIdx.x * kRegTile;
  if (ys >= H || xs >= W) return;
  const uint8_t* m = mask + off;
  int* lab = labels + off;
  const int t = threadIdx.x;
  if (t < kRegTile) {
    const int y = ys, x = xs + t;
    if (y == 0 || x >= W) return;
    const int i = y * W + x;
    const uint8_t c = m[i];
    if (m[i - W] == c) uf_union(lab, i, i - W);
    if (conn8) {
      if (x > 0 && m[i - W - 1] == c) uf_union(lab, i, i - W - 1);
      if (x + 1 < W && m[i - W + 1] == c) uf_union(lab, i, i - W + 1);
    }
  } else {
    const int ly = t - kRegTile, y = ys + ly, x = xs;
    if (x == 0 || y >= H) return;
    const int i = y * W + x;
    const uint8_t c = m[i];
    if (m[i - 1] == c) uf_union(lab, i, i - 1);
    if (conn8) {
      if (ly > 0 && m[i - W - 1] == c) uf_union(lab, i, i - W - 1);
      if (ly < kRegTile - 1 && y + 1 < H && m[i + W - 1] == c) uf_union(lab, i, i + W - 1);
    }
  }
}

// photo-grid kernels: grid (chunks of a photo's flat pixels, B); a thread owns kRegRun consecutive pixels
__global__ __launch_bounds__(kRegThreads) void label_flatten_kernel(const int64_t* __restrict__ table, int64_t cap, int Hmax,
                                                                     int Wmax, int* __restrict__ labels) {
  const int b = blockIdx.y;
  const int64_t off = table[3 * b], H = table[3 * b + 1], W = table[3 * b + 2];
  if (!reg_ok(off, H, W, cap, Hmax, Wmax)) return;
  const int n = (int)(H * W);
  int* lab = labels + off;
  // a store here replaces a parent by the root of the same tree (smaller or equal): parent[i] <= i still holds for the
  // finds of the other threads that run beside it
  for (int64_t i = (int64_t)blockIdx.x * kRegThreads * kRegRun + threadIdx.x, k = 0; k < kRegRun && i < n; ++k, i += kRegThreads)
    lab[i] = uf_find(lab, (int)i);
}

// ------------------------------------------------------------------ records
struct RegAcc {
  int k;                 // record index, -1: nothing pending
  u64 area, x0, y0, x1, y1, sx, sy, sxx, sxy, syy;
};

__device__ __forceinline__ void acc_flush(const RegAcc& a, int64_t* records) {
  u64* r = reinterpret_cast<u64*>(records) + (int64_t)a.k * PSEG_REGION_WORDS;
  atomicAdd(r + 2, a.area);
  atomicMin(r + 3, a.x0);
  atomicMin(r + 4, a.y0);
  atomicMax(r + 5, a.x1);
  atomicMax(r + 6, a.y1);
  atomicAdd(r + 7, a.sx);
  atomicAdd(r + 8, a.sy);
  atomicAdd(r + 9, a.sxx);
  atomicAdd(r + 10, a.sxy);
  atomicAdd(r + 11, a.syy);
}

__device__ __forceinline__ u64 wave_add64(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ u64 wave_min64(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64 u = __shfl_xor(v, o, 64);
    v = u < v ? u : v;
  }
  return v;
}
__device__ __forceinline__ u64 wave_max64(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64 u = __shfl_xor(v, o, 64);
    v = u > v ? u : v;
  }
  return v;
}

__global__ __launch_bounds__(kRegThreads) void region_flag_kernel(const int* __restrict__ labels,
                                                                   const int64_t* __restrict__ table, int64_t cap, int Hmax,
                                                                   int Wmax, uint8_t* __restrict__ flag) {
  const int b = blockIdx.y;
  const int64_t off = table[3 * b], H = table[3 * b + 1], W = table[3 * b + 2];
  if (!reg_ok(off, H, W, cap, Hmax, Wmax)) return;
  const int n = (int)(H * W);
  for (int64_t i = (int64_t)blockIdx.x * kRegThreads * kRegRun + threadIdx.x, k = 0; k < kRegRun && i < n; ++k, i += kRegThreads)
    if (labels[off + i] == (int)i) flag[off + i] = 1;         // the buffer was zeroed: only roots are written
}

__device__ __forceinline__ unsigned reg_block_excl_scan(unsigned v, unsigned* sh, unsigned& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  unsigned inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned u = __shfl_up(inc, o, 64);
    if (lane >= o) inc += u;
  }
  if (lane == 63) sh[w] = inc;
  __syncthreads();
  unsigned offs = 0;
#pragma unroll
  for (int i = 0; i < 3; ++i) offs += (i < w) ? sh[i] : 0u;
  total = sh[0] + sh[1] + sh[2] + sh[3];
  return offs + inc - v;
}

// flags of the 16 packed positions of a thread (zero past the end), as bytes of four words
__device__ __forceinline__ unsigned load_flags(const uint8_t* __restrict__ flag, int64_t q0, int64_t npix, unsigned f[16]) {
  unsigned s = 0;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    f[j] = (q0 + j < npix) ? flag[q0 + j] : 0u;
    s += f[j];
  }
  return s;
}

__global__ __launch_bounds__(kRegThreads) void region_scan_sums_kernel(const uint8_t* __restrict__ flag, int64_t npix,
                                                                        unsigned* __restrict__ bsum) {
  __shared__ unsigned sh[4];
  unsigned f[16], total;
  const unsigned s = load_flags(flag, (int64_t)blockIdx.x * kRegScanChunk + threadIdx.x * 16, npix, f);
  reg_block_excl_scan(s, sh, total);
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// one block: in-place exclusive scan of the nb block sums (as lovasz_scan_rows_kernel does it); count[0] = their total
__global__ __launch_bounds__(kRegThreads) void region_scan_blocks_kernel(unsigned* __restrict__ bsum, unsigned nb,
                                                                          int64_t* __restrict__ count) {
  __shared__ unsigned sh[4];
  const unsigned chunk = (nb + kRegThreads - 1) / kRegThreads;
  const unsigned lo = min(nb, threadIdx.x * chunk), hi = min(nb, lo + chunk);
  unsigned s = 0;
  for (unsigned i = lo; i < hi; ++i) s += bsum[i];
  unsigned total;
  unsigned run = reg_block_excl_scan(s, sh, total);
  for (unsigned i = lo; i < hi; ++i) {
    const unsigned v = bsum[i];
    bsum[i] = run;
    run += v;
  }
  if (threadIdx.x == 0) count[0] = (int64_t)total;
}

// ridx[q] = record index of the root at packed position q; records below max_regions get their neutral start values
__global__ __launch_bounds__(kRegThreads) void region_scan_write_kernel(const uint8_t* __restrict__ flag, int64_t npix,
                                                                         const unsigned* __restrict__ bsum, int64_t max_regions,
                                                                         int* __restrict__ ridx, int64_t* __restrict__ records) {
  __shared__ unsigned sh[4];
  unsigned f[16], total;
  const int64_t q0 = (int64_t)blockIdx.x * kRegScanChunk + threadIdx.x * 16;
  const unsigned s = load_flags(flag, q0, npix, f);
  unsigned run = bsum[blockIdx.x] + reg_block_excl_scan(s, sh, total);
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    if (f[j]) {
      ridx[q0 + j] = (int)run;
      if ((int64_t)run < max_regions) {
        int64_t* r = records + (int64_t)run * PSEG_REGION_WORDS;
#pragma unroll
        for (int w = 0; w < PSEG_REGION_WORDS; ++w) r[w] = (w == 3 || w == 4) ? INT64_MAX : 0;
      }
      ++run;
    }
  }
}

__global__ __launch_bounds__(kRegThreads) void region_accumulate_kernel(const uint8_t* __restrict__ mask,
                                                                         const int* __restrict__ labels,
                                                                         const int64_t* __restrict__ table, int64_t cap, int Hmax,
                                                                         int Wmax, const int* __restrict__ ridx, int64_t max_regions,
                                                                         int64_t* __restrict__ records) {
  const int b = blockIdx.y;
  const int64_t off = table[3 * b], H = table[3 * b + 1], W64 = table[3 * b + 2];
  if (!reg_ok(off, H, W64, cap, Hmax, Wmax)) return;
  const int n = (int)(H * W64), W = (int)W64;
  if ((int64_t)blockIdx.x * kRegThreads * kRegRun >= n) return;        // block-uniform
  const int64_t i0 = ((int64_t)blockIdx.x * kRegThreads + threadIdx.x) * kRegRun;
  RegAcc a = {-1, 0, ~0ull, ~0ull, 0, 0, 0, 0, 0, 0, 0};
  int prev_root = -1, prev_k = -1;
  int y = i0 < n ? (int)(i0 / W) : 0, x = i0 < n ? (int)(i0 - (int64_t)y * W) : 0;
  for (int j = 0; j < kRegRun && i0 + j < n; ++j) {
    const int i = (int)(i0 + j);
    const int root = labels[off + i];
    if (root != prev_root) {
      prev_root = root;
      prev_k = ridx[off + root];
      if ((int64_t)prev_k >= max_regions) prev_k = -1;                 // past the capacity: counted, not recorded
    }
    if (prev_k >= 0 && root == i) {                                    // the root names its record (plain stores: words 0, 1)
      int64_t* r = records + (int64_t)prev_k * PSEG_REGION_WORDS;
      r[0] = (int64_t)b * 256 + mask[off + i];
      r[1] = root;
    }
    if (prev_k != a.k) {
      if (a.k >= 0) acc_flush(a, records);
      a.k = prev_k;
      a.area = 0, a.x0 = ~0ull, a.y0 = ~0ull, a.x1 = 0, a.y1 = 0, a.sx = 0, a.sy = 0, a.sxx = 0, a.sxy = 0, a.syy = 0;
    }
    if (a.k >= 0) {
      const u64 ux = (u64)x, uy = (u64)y;
      a.area += 1;
      a.x0 = ux < a.x0 ? ux : a.x0;
      a.y0 = uy < a.y0 ? uy : a.y0;
      a.x1 = ux > a.x1 ? ux : a.x1;
      a.y1 = uy > a.y1 ? uy : a.y1;
      a.sx += ux, a.sy += uy, a.sxx += ux * ux, a.sxy += ux * uy, a.syy += uy * uy;
    }
    if (++x == W) x = 0, ++y;
  }
  // what is left in each lane: if the whole wave holds the same record, fold it with shuffles and let one lane add it
  const int k0 = __shfl(a.k, 0, 64);
  if (__all(a.k == k0)) {
    if (k0 < 0) return;
    a.area = wave_add64(a.area);
    a.x0 = wave_min64(a.x0), a.y0 = wave_min64(a.y0);
    a.x1 = wave_max64(a.x1), a.y1 = wave_max64(a.y1);
    a.sx = wave_add64(a.sx), a.sy = wave_add64(a.sy);
    a.sxx = wave_add64(a.sxx), a.sxy = wave_add64(a.sxy), a.syy = wave_add64(a.syy);
    if ((threadIdx.x & 63) == 0) acc_flush(a, records);
  } else if (a.k >= 0) {
    acc_flush(a, records);
  }
}

// ------------------------------------------------------------------ cleanup
// roots: area = 0 (only the roots' words of the area array are ever used)
__global__ __launch_bounds__(kRegThreads) void clean_init_kernel(const int* __restrict__ labels, const int64_t* __restrict__ table,
                                                                  int64_t cap, int Hmax, int Wmax, int* __restrict__ area) {
  const int b = blockIdx.y;
  const int64_t off = table[3 * b], H = table[3 * b + 1], W = table[3 * b + 2];
  if (!reg_ok(off, H, W, cap, Hmax, Wmax)) return;
  const int n = (int)(H * W);
  for (int64_t i = (int64_t)blockIdx.x * kRegThreads * kRegRun + threadIdx.x, k = 0; k < kRegRun && i < n; ++k, i += kRegThreads)
    if (labels[off + i] == (int)i) area[off + i] = 0;
}

__global__ __launch_bounds__(kRegThreads) void clean_area_kernel(const int* __restrict__ labels, const int64_t* __restrict__ table,
                                                                  int64_t cap, int Hmax, int Wmax, int* __restrict__ area) {
  const int b = blockIdx.y;
  const int64_t off = table[3 * b], H = table[3 * b + 1], W = table[3 * b + 2];
  if (!reg_ok(off, H, W, cap, Hmax, Wmax)) return;
  const int n = (int)(H * W);
  if ((int64_t)blockIdx.x * kRegThreads * kRegRun >= n) return;        // block-uniform
  const int64_t i0 = ((int64_t)blockIdx.x * kRegThreads + threadIdx.x) * kRegRun;
  int root = -1, cnt = 0;
  for (int j = 0; j < kRegRun && i0 + j < n; ++j) {
    const int r = labels[off + i0 + j];
    if (r != root) {
      if (cnt) atomicAdd(area + off + root, cnt);
      root = r;
      cnt = 0;
    }
    ++cnt;
  }
  const int r0 = __shfl(root, 0, 64);
  if (__all(root == r0)) {
    if (r0 < 0) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(area + off + r0, cnt);
  } else if (cnt) {
    atomicAdd(area + off + root, cnt);
  }
}

// larger area wins, then the smaller label
__device__ __forceinline__ u64 largest_key(int area, int label) { return ((u64)(unsigned)area << 32) | (u64)(0xFFFFFFFFu - (unsigned)label); }

__global__ __launch_bounds__(kRegThreads) void clean_largest_kernel(const uint8_t* __restrict__ mask, const int* __restrict__ labels,
                                                                     const int64_t* __restrict__ table, int64_t cap, int Hmax,
                                                                     int Wmax, const int* __restrict__ area, u64* __restrict__ best) {
  const int b = blockIdx.y;
  const int64_t off = table[3 * b], H = table[3 * b + 1], W = table[3 * b + 2];
  if (!reg_ok(off, H, W, cap, Hmax, Wmax)) return;
  const int n = (int)(H * W);
  for (int64_t i = (int64_t)blockIdx.x * kRegThreads * kRegRun + threadIdx.x, k = 0; k < kRegRun && i < n; ++k, i += kRegThreads) {
    if (labels[off + i] != (int)i) continue;
    const int c = mask[off + i];
    if (c >= 1) atomicMax(best + (int64_t)b * 256 + c, largest_key(area[off + i], (int)i));
  }
}

__device__ __forceinline__ bool clean_small(const uint8_t* m, const int* area, const u64* best, int root, int min_area) {
  const int a = area[root];
  if (a < min_area) return true;
  if (best) {
    const int c = m[root];
    if (c >= 1 && best[c] != largest_key(a, root)) return true;
  }
  return false;
}

// one serial walk per root: the class its component takes
__global__ __launch_bounds__(kRegThreads) void clean_walk_kernel(const uint8_t* __restrict__ mask, const int* __restrict__ labels,
                                                                  const int64_t* __restrict__ table, int64_t cap, int Hmax, int Wmax,
                                                                  int min_area, const int* __restrict__ area,
                                                                  const u64* __restrict__ best, uint8_t* __restrict__ rcls) {
  const int b = blockIdx.y;
  const int64_t off = table[3 * b], H = table[3 * b + 1], W64 = table[3 * b + 2];
  if (!reg_ok(off, H, W64, cap, Hmax, Wmax)) return;
  const int n = (int)(H * W64), W = (int)W64;
  const uint8_t* m = mask + off;
  const int* lab = labels + off;
  const int* ar = area + off;
  const u64* bb = best ? best + (int64_t)b * 256 : nullptr;
  for (int64_t i = (int64_t)blockIdx.x * kRegThreads * kRegRun + threadIdx.x, k = 0; k < kRegRun && i < n; ++k, i += kRegThreads) {
    if (lab[i] != (int)i) continue;
    int cur = (int)i;
    // ends: the pixel above or left of a first pixel `cur` has a flat index below cur and its root is not above it, so
    // cur strictly decreases; the walk stops at the latest at index 0, the photo's corner
    while (cur > 0 && clean_small(m, ar, bb, cur, min_area)) cur = lab[cur >= W ? cur - W : cur - 1];
    rcls[off + i] = m[cur];
  }
}

// mask_out = the class of each pixel's root (rcls), or, without rcls, the mask itself; colours from the result
__global__ __launch_bounds__(kRegThreads) void clean_write_kernel(const uint8_t* mask, const int* __restrict__ labels,
                                                                   const int64_t* __restrict__ table, int64_t cap, int Hmax, int Wmax,
                                                                   const uint8_t* __restrict__ rcls, uint8_t* mask_out,
                                                                   uint8_t* __restrict__ rgb, const uint8_t* __restrict__ lut) {
  const int b = blockIdx.y;
  const int64_t off = table[3 * b], H = table[3 * b + 1], W = table[3 * b + 2];
  if (!reg_ok(off, H, W, cap, Hmax, Wmax)) return;
  const int n = (int)(H * W);
  for (int64_t i = (int64_t)blockIdx.x * kRegThreads * kRegRun + threadIdx.x, k = 0; k < kRegRun && i < n; ++k, i += kRegThreads) {
    const int64_t q = off + i;
    const uint8_t c = rcls ? rcls[off + labels[q]] : mask[q];
    mask_out[q] = c;
    if (rgb) {
      rgb[3 * q] = lut[3 * c];
      rgb[3 * q + 1] = lut[3 * c + 1];
      rgb[3 * q + 2] = lut[3 * c + 2];
    }
  }
}

// ------------------------------------------------------------------ workspace
struct RegPlan {
  int64_t words, bytes1, bsum, best, bytes;   // byte offsets: int32 per pixel, one byte per pixel, block sums, best table
  int nb;
};

static inline int64_t up16(int64_t v) { return (v + 15) / 16 * 16; }

static RegPlan reg_plan(int64_t npix) {
  RegPlan p;
  p.nb = (int)((npix + kRegScanChunk - 1) / kRegScanChunk);
  p.words = 0;
  p.bytes1 = p.words + up16(npix * 4);
  p.bsum = p.bytes1 + up16(npix);
  p.best = p.bsum + up16((int64_t)(p.nb + 1) * 4);
  p.bytes = p.best + (npix < kRegMaxCleanBatch ? npix : (int64_t)kRegMaxCleanBatch) * 256 * 8;
  return p;
}

static int reg_common(const char* fn, const void* table, int B, int64_t npix_total, int Hmax, int Wmax) {
  PSEG_REQUIRE(table != nullptr, "%s: null pointer", fn);
  PSEG_REQUIRE(B >= 1 && B <= 65535, "%s: batch %d outside [1, 65535]", fn, B);
  PSEG_REQUIRE(Hmax >= 1 && Wmax >= 1 && Hmax <= 65535 && Wmax <= 65535, "%s: largest image %dx%d outside [1, 65535]", fn, Hmax, Wmax);
  PSEG_REQUIRE((int64_t)Hmax * Wmax < (1ll << 31), "%s: largest image %dx%d has 2^31 pixels or more (labels are int32)", fn, Hmax, Wmax);
  PSEG_REQUIRE(npix_total >= 1 && npix_total < (1ll << 40), "%s: npix_total %lld", fn, (long long)npix_total);
  return PSEG_OK;
}

static inline dim3 photo_grid(int Hmax, int Wmax, int B) {
  return dim3(cdiv((int64_t)Hmax * Wmax, kRegThreads * kRegRun), B);
}

}  // namespace pseg

using namespace pseg;

extern "C" {

int64_t pseg_regions_workspace_bytes(int64_t npix_total, int64_t max_regions) {
  if (npix_total < 1 || npix_total >= (1ll << 40) || max_regions < 0) return -1;
  return reg_plan(npix_total).bytes;
}

int pseg_mask_label(const uint8_t* mask, const int64_t* table, int B, int64_t npix_total, int Hmax, int Wmax, int connectivity,
                    int* labels, void* ws, int64_t ws_bytes, void* stream) {
  PSEG_REQUIRE(mask && table && labels, "mask_label: null pointer");
  if (int rc = reg_common("mask_label", table, B, npix_total, Hmax, Wmax)) return rc;
  PSEG_REQUIRE(connectivity == 4 || connectivity == 8, "mask_label: connectivity %d is neither 4 nor 8", connectivity);
  (void)ws;
  (void)ws_bytes;                                       // the labels array is the only state of the union-find
  const hipStream_t st = (hipStream_t)stream;
  const int conn8 = connectivity == 8;
  const dim3 tiles(cdiv(Wmax, kRegTile), cdiv(Hmax, kRegTile), B);
  hipLaunchKernelGGL(label_tile_kernel, tiles, dim3(kRegThreads), 0, st, mask, table, npix_total, Hmax, Wmax, conn8, labels);
  hipLaunchKernelGGL(label_merge_kernel, tiles, dim3(2 * kRegTile), 0, st, mask, table, npix_total, Hmax, Wmax, conn8, labels);
  hipLaunchKernelGGL(label_flatten_kernel, photo_grid(Hmax, Wmax, B), dim3(kRegThreads), 0, st, table, npix_total, Hmax, Wmax,
                     labels);
  PSEG_LAUNCH_CHECK();
  return PSEG_OK;
}

int pseg_mask_regions(const uint8_t* mask, const int* labels, const int64_t* table, int B, int64_t npix_total, int Hmax, int Wmax,
                      int64_t max_regions, int64_t* records, int64_t* count, void* ws, int64_t ws_bytes, void* stream) {
  PSEG_REQUIRE(mask && labels && table && count && ws, "mask_regions: null pointer");
  if (int rc = reg_common("mask_regions", table, B, npix_total, Hmax, Wmax)) return rc;
  PSEG_REQUIRE(npix_total < (1ll << 31), "mask_regions: npix_total %lld; record indices are int32", (long long)npix_total);
  PSEG_REQUIRE(max_regions >= 0 && (max_regions == 0 || records), "mask_regions: max_regions %lld needs a records buffer",
               (long long)max_regions);
  const RegPlan pl = reg_plan(npix_total);
  PSEG_REQUIRE(ws_bytes >= pl.bytes, "mask_regions: workspace too small (%lld < %lld bytes)", (long long)ws_bytes, (long long)pl.bytes);
  PSEG_REQUIRE(((uintptr_t)ws & 15) == 0, "mask_regions: workspace must be 16-byte aligned");
  const hipStream_t st = (hipStream_t)stream;
  char* w = (char*)ws;
  int* ridx = (int*)(w + pl.words);
  uint8_t* flag = (uint8_t*)(w + pl.bytes1);
  unsigned* bsum = (unsigned*)(w + pl.bsum);
  if (hipMemsetAsync(flag, 0, (size_t)npix_total, st) != hipSuccess) {
    set_error("mask_regions: hipMemsetAsync failed");
    return PSEG_ERR_HIP;
  }
  const dim3 pg = photo_grid(Hmax, Wmax, B);
  hipLaunchKernelGGL(region_flag_kernel, pg, dim3(kRegThreads), 0, st, labels, table, npix_total, Hmax, Wmax, flag);
  hipLaunchKernelGGL(region_scan_sums_kernel, dim3(pl.nb), dim3(kRegThreads), 0, st, flag, npix_total, bsum);
  hipLaunchKernelGGL(region_scan_blocks_kernel, dim3(1), dim3(kRegThreads), 0, st, bsum, (unsigned)pl.nb, count);
  hipLaunchKernelGGL(region_scan_write_kernel, dim3(pl.nb), dim3(kRegThreads), 0, st, flag, npix_total, bsum, max_regions, ridx,
                     records);
  if (max_regions > 0)
    hipLaunchKernelGGL(region_accumulate_kernel, pg, dim3(kRegThreads), 0, st, mask, labels, table, npix_total, Hmax, Wmax, ridx,
                       max_regions, records);
  PSEG_LAUNCH_CHECK();
  return PSEG_OK;
}

int pseg_mask_clean(const uint8_t* mask, const int* labels, const int64_t* table, int B, int64_t npix_total, int Hmax, int Wmax,
                    int64_t min_area, int largest_only, uint8_t* mask_out, uint8_t* rgb, const uint8_t* lut, void* ws,
                    int64_t ws_bytes, void* stream) {
  PSEG_REQUIRE(mask && labels && table && mask_out && ws, "mask_clean: null pointer");
  PSEG_REQUIRE((rgb == nullptr) == (lut == nullptr), "mask_clean: rgb and lut come together");
  if (int rc = reg_common("mask_clean", table, B, npix_total, Hmax, Wmax)) return rc;
  PSEG_REQUIRE(min_area >= 0, "mask_clean: min_area %lld is negative", (long long)min_area);
  PSEG_REQUIRE(!largest_only || B <= kRegMaxCleanBatch, "mask_clean: largest_only takes at most %d photos per call (got %d)",
               kRegMaxCleanBatch, B);
  const RegPlan pl = reg_plan(npix_total);
  PSEG_REQUIRE(ws_bytes >= pl.bytes, "mask_clean: workspace too small (%lld < %lld bytes)", (long long)ws_bytes, (long long)pl.bytes);
  PSEG_REQUIRE(((uintptr_t)ws & 15) == 0, "mask_clean: workspace must be 16-byte aligned");
  PSEG_REQUIRE(!largest_only || (int64_t)B <= npix_total, "mask_clean: %d photos in %lld pixels", B, (long long)npix_total);
  const hipStream_t st = (hipStream_t)stream;
  const dim3 pg = photo_grid(Hmax, Wmax, B);
  const int min_a = (int)(min_area > 0x7fffffffll ? 0x7fffffffll : min_area);      // areas are below 2^31
  if (min_a <= 1 && !largest_only) {
    hipLaunchKernelGGL(clean_write_kernel, pg, dim3(kRegThreads), 0, st, mask, labels, table, npix_total, Hmax, Wmax,
                       (const uint8_t*)nullptr, mask_out, rgb, lut);
    PSEG_LAUNCH_CHECK();
    return PSEG_OK;
  }
  char* w = (char*)ws;
  int* area = (int*)(w + pl.words);
  uint8_t* rcls = (uint8_t*)(w + pl.bytes1);
  u64* best = largest_only ? (u64*)(w + pl.best) : nullptr;
  hipLaunchKernelGGL(clean_init_kernel, pg, dim3(kRegThreads), 0, st, labels, table, npix_total, Hmax, Wmax, area);
  hipLaunchKernelGGL(clean_area_kernel, pg, dim3(kRegThreads), 0, st, labels, table, npix_total, Hmax, Wmax, area);
  if (largest_only) {
    if (hipMemsetAsync(best, 0, (size_t)B * 256 * 8, st) != hipSuccess) {
      set_error("mask_clean: hipMemsetAsync failed");
      return PSEG_ERR_HIP;
    }
    hipLaunchKernelGGL(clean_largest_kernel, pg, dim3(kRegThreads), 0, st, mask, labels, table, npix_total, Hmax, Wmax, area, best);
  }
  hipLaunchKernelGGL(clean_walk_kernel, pg, dim3(kRegThreads), 0, st, mask, labels, table, npix_total, Hmax, Wmax, min_a, area, best,
                     rcls);
  hipLaunchKernelGGL(clean_write_kernel, pg, dim3(kRegThreads), 0, st, mask, labels, table, npix_total, Hmax, Wmax,
                     (const uint8_t*)rcls, mask_out, rgb, lut);
  PSEG_LAUNCH_CHECK();
  return PSEG_OK;
}

}  // extern "C"
