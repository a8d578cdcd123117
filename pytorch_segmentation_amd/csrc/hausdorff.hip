// Surface-distance evaluation on gfx950: from a predicted and a target label map, per image and class, the record that the
// Hausdorff distance, its percentile (HD95), the average symmetric surface distance and the surface Dice are made of
// (pseg_hausdorff_stats).  The contract is in include/pseg_amd.h; the design is DESIGN.md section 5m.
//
// For class c of image b, P = (pred == c, target not void), G = (target == c); the border of a mask is the set of its pixels
// with an edge neighbour outside it (the outside of the image included).  A record needs, for every pixel of one border, the
// exact squared Euclidean distance to the nearest pixel of the other.  Integer arithmetic only; thirteen launches:
//  - a memset of the counters and the histogram, then hd_border_kernel: a lane per pixel reads its own and its four
//    neighbours' labels and writes, per map, the class whose border the pixel is on (int16, -1 for none); the border pixels
//    are counted per (map, image, class) through an LDS histogram and integer atomics.  Only a class with a border in BOTH
//    maps of an image is `active`: every later kernel leaves the other (image, class) pairs alone.
//  - hd_cols_kernel: a lane per (image, class, map, column) of the active pairs sweeps down and up its column and leaves the
//    distance along the column to the nearest border pixel (int16, kHdNone without one) in the pair's plane.
//  - hd_rows_kernel: Meijster's lower-envelope scan, one lane per row, a block (one wave) per tile of R rows.  The tile of
//    column distances is staged in LDS as 32-bit words, [x][r] (the lanes of a wave on consecutive banks); the lane's stack
//    of parabolas (site, its column distance) grows INSIDE its own row's words -- entry q is written at x = q <= the scan
//    position, where the distance has been read already -- and the breakpoint of an entry is recomputed from the entry below
//    it, so a row costs 4 W bytes of LDS and O(W) steps whatever the distances are.  The backward pass writes the squared
//    distance over the row; then the whole wave walks the tile, and where the OTHER map has a border pixel of the class it
//    stores the distance in val (one int per pixel and direction), and reduces the maximum, the count within the tolerance
//    (integer atomics) and the sum of the square roots (one double per block).
//  - four rounds of hd_hist_kernel / hd_pick_kernel: a segmented radix select, most significant byte first, of the k-th
//    smallest distance of every (image, class, direction) at once.  The histogram pass adds each value whose upper bytes match
//    its segment's prefix into the segment's 256 bins (lanes of a wave that hit the same bin are merged first); the pick pass,
//    a wave per segment, finds the bin that holds rank k, extends the prefix and zeroes the bins.  The last pick writes the
//    record and adds the segment's per-block doubles in a fixed order.
#include "loss_common.h"

#include <math.h>

namespace pseg {

constexpr int kHdMaxSide = 16384;         // H^2 + W^2 <= 2^29
constexpr int kHdMaxClasses = 1024;
constexpr int kHdNone = 32767;            // column distance of a column without a border pixel (a distance is <= 16383)
constexpr int kHdThreads = 256;
constexpr int kHdPix = 4096;              // pixels of one image per block of the per-pixel kernels
constexpr int kHdWave = 64;               // the row pass's block
constexpr int kHdRowWords = 8192;         // LDS words of a row-pass block with W <= 8192 (32 KiB); a wider row takes W words
constexpr int kHdBins = 256;
constexpr int kHdRounds = 4;

__device__ __forceinline__ bool hd_active(const int* __restrict__ cnt, int BC, int bc) { return cnt[bc] > 0 && cnt[BC + bc] > 0; }

// ------------------------------------------------------------------------------------------------ borders
// bl: [2][B][HW], map 0 the prediction, map 1 the target; cnt: [2][B * C]
__global__ __launch_bounds__(kHdThreads) void hd_border_kernel(const int64_t* __restrict__ pred, const int64_t* __restrict__ target,
                                                               int B, int H, int W, int C, int chunks,
                                                               int16_t* __restrict__ bl, int* __restrict__ cnt) {
  extern __shared__ int hd_cnt[];                        // [2][C]
  const int b = blockIdx.x / chunks, ch = blockIdx.x - b * chunks;
  for (int c = threadIdx.x; c < 2 * C; c += kHdThreads) hd_cnt[c] = 0;
  __syncthreads();
  const int HW = H * W;
  const int p0 = ch * kHdPix, p1 = min(HW, p0 + kHdPix);
  const size_t img = (size_t)b * HW;
  const int64_t* tg = target + img;
  const int64_t* pr = pred + img;
  int16_t* outP = bl + img;
  int16_t* outG = bl + (size_t)B * HW + img;
  for (int p = p0 + threadIdx.x; p < p1; p += kHdThreads) {
    const long long t = tg[p];
    int bP = -1, bG = -1;
    if (t >= 0 && t < C) {                               // a void target pixel is in no mask of either map
      const long long q = pr[p];
      const bool hasP = q >= 0 && q < C;
      const int y = p / W, x = p - y * W;
      bool inG = true, inP = true;                       // all four neighbours inside the mask
      const int nb[4] = {p - W, p + W, p - 1, p + 1};
      const bool inside[4] = {y > 0, y < H - 1, x > 0, x < W - 1};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (!inside[k]) {
          inG = inP = false;
        } else {
          const long long tn = tg[nb[k]];
          inG = inG && tn == t;
          if (hasP) inP = inP && tn >= 0 && tn < C && pr[nb[k]] == q;
        }
      }
      if (!inG) bG = (int)t;
      if (hasP && !inP) bP = (int)q;
    }
    outP[p] = (int16_t)bP;
    outG[p] = (int16_t)bG;
    if (bP >= 0) atomicAdd(&hd_cnt[bP], 1);
    if (bG >= 0) atomicAdd(&hd_cnt[C + bG], 1);
  }
  __syncthreads();
  const int BC = B * C;
  for (int c = threadIdx.x; c < 2 * C; c += kHdThreads)
    if (hd_cnt[c]) atomicAdd(&cnt[(c < C ? 0 : BC) + b * C + (c < C ? c : c - C)], hd_cnt[c]);
}

// ------------------------------------------------------------------------------------------------ columns
// plane: [B * C][2][HW]: plane 2 * bc + m holds the distances to the border of class c in map m of image b
__global__ __launch_bounds__(kHdThreads) void hd_cols_kernel(const int16_t* __restrict__ bl, const int* __restrict__ cnt, int B,
                                                             int H, int W, int C, long long total,
                                                             int16_t* __restrict__ plane) {
  const long long g = (long long)blockIdx.x * kHdThreads + threadIdx.x;      // (plane, column)
  if (g >= total) return;                                // (no barrier below)
  const int pl = (int)(g / W), x = (int)(g - (long long)pl * W);
  const int bc = pl >> 1, m = pl & 1;
  if (!hd_active(cnt, B * C, bc)) return;
  const int b = bc / C, c = bc - b * C;
  const size_t HW = (size_t)H * W;
  const int16_t* lab = bl + ((size_t)m * B + b) * HW + x;
  int16_t* out = plane + (size_t)pl * HW + x;
  int run = kHdNone;
#pragma unroll 4
  for (int y = 0; y < H; ++y) {
    run = lab[(size_t)y * W] == c ? 0 : (run == kHdNone ? kHdNone : run + 1);
    out[(size_t)y * W] = (int16_t)run;
  }
  run = kHdNone;
#pragma unroll 4
  for (int y = H - 1; y >= 0; --y) {
    run = lab[(size_t)y * W] == c ? 0 : (run == kHdNone ? kHdNone : run + 1);
    const int up = out[(size_t)y * W];
    out[(size_t)y * W] = (int16_t)min(up, run);
  }
}

// ------------------------------------------------------------------------------------------------ rows
// a stack entry: the site's x in the low half, its column distance in the high half
__device__ __forceinline__ int hd_entry(int x, int g) { return x | (g << 16); }
__device__ __forceinline__ int hd_site(int e) { return e & 0xffff; }
__device__ __forceinline__ int hd_dist(int e) { return e >> 16; }

// 1 + the last x at which the parabola of site i (below) is not above that of site u > i: where u takes over
__device__ __forceinline__ int hd_takeover(int i, int gi, int u, int gu) {
  return 1 + (int)((unsigned)(u * u - i * i + gu * gu - gi * gi) / (unsigned)(2 * (u - i)));
}

__device__ __forceinline__ int hd_takeover_of(const int* __restrict__ row, int R, int q) {     // of entry q >= 0
  if (q == 0) return 0;
  const int lo = row[(q - 1) * R], hi = row[q * R];
  return hd_takeover(hd_site(lo), hd_dist(lo), hd_site(hi), hd_dist(hi));
}

// block: rows [tile * R, + R) of plane blockIdx.x / tiles.  val: [2][B][HW]; mx, ct: [B * C][2]; part: one double per block
__global__ __launch_bounds__(kHdWave) void hd_rows_kernel(const int16_t* __restrict__ bl, const int* __restrict__ cnt,
                                                          const int16_t* __restrict__ plane, int B, int H, int W, int C, int R,
                                                          int tiles, int tol2, int* __restrict__ val, int* __restrict__ mx,
                                                          int* __restrict__ ct, double* __restrict__ part) {
  extern __shared__ int hd_tile[];                       // [W][R]
  const int pl = blockIdx.x / tiles, tile = blockIdx.x - pl * tiles;
  const int bc = pl >> 1, m = pl & 1;
  if (!hd_active(cnt, B * C, bc)) return;                // (the whole block)
  const int b = bc / C, c = bc - b * C;
  const int y0 = tile * R, nr = min(R, H - y0);
  const size_t HW = (size_t)H * W;
  const int16_t* src = plane + (size_t)pl * HW + (size_t)y0 * W;
  const int n = nr * W, tid = threadIdx.x;
  for (int i = tid; i < n; i += kHdWave) {
    const int r = i / W, x = i - r * W;
    hd_tile[x * R + r] = src[i];
  }
  __syncthreads();
  if (tid < nr) {
    int* row = hd_tile + tid;                            // word x of the row: row[x * R]
    int q = -1, st = 0, gt = 0, tt = 0;                  // the top entry: its site, distance and takeover point
    for (int u = 0; u < W; ++u) {
      const int gu = row[u * R];
      if (gu == kHdNone) continue;
      while (q >= 0 && (tt - st) * (tt - st) + gt * gt > (tt - u) * (tt - u) + gu * gu) {
        --q;
        if (q >= 0) {
          const int e = row[q * R];
          st = hd_site(e);
          gt = hd_dist(e);
          tt = hd_takeover_of(row, R, q);
        }
      }
      if (q < 0) {
        q = 0;
        st = u; gt = gu; tt = 0;
        row[0] = hd_entry(u, gu);
      } else {
        const int w = hd_takeover(st, gt, u, gu);
        if (w < W) {
          ++q;                                           // (q <= u: the word was read before)
          st = u; gt = gu; tt = w;
          row[q * R] = hd_entry(u, gu);
        }
      }
    }
    // an active plane has a border pixel, whose column is finite in every row: q >= 0.  Were it not, the row is left far.
    for (int u = W - 1; u >= 0; --u) {
      const int d = q < 0 ? (1 << 30) : (u - st) * (u - st) + gt * gt;
      const bool pop = q >= 0 && u == tt;
      int ns = 0, ng = 0, nt = 0;
      if (pop && q > 0) {                                // (entries below q lie at x < q <= u: not yet overwritten)
        const int e = row[(q - 1) * R];
        ns = hd_site(e);
        ng = hd_dist(e);
        nt = hd_takeover_of(row, R, q - 1);
      }
      row[u * R] = d;
      if (pop) {
        --q;
        st = ns; gt = ng; tt = nt;
      }
    }
  }
  __syncthreads();
  const int qm = 1 - m;                                  // the map whose border pixels ask; also the direction's index
  const size_t qoff = ((size_t)qm * B + b) * HW + (size_t)y0 * W;
  const int16_t* qlab = bl + qoff;
  int* vout = val + qoff;
  int lmax = 0, lct = 0;
  double lsum = 0.0;
  for (int i = tid; i < n; i += kHdWave) {
    if (qlab[i] != c) continue;
    const int r = i / W, x = i - r * W;
    const int d = hd_tile[x * R + r];
    vout[i] = d;
    lmax = max(lmax, d);
    lct += d <= tol2 ? 1 : 0;
    lsum += sqrt((double)d);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lmax = max(lmax, __shfl_xor(lmax, o, 64));
    lct += __shfl_xor(lct, o, 64);
  }
  lsum = wave_sum_d(lsum);
  if (tid == 0) {
    const int seg = bc * 2 + qm;
    if (lmax) atomicMax(&mx[seg], lmax);
    if (lct) atomicAdd(&ct[seg], lct);
    part[blockIdx.x] = lsum;
  }
}

// ------------------------------------------------------------------------------------------------ quantile
// block: chunk (blockIdx.x % chunks) of image b of direction qm.  hist: [B * C][2][256]; selp: [B * C][2]
__global__ __launch_bounds__(kHdThreads) void hd_hist_kernel(const int16_t* __restrict__ bl, const int* __restrict__ val,
                                                             const int* __restrict__ cnt, int B, int HW, int C, int chunks,
                                                             int round, const unsigned* __restrict__ selp,
                                                             int* __restrict__ hist) {
  const int ib = blockIdx.x / chunks, ch = blockIdx.x - ib * chunks;        // ib = qm * B + b
  const int qm = ib / B, b = ib - qm * B;
  const size_t off = (size_t)ib * HW;
  const int p0 = ch * kHdPix, p1 = min(HW, p0 + kHdPix);
  const int lane = threadIdx.x & 63;
  for (int base = p0; base < p1; base += kHdThreads) {   // (the same trip count in every lane)
    const int p = base + threadIdx.x;
    bool act = false;
    unsigned slot = 0;
    if (p < p1) {
      const int c = bl[off + p];
      if (c >= 0 && hd_active(cnt, B * C, b * C + c)) {
        const unsigned seg = (unsigned)(b * C + c) * 2 + qm;
        const unsigned v = (unsigned)val[off + p];
        act = round == 0 || (v >> (32 - 8 * round)) == selp[seg];
        slot = seg * kHdBins + ((v >> (24 - 8 * round)) & 255u);
      }
    }
    unsigned long long todo = __ballot(act);
    while (todo) {                                       // one atomic per distinct bin of the wave
      const int leader = __ffsll((long long)todo) - 1;
      const unsigned ls = __shfl(slot, leader, 64);
      const unsigned long long same = __ballot(act && slot == ls);
      if (lane == leader) atomicAdd(&hist[ls], __popcll(same));
      todo &= ~same;
    }
  }
}

// a wave per segment (image, class, direction): the bin of rank k; in the last round also the record
__global__ __launch_bounds__(kHdWave) void hd_pick_kernel(const int* __restrict__ cnt, int BC, int round, int permille,
                                                          int* __restrict__ hist, unsigned* __restrict__ selp,
                                                          int* __restrict__ selk, const int* __restrict__ mx,
                                                          const int* __restrict__ ct, const double* __restrict__ part,
                                                          int tiles, int64_t* __restrict__ stats, double* __restrict__ sums) {
  const int seg = blockIdx.x, bc = seg >> 1, qm = seg & 1, lane = threadIdx.x;
  const int n = cnt[qm * BC + bc];
  const bool last = round == kHdRounds - 1;
  if (!hd_active(cnt, BC, bc)) {
    if (last && lane == 0) {
      stats[(size_t)bc * 8 + qm] = n;
      stats[(size_t)bc * 8 + 2 + qm] = -1;
      stats[(size_t)bc * 8 + 4 + qm] = -1;
      stats[(size_t)bc * 8 + 6 + qm] = 0;
      sums[(size_t)bc * 2 + qm] = 0.0;
    }
    return;
  }
  const int k = round == 0 ? (int)(((long long)n * permille + 999) / 1000) : selk[seg];
  int* h = hist + (size_t)seg * kHdBins + lane * 4;
  const int4 v = *reinterpret_cast<const int4*>(h);
  *reinterpret_cast<int4*>(h) = make_int4(0, 0, 0, 0);   // the next round, or the next call's memset, finds zeros
  const int own = v.x + v.y + v.z + v.w;
  int inc = own;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  int before = inc - own;
  if (before < k && k <= inc) {                          // exactly one lane: 1 <= k <= the bins' total
    const int bins[4] = {v.x, v.y, v.z, v.w};
    int j = 0;
    while (j < 3 && before + bins[j] < k) before += bins[j++];
    const unsigned prefix = (round == 0 ? 0u : selp[seg] << 8) | (unsigned)(lane * 4 + j);
    selp[seg] = prefix;
    selk[seg] = k - before;
    if (last) stats[(size_t)bc * 8 + 4 + qm] = (int64_t)prefix;
  }
  if (last) {
    // the blocks of the plane that answered this direction: plane 2 * bc + (1 - qm)
    const double* mine = part + (size_t)(bc * 2 + 1 - qm) * tiles;
    double s = 0.0;
    for (int i = lane; i < tiles; i += kHdWave) s += mine[i];
    s = wave_sum_d(s);
    if (lane == 0) {
      stats[(size_t)bc * 8 + qm] = n;
      stats[(size_t)bc * 8 + 2 + qm] = mx[seg];
      stats[(size_t)bc * 8 + 6 + qm] = ct[seg];
      sums[(size_t)bc * 2 + qm] = s;
    }
  }
}

struct HdPlan {
  int HW, chunks, R, tiles;
  int64_t rows_blocks, col_lanes, zero_bytes;
  int64_t cnt, mx, ct, hist, selp, selk, bl, val, part, plane, bytes;      // byte offsets into the workspace
};

static bool hd_sizes_ok(int B, int C, int H, int W) {
  if (B < 1 || H < 1 || W < 1 || C < 1 || C > kHdMaxClasses || H > kHdMaxSide || W > kHdMaxSide) return false;
  if ((int64_t)B * C > ((1ll << 31) - 1) / 4 / ((int64_t)H * W)) return false;         // a map's planes: B * C * H * W * 2 bytes
  return (int64_t)B * C * 2 * kHdBins * 4 < (1ll << 31);                                // the histogram
}

static HdPlan hd_plan(int B, int C, int H, int W) {
  HdPlan p;
  p.HW = H * W;
  p.chunks = cdiv(p.HW, kHdPix);
  int R = 1;
  while (R < kHdWave && 2 * R * W <= kHdRowWords) R *= 2;                               // a power of two: R divides the banks
  p.R = R;
  p.tiles = cdiv(H, R);
  const int64_t BC = (int64_t)B * C;
  p.rows_blocks = 2 * BC * p.tiles;
  p.col_lanes = 2 * BC * W;
  int64_t o = 0;
  p.cnt = o;   o = align256(o + 2 * BC * 4);
  p.mx = o;    o = align256(o + 2 * BC * 4);
  p.ct = o;    o = align256(o + 2 * BC * 4);
  p.hist = o;  o = align256(o + 2 * BC * kHdBins * 4);
  p.zero_bytes = o;                                      // everything up to here is zeroed at the start of a call
  p.selp = o;  o = align256(o + 2 * BC * 4);
  p.selk = o;  o = align256(o + 2 * BC * 4);
  p.bl = o;    o = align256(o + 2 * (int64_t)B * p.HW * 2);
  p.val = o;   o = align256(o + 2 * (int64_t)B * p.HW * 4);
  p.part = o;  o = align256(o + p.rows_blocks * 8);
  p.plane = o; o = align256(o + 2 * BC * p.HW * 2);
  p.bytes = o;
  return p;
}

}  // namespace pseg

using namespace pseg;

extern "C" {

int64_t pseg_hausdorff_workspace_bytes(int B, int C, int H, int W) {
  if (!hd_sizes_ok(B, C, H, W)) return 0;
  return hd_plan(B, C, H, W).bytes;
}

int pseg_hausdorff_stats(const int64_t* pred, const int64_t* target, int B, int H, int W, int C, int permille, int tol,
                         int64_t* stats, double* sums, void* workspace, int64_t workspace_bytes, void* stream) {
  // (the sizes first: a call with made-up sizes and no memory behind it is told about the sizes)
  PSEG_REQUIRE(B >= 1 && H >= 1 && W >= 1, "pseg_hausdorff_stats: sizes B, H, W = %d, %d, %d must be >= 1", B, H, W);
  PSEG_REQUIRE(H <= kHdMaxSide && W <= kHdMaxSide, "pseg_hausdorff_stats: H, W = %d, %d above %d", H, W, kHdMaxSide);
  PSEG_REQUIRE(C >= 1 && C <= kHdMaxClasses, "pseg_hausdorff_stats: class count C = %d outside [1, %d]", C, kHdMaxClasses);
  PSEG_REQUIRE(hd_sizes_ok(B, C, H, W),
               "pseg_hausdorff_stats: a workspace buffer at or above 2 GiB is not supported (B=%d C=%d H=%d W=%d); split the batch",
               B, C, H, W);
  PSEG_REQUIRE(permille >= 1 && permille <= 1000, "pseg_hausdorff_stats: permille = %d outside [1, 1000]", permille);
  PSEG_REQUIRE(tol >= 0 && tol <= 255, "pseg_hausdorff_stats: tol = %d outside [0, 255]", tol);
  PSEG_REQUIRE(pred && target && stats && sums && workspace,
               "pseg_hausdorff_stats: null pointer (pred, target, stats, sums or workspace)");
  const HdPlan pl = hd_plan(B, C, H, W);
  PSEG_REQUIRE(workspace_bytes >= pl.bytes, "pseg_hausdorff_stats: workspace too small (%lld < %lld bytes)",
               (long long)workspace_bytes, (long long)pl.bytes);
  PSEG_REQUIRE(((uintptr_t)workspace & 15) == 0, "pseg_hausdorff_stats: workspace must be 16-byte aligned");
  const hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  int* cnt = (int*)(ws + pl.cnt);
  int* mx = (int*)(ws + pl.mx);
  int* ct = (int*)(ws + pl.ct);
  int* hist = (int*)(ws + pl.hist);
  unsigned* selp = (unsigned*)(ws + pl.selp);
  int* selk = (int*)(ws + pl.selk);
  int16_t* bl = (int16_t*)(ws + pl.bl);
  int* val = (int*)(ws + pl.val);
  double* part = (double*)(ws + pl.part);
  int16_t* plane = (int16_t*)(ws + pl.plane);
  const int BC = B * C;
  if (hipMemsetAsync(ws, 0, (size_t)pl.zero_bytes, st) != hipSuccess) {
    set_error("pseg_hausdorff_stats: hipMemsetAsync failed");
    return PSEG_ERR_HIP;
  }
  hipLaunchKernelGGL(hd_border_kernel, dim3((unsigned)(B * pl.chunks)), dim3(kHdThreads), (size_t)C * 8, st, pred, target, B, H,
                     W, C, pl.chunks, bl, cnt);
  PSEG_LAUNCH_CHECK();
  hipLaunchKernelGGL(hd_cols_kernel, dim3((unsigned)cdiv(pl.col_lanes, kHdThreads)), dim3(kHdThreads), 0, st,
                     (const int16_t*)bl, (const int*)cnt, B, H, W, C, (long long)pl.col_lanes, plane);
  PSEG_LAUNCH_CHECK();
  hipLaunchKernelGGL(hd_rows_kernel, dim3((unsigned)pl.rows_blocks), dim3(kHdWave), (size_t)pl.R * W * 4, st,
                     (const int16_t*)bl, (const int*)cnt, (const int16_t*)plane, B, H, W, C, pl.R, pl.tiles, tol * tol, val, mx,
                     ct, part);
  PSEG_LAUNCH_CHECK();
  for (int round = 0; round < kHdRounds; ++round) {
    hipLaunchKernelGGL(hd_hist_kernel, dim3((unsigned)(2 * B * pl.chunks)), dim3(kHdThreads), 0, st, (const int16_t*)bl,
                       (const int*)val, (const int*)cnt, B, pl.HW, C, pl.chunks, round, (const unsigned*)selp, hist);
    PSEG_LAUNCH_CHECK();
    hipLaunchKernelGGL(hd_pick_kernel, dim3((unsigned)(2 * BC)), dim3(kHdWave), 0, st, (const int*)cnt, BC, round, permille,
                       hist, selp, selk, (const int*)mx, (const int*)ct, (const double*)part, pl.tiles, stats, sums);
    PSEG_LAUNCH_CHECK();
  }
  return PSEG_OK;
}

}  // extern "C"
