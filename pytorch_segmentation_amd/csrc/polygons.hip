// Outlines of the connected regions of the inference masks on gfx950: every region's boundary as closed rings of lattice
// vertices (include/pseg_amd.h, "outlines of the regions").  The data layout is regions.hip's: a ragged batch of uint8 masks
// packed in one buffer under a device table of {pixel offset, H, W}, and the canonical int32 labels of pseg_mask_label.
// All arithmetic is integer, so every result is exact.  No thread ever walks along a ring:
//  1. cracks: one byte per pixel, bit s set iff side s borders another label or the photo's edge; an exclusive scan of the
//     bit counts along the packed buffer numbers the edges, so the compact edge list is in the order of the packed edge id
//     4 * (packed pixel) + s and "smallest id" is "smallest index" from here on.
//  2. edges: every edge writes its id, its photo, its successor's index and its successor's corner flag (an edge has one
//     predecessor, so each flag has one writer).
//  3. start edges: R rounds of pointer doubling over the closed rings, each round {min, next}[e] = {min(min[e],
//     min[next[e]]), next[next[e]]} between two buffers; the minimum runs over corner-edge indices.  After R rounds with
//     2^R >= the longest possible ring every edge knows its ring's start edge.
//  4. list ranking: every ring is opened in front of its start edge and R more rounds of doubling sum the corner flags from
//     each edge to the ring's end; the start edge then holds the ring's vertex count n and a corner edge's position among
//     the ring's vertices is n minus its own sum.
//  5. a scan of (start flag, n) over the edge list gives every ring its index and the offset of its first vertex, in the
//     order of the start edges; the start edges write the ring records, the corner edges scatter their tails.
// The number of launches is 11 + 2 R with R = ceil(log2(min(max_edges, 4 * Hmax * Wmax))).  Every kernel behind the first
// scan reads the device-side edge count E and leaves when E > max_edges; every index that comes out of the edge arrays is
// compared with E (<= max_edges) before it is used, so labels that are not pseg_mask_label's give wrong rings, never an
// access outside the buffers.
#include "common.h"

namespace pseg {

constexpr int kRingThreads = 256;
constexpr int kRingRun = 8;                          // pixels of a photo one thread of a photo-grid kernel takes
constexpr int kRingScanChunk = kRingThreads * 16;    // positions per block of the two scans
constexpr int kRingNone = 0x7fffffff;                // "no corner edge seen yet" of the minimum; larger than every index

__device__ __forceinline__ bool ring_ok(int64_t off, int64_t H, int64_t W, int64_t cap, int Hmax, int Wmax) {
  return off >= 0 && H >= 1 && W >= 1 && H <= Hmax && W <= Wmax && H * W <= cap && off <= cap - H * W;
}

// direction of travel along side s (N east, E south, S west, W north); the pixel is on the right hand, so "left" of s is
// the direction of side (s + 3) % 4
__device__ __forceinline__ int ring_dx(int s) { return s == 0 ? 1 : s == 2 ? -1 : 0; }
__device__ __forceinline__ int ring_dy(int s) { return s == 1 ? 1 : s == 3 ? -1 : 0; }

// ------------------------------------------------------------------ 1. cracks
__global__ __launch_bounds__(kRingThreads) void ring_cracks_kernel(const int* __restrict__ labels, const int64_t* __restrict__ table,
                                                                    int64_t cap, int Hmax, int Wmax, uint8_t* __restrict__ sides) {
  const int b = blockIdx.y;
  const int64_t off = table[3 * b], H64 = table[3 * b + 1], W64 = table[3 * b + 2];
  if (!ring_ok(off, H64, W64, cap, Hmax, Wmax)) return;        // bad record: nothing read or written
  const int H = (int)H64, W = (int)W64, n = H * W;
  const int* lab = labels + off;
  for (int64_t i = (int64_t)blockIdx.x * kRingThreads * kRingRun + threadIdx.x, k = 0; k < kRingRun && i < n; ++k, i += kRingThreads) {
    const int p = (int)i, y = p / W, x = p - y * W, l = lab[p];
    unsigned m = 0;
    if (y == 0 || lab[p - W] != l) m |= 1u;
    if (x == W - 1 || lab[p + 1] != l) m |= 2u;
    if (y == H - 1 || lab[p + W] != l) m |= 4u;
    if (x == 0 || lab[p - 1] != l) m |= 8u;
    if (m) sides[off + p] = (uint8_t)m;                         // the buffer was zeroed
  }
}

// exclusive scan of one value per thread over the block; sh: 4 words; total: the block's sum
__device__ __forceinline__ unsigned ring_block_excl_scan(unsigned v, unsigned* sh, unsigned& total) {
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

__device__ __forceinline__ unsigned ring_load_sides(const uint8_t* __restrict__ sides, int64_t q0, int64_t npix, unsigned f[16]) {
  unsigned s = 0;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    f[j] = (q0 + j < npix) ? (unsigned)__popc((unsigned)sides[q0 + j]) : 0u;
    s += f[j];
  }
  return s;
}

__global__ __launch_bounds__(kRingThreads) void ring_pixel_sums_kernel(const uint8_t* __restrict__ sides, int64_t npix,
                                                                        unsigned* __restrict__ bsum) {
  __shared__ unsigned sh[4];
  unsigned f[16], total;
  const unsigned s = ring_load_sides(sides, (int64_t)blockIdx.x * kRingScanChunk + threadIdx.x * 16, npix, f);
  ring_block_excl_scan(s, sh, total);
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// one block: in-place exclusive scan of the nb block sums; counts[0] = the number of edges, and when that is above the
// capacity counts[1] = counts[2] = -1: every later kernel then leaves at once
__global__ __launch_bounds__(kRingThreads) void ring_pixel_blocks_kernel(unsigned* __restrict__ bsum, unsigned nb, int64_t max_edges,
                                                                          int64_t* __restrict__ counts) {
  __shared__ unsigned sh[4];
  const unsigned chunk = (nb + kRingThreads - 1) / kRingThreads;
  const unsigned lo = min(nb, threadIdx.x * chunk), hi = min(nb, lo + chunk);
  unsigned s = 0;
  for (unsigned i = lo; i < hi; ++i) s += bsum[i];
  unsigned total;
  unsigned run = ring_block_excl_scan(s, sh, total);
  for (unsigned i = lo; i < hi; ++i) {
    const unsigned v = bsum[i];
    bsum[i] = run;
    run += v;
  }
  if (threadIdx.x == 0) {
    counts[0] = (int64_t)total;
    if ((int64_t)total > max_edges) counts[1] = counts[2] = -1;
  }
}

// base[q] = index of the first edge of packed pixel q
__global__ __launch_bounds__(kRingThreads) void ring_pixel_write_kernel(const uint8_t* __restrict__ sides, int64_t npix,
                                                                         const unsigned* __restrict__ bsum, int* __restrict__ base) {
  __shared__ unsigned sh[4];
  unsigned f[16], total;
  const int64_t q0 = (int64_t)blockIdx.x * kRingScanChunk + threadIdx.x * 16;
  const unsigned s = ring_load_sides(sides, q0, npix, f);
  unsigned run = bsum[blockIdx.x] + ring_block_excl_scan(s, sh, total);
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    if (q0 + j < npix) base[q0 + j] = (int)run;
    run += f[j];
  }
}

// ------------------------------------------------------------------ 2. edges
__global__ __launch_bounds__(kRingThreads) void ring_edges_kernel(const int* __restrict__ labels, const int64_t* __restrict__ table,
                                                                   int64_t cap, int Hmax, int Wmax, int conn8,
                                                                   const uint8_t* __restrict__ sides, const int* __restrict__ base,
                                                                   const int64_t* __restrict__ counts, int64_t max_edges,
                                                                   int* __restrict__ eid, int* __restrict__ ephoto,
                                                                   int* __restrict__ succ, uint8_t* __restrict__ corner) {
  const int64_t E64 = counts[0];
  if (E64 > max_edges) return;
  const int E = (int)E64;
  const int b = blockIdx.y;
  const int64_t off = table[3 * b], H64 = table[3 * b + 1], W64 = table[3 * b + 2];
  if (!ring_ok(off, H64, W64, cap, Hmax, Wmax)) return;
  const int H = (int)H64, W = (int)W64, n = H * W;
  const int* lab = labels + off;
  const uint8_t* sd = sides + off;
  const int* bs = base + off;
  for (int64_t i = (int64_t)blockIdx.x * kRingThreads * kRingRun + threadIdx.x, k = 0; k < kRingRun && i < n; ++k, i += kRingThreads) {
    const int p = (int)i;
    const unsigned m = sd[p];
    if (!m) continue;
    const int y = p / W, x = p - y * W, l = lab[p];
    int e = bs[p];
    for (int s = 0; s < 4; ++s) {
      if (!(m >> s & 1u)) continue;
      if ((unsigned)e >= (unsigned)E) break;                   // cannot happen with a consistent scan; checked all the same
      const int ax = x + ring_dx(s), ay = y + ring_dy(s);
      const int bx = ax + ring_dx((s + 3) & 3), by = ay + ring_dy((s + 3) & 3);
      const bool in_a = ax >= 0 && ax < W && ay >= 0 && ay < H && lab[ay * W + ax] == l;
      const bool in_b = bx >= 0 && bx < W && by >= 0 && by < H && lab[by * W + bx] == l;
      int np, ns;                                              // the successor: pixel of this photo, side
      if (in_b && (in_a || conn8)) np = by * W + bx, ns = (s + 3) & 3;      // left turn (with 8-connectivity also at a saddle)
      else if (in_a) np = ay * W + ax, ns = s;                              // straight on
      else np = p, ns = (s + 1) & 3;                                        // right turn
      int f = bs[np] + __popc((unsigned)sd[np] & ((1u << ns) - 1u));
      if ((unsigned)f >= (unsigned)E) f = e;                   // only with labels that are not mask_label's: stay inside
      eid[e] = (int)(4 * (off + p) + s);
      ephoto[e] = b;
      succ[e] = f;
      corner[f] = ns != s;                                     // f's only predecessor is e
      ++e;
    }
  }
}

// ------------------------------------------------------------------ 3. start edges
__global__ __launch_bounds__(kRingThreads) void ring_min_init_kernel(const int* __restrict__ succ, const uint8_t* __restrict__ corner,
                                                                      const int64_t* __restrict__ counts, int64_t max_edges,
                                                                      int2* __restrict__ a) {
  const int64_t E = counts[0];
  const int64_t e = (int64_t)blockIdx.x * kRingThreads + threadIdx.x;
  if (E > max_edges || e >= E) return;
  a[e] = make_int2(corner[e] ? (int)e : kRingNone, succ[e]);
}

// one round: the window of every edge doubles.  One coalesced load, one dependent 8-byte gather, one coalesced store.
__global__ __launch_bounds__(kRingThreads) void ring_min_round_kernel(const int2* __restrict__ a, int2* __restrict__ o,
                                                                       const int64_t* __restrict__ counts, int64_t max_edges) {
  const int64_t E = counts[0];
  const int64_t e = (int64_t)blockIdx.x * kRingThreads + threadIdx.x;
  if (E > max_edges || e >= E) return;
  const int2 v = a[e];
  const int2 u = a[(unsigned)v.y < (unsigned)E ? v.y : (int)e];      // ring_edges_kernel checked every successor; so does this
  o[e] = make_int2(min(v.x, u.x), u.y);
}

// ------------------------------------------------------------------ 4. list ranking
// start[e] = the ring's start edge; the list is opened in front of it: the edge whose successor is the start edge ends it
__global__ __launch_bounds__(kRingThreads) void ring_rank_init_kernel(const int2* __restrict__ mins, const int* __restrict__ succ,
                                                                       const uint8_t* __restrict__ corner,
                                                                       const int64_t* __restrict__ counts, int64_t max_edges,
                                                                       int* __restrict__ start, int2* __restrict__ o) {
  const int64_t E = counts[0];
  const int64_t e = (int64_t)blockIdx.x * kRingThreads + threadIdx.x;
  if (E > max_edges || e >= E) return;
  const int st = mins[e].x, f = succ[e];
  start[e] = st;
  o[e] = make_int2((int)corner[e], f == st ? -1 : f);
}

__global__ __launch_bounds__(kRingThreads) void ring_rank_round_kernel(const int2* __restrict__ a, int2* __restrict__ o,
                                                                        const int64_t* __restrict__ counts, int64_t max_edges) {
  const int64_t E = counts[0];
  const int64_t e = (int64_t)blockIdx.x * kRingThreads + threadIdx.x;
  if (E > max_edges || e >= E) return;
  int2 v = a[e];
  if ((unsigned)v.y < (unsigned)E) {                           // -1 ends the list
    const int2 u = a[v.y];
    v = make_int2(v.x + u.x, u.y);
  }
  o[e] = v;
}

// ------------------------------------------------------------------ 5. ring index, vertex offsets, scatter
// the two scanned values of the 16 edges of a thread: start flag and, at a start edge, the ring's vertex count
__device__ __forceinline__ void ring_load_starts(const int* __restrict__ start, const int2* __restrict__ rank, int64_t e0, int64_t E,
                                                 unsigned f[16], unsigned n[16], unsigned& sf, unsigned& sn) {
  sf = 0, sn = 0;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const bool is = e0 + j < E && (int64_t)start[e0 + j] == e0 + j;
    f[j] = is ? 1u : 0u;
    n[j] = is ? (unsigned)rank[e0 + j].x : 0u;
    sf += f[j];
    sn += n[j];
  }
}

__global__ __launch_bounds__(kRingThreads) void ring_edge_sums_kernel(const int* __restrict__ start, const int2* __restrict__ rank,
                                                                       const int64_t* __restrict__ counts, int64_t max_edges,
                                                                       uint2* __restrict__ bsum) {
  __shared__ unsigned sh[8];
  const int64_t E = counts[0];
  if (E > max_edges) return;
  unsigned f[16], n[16], sf, sn, tf, tn;
  ring_load_starts(start, rank, (int64_t)blockIdx.x * kRingScanChunk + threadIdx.x * 16, E, f, n, sf, sn);
  ring_block_excl_scan(sf, sh, tf);
  ring_block_excl_scan(sn, sh + 4, tn);
  if (threadIdx.x == 0) bsum[blockIdx.x] = make_uint2(tf, tn);
}

__global__ __launch_bounds__(kRingThreads) void ring_edge_blocks_kernel(uint2* __restrict__ bsum, unsigned nb, int64_t max_edges,
                                                                         int64_t* __restrict__ counts) {
  __shared__ unsigned sh[8];
  if (counts[0] > max_edges) return;
  const unsigned chunk = (nb + kRingThreads - 1) / kRingThreads;
  const unsigned lo = min(nb, threadIdx.x * chunk), hi = min(nb, lo + chunk);
  unsigned sf = 0, sn = 0, tf, tn;
  for (unsigned i = lo; i < hi; ++i) sf += bsum[i].x, sn += bsum[i].y;
  unsigned rf = ring_block_excl_scan(sf, sh, tf);
  unsigned rn = ring_block_excl_scan(sn, sh + 4, tn);
  for (unsigned i = lo; i < hi; ++i) {
    const uint2 v = bsum[i];
    bsum[i] = make_uint2(rf, rn);
    rf += v.x, rn += v.y;
  }
  if (threadIdx.x == 0) counts[1] = (int64_t)tf, counts[2] = (int64_t)tn;
}

// the start edges write their ring's record and leave the offset of its first vertex in voff[start edge]
__global__ __launch_bounds__(kRingThreads) void ring_edge_write_kernel(const uint8_t* __restrict__ mask, const int* __restrict__ labels,
                                                                        const int64_t* __restrict__ table, int B, int64_t cap,
                                                                        const int* __restrict__ start, const int2* __restrict__ rank,
                                                                        const int* __restrict__ eid, const int* __restrict__ ephoto,
                                                                        const uint2* __restrict__ bsum,
                                                                        const int64_t* __restrict__ counts, int64_t max_edges,
                                                                        int* __restrict__ voff, int64_t* __restrict__ rings) {
  __shared__ unsigned sh[8];
  const int64_t E = counts[0];
  if (E > max_edges) return;
  unsigned f[16], n[16], sf, sn, tf, tn;
  const int64_t e0 = (int64_t)blockIdx.x * kRingScanChunk + threadIdx.x * 16;
  ring_load_starts(start, rank, e0, E, f, n, sf, sn);
  const uint2 head = bsum[blockIdx.x];
  unsigned rf = head.x + ring_block_excl_scan(sf, sh, tf);
  unsigned rn = head.y + ring_block_excl_scan(sn, sh + 4, tn);
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    if (!f[j]) continue;
    const int64_t e = e0 + j;
    voff[e] = (int)rn;
    const int b = ephoto[e], id = eid[e];
    const int64_t q = id >> 2;
    if ((int64_t)rf < max_edges / 4 && b >= 0 && b < B && q >= 0 && q < cap) {
      const int64_t rel = (int64_t)id - 4 * table[3 * b];
      const int64_t label = labels[q];
      int64_t* r = rings + (int64_t)rf * PSEG_RING_WORDS;
      r[0] = (int64_t)b * 256 + mask[q];
      r[1] = label;
      r[2] = rel;
      r[3] = (int64_t)rn;
      r[4] = (int64_t)n[j];
      r[5] = rel != 4 * label;
    }
    rf += 1;
    rn += n[j];
  }
}

// every corner edge writes its tail where it stands among its ring's vertices
__global__ __launch_bounds__(kRingThreads) void ring_scatter_kernel(const int64_t* __restrict__ table, int B,
                                                                     const int* __restrict__ start, const int2* __restrict__ rank,
                                                                     const uint8_t* __restrict__ corner, const int* __restrict__ eid,
                                                                     const int* __restrict__ ephoto, const int* __restrict__ voff,
                                                                     const int64_t* __restrict__ counts, int64_t max_edges,
                                                                     int* __restrict__ vertices) {
  const int64_t E = counts[0];
  const int64_t e = (int64_t)blockIdx.x * kRingThreads + threadIdx.x;
  if (E > max_edges || e >= E || !corner[e]) return;
  const int st = start[e], b = ephoto[e];
  if ((unsigned)st >= (unsigned)E || b < 0 || b >= B) return;
  const int64_t pos = (int64_t)voff[st] + rank[st].x - rank[e].x;
  if (pos < 0 || pos >= max_edges) return;
  const int id = eid[e], s = id & 3;
  const int64_t p = (int64_t)(id >> 2) - table[3 * b], W = table[3 * b + 2];
  if (p < 0 || W < 1) return;
  const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
  vertices[2 * pos] = x + (s == 1 || s == 2);
  vertices[2 * pos + 1] = y + (s >= 2);
}

// ------------------------------------------------------------------ workspace
struct RingPlan {
  int64_t sides, base, psum, eid, ephoto, succ, start, voff, corner, buf0, buf1, esum, bytes;   // byte offsets
  int nbp, nbe, rounds;
};

static inline int64_t ring_up16(int64_t v) { return (v + 15) / 16 * 16; }

static RingPlan ring_plan(int64_t npix, int64_t max_edges) {
  RingPlan p;
  const int64_t m = max_edges > 0 ? max_edges : 1;
  p.nbp = (int)((npix + kRingScanChunk - 1) / kRingScanChunk);
  p.nbe = (int)((m + kRingScanChunk - 1) / kRingScanChunk);
  p.rounds = 0;
  p.sides = 0;
  p.base = p.sides + ring_up16(npix);
  p.psum = p.base + ring_up16(npix * 4);
  p.eid = p.psum + ring_up16((int64_t)(p.nbp + 1) * 4);
  p.ephoto = p.eid + ring_up16(m * 4);
  p.succ = p.ephoto + ring_up16(m * 4);
  p.start = p.succ + ring_up16(m * 4);
  p.voff = p.start + ring_up16(m * 4);
  p.corner = p.voff + ring_up16(m * 4);
  p.buf0 = p.corner + ring_up16(m);
  p.buf1 = p.buf0 + ring_up16(m * 8);
  p.esum = p.buf1 + ring_up16(m * 8);
  p.bytes = p.esum + ring_up16((int64_t)(p.nbe + 1) * 8);
  return p;
}

// rounds of doubling: the smallest R with 2^R >= the longest ring there can be
static int ring_rounds(int64_t max_edges, int Hmax, int Wmax) {
  int64_t longest = 4ll * Hmax * Wmax;
  if (max_edges < longest) longest = max_edges;
  int r = 0;
  while ((1ll << r) < longest) ++r;
  return r;
}

static inline bool ring_sizes_ok(int64_t npix_total, int64_t max_edges) {
  return npix_total >= 1 && npix_total < (1ll << 29) && max_edges >= 0 && max_edges <= 4 * npix_total;
}

}  // namespace pseg

using namespace pseg;

extern "C" {

int64_t pseg_mask_rings_workspace_bytes(int64_t npix_total, int64_t max_edges) {
  if (!ring_sizes_ok(npix_total, max_edges)) return -1;
  return ring_plan(npix_total, max_edges).bytes;
}

int pseg_mask_rings(const uint8_t* mask, const int* labels, const int64_t* table, int B, int64_t npix_total, int Hmax, int Wmax,
                    int connectivity, int64_t max_edges, int64_t* rings, int32_t* vertices, int64_t* counts, void* ws,
                    int64_t ws_bytes, void* stream) {
  PSEG_REQUIRE(mask && labels && table && counts && ws, "mask_rings: null pointer");
  PSEG_REQUIRE(B >= 1 && B <= 65535, "mask_rings: batch %d outside [1, 65535]", B);
  PSEG_REQUIRE(Hmax >= 1 && Wmax >= 1 && Hmax <= 65535 && Wmax <= 65535, "mask_rings: largest image %dx%d outside [1, 65535]", Hmax,
               Wmax);
  PSEG_REQUIRE((int64_t)Hmax * Wmax < (1ll << 31), "mask_rings: largest image %dx%d has 2^31 pixels or more (labels are int32)", Hmax,
               Wmax);
  PSEG_REQUIRE(npix_total >= 1 && npix_total < (1ll << 29), "mask_rings: npix_total %lld outside [1, 2^29): edge ids are int32",
               (long long)npix_total);
  PSEG_REQUIRE(connectivity == 4 || connectivity == 8, "mask_rings: connectivity %d is neither 4 nor 8", connectivity);
  PSEG_REQUIRE(max_edges >= 0 && max_edges <= 4 * npix_total, "mask_rings: max_edges %lld outside [0, 4 * npix_total]",
               (long long)max_edges);
  PSEG_REQUIRE(max_edges == 0 || (rings && vertices), "mask_rings: max_edges %lld needs the rings and vertices buffers",
               (long long)max_edges);
  const RingPlan pl = ring_plan(npix_total, max_edges);
  PSEG_REQUIRE(ws_bytes >= pl.bytes, "mask_rings: workspace too small (%lld < %lld bytes)", (long long)ws_bytes, (long long)pl.bytes);
  PSEG_REQUIRE(((uintptr_t)ws & 15) == 0, "mask_rings: workspace must be 16-byte aligned");
  const hipStream_t st = (hipStream_t)stream;
  char* w = (char*)ws;
  uint8_t* sides = (uint8_t*)(w + pl.sides);
  int* base = (int*)(w + pl.base);
  unsigned* psum = (unsigned*)(w + pl.psum);
  int* eid = (int*)(w + pl.eid);
  int* ephoto = (int*)(w + pl.ephoto);
  int* succ = (int*)(w + pl.succ);
  int* start = (int*)(w + pl.start);
  int* voff = (int*)(w + pl.voff);
  uint8_t* corner = (uint8_t*)(w + pl.corner);
  int2* buf[2] = {(int2*)(w + pl.buf0), (int2*)(w + pl.buf1)};
  uint2* esum = (uint2*)(w + pl.esum);
  if (hipMemsetAsync(sides, 0, (size_t)npix_total, st) != hipSuccess || hipMemsetAsync(counts + 1, 0, 16, st) != hipSuccess) {
    set_error("mask_rings: hipMemsetAsync failed");
    return PSEG_ERR_HIP;
  }
  const dim3 pg(cdiv((int64_t)Hmax * Wmax, kRingThreads * kRingRun), B), th(kRingThreads);
  hipLaunchKernelGGL(ring_cracks_kernel, pg, th, 0, st, labels, table, npix_total, Hmax, Wmax, sides);
  hipLaunchKernelGGL(ring_pixel_sums_kernel, dim3(pl.nbp), th, 0, st, (const uint8_t*)sides, npix_total, psum);
  hipLaunchKernelGGL(ring_pixel_blocks_kernel, dim3(1), th, 0, st, psum, (unsigned)pl.nbp, max_edges, counts);
  if (max_edges > 0) {
    const int R = ring_rounds(max_edges, Hmax, Wmax);
    const dim3 eg(cdiv(max_edges, kRingThreads));
    hipLaunchKernelGGL(ring_pixel_write_kernel, dim3(pl.nbp), th, 0, st, (const uint8_t*)sides, npix_total, (const unsigned*)psum, base);
    hipLaunchKernelGGL(ring_edges_kernel, pg, th, 0, st, labels, table, npix_total, Hmax, Wmax, (int)(connectivity == 8),
                       (const uint8_t*)sides, (const int*)base, (const int64_t*)counts, max_edges, eid, ephoto, succ, corner);
    int cur = 0;
    hipLaunchKernelGGL(ring_min_init_kernel, eg, th, 0, st, (const int*)succ, (const uint8_t*)corner, (const int64_t*)counts, max_edges,
                       buf[cur]);
    for (int r = 0; r < R; ++r, cur ^= 1)
      hipLaunchKernelGGL(ring_min_round_kernel, eg, th, 0, st, (const int2*)buf[cur], buf[cur ^ 1], (const int64_t*)counts, max_edges);
    hipLaunchKernelGGL(ring_rank_init_kernel, eg, th, 0, st, (const int2*)buf[cur], (const int*)succ, (const uint8_t*)corner,
                       (const int64_t*)counts, max_edges, start, buf[cur ^ 1]);
    cur ^= 1;
    for (int r = 0; r < R; ++r, cur ^= 1)
      hipLaunchKernelGGL(ring_rank_round_kernel, eg, th, 0, st, (const int2*)buf[cur], buf[cur ^ 1], (const int64_t*)counts, max_edges);
    const int2* rank = buf[cur];
    hipLaunchKernelGGL(ring_edge_sums_kernel, dim3(pl.nbe), th, 0, st, (const int*)start, rank, (const int64_t*)counts, max_edges, esum);
    hipLaunchKernelGGL(ring_edge_blocks_kernel, dim3(1), th, 0, st, esum, (unsigned)pl.nbe, max_edges, counts);
    hipLaunchKernelGGL(ring_edge_write_kernel, dim3(pl.nbe), th, 0, st, mask, labels, table, B, npix_total, (const int*)start, rank,
                       (const int*)eid, (const int*)ephoto, (const uint2*)esum, (const int64_t*)counts, max_edges, voff, rings);
    hipLaunchKernelGGL(ring_scatter_kernel, eg, th, 0, st, table, B, (const int*)start, rank, (const uint8_t*)corner, (const int*)eid,
                       (const int*)ephoto, (const int*)voff, (const int64_t*)counts, max_edges, vertices);
  }
  PSEG_LAUNCH_CHECK();
  return PSEG_OK;
}

}  // extern "C"
