// Multi-class Lovasz-softmax loss (Berman et al., CVPR 2018; classes = 'present', one batch-wide set of pixels) with its
// gradient with respect to the logits, on gfx950.  The contract is in include/pseg_amd.h (pseg_lovasz_softmax_fwd_bwd).
//
// Per present class c the errors e_i = |[t_i == c] - softmax_c(logits_i)| of all pixels are sorted descending (ties by
// ascending pixel index) and weighted by the discrete differences of the Jaccard loss along that order.  Stages, all
// on the caller's stream, nothing read back by the host:
//   0. lovasz_hist_kernel / lovasz_present_kernel: per-class foreground histogram, n_valid, n_bad, n_present.
//   1. lovasz_errors_kernel: softmax + errors; one 32-bit key word per (class, pixel).  A key is
//      0x3F800000 - bits(e) (e in [0, 1], so non-negative floats order as unsigned integers and ASCENDING keys are
//      DESCENDING errors); bit 31 carries the foreground flag and is never a sort digit.  Pixels that do not count get
//      the key 0x3F800001, behind every valid one, so the valid pixels of a class are a prefix of its sorted segment.
//   2. a stable LSD radix sort of (key, pixel index), 8-bit digits over the 30 key bits (4 passes), one segment per
//      present class: lovasz_sort_hist_kernel (per-tile digit counts, LDS atomics) -> lovasz_scan_rows_kernel (per digit
//      over the tiles) -> lovasz_sort_scatter_kernel (ranks by wave64 ballots in element order, hence stable).  The
//      first pass synthesises the pixel index from the position, which is also what makes ties end up index-ascending.
//   3. lovasz_fg_count_kernel -> lovasz_scan_rows_kernel -> lovasz_grad_kernel: inclusive foreground count F_k along the
//      sorted order (ballot + popcount), the closed-form differences from the INTEGER counts
//          I_k = P - F_k, U_k = P + (k + 1 - F_k);   foreground: 1 / U_k;   background: I_k / ((U_k - 1) * U_k)
//      (never a difference of two values near 1), the per-tile dot product in double, and dL/dp scattered to the pixel's
//      slot of dlogits, which serves as the scratch for it.
//   4. lovasz_softmax_bwd_kernel: softmax Jacobian in place on dlogits.
// Classes are processed in groups so that the sort buffers (16 bytes per class and pixel) stay inside kLvSortBudget.
// Absent classes cost an early exit per block: every kernel of stages 1-3 reads the device histogram.
// Sums of floats are taken in a fixed order (per thread, xor-shuffle tree, waves in order, tiles in order); atomics add
// integers only, so two calls give identical bits.
#include "loss_common.h"

#include <math.h>
#include <stdlib.h>

namespace pseg {

constexpr int kLvThreads = 256;
constexpr int kLvItems = 16;                        // keys per thread and tile
constexpr int kLvTile = kLvThreads * kLvItems;      // 4096 keys per block
constexpr int kLvWaveSpan = 64 * kLvItems;          // consecutive keys one wave ranks
constexpr int kLvMaxClasses = 1024;                 // bins of the LDS label histogram
constexpr unsigned kLvKeyOne = 0x3F800000u;         // bits(1.0f): key of e is kLvKeyOne - bits(e)
constexpr unsigned kLvKeyInvalid = 0x3F800001u;     // ignored / out-of-range pixels, behind every valid key
constexpr unsigned kLvFg = 0x80000000u;             // foreground flag of a key word
constexpr int kLvPasses = 4;                        // 8-bit digits over key bits 0..29
constexpr int64_t kLvSortBudget = 512ll << 20;      // bytes of sort buffers one class group may take
constexpr int kLvMaxBlocks = 4096;
static_assert(kLvThreads == 256, "capped_blocks (loss_common.h) counts blocks of 256 threads");

struct LvHeader {
  int n_valid, n_bad, n_present, pad;
  int hist[kLvMaxClasses];      // foreground pixels per class
};

__device__ __forceinline__ unsigned lv_digit(unsigned kw, int shift) { return ((kw & ~kLvFg) >> shift) & 0xFFu; }

// exclusive scan over the 256 threads of a block (sh: 4 words, not reused by the caller before its next barrier)
__device__ __forceinline__ unsigned lv_block_excl_scan(unsigned v, unsigned* sh, unsigned& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  unsigned inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned u = __shfl_up(inc, o, 64);
    if (lane >= o) inc += u;
  }
  if (lane == 63) sh[w] = inc;
  __syncthreads();
  unsigned off = 0;
#pragma unroll
  for (int i = 0; i < 3; ++i) off += (i < w) ? sh[i] : 0u;
  total = sh[0] + sh[1] + sh[2] + sh[3];
  return off + inc - v;
}

// ------------------------------------------------------------------------------------------------ stage 0
__global__ __launch_bounds__(kLvThreads) void lovasz_hist_kernel(const int64_t* __restrict__ target, unsigned npix,
                                                                 long long ignore_index, int C, LvHeader* __restrict__ hdr) {
  __shared__ int bins[kLvMaxClasses];
  __shared__ int sh[2][4];
  for (int i = threadIdx.x; i < C; i += kLvThreads) bins[i] = 0;
  __syncthreads();
  int cnt = 0, bad = 0;
  for (unsigned i = blockIdx.x * kLvThreads + threadIdx.x; i < npix; i += gridDim.x * kLvThreads) {
    const long long t = target[i];
    if (ce_valid(t, ignore_index, C)) {
      atomicAdd(&bins[(int)t], 1);
      ++cnt;
    } else if (t != ignore_index) {
      ++bad;
    }
  }
  block_count(cnt, bad, &hdr->n_valid, &hdr->n_bad, sh);
  for (int i = threadIdx.x; i < C; i += kLvThreads)
    if (bins[i]) atomicAdd(&hdr->hist[i], bins[i]);
}

__global__ __launch_bounds__(kLvThreads) void lovasz_present_kernel(int C, LvHeader* __restrict__ hdr) {
  __shared__ unsigned sh[4];
  unsigned n = 0;
  for (int i = threadIdx.x; i < C; i += kLvThreads) n += hdr->hist[i] > 0 ? 1u : 0u;
  unsigned total;
  lv_block_excl_scan(n, sh, total);
  if (threadIdx.x == 0) hdr->n_present = (int)total;
}

// ------------------------------------------------------------------------------------------------ stage 1
// max and sum of exp of one pixel's logits (class stride HW); the correctly rounded expf and a true division keep each
// probability within a few 1e-8 of the exact one, which is what bounds the loss error (see the header's contract)
__device__ __forceinline__ void lv_softmax_stats(const float* __restrict__ lp, int C, size_t HW, float& m, float& s) {
  m = lp[0];
  for (int c = 1; c < C; ++c) m = fmaxf(m, lp[c * HW]);
  s = 0.f;
  for (int c = 0; c < C; ++c) s += expf(lp[c * HW] - m);
}

__global__ __launch_bounds__(kLvThreads) void lovasz_errors_kernel(const float* __restrict__ logits,
                                                                   const int64_t* __restrict__ target, int C, unsigned HW,
                                                                   unsigned npix, long long ignore_index,
                                                                   const LvHeader* __restrict__ hdr, int c0, int G, size_t S,
                                                                   unsigned* __restrict__ keys) {
  for (unsigned g = blockIdx.x * kLvThreads + threadIdx.x; g < npix; g += gridDim.x * kLvThreads) {
    const unsigned b = g / HW;
    const unsigned p = g - b * HW;
    const float* lp = logits + (size_t)b * C * HW + p;
    const long long t = target[g];
    const bool valid = ce_valid(t, ignore_index, C);
    float m = 0.f, s = 1.f;
    if (valid) lv_softmax_stats(lp, C, HW, m, s);
    for (int k = 0; k < G; ++k) {
      const int c = c0 + k;
      if (hdr->hist[c] == 0) continue;     // absent class: its segment is never read
      unsigned kw = kLvKeyInvalid;
      if (valid) {
        const float pr = expf(lp[(size_t)c * HW] - m) / s;
        const bool fg = (t == c);
        const float e = fminf(fmaxf(fg ? 1.f - pr : pr, 0.f), 1.f);
        kw = (kLvKeyOne - __builtin_bit_cast(unsigned, e)) | (fg ? kLvFg : 0u);
      }
      keys[(size_t)k * S + g] = kw;
    }
  }
}

// ------------------------------------------------------------------------------------------------ stage 2
// digit counts of one tile of one segment -> blockhist[segment][digit][tile]
__global__ __launch_bounds__(kLvThreads) void lovasz_sort_hist_kernel(const unsigned* __restrict__ keys, unsigned npix, size_t S,
                                                                      int shift, const LvHeader* __restrict__ hdr, int c0,
                                                                      unsigned nb, unsigned* __restrict__ blockhist) {
  if (hdr->hist[c0 + blockIdx.y] == 0) return;
  __shared__ unsigned h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const unsigned* k = keys + (size_t)blockIdx.y * S;      // S % 4 == 0 and the base is 256-byte aligned: 16-byte loads
  const unsigned base = blockIdx.x * kLvTile;
  if (base + kLvTile <= npix) {
#pragma unroll
    for (int j = 0; j < kLvItems / 4; ++j) {
      const uint4 v = *reinterpret_cast<const uint4*>(k + base + (j * kLvThreads + threadIdx.x) * 4);
      atomicAdd(&h[lv_digit(v.x, shift)], 1u);
      atomicAdd(&h[lv_digit(v.y, shift)], 1u);
      atomicAdd(&h[lv_digit(v.z, shift)], 1u);
      atomicAdd(&h[lv_digit(v.w, shift)], 1u);
    }
  } else {
    for (int j = 0; j < kLvItems; ++j) {
      const unsigned i = base + j * kLvThreads + threadIdx.x;
      if (i < npix) atomicAdd(&h[lv_digit(k[i], shift)], 1u);
    }
  }
  __syncthreads();
  blockhist[((size_t)blockIdx.y * 256 + threadIdx.x) * nb + blockIdx.x] = h[threadIdx.x];
}

// In-place exclusive scan of rows of `len` words: grid (rows per segment, segments); totals (nullable) gets each row's sum.
__global__ __launch_bounds__(kLvThreads) void lovasz_scan_rows_kernel(unsigned* __restrict__ data, unsigned len,
                                                                      unsigned* __restrict__ totals,
                                                                      const LvHeader* __restrict__ hdr, int c0) {
  if (hdr->hist[c0 + blockIdx.y] == 0) return;
  __shared__ unsigned sh[4];
  const size_t row = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
  unsigned* d = data + row * len;
  const unsigned chunk = (len + kLvThreads - 1) / kLvThreads;
  const unsigned lo = min(len, threadIdx.x * chunk), hi = min(len, lo + chunk);
  unsigned s = 0;
  for (unsigned i = lo; i < hi; ++i) s += d[i];
  unsigned total;
  unsigned run = lv_block_excl_scan(s, sh, total);
  for (unsigned i = lo; i < hi; ++i) {
    const unsigned v = d[i];
    d[i] = run;
    run += v;
  }
  if (totals && threadIdx.x == 0) totals[row] = total;
}

// Stable scatter of one tile.  Wave w ranks the kLvWaveSpan consecutive elements [w * 1024, (w + 1) * 1024) of the tile in
// 16 rounds of 64: lanes with the same digit find each other with 8 ballots, the lowest of them takes the group's slots
// from the wave's own counter (an LDS atomic nobody else touches), and a lane's slot is that base plus the number of
// lower lanes in its group.  Rounds, lanes and waves are visited in element order, so equal digits keep their order.
template <bool FIRST>
__global__ __launch_bounds__(kLvThreads) void lovasz_sort_scatter_kernel(const unsigned* __restrict__ keys_in,
                                                                         const unsigned* __restrict__ idx_in,
                                                                         unsigned* __restrict__ keys_out,
                                                                         unsigned* __restrict__ idx_out, unsigned npix, size_t S,
                                                                         int shift, const LvHeader* __restrict__ hdr, int c0,
                                                                         unsigned nb, const unsigned* __restrict__ blockhist,
                                                                         const unsigned* __restrict__ totals) {
  if (hdr->hist[c0 + blockIdx.y] == 0) return;
  __shared__ unsigned wcnt[4][256];
  __shared__ unsigned sh[4];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
#pragma unroll
  for (int i = 0; i < 4; ++i) wcnt[i][t] = 0;
  // first slot of digit t for this tile: digits below it in the whole segment + the same digit in earlier tiles
  unsigned total;
  unsigned dbase = lv_block_excl_scan(totals[(size_t)blockIdx.y * 256 + t], sh, total);      // (barrier inside)
  dbase += blockhist[((size_t)blockIdx.y * 256 + t) * nb + blockIdx.x];
  const unsigned* kin = keys_in + (size_t)blockIdx.y * S;
  const unsigned* iin = idx_in + (size_t)blockIdx.y * S;
  unsigned* kout = keys_out + (size_t)blockIdx.y * S;
  unsigned* iout = idx_out + (size_t)blockIdx.y * S;
  const unsigned base = blockIdx.x * kLvTile + w * kLvWaveSpan + lane;
  const unsigned long long lt = (1ull << lane) - 1ull;
  unsigned kw[kLvItems], id[kLvItems], slot[kLvItems];
#pragma unroll
  for (int j = 0; j < kLvItems; ++j) {
    const unsigned i = base + j * 64;
    const bool in = i < npix;
    kw[j] = in ? kin[i] : 0u;
    id[j] = FIRST ? i : (in ? iin[i] : 0u);
  }
#pragma unroll
  for (int j = 0; j < kLvItems; ++j) {
    const bool in = base + j * 64 < npix;
    const unsigned d = lv_digit(kw[j], shift);
    unsigned long long peers = __ballot(in);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const unsigned long long bal = __ballot(in && bit);
      peers &= bit ? bal : ~bal;
    }
    const unsigned rank = __popcll(peers & lt);
    unsigned first = 0;
    if (in && rank == 0) first = atomicAdd(&wcnt[w][d], (unsigned)__popcll(peers));
    const int leader = in ? __ffsll((long long)peers) - 1 : lane;
    slot[j] = __shfl(first, leader, 64) + rank;
  }
  __syncthreads();
  {
    const unsigned n0 = wcnt[0][t], n1 = wcnt[1][t], n2 = wcnt[2][t];
    wcnt[0][t] = dbase;
    wcnt[1][t] = dbase + n0;
    wcnt[2][t] = dbase + n0 + n1;
    wcnt[3][t] = dbase + n0 + n1 + n2;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kLvItems; ++j) {
    if (base + j * 64 < npix) {
      const unsigned p = wcnt[w][lv_digit(kw[j], shift)] + slot[j];
      if (p < npix) {       // always true for consistent counts; a store outside the segment must not exist
        kout[p] = kw[j];
        iout[p] = id[j];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ stage 3
__global__ __launch_bounds__(kLvThreads) void lovasz_fg_count_kernel(const unsigned* __restrict__ keys, unsigned npix, size_t S,
                                                                     const LvHeader* __restrict__ hdr, int c0, unsigned nb,
                                                                     unsigned* __restrict__ tilecnt) {
  if (hdr->hist[c0 + blockIdx.y] == 0) return;
  __shared__ unsigned sh[4];
  const unsigned* k = keys + (size_t)blockIdx.y * S;
  const unsigned base = blockIdx.x * kLvTile;
  unsigned n = 0;
  for (int j = 0; j < kLvItems; ++j) {
    const unsigned i = base + j * kLvThreads + threadIdx.x;
    if (i < npix) n += k[i] >> 31;
  }
  unsigned total;
  lv_block_excl_scan(n, sh, total);
  if (threadIdx.x == 0) tilecnt[(size_t)blockIdx.y * nb + blockIdx.x] = total;
}

// Sorted segment -> differences of the Jaccard loss, the tile's share of loss_c (double), dL/dp into the pixel's slot.
__global__ __launch_bounds__(kLvThreads) void lovasz_grad_kernel(const unsigned* __restrict__ keys, const unsigned* __restrict__ idx,
                                                                 unsigned npix, size_t S, unsigned HW, int C,
                                                                 const LvHeader* __restrict__ hdr, int c0, unsigned nb,
                                                                 const unsigned* __restrict__ tile_excl,
                                                                 double* __restrict__ partial, float* __restrict__ dlogits) {
  const int c = c0 + blockIdx.y;
  const long long P = hdr->hist[c];
  if (P == 0) return;
  __shared__ unsigned tot[64];
  __shared__ double shd[4];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const unsigned* k = keys + (size_t)blockIdx.y * S;
  const unsigned* ix = idx + (size_t)blockIdx.y * S;
  const unsigned base = blockIdx.x * kLvTile + w * kLvWaveSpan + lane;
  const unsigned long long lt = (1ull << lane) - 1ull;
  unsigned kw[kLvItems];
#pragma unroll
  for (int j = 0; j < kLvItems; ++j) {
    const unsigned i = base + j * 64;
    kw[j] = i < npix ? k[i] : kLvKeyInvalid;
    const unsigned long long bal = __ballot((kw[j] >> 31) != 0);
    if (lane == 0) tot[w * kLvItems + j] = (unsigned)__popcll(bal);
  }
  __syncthreads();
  if (w == 0) {      // exclusive scan of the 64 (wave, round) totals, which are in element order
    const unsigned v = tot[lane];
    unsigned inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned u = __shfl_up(inc, o, 64);
      if (lane >= o) inc += u;
    }
    tot[lane] = inc - v;
  }
  __syncthreads();
  const long long F0 = tile_excl[(size_t)blockIdx.y * nb + blockIdx.x];
  const int np = hdr->n_present;
  const double inv_np = np > 0 ? 1.0 / (double)np : 0.0;
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < kLvItems; ++j) {
    const unsigned i = base + j * 64;
    const bool fg = (kw[j] >> 31) != 0;
    const unsigned K = kw[j] & ~kLvFg;
    const unsigned long long bal = __ballot(fg);
    // valid keys are a prefix of the sorted segment, so the position is the rank among valid pixels
    if (K <= kLvKeyOne) {
      const long long F = F0 + tot[w * kLvItems + j] + __popcll(bal & lt) + (fg ? 1 : 0);      // foreground in [0, k]
      const long long U = P + ((long long)i + 1 - F);
      const long long I = P - F;
      const double d = fg ? 1.0 / (double)U : (double)I / ((double)(U - 1) * (double)U);
      acc += (double)__builtin_bit_cast(float, kLvKeyOne - K) * d;
      if (dlogits) {
        const unsigned id = ix[i];
        if (id < npix) {
          const unsigned b = id / HW;
          const unsigned p = id - b * HW;
          dlogits[((size_t)b * C + c) * HW + p] = (float)((fg ? -d : d) * inv_np);
        }
      }
    }
  }
  acc = block_sum_d(acc, shd);
  if (t == 0) partial[(size_t)c * nb + blockIdx.x] = acc;
}

__global__ __launch_bounds__(kLvThreads) void lovasz_finish_kernel(const double* __restrict__ partial, int C, unsigned nb,
                                                                   const LvHeader* __restrict__ hdr, float* __restrict__ out) {
  __shared__ double shd[4];
  double s = 0.0;
  for (int c = 0; c < C; ++c) {
    if (hdr->hist[c] == 0) continue;
    for (unsigned i = threadIdx.x; i < nb; i += kLvThreads) s += partial[(size_t)c * nb + i];
  }
  s = block_sum_d(s, shd);
  if (threadIdx.x == 0) {
    const int np = hdr->n_present;
    out[0] = np > 0 ? (float)(s / (double)np) : 0.f;
    out[1] = (float)hdr->n_valid;
    out[2] = (float)hdr->n_bad;
    out[3] = (float)np;
  }
}

// ------------------------------------------------------------------------------------------------ stage 4
// dlogits holds g_c = dL/dp_c of the present classes at valid pixels (anything elsewhere); dz_j = p_j * (g_j - sum_c g_c p_c)
__global__ __launch_bounds__(kLvThreads) void lovasz_softmax_bwd_kernel(const float* __restrict__ logits,
                                                                        const int64_t* __restrict__ target, int C, unsigned HW,
                                                                        unsigned npix, long long ignore_index,
                                                                        const LvHeader* __restrict__ hdr,
                                                                        float* __restrict__ dlogits) {
  for (unsigned g = blockIdx.x * kLvThreads + threadIdx.x; g < npix; g += gridDim.x * kLvThreads) {
    const unsigned b = g / HW;
    const unsigned p = g - b * HW;
    const float* lp = logits + (size_t)b * C * HW + p;
    float* dp = dlogits + (size_t)b * C * HW + p;
    if (!ce_valid(target[g], ignore_index, C)) {
      for (int c = 0; c < C; ++c) dp[(size_t)c * HW] = 0.f;
      continue;
    }
    float m, s;
    lv_softmax_stats(lp, C, HW, m, s);
    float dot = 0.f;
    for (int c = 0; c < C; ++c)
      if (hdr->hist[c] > 0) dot += dp[(size_t)c * HW] * (expf(lp[(size_t)c * HW] - m) / s);
    for (int c = 0; c < C; ++c) {
      const float pr = expf(lp[(size_t)c * HW] - m) / s;
      const float gc = hdr->hist[c] > 0 ? dp[(size_t)c * HW] : 0.f;
      dp[(size_t)c * HW] = pr * (gc - dot);
    }
  }
}

// ------------------------------------------------------------------------------------------------ host
struct LvPlan {
  unsigned nb;        // tiles per segment
  int G;              // classes per group
  size_t S;           // words per segment (pixels rounded up to 4: 16-byte aligned segments)
  int64_t totals, blockhist, tilecnt, partial, keys[2], idx[2], bytes;   // byte offsets into the workspace
};

static LvPlan lv_plan(int64_t npix, int C) {
  LvPlan p;
  p.nb = (unsigned)((npix + kLvTile - 1) / kLvTile);
  p.S = (size_t)((npix + 3) / 4 * 4);
  const int64_t gmax = kLvSortBudget / (16 * (int64_t)p.S) > 0 ? kLvSortBudget / (16 * (int64_t)p.S) : 1;
  const int64_t ngroups = (C + gmax - 1) / gmax;
  p.G = (int)((C + ngroups - 1) / ngroups);
  int64_t o = align256(sizeof(LvHeader));
  p.totals = o;    o = align256(o + (int64_t)p.G * 256 * 4);
  p.blockhist = o; o = align256(o + (int64_t)p.G * 256 * p.nb * 4);
  p.tilecnt = o;   o = align256(o + (int64_t)p.G * p.nb * 4);
  p.partial = o;   o = align256(o + (int64_t)C * p.nb * 8);
  for (int i = 0; i < 2; ++i) {
    p.keys[i] = o; o = align256(o + (int64_t)p.G * p.S * 4);
    p.idx[i] = o;  o = align256(o + (int64_t)p.G * p.S * 4);
  }
  p.bytes = o;
  return p;
}

static bool lv_sizes_ok(int B, int C, int64_t HW) {
  if (B <= 0 || C <= 0 || HW <= 0 || C > kLvMaxClasses) return false;
  if (HW > (1ll << 31) / 8 / B) return false;                            // targets: B * HW * 8 bytes
  return (int64_t)B * HW * C * 4 < (1ll << 31) && (int64_t)B * HW * 8 < (1ll << 31);
}

// PSEG_LOVASZ_GROUP=n: at most n classes per group (never more than the plan's, so the workspace size does not change);
// read per call, so that a test can take the multi-group path at a small shape
static int lv_group_override(int G) {
  const char* e = getenv("PSEG_LOVASZ_GROUP");
  const int v = e ? atoi(e) : 0;
  return (v > 0 && v < G) ? v : G;
}

}  // namespace pseg

using namespace pseg;

extern "C" {

int64_t pseg_lovasz_workspace_bytes(int B, int C, int64_t HW) {
  if (!lv_sizes_ok(B, C, HW)) return 0;
  return lv_plan((int64_t)B * HW, C).bytes;
}

int pseg_lovasz_softmax_fwd_bwd(const float* logits, const int64_t* target, int B, int C, int64_t HW, int64_t ignore_index,
                                float* dlogits, float* out, void* workspace, int64_t workspace_bytes, void* stream) {
  PSEG_REQUIRE(logits && target && out && workspace, "lovasz: null pointer");
  PSEG_REQUIRE(B > 0 && C > 0 && HW > 0, "lovasz: bad sizes");
  PSEG_REQUIRE(C <= kLvMaxClasses, "lovasz: at most %d classes (got %d)", kLvMaxClasses, C);
  PSEG_REQUIRE(lv_sizes_ok(B, C, HW),
               "lovasz: logits or targets above 2 GiB are not supported (B=%d C=%d HW=%lld); split the batch", B, C,
               (long long)HW);
  const int64_t npix64 = (int64_t)B * HW;
  const LvPlan pl = lv_plan(npix64, C);
  PSEG_REQUIRE(workspace_bytes >= pl.bytes, "lovasz: workspace too small (%lld < %lld bytes)", (long long)workspace_bytes,
               (long long)pl.bytes);
  PSEG_REQUIRE(((uintptr_t)workspace & 15) == 0, "lovasz: workspace must be 16-byte aligned");
  PSEG_REQUIRE(dlogits != logits, "lovasz: dlogits must not alias logits");
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  LvHeader* hdr = (LvHeader*)ws;
  unsigned* totals = (unsigned*)(ws + pl.totals);
  unsigned* blockhist = (unsigned*)(ws + pl.blockhist);
  unsigned* tilecnt = (unsigned*)(ws + pl.tilecnt);
  double* partial = (double*)(ws + pl.partial);
  unsigned* keys[2] = {(unsigned*)(ws + pl.keys[0]), (unsigned*)(ws + pl.keys[1])};
  unsigned* idx[2] = {(unsigned*)(ws + pl.idx[0]), (unsigned*)(ws + pl.idx[1])};
  const unsigned npix = (unsigned)npix64, hw = (unsigned)HW, nb = pl.nb;
  const size_t S = pl.S;
  const int G = lv_group_override(pl.G);
  const long long ign = (long long)ignore_index;

  if (hipMemsetAsync(hdr, 0, sizeof(LvHeader), st) != hipSuccess) {
    set_error("lovasz: hipMemsetAsync failed");
    return PSEG_ERR_HIP;
  }
  hipLaunchKernelGGL(lovasz_hist_kernel, dim3(capped_blocks(npix64, 2048)), dim3(kLvThreads), 0, st,
                     target, npix, ign, C, hdr);
  PSEG_LAUNCH_CHECK();
  hipLaunchKernelGGL(lovasz_present_kernel, dim3(1), dim3(kLvThreads), 0, st, C, hdr);
  PSEG_LAUNCH_CHECK();
  for (int c0 = 0; c0 < C; c0 += G) {
    const int g = C - c0 < G ? C - c0 : G;
    const dim3 tiles(nb, g);
    hipLaunchKernelGGL(lovasz_errors_kernel, dim3(capped_blocks(npix64, kLvMaxBlocks)), dim3(kLvThreads), 0, st, logits, target,
                       C, hw, npix, ign, (const LvHeader*)hdr, c0, g, S, keys[0]);
    PSEG_LAUNCH_CHECK();
    for (int pass = 0; pass < kLvPasses; ++pass) {      // keys[0] -> [1] -> [0] -> [1] -> [0]
      const int a = pass & 1, b = a ^ 1, shift = 8 * pass;
      hipLaunchKernelGGL(lovasz_sort_hist_kernel, tiles, dim3(kLvThreads), 0, st, (const unsigned*)keys[a], npix, S, shift,
                         (const LvHeader*)hdr, c0, nb, blockhist);
      PSEG_LAUNCH_CHECK();
      hipLaunchKernelGGL(lovasz_scan_rows_kernel, dim3(256, g), dim3(kLvThreads), 0, st, blockhist, nb, totals,
                         (const LvHeader*)hdr, c0);
      PSEG_LAUNCH_CHECK();
      if (pass == 0)
        hipLaunchKernelGGL((lovasz_sort_scatter_kernel<true>), tiles, dim3(kLvThreads), 0, st, (const unsigned*)keys[a],
                           (const unsigned*)idx[a], keys[b], idx[b], npix, S, shift, (const LvHeader*)hdr, c0, nb,
                           (const unsigned*)blockhist, (const unsigned*)totals);
      else
        hipLaunchKernelGGL((lovasz_sort_scatter_kernel<false>), tiles, dim3(kLvThreads), 0, st, (const unsigned*)keys[a],
                           (const unsigned*)idx[a], keys[b], idx[b], npix, S, shift, (const LvHeader*)hdr, c0, nb,
                           (const unsigned*)blockhist, (const unsigned*)totals);
      PSEG_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(lovasz_fg_count_kernel, tiles, dim3(kLvThreads), 0, st, (const unsigned*)keys[0], npix, S,
                       (const LvHeader*)hdr, c0, nb, tilecnt);
    PSEG_LAUNCH_CHECK();
    hipLaunchKernelGGL(lovasz_scan_rows_kernel, dim3(1, g), dim3(kLvThreads), 0, st, tilecnt, nb, (unsigned*)nullptr,
                       (const LvHeader*)hdr, c0);
    PSEG_LAUNCH_CHECK();
    hipLaunchKernelGGL(lovasz_grad_kernel, tiles, dim3(kLvThreads), 0, st, (const unsigned*)keys[0], (const unsigned*)idx[0],
                       npix, S, hw, C, (const LvHeader*)hdr, c0, nb, (const unsigned*)tilecnt, partial, dlogits);
    PSEG_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(lovasz_finish_kernel, dim3(1), dim3(kLvThreads), 0, st, (const double*)partial, C, nb,
                     (const LvHeader*)hdr, out);
  PSEG_LAUNCH_CHECK();
  if (dlogits) {
    hipLaunchKernelGGL(lovasz_softmax_bwd_kernel, dim3(capped_blocks(npix64, kLvMaxBlocks)), dim3(kLvThreads), 0, st, logits,
                       target, C, hw, npix, ign, (const LvHeader*)hdr, dlogits);
    PSEG_LAUNCH_CHECK();
  }
  return PSEG_OK;
}

}  // extern "C"
