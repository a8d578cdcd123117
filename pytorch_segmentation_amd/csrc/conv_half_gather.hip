// Half-precision (`-mp`) convolution for gfx950, forward and data gradient: fp16 activations / gradients / filters in HBM,
// single-pass v_mfma_f32_32x32x16_f16 with fp32 accumulation.  This is the arithmetic the reference asks apex for with `-mp`
// (train.py:70,102-105,138; README.md:12: fp16 compute, fp32 master weights, loss scaling).  The weight gradient is
// conv_half_wgrad.hip; conv_half.h holds what the two share.
//
//  gather_h_kernel   forward and data gradient: C[M = pixels][N] = A[M][K] * Bw[N][K]^T, both operands K-contiguous fp16.
//     Same implicit-GEMM formulation, GEMM-row orders (patch / parity / liveness-class sorted), tap skipping and fused
//     BatchNorm statistics as gather_f32_dma_kernel (conv_gather.hip); tiles go global -> LDS by `buffer_load_dwordx4 ... lds`
//     into a two-stage ring of [rows][64 halves = 128 B] images (16-byte k-slot XOR (row >> 1) & 7, applied on the source
//     side), one ds_read_b128 = the 8 consecutive k of one MFMA operand.  Output fp16 (or fp32 for the class logits, which
//     the loss reads), written in 16-byte pieces through a wave-private LDS patch.
//     GENERIC = true: channel counts that are not multiples of 64 (HRNet's 32-channel branch, MobileNetV2, the stem): a
//     K-step may straddle taps, every lane derives (tap, channel) of its own 16-byte slot.
//  gather_hp_kernel  the persistent form for the short contractions (described where it is defined).
//  filter_prepare_h_kernel, convert2d_kernel   the fp16 filter copies and the fp32 <-> fp16 tensor conversion.
#include "conv_half.h"

namespace pseg {

struct HGatherParams {
  GatherConvParams g;    // x / w / y are fp16 here (y fp32 when y_f32); element strides as in the fp32 kernels
  int y_f32;
  FastDiv cin_div, kw_div;   // GENERIC: k -> (tap, channel), tap -> (row, column)
  FastDiv howo_div, wo_div;  // gather_hp_kernel: GEMM row -> (image, row, column)
  int ntiles;                // gather_hp_kernel: tiles of the launch (a persistent block walks blockIdx, blockIdx + grid, ...)
  int tail_pad;              // unused: keeps the launch's implicit arguments (block counts), which follow this block, off ntiles'
                             // neighbouring dword -- next to it hipcc fuses the two loads and re-allocates the persistent kernels
};

// KB: halves per K-step = 64 (128-byte LDS rows, 8 rows per DMA wave-instruction) or 32 (64-byte rows, 16 rows per
// wave-instruction).  The short K-step halves the ring -- with the 32-row epilogue patch a 128x128 / 8-wave block needs 36 KB of
// LDS and four of them share a CU (32 waves) -- which is what the many short, latency-bound launches of a training step want
// (a layer's blocks spend most of their life waiting for their first tile and for their stores); the long K-step has half
// the barriers per MAC and serves the deep contractions.
// STAGES: depth of the operand ring.  A block keeps STAGES - 1 tiles in flight; with one fp16 MFMA pass per tile the matrix
// work of a K-step (128-512 cycles) is far shorter than a memory round trip (1500+ cycles under load), so the rate of a CU is
// bytes in flight / latency (Little's law): the ring depth x resident blocks, not the issue rate, is what sets it.
template <int BM, int BN, int WARPS_M, int WARPS_N, bool SKIP, bool GENERIC, int KB, int STAGES, bool BNS = false>
__global__ __launch_bounds__(64 * WARPS_M * WARPS_N) void gather_h_kernel(const HGatherParams hp) {
  const GatherConvParams& p = hp.g;
  set_wave_prio(p.prio);
  static_assert(!(SKIP && GENERIC), "tap skipping needs whole K-steps per tap");
  static_assert(KB == 64 || KB == 32, "K-step");
  constexpr int NW = WARPS_M * WARPS_N;
  static_assert(NW == 16 || NW == 8 || NW == 4, "16, 8 or 4 waves");
  constexpr int WTM = BM / WARPS_M, WTN = BN / WARPS_N, TM = WTM / 32, TN = WTN / 32;
  static_assert(TM >= 1 && TN >= 1 && WTM % 32 == 0 && WTN % 32 == 0, "wave tile");
  constexpr int RDW = KB / 2;                     // dwords per LDS row (32 or 16)
  constexpr int NSLOT = KB / 8;                   // 16-byte k-slots per row (8 or 4)
  constexpr int RPG = 64 / NSLOT;                 // rows per DMA wave-instruction (8 or 16)
  constexpr int kStageDw = (BM + BN) * RDW;
  constexpr int kPatch = NW * 32 * (WTN + 4);
  static_assert(STAGES >= 2 && STAGES <= 4, "ring depth");
  constexpr int kLds = STAGES * kStageDw > kPatch ? STAGES * kStageDw : kPatch;
  static_assert(kLds * 4 <= 160 * 1024, "LDS");
  __shared__ __attribute__((aligned(16))) float lds[kLds];
  unsigned* ldsw = reinterpret_cast<unsigned*>(lds);
  constexpr int kA = 0, kB = BM * RDW;
  // DMA row groups (RPG rows each): wave w owns A groups w, w + NW, ... and B groups likewise
  constexpr int GA = BM / RPG / NW, GB = (BN / RPG + NW - 1) / NW, NG = GA + GB;
  static_assert((BM / RPG) % NW == 0 && GA >= 1, "whole A row groups per wave");
  constexpr bool kBPartial = (BN / RPG) % NW != 0;   // narrow tiles: fewer B groups than waves

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WARPS_N, wn = wave % WARPS_N;
  const int gridN = (p.N + BN - 1) / BN;
  int bid = blockIdx.x;
  bid = remap_tile(p.xcd_remap, bid, (int)gridDim.x);
  const int tile_n = bid % gridN;
  const int tile_m = bid / gridN;
  const int m0 = tile_m * BM, n0 = tile_n * BN;

  const __amdgpu_buffer_rsrc_t xr = make_rsrc(p.x, p.x_bytes);
  const __amdgpu_buffer_rsrc_t wr = make_rsrc(p.w, p.w_bytes);

  // image swizzle: k-slot s of row r lives at physical slot s ^ f(r); f(r) = (r >> 1) & 7 for 128-byte rows, (r >> 2) & 3
  // for 64-byte rows (the 16-lane groups of the fragment ds_read_b128 then cover all 64 banks once)
  auto fsw = [](int row) -> int { return KB == 64 ? ((row >> 1) & 7) : ((row >> 2) & 3); };
  const int lrow = lane / NSLOT, lslot = lane % NSLOT;
  // logical k-slot of this lane: the same for every row group (rows RPG * (wave + NW * g) + lrow: f(row) does not depend
  // on g while NW is even)
  const int lslot_log = lslot ^ fsw(RPG * wave + lrow);
  int a_bh[GA], a_bw[GA], a_img[GA];
  bool a_ok[GA];
#pragma unroll
  for (int g = 0; g < GA; ++g) {
    const int row = RPG * (wave + NW * g) + lrow;
    const int m = m0 + row;
    const bool ok = m < p.M;
    int b, ho, wo;
    row_to_pixel(p, ok ? m : 0, b, ho, wo);
    a_ok[g] = ok;
    a_bh[g] = ho * p.s_out + p.off0;
    a_bw[g] = wo * p.s_out + p.off0;
    a_img[g] = b * p.Hi * p.Wi;
  }
  uint32_t b_rowoff[GB];
  bool b_ok[GB];
  int b_grp[GB];
#pragma unroll
  for (int g = 0; g < GB; ++g) {
    // (narrow tile: a wave beyond the tile's B groups re-loads group (wave mod groups) -- the same bytes into the same
    // place as its owner, harmless -- so that every wave issues, and counts, the same number of DMAs per K-step)
    b_grp[g] = kBPartial ? (wave + NW * g) % (BN / RPG) : (wave + NW * g);
    const int row = RPG * b_grp[g] + lrow;
    b_ok[g] = (n0 + row) < p.N;
    b_rowoff[g] = b_ok[g] ? (uint32_t)(n0 + row) * (uint32_t)p.K * 2u + (uint32_t)(lslot_log * 16) : kOOB;
  }

  auto row_tap_ok = [&](int g, int dh, int dw, int& hn, int& wn_) -> bool {
    hn = a_bh[g] + dh;
    wn_ = a_bw[g] + dw;
    bool ok = a_ok[g];
    if (p.s_in != 1) {
      ok = ok && (hn % p.s_in == 0) && (wn_ % p.s_in == 0);
      hn /= p.s_in;
      wn_ /= p.s_in;
    }
    return ok && ((unsigned)hn < (unsigned)p.Hi) && ((unsigned)wn_ < (unsigned)p.Wi);
  };

  const int kt_end = p.kt_total;
  unsigned tapmask = 0xFFFFFFFFu;
  if (SKIP) {
    unsigned mine = 0;
    for (int t = 0; t < p.ntaps; ++t) {
      const int r = t / p.kw, sx = t - r * p.kw;
      bool any = false;
#pragma unroll
      for (int g = 0; g < GA; ++g) {
        int hn, wn_;
        any = any || row_tap_ok(g, r * p.dstep, sx * p.dstep, hn, wn_);
      }
      if (any) mine |= 1u << t;
    }
    if (tid == 0) ldsw[0] = 0u;
    __syncthreads();
    if (mine) atomicOr(&ldsw[0], mine);
    __syncthreads();
    tapmask = ldsw[0];
    __syncthreads();
  }
  int n_steps;
  int s_chunk = 0, s_lin = 0;
  unsigned s_tm = tapmask;
  if (!SKIP) {
    n_steps = kt_end;            // every K-step, in order (any number of taps)
  } else {
    tapmask &= (p.ntaps >= 32) ? 0xFFFFFFFFu : ((1u << p.ntaps) - 1u);      // (host: skipping only with <= 32 taps)
    s_tm = tapmask;
    n_steps = __builtin_popcount(tapmask) * p.ktiles_per_tap;
  }
  auto next_kt = [&]() -> int {     // next live K-step (tap major), kt_end when exhausted
    if (!SKIP) {
      const int kt = s_lin < kt_end ? s_lin : kt_end;
      ++s_lin;
      return kt;
    }
    if (s_tm == 0u) return kt_end;
    const int kt = __builtin_ctz(s_tm) * p.ktiles_per_tap + s_chunk;
    if (++s_chunk == p.ktiles_per_tap) {
      s_chunk = 0;
      s_tm &= s_tm - 1u;
    }
    return kt;
  };

  int tap_cur = -1;
  uint32_t a_off[GA];
#pragma unroll
  for (int g = 0; g < GA; ++g) a_off[g] = kOOB;
  typedef __attribute__((address_space(3))) void* lds_ptr;
  auto issue = [&](int kt, int st) {
    uint32_t ao[GA], bo[GB];
    if (kt < kt_end) {
      if (GENERIC) {
        // this lane's 16-byte slot: k = kt * KB + 8 * slot -> (tap, channel); slots beyond K read as zeros
        const int kb = kt * KB + lslot_log * 8;
        const bool kin = kb < p.K;
        const uint32_t tap = hp.cin_div.div((uint32_t)kb);
        const int c = kb - (int)tap * p.Cin;
        const uint32_t kr = hp.kw_div.div(tap);
        const int ks = (int)tap - (int)kr * p.kw;
#pragma unroll
        for (int g = 0; g < GA; ++g) {
          int hn, wn_;
          const bool ok = row_tap_ok(g, (int)kr * p.dstep, ks * p.dstep, hn, wn_) && kin;
          ao[g] = ok ? (uint32_t)((a_img[g] + hn * p.Wi + wn_) * p.ldx + c) * 2u : kOOB;
        }
#pragma unroll
        for (int g = 0; g < GB; ++g)
          bo[g] = (kin && b_ok[g]) ? b_rowoff[g] - (uint32_t)(lslot_log * 16) + (uint32_t)kb * 2u : kOOB;
      } else {
        const int tap = kt / p.ktiles_per_tap;
        if (tap != tap_cur) {
          tap_cur = tap;
          const int kr = tap / p.kw, ks = tap - kr * p.kw;
#pragma unroll
          for (int g = 0; g < GA; ++g) {
            int hn, wn_;
            const bool ok = row_tap_ok(g, kr * p.dstep, ks * p.dstep, hn, wn_);
            a_off[g] = ok ? (uint32_t)((a_img[g] + hn * p.Wi + wn_) * p.ldx) * 2u + (uint32_t)(lslot_log * 16) : kOOB;
          }
        }
        const uint32_t kc_b = (uint32_t)((kt - tap * p.ktiles_per_tap) * KB) * 2u;
#pragma unroll
        for (int g = 0; g < GA; ++g) ao[g] = a_off[g] + kc_b;     // kOOB + kc_b stays out of range
#pragma unroll
        for (int g = 0; g < GB; ++g) bo[g] = b_rowoff[g] + (uint32_t)kt * (uint32_t)(KB * 2);
      }
    } else {
#pragma unroll
      for (int g = 0; g < GA; ++g) ao[g] = kOOB;
#pragma unroll
      for (int g = 0; g < GB; ++g) bo[g] = kOOB;
    }
    unsigned* sb = ldsw + st * kStageDw;
#pragma unroll
    for (int g = 0; g < GA; ++g)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(xr, (lds_ptr)(sb + kA + RPG * (wave + NW * g) * RDW), 16, (int)ao[g], 0, 0, 0);
#pragma unroll
    for (int g = 0; g < GB; ++g)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(wr, (lds_ptr)(sb + kB + RPG * b_grp[g] * RDW), 16, (int)bo[g], 0, 0, 0);
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int frag_row = lane & 31;
  const int frag_h = lane >> 5;
  auto swz = [&](int row, int slot) -> int { return row * RDW + ((slot ^ fsw(row)) << 2); };
  constexpr int HK = KB / 32;           // MFMAs (16-deep k-steps) per half of a K-step: 2 or 1
  f32x4 fa[2][HK * TM], fb[2][HK * TN];   // [set][gg * T + tile]: the 8 k of MFMA gg of a half-step
  auto read_frags = [&](int set, int st, int half) {
    const float* sb = lds + st * kStageDw;
#pragma unroll
    for (int gg = 0; gg < HK; ++gg) {
      const int slot = 2 * (half * HK + gg) + frag_h;
#pragma unroll
      for (int i = 0; i < TM; ++i)
        fa[set][gg * TM + i] = *reinterpret_cast<const f32x4*>(&sb[kA + swz(wm * WTM + i * 32 + frag_row, slot)]);
#pragma unroll
      for (int j = 0; j < TN; ++j)
        fb[set][gg * TN + j] = *reinterpret_cast<const f32x4*>(&sb[kB + swz(wn * WTN + j * 32 + frag_row, slot)]);
    }
  };
  auto mfmas = [&](int set) {
#pragma unroll
    for (int gg = 0; gg < HK; ++gg)
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8v, fa[set][gg * TM + i]),
                                                             __builtin_bit_cast(f16x8v, fb[set][gg * TN + j]), acc[i][j],
                                                             0, 0, 0);
  };
  // counted waits: NG DMAs per tile and wave
  if constexpr (GENERIC) {
    if (n_steps > 0) {
#pragma unroll
      for (int s0 = 0; s0 < STAGES; ++s0) issue(next_kt(), s0);
      wait_vmcnt<(STAGES - 1) * NG>();   // tile 0 has landed (this wave's share); STAGES - 1 tiles stay in flight
      __builtin_amdgcn_s_barrier();      // ... and everybody's
      read_frags(0, 0, 0);
      int st = 0;
      for (int it = 0; it < n_steps; ++it) {
        const int st1 = st == STAGES - 1 ? 0 : st + 1;
        read_frags(1, st, 1);
        __builtin_amdgcn_sched_barrier(0);
        mfmas(0);
        __builtin_amdgcn_sched_barrier(0);
        wait_vmcnt<(STAGES - 2) * NG>();                     // the next tile has landed; STAGES - 2 more stay in flight
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave is done reading stage `st`
        __builtin_amdgcn_s_barrier();
        read_frags(0, st1, 0);      // (zeros on the last step: never multiplied)
        __builtin_amdgcn_sched_barrier(0);
        issue(next_kt(), st);       // stage `st` is free now
        mfmas(1);
        __builtin_amdgcn_sched_barrier(0);
        st = st1;
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // dummy DMAs must not land in the output patches
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
  } else if (n_steps > 0) {
    // ---- the K loop with its bookkeeping taken out (round 4).  Counters of round 3's loop on the DeepLabV3+ shapes: 4.8 VALU +
    // 6 SALU instructions per MFMA on the deep contractions, 12 + 12 on the K = 512 pointwise layers (a division of the K-step
    // index by the steps per tap, the tap test and the address rebuild on every step) -- the waves were issuing bookkeeping, not
    // waiting for memory.  Now a K-step costs one add per DMA: a tap is OPENED once (per-row validity and base offsets: the only
    // place that multiplies), its channel chunks advance both operands by KB * 2 bytes, and the ring stage is a compile-time
    // constant of the unrolled step, so fragment and DMA addresses are loop-invariant registers + immediates.
    unsigned taps_left = SKIP ? tapmask : 0u;
    int tap_next = 0, chunks_left = 0;
    uint32_t a_cur[GA], b_cur[GB];
    const uint32_t tap_bytes = (uint32_t)p.Cin * 2u;
    auto open_tap = [&]() {
      int tap = -1;
      if (SKIP) {
        if (taps_left != 0u) {
          tap = __builtin_ctz(taps_left);
          taps_left &= taps_left - 1u;
        }
      } else if (tap_next < p.ntaps) {
        tap = tap_next++;
      }
      if (tap < 0) {                  // exhausted: the remaining (dummy) DMAs move nothing
#pragma unroll
        for (int g = 0; g < GA; ++g) a_cur[g] = kOOB;
#pragma unroll
        for (int g = 0; g < GB; ++g) b_cur[g] = kOOB;
        chunks_left = 0x7fffffff;
        return;
      }
      const int kr = (int)hp.kw_div.div((uint32_t)tap), ks = tap - kr * p.kw;
#pragma unroll
      for (int g = 0; g < GA; ++g) {
        int hn, wn_;
        const bool ok = row_tap_ok(g, kr * p.dstep, ks * p.dstep, hn, wn_);
        a_cur[g] = ok ? (uint32_t)((a_img[g] + hn * p.Wi + wn_) * p.ldx) * 2u + (uint32_t)(lslot_log * 16) : kOOB;
      }
#pragma unroll
      for (int g = 0; g < GB; ++g) b_cur[g] = b_rowoff[g] + (uint32_t)tap * tap_bytes;     // (kOOB rows stay out of range)
      chunks_left = p.ktiles_per_tap;
    };
    auto issue_c = [&](auto stc) {
      constexpr int ST = decltype(stc)::value;
      if (chunks_left == 0) open_tap();
      unsigned* sb = ldsw + ST * kStageDw;
#pragma unroll
      for (int g = 0; g < GA; ++g)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(xr, (lds_ptr)(sb + kA + RPG * (wave + NW * g) * RDW), 16, (int)a_cur[g], 0, 0, 0);
#pragma unroll
      for (int g = 0; g < GB; ++g)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(wr, (lds_ptr)(sb + kB + RPG * b_grp[g] * RDW), 16, (int)b_cur[g], 0, 0, 0);
#pragma unroll
      for (int g = 0; g < GA; ++g) a_cur[g] += (uint32_t)(KB * 2);
#pragma unroll
      for (int g = 0; g < GB; ++g) b_cur[g] += (uint32_t)(KB * 2);
      --chunks_left;
    };
    // loop-invariant fragment addresses (dwords inside a stage): [half * HK + gg] of the wave's first A / B tile row
    int fa_off[2 * HK], fb_off[2 * HK];
#pragma unroll
    for (int q = 0; q < 2 * HK; ++q) {
      fa_off[q] = kA + swz(wm * WTM + frag_row, 2 * q + frag_h);
      fb_off[q] = kB + swz(wn * WTN + frag_row, 2 * q + frag_h);
    }
    auto read_c = [&](auto stc, auto setc, auto halfc) {
      constexpr int ST = decltype(stc)::value, SET = decltype(setc)::value, HALF = decltype(halfc)::value;
      const float* sb = lds + ST * kStageDw;
#pragma unroll
      for (int gg = 0; gg < HK; ++gg) {
#pragma unroll
        for (int i = 0; i < TM; ++i)      // (tile rows 32 apart keep the swizzle: f(row + 32) = f(row))
          fa[SET][gg * TM + i] = *reinterpret_cast<const f32x4*>(&sb[fa_off[HALF * HK + gg] + i * 32 * RDW]);
#pragma unroll
        for (int j = 0; j < TN; ++j)
          fb[SET][gg * TN + j] = *reinterpret_cast<const f32x4*>(&sb[fb_off[HALF * HK + gg] + j * 32 * RDW]);
      }
    };
    typedef std::integral_constant<int, 0> c0;
    typedef std::integral_constant<int, 1> c1;
    issue_c(c0{});
    if constexpr (STAGES >= 2) issue_c(c1{});
    if constexpr (STAGES >= 3) issue_c(std::integral_constant<int, 2>{});
    if constexpr (STAGES >= 4) issue_c(std::integral_constant<int, 3>{});
    wait_vmcnt<(STAGES - 1) * NG>();   // tile 0 has landed (this wave's share); STAGES - 1 tiles stay in flight
    __builtin_amdgcn_s_barrier();      // ... and everybody's
    read_c(c0{}, c0{}, c0{});
#define PSEG_GH_STEP(S)                                                                                          \
  {                                                                                                              \
    typedef std::integral_constant<int, (S)> cs;                                                                 \
    typedef std::integral_constant<int, ((S) + 1) % STAGES> cs1;                                                 \
    read_c(cs{}, c1{}, c1{});                                                                                    \
    __builtin_amdgcn_sched_barrier(0);                                                                           \
    mfmas(0);                                                                                                    \
    __builtin_amdgcn_sched_barrier(0);                                                                           \
    wait_vmcnt<(STAGES - 2) * NG>();                   /* the next tile has landed; STAGES - 2 more in flight */  \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); /* this wave is done reading stage S */                   \
    __builtin_amdgcn_s_barrier();                                                                                \
    read_c(cs1{}, c0{}, c0{});                         /* (zeros on the last step: never multiplied) */          \
    __builtin_amdgcn_sched_barrier(0);                                                                           \
    issue_c(cs{});                                     /* stage S is free now */                                 \
    mfmas(1);                                                                                                    \
    __builtin_amdgcn_sched_barrier(0);                                                                           \
  }
    for (int it = 0;;) {
      PSEG_GH_STEP(0)
      if (++it == n_steps) break;
      PSEG_GH_STEP(1)
      if (++it == n_steps) break;
      if constexpr (STAGES >= 3) {
        PSEG_GH_STEP(2)
        if (++it == n_steps) break;
      }
      if constexpr (STAGES >= 4) {
        PSEG_GH_STEP(3)
        if (++it == n_steps) break;
      }
    }
#undef PSEG_GH_STEP
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // dummy DMAs must not land in the output patches
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }

  // ---- epilogue: bias / accumulate / row map, fused BatchNorm statistics
  const int col_l = lane & 31;
  const int row_h = (lane >> 5) * 4;
  float* patch = lds + wave * (32 * (WTN + 4));
  const int col0 = n0 + wn * WTN;
  int cv = p.N - col0;
  cv = cv < 0 ? 0 : (cv > WTN ? WTN : cv);
  auto rowmap = [&](int m) {
    if (!p.row_perm) return m;
    int b, ho, wo;
    row_to_pixel(p, m, b, ho, wo);
    return (b * p.Ho + ho) * p.Wo + wo;
  };
  if constexpr (BNS) {
    // (the host only launches this instantiation for an fp16 result without bias / accumulation)
    constexpr int C8 = WTN / 8;
    const int c8 = lane % C8, rr = lane / C8;
    const bool cok = c8 * 8 < cv;
    HBnsCoef bc;
    HBnsSums bs;
    bns_load_coef(p, col0 + c8 * 8, cok, bc);
#pragma unroll
    for (int h = 0; h < 2; ++h) bs.s1[h] = bs.s2[h] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int row0 = m0 + wm * WTM + i * 32;
      int rv = p.M - row0;
      rv = rv < 0 ? 0 : (rv > 32 ? 32 : rv);
      store_row32<TN, true>(acc[i], patch, p.y, false, p.ldy, row0, col0, rv, cv, nullptr, false, lane, rowmap, p, bc, bs);
    }
#pragma unroll
    for (int o = C8; o < 64; o <<= 1)
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          bs.s1[h][e] += __shfl_xor(bs.s1[h][e], o, 64);
          bs.s2[h][e] += __shfl_xor(bs.s2[h][e], o, 64);
        }
    if (rr == 0 && cok) {
      const long long o = (long long)(tile_m * WARPS_M + wm) * p.N + col0 + c8 * 8;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        *reinterpret_cast<f32x4*>(p.bns_db + o + 4 * h) = bs.s1[h];
        *reinterpret_cast<f32x4*>(p.bns_dg + o + 4 * h) = bs.s2[h];
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int row0 = m0 + wm * WTM + i * 32;
      int rv = p.M - row0;
      rv = rv < 0 ? 0 : (rv > 32 ? 32 : rv);
      store_row32<TN>(acc[i], patch, p.y, hp.y_f32 != 0, p.ldy, row0, col0, rv, cv, p.bias, p.accumulate != 0, lane, rowmap);
    }
  }
  if (p.stat != nullptr) {
    // BatchNorm statistics of the tensor AS STORED: an fp16 result is rounded before it is summed, so that the layer
    // normalises exactly the values its backward pass and the next layer read (what a BatchNorm fed by an fp16 conv sees)
    const bool f32out = hp.y_f32 != 0;
    auto rnd = [&](float v) -> float { return f32out ? v : (float)(half_t)v; };
    const int group = tile_m * WARPS_M + wm;
    const long long gsz = (long long)p.stat_rows * p.N;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int col = n0 + wn * WTN + j * 32 + col_l;
      const float k0 = __shfl(rnd(acc[0][j][0]), lane & 31, 64);
      float s1 = 0.f, s2 = 0.f;
      if (m0 + BM <= p.M) {       // (block-uniform: every row of the tile is a pixel -- no per-element test)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float d = rnd(acc[i][j][r]) - k0;
            s1 += d;
            s2 += d * d;
          }
      } else {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int row = m0 + wm * WTM + i * 32 + (r & 3) + 8 * (r >> 2) + row_h;
            if (row < p.M) {
              const float d = rnd(acc[i][j][r]) - k0;
              s1 += d;
              s2 += d * d;
            }
          }
      }
      s1 += __shfl_xor(s1, 32, 64);
      s2 += __shfl_xor(s2, 32, 64);
      if (lane < 32 && col < p.N) {
        const long long o = (long long)group * p.N + col;
        p.stat[o] = k0;
        p.stat[gsz + o] = s1;
        p.stat[2 * gsz + o] = s2;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ persistent gather kernel
// Round 4.  What the ablation of gather_h_kernel on the DeepLabV3+ shapes showed (profiles/scripts/exp_ablate.sh, profiles/EXPERIMENTS.md):
// with stores, statistics, operand DMAs, fragment reads and MFMAs ALL switched off, half of the time of a launch is still
// there -- a block's life is a latency chain (kernel arguments, row -> pixel arithmetic, the first tile's round trip, eight
// waves meeting at a barrier, the LDS round trip of the epilogue, the stores' drain) and a CU holds only two or three blocks
// to hide one chain behind another; the short contractions (K <= 512: 2-16 K-steps) are nothing but chain.
// Here a block is PERSISTENT: it walks tiles blockIdx, blockIdx + grid, ... and the operand ring never drains -- the DMAs of
// the next tile's first K-steps are issued before the current tile's last MFMA, its row -> pixel arithmetic runs inside
// that issue slot, and the epilogue works out of a wave-private patch of its own while they land:
//   * one continuous stream of (tile, tap, channel chunk) K-steps; a tap is opened once, chunks advance by KB * 2 bytes;
//   * the ring stage is a compile-time constant of the unrolled step (a switch re-enters the unrolled sequence at the
//     phase the previous tile ended on);
//   * epilogue for fp16 results: the 32x32 accumulator tile goes to LDS TRANSPOSED, four 8-byte writes per lane
//     (ds_write_b64: a lane's four consecutive rows of one column), and comes back through ds_read_b64_tr_b16 as 8
//     consecutive channels per lane for 16-byte stores -- 8 LDS instructions per tile where the fp32 patch of
//     gather_h_kernel takes 20, and 2.3 KB of patch per wave instead of 4.6; no block barrier anywhere in it.
// Covers what most launches of a training step are: every tap live (no skipping), channels a multiple of the K-step, fp16
// result without bias / accumulation, rows in natural order.  Everything else stays on gather_h_kernel.
typedef short s16x4g __attribute__((ext_vector_type(4)));
typedef short s16x8g __attribute__((ext_vector_type(8)));

template <int BM, int BN, int WARPS_M, int WARPS_N, int KB, int STAGES, bool BNS = false>
__global__ __launch_bounds__(64 * WARPS_M * WARPS_N) void gather_hp_kernel(const HGatherParams hp) {
  const GatherConvParams& p = hp.g;
  set_wave_prio(p.prio);
  static_assert(KB == 64 || KB == 32, "K-step");
  constexpr int NW = WARPS_M * WARPS_N;
  static_assert(NW == 8 || NW == 4, "8 or 4 waves");
  constexpr int WTM = BM / WARPS_M, WTN = BN / WARPS_N, TM = WTM / 32, TN = WTN / 32;
  static_assert(TM >= 1 && TN >= 1 && WTM % 32 == 0 && WTN % 32 == 0, "wave tile");
  constexpr int RDW = KB / 2, NSLOT = KB / 8, RPG = 64 / NSLOT;
  constexpr int kStageDw = (BM + BN) * RDW;
  static_assert(STAGES == 2 || STAGES == 3, "ring depth");
  constexpr int kPitch = 72;                         // bytes per patch row = one output column: 32 rows x 2 B + 8 (bank spread)
  constexpr int kPatchB = 32 * kPitch;
  constexpr int kRingB = STAGES * kStageDw * 4;
  constexpr int kLdsB = kRingB + NW * kPatchB;
  static_assert(kLdsB <= 160 * 1024, "LDS");
  __shared__ __attribute__((aligned(16))) unsigned char lds_raw[kLdsB];
  float* lds = reinterpret_cast<float*>(lds_raw);
  unsigned* ldsw = reinterpret_cast<unsigned*>(lds_raw);
  constexpr int kA = 0, kB = BM * RDW;
  constexpr int GA = BM / RPG / NW, GB = (BN / RPG + NW - 1) / NW, NG = GA + GB;
  static_assert((BM / RPG) % NW == 0 && GA >= 1, "whole A row groups per wave");
  constexpr bool kBPartial = (BN / RPG) % NW != 0;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WARPS_N, wn = wave % WARPS_N;
  const int gridN = (p.N + BN - 1) / BN;
  const int ntiles = hp.ntiles;
  const int nblocks = (int)gridDim.x;

  const __amdgpu_buffer_rsrc_t xr = make_rsrc(p.x, p.x_bytes);
  const __amdgpu_buffer_rsrc_t wr = make_rsrc(p.w, p.w_bytes);
  auto fsw = [](int row) -> int { return KB == 64 ? ((row >> 1) & 7) : ((row >> 2) & 3); };
  const int lrow = lane / NSLOT, lslot = lane % NSLOT;
  const int lslot_log = lslot ^ fsw(RPG * wave + lrow);
  int b_grp[GB];
#pragma unroll
  for (int g = 0; g < GB; ++g) b_grp[g] = kBPartial ? (wave + NW * g) % (BN / RPG) : (wave + NW * g);

  // ---- issue side: the stream of K-steps over this block's tiles
  int i_vt = (int)blockIdx.x;          // next virtual tile to open
  int tap_next = p.ntaps;              // (== ntaps: the first open_tap opens a tile)
  int chunks_left = 0;
  int a_bh[GA], a_bw[GA], a_img[GA];
  bool a_ok[GA];
  uint32_t b_rowoff[GB];
  uint32_t a_cur[GA], b_cur[GB];
  const uint32_t tap_bytes = (uint32_t)p.Cin * 2u;
  auto open_tile = [&]() -> bool {
    if (i_vt >= ntiles) return false;
    const int t = remap_tile(p.xcd_remap, i_vt, ntiles);
    i_vt += nblocks;
    const int tile_n = t % gridN, tile_m = t / gridN;
    const int m0 = tile_m * BM, n0 = tile_n * BN;
#pragma unroll
    for (int g = 0; g < GA; ++g) {
      const int m = m0 + RPG * (wave + NW * g) + lrow;
      const bool ok = m < p.M;
      // rows in natural order only (the host sends the permuted orders -- patches, parity classes, liveness classes -- to
      // gather_h_kernel): pixel m of the [B, Ho, Wo] row space, or of the 1 x M image of a pointwise conv (HoWo = Wo = M)
      const uint32_t mm = ok ? (uint32_t)m : 0u;
      const uint32_t b = hp.howo_div.div(mm);
      const uint32_t rem = mm - b * (uint32_t)p.HoWo;
      const uint32_t ho = hp.wo_div.div(rem);
      const uint32_t wo = rem - ho * (uint32_t)p.Wo;
      a_ok[g] = ok;
      a_bh[g] = (int)ho * p.s_out + p.off0;
      a_bw[g] = (int)wo * p.s_out + p.off0;
      a_img[g] = (int)b * p.Hi * p.Wi;
    }
#pragma unroll
    for (int g = 0; g < GB; ++g) {
      const int row = n0 + RPG * b_grp[g] + lrow;
      b_rowoff[g] = row < p.N ? (uint32_t)row * (uint32_t)p.K * 2u + (uint32_t)(lslot_log * 16) : kOOB;
    }
    tap_next = 0;
    return true;
  };
  auto open_tap = [&]() {
    if (tap_next >= p.ntaps && !open_tile()) {      // exhausted: the remaining (dummy) DMAs fetch nothing
#pragma unroll
      for (int g = 0; g < GA; ++g) a_cur[g] = kOOB;
#pragma unroll
      for (int g = 0; g < GB; ++g) b_cur[g] = kOOB;
      chunks_left = 0x7fffffff;
      return;
    }
    const int tap = tap_next++;
    const int kr = (int)hp.kw_div.div((uint32_t)tap), ks = tap - kr * p.kw;
    const int dh = kr * p.dstep, dw = ks * p.dstep;
#pragma unroll
    for (int g = 0; g < GA; ++g) {
      int hn = a_bh[g] + dh, wn_ = a_bw[g] + dw;
      bool ok = a_ok[g];
      if (p.s_in != 1) {
        ok = ok && (hn % p.s_in == 0) && (wn_ % p.s_in == 0);
        hn /= p.s_in;
        wn_ /= p.s_in;
      }
      ok = ok && ((unsigned)hn < (unsigned)p.Hi) && ((unsigned)wn_ < (unsigned)p.Wi);
      a_cur[g] = ok ? (uint32_t)((a_img[g] + hn * p.Wi + wn_) * p.ldx) * 2u + (uint32_t)(lslot_log * 16) : kOOB;
    }
#pragma unroll
    for (int g = 0; g < GB; ++g) b_cur[g] = b_rowoff[g] + (uint32_t)tap * tap_bytes;     // (kOOB rows stay out of range)
    chunks_left = p.ktiles_per_tap;
  };
  typedef __attribute__((address_space(3))) void* lds_ptr;
  auto issue_c = [&](auto stc) {
    constexpr int ST = decltype(stc)::value;
    if (chunks_left == 0) open_tap();
    unsigned* sb = ldsw + ST * kStageDw;
#pragma unroll
    for (int g = 0; g < GA; ++g)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(xr, (lds_ptr)(sb + kA + RPG * (wave + NW * g) * RDW), 16, (int)a_cur[g], 0, 0, 0);
#pragma unroll
    for (int g = 0; g < GB; ++g)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(wr, (lds_ptr)(sb + kB + RPG * b_grp[g] * RDW), 16, (int)b_cur[g], 0, 0, 0);
#pragma unroll
    for (int g = 0; g < GA; ++g) a_cur[g] += (uint32_t)(KB * 2);
#pragma unroll
    for (int g = 0; g < GB; ++g) b_cur[g] += (uint32_t)(KB * 2);
    --chunks_left;
  };

  // ---- compute side
  f32x16 acc[TM][TN];
  const int frag_row = lane & 31, frag_h = lane >> 5;
  auto swz = [&](int row, int slot) -> int { return row * RDW + ((slot ^ fsw(row)) << 2); };
  constexpr int HK = KB / 32;
  f32x4 fa[2][HK * TM], fb[2][HK * TN];
  int fa_off[2 * HK], fb_off[2 * HK];
#pragma unroll
  for (int q = 0; q < 2 * HK; ++q) {
    fa_off[q] = kA + swz(wm * WTM + frag_row, 2 * q + frag_h);
    fb_off[q] = kB + swz(wn * WTN + frag_row, 2 * q + frag_h);
  }
  auto read_c = [&](auto stc, auto setc, auto halfc) {
    constexpr int ST = decltype(stc)::value, SET = decltype(setc)::value, HALF = decltype(halfc)::value;
    const float* sb = lds + ST * kStageDw;
#pragma unroll
    for (int gg = 0; gg < HK; ++gg) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
        fa[SET][gg * TM + i] = *reinterpret_cast<const f32x4*>(&sb[fa_off[HALF * HK + gg] + i * 32 * RDW]);
#pragma unroll
      for (int j = 0; j < TN; ++j)
        fb[SET][gg * TN + j] = *reinterpret_cast<const f32x4*>(&sb[fb_off[HALF * HK + gg] + j * 32 * RDW]);
    }
  };
  auto mfmas = [&](int set) {
#pragma unroll
    for (int gg = 0; gg < HK; ++gg)
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8v, fa[set][gg * TM + i]),
                                                             __builtin_bit_cast(f16x8v, fb[set][gg * TN + j]), acc[i][j],
                                                             0, 0, 0);
  };

  // ---- epilogue of one tile: transposed fp16 patch, fused BatchNorm statistics of the values as stored
  unsigned char* patch = lds_raw + kRingB + wave * kPatchB;
  const int col_l = lane & 31, hh = lane >> 5;
  const int g16 = lane >> 4, i16 = lane & 15, tqq = i16 >> 2, tpp = i16 & 3;
  const uint32_t tr_addr = lds_addr_of(patch + (8 * g16 + tqq) * kPitch + 8 * tpp);   // block (patch rows 8 g16 + qq, columns 4 pp ..)
  auto epilogue = [&](int cm0, int cn0, int ctile_m) {
    half_t* out = reinterpret_cast<half_t*>(p.y);
    const bool full = cm0 + BM <= p.M;
    const long long gsz = (long long)p.stat_rows * p.N;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int col0 = cn0 + wn * WTN + j * 32;
      float k0 = 0.f, s1 = 0.f, s2 = 0.f;
      // BNS (see store_row32): this lane stores channels col0 + 8 g16 .. + 7 of rows row0 + i16 and row0 + 16 + i16
      const bool bns_cok = col0 + 8 * g16 < p.N;
      HBnsCoef bc;
      HBnsSums bs;
      f16x8v ypre[TM][2];
      if constexpr (BNS) {
        bns_load_coef(p, col0 + 8 * g16, bns_cok, bc);
#pragma unroll
        for (int h = 0; h < 2; ++h) bs.s1[h] = bs.s2[h] = f32x4{0.f, 0.f, 0.f, 0.f};
        // the rows of y this lane will need, requested before the accumulators make their way through the patch
        const half_t* yb = reinterpret_cast<const half_t*>(p.bns_y) + col0 + 8 * g16;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int hb = 0; hb < 2; ++hb) {
            const int row = cm0 + wm * WTM + i * 32 + 16 * hb + i16;
            ypre[i][hb] = f16x8v{0, 0, 0, 0, 0, 0, 0, 0};
            if (row < p.M && bns_cok) ypre[i][hb] = *reinterpret_cast<const f16x8v*>(yb + (long long)row * p.bns_ldy);
          }
      }
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int row0 = cm0 + wm * WTM + i * 32;
        // accumulator registers 4q .. 4q + 3 are rows 8q + 4h + 0 .. 3 of column (lane & 31)
        f16x4v hq[4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int e = 0; e < 4; ++e) hq[q][e] = (half_t)acc[i][j][4 * q + e];
#pragma unroll
        for (int q = 0; q < 4; ++q) *reinterpret_cast<f16x4v*>(patch + col_l * kPitch + (8 * q + 4 * hh) * 2) = hq[q];
        if (p.stat != nullptr) {
          if (i == 0) k0 = __shfl((float)hq[0][0], lane & 31, 64);
          if (full) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const float d = (float)hq[q][e] - k0;
                s1 += d;
                s2 += d * d;
              }
          } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
              for (int e = 0; e < 4; ++e)
                if (row0 + 8 * q + 4 * hh + e < p.M) {
                  const float d = (float)hq[q][e] - k0;
                  s1 += d;
                  s2 += d * d;
                }
          }
        }
        // (the patch is private to this wave and LDS executes a wave's instructions in order: the writes are visible to the
        // reads below once they have been counted out -- no fence, which would also wait for the operand DMAs of the NEXT tile
        // that are in flight by design)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
        // ds_read_b64_tr_b16 per 16-lane group: the block of 4 patch rows (= output columns 8 g16 + [0, 4) or + [4, 8)) x 16
        // patch columns (= output rows r0 .. r0 + 15); lane 4 qq + pp supplies (patch row qq, columns 4 pp ..), lane i16 receives
        // output row r0 + i16, the four columns.  Two reads = 8 consecutive channels = one 16-byte store; the four lane groups
        // cover the four channel octets of a row: 64 contiguous bytes per output row and instruction.
        {
          const s16x4t lo0 = tr_read_asm<0>(tr_addr), hi0 = tr_read_asm<4 * kPitch>(tr_addr);
          const s16x4t lo1 = tr_read_asm<32>(tr_addr), hi1 = tr_read_asm<4 * kPitch + 32>(tr_addr);
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          __builtin_amdgcn_sched_barrier(0);
          const int col = col0 + 8 * g16;
          const int row_a = row0 + i16, row_b = row0 + 16 + i16;
          const s16x8g va = s16x8g{lo0[0], lo0[1], lo0[2], lo0[3], hi0[0], hi0[1], hi0[2], hi0[3]};
          const s16x8g vb = s16x8g{lo1[0], lo1[1], lo1[2], lo1[3], hi1[0], hi1[1], hi1[2], hi1[3]};
          if (row_a < p.M && col < p.N) *reinterpret_cast<s16x8g*>(out + (long long)row_a * p.ldy + col) = va;
          if (row_b < p.M && col < p.N) *reinterpret_cast<s16x8g*>(out + (long long)row_b * p.ldy + col) = vb;
          if constexpr (BNS) {
            if (row_a < p.M && bns_cok) bns_add8(__builtin_bit_cast(f16x8v, va), ypre[i][0], p.bns_act, bc, bs);
            if (row_b < p.M && bns_cok) bns_add8(__builtin_bit_cast(f16x8v, vb), ypre[i][1], p.bns_act, bc, bs);
          }
        }
        __builtin_amdgcn_wave_barrier();      // (the patch is rewritten by the next tile: its reads above have been waited for)
      }
      if constexpr (BNS) {
#pragma unroll
        for (int o = 1; o < 16; o <<= 1)
#pragma unroll
          for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              bs.s1[h][e] += __shfl_xor(bs.s1[h][e], o, 64);
              bs.s2[h][e] += __shfl_xor(bs.s2[h][e], o, 64);
            }
        if (i16 == 0 && bns_cok) {
          const long long o = (long long)(ctile_m * WARPS_M + wm) * p.N + col0 + 8 * g16;
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            *reinterpret_cast<f32x4*>(p.bns_db + o + 4 * h) = bs.s1[h];
            *reinterpret_cast<f32x4*>(p.bns_dg + o + 4 * h) = bs.s2[h];
          }
        }
      }
      if (p.stat != nullptr) {
        s1 += __shfl_xor(s1, 32, 64);
        s2 += __shfl_xor(s2, 32, 64);
        const int col = col0 + col_l;
        if (lane < 32 && col < p.N) {
          const long long o = (long long)(ctile_m * WARPS_M + wm) * p.N + col;
          p.stat[o] = k0;
          p.stat[gsz + o] = s1;
          p.stat[2 * gsz + o] = s2;
        }
      }
    }
  };

  const int n_steps = p.ntaps * p.ktiles_per_tap;
  typedef std::integral_constant<int, 0> c0;
  typedef std::integral_constant<int, 1> c1;
  typedef std::integral_constant<int, 2> c2;
  issue_c(c0{});
  issue_c(c1{});
  if constexpr (STAGES >= 3) issue_c(c2{});
  wait_vmcnt<(STAGES - 1) * NG>();   // step 0 has landed (this wave's share); STAGES - 1 steps stay in flight
  __builtin_amdgcn_s_barrier();      // ... and everybody's
  read_c(c0{}, c0{}, c0{});
#define PSEG_GHP_STEP(S)                                                                                         \
  {                                                                                                              \
    typedef std::integral_constant<int, (S)> cs;                                                                 \
    typedef std::integral_constant<int, ((S) + 1) % STAGES> cs1;                                                 \
    read_c(cs{}, c1{}, c1{});                                                                                    \
    __builtin_amdgcn_sched_barrier(0);                                                                           \
    mfmas(0);                                                                                                    \
    __builtin_amdgcn_sched_barrier(0);                                                                           \
    wait_vmcnt<(STAGES - 2) * NG>();                   /* the next step has landed; STAGES - 2 more in flight */  \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); /* this wave is done reading stage S */                   \
    __builtin_amdgcn_s_barrier();                                                                                \
    read_c(cs1{}, c0{}, c0{});                         /* (the next TILE's first step at a tile boundary) */     \
    __builtin_amdgcn_sched_barrier(0);                                                                           \
    issue_c(cs{});                                     /* stage S is free now */                                 \
    mfmas(1);                                                                                                    \
    __builtin_amdgcn_sched_barrier(0);                                                                           \
  }
#define PSEG_GHP_CASE(S)                     \
  case (S):                                  \
    PSEG_GHP_STEP(S)                         \
    if (--left == 0) {                       \
      stage = ((S) + 1) % STAGES;            \
      running = false;                       \
      break;                                 \
    }
  int stage = 0;       // ring phase the next K-step computes from: carried over tile boundaries
  for (int c_vt = (int)blockIdx.x; c_vt < ntiles; c_vt += nblocks) {
    const int t = remap_tile(p.xcd_remap, c_vt, ntiles);
    const int ctile_n = t % gridN, ctile_m = t / gridN;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    int left = n_steps;
    bool running = true;
    while (running) {
      if constexpr (STAGES == 2) {
        switch (stage) {
          PSEG_GHP_CASE(0)
          PSEG_GHP_CASE(1)
        }
      } else {
        switch (stage) {
          PSEG_GHP_CASE(0)
          PSEG_GHP_CASE(1)
          PSEG_GHP_CASE(2)
        }
      }
      if (running) stage = 0;
    }
    epilogue(ctile_m * BM, ctile_n * BN, ctile_m);
  }
#undef PSEG_GHP_CASE
#undef PSEG_GHP_STEP
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // no DMA may land after the block has given its LDS back
}

// ------------------------------------------------------------------------------------------------ filters
// Every dense conv filter of a model in ONE launch, from the fp32 master copy: the fp16 filter [Cout'][taps][Cin'] the
// forward convs read AND its transposed fp16 copy [Cin'][taps][Cout'] for the data gradients.  The fp16 copies may be padded
// further than the master ([Cout][taps][Cin] -> Cout' >= Cout, Cin' >= Cin: 8-channel granules; the padding is zero-filled).
// jobs[j] = {w fp32, w_h, wT_h, Cout, taps, Cin, Cout', Cin', first 32x32 tile of job j} (9 x int64, device memory, tile
// offsets ascending; tiles cover the PADDED extents); block b finds its job by bisection.
__global__ __launch_bounds__(256) void filter_prepare_h_kernel(const long long* __restrict__ jobs, int n) {
  PSEG_HELPER_PRIO();
  __shared__ float tile[32][33];
  const long long b = blockIdx.x;
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[mid * 9 + 8] <= b) lo = mid;
    else hi = mid - 1;
  }
  const long long* job = jobs + lo * 9;
  const float* w = reinterpret_cast<const float*>(job[0]);
  half_t* wh = reinterpret_cast<half_t*>(job[1]);
  half_t* wT = reinterpret_cast<half_t*>(job[2]);
  const int Cout = (int)job[3], taps = (int)job[4], Cin = (int)job[5], CoutP = (int)job[6], CinP = (int)job[7];
  const int tci = (CinP + 31) / 32, tco = (CoutP + 31) / 32;
  int local = (int)(b - job[8]);
  const int t = local / (tci * tco);
  local -= t * tci * tco;
  if (t >= taps) return;
  const int co0 = (local / tci) * 32, ci0 = (local % tci) * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8) {
    const int co = co0 + r, ci = ci0 + tx;
    float v = 0.f;
    if (co < Cout && ci < Cin) v = w[((long long)co * taps + t) * Cin + ci];
    if (wh != nullptr && co < CoutP && ci < CinP) wh[((long long)co * taps + t) * CinP + ci] = (half_t)v;
    tile[r][tx] = v;
  }
  __syncthreads();
  if (wT != nullptr)
    for (int r = ty; r < 32; r += 8) {
      const int ci = ci0 + r, co = co0 + tx;
      if (ci < CinP && co < CoutP) wT[((long long)ci * taps + t) * CoutP + co] = (half_t)tile[tx][r];
    }
}

// strided [M][C] conversion between fp32 and fp16 tensors with an optional multiplier: y = convert(x * scale), where
// scale = *dev_scale (device scalar: the dynamic loss scale) when non-null.  4 channels per lane.
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void convert2d_kernel(const TI* __restrict__ x, int ldx, TO* __restrict__ y, int ldy,
                                                        uint32_t total, FastDiv c4div, const float* __restrict__ dev_scale) {
  PSEG_HELPER_PRIO();
  const float s = dev_scale != nullptr ? *dev_scale : 1.f;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    const uint32_t r = c4div.div(i);
    const uint32_t c = (i - r * c4div.d) * 4;
    stv4(y + (long long)r * ldy + c, ldv4(x + (long long)r * ldx + c) * s);
  }
}

// ------------------------------------------------------------------------------------------------ host side
// The tiles of the fp16 gather kernels, stated once: select_gather_h picks an entry, the launch helpers map it to template
// arguments.  Which (entry, K-step, ring depth) is instantiated is said by the constexpr predicates below and nowhere else: the
// selection calls them at run time, the launch helpers in `if constexpr`.  Threads per block = 64 * wm * wn; the wm wave rows are
// the statistics groups of a row tile.
struct HTile {
  int bm, bn, wm, wn;
  bool persistent;   // gather_hp_kernel is instantiated for it
  int bns_kb;        // K-steps (32 | 64) with which it carries the fused BatchNorm-backward sums: the tiles the Bottleneck and
                     // BasicBlock data gradients of the reference's models are planned onto
};
constexpr HTile kHTiles[] = {{128, 128, 2, 4, true, 32 | 64}, {128, 64, 2, 2, true, 32 | 64}, {64, 128, 2, 2, true, 0}, {128, 32, 4, 1, true, 32}};
constexpr int kNumHTiles = (int)(sizeof(kHTiles) / sizeof(kHTiles[0]));

static int h_tile_index(TileCfg t) {
  for (int i = 0; i < kNumHTiles; ++i)
    if (kHTiles[i].bm == t.bm && kHTiles[i].bn == t.bn) return i;
  return -1;
}

// LDS of one block: gather_h_kernel's epilogue patch overlays its ring, gather_hp_kernel keeps a (smaller) patch beside it
constexpr long long h_ring_lds(const HTile& t, int kb, int st) {
  const long long ring = (long long)st * (t.bm + t.bn) * kb * 2, patch = (long long)t.wm * t.wn * 32 * (t.bn / t.wn + 4) * 4;
  return ring > patch ? ring : patch;
}
constexpr long long h_persistent_lds(const HTile& t, int kb, int st) {
  return (long long)st * (t.bm + t.bn) * kb * 2 + (long long)t.wm * t.wn * 32 * 72;
}
// (K-step, ring depth) pairs with a BNS = true instantiation: what the heuristics of select_gather_h give those data gradients
constexpr bool h_bns_steps(int kb, int st, bool persistent) {
  return (kb == 32 && st == 3) || (kb == 64 && (st == 2 || (st == 3 && !persistent)));
}
constexpr bool h_ring_exists(const HTile& t, int kb, int st, bool bns) {
  return h_ring_lds(t, kb, st) <= kLdsBytes &&
         (!bns || ((t.bns_kb & kb) != 0 && h_bns_steps(kb, st, false)));
}
constexpr bool h_persistent_exists(const HTile& t, int kb, int st, bool bns) {      // (its ring is two or three deep)
  return t.persistent && st <= 3 && h_persistent_lds(t, kb, st) <= kLdsBytes &&
         (!bns || ((t.bns_kb & kb) != 0 && h_bns_steps(kb, st, true)));
}

// f(std::integral_constant<int, tile>, HSteps<kb, st>) for a table entry, a K-step (32 / 64) and a ring depth (2 .. 4): the
// entry's fields and the steps are then template arguments
template <int I, typename F>
static void with_h_steps(int kb, int st, F&& f) {
  constexpr std::integral_constant<int, I> tile{};
  if (kb == 32 && st == 2) f(tile, HSteps<32, 2>{});
  else if (kb == 32 && st == 3) f(tile, HSteps<32, 3>{});
  else if (kb == 32) f(tile, HSteps<32, 4>{});
  else if (st == 2) f(tile, HSteps<64, 2>{});
  else if (st == 3) f(tile, HSteps<64, 3>{});
  else f(tile, HSteps<64, 4>{});
}
template <typename F>
static void with_h_kernel(int tile, int kb, int st, F&& f) {
  with_index(tile, [&](auto t) { with_h_steps<decltype(t)::value>(kb, st, f); }, std::make_integer_sequence<int, kNumHTiles>{});
}

// the planner's tile -> one of the default entries of kHTiles
static TileCfg half_tile(TileCfg t) {
  if (t.bm == 256) t.bm = 128;
  if (t.bm == 32) t.bm = 64;
  if (t.bm == 64) t.bn = 128;
  if (t.bm == 128 && !(t.bn == 128 || t.bn == 64 || t.bn == 32)) t.bn = 128;
  return t;
}

// K-step (halves per LDS row) of a gather problem.  PSEG_HCONV_KB = 32 / 64 forces one.
static int hconv_kb(int Cin, int K) {
  const int forced = cfg().hconv_kb;
  if (forced == 32 || forced == 64) return forced;
  if (Cin % 64 != 0) return 32;          // 32-channel layers stay on the hoisted (tap-uniform) addressing with the short step
  // measured (tools/bench_conv_half.py over PSEG_HCONV_KB x PSEG_HCONV_STAGES): the short step with a three-deep ring wins
  // 5-20 % on the bandwidth-bound layers with K <= 576 (64 -> 256 channels on 128x128 maps: 40 vs 52 us against an HBM floor of
  // 31; 3x3 on 64 channels 42 vs 45) and loses 10-25 % on the deep contractions (layer-2..4 3x3, ASPP)
  return K <= 576 ? 32 : 64;
}

// A gather problem as run_gather_h sees it: the geometry plus what the caller asks of the kernel.
struct HGatherProblem : GatherGeom {
  bool y_f32, bias, stats, accumulate, bns;   // fp32 result / bias / fused statistics / y += / fused BatchNorm-backward sums
};

// Everything run_gather_h decides before it launches; the queries read their answers off the same choice.
struct HGatherChoice {
  FwdPlan pl;       // (never split-K)
  RowOrder order;
  int tile;         // entry of kHTiles; -1: a forced tile that nothing is instantiated for
  int kb, stages;   // K-step and ring depth of gather_h_kernel
  int variant;      // 0 plain, 1 tap-skipping, 2 GENERIC (channels off the K-step grid)
  bool persistent;  // gather_hp_kernel is offered the problem first (and is instantiated for it, with the sums if asked) ...
  int pstages;      // ... with a ring this deep
  bool ring;        // the gather_h_kernel instantiation exists (with the sums if asked)
  bool sums;        // the fused sums are asked for and a kernel that carries them takes the problem
  int wave_rows() const { return tile >= 0 ? kHTiles[tile].wm : 2; }
  int stat_rows() const { return pl.gridM * wave_rows(); }
};

// The one place that picks the kernel of an fp16 gather conv.  Pure: launches nothing, touches no device.
static HGatherChoice select_gather_h(const HGatherProblem& q) {
  HGatherChoice c;
  const long long M = q.M;
  const int N = q.N, K = q.K;
  const int kb = c.kb = hconv_kb(q.Cin, K);
  const bool generic = q.Cin % kb != 0;
  // the plan: tile and row order from the shared planner (the schedules of the dilated convs carry over), never split-K.
  // Dilated convs: the tap-skipping schedules (patch / class-sorted rows, 64-row candidate tiles) are only searched when the
  // plain plan lands on a 4-wave tile; a 128x128 / 8-wave problem runs dense and row-major (see below)
  DilGeom geom;
  const bool has_geom = !generic && dil_geom(geom, q.Ho, q.Wo, q.Hi, q.Wi, q.taps_h, q.taps_w, q.Cin, q.s_out, q.s_in, q.dstep, q.off0);
  FwdPlan& pl = c.pl;
  pl = plan_gather(M, N, K, false, nullptr);
  if (has_geom && !(pl.tile.bm == 128 && pl.tile.bn == 128)) pl = plan_gather(M, N, K, false, &geom);
  // one 128x128 block per CU beats two 128x64 blocks on the fp16 kernels when the problem has no dead taps to skip (round 4:
  // M = 16384 x N = 256, K = 2304 -- layer 3's 3x3 convs -- 32 -> 28 us, 26 on the persistent kernel): the kernels are bound by
  // the bytes a CU pulls through its LDS-DMA path, and the wider tile pulls a third fewer of them per MAC
  if (!has_geom && pl.tile.bm == 128 && pl.tile.bn == 64 && N >= 128 && K >= 1024 &&
      (long long)cdiv(M, 128) * cdiv(N, 128) >= 256 && cfg().conv_bm == 0)
    pl.tile.bn = 128;
  TileCfg t = half_tile(pl.tile);
  // (a substituted tile keeps the plain row order: patch / class schedules were costed for the planner's own tile)
  if (t.bm != pl.tile.bm) {
    pl.patch_h = pl.patch_w = 0;
    pl.banded = false;
  }
  c.tile = h_tile_index(t);
  pl.tile = t;
  pl.gridM = cdiv(M, t.bm);
  pl.gridN = cdiv(N, t.bn);
  pl.splits = 1;
  pl.kt_total = pl.kt_per_split = cdiv(K, kb);
  // dilated convs: K-steps of taps that are zero padding for the whole M tile are skipped -- on the 4-wave tiles only.  On the
  // 128x128 / 8-wave tile (the ASPP data gradients: N = 2048) the tap-skipping instantiation is SLOWER than the dense one
  // even where it skips half the K-steps (rate 18: 269 us patch-ordered / 290 class-sorted against 168 dense; rate 6: 272
  // against 206): one fp16 MFMA pass per tile leaves the kernel bound by its operand stream, a padding tap's DMA is an
  // out-of-range no-op that costs nothing, and the skip bookkeeping does (tools/bench_conv_half.py with PSEG_CONV_NOSKIP=1).
  // The stride-2 data gradient runs parity-homogeneous tiles on every tile shape, 3/4 of the taps skipped.
  c.order = gather_row_order(q, pl, !generic && !(t.bm == 128 && t.bn == 128), !generic);
  c.variant = generic ? 2 : (c.order.skip_taps != 0 ? 1 : 0);
  // ring depth (PSEG_HCONV_STAGES forces 2 / 3 / 4); never deeper than the K loop is long
  // Measured: the short K-step always wants three stages (its blocks are small: four to eight stay resident anyway); the long
  // one only on narrow tiles with a deep contraction, where a deeper ring costs no resident block the grid needs -- the ASPP
  // convs (128x64 tiles, K = 18432: 237 -> 197 / 208 -> 151 us with three stages) and the classifier (128x32, K = 3456: 238 ->
  // 158 us with four); 128x128 tiles lose their second resident block to a third stage (layer-4 3x3: 89 -> 98 us).
  const int forced_stages = cfg().hconv_stages;
  int stages = 2;
  if (kb == 32) stages = 3;
  else if (t.bn == 32 && K >= 2048) stages = 4;
  else if (t.bn == 64 && t.bm == 128 && K >= 2048) stages = 3;
  if (forced_stages >= 2 && forced_stages <= 4) stages = forced_stages;
  if (pl.kt_total < stages) stages = pl.kt_total < 2 ? 2 : pl.kt_total;
  c.stages = stages;
  c.pstages = stages >= 3 ? 3 : 2;
  // the persistent kernel (gather_hp_kernel) takes the launches it covers; PSEG_HCONV_PERSIST=0 keeps everything on
  // gather_h_kernel (A/B runs)
  // ... where it pays: SHORT contractions (measured, tools/bench_conv_half.py with PSEG_HCONV_PERSIST=0/1: K <= 1280 -- 2 to 20
  // K-steps per tile -- 5-20 % faster, e.g. 64 -> 256 channels on 128x128 maps 41 -> 35 us = 4.8 TB/s of operand + result
  // traffic; the deep contractions lose 15-25 %: ring + patch leave one resident block per CU where gather_h_kernel holds two,
  // and with 32+ K-steps per tile there is no chain left to hide).  PSEG_HCONV_PERSIST=2 forces it everywhere it is valid.
  constexpr int kPersistMaxKSteps = 24;
  const int persist = cfg().hconv_persist;
  const bool offered = persist != 0 && c.variant == 0 && !q.y_f32 && !q.bias && !q.accumulate &&
                       (c.order.row_perm == 0 || c.order.row_perm == 3) && pl.kt_total >= 1 &&
                       (pl.kt_total <= kPersistMaxKSteps || persist == 2 || (pl.gridM * pl.gridN <= 256 && pl.kt_total <= 48));
  c.persistent = offered && c.tile >= 0 && h_persistent_exists(kHTiles[c.tile], kb, c.pstages, q.bns);
  // (the sums come with the plain variant only: every tap live, channels in whole K-steps)
  c.ring = c.tile >= 0 && h_ring_exists(kHTiles[c.tile], kb, stages, q.bns) && !(q.bns && c.variant != 0);
  c.sums = q.bns && !q.y_f32 && !q.bias && !q.stats && !q.accumulate && (c.persistent || c.ring);
  return c;
}

// the gather_h_kernel instantiation of a choice (c.ring says that it exists)
static void launch_ring_h(const HGatherChoice& c, bool bns, hipStream_t st, const HGatherParams& hp) {
  const dim3 grid((unsigned)(c.pl.gridM * c.pl.gridN), 1, 1);
  with_h_kernel(c.tile, c.kb, c.stages, [&](auto tile, auto steps) {
    constexpr HTile t = kHTiles[decltype(tile)::value];
    constexpr int KB = decltype(steps)::kb, ST = decltype(steps)::st;
    if constexpr (h_ring_exists(t, KB, ST, false)) {
      const dim3 block(64 * t.wm * t.wn);
      if (bns) {
        if constexpr (h_ring_exists(t, KB, ST, true))
          hipLaunchKernelGGL((gather_h_kernel<t.bm, t.bn, t.wm, t.wn, false, false, KB, ST, true>), grid, block, 0, st, hp);
      } else if (c.variant == 2) hipLaunchKernelGGL((gather_h_kernel<t.bm, t.bn, t.wm, t.wn, false, true, KB, ST>), grid, block, 0, st, hp);
      else if (c.variant == 1) hipLaunchKernelGGL((gather_h_kernel<t.bm, t.bn, t.wm, t.wn, true, false, KB, ST>), grid, block, 0, st, hp);
      else hipLaunchKernelGGL((gather_h_kernel<t.bm, t.bn, t.wm, t.wn, false, false, KB, ST>), grid, block, 0, st, hp);
    }
  });
}

// one instantiation of the persistent kernel; grid = min(tiles, CUs x resident blocks per CU).  false: the device does not say
// how many blocks it holds
template <int BM, int BN, int WM, int WN, int KB, int ST, bool BNS>
static bool launch_gather_hp_one(int ntiles, hipStream_t st, const HGatherParams& hp) {
  constexpr int NW = WM * WN;
  static int resident = 0;      // blocks of this instantiation the device holds at once
  if (resident == 0) {
    int per_cu = 0, dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, gather_hp_kernel<BM, BN, WM, WN, KB, ST, BNS>, 64 * NW, 0) != hipSuccess ||
        per_cu < 1)
      return false;
    const int by_lds = (int)(kLdsBytes / h_persistent_lds(HTile{BM, BN, WM, WN, true, 0}, KB, ST));
    if (per_cu > by_lds) per_cu = by_lds;
    resident = prop.multiProcessorCount * per_cu;
  }
  const int blocks = ntiles < resident ? ntiles : resident;
  hipLaunchKernelGGL((gather_hp_kernel<BM, BN, WM, WN, KB, ST, BNS>), dim3((unsigned)blocks), dim3(64 * NW), 0, st, hp);
  return true;
}

// the gather_hp_kernel instantiation of a choice (c.persistent says that it exists)
static bool launch_persistent_h(const HGatherChoice& c, bool bns, hipStream_t st, const HGatherParams& hp) {
  bool ok = false;
  with_h_kernel(c.tile, c.kb, c.pstages, [&](auto tile, auto steps) {
    constexpr HTile t = kHTiles[decltype(tile)::value];
    constexpr int KB = decltype(steps)::kb, ST = decltype(steps)::st;
    if constexpr (h_persistent_exists(t, KB, ST, false)) {
      if (bns) {
        if constexpr (h_persistent_exists(t, KB, ST, true)) ok = launch_gather_hp_one<t.bm, t.bn, t.wm, t.wn, KB, ST, true>(hp.ntiles, st, hp);
      } else {
        ok = launch_gather_hp_one<t.bm, t.bn, t.wm, t.wn, KB, ST, false>(hp.ntiles, st, hp);
      }
    }
  });
  return ok;
}

// What the kernels' 32-bit row indices and buffer addressing cap, for the launch and the fused-sums query alike: nullptr, or
// what is wrong with the sizes of a problem whose source tensor spans x_bytes and whose result has the row stride ldy.
static const char* gather_size_error_h(const GatherGeom& g, long long x_bytes, int ldy) {
  if (!(g.M > 0 && g.M < (1LL << 31) && g.N > 0 && g.K > 0)) return "empty or oversized problem";
  if (!(x_bytes < kMaxBytes && (long long)g.N * g.K * 2 < kMaxBytes)) return "x or w exceeds 2 GiB";
  if (!(((g.M - 1) * ldy + g.N) * 4 < (1LL << 40))) return "output too large";
  return nullptr;
}

// the instantiation the calling thread's last launch of run_gather_h ran (pseg_debug_last_gather_h): tile rows, tile columns,
// K-step, ring depth as launched, variant, fused sums
static thread_local int g_last_gather_h[6] = {0, 0, 0, 0, 0, 0};
static void note_gather_h(const HGatherChoice& c, int depth, bool bns) {
  const int rec[6] = {c.pl.tile.bm, c.pl.tile.bn, c.kb, depth, c.variant, bns ? 1 : 0};
  for (int i = 0; i < 6; ++i) g_last_gather_h[i] = rec[i];
}

// validate, select, fill the parameters from the choice and launch
static int run_gather_h(const GatherGeom& g, const void* x, long long x_bytes, int ldx, const void* w, void* y, int ldy, int y_f32,
                        const float* bias, float* stat, int accumulate, hipStream_t st, const BnsArgs* bns = nullptr) {
  const char* size_error = gather_size_error_h(g, x_bytes, ldy);
  PSEG_REQUIRE(size_error == nullptr, "conv_h: %s (M=%lld N=%d K=%d, x %lld bytes, ldy %d)", size_error, g.M, g.N, g.K, x_bytes, ldy);
  PSEG_REQUIRE(g.Cin % 8 == 0 && ldx % 8 == 0 && g.N % 8 == 0, "conv_h: Cin (%d), ldx (%d) and the output channels (%d) must be multiples of 8",
               g.Cin, ldx, g.N);
  PSEG_REQUIRE(ldy % (y_f32 ? 4 : 8) == 0 && ldy >= g.N, "conv_h: ldy (%d) must cover N and be a multiple of %d", ldy, y_f32 ? 4 : 8);
  PSEG_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)w & 15) == 0 && ((uintptr_t)y & 15) == 0, "conv_h: x / w / y must be 16-byte aligned");
  PSEG_REQUIRE(bns == nullptr || (!y_f32 && bias == nullptr && !accumulate && stat == nullptr),
               "conv_h: the fused BatchNorm-backward sums need an fp16 result without bias / accumulation / statistics");

  const HGatherChoice c = select_gather_h(HGatherProblem{g, y_f32 != 0, bias != nullptr, stat != nullptr, accumulate != 0, bns != nullptr});
  const FwdPlan& pl = c.pl;
  PSEG_REQUIRE(bns == nullptr || bns->rows == c.stat_rows(), "conv_h: %d partial rows handed in, the plan has %d",
               bns == nullptr ? 0 : bns->rows, c.stat_rows());

  HGatherParams hp{};      // (everything a gather conv of this kind does not use stays null / zero)
  GatherConvParams& p = hp.g;
  p.x = reinterpret_cast<const float*>(x);
  p.w = reinterpret_cast<const float*>(w);
  p.y = reinterpret_cast<float*>(y);
  p.ldy = ldy;
  p.bias = bias;
  p.stat = stat;
  p.stat_rows = c.stat_rows();
  p.x_bytes = (uint32_t)x_bytes;
  p.w_bytes = (uint32_t)((long long)g.N * g.K * 2);
  p.ldx = ldx;
  p.accumulate = accumulate;
  p.ktiles_per_tap = c.variant == 2 ? 1 : g.Cin / c.kb;
  set_gather_geometry(p, g, pl, c.order);
  set_bns_params(p, bns);
  hp.y_f32 = y_f32;
  hp.cin_div = FastDiv((uint32_t)g.Cin);
  hp.kw_div = FastDiv((uint32_t)g.taps_w);
  hp.howo_div = FastDiv((uint32_t)p.HoWo);      // (after the pointwise rewrite of set_gather_geometry: HoWo = Wo = M there)
  hp.wo_div = FastDiv((uint32_t)p.Wo);
  hp.ntiles = pl.gridM * pl.gridN;
  if (c.persistent && launch_persistent_h(c, bns != nullptr, st, hp)) {
    g_last_conv_kernel = PSEG_KERNEL_GATHER_H_PERSISTENT;
    note_gather_h(c, c.pstages, bns != nullptr);
    PSEG_LAUNCH_CHECK();
    return PSEG_OK;
  }
  if (!c.ring) {
    set_error("conv_h: no kernel for tile %dx%d (K-step %d, %d stages)%s", pl.tile.bm, pl.tile.bn, c.kb, c.stages,
              bns != nullptr ? " with the fused BatchNorm-backward sums" : "");
    return PSEG_ERR_ARG;
  }
  launch_ring_h(c, bns != nullptr, st, hp);
  g_last_conv_kernel = PSEG_KERNEL_GATHER_H;
  note_gather_h(c, c.stages, bns != nullptr);
  PSEG_LAUNCH_CHECK();
  return PSEG_OK;
}

}  // namespace pseg

using namespace pseg;

extern "C" {

// the choice of a forward conv with fused statistics (the queries know Ho / Wo only: the smallest input that gives them)
static HGatherChoice select_fwd_stats_h(int B, int Ho, int Wo, int Cin, int Cout, int kh, int kw, int stride, int pad, int dil) {
  return select_gather_h(HGatherProblem{fwd_stats_geom(B, Ho, Wo, Cin, Cout, kh, kw, stride, pad, dil), false, false, true, false, false});
}

int pseg_conv2d_stat_rows_h(int B, int Ho, int Wo, int Cin, int Cout, int kh, int kw, int stride, int pad, int dil) {
  return select_fwd_stats_h(B, Ho, Wo, Cin, Cout, kh, kw, stride, pad, dil).stat_rows();
}

int pseg_conv2d_stat_group_h(int B, int Ho, int Wo, int Cin, int Cout, int kh, int kw, int stride, int pad, int dil) {
  const HGatherChoice c = select_fwd_stats_h(B, Ho, Wo, Cin, Cout, kh, kw, stride, pad, dil);
  return c.pl.tile.bm / c.wave_rows();
}

int pseg_conv2d_fwd_h(const pseg_half_t* x, int ldx, const pseg_half_t* w, const float* bias, void* y, int ldy, int y_is_f32,
                      int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad, int dil,
                      int accumulate, float* stat, void* stream) {
  PSEG_REQUIRE(x && w && y, "conv2d_fwd_h: null pointer");
  const int rc = check_fwd_geometry("conv2d_fwd_h", H, W, Ho, Wo, kh, kw, stride, pad, dil);
  if (rc != PSEG_OK) return rc;
  return run_gather_h(fwd_geom(B, H, W, Cin, Ho, Wo, Cout, kh, kw, stride, pad, dil), x, nhwc_bytes_h(B, H, W, Cin, ldx), ldx, w, y,
                      ldy, y_is_f32, bias, stat, accumulate, (hipStream_t)stream);
}

int pseg_conv2d_dgrad_h(const pseg_half_t* dy, int ldy, const pseg_half_t* wT, pseg_half_t* dx, int ldx, int B, int H, int W,
                        int Cin, int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad, int dil, int accumulate,
                        void* stream) {
  PSEG_REQUIRE(dy && wT && dx, "conv2d_dgrad_h: null pointer");
  PSEG_REQUIRE(stride >= 1 && dil >= 1 && pad >= 0, "conv2d_dgrad_h: bad geometry");
  return run_gather_h(dgrad_geom(B, H, W, Cin, Ho, Wo, Cout, kh, kw, stride, pad, dil), dy, nhwc_bytes_h(B, Ho, Wo, Cout, ldy), ldy,
                      wT, dx, ldx, 0, nullptr, nullptr, accumulate, (hipStream_t)stream);
}

int pseg_conv2d_dgrad_bnstat_rows_h(int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad,
                                    int dil) {
  if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || kh <= 0 || kw <= 0 || Cin % 8 != 0 || Cout % 8 != 0 || stride < 1 ||
      dil < 1 || pad < 0)
    return 0;
  // the problem pseg_conv2d_dgrad_bnstat_h hands to run_gather_h (densely packed): 0 where the launch refuses its sizes or no
  // kernel that carries the fused sums takes it
  const GatherGeom g = dgrad_geom(B, H, W, Cin, Ho, Wo, Cout, kh, kw, stride, pad, dil);
  if (gather_size_error_h(g, nhwc_bytes_h(B, Ho, Wo, Cout, Cout), Cin) != nullptr) return 0;
  const HGatherChoice c = select_gather_h(HGatherProblem{g, false, false, false, false, true});
  return c.sums ? c.stat_rows() : 0;
}

int pseg_conv2d_dgrad_bnstat_h(const pseg_half_t* dy, int ldy, const pseg_half_t* wT, pseg_half_t* dx, int ldx, int B, int H, int W,
                               int Cin, int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad, int dil,
                               const pseg_half_t* y_prev, int ldy_prev, const float* mean, const float* invstd, const float* scale,
                               const float* shift, int act, float* part_db, float* part_dg, int part_rows, void* stream) {
  const BnsArgs bns{y_prev, ldy_prev, mean, invstd, scale, shift, act, part_db, part_dg, part_rows};
  const int rc = check_dgrad_bnstat_args("conv2d_dgrad_bnstat_h", 8, dy, wT, dx, Cin, stride, pad, dil, bns);
  if (rc != PSEG_OK) return rc;
  PSEG_REQUIRE(part_rows > 0 && part_rows == pseg_conv2d_dgrad_bnstat_rows_h(B, H, W, Cin, Ho, Wo, Cout, kh, kw, stride, pad, dil),
               "conv2d_dgrad_bnstat_h: part_rows (%d) is not pseg_conv2d_dgrad_bnstat_rows_h() of this problem", part_rows);
  return run_gather_h(dgrad_geom(B, H, W, Cin, Ho, Wo, Cout, kh, kw, stride, pad, dil), dy, nhwc_bytes_h(B, Ho, Wo, Cout, ldy), ldy,
                      wT, dx, ldx, 0, nullptr, nullptr, 0, (hipStream_t)stream, &bns);
}

int pseg_debug_last_gather_h(int* out6) {
  PSEG_REQUIRE(out6 != nullptr, "debug_last_gather_h: null pointer");
  for (int i = 0; i < 6; ++i) out6[i] = g_last_gather_h[i];
  return PSEG_OK;
}

int pseg_filter_prepare_h(const int64_t* jobs, int n, int64_t total_tiles, void* stream) {
  PSEG_REQUIRE(jobs && n > 0 && total_tiles > 0 && total_tiles < (1LL << 31), "filter_prepare_h: bad argument");
  hipLaunchKernelGGL(filter_prepare_h_kernel, dim3((unsigned)total_tiles), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const long long*>(jobs), n);
  PSEG_LAUNCH_CHECK();
  return PSEG_OK;
}

int pseg_convert2d(const void* x, int x_is_half, int ldx, void* y, int y_is_half, int ldy, int64_t M, int C,
                   const float* dev_scale, void* stream) {
  PSEG_REQUIRE(x && y && M > 0 && C > 0 && C % 4 == 0, "convert2d: need M > 0, C %% 4 == 0");
  PSEG_REQUIRE(ldx % 4 == 0 && ldy % 4 == 0 && ldx >= C && ldy >= C, "convert2d: ld %% 4 == 0, ld >= C");
  PSEG_REQUIRE((((uintptr_t)x | (uintptr_t)y) & 7) == 0, "convert2d: alignment");
  PSEG_REQUIRE((long long)M * (C / 4) < (1LL << 31), "convert2d: tensor too large");
  const uint32_t total = (uint32_t)(M * (C / 4));
  long long blocks = ((long long)total + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  const FastDiv c4((uint32_t)(C / 4));
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)blocks), block(256);
  if (x_is_half && y_is_half)
    hipLaunchKernelGGL((convert2d_kernel<half_t, half_t>), grid, block, 0, st, (const half_t*)x, ldx, (half_t*)y, ldy, total, c4, dev_scale);
  else if (x_is_half)
    hipLaunchKernelGGL((convert2d_kernel<half_t, float>), grid, block, 0, st, (const half_t*)x, ldx, (float*)y, ldy, total, c4, dev_scale);
  else if (y_is_half)
    hipLaunchKernelGGL((convert2d_kernel<float, half_t>), grid, block, 0, st, (const float*)x, ldx, (half_t*)y, ldy, total, c4, dev_scale);
  else
    hipLaunchKernelGGL((convert2d_kernel<float, float>), grid, block, 0, st, (const float*)x, ldx, (float*)y, ldy, total, c4, dev_scale);
  PSEG_LAUNCH_CHECK();
  return PSEG_OK;
}

}  // extern "C"
