// Half-precision (`-mp`) weight gradient for gfx950: fp16 activations and gradients in HBM, single-pass
// v_mfma_f32_32x32x16_f16 with fp32 accumulation into fp32 slabs.  Forward and data gradient are conv_half_gather.hip;
// conv_half.h holds what the two share.
//
//  wgrad_h_kernel    weight gradient: dW[Cout][K] = dY[P][Cout]^T * A[P][K], contraction over pixels.  Both operands lie
//     pixel-major in memory ([pixel][channels]) and are DMA'd as they lie into [64 px][cols] LDS images; the MFMA wants 8
//     consecutive k (= pixels) of one channel per lane, which `ds_read_b64_tr_b16` delivers from the pixel-major image (a
//     4-pixel x 16-channel block per 16 lanes, transposed on the way out).  16-byte chunks are XOR-swizzled by the pixel
//     row (on the source side of the DMA) so that the four rows of a block fall on different banks.  fp32 slabs per pixel
//     split, reduced in a fixed order by the same slab kernels as the fp32 path (bit-reproducible).
#include "conv_half.h"

namespace pseg {

struct HWgradParams {
  WgradParams g;           // x / dy are fp16 here
  FastDiv howo_div, wo_div;
};

// chunk swizzle of the pixel-major LDS images: XOR of the 16-byte chunk index of pixel row `row`, by row length

template <int ROWBYTES>
__device__ __forceinline__ int wg_swz(int row) {
  if constexpr (ROWBYTES >= 256) return (row & 3) << 2;
  else if constexpr (ROWBYTES == 128) return ((row >> 1) & 1) << 2;
  else return 0;
}

template <int BM, int BN, int WARPS_M, int WARPS_N, bool SKIP, int STAGES, int BKP>
__global__ __launch_bounds__(256) void wgrad_h_kernel(const HWgradParams hp) {
  const WgradParams& p = hp.g;
  static_assert(WARPS_M * WARPS_N == 4, "4 waves");
  constexpr int NW = 4;
  constexpr int WTM = BM / WARPS_M, WTN = BN / WARPS_N;
  constexpr int TM = WTM / 32, TN = WTN / 32;
  static_assert(TM >= 1 && TN >= 1 && WTM % 32 == 0 && WTN % 32 == 0, "wave tile");
  constexpr int RBA = BM * 2, RBB = BN * 2;                     // bytes per pixel row of the images
  constexpr int kStageB = BKP * (RBA + RBB);                    // bytes per stage
  static_assert(STAGES >= 2 && STAGES <= 4, "ring depth");
  static_assert(BKP == 64 || BKP == 32, "K-step");
  constexpr int NSUB = BKP / 32;                                // 32-pixel sub-steps per K-step
  constexpr int kPatchB = NW * 32 * (WTN + 4) * 4;              // one 32-row tile row per wave at a time (store_row32)
  constexpr int kLdsB = STAGES * kStageB > kPatchB ? STAGES * kStageB : kPatchB;
  static_assert(kLdsB <= 160 * 1024, "LDS");
  __shared__ __attribute__((aligned(16))) unsigned char lds_raw[kLdsB];
  constexpr int kA = 0, kB = BKP * RBA;                         // byte offsets inside a stage
  // DMA pieces (1 KiB = one wave-instruction): RA / RB pixel rows each, IA / IB pieces per wave and K-step
  constexpr int RA = 1024 / RBA, RB = 1024 / RBB;
  constexpr int PA = BKP / RA, PB = BKP / RB;                   // pieces per K-step
  constexpr int IA = (PA + NW - 1) / NW, IB = (PB + NW - 1) / NW;
  // (fewer pieces than waves -- a 32-column operand with the short K-step: the spare waves re-load piece (wave mod pieces),
  // the same bytes into the same place, so that every wave issues and counts the same number of DMAs)
  static_assert((PA % NW == 0 || PA < NW) && (PB % NW == 0 || PB < NW), "whole pieces per wave");
  static_assert(RA >= 4 && RB >= 4 && RA <= 32 && RB <= 32, "a piece covers whole 4-row groups inside one 32-pixel sub-step");
  constexpr int CA = RBA / 16, CB = RBB / 16;                   // 16-byte chunks per pixel row

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WARPS_N, wn = wave % WARPS_N;
  const int gridN = (p.K + BN - 1) / BN;
  int wg_tile, wg_split;
  wgrad_block((int)gridDim.x, wg_tile, wg_split);
  const int tile_n = wg_tile % gridN;
  const int tile_m = wg_tile / gridN;
  const int m0 = tile_m * BM, n0 = tile_n * BN;

  const __amdgpu_buffer_rsrc_t xr = make_rsrc(p.x, p.x_bytes);
  const __amdgpu_buffer_rsrc_t dr = make_rsrc(p.dy, p.dy_bytes);

  const int p_begin = wg_split * p.pix_per_split;
  int p_end = p_begin + p.pix_per_split;
  if (p_end > p.P) p_end = p.P;

  // ---- per-lane constants of the DMA pieces.  Piece q = wave + NW * g of the K-step covers pixel rows [R q, R q + R);
  // lane l fills (row l / C, physical chunk l % C) and therefore fetches the logical chunk (l % C) ^ swz(row).
  int a_row[IA], a_col[IA];        // pixel row inside the K-step (0..63), first channel of the chunk or -1
  int a_ih[IA], a_iw[IA];          // patch mode: position inside the 32-pixel patch
  int b_row[IB], b_c[IB], b_dh[IB], b_dw[IB], b_ih[IB], b_iw[IB];
  bool b_colok[IB];
  int a_piece[IA], b_piece[IB];
#pragma unroll
  for (int g = 0; g < IA; ++g) {
    a_piece[g] = (wave + NW * g) % PA;
    const int row = RA * a_piece[g] + lane / CA;
    const int col = m0 + 8 * ((lane % CA) ^ wg_swz<RBA>(row));
    a_row[g] = row;
    a_col[g] = col < p.Cout ? col : -1;
    const int rr = row & 31;
    a_ih[g] = rr / p.patch_w;
    a_iw[g] = rr - a_ih[g] * p.patch_w;
  }
#pragma unroll
  for (int g = 0; g < IB; ++g) {
    b_piece[g] = (wave + NW * g) % PB;
    const int row = RB * b_piece[g] + lane / CB;
    const int col = n0 + 8 * ((lane % CB) ^ wg_swz<RBB>(row));
    b_row[g] = row;
    b_colok[g] = col < p.K;
    const int tap = b_colok[g] ? col / p.Cin : 0;
    b_c[g] = col - tap * p.Cin;
    const int r = tap / p.kw, sx = tap - r * p.kw;
    b_dh[g] = r * p.dil - p.pad;
    b_dw[g] = sx * p.dil - p.pad;
    const int rr = row & 31;
    b_ih[g] = rr / p.patch_w;
    b_iw[g] = rr - b_ih[g] * p.patch_w;
  }

  // patch mode (the map tiles into 32-pixel patches: every DeepLabV3+ / UNet / HRNet layer but the smallest maps): the byte
  // offset of a piece is a block-uniform patch origin + a per-lane constant, so a K-step costs no address arithmetic for the dy
  // operand (the origin rides in the scalar offset of the DMA) and one add + the range test of its tap for the x operand
  // (round 4: the per-piece multiply chains were 9 VALU + 11 SALU instructions per MFMA)
  uint32_t a_loff[IA];
  int b_loff[IB], b_ch[IB], b_cw[IB];
#pragma unroll
  for (int g = 0; g < IA; ++g)
    a_loff[g] = a_col[g] >= 0 ? (uint32_t)((a_ih[g] * p.Wo + a_iw[g]) * p.ldy + a_col[g]) * 2u : kOOB;
#pragma unroll
  for (int g = 0; g < IB; ++g) {
    b_ch[g] = b_ih[g] * p.stride + b_dh[g];
    b_cw[g] = b_iw[g] * p.stride + b_dw[g];
    b_loff[g] = ((b_ch[g] * p.Wi + b_cw[g]) * p.ldx + b_c[g]) * 2;
  }

  const int t_dh = (n0 / p.Cin / p.kw) * p.dil - p.pad;
  const int t_dw = ((n0 / p.Cin) % p.kw) * p.dil - p.pad;
  // the stream of live 32-pixel sub-steps; a K-step takes two of them (the second may be none: zeros)
  auto next_valid = [&](int pt) -> int {
    if (SKIP)
      while (pt < p_end && wg_step_dead(p, pt, p_end, t_dh, t_dw)) pt += 32;
    return pt;
  };

  typedef __attribute__((address_space(3))) void* lds_ptr;
  auto issue = [&](int pt0, int pt1, int st) {     // sub-steps at pixels pt0 / pt1 (>= p_end: all-zero pieces)
    unsigned char* sb = lds_raw + st * kStageB;
    if (p.patch_mode) {
      uint32_t oa[NSUB], obx[NSUB];      // block-uniform byte origins of the sub-steps' patches in dy / x (kOOB: no such sub-step)
      int hs[NSUB], ws[NSUB];
#pragma unroll
      for (int s = 0; s < NSUB; ++s) {
        const int pt = s ? pt1 : pt0;
        int b = 0, h0 = 0, w0 = 0;
        const bool live = pt < p_end;
        if (live) wg_patch_origin(p, pt, b, h0, w0);
        hs[s] = h0 * p.stride;
        ws[s] = w0 * p.stride;
        oa[s] = live ? (uint32_t)(((b * p.Ho + h0) * p.Wo + w0) * p.ldy) * 2u : kOOB;
        obx[s] = live ? (uint32_t)(((b * p.Hi + hs[s]) * p.Wi + ws[s]) * p.ldx) * 2u : kOOB;
      }
#pragma unroll
      for (int g = 0; g < IA; ++g) {
        const int s = a_row[g] >> 5;
        // (a dead sub-step or a channel chunk beyond Cout: origin or lane constant is kOOB, the sum stays out of range)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(dr, (lds_ptr)(sb + kA + RA * a_piece[g] * RBA), 16, (int)(oa[s] + a_loff[g]), 0, 0, 0);
      }
#pragma unroll
      for (int g = 0; g < IB; ++g) {
        const int s = b_row[g] >> 5;
        const int hi = hs[s] + b_ch[g], wi = ws[s] + b_cw[g];
        const bool ok = b_colok[g] && obx[s] != kOOB && ((unsigned)hi < (unsigned)p.Hi) && ((unsigned)wi < (unsigned)p.Wi);
        const uint32_t off = ok ? obx[s] + (uint32_t)b_loff[g] : kOOB;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(xr, (lds_ptr)(sb + kB + RB * b_piece[g] * RBB), 16, (int)off, 0, 0, 0);
      }
      return;
    }
    int ob[NSUB], oh[NSUB], ow[NSUB];
    bool live[NSUB];
#pragma unroll
    for (int s = 0; s < NSUB; ++s) {
      const int pt = s ? pt1 : pt0;
      live[s] = pt < p_end;
      ob[s] = oh[s] = ow[s] = 0;
      if (live[s] && p.patch_mode) wg_patch_origin(p, pt, ob[s], oh[s], ow[s]);
    }
#pragma unroll
    for (int g = 0; g < IA; ++g) {
      const int s = a_row[g] >> 5;
      const int pt = s ? pt1 : pt0;
      int b, ho, wo;
      bool ok = live[s] && a_col[g] >= 0;
      if (p.patch_mode) {
        b = ob[s];
        ho = oh[s] + a_ih[g];
        wo = ow[s] + a_iw[g];
      } else {
        const int pix = pt + (a_row[g] & 31);
        ok = ok && pix < p_end;
        const uint32_t bb = hp.howo_div.div((uint32_t)(ok ? pix : 0));
        const uint32_t rem = (uint32_t)(ok ? pix : 0) - bb * hp.howo_div.d;
        const uint32_t hh = hp.wo_div.div(rem);
        b = (int)bb;
        ho = (int)hh;
        wo = (int)(rem - hh * hp.wo_div.d);
      }
      const uint32_t off = ok ? (uint32_t)(((b * p.Ho + ho) * p.Wo + wo) * p.ldy + a_col[g]) * 2u : kOOB;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(dr, (lds_ptr)(sb + kA + RA * a_piece[g] * RBA), 16, (int)off, 0, 0, 0);
    }
#pragma unroll
    for (int g = 0; g < IB; ++g) {
      const int s = b_row[g] >> 5;
      const int pt = s ? pt1 : pt0;
      int b, ho, wo;
      bool ok = live[s] && b_colok[g];
      if (p.patch_mode) {
        b = ob[s];
        ho = oh[s] + b_ih[g];
        wo = ow[s] + b_iw[g];
      } else {
        const int pix = pt + (b_row[g] & 31);
        ok = ok && pix < p_end;
        const uint32_t bb = hp.howo_div.div((uint32_t)(ok ? pix : 0));
        const uint32_t rem = (uint32_t)(ok ? pix : 0) - bb * hp.howo_div.d;
        const uint32_t hh = hp.wo_div.div(rem);
        b = (int)bb;
        ho = (int)hh;
        wo = (int)(rem - hh * hp.wo_div.d);
      }
      const int hi = ho * p.stride + b_dh[g], wi = wo * p.stride + b_dw[g];
      ok = ok && ((unsigned)hi < (unsigned)p.Hi) && ((unsigned)wi < (unsigned)p.Wi);
      const uint32_t off = ok ? (uint32_t)(((b * p.Hi + hi) * p.Wi + wi) * p.ldx + b_c[g]) * 2u : kOOB;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(xr, (lds_ptr)(sb + kB + RB * b_piece[g] * RBB), 16, (int)off, 0, 0, 0);
    }
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // ---- transposed fragment reads.  MFMA operand of lane l: row (channel) l & 31, k (pixels) 8 * (l >> 5) + 0..7.
  // ds_read_b64_tr_b16 per 16-lane group: a block of 4 pixel rows x 16 channels; lane 4q + pp supplies the address of
  // (row q, channels 4 pp .. 4 pp + 3), lane i receives channel i of the 4 rows.  Read r (0 / 1) of k16-step kk takes pixel
  // rows 16 kk + 8 (l >> 5) + 4 r + q, channels tile + 16 ((l >> 4) & 1) + ...: element e of read r is k = 4 r + e.
  const int tq = (lane & 15) >> 2, tp = lane & 3, tg = (lane >> 4) & 1, th = lane >> 5;
  int offA[TM], offB[TN];          // byte offsets inside a stage for kk = 0, r = 0
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int row = 8 * th + tq;                                              // (+ 16 kk + 4 r: multiples of 4)
    const int chunk = (wm * WTM + 32 * i) / 8 + 2 * tg + (tp >> 1);
    offA[i] = kA + row * RBA + 16 * (chunk ^ wg_swz<RBA>(row)) + 8 * (tp & 1);
  }
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int row = 8 * th + tq;
    const int chunk = (wn * WTN + 32 * j) / 8 + 2 * tg + (tp >> 1);
    offB[j] = kB + row * RBB + 16 * (chunk ^ wg_swz<RBB>(row)) + 8 * (tp & 1);
  }
  typedef short s16x8 __attribute__((ext_vector_type(8)));
  constexpr int HK = BKP / 32;           // 16-pixel MFMA steps per half of a K-step: 2 or 1
  // fragment halves as the transposing reads deliver them (inline assembly: see tr_read_asm -- the builtin made hipcc drain the
  // operand ring with `s_waitcnt vmcnt(0)` in front of every K-step's first read); [set][k2 * T + tile], k2 = 16-pixel step
  // inside the half.  The halves are joined into MFMA operands only AFTER the wait that covers them.
  s16x4t falo[2][HK * TM], fahi[2][HK * TM], fblo[2][HK * TN], fbhi[2][HK * TN];
  constexpr int kReadsPerCall = HK * (TM + TN) * 2;
  const uint32_t lds0 = lds_addr_of(lds_raw);
  auto read_frags = [&](auto setc, int st, auto halfc) {
    constexpr int SET = decltype(setc)::value, HALF = decltype(halfc)::value;
    const uint32_t sbase = lds0 + (uint32_t)(st * kStageB);
    static_for<HK>([&](auto k2c) {
      constexpr int k2 = decltype(k2c)::value, kk = HALF * HK + k2;
      static_for<TM>([&](auto ic) {
        constexpr int i = decltype(ic)::value;
        const uint32_t a = sbase + (uint32_t)offA[i];
        falo[SET][k2 * TM + i] = tr_read_asm<(16 * kk) * RBA>(a);
        fahi[SET][k2 * TM + i] = tr_read_asm<(16 * kk + 4) * RBA>(a);
      });
      static_for<TN>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        const uint32_t b = sbase + (uint32_t)offB[j];
        fblo[SET][k2 * TN + j] = tr_read_asm<(16 * kk) * RBB>(b);
        fbhi[SET][k2 * TN + j] = tr_read_asm<(16 * kk + 4) * RBB>(b);
      });
    });
  };
  auto mfmas = [&](auto setc) {
    constexpr int SET = decltype(setc)::value;
#pragma unroll
    for (int k2 = 0; k2 < HK; ++k2)
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const s16x4t al = falo[SET][k2 * TM + i], ah = fahi[SET][k2 * TM + i];
          const s16x4t bl = fblo[SET][k2 * TN + j], bh = fbhi[SET][k2 * TN + j];
          const s16x8 av = s16x8{al[0], al[1], al[2], al[3], ah[0], ah[1], ah[2], ah[3]};
          const s16x8 bv = s16x8{bl[0], bl[1], bl[2], bl[3], bh[0], bh[1], bh[2], bh[3]};
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8v, av), __builtin_bit_cast(f16x8v, bv), acc[i][j],
                                                             0, 0, 0);
        }
  };
  // all but the youngest N LDS reads have returned (the counter has four bits)
  auto wait_older_reads = [&]() {
    constexpr int N = kReadsPerCall < 15 ? kReadsPerCall : 15;
    if constexpr (N == 15) asm volatile("s_waitcnt lgkmcnt(15)" ::: "memory");
    else if constexpr (N == 12) asm volatile("s_waitcnt lgkmcnt(12)" ::: "memory");
    else if constexpr (N == 8) asm volatile("s_waitcnt lgkmcnt(8)" ::: "memory");
    else if constexpr (N == 6) asm volatile("s_waitcnt lgkmcnt(6)" ::: "memory");
    else if constexpr (N == 4) asm volatile("s_waitcnt lgkmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  };
  typedef std::integral_constant<int, 0> c0;
  typedef std::integral_constant<int, 1> c1;
  {
    // the stream of live 32-pixel sub-steps, two per K-step; head[i] = first sub-step of the i-th tile of the ring (head[0] is
    // the one being multiplied, the others are in flight), p_end once the stream is exhausted (all-zero dummy pieces)
    constexpr int NG = IA + IB;
    int cursor = next_valid(p_begin);
    auto take = [&]() -> int {
      const int q = cursor;
      if (cursor < p_end) cursor = next_valid(cursor + 32);
      return q;
    };
    int head[STAGES];
    if (cursor < p_end) {
#pragma unroll
      for (int s0 = 0; s0 < STAGES; ++s0) {
        const int u = take(), v = NSUB == 2 ? take() : p_end;
        head[s0] = u;
        issue(u, v, s0);
      }
      wait_vmcnt<(STAGES - 1) * NG>();
      __builtin_amdgcn_s_barrier();
      read_frags(c0{}, 0, c0{});
      int st = 0;
      while (head[0] < p_end) {
        const int st1 = st == STAGES - 1 ? 0 : st + 1;
        read_frags(c1{}, st, c1{});
        wait_older_reads();             // set 0 (issued one phase ago) is in its registers; set 1 may still be on its way
        __builtin_amdgcn_sched_barrier(0);
        mfmas(c0{});
        __builtin_amdgcn_sched_barrier(0);
        wait_vmcnt<(STAGES - 2) * NG>();                    // the next K-step has landed; STAGES - 2 more stay in flight
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // set 1 is in; this wave is done reading stage `st`
        __builtin_amdgcn_s_barrier();
        read_frags(c0{}, st1, c0{});    // (zeros on the last step: never multiplied)
        __builtin_amdgcn_sched_barrier(0);
        const int u = take(), v = NSUB == 2 ? take() : p_end;
        issue(u, v, st);              // stage `st` is free now
        mfmas(c1{});
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s0 = 0; s0 + 1 < STAGES; ++s0) head[s0] = head[s0 + 1];
        head[STAGES - 1] = u;
        st = st1;
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // dummy pieces must not land in the output patches
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
  }

  float* out = p.dw + (long long)wg_split * p.slab_stride;
  {
    float* patch = reinterpret_cast<float*>(lds_raw) + wave * (32 * (WTN + 4));
    const int col0 = n0 + wn * WTN;
    int cv = p.K - col0;
    cv = cv < 0 ? 0 : (cv > WTN ? WTN : cv);
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int row0 = m0 + wm * WTM + i * 32;
      int rv = p.Cout - row0;
      rv = rv < 0 ? 0 : (rv > 32 ? 32 : rv);
      store_row32<TN>(acc[i], patch, out, true, p.K, row0, col0, rv, cv, nullptr, p.accumulate != 0, lane, [](int m) { return m; });
    }
  }
}

// ------------------------------------------------------------------------------------------------ host side
// The tiles wgrad_h_kernel is instantiated for (rows = Cout, columns = K; four waves), stated once: select_wgrad_h picks an
// entry, launch_wgrad_h maps it to template arguments.
struct HWgradTile {
  int bm, bn, wm, wn;
};
constexpr HWgradTile kHWgradTiles[] = {{128, 128, 2, 2}, {128, 64, 2, 2}, {128, 32, 4, 1}, {64, 128, 2, 2}, {32, 128, 1, 4}};
constexpr int kNumHWgradTiles = (int)(sizeof(kHWgradTiles) / sizeof(kHWgradTiles[0]));

// Everything run_wgrad_h decides before it launches; the queries read their answers off the same choice.
struct HWgradChoice {
  WgradPlan pl;
  WgradPixelOrder order;
  int tile;        // entry of kHWgradTiles; -1: a forced tile that nothing is instantiated for
  bool skip;       // the kernel's SKIP template flag
  int bkp;         // pixels per K-step, 32 / 64
};
constexpr int kHWgradStages = 2;      // ring depth of wgrad_h_kernel (select_wgrad_h says why)

// The one place that picks the kernel of an fp16 weight gradient.  Pure: launches nothing, touches no device.
static HWgradChoice select_wgrad_h(const WgradGeom& q) {
  HWgradChoice c;
  // pixel splits for ONE resident block per CU (round 4): every split writes and re-reads a [Cout][K] fp32 slab, and under the
  // half policy that traffic was 40 % of the weight-gradient bytes (2.1 GB written + 2.1 GB read per DeepLabV3+ step for 157 MB
  // of gradients).  Half as many splits halve it; the step got 1.2 % faster with it (15.15 -> 14.97 ms: the blocks share the CUs
  // with the data gradients of the other stream anyway).  PSEG_WGRAD_BPC overrides.
  c.pl = plan_wgrad(q.P(), q.Cout, q.K(), false, true, 1);
  if (c.pl.tile.bm == 256) c.pl.tile.bm = 128;      // (no 256-row tile here; the grid keeps the plan's rows)
  c.order = wgrad_pixel_order(q, c.pl.tile.bn);
  c.skip = c.order.mode != kWgDense;
  c.tile = -1;
  for (int i = 0; i < kNumHWgradTiles; ++i)
    if (kHWgradTiles[i].bm == c.pl.tile.bm && kHWgradTiles[i].bn == c.pl.tile.bn) c.tile = i;
  // ring depth: always kHWgradStages = 2 -- a deeper ring costs the resident blocks the grid wants and measured slower on every
  // layer (profiles/EXPERIMENTS.md, "Weight gradient: ring depth hurts, resident blocks help")
  // pixels per K-step: 32 halves the ring (four blocks per CU instead of two) and pays on the deep 3x3 layers -- ASPP 361 -> 298
  // / 294 -> 238 / 250 -> 216 us, layer-4 3x3 140 -> 111 -- while the short launches (bounded by their slab traffic and
  // their prologue / epilogue) do not care and the narrow classifier loses 10 % (tools/bench_conv_half.py, PSEG_HWGRAD_BKP)
  const int forced_bkp = cfg().hwgrad_bkp;
  c.bkp = (forced_bkp == 32 || forced_bkp == 64) ? forced_bkp : ((q.kh * q.kw > 1 && q.Cout >= 128 && q.K() >= 4096) ? 32 : 64);
  return c;
}

// the record of a choice (pseg_debug_last_wgrad, pseg_conv2d_wgrad_choice_h)
static void record_wgrad_h(const HWgradChoice& c, int* out11) { wgrad_record(out11, PSEG_KERNEL_WGRAD_H, c.pl, c.order, c.bkp, c.skip); }

template <int... I>
static void launch_wgrad_h(const HWgradChoice& c, dim3 grid, hipStream_t st, const HWgradParams& hp, std::integer_sequence<int, I...>) {
  auto launch = [&](auto tile, auto steps) {
    constexpr HWgradTile t = kHWgradTiles[decltype(tile)::value];
    using S = decltype(steps);
    if (c.skip) hipLaunchKernelGGL((wgrad_h_kernel<t.bm, t.bn, t.wm, t.wn, true, S::st, S::kb>), grid, dim3(256), 0, st, hp);
    else hipLaunchKernelGGL((wgrad_h_kernel<t.bm, t.bn, t.wm, t.wn, false, S::st, S::kb>), grid, dim3(256), 0, st, hp);
  };
  (void)((c.tile == I && (c.bkp == 32 ? launch(std::integral_constant<int, I>{}, HSteps<32, kHWgradStages>{})
                                      : launch(std::integral_constant<int, I>{}, HSteps<64, kHWgradStages>{}), true)) || ...);
}

// validate, select, check the workspace, fill the parameters from the choice and launch, reduce the slabs.
// defer: a split plan leaves its slabs in the workspace (the caller reduces them later, pseg_slab_reduce_batch)
static int run_wgrad_h(const WgradGeom& q, const void* x, int ldx, const void* dy, int ldy, float* dw, int accumulate,
                       void* workspace, int64_t workspace_bytes, hipStream_t st, bool defer) {
  PSEG_REQUIRE(x && dy && dw, "conv2d_wgrad_h: null pointer");
  PSEG_REQUIRE(q.Cin % 8 == 0 && q.Cout % 8 == 0 && ldx % 8 == 0 && ldy % 8 == 0, "conv2d_wgrad_h: Cin, Cout, ldx, ldy must be multiples of 8");
  PSEG_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)dy & 15) == 0 && ((uintptr_t)dw & 15) == 0,
               "conv2d_wgrad_h: x / dy / dw must be 16-byte aligned");
  PSEG_REQUIRE(q.P() > 0 && q.P() < (1LL << 31), "conv2d_wgrad_h: bad pixel count");
  const long long xb = nhwc_bytes_h(q.B, q.H, q.W, q.Cin, ldx), db = nhwc_bytes_h(q.B, q.Ho, q.Wo, q.Cout, ldy);
  PSEG_REQUIRE(xb < kMaxBytes && db < kMaxBytes, "conv2d_wgrad_h: tensor exceeds 2 GiB");
  const HWgradChoice c = select_wgrad_h(q);
  const WgradPlan& pl = c.pl;
  HWgradParams hp;
  WgradParams& p = hp.g;
  p.x = reinterpret_cast<const float*>(x);
  p.dy = reinterpret_cast<const float*>(dy);
  p.x_bytes = (uint32_t)xb;
  p.dy_bytes = (uint32_t)db;
  p.ldx = ldx;
  p.ldy = ldy;
  set_wgrad_geometry(p, q, pl, c.order);
  hp.howo_div = FastDiv((uint32_t)(q.Ho * q.Wo));
  hp.wo_div = FastDiv((uint32_t)q.Wo);
  const int rc = set_wgrad_output(p, pl, dw, accumulate, workspace, workspace_bytes, "conv2d_wgrad_h");
  if (rc != PSEG_OK) return rc;
  PSEG_REQUIRE(c.tile >= 0, "conv2d_wgrad_h: no kernel for tile %dx%d", pl.tile.bm, pl.tile.bn);
  g_last_conv_kernel = PSEG_KERNEL_WGRAD_H;
  record_wgrad_h(c, g_last_wgrad);
  launch_wgrad_h(c, dim3((unsigned)(pl.gridM * pl.gridN), 1, (unsigned)pl.splits), st, hp, std::make_integer_sequence<int, kNumHWgradTiles>{});
  PSEG_LAUNCH_CHECK();
  if (pl.splits > 1 && !defer)
    return launch_slab_reduce((const float*)workspace, p.slab_stride, pl.splits, dw, p.K, (long long)q.Cout, p.K, nullptr, accumulate, st);
  return PSEG_OK;
}

}  // namespace pseg

using namespace pseg;

extern "C" {

// the problem of a query, which knows Ho / Wo only: the smallest unit-stride input that gives them (the pixel split does not
// depend on it)
static WgradGeom wgrad_query_problem_h(int B, int Ho, int Wo, int Cin, int Cout, int kh, int kw) {
  return WgradGeom{B, Ho + kh - 1, Wo + kw - 1, Cin, Ho, Wo, Cout, kh, kw, 1, 0, 1};
}

int pseg_conv2d_wgrad_splits_h(int B, int Ho, int Wo, int Cin, int Cout, int kh, int kw) {
  if (B <= 0 || Ho <= 0 || Wo <= 0 || Cin <= 0 || Cout <= 0) return 0;
  return select_wgrad_h(wgrad_query_problem_h(B, Ho, Wo, Cin, Cout, kh, kw)).pl.splits;
}

int pseg_conv2d_wgrad_choice_h(int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad, int dil,
                               int* out11) {
  PSEG_REQUIRE(out11 != nullptr, "conv2d_wgrad_choice_h: null pointer");
  PSEG_REQUIRE(B > 0 && H > 0 && W > 0 && Cin > 0 && Ho > 0 && Wo > 0 && Cout > 0 && kh > 0 && kw > 0 && stride > 0 && pad >= 0 && dil > 0,
               "conv2d_wgrad_choice_h: bad geometry");
  record_wgrad_h(select_wgrad_h(WgradGeom{B, H, W, Cin, Ho, Wo, Cout, kh, kw, stride, pad, dil}), out11);
  return PSEG_OK;
}

int64_t pseg_conv2d_wgrad_workspace_bytes_h(int B, int Ho, int Wo, int Cin, int Cout, int kh, int kw) {
  const int splits = select_wgrad_h(wgrad_query_problem_h(B, Ho, Wo, Cin, Cout, kh, kw)).pl.splits;
  return splits > 1 ? (int64_t)splits * Cout * kh * kw * Cin * 4 : 0;
}

int pseg_conv2d_wgrad_h(const pseg_half_t* x, int ldx, const pseg_half_t* dy, int ldy, float* dw, int B, int H, int W,
                        int Cin, int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad, int dil, int accumulate,
                        void* workspace, int64_t workspace_bytes, void* stream) {
  return run_wgrad_h(WgradGeom{B, H, W, Cin, Ho, Wo, Cout, kh, kw, stride, pad, dil}, x, ldx, dy, ldy, dw, accumulate, workspace,
                     workspace_bytes, (hipStream_t)stream, false);
}

int pseg_conv2d_wgrad_slabs_h(const pseg_half_t* x, int ldx, const pseg_half_t* dy, int ldy, float* slabs, int B, int H,
                              int W, int Cin, int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad, int dil,
                              int64_t slab_bytes, void* stream) {
  PSEG_REQUIRE(pseg_conv2d_wgrad_splits_h(B, Ho, Wo, Cin, Cout, kh, kw) > 1,
               "conv2d_wgrad_slabs_h: this plan does not split -- call pseg_conv2d_wgrad_h");
  return run_wgrad_h(WgradGeom{B, H, W, Cin, Ho, Wo, Cout, kh, kw, stride, pad, dil}, x, ldx, dy, ldy, slabs, 0, slabs, slab_bytes,
                     (hipStream_t)stream, true);
}

}  // extern "C"
