// Implicit-GEMM convolution for gfx950 on v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulate): the gather side.
//
// One GEMM covers forward and data-gradient of every dense conv on the hot path (the weight gradient: conv_wgrad.hip)
// (reference models/aspp.py:12,27-30, models/deeplabv3plus.py:20,22, models/unet.py:19-23):
//
//  gather_conv_kernel  C[M=pixels][N] = A[M][K] * Bw[N][K]^T,  both operands K-contiguous.
//     A is never materialised: row m = (b,ho,wo), column k = (r,s,c) is gathered from the NHWC tensor at
//     ((ho*s_out + off0 + r*dstep)/s_in, (wo*s_out + off0 + s*dstep)/s_in).  fwd: s_out=stride, s_in=1,
//     dstep=+dil, off0=-pad.  dgrad: source = dy, s_out=1, s_in=stride, dstep=-dil, off0=+pad, Bw = the
//     transposed filter.  Taps that land in the zero padding (most of them for the rate-18 ASPP branch)
//     are fetched through a buffer descriptor with an out-of-range offset: the hardware returns 0.
//
// Tile: 256 threads = 4 waves, each wave owns a (BM/WARPS_M)x(BN/WARPS_N) block of 32x32 MFMA tiles.
// K-step 32, register-staged global->LDS double buffer (loads for step t+1 are issued before the MFMAs of
// step t and written to LDS after them), one barrier per step.  The fp32 MFMA issues once per 64 cycles per
// SIMD, so a step carries 16*TM*TN*64 cycles of matrix work per wave (4096 for the 128x128 tile) against
// 4-8 16-byte loads per lane; measured: the step's fixed costs (barrier, LDS write, first-read latency, address
// arithmetic) are what separates the kernel from the MFMA peak, hence the long step.
//
// LDS image:
//  gather_conv: [rows][32+4] floats (row stride 144 B = 9 x 16-B slots, 9 coprime to 16 -> the 16-lane groups
//     of ds_read_b128 hit 16 different slots; the 8 lanes of a ds_write_b128 group write one contiguous row).
//     Lane (i=l&31, h=l>>5) reads 4 consecutive k's {g*8+4h .. g*8+4h+3}; MFMA step j of group g therefore
//     contracts k = g*8+j (h=0 lanes) and g*8+4+j (h=1 lanes).  A and B use the same permutation, so the sum
//     over k is unchanged.
#include "conv_common.h"
#include "conv_limb.h"

// Per-block phase timestamps in gather_f32_dma_kernel: compiled in only with -DPSEG_CONV_TRACE=1 (PSEG_BUILD_TRACE=1 python -m
// pytorch_segmentation_amd.csrc.build --force) -- even dormant, the four extra branches cost 0.45 ms of the 46.3 ms step.
#ifndef PSEG_CONV_TRACE
#define PSEG_CONV_TRACE 0
#endif
constexpr bool kConvTrace = PSEG_CONV_TRACE != 0;

namespace pseg {

// PREC: 0 = exact fp32 (v_mfma_f32_32x32x2_f32); 1 = two bf16 limbs, 3 partial products (~17 bits per product);
//       2 = three bf16 limbs, 6 partial products down to 2^-16 (error ~2^-23 per product: fp32-equivalent);
//       3 = two fp16 limbs of the power-of-two-scaled operand, 3 partial products (~2^-22 per product)
template <int BM, int BN, int WARPS_M, int WARPS_N, bool SKIP, int PREC>
__global__ __launch_bounds__(64 * WARPS_M * WARPS_N) void gather_conv_kernel(const GatherConvParams p) {
  set_wave_prio(p.prio);
  static_assert(WARPS_M * WARPS_N == 4 || WARPS_M * WARPS_N == 8, "4 waves, or 8 for the 256-row tile");
  constexpr int NT = 64 * WARPS_M * WARPS_N;   // threads
  constexpr int RPP = NT / CPR;                // rows covered by one pass of the block's threads (shadows the 256-thread global)
  constexpr int WTM = BM / WARPS_M, WTN = BN / WARPS_N;
  constexpr int TM = WTM / 32, TN = WTN / 32;
  static_assert(TM >= 1 && TN >= 1 && WTM % 32 == 0 && WTN % 32 == 0, "wave tile");
  constexpr int AR = (BM + RPP - 1) / RPP, BR = (BN + RPP - 1) / RPP;

  // staging: fp32 -> 2 x [rows][BK+4] floats; split-bf16 -> 2 x NL limb images x [rows][16 dwords]
  constexpr int NL = PREC == 0 ? 1 : (PREC == 3 ? 2 : PREC + 1);
  constexpr int kStage = PREC == 0 ? 2 * (BM + BN) * LDT : 2 * (BM + BN) * 16 * NL;
  constexpr int kPatch = (NT / 64) * WTM * (WTN + 4);
  __shared__ __attribute__((aligned(16))) float lds[kStage > kPatch ? kStage : kPatch];
  float* As = lds;
  float* Bs = lds + 2 * BM * LDT;
  unsigned* ldsw = reinterpret_cast<unsigned*>(lds);
  // split-bf16 image bases (dwords): A limb l at kAl(l), B limb l at kBl(l), each [2 buffers][rows][16]
  constexpr int kAsz = 2 * BM * 16, kBsz = 2 * BN * 16, kBbase = NL * kAsz;

  const int tid = threadIdx.x;
  __builtin_assume(tid >= 0 && tid < NT);
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WARPS_N, wn = wave % WARPS_N;
  const int gridN = (p.N + BN - 1) / BN;
  // XCD-aware tile order: the dispatcher deals consecutive workgroups round-robin over the 8 XCDs, each with its own
  // L2.  Remap so that XCD x works on a CONTIGUOUS range of tiles: the gridN column tiles that share one gathered A
  // tile (and neighbouring row tiles that share halo pixels) then hit the same L2 instead of fetching A once per XCD.
  int bid = blockIdx.x;
  bid = remap_tile(p.xcd_remap, bid, (int)gridDim.x);
  const int tile_n = bid % gridN;
  const int tile_m = bid / gridN;
  const int m0 = tile_m * BM, n0 = tile_n * BN;

  const __amdgpu_buffer_rsrc_t xr = make_rsrc(p.x, p.x_bytes);
  const __amdgpu_buffer_rsrc_t wr = make_rsrc(p.w, p.w_bytes);
  const ResidualSel rsel;

  float scale_a = 1.f, scale_b = 1.f, unscale = 1.f;
  if constexpr (PREC == 3) {
    int ea, eb;
    scale_a = pow2_scale_for(*p.amax_a, ea);
    scale_b = pow2_scale_for(*p.amax_b, eb);
    unscale = __builtin_bit_cast(float, (unsigned)(127 - (ea + eb)) << 23);  // |ea + eb| <= 200 < 127? clamp below
    if (ea + eb > 126 || ea + eb < -126) unscale = exp2f(-(float)(ea + eb));
  }

  // ---- per-thread load assignment: 16-byte chunk cc of rows r0 + RPP*i
  const int cc = tid % CPR;
  const int r0 = tid / CPR;
  int a_bh[AR], a_bw[AR], a_img[AR];
  bool a_ok[AR];
#pragma unroll
  for (int i = 0; i < AR; ++i) {
    const int row = r0 + RPP * i;
    const int m = m0 + row;
    const bool ok = (row < BM) && (m < p.M);
    const int mm = ok ? m : 0;
    int b, ho, wo;
    row_to_pixel(p, mm, b, ho, wo);
    a_ok[i] = ok;
    a_bh[i] = ho * p.s_out + p.off0;
    a_bw[i] = wo * p.s_out + p.off0;
    a_img[i] = b * p.Hi * p.Wi;
  }
  uint32_t b_off[BR];
  bool b_ok[BR];
#pragma unroll
  for (int i = 0; i < BR; ++i) {
    const int row = r0 + RPP * i;
    const int n = n0 + row;
    b_ok[i] = (row < BN) && (n < p.N);
    b_off[i] = (uint32_t)n * (uint32_t)p.K;
  }

  // ---- K range of this block (split-K slice)
  const int kt_begin = blockIdx.z * p.kt_per_split;
  int kt_end = kt_begin + p.kt_per_split;
  if (kt_end > p.kt_total) kt_end = p.kt_total;

  // validity of tap (r, s) for load row i (the same test the loader applies)
  auto row_tap_ok = [&](int i, int dh, int dw, int& hn, int& wn_) -> bool {
    hn = a_bh[i] + dh;
    wn_ = a_bw[i] + dw;
    bool ok = a_ok[i];
    if (p.s_in != 1) {
      ok = ok && (hn % p.s_in == 0) && (wn_ % p.s_in == 0);
      hn /= p.s_in;
      wn_ /= p.s_in;
    }
    return ok && ((unsigned)hn < (unsigned)p.Hi) && ((unsigned)wn_ < (unsigned)p.Wi);
  };

  // ---- dilated convs: which taps touch at least one in-bounds pixel of this M tile?  (For the rate-18 ASPP branch
  // at 32x32 most (tile, tap) pairs are pure zero padding; their K-steps are never loaded nor multiplied.)
  unsigned tapmask = 0xFFFFFFFFu;
  if (SKIP) {
    unsigned mine = 0;
    for (int t = 0; t < p.ntaps; ++t) {
      const int r = t / p.kw, sx = t - r * p.kw;
      bool any = false;
#pragma unroll
      for (int i = 0; i < AR; ++i) {
        int hn, wn_;
        any = any || row_tap_ok(i, r * p.dstep, sx * p.dstep, hn, wn_);
      }
      if (any) mine |= 1u << t;
    }
    unsigned* sm = reinterpret_cast<unsigned*>(lds);
    if (tid == 0) sm[0] = 0u;
    __syncthreads();
    if (mine) atomicOr(&sm[0], mine);
    __syncthreads();
    tapmask = sm[0];
    __syncthreads();  // the staging buffers are written next
  }
  auto next_valid = [&](int kt) -> int {
    if (SKIP) {
      while (kt < kt_end) {
        const int tap = kt / p.ktiles_per_tap;
        if ((tapmask >> tap) & 1u) break;
        kt = (tap + 1) * p.ktiles_per_tap;
      }
      if (kt > kt_end) kt = kt_end;
    }
    return kt;
  };
  // K-step after `kt`: inside a live tap the successor is kt + 1 (no division); only a tap boundary rescans the mask
  int nv_tap_end = 0;   // first K-step of the tap after the one `kt` walks in (SKIP only)
  auto next_after = [&](int kt) -> int {
    if (!SKIP) return kt + 1;
    if (kt + 1 < nv_tap_end) return kt + 1;
    const int n = next_valid(kt + 1);
    nv_tap_end = (n / p.ktiles_per_tap + 1) * p.ktiles_per_tap;
    return n;
  };

  f32x4 areg[AR], breg[BR];

  // K-step kt: this thread's chunk is k = kt*BK + cc*4 = (r*kw + s)*Cin + c.  Everything that depends on the tap
  // (r, s) -- the in-range test of each gathered row and its pixel offset -- is computed when the tap CHANGES
  // (every Cin/BK steps for Cin >= BK) and kept as one byte offset per row (kOOB = zero padding); a plain K-step then
  // costs one add per load.  (Measured before this hoist: 2 VALU instructions per MFMA and ~500 instructions of
  // branchy address arithmetic in front of every 64-MFMA burst.)
  int kt_cur = -1, k_cur = 0, kr_cur = 0, ks_cur = 0, kc_cur = 0;
  uint32_t a_off[AR];
  uint32_t b_offb[BR];
#pragma unroll
  for (int i = 0; i < BR; ++i) b_offb[i] = b_ok[i] ? b_off[i] * 4u : kOOB;
  auto retap = [&]() {
    const int dh = kr_cur * p.dstep, dw = ks_cur * p.dstep;
    const bool tap_ok = kr_cur * p.kw + ks_cur < p.ntaps;   // K tail (K % BK != 0): chunks beyond the last tap are zero
#pragma unroll
    for (int i = 0; i < AR; ++i) {
      int hn, wn_;
      const bool ok = row_tap_ok(i, dh, dw, hn, wn_) && tap_ok;
      a_off[i] = ok ? (uint32_t)((a_img[i] + hn * p.Wi + wn_) * p.ldx) * 4u : kOOB;
    }
  };
  auto seek = [&](int kt) {
    k_cur = kt * BK + cc * 4;
    const int tap = k_cur / p.Cin;
    kc_cur = k_cur - tap * p.Cin;
    kr_cur = tap / p.kw;
    ks_cur = tap - kr_cur * p.kw;
    kt_cur = kt;
    retap();
  };
  auto load_tile = [&](int kt) {
    if (SKIP) {
      if (kt != kt_cur) seek(kt);  // the tap-skipping walk jumps; plain steps stay incremental
    } else if (kt_cur < 0) {
      seek(kt);
    }
    const uint32_t kcb = (uint32_t)kc_cur * 4u;
#pragma unroll
    for (int i = 0; i < AR; ++i) areg[i] = buf_load4(xr, a_off[i] + kcb);   // kOOB + kcb stays out of range
    const bool kvalid = k_cur < p.K;
    const uint32_t kb = (uint32_t)k_cur * 4u;
#pragma unroll
    for (int i = 0; i < BR; ++i) breg[i] = buf_load4(wr, kvalid ? b_offb[i] + kb : kOOB);
    // advance to the next K-step
    k_cur += BK;
    kc_cur += BK;
    if (kc_cur >= p.Cin) {
      do {
        kc_cur -= p.Cin;
        if (++ks_cur == p.kw) {
          ks_cur = 0;
          ++kr_cur;
        }
      } while (kc_cur >= p.Cin);
      retap();
    }
    kt_cur = kt + 1;
  };

  auto store_tile = [&](int buf) {
    if constexpr (PREC == 0) {
#pragma unroll
      for (int i = 0; i < AR; ++i) {
        const int row = r0 + RPP * i;
        if (row < BM) *reinterpret_cast<f32x4*>(&As[(buf * BM + row) * LDT + cc * 4]) = areg[i];
      }
#pragma unroll
      for (int i = 0; i < BR; ++i) {
        const int row = r0 + RPP * i;
        if (row < BN) *reinterpret_cast<f32x4*>(&Bs[(buf * BN + row) * LDT + cc * 4]) = breg[i];
      }
    } else {
      // chunk cc = k 4cc..4cc+3 -> 8 bytes at half (cc&1) of k-slot (cc>>1)
#pragma unroll
      for (int i = 0; i < AR; ++i) {
        const int row = r0 + RPP * i;
        if (row < BM) {
          u32x2 limb[NL];
          if constexpr (PREC == 3) split4h(areg[i], scale_a, limb);
          else split4n<NL>(areg[i], limb, rsel);
          const int o = buf * BM * 16 + swz(row, cc >> 1) + (cc & 1) * 2;
#pragma unroll
          for (int l = 0; l < NL; ++l) *reinterpret_cast<u32x2*>(&ldsw[l * kAsz + o]) = limb[l];
        }
      }
#pragma unroll
      for (int i = 0; i < BR; ++i) {
        const int row = r0 + RPP * i;
        if (row < BN) {
          u32x2 limb[NL];
          if constexpr (PREC == 3) split4h(breg[i], scale_b, limb);
          else split4n<NL>(breg[i], limb, rsel);
          const int o = buf * BN * 16 + swz(row, cc >> 1) + (cc & 1) * 2;
#pragma unroll
          for (int l = 0; l < NL; ++l) *reinterpret_cast<u32x2*>(&ldsw[kBbase + l * kBsz + o]) = limb[l];
        }
      }
    }
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int frag_row = lane & 31;
  const int frag_k = (lane >> 5) * 4;

  // ---- main loop.  Two fragment sets alternate between the two 16-deep halves of a K-step; three tiles are in flight:
  // `cur` in LDS buffer `buf` (being multiplied), `nxt` complete in buffer buf^1, `stg` in the staging registers (its
  // global loads were issued one whole K-step earlier).  Per K-step:
  //   A  fetch the fragments of half 1 of `cur`
  //   B  MFMAs on half 0 (fragments fetched during the previous burst)                 -- hides A
  //   C  barrier: every wave is done reading `buf`; buf^1 (written a K-step ago) is visible
  //   D  fetch the fragments of half 0 of `nxt` from buf^1
  //   E  split + write `stg` into `buf`, issue the global loads of the tile after it,
  //      MFMAs on half 1 (already in registers)                                        -- hides D and the traffic
  // so nothing the matrix pipe waits for is issued right in front of it, and the barrier has no data to wait for.
  // The tap bookkeeping of the load stream (carry into the next tap, tap-skipping jumps, end of stream) runs at the TOP
  // of an iteration, which leaves block E straight-line code the scheduler can spread over the MFMAs.  An exhausted
  // stream keeps "loading" with out-of-range offsets (zeros) into a buffer nobody reads again.
  static_assert(BK == 32, "two half-steps per K-step");
  constexpr int FRA = PREC == 0 ? 2 * TM : NL * TM, FRB = PREC == 0 ? 2 * TN : NL * TN;
  f32x4 fa[2][FRA], fb[2][FRB];   // PREC 0: [gg][tile] fp32 k-quads; limb variants: [limb][tile] 8 x 16-bit
  auto read_frags = [&](int set, int buf, int half) {
    if constexpr (PREC == 0) {
#pragma unroll
      for (int gg = 0; gg < 2; ++gg) {
        const int g = half * 2 + gg;
#pragma unroll
        for (int i = 0; i < TM; ++i)
          fa[set][gg * TM + i] = *reinterpret_cast<const f32x4*>(
              &As[(buf * BM + wm * WTM + i * 32 + frag_row) * LDT + g * 8 + frag_k]);
#pragma unroll
        for (int j = 0; j < TN; ++j)
          fb[set][gg * TN + j] = *reinterpret_cast<const f32x4*>(
              &Bs[(buf * BN + wn * WTN + j * 32 + frag_row) * LDT + g * 8 + frag_k]);
      }
    } else {
      // one 16-deep k-slice: lane (row = l&31, h = l>>5) holds k = 16*half + 8h .. +7 (k-slot 2*half + h) of its row
      const int slot = half * 2 + (lane >> 5);
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int o = buf * BM * 16 + swz(wm * WTM + i * 32 + frag_row, slot);
#pragma unroll
        for (int l = 0; l < NL; ++l) fa[set][l * TM + i] = *reinterpret_cast<const f32x4*>(&ldsw[l * kAsz + o]);
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int o = buf * BN * 16 + swz(wn * WTN + j * 32 + frag_row, slot);
#pragma unroll
        for (int l = 0; l < NL; ++l) fb[set][l * TN + j] = *reinterpret_cast<const f32x4*>(&ldsw[kBbase + l * kBsz + o]);
      }
    }
  };
  auto mfmas = [&](int set) {
    if constexpr (PREC == 0) {
#pragma unroll
      for (int gg = 0; gg < 2; ++gg)
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[set][gg * TM + i][e], fb[set][gg * TN + j][e], acc[i][j],
                                                               0, 0, 0);
    } else {
      // partial products la + lb <= NL - 1 (orders 2^0, 2^-8, 2^-16), smallest first
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int ord = NL - 1; ord >= 0; --ord)
#pragma unroll
            for (int la = 0; la <= ord; ++la) {
              if constexpr (PREC == 3)
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, fa[set][la * TM + i]),
                                                                   __builtin_bit_cast(f16x8, fb[set][(ord - la) * TN + j]),
                                                                   acc[i][j], 0, 0, 0);
              else
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fa[set][la * TM + i]),
                                                                    __builtin_bit_cast(bf16x8, fb[set][(ord - la) * TN + j]),
                                                                    acc[i][j], 0, 0, 0);
            }
    }
  };
  auto issue_load = [&]() {
    const uint32_t kcb = (uint32_t)kc_cur * 4u;
#pragma unroll
    for (int i = 0; i < AR; ++i) areg[i] = buf_load4(xr, a_off[i] + kcb);
    const bool kvalid = k_cur < p.K;
    const uint32_t kb = (uint32_t)k_cur * 4u;
#pragma unroll
    for (int i = 0; i < BR; ++i) breg[i] = buf_load4(wr, kvalid ? b_offb[i] + kb : kOOB);
    k_cur += BK;
    kc_cur += BK;
    kt_cur += 1;
  };
  {
    const int t0 = next_valid(kt_begin);
    if (t0 < kt_end) {
      load_tile(t0);
      store_tile(0);
      int cur = t0, nxt = next_after(t0), stg = kt_end;
      if (nxt < kt_end) {
        load_tile(nxt);
        store_tile(1);
        stg = next_after(nxt);
        if (stg < kt_end) load_tile(stg);
      } else {
        nxt = kt_end;
      }
      __syncthreads();
      read_frags(0, 0, 0);
      int buf = 0;
      bool dead = false;
      while (cur < kt_end) {
        const int after = stg < kt_end ? next_after(stg) : kt_end;
        if (after < kt_end) {
          if (SKIP && after != kt_cur) {
            seek(after);
          } else if (kc_cur >= p.Cin) {
            do {
              kc_cur -= p.Cin;
              if (++ks_cur == p.kw) {
                ks_cur = 0;
                ++kr_cur;
              }
            } while (kc_cur >= p.Cin);
            retap();
          }
        } else if (!dead) {
          dead = true;
#pragma unroll
          for (int i = 0; i < AR; ++i) a_off[i] = kOOB;
          k_cur = p.K;
          kc_cur = 0;
        }
        read_frags(1, buf, 1);
        __builtin_amdgcn_sched_barrier(0);
        mfmas(0);
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();
        read_frags(0, buf ^ 1, 0);   // (garbage on the last step: never multiplied)
        __builtin_amdgcn_sched_barrier(0);
        store_tile(buf);
        issue_load();
        mfmas(1);
        __builtin_amdgcn_sched_barrier(0);
        cur = nxt;
        nxt = stg;
        stg = after;
        buf ^= 1;
      }
      __syncthreads();   // the epilogue reuses the staging buffers as output patches
    }
  }

  if constexpr (PREC == 3) {  // undo the operand scaling (exact: a power of two)
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) acc[i][j] *= unscale;
  }

  // ---- epilogue.  C/D map of the 32x32 MFMA: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5).
  // (the main loop ended with a barrier: the staging buffers are free, each wave takes a private patch)
  float* yout = p.y + (long long)blockIdx.z * p.slab_stride;
  const int col_l = lane & 31;
  const int row_h = (lane >> 5) * 4;
  {
    float* patch = lds + wave * (WTM * (WTN + 4));
    const int row0 = m0 + wm * WTM, col0 = n0 + wn * WTN;
    int rv = p.M - row0, cv = p.N - col0;
    rv = rv < 0 ? 0 : (rv > WTM ? WTM : rv);
    cv = cv < 0 ? 0 : (cv > WTN ? WTN : cv);
    store_tiles<TM, TN>(acc, patch, yout, p.ldy, row0, col0, rv, cv, p.bias, p.accumulate != 0, lane, [&](int m) {
      if (!p.row_perm) return m;
      int b, ho, wo;
      row_to_pixel(p, m, b, ho, wo);
      return (b * p.Ho + ho) * p.Wo + wo;
    });
  }

  // ---- fused BatchNorm batch statistics: one row group per (M tile, wave row), shifted by the group's first
  // sample so that sum((y-K)^2) does not cancel when |mean| >> std.  No LDS, no barrier.
  if (p.stat != nullptr) {
    const int group = tile_m * WARPS_M + wm;
    const long long gsz = (long long)p.stat_rows * p.N;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int col = n0 + wn * WTN + j * 32 + col_l;
      // row 0 of this wave's sub-tile lives in register 0 of the lanes with (lane>>5) == 0
      const float k0 = __shfl(acc[0][j][0], lane & 31, 64);
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = m0 + wm * WTM + i * 32 + (r & 3) + 8 * (r >> 2) + row_h;
          if (row < p.M) {
            const float d = acc[i][j][r] - k0;
            s1 += d;
            s2 += d * d;
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

// ------------------------------------------------------------------------------------------------
// Split-bf16 gather GEMM on PRE-SPLIT operands, staged by LDS-DMA.
//
// The limb variants of gather_conv_kernel spend 4-7 VALU instructions and one ds_write per MFMA on splitting fp32
// operands into bf16 limbs in every consumer (measured: MFMA pipe busy 0.25-0.5, issue-bound).  Here the producers split
// ONCE (pseg_split_planes / the BatchNorm backward pass emit bf16 hi and lo planes, 4 bytes per element like the fp32
// tensor) and the tiles go global -> LDS with `buffer_load_dwordx4 ... lds`: no staging registers, no VALU, no ds_write.
// The swizzled LDS image (16-byte k-slot XOR (row>>2)&3, conflict-free ds_read_b128) is produced on the SOURCE side: a
// wave-instruction fills 16 rows x 64 bytes of LDS linearly, lane l lands at (row l/4, physical slot l%4) and therefore
// fetches logical slot (l%4) ^ ((row>>2)&3) of its row.  Zero padding = out-of-range buffer offset = zeros in LDS.
//
// 256x128 tile, 8 waves (4x2), K-step 32, THREE LDS stages of 48 KB (A hi/lo 256 rows + B hi/lo 128 rows, 64 B per row):
// tile i is multiplied while i+1 and i+2 are in flight; per K-step one counted s_waitcnt vmcnt(6) (leaves the 6 DMAs of
// tile i+2 outstanding), one raw s_barrier, then the 6 DMAs of tile i+3 go into the stage that barrier freed.  An
// exhausted stream keeps issuing out-of-range DMAs so that the count stays exact.
// Requirements (host-checked): channels of the gathered tensor % 32 == 0 (a K-step never straddles a tap), no split-K.
constexpr int kDmaBM = 256, kDmaBN = 128;
constexpr int kDmaStageDw = (2 * kDmaBM + 2 * kDmaBN) * 16;   // dwords per stage: A_hi, A_lo, B_hi, B_lo

template <bool SKIP>
__global__ __launch_bounds__(512) void gather_limb_dma_kernel(const GatherConvParams p) {
  set_wave_prio(p.prio);
  constexpr int BM = kDmaBM, BN = kDmaBN, WARPS_N = 2;
  constexpr int WTM = 64, WTN = 64, TM = 2, TN = 2, NL = 2;
  constexpr int kPatch = 8 * WTM * (WTN + 4);
  constexpr int kLds = 3 * kDmaStageDw > kPatch ? 3 * kDmaStageDw : kPatch;
  __shared__ __attribute__((aligned(16))) float lds[kLds];
  unsigned* ldsw = reinterpret_cast<unsigned*>(lds);
  // plane bases inside a stage (dwords)
  constexpr int kAhi = 0, kAlo = BM * 16, kBhi = 2 * BM * 16, kBlo = 2 * BM * 16 + BN * 16;

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

  const __amdgpu_buffer_rsrc_t xhr = make_rsrc(p.xh, p.xp_bytes), xlr = make_rsrc(p.xl, p.xp_bytes);
  const __amdgpu_buffer_rsrc_t whr = make_rsrc(p.wh, p.wp_bytes), wlr = make_rsrc(p.wl, p.wp_bytes);

  // ---- loader roles: wave w fills A rows [32w, 32w+32) (two 16-row groups) and B rows [16w, 16w+16), hi and lo
  const int lrow = lane >> 2, lslot = lane & 3;
  int a_bh[2], a_bw[2], a_img[2];
  bool a_ok[2];
  int a_slot_b[2];   // byte offset of this lane's LOGICAL k-slot inside a 32-deep K-step (8 bf16 = 16 B per slot)
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    const int row = 32 * wave + 16 * g + lrow;
    const int m = m0 + row;
    const bool ok = m < p.M;
    int b, ho, wo;
    row_to_pixel(p, ok ? m : 0, b, ho, wo);
    a_ok[g] = ok;
    a_bh[g] = ho * p.s_out + p.off0;
    a_bw[g] = wo * p.s_out + p.off0;
    a_img[g] = b * p.Hi * p.Wi;
    a_slot_b[g] = (lslot ^ ((row >> 2) & 3)) * 16;
  }
  const int b_row = 16 * wave + lrow;
  const bool b_ok = (n0 + b_row) < p.N;
  const uint32_t b_rowoff = b_ok ? (uint32_t)(n0 + b_row) * (uint32_t)p.K * 2u + (uint32_t)((lslot ^ ((b_row >> 2) & 3)) * 16) : kOOB;

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
      int hn, wn_;
      const bool any = row_tap_ok(0, r * p.dstep, sx * p.dstep, hn, wn_) || row_tap_ok(1, r * p.dstep, sx * p.dstep, hn, wn_);
      if (any) mine |= 1u << t;
    }
    if (tid == 0) ldsw[0] = 0u;
    __syncthreads();
    if (mine) atomicOr(&ldsw[0], mine);
    __syncthreads();
    tapmask = ldsw[0];
    __syncthreads();
  }
  // ---- the stream of live K-steps, TAP major (all 32-channel chunks of a live tap, then the next live tap).
  // (Channel-chunk-major order -- the taps of one chunk back to back, so that the shifted re-reads of a tile's pixels hit
  // L1 / L2 -- was measured SLOWER, 370 -> 348 TF on the 512->512 3x3 layer: consecutive K-steps of a filter row then lie
  // Cout*2 bytes apart and every 64-byte k-slot costs its own half-used 128-byte line.)
  tapmask &= (p.ntaps >= 32) ? 0xFFFFFFFFu : ((1u << p.ntaps) - 1u);
  const int nlive = __builtin_popcount(tapmask);
  const int n_steps = nlive * p.ktiles_per_tap;
  int s_chunk = 0;
  unsigned s_tm = tapmask;
  auto next_kt = [&]() -> int {     // next K-step of the stream, kt_end when exhausted
    if (s_tm == 0u) return kt_end;
    const int kt = __builtin_ctz(s_tm) * p.ktiles_per_tap + s_chunk;
    if (++s_chunk == p.ktiles_per_tap) {
      s_chunk = 0;
      s_tm &= s_tm - 1u;
    }
    return kt;
  };

  // ---- DMA issue of K-step kt into stage st (kt >= kt_end: all-zero dummy tile, keeps the vmcnt arithmetic exact)
  int tap_cur = -1;
  uint32_t a_off[2] = {kOOB, kOOB};
  auto issue = [&](int kt, int st) {
    uint32_t ao[2], bo;
    if (kt < kt_end) {
      const int tap = kt / p.ktiles_per_tap;
      if (tap != tap_cur) {
        tap_cur = tap;
        const int kr = tap / p.kw, ks = tap - kr * p.kw;
#pragma unroll
        for (int g = 0; g < 2; ++g) {
          int hn, wn_;
          const bool ok = row_tap_ok(g, kr * p.dstep, ks * p.dstep, hn, wn_);
          a_off[g] = ok ? (uint32_t)((a_img[g] + hn * p.Wi + wn_) * p.ldxp) * 2u + (uint32_t)a_slot_b[g] : kOOB;
        }
      }
      const uint32_t kc_b = (uint32_t)((kt - tap * p.ktiles_per_tap) * BK) * 2u;
      ao[0] = a_off[0] + kc_b;     // kOOB + kc_b stays out of range
      ao[1] = a_off[1] + kc_b;
      bo = b_rowoff + (uint32_t)kt * (uint32_t)(BK * 2);
    } else {
      ao[0] = ao[1] = bo = kOOB;
    }
    unsigned* sb = ldsw + st * kDmaStageDw;
    typedef __attribute__((address_space(3))) void* lds_ptr;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const int ro = (32 * wave + 16 * g) * 16;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(xhr, (lds_ptr)(sb + kAhi + ro), 16, (int)ao[g], 0, 0, 0);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(xlr, (lds_ptr)(sb + kAlo + ro), 16, (int)ao[g], 0, 0, 0);
    }
    __builtin_amdgcn_raw_ptr_buffer_load_lds(whr, (lds_ptr)(sb + kBhi + 16 * wave * 16), 16, (int)bo, 0, 0, 0);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(wlr, (lds_ptr)(sb + kBlo + 16 * wave * 16), 16, (int)bo, 0, 0, 0);
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int frag_row = lane & 31;
  f32x4 fa[2][NL * TM], fb[2][NL * TN];
  auto read_frags = [&](int set, int st, int half) {
    const int slot = half * 2 + (lane >> 5);
    const unsigned* sb = ldsw + st * kDmaStageDw;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int o = swz(wm * WTM + i * 32 + frag_row, slot);
      fa[set][0 * TM + i] = *reinterpret_cast<const f32x4*>(&sb[kAhi + o]);
      fa[set][1 * TM + i] = *reinterpret_cast<const f32x4*>(&sb[kAlo + o]);
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int o = swz(wn * WTN + j * 32 + frag_row, slot);
      fb[set][0 * TN + j] = *reinterpret_cast<const f32x4*>(&sb[kBhi + o]);
      fb[set][1 * TN + j] = *reinterpret_cast<const f32x4*>(&sb[kBlo + o]);
    }
  };
  auto mfmas = [&](int set) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int ord = NL - 1; ord >= 0; --ord)
#pragma unroll
          for (int la = 0; la <= ord; ++la)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fa[set][la * TM + i]),
                                                                __builtin_bit_cast(bf16x8, fb[set][(ord - la) * TN + j]),
                                                                acc[i][j], 0, 0, 0);
  };

  {
    // tile i is multiplied while i+1 and i+2 are in flight and i+3 is issued
    if (n_steps > 0) {
      issue(next_kt(), 0);
      issue(next_kt(), 1);
      issue(next_kt(), 2);
      asm volatile("s_waitcnt vmcnt(12)" ::: "memory");   // tile 0 has landed (this wave's share)
      __builtin_amdgcn_s_barrier();                        // ... and everybody's
      read_frags(0, 0, 0);
      int st = 0;
      for (int it = 0; it < n_steps; ++it) {
        const int st1 = st == 2 ? 0 : st + 1;
        read_frags(1, st, 1);
        __builtin_amdgcn_sched_barrier(0);
        mfmas(0);
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt vmcnt(6)" ::: "memory");   // the tile after this one has landed; one more stays in flight
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // this wave is done reading stage `st`
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
  }

  // ---- epilogue (the stages are free: each wave takes a private patch)
  float* yout = p.y;
  {
    float* patch = lds + wave * (WTM * (WTN + 4));
    const int row0 = m0 + wm * WTM, col0 = n0 + wn * WTN;
    int rv = p.M - row0, cv = p.N - col0;
    rv = rv < 0 ? 0 : (rv > WTM ? WTM : rv);
    cv = cv < 0 ? 0 : (cv > WTN ? WTN : cv);
    store_tiles<TM, TN>(acc, patch, yout, p.ldy, row0, col0, rv, cv, nullptr, p.accumulate != 0, lane, [&](int m) {
      if (!p.row_perm) return m;
      int b, ho, wo;
      row_to_pixel(p, m, b, ho, wo);
      return (b * p.Ho + ho) * p.Wo + wo;
    });
  }
}

// ------------------------------------------------------------------------------------------------
// Exact-fp32 gather GEMM staged by LDS-DMA: the same K-step stream, three-stage ring and barrier / vmcnt protocol as
// gather_limb_dma_kernel, on the fp32 tensors themselves (no planes needed) and v_mfma_f32_32x32x2_f32.
// LDS image: [rows][32 floats = 128 B = eight 16-byte k-slots], slot XOR ((row >> 1) & 7): the 16-lane groups of the
// fragment ds_read_b128 (rows {0-3,12-15,20-27} of a 32-row fragment, one slot) then cover all sixteen (row & 1, slot)
// bank groups once.  A wave-instruction of the DMA fills 8 rows x 128 B linearly: lane l = (row l/8, physical slot l%8)
// fetches logical slot (l%8) ^ ((row>>1)&7) of its row.  Compared with gather_conv_kernel<..., 0> there are no staging
// registers, no ds_write_b128, no per-K-step address VALU, and the prefetch is two tiles deep.
// Tiles: 256x128 / 128x128 with 8 waves (one block per CU), 128x64 / 64x128 with 4 waves (two blocks per CU).
// Requirements (host-checked): channels of the gathered tensor % 32 == 0, no split-K.
// GENERIC (round 5): channel counts that are NOT a multiple of the K-step (the 7x7 stem on 4 channels, the classifier's data
// gradient on 24): a K-step then straddles taps, and every lane derives (tap, channel) of its own 16-byte k-slot -- K-slot index
// / slots per tap -- once per K-step and row group (two divisions by multiply-shift; ~40 VALU instructions per wave and K-step
// beside 2048 matrix cycles).  Every tap is issued (no skipping); slots past K read nothing.
template <int BM, int BN, int WARPS_M, int WARPS_N, bool SKIP, int STAGES = 3, bool GENERIC = false>
__global__ __launch_bounds__(64 * WARPS_M * WARPS_N) void gather_f32_dma_kernel(const GatherConvParams p) {
  static_assert(!(SKIP && GENERIC), "tap skipping needs whole K-steps per tap");
  set_wave_prio(p.prio);
  static_assert(STAGES == 2 || STAGES == 3, "ring depth");
  constexpr int NW = WARPS_M * WARPS_N, NT = 64 * NW;
  static_assert(NW == 8 || NW == 4, "8 or 4 waves");
  constexpr int WTM = BM / WARPS_M, WTN = BN / WARPS_N, TM = WTM / 32, TN = WTN / 32;
  static_assert(TM >= 1 && TN >= 1 && WTM % 32 == 0 && WTN % 32 == 0, "wave tile");
  constexpr int kStageDw = (BM + BN) * 32;
  constexpr int kPatch = NW * WTM * (WTN + 4);
  constexpr int kLds = STAGES * kStageDw > kPatch ? STAGES * kStageDw : kPatch;
  __shared__ __attribute__((aligned(16))) float lds[kLds];
  unsigned* ldsw = reinterpret_cast<unsigned*>(lds);
  constexpr int kA = 0, kB = BM * 32;
  // DMA row groups (8 rows each): A groups [0, BM/8), then B groups; wave w owns groups w, w + NW, ...
  constexpr int GA = BM / 8 / NW, GB = BN / 8 / NW, NG = GA + GB;
  static_assert((BM / 8) % NW == 0 && (BN / 8) % NW == 0, "whole row groups per wave");

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

  const int lrow = lane >> 3, lslot = lane & 7;
  int a_bh[GA], a_bw[GA], a_img[GA], a_slot_b[GA];
  bool a_ok[GA];
#pragma unroll
  for (int g = 0; g < GA; ++g) {
    const int row = 8 * (wave + NW * g) + lrow;
    const int m = m0 + row;
    const bool ok = m < p.M;
    int b, ho, wo;
    row_to_pixel(p, ok ? m : 0, b, ho, wo);
    a_ok[g] = ok;
    a_bh[g] = ho * p.s_out + p.off0;
    a_bw[g] = wo * p.s_out + p.off0;
    a_img[g] = b * p.Hi * p.Wi;
    a_slot_b[g] = (lslot ^ ((row >> 1) & 7)) * 16;
  }
  uint32_t b_rowoff[GB];
  int b_slot[GB];      // GENERIC: logical k-slot of this lane in row group g (the filter row ends at K: slots past it read nothing)
#pragma unroll
  for (int g = 0; g < GB; ++g) {
    const int row = 8 * (wave + NW * g) + lrow;
    b_slot[g] = lslot ^ ((row >> 1) & 7);
    b_rowoff[g] = (n0 + row) < p.N ? (uint32_t)(n0 + row) * (uint32_t)p.K * 4u + (uint32_t)(b_slot[g] * 16) : kOOB;
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
  tapmask &= (p.ntaps >= 32) ? 0xFFFFFFFFu : ((1u << p.ntaps) - 1u);
  const int n_steps = GENERIC ? kt_end : __builtin_popcount(tapmask) * p.ktiles_per_tap;
  int s_chunk = 0, g_next = 0;
  unsigned s_tm = tapmask;
  auto next_kt = [&]() -> int {     // next live K-step (tap major), kt_end when exhausted
    if (GENERIC) return g_next < kt_end ? g_next++ : kt_end;      // (K-steps in order: they straddle taps)
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
    if (GENERIC && kt < kt_end) {
      const int spt = p.Cin >> 2;                     // 16-byte slots per tap
#pragma unroll
      for (int g = 0; g < GA; ++g) {
        const uint32_t s = (uint32_t)kt * 8u + (uint32_t)(a_slot_b[g] >> 4);      // logical k-slot of this lane
        const uint32_t tap = p.gen_spt.div(s);
        const uint32_t ch = (s - tap * (uint32_t)spt) * 4u;
        const uint32_t kr = p.gen_kw.div(tap), ks = tap - kr * (uint32_t)p.kw;
        int hn, wn_;
        const bool ok = (int)tap < p.ntaps && row_tap_ok(g, (int)kr * p.dstep, (int)ks * p.dstep, hn, wn_);
        ao[g] = ok ? (uint32_t)((a_img[g] + hn * p.Wi + wn_) * p.ldx + (int)ch) * 4u : kOOB;
      }
#pragma unroll
      for (int g = 0; g < GB; ++g) {
        const bool in_k = (kt * 8 + b_slot[g]) * 4 < p.K;
        bo[g] = in_k ? b_rowoff[g] + (uint32_t)kt * (uint32_t)(BK * 4) : kOOB;
      }
    } else if (kt < kt_end) {
      const int tap = kt / p.ktiles_per_tap;
      if (tap != tap_cur) {
        tap_cur = tap;
        const int kr = tap / p.kw, ks = tap - kr * p.kw;
#pragma unroll
        for (int g = 0; g < GA; ++g) {
          int hn, wn_;
          const bool ok = row_tap_ok(g, kr * p.dstep, ks * p.dstep, hn, wn_);
          a_off[g] = ok ? (uint32_t)((a_img[g] + hn * p.Wi + wn_) * p.ldx) * 4u + (uint32_t)a_slot_b[g] : kOOB;
        }
      }
      const uint32_t kc_b = (uint32_t)((kt - tap * p.ktiles_per_tap) * BK) * 4u;
#pragma unroll
      for (int g = 0; g < GA; ++g) ao[g] = a_off[g] + kc_b;     // kOOB + kc_b stays out of range
#pragma unroll
      for (int g = 0; g < GB; ++g) bo[g] = b_rowoff[g] + (uint32_t)kt * (uint32_t)(BK * 4);
    } else {
#pragma unroll
      for (int g = 0; g < GA; ++g) ao[g] = kOOB;
#pragma unroll
      for (int g = 0; g < GB; ++g) bo[g] = kOOB;
    }
    unsigned* sb = ldsw + st * kStageDw;
#pragma unroll
    for (int g = 0; g < GA; ++g)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(xr, (lds_ptr)(sb + kA + 8 * (wave + NW * g) * 32), 16, (int)ao[g], 0, 0, 0);
#pragma unroll
    for (int g = 0; g < GB; ++g)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(wr, (lds_ptr)(sb + kB + 8 * (wave + NW * g) * 32), 16, (int)bo[g], 0, 0, 0);
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
  auto swz32 = [](int row, int slot) -> int { return row * 32 + ((slot ^ ((row >> 1) & 7)) << 2); };
  f32x4 fa[2][2 * TM], fb[2][2 * TN];   // [set][gg * T + tile]: k-quads gg of a 16-deep half-step
  auto read_frags = [&](int set, int st, int half) {
    const float* sb = lds + st * kStageDw;
#pragma unroll
    for (int gg = 0; gg < 2; ++gg) {
      const int slot = 2 * (half * 2 + gg) + frag_h;
#pragma unroll
      for (int i = 0; i < TM; ++i)
        fa[set][gg * TM + i] = *reinterpret_cast<const f32x4*>(&sb[kA + swz32(wm * WTM + i * 32 + frag_row, slot)]);
#pragma unroll
      for (int j = 0; j < TN; ++j)
        fb[set][gg * TN + j] = *reinterpret_cast<const f32x4*>(&sb[kB + swz32(wn * WTN + j * 32 + frag_row, slot)]);
    }
  };
  auto mfmas = [&](int set) {
#pragma unroll
    for (int gg = 0; gg < 2; ++gg)
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[set][gg * TM + i][e], fb[set][gg * TN + j][e], acc[i][j], 0, 0,
                                                             0);
  };
  // counted waits: NG DMAs per tile and wave
  // (STAGES - 1) tiles stay in flight after the prologue wait, (STAGES - 2) inside the loop
  auto wait_two_left = [&]() {
    constexpr int left = (STAGES - 1) * NG;
    if constexpr (left == 12) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
    else if constexpr (left == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if constexpr (left == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else if constexpr (left == 5) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
    else if constexpr (left == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else if constexpr (left == 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
    else if constexpr (left == 10) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  };
  auto wait_one_left = [&]() {
    constexpr int left = (STAGES - 2) * NG;
    if constexpr (left == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else if constexpr (left == 5) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
    else if constexpr (left == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else if constexpr (left == 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  };
  static_assert(NG == 6 || NG == 5 || NG == 4 || NG == 3, "vmcnt immediates");

  unsigned long long tr0 = 0, tr1 = 0, tr2 = 0;
  if (kConvTrace && p.trace != nullptr) tr0 = wall_clock64();
  if (n_steps > 0) {
    issue(next_kt(), 0);
    issue(next_kt(), 1);
    if constexpr (STAGES == 3) issue(next_kt(), 2);
    wait_two_left();                   // tile 0 has landed (this wave's share)
    __builtin_amdgcn_s_barrier();      // ... and everybody's
    if (kConvTrace && p.trace != nullptr) tr1 = wall_clock64();
    read_frags(0, 0, 0);
    int st = 0;
    for (int it = 0; it < n_steps; ++it) {
      const int st1 = st == STAGES - 1 ? 0 : st + 1;
      read_frags(1, st, 1);
      __builtin_amdgcn_sched_barrier(0);
      mfmas(0);
      __builtin_amdgcn_sched_barrier(0);
      wait_one_left();                                     // the next tile has landed; one more stays in flight
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

  if (kConvTrace && p.trace != nullptr) tr2 = wall_clock64();
  // ---- epilogue: as gather_conv_kernel (bias / accumulate / row map, fused BatchNorm statistics)
  const int col_l = lane & 31;
  const int row_h = (lane >> 5) * 4;
  {
    float* patch = lds + wave * (WTM * (WTN + 4));
    const int row0 = m0 + wm * WTM, col0 = n0 + wn * WTN;
    int rv = p.M - row0, cv = p.N - col0;
    rv = rv < 0 ? 0 : (rv > WTM ? WTM : rv);
    cv = cv < 0 ? 0 : (cv > WTN ? WTN : cv);
    auto out_row = [&](int m) {
      if (!p.row_perm) return m;
      int b, ho, wo;
      row_to_pixel(p, m, b, ho, wo);
      return (b * p.Ho + ho) * p.Wo + wo;
    };
    if (p.bns_y != nullptr) {
      // data gradient that is the dz of a BatchNorm layer: its backward partial sums ride on the store loop
      const BnsEpilogue be{p.bns_y, p.bns_ldy, p.bns_mean, p.bns_invstd, p.bns_scale, p.bns_shift, p.bns_act, p.bns_db, p.bns_dg,
                           (long long)(tile_m * WARPS_M + wm) * p.N};
      store_tiles<TM, TN, false, true>(acc, patch, p.y, p.ldy, row0, col0, rv, cv, p.bias, p.accumulate != 0, lane, out_row, &be);
    } else {
      store_tiles<TM, TN>(acc, patch, p.y, p.ldy, row0, col0, rv, cv, p.bias, p.accumulate != 0, lane, out_row);
    }
  }
  if (p.stat != nullptr) {
    const int group = tile_m * WARPS_M + wm;
    const long long gsz = (long long)p.stat_rows * p.N;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int col = n0 + wn * WTN + j * 32 + col_l;
      const float k0 = __shfl(acc[0][j][0], lane & 31, 64);
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = m0 + wm * WTM + i * 32 + (r & 3) + 8 * (r >> 2) + row_h;
          if (row < p.M) {
            const float d = acc[i][j][r] - k0;
            s1 += d;
            s2 += d * d;
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
  if (kConvTrace && p.trace != nullptr && tid == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the stores of this wave have left
    unsigned hwid;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
    unsigned long long* t = p.trace + (long long)blockIdx.x * 5;
    t[0] = tr0;
    t[1] = tr1;
    t[2] = tr2;
    t[3] = wall_clock64();
    t[4] = hwid;
  }
}

// ------------------------------------------------------------------------------------------------
// HALO-STAGED 3x3 for NARROW outputs, exact fp32 (round 5; VERDICT r4 item 4 / item 2 "classifier kernel").  A 128x32 tile of
// gather_f32_dma_kernel pulls its A operand once per TAP: 16 KB of pixels + 4 KB of filter per 32-channel K-step for 1024 matrix
// cycles per SIMD -- 20 bytes per clock and CU through an LDS-DMA path that sustains ~27: with a 32-column tile the operand
// STREAM, not the matrix pipe, is the bound (HRNet's 32 -> 32 3x3 on 128x128 maps: 32 us for 18 us of matrix work; the classifier).
// Here an M tile is an 8 x 16 PATCH of output pixels and a 32-channel chunk of the A operand is DMA'd ONCE, as the 10 x 18 halo patch
// (23 KB; out-of-image pixels read as zeros = the conv's padding); the nine taps read their A fragments from it at shifted pixel
// rows.  The filter slice of the chunk runs through a three-stage ring of single taps ([BN columns][32 channels], 4 / 8 KB): one
// barrier per tap, the A fragments of the next tap are read before it (the halo image does not change inside a chunk).
// LDS 35 KB (32 columns: FOUR 4-wave blocks per CU) / 47 KB (64 columns: three).  A first form kept the chunk's whole filter slice
// resident (60 KB, two blocks per CU): faster alone, SLOWER in the steps, whose narrow layers run beside other kernels (HRNet's five
// replay lanes) -- residency is what they compete for (profiles/EXPERIMENTS.md 5.9).
//   halo image: row = halo pixel (hr * 18 + hc), 128 B = eight 16-byte k-slots, slot XOR ((hc >> 1) & 7).  A fragment ds_read_b128
//   serves lanes in groups {0-3, 12-15, 20-27} ...: 16 pixels of consecutive columns (two patch rows), i.e. 16 consecutive hc at
//   every tap, and 18 is even, so (LDS row parity, slot) = (hc & 1, slot ^ (hc >> 1) & 7) takes all sixteen values: conflict-free.
//   filter ring: row = stage * BN + column, the ring kernels' swizzle.
// Wave layouts = the ring kernel's for the same plan tile (so the statistics groups are the plan's): 128x32 on 4 x 1 waves (a wave:
// 2 patch rows x 32 columns), 128x64 on 2 x 2 (4 patch rows x 32 columns, two accumulators).
// Covers: 3x3, unit stride, dilation 1, padding 1 (forward and data gradient: the same gather with the taps reversed), channels of
// the gathered tensor % 32 == 0, maps of whole 8 x 16 patches (rows in patch order: row_perm 2); bias / accumulate / fused
// BatchNorm statistics / BatchNorm-backward sums as the ring kernel.  PSEG_CONV_HALO=0: off.
constexpr int kHaloPH = 8, kHaloPW = 16, kHaloHC = kHaloPW + 2, kHaloRows = (kHaloPH + 2) * kHaloHC;      // 180
constexpr int kHaloRowsPad = (kHaloRows + 7) / 8 * 8;                                                     // 184
template <int WARPS_M, int WARPS_N>
__global__ __launch_bounds__(256, WARPS_N == 1 ? 4 : 3) void gather_f32_halo_kernel(const GatherConvParams p) {
  set_wave_prio(p.prio);
  constexpr int NW = WARPS_M * WARPS_N;
  static_assert(NW == 4, "four waves");
  constexpr int BN = 32 * WARPS_N, WTM = 128 / WARPS_M, TM = WTM / 32;
  constexpr int kEpiDw = NW * WTM * 36;
  constexpr int kA = 0, kB = kHaloRowsPad * 32, kRing = kB + 3 * BN * 32, kLdsDw = kRing > kEpiDw ? kRing : kEpiDw;
  constexpr int GA = (kHaloRowsPad / 8 + NW - 1) / NW;      // 6 row groups of the halo image per wave (the last wave: 5)
  constexpr int GB = BN / 8 / NW;                            // row groups of one tap of the filter ring per wave (1 / 2)
  __shared__ __attribute__((aligned(16))) float lds[kLdsDw];
  unsigned* ldsw = reinterpret_cast<unsigned*>(lds);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WARPS_N, wn = wave % WARPS_N;
  const int gridN = (p.N + BN - 1) / BN;
  int bid = blockIdx.x;
  bid = remap_tile(p.xcd_remap, bid, (int)gridDim.x);
  const int tile_n = bid % gridN;
  const int tile_m = bid / gridN;
  const int m0 = tile_m * 128, n0 = tile_n * BN;
  // the patch of this tile (rows are in patch order: row_perm 2 with 8 x 16 patches)
  const int img = m0 / p.HoWo;
  const int patch = (m0 - img * p.HoWo) / (kHaloPH * kHaloPW);
  const int ph = patch / p.patches_per_row, pw = patch - ph * p.patches_per_row;
  const int h0 = ph * kHaloPH - 1, w0 = pw * kHaloPW - 1;     // image position of halo pixel (0, 0)

  const __amdgpu_buffer_rsrc_t xr = make_rsrc(p.x, p.x_bytes);
  const __amdgpu_buffer_rsrc_t wr = make_rsrc(p.w, p.w_bytes);
  const int lrow = lane >> 3, lslot = lane & 7;
  uint32_t a_off[GA], b_off[GB];
#pragma unroll
  for (int g = 0; g < GA; ++g) {
    const int idx = 8 * (wave + NW * g) + lrow;
    const int hr = idx / kHaloHC, hc = idx - hr * kHaloHC;
    const int y = h0 + hr, x = w0 + hc;
    const bool ok = idx < kHaloRows && (unsigned)y < (unsigned)p.Hi && (unsigned)x < (unsigned)p.Wi;
    const int slot = lslot ^ ((hc >> 1) & 7);
    a_off[g] = ok ? (uint32_t)(((img * p.Hi + y) * p.Wi + x) * p.ldx) * 4u + (uint32_t)(slot * 16) : kOOB;
  }
#pragma unroll
  for (int g = 0; g < GB; ++g) {
    const int n = 8 * (wave + NW * g) + lrow;         // column of the tile; its row of whichever tap is issued
    const int slot = lslot ^ ((n >> 1) & 7);
    b_off[g] = (n0 + n) < p.N ? (uint32_t)(n0 + n) * (uint32_t)p.K * 4u + (uint32_t)(slot * 16) : kOOB;
  }
  typedef __attribute__((address_space(3))) void* lds_ptr;
  auto issue_a = [&](int chunk) {
    const uint32_t kc = (uint32_t)chunk * 128u;
#pragma unroll
    for (int g = 0; g < GA; ++g)
      if (wave + NW * g < kHaloRowsPad / 8)      // (wave-uniform)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(xr, (lds_ptr)(ldsw + kA + 8 * (wave + NW * g) * 32), 16, (int)(a_off[g] + kc), 0, 0, 0);
  };
  auto issue_b = [&](int chunk, int t) {     // tap t of the chunk into stage t % 3
    const uint32_t kc = (uint32_t)chunk * 128u + (uint32_t)(t * p.Cin) * 4u;
#pragma unroll
    for (int g = 0; g < GB; ++g)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(wr, (lds_ptr)(ldsw + kB + ((t % 3) * BN + 8 * (wave + NW * g)) * 32), 16,
                                               (int)(b_off[g] == kOOB ? kOOB : b_off[g] + kc), 0, 0, 0);
  };

  f32x16 acc[TM][1];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][0][r] = 0.f;

  // fragment addressing: this lane's pixel in each of the wave's 2 x 16 strips, its halo row at tap offset (0, 0), the swizzle
  // terms of the three column offsets
  const int frag_row = lane & 31, frag_h = lane >> 5;
  const int pcol = frag_row & 15;
  const int hbase = (2 * wm * TM + (frag_row >> 4) + 1) * kHaloHC + (pcol + 1);      // strip i: + 2 i rows
  int a_col_dw[3], a_swz[3];
#pragma unroll
  for (int ts = 0; ts < 3; ++ts) {
    const int os = p.off0 + ts * p.dstep;          // -1, 0, +1 (forward) or +1, 0, -1 (data gradient)
    a_col_dw[ts] = os * 32;
    a_swz[ts] = ((pcol + 1 + os) >> 1) & 7;
  }
  const int b_frag = (wn * 32 + frag_row) * 32, b_swz = (frag_row >> 1) & 7;
  f32x4 fa[2][TM][4], fb[4];
  auto read_a = [&](int set, int t) {
    const int tr = t / 3, ts = t - tr * 3;
    const int orow = p.off0 + tr * p.dstep;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int arow = kA + (hbase + (2 * i + orow) * kHaloHC) * 32 + a_col_dw[ts];
#pragma unroll
      for (int q = 0; q < 4; ++q) fa[set][i][q] = *reinterpret_cast<const f32x4*>(&lds[arow + (((2 * q + frag_h) ^ a_swz[ts]) << 2)]);
    }
  };
  auto read_b = [&](int t) {
    const int brow = kB + (t % 3) * BN * 32 + b_frag;
#pragma unroll
    for (int q = 0; q < 4; ++q) fb[q] = *reinterpret_cast<const f32x4*>(&lds[brow + (((2 * q + frag_h) ^ b_swz) << 2)]);
  };
  auto mfmas = [&](int set) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int i = 0; i < TM; ++i) acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[set][i][q][e], fb[q][e], acc[i][0], 0, 0, 0);
  };

  const int nchunks = p.Cin >> 5;
  for (int c = 0; c < nchunks; ++c) {
    issue_a(c);
    issue_b(c, 0);
    issue_b(c, 1);
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      // in order: the halo image and taps <= t have landed when at most one younger tap (t + 1: GB DMAs) is outstanding
      if (t < 8) {
        if constexpr (GB == 1) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();               // ... everybody's share; and everybody is done with tap t - 1's ring stage
      if (t + 2 < 9) issue_b(c, t + 2);           // into the stage tap t - 1 was read from
      if (t == 0) read_a(0, 0);
      read_b(t);
      __builtin_amdgcn_sched_barrier(0);
      if (t + 1 < 9) read_a((t + 1) & 1, t + 1);
      mfmas(t & 1);
      __builtin_amdgcn_sched_barrier(0);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();          // everybody is done reading: the next chunk (or the output patches) may land
  }

  // ---- epilogue: as gather_f32_dma_kernel (bias / accumulate / row map, fused BatchNorm statistics / BatchNorm-backward sums)
  const int col_l = lane & 31;
  const int row_h = (lane >> 5) * 4;
  {
    float* patchb = lds + wave * (WTM * 36);
    const int row0 = m0 + wm * WTM, col0 = n0 + wn * 32;
    int rv = p.M - row0, cv = p.N - col0;
    rv = rv < 0 ? 0 : (rv > WTM ? WTM : rv);
    cv = cv < 0 ? 0 : (cv > 32 ? 32 : cv);
    auto out_row = [&](int m) {
      int b, ho, wo;
      row_to_pixel(p, m, b, ho, wo);
      return (b * p.Ho + ho) * p.Wo + wo;
    };
    if (p.bns_y != nullptr) {
      const BnsEpilogue be{p.bns_y, p.bns_ldy, p.bns_mean, p.bns_invstd, p.bns_scale, p.bns_shift, p.bns_act, p.bns_db, p.bns_dg,
                           (long long)(tile_m * WARPS_M + wm) * p.N};
      store_tiles<TM, 1, false, true>(acc, patchb, p.y, p.ldy, row0, col0, rv, cv, p.bias, p.accumulate != 0, lane, out_row, &be);
    } else {
      store_tiles<TM, 1>(acc, patchb, p.y, p.ldy, row0, col0, rv, cv, p.bias, p.accumulate != 0, lane, out_row);
    }
  }
  if (p.stat != nullptr) {
    const int group = tile_m * WARPS_M + wm;
    const long long gsz = (long long)p.stat_rows * p.N;
    const int col = n0 + wn * 32 + col_l;
    const float k0 = __shfl(acc[0][0][0], lane & 31, 64);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = m0 + wm * WTM + i * 32 + (r & 3) + 8 * (r >> 2) + row_h;
        if (row < p.M) {
          const float d = acc[i][0][r] - k0;
          s1 += d;
          s2 += d * d;
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

// ------------------------------------------------------------------------------------------------
// PERSISTENT form of the exact-fp32 LDS-DMA gather kernel for POINTWISE convs (round 5).  The 1x1 layers of a bottleneck network
// are short contractions on big maps: 8-16 K-steps per 128x128 tile.  Per-block stamps of gather_f32_dma_kernel on 256 -> 1024
// channels at 32x32 (profiles/EXPERIMENTS.md 5.1): prologue 4.0 us + K loop 24.9 us + epilogue 6.6 us -- the matrix pipe is busy
// 74 % of the launch, and what idles it is the chain kernel arguments -> row setup -> first DMA round trip at one end and the
// store drain at the other, once per TILE.  Here a block walks tiles blockIdx, blockIdx + grid, ...: ONE continuous stream of
// K-steps through the two-stage ring -- when a tile's last K-steps are being multiplied the DMAs of the next tile's first ones
// are already in flight -- and the epilogue works out of an 8-row patch of its own (store_tiles_rows8) beside the ring, so a
// block still takes 73 KB of LDS and two share a CU.  Pointwise only (rows are pixels: no index arithmetic per tile beyond two
// multiplications), channels a multiple of the K-step, no split-K; bias / accumulate / fused BatchNorm statistics / fused
// BatchNorm-backward sums as the tile-per-block kernel.
// (register budget: two 8-wave blocks, or three 4-wave blocks, per CU -- 4 / 3 waves per SIMD)
template <int BM, int BN, int WARPS_M, int WARPS_N, bool BNS>
__global__ __launch_bounds__(64 * WARPS_M * WARPS_N, (WARPS_M * WARPS_N == 8 ? 4 : 3)) void gather_f32_pw_kernel(
    const GatherConvParams p, int ntiles) {
  set_wave_prio(p.prio);
  constexpr int NW = WARPS_M * WARPS_N;
  static_assert(NW == 8 || NW == 4, "8 or 4 waves");
  constexpr int WTM = BM / WARPS_M, WTN = BN / WARPS_N, TM = WTM / 32, TN = WTN / 32;
  static_assert(TM >= 1 && TN >= 1 && WTM % 32 == 0 && WTN % 32 == 0, "wave tile");
  constexpr int kStageDw = (BM + BN) * 32;
  constexpr int kPatch8 = 8 * (WTN + 4);
  __shared__ __attribute__((aligned(16))) float lds[2 * kStageDw + NW * kPatch8];
  unsigned* ldsw = reinterpret_cast<unsigned*>(lds);
  constexpr int kA = 0, kB = BM * 32;
  constexpr int GA = BM / 8 / NW, GB = BN / 8 / NW;
  static_assert((BM / 8) % NW == 0 && (BN / 8) % NW == 0, "whole row groups per wave");

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WARPS_N, wn = wave % WARPS_N;
  const int gridN = (p.N + BN - 1) / BN;
  const int nblocks = (int)gridDim.x;
  const int ksteps = p.kt_total;

  const __amdgpu_buffer_rsrc_t xr = make_rsrc(p.x, p.x_bytes);
  const __amdgpu_buffer_rsrc_t wr = make_rsrc(p.w, p.w_bytes);
  const int lrow = lane >> 3, lslot = lane & 7;

  // ---- issue side: K-steps of this block's tiles, in order
  int i_vt = (int)blockIdx.x - nblocks;      // virtual tile whose K-steps are being issued (opened below)
  int i_kt = ksteps;                         // (== ksteps: the first issue opens a tile)
  bool i_done = false;
  uint32_t a_cur[GA], b_cur[GB];
  typedef __attribute__((address_space(3))) void* lds_ptr;
  auto issue = [&](int st) {
    if (i_kt == ksteps) {
      i_vt += nblocks;
      if (i_vt < ntiles) {
        const int t = remap_tile(p.xcd_remap, i_vt, ntiles);
        const int tn = t % gridN, tm = t / gridN;
#pragma unroll
        for (int g = 0; g < GA; ++g) {
          const int row = 8 * (wave + NW * g) + lrow;
          const int m = tm * BM + row;
          a_cur[g] = m < p.M ? (uint32_t)m * (uint32_t)p.ldx * 4u + (uint32_t)((lslot ^ ((row >> 1) & 7)) * 16) : kOOB;
        }
#pragma unroll
        for (int g = 0; g < GB; ++g) {
          const int row = 8 * (wave + NW * g) + lrow;
          const int n = tn * BN + row;
          b_cur[g] = n < p.N ? (uint32_t)n * (uint32_t)p.K * 4u + (uint32_t)((lslot ^ ((row >> 1) & 7)) * 16) : kOOB;
        }
        i_kt = 0;
      } else {
        i_done = true;
      }
    }
    if (i_done) return;          // nothing left: the stage keeps its old bytes, which nobody multiplies
    unsigned* sb = ldsw + st * kStageDw;
#pragma unroll
    for (int g = 0; g < GA; ++g)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(xr, (lds_ptr)(sb + kA + 8 * (wave + NW * g) * 32), 16, (int)a_cur[g], 0, 0, 0);
#pragma unroll
    for (int g = 0; g < GB; ++g)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(wr, (lds_ptr)(sb + kB + 8 * (wave + NW * g) * 32), 16, (int)b_cur[g], 0, 0, 0);
#pragma unroll
    for (int g = 0; g < GA; ++g) a_cur[g] += (uint32_t)(BK * 4);      // (kOOB + anything a launch can add stays out of range)
#pragma unroll
    for (int g = 0; g < GB; ++g) b_cur[g] += (uint32_t)(BK * 4);
    ++i_kt;
  };

  // ---- compute side
  f32x16 acc[TM][TN];
  const int frag_row = lane & 31, frag_h = lane >> 5;
  auto swz32 = [](int row, int slot) -> int { return row * 32 + ((slot ^ ((row >> 1) & 7)) << 2); };
  f32x4 fa[2][2 * TM], fb[2][2 * TN];
  auto read_frags = [&](int set, int st, int half) {
    const float* sb = lds + st * kStageDw;
#pragma unroll
    for (int gg = 0; gg < 2; ++gg) {
      const int slot = 2 * (half * 2 + gg) + frag_h;
#pragma unroll
      for (int i = 0; i < TM; ++i)
        fa[set][gg * TM + i] = *reinterpret_cast<const f32x4*>(&sb[kA + swz32(wm * WTM + i * 32 + frag_row, slot)]);
#pragma unroll
      for (int j = 0; j < TN; ++j)
        fb[set][gg * TN + j] = *reinterpret_cast<const f32x4*>(&sb[kB + swz32(wn * WTN + j * 32 + frag_row, slot)]);
    }
  };
  auto mfmas = [&](int set) {
#pragma unroll
    for (int gg = 0; gg < 2; ++gg)
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[set][gg * TM + i][e], fb[set][gg * TN + j][e], acc[i][j], 0, 0,
                                                             0);
  };

  float* patch8 = lds + 2 * kStageDw + wave * kPatch8;
  const int col_l = lane & 31, row_h = (lane >> 5) * 4;
  auto epilogue = [&](int tile_m, int tile_n) {
    const int m0 = tile_m * BM, n0 = tile_n * BN;
    const int row0 = m0 + wm * WTM, col0 = n0 + wn * WTN;
    int rv = p.M - row0, cv = p.N - col0;
    rv = rv < 0 ? 0 : (rv > WTM ? WTM : rv);
    cv = cv < 0 ? 0 : (cv > WTN ? WTN : cv);
    auto out_row = [](int m) { return m; };      // pointwise: GEMM row m is pixel m
    if constexpr (BNS) {
      const BnsEpilogue be{p.bns_y, p.bns_ldy, p.bns_mean, p.bns_invstd, p.bns_scale, p.bns_shift, p.bns_act, p.bns_db, p.bns_dg,
                           (long long)(tile_m * WARPS_M + wm) * p.N};
      store_tiles_rows8<TM, TN, true>(acc, patch8, p.y, p.ldy, row0, col0, rv, cv, p.bias, p.accumulate != 0, lane, out_row, &be);
    } else {
      store_tiles_rows8<TM, TN>(acc, patch8, p.y, p.ldy, row0, col0, rv, cv, p.bias, p.accumulate != 0, lane, out_row);
    }
    if (p.stat != nullptr) {       // fused BatchNorm statistics, as gather_f32_dma_kernel
      const int group = tile_m * WARPS_M + wm;
      const long long gsz = (long long)p.stat_rows * p.N;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int col = n0 + wn * WTN + j * 32 + col_l;
        const float k0 = __shfl(acc[0][j][0], lane & 31, 64);
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int row = m0 + wm * WTM + i * 32 + (r & 3) + 8 * (r >> 2) + row_h;
            if (row < p.M) {
              const float d = acc[i][j][r] - k0;
              s1 += d;
              s2 += d * d;
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
  };

  issue(0);
  issue(1);
  // K-step 0 has landed (this wave's share): all but the youngest GA + GB DMAs -- or everything, when the block has one K-step
  if (ksteps == 1 && (int)blockIdx.x + nblocks >= ntiles) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  else if constexpr (GA + GB == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
  else if constexpr (GA + GB == 5) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
  else if constexpr (GA + GB == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  else if constexpr (GA + GB == 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  read_frags(0, 0, 0);
  int st = 0;
  for (int c_vt = (int)blockIdx.x; c_vt < ntiles; c_vt += nblocks) {
    const int t = remap_tile(p.xcd_remap, c_vt, ntiles);
    const int tile_n = t % gridN, tile_m = t / gridN;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    for (int it = 0; it < ksteps; ++it) {
      const int st1 = st ^ 1;
      read_frags(1, st, 1);
      __builtin_amdgcn_sched_barrier(0);
      mfmas(0);
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the next K-step (of this tile or of the next) has landed
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave is done reading stage `st`
      __builtin_amdgcn_s_barrier();
      read_frags(0, st1, 0);      // (the next TILE's first half-step at a tile boundary; stale bytes after the last tile)
      __builtin_amdgcn_sched_barrier(0);
      issue(st);                  // stage `st` is free now
      mfmas(1);
      __builtin_amdgcn_sched_barrier(0);
      st = st1;
    }
    epilogue(tile_m, tile_n);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // no DMA may land after the block has given its LDS back
}

// fp32 [M][ld] -> bf16 hi / lo planes [M][ldp] (hi = bf16_rne(x), lo = bf16_rne(x - hi)); columns [C, ldp) are zeroed
__global__ __launch_bounds__(256) void split_planes_kernel(const float* __restrict__ x, int ldx, long long M, int C,
                                                           uint16_t* __restrict__ hi, uint16_t* __restrict__ lo, int ldp) {
  PSEG_HELPER_PRIO();
  const ResidualSel rs;
  const int c8n = ldp / 8;
  const long long total = M * c8n;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long r = i / c8n;
    const int c = (int)(i - r * c8n) * 8;
    f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = {0.f, 0.f, 0.f, 0.f};
    if (c < C) v0 = *reinterpret_cast<const f32x4*>(x + r * ldx + c);
    if (c + 4 < C) v1 = *reinterpret_cast<const f32x4*>(x + r * ldx + c + 4);
    u32x2 l0[2], l1[2];
    split4n<2>(v0, l0, rs);
    split4n<2>(v1, l1, rs);
    *reinterpret_cast<u32x4*>(hi + r * ldp + c) = u32x4{l0[0][0], l0[0][1], l1[0][0], l1[0][1]};
    *reinterpret_cast<u32x4*>(lo + r * ldp + c) = u32x4{l0[1][0], l0[1][1], l1[1][0], l1[1][1]};
  }
}

// w[Cout][taps][Cin] -> wT[Cin][taps][Cout]   (32x32 LDS tile per tap)
__global__ __launch_bounds__(256) void filter_transpose_kernel(const float* __restrict__ w, float* __restrict__ wT,
                                                               int Cout, int taps, int Cin) {
  PSEG_HELPER_PRIO();
  __shared__ float tile[32][33];
  const int t = blockIdx.z;
  const int ci0 = blockIdx.x * 32, co0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  for (int r = ty; r < 32; r += 8) {
    const int co = co0 + r, ci = ci0 + tx;
    tile[r][tx] = (co < Cout && ci < Cin) ? w[((long long)co * taps + t) * Cin + ci] : 0.f;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int ci = ci0 + r, co = co0 + tx;
    if (ci < Cin && co < Cout) wT[((long long)ci * taps + t) * Cout + co] = tile[tx][r];
  }
}

// debug: per-block phase timestamps of gather_f32_dma_kernel (pseg_debug_conv_trace; tools/conv_phases.py)
static unsigned long long* g_conv_trace = nullptr;

// pre-split bf16 limb planes of both operands of a gather GEMM (see gather_limb_dma_kernel)
struct LimbPlanes {
  const uint16_t* xh;
  const uint16_t* xl;
  const uint16_t* wh;
  const uint16_t* wl;
  int ldxp;
  long long xp_bytes, wp_bytes;
};

// The tiles of the exact-fp32 LDS-DMA kernels, stated once: select_gather reads from this table what each family covers, the
// launch helpers below map an entry to template arguments.  gather_f32_dma_kernel (plain and GENERIC) is instantiated for every
// entry, gather_f32_pw_kernel / gather_f32_halo_kernel for those marked.  Threads per block = 64 * wm * wn.
struct F32Tile {
  int bm, bn, wm, wn;
  bool pw;       // persistent pointwise kernel
  int halo;      // halo-staged kernel: the lowest PSEG_CONV_HALO that takes the tile (0: not instantiated)
};
constexpr F32Tile kF32Tiles[] = {{128, 128, 2, 4, true, 0},
                                 {128, 64, 2, 2, true, 2},
                                 {64, 128, 2, 2, true, 0},
                                 {128, 32, 4, 1, false, 1}};   // narrow outputs (HRNet's 32-channel branch, the 21-class classifier)
constexpr int kNumF32Tiles = (int)(sizeof(kF32Tiles) / sizeof(kF32Tiles[0]));

static int f32_tile_index(TileCfg t) {
  for (int i = 0; i < kNumF32Tiles; ++i)
    if (kF32Tiles[i].bm == t.bm && kF32Tiles[i].bn == t.bn) return i;
  return -1;
}

template <typename F>
static void with_f32_tile(int i, F&& f) {
  with_index(i, f, std::make_integer_sequence<int, kNumF32Tiles>{});
}

// A gather problem as run_gather sees it: the geometry plus what the caller asks of the kernel.
struct GatherProblem : GatherGeom {
  int precision;
  bool stats, bias, planes, bns, accumulate;   // fused statistics / bias / pre-split limb planes / fused BatchNorm-backward sums
};

constexpr int kPwMaxKSteps = 32;     // longest contraction, in K-steps, that the persistent pointwise kernel is offered
constexpr int kGatherRefused = 0;    // GatherChoice::kernel: no kernel carries the limb planes / fused sums asked for

// Everything run_gather decides before it launches; the queries read their answers off the same choice.
struct GatherChoice {
  FwdPlan pl;
  RowOrder order;   // (row_perm == 4: the classes are pl.band)
  int kernel;       // PSEG_KERNEL_GATHER_* that runs -- after the pointwise kernel declined, if try_pw -- or kGatherRefused
  int f32_tile;     // entry of kF32Tiles (ring, pointwise and halo kernels)
  int stages;       // ring depth of gather_f32_dma_kernel
  bool generic;     // ... and its GENERIC form
  bool try_pw;      // offer the problem to the persistent pointwise kernel first; launch_pw declines by device occupancy
  int stat_rows() const { return pl.gridM * waves_m(pl.tile); }
};

// The one place that picks the kernel of an exact-fp32 / limb gather conv.  Pure: launches nothing, touches no device.
static GatherChoice select_gather(const GatherProblem& q) {
  GatherChoice c;
  DilGeom geom;
  const bool has_geom = dil_geom(geom, q.Ho, q.Wo, q.Hi, q.Wi, q.taps_h, q.taps_w, q.Cin, q.s_out, q.s_in, q.dstep, q.off0);
  // the 256x128 / 8-wave tile (one block per CU) of the limb kernels: measured 1 % SLOWER in the round-2 training step than
  // two 128-row blocks per CU (mixed policy 35.85 vs 35.45 ms) -- only forced (PSEG_CONV_FORCEBIG); the pre-split DMA kernel
  // is built on it
  const bool allow_big = !q.stats && (q.precision == 1 || q.precision == 3) && (q.planes || cfg().conv_forcebig != 0);
  c.pl = plan_gather(q.M, q.N, q.K, allow_big, has_geom ? &geom : nullptr);
  const FwdPlan& pl = c.pl;
  const bool whole = q.Cin % BK == 0;    // whole K-steps inside a tap
  c.order = gather_row_order(q, pl, whole, whole && pl.splits == 1);
  c.kernel = q.bns ? kGatherRefused : PSEG_KERNEL_GATHER_REGISTER;
  c.f32_tile = f32_tile_index(pl.tile);
  c.stages = 0;
  c.generic = c.try_pw = false;
  if (q.planes) {
    // the LDS-DMA limb kernel or nothing: whole K-steps inside a tap, the 256x128 tile, no split-K
    const bool ok = q.precision == 1 && !q.stats && !q.bias && !q.bns && pl.tile.bm == kDmaBM && pl.tile.bn == kDmaBN &&
                    pl.splits == 1 && whole && q.N >= kDmaBN;
    c.kernel = ok ? PSEG_KERNEL_GATHER_LIMB_DMA : kGatherRefused;
    return c;
  }
  if (!(q.precision == 0 && pl.splits == 1 && cfg().conv_f32dma != 0 && c.f32_tile >= 0)) return c;
  const F32Tile& t = kF32Tiles[c.f32_tile];
  const bool sk = c.order.skip_taps != 0;
  const int taps = q.taps_h * q.taps_w;
  if (!whole && q.Cin % 4 == 0 && !sk && (c.order.row_perm == 0 || c.order.row_perm == 3) && !q.bns) {
    // channel counts off the K-step grid (stem, classifier data gradient, MobileNetV2 widths): the GENERIC form of the ring
    // kernel with per-slot (tap, channel) derivation; two-stage ring
    c.kernel = PSEG_KERNEL_GATHER_RING_GENERIC;
    c.stages = 2;
    c.generic = true;
    return c;
  }
  // Exact-fp32 problems whose K-steps never straddle a tap run on the LDS-DMA kernel (same tile, same statistics
  // layout).  PSEG_CONV_F32DMA: 3 (default) = two-stage ring for every such problem, 2 = only for those without tap
  // skipping (51.0 -> 49.4 ms; the tap-skipping ASPP / stride-2 problems add 49.0 -> 48.4) -- 64 / 48 KB of LDS
  // and ~100 VGPRs, so TWO blocks of 8 waves (128x128) or THREE of 4 (128x64) share a CU and one block's prologue /
  // epilogue hides behind the others' MFMAs: medium and short-K layers +5-10 % (128x128 maps, 64 channels: 98 -> 109 TF),
  // fp32 step 51.0 -> 49.4 ms; 1 = three-stage ring everywhere (one block per CU: equal to the register-staged kernel in
  // the step); 0 = register-staged kernel only.  The large layers sit at the sustained fp32-MFMA rate either way.
  if (!(whole && q.K % BK == 0 && taps <= 32 && !(cfg().conv_f32dma == 2 && sk))) return c;
  if (q.bns && q.accumulate) return c;      // (the fused sums are those of the tile written, not of what it is added to)
  // pointwise convs with short contractions and more tiles than the device holds blocks: the persistent kernel
  // (PSEG_CONV_PW=0: off)
  c.try_pw = t.pw && cfg().conv_pw != 0 && c.order.row_perm == 3 && !sk && pl.kt_total <= kPwMaxKSteps && cfg().conv_f32dma >= 2;
  // narrow 3x3: the halo-staged kernel where the map is made of whole 8 x 16 patches (see gather_f32_halo_kernel)
  const int halo = cfg().conv_halo;
  if (halo != 0 && t.halo != 0 && (t.halo == 1 || halo >= t.halo) && !sk && taps == 9 && q.taps_w == 3 && q.s_out == 1 &&
      q.s_in == 1 && (q.dstep == 1 || q.dstep == -1) && q.off0 == -q.dstep && q.Cin % 32 == 0 && q.Hi == q.Ho && q.Wi == q.Wo &&
      q.Ho % kHaloPH == 0 && q.Wo % kHaloPW == 0 && c.order.row_perm == 0) {
    c.kernel = PSEG_KERNEL_GATHER_HALO;
    c.order.row_perm = 2;
    c.order.patch_w = kHaloPW;
    c.order.patch_hw = kHaloPH * kHaloPW;
    c.order.patches_per_row = q.Wo / kHaloPW;
    return c;
  }
  c.kernel = PSEG_KERNEL_GATHER_RING;
  c.stages = cfg().conv_f32dma >= 2 ? 2 : 3;   // two-stage ring: 64 / 48 KB of LDS, 2 / 3 blocks per CU
  return c;
}

// The register-staged kernel: five tiles x SKIP x four arithmetics; the 256x128 tile (8 waves, one block per CU) exists for the
// LDS-staging-bound two-limb variants.  [SKIP][tile_slot]; nullptr = not instantiated.
typedef void (*GatherFn)(const GatherConvParams);
typedef GatherFn GatherFnTable[2][6];
static const GatherFnTable& register_kernels(int precision) {
#define PSEG_GATHER_ROW(SK, PR, BIG)                                                                   \
  {gather_conv_kernel<128, 128, 2, 2, SK, PR>, gather_conv_kernel<128, 64, 2, 2, SK, PR>,              \
   gather_conv_kernel<128, 32, 4, 1, SK, PR>, gather_conv_kernel<64, 128, 2, 2, SK, PR>,               \
   gather_conv_kernel<32, 128, 1, 4, SK, PR>, BIG}
  static const GatherFnTable fns32 = {PSEG_GATHER_ROW(false, 0, nullptr), PSEG_GATHER_ROW(true, 0, nullptr)};
  static const GatherFnTable fnsb3 = {PSEG_GATHER_ROW(false, 1, (gather_conv_kernel<256, 128, 4, 2, false, 1>)),
                                      PSEG_GATHER_ROW(true, 1, (gather_conv_kernel<256, 128, 4, 2, true, 1>))};
  static const GatherFnTable fnsb6 = {PSEG_GATHER_ROW(false, 2, nullptr), PSEG_GATHER_ROW(true, 2, nullptr)};
  static const GatherFnTable fnsh3 = {PSEG_GATHER_ROW(false, 3, (gather_conv_kernel<256, 128, 4, 2, false, 3>)),
                                      PSEG_GATHER_ROW(true, 3, (gather_conv_kernel<256, 128, 4, 2, true, 3>))};
#undef PSEG_GATHER_ROW
  return precision == 3 ? fnsh3 : precision == 2 ? fnsb6 : precision == 1 ? fnsb3 : fns32;
}

// The record of a gather choice (pseg_debug_last_gather, pseg_conv2d_gather_choice; layout: pseg_amd.h): tile, SKIP flag, ring
// depth, GENERIC flag, row order and K split as the launch reads them off the choice; `kernel` and `precision` as launched (the
// pointwise kernel's code once it accepted; the arithmetic the kernel runs with, not the caller's request).
constexpr int kGatherRecord = 13;
static thread_local int g_last_gather[kGatherRecord] = {};
static void gather_record(int* out, const GatherChoice& c, int kernel, int precision, bool bns) {
  const bool ring = kernel == PSEG_KERNEL_GATHER_RING || kernel == PSEG_KERNEL_GATHER_RING_GENERIC;
  const bool patches = c.order.row_perm == 2;
  const int rec[kGatherRecord] = {kernel, c.pl.tile.bm, c.pl.tile.bn, precision, c.order.skip_taps != 0 ? 1 : 0, ring ? c.stages : 0,
                                  c.generic ? 1 : 0, c.order.row_perm, patches ? c.order.patch_hw / c.order.patch_w : 0,
                                  patches ? c.order.patch_w : 0, c.pl.splits, bns ? 1 : 0, c.try_pw ? 1 : 0};
  for (int i = 0; i < kGatherRecord; ++i) out[i] = rec[i];
}

// the arithmetic a choice runs with: the register-staged kernel has every one, the others are fixed
static int gather_precision(const GatherChoice& c, int precision) {
  return c.kernel == PSEG_KERNEL_GATHER_REGISTER ? precision : (c.kernel == PSEG_KERNEL_GATHER_LIMB_DMA ? 1 : 0);
}

template <int I, bool SKIP, int STAGES, bool GENERIC>
static void launch_ring_as(dim3 grid, hipStream_t st, const GatherConvParams& p) {
  constexpr F32Tile t = kF32Tiles[I];
  hipLaunchKernelGGL((gather_f32_dma_kernel<t.bm, t.bn, t.wm, t.wn, SKIP, STAGES, GENERIC>), grid, dim3(64 * t.wm * t.wn), 0, st, p);
}

static void launch_ring(const GatherChoice& c, dim3 grid, hipStream_t st, const GatherConvParams& p) {
  const bool sk = c.order.skip_taps != 0, two = c.stages == 2;
  with_f32_tile(c.f32_tile, [&](auto tile) {
    constexpr int I = decltype(tile)::value;
    if (c.generic) launch_ring_as<I, false, 2, true>(grid, st, p);
    else if (two && sk) launch_ring_as<I, true, 2, false>(grid, st, p);
    else if (two) launch_ring_as<I, false, 2, false>(grid, st, p);
    else if (sk) launch_ring_as<I, true, 3, false>(grid, st, p);
    else launch_ring_as<I, false, 3, false>(grid, st, p);
  });
}

static void launch_halo(const GatherChoice& c, dim3 grid, hipStream_t st, const GatherConvParams& p) {
  with_f32_tile(c.f32_tile, [&](auto tile) {
    constexpr F32Tile t = kF32Tiles[decltype(tile)::value];
    if constexpr (t.halo != 0) hipLaunchKernelGGL((gather_f32_halo_kernel<t.wm, t.wn>), grid, dim3(64 * t.wm * t.wn), 0, st, p);
  });
}

// one instantiation of the persistent pointwise kernel: grid = the blocks the device holds at once; 0 = launched, 1 = not worth it
// (fewer tiles than resident blocks: every block would own one tile) or not launchable
template <int BM, int BN, int WM, int WN>
static int launch_pw(int ntiles, hipStream_t st, const GatherConvParams& p) {
  static int resident = 0;
  if (resident == 0) {
    int per_cu = 0, dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, gather_f32_pw_kernel<BM, BN, WM, WN, false>, 64 * WM * WN, 0) != hipSuccess ||
        per_cu < 1) {
      resident = -1;
    } else {
      constexpr long long lds_bytes = (2LL * (BM + BN) * 32 + WM * WN * 8 * (BN / WN + 4)) * 4;
      const int by_lds = (int)((160 * 1024) / lds_bytes);
      if (per_cu > by_lds) per_cu = by_lds;
      resident = prop.multiProcessorCount * per_cu;
    }
  }
  int grid = resident;
  if (cfg().conv_pw_resident > 0) grid = cfg().conv_pw_resident;      // (tests: several tiles per block on small problems)
  if (grid <= 0 || ntiles <= grid) return 1;
  if (p.bns_y != nullptr)
    hipLaunchKernelGGL((gather_f32_pw_kernel<BM, BN, WM, WN, true>), dim3((unsigned)grid), dim3(64 * WM * WN), 0, st, p, ntiles);
  else
    hipLaunchKernelGGL((gather_f32_pw_kernel<BM, BN, WM, WN, false>), dim3((unsigned)grid), dim3(64 * WM * WN), 0, st, p, ntiles);
  return 0;
}

static int launch_pointwise(const GatherChoice& c, hipStream_t st, const GatherConvParams& p) {
  int rc = 1;
  with_f32_tile(c.f32_tile, [&](auto tile) {
    constexpr F32Tile t = kF32Tiles[decltype(tile)::value];
    if constexpr (t.pw) rc = launch_pw<t.bm, t.bn, t.wm, t.wn>(c.pl.gridM * c.pl.gridN, st, p);
  });
  return rc;
}

// validate, select, fill the parameters from the choice and launch
static int run_gather(const GatherGeom& g, const float* x, long long x_bytes, int ldx, const float* w, float* y, int ldy,
                      const float* bias, float* stat, int accumulate, int precision, const unsigned* amax_a,
                      const unsigned* amax_b, void* workspace, int64_t workspace_bytes, hipStream_t st,
                      const LimbPlanes* planes = nullptr, const BnsArgs* bns = nullptr) {
  const long long M = g.M;
  const int N = g.N, K = g.K, Cin = g.Cin;
  PSEG_REQUIRE(M > 0 && M < (1LL << 31) && N > 0 && K > 0, "conv: empty or oversized problem M=%lld N=%d K=%d", M, N, K);
  PSEG_REQUIRE(Cin % 4 == 0 && ldx % 4 == 0, "conv: Cin (%d) and ldx (%d) must be multiples of 4", Cin, ldx);
  PSEG_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)w & 15) == 0, "conv: x / w must be 16-byte aligned");
  const long long w_bytes = (long long)N * K * 4;
  PSEG_REQUIRE(x_bytes < kMaxBytes && w_bytes < kMaxBytes, "conv: tensor exceeds 2 GiB (x %lld, w %lld bytes)", x_bytes,
               w_bytes);
  PSEG_REQUIRE(((M - 1) * ldy + N) * 4 < (1LL << 40), "conv: output too large");

  const GatherChoice c = select_gather(GatherProblem{g, precision, stat != nullptr, bias != nullptr, planes != nullptr,
                                                     bns != nullptr, accumulate != 0});
  const FwdPlan& pl = c.pl;
  if (stat != nullptr && pl.splits > 1) {
    set_error("conv2d_fwd: fused statistics are unavailable when the plan splits K; use pseg_col_stats");
    return PSEG_ERR_ARG;
  }
  if (planes != nullptr && c.kernel != PSEG_KERNEL_GATHER_LIMB_DMA) {
    set_error("conv: the pre-split (LDS-DMA) limb kernel does not cover this problem (M=%lld N=%d K=%d Cin=%d)", M, N, K, Cin);
    return PSEG_ERR_ARG;
  }

  GatherConvParams p;
  p.x = x;
  p.w = w;
  p.bias = bias;
  p.stat = stat;
  p.stat_rows = c.stat_rows();
  p.x_bytes = (uint32_t)x_bytes;
  p.w_bytes = (uint32_t)w_bytes;
  p.ldx = ldx;
  set_gather_geometry(p, g, pl, c.order);
  p.ktiles_per_tap = Cin / BK;
  const dim3 grid((unsigned)(pl.gridM * pl.gridN), 1, (unsigned)pl.splits);
  if (pl.splits == 1) {
    p.y = y;
    p.ldy = ldy;
    p.accumulate = accumulate;
    p.slab_stride = 0;
  } else {
    const long long need = (long long)pl.splits * M * N * 4;
    if (workspace == nullptr || workspace_bytes < need) {
      set_error("conv: split-K needs %lld workspace bytes, got %lld", need, (long long)workspace_bytes);
      return PSEG_ERR_WORKSPACE;
    }
    p.y = (float*)workspace;
    p.ldy = N;
    p.accumulate = 0;
    p.bias = nullptr;
    p.stat = nullptr;
    p.slab_stride = M * N;
  }
  p.trace = g_conv_trace;
  p.xh = p.xl = p.wh = p.wl = nullptr;
  p.xp_bytes = p.wp_bytes = 0;
  p.ldxp = 0;
  // only the exact-fp32 LDS-DMA kernels carry the fused sums: the caller asked pseg_conv2d_dgrad_bnstat_rows first
  if (bns != nullptr && (c.kernel == kGatherRefused || bns->rows != c.stat_rows())) {
    set_error("conv: the fused BatchNorm-backward sums are not available for this data gradient (M=%lld N=%d K=%d, rows %d)", M, N,
              K, bns->rows);
    return PSEG_ERR_ARG;
  }
  set_bns_params(p, bns);
  const bool reg = c.kernel == PSEG_KERNEL_GATHER_REGISTER;     // the one kernel with every arithmetic; the others are fixed
  p.precision = gather_precision(c, precision);
  p.amax_a = reg ? amax_a : nullptr;
  p.amax_b = reg ? amax_b : nullptr;
  if (reg && precision == 3 && (amax_a == nullptr || amax_b == nullptr)) {
    set_error("conv: PSEG_PREC_FP16X3 needs the amax of both operands");
    return PSEG_ERR_ARG;
  }
  if (planes != nullptr) {
    PSEG_REQUIRE(planes->xp_bytes < kMaxBytes && planes->wp_bytes < kMaxBytes && planes->ldxp % 8 == 0 &&
                     ((uintptr_t)planes->xh & 15) == 0 && ((uintptr_t)planes->xl & 15) == 0 &&
                     ((uintptr_t)planes->wh & 15) == 0 && ((uintptr_t)planes->wl & 15) == 0,
                 "conv: limb planes must be 16-byte aligned, ld %% 8 == 0, < 2 GiB");
    p.xh = planes->xh;
    p.xl = planes->xl;
    p.wh = planes->wh;
    p.wl = planes->wl;
    p.xp_bytes = (uint32_t)planes->xp_bytes;
    p.wp_bytes = (uint32_t)planes->wp_bytes;
    p.ldxp = planes->ldxp;
  }
  if (c.try_pw && launch_pointwise(c, st, p) == 0) {
    g_last_conv_kernel = PSEG_KERNEL_GATHER_POINTWISE;
    gather_record(g_last_gather, c, PSEG_KERNEL_GATHER_POINTWISE, p.precision, bns != nullptr);
    PSEG_LAUNCH_CHECK();
    return PSEG_OK;
  }
  g_last_conv_kernel = c.kernel;
  switch (c.kernel) {
    case PSEG_KERNEL_GATHER_LIMB_DMA:
      if (p.skip_taps) hipLaunchKernelGGL(gather_limb_dma_kernel<true>, grid, dim3(512), 0, st, p);
      else hipLaunchKernelGGL(gather_limb_dma_kernel<false>, grid, dim3(512), 0, st, p);
      break;
    case PSEG_KERNEL_GATHER_RING_GENERIC:
      p.gen_spt = FastDiv((uint32_t)(Cin / 4));
      p.gen_kw = FastDiv((uint32_t)g.taps_w);
      launch_ring(c, grid, st, p);
      break;
    case PSEG_KERNEL_GATHER_RING:
      launch_ring(c, grid, st, p);
      break;
    case PSEG_KERNEL_GATHER_HALO:
      launch_halo(c, grid, st, p);
      break;
    default: {
      const int rc = launch_tiles<GatherConvParams, GatherFn, 6>(register_kernels(precision), p.skip_taps != 0, pl.tile, grid, p, st);
      if (rc != PSEG_OK) return rc;
      gather_record(g_last_gather, c, c.kernel, p.precision, false);
      if (pl.splits > 1) return launch_slab_reduce((const float*)workspace, M * N, pl.splits, y, ldy, M, N, bias, accumulate, st);
      return PSEG_OK;
    }
  }
  gather_record(g_last_gather, c, c.kernel, p.precision, bns != nullptr);
  PSEG_LAUNCH_CHECK();
  return PSEG_OK;
}

}  // namespace pseg

using namespace pseg;

extern "C" {

int pseg_debug_conv_trace(void* buffer) {
  if (!kConvTrace && buffer != nullptr) {
    pseg::set_error("debug_conv_trace: the library was built without -DPSEG_CONV_TRACE=1 (PSEG_BUILD_TRACE=1 ... build --force)");
    return PSEG_ERR_ARG;
  }
  pseg::g_conv_trace = (unsigned long long*)buffer;
  return PSEG_OK;
}

// the choice of a forward conv with fused statistics (the queries know Ho / Wo only: the smallest input that gives them)
static GatherChoice select_fwd_stats(int B, int Ho, int Wo, int Cin, int Cout, int kh, int kw, int stride, int pad, int dil) {
  return select_gather(GatherProblem{fwd_stats_geom(B, Ho, Wo, Cin, Cout, kh, kw, stride, pad, dil), PSEG_PREC_FP32, true, false,
                                     false, false, false});
}

int pseg_conv2d_stat_rows(int B, int Ho, int Wo, int Cin, int Cout, int kh, int kw, int stride, int pad, int dil) {
  return select_fwd_stats(B, Ho, Wo, Cin, Cout, kh, kw, stride, pad, dil).stat_rows();
}

int pseg_conv2d_stat_group(int B, int Ho, int Wo, int Cin, int Cout, int kh, int kw, int stride, int pad, int dil) {
  const TileCfg t = select_fwd_stats(B, Ho, Wo, Cin, Cout, kh, kw, stride, pad, dil).pl.tile;
  return t.bm / waves_m(t);
}

int64_t pseg_conv2d_fwd_workspace_bytes(int B, int Ho, int Wo, int Cin, int Cout, int kh, int kw) {
  const long long M = (long long)B * Ho * Wo;
  // plans without geometry (the signature has no stride / dilation): geometry only swaps tiles among plans of >= 256 tiles, never splits
  FwdPlan pl = plan_gather(M, Cout, kh * kw * Cin);
  return pl.splits > 1 ? (int64_t)pl.splits * M * Cout * 4 : 0;
}

int pseg_conv2d_fwd(const float* x, int ldx, const float* w, const float* bias, float* y, int ldy, int B, int H, int W,
                    int Cin, int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad, int dil, int accumulate,
                    int precision, const float* amax_x, const float* amax_w, float* stat, void* workspace,
                    int64_t workspace_bytes, void* stream) {
  PSEG_REQUIRE(x && w && y, "conv2d_fwd: null pointer");
  const int rc = check_fwd_geometry("conv2d_fwd", H, W, Ho, Wo, kh, kw, stride, pad, dil);
  if (rc != PSEG_OK) return rc;
  PSEG_REQUIRE(precision >= 0 && precision <= 3, "conv2d_fwd: precision must be one of PSEG_PREC_*");
  return run_gather(fwd_geom(B, H, W, Cin, Ho, Wo, Cout, kh, kw, stride, pad, dil), x, nhwc_bytes(B, H, W, Cin, ldx), ldx, w, y, ldy,
                    bias, stat, accumulate, precision, (const unsigned*)amax_x, (const unsigned*)amax_w, workspace,
                    workspace_bytes, (hipStream_t)stream);
}

int pseg_conv2d_dgrad(const float* dy, int ldy, const float* wT, float* dx, int ldx, int B, int H, int W, int Cin, int Ho,
                      int Wo, int Cout, int kh, int kw, int stride, int pad, int dil, int accumulate, int precision,
                      const float* amax_dy, const float* amax_w, void* workspace, int64_t workspace_bytes,
                      void* stream) {
  PSEG_REQUIRE(dy && wT && dx, "conv2d_dgrad: null pointer");
  PSEG_REQUIRE(precision >= 0 && precision <= 3, "conv2d_dgrad: precision must be one of PSEG_PREC_*");
  PSEG_REQUIRE(stride >= 1 && dil >= 1 && pad >= 0, "conv2d_dgrad: bad geometry");
  return run_gather(dgrad_geom(B, H, W, Cin, Ho, Wo, Cout, kh, kw, stride, pad, dil), dy, nhwc_bytes(B, Ho, Wo, Cout, ldy), ldy, wT,
                    dx, ldx, nullptr, nullptr, accumulate, precision, (const unsigned*)amax_dy, (const unsigned*)amax_w,
                    workspace, workspace_bytes, (hipStream_t)stream);
}

int pseg_conv2d_dgrad_bnstat_rows(int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad,
                                  int dil) {
  if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || kh <= 0 || kw <= 0 || kh * kw > 32 || Cin % 4 != 0) return 0;
  if ((long long)B * H * W >= (1LL << 31)) return 0;
  // the problem pseg_conv2d_dgrad_bnstat hands to run_gather: 0 unless a kernel that carries the fused sums takes it
  const GatherChoice c = select_gather(GatherProblem{dgrad_geom(B, H, W, Cin, Ho, Wo, Cout, kh, kw, stride, pad, dil), PSEG_PREC_FP32,
                                                     false, false, false, true, false});
  return c.kernel == kGatherRefused ? 0 : c.stat_rows();
}

int pseg_conv2d_dgrad_bnstat(const float* dy, int ldy, const float* wT, float* dx, int ldx, int B, int H, int W, int Cin, int Ho,
                             int Wo, int Cout, int kh, int kw, int stride, int pad, int dil, const float* y_prev, int ldy_prev,
                             const float* mean, const float* invstd, const float* scale, const float* shift, int act,
                             float* part_db, float* part_dg, int part_rows, void* stream) {
  const BnsArgs bns{y_prev, ldy_prev, mean, invstd, scale, shift, act, part_db, part_dg, part_rows};
  const int rc = check_dgrad_bnstat_args("conv2d_dgrad_bnstat", 4, dy, wT, dx, Cin, stride, pad, dil, bns);
  if (rc != PSEG_OK) return rc;
  PSEG_REQUIRE(part_rows > 0 && part_rows == pseg_conv2d_dgrad_bnstat_rows(B, H, W, Cin, Ho, Wo, Cout, kh, kw, stride, pad, dil),
               "conv2d_dgrad_bnstat: part_rows (%d) is not pseg_conv2d_dgrad_bnstat_rows() of this problem (0 = not covered)",
               part_rows);
  return run_gather(dgrad_geom(B, H, W, Cin, Ho, Wo, Cout, kh, kw, stride, pad, dil), dy, nhwc_bytes(B, Ho, Wo, Cout, ldy), ldy, wT,
                    dx, ldx, nullptr, nullptr, 0, PSEG_PREC_FP32, nullptr, nullptr, nullptr, 0, (hipStream_t)stream, nullptr, &bns);
}

int pseg_split_planes(const float* x, int ldx, int64_t M, int C, uint16_t* hi, uint16_t* lo, int ldp, void* stream) {
  PSEG_REQUIRE(x && hi && lo && M > 0 && C > 0, "split_planes: bad argument");
  PSEG_REQUIRE(C % 4 == 0 && ldx % 4 == 0 && ldp % 8 == 0 && ldp >= C, "split_planes: C %% 4, ldx %% 4, ldp %% 8, ldp >= C");
  PSEG_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)hi & 15) == 0 && ((uintptr_t)lo & 15) == 0, "split_planes: alignment");
  const long long total = (long long)M * (ldp / 8);
  const int blocks = (int)(total / 256 + 1 < 8192 ? total / 256 + 1 : 8192);
  hipLaunchKernelGGL(split_planes_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, ldx, (long long)M, C, hi, lo,
                     ldp);
  PSEG_LAUNCH_CHECK();
  return PSEG_OK;
}

int pseg_conv2d_dgrad_planes_ok(int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad,
                                int dil) {
  if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return 0;
  // the problem pseg_conv2d_dgrad_planes hands to run_gather
  const GatherChoice c = select_gather(GatherProblem{dgrad_geom(B, H, W, Cin, Ho, Wo, Cout, kh, kw, stride, pad, dil),
                                                     PSEG_PREC_BF16X3, false, false, true, false, false});
  return c.kernel == PSEG_KERNEL_GATHER_LIMB_DMA ? 1 : 0;
}

int pseg_conv2d_dgrad_planes(const uint16_t* dy_hi, const uint16_t* dy_lo, int ldp, const uint16_t* wT_hi,
                             const uint16_t* wT_lo, float* dx, int ldx, int B, int H, int W, int Cin, int Ho, int Wo,
                             int Cout, int kh, int kw, int stride, int pad, int dil, int accumulate, void* stream) {
  PSEG_REQUIRE(dy_hi && dy_lo && wT_hi && wT_lo && dx, "conv2d_dgrad_planes: null pointer");
  PSEG_REQUIRE(stride >= 1 && dil >= 1 && pad >= 0 && ldp >= Cout, "conv2d_dgrad_planes: bad geometry");
  const GatherGeom g = dgrad_geom(B, H, W, Cin, Ho, Wo, Cout, kh, kw, stride, pad, dil);
  LimbPlanes pln{dy_hi, dy_lo, wT_hi, wT_lo, ldp, (((long long)B * Ho * Wo - 1) * ldp + Cout) * 2, (long long)Cin * g.K * 2};
  // (x / w of run_gather are unused on this path; pass the planes for the alignment checks)
  return run_gather(g, reinterpret_cast<const float*>(dy_hi), 16, 4, reinterpret_cast<const float*>(wT_hi), dx, ldx, nullptr,
                    nullptr, accumulate, PSEG_PREC_BF16X3, nullptr, nullptr, nullptr, 0, (hipStream_t)stream, &pln);
}

int pseg_debug_last_gather(int* out13) {
  PSEG_REQUIRE(out13 != nullptr, "debug_last_gather: null pointer");
  for (int i = 0; i < kGatherRecord; ++i) out13[i] = g_last_gather[i];
  return PSEG_OK;
}

int pseg_conv2d_gather_choice(int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad, int dil,
                              int dgrad, int precision, int stats, int bias, int planes, int bns, int accumulate, int* out13) {
  PSEG_REQUIRE(out13 != nullptr, "conv2d_gather_choice: null pointer");
  PSEG_REQUIRE(B > 0 && H > 0 && W > 0 && Cin > 0 && Ho > 0 && Wo > 0 && Cout > 0 && kh > 0 && kw > 0 && stride > 0 && pad >= 0 &&
                   dil > 0 && precision >= 0 && precision <= 3 && (dgrad ? Cout : Cin) % 4 == 0 &&
                   (long long)B * (dgrad ? H * (long long)W : Ho * (long long)Wo) < (1LL << 31),
               "conv2d_gather_choice: bad geometry or precision (the gathered channels come in fours)");
  if (!dgrad) {
    const int rc = check_fwd_geometry("conv2d_gather_choice", H, W, Ho, Wo, kh, kw, stride, pad, dil);
    if (rc != PSEG_OK) return rc;
  }
  const GatherGeom g = dgrad ? dgrad_geom(B, H, W, Cin, Ho, Wo, Cout, kh, kw, stride, pad, dil)
                             : fwd_geom(B, H, W, Cin, Ho, Wo, Cout, kh, kw, stride, pad, dil);
  // the problem run_gather builds from the same arguments, and its choice
  GatherChoice c = select_gather(GatherProblem{g, precision, stats != 0, bias != 0, planes != 0, bns != 0, accumulate != 0});
  // what run_gather refuses on the choice alone: fused statistics of a plan that splits K, a tile the register-staged kernel is
  // not instantiated for in this arithmetic
  if (stats != 0 && c.pl.splits > 1) c.kernel = kGatherRefused;
  if (c.kernel == PSEG_KERNEL_GATHER_REGISTER) {
    const int slot = tile_slot(c.pl.tile, 6);
    if (slot < 0 || register_kernels(precision)[c.order.skip_taps != 0 ? 1 : 0][slot] == nullptr) c.kernel = kGatherRefused;
  }
  gather_record(out13, c, c.kernel, gather_precision(c, precision), bns != 0 && c.kernel != kGatherRefused);
  return PSEG_OK;
}

// All filters of a model in ONE launch: jobs[j] = {w, wT, Cout, taps, Cin, first 32x32 tile of job j} (6 x int64, device
// memory, tile offsets ascending); block b finds its job by bisection.
__global__ __launch_bounds__(256) void filter_transpose_batch_kernel(const long long* __restrict__ jobs, int n) {
  PSEG_HELPER_PRIO();
  __shared__ float tile[32][33];
  const long long b = blockIdx.x;
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[mid * 6 + 5] <= b) lo = mid;
    else hi = mid - 1;
  }
  const long long* job = jobs + lo * 6;
  const float* w = reinterpret_cast<const float*>(job[0]);
  float* wT = reinterpret_cast<float*>(job[1]);
  const int Cout = (int)job[2], taps = (int)job[3], Cin = (int)job[4];
  const int tci = (Cin + 31) / 32, tco = (Cout + 31) / 32;
  int local = (int)(b - job[5]);
  const int t = local / (tci * tco);
  local -= t * tci * tco;
  if (t >= taps) return;
  const int co0 = (local / tci) * 32, ci0 = (local % tci) * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8) {
    const int co = co0 + r, ci = ci0 + tx;
    tile[r][tx] = (co < Cout && ci < Cin) ? w[((long long)co * taps + t) * Cin + ci] : 0.f;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int ci = ci0 + r, co = co0 + tx;
    if (ci < Cin && co < Cout) wT[((long long)ci * taps + t) * Cout + co] = tile[tx][r];
  }
}

int pseg_filter_transpose_batch(const int64_t* jobs, int n, int64_t total_tiles, void* stream) {
  PSEG_REQUIRE(jobs && n > 0 && total_tiles > 0 && total_tiles < (1LL << 31), "filter_transpose_batch: bad argument");
  hipLaunchKernelGGL(filter_transpose_batch_kernel, dim3((unsigned)total_tiles), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const long long*>(jobs), n);
  PSEG_LAUNCH_CHECK();
  return PSEG_OK;
}

int pseg_filter_transpose(const float* w, float* wT, int Cout, int taps, int Cin, void* stream) {
  PSEG_REQUIRE(w && wT && Cout > 0 && taps > 0 && Cin > 0, "filter_transpose: bad argument");
  PSEG_REQUIRE(taps <= 65535, "filter_transpose: too many taps");
  dim3 grid((unsigned)cdiv(Cin, 32), (unsigned)cdiv(Cout, 32), (unsigned)taps);
  hipLaunchKernelGGL(filter_transpose_kernel, grid, dim3(256), 0, (hipStream_t)stream, w, wT, Cout, taps, Cin);
  PSEG_LAUNCH_CHECK();
  return PSEG_OK;
}

}  // extern "C"
