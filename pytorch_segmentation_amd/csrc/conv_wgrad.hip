// Weight gradient of every dense conv on the hot path, on v_mfma_f32_32x32x2_f32 (exact fp32) or bf16 limbs, and the
// fixed-order reduction of split slabs (the gather side -- forward, data gradient: conv_gather.hip).
//
//  wgrad_kernel        dW[Cout][K] = dY[P][Cout]^T * A[P][K],  both operands K(=pixel)-strided.
//
// Tile, K-step and the register-staged double buffer are those of gather_conv_kernel (conv_gather.hip).
//
// LDS image:
//  wgrad: [32 pixels][cols] floats, read with ds_read_b32 (32 consecutive floats per half-wave); all fragments of
//     half a step are fetched before its MFMAs so LDS latency is paid once per 16*TM*TN... MFMAs, not per 4.
#include "conv_common.h"
#include "conv_limb.h"

namespace pseg {

template <int BM, int BN, int WARPS_M, int WARPS_N, bool SKIP>
__global__ __launch_bounds__(256) void wgrad_kernel(const WgradParams p) {
  static_assert(WARPS_M * WARPS_N == 4, "4 waves");
  constexpr int WTM = BM / WARPS_M, WTN = BN / WARPS_N;
  constexpr int TM = WTM / 32, TN = WTN / 32;
  static_assert(TM >= 1 && TN >= 1 && WTM % 32 == 0 && WTN % 32 == 0, "wave tile");
  constexpr int CPR_A = BM / 4, CPR_B = BN / 4;            // 16-byte chunks per pixel row
  constexpr int RPP_A = 256 / CPR_A, RPP_B = 256 / CPR_B;  // pixel rows covered per pass
  constexpr int AR = (BK + RPP_A - 1) / RPP_A, BR = (BK + RPP_B - 1) / RPP_B;

  constexpr int kStage = 2 * BK * (BM + BN), kPatch = 4 * WTM * (WTN + 4);
  __shared__ __attribute__((aligned(16))) float lds[kStage > kPatch ? kStage : kPatch];
  float* As = lds;                // [2][BK][BM]   (dy^T tile)
  float* Bs = lds + 2 * BK * BM;  // [2][BK][BN]   (gathered x tile)

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WARPS_N, wn = wave % WARPS_N;
  const int gridN = (p.K + BN - 1) / BN;
  int wg_tile, wg_split;
  wgrad_block((int)gridDim.x, wg_tile, wg_split);
  const int tile_n = wg_tile % gridN;
  const int tile_m = wg_tile / gridN;
  const int m0 = tile_m * BM, n0 = tile_n * BN;

  const __amdgpu_buffer_rsrc_t xr = make_rsrc(p.x, p.x_bytes);
  const __amdgpu_buffer_rsrc_t dr = make_rsrc(p.dy, p.dy_bytes);

  const int ca = tid % CPR_A, pra = tid / CPR_A;
  const int cb = tid % CPR_B, prb = tid / CPR_B;
  const int a_col = m0 + ca * 4;
  const bool a_cok = a_col < p.Cout;
  const int b_col = n0 + cb * 4;
  const bool b_cok = b_col < p.K;
  int b_dh, b_dw, b_c;
  {
    const int kk = b_cok ? b_col : 0;
    const int tap = kk / p.Cin;
    b_c = kk - tap * p.Cin;
    const int r = tap / p.kw;
    const int s = tap - r * p.kw;
    b_dh = r * p.dil - p.pad;
    b_dw = s * p.dil - p.pad;
  }

  const int p_begin = wg_split * p.pix_per_split;
  int p_end = p_begin + p.pix_per_split;
  if (p_end > p.P) p_end = p.P;

  // ---- pixel walkers: slot i of this thread gathers pixel pt + prb + RPP_B*i of K-step pt.  (b, ho, wo) is decoded
  // by division only when the walk jumps (start, skipped steps); consecutive steps advance by BK pixels with carries.
  int w_ho[BR], w_wo[BR], w_img[BR];
  const int himg = p.Hi * p.Wi;
  int w_pt = -1;  // K-step the walkers currently point at
  const bool patch = p.patch_mode != 0;
  // patch mode: in-patch coordinates of this thread's rows are constants; a K-step adds a block-uniform origin
  int a_rel[AR], b_rel[BR], b_hh[BR], b_ww[BR];
#pragma unroll
  for (int i = 0; i < AR; ++i) {
    const int row = pra + RPP_A * i;
    a_rel[i] = ((row / p.patch_w) * p.Wo + row % p.patch_w) * p.ldy + a_col;
  }
#pragma unroll
  for (int i = 0; i < BR; ++i) {
    const int row = prb + RPP_B * i;
    b_hh[i] = (row / p.patch_w) * p.stride + b_dh;
    b_ww[i] = (row % p.patch_w) * p.stride + b_dw;
    b_rel[i] = (b_hh[i] * p.Wi + b_ww[i]) * p.ldx + b_c;
  }
  auto seek = [&](int pt) {
#pragma unroll
    for (int i = 0; i < BR; ++i) {
      const int pix = pt + prb + RPP_B * i;
      const int b = pix / p.HoWo;
      const int rem = pix - b * p.HoWo;
      w_ho[i] = rem / p.Wo;
      w_wo[i] = rem - w_ho[i] * p.Wo;
      w_img[i] = b * himg;
    }
    w_pt = pt;
  };

  // block-uniform: is K-step [pt, pt+BK) pure padding for this block's tap?
  const int t_dh = (n0 / p.Cin / p.kw) * p.dil - p.pad;
  const int t_dw = ((n0 / p.Cin) % p.kw) * p.dil - p.pad;
  auto step_dead = [&](int pt) -> bool { return wg_step_dead(p, pt, p_end, t_dh, t_dw); };
  auto next_valid = [&](int pt) -> int {
    if (SKIP)
      while (pt < p_end && step_dead(pt)) pt += BK;
    return pt;
  };

  f32x4 areg[AR], breg[BR];

  auto load_tile = [&](int pt) {
    if (patch) {
      // whole K-steps only (P, pix_per_split multiples of 32): no pixel-tail tests
      int pb, h0, w0;
      wg_patch_origin(p, pt, pb, h0, w0);
      const int a_base = ((pb * p.Ho + h0) * p.Wo + w0) * p.ldy;
      const int hs = h0 * p.stride, ws = w0 * p.stride;
      const int b_base = ((pb * p.Hi + hs) * p.Wi + ws) * p.ldx;
#pragma unroll
      for (int i = 0; i < AR; ++i) {
        const bool ok = (pra + RPP_A * i < BK) && a_cok;
        areg[i] = buf_load4(dr, ok ? (uint32_t)((a_base + a_rel[i]) * 4) : kOOB);
      }
#pragma unroll
      for (int i = 0; i < BR; ++i) {
        const bool ok = (prb + RPP_B * i < BK) && b_cok && ((unsigned)(hs + b_hh[i]) < (unsigned)p.Hi) &&
                        ((unsigned)(ws + b_ww[i]) < (unsigned)p.Wi);
        breg[i] = buf_load4(xr, ok ? (uint32_t)((b_base + b_rel[i]) * 4) : kOOB);
      }
      return;
    }
    if (SKIP) {
      if (pt != w_pt) seek(pt);
    } else if (w_pt < 0) {
      seek(pt);
    }
#pragma unroll
    for (int i = 0; i < AR; ++i) {
      const int row = pra + RPP_A * i;
      const int pix = pt + row;
      const bool ok = (row < BK) && a_cok && (pix < p_end);
      const uint32_t off = ok ? (uint32_t)((pix * p.ldy + a_col) * 4) : kOOB;
      areg[i] = buf_load4(dr, off);
    }
#pragma unroll
    for (int i = 0; i < BR; ++i) {
      const int row = prb + RPP_B * i;
      const int pix = pt + row;
      const int hi = w_ho[i] * p.stride + b_dh;
      const int wi = w_wo[i] * p.stride + b_dw;
      const bool ok = (row < BK) && b_cok && (pix < p_end) && ((unsigned)hi < (unsigned)p.Hi) &&
                      ((unsigned)wi < (unsigned)p.Wi);
      const uint32_t off = ok ? (uint32_t)(((w_img[i] + hi * p.Wi + wi) * p.ldx + b_c) * 4) : kOOB;
      breg[i] = buf_load4(xr, off);
      // advance this walker by BK pixels
      w_wo[i] += BK;
      while (w_wo[i] >= p.Wo) {
        w_wo[i] -= p.Wo;
        if (++w_ho[i] == p.Ho) {
          w_ho[i] = 0;
          w_img[i] += himg;
        }
      }
    }
    w_pt = pt + BK;
  };

  auto store_tile = [&](int buf) {
#pragma unroll
    for (int i = 0; i < AR; ++i) {
      const int row = pra + RPP_A * i;
      if (row < BK) *reinterpret_cast<f32x4*>(&As[(buf * BK + row) * BM + ca * 4]) = areg[i];
    }
#pragma unroll
    for (int i = 0; i < BR; ++i) {
      const int row = prb + RPP_B * i;
      if (row < BK) *reinterpret_cast<f32x4*>(&Bs[(buf * BK + row) * BN + cb * 4]) = breg[i];
    }
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int frag_col = lane & 31;
  const int frag_h = lane >> 5;

  // Same three-tile pipeline as the gather kernel: tile `cur` is multiplied from LDS buffer `buf`, `nxt` is complete in
  // buf^1, `stg` waits in the staging registers (its global loads were issued one whole K-step earlier).  Two fragment
  // sets alternate between the 16-pixel halves of a K-step: the ds_read_b32 words of the next half are fetched under the
  // current MFMA burst, the barrier has no data to wait for, and the staged tile is written + the tile after it requested
  // under the second burst.
  // Operands TM / TN at a time: MFMA tile i of the wave takes rows TM*t + i (t = lane & 31), so one ds_read_b32 / b64 /
  // b128 per k delivers the lane's operand for ALL TM row tiles (same for the TN column tiles).  A half-step is then 16
  // LDS reads for TM = TN = 2 instead of 32 ds_read_b32 -- the LGKM counter holds 15 outstanding operations, and the
  // second half of a 32-read burst used to stall the wave in front of its MFMAs.  (The output rows / columns are mapped
  // back in the epilogue: store_tiles<..., IL = true>.)
  typedef float fvm __attribute__((ext_vector_type(TM)));
  typedef float fvn __attribute__((ext_vector_type(TN)));
  float fa[2][8][TM], fb[2][8][TN];
  auto read_frags = [&](int set, int buf, int half) {
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int kk = half * 16 + 2 * s + frag_h;
      if constexpr (TM == 1) {
        fa[set][s][0] = As[(buf * BK + kk) * BM + wm * WTM + frag_col];
      } else {
        const fvm v = *reinterpret_cast<const fvm*>(&As[(buf * BK + kk) * BM + wm * WTM + TM * frag_col]);
#pragma unroll
        for (int i = 0; i < TM; ++i) fa[set][s][i] = v[i];
      }
      if constexpr (TN == 1) {
        fb[set][s][0] = Bs[(buf * BK + kk) * BN + wn * WTN + frag_col];
      } else {
        const fvn v = *reinterpret_cast<const fvn*>(&Bs[(buf * BK + kk) * BN + wn * WTN + TN * frag_col]);
#pragma unroll
        for (int j = 0; j < TN; ++j) fb[set][s][j] = v[j];
      }
    }
  };
  auto mfmas = [&](int set) {
#pragma unroll
    for (int s = 0; s < 8; ++s)
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[set][s][i], fb[set][s][j], acc[i][j], 0, 0, 0);
  };

  {
    const int t0 = next_valid(p_begin);
    if (t0 < p_end) {
      load_tile(t0);
      store_tile(0);
      int cur = t0, nxt = next_valid(t0 + BK), stg = p_end;
      if (nxt < p_end) {
        load_tile(nxt);
        store_tile(1);
        stg = next_valid(nxt + BK);
        if (stg < p_end) load_tile(stg);
      }
      if (nxt > p_end) nxt = p_end;
      if (stg > p_end) stg = p_end;
      __syncthreads();
      read_frags(0, 0, 0);
      int buf = 0;
      while (cur < p_end) {
        int after = p_end;
        if (stg < p_end) {
          after = next_valid(stg + BK);
          if (after > p_end) after = p_end;
        }
        read_frags(1, buf, 1);
        __builtin_amdgcn_sched_barrier(0);
        mfmas(0);
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();
        read_frags(0, buf ^ 1, 0);   // (garbage on the last step: never multiplied)
        __builtin_amdgcn_sched_barrier(0);
        if (stg < p_end) store_tile(buf);
        if (after < p_end) load_tile(after);
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

  float* out = p.dw + (long long)wg_split * p.slab_stride;
  {
    float* patch = lds + wave * (WTM * (WTN + 4));
    const int row0 = m0 + wm * WTM, col0 = n0 + wn * WTN;
    int rv = p.Cout - row0, cv = p.K - col0;
    rv = rv < 0 ? 0 : (rv > WTM ? WTM : rv);
    cv = cv < 0 ? 0 : (cv > WTN ? WTN : cv);
    store_tiles<TM, TN, true>(acc, patch, out, p.K, row0, col0, rv, cv, nullptr, p.accumulate != 0, lane,
                        [](int m) { return m; });
  }
}

// ------------------------------------------------------------------------------------------------
// Exact-fp32 weight gradient staged by LDS-DMA.  The LDS image of wgrad_kernel -- [32 pixels][BM] / [32 pixels][BN] floats
// -- is exactly how the operands lie in memory (a pixel's channels are contiguous), so `buffer_load_dwordx4 ... lds`
// fills it without any swizzle: one wave-instruction = 1 KiB = 1024 / (4*BM) whole pixel rows.  No staging registers, no
// ds_write; two-stage ring, 8 waves per block and ~100 VGPRs: two blocks (16 waves) share a CU where the register-staged
// kernel has 8 waves, which is what hides a block's prologue / slab epilogue behind the other's MFMAs.
// Pixel order of the contraction: patch mode only (host-checked: p.patch_mode, whole 32-pixel K-steps).
// Round 5: (a) the pieces of a K-step are dealt in 16-byte CHUNK order -- chunk 64 * piece + lane of the [32 px][BN] image -- so a
// tile's pixel row need not be a whole number of pieces: 32 x 288 on NINE waves takes the whole 3x3 filter of a 32-channel layer
// (HRNet's fine branch) as ONE column tile, dy fetched once per K-step instead of once per 128 columns; (b) skip_rows == 4: pixels
// in plain row-major order with each lane deriving its pixel by two divisions -- maps that do not tile into 32-pixel patches
// no longer fall back to the register-staged kernel.
template <int BM, int BN, int WARPS_M, int WARPS_N, bool SKIP>
__global__ __launch_bounds__(64 * WARPS_M * WARPS_N) void wgrad_f32_dma_kernel(const WgradParams p) {
  static_assert(WARPS_M * WARPS_N == 8 || WARPS_M * WARPS_N == 9, "8 or 9 waves");
  constexpr int NW = WARPS_M * WARPS_N;
  constexpr int WTM = BM / WARPS_M, WTN = BN / WARPS_N;
  constexpr int TM = WTM / 32, TN = WTN / 32;
  static_assert(TM >= 1 && TN >= 1 && WTM % 32 == 0 && WTN % 32 == 0, "wave tile");
  constexpr int kStageF = BK * (BM + BN);
  constexpr int kPatch = NW * WTM * (WTN + 4);
  __shared__ __attribute__((aligned(16))) float lds[2 * kStageF > kPatch ? 2 * kStageF : kPatch];
  constexpr int kA = 0, kB = BK * BM;                           // inside a stage
  // DMA pieces: RA / RB pixel rows per wave-instruction, IA / IB instructions per wave and K-step
  constexpr int RA = 256 / BM;                                  // dy rows per piece: 1024 B / (4*BM B per row)
  constexpr int CB = BN / 4;                                    // 16-byte chunks per x row
  // pieces per K-step: PA of dy, PB of x, dealt round-robin over the waves (piece q = wave + NW * g).  A 32-row tile has
  // PA = 4 < NW: waves 0..3 carry one dy piece each, the others none -- the per-wave DMA count is wave-uniform, not block-uniform
  constexpr int PA = BK / RA, PB = BK * CB / 64;
  constexpr int IA = (PA + NW - 1) / NW, IB = (PB + NW - 1) / NW;
  static_assert(PA >= 1 && PB >= 1 && BK % RA == 0 && (BK * CB) % 64 == 0 && (PA % NW == 0 || PA < NW) && PB % NW == 0, "pieces per wave");
  constexpr bool kAPartial = PA < NW;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WARPS_N, wn = wave % WARPS_N;
  const int gridN = (p.K + BN - 1) / BN;
  int wg_tile, wg_split;
  wgrad_block((int)gridDim.x, wg_tile, wg_split);
  int tile_n = wg_tile % gridN;
  const int tile_m = wg_tile / gridN;
  if (SKIP && p.lpt_per > 0) {
    // longest-first order of the column tiles (see WgradParams::lpt_per)
    const int tpt = p.Cin / BN, ntap = p.K / p.Cin, grp = ntap * p.lpt_per;
    const int h = tile_n / grp, rem = tile_n - h * grp;
    const int rank = rem / p.lpt_per, c = rem - rank * p.lpt_per;
    tile_n = p.tap_order[rank] * tpt + h * p.lpt_per + c;
  }
  const int m0 = tile_m * BM, n0 = tile_n * BN;

  const __amdgpu_buffer_rsrc_t xr = make_rsrc(p.x, p.x_bytes);
  const __amdgpu_buffer_rsrc_t dr = make_rsrc(p.dy, p.dy_bytes);

  int p_begin = wg_split * p.pix_per_split;
  int p_end = p_begin + p.pix_per_split;
  if (p_end > p.P) p_end = p.P;
  // packed contraction (skip_rows == 3): the live rectangle of this block's tap, block-uniform
  const bool packed = SKIP && p.skip_rows == kWgPacked;
  int pk_r0 = 0, pk_c0 = 0, pk_total = 0, pk_dh = 0, pk_dw = 0;
  FastDiv pk_area_div, pk_lw_div;
  if (packed) {
    const int tap = n0 / p.Cin;
    pk_dh = (tap / p.kw) * p.dil - p.pad;
    pk_dw = (tap % p.kw) * p.dil - p.pad;
    pk_r0 = pk_dh < 0 ? -pk_dh : 0;
    pk_c0 = pk_dw < 0 ? -pk_dw : 0;
    int r1 = p.Hi - pk_dh, c1 = p.Wi - pk_dw;
    r1 = r1 > p.Ho ? p.Ho : r1;
    c1 = c1 > p.Wo ? p.Wo : c1;
    const int lh = r1 > pk_r0 ? r1 - pk_r0 : 0, lw = c1 > pk_c0 ? c1 - pk_c0 : 0;
    const int area = lh * lw;
    pk_total = (p.P / p.HoWo) * area;
    pk_area_div = FastDiv((uint32_t)(area > 0 ? area : 1));
    pk_lw_div = FastDiv((uint32_t)(lw > 0 ? lw : 1));
    const int steps = (pk_total + BK - 1) / BK, nsplit = (int)gridDim.z;
    const int per = (steps + nsplit - 1) / nsplit;
    p_begin = wg_split * per * BK;
    p_end = p_begin + per * BK;
    if (p_end > steps * BK) p_end = steps * BK;
    if (p_begin > p_end) p_begin = p_end;
  }

  // ---- per-lane constants of the DMA pieces (patch mode: K-step origin + these)
  int a_rel[IA];      // float offset inside dy relative to the K-step's first pixel, or -1 (column beyond Cout)
  int b_rel[IB], b_hh[IB], b_ww[IB];
#pragma unroll
  for (int g = 0; g < IA; ++g) {
    const int row = RA * (wave + NW * g) + lane / (BM / 4);       // pixel row of the K-step
    const int col = m0 + 4 * (lane % (BM / 4));
    a_rel[g] = col < p.Cout ? ((row / p.patch_w) * p.Wo + row % p.patch_w) * p.ldy + col : -1;
    if (packed) a_rel[g] = col < p.Cout ? col : -1;               // (packed: the column; the pixel comes per K-step)
  }
  const bool rowmajor = p.skip_rows == kWgRowMajorDma;      // plain pixel order, per-lane pixel derivation (no patches)
  int b_prow[IB];                              // pixel row (0..31) of the K-step this lane's chunk of piece g belongs to
#pragma unroll
  for (int g = 0; g < IB; ++g) {
    const int ci = 64 * (wave + NW * g) + lane;                   // chunk of the [32 px][BN] image
    const int row = ci / CB;
    const int col = n0 + 4 * (ci - row * CB);
    b_prow[g] = row;
    if (col < p.K) {
      const int tap = col / p.Cin;
      const int c = col - tap * p.Cin;
      const int r = tap / p.kw, sx = tap - r * p.kw;
      b_hh[g] = (row / p.patch_w) * p.stride + r * p.dil - p.pad;
      b_ww[g] = (row % p.patch_w) * p.stride + sx * p.dil - p.pad;
      b_rel[g] = (b_hh[g] * p.Wi + b_ww[g]) * p.ldx + c;
      if (packed) b_rel[g] = c;                                   // (packed: the channel inside the block's tap)
      if (rowmajor) {                                             // (row-major: the tap's offsets and the channel)
        b_hh[g] = r * p.dil - p.pad;
        b_ww[g] = sx * p.dil - p.pad;
        b_rel[g] = c;
      }
    } else {
      b_hh[g] = b_ww[g] = -(1 << 28);     // never in range
      b_rel[g] = (packed || rowmajor) ? -1 : 0;
    }
  }
  if (rowmajor) {
#pragma unroll
    for (int g = 0; g < IA; ++g) {
      const int col = m0 + 4 * (lane % (BM / 4));
      a_rel[g] = col < p.Cout ? col : -1;
    }
  }

  const int t_dh = (n0 / p.Cin / p.kw) * p.dil - p.pad;
  const int t_dw = ((n0 / p.Cin) % p.kw) * p.dil - p.pad;
  auto next_valid = [&](int pt) -> int {
    if (SKIP && !packed)
      while (pt < p_end && wg_step_dead(p, pt, p_end, t_dh, t_dw)) pt += BK;
    return pt;
  };

  typedef __attribute__((address_space(3))) void* lds_ptr;
  // packed pixel q of this block's tap -> float offsets of its dy pixel and of its source pixel (always inside the image)
  auto packed_pixel = [&](int q, int& a_pix, int& b_pix) {
    const uint32_t b = pk_area_div.div((uint32_t)q);
    const uint32_t rem = (uint32_t)q - b * pk_area_div.d;
    const uint32_t hh = pk_lw_div.div(rem);
    const uint32_t ww = rem - hh * pk_lw_div.d;
    const int ho = pk_r0 + (int)hh, wo = pk_c0 + (int)ww;
    a_pix = (((int)b * p.Ho + ho) * p.Wo + wo) * p.ldy;
    b_pix = (((int)b * p.Hi + ho + pk_dh) * p.Wi + wo + pk_dw) * p.ldx;
  };
  auto issue = [&](int pt, int st) {     // pt >= p_end: all-zero dummy pieces
    float* sb = lds + st * kStageF;
    if (packed) {
      const bool live_step = pt < p_end;
#pragma unroll
      for (int g = 0; g < IA; ++g) {
        if (kAPartial && wave >= PA) break;
        const int q = pt + RA * (wave + NW * g) + lane / (BM / 4);
        int a_pix, b_pix;
        packed_pixel(q < pk_total ? q : 0, a_pix, b_pix);
        const uint32_t off = (live_step && q < pk_total && a_rel[g] >= 0) ? (uint32_t)((a_pix + a_rel[g]) * 4) : kOOB;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(dr, (lds_ptr)(sb + kA + RA * (wave + NW * g) * BM), 16, (int)off, 0, 0, 0);
      }
#pragma unroll
      for (int g = 0; g < IB; ++g) {
        const int q = pt + b_prow[g];
        int a_pix, b_pix;
        packed_pixel(q < pk_total ? q : 0, a_pix, b_pix);
        const uint32_t off = (live_step && q < pk_total && b_rel[g] >= 0) ? (uint32_t)((b_pix + b_rel[g]) * 4) : kOOB;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(xr, (lds_ptr)(sb + kB + 256 * (wave + NW * g)), 16, (int)off, 0, 0, 0);
      }
      return;
    }
    if (rowmajor) {
      // pixel pt + row of the [B, Ho, Wo] raster, by two divisions per piece; pixels at or past p_end read nothing
      auto pixel = [&](int q, int& b, int& ho, int& wo) {
        const uint32_t bb = p.rm_howo.div((uint32_t)q);
        const uint32_t rem = (uint32_t)q - bb * p.rm_howo.d;
        const uint32_t hh = p.rm_wo.div(rem);
        b = (int)bb;
        ho = (int)hh;
        wo = (int)(rem - hh * p.rm_wo.d);
      };
#pragma unroll
      for (int g = 0; g < IA; ++g) {
        if (kAPartial && wave >= PA) break;
        const int q = pt + RA * (wave + NW * g) + lane / (BM / 4);
        int b, ho, wo;
        pixel(q < p_end ? q : 0, b, ho, wo);
        const uint32_t off = (q < p_end && a_rel[g] >= 0) ? (uint32_t)((((b * p.Ho + ho) * p.Wo + wo) * p.ldy + a_rel[g]) * 4) : kOOB;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(dr, (lds_ptr)(sb + kA + RA * (wave + NW * g) * BM), 16, (int)off, 0, 0, 0);
      }
#pragma unroll
      for (int g = 0; g < IB; ++g) {
        const int q = pt + b_prow[g];
        int b, ho, wo;
        pixel(q < p_end ? q : 0, b, ho, wo);
        const int hi = ho * p.stride + b_hh[g], wi = wo * p.stride + b_ww[g];
        const bool ok = q < p_end && b_rel[g] >= 0 && ((unsigned)hi < (unsigned)p.Hi) && ((unsigned)wi < (unsigned)p.Wi);
        const uint32_t off = ok ? (uint32_t)((((b * p.Hi + hi) * p.Wi + wi) * p.ldx + b_rel[g]) * 4) : kOOB;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(xr, (lds_ptr)(sb + kB + 256 * (wave + NW * g)), 16, (int)off, 0, 0, 0);
      }
      return;
    }
    int pb = 0, h0 = 0, w0 = 0;
    const bool live = pt < p_end;
    if (live) wg_patch_origin(p, pt, pb, h0, w0);
    const int a_base = ((pb * p.Ho + h0) * p.Wo + w0) * p.ldy;
    const int hs = h0 * p.stride, ws = w0 * p.stride;
    const int b_base = ((pb * p.Hi + hs) * p.Wi + ws) * p.ldx;
#pragma unroll
    for (int g = 0; g < IA; ++g) {
      if (kAPartial && wave >= PA) break;      // (wave-uniform)
      const uint32_t off = (live && a_rel[g] >= 0) ? (uint32_t)((a_base + a_rel[g]) * 4) : kOOB;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(dr, (lds_ptr)(sb + kA + RA * (wave + NW * g) * BM), 16, (int)off, 0, 0, 0);
    }
#pragma unroll
    for (int g = 0; g < IB; ++g) {
      const bool ok = live && ((unsigned)(hs + b_hh[g]) < (unsigned)p.Hi) && ((unsigned)(ws + b_ww[g]) < (unsigned)p.Wi);
      const uint32_t off = ok ? (uint32_t)((b_base + b_rel[g]) * 4) : kOOB;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(xr, (lds_ptr)(sb + kB + 256 * (wave + NW * g)), 16, (int)off, 0, 0, 0);
    }
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int frag_col = lane & 31;
  const int frag_h = lane >> 5;
  typedef float fvm __attribute__((ext_vector_type(TM)));
  typedef float fvn __attribute__((ext_vector_type(TN)));
  float fa[2][8][TM], fb[2][8][TN];
  auto read_frags = [&](int set, int st, int half) {
    const float* sb = lds + st * kStageF;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int kk = half * 16 + 2 * s + frag_h;
      if constexpr (TM == 1) {
        fa[set][s][0] = sb[kA + kk * BM + wm * WTM + frag_col];
      } else {
        const fvm v = *reinterpret_cast<const fvm*>(&sb[kA + kk * BM + wm * WTM + TM * frag_col]);
#pragma unroll
        for (int i = 0; i < TM; ++i) fa[set][s][i] = v[i];
      }
      if constexpr (TN == 1) {
        fb[set][s][0] = sb[kB + kk * BN + wn * WTN + frag_col];
      } else {
        const fvn v = *reinterpret_cast<const fvn*>(&sb[kB + kk * BN + wn * WTN + TN * frag_col]);
#pragma unroll
        for (int j = 0; j < TN; ++j) fb[set][s][j] = v[j];
      }
    }
  };
  auto mfmas = [&](int set) {
#pragma unroll
    for (int s = 0; s < 8; ++s)
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[set][s][i], fb[set][s][j], acc[i][j], 0, 0, 0);
  };

  {
    int q0 = next_valid(p_begin);
    if (q0 < p_end) {
      int q1 = next_valid(q0 + BK);
      issue(q0, 0);
      issue(q1, 1);
      int q2 = q1 < p_end ? next_valid(q1 + BK) : p_end;
      // K-step q0 has landed (this wave's share), q1 stays in flight: all but the youngest (pieces of this wave per K-step)
      if constexpr (kAPartial) {
        static_assert(IA == 1 && IB == 4, "partial-A tile: 5 or 4 pieces per wave");      // (32x256 on 8 waves, 32x288 on 9)
        if (wave < PA) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      } else if constexpr (IA + IB == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      else if constexpr (IA + IB == 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      read_frags(0, 0, 0);
      int st = 0;
      while (q0 < p_end) {
        read_frags(1, st, 1);
        __builtin_amdgcn_sched_barrier(0);
        mfmas(0);
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // the next K-step has landed
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave is done reading stage `st`
        __builtin_amdgcn_s_barrier();
        read_frags(0, st ^ 1, 0);     // (zeros on the last step: never multiplied)
        __builtin_amdgcn_sched_barrier(0);
        issue(q2, st);                // stage `st` is free now
        mfmas(1);
        __builtin_amdgcn_sched_barrier(0);
        q0 = q1;
        q1 = q2;
        q2 = q2 < p_end ? next_valid(q2 + BK) : p_end;
        st ^= 1;
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // dummy pieces must not land in the output patches
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
  }

  float* out = p.dw + (long long)wg_split * p.slab_stride;
  {
    float* patch = lds + wave * (WTM * (WTN + 4));
    const int row0 = m0 + wm * WTM, col0 = n0 + wn * WTN;
    int rv = p.Cout - row0, cv = p.K - col0;
    rv = rv < 0 ? 0 : (rv > WTM ? WTM : rv);
    cv = cv < 0 ? 0 : (cv > WTN ? WTN : cv);
    store_tiles<TM, TN, true>(acc, patch, out, p.K, row0, col0, rv, cv, nullptr, p.accumulate != 0, lane,
                              [](int m) { return m; });
  }
}

// ------------------------------------------------------------------------------------------------
// Split-bf16 weight gradient.  dW[Cout][K] = dY^T * A with the contraction over pixels; the bf16 MFMA wants 8 consecutive
// k (= pixels) per lane, but both operands arrive pixel-major (4 consecutive CHANNELS per 16-byte load).  Each loader
// thread therefore takes one 4-channel chunk of 8 consecutive pixels (8 loads), transposes them in registers into four
// 8-pixel runs, splits each run into NL bf16 limbs and writes them as 16-byte k-slots of the channel-major LDS image
// ([row = channel or K-column][32 pixels], same swizzle as the gather kernel).  Threads [0, BM) load dY^T, threads
// [256-BN, 256) gather A; the MFMA block, pixel-split slabs, row skipping and epilogue are those of the fp32 kernel.
// ------------------------------------------------------------------------------------------------
// HALO-STAGED weight gradient of a 3x3 (unit stride, dilation 1, padding 1) for NARROW filters, exact fp32 (round 5).
// wgrad_f32_dma_kernel<32, 288, 1, 9> fetches the x operand of a 32-pixel K-step as nine shifted copies -- [32 px][9 taps x 32 ch] =
// 36 KB + 4 KB of dy for 1024 matrix cycles of each of its nine waves: 40 bytes per clock and CU against an LDS-DMA path that
// sustains ~27 -- and a 32 / 64-row tile has no other way to be wide.  Here a K-step is a 2 x 16 STRIP of output pixels; x comes in
// ONCE per K-step as the 4 x 18 halo strip of a 32-channel chunk (9 KB), dy as [32 px][BM] (4 / 8 KB), and wave t (tap t) reads its
// B fragments from the halo strip at its tap's shift: dw[co][t][ci] += sum_p dy[p][co] x[p + t][ci].  Nine waves = nine taps, each
// with BM x 32 accumulators; a block = (row tile of BM filters, one 32-channel chunk of the input, one pixel split).  13 / 17 KB
// per K-step, 41 KB of LDS (the nine epilogue patches).  Same pixel splits / slabs / reduction as wgrad_f32_dma_kernel.
//   LDS reads are single dwords (pixel-major images, as wgrad_f32_dma_kernel): lanes 0-31 = 32 consecutive floats of one pixel
//   row, lanes 32-63 of the NEXT pixel (k = 2 s + (lane >> 5)): adjacent pixels are adjacent 128-byte rows -- the two halves of the
//   64 banks -- at every tap shift (18 is even), so no swizzle.
template <int BM>
__global__ __launch_bounds__(576) void wgrad_f32_halo_kernel(const WgradParams p) {
  constexpr int NW = 9, TM = BM / 32;
  static_assert(BM == 32 || BM == 64, "row tile");
  constexpr int kHS = 4 * 18;                                  // halo strip pixels
  constexpr int kA = 0, kB = BK * BM, kStageF = BK * BM + kHS * 32;
  constexpr int kPatch = NW * 32 * 36;
  __shared__ __attribute__((aligned(16))) float lds[2 * kStageF > kPatch ? 2 * kStageF : kPatch];
  // DMA pieces per K-step: dy rows of BM floats (BM * 4 bytes): 1024 / (4 BM) pixel rows per wave-instruction -> NA instructions
  constexpr int RA = 256 / BM, NA = BK / RA;                   // 8 rows, 4 instructions (BM = 32) / 4 rows, 8 instructions (64)
  static_assert(NA <= NW, "one dy piece per wave at most");

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int gridN = p.Cin >> 5;
  int wg_tile, wg_split;
  wgrad_block((int)gridDim.x, wg_tile, wg_split);
  const int tile_n = wg_tile % gridN, tile_m = wg_tile / gridN;
  const int m0 = tile_m * BM, c0 = tile_n * 32;

  const __amdgpu_buffer_rsrc_t xr = make_rsrc(p.x, p.x_bytes);
  const __amdgpu_buffer_rsrc_t dr = make_rsrc(p.dy, p.dy_bytes);
  const int p_begin = wg_split * p.pix_per_split;
  int p_end = p_begin + p.pix_per_split;
  if (p_end > p.P) p_end = p.P;

  // this lane's share of a K-step's DMAs, relative to the strip's top-left output pixel (h0, w0) of image b
  int a_rel = -1;                                              // dy: float offset, or -1 (no piece / column beyond Cout)
  if (wave < NA) {
    const int row = RA * wave + lane / (BM / 4);               // pixel of the strip: (row >> 4, row & 15)
    const int col = m0 + 4 * (lane % (BM / 4));
    if (col < p.Cout) a_rel = ((row >> 4) * p.Wo + (row & 15)) * p.ldy + col;
  }
  const int hidx = 8 * wave + (lane >> 3);                     // halo pixel (hidx / 18 - 1, hidx % 18 - 1) relative to (h0, w0)
  const int h_dh = hidx / 18 - 1, h_dw = hidx % 18 - 1;
  const int h_rel = (h_dh * p.Wi + h_dw) * p.ldx + c0 + 4 * (lane & 7);
  typedef __attribute__((address_space(3))) void* lds_ptr;
  unsigned* ldsw = reinterpret_cast<unsigned*>(lds);
  auto issue = [&](int pt, int st) {
    unsigned* sb = ldsw + st * kStageF;
    const bool live = pt < p_end;
    int pb = 0, h0 = 0, w0 = 0;
    if (live) wg_patch_origin(p, pt, pb, h0, w0);
    if (wave < NA) {                                           // (wave-uniform)
      const uint32_t off = (live && a_rel >= 0) ? (uint32_t)((((pb * p.Ho + h0) * p.Wo + w0) * p.ldy + a_rel) * 4) : kOOB;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(dr, (lds_ptr)(sb + kA + RA * wave * BM), 16, (int)off, 0, 0, 0);
    }
    const bool ok = live && ((unsigned)(h0 + h_dh) < (unsigned)p.Hi) && ((unsigned)(w0 + h_dw) < (unsigned)p.Wi);
    const uint32_t off = ok ? (uint32_t)((((pb * p.Hi + h0) * p.Wi + w0) * p.ldx + h_rel) * 4) : kOOB;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(xr, (lds_ptr)(sb + kB + 8 * wave * 32), 16, (int)off, 0, 0, 0);
  };

  f32x16 acc[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

  const int frag_col = lane & 31, frag_h = lane >> 5;
  const int tr = wave / 3, ts = wave - 3 * tr;                 // this wave's tap: x pixel = output pixel + (tr - 1, ts - 1)
  float fa[2][8][TM], fb[2][8];
  auto read_frags = [&](int set, int st, int half) {
    const float* sb = lds + st * kStageF;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int kk = half * 16 + 2 * s + frag_h;               // pixel of the strip: (half, 2 s + frag_h)
#pragma unroll
      for (int i = 0; i < TM; ++i) fa[set][s][i] = sb[kA + kk * BM + i * 32 + frag_col];
      fb[set][s] = sb[kB + ((half + tr) * 18 + (2 * s + frag_h) + ts) * 32 + frag_col];
    }
  };
  auto mfmas = [&](int set) {
#pragma unroll
    for (int s = 0; s < 8; ++s)
#pragma unroll
      for (int i = 0; i < TM; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[set][s][i], fb[set][s], acc[i], 0, 0, 0);
  };

  if (p_begin < p_end) {
    int q0 = p_begin;
    issue(q0, 0);
    issue(q0 + BK, 1);
    // K-step q0 has landed (this wave's share) when only the second K-step's pieces of this wave are outstanding
    if (wave < NA) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    read_frags(0, 0, 0);
    int st = 0;
    while (q0 < p_end) {
      read_frags(1, st, 1);
      __builtin_amdgcn_sched_barrier(0);
      mfmas(0);
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // the next K-step has landed
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave is done reading stage `st`
      __builtin_amdgcn_s_barrier();
      read_frags(0, st ^ 1, 0);     // (zeros past the end: never multiplied)
      __builtin_amdgcn_sched_barrier(0);
      issue(q0 + 2 * BK, st);       // stage `st` is free now
      mfmas(1);
      __builtin_amdgcn_sched_barrier(0);
      q0 += BK;
      st ^= 1;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // dummy pieces must not land in the output patches
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }

  float* out = p.dw + (long long)wg_split * p.slab_stride;
  float* patch = lds + wave * (32 * 36);
  const int col0 = wave * p.Cin + c0;                          // K index of (tap, channel): tap * Cin + channel
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int row0 = m0 + i * 32;
    int rv = p.Cout - row0;
    rv = rv < 0 ? 0 : (rv > 32 ? 32 : rv);
    const f32x16 (&acc1)[1][1] = reinterpret_cast<const f32x16 (&)[1][1]>(acc[i]);
    store_tiles<1, 1>(acc1, patch, out, p.K, row0, col0, rv, 32, nullptr, p.accumulate != 0, lane, [](int m) { return m; });
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();                           // the patch is rewritten by the next row half
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  }
}

template <int NL>
__device__ __forceinline__ void split8n(float (&v)[8], u32x4 (&limb)[NL], const ResidualSel& rs) {
#pragma unroll
  for (int l = 0; l < NL; ++l) {
    unsigned pk[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      pk[q] = pack_bf16(v[2 * q], v[2 * q + 1]);
      if (l + 1 < NL) {
        v[2 * q] = resid_lo(pk[q], v[2 * q], rs);
        v[2 * q + 1] = resid_hi(pk[q], v[2 * q + 1], rs);
      }
    }
    limb[l] = u32x4{pk[0], pk[1], pk[2], pk[3]};
  }
}

template <int BM, int BN, int WARPS_M, int WARPS_N, bool SKIP, int NL>
__global__ __launch_bounds__(64 * WARPS_M * WARPS_N) void wgrad_limb_kernel(const WgradParams p) {
  static_assert(WARPS_M * WARPS_N == 4 || WARPS_M * WARPS_N == 8, "4 waves, or 8 for the 256-row tile");
  constexpr int NT = 64 * WARPS_M * WARPS_N;
  static_assert(BM + BN <= NT && BK == 32, "one loader slot per thread");
  constexpr int WTM = BM / WARPS_M, WTN = BN / WARPS_N;
  constexpr int TM = WTM / 32, TN = WTN / 32;
  constexpr int kStage = 2 * (BM + BN) * 16 * NL, kPatch = (NT / 64) * WTM * (WTN + 4);
  __shared__ __attribute__((aligned(16))) float lds[kStage > kPatch ? kStage : kPatch];
  unsigned* ldsw = reinterpret_cast<unsigned*>(lds);
  constexpr int kAsz = 2 * BM * 16, kBsz = 2 * BN * 16, kBbase = NL * kAsz;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WARPS_N, wn = wave % WARPS_N;
  const int gridN = (p.K + BN - 1) / BN;
  int wg_tile, wg_split;
  wgrad_block((int)gridDim.x, wg_tile, wg_split);
  const int tile_n = wg_tile % gridN;
  const int tile_m = wg_tile / gridN;
  const int m0 = tile_m * BM, n0 = tile_n * BN;

  const __amdgpu_buffer_rsrc_t xr = make_rsrc(p.x, p.x_bytes);
  const __amdgpu_buffer_rsrc_t dr = make_rsrc(p.dy, p.dy_bytes);
  const ResidualSel rsel;

  // loader roles
  const bool is_a = tid < BM;
  const bool is_b = tid >= NT - BN;
  const int sa = tid, sb = tid - (NT - BN);
  const int ca = sa % (BM / 4), ga = sa / (BM / 4);        // channel chunk, 8-pixel group (0..3)
  const int cb = (is_b ? sb : 0) % (BN / 4), gb = (is_b ? sb : 0) / (BN / 4);
  const int a_col = m0 + ca * 4;
  const bool a_cok = is_a && a_col < p.Cout;
  const int b_col = n0 + cb * 4;
  const bool b_cok = is_b && b_col < p.K;
  int b_dh, b_dw, b_c;
  {
    const int kk = b_cok ? b_col : 0;
    const int tap = kk / p.Cin;
    b_c = kk - tap * p.Cin;
    const int r = tap / p.kw;
    const int s = tap - r * p.kw;
    b_dh = r * p.dil - p.pad;
    b_dw = s * p.dil - p.pad;
  }

  const int p_begin = wg_split * p.pix_per_split;
  int p_end = p_begin + p.pix_per_split;
  if (p_end > p.P) p_end = p.P;

  const int t_dh = (n0 / p.Cin / p.kw) * p.dil - p.pad;
  const int t_dw = ((n0 / p.Cin) % p.kw) * p.dil - p.pad;
  const bool patch = p.patch_mode != 0;
  auto step_dead = [&](int pt) -> bool { return wg_step_dead(p, pt, p_end, t_dh, t_dw); };
  auto next_valid = [&](int pt) -> int {
    if (SKIP)
      while (pt < p_end && step_dead(pt)) pt += BK;
    return pt;
  };

  const int himg = p.Hi * p.Wi;
  f32x4 reg[8];

  // B loader: (image base, ho, wo) of this thread's first pixel, advanced incrementally (a K-step moves 32 pixels on);
  // a division only on the first step and on row-skipping jumps.
  int bs_pix = -(1 << 30), bs_img = 0, bs_ho = 0, bs_wo = 0;
  // patch mode (the map tiles into patch_h x patch_w = 32-pixel patches, patch_w % 8 == 0): this thread's 8-pixel run
  // sits at a constant place inside every patch; a K-step adds the block-uniform patch origin
  const int pg = is_a ? ga : gb;
  const int pm_ih = (pg * 8) / p.patch_w, pm_iw = (pg * 8) % p.patch_w;
  const int pm_a_rel = (pm_ih * p.Wo + pm_iw) * p.ldy + a_col;
  const int pm_hh = pm_ih * p.stride + b_dh, pm_ww = pm_iw * p.stride + b_dw;
  const int pm_b_rel = (pm_hh * p.Wi + pm_ww) * p.ldx + b_c;
  auto load_tile = [&](int pt) {
    if (patch) {
      int pb, h0, w0;
      wg_patch_origin(p, pt, pb, h0, w0);
      if (is_a) {
        const uint32_t off0 = (uint32_t)((((pb * p.Ho + h0) * p.Wo + w0) * p.ldy + pm_a_rel) * 4);
        const uint32_t dpx = (uint32_t)p.ldy * 4u;
#pragma unroll
        for (int j = 0; j < 8; ++j) reg[j] = buf_load4(dr, a_cok ? off0 + (uint32_t)j * dpx : kOOB);
      } else if (is_b) {
        const int hs = h0 * p.stride, ws = w0 * p.stride;
        const bool rok = b_cok && ((unsigned)(hs + pm_hh) < (unsigned)p.Hi);
        const int wi0 = ws + pm_ww;
        const uint32_t off0 = (uint32_t)((((pb * p.Hi + hs) * p.Wi + ws) * p.ldx + pm_b_rel) * 4);   // may wrap; used when ok
        const uint32_t dpx = (uint32_t)(p.stride * p.ldx) * 4u;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const bool ok = rok && ((unsigned)(wi0 + j * p.stride) < (unsigned)p.Wi);
          reg[j] = buf_load4(xr, ok ? off0 + (uint32_t)j * dpx : kOOB);
        }
      }
      return;
    }
    if (is_a) {
      const int pix0 = pt + ga * 8;
      const int nval = a_cok ? p_end - pix0 : 0;
      const uint32_t off0 = (uint32_t)((pix0 * p.ldy + a_col) * 4);
      const uint32_t dpx = (uint32_t)p.ldy * 4u;
#pragma unroll
      for (int j = 0; j < 8; ++j) reg[j] = buf_load4(dr, j < nval ? off0 + (uint32_t)j * dpx : kOOB);
    } else if (is_b) {
      const int pix0 = pt + gb * 8;
      if (pix0 == bs_pix + BK) {
        bs_wo += BK;
        while (bs_wo >= p.Wo) {
          bs_wo -= p.Wo;
          if (++bs_ho == p.Ho) {
            bs_ho = 0;
            bs_img += himg;
          }
        }
      } else {
        const int b = pix0 / p.HoWo;
        const int rem = pix0 - b * p.HoWo;
        bs_ho = rem / p.Wo;
        bs_wo = rem - bs_ho * p.Wo;
        bs_img = b * himg;
      }
      bs_pix = pix0;
      const int nval = b_cok ? p_end - pix0 : 0;
      if (bs_wo + 8 <= p.Wo) {
        // the 8 pixels lie in one output row (always, when Wo % 8 == 0): one row test, offsets a constant stride apart
        const int hi = bs_ho * p.stride + b_dh;
        const int wi0 = bs_wo * p.stride + b_dw;
        const bool rok = (unsigned)hi < (unsigned)p.Hi;
        const uint32_t off0 = (uint32_t)(((bs_img + hi * p.Wi + wi0) * p.ldx + b_c) * 4);   // may wrap; used when ok
        const uint32_t dpx = (uint32_t)(p.stride * p.ldx) * 4u;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const bool ok = rok && j < nval && ((unsigned)(wi0 + j * p.stride) < (unsigned)p.Wi);
          reg[j] = buf_load4(xr, ok ? off0 + (uint32_t)j * dpx : kOOB);
        }
      } else {
        int ho = bs_ho, wo = bs_wo, img = bs_img;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int hi = ho * p.stride + b_dh, wi = wo * p.stride + b_dw;
          const bool ok = j < nval && ((unsigned)hi < (unsigned)p.Hi) && ((unsigned)wi < (unsigned)p.Wi);
          const uint32_t off = ok ? (uint32_t)(((img + hi * p.Wi + wi) * p.ldx + b_c) * 4) : kOOB;
          reg[j] = buf_load4(xr, off);
          if (++wo == p.Wo) {
            wo = 0;
            if (++ho == p.Ho) {
              ho = 0;
              img += himg;
            }
          }
        }
      }
    }
  };

  auto store_tile = [&](int buf) {
    if (!(is_a || is_b)) return;
    const int rows = is_a ? BM : BN;
    const int base = is_a ? 0 : kBbase;
    const int isz = is_a ? kAsz : kBsz;
    const int c4 = is_a ? ca : cb, g = is_a ? ga : gb;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = reg[j][e];
      u32x4 limb[NL];
      split8n<NL>(v, limb, rsel);
      const int o = buf * rows * 16 + swz(c4 * 4 + e, g);
#pragma unroll
      for (int l = 0; l < NL; ++l) *reinterpret_cast<u32x4*>(&ldsw[base + l * isz + o]) = limb[l];
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

  // Same pipeline as the gather kernel: two fragment sets alternate between the 16-pixel halves of a K-step; tile `cur`
  // is multiplied from LDS buffer `buf`, `nxt` is complete in buf^1, `stg` waits in the staging registers (loaded one
  // whole K-step earlier) and is split + written into `buf` after the barrier, under the second MFMA burst.
  f32x4 fa[2][NL * TM], fb[2][NL * TN];
  auto read_frags = [&](int set, int buf, int half) {
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
    const int t0 = next_valid(p_begin);
    if (t0 < p_end) {
      load_tile(t0);
      store_tile(0);
      int cur = t0, nxt = next_valid(t0 + BK), stg = p_end;
      if (nxt < p_end) {
        load_tile(nxt);
        store_tile(1);
        stg = next_valid(nxt + BK);
        if (stg < p_end) load_tile(stg);
      }
      if (nxt > p_end) nxt = p_end;
      if (stg > p_end) stg = p_end;
      __syncthreads();
      read_frags(0, 0, 0);
      int buf = 0;
      while (cur < p_end) {
        int after = p_end;
        if (stg < p_end) {
          after = next_valid(stg + BK);
          if (after > p_end) after = p_end;
        }
        read_frags(1, buf, 1);
        __builtin_amdgcn_sched_barrier(0);
        mfmas(0);
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();
        read_frags(0, buf ^ 1, 0);   // (garbage on the last step: never multiplied)
        __builtin_amdgcn_sched_barrier(0);
        if (stg < p_end) store_tile(buf);
        if (after < p_end) load_tile(after);
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

  float* out = p.dw + (long long)wg_split * p.slab_stride;
  {
    float* patch = lds + wave * (WTM * (WTN + 4));
    const int row0 = m0 + wm * WTM, col0 = n0 + wn * WTN;
    int rv = p.Cout - row0, cv = p.K - col0;
    rv = rv < 0 ? 0 : (rv > WTM ? WTM : rv);
    cv = cv < 0 ? 0 : (cv > WTN ? WTN : cv);
    store_tiles<TM, TN>(acc, patch, out, p.K, row0, col0, rv, cv, nullptr, p.accumulate != 0, lane,
                        [](int m) { return m; });
  }
}

// ------------------------------------------------------------------------------------------------
// Fixed-order reduction of split slabs: out[m*ld + n] = (acc ? out : 0) + bias[n] + sum_z slab[z][m][n].
__global__ __launch_bounds__(256) void slab_reduce_kernel(const float* __restrict__ slabs, long long slab_stride,
                                                          int nslab, float* __restrict__ out, int ld, long long M,
                                                          int N, const float* __restrict__ bias, int accumulate) {
  const long long total = M * N;
  if ((N & 3) == 0 && (ld & 3) == 0 && (slab_stride & 3) == 0 && (((uintptr_t)slabs | (uintptr_t)out) & 15) == 0) {
    // 16 bytes per lane, slabs in a fixed order; two elements in flight per lane
    const long long total4 = total >> 2;
    const int n4 = N >> 2;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total4; i += (long long)gridDim.x * 256) {
      const long long m = i / n4;
      const int n = (int)(i - m * n4) * 4;
      const float* sp = slabs + i * 4;
      f32x4 v = *reinterpret_cast<const f32x4*>(sp);
      // slabs added strictly in order, their loads sixteen / four at a time: the narrow layers of the encoder split into
      // up to 256 slabs of a few thousand elements -- a handful of blocks, each lane a chain of nslab round trips
      // (230 us per launch beside the data gradients; the weight-gradient stream ends the fp32 step 0.5 ms late)
      int z = 1;
      for (; z + 15 < nslab; z += 16) {
        f32x4 t[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) t[k] = *reinterpret_cast<const f32x4*>(sp + (long long)(z + k) * slab_stride);
#pragma unroll
        for (int k = 0; k < 16; ++k) v += t[k];
      }
      for (; z + 3 < nslab; z += 4) {
        f32x4 t[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) t[k] = *reinterpret_cast<const f32x4*>(sp + (long long)(z + k) * slab_stride);
#pragma unroll
        for (int k = 0; k < 4; ++k) v += t[k];
      }
      for (; z < nslab; ++z) v += *reinterpret_cast<const f32x4*>(sp + (long long)z * slab_stride);
      if (bias != nullptr) v += *reinterpret_cast<const f32x4*>(bias + n);
      float* op = out + m * ld + n;
      if (accumulate) v += *reinterpret_cast<const f32x4*>(op);
      *reinterpret_cast<f32x4*>(op) = v;
    }
    return;
  }
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long m = i / N;
    const int n = (int)(i - m * N);
    float v = 0.f;
    for (int z = 0; z < nslab; ++z) v += slabs[(long long)z * slab_stride + i];
    if (bias != nullptr) v += bias[n];
    const long long o = m * ld + n;
    if (accumulate) v += out[o];
    out[o] = v;
  }
}

// Every split weight gradient of a backward pass reduced in ONE launch (pseg_slab_reduce_batch): jobs[j] = {slabs, out,
// elements (a multiple of 4), slab count, index of the job's first block}; a block covers kSlabBlock consecutive
// elements of one job and finds it by bisection.  Fixed slab order, same arithmetic as slab_reduce_kernel.
constexpr int kSlabBlock = 4096;   // floats per block: 256 lanes x 4 x 16 bytes
__global__ __launch_bounds__(256) void slab_reduce_batch_kernel(const long long* __restrict__ jobs, int n, int accumulate) {
  const long long b = blockIdx.x;
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[mid * 5 + 4] <= b) lo = mid;
    else hi = mid - 1;
  }
  const long long* job = jobs + lo * 5;
  const float* slabs = reinterpret_cast<const float*>(job[0]);
  float* out = reinterpret_cast<float*>(job[1]);
  const long long elems = job[2];
  const int nslab = (int)job[3];
  const long long base = (b - job[4]) * kSlabBlock;
#pragma unroll
  for (int u = 0; u < kSlabBlock / 1024; ++u) {
    const long long i = base + (long long)u * 1024 + threadIdx.x * 4;
    if (i < elems) {
      f32x4 v = *reinterpret_cast<const f32x4*>(slabs + i);
      int z = 1;      // in order, loads sixteen / four at a time (as in slab_reduce_kernel)
      for (; z + 15 < nslab; z += 16) {
        f32x4 t[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) t[k] = *reinterpret_cast<const f32x4*>(slabs + (long long)(z + k) * elems + i);
#pragma unroll
        for (int k = 0; k < 16; ++k) v += t[k];
      }
      for (; z + 3 < nslab; z += 4) {
        f32x4 t[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) t[k] = *reinterpret_cast<const f32x4*>(slabs + (long long)(z + k) * elems + i);
#pragma unroll
        for (int k = 0; k < 4; ++k) v += t[k];
      }
      for (; z < nslab; ++z) v += *reinterpret_cast<const f32x4*>(slabs + (long long)z * elems + i);
      if (accumulate) v += *reinterpret_cast<const f32x4*>(out + i);
      *reinterpret_cast<f32x4*>(out + i) = v;
    }
  }
}

int launch_slab_reduce(const float* slabs, long long slab_stride, int nslab, float* out, int ld, long long M, int N,
                       const float* bias, int accumulate, hipStream_t st) {
  const long long total = M * N;
  const int blocks = (int)(total / 256 + 1 < 4096 ? total / 256 + 1 : 4096);
  hipLaunchKernelGGL(slab_reduce_kernel, dim3(blocks), dim3(256), 0, st, slabs, slab_stride, nslab, out, ld, M, N, bias,
                     accumulate);
  PSEG_LAUNCH_CHECK();
  return PSEG_OK;
}


// ------------------------------------------------------------------------------------------------ weight gradient
// The tiles of wgrad_f32_dma_kernel (rows = Cout, columns = K), stated once: select_wgrad reads from this table what the kernel
// covers, launch_wgrad_dma maps an entry to template arguments.  Threads per block = 64 * wm * wn.
struct WgradDmaTile {
  int bm, bn, wm, wn;
  bool skip;     // a SKIP = true instantiation exists
};
constexpr WgradDmaTile kWgradDmaTiles[] = {{128, 128, 2, 4, true},
                                           {128, 64, 4, 2, true},
                                           {64, 128, 2, 4, true},
                                           {32, 256, 1, 8, true},     // narrow outputs (the 21-class classifier, HRNet's 32-channel branch): the x operand by DMA
                                           {32, 288, 1, 9, false}};   // 3x3 on 32 channels: the whole filter as one column tile, nine waves
constexpr int kNumWgradDmaTiles = (int)(sizeof(kWgradDmaTiles) / sizeof(kWgradDmaTiles[0]));

static int wgrad_dma_tile_index(TileCfg t) {
  for (int i = 0; i < kNumWgradDmaTiles; ++i)
    if (kWgradDmaTiles[i].bm == t.bm && kWgradDmaTiles[i].bn == t.bn) return i;
  return -1;
}

// A weight gradient as run_wgrad sees it: the geometry plus what the caller asks of the plan.
struct WgradProblem : WgradGeom {
  int precision;
  bool concurrent;   // the launch shares the chip with another stream's kernels (see plan_wgrad)
};

// Everything run_wgrad decides before it launches; the queries read their answers off the same choice.
struct WgradChoice {
  WgradPlan pl;            // (the halo kernel's 32 x 288 tile and grid included)
  WgradPixelOrder order;   // ... with the packed tap order and lpt_per
  int kernel;              // PSEG_KERNEL_WGRAD_* that runs
  int dma_tile;            // entry of kWgradDmaTiles, -1: none
  bool skip;               // the kernel's SKIP template flag
};

// The one place that picks the kernel of an exact-fp32 / limb weight gradient.  Pure: launches nothing, touches no device.
static WgradChoice select_wgrad(const WgradProblem& q) {
  WgradChoice c;
  const long long P = q.P();
  const int taps = q.kh * q.kw;
  c.pl = plan_wgrad(P, q.Cout, q.K(), q.precision == 1, q.precision != 0, 0, q.concurrent);
  c.order = wgrad_pixel_order(q, c.pl.tile.bn);
  WgradPixelOrder& o = c.order;
  const bool dma = q.precision == 0 && cfg().wgrad_f32dma != 0;
  // narrow 3x3 filters on few channels: the halo-staged kernel (wgrad_f32_halo_kernel) on the plan's pixel splits -- a block is
  // (row tile of 32 filters, one 32-channel chunk of the input, one split); K-steps are 2 x 16 strips of the output map.
  // Measured (profiles/EXPERIMENTS.md 5.13): 32 -> 32 on 128x128 53 -> 45 us, HRNet fp32 14.19 -> 14.07 ms; the classifier (384
  // channels: 583 -> 540 us alone) is SLOWER inside the two-stream DeepLabV3+ step (42.93 -> 43.03 ms) and 64-filter layers lose
  // outright (64 -> 64: 40 -> 72 us) -- hence at most 64 input channels and 32 filters; PSEG_WGRAD_HALO=2 lifts the channel cap.
  const bool halo = dma && cfg().wgrad_halo != 0 && q.kh == 3 && q.kw == 3 && q.stride == 1 && q.dil == 1 && q.pad == 1 &&
                    q.Cin % 32 == 0 && (q.Cin <= 64 || cfg().wgrad_halo >= 2) && q.Cout <= 32 && q.H == q.Ho && q.W == q.Wo &&
                    q.Ho % 2 == 0 && q.Wo % 16 == 0 && P % BK == 0;
  if (halo) {
    o.mode = kWgDense;
    o.patch_mode = 1;
    o.patch_h = 2;
    o.patch_w = 16;
    c.pl.tile = TileCfg{32, 288};
    c.pl.gridM = cdiv(q.Cout, 32);
    c.pl.gridN = q.Cin / 32;
  }
  const WgradPlan& pl = c.pl;
  c.dma_tile = wgrad_dma_tile_index(pl.tile);
  if (!dma || c.dma_tile < 0) {
    // register-staged / limb kernels, in the shared pixel order
    // (never the 32 x 288 tile: plan_wgrad and the halo branch above give it to the LDS-DMA kernels only)
    c.kernel = q.precision == 0 ? PSEG_KERNEL_WGRAD_REGISTER : PSEG_KERNEL_WGRAD_LIMB;
    c.skip = o.mode != kWgDense;
    return c;
  }
  // exact-fp32 weight gradient on the LDS-DMA kernel (8 waves, two blocks per CU); same tile, same split plan
  c.kernel = halo ? PSEG_KERNEL_WGRAD_HALO : PSEG_KERNEL_WGRAD_DMA;
  if (!o.patch_mode) {
    // a map that does not tile into 32-pixel patches: plain row-major pixel order instead of the register-staged kernel
    o.mode = kWgRowMajorDma;
  } else if (o.can_skip && q.stride == 1 && taps <= 9) {
    // dilated conv: packed live rectangles instead of 32-pixel patches
    o.mode = kWgPacked;
    // longest-first order of the taps (live area, descending; ties keep the tap order: deterministic)
    int area[9];
    for (int t = 0; t < taps; ++t) {
      const int dh = (t / q.kw) * q.dil - q.pad, dwv = (t % q.kw) * q.dil - q.pad;
      const int r0 = dh < 0 ? -dh : 0, c0 = dwv < 0 ? -dwv : 0;
      const int r1 = q.H - dh < q.Ho ? q.H - dh : q.Ho, c1 = q.W - dwv < q.Wo ? q.W - dwv : q.Wo;
      area[t] = (r1 > r0 ? r1 - r0 : 0) * (c1 > c0 ? c1 - c0 : 0);
    }
    for (int i = 1; i < taps; ++i)
      for (int j = i; j > 0 && area[o.tap_order[j]] > area[o.tap_order[j - 1]]; --j) {
        const int t = o.tap_order[j];
        o.tap_order[j] = o.tap_order[j - 1];
        o.tap_order[j - 1] = t;
      }
    // one group = what one XCD walks in order (wgrad_block: eight contiguous ranges of the (split, tile) pairs)
    const int tpt = q.Cin / pl.tile.bn;
    const long long total = (long long)pl.gridM * pl.gridN * pl.splits;
    int groups = 1;
    if (total % 8 == 0 && pl.gridN % (total / 8) == 0) groups = (int)(pl.gridN / (total / 8));
    if (groups < 1 || tpt % groups != 0) groups = 1;
    o.lpt_per = tpt / groups;
  }
  c.skip = kWgradDmaTiles[c.dma_tile].skip && (o.mode == kWgSkipPatches || o.mode == kWgPacked);
  return c;
}

// the record of a choice (pseg_debug_last_wgrad, pseg_conv2d_wgrad_choice): every kernel here takes 32 pixels per K-step
static void record_wgrad(const WgradChoice& c, int* out11) { wgrad_record(out11, c.kernel, c.pl, c.order, BK, c.skip); }

static void launch_wgrad_dma(const WgradChoice& c, dim3 grid, hipStream_t st, const WgradParams& p) {
  with_index(c.dma_tile, [&](auto tile) {
    constexpr WgradDmaTile t = kWgradDmaTiles[decltype(tile)::value];
    const dim3 block(64 * t.wm * t.wn);
    if constexpr (t.skip) {
      if (c.skip) {
        hipLaunchKernelGGL((wgrad_f32_dma_kernel<t.bm, t.bn, t.wm, t.wn, true>), grid, block, 0, st, p);
        return;
      }
    }
    hipLaunchKernelGGL((wgrad_f32_dma_kernel<t.bm, t.bn, t.wm, t.wn, false>), grid, block, 0, st, p);
  }, std::make_integer_sequence<int, kNumWgradDmaTiles>{});
}

// the register-staged exact-fp32 kernel and the limb kernels
static int launch_wgrad_staged(const WgradChoice& c, int precision, dim3 grid, hipStream_t st, const WgradParams& p) {
  if (precision == 0 && c.pl.tile.bm == 32 && c.pl.tile.bn == 256) {
    // (the 32 x 256 tile off the DMA kernel -- PSEG_WGRAD_F32DMA=0: two accumulators per wave)
    if (c.skip) hipLaunchKernelGGL((wgrad_kernel<32, 256, 1, 4, true>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((wgrad_kernel<32, 256, 1, 4, false>), grid, dim3(256), 0, st, p);
    PSEG_LAUNCH_CHECK();
    return PSEG_OK;
  }
  typedef void (*Kfn)(const WgradParams);
#define PSEG_WGRAD_ROW(KERNEL, BIG, ...)                                                                                \
  {KERNEL<128, 128, 2, 2, __VA_ARGS__>, KERNEL<128, 64, 2, 2, __VA_ARGS__>, KERNEL<128, 32, 4, 1, __VA_ARGS__>,         \
   KERNEL<64, 128, 2, 2, __VA_ARGS__>, KERNEL<32, 128, 1, 4, __VA_ARGS__>, BIG}
  // the 256x128 tile (8 waves, one block per CU) exists for the two-limb variant
  static const Kfn fns32[2][6] = {PSEG_WGRAD_ROW(wgrad_kernel, nullptr, false), PSEG_WGRAD_ROW(wgrad_kernel, nullptr, true)};
  static const Kfn fnsb3[2][6] = {PSEG_WGRAD_ROW(wgrad_limb_kernel, (wgrad_limb_kernel<256, 128, 4, 2, false, 2>), false, 2),
                                  PSEG_WGRAD_ROW(wgrad_limb_kernel, (wgrad_limb_kernel<256, 128, 4, 2, true, 2>), true, 2)};
  static const Kfn fnsb6[2][6] = {PSEG_WGRAD_ROW(wgrad_limb_kernel, nullptr, false, 3),
                                  PSEG_WGRAD_ROW(wgrad_limb_kernel, nullptr, true, 3)};
#undef PSEG_WGRAD_ROW
  const auto& fns = precision == 2 ? fnsb6 : precision == 1 ? fnsb3 : fns32;
  return launch_tiles<WgradParams, Kfn, 6>(fns, c.skip, c.pl.tile, grid, p, st);
}

// validate, select, check the workspace, fill the parameters from the choice and launch, reduce the slabs.
// defer: a split plan leaves its slabs in the workspace (the caller reduces them later, pseg_slab_reduce_batch)
static int run_wgrad(const WgradProblem& q, const float* x, int ldx, const float* dy, int ldy, float* dw, int accumulate,
                     void* workspace, int64_t workspace_bytes, hipStream_t st, bool defer) {
  PSEG_REQUIRE(x && dy && dw, "conv2d_wgrad: null pointer");
  PSEG_REQUIRE(q.precision >= 0 && q.precision <= 2, "conv2d_wgrad: precision must be PSEG_PREC_FP32 / _BF16X3 / _BF16X6");
  PSEG_REQUIRE(q.Cin % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0, "conv2d_wgrad: Cin, ldx, ldy must be multiples of 4");
  PSEG_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)dy & 15) == 0, "conv2d_wgrad: x / dy must be 16-byte aligned");
  const long long P = q.P();
  PSEG_REQUIRE(P > 0 && P < (1LL << 31), "conv2d_wgrad: bad pixel count");
  const long long xb = nhwc_bytes(q.B, q.H, q.W, q.Cin, ldx), db = nhwc_bytes(q.B, q.Ho, q.Wo, q.Cout, ldy);
  // dy chunks are read 4 channels at a time: the last chunk of a row may run up to 3 floats past Cout (inside ldy)
  PSEG_REQUIRE(xb < kMaxBytes && db < kMaxBytes, "conv2d_wgrad: tensor exceeds 2 GiB");
  PSEG_REQUIRE((q.Cout + 3) / 4 * 4 <= ldy, "conv2d_wgrad: ldy must cover Cout rounded up to 4");
  const WgradChoice c = select_wgrad(q);
  const WgradPlan& pl = c.pl;
  WgradParams p;
  p.x = x;
  p.dy = dy;
  p.x_bytes = (uint32_t)xb;
  p.dy_bytes = (uint32_t)(((P - 1) * ldy + (q.Cout + 3) / 4 * 4) * 4);
  p.ldx = ldx;
  p.ldy = ldy;
  set_wgrad_geometry(p, q, pl, c.order);
  const int rc = set_wgrad_output(p, pl, dw, accumulate, workspace, workspace_bytes, "conv2d_wgrad");
  if (rc != PSEG_OK) return rc;
  const dim3 grid((unsigned)(pl.gridM * pl.gridN), 1, (unsigned)pl.splits);
  g_last_conv_kernel = c.kernel;
  record_wgrad(c, g_last_wgrad);
  if (c.kernel == PSEG_KERNEL_WGRAD_HALO) {
    hipLaunchKernelGGL(wgrad_f32_halo_kernel<32>, grid, dim3(576), 0, st, p);
  } else if (c.kernel == PSEG_KERNEL_WGRAD_DMA) {
    launch_wgrad_dma(c, grid, st, p);
  } else {
    const int rl = launch_wgrad_staged(c, q.precision, grid, st, p);
    if (rl != PSEG_OK) return rl;
  }
  PSEG_LAUNCH_CHECK();
  if (pl.splits > 1 && !defer)
    return launch_slab_reduce((const float*)workspace, p.slab_stride, pl.splits, dw, p.K, (long long)q.Cout, p.K, nullptr, accumulate, st);
  return PSEG_OK;
}

}  // namespace pseg

using namespace pseg;

extern "C" {

int pseg_conv2d_wgrad(const float* x, int ldx, const float* dy, int ldy, float* dw, int B, int H, int W, int Cin, int Ho,
                      int Wo, int Cout, int kh, int kw, int stride, int pad, int dil, int accumulate, int precision,
                      int concurrent, void* workspace, int64_t workspace_bytes, void* stream) {
  return run_wgrad(WgradProblem{{B, H, W, Cin, Ho, Wo, Cout, kh, kw, stride, pad, dil}, precision, concurrent != 0}, x, ldx, dy, ldy,
                   dw, accumulate, workspace, workspace_bytes, (hipStream_t)stream, false);
}

// the problem of a query, which knows Ho / Wo only: the smallest unit-stride input that gives them (the pixel split does not
// depend on it)
static WgradProblem wgrad_query_problem(int B, int Ho, int Wo, int Cin, int Cout, int kh, int kw, int precision, int concurrent) {
  return WgradProblem{{B, Ho + kh - 1, Wo + kw - 1, Cin, Ho, Wo, Cout, kh, kw, 1, 0, 1}, precision, concurrent != 0};
}

int pseg_conv2d_wgrad_splits(int B, int Ho, int Wo, int Cin, int Cout, int kh, int kw, int precision, int concurrent) {
  if (B <= 0 || Ho <= 0 || Wo <= 0 || Cin <= 0 || Cout <= 0 || precision < 0 || precision > 2) return 0;
  return select_wgrad(wgrad_query_problem(B, Ho, Wo, Cin, Cout, kh, kw, precision, concurrent)).pl.splits;
}

int pseg_conv2d_wgrad_choice(int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad, int dil,
                             int precision, int concurrent, int* out11) {
  PSEG_REQUIRE(out11 != nullptr, "conv2d_wgrad_choice: null pointer");
  PSEG_REQUIRE(B > 0 && H > 0 && W > 0 && Cin > 0 && Ho > 0 && Wo > 0 && Cout > 0 && kh > 0 && kw > 0 && stride > 0 && pad >= 0 &&
                   dil > 0 && precision >= 0 && precision <= 2,
               "conv2d_wgrad_choice: bad geometry or precision");
  record_wgrad(select_wgrad(WgradProblem{{B, H, W, Cin, Ho, Wo, Cout, kh, kw, stride, pad, dil}, precision, concurrent != 0}), out11);
  return PSEG_OK;
}

int64_t pseg_conv2d_wgrad_workspace_bytes(int B, int Ho, int Wo, int Cin, int Cout, int kh, int kw) {
  // the plan depends on the arithmetic and on what the launch runs beside: size for the most slabs any of them asks for
  int splits = 0;
  for (int precision = 0; precision <= 2; ++precision)
    for (int concurrent = 0; concurrent <= 1; ++concurrent) {
      const int s = select_wgrad(wgrad_query_problem(B, Ho, Wo, Cin, Cout, kh, kw, precision, concurrent)).pl.splits;
      splits = s > splits ? s : splits;
    }
  return splits > 1 ? (int64_t)splits * Cout * kh * kw * Cin * 4 : 0;
}

int pseg_conv2d_wgrad_slabs(const float* x, int ldx, const float* dy, int ldy, float* slabs, int B, int H, int W, int Cin,
                            int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad, int dil, int precision,
                            int concurrent, int64_t slab_bytes, void* stream) {
  PSEG_REQUIRE(pseg_conv2d_wgrad_splits(B, Ho, Wo, Cin, Cout, kh, kw, precision, concurrent) > 1,
               "conv2d_wgrad_slabs: this plan does not split -- call pseg_conv2d_wgrad");
  // (dw is unused by a split plan; the slabs pointer stands in for the null check)
  return run_wgrad(WgradProblem{{B, H, W, Cin, Ho, Wo, Cout, kh, kw, stride, pad, dil}, precision, concurrent != 0}, x, ldx, dy, ldy,
                   slabs, 0, slabs, slab_bytes, (hipStream_t)stream, true);
}

int pseg_slab_reduce_batch(const int64_t* jobs, int n, int64_t total_blocks, int accumulate, void* stream) {
  PSEG_REQUIRE(jobs && n > 0 && total_blocks > 0 && total_blocks < (1LL << 31), "slab_reduce_batch: bad argument");
  hipLaunchKernelGGL(slab_reduce_batch_kernel, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const long long*>(jobs), n, accumulate);
  PSEG_LAUNCH_CHECK();
  return PSEG_OK;
}

int pseg_slab_reduce_block(void) { return kSlabBlock; }

}  // extern "C"
