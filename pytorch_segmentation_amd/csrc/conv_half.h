// Shared by the two half-precision (`-mp`) conv units, conv_half_gather.hip (forward and data gradient) and conv_half_wgrad.hip
// (weight gradient): counted waits, the transposing LDS read, the 32-row store epilogue with its fused BatchNorm-backward sums
// (the weight gradient writes its slabs through it too), and the few host-side pieces both launch paths use.
#pragma once
#include "conv_common.h"
#include "half_io.h"

namespace pseg {

constexpr int BKH = 64;    // long K-step of the gather kernel in halves (128-byte LDS rows); the short one is 32
// (the weight-gradient kernel contracts over BKP = 64 or 32 pixels per K-step: two or one 32-pixel sub-steps)

// s_waitcnt vmcnt(N) with a compile-time N (the instruction takes an immediate)
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  static_assert(N >= 0 && N <= 24, "vmcnt immediate");
#define PSEG_VMCNT_CASE(V) else if constexpr (N == V) asm volatile("s_waitcnt vmcnt(" #V ")" ::: "memory")
  if constexpr (N == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  PSEG_VMCNT_CASE(1); PSEG_VMCNT_CASE(2); PSEG_VMCNT_CASE(3); PSEG_VMCNT_CASE(4); PSEG_VMCNT_CASE(5); PSEG_VMCNT_CASE(6);
  PSEG_VMCNT_CASE(7); PSEG_VMCNT_CASE(8); PSEG_VMCNT_CASE(9); PSEG_VMCNT_CASE(10); PSEG_VMCNT_CASE(11); PSEG_VMCNT_CASE(12);
  PSEG_VMCNT_CASE(13); PSEG_VMCNT_CASE(14); PSEG_VMCNT_CASE(15); PSEG_VMCNT_CASE(16); PSEG_VMCNT_CASE(17); PSEG_VMCNT_CASE(18);
  PSEG_VMCNT_CASE(19); PSEG_VMCNT_CASE(20); PSEG_VMCNT_CASE(21); PSEG_VMCNT_CASE(22); PSEG_VMCNT_CASE(23); PSEG_VMCNT_CASE(24);
#undef PSEG_VMCNT_CASE
}

// ds_read_b64_tr_b16 as inline assembly, with the byte offset as an immediate.  Why not the builtin: hipcc treats the
// intrinsic as a read of ANY LDS byte and puts `s_waitcnt vmcnt(0)` in front of it whenever an LDS-DMA (`buffer_load ... lds`, a
// pending LDS write on the VM counter) is in flight -- which drains the operand ring once per K-step in the weight gradient
// and once per tile in the persistent kernel's epilogue (round 4: found in the disassembly).  An asm statement is invisible to
// that pass; its result is NOT covered by the compiler's own waits either: the caller waits (`s_waitcnt lgkmcnt`) before use.
typedef short s16x4t __attribute__((ext_vector_type(4)));
template <int OFF>
__device__ __forceinline__ s16x4t tr_read_asm(uint32_t lds_byte_addr) {
  static_assert(OFF >= 0 && OFF < 65536, "ds offset field");
  s16x4t v;
#if defined(__HIP_DEVICE_COMPILE__) && defined(PSEG_TR_BUILTIN) && PSEG_TR_BUILTIN
  // (A/B build, `python -m pytorch_segmentation_amd.csrc.build --trbuiltin`: the compiler-visible read, with its vmcnt(0))
  typedef __attribute__((address_space(3))) s16x4t* lds_s16x4p;
  v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4p)(uintptr_t)(lds_byte_addr + OFF));
#elif defined(__HIP_DEVICE_COMPILE__)
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(v) : "v"(lds_byte_addr), "i"(OFF));
#else
  v = s16x4t{0, 0, 0, 0};
  (void)lds_byte_addr;
#endif
  return v;
}
__device__ __forceinline__ uint32_t lds_addr_of(const void* p) {
  return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const void*)p;
}
// compile-time loop: f(std::integral_constant<int, 0>{}), ..., f(std::integral_constant<int, N - 1>{})
template <int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (N > 0) {
    static_for<N - 1>(f);
    f(std::integral_constant<int, N - 1>{});
  }
}

// One 32-row tile row of a wave's accumulators -> global memory through a wave-private [32][WTN + 4] fp32 patch, 8 columns
// per lane: 16-byte stores of fp16 (or two of fp32).  Called once per tile row, so the patch is a quarter / half of what the
// whole wave tile would need: LDS per block is set by the operand ring, not by the epilogue (more blocks per CU).
// BNS (a data gradient that feeds a BatchNorm backward; GatherConvParams::bns_y, fp16 here): the lanes that store eight channels
// of a row of dx read the producing layer's y at the same place and keep sum(g) / sum(g * x_hat) per channel, g = the value AS
// STORED (rounded to fp16: what bn_bwd_reduce_kernel would read back) under the activation mask of the forward pass's own
// expression.  The coefficients of the lane's eight channels are loaded once per tile (HBnsCoef), the sums are folded over
// the lanes of a channel octet after the last tile row (bns_fold8).
struct HBnsCoef {
  f32x4 mu[2], is[2], sc[2], sh[2];
};
struct HBnsSums {
  f32x4 s1[2], s2[2];
};

__device__ __forceinline__ void bns_load_coef(const GatherConvParams& p, int col, bool ok, HBnsCoef& c) {
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    c.mu[h] = ok ? *reinterpret_cast<const f32x4*>(p.bns_mean + col + 4 * h) : z;
    c.is[h] = ok ? *reinterpret_cast<const f32x4*>(p.bns_invstd + col + 4 * h) : z;
    c.sc[h] = ok ? *reinterpret_cast<const f32x4*>(p.bns_scale + col + 4 * h) : z;
    c.sh[h] = ok ? *reinterpret_cast<const f32x4*>(p.bns_shift + col + 4 * h) : z;
  }
}

// eight stored channels of one row (ov) against the layer's y at `yrow` (channels col ..)
__device__ __forceinline__ void bns_add8(const f16x8v& ov, const f16x8v& yv, int act, const HBnsCoef& c, HBnsSums& s) {
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float d = (float)yv[4 * h + e] - c.mu[h][e];
      const float pre = d * c.sc[h][e] + c.sh[h][e];       // the forward pass's own expression: the mask is the one it applied
      bool on = true;
      if (act == PSEG_ACT_RELU) on = pre > 0.f;
      else if (act == PSEG_ACT_RELU6) on = (pre > 0.f) && (pre < 6.f);
      const float g = on ? (float)ov[4 * h + e] : 0.f;
      s.s1[h][e] += g;
      s.s2[h][e] += g * (d * c.is[h][e]);
    }
}

template <int TN, bool BNS, typename RowMap>
__device__ __forceinline__ void store_row32(const f32x16 (&acc)[TN], float* patch, void* out, bool out_f32, long long ld, int row0,
                                            int col0, int rows_valid, int cols_valid, const float* bias, bool accumulate,
                                            int lane, RowMap&& out_row, const GatherConvParams& bns, const HBnsCoef& bc,
                                            HBnsSums& bs) {
  constexpr int WTN = TN * 32, LDW = WTN + 4;
  const int col_l = lane & 31;
  const int row_h = (lane >> 5) * 4;
  // BNS: the rows of y this lane will need are requested before the accumulators make their way through the patch
  constexpr int kC8 = WTN / 8, kRPI = 64 / kC8;
  f16x8v ypre[32 / kRPI];
  if constexpr (BNS) {
#pragma unroll
    for (int it = 0; it < 32 / kRPI; ++it) {
      const int row = it * kRPI + lane / kC8;
      const int colp = (lane % kC8) * 8;
      ypre[it] = f16x8v{0, 0, 0, 0, 0, 0, 0, 0};
      if (colp < cols_valid && row < rows_valid)
        ypre[it] = *reinterpret_cast<const f16x8v*>(reinterpret_cast<const half_t*>(bns.bns_y) +
                                                    (long long)out_row(row0 + row) * bns.bns_ldy + col0 + colp);
    }
  }
#pragma unroll
  for (int j = 0; j < TN; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) patch[((r & 3) + 8 * (r >> 2) + row_h) * LDW + j * 32 + col_l] = acc[j][r];
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  constexpr int C8 = WTN / 8;          // 8-column chunks per row
  constexpr int RPI = 64 / C8;         // rows per wave-instruction
  const int c8 = lane % C8, rr = lane / C8;
  const int col = c8 * 8;
  const bool cok = col < cols_valid;   // cols_valid is a multiple of 8
  f32x4 b0 = {0.f, 0.f, 0.f, 0.f}, b1 = {0.f, 0.f, 0.f, 0.f};
  if (bias != nullptr && cok) {
    b0 = *reinterpret_cast<const f32x4*>(bias + col0 + col);
    b1 = *reinterpret_cast<const f32x4*>(bias + col0 + col + 4);
  }
#pragma unroll
  for (int it = 0; it < 32 / RPI; ++it) {
    const int row = it * RPI + rr;
    if (cok && row < rows_valid) {
      f32x4 v0 = *reinterpret_cast<const f32x4*>(&patch[row * LDW + col]) + b0;
      f32x4 v1 = *reinterpret_cast<const f32x4*>(&patch[row * LDW + col + 4]) + b1;
      const long long orow = (long long)out_row(row0 + row);
      const long long o = orow * ld + col0 + col;
      if (out_f32) {
        float* gp = reinterpret_cast<float*>(out) + o;
        if (accumulate) {
          v0 += *reinterpret_cast<const f32x4*>(gp);
          v1 += *reinterpret_cast<const f32x4*>(gp + 4);
        }
        *reinterpret_cast<f32x4*>(gp) = v0;
        *reinterpret_cast<f32x4*>(gp + 4) = v1;
      } else {
        half_t* gp = reinterpret_cast<half_t*>(out) + o;
        if (accumulate) {
          const f16x8v old = *reinterpret_cast<const f16x8v*>(gp);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            v0[e] += (float)old[e];
            v1[e] += (float)old[4 + e];
          }
        }
        f16x8v ov;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          ov[e] = (half_t)v0[e];
          ov[4 + e] = (half_t)v1[e];
        }
        *reinterpret_cast<f16x8v*>(gp) = ov;
        if constexpr (BNS) bns_add8(ov, ypre[it], bns.bns_act, bc, bs);
      }
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();      // the patch is rewritten by the next tile row
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

template <int TN, typename RowMap>
__device__ __forceinline__ void store_row32(const f32x16 (&acc)[TN], float* patch, void* out, bool out_f32, long long ld, int row0,
                                            int col0, int rows_valid, int cols_valid, const float* bias, bool accumulate,
                                            int lane, RowMap&& out_row) {
  GatherConvParams none;       // (never read: BNS == false)
  HBnsCoef bc;
  HBnsSums bs;
  store_row32<TN, false>(acc, patch, out, out_f32, ld, row0, col0, rows_valid, cols_valid, bias, accumulate, lane, out_row, none,
                         bc, bs);
}

// ------------------------------------------------------------------------------------------------ host side
static long long nhwc_bytes_h(int B, int H, int W, int C, int ld) { return (((long long)B * H * W - 1) * ld + C) * 2; }

constexpr long long kLdsBytes = 160 * 1024;    // LDS of a CU: what a block's ring and patch must fit in

// a K-step (halves, or pixels in the weight gradient) and a ring depth as template arguments of a launch helper's callback
template <int KB, int ST>
struct HSteps { static constexpr int kb = KB, st = ST; };

}  // namespace pseg
