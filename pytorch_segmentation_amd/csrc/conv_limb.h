// Limb arithmetic of the conv kernels (conv_gather.hip, conv_wgrad.hip): an fp32 operand as two or three bf16 limbs, or as two
// fp16 limbs of the power-of-two-scaled value, and the swizzled LDS image of a split tile.
#pragma once
#include "common.h"

namespace pseg {

// ------------------------------------------------------------------------------------------------
// Split-bf16 ("bf16x3") arithmetic: every fp32 operand x is split into hi = bf16_rne(x), lo = bf16_rne(x - hi)
// (x - hi is exact in fp32), and a product a*b is evaluated as ah*bh + ah*bl + al*bh on v_mfma_f32_32x32x16_bf16 with
// fp32 accumulation.  The dropped al*bl term and the rounding of lo are ~2^-17 of |a*b| (rms), i.e. the result carries
// ~17 significant bits per product -- two orders of magnitude inside the 1e-3 contract and of the same size as the
// summation-order noise of a K = 18432 fp32 contraction -- at 3/16 of the fp32-MFMA instruction time per MAC.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned pack_bf16(float a, float b) {   // v_cvt_pk_bf16_f32: round-to-nearest-even
  bf16x2 v = {(__bf16)a, (__bf16)b};
  return __builtin_bit_cast(unsigned, v);
}

// N-limb split of 4 consecutive-k fp32 values: limb[0] = bf16(x), limb[1] = bf16(x - limb0), limb[2] = bf16(x - l0 - l1);
// every subtraction is exact in fp32, so three limbs carry all 24 mantissa bits.
// x - float(bf16 half of `packed`) in ONE instruction: v_dot2c_f32_bf16 computes p.lo*m.lo + p.hi*m.hi + acc with the
// products and the sum exact here (one factor is -1 or 0, and x - bf16(x) is representable).  The selector constants
// {-1, 0} / {0, -1} travel through an opaque SGPR: written as literals the compiler folds {-1, 0} into the inline
// constant "-1.0", which the hardware expands to 0xBF800000 = {0, -1} (tools/micro/dot2c_split.hip).
// (A non-finite partner in the same pair would turn 0 * inf into NaN; finite training tensors never reach bf16's range.)
struct ResidualSel {
  bf16x2 lo, hi;
  __device__ __forceinline__ ResidualSel() {
    unsigned c0 = 0x0000BF80u, c1 = 0xBF800000u;
    asm volatile("" : "+s"(c0), "+s"(c1));
    lo = __builtin_bit_cast(bf16x2, c0);
    hi = __builtin_bit_cast(bf16x2, c1);
  }
};
__device__ __forceinline__ float resid_lo(unsigned packed, float x, const ResidualSel& rs) {
  return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, packed), rs.lo, x, false);
}
__device__ __forceinline__ float resid_hi(unsigned packed, float x, const ResidualSel& rs) {
  return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, packed), rs.hi, x, false);
}

template <int NL>
__device__ __forceinline__ void split4n(f32x4 v, u32x2 (&limb)[NL], const ResidualSel& rs) {
#pragma unroll
  for (int l = 0; l < NL; ++l) {
    const unsigned p01 = pack_bf16(v[0], v[1]), p23 = pack_bf16(v[2], v[3]);
    limb[l] = u32x2{p01, p23};
    if (l + 1 < NL) {
      v[0] = resid_lo(p01, v[0], rs);
      v[1] = resid_hi(p01, v[1], rs);
      v[2] = resid_lo(p23, v[2], rs);
      v[3] = resid_hi(p23, v[3], rs);
    }
  }
}

// fp16 limbs: x*2^e = hi + lo with two 11-bit limbs (22-bit operands, products accurate to ~2^-22).  fp16 has only a
// 5-bit exponent, so the operand is first scaled by an exact power of two chosen from its per-tensor max |x| (published
// by the producer kernels as the bit pattern of a non-negative float, see amax_update): amax * 2^e lies in [2^14, 2^15).
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned pack_f16(float a, float b) {  // v_cvt_f16_f32 (RNE) x2 + pack
  f16x2 v = {(_Float16)a, (_Float16)b};
  return __builtin_bit_cast(unsigned, v);
}
__device__ __forceinline__ float f16_lo(unsigned p) { return (float)__builtin_bit_cast(f16x2, p)[0]; }
__device__ __forceinline__ float f16_hi(unsigned p) { return (float)__builtin_bit_cast(f16x2, p)[1]; }

__device__ __forceinline__ void split4h(f32x4 v, float scale, u32x2 (&limb)[2]) {
  v *= scale;
  const unsigned h01 = pack_f16(v[0], v[1]), h23 = pack_f16(v[2], v[3]);
  limb[0] = u32x2{h01, h23};
  limb[1] = u32x2{pack_f16(v[0] - f16_lo(h01), v[1] - f16_hi(h01)), pack_f16(v[2] - f16_lo(h23), v[3] - f16_hi(h23))};
}

// exponent e such that amax * 2^e is in [2^14, 2^15) (e = 0 for an all-zero / non-finite tensor), as a float 2^e
__device__ __forceinline__ float pow2_scale_for(unsigned amax_bits, int& e_out) {
  const int ex = (int)((amax_bits >> 23) & 0xFFu);
  int e = 0;
  if (ex != 0 && ex != 255) e = 14 - (ex - 127);
  if (e > 100) e = 100;
  if (e < -100) e = -100;
  e_out = e;
  return __builtin_bit_cast(float, (unsigned)(e + 127) << 23);
}

// LDS image of a split tile: [row][32 bf16 = 64 bytes = four 16-byte k-slots], slot XOR-swizzled with (row>>2)&3 so the
// 16-lane groups of ds_read_b128 (rows {0-3,12-15,20-27} of a 32-row fragment, same slot) fall on 16 different 16-byte
// bank slots.  Returns the dword offset of k-slot `slot` of `row`.
__device__ __forceinline__ int swz(int row, int slot) { return row * 16 + ((slot ^ ((row >> 2) & 3)) << 2); }

}  // namespace pseg
