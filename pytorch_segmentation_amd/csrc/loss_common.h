// What the loss kernels (loss.hip, ce_opts.hip, lovasz.hip, tversky.hip) share: the fixed-order reductions of a 256-thread
// block that keep two calls bit-identical, and the host's launch and workspace-layout helpers.
#pragma once

#include "common.h"

namespace pseg {

#ifdef __HIPCC__

// Sum of a double over the 256 threads of a block, the same value in every thread: xor-shuffle tree over the lanes
// (wave_sum_d), then the four waves in order.  sh: 4 doubles.
// Single use: no barrier before the LDS write and none after the reads, so a block calls it ONCE on `sh` -- or puts a
// barrier of its own between two calls.
__device__ __forceinline__ double block_sum_d(double v, double* sh) {
  v = wave_sum_d(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// The same sum, callable again and again on the same four slots (a barrier on either side of the LDS write).
__device__ __forceinline__ double block_sum_d_again(double v, double* sh) {
  v = wave_sum_d(v);
  __syncthreads();       // (sh may still be read from an earlier call)
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// Two integer counts of a block added into a header (pb may be null: one count).  Integer sums are order-independent, so the
// atomics are bit-reproducible.  sh: int [2][4], single use; every thread passes the barrier inside.
__device__ __forceinline__ void block_count(int a, int b, int* pa, int* pb, int (*sh)[4]) {
  for (int o = 32; o > 0; o >>= 1) {
    a += __shfl_xor(a, o, 64);
    b += __shfl_xor(b, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    sh[0][threadIdx.x >> 6] = a;
    sh[1][threadIdx.x >> 6] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int ta = sh[0][0] + sh[0][1] + sh[0][2] + sh[0][3];
    const int tb = sh[1][0] + sh[1][1] + sh[1][2] + sh[1][3];
    if (ta) atomicAdd(pa, ta);
    if (tb && pb) atomicAdd(pb, tb);
  }
}

// One block over nblocks partials, fixed order: this thread's sum of partials t, t + 256, ... with eight loads in flight (the
// up-sampled loss leaves 16384 partials; one dependent round trip each was 64 us between the forward and the backward pass).
// The caller sums the threads with one of the block sums above.
__device__ __forceinline__ double thread_sum_partials(const double* __restrict__ partial, int nblocks) {
  double s = 0.0;
  int i = threadIdx.x;
  for (; i + 7 * 256 < nblocks; i += 8 * 256) {
    double t[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) t[k] = partial[i + k * 256];
#pragma unroll
    for (int k = 0; k < 8; ++k) s += t[k];
  }
  for (; i < nblocks; i += 256) s += partial[i];
  return s;
}

#endif  // __HIPCC__

// blocks of 256 threads for work_items, at least 1 and at most cap
static inline int capped_blocks(long long work_items, int cap) {
  long long b = (work_items + 255) / 256;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (int)b;
}

// workspace regions start on 256-byte boundaries
static inline int64_t align256(int64_t v) { return (v + 255) / 256 * 256; }

}  // namespace pseg
