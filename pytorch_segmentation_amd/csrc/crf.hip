// Local dense-CRF refinement of logits on gfx950 (Teichmann & Cipolla, "Convolutional CRFs for Semantic Segmentation",
// 2018): mean-field inference with the Kraehenbuehl-Koltun appearance and smoothness kernels truncated to a dilated
// (2R+1) x (2R+1) window.  Definition: include/pseg_amd.h; design and LDS budget: DESIGN.md 5k.
//  - Q lives pixel-major [B,h,w,CP] (pseg_softmax_views' layout, which also forms Q^0) in two ping-pong buffers: the
//    whole workspace.  One launch per iteration; the last one writes the NCHW logits L^T itself.
//  - A block owns a 32 x 16 tile, a thread two pixels of one column eight rows apart.  The guide tile with its R*D halo
//    (pre-multiplied by the guide scales) stays in LDS for the whole block; Q's tile with the same halo passes through LDS
//    one CLASS CHUNK (CC = 8 or 4 floats per pixel) at a time, stored as CC/4 planes of 16-byte vectors so that the lanes
//    of a wave -- consecutive x -- read consecutive vectors.  The pair weights are never stored: each chunk recomputes them
//    from the guide tile (an exp per pair and chunk; the accumulators of all classes would not fit the registers at C = 256).
//  - Each kernel's weights are taken relative to the pixel's largest one, exp(e - max e): the ratios of the definition do
//    not change, and a pixel whose every neighbour differs by more than ~170 grey levels (exp underflows in fp32) keeps a
//    finite message instead of 0 / 0.
//  - A thread writes its pixels' L^t chunk by chunk into the output buffer while it keeps the running maximum and sum of
//    exponentials, and then turns what it wrote into the softmax in place: reads only its own stores, no block-wide exchange.
#include "common.h"

#include <math.h>

namespace pseg {

constexpr int kCrfTW = 32, kCrfTH = 16;                    // the tile; 256 threads = 32 columns x 8 rows, two rows each
constexpr int kCrfMaxR = 5, kCrfMaxD = 4, kCrfMaxT = 10, kCrfMaxC = 256;
constexpr int kCrfLdsTwoBlocks = 80 * 1024;                // a tile up to here leaves room for a second block on the CU
constexpr int kCrfLdsStatic = 64 * 1024;                   // dynamic LDS beyond this needs the function attribute

struct CrfArgs {
  int C, CP, h, w, tiles_x, R, D;
  float g[3];              // guide scales
  float ia, ib, ig;        // 1 / (2 theta_alpha^2), 1 / (2 theta_beta^2), 1 / (2 theta_gamma^2)
  float wa, ws;
};

// The appearance exponent of the pair (centre colour cg, tile pixel q): -(spa + |colour difference|^2 * ib)
__device__ __forceinline__ float crf_ea(const float* Gs, int NP, int q, const float* cg, float spa, float ib) {
  const float d0 = cg[0] - Gs[q], d1 = cg[1] - Gs[NP + q], d2 = cg[2] - Gs[2 * NP + q];
  return -(spa + (d0 * d0 + d1 * d1 + d2 * d2) * ib);
}

// U and out may be one buffer (a thread reads its own pixels' logits before it writes them); qout is read back by the
// thread that wrote it.  qout != null: an inner iteration (Q^t, pixel-major); else the last one (L^T to out, NCHW).
template <int CC>
__global__ __launch_bounds__(256) void crf_iter_kernel(const float* U, const float* __restrict__ G, const float* __restrict__ qin,
                                                       float* qout, float* out, CrfArgs a, FastDiv pw_div) {
  extern __shared__ f32x4 crf_lds[];
  constexpr int NV = CC / 4;
  const int H = a.R * a.D, PW = kCrfTW + 2 * H, PH = kCrfTH + 2 * H, NP = PW * PH;
  f32x4* Qs = crf_lds;                                        // [NV][NP]
  float* Gs = reinterpret_cast<float*>(crf_lds + NV * NP);    // [3][NP]
  const int tid = threadIdx.x, b = blockIdx.y;
  const int tile_y = blockIdx.x / a.tiles_x, tile_x = blockIdx.x - tile_y * a.tiles_x;
  const int y0 = tile_y * kCrfTH, x0 = tile_x * kCrfTW;
  const int h = a.h, w = a.w, C = a.C, n4 = a.CP / 4;
  const int64_t plane = (int64_t)h * w;

  for (int r = tid; r < NP; r += 256) {
    const int py = (int)pw_div.div((uint32_t)r), px = r - py * PW;
    const int gy = y0 - H + py, gx = x0 - H + px;
    const bool in = (unsigned)gy < (unsigned)h && (unsigned)gx < (unsigned)w;
#pragma unroll
    for (int c = 0; c < 3; ++c)
      Gs[c * NP + r] = in ? G[((int64_t)b * 3 + c) * plane + (int64_t)gy * w + gx] * a.g[c] : 0.f;
  }
  __syncthreads();

  const int tx = tid & 31, ty = tid >> 5;
  const int gx = x0 + tx;
  int gy[2], ci[2];
  bool ok[2];
  float cg[2][3], Ma[2], Ms[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    gy[i] = y0 + ty + 8 * i;
    ci[i] = (ty + 8 * i + H) * PW + tx + H;
    ok[i] = gx < w && gy[i] < h;
#pragma unroll
    for (int c = 0; c < 3; ++c) cg[i][c] = Gs[c * NP + ci[i]];
    Ma[i] = Ms[i] = -INFINITY;
  }
  // the largest exponent of each kernel over the pixel's in-image neighbours
  for (int dy = -a.R; dy <= a.R; ++dy) {
    for (int dx = -a.R; dx <= a.R; ++dx) {
      if (dy == 0 && dx == 0) continue;
      const float d2 = (float)(a.D * a.D * (dy * dy + dx * dx));
      const int off = (dy * PW + dx) * a.D;
      const bool xin = (unsigned)(gx + dx * a.D) < (unsigned)w;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        if (ok[i] && xin && (unsigned)(gy[i] + dy * a.D) < (unsigned)h) {
          Ma[i] = fmaxf(Ma[i], crf_ea(Gs, NP, ci[i] + off, cg[i], d2 * a.ia, a.ib));
          Ms[i] = fmaxf(Ms[i], -d2 * a.ig);
        }
      }
    }
  }

  float M[2] = {-INFINITY, -INFINITY}, S[2] = {0.f, 0.f};      // the running softmax of an inner iteration
  const int nchunks = (a.CP + CC - 1) / CC;
  for (int ch = 0; ch < nchunks; ++ch) {
    const int v0 = ch * NV;
    for (int i = tid; i < NP * NV; i += 256) {
      const int r = i / NV, j = i - r * NV;
      const int py = (int)pw_div.div((uint32_t)r), px = r - py * PW;
      const int qy = y0 - H + py, qx = x0 - H + px;
      f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
      if ((unsigned)qy < (unsigned)h && (unsigned)qx < (unsigned)w && v0 + j < n4)
        v = reinterpret_cast<const f32x4*>(qin)[(((int64_t)b * h + qy) * w + qx) * n4 + v0 + j];
      Qs[j * NP + r] = v;
    }
    __syncthreads();

    float u[2][CC];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int e = 0; e < CC; ++e) {
        const int c = ch * CC + e;
        u[i][e] = ok[i] && c < C ? U[((int64_t)b * C + c) * plane + (int64_t)gy[i] * w + gx] : 0.f;
      }
    }
    f32x4 aa[2][NV], as[2][NV];
    float na[2] = {0.f, 0.f}, ns[2] = {0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int j = 0; j < NV; ++j) aa[i][j] = as[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (int dy = -a.R; dy <= a.R; ++dy) {
      for (int dx = -a.R; dx <= a.R; ++dx) {
        if (dy == 0 && dx == 0) continue;
        const float d2 = (float)(a.D * a.D * (dy * dy + dx * dx));
        const int off = (dy * PW + dx) * a.D;
        const bool xin = (unsigned)(gx + dx * a.D) < (unsigned)w;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          if (ok[i] && xin && (unsigned)(gy[i] + dy * a.D) < (unsigned)h) {     // interior waves take it whole
            const int q = ci[i] + off;
            const float ka = expf(crf_ea(Gs, NP, q, cg[i], d2 * a.ia, a.ib) - Ma[i]);
            const float ks = expf(-d2 * a.ig - Ms[i]);
            na[i] += ka;
            ns[i] += ks;
#pragma unroll
            for (int j = 0; j < NV; ++j) {
              const f32x4 v = Qs[j * NP + q];
              aa[i][j] += ka * v;
              as[i][j] += ks * v;
            }
          }
        }
      }
    }

#pragma unroll
    for (int i = 0; i < 2; ++i) {
      if (!ok[i]) continue;
      // every in-image neighbour's weight is in (0, 1] and the largest is 1; no neighbour at all (D >= the image): no message
      const float ra = na[i] > 0.f ? a.wa / na[i] : 0.f, rs = ns[i] > 0.f ? a.ws / ns[i] : 0.f;
      float L[CC];
#pragma unroll
      for (int e = 0; e < CC; ++e) L[e] = u[i][e] + (aa[i][e >> 2][e & 3] * ra + as[i][e >> 2][e & 3] * rs);
      if (!qout) {
#pragma unroll
        for (int e = 0; e < CC; ++e) {
          const int c = ch * CC + e;
          if (c < C) out[((int64_t)b * C + c) * plane + (int64_t)gy[i] * w + gx] = L[e];
        }
        continue;
      }
      float m = M[i];
#pragma unroll
      for (int e = 0; e < CC; ++e) {
        if (ch * CC + e < C) m = fmaxf(m, L[e]);
        else L[e] = -INFINITY;                                 // pad lanes: exp gives the 0 the layout asks for
      }
      float s = S[i] * expf(M[i] - m);                         // first chunk: 0 * exp(-inf) = 0
#pragma unroll
      for (int e = 0; e < CC; ++e) s += expf(L[e] - m);
      M[i] = m;
      S[i] = s;
      f32x4* o = reinterpret_cast<f32x4*>(qout) + (((int64_t)b * h + gy[i]) * w + gx) * n4 + v0;
#pragma unroll
      for (int j = 0; j < NV; ++j)
        if (v0 + j < n4) o[j] = f32x4{L[4 * j], L[4 * j + 1], L[4 * j + 2], L[4 * j + 3]};
    }
    __syncthreads();                                           // the tile is free for the next chunk
  }

  if (qout) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      if (!ok[i]) continue;
      f32x4* o = reinterpret_cast<f32x4*>(qout) + (((int64_t)b * h + gy[i]) * w + gx) * n4;
      for (int j = 0; j < n4; ++j) {
        f32x4 v = o[j];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = expf(v[e] - M[i]) / S[i];
        o[j] = v;
      }
    }
  }
}

static inline int64_t crf_up16(int64_t n) { return (n + 15) & ~(int64_t)15; }

static bool crf_sizes_ok(int B, int C, int h, int w) {
  return B >= 1 && B <= 65535 && h >= 1 && h <= 65535 && w >= 1 && w <= 65535 && (int64_t)h * w > 1 && C >= 1 && C <= kCrfMaxC;
}

// bytes of one Q buffer [B,h,w,CP]
static int64_t crf_q_bytes(int B, int C, int h, int w) { return (int64_t)B * h * w * class_pad(C) * 4; }

static size_t crf_lds_bytes(int R, int D, int CC) {
  const int H = R * D;
  return (size_t)(kCrfTW + 2 * H) * (kCrfTH + 2 * H) * (CC + 3) * sizeof(float);
}

template <int CC>
static int crf_launch(dim3 grid, size_t lds, hipStream_t st, const float* U, const float* G, const float* qin, float* qout,
                      float* out, const CrfArgs& a) {
  if (lds > (size_t)kCrfLdsStatic) {
    static bool raised = false;                                // per instantiation; the value never changes
    if (!raised) {
      if (hipFuncSetAttribute(reinterpret_cast<const void*>(&crf_iter_kernel<CC>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024) != hipSuccess) {
        (void)hipGetLastError();
        set_error("crf_refine: the device refused %zu bytes of LDS per block", lds);
        return PSEG_ERR_HIP;
      }
      raised = true;
    }
  }
  hipLaunchKernelGGL(crf_iter_kernel<CC>, grid, dim3(256), lds, st, U, G, qin, qout, out, a,
                     FastDiv((uint32_t)(kCrfTW + 2 * a.R * a.D)));
  return PSEG_OK;
}

}  // namespace pseg

using namespace pseg;

extern "C" {

int64_t pseg_crf_workspace_bytes(int B, int C, int h, int w) {
  if (!crf_sizes_ok(B, C, h, w) || crf_q_bytes(B, C, h, w) >= (1ll << 31)) return -1;
  return 2 * crf_up16(crf_q_bytes(B, C, h, w));
}

int pseg_crf_refine(const float* logits, const float* guide, int B, int C, int h, int w, float g0, float g1, float g2, int R, int D,
                    int T, float theta_alpha, float theta_beta, float theta_gamma, float w_a, float w_s, float* out, void* workspace,
                    int64_t workspace_bytes, void* stream) {
  PSEG_REQUIRE(logits && guide && out && workspace, "crf_refine: null pointer");
  PSEG_REQUIRE(B >= 1 && B <= 65535 && h >= 1 && h <= 65535 && w >= 1 && w <= 65535,
               "crf_refine: sizes B, h, w = %d, %d, %d outside [1, 65535]", B, h, w);
  PSEG_REQUIRE((int64_t)h * w > 1, "crf_refine: a 1 x 1 map has no neighbours");
  PSEG_REQUIRE(C >= 1 && C <= kCrfMaxC, "crf_refine: %d classes; 1 <= C <= %d supported", C, kCrfMaxC);
  PSEG_REQUIRE(R >= 1 && R <= kCrfMaxR, "crf_refine: radius R = %d outside [1, %d]", R, kCrfMaxR);
  PSEG_REQUIRE(D >= 1 && D <= kCrfMaxD, "crf_refine: dilation D = %d outside [1, %d]", D, kCrfMaxD);
  PSEG_REQUIRE(T >= 1 && T <= kCrfMaxT, "crf_refine: iterations T = %d outside [1, %d]", T, kCrfMaxT);
  PSEG_REQUIRE(isfinite(theta_alpha) && isfinite(theta_beta) && isfinite(theta_gamma) && theta_alpha > 0.f && theta_beta > 0.f &&
                   theta_gamma > 0.f,
               "crf_refine: theta_alpha, theta_beta, theta_gamma = %g, %g, %g must be finite and > 0", theta_alpha, theta_beta,
               theta_gamma);
  const float ia = 1.f / (2.f * theta_alpha * theta_alpha), ib = 1.f / (2.f * theta_beta * theta_beta);
  const float ig = 1.f / (2.f * theta_gamma * theta_gamma);
  PSEG_REQUIRE(isfinite(ia) && isfinite(ib) && isfinite(ig), "crf_refine: a theta of %g, %g, %g is too small: 1 / (2 theta^2) overflows",
               theta_alpha, theta_beta, theta_gamma);
  PSEG_REQUIRE(isfinite(w_a) && isfinite(w_s) && w_a >= 0.f && w_s >= 0.f, "crf_refine: weights w_a, w_s = %g, %g must be finite and >= 0",
               w_a, w_s);
  PSEG_REQUIRE(isfinite(g0) && isfinite(g1) && isfinite(g2) && g0 >= 0.f && g1 >= 0.f && g2 >= 0.f,
               "crf_refine: guide scales %g, %g, %g must be finite and >= 0", g0, g1, g2);
  const int64_t qb = crf_q_bytes(B, C, h, w);
  PSEG_REQUIRE((int64_t)B * C * h * w * 4 < (1ll << 31) && (int64_t)B * 3 * h * w * 4 < (1ll << 31) && qb < (1ll << 31),
               "crf_refine: an operand of [%d,%d,%d,%d] reaches 2 GiB; split the batch", B, C, h, w);
  const int64_t need = 2 * crf_up16(qb);
  PSEG_REQUIRE(((uintptr_t)workspace & 15) == 0, "crf_refine: the workspace must be 16-byte aligned");
  PSEG_REQUIRE(workspace_bytes >= need, "crf_refine: workspace too small (%lld < %lld bytes)", (long long)workspace_bytes,
               (long long)need);
  const char* wsb = (const char*)workspace;
  const int64_t ubytes = (int64_t)B * C * h * w * 4;
  PSEG_REQUIRE((const char*)out + ubytes <= wsb || wsb + need <= (const char*)out, "crf_refine: out lies inside the workspace");
  PSEG_REQUIRE(out != guide, "crf_refine: out must not be the guide");
  const hipStream_t st = (hipStream_t)stream;
  if (w_a == 0.f && w_s == 0.f) {                              // L^T = U whatever T: the input's bits, -0 and NaN included
    if (out != logits && hipMemcpyAsync(out, logits, (size_t)ubytes, hipMemcpyDeviceToDevice, st) != hipSuccess) {
      set_error("crf_refine: copy failed: %s", hipGetErrorString(hipGetLastError()));
      return PSEG_ERR_HIP;
    }
    return PSEG_OK;
  }
  float* q[2] = {(float*)workspace, (float*)((char*)workspace + crf_up16(qb))};
  const int CP = class_pad(C);
  if (int rc = pseg_softmax_views(logits, B, 0, C, h, w, q[0], 0, (int64_t)B * h * w * CP, stream)) return rc;     // Q^0
  CrfArgs a;
  a.C = C, a.CP = CP, a.h = h, a.w = w, a.tiles_x = cdiv(w, kCrfTW), a.R = R, a.D = D;
  a.g[0] = g0, a.g[1] = g1, a.g[2] = g2;
  a.ia = ia, a.ib = ib, a.ig = ig;
  a.wa = w_a, a.ws = w_s;
  const dim3 grid((unsigned)(a.tiles_x * cdiv(h, kCrfTH)), (unsigned)B);
  const bool wide = crf_lds_bytes(R, D, 8) <= (size_t)kCrfLdsTwoBlocks;
  const size_t lds = crf_lds_bytes(R, D, wide ? 8 : 4);
  for (int t = 1; t <= T; ++t) {
    float* qo = t < T ? q[t & 1] : nullptr;
    const int rc = wide ? crf_launch<8>(grid, lds, st, logits, guide, q[(t - 1) & 1], qo, out, a)
                        : crf_launch<4>(grid, lds, st, logits, guide, q[(t - 1) & 1], qo, out, a);
    if (rc) return rc;
  }
  PSEG_LAUNCH_CHECK();
  return PSEG_OK;
}

}  // extern "C"
