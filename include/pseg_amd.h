/* pseg_amd.h -- C ABI of libpseg_amd.so: the MI355X (gfx950) hot path of
 * WoodsGao/pytorch_segmentation, hand-written HIP.
 *
 * The reference has no native layer: its hot path is stock torch ops dispatched from
 * Python (conv2d / batch_norm / relu / interpolate / cross_entropy / max).  Each entry
 * point below names the reference call site (file:line under the reference tree) whose
 * arithmetic it replaces.  A reference maintainer binds these with ctypes (see
 * INTEGRATION.md); pytorch_segmentation_amd/_lib.py is exactly that binding.
 *
 * Conventions
 *  - Every pointer is a DEVICE pointer owned by the caller (PyTorch's caching allocator
 *    in practice); the library never allocates or frees device memory.  Scratch is passed
 *    in as (workspace, workspace_bytes); pseg_*_workspace_bytes() gives the size.
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream).  All work is
 *    enqueued on it; nothing here synchronises the host, so calls are graph-capturable.
 *  - Activations are fp32 NHWC: element (b,h,w,c) of a tensor with pixel stride `ld`
 *    (in floats, ld >= C, ld % 4 == 0, base 16-byte aligned) lives at
 *    ((b*H + h)*W + w)*ld + c.  A channel slice of a wider concat buffer is simply a
 *    base pointer + ld of the wide buffer: concatenation costs no copy.
 *  - Conv weights are [Cout][kh][kw][Cin] (= a torch OIHW tensor in channels_last memory
 *    format), Cin % 4 == 0.  Logits / targets for the loss are NCHW fp32 / NHW int64, as
 *    the reference's nn.CrossEntropyLoss sees them.
 *  - Every tensor must be smaller than 2 GiB (32-bit buffer-descriptor addressing).
 *  - Return value: 0 on success, negative on error (PSEG_ERR_*); pseg_last_error() gives
 *    the message for the calling thread.  Nothing aborts the process.
 *  - Thread safety: functions are re-entrant; they keep no global state besides the
 *    thread-local error string (autograd calls backward from its own worker thread).
 */
#ifndef PSEG_AMD_H
#define PSEG_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PSEG_OK 0
#define PSEG_ERR_ARG (-1)
#define PSEG_ERR_HIP (-2)
#define PSEG_ERR_WORKSPACE (-3)

/* conv arithmetic (all accumulate in fp32):
 *  FP32    exact fp32 products on v_mfma_f32_32x32x2_f32;
 *  BF16X3  each fp32 operand split into two bf16 limbs, a*b = ah*bh + ah*bl + al*bh on v_mfma_f32_32x32x16_bf16
 *          (~17 significant bits per product);
 *  BF16X6  three bf16 limbs (exactly the 24 mantissa bits) and the six partial products down to 2^-16:
 *          error ~2^-23 per product, i.e. fp32-equivalent results at 6/16 of the fp32-MFMA instruction time. */
#define PSEG_PREC_FP32 0
#define PSEG_PREC_BF16X3 1
#define PSEG_PREC_BF16X6 2
/*  FP16X3  two fp16 limbs (22-bit operands) of the operand scaled by an exact power of two taken from its per-tensor
 *          max|x| (`amax_*`: device pointer to one float, maintained with pseg_amax / the producer kernels);
 *          ~2^-22 per product at the BF16X3 cost.  fwd / dgrad only. */
#define PSEG_PREC_FP16X3 3

#define PSEG_ACT_NONE 0
#define PSEG_ACT_RELU 1
#define PSEG_ACT_RELU6 2

/* bumped whenever an existing prototype changes incompatibly; pseg_abi_version() returns the value the library was built with.
 * Entry points added since 14 (pseg_image_preprocess_views, pseg_softmax_views, pseg_seg_decode_ensemble, the
 * connected-region calls pseg_regions_workspace_bytes, pseg_mask_label, pseg_mask_regions, pseg_mask_clean, and the
 * sliding-window calls pseg_image_preprocess_windows, pseg_seg_decode_windows, and the grouped optimiser calls
 * pseg_grad_sumsq_workspace_bytes, pseg_grad_sumsq, pseg_opt_step_sgd, pseg_opt_step_adam, and the contour-measure calls
 * pseg_label_depth, pseg_boundary_counts_workspace_bytes, pseg_boundary_counts, and the outline calls
 * pseg_mask_rings_workspace_bytes, pseg_mask_rings, and the dense-CRF calls pseg_crf_workspace_bytes, pseg_crf_refine, and
 * the surface-loss calls pseg_class_sdist_workspace_bytes, pseg_class_sdist, pseg_surface_workspace_bytes, pseg_surface_fwd_bwd,
 * and the surface-distance calls pseg_hausdorff_workspace_bytes, pseg_hausdorff_stats) are purely
 * additive and do not bump it: the loader checks every declared prototype against the library's exports by name. */
#define PSEG_ABI_VERSION 14
int pseg_abi_version(void);
const char* pseg_last_error(void);
/* The PSEG_CONV_* / PSEG_WGRAD_* planning overrides are read from the environment once, at the first launch;
 * call this after changing them at run time (tests do). */
int pseg_config_reload(void);

/* ------------------------------------------------------------------ convolution
 * Replaces torch conv2d as used by ConvNormAct / nn.Conv2d on the hot path:
 * models/aspp.py:12,27-30  models/deeplabv3plus.py:20,22  models/unet.py:19-23
 * (padding = (k-1)/2*dilation for ConvNormAct, 1 for the 3x3 cls_conv).
 * Implicit GEMM on v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulate).
 *
 * pseg_conv2d_fwd:  y[b,ho,wo,:] = sum_{r,s,ci} x[b,ho*stride-pad+r*dil, wo*stride-pad+s*dil, ci] * w[:,r,s,ci] (+bias)
 *   stat (nullable): column statistics of y per row group, float [3][rows][Cout] with
 *   rows = pseg_conv2d_stat_rows(...), each group covering pseg_conv2d_stat_group(...) consecutive
 *   GEMM rows (= pixels in the kernel's own order: row-major, or patch-major for dilated convs): [0] = pivot K (the group's first sample), [1] = sum(y-K), [2] = sum((y-K)^2).
 *   Shifted sums keep the variance exact to fp32 even when |mean| >> std; consumed by
 *   pseg_bn_finalize (fuses the BatchNorm batch-statistics pass into the conv epilogue).
 *   accumulate != 0: y += result.
 */
int pseg_conv2d_fwd(const float* x, int ldx, const float* w, const float* bias, float* y, int ldy,
                    int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int kh, int kw,
                    int stride, int pad, int dil, int accumulate, int precision, const float* amax_x,
                    const float* amax_w, float* stat, void* workspace, int64_t workspace_bytes, void* stream);
int pseg_conv2d_stat_rows(int B, int Ho, int Wo, int Cin, int Cout, int kh, int kw, int stride, int pad, int dil);
int pseg_conv2d_stat_group(int B, int Ho, int Wo, int Cin, int Cout, int kh, int kw, int stride, int pad, int dil);
int64_t pseg_conv2d_fwd_workspace_bytes(int B, int Ho, int Wo, int Cin, int Cout, int kh, int kw);

/* dgrad: dx[b,h,w,ci] = sum_{r,s,co} dy[b,(h+pad-r*dil)/stride,(w+pad-s*dil)/stride,co] * w[co,r,s,ci]
 * wT is the transposed filter [Cin][kh][kw][Cout] made by pseg_filter_transpose.
 * accumulate != 0: dx += result (merges the two gradient paths of a residual block). */
int pseg_conv2d_dgrad(const float* dy, int ldy, const float* wT, float* dx, int ldx,
                      int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int kh, int kw,
                      int stride, int pad, int dil, int accumulate, int precision, const float* amax_dy,
                      const float* amax_w, void* workspace, int64_t workspace_bytes, void* stream);
/* The same data gradient (exact fp32, no accumulate) when dx is the gradient dz of the BatchNorm + activation layer that produced
 * the conv's input -- conv -> BN -> ReLU -> THIS conv, the interior of every ConvNormAct chain and ResNet bottleneck (reference
 * models/aspp.py:27-30, models/unet.py:19-23 via pytorch_modules' ConvNormAct; one consumer, no residual).  While the tile is
 * stored, the epilogue reads that layer's saved conv output y_prev at the same pixels, recomputes the activation mask from it
 * exactly as pseg_bn_act_fwd applied it ((y - mean) * scale + shift against 0 / 6), and writes the per-row-group partial sums
 * part_db[g][c] = sum dz * act', part_dg[g][c] = sum dz * act' * (y - mean) * invstd -- what pseg_bn_act_bwd_reduce would re-read
 * dz and y for: one activation-sized read less per layer, one launch fewer on the backward chain.  part_db / part_dg are
 * [part_rows][Cin] floats, fed to pseg_bn_bwd_finalize as they are.  pseg_conv2d_dgrad_bnstat_rows(...) -> part_rows, or 0 when
 * this problem does not run on the kernel that carries the sums (channel counts not multiples of 32, split-K plans): the caller
 * then uses pseg_conv2d_dgrad + pseg_bn_act_bwd_reduce. */
int pseg_conv2d_dgrad_bnstat_rows(int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad,
                                  int dil);
int pseg_conv2d_dgrad_bnstat(const float* dy, int ldy, const float* wT, float* dx, int ldx, int B, int H, int W, int Cin, int Ho,
                             int Wo, int Cout, int kh, int kw, int stride, int pad, int dil, const float* y_prev, int ldy_prev,
                             const float* mean, const float* invstd, const float* scale, const float* shift, int act,
                             float* part_db, float* part_dg, int part_rows, void* stream);
int pseg_filter_transpose(const float* w, float* wT, int Cout, int taps, int Cin, void* stream);
/* BF16X3 data gradient on PRE-SPLIT operands (the fast form of the split-bf16 arithmetic: the consumer neither splits nor
 * stages through registers -- its tiles go global -> LDS by DMA).  pseg_split_planes writes the two bf16 limb planes of an
 * fp32 [M][C] tensor (hi = bf16(x), lo = bf16(x - hi); [M][ldp] uint16 each, ldp % 8 == 0, columns >= C zeroed); results
 * are bit-identical to pseg_conv2d_dgrad(..., PSEG_PREC_BF16X3) up to the accumulation grouping.
 * pseg_conv2d_dgrad_planes_ok(...) != 0 says whether the shape is covered (dy channels % 32 == 0, Cin >= 128, enough
 * 256x128 tiles to fill the chip); otherwise call pseg_conv2d_dgrad. */
int pseg_split_planes(const float* x, int ldx, int64_t M, int C, uint16_t* hi, uint16_t* lo, int ldp, void* stream);
int pseg_conv2d_dgrad_planes_ok(int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int kh, int kw, int stride,
                                int pad, int dil);
int pseg_conv2d_dgrad_planes(const uint16_t* dy_hi, const uint16_t* dy_lo, int ldp, const uint16_t* wT_hi,
                             const uint16_t* wT_lo, float* dx, int ldx, int B, int H, int W, int Cin, int Ho, int Wo,
                             int Cout, int kh, int kw, int stride, int pad, int dil, int accumulate, void* stream);
/* every filter of a model in one launch.  jobs: device array of n records of six int64
 * {w (device address), wT (device address), Cout, taps, Cin, index of the record's first 32x32 tile}, tile indices
 * ascending from 0; a record covers taps * ceil(Cout/32) * ceil(Cin/32) tiles; total_tiles = their sum. */
int pseg_filter_transpose_batch(const int64_t* jobs, int n, int64_t total_tiles, void* stream);

/* wgrad: dw[co,r,s,ci] = sum_{b,ho,wo} dy[b,ho,wo,co] * x[b,ho*stride-pad+r*dil, wo*stride-pad+s*dil, ci]
 * Split over pixels into workspace slabs that are reduced in a fixed order (bit-reproducible).
 * accumulate != 0: dw += result (gradient accumulation over micro-batches, train.py --accumulate). */
int pseg_conv2d_wgrad(const float* x, int ldx, const float* dy, int ldy, float* dw,
                      int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int kh, int kw,
                      int stride, int pad, int dil, int accumulate, int precision, int concurrent,
                      void* workspace, int64_t workspace_bytes, void* stream);
/* concurrent != 0 (here and in pseg_conv2d_wgrad_splits / _slabs; the three must agree): the launch runs beside another
 * stream's kernels -- the training step puts its weight gradients on a second stream next to the data gradients -- and the
 * exact-fp32 plan then splits the pixels for ONE resident block per CU (half the slabs: 2.2 GB less written and re-read per
 * DeepLabV3+ step); 0: the launch has the chip to itself and gets two.  The workspace size covers both. */
int64_t pseg_conv2d_wgrad_workspace_bytes(int B, int Ho, int Wo, int Cin, int Cout, int kh, int kw);
/* The same weight gradient with the slab reduction DEFERRED: a training step runs ~60 (DeepLabV3+) to ~300 (HRNet) split
 * weight gradients, and their reductions are launch-bound one by one (23 us each for 37 MB on average).
 * pseg_conv2d_wgrad_splits: slab count of the plan (1: not split -- call pseg_conv2d_wgrad).  pseg_conv2d_wgrad_slabs
 * leaves the `splits` partial gradients in `slabs` ([splits][Cout][kh][kw][Cin] floats, slab_bytes >= that; the caller
 * keeps one such region per layer alive until the reduction).  pseg_slab_reduce_batch then reduces every layer of the
 * backward pass in ONE launch, slabs in a fixed order (bit-reproducible): jobs = device array of n records of five int64
 * {slabs (device address), dw (device address), elements per slab (% 4 == 0), slab count, index of the record's first
 * block}, block indices ascending from 0, a record covers ceil(elements / pseg_slab_reduce_block()) blocks, total_blocks
 * = their sum.  accumulate != 0: dw += sum (train.py --accumulate). */
int pseg_conv2d_wgrad_splits(int B, int Ho, int Wo, int Cin, int Cout, int kh, int kw, int precision, int concurrent);
int pseg_conv2d_wgrad_slabs(const float* x, int ldx, const float* dy, int ldy, float* slabs, int B, int H, int W, int Cin,
                            int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad, int dil, int precision,
                            int concurrent, int64_t slab_bytes, void* stream);
int pseg_slab_reduce_batch(const int64_t* jobs, int n, int64_t total_blocks, int accumulate, void* stream);
int pseg_slab_reduce_block(void);

/* ------------------------------------------------------------------ half-precision (`-mp`) convolution
 * The reference's mixed-precision mode (train.py:70 `-mp`, :102-105, :138; README.md:12 -- apex: fp16 compute, fp32 master
 * weights, loss scaling).  Activations, their gradients and the filters are IEEE binary16 in memory (pseg_half_t = the bit
 * pattern), element strides as in the fp32 entry points, C % 8 == 0, ld % 8 == 0, 16-byte aligned bases; products are exact
 * (fp16 x fp16 on v_mfma_f32_32x32x16_f16) and every sum is fp32.
 * pseg_conv2d_fwd_h: y fp16, or fp32 when y_is_f32 (the class logits, which the loss reads in fp32); stat as pseg_conv2d_fwd
 *   with the row grouping of pseg_conv2d_stat_rows_h / _group_h, taken over y AS STORED: an fp16 result is rounded before it is
 *   summed (the layer normalises the values it reads back), an fp32 result is summed from the accumulators.  bias is fp32.
 * pseg_conv2d_dgrad_h: wT = the transposed fp16 filter [Cin][kh][kw][Cout].
 * pseg_conv2d_wgrad_h: dw fp32 [Cout][kh][kw][Cin] (the master gradient arena); split / slab protocol as pseg_conv2d_wgrad.
 * pseg_filter_prepare_h: every dense filter of a model in one launch, from the fp32 master weights: the fp16 copy AND the
 *   transposed fp16 copy, both optionally padded further than the master (8-channel granules; padding zero-filled).  jobs:
 *   device array of n records of nine int64 {w fp32 [Cout][taps][Cin], w_h [CoutP][taps][CinP], wT_h [CinP][taps][CoutP]
 *   (device addresses; either output may be 0), Cout, taps, Cin, CoutP, CinP, index of the record's first 32x32 tile}; a
 *   record covers taps * ceil(CoutP/32) * ceil(CinP/32) tiles, tile indices ascending from 0.
 * pseg_convert2d: y[M][C] = convert(x[M][C] * scale) between fp32 / fp16 tensors (x_is_half / y_is_half), scale = *dev_scale
 *   when non-NULL (a device scalar: the dynamic loss scale multiplies the loss gradient on its way into fp16). */
typedef uint16_t pseg_half_t;
int pseg_conv2d_fwd_h(const pseg_half_t* x, int ldx, const pseg_half_t* w, const float* bias, void* y, int ldy, int y_is_f32,
                      int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad, int dil,
                      int accumulate, float* stat, void* stream);
int pseg_conv2d_stat_rows_h(int B, int Ho, int Wo, int Cin, int Cout, int kh, int kw, int stride, int pad, int dil);
int pseg_conv2d_stat_group_h(int B, int Ho, int Wo, int Cin, int Cout, int kh, int kw, int stride, int pad, int dil);
int pseg_conv2d_dgrad_h(const pseg_half_t* dy, int ldy, const pseg_half_t* wT, pseg_half_t* dx, int ldx, int B, int H, int W,
                        int Cin, int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad, int dil, int accumulate,
                        void* stream);
/* pseg_conv2d_dgrad_bnstat_h: pseg_conv2d_dgrad_bnstat for the fp16 tensors (dx overwritten; y_prev fp16 with ldy_prev % 8 == 0;
 * the sums are taken over dx AS STORED, i.e. rounded to fp16, like pseg_bn_act_bwd_reduce_h reading it back).  The plain
 * instantiations of the tiles and (K-step, ring depth) pairs the default plan gives such data gradients carry the epilogue;
 * pseg_conv2d_dgrad_bnstat_rows_h is 0 for an invalid problem AND for one whose kernel does not (tap-skipping, channels off the
 * K-step grid, a forced tile / K-step / ring depth outside that set): the caller then runs pseg_conv2d_dgrad_h and the layer's
 * own reduction pass, and pseg_conv2d_dgrad_bnstat_h refuses the problem -- never a launch without the sums. */
int pseg_conv2d_dgrad_bnstat_rows_h(int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad,
                                    int dil);
int pseg_conv2d_dgrad_bnstat_h(const pseg_half_t* dy, int ldy, const pseg_half_t* wT, pseg_half_t* dx, int ldx, int B, int H, int W,
                               int Cin, int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad, int dil,
                               const pseg_half_t* y_prev, int ldy_prev, const float* mean, const float* invstd, const float* scale,
                               const float* shift, int act, float* part_db, float* part_dg, int part_rows, void* stream);
int pseg_conv2d_wgrad_h(const pseg_half_t* x, int ldx, const pseg_half_t* dy, int ldy, float* dw, int B, int H, int W,
                        int Cin, int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad, int dil, int accumulate,
                        void* workspace, int64_t workspace_bytes, void* stream);
int64_t pseg_conv2d_wgrad_workspace_bytes_h(int B, int Ho, int Wo, int Cin, int Cout, int kh, int kw);
int pseg_conv2d_wgrad_splits_h(int B, int Ho, int Wo, int Cin, int Cout, int kh, int kw);
int pseg_conv2d_wgrad_slabs_h(const pseg_half_t* x, int ldx, const pseg_half_t* dy, int ldy, float* slabs, int B, int H,
                              int W, int Cin, int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad, int dil,
                              int64_t slab_bytes, void* stream);
int pseg_filter_prepare_h(const int64_t* jobs, int n, int64_t total_tiles, void* stream);
int pseg_convert2d(const void* x, int x_is_half, int ldx, void* y, int y_is_half, int ldy, int64_t M, int C,
                   const float* dev_scale, void* stream);

/* fp16-storage variants of the bandwidth-bound passes: the same kernels instantiated on 2-byte activations (arguments and
 * semantics of the entry point without the suffix; statistics, per-channel vectors, filters of the depthwise convs and
 * every sum stay fp32; the amax / limb-plane arguments of the fp32 forms do not exist here).  Under `-mp` these halve the
 * bytes of the passes that are 40 % of a step's HBM traffic.
 * Every fp16 tensor needs ld % 8 == 0.  pseg_bn_act_fwd_h, pseg_bn_act_bwd_reduce_h and pseg_bn_act_bwd_apply_h work in lanes of
 * eight channels and need C % 8 == 0 as well (refused with PSEG_ERR_ARG otherwise); the others here take C % 4 == 0. */
int pseg_col_stats_h(const pseg_half_t* y, int ldy, int64_t M, int C, float* stat, void* stream);
int pseg_bn_act_fwd_h(const pseg_half_t* y, int ldy, const float* mean, const float* scale, const float* shift,
                      const pseg_half_t* residual, int ldr, int act, pseg_half_t* z, int ldz, int64_t M, int C,
                      uint32_t* mask_out, void* stream);
int pseg_bn_fwd_fused_h(const float* stat, int rows, int group, int64_t count, int C, const float* gamma, const float* beta,
                        float* running_mean, float* running_var, float momentum, float eps, float* mean, float* invstd,
                        float* scale, float* shift, const pseg_half_t* y, int ldy, const pseg_half_t* residual, int ldr,
                        int act, pseg_half_t* z, int ldz, int64_t M, void* stream);
int pseg_bn_bwd_fused_h(const float* part_db, const float* part_dg, int rows, int64_t count, int C, float* dgamma,
                        float* dbeta, int accumulate, int frozen, const pseg_half_t* dz, int lddz, const pseg_half_t* z,
                        int ldz, const pseg_half_t* y, int ldy, const float* mean, const float* invstd, const float* scale,
                        const float* shift, int act, pseg_half_t* dy, int lddy, pseg_half_t* dres, int lddres,
                        int res_accumulate, int64_t M, void* stream);
int pseg_bn_act_bwd_reduce_h(const pseg_half_t* dz, int lddz, const pseg_half_t* z, int ldz, const pseg_half_t* y, int ldy,
                             const float* mean, const float* invstd, const float* scale, const float* shift, int act,
                             int64_t M, int C, float* part_db, float* part_dg, const uint32_t* mask, void* stream);
int pseg_bn_act_bwd_apply_h(const pseg_half_t* dz, int lddz, const pseg_half_t* z, int ldz, const pseg_half_t* y, int ldy,
                            const float* mean, const float* invstd, const float* scale, const float* shift, const float* c1,
                            const float* c2, int act, pseg_half_t* dy, int lddy, pseg_half_t* dres, int lddres,
                            int res_accumulate, int64_t M, int C, const uint32_t* mask, void* stream);
int pseg_act_bwd_h(const pseg_half_t* dz, int lddz, const pseg_half_t* z, int ldz, const float* scale, int act,
                   pseg_half_t* dy, int lddy, pseg_half_t* dres, int lddres, int res_accumulate, int64_t M, int C,
                   void* stream);
int pseg_col_sum_h(const pseg_half_t* dy, int ldy, int64_t M, int C, float* out, int accumulate, void* workspace,
                   int64_t workspace_bytes, void* stream);
int pseg_copy2d_h(const pseg_half_t* x, int ldx, pseg_half_t* y, int ldy, int64_t M, int C, int accumulate, void* stream);
int pseg_pool_sum_h(const pseg_half_t* x, int ldx, int B, int HW, int C, float scale, pseg_half_t* out, int ldo,
                    void* stream);
int pseg_broadcast_h(const pseg_half_t* x, int ldx, int B, int HW, int C, float scale, pseg_half_t* y, int ldy,
                     int accumulate, void* stream);
/* NHWC -> NHWC only (the NCHW forms serve the fp32 logits) */
int pseg_bilinear_fwd_h(const pseg_half_t* x, int ldx, int B, int Hi, int Wi, int C, pseg_half_t* y, int ldy, int Ho, int Wo,
                        int align_corners, void* stream);
int pseg_bilinear_bwd_h(const pseg_half_t* dy, int ldy, int B, int Hi, int Wi, int C, pseg_half_t* dx, int ldx, int Ho,
                        int Wo, int align_corners, int accumulate, void* stream);
int pseg_maxpool_fwd_h(const pseg_half_t* x, int ldx, int B, int H, int W, int C, pseg_half_t* y, int ldy, uint8_t* argmax,
                       int Ho, int Wo, int k, int stride, int pad, void* stream);
int pseg_maxpool_bwd_h(const pseg_half_t* dy, int ldy, const uint8_t* argmax, int B, int H, int W, int C, pseg_half_t* dx,
                       int ldx, int Ho, int Wo, int k, int stride, int pad, int accumulate, void* stream);
int pseg_dwconv_fwd_h(const pseg_half_t* x, int ldx, const float* w, pseg_half_t* y, int ldy, int B, int H, int W, int C,
                      int Ho, int Wo, int k, int stride, int pad, void* stream);
int pseg_dwconv_dgrad_h(const pseg_half_t* dy, int ldy, const float* w, pseg_half_t* dx, int ldx, int B, int H, int W, int C,
                        int Ho, int Wo, int k, int stride, int pad, void* stream);
int pseg_dwconv_wgrad_h(const pseg_half_t* x, int ldx, const pseg_half_t* dy, int ldy, float* dw, int B, int H, int W, int C,
                        int Ho, int Wo, int k, int stride, int pad, int accumulate, void* workspace, int64_t workspace_bytes,
                        void* stream);

/* ---- dynamic loss scaling + master-weight optimiser of the `-mp` path (apex O1/O2 semantics: train.py:102-105).
 * `state` = 8 floats on the device: [0] loss scale S, [1] 1/S, [2] clean steps since S last changed, [3] found-inf flag of
 * the step in flight, [4] optimiser steps applied, [5] steps skipped.  Nothing here synchronises the host.
 *   pseg_mp_state_init: S = init_scale, everything else 0.
 *   pseg_mp_check: raises state[3] when any of the n gradient floats is inf / nan (call after the gradient all-reduce, so
 *     every rank decides alike).
 *   pseg_sgd_step_mp / pseg_adam_step_mp: the steps of pseg_sgd_step / pseg_adam_step with grad_scale * (1/S) and -- when
 *     state[3] is raised -- no update at all; first-step / bias-correction counts come from state[4].
 *   pseg_mp_update: after a flagged step S *= backoff_factor (>= min_scale), after growth_interval clean ones S *= growth_factor
 *     (<= max_scale); clears the flag and counts the step as applied or skipped. */
int pseg_mp_state_init(float* state, float init_scale, void* stream);
int pseg_mp_check(const float* grad, int64_t n, float* state, void* stream);
int pseg_mp_update(float* state, float growth_factor, float backoff_factor, int growth_interval, float min_scale,
                   float max_scale, void* stream);
int pseg_sgd_step_mp(float* param, const float* grad, float* momentum_buf, int64_t n, float lr, float momentum,
                     float weight_decay, int nesterov, float grad_scale, const float* state, void* stream);
int pseg_adam_step_mp(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                      float beta2, float eps, float weight_decay, int decoupled, float grad_scale, const float* state,
                      void* stream);

/* depthwise 3x3 (MobileNetV2 encoder of models/unet.py:16-17); w is [kh][kw][C]. */
int pseg_dwconv_fwd(const float* x, int ldx, const float* w, float* y, int ldy, int B, int H, int W, int C,
                    int Ho, int Wo, int k, int stride, int pad, void* stream);
int pseg_dwconv_dgrad(const float* dy, int ldy, const float* w, float* dx, int ldx, int B, int H, int W, int C,
                      int Ho, int Wo, int k, int stride, int pad, void* stream);
int pseg_dwconv_wgrad(const float* x, int ldx, const float* dy, int ldy, float* dw, int B, int H, int W, int C,
                      int Ho, int Wo, int k, int stride, int pad, int accumulate,
                      void* workspace, int64_t workspace_bytes, void* stream);
int64_t pseg_dwconv_wgrad_workspace_bytes(int B, int Ho, int Wo, int C, int k);

/* ------------------------------------------------------------------ BatchNorm (+activation, +residual)
 * Replaces nn.BatchNorm2d + activation inside ConvNormAct (training: batch statistics,
 * biased variance for normalisation, unbiased for running_var, momentum 0.1, eps 1e-5).
 *
 * pseg_col_stats: the same [3][rows][C] shifted statistics for any y[M][C] (when the producer did not
 *   emit them); rows = pseg_col_stats_rows(M, C), group size = pseg_col_stats_group(M, C) (chosen so the
 *   reduction grid fills the chip).  The backward partials of pseg_bn_act_bwd_reduce use the same row count.
 * pseg_bn_finalize: group statistics -> (Chan's parallel merge, in double) mean, invstd,
 *   scale=gamma*invstd, shift=beta; updates running_mean/var in place when non-NULL.
 * pseg_bn_eval_coeffs: the same four vectors from the running statistics (model.eval(), test.py:17).
 * pseg_bn_act_fwd: z = act((y - mean)*scale + shift (+ residual)); the mean is subtracted BEFORE scaling so
 *   channels with |mean| >> std keep full fp32 precision.  mean = scale = shift = NULL: plain act / residual add.
 */
int pseg_col_stats_rows(int64_t M, int C);
int pseg_col_stats_group(int64_t M, int C);
int pseg_col_stats(const float* y, int ldy, int64_t M, int C, float* stat, void* stream);
int pseg_bn_finalize(const float* stat, int rows, int group, int64_t count, int C,
                     const float* gamma, const float* beta, float* running_mean, float* running_var,
                     float momentum, float eps, float* mean, float* invstd, float* scale, float* shift,
                     void* workspace, int64_t workspace_bytes, void* stream);
int64_t pseg_bn_finalize_workspace_bytes(int rows, int C);
int pseg_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean,
                        const float* running_var, float eps, int C, float* mean, float* invstd, float* scale,
                        float* shift, void* stream);
int pseg_bn_act_fwd(const float* y, int ldy, const float* mean, const float* scale, const float* shift,
                    const float* residual, int ldr, int act, float* z, int ldz, int64_t M, int C, float* amax_z,
                    uint32_t* mask_out, void* stream);
/* amax_z (nullable): amax_z[0] = max(amax_z[0], max|z|), see pseg_amax.
 * mask_out (nullable; needs C % 32 == 0 and an activation): the activation bitmask of z, [M][C/32] words, bit c % 32 of
 * word c / 32 set when act'(z) = 1.  For a layer WITH a residual the backward passes cannot recompute the mask from y;
 * given this bitmask (argument `mask` of pseg_bn_act_bwd_reduce / _apply) they read 1 bit per element instead of z. */
/* Small tensors (launch-bound configurations): finalize folded into the apply pass, one launch instead of two, with
 * bit-identical coefficients.  pseg_bn_small_path(rows, M, C) != 0 says when the library recommends them
 * (rows = number of statistic / partial row groups). */
int pseg_bn_small_path(int rows, int64_t M, int C);
int pseg_bn_fwd_fused(const float* stat, int rows, int group, int64_t count, int C, const float* gamma,
                      const float* beta, float* running_mean, float* running_var, float momentum, float eps,
                      float* mean, float* invstd, float* scale, float* shift, const float* y, int ldy,
                      const float* residual, int ldr, int act, float* z, int ldz, int64_t M, float* amax_z,
                      void* stream);
int pseg_bn_bwd_fused(const float* part_db, const float* part_dg, int rows, int64_t count, int C, float* dgamma,
                      float* dbeta, int accumulate, int frozen, const float* dz, int lddz, const float* z, int ldz,
                      const float* y, int ldy, const float* mean, const float* invstd, const float* scale,
                      const float* shift, int act, float* dy, int lddy, float* dres, int lddres,
                      int res_accumulate, int64_t M, void* stream);
/* backward, two passes over (dz, y[, z]).  z may be NULL when there is no residual: the activation argument is then
 * recomputed from y as (y - mean)*scale + shift, bit-identically to the forward pass (one tensor read fewer per pass).
 *  reduce: dyh = dz * act'(z); partials of sum(dyh), sum(dyh * xhat)         [rows][C] each
 *  finalize: dgamma, dbeta (+= when accumulate), c1 = dbeta/M, c2 = dgamma/M; frozen != 0 (eval-mode BatchNorm:
 *            mean / invstd are the running statistics, constants of the graph): c1 = c2 = 0, so apply gives
 *            dy = scale * dyh while dgamma = sum(dyh * xhat), dbeta = sum(dyh) are still produced
 *  apply: dy = scale * (dyh - c1 - xhat*c2); dres (nullable) = dyh (+= when res_accumulate) */
int pseg_bn_act_bwd_reduce(const float* dz, int lddz, const float* z, int ldz, const float* y, int ldy,
                           const float* mean, const float* invstd, const float* scale, const float* shift, int act,
                           int64_t M, int C, float* part_db, float* part_dg, const uint32_t* mask, void* stream);
int pseg_bn_bwd_finalize(const float* part_db, const float* part_dg, int rows, int64_t count, int C,
                         float* dgamma, float* dbeta, int accumulate, int frozen, float* c1, float* c2,
                         void* stream);
int pseg_bn_act_bwd_apply(const float* dz, int lddz, const float* z, int ldz, const float* y, int ldy,
                          const float* mean, const float* invstd, const float* scale, const float* shift,
                          const float* c1, const float* c2, int act, float* dy, int lddy, float* dres, int lddres,
                          int res_accumulate, int64_t M, int C, const uint32_t* mask, uint16_t* dy_hi, uint16_t* dy_lo,
                          int ldp, void* stream);
/* dy_hi / dy_lo (nullable, together; ldp == C, C % 8 == 0): the pass also writes dy as bf16 limb planes (hi = bf16(dy),
 * lo = bf16(dy - hi); exactly what pseg_split_planes(dy) would produce) for pseg_conv2d_dgrad_planes -- the consumer's
 * tiles then go global -> LDS by DMA with no split arithmetic. */
/* eval-mode / frozen-statistics backward and plain activation backward:
 *   dy = scale * dz * act'(z)   (scale NULL -> 1) ; dres as above */
int pseg_act_bwd(const float* dz, int lddz, const float* z, int ldz, const float* scale, int act,
                 float* dy, int lddy, float* dres, int lddres, int res_accumulate, int64_t M, int C,
                 void* stream);
/* column sums of dy[M][C] (bias gradient of the cls_conv, models/deeplabv3plus.py:22) */
int pseg_col_sum(const float* dy, int ldy, int64_t M, int C, float* out, int accumulate,
                 void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ pooling / resize / layout
 * pseg_pool_sum: out[b,c] = scale * sum_p x[b,p,c]   (AdaptiveAvgPool2d(1), models/aspp.py:11,
 *   and the backward of the pooled branch's broadcast)
 * pseg_broadcast: y[b,p,c] = x[b,c] * scale            (bilinear from 1x1, models/aspp.py:16-19; GAP backward)
 * pseg_bilinear_*: F.interpolate(mode='bilinear') NHWC -> NHWC slice
 *   (models/deeplabv3plus.py:34-37,40-43; models/unet.py:30-55; utils/utils.py:18-20)
 *   out_nchw != 0: the output (fwd) / incoming gradient (bwd) is a contiguous NCHW tensor, which is
 *   what the loss and argmax consume.
 */
int pseg_pool_sum(const float* x, int ldx, int B, int HW, int C, float scale, float* out, int ldo, void* stream);
int pseg_broadcast(const float* x, int ldx, int B, int HW, int C, float scale, float* y, int ldy,
                   int accumulate, void* stream);
int pseg_bilinear_fwd(const float* x, int ldx, int B, int Hi, int Wi, int C, float* y, int ldy, int Ho, int Wo,
                      int align_corners, int out_nchw, void* stream);
/* dy_nchw = 1 with scratch of pseg_bilinear_bwd_workspace_bytes(): separable two-pass form (the weights factor into
 * a column pass and a row pass); without scratch (workspace NULL) a single gather pass. */
int64_t pseg_bilinear_bwd_workspace_bytes(int B, int Hi, int Wi, int C, int Ho, int Wo, int dy_nchw);
int pseg_bilinear_bwd(const float* dy, int ldy, int B, int Hi, int Wi, int C, float* dx, int ldx, int Ho, int Wo,
                      int align_corners, int dy_nchw, int accumulate, void* workspace, int64_t workspace_bytes,
                      void* stream);
/* pseg_bn_act_maxpool_fwd: max-pooling of z = act((x - mean) * scale + shift) without z ever existing (the ResNet stem in training:
 * conv -> BatchNorm -> ReLU -> MaxPool(3, 2, 1), torchvision's resnet / the reference's pytorch_modules backbone; mean / scale /
 * shift = rows 0, 2, 3 of pseg_bn_finalize's coefficients).  Same values, same argmax as pseg_bn_act_fwd + pseg_maxpool_fwd. */
int pseg_bn_act_maxpool_fwd(const float* x, int ldx, const float* mean, const float* scale, const float* shift, int act, int B,
                            int H, int W, int C, float* y, int ldy, uint8_t* argmax, int Ho, int Wo, int k, int stride, int pad,
                            void* stream);
int pseg_bn_act_maxpool_fwd_h(const pseg_half_t* x, int ldx, const float* mean, const float* scale, const float* shift, int act,
                              int B, int H, int W, int C, pseg_half_t* y, int ldy, uint8_t* argmax, int Ho, int Wo, int k,
                              int stride, int pad, void* stream);
int pseg_maxpool_fwd(const float* x, int ldx, int B, int H, int W, int C, float* y, int ldy, uint8_t* argmax,
                     int Ho, int Wo, int k, int stride, int pad, void* stream);
int pseg_maxpool_bwd(const float* dy, int ldy, const uint8_t* argmax, int B, int H, int W, int C, float* dx,
                     int ldx, int Ho, int Wo, int k, int stride, int pad, int accumulate, void* stream);
/* NCHW [B][C][HW] -> NHWC [B][HW][ld] (channels >= C zero-filled up to Cpad) and back. */
int pseg_nchw_to_nhwc(const float* x, float* y, int ldy, int B, int C, int HW, int Cpad, void* stream);
int pseg_nhwc_to_nchw(const float* x, int ldx, float* y, int B, int C, int HW, void* stream);
/* fp32 NCHW image (C <= 8) -> fp16 NHWC with 8 channels per pixel (zero-filled): the half-precision policy's network input */
int pseg_nchw_to_nhwc_h(const float* x, pseg_half_t* y, int ldy, int B, int C, int HW, void* stream);
/* strided 2-D copy / add of an [M][C] block (concat-slice plumbing, residual adds) */
int pseg_copy2d(const float* x, int ldx, float* y, int ldy, int64_t M, int C, int accumulate, void* stream);

/* ------------------------------------------------------------------ loss / masks / metrics
 * pseg_ce_fwd_bwd: nn.CrossEntropyLoss() defaults (utils/utils.py:12,21): mean over non-ignored pixels,
 *   ignore_index -100.  ONE pass over the logits writes dlogits = (softmax - onehot)/n_valid and the
 *   loss partials.  loss_out[3]: [0] = mean loss, [1] = n_valid, [2] = n_out_of_range (as floats).  A pixel is valid
 *   iff target != ignore_index and 0 <= target < C -- the same predicate for the divisor, the sum and the gradient.
 *   Targets outside [0, C) other than ignore_index (torch raises IndexError on them) contribute nothing and are
 *   counted in loss_out[2] so the caller can raise without a second pass.  dlogits may be NULL (eval).
 * pseg_scale_inplace: dlogits *= *gscale (device scalar; returns immediately on the device when it is 1).
 * pseg_argmax: outputs.max(1)[1] (test.py:31), first index on ties.
 * pseg_confusion: per-class tp / fn / fp counts (test.py:34-46) accumulated into int64 counters[3][C].
 */
int64_t pseg_ce_workspace_bytes(int64_t npix);
int pseg_ce_fwd_bwd(const float* logits, const int64_t* target, int B, int C, int64_t HW, int64_t ignore_index,
                    float* dlogits, float* loss_out, void* workspace, int64_t workspace_bytes, void* stream);
/* The same loss on bilinearly up-sampled logits WITHOUT the full-resolution tensor (models/deeplabv3plus.py:40-43 +
 * utils/utils.py:18-21): logits_lr is the fp32 NHWC [B,h,w] x ld tensor of class logits (C <= 24 classes in the first
 * channels, ld % 4 == 0), target the [B,H,W] labels; the loss is CE(interpolate(logits, (H, W), 'bilinear', align_corners),
 * target) and dlogits_lr ([B,h,w] x ldd, nullable; ldd >= C, ldd % 4 == 0, 16-byte aligned: it is written 16 bytes at a
 * time) receives its gradient with respect to the LOW-resolution logits (channels [C, ldd) are written as 0, also past the 24
 * the kernels compute in).  loss_out as for pseg_ce_fwd_bwd; with no valid pixel the loss is NaN and the gradient 0.  Deterministic (no floating-point atomics).  pseg_ce_upsampled_ok(...) != 0 says
 * whether the scale factors are covered (about x4 or less per axis); otherwise use pseg_bilinear_fwd + pseg_ce_fwd_bwd +
 * pseg_bilinear_bwd. */
int pseg_ce_upsampled_ok(int h, int w, int C, int H, int W, int align_corners);
int64_t pseg_ce_upsampled_workspace_bytes(int B, int h, int w);
int pseg_ce_upsampled_fwd_bwd(const float* logits_lr, int ld, int B, int h, int w, int C, const int64_t* target, int H,
                              int W, int align_corners, int64_t ignore_index, float* dlogits_lr, int ldd,
                              float* loss_out, void* workspace, int64_t workspace_bytes, void* stream);
/* pseg_lovasz_softmax_fwd_bwd (csrc/lovasz.hip): the multi-class Lovasz-softmax loss of Berman et al. (the reference names
 *   it in utils/criterions.py: lovasz_softmax(probas, labels, classes='present', per_image=False, ignore=...)) and its
 *   gradient with respect to the logits.  logits fp32 NCHW [B][C][HW], target int64 [B][HW].  A pixel is valid iff
 *   target != ignore_index and 0 <= target < C (the predicate of pseg_ce_fwd_bwd); other targets that are not ignore_index
 *   are counted in out[2].  p = softmax(logits) in fp32 with the max subtracted.  For every class c with n_c > 0 valid
 *   pixels of label c ("present"): e_i = |[t_i == c] - p_ic| over all valid pixels, sorted descending, equal errors by
 *   ascending flat pixel index b * HW + y * W + x; with I_k / U_k the intersection / union counts after the first k + 1
 *   elements and J_k = 1 - I_k / U_k, loss_c = sum_k e_(k) * (J_k - J_(k-1)), J_(-1) = 0.  The differences are formed in
 *   closed form from the integer counts (foreground element: 1 / U_k; background: I_k / (U_(k-1) * U_k)), never by
 *   subtracting two values near 1.  out[4]: [0] = mean of loss_c over the present classes (0 when no pixel is valid),
 *   [1] = n_valid, [2] = n_out_of_range, [3] = n_present (as floats).  dlogits ([B][C][HW], nullable, must not alias
 *   logits) receives d out[0] / d logits (zero at invalid pixels); it is also the scratch of the call.  Deterministic: two
 *   calls on the same input give the same bits.  No host synchronisation; absent classes are skipped on the device.
 *   C <= 1024.  logits and target must each be below 2 GiB (B * C * HW * 4 and B * HW * 8 bytes): larger operands are
 *   refused (PSEG_ERR_ARG), not chunked.  workspace: pseg_lovasz_workspace_bytes(B, C, HW) bytes, 16-byte aligned; it
 *   holds the sort buffers of one group of classes (16 bytes per class and pixel, groups sized to stay near 512 MiB), so
 *   it does not grow with C beyond that.  PSEG_LOVASZ_GROUP=n caps the classes per group (same workspace, same result). */
int64_t pseg_lovasz_workspace_bytes(int B, int C, int64_t HW);
int pseg_lovasz_softmax_fwd_bwd(const float* logits, const int64_t* target, int B, int C, int64_t HW, int64_t ignore_index,
                                float* dlogits, float* out, void* workspace, int64_t workspace_bytes, void* stream);
/* pseg_ce_opts_fwd_bwd (csrc/ce_opts.hip): cross-entropy with per-class weights, label smoothing, the focal modulation and
 *   online hard-pixel selection (OHEM), with its gradient.  logits fp32 NCHW [B][C][HW], target int64 [B][HW]; validity is
 *   the predicate of pseg_ce_fwd_bwd, other targets that are not ignore_index are ignored and counted.  With z the logits
 *   of a pixel, t its label, p = softmax(z), w = class_weight (device, [C], non-negative; NULL = all ones),
 *   eps = label_smoothing, gamma = focal_gamma:
 *       l = (1 - eps) w_t (-log p_t) + (eps / C) sum_c w_c (-log p_c)      (F.cross_entropy(weight=, label_smoothing=))
 *       f = (1 - p_t)^gamma l                                               (the gradient flows through the factor)
 *       df/dz_j = m [(1 - eps) w_t (p_j - d_jt) + (eps / C)(p_j sum_c w_c - w_j)] - l gamma (1 - p_t)^(gamma - 1) p_t (d_jt - p_j),
 *   m = (1 - p_t)^gamma; 1 - p_t is formed from the sum of the other classes' exponentials.  Selection: keep_ratio == 1
 *   keeps every valid pixel (no selection runs); otherwise k = clamp(ceil((double)keep_ratio * n_valid), 1, n_valid), tau =
 *   the k-th largest f (the fp32 values the kernel computed, parked at 4 bytes per pixel in the workspace and selected on
 *   the device by a four-round radix select), kept = valid pixels with f >= tau: ties at tau are all kept, n_kept >= k.
 *   loss = sum_kept f / sum_kept w_t; dlogits ([B][C][HW], nullable) receives the gradient of that quotient with the kept
 *   set held fixed, zero on every pixel that is not kept.  A zero divisor (no valid pixel, or every kept weight zero)
 *   gives a NaN loss and an all-zero gradient.  loss_out[6] = [loss, n_valid, n_out_of_range, n_kept, tau (0 when
 *   keep_ratio == 1), sum_kept w_t] (as floats).  Refused with PSEG_ERR_ARG: null logits / target / loss_out / workspace,
 *   non-positive sizes, B * HW >= 2^31, a workspace below pseg_ce_opts_workspace_bytes(B, C, HW) or not 16-byte aligned,
 *   label_smoothing outside [0, 1), keep_ratio outside (0, 1], focal_gamma other than 0 or a value in [1, 8] (for
 *   0 < gamma < 1 the derivative of the factor is unbounded).  Deterministic: floating-point sums go through per-block
 *   partials in a fixed order in double, atomics add integers only; no host synchronisation.  With keep_ratio == 1 the
 *   call is one read of the logits and one write of dlogits after a targets-only pass for the divisor. */
int64_t pseg_ce_opts_workspace_bytes(int B, int C, int64_t HW);
int pseg_ce_opts_fwd_bwd(const float* logits, const int64_t* target, int B, int C, int64_t HW, int64_t ignore_index,
                         const float* class_weight, float label_smoothing, float focal_gamma, float keep_ratio,
                         float* dlogits, float* loss_out, void* workspace, int64_t workspace_bytes, void* stream);
/* pseg_ce_opts_binned_fwd_bwd (csrc/ce_opts.hip): pseg_ce_opts_fwd_bwd with a per-pixel weight taken from a table by a byte
 *   per pixel -- the boundary-weighted cross-entropy when the byte is pseg_label_depth's depth.  pixel_bin uint8 [B][HW]
 *   (device; no alignment beyond one byte is needed), bin_weight 256 fp32 values (device).  PRECONDITION: the 256 values are
 *   finite and non-negative; the call cannot read device memory on the host, so the caller checks them before upload.
 *   The pixel weight is u_i = bin_weight[pixel_bin[i]].  Everything else is pseg_ce_opts_fwd_bwd's contract with, f_i as
 *   defined there, the per-pixel quantity g_i = u_i f_i in f_i's place:
 *       the selection (keep_ratio < 1) parks and ranks g_i; tau = the k-th largest g; kept = valid pixels with g_i >= tau,
 *         ties at tau all kept;
 *       loss = sum_kept g_i / sum_kept (u_i w_{t_i});      dlogits_i = u_i (df_i/dz) / divisor on kept pixels, 0 elsewhere.
 *   A pixel with u_i = 0 is still valid: it is counted in n_valid, may be kept, and contributes 0 to both sums and a zero
 *   gradient.  loss_out[6] has the same layout, [5] = sum_kept u_i w_{t_i}; a zero divisor gives a NaN loss and an all-zero
 *   gradient.  The same arguments are refused, and null pixel_bin / bin_weight; the messages start with
 *   "pseg_ce_opts_binned_fwd_bwd:" and come before any launch.  workspace: pseg_ce_opts_workspace_bytes(B, C, HW), unchanged.
 *   Deterministic under the same rules.  With bin_weight all ones the loss, tau, the counts and every gradient element equal
 *   pseg_ce_opts_fwd_bwd's bit for bit (1.0f * x is exact).  One byte per pixel is read beside the target in every pass
 *   that reads the target; the table lives in LDS; no fp32 weight map exists. */
int pseg_ce_opts_binned_fwd_bwd(const float* logits, const int64_t* target, const uint8_t* pixel_bin,
                                const float* bin_weight, int B, int C, int64_t HW, int64_t ignore_index,
                                const float* class_weight, float label_smoothing, float focal_gamma, float keep_ratio,
                                float* dlogits, float* loss_out, void* workspace, int64_t workspace_bytes, void* stream);
/* pseg_tversky_fwd_bwd (csrc/tversky.hip): the soft region-overlap loss -- soft Dice, Tversky (Salehi et al.) and
 *   focal-Tversky (Abraham & Khan) -- over the softmax of the logits, with its gradient.  logits fp32 NCHW [B][C][HW], target
 *   int64 [B][HW].  A pixel is valid iff target != ignore_index and 0 <= target < C (the predicate of pseg_ce_fwd_bwd);
 *   other targets that are not ignore_index are counted as out of range and ignored.  p = softmax(logits) in fp32 with the
 *   max subtracted.  A group is the whole batch (per_image = 0) or one image (per_image = 1).  For a group and a class c,
 *   over the group's valid pixels:
 *       n_c = #{t_i = c}      S_c = sum_i p_ic      TP_c = sum_{t_i = c} p_ic
 *       FP_c = S_c - TP_c     FN_c = n_c - TP_c
 *       N = TP_c + smooth     D = TP_c + alpha FP_c + beta FN_c + smooth
 *       TI_c = N / D          (TI_c = 1 when D == 0)
 *       term_c = (1 - TI_c)^power
 *   Counted classes of a group: with all_classes = 0 the classes with n_c > 0 ("present"); with all_classes = 1 every
 *   class of a group that has at least one valid pixel.  The group loss is the mean of term_c over the group's counted
 *   classes; the loss is the mean of the group losses over the groups with at least one counted class, and 0 with an
 *   all-zero gradient when there is no such group.  alpha = beta = 0.5, power = 1 is soft Dice; alpha + beta = 1 is
 *   Tversky; power != 1 is focal-Tversky (Abraham & Khan write the exponent as 1 / gamma).
 *   Gradient, the group fixed, with K_c = -power (1 - TI_c)^(power - 1) / (n_counted(group) * n_groups_counted) and
 *   K_c = 0 where 1 - TI_c <= 0 (so power < 1 never produces inf * 0):
 *       g_ic = K_c * ( t_i == c ?  (beta N + alpha FP_c + beta FN_c) / D^2  :  -alpha N / D^2 )    (0 for classes not counted)
 *       dlogits_ij = p_ij * (g_ij - sum_k g_ik p_ik)                                               (0 at invalid pixels)
 *   The target-pixel numerator is D - N (1 - beta) written as a sum of non-negative terms; it is formed that way, never
 *   by subtraction.  In the same spirit the kernels accumulate FP_c directly (the sum of p_ic over the valid pixels with
 *   t_i != c; S_c is that plus TP_c) and form 1 - TI_c as (alpha FP_c + beta FN_c) / D.
 *   out[5] = [loss, n_valid, n_out_of_range, n_terms (counted (group, class) pairs), n_groups_counted] (as floats).
 *   dlogits ([B][C][HW], nullable, must not alias logits) receives d out[0] / d logits.  class_sums (device memory,
 *   nullable): [G][C][3] doubles = n_c, S_c, TP_c, G = per_image ? B : 1.  Work: a reduction pass reads the logits and
 *   the targets once (per-block partials in double, added in a fixed order; no atomics); the coefficients and out[] are
 *   computed in double on the device; only when dlogits != NULL a gradient pass reads the logits and targets again,
 *   recomputes p and writes dlogits once.  No host synchronisation.  Deterministic: two calls on the same input give the
 *   same bits, and the loss is the same bits with and without dlogits.
 *   Refused with PSEG_ERR_ARG before any launch: null logits / target / out / workspace, non-positive sizes, C > 1024,
 *   logits or target at or above 2 GiB (B * C * HW * 4 and B * HW * 8 bytes: refused, not chunked), dlogits aliasing
 *   logits, a workspace below pseg_tversky_workspace_bytes(B, C, HW) (0 for sizes that are refused) or not 16-byte
 *   aligned, alpha < 0, beta < 0, alpha + beta == 0, smooth < 0, power outside [0.5, 4], a non-finite option.
 *   The workspace holds 24 bytes per class and block of 1024 pixels of an image, plus 40 bytes per (group, class). */
int64_t pseg_tversky_workspace_bytes(int B, int C, int64_t HW);
int pseg_tversky_fwd_bwd(const float* logits, const int64_t* target, int B, int C, int64_t HW, int64_t ignore_index,
                         float alpha, float beta, float smooth, float power, int per_image, int all_classes,
                         float* dlogits, float* out, double* class_sums, void* workspace, int64_t workspace_bytes,
                         void* stream);
int pseg_scale_inplace(float* x, int64_t n, const float* gscale, void* stream);
int pseg_argmax(const float* logits, int B, int C, int64_t HW, int64_t* mask, void* stream);
int pseg_confusion(const int64_t* pred, const int64_t* target, int64_t n, int C, int64_t* counters, void* stream);

/* ------------------------------------------------------------------ batched inference (csrc/infer.hip)
 * The host passes of the reference's inference (utils/inference.py:10-22: cv2.resize, /255, softmax, cv2.resize of the
 * probabilities to each photo's size, argmax) on the device, for a ragged batch of photos.  `table` is a device array of
 * B records of three int64 {offset, H, W}: photo (or output image) b is H x W.  Records whose extent leaves the buffer
 * (offset + H*W*elements > capacity, H or W outside [1, 65535]) are skipped on the device -- nothing is read or written
 * for them -- so validate the table on the host.
 *
 * pseg_image_preprocess: src holds B uint8 HWC 3-channel photos back to back (photo b at byte table[b].offset, src_bytes
 *   in all); out is the fp32 NCHW model input [B,3,oh,ow]: out[b,c,y,x] = (v - mean_c) / std_c, v = the photo resampled
 *   with INTER_LINEAR geometry (= F.interpolate bilinear, align_corners=False, no antialias: source coordinate
 *   (d + 0.5) * in/out - 0.5 clamped at 0, upper tap clamped to in - 1) in fp32 and rounded to 8 bits half up,
 *   saturated; correctly rounded fp32 division.  bgr != 0: the photo's channels are B, G, R (cv2.imread) and are swapped
 *   to RGB on load.  A photo already at oh x ow gives exactly CocoDataset.post_fetch_fn's input.
 * pseg_seg_decode: logits fp32 NCHW [B,C,h,w] (what every model returns); for each b, mask[table[b].offset + y*W + x] =
 *   argmax_c bilinear(softmax_c(logits[b]), (H, W), align_corners=False)[c, y, x] as uint8, first index on ties;
 *   npix_total = the mask buffer's size in bytes.  rgb (nullable, 3 * npix_total bytes) receives lut[3*mask .. 3*mask+2]
 *   at 3 * (offset + y*W + x); lut = 256 x 3 bytes, given with rgb.  1 <= C <= 256.  The softmax is evaluated once per
 *   source pixel of a tile (tiles share a one-pixel halo); no full-resolution C-channel tensor exists anywhere.
 */
int pseg_image_preprocess(const uint8_t* src, int64_t src_bytes, const int64_t* table, int B, int bgr, float mean0, float mean1,
                          float mean2, float std0, float std1, float std2, float* out, int oh, int ow, void* stream);
int pseg_seg_decode(const float* logits, int B, int C, int h, int w, const int64_t* table, int64_t npix_total, uint8_t* mask,
                    uint8_t* rgb, const uint8_t* lut, void* stream);

/* ------------------------------------------------------------------ test-time ensembling (csrc/infer.hip)
 * Multi-scale and mirrored prediction, the evaluation protocol DeepLabV3+ and HRNet figures are published with.
 * Scales: for a model input size (h, w) and scales s_1..s_S (1 <= S <= 8) the size at scale s is
 *   (max(32, int(h*s/32)*32), max(32, int(w*s/32)*32)) -- the training loader's multi-scale rule; scales that give the
 *   same size are merged by the host.
 * Views: with flipping each scale has two views, the image and the image mirrored left-right; K = S * (2 or 1).
 * Ensemble, for a photo of H x W:
 *   P = sum over the views of bilinear(unmirror(softmax_c(logits_view)), (H, W), align_corners=False)
 *   mask = argmax_c P, the first index winning ties.
 * The sum is unweighted (the argmax does not see the 1/K).  One map at scale 1 without flipping is pseg_seg_decode's
 * definition.
 *
 * pseg_image_preprocess_views: pseg_image_preprocess with `rows` table records of FOUR int64 {byte offset, H, W, flags};
 *   several records may name the same photo; out is [rows,3,oh,ow].  Flag PSEG_VIEW_MIRROR mirrors the OUTPUT row:
 *   out[r,c,y,x] is the unflagged value at column ow-1-x (the resampled result is mirrored, not the photo), so a
 *   flagged record equals the unflagged one flipped along x bit for bit, and a record with flags 0 equals
 *   pseg_image_preprocess bit for bit.  The table lives on the device, so the host states in `flag_mask` which flag bits
 *   its records use: a flag_mask with unknown bits is refused on the host, and a record with a flag bit outside
 *   flag_mask is skipped on the device like a record that leaves src.
 * pseg_softmax_views: logits fp32 NCHW [n,C,h,w], n = B (pairs = 0) or 2B (pairs = 1: rows B..2B-1 are the logits of the
 *   mirrored inputs of rows 0..B-1).  Writes the probability map [B,h,w,CP] fp32, pixel-major, at prob + prob_offset
 *   (floats; prob 16-byte aligned, prob_offset a multiple of 4, the map inside prob_floats): CP = 8 for C <= 8,
 *   otherwise C rounded up to a multiple of 4 (pseg_seg_decode's padding); lanes C..CP-1 are written as 0.
 *   out[b,y,x,:] = softmax(logits[b,:,y,x]) (+ softmax(logits[B+b,:,y,w-1-x]) with pairs: the mirrored twin is
 *   un-mirrored and added here -- bilinear resizing is linear, so this is the ensemble's sum).  One softmax per source
 *   pixel and view.  1 <= C <= 256.
 * pseg_seg_decode_ensemble: prob is the packed buffer of prob_floats floats holding S maps; maps is a device array of S
 *   records of three int64 {float offset, h_s, w_s}, map s being [B,h_s,w_s,CP] as pseg_softmax_views writes it
 *   (1 <= S <= 8).  table, npix_total, mask, rgb, lut as pseg_seg_decode: for each b,
 *   mask[table[b].offset + y*W + x] = argmax_c sum_s bilinear(map_s[b], (H, W), align_corners=False)[y, x, c], uint8,
 *   first index on ties, fp32 with pseg_seg_decode's tap geometry.  Hmax, Wmax: the largest H and W of the table; they
 *   size the grid.  Skipped on the device, nothing read or written: a table record whose extent leaves the mask buffer or
 *   whose H > Hmax or W > Wmax; and, if ANY map record leaves prob (or has a misaligned offset or a size outside
 *   [1, 65535]), every image -- there is no ensemble without all its maps.  No C-channel tensor at photo size exists.
 */
#define PSEG_VIEW_MIRROR 1
int pseg_image_preprocess_views(const uint8_t* src, int64_t src_bytes, const int64_t* table, int rows, int flag_mask, int bgr,
                                float mean0, float mean1, float mean2, float std0, float std1, float std2, float* out, int oh,
                                int ow, void* stream);
int pseg_softmax_views(const float* logits, int B, int pairs, int C, int h, int w, float* prob, int64_t prob_offset,
                       int64_t prob_floats, void* stream);
int pseg_seg_decode_ensemble(const float* prob, int64_t prob_floats, const int64_t* maps, int S, int B, int C, const int64_t* table,
                             int64_t npix_total, int Hmax, int Wmax, uint8_t* mask, uint8_t* rgb, const uint8_t* lut,
                             void* stream);

/* ------------------------------------------------------------------ sliding-window inference (csrc/infer.hip)
 * A photo larger than the model input is not squeezed into it: the model runs on overlapping windows of its input size
 * laid over the photo at its own (or a scaled) resolution, the class probabilities of the windows covering a pixel are
 * averaged, and the argmax is taken.  Given: the window (h, w) = the model input size, a stride (sy, sx), scales
 * s_1..s_S (1 <= S <= 8) and a photo of H x W.
 * Working image at scale s: (Hs, Ws) = (max(1, int(H*s + 0.5)), max(1, int(W*s + 0.5))); the photo resampled with
 *   pseg_image_preprocess's geometry and 8-bit rounding, exactly as that call gives it at oh = Hs, ow = Ws (at s = 1 the
 *   photo itself, bit for bit: the taps degenerate to weights 1 / 0).
 * Window grid of a working image: ny = ceil(max(Hs - h, 0) / sy) + 1 rows and nx = ceil(max(Ws - w, 0) / sx) + 1 columns;
 *   window (i, j) has its origin at y0 = min(i*sy, max(Hs - h, 0)), x0 = min(j*sx, max(Ws - w, 0)): the last row and
 *   column are shifted back inside the image, not hung over its edge; an image smaller than the window along an axis has
 *   one window along it, whose positions outside the image hold the normalised value 0.0 (the mean colour) and are never
 *   sampled by the decode.  Strides: ceil(h/2) <= sy <= h and ceil(w/2) <= sx <= w, so a pixel is covered by at most
 *   3 windows per axis; the usual choice is (ceil(2h/3), ceil(2w/3)).
 * Working probability: P_s(Y, X, c) = (sum over the windows covering (Y, X), in (i, j) order, of
 *   p_win(Y - y0, X - x0, c)) / n(Y, X), p_win being the window's softmax (with mirroring: plus the un-mirrored softmax of
 *   the mirrored window, what pseg_softmax_views writes with pairs), n the integer number of covering windows; fp32, the
 *   division correctly rounded; the average is unweighted.
 * Mask: mask(y, x) = argmax_c sum_s bilinear(P_s, (H, W), align_corners=False)[y, x, c] with pseg_seg_decode's tap
 *   geometry, the first index winning ties, uint8; colours through the lut as in pseg_seg_decode.
 *
 * pseg_image_preprocess_windows: pseg_image_preprocess_views with `rows` table records of EIGHT int64 {byte offset, H, W,
 *   flags, Hs, Ws, y0, x0}; out is [rows,3,oh,ow] with (oh, ow) the window: out[r,c,y,x] = the normalised working-image
 *   value at (y0 + y, x0 + x), or 0.0f where that position lies outside Hs x Ws; PSEG_VIEW_MIRROR mirrors the output row as
 *   in the views call.  The arithmetic is the views call's, so a record {.., flags, oh, ow, 0, 0} equals its row bit for
 *   bit, and a window equals the crop of the record {.., 0, Hs, Ws, 0, 0} rendered at oh = Hs, ow = Ws bit for bit.
 *   Skipped on the device, nothing read or written: a record whose photo leaves src, whose Hs or Ws is outside
 *   [1, 65535], whose y0 or x0 is negative or >= Hs / Ws, or with a flag bit outside flag_mask.
 * pseg_seg_decode_windows: groups is a device array of S * B records of three int64 {float offset, Hs, Ws}, scale-major
 *   (record s * B + b: the windows of photo b at scale s), a group being [ny*nx, h, w, CP] as pseg_softmax_views writes
 *   it, window (i, j) at index i*nx + j; ny and nx follow from the grid rule.  table, npix_total, Hmax, Wmax, mask, rgb
 *   and lut are pseg_seg_decode_ensemble's.  Skipped on the device, nothing written: a photo whose table record leaves
 *   the mask buffer or exceeds Hmax / Wmax, and a photo ANY of whose S group records leaves prob, has an offset that is
 *   not a multiple of 4 or a size outside [1, 65535] (other photos are not affected).  PSEG_ERR_ARG: null pointers, S
 *   outside [1, 8], C outside [1, 256], strides outside the limits above, non-positive sizes.  A gather by output tile:
 *   per photo pixel and scale the covering windows' vectors are summed and divided per bilinear tap, the taps blended
 *   and the scales accumulated in registers; no atomics, no C-channel tensor at working or photo size, deterministic.
 */
int pseg_image_preprocess_windows(const uint8_t* src, int64_t src_bytes, const int64_t* table, int rows, int flag_mask, int bgr,
                                  float mean0, float mean1, float mean2, float std0, float std1, float std2, float* out, int oh,
                                  int ow, void* stream);
int pseg_seg_decode_windows(const float* prob, int64_t prob_floats, const int64_t* groups, int S, int B, int C, int h, int w, int sy,
                            int sx, const int64_t* table, int64_t npix_total, int Hmax, int Wmax, uint8_t* mask, uint8_t* rgb,
                            const uint8_t* lut, void* stream);

/* ------------------------------------------------------------------ connected regions of the masks (csrc/regions.hip)
 * The step after the argmax: label the connected regions of each mask, describe them, and clean the mask.  mask, table,
 * npix_total, Hmax and Wmax are pseg_seg_decode_ensemble's: a packed buffer of npix_total uint8 pixels under a device table
 * of B records {pixel offset, H, W}.  A record whose extent leaves the buffer, or whose H > Hmax or W > Wmax, is skipped on
 * the device: nothing is read or written for it.  Hmax * Wmax < 2^31 (labels are int32), otherwise PSEG_ERR_ARG.  A
 * component is a maximal connected set of pixels of one class value; every value 0..255 is a class, background included.
 * Integer arithmetic only (integer atomics, no floating point anywhere), a fixed number of launches, no host
 * synchronisation.  These entry points are additive: PSEG_ABI_VERSION does not move.
 *
 * pseg_regions_workspace_bytes(npix_total, max_regions): bytes of the 16-byte aligned workspace the three calls below take
 *   (-1 for arguments out of range).  It holds one int32 and one byte per pixel, the scan's block sums and the
 *   (photo, class) table of largest_only for min(npix_total, PSEG_REGIONS_MAX_LARGEST_BATCH) photos; records are the
 *   caller's buffer, so max_regions does not add to it.
 * pseg_mask_label: connectivity 4 or 8.  labels (int32, npix_total words, at the mask's packed offsets):
 *   labels[offset + y*W + x] = y0*W + x0 of the first pixel, in raster order, of that pixel's component -- the canonical
 *   labelling, equal element for element to any correct one.  Three launches: a union-find over PSEG_REGIONS_TILE x
 *   PSEG_REGIONS_TILE tiles (origin at the photo's corner) in LDS, the union of the pixel pairs across tile borders in
 *   global memory (atomicMin toward the smaller index, retried), and a pass that points every pixel at its root.  The
 *   workspace is not used by this call (ws may be null).
 * pseg_mask_regions: one record of PSEG_REGION_WORDS int64 per component, in the order (photo, label) -- the exclusive scan
 *   of the root flags labels[p] == p along the packed buffer (so table offsets must ascend with the photo index for the
 *   order to be by photo).  Words: [0] photo * 256 + class, [1] label, [2] area, [3] x0, [4] y0, [5] x1, [6] y1 (the
 *   bounding box, inclusive), [7] Sx, [8] Sy, [9] Sxx, [10] Sxy, [11] Syy = sums over the component's pixels of x, y, x*x,
 *   x*y, y*y with x, y measured from the PHOTO's corner (pixel (0, 0) contributes nothing).  Bound: with H * W < 2^31 and
 *   H, W <= 65535, Sxx <= H * (W-1)W(2W-1)/6 < (H*W) * W^2 / 3 < 2^31 * 2^32 / 3 < 2^62, likewise Syy, and
 *   Sxy <= (H(H-1)/2) * (W(W-1)/2) < (H*W)^2 / 4 < 2^60: every sum stays inside int64.  count[0] (int64) receives the
 *   full number of components; only records 0 .. min(count, max_regions) - 1 are written.  npix_total < 2^31.
 * pseg_mask_clean: a component is SMALL if its area < min_area; with largest_only != 0 a component of class >= 1 is also
 *   small unless it is the largest component of its class in its photo (equal areas: the smaller label wins; then
 *   B <= PSEG_REGIONS_MAX_LARGEST_BATCH).  Every pixel of a small component takes the class found by this walk: from the
 *   component's first pixel step to the pixel above it, or, in the top row, to the pixel left of it; if that pixel's
 *   component is small too, go on from ITS first pixel; a component whose first pixel is the photo's corner keeps its
 *   class.  Labels strictly decrease along the walk; it is one serial walk per component.  mask_out may equal mask.  rgb
 *   (nullable, 3 * npix_total bytes) receives lut[3*c .. 3*c+2] of the cleaned class c, as pseg_seg_decode's.  min_area <= 1
 *   without largest_only copies the mask (and colours it).  labels must be pseg_mask_label's result for mask.
 */
#define PSEG_REGIONS_TILE 32
#define PSEG_REGION_WORDS 12
#define PSEG_REGIONS_MAX_LARGEST_BATCH 4096
int64_t pseg_regions_workspace_bytes(int64_t npix_total, int64_t max_regions);
int pseg_mask_label(const uint8_t* mask, const int64_t* table, int B, int64_t npix_total, int Hmax, int Wmax, int connectivity,
                    int* labels, void* ws, int64_t ws_bytes, void* stream);
int pseg_mask_regions(const uint8_t* mask, const int* labels, const int64_t* table, int B, int64_t npix_total, int Hmax, int Wmax,
                      int64_t max_regions, int64_t* records, int64_t* count, void* ws, int64_t ws_bytes, void* stream);
int pseg_mask_clean(const uint8_t* mask, const int* labels, const int64_t* table, int B, int64_t npix_total, int Hmax, int Wmax,
                    int64_t min_area, int largest_only, uint8_t* mask_out, uint8_t* rgb, const uint8_t* lut, void* ws,
                    int64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ outlines of the regions (csrc/polygons.hip)
 * The boundary of every connected region as closed rings of lattice vertices.  mask, labels, table, npix_total, Hmax, Wmax
 * are the regions section's; labels must be pseg_mask_label's result for mask with the SAME connectivity.  Integer
 * arithmetic only, so results are exact and bit-reproducible.  These entry points are additive: PSEG_ABI_VERSION does not move.
 *
 * Lattice.  Pixel (x, y) of a photo is the unit square [x, x+1] x [y, y+1]; vertices are the integer points 0..W x 0..H.
 *   (The records' pixel-centre coordinates are these minus 0.5.)
 * Cracks.  Side s of pixel p is a directed unit edge with the pixel on its right hand:
 *     s = 0  N  east   (x, y)     -> (x+1, y)          s = 2  S  west   (x+1, y+1) -> (x, y+1)
 *     s = 1  E  south  (x+1, y)   -> (x+1, y+1)        s = 3  W  north  (x, y+1)   -> (x, y)
 *   The edge exists iff the pixel across that side lies outside the photo or has another LABEL.  Edge id = 4 * (pixel
 *   index) + s: photo-relative (pixel index y*W + x) in the records, packed-buffer-relative (offset + y*W + x) for ordering.
 * Successor.  At the head of edge (p, s) let a be the pixel ahead of p in the travel direction, b the pixel ahead-left
 *   (diagonal to p), and in(q) mean: q is inside the photo and labels[q] == labels[p].  Then the successor is
 *     in(a) and in(b):   turn left,  (b, (s+3)%4)
 *     in(a), not in(b):  straight,   (a, s)
 *     neither:           turn right, (p, (s+1)%4)
 *     in(b), not in(a) -- a saddle:  connectivity 8 turns left, (b, (s+3)%4); connectivity 4 turns right, (p, (s+1)%4).
 *   Every edge has exactly one successor and one predecessor, so the edges fall into closed RINGS.  With connectivity 8 a
 *   component has one outer ring, which may pass a vertex twice, and its holes are the 4-connected pieces of its
 *   complement; with connectivity 4 all rings are simple and the holes are the 8-connected pieces of the complement.
 * Corner edge: an edge whose predecessor has a different s.  A ring's VERTICES are the tails of its corner edges, in ring
 *   order, beginning at the corner edge of smallest id, the ring's START EDGE.  A ring has at least 4 vertices, an even
 *   count, and horizontal and vertical segments alternate.
 * Outer ring and holes.  The outer ring of a component is the one whose start edge is 4 * label + 0; every other ring of
 *   that label is a hole.  With y down the shoelace sum sum(x_i * y_{i+1} - x_{i+1} * y_i) is positive for outer rings and
 *   negative for holes, and the signed areas of a component's rings add up to its pixel area exactly.
 * Output order: rings ascend by the packed id of their start edge -- photo first (table offsets ascending), then raster.
 *
 * pseg_mask_rings_workspace_bytes(npix_total, max_edges): bytes of the 16-byte aligned workspace (5 bytes per pixel and 37
 *   per edge of capacity, plus the scans' block sums); -1 for arguments out of range.
 * pseg_mask_rings: npix_total < 2^29 (edge ids and indices are int32), 0 <= max_edges <= 4 * npix_total, connectivity 4 or
 *   8; otherwise PSEG_ERR_ARG.  rings: max_edges / 4 records of PSEG_RING_WORDS int64: [0] photo * 256 + class, [1] label,
 *   [2] start edge id (photo-relative), [3] offset of the first vertex, [4] vertex count, [5] 1 for a hole, 0 for an outer
 *   ring.  vertices: max_edges (x, y) int32 pairs; each ring's vertices are contiguous, in ring order.  counts[0..2]
 *   (int64): the full numbers of edges, rings and vertices.  If counts[0] > max_edges the call sets counts[1] = counts[2] =
 *   -1 and writes nothing into rings or vertices (both may be null with max_edges 0): repeat it with max_edges = counts[0].
 *   Words of rings and vertices past the counts are left as they are.  Skipped table records (regions section) are
 *   skipped here too: nothing is read or written for them.  No host synchronisation; the number of launches, 11 + 2 R with
 *   R = ceil(log2(min(max_edges, 4 * Hmax * Wmax))), depends on max_edges, Hmax and Wmax only: cracks per pixel, an
 *   exclusive scan, the compact edge list with successors, R rounds of pointer doubling (minimum over corner-edge ids,
 *   between two buffers) for the start edges, R rounds of list ranking of the rings opened at their start edges, a scan
 *   of ring flags and vertex counts, the scatter.  No thread walks along a ring.
 * Not here: polygon simplification, a device-side convex hull or minimum-area rectangle (utils/regions.py does the
 * rectangle on the host from the ring's vertices), run-length export.
 */
#define PSEG_RING_WORDS 6
int64_t pseg_mask_rings_workspace_bytes(int64_t npix_total, int64_t max_edges);
int pseg_mask_rings(const uint8_t* mask, const int* labels, const int64_t* table, int B, int64_t npix_total, int Hmax, int Wmax,
                    int connectivity, int64_t max_edges, int64_t* rings, int32_t* vertices, int64_t* counts, void* ws,
                    int64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ local dense-CRF refinement of logits (csrc/crf.hip)
 * Mean-field inference of the locally connected dense CRF of Teichmann & Cipolla, "Convolutional CRFs for Semantic
 * Segmentation" (2018): the Kraehenbuehl-Koltun appearance and smoothness kernels truncated to a dilated (2R+1) x (2R+1)
 * window.  Logits in, logits out, on the model-input grid; the guide is the model input.  These entry points are additive:
 * PSEG_ABI_VERSION does not move.
 *
 * Given logits U fp32 NCHW [B,C,h,w], a guide G fp32 NCHW [B,3,h,w], guide scales g_c (the preprocess call's std_c: then
 * (G_c(p) - G_c(q)) * g_c is the colour difference in 8-bit units whatever the normalisation), radius R in 1..5, dilation
 * D in 1..4, iterations T in 1..10, theta_alpha, theta_beta, theta_gamma > 0 and weights w_a, w_s >= 0.
 * Neighbours.  N(p) = the pixels q = p + D * (dy, dx) with |dy|, |dx| <= R, q != p, inside the image.
 * Kernels.    k_a(p,q) = exp(-|p-q|^2 / (2 theta_alpha^2) - sum_c ((G_c(p) - G_c(q)) g_c)^2 / (2 theta_beta^2))
 *             k_s(p,q) = exp(-|p-q|^2 / (2 theta_gamma^2))
 * Iteration.  Q^0 = softmax_c(U); for t = 1..T
 *             m_c(p)   = w_a * (sum_{q in N(p)} k_a Q^{t-1}_c(q)) / (sum_{q in N(p)} k_a)
 *                      + w_s * (sum_{q in N(p)} k_s Q^{t-1}_c(q)) / (sum_{q in N(p)} k_s)
 *             L^t_c(p) = U_c(p) + m_c(p)       (Potts compatibility; the class-independent term drops out of the softmax)
 *             Q^t      = softmax_c(L^t)
 * Result.     out = L^T, fp32 NCHW [B,C,h,w]: its softmax is the refined distribution, so every consumer of logits works
 *             on it as it stands.
 * Each kernel's message is normalised by its own weight sum over the in-image neighbours: a border pixel is not starved,
 * and w_a, w_s are in logit units independent of R and D.  Only the RATIOS k / sum k enter, so the implementation takes
 * each kernel's weights relative to the pixel's largest one, exp(e(q) - max_q e(q)): the same ratios, and a pixel whose
 * every neighbour is far in colour (exp underflows in fp32) still gets a finite message.  A pixel with no in-image
 * neighbour at all (possible only where D reaches the image's size, e.g. 2 x 2 at D = 2) gets no message: L = U there.
 * With w_a = w_s = 0 the output equals U bit for bit (a copy; nothing is launched).  All arithmetic is fp32, there are no
 * atomics, and two calls on the same input give the same bits.  The order of the sum over the window is row-major, so the
 * result of a mirrored input is the mirrored result up to rounding, not bit for bit.
 *
 * pseg_crf_workspace_bytes(B, C, h, w): bytes of the 16-byte aligned workspace -- two ping-pong buffers of Q, pixel-major
 *   [B,h,w,CP] in pseg_softmax_views' layout (CP = 8 for C <= 8, else C rounded up to 4), and nothing else; -1 for sizes
 *   outside the ranges below.
 * pseg_crf_refine: B, h, w in [1, 65535], h * w > 1, C in [1, 256], R, D, T in their ranges, thetas finite and > 0 with
 *   1 / (2 theta^2) finite, weights and guide scales finite and >= 0, every operand (logits, guide, one Q buffer) below
 *   2 GiB -- refused, not chunked --, workspace 16-byte aligned and at least the query's size; otherwise PSEG_ERR_ARG before
 *   any launch.  out may be logits itself; it must not overlap the workspace and must not be the guide.  Launches: one
 *   forms Q^0 (pseg_softmax_views' kernel), then one per iteration; the last iteration writes NCHW L^T itself.  The pair
 *   weights never reach global memory: an iteration recomputes them from a guide tile with its R * D halo in LDS and reads
 *   the neighbours' class vectors from an LDS tile of Q with the same halo, a class chunk at a time.
 * Not here: a learned compatibility matrix, the full-image (permutohedral) CRF, a backward pass, fp16 Q.
 */
int64_t pseg_crf_workspace_bytes(int B, int C, int h, int w);
int pseg_crf_refine(const float* logits, const float* guide, int B, int C, int h, int w, float g0, float g1, float g2, int R, int D,
                    int T, float theta_alpha, float theta_beta, float theta_gamma, float w_a, float w_s, float* out, void* workspace,
                    int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ contour measures of the evaluation (csrc/boundary.hip)
 * Boundary IoU (Cheng et al., CVPR 2021) and the trimap IoU of the DeepLabV3+ paper both come from one quantity per pixel
 * that does not depend on the class count.  These entry points are additive: PSEG_ABI_VERSION does not move.
 *
 * Label depth.  L is a label map of H x W (int64), C the class count, d the width, 1 <= d <= 254.  A label outside [0, C) is
 * VOID.  Two pixels carry a DIFFERENT LABEL when their values differ -- void included: void values are compared by value
 * like any other, so two different void values next to each other are a label change.
 *   depth(p)      = the smallest k >= 1 such that a pixel q INSIDE the image with max(|dx|, |dy|) = k has L(q) != L(p),
 *                   clipped to d + 1 when there is none within d;
 *   depth_edge(p) = min(depth(p), x + 1, W - x, y + 1, H - y): the outside of the image counts as a different label, the
 *                   nearest outside pixel of column 0 being at distance 1.
 * Pixels of another image of the batch never count.  For every class c, with M = (L == c), M & (depth_edge <= d) equals
 * M & ~erode^d(M), erode being the 3 x 3 erosion of the zero-padded mask: the boundary region of the published Boundary IoU
 * code (cv2.copyMakeBorder(..., 0), cv2.erode(ones(3, 3), iterations = d), crop, subtract).  One depth map serves all classes.
 * The depth is separable: with c(q) the distance along q's column to the nearest different label, clipped to d + 1,
 *   depth(p) = min(c(p), min over the pixels q of p's row at offset k, 1 <= |k| <= d, of (L(q) != L(p) ? |k| : max(|k|, c(q)))),
 * which is how the kernels compute it: O(d) work per pixel, no pass per class.
 *
 * pseg_label_depth: labels int64 [B][H][W] -> depth uint8 [B][H][W], the clipped depth (1 .. d + 1) of every pixel, void
 *   pixels included; edge != 0: depth_edge instead.  No workspace: the column distances are staged in `depth` itself.
 *
 * Counters.  counters is int64 [6][C], ACCUMULATED into like pseg_confusion's.  T is the target; P' is the prediction with
 * every pixel whose target is void set to the void value -1 (a pixel nobody labelled can be neither right nor wrong, and must
 * not create a contour in the prediction either).  Depths of T and of P' are taken separately.
 *   row 0      inter[c] = #{T = c, P' = c, depth_edge_T <= d, depth_edge_P' <= d}
 *   row 1      gband[c] = #{T = c, depth_edge_T <= d}
 *   row 2      pband[c] = #{P' = c, depth_edge_P' <= d}
 *   row 3/4/5  trimap tp / fn / fp = pseg_confusion's three counts (same rules, prediction values outside [0, C) included)
 *              over the pixels with a valid target and depth_T <= d -- WITHOUT the edge term: the image border is not an
 *              object contour.
 * Boundary IoU of class c = inter / (gband + pband - inter), trimap IoU = tp / (tp + fn + fp); a denominator <= 0 is
 * replaced by 1 (utils.compute_boundary_metrics, as compute_metrics does).
 * pseg_boundary_counts_workspace_bytes(B, H, W, d): bytes of the workspace (one byte per pixel and map, each plane rounded up
 *   to 16 bytes; nothing depends on C); -1 for arguments out of range.
 * pseg_boundary_counts: pred, target int64 [B][H][W].  Two launches, integer atomics only, no host synchronisation.
 *
 * Both calls: B, H, W >= 1, H, W <= 2^30, B * H * W <= 2^40, 1 <= C <= 1024 (pseg_confusion's bound), 1 <= d <= 254;
 * otherwise PSEG_ERR_ARG with a message that names the argument, before anything is launched. */
int pseg_label_depth(const int64_t* labels, int B, int H, int W, int C, int d, int edge, uint8_t* depth, void* stream);
int64_t pseg_boundary_counts_workspace_bytes(int B, int H, int W, int d);
int pseg_boundary_counts(const int64_t* pred, const int64_t* target, int B, int H, int W, int C, int d, int64_t* counters,
                         void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ surface (boundary-distance) loss (csrc/surface.hip)
 * Kervadec et al., "Boundary loss for highly unbalanced segmentation" (MIDL 2019): the softmax weighted by a signed distance
 * to the target's contour, per class.  The distance map is an exact Euclidean distance transform and a public call of its
 * own.  These entry points are additive: PSEG_ABI_VERSION does not move.
 *
 * pseg_class_sdist: labels int64 [B][H][W] -> sdist int32 [B][C][H][W], the signed SQUARED Euclidean distance to the contour
 *   of every class.  For image b and class c in [0, C) let M = {q in image b : L(q) == c}.  A label outside [0, C)
 *   (ignore_index, 255, anything else) belongs to no class: it is outside M for every c (void labels compare by value, as
 *   in the label depth).  Pixels of another image never count, and the image border is not a contour.
 *       M empty or M the whole image:   sdist = 0 everywhere (the class has no contour in this image)
 *       p not in M:                     sdist(p) = +min over q in M     of |p - q|^2      (>= 1)
 *       p in M:                         sdist(p) = -min over q not in M of |p - q|^2      (<= -1)
 *   Integers, exact; 0 is the "no term" sentinel and occurs in no other way.  Two calls on the same input give the same bits.
 *   The distance is separable: with s(x, y) the signed distance along column x to the nearest pixel of the other kind
 *   (negative in M; "none" when the column has no such pixel),
 *       |sdist(x, y)| = min over x' of (x - x')^2 + f(x'),    f(x') = 0 where (x', y) is of the other kind, else s(x', y)^2,
 *   which is how the kernels compute it: a memset and a pass that packs the labels to 16 bits and counts every class per
 *   image (integer atomics: order-independent), a column sweep that stages s in sdist itself, and a row pass with the row
 *   of s in LDS that searches outwards from x and stops once (x - x')^2 reaches the best value so far.  Integer arithmetic
 *   only; no host synchronisation.
 *   Refused with PSEG_ERR_ARG before any launch: null labels / sdist / workspace, B, H or W below 1, H or W above 16384 (so
 *   H^2 + W^2 <= 2^29 fits), C outside [1, 1024], B * C * H * W * 4 at or above 2 GiB (refused, not chunked), a workspace
 *   below pseg_class_sdist_workspace_bytes(B, C, H, W) (0 for sizes that are refused) or not 16-byte aligned.
 *   The workspace holds 4 bytes per (image, class) and 2 bytes per pixel.
 *
 * pseg_surface_fwd_bwd: logits fp32 NCHW [B][C][HW], target int64 [B][HW], sdist int32 [B][C][HW] (pseg_class_sdist of the
 *   target).  phi = sqrt(sdist) where sdist > 0, -(sqrt(-sdist) - 1) where sdist < 0, 0 where sdist == 0 (Kervadec's
 *   one_hot2dist: edt(neg) neg - (edt(pos) - 1) pos, and a zero map for a class without a contour); with clip > 0, phi is
 *   limited to [-clip, clip]; clip == 0: no limit.  A pixel is valid iff target != ignore_index and 0 <= target < C; other
 *   targets that are not ignore_index are counted as out of range and ignored.  p = softmax(logits), max subtracted.
 *       loss       = (1 / n_valid) sum over valid i, over c of phi_ic p_ic          (0 with a zero gradient when n_valid == 0)
 *       dlogits_ij = p_ij (phi_ij - sum_k phi_ik p_ik) / n_valid                     (0 at invalid pixels)
 *       out[3]     = [loss, n_valid, n_out_of_range] (as floats)
 *   The sum runs over ALL classes and the divisor is the number of valid pixels only.  dlogits ([B][C][HW], nullable) must
 *   alias neither logits nor sdist.  Work: a reduction pass reads logits, sdist and targets once (per-block partials in
 *   double, added in a fixed order; no atomics); one block forms out[]; only when dlogits != NULL a gradient pass reads
 *   logits and sdist twice more and writes dlogits once.  No host synchronisation.  Deterministic: two calls give the same
 *   bits, and the loss is the same bits with and without dlogits.
 *   Refused with PSEG_ERR_ARG before any launch: null logits / target / sdist / out / workspace, non-positive sizes,
 *   C > 1024, logits or target at or above 2 GiB, a negative or non-finite clip, an aliasing dlogits, a workspace below
 *   pseg_surface_workspace_bytes(B, C, HW) (0 for sizes that are refused) or not 16-byte aligned.
 *   The workspace holds 24 bytes per block of 1024 pixels of an image. */
int64_t pseg_class_sdist_workspace_bytes(int B, int C, int H, int W);
int pseg_class_sdist(const int64_t* labels, int B, int H, int W, int C, int32_t* sdist, void* workspace,
                     int64_t workspace_bytes, void* stream);
int64_t pseg_surface_workspace_bytes(int B, int C, int64_t HW);
int pseg_surface_fwd_bwd(const float* logits, const int64_t* target, const int32_t* sdist, int B, int C, int64_t HW,
                         int64_t ignore_index, float clip, float* dlogits, float* out, void* workspace,
                         int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ surface-distance evaluation (csrc/hausdorff.hip)
 * The record behind the Hausdorff distance (HD), its percentile (HD95), the average symmetric surface distance (ASSD) and the
 * surface Dice at a tolerance (NSD), per image and class, from two label maps.  These entry points are additive:
 * PSEG_ABI_VERSION does not move.
 *
 * pred, target: int64 [B][H][W]; C classes.
 * Void.  A pixel whose target is outside [0, C) is void, and its prediction counts as void too (the rule of
 *   pseg_boundary_counts); a prediction outside [0, C) is void.  A void pixel is in no class mask.
 * Masks and border.  For image b and class c, P = (pred == c, not void) and G = (target == c).  The border dM of a mask M is the
 *   set of its pixels with at least one of the four edge neighbours not in M; a neighbour outside the image counts as not in M
 *   (M & ~binary_erosion(M, cross) with a zero border: the edge rule of medpy and MONAI; unlike pseg_class_sdist, the image
 *   border is a contour).
 * Directed distance sets.  D(P->G) holds, for every p in dP, min over q in dG of |p - q|^2: an exact integer, in pixels
 *   squared, no spacing.  D(G->P) is the same the other way round.
 * Record.  stats int64 [B][C][8], sums double [B][C][2]:
 *   stats[0], [1]   n_p = |dP|, n_g = |dG|
 *   stats[2], [3]   the maximum of D(P->G), of D(G->P)
 *   stats[4], [5]   the nearest-rank quantile of each: its k-th smallest element, k = (n * permille + 999) / 1000 in integer
 *                   division (permille = 1000: the maximum)
 *   stats[6], [7]   the number of elements <= tol * tol in each
 *   sums[0], [1]    the sum of sqrt(d2) over each multiset, in double
 *   If n_p == 0 or n_g == 0 the distances are undefined: stats[2..5] = -1, stats[6], [7] = 0 and both sums are 0.
 *   permille: an int in [1, 1000]; tol: an int in [0, 255] pixels.
 *   From the record (utils.compute_surface_metrics): HD = sqrt(max(stats[2], stats[3])), HD95 = sqrt(max(stats[4], stats[5])),
 *   ASSD = (sums[0] / n_p + sums[1] / n_g) / 2 where n_p > 0 and n_g > 0; NSD = (stats[6] + stats[7]) / (n_p + n_g) where
 *   n_p + n_g > 0.
 * The integer fields are exact.  The sums are added from per-block double partials in a fixed order, without floating-point
 * atomics (integer atomics only): two calls on the same input give the same bits.  No host synchronisation.
 * How: the border pixels of both maps are marked and counted per (image, class); only a class with a border in both maps of an
 * image gets any further work.  For those, a column sweep leaves the distance along the column to the nearest border pixel, and
 * a row pass (Meijster's lower-envelope scan: work bounded by the row's length whatever the distances are, a lane per row, the
 * stack inside the row's own LDS words) gives the squared distance, kept only at the other map's border pixels.  The quantile is
 * a four-round segmented radix select over all (image, class, direction) segments at once.
 *
 * pseg_hausdorff_workspace_bytes(B, C, H, W): bytes of the workspace; 0 for sizes that are refused.  It holds 4 C bytes per pixel
 *   (an int16 plane per class and map), 12 bytes per pixel, about 2 KiB per (image, class) and 8 bytes per block of the row pass.
 * pseg_hausdorff_stats: refused with PSEG_ERR_ARG before any launch, with a message that starts "pseg_hausdorff_stats:": B, H
 *   or W below 1, H or W above 16384 (so H^2 + W^2 <= 2^29 fits), C outside [1, 1024], a workspace buffer at or above 2 GiB
 *   (B * C * H * W * 4 or B * C * 2048 at or above 2 GiB: refused, not chunked), permille outside [1, 1000], tol outside [0, 255],
 *   null pred / target / stats / sums / workspace, a workspace below pseg_hausdorff_workspace_bytes(B, C, H, W) or not 16-byte
 *   aligned.  Nothing outside the buffers named by the arguments is touched. */
int64_t pseg_hausdorff_workspace_bytes(int B, int C, int H, int W);
int pseg_hausdorff_stats(const int64_t* pred, const int64_t* target, int B, int H, int W, int C, int permille, int tol,
                         int64_t* stats, double* sums, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ training augmentation (csrc/augment.hip)
 * The geometric and colour-affine part of the reference's online augmentation (utils/datasets.py:26-125, imgaug on the
 * host) fused with CocoDataset.post_fetch_fn (utils/datasets.py:199-213) into one launch over the collated uint8 batch.
 * img uint8 [B,3,H,W] planar RGB, seg uint8 [B,H,W]; out fp32 [B,3,oh,ow], target int64 [B,H,W] (targets keep the input
 * size: the loss resizes the logits).  params: fp32 [B][PSEG_AUGMENT_ROW], one row per sample:
 *   [0..5]   inverse affine a00 a01 a02 a10 a11 a12: output pixel index (x, y) of the H x W working grid reads source index
 *            coordinates sx = a00*x + a01*y + a02, sy = a10*x + a11*y + a12 (pixel centres at integers, fp32 fma).  The
 *            host folds flips, crop-and-pad, scale, rotate, shear, translate and every centre offset into it.
 *   [6..17]  colour matrix M, 3 x 4 row-major, in 0..255 units: output channel c = M[c] . [r, g, b, 1].
 *   [18]     cval, the image fill value (0..255 units)
 *   [19]     image interpolation order: 0 nearest, otherwise bilinear
 *   [20]     border mode: 0 constant (a tap outside the image contributes cval), otherwise edge (tap indices are clamped)
 *   [21..23] reserved, ignored
 * Image, per output pixel (oy, ox): working-grid index ix = min((int)floorf(ox * ((float)W / ow)), W - 1), iy likewise
 * (ATen's nearest: the identity when (oh, ow) == (H, W)); (sx, sy) from the affine; nearest takes floorf(s + 0.5f),
 * bilinear the taps floorf(s) and + 1; the sample is rounded to 8 bits half up and saturated, the colour matrix is applied
 * in fp32 and rounded the same way, then (q - mean_c) / std_c with a correctly rounded division.  Labels, per pixel of
 * [H, W]: the same affine, nearest sample, 0 outside the image, widened to int64 (colour, cval and border mode do not apply).
 * Coordinates are clamped to [-1, size] before they become integers, which changes no result; a NaN / infinite coordinate
 * counts as outside in either border mode (cval / label 0).  Nothing outside img and seg is read, whatever the table holds.
 * Identity rows give exactly post_fetch_fn's tensors (including its multi-scale nearest resize). */
#define PSEG_AUGMENT_ROW 24
int pseg_augment_batch(const uint8_t* img, const uint8_t* seg, const float* params, int B, int H, int W, float mean0, float mean1,
                       float mean2, float std0, float std1, float std2, float* out, int oh, int ow, int64_t* target,
                       void* stream);

/* pseg_augment_batch_nbhd: pseg_augment_batch with a neighbourhood stage and two per-pixel random stages (the reference's
 * GaussianBlur / AverageBlur / Sharpen / Emboss, AdditiveGaussianNoise, Dropout / CoarseDropout).  Arguments, labels, the
 * multi-scale index and the read / write footprint are pseg_augment_batch's.  params: fp32 [B][PSEG_AUGMENT_NBHD_ROW]:
 *   [0..23]    pseg_augment_batch's row, verbatim
 *   [24]       K, the filter size: 0 or 1 = no filter, otherwise odd, at most PSEG_AUGMENT_NBHD_KMAX
 *   [25]       noise scale in 0..255 units (<= 0: no noise)       [26] != 0: one normal per plane, otherwise one per pixel
 *   [27]       dropout probability p as fp32 (<= 0: no dropout)   [28] != 0: one draw per plane, otherwise one per pixel
 *   [29] [30]  mh, mw: the coarse dropout mask's size; 0 0 = one draw per working-grid pixel
 *   [31] [32]  the sample's 64-bit seed, low and high 32 bits, BIT-CAST into the two floats (never converted)
 *   [33..39]   reserved, ignored
 *   [40..208]  K x K filter weights, row-major with row length K
 *   [209..211] reserved, ignored
 * shape_host: HOST int [B][3] = {K, mh, mw} of each row, the values the entry point validates and sizes LDS from (the
 * table itself lives on the device); they must equal the rows'.  The kernel clamps what it reads from the row so that a
 * table that disagrees still touches nothing but img, seg, its row and its own LDS tile.
 * Image, per sample on the H x W working grid, each stage rounded to 8 bits half up and saturated:
 *   1. the warp, exactly pseg_augment_batch's;
 *   2. correlation (cv2 filter2D): f(y, x) = sum_j sum_i w[j][i] * warp(y + j - K/2, x + i - K/2), fp32; indices beyond the
 *      grid reflect without repeating the edge pixel (-1 -> 1, H -> H - 2; the only pixel when the dimension is 1);
 *   3. the 3 x 4 colour matrix;
 *   4. noise: round(q + scale * n), n = sqrtf(-2 logf(u1)) * cosf(2 pi u2), u1 = ((r0 >> 8) + 1) * 2^-24, u2 = (r1 >> 8) * 2^-24;
 *   5. dropout: the value is kept iff u >= p, u = (r0 >> 8) * 2^-24, and is 0 otherwise;
 *   6. (q - mean_c) / std_c.
 * r0..r3 = Philox4x32-10(key = the seed, counter = (n, stream, 0, 0)).  Noise: n = y * W + x of the working-grid pixel,
 * stream 0, or stream c for plane c when per plane.  Dropout: n = y * W + x, or the mask cell (y * mh / H) * mw + x * mw / W
 * (integer division) with a coarse mask; stream 4, or 4 + c when per plane.  An output pixel (multi-scale) takes the result
 * of its working-grid pixel, noise and dropout included.  Rows with K <= 1, scale <= 0 and p <= 0 give pseg_augment_batch's
 * output bit for bit.  Dynamic LDS: 4 bytes per working-grid pixel of the span of a 32 x 8 output tile plus a halo of
 * K/2 for the launch's largest K; refused above 64 KiB (a multi-scale reduction by more than about 3). */
#define PSEG_AUGMENT_NBHD_ROW 212
#define PSEG_AUGMENT_NBHD_KMAX 13
#define PSEG_AUGMENT_NBHD_K 24
#define PSEG_AUGMENT_NBHD_NOISE 25
#define PSEG_AUGMENT_NBHD_DROP 27
#define PSEG_AUGMENT_NBHD_SEED 31
#define PSEG_AUGMENT_NBHD_WEIGHTS 40
int pseg_augment_batch_nbhd(const uint8_t* img, const uint8_t* seg, const float* params, const int* shape_host, int B, int H, int W,
                            float mean0, float mean1, float mean2, float std0, float std1, float std2, float* out, int oh, int ow,
                            int64_t* target, void* stream);

/* pseg_augment_batch_warp: pseg_augment_batch_nbhd with a coordinate map that is not one affine (the reference's
 * ElasticTransformation, PiecewiseAffine and PerspectiveTransform).  Arguments, shape_host [B][3] = {K, mh, mw}, its
 * validation and the LDS sizing are pseg_augment_batch_nbhd's.  params: fp32 [B][PSEG_AUGMENT_WARP_ROW]:
 *   [0..211]   pseg_augment_batch_nbhd's row, verbatim; [0..5] are now the first two rows h00 h01 h02 / h10 h11 h12 of a 3 x 3
 *              inverse homography
 *   [212..214] h20 h21 h22, its third row
 *   [215]      elastic alpha in pixels; anything not > 0 and <= 3e38 means no jitter
 *   [216]      != 0: the 4 x 4 displacement grid is applied
 *   [217..219] reserved, ignored
 *   [220..251] the grid: node (j, i), row j and column i in 0..3, at 220 + 2 * (4 j + i), holds dx, dy in pixels and sits at
 *              index coordinate (i (W-1)/3, j (H-1)/3)
 * Source coordinate of working-grid pixel (x, y), fp32, in this order:
 *   1. px = x, py = y;
 *   2. elastic jitter: r = Philox4x32-10(key = the row's seed [31] [32], counter = (y * W + x, 8, 0, 0)), u(r) = (r >> 8) * 2^-24;
 *      px = fma(alpha, 2 u(r0) - 1, px), py = fma(alpha, 2 u(r1) - 1, py) (2 u - 1 is exact).  Stream 8; streams 0..6 stay
 *      noise and dropout;
 *   3. grid: gu = clamp(px * (3 / (W - 1)), 0, 3), or 0 when W == 1, gv likewise with H; cell i0 = min((int)gu, 2), j0
 *      likewise; with fu = gu - i0, fv = gv - j0 and the cell's nodes n00 n01 / n10 n11, per component
 *      t = fma(fu, n01 - n00, n00), b = fma(fu, n11 - n10, n10), d = fma(fv, b - t, t); px += dx, py += dy.  A coordinate beyond
 *      the image takes the border's displacement.  The clamp comes before the float -> int conversion: no index leaves the row;
 *   4. homography: den = fma(h20, px, fma(h21, py, h22)); sx = fma(h00, px, fma(h01, py, h02)) / den, sy likewise, correctly
 *      rounded divisions.  The pixel is outside in either border mode (image: cval, label: 0) when den is not > 0 or sx or sy
 *      is NaN / infinite; then pseg_augment_batch's clamp to [-1, size] and its nearest / bilinear taps.
 * Everything after the coordinate is pseg_augment_batch_nbhd's: taps, 8-bit rounding, the filter over the LDS tile, colour
 * matrix, noise, dropout, normalisation, the multi-scale index, and the footprint (nothing but img, seg, the row and the
 * block's own LDS tile is touched, whatever the row holds).  The map is a pure function of the working-grid pixel: the
 * filter's halo evaluates it at the REFLECTED pixel's index, jitter included, and the label blocks evaluate the same function
 * on [H, W], so image and labels move together.  A row with h2 = (0, 0, 1), alpha <= 0 and the grid off gives
 * pseg_augment_batch_nbhd's output bit for bit. */
#define PSEG_AUGMENT_WARP_ROW 252
#define PSEG_AUGMENT_WARP_H2 212
#define PSEG_AUGMENT_WARP_ALPHA 215
#define PSEG_AUGMENT_WARP_GRID_ON 216
#define PSEG_AUGMENT_WARP_GRID 220
int pseg_augment_batch_warp(const uint8_t* img, const uint8_t* seg, const float* params, const int* shape_host, int B, int H, int W,
                            float mean0, float mean1, float mean2, float std0, float std1, float std2, float* out, int oh, int ow,
                            int64_t* target, void* stream);

/* pseg_augment_batch_blend: pseg_augment_batch_warp with a median window, a second filter blended in by a mask, a second
 * colour matrix blended in by a mask, and a hue / saturation shift (the reference's MedianBlur, BlendAlphaSimplexNoise over
 * EdgeDetect / DirectedEdgeDetect, BlendAlphaFrequencyNoise over Multiply / LinearContrast, AddToHueAndSaturation).
 * Arguments are pseg_augment_batch_warp's, except shape_host: HOST int [B][5] = {K, mh, mw, kmed, K2} of each row, which the
 * entry point validates and sizes LDS from; they must equal the rows'.  The kernel clamps what it reads from the row so that
 * a table that disagrees still touches nothing but img, seg, its row and its own LDS.  params: fp32 [B][PSEG_AUGMENT_BLEND_ROW]:
 *   [0..251]    pseg_augment_batch_warp's row, verbatim
 *   [252]       kmed, the median window: 0 = none, otherwise odd, 3 .. PSEG_AUGMENT_BLEND_KMEDMAX
 *   [253]       K2, the size of the second filter G: 0 = no edge blend, otherwise odd, 3 .. PSEG_AUGMENT_BLEND_K2MAX
 *   [254]       != 0: the colour blend is on
 *   [255] [256] dh, the hue shift in sixths of the colour circle, and ds, the saturation shift as a fraction; the stage is
 *               skipped when either is NaN / infinite or both are 0
 *   [257..259]  reserved, ignored
 *   [260..271]  the second colour matrix Mb, 3 x 4 row-major, as [6..17]
 *   [272..496]  K2 x K2 weights of G, row-major with row length K2
 *   [497..499]  reserved, ignored
 *   [500..755]  mask table T1 (edge blend), 16 x 16 row-major        [756..1011] mask table T2 (colour blend), likewise
 * Image, per sample on the H x W working grid, each stage rounded to 8 bits half up and saturated (round_u8):
 *   1. the warp, exactly pseg_augment_batch_warp's;
 *   2. median (kmed >= 3), per plane: element (kmed^2 - 1) / 2 of the sorted values of the kmed x kmed window of stage-1 values;
 *      window indices reflect as the filter's (-1 -> 1, H -> H - 2, repeatedly when the window is wider than the grid).  Like
 *      the warp it is a function of the working-grid pixel: stage 3 reads it beyond the grid at the REFLECTED pixel's index;
 *   3. filter and edge blend over stage-2 values (stage-1 values when kmed = 0): y = round_u8(F), pseg_augment_batch_nbhd's
 *      correlation with the K x K weights at [40..] (K <= 1: y is the input); with K2 >= 3, e = round_u8(G) by the same
 *      correlation and reflection with the weights at [272..], and the result is round_u8(fmaf(m1, e - y, y)), m1 = the sample
 *      of T1 at this pixel;
 *   4. colour: qa = round_u8(M v) as pseg_augment_batch; with [254] != 0, qb = round_u8(Mb v) and the result is
 *      round_u8(fmaf(m2, qa - qb, qb)), m2 = the sample of T2;
 *   5. hue and saturation, on the stage-4 integers r, g, b in fp32 with correctly rounded divisions: mx = max, mn = min,
 *      d = mx - mn; s = mx > 0 ? d / mx : 0; the hue h in [0, 6): 0 when d == 0, else (g - b) / d (+ 6 if negative) when
 *      mx == r, else 2 + (b - r) / d when mx == g, else 4 + (r - g) / d; h' = h + dh, h' -= 6 floorf(h' / 6), taken as 0 when
 *      it lands on 6 (or, under an absurd dh, anywhere outside [0, 6)); s' = clamp(s + ds, 0, 1); i = min((int)h', 5),
 *      f = h' - i; p = mx (1 - s'), q = mx (1 - s' f), t = mx (1 - s' (1 - f)); (r, g, b) = (mx, t, p), (q, mx, p), (p, mx, t),
 *      (p, q, mx), (t, p, mx), (mx, p, q) for i = 0..5; each rounded with round_u8;
 *   6. noise, dropout, (q - mean_c) / std_c and the multi-scale index, exactly pseg_augment_batch_warp's.
 * Mask sample of table T at working-grid pixel (x, y): gx = clamp(fmaf((float)x + 0.5f, 16.f / (float)W, -0.5f), 0, 15),
 * i0 = min((int)gx, 14), fu = gx - i0; gy, j0, fv likewise with H; t = fmaf(fu, T[j0][i0+1] - T[j0][i0], T[j0][i0]), b the same
 * on row j0 + 1, m = fmaf(fv, b - t, t), clamped to [0, 1], a NaN counting as 0.  The clamp of gx comes before the float -> int
 * conversion: no index leaves the table.
 * Labels are pseg_augment_batch_warp's: stages 2 to 5 never touch them.  A row with kmed = 0, K2 = 0, [254] = 0 and
 * dh = ds = 0 gives pseg_augment_batch_warp's output bit for bit; T1 all 0 gives the bits of the same row with K2 = 0, T1 all 1
 * those of a row whose F is G with no blend; T2 all 1 gives the bits of the row with M alone, T2 all 0 those of a row with Mb
 * in M's place.  Dynamic LDS, 4 bytes per pixel: the span of a 32 x 8 output tile plus a halo of kmed/2 + max(K/2, K2/2) (at
 * most 12) for stage 1 and, with a median, a second tile with a halo of max(K/2, K2/2) for stage 2, for the sample of the
 * launch that needs most; refused above 64 KiB. */
#define PSEG_AUGMENT_BLEND_ROW 1012
#define PSEG_AUGMENT_BLEND_KMEDMAX 11
#define PSEG_AUGMENT_BLEND_K2MAX 15
#define PSEG_AUGMENT_BLEND_KMED 252
#define PSEG_AUGMENT_BLEND_K2 253
#define PSEG_AUGMENT_BLEND_COLOUR_ON 254
#define PSEG_AUGMENT_BLEND_HUE 255
#define PSEG_AUGMENT_BLEND_MB 260
#define PSEG_AUGMENT_BLEND_WEIGHTS2 272
#define PSEG_AUGMENT_BLEND_T1 500
#define PSEG_AUGMENT_BLEND_T2 756
#define PSEG_AUGMENT_BLEND_TABLE 16
int pseg_augment_batch_blend(const uint8_t* img, const uint8_t* seg, const float* params, const int* shape_host, int B, int H, int W,
                             float mean0, float mean1, float mean2, float std0, float std1, float std2, float* out, int oh, int ow,
                             int64_t* target, void* stream);

/* ------------------------------------------------------------------ optimiser (flat parameter arena)
 * One launch over the whole arena; grad_scale folds the 1/world_size of the data-parallel mean
 * (README.md:42-44, train.py:112-117) and the 1/accumulate of gradient accumulation (train.py:65).
 * decay_mask (nullable, uint8 per 4-element group) selects where weight decay applies. */
int pseg_sgd_step(float* param, const float* grad, float* momentum_buf, int64_t n, float lr, float momentum,
                  float weight_decay, int nesterov, float grad_scale, int first_step, void* stream);
int pseg_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                   float beta1, float beta2, float eps, float weight_decay, int decoupled, float grad_scale,
                   int step, void* stream);
int pseg_fill(float* x, int64_t n, float value, void* stream);

/* ---- grouped step: per-run learning-rate factor and weight decay, global-norm clipping, weight EMA (csrc/optim.hip).
 * Additive: PSEG_ABI_VERSION does not move.
 *
 * A RUN is a contiguous range of the arena whose floats share their hyper-parameters.  The table is an array of
 * pseg_opt_run_t, ascending and disjoint, offset and count multiples of 4 (arena segments are: no 16-byte access straddles
 * a run and there is no scalar tail).  first_block is the index of the run's first 256-thread block; the run owns the blocks
 * up to the next run's first_block (the last one up to total_blocks), at least 1 and at most ceil(count / PSEG_OPT_RUN_SPAN):
 * a block covers PSEG_OPT_RUN_SPAN floats per trip and strides by its run's block count.  `runs` is the table in DEVICE memory
 * (what the kernel reads), `runs_host` the same table in HOST memory: every launch validates the host copy against n and
 * total_blocks before anything is enqueued.
 *
 * pseg_grad_sumsq: clip_state[0] = (float)sqrt(sum of grad[i]^2), squares and sums in fp64, one partial per block into
 *   `workspace` (pseg_grad_sumsq_workspace_bytes(n) bytes, at most 8 * PSEG_GRAD_SUMSQ_MAX_PARTIALS; 8-byte aligned), folded by a
 *   second single-block launch in a fixed order.  The grid depends on n only, there is no atomic: bit-reproducible from call
 *   to call.  n is a multiple of 4.
 * pseg_opt_step_sgd / pseg_opt_step_adam, per element of run r, by the kernel that pseg_sgd_step / pseg_adam_step launch too:
 *     d = g * (gscale_eff * coef);  weight decay wd_r, coupled (d += wd_r * w) or `decoupled` (w *= 1 - lr_r * wd_r);
 *     momentum / Nesterov, or the Adam moments;  w -= lr_r * d  (Adam: step_size = lr_r / bias_correction1),  lr_r = lr * lr_mult_r;
 *     ema (nullable):  e = ema_decay * e + (1 - ema_decay) * w_new.
 *   gscale_eff = grad_scale, times mp_state[1] when mp_state (nullable: the 8-float `-mp` state above) is given.
 *   coef = 1 when max_norm == 0, else min(1, max_norm / (clip_state[0] * |gscale_eff| + 1e-6)) -- torch's clip_grad_norm_ with
 *   error_if_nonfinite=False -- derived by every thread from the device state; one thread records clip_state[1] = coef,
 *   clip_state[2] = clip_state[0] * |gscale_eff| (the norm of the unscaled gradients) and adds 1 to clip_state[3] when coef < 1.
 *   clip_state: 4 floats on the device, required when max_norm > 0.
 *   With mp_state: a raised found-inf flag (mp_state[3]) returns before anything is written -- parameters, moments, EMA and
 *   clip_state[1..3] stay as they were; first step / bias corrections come from mp_state[4] (first_step / step are ignored).
 *   Without it they come from the host: first_step as in pseg_sgd_step, step >= 1 as in pseg_adam_step (bias corrections in double).
 *   pseg_sgd_step, pseg_sgd_step_mp, pseg_adam_step and pseg_adam_step_mp are this step over the whole arena as ONE run with
 *   lr_mult = 1, max_norm = 0 and ema = NULL, passed to the kernel by value (no table; n need not be a multiple of 4): a
 *   one-run table with those values gives their result bit for bit.  Refused with a message naming the check: null / misaligned (16 bytes) pointers, a
 *   table that breaks a rule above, ema_decay outside [0, 1), max_norm < 0. */
#define PSEG_OPT_RUN_SPAN 1024
#define PSEG_GRAD_SUMSQ_MAX_PARTIALS 1024
typedef struct {
  int64_t offset, count, first_block;
  float lr_mult, weight_decay;
} pseg_opt_run_t;
int64_t pseg_grad_sumsq_workspace_bytes(int64_t n);
int pseg_grad_sumsq(const float* grad, int64_t n, void* workspace, int64_t workspace_bytes, float* clip_state, void* stream);
int pseg_opt_step_sgd(float* param, const float* grad, float* momentum_buf, float* ema, int64_t n, const pseg_opt_run_t* runs,
                      const pseg_opt_run_t* runs_host, int n_runs, int64_t total_blocks, float lr, float momentum, int nesterov,
                      int decoupled, float grad_scale, int first_step, float max_norm, float ema_decay, float* clip_state,
                      const float* mp_state, void* stream);
int pseg_opt_step_adam(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n,
                       const pseg_opt_run_t* runs, const pseg_opt_run_t* runs_host, int n_runs, int64_t total_blocks, float lr,
                       float beta1, float beta2, float eps, int decoupled, float grad_scale, int step, float max_norm,
                       float ema_decay, float* clip_state, const float* mp_state, void* stream);
/* amax_inout[0] = max(amax_inout[0], max |x[m*ld + c]|), m < M, c < C (atomic on the float's bit pattern; zero it first) */
int pseg_amax(const float* x, int64_t ld, int64_t M, int C, float* amax_inout, void* stream);
/* max|.| of many contiguous float arrays in one launch (every conv filter of a model, once per step).  jobs: device array
 * of n records of three int64 {device address, element count, index of the record's first 256-thread block}, block
 * indices ascending from 0; total_blocks = their sum.  out[j] = max|x_j| (the launch zeroes out[] first). */
int pseg_amax_batch(const int64_t* jobs, int n, int64_t total_blocks, float* out, void* stream);

/* debug: while `buffer` is non-NULL every block of the exact-fp32 LDS-DMA gather kernel writes five uint64 words to
 * buffer[5 * blockIdx.x ...] -- wall_clock64 at entry / first tile landed / last MFMA issued / stores drained, and HW_ID
 * (tools/conv_phases.py turns them into a phase table).  Debug builds only (-DPSEG_CONV_TRACE=1; the default build returns
 * an error for a non-NULL buffer): one global pointer, no stream ordering. */
int pseg_debug_conv_trace(void* buffer);
/* debug / tests: which kernel did the calling thread's LAST convolution entry point (pseg_conv2d_fwd / _dgrad* / _wgrad* /
 * _wgrad_slabs and their _h forms, the fp16 weight gradient included: code 23) enqueue?  A parity test of a specialised kernel can
 * so assert that the kernel it means to test is the one that ran. */
#define PSEG_KERNEL_GATHER_REGISTER 1        /* gather_conv_kernel (register-staged; every precision, split-K) */
#define PSEG_KERNEL_GATHER_LIMB_DMA 2        /* gather_limb_dma_kernel (pre-split bf16 planes) */
#define PSEG_KERNEL_GATHER_RING 3            /* gather_f32_dma_kernel */
#define PSEG_KERNEL_GATHER_RING_GENERIC 4    /* gather_f32_dma_kernel, channel counts off the K-step grid */
#define PSEG_KERNEL_GATHER_POINTWISE 5       /* gather_f32_pw_kernel (persistent) */
#define PSEG_KERNEL_GATHER_HALO 6            /* gather_f32_halo_kernel */
#define PSEG_KERNEL_WGRAD_REGISTER 11        /* wgrad_kernel */
#define PSEG_KERNEL_WGRAD_LIMB 12            /* wgrad_limb_kernel */
#define PSEG_KERNEL_WGRAD_DMA 13             /* wgrad_f32_dma_kernel */
#define PSEG_KERNEL_WGRAD_HALO 14            /* wgrad_f32_halo_kernel */
#define PSEG_KERNEL_GATHER_H 21              /* gather_h_kernel (fp16) */
#define PSEG_KERNEL_GATHER_H_PERSISTENT 22   /* gather_hp_kernel (fp16) */
#define PSEG_KERNEL_WGRAD_H 23               /* wgrad_h_kernel (fp16) */
int pseg_debug_last_conv_kernel(void);
/* ... and, when that was an fp16 gather launch (codes 21 / 22: pseg_conv2d_fwd_h / _dgrad_h / _dgrad_bnstat_h), WHICH instantiation:
 * out6 = {tile rows, tile columns, K-step in halves (32 | 64), ring depth as launched (after the clamp to the K loop's length;
 * the persistent kernel's own depth, 2 | 3, when it ran), variant (0 plain, 1 tap-skipping, 2 channels off the K-step grid),
 * 1 when the instantiation with the fused BatchNorm-backward sums ran}.  Zeros before the thread's first such launch.  A few
 * host-side integer stores per launch, no device work; additive: PSEG_ABI_VERSION does not move. */
int pseg_debug_last_gather_h(int* out6);
/* ... and, when that was a weight gradient (codes 11-14 and 23: pseg_conv2d_wgrad / _wgrad_slabs / _wgrad_h / _wgrad_slabs_h), WHICH
 * launch: out11 = {kernel code, tile rows, tile columns, pixels per K-step (32 | 64 for fp16, 32 for the fp32 / limb kernels), the
 * kernel's SKIP flag, pixel order (0 dense, 1 dead image rows skipped, 2 dead patches skipped, 3 packed live rectangles, 4 row-major
 * on the LDS-DMA kernel), 1 when the pixels run in patch order, patch rows, patch columns, pixel splits, pixels per split}.
 * Zeros before the thread's first such launch.  Host-side integer stores next to the launch, no device work.
 * pseg_conv2d_wgrad_choice / _choice_h: the same record for the launch that WOULD run for a problem -- a pure function of the integer
 * arguments and the PSEG_* planning switches, read off the selection the launch reads; no device needed.  Additive:
 * PSEG_ABI_VERSION does not move. */
int pseg_debug_last_wgrad(int* out11);
int pseg_conv2d_wgrad_choice(int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad, int dil,
                             int precision, int concurrent, int* out11);
int pseg_conv2d_wgrad_choice_h(int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad, int dil,
                               int* out11);
/* ... and, when that was an exact-fp32 or limb gather launch (codes 1-6: pseg_conv2d_fwd / _dgrad / _dgrad_bnstat / _dgrad_planes),
 * WHICH instantiation: out13 = {kernel code as launched (5 only when the persistent kernel accepted the problem), tile rows, tile
 * columns, the arithmetic the kernel ran with (PSEG_PREC_*: the caller's on the register-staged kernel, BF16X3 on the pre-split
 * limb kernel, FP32 on the LDS-DMA kernels whatever was asked for), the kernel's SKIP flag, ring depth (2 | 3; 0 off the ring
 * kernel), 1 for the ring kernel's GENERIC form, row order (GatherConvParams::row_perm: 0 row-major, 1 parity classes, 2 pixel
 * patches, 3 a 1x1 conv's 1 x M image, 4 rows sorted by liveness class), patch rows, patch columns (0 off the patch order), K
 * splits, 1 when the launch carried the fused BatchNorm-backward sums (on the persistent kernel: its BNS instantiation), 1 when the
 * problem was offered to the persistent pointwise kernel first}.  Zeros before the thread's first such launch; a refused call
 * leaves it alone.  Host-side integer stores next to the launch, no device work.
 * pseg_conv2d_gather_choice: the same record for the launch that WOULD run -- dgrad: 0 the forward conv, 1 the data gradient of the
 * conv so described; precision: the caller's PSEG_PREC_*; stats / bias / planes / bns / accumulate: fused statistics, a bias, the
 * pre-split limb planes, the fused BatchNorm-backward sums and accumulation asked for.  A pure function of its integer arguments and
 * the PSEG_* planning switches, read off the selection the launch reads; no device needed.  The kernel code is the tile-per-block
 * one, with the last field 1 where the persistent kernel is tried first (it declines by device occupancy), and 0 where the launch
 * would be refused on the choice alone (limb planes or fused sums no kernel carries, fused statistics of a plan that splits K, a
 * forced tile without an instantiation in this arithmetic).  Additive: PSEG_ABI_VERSION does not move. */
int pseg_debug_last_gather(int* out13);
/* ... and the calling thread's last BatchNorm / activation / column-sum launch (csrc/norm_act.hip; these launches do not move
 * pseg_debug_last_conv_kernel): out12 = {kernel, storage type (0 fp32, 1 fp16), V = channels per lane, NR = rows (row groups, for the
 * finalize kernels) in flight per lane, MODE, LANES, block x, block y, grid x, grid y, rows per group R (statistics, reduce) or rows
 * per block RB (apply, forward-rows, the fused kernels) or partial rows as the last kernel saw them (finalize, column reduce), 1
 * when pseg_bn_finalize ran its two-stage merge first}.
 *   kernel: 1 col_stats_kernel (MODE 1 shifted statistics, 0 plain sums: pseg_col_sum, whose record is this launch's with LANES of
 *   the col_reduce_kernel launch that followed), 2 bn_bwd_reduce_kernel, 3 stat_merge_kernel (never last), 4 bn_finalize_kernel,
 *   5 bn_bwd_finalize_kernel, 6 col_reduce_kernel (on its own: the depthwise weight gradient), 7 bn_eval_coeffs_kernel,
 *   8 bn_act_fwd_kernel, 9 bn_act_fwd_rows_kernel, 10 bn_act_bwd_apply_kernel, 11 act_bwd_kernel, 12 copy2d_kernel,
 *   13 bn_fwd_small_kernel (pseg_bn_fwd_fused), 14 bn_bwd_small_kernel (pseg_bn_bwd_fused).
 *   MODE of the backward kernels: where act'(z) came from -- 0 no activation, 1 the bitmask, 2 the stored z, 3 recomputed from y.
 *   LANES: row lanes of the finalize / reduce block (32 | 128; 32 inside the fused kernels), 0 elsewhere.
 * Zeros before the thread's first such launch; a refused call leaves it alone.  Host-side integer stores next to the launch, no
 * device work.  Additive: PSEG_ABI_VERSION does not move. */
int pseg_debug_last_norm(int* out12);
/* ... and the calling thread's last loss / mask / metric launch (csrc/loss.hip: pseg_ce_fwd_bwd, pseg_ce_upsampled_fwd_bwd,
 * pseg_argmax, pseg_confusion, pseg_scale_inplace): out8 = {kernel, CMAX = the compile-time class bound (4 | 8 | 24 | 32 on
 * ce_fused_kernel, 24 on the up-sampled kernels, 0 elsewhere), VEC = consecutive pixels (elements, for scale_inplace) per lane,
 * grid x, block x, form of the up-sampled loss (0 none, 1 gather: ce_up_fused_kernel, 2 scatter: ce_up_scatter_kernel +
 * ce_up_combine_kernel), per-block partials handed to the finish kernel (ce_finish_kernel; ce_up_finish_kernel behind the
 * scatter form; 0 where none runs), 1 when a gradient was asked for (dlogits / dlogits_lr not NULL)}.
 *   kernel: 1 ce_fused_kernel, 2 ce_generic_kernel, 3 ce_up_fused_kernel, 4 ce_up_scatter_kernel, 5 argmax_kernel,
 *   6 confusion_kernel, 7 scale_inplace_kernel.
 * Zeros before the thread's first such launch; a refused call leaves it alone.  Host-side integer stores next to the launch, from
 * the variables the launch takes; no device work.  Additive: PSEG_ABI_VERSION does not move. */
int pseg_debug_last_loss(int* out8);
int pseg_conv2d_gather_choice(int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int kh, int kw, int stride, int pad, int dil,
                              int dgrad, int precision, int stats, int bias, int planes, int bns, int accumulate, int* out13);

/* ---- lane executor: a captured hipGraph replayed as plain launches on a few streams (csrc/lanes.hip) --------------------
 * The reference drives its step from Python through torch/apex (train.py:63-72 via pytorch_modules' Trainer); for the
 * launch-bound configurations (BASELINE configs[1], configs[4]) the host, not the GPU, sets the step time.  A step that
 * was captured once (hipStreamBeginCapture -- torch.cuda.graph on the Python side) is replayed here without Python and
 * without hipGraphExec: pseg_lanes_build walks the graph (kernel / memset / empty nodes and their edges; a graph with memcpy or other
 * nodes is refused with an error -- their parameters cannot be read back reliably -- and the caller runs such a step EAGERLY:
 * hipGraphLaunch of a forked graph is not a fallback, DESIGN.md section 5 "Fault records"),
 * assigns the nodes to at most max_lanes stream-ordered lanes and turns the edges between lanes into events;
 * pseg_lanes_launch enqueues the whole step -- lane 0 on `stream`, the other lanes on streams the executor owns, all of
 * them after what `stream` holds so far, and `stream` continues after all of them.  The hipGraph_t (argument blocks,
 * private memory pool) must outlive the executor.  Same launches, dependency-respecting order: results are bit-identical
 * to eager execution.  pseg_lanes_info reports graph nodes, launching nodes, lanes used and cross-lane events. */
int pseg_lanes_build(void* hip_graph, int max_lanes, int64_t* handle);
int pseg_lanes_info(int64_t handle, int* nodes, int* launches, int* lanes, int* events);
int pseg_lanes_launch(int64_t handle, void* stream);
/* The lanes of every executor of a device run on one pool of streams that lives as long as the process (a stream per
 * executor would land on whatever hardware queue the runtime's round-robin has reached: GPU_MAX_HW_QUEUES = 4, two busy
 * lanes on one queue serialise).  pseg_lanes_reserve(lanes) creates -- and touches -- the streams for `lanes` lanes on the
 * current device NOW (the Trainer calls it before it captures its first step -- from its constructor for a model that lives on
 * the replay, so that the pool exists before the process's other streams); pseg_lanes_build reserves what is missing. */
int pseg_lanes_reserve(int lanes);
/* Drains the executor's device (hipDeviceSynchronize: the executor's events are bound to kernels of the last replay on the
 * pool streams AND on the caller's stream), then releases events and host state.  Must not be called while a stream capture
 * is open; on failure nothing is released and the handle stays valid. */
int pseg_lanes_destroy(int64_t handle);

/* Markers: where the REPLAYED step meets work the executor does not own -- the data-parallel gradient exchange
 * (train.py:33-35,112-117: DistributedDataParallel overlaps its bucket all-reduces with backward).  pseg_mark enqueues a
 * one-word memset (zero) of `word` on `stream`; inside a capture that is a memset node which depends on everything the
 * stream holds so far.  pseg_lanes_bind_markers(handle, base, count): every such node of the walked graph whose word lies
 * in base[0..count) becomes marker (word index); the replay records an event right after it on its lane.  After
 * pseg_lanes_launch, pseg_lanes_wait_marker(handle, id, stream) makes `stream` wait for all events of marker `id` (one
 * per stream the marker was set on) of that launch -- the caller then enqueues the bucket's all-reduce on `stream`, and it
 * overlaps the rest of the replayed backward.  (In a graph replayed any other way the markers are harmless memsets.) */
int pseg_mark(void* word, void* stream);
int pseg_lanes_bind_markers(int64_t handle, const void* base, int count, int* bound);
int pseg_lanes_wait_marker(int64_t handle, int id, void* stream);

/* ---- gradient exchange over RCCL (csrc/comm.hip) -----------------------------------------------------------------------
 * allreduce_bucket(flat_grad, stream): what DistributedDataParallel does for the reference inside its external Trainer
 * (README.md:42-44, train.py:33-35,112-117) -- the gradients of one bucket summed over the ranks, in place, on `stream`
 * (the caller's side stream: it overlaps the rest of backward).  A bucket is a contiguous range of the fp32 gradient arena.
 * RCCL is bound at run time (PSEG_RCCL_PATH if set, else the process's own librccl.so, else the loader path):
 * pseg_comm_available() tells whether that worked.  One rank calls pseg_comm_unique_id (128 bytes) and hands the id to the
 * others by whatever channel the host has; every rank then calls pseg_comm_init(id, nranks, rank) with its HIP device
 * current (collective: returns when all ranks have joined).  The mean's 1/nranks is the optimiser's grad_scale. */
int pseg_comm_available(void);
int pseg_comm_unique_id(void* id128);
int pseg_comm_init(const void* id128, int nranks, int rank, int64_t* comm);
int pseg_comm_destroy(int64_t comm);
int pseg_allreduce_bucket(int64_t comm, float* flat_grad, int64_t count, void* stream);
/* RCCL's version code (ncclGetVersion: major * 10000 + minor * 100 + patch), for run records. */
int pseg_comm_version(int* version);
/* The same sum as a reduce-scatter + all-gather pair, in place (on the fully connected 8-GPU xGMI
 * node a direct exchange uses all seven links of a GPU, a ring is bound by one): rank r first receives the sum of slice
 * [r * count_per_rank, (r + 1) * count_per_rank) of the bucket, then the reduced slices are gathered.  The bucket holds
 * nranks * count_per_rank elements (the caller all-reduces a remainder of fewer than nranks elements separately).
 * Replaces the same DistributedDataParallel exchange as pseg_allreduce_bucket (README.md:42-44, train.py:112-117). */
int pseg_reduce_scatter_bucket(int64_t comm, float* flat_grad, int64_t count_per_rank, int rank, void* stream);
int pseg_all_gather_bucket(int64_t comm, float* flat_grad, int64_t count_per_rank, int rank, void* stream);

/* ---- fault diagnostics (csrc/diag.hip) -----------------------------------------------------------------------------------
 * The reference's loop (train.py:71-72) dies with a Python traceback when something below it faults; a fault inside the HIP
 * runtime leaves no native frame in it.  pseg_fault_backtrace_enable() installs handlers for SIGSEGV / SIGBUS / SIGFPE /
 * SIGILL / SIGABRT that write the faulting thread's native frames to stderr (backtrace_symbols_fd) and then chain to the
 * handler installed before (Python's faulthandler) or re-raise with the default action.  PSEG_SEGV_BACKTRACE=1 in the
 * environment installs them when the library is loaded.  pseg_fault_backtrace_enabled() -> 0 / 1. */
int pseg_fault_backtrace_enable(void);
int pseg_fault_backtrace_enabled(void);

#ifdef __cplusplus
}
#endif
#endif /* PSEG_AMD_H */
