/* segamd.h -- C-ABI of libsegamd.so, the MI355X (gfx950) hot path of the
 * SEAME-pt/Team02-ObjectDetection segmentation models (MobileNetV2UNet / UNet).
 *
 * The reference has no native code: its hot path is PyTorch's aten dispatch of
 * the ops in src/unet.py + nn.CrossEntropyLoss (main.py:99, src/train.py:37).
 * Each entry point below replaces the aten op(s) named in its comment; the
 * Python nn.Module / train_model surface (team02-objectdetection_amd/seg_amd)
 * binds them with ctypes, and INTEGRATION.md shows the binding.
 *
 * Contract (all functions):
 *  - activations are NHWC fp32 "row" tensors: row = pixel, `ld*` = row stride in
 *    floats (a multiple of 4, >= round_up(C, 4)); pointers 16-byte aligned;
 *  - the caller owns every buffer, including workspaces (sizes from the
 *    *_workspace / *_splits / *_blocks queries); nothing allocates;
 *  - asynchronous and stream-ordered on `stream`; no host synchronisation, so
 *    every call is hipGraph-capturable; no internal threads or global state;
 *  - returns hipError_t (0 = success); argument errors return
 *    hipErrorInvalidValue before any launch;
 *  - reductions are deterministic (fixed-order partial slabs, no float atomics).
 */
#ifndef SEGAMD_H
#define SEGAMD_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* act codes: 0 none, 1 ReLU (src/unet.py:60,63,115), 2 ReLU6 (torchvision). */

/* ---- convolution (aten conv2d / convolution_backward) ----------------------- */

/* Implicit-GEMM conv on f32 MFMA: out = conv(in, W) (+bias) (+add).
 * Replaces nn.Conv2d forward of the dense 3x3 convs (src/unet.py:58,61), the 1x1
 * head (src/unet.py:113,116) and torchvision's expand/project 1x1 convs
 * (reached through src/unet.py:15-19); with mode-1 packed weights it is also the
 * data gradient of those (stride-1) convs.  ks in {1,3}.  `stat` (optional):
 * per-row-tile BatchNorm partials of conv + bias ([row_tiles][2][Cout]: tile sum, tile
 * M2 about the tile mean; from the fp32 accumulators, before `add` and before any
 * rounding to the storage type), consumed by seg_bn_stats_tiles -- the BN statistics
 * pass fused into the conv epilogue. */
int seg_conv_igemm(const float* in, long ldin, int N, int H, int W, int Cin,
                   const float* wk, int ldk, const float* bias,
                   float* out, long ldout, int Ho, int Wo, int Cout,
                   int ks, int stride, int pad,
                   const float* add, long ldadd, float* stat, hipStream_t stream);
/* seg_conv_igemm with an epilogue activation: out = act(conv + bias + add).  The
 * inference path (BatchNorm folded into wk/bias by seg_bn_fold_batch) uses it for
 * conv -> BN -> ReLU/ReLU6 of src/unet.py:58-63,113-115 and torchvision's
 * Conv2dNormActivation in one launch.  act != 0 excludes `stat`.  splits > 1
 * (seg_conv_igemm_splits) runs split-K: raw partials in `work` (>= splits * M *
 * Cout floats, M = N*Ho*Wo), then a fixed-order reduce that applies the epilogue;
 * it excludes `stat`.  splits == 1: `work` unused. */
int seg_conv_igemm_act(const float* in, long ldin, int N, int H, int W, int Cin,
                       const float* wk, int ldk, const float* bias,
                       float* out, long ldout, int Ho, int Wo, int Cout,
                       int ks, int stride, int pad,
                       const float* add, long ldadd, float* stat, int act, float* work, int splits,
                       hipStream_t stream);
/* seg_conv_igemm_act with bf16 math (BASELINE configs[2]/[4], the bf16 configurations;
 * replaces the autocast bf16 conv2d of the same call sites): the same fp32 tensors,
 * both operands rounded to bf16 (round-to-nearest-even) in the LDS staging,
 * v_mfma_f32_32x32x16_bf16 with fp32 accumulation, the fp32 epilogue. */
int seg_conv_igemm_bf16(const float* in, long ldin, int N, int H, int W, int Cin,
                        const float* wk, int ldk, const float* bias,
                        float* out, long ldout, int Ho, int Wo, int Cout,
                        int ks, int stride, int pad,
                        const float* add, long ldadd, float* stat, int act, float* work, int splits,
                        hipStream_t stream);
/* seg_conv_igemm_act with fp16 math (BASELINE configs[3], the fp16 inference
 * configuration; replaces the autocast fp16 conv2d of inference.py:162-163): operands
 * rounded to fp16 (RNE) in the LDS staging, v_mfma_f32_32x32x16_f16, fp32 accumulation
 * and epilogue.  Operands beyond the fp16 range become inf, as under autocast. */
int seg_conv_igemm_f16(const float* in, long ldin, int N, int H, int W, int Cin,
                       const float* wk, int ldk, const float* bias,
                       float* out, long ldout, int Ho, int Wo, int Cout,
                       int ks, int stride, int pad,
                       const float* add, long ldadd, float* stat, int act, float* work, int splits,
                       hipStream_t stream);
/* Thin-K 1x1 conv (stride 1) as a GEMM: out[M][N] = in[M][K] . W^T (+ bias) (+ add), K <= 32,
 * K % 8 == 0, N <= 192 -- the output-heavy expand convs of torchvision's InvertedResidual
 * (16 -> 96, 24 -> 144, 32 -> 192; src/unet.py:15-19), outconv (src/unet.py:113,116) and the
 * data gradients of thin project convs.  wk: [N][ldk] (the 1x1 weight as is, or its data-gradient
 * pack).  stat (optional): BN partials [seg_conv_pw_row_tiles(M)][2][N] (tile sum, M2 about the
 * tile mean; 128-row tiles) for seg_bn_stats_tiles.  in_scale / in_shift / in_act (optional):
 * the producer's lazy BatchNorm + activation applied on load (as seg_conv_igemm_xf).  Rows in
 * 16-byte vectors (ld % 4). */
int seg_conv_pw_row_tiles(long M);
int seg_conv_pw(const float* in, long ldin, long M, int K, const float* wk, int ldk, const float* bias,
                float* out, long ldout, int N, const float* add, long ldadd, float* stat,
                const float* in_scale, const float* in_shift, int in_act, hipStream_t stream);
/* Split-K factor for seg_conv_igemm_act (1 = none): > 1 only when the output tiles
 * cannot fill the 256 CUs (batch-1 inference). */
int seg_conv_igemm_splits(long M, int Cout, int Cin, int ks);
/* seg_conv_igemm_act / _bf16 / _f16 with split-K combined inside the launch (the inference forward's
 * batch-1 convs): when the whole grid is co-resident (and splits <= 32) the split blocks of a tile combine it
 * together, each applying the split-K epilogue to its share -- a block that cannot wait for its peers (another
 * kernel holding the CUs) leaves its share to the tile's last arrival, so no block ever spins on a peer that is
 * not resident; else the separate reduce runs.  Bitwise the two-launch result.  cnt: 4 *
 * seg_conv_igemm_tiles(M, Cout) unsigned, zero before the first launch (epoch words: never re-armed; one counter
 * buffer per concurrently running launch).  No BN statistics. */
int seg_conv_igemm_tiles(long M, int Cout);
/* Plan for those launches: out[3] = (splits, tile, output tiles -- the counters are 4 per tile).  tile -1 =
 * the cost model's (seg_conv_igemm_tiles), else an index into the kernel's tile table (the batch-1 rule:
 * short K unsplit on 64x64 tiles, long K split on 8-wave 128x64 tiles).  Tile choice does not change
 * results; the split count does (another K partition). */
int seg_conv_igemm_plan_b1(long M, int Cout, int Cin, int ks, int* out);
int seg_conv_igemm_act_ic(const float* in, long ldin, int N, int H, int W, int Cin, const float* wk, int ldk,
                          const float* bias, float* out, long ldout, int Ho, int Wo, int Cout, int ks, int stride,
                          int pad, const float* add, long ldadd, int act, float* work, int splits, int tile, unsigned* cnt,
                          hipStream_t stream);
int seg_conv_igemm_bf16_ic(const float* in, long ldin, int N, int H, int W, int Cin, const float* wk, int ldk,
                           const float* bias, float* out, long ldout, int Ho, int Wo, int Cout, int ks, int stride,
                           int pad, const float* add, long ldadd, int act, float* work, int splits, int tile, unsigned* cnt,
                           hipStream_t stream);
int seg_conv_igemm_f16_ic(const float* in, long ldin, int N, int H, int W, int Cin, const float* wk, int ldk,
                          const float* bias, float* out, long ldout, int Ho, int Wo, int Cout, int ks, int stride,
                          int pad, const float* add, long ldadd, int act, float* work, int splits, int tile, unsigned* cnt,
                          hipStream_t stream);

/* seg_conv_igemm as a stride-1 data gradient (pad ks/2, no bias, optional fused addend) that
 * completes dA of a BatchNorm layer whose pre-BN output is `by`: the epilogue also writes that
 * layer's BN-backward partials per row tile, bpart[seg_conv_igemm_row_tiles(M, Cout)][2][Cout] =
 * (sum dz, sum dz (by - bmean)), dz = out * act'(by * bscale + bshift) on the values as stored --
 * for seg_bn_bwd_finalize_tiles, in place of seg_bn_bwd_coef's reduction pass over dA (the
 * BN-backward chain of src/unet.py:59-63 / torchvision's BatchNorm via src/unet.py:15-19). */
int seg_conv_igemm_bnout_ok(long M, int Cout, int bf16);
int seg_conv_igemm_bnout(const float* in, long ldin, int N, int H, int W, int Cin, const float* wk, int ldk,
                         float* out, long ldout, int Cout, int ks, const float* add, long ldadd,
                         const float* by, long ldby, const float* bscale, const float* bshift,
                         const float* bmean, int bact, float* bpart, hipStream_t stream);

/* The implicit GEMM's tile table: BM x BN output rows x channels per block, waves per block.
 *    0  128x128  4     1   64x128  4     2  128x64   4     3   64x64   4     4  128x96   4
 *    5  128x160  4     6  256x32   4     7  128x32   4     8  128x128  8     9  128x128  8
 *   10  256x128  8    11  128x256  8    12  128x64   8    13  256x64   8    14   64x128  8
 * (8 and 9 differ in the wave layout: 64x32 and 32x64 accumulators per wave.)  The cost model picks among
 * 0..7; 8..14 are reached through the hook below and the `tile` argument of the _ic entry points.
 * seg_conv_igemm_bnout* needs 64 % (BN / v) == 0, v = 4 (fp32 storage) or 8 (bf16) output elements per
 * 16-byte store: every tile but 4 and 5 (seg_conv_igemm_bnout_ok).
 * Tuning hook: force tile configuration t (0..14) for the following seg_conv_igemm* launches and
 * seg_conv_igemm_row_tiles / _tiles / _tile / _bnout_ok queries of this process, -1 = the built-in cost
 * model.  Tile choice does not change results, except the row partition of the BN partials. */
int seg_igemm_force_tile(int t);
/* The table entry an M x Cout output runs on. */
int seg_conv_igemm_tile(long M, int Cout);
/* Row tiles (and their height) seg_conv_igemm uses for an M x Cout output. */
int seg_conv_igemm_row_tiles(long M, int Cout, int* tile_rows);

/* Pack w[Cout][Cin][ks][ks]: mode 0 -> wk[Cout][ldk] (forward; tap runs padded
 * to kin_pad >= Cin channels), mode 1 -> wk[Cin][ldk] transposed + tap-flipped
 * (data gradient; tap runs padded to kin_pad >= Cout channels). */
int seg_pack_conv_weight(const float* w, float* wk, int Cout, int Cin, int ks, int ldk,
                         int mode, int kin_pad, hipStream_t stream);

/* Weight gradient (convolution_backward, weight path) as split-K partial slabs
 * part[splits][Cout][ks*ks][Cin], Cin as passed (a multiple of 4: the engine pads the stems' 3 channels with a
 * zero one); splits from seg_conv_wgrad_splits, but any splits >= 1 is legal.
 * Split s sums the output pixels [s * kchunk, min(M, (s + 1) * kchunk)) in NHWC row order (M = N * Ho * Wo),
 * kchunk = ceil(M / splits) rounded up to whole K chunks: 16 pixels, the bf16-math entry points 32.  The rounding
 * can leave trailing splits with an empty range; such a split writes an all-zero slab, so seg_conv_wgrad_reduce
 * always sums `splits` slabs.
 * Tile (rows of Cout x columns of Nw = ks*ks*Cin) of the launch:
 *   Cout >= 128:       128x128 if Nw >= 128, else 128x32
 *   64 <= Cout < 128:  64x128 if Nw >= 128, else 64x64
 *   Cout < 64:         32x128 */
int seg_conv_wgrad_splits(long M, int Cout, int Cin, int ks);
/* The split count the engine uses for the bf16-math weight gradients (fewer, longer blocks). */
int seg_conv_wgrad_splits_bf16(long M, int Cout, int Cin, int ks);
/* The geometry seg_conv_wgrad (bf16 0) or seg_conv_wgrad_bf16 / _bf16io (bf16 1) and their _xf forms launch with
 * for `splits` splits: out3 = {tile rows BM, tile columns BN, kchunk}.  A host function (the launch takes its tile
 * and kchunk from the same code); hipErrorInvalidValue for arguments the launch refuses. */
int seg_conv_wgrad_geometry(long M, int Cout, int Cin, int ks, int splits, int bf16, int* out3);
int seg_conv_wgrad(const float* dy, long lddy, const float* x, long ldx,
                   int N, int H, int W, int Cin, int Ho, int Wo, int Cout,
                   int ks, int stride, int pad, float* part, int splits, hipStream_t stream);

/* seg_conv_wgrad with bf16 math: dY and X rounded to bf16 (RNE) in the LDS staging,
 * fp32 accumulation into the same fp32 partial slabs (seg_conv_wgrad_reduce). */
int seg_conv_wgrad_bf16(const float* dy, long lddy, const float* x, long ldx,
                        int N, int H, int W, int Cin, int Ho, int Wo, int Cout,
                        int ks, int stride, int pad, float* part, int splits, hipStream_t stream);

/* Lazy BatchNorm of a 1x1 conv's input (training): the input is the RAW output of a
 * BatchNorm'd producer (a depthwise conv of an inverted residual, torchvision
 * mobilenetv2.py InvertedResidual; the first conv of src/unet.py:113-115's OutConv),
 * and x = act(in * in_scale[c] + in_shift[c]) -- the per-channel BN coefficients of
 * seg_bn_finalize, act SEG_ACT_* -- is formed while the operand is staged in LDS
 * instead of by a separate seg_bn_apply pass.  Bitwise the same as seg_bn_apply
 * followed by the plain conv (bf16 storage: the transformed value is rounded to bf16
 * as seg_bn_apply_bf16io would store it).  ks 1, or ks 3 with Cin >= the K chunk (padding taps
 * stay zero; double_conv's first conv feeding its second); no split-K. */
int seg_conv_igemm_xf(const float* in, long ldin, int N, int H, int W, int Cin,
                      const float* wk, int ldk, const float* bias,
                      float* out, long ldout, int Ho, int Wo, int Cout,
                      int ks, int stride, int pad,
                      const float* add, long ldadd, float* stat, const float* in_scale, const float* in_shift,
                      int in_act, hipStream_t stream);
int seg_conv_igemm_bf16_xf(const float* in, long ldin, int N, int H, int W, int Cin,
                           const float* wk, int ldk, const float* bias,
                           float* out, long ldout, int Ho, int Wo, int Cout,
                           int ks, int stride, int pad,
                           const float* add, long ldadd, float* stat, const float* in_scale, const float* in_shift,
                           int in_act, hipStream_t stream);
int seg_conv_wgrad_xf(const float* dy, long lddy, const float* x, long ldx,
                      int N, int H, int W, int Cin, int Ho, int Wo, int Cout,
                      int ks, int stride, int pad, float* part, int splits,
                      const float* in_scale, const float* in_shift, int in_act, hipStream_t stream);
int seg_conv_wgrad_bf16_xf(const float* dy, long lddy, const float* x, long ldx,
                           int N, int H, int W, int Cin, int Ho, int Wo, int Cout,
                           int ks, int stride, int pad, float* part, int splits,
                           const float* in_scale, const float* in_shift, int in_act, hipStream_t stream);

/* dW (PyTorch layout) = fixed-order sum of partial slabs.  mode 0: igemm
 * partials (K runs of round_up(Cin,4) channels), 1: depthwise partials. */
int seg_conv_wgrad_reduce(const float* part, int splits, float* dw, int Cout, int Cin, int ks,
                          int mode, int accumulate, hipStream_t stream);

/* Winograd F(2x2,3x3) convolution (stride 1, pad 1; H, W even) on the f32 matrix
 * cores: 2.25x fewer MFMA FLOPs than the direct sum for the deep decoder convs
 * (src/unet.py:58,61) where the transforms are cheap; forward (U from
 * seg_pack_batch mode 3) and data gradient (mode 4).  out = conv + bias + add;
 * `work` >= 16 * N*(H/2)*(W/2) * Cout floats; `stat` (optional): BatchNorm
 * partials in seg_conv_igemm's layout with seg_conv_wino_row_tiles tiles of
 * seg_conv_wino_tile_rows() rows.  seg_conv_wino_pick: 1 when the cost model prefers it to seg_conv_igemm, 2 when
 * it prefers seg_conv_wino_fused (below), 0 otherwise. */
int seg_conv_wino_pick(int N, int H, int W, int Cin, int Cout);
int seg_conv_wino_tile_rows(void);  /* pixels per BN row tile of seg_conv_wino */
int seg_conv_wino_row_tiles(int N, int H, int W);
int seg_conv_wino(const float* in, long ldin, int N, int H, int W, int Cin, const float* wk, int ldk,
                  const float* bias, float* out, long ldout, int Cout, const float* add, long ldadd,
                  float* stat, float* work, hipStream_t stream);
/* seg_conv_wino in one launch and no workspace (csrc/wino.hip wino_fused_kernel: the 16 GEMMs and the output
 * transform fused, M kept in registers -- VERDICT r4 item 4).  Same arguments without `work`; the result
 * differs from seg_conv_wino's only by the association of the input transform's adds. */
int seg_conv_wino_fused(const float* in, long ldin, int N, int H, int W, int Cin, const float* wk, int ldk,
                        const float* bias, float* out, long ldout, int Cout, const float* add, long ldadd, float* stat,
                        hipStream_t stream);
/* 1 when seg_conv_wino_fused accepts an input of this shape and row stride (its 32-bit buffer offsets cover the
 * images one block reads); seg_conv_wino_pick assumes ldin = Cin + 64, so a caller with a wider strided view checks
 * this and takes seg_conv_wino otherwise. */
int seg_conv_wino_fused_ok(int N, int H, int W, long ldin);
/* Weight gradient of the same convs by Winograd F(3x3,2x2):
 * dW = G^T [sum_t (A dY_t A^T) .* (B^T X_t B)] G.  seg_conv_wino_wgrad writes
 * fixed-order split-K partial slabs part[splits][16][Cout][Cin] (Cin = the padded
 * input channels, % 4 == 0; splits from seg_conv_wino_wgrad_splits), and
 * seg_conv_wino_wgrad_reduce sums them and writes dW [Cout][Cin_real][3][3].
 * Any splits >= 1 is legal.  Split s sums the 2x2 output tiles [s * kchunk, min(T, (s + 1) * kchunk)) in
 * (n, tile row, tile column) order, T = N * (H/2) * (W/2), kchunk = ceil(T / splits) rounded up to 16 tiles.  The
 * rounding can leave trailing splits with an empty range; such a split writes an all-zero slab, so
 * seg_conv_wino_wgrad_reduce always sums `splits` slabs.  Slab element [xi][co][ci], xi = 4 r + c, is
 * sum_t (A dY_t A^T)[r][c] * (B^T X_t B)[r][c] with the matrices of csrc/wino.hip's header comment.
 * Tile (rows of Cout x columns of Cin) of seg_conv_wino_wgrad's launch:
 *   Cout >= 128:       128x128 if Cin >= 128, else 128x64
 *   64 <= Cout < 128:  64x128 if Cin >= 128, else 64x64
 *   Cout < 64:         32x128
 * Tile (square, Cout x Cin) of seg_conv_wino_wgrad16's launch: 64 if Cin >= 128 and Cout >= 128, else 32.  A split
 * of that kernel addresses its pixel rows with 31-bit byte offsets: where
 * (2 * (ceil(kchunk / (W/2)) + 1) + 2) * W * max(ldx, lddy) * 4 >= 2^31 - 16 the launch is handed to
 * seg_conv_wino_wgrad's kernel, which writes the same slabs.
 * Column tile (output channels per block, 128 tiles each) of the 16 GEMMs of seg_conv_wino:
 *   Cout >= 256 and ceil(Cout / 256) * 2 == ceil(Cout / 128):  256 (8 waves)
 *   otherwise Cout >= 128:  128
 *   Cout < 128:  64
 * seg_conv_wino_fused has one tile (128 tiles x 32 output channels) and requires
 * min(N, 128 / ((H/2) * (W/2)) + 2) * H * W * ldin * 4 < 2^31 - 16 (seg_conv_wino_fused_ok). */
/* The geometry the three launchers use for this shape: out6 = {column tile of seg_conv_wino's GEMM, tile rows BM and
 * columns BN of seg_conv_wino_wgrad, tile of seg_conv_wino_wgrad16, kchunk for `splits` splits, 1 if
 * seg_conv_wino_wgrad16 hands the launch to the per-point kernel with ld = max(ldx, lddy), else 0}.  A host function
 * (the launches take their tile, kchunk and that decision from the same code); hipErrorInvalidValue for arguments
 * the launches refuse (odd H or W, Cin or Cout % 4, ld % 4, splits < 1) and for an empty problem. */
int seg_conv_wino_geometry(int N, int H, int W, int Cin, int Cout, int splits, long ld, int* out6);
int seg_conv_wino_wgrad_pick(int N, int H, int W, int Cin, int Cout);
int seg_conv_wino_wgrad_splits(int N, int H, int W, int Cin, int Cout);
int seg_conv_wino_wgrad(const float* dy, long lddy, const float* x, long ldx, int N, int H, int W, int Cin,
                        int Cout, float* part, int splits, hipStream_t stream);
/* The same slabs as seg_conv_wino_wgrad (same arguments, split boundaries and sums) from blocks that own
 * all 16 transform points of a (Cout, Cin) tile; splits from seg_conv_wino_wgrad16_splits.  Replaces the
 * direct split-K weight gradient of the stride-1 3x3 convs (csrc/wgrad.hip) where
 * seg_conv_wino_wgrad_pick returns 2 (reference: the autograd weight gradient of the dense 3x3
 * nn.Conv2d of src/unet.py:58,61, reached through src/train.py:37 loss.backward()). */
int seg_conv_wino_wgrad16_splits(int N, int H, int W, int Cin, int Cout);
int seg_conv_wino_wgrad16(const float* dy, long lddy, const float* x, long ldx, int N, int H, int W, int Cin,
                          int Cout, float* part, int splits, hipStream_t stream);
/* Above 16 splits the reduce first sums runs of slabs in place: `part` is consumed. */
int seg_conv_wino_wgrad_reduce(float* part, int splits, float* dw, int Cout, int Cin, int Cin_pad,
                               int accumulate, hipStream_t stream);

/* Direct 3x3 conv (stride 1, pad 1) with an LDS halo tile for narrow outputs
 * (Cout <= 96; H % 4 == 0, W % 64 == 0): the 4x64-pixel tile's input halo is
 * loaded once per channel chunk and the 9 taps read it from LDS.  Same packed
 * weights, bias / addend / BN-partials contract as seg_conv_igemm (partials:
 * seg_conv_halo_row_tiles tiles of 256 rows). */
int seg_conv_halo_ok(int N, int H, int W, int Cin, int Cout);
int seg_conv_halo_pick(int N, int H, int W, int Cin, int Cout);
int seg_conv_halo_row_tiles(int N, int H, int W);
int seg_conv_halo(const float* in, long ldin, int N, int H, int W, int Cin, const float* wk, int ldk,
                  const float* bias, float* out, long ldout, int Cout, const float* add, long ldadd,
                  float* stat, hipStream_t stream);

/* Every weight repack of a step in one launch.  `jobs` is a DEVICE array of
 * njobs seg_pack_job (mode 0/1 as seg_pack_conv_weight, mode 2 = depthwise
 * [9][C] as seg_pack_dw_weight with cout = C, modes 3/4 = Winograd filter
 * transforms [16][rows][ldk] for seg_conv_wino's forward / data gradient; mode 0/1 | 16 =
 * the same packs written as bf16 (RNE) into wk for the _w16 GEMM entry points).  One thread
 * per output element; job k owns the launch's blocks [blk0, blk0 + nblk), nblk =
 * ceil(elements / 256), jobs sorted by blk0; nblocks = the total.  Replaces the
 * per-conv packs of the engine's step. */
typedef struct seg_pack_job {
  const float* w;
  float* wk;
  int cout, cin, ks, ldk, mode, kin_pad;
  int blk0, nblk;
} seg_pack_job;
int seg_pack_batch(const void* jobs, int njobs, long nblocks, hipStream_t stream);

/* Depthwise 3x3 (torchvision InvertedResidual dw conv, features[1..17] via
 * src/unet.py:15-19): forward, data gradient, weight-gradient partials.
 * in_scale/in_shift/in_act (both pointers null = off): the producing layer's
 * BatchNorm affine + activation applied to the input on load ("lazy BN"), so
 * the expand conv's activated output need not be materialised; padding stays 0. */
int seg_pack_dw_weight(const float* w, float* wk, int C, hipStream_t stream);
int seg_dw_fwd(const float* in, long ldin, int N, int H, int W, int C,
               const float* in_scale, const float* in_shift, int in_act, const float* wk,
               float* out, long ldout, int Ho, int Wo, int stride, hipStream_t stream);
/* Inference depthwise conv with its BatchNorm folded (seg_bn_fold_batch):
 * out = act(dwconv(in, wk) + bias). */
int seg_dw_fwd_bias_act(const float* in, long ldin, int N, int H, int W, int C, const float* wk,
                        const float* bias, int act, float* out, long ldout, int Ho, int Wo, int stride,
                        hipStream_t stream);
int seg_dw_dgrad(const float* dy, long lddy, int N, int Ho, int Wo, int C, const float* wk,
                 float* dx, long lddx, int H, int W, int stride, int accumulate, hipStream_t stream);
long seg_dw_wgrad_blocks(int N, int Ho, int Wo, int C);
/* The launch geometry of seg_dw_wgrad for this output shape, from the code the launch itself uses: out7 = {TC
 * channel-group lanes per block, gy channel chunks, RG row groups, strips per block, row blocks (==
 * seg_dw_wgrad_blocks), the weight gradient's strip width, the forward / data gradient's strip width}.  Strips are
 * out7[5] consecutive output pixels of one output row in (n, ho, strip) order; row block b sums the strips
 * [b * out7[3], min(nstrips, (b + 1) * out7[3])) into part[b][tap][C], and every launch writes all blocks * 9 * C
 * floats.  A host function; hipErrorInvalidValue, nothing written, for C % 4, non-positive sizes or a null out7. */
int seg_dw_wgrad_geometry(int N, int Ho, int Wo, int C, int* out7);
int seg_dw_wgrad(const float* dy, long lddy, const float* x, long ldx, int N, int H, int W, int C,
                 const float* in_scale, const float* in_shift, int in_act,
                 int Ho, int Wo, int stride, float* part, hipStream_t stream);

/* The NCHW image batch (as the reference's DataLoader delivers it) as NHWC rows of
 * `ld` channels, zero-padded: the Cin = 3 first conv (MobileNetV2 features[0],
 * src/unet.py:15,34; UNet inc, src/unet.py:127) then runs on seg_conv_igemm with
 * K = 9 taps x 4 channels (the 4th weight channel packed as zero). */
int seg_nchw_to_nhwc(const float* x, int N, int C, int H, int W, float* out, int ld, hipStream_t stream);

/* ---- BatchNorm2d + activation (aten native_batch_norm(+_backward), hardtanh,
 *      threshold; src/unet.py:59-63,114-115 and torchvision norms) ----------- */
/* partial-sum workspace (floats) of the channel reductions over [M][C]; the
 * partition depends on M and C (seg_colsum: pass round_up(C, 4)) */
long seg_chan_workspace_floats(long M, int C);
int seg_bn_stats(const float* y, long ldy, long M, int C, const float* gamma, const float* beta,
                 float eps, float momentum, float* running_mean, float* running_var,
                 long long* num_batches_tracked, float* work,
                 float* mean, float* invstd, float* scale, float* shift, hipStream_t stream);
int seg_bn_stats_tiles(const float* part, int ntiles, int tile_rows, long M, int C, const float* gamma,
                       const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                       long long* num_batches_tracked, float* mean, float* invstd, float* scale, float* shift,
                       hipStream_t stream);
/* seg_bn_stats_tiles for many-tile layers: with ntiles > 1024, 16 consecutive tiles are merged per row
 * first (coalesced, into `work`: seg_bn_stats_tiles_work_floats(ntiles, C) floats, 0 below the
 * threshold) and the merged rows are finalized -- the same fp64 fixed-order statistics, regrouped. */
long seg_bn_stats_tiles_work_floats(int ntiles, int C);
int seg_bn_stats_tiles_ws(const float* part, int ntiles, int tile_rows, long M, int C, const float* gamma,
                          const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                          long long* num_batches_tracked, float* mean, float* invstd, float* scale, float* shift,
                          float* work, hipStream_t stream);
int seg_bn_eval_coef(const float* gamma, const float* beta, const float* running_mean,
                     const float* running_var, float eps, int C, float* scale, float* shift,
                     hipStream_t stream);
int seg_bn_apply(const float* y, long ldy, long M, int C, const float* scale, const float* shift,
                 int act, const float* res, long ldres, float* out, long ldout, hipStream_t stream);
int seg_bn_backward(const float* da, long ldda, const float* y, long ldy, long M, int C,
                    const float* gamma, const float* mean, const float* invstd,
                    const float* scale, const float* shift, int act,
                    float* dgamma, float* dbeta, float* work, float* dy, long lddy, hipStream_t stream);
/* The two halves of seg_bn_backward (same arguments and arithmetic), for callers that fuse one of
 * them into a neighbouring kernel:
 * seg_bn_bwd_coef: the reduction -- dgamma, dbeta and coef[3][C] = (gamma*invstd, mean(dz),
 * mean(dz*xhat)*invstd); work >= seg_chan_workspace_floats(M, C) floats.  seg_bn_bwd_apply:
 * dy = coef[0] * (dz - coef[1] - (y - mean) * coef[2]), dz = da * act'(y*scale + shift). */
/* dgamma, dbeta and coef[3][C] (as seg_bn_bwd_coef) from BN-backward tile partials written by a
 * producer's epilogue (seg_conv_igemm_bnout*: part[ntiles][2][C]) over M rows; fixed-order fp64. */
int seg_bn_bwd_finalize_tiles(const float* part, int ntiles, long M, int C, const float* gamma,
                              const float* invstd, float* dgamma, float* dbeta, float* coef, hipStream_t stream);
int seg_bn_bwd_coef(const float* da, long ldda, const float* y, long ldy, long M, int C, const float* gamma,
                    const float* mean, const float* invstd, const float* scale, const float* shift, int act,
                    float* dgamma, float* dbeta, float* work, float* coef, hipStream_t stream);
int seg_bn_bwd_apply(const float* da, long ldda, const float* y, long ldy, long M, int C, const float* mean,
                     const float* scale, const float* shift, int act, const float* coef, float* dy, long lddy,
                     hipStream_t stream);
int seg_bn_eval_backward(const float* da, long ldda, const float* y, long ldy, long M, int C,
                         const float* scale, const float* shift, int act, float* dy, long lddy,
                         hipStream_t stream);
/* Backward through a BatchNorm on frozen (running) statistics, scale / shift from seg_bn_eval_coef, in one pass
 * over da and y: dy = scale * dz, dbeta = sum(dz), dgamma = sum(dz * (y - running_mean)) / sqrt(running_var + eps),
 * dz = da * act'(y*scale + shift).  dgamma == dbeta == NULL: no reduction, the elementwise pass alone
 * (seg_bn_eval_backward's dy); dy == NULL: the affine gradients alone.  work >= seg_chan_workspace_floats(M, C)
 * floats (unused without an affine gradient).  Fixed-order sums: bitwise reproducible, fp32 and bf16io alike. */
int seg_bn_frozen_backward(const float* da, long ldda, const float* y, long ldy, long M, int C,
                           const float* scale, const float* shift, const float* running_mean,
                           const float* running_var, float eps, int act, float* dgamma, float* dbeta,
                           float* work, float* dy, long lddy, hipStream_t stream);
/* conv bias gradient: out[c] (+)= sum_r y[r][c]; work >= seg_chan_workspace_floats(M, round_up(C, 4)) */
int seg_colsum(const float* y, long ldy, long M, int C, float* work, float* out, int accumulate,
               hipStream_t stream);
/* gradient fan-in (residual add of InvertedResidual, skip reuse): out = a (+ b) */
int seg_add(const float* a, long lda, const float* b, long ldb, long M, int C, float* out, long ldout,
            hipStream_t stream);

/* ---- resampling (aten upsample_bilinear2d(+_backward), max_pool2d) ---------- */
/* nn.Upsample(x2, bilinear) of `up` (src/unet.py:97,101; ac = 0) into the concat
 * slice of torch.cat([skip, up]) (src/unet.py:103). */
int seg_upsample_fwd(const float* in, long ldin, int N, int H, int W, int C,
                     float* out, long ldout, int Ho, int Wo, int ac, hipStream_t stream);
/* Gradient of seg_upsample_fwd / seg_upsample_to_nchw, a gather without atomics.  ac = 0 / 1 as in the forward;
 * ac = 2: align_corners=True with the tap weights of the fused losses' own upsample (csrc/loss.hip: the fraction
 * scale * dst - floor from one fma, where ac = 1 rounds the product first as aten's float arithmetic does), i.e. the
 * transpose of the blend the seg_kd_* kernels compute.  At 384 source rows ac = 1 puts up to 1.9e-5 on a tap weight,
 * ac = 2 below 4.3e-6. */
int seg_upsample_bwd(const float* dout, long ldout, int nchw_grad, int N, int Ho, int Wo, int C,
                     float* din, long ldin, int H, int W, int ac, int accumulate, hipStream_t stream);
/* final_upsample (align_corners=True, src/unet.py:30,49): NHWC -> NCHW logits */
int seg_upsample_to_nchw(const float* in, long ldin, int N, int H, int W, int C,
                         float* out, int Ho, int Wo, int ac, hipStream_t stream);
/* nn.MaxPool2d(2) of UNet.down (src/unet.py:85) */
int seg_maxpool2_fwd(const float* in, long ldin, int N, int H, int W, int C,
                     float* out, long ldout, hipStream_t stream);
int seg_maxpool2_bwd(const float* in, long ldin, const float* dout, long lddout, int N, int H, int W,
                     int C, float* din, long lddin, int accumulate, hipStream_t stream);

/* ---- loss (nn.CrossEntropyLoss, main.py:99 / src/train.py:37) fused with the
 *      align_corners=True final upsample (src/unet.py:30,49) -----------------
 * out2 = [loss, #non-ignored pixels, #labels outside [0, C) that are not
 * ignore_index] (3 floats; despite the name).  Out-of-range labels (aten raises
 * "Target out of bounds") make the loss and every gradient NaN; the caller raises
 * when it reads them (seg_amd.engine.check_targets).
 * hipErrorInvalidValue before any launch, for these and the seg_cew_* entry points as for
 * every fused-loss family: C outside [1, 32], ld (ldh) % 4 != 0, ld < C, ldh < C (the kernels
 * read and write round4(C) floats per row), or (_eval) confusion NULL. */
long seg_ce_workspace_floats(long pixels);
int seg_ce_upsample_loss(const float* low, long ld, int N, int H, int W, int C,
                         const long long* labels, int Ho, int Wo, int ignore_index,
                         float* work, float* out2, hipStream_t stream);
int seg_ce_upsample_grad(const float* low, long ld, int N, int H, int W, int C,
                         const long long* labels, int Ho, int Wo, int ignore_index,
                         const float* grad_out, const float* stats, float* dhigh, long ldh,
                         hipStream_t stream);
/* Validation (the reference's disabled block, src/train.py:46-76, plus the metrics a
 * segmenter reports): seg_ce_upsample_loss -- out3 is bitwise what it returns -- and, in
 * the same pass, confusion[label * C + argmax] += 1 for every pixel whose label is neither
 * ignore_index nor outside [0, C).  The argmax runs over the C real classes of the
 * recomputed full-resolution logits; ties go to the lowest class (torch.max).
 * `confusion`: C*C int64 in device memory, ADDED to (zero it once per epoch); NULL is
 * hipErrorInvalidValue.  `work` >= seg_ce_workspace_floats(N*Ho*Wo). */
int seg_ce_upsample_eval(const float* low, long ld, int N, int H, int W, int C,
                         const long long* labels, int Ho, int Wo, int ignore_index,
                         float* work, float* out3, long long* confusion, hipStream_t stream);
/* nn.CrossEntropyLoss(weight=w, label_smoothing=eps, reduction="mean" | "sum") for class-index
 * targets, fused with the same upsample: the weighted / smoothed forms of the three kernels
 * above (same grid, same pixel -> thread mapping, the full-resolution logits never stored).
 * Over the valid pixels V (label neither ignore_index nor outside [0, C)), with z_p the
 * recomputed logits and lse_p = logsumexp(z_p):
 *   nll = sum_p w[y_p] (lse_p - z_p[y_p]),  smooth = sum_p sum_c w[c] (lse_p - z_p[c]),
 *   D = sum_p w[y_p] (mean) | 1 (sum),      loss = ((1 - eps) nll + (eps / C) smooth) / D,
 *   dloss/dz_p[c] = g / D [(1 - eps) w[y_p] (softmax_c - [c == y_p]) + (eps / C) (softmax_c sum_k w[k] - w[c])].
 * class_weight: C floats in device memory, or NULL (all ones).  reduction: 0 = mean, 1 = sum.
 * out4 = [loss, D, #labels outside [0, C) that are not ignore_index, #valid pixels]: the first
 * three slots are out2's, so a caller of the plain entry points reads them unchanged.  Mean
 * reduction with D == 0 gives NaN (0/0, as aten); sum reduction over no valid pixel gives 0; an
 * out-of-range label makes the loss and every gradient NaN.  With class_weight NULL or all
 * ones, eps = 0 and reduction 0, out4[0..2] and dhigh are bitwise the plain entry points' (every
 * rounding of csrc/loss.hip is written out, so all its kernels recompute the same logits).
 * `stats` of _grad is the out4 of _loss / _eval; `work` >= seg_cew_workspace_floats(N*Ho*Wo).
 * hipErrorInvalidValue before any launch: reduction not 0 / 1, label_smoothing outside [0, 1],
 * C outside [1, 32], ld (ldh) % 4 != 0, or (_eval) confusion NULL. */
long seg_cew_workspace_floats(long pixels);
int seg_cew_upsample_loss(const float* low, long ld, int N, int H, int W, int C,
                          const long long* labels, int Ho, int Wo, int ignore_index,
                          const float* class_weight, float label_smoothing, int reduction,
                          float* work, float* out4, hipStream_t stream);
int seg_cew_upsample_grad(const float* low, long ld, int N, int H, int W, int C,
                          const long long* labels, int Ho, int Wo, int ignore_index,
                          const float* class_weight, float label_smoothing,
                          const float* grad_out, const float* stats, float* dhigh, long ldh,
                          hipStream_t stream);
int seg_cew_upsample_eval(const float* low, long ld, int N, int H, int W, int C,
                          const long long* labels, int Ho, int Wo, int ignore_index,
                          const float* class_weight, float label_smoothing, int reduction,
                          float* work, float* out4, long long* confusion, hipStream_t stream);
/* seg_amd.SegLoss: a focal term and a soft Dice term beside cross-entropy, fused with the same
 * upsample (same grid, same pixel -> thread mapping, the full-resolution logits never stored).
 * Over the valid pixels V, with s_p = softmax(z_p), pt_p = s_p[y_p] and w = class_weight (ones
 * when NULL):
 *   F    = sum_p w[y_p] (1 - pt_p)^gamma (-log pt_p) / D,   D = sum_p w[y_p]      (gamma > 0)
 *   F    = seg_cew_*'s mean loss with label_smoothing                             (gamma == 0)
 *   I_c = sum_p s_p[c] [y_p = c],  S_c = sum_p s_p[c],  T_c = sum_p [y_p = c],  U_c = S_c + T_c + dice_smooth
 *   Dice = sum_c m_c (1 - (2 I_c + dice_smooth) / U_c) / max(M, 1),  m_c = [T_c > 0],  M = sum_c m_c
 *   loss = ce F + dice Dice   (a term whose coefficient is 0 is left out)
 *   dloss/dz_p[k] = g / D ce [(1 - eps) w[y] f_p (s_k - [k = y]) + (eps / C) (s_k sum_c w[c] - w[k])]
 *                   + g dice s_k (q_k - sum_c q_c s_c),
 *   f_p = (1 - pt)^gamma - gamma pt (1 - pt)^(gamma - 1) log pt,  q_c = b_c - a_c [c = y],
 *   a_c = m_c 2 / (M U_c),  b_c = m_c (2 I_c + dice_smooth) / (M U_c^2).
 * out6 = [loss, D, #labels outside [0, C) that are not ignore_index, #valid pixels, F, Dice]: the
 * first four slots are out4's.  table: 64 floats in device memory, a_c at [c] and b_c at [32 + c],
 * written by _loss / _eval and read by _grad, whose `stats` is their out6.  No float atomics: two
 * calls on the same inputs agree bitwise.  _eval adds the confusion matrix of seg_ce_upsample_eval.
 * An out-of-range label makes the loss and every gradient NaN.  `work` >=
 * seg_sl_workspace_floats(N*Ho*Wo).  hipErrorInvalidValue before any launch: a negative or
 * non-finite ce, dice or focal_gamma, ce and dice both 0, dice_smooth <= 0, label_smoothing outside
 * [0, 1] or > 0 with focal_gamma > 0, C outside [1, 32], ld (ldh) % 4 != 0 or < C, or (_eval)
 * confusion NULL. */
long seg_sl_workspace_floats(long pixels);
int seg_sl_upsample_loss(const float* low, long ld, int N, int H, int W, int C,
                         const long long* labels, int Ho, int Wo, int ignore_index,
                         const float* class_weight, float label_smoothing, float ce, float dice,
                         float focal_gamma, float dice_smooth, float* work, float* out6, float* table,
                         hipStream_t stream);
int seg_sl_upsample_eval(const float* low, long ld, int N, int H, int W, int C,
                         const long long* labels, int Ho, int Wo, int ignore_index,
                         const float* class_weight, float label_smoothing, float ce, float dice,
                         float focal_gamma, float dice_smooth, float* work, float* out6, float* table,
                         long long* confusion, hipStream_t stream);
int seg_sl_upsample_grad(const float* low, long ld, int N, int H, int W, int C,
                         const long long* labels, int Ho, int Wo, int ignore_index,
                         const float* class_weight, float label_smoothing, float ce, float dice,
                         float focal_gamma, const float* grad_out, const float* stats,
                         const float* table, float* dhigh, long ldh, hipStream_t stream);
/* seg_amd.OhemCELoss: cross-entropy with online hard example mining, fused with the same upsample
 * (the full-resolution logits never stored, no float atomics, no host wait).  Over the valid
 * pixels V, with l_p = lse_p - z_p[y_p] (unweighted), w = class_weight (ones when NULL),
 * tau = loss_thresh = -log(thresh) and k = min(min_kept, |V|):
 *   lambda = the k-th largest l_p over V,   K = {p in V : l_p > tau or l_p >= lambda},
 *   D = sum_K w[y_p],   loss = sum_K w[y_p] l_p / D,
 *   dloss/dz_p[c] = g / D w[y_p] (softmax_c - [c == y_p]) for p in K, exactly 0 elsewhere.
 * A tie group at lambda is kept whole, so K depends on neither the pixel order nor the thread
 * mapping.  lambda is found exactly by a three-level radix select (11 / 10 / 10 bits) over the bit
 * patterns of the l_p, which are >= 0: integer histograms only, a fixed launch sequence, and two
 * calls on the same inputs agree bitwise.
 * out6 = [loss, D, #labels outside [0, C) that are not ignore_index, #valid pixels, #kept pixels,
 * cut = min(tau, lambda)]: the first three slots mean what they mean in seg_cew_*.  No pixel kept
 * (none valid) gives NaN (0/0, as aten); an out-of-range label makes the loss and every gradient
 * NaN.  _eval adds the confusion matrix of seg_ce_upsample_eval, over all valid pixels, not over K.
 * `work` >= seg_ohem_workspace_floats(N*Ho*Wo) floats; its histograms and counters are cleared on
 * the stream by every call.  Its first N*Ho*Wo floats are the per-pixel losses l_p in pixel order
 * (-1 where the label is ignore_index or out of range); _grad reads them and lambda back from the
 * `work` of the _loss / _eval call whose out6 is its `stats`, and never recomputes the keep decision.  On K its rows
 * are what seg_cew_upsample_grad writes for the labels with every pixel outside K ignored.
 * seg_ohem_upsample_grad_bf16io writes the full-resolution gradient as fp32 NCHW [N][C][Ho][Wo] (no `ldh`; follow
 * with seg_upsample_bwd_bf16io(nchw_grad = 1)): the low-resolution gradient then sums unrounded terms, as behind the
 * model's full-resolution logits, where bf16 rows would put 2^-9 on every term.
 * hipErrorInvalidValue before any launch: C outside [1, 32], ld (ldh) % 4 != 0 or < C, min_kept < 1,
 * loss_thresh negative or not finite, N*Ho*Wo >= 2^31, or (_eval) confusion NULL. */
long seg_ohem_workspace_floats(long pixels);
int seg_ohem_upsample_loss(const float* low, long ld, int N, int H, int W, int C,
                           const long long* labels, int Ho, int Wo, int ignore_index,
                           const float* class_weight, float loss_thresh, long min_kept,
                           float* work, float* out6, hipStream_t stream);
int seg_ohem_upsample_eval(const float* low, long ld, int N, int H, int W, int C,
                           const long long* labels, int Ho, int Wo, int ignore_index,
                           const float* class_weight, float loss_thresh, long min_kept,
                           float* work, float* out6, long long* confusion, hipStream_t stream);
int seg_ohem_upsample_grad(const float* low, long ld, int N, int H, int W, int C,
                           const long long* labels, int Ho, int Wo, int ignore_index,
                           const float* class_weight, float loss_thresh, const float* work,
                           const float* grad_out, const float* stats, float* dhigh, long ldh,
                           hipStream_t stream);
/* seg_amd.DistillLoss: pixel-wise knowledge distillation, cross-entropy plus the tempered KL divergence to a
 * teacher's logits, fused with the same upsample (neither model's full-resolution logits are ever stored, no float
 * atomics: two calls on the same inputs agree bitwise).  `teacher`: fp32 NHWC rows [N][Ht][Wt] with leading
 * dimension ldt (a multiple of 4, >= C; pads ignored), upsampled to (Ho, Wo) by the same align_corners=True
 * bilinear as `low`; (Ht, Wt) is independent of (H, W), and with Ht == Ho, Wt == Wo the taps are the pixel itself.
 * Over the valid pixels V and the distilled pixels P (kd_ignored != 0: every pixel, else V), with z_p / u_p the
 * student's / teacher's full-resolution logits, s = softmax(z_p / T), q = softmax(u_p / T), w = class_weight:
 *   CE = sum_V w[y_p] (lse(z_p) - z_p[y_p]) / D,  D = sum_V w[y_p],
 *   KD = T^2 / |P| sum_P sum_c q_c (log q_c - log s_c),   loss = ce CE + kd KD  (ce == 0: CE left out),
 *   dloss/dz_p[c] = g [ce / D w[y_p] (softmax(z_p)_c - [c == y_p]) [p in V] + kd T / |P| (s_c - q_c) [p in P]].
 * q and s come from one device function, so teacher rows that are bit for bit the student's rows at the same
 * resolution give KD exactly 0 and, with ce == 0, an all-zero gradient (fp32 entry points).
 * out6 = [loss, D, #labels outside [0, C) that are not ignore_index, #valid pixels, CE, KD]: the first four slots
 * are seg_cew_*'s out4.  An out-of-range label makes the loss and every gradient NaN; no valid pixel gives a NaN CE
 * (0/0, as aten) and, with kd_ignored == 0, a NaN KD.  `stats` of _grad is the out6 of _loss (D and #valid are read
 * from it); `work` >= seg_kd_workspace_floats(N*Ho*Wo).  In the _bf16io twins `low` and `dhigh` are seg_bf16; the
 * teacher stays fp32.  seg_kd_upsample_grad_bf16io_nchw is the gradient twin with the full-resolution gradient written
 * as fp32 NCHW [N][C][Ho][Wo] (no `ldh`; follow with seg_upsample_bwd_bf16io(nchw_grad = 1)): the low-resolution
 * gradient then sums unrounded terms, as behind the model's full-resolution logits -- what the engine launches, for
 * the reason given at seg_ohem_upsample_grad_bf16io.  hipErrorInvalidValue before any launch: C outside [1, 32],
 * ld / ldt (ldh) % 4 != 0 or < C, Ht or Wt < 1, kd <= 0, ce < 0, temperature <= 0, any of them non-finite, teacher
 * NULL. */
long seg_kd_workspace_floats(long pixels);
int seg_kd_upsample_loss(const float* low, long ld, int N, int H, int W, int C,
                         const float* teacher, long ldt, int Ht, int Wt,
                         const long long* labels, int Ho, int Wo, int ignore_index,
                         const float* class_weight, float ce, float kd, float temperature, int kd_ignored,
                         float* work, float* out6, hipStream_t stream);
int seg_kd_upsample_grad(const float* low, long ld, int N, int H, int W, int C,
                         const float* teacher, long ldt, int Ht, int Wt,
                         const long long* labels, int Ho, int Wo, int ignore_index,
                         const float* class_weight, float ce, float kd, float temperature, int kd_ignored,
                         const float* grad_out, const float* stats, float* dhigh, long ldh, hipStream_t stream);
/* The C real channels of `rows` NHWC rows copied into caller-owned fp32 rows of leading dimension ldo (>= C, % 4;
 * channels C..ldo-1 written as 0), one launch: a model's low-resolution logits as seg_kd_*'s `teacher`
 * (model.forward_low_logits).  The _bf16io twin widens seg_bf16 rows. */
int seg_low_logits_f32(const float* low, long ld, long rows, int C, float* out, long ldo, hipStream_t stream);
/* seg_amd.BinarySegLoss: a one-logit model's sigmoid loss -- binary cross-entropy with pos_weight and a focal
 * exponent, plus soft Dice of the foreground -- fused with the same upsample (the full-resolution logits never
 * stored, no float atomics: two calls on the same inputs agree bitwise).  C must be 1: rows of ld floats (ld % 4 ==
 * 0) whose lane 0 is the logit; the pad lanes are loaded and never used.  Labels t_p are 0, 1 or ignore_index;
 * anything else is out of range.  Over the valid pixels V, with z_p the pixel's upsampled logit (bitwise lane 0 of
 * what the other families recompute), s_p = sigmoid(z_p), pt_p = s_p where t_p = 1 else 1 - s_p, w_p = pos_weight
 * where t_p = 1 else 1:
 *   F    = sum_V w_p (1 - pt_p)^gamma (-log pt_p) / |V|       (the divisor is |V|, not sum w: with gamma = 0 it is
 *          nn.BCEWithLogitsLoss(pos_weight)'s mean)
 *   I = sum_V s_p t_p,  S = sum_V s_p,  T = sum_V t_p,  U = S + T + dice_smooth,  Dice = 1 - (2 I + dice_smooth) / U
 *   loss = bce F + dice Dice   (a term whose coefficient is 0 is left out)
 *   dloss/dz_p = g bce / |V| (t_p ? -1 : 1) w_p (1 - pt)^gamma ((1 - pt) + gamma pt (-log pt))
 *                - g dice (a t_p - b) s_p (1 - s_p),    a = 2 / U,  b = (2 I + dice_smooth) / U^2.
 * -log sigmoid(x) is max(-x, 0) + log1p(exp(-|x|)) and sigmoid comes from exp(-|x|): every value is finite for any
 * finite logit, and (1 - pt)^gamma is exactly 0 where 1 - pt rounds to 0.
 * stats8 = [loss, #valid pixels, #labels outside {0, 1} that are not ignore_index, #valid pixels, F, Dice, a, b]: the
 * first four slots are seg_cew_*'s out4 (D = #valid); a and b are written by _loss / _eval and read by _grad, whose
 * `stats8` is theirs.  No valid pixel gives a NaN F (0/0, as aten); an out-of-range label is counted, put in no bin,
 * and makes the loss and every gradient NaN.  `work` >= seg_bce_workspace_floats(N*Ho*Wo).
 * _eval: the same loss and stats, bitwise, and confusion[t_p * 2 + (z_p > zthr)] += 1 for every valid pixel (int64
 * [2][2] in device memory, added to; 64-bit integer atomics).  zthr = log(threshold / (1 - threshold)); the comparison
 * is strict, so a tie or a NaN logit is background -- "first maximum wins" for the two-class view [0, z].
 * _grad: dhigh is fp32 [N][Ho][Wo], ONE float per pixel and no `ldh`, in the _bf16io twins too (their `low` is
 * seg_bf16): at C = 1 this is the NCHW plane seg_upsample_bwd(nchw_grad = 1, ac = 2) reads, it costs 4 B a pixel where
 * a round4(C) row costs 16, and the low-resolution gradient sums unrounded terms (the reason given at
 * seg_ohem_upsample_grad_bf16io).  Exactly 0 on ignored pixels.
 * hipErrorInvalidValue before any launch: C != 1, ld % 4 != 0, pos_weight <= 0, a negative bce, dice or focal_gamma,
 * bce and dice both 0, dice_smooth <= 0, any of them non-finite, or (_eval) confusion NULL. */
long seg_bce_workspace_floats(long pixels);
int seg_bce_upsample_loss(const float* low, long ld, int N, int H, int W, int C,
                          const long long* labels, int Ho, int Wo, int ignore_index,
                          float pos_weight, float bce, float dice, float focal_gamma, float dice_smooth,
                          float* work, float* stats8, hipStream_t stream);
int seg_bce_upsample_eval(const float* low, long ld, int N, int H, int W, int C,
                          const long long* labels, int Ho, int Wo, int ignore_index,
                          float pos_weight, float bce, float dice, float focal_gamma, float dice_smooth,
                          float* work, float* stats8, float zthr, long long* confusion, hipStream_t stream);
int seg_bce_upsample_grad(const float* low, long ld, int N, int H, int W, int C,
                          const long long* labels, int Ho, int Wo, int ignore_index,
                          float pos_weight, float bce, float dice, float focal_gamma,
                          const float* grad_out, const float* stats8, float* dhigh, hipStream_t stream);

/* ---- inference (inference.py: preprocess_image :28-46, model.eval() forward
 *      :23-25,162-163, overlay_predictions' argmax + resize :64-70) ---------- */
/* Fold eval-mode BatchNorm2d into the preceding conv, all layers in one launch:
 * w' = w * g/sqrt(rv+eps), b' = b * g/sqrt(rv+eps) + beta - rm * g/sqrt(rv+eps)
 * (gamma == NULL: plain copy).  `jobs` is a DEVICE array of seg_fold_job;
 * max_elems = the largest cout*kper + cout. */
typedef struct seg_fold_job {
  const float *w, *bias, *gamma, *beta, *running_mean, *running_var;
  float *w_out, *b_out;
  int cout, kper;
  float eps;
  int pad_;
} seg_fold_job;
int seg_bn_fold_batch(const void* jobs, int njobs, long max_elems, hipStream_t stream);
/* cv2.resize(frame, (W, H)) (INTER_LINEAR, uint8) -> cvtColor(BGR2RGB) ->
 * ToTensor -> Normalize(mean, std), fused: N uint8 BGR frames [N][Hf][row_bytes]
 * -> NHWC rows out[N*H*W][ld] (ld >= 4, channel 3 zeroed). */
int seg_preprocess_bgr(const unsigned char* frame, int N, int Hf, int Wf, long row_bytes, float* out, int ld,
                       int H, int W, float mean_r, float mean_g, float mean_b, float std_r, float std_g,
                       float std_b, hipStream_t stream);
/* uint8 class mask [N][Hf][Wf]: torch.max(dim=1) of the model's logits (the
 * align_corners=True x(Hm/H) upsample of the low-res NHWC logits, src/unet.py:49)
 * resized to the frame with cv2 INTER_NEAREST.  First maximum wins. */
int seg_argmax_nearest(const float* low, long ld, int N, int H, int W, int C, int Hm, int Wm,
                       unsigned char* mask, int Hf, int Wf, hipStream_t stream);
/* seg_argmax_nearest for a one-logit model (rows of ld floats, ld % 4 == 0, lane 0 the logit): mask = 1 where the
 * upsampled logit of the nearest model pixel is > zthr = log(threshold / (1 - threshold)), else 0.  Strict: a tie or
 * a NaN logit gives 0.  hipErrorInvalidValue for ld % 4 != 0, a non-positive size or a NaN zthr. */
int seg_threshold_nearest(const float* low, long ld, int N, int H, int W, int Hm, int Wm, float zthr,
                          unsigned char* mask, int Hf, int Wf, hipStream_t stream);
/* seg_argmax_nearest for video: the class of the exponential moving average over the frames of the
 * per-pixel class probabilities.  Per model pixel (Hm x Wm), in fp32: z = its upsampled logits (as
 * seg_upsample_to_nchw forms them), p = softmax(z); s = p when *fresh != 0 (or alpha == 1), else
 * s += alpha (p - s); class = the first maximum of s, or fallback_class when that maximum < min_conf;
 * mask = cv2 INTER_NEAREST of the classes to Hf x Wf.  A pixel with a non-finite z (a NaN or +-Inf logit
 * among its four taps) keeps s (1/C when *fresh != 0) and is classified from it, so one bad frame does not
 * stay in the average.
 *   state  [N*Hm*Wm][lds] fp32, lds >= C, lds % 4 == 0, 16-byte aligned: s, read and written once per call
 *          (lanes C..lds-1 need no initial value; those of the written quads become 0);
 *   fresh  one device word: read by the first launch, set to 0 by the second -- the caller sets it (a
 *          stream-ordered write) to start a new average: first frame, scene cut, seek;
 *   labels [N][Hm][Wm] scratch: the classes at model resolution.
 * alpha in (0, 1] (the weight of the newest frame), min_conf in [0, 1], fallback_class in [0, C), C in
 * 1..255.  Two launches, no atomics: the same values eagerly and in a replayed graph. */
int seg_temporal_argmax_nearest(const float* low, long ld, int N, int H, int W, int C, int Hm, int Wm,
                                float* state, int lds, int* fresh, float alpha, float min_conf,
                                int fallback_class, unsigned char* labels, unsigned char* mask, int Hf, int Wf,
                                hipStream_t stream);

/* ---- test-time augmentation: flip / multi-scale ensembles (csrc/tta.h, tta.hip, infer.hip) ----
 * A view is a forward of a resized and / or mirrored copy of the same images.  Its low-resolution NHWC
 * logits `low` [N][H][W][ld] (image n at low + n*H*W*ld; pad lanes C..ld-1 never used; 16-byte aligned,
 * ld % 4 == 0, ld >= C) map onto the model's Ho x Wo output grid as the model's final align_corners=True
 * upsample maps them (source coordinate and tap index in fp32: one interpolation, whatever the view's
 * size); a mirrored view (flip != 0) is read at x_v = Wo - 1 - x.  Per output pixel, in fp32:
 *   z_v = the blend of the view's four taps,  p = sum_v w_v * softmax(z_v),  class = first maximum of p,
 * with w_v = weight_v / sum of the weights (every weight positive and finite).  The entry points take a
 * HOST array of 1..SEG_TTA_MAX_VIEWS descriptors and pass it to their kernels by value: no device
 * allocation, no copy, capturable in a graph.  Anything else: hipErrorInvalidValue before any launch. */
#define SEG_TTA_MAX_VIEWS 8
typedef struct seg_tta_view {
  const float* low;
  long ld;
  int H, W;
  int flip;
  float weight;
} seg_tta_view;
/* out [N][C][Hv][Wv] = flip(F.interpolate(x [N][C][H][W], (Hv, Wv), mode="bilinear", align_corners=False),
 * -1) when flip != 0, the resize alone otherwise (fp32 NCHW; a view of x's own size is a copy / mirror). */
int seg_tta_view_nchw(const float* x, int N, int C, int H, int W, float* out, int Hv, int Wv, int flip,
                      hipStream_t stream);
/* seg_preprocess_bgr of ONE frame into `copies` (1..8) images out[copies*H*W][ld]: image i is mirrored
 * left-right when bit i of flip_mask is set, its pixel (y, x) bitwise seg_preprocess_bgr's at (y, W-1-x). */
int seg_preprocess_bgr_views(const unsigned char* frame, int Hf, int Wf, long row_bytes, float* out, int ld,
                             int H, int W, int copies, int flip_mask, float mean_r, float mean_g, float mean_b,
                             float std_r, float std_g, float std_b, hipStream_t stream);
/* The ensemble's validation step in one kernel (+ a finalize): loss = nn.NLLLoss(class_weight, ignore_index,
 * reduction)(log p, labels) and confusion[label * C + class] += 1 for every valid pixel.  views: const
 * seg_tta_view[nviews]; labels int64 [N][Ho][Wo]; class_weight C device floats or NULL; reduction 0 = mean,
 * 1 = sum; work >= seg_tta_workspace_floats(N*Ho*Wo) floats; out4 = [loss, D, #out-of-range labels, #valid
 * pixels] as seg_cew_upsample_eval's (an out-of-range label makes the loss NaN); confusion int64 [C][C], added
 * to; prob NULL or fp32 [N][C][Ho][Wo], which receives p at every pixel.  C in 1..32.  labels == NULL (prob given):
 * probabilities only -- every pixel counts as ignored and confusion may be NULL too.  A non-finite logit
 * gets no special case: the loss becomes non-finite and the pixel is binned under some class in [0, C).
 * Per-block partials and a fixed-order finalize, integer atomics for the matrix: two runs are bitwise equal. */
long seg_tta_workspace_floats(long pixels);
int seg_tta_upsample_eval(const void* views, int nviews, int N, int C, const long long* labels, int Ho, int Wo,
                          int ignore_index, const float* class_weight, int reduction, float* work, float* out4,
                          long long* confusion, float* prob, hipStream_t stream);
/* seg_argmax_nearest on the ensemble: state [N*Hm*Wm][lds] (seg_temporal_argmax_nearest's layout; pad lanes of
 * the written quads 0) receives p, labels [N][Hm][Wm] its classes -- fallback_class where the largest p <
 * min_conf -- and mask [N][Hf][Wf] their cv2 INTER_NEAREST.  A view whose z_v is non-finite at a pixel is left
 * out there and the remaining weights are renormalised; none left: p = 1/C.  C in 1..255.  Two launches, no
 * atomics: the same values eagerly and in a replayed graph. */
int seg_tta_argmax_nearest(const void* views, int nviews, int N, int C, int Hm, int Wm, float* state, int lds,
                           float min_conf, int fallback_class, unsigned char* labels, unsigned char* mask, int Hf,
                           int Wf, hipStream_t stream);

/* ---- GPU augmentation (the readers' albumentations pipeline,
 *      src/BDD100KDataset.py:38-52) ---------------------- */
/* Resize a batch [N][Hs][src_row] of uint8 images (C = 3: cv2 INTER_LINEAR 8-bit)
 * or class masks (C = 1: INTER_NEAREST, then lut[v] if lut != NULL) to [N][H][W][C]. */
int seg_resize_u8(const unsigned char* src, int N, int Hs, int Ws, long src_row, unsigned char* dst, int H,
                  int W, int C, const unsigned char* lut, hipStream_t stream);
/* Per-sample flip + ShiftScaleRotate (inverse affine, BORDER_REFLECT_101) +
 * brightness/contrast + Normalize + ToTensorV2: img [N][H][W][3] u8, mask
 * [N][H][W] u8 -> x [N][3][H][W] f32, y [N][H][W] int64.  params: DEVICE array of
 * seg_aug_param; mean255/rstd255: 255*mean and 1/(255*std) per channel. */
typedef struct seg_aug_param {
  float m[6];
  float alpha, beta;
  int flip, warp, bc, pad_;
} seg_aug_param;
int seg_augment(const unsigned char* img, const unsigned char* mask, int N, int H, int W, const void* params,
                float mean_r, float mean_g, float mean_b, float rstd_r, float rstd_g, float rstd_b, float* x,
                long long* y, hipStream_t stream);


/* ---------------------------------------------------------------- bf16 storage
 * `_bf16io` entry points: the same operations as their fp32 namesakes (same argument
 * meaning, strides in elements) on bf16 activation / gradient tensors -- the storage of
 * the "bf16io" configuration (engine math "bf16io": bf16 conv operands AND bf16
 * tensors between kernels).  Arithmetic inside every kernel stays fp32: loads widen
 * bf16 -> fp32, stores round fp32 -> bf16 (round-to-nearest-even); BatchNorm
 * statistics, reduction partials, coefficients, weights and parameter gradients stay
 * fp32.  seg_bf16 = the raw 16-bit bf16 pattern. */
typedef uint16_t seg_bf16;
int seg_add_bf16io(const seg_bf16* a, long lda, const seg_bf16* b, long ldb, long M, int C, seg_bf16* out, long ldout,
    hipStream_t stream);
int seg_bn_stats_bf16io(const seg_bf16* y, long ldy, long M, int C, const float* gamma, const float* beta, float eps,
    float momentum, float* running_mean, float* running_var, long long* num_batches_tracked, float* work, float* mean,
    float* invstd, float* scale, float* shift, hipStream_t stream);
int seg_bn_apply_bf16io(const seg_bf16* y, long ldy, long M, int C, const float* scale, const float* shift, int act,
    const seg_bf16* res, long ldres, seg_bf16* out, long ldout, hipStream_t stream);
int seg_bn_backward_bf16io(const seg_bf16* da, long ldda, const seg_bf16* y, long ldy, long M, int C, const float*
    gamma, const float* mean, const float* invstd, const float* scale, const float* shift, int act, float* dgamma,
    float* dbeta, float* work, seg_bf16* dy, long lddy, hipStream_t stream);
int seg_bn_frozen_backward_bf16io(const seg_bf16* da, long ldda, const seg_bf16* y, long ldy, long M, int C,
    const float* scale, const float* shift, const float* running_mean, const float* running_var, float eps, int act,
    float* dgamma, float* dbeta, float* work, seg_bf16* dy, long lddy, hipStream_t stream);
int seg_colsum_bf16io(const seg_bf16* y, long ldy, long M, int C, float* work, float* out, int accumulate, hipStream_t
    stream);
int seg_dw_fwd_bf16io(const seg_bf16* in, long ldin, int N, int H, int W, int C, const float* in_scale, const float*
    in_shift, int in_act, const float* wk, seg_bf16* out, long ldout, int Ho, int Wo, int stride, hipStream_t stream);
int seg_dw_dgrad_bf16io(const seg_bf16* dy, long lddy, int N, int Ho, int Wo, int C, const float* wk, seg_bf16* dx,
    long lddx, int H, int W, int stride, int accumulate, hipStream_t stream);
int seg_conv_igemm_bnout_bf16io(const seg_bf16* in, long ldin, int N, int H, int W, int Cin, const float* wk,
                                int ldk, seg_bf16* out, long ldout, int Cout, int ks, const seg_bf16* add,
                                long ldadd, const seg_bf16* by, long ldby, const float* bscale,
                                const float* bshift, const float* bmean, int bact, float* bpart,
                                hipStream_t stream);
int seg_conv_igemm_bnout_bf16io_w16(const seg_bf16* in, long ldin, int N, int H, int W, int Cin,
                                    const seg_bf16* wk, int ldk, seg_bf16* out, long ldout, int Cout, int ks,
                                    const seg_bf16* add, long ldadd, const seg_bf16* by, long ldby,
                                    const float* bscale, const float* bshift, const float* bmean, int bact,
                                    float* bpart, hipStream_t stream);
int seg_bn_bwd_coef_bf16io(const seg_bf16* da, long ldda, const seg_bf16* y, long ldy, long M, int C,
                           const float* gamma, const float* mean, const float* invstd, const float* scale,
                           const float* shift, int act, float* dgamma, float* dbeta, float* work, float* coef,
                           hipStream_t stream);
int seg_bn_bwd_apply_bf16io(const seg_bf16* da, long ldda, const seg_bf16* y, long ldy, long M, int C,
                            const float* mean, const float* scale, const float* shift, int act, const float* coef,
                            seg_bf16* dy, long lddy, hipStream_t stream);
int seg_dw_wgrad_bf16io(const seg_bf16* dy, long lddy, const seg_bf16* x, long ldx, int N, int H, int W, int C, const
    float* in_scale, const float* in_shift, int in_act, int Ho, int Wo, int stride, float* part, hipStream_t stream);
int seg_conv_igemm_bf16io(const seg_bf16* in, long ldin, int N, int H, int W, int Cin, const float* wk, int ldk, const
    float* bias, seg_bf16* out, long ldout, int Ho, int Wo, int Cout, int ks, int stride, int pad, const seg_bf16*
    add, long ldadd, float* stat, hipStream_t stream);
int seg_ce_upsample_loss_bf16io(const seg_bf16* low, long ld, int N, int H, int W, int C, const long long* labels, int
    Ho, int Wo, int ignore_index, float* work, float* out2, hipStream_t stream);
int seg_ce_upsample_eval_bf16io(const seg_bf16* low, long ld, int N, int H, int W, int C, const long long* labels, int
    Ho, int Wo, int ignore_index, float* work, float* out3, long long* confusion, hipStream_t stream);
int seg_ce_upsample_grad_bf16io(const seg_bf16* low, long ld, int N, int H, int W, int C, const long long* labels, int
    Ho, int Wo, int ignore_index, const float* grad_out, const float* stats, seg_bf16* dhigh, long ldh, hipStream_t
    stream);
int seg_cew_upsample_loss_bf16io(const seg_bf16* low, long ld, int N, int H, int W, int C, const long long* labels, int
    Ho, int Wo, int ignore_index, const float* class_weight, float label_smoothing, int reduction, float* work, float*
    out4, hipStream_t stream);
int seg_cew_upsample_eval_bf16io(const seg_bf16* low, long ld, int N, int H, int W, int C, const long long* labels, int
    Ho, int Wo, int ignore_index, const float* class_weight, float label_smoothing, int reduction, float* work, float*
    out4, long long* confusion, hipStream_t stream);
int seg_cew_upsample_grad_bf16io(const seg_bf16* low, long ld, int N, int H, int W, int C, const long long* labels, int
    Ho, int Wo, int ignore_index, const float* class_weight, float label_smoothing, const float* grad_out, const float*
    stats, seg_bf16* dhigh, long ldh, hipStream_t stream);
int seg_sl_upsample_loss_bf16io(const seg_bf16* low, long ld, int N, int H, int W, int C, const long long* labels, int
    Ho, int Wo, int ignore_index, const float* class_weight, float label_smoothing, float ce, float dice, float
    focal_gamma, float dice_smooth, float* work, float* out6, float* table, hipStream_t stream);
int seg_sl_upsample_eval_bf16io(const seg_bf16* low, long ld, int N, int H, int W, int C, const long long* labels, int
    Ho, int Wo, int ignore_index, const float* class_weight, float label_smoothing, float ce, float dice, float
    focal_gamma, float dice_smooth, float* work, float* out6, float* table, long long* confusion, hipStream_t stream);
int seg_sl_upsample_grad_bf16io(const seg_bf16* low, long ld, int N, int H, int W, int C, const long long* labels, int
    Ho, int Wo, int ignore_index, const float* class_weight, float label_smoothing, float ce, float dice, float
    focal_gamma, const float* grad_out, const float* stats, const float* table, seg_bf16* dhigh, long ldh, hipStream_t
    stream);
int seg_ohem_upsample_loss_bf16io(const seg_bf16* low, long ld, int N, int H, int W, int C, const long long* labels,
    int Ho, int Wo, int ignore_index, const float* class_weight, float loss_thresh, long min_kept, float* work, float*
    out6, hipStream_t stream);
int seg_ohem_upsample_eval_bf16io(const seg_bf16* low, long ld, int N, int H, int W, int C, const long long* labels,
    int Ho, int Wo, int ignore_index, const float* class_weight, float loss_thresh, long min_kept, float* work, float*
    out6, long long* confusion, hipStream_t stream);
int seg_ohem_upsample_grad_bf16io(const seg_bf16* low, long ld, int N, int H, int W, int C, const long long* labels,
    int Ho, int Wo, int ignore_index, const float* class_weight, float loss_thresh, const float* work, const float*
    grad_out, const float* stats, float* dhigh_nchw, hipStream_t stream);
int seg_kd_upsample_loss_bf16io(const seg_bf16* low, long ld, int N, int H, int W, int C, const float* teacher, long
    ldt, int Ht, int Wt, const long long* labels, int Ho, int Wo, int ignore_index, const float* class_weight, float ce,
    float kd, float temperature, int kd_ignored, float* work, float* out6, hipStream_t stream);
int seg_kd_upsample_grad_bf16io(const seg_bf16* low, long ld, int N, int H, int W, int C, const float* teacher, long
    ldt, int Ht, int Wt, const long long* labels, int Ho, int Wo, int ignore_index, const float* class_weight, float ce,
    float kd, float temperature, int kd_ignored, const float* grad_out, const float* stats, seg_bf16* dhigh, long ldh,
    hipStream_t stream);
int seg_kd_upsample_grad_bf16io_nchw(const seg_bf16* low, long ld, int N, int H, int W, int C, const float* teacher,
    long ldt, int Ht, int Wt, const long long* labels, int Ho, int Wo, int ignore_index, const float* class_weight,
    float ce, float kd, float temperature, int kd_ignored, const float* grad_out, const float* stats, float*
    dhigh_nchw, hipStream_t stream);
int seg_low_logits_f32_bf16io(const seg_bf16* low, long ld, long rows, int C, float* out, long ldo, hipStream_t
    stream);
int seg_bce_upsample_loss_bf16io(const seg_bf16* low, long ld, int N, int H, int W, int C, const long long* labels, int
    Ho, int Wo, int ignore_index, float pos_weight, float bce, float dice, float focal_gamma, float dice_smooth, float*
    work, float* stats8, hipStream_t stream);
int seg_bce_upsample_eval_bf16io(const seg_bf16* low, long ld, int N, int H, int W, int C, const long long* labels, int
    Ho, int Wo, int ignore_index, float pos_weight, float bce, float dice, float focal_gamma, float dice_smooth, float*
    work, float* stats8, float zthr, long long* confusion, hipStream_t stream);
int seg_bce_upsample_grad_bf16io(const seg_bf16* low, long ld, int N, int H, int W, int C, const long long* labels, int
    Ho, int Wo, int ignore_index, float pos_weight, float bce, float dice, float focal_gamma, const float* grad_out,
    const float* stats8, float* dhigh, hipStream_t stream);
int seg_upsample_fwd_bf16io(const seg_bf16* in, long ldin, int N, int H, int W, int C, seg_bf16* out, long ldout, int
    Ho, int Wo, int ac, hipStream_t stream);
int seg_upsample_bwd_bf16io(const void* dout, long ldout, int nchw_grad, int N, int Ho, int Wo, int C, seg_bf16* din,
    long ldin, int H, int W, int ac, int accumulate, hipStream_t stream);
int seg_upsample_to_nchw_bf16io(const seg_bf16* in, long ldin, int N, int H, int W, int C, float* out, int Ho, int Wo,
    int ac, hipStream_t stream);
int seg_nchw_to_nhwc_bf16io(const float* x, int N, int C, int H, int W, seg_bf16* out, int ld, hipStream_t stream);
int seg_maxpool2_fwd_bf16io(const seg_bf16* in, long ldin, int N, int H, int W, int C, seg_bf16* out, long ldout,
    hipStream_t stream);
int seg_maxpool2_bwd_bf16io(const seg_bf16* in, long ldin, const seg_bf16* dout, long lddout, int N, int H, int W, int
    C, seg_bf16* din, long lddin, int accumulate, hipStream_t stream);
/* seg_conv_igemm_bf16io / _xf with the weights packed as bf16 (seg_pack_batch mode | 16):
 * [Cout][ldk] bf16, ldk % 8 == 0, 16-byte aligned, zero beyond K.  Bitwise the fp32-weight
 * launch (the same RNE rounding, done once at pack time); half the weight bytes. */
int seg_conv_pw_bf16io(const seg_bf16* in, long ldin, long M, int K, const seg_bf16* wk, int ldk, const float* bias,
    seg_bf16* out, long ldout, int N, const seg_bf16* add, long ldadd, float* stat, const float* in_scale, const float*
    in_shift, int in_act, hipStream_t stream);
int seg_conv_igemm_bf16io_w16(const seg_bf16* in, long ldin, int N, int H, int W, int Cin, const seg_bf16* wk,
    int ldk, const float* bias, seg_bf16* out, long ldout, int Ho, int Wo, int Cout, int ks, int stride, int pad,
    const seg_bf16* add, long ldadd, float* stat, hipStream_t stream);
int seg_conv_igemm_bf16io_xf_w16(const seg_bf16* in, long ldin, int N, int H, int W, int Cin, const seg_bf16* wk,
    int ldk, const float* bias, seg_bf16* out, long ldout, int Ho, int Wo, int Cout, int ks, int stride, int pad,
    const seg_bf16* add, long ldadd, float* stat, const float* in_scale, const float* in_shift, int in_act,
    hipStream_t stream);
/* seg_conv_halo_bf16io with bf16-packed weights (mode | 16, ldk % 8 == 0): bitwise the same. */
int seg_conv_halo_bf16io_w16(const seg_bf16* in, long ldin, int N, int H, int W, int Cin, const seg_bf16* wk,
    int ldk, const float* bias, seg_bf16* out, long ldout, int Cout, const seg_bf16* add, long ldadd, float* stat,
    hipStream_t stream);
int seg_conv_halo_bf16io(const seg_bf16* in, long ldin, int N, int H, int W, int Cin, const float* wk, int ldk,
    const float* bias, seg_bf16* out, long ldout, int Cout, const seg_bf16* add, long ldadd, float* stat,
    hipStream_t stream);
int seg_conv_wgrad_bf16io(const seg_bf16* dy, long lddy, const seg_bf16* x, long ldx, int N, int H, int W, int Cin,
    int Ho, int Wo, int Cout, int ks, int stride, int pad, float* part, int splits, hipStream_t stream);
/* bf16-storage twins of seg_conv_igemm_xf / seg_conv_wgrad_xf. */
int seg_conv_igemm_bf16io_xf(const seg_bf16* in, long ldin, int N, int H, int W, int Cin, const float* wk, int ldk,
    const float* bias, seg_bf16* out, long ldout, int Ho, int Wo, int Cout, int ks, int stride, int pad,
    const seg_bf16* add, long ldadd, float* stat, const float* in_scale, const float* in_shift, int in_act,
    hipStream_t stream);
int seg_conv_wgrad_bf16io_xf(const seg_bf16* dy, long lddy, const seg_bf16* x, long ldx, int N, int H, int W,
    int Cin, int Ho, int Wo, int Cout, int ks, int stride, int pad, float* part, int splits, const float* in_scale,
    const float* in_shift, int in_act, hipStream_t stream);

/* ---- Adam (optim.Adam(model.parameters(), lr=1.5e-4), main.py:100; step at
 *      src/train.py:39): one launch over every parameter with a gradient, the
 *      foreach implementation's fp32 arithmetic per element ------------------- */
typedef struct SegAdamTensor {
  float* p;
  const float* g;
  float* m;          /* exp_avg */
  float* v;          /* exp_avg_sq */
  long n;
  float step_size;   /* -lr / (1 - beta1^t) */
  float bc2_sqrt;    /* sqrt(1 - beta2^t) */
} SegAdamTensor;
/* tensors: device array; chunks: device array of nchunks (tensor index, first
 * element) int64 pairs covering every tensor in pieces of <= chunk elements */
int seg_adam_step(const SegAdamTensor* tensors, const long* chunks, int nchunks, int chunk,
                  float one_minus_beta1, float beta2, float one_minus_beta2, float eps, hipStream_t stream);
/* seg_adam_step, skipped on the device when *skip != 0 (skip: a device float, e.g. the out-of-range label count
 * of the batch, summed or averaged over ranks; NULL = never): train_one_epoch queues the step without waiting
 * for the label check (nn.CrossEntropyLoss raises before any update, src/train.py:37), and raises after
 * loss.item() (src/train.py:41). */
int seg_adam_step_skip(const SegAdamTensor* tensors, const long* chunks, int nchunks, int chunk,
                       float one_minus_beta1, float beta2, float one_minus_beta2, float eps, const float* skip,
                       hipStream_t stream);

/* ---- AdamW and global-norm gradient clipping over the same chunk map ----------
 * The tensor table of these entry points is a device array of 56-byte records,
 * passed as const void*:
 *   struct SegAdamWTensor {
 *     float* p; const float* g; float* m; float* v;   exp_avg, exp_avg_sq as above
 *     long n;
 *     float step_size;   -lr / (1 - beta1^t)
 *     float bc2_sqrt;    sqrt(1 - beta2^t)
 *     float decay;       (float)(1 - lr * weight_decay), formed in double
 *     float pad;
 *   };
 * seg_grad_sumsq and seg_grad_scale read only g and n of each record. */
/* torch's foreach AdamW (decoupled_weight_decay) per element, fp32, in its order:
 *   g *= *grad_scale; p *= decay; then the Adam arithmetic of seg_adam_step.
 * Both products are rounded on their own, so decay == 1 with grad_scale == NULL is
 * bit for bit seg_adam_step_skip, and a grad_scale is bit for bit seg_grad_scale
 * followed by the unscaled step.  skip: as seg_adam_step_skip.  grad_scale: one
 * device float (NULL = 1), e.g. out + 1 of seg_grad_sumsq; .grad is not written. */
int seg_adamw_step(const void* tensors, const long* chunks, int nchunks, int chunk,
                   float one_minus_beta1, float beta2, float one_minus_beta2, float eps, const float* skip,
                   const float* grad_scale, hipStream_t stream);
/* floats of workspace seg_grad_sumsq needs for nchunks chunks */
long seg_grad_norm_workspace_floats(int nchunks);
/* Global L2 norm of every gradient in the table: one partial sum of squares per
 * chunk into `work`, then a one-block launch that adds the partials in a fixed
 * order (no atomics: bitwise the same on every run) and writes
 *   out[0] = norm,
 *   out[1] = min(max_norm / (norm + 1e-6), 1)  (torch.nn.utils.clip_grad_norm_'s
 *            coefficient; NaN for a NaN norm; 1 when max_norm <= 0 or infinite),
 *   out[2] = 1 if the norm is inf or NaN, else 0. */
int seg_grad_sumsq(const void* tensors, const long* chunks, int nchunks, int chunk, float max_norm,
                   float* work, float* out, hipStream_t stream);
/* g *= *scale in place (scale: one device float); when *scale == 1 the kernel
 * returns without touching memory.  For optimizers without a fused grad_scale. */
int seg_grad_scale(const void* tensors, const long* chunks, int nchunks, int chunk, const float* scale,
                   hipStream_t stream);

/* ---- weight averaging (seg_amd/ema.py) over a chunk map of the same kind ------
 * The tensor table is a device array of 24-byte records, passed as const void*:
 *   struct SegEmaTensor {
 *     float* ema;   the shadow (the average)
 *     float* p;     its source: a parameter or a BatchNorm running statistic
 *     long n;
 *   };
 * nchunks < 0 or chunk < 1: hipErrorInvalidValue; nchunks == 0: success, no launch. */
/* ema = ema + one_minus_decay * (p - ema) per element in fp32 (torch.lerp's
 * weight < 0.5 form, for every weight in [0, 1]); one_minus_decay is
 * (float)(1 - decay) formed in double.  p is only read.  skip: as
 * seg_adam_step_skip -- when *skip != 0 the kernel returns without touching memory. */
int seg_ema_update(const void* tensors, const long* chunks, int nchunks, int chunk, float one_minus_decay,
                   const float* skip, hipStream_t stream);
/* ema[i] <-> p[i]: each element read and written by the same lane, no temporary in
 * memory; a second call restores both sides bit for bit. */
int seg_ema_swap(const void* tensors, const long* chunks, int nchunks, int chunk, hipStream_t stream);

/* ---- SGD with momentum (seg_amd.SGD) over the same chunk map --------------------
 * The tensor table is a device array of the 56-byte SegAdamWTensor records above,
 * passed as const void* and filled like this:
 *   p, g, n            the parameter, its gradient, their element count
 *   m                  momentum_buffer (NULL, and never read, when momentum == 0)
 *   v                  unused (NULL)
 *   step_size, bc2_sqrt, decay   unused
 *   pad                the seed flag: non-zero on the step that creates this
 *                      tensor's momentum_buffer, which then receives d itself
 * torch's foreach SGD (torch/optim/sgd.py::_multi_tensor_sgd) per element, fp32, in
 * its order, every element read once and written once:
 *   g = g * *grad_scale                    a product rounded on its own, as seg_adamw_step
 *   d = g + weight_decay * p               L2 form; weight_decay == 0: d is g bit for bit
 *   if momentum != 0:
 *     buf = seed ? d : buf * momentum + one_minus_dampening * d
 *     d   = nesterov ? d + momentum * buf : buf
 *   p = p - lr * d
 * one_minus_dampening is (float)(1 - dampening) formed in double.  skip and
 * grad_scale: as seg_adamw_step -- when *skip != 0 no parameter and no buffer
 * changes; .grad is never written.  nchunks < 0 or chunk < 1:
 * hipErrorInvalidValue; nchunks == 0: success, no launch. */
int seg_sgd_step(const void* tensors, const long* chunks, int nchunks, int chunk, float lr, float momentum,
                 float one_minus_dampening, float weight_decay, int nesterov, const float* skip,
                 const float* grad_scale, hipStream_t stream);

/* ---- launch tape (csrc/tape.hip): a recorded sequence of the launches above,
 *      replayed by one host call per segment -- the engine's training step
 *      (seg_amd/tape.py) without ~600 per-launch ctypes calls.  Not a hipGraph:
 *      the launches are issued on the caller's two streams (main + side), keeping
 *      their overlap.  `entries`: n records {int32 kind, fn, stream, pad; int64
 *      arg} (kind 0 launch of entry point `fn` (seg_tape_fn_index) with its
 *      arguments at args[arg..], 1 event record, 2 stream wait, 3 2-D memset,
 *      4 stop = host callback); args: 64-bit slots (fp32 values as bit
 *      patterns). */
int seg_tape_fn_index(const char* name);
int seg_tape_fn_nargs(int fn);
int seg_tape_create(const void* entries, int n, const void* args, long nargs, int nevents, void** out);
int seg_tape_destroy(void* tape);
int seg_tape_set_arg(void* tape, long i, long value);
int seg_tape_timing(void* tape, const int* idx, int n, int max_replays);
int seg_tape_elapsed(void* tape, float* out);
/* The timed launches of replay r as a timeline (tools/timeline.py): out[2k], out[2k + 1] = start / end of timed
 * launch k in ms after the start of timed launch 0.  Returns 0, or minus a hipError_t. */
int seg_tape_timeline(void* tape, int r, float* out);
int seg_tape_run(void* tape, int begin, hipStream_t main, hipStream_t side, int* stop);

/* seg_conv_igemm2_bf16io: implicit GEMM for the deep convs of the bf16io configuration
 * (replaces aten conv2d / convolution_backward(input) of src/unet.py:58,61 and 1x1 convs
 * with Cin >= 64): 8-wave 128x256 / 256x128 tiles, LDS-DMA operand staging, split-K
 * combined in-launch by the last-arriving K slice (csrc/igemm2.hip).  Stride 1, pad
 * (ks-1)/2, ks 1 or 3, bf16 rows (ldin, ldout, ldadd % 8 == 0, 16-byte aligned), bf16
 * packed weights (seg_pack_batch mode | 16, ldk % 8 == 0).  seg_conv_igemm2_plan(M, Cout,
 * Cin, ks, out[4]) returns 1 when the kernel applies and fills {tile rows, row tiles,
 * split-K slices, workspace floats}; stat (optional) = BN partials [row tiles][2][Cout];
 * work = that many floats, zeroed once before the first use (calls leave it re-armed). */
int seg_conv_igemm2_plan(long M, int Cout, int Cin, int ks, long* out);
int seg_conv_igemm2_bf16io(const seg_bf16* in, long ldin, int N, int H, int W, int Cin, const seg_bf16* wk, int ldk,
                           const float* bias, seg_bf16* out, long ldout, int Cout, int ks, const seg_bf16* add,
                           long ldadd, float* stat, float* work, hipStream_t stream);
/* Round 4: the plan also picks 4-wave 128x128 / 128x64 / 64x128 / 64x64 tiles (small-image 1x1 and 3x3
 * convs of the MobileNetV2 encoder); seg_igemm2_force_tile(t) forces table entry t (-1 = the plan). */
int seg_igemm2_force_tile(int t);
/* Tuning hook: split-K of the 4-wave tiles up to target_blocks blocks with >= min_steps 64-deep K
 * steps per slice (defaults 512, 3); values <= 0 keep the current setting. */
int seg_igemm2_tune(int target_blocks, int min_steps);

/* seg_conv_wgrad2_bf16io: the weight gradient of those narrow 3x3 convs (replaces aten's
 * convolution_backward weight path of src/unet.py:58,61 where Cout <= 64; csrc/wgrad2.hip): persistent
 * blocks walk 4 x 64-pixel tiles, the input halo and dY rows streamed into LDS by LDS-DMA once per tile
 * and 32-channel chunk, transposing LDS reads into v_mfma_f32_32x32x16_bf16.  Writes one fp32 partial
 * slab per block, part[seg_conv_wgrad2_blocks(N, H, W)][Cout][9][r4(Cin)] -- the layout of
 * seg_conv_wgrad's slabs, summed by seg_conv_wgrad_reduce(part, blocks, dw, Cout, Cin, 3, 0, acc).
 * dy: [N*H*W][lddy] (Cout channels), x: [N*H*W][ldx] (Cin channels); ld % 8 == 0, 16-byte aligned.
 * seg_conv_wgrad2_ok: H % 4 == 0, W % 64 == 0, Cin % 8 == 0, Cout % 8 == 0, Cout <= 64. */
int seg_conv_wgrad2_ok(int N, int H, int W, int Cin, int Cout);
int seg_conv_wgrad2_blocks(int N, int H, int W);
int seg_conv_wgrad2_bf16io(const seg_bf16* dy, long lddy, const seg_bf16* x, long ldx, int N, int H, int W, int Cin,
                           int Cout, float* part, hipStream_t stream);

/* Fused inverted residual of the BatchNorm-folded fp16 inference forward (BASELINE configs[3];
 * torchvision's InvertedResidual reached through src/unet.py:15-19, run per frame by
 * inference.py:162-163; csrc/mbconv.hip): out = project(relu6(dw3x3_s(relu6(expand(x) + be)) + bd))
 * + bp (+ res) in one launch, the expanded tile kept in LDS.  Weights are the folded fp32 ones
 * (seg_bn_fold_batch): we [Ch][Cin] (NULL: no expand, Ch == Cin), wd [9][Ch] (seg_pack_dw_weight
 * layout), wp [Cout][Ch]; fp16 operands with fp32 accumulation for the 1x1 convs (as
 * seg_conv_igemm_f16), fp32 depthwise (as seg_dw_fwd_bias_act).  seg_mbconv_ok: stride 1 / 2,
 * Cin <= 160 with an expand, Cout <= 320, channels % 4; res only at stride 1.  work / cnt:
 * seg_mbconv_work_floats floats and *counters unsigned (zero before the first launch; epoch words, never re-armed). */
/* The folded fp16 forward's segmentation head, outconv (src/unet.py:108-121: 1x1 -> BN -> ReLU -> 1x1, BN
 * folded), in one launch: out[M][ldo] = w2[C2][C1] . f16(act1(w1[C1][Cin] . f16(x) + b1)) + b2 -- fp16
 * operands and fp32 accumulation as seg_conv_igemm_f16 (another sum order).  seg_pw2_ok: (Cin, C1) = (32, 16),
 * C2 <= 64.  b1 / b2 may be NULL; x rows 16-byte aligned (ldx % 4 == 0). */
int seg_pw2_ok(int Cin, int C1, int C2);
int seg_pw2_f16(const float* x, long ldx, long M, int Cin, const float* w1, const float* b1, int C1, int act1,
                const float* w2, const float* b2, int C2, float* out, long ldo, hipStream_t stream);
/* The preprocess (seg_preprocess_bgr, N = 1) formed on load by the folded fp16 forward's stem conv
 * (features[0]: 3x3 stride 2 pad 1, Cin 3 padded to 4, Cout 32, BN folded): wk / ldk / bias / act as
 * seg_conv_igemm_f16's (fp16 operands, fp32 accumulation, another sum order); out [Ho*Wo][ldo] with
 * Ho = (H-1)/2+1, Wo = (W-1)/2+1. */
int seg_stem_pre_f16(const unsigned char* frame, int Hf, int Wf, long row_bytes, int H, int W, float mean_r, float mean_g,
                     float mean_b, float std_r, float std_g, float std_b, const float* wk, int ldk, const float* bias,
                     int act, int Cout, float* out, long ldo, hipStream_t stream);
/* Tuning hook: the blocks per launch seg_mbconv_f16's hidden splits aim for (> 0 sets it; returns the
 * previous value). */
int seg_mbconv_tune(int max_blocks);
int seg_mbconv_ok(int Cin, int Ch, int Cout, int stride, int expand);
long seg_mbconv_work_floats(int N, int H, int W, int Ch, int Cout, int stride, int* counters);
/* Test hook: the poll bound of every in-launch split combine (seg_mbconv_f16, seg_conv_igemm_*_ic); -1 = automatic,
 * 0 = no poll -- every block but a tile's last hands its share to the last arrival.  Results are identical. */
int seg_set_combine_spin(int spin);
int seg_mbconv_f16(const float* x, long ldx, int N, int H, int W, int Cin, const float* we, const float* be, int Ch,
                   const float* wd, const float* bd, int stride, const float* wp, const float* bp, int Cout,
                   const float* res, long ldres, float* out, long ldo, float* work, unsigned* cnt,
                   hipStream_t stream);

/* ---- overlay post-processing (inference.py:72-146, overlay_predictions; csrc/overlay.hip) --------
 * The reference's per-frame OpenCV stage on the GPU: road = (cls == 1) -> 5x5 close -> 8-connected
 * components -> largest -> cleaned = cls with that component painted 1 -> class colours -> car blobs
 * (components of cleaned == 2) with boxes -> 0.6 / 0.4 blend -> box outlines.  All entries are
 * stream-ordered with no host round trip; every result is independent of scheduling.  Frames, masks and
 * results are contiguous ([Hf][Wf][3] / [Hf][Wf] bytes); Hf * Wf < 2^31.
 *   labels: int [Hf][Wf], the smallest linear index y*Wf + x of the pixel's component, background -1;
 *   boxes:  int [max_boxes][5] = x, y, w, h, area (pixel count) of the components with area > min_area, in
 *           ascending label order; count[2] = {stored (<= max_boxes), passed};
 *   table:  [ncolors][4] bytes = the class's colour in the frame's channel order + a "listed" flag; a class
 *           that is not listed (or >= ncolors) keeps the frame's pixel;
 *   work:   seg_overlay_workspace_bytes(Hf, Wf, max_boxes) bytes (0 = invalid sizes), 16-byte aligned,
 *           caller-owned, needs no clearing between frames.
 * seg_cc_tile_h / _w: the labelling tile (tests place shapes on its borders). */
int seg_cc_tile_h(void);
int seg_cc_tile_w(void);
long seg_overlay_workspace_bytes(int Hf, int Wf, int max_boxes);
/* out = 5x5 close (all-ones element, one iteration, cv2's constant border) of (mask == class_id), 0 / 1 */
int seg_morph_close5(const unsigned char* mask, int Hf, int Wf, int class_id, unsigned char* out,
                     hipStream_t stream);
int seg_cc_label8(const unsigned char* mask, int Hf, int Wf, int* labels, hipStream_t stream);
/* out[2] = root, area of the largest component (ties: the smaller root); {-1, 0} without foreground */
int seg_cc_largest(const int* labels, int Hf, int Wf, int* out, void* work, long work_bytes, hipStream_t stream);
int seg_cc_boxes(const int* labels, int Hf, int Wf, int min_area, int max_boxes, int* boxes, int* count, void* work,
                 long work_bytes, hipStream_t stream);
/* result = rint(float(frame) * 0.6f + float(overlay) * 0.4f), overlay = table[cleaned] (cv2.addWeighted's
 * 8-bit path as published: float32 products and sum, no fused multiply-add, half to even) */
int seg_overlay_blend(const unsigned char* frame, const unsigned char* cleaned, int Hf, int Wf,
                      const unsigned char* table, int ncolors, unsigned char* result, hipStream_t stream);
/* per stored box: the pixels of [x, x+w] x [y, y+h] (clipped) outside [x+2, x+w-2] x [y+2, y+h-2] become
 * blend(frame, (0, 255, 0)) */
int seg_overlay_outline(const unsigned char* frame, int Hf, int Wf, const int* boxes, const int* count,
                        int max_boxes, unsigned char* result, hipStream_t stream);
/* the whole stage on the class mask cls (what seg_argmax_nearest writes): 16 launches, one chain */
int seg_overlay_frame(const unsigned char* frame, const unsigned char* cls, int Hf, int Wf,
                      const unsigned char* table, int ncolors, int min_area, int max_boxes, int draw_boxes,
                      unsigned char* cleaned, unsigned char* result, int* boxes, int* count, void* work,
                      long work_bytes, hipStream_t stream);

/* Build identity (host only): copies the SHA-256 (64 hex chars + NUL) of the sources this
 * library was built from -- every csrc file, this header, compiler and flags
 * (seg_amd/build.py source_hash) -- into out when cap > 64; returns the length.  The
 * Python binding refuses a library whose hash differs from the tree it runs in. */
int seg_build_hash(char* out, int cap);

#ifdef __cplusplus
}
#endif
#endif /* SEGAMD_H */
