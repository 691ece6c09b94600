// The fused segmentation losses: per-pixel criteria fused with the model's final align_corners=True
// bilinear upsample.  Six kernel families share one file and one set of per-pixel helpers:
//   seg_ce_*    nn.CrossEntropyLoss() as the reference applies it (main.py:99, src/train.py:37) to the model
//               output, whose last op is final_upsample (src/unet.py:30,49): weight=None, ignore_index=-100,
//               label_smoothing=0, labels int64.  loss = sum_{valid p} (logsumexp(z_p) - z_p[y_p]) / #valid,
//               d loss / d z_p = g * (softmax(z_p) - onehot(y_p)) / #valid  (g = upstream grad).
//   seg_cew_*   aten's remaining options for class-index targets: class weights, label smoothing, mean / sum.
//   seg_sl_*    a focal term and soft Dice beside cross-entropy (seg_amd.SegLoss).
//   seg_ohem_*  online hard example mining (seg_amd.OhemCELoss).
//   seg_kd_*    knowledge distillation from a teacher's logits (seg_amd.DistillLoss).
//   seg_bce_*   one logit per pixel: sigmoid cross-entropy, focal exponent and soft Dice (seg_amd.BinarySegLoss).
// Each family's formulas stand above its kernels.
//
// The full-resolution logits z_p are never stored: each kernel recomputes them from the NHWC low-resolution
// logits (4 taps x C), which stay L2-resident.  Every reduction is deterministic: register accumulators, per-block
// partials in a fixed order, then one fp64 pass; integer atomics where counts are binned (integer sums do not
// depend on arrival order).  A label outside [0, C) that is not ignore_index (aten raises "Target out of bounds")
// is counted in stats[2] and poisons the loss and the gradient with NaN -- stream-ordered, no host sync; the host
// raises when it reads the loss (seg_amd.train / engine.check_targets).
//
// What is shared, each defined once in the first namespace below, and what therefore holds bit for bit by
// construction rather than by keeping copies in step:
//   pixel_of, full_res_logits, softmax_stats   every kernel of every family recomputes the same logits, row maximum,
//                                              exponentials and z[y] of a pixel: eval = loss, gradient = forward;
//   class_weights, pick                        w[y] by the select that picks z[y]; with w = 1 (or NULL), eps = 0 and
//                                              mean reduction every weighted term is the plain term times 1 plus 0,
//                                              so seg_cew_* without options is seg_ce_*, and so on up the families;
//   ce_scale                                   the gradient's g / D, NaN behind an out-of-range label: the OHEM
//                                              gradient on K is the weighted gradient;
//   argmax_real, hist_clear / _count / _flush  validation's argmax (strict >, ascending: ties go to the lowest index,
//                                              torch.max's rule; padded lanes never compete) and confusion matrix;
//   block_partials, column_sums_f64            the per-block partials and the finalize's fp64 sums: out[0..2] of an
//                                              eval call are the loss call's;
//   zero_row, store_quad                       the gradient rows or NCHW planes, bf16 = fp32 rounded once;
//   up_scale, loss_blocks, grad_blocks,        the host side: align-corners scales, grids, the argument checks and
//   loss_geom_ok, rows_ok, SEG_LAUNCH_CP       the dispatch over CP = round4(C).
// A new loss family calls these; it does not copy them.
#include "common.h"

// Every rounding in this file is written out: no implicit contraction of a * b + c into an fma,
// and __builtin_fmaf where one is meant.  Left to the compiler, the same source expression (the
// bilinear blend above all) was contracted differently from one instantiation to the next, so
// kernels that should agree recomputed logits that differed in the last bit.  The forms chosen
// are the ones the fp32 gradient kernels always compiled to.
#pragma clang fp contract(off)

namespace {

// LinAC / lin_ac (common.h): the align_corners=True source index and tap weights of every kernel in this file.

constexpr int CMAX = 32;

// Pixel p of [N][Ho][Wo]: image, offset in its plane, row, column.
struct Pix {
  int n, rem, r, s;
};
__device__ __forceinline__ Pix pixel_of(long p, int Ho, int Wo) {
  const int n = (int)(p / ((long)Ho * Wo));
  const int rem = (int)(p - (long)n * Ho * Wo);
  const int r = rem / Wo;
  return Pix{n, rem, r, rem - r * Wo};
}

// Recompute the CP (= round4(C)) full-res logits of pixel (n, r, s); the class
// loops are unrolled over CP so z stays in registers with constant indices.
template <int CP, typename T>
__device__ __forceinline__ void full_res_logits(const T* __restrict__ low, long ld, int H, int W, int n, int r,
                                                int s, float sh, float sw, float (&z)[CP]) {
  const LinAC lh = lin_ac(r, H, sh), lw = lin_ac(s, W, sw);
  const T* base = low + (long)n * H * W * ld;
  const T* p00 = base + ((long)lh.i0 * W + lw.i0) * ld;
  const T* p01 = base + ((long)lh.i0 * W + lw.i1) * ld;
  const T* p10 = base + ((long)lh.i1 * W + lw.i0) * ld;
  const T* p11 = base + ((long)lh.i1 * W + lw.i1) * ld;
#pragma unroll
  for (int c = 0; c < CP; c += 4) {
    const f32x4 v00 = ld4(p00 + c), v01 = ld4(p01 + c), v10 = ld4(p10 + c), v11 = ld4(p11 + c);
#pragma unroll
    for (int j = 0; j < 4; ++j) {  // lh.l0 * (lw.l0 * v00 + lw.l1 * v01) + lh.l1 * (lw.l0 * v10 + lw.l1 * v11)
      const float top = __builtin_fmaf(v01[j], lw.l1, v00[j] * lw.l0);
      const float bot = __builtin_fmaf(v11[j], lw.l1, v10[j] * lw.l0);
      z[c + j] = lh.l0 * top + lh.l1 * bot;
    }
  }
}

// max, sum of exp(z - max) and z[y] over the C valid classes
template <int CP>
__device__ __forceinline__ void softmax_stats(float (&z)[CP], int C, int y, float& m, float& se, float& zy,
                                              bool keep_exp) {
  m = z[0];
#pragma unroll
  for (int c = 1; c < CP; ++c)
    if (c < C) m = fmaxf(m, z[c]);
  se = 0.f;
  zy = 0.f;
#pragma unroll
  for (int c = 0; c < CP; ++c) {
    const float e = c < C ? expf(z[c] - m) : 0.f;
    zy = c == y ? z[c] : zy;
    se += e;
    if (keep_exp) z[c] = e;
  }
}

// The class weights as CP wave-uniform values (scalar loads; 1 when cw is NULL, 0 on the padded
// lanes) and their sum over the C real classes, in ascending order.
template <int CP>
__device__ __forceinline__ float class_weights(const float* __restrict__ cw, int C, float (&w)[CP]) {
  float sw = 0.f;
#pragma unroll
  for (int c = 0; c < CP; ++c) {
    w[c] = c < C ? (cw ? cw[c] : 1.f) : 0.f;
    sw += w[c];
  }
  return sw;
}

// w[y] by the select that picks z[y] in softmax_stats (0 when y is no lane of w)
template <int CP>
__device__ __forceinline__ float pick(const float (&w)[CP], int y) {
  float v = 0.f;
#pragma unroll
  for (int c = 0; c < CP; ++c) v = c == y ? w[c] : v;
  return v;
}

// The cross-entropy gradient's scale g / D, or NaN when the forward counted an out-of-range label (stats[2]): the
// loss already is
__device__ __forceinline__ float ce_scale(const float* __restrict__ stats, const float* __restrict__ gout) {
  return stats[2] > 0.f ? __builtin_nanf("") : gout[0] / stats[1];
}

// Validation: the argmax over the C real classes (strict >, ascending; the padded lanes C..CP-1 never compete) ...
template <int CP>
__device__ __forceinline__ int argmax_real(const float (&z)[CP], int C) {
  int pred = 0;
  float best = z[0];
#pragma unroll
  for (int c = 1; c < CP; ++c)
    if (c < C && z[c] > best) {
      best = z[c];
      pred = c;
    }
  return pred;
}

// ... binned into a per-block LDS histogram [label][prediction] (`__shared__ int hist[CMAX * CMAX]` in the kernel),
// whose non-zero bins are then added to `confusion` with 64-bit integer atomics.  The caller puts a __syncthreads()
// between clear and count and between count and flush; both are barriers the kernel has anyway.
__device__ __forceinline__ void hist_clear(int* hist, int C) {
  for (int i = threadIdx.x; i < C * C; i += blockDim.x) hist[i] = 0;
}
__device__ __forceinline__ void hist_count(int* hist, int C, int y, int pred) { atomicAdd(&hist[y * C + pred], 1); }
__device__ __forceinline__ void hist_flush(const int* hist, int C, unsigned long long* __restrict__ confusion) {
  for (int i = threadIdx.x; i < C * C; i += blockDim.x) {
    const int v = hist[i];
    if (v) atomicAdd(confusion + i, (unsigned long long)v);
  }
}

// A 256-thread block's NP sums: the wave butterfly, lane 0 of each of the four waves through LDS, one
// __syncthreads() -- which also closes whatever LDS counters the kernel filled before the call -- then thread j
// writes red[0][j] + red[1][j] + red[2][j] + red[3][j] to part[at(j)] (at(j) < 0: no store).  Which thread adds the
// four does not change the number: the same four addends in the same order.
template <int NP, typename At>
__device__ __forceinline__ void block_partials(const float (&v)[NP], float (&red)[4][NP], float* __restrict__ part,
                                               At at) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const float s = wave_sum(v[j]);
    if (lane == 0) red[wave][j] = s;
  }
  __syncthreads();
  if (threadIdx.x < NP) {
    const int j = threadIdx.x;
    const long i = at(j);
    if (i >= 0) part[i] = red[0][j] + red[1][j] + red[2][j] + red[3][j];
  }
}
// ... in rows of NP per block, part[NP * block + j]
template <int NP>
__device__ __forceinline__ void block_partials(const float (&v)[NP], float (&red)[4][NP], float* __restrict__ part) {
  block_partials<NP>(v, red, part, [](int j) { return (long)(NP * blockIdx.x + j); });
}

// The finalize's sums over the blocks, by one wave in fp64: tot[j] = sum_k part[stride * k + j], lane i taking
// blocks i, i + 64, ..., then a 64-lane butterfly that leaves the totals in every lane.
template <int NC>
__device__ __forceinline__ void column_sums_f64(const float* __restrict__ part, int nblk, int stride,
                                                double (&tot)[NC]) {
#pragma unroll
  for (int j = 0; j < NC; ++j) tot[j] = 0.0;
  for (int k = threadIdx.x & 63; k < nblk; k += 64) {
#pragma unroll
    for (int j = 0; j < NC; ++j) tot[j] += part[stride * k + j];
  }
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int j = 0; j < NC; ++j) tot[j] += __shfl_xor(tot[j], o, 64);
  }
}

// The gradient of one pixel: T rows [pixel][ldh] at d, or (NCHW) fp32 planes [N][C][Ho][Wo] with this pixel's
// class 0 at dn.  The planes are what the bf16io twins of seg_ohem_* and seg_kd_* write: the low-resolution
// gradient then sums unrounded terms, as it does behind the full-resolution logits of the model's forward; bf16 rows
// would put an error of 2^-9 on every term, 2e-4 on the head's parameter gradients.
template <int CP, bool NCHW, typename T>
__device__ __forceinline__ void zero_row(T* d, float* dn = nullptr, int C = 0, long plane = 0) {
  if constexpr (NCHW) {
    for (int c = 0; c < C; ++c) dn[c * plane] = 0.f;
  } else {
#pragma unroll
    for (int c = 0; c < CP; c += 4) st4(d + c, f32x4{0.f, 0.f, 0.f, 0.f});
  }
}
template <bool NCHW, typename T>
__device__ __forceinline__ void store_quad(T* d, float* dn, int c, int C, long plane, f32x4 o) {
  if constexpr (NCHW) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (c + j < C) dn[(c + j) * plane] = o[j];
  } else {
    st4(d + c, o);
  }
}

// ---- the host side ----
struct UpScale {
  float sh, sw;
};
inline UpScale up_scale(int H, int W, int Ho, int Wo) {
  return UpScale{Ho > 1 ? (float)(H - 1) / (float)(Ho - 1) : 0.f, Wo > 1 ? (float)(W - 1) / (float)(Wo - 1) : 0.f};
}

int loss_blocks(long total) { return (int)std::min<long>(seg_cdiv(total, 256), 2048); }
int grad_blocks(long total) { return (int)std::min<long>(seg_cdiv(total, 256), 8192); }

// Low-resolution rows of ld floats hold CP = round4(C) readable ones; the gradient's rows of ldh likewise.
inline bool loss_geom_ok(long ld, int C) { return !(ld & 3) && C >= 1 && C <= CMAX && ld >= C; }
inline bool rows_ok(long ldh, int C) { return !(ldh & 3) && ldh >= C; }

// Launch KERNEL<CP, TARGS...> with CP = round4(C) on `grid` blocks of 256: the class loops of every kernel are
// unrolled over CP.  TARGS is the parenthesised rest of the template argument list.
#define SEG_UNPAREN(...) __VA_ARGS__
#define SEG_CP_CASE(CP, KERNEL, TARGS, grid, stream, ...)                                                     \
  case CP:                                                                                                    \
    hipLaunchKernelGGL((KERNEL<CP, SEG_UNPAREN TARGS>), dim3(grid), dim3(256), 0, stream, __VA_ARGS__);       \
    break;
#define SEG_LAUNCH_CP(C, KERNEL, TARGS, grid, stream, ...)          \
  switch ((C + 3) & ~3) {                                           \
    SEG_CP_CASE(4, KERNEL, TARGS, grid, stream, __VA_ARGS__)        \
    SEG_CP_CASE(8, KERNEL, TARGS, grid, stream, __VA_ARGS__)        \
    SEG_CP_CASE(12, KERNEL, TARGS, grid, stream, __VA_ARGS__)       \
    SEG_CP_CASE(16, KERNEL, TARGS, grid, stream, __VA_ARGS__)       \
    SEG_CP_CASE(20, KERNEL, TARGS, grid, stream, __VA_ARGS__)       \
    SEG_CP_CASE(24, KERNEL, TARGS, grid, stream, __VA_ARGS__)       \
    SEG_CP_CASE(28, KERNEL, TARGS, grid, stream, __VA_ARGS__)       \
    SEG_CP_CASE(32, KERNEL, TARGS, grid, stream, __VA_ARGS__)       \
  }

// ---- seg_ce_* and, with a CeOpt, seg_cew_* ----
// Over the valid pixels V, with class weights w (all ones when NULL), label smoothing eps, reduction mean / sum:
//   nll    = sum_p w[y_p] * (lse_p - z_p[y_p]),   smooth = sum_p sum_c w[c] * (lse_p - z_p[c]),
//   D      = sum_p w[y_p] (mean) | 1 (sum),       loss   = ((1 - eps) * nll + (eps / C) * smooth) / D,
//   d loss / d z_p[c] = (g / D) * [(1 - eps) * w[y_p] * (softmax_c - [c == y_p])
//                                  + (eps / C) * (softmax_c * sum_k w[k] - w[c])].
// The kernels take the options as a trailing parameter pack that is empty for the plain entry points, whose
// instantiations therefore keep their parameters and compile none of the option code.
struct CeOpt {
  const float* cw;  // C class weights in device memory, or NULL = all ones
  float eps;        // label smoothing
  int reduction;    // 0 = mean, 1 = sum (read by the finalize only)
};
__device__ __forceinline__ CeOpt ce_opt() { return CeOpt{nullptr, 0.f, 0}; }
__device__ __forceinline__ CeOpt ce_opt(CeOpt o) { return o; }

// Three partials per block [nll, #valid, #out-of-range]; O = CeOpt: five, [nll, sum of w[y], #out-of-range, smooth,
// #valid].  EVAL: the validation form, the same partials plus the confusion matrix.
template <int CP, typename T, bool EVAL, typename... O>
__global__ __launch_bounds__(256) void ce_up_loss_kernel(const T* __restrict__ low, long ld, int N, int H, int W,
                                                         int C, const long long* __restrict__ labels, int Ho, int Wo,
                                                         float sh, float sw, int ignore_index,
                                                         float* __restrict__ part,
                                                         unsigned long long* __restrict__ confusion, O... opt) {
  constexpr bool WS = sizeof...(O) > 0;
  constexpr int NP = WS ? 5 : 3;
  __shared__ float red[4][NP];
  __shared__ int hist[EVAL ? CMAX * CMAX : 1];
  if constexpr (EVAL) {
    hist_clear(hist, C);
    __syncthreads();
  }
  const long total = (long)N * Ho * Wo;
  float lsum = 0.f, cnt = 0.f, bad = 0.f, ssum = 0.f, val = 0.f;
  float w[WS ? CP : 1];
  float wsum = 0.f;
  if constexpr (WS) wsum = class_weights<CP>(ce_opt(opt...).cw, C, w);
  for (long p = blockIdx.x * (long)blockDim.x + threadIdx.x; p < total; p += (long)gridDim.x * blockDim.x) {
    const long long y = labels[p];
    if (y == ignore_index) continue;
    if (y < 0 || y >= C) {
      bad += 1.f;
      continue;
    }
    const Pix px = pixel_of(p, Ho, Wo);
    float z[CP];
    full_res_logits<CP, T>(low, ld, H, W, px.n, px.r, px.s, sh, sw, z);
    float m, se, zy;
    softmax_stats<CP>(z, C, (int)y, m, se, zy, false);
    if constexpr (WS) {
      const float wy = pick<CP>(w, (int)y);
      float wz = 0.f;  // sum_c w[c] * (z[c] - m) after the row maximum is gone
#pragma unroll
      for (int c = 0; c < CP; ++c)
        if (c < C) wz = __builtin_fmaf(w[c], z[c] - m, wz);  // the padded lanes may hold anything
      const float lse = logf(se);
      lsum = __builtin_fmaf(wy, m + lse - zy, lsum);  // wy = 1: the plain branch's sum
      cnt += wy;
      ssum += __builtin_fmaf(wsum, lse, -wz);
      val += 1.f;
    } else {
      lsum += m + logf(se) - zy;
      cnt += 1.f;
    }
    if constexpr (EVAL) hist_count(hist, C, (int)y, argmax_real<CP>(z, C));
  }
  float v[NP];
  v[0] = lsum, v[1] = cnt, v[2] = bad;
  if constexpr (WS) v[3] = ssum, v[4] = val;
  block_partials<NP>(v, red, part);
  if constexpr (EVAL) hist_flush(hist, C, confusion);
}

// out[0] = mean loss, out[1] = #valid pixels, out[2] = #out-of-range labels (as floats)
__global__ void ce_finalize_kernel(const float* __restrict__ part, int nblk, float* out) {
  double t[3];
  column_sums_f64<3>(part, nblk, 3, t);
  const double l = t[0], c = t[1], b = t[2];
  if (threadIdx.x == 0) {
    out[0] = b > 0.0 ? __builtin_nanf("") : (float)(l / c);  // 0/0 = nan when every pixel is ignored, as aten
    out[1] = (float)c;
    out[2] = (float)b;
  }
}

// out4 = [loss, D, #out-of-range labels, #valid pixels] of the weighted / smoothed form; D = sum of
// w[y] (mean; 0/0 = nan as aten when it is 0) or 1 (sum).  eps == 0 leaves the smoothing sum out, so
// the loss is then the plain finalize's l / c.
__global__ void cew_finalize_kernel(const float* __restrict__ part, int nblk, float eps, int C, int reduction,
                                    float* out) {
  double t[5];
  column_sums_f64<5>(part, nblk, 5, t);
  const double l = t[0], c = t[1], b = t[2], sm = t[3], v = t[4];
  if (threadIdx.x == 0) {
    const double d = reduction == 0 ? c : 1.0;
    const double num = eps > 0.f ? (1.0 - (double)eps) * l + ((double)eps / C) * sm : l;
    out[0] = b > 0.0 ? __builtin_nanf("") : (float)(num / d);
    out[1] = (float)d;
    out[2] = (float)b;
    out[3] = (float)v;
  }
}

// dhigh[p][c] = g * (softmax(z_p)[c] - [c == y_p]) / count, NHWC rows; O = CeOpt: the weighted form, D = stats[1].
template <int CP, typename T, typename... O>
__global__ __launch_bounds__(256) void ce_up_grad_kernel(const T* __restrict__ low, long ld, int N, int H, int W,
                                                         int C, const long long* __restrict__ labels, int Ho, int Wo,
                                                         float sh, float sw, int ignore_index,
                                                         const float* __restrict__ gout, const float* __restrict__ stats,
                                                         T* __restrict__ dhigh, long ldh, O... opt) {
  constexpr bool WS = sizeof...(O) > 0;
  const long total = (long)N * Ho * Wo;
  const float scale = ce_scale(stats, gout);
  float w[WS ? CP : 1];
  float wsum = 0.f, keep = 1.f, spread = 0.f;
  if constexpr (WS) {
    const CeOpt o = ce_opt(opt...);
    wsum = class_weights<CP>(o.cw, C, w);
    keep = 1.f - o.eps;
    spread = o.eps / (float)C;
  }
  for (long p = blockIdx.x * (long)blockDim.x + threadIdx.x; p < total; p += (long)gridDim.x * blockDim.x) {
    const long long y = labels[p];
    T* d = dhigh + p * ldh;
    if (y == ignore_index || y < 0 || y >= C) {
      zero_row<CP, false>(d);
      continue;
    }
    const Pix px = pixel_of(p, Ho, Wo);
    float z[CP];
    full_res_logits<CP, T>(low, ld, H, W, px.n, px.r, px.s, sh, sw, z);
    float m, se, zy;
    softmax_stats<CP>(z, C, (int)y, m, se, zy, true);
    const float inv = 1.f / se;
    float kw = 0.f;  // (1 - eps) * w[y]
    if constexpr (WS) kw = pick<CP>(w, (int)y) * keep;
#pragma unroll
    for (int c = 0; c < CP; c += 4) {
      f32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int cc = c + j;
        const float nl = __builtin_fmaf(z[cc], inv, cc == (int)y ? -1.f : -0.f);
        if constexpr (WS) {
          // with w = 1 and eps = 0 the rest is * 1 and + 0
          const float sm = __builtin_fmaf(z[cc] * inv, wsum, -w[cc]);
          o[j] = cc < C ? scale * __builtin_fmaf(spread, sm, kw * nl) : 0.f;
        } else {
          o[j] = cc < C ? scale * nl : 0.f;
        }
      }
      st4(d + c, o);
    }
  }
}

}  // namespace

SEG_API long seg_ce_workspace_floats(long pixels) { return 3L * loss_blocks(pixels); }

inline bool ce_opt_ok() { return true; }
inline bool ce_opt_ok(CeOpt o) { return (o.reduction == 0 || o.reduction == 1) && o.eps >= 0.f && o.eps <= 1.f; }

// opt (seg_cew_*): one CeOpt; out2 is then out4.
template <typename T, bool EVAL = false, typename... O>
static int ce_loss_impl(const T* low, long ld, int N, int H, int W, int C, const long long* labels, int Ho, int Wo,
                        int ignore_index, float* work, float* out2, hipStream_t stream, long long* confusion,
                        O... opt) {
  constexpr bool WS = sizeof...(O) > 0;
  if (!loss_geom_ok(ld, C) || (EVAL && !confusion) || !ce_opt_ok(opt...)) return (int)hipErrorInvalidValue;
  const int nb = loss_blocks((long)N * Ho * Wo);
  const UpScale up = up_scale(H, W, Ho, Wo);
  SEG_LAUNCH_CP(C, ce_up_loss_kernel, (T, EVAL, O...), nb, stream, low, ld, N, H, W, C, labels, Ho, Wo, up.sh, up.sw,
                ignore_index, work, (unsigned long long*)confusion, opt...)
  if constexpr (WS) {
    const CeOpt o = CeOpt{opt...};
    hipLaunchKernelGGL(cew_finalize_kernel, dim3(1), dim3(64), 0, stream, work, nb, o.eps, C, o.reduction, out2);
  } else
    hipLaunchKernelGGL(ce_finalize_kernel, dim3(1), dim3(64), 0, stream, work, nb, out2);
  SEG_RET_LAST();
}

// Mean CE of bilinear_ac_true_x(Ho,Wo)(low) against labels.  out3[0] = loss, out3[1] = number of non-ignored
// pixels, out3[2] = number of out-of-range labels.  `work` >= seg_ce_workspace_floats(N*Ho*Wo).
SEG_API int seg_ce_upsample_loss(const float* low, long ld, int N, int H, int W, int C, const long long* labels, int Ho,
                                 int Wo, int ignore_index, float* work, float* out2, hipStream_t stream) {
  return ce_loss_impl(low, ld, N, H, W, C, labels, Ho, Wo, ignore_index, work, out2, stream, nullptr);
}
SEG_API int seg_ce_upsample_loss_bf16io(const __bf16* low, long ld, int N, int H, int W, int C,
                                        const long long* labels, int Ho, int Wo, int ignore_index, float* work,
                                        float* out2, hipStream_t stream) {
  return ce_loss_impl(low, ld, N, H, W, C, labels, Ho, Wo, ignore_index, work, out2, stream, nullptr);
}

// Validation: seg_ce_upsample_loss plus the confusion matrix of the full-resolution argmax,
// confusion[label * C + prediction] += 1 per non-ignored in-range pixel (C*C int64, device memory).
SEG_API int seg_ce_upsample_eval(const float* low, long ld, int N, int H, int W, int C, const long long* labels, int Ho,
                                 int Wo, int ignore_index, float* work, float* out3, long long* confusion,
                                 hipStream_t stream) {
  return ce_loss_impl<float, true>(low, ld, N, H, W, C, labels, Ho, Wo, ignore_index, work, out3, stream, confusion);
}
SEG_API int seg_ce_upsample_eval_bf16io(const __bf16* low, long ld, int N, int H, int W, int C,
                                        const long long* labels, int Ho, int Wo, int ignore_index, float* work,
                                        float* out3, long long* confusion, hipStream_t stream) {
  return ce_loss_impl<__bf16, true>(low, ld, N, H, W, C, labels, Ho, Wo, ignore_index, work, out3, stream, confusion);
}

// Full-resolution logit gradient (NHWC rows of ldh); follow with seg_upsample_bwd(nchw_grad = 0, ac = 1) to reach
// the low-res logits.
template <typename T, typename... O>
static int ce_grad_impl(const T* low, long ld, int N, int H, int W, int C, const long long* labels, int Ho, int Wo,
                        int ignore_index, const float* grad_out, const float* stats, T* dhigh, long ldh,
                        hipStream_t stream, O... opt) {
  if (!loss_geom_ok(ld, C) || !rows_ok(ldh, C) || !ce_opt_ok(opt...)) return (int)hipErrorInvalidValue;
  const UpScale up = up_scale(H, W, Ho, Wo);
  SEG_LAUNCH_CP(C, ce_up_grad_kernel, (T, O...), grad_blocks((long)N * Ho * Wo), stream, low, ld, N, H, W, C, labels,
                Ho, Wo, up.sh, up.sw, ignore_index, grad_out, stats, dhigh, ldh, opt...)
  SEG_RET_LAST();
}
SEG_API int seg_ce_upsample_grad(const float* low, long ld, int N, int H, int W, int C, const long long* labels, int Ho,
                                 int Wo, int ignore_index, const float* grad_out, const float* stats, float* dhigh,
                                 long ldh, hipStream_t stream) {
  return ce_grad_impl(low, ld, N, H, W, C, labels, Ho, Wo, ignore_index, grad_out, stats, dhigh, ldh, stream);
}
SEG_API int seg_ce_upsample_grad_bf16io(const __bf16* low, long ld, int N, int H, int W, int C,
                                        const long long* labels, int Ho, int Wo, int ignore_index,
                                        const float* grad_out, const float* stats, __bf16* dhigh, long ldh,
                                        hipStream_t stream) {
  return ce_grad_impl(low, ld, N, H, W, C, labels, Ho, Wo, ignore_index, grad_out, stats, dhigh, ldh, stream);
}

// out4 = [loss, D, #out-of-range labels, #valid pixels]; `work` >= seg_cew_workspace_floats(N*Ho*Wo).
SEG_API long seg_cew_workspace_floats(long pixels) { return 5L * loss_blocks(pixels); }

SEG_API int seg_cew_upsample_loss(const float* low, long ld, int N, int H, int W, int C, const long long* labels,
                                  int Ho, int Wo, int ignore_index, const float* class_weight, float label_smoothing,
                                  int reduction, float* work, float* out4, hipStream_t stream) {
  return ce_loss_impl<float, false>(low, ld, N, H, W, C, labels, Ho, Wo, ignore_index, work, out4, stream, nullptr,
                                    CeOpt{class_weight, label_smoothing, reduction});
}
SEG_API int seg_cew_upsample_loss_bf16io(const __bf16* low, long ld, int N, int H, int W, int C,
                                         const long long* labels, int Ho, int Wo, int ignore_index,
                                         const float* class_weight, float label_smoothing, int reduction, float* work,
                                         float* out4, hipStream_t stream) {
  return ce_loss_impl<__bf16, false>(low, ld, N, H, W, C, labels, Ho, Wo, ignore_index, work, out4, stream, nullptr,
                                     CeOpt{class_weight, label_smoothing, reduction});
}
SEG_API int seg_cew_upsample_eval(const float* low, long ld, int N, int H, int W, int C, const long long* labels,
                                  int Ho, int Wo, int ignore_index, const float* class_weight, float label_smoothing,
                                  int reduction, float* work, float* out4, long long* confusion, hipStream_t stream) {
  return ce_loss_impl<float, true>(low, ld, N, H, W, C, labels, Ho, Wo, ignore_index, work, out4, stream, confusion,
                                   CeOpt{class_weight, label_smoothing, reduction});
}
SEG_API int seg_cew_upsample_eval_bf16io(const __bf16* low, long ld, int N, int H, int W, int C,
                                         const long long* labels, int Ho, int Wo, int ignore_index,
                                         const float* class_weight, float label_smoothing, int reduction, float* work,
                                         float* out4, long long* confusion, hipStream_t stream) {
  return ce_loss_impl<__bf16, true>(low, ld, N, H, W, C, labels, Ho, Wo, ignore_index, work, out4, stream, confusion,
                                    CeOpt{class_weight, label_smoothing, reduction});
}
SEG_API int seg_cew_upsample_grad(const float* low, long ld, int N, int H, int W, int C, const long long* labels,
                                  int Ho, int Wo, int ignore_index, const float* class_weight, float label_smoothing,
                                  const float* grad_out, const float* stats, float* dhigh, long ldh,
                                  hipStream_t stream) {
  return ce_grad_impl(low, ld, N, H, W, C, labels, Ho, Wo, ignore_index, grad_out, stats, dhigh, ldh, stream,
                      CeOpt{class_weight, label_smoothing, 0});
}
SEG_API int seg_cew_upsample_grad_bf16io(const __bf16* low, long ld, int N, int H, int W, int C,
                                         const long long* labels, int Ho, int Wo, int ignore_index,
                                         const float* class_weight, float label_smoothing, const float* grad_out,
                                         const float* stats, __bf16* dhigh, long ldh, hipStream_t stream) {
  return ce_grad_impl(low, ld, N, H, W, C, labels, Ho, Wo, ignore_index, grad_out, stats, dhigh, ldh, stream,
                      CeOpt{class_weight, label_smoothing, 0});
}

// ---- focal term and soft Dice beside cross-entropy: seg_sl_* (the criterion is seg_amd.SegLoss) ----
// Over the valid pixels V, with s_p = softmax(z_p), pt_p = s_p[y_p], w the class weights (all ones when NULL):
//   F    = sum_p w[y_p] (1 - pt_p)^gamma (-log pt_p) / D,  D = sum_p w[y_p]   (gamma > 0; label smoothing is then 0)
//   F    = the seg_cew_* mean loss ((1 - eps) nll + (eps / C) smooth) / D     (gamma == 0)
//   I_c  = sum_p s_p[c] [y_p = c],  S_c = sum_p s_p[c],  T_c = sum_p [y_p = c],  U_c = S_c + T_c + smooth,
//   Dice = sum_c m_c (1 - (2 I_c + smooth) / U_c) / max(M, 1),  m_c = [T_c > 0],  M = sum_c m_c,
//   loss = ce F + dice Dice    (a term whose coefficient is 0 is left out, so its 0/0 never reaches the loss).
// One pass over the pixels writes, per block, the five partials of the seg_cew_* kernels, the focal sum and I_c, S_c,
// T_c (T_c is an LDS integer count: exact).  The partials lie column-major, part[col * nblk + block], so that the
// one-block fp64 finalize reads them coalesced; it writes stats = [loss, D, #out-of-range labels, #valid, F, Dice]
// and the table of the Dice gradient's per-class coefficients
//   a_c = m_c 2 / (M U_c)  at table[c],   b_c = m_c (2 I_c + smooth) / (M U_c^2)  at table[32 + c]
// (d Dice / d s_p[c] = q_c = b_c - a_c [c = y_p]).  The gradient kernel reads them as wave-uniform values, like the
// class weights:
//   dz_k = (g / D) ce [(1 - eps) w[y] f_p (s_k - [k = y]) + (eps / C) (s_k sum_c w[c] - w[k])]
//          + g dice s_k (q_k - sum_c q_c s_c),     f_p = (1 - pt)^gamma - gamma pt (1 - pt)^(gamma - 1) log pt.
// Numerical form: 1 - pt is sum_{c != y} e_c / sum_c e_c, never 1.f - pt (no correct bit is left of that when the
// label's class dominates), and s_y - 1 is its negative; f_p is written (1 - pt)^gamma (1 + gamma pt (-log pt) /
// (1 - pt)) -- two non-negative terms, no power with a negative exponent -- and f_p and the focal loss term are
// exactly 0 where 1 - pt is 0.
namespace {

constexpr int SL_FIXED = 6;                       // nll, sum of w[y], #out-of-range, smooth, #valid, focal
constexpr int SL_COLS = SL_FIXED + 3 * CMAX;      // + I_c, S_c, T_c

struct SlOpt {
  const float* cw;  // C class weights in device memory, or NULL = all ones
  float eps;        // label smoothing (gamma == 0 only)
  float ce, dice;   // the two coefficients
  float gamma;      // focal exponent
  float smooth;     // dice_smooth
};

inline bool sl_opt_ok(const SlOpt& o) {
  return std::isfinite(o.eps) && std::isfinite(o.ce) && std::isfinite(o.dice) && std::isfinite(o.gamma) &&
         std::isfinite(o.smooth) && o.eps >= 0.f && o.eps <= 1.f && o.ce >= 0.f && o.dice >= 0.f &&
         (o.ce > 0.f || o.dice > 0.f) && o.gamma >= 0.f && o.smooth > 0.f && !(o.eps > 0.f && o.gamma > 0.f);
}

template <int CP, typename T, bool EVAL>
__global__ __launch_bounds__(256) void sl_up_loss_kernel(const T* __restrict__ low, long ld, int N, int H, int W,
                                                         int C, const long long* __restrict__ labels, int Ho, int Wo,
                                                         float sh, float sw, int ignore_index,
                                                         float* __restrict__ part,
                                                         unsigned long long* __restrict__ confusion, SlOpt o) {
  constexpr int NR = SL_FIXED + 2 * CP;
  __shared__ float red[4][NR];
  __shared__ int tcnt[CP];
  __shared__ int hist[EVAL ? CMAX * CMAX : 1];
  if (threadIdx.x < CP) tcnt[threadIdx.x] = 0;
  if constexpr (EVAL) hist_clear(hist, C);
  __syncthreads();
  const long total = (long)N * Ho * Wo;
  float lsum = 0.f, cnt = 0.f, bad = 0.f, ssum = 0.f, val = 0.f, fsum = 0.f;
  float Ic[CP], Sc[CP];
#pragma unroll
  for (int c = 0; c < CP; ++c) Ic[c] = Sc[c] = 0.f;
  float w[CP];
  const float wsum = class_weights<CP>(o.cw, C, w);
  const bool focal = o.gamma > 0.f;
  for (long p = blockIdx.x * (long)blockDim.x + threadIdx.x; p < total; p += (long)gridDim.x * blockDim.x) {
    const long long y = labels[p];
    if (y == ignore_index) continue;
    if (y < 0 || y >= C) {
      bad += 1.f;
      continue;
    }
    const Pix px = pixel_of(p, Ho, Wo);
    float z[CP];
    full_res_logits<CP, T>(low, ld, H, W, px.n, px.r, px.s, sh, sw, z);
    float m, se, zy;
    softmax_stats<CP>(z, C, (int)y, m, se, zy, false);
    const float inv = 1.f / se;
    const float wy = pick<CP>(w, (int)y);
    float wz = 0.f, rest = 0.f;
#pragma unroll
    for (int c = 0; c < CP; ++c) {
      const bool lab = c == (int)y;
      const float d = z[c] - m;
      const float e = c < C ? expf(d) : 0.f;  // the padded lanes may hold anything
      rest += lab ? 0.f : e;                  // sum_{c != y} e_c
      if (c < C) wz = __builtin_fmaf(w[c], d, wz);
      const float sc = e * inv;
      Sc[c] += sc;
      Ic[c] += lab ? sc : 0.f;
    }
    const float lse = logf(se);
    const float nlp = m + lse - zy;  // -log pt
    lsum = __builtin_fmaf(wy, nlp, lsum);
    cnt += wy;
    ssum += __builtin_fmaf(wsum, lse, -wz);
    val += 1.f;
    if (focal) {
      const float omp = rest * inv;  // 1 - pt
      const float pw = omp > 0.f ? powf(omp, o.gamma) : 0.f;
      fsum = __builtin_fmaf(wy * pw, nlp, fsum);
    }
    atomicAdd(&tcnt[(int)y], 1);
    if constexpr (EVAL) hist_count(hist, C, (int)y, argmax_real<CP>(z, C));
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  lsum = wave_sum(lsum);
  cnt = wave_sum(cnt);
  bad = wave_sum(bad);
  ssum = wave_sum(ssum);
  val = wave_sum(val);
  fsum = wave_sum(fsum);
  if (lane == 0) {
    red[wave][0] = lsum; red[wave][1] = cnt; red[wave][2] = bad;
    red[wave][3] = ssum; red[wave][4] = val; red[wave][5] = fsum;
  }
#pragma unroll
  for (int c = 0; c < CP; ++c) {
    const float vi = wave_sum(Ic[c]), vs = wave_sum(Sc[c]);
    if (lane == 0) { red[wave][SL_FIXED + c] = vi; red[wave][SL_FIXED + CP + c] = vs; }
  }
  __syncthreads();  // also closes tcnt and the histogram
  const long nb = gridDim.x;
  if (threadIdx.x < NR) {
    const int j = threadIdx.x;
    const float v = red[0][j] + red[1][j] + red[2][j] + red[3][j];
    if (j < SL_FIXED)
      part[j * nb + blockIdx.x] = v;
    else if (j < SL_FIXED + CP) {
      if (j - SL_FIXED < C) part[(long)j * nb + blockIdx.x] = v;  // I_c: column 6 + c
    } else if (j - SL_FIXED - CP < C)
      part[(long)(j - CP + C) * nb + blockIdx.x] = v;                // S_c: column 6 + C + c
  }
  if (threadIdx.x < C) part[(long)(SL_FIXED + 2 * C + threadIdx.x) * nb + blockIdx.x] = (float)tcnt[threadIdx.x];
  if constexpr (EVAL) hist_flush(hist, C, confusion);
}

// One block, four waves: each wave sums whole columns of the partials in fp64, thread 0 forms the stats and the
// coefficient table from the 6 + 3 C totals.
__global__ __launch_bounds__(256) void sl_finalize_kernel(const float* __restrict__ part, int nblk, int C, float eps,
                                                          float ce, float dice, float gamma, float smooth,
                                                          float* __restrict__ out, float* __restrict__ table) {
  __shared__ double tot[SL_COLS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ncol = SL_FIXED + 3 * C;
  for (int col = wave; col < ncol; col += 4) {
    double a[1];
    column_sums_f64<1>(part + (long)col * nblk, nblk, 1, a);
    if (lane == 0) tot[col] = a[0];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double l = tot[0], d = tot[1], b = tot[2], sm = tot[3], v = tot[4], f = tot[5];
    const double* I = tot + SL_FIXED;
    const double* S = I + C;
    const double* Tc = S + C;
    int M = 0;
    for (int c = 0; c < C; ++c) M += Tc[c] > 0.0 ? 1 : 0;
    const double Mx = M > 0 ? (double)M : 1.0;
    double dsum = 0.0;
    for (int c = 0; c < CMAX; ++c) {
      float a_c = 0.f, b_c = 0.f;
      if (c < C && Tc[c] > 0.0) {
        const double U = S[c] + Tc[c] + (double)smooth;
        const double num = 2.0 * I[c] + (double)smooth;
        dsum += 1.0 - num / U;
        a_c = (float)(2.0 / (Mx * U));
        b_c = (float)(num / (Mx * U * U));
      }
      table[c] = a_c;
      table[CMAX + c] = b_c;
    }
    const double Dice = dsum / Mx;
    const double num = gamma > 0.f ? f : eps > 0.f ? (1.0 - (double)eps) * l + ((double)eps / C) * sm : l;
    const double F = num / d;  // 0/0 = nan when no valid pixel carries weight, as aten
    double loss = 0.0;
    if (ce > 0.f) loss += (double)ce * F;
    if (dice > 0.f) loss += (double)dice * Dice;
    out[0] = b > 0.0 ? __builtin_nanf("") : (float)loss;
    out[1] = (float)d;
    out[2] = (float)b;
    out[3] = (float)v;
    out[4] = (float)F;
    out[5] = (float)Dice;
  }
}

template <int CP, typename T>
__global__ __launch_bounds__(256) void sl_up_grad_kernel(const T* __restrict__ low, long ld, int N, int H, int W,
                                                         int C, const long long* __restrict__ labels, int Ho, int Wo,
                                                         float sh, float sw, int ignore_index,
                                                         const float* __restrict__ gout,
                                                         const float* __restrict__ stats,
                                                         const float* __restrict__ table, T* __restrict__ dhigh,
                                                         long ldh, SlOpt o) {
  const long total = (long)N * Ho * Wo;
  const bool poisoned = stats[2] > 0.f, has_ce = o.ce > 0.f, has_dice = o.dice > 0.f, focal = o.gamma > 0.f;
  const float sce = poisoned ? __builtin_nanf("") : has_ce ? gout[0] * o.ce / stats[1] : 0.f;  // (g / D) ce
  const float sdi = poisoned ? __builtin_nanf("") : gout[0] * o.dice;                           // g dice
  float w[CP];
  const float wsum = class_weights<CP>(o.cw, C, w);
  const float keep = 1.f - o.eps, spread = o.eps / (float)C;
  for (long p = blockIdx.x * (long)blockDim.x + threadIdx.x; p < total; p += (long)gridDim.x * blockDim.x) {
    const long long y = labels[p];
    T* d = dhigh + p * ldh;
    if (y == ignore_index || y < 0 || y >= C) {
      zero_row<CP, false>(d);
      continue;
    }
    const Pix px = pixel_of(p, Ho, Wo);
    float z[CP];
    full_res_logits<CP, T>(low, ld, H, W, px.n, px.r, px.s, sh, sw, z);
    float m, se, zy;
    softmax_stats<CP>(z, C, (int)y, m, se, zy, true);  // z[c] = e_c now
    const float inv = 1.f / se;
    const float wy = pick<CP>(w, (int)y), ey = pick<CP>(z, (int)y);
    float rest = 0.f, ay = 0.f, sb = 0.f;
#pragma unroll
    for (int c = 0; c < CP; ++c) {
      const bool lab = c == (int)y;
      rest += lab ? 0.f : z[c];
      if (has_dice) {
        ay = lab ? table[c] : ay;
        sb = __builtin_fmaf(table[CMAX + c], z[c] * inv, sb);  // sum_c b_c s_c (b is 0 on the padded lanes, as e is)
      }
    }
    const float omp = rest * inv, sy = ey * inv;  // 1 - pt, pt
    const float sq = __builtin_fmaf(-ay, sy, sb);  // sum_c q_c s_c
    float fp = 1.f;
    if (focal) {
      const float nlp = m + logf(se) - zy;
      fp = omp > 0.f ? powf(omp, o.gamma) * __builtin_fmaf(o.gamma * sy, nlp / omp, 1.f) : 0.f;
    }
    const float kw = keep * wy * fp;
#pragma unroll
    for (int c = 0; c < CP; c += 4) {
      f32x4 ov;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int cc = c + j;
        const bool lab = cc == (int)y;
        const float sk = z[cc] * inv;
        const float nl = lab ? -omp : sk;  // s_k - [k = y]
        float g = sce * __builtin_fmaf(spread, __builtin_fmaf(sk, wsum, -w[cc]), kw * nl);
        if (has_dice) {
          const float q = table[CMAX + cc] - (lab ? ay : 0.f);
          g = __builtin_fmaf(sdi * sk, q - sq, g);
        }
        ov[j] = cc < C ? g : 0.f;
      }
      st4(d + c, ov);
    }
  }
}

template <typename T, bool EVAL>
int sl_loss_impl(const T* low, long ld, int N, int H, int W, int C, const long long* labels, int Ho, int Wo,
                 int ignore_index, SlOpt o, float* work, float* out6, float* table, long long* confusion,
                 hipStream_t stream) {
  if (!loss_geom_ok(ld, C) || (EVAL && !confusion) || !sl_opt_ok(o)) return (int)hipErrorInvalidValue;
  const int nb = loss_blocks((long)N * Ho * Wo);
  const UpScale up = up_scale(H, W, Ho, Wo);
  SEG_LAUNCH_CP(C, sl_up_loss_kernel, (T, EVAL), nb, stream, low, ld, N, H, W, C, labels, Ho, Wo, up.sh, up.sw,
                ignore_index, work, (unsigned long long*)confusion, o)
  hipLaunchKernelGGL(sl_finalize_kernel, dim3(1), dim3(256), 0, stream, work, nb, C, o.eps, o.ce, o.dice, o.gamma,
                     o.smooth, out6, table);
  SEG_RET_LAST();
}

template <typename T>
int sl_grad_impl(const T* low, long ld, int N, int H, int W, int C, const long long* labels, int Ho, int Wo,
                 int ignore_index, SlOpt o, const float* grad_out, const float* stats, const float* table, T* dhigh,
                 long ldh, hipStream_t stream) {
  if (!loss_geom_ok(ld, C) || !rows_ok(ldh, C) || !sl_opt_ok(o)) return (int)hipErrorInvalidValue;
  const UpScale up = up_scale(H, W, Ho, Wo);
  SEG_LAUNCH_CP(C, sl_up_grad_kernel, (T), grad_blocks((long)N * Ho * Wo), stream, low, ld, N, H, W, C, labels, Ho,
                Wo, up.sh, up.sw, ignore_index, grad_out, stats, table, dhigh, ldh, o)
  SEG_RET_LAST();
}

}  // namespace

// out6 = [loss, D, #out-of-range labels, #valid, F, Dice]; table: 64 floats (a_c at c, b_c at 32 + c), written by
// the finalize, read by seg_sl_upsample_grad; `work` >= seg_sl_workspace_floats(N*Ho*Wo).
SEG_API long seg_sl_workspace_floats(long pixels) { return (long)SL_COLS * loss_blocks(pixels); }

SEG_API int seg_sl_upsample_loss(const float* low, long ld, int N, int H, int W, int C, const long long* labels, int Ho,
                                 int Wo, int ignore_index, const float* class_weight, float label_smoothing, float ce,
                                 float dice, float focal_gamma, float dice_smooth, float* work, float* out6,
                                 float* table, hipStream_t stream) {
  return sl_loss_impl<float, false>(low, ld, N, H, W, C, labels, Ho, Wo, ignore_index,
                                    SlOpt{class_weight, label_smoothing, ce, dice, focal_gamma, dice_smooth}, work,
                                    out6, table, nullptr, stream);
}
SEG_API int seg_sl_upsample_loss_bf16io(const __bf16* low, long ld, int N, int H, int W, int C,
                                        const long long* labels, int Ho, int Wo, int ignore_index,
                                        const float* class_weight, float label_smoothing, float ce, float dice,
                                        float focal_gamma, float dice_smooth, float* work, float* out6, float* table,
                                        hipStream_t stream) {
  return sl_loss_impl<__bf16, false>(low, ld, N, H, W, C, labels, Ho, Wo, ignore_index,
                                     SlOpt{class_weight, label_smoothing, ce, dice, focal_gamma, dice_smooth}, work,
                                     out6, table, nullptr, stream);
}
SEG_API int seg_sl_upsample_eval(const float* low, long ld, int N, int H, int W, int C, const long long* labels, int Ho,
                                 int Wo, int ignore_index, const float* class_weight, float label_smoothing, float ce,
                                 float dice, float focal_gamma, float dice_smooth, float* work, float* out6,
                                 float* table, long long* confusion, hipStream_t stream) {
  return sl_loss_impl<float, true>(low, ld, N, H, W, C, labels, Ho, Wo, ignore_index,
                                   SlOpt{class_weight, label_smoothing, ce, dice, focal_gamma, dice_smooth}, work,
                                   out6, table, confusion, stream);
}
SEG_API int seg_sl_upsample_eval_bf16io(const __bf16* low, long ld, int N, int H, int W, int C,
                                        const long long* labels, int Ho, int Wo, int ignore_index,
                                        const float* class_weight, float label_smoothing, float ce, float dice,
                                        float focal_gamma, float dice_smooth, float* work, float* out6, float* table,
                                        long long* confusion, hipStream_t stream) {
  return sl_loss_impl<__bf16, true>(low, ld, N, H, W, C, labels, Ho, Wo, ignore_index,
                                    SlOpt{class_weight, label_smoothing, ce, dice, focal_gamma, dice_smooth}, work,
                                    out6, table, confusion, stream);
}
SEG_API int seg_sl_upsample_grad(const float* low, long ld, int N, int H, int W, int C, const long long* labels, int Ho,
                                 int Wo, int ignore_index, const float* class_weight, float label_smoothing, float ce,
                                 float dice, float focal_gamma, const float* grad_out, const float* stats,
                                 const float* table, float* dhigh, long ldh, hipStream_t stream) {
  return sl_grad_impl(low, ld, N, H, W, C, labels, Ho, Wo, ignore_index,
                      SlOpt{class_weight, label_smoothing, ce, dice, focal_gamma, 1.f}, grad_out, stats, table, dhigh,
                      ldh, stream);
}
SEG_API int seg_sl_upsample_grad_bf16io(const __bf16* low, long ld, int N, int H, int W, int C,
                                        const long long* labels, int Ho, int Wo, int ignore_index,
                                        const float* class_weight, float label_smoothing, float ce, float dice,
                                        float focal_gamma, const float* grad_out, const float* stats,
                                        const float* table, __bf16* dhigh, long ldh, hipStream_t stream) {
  return sl_grad_impl(low, ld, N, H, W, C, labels, Ho, Wo, ignore_index,
                      SlOpt{class_weight, label_smoothing, ce, dice, focal_gamma, 1.f}, grad_out, stats, table, dhigh,
                      ldh, stream);
}

// ---- online hard example mining: seg_ohem_* (the criterion is seg_amd.OhemCELoss) ----
// Over the valid pixels V, with l_p = lse_p - z_p[y_p] the unweighted cross-entropy, tau = -log(thresh) and
// k = min(min_kept, |V|):
//   lambda = the k-th largest l_p over V,   K = {p in V : l_p > tau or l_p >= lambda}   (a tie group at lambda whole),
//   D = sum_K w[y_p],   loss = sum_K w[y_p] l_p / D,   d loss / d z_p = g w[y_p] (softmax(z_p) - onehot(y_p)) / D on K, 0 elsewhere.
// l_p >= 0 in fp32 (se >= 1 and m >= z_y, every rounding monotone), so its low 31 bits are an unsigned key in the
// order of the values, and lambda is found exactly by a radix select over three digits of 11 / 10 / 10 bits:
//   1. the loss pass stores l_p (4 B per pixel, -1 for an ignored or out-of-range label) at the front of `work`,
//      counts #valid, #out-of-range and #{l_p > tau}, and histograms the top digit (per-block LDS histogram, its
//      non-zero bins added to the global one);
//   2. two refine passes over the 4 B per pixel: every block finds the bin of the k-th largest in the last
//      histogram for itself (one scan of <= 2048 counters from L2, the same result in every block; block 0 leaves it
//      in `work` for the next launch) and histograms the next digit of the pixels in that bin.  When #{l_p > tau}
//      already reaches k, K = {l_p > tau} and lambda is not needed: both passes return at once (the launch
//      sequence is fixed, the tape replays it);
//   3. the reduce pass picks the last digit -- lambda is exact -- and sums w[y] l and w[y] over K into per-block
//      partials; one fp64 finalize writes stats = [loss, D, #out-of-range, #valid, #kept, cut], cut = min(tau, lambda).
// The gradient kernel reads the keep decision from the stored l_p, tau and lambda (in `work`; +inf in threshold
// mode), so forward and backward agree on K by construction.
// work: [pixels] l_p | OH_CTL words of histograms and counters (cleared on the stream by every call) | 2 floats per block.
namespace {

constexpr int OH_B0 = 2048, OH_B1 = 1024, OH_B2 = 1024;  // bins of key >> 20, (key >> 10) & 1023, key & 1023
constexpr int OH_H1 = OH_B0, OH_H2 = OH_B0 + OH_B1, OH_CNT = OH_B0 + OH_B1 + OH_B2;
// counters behind the histograms: #valid, #out-of-range, #{l > tau}, #kept, then the select's state
enum { OH_VALID = 0, OH_BAD, OH_ABOVE, OH_KEPT, OH_BIN0, OH_NEED0, OH_BIN1, OH_NEED1, OH_LAMBDA, OH_NCNT = 16 };
constexpr int OH_CTL = OH_CNT + OH_NCNT;
constexpr unsigned OH_INF = 0x7f800000u;

__device__ __forceinline__ unsigned oh_key(float l) { return __float_as_uint(l) & 0x7fffffffu; }
__device__ __forceinline__ bool oh_valid(float l) { return l != -1.f; }
__device__ __forceinline__ bool oh_keep(float l, float tau, float lambda) { return l > tau || l >= lambda; }

// k = min(min_kept, #valid); threshold mode (nothing to select) when no pixel is valid or #{l > tau} >= k
__device__ __forceinline__ bool oh_select(const unsigned* __restrict__ cnt, long min_kept, unsigned& k) {
  const unsigned nv = cnt[OH_VALID];
  k = (unsigned)(min_kept < (long)nv ? min_kept : (long)nv);
  return nv > 0 && cnt[OH_ABOVE] < k;
}

// Block-wide (256 threads): the bin of the need-th largest entry of hist[NB] (1 <= need <= its total), counted from
// the top bin down, and the rank that is left inside that bin.  s: 6 words of LDS.
template <int NB>
__device__ __forceinline__ void oh_pick(const unsigned* __restrict__ hist, unsigned need, unsigned* s, unsigned& bin,
                                        unsigned& rest) {
  constexpr int PER = NB / 256;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  unsigned c[PER], sum = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    c[j] = hist[NB - 1 - (t * PER + j)];
    sum += c[j];
  }
  unsigned incl = sum;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned v = __shfl_up(incl, o, 64);
    if (lane >= o) incl += v;
  }
  if (t == 0) { s[4] = 0; s[5] = 1; }
  if (lane == 63) s[wave] = incl;
  __syncthreads();
  for (int w = 0; w < wave; ++w) incl += s[w];
  unsigned acc = incl - sum;
  if (acc < need && need <= incl) {
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      if (acc < need && need <= acc + c[j]) { s[4] = NB - 1 - (t * PER + j); s[5] = need - acc; }
      acc += c[j];
    }
  }
  __syncthreads();
  bin = s[4];
  rest = s[5];
  __syncthreads();
}

// EVAL: also the confusion matrix of seg_ce_upsample_eval (over all valid pixels, not over K).
template <int CP, typename T, bool EVAL>
__global__ __launch_bounds__(256) void oh_up_loss_kernel(const T* __restrict__ low, long ld, int N, int H, int W,
                                                         int C, const long long* __restrict__ labels, int Ho, int Wo,
                                                         float sh, float sw, int ignore_index, float tau,
                                                         float* __restrict__ lbuf, unsigned* __restrict__ ctl,
                                                         unsigned long long* __restrict__ confusion) {
  __shared__ unsigned h0[OH_B0];
  __shared__ unsigned cnt[3];
  __shared__ int hist[EVAL ? CMAX * CMAX : 1];
  for (int i = threadIdx.x; i < OH_B0; i += blockDim.x) h0[i] = 0;
  if (threadIdx.x < 3) cnt[threadIdx.x] = 0;
  if constexpr (EVAL) hist_clear(hist, C);
  __syncthreads();
  const long total = (long)N * Ho * Wo;
  unsigned nvalid = 0, nbad = 0, nabove = 0;
  for (long p = blockIdx.x * (long)blockDim.x + threadIdx.x; p < total; p += (long)gridDim.x * blockDim.x) {
    const long long y = labels[p];
    if (y == ignore_index || y < 0 || y >= C) {
      nbad += y == ignore_index ? 0u : 1u;
      lbuf[p] = -1.f;
      continue;
    }
    const Pix px = pixel_of(p, Ho, Wo);
    float z[CP];
    full_res_logits<CP, T>(low, ld, H, W, px.n, px.r, px.s, sh, sw, z);
    float m, se, zy;
    softmax_stats<CP>(z, C, (int)y, m, se, zy, false);
    const float l = m + logf(se) - zy;  // the plain kernel's per-pixel term
    lbuf[p] = l;
    nvalid += 1u;
    nabove += l > tau ? 1u : 0u;
    atomicAdd(&h0[oh_key(l) >> 20], 1u);
    if constexpr (EVAL) {  // argmax_real's text: through the call, two bf16 instantiations lose a wave of occupancy
      int pred = 0;
      float best = z[0];
#pragma unroll
      for (int c = 1; c < CP; ++c)
        if (c < C && z[c] > best) {
          best = z[c];
          pred = c;
        }
      hist_count(hist, C, (int)y, pred);
    }
  }
  if (nvalid) atomicAdd(&cnt[0], nvalid);
  if (nbad) atomicAdd(&cnt[1], nbad);
  if (nabove) atomicAdd(&cnt[2], nabove);
  __syncthreads();
  for (int i = threadIdx.x; i < OH_B0; i += blockDim.x) {
    const unsigned v = h0[i];
    if (v) atomicAdd(ctl + i, v);
  }
  if (threadIdx.x < 3 && cnt[threadIdx.x]) atomicAdd(ctl + OH_CNT + threadIdx.x, cnt[threadIdx.x]);
  if constexpr (EVAL) hist_flush(hist, C, confusion);
}

// LEVEL 1: pick the top digit's bin from the loss pass's histogram, histogram the middle digit of its pixels.
// LEVEL 2: pick the middle digit's bin, histogram the last digit.
template <int LEVEL>
__global__ __launch_bounds__(256) void oh_refine_kernel(const float* __restrict__ lbuf, long total, long min_kept,
                                                        unsigned* __restrict__ ctl) {
  __shared__ unsigned h[OH_B1];
  __shared__ unsigned s[6];
  unsigned* cnt = ctl + OH_CNT;
  unsigned k;
  if (!oh_select(cnt, min_kept, k)) return;  // threshold mode: the same answer in every thread of every block
  unsigned bin, rest, prefix;
  if constexpr (LEVEL == 1) {
    oh_pick<OH_B0>(ctl, k, s, bin, rest);
    prefix = bin;
    if (blockIdx.x == 0 && threadIdx.x == 0) { cnt[OH_BIN0] = bin; cnt[OH_NEED0] = rest; }
  } else {
    oh_pick<OH_B1>(ctl + OH_H1, cnt[OH_NEED0], s, bin, rest);
    prefix = (cnt[OH_BIN0] << 10) | bin;
    if (blockIdx.x == 0 && threadIdx.x == 0) { cnt[OH_BIN1] = bin; cnt[OH_NEED1] = rest; }
  }
  constexpr int SHIFT = LEVEL == 1 ? 10 : 0;  // of this level's digit; the prefix is everything above it
  for (int i = threadIdx.x; i < OH_B1; i += blockDim.x) h[i] = 0;
  __syncthreads();
  for (long p = blockIdx.x * (long)blockDim.x + threadIdx.x; p < total; p += (long)gridDim.x * blockDim.x) {
    const float l = lbuf[p];
    const unsigned key = oh_key(l);
    if (oh_valid(l) && (key >> (SHIFT + 10)) == prefix) atomicAdd(&h[(key >> SHIFT) & 1023u], 1u);
  }
  __syncthreads();
  unsigned* out = ctl + (LEVEL == 1 ? OH_H1 : OH_H2);
  for (int i = threadIdx.x; i < OH_B1; i += blockDim.x) {
    const unsigned v = h[i];
    if (v) atomicAdd(out + i, v);
  }
}

// lambda from the last digit (+inf in threshold mode), then this block's sums of w[y] l and w[y] over K.
__global__ __launch_bounds__(256) void oh_reduce_kernel(const float* __restrict__ lbuf,
                                                        const long long* __restrict__ labels, long total,
                                                        long min_kept, float tau, const float* __restrict__ cw,
                                                        unsigned* __restrict__ ctl, float* __restrict__ part) {
  __shared__ unsigned s[6];
  __shared__ float red[4][2];
  __shared__ unsigned kept;
  unsigned* cnt = ctl + OH_CNT;
  unsigned k, lbits = OH_INF;
  if (oh_select(cnt, min_kept, k)) {
    unsigned bin, rest;
    oh_pick<OH_B2>(ctl + OH_H2, cnt[OH_NEED1], s, bin, rest);
    lbits = (cnt[OH_BIN0] << 20) | (cnt[OH_BIN1] << 10) | bin;
  }
  const float lambda = __uint_as_float(lbits);
  if (threadIdx.x == 0) kept = 0;
  __syncthreads();
  float lsum = 0.f, dsum = 0.f;
  unsigned nk = 0;
  for (long p = blockIdx.x * (long)blockDim.x + threadIdx.x; p < total; p += (long)gridDim.x * blockDim.x) {
    const float l = lbuf[p];
    if (!oh_valid(l) || !oh_keep(l, tau, lambda)) continue;
    const float wy = cw ? cw[labels[p]] : 1.f;  // a valid pixel's label is in [0, C)
    lsum = __builtin_fmaf(wy, l, lsum);
    dsum += wy;
    nk += 1u;
  }
  if (nk) atomicAdd(&kept, nk);
  const float v[2] = {lsum, dsum};
  block_partials<2>(v, red, part);  // its barrier also closes `kept`
  if (threadIdx.x == 0) {
    if (kept) atomicAdd(cnt + OH_KEPT, kept);
    if (blockIdx.x == 0) cnt[OH_LAMBDA] = lbits;
  }
}

// out6 = [loss, D, #out-of-range labels, #valid, #kept, cut = min(tau, lambda)]
__global__ void oh_finalize_kernel(const float* __restrict__ part, int nblk, float tau,
                                   const unsigned* __restrict__ ctl, float* out) {
  double t[2];
  column_sums_f64<2>(part, nblk, 2, t);
  const double l = t[0], d = t[1];
  if (threadIdx.x == 0) {
    const unsigned* cnt = ctl + OH_CNT;
    out[0] = cnt[OH_BAD] > 0 ? __builtin_nanf("") : (float)(l / d);  // 0/0 = nan when nothing is kept, as aten
    out[1] = (float)d;
    out[2] = (float)cnt[OH_BAD];
    out[3] = (float)cnt[OH_VALID];
    out[4] = (float)cnt[OH_KEPT];
    out[5] = fminf(tau, __uint_as_float(cnt[OH_LAMBDA]));
  }
}

// dhigh[p][c] = g w[y_p] (softmax(z_p)[c] - [c == y_p]) / D on K (read from the stored l_p), zeros elsewhere: the
// weighted gradient kernel's expression, scale * (w[y] * (softmax - onehot)), so on K the rows are what
// seg_cew_upsample_grad writes for the labels with every pixel outside K ignored.  NCHW: the bf16io twin (store_quad).
template <int CP, typename T, bool NCHW>
__global__ __launch_bounds__(256) void oh_up_grad_kernel(const T* __restrict__ low, long ld, int N, int H, int W,
                                                         int C, const long long* __restrict__ labels, int Ho, int Wo,
                                                         float sh, float sw, float tau, const float* __restrict__ cw,
                                                         const float* __restrict__ lbuf,
                                                         const unsigned* __restrict__ ctl,
                                                         const float* __restrict__ gout,
                                                         const float* __restrict__ stats, void* __restrict__ dout,
                                                         long ldh) {
  const long total = (long)N * Ho * Wo;
  const long plane = (long)Ho * Wo;
  const float scale = ce_scale(stats, gout);
  const float lambda = __uint_as_float(ctl[OH_CNT + OH_LAMBDA]);
  float w[CP];
  class_weights<CP>(cw, C, w);
  for (long p = blockIdx.x * (long)blockDim.x + threadIdx.x; p < total; p += (long)gridDim.x * blockDim.x) {
    const float l = lbuf[p];
    const Pix px = pixel_of(p, Ho, Wo);
    T* d = static_cast<T*>(dout) + p * ldh;
    float* dn = static_cast<float*>(dout) + (long)px.n * C * plane + px.rem;
    if (!oh_valid(l) || !oh_keep(l, tau, lambda)) {
      zero_row<CP, NCHW>(d, dn, C, plane);
      continue;
    }
    const int y = (int)labels[p];
    float z[CP];
    full_res_logits<CP, T>(low, ld, H, W, px.n, px.r, px.s, sh, sw, z);
    float m, se, zy;
    softmax_stats<CP>(z, C, y, m, se, zy, true);
    const float inv = 1.f / se;
    const float wy = pick<CP>(w, y);
#pragma unroll
    for (int c = 0; c < CP; c += 4) {
      f32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int cc = c + j;
        o[j] = cc < C ? scale * (wy * __builtin_fmaf(z[cc], inv, cc == y ? -1.f : -0.f)) : 0.f;
      }
      store_quad<NCHW>(d, dn, c, C, plane, o);
    }
  }
}

inline bool oh_args_ok(long ld, int C, long total, float tau, long min_kept) {
  return loss_geom_ok(ld, C) && total >= 0 && total < (1L << 31) && std::isfinite(tau) && tau >= 0.f && min_kept >= 1;
}

template <typename T, bool EVAL>
int oh_loss_impl(const T* low, long ld, int N, int H, int W, int C, const long long* labels, int Ho, int Wo,
                 int ignore_index, const float* cw, float tau, long min_kept, float* work, float* out6,
                 long long* confusion, hipStream_t stream) {
  const long total = (long)N * Ho * Wo;
  if (!oh_args_ok(ld, C, total, tau, min_kept) || (EVAL && !confusion)) return (int)hipErrorInvalidValue;
  const int nb = loss_blocks(total);
  const UpScale up = up_scale(H, W, Ho, Wo);
  float* lbuf = work;
  unsigned* ctl = reinterpret_cast<unsigned*>(work + total);
  float* part = work + total + OH_CTL;
  // every call clears its histograms and counters on the stream: a replayed tape never sees the last step's bins
  const hipError_t e = hipMemsetAsync(ctl, 0, sizeof(unsigned) * OH_CTL, stream);
  if (e != hipSuccess) return (int)e;
  SEG_LAUNCH_CP(C, oh_up_loss_kernel, (T, EVAL), nb, stream, low, ld, N, H, W, C, labels, Ho, Wo, up.sh, up.sw,
                ignore_index, tau, lbuf, ctl, (unsigned long long*)confusion)
  hipLaunchKernelGGL(oh_refine_kernel<1>, dim3(nb), dim3(256), 0, stream, lbuf, total, min_kept, ctl);
  hipLaunchKernelGGL(oh_refine_kernel<2>, dim3(nb), dim3(256), 0, stream, lbuf, total, min_kept, ctl);
  hipLaunchKernelGGL(oh_reduce_kernel, dim3(nb), dim3(256), 0, stream, lbuf, labels, total, min_kept, tau, cw, ctl,
                     part);
  hipLaunchKernelGGL(oh_finalize_kernel, dim3(1), dim3(64), 0, stream, part, nb, tau, ctl, out6);
  SEG_RET_LAST();
}

template <typename T, bool NCHW>
int oh_grad_impl(const T* low, long ld, int N, int H, int W, int C, const long long* labels, int Ho, int Wo,
                 const float* cw, float tau, const float* work, const float* grad_out, const float* stats, void* dhigh,
                 long ldh, hipStream_t stream) {
  const long total = (long)N * Ho * Wo;
  if (!oh_args_ok(ld, C, total, tau, 1) || (!NCHW && !rows_ok(ldh, C))) return (int)hipErrorInvalidValue;
  const UpScale up = up_scale(H, W, Ho, Wo);
  const unsigned* ctl = reinterpret_cast<const unsigned*>(work + total);
  SEG_LAUNCH_CP(C, oh_up_grad_kernel, (T, NCHW), grad_blocks(total), stream, low, ld, N, H, W, C, labels, Ho, Wo,
                up.sh, up.sw, tau, cw, work, ctl, grad_out, stats, dhigh, ldh)
  SEG_RET_LAST();
}

}  // namespace

// out6 = [loss, D, #out-of-range labels, #valid, #kept, cut]; loss_thresh is tau = -log(thresh); the first `pixels`
// floats of `work` (>= seg_ohem_workspace_floats(N*Ho*Wo)) are the per-pixel losses, which seg_ohem_upsample_grad
// reads back together with lambda.
SEG_API long seg_ohem_workspace_floats(long pixels) { return pixels + OH_CTL + 2L * loss_blocks(pixels); }

SEG_API int seg_ohem_upsample_loss(const float* low, long ld, int N, int H, int W, int C, const long long* labels,
                                   int Ho, int Wo, int ignore_index, const float* class_weight, float loss_thresh,
                                   long min_kept, float* work, float* out6, hipStream_t stream) {
  return oh_loss_impl<float, false>(low, ld, N, H, W, C, labels, Ho, Wo, ignore_index, class_weight, loss_thresh,
                                    min_kept, work, out6, nullptr, stream);
}
SEG_API int seg_ohem_upsample_loss_bf16io(const __bf16* low, long ld, int N, int H, int W, int C,
                                          const long long* labels, int Ho, int Wo, int ignore_index,
                                          const float* class_weight, float loss_thresh, long min_kept, float* work,
                                          float* out6, hipStream_t stream) {
  return oh_loss_impl<__bf16, false>(low, ld, N, H, W, C, labels, Ho, Wo, ignore_index, class_weight, loss_thresh,
                                     min_kept, work, out6, nullptr, stream);
}
SEG_API int seg_ohem_upsample_eval(const float* low, long ld, int N, int H, int W, int C, const long long* labels,
                                   int Ho, int Wo, int ignore_index, const float* class_weight, float loss_thresh,
                                   long min_kept, float* work, float* out6, long long* confusion,
                                   hipStream_t stream) {
  return oh_loss_impl<float, true>(low, ld, N, H, W, C, labels, Ho, Wo, ignore_index, class_weight, loss_thresh,
                                   min_kept, work, out6, confusion, stream);
}
SEG_API int seg_ohem_upsample_eval_bf16io(const __bf16* low, long ld, int N, int H, int W, int C,
                                          const long long* labels, int Ho, int Wo, int ignore_index,
                                          const float* class_weight, float loss_thresh, long min_kept, float* work,
                                          float* out6, long long* confusion, hipStream_t stream) {
  return oh_loss_impl<__bf16, true>(low, ld, N, H, W, C, labels, Ho, Wo, ignore_index, class_weight, loss_thresh,
                                    min_kept, work, out6, confusion, stream);
}
SEG_API int seg_ohem_upsample_grad(const float* low, long ld, int N, int H, int W, int C, const long long* labels,
                                   int Ho, int Wo, int ignore_index, const float* class_weight, float loss_thresh,
                                   const float* work, const float* grad_out, const float* stats, float* dhigh,
                                   long ldh, hipStream_t stream) {
  return oh_grad_impl<float, false>(low, ld, N, H, W, C, labels, Ho, Wo, class_weight, loss_thresh, work, grad_out,
                                    stats, dhigh, ldh, stream);
}
// The twin writes the full-resolution gradient as fp32 NCHW [N][C][Ho][Wo]: follow with
// seg_upsample_bwd_bf16io(nchw_grad = 1, ac = 1).
SEG_API int seg_ohem_upsample_grad_bf16io(const __bf16* low, long ld, int N, int H, int W, int C,
                                          const long long* labels, int Ho, int Wo, int ignore_index,
                                          const float* class_weight, float loss_thresh, const float* work,
                                          const float* grad_out, const float* stats, float* dhigh_nchw,
                                          hipStream_t stream) {
  return oh_grad_impl<__bf16, true>(low, ld, N, H, W, C, labels, Ho, Wo, class_weight, loss_thresh, work, grad_out,
                                    stats, dhigh_nchw, 0, stream);
}

// ---- knowledge distillation: seg_kd_* (the criterion is seg_amd.DistillLoss) ----
// A second low-resolution tensor, the teacher's logits (fp32 NHWC rows [N][Ht][Wt], leading dimension ldt), is
// upsampled to (Ho, Wo) by the same align_corners=True bilinear as the student's: full_res_logits on its own
// geometry.  (Ht, Wt) is independent of (H, W); with Ht == Ho the scale is 1 and the four taps are the pixel itself.
// Over the valid pixels V and the distilled pixels P (every pixel with kd_ignored, else V), with z_p / u_p the
// student's / teacher's full-resolution logits, s = softmax(z_p / T), q = softmax(u_p / T), w the class weights:
//   CE   = sum_V w[y_p] (lse(z_p) - z_p[y_p]) / D,   D = sum_V w[y_p],
//   KD   = T^2 / |P| sum_P sum_c q_c (log q_c - log s_c),
//   loss = ce CE + kd KD    (a term whose coefficient is 0 is left out, so its 0/0 never reaches the loss),
//   d loss / d z_p[c] = g [ce / D w[y_p] (softmax(z_p)_c - [c = y_p]) [p in V] + kd T / |P| (s_c - q_c) [p in P]].
// q and s come from one device function (kd_softmax) applied to u and to z: d_c = v_c / T - max, e_c = exp(d_c),
// the sum in ascending class order.  log q_c - log s_c is (du_c - log su) - (dz_c - log sz), so teacher logits that
// are bit for bit the student's give KD exactly 0 and s_c - q_c exactly 0.  v_c / T is v_c * (1 / T): one rounding
// of 1 / T on the host, exact for the powers of two.
// One pass writes five partials per block [nll, sum of w[y], #out-of-range, #valid, kd sum]; the fp64 finalize
// forms out6 = [loss, D, #out-of-range labels, #valid, CE, KD].  The gradient kernel reads D and #valid from it.
namespace {

struct KdOpt {
  const float* cw;  // C class weights in device memory, or NULL = all ones
  float ce, kd;     // the two coefficients
  float T;          // temperature
  int all;          // kd_ignored: P is every pixel (else the valid ones)
};

inline bool kd_opt_ok(const KdOpt& o) {
  return std::isfinite(o.ce) && std::isfinite(o.kd) && std::isfinite(o.T) && o.ce >= 0.f && o.kd > 0.f && o.T > 0.f;
}

// Teacher geometry: rows, leading dimension, size and the align_corners scales to (Ho, Wo).
struct KdTeacher {
  const float* rows;
  long ld;
  int H, W;
  float sh, sw;
};

// softmax(v / T) over the C real classes as d_c = v_c * invT - max and e_c = exp(d_c) (0 on the padded lanes, which
// may hold anything); returns sum_c e_c.
template <int CP>
__device__ __forceinline__ float kd_softmax(const float (&v)[CP], int C, float invT, float (&d)[CP], float (&e)[CP]) {
  float m = v[0] * invT;
#pragma unroll
  for (int c = 1; c < CP; ++c)
    if (c < C) m = fmaxf(m, v[c] * invT);
  float se = 0.f;
#pragma unroll
  for (int c = 0; c < CP; ++c) {
    d[c] = c < C ? v[c] * invT - m : 0.f;
    e[c] = c < C ? expf(d[c]) : 0.f;
    se += e[c];
  }
  return se;
}

template <int CP, typename T>
__global__ __launch_bounds__(256) void kd_up_loss_kernel(const T* __restrict__ low, long ld, int N, int H, int W,
                                                         int C, KdTeacher te, const long long* __restrict__ labels,
                                                         int Ho, int Wo, float sh, float sw, int ignore_index,
                                                         float* __restrict__ part, KdOpt o) {
  constexpr int NP = 5;
  __shared__ float red[4][NP];
  const long total = (long)N * Ho * Wo;
  float lsum = 0.f, cnt = 0.f, bad = 0.f, val = 0.f, ksum = 0.f;
  float w[CP];
  class_weights<CP>(o.cw, C, w);
  const float invT = 1.f / o.T;
  const bool has_ce = o.ce > 0.f;
  for (long p = blockIdx.x * (long)blockDim.x + threadIdx.x; p < total; p += (long)gridDim.x * blockDim.x) {
    const long long y = labels[p];
    const bool ign = y == ignore_index;
    const bool oob = !ign && (y < 0 || y >= C);
    if (oob) bad += 1.f;
    const bool valid = !ign && !oob;
    if (!valid && !o.all) continue;
    const Pix px = pixel_of(p, Ho, Wo);
    float z[CP], u[CP];
    full_res_logits<CP, T>(low, ld, H, W, px.n, px.r, px.s, sh, sw, z);
    full_res_logits<CP, float>(te.rows, te.ld, te.H, te.W, px.n, px.r, px.s, te.sh, te.sw, u);
    {
      float dz[CP], ez[CP], du[CP], eu[CP];
      const float sz = kd_softmax<CP>(z, C, invT, dz, ez);
      const float su = kd_softmax<CP>(u, C, invT, du, eu);
      const float lz = logf(sz), lu = logf(su), inv = 1.f / su;
      float k = 0.f;
#pragma unroll
      for (int c = 0; c < CP; ++c)
        if (c < C) k = __builtin_fmaf(eu[c] * inv, (du[c] - lu) - (dz[c] - lz), k);
      ksum += k;
    }
    if (valid) {
      val += 1.f;
      const float wy = pick<CP>(w, (int)y);
      cnt += wy;
      if (has_ce) {
        float m, se, zy;
        softmax_stats<CP>(z, C, (int)y, m, se, zy, false);
        lsum = __builtin_fmaf(wy, m + logf(se) - zy, lsum);
      }
    }
  }
  lsum = wave_sum(lsum);
  cnt = wave_sum(cnt);
  bad = wave_sum(bad);
  val = wave_sum(val);
  ksum = wave_sum(ksum);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    red[wave][0] = lsum; red[wave][1] = cnt; red[wave][2] = bad; red[wave][3] = val; red[wave][4] = ksum;
  }
  __syncthreads();
  if (threadIdx.x < NP) {
    const int j = threadIdx.x;
    part[NP * blockIdx.x + j] = red[0][j] + red[1][j] + red[2][j] + red[3][j];
  }
}

// out6 = [loss, D, #out-of-range labels, #valid pixels, CE, KD].  D is the sum of w[y] over V; |P| = total
// (kd_ignored) or #valid; 0/0 = nan as aten (CE is 0 and left out when ce == 0).
__global__ void kd_finalize_kernel(const float* __restrict__ part, int nblk, double total, float ce, float kd,
                                   float T, int all, float* out) {
  double t[5];
  column_sums_f64<5>(part, nblk, 5, t);
  const double l = t[0], c = t[1], b = t[2], v = t[3], k = t[4];
  if (threadIdx.x == 0) {
    const double P = all ? total : v;
    const double CE = ce > 0.f ? l / c : 0.0;
    const double KD = (double)T * (double)T * k / P;
    double loss = (double)kd * KD;
    if (ce > 0.f) loss += (double)ce * CE;
    out[0] = b > 0.0 ? __builtin_nanf("") : (float)loss;
    out[1] = (float)c;
    out[2] = (float)b;
    out[3] = (float)v;
    out[4] = (float)CE;
    out[5] = (float)KD;
  }
}

// NCHW (seg_kd_upsample_grad_bf16io_nchw): fp32 planes instead of T rows, as in the seg_ohem_* twin (store_quad).
template <int CP, typename T, bool NCHW>
__global__ __launch_bounds__(256) void kd_up_grad_kernel(const T* __restrict__ low, long ld, int N, int H, int W,
                                                         int C, KdTeacher te, const long long* __restrict__ labels,
                                                         int Ho, int Wo, float sh, float sw, int ignore_index,
                                                         const float* __restrict__ gout,
                                                         const float* __restrict__ stats, void* __restrict__ dout,
                                                         long ldh, KdOpt o) {
  const long plane = (long)Ho * Wo, total = (long)N * plane;
  const bool poisoned = stats[2] > 0.f, has_ce = o.ce > 0.f;
  const float nan = __builtin_nanf("");
  const float sce = poisoned ? nan : has_ce ? gout[0] * o.ce / stats[1] : 0.f;                  // g ce / D
  const float skd = poisoned ? nan : gout[0] * o.kd * o.T / (o.all ? (float)total : stats[3]);  // g kd T / |P|
  float w[CP];
  class_weights<CP>(o.cw, C, w);
  const float invT = 1.f / o.T;
  for (long p = blockIdx.x * (long)blockDim.x + threadIdx.x; p < total; p += (long)gridDim.x * blockDim.x) {
    const long long y = labels[p];
    const Pix px = pixel_of(p, Ho, Wo);
    T* d = static_cast<T*>(dout) + p * ldh;
    float* dn = static_cast<float*>(dout) + (long)px.n * C * plane + px.rem;
    const bool valid = !(y == ignore_index || y < 0 || y >= C);
    if (!valid && !o.all) {
      zero_row<CP, NCHW>(d, dn, C, plane);
      continue;
    }
    float z[CP], u[CP];
    full_res_logits<CP, T>(low, ld, H, W, px.n, px.r, px.s, sh, sw, z);
    full_res_logits<CP, float>(te.rows, te.ld, te.H, te.W, px.n, px.r, px.s, te.sh, te.sw, u);
    float dz[CP], ez[CP], du[CP], eu[CP];
    const float sz = kd_softmax<CP>(z, C, invT, dz, ez);
    const float su = kd_softmax<CP>(u, C, invT, du, eu);
    const float iz = 1.f / sz, iu = 1.f / su;
    const bool with_ce = valid && has_ce;
    float inv = 0.f, kw = 0.f;  // 1 / sum exp(z - max), (g ce / D) w[y]
    if (with_ce) {
      float m, se, zy;
      softmax_stats<CP>(z, C, (int)y, m, se, zy, true);  // z[c] = exp(z_c - max) now
      inv = 1.f / se;
      kw = pick<CP>(w, (int)y) * sce;
    }
#pragma unroll
    for (int c = 0; c < CP; c += 4) {
      f32x4 ov;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int cc = c + j;
        const float hard = with_ce ? kw * __builtin_fmaf(z[cc], inv, cc == (int)y ? -1.f : -0.f) : 0.f;
        ov[j] = cc < C ? __builtin_fmaf(skd, ez[cc] * iz - eu[cc] * iu, hard) : 0.f;
      }
      store_quad<NCHW>(d, dn, c, C, plane, ov);
    }
  }
}

inline bool kd_args_ok(long ld, int C, const float* teacher, long ldt, int Ht, int Wt, const KdOpt& o) {
  return loss_geom_ok(ld, C) && rows_ok(ldt, C) && Ht >= 1 && Wt >= 1 && teacher && kd_opt_ok(o);
}

inline KdTeacher kd_teacher(const float* teacher, long ldt, int Ht, int Wt, int Ho, int Wo) {
  const UpScale up = up_scale(Ht, Wt, Ho, Wo);
  return KdTeacher{teacher, ldt, Ht, Wt, up.sh, up.sw};
}

template <typename T>
int kd_loss_impl(const T* low, long ld, int N, int H, int W, int C, const float* teacher, long ldt, int Ht, int Wt,
                 const long long* labels, int Ho, int Wo, int ignore_index, KdOpt o, float* work, float* out6,
                 hipStream_t stream) {
  if (!kd_args_ok(ld, C, teacher, ldt, Ht, Wt, o)) return (int)hipErrorInvalidValue;
  const long total = (long)N * Ho * Wo;
  const int nb = loss_blocks(total);
  const UpScale up = up_scale(H, W, Ho, Wo);
  const KdTeacher te = kd_teacher(teacher, ldt, Ht, Wt, Ho, Wo);
  SEG_LAUNCH_CP(C, kd_up_loss_kernel, (T), nb, stream, low, ld, N, H, W, C, te, labels, Ho, Wo, up.sh, up.sw,
                ignore_index, work, o)
  hipLaunchKernelGGL(kd_finalize_kernel, dim3(1), dim3(64), 0, stream, work, nb, (double)total, o.ce, o.kd, o.T,
                     o.all, out6);
  SEG_RET_LAST();
}

template <typename T, bool NCHW = false>
int kd_grad_impl(const T* low, long ld, int N, int H, int W, int C, const float* teacher, long ldt, int Ht, int Wt,
                 const long long* labels, int Ho, int Wo, int ignore_index, KdOpt o, const float* grad_out,
                 const float* stats, void* dhigh, long ldh, hipStream_t stream) {
  if (!kd_args_ok(ld, C, teacher, ldt, Ht, Wt, o) || (!NCHW && !rows_ok(ldh, C))) return (int)hipErrorInvalidValue;
  const UpScale up = up_scale(H, W, Ho, Wo);
  const KdTeacher te = kd_teacher(teacher, ldt, Ht, Wt, Ho, Wo);
  SEG_LAUNCH_CP(C, kd_up_grad_kernel, (T, NCHW), grad_blocks((long)N * Ho * Wo), stream, low, ld, N, H, W, C, te,
                labels, Ho, Wo, up.sh, up.sw, ignore_index, grad_out, stats, dhigh, ldh, o)
  SEG_RET_LAST();
}

// out[row][c] = low[row][c] for c < C, 0 for C <= c < ldo: one thread per 4 channels of an output row.
template <typename T>
__global__ __launch_bounds__(256) void low_logits_kernel(const T* __restrict__ low, long ld, long rows, int C,
                                                         float* __restrict__ out, long ldo) {
  const long quads = ldo >> 2, total = rows * quads;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long row = i / quads;
    const int c = (int)(i - row * quads) * 4;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (c < C) {
      const f32x4 x = ld4(low + row * ld + c);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = c + j < C ? x[j] : 0.f;
    }
    st4(out + row * ldo + c, v);
  }
}

template <typename T>
int low_logits_impl(const T* low, long ld, long rows, int C, float* out, long ldo, hipStream_t stream) {
  if ((ld & 3) || (ldo & 3) || C < 1 || ld < C || ldo < C || rows < 0 || !low || !out)
    return (int)hipErrorInvalidValue;
  if (rows == 0) return (int)hipSuccess;
  const int grid = (int)std::min<long>(seg_cdiv(rows * (ldo >> 2), 256), 8192);
  hipLaunchKernelGGL(low_logits_kernel<T>, dim3(grid), dim3(256), 0, stream, low, ld, rows, C, out, ldo);
  SEG_RET_LAST();
}

}  // namespace

// out6 = [loss, D, #out-of-range labels, #valid, CE, KD]; `work` >= seg_kd_workspace_floats(N*Ho*Wo).
SEG_API long seg_kd_workspace_floats(long pixels) { return 5L * loss_blocks(pixels); }

SEG_API int seg_kd_upsample_loss(const float* low, long ld, int N, int H, int W, int C, const float* teacher, long ldt,
                                 int Ht, int Wt, const long long* labels, int Ho, int Wo, int ignore_index,
                                 const float* class_weight, float ce, float kd, float temperature, int kd_ignored,
                                 float* work, float* out6, hipStream_t stream) {
  return kd_loss_impl(low, ld, N, H, W, C, teacher, ldt, Ht, Wt, labels, Ho, Wo, ignore_index,
                      KdOpt{class_weight, ce, kd, temperature, kd_ignored != 0}, work, out6, stream);
}
SEG_API int seg_kd_upsample_loss_bf16io(const __bf16* low, long ld, int N, int H, int W, int C, const float* teacher,
                                        long ldt, int Ht, int Wt, const long long* labels, int Ho, int Wo,
                                        int ignore_index, const float* class_weight, float ce, float kd,
                                        float temperature, int kd_ignored, float* work, float* out6,
                                        hipStream_t stream) {
  return kd_loss_impl(low, ld, N, H, W, C, teacher, ldt, Ht, Wt, labels, Ho, Wo, ignore_index,
                      KdOpt{class_weight, ce, kd, temperature, kd_ignored != 0}, work, out6, stream);
}
SEG_API int seg_kd_upsample_grad(const float* low, long ld, int N, int H, int W, int C, const float* teacher, long ldt,
                                 int Ht, int Wt, const long long* labels, int Ho, int Wo, int ignore_index,
                                 const float* class_weight, float ce, float kd, float temperature, int kd_ignored,
                                 const float* grad_out, const float* stats, float* dhigh, long ldh,
                                 hipStream_t stream) {
  return kd_grad_impl(low, ld, N, H, W, C, teacher, ldt, Ht, Wt, labels, Ho, Wo, ignore_index,
                      KdOpt{class_weight, ce, kd, temperature, kd_ignored != 0}, grad_out, stats, dhigh, ldh, stream);
}
SEG_API int seg_kd_upsample_grad_bf16io(const __bf16* low, long ld, int N, int H, int W, int C, const float* teacher,
                                        long ldt, int Ht, int Wt, const long long* labels, int Ho, int Wo,
                                        int ignore_index, const float* class_weight, float ce, float kd,
                                        float temperature, int kd_ignored, const float* grad_out, const float* stats,
                                        __bf16* dhigh, long ldh, hipStream_t stream) {
  return kd_grad_impl(low, ld, N, H, W, C, teacher, ldt, Ht, Wt, labels, Ho, Wo, ignore_index,
                      KdOpt{class_weight, ce, kd, temperature, kd_ignored != 0}, grad_out, stats, dhigh, ldh, stream);
}
// seg_kd_upsample_grad_bf16io with the full-resolution gradient written as fp32 NCHW [N][C][Ho][Wo]: follow with
// seg_upsample_bwd_bf16io(nchw_grad = 1, ac = 2).
SEG_API int seg_kd_upsample_grad_bf16io_nchw(const __bf16* low, long ld, int N, int H, int W, int C,
                                             const float* teacher, long ldt, int Ht, int Wt, const long long* labels,
                                             int Ho, int Wo, int ignore_index, const float* class_weight, float ce,
                                             float kd, float temperature, int kd_ignored, const float* grad_out,
                                             const float* stats, float* dhigh_nchw, hipStream_t stream) {
  return kd_grad_impl<__bf16, true>(low, ld, N, H, W, C, teacher, ldt, Ht, Wt, labels, Ho, Wo, ignore_index,
                                    KdOpt{class_weight, ce, kd, temperature, kd_ignored != 0}, grad_out, stats,
                                    dhigh_nchw, 0, stream);
}

// The C real channels of each NHWC row as fp32 rows the caller owns (pads 0): the teacher's low-resolution logits
// handed to seg_kd_*.
SEG_API int seg_low_logits_f32(const float* low, long ld, long rows, int C, float* out, long ldo, hipStream_t stream) {
  return low_logits_impl(low, ld, rows, C, out, ldo, stream);
}
SEG_API int seg_low_logits_f32_bf16io(const __bf16* low, long ld, long rows, int C, float* out, long ldo,
                                      hipStream_t stream) {
  return low_logits_impl(low, ld, rows, C, out, ldo, stream);
}

// ---- one logit per pixel: sigmoid cross-entropy with a focal exponent, plus soft Dice: seg_bce_* ----
// (the criterion is seg_amd.BinarySegLoss).  C = 1; labels t_p in {0, 1}, anything else that is not ignore_index is
// out of range.  Over the valid pixels V, with z_p the pixel's logit, s_p = sigmoid(z_p), pt_p = s_p where t_p = 1
// else 1 - s_p, and w_p = pos_weight where t_p = 1 else 1:
//   F    = sum_V w_p (1 - pt_p)^gamma (-log pt_p) / |V|
//   I = sum_V s_p t_p,  S = sum_V s_p,  T = sum_V t_p,  U = S + T + smooth,  Dice = 1 - (2 I + smooth) / U
//   loss = bce F + dice Dice    (a term whose coefficient is 0 is left out, so its 0/0 never reaches the loss).
// One pass writes six partials per block [focal sum, #valid, #out-of-range, I, S, T]; the one-wave fp64 finalize
// writes stats8 = [loss, #valid, #out-of-range, #valid, F, Dice, a, b] with the Dice gradient's two coefficients
// a = 2 / U and b = (2 I + smooth) / U^2, so the gradient kernel needs no table:
//   dz_p = (g bce / |V|) (t_p ? -1 : 1) w_p (1 - pt)^gamma ((1 - pt) + gamma pt (-log pt)) - g dice (a t_p - b) s (1 - s).
// Numerical form: e = exp(-|z|) is the only exponential; s and 1 - s are 1 / (1 + e) and e / (1 + e) by the sign
// of z (never 1.f - s), s (1 - s) their product, -log sigmoid(x) = max(-x, 0) + log1p(e); everything is finite for
// any finite z, and (1 - pt)^gamma is exactly 0 where 1 - pt is (seg_sl_*'s rule).
// The z of a pixel is lane 0 of full_res_logits<4>: the row's three pad lanes are loaded with it and never used.
// The gradient is ONE fp32 per pixel, [N][Ho][Wo] -- at C = 1 the NCHW plane seg_upsample_bwd(nchw_grad = 1) reads --
// in both maths: 4 B a pixel where a round4(C) row costs 16, and (the seg_ohem_* / seg_kd_* twins' reason) the
// low-resolution gradient of the bf16io twin sums unrounded terms.
namespace {

constexpr int BCE_NP = 6;

struct BceOpt {
  float pos_weight;
  float bce, dice;  // the two coefficients
  float gamma;      // focal exponent
  float smooth;     // dice_smooth
};

inline bool bce_opt_ok(const BceOpt& o) {
  return std::isfinite(o.pos_weight) && std::isfinite(o.bce) && std::isfinite(o.dice) && std::isfinite(o.gamma) &&
         std::isfinite(o.smooth) && o.pos_weight > 0.f && o.bce >= 0.f && o.dice >= 0.f &&
         (o.bce > 0.f || o.dice > 0.f) && o.gamma >= 0.f && o.smooth > 0.f;
}
inline bool bce_geom_ok(long ld, int C) { return loss_geom_ok(ld, C) && C == 1; }

// sigmoid(z), sigmoid(-z) and log1p(exp(-|z|)) from the one exponential
struct Sig {
  float s, c, l1p;
};
__device__ __forceinline__ Sig sigmoid_of(float z) {
  const float e = expf(-fabsf(z));
  const float inv = 1.f / (1.f + e);
  const float big = inv, small = e * inv;
  const bool pos = z >= 0.f;
  return Sig{pos ? big : small, pos ? small : big, log1pf(e)};
}

template <typename T>
__device__ __forceinline__ float one_logit(const T* __restrict__ low, long ld, int H, int W, const Pix& px, float sh,
                                           float sw) {
  float z[4];
  full_res_logits<4, T>(low, ld, H, W, px.n, px.r, px.s, sh, sw, z);
  return z[0];
}

template <typename T, bool EVAL>
__global__ __launch_bounds__(256) void bce_up_loss_kernel(const T* __restrict__ low, long ld, int N, int H, int W,
                                                          const long long* __restrict__ labels, int Ho, int Wo,
                                                          float sh, float sw, int ignore_index,
                                                          float* __restrict__ part, float zthr,
                                                          unsigned long long* __restrict__ confusion, BceOpt o) {
  __shared__ float red[4][BCE_NP];
  __shared__ int hist[4];
  if constexpr (EVAL) {
    hist_clear(hist, 2);
    __syncthreads();
  }
  const long total = (long)N * Ho * Wo;
  const bool focal = o.gamma > 0.f;
  float fsum = 0.f, cnt = 0.f, bad = 0.f, isum = 0.f, ssum = 0.f, tsum = 0.f;
  for (long p = blockIdx.x * (long)blockDim.x + threadIdx.x; p < total; p += (long)gridDim.x * blockDim.x) {
    const long long y = labels[p];
    if (y == ignore_index) continue;
    if (y < 0 || y > 1) {
      bad += 1.f;
      continue;
    }
    const bool fg = y == 1;
    const float z = one_logit<T>(low, ld, H, W, pixel_of(p, Ho, Wo), sh, sw);
    const Sig g = sigmoid_of(z);
    const float nlp = fmaxf(fg ? -z : z, 0.f) + g.l1p;  // -log pt
    const float omp = fg ? g.c : g.s;                   // 1 - pt
    const float wy = fg ? o.pos_weight : 1.f;
    float pw = 1.f;
    if (focal) pw = omp > 0.f ? powf(omp, o.gamma) : 0.f;
    fsum = __builtin_fmaf(wy * pw, nlp, fsum);
    cnt += 1.f;
    ssum += g.s;
    isum += fg ? g.s : 0.f;
    tsum += fg ? 1.f : 0.f;
    if constexpr (EVAL) hist_count(hist, 2, (int)y, z > zthr ? 1 : 0);  // strict: a tie or a NaN is background
  }
  const float v[BCE_NP] = {fsum, cnt, bad, isum, ssum, tsum};
  block_partials<BCE_NP>(v, red, part);
  if constexpr (EVAL) hist_flush(hist, 2, confusion);
}

__global__ void bce_finalize_kernel(const float* __restrict__ part, int nblk, float bce, float dice, float smooth,
                                    float* __restrict__ out) {
  double t[BCE_NP];
  column_sums_f64<BCE_NP>(part, nblk, BCE_NP, t);
  if (threadIdx.x == 0) {
    const double f = t[0], c = t[1], b = t[2], I = t[3], S = t[4], Tc = t[5];
    const double F = f / c;  // 0/0 = nan when every pixel is ignored, as aten
    const double U = S + Tc + (double)smooth, num = 2.0 * I + (double)smooth;
    const double Dice = 1.0 - num / U;
    double loss = 0.0;
    if (bce > 0.f) loss += (double)bce * F;
    if (dice > 0.f) loss += (double)dice * Dice;
    out[0] = b > 0.0 ? __builtin_nanf("") : (float)loss;
    out[1] = (float)c;
    out[2] = (float)b;
    out[3] = (float)c;
    out[4] = (float)F;
    out[5] = (float)Dice;
    out[6] = (float)(2.0 / U);
    out[7] = (float)(num / (U * U));
  }
}

template <typename T>
__global__ __launch_bounds__(256) void bce_up_grad_kernel(const T* __restrict__ low, long ld, int N, int H, int W,
                                                          const long long* __restrict__ labels, int Ho, int Wo,
                                                          float sh, float sw, int ignore_index,
                                                          const float* __restrict__ gout,
                                                          const float* __restrict__ stats, float* __restrict__ dhigh,
                                                          BceOpt o) {
  const long total = (long)N * Ho * Wo;
  const bool poisoned = stats[2] > 0.f, has_bce = o.bce > 0.f, has_dice = o.dice > 0.f, focal = o.gamma > 0.f;
  const float sce = poisoned ? __builtin_nanf("") : has_bce ? gout[0] * o.bce / stats[1] : 0.f;  // g bce / |V|
  const float sdi = poisoned ? __builtin_nanf("") : gout[0] * o.dice;                             // g dice
  const float a = stats[6], b = stats[7];
  for (long p = blockIdx.x * (long)blockDim.x + threadIdx.x; p < total; p += (long)gridDim.x * blockDim.x) {
    const long long y = labels[p];
    if (y == ignore_index || y < 0 || y > 1) {
      dhigh[p] = 0.f;
      continue;
    }
    const bool fg = y == 1;
    const float z = one_logit<T>(low, ld, H, W, pixel_of(p, Ho, Wo), sh, sw);
    const Sig g = sigmoid_of(z);
    const float omp = fg ? g.c : g.s, pt = fg ? g.s : g.c;
    float fp = omp;  // (1 - pt)^gamma ((1 - pt) + gamma pt (-log pt))
    if (focal) {
      const float nlp = fmaxf(fg ? -z : z, 0.f) + g.l1p;
      fp = omp > 0.f ? powf(omp, o.gamma) * __builtin_fmaf(o.gamma * pt, nlp, omp) : 0.f;
    }
    const float wy = fg ? o.pos_weight : 1.f;
    float d = sce * (fg ? -(wy * fp) : wy * fp);
    if (has_dice) d = __builtin_fmaf(sdi * (g.s * g.c), fg ? b - a : b, d);
    dhigh[p] = d;
  }
}

template <typename T, bool EVAL>
int bce_loss_impl(const T* low, long ld, int N, int H, int W, int C, const long long* labels, int Ho, int Wo,
                  int ignore_index, BceOpt o, float* work, float* out8, float zthr, long long* confusion,
                  hipStream_t stream) {
  if (!bce_geom_ok(ld, C) || (EVAL && !confusion) || !bce_opt_ok(o)) return (int)hipErrorInvalidValue;
  const int nb = loss_blocks((long)N * Ho * Wo);
  const UpScale up = up_scale(H, W, Ho, Wo);
  hipLaunchKernelGGL((bce_up_loss_kernel<T, EVAL>), dim3(nb), dim3(256), 0, stream, low, ld, N, H, W, labels, Ho, Wo,
                     up.sh, up.sw, ignore_index, work, zthr, (unsigned long long*)confusion, o);
  hipLaunchKernelGGL(bce_finalize_kernel, dim3(1), dim3(64), 0, stream, work, nb, o.bce, o.dice, o.smooth, out8);
  SEG_RET_LAST();
}

template <typename T>
int bce_grad_impl(const T* low, long ld, int N, int H, int W, int C, const long long* labels, int Ho, int Wo,
                  int ignore_index, BceOpt o, const float* grad_out, const float* stats, float* dhigh,
                  hipStream_t stream) {
  if (!bce_geom_ok(ld, C) || !bce_opt_ok(o)) return (int)hipErrorInvalidValue;
  const UpScale up = up_scale(H, W, Ho, Wo);
  hipLaunchKernelGGL((bce_up_grad_kernel<T>), dim3(grad_blocks((long)N * Ho * Wo)), dim3(256), 0, stream, low, ld, N,
                     H, W, labels, Ho, Wo, up.sh, up.sw, ignore_index, grad_out, stats, dhigh, o);
  SEG_RET_LAST();
}

}  // namespace

// stats8 = [loss, #valid, #out-of-range labels, #valid, F, Dice, a, b]; `work` >= seg_bce_workspace_floats(N*Ho*Wo).
SEG_API long seg_bce_workspace_floats(long pixels) { return (long)BCE_NP * loss_blocks(pixels); }

SEG_API int seg_bce_upsample_loss(const float* low, long ld, int N, int H, int W, int C, const long long* labels,
                                  int Ho, int Wo, int ignore_index, float pos_weight, float bce, float dice,
                                  float focal_gamma, float dice_smooth, float* work, float* stats8,
                                  hipStream_t stream) {
  return bce_loss_impl<float, false>(low, ld, N, H, W, C, labels, Ho, Wo, ignore_index,
                                     BceOpt{pos_weight, bce, dice, focal_gamma, dice_smooth}, work, stats8, 0.f,
                                     nullptr, stream);
}
SEG_API int seg_bce_upsample_loss_bf16io(const __bf16* low, long ld, int N, int H, int W, int C,
                                         const long long* labels, int Ho, int Wo, int ignore_index, float pos_weight,
                                         float bce, float dice, float focal_gamma, float dice_smooth, float* work,
                                         float* stats8, hipStream_t stream) {
  return bce_loss_impl<__bf16, false>(low, ld, N, H, W, C, labels, Ho, Wo, ignore_index,
                                      BceOpt{pos_weight, bce, dice, focal_gamma, dice_smooth}, work, stats8, 0.f,
                                      nullptr, stream);
}
// Validation: the same loss and stats, and confusion[t * 2 + (z > zthr)] += 1 per valid pixel (int64 [2][2]).
SEG_API int seg_bce_upsample_eval(const float* low, long ld, int N, int H, int W, int C, const long long* labels,
                                  int Ho, int Wo, int ignore_index, float pos_weight, float bce, float dice,
                                  float focal_gamma, float dice_smooth, float* work, float* stats8, float zthr,
                                  long long* confusion, hipStream_t stream) {
  return bce_loss_impl<float, true>(low, ld, N, H, W, C, labels, Ho, Wo, ignore_index,
                                    BceOpt{pos_weight, bce, dice, focal_gamma, dice_smooth}, work, stats8, zthr,
                                    confusion, stream);
}
SEG_API int seg_bce_upsample_eval_bf16io(const __bf16* low, long ld, int N, int H, int W, int C,
                                         const long long* labels, int Ho, int Wo, int ignore_index, float pos_weight,
                                         float bce, float dice, float focal_gamma, float dice_smooth, float* work,
                                         float* stats8, float zthr, long long* confusion, hipStream_t stream) {
  return bce_loss_impl<__bf16, true>(low, ld, N, H, W, C, labels, Ho, Wo, ignore_index,
                                     BceOpt{pos_weight, bce, dice, focal_gamma, dice_smooth}, work, stats8, zthr,
                                     confusion, stream);
}
// dhigh: fp32 [N][Ho][Wo] in both maths; follow with seg_upsample_bwd(nchw_grad = 1, ac = 2).
SEG_API int seg_bce_upsample_grad(const float* low, long ld, int N, int H, int W, int C, const long long* labels,
                                  int Ho, int Wo, int ignore_index, float pos_weight, float bce, float dice,
                                  float focal_gamma, const float* grad_out, const float* stats8, float* dhigh,
                                  hipStream_t stream) {
  return bce_grad_impl(low, ld, N, H, W, C, labels, Ho, Wo, ignore_index,
                       BceOpt{pos_weight, bce, dice, focal_gamma, 1.f}, grad_out, stats8, dhigh, stream);
}
SEG_API int seg_bce_upsample_grad_bf16io(const __bf16* low, long ld, int N, int H, int W, int C,
                                         const long long* labels, int Ho, int Wo, int ignore_index, float pos_weight,
                                         float bce, float dice, float focal_gamma, const float* grad_out,
                                         const float* stats8, float* dhigh, hipStream_t stream) {
  return bce_grad_impl(low, ld, N, H, W, C, labels, Ho, Wo, ignore_index,
                       BceOpt{pos_weight, bce, dice, focal_gamma, 1.f}, grad_out, stats8, dhigh, stream);
}
