// Test-time augmentation for validation: the flip / multi-scale ensemble's loss, argmax and confusion
// matrix in one kernel from the views' low-resolution logits (tta.h has the definition), and the kernel
// that forms a view of an NCHW batch.
//
//   seg_tta_view_nchw      flip(F.interpolate(x, (Hv, Wv), mode="bilinear", align_corners=False), -1)
//   seg_tta_upsample_eval  p = sum_v w_v softmax(z_v) per output pixel; loss = NLLLoss(weight, ignore_index,
//                          reduction)(log p, labels); confusion[label][first maximum of p] += 1 per valid
//                          pixel; optionally p itself as [N][C][Ho][Wo]
// Reductions follow loss.hip: per-block partials in `work`, one fixed-order fp64 finalize, a per-block LDS
// histogram flushed with 64-bit integer atomics -- two runs are bitwise equal.  A label outside [0, C)
// that is not ignore_index is counted in out4[2] and makes the loss NaN, as in seg_cew_upsample_eval.  A
// non-finite logit gets no special case: its pixel's p is NaN, so is the loss, and the pixel is binned
// under class 0 or the last class whose comparison still held.
#include "tta.h"

#pragma clang fp contract(off)

namespace {

constexpr int kTtaEvalMaxC = 32;

int tta_blocks(long total) { return (int)std::min<long>(seg_cdiv(total, 256), 2048); }

// One thread per output pixel (grid-stride).  Partials per block: [nll, sum of w[y], #out-of-range, 0, #valid]
// (seg_cew_upsample_eval's five columns; there is no smoothing sum).  z and p of a view stay in registers for
// every C <= 32 (2 * NQ quads).
template <int NQ>
__global__ __launch_bounds__(256) void tta_eval_kernel(const TtaTable t, int N, int C,
                                                       const long long* __restrict__ labels, int Ho, int Wo,
                                                       int ignore_index, const float* __restrict__ cw,
                                                       float* __restrict__ part,
                                                       unsigned long long* __restrict__ confusion,
                                                       float* __restrict__ prob) {
  __shared__ float red[4][4];
  __shared__ int hist[kTtaEvalMaxC * kTtaEvalMaxC];
  for (int i = threadIdx.x; i < C * C; i += 256) hist[i] = 0;
  __syncthreads();
  const long total = (long)N * Ho * Wo;
  float lsum = 0.f, cnt = 0.f, bad = 0.f, val = 0.f;
  for (long px = blockIdx.x * 256L + threadIdx.x; px < total; px += (long)gridDim.x * 256) {
    const long long y = labels ? labels[px] : (long long)ignore_index;  // no labels: probabilities only
    const bool ignored = y == ignore_index;
    const bool valid = !ignored && y >= 0 && y < C;
    if (!ignored && !valid) bad += 1.f;
    if (!valid && !prob) continue;
    const int n = (int)(px / ((long)Ho * Wo));
    const int rem = (int)(px - (long)n * Ho * Wo);
    const int r = rem / Wo, s = rem - r * Wo;
    f32x4 p[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) p[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int v = 0; v < t.n; ++v)  // wave-uniform: the view's fields are scalar loads
      tta_accumulate<NQ, false>(t.v[v], n, r, s, Wo, C, p);
    if (prob) {
      float* o = prob + ((long)n * C * Ho + r) * Wo + s;
#pragma unroll
      for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (4 * q + j < C) o[(long)(4 * q + j) * Ho * Wo] = p[q][j];
    }
    if (!valid) continue;
    int pred = 0;
    float best = p[0][0], py = 0.f;
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = 4 * q + j;
        py = k == (int)y ? p[q][j] : py;
        if (k > 0 && k < C && p[q][j] > best) {  // strict >, ascending: the first maximum
          best = p[q][j];
          pred = k;
        }
      }
    const float wy = cw ? cw[y] : 1.f;
    lsum = __builtin_fmaf(wy, -logf(py), lsum);
    cnt += wy;
    val += 1.f;
    atomicAdd(&hist[(int)y * C + pred], 1);
  }
  lsum = wave_sum(lsum);
  cnt = wave_sum(cnt);
  bad = wave_sum(bad);
  val = wave_sum(val);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    red[0][wave] = lsum;
    red[1][wave] = cnt;
    red[2][wave] = bad;
    red[3][wave] = val;
  }
  __syncthreads();  // closes the histogram as well
  if (threadIdx.x == 0) {
    float* o = part + 5L * blockIdx.x;
    o[0] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    o[1] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    o[2] = red[2][0] + red[2][1] + red[2][2] + red[2][3];
    o[3] = 0.f;
    o[4] = red[3][0] + red[3][1] + red[3][2] + red[3][3];
  }
  for (int i = threadIdx.x; i < C * C; i += 256) {
    const int v = hist[i];
    if (v) atomicAdd(confusion + i, (unsigned long long)v);
  }
}

// out4 = [loss, D, #out-of-range labels, #valid pixels]; D = sum of w[y] (mean; 0/0 = nan as aten) or 1 (sum)
__global__ void tta_finalize_kernel(const float* __restrict__ part, int nblk, int reduction, float* out) {
  double l = 0.0, c = 0.0, b = 0.0, v = 0.0;
  for (int k = threadIdx.x; k < nblk; k += 64) {
    l += part[5 * k];
    c += part[5 * k + 1];
    b += part[5 * k + 2];
    v += part[5 * k + 4];
  }
  for (int o = 32; o > 0; o >>= 1) {
    l += __shfl_xor(l, o, 64);
    c += __shfl_xor(c, o, 64);
    b += __shfl_xor(b, o, 64);
    v += __shfl_xor(v, o, 64);
  }
  if (threadIdx.x == 0) {
    const double d = reduction == 0 ? c : 1.0;
    out[0] = b > 0.0 ? __builtin_nanf("") : (float)(l / d);
    out[1] = (float)d;
    out[2] = (float)b;
    out[3] = (float)v;
  }
}

// out[n][c][yv][xv] = the align_corners=False bilinear sample of x[n][c] at (yv, flip ? Wv - 1 - xv : xv):
// aten's source index and weights (lin_index(.., 0)), one fixed fma association (up_blend4's).  A view of
// the input's own size takes the tap itself: a copy, or the mirror image.
__global__ __launch_bounds__(256) void tta_view_kernel(const float* __restrict__ x, long planes, int H, int W,
                                                       float* __restrict__ out, int Hv, int Wv, int flip, float sh,
                                                       float sw) {
  const long total = planes * Hv * Wv;
  const bool same = Hv == H && Wv == W;
  for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const long pl = e / ((long)Hv * Wv);
    const int rem = (int)(e - pl * Hv * Wv);
    const int yv = rem / Wv, xo = rem - yv * Wv;
    const int xv = flip ? Wv - 1 - xo : xo;
    const float* src = x + pl * H * W;
    if (same) {
      out[e] = src[(long)yv * W + xv];
      continue;
    }
    const Lin lh = lin_index(yv, H, sh, 0), lw = lin_index(xv, W, sw, 0);
    const float v00 = src[(long)lh.i0 * W + lw.i0], v01 = src[(long)lh.i0 * W + lw.i1];
    const float v10 = src[(long)lh.i1 * W + lw.i0], v11 = src[(long)lh.i1 * W + lw.i1];
    const float top = __builtin_fmaf(lw.l1, v01, lw.l0 * v00);
    const float bot = __builtin_fmaf(lw.l1, v11, lw.l0 * v10);
    out[e] = __builtin_fmaf(lh.l1, bot, lh.l0 * top);
  }
}

}  // namespace

// A TTA view of an NCHW fp32 batch x [N][C][H][W] -> out [N][C][Hv][Wv] (flip != 0: mirrored left-right).
SEG_API int seg_tta_view_nchw(const float* x, int N, int C, int H, int W, float* out, int Hv, int Wv, int flip,
                              hipStream_t stream) {
  if (!x || !out || N <= 0 || C <= 0 || H <= 0 || W <= 0 || Hv <= 0 || Wv <= 0) return (int)hipErrorInvalidValue;
  const long planes = (long)N * C;
  const int grid = (int)std::min<long>(seg_cdiv(planes * Hv * Wv, 256), 8192);
  hipLaunchKernelGGL(tta_view_kernel, dim3(grid), dim3(256), 0, stream, x, planes, H, W, out, Hv, Wv, flip != 0,
                     (float)H / (float)Hv, (float)W / (float)Wv);
  SEG_RET_LAST();
}

SEG_API long seg_tta_workspace_floats(long pixels) { return 5L * tta_blocks(pixels); }

// The ensemble's validation step.  views: HOST array of nviews (1..8) seg_tta_view; labels int64 [N][Ho][Wo];
// class_weight: C floats in device memory or NULL; reduction 0 = mean, 1 = sum; work >=
// seg_tta_workspace_floats(N*Ho*Wo); out4 = [loss, D, #out-of-range labels, #valid pixels]; confusion int64
// [C][C], added to; prob NULL or fp32 [N][C][Ho][Wo], every pixel written.  C in 1..32.  labels == NULL (with prob):
// probabilities only -- every pixel counts as ignored, nothing is binned and confusion may be NULL.
SEG_API int seg_tta_upsample_eval(const void* views, int nviews, int N, int C, const long long* labels, int Ho, int Wo,
                                  int ignore_index, const float* class_weight, int reduction, float* work,
                                  float* out4, long long* confusion, float* prob, hipStream_t stream) {
  TtaTable t;
  if (C > kTtaEvalMaxC || N <= 0 || !tta_table(views, nviews, C, Ho, Wo, &t) || (reduction != 0 && reduction != 1) ||
      !work || !out4 || (labels ? !confusion : !prob))
    return (int)hipErrorInvalidValue;
  const int nb = tta_blocks((long)N * Ho * Wo);
#define SEG_TTA_EVAL(NQ)                                                                                         \
  case NQ:                                                                                                       \
    hipLaunchKernelGGL(tta_eval_kernel<NQ>, dim3(nb), dim3(256), 0, stream, t, N, C, labels, Ho, Wo, ignore_index, \
                       class_weight, work, (unsigned long long*)confusion, prob);                                \
    break
  switch ((C + 3) / 4) {
    SEG_TTA_EVAL(1); SEG_TTA_EVAL(2); SEG_TTA_EVAL(3); SEG_TTA_EVAL(4);
    SEG_TTA_EVAL(5); SEG_TTA_EVAL(6); SEG_TTA_EVAL(7); SEG_TTA_EVAL(8);
  }
#undef SEG_TTA_EVAL
  hipLaunchKernelGGL(tta_finalize_kernel, dim3(1), dim3(64), 0, stream, work, nb, reduction, out4);
  SEG_RET_LAST();
}
