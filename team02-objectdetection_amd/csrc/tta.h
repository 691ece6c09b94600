// Test-time augmentation (flip / multi-scale ensembles): what the validation kernel (tta.hip) and the
// Predictor's kernel (infer.hip) share.
//
// A view v is a forward of a resized and / or mirrored copy of the image; its low-resolution NHWC logits
// L_v [N][H_v][W_v][ld_v] map onto the model's Ho x Wo output grid exactly as the model's final
// align_corners=True upsample maps them (lin_index(.., 1)'s taps and weights with their roundings written
// out -- tta_lin -- and bilerp4's blend), a mirrored view read at x_v = Wo - 1 - x.  Per output pixel, in fp32:
//   z_v = the blend of L_v's four taps,  p = sum_v w_v * softmax(z_v),  class = the first maximum of p.
// The views arrive as a HOST array of seg_tta_view (include/segamd.h); tta_table() checks them, normalises
// the weights to sum 1 and packs them with their two source scales into ONE kernel argument passed by
// value: no device allocation, no copy, capturable in a graph.  The kernels index the table with the
// wave-uniform view counter only, so its fields arrive by scalar loads from the kernel-argument segment.
#pragma once
#include <stddef.h>

#include "common.h"

constexpr int kTtaMaxViews = 8;  // SEG_TTA_MAX_VIEWS

struct SegTtaView {  // seg_tta_view of include/segamd.h, field for field
  const float* low;
  long ld;
  int H, W;
  int flip;
  float weight;
};
static_assert(sizeof(SegTtaView) == 32 && offsetof(SegTtaView, low) == 0 && offsetof(SegTtaView, ld) == 8 &&
                  offsetof(SegTtaView, H) == 16 && offsetof(SegTtaView, W) == 20 && offsetof(SegTtaView, flip) == 24 &&
                  offsetof(SegTtaView, weight) == 28,
              "seg_tta_view ABI");

struct TtaView {
  const float* low;
  long ld;
  int H, W;
  int flip;
  float weight;  // normalised: the table's weights sum to 1
  float sh, sw;  // (H - 1) / (Ho - 1), (W - 1) / (Wo - 1): the final upsample's source scales
};
struct TtaTable {
  TtaView v[kTtaMaxViews];
  int n;
};

// false: an argument the entry points reject (hipErrorInvalidValue, before any launch)
static inline bool tta_table(const void* views, int nviews, int C, int Ho, int Wo, TtaTable* t) {
  if (!views || nviews < 1 || nviews > kTtaMaxViews || C < 1 || Ho <= 0 || Wo <= 0) return false;
  const SegTtaView* in = reinterpret_cast<const SegTtaView*>(views);
  double total = 0.0;
  for (int i = 0; i < nviews; ++i) {
    const SegTtaView& s = in[i];
    if (!s.low || ((uintptr_t)s.low & 15) || (s.ld & 3) || s.ld < C || s.H <= 0 || s.W <= 0) return false;
    if (!(s.weight > 0.f) || !(s.weight < __builtin_inff())) return false;  // a NaN fails the first test
    total += (double)s.weight;
  }
  for (int i = 0; i < kTtaMaxViews; ++i) {
    const SegTtaView& s = in[i < nviews ? i : 0];  // the unused slots repeat view 0 (never read)
    TtaView& d = t->v[i];
    d.low = s.low;
    d.ld = s.ld;
    d.H = s.H;
    d.W = s.W;
    d.flip = s.flip != 0;
    d.weight = (float)((double)s.weight / total);
    d.sh = Ho > 1 ? (float)(s.H - 1) / (float)(Ho - 1) : 0.f;
    d.sw = Wo > 1 ? (float)(s.W - 1) / (float)(Wo - 1) : 0.f;
  }
  t->n = nviews;
  return true;
}

#ifdef __HIPCC__
// The four taps of view v at output pixel (y, x) of image n.
struct TtaTaps {
  const float *t00, *t01, *t10, *t11;
  Lin lh, lw;
};
// lin_index(.., 1) with every rounding written out: the source coordinate scale * dst is rounded to fp32 BEFORE the
// tap index is taken off it, as the definition says and the float64 restatement of the tests does.  Left to the
// compiler, the product and the subtraction contract into one fma, which at a source coordinate near 256 moves a tap
// weight by up to 1e-5 -- times a logit difference of 10 or more, that is beyond the 1e-5 bound on p.
__device__ __forceinline__ Lin tta_lin(int dst, int in, float scale) {
#pragma clang fp contract(off)
  const float src = scale * (float)dst;
  int i0 = (int)floorf(src);
  if (i0 > in - 1) i0 = in - 1;
  Lin r;
  r.i0 = i0;
  r.i1 = i0 + (i0 < in - 1 ? 1 : 0);
  r.l1 = fminf(fmaxf(src - (float)i0, 0.f), 1.f);
  r.l0 = 1.f - r.l1;
  return r;
}
__device__ __forceinline__ TtaTaps tta_taps(const TtaView& v, int n, int y, int x, int Wo) {
  TtaTaps t;
  t.lh = tta_lin(y, v.H, v.sh);
  t.lw = tta_lin(v.flip ? Wo - 1 - x : x, v.W, v.sw);
  const float* base = v.low + (long)n * v.H * v.W * v.ld;
  t.t00 = base + ((long)t.lh.i0 * v.W + t.lw.i0) * v.ld;
  t.t01 = base + ((long)t.lh.i0 * v.W + t.lw.i1) * v.ld;
  t.t10 = base + ((long)t.lh.i1 * v.W + t.lw.i0) * v.ld;
  t.t11 = base + ((long)t.lh.i1 * v.W + t.lw.i1) * v.ld;
  return t;
}
__device__ __forceinline__ f32x4 tta_blend(const TtaTaps& t, int q) {
  return bilerp4(ld4(t.t00 + 4 * q), ld4(t.t01 + 4 * q), ld4(t.t10 + 4 * q), ld4(t.t11 + 4 * q), t.lh, t.lw);
}

// p += w_v * softmax(z_v) over the C channels of NQ register quads; returns the weight added.  z_v's quads stay
// in registers between the three passes (max, sum, accumulate).  GUARD: a view with a non-finite z_v adds nothing and returns 0 (the
// Predictor's rule); without it the NaN goes into p (the validation's rule).  Pad lanes C.. of a quad are
// loaded with it and never used; p's stay as they were.
template <int NQ, bool GUARD>
__device__ __forceinline__ float tta_accumulate(const TtaView& v, int n, int y, int x, int Wo, int C,
                                                f32x4 (&p)[NQ]) {
  const TtaTaps t = tta_taps(v, n, y, x, Wo);
  f32x4 zr[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) zr[q] = tta_blend(t, q);
  float zmax = -__builtin_inff();
  bool finite = true;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const f32x4 z = zr[q];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (4 * q + j >= C) continue;
      finite = finite && fabsf(z[j]) < __builtin_inff();  // false for a NaN as well
      zmax = fmaxf(zmax, z[j]);
    }
  }
  if (GUARD && !finite) return 0.f;
  float sum = 0.f;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const f32x4 z = zr[q];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (4 * q + j < C) sum += expf(z[j] - zmax);
  }
  const float ws = v.weight / sum;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const f32x4 z = zr[q];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (4 * q + j < C) p[q][j] = __builtin_fmaf(expf(z[j] - zmax), ws, p[q][j]);
  }
  return v.weight;
}
#endif
