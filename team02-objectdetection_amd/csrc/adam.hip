// Adam step over every parameter tensor of a model in one launch.
//
// Reference: optim.Adam(model.parameters(), lr=1.5e-4) (main.py:100) stepped once
// per batch (src/train.py:39) -- defaults betas (0.9, 0.999), eps 1e-8, no weight
// decay, no amsgrad.  On the GPU torch runs it as the foreach
// implementation: ~8 multi-tensor launches per step, each streaming p / g / m / v
// again.  Here each element is read once and written once, with the arithmetic of the
// foreach ops in the same order, in fp32:
//   m = lerp(m, g, 1 - b1)                 _foreach_lerp_   (weight < 0.5 branch)
//   v = v * b2;  v = v + (1 - b2) * g * g  _foreach_mul_, _foreach_addcmul_
//   d = sqrt(v) / sqrt(bc2) + eps          _foreach_sqrt, _foreach_div_, _foreach_add_
//   p = p + (-lr / bc1) * (m / d)          _foreach_addcdiv_
// bc1 = 1 - b1^t and bc2 = 1 - b2^t are per tensor, computed on the host (as torch does
// from its CPU step counters) and passed in the tensor table.
//
// Work split: a host-built chunk map (tensor index, first element) of at most
// `chunk` elements each; one 256-thread block per chunk.  Parameters with no
// gradient (the unused classifier) are simply absent from the table.
//
// AdamW and gradient clipping (seg_adamw_step, seg_grad_sumsq, seg_grad_scale) run over the
// same chunk map with a wider record, SegAdamWTensor; see the second half of this file.  SGD with momentum
// (seg_sgd_step) uses that record too and is the last section.
#include "common.h"

struct SegAdamTensor {  // 48 bytes, the layout seg_amd/optim.py packs
  float* p;
  const float* g;
  float* m;
  float* v;
  long n;
  float step_size;  // -lr / bc1
  float bc2_sqrt;   // sqrt(1 - b2^t)
};

namespace {

__global__ __launch_bounds__(256) void adam_kernel(const SegAdamTensor* __restrict__ ts,
                                                   const long* __restrict__ chunks, int chunk, float w, float b2,
                                                   float cv, float eps, const float* __restrict__ skip) {
  if (skip && *skip != 0.f) return;  // the batch had an out-of-range label: no parameter or moment changes
  const long ti = chunks[2 * blockIdx.x], start = chunks[2 * blockIdx.x + 1];
  const SegAdamTensor t = ts[ti];
  const long end = std::min<long>(t.n, start + chunk);
  for (long i = start + threadIdx.x; i < end; i += 256) {
    const float g = t.g[i];
    float m = t.m[i], v = t.v[i];
    m = m + w * (g - m);
    v = v * b2;
    v = v + cv * g * g;
    const float d = sqrtf(v) / t.bc2_sqrt + eps;
    t.p[i] = t.p[i] + t.step_size * (m / d);
    t.m[i] = m;
    t.v[i] = v;
  }
}

}  // namespace

// tensors: device array of ntensors SegAdamTensor; chunks: device array of nchunks
// (tensor index, first element) int64 pairs, each chunk <= `chunk` elements.
// one_minus_beta1 / one_minus_beta2 are 1 - beta rounded once from double (torch
// passes the double 1 - beta as the lerp weight / addcmul value), not 1.f - (float)beta.
SEG_API int seg_adam_step_skip(const SegAdamTensor* tensors, const long* chunks, int nchunks, int chunk,
                               float one_minus_beta1, float beta2, float one_minus_beta2, float eps, const float* skip,
                               hipStream_t stream) {
  if (nchunks < 0 || chunk < 1) return (int)hipErrorInvalidValue;
  if (nchunks == 0) return (int)hipSuccess;
  hipLaunchKernelGGL(adam_kernel, dim3(nchunks), dim3(256), 0, stream, tensors, chunks, chunk, one_minus_beta1, beta2,
                     one_minus_beta2, eps, skip);
  SEG_RET_LAST();
}
SEG_API int seg_adam_step(const SegAdamTensor* tensors, const long* chunks, int nchunks, int chunk,
                          float one_minus_beta1, float beta2, float one_minus_beta2, float eps, hipStream_t stream) {
  return seg_adam_step_skip(tensors, chunks, nchunks, chunk, one_minus_beta1, beta2, one_minus_beta2, eps, nullptr,
                            stream);
}

// ---- AdamW, global-norm clipping -------------------------------------------------------
//
// seg_adamw_step: torch's foreach AdamW (torch/optim/adam.py::_multi_tensor_adam with
// decoupled_weight_decay=True), the Adam arithmetic above with two more fp32 multiplies:
//   g = g * (*grad_scale)                  the clip coefficient, applied as the gradient is loaded
//   p = p * decay                          _foreach_mul_(params, 1 - lr * weight_decay)
// Both are rounded products of their own (mul_rn: never contracted into the add that
// follows), so decay == 1 and no grad_scale is bit for bit seg_adam_step_skip, and a fused
// grad_scale is bit for bit seg_grad_scale followed by the unscaled step.  Multiplying by
// exactly 1.f changes no value, so neither multiply needs a branch.
//
// seg_grad_sumsq: the global L2 norm of every gradient in the table.  One block per chunk
// writes its sum of squares to part[block]; a second, one-block launch adds the partials in
// a fixed order (in double) and writes out[0..2].  No atomics: the result is the same bit
// pattern on every run.  The second launch instead of a last-block-done ticket: it needs no
// zeroed counter in the workspace and no cross-XCD hand-off, and its cost is one kernel
// boundary.
struct SegAdamWTensor {  // 56 bytes, the layout seg_amd/optim.py packs (_pack_w)
  float* p;
  const float* g;
  float* m;
  float* v;
  long n;
  float step_size;  // -lr / bc1
  float bc2_sqrt;   // sqrt(1 - b2^t)
  float decay;      // float(1 - lr * weight_decay)
  float pad;
};

namespace {

// a * b rounded to fp32 by itself: the empty asm hides the product from the contraction pass
__device__ __forceinline__ float mul_rn(float a, float b) {
  float r = a * b;
  asm("" : "+v"(r));
  return r;
}

__global__ __launch_bounds__(256) void adamw_kernel(const SegAdamWTensor* __restrict__ ts,
                                                    const long* __restrict__ chunks, int chunk, float w, float b2,
                                                    float cv, float eps, const float* __restrict__ skip,
                                                    const float* __restrict__ grad_scale) {
  if (skip && *skip != 0.f) return;
  const float gs = grad_scale ? *grad_scale : 1.f;
  const long ti = chunks[2 * blockIdx.x], start = chunks[2 * blockIdx.x + 1];
  const SegAdamWTensor t = ts[ti];
  const long end = std::min<long>(t.n, start + chunk);
  for (long i = start + threadIdx.x; i < end; i += 256) {
    const float g = mul_rn(t.g[i], gs);
    float m = t.m[i], v = t.v[i];
    const float p = mul_rn(t.p[i], t.decay);
    m = m + w * (g - m);
    v = v * b2;
    v = v + cv * g * g;
    const float d = sqrtf(v) / t.bc2_sqrt + eps;
    t.p[i] = p + t.step_size * (m / d);
    t.m[i] = m;
    t.v[i] = v;
  }
}

// part[block] = sum of g^2 over the block's chunk: per thread a serial fma chain over its
// <= chunk / 256 elements, then the 6-level wave butterfly and a 2-level sum of the 4 waves.
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const SegAdamWTensor* __restrict__ ts,
                                                         const long* __restrict__ chunks, int chunk,
                                                         float* __restrict__ part) {
  __shared__ float ws[4];
  const long ti = chunks[2 * blockIdx.x], start = chunks[2 * blockIdx.x + 1];
  const float* __restrict__ g = ts[ti].g;
  const long end = std::min<long>(ts[ti].n, start + chunk);
  float acc = 0.f;
  for (long i = start + threadIdx.x; i < end; i += 256) {
    const float x = g[i];
    acc = fmaf(x, x, acc);
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
}

// One block: thread t adds part[t], part[t + 256], ... in double, then a fixed tree over the 256 sums.
__global__ __launch_bounds__(256) void grad_norm_finalize_kernel(const float* __restrict__ part, int n,
                                                                 float max_norm, float* __restrict__ out) {
  __shared__ double s[256];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) acc += (double)part[i];
  s[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(s[0]);
    float coef = 1.f;
    if (max_norm > 0.f && max_norm < __builtin_inff()) {
      coef = max_norm / (norm + 1e-6f);  // torch.nn.utils.clip_grads_with_norm_
      coef = coef > 1.f ? 1.f : coef;    // clamp(max=1): a NaN stays a NaN
    }
    out[0] = norm;
    out[1] = coef;
    out[2] = (norm == norm && norm != __builtin_inff()) ? 0.f : 1.f;
  }
}

__global__ __launch_bounds__(256) void grad_scale_kernel(const SegAdamWTensor* __restrict__ ts,
                                                         const long* __restrict__ chunks, int chunk,
                                                         const float* __restrict__ scale) {
  const float s = *scale;
  if (s == 1.f) return;  // nothing was clipped: the gradients stay as they are, untouched
  const long ti = chunks[2 * blockIdx.x], start = chunks[2 * blockIdx.x + 1];
  float* __restrict__ g = const_cast<float*>(ts[ti].g);
  const long end = std::min<long>(ts[ti].n, start + chunk);
  for (long i = start + threadIdx.x; i < end; i += 256) g[i] = g[i] * s;
}

}  // namespace

// tensors: device array of SegAdamWTensor (passed as const void*: include/segamd.h documents the
// record); chunks / nchunks / chunk and the four scalars as seg_adam_step_skip.  skip: as there.
// grad_scale: one device float every gradient element is multiplied by as it is loaded (NULL = 1);
// .grad itself is not written.
SEG_API int seg_adamw_step(const void* tensors, const long* chunks, int nchunks, int chunk, float one_minus_beta1,
                           float beta2, float one_minus_beta2, float eps, const float* skip, const float* grad_scale,
                           hipStream_t stream) {
  if (nchunks < 0 || chunk < 1) return (int)hipErrorInvalidValue;
  if (nchunks == 0) return (int)hipSuccess;
  hipLaunchKernelGGL(adamw_kernel, dim3(nchunks), dim3(256), 0, stream, (const SegAdamWTensor*)tensors, chunks, chunk,
                     one_minus_beta1, beta2, one_minus_beta2, eps, skip, grad_scale);
  SEG_RET_LAST();
}

// Floats of workspace seg_grad_sumsq needs: one partial per chunk.
SEG_API long seg_grad_norm_workspace_floats(int nchunks) { return nchunks > 0 ? (long)nchunks : 0; }

// out[0] = sqrt(sum g^2) over the table (only g and n of each record are read);
// out[1] = min(max_norm / (out[0] + 1e-6), 1), or 1 when max_norm <= 0 or infinite; NaN when the norm is NaN;
// out[2] = 1 if the norm is inf or NaN, else 0.  work: seg_grad_norm_workspace_floats(nchunks) floats.
SEG_API int seg_grad_sumsq(const void* tensors, const long* chunks, int nchunks, int chunk, float max_norm,
                           float* work, float* out, hipStream_t stream) {
  if (nchunks < 0 || chunk < 1) return (int)hipErrorInvalidValue;
  if (nchunks == 0) return (int)hipSuccess;
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3(nchunks), dim3(256), 0, stream, (const SegAdamWTensor*)tensors, chunks,
                     chunk, work);
  hipLaunchKernelGGL(grad_norm_finalize_kernel, dim3(1), dim3(256), 0, stream, work, nchunks, max_norm, out);
  SEG_RET_LAST();
}

// g *= *scale in place over the table (only g and n are read); returns at once on the device when *scale == 1.
SEG_API int seg_grad_scale(const void* tensors, const long* chunks, int nchunks, int chunk, const float* scale,
                           hipStream_t stream) {
  if (nchunks < 0 || chunk < 1) return (int)hipErrorInvalidValue;
  if (nchunks == 0) return (int)hipSuccess;
  hipLaunchKernelGGL(grad_scale_kernel, dim3(nchunks), dim3(256), 0, stream, (const SegAdamWTensor*)tensors, chunks,
                     chunk, scale);
  SEG_RET_LAST();
}

// ---- weight averaging (seg_amd/ema.py) ---------------------------------------------------
//
// seg_ema_update: the exponential moving average of every floating-point state_dict entry (parameters and
// BatchNorm running statistics) in one launch over a chunk map of the optimizer's kind:
//   e = e + w * (p - e)                    torch.lerp(e, p, w) in its weight < 0.5 form, kept for every w in [0, 1]
// in fp32, w = float(1 - decay) formed in double on the host, as adam_kernel's 1 - beta1.  w == 0 and p == e both
// leave e as it is, bit for bit.  p is only read.  skip: adam_kernel's flag -- a step the device skipped is not
// averaged in either.
//
// seg_ema_swap: ema[i] <-> p[i].  Each element is read and written by the same lane, so there is nothing to
// order and no temporary in memory; two swaps restore both sides bit for bit.
//
// Both keep adam_kernel's walk (one 256-thread block per chunk, dword loads and stores): the pass is ~80 MB of
// traffic that the 256 MB of last-level cache holds, beside a step of 8-16 ms (DESIGN.md has the measurement).
struct SegEmaTensor {  // 24 bytes, the layout seg_amd/ema.py packs
  float* ema;
  float* p;
  long n;
};

namespace {

__global__ __launch_bounds__(256) void ema_update_kernel(const SegEmaTensor* __restrict__ ts,
                                                         const long* __restrict__ chunks, int chunk, float w,
                                                         const float* __restrict__ skip) {
  if (skip && *skip != 0.f) return;  // the optimizer step was skipped: the average does not move either
  const long ti = chunks[2 * blockIdx.x], start = chunks[2 * blockIdx.x + 1];
  const SegEmaTensor t = ts[ti];
  const float* __restrict__ p = t.p;
  float* __restrict__ e = t.ema;
  const long end = std::min<long>(t.n, start + chunk);
  for (long i = start + threadIdx.x; i < end; i += 256) {
    const float ev = e[i];
    e[i] = ev + w * (p[i] - ev);
  }
}

__global__ __launch_bounds__(256) void ema_swap_kernel(const SegEmaTensor* __restrict__ ts,
                                                       const long* __restrict__ chunks, int chunk) {
  const long ti = chunks[2 * blockIdx.x], start = chunks[2 * blockIdx.x + 1];
  const SegEmaTensor t = ts[ti];
  const long end = std::min<long>(t.n, start + chunk);
  for (long i = start + threadIdx.x; i < end; i += 256) {
    const float ev = t.ema[i], pv = t.p[i];
    t.ema[i] = pv;
    t.p[i] = ev;
  }
}

}  // namespace

// tensors: device array of SegEmaTensor (const void*: include/segamd.h documents the record); chunks / nchunks /
// chunk as seg_adam_step_skip.  one_minus_decay: float(1 - decay) from double.  skip: as seg_adam_step_skip.
SEG_API int seg_ema_update(const void* tensors, const long* chunks, int nchunks, int chunk, float one_minus_decay,
                           const float* skip, hipStream_t stream) {
  if (nchunks < 0 || chunk < 1) return (int)hipErrorInvalidValue;
  if (nchunks == 0) return (int)hipSuccess;
  hipLaunchKernelGGL(ema_update_kernel, dim3(nchunks), dim3(256), 0, stream, (const SegEmaTensor*)tensors, chunks,
                     chunk, one_minus_decay, skip);
  SEG_RET_LAST();
}

// ema[i] <-> p[i] over the table.
SEG_API int seg_ema_swap(const void* tensors, const long* chunks, int nchunks, int chunk, hipStream_t stream) {
  if (nchunks < 0 || chunk < 1) return (int)hipErrorInvalidValue;
  if (nchunks == 0) return (int)hipSuccess;
  hipLaunchKernelGGL(ema_swap_kernel, dim3(nchunks), dim3(256), 0, stream, (const SegEmaTensor*)tensors, chunks,
                     chunk);
  SEG_RET_LAST();
}

// ---- SGD with momentum (seg_amd.SGD) -----------------------------------------------------
//
// seg_sgd_step: torch's foreach SGD (torch/optim/sgd.py::_multi_tensor_sgd) over adam_kernel's chunk map, each
// element read once and written once, fp32, in torch's order:
//   g = g * (*grad_scale)                  the clip coefficient, as adamw_kernel applies it (mul_rn)
//   d = g + weight_decay * p               _foreach_add(grads, params, alpha=weight_decay): the L2 form
//   buf = d                                a tensor's first step: torch clones d, no dampening (the seed flag)
//   buf = buf * momentum                   _foreach_mul_(bufs, momentum), a rounded product of its own
//   buf = buf + (1 - dampening) * d        _foreach_add_(bufs, grads, alpha=1 - dampening)
//   d = nesterov ? d + momentum * buf : buf
//   p = p - lr * d                         _foreach_add_(params, grads, alpha=-lr)
// The record is SegAdamWTensor: m is the momentum buffer, v is unused, and the last float (`pad`) is the seed
// flag -- non-zero on the step that creates the tensor's buffer, which then receives d itself instead of the
// recurrence (0 * momentum + (1 - dampening) * d is not d when dampening != 0).  The scalars are per parameter
// group and so kernel arguments.  weight_decay == 0 is a select on the argument, not a multiplication by zero:
// without decay d is g bit for bit whatever p holds.  momentum == 0 is an instantiation of its own (MOM = false)
// without the buffer's load and store: the pointer (NULL) is never read.  With MOM the three loads are issued
// together in front of the arithmetic, as adam_kernel's four are -- on a seeding step the buffer (zeros) is loaded
// and its value dropped by the select, rather than a branch putting its load behind the other two.  skip:
// adam_kernel's flag.  Five streams (p, g, buf read; p, buf written) to adam_kernel's seven.
namespace {

template <bool MOM>
__global__ __launch_bounds__(256) void sgd_kernel(const SegAdamWTensor* __restrict__ ts,
                                                  const long* __restrict__ chunks, int chunk, float lr, float momentum,
                                                  float omd, float wd, int nesterov, const float* __restrict__ skip,
                                                  const float* __restrict__ grad_scale) {
  if (skip && *skip != 0.f) return;  // the batch had an out-of-range label: no parameter or buffer changes
  const float gs = grad_scale ? *grad_scale : 1.f;
  const long ti = chunks[2 * blockIdx.x], start = chunks[2 * blockIdx.x + 1];
  const SegAdamWTensor t = ts[ti];
  const bool seed = t.pad != 0.f;
  const long end = std::min<long>(t.n, start + chunk);
  for (long i = start + threadIdx.x; i < end; i += 256) {
    float d = mul_rn(t.g[i], gs);
    const float p = t.p[i];
    float b = MOM ? t.m[i] : 0.f;
    d = wd != 0.f ? d + wd * p : d;
    if (MOM) {
      b = mul_rn(b, momentum);
      b = b + omd * d;
      b = seed ? d : b;
      t.m[i] = b;
      d = nesterov ? d + momentum * b : b;
    }
    t.p[i] = p - lr * d;
  }
}

}  // namespace

// tensors: device array of SegAdamWTensor (const void*: include/segamd.h documents how SGD fills the record);
// chunks / nchunks / chunk / skip / grad_scale as seg_adamw_step.  one_minus_dampening: float(1 - dampening) formed
// in double.  momentum == 0: no record's m is read.
SEG_API int seg_sgd_step(const void* tensors, const long* chunks, int nchunks, int chunk, float lr, float momentum,
                         float one_minus_dampening, float weight_decay, int nesterov, const float* skip,
                         const float* grad_scale, hipStream_t stream) {
  if (nchunks < 0 || chunk < 1) return (int)hipErrorInvalidValue;
  if (nchunks == 0) return (int)hipSuccess;
  const auto kernel = momentum != 0.f ? sgd_kernel<true> : sgd_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3(nchunks), dim3(256), 0, stream, (const SegAdamWTensor*)tensors, chunks, chunk, lr,
                     momentum, one_minus_dampening, weight_decay, nesterov, skip, grad_scale);
  SEG_RET_LAST();
}
