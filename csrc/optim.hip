// Fused multi-tensor optimiser steps over ONE flat parameter buffer.
//
// Reference semantics:
//   GD    : p -= lr*g                               (task1/pytorch/MyOptimizer.py:24)
//   Adam  : m = b1 m + (1-b1) g ; v = b2 v + (1-b2) g^2 ;
//           p -= lr/(sqrt(v)+eps) * m               (MyOptimizer.py:39-43, no bias corr.)
//   SGD   : torch.optim.SGD(momentum, dampening, nesterov, weight_decay)
//           used by task2/model.py:131, task3/model.py:118.
// The reference issues ~8 elementwise kernels per parameter tensor; here one
// launch covers every parameter (all params are views of one flat fp32 buffer),
// the 1/world_size gradient average is folded in as `grad_scale`, and an
// optional bf16 shadow copy of the updated weights is written in the same pass
// so the next forward reads bf16 weights without a separate cast kernel.
#include "common.h"

namespace dm {

template <bool HAS_MOM, bool NESTEROV, bool WRITE_BF16>
__global__ void __launch_bounds__(256) sgd_kernel(
    float* __restrict__ p, const float* __restrict__ g, float* __restrict__ mom,
    bf16_t* __restrict__ pbf, long long n4, long long n, float lr, float momentum,
    float dampening, float wd, float gscale, int first) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i < n4; i += stride) {
    float4 pv = reinterpret_cast<float4*>(p)[i];
    float4 gv = reinterpret_cast<const float4*>(g)[i];
    float pa[4] = {pv.x, pv.y, pv.z, pv.w};
    float ga[4] = {gv.x, gv.y, gv.z, gv.w};
    float ma[4] = {0.f, 0.f, 0.f, 0.f};
    if (HAS_MOM && !first) {
      float4 mv = reinterpret_cast<float4*>(mom)[i];
      ma[0] = mv.x; ma[1] = mv.y; ma[2] = mv.z; ma[3] = mv.w;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float d = ga[j] * gscale + wd * pa[j];
      if (HAS_MOM) {
        ma[j] = first ? d : momentum * ma[j] + (1.f - dampening) * d;
        d = NESTEROV ? d + momentum * ma[j] : ma[j];
      }
      pa[j] -= lr * d;
    }
    reinterpret_cast<float4*>(p)[i] = make_float4(pa[0], pa[1], pa[2], pa[3]);
    if (HAS_MOM)
      reinterpret_cast<float4*>(mom)[i] = make_float4(ma[0], ma[1], ma[2], ma[3]);
    if (WRITE_BF16)
      reinterpret_cast<uint2*>(pbf)[i] =
          make_uint2(pack_bf2(pa[0], pa[1]), pack_bf2(pa[2], pa[3]));
  }
  // scalar tail (n not a multiple of 4)
  for (long long t = n4 * 4 + (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n;
       t += stride) {
    float pv = p[t];
    float d = g[t] * gscale + wd * pv;
    if (HAS_MOM) {
      float m = first ? d : momentum * mom[t] + (1.f - dampening) * d;
      mom[t] = m;
      d = NESTEROV ? d + momentum * m : m;
    }
    pv -= lr * d;
    p[t] = pv;
    if (WRITE_BF16) pbf[t] = f2bf(pv);
  }
}

template <bool WRITE_BF16>
__global__ void __launch_bounds__(256) adam_kernel(
    float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
    float* __restrict__ v, bf16_t* __restrict__ pbf, long long n, float lr, float b1,
    float b2, float eps, float wd, float gscale, float bc1, float bc2) {
  // bc1 = 1/(1-b1^t), bc2 = 1/(1-b2^t)  (1.0 for the reference's no-correction form)
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long n4 = n >> 2;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 pv = reinterpret_cast<float4*>(p)[i];
    float4 gv = reinterpret_cast<const float4*>(g)[i];
    float4 mv = reinterpret_cast<float4*>(m)[i];
    float4 vv = reinterpret_cast<float4*>(v)[i];
    float pa[4] = {pv.x, pv.y, pv.z, pv.w}, ga[4] = {gv.x, gv.y, gv.z, gv.w};
    float ma[4] = {mv.x, mv.y, mv.z, mv.w}, va[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float gg = ga[j] * gscale + wd * pa[j];
      ma[j] = b1 * ma[j] + (1.f - b1) * gg;
      va[j] = b2 * va[j] + (1.f - b2) * gg * gg;
      pa[j] -= lr * (ma[j] * bc1) / (sqrtf(va[j] * bc2) + eps);
    }
    reinterpret_cast<float4*>(p)[i] = make_float4(pa[0], pa[1], pa[2], pa[3]);
    reinterpret_cast<float4*>(m)[i] = make_float4(ma[0], ma[1], ma[2], ma[3]);
    reinterpret_cast<float4*>(v)[i] = make_float4(va[0], va[1], va[2], va[3]);
    if (WRITE_BF16)
      reinterpret_cast<uint2*>(pbf)[i] =
          make_uint2(pack_bf2(pa[0], pa[1]), pack_bf2(pa[2], pa[3]));
  }
  for (long long t = n4 * 4 + (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n;
       t += stride) {
    float gg = g[t] * gscale + wd * p[t];
    float mm = b1 * m[t] + (1.f - b1) * gg;
    float vv = b2 * v[t] + (1.f - b2) * gg * gg;
    m[t] = mm;
    v[t] = vv;
    float pv = p[t] - lr * (mm * bc1) / (sqrtf(vv * bc2) + eps);
    p[t] = pv;
    if (WRITE_BF16) pbf[t] = f2bf(pv);
  }
}

__global__ void __launch_bounds__(256) cast_f32_bf16_kernel(const float* __restrict__ x,
                                                            bf16_t* __restrict__ y,
                                                            long long n) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long n4 = n >> 2;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 v = reinterpret_cast<const float4*>(x)[i];
    reinterpret_cast<uint2*>(y)[i] = make_uint2(pack_bf2(v.x, v.y), pack_bf2(v.z, v.w));
  }
  for (long long t = n4 * 4 + (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n;
       t += stride)
    y[t] = f2bf(x[t]);
}

// out[i] = scale * sum_r x[r*n + i]  (all-gather aggregation: [ws, N] -> [N])
__global__ void __launch_bounds__(256) rows_mean_kernel(const float* __restrict__ x,
                                                        float* __restrict__ out, int rows,
                                                        long long n, float scale) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    float s = 0.f;
    for (int r = 0; r < rows; ++r) s += x[(long long)r * n + i];
    out[i] = s * scale;
  }
}

// ---------------------------------------------------------------- launchers
void sgd_step(float* p, const float* g, float* mom, bf16_t* pbf, long long n, float lr,
              float momentum, float dampening, float wd, float gscale, bool nesterov,
              bool first, hipStream_t st) {
  if (n <= 0) return;
  const long long n4 = ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)mom | (uintptr_t)pbf) & 15) == 0)
                           ? (n >> 2) : 0;  // vector path only when 16-B aligned
  const int grid = grid_for(n4 ? n4 : n, 256);
  const bool hm = momentum != 0.f;
#define DM_SGD(HM, NE, WB)                                                            \
  sgd_kernel<HM, NE, WB><<<grid, 256, 0, st>>>(p, g, mom, pbf, n4, n, lr, momentum, \
                                               dampening, wd, gscale, first ? 1 : 0)
  if (pbf) {
    if (!hm) DM_SGD(false, false, true);
    else if (nesterov) DM_SGD(true, true, true);
    else DM_SGD(true, false, true);
  } else {
    if (!hm) DM_SGD(false, false, false);
    else if (nesterov) DM_SGD(true, true, false);
    else DM_SGD(true, false, false);
  }
#undef DM_SGD
}

void adam_step(float* p, const float* g, float* m, float* v, bf16_t* pbf, long long n,
               float lr, float b1, float b2, float eps, float wd, float gscale, float bc1,
               float bc2, hipStream_t st) {
  if (n <= 0) return;
  const int grid = grid_for((n + 3) / 4, 256);
  if (pbf)
    adam_kernel<true><<<grid, 256, 0, st>>>(p, g, m, v, pbf, n, lr, b1, b2, eps, wd, gscale,
                                            bc1, bc2);
  else
    adam_kernel<false><<<grid, 256, 0, st>>>(p, g, m, v, pbf, n, lr, b1, b2, eps, wd, gscale,
                                             bc1, bc2);
}

void cast_f32_bf16(const float* x, bf16_t* y, long long n, hipStream_t st) {
  if (n <= 0) return;
  cast_f32_bf16_kernel<<<grid_for((n + 3) / 4, 256), 256, 0, st>>>(x, y, n);
}

void rows_mean(const float* x, float* out, int rows, long long n, float scale,
               hipStream_t st) {
  if (n <= 0) return;
  rows_mean_kernel<<<grid_for(n, 256), 256, 0, st>>>(x, out, rows, n, scale);
}

}  // namespace dm
