// Cross-entropy (fused log-softmax + NLL + backward seed), evaluation counter and
// a device spin kernel.
//
// the reference runs log_softmax, nll_loss (mean) and, in
// backward, their two gradients as separate ATen kernels.  Here ONE pass per row
// computes the row loss AND d(logits) = (softmax − onehot) * scale (scale = 1/B
// for the mean), so backward only rescales by the incoming grad.  Per-row losses
// are summed by a second single-block kernel in fixed order (deterministic).
// K26: the eval loop's argmax/eq/sum/.item() per batch becomes an on-device
// argmax+compare+counter with one D2H read per evaluation.
// The label-smoothed loss and the top-k / test-loss metrics (docs/KERNELS.md) keep the same
// shape: a row kernel plus a single-block fixed-order finish, two launches per call.
#include "common.h"

namespace dm {

template <typename T> __device__ __forceinline__ float ldv(const T* p, long long i);
template <> __device__ __forceinline__ float ldv<float>(const float* p, long long i) { return p[i]; }
template <> __device__ __forceinline__ float ldv<bf16_t>(const bf16_t* p, long long i) {
  return bf2f(p[i]);
}

// one wave per row; block = 256 (4 rows)
template <typename T>
__global__ void __launch_bounds__(256) ce_fwd_bwd_kernel(const T* __restrict__ logits,
                                                         const long long* __restrict__ labels,
                                                         float* __restrict__ rowloss,
                                                         T* __restrict__ dlogits, int B, int C,
                                                         float scale, int ignore_index) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B) return;
  const T* x = logits + (long long)row * C;
  float m = -INFINITY;
  for (int c = lane; c < C; c += 64) m = fmaxf(m, ldv(x, c));
  m = wave_max(m);
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += __expf(ldv(x, c) - m);
  s = wave_sum(s);
  const float lse = m + __logf(s);
  const long long y = labels[row];
  const bool valid = y != ignore_index && y >= 0 && y < C;
  if (lane == 0) rowloss[row] = valid ? (lse - ldv(x, y)) : 0.f;
  if (dlogits) {
    T* d = dlogits + (long long)row * C;
    const float inv = 1.f / s;
    for (int c = lane; c < C; c += 64) {
      float g = valid ? (__expf(ldv(x, c) - m) * inv - (c == y ? 1.f : 0.f)) * scale : 0.f;
      if constexpr (sizeof(T) == 4) d[c] = g;
      else d[c] = f2bf(g);
    }
  }
}

__global__ void __launch_bounds__(256) sum_scale_kernel(const float* __restrict__ v, int n,
                                                        float scale, float* __restrict__ out) {
  __shared__ float red[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) s += v[i];
  s = block_sum(s, red);
  if (threadIdx.x == 0) out[0] = s * scale;
}

// correct[0] += #rows with argmax(logits[row]) == label[row]
template <typename T>
__global__ void __launch_bounds__(256) argmax_count_kernel(const T* __restrict__ logits,
                                                           const long long* __restrict__ labels,
                                                           int B, int C,
                                                           unsigned long long* __restrict__ correct) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B) return;
  const T* x = logits + (long long)row * C;
  float best = -INFINITY;
  int arg = 0x7fffffff;
  for (int c = lane; c < C; c += 64) {
    const float v = ldv(x, c);
    if (v > best) { best = v; arg = c; }  // first max within the lane's strided set
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int oa = __shfl_xor(arg, o, 64);
    if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }  // torch: first index
  }
  if (lane == 0 && arg == labels[row]) atomicAdd(correct, 1ull);
}

// Label-smoothed cross-entropy, same layout as ce_fwd_bwd_kernel (which stays the eps = 0
// path, untouched): the target distribution is (1-eps)*onehot + eps/C, so
//   rowloss = (1-eps)*(lse - x_y) + eps*(lse - mean_c x_c)
//   dlogits = (softmax - (1-eps)*onehot - eps/C) * scale
// The only extra work is the row sum of x, accumulated in the max pass.
template <typename T>
__global__ void __launch_bounds__(256) ce_smooth_fwd_bwd_kernel(
    const T* __restrict__ logits, const long long* __restrict__ labels,
    float* __restrict__ rowloss, T* __restrict__ dlogits, int B, int C, float scale, float eps,
    int ignore_index) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B) return;
  const T* x = logits + (long long)row * C;
  float m = -INFINITY, sx = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float v = ldv(x, c);
    m = fmaxf(m, v);
    sx += v;
  }
  m = wave_max(m);
  sx = wave_sum(sx);
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += __expf(ldv(x, c) - m);
  s = wave_sum(s);
  const float lse = m + __logf(s);
  const long long y = labels[row];
  const bool valid = y != ignore_index && y >= 0 && y < C;
  const float uni = eps / (float)C;
  if (lane == 0)
    rowloss[row] = valid ? (1.f - eps) * (lse - ldv(x, y)) + eps * (lse - sx / (float)C) : 0.f;
  if (dlogits) {
    T* d = dlogits + (long long)row * C;
    const float inv = 1.f / s;
    for (int c = lane; c < C; c += 64) {
      float g = valid ? (__expf(ldv(x, c) - m) * inv - (c == y ? 1.f - eps : 0.f) - uni) * scale
                      : 0.f;
      if constexpr (sizeof(T) == 4) d[c] = g;
      else d[c] = f2bf(g);
    }
  }
}

// Mixed-target cross-entropy (mixup / CutMix), the smoothed kernel with two labels per row: the
// target is lam*smooth(ya) + (1-lam)*smooth(yb), so with t = lam*x_ya + (1-lam)*x_yb
//   rowloss = (1-eps)*(lse - t) + eps*(lse - mean_c x_c)
//   dlogits = (softmax - (1-eps)*(lam*[c==ya] + (1-lam)*[c==yb]) - eps/C) * scale
// (ya == yb gives weight 1).  A row is valid iff both labels are in [0,C) and neither is
// ignore_index; an invalid row has loss 0 and zero gradient, and its labels index nothing.
template <typename T>
__global__ void __launch_bounds__(256) ce_mix_fwd_bwd_kernel(
    const T* __restrict__ logits, const long long* __restrict__ ya,
    const long long* __restrict__ yb, const float* __restrict__ lam, float* __restrict__ rowloss,
    T* __restrict__ dlogits, int B, int C, float scale, float eps, int ignore_index) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B) return;
  const T* x = logits + (long long)row * C;
  float m = -INFINITY, sx = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float v = ldv(x, c);
    m = fmaxf(m, v);
    sx += v;
  }
  m = wave_max(m);
  sx = wave_sum(sx);
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += __expf(ldv(x, c) - m);
  s = wave_sum(s);
  const float lse = m + __logf(s);
  const long long a = ya[row], b = yb[row];
  const bool valid = a != ignore_index && a >= 0 && a < C && b != ignore_index && b >= 0 && b < C;
  const float la = lam[row], lb = 1.f - la;
  const float uni = eps / (float)C;
  if (lane == 0) {
    const float t = valid ? la * ldv(x, a) + lb * ldv(x, b) : 0.f;
    rowloss[row] = valid ? (1.f - eps) * (lse - t) + eps * (lse - sx / (float)C) : 0.f;
  }
  if (dlogits) {
    T* d = dlogits + (long long)row * C;
    const float inv = 1.f / s;
    const float wa = (1.f - eps) * la, wb = (1.f - eps) * lb;
    for (int c = lane; c < C; c += 64) {
      const float hot = (c == a ? wa : 0.f) + (c == b ? wb : 0.f);
      float g = valid ? (__expf(ldv(x, c) - m) * inv - hot - uni) * scale : 0.f;
      if constexpr (sizeof(T) == 4) d[c] = g;
      else d[c] = f2bf(g);
    }
  }
}

// Evaluation metrics, one pass per batch.  Per row: the (unsmoothed) NLL and the label's rank
//   rank = #{c : x_c > x_y} + #{c < y : x_c == x_y}
// so that the row hits at k iff rank < k (k = 1: argmax_count_kernel's first-index rule).  A
// label outside [0, C) is never used as an index: the row gets loss 0 and rank INT_MAX (a
// miss at every k); so does, for the rank, a NaN label logit.
#define DM_RANK_MISS 0x7fffffff
template <typename T>
__global__ void __launch_bounds__(256) eval_rows_kernel(const T* __restrict__ logits,
                                                        const long long* __restrict__ labels,
                                                        float* __restrict__ rowloss,
                                                        int* __restrict__ rowrank, int B, int C) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B) return;
  const T* x = logits + (long long)row * C;
  const long long y = labels[row];
  const bool valid = y >= 0 && y < C;
  const float xy = valid ? ldv(x, y) : 0.f;
  const int yi = valid ? (int)y : 0;
  float m = -INFINITY;
  int above = 0;
  for (int c = lane; c < C; c += 64) {
    const float v = ldv(x, c);
    m = fmaxf(m, v);
    above += (v > xy || (v == xy && c < yi)) ? 1 : 0;
  }
  m = wave_max(m);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) above += __shfl_xor(above, o, 64);
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += __expf(ldv(x, c) - m);
  s = wave_sum(s);
  if (lane == 0) {
    rowloss[row] = valid ? (m + __logf(s)) - xy : 0.f;
    rowrank[row] = (valid && xy == xy) ? above : DM_RANK_MISS;
  }
}

// Adds one batch's rows into the persistent state in a fixed order (single block, strided
// partial sums, shared-memory tree): counts = {n, top-1 hits, top-k hits}, loss = float64
// sum of the row losses.  No atomics, so two runs over the same batches give the same bits.
__global__ void __launch_bounds__(256) eval_finish_kernel(const float* __restrict__ rowloss,
                                                          const int* __restrict__ rowrank, int B,
                                                          int k, long long* __restrict__ counts,
                                                          double* __restrict__ loss) {
  __shared__ double sl[256];
  __shared__ int s1[256], sk[256];
  double l = 0.0;
  int h1 = 0, hk = 0;
  for (int i = threadIdx.x; i < B; i += 256) {
    l += (double)rowloss[i];
    const int r = rowrank[i];
    h1 += r < 1 ? 1 : 0;
    hk += r < k ? 1 : 0;
  }
  sl[threadIdx.x] = l; s1[threadIdx.x] = h1; sk[threadIdx.x] = hk;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      sl[threadIdx.x] += sl[threadIdx.x + o];
      s1[threadIdx.x] += s1[threadIdx.x + o];
      sk[threadIdx.x] += sk[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    counts[0] += B;
    counts[1] += s1[0];
    counts[2] += sk[0];
    loss[0] += sl[0];
  }
}

// Busy-wait on the device for `us` microseconds (straggler injection, graph-safe).
__global__ void spin_kernel(unsigned long long cycles) {
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  while (__builtin_amdgcn_s_memrealtime() - t0 < cycles) __builtin_amdgcn_s_sleep(8);
}

// ------------------------------------------------------------------ launchers
void cross_entropy(const void* logits, const long long* labels, float* rowloss, float* loss,
                   void* dlogits, int B, int C, float scale, int ignore_index, bool bf16,
                   hipStream_t st) {
  const int grid = (B + 3) / 4;
  if (bf16)
    ce_fwd_bwd_kernel<bf16_t><<<grid, 256, 0, st>>>((const bf16_t*)logits, labels, rowloss,
                                                    (bf16_t*)dlogits, B, C, scale, ignore_index);
  else
    ce_fwd_bwd_kernel<float><<<grid, 256, 0, st>>>((const float*)logits, labels, rowloss,
                                                   (float*)dlogits, B, C, scale, ignore_index);
  sum_scale_kernel<<<1, 256, 0, st>>>(rowloss, B, scale, loss);
}

void argmax_count(const void* logits, const long long* labels, int B, int C,
                  unsigned long long* correct, bool bf16, hipStream_t st) {
  const int grid = (B + 3) / 4;
  if (bf16)
    argmax_count_kernel<bf16_t><<<grid, 256, 0, st>>>((const bf16_t*)logits, labels, B, C, correct);
  else
    argmax_count_kernel<float><<<grid, 256, 0, st>>>((const float*)logits, labels, B, C, correct);
}

void cross_entropy_smooth(const void* logits, const long long* labels, float* rowloss, float* loss,
                          void* dlogits, int B, int C, float scale, float eps, int ignore_index,
                          bool bf16, hipStream_t st) {
  const int grid = (B + 3) / 4;
  if (bf16)
    ce_smooth_fwd_bwd_kernel<bf16_t><<<grid, 256, 0, st>>>((const bf16_t*)logits, labels, rowloss,
                                                           (bf16_t*)dlogits, B, C, scale, eps,
                                                           ignore_index);
  else
    ce_smooth_fwd_bwd_kernel<float><<<grid, 256, 0, st>>>((const float*)logits, labels, rowloss,
                                                          (float*)dlogits, B, C, scale, eps,
                                                          ignore_index);
  sum_scale_kernel<<<1, 256, 0, st>>>(rowloss, B, scale, loss);
}

void cross_entropy_mix(const void* logits, const long long* ya, const long long* yb,
                       const float* lam, float* rowloss, float* loss, void* dlogits, int B, int C,
                       float scale, float eps, int ignore_index, bool bf16, hipStream_t st) {
  const int grid = (B + 3) / 4;
  if (bf16)
    ce_mix_fwd_bwd_kernel<bf16_t><<<grid, 256, 0, st>>>((const bf16_t*)logits, ya, yb, lam, rowloss,
                                                        (bf16_t*)dlogits, B, C, scale, eps,
                                                        ignore_index);
  else
    ce_mix_fwd_bwd_kernel<float><<<grid, 256, 0, st>>>((const float*)logits, ya, yb, lam, rowloss,
                                                       (float*)dlogits, B, C, scale, eps,
                                                       ignore_index);
  sum_scale_kernel<<<1, 256, 0, st>>>(rowloss, B, scale, loss);
}

void eval_metrics(const void* logits, const long long* labels, float* rowloss, int* rowrank, int B,
                  int C, int k, long long* counts, double* loss, bool bf16, hipStream_t st) {
  const int grid = (B + 3) / 4;
  if (bf16)
    eval_rows_kernel<bf16_t><<<grid, 256, 0, st>>>((const bf16_t*)logits, labels, rowloss, rowrank,
                                                   B, C);
  else
    eval_rows_kernel<float><<<grid, 256, 0, st>>>((const float*)logits, labels, rowloss, rowrank,
                                                  B, C);
  eval_finish_kernel<<<1, 256, 0, st>>>(rowloss, rowrank, B, k, counts, loss);
}

void spin_us(double us, hipStream_t st) {
  // s_memrealtime runs at a constant 100 MHz on CDNA
  const unsigned long long cycles = (unsigned long long)(us * 100.0);
  spin_kernel<<<1, 64, 0, st>>>(cycles);
}

}  // namespace dm
