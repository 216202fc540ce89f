// Fused LARS (layer-wise adaptive rate scaling, You et al. 2017) over the flat
// parameter buffer: three launches per step, whatever the number of tensors.
//
// Per tensor t with weights w, raw gradient g and momentum buffer b:
//   g' = c * grad_scale * g
//   adapted:  r = eta*|w| / (|g'| + wd*|w| + eps)  if |w| > 0 and |g'| > 0 else 1
//             d = r * (g' + wd*w)
//   else:     d = g'                                   (r = 1, no weight decay)
//   b = mu*b + d ;  w -= lr * (nesterov ? d + mu*b : b)
// with c = min(1, max_grad_norm / (G + 1e-6)), G = sqrt(sum_t |grad_scale*g_t|^2)
// when clipping is on and c = 1 otherwise.
//
// Tables (built once per optimiser on the host, see lars_table in bindings.cpp):
//   seg  [n_tensors, 5] int64 : offset, numel, adapted, first chunk, chunk count
//   chunk[n_chunks,  3] int64 : start (element offset in the flat buffer), length, tensor
// A chunk lies inside one tensor, starts on a 16-B boundary and holds at most
// LARS_CHUNK elements, so the slot padding is never touched.
//
//   1. lars_partial  : one 256-thread block per chunk -> partial[chunk] = (sum w^2, sum (gs*g)^2)
//   2. lars_totals   : one wave per tensor sums that tensor's partials in a fixed order
//                      -> tot[tensor]
//   3. lars_update   : one block per chunk: c from the per-tensor sums (same order in every
//                      block, only when clipping), r from its tensor's totals, then the
//                      update; a tensor's first chunk writes the logging stats
// Every sum has a fixed order and there are no atomics: the same state gives the same
// bits, on every replica.  lr and the other hyper-parameters are read from a device
// tensor, so a step captured in a hipGraph follows a schedule written by the host.
#include "common.h"
#include "kernels.h"

namespace dm {

namespace {

constexpr int LARS_CHUNK = 4096;  // elements; 4 float4 per thread of a 256-thread block
constexpr int LARS_VEC = LARS_CHUNK / 4 / 256;  // 16-B vectors per thread and chunk
static_assert(LARS_CHUNK % (4 * 256) == 0, "a chunk is whole 16-B vectors for every thread");

// hyper-parameter slots of the device tensor
enum { H_LR = 0, H_MU, H_WD, H_ETA, H_EPS, H_GSCALE, H_MAXNORM, H_COUNT };

struct Chunk {
  long long start, len, tensor;
};

__device__ __forceinline__ bool chunk_ok(const Chunk& c, long long total, int n_tensors) {
  return c.start >= 0 && c.len >= 0 && c.len <= LARS_CHUNK && c.start + c.len <= total &&
         (c.start & 3) == 0 && c.tensor >= 0 && c.tensor < n_tensors;
}

// sums of both quantities over the block in one pass: two barriers instead of four
__device__ __forceinline__ float2 block_sum2(float a, float b, float* smem) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  a = wave_sum(a);
  b = wave_sum(b);
  __syncthreads();
  if (lane == 0) {
    smem[wid] = a;
    smem[4 + wid] = b;
  }
  __syncthreads();
  return make_float2((smem[0] + smem[1]) + (smem[2] + smem[3]),
                     (smem[4] + smem[5]) + (smem[6] + smem[7]));
}

__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8)))
lars_partial_kernel(
    const float* __restrict__ w, const float* __restrict__ g,
    const long long* __restrict__ chunks, int n_chunks, int n_tensors, long long total,
    const float* __restrict__ hyper, float2* __restrict__ partial) {
  __shared__ float red[8];
  const float gs = hyper[H_GSCALE];
  for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const Chunk ck = {chunks[3 * c], chunks[3 * c + 1], chunks[3 * c + 2]};
    float sw = 0.f, sg = 0.f;
    if (chunk_ok(ck, total, n_tensors)) {
      const float4* w4 = reinterpret_cast<const float4*>(w + ck.start);
      const float4* g4 = reinterpret_cast<const float4*>(g + ck.start);
      const int n4 = (int)(ck.len >> 2);
      // a chunk is at most LARS_CHUNK/4/256 vectors per thread: all loads issue before any use
      float4 a[LARS_VEC], b[LARS_VEC];
#pragma unroll
      for (int k = 0; k < LARS_VEC; ++k) {
        const int i = threadIdx.x + 256 * k;
        a[k] = b[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < n4) {
          a[k] = w4[i];
          b[k] = g4[i];
        }
      }
#pragma unroll
      for (int k = 0; k < LARS_VEC; ++k) {
        b[k].x *= gs; b[k].y *= gs; b[k].z *= gs; b[k].w *= gs;
        sw += (a[k].x * a[k].x + a[k].y * a[k].y) + (a[k].z * a[k].z + a[k].w * a[k].w);
        sg += (b[k].x * b[k].x + b[k].y * b[k].y) + (b[k].z * b[k].z + b[k].w * b[k].w);
      }
      const int t = (n4 << 2) + threadIdx.x;  // scalar tail (len % 4 elements)
      if (t < ck.len) {
        const float x = w[ck.start + t], y = g[ck.start + t] * gs;
        sw += x * x;
        sg += y * y;
      }
    }
    const float2 s = block_sum2(sw, sg, red);
    if (threadIdx.x == 0) partial[c] = s;
  }
}

// One wave per tensor: lane l sums that tensor's partials l, l+64, ... in order, then the
// butterfly adds the 64 lane sums -> tot[t] = (sum w^2, sum (gs*g)^2).
__global__ void __launch_bounds__(64) lars_totals_kernel(
    const long long* __restrict__ seg, int n_tensors, int n_chunks,
    const float2* __restrict__ partial, float2* __restrict__ tot) {
  const int lane = threadIdx.x;
  for (int t = blockIdx.x; t < n_tensors; t += gridDim.x) {
    long long first = seg[5 * t + 3], cnt = seg[5 * t + 4];
    if (first < 0 || cnt < 0 || first + cnt > n_chunks) cnt = 0;
    float sw = 0.f, sg = 0.f;
    for (long long i = lane; i < cnt; i += 64) {
      const float2 p = partial[first + i];
      sw += p.x;
      sg += p.y;
    }
    sw = wave_sum(sw);
    sg = wave_sum(sg);
    if (lane == 0) tot[t] = make_float2(sw, sg);
  }
}

template <bool NESTEROV>
__global__ void __launch_bounds__(256) lars_update_kernel(
    float* __restrict__ w, const float* __restrict__ g, float* __restrict__ buf,
    const long long* __restrict__ seg, const long long* __restrict__ chunks, int n_chunks,
    int n_tensors, long long total, const float* __restrict__ hyper,
    const float2* __restrict__ tot, float* __restrict__ stats, float* __restrict__ gnorm) {
  __shared__ float red[4];
  const float lr = hyper[H_LR], mu = hyper[H_MU], wd0 = hyper[H_WD], eta = hyper[H_ETA],
              eps = hyper[H_EPS], gs = hyper[H_GSCALE], maxn = hyper[H_MAXNORM];
  // the clipping factor: every block adds the per-tensor sums in the same order (thread i
  // takes tensors i, i+256, ...), so all of them get the same bits.  Only needed when
  // clipping is on; block 0 also computes it for the log.
  float c = 1.f;
  if (maxn > 0.f || blockIdx.x == 0) {
    float gg = 0.f;
    for (int t = threadIdx.x; t < n_tensors; t += 256) gg += tot[t].y;
    const float G = sqrtf(block_sum(gg, red));
    if (maxn > 0.f) c = fminf(1.f, maxn / (G + 1e-6f));
    if (blockIdx.x == 0 && threadIdx.x == 0) gnorm[0] = G;
  }
  const float cg = c * gs;
  for (int ci = blockIdx.x; ci < n_chunks; ci += gridDim.x) {
    const Chunk ck = {chunks[3 * ci], chunks[3 * ci + 1], chunks[3 * ci + 2]};
    if (!chunk_ok(ck, total, n_tensors)) continue;
    const float2 s = tot[ck.tensor];
    const bool adapted = seg[5 * ck.tensor + 2] != 0;
    const float wn = sqrtf(s.x), gn = c * sqrtf(s.y);
    float r = 1.f;
    if (adapted && wn > 0.f && gn > 0.f) r = eta * wn / (gn + wd0 * wn + eps);
    const float wd = adapted ? wd0 : 0.f;
    if (threadIdx.x == 0 && seg[5 * ck.tensor + 3] == ci) {  // the tensor's first chunk logs
      stats[3 * ck.tensor + 0] = wn;
      stats[3 * ck.tensor + 1] = gn;
      stats[3 * ck.tensor + 2] = r;
    }
    float4* w4 = reinterpret_cast<float4*>(w + ck.start);
    const float4* g4 = reinterpret_cast<const float4*>(g + ck.start);
    float4* b4 = reinterpret_cast<float4*>(buf + ck.start);
    const int n4 = (int)(ck.len >> 2);
    for (int i = threadIdx.x; i < n4; i += 256) {
      const float4 wv = w4[i], gv = g4[i], bv = b4[i];
      float wa[4] = {wv.x, wv.y, wv.z, wv.w};
      const float ga[4] = {gv.x, gv.y, gv.z, gv.w};
      float ba[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float d = r * (cg * ga[j] + wd * wa[j]);
        ba[j] = mu * ba[j] + d;
        wa[j] -= lr * (NESTEROV ? d + mu * ba[j] : ba[j]);
      }
      w4[i] = make_float4(wa[0], wa[1], wa[2], wa[3]);
      b4[i] = make_float4(ba[0], ba[1], ba[2], ba[3]);
    }
    const int t = (n4 << 2) + threadIdx.x;  // scalar tail
    if (t < ck.len) {
      const long long k = ck.start + t;
      const float wv = w[k];
      const float d = r * (cg * g[k] + wd * wv);
      const float b = mu * buf[k] + d;
      buf[k] = b;
      w[k] = wv - lr * (NESTEROV ? d + mu * b : b);
    }
  }
}

}  // namespace

int lars_chunk() { return LARS_CHUNK; }
int lars_hyper_count() { return H_COUNT; }

void lars_step(float* w, const float* g, float* buf, long long total, const long long* seg,
               int n_tensors, const long long* chunks, int n_chunks, const float* hyper,
               float* partial, float* tot, float* stats, float* gnorm, bool nesterov,
               int launches, hipStream_t st) {
  if (n_tensors <= 0 || n_chunks <= 0) return;
  const int grid = grid_for(n_chunks, 1, 4096);
  const float2* tot2 = reinterpret_cast<const float2*>(tot);
  if (launches & 1)
    lars_partial_kernel<<<grid, 256, 0, st>>>(w, g, chunks, n_chunks, n_tensors, total, hyper,
                                              reinterpret_cast<float2*>(partial));
  if (launches & 2)
    lars_totals_kernel<<<grid_for(n_tensors, 1, 1024), 64, 0, st>>>(
        seg, n_tensors, n_chunks, reinterpret_cast<const float2*>(partial),
        reinterpret_cast<float2*>(tot));
  if (!(launches & 4)) return;
  if (nesterov)
    lars_update_kernel<true><<<grid, 256, 0, st>>>(w, g, buf, seg, chunks, n_chunks, n_tensors,
                                                   total, hyper, tot2, stats, gnorm);
  else
    lars_update_kernel<false><<<grid, 256, 0, st>>>(w, g, buf, seg, chunks, n_chunks, n_tensors,
                                                    total, hyper, tot2, stats, gnorm);
}

}  // namespace dm
