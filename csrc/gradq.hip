// "q8": block-wise int8 gradient quantisation with error feedback (dmlab/parallel/compress.py).
//
// A bucket is one contiguous fp32 slice of n elements, cut into blocks of 256 consecutive
// elements counted from the slice's start (the last one may be partial).  Per block:
//   e = g + r (r: the persistent residual; e = g without error feedback)
//   a = max |e| ; s = a / 127 (IEEE division, round to nearest)
//   s == 0        : codes 0, r = e
//   a not finite  : s = NaN, codes 0, r = 0   (the block decodes to NaN on every rank)
//   otherwise     : q = clamp(rint(e / s), -127, 127) (IEEE division, ties to even),
//                   r = e - q*s (product rounded, then the difference: no FMA)
// One rank's payload: ceil(n/256) fp32 scales, then n int8 codes, padded to 16 bytes.
// Decode-mean of [ws, payload]: out = c * sum_{rank 0..ws-1} q*s, fp32, in rank order
// (product rounded, then added: no FMA), so every rank computes the same bits.
//
// Both kernels stream: no LDS, no atomics.  Encode: one wave per block, 4 elements per lane
// (16-B loads of g and r, a 16-B store of r, the four codes packed into one 32-bit store),
// the block maximum by __shfl_xor over the wave.  Decode: 4 consecutive elements per lane, one
// packed word and one scale per rank, one 16-B store.  Slices that are not 16-B aligned (a view
// into the flat buffer starts at any 4-B offset) and the partial last block take scalar
// accesses with the same lane ownership.
#include "common.h"

// the torch mirror of these formulas rounds every product before it is added or subtracted
#pragma clang fp contract(off)

namespace dm {

namespace {

constexpr int Q8_BLOCK = 256;

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t w = (uint32_t)__shfl_xor((int)v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}

template <bool HAS_R, bool VEC>
__global__ void __launch_bounds__(256) q8_encode_kernel(const float* __restrict__ g,
                                                        float* __restrict__ r,
                                                        float* __restrict__ scales,
                                                        uint32_t* __restrict__ codes,
                                                        long long n, long long nblk) {
  const int lane = threadIdx.x & 63;
  const long long nwaves = (long long)gridDim.x * 4;
  // blk is wave-uniform: all 64 lanes run every iteration, so the shuffles see the whole wave
  for (long long blk = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); blk < nblk;
       blk += nwaves) {
    const long long i0 = blk * Q8_BLOCK + lane * 4;
    const long long left = n - i0;
    const int cnt = left >= 4 ? 4 : (left > 0 ? (int)left : 0);
    float e[4] = {0.f, 0.f, 0.f, 0.f};  // lanes past the end contribute 0 to the maximum
    if (VEC && cnt == 4) {
      const float4 gv = *reinterpret_cast<const float4*>(g + i0);
      e[0] = gv.x; e[1] = gv.y; e[2] = gv.z; e[3] = gv.w;
      if (HAS_R) {
        const float4 rv = *reinterpret_cast<const float4*>(r + i0);
        e[0] += rv.x; e[1] += rv.y; e[2] += rv.z; e[3] += rv.w;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < cnt) e[j] = HAS_R ? g[i0 + j] + r[i0 + j] : g[i0 + j];
    }
    // |e| as an integer: ordered like the floats, and a NaN (above the infinity pattern) wins
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t b = __float_as_uint(e[j]) & 0x7fffffffu;
      m = b > m ? b : m;
    }
    m = wave_max_u32(m);
    const bool finite = m < 0x7f800000u;
    const float s = finite ? __uint_as_float(m) / 127.f : __uint_as_float(0x7fc00000u);
    float res[4];
    uint32_t word = 0;
    if (!finite) {
#pragma unroll
      for (int j = 0; j < 4; ++j) res[j] = 0.f;
    } else if (s == 0.f) {
#pragma unroll
      for (int j = 0; j < 4; ++j) res[j] = e[j];
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float q = fminf(fmaxf(rintf(e[j] / s), -127.f), 127.f);
        res[j] = e[j] - q * s;
        word |= ((uint32_t)(int)q & 0xffu) << (8 * j);
      }
    }
    if (cnt == 4) {
      codes[blk * (Q8_BLOCK / 4) + lane] = word;
    } else {
      uint8_t* cb = reinterpret_cast<uint8_t*>(codes) + i0;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < cnt) cb[j] = (uint8_t)(word >> (8 * j));
    }
    if (HAS_R) {
      if (VEC && cnt == 4) {
        *reinterpret_cast<float4*>(r + i0) = make_float4(res[0], res[1], res[2], res[3]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j < cnt) r[i0 + j] = res[j];
      }
    }
    if (lane == 0) scales[blk] = s;
  }
}

template <bool VEC>
__global__ void __launch_bounds__(256) q8_decode_mean_kernel(const uint8_t* __restrict__ gathered,
                                                             long long row_bytes, int ws,
                                                             float* __restrict__ out, long long n,
                                                             long long nblk, float c) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long nquad = (n + 3) >> 2;
  for (long long qd = (long long)blockIdx.x * blockDim.x + threadIdx.x; qd < nquad;
       qd += stride) {
    const long long i0 = qd * 4;
    const long long blk = i0 / Q8_BLOCK;  // 4 divides 256: a lane's elements share one block
    const long long left = n - i0;
    const int cnt = left >= 4 ? 4 : (int)left;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int rk = 0; rk < ws; ++rk) {
      const uint8_t* row = gathered + (long long)rk * row_bytes;
      const float s = reinterpret_cast<const float*>(row)[blk];
      // the codes are padded to 16 bytes, so the last (partial) word lies inside the row
      const uint32_t word = reinterpret_cast<const uint32_t*>(row + 4 * nblk)[qd];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] += (float)(int8_t)(word >> (8 * j)) * s;
    }
    if (VEC && cnt == 4) {
      *reinterpret_cast<float4*>(out + i0) =
          make_float4(acc[0] * c, acc[1] * c, acc[2] * c, acc[3] * c);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < cnt) out[i0 + j] = acc[j] * c;
    }
  }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

inline int capped(int grid, int max_blocks) {
  return max_blocks > 0 && grid > max_blocks ? max_blocks : grid;
}

}  // namespace

long long q8_payload_bytes(long long n) {
  const long long nblk = (n + Q8_BLOCK - 1) / Q8_BLOCK;
  return (4 * nblk + n + 15) / 16 * 16;
}

void q8_encode(const float* g, float* r, uint8_t* payload, long long n, int max_blocks,
               hipStream_t st) {
  if (n <= 0) return;
  const long long nblk = (n + Q8_BLOCK - 1) / Q8_BLOCK;
  float* scales = reinterpret_cast<float*>(payload);
  uint32_t* codes = reinterpret_cast<uint32_t*>(payload + 4 * nblk);
  const int grid = capped(grid_for(nblk, 4), max_blocks);  // one wave per block, 4 per workgroup
  const bool vec = aligned16(g) && (r == nullptr || aligned16(r));
  if (r) {
    if (vec) q8_encode_kernel<true, true><<<grid, 256, 0, st>>>(g, r, scales, codes, n, nblk);
    else q8_encode_kernel<true, false><<<grid, 256, 0, st>>>(g, r, scales, codes, n, nblk);
  } else {
    if (vec) q8_encode_kernel<false, true><<<grid, 256, 0, st>>>(g, r, scales, codes, n, nblk);
    else q8_encode_kernel<false, false><<<grid, 256, 0, st>>>(g, r, scales, codes, n, nblk);
  }
}

void q8_decode_mean(const uint8_t* gathered, long long row_bytes, int ws, float* out,
                    long long n, float scale, int max_blocks, hipStream_t st) {
  if (n <= 0) return;
  const long long nblk = (n + Q8_BLOCK - 1) / Q8_BLOCK;
  const int grid = capped(grid_for((n + 3) / 4, 256), max_blocks);
  if (aligned16(out))
    q8_decode_mean_kernel<true><<<grid, 256, 0, st>>>(gathered, row_bytes, ws, out, n, nblk,
                                                      scale);
  else
    q8_decode_mean_kernel<false><<<grid, 256, 0, st>>>(gathered, row_bytes, ws, out, n, nblk,
                                                       scale);
}

}  // namespace dm
