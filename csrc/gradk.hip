// "topk": block-wise top-K gradient sparsification with error feedback
// (dmlab/parallel/compress.py).
//
// A bucket is one contiguous fp32 slice of n elements, cut into blocks of 2048 consecutive
// elements counted from the slice's start (the last one may hold m < 2048).  Per block, with
// K = keep (1..256):
//   e = g + r (r: the persistent residual; e = g without error feedback)
//   key(i) = bits(e[i]) & 0x7fffffff   (the magnitude as an integer: +-0 -> 0, Inf above every
//                                       finite value, NaN above Inf)
//   selected = the min(K, m) largest keys, equal keys in ascending in-block index
//   slot j (ascending index) = (e[i_j] bit for bit, i_j as uint16); unused slots (m < K only)
//   hold index 0xFFFF and +0.0;  r = +0.0 at the selected positions, e elsewhere.
// One rank's payload, nb = ceil(n/2048): nb*K fp32 values, nb*K uint16 indices, padding to 16 B.
// Decode-mean of [ws, payload]: acc = +0.0; rank 0..ws-1 in order: acc += v where the rank's
// block lists the element; out = c * acc, every element written.
//
// Encode: one 256-thread workgroup per block, thread t owns elements 8t..8t+7 (two 16-B loads
// of g and of r), so index order is thread order.  The K-th largest key comes from a radix
// select over the 31 key bits, most significant first, 8/8/8/7 bits: per pass one 256-bin LDS
// histogram (integer ds_add: order-independent) of the elements that still match the prefix,
// ONE barrier, then every wave scans the whole histogram on its own (4 bins per lane, a
// prefix sum over the lanes in six DPP adds) and finds the digit that holds the K-th element,
// so no second barrier broadcasts it.  The four passes have a histogram each, zeroed together
// up front, and the select stops at the first pass whose threshold bin is taken whole (its lower bits
// then decide nothing; on random data that is the second or third pass).
// A fifth histogram, of the 256 thread maxima's leading digit, runs first: the K-th largest
// thread maximum bounds the threshold from below, so the first pass counts only the elements
// at or above that digit (gradient-like data crowds a few exponent bins, and 2048 LDS adds
// on a handful of addresses serialise).
// Keys above the threshold are all taken, keys equal to it in index order until K is reached:
// one packed scan (count(key > T) << 16 | count(key == T), the same DPP wave prefix, cross-wave
// through 4 LDS words) gives a thread both its rank among the equals and its first output slot.
// No global atomics, g and r read once, r written once.
// Decode: one workgroup per block, a 2048-float LDS accumulator, one rank's K entries added by
// K threads (distinct indices: no conflicts), a barrier between ranks, 16-B stores of c * acc.
// Slices that are not 16-B aligned and the partial last block take scalar accesses with the
// same ownership.
#include "common.h"

namespace dm {

namespace {

constexpr int TK_BLOCK = 2048;
constexpr int TK_THREADS = 256;
constexpr int TK_PER = TK_BLOCK / TK_THREADS;  // 8 elements per thread
constexpr int TK_MAX_KEEP = 256;

// Inclusive prefix sum over the 64 lanes of a wave in six DPP adds (no LDS, no bpermute):
// row_shr 1, 2, 4, 8 scan each row of 16 lanes, row_bcast:15 adds a row's total to the next
// row (rows 1 and 3), row_bcast:31 adds the lower half's total to rows 2 and 3.  A lane whose
// source is out of range or masked adds `old` = 0.
__device__ __forceinline__ uint32_t wave_prefix_sum(uint32_t v) {
  int x = (int)v;
  x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, false);  // row_shr:1
  x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, false);  // row_shr:2
  x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, false);  // row_shr:4
  x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, false);  // row_shr:8
  x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xa, 0xf, false);  // row_bcast:15
  x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xc, 0xf, false);  // row_bcast:31
  return (uint32_t)x;
}

// Every lane of a wave calls this after the barrier that completes the 256-bin histogram h:
// the bin that holds the need-th largest element (1 <= need <= the histogram's total), the
// number of elements in the bins above it and the number in it (both <= 2048).  Lane l takes
// the 4 consecutive bins from 4*(63-l), so lane 0 has the highest and a prefix sum over the
// lanes counts from the top; the same result in every lane of every wave, no LDS exchange.
__device__ __forceinline__ void find_digit(const uint32_t* h256, int lane, uint32_t need,
                                           uint32_t& digit, uint32_t& above, uint32_t& inbin) {
  const int base = 4 * (63 - lane);
  const uint4 h = *reinterpret_cast<const uint4*>(h256 + base);
  const uint32_t own = h.x + h.y + h.z + h.w;
  const uint32_t a3 = wave_prefix_sum(own) - own;  // elements in bins above bin base+3
  const uint32_t a2 = a3 + h.w, a1 = a2 + h.z, a0 = a1 + h.y;
  // found: bin | above << 8 | inbin << 20
  uint32_t found = 0;
  bool mine = true;
  if (a3 < need && need <= a3 + h.w) found = (uint32_t)(base + 3) | a3 << 8 | h.w << 20;
  else if (a2 < need && need <= a2 + h.z) found = (uint32_t)(base + 2) | a2 << 8 | h.z << 20;
  else if (a1 < need && need <= a1 + h.y) found = (uint32_t)(base + 1) | a1 << 8 | h.y << 20;
  else if (a0 < need && need <= a0 + h.x) found = (uint32_t)base | a0 << 8 | h.x << 20;
  else mine = false;
  const unsigned long long hit = __ballot(mine);  // exactly one lane
  const int src = hit ? __ffsll((long long)hit) - 1 : 0;
  found = (uint32_t)__builtin_amdgcn_readlane((int)found, src);
  digit = found & 0xffu;
  above = (found >> 8) & 0xfffu;
  inbin = found >> 20;
}

// One block of m elements (FULL: m == 2048, every thread owns 8 and VEC may hold; otherwise the
// accesses are scalar and thread t owns cnt = clamp(m - 8t, 0, 8)).  hist is zero on entry
// (the caller's barrier) and is left to the caller to zero again.
template <bool HAS_R, bool VEC, bool FULL>
__device__ __forceinline__ void topk_encode_block(const float* __restrict__ g,
                                                  float* __restrict__ r, float* __restrict__ bv,
                                                  uint16_t* __restrict__ bi, int m, int keep,
                                                  uint32_t (*hist)[256], uint32_t* wtot) {
  const int t = threadIdx.x;
  const int lane = t & 63;
  const int wave = t >> 6;
  const int kk = keep < m ? keep : m;
  const int left = m - t * TK_PER;
  const int cnt = FULL ? TK_PER : (left >= TK_PER ? TK_PER : (left > 0 ? left : 0));
  g += t * TK_PER;
  if (HAS_R) r += t * TK_PER;
  float e[TK_PER];
#pragma unroll
  for (int j = 0; j < TK_PER; ++j) e[j] = 0.f;
  if (FULL && VEC) {
    const float4 a = *reinterpret_cast<const float4*>(g);
    const float4 b = *reinterpret_cast<const float4*>(g + 4);
    e[0] = a.x; e[1] = a.y; e[2] = a.z; e[3] = a.w;
    e[4] = b.x; e[5] = b.y; e[6] = b.z; e[7] = b.w;
    if (HAS_R) {
      const float4 c = *reinterpret_cast<const float4*>(r);
      const float4 d = *reinterpret_cast<const float4*>(r + 4);
      e[0] += c.x; e[1] += c.y; e[2] += c.z; e[3] += c.w;
      e[4] += d.x; e[5] += d.y; e[6] += d.z; e[7] += d.w;
    }
  } else {
#pragma unroll
    for (int j = 0; j < TK_PER; ++j)
      if (j < cnt) e[j] = HAS_R ? g[j] + r[j] : g[j];
  }
  uint32_t key[TK_PER];
#pragma unroll
  for (int j = 0; j < TK_PER; ++j) key[j] = __float_as_uint(e[j]) & 0x7fffffffu;

  // A lower bound first, from 256 LDS adds instead of 2048: with at least kk non-empty
  // threads, the kk-th largest THREAD maximum has kk elements at or above it, so the
  // threshold is no smaller and an element below that maximum's leading digit is never
  // selected.  Gradient-like data puts most elements into a few exponent bins; this keeps
  // them out of the first pass, whose adds would otherwise serialise on those bins.
  uint32_t floor_key = 0;
  if (FULL || (m + TK_PER - 1) / TK_PER >= kk) {  // block-uniform
    if (cnt > 0) {
      uint32_t mx = 0;
#pragma unroll
      for (int j = 0; j < TK_PER; ++j)
        if (j < cnt) mx = key[j] > mx ? key[j] : mx;
      atomicAdd(&hist[4][mx >> 23], 1u);
    }
    __syncthreads();
    uint32_t d, ab, in;
    find_digit(hist[4], lane, (uint32_t)kk, d, ab, in);
    floor_key = d << 23;
  }

  // radix select: `prefix` holds the threshold's bits above `shift`, `need` how many of the
  // elements that match it are still to be taken (1 <= need <= their number).  It ends with
  //   take_from: every key >= it is taken;  eq_key: the `need` first keys equal to it are too.
  // When a pass finds that ALL elements of the threshold's bin are taken, the lower bits
  // decide nothing: the select stops there (block-uniform: every wave computes the same).
  uint32_t prefix = 0, take_from = 0, eq_key = 0xffffffffu;  // no key equals 0xffffffff
  int need = kk;
  bool open = true;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int shift = p == 0 ? 23 : (p == 1 ? 15 : (p == 2 ? 7 : 0));
    const int up = p == 0 ? 31 : (p == 1 ? 23 : (p == 2 ? 15 : 7));  // bits >= up are fixed
    const uint32_t dmask = p == 3 ? 0x7fu : 0xffu;
    if (open) {
#pragma unroll
      for (int j = 0; j < TK_PER; ++j) {
        if (j < cnt && (p == 0 ? key[j] >= floor_key : (key[j] >> up) == prefix))
          atomicAdd(&hist[p][(key[j] >> shift) & dmask], 1u);
      }
      __syncthreads();
      uint32_t digit, above, inbin;
      find_digit(hist[p], lane, (uint32_t)need, digit, above, inbin);
      prefix = (prefix << (p == 3 ? 7 : 8)) | (digit & dmask);
      need -= (int)above;
      if ((uint32_t)need == inbin) {  // the whole bin is taken
        take_from = prefix << shift;
        need = 0;
        open = false;
      } else if (p == 3) {  // prefix is the K-th largest key; `need` of its equals are taken
        take_from = prefix + 1;
        eq_key = prefix;
      }
    }
  }

  // one packed scan: (elements taken for sure) << 16 | (elements equal to eq_key)
  uint32_t mine = 0;
#pragma unroll
  for (int j = 0; j < TK_PER; ++j)
    if (j < cnt) mine += key[j] >= take_from ? 0x10000u : (key[j] == eq_key ? 1u : 0u);
  const uint32_t scan = wave_prefix_sum(mine);
  if (lane == 63) wtot[wave] = scan;
  __syncthreads();
  uint32_t before = scan - mine;
  for (int w = 0; w < wave; ++w) before += wtot[w];
  int eq_rank = (int)(before & 0xffffu);  // equals in front of this thread
  int slot = (int)(before >> 16) + (eq_rank < need ? eq_rank : need);
#pragma unroll
  for (int j = 0; j < TK_PER; ++j) {
    bool take = false;
    if (j < cnt) {
      if (key[j] >= take_from) take = true;
      else if (key[j] == eq_key) take = eq_rank++ < need;
    }
    // 0 <= slot < kk by construction; the test keeps the store in bounds whatever happens
    if (take && (unsigned)slot < (unsigned)keep) {
      bv[slot] = e[j];
      bi[slot] = (uint16_t)(t * TK_PER + j);
      ++slot;
      e[j] = 0.f;
    }
  }
  if (!FULL && t >= kk && t < keep) {  // m < K: the unused slots
    bv[t] = 0.f;
    bi[t] = (uint16_t)0xFFFFu;
  }
  if (HAS_R) {
    if (FULL && VEC) {
      *reinterpret_cast<float4*>(r) = make_float4(e[0], e[1], e[2], e[3]);
      *reinterpret_cast<float4*>(r + 4) = make_float4(e[4], e[5], e[6], e[7]);
    } else {
#pragma unroll
      for (int j = 0; j < TK_PER; ++j)
        if (j < cnt) r[j] = e[j];
    }
  }
}

template <bool HAS_R, bool VEC>
__global__ void __launch_bounds__(TK_THREADS) topk_encode_kernel(const float* __restrict__ g,
                                                                 float* __restrict__ r,
                                                                 float* __restrict__ vals,
                                                                 uint16_t* __restrict__ idxs,
                                                                 long long n, long long nblk,
                                                                 int keep) {
  __shared__ __attribute__((aligned(16))) uint32_t hist[5][256];  // [4]: the thread maxima
  __shared__ uint32_t wtot[4];
  const int t = threadIdx.x;
  for (long long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    // every read of the previous block's histograms lies before its last barrier
#pragma unroll
    for (int p = 0; p < 5; ++p) hist[p][t] = 0;
    __syncthreads();
    const long long b0 = blk * TK_BLOCK;
    const long long rest = n - b0;  // >= 1
    float* bv = vals + blk * keep;
    uint16_t* bi = idxs + blk * keep;
    float* rb = HAS_R ? r + b0 : nullptr;
    if (rest >= TK_BLOCK)
      topk_encode_block<HAS_R, VEC, true>(g + b0, rb, bv, bi, TK_BLOCK, keep, hist, wtot);
    else
      topk_encode_block<HAS_R, false, false>(g + b0, rb, bv, bi, (int)rest, keep, hist, wtot);
  }
}

template <bool VEC>
__global__ void __launch_bounds__(TK_THREADS) topk_decode_mean_kernel(
    const uint8_t* __restrict__ gathered, long long row_bytes, int ws, float* __restrict__ out,
    long long n, long long nblk, int keep, float c) {
  __shared__ __attribute__((aligned(16))) float acc[TK_BLOCK];
  const int t = threadIdx.x;
  const long long idx_off = 4 * nblk * keep;
  for (long long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    // the previous block's reads of acc lie before its last barrier below
#pragma unroll
    for (int j = 0; j < TK_PER; ++j) acc[t + j * TK_THREADS] = 0.f;
    __syncthreads();
    // rank rk+1's entry is loaded before rank rk's is added: one global latency, not ws
    const long long s = blk * keep + (t < keep ? t : 0);
    uint32_t i = reinterpret_cast<const uint16_t*>(gathered + idx_off)[s];
    float v = reinterpret_cast<const float*>(gathered)[s];
    for (int rk = 0; rk < ws; ++rk) {
      uint32_t i_next = 0;
      float v_next = 0.f;
      if (rk + 1 < ws) {
        const uint8_t* row = gathered + (long long)(rk + 1) * row_bytes;
        i_next = reinterpret_cast<const uint16_t*>(row + idx_off)[s];
        v_next = reinterpret_cast<const float*>(row)[s];
      }
      if (t < keep && i < (uint32_t)TK_BLOCK)  // 0xFFFF: an unused slot
        acc[i] = acc[i] + v;
      __syncthreads();
      i = i_next;
      v = v_next;
    }
    const long long i0 = blk * TK_BLOCK + t * TK_PER;
    const long long left = n - i0;
    const int cnt = left >= TK_PER ? TK_PER : (left > 0 ? (int)left : 0);
    const float4 a = *reinterpret_cast<const float4*>(&acc[t * TK_PER]);
    const float4 b = *reinterpret_cast<const float4*>(&acc[t * TK_PER + 4]);
    const float o[TK_PER] = {a.x * c, a.y * c, a.z * c, a.w * c, b.x * c, b.y * c, b.z * c, b.w * c};
    if (VEC && cnt == TK_PER) {
      *reinterpret_cast<float4*>(out + i0) = make_float4(o[0], o[1], o[2], o[3]);
      *reinterpret_cast<float4*>(out + i0 + 4) = make_float4(o[4], o[5], o[6], o[7]);
    } else {
#pragma unroll
      for (int j = 0; j < TK_PER; ++j)
        if (j < cnt) out[i0 + j] = o[j];
    }
    __syncthreads();  // acc is read: the next block may zero it
  }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

inline int capped(int grid, int max_blocks) {
  return max_blocks > 0 && grid > max_blocks ? max_blocks : grid;
}

}  // namespace

int topk_block() { return TK_BLOCK; }
int topk_max_keep() { return TK_MAX_KEEP; }

long long topk_payload_bytes(long long n, int keep) {
  const long long nblk = (n + TK_BLOCK - 1) / TK_BLOCK;
  return (6 * nblk * keep + 15) / 16 * 16;
}

void topk_encode(const float* g, float* r, uint8_t* payload, long long n, int keep,
                 int max_blocks, hipStream_t st) {
  if (n <= 0 || keep < 1 || keep > TK_MAX_KEEP) return;
  const long long nblk = (n + TK_BLOCK - 1) / TK_BLOCK;
  float* vals = reinterpret_cast<float*>(payload);
  uint16_t* idxs = reinterpret_cast<uint16_t*>(payload + 4 * nblk * keep);
  // one workgroup per block, all of them launched: the hardware hands a finished workgroup's
  // slot to the next block, which balances the CUs better than a grid-stride loop over fewer
  const int grid = capped(grid_for(nblk, 1, 1 << 30), max_blocks);
  const bool vec = aligned16(g) && (r == nullptr || aligned16(r));
  if (r) {
    if (vec)
      topk_encode_kernel<true, true><<<grid, TK_THREADS, 0, st>>>(g, r, vals, idxs, n, nblk, keep);
    else
      topk_encode_kernel<true, false><<<grid, TK_THREADS, 0, st>>>(g, r, vals, idxs, n, nblk, keep);
  } else {
    if (vec)
      topk_encode_kernel<false, true><<<grid, TK_THREADS, 0, st>>>(g, r, vals, idxs, n, nblk, keep);
    else
      topk_encode_kernel<false, false><<<grid, TK_THREADS, 0, st>>>(g, r, vals, idxs, n, nblk,
                                                                    keep);
  }
}

void topk_decode_mean(const uint8_t* gathered, long long row_bytes, int ws, float* out,
                      long long n, int keep, float scale, int max_blocks, hipStream_t st) {
  if (n <= 0 || keep < 1 || keep > TK_MAX_KEEP) return;
  const long long nblk = (n + TK_BLOCK - 1) / TK_BLOCK;
  const int grid = capped(grid_for(nblk, 1, 1 << 30), max_blocks);
  if (aligned16(out))
    topk_decode_mean_kernel<true><<<grid, TK_THREADS, 0, st>>>(gathered, row_bytes, ws, out, n,
                                                               nblk, keep, scale);
  else
    topk_decode_mean_kernel<false><<<grid, TK_THREADS, 0, st>>>(gathered, row_bytes, ws, out, n,
                                                                nblk, keep, scale);
}

}  // namespace dm
