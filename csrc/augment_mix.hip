// On-device mixup / CutMix fused into the augmentation gather (docs/KERNELS.md,
// "Augmentation"): one launch writes the batch once, from two dataset rows per sample where the
// sample is mixed.
//
// images, idx, params, out as in augment.hip; mix int32 [B,4] = partner, L, xbox, ybox (box =
// lo | hi << 16, inclusive, in OUTPUT pixel coordinates; empty is lo > hi).  Per output pixel
// (oy, ox) of sample b, with A = what augment_kernel computes for (idx[b], params[b]) and P the
// same for (idx[partner], params[partner]):
//   inside the box:                 out = P, as augment_kernel stores it
//   outside, L == 65536:            out = A, as augment_kernel stores it; the partner is not read
//   otherwise, u8:                  (L*a + (65536-L)*p + 32768) >> 16 on the two rounded values
//   otherwise, fp32 / bf16:         ((float)L*a' + (float)(65536-L)*p') * 2^-16 on the unrounded
//                                   fp32 blend results, each operation rounded on its own, one
//                                   round-to-nearest-even into bf16 at the end
// L is clamped to [0, 65536].  A partner outside [0,B) is never used as an index: the row is
// written unmixed.  A partner whose idx is outside the dataset contributes zeros (augment.hip's
// rule).  The box only enters comparisons with ox, oy, never an address.
//
// The thread layout, the 16-byte non-temporal stores and the scalar tail are augment_kernel's.
// A pixel first evaluates ONE sample, the partner inside the box and the sample itself
// elsewhere: the choice is a select over the per-sample state, not a branch, so unmixed and
// CutMix pixels issue exactly augment_kernel's four loads.  Only a pixel that blends (L < 65536
// outside the box) then evaluates the partner too, behind a branch that no lane of a wave takes
// when its samples are unmixed or CutMix.
#include "augment_common.h"

namespace dm {

// what a pixel needs of one sample: the x axis, where the sample starts, and the y taps of the
// current output row (the y axis itself is kept beside it: only a new row uses it)
struct AugSample {
  AugAxis ax;
  long long src;
  bool rowok, flip;
  int y0, y1, fy;
  bool vy0, vy1;

  __device__ __forceinline__ void load(const long long* __restrict__ idx,
                                       const int* __restrict__ params, int b, long long N, int H,
                                       int W, int C, AugAxis& ay) {
    // the sample's 32-byte parameter row: two 16-byte loads
    const aug_i32x4 pa = *reinterpret_cast<const aug_i32x4*>(params + (long long)b * 8);
    const aug_i32x4 pb = *reinterpret_cast<const aug_i32x4*>(params + (long long)b * 8 + 4);
    const long long n = idx[b];
    rowok = n >= 0 && n < N;
    src = (rowok ? n : 0) * ((long long)H * W * C);
    flip = pb[0] & 1;
    const int zero = (pb[0] >> 1) & 1;
    const uint32_t xb = (uint32_t)pb[1], yb = (uint32_t)pb[2];
    // the box clamped to the image (lo <= hi <= size-1 after this, whatever was passed)
    ax.hi = min((int)(xb >> 16), W - 1);
    ax.lo = min((int)(xb & 0xffffu), ax.hi);
    ay.hi = min((int)(yb >> 16), H - 1);
    ay.lo = min((int)(yb & 0xffffu), ay.hi);
    ax.origin = pa[0]; ay.origin = pa[1];
    ax.step = pa[2]; ay.step = pa[3];
    ax.zero = zero; ay.zero = zero;
  }
  __device__ __forceinline__ void row(const AugAxis& ay, int oy) {
    ay.taps(oy, y0, y1, vy0, vy1, fy);
  }
};

__device__ __forceinline__ AugSample aug_select(bool second, const AugSample& a,
                                                const AugSample& p) {
  AugSample s;
  s.ax.origin = second ? p.ax.origin : a.ax.origin;
  s.ax.step = second ? p.ax.step : a.ax.step;
  s.ax.lo = second ? p.ax.lo : a.ax.lo;
  s.ax.hi = second ? p.ax.hi : a.ax.hi;
  s.ax.zero = second ? p.ax.zero : a.ax.zero;
  s.src = second ? p.src : a.src;
  s.rowok = second ? p.rowok : a.rowok;
  s.flip = second ? p.flip : a.flip;
  s.y0 = second ? p.y0 : a.y0;
  s.y1 = second ? p.y1 : a.y1;
  s.fy = second ? p.fy : a.fy;
  s.vy0 = second ? p.vy0 : a.vy0;
  s.vy1 = second ? p.vy1 : a.vy1;
  return s;
}

// the rounded u8 value, or the unrounded fp32 blend, of a sample's four taps
__device__ __forceinline__ int aug_mix_value(int p00, int p01, int p10, int p11, int w00, int w01,
                                             int w10, int w11) {
  return (w00 * p00 + w01 * p01 + w10 * p10 + w11 * p11 + 32768) >> 16;
}
__device__ __forceinline__ float aug_mix_value(float p00, float p01, float p10, float p11,
                                               int w00, int w01, int w10, int w11) {
  return aug_blend_f(p00, p01, p10, p11, w00, w01, w10, w11);
}

// One sample at output column ox of its current row: what augment_kernel computes, before the
// conversion to the storage type (0 for a row outside the dataset).
template <typename T, int C, bool PACK>
__device__ __forceinline__ void aug_sample_pixel(const T* __restrict__ images, long long total,
                                                 const AugSample& s, int ox, int OW, int W,
                                                 typename AugPix<T>::acc_t (&v)[C]) {
  typedef typename AugPix<T>::acc_t acc_t;
  int x0, x1, fx;
  bool vx0, vx1;
  s.ax.taps(s.flip ? OW - 1 - ox : ox, x0, x1, vx0, vx1, fx);
  const int w00 = (256 - s.fy) * (256 - fx), w01 = (256 - s.fy) * fx;
  const int w10 = s.fy * (256 - fx), w11 = s.fy * fx;
  const long long r0 = s.src + (long long)s.y0 * W * C, r1 = s.src + (long long)s.y1 * W * C;
  // the tap positions are clamped into the sample (row 0 for a bad idx), so every load is in
  // range; loading first and selecting afterwards keeps the loads independent
  acc_t p00[C], p01[C], p10[C], p11[C];
  aug_tap<T, C, PACK>(images, r0 + x0 * C, total, p00);
  aug_tap<T, C, PACK>(images, r0 + x1 * C, total, p01);
  aug_tap<T, C, PACK>(images, r1 + x0 * C, total, p10);
  aug_tap<T, C, PACK>(images, r1 + x1 * C, total, p11);
  const bool v00 = s.vy0 && vx0, v01 = s.vy0 && vx1, v10 = s.vy1 && vx0, v11 = s.vy1 && vx1;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const acc_t a00 = v00 ? p00[c] : (acc_t)0, a01 = v01 ? p01[c] : (acc_t)0;
    const acc_t a10 = v10 ? p10[c] : (acc_t)0, a11 = v11 ? p11[c] : (acc_t)0;
    v[c] = s.rowok ? aug_mix_value(a00, a01, a10, a11, w00, w01, w10, w11) : (acc_t)0;
  }
}

__device__ __forceinline__ int aug_lerp(int a, int p, int L) {
  return (L * a + (65536 - L) * p + 32768) >> 16;  // < 2^24 + 2^15: no overflow
}
__device__ __forceinline__ float aug_lerp(float a, float p, int L) {
#pragma clang fp contract(off)
  const float x = (float)L * a;
  const float y = (float)(65536 - L) * p;
  return (x + y) * 0x1p-16f;
}

__device__ __forceinline__ uint8_t aug_store(int v, uint8_t) { return (uint8_t)v; }
__device__ __forceinline__ float aug_store(float v, float) { return v; }
__device__ __forceinline__ bf16_t aug_store(float v, bf16_t) { return f2bf(v); }

template <typename T, int C, bool PACK>
__global__ void __launch_bounds__(256) augment_mix_kernel(
    const T* __restrict__ images, const long long* __restrict__ idx,
    const int* __restrict__ params, const int* __restrict__ mix, T* __restrict__ out, long long N,
    int H, int W, int B, int OH, int OW, long long npix, int vec) {
  typedef typename AugPix<T>::acc_t acc_t;
  constexpr int PPT = 16 / (int)sizeof(T);  // pixels per thread = C 16-byte chunks
  const long long p0 = ((long long)blockIdx.x * 256 + threadIdx.x) * PPT;
  if (p0 >= npix) return;
  const long long plane = (long long)OH * OW;
  int b = (int)(p0 / plane);
  const int r = (int)(p0 - (long long)b * plane);
  int oy = r / OW;
  int ox = r - oy * OW;

  alignas(16) T vals[PPT * C];
  AugSample sa, sp;
  AugAxis aya, ayp;
  const long long total = N * H * W * C;
  int L = 65536;
  int bx0 = 1, bx1 = 0, by0 = 1, by1 = 0;  // the paste box, inclusive
  bool inrow = false;                       // oy inside the box
  bool newb = true, newy = true;
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    if (p0 + k < npix) {
      if (newb) {
        sa.load(idx, params, b, N, H, W, C, aya);
        const aug_i32x4 m = *reinterpret_cast<const aug_i32x4*>(mix + (long long)b * 4);
        const bool pok = m[0] >= 0 && m[0] < B;
        // a partner outside the batch: the sample itself, unmixed
        sp.load(idx, params, pok ? m[0] : b, N, H, W, C, ayp);
        L = pok ? min(max(m[1], 0), 65536) : 65536;
        const uint32_t xb = (uint32_t)m[2], yb = (uint32_t)m[3];
        bx0 = pok ? (int)(xb & 0xffffu) : 1;
        bx1 = pok ? (int)(xb >> 16) : 0;
        by0 = (int)(yb & 0xffffu);
        by1 = (int)(yb >> 16);
        newb = false;
        newy = true;
      }
      if (newy) {
        sa.row(aya, oy);
        sp.row(ayp, oy);
        inrow = oy >= by0 && oy <= by1;
        newy = false;
      }
      const bool inbox = inrow && ox >= bx0 && ox <= bx1;
      acc_t v[C];
      aug_sample_pixel<T, C, PACK>(images, total, aug_select(inbox, sa, sp), ox, OW, W, v);
      if (!inbox && L < 65536) {
        acc_t q[C];
        aug_sample_pixel<T, C, PACK>(images, total, sp, ox, OW, W, q);
#pragma unroll
        for (int c = 0; c < C; ++c) v[c] = aug_lerp(v[c], q[c], L);
      }
#pragma unroll
      for (int c = 0; c < C; ++c) vals[k * C + c] = aug_store(v[c], T());
      if (++ox == OW) {
        ox = 0;
        newy = true;
        if (++oy == OH) {
          oy = 0;
          ++b;
          newb = true;
        }
      }
    } else {
#pragma unroll
      for (int c = 0; c < C; ++c) vals[k * C + c] = (T)0;
    }
  }

  T* dst = out + p0 * C;
  if (vec && p0 + PPT <= npix) {
    const aug_u32x4* v = reinterpret_cast<const aug_u32x4*>(vals);
#pragma unroll
    for (int c = 0; c < C; ++c)
      __builtin_nontemporal_store(v[c], reinterpret_cast<aug_u32x4*>(dst) + c);
  } else {
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
      if (p0 + k < npix) {
#pragma unroll
        for (int c = 0; c < C; ++c) dst[k * C + c] = vals[k * C + c];
      }
    }
  }
}

template <typename T>
static void augment_mix_launch(const void* images, const long long* idx, const int* params,
                               const int* mix, void* out, long long N, int H, int W, int C, int B,
                               int OH, int OW, hipStream_t st) {
  constexpr int PPT = 16 / (int)sizeof(T);
  const long long npix = (long long)B * OH * OW;
  const long long threads = (npix + PPT - 1) / PPT;
  const unsigned grid = (unsigned)((threads + 255) / 256);
  const int vec = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  const T* im = (const T*)images;
  T* o = (T*)out;
  if (C == 1)
    augment_mix_kernel<T, 1, false><<<grid, 256, 0, st>>>(im, idx, params, mix, o, N, H, W, B, OH,
                                                          OW, npix, vec);
  else if (N * H * W * 3 >= 4)
    augment_mix_kernel<T, 3, true><<<grid, 256, 0, st>>>(im, idx, params, mix, o, N, H, W, B, OH,
                                                         OW, npix, vec);
  else  // a single 1 x 1 image: no room for a 4-element load
    augment_mix_kernel<T, 3, false><<<grid, 256, 0, st>>>(im, idx, params, mix, o, N, H, W, B, OH,
                                                          OW, npix, vec);
}

// dtype: 0 = u8, 1 = fp32, 2 = bf16
void augment_mix_apply(const void* images, const long long* idx, const int* params, const int* mix,
                       void* out, long long N, int H, int W, int C, int B, int OH, int OW,
                       int dtype, hipStream_t st) {
  if (dtype == 0)
    augment_mix_launch<uint8_t>(images, idx, params, mix, out, N, H, W, C, B, OH, OW, st);
  else if (dtype == 1)
    augment_mix_launch<float>(images, idx, params, mix, out, N, H, W, C, B, OH, OW, st);
  else
    augment_mix_launch<bf16_t>(images, idx, params, mix, out, N, H, W, C, B, OH, OW, st);
}

}  // namespace dm
