// What the augmentation kernels share (augment.hip, augment_mix.hip): the tap loads, the
// per-axis tap positions and the four-tap blend.  The arithmetic is written down in
// augment.hip's header and in docs/KERNELS.md, "Augmentation".
#pragma once
#include "common.h"

namespace dm {

typedef uint32_t aug_u32x4 __attribute__((ext_vector_type(4)));
typedef int aug_i32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t aug_u32_unaligned __attribute__((aligned(1)));

template <typename T> struct AugPix;
template <> struct AugPix<uint8_t> {
  typedef int acc_t;
  typedef uint8_t vec4 __attribute__((ext_vector_type(4), aligned(1)));
  static __device__ __forceinline__ int cvt(uint8_t v) { return v; }
};
template <> struct AugPix<float> {
  typedef float acc_t;
  typedef float vec4 __attribute__((ext_vector_type(4), aligned(4)));
  static __device__ __forceinline__ float cvt(float v) { return v; }
};
template <> struct AugPix<bf16_t> {
  typedef float acc_t;
  typedef bf16_t vec4 __attribute__((ext_vector_type(4), aligned(2)));
  static __device__ __forceinline__ float cvt(bf16_t v) { return bf2f(v); }
};

// The C channels of the pixel at element offset `off` of the tensor (`total` elements).
// PACK (C = 3, total >= 4): one 4-element load; it starts at the pixel unless that would pass
// the end of the tensor, then one element earlier.
template <typename T, int C, bool PACK>
__device__ __forceinline__ void aug_tap(const T* __restrict__ base, long long off,
                                        long long total, typename AugPix<T>::acc_t (&p)[C]) {
  if constexpr (PACK) {
    static_assert(C == 3, "packed taps are 3-channel");
    const bool back = off + 4 > total;
    if constexpr (sizeof(T) == 1) {
      // as one 32-bit word (a byte vector is split back into byte loads by the compiler)
      uint32_t v = *reinterpret_cast<const aug_u32_unaligned*>(base + (off - (back ? 1 : 0)));
      v = back ? v >> 8 : v;
      p[0] = v & 255u;
      p[1] = (v >> 8) & 255u;
      p[2] = (v >> 16) & 255u;
    } else {
      const typename AugPix<T>::vec4 v =
          *reinterpret_cast<const typename AugPix<T>::vec4*>(base + (off - (back ? 1 : 0)));
      p[0] = AugPix<T>::cvt(back ? v[1] : v[0]);
      p[1] = AugPix<T>::cvt(back ? v[2] : v[1]);
      p[2] = AugPix<T>::cvt(back ? v[3] : v[2]);
    }
  } else {
#pragma unroll
    for (int c = 0; c < C; ++c) p[c] = AugPix<T>::cvt(base[off + c]);
  }
}

__device__ __forceinline__ uint8_t aug_blend(int p00, int p01, int p10, int p11, int w00,
                                              int w01, int w10, int w11, uint8_t) {
  return (uint8_t)((w00 * p00 + w01 * p01 + w10 * p10 + w11 * p11 + 32768) >> 16);
}

// fp32 arithmetic with every multiply and add rounded separately
__device__ __forceinline__ float aug_blend_f(float p00, float p01, float p10, float p11, int w00,
                                             int w01, int w10, int w11) {
#pragma clang fp contract(off)
  const float a = (float)w00 * p00;
  const float b = (float)w01 * p01;
  const float c = (float)w10 * p10;
  const float d = (float)w11 * p11;
  const float top = a + b;
  const float bot = c + d;
  return (top + bot) * 0x1p-16f;
}
__device__ __forceinline__ float aug_blend(float p00, float p01, float p10, float p11, int w00,
                                           int w01, int w10, int w11, float) {
  return aug_blend_f(p00, p01, p10, p11, w00, w01, w10, w11);
}
__device__ __forceinline__ bf16_t aug_blend(float p00, float p01, float p10, float p11, int w00,
                                            int w01, int w10, int w11, bf16_t) {
  return f2bf(aug_blend_f(p00, p01, p10, p11, w00, w01, w10, w11));
}

// one axis of a sample: source coordinate of output position o -> the two tap positions
// (always inside [0, size)), whether each may be read, and the 8-bit fraction
struct AugAxis {
  int origin, step, lo, hi, zero;
  __device__ __forceinline__ void taps(int o, int& c0, int& c1, bool& v0, bool& v1,
                                       int& f) const {
    // wrapping arithmetic: an overflowing parameter gives a wrong pixel, not undefined behaviour
    const int s = (int)((uint32_t)origin + (uint32_t)o * (uint32_t)step);
    const int i0 = s >> 16;
    const int i1 = (int)((uint32_t)i0 + 1u);
    f = (s >> 8) & 255;
    v0 = !zero || (i0 >= lo && i0 <= hi);
    v1 = !zero || (i1 >= lo && i1 <= hi);
    c0 = min(max(i0, lo), hi);
    c1 = min(max(i1, lo), hi);
  }
};

}  // namespace dm
