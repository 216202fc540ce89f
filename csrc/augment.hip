// On-device data augmentation: one launch gathers a batch by dataset row and applies a
// per-sample crop / resize / horizontal flip (docs/KERNELS.md, "Augmentation").
//
// images (N,H,W,C) channel-innermost, C = 1 or 3, u8 / fp32 / bf16; idx int64 [B]; params
// int32 [B,8] = X0, Y0, DX, DY, flags, xbox, ybox, 0 (16.16 fixed point; flags bit 0 flip,
// bit 1 zero-fill; box = lo | hi << 16, inclusive); out (B,OH,OW,C).  Per output pixel
//   ox' = flip ? OW-1-ox : ox;  sx = X0 + ox'*DX;  xi = sx >> 16;  fx = (sx >> 8) & 255
// (the same for y), four taps (yi|yi+1, xi|xi+1) with integer weights (256-fy|fy)*(256-fx|fx).
// u8: (sum w*p + 32768) >> 16 in int32.  fp32 / bf16: ((w00*p00 + w01*p01) + (w10*p10 +
// w11*p11)) * 2^-16 in fp32, every operation rounded on its own (no FMA contraction), then
// round-to-nearest-even into the storage type.  A tap outside the box reads as zero (zero-fill)
// or is clamped to the box; the box itself is clamped to the image, so no parameter value can
// produce an address outside the sample.  A row whose idx is outside [0,N) is written as
// zeros and never used as an address (the rule eval_metrics applies to labels).
//
// Memory-bound: a thread owns 16/sizeof(T) consecutive output pixels, i.e. C 16-byte chunks
// of the flat output, computes them into registers and writes them with non-temporal 16-byte
// stores (the batch is read once, by the next kernel, long after).  The four taps of
// neighbouring pixels overlap, so the reads are served by L1/L2 after the first touch; what
// limits the kernel is the number of load instructions, so a 3-channel tap is ONE load of four
// elements at the pixel's own (element-aligned) address, the fourth dropped; the tap that ends
// the tensor starts one element earlier instead.  An output that is not 16-byte aligned, and
// the last partial chunk, take scalar stores.
#include "augment_common.h"

namespace dm {

template <typename T, int C, bool PACK>
__global__ void __launch_bounds__(256) augment_kernel(
    const T* __restrict__ images, const long long* __restrict__ idx,
    const int* __restrict__ params, T* __restrict__ out, long long N, int H, int W, int B, int OH,
    int OW, long long npix, int vec) {
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
  AugAxis ax, ay;
  long long src = 0;  // element offset of the sample
  const long long total = N * H * W * C;
  bool rowok = false, flip = false;
  int y0 = 0, y1 = 0, fy = 0;
  bool vy0 = false, vy1 = false;
  bool newb = true, newy = true;
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    if (p0 + k < npix) {
      if (newb) {
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
        newb = false;
        newy = true;
      }
      if (newy) {
        ay.taps(oy, y0, y1, vy0, vy1, fy);
        newy = false;
      }
      int x0, x1, fx;
      bool vx0, vx1;
      ax.taps(flip ? OW - 1 - ox : ox, x0, x1, vx0, vx1, fx);
      const int w00 = (256 - fy) * (256 - fx), w01 = (256 - fy) * fx;
      const int w10 = fy * (256 - fx), w11 = fy * fx;
      const long long r0 = src + (long long)y0 * W * C, r1 = src + (long long)y1 * W * C;
      // the tap positions are clamped into the sample (row 0 for a bad idx), so every load is
      // in range; loading first and selecting afterwards keeps the loads independent
      acc_t p00[C], p01[C], p10[C], p11[C];
      aug_tap<T, C, PACK>(images, r0 + x0 * C, total, p00);
      aug_tap<T, C, PACK>(images, r0 + x1 * C, total, p01);
      aug_tap<T, C, PACK>(images, r1 + x0 * C, total, p10);
      aug_tap<T, C, PACK>(images, r1 + x1 * C, total, p11);
      const bool v00 = vy0 && vx0, v01 = vy0 && vx1, v10 = vy1 && vx0, v11 = vy1 && vx1;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const acc_t a00 = v00 ? p00[c] : (acc_t)0, a01 = v01 ? p01[c] : (acc_t)0;
        const acc_t a10 = v10 ? p10[c] : (acc_t)0, a11 = v11 ? p11[c] : (acc_t)0;
        vals[k * C + c] = rowok ? aug_blend(a00, a01, a10, a11, w00, w01, w10, w11, T())
                                : (T)0;
      }
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
static void augment_launch(const void* images, const long long* idx, const int* params, void* out,
                           long long N, int H, int W, int C, int B, int OH, int OW,
                           hipStream_t st) {
  constexpr int PPT = 16 / (int)sizeof(T);
  const long long npix = (long long)B * OH * OW;
  const long long threads = (npix + PPT - 1) / PPT;
  const unsigned grid = (unsigned)((threads + 255) / 256);
  const int vec = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  const T* im = (const T*)images;
  T* o = (T*)out;
  if (C == 1)
    augment_kernel<T, 1, false><<<grid, 256, 0, st>>>(im, idx, params, o, N, H, W, B, OH, OW, npix,
                                                      vec);
  else if (N * H * W * 3 >= 4)
    augment_kernel<T, 3, true><<<grid, 256, 0, st>>>(im, idx, params, o, N, H, W, B, OH, OW, npix,
                                                     vec);
  else  // a single 1 x 1 image: no room for a 4-element load
    augment_kernel<T, 3, false><<<grid, 256, 0, st>>>(im, idx, params, o, N, H, W, B, OH, OW, npix,
                                                      vec);
}

// dtype: 0 = u8, 1 = fp32, 2 = bf16
void augment_apply(const void* images, const long long* idx, const int* params, void* out,
                   long long N, int H, int W, int C, int B, int OH, int OW, int dtype,
                   hipStream_t st) {
  if (dtype == 0)
    augment_launch<uint8_t>(images, idx, params, out, N, H, W, C, B, OH, OW, st);
  else if (dtype == 1)
    augment_launch<float>(images, idx, params, out, N, H, W, C, B, OH, OW, st);
  else
    augment_launch<bf16_t>(images, idx, params, out, N, H, W, C, B, OH, OW, st);
}

}  // namespace dm
