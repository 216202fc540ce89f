// Geometry of one implicit-GEMM convolution launch (shared by host and device code).
#pragma once

namespace dm {

constexpr int MAXTAPS = 64;

struct ConvGeom {
  int N, H, W, C;            // input tensor NHWC; C % 8 == 0 and C/8 a power of two
  int lgC8;                  // log2(C / 8)
  int Hg, Wg;                // GEMM rows: m = (n*Hg + y)*Wg + x
  int isy, isx;              // input coordinate = (y*isy + dy_t, x*isx + dx_t)
  int OH, OW, OC;            // output tensor (NHWC, channel count OC)
  int osy, osx, oy0, ox0;    // output coordinate = (y*osy + oy0, x*osx + ox0)
  // tap grid: t = th*ntw + tw, th < nth, tw < ntw
  int nth, ntw;
  int dy0, dys, dx0, dxs;    // dy_t = dy0 + th*dys, dx_t = dx0 + tw*dxs
  int kh0, khs, kw0, kws, KW;// packed-weight tap = (kh0 + th*khs)*KW + (kw0 + tw*kws)
  int Ncols;                 // output channels of the GEMM
  int wK;                    // packed weight row length (elements) = KH*KW*C
  long long M;               // N*Hg*Wg
  int K;                     // ntaps*C
  // magic-number division by Wg and Hg (m < 2^31): q = (umulhi(n, mul) + n) >> shr
  unsigned wg_mul, wg_shr, hg_mul, hg_shr;
  // optional 1-bit mask of the epilogue's ADD operand (bit j of byte i = element 8i + j of the
  // NHWC output): the identity-skip gradient dres = dout * mask is added without ever being
  // materialised (0 = plain ADD)
  const unsigned char* addm;
};

// several geometries for one launch (selected by blockIdx.z)
struct ConvGeomSet {
  ConvGeom g[4];
  static ConvGeomSet one(const ConvGeom& g0) {
    ConvGeomSet s{};
    s.g[0] = g0;
    return s;
  }
};

// A second K segment appended to one geometry of a ConvGeomSet launch: after the geometry's
// own taps, the block accumulates X2[pixel] . W2 over C2 more channels at the SAME GEMM row
// pixel (tap offset 0).  The stride-2 block's 1x1/s2/p0 projection has exactly the pixel map
// of the 3x3/s2/p1 conv's parity class (0,0) centre tap, so its data gradient joins that
// class's K loop and the block output gradient is written once (no accumulate pass).
struct DgradSeg2 {
  const void* X2;      // bf16 [N][H][W][C2] (the geometry's input grid)
  const void* W2;      // bf16 [Ncols][C2]
  unsigned x2bytes, w2bytes;
  int C2;              // channels of X2 (multiple of 64)
  int z;               // geometry index (blockIdx.z) that takes the segment
};

inline void fastdiv_init(unsigned d, unsigned& mul, unsigned& shr) {
  unsigned l = 0;
  while ((1u << l) < d) ++l;
  mul = (unsigned)((((unsigned long long)1 << 32) * ((1ull << l) - d)) / d + 1);
  shr = l;
}
inline void geom_finalize(ConvGeom& g) {
  fastdiv_init((unsigned)g.Wg, g.wg_mul, g.wg_shr);
  fastdiv_init((unsigned)g.Hg, g.hg_mul, g.hg_shr);
}

// ---- the geometries of a conv's three GEMMs from plain conv parameters.  The builders that can
// meet invalid input return its message (nullptr = fine) for the caller to raise.
inline const char* geom_channels(ConvGeom& g, int C) {
  g.C = C;
  for (g.lgC8 = 0; (1 << g.lgC8) < C / 8;) ++g.lgC8;
  return (1 << g.lgC8) == C / 8 ? nullptr : "C/8 must be a power of two";
}

// forward (and the weight gradient's operand walk): x [N,H,W,C] -> y [N,OH,OW,Cout]
inline const char* conv_fwd_geom(ConvGeom& g, int N, int H, int W, int C, int Cout, int KH,
                                 int KW, int stride, int pad, int OH, int OW) {
  g = ConvGeom{};
  g.N = N; g.H = H; g.W = W;
  if (const char* err = geom_channels(g, C)) return err;
  g.Hg = OH; g.Wg = OW; g.isy = stride; g.isx = stride;
  g.OH = OH; g.OW = OW; g.OC = Cout; g.osy = 1; g.osx = 1; g.oy0 = 0; g.ox0 = 0;
  g.nth = KH; g.ntw = KW; g.dy0 = -pad; g.dys = 1; g.dx0 = -pad; g.dxs = 1;
  g.kh0 = 0; g.khs = 1; g.kw0 = 0; g.kws = 1; g.KW = KW;
  g.Ncols = Cout; g.wK = KH * KW * C;
  g.M = (long long)N * OH * OW; g.K = KH * KW * C;
  if (KH * KW > MAXTAPS) return "too many taps";
  geom_finalize(g);
  return nullptr;
}

// A data gradient as a forward-style GEMM: dy [N,OH,OW,Cout] is the input, dx [N,H,W,Cin] the
// output; the tap grid is filled in per parity class below
inline const char* dgrad_base_geom(ConvGeom& g, int N, int OH, int OW, int Cout, int H, int W,
                                   int Cin, int KH, int KW) {
  g = ConvGeom{};
  g.N = N; g.H = OH; g.W = OW;
  g.OH = H; g.OW = W; g.OC = Cin;
  g.KW = KW; g.Ncols = Cin; g.wK = KH * KW * Cout;
  return geom_channels(g, Cout);
}

// The parity classes of a data gradient of stride s = 1 or 2: class (a, b), a, b < s, writes the
// output pixels (s*y + a, s*x + b), which are disjoint, from the taps kh = (a + pad) mod s, + s,
// ... (tap offsets (a + pad - kh) / s encode the 180-degree flip).  Stride 1 is the one class of
// every pixel and tap.  The classes go into set a-major and their count is returned; one
// without pixels or without taps is left out (any_empty: some class has no taps, e.g. the odd
// pixels of a 1x1/s2 conv, so its pixels are exactly zero)
inline int dgrad_classes(const ConvGeom& base, int KH, int KW, int s, int pad, ConvGeomSet& set,
                         bool& any_empty) {
  int ng = 0;
  any_empty = false;
  for (int a = 0; a < s; ++a)
    for (int b = 0; b < s; ++b) {
      ConvGeom g = base;
      const int kh0 = (a + pad) % s, kw0 = (b + pad) % s;
      const int nth = (KH - kh0 + s - 1) / s, ntw = (KW - kw0 + s - 1) / s;
      if (nth <= 0 || ntw <= 0) { any_empty = true; continue; }
      g.Hg = (g.OH - a + s - 1) / s; g.Wg = (g.OW - b + s - 1) / s;
      if (g.Hg <= 0 || g.Wg <= 0) continue;
      g.isy = 1; g.isx = 1; g.osy = s; g.osx = s; g.oy0 = a; g.ox0 = b;
      g.nth = nth; g.ntw = ntw;
      g.dy0 = (a + pad - kh0) / s; g.dys = -1; g.dx0 = (b + pad - kw0) / s; g.dxs = -1;
      g.kh0 = kh0; g.khs = s; g.kw0 = kw0; g.kws = s;
      g.M = (long long)g.N * g.Hg * g.Wg; g.K = nth * ntw * g.C;
      geom_finalize(g);
      set.g[ng++] = g;
    }
  return ng;
}

}  // namespace dm
