// Host-side check of the implicit-GEMM geometry helpers (csrc/conv_geom.h), built with
// AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_host_sanitizers.py.
// The device code divides pixel indices by the GEMM grid sizes with
//   q = (umulhi(n, mul) + n) >> shr        (32-bit, n < 2^31)
// — this program checks that formula against n / d for every divisor the kernels use
// (1..4096) on edge values and a pseudo-random sweep, and checks geom_finalize on the
// ResNet-18 layer grids.  Then the data-gradient geometries (dgrad_classes, stride 1 and 2)
// over small images: the (output pixel, dY pixel, weight tap) triples they enumerate must be the
// brute-force set of oy = iy*stride - pad + kh, each once, with disjoint parity classes.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../csrc/conv_geom.h"

static inline unsigned umulhi(unsigned a, unsigned b) {
  return (unsigned)(((unsigned long long)a * b) >> 32);
}

// every (output pixel, dY pixel, packed-weight tap) one geometry visits, and the pixels it writes
static void enumerate(const dm::ConvGeom& g, std::vector<long long>& triples,
                      std::vector<int>& pixels) {
  for (int y = 0; y < g.Hg; ++y)
    for (int x = 0; x < g.Wg; ++x) {
      const int oy = y * g.osy + g.oy0, ox = x * g.osx + g.ox0;
      pixels.push_back(oy < g.OH && ox < g.OW && oy >= 0 && ox >= 0 ? oy * 64 + ox : -1);
      for (int th = 0; th < g.nth; ++th)
        for (int tw = 0; tw < g.ntw; ++tw) {
          const int iy = y * g.isy + g.dy0 + th * g.dys, ix = x * g.isx + g.dx0 + tw * g.dxs;
          if (iy < 0 || iy >= g.H || ix < 0 || ix >= g.W) continue;
          const int tap = (g.kh0 + th * g.khs) * g.KW + (g.kw0 + tw * g.kws);
          triples.push_back(((long long)(oy * 64 + ox) * 4096 + iy * 64 + ix) * 64 + tap);
        }
    }
}

// one conv shape: 0 = fine, else the failed property
static const char* dgrad_case(int H, int W, int K, int stride, int pad) {
  const int OH = (H + 2 * pad - K) / stride + 1, OW = (W + 2 * pad - K) / stride + 1;
  std::vector<long long> want, got;
  std::vector<bool> contributes(64 * 64, false);
  for (int iy = 0; iy < OH; ++iy)
    for (int ix = 0; ix < OW; ++ix)
      for (int kh = 0; kh < K; ++kh)
        for (int kw = 0; kw < K; ++kw) {
          const int oy = iy * stride - pad + kh, ox = ix * stride - pad + kw;
          if (oy < 0 || oy >= H || ox < 0 || ox >= W) continue;
          want.push_back(((long long)(oy * 64 + ox) * 4096 + iy * 64 + ix) * 64 + kh * K + kw);
          contributes[oy * 64 + ox] = true;
        }
  dm::ConvGeom base;
  if (dm::dgrad_base_geom(base, 1, OH, OW, 8, H, W, 8, K, K)) return "base geometry refused";
  std::vector<int> pixels;
  bool any_empty = false;
  dm::ConvGeomSet set{};
  const int ng = dm::dgrad_classes(base, K, K, stride, pad, set, any_empty);
  if (ng < 0 || ng > stride * stride || (stride == 1 && ng != 1)) return "class count";
  for (int i = 0; i < ng; ++i) enumerate(set.g[i], got, pixels);
  std::sort(got.begin(), got.end());
  std::sort(want.begin(), want.end());
  if (std::adjacent_find(got.begin(), got.end()) != got.end()) return "a triple is visited twice";
  if (got != want) return "triples differ from the brute-force set";
  std::sort(pixels.begin(), pixels.end());
  if (!pixels.empty() && pixels.front() < 0) return "a row outside the output";
  if (std::adjacent_find(pixels.begin(), pixels.end()) != pixels.end())
    return "an output pixel belongs to two classes";
  for (int oy = 0; oy < H; ++oy)
    for (int ox = 0; ox < W; ++ox)
      if (!std::binary_search(pixels.begin(), pixels.end(), oy * 64 + ox) &&
          (!any_empty || contributes[oy * 64 + ox]))
        return "an uncovered pixel without any_empty, or one that receives a contribution";
  return nullptr;
}

int main() {
  unsigned long long checked = 0;
  unsigned x = 12345u;
  for (unsigned d = 1; d <= 4096; ++d) {
    unsigned mul, shr;
    dm::fastdiv_init(d, mul, shr);
    const unsigned edge[] = {0u, 1u, d - 1, d, d + 1, 2 * d - 1, 2 * d, 0x7fffffffu,
                             0x7fffffffu - d, (0x7fffffffu / d) * d, (0x7fffffffu / d) * d - 1};
    for (unsigned n : edge) {
      if (n > 0x7fffffffu) continue;
      const unsigned q = (umulhi(n, mul) + n) >> shr;
      if (q != n / d) {
        std::printf("fastdiv mismatch d=%u n=%u q=%u\n", d, n, q);
        return 1;
      }
      ++checked;
    }
    for (int i = 0; i < 2000; ++i) {
      x = x * 1664525u + 1013904223u;
      const unsigned n = x & 0x7fffffffu;
      const unsigned q = (umulhi(n, mul) + n) >> shr;
      if (q != n / d) {
        std::printf("fastdiv mismatch d=%u n=%u q=%u\n", d, n, q);
        return 1;
      }
      ++checked;
    }
  }
  // ResNet-18 grids: m = (n*Hg + y)*Wg + x decomposed back exactly
  const int grids[][2] = {{112, 112}, {56, 56}, {28, 28}, {14, 14}, {7, 7}, {56, 28}};
  for (auto& gr : grids) {
    dm::ConvGeom g{};
    g.Hg = gr[0];
    g.Wg = gr[1];
    dm::geom_finalize(g);
    for (unsigned m = 0; m < 256u * g.Hg * g.Wg; m += 97) {
      const unsigned t = (umulhi(m, g.wg_mul) + m) >> g.wg_shr;
      const unsigned xx = m - t * g.Wg;
      const unsigned n = (umulhi(t, g.hg_mul) + t) >> g.hg_shr;
      const unsigned y = t - n * g.Hg;
      if (xx >= (unsigned)g.Wg || y >= (unsigned)g.Hg || (n * g.Hg + y) * g.Wg + xx != m) {
        std::printf("decompose mismatch grid %dx%d m=%u\n", g.Hg, g.Wg, m);
        return 1;
      }
      ++checked;
    }
  }
  int cases = 0;
  for (int H = 1; H <= 7; ++H)
    for (int W = 1; W <= 7; ++W)
      for (int K : {1, 2, 3, 4, 5, 7})
        for (int stride = 1; stride <= 2; ++stride)
          for (int pad = 0; pad < K; ++pad) {
            if (H + 2 * pad < K || W + 2 * pad < K) continue;
            if (const char* err = dgrad_case(H, W, K, stride, pad)) {
              std::printf("dgrad geometry H=%d W=%d K=%d stride=%d pad=%d: %s\n", H, W, K, stride,
                          pad, err);
              return 1;
            }
            ++cases;
          }
  if (cases != 1638) {
    std::printf("dgrad geometry sweep: %d cases, not 1638\n", cases);
    return 1;
  }
  std::printf("ok %llu + %d dgrad geometries\n", checked, cases);
  return 0;
}
