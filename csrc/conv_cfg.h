// The conv kernel configs: what every forward-style `cfg` and weight-gradient `cfg` id is and
// can do, in one table each, and the routing rule (conv_route / conv_route_multi / wgrad_route):
// which kernel a call with these operands runs on.  Host-only plain C++17 (no HIP, no torch):
// the dispatcher (conv_launch.cpp), the launchers, the bindings and (through conv_cfg_info /
// wgrad_cfg_info) the Python layer read it; tests/native/cfg_table.cpp checks and prints the
// tables and tests/native/conv_route.cpp the routes.  Adding a kernel = one row, one launcher,
// one line in the dispatcher.  Which id a layer gets is policy and lives in
// dmlab/ops/convbn.py.
#pragma once
#include <cstddef>
#include <type_traits>

namespace dm {

enum class ConvFamily { igemm, halo, stem, res64, pipe };

// A forward-style conv GEMM (forward, stride-1 dgrad, the parity classes of a stride-2 dgrad)
struct ConvCfg {
  int id;
  ConvFamily family;
  // tile: BM pixels x BN output channels on WM x WN waves; mf32 = 32x32x16 MFMA (else
  // 16x16x32); depth = weight tiles of register prefetch; minw = workgroups per CU the pipe
  // kernel is compiled for; halo_waves = conv_halo's tile selector.  0 where a family has none
  int bm, bn, wm, wn;
  bool mf32;
  int depth, minw, halo_waves;
  // rows per statistics / reduction slab row (0 = one row per workgroup of the persistent res64)
  int rowtile;
  // igemm tile launched when the specialised kernel refuses the geometry (fallback128 when
  // Ncols % 128 == 0), chosen with the same row tile so the slab rows still match; 0 = none
  // (igemm runs everything, res64 throws)
  int fallback, fallback128;
  bool pre_bn;       // stages a fused pre-BN operand relu(x*scale + shift)
  int pre_reroute;   // the id a pre-BN forward runs on instead (0 = none)
  bool red_s1;       // its stride-1 launch takes the BN-backward reduction (RED) epilogue
  bool multi;        // has a multi-geometry launch (a stride-2 dgrad's parity classes)
  bool multi_merge_red;  // ... which takes the merged projection segment and RED
  bool merge_same_c;     // ... whose merged segment needs the projection's channels == dy's
};

// ids below 0 are igemm tiles that exist only as fallbacks: conv_tile() finds them,
// conv_cfg() (what callers may name) does not
constexpr int kTile256x64 = -1, kTile256x128 = -2;

#define DM_IG ConvFamily::igemm
constexpr ConvCfg kConvCfgs[] = {
    // id family   bm   bn wm wn mf32 dp mw hw  rowt fb fb128 pre rr red_s1 multi m+red sameC
    {9, DM_IG, 128, 128, 2, 2, false, 1, 0, 0, 128, 0, 0, false, 0, false, false, false, false},
    {10, DM_IG, 128, 64, 2, 2, false, 1, 0, 0, 128, 0, 0, false, 0, false, false, false, false},
    {11, DM_IG, 64, 64, 2, 2, false, 1, 0, 0, 64, 0, 0, false, 0, false, true, true, false},
    {12, DM_IG, 128, 128, 2, 2, true, 1, 0, 0, 128, 0, 0, false, 0, false, true, true, false},
    {13, DM_IG, 128, 64, 2, 2, true, 1, 0, 0, 128, 0, 0, false, 0, false, true, true, false},
    // 64x64 has no 32x32x16 variant: 14 is an alias of 11
    {14, DM_IG, 64, 64, 2, 2, false, 1, 0, 0, 64, 0, 0, false, 0, false, true, true, false},
    {15, DM_IG, 128, 128, 2, 2, true, 2, 0, 0, 128, 0, 0, false, 0, false, true, true, false},
    {16, DM_IG, 128, 64, 2, 2, true, 2, 0, 0, 128, 0, 0, false, 0, false, true, true, false},
    {17, DM_IG, 64, 64, 2, 2, false, 2, 0, 0, 64, 0, 0, false, 0, false, true, true, false},
    // halo-staged unit-stride tiles (conv_halo.hip): 256 px of 4 x 2 / 4 x 1 waves; 128 px of
    // 2 x 2 waves with two weight tiles of register prefetch
    {39, ConvFamily::halo, 256, 64, 4, 2, true, 1, 0, 16, 256, kTile256x64, kTile256x64,
     true, 0, false, false, false, false},
    {41, ConvFamily::halo, 256, 64, 4, 1, true, 1, 0, 32, 256, kTile256x64, kTile256x64,
     true, 0, false, false, false, false},
    {42, ConvFamily::halo, 128, 128, 2, 2, true, 2, 0, 4 | 0x100, 128, 12, 12,
     true, 0, true, false, false, false},
    // space-to-depth stem with resident weights (conv_stem.hip); not with ADD
    {60, ConvFamily::stem, 256, 64, 0, 0, false, 0, 0, 0, 256, kTile256x64, kTile256x64,
     false, 0, false, false, false, false},
    // persistent resident-weight 64 -> 64 channel 3x3 conv (conv_res64.hip)
    {80, ConvFamily::res64, 0, 0, 0, 0, false, 0, 0, 0, 0, 0, 0, true, 0, true, false, false, false},
    // pipelined LDS-DMA tiles (conv_pipe.hip): 8 waves of 128 x 64 / of 64 x 64, 4 waves of
    // 128 x 64 / of 64 x 64 (two workgroups per CU, 80 KB of LDS each).  They take no fused
    // pre-BN (measured slower than materialising it); the halo tile with the same 256-row
    // slab does
    {90, ConvFamily::pipe, 256, 256, 2, 4, true, 0, 1, 0, 256, kTile256x64, kTile256x128,
     false, 41, true, true, true, true},
    {91, ConvFamily::pipe, 256, 128, 4, 2, true, 0, 1, 0, 256, kTile256x64, kTile256x128,
     false, 41, true, true, true, true},
    {92, ConvFamily::pipe, 256, 128, 2, 2, true, 0, 1, 0, 256, kTile256x64, kTile256x128,
     false, 41, true, true, true, true},
    {93, ConvFamily::pipe, 256, 64, 4, 1, true, 0, 2, 0, 256, kTile256x64, kTile256x128,
     false, 41, true, true, true, true},
    {kTile256x64, DM_IG, 256, 64, 4, 2, true, 1, 0, 0, 256, 0, 0, false, 0, false, false, false, false},
    {kTile256x128, DM_IG, 256, 128, 4, 2, true, 1, 0, 0, 256, 0, 0, false, 0, false, false, false, false},
};
#undef DM_IG
constexpr size_t kNumConvCfgs = sizeof(kConvCfgs) / sizeof(kConvCfgs[0]);

constexpr const ConvCfg* conv_tile(int id) {
  for (size_t i = 0; i < kNumConvCfgs; ++i)
    if (kConvCfgs[i].id == id) return &kConvCfgs[i];
  return nullptr;
}
constexpr const ConvCfg* conv_cfg(int id) { return id > 0 ? conv_tile(id) : nullptr; }

enum class WgradFamily { v2, halo, s2, res64 };

// A weight-gradient GEMM into S fp32 slabs
struct WgradCfg {
  int id;
  WgradFamily family;
  int bm, bk;    // v2 tile: output channels x K columns
  int taps;      // halo / s2: taps per block
  bool pre_bn;   // stages a fused pre-BN operand (no fallback is taken with one)
  // v2 tile launched when the kernel refuses the geometry (fallback128 when Ncols % 128 == 0);
  // 0 = none (v2 runs everything, res64 throws)
  int fallback, fallback128;
};

constexpr WgradCfg kWgradCfgs[] = {
    {2, WgradFamily::v2, 128, 128, 0, false, 0, 0},
    {3, WgradFamily::v2, 64, 128, 0, false, 0, 0},
    // halo-staged 3x3 unit-stride kernel (wgrad_halo.hip)
    {4, WgradFamily::halo, 0, 0, 9, true, 3, 2},
    {5, WgradFamily::halo, 0, 0, 3, true, 3, 2},
    // 64 x 256: the whole K of the s2d stem (4x4 taps x 16 ch) in one tile, so every dY row
    // is read once instead of once per 128-column K tile
    {6, WgradFamily::v2, 64, 256, 0, false, 0, 0},
    // stride-2 3x3 kernel over the input's parity planes (wgrad_halo.hip)
    {7, WgradFamily::s2, 0, 0, 9, false, 3, 2},
    // row-streaming 64 -> 64 channel 3x3 kernel (wgrad_res64.hip), one slab per workgroup
    {8, WgradFamily::res64, 0, 0, 0, true, 0, 0},
};
constexpr size_t kNumWgradCfgs = sizeof(kWgradCfgs) / sizeof(kWgradCfgs[0]);

constexpr const WgradCfg* wgrad_cfg(int id) {
  for (size_t i = 0; i < kNumWgradCfgs; ++i)
    if (kWgradCfgs[i].id == id) return &kWgradCfgs[i];
  return nullptr;
}

// the tile a row (of either table) runs on when its specialised kernel refuses a geometry of
// ncols columns
template <class Row>
constexpr int cfg_fallback(const Row& c, int ncols) {
  return ncols % 128 == 0 ? c.fallback128 : c.fallback;
}

// ---- routing: the kernel a launch runs on.  `fits` is the answer of the routed row's own
// *_supported(geometry) predicate (they stay with their kernels' constants); everything else is
// decided here.  kernel + tile name what runs: an igemm / v2 tile id, or the row of the
// specialised kernel; ok = false: the call is refused.
struct ConvRoute { ConvFamily kernel; int tile; bool ok; };
struct WgradRoute { WgradFamily kernel; int tile; bool ok; };

// One geometry: forward, stride-1 dgrad, one parity class.  add / pre / red: the launch has an
// ADD operand / a fused pre-BN operand / the BN-backward reduction (RED) epilogue.  A tile that
// takes no fused pre-BN names the one (same statistics slab rows) that does: with pre, the row
// is first replaced by its pre_reroute, and `fits` is that row's
constexpr ConvRoute conv_route(const ConvCfg& c0, bool fits, bool add, bool pre, bool red,
                               int ncols) {
  const ConvCfg& c = pre && c0.pre_reroute ? *conv_cfg(c0.pre_reroute) : c0;
  const ConvFamily f = c.family;
  const bool res64 = f == ConvFamily::res64;
  const ConvRoute own{f, c.id, true}, refuse{f, c.id, false};
  if (pre || red) {  // no fallback tile stages a pre-BN operand or reduces; never both at once
    const bool has = res64 || f == ConvFamily::halo || (red && f == ConvFamily::pipe);
    return !(pre && red) && (pre ? c.pre_bn : c.red_s1) && has && fits ? own : refuse;
  }
  // its own kernel where it fits (the stem takes no ADD); else the fallback tile, res64 has none
  if (f == ConvFamily::igemm || (fits && !(add && f == ConvFamily::stem))) return own;
  return res64 ? refuse : ConvRoute{ConvFamily::igemm, cfg_fallback(c, ncols), true};
}

// The parity classes of a stride-2 dgrad in one launch.  fits_all: every class fits; seg2: a
// merged projection segment, seg2_same_c: of the operand's channel count; red: RED epilogue.
// tile kPerClass = no single launch: one conv_route launch per class instead
constexpr int kPerClass = 0;
constexpr ConvRoute conv_route_multi(const ConvCfg& c, bool fits_all, bool seg2, bool seg2_same_c,
                                     bool red) {
  const bool special = seg2 || red;
  const bool single = c.family == ConvFamily::pipe ? fits_all && (!seg2 || seg2_same_c)
                      : c.family == ConvFamily::igemm && (c.multi_merge_red || (c.multi && !special));
  return single ? ConvRoute{c.family, c.id, true} : ConvRoute{c.family, kPerClass, !special};
}

constexpr WgradRoute wgrad_route(const WgradCfg& c, bool fits, bool pre, int ncols) {
  const WgradFamily f = c.family;
  const WgradRoute own{f, c.id, true}, refuse{f, c.id, false};
  const bool res64 = f == WgradFamily::res64;
  if (pre)  // no fallback tile stages a pre-BN operand
    return c.pre_bn && (res64 || f == WgradFamily::halo) && fits ? own : refuse;
  if (f == WgradFamily::v2 || fits) return own;
  return res64 ? refuse : WgradRoute{WgradFamily::v2, cfg_fallback(c, ncols), true};
}

constexpr const char* kConvFamilyNames[] = {"igemm", "halo", "stem", "res64", "pipe"};
constexpr const char* kWgradFamilyNames[] = {"v2", "halo", "s2", "res64"};
constexpr const char* family_name(ConvFamily f) { return kConvFamilyNames[(int)f]; }
constexpr const char* family_name(WgradFamily f) { return kWgradFamilyNames[(int)f]; }

// Every field of a row as f(name, value), value a const char*, int or bool: the one list behind
// the conv_cfg_info / wgrad_cfg_info dicts and the lines tests/native/cfg_table.cpp prints
template <class F>
void cfg_fields(const ConvCfg& c, F&& f) {
  f("id", c.id); f("family", family_name(c.family));
  f("bm", c.bm); f("bn", c.bn); f("wm", c.wm); f("wn", c.wn); f("mf32", c.mf32);
  f("depth", c.depth); f("minw", c.minw); f("halo_waves", c.halo_waves);
  f("rowtile", c.rowtile); f("fallback", c.fallback); f("fallback128", c.fallback128);
  f("pre_bn", c.pre_bn); f("pre_reroute", c.pre_reroute); f("red_s1", c.red_s1);
  f("multi", c.multi); f("multi_merge_red", c.multi_merge_red);
  f("merge_same_c", c.merge_same_c);
}
template <class F>
void cfg_fields(const WgradCfg& c, F&& f) {
  f("id", c.id); f("family", family_name(c.family));
  f("bm", c.bm); f("bk", c.bk); f("taps", c.taps); f("pre_bn", c.pre_bn);
  f("fallback", c.fallback); f("fallback128", c.fallback128);
}

// Runtime id -> compile-time row: calls f(std::integral_constant<size_t, I>) for the row I of
// TABLE (kConvCfgs / kWgradCfgs) that has this id and family FAM, so a launcher takes its
// template arguments from TABLE[I]; false when the family has no such id
template <auto& TABLE, auto FAM, size_t I = 0, class F>
bool with_cfg_row(int id, F&& f) {
  if constexpr (I < sizeof(TABLE) / sizeof(TABLE[0])) {
    if constexpr (TABLE[I].family == FAM) {
      if (TABLE[I].id == id) {
        f(std::integral_constant<size_t, I>{});
        return true;
      }
    }
    return with_cfg_row<TABLE, FAM, I + 1>(id, f);
  } else {
    return false;
  }
}

}  // namespace dm
