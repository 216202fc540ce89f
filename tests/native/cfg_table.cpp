// Host-side check of the conv kernel config tables (csrc/conv_cfg.h): internal consistency,
// then one line per row in a fixed `key=value` format ("fwd ..." / "wgrad ..." for the ids
// callers may name, "tile ..." for the fallback-only igemm tiles), then "ok".  The tests
// read those lines (tests/test_cpu_components.py, tests/test_native_resnet_kernels.py), and
// tests/test_host_sanitizers.py builds this with AddressSanitizer + UBSan.
#include <cstdio>
#include <initializer_list>
#include <type_traits>

#include "../../csrc/conv_cfg.h"

using namespace dm;

static int fail(const char* what, int id) {
  std::printf("cfg table: %s (id %d)\n", what, id);
  return 1;
}

template <class Row>
static void print_row(const char* kind, const Row& c) {
  std::printf("%s", kind);
  cfg_fields(c, [](const char* k, auto v) {
    if constexpr (std::is_same_v<decltype(v), const char*>) std::printf(" %s=%s", k, v);
    else std::printf(" %s=%d", k, (int)v);
  });
  std::printf("\n");
}

int main() {
  for (size_t i = 0; i < kNumConvCfgs; ++i) {
    const ConvCfg& c = kConvCfgs[i];
    for (size_t j = 0; j < i; ++j)
      if (kConvCfgs[j].id == c.id) return fail("duplicate id", c.id);
    if (c.id == 0) return fail("id 0 means none", c.id);
    if (conv_tile(c.id) != &c || (conv_cfg(c.id) != nullptr) != (c.id > 0))
      return fail("lookup", c.id);
    // a fallback is an igemm tile with the same row tile (the statistics slab rows match)
    for (int fb : {c.fallback, c.fallback128}) {
      if (c.family == ConvFamily::igemm || c.family == ConvFamily::res64) {
        if (fb) return fail("igemm / res64 take no fallback", c.id);
        continue;
      }
      const ConvCfg* t = conv_tile(fb);
      if (!t || t->family != ConvFamily::igemm || t->rowtile != c.rowtile)
        return fail("fallback does not resolve to an igemm tile of the same row tile", c.id);
    }
    if (c.pre_reroute) {
      const ConvCfg* r = conv_cfg(c.pre_reroute);
      if (c.pre_bn || !r || !r->pre_bn || r->pre_reroute || r->rowtile != c.rowtile)
        return fail("pre-BN reroute", c.id);
    }
    const bool tiled = c.family != ConvFamily::res64;
    if (tiled ? c.rowtile != c.bm || c.bm <= 0 || c.bn <= 0 : c.rowtile != 0)
      return fail("row tile != BM", c.id);
    if (c.family == ConvFamily::halo && !c.halo_waves) return fail("halo tile selector", c.id);
    if (c.family == ConvFamily::pipe && (!c.minw || c.bm != 256)) return fail("pipe tile", c.id);
    if (c.multi_merge_red && !c.multi) return fail("merged / RED multi launch without multi", c.id);
    if (c.merge_same_c && !c.multi_merge_red) return fail("merge_same_c without merge", c.id);
    bool found = false;  // the compile-time row lookup agrees with the runtime one
    const bool hit = with_cfg_row<kConvCfgs, ConvFamily::igemm>(c.id, [&](auto row) {
      found = kConvCfgs[decltype(row)::value].id == c.id;
    });
    if (hit != (c.family == ConvFamily::igemm) || found != hit) return fail("with_cfg_row", c.id);
  }
  if (conv_tile(14)->bm != conv_tile(11)->bm || conv_tile(14)->mf32 != conv_tile(11)->mf32 ||
      conv_tile(14)->depth != conv_tile(11)->depth)
    return fail("14 is an alias of 11", 14);
  for (size_t i = 0; i < kNumWgradCfgs; ++i) {
    const WgradCfg& c = kWgradCfgs[i];
    for (size_t j = 0; j < i; ++j)
      if (kWgradCfgs[j].id == c.id) return fail("duplicate wgrad id", c.id);
    if (c.id <= 0 || wgrad_cfg(c.id) != &c) return fail("wgrad lookup", c.id);
    const bool falls = c.family == WgradFamily::halo || c.family == WgradFamily::s2;
    for (int fb : {c.fallback, c.fallback128}) {
      const WgradCfg* t = fb ? wgrad_cfg(fb) : nullptr;
      if (falls ? !t || t->family != WgradFamily::v2 : fb != 0) return fail("wgrad fallback", c.id);
    }
    if (falls && wgrad_cfg(c.fallback128)->bm != 128) return fail("wgrad fallback128 tile", c.id);
    if ((c.family == WgradFamily::v2) != (c.bm > 0 && c.bk > 0)) return fail("v2 tile", c.id);
    if (falls != (c.taps > 0 && c.taps % 3 == 0)) return fail("taps per block", c.id);
  }
  if (conv_cfg(0) || conv_cfg(-1) || conv_cfg(18) || conv_cfg(94) || wgrad_cfg(0) || wgrad_cfg(1) ||
      wgrad_cfg(9))
    return fail("an id outside the table resolves", 0);
  for (size_t i = 0; i < kNumConvCfgs; ++i)
    print_row(kConvCfgs[i].id > 0 ? "fwd" : "tile", kConvCfgs[i]);
  for (size_t i = 0; i < kNumWgradCfgs; ++i) print_row("wgrad", kWgradCfgs[i]);
  std::printf("ok\n");
  return 0;
}
