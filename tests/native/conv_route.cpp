// The conv routing rule (csrc/conv_cfg.h: conv_route, conv_route_multi, wgrad_route) for every
// row and every combination of its boolean inputs, ncols 64 and 128, one line each:
//   conv <id> fits= add= pre= red= ncols= : <family> <tile> | refuse
//   multi <id> fits= seg2= same= red= : <family> <tile> | loop | refuse
//   wgrad <id> fits= pre= ncols= : <family> <tile> | refuse
// then "ok".  tests/test_conv_route_cpu.py compares the lines with the rule written out per id;
// tests/test_host_sanitizers.py builds this with AddressSanitizer + UBSan.
#include <cstdio>
#include <initializer_list>

#include "../../csrc/conv_cfg.h"

using namespace dm;

template <class Route>
static void print_route(const Route& r, bool per_class = false) {
  if (!r.ok) std::printf(" : refuse\n");
  else if (per_class) std::printf(" : loop\n");
  else std::printf(" : %s %d\n", family_name(r.kernel), r.tile);
}

// the rule is constexpr: a route is usable as a template argument or in a static_assert
static_assert(conv_route(*conv_cfg(90), false, false, false, false, 128).tile == kTile256x128, "");
static_assert(!wgrad_route(*wgrad_cfg(8), false, false, 64).ok, "");

int main() {
  for (size_t i = 0; i < kNumConvCfgs; ++i) {
    const ConvCfg& c = kConvCfgs[i];
    for (int b = 0; b < 16; ++b)
      for (int ncols : {64, 128}) {
        const bool fits = b & 1, add = b & 2, pre = b & 4, red = b & 8;
        std::printf("conv %d fits=%d add=%d pre=%d red=%d ncols=%d", c.id, fits, add, pre, red,
                    ncols);
        print_route(conv_route(c, fits, add, pre, red, ncols));
      }
    for (int b = 0; b < 16; ++b) {
      const bool fits = b & 1, seg2 = b & 2, same = b & 4, red = b & 8;
      std::printf("multi %d fits=%d seg2=%d same=%d red=%d", c.id, fits, seg2, same, red);
      const ConvRoute r = conv_route_multi(c, fits, seg2, same, red);
      print_route(r, r.tile == kPerClass);
    }
  }
  for (size_t i = 0; i < kNumWgradCfgs; ++i)
    for (int b = 0; b < 4; ++b)
      for (int ncols : {64, 128}) {
        const bool fits = b & 1, pre = b & 2;
        std::printf("wgrad %d fits=%d pre=%d ncols=%d", kWgradCfgs[i].id, fits, pre, ncols);
        print_route(wgrad_route(kWgradCfgs[i], fits, pre, ncols));
      }
  std::printf("ok\n");
  return 0;
}
