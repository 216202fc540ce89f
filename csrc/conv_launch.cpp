// The conv dispatcher: every forward-style and weight-gradient launch goes through here.  The
// routing rule itself is conv_cfg.h's (conv_route / conv_route_multi / wgrad_route, pure and
// tested on the CPU); this file feeds it the `fits` answers of the kernels' *_supported
// predicates and calls the family's launcher.  A new kernel = one line in fits() and in run().
// With `dry` set an entry point reports the route it would take and launches nothing.
#include <stdexcept>
#include <string>

#include "kernels.h"

namespace dm {
namespace {

bool fits(const ConvCfg& c, const ConvGeom& g) {
  switch (c.family) {
    case ConvFamily::igemm: return true;
    case ConvFamily::halo: return conv_halo_supported(g);
    case ConvFamily::stem: return stem_conv_supported(g);
    case ConvFamily::res64: return conv_res64_supported(g);
    case ConvFamily::pipe: return conv_pipe_supported(g, c.id);
  }
  return false;
}
bool fits(const WgradCfg& c, const ConvGeom& g) {
  switch (c.family) {
    case WgradFamily::v2: return true;
    case WgradFamily::halo: return wgrad_halo_supported(g);
    case WgradFamily::s2: return wgrad_s2_supported(g);
    case WgradFamily::res64: return wgrad_res64_supported(g);
  }
  return false;
}

void run(const ConvRoute& r, const ConvOperands& ops, const ConvGeomSet& gs, int ng,
         hipStream_t st) {
  const ConvCfg& row = *conv_tile(r.tile);
  switch (r.kernel) {
    case ConvFamily::igemm: return igemm_tile(ops, gs, ng, row, st);
    case ConvFamily::pipe: return conv_pipe(ops, gs, ng, row, st);
    case ConvFamily::halo: return conv_halo(ops, gs.g[0], row, st);
    case ConvFamily::stem: return stem_conv(ops, gs.g[0], row, st);
    case ConvFamily::res64: return conv_res64(ops, gs.g[0], row, st);
  }
}

// (csrc/conv_cfg.h: pre_bn, red_s1, multi_merge_red; the kernels' *_supported limits)
[[noreturn]] void refuse(const char* what, int cfg) {
  throw std::runtime_error(std::string(what) + ": cfg " + std::to_string(cfg) +
                           " has no kernel for these operands on this geometry");
}

}  // namespace

void conv_launch(const ConvOperands& ops, const ConvGeom& g, const ConvCfg& cfg, hipStream_t st,
                 ConvRoute* dry) {
  // a pre-BN launch asks the row it is rerouted to
  const bool pre = ops.pre_sc;
  const bool fit = fits(pre && cfg.pre_reroute ? *conv_cfg(cfg.pre_reroute) : cfg, g);
  const ConvRoute r = conv_route(cfg, fit, ops.add, pre, ops.red, g.Ncols);
  if (dry) *dry = r;
  else if (!r.ok || ops.seg2) refuse("conv_launch", cfg.id);
  else run(r, ops, ConvGeomSet::one(g), 1, st);
}

bool conv_launch_multi(const ConvOperands& ops, const ConvGeomSet& gs, int ng, const ConvCfg& cfg,
                       hipStream_t st, ConvRoute* dry) {
  if (ops.stats || ops.pre_sc)  // the classes' statistics row tiles would collide
    throw std::runtime_error("conv_launch_multi: no statistics and no pre-BN operand");
  const bool seg2 = ops.seg2, red = ops.red;
  if (ng < 1 && !dry) return !seg2 && !red;  // no classes: nothing to launch
  bool all = true;
  for (int i = 0; all && i < ng; ++i) all = fits(cfg, gs.g[i]);
  const ConvRoute r = conv_route_multi(cfg, all, seg2, seg2 && ops.seg2->C2 == gs.g[0].C, red);
  if (dry) *dry = r;
  if (dry || !r.ok) return r.ok;
  ConvOperands one = ops;
  one.sched = 0;  // one launch per class: the data-parallel schedule, whatever `balance` said
  if (r.tile != kPerClass) run(r, ops, gs, ng, st);
  else for (int i = 0; i < ng; ++i) conv_launch(one, gs.g[i], cfg, st);
  return true;
}

void wgrad_launch(const WgradOperands& ops, const ConvGeom& g, const WgradCfg& cfg, hipStream_t st,
                  WgradRoute* dry) {
  const WgradRoute r = wgrad_route(cfg, fits(cfg, g), ops.pre_sc, g.Ncols);
  if (dry) return (void)(*dry = r);
  if (!r.ok) refuse("wgrad_launch", cfg.id);
  const WgradCfg& row = *wgrad_cfg(r.tile);
  switch (r.kernel) {
    case WgradFamily::v2: return wgrad_tile(ops, g, row, st);
    case WgradFamily::halo: return wgrad_halo(ops, g, row, st);
    case WgradFamily::s2: return wgrad_s2(ops, g, row, st);
    case WgradFamily::res64: return wgrad_res64(ops, g, row, st);
  }
}

int device_cu_count() {
  static int cus[64] = {};
  int dev = 0, n = 0;
  const bool ok = hipGetDevice(&dev) == hipSuccess;
  int& c = dev >= 0 && dev < 64 ? cus[dev] : n;
  if (!ok || (!c && hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev)))
    throw std::runtime_error("device_cu_count: the HIP runtime reports an error");
  return c;
}

long long conv_stats_rows(long long M, const ConvCfg& cfg) {
  return cfg.rowtile ? (M + cfg.rowtile - 1) / cfg.rowtile : res64_grid(M);
}
long long conv_multi_red_rows(const ConvGeomSet& gs, int ng, const ConvCfg& cfg) {
  if (!cfg.multi_merge_red) return 0;
  long long mmax = 0;
  for (int i = 0; i < ng; ++i) mmax = gs.g[i].M > mmax ? gs.g[i].M : mmax;
  return ng * ((mmax + cfg.rowtile - 1) / cfg.rowtile);
}

}  // namespace dm
