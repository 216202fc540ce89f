// Bindings for the NHWC bf16 ResNet kernels: implicit-GEMM conv (fwd / dgrad /
// wgrad), BatchNorm, pooling, input/weight packing.  The conv bindings check their operands,
// build the geometry (conv_geom.h) from plain conv parameters, so Python never sees kernel
// structs, and hand both to the dispatcher (conv_launch.cpp), which picks the kernel.
#include <torch/extension.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

#include <map>
#include <mutex>

#include "kernels.h"

namespace {

inline hipStream_t cur_stream() {
  return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
}
using DeviceGuard = c10::hip::HIPGuardMasqueradingAsCUDA;
using bf = dm::bf16_t;

inline bf* bp(const at::Tensor& t) { return reinterpret_cast<bf*>(t.data_ptr()); }
inline float* fp(const at::Tensor& t) { return t.data_ptr<float>(); }

void need_bf16_nhwc(const at::Tensor& t, const char* n) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kBFloat16 && t.is_contiguous() && t.dim() == 4,
              n, " must be a contiguous 4-D bf16 HIP tensor [N,H,W,C]");
  TORCH_CHECK(t.size(3) % 8 == 0, n, ": channels must be a multiple of 8");
  TORCH_CHECK((reinterpret_cast<uintptr_t>(t.data_ptr()) & 15) == 0, n, " must be 16-B aligned");
}
void need_f32(const at::Tensor& t, const char* n, int64_t numel = -1) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat && t.is_contiguous(), n,
              " must be a contiguous fp32 HIP tensor");
  if (numel >= 0) TORCH_CHECK(t.numel() >= numel, n, " too small");
}
// the forward geometry of a conv over x [N,H,W,C] (conv_geom.h), its complaints raised
dm::ConvGeom fwd_geom(int N, int H, int W, int C, int Cout, int KH, int KW, int stride, int pad,
                      int OH, int OW) {
  dm::ConvGeom g;
  const char* err = dm::conv_fwd_geom(g, N, H, W, C, Cout, KH, KW, stride, pad, OH, OW);
  TORCH_CHECK(!err, err);
  return g;
}

// the rows of csrc/conv_cfg.h behind a cfg argument
template <class Row>
const Row& row_of(const Row* c, int64_t cfg) {
  TORCH_CHECK(c, "unknown cfg ", cfg);
  return *c;
}
const dm::ConvCfg& cfg_of(int64_t cfg) { return row_of(dm::conv_cfg((int)cfg), cfg); }
const dm::WgradCfg& wgrad_cfg_of(int64_t cfg) { return row_of(dm::wgrad_cfg((int)cfg), cfg); }

// statistics rows a forward conv of this cfg writes
int64_t conv_stats_rows(int64_t M, int64_t cfg) { return dm::conv_stats_rows(M, cfg_of(cfg)); }

bool is_u8(const at::Tensor& t) {
  return t.is_cuda() && t.scalar_type() == at::kByte && t.is_contiguous();
}

// A 1-bit mask over the elements of `of` (bit j of byte i = element 8i + j), or null
const unsigned char* bit_mask(const c10::optional<at::Tensor>& m, const at::Tensor& of,
                              const char* n) {
  if (!m.has_value()) return nullptr;
  TORCH_CHECK(is_u8(*m) && m->numel() * 8 >= of.numel(), n, ": uint8 [numel/8] on the device");
  return m->data_ptr<uint8_t>();
}
// The 1-bit (out > 0) mask bn_apply writes and bn_backward's mode 4 reads: exactly numel/8 bytes
uint8_t* relu_mask(const c10::optional<at::Tensor>& m, const at::Tensor& y, const char* msg) {
  TORCH_CHECK(m.has_value() && is_u8(*m) && m->numel() == y.numel() / 8, msg);
  return m->data_ptr<uint8_t>();
}

// The fused pre-BN operand of a conv over `x` (the kernel stages relu(x*scale + shift)):
// the checked {scale, shift} pointers
std::pair<const float*, const float*> pre_bn(const c10::optional<at::Tensor>& scale,
                                             const c10::optional<at::Tensor>& shift,
                                             const at::Tensor& x) {
  TORCH_CHECK(shift.has_value(), "pre_scale needs pre_shift");
  need_f32(*scale, "pre_scale", x.size(3));
  need_f32(*shift, "pre_shift", x.size(3));
  return {fp(*scale), fp(*shift)};
}

// The pipelined conv's balanced schedule (csrc/conv_pipe_plan.h) needs a workspace: one per
// (device, stream), allocated zeroed at the first balanced launch on that stream and kept for
// every later one, so that the side stream's launches never share the main stream's.  The
// launcher asks for it through pipe_workspace() with the stream it launches on.
struct PipeWs {
  at::Tensor slots, words;  // [cap][256 x 256] fp32; [cap flags + timeout word (+ pad)] int32
  unsigned seq = 0;
  int cap = 0;
};
std::map<std::pair<int, hipStream_t>, PipeWs>& pipe_ws_map() {
  static auto* m = new std::map<std::pair<int, hipStream_t>, PipeWs>();  // outlives torch's teardown
  return *m;
}
std::mutex& pipe_ws_mutex() {
  static std::mutex m;
  return m;
}
dm::PipeWorkspace pipe_workspace(hipStream_t st, int cap) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || cap < 1) return {};
  const std::lock_guard<std::mutex> lock(pipe_ws_mutex());
  PipeWs& w = pipe_ws_map()[{dev, st}];
  if (w.cap < cap) {
    TORCH_CHECK(w.cap == 0, "pipe workspace: the CU count of a device does not change");
    const auto dv = at::Device(at::kCUDA, (c10::DeviceIndex)dev);
    w.slots = at::zeros({cap, 256 * 256}, at::TensorOptions().dtype(at::kFloat).device(dv));
    w.words = at::zeros({(cap + 1 + 3) / 4 * 4}, at::TensorOptions().dtype(at::kInt).device(dv));
    w.cap = cap;
  }
  if (++w.seq == 0) w.seq = 1;  // 0 is the untouched flag
  unsigned* words = reinterpret_cast<unsigned*>(w.words.data_ptr<int>());
  return {w.slots.data_ptr<float>(), words, words + w.cap, w.seq, w.cap};
}

// [(device, balanced launches so far, timeout word)] of every workspace (synchronises): the
// tests' view of which schedule ran; raises like dmlab/parallel/xgmi.py's check() when a
// workgroup gave up waiting for its neighbour's partial tile
py::list conv_pipe_balance_state() {
  py::list out;
  const std::lock_guard<std::mutex> lock(pipe_ws_mutex());
  for (auto& [key, w] : pipe_ws_map()) {
    if (!w.cap) continue;
    const int tmo = w.words[w.cap].item<int>();
    TORCH_CHECK(!tmo, "conv_pipe: a workgroup of the balanced schedule timed out waiting for its "
                      "neighbour's partial tile; that launch's output is incomplete");
    out.append(py::make_tuple(key.first, (int64_t)w.seq, tmo));
  }
  return out;
}

// the `balance` argument of conv_fwd / conv_dgrad: "auto" (the launcher decides), "off" (the
// data-parallel launch) or the workgroup count G of a forced balanced launch
int pipe_sched(const py::object& balance) {
  if (py::isinstance<py::str>(balance)) {
    const auto v = balance.cast<std::string>();
    TORCH_CHECK(v == "auto" || v == "off", "balance: \"auto\", \"off\" or a workgroup count");
    return v == "auto" ? dm::kPipeAuto : 0;
  }
  const int G = balance.cast<int>();
  TORCH_CHECK(G > 0, "balance: a workgroup count > 0");
  return G;
}

// y = conv(x, w)  (+add) ; stats [T][2][Cout] optional
void conv_fwd(at::Tensor x, at::Tensor wpack, at::Tensor y, c10::optional<at::Tensor> stats,
              c10::optional<at::Tensor> add, int64_t KH, int64_t KW, int64_t stride, int64_t pad,
              int64_t cfg, c10::optional<at::Tensor> pre_scale,
              c10::optional<at::Tensor> pre_shift, py::object balance) {
  // pre_scale/pre_shift: x is the previous conv's raw output and the conv consumes
  // relu(x*pre_scale + pre_shift) (fused BN-apply + ReLU; halo kernels only)
  need_bf16_nhwc(x, "x");
  need_bf16_nhwc(y, "y");
  const int Cout = y.size(3), OH = y.size(1), OW = y.size(2);
  // pad is the top/left padding; the output size (taken from y) may imply a smaller
  // bottom/right padding (space-to-depth stem), never a larger one
  TORCH_CHECK(OH <= (x.size(1) + 2 * pad - KH) / stride + 1 && OW <= (x.size(2) + 2 * pad - KW) / stride + 1,
              "output spatial size mismatch");
  TORCH_CHECK(wpack.scalar_type() == at::kBFloat16 && wpack.numel() == (int64_t)Cout * KH * KW * x.size(3),
              "wpack must be bf16 [Cout][KH][KW][C]");
  auto g = fwd_geom(x.size(0), x.size(1), x.size(2), x.size(3), Cout, KH, KW, stride, pad, OH, OW);
  dm::ConvOperands ops{bp(x), bp(wpack), bp(y), pipe_sched(balance)};
  if (stats.has_value()) {
    need_f32(*stats, "stats", conv_stats_rows(g.M, cfg) * 2 * Cout);
    ops.stats = fp(*stats);
  }
  if (add.has_value()) { need_bf16_nhwc(*add, "add"); TORCH_CHECK(add->sizes() == y.sizes()); ops.add = bp(*add); }
  if (pre_scale.has_value()) std::tie(ops.pre_sc, ops.pre_sh) = pre_bn(pre_scale, pre_shift, x);
  const DeviceGuard guard(x.device());
  dm::conv_launch(ops, g, cfg_of(cfg), cur_stream());
}

// part rows of a stride-2 3x3/p1 data gradient with the reduction epilogue (conv_dgrad red_part)
int64_t dgrad_s2_red_rows(int64_t N, int64_t H, int64_t W, int64_t cfg) {
  dm::ConvGeom base{};
  base.N = N; base.OH = H; base.OW = W;
  dm::ConvGeomSet set{};
  bool any_empty;
  const int ng = dm::dgrad_classes(base, 3, 3, 2, 1, set, any_empty);
  return dm::conv_multi_red_rows(set, ng, cfg_of(cfg));
}

// dx = conv_transpose(dy, w) for stride 1 or 2; add: tensor added to the result (may alias dx
// for in-place accumulation)
void conv_dgrad(at::Tensor dy, at::Tensor wd, at::Tensor dx, int64_t KH, int64_t KW,
                int64_t stride, int64_t pad, c10::optional<at::Tensor> add, int64_t cfg,
                c10::optional<at::Tensor> add_mask, c10::optional<at::Tensor> red_y,
                c10::optional<at::Tensor> red_scale, c10::optional<at::Tensor> red_shift,
                c10::optional<at::Tensor> red_mean, c10::optional<at::Tensor> red_invstd,
                c10::optional<at::Tensor> red_part, c10::optional<at::Tensor> red_mask,
                c10::optional<at::Tensor> dy2, c10::optional<at::Tensor> wd2,
                py::object balance) {
  // dy2 / wd2 (optional, stride 2): a 1x1/s2/p0 projection's output gradient and packed data-
  // gradient weights [Cin][1][1][C2]; its data gradient is merged into this launch (parity
  // class (0,0) gets a second K segment), so dx is written once, complete
  // red_* (optional; stride 1: a cfg with red_s1; stride 2: a complete data gradient on a cfg
  // with multi_merge_red, csrc/conv_cfg.h): the backward reduction of the BatchNorm + ReLU whose
  // output gradient dx is (its input red_y, forward scale/shift, mean/invstd, optionally the
  // 1-bit red_mask instead of the mask from red_y) runs in this dgrad's epilogue -> red_part
  // [rows][2][Cin] (bn_backward's pre_slab; rows = conv_stats_rows, stride 2: dgrad_s2_red_rows)
  // add_mask (optional, stride 1): 1-bit mask of `add` (bit j of byte i = element 8i + j), so
  // the identity-skip gradient dres = add * mask is added without being materialised
  need_bf16_nhwc(dy, "dy");
  need_bf16_nhwc(dx, "dx");
  const int N = dy.size(0), OH = dy.size(1), OW = dy.size(2), Cout = dy.size(3);
  const int H = dx.size(1), W = dx.size(2), Cin = dx.size(3);
  TORCH_CHECK(dx.size(0) == N);
  TORCH_CHECK(OH == (H + 2 * pad - KH) / stride + 1 && OW == (W + 2 * pad - KW) / stride + 1,
              "dgrad shape mismatch");
  TORCH_CHECK(wd.scalar_type() == at::kBFloat16 && wd.numel() == (int64_t)Cin * KH * KW * Cout,
              "wd must be bf16 [Cin][KH][KW][Cout]");
  TORCH_CHECK(stride == 1 || stride == 2, "stride must be 1 or 2");
  const dm::ConvCfg& c = cfg_of(cfg);
  dm::ConvOperands ops{bp(dy), bp(wd), bp(dx), pipe_sched(balance)};
  if (add.has_value()) { need_bf16_nhwc(*add, "add"); TORCH_CHECK(add->sizes() == dx.sizes()); ops.add = bp(*add); }
  const bool accumulate = ops.add != nullptr;
  TORCH_CHECK(stride == 1 || !accumulate || ops.add == bp(dx),
              "stride-2 dgrad accumulates only in place (add must alias dx)");
  const DeviceGuard guard(dy.device());
  auto st = cur_stream();
  dm::ConvGeom base;
  const char* err = dm::dgrad_base_geom(base, N, OH, OW, Cout, H, W, Cin, KH, KW);
  TORCH_CHECK(!err, err);
  if (add_mask.has_value())
    TORCH_CHECK(ops.add && stride == 1 && ops.add != bp(dx),
                "add_mask needs a separate add tensor and a stride-1 data gradient");
  const unsigned char* addm = bit_mask(add_mask, dx, "add_mask");
  // the red_* operands, checked against dx and the launch's part rows, become the launch's
  dm::BnBwdRed red{};
  auto red_in = [&](int64_t rows) {
    need_bf16_nhwc(*red_y, "red_y");
    TORCH_CHECK(red_y->sizes() == dx.sizes(), "red_y: dx's shape");
    TORCH_CHECK(red_scale && red_shift && red_mean && red_invstd && red_part,
                "red_*: scale, shift, mean, invstd and part are all required");
    need_f32(*red_scale, "red_scale", Cin);
    need_f32(*red_shift, "red_shift", Cin);
    need_f32(*red_mean, "red_mean", Cin);
    need_f32(*red_invstd, "red_invstd", Cin);
    need_f32(*red_part, "red_part", rows * 2 * Cin);
    red = dm::BnBwdRed{bp(*red_y), bit_mask(red_mask, dx, "red_mask"), fp(*red_scale),
                       fp(*red_shift), fp(*red_mean), fp(*red_invstd), fp(*red_part)};
    ops.red = &red;
  };
  dm::ConvGeomSet set{};
  bool any_empty;
  const int ng = dm::dgrad_classes(base, KH, KW, stride, pad, set, any_empty);
  if (stride == 1) {
    TORCH_CHECK(ng == 1, "dgrad: empty dx");
    set.g[0].addm = addm;
    if (red_y.has_value()) red_in(conv_stats_rows(set.g[0].M, cfg));
    dm::conv_launch(ops, set.g[0], c, st);
    return;
  }
  // a class with no taps is exactly zero, so zero-fill once up front when needed
  if (any_empty && !accumulate)
    TORCH_CHECK(hipMemsetAsync(dx.data_ptr(), 0, dx.numel() * 2, st) == hipSuccess);
  dm::DgradSeg2 seg2{};
  const bool merged = dy2.has_value();
  if (merged) {
    // (the pipelined tiles merge a projection of dy's own channel count: ResNet's always is)
    TORCH_CHECK(c.multi_merge_red && (!c.merge_same_c || dy2->size(3) == Cout) && !accumulate &&
                    ng == 4 && pad == 1 && KH == 3 && KW == 3,
                "dy2: a 3x3/s2/p1 data gradient on a cfg with a merged multi-geometry launch "
                "(csrc/conv_cfg.h multi_merge_red; merge_same_c: projection channels == dy's), "
                "no add");
    need_bf16_nhwc(*dy2, "dy2");
    TORCH_CHECK(dy2->size(0) == N && dy2->size(1) == OH && dy2->size(2) == OW && dy2->size(3) % 64 == 0,
                "dy2: [N, OH, OW, C2] with dy's grid, C2 % 64 == 0");
    TORCH_CHECK(wd2.has_value() && wd2->scalar_type() == at::kBFloat16 && wd2->is_contiguous() &&
                    wd2->numel() == (int64_t)Cin * dy2->size(3),
                "wd2 must be bf16 [Cin][1][1][C2]");
    // the kernels address both through 32-bit buffer ranges (x2bytes / w2bytes below)
    TORCH_CHECK(dy2->numel() * 2 < (1LL << 31) && wd2->numel() * 2 < (1LL << 31),
                "dy2 / wd2: each must be below 2 GiB");
    // class (a, b) = (0, 0) is geometry 0 (a-major): rows (y, x) are the output pixels
    // (2y, 2x), read dY at (y, x) through the centre tap -- the 1x1/s2/p0 map
    TORCH_CHECK(set.g[0].oy0 == 0 && set.g[0].ox0 == 0 && set.g[0].Hg == OH && set.g[0].Wg == OW,
                "dy2: parity class (0,0) must cover dy's grid");
    seg2.X2 = dy2->data_ptr();
    seg2.W2 = wd2->data_ptr();
    seg2.x2bytes = (unsigned)(dy2->numel() * 2);
    seg2.w2bytes = (unsigned)(wd2->numel() * 2);
    seg2.C2 = (int)dy2->size(3);
    seg2.z = 0;
    ops.seg2 = &seg2;
  }
  if (red_y.has_value()) {
    TORCH_CHECK(c.multi_merge_red && !accumulate && !any_empty && ng == 4,
                "red_* with stride 2: a complete data gradient (all 4 parity classes, no add) on "
                "a cfg with a reducing multi-geometry launch (csrc/conv_cfg.h multi_merge_red)");
    red_in(dm::conv_multi_red_rows(set, ng, c));
  }
  TORCH_CHECK(dm::conv_launch_multi(ops, set, ng, c, st),
              "merged / reducing stride-2 dgrad: unsupported cfg / geometry");
}

// dw (fp32 OIHW [Cout][Cin][KH][KW]) = beta*dw + Σ_m dy ⊗ im2col(x)
void conv_wgrad(at::Tensor x, at::Tensor dy, at::Tensor dw, at::Tensor slab, int64_t Cin,
                int64_t KH, int64_t KW, int64_t stride, int64_t pad, double beta, int64_t S,
                int64_t cfg, bool s2d, c10::optional<at::Tensor> pre_scale,
                c10::optional<at::Tensor> pre_shift) {
  // s2d: x/dy are the space-to-depth stem operands (4x4/s1 conv over 4*Cin channels);
  // dw is the original [Cout][Cin][7][7] gradient
  need_bf16_nhwc(x, "x");
  need_bf16_nhwc(dy, "dy");
  const int Cout = dy.size(3);
  need_f32(dw, "dw", s2d ? (int64_t)Cout * Cin * 49 : (int64_t)Cout * Cin * KH * KW);
  auto g = fwd_geom(x.size(0), x.size(1), x.size(2), x.size(3), Cout, KH, KW, stride, pad,
                    dy.size(1), dy.size(2));
  TORCH_CHECK(dy.size(0) == x.size(0));
  need_f32(slab, "slab", (int64_t)S * Cout * g.K);
  const long long steps = (g.M + 63) / 64;
  const long long mchunk = ((steps + S - 1) / S) * 64;  // multiple of both kernels' row step
  const DeviceGuard guard(x.device());
  auto st = cur_stream();
  dm::WgradOperands ops{bp(x), bp(dy), fp(slab), (int)S, mchunk};
  if (pre_scale.has_value()) {
    // x = previous conv's raw output, operand relu(x*sc + sh)
    TORCH_CHECK(pre_shift.has_value() && !s2d, "pre_scale needs pre_shift (not with s2d)");
    std::tie(ops.pre_sc, ops.pre_sh) = pre_bn(pre_scale, pre_shift, x);
  }
  dm::wgrad_launch(ops, g, wgrad_cfg_of(cfg), st);
  if (s2d)
    dm::wgrad_reduce_s2d(fp(slab), (int)S, Cout, (int)Cin, g.C, fp(dw), (float)beta, st);
  else
    dm::wgrad_reduce(fp(slab), (int)S, Cout, g.C, (int)Cin, KH, KW, fp(dw), (float)beta, st);
}

void pack_weights_s2d(at::Tensor w, at::Tensor wf) {
  need_f32(w, "w");
  TORCH_CHECK(w.dim() == 4 && w.size(2) == 7 && w.size(3) == 7, "s2d stem needs a 7x7 kernel");
  const int Cout = w.size(0), C = w.size(1);
  TORCH_CHECK(wf.scalar_type() == at::kBFloat16 && wf.numel() % (Cout * 16) == 0);
  const int Cp = wf.numel() / (Cout * 16);
  TORCH_CHECK(Cp % 8 == 0 && Cp >= 4 * C);
  const DeviceGuard guard(w.device());
  dm::pack_weights_s2d(fp(w), bp(wf), Cout, C, Cp, cur_stream());
}

// idx (optional, int64 [y.size(0)] on the device): y's image n is x's row idx[n] -- the
// device-resident loader's batch gather fused into the packing pass (x = the whole dataset)
void pack_input_s2d(at::Tensor x, at::Tensor y, c10::optional<at::Tensor> idx) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4);
  TORCH_CHECK(x.scalar_type() == at::kFloat || x.scalar_type() == at::kBFloat16);
  need_bf16_nhwc(y, "y");
  TORCH_CHECK(x.size(2) % 2 == 0 && x.size(3) % 2 == 0, "s2d needs even H, W");
  const bool gather = idx.has_value() && idx->defined();
  if (gather) {
    TORCH_CHECK(idx->is_cuda() && idx->scalar_type() == at::kLong && idx->is_contiguous() &&
                    idx->numel() == y.size(0), "idx: int64 [N] row indices on the device");
  } else {
    TORCH_CHECK(y.size(0) == x.size(0));
  }
  TORCH_CHECK(y.size(1) * 2 == x.size(2) && y.size(2) * 2 == x.size(3) && y.size(3) >= 4 * x.size(1));
  const DeviceGuard guard(x.device());
  dm::pack_input_s2d(x.data_ptr(), x.scalar_type() == at::kBFloat16, bp(y), y.size(0), x.size(1),
                     y.size(1), y.size(2), y.size(3), x.stride(0), x.stride(1), x.stride(2),
                     x.stride(3),
                     gather ? reinterpret_cast<const long long*>(idx->data_ptr<int64_t>()) : nullptr,
                     x.size(0), cur_stream());
}

void pack_weights(at::Tensor w, at::Tensor wf, c10::optional<at::Tensor> wd, int64_t Cpad) {
  need_f32(w, "w");
  TORCH_CHECK(w.dim() == 4);
  const int Cout = w.size(0), Cin = w.size(1), KH = w.size(2), KW = w.size(3);
  TORCH_CHECK(wf.scalar_type() == at::kBFloat16 && wf.numel() == (int64_t)Cout * KH * KW * Cpad);
  bf* wdp = nullptr;
  if (wd.has_value()) {
    TORCH_CHECK(wd->scalar_type() == at::kBFloat16 && wd->numel() == (int64_t)Cin * KH * KW * Cout);
    wdp = bp(*wd);
  }
  const DeviceGuard guard(w.device());
  dm::pack_weights(fp(w), bp(wf), wdp, Cout, Cin, Cpad, KH, KW, cur_stream());
}

// LDS-tiled variant: tprefix[l] = first 32x32 (co, ci) tile of layer l
void pack_weights_tiled(at::Tensor desc, at::Tensor tprefix, int64_t ntiles) {
  TORCH_CHECK(desc.is_cuda() && tprefix.is_cuda() && desc.scalar_type() == at::kLong &&
              tprefix.scalar_type() == at::kInt, "desc int64 / tprefix int32 device tensors");
  const int nl = tprefix.numel() - 1;
  TORCH_CHECK(nl >= 1 && nl <= 32 && desc.numel() == 8 * nl, "pack_weights_tiled: 1..32 layers");
  TORCH_CHECK(ntiles >= 1 && ntiles < (1 << 24), "pack_weights_tiled: tile count");
  const DeviceGuard guard(desc.device());
  dm::pack_weights_tiled((const long long*)desc.data_ptr(), tprefix.data_ptr<int>(), nl, (int)ntiles,
                         cur_stream());
}

// ------------------------------------------------------------------ BN
// BatchNorm num_batches_tracked (optional), incremented in the finalize kernels
static long long* num_batches_ptr(const c10::optional<at::Tensor>& nb, const at::Tensor& on) {
  if (!nb.has_value()) return nullptr;
  TORCH_CHECK(nb->scalar_type() == at::kLong && nb->numel() == 1 && nb->device() == on.device(),
              "num_batches: int64 scalar on the device");
  return (long long*)nb->data_ptr();
}

void bn_stats_finalize(at::Tensor stats, int64_t T, double count, at::Tensor gamma, at::Tensor beta,
                       c10::optional<at::Tensor> rmean, c10::optional<at::Tensor> rvar,
                       double momentum, double eps, at::Tensor scale, at::Tensor shift,
                       at::Tensor mean, at::Tensor invstd, at::Tensor work,
                       c10::optional<at::Tensor> num_batches) {
  const int C = gamma.numel();
  need_f32(stats, "stats", T * 2 * C);
  long long* nb = num_batches_ptr(num_batches, stats);
  need_f32(work, "work", 256 * 2 * C);
  for (auto* t : {&gamma, &beta, &scale, &shift, &mean, &invstd}) need_f32(*t, "bn vec", C);
  const DeviceGuard guard(stats.device());
  dm::bn_stats_finalize(fp(stats), T, C, count, fp(gamma), fp(beta),
                        rmean.has_value() ? fp(*rmean) : nullptr, rvar.has_value() ? fp(*rvar) : nullptr,
                        momentum, eps, fp(scale), fp(shift), fp(mean), fp(invstd), fp(work), nb,
                        cur_stream());
}

// ---- cross-rank (synchronized) BatchNorm: float64 rows / sums, the global count on the device
static double* need_f64(const at::Tensor& t, const char* name, int64_t n) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kDouble && t.is_contiguous() && t.numel() == n,
              name, ": contiguous float64 device tensor of ", n, " elements");
  return t.data_ptr<double>();
}

// stats [T][2C], this rank's element count -> row [mean (C) | M2 (C) | n] float64
void bn_sync_local(at::Tensor stats, int64_t T, double count, int64_t C, at::Tensor row,
                   at::Tensor work) {
  TORCH_CHECK(C >= 1 && T >= 1 && count >= 1, "bn_sync_local: C, T, count >= 1");
  need_f32(stats, "stats", T * 2 * C);
  need_f32(work, "work", 256 * 2 * C);
  double* rp = need_f64(row, "row", 2 * C + 1);
  TORCH_CHECK(row.device() == stats.device() && work.device() == stats.device());
  const DeviceGuard guard(stats.device());
  dm::bn_sync_local(fp(stats), (int)T, (int)C, count, rp, fp(work), cur_stream());
}

// rows [ws][2C+1] (every rank's bn_sync_local row, rank order) -> scale/shift/mean/invstd, the
// running statistics, num_batches += 1, total = Σ n (float64 device scalar)
void bn_sync_finalize(at::Tensor rows, at::Tensor gamma, at::Tensor beta,
                      c10::optional<at::Tensor> rmean, c10::optional<at::Tensor> rvar,
                      double momentum, double eps, at::Tensor scale, at::Tensor shift,
                      at::Tensor mean, at::Tensor invstd, c10::optional<at::Tensor> num_batches,
                      at::Tensor total) {
  const int C = gamma.numel();
  TORCH_CHECK(rows.dim() == 2 && rows.size(0) >= 1 && rows.size(1) == 2 * C + 1,
              "rows: [ws][2C+1]");
  const double* rp = need_f64(rows, "rows", rows.size(0) * (2 * C + 1));
  double* tp = need_f64(total, "total", 1);
  long long* nb = num_batches_ptr(num_batches, rows);
  for (auto* t : {&gamma, &beta, &scale, &shift, &mean, &invstd}) need_f32(*t, "bn vec", C);
  if (rmean.has_value()) need_f32(*rmean, "rmean", C);
  if (rvar.has_value()) need_f32(*rvar, "rvar", C);
  TORCH_CHECK(rmean.has_value() == rvar.has_value(), "running mean and var: both or neither");
  const DeviceGuard guard(rows.device());
  dm::bn_sync_finalize(rp, (int)rows.size(0), C, fp(gamma), fp(beta),
                       rmean.has_value() ? fp(*rmean) : nullptr,
                       rvar.has_value() ? fp(*rvar) : nullptr, momentum, eps, fp(scale), fp(shift),
                       fp(mean), fp(invstd), nb, tp, cur_stream());
}

void bn_eval_coeffs(at::Tensor gamma, at::Tensor beta, at::Tensor rmean, at::Tensor rvar, double eps,
                    at::Tensor scale, at::Tensor shift) {
  const int C = gamma.numel();
  TORCH_CHECK(C >= 1, "bn_eval_coeffs: C >= 1");
  for (auto* t : {&gamma, &beta, &rmean, &rvar, &scale, &shift}) {
    need_f32(*t, "bn vec");
    TORCH_CHECK(t->numel() == C && t->device() == gamma.device(),
                "bn_eval_coeffs: six fp32 vectors of C elements on one device");
  }
  const DeviceGuard guard(gamma.device());
  dm::bn_eval_coeffs(fp(gamma), fp(beta), fp(rmean), fp(rvar), eps, C, fp(scale), fp(shift),
                     cur_stream());
}

void bn_apply(at::Tensor y, c10::optional<at::Tensor> res, at::Tensor scale, at::Tensor shift,
              at::Tensor out, bool relu, c10::optional<at::Tensor> mask) {
  need_bf16_nhwc(y, "y");
  need_bf16_nhwc(out, "out");
  const int C = y.size(3);
  dm::ConvGeom cg;  // the kernel takes a chunk's channel as i & (C/8 - 1)
  const char* err = dm::geom_channels(cg, C);
  TORCH_CHECK(!err, err);
  need_f32(scale, "scale", C);
  need_f32(shift, "shift", C);
  const bf* rp = nullptr;
  if (res.has_value()) { need_bf16_nhwc(*res, "res"); TORCH_CHECK(res->sizes() == y.sizes()); rp = bp(*res); }
  TORCH_CHECK(out.sizes() == y.sizes());
  const DeviceGuard guard(y.device());
  uint8_t* mp = nullptr;
  if (mask.has_value()) {
    TORCH_CHECK(relu, "mask: ReLU outputs only");
    mp = relu_mask(mask, y, "mask: contiguous uint8, one byte per 8 channels");
  }
  dm::bn_apply(bp(y), rp, fp(scale), fp(shift), bp(out), y.numel(), C, relu, cur_stream(), mp);
}

// floats of a BatchNorm backward's work tensor: enough for any dz source of an [M][C] operand
int64_t bn_bwd_work(int64_t M, int64_t C) { return dm::bn_bwd_work_floats(dm::bn_bwd_groups(M, C), C); }

// Stem backward without the full-resolution dy: BN-backward coefficients from the pooled-
// domain sums (pre_slab, bn_bwd_reduce_masked), then the fused gather + apply + s2d weight
// gradient (conv_stem.hip) into slab, then the fixed-order reduce into dw [Cout][Cin][7][7].
bool stem_bwd_fused_supported(at::Tensor y, at::Tensor xs) {
  return y.dim() == 4 && xs.dim() == 4 && y.size(0) == xs.size(0) && y.size(1) == xs.size(1) &&
         y.size(2) == xs.size(2) &&
         dm::stem_wgrad_fused_supported(y.size(0), y.size(1), y.size(2), y.size(3), xs.size(3));
}

int64_t stem_bwd_slab_floats(int64_t N, int64_t H) {
  return (int64_t)dm::stem_wgrad_fused_blocks((int)N, (int)H) * 64 * 256;
}

void stem_bwd_fused(at::Tensor y, at::Tensor mean, at::Tensor invstd, at::Tensor gamma,
                    at::Tensor dgamma, at::Tensor dbeta, double gbeta, at::Tensor scale,
                    at::Tensor shift, at::Tensor pdy, at::Tensor pidx, at::Tensor pre_slab,
                    int64_t pre_rows, at::Tensor xs, int64_t Cin, at::Tensor dw, double wbeta,
                    at::Tensor work, at::Tensor slab) {
  need_bf16_nhwc(y, "y");
  need_bf16_nhwc(xs, "xs");
  need_bf16_nhwc(pdy, "pdy");
  TORCH_CHECK(stem_bwd_fused_supported(y, xs), "stem_bwd_fused: unsupported shape");
  const int N = y.size(0), H = y.size(1), W = y.size(2), C = y.size(3);
  TORCH_CHECK(pdy.size(0) == N && pdy.size(1) == H / 2 && pdy.size(2) == W / 2 && pdy.size(3) == C,
              "pdy must be the 3x3/s2/p1 pooled gradient");
  TORCH_CHECK(is_u8(pidx) && pidx.numel() == pdy.numel());
  const long long M = (long long)N * H * W;
  need_f32(work, "work", bn_bwd_work(M, C));
  need_f32(pre_slab, "pre_slab", pre_rows * 2 * C);
  need_f32(scale, "scale", C);
  need_f32(shift, "shift", C);
  need_f32(dw, "dw", (int64_t)C * Cin * 49);
  const int S = dm::stem_wgrad_fused_blocks(N, H);
  need_f32(slab, "slab", (int64_t)S * 64 * 256);
  const DeviceGuard guard(y.device());
  auto st = cur_stream();
  const dm::BnBwdWork w = dm::bn_bwd_carve(fp(work), 0, C);  // pre_slab: no partial rows here
  dm::bn_bwd_finalize(fp(pre_slab), (int)pre_rows, M, C, fp(gamma), fp(mean), fp(invstd),
                      fp(dgamma), fp(dbeta), (float)gbeta, w.coef, w.part2, st);
  dm::stem_wgrad_fused(bp(xs), bp(y), bp(pdy), (const uint8_t*)pidx.data_ptr(), w.coef,
                       fp(scale), fp(shift), fp(slab), N, H, W, S, st);
  dm::wgrad_reduce_s2d(fp(slab), S, C, (int)Cin, xs.size(3), fp(dw), (float)wbeta, st);
}


// mode (dm::BnDz): 0 no ReLU, 1 mask from `out`, 2 mask from y*scale+shift, 3 (stem) dz gathered
// from the following max-pool's gradient (pdy, pidx; pool K/S/P) with mask from y, 4 mask
// from the 1-bit (out > 0) mask that bn_apply wrote in the forward.
void bn_backward(c10::optional<at::Tensor> dout, c10::optional<at::Tensor> out, at::Tensor y,
                 at::Tensor mean, at::Tensor invstd, at::Tensor gamma, at::Tensor dgamma,
                 at::Tensor dbeta, double gbeta, int64_t mode, c10::optional<at::Tensor> scale,
                 c10::optional<at::Tensor> shift, c10::optional<at::Tensor> pdy,
                 c10::optional<at::Tensor> pidx, int64_t K, int64_t S, int64_t P,
                 at::Tensor dy, c10::optional<at::Tensor> dres, at::Tensor work,
                 c10::optional<at::Tensor> pre_slab, int64_t pre_rows,
                 c10::optional<at::Tensor> mask, int64_t stage,
                 c10::optional<at::Tensor> sums, c10::optional<at::Tensor> total) {
  // stage 1 / 2: the two halves of a cross-rank BatchNorm backward (dm::BnStage);
  // sums [2C] float64 is written by stage 1 and read, summed over the ranks, by stage 2
  TORCH_CHECK(stage >= 0 && stage <= 2, "stage: 0 whole, 1 sums, 2 apply");
  const auto stg = (dm::BnStage)stage;
  TORCH_CHECK(stg == dm::BnStage::Whole || sums.has_value(), "stage 1 / 2 need sums");
  double* sums_p = stg != dm::BnStage::Whole ? need_f64(*sums, "sums", 2 * y.size(3)) : nullptr;
  TORCH_CHECK(stg != dm::BnStage::Apply || total.has_value(), "stage 2 needs total");
  const double* total_p = stg == dm::BnStage::Apply ? need_f64(*total, "total", 1) : nullptr;
  need_bf16_nhwc(y, "y");
  need_bf16_nhwc(dy, "dy");
  TORCH_CHECK(dy.sizes() == y.sizes());
  TORCH_CHECK(mode >= 0 && mode <= 4);
  const auto src = (dm::BnDz)mode;
  const int C = y.size(3);
  TORCH_CHECK(C % 8 == 0 && 256 % (C / 8) == 0, "bn_backward: C/8 must divide 256");
  dm::BnBwdArgs a{};
  a.M = y.numel() / C;
  need_f32(work, "work", bn_bwd_work(a.M, C));
  if (pre_slab.has_value()) {
    TORCH_CHECK(pre_rows >= 1, "pre_slab: >= 1 row");
    need_f32(*pre_slab, "pre_slab", pre_rows * 2 * C);
  }
  if (src != dm::BnDz::Pool) {
    TORCH_CHECK(dout.has_value());
    need_bf16_nhwc(*dout, "dout");
    TORCH_CHECK(dout->sizes() == y.sizes());
    a.dout = bp(*dout);
  }
  if (src == dm::BnDz::OutMask) {
    TORCH_CHECK(out.has_value());
    need_bf16_nhwc(*out, "out");
    TORCH_CHECK(out->sizes() == y.sizes());
    a.out = bp(*out);
  }
  if (src == dm::BnDz::YMask || src == dm::BnDz::Pool) {
    TORCH_CHECK(scale.has_value() && shift.has_value());
    need_f32(*scale, "scale", C);
    need_f32(*shift, "shift", C);
    a.scale = fp(*scale); a.shift = fp(*shift);
  }
  if (src == dm::BnDz::Pool) {
    TORCH_CHECK(pdy.has_value() && pidx.has_value());
    need_bf16_nhwc(*pdy, "pdy");
    TORCH_CHECK(pidx->scalar_type() == at::kByte && pidx->numel() == pdy->numel());
    TORCH_CHECK(pdy->size(0) == y.size(0) && pdy->size(3) == C);
    a.OH = pdy->size(1); a.OW = pdy->size(2);
    TORCH_CHECK(a.OH == (y.size(1) + 2 * P - K) / S + 1 && a.OW == (y.size(2) + 2 * P - K) / S + 1);
    a.pdy = bp(*pdy); a.pidx = (const uint8_t*)pidx->data_ptr();
  }
  if (src == dm::BnDz::BitMask) a.mask = relu_mask(mask, y, "mode 4 needs the uint8 mask");
  bf* drp = nullptr;
  if (dres.has_value()) {
    need_bf16_nhwc(*dres, "dres");
    TORCH_CHECK(dres->sizes() == y.sizes(), "dres: the shape of y");
    drp = bp(*dres);
  }
  a.y = bp(y); a.mean = fp(mean); a.invstd = fp(invstd);
  a.H = y.size(1); a.W = y.size(2); a.K = K; a.S = S; a.P = P; a.C = C;
  const DeviceGuard guard(y.device());
  auto st = cur_stream();
  float *gm = fp(gamma), *dg = fp(dgamma), *db = fp(dbeta);
  // the partial rows are the reduce's own unless a producing kernel left them (pre_slab) or,
  // in stage 2, the sums of all ranks replace them
  const bool reduce = !pre_slab.has_value() && stg != dm::BnStage::Apply;
  const dm::BnBwdWork w =
      dm::bn_bwd_carve(fp(work), reduce ? dm::bn_bwd_rows(src, a, drp != nullptr) : 0, C);
  if (stg == dm::BnStage::Apply) {
    dm::bn_bwd_coef(sums_p, total_p, gm, a.mean, a.invstd, C, w.coef, st);
  } else {
    const float* part = reduce ? w.part : fp(*pre_slab);
    const int rows = reduce ? dm::bn_bwd_reduce(src, a, drp != nullptr, w.part, st) : (int)pre_rows;
    if (stg == dm::BnStage::Sums)
      return dm::bn_bwd_sums(part, rows, C, dg, db, (float)gbeta, sums_p, w.part2, st);
    dm::bn_bwd_finalize(part, rows, a.M, C, gm, a.mean, a.invstd, dg, db, (float)gbeta, w.coef,
                        w.part2, st);
  }
  dm::bn_bwd_apply(src, a, w.coef, bp(dy), drp, st);
}

// Stage "sums" of a coefficient-only BatchNorm backward (the fused stem): dgamma / dbeta from
// this rank's pre-reduced partial rows, sums [2C] float64 out
void bn_bwd_sums(at::Tensor pre_slab, int64_t pre_rows, int64_t C, at::Tensor dgamma,
                 at::Tensor dbeta, double gbeta, at::Tensor work, at::Tensor sums) {
  TORCH_CHECK(pre_rows >= 1 && C >= 1, "bn_bwd_sums: >= 1 row");
  need_f32(pre_slab, "pre_slab", pre_rows * 2 * C);
  need_f32(dgamma, "dgamma", C);
  need_f32(dbeta, "dbeta", C);
  need_f32(work, "work", dm::bn_bwd_work_floats(0, C));
  double* sp = need_f64(sums, "sums", 2 * C);
  const DeviceGuard guard(pre_slab.device());
  dm::bn_bwd_sums(fp(pre_slab), (int)pre_rows, (int)C, fp(dgamma), fp(dbeta), (float)gbeta, sp,
                  dm::bn_bwd_carve(fp(work), 0, C).part2, cur_stream());
}

void bn_relu_maxpool(at::Tensor y, at::Tensor scale, at::Tensor shift, at::Tensor out,
                     at::Tensor idx, int64_t K, int64_t S, int64_t P,
                     c10::optional<at::Tensor> yarg) {
  need_bf16_nhwc(y, "y");
  need_bf16_nhwc(out, "out");
  const int C = y.size(3);
  need_f32(scale, "scale", C);
  need_f32(shift, "shift", C);
  TORCH_CHECK(idx.scalar_type() == at::kByte && idx.numel() == out.numel());
  TORCH_CHECK(out.size(1) == (y.size(1) + 2 * P - K) / S + 1 && out.size(2) == (y.size(2) + 2 * P - K) / S + 1);
  const DeviceGuard guard(y.device());
  bf* yargp = nullptr;
  if (yarg.has_value()) {
    need_bf16_nhwc(*yarg, "yarg");
    TORCH_CHECK(yarg->sizes() == out.sizes(), "yarg: pooled shape");
    yargp = bp(*yarg);
  }
  dm::bn_relu_maxpool(bp(y), fp(scale), fp(shift), bp(out), (uint8_t*)idx.data_ptr(), y.size(0),
                      y.size(1), y.size(2), C, out.size(1), out.size(2), K, S, P, cur_stream(),
                      yargp);
}

int64_t bn_bwd_rows(int64_t M, int64_t C) { return dm::bn_bwd_groups(M, C); }

// Σdz, Σdz·x̂ partials of (dout masked by y*scale+shift > 0) -> part [rows][2C]; returns rows
int64_t bn_bwd_reduce_masked(at::Tensor dout, at::Tensor y, at::Tensor mean, at::Tensor invstd,
                             at::Tensor scale, at::Tensor shift, at::Tensor part) {
  need_bf16_nhwc(dout, "dout");
  need_bf16_nhwc(y, "y");
  TORCH_CHECK(dout.sizes() == y.sizes());
  const int C = y.size(3);
  TORCH_CHECK(C % 8 == 0 && 256 % (C / 8) == 0, "C/8 must divide 256");
  need_f32(mean, "mean", C);
  need_f32(invstd, "invstd", C);
  need_f32(scale, "scale", C);
  need_f32(shift, "shift", C);
  dm::BnBwdArgs a{};
  a.dout = bp(dout); a.y = bp(y); a.mean = fp(mean); a.invstd = fp(invstd);
  a.scale = fp(scale); a.shift = fp(shift); a.M = y.numel() / C; a.C = C;
  need_f32(part, "part", (int64_t)dm::bn_bwd_rows(dm::BnDz::YMask, a, false) * 2 * C);
  const DeviceGuard guard(y.device());
  return dm::bn_bwd_reduce(dm::BnDz::YMask, a, false, fp(part), cur_stream());
}

// ------------------------------------------------------------------ pooling / packing
// x [N][H][W][C] and its KxK / stride S / pad P pooled tensor y, with the argmax codes idx
// (kh*K + kw in one byte; 15 is the fused stem tail's "no gradient" code)
void need_maxpool(const at::Tensor& x, const at::Tensor& y, const at::Tensor& idx, int64_t K,
                  int64_t S, int64_t P) {
  TORCH_CHECK(K >= 1 && S >= 1 && P >= 0 && 2 * P <= K && K * K <= 255,
              "max pool: K, S >= 1, 0 <= 2P <= K, K*K <= 255");
  TORCH_CHECK(x.size(1) + 2 * P >= K && x.size(2) + 2 * P >= K, "max pool: window larger than input");
  TORCH_CHECK(y.size(0) == x.size(0) && y.size(3) == x.size(3), "max pool: N and C must agree");
  TORCH_CHECK(y.size(1) == (x.size(1) + 2 * P - K) / S + 1 &&
              y.size(2) == (x.size(2) + 2 * P - K) / S + 1,
              "max pool: the pooled extent must be (H + 2P - K) / S + 1");
  TORCH_CHECK(y.device() == x.device() && idx.device() == x.device(), "max pool: one device");
  TORCH_CHECK(idx.is_cuda() && idx.scalar_type() == at::kByte && idx.is_contiguous() &&
              idx.numel() == y.numel(), "idx: contiguous uint8, one code per pooled element");
  TORCH_CHECK((reinterpret_cast<uintptr_t>(idx.data_ptr()) & 7) == 0, "idx must be 8-B aligned");
}

void maxpool_fwd(at::Tensor x, at::Tensor y, at::Tensor idx, int64_t K, int64_t S, int64_t P) {
  need_bf16_nhwc(x, "x");
  need_bf16_nhwc(y, "y");
  need_maxpool(x, y, idx, K, S, P);
  const DeviceGuard guard(x.device());
  dm::maxpool_fwd(bp(x), bp(y), (uint8_t*)idx.data_ptr(), x.size(0), x.size(1), x.size(2), x.size(3),
                  y.size(1), y.size(2), K, S, P, cur_stream());
}

void maxpool_bwd(at::Tensor dy, at::Tensor idx, at::Tensor dx, int64_t K, int64_t S, int64_t P) {
  need_bf16_nhwc(dy, "dy");
  need_bf16_nhwc(dx, "dx");
  need_maxpool(dx, dy, idx, K, S, P);
  const DeviceGuard guard(dy.device());
  dm::maxpool_bwd(bp(dy), (const uint8_t*)idx.data_ptr(), bp(dx), dx.size(0), dx.size(1), dx.size(2),
                  dx.size(3), dy.size(1), dy.size(2), K, S, P, cur_stream());
}

void avgpool_fwd(at::Tensor x, at::Tensor y) {
  need_bf16_nhwc(x, "x");
  TORCH_CHECK(y.scalar_type() == at::kBFloat16 && y.numel() == x.size(0) * x.size(3));
  TORCH_CHECK(y.is_cuda() && y.is_contiguous() && y.device() == x.device(),
              "avgpool_fwd: y must be contiguous and on x's device");
  TORCH_CHECK((reinterpret_cast<uintptr_t>(y.data_ptr()) & 15) == 0, "y must be 16-B aligned");
  const DeviceGuard guard(x.device());
  dm::avgpool_fwd(bp(x), bp(y), x.size(0), x.size(1) * x.size(2), x.size(3), cur_stream());
}

void avgpool_bwd(at::Tensor dy, at::Tensor dx) {
  need_bf16_nhwc(dx, "dx");
  TORCH_CHECK(dy.scalar_type() == at::kBFloat16 && dy.is_contiguous() && dy.numel() == dx.size(0) * dx.size(3));
  TORCH_CHECK(dy.is_cuda() && dy.device() == dx.device(), "avgpool_bwd: dy must be on dx's device");
  TORCH_CHECK((reinterpret_cast<uintptr_t>(dy.data_ptr()) & 15) == 0, "dy must be 16-B aligned");
  const DeviceGuard guard(dx.device());
  dm::avgpool_bwd(bp(dy), bp(dx), dx.size(0), dx.size(1) * dx.size(2), dx.size(3), cur_stream());
}

void pack_input(at::Tensor x, at::Tensor y) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4);
  TORCH_CHECK(x.scalar_type() == at::kFloat || x.scalar_type() == at::kBFloat16);
  need_bf16_nhwc(y, "y");
  TORCH_CHECK(y.size(0) == x.size(0) && y.size(1) == x.size(2) && y.size(2) == x.size(3) &&
              y.size(3) >= x.size(1));
  const DeviceGuard guard(x.device());
  dm::pack_input(x.data_ptr(), x.scalar_type() == at::kBFloat16, bp(y), x.size(0), x.size(1),
                 x.size(2), x.size(3), y.size(3), x.stride(0), x.stride(1), x.stride(2), x.stride(3),
                 cur_stream());
}

}  // namespace

// ----------------------------------------------------------------- fused K-dense stem
// img: the raw input as stored -- (N, 3, H, W) channels_last or (N, H, W, 3) contiguous, fp32 /
// bf16 / u8; idx (optional int64 [B]): batch row -> image row (the loader's gather)
struct ImgView {
  const void* ptr;
  int dtype, N, H, W;
};
ImgView img_view(const at::Tensor& img) {
  TORCH_CHECK(img.is_cuda() && img.dim() == 4, "stem input must be a 4-D HIP tensor");
  ImgView v{img.data_ptr(), 0, (int)img.size(0), 0, 0};
  if (img.size(1) == 3 && img.size(3) != 3) {
    TORCH_CHECK(img.is_contiguous(at::MemoryFormat::ChannelsLast),
                "stem input (N,3,H,W) must be channels_last");
    v.H = img.size(2);
    v.W = img.size(3);
  } else {
    TORCH_CHECK(img.size(3) == 3 && img.is_contiguous(), "stem input (N,H,W,3) must be contiguous");
    v.H = img.size(1);
    v.W = img.size(2);
  }
  const auto t = img.scalar_type();
  TORCH_CHECK(t == at::kFloat || t == at::kBFloat16 || t == at::kByte,
              "stem input must be fp32, bf16 or uint8");
  v.dtype = t == at::kFloat ? 0 : t == at::kBFloat16 ? 1 : 2;
  return v;
}

bool stem_fused_supported(int64_t Hin, int64_t Win) { return dm::stem_fused_supported(Hin, Win); }
int64_t stem_fused_grid(int64_t N) { return dm::stem_fused_grid((int)N); }
// floats of the backward's slab workspace for `grid` workgroups: D and G partials + their sums
int64_t stem_bwd_slab_len(int64_t grid) {
  const int64_t gk = dm::stem_gram_cols();
  return grid * (64 * dm::stem_slab_cols() + gk * gk) + dm::stem_sums_len();
}

const long long* idx_ptr(const c10::optional<at::Tensor>& idx, int B, int Nimg) {
  if (!idx.has_value()) {
    TORCH_CHECK(B <= Nimg, "stem: batch larger than the image tensor");
    return nullptr;
  }
  TORCH_CHECK(idx->is_cuda() && idx->scalar_type() == at::kLong && idx->is_contiguous() &&
                  idx->numel() == B, "stem: idx must be a contiguous int64 HIP tensor of B rows");
  return reinterpret_cast<const long long*>(idx->data_ptr());
}

void stem_fwd_fused(at::Tensor img, c10::optional<at::Tensor> idx, std::vector<double> nsc,
                    std::vector<double> nbi, at::Tensor wk, at::Tensor gamma, at::Tensor pext,
                    at::Tensor code, c10::optional<at::Tensor> stats, int64_t grid) {
  const ImgView v = img_view(img);
  TORCH_CHECK(dm::stem_fused_supported(v.H, v.W), "fused stem: unsupported input size");
  need_bf16_nhwc(pext, "pext");
  const int B = pext.size(0);
  TORCH_CHECK(pext.size(1) == v.H / 4 && pext.size(2) == v.W / 4 && pext.size(3) == 64,
              "pext must be [B, H/4, W/4, 64]");
  TORCH_CHECK(code.is_cuda() && code.scalar_type() == at::kByte && code.is_contiguous() &&
              code.numel() * 2 == pext.numel(), "code must be uint8 [N][PH][PW][32] (4-bit codes)");
  TORCH_CHECK(wk.is_cuda() && wk.scalar_type() == at::kBFloat16 && wk.is_contiguous() &&
              wk.numel() == 64 * dm::stem_wk_cols(), "wk must be packed [64][176] bf16");
  need_f32(gamma, "gamma", 64);
  TORCH_CHECK(nsc.size() == 3 && nbi.size() == 3, "3 normalisation scales / biases");
  TORCH_CHECK(grid >= 1 && grid <= B, "grid must be in [1, B]");
  if (stats.has_value()) need_f32(*stats, "stats", grid * 128);
  const float s3[3] = {(float)nsc[0], (float)nsc[1], (float)nsc[2]};
  const float b3[3] = {(float)nbi[0], (float)nbi[1], (float)nbi[2]};
  const DeviceGuard guard(pext.device());
  dm::stem_fwd_fused(v.ptr, v.dtype, idx_ptr(idx, B, v.N), s3, b3, bp(wk), fp(gamma), bp(pext),
                     (uint8_t*)code.data_ptr(), stats ? fp(*stats) : nullptr, B, v.N, v.H, v.W,
                     (int)grid, cur_stream());
}

// out = relu(scale * pext + shift); with code4: the backward's 4-bit window codes (15 where
// the output is 0) from the forward's byte codes
void stem_pool_apply(at::Tensor pext, c10::optional<at::Tensor> code, at::Tensor scale,
                     at::Tensor shift, at::Tensor out, c10::optional<at::Tensor> code4) {
  need_bf16_nhwc(pext, "pext");
  need_bf16_nhwc(out, "out");
  TORCH_CHECK(out.numel() == pext.numel() && pext.size(3) == 64, "pooled shapes");
  TORCH_CHECK(code.has_value() == code4.has_value(), "code and code4 go together");
  if (code.has_value()) {
    TORCH_CHECK(code->is_cuda() && code->scalar_type() == at::kByte && code->is_contiguous() &&
                    code->numel() * 2 == pext.numel(), "code must be uint8 [N][PH][PW][32]");
    TORCH_CHECK(code4->is_cuda() && code4->scalar_type() == at::kByte && code4->is_contiguous() &&
                    code4->numel() * 2 == pext.numel(), "code4 must be uint8 [N][PH][PW][32]");
  }
  need_f32(scale, "scale", 64);
  need_f32(shift, "shift", 64);
  const DeviceGuard guard(pext.device());
  dm::stem_pool_apply(bp(pext), code ? (const uint8_t*)code->data_ptr() : nullptr, fp(scale),
                      fp(shift), bp(out), code4 ? (uint8_t*)code4->data_ptr() : nullptr,
                      pext.numel(), cur_stream());
}

// BN-backward coefficients (a, b, cc) from the pooled-domain sums (pre_slab); the per-workgroup
// D = dz^T X and G = X^T X partials into dslab; dW = beta dW + a D + b W G + cc colsum(X)
void stem_bwd_fused2(at::Tensor img, c10::optional<at::Tensor> idx, std::vector<double> nsc,
                     std::vector<double> nbi, at::Tensor wk, at::Tensor pdy, at::Tensor code4,
                     at::Tensor mean, at::Tensor invstd, at::Tensor gamma, at::Tensor dgamma,
                     at::Tensor dbeta, double gbeta, at::Tensor pre_slab, int64_t pre_rows,
                     at::Tensor dw, double wbeta, at::Tensor work, at::Tensor dslab, int64_t grid,
                     c10::optional<at::Tensor> bn_sums, c10::optional<at::Tensor> bn_total) {
  // bn_sums + bn_total (cross-rank BatchNorm): the coefficients come from the global sums
  // (dm::bn_bwd_coef); dgamma / dbeta were written by bn_bwd_sums and stay untouched
  TORCH_CHECK(bn_sums.has_value() == bn_total.has_value(), "sums and total: both or neither");
  const ImgView v = img_view(img);
  TORCH_CHECK(dm::stem_fused_supported(v.H, v.W), "fused stem: unsupported input size");
  need_bf16_nhwc(pdy, "pdy");
  const int B = pdy.size(0), C = 64;
  TORCH_CHECK(pdy.size(1) == v.H / 4 && pdy.size(2) == v.W / 4 && pdy.size(3) == C, "pdy shape");
  TORCH_CHECK(code4.is_cuda() && code4.scalar_type() == at::kByte && code4.is_contiguous() &&
                  code4.numel() * 2 == pdy.numel(), "code4 must be uint8 [N][PH][PW][32]");
  const long long M = (long long)B * (v.H / 2) * (v.W / 2);
  need_f32(work, "work", bn_bwd_work(M, C));
  need_f32(pre_slab, "pre_slab", pre_rows * 2 * C);
  need_f32(dw, "dw", (int64_t)C * 3 * 49);
  TORCH_CHECK(wk.is_cuda() && wk.scalar_type() == at::kBFloat16 && wk.is_contiguous() &&
              wk.numel() == 64 * dm::stem_wk_cols(), "wk must be packed [64][176] bf16");
  TORCH_CHECK(grid >= 1 && grid <= B, "grid must be in [1, B]");
  need_f32(dslab, "dslab", stem_bwd_slab_len(grid));
  const float s3[3] = {(float)nsc[0], (float)nsc[1], (float)nsc[2]};
  const float b3[3] = {(float)nbi[0], (float)nbi[1], (float)nbi[2]};
  const DeviceGuard guard(pdy.device());
  auto st = cur_stream();
  // the coefficients (a, b, cc) only: the kernels below apply them
  const dm::BnBwdWork w = dm::bn_bwd_carve(fp(work), 0, C);  // pre_slab: no partial rows here
  if (bn_sums.has_value())
    dm::bn_bwd_coef(need_f64(*bn_sums, "sums", 2 * C), need_f64(*bn_total, "total", 1), fp(gamma),
                    fp(mean), fp(invstd), C, w.coef, st);
  else
    dm::bn_bwd_finalize(fp(pre_slab), (int)pre_rows, M, C, fp(gamma), fp(mean), fp(invstd),
                        fp(dgamma), fp(dbeta), (float)gbeta, w.coef, w.part2, st);
  float* d_part = fp(dslab);
  float* g_part = d_part + grid * C * dm::stem_slab_cols();
  float* sums = g_part + grid * dm::stem_gram_cols() * dm::stem_gram_cols();
  dm::stem_bwd_fused2(v.ptr, v.dtype, idx_ptr(idx, B, v.N), s3, b3, bp(wk), bp(pdy),
                      (const uint8_t*)code4.data_ptr(), d_part, g_part, B, v.N, v.H, v.W,
                      (int)grid, st);
  dm::stem_wcombine(d_part, g_part, (int)grid, bp(wk), w.coef, sums, fp(dw), (float)wbeta, st);
}

void stem_pack_weights(at::Tensor w, at::Tensor wk) {
  need_f32(w, "w", 64 * 3 * 49);
  TORCH_CHECK(w.dim() == 4 && w.size(0) == 64 && w.size(1) == 3 && w.size(2) == 7 && w.size(3) == 7,
              "stem weight must be [64][3][7][7]");
  TORCH_CHECK(wk.scalar_type() == at::kBFloat16 && wk.numel() == 64 * dm::stem_wk_cols(), "wk");
  const DeviceGuard guard(w.device());
  dm::stem_pack_weights(fp(w), bp(wk), cur_stream());
}

// a row of csrc/conv_cfg.h as a dict; None for an id the table does not have
template <class Row>
py::object cfg_dict(const Row* c) {
  if (!c) return py::none();
  py::dict d;
  dm::cfg_fields(*c, [&](const char* k, auto v) { d[k] = v; });
  return d;
}
py::object conv_cfg_info(int64_t cfg) { return cfg_dict(dm::conv_cfg((int)cfg)); }
py::object wgrad_cfg_info(int64_t cfg) { return cfg_dict(dm::wgrad_cfg((int)cfg)); }

// The kernel a conv over x [N,H,W,C] -> y [.,.,.,Cout] with these operands would run on, as
// (family, tile, ok): a dry run of the launch entry point, operands standing in for the flags;
// ok = false: the call is refused.  dgrad: the data gradient; stride 2: the parity classes'
// launch (tile 0 = one launch per class; `add` plays no part; `merged` = with a projection of
// dy's own channel count, another count cannot be asked for here); otherwise the forward
py::tuple conv_route_info(int64_t N, int64_t H, int64_t W, int64_t C, int64_t Cout, int64_t k,
                          int64_t stride, int64_t pad, int64_t cfg, bool add, bool pre, bool red,
                          bool dgrad, bool merged) {
  const int OH = (H + 2 * pad - k) / stride + 1, OW = (W + 2 * pad - k) / stride + 1;
  dm::ConvGeom g;
  const char* err = dgrad ? dm::dgrad_base_geom(g, N, OH, OW, Cout, H, W, C, k, k)
                          : dm::conv_fwd_geom(g, N, H, W, C, Cout, k, k, stride, pad, OH, OW);
  TORCH_CHECK(!err, err);
  const bf b{};
  const float f{};
  const dm::BnBwdRed rd{};
  const dm::DgradSeg2 s2{nullptr, nullptr, 0, 0, g.C, 0};
  const dm::ConvOperands ops{nullptr, nullptr, nullptr, dm::kPipeAuto, add ? &b : nullptr, nullptr,
                             pre ? &f : nullptr, pre ? &f : nullptr, red ? &rd : nullptr,
                             merged ? &s2 : nullptr};
  dm::ConvRoute r{};
  dm::ConvGeomSet set{};
  bool any_empty;
  const int ng = dgrad ? dm::dgrad_classes(g, k, k, stride, pad, set, any_empty) : 0;
  if (dgrad && stride == 2) dm::conv_launch_multi(ops, set, ng, cfg_of(cfg), nullptr, &r);
  else dm::conv_launch(ops, dgrad ? set.g[0] : g, cfg_of(cfg), nullptr, &r);
  return py::make_tuple(dm::family_name(r.kernel), r.tile, r.ok);
}
py::tuple wgrad_route_info(int64_t N, int64_t H, int64_t W, int64_t C, int64_t Cout, int64_t k,
                           int64_t stride, int64_t pad, int64_t cfg, bool pre) {
  const int OH = (H + 2 * pad - k) / stride + 1, OW = (W + 2 * pad - k) / stride + 1;
  const float f{};
  dm::WgradRoute r{};
  dm::wgrad_launch({nullptr, nullptr, nullptr, 1, 64, pre ? &f : nullptr, pre ? &f : nullptr},
                   fwd_geom(N, H, W, C, Cout, k, k, stride, pad, OH, OW), wgrad_cfg_of(cfg), nullptr, &r);
  return py::make_tuple(dm::family_name(r.kernel), r.tile, r.ok);
}

void register_resnet(pybind11::module_& m) {
  m.def("conv_fwd", &conv_fwd, py::arg("x"), py::arg("wpack"), py::arg("y"), py::arg("stats"),
        py::arg("add"), py::arg("KH"), py::arg("KW"), py::arg("stride"), py::arg("pad"),
        py::arg("cfg"), py::arg("pre_scale") = py::none(), py::arg("pre_shift") = py::none(),
        py::arg("balance") = "auto");
  dm::conv_pipe_set_workspace(&pipe_workspace);
  m.def("conv_pipe_balance_state", &conv_pipe_balance_state);
  // ncols: unused; still accepted from the callers that pass it
  m.def("conv_stats_rows", [](int64_t M, int64_t cfg, int64_t) { return conv_stats_rows(M, cfg); },
        py::arg("M"), py::arg("cfg"), py::arg("ncols") = -1);
  m.def("conv_cfg_info", &conv_cfg_info, py::arg("cfg"));
  m.def("wgrad_cfg_info", &wgrad_cfg_info, py::arg("cfg"));
  m.def("conv_route_info", &conv_route_info, py::arg("N"), py::arg("H"), py::arg("W"), py::arg("C"),
        py::arg("Cout"), py::arg("k"), py::arg("stride"), py::arg("pad"), py::arg("cfg"),
        py::arg("add") = false, py::arg("pre") = false, py::arg("red") = false,
        py::arg("dgrad") = false, py::arg("merged") = false);
  m.def("wgrad_route_info", &wgrad_route_info, py::arg("N"), py::arg("H"), py::arg("W"),
        py::arg("C"), py::arg("Cout"), py::arg("k"), py::arg("stride"), py::arg("pad"),
        py::arg("cfg"), py::arg("pre") = false);
  m.def("conv_dgrad", &conv_dgrad, py::arg("dy"), py::arg("wd"), py::arg("dx"), py::arg("KH"),
        py::arg("KW"), py::arg("stride"), py::arg("pad"),
        py::arg("add") = py::none(), py::arg("cfg") = 12, py::arg("add_mask") = py::none(),
        py::arg("red_y") = py::none(), py::arg("red_scale") = py::none(),
        py::arg("red_shift") = py::none(), py::arg("red_mean") = py::none(),
        py::arg("red_invstd") = py::none(), py::arg("red_part") = py::none(),
        py::arg("red_mask") = py::none(), py::arg("dy2") = py::none(),
        py::arg("wd2") = py::none(), py::arg("balance") = "auto");
  m.def("dgrad_s2_red_rows", &dgrad_s2_red_rows, py::arg("N"), py::arg("H"), py::arg("W"),
        py::arg("cfg"));
  m.def("conv_wgrad", &conv_wgrad, py::arg("x"), py::arg("dy"), py::arg("dw"), py::arg("slab"),
        py::arg("Cin"), py::arg("KH"), py::arg("KW"), py::arg("stride"), py::arg("pad"),
        py::arg("beta"), py::arg("S"), py::arg("cfg"), py::arg("s2d"),
        py::arg("pre_scale") = py::none(), py::arg("pre_shift") = py::none());
  m.def("pack_weights", &pack_weights);
  m.def("pack_weights_tiled", &pack_weights_tiled);
  m.def("bn_stats_finalize", &bn_stats_finalize, py::arg("stats"), py::arg("T"), py::arg("count"),
        py::arg("gamma"), py::arg("beta"), py::arg("rmean"), py::arg("rvar"), py::arg("momentum"),
        py::arg("eps"), py::arg("scale"), py::arg("shift"), py::arg("mean"), py::arg("invstd"),
        py::arg("work"), py::arg("num_batches") = py::none());
  m.def("bn_eval_coeffs", &bn_eval_coeffs);
  m.def("bn_apply", &bn_apply, py::arg("y"), py::arg("res"), py::arg("scale"), py::arg("shift"),
        py::arg("out"), py::arg("relu"), py::arg("mask") = py::none());
  m.def("bn_bwd_work", &bn_bwd_work);
  m.def("stem_bwd_fused_supported", &stem_bwd_fused_supported);
  m.def("stem_bwd_slab_floats", &stem_bwd_slab_floats);
  m.def("stem_bwd_fused", &stem_bwd_fused, py::arg("y"), py::arg("mean"), py::arg("invstd"),
        py::arg("gamma"), py::arg("dgamma"), py::arg("dbeta"), py::arg("gbeta"), py::arg("scale"),
        py::arg("shift"), py::arg("pdy"), py::arg("pidx"), py::arg("pre_slab"), py::arg("pre_rows"),
        py::arg("xs"), py::arg("Cin"), py::arg("dw"), py::arg("wbeta"), py::arg("work"),
        py::arg("slab"));
  m.def("bn_backward", &bn_backward, py::arg("dout"), py::arg("out"), py::arg("y"), py::arg("mean"), py::arg("invstd"), py::arg("gamma"), py::arg("dgamma"), py::arg("dbeta"), py::arg("gbeta"), py::arg("mode"), py::arg("scale"), py::arg("shift"), py::arg("pdy"), py::arg("pidx"), py::arg("K"), py::arg("S"), py::arg("P"), py::arg("dy"), py::arg("dres"), py::arg("work"),
        py::arg("pre_slab") = py::none(), py::arg("pre_rows") = 0, py::arg("mask") = py::none(),
        py::arg("stage") = 0, py::arg("sums") = py::none(), py::arg("total") = py::none());
  m.def("bn_bwd_sums", &bn_bwd_sums, py::arg("pre_slab"), py::arg("pre_rows"), py::arg("C"),
        py::arg("dgamma"), py::arg("dbeta"), py::arg("gbeta"), py::arg("work"), py::arg("sums"));
  m.def("bn_sync_local", &bn_sync_local, py::arg("stats"), py::arg("T"), py::arg("count"),
        py::arg("C"), py::arg("row"), py::arg("work"));
  m.def("bn_sync_finalize", &bn_sync_finalize, py::arg("rows"), py::arg("gamma"), py::arg("beta"),
        py::arg("rmean"), py::arg("rvar"), py::arg("momentum"), py::arg("eps"), py::arg("scale"),
        py::arg("shift"), py::arg("mean"), py::arg("invstd"), py::arg("num_batches"),
        py::arg("total"));
  m.def("bn_relu_maxpool", &bn_relu_maxpool, py::arg("y"), py::arg("scale"), py::arg("shift"),
        py::arg("out"), py::arg("idx"), py::arg("K"), py::arg("S"), py::arg("P"),
        py::arg("yarg") = py::none());
  m.def("bn_bwd_rows", &bn_bwd_rows);
  m.def("bn_bwd_reduce_masked", &bn_bwd_reduce_masked);
  m.def("maxpool_fwd", &maxpool_fwd);
  m.def("maxpool_bwd", &maxpool_bwd);
  m.def("avgpool_fwd", &avgpool_fwd);
  m.def("avgpool_bwd", &avgpool_bwd);
  m.def("pack_input", &pack_input);
  m.def("pack_input_s2d", &pack_input_s2d, py::arg("x"), py::arg("y"),
        py::arg("idx") = py::none());
  m.def("pack_weights_s2d", &pack_weights_s2d);
  m.def("stem_fused_supported", &stem_fused_supported);
  m.def("stem_fused_grid", &stem_fused_grid);
  m.def("stem_bwd_slab_len", &stem_bwd_slab_len);
  m.def("stem_fwd_fused", &stem_fwd_fused, py::arg("img"), py::arg("idx"), py::arg("nsc"),
        py::arg("nbi"), py::arg("wk"), py::arg("gamma"), py::arg("pext"), py::arg("code"),
        py::arg("stats"), py::arg("grid"));
  m.def("stem_pool_apply", &stem_pool_apply, py::arg("pext"), py::arg("code"), py::arg("scale"),
        py::arg("shift"), py::arg("out"), py::arg("code4") = py::none());
  m.def("stem_bwd_fused2", &stem_bwd_fused2, py::arg("img"), py::arg("idx"), py::arg("nsc"),
        py::arg("nbi"), py::arg("wk"), py::arg("pdy"), py::arg("code4"), py::arg("mean"),
        py::arg("invstd"), py::arg("gamma"), py::arg("dgamma"), py::arg("dbeta"),
        py::arg("gbeta"), py::arg("pre_slab"), py::arg("pre_rows"), py::arg("dw"),
        py::arg("wbeta"), py::arg("work"), py::arg("dslab"), py::arg("grid"),
        py::arg("sums") = py::none(), py::arg("total") = py::none());
  m.def("stem_pack_weights", &stem_pack_weights);
}
