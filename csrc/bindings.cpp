// Python bindings for the dmlab HIP kernels (module dmlab._C).
// Each binding validates shapes/dtypes on the host, then launches on the
// current PyTorch HIP stream so kernels compose with RCCL/torch streams and
// hipGraph capture.
#include <torch/extension.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

#include "kernels.h"

namespace {

inline hipStream_t cur_stream() {
  return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
}
using DeviceGuard = c10::hip::HIPGuardMasqueradingAsCUDA;

#define CHECK_CUDA(t) TORCH_CHECK((t).is_cuda(), #t " must be a HIP device tensor")
#define CHECK_CONTIG(t) TORCH_CHECK((t).is_contiguous(), #t " must be contiguous")
#define CHECK_F32(t) TORCH_CHECK((t).scalar_type() == at::kFloat, #t " must be float32")
#define CHECK_BF16(t) TORCH_CHECK((t).scalar_type() == at::kBFloat16, #t " must be bfloat16")
#define CHECK_ALIGN16(t) \
  TORCH_CHECK((reinterpret_cast<uintptr_t>((t).data_ptr()) & 15) == 0, #t " must be 16-B aligned")

inline dm::bf16_t* bfp(const at::Tensor& t) {
  return reinterpret_cast<dm::bf16_t*>(t.data_ptr());
}
inline dm::bf16_t* opt_bfp(const c10::optional<at::Tensor>& t) {
  if (!t.has_value() || !t->defined()) return nullptr;
  CHECK_CUDA(*t);
  CHECK_BF16(*t);
  CHECK_ALIGN16(*t);
  return bfp(*t);
}

void sgd_step(at::Tensor p, at::Tensor g, c10::optional<at::Tensor> mom,
              c10::optional<at::Tensor> pbf, double lr, double momentum, double dampening,
              double wd, double gscale, bool nesterov, bool first) {
  CHECK_CUDA(p); CHECK_CUDA(g); CHECK_F32(p); CHECK_F32(g);
  CHECK_CONTIG(p); CHECK_CONTIG(g);
  TORCH_CHECK(p.numel() == g.numel(), "param/grad size mismatch");
  float* mp = nullptr;
  if (momentum != 0.0) {
    TORCH_CHECK(mom.has_value() && mom->defined(), "momentum buffer required");
    CHECK_CUDA(*mom); CHECK_F32(*mom);
    TORCH_CHECK(mom->numel() == p.numel(), "momentum size mismatch");
    mp = mom->data_ptr<float>();
  }
  dm::bf16_t* pb = opt_bfp(pbf);
  if (pb) TORCH_CHECK(pbf->numel() == p.numel(), "bf16 shadow size mismatch");
  const DeviceGuard guard(p.device());
  dm::sgd_step(p.data_ptr<float>(), g.data_ptr<float>(), mp, pb, p.numel(), (float)lr,
               (float)momentum, (float)dampening, (float)wd, (float)gscale, nesterov, first,
               cur_stream());
}

void adam_step(at::Tensor p, at::Tensor g, at::Tensor m, at::Tensor v,
               c10::optional<at::Tensor> pbf, double lr, double b1, double b2, double eps,
               double wd, double gscale, double bc1, double bc2) {
  for (auto* t : {&p, &g, &m, &v}) {
    CHECK_CUDA(*t); CHECK_F32(*t); CHECK_CONTIG(*t); CHECK_ALIGN16(*t);
    TORCH_CHECK(t->numel() == p.numel(), "adam buffer size mismatch");
  }
  dm::bf16_t* pb = opt_bfp(pbf);
  const DeviceGuard guard(p.device());
  dm::adam_step(p.data_ptr<float>(), g.data_ptr<float>(), m.data_ptr<float>(),
                v.data_ptr<float>(), pb, p.numel(), (float)lr, (float)b1, (float)b2,
                (float)eps, (float)wd, (float)gscale, (float)bc1, (float)bc2, cur_stream());
}

void cast_f32_bf16(at::Tensor x, at::Tensor y) {
  CHECK_CUDA(x); CHECK_CUDA(y); CHECK_F32(x); CHECK_BF16(y);
  CHECK_CONTIG(x); CHECK_CONTIG(y); CHECK_ALIGN16(x); CHECK_ALIGN16(y);
  TORCH_CHECK(x.numel() == y.numel(), "size mismatch");
  const DeviceGuard guard(x.device());
  dm::cast_f32_bf16(x.data_ptr<float>(), bfp(y), x.numel(), cur_stream());
}

void rows_mean(at::Tensor x, at::Tensor out, double scale) {
  CHECK_CUDA(x); CHECK_CUDA(out); CHECK_F32(x); CHECK_F32(out);
  CHECK_CONTIG(x); CHECK_CONTIG(out);
  TORCH_CHECK(x.dim() == 2 && x.size(1) == out.numel(), "x must be [rows, N]");
  const DeviceGuard guard(x.device());
  dm::rows_mean(x.data_ptr<float>(), out.data_ptr<float>(), (int)x.size(0), out.numel(),
                (float)scale, cur_stream());
}

// ------------------------------------------------------------------ q8 codec (csrc/gradq.hip)
void q8_encode(at::Tensor g, c10::optional<at::Tensor> r, at::Tensor payload,
               int64_t max_blocks) {
  CHECK_CUDA(g); CHECK_F32(g); CHECK_CONTIG(g);
  CHECK_CUDA(payload); CHECK_CONTIG(payload);
  TORCH_CHECK(payload.scalar_type() == at::kByte, "payload must be uint8");
  TORCH_CHECK(g.dim() == 1 && payload.dim() == 1, "g and payload must be 1-d");
  TORCH_CHECK(payload.numel() == dm::q8_payload_bytes(g.numel()),
              "payload must hold q8_payload_bytes(n) = ", dm::q8_payload_bytes(g.numel()),
              " bytes, got ", payload.numel());
  TORCH_CHECK((reinterpret_cast<uintptr_t>(payload.data_ptr()) & 3) == 0,
              "payload must be 4-B aligned");
  TORCH_CHECK(g.device() == payload.device(), "g and payload on different devices");
  float* rp = nullptr;
  if (r.has_value() && r->defined()) {
    CHECK_CUDA(*r); CHECK_F32(*r); CHECK_CONTIG(*r);
    TORCH_CHECK(r->dim() == 1 && r->numel() == g.numel(), "residual size mismatch");
    TORCH_CHECK(r->device() == g.device(), "g and residual on different devices");
    rp = r->data_ptr<float>();
  }
  const DeviceGuard guard(g.device());
  dm::q8_encode(g.data_ptr<float>(), rp, payload.data_ptr<uint8_t>(), g.numel(),
                (int)max_blocks, cur_stream());
}

void q8_decode_mean(at::Tensor gathered, at::Tensor out, double scale, int64_t max_blocks) {
  CHECK_CUDA(gathered); CHECK_CONTIG(gathered);
  CHECK_CUDA(out); CHECK_F32(out); CHECK_CONTIG(out);
  TORCH_CHECK(gathered.scalar_type() == at::kByte, "gathered must be uint8");
  TORCH_CHECK(gathered.dim() == 2 && out.dim() == 1, "gathered must be [ws, payload], out 1-d");
  TORCH_CHECK(gathered.size(0) >= 1 && gathered.size(0) <= INT32_MAX, "bad row count");
  TORCH_CHECK(gathered.size(1) == dm::q8_payload_bytes(out.numel()),
              "rows must hold q8_payload_bytes(n) = ", dm::q8_payload_bytes(out.numel()),
              " bytes, got ", gathered.size(1));
  TORCH_CHECK((reinterpret_cast<uintptr_t>(gathered.data_ptr()) & 3) == 0,
              "gathered must be 4-B aligned");
  TORCH_CHECK(gathered.device() == out.device(), "gathered and out on different devices");
  const DeviceGuard guard(out.device());
  dm::q8_decode_mean(gathered.data_ptr<uint8_t>(), gathered.size(1), (int)gathered.size(0),
                     out.data_ptr<float>(), out.numel(), (float)scale, (int)max_blocks,
                     cur_stream());
}

// ------------------------------------------------------------------ topk codec (csrc/gradk.hip)
static void topk_check_keep(int64_t keep) {
  TORCH_CHECK(keep >= 1 && keep <= dm::topk_max_keep(), "keep must be in 1..",
              dm::topk_max_keep(), ", got ", keep);
}

int64_t topk_payload_bytes(int64_t n, int64_t keep) {
  topk_check_keep(keep);
  TORCH_CHECK(n >= 0, "n must be >= 0");
  return (int64_t)dm::topk_payload_bytes(n, (int)keep);
}

void topk_encode(at::Tensor g, c10::optional<at::Tensor> r, at::Tensor payload, int64_t keep,
                 int64_t max_blocks) {
  topk_check_keep(keep);
  CHECK_CUDA(g); CHECK_F32(g); CHECK_CONTIG(g);
  CHECK_CUDA(payload); CHECK_CONTIG(payload);
  TORCH_CHECK(payload.scalar_type() == at::kByte, "payload must be uint8");
  TORCH_CHECK(g.dim() == 1 && payload.dim() == 1, "g and payload must be 1-d");
  // one launch indexes bytes of the slice with 31 bits to spare: split a larger slice
  TORCH_CHECK(g.numel() * 4 < (int64_t(1) << 31), "topk_encode: at most 2^29 - 1 elements per "
              "call, got ", g.numel());
  TORCH_CHECK(payload.numel() == dm::topk_payload_bytes(g.numel(), (int)keep),
              "payload must hold topk_payload_bytes(n, keep) = ",
              dm::topk_payload_bytes(g.numel(), (int)keep), " bytes, got ", payload.numel());
  TORCH_CHECK((reinterpret_cast<uintptr_t>(payload.data_ptr()) & 3) == 0,
              "payload must be 4-B aligned");
  TORCH_CHECK(g.device() == payload.device(), "g and payload on different devices");
  float* rp = nullptr;
  if (r.has_value() && r->defined()) {
    CHECK_CUDA(*r); CHECK_F32(*r); CHECK_CONTIG(*r);
    TORCH_CHECK(r->dim() == 1 && r->numel() == g.numel(), "residual size mismatch");
    TORCH_CHECK(r->device() == g.device(), "g and residual on different devices");
    rp = r->data_ptr<float>();
  }
  const DeviceGuard guard(g.device());
  dm::topk_encode(g.data_ptr<float>(), rp, payload.data_ptr<uint8_t>(), g.numel(), (int)keep,
                  (int)max_blocks, cur_stream());
}

void topk_decode_mean(at::Tensor gathered, at::Tensor out, int64_t keep, double scale,
                      int64_t max_blocks) {
  topk_check_keep(keep);
  CHECK_CUDA(gathered); CHECK_CONTIG(gathered);
  CHECK_CUDA(out); CHECK_F32(out); CHECK_CONTIG(out);
  TORCH_CHECK(gathered.scalar_type() == at::kByte, "gathered must be uint8");
  TORCH_CHECK(gathered.dim() == 2 && out.dim() == 1, "gathered must be [ws, payload], out 1-d");
  TORCH_CHECK(gathered.size(0) >= 1 && gathered.size(0) <= INT32_MAX, "bad row count");
  TORCH_CHECK(out.numel() * 4 < (int64_t(1) << 31), "topk_decode_mean: at most 2^29 - 1 "
              "elements per call, got ", out.numel());
  TORCH_CHECK(gathered.size(1) == dm::topk_payload_bytes(out.numel(), (int)keep),
              "rows must hold topk_payload_bytes(n, keep) = ",
              dm::topk_payload_bytes(out.numel(), (int)keep), " bytes, got ", gathered.size(1));
  TORCH_CHECK((reinterpret_cast<uintptr_t>(gathered.data_ptr()) & 3) == 0,
              "gathered must be 4-B aligned");
  TORCH_CHECK(gathered.device() == out.device(), "gathered and out on different devices");
  const DeviceGuard guard(out.device());
  dm::topk_decode_mean(gathered.data_ptr<uint8_t>(), gathered.size(1), (int)gathered.size(0),
                       out.data_ptr<float>(), out.numel(), (int)keep, (float)scale,
                       (int)max_blocks, cur_stream());
}

// ------------------------------------------------------------------ LARS (csrc/lars.hip)
// Build the segment and chunk tables for tensors at `offsets` (elements, 16-B aligned) with
// `numels` elements each inside a flat buffer of `total` elements.  Returns CPU int64 tensors
// (seg [n,5], chunks [m,3]); the caller moves them to the device once.  Everything the kernels
// index with is validated here, on the host.
std::vector<at::Tensor> lars_table(std::vector<int64_t> offsets, std::vector<int64_t> numels,
                                   std::vector<bool> adapted, int64_t total) {
  const size_t n = offsets.size();
  TORCH_CHECK(numels.size() == n && adapted.size() == n, "lars_table: list lengths differ");
  TORCH_CHECK(n < (size_t)1 << 30, "lars_table: too many tensors");
  const int64_t C = dm::lars_chunk();
  int64_t m = 0;
  for (size_t t = 0; t < n; ++t) {
    TORCH_CHECK(offsets[t] >= 0 && numels[t] >= 0 && offsets[t] + numels[t] <= total,
                "lars_table: tensor ", t, " lies outside the flat buffer");
    TORCH_CHECK(offsets[t] % 4 == 0, "lars_table: tensor ", t, " is not 16-B aligned");
    for (size_t u = 0; u < t; ++u)
      TORCH_CHECK(offsets[u] + numels[u] <= offsets[t] || offsets[t] + numels[t] <= offsets[u],
                  "lars_table: tensors ", u, " and ", t, " overlap");
    m += (numels[t] + C - 1) / C;
  }
  TORCH_CHECK(m < (int64_t)1 << 30, "lars_table: too many chunks");
  auto opt = at::TensorOptions().dtype(at::kLong);
  at::Tensor seg = at::empty({(int64_t)n, 5}, opt), chunks = at::empty({m, 3}, opt);
  int64_t* sp = seg.data_ptr<int64_t>();
  int64_t* cp = chunks.data_ptr<int64_t>();
  int64_t c = 0;
  for (size_t t = 0; t < n; ++t) {
    const int64_t cnt = (numels[t] + C - 1) / C;
    sp[5 * t + 0] = offsets[t];
    sp[5 * t + 1] = numels[t];
    sp[5 * t + 2] = adapted[t] ? 1 : 0;
    sp[5 * t + 3] = c;
    sp[5 * t + 4] = cnt;
    for (int64_t i = 0; i < cnt; ++i, ++c) {
      cp[3 * c + 0] = offsets[t] + i * C;
      cp[3 * c + 1] = std::min(C, numels[t] - i * C);
      cp[3 * c + 2] = (int64_t)t;
    }
  }
  return {seg, chunks};
}

void lars_step(at::Tensor w, at::Tensor g, at::Tensor buf, at::Tensor seg, at::Tensor chunks,
               at::Tensor hyper, at::Tensor partial, at::Tensor tot, at::Tensor stats,
               at::Tensor gnorm, bool nesterov, int64_t launches) {
  for (auto* t : {&w, &g, &buf, &hyper, &partial, &tot, &stats, &gnorm}) {
    CHECK_CUDA(*t); CHECK_F32(*t); CHECK_CONTIG(*t); CHECK_ALIGN16(*t);
    TORCH_CHECK(t->device() == w.device(), "lars_step: tensors on different devices");
  }
  for (auto* t : {&seg, &chunks}) {
    CHECK_CUDA(*t); CHECK_CONTIG(*t);
    TORCH_CHECK(t->scalar_type() == at::kLong && t->dim() == 2 && t->device() == w.device(),
                "lars_step: tables are 2-D int64 tensors on the parameters' device");
  }
  TORCH_CHECK(g.numel() == w.numel() && buf.numel() == w.numel(), "param/grad/buf size mismatch");
  TORCH_CHECK(seg.size(1) == 5 && chunks.size(1) == 3, "lars_step: seg [n,5], chunks [m,3]");
  const int64_t n = seg.size(0), m = chunks.size(0);
  TORCH_CHECK(n < ((int64_t)1 << 30) && m < ((int64_t)1 << 30), "lars_step: table too large");
  TORCH_CHECK(hyper.numel() == dm::lars_hyper_count(), "lars_step: hyper holds ",
              dm::lars_hyper_count(), " floats");
  TORCH_CHECK(partial.numel() == 2 * m && tot.numel() == 2 * n && stats.numel() == 3 * n &&
                  gnorm.numel() == 1,
              "lars_step: workspace sizes do not match the tables");
  TORCH_CHECK(launches >= 1 && launches <= 7, "lars_step: launches is a mask of bits 0..2");
  const DeviceGuard guard(w.device());
  dm::lars_step(w.data_ptr<float>(), g.data_ptr<float>(), buf.data_ptr<float>(), w.numel(),
                reinterpret_cast<const long long*>(seg.data_ptr<int64_t>()), (int)n,
                reinterpret_cast<const long long*>(chunks.data_ptr<int64_t>()), (int)m,
                hyper.data_ptr<float>(), partial.data_ptr<float>(), tot.data_ptr<float>(),
                stats.data_ptr<float>(), gnorm.data_ptr<float>(), nesterov, (int)launches,
                cur_stream());
}

// ------------------------------------------------------------------ small conv (LeNet)
inline bool is_bf16(const at::Tensor& t) { return t.scalar_type() == at::kBFloat16; }
inline void check_act(const at::Tensor& t, const char* n) {
  TORCH_CHECK(t.is_cuda(), n, " must be a HIP tensor");
  TORCH_CHECK(t.is_contiguous(), n, " must be contiguous");
  TORCH_CHECK(t.scalar_type() == at::kFloat || t.scalar_type() == at::kBFloat16, n,
              " must be fp32/bf16");
}
inline const void* optp(const c10::optional<at::Tensor>& t) {
  return (t.has_value() && t->defined()) ? t->data_ptr() : nullptr;
}

// every tensor of one call lives on the device of the first
inline void check_same_dev(const at::Tensor& ref, const at::Tensor& t, const char* n) {
  TORCH_CHECK(t.is_cuda() && t.device() == ref.device(), n, " must be on the same device as ",
              "the first operand (", ref.device(), "), got ", t.device());
}
inline bool has(const c10::optional<at::Tensor>& t) { return t.has_value() && t->defined(); }
inline void check_f32_vec(const at::Tensor& ref, const at::Tensor& t, int64_t n, const char* name) {
  check_same_dev(ref, t, name);
  TORCH_CHECK(t.scalar_type() == at::kFloat && t.is_contiguous() && t.numel() == n, name,
              " must be a contiguous fp32 tensor of ", n, " elements");
}
inline void check_shape4(const at::Tensor& t, int64_t a, int64_t b, int64_t c, int64_t d,
                         const char* name) {
  TORCH_CHECK(t.dim() == 4 && t.size(0) == a && t.size(1) == b && t.size(2) == c && t.size(3) == d,
              name, " shape mismatch: expected [", a, ", ", b, ", ", c, ", ", d, "], got ", t.sizes());
}
inline void check_pool_mask(const at::Tensor& ref, const c10::optional<at::Tensor>& mask,
                            int64_t n) {
  TORCH_CHECK(has(mask), "mask required with pool 2");
  check_same_dev(ref, *mask, "mask");
  TORCH_CHECK(mask->scalar_type() == at::kByte && mask->is_contiguous() && mask->numel() == n,
              "mask must be a contiguous uint8 tensor of ", n, " elements (one per pooled element)");
}

// geometry shared by the two thin-conv bindings; refuses what the kernels have no template for
struct SmallConvGeom { int B, Cin, H, W, Cout, K, OH, OW, PH, PW; };
inline SmallConvGeom small_conv_geom(const at::Tensor& x, const at::Tensor& w, int64_t pad,
                                     int64_t pool) {
  check_act(x, "x");
  check_same_dev(x, w, "w");
  CHECK_F32(w); CHECK_CONTIG(w);
  TORCH_CHECK(x.dim() == 4 && w.dim() == 4 && w.size(1) == x.size(1) && w.size(2) == w.size(3),
              "w must be [Cout, Cin, K, K] with x's Cin, got ", w.sizes(), " for x ", x.sizes());
  TORCH_CHECK(x.numel() > 0 && w.size(0) >= 1, "empty x or w");
  const int64_t K = w.size(2);
  TORCH_CHECK(K == 3 || K == 5, "conv_small supports K in {3,5}, got ", K);
  TORCH_CHECK(pool == 1 || pool == 2, "pool must be 1 or 2, got ", pool);
  TORCH_CHECK(pad >= 0, "pad must be >= 0, got ", pad);
  const int64_t OH = x.size(2) + 2 * pad - K + 1, OW = x.size(3) + 2 * pad - K + 1;
  TORCH_CHECK(OH >= pool && OW >= pool, "image ", x.size(2), " x ", x.size(3),
              " too small for K ", K, ", pad ", pad, ", pool ", pool);
  return {(int)x.size(0), (int)x.size(1), (int)x.size(2), (int)x.size(3), (int)w.size(0), (int)K,
          (int)OH, (int)OW, (int)(OH / pool), (int)(OW / pool)};
}

void conv_small_fwd(at::Tensor x, at::Tensor w, c10::optional<at::Tensor> bias, at::Tensor y,
                    c10::optional<at::Tensor> mask, int64_t pad, int64_t pool, bool relu) {
  const SmallConvGeom g = small_conv_geom(x, w, pad, pool);
  check_act(y, "y");
  check_same_dev(x, y, "y");
  TORCH_CHECK(is_bf16(x) == is_bf16(y), "x/y dtype mismatch");
  check_shape4(y, g.B, g.Cout, g.PH, g.PW, "y");
  if (has(bias)) check_f32_vec(x, *bias, g.Cout, "bias");
  if (pool > 1) check_pool_mask(x, mask, y.numel());
  const DeviceGuard guard(x.device());
  const size_t lds = sizeof(float) * g.Cin * g.K * g.K;
  TORCH_CHECK(lds <= dm::conv_small_lds_limit(), "conv_small_fwd: Cin ", g.Cin, " with K ", g.K,
              " needs ", lds, " bytes of LDS, the launch has ", dm::conv_small_lds_limit());
  dm::conv_small_fwd(x.data_ptr(), w.data_ptr<float>(),
                     has(bias) ? bias->data_ptr<float>() : nullptr, y.data_ptr(),
                     pool > 1 ? (uint8_t*)mask->data_ptr() : nullptr, g.B, g.Cin, g.H, g.W, g.Cout,
                     g.K, (int)pad, (int)pool, relu ? 1 : 0, is_bf16(x), cur_stream());
}

int64_t conv_small_workspace(int64_t B, int64_t Cin, int64_t H, int64_t W, int64_t Cout,
                             int64_t K, int64_t pad, int64_t bs) {
  TORCH_CHECK(bs >= 1, "bs must be >= 1, got ", bs);
  const long long OH = H + 2 * pad - K + 1, OW = W + 2 * pad - K + 1;
  const long long total = B * Cout * OH * OW;
  const long long S = (B + bs - 1) / bs;
  return (total + 63) / 64 * 64 + S * (Cout * Cin * K * K + Cout);
}

void conv_small_bwd(at::Tensor x, at::Tensor w, at::Tensor dp, at::Tensor yp,
                    c10::optional<at::Tensor> mask, c10::optional<at::Tensor> dx, at::Tensor dw,
                    c10::optional<at::Tensor> db, at::Tensor work, int64_t pad, int64_t pool,
                    bool relu, double beta, int64_t bs) {
  const SmallConvGeom g = small_conv_geom(x, w, pad, pool);
  TORCH_CHECK(bs >= 1, "bs must be >= 1, got ", bs);
  for (auto t : {std::make_pair(&dp, "dp"), std::make_pair(&yp, "yp")}) {
    check_act(*t.first, t.second);
    check_same_dev(x, *t.first, t.second);
    TORCH_CHECK(is_bf16(*t.first) == is_bf16(x), t.second, " must have x's dtype");
    check_shape4(*t.first, g.B, g.Cout, g.PH, g.PW, t.second);
  }
  check_same_dev(x, dw, "dw");
  CHECK_F32(dw); CHECK_CONTIG(dw);
  TORCH_CHECK(dw.sizes() == w.sizes(), "dw shape mismatch: expected ", w.sizes(), ", got ", dw.sizes());
  if (has(db)) check_f32_vec(x, *db, g.Cout, "db");
  if (has(dx)) {
    check_act(*dx, "dx");
    check_same_dev(x, *dx, "dx");
    TORCH_CHECK(is_bf16(*dx) == is_bf16(x), "dx must have x's dtype");
    TORCH_CHECK(dx->sizes() == x.sizes(), "dx shape mismatch: expected ", x.sizes(), ", got ", dx->sizes());
  }
  check_same_dev(x, work, "work");
  CHECK_F32(work); CHECK_CONTIG(work);
  const int64_t need = conv_small_workspace(g.B, g.Cin, g.H, g.W, g.Cout, g.K, pad, bs);
  TORCH_CHECK(work.numel() >= need, "workspace too small: ", work.numel(), " < ", need);
  if (pool > 1) check_pool_mask(x, mask, dp.numel());
  const DeviceGuard guard(x.device());
  if (has(dx)) {
    // backward-data stages one image's padded upstream gradient in LDS: refuse an image that does
    // not fit instead of a launch that fails and leaves dx unwritten
    const size_t lds = dm::conv_small_bwd_data_lds(g.Cout, g.K, g.OH, g.OW);
    TORCH_CHECK(lds <= dm::conv_small_lds_limit(), "conv_small_bwd: backward-data of a ", g.H,
                " x ", g.W, " image (conv output ", g.OH, " x ", g.OW, ", Cout ", g.Cout, ", K ",
                g.K, ") needs ", lds, " bytes of LDS, the launch has ", dm::conv_small_lds_limit());
  }
  dm::conv_small_bwd(x.data_ptr(), w.data_ptr<float>(), dp.data_ptr(), yp.data_ptr(),
                     pool > 1 ? (const uint8_t*)mask->data_ptr() : nullptr,
                     has(dx) ? dx->data_ptr() : nullptr, dw.data_ptr<float>(),
                     has(db) ? db->data_ptr<float>() : nullptr, work.data_ptr<float>(), g.B,
                     g.Cin, g.H, g.W, g.Cout, g.K, (int)pad, (int)pool, relu ? 1 : 0, (float)beta,
                     (int)bs, is_bf16(x), cur_stream());
}

// ------------------------------------------------------------------ strided GEMM
// (S, kchunk, chunks) of dm::gemm_plan: the split-K decision gemm() takes for a shape
std::tuple<int64_t, int64_t, int64_t> gemm_plan(int64_t M, int64_t N, int64_t K, bool a_bf16,
                                                bool lowp) {
  TORCH_CHECK(M >= 0 && N >= 0 && K >= 1, "gemm_plan: M, N >= 0 and K >= 1");
  const dm::GemmPlan p = dm::gemm_plan(M, N, K, a_bf16 ? 1 : 0, lowp ? 1 : 0);
  return {p.S, p.kchunk, p.chunks};
}

// C[m,n] = alpha * sum_k A(m,k) B(k,n) + beta*C + bias ; strides in elements.
void gemm(at::Tensor A, c10::optional<at::Tensor> Amask, at::Tensor B, c10::optional<at::Tensor> C,
          c10::optional<at::Tensor> C32, c10::optional<at::Tensor> bias, int64_t M, int64_t N,
          int64_t K, int64_t sam, int64_t sak, int64_t sbk, int64_t sbn, int64_t scm,
          double alpha, double beta, bool relu, bool lowp) {
  TORCH_CHECK(A.is_cuda(), "A must be a HIP tensor");
  check_same_dev(A, B, "B");
  auto lowp_or_f32 = [](const at::Tensor& t, const char* n) {
    TORCH_CHECK(t.scalar_type() == at::kFloat || t.scalar_type() == at::kBFloat16, n,
                " must be fp32 or bf16, got ", t.scalar_type());
  };
  lowp_or_f32(A, "A");
  lowp_or_f32(B, "B");
  TORCH_CHECK(M >= 0 && N >= 0, "M and N must be >= 0, got ", M, ", ", N);
  TORCH_CHECK(K >= 1, "K must be >= 1, got ", K);
  TORCH_CHECK(M < (1LL << 31) && N < (1LL << 31) && K < (1LL << 31), "M, N, K must fit an int");
  TORCH_CHECK(sam >= 0 && sak >= 0 && sbk >= 0 && sbn >= 0 && scm >= 0,
              "strides must be non-negative");
  auto span_ok = [](const at::Tensor& t, int64_t r, int64_t c, int64_t sr, int64_t sc) {
    return r == 0 || c == 0 || (r - 1) * sr + (c - 1) * sc < t.numel();
  };
  TORCH_CHECK(span_ok(A, M, K, sam, sak), "A too small for M,K,strides");
  TORCH_CHECK(span_ok(B, K, N, sbk, sbn), "B too small for K,N,strides");
  if (has(Amask)) {
    check_same_dev(A, *Amask, "Amask");
    TORCH_CHECK(Amask->scalar_type() == A.scalar_type(), "Amask must have A's dtype");
    TORCH_CHECK(Amask->numel() >= A.numel(), "Amask must have at least A's ", A.numel(), " elements");
  }
  void* cp = nullptr;
  int cbf = 0;
  if (has(C)) {
    check_same_dev(A, *C, "C");
    lowp_or_f32(*C, "C");
    cp = C->data_ptr(); cbf = is_bf16(*C);
    TORCH_CHECK(span_ok(*C, M, N, scm, 1), "C too small for M,N,scm");
  }
  float* c32 = nullptr;
  if (has(C32)) {
    check_same_dev(A, *C32, "C32");
    CHECK_F32(*C32); c32 = C32->data_ptr<float>();
    TORCH_CHECK(span_ok(*C32, M, N, scm, 1), "C32 too small for M,N,scm");
  }
  TORCH_CHECK(cp || c32, "an output is required");
  if (has(bias)) {
    check_same_dev(A, *bias, "bias");
    CHECK_F32(*bias); TORCH_CHECK(bias->numel() >= N, "bias must have at least N elements");
  }
  if (M == 0 || N == 0) return;  // nothing to write (and no zero-sized grid)
  const DeviceGuard guard(A.device());
  const dm::GemmPlan plan = dm::gemm_plan(M, N, K, is_bf16(A), lowp ? 1 : 0);
  at::Tensor part;
  if (plan.S > 1) part = at::empty({(long long)plan.S * M * N}, A.options().dtype(at::kFloat));
  dm::gemm_strided(A.data_ptr(), optp(Amask), is_bf16(A), B.data_ptr(), is_bf16(B), cp, cbf, c32,
                   has(bias) ? bias->data_ptr<float>() : nullptr, M, N, K, sam, sak, sbk,
                   sbn, scm, (float)alpha, (float)beta, relu ? 1 : 0, lowp ? 1 : 0,
                   plan.S > 1 ? part.data_ptr<float>() : nullptr, plan, cur_stream());
}

// ------------------------------------------------------------ CU-masked streams
// A stream whose kernels may only use the CUs set in `mask` (32 CUs per word).  Its own
// hardware queue carries the mask, so two processes on one GPU can each own a disjoint CU
// partition: the lab-4 pipeline uses it to give every stage a "device" of its own.
int64_t cu_mask_stream(std::vector<int64_t> mask) {
  TORCH_CHECK(!mask.empty(), "empty CU mask");
  std::vector<uint32_t> m(mask.begin(), mask.end());
  hipStream_t st = nullptr;
  TORCH_CHECK(hipExtStreamCreateWithCUMask(&st, (uint32_t)m.size(), m.data()) == hipSuccess,
              "hipExtStreamCreateWithCUMask failed");
  return (int64_t)(uintptr_t)st;
}
std::vector<int64_t> cu_mask_of(int64_t stream, int64_t words) {
  std::vector<uint32_t> m((size_t)words, 0u);
  TORCH_CHECK(hipExtStreamGetCUMask((hipStream_t)(uintptr_t)stream, (uint32_t)words, m.data()) ==
              hipSuccess, "hipExtStreamGetCUMask failed");
  return std::vector<int64_t>(m.begin(), m.end());
}
// ------------------------------------------------------------ xGMI one-/two-shot all-reduce
int64_t xgmi_alloc(int64_t bytes) { return (int64_t)(uintptr_t)dm::xgmi_alloc((size_t)bytes); }
void xgmi_free(int64_t ptr) { dm::xgmi_free((void*)(uintptr_t)ptr); }
py::bytes xgmi_get_handle(int64_t ptr) {
  char h[64];
  dm::xgmi_get_handle((void*)(uintptr_t)ptr, h);
  return py::bytes(h, 64);
}
int64_t xgmi_open_handle(py::bytes handle) {
  std::string h = handle;
  TORCH_CHECK(h.size() == 64, "IPC handle must be 64 bytes");
  return (int64_t)(uintptr_t)dm::xgmi_open_handle(h.data());
}
void xgmi_close_handle(int64_t ptr) { dm::xgmi_close_handle((void*)(uintptr_t)ptr); }
void xgmi_allreduce(at::Tensor in, at::Tensor out, int64_t cap, std::vector<int64_t> data,
                    std::vector<int64_t> flags, int64_t rank, double scale, at::Tensor state,
                    int64_t algo, int64_t share) {
  CHECK_F32(in);
  CHECK_F32(out);
  TORCH_CHECK(in.is_contiguous() && out.is_contiguous() && in.numel() == out.numel());
  TORCH_CHECK(in.numel() <= cap, "tensor larger than the shared buffer");
  const int W = data.size();
  TORCH_CHECK(W >= 1 && W <= 8 && (int)flags.size() == W && rank >= 0 && rank < W);
  // [timeout flag, last published epoch, done-block counter, pad] on the device
  TORCH_CHECK(state.scalar_type() == at::kInt && state.is_cuda() && state.numel() >= 3 &&
              state.device() == in.device());
  std::vector<void*> d(W), f(W);
  for (int q = 0; q < W; ++q) {
    d[q] = (void*)(uintptr_t)data[q];
    f[q] = (void*)(uintptr_t)flags[q];
  }
  const DeviceGuard guard(in.device());
  dm::xgmi_allreduce(in.data_ptr<float>(), out.data_ptr<float>(), in.numel(), cap, d.data(),
                     f.data(), (int)rank, W, (float)scale,
                     reinterpret_cast<unsigned*>(state.data_ptr<int>()), (int)algo, cur_stream(),
                     (int)share);
}

// P2P channel (csrc/p2p_xgmi.hip): src/dst tensors contiguous, 16-B aligned, bytes % 16 == 0;
// ring/full/free are raw device addresses (own or IPC-opened), state an int32[4] device tensor
void p2p_xgmi_send(at::Tensor src, int64_t ring, int64_t full, int64_t free_, int64_t slot_bytes,
                   int64_t nslot, at::Tensor state) {
  CHECK_CUDA(src); CHECK_CONTIG(src); CHECK_ALIGN16(src); CHECK_CUDA(state);
  const int64_t bytes = src.numel() * src.element_size();
  TORCH_CHECK(bytes % 16 == 0 && bytes <= slot_bytes && slot_bytes % 16 == 0 && nslot >= 1,
              "p2p send: payload must be a multiple of 16 B and fit a ring slot");
  TORCH_CHECK(state.scalar_type() == at::kInt && state.numel() >= 4, "state: int32[4]");
  const DeviceGuard guard(src.device());
  dm::p2p_xgmi_send(src.data_ptr(), bytes, (void*)(uintptr_t)ring, (void*)(uintptr_t)full,
                    (const void*)(uintptr_t)free_, slot_bytes, (int)nslot,
                    reinterpret_cast<unsigned*>(state.data_ptr<int>()), cur_stream());
}

void p2p_xgmi_recv(at::Tensor dst, int64_t ring, int64_t full, int64_t free_, int64_t slot_bytes,
                   int64_t nslot, at::Tensor state) {
  CHECK_CUDA(dst); CHECK_CONTIG(dst); CHECK_ALIGN16(dst); CHECK_CUDA(state);
  const int64_t bytes = dst.numel() * dst.element_size();
  TORCH_CHECK(bytes % 16 == 0 && bytes <= slot_bytes && slot_bytes % 16 == 0 && nslot >= 1,
              "p2p recv: payload must be a multiple of 16 B and fit a ring slot");
  TORCH_CHECK(state.scalar_type() == at::kInt && state.numel() >= 4, "state: int32[4]");
  const DeviceGuard guard(dst.device());
  dm::p2p_xgmi_recv(dst.data_ptr(), bytes, (const void*)(uintptr_t)ring,
                    (const void*)(uintptr_t)full, (void*)(uintptr_t)free_, slot_bytes, (int)nslot,
                    reinterpret_cast<unsigned*>(state.data_ptr<int>()), cur_stream());
}

void colsum(at::Tensor A, c10::optional<at::Tensor> Amask, at::Tensor out, double beta) {
  TORCH_CHECK(A.is_cuda() && A.dim() == 2 && A.is_contiguous(), "A must be a contiguous 2-d HIP tensor");
  TORCH_CHECK(A.scalar_type() == at::kFloat || A.scalar_type() == at::kBFloat16,
              "A must be fp32 or bf16, got ", A.scalar_type());
  if (has(Amask)) {
    check_same_dev(A, *Amask, "Amask");
    TORCH_CHECK(Amask->scalar_type() == A.scalar_type(), "Amask must have A's dtype");
    TORCH_CHECK(Amask->sizes() == A.sizes() && Amask->is_contiguous(),
                "Amask must be contiguous with A's shape ", A.sizes(), ", got ", Amask->sizes());
  }
  check_f32_vec(A, out, A.size(1), "out");
  if (A.size(1) == 0) return;
  const DeviceGuard guard(A.device());
  dm::colsum(A.data_ptr(), optp(Amask), is_bf16(A), out.data_ptr<float>(), A.size(0), A.size(1),
             (float)beta, cur_stream());
}

void bias_act(at::Tensor y, c10::optional<at::Tensor> bias, at::Tensor out, bool relu) {
  CHECK_F32(y);
  TORCH_CHECK(y.is_cuda() && y.dim() == 2 && y.is_contiguous());
  TORCH_CHECK(out.is_cuda() && out.is_contiguous() && out.sizes() == y.sizes() &&
              (out.scalar_type() == at::kFloat || out.scalar_type() == at::kBFloat16));
  if (bias.has_value()) { CHECK_F32(*bias); TORCH_CHECK(bias->numel() == y.size(1)); }
  const DeviceGuard guard(y.device());
  dm::bias_act(y.data_ptr<float>(), bias.has_value() ? bias->data_ptr<float>() : nullptr,
               out.data_ptr(), is_bf16(out), y.size(0), y.size(1), relu ? 1 : 0, cur_stream());
}

// ------------------------------------------------------------------ loss / eval / spin
void cross_entropy(at::Tensor logits, at::Tensor labels, at::Tensor rowloss, at::Tensor loss,
                   c10::optional<at::Tensor> dlogits, double scale) {
  check_act(logits, "logits");
  TORCH_CHECK(logits.dim() == 2 && labels.scalar_type() == at::kLong && labels.numel() == logits.size(0));
  CHECK_F32(rowloss); CHECK_F32(loss);
  TORCH_CHECK(rowloss.numel() >= logits.size(0));
  if (dlogits.has_value()) { check_act(*dlogits, "dlogits"); TORCH_CHECK(dlogits->sizes() == logits.sizes() && is_bf16(*dlogits) == is_bf16(logits)); }
  const DeviceGuard guard(logits.device());
  dm::cross_entropy(logits.data_ptr(), (const long long*)labels.data_ptr(), rowloss.data_ptr<float>(),
                    loss.data_ptr<float>(), dlogits.has_value() ? dlogits->data_ptr() : nullptr,
                    logits.size(0), logits.size(1), (float)scale, -100, is_bf16(logits),
                    cur_stream());
}

void argmax_count(at::Tensor logits, at::Tensor labels, at::Tensor correct) {
  check_act(logits, "logits");
  TORCH_CHECK(correct.scalar_type() == at::kLong && labels.scalar_type() == at::kLong);
  const DeviceGuard guard(logits.device());
  dm::argmax_count(logits.data_ptr(), (const long long*)labels.data_ptr(), logits.size(0), logits.size(1),
                   (unsigned long long*)correct.data_ptr(), is_bf16(logits), cur_stream());
}

void cross_entropy_smooth(at::Tensor logits, at::Tensor labels, at::Tensor rowloss, at::Tensor loss,
                          c10::optional<at::Tensor> dlogits, double scale, double eps) {
  check_act(logits, "logits");
  TORCH_CHECK(logits.dim() == 2 && labels.scalar_type() == at::kLong && labels.numel() == logits.size(0));
  TORCH_CHECK(labels.is_cuda() && labels.is_contiguous(), "labels: contiguous device tensor");
  TORCH_CHECK(eps >= 0.0 && eps <= 1.0, "label smoothing must be in [0, 1]");
  TORCH_CHECK(logits.size(0) >= 1 && logits.size(1) >= 1 && logits.size(0) < (1ll << 31) &&
              logits.size(1) < (1ll << 31), "logits: empty or too large");
  TORCH_CHECK(rowloss.is_cuda() && rowloss.is_contiguous(), "rowloss: contiguous device tensor");
  CHECK_F32(rowloss); CHECK_F32(loss);
  TORCH_CHECK(rowloss.numel() >= logits.size(0) && loss.numel() >= 1);
  if (dlogits.has_value()) { check_act(*dlogits, "dlogits"); TORCH_CHECK(dlogits->sizes() == logits.sizes() && is_bf16(*dlogits) == is_bf16(logits)); }
  const DeviceGuard guard(logits.device());
  dm::cross_entropy_smooth(logits.data_ptr(), (const long long*)labels.data_ptr(),
                           rowloss.data_ptr<float>(), loss.data_ptr<float>(),
                           dlogits.has_value() ? dlogits->data_ptr() : nullptr, logits.size(0),
                           logits.size(1), (float)scale, (float)eps, -100, is_bf16(logits),
                           cur_stream());
}

// Mixed-target cross-entropy: ya, yb int64 [B], lam float32 [B] (the weight of ya)
void cross_entropy_mix(at::Tensor logits, at::Tensor ya, at::Tensor yb, at::Tensor lam,
                       at::Tensor rowloss, at::Tensor loss, c10::optional<at::Tensor> dlogits,
                       double scale, double eps) {
  check_act(logits, "logits");
  TORCH_CHECK(logits.dim() == 2, "logits: (B, C)");
  for (const at::Tensor* y : {&ya, &yb})
    TORCH_CHECK(y->scalar_type() == at::kLong && y->numel() == logits.size(0) && y->is_cuda() &&
                y->is_contiguous() && y->device() == logits.device(),
                "labels: contiguous int64 [B] on the device of logits");
  TORCH_CHECK(lam.scalar_type() == at::kFloat && lam.numel() == logits.size(0) && lam.is_cuda() &&
              lam.is_contiguous() && lam.device() == logits.device(),
              "lam: contiguous float32 [B] on the device of logits");
  TORCH_CHECK(eps >= 0.0 && eps <= 1.0, "label smoothing must be in [0, 1]");
  TORCH_CHECK(logits.size(0) >= 1 && logits.size(1) >= 1 && logits.size(0) < (1ll << 31) &&
              logits.size(1) < (1ll << 31), "logits: empty or too large");
  TORCH_CHECK(rowloss.is_cuda() && rowloss.is_contiguous(), "rowloss: contiguous device tensor");
  CHECK_F32(rowloss); CHECK_F32(loss);
  TORCH_CHECK(rowloss.numel() >= logits.size(0) && loss.numel() >= 1);
  if (dlogits.has_value()) { check_act(*dlogits, "dlogits"); TORCH_CHECK(dlogits->sizes() == logits.sizes() && is_bf16(*dlogits) == is_bf16(logits)); }
  const DeviceGuard guard(logits.device());
  dm::cross_entropy_mix(logits.data_ptr(), (const long long*)ya.data_ptr(),
                        (const long long*)yb.data_ptr(), lam.data_ptr<float>(),
                        rowloss.data_ptr<float>(), loss.data_ptr<float>(),
                        dlogits.has_value() ? dlogits->data_ptr() : nullptr, logits.size(0),
                        logits.size(1), (float)scale, (float)eps, -100, is_bf16(logits),
                        cur_stream());
}

// counts: int64[3] = {n, top-1 hits, top-k hits}; loss: float64[1]; both accumulate
void eval_metrics(at::Tensor logits, at::Tensor labels, at::Tensor rowloss, at::Tensor rowrank,
                  int64_t k, at::Tensor counts, at::Tensor loss) {
  check_act(logits, "logits");
  TORCH_CHECK(logits.dim() == 2 && labels.scalar_type() == at::kLong && labels.numel() == logits.size(0));
  TORCH_CHECK(labels.is_cuda() && labels.is_contiguous(), "labels: contiguous device tensor");
  TORCH_CHECK(logits.size(0) >= 1 && logits.size(1) >= 1 && logits.size(0) < (1ll << 31) &&
              logits.size(1) < (1ll << 31), "logits: empty or too large");
  TORCH_CHECK(rowloss.is_cuda() && rowloss.is_contiguous(), "rowloss: contiguous device tensor");
  TORCH_CHECK(k >= 1 && k < 0x7fffffff, "k must be >= 1");
  CHECK_F32(rowloss);
  TORCH_CHECK(rowrank.is_cuda() && rowrank.is_contiguous() && rowrank.scalar_type() == at::kInt);
  TORCH_CHECK(rowloss.numel() >= logits.size(0) && rowrank.numel() >= logits.size(0));
  TORCH_CHECK(counts.is_cuda() && counts.is_contiguous() && counts.scalar_type() == at::kLong &&
              counts.numel() >= 3, "counts: int64[3]");
  TORCH_CHECK(loss.is_cuda() && loss.is_contiguous() && loss.scalar_type() == at::kDouble &&
              loss.numel() >= 1, "loss: float64[1]");
  const DeviceGuard guard(logits.device());
  dm::eval_metrics(logits.data_ptr(), (const long long*)labels.data_ptr(), rowloss.data_ptr<float>(),
                   rowrank.data_ptr<int>(), logits.size(0), logits.size(1), (int)k,
                   (long long*)counts.data_ptr(), loss.data_ptr<double>(), is_bf16(logits),
                   cur_stream());
}

void spin_us(double us) { dm::spin_us(us, cur_stream()); }

// (N,H,W,C) view of an image batch: a contiguous (N,H,W,C) tensor or a channels_last
// (N,C,H,W) one, C = 1 or 3 -> sizes {N,H,W,C}
std::array<int64_t, 4> aug_nhwc(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.dim() == 4, name, ": expected a 4-D image batch");
  const auto c1 = t.size(1), c3 = t.size(3);
  if ((c1 == 1 || c1 == 3) && t.permute({0, 2, 3, 1}).is_contiguous())
    return {t.size(0), t.size(2), t.size(3), c1};
  TORCH_CHECK((c3 == 1 || c3 == 3) && t.is_contiguous(), name,
              ": expected (N,H,W,C) contiguous or (N,C,H,W) channels_last with C = 1 or 3");
  return {t.size(0), t.size(1), t.size(2), c3};
}

// What augment_apply and augment_mix_apply check of their common arguments; the sizes of the
// (N,H,W,C) views of images and out
struct AugArgs {
  std::array<int64_t, 4> is, os;
  int64_t B;
  int dtype;
};
AugArgs aug_check(const at::Tensor& images, const at::Tensor& idx, const at::Tensor& params,
                  const at::Tensor& out, const char* fn) {
  CHECK_CUDA(images); CHECK_CUDA(idx); CHECK_CUDA(params); CHECK_CUDA(out);
  TORCH_CHECK(images.device() == idx.device() && images.device() == params.device() &&
              images.device() == out.device(), fn, ": tensors on different devices");
  const auto st = images.scalar_type();
  TORCH_CHECK(st == at::kByte || st == at::kFloat || st == at::kBFloat16,
              "images must be uint8, float32 or bfloat16");
  TORCH_CHECK(out.scalar_type() == st, "out must have the dtype of images");
  const auto is = aug_nhwc(images, "images");
  const auto os = aug_nhwc(out, "out");
  TORCH_CHECK(idx.scalar_type() == at::kLong && idx.dim() == 1 && idx.is_contiguous(),
              "idx must be a contiguous int64 vector");
  const int64_t B = idx.numel();
  TORCH_CHECK(params.scalar_type() == at::kInt && params.dim() == 2 && params.size(0) == B &&
              params.size(1) == 8 && params.is_contiguous(), "params must be int32 [B,8]");
  CHECK_ALIGN16(params);
  TORCH_CHECK(os[0] == B && os[3] == is[3], "out must be (B,OH,OW,C) with the batch of idx and "
              "the channels of images");
  TORCH_CHECK(is[0] >= 1 && is[1] >= 1 && is[2] >= 1 && is[1] <= 16384 && is[2] <= 16384,
              "images: empty or larger than 16384 x 16384");
  TORCH_CHECK(os[1] >= 1 && os[2] >= 1 && os[1] <= 16384 && os[2] <= 16384,
              "out: empty or larger than 16384 x 16384");
  TORCH_CHECK(B < (1ll << 31) && B * os[1] * os[2] < (1ll << 38), "batch too large");
  const char* ib = static_cast<const char*>(images.data_ptr());
  const char* ob = static_cast<const char*>(out.data_ptr());
  const int64_t esz = images.element_size();
  const int64_t in_bytes = is[0] * is[1] * is[2] * is[3] * esz;
  const int64_t out_bytes = B * os[1] * os[2] * os[3] * esz;
  TORCH_CHECK(ob + out_bytes <= ib || ib + in_bytes <= ob, "out must not alias images");
  return {is, os, B, st == at::kByte ? 0 : st == at::kFloat ? 1 : 2};
}

// Gather + crop / resize / flip of a batch (csrc/augment.hip): out[b] = transform(params[b],
// images[idx[b]]).  No allocation, no synchronisation.
void augment_apply(at::Tensor images, at::Tensor idx, at::Tensor params, at::Tensor out) {
  const AugArgs a = aug_check(images, idx, params, out, "augment_apply");
  if (a.B == 0) return;
  const DeviceGuard guard(images.device());
  dm::augment_apply(images.data_ptr(), (const long long*)idx.data_ptr(), params.data_ptr<int>(),
                    out.data_ptr(), a.is[0], (int)a.is[1], (int)a.is[2], (int)a.is[3], (int)a.B,
                    (int)a.os[1], (int)a.os[2], a.dtype, cur_stream());
}

// The same with mixup / CutMix (csrc/augment_mix.hip): mix int32 [B,4] = partner, L, xbox, ybox.
void augment_mix_apply(at::Tensor images, at::Tensor idx, at::Tensor params, at::Tensor mix,
                       at::Tensor out) {
  const AugArgs a = aug_check(images, idx, params, out, "augment_mix_apply");
  CHECK_CUDA(mix);
  TORCH_CHECK(mix.device() == images.device(), "augment_mix_apply: tensors on different devices");
  TORCH_CHECK(mix.scalar_type() == at::kInt && mix.dim() == 2 && mix.size(0) == a.B &&
              mix.size(1) == 4 && mix.is_contiguous(), "mix must be int32 [B,4]");
  CHECK_ALIGN16(mix);
  if (a.B == 0) return;
  const DeviceGuard guard(images.device());
  dm::augment_mix_apply(images.data_ptr(), (const long long*)idx.data_ptr(),
                        params.data_ptr<int>(), mix.data_ptr<int>(), out.data_ptr(), a.is[0],
                        (int)a.is[1], (int)a.is[2], (int)a.is[3], (int)a.B, (int)a.os[1],
                        (int)a.os[2], a.dtype, cur_stream());
}

// One LeNet training step (csrc/lenet_fused.hip).  w: conv1.w, conv1.b, conv2.w, conv2.b,
// fc1.w, fc1.b, fc2.w, fc2.b (fp32 masters); off: flat-buffer offsets of fc2.w, fc2.b, fc1.w,
// fc1.b, conv2.w, conv2.b, conv1.w, conv1.b; p/mom given: the SGD update runs in the same
// dispatch as the gradient reduction (p = the flat fp32 parameters, mom its momentum buffer).
void lenet_fused_step(at::Tensor x, at::Tensor labels, std::vector<at::Tensor> w, at::Tensor rec,
                      at::Tensor cslab, at::Tensor rowloss, at::Tensor grad,
                      std::vector<int64_t> off, c10::optional<at::Tensor> p,
                      c10::optional<at::Tensor> mom, double lr, double momentum, double dampening,
                      double wd, double gscale, bool nesterov, bool first, at::Tensor loss,
                      c10::optional<at::Tensor> sidx, c10::optional<at::Tensor> cursor,
                      int64_t batch, c10::optional<at::Tensor> loss_sum,
                      c10::optional<at::Tensor> probe) {
  CHECK_CUDA(x); CHECK_CONTIG(x);
  TORCH_CHECK(x.dim() == 4 && x.size(1) == 1 && x.size(2) == 28 && x.size(3) == 28,
              "x: [B, 1, 28, 28]");
  TORCH_CHECK(x.scalar_type() == at::kFloat || x.scalar_type() == at::kBFloat16, "x: fp32 or bf16");
  // sidx given: x / labels are the whole device-resident dataset; this step's samples are rows
  // sidx[cursor*batch : (cursor+1)*batch] (sampler order), the cursor advancing on the device
  const bool indexed = sidx.has_value() && sidx->defined();
  const int B = indexed ? (int)batch : (int)x.size(0);
  int nbatch = 0;
  if (indexed) {
    CHECK_CUDA(*sidx); CHECK_CONTIG(*sidx);
    TORCH_CHECK(sidx->scalar_type() == at::kLong && batch >= 1, "sidx: int64 row indices");
    TORCH_CHECK(cursor.has_value() && cursor->is_cuda() && cursor->scalar_type() == at::kInt &&
                    cursor->numel() == 1, "cursor: int32 [1] on the device");
    nbatch = (int)(sidx->numel() / batch);
    TORCH_CHECK(nbatch >= 1, "sidx holds fewer than one batch");
    TORCH_CHECK(labels.numel() == x.size(0), "labels: one per dataset row");
  }
  TORCH_CHECK(B >= 1 && labels.is_cuda() && labels.scalar_type() == at::kLong &&
                  labels.is_contiguous() && (indexed || labels.numel() == B), "labels: int64 [B]");
  TORCH_CHECK(w.size() == 8 && off.size() == 8, "8 parameter tensors / offsets");
  const int64_t want[8] = {150, 6, 2400, 16, 48000, 120, 1200, 10};
  const float* wp[8];
  for (int i = 0; i < 8; ++i) {
    CHECK_CUDA(w[i]); CHECK_F32(w[i]); CHECK_CONTIG(w[i]);
    TORCH_CHECK(w[i].numel() == want[i], "parameter ", i, " has the wrong size");
    wp[i] = w[i].data_ptr<float>();
  }
  for (auto* t : {&rec, &cslab, &rowloss, &grad, &loss}) { CHECK_CUDA(*t); CHECK_F32(*t); CHECK_CONTIG(*t); }
  TORCH_CHECK(rec.numel() >= (int64_t)B * dm::lenet_record_floats() &&
                  cslab.numel() >= (int64_t)B * dm::lenet_slab_floats() && rowloss.numel() >= B &&
                  loss.numel() == 1, "workspace too small");
  const int64_t segn[8] = {1200, 10, 48000, 120, 2400, 16, 150, 6};
  int o[8];
  for (int i = 0; i < 8; ++i) {
    TORCH_CHECK(off[i] >= 0 && off[i] + segn[i] <= grad.numel(), "flat offset out of range");
    o[i] = (int)off[i];
  }
  float* pp = nullptr;
  float* mp = nullptr;
  if (p.has_value()) {
    CHECK_CUDA(*p); CHECK_F32(*p); CHECK_CONTIG(*p);
    TORCH_CHECK(p->numel() == grad.numel(), "p: the flat parameter buffer");
    pp = p->data_ptr<float>();
    if (momentum != 0.0) {
      TORCH_CHECK(mom.has_value() && mom->numel() == grad.numel() && mom->scalar_type() == at::kFloat,
                  "mom: the flat momentum buffer");
      mp = mom->data_ptr<float>();
    }
  }
  float* lsum = nullptr;
  if (loss_sum.has_value() && loss_sum->defined()) {
    CHECK_CUDA(*loss_sum); CHECK_F32(*loss_sum);
    TORCH_CHECK(loss_sum->numel() == 1, "loss_sum: fp32 [1] on the device");
    lsum = loss_sum->data_ptr<float>();
  }
  unsigned long long* pr = nullptr;
  if (probe.has_value() && probe->defined()) {  // phase timestamps (tools/lenet_phases.py)
    CHECK_CUDA(*probe); CHECK_CONTIG(*probe);
    TORCH_CHECK(probe->scalar_type() == at::kLong && probe->numel() >= (int64_t)B * dm::lenet_probe_stamps(),
                "probe: int64 [B * lenet_probe_stamps()]");
    pr = reinterpret_cast<unsigned long long*>(probe->data_ptr<int64_t>());
  }
  const DeviceGuard guard(x.device());
  dm::lenet_fused_step(x.data_ptr(), x.scalar_type() == at::kBFloat16,
                       reinterpret_cast<const long long*>(labels.data_ptr<int64_t>()),
                       B, wp, rec.data_ptr<float>(), cslab.data_ptr<float>(),
                       rowloss.data_ptr<float>(), grad.data_ptr<float>(), o, pp, mp, (float)lr,
                       (float)momentum, (float)dampening, (float)wd, (float)gscale, nesterov,
                       first, pp != nullptr, loss.data_ptr<float>(),
                       indexed ? reinterpret_cast<const long long*>(sidx->data_ptr<int64_t>()) : nullptr,
                       indexed ? cursor->data_ptr<int>() : nullptr, x.size(0), nbatch, lsum,
                       cur_stream(), pr);
}

}  // namespace

void register_resnet(pybind11::module_& m);
void register_reducer(pybind11::module_& m);

// generated per build by dmlab/_build.py (build/native/source_hash.cpp): sha256 of the csrc/
// tree and build configuration this library was linked from
extern "C" const char* dmlab_source_hash();

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("source_hash", []() { return std::string(dmlab_source_hash()); },
        "sha256 of the csrc/ sources + build flags this extension was built from");
  register_resnet(m);
  register_reducer(m);
  m.doc() = "dmlab native HIP kernels for MI355X (gfx950)";
  m.def("sgd_step", &sgd_step, "fused flat SGD/GD step");
  m.def("adam_step", &adam_step, "fused flat Adam step");
  m.def("cast_f32_bf16", &cast_f32_bf16, "fp32 -> bf16 cast");
  m.def("rows_mean", &rows_mean, "[rows,N] -> [N] scaled row sum");
  m.def("q8_payload_bytes", [](int64_t n) { return (int64_t)dm::q8_payload_bytes(n); },
        "bytes of one rank's q8 payload for n gradient elements");
  m.def("q8_encode", &q8_encode, "fp32 slice (+ residual) -> q8 payload (scales, int8 codes)",
        py::arg("g"), py::arg("r"), py::arg("payload"), py::arg("max_blocks") = 0);
  m.def("q8_decode_mean", &q8_decode_mean, "[ws, payload] -> scale * sum of decoded rows",
        py::arg("gathered"), py::arg("out"), py::arg("scale"), py::arg("max_blocks") = 0);
  m.def("topk_payload_bytes", &topk_payload_bytes,
        "bytes of one rank's topk payload for n gradient elements, keep entries per 2048-block",
        py::arg("n"), py::arg("keep"));
  m.def("topk_encode", &topk_encode,
        "fp32 slice (+ residual) -> topk payload (fp32 values, uint16 in-block indices)",
        py::arg("g"), py::arg("r"), py::arg("payload"), py::arg("keep"),
        py::arg("max_blocks") = 0);
  m.def("topk_decode_mean", &topk_decode_mean,
        "[ws, payload] -> scale * sum over rows of the listed values, every element written",
        py::arg("gathered"), py::arg("out"), py::arg("keep"), py::arg("scale"),
        py::arg("max_blocks") = 0);
  m.def("lars_chunk", &dm::lars_chunk, "elements per LARS chunk (compile-time constant)");
  m.def("lars_table", &lars_table, "host-validated LARS segment/chunk tables (CPU int64)",
        py::arg("offsets"), py::arg("numels"), py::arg("adapted"), py::arg("total"));
  m.def("lars_step", &lars_step, "fused flat LARS step (3 launches)", py::arg("w"),
        py::arg("g"), py::arg("buf"), py::arg("seg"), py::arg("chunks"), py::arg("hyper"),
        py::arg("partial"), py::arg("tot"), py::arg("stats"), py::arg("gnorm"),
        py::arg("nesterov"), py::arg("launches") = 7);
  m.def("conv_small_fwd", &conv_small_fwd);
  m.def("conv_small_bwd", &conv_small_bwd);
  m.def("conv_small_workspace", &conv_small_workspace);
  m.def("gemm", &gemm, py::arg("A"), py::arg("Amask"), py::arg("B"), py::arg("C"), py::arg("C32"),
        py::arg("bias"), py::arg("M"), py::arg("N"), py::arg("K"), py::arg("sam"), py::arg("sak"),
        py::arg("sbk"), py::arg("sbn"), py::arg("scm"), py::arg("alpha"), py::arg("beta"),
        py::arg("relu"), py::arg("lowp") = false);
  m.def("gemm_plan", &gemm_plan, py::arg("M"), py::arg("N"), py::arg("K"), py::arg("a_bf16"),
        py::arg("lowp"));
  m.def("colsum", &colsum);
  m.def("bias_act", &bias_act, py::arg("y"), py::arg("bias"), py::arg("out"), py::arg("relu"));
  m.def("cu_mask_stream", &cu_mask_stream);
  m.def("cu_mask_of", &cu_mask_of);
  m.def("xgmi_alloc", &xgmi_alloc);
  m.def("xgmi_free", &xgmi_free);
  m.def("xgmi_get_handle", &xgmi_get_handle);
  m.def("xgmi_open_handle", &xgmi_open_handle);
  m.def("xgmi_close_handle", &xgmi_close_handle);
  m.def("xgmi_allreduce", &xgmi_allreduce, py::arg("in"), py::arg("out"), py::arg("cap"),
        py::arg("data"), py::arg("flags"), py::arg("rank"), py::arg("scale"), py::arg("state"),
        py::arg("algo"), py::arg("share") = 1);
  m.def("p2p_xgmi_send", &p2p_xgmi_send);
  m.def("p2p_xgmi_recv", &p2p_xgmi_recv);
  m.def("cross_entropy", &cross_entropy);
  m.def("argmax_count", &argmax_count);
  m.def("cross_entropy_smooth", &cross_entropy_smooth);
  m.def("cross_entropy_mix", &cross_entropy_mix);
  m.def("eval_metrics", &eval_metrics);
  m.def("spin_us", &spin_us);
  m.def("augment_apply", &augment_apply);
  m.def("augment_mix_apply", &augment_mix_apply);
  m.def("lenet_fused_step", &lenet_fused_step, "one fused LeNet training step (2 dispatches)",
        py::arg("x"), py::arg("labels"), py::arg("w"), py::arg("rec"), py::arg("cslab"),
        py::arg("rowloss"), py::arg("grad"), py::arg("off"), py::arg("p"), py::arg("mom"),
        py::arg("lr"), py::arg("momentum"), py::arg("dampening"), py::arg("wd"),
        py::arg("gscale"), py::arg("nesterov"), py::arg("first"), py::arg("loss"),
        py::arg("sidx") = py::none(), py::arg("cursor") = py::none(), py::arg("batch") = 0,
        py::arg("loss_sum") = py::none(), py::arg("probe") = py::none());
  m.def("lenet_record_floats", &dm::lenet_record_floats);
  m.def("lenet_slab_floats", &dm::lenet_slab_floats);
  m.def("lenet_probe_stamps", &dm::lenet_probe_stamps);
  m.attr("arch") = "gfx950";
}
