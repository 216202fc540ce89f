// Host-side launcher declarations for every dmlab HIP kernel.
// All launchers are allocation-free and sync-free (hipGraph-capturable).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "conv_cfg.h"
#include "conv_geom.h"

namespace dm {
typedef unsigned short bf16_t;

// optim.hip
void sgd_step(float* p, const float* g, float* mom, bf16_t* pbf, long long n, float lr,
              float momentum, float dampening, float wd, float gscale, bool nesterov,
              bool first, hipStream_t st);
void adam_step(float* p, const float* g, float* m, float* v, bf16_t* pbf, long long n,
               float lr, float b1, float b2, float eps, float wd, float gscale, float bc1,
               float bc2, hipStream_t st);
void cast_f32_bf16(const float* x, bf16_t* y, long long n, hipStream_t st);
void rows_mean(const float* x, float* out, int rows, long long n, float scale,
               hipStream_t st);

// gradq.hip: "q8" block-wise int8 gradient codec (blocks of 256 from the slice's start).
// payload = ceil(n/256) fp32 scales, n int8 codes, padding to 16 bytes (q8_payload_bytes);
// r = nullptr: no error feedback.  gathered holds ws payloads row_bytes apart;
// out = scale * sum over rows of code*scale in row order.  max_blocks > 0 caps the grid.
long long q8_payload_bytes(long long n);
void q8_encode(const float* g, float* r, uint8_t* payload, long long n, int max_blocks,
               hipStream_t st);
void q8_decode_mean(const uint8_t* gathered, long long row_bytes, int ws, float* out,
                    long long n, float scale, int max_blocks, hipStream_t st);

// gradk.hip: "topk" block-wise gradient sparsification (blocks of 2048 from the slice's start,
// the `keep` = 1..256 largest magnitudes of each).  payload = nb*keep fp32 values, nb*keep
// uint16 in-block indices, padding to 16 bytes (topk_payload_bytes); r = nullptr: no error
// feedback, otherwise r = 0 at the sent positions and g + r elsewhere.  gathered holds ws
// payloads row_bytes apart; out = scale * sum over rows, in row order, of the listed values,
// every element written.  max_blocks > 0 caps the grid.
int topk_block();
int topk_max_keep();
long long topk_payload_bytes(long long n, int keep);
void topk_encode(const float* g, float* r, uint8_t* payload, long long n, int keep,
                 int max_blocks, hipStream_t st);
void topk_decode_mean(const uint8_t* gathered, long long row_bytes, int ws, float* out,
                      long long n, int keep, float scale, int max_blocks, hipStream_t st);

// lars.hip: fused LARS step over the flat buffers (3 launches).  seg [n_tensors,5] and
// chunks [n_chunks,3] are the int64 device tables described there; hyper holds
// lars_hyper_count() floats (lr, momentum, weight decay, trust coefficient, eps,
// grad_scale, max_grad_norm or <= 0); partial [n_chunks,2] and tot [n_tensors,2] are
// workspaces; stats [n_tensors,3] and gnorm [1] are outputs.
// launches: bit 0 partial sums, bit 1 per-tensor totals, bit 2 update (7 = the step; a subset only
// to time the launches one by one, tools/bench_optim.py).
int lars_chunk();
int lars_hyper_count();
void lars_step(float* w, const float* g, float* buf, long long total, const long long* seg,
               int n_tensors, const long long* chunks, int n_chunks, const float* hyper,
               float* partial, float* tot, float* stats, float* gnorm, bool nesterov,
               int launches, hipStream_t st);

}  // namespace dm

namespace dm {
// conv_small.hip  (NCHW, tiny channel counts; x/y/dx fp32 or bf16, weights fp32)
void conv_small_fwd(const void* x, const float* w, const float* bias, void* y, uint8_t* mask,
                    int B, int Cin, int H, int W, int Cout, int K, int pad, int pool, int relu,
                    bool bf16, hipStream_t st);
void conv_small_bwd(const void* x, const float* w, const void* dp, const void* yp,
                    const uint8_t* mask, void* dx, float* dw, float* db, float* work, int B,
                    int Cin, int H, int W, int Cout, int K, int pad, int pool, int relu,
                    float beta, int bs, bool bf16, hipStream_t st);
// dynamic LDS the backward-data kernel asks for, and the most a launch on the current device gets
size_t conv_small_bwd_data_lds(int Cout, int K, int OH, int OW);
size_t conv_small_lds_limit();
// gemm.hip
// split-K decision of one GEMM shape: part holds S slabs of M*N floats, block z of `chunks`
// reduces k in [z*kchunk, (z+1)*kchunk).  S == 1: no split (kchunk = K, chunks = 1)
struct GemmPlan { int S, kchunk, chunks; };
GemmPlan gemm_plan(long long M, long long N, long long K, int a_bf16, int lowp);
void gemm_strided(const void* A, const void* Amask, int a_bf16, const void* B, int b_bf16,
                  void* C, int c_bf16, float* C32, const float* bias, int M, int N, int K,
                  long long sam, long long sak, long long sbk, long long sbn, long long scm,
                  float alpha, float beta, int relu, int lowp, float* part,
                  const GemmPlan& plan, hipStream_t st);
void bias_act(const float* y, const float* bias, void* out, int out_bf16, int M, int N, int relu,
              hipStream_t st);
void colsum(const void* A, const void* Amask, int bf16, float* out, int M, int N, float beta,
            hipStream_t st);
// loss.hip
void cross_entropy(const void* logits, const long long* labels, float* rowloss, float* loss,
                   void* dlogits, int B, int C, float scale, int ignore_index, bool bf16,
                   hipStream_t st);
void argmax_count(const void* logits, const long long* labels, int B, int C,
                  unsigned long long* correct, bool bf16, hipStream_t st);
// label-smoothed cross-entropy (eps in [0, 1]); same two launches as cross_entropy
void cross_entropy_smooth(const void* logits, const long long* labels, float* rowloss, float* loss,
                          void* dlogits, int B, int C, float scale, float eps, int ignore_index,
                          bool bf16, hipStream_t st);
// mixed-target cross-entropy: the target of a row is lam*smooth(ya) + (1-lam)*smooth(yb)
void cross_entropy_mix(const void* logits, const long long* ya, const long long* yb,
                       const float* lam, float* rowloss, float* loss, void* dlogits, int B, int C,
                       float scale, float eps, int ignore_index, bool bf16, hipStream_t st);
// per-row NLL + label rank (B floats / B ints of scratch), then counts[3] = {n, top-1 hits,
// top-k hits} and loss[1] (float64 sum) updated in fixed order
void eval_metrics(const void* logits, const long long* labels, float* rowloss, int* rowrank, int B,
                  int C, int k, long long* counts, double* loss, bool bf16, hipStream_t st);
void spin_us(double us, hipStream_t st);
// augment.hip: gather + crop / resize / flip of a batch in one launch.  images (N,H,W,C), C = 1
// or 3; params int32 [B,8] (16-B aligned); out (B,OH,OW,C); dtype 0 = u8, 1 = fp32, 2 = bf16
void augment_apply(const void* images, const long long* idx, const int* params, void* out,
                   long long N, int H, int W, int C, int B, int OH, int OW, int dtype,
                   hipStream_t st);
// augment_mix.hip: the same launch with mixup / CutMix: mix int32 [B,4] = partner, L, xbox, ybox
// (16-B aligned); sample b is blended with, or has a box pasted from, batch row `partner`
void augment_mix_apply(const void* images, const long long* idx, const int* params, const int* mix,
                       void* out, long long N, int H, int W, int C, int B, int OH, int OW,
                       int dtype, hipStream_t st);
// lenet_fused.hip: the whole LeNet training step in 2 dispatches
int lenet_record_floats();
int lenet_slab_floats();
void lenet_fused_step(const void* x, bool x_bf16, const long long* labels, int B,
                      const float* const* w, float* rec, float* cslab, float* rowloss, float* grad,
                      const int* off, float* p, float* mom, float lr, float momentum,
                      float dampening, float wd, float gscale, bool nesterov, bool first,
                      bool do_sgd, float* loss, const long long* sidx, int* cursor,
                      long long nrows, int nbatch, float* loss_sum, hipStream_t st,
                      unsigned long long* probe = nullptr);
int lenet_probe_stamps();
}  // namespace dm

namespace dm {
// comm_xgmi.hip
void* xgmi_alloc(size_t bytes);
void xgmi_free(void* ptr);
void xgmi_get_handle(void* ptr, void* handle64);
void* xgmi_open_handle(const void* handle64);
void xgmi_close_handle(void* ptr);
void xgmi_allreduce(const float* in, float* out, long long n, long long cap, void* const* data,
                    void* const* flags, int rank, int W, float scale, unsigned* state, int algo,
                    hipStream_t st, int share = 1);
// p2p_xgmi.hip: one-direction stage-to-stage channel over IPC peer memory
void p2p_xgmi_send(const void* src, long long bytes, void* ring, void* full, const void* free_,
                   long long slot_bytes, int nslot, unsigned* state, hipStream_t st);
void p2p_xgmi_recv(void* dst, long long bytes, const void* ring, const void* full, void* free_,
                   long long slot_bytes, int nslot, unsigned* state, hipStream_t st);
// ---- the conv launches; every `cfg` below is an id / a row of csrc/conv_cfg.h
struct BnBwdRed;
// sched: the pipelined tiles' schedule (the other kernels have none).  kPipeAuto = the launcher
// decides (conv_pipe_plan.h), 0 = the data-parallel launch, G > 0 = the balanced schedule on G
// workgroups wherever it is eligible (tests and A/B runs)
constexpr int kPipeAuto = -1;
// The operands of a forward-style conv GEMM (forward, stride-1 dgrad, the parity classes of a
// stride-2 dgrad); everything after Y is optional.  add: added to the result; stats [T][2][Cout]:
// the BatchNorm batch statistics; pre_sc / pre_sh: X is staged as relu(X*pre_sc + pre_sh); red:
// the consumer BatchNorm's backward sums in the epilogue (one part row per block, class-major);
// seg2: a second K segment of geometry seg2->z (a 1x1/s2 projection's data gradient merged into
// the stride-2 dgrad's parity class (0,0))
struct ConvOperands {
  const bf16_t *X, *Wp;
  bf16_t* Y;
  int sched;
  const bf16_t* add;
  float* stats;
  const float *pre_sc, *pre_sh;
  const BnBwdRed* red;
  const DgradSeg2* seg2;
};
// The operands of a weight gradient into S fp32 slabs [Cout][K] (rows split in chunks of mchunk)
struct WgradOperands {
  const bf16_t *X, *DY;
  float* slab;
  int S;
  long long mchunk;
  const float *pre_sc, *pre_sh;
};
// conv_launch.cpp: the dispatcher.  The one place that evaluates the *_supported predicates,
// asks conv_cfg.h's route functions and names a family's launcher; a refused route throws
// std::runtime_error.  conv_launch_multi: up to four geometries sharing X / W / Y (the parity
// classes of a stride-2 dgrad) in one launch, or one launch per class (data-parallel schedule)
// where the row has none; false = refused (a merged segment / RED needs the single launch).
// dry: the route (conv_cfg.h) is reported there and nothing is launched
void conv_launch(const ConvOperands& ops, const ConvGeom& g, const ConvCfg& cfg, hipStream_t st,
                 ConvRoute* dry = nullptr);
bool conv_launch_multi(const ConvOperands& ops, const ConvGeomSet& gs, int ng, const ConvCfg& cfg,
                       hipStream_t st, ConvRoute* dry = nullptr);
void wgrad_launch(const WgradOperands& ops, const ConvGeom& g, const WgradCfg& cfg, hipStream_t st,
                  WgradRoute* dry = nullptr);
// statistics / part rows a single-geometry launch of this row writes (one per row tile, or per
// workgroup of the persistent res64 kernel), and the part rows of the classes' single launch with
// RED (class major, row tile minor; every block writes its row); 0 if the row has no such launch
long long conv_stats_rows(long long M, const ConvCfg& cfg);
long long conv_multi_red_rows(const ConvGeomSet& gs, int ng, const ConvCfg& cfg);
// compute units of the current device (cached per device): the grid limit of the persistent
// kernels (res64, stem, the pipelined tiles' balanced schedule); defined next to the dispatcher
int device_cu_count();
// conv_igemm.hip: the igemm tiles (cfg: an igemm row; ng geometries, blockIdx.z = geometry) and
// the v2 weight-gradient tiles
void igemm_tile(const ConvOperands& ops, const ConvGeomSet& gs, int ng, const ConvCfg& cfg,
                hipStream_t st);
void wgrad_tile(const WgradOperands& ops, const ConvGeom& g, const WgradCfg& cfg, hipStream_t st);
// conv_stem.hip: s2d stem (16 channels, 16 taps, 64 outputs) with resident weights (cfg 60)
bool stem_conv_supported(const ConvGeom& g);
void stem_conv(const ConvOperands& ops, const ConvGeom& g, const ConvCfg& cfg, hipStream_t st);
// fused stem BN backward (quad max-pool gather) + s2d weight gradient -> slabs [S][64][256]
bool stem_wgrad_fused_supported(int N, int H, int W, int C, int Cpad);
int stem_wgrad_fused_blocks(int N, int H);
void stem_wgrad_fused(const bf16_t* xs, const bf16_t* y, const bf16_t* pdy, const uint8_t* pidx,
                      const float* coef, const float* sc, const float* sh, float* slab, int N,
                      int H, int W, int S, hipStream_t st);
// stem_fused.hip: K-dense fused stem (raw-input gather + 7x7/s2 conv + BN statistics + pooled
// extremum), pooled BN apply, backward (y recomputed, dy = a dz + b y + cc) wgrad, reduce
bool stem_fused_supported(int Hin, int Win);
int stem_fused_grid(int N);
int stem_slab_cols();
int stem_wk_cols();
void stem_fwd_fused(const void* img, int dtype, const long long* idx, const float* nsc,
                    const float* nbi, const bf16_t* wk, const float* gamma, bf16_t* pext,
                    uint8_t* code, float* stats, int N, int nimg, int Hin, int Win, int grid,
                    hipStream_t st);
void stem_pool_apply(const bf16_t* pext, const uint8_t* code, const float* scale,
                     const float* shift, bf16_t* out, uint8_t* code4, long long n, hipStream_t st);
void stem_bwd_fused2(const void* img, int dtype, const long long* idx, const float* nsc,
                     const float* nbi, const bf16_t* wk, const bf16_t* pdy, const uint8_t* code4,
                     float* dslab, float* gslab, int N, int nimg, int Hin, int Win, int grid,
                     hipStream_t st);
void stem_wcombine(const float* dslab, const float* gslab, int GD, const bf16_t* wk,
                   const float* coef, float* sums, float* dw, float beta, hipStream_t st);
int stem_gram_cols();
int stem_sums_len();
void stem_pack_weights(const float* w, bf16_t* wk, hipStream_t st);
// The BatchNorm backward reduction of the layer whose output gradient a data gradient
// produces, done in that dgrad's epilogue: with dz = Y * relu-mask (mask from y*sc + sh > 0,
// or the 1-bit `mask` when set), part[wg][0][c] = Σ dz and part[wg][1][c] = Σ dz (y - mu) is
// (one row per workgroup, the pre-reduced rows bn_bwd_finalize / bn_bwd_sums consume)
struct BnBwdRed {
  const bf16_t* y;
  const uint8_t* mask;
  const float *sc, *sh, *mu, *is;
  float* part;
};
// conv_pipe.hip: pipelined LDS-DMA implicit-GEMM conv (cfg 90-93: 256-pixel tiles); ng
// geometries (blockIdx.y = geometry), no statistics with more than one
bool conv_pipe_supported(const ConvGeom& g, int cfg);
void conv_pipe(const ConvOperands& ops, const ConvGeomSet& gs, int ng, const ConvCfg& cfg,
               hipStream_t st);
// The balanced schedule's workspace of one (device, stream), owned by the bindings: `cap` slots
// of 256 x 256 fp32 accumulators, `cap` flag words and the timeout word, all zero at first; seq
// is this launch's sequence number (a host counter per workspace, never 0), so that no word is
// ever reset: a flag of an earlier launch cannot match.  Null slots = none (data-parallel).
struct PipeWorkspace {
  float* slots;
  unsigned* flags;
  unsigned* timeout;
  unsigned seq;
  int cap;
};
using PipeWorkspaceFn = PipeWorkspace (*)(hipStream_t st, int cap);
void conv_pipe_set_workspace(PipeWorkspaceFn fn);
// conv_res64.hip: persistent register-resident-weight 3x3 conv, 64 -> 64 channels (cfg 80);
// statistics rows = res64_grid(M) (one per workgroup)
bool conv_res64_supported(const ConvGeom& g);
int res64_grid(long long M);
void conv_res64(const ConvOperands& ops, const ConvGeom& g, const ConvCfg& cfg, hipStream_t st);
// conv_halo.hip: halo-staged unit-stride tiles (the row's bn / halo_waves select the tile)
bool conv_halo_supported(const ConvGeom& g);
void conv_halo(const ConvOperands& ops, const ConvGeom& g, const ConvCfg& cfg, hipStream_t st);
// wgrad_halo.hip: halo-staged 3x3 unit-stride weight gradient (wgrad cfg 4, 5: taps per block)
bool wgrad_halo_supported(const ConvGeom& g);
void wgrad_halo(const WgradOperands& ops, const ConvGeom& g, const WgradCfg& cfg, hipStream_t st);
// stride-2 3x3 weight gradient over the four input parity planes (wgrad cfg 7)
bool wgrad_s2_supported(const ConvGeom& g);
void wgrad_s2(const WgradOperands& ops, const ConvGeom& g, const WgradCfg& cfg, hipStream_t st);
// wgrad_res64.hip: row-streaming 64 -> 64 channel 3x3 weight gradient (wgrad cfg 8); S slabs
bool wgrad_res64_supported(const ConvGeom& g);
void wgrad_res64(const WgradOperands& ops, const ConvGeom& g, const WgradCfg& cfg, hipStream_t st);
void pack_weights_tiled(const long long* desc, const int* tprefix, int nl, int ntiles,
                        hipStream_t st);
void wgrad_reduce(const float* slab, int S, int Cout, int C, int Cin, int KH, int KW, float* dw,
                  float beta, hipStream_t st);
void pack_weights(const float* w, bf16_t* wf, bf16_t* wd, int Cout, int Cin, int Cpad, int KH,
                  int KW, hipStream_t st);
// bn_pool.hip
void bn_stats_finalize(const float* stats, int T, int C, double count, const float* gamma,
                       const float* beta, float* rmean, float* rvar, float momentum, float eps,
                       float* scale, float* shift, float* mean, float* invstd, float* work, long long* num_batches,
                       hipStream_t st);
void bn_eval_coeffs(const float* gamma, const float* beta, const float* rmean, const float* rvar,
                    float eps, int C, float* scale, float* shift, hipStream_t st);
void bn_apply(const bf16_t* y, const bf16_t* res, const float* scale, const float* shift,
              bf16_t* out, long long n, int C, bool relu, hipStream_t st, uint8_t* mask = nullptr);
// BatchNorm backward, as the steps the bindings chain: reduce -> finalize -> apply; across
// ranks reduce -> sums, the all-reduce of sums [2C] float64, then coefficients -> apply.
// dz = the upstream gradient under the ReLU mask; its source is the kernels' MODE:
//   0 Plain    dout tensor, no ReLU
//   1 OutMask  dout tensor, mask from the saved output (out > 0)          -- residual layers
//   2 YMask    dout tensor, mask recomputed from y (y*scale + shift > 0)   -- no `out` read
//   3 Pool     gathered from a following max-pool's grads + argmax codes, mask from y
//              (stem: neither `out` nor the unpooled gradient is ever materialised)
//   4 BitMask  dout tensor, mask from the forward's 1-bit (out > 0) mask    -- residual layers
enum class BnDz { Plain, OutMask, YMask, Pool, BitMask };
// which half of a cross-rank backward a caller asks for (Sums writes sums, Apply reads them)
enum class BnStage { Whole, Sums, Apply };
struct BnBwdArgs {
  const bf16_t* dout;
  const bf16_t* out;
  const bf16_t* y;
  const float* mean;
  const float* invstd;
  const float* scale;   // forward BN scale/shift (modes 2, 3)
  const float* shift;
  const bf16_t* pdy;    // mode 3: pooled-output gradient [N][OH][OW][C]
  const uint8_t* pidx;  //         argmax codes (kh*K + kw), same shape
  int H, W, OH, OW, K, S, P;
  long long M;
  int C;
  const uint8_t* mask;  // mode 4: bit j of byte i = (out > 0) of chunk i, channel j
};
// The workspace of one backward: part [rows][2C] (the reduce's partial rows; rows = 0 when they
// come pre-reduced from a producing kernel, or the sums from the other ranks), coef [3C]
// (dy = a dz + b y + cc), part2 [<= 256][2C] (the finalize's second-level partials)
struct BnBwdWork { float *part, *coef, *part2; };
inline long long bn_bwd_work_floats(int rows, int C) { return (2LL * rows + 3 + 2 * 256) * C; }
inline BnBwdWork bn_bwd_carve(float* work, int rows, int C) {
  float* coef = work + 2LL * rows * C;
  return {work, coef, coef + 3 * C};
}
int bn_bwd_groups(long long M, int C);
// rows the reduce writes.  dres (the apply also emits the residual branch's dz) only enters
// through the choice of the stem's quad kernels, which the reduce and the apply must make alike
int bn_bwd_rows(BnDz src, const BnBwdArgs& a, bool dres);
// part [rows][2C] = partial Σdz, Σdz·x̂ over a's M rows; returns rows
int bn_bwd_reduce(BnDz src, const BnBwdArgs& a, bool dres, float* part, hipStream_t st);
// dgamma / dbeta (gbeta: accumulate) and coef from the partial rows of M elements per channel
void bn_bwd_finalize(const float* part, int rows, long long M, int C, const float* gamma,
                     const float* mean, const float* invstd, float* dgamma, float* dbeta,
                     float gbeta, float* coef, float* part2, hipStream_t st);
// cross-rank: dgamma / dbeta from this rank's rows and sums [2C] float64 out; then coef from the
// sums of all ranks and the device scalar total (Σ of the ranks' M)
void bn_bwd_sums(const float* part, int rows, int C, float* dgamma, float* dbeta, float gbeta,
                 double* sums, float* part2, hipStream_t st);
void bn_bwd_coef(const double* sums, const double* total, const float* gamma, const float* mean,
                 const float* invstd, int C, float* coef, hipStream_t st);
// dy = a dz + b y + cc, and dres = dz when set
void bn_bwd_apply(BnDz src, const BnBwdArgs& a, const float* coef, bf16_t* dy, bf16_t* dres,
                  hipStream_t st);
// cross-rank BatchNorm forward: this rank's float64 row [mean (C) | M2 (C) | n] from its
// statistics slab; then the merge of all ranks' rows [ws][2C+1] in rank order (total = Σn)
void bn_sync_local(const float* stats, int T, int C, double count, double* row, float* work,
                   hipStream_t st);
void bn_sync_finalize(const double* rows, int ws, int C, const float* gamma, const float* beta,
                      float* rmean, float* rvar, float momentum, float eps, float* scale,
                      float* shift, float* mean, float* invstd, long long* num_batches,
                      double* total, hipStream_t st);
void bn_relu_maxpool(const bf16_t* y, const float* scale, const float* shift, bf16_t* out,
                     uint8_t* idx, int N, int H, int W, int C, int OH, int OW, int K, int S,
                     int P, hipStream_t st, bf16_t* yarg = nullptr);
void maxpool_fwd(const bf16_t* x, bf16_t* y, uint8_t* idx, int N, int H, int W, int C, int OH,
                 int OW, int K, int S, int P, hipStream_t st);
void maxpool_bwd(const bf16_t* dy, const uint8_t* idx, bf16_t* dx, int N, int H, int W, int C,
                 int OH, int OW, int K, int S, int P, hipStream_t st);
void avgpool_fwd(const bf16_t* x, bf16_t* y, int N, int HW, int C, hipStream_t st);
void avgpool_bwd(const bf16_t* dy, bf16_t* dx, int N, int HW, int C, hipStream_t st);
void pack_input(const void* x, bool bf16, bf16_t* y, int N, int C, int H, int W, int Cp,
                long long sn, long long sc, long long sh, long long sw, hipStream_t st);
void pack_input_s2d(const void* x, bool bf16, bf16_t* y, int N, int C, int H2, int W2, int Cp,
                    long long sn, long long sc, long long sh, long long sw, const long long* idx,
                    long long nsrc, hipStream_t st);
void pack_weights_s2d(const float* w, bf16_t* wf, int Cout, int C, int Cp, hipStream_t st);
void wgrad_reduce_s2d(const float* slab, int S, int Cout, int C, int Cp, float* dw, float beta,
                      hipStream_t st);
}  // namespace dm
