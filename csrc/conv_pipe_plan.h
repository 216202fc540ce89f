// The balanced schedule of the pipelined conv (conv_pipe.hip): which K steps each workgroup of
// a persistent grid runs, and when a launch takes that schedule at all.  Host-only plain C++17
// (no HIP, no torch), like conv_cfg.h: the launcher reads it and tests/native/pipe_plan.cpp
// checks it on the CPU.  The kernel repeats pipe_range() with the same integers.
//
// A launch has T tiles (M tile major, N tile minor, so the N tiles of one M tile are adjacent and
// share their A rows through L2) of S K steps each, T*S steps in all.  Workgroup w of G runs the
// contiguous steps [w q + min(w, r), ...) of length q (+1 for the first r workgroups), q = T S / G,
// r = T S % G.  A range is the tail of a tile the previous workgroup started, whole tiles, and
// the head of a tile the next workgroup finishes; with q >= S no tile has a third contributor.
#pragma once

namespace dm {

struct PipeRange {
  long long k0, k1;  // global K steps [k0, k1); tile = k / S, step within the tile = k % S
};

inline PipeRange pipe_range(long long T, int S, int G, int w) {
  const long long tot = T * S, q = tot / G, r = tot % G;
  const long long b = w * q + (w < r ? w : r);
  return {b, b + q + (w < r ? 1 : 0)};
}

// K steps of the busiest workgroup: the data-parallel launch on G slots, and the balanced one
inline long long pipe_rounds_steps(long long T, int S, int G) { return (T + G - 1) / G * S; }
inline long long pipe_balanced_steps(long long T, int S, int G) { return (T * S + G - 1) / G; }

// What the balanced schedule can run: one geometry, no merged segment, more tiles than
// workgroups (else the data-parallel launch is one round already) and at least a tile's worth of
// steps per workgroup (so a tile never has more than two contributors)
inline bool pipe_balanced_eligible(long long T, int S, int G, int ng, bool seg2) {
  if (ng != 1 || seg2 || G < 1 || S < 1) return false;
  if (T <= G) return false;
  return T * S / G >= S;
}

// The automatic choice, settled from isolated timings on an MI355X at 1024 images
// (profiles/conv_pipe_balanced_iso_r7a.json; docs/KERNELS.md "Balanced schedule of the
// pipelined conv").  Against the data-parallel launch's own time per K step the balanced one
// ran as if its busiest workgroup had S / 3 more steps than its range: 12 at S = 36 (layer 3:
// 111 + 12 against 144, measured -15 % forward, -10 % data gradient), 24 at S = 72 (layer 4:
// 111 + 24 against 144, measured -6 %).  That is the two extra tile set-ups, prologues and the
// 256 KB accumulator hand-off of a range's head and tail.  The balanced launch is taken when
// this model still predicts kPipeMarginPct percent fewer steps than the rounds of the
// data-parallel launch, and only for tiles at least as deep as the shallowest one measured.
constexpr int kPipeMinSteps = 36;
constexpr int kPipeMarginPct = 5;
inline bool pipe_balanced_wins(long long T, int S, int G) {
  if (S < kPipeMinSteps) return false;
  const long long bal = pipe_balanced_steps(T, S, G) + S / 3;
  return bal * (100 + kPipeMarginPct) <= pipe_rounds_steps(T, S, G) * 100;
}

}  // namespace dm
