// Stand-alone check of the pipelined conv's balanced schedule (csrc/conv_pipe_plan.h), plain
// host C++: over a sweep of (T tiles, S K steps, G workgroups) the ranges cover every
// (tile, K step) exactly once, in order, no tile has more than two contributors, a range is
// [tail of a started tile] [whole tiles] [head of a tile the next workgroup finishes], and the
// eligibility rule refuses what the kernel cannot run.  Prints "ok" or the first failure.
#include <cstdio>
#include <vector>

#include "../../csrc/conv_pipe_plan.h"

using namespace dm;

static int fail(const char* what, long long T, int S, int G, long long v) {
  std::printf("FAIL %s: T=%lld S=%d G=%d (%lld)\n", what, T, S, G, v);
  return 1;
}

static int check(long long T, int S, int G) {
  std::vector<int> hits((size_t)(T * S), 0), contrib((size_t)T, 0);
  long long next = 0, longest = 0;
  for (int w = 0; w < G; ++w) {
    const PipeRange r = pipe_range(T, S, G, w);
    if (r.k0 != next) return fail("ranges are not contiguous", T, S, G, w);
    if (r.k1 < r.k0 || r.k1 > T * S) return fail("range bounds", T, S, G, w);
    next = r.k1;
    const long long len = r.k1 - r.k0;
    longest = len > longest ? len : longest;
    if (len < T * S / G || len > T * S / G + 1) return fail("range length", T, S, G, w);
    if (len > T * S / G && w >= T * S % G) return fail("the extra step goes to the first", T, S, G, w);
    long long last_tile = -1;
    for (long long k = r.k0; k < r.k1; ++k) {
      ++hits[(size_t)k];
      if (k / S != last_tile) ++contrib[(size_t)(k / S)], last_tile = k / S;
    }
    // the kernel's decomposition: tail of tA from kA, whole tiles, head of tB up to kB
    const long long tA = r.k0 / S, kA = r.k0 % S, tB = r.k1 / S, kB = r.k1 % S;
    if (pipe_balanced_eligible(T, S, G, 1, false)) {
      if (kA > 0 && tB <= tA) return fail("a tail that is not finished in its range", T, S, G, w);
      if (kA > 0 && w == 0) return fail("workgroup 0 has a predecessor", T, S, G, w);
      if (kB > 0 && w == G - 1) return fail("the last workgroup has a successor", T, S, G, w);
      long long steps = (kA > 0 ? S - kA : 0) + kB;
      for (long long t = tA + (kA > 0 ? 1 : 0); t < tB; ++t) steps += S;
      if (steps != len) return fail("decomposition length", T, S, G, w);
    }
  }
  if (next != T * S) return fail("ranges do not reach the end", T, S, G, next);
  for (long long k = 0; k < T * S; ++k)
    if (hits[(size_t)k] != 1) return fail("a K step not covered exactly once", T, S, G, k);
  if (longest != pipe_balanced_steps(T, S, G)) return fail("pipe_balanced_steps", T, S, G, longest);
  if (pipe_balanced_eligible(T, S, G, 1, false)) {
    for (long long t = 0; t < T; ++t)
      if (contrib[(size_t)t] < 1 || contrib[(size_t)t] > 2)
        return fail("contributors of a tile", T, S, G, t);
    if (T * S / G < S || T <= G) return fail("eligible but q < S or T <= G", T, S, G, 0);
  }
  return 0;
}

int main() {
  for (long long T = 1; T <= 40; ++T)
    for (int S : {1, 2, 3, 4, 9, 36, 72})
      for (int G = 1; G <= 24; ++G)
        if (check(T, S, G)) return 1;
  // the two real shapes (ResNet-18 layers 3 and 4 at 1024 images) and the test shapes
  const long long real[][3] = {{784, 36, 256}, {392, 72, 256}, {784, 2, 256}, {5, 36, 4},
                               {5, 36, 3}, {8, 72, 5}, {4, 36, 2}, {5, 4, 4}, {1568, 9, 304}};
  for (auto& c : real)
    if (check(c[0], (int)c[1], (int)c[2])) return 1;
  // eligibility
  struct { long long T; int S, G, ng; bool seg2, want; } rules[] = {
      {784, 36, 256, 1, false, true},  {392, 72, 256, 1, false, true},
      {784, 36, 256, 2, false, false},  // several geometries
      {784, 36, 256, 4, false, false}, {784, 36, 256, 1, true, false},  // merged segment
      {256, 36, 256, 1, false, false},  // T == G: one round already
      {100, 36, 256, 1, false, false},  // T < G
      {5, 36, 4, 1, false, true},      {5, 36, 8, 1, false, false},
      {4, 36, 2, 1, false, true},      {8, 72, 5, 1, false, true},
      {5, 36, 0, 1, false, false},
  };
  for (auto& r : rules)
    if (pipe_balanced_eligible(r.T, r.S, r.G, r.ng, r.seg2) != r.want)
      return fail("eligibility", r.T, r.S, r.G, r.ng * 2 + r.seg2);
  // q < S cannot coexist with T > G (q = T S / G >= S); the rule still states it: whatever it
  // accepts has both
  for (long long T = 1; T <= 64; ++T)
    for (int S = 1; S <= 12; ++S)
      for (int G = 1; G <= 64; ++G)
        if (pipe_balanced_eligible(T, S, G, 1, false) && (T * S / G < S || T <= G))
          return fail("accepted q < S or T <= G", T, S, G, 0);
  // the automatic choice: both real 3x3 shapes win at 256 workgroups (111 + S / 3 steps against
  // 144), tiles shallower than the measured ones (a 1x1 projection, the 128-channel stride-2
  // forward) keep the data-parallel launch, an exact multiple of the grid has nothing to win
  if (pipe_balanced_wins(784, 18, 256)) return fail("S = 18 was not measured", 784, 18, 256, 0);
  if (!pipe_balanced_wins(784, 36, 256) || !pipe_balanced_wins(392, 72, 256))
    return fail("the real shapes must win", 784, 36, 256, 0);
  if (pipe_balanced_wins(784, 2, 256)) return fail("S = 2 must not win", 784, 2, 256, 0);
  if (pipe_balanced_wins(512, 36, 256)) return fail("whole rounds must not win", 512, 36, 256, 0);
  if (pipe_rounds_steps(784, 36, 256) != 144 || pipe_balanced_steps(784, 36, 256) != 111)
    return fail("step counts", 784, 36, 256, 0);
  std::printf("ok\n");
  return 0;
}
