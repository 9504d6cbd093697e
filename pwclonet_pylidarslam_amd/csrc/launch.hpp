// Host-side launch policy of the fused stack kernels (fused_layers.hip, fused_hoisted.hip, fused_sa.hip): the
// PWCLO_* switches, the size of a packed stack per weight format, the runtime-format -> template-argument
// dispatch and the persistent-grid launcher (on launch_grid, common.hpp).  No device code lives here.
#pragma once
#include <type_traits>

#include "mlp_core.hpp"

namespace pwclo {

// PWCLO_* switches of the stack kernels (tuning(): common.hpp), each read once per process.
static inline int fl_wide() { static const int v = tuning("PWCLO_FL_WIDE", 1); return v; }        // 16-wave workgroups
static inline int fl_stagger() { static const int v = tuning("PWCLO_FL_STAGGER", 0); return v; }  // mlp_core.hpp: stagger_start
static inline int coarse_w4() { static const int v = tuning("PWCLO_COARSE_W4", 1); return v; }

// Largest launch (in wave tiles) that still takes the 4-wave workgroup variants of the point-wise / coarse-level kernels.  Narrow
// workgroups reach more CUs -- lower latency of a lone forward (batch 1: +7 %, batch 4: +5 %) -- but every workgroup stages the
// stack's 100-160 KB of weights again, which costs CU-time: in the pipelined batch-32 run the launches of exactly 2048 tiles
// (level-2 flow predictors) are better off wide (+0.3 %, profiles/r03/r03_v7_ab_coarse_w4.txt); smaller ones stay narrow.
static inline int coarse_tiles() { static const int v = tuning("PWCLO_COARSE_W4_TILES", 2047); return v; }

// Wave tiles of a launch: b clouds of s queries with kp pixel slots each, cut into tiles of p 16-pixel blocks.
static inline long long stack_tiles(int b, int s, int kp, int p) {
  return (long long)b * (((long long)s * kp + 16 * p - 1) / (16 * p));
}

// A packed stack as its layers' (input blocks, output blocks) pairs, e.g. Stack<1, 8, 8, 4, 4, 4> for
// geometry -> 128 -> 64 -> 64: floats / bytes the stack occupies when packed in format FMT (layer_floats_any).
template <int... D> struct Stack {
  template <int FMT = 0> static constexpr int floats() { return 0; }
};
template <int NBI, int NBO, int... Rest> struct Stack<NBI, NBO, Rest...> {
  template <int FMT = 0> static constexpr int floats() {
    return layer_floats_any<FMT>(NBI, NBO) + Stack<Rest...>::template floats<FMT>();
  }
  template <int FMT = 0> static constexpr int bytes() { return 4 * floats<FMT>(); }
};

// Calls f(std::integral_constant<int, FMT>) for the runtime weight format wfmt (validated by PWCLO_REQUIRE_PACKED).
template <int V> using int_c = std::integral_constant<int, V>;
template <typename F> static inline void with_format(int wfmt, F &&f) {
  if (wfmt == PWCLO_WFMT_BF16X3) f(int_c<PWCLO_WFMT_BF16X3>{});
  else if (wfmt == PWCLO_WFMT_BF16) f(int_c<PWCLO_WFMT_BF16>{});
  else f(int_c<PWCLO_WFMT_F32>{});
}

// The format of a packed weight buffer is a property of the BUFFER, fixed when it was packed (fused.py records it
// on the packed object): the stack launchers take it as an explicit argument `wfmt` together with the buffer's
// length in floats, and refuse a length that does not match the layout the selected kernel will index
// (a buffer packed in one format and launched as the other would otherwise be read out of bounds, silently).
// STACK: the Stack<...> type of the wrapper's kernels.
#define PWCLO_REQUIRE_PACKED(what, wfmt, packed_floats, STACK)                                                   \
  do {                                                                                                           \
    PWCLO_REQUIRE((wfmt) >= PWCLO_WFMT_F32 && (wfmt) <= PWCLO_WFMT_BF16, what ": unknown weight format %d",        \
                  (int)(wfmt));                                                                                  \
    int expect_ = 0;                                                                                             \
    with_format(wfmt, [&](auto fmt_) { expect_ = STACK::template floats<decltype(fmt_)::value>(); });            \
    PWCLO_REQUIRE((packed_floats) == expect_, what ": packed weights hold %d floats, format %d needs %d",          \
                  (int)(packed_floats), (int)(wfmt), expect_);                                                   \
  } while (0)

// Persistent grid over ntiles wave tiles: one workgroup per W tiles, at most 256 CUs x per_cu resident workgroups x
// rounds.  Workgroups beyond one resident set queue behind it; >1 "rounds" keeps the kernel balanced when part of the
// chip is held by another stream's kernels (e.g. the other in-flight batch's FPS).  The two rules in use:
struct GridRule {
  int rounds;        // default of PWCLO_FL_ROUNDS
  bool wide_alone;   // a workgroup of more than 8 waves has its CU to itself whatever its LDS size
};
constexpr GridRule STACK_GRID{1, true};    // fused_layers.hip, fused_hoisted.hip
constexpr GridRule SA_GRID{2, false};      // fused_sa.hip: per_cu from the LDS size alone, two rounds

template <auto Kern, int W, typename Args>
static void launch_persistent(int lds_bytes, long long ntiles, const Args &a, GridRule rule = STACK_GRID) {
  static const int rounds = tuning("PWCLO_FL_ROUNDS", rule.rounds);
  const int per_cu = (lds_bytes > 80 * 1024 || (rule.wide_alone && W > 8)) ? 1 : 2;
  long long grid = (ntiles + W - 1) / W;
  if (grid > 256LL * per_cu * rounds) grid = 256LL * per_cu * rounds;
  if (grid < 1) grid = 1;
  launch_grid<Kern, W>(dim3((unsigned)grid), lds_bytes, a);
}

}  // namespace pwclo
