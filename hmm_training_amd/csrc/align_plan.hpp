// align_plan.hpp — the host-side plan of hmmbw_align (align.hip): forced alignment is the hard-decision
// counterpart of the embedded E-step on the same chain, so the lane-group width (one lane per transcript
// position), the table layout (EmbedTab, here holding logarithms), where the emission table lives and the checks
// of the transcripts are embed_plan.hpp's, and the checks of the bank wordnet_plan.hpp's.  What is new here: the
// size of a back-pointer row and of the workspace, and the checks of the flags and of the output lengths.  Plain
// C++17 with no HIP dependency, so that a host compiler can build a probe of it (tests/native/align_plan_probe.cpp).
// The per-slot output offsets and the per-wave back-pointer row offsets are plan_viterbi_group's
// (viterbi_plan.hpp) with this group width.
#pragma once

#include "embed_plan.hpp"

namespace hmmbw {

constexpr int kAlMaxWords = kEmMaxWords;    // words of a bank, and positions of a transcript: one lane each
constexpr int kAlMaxStates = kEmMaxStates;  // a lane keeps its instance's deltas and a dense log A (N^2) in registers
constexpr int kAlFlags = 1 | 2;             // HMMBW_ALIGN_END_FINAL | HMMBW_ALIGN_DENSE (include/hmmbw.h)

// lane-group width: the smallest of 8, 16, 32, 64 that holds the longest transcript (lane l = position l)
constexpr int align_gw(int max_words) { return embed_gw(max_words); }
// the log tables: log pi [W][NP] | log A [W][N][N] | log B [K][W][NP], EmbedTab's indexing; states >= N hold -inf
constexpr EmbedTab align_tab(int W, int N, int K) { return embed_tab(W, N, K); }

// Back-pointers of one (step, decoding wave): 64 lanes x 4 bytes, a nibble per state: bits 0-2 the within-word
// predecessor i, bit 3 the entry arc.  The entry source is always (l - 1, N - 1): no source byte.
constexpr int kAlRowBytes = kVitWave * 4;
static_assert(kAlMaxStates * 4 <= 32, "a nibble per state in one 32-bit word");
static_assert(kAlMaxStates <= 8, "three bits of predecessor");
constexpr size_t align_bp_bytes(long long rows) { return (size_t)rows * kAlRowBytes; }

// With optional positions (hmmbw_align_optional) the entry arc has two possible sources, (l - 1, N - 1) and, past
// an optional position, (l - 2, N - 1).  Both carry the weight log pi_{w_l}[j], so which one wins does not depend
// on j: one bit per lane and step.  At N = 8 the nibble word is full, so the bits of a (step, wave) row go to a
// 64-bit lane mask of their own, bit = lane of the wave, 1 = the source two positions back.
constexpr int kAlSkipRowBytes = 8;
static_assert(kAlSkipRowBytes * 8 == kVitWave, "a bit per lane of the wave");
constexpr size_t align_skip_bytes(long long rows) { return (size_t)rows * kAlSkipRowBytes; }

constexpr bool align_flags_ok(int flags) { return (flags & ~kAlFlags) == 0; }

// the output lengths: 0 ok, 1 path_len is not the number of loaded symbols, 2 bounds_len is not the number of
// transcript positions (checked whether or not the outputs are asked for)
constexpr int align_lengths_check(long long path_len, long long total, long long bounds_len, long long n_positions) {
    return path_len != total ? 1 : bounds_len != n_positions ? 2 : 0;
}

}  // namespace hmmbw
