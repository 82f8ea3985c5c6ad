// wordnet_plan.hpp — the host-side plan of hmmbw_wordnet_decode (wordnet.hip): the lane-group width (one lane per
// word), the layout of the log tables, where the emission table lives, the size of a back-pointer row, and the
// checks of the bank the entry point makes before it launches.  Plain C++17 with no HIP dependency, so that a
// host compiler can build a probe of it (tests/native/wordnet_plan_probe.cpp).  The per-slot output offsets and
// the per-wave back-pointer row offsets are plan_viterbi_group's (viterbi_plan.hpp) with this group width.
#pragma once

#include "viterbi_plan.hpp"

namespace hmmbw {

constexpr int kWnMaxWords = 64;   // one lane per word, one wave per group at most
constexpr int kWnMaxStates = 8;   // a lane keeps its word's deltas (and a dense log A, N^2 values) in registers

// lane-group width: the smallest of 8, 16, 32, 64 that holds the words (lane w = word w)
constexpr int wordnet_gw(int W) { return viterbi_gv(W); }
// a lane's N values of one table row, padded so that they load as 16-B pairs
constexpr int wordnet_np(int N) { return N <= 1 ? 1 : N <= 2 ? 2 : N <= 4 ? 4 : 8; }

// The log tables, offsets in doubles; words >= W and states >= N hold log 0 = -inf
struct WordnetTab {
    long long pi = 0;     // [GW][NP]       log pi_w[j]
    long long init = 0;   // [GW]           log init_w
    long long A = 0;      // [GW][N][N]     log a_w[i][j], row-major
    long long G = 0;      // [GW w][GW v]   log G[v][w]: lane w's column contiguous (all 0 = log 1 without word_trans)
    long long B = 0;      // [K][GW][NP]    log b_w,j(k): a lane's values for one symbol contiguous
    long long total = 0;
};
constexpr WordnetTab wordnet_tab(int GW, int N, int K) {
    WordnetTab t;
    t.pi = 0;
    t.init = t.pi + (long long)GW * wordnet_np(N);
    t.A = t.init + GW;
    t.G = t.A + (long long)GW * N * N;
    t.B = (t.G + (long long)GW * GW + 1) / 2 * 2;  // 16-B aligned rows
    t.total = t.B + (long long)K * GW * wordnet_np(N);
    return t;
}

// the bank as the entry point stages it for the prep kernel (linear doubles): pi [W][N] | A [W][N][N] |
// B [W][N][K] | init [W] | G [W][W]
constexpr long long wordnet_in_len(int W, int N, int K) {
    return (long long)W * N + (long long)W * N * N + (long long)W * N * K + W + (long long)W * W;
}

// The emission table goes into LDS when it fits the decoder's budget (viterbi_plan.hpp: 64 KiB, no raised
// dynamic-LDS limit); otherwise it stays in global memory, read through L2.
constexpr size_t wordnet_emis_bytes(int K, int GW, int N) { return (size_t)K * GW * wordnet_np(N) * sizeof(double); }
constexpr bool wordnet_emis_in_lds(int K, int GW, int N) { return wordnet_emis_bytes(K, GW, N) <= kVitLdsBudget; }

// Back-pointers of one (step, decoding wave): 64 lanes x 4 bytes (a nibble per state: bits 0-2 the within-word
// predecessor i, bit 3 the entry arc) and 64 lanes x 1 byte (the entry source word v)
constexpr int kWnRowBytes = kVitWave * 4 + kVitWave;

// every A of the bank left-to-right (a_ij = 0 unless j = i or j = i + 1)?
inline bool wordnet_is_lr(const double *A, int W, int N) {
    for (long long w = 0; w < W; ++w)
        for (int i = 0; i < N; ++i)
            for (int j = 0; j < N; ++j)
                if (j != i && j != i + 1 && A[(w * N + i) * N + j] != 0.0) return false;
    return true;
}

// n finite non-negative numbers (no NaN)?
inline bool wordnet_weights_ok(const double *x, long long n) {
    for (long long i = 0; i < n; ++i)
        if (!(x[i] >= 0.0 && x[i] <= 1.7976931348623157e308)) return false;
    return true;
}

}  // namespace hmmbw
