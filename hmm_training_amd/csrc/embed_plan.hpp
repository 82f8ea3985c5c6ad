// embed_plan.hpp — the host-side plan of hmmbw_embedded_train (embedded.hip): the lane-group width (one lane per
// transcript position), the layout of the parameter tables and of the statistics, where the emission table lives,
// the size of the forward workspace, the device-side training state, and the checks of the bank and of the
// transcripts the entry point makes before it launches.  Plain C++17 with no HIP dependency, so that a host
// compiler can build a probe of it (tests/native/embed_plan_probe.cpp).  The per-wave workspace row offsets are
// plan_viterbi_group's (viterbi_plan.hpp) with this group width; the bank checks are wordnet_plan.hpp's.
#pragma once

#include "wordnet_plan.hpp"

namespace hmmbw {

constexpr int kEmMaxWords = kWnMaxWords;    // words of a bank, and positions of a transcript: one lane each
constexpr int kEmMaxStates = kWnMaxStates;  // a lane keeps its instance's alpha, beta, xi (N^2) and a dense A (N^2)
constexpr int kEmChunk = 16;                // iterations enqueued between two reads of the device state

// lane-group width: the smallest of 8, 16, 32, 64 that holds the longest transcript (lane l = position l)
constexpr int embed_gw(int max_words) { return viterbi_gv(max_words); }
constexpr int embed_np(int N) { return wordnet_np(N); }

// The parameter tables, offsets in doubles, linear; states >= N hold 0.  Lanes gather by their word id, so the
// tables hold W words, not a group's width.
struct EmbedTab {
    long long pi = 0;   // [W][NP]
    long long A = 0;    // [W][N][N]   a_w[i][j], row-major
    long long B = 0;    // [K][W][NP]  b_w,j(k): a lane's values for one symbol contiguous, 16-B aligned
    long long total = 0;
};
constexpr EmbedTab embed_tab(int W, int N, int K) {
    EmbedTab t;
    t.pi = 0;
    t.A = t.pi + (long long)W * embed_np(N);
    t.B = (t.A + (long long)W * N * N + 1) / 2 * 2;
    t.total = t.B + (long long)K * W * embed_np(N);
    return t;
}

// The statistics, offsets in doubles; a_den is the row sum of xi, formed by the M-step
struct EmbedStats {
    long long entry = 0;  // [W][N]
    long long xi = 0;     // [W][N][N]
    long long gall = 0;   // [W][N]
    long long bnum = 0;   // [K][W][NP]: the emission table's own indexing
    long long total = 0;
};
constexpr EmbedStats embed_stats(int W, int N, int K) {
    EmbedStats s;
    s.entry = 0;
    s.xi = s.entry + (long long)W * N;
    s.gall = s.xi + (long long)W * N * N;
    s.bnum = s.gall + (long long)W * N;
    s.total = s.bnum + (long long)K * W * embed_np(N);
    return s;
}

// the bank as the entry point stages it (and reads it back): pi [W][N] | A [W][N][N] | B [W][N][K]
constexpr long long embed_bank_len(int W, int N, int K) {
    return (long long)W * N + (long long)W * N * N + (long long)W * N * K;
}

// The emission table goes into LDS when it fits the decoders' budget (viterbi_plan.hpp), else it is read through L2
constexpr size_t embed_emis_bytes(int K, int W, int N) { return (size_t)K * W * embed_np(N) * sizeof(double); }
constexpr bool embed_emis_in_lds(int K, int W, int N) { return embed_emis_bytes(K, W, N) <= kVitLdsBudget; }

// The forward workspace: per (step, decoding wave) a row of N x 64 doubles, [j][lane]
constexpr long long embed_row_doubles(int N) { return (long long)N * kVitWave; }
constexpr size_t embed_work_bytes(long long rows, int N) { return (size_t)rows * embed_row_doubles(N) * sizeof(double); }

// The device-side state of a call: the convergence state of hmm_training.py:503-514 and the records of the
// iterations since the host last looked (record r of the call sits in slot r % kEmChunk)
struct EmbedState {
    double prev_L, last_L, last_diff, epsilon;
    long long iteration, max_iterations;
    int done, converged;
    double ring[2 * kEmChunk];  // (L, diff)
};

// transcripts as CSR: 0 ok, 1 an empty transcript, 2 a word id outside [0, W), 3 offsets that do not start at 0 or
// decrease; *longest gets the longest transcript's length, count[w] (W entries, or nullptr) the instances of w
inline int embed_transcripts_check(const int64_t *off, const int32_t *ids, long long R, int W, long long *longest,
                                   long long *count) {
    *longest = 0;
    if (count) std::fill(count, count + W, 0LL);
    if (R > 0 && off[0] != 0) return 3;
    for (long long r = 0; r < R; ++r) {
        const long long n = off[r + 1] - off[r];
        if (n < 0) return 3;
        if (n == 0) return 1;
        *longest = std::max(*longest, n);
        for (long long p = off[r]; p < off[r + 1]; ++p) {
            if (ids[p] < 0 || ids[p] >= W) return 2;
            if (count) ++count[ids[p]];
        }
    }
    return 0;
}

// Optional transcript positions (hmmbw_embedded_train_optional, hmmbw_align_optional): opt has one byte per
// position in the CSR order of ids, or is nullptr (no optional position).  A path may pass over a position with
// opt = 1.  0 ok, 1 a flag other than 0 or 1, 2 two adjacent optional positions, 3 a transcript without a mandatory
// position.  Call after embed_transcripts_check has accepted the offsets.  mand[w] (W entries, or nullptr) gets the
// mandatory instances of w, which without flags is embed_transcripts_check's count[w].
inline int embed_optional_check(const int64_t *off, const int32_t *ids, const uint8_t *opt, long long R, int W,
                                long long *mand) {
    if (mand) std::fill(mand, mand + W, 0LL);
    for (long long r = 0; r < R; ++r) {
        long long mandatory = 0;
        for (long long p = off[r]; p < off[r + 1]; ++p) {
            const int f = opt ? opt[p] : 0;
            if (f > 1) return 1;
            if (f && p > off[r] && opt[p - 1]) return 2;
            if (!f) {
                ++mandatory;
                if (mand) ++mand[ids[p]];
            }
        }
        if (mandatory == 0) return 3;
    }
    return 0;
}

// The statistics of the optional path follow EmbedStats' block, which keeps its layout: present [W], the summed
// entry mass of the optional instances of a word (the M-step adds it to the word's mandatory count for the
// denominator of pi), and touched [W], nonzero once an M-step has re-estimated the word (a word whose denominator
// stayed 0 throughout keeps the caller's parameters bit for bit)
constexpr long long embed_present_off(int W, int N, int K) { return embed_stats(W, N, K).total; }
constexpr long long embed_touched_off(int W, int N, int K) { return embed_present_off(W, N, K) + W; }
constexpr long long embed_stats_optional_total(int W, int N, int K) { return embed_touched_off(W, N, K) + W; }

}  // namespace hmmbw
