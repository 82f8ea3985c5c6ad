// viterbi_plan.hpp — the host-side plan of hmmbw_viterbi (viterbi.hip): the lane-group width, where the
// log-emission table lives, what the symbol packs must be divided by, and the per-slot output offsets and
// per-wave back-pointer offsets of the loaded observations.  Plain C++17 with no HIP dependency, so that a
// host compiler can build a probe of it (tests/native/viterbi_plan_probe.cpp).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace hmmbw {

constexpr int kVitWave = 64;
constexpr int kVitBlock = 256;  // threads per decoding workgroup (4 waves)

// lane-group width of the decoder: the smallest of 8, 16, 32, 64 that holds the states (lane j = state j)
constexpr int viterbi_gv(int N) { return N <= 8 ? 8 : N <= 16 ? 16 : N <= 32 ? 32 : 64; }

// The log B^T table [K][GV] of doubles goes into LDS when it fits this budget: 64 KiB leaves a CU's 160 KiB
// room for two workgroups and needs no raised dynamic-LDS limit.  N = 64, K = 1024 (512 KiB) stays in global
// memory.
constexpr size_t kVitLdsBudget = size_t(64) << 10;
constexpr size_t viterbi_table_bytes(int K, int GV) { return (size_t)K * GV * sizeof(double); }
constexpr bool viterbi_table_in_lds(int K, int GV) { return viterbi_table_bytes(K, GV) <= kVitLdsBudget; }

// What a pack entry must be divided by to give the symbol: the packs hold symbol * (LDS row stride of the
// E-step's emission tables) when those tables live in LDS (hmmbw_ctx::lds_tables), symbol ids otherwise.
constexpr long long viterbi_pack_div(bool lds_tables, int G, int tab_pad) {
    return lds_tables ? (long long)(G + tab_pad) * 16 : 1;
}
// log2 of the divisor when it is a power of two (the kernel then shifts), -1 otherwise
constexpr int viterbi_pack_shift(long long div) {
    if (div <= 0 || (div & (div - 1)) != 0) return -1;
    int s = 0;
    while ((1LL << s) < div) ++s;
    return s;
}

struct ViterbiPlan {
    int GV = 8, spw = 8;            // lane-group width | slots per decoding wave (64 / GV)
    long long nslots = 0, nvw = 0;  // layout slots (padding included) | decoding waves
    long long total = 0;            // symbols of all sequences = entries of the path
    std::vector<long long> slot_out;  // slot -> first entry of its sequence in the caller's CSR order (-1: padding)
    std::vector<long long> psi_off;   // decoding wave -> its first back-pointer row ([t][64 lanes] bytes per wave)
    long long psi_rows = 0;           // rows of all decoding waves
};

// slot_len / slot_seq: the observation layout's slot arrays (obs_plan.hpp: 0 / -1 in padding slots); R sequences.
// The output offsets are the prefix sum of the lengths in caller order; a decoding wave holds spw consecutive
// slots and as many back-pointer rows as its longest slot has steps.
// plan_viterbi_group takes the lane-group width itself (8, 16, 32 or 64): the word-loop decoder's groups hold
// words, not states (wordnet_plan.hpp).
inline ViterbiPlan plan_viterbi_group(const std::vector<int> &slot_len, const std::vector<int> &slot_seq, long long R,
                                      int GV) {
    ViterbiPlan P;
    P.GV = GV;
    P.spw = kVitWave / P.GV;
    P.nslots = (long long)slot_len.size();
    P.nvw = (P.nslots + P.spw - 1) / P.spw;
    std::vector<long long> off((size_t)R + 1, 0);
    for (long long s = 0; s < P.nslots; ++s)
        if (slot_seq[(size_t)s] >= 0) off[(size_t)slot_seq[(size_t)s] + 1] = slot_len[(size_t)s];
    for (long long r = 0; r < R; ++r) off[(size_t)r + 1] += off[(size_t)r];
    P.total = off[(size_t)R];
    P.slot_out.assign((size_t)P.nslots, -1);
    for (long long s = 0; s < P.nslots; ++s)
        if (slot_seq[(size_t)s] >= 0) P.slot_out[(size_t)s] = off[(size_t)slot_seq[(size_t)s]];
    P.psi_off.assign((size_t)P.nvw, 0);
    for (long long w = 0; w < P.nvw; ++w) {
        int Tw = 0;
        for (long long s = w * P.spw; s < std::min((w + 1) * P.spw, P.nslots); ++s) Tw = std::max(Tw, slot_len[(size_t)s]);
        P.psi_off[(size_t)w] = P.psi_rows;
        P.psi_rows += Tw;
    }
    return P;
}

inline ViterbiPlan plan_viterbi(const std::vector<int> &slot_len, const std::vector<int> &slot_seq, long long R, int N) {
    return plan_viterbi_group(slot_len, slot_seq, R, viterbi_gv(N));
}

}  // namespace hmmbw
