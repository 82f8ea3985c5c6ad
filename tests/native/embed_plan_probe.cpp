// Host probe of the embedded trainer's plan (hmm_training_amd/csrc/embed_plan.hpp and plan_viterbi_group of
// viterbi_plan.hpp), built by tests/test_embedded.py with the host compiler and the address / undefined-behaviour
// sanitizers:
//   embed_plan_probe W N K U longest len_0 len_1 ...
// lays the sequences out as hmmbw_set_observations does (obs_plan.hpp, plan_layout) and prints the plan:
//   fig GW spw nslots nvw rows | work_off .. | tab pi A B total np bank_len | stats entry xi gall bnum total
//   | place in_lds bytes | work row_doubles bytes | state bytes chunk
//   | check (of a good CSR, an empty transcript, an id = W, an id < 0, offsets not from 0) | longest | count ..
#include <cstdio>
#include <cstdlib>

#include "../../hmm_training_amd/csrc/embed_plan.hpp"
#include "../../hmm_training_amd/csrc/obs_plan.hpp"

using namespace hmmbw;

static_assert(embed_gw(1) == 8 && embed_gw(8) == 8 && embed_gw(9) == 16 && embed_gw(16) == 16, "GW");
static_assert(embed_gw(17) == 32 && embed_gw(32) == 32 && embed_gw(33) == 64 && embed_gw(64) == 64, "GW");
static_assert(embed_np(1) == 1 && embed_np(2) == 2 && embed_np(3) == 4 && embed_np(5) == 8 && embed_np(8) == 8, "NP");
// the LDS decision at its boundary: 64 KiB = 8192 doubles = K W NP
static_assert(embed_emis_in_lds(32, 32, 8) && !embed_emis_in_lds(33, 32, 8), "K at the boundary");
static_assert(embed_emis_in_lds(256, 4, 8) && !embed_emis_in_lds(256, 5, 8) && embed_emis_in_lds(256, 8, 4), "W at the boundary");
static_assert(embed_emis_bytes(256, 64, 8) == (size_t(1) << 20) && !embed_emis_in_lds(256, 64, 8), "the 1 MB table");
static_assert(embed_tab(3, 3, 4).B % 2 == 0 && embed_tab(1, 1, 7).B % 2 == 0 && embed_tab(5, 5, 7).B % 2 == 0, "16-B aligned rows");
static_assert(embed_stats(3, 3, 4).total - embed_stats(3, 3, 4).bnum == embed_tab(3, 3, 4).total - embed_tab(3, 3, 4).B,
              "b_num is indexed as the emission table");
static_assert(embed_row_doubles(5) == 320 && embed_work_bytes(10, 8) == 10 * 8 * 64 * 8, "a workspace row");

template <class T>
static void row(const char *tag, const std::vector<T> &v) {
    std::printf("%s", tag);
    for (const T &x : v) std::printf(" %lld", (long long)x);
    std::printf("\n");
}

int main(int argc, char **argv) {
    if (argc < 6) return 2;
    const int W = std::atoi(argv[1]), N = std::atoi(argv[2]), K = std::atoi(argv[3]), U = std::atoi(argv[4]);
    const int longest = std::atoi(argv[5]);
    std::vector<int> len;
    for (int i = 6; i < argc; ++i) len.push_back(std::atoi(argv[i]));
    const ObsLayout L = plan_layout(len, U, false, 0);
    const int GW = embed_gw(longest);
    const ViterbiPlan P = plan_viterbi_group(L.slot_len, L.slot_seq, L.R, GW);
    std::printf("fig %d %d %lld %lld %lld\n", P.GV, P.spw, P.nslots, P.nvw, P.psi_rows);
    row("slot_len", L.slot_len);
    row("work_off", P.psi_off);
    const EmbedTab t = embed_tab(W, N, K);
    std::printf("tab %lld %lld %lld %lld %d %lld\n", t.pi, t.A, t.B, t.total, embed_np(N), embed_bank_len(W, N, K));
    const EmbedStats s = embed_stats(W, N, K);
    std::printf("stats %lld %lld %lld %lld %lld\n", s.entry, s.xi, s.gall, s.bnum, s.total);
    std::printf("place %d %zu\n", embed_emis_in_lds(K, W, N) ? 1 : 0, embed_emis_bytes(K, W, N));
    std::printf("work %lld %zu\n", embed_row_doubles(N), embed_work_bytes(P.psi_rows, N));
    std::printf("state %zu %d\n", sizeof(EmbedState), kEmChunk);
    // transcripts: R = 3 of lengths longest, 1, 2 over the words 0 .. W-1 in turn
    std::vector<int64_t> off = {0, longest, longest + 1, longest + 3};
    std::vector<int32_t> ids((size_t)longest + 3);
    for (size_t i = 0; i < ids.size(); ++i) ids[i] = (int32_t)(i % (size_t)W);
    std::vector<long long> count((size_t)W, -1);
    long long lg = -1, tmp = 0;
    const int good = embed_transcripts_check(off.data(), ids.data(), 3, W, &lg, count.data());
    std::vector<int64_t> empty = {0, longest, longest, longest + 3};
    const int e1 = embed_transcripts_check(empty.data(), ids.data(), 3, W, &tmp, nullptr);
    std::vector<int32_t> big = ids, neg = ids;
    big.back() = W;
    neg[0] = -1;
    const int e2 = embed_transcripts_check(off.data(), big.data(), 3, W, &tmp, nullptr);
    const int e3 = embed_transcripts_check(off.data(), neg.data(), 3, W, &tmp, nullptr);
    std::vector<int64_t> shifted = {1, longest, longest + 1, longest + 3};
    const int e4 = embed_transcripts_check(shifted.data(), ids.data(), 3, W, &tmp, nullptr);
    const int e5 = embed_transcripts_check(off.data(), ids.data(), 0, W, &tmp, nullptr);
    std::printf("check %d %d %d %d %d %d\n", good, e1, e2, e3, e4, e5);
    std::printf("longest %lld\n", lg);
    row("count", count);
    return 0;
}
