// Host probe of the aligner's plan (hmm_training_amd/csrc/align_plan.hpp and plan_viterbi_group of
// viterbi_plan.hpp), built by tests/test_align.py with the host compiler and the address / undefined-behaviour
// sanitizers:
//   align_plan_probe W N K U longest len_0 len_1 ...
// lays the sequences out as hmmbw_set_observations does (obs_plan.hpp, plan_layout) and prints the plan:
//   fig GW spw nslots nvw rows total | slot_len .. | slot_out .. | psi_off .. | tab pi A B total np bank_len
//   | place in_lds bytes | bp row_bytes bytes | flags ok(0) ok(1) ok(2) ok(3) ok(4) ok(-1)
//   | lengths (good, wrong path_len, wrong bounds_len, both wrong, both zero)
#include <cstdio>
#include <cstdlib>

#include "../../hmm_training_amd/csrc/align_plan.hpp"
#include "../../hmm_training_amd/csrc/obs_plan.hpp"

using namespace hmmbw;

static_assert(align_gw(1) == 8 && align_gw(8) == 8 && align_gw(9) == 16 && align_gw(16) == 16, "GW");
static_assert(align_gw(17) == 32 && align_gw(32) == 32 && align_gw(33) == 64 && align_gw(64) == 64, "GW");
static_assert(kAlMaxWords == 64 && kAlMaxStates == 8, "one lane per position, a nibble per state");
static_assert(kAlRowBytes == 256 && kAlRowBytes < kWnRowBytes, "no entry-source byte");
static_assert(align_bp_bytes(0) == 0 && align_bp_bytes(10) == 2560, "the workspace");
static_assert(align_bp_bytes((1LL << 23) + 1) == ((size_t(1) << 23) + 1) * 256, "rows past 2^31 bytes");
static_assert(align_tab(3, 3, 4).B == embed_tab(3, 3, 4).B && align_tab(5, 5, 7).total == embed_tab(5, 5, 7).total,
              "the trainer's table layout");
static_assert(align_flags_ok(0) && align_flags_ok(1) && align_flags_ok(2) && align_flags_ok(3), "known flags");
static_assert(!align_flags_ok(4) && !align_flags_ok(8 | 1) && !align_flags_ok(-1), "unknown flag bits");
static_assert(align_lengths_check(5, 5, 2, 2) == 0 && align_lengths_check(4, 5, 2, 2) == 1, "path_len");
static_assert(align_lengths_check(5, 5, 3, 2) == 2 && align_lengths_check(4, 5, 3, 2) == 1, "bounds_len, path_len first");

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
    long long total = 0;
    for (int i = 6; i < argc; ++i) {
        len.push_back(std::atoi(argv[i]));
        total += len.back();
    }
    const ObsLayout L = plan_layout(len, U, false, 0);
    const int GW = align_gw(longest);
    const ViterbiPlan P = plan_viterbi_group(L.slot_len, L.slot_seq, L.R, GW);
    std::printf("fig %d %d %lld %lld %lld %lld\n", P.GV, P.spw, P.nslots, P.nvw, P.psi_rows, P.total);
    row("slot_len", L.slot_len);
    row("slot_out", P.slot_out);
    row("psi_off", P.psi_off);
    const EmbedTab t = align_tab(W, N, K);
    std::printf("tab %lld %lld %lld %lld %d %lld\n", t.pi, t.A, t.B, t.total, embed_np(N), embed_bank_len(W, N, K));
    std::printf("place %d %zu\n", embed_emis_in_lds(K, W, N) ? 1 : 0, embed_emis_bytes(K, W, N));
    std::printf("bp %d %zu\n", kAlRowBytes, align_bp_bytes(P.psi_rows));
    std::printf("flags %d %d %d %d %d %d\n", align_flags_ok(0), align_flags_ok(1), align_flags_ok(2), align_flags_ok(3),
                align_flags_ok(4), align_flags_ok(-1));
    const long long n_pos = (long long)longest + 3;
    std::printf("lengths %d %d %d %d %d\n", align_lengths_check(total, total, n_pos, n_pos),
                align_lengths_check(total + 1, total, n_pos, n_pos), align_lengths_check(total, total, n_pos - 1, n_pos),
                align_lengths_check(total - 1, total, n_pos + 1, n_pos), align_lengths_check(0, total, 0, n_pos));
    return 0;
}
