// Host probe of the Viterbi decoder's plan (hmm_training_amd/csrc/viterbi_plan.hpp), built by
// tests/test_viterbi.py with the host compiler and the address / undefined-behaviour sanitizers:
//   viterbi_plan_probe N U len_0 len_1 ...
// lays the sequences out as hmmbw_set_observations does (obs_plan.hpp, plan_layout) and prints the plan:
//   fig GV spw nslots nvw total psi_rows | slot_len .. | slot_seq .. | slot_out .. | psi_off ..
// then the table placement (place: K GV in_lds, ...), the pack divisor (div: lds_tables G div shift, ...)
// and the shift of a few divisors.
#include <cstdio>
#include <cstdlib>

#include "../../hmm_training_amd/csrc/obs_plan.hpp"
#include "../../hmm_training_amd/csrc/viterbi_plan.hpp"

using namespace hmmbw;

static_assert(viterbi_gv(1) == 8 && viterbi_gv(8) == 8 && viterbi_gv(9) == 16 && viterbi_gv(16) == 16, "GV");
static_assert(viterbi_gv(17) == 32 && viterbi_gv(32) == 32 && viterbi_gv(33) == 64 && viterbi_gv(64) == 64, "GV");
static_assert(viterbi_table_in_lds(1024, 8) && !viterbi_table_in_lds(1025, 8) && !viterbi_table_in_lds(1024, 64), "LDS");
static_assert(viterbi_pack_div(true, 8, 0) == 128 && viterbi_pack_div(false, 8, 0) == 1, "divisor");
static_assert(viterbi_pack_shift(128) == 7 && viterbi_pack_shift(1) == 0 && viterbi_pack_shift(144) == -1, "shift");

template <class T>
static void row(const char *tag, const std::vector<T> &v) {
    std::printf("%s", tag);
    for (const T &x : v) std::printf(" %lld", (long long)x);
    std::printf("\n");
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    const int N = std::atoi(argv[1]), U = std::atoi(argv[2]);
    std::vector<int> len;
    for (int i = 3; i < argc; ++i) len.push_back(std::atoi(argv[i]));
    const ObsLayout L = plan_layout(len, U, N > 16, N > 16 ? 16 * ((N + 15) / 16) : 0);
    const ViterbiPlan P = plan_viterbi(L.slot_len, L.slot_seq, L.R, N);
    std::printf("fig %d %d %lld %lld %lld %lld\n", P.GV, P.spw, P.nslots, P.nvw, P.total, P.psi_rows);
    row("slot_len", L.slot_len);
    row("slot_seq", L.slot_seq);
    row("slot_out", P.slot_out);
    row("psi_off", P.psi_off);
    std::printf("place");
    for (int K : {4, 128, 256, 1024})
        for (int GV : {8, 16, 32, 64}) std::printf(" %d %d %d", K, GV, viterbi_table_in_lds(K, GV) ? 1 : 0);
    std::printf("\ndiv");
    for (int lds = 0; lds < 2; ++lds)
        for (int G : {2, 4, 8, 16}) {
            const long long d = viterbi_pack_div(lds != 0, G, 0);
            std::printf(" %d %d %lld %d", lds, G, d, viterbi_pack_shift(d));
        }
    std::printf("\nshift");
    for (long long d : {0LL, 1LL, 48LL, 16LL, -8LL}) std::printf(" %d", viterbi_pack_shift(d));
    std::printf("\n");
    return 0;
}
