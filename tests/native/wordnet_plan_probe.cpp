// Host probe of the word-loop decoder's plan (hmm_training_amd/csrc/wordnet_plan.hpp and plan_viterbi_group of
// viterbi_plan.hpp), built by tests/test_wordnet.py with the host compiler and the address / undefined-behaviour
// sanitizers:
//   wordnet_plan_probe W N K U len_0 len_1 ...
// lays the sequences out as hmmbw_set_observations does (obs_plan.hpp, plan_layout) and prints the plan:
//   fig GW spw nslots nvw total psi_rows | slot_len .. | slot_out .. | psi_off .. | same (1: plan_viterbi(N) equals
//   plan_viterbi_group(viterbi_gv(N))) | tab pi init A G B total np in_len | place in_lds bytes row_bytes
//   | lr (of a left-to-right, a dense and a skipping bank of W x N) | ok (of good, negative, NaN, infinite weights)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "../../hmm_training_amd/csrc/obs_plan.hpp"
#include "../../hmm_training_amd/csrc/wordnet_plan.hpp"

using namespace hmmbw;

static_assert(wordnet_gw(1) == 8 && wordnet_gw(8) == 8 && wordnet_gw(9) == 16 && wordnet_gw(16) == 16, "GW");
static_assert(wordnet_gw(17) == 32 && wordnet_gw(32) == 32 && wordnet_gw(33) == 64 && wordnet_gw(64) == 64, "GW");
static_assert(wordnet_np(1) == 1 && wordnet_np(2) == 2 && wordnet_np(3) == 4 && wordnet_np(5) == 8 && wordnet_np(8) == 8, "NP");
static_assert(wordnet_emis_bytes(256, 64, 8) == (size_t(1) << 20) && !wordnet_emis_in_lds(256, 64, 8), "the 1 MB table");
static_assert(wordnet_emis_in_lds(32, 16, 5) && wordnet_emis_in_lds(16, 64, 8) && !wordnet_emis_in_lds(17, 64, 8), "LDS");
static_assert(wordnet_tab(8, 3, 4).B % 2 == 0 && wordnet_tab(16, 5, 7).B % 2 == 0, "16-B aligned emission rows");
static_assert(kWnRowBytes == 320, "4 + 1 bytes per lane");

template <class T>
static void row(const char *tag, const std::vector<T> &v) {
    std::printf("%s", tag);
    for (const T &x : v) std::printf(" %lld", (long long)x);
    std::printf("\n");
}

int main(int argc, char **argv) {
    if (argc < 5) return 2;
    const int W = std::atoi(argv[1]), N = std::atoi(argv[2]), K = std::atoi(argv[3]), U = std::atoi(argv[4]);
    std::vector<int> len;
    for (int i = 5; i < argc; ++i) len.push_back(std::atoi(argv[i]));
    const ObsLayout L = plan_layout(len, U, false, 0);
    const int GW = wordnet_gw(W);
    const ViterbiPlan P = plan_viterbi_group(L.slot_len, L.slot_seq, L.R, GW);
    std::printf("fig %d %d %lld %lld %lld %lld\n", P.GV, P.spw, P.nslots, P.nvw, P.total, P.psi_rows);
    row("slot_len", L.slot_len);
    row("slot_out", P.slot_out);
    row("psi_off", P.psi_off);
    const ViterbiPlan Q = plan_viterbi(L.slot_len, L.slot_seq, L.R, N), Q2 = plan_viterbi_group(L.slot_len, L.slot_seq, L.R, viterbi_gv(N));
    std::printf("same %d\n", Q.GV == Q2.GV && Q.spw == Q2.spw && Q.nvw == Q2.nvw && Q.total == Q2.total &&
                                 Q.psi_rows == Q2.psi_rows && Q.slot_out == Q2.slot_out && Q.psi_off == Q2.psi_off && Q.slot_out == P.slot_out);
    const WordnetTab t = wordnet_tab(GW, N, K);
    std::printf("tab %lld %lld %lld %lld %lld %lld %d %lld\n", t.pi, t.init, t.A, t.G, t.B, t.total, wordnet_np(N),
                wordnet_in_len(W, N, K));
    std::printf("place %d %zu %d\n", wordnet_emis_in_lds(K, GW, N) ? 1 : 0, wordnet_emis_bytes(K, GW, N), kWnRowBytes);
    // banks: left-to-right, dense, and one with a skip arc in the last word only
    std::vector<double> A((size_t)W * N * N, 0.0);
    for (int w = 0; w < W; ++w)
        for (int i = 0; i < N; ++i) {
            A[((size_t)w * N + i) * N + i] = 0.5;
            if (i + 1 < N) A[((size_t)w * N + i) * N + i + 1] = 0.5;
        }
    const int lr = wordnet_is_lr(A.data(), W, N) ? 1 : 0;
    std::vector<double> D((size_t)W * N * N, 0.25);
    const int dense = wordnet_is_lr(D.data(), W, N) ? 1 : 0;
    int skip = -1;
    if (N >= 3) {
        A[((size_t)(W - 1) * N + 0) * N + 2] = 0.1;
        skip = wordnet_is_lr(A.data(), W, N) ? 1 : 0;
    }
    std::printf("lr %d %d %d\n", lr, dense, skip);
    const double good[3] = {0.0, 2.5, 1e300}, neg[3] = {0.1, -1e-300, 0.2}, nan[2] = {0.5, std::nan("")},
                 inf[2] = {std::numeric_limits<double>::infinity(), 0.5};
    std::printf("ok %d %d %d %d %d\n", wordnet_weights_ok(good, 3) ? 1 : 0, wordnet_weights_ok(neg, 3) ? 1 : 0,
                wordnet_weights_ok(nan, 2) ? 1 : 0, wordnet_weights_ok(inf, 2) ? 1 : 0, wordnet_weights_ok(good, 0) ? 1 : 0);
    return 0;
}
