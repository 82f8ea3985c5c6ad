// lbg_plan_probe — prints what hmm_training_amd/csrc/lbg_plan.hpp decides, for tests/test_lbg.py (built with the host
// compiler and the address / undefined-behaviour sanitizers; no HIP).
//   offsets K                          G, each generation's first row and row count, the rows of the output
//   validate F stride first dims K eps max_it have_frames have_centroids      the status
//   lds K stride dims                  staged?, accumulator doubles, LDS bytes, the budget
//   passes G max_it                    the bound on the passes of a call
//   run eps max_it G d0 d1 ...         the state machine over the distortions d0 (c0's pass), d1, ...: one line per pass
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../hmm_training_amd/csrc/lbg_plan.hpp"

using namespace hmmbw;

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const char *cmd = argv[1];
    auto I = [&](int i) { return i < argc ? std::atoll(argv[i]) : 0LL; };
    auto D = [&](int i) { return i < argc ? std::strtod(argv[i], nullptr) : 0.0; };
    if (!std::strcmp(cmd, "offsets")) {
        const int K = (int)I(2), G = lbg_generations(K);
        std::printf("G %d\n", G);
        for (int g = 0; g <= G; ++g) std::printf("gen %d %lld %lld\n", g, lbg_gen_offset(g), lbg_gen_rows(g));
        std::printf("total %lld\n", lbg_total_rows(K));
        return 0;
    }
    if (!std::strcmp(cmd, "validate")) {
        std::printf("%d\n", lbg_validate(I(2), (int)I(3), (int)I(4), (int)I(5), (int)I(6), D(7), I(8), I(9) != 0, I(10) != 0));
        return 0;
    }
    if (!std::strcmp(cmd, "lds")) {
        const int K = (int)I(2), stride = (int)I(3), dims = (int)I(4);
        std::printf("%d %lld %zu %zu\n", (int)lbg_scan_staged(dims), lbg_acc_doubles(K, stride), lbg_lds_bytes(K, stride, dims),
                    kLbgLdsBudget);
        return 0;
    }
    if (!std::strcmp(cmd, "passes")) {
        std::printf("%lld\n", lbg_max_passes((int)I(2), I(3)));
        return 0;
    }
    if (!std::strcmp(cmd, "run")) {
        const double eps = D(2);
        const long long max_it = I(3);
        const int G = (int)I(4);
        LbgState s = lbg_initial_state();
        for (int i = 5; i < argc && !s.done; ++i) {
            const LbgStep r = lbg_advance(s, D(i), eps, max_it, G);
            std::printf("%d %d %d %d %lld %.17g | %d %d %d %lld %lld %.17g\n", (int)r.record, (int)r.stop, (int)r.split,
                        r.generation, r.iteration, r.diff, s.generation, s.K_now, s.done, s.iteration, s.n_records, s.prev);
        }
        return 0;
    }
    return 2;
}
