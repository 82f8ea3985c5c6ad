// preproc_plan_probe.cpp — prints what hmm_training_amd/csrc/preproc_plan.hpp plans, for tests/test_preprocess.py.
// Built by a host compiler with the address and undefined-behaviour sanitizers: the header has no HIP dependency.
//   frames n win hop          -> "nf last_len ok"
//   window m wlen whop        -> "q partial cover"
//   validate n_rec kind coeff win hop f0 f1 f2 f3 have_pointers -> code
//   offsets win hop o0 o1 ... -> code
//   wvalidate n_rec wlen whop have_pointers -> code
//   shapes n_rec              -> "block chunks"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../hmm_training_amd/csrc/preproc_plan.hpp"

using namespace hmmbw;

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const char *cmd = argv[1];
    auto I = [&](int i) { return std::atoll(argv[i]); };
    auto D = [&](int i) { return std::strtod(argv[i], nullptr); };
    if (!std::strcmp(cmd, "frames") && argc == 5) {
        const long long n = I(2);
        const int win = (int)I(3), hop = (int)I(4);
        const long long nf = pre_frame_count(n, win, hop);
        std::printf("%lld %lld %d\n", nf, nf >= 1 ? pre_last_frame_len(n, win, hop) : -1LL, (int)pre_rec_ok(n, win, hop));
        return 0;
    }
    if (!std::strcmp(cmd, "window") && argc == 5) {
        const long long m = I(2);
        const int wlen = (int)I(3), whop = (int)I(4);
        std::printf("%lld %lld %d\n", pre_window_frames(m, wlen, whop), pre_window_partial(m, wlen, whop),
                    pre_window_cover(wlen, whop));
        return 0;
    }
    if (!std::strcmp(cmd, "validate") && argc == 12) {
        const double f[4] = {D(7), D(8), D(9), D(10)};
        std::printf("%d\n", pre_validate(I(2), (int)I(3), D(4), (int)I(5), (int)I(6), f, I(11) != 0));
        return 0;
    }
    if (!std::strcmp(cmd, "offsets") && argc >= 5) {
        std::vector<long long> off;
        for (int i = 4; i < argc; ++i) off.push_back(I(i));
        std::printf("%d\n", pre_validate_offsets(off.data(), (long long)off.size() - 1, (int)I(2), (int)I(3)));
        return 0;
    }
    if (!std::strcmp(cmd, "wvalidate") && argc == 6) {
        std::printf("%d\n", pre_window_validate(I(2), (int)I(3), (int)I(4), I(5) != 0));
        return 0;
    }
    if (!std::strcmp(cmd, "shapes") && argc == 3) {
        std::printf("%d %d\n", pre_block(I(2)), pre_window_chunks(I(2)));
        return 0;
    }
    return 2;
}
