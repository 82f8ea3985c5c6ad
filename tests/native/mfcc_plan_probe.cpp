// mfcc_plan_probe — prints what hmm_training_amd/csrc/mfcc_plan.hpp decides, for tests/test_mfcc.py (built with the
// host compiler and the address / undefined-behaviour sanitizers; no HIP).
//   frames n_samples frame_size hop_size      the count, then "start length" per frame
//   validate n_samples n_frames L n_mels n_mfcc amin out_stride have_pointers      the status
//   inrange start L n_samples                 1 / 0
//   tvalidate L sample_rate n_mels n_mfcc have_pointers                            the status of the table call
//   sizes L n_mels                            H Hp Kp Hs Ps blocks, the LDS offsets, the LDS bytes, the budget
//   mfmas L waves                             matrix instructions per tile
//   tables L sample_rate n_mels n_mfcc        every table value as the hex of its bits: "window", "twiddle", "mel m"
//                                             rows, "band m first count" rows and "dct i" rows
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../hmm_training_amd/csrc/mfcc_plan.hpp"

using namespace hmmbw;

static void row(const char *name, int idx, const double *v, int n) {
    if (idx >= 0)
        std::printf("%s %d", name, idx);
    else
        std::printf("%s", name);
    for (int i = 0; i < n; ++i) {
        uint64_t b;
        std::memcpy(&b, v + i, 8);
        std::printf(" %016llx", (unsigned long long)b);
    }
    std::printf("\n");
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const char *cmd = argv[1];
    auto I = [&](int i) { return i < argc ? std::atoll(argv[i]) : 0LL; };
    auto D = [&](int i) { return i < argc ? std::strtod(argv[i], nullptr) : 0.0; };
    if (!std::strcmp(cmd, "frames")) {
        const long long n = I(2);
        const int fs = (int)I(3), hop = (int)I(4);
        const long long cnt = fs >= 1 && hop >= 1 && n >= 0 ? mfcc_frame_count(n, fs, hop) : 0;
        std::vector<long long> s((size_t)cnt + 1), l((size_t)cnt + 1);
        const long long got = mfcc_frame_table(n, fs, hop, s.data(), l.data());
        std::printf("%lld %lld\n", cnt, got);
        for (long long i = 0; i < got; ++i) std::printf("%lld %lld\n", s[(size_t)i], l[(size_t)i]);
        return 0;
    }
    if (!std::strcmp(cmd, "validate")) {
        std::printf("%d\n", mfcc_validate(I(2), I(3), (int)I(4), (int)I(5), (int)I(6), D(7), I(8), I(9) != 0));
        return 0;
    }
    if (!std::strcmp(cmd, "inrange")) {
        std::printf("%d\n", (int)mfcc_frame_in_range(I(2), (int)I(3), I(4)));
        return 0;
    }
    if (!std::strcmp(cmd, "tvalidate")) {
        std::printf("%d\n", mfcc_tables_validate((int)I(2), D(3), (int)I(4), (int)I(5), I(6) != 0));
        return 0;
    }
    if (!std::strcmp(cmd, "sizes")) {
        const int L = (int)I(2), n_mels = (int)I(3);
        const MfccLds l = mfcc_lds(L, n_mels);
        std::printf("%d %d %d %d %d %d\n", mfcc_half(L), mfcc_half_padded(L), mfcc_bins_padded(L), mfcc_fold_stride(L),
                    mfcc_power_stride(L), mfcc_bin_blocks(L));
        std::printf("%d %d %d %d %d %d %d %d\n", l.twiddle, l.even, l.odd, l.power, l.db, l.band, l.flag, l.total);
        std::printf("%zu %zu\n", mfcc_lds_bytes(L, n_mels), kMfccLdsBudget);
        return 0;
    }
    if (!std::strcmp(cmd, "mfmas")) {
        std::printf("%lld\n", mfcc_tile_mfmas((int)I(2), (int)I(3)));
        return 0;
    }
    if (!std::strcmp(cmd, "tables")) {
        const int L = (int)I(2), n_mels = (int)I(4), n_mfcc = (int)I(5), H = mfcc_half(L);
        const double sr = D(3);
        if (mfcc_tables_validate(L, sr, n_mels, n_mfcc, true) != kMfccOk) return 3;
        std::vector<double> w((size_t)L), tw((size_t)2 * L), mel((size_t)n_mels * H), dct((size_t)n_mfcc * n_mels);
        mfcc_tables(L, sr, n_mels, n_mfcc, w.data(), tw.data(), mel.data(), dct.data());
        row("window", -1, w.data(), L);
        row("twiddle", -1, tw.data(), 2 * L);
        for (int m = 0; m < n_mels; ++m) {
            row("mel", m, mel.data() + (size_t)m * H, H);
            int first, count;
            mfcc_band(mel.data() + (size_t)m * H, H, &first, &count);
            std::printf("band %d %d %d\n", m, first, count);
        }
        for (int i = 0; i < n_mfcc; ++i) row("dct", i, dct.data() + (size_t)i * n_mels, n_mels);
        return 0;
    }
    return 2;
}
