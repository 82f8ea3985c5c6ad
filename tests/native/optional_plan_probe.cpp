// Host probe of the plan of the optional transcript positions (hmm_training_amd/csrc/embed_plan.hpp:
// embed_optional_check and the statistics that follow EmbedStats; align_plan.hpp: the entry-source masks), built by
// tests/test_optional.py with the host compiler and the address / undefined-behaviour sanitizers:
//   optional_plan_probe W N K rows  len_0 len_1 ... -- id_0 id_1 ... -- flag_0 flag_1 ...     (flags may be absent)
// prints
//   check code | mand m_0 .. m_{W-1} | count c_0 .. | stats present touched total base | skip row_bytes bytes bp_bytes
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../hmm_training_amd/csrc/align_plan.hpp"

using namespace hmmbw;

static_assert(embed_present_off(3, 2, 4) == embed_stats(3, 2, 4).total, "present follows the statistics as they were");
static_assert(embed_touched_off(3, 2, 4) == embed_stats(3, 2, 4).total + 3, "touched follows present");
static_assert(embed_stats_optional_total(64, 8, 256) == embed_stats(64, 8, 256).total + 128, "two doubles per word");
static_assert(kAlSkipRowBytes == 8 && kAlRowBytes == 256, "a lane mask per row beside the nibble words");
static_assert(align_skip_bytes(0) == 0 && align_skip_bytes(10) == 80, "the masks");
static_assert(align_skip_bytes((1LL << 29) + 1) == ((size_t(1) << 29) + 1) * 8, "rows past 2^31 bytes");
static_assert(align_bp_bytes(10) == 2560, "the back-pointer rows keep their size");

int main(int argc, char **argv) {
    if (argc < 5) return 2;
    const int W = std::atoi(argv[1]), N = std::atoi(argv[2]), K = std::atoi(argv[3]);
    const long long rows = std::atoll(argv[4]);
    std::vector<int64_t> off{0};
    std::vector<int32_t> ids;
    std::vector<uint8_t> flags;
    int part = 0;
    for (int i = 5; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--")) {
            ++part;
            continue;
        }
        const long long v = std::atoll(argv[i]);
        if (part == 0) off.push_back(off.back() + v);
        else if (part == 1) ids.push_back((int32_t)v);
        else flags.push_back((uint8_t)v);
    }
    if ((long long)ids.size() != off.back() || (part == 2 && flags.size() != ids.size())) return 2;
    const long long R = (long long)off.size() - 1;
    std::vector<long long> mand((size_t)W, -1), count((size_t)W, -1);
    long long longest = 0;
    if (embed_transcripts_check(off.data(), ids.data(), R, W, &longest, count.data()) != 0) return 3;
    const int code = embed_optional_check(off.data(), ids.data(), part == 2 ? flags.data() : nullptr, R, W, mand.data());
    std::printf("check %d\n", code);
    std::printf("mand");
    for (long long m : mand) std::printf(" %lld", m);
    std::printf("\ncount");
    for (long long m : count) std::printf(" %lld", m);
    std::printf("\nstats %lld %lld %lld %lld\n", embed_present_off(W, N, K), embed_touched_off(W, N, K),
                embed_stats_optional_total(W, N, K), embed_stats(W, N, K).total);
    std::printf("skip %d %zu %zu\n", kAlSkipRowBytes, align_skip_bytes(rows), align_bp_bytes(rows));
    // without a count to fill
    if (embed_optional_check(off.data(), ids.data(), part == 2 ? flags.data() : nullptr, R, W, nullptr) != code) return 4;
    return 0;
}
