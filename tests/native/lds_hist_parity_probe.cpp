// Host probe of the histogram parity halves of the class-split LDS tables (hmm_training_amd/csrc/lds_layout.hpp),
// built by tests/test_lds_hist_parity.py with the host compiler:  lds_hist_parity_probe GP K
// Prints the constants, then one line per (sequence slot, symbol, state column): the byte offsets of the slot's
// P entry and of the 8-byte field its histogram add goes to; then one line per (symbol, state column) of the
// b table.
#include <cstdio>
#include <cstdlib>

#include "../../hmm_training_amd/csrc/lds_layout.hpp"

using namespace hmmbw;

static_assert(lay2_add_off(8, 0) == 128 && lay2_add_off(8, 1) == 136 && lay2_add_off(8, 6) == 128, "halves by slot parity");
static_assert(lay2_b_off(256, 8, 0, 0) == lay2_table_bytes(256, 8) && lay2_b_bytes(256, 8) == 16384, "b table");
static_assert(lay2_total_bytes(256, 8) + kLay2OtherBytes <= kCuLdsBytes, "K = 256 fits a CU's LDS");

int main(int argc, char **argv) {
    const int GP = argc > 1 ? std::atoi(argv[1]) : 8, K = argc > 2 ? std::atoi(argv[2]) : 256;
    int kfirst = 1;  // the first K the layout refuses
    while (lay2_lds_fit(kfirst, GP)) ++kfirst;
    std::printf("table_bytes %zu b_bytes %zu total_bytes %zu other_bytes %zu cu_bytes %zu fit %d first_unfit_K %d "
                "b_pack_shift %d\n",
                lay2_table_bytes(K, GP), lay2_b_bytes(K, GP), lay2_total_bytes(K, GP), kLay2OtherBytes, kCuLdsBytes,
                lay2_lds_fit(K, GP) ? 1 : 0, kfirst, kLay2BPackShift);
    for (int u = 0; u < 64 / GP; ++u)
        for (int o = 0; o < K; ++o)
            for (int j = 0; j < GP; ++j) {
                const size_t p = lay2_p_off(GP, lay2_class(u), o, j);
                std::printf("a %d %d %d %zu %zu\n", u, o, j, p, p + lay2_add_off(GP, u));
            }
    for (int o = 0; o < K; ++o)
        for (int j = 0; j < GP; ++j) std::printf("b %d %d %zu\n", o, j, lay2_b_off(K, GP, o, j));
    return 0;
}
