// Host probe of the class-split LDS table layout (hmm_training_amd/csrc/lds_layout.hpp), built by
// tests/test_lds_layout.py with the host compiler:  lds_layout_probe GP K
// Prints the layout's constants, then one line per (class, symbol, state column): the byte offsets of the
// P entry and of its H entry.
#include <cstdio>
#include <cstdlib>

#include "../../hmm_training_amd/csrc/lds_layout.hpp"

using namespace hmmbw;

static_assert(lay2_p_off(8, 0, 0, 0) == 0 && lay2_row_bytes(8) == 256 && lay2_hist_off(8) == 128, "G = 8 rows");
static_assert(lay2_table_bytes(256, 8) == 131200 && lay2_tables_fit(256, 8) && !lay2_tables_fit(257, 8), "K = 256");

int main(int argc, char **argv) {
    const int GP = argc > 1 ? std::atoi(argv[1]) : 8, K = argc > 2 ? std::atoi(argv[2]) : 256;
    std::printf("row_bytes %d hist_off %d class_off %d table_bytes %zu fit %d\n", lay2_row_bytes(GP), lay2_hist_off(GP),
                lay2_class_off(GP), lay2_table_bytes(K, GP), lay2_tables_fit(K, GP) ? 1 : 0);
    std::printf("classes");
    for (int u = 0; u < 64 / GP; ++u) std::printf(" %d", lay2_class(u));
    std::printf("\n");
    for (int c = 0; c < 2; ++c)
        for (int o = 0; o < K; ++o)
            for (int j = 0; j < GP; ++j) {
                const size_t p = lay2_p_off(GP, c, o, j);
                std::printf("%d %d %d %zu %zu\n", c, o, j, p, p + lay2_hist_off(GP));
            }
    return 0;
}
