// Host probe of the observation layout and the launch map (hmm_training_amd/csrc/obs_plan.hpp), built by
// tests/test_obs_plan.py with the host compiler.
//   obs_plan_probe map nwaves steps ncu wide det lds_tables split_tables topo_req topo
//                      split_extra join join_dense lds_layout xact
//     prints the map and its predicates, then, for the separate launch (J = 0: grid nblocks, 4 waves) and, where the
//     extra workgroups fit the full ones, the joined launch (J = 1: grid nfull, 8 waves), what wave_role gives every
//     (workgroup, wave): "role" with EArgs::split_extra = split_extra_on(), "orole" with the value the planner set
//     before the rule moved into split_extra_on (the switch, zeroed for a left-to-right launch off the joined map).
//   obs_plan_probe layout file U wide NP G
//     file: R, then per sequence its length and its symbols.  Prints the layout, the packs (row scale 16 G), the
//     class-split packs made from them, and the gather index of both builders.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../hmm_training_amd/csrc/obs_plan.hpp"

using namespace hmmbw;

static_assert(pack_pos(100, 8, 0, 0) == 100 && pack_pos(100, 8, 3, 7) == 100 + 3 * 8 + 7, "chunk 0: [u][8]");
static_assert(pack_pos(0, 8, 0, 8) == 64 && pack_pos(0, 4, 1, 17) == (2 * 4 + 1) * 8 + 1, "chunk-major");

template <bool J>
static void roles(const char *tag, const LaunchMap &m, bool allowed) {
    const long long grid = J ? m.nfull : m.nblocks;
    for (long long b = 0; b < grid; ++b)
        for (int wv = 0; wv < (J ? 2 : 1) * kWpb; ++wv) {
            const WaveRole r = wave_role<J>(b, wv, kWpb, m.nfull, m.xact, allowed);
            std::printf("%s %d %lld %d %lld %d %d %d %d %d\n", tag, J ? 1 : 0, b, wv, r.wave, r.slot, r.xblk ? 1 : 0,
                        r.split ? 1 : 0, r.brole ? 1 : 0, r.active ? 1 : 0);
        }
}

static int probe_map(char **v) {
    MapInputs in;
    in.nwaves = std::atoll(v[0]);
    in.steps = std::atoll(v[1]);
    in.ncu = std::atoi(v[2]);
    in.wide = std::atoi(v[3]) != 0;
    in.det = std::atoi(v[4]) != 0;
    in.lds_tables = std::atoi(v[5]) != 0;
    in.split_tables = std::atoi(v[6]) != 0;
    in.topo_req = std::atoi(v[7]);
    const int topo = std::atoi(v[8]);
    in.sw.split_extra = std::atoi(v[9]);
    in.sw.join = std::atoi(v[10]);
    in.sw.join_dense = std::atoi(v[11]);
    in.sw.lds_layout = std::atoi(v[12]);
    in.sw.xact = std::atoi(v[13]);
    const LaunchMap m = plan_map(in);
    const bool jn = joined(m, topo);
    std::printf("nblocks %lld nfull %lld xact %d fits_cus %d sym2 %d joined %d split_extra %d split_tables %d\n", m.nblocks,
                m.nfull, m.xact, m.fits_cus ? 1 : 0, m.sym2 ? 1 : 0, jn ? 1 : 0, split_extra_on(m, topo, jn) ? 1 : 0,
                split_tables_on(m, topo, m.sym2) ? 1 : 0);
    if (in.wide) return 0;
    const bool lr = topo == HMMBW_TOPOLOGY_LEFT_TO_RIGHT;
    // SPLITOK of the E-step kernel of each launch (estep_small_body)
    const bool ok0 = !lr && m.lds_atomic, ok1 = m.lds_atomic;
    roles<false>("role", m, ok0 && split_extra_on(m, topo, false));
    roles<false>("orole", m, ok0 && in.sw.split_extra && !lr);
    if (m.nblocks - m.nfull <= m.nfull) {
        roles<true>("role", m, ok1 && split_extra_on(m, topo, true));
        roles<true>("orole", m, ok1 && in.sw.split_extra);
    }
    return 0;
}

template <class T>
static void line(const char *tag, const std::vector<T> &v) {
    std::printf("%s", tag);
    for (const T &x : v) std::printf(" %lld", (long long)x);
    std::printf("\n");
}

static int probe_layout(char **v) {
    std::FILE *f = std::fopen(v[0], "r");
    if (!f) return 2;
    const int U = std::atoi(v[1]), NP = std::atoi(v[3]), G = std::atoi(v[4]);
    const bool wide = std::atoi(v[2]) != 0;
    long long R = 0;
    if (std::fscanf(f, "%lld", &R) != 1) return 2;
    std::vector<int> len((size_t)R);
    std::vector<int64_t> off(1, 0);
    std::vector<int32_t> sym;
    int K = 1;
    for (long long r = 0; r < R; ++r) {
        if (std::fscanf(f, "%d", &len[(size_t)r]) != 1) return 2;
        for (int t = 0; t < len[(size_t)r]; ++t) {
            int s = 0;
            if (std::fscanf(f, "%d", &s) != 1) return 2;
            sym.push_back(s);
            K = std::max(K, s + 1);
        }
        off.push_back((int64_t)sym.size());
    }
    std::fclose(f);
    const ObsLayout L = plan_layout(len, U, wide, NP);
    std::printf("tot %lld %lld %lld %lld\n", L.nwaves, L.symtot, L.cktot, L.sptot);
    line("slot_len", L.slot_len);
    line("slot_seq", L.slot_seq);
    line("wave_T", L.wave_T);
    line("wave_full", L.wave_full);
    line("symoff", L.symoff);
    line("ckoff", L.ckoff);
    line("spoff", L.spoff);
    const long long row_bytes = 16LL * G;
    std::vector<uint16_t> pack = fill_packs(L, off.data(), sym.data(), row_bytes);
    line("pack", pack);
    to_split_packs(pack, row_bytes, G);
    line("pack2", pack);
    const long long total = off[(size_t)R];
    std::vector<long long> bptr;
    std::vector<unsigned> rows((size_t)std::max(total, 1LL));
    build_gather_index(L, off.data(), sym.data(), K, false,
                       [&](long long w, int u, int t) { return pack_pos(L.symoff[(size_t)w], U, u, t); }, bptr, rows);
    line("bptr", bptr);
    line("rows", rows);
    // by position: the wide path's tile rows, the pack positions otherwise; the padding's rank is `total`
    std::vector<unsigned> prow((size_t)std::max(wide ? L.cktot / NP : L.symtot, 1LL), (unsigned)total);
    build_gather_index(L, off.data(), sym.data(), K, true, [&](long long w, int u, int t) {
        return wide ? L.ckoff[(size_t)w] / NP + (long long)t * U + u : pack_pos(L.symoff[(size_t)w], U, u, t);
    }, bptr, prow);
    line("prow", prow);
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 16 && !std::strcmp(argv[1], "map")) return probe_map(argv + 2);
    if (argc == 7 && !std::strcmp(argv[1], "layout")) return probe_layout(argv + 2);
    std::fprintf(stderr, "usage: obs_plan_probe map ... | layout ... (see the source's header)\n");
    return 1;
}
