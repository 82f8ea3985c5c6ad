// obs_plan.hpp — the observation layout and the wave -> workgroup launch map of the small kernels: what
// hmmbw_set_observations lays out and plans (hmmbw.hip), the predicates the planner and the info keys read off the
// map, and wave_role, the statement of the kernel's side of the same map (estep_small_body, hmmbw_device.hpp).
// Plain C++17 with no HIP dependency, so that a host compiler can build a probe of it
// (tests/native/obs_plan_probe.cpp).
#pragma once

#include <algorithm>
#include <cstdint>
#include <numeric>
#include <vector>

#include "lds_layout.hpp"

#include "../../include/hmmbw.h"

namespace hmmbw {

constexpr int kWave = 64;
constexpr int kChunk = 8;  // time steps per packed symbol load (8 x uint16 = 16 B)
constexpr int kBlock = 256;  // threads per E-step workgroup (4 waves)
constexpr int kWpb = kBlock / kWave;  // waves of a full (sequence-group) workgroup

// ---------------------------------------------------------------------------------------------
// Observation layout (hmmbw_args.hpp, struct Layout)
// ---------------------------------------------------------------------------------------------

// index in a wave's symbol pack ([chunk][u][8] uint16 from symoff) of step t of the wave's sequence slot u
HMMBW_HD constexpr long long pack_pos(long long symoff, int U, int u, int t) {
    return symoff + ((long long)(t / kChunk) * U + u) * kChunk + t % kChunk;
}

struct ObsLayout {
    long long R = 0, nwaves = 0;
    int U = 1;
    // slot = wave * U + u -> caller sequence slot_seq[slot] (-1: padding) of length slot_len[slot] (0: padding);
    // slot_seq[0, R) is the length-descending stable permutation of the sequences
    std::vector<int> slot_len, slot_seq;
    std::vector<int> wave_T, wave_full;  // longest slot of the wave | 1: every real slot has that length
    std::vector<long long> symoff, ckoff, spoff;  // running sums of the waves' chunk-rounded sizes
    long long symtot = 0, cktot = 0, sptot = 0;
};

// length-sorted (descending, stable) assignment of sequences to wave slots: the sequences that
// share a wave have near-equal lengths, so the lockstep time loop wastes little
inline ObsLayout plan_layout(const std::vector<int> &len, int U, bool wide, int NP) {
    ObsLayout L;
    const long long R = L.R = (long long)len.size();
    L.U = U;
    std::vector<int64_t> perm((size_t)R);
    std::iota(perm.begin(), perm.end(), 0);
    std::stable_sort(perm.begin(), perm.end(), [&](int64_t x, int64_t y) { return len[(size_t)x] > len[(size_t)y]; });
    const long long nwaves = L.nwaves = (R + U - 1) / U;
    L.symoff.resize((size_t)nwaves), L.ckoff.resize((size_t)nwaves), L.spoff.resize((size_t)nwaves);
    L.wave_T.resize((size_t)nwaves), L.wave_full.resize((size_t)nwaves);
    L.slot_len.assign((size_t)(nwaves * U), 0), L.slot_seq.assign((size_t)(nwaves * U), -1);
    for (long long w = 0; w < nwaves; ++w) {
        int Tw = 0, Tmin = 1 << 30;
        for (int u = 0; u < U; ++u) {
            const long long s = w * U + u;
            if (s < R) {
                L.slot_len[(size_t)s] = len[(size_t)perm[(size_t)s]];
                L.slot_seq[(size_t)s] = (int)perm[(size_t)s];
                Tw = std::max(Tw, L.slot_len[(size_t)s]);
                Tmin = std::min(Tmin, L.slot_len[(size_t)s]);
            }
        }
        const long long nch = (Tw + kChunk - 1) / kChunk;
        L.wave_T[(size_t)w] = Tw;
        L.wave_full[(size_t)w] = (Tmin == Tw) ? 1 : 0;
        L.symoff[(size_t)w] = L.symtot;
        L.ckoff[(size_t)w] = L.cktot;
        L.spoff[(size_t)w] = L.sptot;
        L.symtot += nch * U * kChunk;
        if (wide) {  // full alpha_hat [t][NP/16 waves][4][64 lanes] + exponents [t][16]
            L.cktot += nch * kChunk * (long long)NP * 16;
            L.sptot += nch * kChunk * 16;
        } else {     // one checkpoint per chunk [c][64] + exponent packs [c][u]
            L.cktot += nch * kWave;
            L.sptot += nch * U;
        }
    }
    return L;
}

// f(w, u, r, t) for every step t of every real slot (wave w, slot u, caller sequence r), in slot order
template <class F>
inline void for_each_step(const ObsLayout &L, F f) {
    for (long long w = 0; w < L.nwaves; ++w)
        for (int u = 0; u < L.U; ++u) {
            const long long s = w * L.U + u;
            if (s >= L.R) continue;
            const int r = L.slot_seq[(size_t)s];
            for (int t = 0; t < L.slot_len[(size_t)s]; ++t) f(w, u, r, t);
        }
}

// The symbol packs: symbol * scale at pack_pos of every step, 0 in the padding (scale: the byte stride of the LDS
// emission rows when the tables live in LDS, < 64 KiB so they fit uint16; 1: symbol ids)
inline std::vector<uint16_t> fill_packs(const ObsLayout &L, const int64_t *offsets, const int32_t *symbols,
                                        long long scale) {
    static_assert(pack_pos(0, 8, 3, 2 * kChunk + 5) == pack_pos(0, 8, 3, 2 * kChunk) + 5, "a chunk's steps are contiguous");
    std::vector<uint16_t> pack((size_t)std::max(L.symtot, 1LL), 0);
    const int U = L.U;
    for (long long s = 0; s < L.R; ++s) {  // chunk by chunk: the 8 steps from pack_pos of the chunk's first
        const int32_t *src = symbols + offsets[L.slot_seq[(size_t)s]];
        const long long symoff = L.symoff[(size_t)(s / U)];
        const int u = (int)(s % U), T = L.slot_len[(size_t)s];
        for (int t0 = 0; t0 < T; t0 += kChunk) {
            uint16_t *dst = pack.data() + pack_pos(symoff, U, u, t0);
            for (int k = 0; k < std::min(kChunk, T - t0); ++k) dst[k] = (uint16_t)(src[t0 + k] * scale);
        }
    }
    return pack;
}

// the packs of the class-split tables from those of the row tables: the class-split rows are twice as long,
// o * row_bytes -> o * lay2_row_bytes (<= 65,280)
inline void to_split_packs(std::vector<uint16_t> &pack, long long row_bytes, int G) {
    static_assert(lay2_row_bytes(8) == 2 * 8 * 16, "class-split row stride");
    for (uint16_t &e : pack) e = (uint16_t)(e / row_bytes * lay2_row_bytes(G));
}

// Symbol -> gamma rows index of k_bnum_gather: bptr[k], bptr[k + 1] bound symbol k's ranks (its steps in slot
// order, stable), pos(w, u, t) is the gamma row the E-step writes for a step.  by_pos = false: rows[rank] = pos
// (rows must hold the step count); by_pos = true: rows[pos] = rank (the wide E-step scatters each row to its
// rank; rows is pre-filled with the rank of the padding positions).
template <class Pos>
inline void build_gather_index(const ObsLayout &L, const int64_t *offsets, const int32_t *symbols, int K, bool by_pos,
                               Pos pos, std::vector<long long> &bptr, std::vector<unsigned> &rows) {
    bptr.assign((size_t)K + 1, 0);
    for (int64_t i = 0; i < offsets[L.R]; ++i) ++bptr[(size_t)symbols[i] + 1];
    for (int k = 0; k < K; ++k) bptr[(size_t)k + 1] += bptr[(size_t)k];
    std::vector<long long> fill(bptr.begin(), bptr.end() - 1);
    for_each_step(L, [&](long long w, int u, int r, int t) {
        const long long rank = fill[(size_t)symbols[offsets[r] + t]]++, p = pos(w, u, t);
        rows[(size_t)(by_pos ? p : rank)] = (unsigned)(by_pos ? rank : p);
    });
}

// ---------------------------------------------------------------------------------------------
// Launch map
// ---------------------------------------------------------------------------------------------

// A/B switches of the map (environment, read by hmmbw_set_observations) and the table layout option
struct MapSwitches {
    int split_extra = 1;  // EArgs::split_extra (HMMBW_SPLIT_EXTRA=0 turns it off)
    int join = 1;         // left-to-right E-step on the joined spread map (k_estep_join; HMMBW_JOIN=0 off)
    int join_dense = 1;   // the dense E-step on it too (HMMBW_JOIN_DENSE=0 off)
    int lds_layout = -1;  // HMMBW_OPT_LDS_LAYOUT: the joined map on the class-split LDS tables (G = 8):
                          // -1 where they pay (LaunchMap::sym2), 0 never, 1 wherever they can run
    int xact = 0;         // HMMBW_XACT (diagnostics: 1..4, 4 = every workgroup full); 0: the planner's choice
};

struct MapInputs {
    long long nwaves = 0;
    long long steps = 0;  // the waves' steps, each wave's rounded up to whole chunks (symtot / U)
    int ncu = 0;
    bool wide = false, det = false;
    bool lds_tables = false;    // the context's lds_tables()
    bool split_tables = false;  // ... and split_tables()
    int topo_req = HMMBW_TOPOLOGY_AUTO;
    MapSwitches sw;
};

struct LaunchMap {
    long long nblocks = 0;
    long long nfull = 0;    // small kernels: workgroups with 4 active waves (then xact-wave ones)
    int xact = kWpb;
    bool fits_cus = false;  // the map's workgroups fit one per CU
    bool sym2 = false;      // a second pack set (the class-split tables') is wanted
    // what it was planned under, for the predicates below
    int ncu = 0;
    bool lds_atomic = false;  // small kernels with LDS tables and atomic statistics
    bool split_tables = false;
    MapSwitches sw;
};

// The joined launch runs on the class-split LDS tables (k_estep_join<.., 1>, lds_layout.hpp).  The context keeps a
// second pack set for it (d_sym2, row offsets of the 256-B rows): the scorer, the statistics pass off the joined
// map, the grouped and the deterministic kernels keep d_sym, the row tables (64 KiB, two workgroups per CU) and
// their code as it was.  HMMBW_OPT_LDS_LAYOUT / HMMBW_LDS_LAYOUT = 0 keeps the joined launch on the row tables too.
// The second class's tables are 64 KB more LDS stores in every launch's prologue, +0.4 to +0.55 us whatever the
// shape (T = 8 at 8,192 sequences 13.07 -> 13.64 us), against conflict-free emission reads in the sweeps, which
// pay where a CU's LDS array is the busy resource: on the spread map's CUs with extra groups, in long sweeps.
// Measured (profiles/r7/lds_layout_sweep.txt, us per iteration, row -> class-split tables): 10,000 sequences
// T = 96 20.35 -> 20.63, 128 22.61 -> 22.81, 144 24.13 -> 23.96, 160 25.58 -> 25.32, 200 28.6 -> 28.0; 12,500
// sequences T = 128 25.50 -> 25.32, 160 28.39 -> 27.90, 200 32.6 -> 31.7; without extra groups 8,192 x 200 27.05
// -> 27.39; dense cfg3 (ds_read_b64 emissions, other lane groups) 58.8 -> 59.3.  So by default (-1): left-to-right,
// extra groups, and a mean wave length of at least kSplitTablesMinSteps; 1 forces them wherever they can run.
constexpr long long kSplitTablesMinSteps = 144;

inline LaunchMap plan_map(const MapInputs &in) {
    LaunchMap m;
    m.sw = in.sw;
    m.ncu = in.ncu;
    m.lds_atomic = !in.wide && !in.det && in.lds_tables;
    m.split_tables = in.split_tables;
    const long long ncu = in.ncu;
    m.nblocks = in.wide ? in.nwaves : (in.nwaves + kWpb - 1) / kWpb;  // wide: one tile per block
    m.nfull = m.nblocks;
    // Small kernels, more waves than SIMDs: one full 4-wave workgroup per CU, then the remaining waves
    // in workgroups of xact = 2 active waves (one per CU while they fit), so the SIMDs that must run a
    // second wave are spread over twice as many CUs, which then share their LDS and memory pipes among
    // 6 waves instead of 8.  cfg3 (1,250 waves): 38.2 -> 36.5 us per iteration; xact = 1 (a prologue
    // and histogram flush per extra wave) and 3 measured no better.  HMMBW_XACT
    // overrides it (diagnostics: 1..4, 4 = every workgroup full).
    if (!in.wide && !in.det && ncu > 0 && in.nwaves > ncu * kWpb) {
        const long long extra = in.nwaves - ncu * kWpb;
        int xa = extra <= 2 * ncu ? 2 : kWpb;
        // dense (as requested before the observations) with the split extra waves: one group per extra
        // workgroup while they fit one per CU (cfg3 dense 63.5 -> 62.2 us, profiles/r5/spread_knobs.txt)
        if (in.topo_req == HMMBW_TOPOLOGY_DENSE && in.sw.split_extra && extra <= ncu) xa = 1;
        if (in.sw.xact) xa = std::max(1, std::min(kWpb, in.sw.xact));
        // left-to-right on the joined map: past 2 extra groups per CU they still join the full workgroups,
        // up to 4 per CU (cfg4 shard, 12,500 sequences: 135 workgroups of 8 waves instead of 2 x 135 of 4)
        const bool join4 = !in.sw.xact && xa == kWpb && in.sw.join && in.topo_req != HMMBW_TOPOLOGY_DENSE;
        if ((xa < kWpb || join4) && (extra + xa - 1) / xa <= ncu) {
            m.nfull = ncu;
            m.xact = xa;
            m.nblocks = m.nfull + (extra + xa - 1) / xa;
        }
    }
    m.fits_cus = ncu > 0 && m.nblocks <= ncu;
    m.sym2 = in.split_tables && (in.sw.lds_layout == 1 || (in.sw.lds_layout == -1 && m.nblocks > m.nfull &&
                                                           in.steps >= kSplitTablesMinSteps * in.nwaves));
    return m;
}

// The left-to-right E-step runs the joined spread map (k_estep_join): every extra workgroup of the spread map
// (at most one per CU) becomes waves 4.. of the full workgroup with its index, so each CU runs one 8-wave
// workgroup: one M-step prologue, one set of LDS tables and one histogram flush instead of two on the CUs
// that host an extra workgroup.  cfg3: 32.2 -> 30.9 us per iteration (profiles/r5/join_ab.txt).
// Round 6: the dense E-step joins too (HMMBW_JOIN_DENSE=0 keeps its separate extra workgroups); its split B
// waves take A's hand-over through an LDS flag, so the joined workgroup's full waves are never held.
// topo: the resolved topology (HMMBW_TOPOLOGY_DENSE or _LEFT_TO_RIGHT)
inline bool joined(const LaunchMap &m, int topo) {
    const bool topo_ok = topo == HMMBW_TOPOLOGY_LEFT_TO_RIGHT || (topo == HMMBW_TOPOLOGY_DENSE && m.sw.join_dense);
    const int xw = (topo == HMMBW_TOPOLOGY_DENSE && m.sw.split_extra && 2 * m.xact <= kWpb) ? 2 * m.xact : m.xact;
    // Round 6: left-to-right without extra groups too (at most 4 groups per CU, one workgroup per CU), the idle waves
    // 4-7 then only sharing the prologue's table build and the flush: T = 8 at 8,192 sequences 13.51 -> 12.96 us,
    // 8,192 x 200 27.59 -> 27.32, 4,096 x 200 24.30 -> 23.72 (profiles/r6/join_all_ab.txt)
    const bool all = topo == HMMBW_TOPOLOGY_LEFT_TO_RIGHT && m.nblocks == m.nfull && m.fits_cus;
    return m.sw.join && topo_ok && m.lds_atomic && (m.nblocks > m.nfull || all) && m.nblocks - m.nfull <= m.nfull &&
           xw <= kWpb;
}

// the joined launch reads the class-split tables (have_sym2: the context holds their packs)
inline bool split_tables_on(const LaunchMap &m, int topo, bool have_sym2) {
    return m.split_tables && have_sym2 && joined(m, topo) &&
           (m.sw.lds_layout == 1 || topo == HMMBW_TOPOLOGY_LEFT_TO_RIGHT);
}

// The split extra waves run in a launch (estep_small_body SPLITOK, "split"; EArgs::split_extra): dense, and
// left-to-right on the joined launch only (round 6, cfg3 29.63 -> 28.33 us, profiles/r6/split_lr_ab.txt); beside
// separate extra workgroups they cost more than they save (round 5: 34.0 -> 35.6 us).
// joined_launch: the launch in question is the joined one (the E-step's, when joined(m, topo))
inline bool split_extra_on(const LaunchMap &m, int topo, bool joined_launch) {
    const bool topo_ok = topo == HMMBW_TOPOLOGY_DENSE || (topo == HMMBW_TOPOLOGY_LEFT_TO_RIGHT && joined_launch);
    return m.sw.split_extra && topo_ok && m.lds_atomic && m.nblocks > m.nfull && 2 * m.xact <= kWpb;
}

// ---------------------------------------------------------------------------------------------
// The kernel's side of the map: what wave wv of workgroup bid runs.  estep_small_body keeps this arithmetic
// written out (the wpb .. wactive block): calling wave_role there changed the small kernels' register
// allocation (profiles/r8/isa_identity.txt), so this is the statement of it that the CPU test checks against
// the map; change the two together.
// ---------------------------------------------------------------------------------------------
struct WaveRole {
    long long wave;  // sequence group (active only below the wave count)
    int slot;        // the group's hand-over slot among its workgroup's extra groups
    bool xblk;       // this wave runs an extra group
    bool split;      // ... in a workgroup whose extra groups are split
    bool brole;      // ... as the B partner: the lower half of the group's backward
    bool active;
};

// JOIN: the joined map (waves wpb.. of workgroup bid run extra workgroup bid's groups); wpb: waves of a full
// workgroup; split_allowed: the kernel can split (SPLITOK) and EArgs::split_extra is set
template <bool JOIN>
HMMBW_HD inline WaveRole wave_role(long long bid, int wv, int wpb, long long nfull, int xact, bool split_allowed) {
    const bool xblk = JOIN ? wv >= wpb : bid >= nfull;
    const int wx = JOIN ? wv - wpb : wv;  // index among the extra group's waves
    // split extra waves: with 2 xact <= 4 extra waves, extra wave wx in [xact, 2 xact) is the B partner of extra
    // wave wx - xact (same sequence group): it runs the lower half of the group's backward
    const bool split = split_allowed && xblk && 2 * xact <= wpb;
    const bool brole = split && wx >= xact && wx < 2 * xact;
    const int wvg = brole ? wv - xact : wv;
    const int slot = JOIN ? wvg - wpb : wvg;
    const long long wave = JOIN ? (xblk ? nfull * wpb + bid * xact + (wvg - wpb) : bid * wpb + wv)
                                : (xblk ? nfull * wpb + (bid - nfull) * xact + wvg : bid * wpb + wv);
    return WaveRole{wave, slot, xblk, split, brole, !xblk || wx < xact || brole};
}

}  // namespace hmmbw
