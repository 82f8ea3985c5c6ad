// hmmbw_args.hpp — the argument structs the host fills and the kernels read, with their constants.
// All a host unit needs of the device side (host.hpp includes this and no device code).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "obs_plan.hpp"  // kWave, kChunk, kBlock

namespace hmmbw {

constexpr int kHist = 4096;

struct IterState {
    double prev_L;
    double last_L;
    double last_diff;
    double epsilon;
    long long iteration;
    long long max_iterations;
    int done;
    int converged;
    int error;      // HMMBW_E_* of a device-side failure; done is set with it
    int error_src;  // which bounded wait failed: kErrPeer (peer all-reduce) or kErrWorkQueue (wide work queue)
};
constexpr int kErrPeer = 1;
constexpr int kErrWorkQueue = 2;

// Observation layout in HBM (built once by hmmbw_set_observations).
//   slot = wave * U + u  ->  caller sequence slot_seq[slot] (-1: padding), length slot_len[slot]
//   sym    : per wave, chunk-major [chunk][u][8] uint16  (one 16-B load = 8 steps of one sequence)
//   ckpt   : per wave [chunk][64 lanes] fp64 — alpha_hat at the first step of every chunk (small N)
//   spack  : per wave [chunk][u] 8 x int16 — the power-of-two scale exponent of every step
//   alpha  : per wave [t][64 lanes] fp64 + ebuf [t][u] int32 — full alpha_hat (wide kernel only)
struct Layout {
    const uint16_t *sym;
    const long long *wave_symoff;
    const long long *wave_ckoff;   // doubles (small) | alpha doubles (wide)
    const long long *wave_spoff;   // uint4 units (small) | ebuf ints (wide)
    const int *wave_T;
    const int *wave_full;          // 1: every real slot of the wave has length wave_T
    const int *slot_len;
    const int *slot_seq;
    long long nwaves;
};

// Host-visible mirror of the convergence state (HMMBW_OPT_LIVE_STATUS), in fine-grained pinned host
// memory: every M-step that records an iteration also writes the record and the new state here with
// write-through stores, then publishes pub = epoch << 32 | iteration.  The state goes to slot
// iteration % 2, so a reader that sees pub unchanged around its copy of that slot read one record.
struct LiveBlock {
    unsigned long long pub;
    unsigned long long pad_[7];
    IterState slot[2];
    double hist[2 * kHist];  // (L, diff) of iteration i at 2 (i % kHist)
};

// Column of state j in the wide kernels' emission table (estep_mfma.hpp; MArgs::bt_perm): j = 16m + 4r + g is
// stored at 16m + 4g + r, so the 4 states one lane owns are contiguous.
__host__ __device__ inline int bt_col(int j) { return (j & ~15) | ((j & 3) << 2) | ((j >> 2) & 3); }

struct MArgs {
    const double *src;     // statistics: the copies (single rank) or the all-reduced buffer
    double *zero_ll;       // LL slots to clear (multi-rank) or nullptr
    int nsrc;
    long long copy_len;
    double *pi, *A, *B, *Bt;
    const double *llpart;
    long long nblocks;
    long long R_global;
    const IterState *state;  // convergence state entering this M-step
    IterState *state_out;    // ... and after it (double-buffered: the host flips the slots per M-step)
    double *hist;
    int N, K, G, world;
    int local_lse;
    int bt_perm;           // 1: B^T columns in the wide kernels' order (bt_col)
    long long off_S, off_gex, off_gall, off_bnum, off_ll;
    LiveBlock *live;       // HMMBW_OPT_LIVE_STATUS: the host mirror (or nullptr)
    unsigned live_epoch;   // the host's reset count: records of an earlier run never match
};

// statistics per launch the merged M-step prologue (merged_mstep, hmmbw_device.hpp) holds in registers: the
// host merges the M-step into the E-step launch up to this copy_len
constexpr int kMergedMaxStats = 16 * kBlock;

struct EArgs {
    Layout L;
    const double *pi;
    const double *A;
    const double *Bt;  // [K][G] + G zero pad
    double *ckpt;      // small: checkpoints | wide: alpha_hat
    double *gam;       // wide: gamma rows [position][NP] (bt_col order) for k_bnum_gather
    const unsigned *gdst;  // wide: row of position (tile row = wave_ckoff / NP + t * 16 + s) in symbol order
    uint4 *spack;      // small: scale exponents
    int *ebuf;         // wide: scale exponents
    double *copies;    // [ncopies][copy_len] statistics accumulators (workgroup b adds into copy b % ncopies)
    long long copy_len;
    int ncopies;
    double *logp;
    double *llpart;    // [blocks][2]: per-block (max, sum exp) of log P
    const IterState *state;
    int K;
    int N;
    int force_safe;    // 1: per-step normalisation (no lagged scaling)
    int ablate;        // diagnostics only: bit 0 skips the statistics flush, bit 1 the backward sweep
    int merged;        // 1: run the previous iteration's M-step (m) in the prologue of every workgroup
    double *zero;      // statistics buffer of the NEXT iteration, cleared by this launch (or nullptr)
    long long zero_len;
    double *part;      // deterministic mode: per-workgroup partial statistics [blocks][off_bnum]
    double *rank_ll;   // multi-rank fused: this rank's (max, sum exp) slot in the all-reduce buffer (or nullptr)
    int *done_ctr;     // ... and the workgroup completion counter that picks the workgroup forming it
    MArgs m;
    long long off_S, off_gex, off_gall, off_bnum;
    // wave -> workgroup map of the small kernels: workgroups [0, nfull) run 4 sequence-group waves each,
    // the workgroups after them only xact (the waves beyond one per SIMD spread over more CUs)
    long long nfull;
    int xact;
    // wave priority (HMMBW_PRIO overrides): 2 (default) = s_setprio 1 for the spread map's extra waves, the
    // second wave on their SIMDs (cfg3 34.5-34.7 us per iteration against 36.0-36.8 at 0, two interleaved
    // rounds; no effect without extra waves, e.g. 12,500 sequences); 1 = for the full workgroups' waves
    int prio;
    // split extra waves (small kernels, LDS tables): the idle waves of the spread map's extra workgroups run
    // the lower half of their partner's backward sweep (estep_small_body, "split"); 0 off
    int split_extra;
    // wide work queue (k_estep_mfma<..., WQ>): [0] next unit, [1] workgroups done; per-tile forward flags
    unsigned *wq;
    unsigned *wq_flag;
    int wq_units;  // tiles
    long long wq_timeout_ticks;  // bound (wall-clock ticks) of a backward unit's wait for its forward
};

// Grouped launch (k_estep_small_group): per-model arguments and first workgroups (start[nm] = grid)
struct GroupArgs {
    const EArgs *__restrict__ args;
    const long long *__restrict__ start;
    int nm;
};

}  // namespace hmmbw
