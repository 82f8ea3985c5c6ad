// host.hpp — what the host-side units share (internal; declarations only): the error channel, the
// allocator's interface, the timing event pool, the launch plan, the context and the few helpers that
// cross units.  Owners: alloc.hip (block cache, ledger), peer.hip (peer all-reduce), comm.hip (RCCL),
// group.hip (grouped launches), viterbi.hip (hmmbw_viterbi and its kernels), posterior.hip (hmmbw_posterior and
// its kernels), wordnet.hip (hmmbw_wordnet_decode and its kernels), embedded.hip (hmmbw_embedded_train and its
// kernels; it keeps nothing in the context), align.hip (hmmbw_align and its kernels), train.hip (the M-step kernels
// and the pending M-step, hmmbw_reset_training / _estep / _mstep / _iterate*), status.hip (the status readers, the
// snapshot slots and the live mirror), hmmbw.hip (the life cycle, observations, options, parameters, the launch
// planner, scoring and timing).  What wordnet.hip, embedded.hip and align.hip share beyond this
// header, and the slot arguments they fill as viterbi.hip and posterior.hip do, is word_units.hpp's.
// The observation layout and the launch map hmmbw.hip plans are obs_plan.hpp's: pure, shared with the
// kernels, tested without a GPU (tests/test_obs_plan.py).
#pragma once

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>
#include <rccl/rccl.h>

#include "hmmbw_args.hpp"
#include "hmmbw_kernels.hpp"
#include "lds_layout.hpp"
#include "obs_plan.hpp"
#include "viterbi_plan.hpp"
#include "wordnet_plan.hpp"

namespace hmmbw {

extern thread_local std::string g_err;  // hmmbw_last_error
int fail(int code, const std::string &msg);

#define HIP_TRY(expr)                                                                            \
    do {                                                                                         \
        hipError_t _e = (expr);                                                                  \
        if (_e != hipSuccess)                                                                    \
            return fail(HMMBW_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));         \
    } while (0)

// alloc.hip: the block cache of small device buffers and pinned blocks, and the allocation ledger
// (HMMBW_DEBUG_ALLOC) that also tracks the allocations made past the cache
enum { kDevBlock = 0, kPinnedBlock = 1 };
hipError_t cached_alloc(void **p, size_t bytes, int kind);
void cached_free(void *p, int kind);
size_t cache_trim();
void ledger_add(const void *p, size_t bytes, const char *what);
void ledger_remove(const void *p, const char *what);

template <class T>
int dalloc(T **p, size_t n) {
    *p = nullptr;
    if (n == 0) n = 1;
    HIP_TRY(cached_alloc(reinterpret_cast<void **>(p), n * sizeof(T), kDevBlock));
    return HMMBW_OK;
}

template <class T>
void dfree(T *&p) {
    cached_free(p, kDevBlock);
    p = nullptr;
}

// Pool of HIP event pairs (start, stop) for timing: the context's E-step launches, its all-reduces and a
// group's launches each own one.  take() .. done() bracket the timed work on a stream; drain() waits for
// the queued pairs and adds their times to ms / n.
struct EventPairs {
    std::vector<hipEvent_t> free, pending;  // pending: (start, stop), (start, stop), ...
    hipEvent_t e0 = nullptr, e1 = nullptr;  // the pair between take and done
    double ms = 0.0;
    long long n = 0;
    int take(hipStream_t stream);  // a pair from the pool; records its start
    int done(hipStream_t stream);  // records the stop and queues the pair
    int drain();
    void destroy();
};

// Where one E-step launch reads and writes.  The three ways of filling it are hmmbw_ctx's io_local, io_packed and
// io_fused, next to copies(e) / llpart(e).
struct EstepIo {
    const IterState *state = nullptr;  // the convergence state the launch reads (a done run is a no-op)
    double *copies = nullptr;          // [ncopies][copy_len] statistics the launch adds into
    double *llpart = nullptr;          // the per-workgroup (max, sum exp) pairs of log P it writes
    double *zero = nullptr;            // zero_len doubles it clears for a later launch, or nullptr
    long long zero_len = 0;
    double *rank_ll = nullptr;         // fused all-reduce: this rank's pair, written by the last workgroup; or nullptr
    int ncopies = 0;
};

// One E-step / scorer launch of a context, resolved but not yet enqueued (launch_estep / launch_score enqueue
// it alone, group_launch concatenates several contexts' plans into one grouped launch).
struct Plan {
    EArgs a{};
    KernelFn fn = nullptr;
    GroupFn gfn = nullptr;
    unsigned grid = 0, block = kBlock;
    size_t lds = 0;
    bool flip = false;
    long long nll = 0;  // per-workgroup log-likelihood pairs the launch writes (tiles on the wide work queue)
};

}  // namespace hmmbw

using namespace hmmbw;

struct hmmbw_ctx {
    int device = 0, N = 0, K = 0, G = 0, U = 0;
    bool wide = false;
    int NP = 0;
    int topo_req = HMMBW_TOPOLOGY_AUTO, topo = HMMBW_TOPOLOGY_DENSE;
    int rank = 0, world = 1;
    hipStream_t stream = nullptr;
    // parameters (linear, working copy)
    double *d_pi = nullptr, *d_A = nullptr, *d_B = nullptr, *d_Bt = nullptr, *d_out = nullptr;
    std::vector<double> h_A;
    bool has_params = false;
    // training state
    IterState *d_state = nullptr;  // [2]: the current slot is scur; every M-step writes the other
    int scur = 0;
    double *d_hist = nullptr;
    // hmmbw_status_post / _wait: two pinned snapshots (state + record ring) taken on the stream
    struct Snap {
        hipEvent_t ev = nullptr;
        IterState *st = nullptr;
        double *hist = nullptr;  // records [first, st->iteration)
        long long first = 0;
        long long ticket = -1;
    } snaps[2];
    long long snap_next = 0;
    // HMMBW_OPT_LIVE_STATUS: the host mirror every recording M-step writes (hmmbw_status_live_wait)
    LiveBlock *h_live = nullptr;
    unsigned live_epoch = 1;
    double *d_copies = nullptr;   // [3][ncopies][copy_len] E-step accumulators (iteration e uses e % 3)
    int ncopies = 2;              // HMMBW_OPT_STAT_COPIES default: halves the flush atomics per address (measured -3 %)
    bool merge_mstep = true;      // run each M-step in the prologue of the next E-step launch
    bool det = false;             // HMMBW_OPT_DETERMINISTIC: no floating-point atomics (LDS-table or wide kernels)
    double *d_part = nullptr;     // det: per-workgroup partial statistics [blocks][off_bnum]
    bool armed = false;
    long long e_count = 0;        // E-step launches since the statistics were last cleared
    // an M-step whose statistics are ready but which has not run yet (it runs in the next merged
    // E-step launch, or on its own in flush_mstep before anything reads parameters or state)
    struct Pending {
        bool on = false;
        bool local = true;        // statistics are this context's copies (single rank)
        const double *src = nullptr;
        int nsrc = 1;
        const double *ll = nullptr;  // (max, sum exp) pairs of log P
        long long nll = 0;
        double *ext = nullptr;    // multi-rank: the caller's all-reduced buffer
        long long R = 0;
    } pend;
    // observations
    long long R = 0, nwaves = 0;
    MapSwitches sw;               // the map's A/B switches and HMMBW_OPT_LDS_LAYOUT (obs_plan.hpp)
    LaunchMap map;                // the wave -> workgroup launch map of the observations (obs_plan.hpp, plan_map;
                                  // stored by set_observations with everything else)
    int prio = -1;                // wave priority of the small kernels (EArgs::prio): -1 auto (left-to-right 2,
                                  // dense 0: profiles/r5/spread_knobs.txt); HMMBW_PRIO overrides it
    long long last_nll = 0;       // per-workgroup log-likelihood pairs written by the last E-step launch
    uint16_t *d_sym = nullptr;
    uint16_t *d_sym2 = nullptr;   // the packs of the class-split tables (row offsets o 2 G 16), or nullptr: the
                                  // joined kernel alone reads them; every other kernel keeps d_sym and its layout
    long long *d_wsym = nullptr, *d_wckoff = nullptr, *d_wspoff = nullptr;
    int *d_wT = nullptr, *d_wfull = nullptr, *d_slen = nullptr, *d_sseq = nullptr;
    double *d_ck = nullptr, *d_logp = nullptr, *d_llpart = nullptr;  // llpart: [2][nblocks][2]
    long long cktot = 0;          // checkpoint doubles of the layout
    double *d_zf = nullptr;       // dense small kernels: every z_t, kChunk x cktot (allocated on first use)
    // wide path: gamma rows per position and the symbol -> rows index of k_bnum_gather
    double *d_gam = nullptr;
    long long *d_bptr = nullptr;
    unsigned *d_brows = nullptr;
    unsigned *d_wq = nullptr;  // wide work queue (EArgs::wq): 2 counters + a flag per tile, or nullptr
    long long wq_grid = 0;     // its grid (a workgroup per unit: 2 x tiles)
    int wq_mode = -1;          // HMMBW_OPT_WIDE_WQ: -1 auto (from 4 tiles per CU), 0 off, 1 on (more tiles than CUs)
    long long wq_timeout_ms = 10000;  // HMMBW_OPT_WQ_TIMEOUT_MS: bound of a backward unit's wait
    uint4 *d_sp = nullptr;
    int *d_ebuf = nullptr;
    // hmmbw_viterbi (viterbi.hip): the host's copy of the layout's slot arrays (set_observations) and the
    // decoder's buffers, allocated on first use and freed with the observations
    std::vector<int> h_slen, h_sseq;
    struct Viterbi {
        bool planned = false;
        ViterbiPlan plan;                 // slot_out / psi_off are moved to the device, the figures stay
        double *d_tab = nullptr;          // [GV] log pi | [GV][GV] log A (lane j's column contiguous) | [K][GV] log B^T
        long long *d_slot_out = nullptr, *d_psi_off = nullptr;
        double *d_logp = nullptr;
        int32_t *d_path = nullptr;        // with paths only: caller CSR order
        unsigned char *d_psi = nullptr;   // with paths only: back-pointers, [t][64 lanes] bytes per decoding wave
    } vit;
    // hmmbw_posterior (posterior.hip): it shares the decoder's plan, offsets and device logp; its own buffers are
    // allocated on first use and freed with the observations
    struct Posterior {
        double *d_tab = nullptr;      // [GV] pi | [GV][GV] A row-major | [K][GV] B^T, linear, 0 in states >= N
        double *d_scratch = nullptr;  // [total][N]: the alpha_hat -> gamma workspace of calls without gamma_dev
        int32_t *d_path = nullptr;    // with paths only: caller CSR order
    } post;
    // hmmbw_wordnet_decode (wordnet.hip) and hmmbw_align (align.hip): both share the decoder's slot_out and device
    // logp; their own buffers are allocated on first use (the back-pointers on the first call with paths) and freed
    // with the observations.  WordDecode is what the two keep alike (word_units.hpp, word_decode_buffers).
    struct WordDecode {
        int GW = 0;                        // the group width d_psi_off and d_bp were planned for (0: none)
        long long rows = 0, nvw = 0;       // back-pointer rows of all decoding waves | decoding waves
        long long *d_psi_off = nullptr;    // decoding wave -> its first back-pointer row
        double *d_in = nullptr, *d_tab = nullptr;  // the staged bank (linear) | the log tables (wordnet_plan.hpp, align_plan.hpp)
        size_t n_in = 0, n_tab = 0;        // their lengths in doubles
        int32_t *d_path = nullptr;         // with paths only: caller CSR order of the observations
    };
    struct Wordnet : WordDecode {
        unsigned char *d_start = nullptr;  // with paths only: caller CSR order
        unsigned char *d_bp = nullptr;     // with paths only: rows x kWnRowBytes
    } wn;
    struct Align : WordDecode {
        long long *d_word_off = nullptr;   // [R + 1] the transcripts, CSR in caller order
        int *d_word_ids = nullptr;
        size_t n_ids = 0, n_bounds = 0;    // lengths in elements
        int32_t *d_bounds = nullptr;       // with paths only: caller CSR order of the transcripts
        unsigned *d_bp = nullptr;          // with paths only: rows x 64 lanes
        // hmmbw_align_optional with flags only
        unsigned char *d_opt = nullptr;    // a byte per transcript position, d_word_ids' order
        size_t n_opt = 0;
        unsigned long long *d_skip = nullptr;  // with paths: rows lane masks (align_plan.hpp, align_skip_bytes)
    } al;
    // native RCCL communicator (hmmbw_comm_init): the multi-rank hmmbw_iterate all-reduces d_ext
    ncclComm_t comm = nullptr;
    double *d_ext = nullptr;      // non-fused multi-rank paths: the packed statistics to all-reduce
    long long ext_len = 0;
    // hmmbw_iterate_begin / _end: one multi-rank iteration split at its all-reduce (the same enqueue
    // sequence hmmbw_iterate runs around ncclAllReduce); open between the two calls
    bool ar_open = false;
    bool ar_fused = false;
    double *ar_cur = nullptr;
    long long ar_R = 0;
    // fused native path (small kernels): the E-step accumulates straight into a triple-buffered
    // all-reduce buffer [3][xlen] = {ncopies statistics copies, (max, sum exp) per rank}; the last
    // workgroup of each launch writes the rank's pair (d_ctr: completion counter)
    double *d_xbuf = nullptr;
    // peer all-reduce (HMMBW_OPT_ALLREDUCE = 1): this rank's receive region, every rank's region as
    // addressable here (attached), the IPC mappings to close, and the iteration sequence number
    // (owned by peer.hip: the other units go through peer_mode() and the peer_* calls below)
    int ar_kind = HMMBW_ALLREDUCE_RCCL;
    long long peer_timeout_ms = 30000;  // HMMBW_OPT_PEER_TIMEOUT_MS
    struct Peer {
        double *region = nullptr;     // this rank's receive region
        size_t bytes = 0;
        long long n = 0, slot = 0, nch = 0;
        int dpt = 1;
        double *d_xsum = nullptr;     // the all-reduced sums the pending M-step reads (peer mode)
        int world = 0;
        bool on = false;
        bool revoked = false;         // a region this context was attached to was freed by its owner
        bool special = false;         // the region is uncached / fine-grained (HMMBW_PEER_MEM)
        double perturb = 0.0;         // diagnostics: HMMBW_DIAG_PEER_PERTURB=<rank>:<value> (bench's leg check)
        std::vector<double *> regions;
        std::vector<void *> mapped;
        unsigned long long seq = 0;
    } peer;
    long long wall_khz = 100000;  // hipDeviceAttributeWallClockRate (100 MHz on MI355X)
    long long ar_len_last = 0;    // doubles in the last all-reduce hmmbw_iterate enqueued
    long long xlen = 0;
    int *d_ctr = nullptr;
    // all-reduce timing (hmmbw_comm_info): event pairs around ncclAllReduce, same schedule as timing
    long long ar_seq = 0;
    EventPairs ar_timed;
    long long R_global = 0;
    bool has_obs = false;
    int force_safe = 0;
    int ablate = 0;
    // timing
    int timing = 0;              // 0: off; k >= 1: time every k-th E-step launch
    long long timing_seq = 0;
    EventPairs timed;
    // launches with a follow-up kernel (wide: k_bnum_gather): an event between the E-step kernel and
    // it, one entry per pending pair (nullptr: none), so hmmbw_timing_split can price the E-step alone
    std::vector<hipEvent_t> mid_free, mid_pending;
    double timed_main_ms = 0.0;
    long long timed_main_n = 0;

    long long off_S() const { return N; }
    long long off_gex() const { return N + (long long)N * N; }
    long long off_gall() const { return off_gex() + N; }
    long long off_bnum() const { return off_gall() + N; }
    long long off_ll() const { return off_bnum() + (long long)K * N; }
    long long stats_len() const { return off_ll() + 2LL * world; }
    long long copy_len() const { return off_ll(); }
    // emission P/H tables in LDS (two [K][G] tables of 16-B entries kHistOff bytes apart, see
    // hmmbw_device.hpp) when the first fits below kHistOff (the row offsets then fit the uint16 packs)
    bool lds_tables() const { return !wide && lds_tables_fit(K, G); }
    // LDS doubles of the small kernels' tables
    size_t lds_table_doubles() const { return lds_tables() ? lds_table_bytes(K, G) / sizeof(double) : 0; }
    // the class-split tables (lds_layout.hpp, lay2_p_off) can serve this context's joined launches: G = 8,
    // the rows of one class within 64 KiB (uint16 packs); both classes and the b table then fit the CU's 160 KiB
    // with the scratch and the kernel's static LDS (lay2_lds_fit)
    bool split_tables() const {
        return sw.lds_layout != 0 && !wide && !det && G == 8 && lds_tables() && lay2_lds_fit(K, G);
    }
    size_t split_table_doubles() const { return lay2_total_bytes(K, G) / sizeof(double); }
    bool can_merge() const { return merge_mstep && lds_tables() && copy_len() <= kMergedMaxStats && nwaves > 0; }
    // statistics copies in the fused all-reduce buffer: the wide path's B numerator is written once (by
    // k_bnum_gather, into copy 0), and its tiles finish at different times, so its atomics need no
    // spreading: one copy, and the all-reduce carries no K x N block of zeros (cfg5: 0.56 MB, not 1.1)
    int xcopies() const { return wide ? 1 : ncopies; }
    // doubles of the per-iteration multi-rank all-reduce: the fused buffer (copies + one (max, sum exp)
    // pair per rank, 256-B aligned) or, in deterministic mode, the packed statistics
    long long ar_payload() const {
        return det ? stats_len() : ((long long)xcopies() * copy_len() + 2LL * world + 31) / 32 * 32;
    }
    bool peer_mode() const { return ar_kind == HMMBW_ALLREDUCE_PEER && peer.on; }
    IterState *state() const { return d_state + scur; }
    double *copies(long long e) const { return d_copies + (e % 3) * (long long)ncopies * copy_len(); }
    double *llpart(long long e) const { return d_llpart + (e % 2) * 2 * std::max(map.nblocks, 1LL); }
    // E-step launch e of a single rank.  Statistics triple buffer: the launch adds into e, the merged M-step reads
    // e - 1, and e + 1 (read by launch e - 2) is cleared for the next launch.
    EstepIo io_local(long long e) const {
        return EstepIo{state(), copies(e), llpart(e), copies(e + 1), (long long)ncopies * copy_len(), nullptr, ncopies};
    }
    // hmmbw_estep: one copy set, summed into the caller's packed statistics and cleared by k_reduce_local
    EstepIo io_packed(long long e) const { return EstepIo{state(), copies(0), llpart(e), nullptr, 0, nullptr, ncopies}; }
    // Fused all-reduce: the launch adds into buffer e of d_xbuf (the merged M-step reads the previous, all-reduced
    // one), clears the next, and its last workgroup writes this rank's pair behind the xcopies() statistics copies.
    EstepIo io_fused(long long e) const {
        double *X = d_xbuf + (e % 3) * xlen, *Xn = d_xbuf + ((e + 1) % 3) * xlen;
        const long long ll_off = (long long)xcopies() * copy_len();
        return EstepIo{state(), X, llpart(e), Xn, xlen, X + ll_off + 2LL * rank, xcopies()};
    }
};

namespace hmmbw {

// hmmbw.hip
int set_device(hmmbw_ctx *c);
void sync_ctx(hmmbw_ctx *c);
long long ms_to_ticks(const hmmbw_ctx *c, long long ms);
int check_ready(hmmbw_ctx *c, bool need_armed);
int check_closed(const hmmbw_ctx *c);  // HMMBW_E_STATE between hmmbw_iterate_begin and _end
int allow_lds(const void *f, size_t lds);
// Resolve a training launch that reads and writes io; it runs the pending M-step in its prologue when that can
// merge (which consumes c->pend).  allow_join: the joined spread map may serve it (a grouped launch cannot).
int plan_estep(hmmbw_ctx *c, const EstepIo &io, bool allow_join, Plan *P);
int plan_score(hmmbw_ctx *c, Plan *P);  // the forward-only scorer: log P of every sequence into d_logp
int launch_estep(hmmbw_ctx *c, const EstepIo &io);
int launch_score(hmmbw_ctx *c);
int drain_timing(hmmbw_ctx *c);  // the queued E-step timing pairs into the context's sums

// train.hip
void init_state(hmmbw_ctx *c, IterState *slot, double epsilon, long long max_iterations);  // enqueues k_init_state
MArgs make_margs(hmmbw_ctx *c, const hmmbw_ctx::Pending &p);
int flush_mstep(hmmbw_ctx *c);
// head of every training enqueue: the pending M-step runs now if the launch cannot merge it; *e: the launch's number
int next_estep(hmmbw_ctx *c, long long *e);
// the statistics of E-step launch e (nll log-likelihood pairs) become the pending M-step's input
void pend_local(hmmbw_ctx *c, long long e, long long nll);

// status.hip
int live_status_set(hmmbw_ctx *c, bool on);  // HMMBW_OPT_LIVE_STATUS: allocate and seed the host mirror, or free it
void status_free(hmmbw_ctx *c);  // the snapshot slots and the live mirror; callers synchronise the device first

// viterbi.hip
void viterbi_free(hmmbw_ctx *c);  // the decoder's buffers; callers synchronise the context first
int viterbi_plan_ready(hmmbw_ctx *c);  // c->vit.plan, d_slot_out and d_logp of the loaded observations (made once)

// posterior.hip
void posterior_free(hmmbw_ctx *c);  // hmmbw_posterior's buffers; callers synchronise the context first

// wordnet.hip
void wordnet_free(hmmbw_ctx *c);  // hmmbw_wordnet_decode's buffers; callers synchronise the context first

// align.hip
void align_free(hmmbw_ctx *c);  // hmmbw_align's buffers; callers synchronise the context first

// peer.hip
std::string peer_off_msg(const hmmbw_ctx *c);
void peer_detach(hmmbw_ctx *c);
void peer_destroy(hmmbw_ctx *c);  // detach, free the region and the sums; callers synchronise the device first
int peer_push(hmmbw_ctx *c, const double *buf, long long len);
int peer_allreduce(hmmbw_ctx *c, double *buf, long long len);
int peer_reduce(hmmbw_ctx *c);
int peer_info(const hmmbw_ctx *c, int key, int64_t *value);  // the HMMBW_INFO_PEER_* keys of hmmbw_get_option

// comm.hip
int comm_allreduce(hmmbw_ctx *c, double *buf, long long len);  // ncclAllReduce (sum, in place) on the stream
void comm_destroy(hmmbw_ctx *c);

}  // namespace hmmbw
