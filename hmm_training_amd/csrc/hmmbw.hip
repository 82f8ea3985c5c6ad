// hmmbw.hip — MI355X (gfx950, CDNA4) Baum-Welch engine behind the C ABI in include/hmmbw.h.
//
// Replaces the hot path of DemianMArin/HMM_Training HMM/hmm_training.py:265-541 (hmm_training):
//   E-step  :351-410  forward alpha / backward beta (calculate_log_alpha :122-160,
//                     calculate_log_beta :163-199), gamma, xi
//   M-step  :415-500  pi, A, B re-estimation (incl. the 1e-20 floor at :497)
//   converge:503-514  L = LSE_r log P_r, diff, stop rule of :346
//   finalise:524-541  safe_exp + normalisation
// and the forward-only scorer of HMM/hmm_testing.py:49-104.
//
// Numerics.  The reference works in the log domain.  Here every recursion is
// fp64 *scaled linear*: alpha_t is renormalised by an exact power of two 2^-e_t (frexp/ldexp, no
// rounding), log P = log(sum alpha_hat_{T-1}) + ln2 * sum_t e_t, beta_hat shares the same scale
// factors (Rabiner scaling with c_t = 2^e_t), so gamma_t = alpha_hat_t * beta_hat_t and
// xi_t(i,j) = a_ij * alpha_hat_t(i) * v_{t+1}(j) with v = b(o_{t+1}) * beta_hat_{t+1} * 2^-e_{t+1}.
// The reference's "-inf term dropped" rules are exactly "zero term adds nothing" here.
//
// Kernel map:
//   k_estep_small<N,G,LR,LDSTAB,FWD_ONLY>  N <= 16: a sequence is a group of G = pow2ceil(N) lanes,
//        lane j = state j, 64/G sequences per wavefront.  Cross-lane exchange by DPP (quad_perm,
//        row_shr/shl, row_half_mirror, row_mirror, row_newbcast); B^T and the B-numerator histogram
//        in LDS; the forward sweep stores one alpha_hat checkpoint per 8-step chunk plus the int16
//        scale exponents, the backward sweep recomputes each chunk's alpha_hat in registers
//        (bit-identical) and fuses beta, gamma, xi and the histogram scatter (hmmbw_device.hpp).
//   k_estep_join<N,G,LR,LAY>, k_estep_small_group<...>  the same body on the joined spread map (one
//        8-wave workgroup per CU; LAY = 1: class-split LDS tables) and for several models in one launch.
//   k_estep_mfma<NT,FWD_ONLY,DET,WQ>       16 < N <= 64: a workgroup owns a tile of 16 sequences, wave m
//        the 16-state block m; the recursions and xi on the fp64 MFMA, the other waves' blocks through
//        LDS (estep_mfma.hpp).  k_bnum_gather sums its gamma rows per symbol into the B numerator.
//   k_det_reduce    (deterministic mode) sum the per-workgroup partial statistics in workgroup order: a
//                   follow-up of the E-step launch, as k_bnum_gather is (enqueue_plan).
//   k_finalise      the reference's return-path normalisation (:524-541).
//   train.hip:
//   k_reduce_local  (multi-rank) sum the statistics copies into the all-reduce buffer + the rank's
//                   (max, sum exp) pair of log P_r.
//   k_mstep / k_mstep_staged  one workgroup: L, M-step, convergence record, zero the statistics
//                   (staged: all statistics gathered into LDS with one batch of loads).
//   k_mstep_grid    large N x K (wide path): B re-estimated by the whole grid, the rest by workgroup 0.
//                   (Their bodies: mstep.hpp; merged into the next E-step launch: merged_mstep.)
//   k_init_state    the convergence state of a new run.
//   status.hip:
//   k_snapshot      the state and the iteration records into pinned host memory (hmmbw_status_post).
//   (peer.hip, viterbi.hip and vq.hip hold their own kernels.)
//
// Host units (host.hpp): this one holds the context's life cycle, observations, options and parameters,
// the launch planner (plan_estep / plan_score and their launches), scoring, timing and hmmbw_vq_encode;
// train.hip the M-step, the pending M-step and hmmbw_reset_training / _estep / _mstep / _iterate*, status.hip
// the status readers, alloc.hip the block cache and the allocation ledger, peer.hip the peer all-reduce (kernels
// included), comm.hip the RCCL communicator, group.hip the grouped launches, viterbi.hip the Viterbi decoder.
#include <map>
#include <mutex>

#include "host.hpp"

namespace hmmbw {

// Deterministic mode: sum the per-workgroup partial statistics [blocks][n] in workgroup order.
__global__ void __launch_bounds__(256) k_det_reduce(const double *part, long long nblocks, long long n, double *out,
                                                    const IterState *state) {
    if (state->done) return;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        double v = 0.0;
        for (long long b = 0; b < nblocks; ++b) v += part[b * n + i];
        out[i] = v;
    }
}

// safe_exp + normalisation of the returned parameters (:524-541)
__global__ void k_finalise(const double *pi, const double *A, const double *B, int N, int K, double *out) {
    double *opi = out, *oA = out + N, *oB = out + N + N * N;
    const int tid = threadIdx.x;
    if (tid == 0) {
        double s = 0.0;
        for (int i = 0; i < N; ++i) s += pi[i];
        for (int i = 0; i < N; ++i) opi[i] = pi[i] / s;
    }
    for (int i = tid; i < N; i += blockDim.x) {
        double s = 0.0;
        for (int k = 0; k < N; ++k) s += A[i * N + k];
        for (int k = 0; k < N; ++k) oA[i * N + k] = s > 0.0 ? A[i * N + k] / s : A[i * N + k];
        double sb = 0.0;
        for (int k = 0; k < K; ++k) sb += B[(long long)i * K + k];
        for (int k = 0; k < K; ++k) oB[(long long)i * K + k] = sb > 0.0 ? B[(long long)i * K + k] / sb : B[(long long)i * K + k];
    }
}

// ---------------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------------
thread_local std::string g_err;

int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

int EventPairs::take(hipStream_t stream) {
    while (free.size() < 2) {
        hipEvent_t x;
        HIP_TRY(hipEventCreate(&x));
        free.push_back(x);
    }
    e1 = free.back(); free.pop_back();
    e0 = free.back(); free.pop_back();
    HIP_TRY(hipEventRecord(e0, stream));
    return HMMBW_OK;
}

int EventPairs::done(hipStream_t stream) {
    HIP_TRY(hipEventRecord(e1, stream));
    pending.push_back(e0);
    pending.push_back(e1);
    e0 = e1 = nullptr;
    return HMMBW_OK;
}

int EventPairs::drain() {
    for (size_t i = 0; i + 1 < pending.size(); i += 2) {
        HIP_TRY(hipEventSynchronize(pending[i + 1]));
        float t = 0.f;
        HIP_TRY(hipEventElapsedTime(&t, pending[i], pending[i + 1]));
        ms += t;
        n += 1;
        free.push_back(pending[i]);
        free.push_back(pending[i + 1]);
    }
    pending.clear();
    return HMMBW_OK;
}

void EventPairs::destroy() {
    for (hipEvent_t e : free) (void)hipEventDestroy(e);
    for (hipEvent_t e : pending) (void)hipEventDestroy(e);
    free.clear();
    pending.clear();
}

// E-step kernel pointers live in the instantiation units (hmmbw_kernels.hpp)
template <bool LR, bool LDSTAB>
static Kernels pick_small_n(int N) {
    switch (N) {
#define CASE(n) \
    case n: return small_kernels_n<n>(LR, LDSTAB);
        CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8)
        CASE(9) CASE(10) CASE(11) CASE(12) CASE(13) CASE(14) CASE(15) CASE(16)
#undef CASE
        default: return Kernels{};
    }
}

int set_device(hmmbw_ctx *c) {
    HIP_TRY(hipSetDevice(c->device));
    return HMMBW_OK;
}

// the block cache hands a freed block to the next allocation at once (hipFree used to synchronise the
// device): the context's queued work must be done with a block before it is freed
void sync_ctx(hmmbw_ctx *c) {
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    else (void)hipDeviceSynchronize();
}

// wall-clock ticks of a bound in ms, saturated (a huge bound must not wrap to a negative count, which
// would end every wait at once)
long long ms_to_ticks(const hmmbw_ctx *c, long long ms) {
    const long long khz = std::max(1LL, c->wall_khz);
    if (ms <= 0) return 0;
    return ms > LLONG_MAX / khz ? LLONG_MAX : ms * khz;
}

// an integer from the environment: *v is written, and true returned, only if the variable is set
static bool env_int(const char *name, int *v) {
    const char *e = std::getenv(name);
    if (e) *v = std::atoi(e);
    return e != nullptr;
}

int check_closed(const hmmbw_ctx *c) {
    if (c->ar_open) return fail(HMMBW_E_STATE, "an iteration is open (hmmbw_iterate_end first)");
    return HMMBW_OK;
}

static void free_obs(hmmbw_ctx *c) {
    sync_ctx(c);
    dfree(c->d_sym); dfree(c->d_sym2); dfree(c->d_wsym); dfree(c->d_wckoff); dfree(c->d_wspoff);
    dfree(c->d_wT); dfree(c->d_wfull); dfree(c->d_slen); dfree(c->d_sseq);
    dfree(c->d_ck); dfree(c->d_sp); dfree(c->d_ebuf); dfree(c->d_logp); dfree(c->d_llpart); dfree(c->d_zf);
    dfree(c->d_gam); dfree(c->d_bptr); dfree(c->d_brows); dfree(c->d_part); dfree(c->d_wq);
    viterbi_free(c);
    posterior_free(c);
    wordnet_free(c);
    align_free(c);
    c->wq_grid = 0;
    c->has_obs = false;
}

static int realloc_stats(hmmbw_ctx *c) {
    sync_ctx(c);
    dfree(c->d_copies);
    c->pend.on = false;
    c->e_count = 0;
    const size_t n = 3 * (size_t)c->ncopies * c->copy_len();
    if (int rc = dalloc(&c->d_copies, n)) return rc;
    HIP_TRY(hipMemsetAsync(c->d_copies, 0, sizeof(double) * n, c->stream));
    return HMMBW_OK;
}

// what a launch's arguments take from the context; where it reads and writes is the EstepIo's (plan_launch)
static EArgs make_eargs(hmmbw_ctx *c) {
    EArgs a{};
    a.L = Layout{c->d_sym, c->d_wsym, c->d_wckoff, c->d_wspoff, c->d_wT, c->d_wfull, c->d_slen, c->d_sseq,
                 c->nwaves};
    a.pi = c->d_pi;
    a.A = c->d_A;
    a.Bt = c->d_Bt;
    a.ckpt = c->d_ck;
    a.gam = c->d_gam;
    a.gdst = c->wide ? c->d_brows : nullptr;
    a.part = c->d_part;
    a.spack = c->d_sp;
    a.ebuf = c->d_ebuf;
    a.copy_len = c->copy_len();
    a.logp = c->d_logp;
    a.force_safe = c->force_safe;
    a.ablate = c->ablate;
    a.K = c->K;
    a.N = c->N;
    a.off_S = c->off_S();
    a.off_gex = c->off_gex();
    a.off_gall = c->off_gall();
    a.off_bnum = c->off_bnum();
    a.nfull = c->map.nfull;
    a.xact = c->map.xact;
    a.prio = c->prio >= 0 ? c->prio : (c->topo == HMMBW_TOPOLOGY_LEFT_TO_RIGHT ? 2 : 0);
    return a;
}

// The largest dynamic LDS each kernel has been allowed so far on each device: hipFuncSetAttribute once
// per kernel and size, not on every launch (the LR cfg3 launch asks for 66,880 B every EM iteration).
struct LdsGrants {
    std::mutex mu;
    std::map<std::pair<int, const void *>, size_t> have;
};
static LdsGrants &lds_grants() {
    static LdsGrants g;
    return g;
}

int allow_lds(const void *f, size_t lds) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    LdsGrants &g = lds_grants();
    std::lock_guard<std::mutex> lk(g.mu);
    size_t &have = g.have[std::make_pair(dev, f)];
    if (have >= lds) return HMMBW_OK;
    HIP_TRY(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    have = lds;
    return HMMBW_OK;
}

template <class F>
static int launch_lds(F f, unsigned grid, size_t lds, hipStream_t stream, const EArgs &a, unsigned block = kBlock) {
    if (lds > 64 * 1024)
        if (int rc = allow_lds(reinterpret_cast<const void *>(f), lds)) return rc;
    hipLaunchKernelGGL(f, dim3(grid), dim3(block), lds, stream, a);
    HIP_TRY(hipGetLastError());
    return HMMBW_OK;
}

// Dense small kernels store every z_t (ZF, hmmbw_device.hpp): kChunk x the checkpoint layout.  Allocated
// as soon as observations and a dense A are both known (set_observations / set_params), so an
// out-of-memory surfaces there rather than in the first training call.
static int ensure_zf(hmmbw_ctx *c) {
    if (c->wide || !c->has_obs || !c->has_params || c->topo == HMMBW_TOPOLOGY_LEFT_TO_RIGHT || c->d_zf)
        return HMMBW_OK;
    if (int rc = dalloc(&c->d_zf, (size_t)std::max(c->cktot * kChunk, 1LL)))
        return fail(rc, "dense A: the forward's every-step store (" + std::to_string(8 * c->cktot * kChunk) +
                            " bytes) does not fit: " + g_err);
    return HMMBW_OK;
}

// Wide path with many tiles per CU: a workgroup per forward and per backward sweep, taken from a queue
// in dispatch order (k_estep_mfma<..., WQ>), so the CUs' loads even out in sweeps instead of whole
// tiles.  Measured (round 4): whole cfg5 (3,125 tiles) 12.06 against 12.37 ms per iteration; the cfg5
// shard (391 tiles, 1.5 per CU) 2.17 against 1.85 ms: with so few tiles per CU the backward sweeps
// (0.63 of a tile) start late and form the tail, so by default (HMMBW_OPT_WIDE_WQ = -1) the queue is
// used from 4 tiles per CU; 1 uses it whenever there are more tiles than CUs, 0 never (the environment
// variable HMMBW_WIDE_WQ = 0 / 1 gives the default of a new context).  (Re)allocates or frees the queue
// to match the current observations; the counters and flags start cleared.
static int ensure_wq(hmmbw_ctx *c) {
    bool want = false;
    if (c->has_obs && c->wide && !c->det && c->map.nblocks < (1LL << 30)) {
        const int ncu = c->map.ncu;  // the device's CU count (set_observations)
        if (ncu > 0 && c->wq_mode != 0) want = c->map.nblocks > (c->wq_mode == 1 ? ncu : 4LL * ncu);
    }
    if (c->d_wq && (!want || c->wq_grid != 2 * c->map.nblocks)) {
        sync_ctx(c);
        dfree(c->d_wq);
        c->wq_grid = 0;
    }
    if (want && !c->d_wq) {
        if (int rc = dalloc(&c->d_wq, (size_t)c->map.nblocks + 2)) return rc;
        HIP_TRY(hipMemset(c->d_wq, 0, sizeof(unsigned) * ((size_t)c->map.nblocks + 2)));
        c->wq_grid = 2 * c->map.nblocks;
    }
    return HMMBW_OK;
}

// Resolve the kernel, the grid and the arguments of a training (plan_estep) or scoring (plan_score) launch.  A
// training launch first runs the pending M-step in its prologue when that can merge (which consumes c->pend).
static int plan_launch(hmmbw_ctx *c, bool fwd_only, const EstepIo &io, bool allow_join, Plan *P) {
    Plan &p = *P;
    p = Plan{};
    EArgs &a = p.a;
    a = make_eargs(c);
    a.state = io.state;
    a.ncopies = io.ncopies;
    a.copies = io.copies;
    a.llpart = io.llpart;
    a.zero = io.zero;
    a.zero_len = io.zero ? io.zero_len : 0;
    a.rank_ll = io.rank_ll;
    a.done_ctr = c->d_ctr;
    const int wpb = kBlock / kWave;
    p.grid = (unsigned)c->map.nblocks;
    p.nll = c->map.nblocks;
    if (c->wide) {
        // exchange images [2][2 NP][17] (+ the backward's masked-z images [2][NP][17]) and the per-block
        // reduction scratch (estep_mfma.hpp)
        const int nt = c->NP / 16;
        p.lds = sizeof(double) * ((fwd_only ? 4 * (size_t)c->NP * 17 : 6 * (size_t)c->NP * 17) + (size_t)nt * 16 + 16);
        const Kernels kw = wide_kernels(c->NP);
        p.fn = fwd_only ? kw.score : (c->det ? kw.det_estep : kw.estep);
        p.block = (unsigned)(nt * kWave);
        if (!p.fn) return fail(HMMBW_E_UNSUPPORTED, "no wide kernel for N");
        if (!fwd_only && !c->det && c->d_wq) {  // more tiles than CUs: the work-queue form (estep_mfma.hpp)
            p.fn = wide_wq_kernel(c->NP);
            p.grid = (unsigned)c->wq_grid;
            a.wq = c->d_wq;
            a.wq_flag = c->d_wq + 2;
            a.wq_units = (int)c->map.nblocks;
            a.wq_timeout_ticks = ms_to_ticks(c, c->wq_timeout_ms);
            if (!p.fn) return fail(HMMBW_E_UNSUPPORTED, "no wide work-queue kernel for N");
        }
    } else {
        const bool lr = c->topo == HMMBW_TOPOLOGY_LEFT_TO_RIGHT;
        const bool lds_tab = c->lds_tables();
        {
            Kernels ks = lr ? (lds_tab ? pick_small_n<true, true>(c->N) : pick_small_n<true, false>(c->N))
                            : (lds_tab ? pick_small_n<false, true>(c->N) : pick_small_n<false, false>(c->N));
            p.fn = fwd_only ? ks.score : (c->det ? ks.det_estep : ks.estep);
            p.gfn = fwd_only ? ks.group_score : (c->det ? nullptr : ks.group_estep);
            if (!p.fn) return fail(HMMBW_E_UNSUPPORTED, "no kernel for N");
            const int NV = (lr ? 2 : c->N) + 3;
            const size_t tabs = c->lds_table_doubles();
            p.lds = sizeof(double) * (tabs + (size_t)wpb * c->G * NV + 8);
            // joined spread map: extra workgroup b's waves become waves 4.. of full workgroup b
            if (!fwd_only && allow_join && joined(c->map, c->topo) && ks.join_estep) {
                p.fn = ks.join_estep;
                p.grid = (unsigned)c->map.nfull;
                p.nll = c->map.nfull;
                p.block = 2 * kBlock;
                p.lds = sizeof(double) * (tabs + (size_t)(2 * wpb) * c->G * NV + 16);  // + [8 waves][2] LL pairs
                // the class-split tables and their packs
                if (split_tables_on(c->map, c->topo, c->d_sym2 != nullptr) && ks.join_estep_split) {
                    p.fn = ks.join_estep_split;
                    a.L.sym = c->d_sym2;
                    p.lds = sizeof(double) * (c->split_table_doubles() + (size_t)(2 * wpb) * c->G * NV + 16);
                }
            }
            a.split_extra = split_extra_on(c->map, c->topo, p.block == 2 * kBlock) ? 1 : 0;
            if (!lr && !fwd_only) {  // dense: the forward stores every z_t (hmmbw_device.hpp)
                if (int rc = ensure_zf(c)) return rc;
                a.ckpt = c->d_zf;
            }
        }
    }
    if (p.grid > 0 && !fwd_only && c->pend.on && c->can_merge()) {
        a.merged = 1;
        a.m = make_margs(c, c->pend);
        c->pend.on = false;
        p.flip = true;  // the launch's M-step writes the other state slot
    }
    return HMMBW_OK;
}

int plan_estep(hmmbw_ctx *c, const EstepIo &io, bool allow_join, Plan *P) {
    return plan_launch(c, false, io, allow_join, P);
}

// forward only: no state to read and no statistics to keep; the arguments carry the first buffer of each kind
int plan_score(hmmbw_ctx *c, Plan *P) {
    return plan_launch(c, true, EstepIo{nullptr, c->copies(0), c->llpart(0), nullptr, 0, nullptr, c->ncopies}, true, P);
}

// enqueue a context's own launch, with its follow-up kernels and its timing events
static int enqueue_plan(hmmbw_ctx *c, bool fwd_only, const Plan &p) {
    if (p.grid == 0) return HMMBW_OK;
    const EArgs &a = p.a;
    const bool timed = c->timing && !fwd_only && (c->timing_seq++ % c->timing) == 0;
    if (timed)
        if (int rc = c->timed.take(c->stream)) return rc;
    if (int rc = launch_lds(p.fn, p.grid, p.lds, c->stream, a, p.block)) return rc;
    if (!fwd_only) c->last_nll = p.nll;
    hipEvent_t em = nullptr;
    if (timed && (c->wide || c->det)) {
        if (c->mid_free.empty()) {
            hipEvent_t x;
            HIP_TRY(hipEventCreate(&x));
            c->mid_free.push_back(x);
        }
        em = c->mid_free.back();
        c->mid_free.pop_back();
        HIP_TRY(hipEventRecord(em, c->stream));
    }
    if ((c->wide || c->det) && !fwd_only) {
        if (c->det) {  // deterministic mode: the other statistics from the partials, in workgroup order
            const long long n = c->off_bnum();
            hipLaunchKernelGGL(k_det_reduce, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, c->d_part,
                               (long long)p.grid, n, a.copies, a.state);
        }
        if (c->wide)  // B numerator: per-symbol gather of the gamma rows (estep_mfma.hpp)
            hipLaunchKernelGGL(bnum_gather_kernel(true), dim3((unsigned)c->K), dim3(256), 0, c->stream, c->d_gam,
                               nullptr, c->d_bptr, c->NP, c->N, 1, a.copies + c->off_bnum(), a.state);
        else  // deterministic mode: fixed-order sums of the gamma rows
            hipLaunchKernelGGL(bnum_gather_kernel(false), dim3((unsigned)c->K), dim3(256), 0, c->stream, c->d_gam,
                               c->d_brows, c->d_bptr, c->G, c->N, 0, a.copies + c->off_bnum(), a.state);
        HIP_TRY(hipGetLastError());
    }
    if (p.flip) c->scur ^= 1;
    if (timed) {
        if (int rc = c->timed.done(c->stream)) return rc;
        c->mid_pending.push_back(em);  // one entry per pending pair
    }
    return HMMBW_OK;
}

int launch_estep(hmmbw_ctx *c, const EstepIo &io) {
    Plan p;
    if (int rc = plan_estep(c, io, true, &p)) return rc;
    return enqueue_plan(c, false, p);
}

int launch_score(hmmbw_ctx *c) {
    Plan p;
    if (int rc = plan_score(c, &p)) return rc;
    return enqueue_plan(c, true, p);
}

// the E-step pairs, and the mid events' share of theirs (hmmbw_timing_split)
int drain_timing(hmmbw_ctx *c) {
    for (size_t i = 0; i < c->mid_pending.size(); ++i) {
        hipEvent_t em = c->mid_pending[i];
        if (!em) continue;
        HIP_TRY(hipEventSynchronize(c->timed.pending[2 * i + 1]));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, c->timed.pending[2 * i], em));
        c->timed_main_ms += ms;
        c->timed_main_n += 1;
        c->mid_free.push_back(em);
    }
    c->mid_pending.clear();
    return c->timed.drain();
}

int check_ready(hmmbw_ctx *c, bool need_armed) {
    if (!c) return fail(HMMBW_E_INVALID, "null context");
    if (!c->has_obs) return fail(HMMBW_E_STATE, "observations not set");
    if (!c->has_params) return fail(HMMBW_E_STATE, "parameters not set");
    if (need_armed && !c->armed) return fail(HMMBW_E_STATE, "training not armed (hmmbw_reset_training)");
    return set_device(c);
}

static void resolve_topology(hmmbw_ctx *c) {
    int t = c->topo_req;
    if (c->wide) t = HMMBW_TOPOLOGY_DENSE;
    if (t == HMMBW_TOPOLOGY_AUTO || t == HMMBW_TOPOLOGY_LEFT_TO_RIGHT) {
        bool lr = true;
        for (int i = 0; i < c->N && lr; ++i)
            for (int k = 0; k < c->N; ++k)
                if (c->h_A[(size_t)i * c->N + k] != 0.0 && k != i && k != i + 1) { lr = false; break; }
        t = lr ? HMMBW_TOPOLOGY_LEFT_TO_RIGHT : HMMBW_TOPOLOGY_DENSE;
    }
    c->topo = t;
}

}  // namespace hmmbw

// the CSR input of hmmbw_set_observations; len: the sequences' lengths
static int validate_obs(const hmmbw_ctx *c, const int64_t *offsets, const int32_t *symbols, int64_t R,
                        std::vector<int> *len) {
    if (!c || !offsets || (R > 0 && !symbols && offsets[R] > 0)) return fail(HMMBW_E_INVALID, "null argument");
    if (R < 0) return fail(HMMBW_E_INVALID, "negative sequence count");
    if (offsets[0] != 0) return fail(HMMBW_E_INVALID, "offsets[0] must be 0");
    if (int rc = check_closed(c)) return rc;
    len->resize((size_t)R);
    for (int64_t r = 0; r < R; ++r) {
        const int64_t T = offsets[r + 1] - offsets[r];
        if (T < 0) return fail(HMMBW_E_INVALID, "offsets must be non-decreasing");
        if (T == 0) return fail(HMMBW_E_EMPTY_SEQUENCE, "sequence " + std::to_string(r) + " is empty");
        if (T > (1 << 28)) return fail(HMMBW_E_UNSUPPORTED, "sequence too long");
        (*len)[(size_t)r] = (int)T;
    }
    for (int64_t i = 0; i < offsets[R]; ++i)
        if (symbols[i] < 0 || symbols[i] >= c->K)
            return fail(HMMBW_E_SYMBOL_RANGE, "symbol " + std::to_string(symbols[i]) + " at position " +
                                                  std::to_string(i) + " is outside [0, M)");
    return HMMBW_OK;
}

// A/B switches of the environment, read at every hmmbw_set_observations (before the map, which depends on them)
static void read_switches(hmmbw_ctx *c) {
    MapSwitches &sw = c->sw;
    int v = 0;
    env_int("HMMBW_PRIO", &c->prio);
    if (env_int("HMMBW_SPLIT_EXTRA", &v)) sw.split_extra = v != 0;
    if (env_int("HMMBW_JOIN", &v)) sw.join = v != 0;
    if (env_int("HMMBW_JOIN_DENSE", &v)) sw.join_dense = v != 0;
    sw.xact = env_int("HMMBW_XACT", &v) ? std::max(1, std::min(kWpb, v)) : 0;
}

template <class T>
static int upload(T *dst, const std::vector<T> &v) {
    if (!v.empty()) HIP_TRY(hipMemcpy(dst, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice));
    return HMMBW_OK;
}

extern "C" {

int hmmbw_abi_version(void) { return HMMBW_ABI_VERSION; }

const char *hmmbw_last_error(void) { return g_err.c_str(); }

int hmmbw_device_count(int *out) {
    if (!out) return fail(HMMBW_E_INVALID, "null out");
    int n = 0;
    HIP_TRY(hipGetDeviceCount(&n));
    *out = n;
    return HMMBW_OK;
}

int hmmbw_ctx_create(int device, int n_states, int n_symbols, hmmbw_ctx **out) {
    if (!out) return fail(HMMBW_E_INVALID, "null out");
    *out = nullptr;
    if (n_states < 1 || n_symbols < 1) return fail(HMMBW_E_INVALID, "N and M must be >= 1");
    if (n_states > 64) return fail(HMMBW_E_UNSUPPORTED, "N > 64 states is not implemented");
    if (n_symbols > 65536) return fail(HMMBW_E_UNSUPPORTED, "M > 65536 symbols is not implemented");
    hmmbw_ctx *c = new hmmbw_ctx();
    c->device = device;
    c->N = n_states;
    c->K = n_symbols;
    c->wide = n_states > 16;
    // wide: 16-state MFMA blocks, a tile of 16 sequences per workgroup (estep_mfma.hpp)
    c->NP = c->wide ? 16 * ((n_states + 15) / 16) : 0;
    c->G = c->wide ? c->NP : (n_states <= 2 ? 2 : n_states <= 4 ? 4 : n_states <= 8 ? 8 : 16);
    c->U = c->wide ? 16 : kWave / c->G;
    int v = 0;
    if (env_int("HMMBW_LDS_LAYOUT", &v)) c->sw.lds_layout = v == 0 ? 0 : (v == 1 ? 1 : -1);
    if (env_int("HMMBW_WIDE_WQ", &v)) c->wq_mode = v == 0 ? 0 : (v == 1 ? 1 : -1);
    int rc = set_device(c);
    if (!rc) {
        int khz = 0;
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device) == hipSuccess && khz > 0)
            c->wall_khz = khz;
    }
    if (!rc) rc = dalloc(&c->d_pi, c->N);
    if (!rc) rc = dalloc(&c->d_A, (size_t)c->N * c->N);
    if (!rc) rc = dalloc(&c->d_B, (size_t)c->N * c->K);
    if (!rc) rc = dalloc(&c->d_Bt, (size_t)c->K * c->G + c->G);
    if (!rc) rc = dalloc(&c->d_out, (size_t)c->N + (size_t)c->N * c->N + (size_t)c->N * c->K);
    if (!rc) rc = dalloc(&c->d_state, 2);
    if (!rc) rc = dalloc(&c->d_hist, 2 * (size_t)kHist);
    if (!rc) rc = dalloc(&c->d_ctr, 1);
    if (!rc) {
        const hipError_t e = hipMemset(c->d_ctr, 0, sizeof(int));
        if (e != hipSuccess) rc = fail(HMMBW_E_HIP, std::string("init: ") + hipGetErrorString(e));
    }
    if (!rc) rc = realloc_stats(c);
    if (!rc) {
        init_state(c, c->d_state, 0.0, 0);
        init_state(c, c->d_state + 1, 0.0, 0);
        hipError_t e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) rc = fail(HMMBW_E_HIP, std::string("init: ") + hipGetErrorString(e));
    }
    if (rc) {
        hmmbw_ctx_destroy(c);
        return rc;
    }
    *out = c;
    return HMMBW_OK;
}

int hmmbw_ctx_destroy(hmmbw_ctx *c) {
    if (!c) return HMMBW_OK;
    (void)hipSetDevice(c->device);
    // the whole device, not just the context stream: a caller may still use a buffer the context
    // handed out (hmmbw_iterate_begin) on its own stream, and the block cache reuses freed blocks at
    // once (hipFree used to synchronise the device implicitly)
    (void)hipDeviceSynchronize();
    dfree(c->d_pi); dfree(c->d_A); dfree(c->d_B); dfree(c->d_Bt); dfree(c->d_out);
    status_free(c);
    dfree(c->d_state); dfree(c->d_hist); dfree(c->d_copies); dfree(c->d_ext); dfree(c->d_xbuf); dfree(c->d_ctr);
    comm_destroy(c);
    peer_destroy(c);
    free_obs(c);
    c->timed.destroy();
    for (auto e : c->mid_free) (void)hipEventDestroy(e);
    for (auto e : c->mid_pending)
        if (e) (void)hipEventDestroy(e);
    c->ar_timed.destroy();
    delete c;
    return HMMBW_OK;
}

int hmmbw_set_stream(hmmbw_ctx *c, void *stream) {
    if (!c) return fail(HMMBW_E_INVALID, "null context");
    if (int rc = check_closed(c)) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (s != c->stream) {
        // later frees synchronise only the NEW stream: the block cache must not hand a buffer that work
        // queued on the old one still uses to another context
        if (int rc = set_device(c)) return rc;
        if (c->stream) HIP_TRY(hipStreamSynchronize(c->stream));
        else HIP_TRY(hipDeviceSynchronize());
    }
    c->stream = s;
    return HMMBW_OK;
}

int hmmbw_set_rank(hmmbw_ctx *c, int rank, int world) {
    if (!c) return fail(HMMBW_E_INVALID, "null context");
    if (int rc = check_closed(c)) return rc;
    if (world < 1 || rank < 0 || rank >= world) return fail(HMMBW_E_INVALID, "bad rank/world");
    if (int rc = set_device(c)) return rc;
    if (int rc = flush_mstep(c)) return rc;
    if (c->rank != rank || c->world != world) peer_detach(c);  // the regions are sized for the old world
    c->rank = rank;
    c->world = world;
    return realloc_stats(c);
}

int hmmbw_set_topology(hmmbw_ctx *c, int topology) {
    if (!c) return fail(HMMBW_E_INVALID, "null context");
    if (topology < HMMBW_TOPOLOGY_AUTO || topology > HMMBW_TOPOLOGY_LEFT_TO_RIGHT)
        return fail(HMMBW_E_INVALID, "bad topology");
    c->topo_req = topology;
    if (c->has_params) {
        resolve_topology(c);
        if (topology == HMMBW_TOPOLOGY_LEFT_TO_RIGHT && c->topo != HMMBW_TOPOLOGY_LEFT_TO_RIGHT)
            return fail(HMMBW_E_INVALID, "A is not left-to-right (nonzero a_ij with j not in {i, i+1})");
    }
    return HMMBW_OK;
}

int hmmbw_get_topology(const hmmbw_ctx *c, int *out) {
    if (!c || !out) return fail(HMMBW_E_INVALID, "null argument");
    *out = c->topo;
    return HMMBW_OK;
}

// validate, lay out, plan the map, allocate, upload, store
int hmmbw_set_observations(hmmbw_ctx *c, const int64_t *offsets, const int32_t *symbols, int64_t R) {
    std::vector<int> len;
    if (int rc = validate_obs(c, offsets, symbols, R, &len)) return rc;
    if (int rc = set_device(c)) return rc;
    if (int rc = flush_mstep(c)) return rc;      // it reads this layout's log-likelihood pairs
    HIP_TRY(hipStreamSynchronize(c->stream));  // buffers may still be in use by enqueued work
    const ObsLayout L = plan_layout(len, c->U, c->wide, c->NP);
    const int64_t total = offsets[R];
    // packs hold LDS byte offsets of the emission record rows when the tables live in LDS (< 64 KiB,
    // so they fit uint16), symbol ids otherwise
    const long long row_bytes = (long long)c->G * 16;  // 16-B table entries
    std::vector<uint16_t> hsym = fill_packs(L, offsets, symbols, c->lds_tables() ? row_bytes : 1);
    free_obs(c);

    read_switches(c);
    MapInputs in;
    in.nwaves = L.nwaves;
    in.steps = L.symtot / L.U;
    (void)hipDeviceGetAttribute(&in.ncu, hipDeviceAttributeMultiprocessorCount, c->device);
    in.wide = c->wide;
    in.det = c->det;
    in.lds_tables = c->lds_tables();
    in.split_tables = c->split_tables();
    in.topo_req = c->topo_req;
    in.sw = c->sw;
    const LaunchMap m = plan_map(in);

    // symbol -> gamma rows index of k_bnum_gather (wide path, deterministic mode)
    std::vector<long long> bptr;
    std::vector<unsigned> brows;
    if (c->wide) {
        // position -> its row in symbol order (positions of one symbol in tile-row order): the E-step writes
        // the gamma row of tile row wck / NP + t * 16 + u there (brows, indexed by tile row), so symbol k's
        // rows are [bptr[k], bptr[k+1]) and k_bnum_gather streams them
        if (L.cktot / c->NP >= (1LL << 32)) return fail(HMMBW_E_UNSUPPORTED, "too many positions for the wide path");
        // rows of padding slots (a tile's slots past the last sequence: full-tile code paths store their
        // exact-zero gamma rows unmasked) all go to one scratch row past the real ones
        brows.assign((size_t)std::max(L.cktot / c->NP, 1LL), (unsigned)total);
        build_gather_index(L, offsets, symbols, c->K, true, [&](long long w, int u, int t) {
            return L.ckoff[(size_t)w] / c->NP + (long long)t * L.U + u;
        }, bptr, brows);
    } else if (c->det) {  // deterministic mode: symbol -> pack positions (gamma row = pack index), stable
        if (L.symtot >= (1LL << 32)) return fail(HMMBW_E_UNSUPPORTED, "too many positions for the deterministic mode");
        brows.resize((size_t)std::max<int64_t>(total, 1));
        build_gather_index(L, offsets, symbols, c->K, false, [&](long long w, int u, int t) {
            return pack_pos(L.symoff[(size_t)w], L.U, u, t);
        }, bptr, brows);
    }

    const size_t nw = (size_t)L.nwaves, nb1 = (size_t)std::max(m.nblocks, 1LL);
    int rc = dalloc(&c->d_sym, hsym.size());
    if (!rc && m.sym2) rc = dalloc(&c->d_sym2, hsym.size());
    if (!rc) rc = dalloc(&c->d_wsym, nw);
    if (!rc) rc = dalloc(&c->d_wckoff, nw);
    if (!rc) rc = dalloc(&c->d_wspoff, nw);
    if (!rc) rc = dalloc(&c->d_wT, nw);
    if (!rc) rc = dalloc(&c->d_wfull, nw);
    if (!rc) rc = dalloc(&c->d_slen, L.slot_len.size());
    if (!rc) rc = dalloc(&c->d_sseq, L.slot_seq.size());
    if (!rc) rc = dalloc(&c->d_ck, (size_t)std::max(L.cktot, 1LL));
    c->cktot = L.cktot;
    const size_t nsp = (size_t)std::max(L.sptot, 1LL);
    if (!rc) rc = c->wide ? dalloc(&c->d_ebuf, nsp) : dalloc(&c->d_sp, nsp);
    if (c->wide || c->det) {  // gamma rows: per position (wide), per pack entry (deterministic mode)
        if (!rc) rc = dalloc(&c->d_gam, c->wide ? (size_t)(total + 1) * c->NP : hsym.size() * c->G);
        if (!rc) rc = dalloc(&c->d_bptr, bptr.size());
        if (!rc) rc = dalloc(&c->d_brows, brows.size());
        if (!rc && c->det) rc = dalloc(&c->d_part, nb1 * (size_t)c->off_bnum());
    }
    if (!rc) rc = dalloc(&c->d_logp, (size_t)std::max<int64_t>(R, 1));
    if (!rc) rc = dalloc(&c->d_llpart, 4 * nb1);

    if (!rc) rc = upload(c->d_sym, hsym);
    if (!rc && m.sym2) {
        to_split_packs(hsym, row_bytes, c->G);
        rc = upload(c->d_sym2, hsym);
    }
    if (!rc && (c->wide || c->det)) rc = upload(c->d_bptr, bptr);
    if (!rc && (c->wide || c->det)) rc = upload(c->d_brows, brows);
    if (!rc) rc = upload(c->d_wsym, L.symoff);
    if (!rc) rc = upload(c->d_wckoff, L.ckoff);
    if (!rc) rc = upload(c->d_wspoff, L.spoff);
    if (!rc) rc = upload(c->d_wT, L.wave_T);
    if (!rc) rc = upload(c->d_wfull, L.wave_full);
    if (!rc) rc = upload(c->d_slen, L.slot_len);
    if (!rc) rc = upload(c->d_sseq, L.slot_seq);
    if (!rc) rc = upload(c->d_logp, std::vector<double>((size_t)std::max<int64_t>(R, 1), -INFINITY));
    if (!rc) rc = upload(c->d_llpart, std::vector<double>(4 * nb1, 0.0));
    if (rc) return rc;

    c->R = R;
    c->nwaves = L.nwaves;
    c->h_slen = L.slot_len;
    c->h_sseq = L.slot_seq;
    c->map = m;
    c->has_obs = true;
    if (int rc2 = ensure_wq(c)) return rc2;
    return ensure_zf(c);
}

int hmmbw_set_option(hmmbw_ctx *c, int key, int64_t value) {
    if (!c) return fail(HMMBW_E_INVALID, "null context");
    if (int rc = check_closed(c)) return rc;
    if (key == HMMBW_OPT_SAFE_SCALING) {
        c->force_safe = value != 0;
        return HMMBW_OK;
    }
    if (key == HMMBW_OPT_STAT_COPIES) {
        if (value < 1 || value > 1024) return fail(HMMBW_E_INVALID, "statistics copies must be in [1, 1024]");
        if (int rc = set_device(c)) return rc;
        if (int rc = flush_mstep(c)) return rc;
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->ncopies = (int)value;
        return realloc_stats(c);
    }
    if (key == HMMBW_OPT_DETERMINISTIC) {
        if (c->has_obs) return fail(HMMBW_E_STATE, "set the deterministic mode before hmmbw_set_observations");
        if (value != 0 && !c->wide && !c->lds_tables())
            return fail(HMMBW_E_UNSUPPORTED, "deterministic mode needs the LDS emission tables (N <= 16) or the wide path");
        c->det = value != 0;
        return HMMBW_OK;
    }
    if (key == HMMBW_OPT_LDS_LAYOUT) {
        if (value < -1 || value > 1)
            return fail(HMMBW_E_INVALID, "HMMBW_OPT_LDS_LAYOUT: -1 (auto), 0 (row tables) or 1 (class-split)");
        if (c->has_obs) return fail(HMMBW_E_STATE, "set the LDS table layout before hmmbw_set_observations");
        c->sw.lds_layout = (int)value;
        return HMMBW_OK;
    }
    if (key == HMMBW_OPT_MERGE_MSTEP) {
        if (int rc = set_device(c)) return rc;
        if (int rc = flush_mstep(c)) return rc;
        c->merge_mstep = value != 0;
        return HMMBW_OK;
    }
    if (key == HMMBW_OPT_ALLREDUCE) {
        if (value != HMMBW_ALLREDUCE_RCCL && value != HMMBW_ALLREDUCE_PEER)
            return fail(HMMBW_E_INVALID, "HMMBW_OPT_ALLREDUCE: 0 (RCCL / caller) or 1 (peer)");
        c->ar_kind = (int)value;
        return HMMBW_OK;
    }
    if (key == HMMBW_OPT_PEER_TIMEOUT_MS) {
        if (value < 1) return fail(HMMBW_E_INVALID, "peer timeout must be >= 1 ms");
        c->peer_timeout_ms = value;
        return HMMBW_OK;
    }
    if (key == HMMBW_OPT_LIVE_STATUS) {
        return live_status_set(c, value != 0);
    }
    if (key == HMMBW_OPT_WQ_TIMEOUT_MS) {
        if (value < 0) return fail(HMMBW_E_INVALID, "work-queue timeout must be >= 0 ms");
        c->wq_timeout_ms = value;
        return HMMBW_OK;
    }
    if (key == HMMBW_OPT_WIDE_WQ) {
        if (value < -1 || value > 1) return fail(HMMBW_E_INVALID, "HMMBW_OPT_WIDE_WQ: -1 (auto), 0 (off) or 1 (on)");
        if (int rc = set_device(c)) return rc;
        c->wq_mode = (int)value;
        return ensure_wq(c);
    }
    if (key == HMMBW_OPT_ABLATE) {  // diagnostics: results are wrong while set
        c->ablate = (int)value;
        return HMMBW_OK;
    }
    return fail(HMMBW_E_INVALID, "unknown option " + std::to_string(key));
}

int hmmbw_get_option(const hmmbw_ctx *c, int key, int64_t *value) {
    if (!c || !value) return fail(HMMBW_E_INVALID, "null argument");
    switch (key) {
        case HMMBW_OPT_SAFE_SCALING: *value = c->force_safe; return HMMBW_OK;
        case HMMBW_OPT_ABLATE: *value = c->ablate; return HMMBW_OK;
        case HMMBW_OPT_STAT_COPIES: *value = c->ncopies; return HMMBW_OK;
        case HMMBW_OPT_MERGE_MSTEP: *value = c->merge_mstep ? 1 : 0; return HMMBW_OK;
        case HMMBW_OPT_DETERMINISTIC: *value = c->det ? 1 : 0; return HMMBW_OK;
        case HMMBW_OPT_ALLREDUCE: *value = c->ar_kind; return HMMBW_OK;
        case HMMBW_OPT_PEER_TIMEOUT_MS: *value = c->peer_timeout_ms; return HMMBW_OK;
        case HMMBW_OPT_LIVE_STATUS: *value = c->h_live ? 1 : 0; return HMMBW_OK;
        case HMMBW_OPT_WQ_TIMEOUT_MS: *value = c->wq_timeout_ms; return HMMBW_OK;
        case HMMBW_OPT_WIDE_WQ: *value = c->wq_mode; return HMMBW_OK;
        case HMMBW_OPT_LDS_LAYOUT: *value = c->sw.lds_layout; return HMMBW_OK;
        case HMMBW_INFO_LDS_LAYOUT:
            *value = c->has_obs && split_tables_on(c->map, c->topo, c->d_sym2 != nullptr) ? 1 : 0;
            return HMMBW_OK;
        case HMMBW_INFO_WIDE_WQ_ACTIVE: *value = c->d_wq ? 1 : 0; return HMMBW_OK;
        case HMMBW_INFO_WAVES: *value = c->wide ? c->map.nblocks * (c->NP / 16) : c->nwaves; return HMMBW_OK;
        case HMMBW_INFO_WORKGROUPS: *value = c->d_wq ? c->wq_grid : c->map.nblocks; return HMMBW_OK;
        case HMMBW_INFO_WAVES_PER_WORKGROUP: *value = c->wide ? c->NP / 16 : kBlock / kWave; return HMMBW_OK;
        case HMMBW_INFO_FULL_WORKGROUPS: *value = c->wide ? c->map.nblocks : std::min(c->map.nfull, c->map.nblocks); return HMMBW_OK;
        case HMMBW_INFO_EXTRA_WAVES: *value = c->wide ? 0 : c->map.xact; return HMMBW_OK;
        case HMMBW_INFO_JOINED: *value = c->has_obs && joined(c->map, c->topo) ? 1 : 0; return HMMBW_OK;
        case HMMBW_INFO_SPLIT_EXTRA:
            *value = c->has_obs && split_extra_on(c->map, c->topo, joined(c->map, c->topo)) ? 1 : 0;
            return HMMBW_OK;
        case HMMBW_INFO_PEER_CHUNKS:
        case HMMBW_INFO_PEER_SUM_PTR:
        case HMMBW_INFO_PEER_REGIONS_VALIDATED:
        case HMMBW_INFO_PEER_REGIONS_REJECTED: return peer_info(c, key, value);
        default: return fail(HMMBW_E_INVALID, "unknown option " + std::to_string(key));
    }
}

int hmmbw_set_params(hmmbw_ctx *c, const double *pi, const double *A, const double *B) {
    if (!c || !pi || !A || !B) return fail(HMMBW_E_INVALID, "null argument");
    if (int rc = check_closed(c)) return rc;
    if (int rc = set_device(c)) return rc;
    if (int rc = flush_mstep(c)) return rc;  // it would overwrite the new parameters later
    HIP_TRY(hipStreamSynchronize(c->stream));
    const int N = c->N, K = c->K, G = c->G;
    // safe_log semantics (hmm_training.py:46-54): x <= 0 (and NaN) is a zero probability
    auto clean = [](double x) { return x > 0.0 ? x : 0.0; };
    std::vector<double> hpi(N), hA((size_t)N * N), hB((size_t)N * K), hBt((size_t)K * G + G, 0.0);
    for (int i = 0; i < N; ++i) hpi[i] = clean(pi[i]);
    for (size_t i = 0; i < hA.size(); ++i) hA[i] = clean(A[i]);
    for (int jj = 0; jj < N; ++jj)
        for (int k = 0; k < K; ++k) {
            const double v = clean(B[(size_t)jj * K + k]);
            hB[(size_t)jj * K + k] = v;
            hBt[(size_t)k * G + (c->wide ? bt_col(jj) : jj)] = v;
        }
    HIP_TRY(hipMemcpy(c->d_pi, hpi.data(), sizeof(double) * N, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->d_A, hA.data(), sizeof(double) * hA.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->d_B, hB.data(), sizeof(double) * hB.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->d_Bt, hBt.data(), sizeof(double) * hBt.size(), hipMemcpyHostToDevice));
    c->h_A = hA;
    c->has_params = true;
    resolve_topology(c);
    return ensure_zf(c);
}

int hmmbw_stats_len(const hmmbw_ctx *c, int64_t *n) {
    if (!c || !n) return fail(HMMBW_E_INVALID, "null argument");
    *n = c->stats_len();
    return HMMBW_OK;
}

int hmmbw_get_params(hmmbw_ctx *c, double *pi, double *A, double *B, int normalise) {
    if (!c || !pi || !A || !B) return fail(HMMBW_E_INVALID, "null argument");
    if (!c->has_params) return fail(HMMBW_E_STATE, "parameters not set");
    if (int rc = set_device(c)) return rc;
    if (int rc = flush_mstep(c)) return rc;
    const size_t N = c->N, K = c->K;
    if (normalise) {
        hipLaunchKernelGGL(k_finalise, dim3(1), dim3(64), 0, c->stream, c->d_pi, c->d_A, c->d_B, c->N, c->K, c->d_out);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(pi, c->d_out, sizeof(double) * N, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(A, c->d_out + N, sizeof(double) * N * N, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(B, c->d_out + N + N * N, sizeof(double) * N * K, hipMemcpyDeviceToHost, c->stream));
    } else {
        HIP_TRY(hipMemcpyAsync(pi, c->d_pi, sizeof(double) * N, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(A, c->d_A, sizeof(double) * N * N, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(B, c->d_B, sizeof(double) * N * K, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return HMMBW_OK;
}

int hmmbw_get_loglik(hmmbw_ctx *c, double *out) {
    if (!c || !out) return fail(HMMBW_E_INVALID, "null argument");
    if (!c->has_obs) return fail(HMMBW_E_STATE, "observations not set");
    if (int rc = set_device(c)) return rc;
    if (c->R > 0)
        HIP_TRY(hipMemcpyAsync(out, c->d_logp, sizeof(double) * c->R, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return HMMBW_OK;
}

int hmmbw_score(hmmbw_ctx *c, double *out) {
    if (int rc = check_ready(c, false)) return rc;
    if (!out) return fail(HMMBW_E_INVALID, "null argument");
    if (int rc = check_closed(c)) return rc;
    if (int rc = flush_mstep(c)) return rc;
    if (int rc = launch_score(c)) return rc;
    return hmmbw_get_loglik(c, out);
}

int hmmbw_timing(hmmbw_ctx *c, int enable, double *total_ms, int64_t *count) {
    if (!c) return fail(HMMBW_E_INVALID, "null context");
    if (int rc = set_device(c)) return rc;
    if (int rc = drain_timing(c)) return rc;
    if (total_ms) *total_ms = c->timed.ms;
    if (count) *count = c->timed.n;
    if (enable >= 0) {
        c->timing = enable;
        c->timing_seq = 0;
        c->timed.ms = 0.0;
        c->timed.n = 0;
        c->timed_main_ms = 0.0;
        c->timed_main_n = 0;
    }
    return HMMBW_OK;
}

int hmmbw_timing_split(hmmbw_ctx *c, double *main_ms, int64_t *count) {
    if (!c) return fail(HMMBW_E_INVALID, "null context");
    if (int rc = set_device(c)) return rc;
    if (int rc = drain_timing(c)) return rc;
    if (main_ms) *main_ms = c->timed_main_ms;
    if (count) *count = c->timed_main_n;
    return HMMBW_OK;
}

int hmmbw_vq_encode(void *stream, const double *frames, int64_t n_frames, int frame_stride, int first_dim, int dims,
                    const double *centroids, int n_centroids, int32_t *symbols, double *distances) {
    if (n_frames < 0) return fail(HMMBW_E_INVALID, "negative frame count");
    if (n_frames == 0) return HMMBW_OK;
    if (!frames || !centroids || !symbols) return fail(HMMBW_E_INVALID, "null argument");
    if (dims < 1 || dims > 64 || first_dim < 0 || frame_stride < first_dim + dims)
        return fail(HMMBW_E_INVALID, "need 1 <= dims <= 64 and first_dim + dims <= frame_stride");
    if (n_centroids < 1) return fail(HMMBW_E_INVALID, "empty codebook");
    if ((long long)n_centroids * dims > 20480) return fail(HMMBW_E_UNSUPPORTED, "codebook larger than 160 KiB of LDS");
    if (n_frames > (1LL << 40)) return fail(HMMBW_E_UNSUPPORTED, "too many frames");
    hipError_t e = launch_vq(reinterpret_cast<hipStream_t>(stream), frames, n_frames, frame_stride, first_dim, dims,
                             centroids, n_centroids, symbols, distances);
    if (e != hipSuccess) return fail(HMMBW_E_HIP, std::string("vq launch: ") + hipGetErrorString(e));
    return HMMBW_OK;
}

}  // extern "C"
