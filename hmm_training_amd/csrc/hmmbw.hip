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
//   k_reduce_local  (multi-rank) sum the statistics copies into the all-reduce buffer + the rank's
//                   (max, sum exp) pair of log P_r.
//   k_det_reduce    (deterministic mode) sum the per-workgroup partial statistics in workgroup order.
//   k_mstep / k_mstep_staged  one workgroup: L, M-step, convergence record, zero the statistics
//                   (staged: all statistics gathered into LDS with one batch of loads).
//   k_mstep_grid    large N x K (wide path): B re-estimated by the whole grid, the rest by workgroup 0.
//                   (Their bodies: mstep.hpp; merged into the next E-step launch: merged_mstep.)
//   k_snapshot      the state and the iteration records into pinned host memory (hmmbw_status_post).
//   k_finalise  the reference's return-path normalisation (:524-541).
//   k_init_state    the convergence state of a new run.
//   (peer.hip, viterbi.hip and vq.hip hold their own kernels.)
//
// Host units (host.hpp): this one holds the context's life cycle, observations, options and parameters,
// the launch planner, hmmbw_estep / _mstep / _iterate*, status, scoring and timing; alloc.hip the block
// cache and the allocation ledger, peer.hip the peer all-reduce (kernels included), comm.hip the RCCL
// communicator, group.hip the grouped launches, viterbi.hip the Viterbi decoder.
#include <atomic>
#include <map>
#include <mutex>

#include "host.hpp"
#include "mstep.hpp"

namespace hmmbw {

// Multi-rank: sum this rank's statistics copies into the caller's buffer (for the all-reduce),
// zero the copies, and write the rank's (max, sum exp) pair of log P into its slot.
__global__ void __launch_bounds__(256) k_reduce_local(double *copies, int ncopies, long long copy_len,
                                                      const double *llpart, long long nblocks, double *stats,
                                                      long long off_ll, int world, int rank,
                                                      const IterState *state) {
    __shared__ double sh[16];
    if (state->done) return;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < copy_len;
         idx += (long long)gridDim.x * blockDim.x) {
        double v = 0.0;
        for (int c = 0; c < ncopies; ++c) {
            v += copies[c * copy_len + idx];
            copies[c * copy_len + idx] = 0.0;
        }
        stats[idx] = v;
    }
    if (blockIdx.x == 0) {
        double m, s;
        combine_ll_pairs(llpart, nblocks, sh, &m, &s);
        if (threadIdx.x < 2 * world) stats[off_ll + threadIdx.x] = 0.0;
        __syncthreads();
        if (threadIdx.x == 0) {
            stats[off_ll + 2 * rank] = (s > 0.0) ? m : 0.0;
            stats[off_ll + 2 * rank + 1] = s;
        }
    }
}

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

__global__ void __launch_bounds__(256) k_mstep(MArgs m) {
    if (carry_if_done(m)) return;
    mstep_block(m);
}

__global__ void __launch_bounds__(256) k_mstep_grid(MArgs m) {
    if (carry_if_done(m)) return;
    mstep_grid(m);
}

// single-rank M-step with the statistics staged in dynamic LDS (copy_len doubles)
__global__ void __launch_bounds__(256) k_mstep_staged(MArgs m) {
    extern __shared__ double sSt[];
    if (carry_if_done(m)) return;
    mstep_staged(m, sSt);
}

// Status snapshot for hmmbw_status_post: the state record and the iteration records [first, iteration)
// written straight into pinned host memory (one small launch on the stream instead of DMA copies).
__global__ void __launch_bounds__(256) k_snapshot(const IterState *st, const double *hist, long long first,
                                                   IterState *hst, double *hrec) {
    const IterState s = *st;
    const long long n = min(max(s.iteration - first, 0LL), (long long)kHist);
    for (long long i = threadIdx.x; i < n; i += blockDim.x) {
        const long long k = (first + i) % kHist;
        hrec[2 * i] = hist[2 * k];
        hrec[2 * i + 1] = hist[2 * k + 1];
    }
    if (threadIdx.x == 0) *hst = s;
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

__global__ void k_init_state(IterState *st, double eps, long long max_it) {
    st->prev_L = -INFINITY;
    st->last_L = -INFINITY;
    st->last_diff = INFINITY;
    st->epsilon = eps;
    st->iteration = 0;
    st->max_iterations = max_it;
    st->done = max_it <= 0 ? 1 : 0;
    st->converged = 0;
    st->error = 0;
    st->error_src = 0;
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
    a.copies = c->copies(0);
    a.copy_len = c->copy_len();
    a.ncopies = c->ncopies;
    a.logp = c->d_logp;
    a.llpart = c->llpart(0);
    a.force_safe = c->force_safe;
    a.ablate = c->ablate;
    a.state = c->state();
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

// M-step arguments for the pending statistics: this context's copies (single rank) or the caller's
// all-reduced buffer with one (max, sum exp) pair per rank
static MArgs make_margs(hmmbw_ctx *c, const hmmbw_ctx::Pending &p) {
    MArgs m{};
    m.src = p.src;
    m.zero_ll = p.local ? nullptr : const_cast<double *>(p.ll);
    m.nsrc = p.nsrc;
    m.copy_len = c->copy_len();
    m.pi = c->d_pi;
    m.A = c->d_A;
    m.B = c->d_B;
    m.Bt = c->d_Bt;
    m.llpart = p.ll;
    m.nblocks = p.nll;
    m.R_global = p.R;
    m.state = c->state();
    m.state_out = c->d_state + (c->scur ^ 1);
    m.hist = c->d_hist;
    m.N = c->N;
    m.K = c->K;
    m.G = c->G;
    m.world = c->world;
    m.local_lse = p.local ? 1 : 0;
    m.bt_perm = c->wide ? 1 : 0;
    m.off_S = c->off_S();
    m.off_gex = c->off_gex();
    m.off_gall = c->off_gall();
    m.live = c->h_live;
    m.live_epoch = c->live_epoch;
    m.off_bnum = c->off_bnum();
    m.off_ll = c->off_ll();
    return m;
}

// run the pending M-step as its own one-workgroup kernel
int flush_mstep(hmmbw_ctx *c) {
    if (!c->pend.on) return HMMBW_OK;
    c->pend.on = false;
    if (c->ablate & 4) return HMMBW_OK;  // diagnostics (HMMBW_OPT_ABLATE bit 2): no separate M-step kernel
    const MArgs m = make_margs(c, c->pend);
    const size_t staged = sizeof(double) * (size_t)c->copy_len();
    const long long nb = (long long)c->N * c->K;
    if (m.local_lse && staged <= 64 * 1024 && c->N * c->N <= 256)
        hipLaunchKernelGGL(k_mstep_staged, dim3(1), dim3(256), staged, c->stream, m);
    else if (nb > 8192)  // large B: the whole grid re-estimates it (one workgroup took 150 us at 64 x 1024)
        hipLaunchKernelGGL(k_mstep_grid, dim3((unsigned)std::min<long long>((nb + 1023) / 1024, 256)), dim3(256), 0,
                           c->stream, m);
    else
        hipLaunchKernelGGL(k_mstep, dim3(1), dim3(256), 0, c->stream, m);
    HIP_TRY(hipGetLastError());
    c->scur ^= 1;
    return HMMBW_OK;
}

// The pending M-step reads this context's statistics of E-step launch e (single rank); nll: the
// log-likelihood pairs that launch wrote.
void pend_local(hmmbw_ctx *c, long long e, long long nll) {
    hmmbw_ctx::Pending &p = c->pend;
    p.on = true;
    p.local = true;
    p.src = c->copies(e);
    p.nsrc = c->det ? 1 : c->ncopies;
    p.ll = c->llpart(e);
    p.nll = nll;
    p.ext = nullptr;
    p.R = c->R;
}

// The pending M-step reads an all-reduced buffer: nsrc statistics copies, then one (max, sum exp) pair per
// rank (copy_len() == off_ll(), so the packed statistics of hmmbw_mstep are the nsrc = 1 case).
// Deferred into the next E-step launch when that can merge it; queries flush it.
static int pend_reduced(hmmbw_ctx *c, double *src, int nsrc, long long R) {
    hmmbw_ctx::Pending &p = c->pend;
    p.on = true;
    p.local = false;
    p.src = src;
    p.nsrc = nsrc;
    p.ll = src + (long long)nsrc * c->copy_len();
    p.nll = c->world;
    p.ext = src;
    p.R = R;
    return c->can_merge() ? HMMBW_OK : flush_mstep(c);
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

// E-step launch e accumulates into copies and llpart; it clears `zero` (zero_len doubles) and, when
// `merge` is set, first runs the pending M-step in its prologue (which consumes c->pend).
int plan_estep(hmmbw_ctx *c, bool fwd_only, const IterState *state, double *copies, double *llpart, double *zero,
               long long zero_len, bool merge, Plan *P, double *rank_ll, int ncopies, bool allow_join) {
    Plan &p = *P;
    p = Plan{};
    EArgs &a = p.a;
    a = make_eargs(c);
    a.state = state;
    if (ncopies > 0) a.ncopies = ncopies;
    if (copies) a.copies = copies;
    if (llpart) a.llpart = llpart;
    a.zero = zero;
    a.zero_len = zero ? zero_len : 0;
    a.rank_ll = rank_ll;
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
    if (p.grid > 0 && merge && !fwd_only && c->pend.on && c->can_merge()) {
        a.merged = 1;
        a.m = make_margs(c, c->pend);
        c->pend.on = false;
        p.flip = true;  // the launch's M-step writes the other state slot
    }
    return HMMBW_OK;
}

int launch_estep(hmmbw_ctx *c, bool fwd_only, const IterState *state, double *copies, double *llpart, double *zero,
                 long long zero_len, bool merge, double *rank_ll, int ncopies) {
    Plan p;
    if (int rc = plan_estep(c, fwd_only, state, copies, llpart, zero, zero_len, merge, &p, rank_ll, ncopies)) return rc;
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

// the E-step pairs, and the mid events' share of theirs (hmmbw_timing_split)
static int drain_timing(hmmbw_ctx *c) {
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

// message of a device-side stop (IterState::error, set with done by a bounded wait that expired)
static std::string device_error(const IterState &h) {
    if (h.error_src == kErrWorkQueue)
        return "EM stopped on a device-side failure: a wide work-queue backward sweep did not see its tile's "
               "forward sweep finish within HMMBW_OPT_WQ_TIMEOUT_MS";
    return "EM stopped on a device-side failure: a rank did not deliver its statistics to the peer all-reduce "
           "within HMMBW_OPT_PEER_TIMEOUT_MS";
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
        hipLaunchKernelGGL(k_init_state, dim3(1), dim3(1), 0, c->stream, c->d_state, 0.0, 0LL);
        hipLaunchKernelGGL(k_init_state, dim3(1), dim3(1), 0, c->stream, c->d_state + 1, 0.0, 0LL);
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
    for (auto &sn : c->snaps) {
        if (sn.ev) (void)hipEventDestroy(sn.ev);
        cached_free(sn.st, kPinnedBlock);
        cached_free(sn.hist, kPinnedBlock);
    }
    dfree(c->d_state); dfree(c->d_hist); dfree(c->d_copies); dfree(c->d_ext); dfree(c->d_xbuf); dfree(c->d_ctr);
    cached_free(c->h_live, kPinnedBlock);
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
        if (int rc = set_device(c)) return rc;
        HIP_TRY(hipStreamSynchronize(c->stream));  // no launch of the old setting is still in flight
        if (value == 0) {
            cached_free(c->h_live, kPinnedBlock);
            c->h_live = nullptr;
            return HMMBW_OK;
        }
        if (c->h_live) return HMMBW_OK;
        HIP_TRY(cached_alloc(reinterpret_cast<void **>(&c->h_live), sizeof(LiveBlock), kPinnedBlock));
        // seed the mirror with the state as it stands (records of a pending M-step follow when it runs)
        IterState h{};
        HIP_TRY(hipMemcpy(&h, c->state(), sizeof(IterState), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(c->h_live->hist, c->d_hist, sizeof(double) * 2 * (size_t)kHist, hipMemcpyDeviceToHost));
        c->h_live->slot[h.iteration & 1] = h;
        std::atomic_thread_fence(std::memory_order_release);
        reinterpret_cast<volatile unsigned long long &>(c->h_live->pub) =
            ((unsigned long long)c->live_epoch << 32) | (unsigned long long)(unsigned)h.iteration;
        return HMMBW_OK;
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

int hmmbw_reset_training(hmmbw_ctx *c, double epsilon, int64_t max_iterations) {
    if (!c) return fail(HMMBW_E_INVALID, "null context");
    if (int rc = check_closed(c)) return rc;
    if (int rc = set_device(c)) return rc;
    if (int rc = flush_mstep(c)) return rc;
    hipLaunchKernelGGL(k_init_state, dim3(1), dim3(1), 0, c->stream, c->state(), epsilon, (long long)max_iterations);
    HIP_TRY(hipGetLastError());
    ++c->live_epoch;  // the mirror's records of the previous run no longer count (hmmbw_status_live_wait)
    HIP_TRY(hipMemsetAsync(c->d_copies, 0, sizeof(double) * 3 * c->ncopies * c->copy_len(), c->stream));
    if (c->d_xbuf) HIP_TRY(hipMemsetAsync(c->d_xbuf, 0, sizeof(double) * 3 * (size_t)c->xlen, c->stream));
    // the work queue's counters and flags: a run stopped by a work-queue timeout leaves them armed (the
    // workgroups that start after the stop return at once and never reach the re-arm)
    if (c->d_wq) HIP_TRY(hipMemsetAsync(c->d_wq, 0, sizeof(unsigned) * ((size_t)c->map.nblocks + 2), c->stream));
    // the fused multi-rank completion counter: workgroups that start after a device-side stop return
    // before counting their log-likelihood pair, so a stopped launch leaves it part-way; the next run's
    // last-workgroup fold must start from zero
    HIP_TRY(hipMemsetAsync(c->d_ctr, 0, sizeof(int), c->stream));
    c->e_count = 0;
    c->armed = true;
    return HMMBW_OK;
}

int hmmbw_stats_len(const hmmbw_ctx *c, int64_t *n) {
    if (!c || !n) return fail(HMMBW_E_INVALID, "null argument");
    *n = c->stats_len();
    return HMMBW_OK;
}

int hmmbw_estep(hmmbw_ctx *c, double *stats_dev) {
    if (int rc = check_ready(c, true)) return rc;
    if (int rc = check_closed(c)) return rc;
    if (!stats_dev) return fail(HMMBW_E_INVALID, "null stats buffer");
    if (c->pend.on && !c->can_merge())
        if (int rc = flush_mstep(c)) return rc;
    const long long e = c->e_count++;
    double *llp = c->llpart(e);
    // multi-rank: one copy set, cleared by k_reduce_local
    if (int rc = launch_estep(c, false, c->state(), c->copies(0), llp, nullptr, 0, true)) return rc;
    const long long n = c->copy_len();
    const unsigned grid = (unsigned)std::min<long long>((n + 255) / 256, 64);
    hipLaunchKernelGGL(k_reduce_local, dim3(grid), dim3(256), 0, c->stream, c->copies(0), c->det ? 1 : c->ncopies, n, llp,
                       c->last_nll, stats_dev, c->off_ll(), c->world, c->rank, c->state());
    HIP_TRY(hipGetLastError());
    return HMMBW_OK;
}

int hmmbw_mstep(hmmbw_ctx *c, double *stats_dev, int64_t n_seq_global) {
    if (int rc = check_ready(c, true)) return rc;
    if (int rc = check_closed(c)) return rc;
    if (!stats_dev) return fail(HMMBW_E_INVALID, "null stats buffer");
    if (int rc = flush_mstep(c)) return rc;
    return pend_reduced(c, stats_dev, 1, n_seq_global);
}

// First half of one multi-rank EM iteration: this rank's E-step, leaving in *buf (*len doubles, device
// memory of the context) the partial statistics that every rank must all-reduce (sum) before mr_end.
// Small kernels: fused (the E-step accumulates straight into a triple-buffered all-reduce buffer and
// its last workgroup writes the rank's (max, sum exp) pair; no k_reduce_local launch).  Wide and
// deterministic paths: hmmbw_estep + k_reduce_local into d_ext.  The layout is rank-independent: every
// rank all-reduces the same buffer shape, also a rank whose shard is empty.
static int mr_begin(hmmbw_ctx *c, long long n_seq_global, double **buf, long long *len) {
    if (int rc = check_closed(c)) return rc;
    const bool fused = !c->det;  // the small and the wide E-step accumulate into the all-reduce buffer
    if (fused) {
        // rounded to 256 B so all three buffers keep the copies' alignment (a 16-B shift splits the
        // B-numerator rows' 64-B segments over two cache lines; ~0.7 us per launch at cfg3)
        const int nc = c->xcopies();
        const long long xl = c->ar_payload();
        if (c->xlen != xl) {
            if (int rc = flush_mstep(c)) return rc;
            // the caller may still read or write the old buffer on its own stream (its all-reduce)
            HIP_TRY(hipDeviceSynchronize());
            dfree(c->d_xbuf);
            if (int rc = dalloc(&c->d_xbuf, 3 * (size_t)xl)) return rc;
            HIP_TRY(hipMemsetAsync(c->d_xbuf, 0, sizeof(double) * 3 * (size_t)xl, c->stream));
            c->xlen = xl;
            c->e_count = 0;
        }
        if (c->pend.on && !c->can_merge())
            if (int rc = flush_mstep(c)) return rc;
        const long long e = c->e_count++;
        double *X = c->d_xbuf + (e % 3) * c->xlen, *Xn = c->d_xbuf + ((e + 1) % 3) * c->xlen;
        const long long ll_off = (long long)nc * c->copy_len();
        // accumulate into X (the merged M-step reads the previous, all-reduced X), clear the next
        if (c->map.nblocks > 0) {
            if (int rc = launch_estep(c, false, c->state(), X, c->llpart(e), Xn, c->xlen, true,
                                      X + ll_off + 2LL * c->rank, nc))
                return rc;
        } else {  // empty shard: contribute zeros (no E-step launch clears the buffers)
            HIP_TRY(hipMemsetAsync(X, 0, sizeof(double) * (size_t)c->xlen, c->stream));
        }
        *buf = X;
        *len = c->xlen;
    } else {
        if (c->ext_len != c->stats_len()) {  // sized by the world of hmmbw_set_rank
            if (int rc = flush_mstep(c)) return rc;
            HIP_TRY(hipStreamSynchronize(c->stream));
            dfree(c->d_ext);
            if (int rc = dalloc(&c->d_ext, (size_t)c->stats_len())) return rc;
            HIP_TRY(hipMemsetAsync(c->d_ext, 0, sizeof(double) * (size_t)c->stats_len(), c->stream));
            c->ext_len = c->stats_len();
        }
        if (int rc = hmmbw_estep(c, c->d_ext)) return rc;
        *buf = c->d_ext;
        *len = c->ext_len;
    }
    c->ar_open = true;
    c->ar_fused = fused;
    c->ar_cur = *buf;
    c->ar_R = n_seq_global;
    return HMMBW_OK;
}

// Second half: the M-step from the all-reduced buffer (merged into the next E-step launch when it can).
static int mr_end(hmmbw_ctx *c) {
    if (!c->ar_open) return fail(HMMBW_E_STATE, "no open iteration (hmmbw_iterate_begin first)");
    c->ar_open = false;
    if (!c->ar_fused) return hmmbw_mstep(c, c->ar_cur, c->ar_R);
    return pend_reduced(c, c->ar_cur, c->xcopies(), c->ar_R);
}

int hmmbw_iterate_begin(hmmbw_ctx *c, int64_t n_seq_global, double **buf, int64_t *n_doubles) {
    if (int rc = check_ready(c, true)) return rc;
    if (!buf || !n_doubles) return fail(HMMBW_E_INVALID, "null argument");
    if (n_seq_global < 0) return fail(HMMBW_E_INVALID, "negative sequence count");
    if (c->ar_kind == HMMBW_ALLREDUCE_PEER && !c->peer_mode()) return fail(HMMBW_E_STATE, peer_off_msg(c));
    long long len = 0;
    if (int rc = mr_begin(c, n_seq_global, buf, &len)) return rc;
    if (c->peer_mode()) {  // the whole exchange is the engine's: push now, wait + sum in _end
        if (int rc = peer_push(c, *buf, len)) {
            c->ar_open = false;
            return rc;
        }
        c->ar_len_last = len;
    }
    *n_doubles = len;
    return HMMBW_OK;
}

int hmmbw_iterate_end(hmmbw_ctx *c) {
    if (int rc = check_ready(c, true)) return rc;
    if (c->ar_open && c->peer_mode())
        if (int rc = peer_reduce(c)) {
            c->ar_open = false;
            return rc;
        }
    return mr_end(c);
}

int hmmbw_allreduce_kind(const hmmbw_ctx *c, int *kind) {
    if (!c || !kind) return fail(HMMBW_E_INVALID, "null argument");
    if (c->peer_mode()) *kind = HMMBW_ALLREDUCE_PEER;
    else if (c->world > 1 || c->comm) *kind = HMMBW_ALLREDUCE_RCCL;
    else *kind = -1;
    return HMMBW_OK;
}

int hmmbw_iterate(hmmbw_ctx *c, int64_t n_iter) {
    if (int rc = check_ready(c, true)) return rc;
    if (int rc = check_closed(c)) return rc;
    if (c->world != 1 || c->comm || c->peer_mode()) {
        // multi-rank with the engine's own all-reduce: estep -> ncclAllReduce (this stream) or the peer
        // push / wait + sum -> mstep
        const bool peer = c->peer_mode();
        if (c->ar_kind == HMMBW_ALLREDUCE_PEER && !peer) return fail(HMMBW_E_STATE, peer_off_msg(c));
        if (!peer && !c->comm)
            return fail(HMMBW_E_STATE, "multi-rank hmmbw_iterate needs hmmbw_comm_init or the peer all-reduce "
                                       "(or use hmmbw_iterate_begin / all-reduce / _end)");
        if (!peer)
            if (int rc = hmmbw_comm_probe(nullptr)) return rc;
        for (int64_t i = 0; i < n_iter; ++i) {
            double *ar = nullptr;
            long long ar_len = 0;
            if (int rc = mr_begin(c, c->R_global, &ar, &ar_len)) return rc;
            // between mr_begin and mr_end: any failure closes the iteration again, or every later
            // training call would fail with HMMBW_E_STATE
            auto collective = [&]() -> int {
                const bool timed = c->timing && (c->ar_seq++ % c->timing) == 0;
                if (timed)
                    if (int rc = c->ar_timed.take(c->stream)) return rc;
                // also at world 1 (RCCL's in-place 1-rank sum is a copy kernel, ~2 us): the 1-rank
                // communicator tests then exercise the same ncclAllReduce call as an 8-GPU run
                c->ar_len_last = ar_len;
                if (peer) {
                    if (int rc = peer_allreduce(c, ar, ar_len)) return rc;
                } else {
                    if (int rc = comm_allreduce(c, ar, ar_len)) return rc;
                }
                if (timed) {
                    if (int rc = c->ar_timed.done(c->stream)) return rc;
                    if (c->ar_timed.pending.size() >= 256)
                        if (int rc = c->ar_timed.drain()) return rc;
                }
                return HMMBW_OK;
            };
            if (int rc = collective()) {
                c->ar_open = false;
                return rc;
            }
            if (int rc = mr_end(c)) return rc;
        }
        return HMMBW_OK;
    }
    const long long nz = (long long)c->ncopies * c->copy_len();
    for (int64_t i = 0; i < n_iter; ++i) {
        if (c->pend.on && !c->can_merge())
            if (int rc = flush_mstep(c)) return rc;
        const long long e = c->e_count++;
        // statistics triple buffer: this launch adds into e, the merged M-step reads e - 1, and e + 1
        // (read by launch e - 2) is cleared for the next launch
        if (int rc = launch_estep(c, false, c->state(), c->copies(e), c->llpart(e), c->copies(e + 1), nz, true))
            return rc;
        pend_local(c, e, c->last_nll);
        if (!c->can_merge())
            if (int rc = flush_mstep(c)) return rc;
        if (c->timing && c->timed.pending.size() >= 256)
            if (int rc = drain_timing(c)) return rc;
    }
    return HMMBW_OK;
}

static void fill_status(const IterState &h, hmmbw_status *st) {
    st->iterations = h.iteration;
    st->done = h.done;
    st->converged = h.converged;
    st->last_log_likelihood = h.last_L;
    st->last_diff = h.last_diff;
}

int hmmbw_get_status(hmmbw_ctx *c, hmmbw_status *st, hmmbw_iter_record *rec, int64_t first, int64_t count) {
    if (!c || !st) return fail(HMMBW_E_INVALID, "null argument");
    if (int rc = set_device(c)) return rc;
    if (int rc = flush_mstep(c)) return rc;
    IterState h{};
    HIP_TRY(hipMemcpyAsync(&h, c->state(), sizeof(IterState), hipMemcpyDeviceToHost, c->stream));
    std::vector<double> hist(2 * (size_t)kHist);
    if (rec && count > 0)
        HIP_TRY(hipMemcpyAsync(hist.data(), c->d_hist, sizeof(double) * hist.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    fill_status(h, st);
    if (h.error) return fail(h.error, device_error(h));
    if (rec && count > 0) {
        if (first < 0 || first + count > h.iteration || first < h.iteration - kHist)
            return fail(HMMBW_E_INVALID, "requested iteration records are not available");
        for (int64_t i = 0; i < count; ++i) {
            const int64_t k = (first + i) % kHist;
            rec[i].log_likelihood = hist[2 * k];
            rec[i].diff = hist[2 * k + 1];
        }
    }
    return HMMBW_OK;
}

int hmmbw_status_post(hmmbw_ctx *c, int64_t first, int64_t *ticket) {
    if (!c || !ticket) return fail(HMMBW_E_INVALID, "null argument");
    if (first < 0) return fail(HMMBW_E_INVALID, "negative first iteration");
    if (int rc = set_device(c)) return rc;
    hmmbw_ctx::Snap &sn = c->snaps[c->snap_next % 2];
    if (!sn.ev) {
        HIP_TRY(hipEventCreateWithFlags(&sn.ev, hipEventDisableTiming));
        // fine-grained host memory the snapshot kernel writes (visible once its event has completed)
        HIP_TRY(cached_alloc(reinterpret_cast<void **>(&sn.st), sizeof(IterState), kPinnedBlock));
        HIP_TRY(cached_alloc(reinterpret_cast<void **>(&sn.hist), sizeof(double) * 2 * (size_t)kHist, kPinnedBlock));
    } else {
        HIP_TRY(hipEventSynchronize(sn.ev));  // the slot's previous snapshot has landed (two posts ago)
    }
    // no flush: a pending (merged) M-step stays pending, so the snapshot holds the records of every
    // iteration enqueued so far except the last one
    hipLaunchKernelGGL(k_snapshot, dim3(1), dim3(256), 0, c->stream, c->state(), c->d_hist, (long long)first, sn.st,
                       sn.hist);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(sn.ev, c->stream));
    sn.first = first;
    sn.ticket = c->snap_next++;
    *ticket = sn.ticket;
    return HMMBW_OK;
}

int hmmbw_status_wait(hmmbw_ctx *c, int64_t ticket, hmmbw_status *st, hmmbw_iter_record *rec, int64_t first,
                      int64_t count) {
    if (!c || !st) return fail(HMMBW_E_INVALID, "null argument");
    if (ticket < 0 || ticket >= c->snap_next || ticket < c->snap_next - 2)
        return fail(HMMBW_E_INVALID, "status ticket is not one of the last two posted");
    if (int rc = set_device(c)) return rc;
    hmmbw_ctx::Snap &sn = c->snaps[ticket % 2];
    HIP_TRY(hipEventSynchronize(sn.ev));  // this snapshot only, not the work enqueued after it
    const IterState h = *sn.st;
    fill_status(h, st);
    if (h.error) return fail(h.error, device_error(h));
    if (rec && count > 0) {
        if (first < sn.first || first + count > h.iteration || first + count > sn.first + kHist ||
            first < h.iteration - kHist)  // overwritten in the ring before the snapshot was taken
            return fail(HMMBW_E_INVALID, "requested iteration records are not in this snapshot");
        for (int64_t i = 0; i < count; ++i) {
            const int64_t k = first + i - sn.first;
            rec[i].log_likelihood = sn.hist[2 * k];
            rec[i].diff = sn.hist[2 * k + 1];
        }
    }
    return HMMBW_OK;
}

int hmmbw_status_live_wait(hmmbw_ctx *c, int64_t iterations, hmmbw_status *st, hmmbw_iter_record *rec,
                           int64_t first, int64_t count) {
    if (!c || !st) return fail(HMMBW_E_INVALID, "null argument");
    if (!c->h_live) return fail(HMMBW_E_STATE, "HMMBW_OPT_LIVE_STATUS is off");
    if (int rc = set_device(c)) return rc;
    volatile LiveBlock *lv = c->h_live;
    IterState h{};
    bool have = false;
    for (long long spin = 0;; ++spin) {
        const unsigned long long p0 = lv->pub;
        std::atomic_thread_fence(std::memory_order_acquire);
        if ((unsigned)(p0 >> 32) == c->live_epoch) {
            const long long n = (long long)(unsigned)(p0 & 0xffffffffULL);
            const volatile IterState &sl = lv->slot[n & 1];
            h.prev_L = sl.prev_L;
            h.last_L = sl.last_L;
            h.last_diff = sl.last_diff;
            h.epsilon = sl.epsilon;
            h.iteration = sl.iteration;
            h.max_iterations = sl.max_iterations;
            h.done = sl.done;
            h.converged = sl.converged;
            h.error = sl.error;
            std::atomic_thread_fence(std::memory_order_acquire);
            const unsigned long long p1 = lv->pub;
            // the slot is rewritten only by the record after next: two publications apart
            const bool stable = (unsigned)(p1 >> 32) == c->live_epoch && (long long)(unsigned)(p1 & 0xffffffffULL) <= n + 1;
            if (stable && h.iteration == n && (n >= iterations || h.done)) {
                have = true;
                break;
            }
        }
        // the stream ran dry without the record (a pending M-step, a device-side stop the mirror does not
        // carry, or a reset): the device state is the answer
        if ((spin & 63) == 63 && hipStreamQuery(c->stream) == hipSuccess) {
            const unsigned long long p2 = lv->pub;
            if ((unsigned)(p2 >> 32) == c->live_epoch && (long long)(unsigned)(p2 & 0xffffffffULL) >= iterations) continue;
            break;
        }
    }
    std::vector<double> dh;
    if (!have) {
        HIP_TRY(hipMemcpy(&h, c->state(), sizeof(IterState), hipMemcpyDeviceToHost));
        if (rec && count > 0) {
            dh.resize(2 * (size_t)kHist);
            HIP_TRY(hipMemcpy(dh.data(), c->d_hist, sizeof(double) * dh.size(), hipMemcpyDeviceToHost));
        }
    }
    fill_status(h, st);
    if (h.error) return fail(h.error, device_error(h));
    if (rec && count > 0) {
        if (first < 0 || first + count > h.iteration || first < h.iteration - kHist)
            return fail(HMMBW_E_INVALID, "requested iteration records are not available");
        for (int64_t i = 0; i < count; ++i) {
            const int64_t k = (first + i) % kHist;
            rec[i].log_likelihood = have ? lv->hist[2 * k] : dh[2 * k];
            rec[i].diff = have ? lv->hist[2 * k + 1] : dh[2 * k + 1];
        }
    }
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
    if (int rc = launch_estep(c, true, nullptr)) return rc;
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
