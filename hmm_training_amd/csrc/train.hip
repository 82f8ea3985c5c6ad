// train.hip — the M-step and the training loops: hmmbw_reset_training, hmmbw_estep / _mstep, hmmbw_iterate and its
// multi-rank halves hmmbw_iterate_begin / _end.
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

void init_state(hmmbw_ctx *c, IterState *slot, double epsilon, long long max_iterations) {
    hipLaunchKernelGGL(k_init_state, dim3(1), dim3(1), 0, c->stream, slot, epsilon, max_iterations);
}

// ---------------------------------------------------------------------------------------------
// The pending M-step
// ---------------------------------------------------------------------------------------------
// M-step arguments for the pending statistics: this context's copies (single rank) or the caller's
// all-reduced buffer with one (max, sum exp) pair per rank
MArgs make_margs(hmmbw_ctx *c, const hmmbw_ctx::Pending &p) {
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

int next_estep(hmmbw_ctx *c, long long *e) {
    if (c->pend.on && !c->can_merge())
        if (int rc = flush_mstep(c)) return rc;
    *e = c->e_count++;
    return HMMBW_OK;
}

}  // namespace hmmbw

extern "C" {

int hmmbw_reset_training(hmmbw_ctx *c, double epsilon, int64_t max_iterations) {
    if (!c) return fail(HMMBW_E_INVALID, "null context");
    if (int rc = check_closed(c)) return rc;
    if (int rc = set_device(c)) return rc;
    if (int rc = flush_mstep(c)) return rc;
    init_state(c, c->state(), epsilon, (long long)max_iterations);
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

int hmmbw_estep(hmmbw_ctx *c, double *stats_dev) {
    if (int rc = check_ready(c, true)) return rc;
    if (int rc = check_closed(c)) return rc;
    if (!stats_dev) return fail(HMMBW_E_INVALID, "null stats buffer");
    long long e = 0;
    if (int rc = next_estep(c, &e)) return rc;
    const EstepIo io = c->io_packed(e);
    if (int rc = launch_estep(c, io)) return rc;
    const long long n = c->copy_len();
    const unsigned grid = (unsigned)std::min<long long>((n + 255) / 256, 64);
    // last_nll, not map.nblocks: the joined map writes one pair per full workgroup.  c->state(), not io.state: a
    // merged M-step in the launch has flipped the slot.
    hipLaunchKernelGGL(k_reduce_local, dim3(grid), dim3(256), 0, c->stream, io.copies, c->det ? 1 : c->ncopies, n,
                       io.llpart, c->last_nll, stats_dev, c->off_ll(), c->world, c->rank, c->state());
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
        const long long xl = c->ar_payload();
        if (c->xlen != xl) {
            if (int rc = flush_mstep(c)) return rc;
            // the caller may still read or write the old buffer on its own stream (its all-reduce)
            HIP_TRY(hipDeviceSynchronize());
            dfree(c->d_xbuf);
            if (int rc = dalloc(&c->d_xbuf, 3 * (size_t)xl)) return rc;
            HIP_TRY(hipMemsetAsync(c->d_xbuf, 0, sizeof(double) * 3 * (size_t)xl, c->stream));
            c->xlen = xl;
            c->e_count = 0;  // all three new buffers are clear: the rotation starts over
        }
        long long e = 0;
        if (int rc = next_estep(c, &e)) return rc;
        const EstepIo io = c->io_fused(e);
        if (c->map.nblocks > 0) {
            if (int rc = launch_estep(c, io)) return rc;
        } else {  // empty shard: contribute zeros (no E-step launch clears the buffers)
            HIP_TRY(hipMemsetAsync(io.copies, 0, sizeof(double) * (size_t)c->xlen, c->stream));
        }
        *buf = io.copies;
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
    for (int64_t i = 0; i < n_iter; ++i) {
        long long e = 0;
        if (int rc = next_estep(c, &e)) return rc;
        if (int rc = launch_estep(c, c->io_local(e))) return rc;
        pend_local(c, e, c->last_nll);  // what the launch wrote: the joined map has one pair per full workgroup
        if (!c->can_merge())
            if (int rc = flush_mstep(c)) return rc;
        if (c->timing && c->timed.pending.size() >= 256)
            if (int rc = drain_timing(c)) return rc;
    }
    return HMMBW_OK;
}

}  // extern "C"
