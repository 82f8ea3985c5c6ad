// mstep.hpp — the M-step and the convergence step (hmm_training.py:415-514): the element formulas every variant
// shares, the folding of the log-likelihood (max, sum exp) pairs, the iteration record, and the three stand-alone
// bodies (k_mstep, k_mstep_grid, k_mstep_staged in hmmbw.hip).  The fourth variant, merged_mstep, runs in the
// small E-step's prologue and fills its LDS tables, so it sits with them in hmmbw_device.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "hmmbw_args.hpp"
#include "lane_ops.hpp"

namespace hmmbw {

// ---------------------------------------------------------------------------------------------
// Element formulas.  Every M-step variant forms pi, A and B entries with these, from statistics summed
// over the copies in the same order, so all of them produce bit-identical parameters.
// ---------------------------------------------------------------------------------------------
// pi_i (:415-424) from its numerator and the number of sequences R; no term -> 0
__device__ __forceinline__ double mstep_pi(double num, long long R) { return num > 0.0 ? num / (double)R : 0.0; }
// a_ij (:429-455) from the xi numerator and the row's denominator, which excludes the last frame
__device__ __forceinline__ double mstep_a(double num, double den) {
    return (den > 0.0 && num > 0.0) ? num / den : 0.0;
}
// B entry from its numerator and the reciprocal of its row's denominator (:460-497): 1e-20 floor when
// no gamma term carries the symbol, 0 for an empty row.
__device__ __forceinline__ double mstep_inv(double den) { return den > 0.0 ? 1.0 / den : 0.0; }
__device__ __forceinline__ double bnum_to_b(double num, double inv) {
    return inv > 0.0 ? (num > 0.0 ? num * inv : 1e-20) : 0.0;
}
// b_jj(k) into B [N][K] and into B^T [K][G], the kernels' emission table (bt_perm: in the wide kernels' column order)
__device__ __forceinline__ void put_b(const MArgs &m, int jj, int k, double v) {
    m.B[(long long)jj * m.K + k] = v;
    m.Bt[(long long)k * m.G + (m.bt_perm ? bt_col(jj) : jj)] = v;
}

// sum of one statistic over the copies, clearing them for the next iteration
__device__ __forceinline__ double take(const MArgs &m, long long idx) {
    double v = 0.0;
    double *p = const_cast<double *>(m.src) + idx;
    for (int c = 0; c < m.nsrc; ++c) {
        v += p[c * m.copy_len];
        p[c * m.copy_len] = 0.0;
    }
    return v;
}

// ... and only reading them (each E-step launch clears the buffer it will fill)
__device__ __forceinline__ double peek(const MArgs &m, long long idx) {
    double v = 0.0;
    for (int c = 0; c < m.nsrc; ++c) v += m.src[c * m.copy_len + idx];
    return v;
}

// ---------------------------------------------------------------------------------------------
// Log-likelihood pairs: every E-step workgroup writes (max, sum exp(x - max)) of its sequences' log P;
// L = LSE_r log P_r (:503) is folded from them.
// ---------------------------------------------------------------------------------------------
// Per-block (max, sum exp(x - max)) of the sequences' log P (each sequence contributes from
// exactly one lane with valid = true).  All threads of the block call it.
__device__ __forceinline__ void block_ll_partial(double lp, bool valid, double *sh, double *out) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nw = blockDim.x >> 6;
    double m = wave_max(valid ? lp : -INFINITY);
    if (lane == 0) sh[wv] = m;
    __syncthreads();
    double M = -INFINITY;
    for (int w = 0; w < nw; ++w) M = fmax(M, sh[w]);
    const double s = gsum<64>((valid && M != -INFINITY && lp != -INFINITY) ? exp(lp - M) : 0.0);
    __syncthreads();
    if (lane == 0) sh[wv] = s;
    __syncthreads();
    if (tid == 0) {
        double S = 0.0;
        for (int w = 0; w < nw; ++w) S += sh[w];
        // memory-side atomics: in a fused multi-rank launch rank_ll_fold reads the pairs with atomics too
        atomicExch(&out[0], (S > 0.0) ? M : 0.0);
        atomicExch(&out[1], S);
    }
}

// ATOMIC: read with a returning memory-side atomic (inside the producing kernel, where the per-XCD
// L2s give no cross-workgroup visibility for plain loads).
template <bool ATOMIC = false>
__device__ __forceinline__ double rd(const double *p) {
    if constexpr (ATOMIC) return unsafeAtomicAdd(const_cast<double *>(p), 0.0);
    else return *p;
}

// Combine per-block (max, sum exp) pairs into this rank's pair (log_sum_exp :66-79 over :503), by one
// workgroup after a kernel boundary.
__device__ void combine_ll_pairs(const double *pairs, long long n, double *sh, double *m_out, double *s_out) {
    double mx = -INFINITY;
    for (long long r = threadIdx.x; r < n; r += blockDim.x)
        if (rd(&pairs[2 * r + 1]) > 0.0) mx = fmax(mx, rd(&pairs[2 * r]));
    mx = block_reduce(mx, sh, true);
    double s = 0.0;
    if (mx != -INFINITY)
        for (long long r = threadIdx.x; r < n; r += blockDim.x) {
            const double sr = rd(&pairs[2 * r + 1]);
            if (sr > 0.0) s += sr * exp(rd(&pairs[2 * r]) - mx);
        }
    s = block_reduce(s, sh, false);
    *m_out = mx;
    *s_out = s;
}

// merge (max, sum exp) pairs: online log-sum-exp
__device__ __forceinline__ void ll_merge(double &M, double &S, double m2, double s2) {
    if (!(s2 > 0.0)) return;
    if (!(S > 0.0)) { M = m2; S = s2; return; }
    if (m2 > M) { S = S * exp(M - m2) + s2; M = m2; }
    else S += s2 * exp(m2 - M);
}

// L = LSE_r log P_r (:503) from one all-reduced (max, sum exp) pair per rank, by ONE thread in rank
// order.  Every multi-rank M-step variant (the merged prologue, k_mstep, k_mstep_grid) forms L with
// this function, so ranks that run different variants (an empty shard cannot merge its M-step) still
// hold bitwise-identical L and diff and take the same stop decision (:346).
__device__ __forceinline__ double lse_rank_pairs(const double *ll, long long n) {
    double mx = -INFINITY;
    for (long long r = 0; r < n; ++r)
        if (ll[2 * r + 1] > 0.0) mx = fmax(mx, ll[2 * r]);
    double s = 0.0;
    if (mx != -INFINITY)
        for (long long r = 0; r < n; ++r)
            if (ll[2 * r + 1] > 0.0) s += ll[2 * r + 1] * exp(ll[2 * r] - mx);
    return (s > 0.0) ? mx + log(s) : -INFINITY;
}

// Multi-rank fused E-step (hmmbw_iterate with the engine communicator): the workgroups accumulate
// straight into the all-reduce buffer, and wave 0 of the LAST workgroup to count its pair in (completion
// counter) folds the per-workgroup (max, sum exp) pairs into this rank's slot (what k_reduce_local did
// in its own launch).  No __threadfence: a device-scope release writes back the XCD's L2 (this launch's
// checkpoints), which cost ~20 us per launch; the pairs are memory-side atomics, so thread 0 only has
// to see its own pair land (vmcnt(0)) before it counts, and the folding wave reads them with atomics.
__device__ __forceinline__ int rank_ll_count(const EArgs &a) {
    __builtin_amdgcn_s_waitcnt(0x0F70);  // s_waitcnt vmcnt(0): block_ll_partial's atomicExch has landed
    return atomicAdd(a.done_ctr, 1);
}

__device__ __forceinline__ void rank_ll_fold(const EArgs &a, long long nblk) {  // one wave
    const int lane = threadIdx.x & 63;
    double tm = -INFINITY, ts = 0.0;
    for (long long r0 = 0; r0 < nblk; r0 += 4 * 64) {
        double pm[4], ps[4];  // every round's memory-side reads issued together
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const long long r = r0 + lane + q * 64;
            pm[q] = r < nblk ? rd<true>(&a.llpart[2 * r]) : 0.0;
            ps[q] = r < nblk ? rd<true>(&a.llpart[2 * r + 1]) : 0.0;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (!(ps[q] > 0.0)) continue;
            if (pm[q] > tm) {
                ts = (tm == -INFINITY) ? ps[q] : ps[q] + ts * exp(tm - pm[q]);
                tm = pm[q];
            } else {
                ts += ps[q] * exp(pm[q] - tm);
            }
        }
    }
    const double mx = wave_max(tm);
    const double s = gsum<64>((mx != -INFINITY && ts > 0.0) ? ts * exp(tm - mx) : 0.0);
    if (lane == 0) {
        atomicExch(&a.rank_ll[0], (s > 0.0) ? mx : 0.0);
        atomicExch(&a.rank_ll[1], s);
        atomicExch(a.done_ctr, 0);
    }
}

// ---------------------------------------------------------------------------------------------
// The iteration record and the stand-alone M-step bodies
// ---------------------------------------------------------------------------------------------
// Convergence record of one EM iteration (hmm_training.py:503-514): L of the parameters that entered
// it, diff (+inf on the first iteration), the stop rule of :346; written to the next state slot.
__device__ bool record_iteration(const MArgs &m, const IterState &in, double L) {
    const double diff = (in.prev_L != -INFINITY) ? fabs(L - in.prev_L) : INFINITY;  // :505-508
    const long long it = in.iteration;
    const bool cont = (diff >= in.epsilon) && (it + 1 < in.max_iterations);
    m.hist[2 * (it % kHist)] = L;
    m.hist[2 * (it % kHist) + 1] = diff;
    IterState o = in;
    o.prev_L = L;
    o.last_L = L;
    o.last_diff = diff;
    o.iteration = it + 1;
    if (!cont) {
        o.done = 1;
        o.converged = (it + 1 < in.max_iterations) ? 1 : 0;
    }
    *m.state_out = o;
    if (m.live != nullptr) {  // the host mirror: record and state first, then (acknowledged) the publication
        auto sys = [](auto *p, auto v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); };
        sys(&m.live->hist[2 * (it % kHist)], L);
        sys(&m.live->hist[2 * (it % kHist) + 1], diff);
        IterState *sl = &m.live->slot[o.iteration & 1];
        sys(&sl->prev_L, o.prev_L);
        sys(&sl->last_L, o.last_L);
        sys(&sl->last_diff, o.last_diff);
        sys(&sl->epsilon, o.epsilon);
        sys(&sl->iteration, o.iteration);
        sys(&sl->max_iterations, o.max_iterations);
        sys(&sl->done, o.done);
        sys(&sl->converged, o.converged);
        sys(&sl->error, o.error);
        sys(&sl->error_src, o.error_src);
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): every store above is acknowledged
        sys(&m.live->pub, ((unsigned long long)m.live_epoch << 32) | (unsigned long long)(unsigned)o.iteration);
    }
    return cont;
}

// M-step kernels entered after convergence carry the state over to the next slot and do nothing else
__device__ __forceinline__ bool carry_if_done(const MArgs &m) {
    if (!m.state->done) return false;
    if (threadIdx.x == 0 && blockIdx.x == 0) *m.state_out = *m.state;
    return true;
}

// M-step + convergence by one workgroup of 256 threads (hmm_training.py:415-514).
__device__ void mstep_block(const MArgs &m) {
    __shared__ double sh[16];
    __shared__ double sL;
    __shared__ double sPi[64], sGex[64], sGall[64];
    const IterState *st = m.state;
    const int tid = threadIdx.x;
    // L = LSE_r log P_r over all ranks (:503)
    if (m.local_lse) {
        double mx, s;
        combine_ll_pairs(m.llpart, m.nblocks, sh, &mx, &s);
        if (tid == 0) sL = (s > 0.0) ? mx + log(s) : -INFINITY;
    } else if (tid == 0) {
        sL = lse_rank_pairs(m.llpart, m.nblocks);  // one (max, sum exp) pair per rank, all-reduced
        for (long long r = 0; r < 2 * m.nblocks; ++r) m.zero_ll[r] = 0.0;
    }
    const int N = m.N, K = m.K;
    for (int i = tid; i < N; i += blockDim.x) {
        sPi[i] = take(m, i);
        sGex[i] = take(m, m.off_gex + i);
        sGall[i] = take(m, m.off_gall + i);
    }
    __syncthreads();
    for (int i = tid; i < N; i += blockDim.x) m.pi[i] = mstep_pi(sPi[i], m.R_global);
    for (int idx = tid; idx < N * N; idx += blockDim.x) {
        const double den = sGex[idx / N];
        const double num = take(m, m.off_S + idx);
        m.A[idx] = mstep_a(num, den);
    }
    for (long long idx = tid; idx < (long long)N * K; idx += blockDim.x) {
        const int jj = (int)(idx % N), k = (int)(idx / N);  // symbol-major: coalesced over the copies
        const double num = take(m, m.off_bnum + idx);
        put_b(m, jj, k, bnum_to_b(num, mstep_inv(sGall[jj])));
    }
    __syncthreads();
    if (tid == 0) record_iteration(m, *st, sL);
}

// M-step + convergence spread over the whole grid (large N x K, e.g. the wide path's 64 x 1024 B):
// every workgroup re-estimates its grid-stride share of B and A from the statistics summed over the
// copies; workgroup 0 also does pi, L and the convergence record (:503-514).  The statistics are only
// read (peek), so no workgroup depends on another.
__device__ void mstep_grid(const MArgs &m) {
    __shared__ double sh[16];
    __shared__ double sL;
    __shared__ double sGall[64];
    const int tid = threadIdx.x;
    const int N = m.N, K = m.K;
    for (int i = tid; i < N; i += blockDim.x) sGall[i] = mstep_inv(peek(m, m.off_gall + i));
    __syncthreads();
    for (long long idx = (long long)blockIdx.x * blockDim.x + tid; idx < (long long)N * K;
         idx += (long long)gridDim.x * blockDim.x) {
        const int jj = (int)(idx % N), k = (int)(idx / N);  // symbol-major: coalesced reads
        put_b(m, jj, k, bnum_to_b(peek(m, m.off_bnum + idx), sGall[jj]));
    }
    for (long long idx = (long long)blockIdx.x * blockDim.x + tid; idx < (long long)N * N;
         idx += (long long)gridDim.x * blockDim.x) {
        const double den = peek(m, m.off_gex + idx / N);
        const double num = peek(m, m.off_S + idx);
        m.A[idx] = mstep_a(num, den);
    }
    if (blockIdx.x != 0) return;
    if (m.local_lse) {
        double mx, s;
        combine_ll_pairs(m.llpart, m.nblocks, sh, &mx, &s);
        if (tid == 0) sL = (s > 0.0) ? mx + log(s) : -INFINITY;
    } else if (tid == 0) {
        sL = lse_rank_pairs(m.llpart, m.nblocks);  // one (max, sum exp) pair per rank, all-reduced
    }
    for (int i = tid; i < N; i += blockDim.x) m.pi[i] = mstep_pi(peek(m, i), m.R_global);
    __syncthreads();
    if (tid == 0) record_iteration(m, *m.state, sL);
}

// M-step staged through LDS (sSt: copy_len doubles), single rank, its own kernel: the statistics (summed
// over the copies, which are cleared) and the per-workgroup log-likelihood pairs are gathered with plain
// loads in independent batches, then the update runs from LDS.
__device__ void mstep_staged(const MArgs &m, double *sSt) {
    __shared__ double sM[16], sS[16];
    __shared__ double sL;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nw = blockDim.x >> 6;
    const int N = m.N, K = m.K;
    const long long len = m.copy_len;
    // ---- one batch of independent loads: convergence state, LL pairs, statistics ----
    IterState in{};
    if (tid == 0) in = *m.state;
    // Branch-free, clamped addresses so the compiler issues every load of a batch before the first
    // wait (a guarded load inside a runtime loop serialises on its own s_waitcnt).
    constexpr int PB = 4;
    double pm[PB], ps[PB];
    double M = -INFINITY, S = 0.0;
    const long long nb = m.nblocks;  // >= 1 (a launch with no workgroups leaves nothing pending)
    for (long long r0 = 0; r0 < nb; r0 += (long long)PB * blockDim.x) {
#pragma unroll
        for (int u = 0; u < PB; ++u) {
            const long long r = r0 + (long long)u * blockDim.x + tid;
            const long long rc = r < nb ? r : nb - 1;
            pm[u] = rd(m.llpart + 2 * rc);
            ps[u] = rd(m.llpart + 2 * rc + 1);
        }
#pragma unroll
        for (int u = 0; u < PB; ++u) {
            const bool ok = r0 + (long long)u * blockDim.x + tid < nb;
            ll_merge(M, S, ok ? pm[u] : -INFINITY, ok ? ps[u] : 0.0);
        }
    }
    constexpr int B = 16;
    double *src = const_cast<double *>(m.src);
    for (long long base = 0; base < len; base += (long long)B * blockDim.x) {
        double v[B];
#pragma unroll
        for (int u = 0; u < B; ++u) v[u] = 0.0;
        for (int c = 0; c < m.nsrc; ++c) {
            double x[B];
#pragma unroll
            for (int u = 0; u < B; ++u) {
                const long long idx = base + (long long)u * blockDim.x + tid;
                double *q = src + c * len + (idx < len ? idx : len - 1);
                x[u] = *q;
            }
#pragma unroll
            for (int u = 0; u < B; ++u) v[u] += x[u];
        }
#pragma unroll
        for (int u = 0; u < B; ++u) {
            const long long idx = base + (long long)u * blockDim.x + tid;
            if (idx < len) {
                sSt[idx] = v[u];
                for (int c = 0; c < m.nsrc; ++c) src[c * len + idx] = 0.0;
            }
        }
    }
    // ---- L = LSE_r log P_r (:503) ----
    for (int k = 32; k >= 1; k >>= 1) ll_merge(M, S, __shfl_xor(M, k), __shfl_xor(S, k));
    if (lane == 0) { sM[wv] = M; sS[wv] = S; }
    __syncthreads();
    if (tid == 0) {
        double MM = -INFINITY, SS = 0.0;
        for (int w = 0; w < nw; ++w) ll_merge(MM, SS, sM[w], sS[w]);
        sL = (SS > 0.0) ? MM + log(SS) : -INFINITY;
    }
    __syncthreads();
    const double *sPi = sSt, *sS_ = sSt + m.off_S, *sGex = sSt + m.off_gex, *sGall = sSt + m.off_gall,
                 *sBn = sSt + m.off_bnum;
    if (tid < N) m.pi[tid] = mstep_pi(sPi[tid], m.R_global);
    if (tid < N * N) {
        const double den = sGex[tid / N];
        const double num = sS_[tid];
        m.A[tid] = mstep_a(num, den);
    }
    for (int idx = tid; idx < N * K; idx += blockDim.x) {
        const int k = idx / N, jj = idx - k * N;
        put_b(m, jj, k, bnum_to_b(sBn[idx], mstep_inv(sGall[jj])));
    }
    if (tid == 0) record_iteration(m, in, sL);
}

}  // namespace hmmbw
