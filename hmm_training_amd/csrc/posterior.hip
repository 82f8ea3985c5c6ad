// posterior.hip — smoothed state posteriors and posterior (max-marginal) decoding (hmmbw_posterior,
// include/hmmbw.h) for gfx950: gamma_t(i) = P(q_t = i | O, lambda) of every loaded sequence, the state with
// the largest gamma at every step, and log P(O | lambda), under the context's current parameters.
//
// Scaled-linear fp64, no logarithm on the chain:
//   forward   alpha_0(j) = pi_j b_j(o_0),   alpha_t(j) = (sum_i alpha_{t-1}(i) a_ij) b_j(o_t)
//   backward  beta_{T-1} = 1,               beta_t(i)  = sum_j a_ij (b_j(o_{t+1}) beta_{t+1}(j))
// each rescaled at every step by an exact power of two taken from the group's largest exponent, and
//   gamma_t(i) = alpha_t(i) beta_t(i) / sum_i alpha_t(i) beta_t(i).
// The row's own sum normalises it, so the scale factors cancel and none is stored; log P is
// log sum_j alpha_{T-1}(j) + ln 2 (the sum of the forward exponents).
//
// The mapping is the decoder's (viterbi.hip): a group of GV lanes per sequence, lane j = state j, a wave takes
// the 64 / GV consecutive layout slots from v * 64 / GV and reads the symbols from the context's own packs.  The
// output is the workspace: the forward writes alpha_t(j) to gamma[(out + t) N + j], the backward reads it back
// and overwrites it with gamma_t(j); a lane re-reads only what it wrote itself, so program order suffices.  A
// sequence whose forward reaches an all-zero alpha (P(O) = 0) gets zeros in every row and -1 in its path.
#include "word_units.hpp"  // fill_slot_args, check_path_len

namespace hmmbw {

struct PArgs {
    const uint16_t *sym;
    const long long *wave_symoff;
    const int *slot_len, *slot_seq;
    const long long *slot_out;
    const double *tab;   // [GV] pi | [GV][GV] A, tab[GV + i GV + j] = a_ij | [K][GV] B^T; 0 in states >= N
    double *gamma;       // [total][N], caller CSR order (nullptr: forward only)
    double *logp;
    int32_t *path;       // nullptr: no path
    long long nslots;
    int U, N, K;
    int shift;           // pack entry -> symbol: >> shift, or / div when shift < 0
    int div;
};

// tab from the linear parameters (pi [N], A [N][N] row-major, B [N][K])
__global__ void __launch_bounds__(256) k_posterior_prep(const double *__restrict__ pi, const double *__restrict__ A,
                                                        const double *__restrict__ B, int N, int K, int GV,
                                                        double *__restrict__ tab) {
    const long long nA = (long long)GV * GV, n = GV + nA + (long long)K * GV;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        double v = 0.0;
        if (e < GV) {
            if (e < N) v = pi[e];
        } else if (e < GV + nA) {
            const int i = (int)((e - GV) / GV), j = (int)((e - GV) % GV);
            if (i < N && j < N) v = A[i * N + j];
        } else {
            const long long k = (e - GV - nA) / GV;
            const int j = (int)((e - GV - nA) % GV);
            if (j < N) v = B[(long long)j * K + k];
        }
        tab[e] = v;
    }
}

// The transition product of a step, per GV-lane group: sum_i x(lane i) c[i].  The forward gives lane j column j
// of A (c[i] = a_ij), the backward row j (c[i] = a_ji).  Left-to-right: c = {neighbour, self}, the neighbour
// being lane j - 1 in the forward (row_shr:1) and lane j + 1 in the backward (row_shl:1); its coefficient is 0
// where the neighbour is outside the group.  Every lane of the wave must be active.
template <int GV, bool LR, bool FWD, int NC>
__device__ __forceinline__ double trans_dot(double x, const double (&c)[NC], int lane, int N) {
    if constexpr (LR) {
        const double nb = FWD ? dpp<0x111>(x) : dpp<0x101>(x);
        return fma(nb, c[0], x * c[1]);
    } else if constexpr (GV <= 16) {
        double acc0 = 0.0, acc1 = 0.0;
        bcast_dot<GV, GV>(acc0, acc1, x, c);
        return acc0 + acc1;
    } else {
        // v_readlane broadcasts in straight-line blocks of 16; a block wholly past N is skipped (wave-uniform)
        double acc0 = 0.0, acc1 = 0.0;
        sfor<0, GV / 16>([&](auto Bk) {
            constexpr int b = decltype(Bk)::value;
            if (b == 0 || b * 16 < N) {
                sfor<0, 8>([&](auto P) {
                    constexpr int i0 = b * 16 + 2 * decltype(P)::value, i1 = i0 + 1;
                    acc0 = fma(gbcast_wide<GV, i0>(x, lane), c[i0], acc0);
                    acc1 = fma(gbcast_wide<GV, i1>(x, lane), c[i1], acc1);
                });
            }
        });
        return acc0 + acc1;
    }
}

template <int GV, bool LR, bool FULL, bool LDSTAB>
__global__ void __launch_bounds__(kVitBlock) k_posterior(PArgs a) {
    static_assert(!LR || GV <= 16, "left-to-right: one row shift inside a 16-lane row");
    extern __shared__ double sB[];  // LDSTAB: B^T [K][GV]
    constexpr int SPW = kVitWave / GV;
    constexpr int NC = LR ? 2 : GV;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int j = lane & (GV - 1);
    const double *tabA = a.tab + GV, *tabB = tabA + GV * GV;
    if constexpr (LDSTAB) {
        for (int i = threadIdx.x; i < a.K * GV; i += kVitBlock) sB[i] = tabB[i];
        __syncthreads();
    }
    const double *bt = LDSTAB ? sB : tabB;

    const long long vw = (long long)blockIdx.x * (kVitBlock / kVitWave) + wv;
    const long long s = vw * SPW + lane / GV;
    const bool real = s < a.nslots;
    const int T = real ? a.slot_len[s] : 0;     // 0 in padding slots
    const int seq = real ? a.slot_seq[s] : -1;  // -1 in padding slots
    int Tw = T;  // the wave's longest sequence
#pragma unroll
    for (int m = GV; m < kVitWave; m <<= 1) Tw = max(Tw, __shfl_xor(Tw, m));
    if (Tw == 0) return;

    // chunk c of the slot: 8 steps in one 16-B load, U loads further on per chunk (pack_pos)
    const uint4 *pk = reinterpret_cast<const uint4 *>(a.sym) +
                      (real ? pack_pos(a.wave_symoff[s / a.U], a.U, (int)(s % a.U), 0) / kChunk : 0);
    const long long out = seq >= 0 ? a.slot_out[s] : 0;
    const bool mine = seq >= 0 && j < a.N;  // this lane owns column j of the sequence's rows
    double *gam = nullptr;
    if constexpr (FULL) gam = a.gamma + (mine ? out * a.N + j : 0);

    auto symbol = [&](const uint4 &q, int k) {
        const unsigned w = k < 2 ? q.x : (k < 4 ? q.y : (k < 6 ? q.z : q.w));
        const unsigned e = (k & 1) ? w >> 16 : w & 0xffffu;
        return a.shift >= 0 ? e >> a.shift : e / (unsigned)a.div;
    };

    // ---- forward: alpha_hat_t, rescaled at every step; its rows go to the output
    double c[NC];
    if constexpr (LR) {
        c[0] = j > 0 ? tabA[(j - 1) * GV + j] : 0.0;
        c[1] = tabA[j * GV + j];
    } else {
#pragma unroll
        for (int i = 0; i < GV; ++i) c[i] = tabA[i * GV + j];
    }
    const double pi = a.tab[j];
    double al = 0.0;      // alpha_hat_{T-1} once the slot's steps are done
    long long esum = 0;   // the exponents taken out so far
    for (int t0 = 0; t0 < Tw; t0 += kChunk) {
        uint4 q = make_uint4(0, 0, 0, 0);
        if (t0 < T) q = pk[(long long)(t0 / kChunk) * a.U];
        double bv[kChunk];  // the chunk's emissions, read ahead of the chain (symbol 0's row past the slot's end, unused)
#pragma unroll
        for (int k = 0; k < kChunk; ++k) bv[k] = bt[(size_t)symbol(q, k) * GV + j];
#pragma unroll
        for (int k = 0; k < kChunk; ++k) {
            const int t = t0 + k;
            double v;
            if (t == 0)
                v = pi * bv[k];
            else
                v = trans_dot<GV, LR, true>(al, c, lane, a.N) * bv[k];
            const int e = group_exp<GV>(v);  // kZeroExp: the whole group is zero, and stays zero
            if (t < T) {
                al = pow2_scale(v, e);
                esum += e;
                if constexpr (FULL)
                    if (mine) gam[(long long)t * a.N] = al;
            }
        }
    }
    const double tot = gsum<GV>(al);
    const bool dead = !(tot > 0.0);  // P(O) = 0
    if (seq >= 0 && j == 0) a.logp[seq] = dead ? -INFINITY : log(tot) + 0.6931471805599453094 * (double)esum;

    if constexpr (FULL) {
        // ---- backward: beta_hat_t, gamma_t over alpha_hat_t in place, and the largest gamma's state
        if constexpr (LR) {
            c[0] = j < GV - 1 ? tabA[j * GV + j + 1] : 0.0;
            c[1] = tabA[j * GV + j];
        } else {
#pragma unroll
            for (int i = 0; i < GV; ++i) c[i] = tabA[j * GV + i];
        }
        double beta = 1.0, bnext = 0.0;  // beta_hat_{t+1}, b_j(o_{t+1})
        for (int t0 = (Tw - 1) / kChunk * kChunk; t0 >= 0; t0 -= kChunk) {
            uint4 q = make_uint4(0, 0, 0, 0);
            if (t0 < T) q = pk[(long long)(t0 / kChunk) * a.U];
            // the chunk's alpha_hat and emissions, read ahead of the chain: their addresses do not depend on it
            double av[kChunk], bv[kChunk];
#pragma unroll
            for (int k = 0; k < kChunk; ++k) {
                av[k] = mine && t0 + k < T ? gam[(long long)(t0 + k) * a.N] : 0.0;
                bv[k] = bt[(size_t)symbol(q, k) * GV + j];
            }
            // the chain: beta_hat_t, and alpha_hat_t beta_hat_t over alpha_hat_t (0 outside the slot's steps and in
            // states >= N)
#pragma unroll
            for (int k = kChunk - 1; k >= 0; --k) {
                const int t = t0 + k;
                const bool act = t < T;
                const double bn = trans_dot<GV, LR, false>(bnext * beta, c, lane, a.N);
                const double bs = pow2_scale(bn, group_exp<GV>(bn));
                beta = act ? (t == T - 1 ? 1.0 : bs) : beta;
                bnext = act ? bv[k] : bnext;
                av[k] *= beta;
            }
            // off the chain, eight independent rows: the normalisation, the store and the arg-max
#pragma unroll
            for (int k = kChunk - 1; k >= 0; --k) {
                const int t = t0 + k;
                const bool act = t < T;
                const double p = av[k];
                const double sum = gsum<GV>(p);  // the same bits in every lane of the group
                const double g = !dead && sum > 0.0 ? p / sum : 0.0;
                if (act && mine) gam[(long long)t * a.N] = g;
                if (a.path) {
                    // the smallest state attaining the largest gamma_t; every lane of the group gets it
                    double v = g;
                    int st = j;
#pragma unroll
                    for (int m = 1; m < GV; m <<= 1) {
                        const double ov = __shfl_xor(v, m, GV);
                        const int oi = __shfl_xor(st, m, GV);
                        if (ov > v || (ov == v && oi < st)) {
                            v = ov;
                            st = oi;
                        }
                    }
                    if (act && seq >= 0 && j == 0) a.path[out + t] = dead ? -1 : st;
                }
            }
        }
    }
}

using PostFn = void (*)(PArgs);

template <int GV, bool LR>
static PostFn post_kernel2(bool full, bool lds) {
    if (full) return lds ? k_posterior<GV, LR, true, true> : k_posterior<GV, LR, true, false>;
    return lds ? k_posterior<GV, LR, false, true> : k_posterior<GV, LR, false, false>;
}

static PostFn post_kernel(int GV, bool lr, bool full, bool lds) {
    switch (GV) {
        case 8: return lr ? post_kernel2<8, true>(full, lds) : post_kernel2<8, false>(full, lds);
        case 16: return lr ? post_kernel2<16, true>(full, lds) : post_kernel2<16, false>(full, lds);
        case 32: return post_kernel2<32, false>(full, lds);
        default: return post_kernel2<64, false>(full, lds);
    }
}

void posterior_free(hmmbw_ctx *c) {
    hmmbw_ctx::Posterior &p = c->post;
    dfree(p.d_tab); dfree(p.d_scratch); dfree(p.d_path);
}

}  // namespace hmmbw

extern "C" int hmmbw_posterior(hmmbw_ctx *c, double *gamma_dev, int64_t gamma_len, int32_t *path_out, int64_t path_len,
                               double *logp_out) {
    if (int rc = check_ready(c, false)) return rc;
    if (!gamma_dev && !path_out && !logp_out) return fail(HMMBW_E_INVALID, "no output asked for");
    if (int rc = check_closed(c)) return rc;
    long long total = 0;
    if (int rc = check_path_len(c, path_len, &total)) return rc;
    if (gamma_len != total * c->N)
        return fail(HMMBW_E_INVALID, "gamma_len " + std::to_string(gamma_len) + " is not the number of loaded symbols x N (" +
                                         std::to_string(total * c->N) + ")");
    if (int rc = flush_mstep(c)) return rc;
    if (c->R == 0) return HMMBW_OK;
    if (int rc = viterbi_plan_ready(c)) return rc;
    const ViterbiPlan &P = c->vit.plan;
    hmmbw_ctx::Posterior &p = c->post;
    const bool path = path_out != nullptr, full = gamma_dev || path;
    const long long ntab = P.GV + (long long)P.GV * P.GV + (long long)c->K * P.GV;
    if (!p.d_tab)
        if (int rc = dalloc(&p.d_tab, (size_t)ntab)) return rc;
    if (full && !gamma_dev && !p.d_scratch)
        if (int rc = dalloc(&p.d_scratch, (size_t)(total * c->N)))
            return fail(rc, "the posterior workspace (" + std::to_string(total * c->N * 8) + " bytes) does not fit: " + g_err);
    if (path && !p.d_path)
        if (int rc = dalloc(&p.d_path, (size_t)total)) return rc;
    hipLaunchKernelGGL(k_posterior_prep, dim3((unsigned)std::min<long long>((ntab + 255) / 256, 1024)), dim3(256), 0,
                       c->stream, c->d_pi, c->d_A, c->d_B, c->N, c->K, P.GV, p.d_tab);
    HIP_TRY(hipGetLastError());
    PArgs a{};
    fill_slot_args(c, a);
    a.slot_out = c->vit.d_slot_out;
    a.tab = p.d_tab;
    a.gamma = full ? (gamma_dev ? gamma_dev : p.d_scratch) : nullptr;
    a.logp = c->vit.d_logp;
    a.path = path ? p.d_path : nullptr;
    a.N = c->N;
    const bool lds = viterbi_table_in_lds(c->K, P.GV);
    const bool lr = c->topo == HMMBW_TOPOLOGY_LEFT_TO_RIGHT && P.GV <= 16;
    const PostFn fn = post_kernel(P.GV, lr, full, lds);
    constexpr int wpb = kVitBlock / kVitWave;
    hipLaunchKernelGGL(fn, dim3((unsigned)((P.nvw + wpb - 1) / wpb)), dim3(kVitBlock),
                       lds ? viterbi_table_bytes(c->K, P.GV) : 0, c->stream, a);
    HIP_TRY(hipGetLastError());
    if (logp_out)
        HIP_TRY(hipMemcpyAsync(logp_out, c->vit.d_logp, sizeof(double) * (size_t)c->R, hipMemcpyDeviceToHost, c->stream));
    if (path)
        HIP_TRY(hipMemcpyAsync(path_out, p.d_path, sizeof(int32_t) * (size_t)total, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return HMMBW_OK;
}
