// viterbi.hip — Viterbi decoding (hmmbw_viterbi, include/hmmbw.h) for gfx950: the most likely state path of
// every loaded sequence and its log-probability, under the context's current parameters.
//
// Log domain, fp64, no rescaling:
//   delta_0(j) = log pi_j + log b_j(o_0)
//   delta_t(j) = max_i (delta_{t-1}(i) + log a_ij) + log b_j(o_t),   psi_t(j) = the smallest i attaining the max
// log 0 = -inf; no +inf ever occurs, so -inf + x never makes a NaN and a -inf candidate never beats a finite one.
//
// k_viterbi_prep builds the log tables from the linear working parameters once per call.  k_viterbi gives
// every sequence a group of GV lanes (viterbi_plan.hpp: 8, 16, 32 or 64), lane j = state j, and reads the
// symbols from the context's own packs (obs_plan.hpp): decoding wave v holds the 64 / GV consecutive layout slots
// from v * 64 / GV, slot s lives in layout wave s / U at u = s % U.  Lane j keeps its column of log A in
// registers; the candidates delta(i) come from cross-lane reads inside the group (DPP up to 16 lanes,
// v_readlane for 32 and 64), scanned from i = 0 with a strict '>'.  Left-to-right models compare only
// i = j - 1 (one row_shr:1) and i = j.  With paths, psi_t goes to HBM as one byte per (step, lane), a
// coalesced 64-B row per step; the backtrace runs in the same kernel and loads eight rows at a time (their
// addresses do not depend on the path, lane j holds psi_t(j)), so the dependent step is a cross-lane pick
// s_{t-1} = psi_t[lane s_t], never a memory access.
#include "word_units.hpp"  // fill_slot_args, check_path_len

namespace hmmbw {

struct VArgs {
    const uint16_t *sym;
    const long long *wave_symoff;
    const int *slot_len, *slot_seq;
    const long long *slot_out, *psi_off;
    const double *tab;   // [GV] log pi | [GV][GV] log A, tab[GV + j GV + i] = log a_ij | [K][GV] log B^T
    unsigned char *psi;
    double *logp;
    int32_t *path;
    long long nslots;
    int U, N, K;
    int shift;           // pack entry -> symbol: >> shift, or / div when shift < 0
    int div;
};

// tab from the linear parameters (pi [N], A [N][N] row-major, B [N][K]); states >= N are -inf
__global__ void __launch_bounds__(256) k_viterbi_prep(const double *__restrict__ pi, const double *__restrict__ A,
                                                      const double *__restrict__ B, int N, int K, int GV,
                                                      double *__restrict__ tab) {
    const long long nA = (long long)GV * GV, n = GV + nA + (long long)K * GV;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        double v = 0.0;  // log 0 = -inf below
        if (e < GV) {
            if (e < N) v = pi[e];
        } else if (e < GV + nA) {
            const int j = (int)((e - GV) / GV), i = (int)((e - GV) % GV);
            if (i < N && j < N) v = A[i * N + j];
        } else {
            const long long k = (e - GV - nA) / GV;
            const int j = (int)((e - GV - nA) % GV);
            if (j < N) v = B[(long long)j * K + k];
        }
        tab[e] = log(v);
    }
}

// max of two doubles that are never NaN: the one instruction (fmax adds a canonicalising v_max_f64 of its own)
__device__ __forceinline__ double vmax_f64(double a, double b) {
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

template <int GV, bool LR, bool PATH, bool LDSTAB>
__global__ void __launch_bounds__(kVitBlock) k_viterbi(VArgs a) {
    static_assert(!LR || GV <= 16, "left-to-right: one row_shr:1 inside a 16-lane row");
    extern __shared__ double sB[];  // LDSTAB: log B^T [K][GV]
    constexpr int SPW = kVitWave / GV;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int j = lane & (GV - 1);
    const double *tabB = a.tab + GV + GV * GV;
    if constexpr (LDSTAB) {
        for (int i = threadIdx.x; i < a.K * GV; i += kVitBlock) sB[i] = tabB[i];
        __syncthreads();
    }
    const double *lbt = LDSTAB ? sB : tabB;

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
    double la[LR ? 2 : GV];  // LR: log a_{j-1,j}, log a_jj | dense: log a_ij, i = 0 ..
    if constexpr (LR) {
        la[0] = j > 0 ? a.tab[GV + j * GV + j - 1] : -INFINITY;
        la[1] = a.tab[GV + j * GV + j];
    } else {
#pragma unroll
        for (int i = 0; i < GV; ++i) la[i] = a.tab[GV + j * GV + i];
    }
    const double lpi = a.tab[j];
    unsigned char *psi = nullptr;
    if constexpr (PATH) psi = a.psi + a.psi_off[vw] * kVitWave + lane;

    double delta = -INFINITY;  // delta_{T-1} once the slot's steps are done
    for (int t0 = 0; t0 < Tw; t0 += kChunk) {
        uint4 q = make_uint4(0, 0, 0, 0);
        if (t0 < T) q = pk[(long long)(t0 / kChunk) * a.U];
        const unsigned qw[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < kChunk; ++k) {
            const int t = t0 + k;
            const unsigned e = (k & 1) ? qw[k >> 1] >> 16 : qw[k >> 1] & 0xffffu;
            const unsigned o = a.shift >= 0 ? e >> a.shift : e / (unsigned)a.div;
            const double lb = lbt[(size_t)o * GV + j];  // symbol 0's row past the slot's end (unused)
            double best;
            int arg = 0;
            if (t == 0) {
                best = lpi;
            } else if constexpr (LR) {
                best = dpp<0x111>(delta) + la[0];  // row_shr:1: delta(j - 1); la[0] = -inf in lane 0 of a group
                arg = j > 0 ? j - 1 : 0;
                const double self = delta + la[1];
                if (self > best) {
                    best = self;
                    arg = j;
                }
            } else {
                // straight-line blocks of up to 16 candidates; a block wholly past N is skipped (wave-uniform), the
                // padded candidates of a block are -inf + -inf and never win
                constexpr int BLK = GV < 16 ? GV : 16;
                best = gbcast_wide<GV,0>(delta, lane) + la[0];
                sfor<0, GV / BLK>([&](auto Bk) {
                    constexpr int b = decltype(Bk)::value;
                    if (b == 0 || b * BLK < a.N) {
                        sfor<(b == 0 ? 1 : b * BLK), (b + 1) * BLK>([&](auto I) {
                            const double c = gbcast_wide<GV,I>(delta, lane) + la[I];
                            arg = c > best ? (int)I : arg;
                            best = vmax_f64(best, c);
                        });
                    }
                });
            }
            if (t < T) {
                delta = best + lb;
                if constexpr (PATH) psi[(long long)t * kVitWave] = (unsigned char)arg;
            }
        }
    }

    // the end state: the smallest j attaining the largest delta_{T-1}(j); every lane of the group gets it
    double v = delta;
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
    if (seq >= 0 && j == 0) a.logp[seq] = v;

    if constexpr (PATH) {
        const bool valid = v > -INFINITY;
        int32_t *out = a.path + (seq >= 0 ? a.slot_out[s] : 0);
        for (int t0 = (Tw - 1) / kChunk * kChunk; t0 >= 0; t0 -= kChunk) {
            int p[kChunk];
#pragma unroll
            for (int k = 0; k < kChunk; ++k) p[k] = t0 + k < T ? (int)psi[(long long)(t0 + k) * kVitWave] : 0;
            int w = -1;  // lane k of the group writes step t0 + k
#pragma unroll
            for (int k = kChunk - 1; k >= 0; --k) {
                const int prev = __shfl(p[k], st, GV);  // psi_t(s_t)
                if (t0 + k < T) {
                    if (j == k) w = st;
                    st = prev;
                }
            }
            if (seq >= 0 && j < kChunk && t0 + j < T) out[t0 + j] = valid ? w : -1;
        }
    }
}

using VitFn = void (*)(VArgs);

template <int GV, bool LR>
static VitFn vit_kernel2(bool path, bool lds) {
    if (path) return lds ? k_viterbi<GV, LR, true, true> : k_viterbi<GV, LR, true, false>;
    return lds ? k_viterbi<GV, LR, false, true> : k_viterbi<GV, LR, false, false>;
}

static VitFn vit_kernel(int GV, bool lr, bool path, bool lds) {
    switch (GV) {
        case 8: return lr ? vit_kernel2<8, true>(path, lds) : vit_kernel2<8, false>(path, lds);
        case 16: return lr ? vit_kernel2<16, true>(path, lds) : vit_kernel2<16, false>(path, lds);
        case 32: return vit_kernel2<32, false>(path, lds);
        default: return vit_kernel2<64, false>(path, lds);
    }
}

void viterbi_free(hmmbw_ctx *c) {
    hmmbw_ctx::Viterbi &v = c->vit;
    dfree(v.d_tab); dfree(v.d_slot_out); dfree(v.d_psi_off); dfree(v.d_logp); dfree(v.d_path); dfree(v.d_psi);
    v.planned = false;
    v.plan = ViterbiPlan{};
}

// the plan of the loaded observations with its offsets on the device, the log tables and the device logp: made
// by the first decode or the first hmmbw_posterior (posterior.hip shares the plan, the offsets and the logp)
int viterbi_plan_ready(hmmbw_ctx *c) {
    hmmbw_ctx::Viterbi &v = c->vit;
    if (!v.planned) {
        viterbi_free(c);  // what a failed earlier attempt left
        ViterbiPlan P =plan_viterbi(c->h_slen, c->h_sseq, c->R, c->N);
        const size_t ntab = (size_t)P.GV + (size_t)P.GV * P.GV + (size_t)c->K * P.GV;
        int rc = dalloc(&v.d_tab, ntab);
        if (!rc) rc = dalloc(&v.d_slot_out, P.slot_out.size());
        if (!rc) rc = dalloc(&v.d_psi_off, P.psi_off.size());
        if (!rc) rc = dalloc(&v.d_logp, (size_t)c->R);
        if (!rc && !P.slot_out.empty())
            HIP_TRY(hipMemcpy(v.d_slot_out, P.slot_out.data(), sizeof(long long) * P.slot_out.size(), hipMemcpyHostToDevice));
        if (!rc && !P.psi_off.empty())
            HIP_TRY(hipMemcpy(v.d_psi_off, P.psi_off.data(), sizeof(long long) * P.psi_off.size(), hipMemcpyHostToDevice));
        if (rc) {
            viterbi_free(c);
            return rc;
        }
        P.slot_out = std::vector<long long>();
        P.psi_off = std::vector<long long>();
        v.plan = P;
        v.planned = true;
    }
    return HMMBW_OK;
}

// the decoder's buffers for the loaded observations: the plan on the first decode, the path and the
// back-pointers on the first decode with paths
static int viterbi_buffers(hmmbw_ctx *c, bool path) {
    if (int rc = viterbi_plan_ready(c)) return rc;
    hmmbw_ctx::Viterbi &v = c->vit;
    if (path && !v.d_path) {
        int rc = dalloc(&v.d_path, (size_t)v.plan.total);
        if (!rc) rc = dalloc(&v.d_psi, (size_t)v.plan.psi_rows * kVitWave);
        if (rc) {
            dfree(v.d_path);
            dfree(v.d_psi);
            return fail(rc, "the Viterbi back-pointers (" + std::to_string(v.plan.psi_rows * kVitWave) +
                                " bytes) do not fit: " + g_err);
        }
    }
    return HMMBW_OK;
}

}  // namespace hmmbw

extern "C" int hmmbw_viterbi(hmmbw_ctx *c, double *logp_out, int32_t *path_out, int64_t path_len) {
    if (int rc = check_ready(c, false)) return rc;
    if (!logp_out) return fail(HMMBW_E_INVALID, "null argument");
    if (int rc = check_closed(c)) return rc;
    long long total = 0;
    if (int rc = check_path_len(c, path_len, &total)) return rc;
    if (int rc = flush_mstep(c)) return rc;
    if (c->R == 0) return HMMBW_OK;
    const bool path = path_out != nullptr;
    if (int rc = viterbi_buffers(c, path)) return rc;
    hmmbw_ctx::Viterbi &v = c->vit;
    const ViterbiPlan &P = v.plan;
    const long long ntab = P.GV + (long long)P.GV * P.GV + (long long)c->K * P.GV;
    hipLaunchKernelGGL(k_viterbi_prep, dim3((unsigned)std::min<long long>((ntab + 255) / 256, 1024)), dim3(256), 0,
                       c->stream, c->d_pi, c->d_A, c->d_B, c->N, c->K, P.GV, v.d_tab);
    HIP_TRY(hipGetLastError());
    VArgs a{};
    fill_slot_args(c, a);
    a.slot_out = v.d_slot_out;
    a.psi_off = v.d_psi_off;
    a.tab = v.d_tab;
    a.psi = path ? v.d_psi : nullptr;
    a.logp = v.d_logp;
    a.path = path ? v.d_path : nullptr;
    a.N = c->N;
    const bool lds = viterbi_table_in_lds(c->K, P.GV);
    const bool lr = c->topo == HMMBW_TOPOLOGY_LEFT_TO_RIGHT && P.GV <= 16;
    const VitFn fn = vit_kernel(P.GV, lr, path, lds);
    constexpr int wpb = kVitBlock / kVitWave;
    hipLaunchKernelGGL(fn, dim3((unsigned)((P.nvw + wpb - 1) / wpb)), dim3(kVitBlock),
                       lds ? viterbi_table_bytes(c->K, P.GV) : 0, c->stream, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(logp_out, v.d_logp, sizeof(double) * (size_t)c->R, hipMemcpyDeviceToHost, c->stream));
    if (path && total > 0)
        HIP_TRY(hipMemcpyAsync(path_out, v.d_path, sizeof(int32_t) * (size_t)total, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return HMMBW_OK;
}
