// wordnet.hip — connected-word decoding (hmmbw_wordnet_decode, include/hmmbw.h) for gfx950: the Viterbi path of
// every loaded sequence through a loop of W word models (a bank: pi [W][N], A [W][N][N], B [W][N][K], word
// weights init [W], word-transition weights G [W][W]), its log-probability and the frames at which a word starts.
//
// Log domain, fp64, no rescaling; composite state (w, j) has index w N + j:
//   delta_0(w,j) = (log init_w + log pi_w[j]) + log b_w,j(o_0)
//   inner_t(w,j) = max_i delta_{t-1}(w,i) + log a_w[i][j]          the smallest i on ties
//   E_t(w)       = max_v delta_{t-1}(v,N-1) + log G[v][w]          the smallest v on ties
//   entry_t(w,j) = E_t(w) + log pi_w[j]
//   delta_t(w,j) = (entry_t > inner_t ? entry_t : inner_t) + log b_w,j(o_t)     the within-word arc wins ties
// log 0 = -inf; no +inf ever occurs, so -inf + x never makes a NaN and a -inf candidate never beats a finite one.
//
// k_wordnet_prep builds the log tables (wordnet_plan.hpp, WordnetTab) from the staged linear bank once per call.
// k_wordnet gives every sequence a group of GW lanes (8, 16, 32 or 64), lane w = word w, and reads the symbols
// from the context's own packs exactly as k_viterbi does (d_sym, viterbi_pack_div): decoding wave v holds the
// 64 / GW consecutive layout slots from v * 64 / GW.  The lane keeps its word's N deltas, its log pi and its
// log A (2 values per state for left-to-right banks, N^2 for dense ones) in registers, so the within-word step
// needs no cross-lane traffic.  The only cross-lane work of a step is E_t(w): without word_trans one group
// max-with-lowest-index reduction of delta(v, N-1); with it a scan of the W broadcasts from v = 0 with a strict
// '>', the lane holding its column of log G (blocks of 16 candidates wholly past W are skipped).  The emissions
// of the next step are loaded while the current step computes (their addresses depend on the symbols alone).
// With paths, a step's back-pointers go to HBM as 4 bytes per lane (a nibble per state: the within-word
// predecessor and the entry-arc bit) and 1 byte per lane (the entry source v), coalesced rows per step and
// wave; the backtrace runs in the same kernel and loads eight steps' rows at a time (their addresses do not
// depend on the path), so the dependent step is a cross-lane pick from lane w, never a memory access.
#include "word_units.hpp"

namespace hmmbw {

struct WArgs {
    const uint16_t *sym;
    const long long *wave_symoff;
    const int *slot_len, *slot_seq;
    const long long *slot_out, *psi_off;
    const double *tab;   // WordnetTab
    unsigned char *bp;   // [row][kWnRowBytes]
    double *logp;
    int32_t *path;
    unsigned char *start;
    long long nslots;
    long long o_init, o_A, o_G, o_B;  // WordnetTab offsets (pi is at 0)
    int U, W, K;
    int shift;           // pack entry -> symbol: >> shift, or / div when shift < 0
    int div;
    int lds;             // the emission table is copied to LDS
    int end_final;       // only the states (w, N - 1) compete for the end
};

// in: pi [W][N] | A [W][N][N] | B [W][N][K] | init [W] | G [W][W]
__global__ void __launch_bounds__(256) k_wordnet_prep(const double *__restrict__ in, int W, int N, int K, int GW,
                                                      WordnetTab o, double *__restrict__ tab) {
    const int NP = wordnet_np(N);
    const double *pi = in, *A = pi + (long long)W * N, *B = A + (long long)W * N * N;
    const double *init = B + (long long)W * N * K, *G = init + W;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < o.total; e += (long long)gridDim.x * blockDim.x) {
        double v = 0.0;  // log 0 = -inf below
        if (e < o.init) {
            const int w = (int)(e / NP), j = (int)(e % NP);
            if (w < W && j < N) v = pi[w * N + j];
        } else if (e < o.A) {
            const int w = (int)(e - o.init);
            if (w < W) v = init[w];
        } else if (e < o.G) {
            const long long x = e - o.A;
            if (x / (N * N) < W) v = A[x];
        } else if (e < o.B) {
            const long long x = e - o.G;
            const int w = (int)(x / GW), u = (int)(x % GW);
            if (x < (long long)GW * GW && w < W && u < W) v = G[(long long)u * W + w];
        } else {
            const long long x = e - o.B;
            const long long k = x / ((long long)GW * NP);
            const int w = (int)(x / NP % GW), j = (int)(x % NP);
            if (w < W && j < N) v = B[((long long)w * N + j) * K + k];
        }
        tab[e] = log(v);
    }
}

// the larger of the group's (v, i) pairs, the smaller i on ties; complete and identical in every lane of the group
template <int G>
__device__ __forceinline__ void gmax_idx(double &v, int &i) {
    auto take = [&](double ov, int oi) {
        const bool t = ov > v || (ov == v && oi < i);
        v = t ? ov : v;
        i = t ? oi : i;
    };
    take(dpp<0xB1>(v), dpp_i32<0xB1>(i));    // quad_perm [1,0,3,2]
    take(dpp<0x4E>(v), dpp_i32<0x4E>(i));    // quad_perm [2,3,0,1]
    take(dpp<0x141>(v), dpp_i32<0x141>(i));  // row_half_mirror
    if constexpr (G >= 16) take(dpp<0x140>(v), dpp_i32<0x140>(i));  // row_mirror
    if constexpr (G >= 32) take(__shfl_xor(v, 16), __shfl_xor(i, 16));
    if constexpr (G >= 64) take(__shfl_xor(v, 32), __shfl_xor(i, 32));
}

template <int GW, int N, bool LR, bool GRAM, bool PATH>
__global__ void __launch_bounds__(kVitBlock) k_wordnet(WArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sB[];  // a.lds: log B [K][GW][NP]
    constexpr int NP = wordnet_np(N);
    constexpr int SPW = kVitWave / GW;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int w = lane & (GW - 1);
    const double *tabB = a.tab + a.o_B;
    if (a.lds) {
        for (int i = threadIdx.x; i < a.K * GW * NP; i += kVitBlock) sB[i] = tabB[i];
        __syncthreads();
    }
    const double *lbt = (a.lds ? sB : tabB) + w * NP;

    const long long vw = (long long)blockIdx.x * (kVitBlock / kVitWave) + wv;
    const long long s = vw * SPW + lane / GW;
    const bool real = s < a.nslots;
    const int T = real ? a.slot_len[s] : 0;     // 0 in padding slots
    const int seq = real ? a.slot_seq[s] : -1;  // -1 in padding slots
    int Tw = T;  // the wave's longest sequence
#pragma unroll
    for (int m = GW; m < kVitWave; m <<= 1) Tw = max(Tw, __shfl_xor(Tw, m));
    if (Tw == 0) return;

    // chunk c of the slot: 8 steps in one 16-B load, U loads further on per chunk (pack_pos)
    const uint4 *pk = reinterpret_cast<const uint4 *>(a.sym) +
                      (real ? pack_pos(a.wave_symoff[s / a.U], a.U, (int)(s % a.U), 0) / kChunk : 0);
    auto chunk = [&](int t0) {
        uint4 q = make_uint4(0, 0, 0, 0);
        if (t0 < T) q = pk[(long long)(t0 / kChunk) * a.U];
        return q;
    };
    auto row_of = [&](unsigned e) {  // symbol 0's row past the slot's end (unused)
        const unsigned o = a.shift >= 0 ? e >> a.shift : e / (unsigned)a.div;
        return lbt + (size_t)o * (GW * NP);
    };

    double la[LR ? 2 * N : N * N];  // LR: log a_{j-1,j}, log a_jj per state j | dense: log a_ij row-major
    {
        const double *tA = a.tab + a.o_A + (long long)w * N * N;
        if constexpr (LR) {
#pragma unroll
            for (int j = 0; j < N; ++j) {
                la[2 * j] = j > 0 ? tA[(j - 1) * N + j] : -INFINITY;
                la[2 * j + 1] = tA[j * N + j];
            }
        } else {
#pragma unroll
            for (int i = 0; i < N * N; ++i) la[i] = tA[i];
        }
    }
    double lpi[N];
    load_row<N>(a.tab + w * NP, lpi);
    const double linit = a.tab[a.o_init + w];
    double lg[GRAM ? GW : 1];  // log G[v][w], v = 0 ..
    if constexpr (GRAM) {
#pragma unroll
        for (int v = 0; v < GW; ++v) lg[v] = a.tab[a.o_G + (long long)w * GW + v];
    }
    unsigned char *bp = nullptr;
    if constexpr (PATH) bp = a.bp + a.psi_off[vw] * kWnRowBytes;

    double d[N];  // delta_{T-1}(w, .) once the slot's steps are done
#pragma unroll
    for (int j = 0; j < N; ++j) d[j] = -INFINITY;

    uint4 qn = chunk(0);
    double lbn[N];  // the next step's emissions
    load_row<N>(row_of(qn.x & 0xffffu), lbn);
    for (int t0 = 0; t0 < Tw; t0 += kChunk) {
        const uint4 q = qn;
        qn = chunk(t0 + kChunk);
        const unsigned long long qlo = q.x | (unsigned long long)q.y << 32, qhi = q.z | (unsigned long long)q.w << 32;
#pragma nounroll
        for (int k = 0; k < kChunk; ++k) {
            const int t = t0 + k;
            double lb[N];
#pragma unroll
            for (int j = 0; j < N; ++j) lb[j] = lbn[j];
            {
                const int kn = k + 1;
                const unsigned long long word = kn < 4 ? qlo : kn < 8 ? qhi : (unsigned long long)qn.x;
                load_row<N>(row_of((unsigned)(word >> (16 * (kn & 3))) & 0xffffu), lbn);
            }
            double nd[N];
            unsigned nib = 0;
            int ev = 0;
            if (t == 0) {
#pragma unroll
                for (int j = 0; j < N; ++j) nd[j] = (linit + lpi[j]) + lb[j];
            } else {
                const double last = d[N - 1];
                double E;
                if constexpr (GRAM) {
                    // straight-line blocks of up to 16 candidates; a block wholly past W is skipped (wave-uniform),
                    // the padded candidates of a block are -inf + -inf and never win
                    constexpr int BLK = GW < 16 ? GW : 16;
                    E = gbcast_wide<GW, 0>(last, lane) + lg[0];
                    sfor<0, GW / BLK>([&](auto Bk) {
                        constexpr int b = decltype(Bk)::value;
                        if (b == 0 || b * BLK < a.W) {
                            sfor<(b == 0 ? 1 : b * BLK), (b + 1) * BLK>([&](auto I) {
                                const double c = gbcast_wide<GW, I>(last, lane) + lg[I];
                                ev = c > E ? (int)I : ev;
                                E = c > E ? c : E;
                            });
                        }
                    });
                } else {
                    E = last;
                    ev = w;
                    gmax_idx<GW>(E, ev);
                }
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    double best;
                    int arg;
                    if constexpr (LR) {
                        best = d[j > 0 ? j - 1 : 0] + la[2 * j];  // la[0] = -inf
                        arg = j > 0 ? j - 1 : 0;
                        const double self = d[j] + la[2 * j + 1];
                        arg = self > best ? j : arg;
                        best = self > best ? self : best;
                    } else {
                        best = d[0] + la[j];
                        arg = 0;
#pragma unroll
                        for (int i = 1; i < N; ++i) {
                            const double c = d[i] + la[i * N + j];
                            arg = c > best ? i : arg;
                            best = c > best ? c : best;
                        }
                    }
                    const double entry = E + lpi[j];
                    const bool in = entry > best;
                    nd[j] = (in ? entry : best) + lb[j];
                    nib |= (unsigned)(arg | (in ? 8 : 0)) << (4 * j);
                }
            }
            if (t < T) {
#pragma unroll
                for (int j = 0; j < N; ++j) d[j] = nd[j];
                if constexpr (PATH) {
                    unsigned char *row = bp + (long long)t * kWnRowBytes;
                    reinterpret_cast<unsigned *>(row)[lane] = nib;
                    row[kVitWave * 4 + lane] = (unsigned char)ev;
                }
            }
        }
    }

    // the end state: the smallest composite index attaining the largest delta_{T-1}; every lane of the group gets it
    double v = d[N - 1];
    int st = w * N + N - 1;
    if (!a.end_final) {
        v = d[0];
        st = w * N;
#pragma unroll
        for (int j = 1; j < N; ++j) {
            st = d[j] > v ? w * N + j : st;
            v = d[j] > v ? d[j] : v;
        }
    }
    gmax_idx<GW>(v, st);
    if (seq >= 0 && w == 0) a.logp[seq] = v;

    if constexpr (PATH) {
        const bool valid = v > -INFINITY;
        const long long out = seq >= 0 ? a.slot_out[s] : 0;
        int cw = st / N, cj = st % N;
        for (int t0 = (Tw - 1) / kChunk * kChunk; t0 >= 0; t0 -= kChunk) {
            unsigned p[kChunk];
            int pe[kChunk];
#pragma unroll
            for (int k = 0; k < kChunk; ++k) {
                const unsigned char *row = bp + (long long)(t0 + k) * kWnRowBytes;
                p[k] = t0 + k < T ? reinterpret_cast<const unsigned *>(row)[lane] : 0u;
                pe[k] = t0 + k < T ? (int)row[kVitWave * 4 + lane] : 0;
            }
            int ws = -1, wf = 0;  // lane k of the group writes step t0 + k
#pragma unroll
            for (int k = kChunk - 1; k >= 0; --k) {
                const unsigned pw = (unsigned)__shfl((int)p[k], cw, GW);  // the back-pointers of word cw
                const int pv = __shfl(pe[k], cw, GW);
                if (t0 + k < T) {
                    const unsigned nb = (pw >> (4 * cj)) & 15u;
                    const bool in = (nb & 8u) != 0;  // never set at t = 0
                    if (w == k) {
                        ws = cw * N + cj;
                        wf = (in || t0 + k == 0) ? 1 : 0;
                    }
                    cj = in ? N - 1 : (int)(nb & 7u);
                    cw = in ? pv : cw;
                }
            }
            if (seq >= 0 && w < kChunk && t0 + w < T) {
                a.path[out + t0 + w] = valid ? ws : -1;
                a.start[out + t0 + w] = (unsigned char)(valid ? wf : 0);
            }
        }
    }
}

using WnFn = void (*)(WArgs);

static WnFn wn_kernel(int GW, int N, bool lr, bool gram, bool path) {
    return pick_gw_n(GW, N, [=](auto gw, auto n) -> WnFn {
        constexpr int G = decltype(gw)::value, S = decltype(n)::value;
        if (lr) {
            if (gram) return path ? k_wordnet<G, S, true, true, true> : k_wordnet<G, S, true, true, false>;
            return path ? k_wordnet<G, S, true, false, true> : k_wordnet<G, S, true, false, false>;
        }
        if (gram) return path ? k_wordnet<G, S, false, true, true> : k_wordnet<G, S, false, true, false>;
        return path ? k_wordnet<G, S, false, false, true> : k_wordnet<G, S, false, false, false>;
    });
}

void wordnet_free(hmmbw_ctx *c) {
    hmmbw_ctx::Wordnet &n = c->wn;
    dfree(n.d_psi_off); dfree(n.d_in); dfree(n.d_tab); dfree(n.d_path); dfree(n.d_start); dfree(n.d_bp);
    n = hmmbw_ctx::Wordnet{};
}

// the decoder's buffers for the loaded observations and this bank shape: what word_decode_buffers keeps, and
// with paths the path, the start flags and the back-pointers
static int wordnet_buffers(hmmbw_ctx *c, int GW, size_t n_in, size_t n_tab, bool path) {
    hmmbw_ctx::Wordnet &n = c->wn;
    if (int rc = word_decode_buffers(c, n, GW, n_in, n_tab)) return rc;
    if (path) {
        const long long total = c->vit.plan.total;
        int rc = HMMBW_OK;
        if (!n.d_path) rc = dalloc(&n.d_path, (size_t)total);
        if (!rc && !n.d_start) rc = dalloc(&n.d_start, (size_t)total);
        if (!rc && !n.d_bp) rc = dalloc(&n.d_bp, (size_t)n.rows * kWnRowBytes);
        if (rc) {  // none of the three is kept: the next call with paths allocates them again
            sync_ctx(c);
            dfree(n.d_path);
            dfree(n.d_start);
            dfree(n.d_bp);
            return fail(rc, "the word-loop back-pointers (" + std::to_string(n.rows * kWnRowBytes) +
                                " bytes) do not fit: " + g_err);
        }
    }
    return HMMBW_OK;
}

}  // namespace hmmbw

extern "C" int hmmbw_wordnet_decode(hmmbw_ctx *c, int n_words, const double *pi, const double *A, const double *B,
                                    const double *word_init, const double *word_trans, int flags, double *logp_out,
                                    int32_t *path_out, uint8_t *start_out, int64_t path_len) {
    if (!c) return fail(HMMBW_E_INVALID, "null context");
    if (!c->has_obs) return fail(HMMBW_E_STATE, "observations not set");
    if (int rc = set_device(c)) return rc;
    if (!pi || !A || !B || !logp_out) return fail(HMMBW_E_INVALID, "null argument");
    if (start_out && !path_out) return fail(HMMBW_E_INVALID, "start_out needs path_out");
    if (flags & ~(HMMBW_WORDNET_END_FINAL | HMMBW_WORDNET_DENSE)) return fail(HMMBW_E_INVALID, "unknown flag");
    if (int rc = check_word_bank(c, n_words, pi, A, B, kWnMaxWords, kWnMaxStates, "a negative or NaN bank parameter"))
        return rc;
    const int W = n_words, N = c->N, K = c->K;
    if ((word_init && !wordnet_weights_ok(word_init, W)) || (word_trans && !wordnet_weights_ok(word_trans, (long long)W * W)))
        return fail(HMMBW_E_INVALID, "a negative or NaN word weight");
    if (int rc = check_closed(c)) return rc;
    long long total = 0;
    if (int rc = check_path_len(c, path_len, &total)) return rc;
    if (c->R == 0) return HMMBW_OK;

    const bool path = path_out != nullptr, gram = word_trans != nullptr;
    const bool lr = !(flags & HMMBW_WORDNET_DENSE) && wordnet_is_lr(A, W, N);
    const int GW = wordnet_gw(W);
    const WordnetTab o = wordnet_tab(GW, N, K);
    const long long n_in = wordnet_in_len(W, N, K);
    if (int rc = wordnet_buffers(c, GW, (size_t)n_in, (size_t)o.total, path)) return rc;
    hmmbw_ctx::Wordnet &n = c->wn;

    std::vector<double> h;
    if (int rc = stage_bank(n.d_in, h, n_in, pi, A, B, W, N, K, word_init, word_trans)) return rc;
    hipLaunchKernelGGL(k_wordnet_prep, dim3((unsigned)std::min<long long>((o.total + 255) / 256, 1024)), dim3(256), 0,
                       c->stream, n.d_in, W, N, K, GW, o, n.d_tab);
    HIP_TRY(hipGetLastError());

    WArgs a{};
    fill_slot_args(c, a);
    a.slot_out = c->vit.d_slot_out;
    a.psi_off = n.d_psi_off;
    a.tab = n.d_tab;
    a.bp = path ? n.d_bp : nullptr;
    a.logp = c->vit.d_logp;
    a.path = path ? n.d_path : nullptr;
    a.start = path ? n.d_start : nullptr;
    a.o_init = o.init;
    a.o_A = o.A;
    a.o_G = o.G;
    a.o_B = o.B;
    a.W = W;
    a.lds = wordnet_emis_in_lds(K, GW, N) ? 1 : 0;
    a.end_final = (flags & HMMBW_WORDNET_END_FINAL) ? 1 : 0;
    const WnFn fn = wn_kernel(GW, N, lr, gram, path);
    constexpr int wpb = kVitBlock / kVitWave;
    hipLaunchKernelGGL(fn, dim3((unsigned)((n.nvw + wpb - 1) / wpb)), dim3(kVitBlock),
                       a.lds ? wordnet_emis_bytes(K, GW, N) : 0, c->stream, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(logp_out, c->vit.d_logp, sizeof(double) * (size_t)c->R, hipMemcpyDeviceToHost, c->stream));
    if (path && total > 0) {
        HIP_TRY(hipMemcpyAsync(path_out, n.d_path, sizeof(int32_t) * (size_t)total, hipMemcpyDeviceToHost, c->stream));
        if (start_out)
            HIP_TRY(hipMemcpyAsync(start_out, n.d_start, (size_t)total, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return HMMBW_OK;
}
