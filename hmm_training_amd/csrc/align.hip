// align.hip — forced alignment (hmmbw_align, include/hmmbw.h) for gfx950: the Viterbi path of every loaded
// utterance through the chain of word models its transcript names (a bank: pi [W][N], A [W][N][N], B [W][N][K]; a
// transcript w_0 .. w_{L-1} of word ids), its log-probability and the frame at which every instance starts.  The
// hard-decision counterpart of embedded.hip's E-step on the same chain, with wordnet.hip's log-domain step,
// back-pointers and in-kernel backtrace.
//
// Log domain, fp64, no rescaling; composite state (l, j), l the transcript position, has index l N + j:
//   delta_0(0,j)  = log pi_{w_0}[j] + log b_{w_0,j}(o_0);   delta_0(l>0, .) = -inf
//   inner_t(l,j)  = max_i delta_{t-1}(l,i) + log a_{w_l}[i][j]       the smallest i on ties
//   entry_t(l,j)  = delta_{t-1}(l-1,N-1) + log pi_{w_l}[j]           -inf for l = 0
//   delta_t(l,j)  = (entry_t > inner_t ? entry_t : inner_t) + log b_{w_l,j}(o_t)     the within-word arc wins ties
// log 0 = -inf; no +inf ever occurs, so -inf + x never makes a NaN and a -inf candidate never beats a finite one.
//
// k_align_prep builds the log tables (align_plan.hpp: EmbedTab's layout) from the staged linear bank once per call,
// with the log of k_wordnet_prep.  k_align gives every utterance a group of GW lanes (8, 16, 32 or 64), lane l =
// transcript position l, and reads the symbols from the context's own packs as the two siblings do; a wave holds
// the 64 / GW consecutive layout slots.  The lane keeps its instance's N deltas, its word's log pi and log A (2
// values per state for left-to-right banks, N^2 for dense ones) in registers.  The only cross-lane work of a step is
// the left neighbour's delta(l-1, N-1), a one-lane shift: the entry source is fixed by the chain, so there is no
// max over words as in k_wordnet.  The emissions of the next step are loaded while the current step computes.
// With paths, a step's back-pointers go to HBM as 4 bytes per lane (a nibble per state: the within-word
// predecessor and the entry-arc bit), one coalesced 256-byte row per step and wave; the backtrace runs in the same
// kernel and loads eight steps' rows at a time, so the dependent step is a cross-lane pick from lane l, never a
// memory access.  Lanes past the transcript's end and padding slots hold -inf throughout and write nothing.
// hmmbw_align_optional runs the same kernel with OPT: a second entry source two lanes away past an optional
// position, and one more back-pointer bit per lane and step in a lane mask of its own (align_plan.hpp).
#include "word_units.hpp"
#include "align_plan.hpp"

namespace hmmbw {

struct AlArgs {
    const uint16_t *sym;
    const long long *wave_symoff;
    const int *slot_len, *slot_seq;
    const long long *slot_out, *psi_off;
    const long long *word_off;   // [R + 1] transcripts, CSR in caller order
    const int *word_ids;
    const double *tab;           // align_tab
    unsigned *bp;                // [row][64 lanes]
    double *logp;
    int32_t *path;
    int32_t *bounds;
    long long nslots;
    long long o_A, o_B;          // table offsets (pi is at 0)
    int U, W, K;
    int shift;                   // pack entry -> symbol: >> shift, or / div when shift < 0
    int div;
    int lds;                     // the emission table is copied to LDS
    int end_final;               // only (L - 1, N - 1) competes for the end
    const uint8_t *optional;     // OPT: a byte per transcript position, word_ids' order
    unsigned long long *skip;    // OPT, with paths: [row] the lanes whose entry source is two positions back
};

// in: pi [W][N] | A [W][N][N] | B [W][N][K]
__global__ void __launch_bounds__(256) k_align_prep(const double *__restrict__ in, int W, int N, int K, EmbedTab o,
                                                    double *__restrict__ tab) {
    const int NP = embed_np(N);
    const double *pi = in, *A = pi + (long long)W * N, *B = A + (long long)W * N * N;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < o.total; e += (long long)gridDim.x * blockDim.x)
        tab[e] = log(embed_bank_value(pi, A, B, W, N, NP, K, o, e));  // log 0 = -inf in the padding
}

// OPT (hmmbw_align_optional with flags): a position with opt = 1 may be passed over.  Position l is then also
// entered from (l - 2, N - 1) when l - 1 is optional, position 1 also starts a path when position 0 is optional,
// and a path also ends in L - 2 when L - 1 is optional; on a tie the path that skips less wins.  OPT = false is
// the kernel as it was.
template <int GW, int N, bool LR, bool PATH, bool OPT>
__global__ void __launch_bounds__(kVitBlock) k_align(AlArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sB[];  // a.lds: log B [K][W][NP]
    constexpr int NP = embed_np(N);
    constexpr int SPW = kVitWave / GW;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int l = lane & (GW - 1);
    const double *tabB = a.tab + a.o_B;
    if (a.lds) {
        for (int i = threadIdx.x; i < a.K * a.W * NP; i += kVitBlock) sB[i] = tabB[i];
        __syncthreads();
    }

    const long long vw = (long long)blockIdx.x * (kVitBlock / kVitWave) + wv;
    const long long s = vw * SPW + lane / GW;
    const bool real = s < a.nslots;
    const int T = real ? a.slot_len[s] : 0;     // 0 in padding slots
    const int seq = real ? a.slot_seq[s] : -1;  // -1 in padding slots
    int Tw = T;  // the wave's longest utterance
#pragma unroll
    for (int m = GW; m < kVitWave; m <<= 1) Tw = max(Tw, __shfl_xor(Tw, m));
    if (Tw == 0) return;

    // the lane's instance: position l of the utterance's transcript (lanes past its end hold -inf throughout)
    int Lw = 0;
    long long woff = 0;
    if (seq >= 0) {
        woff = a.word_off[seq];
        Lw = (int)(a.word_off[seq + 1] - woff);
    }
    const bool live = l < Lw;
    const int wid = live ? a.word_ids[woff + l] : 0;
    const size_t kstride = (size_t)a.W * NP, wrow = (size_t)wid * NP;
    const double *lbt = (a.lds ? sB : tabB) + wrow;
    [[maybe_unused]] bool over = false, start = false, tail_opt = false;  // OPT: l - 1 may be passed over; a path starts here
    if constexpr (OPT) {
        over = live && l >= 2 && a.optional[woff + l - 1] != 0;
        start = l == 0 || (live && l == 1 && a.optional[woff] != 0);
        tail_opt = Lw >= 2 && a.optional[woff + Lw - 1] != 0;
    }
    [[maybe_unused]] unsigned long long *skip = nullptr;
    if constexpr (OPT && PATH) skip = a.skip + a.psi_off[vw];  // row t: skip[t]

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
        return lbt + (size_t)o * kstride;
    };

    double la[LR ? 2 * N : N * N];  // LR: log a_{j-1,j}, log a_jj per state j | dense: log a_ij row-major
    {
        const double *tA = a.tab + a.o_A + (long long)wid * N * N;
        if constexpr (LR) {
#pragma unroll
            for (int j = 0; j < N; ++j) {
                la[2 * j] = live && j > 0 ? tA[(j - 1) * N + j] : -INFINITY;
                la[2 * j + 1] = live ? tA[j * N + j] : -INFINITY;
            }
        } else {
#pragma unroll
            for (int i = 0; i < N * N; ++i) la[i] = live ? tA[i] : -INFINITY;
        }
    }
    double lpi[N];
    load_row<N>(a.tab + wrow, lpi);
#pragma unroll
    for (int j = 0; j < N; ++j) lpi[j] = live ? lpi[j] : -INFINITY;
    unsigned *bp = nullptr;
    if constexpr (PATH) bp = a.bp + a.psi_off[vw] * kVitWave + lane;  // row t: bp[t * 64]

    double d[N];  // delta_{T-1}(l, .) once the slot's steps are done
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
            if (t == 0) {
#pragma unroll
                for (int j = 0; j < N; ++j) nd[j] = (OPT ? start : l == 0) ? lpi[j] + lb[j] : -INFINITY;
            } else {
                double left = from_left<GW>(d[N - 1], l, -INFINITY);
                if constexpr (OPT) {  // the source two positions back wins only if it is strictly better
                    const double left2 = from_left2<GW>(d[N - 1], over, -INFINITY);
                    if constexpr (PATH) {  // off the step's dependent chain
                        const unsigned long long m = __ballot(left2 > left);
                        if (lane == 0 && t < Tw) skip[t] = m;
                    }
                    left = fmax(left, left2);
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
                    const double entry = left + lpi[j];
                    const bool in = entry > best;
                    nd[j] = (in ? entry : best) + lb[j];
                    nib |= (unsigned)(arg | (in ? 8 : 0)) << (4 * j);
                }
            }
            if (t < T) {
#pragma unroll
                for (int j = 0; j < N; ++j) d[j] = nd[j];
                if constexpr (PATH) bp[(long long)t * kVitWave] = nib;
            }
        }
    }

    // the end state: the smallest j attaining the largest delta_{T-1}(L-1, j), found on lane L - 1 and broadcast
    double v = d[N - 1];
    int cj = N - 1;
    if (!a.end_final) {
        v = d[0];
        cj = 0;
#pragma unroll
        for (int j = 1; j < N; ++j) {
            cj = d[j] > v ? j : cj;
            v = d[j] > v ? d[j] : v;
        }
    }
    int tail = max(Lw - 1, 0);
    if constexpr (OPT) {  // an optional last position: L - 2 is an end too, and L - 1 wins ties
        const double v2 = __shfl(v, max(tail - 1, 0), GW);
        tail -= tail_opt && v2 > __shfl(v, tail, GW) ? 1 : 0;
    }
    v = __shfl(v, tail, GW);
    cj = __shfl(cj, tail, GW);
    if (seq >= 0 && l == 0) a.logp[seq] = v;

    if constexpr (PATH) {
        const bool valid = v > -INFINITY;
        const long long out = seq >= 0 ? a.slot_out[s] : 0;
        if constexpr (!OPT)
            if (live && !valid) a.bounds[woff + l] = -1;
        int cl = tail;
        [[maybe_unused]] int mine = -1;  // OPT: the frame at which this lane's position is entered, -1 if the path passes over it
        for (int t0 = (Tw - 1) / kChunk * kChunk; t0 >= 0; t0 -= kChunk) {
            unsigned p[kChunk];
#pragma unroll
            for (int k = 0; k < kChunk; ++k) p[k] = t0 + k < T ? bp[(long long)(t0 + k) * kVitWave] : 0u;
            [[maybe_unused]] unsigned long long sm[OPT ? kChunk : 1];
            if constexpr (OPT) {  // the group's bits of the eight rows (row 0 is never written: nothing enters at t = 0)
#pragma unroll
                for (int k = 0; k < kChunk; ++k) sm[k] = (t0 + k > 0 && t0 + k < T ? skip[t0 + k] : 0ull) >> (lane - l);
            }
            int ws = -1, wb = -1;  // lane k of the group writes step t0 + k
#pragma unroll
            for (int k = kChunk - 1; k >= 0; --k) {
                const unsigned pw = (unsigned)__shfl((int)p[k], cl, GW);  // the back-pointers of position cl
                if (t0 + k < T) {
                    const unsigned nb = (pw >> (4 * cj)) & 15u;
                    const bool in = (nb & 8u) != 0;  // never set at t = 0, nor on lane 0
                    if (l == k) {
                        ws = cl * N + cj;
                        wb = (in || t0 + k == 0) ? cl : -1;
                    }
                    if constexpr (OPT) mine = (in || t0 + k == 0) && cl == l ? t0 + k : mine;
                    cj = in ? N - 1 : (int)(nb & 7u);
                    if constexpr (OPT) cl = in ? cl - 1 - (int)((sm[k] >> cl) & 1ull) : cl;
                    else cl = in ? cl - 1 : cl;
                }
            }
            if (seq >= 0 && l < kChunk && t0 + l < T) {
                a.path[out + t0 + l] = valid ? ws : -1;
                if constexpr (!OPT)
                    if (valid && wb >= 0) a.bounds[woff + wb] = t0 + l;
            }
        }
        if constexpr (OPT)
            if (live) a.bounds[woff + l] = valid ? mine : -1;
    }
}

using AlFn = void (*)(AlArgs);

static AlFn al_kernel(int GW, int N, bool lr, bool path, bool opt) {
    return pick_gw_n(GW, N, [=](auto gw, auto n) -> AlFn {
        constexpr int G = decltype(gw)::value, S = decltype(n)::value;
        if (opt) {
            if (lr) return path ? k_align<G, S, true, true, true> : k_align<G, S, true, false, true>;
            return path ? k_align<G, S, false, true, true> : k_align<G, S, false, false, true>;
        }
        if (lr) return path ? k_align<G, S, true, true, false> : k_align<G, S, true, false, false>;
        return path ? k_align<G, S, false, true, false> : k_align<G, S, false, false, false>;
    });
}

void align_free(hmmbw_ctx *c) {
    hmmbw_ctx::Align &n = c->al;
    dfree(n.d_psi_off); dfree(n.d_in); dfree(n.d_tab); dfree(n.d_word_off); dfree(n.d_word_ids); dfree(n.d_path);
    dfree(n.d_bounds); dfree(n.d_bp); dfree(n.d_opt); dfree(n.d_skip);
    n = hmmbw_ctx::Align{};
}

// the aligner's buffers for the loaded observations, this bank shape and these transcripts: what
// word_decode_buffers keeps, the transcripts, and with paths the path, the bounds and the back-pointers; opt: the
// flags of the optional positions too, and with paths the entry-source masks (planned per width, as d_bp is)
static int align_buffers(hmmbw_ctx *c, int GW, size_t n_in, size_t n_tab, size_t n_pos, bool path, bool opt) {
    hmmbw_ctx::Align &n = c->al;
    if (n.GW != GW && n.d_skip) {
        sync_ctx(c);
        dfree(n.d_skip);
    }
    if (int rc = word_decode_buffers(c, n, GW, n_in, n_tab)) return rc;
    if (int rc = grow(c, n.d_word_ids, n.n_ids, n_pos)) return rc;
    if (opt) {
        if (int rc = grow(c, n.d_opt, n.n_opt, n_pos)) return rc;
        if (path && !n.d_skip)
            if (int rc = dalloc(&n.d_skip, (size_t)n.rows))
                return fail(rc, "the alignment entry-source masks (" + std::to_string(align_skip_bytes(n.rows)) +
                                    " bytes) do not fit: " + g_err);
    }
    if (!n.d_word_off)
        if (int rc = dalloc(&n.d_word_off, (size_t)c->R + 1)) return rc;
    if (path) {
        int rc = grow(c, n.d_bounds, n.n_bounds, n_pos);
        if (!rc && !n.d_path) rc = dalloc(&n.d_path, (size_t)c->vit.plan.total);
        const bool bp = !rc && !n.d_bp;  // the failure is the back-pointers'
        if (bp) rc = dalloc(&n.d_bp, (size_t)n.rows * kVitWave);
        if (rc) {  // none of the three is kept: the next call with paths allocates them again
            sync_ctx(c);
            dfree(n.d_bounds);
            n.n_bounds = 0;
            dfree(n.d_path);
            dfree(n.d_bp);
            if (!bp) return rc;
            return fail(rc, "the alignment back-pointers (" + std::to_string(align_bp_bytes(n.rows)) +
                                " bytes) do not fit: " + g_err);
        }
    }
    return HMMBW_OK;
}

}  // namespace hmmbw

namespace hmmbw {

// hmmbw_align (optional = nullptr) and hmmbw_align_optional
static int align_run(hmmbw_ctx *c, int n_words, const double *pi, const double *A, const double *B,
                     const int64_t *word_offsets, const int32_t *word_ids, const uint8_t *optional, int64_t n_seq,
                     int flags, double *logp_out, int32_t *path_out, int64_t path_len, int32_t *bounds_out,
                     int64_t bounds_len) {
    if (!c) return fail(HMMBW_E_INVALID, "null context");
    if (!c->has_obs) return fail(HMMBW_E_STATE, "observations not set");
    if (int rc = set_device(c)) return rc;
    if (!pi || !A || !B || !word_offsets || !word_ids || !logp_out) return fail(HMMBW_E_INVALID, "null argument");
    if (bounds_out && !path_out) return fail(HMMBW_E_INVALID, "bounds_out needs path_out");
    if (!align_flags_ok(flags)) return fail(HMMBW_E_INVALID, "unknown flag");
    if (int rc = check_n_seq(c, n_seq)) return rc;
    if (int rc = check_word_bank(c, n_words, pi, A, B, kAlMaxWords, kAlMaxStates, "a negative, infinite or NaN bank parameter"))
        return rc;
    const int W = n_words, N = c->N, K = c->K;
    long long longest = 0;
    if (int rc = check_transcripts(word_offsets, word_ids, n_seq, W, kAlMaxWords, &longest, nullptr)) return rc;
    if (optional)
        if (int rc = check_optional(word_offsets, word_ids, optional, n_seq, W, nullptr)) return rc;
    if (int rc = check_closed(c)) return rc;
    long long total = 0;
    if (int rc = check_path_len(c, path_len, &total)) return rc;
    const long long n_pos = n_seq > 0 ? word_offsets[n_seq] : 0;
    if (align_lengths_check(path_len, total, bounds_len, n_pos))
        return fail(HMMBW_E_INVALID, "bounds_len " + std::to_string(bounds_len) +
                                         " is not the number of transcript positions (" + std::to_string(n_pos) + ")");
    if (c->R == 0) return HMMBW_OK;

    const bool path = path_out != nullptr, opt = optional != nullptr;
    const bool lr = !(flags & HMMBW_ALIGN_DENSE) && wordnet_is_lr(A, W, N);
    const int GW = align_gw((int)longest);
    const EmbedTab o = align_tab(W, N, K);
    const long long n_in = embed_bank_len(W, N, K);
    if (int rc = align_buffers(c, GW, (size_t)n_in, (size_t)o.total, (size_t)n_pos, path, opt)) return rc;
    hmmbw_ctx::Align &n = c->al;

    std::vector<double> h;
    if (int rc = stage_bank(n.d_in, h, n_in, pi, A, B, W, N, K)) return rc;
    if (int rc = upload_transcripts(n.d_word_off, n.d_word_ids, word_offsets, word_ids, n_seq, n_pos)) return rc;
    if (opt)
        if (int rc = upload(n.d_opt, std::vector<unsigned char>(optional, optional + n_pos))) return rc;
    hipLaunchKernelGGL(k_align_prep, dim3((unsigned)std::min<long long>((o.total + 255) / 256, 1024)), dim3(256), 0,
                       c->stream, (const double *)n.d_in, W, N, K, o, n.d_tab);
    HIP_TRY(hipGetLastError());

    AlArgs a{};
    fill_slot_args(c, a);
    a.slot_out = c->vit.d_slot_out;
    a.psi_off = n.d_psi_off;
    a.word_off = n.d_word_off;
    a.word_ids = n.d_word_ids;
    a.tab = n.d_tab;
    a.bp = path ? n.d_bp : nullptr;
    a.logp = c->vit.d_logp;
    a.path = path ? n.d_path : nullptr;
    a.bounds = path ? n.d_bounds : nullptr;
    a.o_A = o.A;
    a.o_B = o.B;
    a.W = W;
    a.lds = embed_emis_in_lds(K, W, N) ? 1 : 0;
    a.end_final = (flags & HMMBW_ALIGN_END_FINAL) ? 1 : 0;
    a.optional = opt ? n.d_opt : nullptr;
    a.skip = opt && path ? n.d_skip : nullptr;
    const AlFn fn = al_kernel(GW, N, lr, path, opt);
    constexpr int wpb = kVitBlock / kVitWave;
    hipLaunchKernelGGL(fn, dim3((unsigned)((n.nvw + wpb - 1) / wpb)), dim3(kVitBlock),
                       a.lds ? embed_emis_bytes(K, W, N) : 0, c->stream, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(logp_out, c->vit.d_logp, sizeof(double) * (size_t)c->R, hipMemcpyDeviceToHost, c->stream));
    if (path && total > 0)
        HIP_TRY(hipMemcpyAsync(path_out, n.d_path, sizeof(int32_t) * (size_t)total, hipMemcpyDeviceToHost, c->stream));
    if (bounds_out && n_pos > 0)
        HIP_TRY(hipMemcpyAsync(bounds_out, n.d_bounds, sizeof(int32_t) * (size_t)n_pos, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return HMMBW_OK;
}

}  // namespace hmmbw

extern "C" int hmmbw_align(hmmbw_ctx *c, int n_words, const double *pi, const double *A, const double *B,
                           const int64_t *word_offsets, const int32_t *word_ids, int64_t n_seq, int flags,
                           double *logp_out, int32_t *path_out, int64_t path_len, int32_t *bounds_out,
                           int64_t bounds_len) {
    return hmmbw::align_run(c, n_words, pi, A, B, word_offsets, word_ids, nullptr, n_seq, flags, logp_out, path_out,
                            path_len, bounds_out, bounds_len);
}

extern "C" int hmmbw_align_optional(hmmbw_ctx *c, int n_words, const double *pi, const double *A, const double *B,
                                    const int64_t *word_offsets, const int32_t *word_ids, const uint8_t *optional,
                                    int64_t n_seq, int flags, double *logp_out, int32_t *path_out, int64_t path_len,
                                    int32_t *bounds_out, int64_t bounds_len) {
    return hmmbw::align_run(c, n_words, pi, A, B, word_offsets, word_ids, optional, n_seq, flags, logp_out, path_out,
                            path_len, bounds_out, bounds_len);
}
