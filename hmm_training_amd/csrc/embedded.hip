// embedded.hip — embedded Baum-Welch training over transcribed word sequences (hmmbw_embedded_train,
// include/hmmbw.h) for gfx950: every loaded utterance has a transcript w_0 .. w_{L-1} of word ids into a bank of W
// word models of the context's shape (pi [W][N], A [W][N][N], B [W][N][K]); the models are chained along the
// transcript, forward-backward runs over the chain, every instance of a word adds its posteriors to that word's
// statistics, and the reference's M-step (hmm_training.py:415-500) re-estimates each word.  The training
// counterpart of wordnet.hip: a word is left only from its last state, and the next one is entered at state j with
// weight pi_w[j].
//
// Scaled-linear fp64; composite state (l, j), l the transcript position:
//   alpha_0(0,j) = pi_{w_0}[j] b(o_0),  alpha_0(l>0, .) = 0
//   alpha_t(l,j) = (sum_i alpha_{t-1}(l,i) a_{w_l}[i][j] + alpha_{t-1}(l-1,N-1) pi_{w_l}[j]) b_{w_l,j}(o_t)
//   v_{t+1}(l,j) = b_{w_l,j}(o_{t+1}) beta_{t+1}(l,j)
//   beta_t(l,i)  = sum_j a_{w_l}[i][j] v_{t+1}(l,j) + [i = N-1] sum_j pi_{w_{l+1}}[j] v_{t+1}(l+1,j)
//   beta_{T-1}   = 1 on the states of the last instance (HMMBW_EMBED_END_FINAL: on (L-1, N-1) only), else 0
// each row rescaled by an exact power of two taken from the group's largest exponent, as k_posterior does.  A
// row's posteriors are normalised by the row's own sum S_t = sum alpha_t beta_t (beta_t before its rescale), so no
// scale factor is stored: gamma_t = alpha_t beta_t / S_t, the within-word arc (l,i) -> (l,j) has posterior
// alpha_t(l,i) a[i][j] v_{t+1}(l,j) / S_t and the entry arc into (l,j) alpha_t(l-1,N-1) pi[j] v_{t+1}(l,j) / S_t.
//
// k_embed_prep stages the bank into the tables (embed_plan.hpp, EmbedTab), clears the statistics and sets the
// state.  k_embed_estep gives every utterance a group of GW lanes (8, 16, 32 or 64), lane l = transcript position
// l, and reads the symbols from the context's own packs as the decoders do; a wave holds the 64 / GW consecutive
// layout slots.  The lane keeps its instance's alpha (then beta), its word's pi and A (2 values per state for
// left-to-right banks, N^2 for dense ones) and its xi and entry sums in registers; a forward step takes the left
// neighbour's alpha(l-1, N-1), a backward step the right neighbour's entry sum and the left neighbour's
// alpha(l-1, N-1), each a one-lane shift, plus the group's largest exponent and the row sum.  The forward rows go
// to a workspace ([t][j][64 lanes] per wave) and the backward reads them back; a lane re-reads only what it wrote.
// xi, entry and g_all go to the per-word statistics once per utterance and b_num at every step, by fp64 atomics
// (two lanes may hold the same word).  An utterance with P = 0 writes log P = -inf and adds nothing.
// k_embed_mstep (one workgroup per word) re-estimates the tables from the statistics and clears them;
// k_embed_conv (one workgroup) forms L = LSE_r log P_r, writes the iteration's record and sets done, after which
// every later launch of the three returns at once.  The host enqueues kEmChunk iterations between two reads of the
// state.  hmmbw_embedded_train_optional runs the same kernels with optional transcript positions (OPT, below).
#include "word_units.hpp"
#include "mstep.hpp"  // the element formulas of the M-step

namespace hmmbw {

struct EmArgs {
    const uint16_t *sym;
    const long long *wave_symoff;
    const int *slot_len, *slot_seq;
    const long long *work_off;   // decoding wave -> its first workspace row
    const long long *word_off;   // [R + 1] transcripts, CSR in caller order
    const int *word_ids;
    double *tab;                 // EmbedTab
    double *stats;               // EmbedStats
    double *work;                // rows x embed_row_doubles(N)
    double *logp;                // [R]
    EmbedState *state;
    long long nslots;
    long long o_A, o_B;          // EmbedTab offsets (pi is at 0)
    long long s_xi, s_gall, s_bnum;  // EmbedStats offsets (entry is at 0)
    int U, W, K;
    int shift;                   // pack entry -> symbol: >> shift, or / div when shift < 0
    int div;
    int lds;                     // the emission table is copied to LDS
    int end_final;
    const uint8_t *optional;     // OPT: a byte per transcript position, word_ids' order
    long long s_present;         // OPT: EmbedStats' total, where present [W] | touched [W] follow
};

// in: pi [W][N] | A [W][N][N] | B [W][N][K]
__global__ void __launch_bounds__(256) k_embed_prep(const double *__restrict__ in, int W, int N, int K, EmbedTab o,
                                                    double *__restrict__ tab, double *__restrict__ stats,
                                                    long long nstats, EmbedState *state, double epsilon,
                                                    long long max_iterations) {
    const int NP = embed_np(N);
    const double *pi = in, *A = pi + (long long)W * N, *B = A + (long long)W * N * N;
    const long long stride = (long long)gridDim.x * blockDim.x, first = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    for (long long e = first; e < o.total; e += stride) tab[e] = embed_bank_value(pi, A, B, W, N, NP, K, o, e);
    for (long long e = first; e < nstats; e += stride) stats[e] = 0.0;
    if (first == 0) {
        EmbedState s{};
        s.prev_L = -INFINITY;
        s.last_L = -INFINITY;
        s.last_diff = INFINITY;
        s.epsilon = epsilon;
        s.max_iterations = max_iterations;
        *state = s;
    }
}

template <int N>
__device__ __forceinline__ double max_of(const double (&x)[N]) {
    double m = x[0];
#pragma unroll
    for (int j = 1; j < N; ++j) m = fmax(m, x[j]);
    return m;
}

// OPT (hmmbw_embedded_train_optional with flags): a position with opt = 1 may be passed over.  alpha_0 is set on
// position 1 too when position 0 is optional; position l is also entered from (l - 2, N - 1) when l - 1 is optional,
// so a forward step adds the value two lanes to the left, and beta_t(l, N-1) the entry sum two lanes to the right
// when l + 1 is optional; beta_{T-1} is also set on L - 2 when L - 1 is optional.  An optional instance adds its
// entry mass (the probability that it is visited) to present[w].  OPT = false is the kernel as it was.
template <int GW, int N, bool LR, bool OPT>
__global__ void __launch_bounds__(kVitBlock) k_embed_estep(EmArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sB[];  // a.lds: B [K][W][NP]
    if (a.state->done) return;  // the whole grid
    constexpr int NP = embed_np(N);
    constexpr int SPW = kVitWave / GW;
    constexpr int NA = LR ? 2 * N : N * N;
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

    // the lane's instance: position l of the utterance's transcript (lanes past its end hold zeros throughout)
    int Lw = 0;
    long long woff = 0;
    if (seq >= 0) {
        woff = a.word_off[seq];
        Lw = (int)(a.word_off[seq + 1] - woff);
    }
    const bool live = l < Lw;
    const int wid = live ? a.word_ids[woff + l] : 0;
    const bool last_inst = live && l == Lw - 1;  // the last instance
    [[maybe_unused]] bool over = false, start = false, self_opt = false, end_opt = false;  // OPT: l - 1 may be passed over; a path starts here
    if constexpr (OPT) {
        over = live && l >= 2 && a.optional[woff + l - 1] != 0;
        start = l == 0 || (live && l == 1 && a.optional[woff] != 0);
        self_opt = live && a.optional[woff + l] != 0;
        end_opt = live && l == Lw - 2 && a.optional[woff + Lw - 1] != 0;
    }
    const bool tail = OPT ? last_inst || end_opt : last_inst;  // an instance a path may end in
    const size_t kstride = (size_t)a.W * NP, wrow = (size_t)wid * NP;
    const double *bt = (a.lds ? sB : tabB) + wrow;

    // chunk c of the slot: 8 steps in one 16-B load, U loads further on per chunk (pack_pos)
    const uint4 *pk = reinterpret_cast<const uint4 *>(a.sym) +
                      (real ? pack_pos(a.wave_symoff[s / a.U], a.U, (int)(s % a.U), 0) / kChunk : 0);
    auto chunk = [&](int t0) {
        uint4 q = make_uint4(0, 0, 0, 0);
        if (t0 < T) q = pk[(long long)(t0 / kChunk) * a.U];
        return q;
    };
    auto symbol = [&](const uint4 &q, int k) {  // symbol 0 past the slot's end (unused)
        const unsigned long long word = k < 4 ? (q.x | (unsigned long long)q.y << 32) : (q.z | (unsigned long long)q.w << 32);
        const unsigned e = (unsigned)(word >> (16 * (k & 3))) & 0xffffu;
        return a.shift >= 0 ? e >> a.shift : e / (unsigned)a.div;
    };

    double ca[NA];  // LR: a_{j-1,j}, a_jj per state j | dense: a_ij row-major
    {
        const double *tA = a.tab + a.o_A + (long long)wid * N * N;
        if constexpr (LR) {
#pragma unroll
            for (int j = 0; j < N; ++j) {
                ca[2 * j] = live && j > 0 ? tA[(j - 1) * N + j] : 0.0;
                ca[2 * j + 1] = live ? tA[j * N + j] : 0.0;
            }
        } else {
#pragma unroll
            for (int i = 0; i < N * N; ++i) ca[i] = live ? tA[i] : 0.0;
        }
    }
    double pi[N];
    load_row<N>(a.tab + wrow, pi);
#pragma unroll
    for (int j = 0; j < N; ++j) pi[j] = live ? pi[j] : 0.0;

    double *ws = a.work + a.work_off[vw] * embed_row_doubles(N) + lane;  // row t, state j: ws[(t N + j) 64]

    // ---- forward: alpha_hat_t, rescaled at every step; its rows go to the workspace
    double al[N];  // alpha_hat_{T-1} once the slot's steps are done
#pragma unroll
    for (int j = 0; j < N; ++j) al[j] = 0.0;
    long long esum = 0;  // the exponents taken out so far
    for (int t0 = 0; t0 < Tw; t0 += kChunk) {
        const uint4 q = chunk(t0);
#pragma nounroll
        for (int k = 0; k < kChunk; ++k) {
            const int t = t0 + k;
            if (t >= Tw) break;  // the whole wave
            double b[N];
            load_row<N>(bt + (size_t)symbol(q, k) * kstride, b);
            double left = from_left<GW>(al[N - 1], l, 0.0);
            if constexpr (OPT) left += from_left2<GW>(al[N - 1], over, 0.0);
            double nd[N];
#pragma unroll
            for (int j = 0; j < N; ++j) {
                double x;
                if constexpr (LR) {
                    x = al[j] * ca[2 * j + 1];
                    if (j > 0) x = fma(al[j - 1], ca[2 * j], x);
                } else {
                    x = al[0] * ca[j];
#pragma unroll
                    for (int i = 1; i < N; ++i) x = fma(al[i], ca[i * N + j], x);
                }
                x = fma(left, pi[j], x);
                if (t == 0) x = (OPT ? start : l == 0) ? pi[j] : 0.0;
                nd[j] = x * b[j];
            }
            const int e = group_exp<GW>(max_of<N>(nd));  // kZeroExp: the whole group is zero, and stays zero
            if (t < T) {
                esum += e;
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    al[j] = pow2_scale(nd[j], e);
                    ws[((long long)t * N + j) * kVitWave] = al[j];
                }
            }
        }
    }
    double fin = 0.0;  // the mass on the allowed end states
    if (tail) {
        fin = al[N - 1];
        if (!a.end_final) {
#pragma unroll
            for (int j = 0; j < N - 1; ++j) fin += al[j];
        }
    }
    const double tot = gsum<GW>(fin);
    const bool dead = !(tot > 0.0);  // P = 0
    if (seq >= 0 && l == 0) a.logp[seq] = dead ? -INFINITY : log(tot) + 0.6931471805599453094 * (double)esum;

    // ---- backward: beta_hat_t, the row's posteriors, the sums
    double be[N], bn[N];  // beta_hat_{t+1}, b(o_{t+1})
    double xi[NA], en[N], ga[N];
#pragma unroll
    for (int j = 0; j < N; ++j) be[j] = bn[j] = en[j] = ga[j] = 0.0;
#pragma unroll
    for (int i = 0; i < NA; ++i) xi[i] = 0.0;
    double *bnum = a.stats + a.s_bnum + wrow;
    for (int t0 = (Tw - 1) / kChunk * kChunk; t0 >= 0; t0 -= kChunk) {
        const uint4 q = chunk(t0);
#pragma nounroll
        for (int k = kChunk - 1; k >= 0; --k) {
            const int t = t0 + k;
            if (t >= Tw) continue;  // the whole wave
            const bool act = t < T, last = t == T - 1;
            const unsigned o = symbol(q, k);
            double at[N], b[N];
            load_row<N>(bt + (size_t)o * kstride, b);
#pragma unroll
            for (int j = 0; j < N; ++j) at[j] = act ? ws[((long long)t * N + j) * kVitWave] : 0.0;
            double v[N];
            double es = 0.0;  // this instance's entry sum
#pragma unroll
            for (int j = 0; j < N; ++j) {
                v[j] = bn[j] * be[j];
                es = fma(pi[j], v[j], es);
            }
            double right = from_right<GW>(es, l, 0.0);
            double aleft = from_left<GW>(at[N - 1], l, 0.0);
            if constexpr (OPT) {  // this instance's entry sum also reaches l - 2 when l - 1 is optional
                right += from_right2<GW>(over ? es : 0.0, l, 0.0);
                aleft += from_left2<GW>(at[N - 1], over, 0.0);
            }
            double bp[N];  // beta_t before its rescale
#pragma unroll
            for (int i = 0; i < N; ++i) {
                double x;
                if constexpr (LR) {
                    x = ca[2 * i + 1] * v[i];
                    if (i + 1 < N) x = fma(ca[2 * (i + 1)], v[i + 1], x);
                } else {
                    x = ca[i * N] * v[0];
#pragma unroll
                    for (int j = 1; j < N; ++j) x = fma(ca[i * N + j], v[j], x);
                }
                if (i == N - 1) x += right;
                if (last) x = tail && (!a.end_final || i == N - 1) ? 1.0 : 0.0;
                bp[i] = x;
            }
            double rs = 0.0;
#pragma unroll
            for (int j = 0; j < N; ++j) rs = fma(at[j], bp[j], rs);
            const double S = gsum<GW>(rs);  // the same bits in every lane of the group
            const double inv = act && !dead && S > 0.0 ? 1.0 / S : 0.0;
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const double g = at[j] * bp[j] * inv;
                ga[j] += g;
                if (t == 0 && (OPT ? start : l == 0)) en[j] += g;
                if (g > 0.0) atomicAdd(bnum + (size_t)o * kstride + j, g);
            }
            const double ainv = last ? 0.0 : inv;  // no arc leaves the last row
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const double va = v[j] * ainv;
                en[j] = fma(aleft * pi[j], va, en[j]);
                if constexpr (LR) {
                    xi[2 * j + 1] = fma(at[j] * ca[2 * j + 1], va, xi[2 * j + 1]);
                    if (j > 0) xi[2 * j] = fma(at[j - 1] * ca[2 * j], va, xi[2 * j]);
                } else {
#pragma unroll
                    for (int i = 0; i < N; ++i) xi[i * N + j] = fma(at[i] * ca[i * N + j], va, xi[i * N + j]);
                }
            }
            const int e = group_exp<GW>(max_of<N>(bp));
            if (act) {
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    be[j] = pow2_scale(bp[j], e);
                    bn[j] = b[j];
                }
            }
        }
    }

    // ---- once per utterance: the instance's sums into its word's statistics
    if (live && !dead) {
        double *sen = a.stats + (long long)wid * N, *sga = a.stats + a.s_gall + (long long)wid * N;
        double *sxi = a.stats + a.s_xi + (long long)wid * N * N;
        if constexpr (OPT) {
            double mass = 0.0;
#pragma unroll
            for (int j = 0; j < N; ++j) mass += en[j];
            if (self_opt && mass > 0.0) atomicAdd(a.stats + a.s_present + wid, mass);
        }
#pragma unroll
        for (int j = 0; j < N; ++j) {
            if (en[j] > 0.0) atomicAdd(sen + j, en[j]);
            if (ga[j] > 0.0) atomicAdd(sga + j, ga[j]);
            if constexpr (LR) {
                if (xi[2 * j + 1] > 0.0) atomicAdd(sxi + j * N + j, xi[2 * j + 1]);
                if (j > 0 && xi[2 * j] > 0.0) atomicAdd(sxi + (j - 1) * N + j, xi[2 * j]);
            } else {
#pragma unroll
                for (int i = 0; i < N; ++i)
                    if (xi[i * N + j] > 0.0) atomicAdd(sxi + i * N + j, xi[i * N + j]);
            }
        }
    }
}

// One workgroup per word: the M-step of hmm_training.py:415-500 from the word's statistics into the tables the
// next E-step reads; the statistics are cleared.  A word without an instance keeps its parameters.  With optional
// positions (a.optional set) count[w] holds the mandatory instances and the denominator of pi is count[w] +
// present[w]; a word whose denominator is 0 keeps its parameters, and touched[w] is set for every other word.
__global__ void __launch_bounds__(256) k_embed_mstep(EmArgs a, int N, const long long *__restrict__ count) {
    __shared__ double sDen[kEmMaxStates], sInv[kEmMaxStates];
    if (a.state->done) return;
    const int w = blockIdx.x, tid = threadIdx.x, NP = embed_np(N);
    const long long cnt = count[w];
    double *present = a.optional ? a.stats + a.s_present + w : nullptr;
    const double den_pi = present ? (double)cnt + *present : (double)cnt;
    const bool upd = den_pi > 0.0;
    double *sen = a.stats + (long long)w * N, *sga = a.stats + a.s_gall + (long long)w * N;
    double *sxi = a.stats + a.s_xi + (long long)w * N * N;
    if (tid < N) {
        double den = 0.0;  // a_den: the row sum of xi
        for (int j = 0; j < N; ++j) den += sxi[tid * N + j];
        sDen[tid] = den;
        sInv[tid] = mstep_inv(sga[tid]);
    }
    __syncthreads();
    if (upd) {
        if (tid < N) a.tab[(long long)w * NP + tid] = present ? mstep_a(sen[tid], den_pi) : mstep_pi(sen[tid], cnt);
        if (tid < N * N) a.tab[a.o_A + (long long)w * N * N + tid] = mstep_a(sxi[tid], sDen[tid / N]);
    }
    __syncthreads();
    if (present && tid == 0) {
        *present = 0.0;
        if (upd) present[a.W] = 1.0;  // touched
    }
    if (tid < N) sen[tid] = sga[tid] = 0.0;
    if (tid < N * N) sxi[tid] = 0.0;
    for (int idx = tid; idx < a.K * NP; idx += blockDim.x) {
        const int k = idx / NP, j = idx % NP;
        const long long at = ((long long)k * a.W + w) * NP + j;
        if (j < N && upd) a.tab[a.o_B + at] = bnum_to_b(a.stats[a.s_bnum + at], sInv[j]);
        a.stats[a.s_bnum + at] = 0.0;
    }
}

// One workgroup: L = LSE_r log P_r as a (max, sum exp) pair, the iteration's record and the stop rule
// (hmm_training.py:503-514, :346)
__global__ void __launch_bounds__(256) k_embed_conv(EmbedState *state, const double *__restrict__ logp, long long R) {
    __shared__ double sh[16];
    if (state->done) return;
    double mx = -INFINITY;
    for (long long r = threadIdx.x; r < R; r += blockDim.x) mx = fmax(mx, logp[r]);
    mx = block_reduce(mx, sh, true);
    double s = 0.0;
    if (mx != -INFINITY)
        for (long long r = threadIdx.x; r < R; r += blockDim.x) s += exp(logp[r] - mx);  // exp(-inf) = 0
    s = block_reduce(s, sh, false);
    if (threadIdx.x != 0) return;
    const double L = s > 0.0 ? mx + log(s) : -INFINITY;
    const double diff = state->prev_L != -INFINITY ? fabs(L - state->prev_L) : INFINITY;
    const long long it = state->iteration;
    const bool cont = diff >= state->epsilon && it + 1 < state->max_iterations;
    state->ring[2 * (it % kEmChunk)] = L;
    state->ring[2 * (it % kEmChunk) + 1] = diff;
    state->prev_L = state->last_L = L;
    state->last_diff = diff;
    state->iteration = it + 1;
    if (!cont) {
        state->done = 1;
        state->converged = it + 1 < state->max_iterations ? 1 : 0;
    }
}

// out: pi [W][N] | A [W][N][N] | B [W][N][K] from the tables, one workgroup per word; normalise: the reference's
// return path (hmm_training.py:524-541), pi / sum pi, and the rows of A and B with a positive sum divided by it
__global__ void __launch_bounds__(256) k_embed_export(const double *__restrict__ tab, long long o_A, long long o_B, int W,
                                                      int N, int K, int normalise, double *__restrict__ out) {
    __shared__ double sPi, sA[kEmMaxStates], sBr[kEmMaxStates];
    const int w = blockIdx.x, tid = threadIdx.x, NP = embed_np(N);
    const double *pi = tab + (long long)w * NP, *A = tab + o_A + (long long)w * N * N;
    auto b = [&](int j, int k) { return tab[o_B + ((long long)k * W + w) * NP + j]; };
    if (tid == 0) {
        double s = 0.0;
        for (int j = 0; j < N; ++j) s += pi[j];
        sPi = s;
    }
    if (tid < N) {
        double s = 0.0;
        for (int j = 0; j < N; ++j) s += A[tid * N + j];
        sA[tid] = s;
        double sb = 0.0;
        for (int k = 0; k < K; ++k) sb += b(tid, k);
        sBr[tid] = sb;
    }
    __syncthreads();
    double *opi = out + (long long)w * N, *oA = out + (long long)W * N + (long long)w * N * N;
    double *oB = out + (long long)W * N + (long long)W * N * N + (long long)w * N * K;
    if (tid < N) opi[tid] = normalise && sPi > 0.0 ? pi[tid] / sPi : pi[tid];
    if (tid < N * N) oA[tid] = normalise && sA[tid / N] > 0.0 ? A[tid] / sA[tid / N] : A[tid];
    for (int idx = tid; idx < N * K; idx += blockDim.x) {
        const int j = idx / K, k = idx % K;
        oB[idx] = normalise && sBr[j] > 0.0 ? b(j, k) / sBr[j] : b(j, k);
    }
}

using EmFn = void (*)(EmArgs);

static EmFn em_kernel(int GW, int N, bool lr, bool opt) {
    return pick_gw_n(GW, N, [=](auto gw, auto n) -> EmFn {
        constexpr int G = decltype(gw)::value, S = decltype(n)::value;
        if (opt) return lr ? k_embed_estep<G, S, true, true> : k_embed_estep<G, S, false, true>;
        return lr ? k_embed_estep<G, S, true, false> : k_embed_estep<G, S, false, false>;
    });
}

// the buffers of one call, from the library's block cache
struct EmWork {
    double *in = nullptr, *tab = nullptr, *stats = nullptr, *work = nullptr, *logp = nullptr;
    long long *work_off = nullptr, *word_off = nullptr, *count = nullptr;
    int *word_ids = nullptr;
    unsigned char *optional = nullptr;
    EmbedState *state = nullptr;
    hmmbw_ctx *c = nullptr;
    ~EmWork() {
        sync_ctx(c);
        dfree(in); dfree(tab); dfree(stats); dfree(work); dfree(logp);
        dfree(work_off); dfree(word_off); dfree(count); dfree(word_ids); dfree(optional); dfree(state);
    }
};

template <class T>
static int to_device(T **d, const std::vector<T> &h) {
    if (int rc = dalloc(d, h.size())) return rc;
    return upload(*d, h);
}

}  // namespace hmmbw

namespace hmmbw {

// hmmbw_embedded_train (optional = nullptr) and hmmbw_embedded_train_optional
static int embedded_run(hmmbw_ctx *c, int n_words, double *pi, double *A, double *B, const int64_t *word_offsets,
                        const int32_t *word_ids, const uint8_t *optional, int64_t n_seq, int flags, double epsilon,
                        int64_t max_iterations, int normalise, hmmbw_iter_record *records, int64_t records_cap,
                        int64_t *n_records, double *logp_out) {
    if (!c) return fail(HMMBW_E_INVALID, "null context");
    if (!c->has_obs) return fail(HMMBW_E_STATE, "observations not set");
    if (int rc = set_device(c)) return rc;
    if (!pi || !A || !B || !word_offsets || !word_ids) return fail(HMMBW_E_INVALID, "null argument");
    if (flags & ~(HMMBW_EMBED_END_FINAL | HMMBW_EMBED_DENSE)) return fail(HMMBW_E_INVALID, "unknown flag");
    if (max_iterations < 1) return fail(HMMBW_E_INVALID, "max_iterations " + std::to_string(max_iterations) + " < 1");
    if (!(epsilon >= 0.0)) return fail(HMMBW_E_INVALID, "epsilon is negative or NaN");
    if (int rc = check_n_seq(c, n_seq)) return rc;
    if (c->world > 1) return fail(HMMBW_E_UNSUPPORTED, "embedded training on a multi-rank context");
    if (c->det) return fail(HMMBW_E_UNSUPPORTED, "embedded training in deterministic mode (its sums are floating-point atomics)");
    if (int rc = check_word_bank(c, n_words, pi, A, B, kEmMaxWords, kEmMaxStates, "a negative, infinite or NaN bank parameter"))
        return rc;
    const int W = n_words, N = c->N, K = c->K;
    long long longest = 0;
    std::vector<long long> count((size_t)W, 0);
    if (int rc = check_transcripts(word_offsets, word_ids, n_seq, W, kEmMaxWords, &longest, count.data())) return rc;
    const bool opt = optional != nullptr;
    if (opt)  // count: the mandatory instances
        if (int rc = check_optional(word_offsets, word_ids, optional, n_seq, W, count.data())) return rc;
    if (int rc = check_closed(c)) return rc;
    if (n_records) *n_records = 0;
    if (c->R == 0) return HMMBW_OK;

    const bool lr = !(flags & HMMBW_EMBED_DENSE) && wordnet_is_lr(A, W, N);
    const int GW = embed_gw((int)longest);
    const EmbedTab o = embed_tab(W, N, K);
    const EmbedStats so = embed_stats(W, N, K);
    const long long n_bank = embed_bank_len(W, N, K);
    const long long n_stats = opt ? embed_stats_optional_total(W, N, K) : so.total;
    const ViterbiPlan P = plan_viterbi_group(c->h_slen, c->h_sseq, c->R, GW);

    EmWork w;
    w.c = c;
    if (int rc = dalloc(&w.work, (size_t)(P.psi_rows * embed_row_doubles(N))))
        return fail(rc, "the forward workspace (" + std::to_string(embed_work_bytes(P.psi_rows, N)) +
                            " bytes) does not fit: " + g_err);
    if (int rc = dalloc(&w.in, (size_t)n_bank)) return rc;
    if (int rc = dalloc(&w.tab, (size_t)o.total)) return rc;
    if (int rc = dalloc(&w.stats, (size_t)n_stats)) return rc;
    if (int rc = dalloc(&w.logp, (size_t)c->R)) return rc;
    if (int rc = dalloc(&w.state, 1)) return rc;
    if (int rc = to_device(&w.work_off, P.psi_off)) return rc;
    if (int rc = to_device(&w.count, count)) return rc;
    const long long n_pos = word_offsets[n_seq];
    if (int rc = dalloc(&w.word_off, (size_t)n_seq + 1)) return rc;
    if (int rc = dalloc(&w.word_ids, (size_t)n_pos)) return rc;
    if (int rc = upload_transcripts(w.word_off, w.word_ids, word_offsets, word_ids, n_seq, n_pos)) return rc;
    if (opt)
        if (int rc = to_device(&w.optional, std::vector<unsigned char>(optional, optional + n_pos))) return rc;
    std::vector<double> h;  // the staged bank, and the trained one on the way back
    if (int rc = stage_bank(w.in, h, n_bank, pi, A, B, W, N, K)) return rc;
    const long long nprep = std::max(o.total, n_stats);
    hipLaunchKernelGGL(k_embed_prep, dim3((unsigned)std::min<long long>((nprep + 255) / 256, 1024)), dim3(256), 0,
                       c->stream, w.in, W, N, K, o, w.tab, w.stats, n_stats, w.state, epsilon, (long long)max_iterations);
    HIP_TRY(hipGetLastError());

    EmArgs a{};
    fill_slot_args(c, a);
    a.work_off = w.work_off;
    a.word_off = w.word_off;
    a.word_ids = w.word_ids;
    a.tab = w.tab;
    a.stats = w.stats;
    a.work = w.work;
    a.logp = w.logp;
    a.state = w.state;
    a.o_A = o.A;
    a.o_B = o.B;
    a.s_xi = so.xi;
    a.s_gall = so.gall;
    a.s_bnum = so.bnum;
    a.W = W;
    a.lds = embed_emis_in_lds(K, W, N) ? 1 : 0;
    a.end_final = (flags & HMMBW_EMBED_END_FINAL) ? 1 : 0;
    a.optional = w.optional;
    a.s_present = embed_present_off(W, N, K);
    const EmFn fn = em_kernel(GW, N, lr, opt);
    constexpr int wpb = kVitBlock / kVitWave;
    const unsigned grid = (unsigned)((P.nvw + wpb - 1) / wpb);
    const size_t lds = a.lds ? embed_emis_bytes(K, W, N) : 0;

    EmbedState st{};
    long long enq = 0, seen = 0;
    while (!st.done && enq < max_iterations) {
        const long long nq = std::min<long long>(kEmChunk, max_iterations - enq);
        for (long long i = 0; i < nq; ++i) {
            hipLaunchKernelGGL(fn, dim3(grid), dim3(kVitBlock), lds, c->stream, a);
            hipLaunchKernelGGL(k_embed_mstep, dim3((unsigned)W), dim3(256), 0, c->stream, a, N, (const long long *)w.count);
            hipLaunchKernelGGL(k_embed_conv, dim3(1), dim3(256), 0, c->stream, w.state, (const double *)w.logp, (long long)c->R);
        }
        HIP_TRY(hipGetLastError());
        enq += nq;
        HIP_TRY(hipMemcpyAsync(&st, w.state, sizeof(EmbedState), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        for (; seen < st.iteration; ++seen)
            if (records && seen < records_cap) {
                records[seen].log_likelihood = st.ring[2 * (seen % kEmChunk)];
                records[seen].diff = st.ring[2 * (seen % kEmChunk) + 1];
            }
    }
    if (!st.done) return fail(HMMBW_E_STATE, "hmmbw_embedded_train: the device state did not reach done within its bound");
    if (n_records) *n_records = seen;

    hipLaunchKernelGGL(k_embed_export, dim3((unsigned)W), dim3(256), 0, c->stream, (const double *)w.tab, o.A, o.B, W, N, K,
                       normalise ? 1 : 0, w.in);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h.data(), w.in, sizeof(double) * (size_t)n_bank, hipMemcpyDeviceToHost, c->stream));
    if (logp_out)
        HIP_TRY(hipMemcpyAsync(logp_out, w.logp, sizeof(double) * (size_t)c->R, hipMemcpyDeviceToHost, c->stream));
    std::vector<double> touched;  // opt: nonzero for the words an M-step re-estimated
    if (opt) {
        touched.resize((size_t)W);
        HIP_TRY(hipMemcpyAsync(touched.data(), w.stats + embed_touched_off(W, N, K), sizeof(double) * (size_t)W,
                               hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    // a word without an instance (opt: whose denominator was 0 in every iteration) keeps the caller's values bit for bit
    const double *hpi = h.data(), *hA = hpi + (long long)W * N, *hB = hA + (long long)W * N * N;
    for (long long x = 0; x < W; ++x) {
        if (opt ? touched[(size_t)x] == 0.0 : count[(size_t)x] == 0) continue;
        std::copy(hpi + x * N, hpi + (x + 1) * N, pi + x * N);
        std::copy(hA + x * N * N, hA + (x + 1) * N * N, A + x * N * N);
        std::copy(hB + x * N * K, hB + (x + 1) * N * K, B + x * N * K);
    }
    return HMMBW_OK;
}

}  // namespace hmmbw

extern "C" int hmmbw_embedded_train(hmmbw_ctx *c, int n_words, double *pi, double *A, double *B,
                                    const int64_t *word_offsets, const int32_t *word_ids, int64_t n_seq, int flags,
                                    double epsilon, int64_t max_iterations, int normalise, hmmbw_iter_record *records,
                                    int64_t records_cap, int64_t *n_records, double *logp_out) {
    return hmmbw::embedded_run(c, n_words, pi, A, B, word_offsets, word_ids, nullptr, n_seq, flags, epsilon,
                               max_iterations, normalise, records, records_cap, n_records, logp_out);
}

extern "C" int hmmbw_embedded_train_optional(hmmbw_ctx *c, int n_words, double *pi, double *A, double *B,
                                             const int64_t *word_offsets, const int32_t *word_ids,
                                             const uint8_t *optional, int64_t n_seq, int flags, double epsilon,
                                             int64_t max_iterations, int normalise, hmmbw_iter_record *records,
                                             int64_t records_cap, int64_t *n_records, double *logp_out) {
    return hmmbw::embedded_run(c, n_words, pi, A, B, word_offsets, word_ids, optional, n_seq, flags, epsilon,
                               max_iterations, normalise, records, records_cap, n_records, logp_out);
}
