/*
 * hmmbw.h — C ABI of the MI355X-native Baum-Welch engine (libhmmbw.so).
 *
 * The reference (DemianMArin/HMM_Training, pure Python/NumPy) has no FFI; its hot-path boundary is
 * the Python function
 *     hmm_training(observations, N=4, M=256, epsilon=1e-6, max_iterations=100,
 *                  show_progress=True, word_name=None, load_initial_params=True) -> (A, B, pi)
 * at HMM/hmm_training.py:265-267, its forward-only scorer
 *     calculate_log_likelihood(recording_observations, hmm) -> float   (HMM/hmm_testing.py:49)
 * and its VQ encoder get_observations (HMM/hmm_training.py:82-120).  Each entry point below says
 * which part of those functions it replaces.  The Python drop-in (hmm_training_amd/) binds this
 * ABI with ctypes; INTEGRATION.md shows the binding.
 *
 * Conventions
 *  - Every function returns an int status: HMMBW_OK (0) or a negative HMMBW_E_* code; the message
 *    of the last failure on the calling thread is hmmbw_last_error().  No C++ exception crosses
 *    the ABI.
 *  - All arrays are plain row-major host or device pointers with explicit sizes; no torch types.
 *  - Probabilities are fp64, LINEAR domain (the reference converts with safe_log/safe_exp at
 *    hmm_training.py:323-325 and :524-526; the engine's scaled-linear recursions are the same
 *    quantities).
 *  - Work is enqueued on the context's HIP stream (hmmbw_set_stream) and is asynchronous, except
 *    the functions marked SYNC, which synchronise that stream.
 *  - One context per device per thread; contexts are independent.
 */
#ifndef HMMBW_H
#define HMMBW_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HMMBW_ABI_VERSION 5 /* 2: hmmbw_iterate_begin/_end, status snapshots, comm info/payload;
                              3: peer all-reduce (hmmbw_peer_*), HMMBW_E_TIMEOUT, cache trim, split timing;
                              4: live status mirror (HMMBW_OPT_LIVE_STATUS, hmmbw_status_live_wait);
                              5: hmmbw_get_option, HMMBW_OPT_WQ_TIMEOUT_MS, HMMBW_OPT_WIDE_WQ
                                 (HMMBW_OPT_LDS_LAYOUT / HMMBW_INFO_LDS_LAYOUT are new keys of the same calls:
                                 an older library answers them HMMBW_E_INVALID, no entry point changed;
                                 hmmbw_viterbi is a new entry point of version 5: an older library lacks the
                                 symbol; hmmbw_posterior is a new entry point of version 5: an older library
                                 lacks the symbol; hmmbw_lbg_train is a new entry point of version 5: an older
                                 library lacks the symbol; hmmbw_wordnet_decode is a new entry point of version
                                 5: an older library lacks the symbol; hmmbw_embedded_train is a new entry point
                                 of version 5: an older library lacks the symbol; hmmbw_mfcc and
                                 hmmbw_mfcc_tables are new entry points of version 5: an older library lacks the
                                 symbols; hmmbw_align is a new entry point of version 5: an older library lacks
                                 the symbol; hmmbw_align_optional and hmmbw_embedded_train_optional are new
                                 entry points of version 5: an older library lacks the symbols; hmmbw_preprocess
                                 and hmmbw_window_overlap are new entry points of version 5: an older library
                                 lacks the symbols) */

#define HMMBW_OK 0
#define HMMBW_E_INVALID (-1)        /* bad argument (shape, range, null pointer)             */
#define HMMBW_E_HIP (-2)            /* HIP runtime error                                      */
#define HMMBW_E_UNSUPPORTED (-3)    /* shape outside what the kernels implement (N > 64)       */
#define HMMBW_E_STATE (-4)          /* call order violated (e.g. estep before observations)   */
#define HMMBW_E_EMPTY_SEQUENCE (-5) /* a sequence of length 0: the reference raises IndexError
                                       at hmm_training.py:376 / hmm_testing.py:75              */
#define HMMBW_E_SYMBOL_RANGE (-6)   /* symbol id >= M: numpy IndexError at hmm_training.py:360 */
#define HMMBW_E_TIMEOUT (-7)        /* a bounded device-side wait expired: a rank did not deliver its
                                       statistics to the peer all-reduce in time, or a wide work-queue
                                       backward sweep did not see its forward finish (EM stops, the
                                       status calls report it; hmmbw_last_error says which)           */

/* Transition-matrix kernel variant (the reference skips -inf transitions,
 * hmm_training.py:143-144,186-188; a left-to-right A keeps its zero pattern under EM). */
#define HMMBW_TOPOLOGY_AUTO 0          /* left-to-right if A's zero pattern allows, else dense */
#define HMMBW_TOPOLOGY_DENSE 1
#define HMMBW_TOPOLOGY_LEFT_TO_RIGHT 2 /* a_ij == 0 unless j in {i, i+1}                      */

typedef struct hmmbw_ctx hmmbw_ctx;

/* One EM iteration's convergence record: hmm_training.py:503-513 (L = LSE_r log P_r of the
 * parameters ENTERING the iteration, diff = |L - L_prev| or +inf on the first iteration). */
typedef struct {
    double log_likelihood;
    double diff;
} hmmbw_iter_record;

typedef struct {
    int64_t iterations; /* EM iterations executed (the reference's `iteration`, :514)          */
    int32_t done;       /* 1 once `diff >= epsilon and iteration < max_iterations` (:346) fails */
    int32_t converged;  /* 1 if it stopped on epsilon rather than on max_iterations (:516-521)  */
    double last_log_likelihood;
    double last_diff;
} hmmbw_status;

int hmmbw_abi_version(void);
const char *hmmbw_last_error(void);
int hmmbw_device_count(int *out);

/* The library keeps the small device buffers and pinned snapshot blocks of destroyed contexts (blocks
 * <= 4 MB, at most 32 MB per kind and device) for the next context: the drop-in builds one context per
 * hmm_training call (hmm_training.py:265-267) and hipFree synchronises the device.  This returns every
 * cached block to the driver (e.g. before a memory-hungry phase of the process, or on an
 * out-of-memory); *bytes_released (may be NULL) gets the total.  Blocks of live contexts are not
 * touched. */
int hmmbw_cache_trim(int64_t *bytes_released);

/* Context for one (device, N states, M symbols) model.  Replaces the parameter set-up of
 * hmm_training.py:268-339 (allocation is sized by hmmbw_set_observations). */
int hmmbw_ctx_create(int device, int n_states, int n_symbols, hmmbw_ctx **out);
int hmmbw_ctx_destroy(hmmbw_ctx *ctx);
int hmmbw_set_stream(hmmbw_ctx *ctx, void *hip_stream); /* hipStream_t; NULL = legacy default */
int hmmbw_set_rank(hmmbw_ctx *ctx, int rank, int world_size);
int hmmbw_set_topology(hmmbw_ctx *ctx, int topology);
int hmmbw_get_topology(const hmmbw_ctx *ctx, int *out); /* resolved variant (after AUTO)      */

/* Observation sequences as host CSR: sequence r is symbols[offsets[r] .. offsets[r+1]).
 * Replaces the `observations: List[np.ndarray]` argument (hmm_training.py:265) — the caller
 * keeps ownership; the library copies to HBM in its own length-sorted, time-major layout. */
int hmmbw_set_observations(hmmbw_ctx *ctx, const int64_t *offsets, const int32_t *symbols, int64_t n_seq);

/* Linear (pi[N], A[N*N], B[N*M]) host arrays: the initial parameters (hmm_training.py:299-325). */
int hmmbw_set_params(hmmbw_ctx *ctx, const double *pi, const double *A, const double *B);

/* Arm a training run: epsilon and max_iterations of hmm_training.py:265-266,342-346. */
int hmmbw_reset_training(hmmbw_ctx *ctx, double epsilon, int64_t max_iterations);

/* Length (in doubles) of the packed sufficient-statistics buffer used by estep/mstep. */
int hmmbw_stats_len(const hmmbw_ctx *ctx, int64_t *n_doubles);

/* E-step over this rank's sequences (hmm_training.py:351-410): writes this rank's packed statistics
 * {pi_num[N], xi[N*N], gamma_den_excl_last[N], gamma_den_all[N], B_num[M*N], (m, s)[world]}
 * (linear-domain sums: xi_ij = sum_r sum_t xi_t(i,j), B_num symbol-major [M][N]) into the DEVICE
 * buffer stats_dev (hmmbw_stats_len doubles; its (m, s) pair — the max and sum-exp of log P_r —
 * in slot `rank`, other slots zero).  Multi-rank callers all-reduce(sum) stats_dev, then call
 * hmmbw_mstep.  A deferred M-step (below) runs at the start of this launch. */
int hmmbw_estep(hmmbw_ctx *ctx, double *stats_dev);

/* M-step + convergence (hmm_training.py:415-514) from the (all-reduced) statistics; n_seq_global
 * is the R of :424.  No-op once done.  With HMMBW_OPT_MERGE_MSTEP (default) it is DEFERRED: the
 * next hmmbw_estep runs it in the prologue of its own kernel, so stats_dev must stay untouched until
 * then; hmmbw_get_status / get_params / score / set_params / reset_training complete it first. */
int hmmbw_mstep(hmmbw_ctx *ctx, double *stats_dev, int64_t n_seq_global);

/* Enqueue n_iter iterations of (estep, mstep) with internal statistics (the last M-step stays
 * deferred until a query, as for hmmbw_mstep).  Iterations after convergence are device-side no-ops
 * (same result as stopping, :346).  Single rank, or several ranks with hmmbw_comm_init (below). */
int hmmbw_iterate(hmmbw_ctx *ctx, int64_t n_iter);

/* Native RCCL communicator for the multi-rank loop.  With it, hmmbw_iterate(ctx, n) on a context of
 * world_size > 1 runs n iterations of {estep -> ncclAllReduce(sum) of the packed statistics on the
 * context's stream -> mstep} with no host round trip, replacing the per-iteration
 * torch.distributed.all_reduce hop (one RCCL all-reduce per EM iteration either way).  rccl_path:
 * the RCCL library the process already uses (torch's librccl.so), or NULL to look it up.  Rank 0
 * calls hmmbw_comm_unique_id and shares the 128-byte id (e.g. torch.distributed.broadcast); then
 * every rank calls hmmbw_comm_init (collective: all ranks must call it) after hmmbw_set_rank.
 * n_seq_global is the R of hmm_training.py:424 over all ranks.  (A 1-rank communicator is allowed:
 * hmmbw_iterate then takes the same multi-rank sequence, which is how it is tested on one GPU.) */
int hmmbw_comm_probe(const char *rccl_path); /* HMMBW_OK if the RCCL entry points resolve (local check) */
int hmmbw_comm_unique_id(const char *rccl_path, void *id_out);
int hmmbw_comm_init(hmmbw_ctx *ctx, const char *rccl_path, const void *id, int rank, int world_size,
                    int64_t n_seq_global);
/* SYNC. The engine communicator as created: *n_ranks = ncclCommCount (0 without a communicator),
 * plus the HIP-event time of the ncclAllReduce calls hmmbw_iterate enqueued while E-step timing was
 * on (hmmbw_timing; the same every-k-th schedule), summed in *total_ms over *count calls.  reset=1
 * clears the accumulated time.  Measurement only (bench.py's all-reduce microseconds per iteration). */
int hmmbw_comm_info(hmmbw_ctx *ctx, int *n_ranks, double *total_ms, int64_t *count, int reset);

/* Length in doubles of the last all-reduce hmmbw_iterate enqueued on the engine communicator (0
 * before the first): the fused small path all-reduces its statistics copies plus one (max, sum exp)
 * pair per rank, 256-B aligned; the other paths the packed statistics (hmmbw_stats_len). */
int hmmbw_comm_payload(const hmmbw_ctx *ctx, int64_t *n_doubles);

/* One multi-rank EM iteration split at its all-reduce, for callers that bring their own collective
 * (torch.distributed, MPI, an in-process sum over several contexts) or test the exact enqueue
 * sequence an RCCL run makes without RCCL: hmmbw_iterate_begin enqueues this rank's E-step (on the
 * small kernels the fused one that accumulates straight into the all-reduce buffer and writes the
 * rank's (max, sum exp) pair of log P; elsewhere hmmbw_estep into the packed statistics) and returns
 * the DEVICE buffer *buf of *n_doubles doubles that the caller must all-reduce (sum, in place, ordered
 * after the context's stream) before hmmbw_iterate_end, which enqueues the M-step + convergence step
 * (hmm_training.py:415-514; merged into the next E-step launch when it can).  n_seq_global is the R of
 * :424.  The buffer layout does not depend on the shard, so every rank (an empty shard too) passes the
 * same length.  hmmbw_iterate on a context with hmmbw_comm_init runs exactly begin -> ncclAllReduce ->
 * end per iteration.  Any other training call between the two returns HMMBW_E_STATE. */
int hmmbw_iterate_begin(hmmbw_ctx *ctx, int64_t n_seq_global, double **buf, int64_t *n_doubles);
int hmmbw_iterate_end(hmmbw_ctx *ctx);

/* ---- Peer all-reduce (HMMBW_OPT_ALLREDUCE = HMMBW_ALLREDUCE_PEER) ----
 * The sums the reference forms over all recordings (pi over the global R, hmm_training.py:415-424; A and B,
 * :429-500; L over all sequences, :503) are one elementwise sum of every rank's statistics buffer per EM
 * iteration.  Instead of an RCCL all-reduce, every rank owns a RECEIVE REGION in its HBM with one slot per
 * rank (double-buffered by iteration parity) and one flag per (rank, 2 KB chunk): after its E-step a rank
 * writes its buffer into slot `rank` of every rank's region (system-scope write-through stores over xGMI,
 * then the chunk's flag = the iteration's sequence number), and before its M-step it waits for all the
 * flags of its own region (bounded: HMMBW_OPT_PEER_TIMEOUT_MS) and sums the slots in rank order, so every
 * rank holds bitwise-identical sums and takes the same stop decision (:346).  Set-up, collective over the
 * ranks (all call it, after hmmbw_set_rank and the options, before the first iteration):
 *   hmmbw_peer_region     allocate this rank's receive region (*bytes; *region its device address);
 *   hmmbw_peer_ipc_handle its 64-byte HIP IPC handle, to be exchanged between the rank processes;
 *   hmmbw_peer_open       map every other rank's region from the exchanged handles (world x 64 bytes, in
 *                         rank order) and attach them, or
 *   hmmbw_peer_attach     attach regions already addressable here (world device pointers, rank order;
 *                         several ranks in one process on one GPU, as the tests run it).
 * n_seq_global is the R of hmm_training.py:424 over all ranks (hmmbw_iterate's loop).  Attaching clears
 * the flags: every rank must attach before any rank starts an iteration. */
int hmmbw_peer_region(hmmbw_ctx *ctx, void **region, int64_t *bytes);
int hmmbw_peer_ipc_handle(hmmbw_ctx *ctx, void *handle_out);
int hmmbw_peer_open(hmmbw_ctx *ctx, const void *handles, int64_t n_seq_global);
int hmmbw_peer_attach(hmmbw_ctx *ctx, void *const *regions, int64_t n_seq_global);
/* The all-reduce hmmbw_iterate and hmmbw_iterate_begin/_end use now: -1 none (single rank), 0 RCCL
 * (engine communicator, or the caller's collective for _begin/_end), 1 peer. */
int hmmbw_allreduce_kind(const hmmbw_ctx *ctx, int *kind);

/* SYNC. Status plus the iteration records [first, first+count) (ring of 4096 entries). */
int hmmbw_get_status(hmmbw_ctx *ctx, hmmbw_status *status, hmmbw_iter_record *records, int64_t first,
                     int64_t count);

/* ASYNC. Snapshot the status and the iteration records [first, iterations) on the context stream
 * into pinned host memory (one small kernel; no M-step flush: with merged M-steps the snapshot covers
 * every iteration enqueued before it except the last) and return its ticket.  Lets a host loop keep the next chunk of iterations
 * queued while it reads the previous chunk's status (the drop-in train loop, hmm_training.py
 * :346-514; iterations enqueued past convergence are device-side no-ops).  Two snapshots are kept:
 * posting a third first waits for the oldest to land. */
int hmmbw_status_post(hmmbw_ctx *ctx, int64_t first, int64_t *ticket);

/* Waits for snapshot `ticket` (one of the last two posted) only, not for the work queued after it;
 * then fills status and the records [first, first+count), which must lie inside the snapshot's
 * [first posted, iterations). */
int hmmbw_status_wait(hmmbw_ctx *ctx, int64_t ticket, hmmbw_status *status, hmmbw_iter_record *records,
                      int64_t first, int64_t count);

/* With HMMBW_OPT_LIVE_STATUS = 1 every M-step that records an iteration (:503-514) also writes that
 * record and the new status into pinned host memory from the device, while the launch that runs it (with
 * merged M-steps: the next E-step, in its prologue) is still executing.  This waits, by polling that
 * memory, until `iterations` iterations are recorded or EM has stopped, then fills status and the records
 * [first, first+count).  No stream synchronisation and no extra kernel: a host loop sees iteration e's
 * convergence record a few microseconds into launch e + 1, while launch e + 2 can already be queued
 * behind it (the reference's per-iteration check, :346,503-514, without idling the GPU).  If the stream
 * runs dry first (the last M-step still pending, or a device-side stop), it returns the device status. */
int hmmbw_status_live_wait(hmmbw_ctx *ctx, int64_t iterations, hmmbw_status *status, hmmbw_iter_record *records,
                           int64_t first, int64_t count);

/* SYNC. Current parameters.  normalise=1 applies the reference's return path (safe_exp then
 * pi/sum(pi), row-normalise A and B rows with positive sums, :524-541); normalise=0 returns the
 * unnormalised working parameters (exp of the reference's log_pi/log_a/log_b matrices). */
int hmmbw_get_params(hmmbw_ctx *ctx, double *pi, double *A, double *B, int normalise);

/* SYNC. log P(O_r | lambda) of the last E-step, in the caller's sequence order (:375-377). */
int hmmbw_get_loglik(hmmbw_ctx *ctx, double *out);

/* SYNC. Forward-only scoring of the loaded sequences under the current parameters:
 * hmm_testing.py:49-104 calculate_log_likelihood for every sequence, one launch. */
int hmmbw_score(hmmbw_ctx *ctx, double *out);

/* SYNC. Viterbi decoding of the loaded sequences under the current parameters, log domain, fp64:
 *   delta_0(j) = log pi_j + log b_j(o_0)
 *   delta_t(j) = max_i (delta_{t-1}(i) + log a_ij) + log b_j(o_t)
 *   psi_t(j)   = the SMALLEST i attaining the max (strict '>' scan from i = 0)
 *   end state  = the smallest j attaining max_j delta_{T-1}(j)
 * log 0 = -inf; a -inf candidate never wins against a finite one.
 * logp_out[r] (R doubles, caller order): the best path's log-probability, -inf if no path has positive
 * probability.  path_out (may be NULL: scores only, no back-pointers are stored): int32, caller CSR order,
 * path_out[offsets[r] + t] = state at step t; every entry of a sequence whose logp is -inf is -1.
 * path_len must equal the total number of loaded symbols (HMMBW_E_INVALID otherwise).
 * Any context (1 <= N <= 64, both topologies); a multi-rank context decodes its own shard, no collective.
 * Leaves the log-likelihoods of hmmbw_get_loglik, the statistics and the training state as they were. */
int hmmbw_viterbi(hmmbw_ctx *ctx, double *logp_out, int32_t *path_out, int64_t path_len);

/* SYNC. Smoothed state posteriors of the loaded sequences under the current parameters:
 *   gamma_t(i) = alpha_t(i) beta_t(i) / P(O)            (hmm_training.py:388-394, linear domain)
 * gamma_dev (DEVICE pointer, may be NULL): [total symbols][N] doubles, row-major, caller CSR order,
 *   gamma_dev[(offsets[r] + t) * N + i]; gamma_len must be total * N.
 * path_out (HOST, may be NULL): int32, caller CSR order, the SMALLEST i attaining max_i gamma_t(i);
 *   path_len must be the total number of loaded symbols.
 * logp_out (HOST, may be NULL): R doubles, log P(O_r | lambda).
 * A sequence with P(O) = 0: logp -inf, every gamma entry 0.0, every path entry -1.  No NaN anywhere.
 * At least one output must be non-NULL.
 * Both lengths are checked whether or not their pointer is NULL (HMMBW_E_INVALID), as hmmbw_viterbi checks
 * path_len.  gamma_dev doubles as the workspace (the forward's scaled alpha rows are overwritten by gamma); without
 * it, a call that asks for the path uses a buffer of the same size that the library keeps until the observations
 * change.  A call that asks for logp_out alone runs the forward recursion only and stores no rows.
 * Any context (1 <= N <= 64, both topologies); a multi-rank context handles its own shard, no collective.
 * Leaves the log-likelihoods of hmmbw_get_loglik, the statistics and the training state as they were. */
int hmmbw_posterior(hmmbw_ctx *ctx, double *gamma_dev, int64_t gamma_len,
                    int32_t *path_out, int64_t path_len, double *logp_out);

/* SYNC. Connected-word decoding of the loaded sequences: the Viterbi path through a loop of n_words word models of
 * the context's shape (N states, M symbols), log domain, fp64.  The bank is given with the call, HOST arrays of
 * linear doubles: pi [W][N], A [W][N][N], B [W][N][M], word weights word_init [W] (NULL: all ones) and
 * word-transition weights word_trans [W][W] (NULL: all ones), any non-negative numbers, not necessarily
 * stochastic: 0 forbids a transition, a common factor is a word-insertion penalty.  Composite state (w, j) has
 * index w N + j:
 *   delta_0(w,j) = (log init_w + log pi_w[j]) + log b_w,j(o_0)
 *   inner_t(w,j) = max_i delta_{t-1}(w,i) + log a_w[i][j]       the SMALLEST i on ties (strict '>' scan from 0)
 *   E_t(w)       = max_v delta_{t-1}(v,N-1) + log G[v][w]       the smallest v on ties
 *   entry_t(w,j) = E_t(w) + log pi_w[j]
 *   delta_t(w,j) = (entry_t > inner_t ? entry_t : inner_t) + log b_w,j(o_t)      the within-word arc wins ties
 * A word is left only from its last state N - 1 and may be re-entered at any state j, weighted by pi_w[j].
 * End state: the smallest composite index attaining max delta_{T-1}; with HMMBW_WORDNET_END_FINAL only the
 * states (w, N - 1) compete.  HMMBW_WORDNET_DENSE forces the dense within-word scan even if every A is
 * left-to-right (a_ij = 0 unless j = i or j = i + 1, detected from the bank).
 * logp_out[r] (R doubles, caller order): the best path's log-probability, -inf if no path has positive
 * probability.  path_out (may be NULL: scores only, no back-pointers are stored): int32, caller CSR order,
 * path_out[offsets[r] + t] = w N + j.  start_out (may be NULL; only together with path_out): uint8, caller CSR
 * order, 1 iff frame t is the first frame of a word instance (t = 0, or the step into t took the entry arc).
 * A sequence whose logp is -inf has path -1 and start 0 throughout.  No NaN anywhere.
 * path_len must equal the total number of loaded symbols (HMMBW_E_INVALID otherwise), as in hmmbw_viterbi.
 * HMMBW_E_INVALID: n_words < 1, a NULL pi, A, B or logp_out, start_out without path_out, a negative, infinite
 * or NaN weight or bank parameter.  HMMBW_E_UNSUPPORTED: n_words > 64, or a context of N > 8.
 * HMMBW_E_STATE: no observations loaded, or an iteration is open (hmmbw_iterate_begin).
 * Needs loaded observations only: it neither reads nor changes the context's parameters, statistics,
 * hmmbw_get_loglik values or training state.  A multi-rank context decodes its own shard, no collective. */
#define HMMBW_WORDNET_END_FINAL 1
#define HMMBW_WORDNET_DENSE     2   /* force the dense within-word scan even if every A is left-to-right */
int hmmbw_wordnet_decode(hmmbw_ctx *ctx, int n_words, const double *pi, const double *A, const double *B,
                         const double *word_init, const double *word_trans, int flags,
                         double *logp_out, int32_t *path_out, uint8_t *start_out, int64_t path_len);

/* SYNC. Embedded training: Baum-Welch re-estimation of a bank of n_words word models of the context's shape (N
 * states, M symbols) from the loaded sequences and their transcripts, the training counterpart of
 * hmmbw_wordnet_decode.  Utterance r was spoken as the words word_ids[word_offsets[r] .. word_offsets[r+1]) (CSR,
 * caller order; a word may occur several times, immediate repeats included); where each word lies is not given.
 * The word models are chained along the transcript, composite state (l, j) for position l and state j:
 *   initial weight  pi_{w_0}[j] on (0, j), 0 elsewhere
 *   within-word arc (l,i) -> (l,j)       of weight a_{w_l}[i][j]
 *   entry arc       (l,N-1) -> (l+1,j)   of weight pi_{w_{l+1}}[j]   (the decoder's entry arc, all word-transition
 *                                        weights 1; it does not share a row sum with the self-loop of (l, N-1))
 *   emission        b_{w_l,j}(o_t)
 *   end             any state of the last instance; with HMMBW_EMBED_END_FINAL only (L-1, N-1).
 * P_r is the total weight of all complete paths.  Per iteration, over the utterances with P_r > 0, every instance
 * of word w adds its posteriors to w's sums: entry[w][j] (gamma_0(0,j) for an instance at l = 0, the entry arcs
 * into (l, j) otherwise: 1 per instance in all), xi[w][i][j] (the within-word arcs), a_den[w][i] = sum_j xi[w][i][j],
 * g_all[w][j] = sum_t gamma_t(l,j), b_num[w][j][k] = sum_{t: o_t = k} gamma_t(l,j); count[w] is the number of
 * instances of w in ALL transcripts (those of utterances with P_r = 0 too: the R of hmm_training.py:424).  Then the
 * reference's M-step (:415-500) per word: pi = entry / count, a = xi / a_den (0 where either is 0), b = b_num / g_all
 * (1e-20 where b_num is 0 and g_all > 0, 0 where g_all is 0); a word with count 0 keeps its parameters bit for bit,
 * whatever `normalise` says.  Convergence as :503-514: L = LSE_r log P_r of the parameters entering the iteration,
 * diff = |L - L_prev| (+inf on the first iteration), stop once diff < epsilon or max_iterations is reached.  All
 * iterations run on the device (an E-step kernel, a per-word M-step kernel and a one-workgroup convergence kernel per
 * iteration, no-ops once a device-side done is set); the host reads the state every 16 iterations.
 * pi [W][N], A [W][N][N], B [W][N][M]: HOST, linear doubles, in: the start bank (working parameters, not necessarily
 * normalised), out: the trained bank.  normalise = 1 applies the reference's return path (:524-541) per trained
 * word (pi / sum pi where the sum is positive; the rows of A and B with a positive sum divided by it); normalise = 0
 * returns the working parameters, so that a second call continues exactly where the first stopped.
 * records (or NULL) gets the first records_cap iterations' records, *n_records (or NULL) the iterations made;
 * logp_out (or NULL): R doubles, log P_r of the LAST E-step, -inf where P_r = 0.  No NaN anywhere.
 * The sums are floating-point atomics: two calls agree to rounding, not bit for bit.  A composite state whose scaled
 * forward (or backward) value is below 2^-1022 of its row's largest is treated as 0.
 * HMMBW_EMBED_DENSE forces the dense within-word products even if every A is left-to-right.
 * HMMBW_E_INVALID: n_words < 1, a NULL bank or transcript pointer, n_seq different from the loaded count, an empty
 * transcript, a word id outside [0, W), a negative, infinite or NaN parameter, max_iterations < 1, epsilon negative
 * or NaN, unknown flag bits.  HMMBW_E_UNSUPPORTED: n_words > 64, a transcript longer than 64 words, a context of
 * N > 8, of world_size > 1 (no collective is built here) or in deterministic mode.  HMMBW_E_STATE: no observations
 * loaded, or an iteration is open (hmmbw_iterate_begin).  HMMBW_E_HIP: the workspace (8 N x 64 bytes per step and
 * wave of 64 / GW utterances, GW the smallest of 8, 16, 32, 64 that holds the longest transcript) could not be
 * allocated; the message names its size.
 * Needs loaded observations only: it neither reads nor changes the context's parameters, statistics,
 * hmmbw_get_loglik values or training state. */
#define HMMBW_EMBED_END_FINAL 1
#define HMMBW_EMBED_DENSE     2   /* force the dense within-word products even if every A is left-to-right */
int hmmbw_embedded_train(hmmbw_ctx *ctx, int n_words,
                         double *pi, double *A, double *B,
                         const int64_t *word_offsets, const int32_t *word_ids, int64_t n_seq,
                         int flags, double epsilon, int64_t max_iterations, int normalise,
                         hmmbw_iter_record *records, int64_t records_cap, int64_t *n_records,
                         double *logp_out);

/* SYNC. Forced alignment of the loaded sequences to their transcripts: the Viterbi path of utterance r through the
 * chain of the word models word_ids[word_offsets[r] .. word_offsets[r+1]) names, the hard-decision counterpart of
 * hmmbw_embedded_train on exactly the same chain, log domain, fp64.  The bank and the transcripts are given as for
 * hmmbw_embedded_train: HOST linear doubles pi [W][N], A [W][N][N], B [W][N][M], not necessarily normalised; CSR
 * transcripts in caller order, a word may repeat, immediately too.  Composite state (l, j) for transcript position
 * l and state j has index l N + j; log 0 = -inf:
 *   delta_0(0,j)  = log pi_{w_0}[j] + log b_{w_0,j}(o_0);   delta_0(l>0, .) = -inf
 *   inner_t(l,j)  = max_i delta_{t-1}(l,i) + log a_{w_l}[i][j]     the SMALLEST i on ties (strict '>' scan from 0)
 *   entry_t(l,j)  = delta_{t-1}(l-1,N-1) + log pi_{w_l}[j]         -inf for l = 0
 *   delta_t(l,j)  = (entry_t > inner_t ? entry_t : inner_t) + log b_{w_l,j}(o_t)   the within-word arc wins ties
 * End state: the smallest j attaining max_j delta_{T-1}(L-1, j); with HMMBW_ALIGN_END_FINAL only (L-1, N-1)
 * competes.  Every instance takes at least one frame, so an utterance with T < L has no path.
 * HMMBW_ALIGN_DENSE forces the dense within-word scan even if every A of the bank is left-to-right.
 * logp_out[r] (R doubles, caller order, required): the best path's log-probability, -inf if no complete path has
 * positive probability.  path_out (may be NULL: scores only, no back-pointers are stored): int32, caller CSR order
 * of the observations, path_out[offsets[r] + t] = l N + j; path_len must equal the total number of loaded symbols,
 * checked whether or not path_out is NULL.  bounds_out (may be NULL; only together with path_out): int32, caller
 * CSR order of the transcripts, bounds_out[word_offsets[r] + l] = the first frame of instance l: 0 for l = 0, else
 * the frame whose step took the entry arc into l; instance l ends where l + 1 starts, the last one at T.
 * bounds_len must equal word_offsets[n_seq], checked either way.  A sequence whose logp is -inf has path -1 and
 * bounds -1 throughout.  No NaN anywhere.  Nothing is summed atomically: two calls return identical bytes, and a
 * context in deterministic mode is accepted.
 * HMMBW_E_INVALID: n_words < 1, a NULL bank, transcript or logp_out pointer, bounds_out without path_out, n_seq
 * different from the loaded count, a wrong path_len or bounds_len, an empty transcript, a word id outside [0, W),
 * offsets that do not start at 0 or decrease, a negative, infinite or NaN bank parameter, unknown flag bits.
 * HMMBW_E_UNSUPPORTED: n_words > 64, a transcript longer than 64 words, a context of N > 8.  HMMBW_E_STATE: no
 * observations loaded, or an iteration is open (hmmbw_iterate_begin).  HMMBW_E_HIP: the back-pointer workspace (256
 * bytes per step and wave of 64 / GW utterances, GW the smallest of 8, 16, 32, 64 that holds the longest
 * transcript) could not be allocated; the message names its size.
 * Needs loaded observations only: it neither reads nor changes the context's parameters, statistics,
 * hmmbw_get_loglik values or training state.  A multi-rank context aligns its own shard, no collective. */
#define HMMBW_ALIGN_END_FINAL 1
#define HMMBW_ALIGN_DENSE     2   /* force the dense within-word scan even if every A is left-to-right */
int hmmbw_align(hmmbw_ctx *ctx, int n_words,
                const double *pi, const double *A, const double *B,
                const int64_t *word_offsets, const int32_t *word_ids, int64_t n_seq,
                int flags,
                double *logp_out, int32_t *path_out, int64_t path_len,
                int32_t *bounds_out, int64_t bounds_len);

/* Optional transcript positions: hmmbw_align and hmmbw_embedded_train on a chain in which some positions may be
 * passed over, as in a transcript `sil? one sil? two sil?` for recordings with pauses nobody marked.  `optional`
 * (HOST) has one byte per transcript position, in the CSR order of word_ids: 1 = a complete path may visit the
 * position or not, 0 = it must.  NULL means no optional position: the call is then the plain entry point's, kernel
 * included.  A complete path visits a subset of the positions, in order, that contains every position with
 * optional = 0; every visited position takes at least one frame and is left from its last state.  So, with
 * x(m) = the value of (m, N-1) one step earlier:
 *   entry sources of (l, j): (l-1, N-1), and also (l-2, N-1) if l >= 2 and optional[l-1]; both of weight pi_{w_l}[j]
 *   start positions:         0, and also 1 if optional[0]
 *   end positions:           L-1, and also L-2 if optional[L-1]; the END_FINAL rule holds per end position.
 * An utterance with fewer frames than mandatory positions has no path.  Transcript rules, else HMMBW_E_INVALID:
 * every flag is 0 or 1, no two adjacent positions are optional, every transcript has a mandatory position (so an
 * optional position 0 implies L >= 2).  Every other argument, check, error and output is the plain entry point's.
 *
 * hmmbw_align_optional: the recursion of hmmbw_align with
 *   entry_t(l,j) = max(delta_{t-1}(l-1,N-1), delta_{t-1}(l-2,N-1) if optional[l-1]) + log pi_{w_l}[j]
 *   delta_0(1,j) = log pi_{w_1}[j] + log b_{w_1,j}(o_0) if optional[0].
 * On any tie the path that skips less wins: the within-word arc beats an entry, as in hmmbw_align; the entry from
 * l-1 beats the one from l-2 (the two sources are compared before the common weight is added); an end in L-1 beats
 * one in L-2.  path_out keeps l N + j with l the index in the transcript as given.  bounds_out is -1 for a position
 * the path passes over (a visited position ends where the next visited one starts), and all -1 where logp is -inf.
 * With paths the workspace grows by 8 bytes per step and wave: a 64-bit lane mask that says which entry source won
 * (the nibble word of the back-pointers is full at N = 8).
 *
 * hmmbw_embedded_train_optional: the same sums with + for max.  alpha_0 is set on every start position; the entry
 * term of (l, j) is (x(l-1) + optional[l-1] x(l-2)) pi_{w_l}[j]; beta_t(l, N-1) gains E_{l+1} + optional[l+1] E_{l+2}
 * with E_m = sum_j pi_{w_m}[j] v_{t+1}(m, j); beta_{T-1} is set on every end position.  entry[w][j] collects gamma_0
 * on the start positions and the posteriors of both kinds of entry arc; the other sums are defined as in
 * hmmbw_embedded_train.  The denominator of pi_w is (mandatory instances of w in ALL transcripts) + present[w], where
 * present[w] is the summed entry mass of the optional instances of w (the probability that the instance is visited)
 * over the utterances with P_r > 0; without optional positions that is count[w].  A word whose denominator is 0 in
 * every iteration keeps its parameters bit for bit, whatever `normalise` says.  Multi-rank and deterministic
 * contexts: HMMBW_E_UNSUPPORTED, as for hmmbw_embedded_train. */
int hmmbw_align_optional(hmmbw_ctx *ctx, int n_words,
                         const double *pi, const double *A, const double *B,
                         const int64_t *word_offsets, const int32_t *word_ids, const uint8_t *optional,
                         int64_t n_seq, int flags,
                         double *logp_out, int32_t *path_out, int64_t path_len,
                         int32_t *bounds_out, int64_t bounds_len);
int hmmbw_embedded_train_optional(hmmbw_ctx *ctx, int n_words,
                                  double *pi, double *A, double *B,
                                  const int64_t *word_offsets, const int32_t *word_ids, const uint8_t *optional,
                                  int64_t n_seq,
                                  int flags, double epsilon, int64_t max_iterations, int normalise,
                                  hmmbw_iter_record *records, int64_t records_cap, int64_t *n_records,
                                  double *logp_out);

/* Engine knobs.  HMMBW_OPT_SAFE_SCALING = 1 forces the per-step power-of-two normalisation of the
 * forward recursion (default 0: lagged normalisation, automatic per-wave fallback to the per-step
 * form when, at one of its rescaling steps, the scaled forward value leaves [2^-450, 2^900], or when the
 * sequence's final value is below 2^-900.  The lower bound keeps the value before the next rescale, which
 * carries the decay of the last sixteen steps, above 2^-900 (runs of symbols at the M-step's 1e-20 floor
 * would otherwise take it into the fp64 denormals); the final value speaks for the steps that no rescaling
 * step follows).  Results agree to fp64 rounding either way (tests/test_gpu_scaling.py). */
#define HMMBW_OPT_SAFE_SCALING 1
/* Diagnostics only (profiling ablations; results are WRONG while nonzero): bit 0 skips the E-step's
 * statistics flush, bit 1 skips its backward sweep, bit 2 skips the separate (unmerged) M-step kernel. */
#define HMMBW_OPT_ABLATE 2
/* Number of statistics accumulator copies the E-step's workgroups spread their atomics over
 * (workgroup b adds into copy b % n; default 2). */
#define HMMBW_OPT_STAT_COPIES 3
/* 1 (default): every M-step runs in the prologue of the next E-step launch, computed redundantly by
 * each workgroup straight into its LDS tables (when the emission tables fit LDS); 0: a separate
 * one-workgroup M-step kernel after every E-step. */
#define HMMBW_OPT_MERGE_MSTEP 4
/* 1: deterministic-reduction mode, bitwise-identical results run to run (no floating-point atomics):
 * gamma goes to per-position rows summed per symbol in a fixed order, and the other statistics are
 * per-workgroup partials summed in workgroup order.  About twice the E-step time on the small
 * kernels; the wide path (16 < N <= 64) already gathers gamma rows, so there it only replaces the
 * other statistics' atomics.  Small state counts need the LDS emission tables (HMMBW_E_UNSUPPORTED
 * otherwise); set it before hmmbw_set_observations (HMMBW_E_STATE after).  Default 0. */
#define HMMBW_OPT_DETERMINISTIC 7
/* Multi-rank all-reduce of the per-iteration statistics: 0 (default) = RCCL (hmmbw_comm_init) or the
 * caller's collective between hmmbw_iterate_begin and _end; 1 = the engine's own peer all-reduce
 * (hmmbw_peer_* below; then _begin/_end do the whole exchange and the caller adds nothing between). */
#define HMMBW_OPT_ALLREDUCE 8
#define HMMBW_ALLREDUCE_RCCL 0
#define HMMBW_ALLREDUCE_PEER 1
/* Bound, in milliseconds, of the peer all-reduce's device-side wait for the other ranks' statistics
 * (default 30000).  Past it the iteration fails with HMMBW_E_TIMEOUT instead of spinning. */
#define HMMBW_OPT_PEER_TIMEOUT_MS 9
/* 1: keep a host mirror of the convergence state that the M-steps update (hmmbw_status_live_wait);
 * 0 (default): off.  Synchronises the context stream when changed. */
#define HMMBW_OPT_LIVE_STATUS 10
/* Bound, in milliseconds, of the wide work queue's device-side wait (16 < N <= 64 with many tiles per CU,
 * HMMBW_OPT_WIDE_WQ): a backward sweep waits for its tile's forward sweep, which runs on a resident
 * workgroup, so the wait always ends; past the bound the iteration fails with HMMBW_E_TIMEOUT (EM stops,
 * the sweep's statistics are not added) instead of reading alpha_hat that may not be there.  Default
 * 10000; 0 expires at once (tests the error path). */
#define HMMBW_OPT_WQ_TIMEOUT_MS 11
/* Wide E-step work queue (a workgroup per forward and per backward sweep of each 16-sequence tile, taken
 * in dispatch order, so the CUs' loads even out in sweeps instead of whole tiles): -1 (default) when the
 * tiles exceed 4 per CU, 1 whenever they exceed the CU count, 0 never.  The environment variable
 * HMMBW_WIDE_WQ=0/1 sets a new context's default.  Takes effect at once. */
#define HMMBW_OPT_WIDE_WQ 12
/* LDS emission-table layout of the joined map's E-step (N = 5..8, at most 256 symbols): the class-split tables,
 * whose emission reads are free of bank conflicts at the price of a larger table build per launch, or the row
 * tables every other kernel uses.  -1 (default): class-split where it measured faster (left-to-right, more
 * sequence groups than SIMDs, a mean of at least 144 steps per group); 0: never; 1: wherever the joined map
 * runs.  HMMBW_INFO_LDS_LAYOUT says what a launch uses.  The environment variable HMMBW_LDS_LAYOUT=-1/0/1 sets
 * a new context's default.  Set it before hmmbw_set_observations (the observations are packed for the layout). */
#define HMMBW_OPT_LDS_LAYOUT 13
int hmmbw_set_option(hmmbw_ctx *ctx, int key, int64_t value);
/* The current value of an option above, or a read-only fact about the loaded observations' E-step launch:
 * HMMBW_INFO_WIDE_WQ_ACTIVE    1 if it runs on the wide work queue;
 * HMMBW_INFO_WAVES             active waves (small kernels: sequence-group waves; wide: tiles x NP/16);
 * HMMBW_INFO_WORKGROUPS        workgroups of the spread map (full + extra); with HMMBW_INFO_JOINED = 1
 *                              the launch itself is HMMBW_INFO_FULL_WORKGROUPS workgroups of twice
 *                              HMMBW_INFO_WAVES_PER_WORKGROUP waves (see HMMBW_INFO_JOINED);
 * HMMBW_INFO_WAVES_PER_WORKGROUP  waves per workgroup of the spread map;
 * HMMBW_INFO_FULL_WORKGROUPS   workgroups with every wave active (small kernels: the spread map puts the
 *                              waves past one per SIMD into workgroups of HMMBW_INFO_EXTRA_WAVES active waves
 *                              after these);
 * HMMBW_INFO_EXTRA_WAVES       active waves of each workgroup after the full ones;
 * HMMBW_INFO_PEER_CHUNKS       chunks of the peer all-reduce payload (each rank writes and polls one flag
 *                              per (rank, chunk) per iteration), 0 without a peer region;
 * HMMBW_INFO_JOINED            1 if the E-step runs the joined map (left-to-right): extra workgroup b's
 *                              waves run as waves 4.. of full workgroup b, one 8-wave workgroup per CU, so
 *                              HMMBW_INFO_FULL_WORKGROUPS workgroups are launched (HMMBW_JOIN=0 turns it off);
 * HMMBW_INFO_SPLIT_EXTRA       1 if the extra workgroups' idle waves run the lower backward half of their
 *                              sequence groups (dense split; HMMBW_SPLIT_EXTRA=0 turns it off);
 * HMMBW_INFO_LDS_LAYOUT        LDS emission-table layout of the E-step launch: 1 the class-split tables (joined
 *                              map, N = 5..8, K <= 256, see HMMBW_OPT_LDS_LAYOUT), 0 the row tables (or none).
 * (bench.py's roofline bounds price the busiest CU and SIMD from this map.) */
#define HMMBW_INFO_WIDE_WQ_ACTIVE 101
#define HMMBW_INFO_WAVES 102
#define HMMBW_INFO_WORKGROUPS 103
#define HMMBW_INFO_WAVES_PER_WORKGROUP 104
#define HMMBW_INFO_FULL_WORKGROUPS 105
#define HMMBW_INFO_EXTRA_WAVES 106
#define HMMBW_INFO_PEER_CHUNKS 107
#define HMMBW_INFO_JOINED 108
#define HMMBW_INFO_SPLIT_EXTRA 109
/* diagnostics: device address of the peer all-reduce's sum buffer (the pending M-step's source), 0 without
 * a peer region (tools/peer_diag.py) */
#define HMMBW_INFO_PEER_SUM_PTR 110
/* process-wide: uncached / fine-grained peer regions validated, and rejected (quarantined) because kernel
 * loads did not read back what was written (see hmmbw.hip, peer_region_alloc) */
#define HMMBW_INFO_PEER_REGIONS_VALIDATED 111
#define HMMBW_INFO_PEER_REGIONS_REJECTED 112
#define HMMBW_INFO_LDS_LAYOUT 113
int hmmbw_get_option(const hmmbw_ctx *ctx, int key, int64_t *value);

/* E-step kernel timing with HIP events on the context stream (for bench/roofline).  Returns the
 * accumulated time and count of the timed launches so far, then (enable >= 0) resets and sets the
 * mode: 0 off, k >= 1 record events around every k-th E-step launch (sampling keeps the event
 * overhead out of the timed loop); enable < 0 only queries. */
int hmmbw_timing(hmmbw_ctx *ctx, int enable, double *total_ms, int64_t *count);
/* The timed launches that run a follow-up kernel after the E-step kernel (the wide path's B-numerator
 * gather, hmm_training.py:474-485; deterministic mode's fixed-order reductions): the accumulated time of
 * the E-step kernel alone and the count (same reset as hmmbw_timing).  bench.py prices the fp64-MFMA
 * bound on it. */
int hmmbw_timing_split(hmmbw_ctx *ctx, double *estep_ms, int64_t *count);

/* Vector-quantisation encoder: get_observations, hmm_training.py:82-120.  For every frame f, the index
 * of the nearest centroid (first minimum, strict '<' as at :111) by the Euclidean distance over the
 * columns [first_dim, first_dim + dims) of frames[f * frame_stride ...] and centroids[k * frame_stride
 * ...] (the reference: stride 13, first_dim 1 — mfcc[1:] without the power coefficient — dims 12),
 * computed exactly as np.linalg.norm does (sequential fused multiply-add, correctly rounded sqrt), so
 * the indices are bit-identical to the reference's.  DEVICE pointers (frames [n_frames][stride],
 * centroids [n_centroids][stride] fp64, symbols int32 [n_frames], distances fp64 [n_frames] or NULL:
 * the winning distance, the reference's min_distance); enqueued on `stream` (hipStream_t, NULL =
 * legacy default), asynchronous; the device is the current one.  Codebook <= 160 KiB. */
int hmmbw_vq_encode(void *stream, const double *frames, int64_t n_frames, int frame_stride, int first_dim, int dims,
                    const double *centroids, int n_centroids, int32_t *symbols, double *distances);

/* ---- LBG codebook training: the step that produces the codebook hmmbw_vq_encode reads ----
 * createCodeVector, CodeVector/codevector_functions.py:442-531 (the MFCC variant): c0 is the mean of all frames over
 * all frame_stride columns; each of the G = log2(n_centroids) generations starts from the split of the one before
 * (row i -> rows 2i = c * split_up and 2i + 1 = c * split_down, the reference's 1.001 and 0.999) and repeats
 * "assign every frame to its nearest centroid over the columns [first_dim, first_dim + dims) (hmmbw_vq_encode's
 * arithmetic and tie rule), distortion = sum of the winning distances, centroid k = mean over all columns of its
 * frames (zeros when it has none), diff = |previous distortion - distortion|" while diff > epsilon and fewer than
 * max_iterations passes were made; a NaN diff ends the generation, as in the reference.  The order in which the
 * centroid sums and the distortion are added up is unspecified (floating-point atomics).
 * All passes run on the device: an assign-and-accumulate kernel and a one-workgroup update kernel per pass, the
 * latter advancing a device-side state (generation, pass, previous distortion, centroids in use, done); the host
 * enqueues passes in chunks and reads the state between chunks.
 * DEVICE pointers: frames [n_frames][frame_stride]; centroids [n_centroids][frame_stride], the last generation;
 * generations (or NULL) [2 n_centroids - 1][frame_stride]: c0, then generation 1 (2 rows), ... generation G, each as
 * it stood at the end of its loop; assignments (or NULL) int32 [n_frames]: the LAST pass's, made against the
 * centroids before the last update.  HOST: records (or NULL) gets the first records_cap passes, *n_records (or NULL)
 * the number of passes made.  SYNCHRONOUS on `stream` (hipStream_t, NULL = legacy default); the device is the
 * current one; the workspace comes from the library's block cache.
 * HMMBW_E_INVALID: n_frames < 1, n_centroids not a power of two >= 2, dims < 1, first_dim < 0, first_dim + dims >
 * frame_stride, max_iterations < 1, epsilon negative or NaN, frames or centroids NULL.  HMMBW_E_UNSUPPORTED: the per-workgroup LDS, 8 (1 + n_centroids (frame_stride + 1)) bytes of
 * accumulators plus, for dims != 12, the staged codebook 8 n_centroids dims, exceeds 160 KiB (n_centroids = 1024
 * at stride 13 and dims 12 takes 112 KiB); dims > 64 other than through the dims == 12 scan. */
typedef struct {
    int32_t generation; /* 1 .. G */
    int32_t iteration;  /* pass within the generation, from 1 */
    double distortion;  /* sum of the winning distances of the pass */
    double diff;        /* |distortion of the pass before - distortion| (0 before a generation's first) */
} hmmbw_lbg_record;
int hmmbw_lbg_train(void *stream, const double *frames, int64_t n_frames, int frame_stride, int first_dim, int dims,
                    int n_centroids, double epsilon, int64_t max_iterations, double split_up, double split_down,
                    double *centroids, double *generations, int32_t *assignments,
                    hmmbw_lbg_record *records, int64_t records_cap, int64_t *n_records);

/* ---- MFCC front end: the rows hmmbw_vq_encode and hmmbw_lbg_train read ----
 * RawDataMFCC.calculate_mfcc, CodeVector/codevector_classes.py:226-250: librosa.feature.mfcc(y = frame, sr, n_mfcc,
 * n_fft = len(frame), hop_length = None, center = False, n_mels), one call per frame there.  For a frame x of L =
 * frame_len samples (one STFT column, no padding):
 *   y[n] = x[n] window[n];  P[k] = |sum_n y[n] exp(-2 pi i k n / L)|^2, k = 0 .. L/2;  M[m] = sum_k mel[m][k] P[k];
 *   dB[m] = 10 log10(max(amin, M[m])), then dB[m] = max(dB[m], max_m dB - top_db) unless top_db < 0 (floor off);
 *   out[f * out_stride + i] = sum_m dct[i][m] dB[m], i = 0 .. n_mfcc - 1.
 * A frame with a NaN or +-Inf sample gets n_mfcc zeros (librosa rejects such audio and calculate_mfcc keeps its
 * zeros, :247-250); its neighbours are not affected.  A silent frame gives dB = 10 log10(amin) throughout.
 * The tables are arguments, not constants of the kernel.  hmmbw_mfcc_tables fills HOST arrays with librosa's
 * defaults: window [frame_len], the periodic Hann window; twiddle [frame_len][2], cos and sin of 2 pi m / frame_len;
 * mel [n_mels][frame_len / 2 + 1], the Slaney-scale, Slaney-normalised filter bank from 0 to sample_rate / 2, each
 * weight a float32 value as librosa stores it; dct [n_mfcc][n_mels], the first rows of the orthonormal DCT-II.
 * HMMBW_E_INVALID: frame_len < 2, sample_rate <= 0 or NaN, n_mels < 1, n_mfcc < 1 or > n_mels, a null pointer;
 * HMMBW_E_UNSUPPORTED: frame_len > 512 or n_mels > 64. */
int hmmbw_mfcc_tables(int frame_len, double sample_rate, int n_mels, int n_mfcc, double *window, double *twiddle,
                      double *mel, double *dct);
/* DEVICE pointers throughout: samples fp64 [n_samples]; frame_starts int64 [n_frames], offsets into samples (frames
 * may overlap: they are views, never copies); the four tables as hmmbw_mfcc_tables lays them out; out fp64, row f at
 * out + f * out_stride with out_stride >= n_mfcc (13 writes straight into a stride-13 frame buffer; the columns past
 * n_mfcc are not touched).  One call serves one frame length.  Enqueued on `stream` (hipStream_t, NULL = legacy
 * default); the device is the current one.  The frame table is on the device, so the call first runs a range check
 * over it on `stream` and waits for its 4-byte answer; the MFCC kernel itself is then enqueued and the call returns
 * without waiting for it, as hmmbw_vq_encode does.
 * HMMBW_E_INVALID: a null pointer, n_frames < 0, frame_len < 2, a frame that starts before 0 or runs past n_samples,
 * n_mels < 1, n_mfcc < 1 or > n_mels, out_stride < n_mfcc, amin <= 0 or NaN.  HMMBW_E_UNSUPPORTED: frame_len > 512
 * or n_mels > 64 (the 16-frame tile's LDS).  n_frames == 0 returns HMMBW_OK and launches nothing. */
int hmmbw_mfcc(void *stream, const double *samples, int64_t n_samples, const int64_t *frame_starts, int64_t n_frames,
               int frame_len, const double *window, const double *twiddle, const double *mel, int n_mels,
               const double *dct, int n_mfcc, double amin, double top_db, double *out, int64_t out_stride);

/* ---- Signal conditioning: the processed signal hmmbw_mfcc reads, from the raw recording ----
 * The reference's preemphasis.py (filter_signal :174-183, slice_signal :222-294) and, for the live recogniser,
 * HMM/live_testing.py (slice_signal :48-120 with two pairs of thresholds, do_preemphasis :163-184) with
 * preemphasis.hamming_window (:189-212).  All arithmetic is fp64.  For a recording x[0 .. n):
 *   filter  y[0] = 0, y[i] = x[i] - fl(coeff x[i-1]): the product rounded on its own, never fused into the subtraction
 *           (the reference's bits for int16 and float64 recordings; its float32 arithmetic for a float32 recording
 *           under NumPy 2 is not reproduced: upload such a recording as doubles);
 *   frames  nf = trunc((n - win) / hop) + 1; frame i < nf - 1 is y[i hop, i hop + win), the last one y[(nf - 1) hop,
 *           n - 1): it spares the last sample and has win - 1 .. win + hop - 2 samples;
 *           power[i] = sum f^2 / len(f), zcr[i] = 1/2 sum_j |sign(f[j+1]) - sign(f[j])|, sign(0) = 0;
 *   bounds  factors = (zf, pf, zl, pl); keep_first[i] = zcr[i] > zf max zcr and power[i] > pf max power, keep_last the
 *           same with (zl, pl), all comparisons strict, a negative zcr factor switching that test off.  If a frame
 *           passes keep_first: first = the first of them, last = the LAST frame that passes keep_last (first, if none
 *           does: the reference raises there); otherwise first = 0, last = nf.  bounds_out[r] = (first hop, last hop),
 *           relative to the recording and never past n: the end is the START of the last kept frame, as in the
 *           reference.  Batch mode (preemphasis.py) is (-1, 0.015, -1, 0.015), live mode (0.08, 0.15, 0.03, 0.10).
 * hmmbw_preprocess: DEVICE pointers samples (fp64 for HMMBW_SAMPLES_F64, int16 for HMMBW_SAMPLES_I16: a .wav file's own
 * samples, a quarter of the bytes to upload), rec_offsets int64 [n_rec + 1] ascending from 0, filtered_out fp64, one
 * value per input sample, not overlapping samples: y of every whole recording (nothing is compacted; the trimmed signal is the slice bounds_out
 * names), bounds_out int64 [n_rec][2], stats_out fp64 [sum nf][2] (zcr, power) per frame in recording order, or NULL.
 * factors is a HOST array of 4.  rec_offsets_host is a HOST copy of rec_offsets or NULL: with it the call checks the
 * lengths before it launches anything; without it a recording that has no frame gets bounds (0, 0) and no row of
 * stats_out.  One kernel on `stream` (hipStream_t, NULL = legacy default), one workgroup per recording; nothing waits
 * on the host.  No index leaves a recording's [rec_offsets[r], rec_offsets[r+1]) whatever the samples are; with
 * non-finite samples the statistics and bounds are unspecified (but within the recording).  A requested stats_out
 * costs every workgroup a pass over the offsets before it.
 * HMMBW_E_INVALID: a null pointer (but stats_out, rec_offsets_host), n_rec < 0, an unknown sample_kind, win < 2,
 * hop < 1, hop > win, a NaN coefficient or factor; with rec_offsets_host: offsets that do not ascend from 0, a
 * recording with nf < 1 (n <= win - hop; 160 samples at 16 kHz) or n < 2: the reference raises there too.
 * HMMBW_E_UNSUPPORTED: win > 65536, n_rec >= 2^31, more than 2^46 samples.  n_rec == 0 returns HMMBW_OK. */
#define HMMBW_SAMPLES_F64 0
#define HMMBW_SAMPLES_I16 1
int hmmbw_preprocess(void *stream, const void *samples, int sample_kind, const int64_t *rec_offsets,
                     const int64_t *rec_offsets_host, int64_t n_rec, double coeff, int win, int hop,
                     const double *factors, double *filtered_out, int64_t *bounds_out, double *stats_out);
/* The live recogniser's overlapping window, in place on t = samples[rec_offsets[r] + start_r, .. + finish_r) of m
 * samples, (start, finish) read from the DEVICE array bounds [n_rec][2] (hmmbw_preprocess's bounds_out: the two calls
 * go back to back on one stream), with the DEVICE table window [wlen]:
 *   q = trunc((m - wlen) / whop) + 1;  for i < q: t[i whop, i whop + wlen) *= window (clipped to m);
 *   if q >= 0: t[q whop, m - 1) *= window[0 ..): a partial frame that spares the last sample;  q < 0: nothing.
 * Per sample that is a product over the frames that cover it, taken in ascending frame order, which reproduces the
 * reference's in-place loop bit for bit.  Samples outside [start, finish) are not touched; bounds that do not lie
 * within their recording touch nothing.
 * HMMBW_E_INVALID: a null pointer, n_rec < 0, wlen < 1, whop < 1.  HMMBW_E_UNSUPPORTED: ceil(wlen / whop) > 8,
 * wlen > 65536, n_rec >= 2^31.  n_rec == 0 returns HMMBW_OK. */
int hmmbw_window_overlap(void *stream, double *samples, const int64_t *rec_offsets, const int64_t *bounds,
                         int64_t n_rec, const double *window, int wlen, int whop);

/* ---- Groups: several models of one shape, one launch per EM iteration / per scoring pass ----
 * The reference trains its word models one after another (train_hmm, HMM/main.py:147-152, calling
 * training_with_save -> hmm_training once per word, hmm_training.py:215-247) and scores every
 * (recording, model) pair with its own forward pass (test_hmm, HMM/hmm_testing.py:139-161).  A group
 * advances all member contexts with ONE grouped E-step launch per iteration (each member's M-step runs
 * in its slice's prologue; each member keeps its own parameters, statistics, convergence state and
 * stop rule, exactly as if trained alone) and scores all of them with one launch.
 * Members: single-rank contexts on the same device and stream, with equal N, M and resolved topology,
 * N <= 16 and emission tables that fit LDS, each with observations and parameters set (checked at
 * creation, HMMBW_E_UNSUPPORTED otherwise, and again at every call, where a member that no longer fits
 * is refused before any member is touched); the group does not own them (destroy the group first).
 * A member may hold no sequences (hmmbw_set_observations with R = 0): it is accepted, owns no workgroup
 * of the grouped launches and does exactly what hmmbw_iterate and hmmbw_score do for it alone: every
 * iteration records L = -inf and diff = +inf and re-estimates all-zero parameters until max_iterations,
 * and it adds nothing to hmmbw_group_score's output.  Its M-step cannot run in a slice's prologue, so a
 * group with such a member iterates one launch at a time (tests/test_gpu_group_shapes.py). */
typedef struct hmmbw_group hmmbw_group;
int hmmbw_group_create(hmmbw_ctx *const *ctxs, int n, hmmbw_group **out);
int hmmbw_group_destroy(hmmbw_group *group);
/* hmmbw_iterate(ctx, n_iter) for every member (arm each with hmmbw_reset_training first). */
int hmmbw_group_iterate(hmmbw_group *group, int64_t n_iter);
/* SYNC. hmmbw_score of every member, concatenated in member order (sum of the members' R doubles). */
int hmmbw_group_score(hmmbw_group *group, double *out);
/* Timing of the grouped E-step launches (same protocol as hmmbw_timing). */
int hmmbw_group_timing(hmmbw_group *group, int enable, double *total_ms, int64_t *count);

#ifdef __cplusplus
}
#endif
#endif /* HMMBW_H */
