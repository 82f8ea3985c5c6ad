"""The checker of the optional-position tests (hmmbw_align_optional, hmmbw_embedded_train_optional of
include/hmmbw.h): a plain NumPy restatement from the definitions.  The chain of embedded_ref.composite gets the skip
arcs (l-2, N-1) -> (l, j) past an optional position l-1, a second start block when position 0 is optional and a
second end block when position L-1 is; then a generic scaled forward-backward and a generic log-domain Viterbi run
over the explicit matrices.  The Viterbi takes a rank per arc and per end state for the tie rule "the path that
skips less wins" and carries a margin, as align_ref.align does.  Also the pooled statistics with the `present`
denominator, the M-step and the training loop, the expansions of a transcript (every complete path visits a
definite subset of the optional positions), and the cases the GPU tests share.  Dense matrices, no lanes."""
import itertools

import numpy as np

import align_ref as AR
import embedded_ref as ER
from viterbi_ref import MARGIN, RTOL, _gap  # noqa: F401  (the project's tolerances)


def check_transcript(opt):
    """0 ok, 1 a flag other than 0 or 1, 2 adjacent optional positions, 3 no mandatory position."""
    opt = [int(x) for x in opt]
    if any(x not in (0, 1) for x in opt):
        return 1
    if any(a and b for a, b in zip(opt, opt[1:])):
        return 2
    return 3 if all(opt) else 0


def composite(words, opt, pi, A, B, end_final=False):
    """(init [S], trans [S, S], emis [S, K], end [S], rank [S, S], end_rank [S]) of the chain with optional
    positions.  rank orders the arcs into a state for ties (smaller wins): the within-word arc from state i has rank
    i, the entry from l-1 rank N, the entry from l-2 rank N + 1; end_rank: j in L-1, N + j in L-2."""
    assert check_transcript(opt) == 0 and len(opt) == len(words)
    N = pi.shape[1]
    L = len(words)
    init, trans, emis, end = ER.composite(words, pi, A, B, end_final)
    S = L * N
    rank = np.zeros((S, S), dtype=np.int64)
    for l in range(L):
        rank[l * N:(l + 1) * N, l * N:(l + 1) * N] = np.arange(N)[:, None]
        if l >= 1:
            rank[l * N - 1, l * N:(l + 1) * N] = N
        if l >= 2 and opt[l - 1]:
            trans[(l - 1) * N - 1, l * N:(l + 1) * N] = pi[words[l]]        # the skip arc
            rank[(l - 1) * N - 1, l * N:(l + 1) * N] = N + 1
    if opt[0]:
        init[N:2 * N] = pi[words[1]]                                        # the second start block
    end_rank = np.zeros(S, dtype=np.int64)
    end_rank[S - N:] = np.arange(N)
    if opt[L - 1]:                                                          # the second end block
        if end_final:
            end[S - N - 1] = 1.0
        else:
            end[S - 2 * N:S - N] = 1.0
        end_rank[S - 2 * N:S - N] = N + np.arange(N)
    return init, trans, emis, end, rank, end_rank


def fb(obs, init, trans, emis, end):
    """The scaled forward-backward of embedded_ref.forward_backward on explicit matrices: (log P, alpha [T, S],
    vb [T-1, S], gamma [T, S]) or (-inf, None, None, None) where P = 0."""
    obs = np.asarray(obs).reshape(-1)
    T, S = obs.size, init.size
    dead = (-np.inf, None, None, None)
    alpha, scale = np.zeros((T, S)), np.zeros(T)
    for t in range(T):
        a = (init if t == 0 else alpha[t - 1] @ trans) * emis[:, obs[t]]
        scale[t] = a.sum()
        if not scale[t] > 0.0:
            return dead
        alpha[t] = a / scale[t]
    tail = float(alpha[T - 1] @ end)
    if not tail > 0.0:
        return dead
    logp = float(np.log(scale).sum() + np.log(tail))
    beta, vb = np.zeros((T, S)), np.zeros((max(T - 1, 0), S))
    beta[T - 1] = end / tail
    for t in range(T - 2, -1, -1):
        vb[t] = emis[:, obs[t + 1]] * beta[t + 1] / scale[t + 1]
        beta[t] = trans @ vb[t]
    return logp, alpha, vb, alpha * beta


def viterbi(obs, init, trans, emis, end, rank, end_rank):
    """(path [T] of composite states, logp, margin) of the generic log-domain Viterbi; path None where logp = -inf.
    Among equal candidates the one of the smallest rank wins.  margin: the smallest best-minus-second-best gap over
    the decisions on the best path, the end state included."""
    obs = np.asarray(obs).reshape(-1)
    with np.errstate(divide="ignore"):
        linit, ltrans, lemis = np.log(init), np.log(trans), np.log(emis)
    T, S = obs.size, init.size
    big = np.iinfo(np.int64).max

    def pick(c, rk):
        """Per column of c [n, m]: (row of the largest entry, the smallest rank among equals; best minus second)."""
        best = c.max(axis=0)
        arg = np.argmin(np.where(c == best, rk, big), axis=0)
        if c.shape[0] < 2:
            return arg, np.full(c.shape[1], np.inf)
        second = np.partition(c, -2, axis=0)[-2]
        with np.errstate(invalid="ignore"):
            gap = np.where(second == -np.inf, np.inf, best - second)
        return arg, gap

    delta = linit + lemis[:, obs[0]]
    psi, gaps = np.zeros((T, S), dtype=np.int64), np.full((T, S), np.inf)
    for t in range(1, T):
        c = delta[:, None] + ltrans                         # c[s, s']
        psi[t], gaps[t] = pick(c, rank)
        delta = c.max(axis=0) + lemis[:, obs[t]]
    ends = np.flatnonzero(end > 0)
    k, gap = pick(delta[ends, None], end_rank[ends, None])
    s = int(ends[k[0]])
    logp = float(delta[s])
    if logp == -np.inf:
        return None, logp, np.inf
    margin = float(gap[0])
    path = np.zeros(T, dtype=np.int32)
    for t in range(T - 1, 0, -1):
        path[t] = s
        margin = min(margin, float(gaps[t, s]))
        s = int(psi[t, s])
    path[0] = s
    return path, logp, margin


def bounds_of(path, L, N):
    """The first frame of every visited position, -1 for the others."""
    b = np.full(L, -1, dtype=np.int32)
    pos = np.asarray(path) // N
    for t in range(len(pos) - 1, -1, -1):
        b[pos[t]] = t
    return b


def align(obs, words, opt, pi, A, B, end_final=False):
    """(path int32 [T], bounds int32 [L], logp, margin) of one utterance: hmmbw_align_optional."""
    pi, A, B = np.asarray(pi, float), np.asarray(A, float), np.asarray(B, float)
    T, L, N = len(obs), len(words), pi.shape[1]
    path, logp, margin = viterbi(obs, *composite(words, opt, pi, A, B, end_final))
    if path is None:
        return np.full(T, -1, dtype=np.int32), np.full(L, -1, dtype=np.int32), logp, np.inf
    return path, bounds_of(path, L, N), logp, margin


def align_all(obs, transcripts, optional, pi, A, B, end_final=False):
    out = [align(o, ws, f, pi, A, B, end_final) for o, ws, f in zip(obs, transcripts, optional)]
    return ([x[0] for x in out], [x[1] for x in out], np.array([x[2] for x in out]), np.array([x[3] for x in out]))


def expansions(opt):
    """Every subset of the positions that keeps the mandatory ones, as sorted index lists."""
    free = [l for l, f in enumerate(opt) if f]
    fixed = [l for l, f in enumerate(opt) if not f]
    out = []
    for n in range(len(free) + 1):
        for extra in itertools.combinations(free, n):
            out.append(sorted(fixed + list(extra)))
    return out


def path_logp(path, obs, words, opt, pi, A, B):
    """log-probability of one labelling (composite states l N + j), arc by arc: a step that keeps the position is a
    within-word arc; a step to a later position is an entry arc, -inf unless it leaves a last state and passes over
    at most one position, an optional one; the path starts in position 0, or in 1 past an optional 0."""
    lpi, lA, lB = AR.log_bank(pi, A, B)
    N = lpi.shape[1]
    l, j = divmod(int(path[0]), N)
    ok = l == 0 or (l == 1 and opt[0])
    v = (lpi[words[l], j] if ok else -np.inf) + lB[words[l], j, obs[0]]
    for t in range(1, len(path)):
        pl, pj = l, j
        l, j = divmod(int(path[t]), N)
        if l == pl:
            arc = lA[words[l], pj, j]
        elif pj == N - 1 and (l == pl + 1 or (l == pl + 2 and opt[pl + 1])):
            arc = lpi[words[l], j]
        else:
            arc = -np.inf
        v = (v + arc) + lB[words[l], j, obs[t]]
    return float(v)


def check_align(obs, transcripts, optional, bank_, paths, bounds, logp, end_final=False, min_clear=0.95):
    """An alignment against the checker: logp to RTOL, -inf and -1 in the same places; every labelling valid (it
    re-scores arc by arc to its logp, ends in an end position, bounds consistent with the path); path and bounds
    exactly where the checker's margin exceeds MARGIN, after asserting from the checker alone that min_clear of the
    finite sequences clear it.  Returns the checker's (paths, bounds, logp, margin)."""
    pi, A, B = bank_
    N = np.asarray(pi).shape[1]
    rpaths, rbounds, rlogp, margin = align_all(obs, transcripts, optional, pi, A, B, end_final)
    finite = rlogp > -np.inf
    clear = margin > MARGIN
    if finite.any():
        frac = clear[finite].mean()
        assert frac >= min_clear, f"only {frac:.3f} of the finite sequences clear the margin (checker alone)"
    logp = np.asarray(logp)
    assert logp.shape == rlogp.shape and not np.any(np.isnan(logp))
    assert np.array_equal(logp == -np.inf, ~finite)
    np.testing.assert_allclose(logp, rlogp, rtol=RTOL)
    assert len(paths) == len(bounds) == len(obs)
    for r, (p, b, o, ws, f) in enumerate(zip(paths, bounds, obs, transcripts, optional)):
        assert p.dtype == np.int32 and b.dtype == np.int32 and p.shape == (len(o),) and b.shape == (len(ws),), r
        if not finite[r]:
            assert np.all(p == -1) and np.all(b == -1), r
            continue
        L = len(ws)
        assert np.all((p >= 0) & (p < L * N)), r
        np.testing.assert_allclose(path_logp(p, o, ws, f, pi, A, B), logp[r], rtol=RTOL)
        last = int(p[-1]) // N
        assert last == L - 1 or (last == L - 2 and f[L - 1]), r
        if end_final:
            assert p[-1] % N == N - 1, r
        assert np.array_equal(b, bounds_of(p, L, N)), r
        assert all(b[l] >= 0 for l in range(L) if not f[l]), r
        if clear[r]:
            assert np.array_equal(p, rpaths[r]) and np.array_equal(b, rbounds[r]), r
    return rpaths, rbounds, rlogp, margin


# --------------------------------------------------------------------------------------------------------------
# embedded training
# --------------------------------------------------------------------------------------------------------------
def forward_backward(obs, words, opt, pi, A, B, end_final=False):
    init, trans, emis, end = composite(words, opt, np.asarray(pi, float), np.asarray(A, float), np.asarray(B, float),
                                       end_final)[:4]
    return fb(obs, init, trans, emis, end) + (trans,)


def estep(obs, transcripts, optional, pi, A, B, end_final=False):
    """(Stats, logp [R], mand [W], present [W]): embedded_ref.estep's sums on the chain with optional positions.
    mand counts the mandatory instances in all transcripts, present sums the entry mass of the optional ones over
    the utterances with P > 0.  Stats.count is left at 0: the M-step takes mand + present."""
    pi, A, B = np.asarray(pi, float), np.asarray(A, float), np.asarray(B, float)
    W, N = pi.shape
    st = ER.Stats(W, N, B.shape[2])
    mand, present = np.zeros(W, dtype=np.int64), np.zeros(W)
    logp = np.zeros(len(obs))
    for r, (o, words, f) in enumerate(zip(obs, transcripts, optional)):
        o = np.asarray(o).reshape(-1)
        for w, x in zip(words, f):
            mand[w] += 0 if x else 1
        logp[r], alpha, vb, gamma, trans = forward_backward(o, words, f, pi, A, B, end_final)
        if gamma is None:
            continue
        for l, w in enumerate(words):
            sl = slice(l * N, (l + 1) * N)
            g = gamma[:, sl]
            st.g_all[w] += g.sum(axis=0)
            np.add.at(st.b_num[w].T, o, g)
            st.xi[w] += trans[sl, sl] * (alpha[:-1, sl].T @ vb[:, sl])
            mass = np.zeros(N)
            if l == 0 or (l == 1 and f[0]):
                mass += g[0]
            if l >= 1:
                mass += trans[l * N - 1, sl] * (alpha[:-1, l * N - 1] @ vb[:, sl])
            if l >= 2 and f[l - 1]:
                src = (l - 1) * N - 1
                mass += trans[src, sl] * (alpha[:-1, src] @ vb[:, sl])
            st.entry[w] += mass
            if f[l]:
                present[w] += mass.sum()
    return st, logp, mand, present


def train(obs, transcripts, optional, pi, A, B, epsilon=0.0, max_iterations=1, end_final=False, normalise=False):
    """(pi, A, B, records, logp of the last E-step, touched [W]): embedded_ref.train with the denominator of pi
    mand + present; a word whose denominator is 0 keeps its parameters; touched marks the words re-estimated in
    some iteration, the only ones `normalise` touches."""
    pi, A, B = np.array(pi, float), np.array(A, float), np.array(B, float)
    prev, records = -np.inf, []
    it, diff = 0, np.inf
    logp = None
    touched = np.zeros(pi.shape[0], dtype=bool)
    while diff >= epsilon and it < max_iterations:
        st, logp, mand, present = estep(obs, transcripts, optional, pi, A, B, end_final)
        st.count = mand + present                      # embedded_ref.mstep: pi = entry / count where count > 0
        touched |= st.count > 0
        pi, A, B = ER.mstep(st, pi, A, B)
        L = ER.lse(logp)
        diff = abs(L - prev) if prev != -np.inf else np.inf
        prev = L
        records.append((L, diff))
        it += 1
    if normalise:
        pi, A, B = ER.normalised(pi, A, B, touched.astype(int))
    return pi, A, B, records, logp, touched


# --------------------------------------------------------------------------------------------------------------
# what the tests share
# --------------------------------------------------------------------------------------------------------------
def with_sil(words, sil, keep):
    """`sil? w sil? w ... sil?` with the optional position before word i present where keep[i] (keep has L + 1
    entries, the last one the position after the last word): (words, opt)."""
    out, opt = [], []
    for i, w in enumerate(list(words) + [None]):
        if keep[i]:
            out.append(sil)
            opt.append(1)
        if w is not None:
            out.append(int(w))
            opt.append(0)
    return out, opt


def case(W, N, K, topology, longest, seed, plain_every=3):
    """(obs, transcripts, optional, (pi, A, B)) as align_ref.case: word W - 1 is the silence, the others are drawn
    without immediate repeats (so that a one-state word does not repeat after a skip either, and the optional word
    differs from its neighbours); the first transcript has exactly `longest` positions with optional ones at 0 and
    L - 1 when longest is odd, every plain_every-th transcript has no optional position at all (waves mix both
    kinds), and R is no multiple of the slots per wave.  T: 7, 8, 9, 17 and the mandatory count occur."""
    from viterbi_ref import sequences
    from wordnet_ref import bank
    rng = np.random.default_rng(seed)
    pi, A, B, _, _ = bank(W, N, K, topology, rng)
    sil = W - 1
    spw = 64 // AR.gw_of(longest)
    R = 2 * spw + 3 + (spw == 1)                      # at least six: four fixed lengths, the first and the last

    def draw(n):
        ws = [int(x) for x in rng.integers(0, W - 1, size=n)]
        for i in range(1, n):
            if ws[i] == ws[i - 1]:
                ws[i] = (ws[i] + 1) % (W - 1)
        return ws

    def cap(r):
        return 7 if 1 <= r <= 4 else longest          # utterances 1 .. 4 get T = 7, 8, 9, 17: at most 7 mandatory words

    transcripts, optional = [], []
    for r in range(R):
        if r == 0:
            n = (longest - 1) // 2 if longest % 2 else longest // 2
            n = max(n, 1)
            keep = [True] * (n + 1)
            if longest % 2 == 0:
                keep[0] = False                       # an even length: no optional position 0
            if longest == 1:
                keep = [False, False]
            ws, f = with_sil(draw(n), sil, keep)
            assert len(ws) == longest
        elif r % plain_every == 0:
            ws = draw(int(rng.integers(1, min(longest, cap(r)) + 1)))
            f = [0] * len(ws)
        else:
            n = int(rng.integers(1, min(max((longest - 1) // 2, 1), cap(r)) + 1))
            ws, f = with_sil(draw(n), sil, [bool(x) for x in rng.integers(0, 2, size=n + 1)])
        transcripts.append(ws)
        optional.append(f)
    lens = [len(t) for t in transcripts]
    mand = [len(t) - sum(f) for t, f in zip(transcripts, optional)]
    T = [int(rng.integers(m, 3 * L * N + 1)) for m, L in zip(mand, lens)]
    for r, t in zip(range(1, R), (7, 8, 9, 17)):
        T[r] = max(t, mand[r])
    T[R - 1] = mand[R - 1]                            # every optional position passed over
    T[0] = min(3 * longest * N, 3 * 64)               # the longest chain, long enough to visit every position
    T[0] = max(T[0], lens[0])
    return sequences(T, K, rng), transcripts, optional, (pi, A, B)


def disjoint_case(W, N, n_seq, seed, max_words=4, noise=0.0):
    """The exact-recovery data: W - 1 words and a silence (word W - 1), state j of word w emits symbol w N + j only
    (noise = 0), every state held 1-4 frames; a pause of the silence's N states is present before, between and
    after the words with probability 1/2 each.  Returns (obs, words, truth) with truth[r] = [(word, start, end)]
    of the generated segments, the pauses that are present included."""
    rng = np.random.default_rng(seed)
    K = W * N
    sil = W - 1
    obs, words, truth = [], [], []
    for r in range(n_seq):
        n = int(rng.integers(1, max_words + 1))
        ws = [int(x) for x in rng.integers(0, W - 1, size=n)]
        o, seg = [], []

        def emit(w):
            s = len(o)
            for j in range(N):
                for _ in range(int(rng.integers(1, 5))):
                    k = w * N + j
                    if noise and rng.random() < noise:
                        k = int((k + rng.integers(1, K)) % K)
                    o.append(k)
            seg.append((w, s, len(o)))

        for i, w in enumerate(ws):
            if rng.random() < 0.5:
                emit(sil)
            emit(w)
        if rng.random() < 0.5:
            emit(sil)
        obs.append(np.array(o))
        words.append(ws)
        truth.append(seg)
    return obs, words, truth


def disjoint_bank(W, N, rng):
    """Left-to-right models entered at state 0, stay probabilities in [0.5, 0.7]; state j of word w emits symbol
    w N + j and nothing else."""
    K = W * N
    pi = np.zeros((W, N))
    pi[:, 0] = 1.0
    A = np.zeros((W, N, N))
    stay = rng.uniform(0.5, 0.7, size=(W, N))
    for j in range(N):
        A[:, j, j] = stay[:, j]
        if j < N - 1:
            A[:, j, j + 1] = 1.0 - stay[:, j]
    B = np.zeros((W, N, K))
    for w in range(W):
        for j in range(N):
            B[w, j, w * N + j] = 1.0
    return pi, A, B
