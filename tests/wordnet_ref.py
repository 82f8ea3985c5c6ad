"""The checker of the connected-word decoding tests: a plain NumPy restatement of the word-loop recursion of
include/hmmbw.h (hmmbw_wordnet_decode), with its tie rules: np.log with log 0 = -inf, the first maximum for the
within-word predecessor i, for the entry source v and for the end state, the within-word arc on a tie with the
entry arc, and a path of -1 / start of 0 where no path has positive probability.  Also the margin of a decode, a
returned labelling re-scored arc by arc, the composite model whose ordinary Viterbi score equals the word-loop
score, and the banks and observation sets the GPU tests share."""
import numpy as np

from viterbi_ref import MARGIN, RTOL, _gap  # noqa: F401  (the project's tolerances)


def log_bank(pi, A, B, init=None, G=None):
    pi, A, B = np.asarray(pi, float), np.asarray(A, float), np.asarray(B, float)
    W = pi.shape[0]
    init = np.ones(W) if init is None else np.asarray(init, float)
    G = np.ones((W, W)) if G is None else np.asarray(G, float)
    with np.errstate(divide="ignore"):
        return np.log(pi), np.log(A), np.log(B), np.log(init), np.log(G)


def decode(obs, pi, A, B, init=None, G=None, end_final=False):
    """(path int32 [T], start uint8 [T], logp, margin) of one sequence.  margin: the smallest best-minus-second-best
    gap over the decisions on the best path: the end state; at a within-word step the N inner candidates plus the
    entry candidate; at an entry step entry - inner and the gap among the v candidates.  inf where logp is -inf."""
    lpi, lA, lB, linit, lG = log_bank(pi, A, B, init, G)
    obs = np.asarray(obs).reshape(-1)
    T, (W, N) = obs.size, lpi.shape
    delta = (linit[:, None] + lpi) + lB[:, :, obs[0]]
    hist = [None] * T
    for t in range(1, T):
        c = delta[:, :, None] + lA                     # c[w, i, j] = delta_{t-1}(w, i) + log a_w[i][j]
        psi = np.argmax(c, axis=1)                     # the first maximum
        inner = np.take_along_axis(c, psi[:, None, :], axis=1)[:, 0, :]
        e = delta[:, N - 1][:, None] + lG              # e[v, w]
        src = np.argmax(e, axis=0)
        E = e[src, np.arange(W)]
        entry = E[:, None] + lpi
        take = entry > inner                           # the within-word arc wins ties
        hist[t] = (c, psi, inner, e, src, entry, take)
        delta = np.where(take, entry, inner) + lB[:, :, obs[t]]
    if end_final:
        cand = delta[:, N - 1]
        w = int(np.argmax(cand))
        j = N - 1
    else:
        cand = delta.reshape(-1)
        w, j = divmod(int(np.argmax(cand)), N)
    logp = float(delta[w, j])
    if logp == -np.inf:
        return np.full(T, -1, dtype=np.int32), np.zeros(T, dtype=np.uint8), logp, np.inf
    margin = _gap(cand)
    path, start = np.zeros(T, dtype=np.int32), np.zeros(T, dtype=np.uint8)
    for t in range(T - 1, 0, -1):
        path[t] = w * N + j
        c, psi, inner, e, src, entry, take = hist[t]
        if take[w, j]:
            start[t] = 1
            margin = min(margin, float(entry[w, j] - inner[w, j]), _gap(e[:, w]))
            w, j = int(src[w]), N - 1
        else:
            margin = min(margin, _gap(np.append(c[w, :, j], entry[w, j])))
            j = int(psi[w, j])
    path[0], start[0] = w * N + j, 1
    return path, start, logp, margin


def path_logp(path, start, obs, pi, A, B, init=None, G=None):
    """log-probability of one labelling (composite states and word-start flags), arc by arc in the recursion's
    order.  An entry arc into (w, j) from a state other than a last state scores -inf."""
    lpi, lA, lB, linit, lG = log_bank(pi, A, B, init, G)
    obs = np.asarray(obs).reshape(-1)
    N = lpi.shape[1]
    w, j = divmod(int(path[0]), N)
    v = (linit[w] + lpi[w, j]) + lB[w, j, obs[0]]
    for t in range(1, len(path)):
        pw, pj = w, j
        w, j = divmod(int(path[t]), N)
        if start[t]:
            arc = (lG[pw, w] + lpi[w, j]) if pj == N - 1 else -np.inf
        else:
            arc = lA[w, pj, j] if pw == w else -np.inf
        v = (v + arc) + lB[w, j, obs[t]]
    return float(v)


def composite(pi, A, B, init=None, G=None):
    """(pi', A', B') of W N states whose ordinary Viterbi score is the word-loop score: pi' = init (x) pi, A'
    block-diagonal in the a_w, each last-state row replaced by max(a_v[N-1][.] in its own block, G[v][w] pi_w[.])."""
    pi, A, B = np.asarray(pi, float), np.asarray(A, float), np.asarray(B, float)
    W, N = pi.shape
    init = np.ones(W) if init is None else np.asarray(init, float)
    G = np.ones((W, W)) if G is None else np.asarray(G, float)
    Ac = np.zeros((W * N, W * N))
    for w in range(W):
        Ac[w * N:(w + 1) * N, w * N:(w + 1) * N] = A[w]
    for v in range(W):
        Ac[v * N + N - 1] = np.maximum(Ac[v * N + N - 1], (G[v][:, None] * pi).reshape(-1))
    return (init[:, None] * pi).reshape(-1), Ac, B.reshape(W * N, -1)


def decode_all(obs, pi, A, B, init=None, G=None, end_final=False):
    """The checker over a list of sequences: (paths, starts, logp array, margin array)."""
    out = [decode(o, pi, A, B, init, G, end_final) for o in obs]
    return ([p for p, _, _, _ in out], [s for _, s, _, _ in out], np.array([l for _, _, l, _ in out]),
            np.array([m for _, _, _, m in out]))


# --------------------------------------------------------------------------------------------------------------
# what the GPU tests share
# --------------------------------------------------------------------------------------------------------------
def bank(W, N, K, topology, rng):
    """W models of viterbi_ref.model (Dirichlet pi for dense banks), word_init Dirichlet, word_trans 0.3 x Dirichlet
    rows."""
    from viterbi_ref import model
    ms = [model(N, K, topology, rng) for _ in range(W)]
    pi = np.stack([m[0] for m in ms])
    if topology == "dense":
        pi = rng.dirichlet(np.ones(N), size=W)
    A, B = np.stack([m[1] for m in ms]), np.stack([m[2] for m in ms])
    return pi, A, B, rng.dirichlet(np.ones(W)), 0.3 * rng.dirichlet(np.ones(W), size=W)


def check_labelling(p, s, o, W, N):
    """Check 2's first half: states in range, start[0] = 1, an entry step preceded by a last state, a within-word
    step inside one word."""
    assert p.dtype == np.int32 and s.dtype == np.uint8 and p.shape == s.shape == (len(o),)
    assert np.all((p >= 0) & (p < W * N)) and np.all(s <= 1) and s[0] == 1
    prev = p[:-1]
    ent = s[1:] == 1
    assert np.all(prev[ent] % N == N - 1)
    assert np.all(prev[~ent] // N == p[1:][~ent] // N)


def check_decode(obs, bank_, paths, starts, logp, end_final=False, min_clear=0.95):
    """Checks 1-3 of a decode against the checker; returns the checker's (paths, starts, logp, margin)."""
    pi, A, B, init, G = bank_
    W, N = np.asarray(pi).shape
    rpaths, rstarts, rlogp, margin = decode_all(obs, pi, A, B, init, G, end_final)
    clear = margin > MARGIN
    assert clear.mean() >= min_clear, f"only {clear.mean():.3f} of the sequences clear the margin (checker alone)"
    logp = np.asarray(logp)
    assert logp.shape == rlogp.shape and not np.any(np.isnan(logp))
    np.testing.assert_allclose(logp, rlogp, rtol=RTOL)                                     # 1
    assert len(paths) == len(starts) == len(obs)
    for r, (p, s, o) in enumerate(zip(paths, starts, obs)):
        if rlogp[r] == -np.inf:
            assert p.shape == s.shape == (len(o),) and np.all(p == -1) and np.all(s == 0), r
            continue
        check_labelling(p, s, o, W, N)                                                     # 2: valid ...
        np.testing.assert_allclose(path_logp(p, s, o, pi, A, B, init, G), logp[r], rtol=RTOL)  # ... and optimal
        if end_final:
            assert p[-1] % N == N - 1, r
        if clear[r]:
            assert np.array_equal(p, rpaths[r]) and np.array_equal(s, rstarts[r]), r       # 3
    return rpaths, rstarts, rlogp, margin


def word_sequences(W, N, n_seq, rng, max_words=5):
    """Recovery data: (observations, word lists).  Each sequence concatenates 1 .. max_words words (immediate repeats
    included); in a word every state j is held 1-4 frames and emits symbol w N + j with probability 0.9, any other
    symbol of the W N otherwise."""
    K = W * N
    obs, words = [], []
    for r in range(n_seq):
        n = int(rng.integers(1, max_words + 1))
        ws = [int(x) for x in rng.integers(0, W, size=n)]
        if n >= 2 and r % 2 == 0:
            ws[1] = ws[0]  # an immediate repeat
        o = []
        for w in ws:
            for j in range(N):
                for _ in range(int(rng.integers(1, 5))):
                    k = w * N + j
                    if rng.random() >= 0.9:
                        k = int((k + rng.integers(1, K)) % K)
                    o.append(k)
        obs.append(np.array(o))
        words.append(ws)
    return obs, words


def recovery_bank(W, N, rng):
    """Left-to-right word models entered at state 0, stay probabilities in [0.5, 0.7], state j of word w emitting
    symbol w N + j with probability 0.9 and the rest spread by a Dirichlet draw (no two scores tie)."""
    K = W * N
    pi = np.zeros((W, N))
    pi[:, 0] = 1.0
    A = np.zeros((W, N, N))
    stay = rng.uniform(0.5, 0.7, size=(W, N))
    for j in range(N):
        A[:, j, j] = stay[:, j] if j < N - 1 else 1.0
        if j < N - 1:
            A[:, j, j + 1] = 1.0 - stay[:, j]
    B = np.zeros((W, N, K))
    for w in range(W):
        for j in range(N):
            k = w * N + j
            B[w, j, np.arange(K) != k] = 0.1 * rng.dirichlet(np.full(K - 1, 2.0))
            B[w, j, k] = 0.9
    return pi, A, B
