"""The checker of the embedded-training tests: a plain NumPy restatement of hmmbw_embedded_train (include/hmmbw.h).
Per utterance the word models of the transcript are chained into one composite model with explicit matrices
(states (l, j), the within-word arcs a_w[i][j], the entry arcs (l, N-1) -> (l+1, j) of weight pi_w[j], which do not
share a row sum with the self-loop of (l, N-1)); a forward-backward scaled by the row sums gives log P and the arc
and state posteriors, which are pooled per word; then the reference's M-step per word and its convergence trace.
Written from the definitions, not from the kernel: dense matrices, no lanes, no power-of-two scaling."""
import numpy as np

PARAM_RTOL, PARAM_ATOL, LL_RTOL = 1e-6, 1e-15, 1e-9  # the project's tolerances


class Stats:
    def __init__(self, W, N, K):
        self.entry = np.zeros((W, N))
        self.xi = np.zeros((W, N, N))
        self.g_all = np.zeros((W, N))
        self.b_num = np.zeros((W, N, K))
        self.count = np.zeros(W, dtype=np.int64)

    @property
    def a_den(self):
        return self.xi.sum(axis=2)


def composite(words, pi, A, B, end_final=False):
    """(init [S], trans [S, S], emis [S, K], end [S]) of the chain of the transcript's word models, S = L N."""
    N = pi.shape[1]
    L = len(words)
    S = L * N
    init, trans, end = np.zeros(S), np.zeros((S, S)), np.zeros(S)
    init[:N] = pi[words[0]]
    for l, w in enumerate(words):
        trans[l * N:(l + 1) * N, l * N:(l + 1) * N] = A[w]
        if l + 1 < L:
            trans[l * N + N - 1, (l + 1) * N:(l + 2) * N] = pi[words[l + 1]]
    if end_final:
        end[S - 1] = 1.0
    else:
        end[S - N:] = 1.0
    return init, trans, np.concatenate([B[w] for w in words]), end


def forward_backward(obs, words, pi, A, B, end_final=False):
    """(log P, alpha [T, S], vb [T-1, S], gamma [T, S], trans) of one utterance, or (-inf, None, ...) where P = 0.
    alpha is scaled by its row sums and vb_t = b(o_{t+1}) beta_{t+1} by the same factors, so that gamma_t = alpha_t
    beta_t and the posterior of the arc s -> s' out of row t is alpha_t(s) trans[s, s'] vb_t(s')."""
    obs = np.asarray(obs).reshape(-1)
    init, trans, emis, end = composite(words, pi, A, B, end_final)
    T, S = obs.size, init.size
    dead = (-np.inf, None, None, None, trans)
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
    return logp, alpha, vb, alpha * beta, trans


def utterance(obs, words, pi, A, B, end_final=False):
    """(log P, gamma [T, S], xi [T-1, S, S]) of one utterance, every arc posterior spelt out; (-inf, None, None)
    where P = 0.  For small cases: xi takes T S^2 doubles."""
    logp, alpha, vb, gamma, trans = forward_backward(obs, words, pi, A, B, end_final)
    if gamma is None:
        return logp, None, None
    return logp, gamma, alpha[:-1, :, None] * trans[None] * vb[:, None, :]


def estep(obs, transcripts, pi, A, B, end_final=False):
    """(Stats, logp [R]) of the bank: every instance of a word adds to that word's sums."""
    pi, A, B = np.asarray(pi, float), np.asarray(A, float), np.asarray(B, float)
    W, N = pi.shape
    K = B.shape[2]
    st = Stats(W, N, K)
    logp = np.zeros(len(obs))
    for r, (o, words) in enumerate(zip(obs, transcripts)):
        o = np.asarray(o).reshape(-1)
        for w in words:
            st.count[w] += 1
        logp[r], alpha, vb, gamma, trans = forward_backward(o, words, pi, A, B, end_final)
        if gamma is None:
            continue
        for l, w in enumerate(words):
            sl = slice(l * N, (l + 1) * N)
            g = gamma[:, sl]
            st.g_all[w] += g.sum(axis=0)
            np.add.at(st.b_num[w].T, o, g)
            # the arcs' posteriors summed over the rows: sum_t alpha_t(s) trans[s, s'] vb_t(s')
            st.xi[w] += trans[sl, sl] * (alpha[:-1, sl].T @ vb[:, sl])
            if l == 0:
                st.entry[w] += g[0]
            else:
                st.entry[w] += trans[l * N - 1, sl] * (alpha[:-1, l * N - 1] @ vb[:, sl])
    return st, logp


def mstep(st, pi, A, B):
    """The reference's M-step per word (hmm_training.py:415-500); a word without an instance keeps its parameters."""
    pi, A, B = np.array(pi, float), np.array(A, float), np.array(B, float)
    for w in np.flatnonzero(st.count > 0):
        pi[w] = st.entry[w] / st.count[w]
        den = st.a_den[w][:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            A[w] = np.where((st.xi[w] > 0) & (den > 0), st.xi[w] / den, 0.0)
            g = st.g_all[w][:, None]
            B[w] = np.where(g > 0, np.where(st.b_num[w] > 0, st.b_num[w] / g, 1e-20), 0.0)
    return pi, A, B


def lse(x):
    x = np.asarray(x, float)
    m = x.max() if x.size else -np.inf
    return -np.inf if m == -np.inf else float(m + np.log(np.exp(x - m).sum()))


def normalised(pi, A, B, count=None):
    """The reference's return path (hmm_training.py:524-541) per trained word: pi / sum pi, the rows of A and B with a
    positive sum divided by it."""
    pi, A, B = np.array(pi, float), np.array(A, float), np.array(B, float)
    for w in range(pi.shape[0]):
        if count is not None and count[w] == 0:
            continue
        s = pi[w].sum()
        if s > 0:
            pi[w] /= s
        for M_ in (A[w], B[w]):
            rs = M_.sum(axis=1, keepdims=True)
            np.divide(M_, rs, out=M_, where=rs > 0)
    return pi, A, B


def train(obs, transcripts, pi, A, B, epsilon=0.0, max_iterations=1, end_final=False, normalise=False):
    """(pi, A, B, records [(L, diff)], logp of the last E-step, Stats of the last E-step): hmm_training.py:346-514 on
    working parameters."""
    pi, A, B = np.array(pi, float), np.array(A, float), np.array(B, float)
    prev, records = -np.inf, []
    it, diff = 0, np.inf
    st = logp = None
    while diff >= epsilon and it < max_iterations:
        st, logp = estep(obs, transcripts, pi, A, B, end_final)
        pi, A, B = mstep(st, pi, A, B)
        L = lse(logp)
        diff = abs(L - prev) if prev != -np.inf else np.inf
        prev = L
        records.append((L, diff))
        it += 1
    if normalise:
        pi, A, B = normalised(pi, A, B, st.count)
    return pi, A, B, records, logp, st


def close(mine, ref, what=""):
    mine, ref = np.asarray(mine), np.asarray(ref)
    assert mine.shape == ref.shape and not np.any(np.isnan(mine)), what
    err = np.abs(mine - ref) - (PARAM_RTOL * np.abs(ref) + PARAM_ATOL)
    assert np.all(err <= 0), f"{what}: worst excess {err.max():.3e}"


# --------------------------------------------------------------------------------------------------------------
# what the GPU tests share
# --------------------------------------------------------------------------------------------------------------
def transcripts_for(W, lengths, rng):
    """One transcript per entry of lengths, words drawn uniformly, every second one with an immediate repeat."""
    out = []
    for r, L in enumerate(lengths):
        ws = [int(x) for x in rng.integers(0, W, size=int(L))]
        if L >= 2 and r % 2 == 0:
            ws[1] = ws[0]
        out.append(ws)
    return out


def flat_start(W, N, K, rng):
    """The near-flat start of the recovery test: pi = e_0, stay probability 0.6, B drawn from Dirichlet(50)."""
    pi = np.zeros((W, N))
    pi[:, 0] = 1.0
    A = np.zeros((W, N, N))
    for j in range(N):
        A[:, j, j] = 0.6
        if j + 1 < N:
            A[:, j, j + 1] = 0.4
    return pi, A, rng.dirichlet(np.full(K, 50.0), size=(W, N))
