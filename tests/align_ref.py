"""The checker of the forced-alignment tests: a plain NumPy restatement of the chain recursion of include/hmmbw.h
(hmmbw_align), with its tie rules: np.log with log 0 = -inf, the first maximum for the within-word predecessor i
and for the end state, the within-word arc on a tie with the entry arc, and a path and bounds of -1 where no
complete path has positive probability.  Also the margin of an alignment, a returned labelling re-scored arc by
arc, the validity of a labelling, and the cases the GPU tests share.  Written from the recursion: a [L, N] array
of deltas, no lanes."""
import numpy as np

from embedded_ref import composite, transcripts_for  # noqa: F401  (the chain, and the transcripts of the GPU tests)
from viterbi_ref import MARGIN, RTOL, _gap  # noqa: F401  (the project's tolerances)
from wordnet_ref import bank  # noqa: F401


def log_bank(pi, A, B):
    with np.errstate(divide="ignore"):
        return np.log(np.asarray(pi, float)), np.log(np.asarray(A, float)), np.log(np.asarray(B, float))


def align(obs, words, pi, A, B, end_final=False):
    """(path int32 [T], bounds int32 [L], logp, margin) of one utterance.  margin: the smallest best-minus-second-best
    gap over the decisions on the best path: the end state; at a within-word step the N inner candidates plus the
    entry candidate; at an entry step entry - inner (the entry source is fixed by the chain).  inf where logp is
    -inf."""
    lpi, lA, lB = log_bank(pi, A, B)
    obs = np.asarray(obs).reshape(-1)
    words = np.asarray(words, dtype=np.int64).reshape(-1)
    T, L, N = obs.size, words.size, lpi.shape[1]
    wpi, wA, wB = lpi[words], lA[words], lB[words]         # [L, N], [L, N, N], [L, N, K]
    delta = np.full((L, N), -np.inf)
    delta[0] = wpi[0] + wB[0][:, obs[0]]
    hist = [None] * T
    for t in range(1, T):
        c = delta[:, :, None] + wA                         # c[l, i, j] = delta_{t-1}(l, i) + log a_{w_l}[i][j]
        psi = np.argmax(c, axis=1)                         # the first maximum
        inner = np.take_along_axis(c, psi[:, None, :], axis=1)[:, 0, :]
        left = np.concatenate([[-np.inf], delta[:-1, N - 1]])
        entry = left[:, None] + wpi
        take = entry > inner                               # the within-word arc wins ties
        hist[t] = (c, psi, inner, entry, take)
        delta = np.where(take, entry, inner) + wB[:, :, obs[t]]
    cand = delta[L - 1, N - 1:] if end_final else delta[L - 1]
    j = N - 1 if end_final else int(np.argmax(cand))
    logp = float(delta[L - 1, j])
    if logp == -np.inf:
        return np.full(T, -1, dtype=np.int32), np.full(L, -1, dtype=np.int32), logp, np.inf
    margin = _gap(cand)
    path, bounds = np.zeros(T, dtype=np.int32), np.full(L, -1, dtype=np.int32)
    l = L - 1
    for t in range(T - 1, 0, -1):
        path[t] = l * N + j
        c, psi, inner, entry, take = hist[t]
        if take[l, j]:
            bounds[l] = t
            margin = min(margin, float(entry[l, j] - inner[l, j]))
            l, j = l - 1, N - 1
        else:
            margin = min(margin, _gap(np.append(c[l, :, j], entry[l, j])))
            j = int(psi[l, j])
    path[0], bounds[0] = l * N + j, 0
    assert l == 0
    return path, bounds, logp, margin


def path_logp(path, obs, words, pi, A, B):
    """log-probability of one labelling (composite states l N + j), arc by arc in the recursion's order: a step that
    keeps the position is a within-word arc, a step to the next position an entry arc, which scores -inf from a state
    other than a last state; a path that does not start in position 0 or moves otherwise scores -inf."""
    lpi, lA, lB = log_bank(pi, A, B)
    obs = np.asarray(obs).reshape(-1)
    N = lpi.shape[1]
    l, j = divmod(int(path[0]), N)
    v = (lpi[words[0], j] if l == 0 else -np.inf) + lB[words[l], j, obs[0]]
    for t in range(1, len(path)):
        pl, pj = l, j
        l, j = divmod(int(path[t]), N)
        if l == pl:
            arc = lA[words[l], pj, j]
        elif l == pl + 1 and pj == N - 1:
            arc = lpi[words[l], j]
        else:
            arc = -np.inf
        v = (v + arc) + lB[words[l], j, obs[t]]
    return float(v)


def check_labelling(p, b, T, L, N):
    """A valid labelling: int32 arrays of T and L entries; states in range; the path starts in position 0 and ends
    in position L - 1; positions non-decreasing by steps of at most 1, an increase only from state N - 1; and the
    bounds are the frames at which the positions first appear."""
    assert p.dtype == np.int32 and b.dtype == np.int32 and p.shape == (T,) and b.shape == (L,)
    assert np.all((p >= 0) & (p < L * N))
    pos = p // N
    assert pos[0] == 0 and pos[-1] == L - 1
    step = np.diff(pos)
    assert np.all((step >= 0) & (step <= 1))
    assert np.all(p[:-1][step == 1] % N == N - 1)
    assert np.array_equal(b, np.concatenate([[0], np.flatnonzero(step == 1) + 1]))


def align_all(obs, transcripts, pi, A, B, end_final=False):
    """The checker over a list of utterances: (paths, bounds, logp array, margin array)."""
    out = [align(o, ws, pi, A, B, end_final) for o, ws in zip(obs, transcripts)]
    return ([x[0] for x in out], [x[1] for x in out], np.array([x[2] for x in out]), np.array([x[3] for x in out]))


def check_align(obs, transcripts, bank_, paths, bounds, logp, end_final=False, min_clear=0.95):
    """Checks 1-3 of an alignment against the checker; returns the checker's (paths, bounds, logp, margin)."""
    pi, A, B = bank_
    N = np.asarray(pi).shape[1]
    rpaths, rbounds, rlogp, margin = align_all(obs, transcripts, pi, A, B, end_final)
    finite = rlogp > -np.inf
    clear = margin > MARGIN
    if finite.any():
        frac = clear[finite].mean()
        assert frac >= min_clear, f"only {frac:.3f} of the finite sequences clear the margin (checker alone)"
    logp = np.asarray(logp)
    assert logp.shape == rlogp.shape and not np.any(np.isnan(logp))
    assert np.array_equal(logp == -np.inf, ~finite)
    np.testing.assert_allclose(logp, rlogp, rtol=RTOL)                                           # 1
    assert len(paths) == len(bounds) == len(obs)
    for r, (p, b, o, ws) in enumerate(zip(paths, bounds, obs, transcripts)):
        if not finite[r]:
            assert p.dtype == np.int32 and b.dtype == np.int32 and p.shape == (len(o),) and b.shape == (len(ws),), r
            assert np.all(p == -1) and np.all(b == -1), r
            continue
        check_labelling(p, b, len(o), len(ws), N)                                                # 2: valid ...
        np.testing.assert_allclose(path_logp(p, o, ws, pi, A, B), logp[r], rtol=RTOL)            # ... and optimal
        if end_final:
            assert p[-1] % N == N - 1, r
        if clear[r]:
            assert np.array_equal(p, rpaths[r]) and np.array_equal(b, rbounds[r]), r             # 3
    return rpaths, rbounds, rlogp, margin


# --------------------------------------------------------------------------------------------------------------
# what the GPU tests share
# --------------------------------------------------------------------------------------------------------------
def gw_of(longest):
    return 8 if longest <= 8 else 16 if longest <= 16 else 32 if longest <= 32 else 64


def without_repeats(words, W):
    """The transcript with every immediate repeat of a word replaced by the next word.  With one-state words the
    frame at which the first of two instances of the same word hands over to the second is not determined (every
    placement scores the same arcs: a stay and an entry of the same word, and the same emissions), so such
    transcripts can never clear a margin."""
    out = list(words)
    for l in range(1, len(out)):
        if out[l] == out[l - 1]:
            out[l] = (out[l] + 1) % W
    return out


def case(W, N, K, topology, longest, seed):
    """(obs, transcripts, (pi, A, B)): R is no multiple of the 64 / GW slots of a wave; the first transcript has
    `longest` words, the others 1 .. longest, immediate repeats included (transcripts_for; not for one-state words:
    without_repeats); T from the transcript's
    length (the shortest an utterance can be) up to about 3 L N, some just around the 8-step chunk."""
    from viterbi_ref import sequences
    rng = np.random.default_rng(seed)
    pi, A, B, _, _ = bank(W, N, K, topology, rng)
    R = 2 * (64 // gw_of(longest)) + 3
    lens = [longest] + [int(x) for x in rng.integers(1, longest + 1, size=R - 1)]
    transcripts = transcripts_for(W, lens, rng)
    if N == 1:
        transcripts = [without_repeats(ws, W) for ws in transcripts]
    T = [int(rng.integers(L, 3 * L * N + 1)) for L in lens]
    for r, t in zip(range(1, R), (7, 8, 9, 17)):
        T[r] = max(t, lens[r])
    T[0] = 3 * longest * N  # the longest chain at its longest
    return sequences(T, K, rng), transcripts, (pi, A, B)
