"""The checker of the posterior tests: a plain NumPy log-domain forward-backward (log-sum-exp with the -inf terms
dropped, gamma = exp(log alpha + log beta - log P), zeros where log P = -inf), the max-marginal path by np.argmax
(the first maximum), and per position the gap between the largest and the second-largest gamma.  Also brute-force
enumeration of all N^T paths (what makes the checker trustworthy, tests/test_posterior.py) and check_posterior,
which every GPU case goes through.  The models and observation sets are those of tests/viterbi_ref.py."""
import itertools

import numpy as np

from viterbi_ref import log_params

GAP = 1e-8      # exact path equality is asked where the checker's gap exceeds this
RTOL = 1e-9     # the project's log-likelihood and statistics tolerance
ATOL = 1e-300   # tests/test_gpu_parity.py: the statistics' absolute term
ROW_SUM = 1e-12


def lse(x, axis):
    """log sum exp along axis with the -inf terms dropped; -inf where every term is -inf."""
    m = np.max(x, axis=axis)
    safe = np.where(np.isneginf(m), 0.0, m)
    with np.errstate(divide="ignore"):
        return np.where(np.isneginf(m), -np.inf, safe + np.log(np.sum(np.exp(x - np.expand_dims(safe, axis)), axis=axis)))


def forward_backward(obs, pi, A, B):
    """(log alpha [T, N], log beta [T, N], log P) of one sequence."""
    lpi, lA, lB = log_params(pi, A, B)
    obs = np.asarray(obs).reshape(-1)
    T, N = obs.size, lpi.size
    la, lb = np.empty((T, N)), np.zeros((T, N))
    la[0] = lpi + lB[:, obs[0]]
    for t in range(1, T):
        la[t] = lse(la[t - 1][:, None] + lA, axis=0) + lB[:, obs[t]]
    for t in range(T - 2, -1, -1):
        lb[t] = lse(lA + (lB[:, obs[t + 1]] + lb[t + 1])[None, :], axis=1)
    return la, lb, float(lse(la[-1], axis=0))


def posterior(obs, pi, A, B):
    """(gamma [T, N], path int32 [T], log P, gap [T], log alpha, log beta) of one sequence: zeros and -1 where
    log P = -inf; gap: the largest gamma minus the second largest (inf with one state or a dead sequence)."""
    la, lb, logp = forward_backward(obs, pi, A, B)
    T, N = la.shape
    if logp == -np.inf:
        return np.zeros((T, N)), np.full(T, -1, dtype=np.int32), logp, np.full(T, np.inf), la, lb
    gamma = np.exp(la + lb - logp)
    path = np.argmax(gamma, axis=1).astype(np.int32)
    if N < 2:
        gap = np.full(T, np.inf)
    else:
        top = np.sort(gamma, axis=1)[:, -2:]
        gap = top[:, 1] - top[:, 0]
    return gamma, path, logp, gap, la, lb


def brute_force(obs, pi, A, B):
    """(gamma [T, N] or None, P(O)) by enumeration of all N^T paths, linear domain: gamma_t(i) is the sum over the
    paths through (t, i) divided by the sum over all paths; None where P(O) = 0."""
    N, T = len(pi), len(obs)
    num, tot = np.zeros((T, N)), 0.0
    for p in itertools.product(range(N), repeat=T):
        w = pi[p[0]] * B[p[0], obs[0]]
        for t in range(1, T):
            w *= A[p[t - 1], p[t]] * B[p[t], obs[t]]
        tot += w
        for t in range(T):
            num[t, p[t]] += w
    return (num / tot if tot > 0 else None), tot


def split_rows(gamma, obs):
    """The flat [total, N] gamma (NumPy array or torch tensor) as one [T_r, N] host array per sequence."""
    if isinstance(gamma, (list, tuple)):
        return [np.asarray(g) for g in gamma]
    if hasattr(gamma, "cpu"):
        gamma = gamma.cpu().numpy()
    return np.split(np.asarray(gamma), np.cumsum([len(o) for o in obs])[:-1])


def check_posterior(obs, pi, A, B, gamma, paths, logp, min_clear=0.99):
    """Checks 1-4 of a posterior call against the checker (gamma or paths may be None: not asked for); returns the
    checker's per-sequence results.
    1. logp at rtol 1e-9, -inf exactly;  2. gamma at rtol 1e-9, atol 1e-300, no NaN, exactly 0.0 wherever the
    checker's log alpha or log beta is -inf;  3. every row of a live sequence sums to 1 within 1e-12, every row of a
    dead one is exactly zero and its path is -1;  4. the path equals the checker's wherever the gap exceeds 1e-8
    (asserted first, from the checker alone: at least min_clear of the positions clear it), and elsewhere holds a
    state whose gamma is within 1e-8 of the row's maximum.  Left-to-right paths need not be monotone."""
    N = len(pi)
    ref = [posterior(o, pi, A, B) for o in obs]
    gaps = np.concatenate([r[3] for r in ref]) if ref else np.zeros(0)
    if gaps.size:
        clear = float(np.mean(gaps > GAP))
        assert clear >= min_clear, f"only {clear:.4f} of the positions clear the gap (checker alone)"
    rlogp = np.array([r[2] for r in ref])
    logp = np.asarray(logp, dtype=float)
    assert logp.shape == rlogp.shape and not np.any(np.isnan(logp))
    assert np.array_equal(np.isneginf(logp), np.isneginf(rlogp))                 # 1
    live = np.isfinite(rlogp)
    np.testing.assert_allclose(logp[live], rlogp[live], rtol=RTOL)
    rows = split_rows(gamma, obs) if gamma is not None else [None] * len(obs)
    assert len(rows) == len(obs) and (paths is None or len(paths) == len(obs))
    for r, o in enumerate(obs):
        rg, rpath, _, gap, la, lb = ref[r]
        g = rows[r]
        if g is not None:
            assert g.dtype == np.float64 and g.shape == (len(o), N), r
            assert not np.any(np.isnan(g)), r
            if live[r]:
                np.testing.assert_allclose(g, rg, rtol=RTOL, atol=ATOL, err_msg=f"sequence {r}")   # 2
                assert np.all(g[np.isneginf(la) | np.isneginf(lb)] == 0.0), r
                assert np.all(np.abs(g.sum(axis=1) - 1.0) <= ROW_SUM), r        # 3
            else:
                assert np.all(g == 0.0), r
        if paths is not None:
            p = paths[r]
            assert p.dtype == np.int32 and p.shape == (len(o),), r
            if not live[r]:
                assert np.all(p == -1), r
                continue
            assert np.all((p >= 0) & (p < N)), r
            sure = gap > GAP
            assert np.array_equal(p[sure], rpath[sure]), r                      # 4
            t = np.flatnonzero(~sure)
            assert np.all(rg[t, p[t]] >= rg[t].max(axis=1) - GAP), r
    return ref
