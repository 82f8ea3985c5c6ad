"""CPU checks of tests/scaling_ref.py, the inputs of tests/test_gpu_scaling.py: that the case table is aimed at the
lagged scaling's envelope (every regime of the rule it was drawn against is populated), that the oracle may judge
the GPU on these magnitudes (200-bit mpmath forward sums), that a correct scaled-linear fp64 engine meets the
project tolerances on every case (the per-step normalised analogue of the kernels' safe mode), and that the v1
lagged arithmetic does not: what the GPU test is looking for."""
import collections

import numpy as np
import pytest

import scaling_ref as S

LL_RTOL, STAT_RTOL, STAT_ATOL = 1e-9, 1e-9, 1e-300   # tests/test_gpu_parity.py


@pytest.fixture(scope="module")
def judged(oracle):
    """{case name: (oracle log P, oracle E-step statistics)}, computed once."""
    out = {}
    for c in S.CASES:
        m = S.MODELS[c.model]
        off, sym = S.csr([c.obs])
        out[c.name] = (float(oracle.forward_loglik(off, sym, m.N, m.K, m.pi, m.A, m.B)[0]),
                       oracle.estep_logstats(off, sym, m.N, m.K, m.pi, m.A, m.B))
    return out


def mp_forward(obs, pi, A, B, prec=200):
    import mpmath
    with mpmath.workprec(prec):
        f = mpmath.mpf
        N = len(pi)
        al = [f(float(pi[j])) * f(float(B[j, obs[0]])) for j in range(N)]
        for o in obs[1:]:
            al = [sum(al[i] * f(float(A[i, j])) for i in range(N) if A[i, j] != 0) * f(float(B[j, o]))
                  for j in range(N)]
        p = sum(al)
        return float(mpmath.log(p)) if p > 0 else -np.inf


def test_case_table_shape():
    names = [c.name for c in S.CASES]
    assert len(set(names)) == len(names) and 80 <= len(names) <= 125
    assert max(len(c.obs) for c in S.CASES) <= 72
    for c in S.CASES:
        m = S.MODELS[c.model]
        assert c.obs.min() >= 0 and c.obs.max() < m.K
        np.testing.assert_allclose(m.B.sum(axis=1), 1.0, rtol=1e-14)
        if m.N >= 4:  # below, the reference's defaults are its 4-state arrays cut to N (default_initial_params)
            np.testing.assert_allclose(m.A.sum(axis=1), 1.0, rtol=1e-14)
        assert np.all(m.A.sum(axis=1) <= 1.0 + 1e-14)
    assert {m.N for m in S.MODELS.values()} == set(S.STATE_COUNTS)
    assert {m.K for m in S.MODELS.values()} == {S.K_LDS, S.K_GLOBAL}
    assert np.all(S.MODELS["base"].B[:, -1] == 1e-20)


def test_every_regime_of_the_v1_rule_is_populated():
    reg = S.regimes(S.lagged_regime_v1)
    count = collections.Counter(r.kind for r in reg.values())
    for kind in ("ordinary", "window", "fallback", "dead"):
        assert count[kind] >= 8, count
    deep = [n for n, r in reg.items() if r.kind == "window" and r.min_unscaled < -1050]
    assert len(deep) >= 4, deep
    # e = 112 and 113 straddle the v1 rule's -900 bound on the scaled exponent of the first rare interval
    assert reg["e112"].min_scaled >= -S.LAG_LOW_V1 > reg["e113"].min_scaled


def test_the_current_rule_leaves_no_live_sequence_in_the_window():
    reg = S.regimes(S.lagged_regime)
    v1 = S.regimes(S.lagged_regime_v1)
    assert not [n for n, r in reg.items() if r.kind == "window"]
    for n, r in reg.items():
        if v1[n].kind in ("fallback", "dead"):
            assert r.kind == v1[n].kind, n       # the new trigger only adds re-runs
        if r.kind == "ordinary":
            assert r.min_scaled >= -S.LAG_LOW and r.min_unscaled >= -2 * S.LAG_LOW, n
    # and the lagged mode is still exercised close to its bound, which cases straddle: eight steps of 2^-55 / 2^-57
    # and six / seven floor symbols inside one interval
    assert reg["n6"].kind == reg["n12_start11"].kind == reg["e55"].kind == "ordinary"
    assert reg["n6"].min_scaled < -400 and reg["n12_start11"].min_unscaled < -800
    assert reg["e55"].min_scaled >= -S.LAG_LOW + 5 and -S.LAG_LOW - 5 >= reg["e57"].min_scaled >= -S.LAG_LOW - 10
    assert reg["e57"].kind == reg["n7"].kind == "fallback" and reg["n7"].min_scaled >= -S.LAG_LOW - 20


def test_tail_cases_reach_past_the_last_scale_step():
    """The steps after a sequence's last scale step: under the v1 rule nothing looks at them (`window`: a denormal or
    zero final value of a live sequence), the current rule holds the final value to 2^-900; cases on both sides."""
    v1, reg = S.regimes(S.lagged_regime_v1), S.regimes(S.lagged_regime)
    tails = [c.name for c in S.CASES if c.name.startswith("tail_")]
    assert len(tails) >= 16
    lost = [n for n in tails if v1[n].kind == "window"]
    assert len(lost) >= 6 and all(v1[n].min_scaled >= -S.LAG_LOW for n in lost if "_a0_" in n), lost
    assert all(reg[n].kind == "fallback" for n in lost)
    kept = [n for n in tails if reg[n].kind == "ordinary"]
    assert len(kept) >= 6 and min(reg[n].min_unscaled for n in kept) < -750, kept
    assert all(reg[n].min_unscaled >= -2 * S.LAG_LOW for n in kept)


def test_oracle_agrees_with_200_bit_forward(judged):
    for c in S.CASES:
        m = S.MODELS[c.model]
        lp, s = judged[c.name]
        ref = mp_forward(c.obs, m.pi, m.A, m.B)
        if ref == -np.inf:
            assert lp == -np.inf and S.lagged_regime_v1(c.obs, m.pi, m.A, m.B).kind == "dead", c.name
            live = 0
        else:
            assert abs(lp - ref) <= 1e-12 * abs(ref), (c.name, lp, ref)
            assert abs(s.logP[0] - ref) <= 1e-12 * abs(ref), (c.name, s.logP[0], ref)
            live = len(c.obs)
        with np.errstate(under="ignore"):
            total = np.exp(s.log_gden_all).sum()
        assert abs(total - live) <= 1e-9, (c.name, total, live)


def test_per_step_normalised_engine_meets_the_tolerances(judged):
    for c in S.CASES:
        m = S.MODELS[c.model]
        lp, s = judged[c.name]
        mine, st = S.safe_estep([c.obs], m.pi, m.A, m.B)
        if lp == -np.inf:
            assert mine[0] == -np.inf, c.name
        else:
            np.testing.assert_allclose(mine[0], lp, rtol=LL_RTOL, err_msg=c.name)
        with np.errstate(under="ignore"):
            for key, lkey, atol in (("pi_num", "log_pi_num", STAT_ATOL), ("xi", "log_xi", STAT_ATOL),
                                    ("gamma_den_excl", "log_gden_excl", 0.0), ("gamma_den_all", "log_gden_all", 0.0),
                                    ("B_num", "log_bnum", STAT_ATOL)):
                np.testing.assert_allclose(st[key], np.exp(getattr(s, lkey)), rtol=STAT_RTOL, atol=atol,
                                           err_msg=f"{c.name} {key}")


def test_v1_lagged_arithmetic_misses_the_tolerance_in_the_window(judged):
    reg = S.regimes(S.lagged_regime_v1)
    missed, worst = [], 0.0
    for c in S.CASES:
        m = S.MODELS[c.model]
        lp, fired = S.lagged_forward(c.obs, m.pi, m.A, m.B)
        ref = judged[c.name][0]
        kind = reg[c.name].kind
        assert fired == (kind == "fallback") or kind == "dead", c.name   # the rule and the arithmetic agree
        if kind == "ordinary":
            np.testing.assert_allclose(lp, ref, rtol=LL_RTOL, err_msg=c.name)
        if kind == "window":
            err = abs(lp - ref) / abs(ref)
            worst = max(worst, err)
            if err > LL_RTOL:
                missed.append(c.name)
    assert len(missed) >= 4, (missed, worst)


def test_current_lagged_arithmetic_meets_the_tolerance_wherever_it_does_not_fire(judged):
    """The kernels keep the lagged forward's result only where the trigger did not fire: there the NumPy
    restatement of the current rule's arithmetic meets 1e-9 on every case, and it fires exactly where the rule's
    restatement says `fallback`."""
    reg = S.regimes(S.lagged_regime)
    kept = 0
    for c in S.CASES:
        m = S.MODELS[c.model]
        lp, fired = S.lagged_forward(c.obs, m.pi, m.A, m.B, rule="current")
        ref = judged[c.name][0]
        kind = reg[c.name].kind
        assert kind != "window", c.name
        if kind != "dead":
            assert fired == (kind == "fallback"), c.name
        if not fired:
            kept += 1
            if ref == -np.inf:
                assert lp == -np.inf, c.name
            else:
                np.testing.assert_allclose(lp, ref, rtol=LL_RTOL, err_msg=c.name)
    assert kept >= 20
