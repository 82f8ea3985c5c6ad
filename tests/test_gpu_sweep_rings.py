"""The small-N E-step's sweeps at the edges of their rings (hmmbw_device.hpp: the forward's and the backward's 4-deep
pack rings and 4-chunk trips, the ring offsets shared by the symbol and exponent packs, the one LDS wait per chunk, C_h
recorded only in the trip that holds the cut, the lagged mode's one stored exponent), through
tests/test_gpu_lds_layout.py::run_case: 3 EM iterations and a statistics pass against the oracle on the same inputs at
that file's tolerances (every L and log P at rtol 1e-9, the complete statistics through assert_stats).

A chunk is 8 steps; T steps are (T + 7) // 8 chunks.  The lengths below give 1 to 10 chunks with a full and a partial
top chunk: the ring entered (1 chunk), just filled (4: T = 31, 32), just exceeded (5: T = 33, 40), the first steady trip
entered (chunks 1-4 after chunk 0: T = 33..40), and left with a tail of 1 and of up to 4 chunks (T = 41, 65, 72, 73).
With equal lengths sequence r sits in slot r % 8 of wave r // 8 (G = 8)."""
import numpy as np
import pytest

import scaling_ref as S
from test_gpu_fullsize import LL_RTOL, assert_stats, statistics_pass
from test_gpu_lds_layout import ITERS, _symbols_kind, run_case, uniform

pytestmark = pytest.mark.gpu

RING_T = [1, 7, 8, 9, 16, 17, 31, 32, 33, 40, 41, 65, 72, 73]
LR = "left_to_right"


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: the GPU tests need an MI355X")


# ------------------------------------------------------------------------------------------ ring and unroll edges
@pytest.mark.parametrize("T", RING_T)
@pytest.mark.parametrize("N", [8, 5])
def test_ring_edges(oracle, N, T):
    """R = 96, K = 256, left-to-right, the joined kernel on the class-split tables; N = 5: three padding lanes."""
    run_case(oracle, uniform(96, T, 256, seed=100 * N + T), N, 256, LR, layout=1, joined=True)


@pytest.mark.parametrize("T", [9, 33, 41])
def test_ring_edges_dense(oracle, T):
    """The dense recursion stores every z_t (its checkpoint stream advances a whole chunk per chunk).  Without extra
    groups a dense launch is not joined: k_estep_small on the row tables, which is what the case asserts."""
    run_case(oracle, uniform(96, T, 256, seed=T), 8, 256, "dense", layout=0, joined=False, option=None)


# ---------------------------------------------------------------------------------------------------- split groups
@pytest.mark.parametrize("kind", ["uniform", "two"])
@pytest.mark.parametrize("T", [9, 17, 25, 41, 73])
def test_split_groups(oracle_mt, kind, T):
    """R = 10,000: extra groups whose backward is cut at chunk hc = 1, 1, 2, 3, 5 of 2, 3, 4, 6, 10: the cut in the
    forward's tail (no steady trip, or past the last one), in the first steady trip, and (T = 73: chunks 1-4, 5-8, tail
    9) in a later trip than the first, so the loop runs before and after the trip that records C_h."""
    run_case(oracle_mt, _symbols_kind(kind, 10_000, T, 256), 8, 256, LR, layout=1, joined=True, split_extra=True)


# ---------------------------------------------------------------------------------------------------------- ragged
def test_ragged(oracle):
    """R = 200 with lengths 1..80: masked chunks at every ring position, waves whose shortest sequence ends inside
    the first trip, padding slots."""
    rng = np.random.default_rng(80)
    lens = rng.permutation(np.arange(200) % 80 + 1)
    obs = [rng.integers(0, 256, size=int(t)) for t in lens]
    run_case(oracle, obs, 8, 256, LR, layout=1, joined=True)


# ----------------------------------------------------------------------------------- row tables and the spread map
@pytest.mark.parametrize("T", [9, 33, 41])
def test_row_tables(oracle, T):
    run_case(oracle, uniform(96, T, 256, seed=T + 1), 8, 256, LR, layout=0, joined=True, option=0)


@pytest.mark.parametrize("T", [9, 33, 41])
def test_spread_map(oracle, monkeypatch, T):
    """HMMBW_JOIN=0: k_estep_small runs the same body in 4-wave workgroups (row tables)."""
    monkeypatch.setenv("HMMBW_JOIN", "0")
    run_case(oracle, uniform(96, T, 256, seed=T + 2), 8, 256, LR, layout=0, joined=False, option=None)


# ----------------------------------------------------------------------------------------------------- mode switch
def _switch_set():
    """Model `base` of scaling_ref (left-to-right, N = 8, K = 16, a 1e-20 column in B) and its mixed-wave set "b":
    R = 64, T = 56, the odd waves filled with runs of 17 to 40 floor-probability symbols."""
    m = S.MODELS["base"]
    obs, runs, _ = S.mixed_waves(m, "b")
    return m, obs, runs


def test_switch_set_really_switches(oracle):
    """CPU check of the input of test_mode_switch_natural, with the reference model of the kernels' rule
    (scaling_ref.lagged_regime): under the starting parameters every sequence with a run falls back to safe scaling
    and no other does; under the oracle's parameters after one, two and three iterations (the M-step has re-estimated
    the run's symbol from the sequences that hold it) every sequence is `ordinary`.  So the odd waves run safe in
    iteration 1 and lagged in iterations 2 and 3, and the even waves lagged throughout."""
    m, obs, runs = _switch_set()
    kinds = [S.lagged_regime(o, m.pi, m.A, m.B).kind for o in obs]
    assert all(k == ("fallback" if r else "ordinary") for k, r in zip(kinds, runs)) and runs.any() and not runs.all()
    off, sym = S.csr(obs)
    for it in (1, 2, 3):
        ref = oracle.hmm_training(off, sym, m.N, m.K, 0.0, it, m.pi, m.A, m.B)
        assert all(S.lagged_regime(o, ref.pi, ref.A, ref.B).kind == "ordinary" for o in obs), it


def test_mode_switch_natural(oracle):
    """Safe, then lagged, on the same sequence groups (test_switch_set_really_switches): the lagged iterations store a
    dword into exponent slots that hold a safe iteration's 16 bytes."""
    m, obs, _ = _switch_set()
    run_case(oracle, obs, m.N, m.K, m.topology, layout=0, joined=True, option=0, params=(m.pi, m.A, m.B))
    run_case(oracle, obs, m.N, m.K, m.topology, layout=1, joined=True, option=1, params=(m.pi, m.A, m.B))


@pytest.mark.parametrize("modes", [(0, 1, 0), (1, 0, 1)])
@pytest.mark.parametrize("T", [41, 73])
def test_mode_switch_forced(oracle_mt, modes, T):
    """Lagged, safe, lagged and safe, lagged, safe on one context, every group at once.  No input built from the
    floor-probability runs goes from lagged to safe on its own within 3 iterations (re-estimation only raises the
    emission of a run's symbol: test_switch_set_really_switches), so this order is driven through the option the
    scaling tests use, HMMBW_OPT_SAFE_SCALING, set between the iterations; the statistics pass that ends the case runs
    in the mode opposite to the last iteration's.  R = 10,000 (split groups: the B waves take the safe flag from their
    A waves) with the checks of run_case."""
    from hmm_training_amd._lib import OPT_LDS_LAYOUT, OPT_SAFE_SCALING
    from hmm_training_amd.engine import BaumWelchEngine, to_csr
    from test_gpu_fullsize import _params
    N, K, R = 8, 256, 10_000
    obs = uniform(R, T, K, seed=T)
    off, sym = to_csr(obs)
    sym64 = sym.astype(np.int64)
    pi, A, B = _params(N, K, LR, 7)
    ref = oracle_mt.hmm_training(off, sym64, N, K, 0.0, ITERS, pi, A, B)
    with BaumWelchEngine(N, K, topology=LR) as eng:
        eng.set_option(OPT_LDS_LAYOUT, 1)
        eng.set_observations(obs)
        eng.set_params(pi, A, B)
        lm = eng.launch_map()
        assert lm["joined"] and lm["split_extra"] and lm["lds_layout"] == 1, lm
        eng.reset(0.0, ITERS)
        for mode in modes:
            eng.set_option(OPT_SAFE_SCALING, mode)
            eng.enqueue_iterations(1)
        st, recs = eng.status(0, ITERS)
        assert st.iterations == ITERS
        np.testing.assert_allclose([L for L, _ in recs], ref.trace_L, rtol=LL_RTOL)
        np.testing.assert_allclose(eng.loglik(), ref.logP, rtol=LL_RTOL)
        p_cur, A_cur, B_cur = eng.params(normalise=False)
        eng.set_option(OPT_SAFE_SCALING, 1 - modes[-1])
        g, ll, _ = statistics_pass(eng, N, K, R)
    s = oracle_mt.estep_logstats(off, sym64, N, K, p_cur, A_cur, B_cur)
    np.testing.assert_allclose(ll, s.logP, rtol=LL_RTOL)
    assert_stats(g, s, R, T)
