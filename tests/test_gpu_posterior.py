"""State posteriors on the GPU (hmmbw_posterior, hmm_training_amd/csrc/posterior.hip) against the NumPy
forward-backward of tests/posterior_ref.py.  Every case goes through posterior_ref.check_posterior: 1. logp to
rtol 1e-9, -inf exactly; 2. gamma to rtol 1e-9 / atol 1e-300 with no NaN and exact zeros where the checker's
log alpha or log beta is -inf; 3. rows of a live sequence sum to 1 within 1e-12, a dead sequence has zero rows and
a -1 path; 4. the path equals the checker's wherever its gap exceeds 1e-8, after asserting from the checker alone
that at least 99 % of the positions clear it."""
import ctypes

import numpy as np
import pytest

import posterior_ref as P
import viterbi_ref as V

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: the GPU tests need an MI355X")


def same_bytes(x, y):
    return np.asarray(x).tobytes() == np.asarray(y).tobytes()


def posterior(obs, pi, A, B, topology, **kw):
    """The full call, and beside it every other output combination and a second full call: each returns the same
    bytes for what it returns (no atomics; the library's scratch buffer gives the path of the caller's tensor)."""
    from hmm_training_amd.engine import BaumWelchEngine
    with BaumWelchEngine(len(pi), B.shape[1], topology=topology, **kw) as e:
        e.set_observations(obs)
        e.set_params(pi, A, B)
        gamma, paths, logp = e.posterior()
        gamma = gamma.cpu().numpy()
        g1, p1, l1 = e.posterior(paths=False)                  # gamma only
        g2, p2, l2 = e.posterior(gamma=False)                  # path only: the library's scratch buffer
        g3, p3, l3 = e.posterior(gamma=False, paths=False)     # log P only: the forward alone
        g4, p4, l4 = e.posterior()
        assert e.topology == topology
        assert p1 is None and g2 is None and g3 is None and p3 is None
        assert same_bytes(g1.cpu().numpy(), gamma) and same_bytes(g4.cpu().numpy(), gamma)
        assert all(same_bytes(x, y) for x, y in zip(p2, paths)) and all(same_bytes(x, y) for x, y in zip(p4, paths))
        assert len(p2) == len(p4) == len(paths)
        for l in (l1, l2, l3, l4):
            assert same_bytes(l, logp)
    return gamma, paths, logp


def run_case(N, K, topology, T, seed, min_clear=0.99):
    rng = np.random.default_rng(seed)
    pi, A, B = V.model(N, K, topology, rng)
    obs = V.sequences(T, K, rng)
    gamma, paths, logp = posterior(obs, pi, A, B, topology)
    assert gamma.shape == (sum(len(o) for o in obs), N)
    return obs, P.check_posterior(obs, pi, A, B, gamma, paths, logp, min_clear=min_clear)


STATE_CASES = [(N, topo) for N in (1, 3, 4, 5, 8, 9, 16, 17, 33, 64)
               for topo in (("dense", "left_to_right") if N <= 16 else ("dense",))]


@pytest.mark.parametrize("N,topology", STATE_CASES)
def test_state_counts(N, topology):
    # every lane-group width, each also just above its power of two; K = 4: the emission table in LDS
    rng = np.random.default_rng(100 + N)
    run_case(N, 4, topology, V.ragged_lengths(N, 7, rng), 200 + N)


@pytest.mark.parametrize("N,K,topology", [(8, 256, "left_to_right"),   # LDS table, scaled packs
                                          (8, 256, "dense"),
                                          (16, 256, "dense"),          # LDS table, unscaled packs
                                          (16, 256, "left_to_right"),
                                          (64, 1024, "dense"),         # the table stays in global memory
                                          (33, 256, "dense")])         # 128 KiB: global too
def test_emission_table_placements(N, K, topology):
    rng = np.random.default_rng(300 + N + K)
    run_case(N, K, topology, V.ragged_lengths(N, 9, rng), 400 + N + K)


@pytest.mark.parametrize("tmin", [1, 7, 8, 9, 17, 40])
@pytest.mark.parametrize("N,K,topology", [(8, 256, "left_to_right"), (8, 64, "dense"), (3, 32, "left_to_right"),
                                          (40, 16, "dense")])
def test_lengths_around_the_chunk(tmin, N, K, topology):
    rng = np.random.default_rng(1000 + tmin + N)
    run_case(N, K, topology, V.ragged_lengths(N, tmin, rng), 2000 + tmin + N)


@pytest.mark.parametrize("N,K,topology,T", [(8, 16, "dense", 1), (8, 16, "left_to_right", 13), (20, 16, "dense", 13),
                                            (2, 5, "dense", 1)])
def test_single_sequence(N, K, topology, T):
    run_case(N, K, topology, [T], 3000 + N + T)


def test_long_left_to_right_sequences_need_the_rescaling():
    # an unscaled linear recursion underflows well before 200 steps at K = 256 (about 2^-8 per step)
    N, K = 8, 256
    rng = np.random.default_rng(71)
    obs, ref = run_case(N, K, "left_to_right", V.ragged_lengths(N, 300, rng), 72)
    assert min(r[2] for r in ref) < -1500.0  # log P far below log of the smallest double (-745)
    tiny = min(r[0][r[0] > 0].min() for r in ref)
    assert tiny < 1e-60                      # and gammas far below fp64 epsilon are still held to rtol 1e-9


def test_long_wide_sequence_needs_the_rescaling():
    obs, ref = run_case(64, 16, "dense", [600], 73)
    assert ref[0][2] < -1000.0


def test_exact_ties_take_the_lowest_state():
    N, K = 4, 4
    pi, A, B = np.full(N, 1 / N), np.full((N, N), 1 / N), np.full((N, K), 1 / K)
    rng = np.random.default_rng(5)
    obs = V.sequences(V.ragged_lengths(N, 7, rng), K, rng)
    gamma, paths, logp = posterior(obs, pi, A, B, "dense")
    for p, o in zip(paths, obs):
        assert p.shape == (len(o),) and np.all(p == 0)
    # every state ties whatever the arithmetic, so the gap is 0 and check 4 asks for equality nowhere: min_clear = 0
    P.check_posterior(obs, pi, A, B, gamma, paths, logp, min_clear=0.0)


def test_zero_probability_sequences():
    # left-to-right from state 0 with T < N: the states past t are unreachable (alpha exactly 0); one symbol has
    # a zero emission column, so a sequence that contains it is dead, whether it dies at t = 0 or in the middle
    N, K, zero = 8, 6, 4
    rng = np.random.default_rng(11)
    pi, A, B = V.model(N, K, "left_to_right", rng)
    pi = np.zeros(N)
    pi[0] = 1.0
    B[:, zero] = 0.0
    B /= B.sum(axis=1, keepdims=True)
    obs = V.sequences(rng.integers(1, N, size=45), K, rng)
    obs[0] = np.array([0, 1, 2])            # one that certainly lives
    obs[1] = np.array([0, zero, 2, 1])      # one that dies in the middle
    obs[2] = np.array([zero, 1, 2, 0, 3])   # and one that is dead from the first step
    gamma, paths, logp = posterior(obs, pi, A, B, "left_to_right")
    has_zero = np.array([np.any(o == zero) for o in obs])
    assert has_zero.any() and not has_zero.all()
    assert np.all(logp[has_zero] == -np.inf) and np.all(np.isfinite(logp[~has_zero]))
    rows = P.split_rows(gamma, obs)
    for r in np.flatnonzero(has_zero):
        assert np.all(paths[r] == -1) and np.all(rows[r] == 0.0)
    assert np.all(rows[0][0] == np.eye(N)[0])  # gamma_0 = e_0 exactly
    P.check_posterior(obs, pi, A, B, gamma, paths, logp)


@pytest.mark.parametrize("N,K,topology", [(8, 32, "left_to_right"), (20, 16, "dense")])
def test_sums_of_gamma_are_the_oracle_statistics(N, K, topology, oracle):
    # a second, independent check of the E-step's mathematics: the C oracle's statistics from the returned gamma
    from hmm_training_amd.engine import to_csr
    rng = np.random.default_rng(81 + N)
    pi, A, B = V.model(N, K, topology, rng)
    obs = V.sequences(V.ragged_lengths(N, 7, rng), K, rng)
    gamma, paths, logp = posterior(obs, pi, A, B, topology)
    off, sym = to_csr(obs)
    s = oracle.estep_logstats(off, sym.astype(np.int64), N, K, pi, A, B)
    np.testing.assert_allclose(logp, s.logP, rtol=1e-9)
    first, last = off[:-1], off[1:] - 1
    not_last = np.ones(len(gamma), dtype=bool)
    not_last[last] = False
    bnum = np.zeros((N, K))
    np.add.at(bnum.T, sym, gamma)
    tol = dict(rtol=1e-9, atol=1e-300)
    np.testing.assert_allclose(gamma[first].sum(axis=0), np.exp(s.log_pi_num), **tol)
    np.testing.assert_allclose(gamma[not_last].sum(axis=0), np.exp(s.log_gden_excl), **tol)
    np.testing.assert_allclose(gamma.sum(axis=0), np.exp(s.log_gden_all), **tol)
    np.testing.assert_allclose(bnum, np.exp(s.log_bnum), **tol)


@pytest.mark.parametrize("deterministic", [True, False])
def test_posterior_does_not_disturb_training(deterministic):
    from hmm_training_amd.engine import BaumWelchEngine
    N, K = 8, 32
    rng = np.random.default_rng(21)
    pi, A, B = V.model(N, K, "left_to_right", rng)
    obs = V.sequences(V.ragged_lengths(N, 17, rng), K, rng)

    def run(with_posterior):
        trace = []
        with BaumWelchEngine(N, K, topology="left_to_right", deterministic=deterministic) as e:
            e.set_observations(obs)
            e.set_params(pi, A, B)
            e.train(0.0, 2, lambda k, L, d: trace.append(L))
            ll = e.loglik()
            if with_posterior:
                gamma, paths, logp = e.posterior()
                assert np.array_equal(e.loglik(), ll)      # the E-step's log-likelihoods are untouched
                p, a, b = e.params(normalise=False)
                P.check_posterior(obs, p, a, b, gamma, paths, logp)
            e.train(0.0, 2, lambda k, L, d: trace.append(L))
            return e.params(normalise=False), np.array(trace), ll

    (p1, t1, l1), (p0, t0, l0) = run(True), run(False)
    assert len(t1) == len(t0) == 4
    for x, y in list(zip(p1, p0)) + [(t1, t0), (l1, l0)]:
        if deterministic:
            assert np.array_equal(x, y)
        else:
            np.testing.assert_allclose(x, y, rtol=1e-12)


def test_class_split_layout_context():
    # the context keeps a second pack set for the class-split tables; the posterior kernels read the first
    from hmm_training_amd._lib import OPT_LDS_LAYOUT
    from hmm_training_amd.engine import BaumWelchEngine
    N, K = 8, 256
    rng = np.random.default_rng(31)
    pi, A, B = V.model(N, K, "left_to_right", rng)
    obs = V.sequences(V.ragged_lengths(N, 9, rng), K, rng)
    with BaumWelchEngine(N, K, topology="left_to_right") as e:
        e.set_option(OPT_LDS_LAYOUT, 1)
        e.set_observations(obs)
        e.set_params(pi, A, B)
        assert e.lds_layout == 1 and e.launch_map()["joined"]
        e.train(0.0, 1)
        p, a, b = e.params(normalise=False)
        gamma, paths, logp = e.posterior()
    P.check_posterior(obs, p, a, b, gamma, paths, logp)


def test_errors():
    import torch
    from hmm_training_amd import _lib
    from hmm_training_amd.engine import BaumWelchEngine
    N, K = 4, 8
    rng = np.random.default_rng(41)
    pi, A, B = V.model(N, K, "dense", rng)
    obs = V.sequences([5, 3, 9], K, rng)
    logp = np.zeros(3)
    path = np.zeros(17, dtype=np.int32)
    with BaumWelchEngine(N, K, world_size=2, rank=0, native_comm=False) as e:
        gam = torch.empty((17, N), dtype=torch.float64, device=f"cuda:{e.device}")
        g, pa, lp = ctypes.c_void_p(gam.data_ptr()), path.ctypes.data, logp.ctypes.data
        call = lambda g, gn, pa, pn, lp: e._lib.hmmbw_posterior(e._ctx, g, gn, pa, pn, lp)  # noqa: E731
        assert call(g, 17 * N, pa, 17, lp) == _lib.HMMBW_E_STATE        # no observations
        e.set_observations(obs)
        assert call(g, 17 * N, pa, 17, lp) == _lib.HMMBW_E_STATE        # no parameters
        e.set_params(pi, A, B)
        assert call(g, 17 * N, pa, 16, lp) == _lib.HMMBW_E_INVALID      # wrong path_len
        assert call(g, 17 * N - 1, pa, 17, lp) == _lib.HMMBW_E_INVALID  # wrong gamma_len
        assert call(g, 17, pa, 17, lp) == _lib.HMMBW_E_INVALID          # ... rows, not entries
        assert call(None, 17 * N, None, 17, None) == _lib.HMMBW_E_INVALID  # nothing asked for
        e.reset(0.0, 5)
        e.iterate_begin()
        assert call(g, 17 * N, pa, 17, lp) == _lib.HMMBW_E_STATE        # an iteration is open
        e.iterate_end()
        assert call(g, 17 * N, pa, 17, lp) == _lib.HMMBW_OK
        # what the accepted call wrote, under the parameters the iteration left (17 positions: no gap condition)
        P.check_posterior(obs, *e.params(normalise=False), gam, np.split(path, [5, 8]), logp, min_clear=0.0)
        with pytest.raises(ValueError):
            e.n_symbols_total = 16
            e.posterior()


def test_empty_observations_write_nothing():
    from hmm_training_amd.engine import BaumWelchEngine
    pi, A, B = V.model(4, 8, "dense", np.random.default_rng(1))
    with BaumWelchEngine(4, 8) as e:
        e.set_observations([])
        e.set_params(pi, A, B)
        logp = np.full(1, 7.0)
        assert e._lib.hmmbw_posterior(e._ctx, None, 0, None, 0, logp.ctypes.data) == 0 and logp[0] == 7.0
        gamma, paths, lp = e.posterior()
        assert tuple(gamma.shape) == (0, 4) and paths == [] and lp.shape == (0,)


def test_multi_rank_context_handles_its_shard():
    from hmm_training_amd.engine import shard_bounds
    N, K = 8, 64
    rng = np.random.default_rng(51)
    pi, A, B = V.model(N, K, "dense", rng)
    obs = V.sequences(V.ragged_lengths(N, 8, rng), K, rng)
    lo, hi = shard_bounds([len(o) for o in obs], 2)[1]
    shard = obs[lo:hi]
    gamma, paths, logp = posterior(shard, pi, A, B, "dense", rank=1, world_size=2, native_comm=False)
    P.check_posterior(shard, pi, A, B, gamma, paths, logp)


def test_drop_in_equals_the_engine_call():
    import hmm_training_amd
    from hmm_training_amd.hmm_classes import HMMTrained
    N, K = 5, 16
    rng = np.random.default_rng(61)
    pi, A, B = V.model(N, K, "left_to_right", rng)
    obs = V.sequences(V.ragged_lengths(N, 7, rng), K, rng)
    gammas, paths, logp = hmm_training_amd.posterior_decode(obs, HMMTrained(N, K, A, B, pi, "w"))
    egamma, epaths, elogp = posterior(obs, pi, A, B, "left_to_right")
    assert same_bytes(logp, elogp)
    assert len(gammas) == len(obs) and all(g.shape == (len(o), N) for g, o in zip(gammas, obs))
    assert same_bytes(np.concatenate(gammas), egamma)
    assert all(np.array_equal(p, q) for p, q in zip(paths, epaths))
    P.check_posterior(obs, pi, A, B, gammas, paths, logp)
    assert hmm_training_amd.posterior_decode([], None)[0] == []
