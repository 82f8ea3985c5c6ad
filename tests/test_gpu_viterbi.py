"""Viterbi decoding on the GPU (hmmbw_viterbi, hmm_training_amd/csrc/viterbi.hip) against the NumPy checker of
tests/viterbi_ref.py.  Every case checks (viterbi_ref.check_decode): 1. logp to rtol 1e-9; 2. every returned
path is a valid state sequence whose re-evaluated log-probability is the returned logp (so it is optimal even
where it differs from the checker's); 3. exact path equality wherever the checker's margin exceeds 1e-8, after
asserting from the checker alone that at least 95 % of the sequences clear it; 4. left-to-right paths never
step back or skip; and 5. a scores-only decode returns the same logp bit for bit."""
import ctypes

import numpy as np
import pytest

import viterbi_ref as V

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: the GPU tests need an MI355X")


def decode(obs, pi, A, B, topology, **kw):
    from hmm_training_amd.engine import BaumWelchEngine
    with BaumWelchEngine(len(pi), B.shape[1], topology=topology, **kw) as e:
        e.set_observations(obs)
        e.set_params(pi, A, B)
        paths, logp = e.viterbi()
        none, logp2 = e.viterbi(paths=False)
        assert e.topology == topology
    assert none is None
    assert logp.tobytes() == logp2.tobytes()  # 5
    return paths, logp


def run_case(N, K, topology, T, seed):
    rng = np.random.default_rng(seed)
    pi, A, B = V.model(N, K, topology, rng)
    obs = V.sequences(T, K, rng)
    paths, logp = decode(obs, pi, A, B, topology)
    V.check_decode(obs, pi, A, B, paths, logp, topology)


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


@pytest.mark.parametrize("N,K,topology,T", [(8, 16, "dense", 1), (8, 16, "left_to_right", 13), (20, 16, "dense", 8),
                                            (2, 5, "dense", 9)])
def test_single_sequence(N, K, topology, T):
    run_case(N, K, topology, [T], 3000 + N + T)


def test_exact_ties_take_the_lowest_state():
    N, K = 4, 4
    pi, A, B = np.full(N, 1 / N), np.full((N, N), 1 / N), np.full((N, K), 1 / K)
    rng = np.random.default_rng(5)
    obs = V.sequences(V.ragged_lengths(N, 7, rng), K, rng)
    paths, logp = decode(obs, pi, A, B, "dense")
    for p, o in zip(paths, obs):
        assert p.shape == (len(o),) and np.all(p == 0)
    # every candidate ties whatever the arithmetic, so the margin is 0 and check 3 asks nothing: min_clear = 0
    V.check_decode(obs, pi, A, B, paths, logp, "dense", min_clear=0.0)


def test_zero_probability_sequences():
    # left-to-right from state 0 with T < N: the states past T are unreachable (-inf throughout); one symbol
    # has a zero emission column, so the sequences that contain it have no path
    N, K, zero = 8, 6, 4
    rng = np.random.default_rng(11)
    pi, A, B = V.model(N, K, "left_to_right", rng)
    pi = np.zeros(N)
    pi[0] = 1.0
    B[:, zero] = 0.0
    B /= B.sum(axis=1, keepdims=True)
    obs = V.sequences(rng.integers(1, N, size=45), K, rng)
    obs[0] = np.array([0, 1, 2])          # one that certainly decodes
    obs[1] = np.array([0, zero, 2, 1])    # and one that certainly does not
    paths, logp = decode(obs, pi, A, B, "left_to_right")
    has_zero = np.array([np.any(o == zero) for o in obs])
    assert has_zero.any() and not has_zero.all()
    assert np.all(logp[has_zero] == -np.inf) and np.all(np.isfinite(logp[~has_zero]))
    for r in np.flatnonzero(has_zero):
        assert np.all(paths[r] == -1)
    V.check_decode(obs, pi, A, B, paths, logp, "left_to_right")


@pytest.mark.parametrize("deterministic", [True, False])
def test_decode_does_not_disturb_training(deterministic):
    from hmm_training_amd.engine import BaumWelchEngine
    N, K = 8, 32
    rng = np.random.default_rng(21)
    pi, A, B = V.model(N, K, "left_to_right", rng)
    obs = V.sequences(V.ragged_lengths(N, 17, rng), K, rng)

    def run(with_decode):
        trace = []
        with BaumWelchEngine(N, K, topology="left_to_right", deterministic=deterministic) as e:
            e.set_observations(obs)
            e.set_params(pi, A, B)
            e.train(0.0, 2, lambda k, L, d: trace.append(L))
            ll = e.loglik()
            if with_decode:
                paths, logp = e.viterbi()
                assert np.array_equal(e.loglik(), ll)      # the E-step's log-likelihoods are untouched
                p, a, b = e.params(normalise=False)
                V.check_decode(obs, p, a, b, paths, logp, "left_to_right")
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
    # the context keeps a second pack set for the class-split tables; the decoder reads the first
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
        paths, logp = e.viterbi()
    V.check_decode(obs, p, a, b, paths, logp, "left_to_right")


def test_errors():
    from hmm_training_amd import _lib
    from hmm_training_amd.engine import BaumWelchEngine
    N, K = 4, 8
    rng = np.random.default_rng(41)
    pi, A, B = V.model(N, K, "dense", rng)
    obs = V.sequences([5, 3, 9], K, rng)
    logp = np.zeros(3)
    path = np.zeros(17, dtype=np.int32)
    with BaumWelchEngine(N, K, world_size=2, rank=0, native_comm=False) as e:
        call = lambda lp, pa, n: e._lib.hmmbw_viterbi(e._ctx, lp, pa, n)  # noqa: E731
        assert call(logp.ctypes.data, path.ctypes.data, 17) == _lib.HMMBW_E_STATE      # no observations
        e.set_observations(obs)
        assert call(logp.ctypes.data, path.ctypes.data, 17) == _lib.HMMBW_E_STATE      # no parameters
        e.set_params(pi, A, B)
        assert call(logp.ctypes.data, path.ctypes.data, 16) == _lib.HMMBW_E_INVALID    # wrong path_len
        assert call(logp.ctypes.data, None, 16) == _lib.HMMBW_E_INVALID                # ... also without paths
        assert call(None, path.ctypes.data, 17) == _lib.HMMBW_E_INVALID                # null logp_out
        e.reset(0.0, 5)
        e.iterate_begin()
        assert call(logp.ctypes.data, path.ctypes.data, 17) == _lib.HMMBW_E_STATE      # an iteration is open
        e.iterate_end()
        assert call(logp.ctypes.data, path.ctypes.data, 17) == _lib.HMMBW_OK
        with pytest.raises(ValueError):
            e.n_symbols_total = 16
            e.viterbi()


def test_empty_observations_write_nothing():
    from hmm_training_amd.engine import BaumWelchEngine
    pi, A, B = V.model(4, 8, "dense", np.random.default_rng(1))
    with BaumWelchEngine(4, 8) as e:
        e.set_observations([])
        e.set_params(pi, A, B)
        logp = np.full(1, 7.0)
        assert e._lib.hmmbw_viterbi(e._ctx, logp.ctypes.data, None, 0) == 0 and logp[0] == 7.0
        paths, lp = e.viterbi()
        assert paths == [] and lp.shape == (0,)


def test_multi_rank_context_decodes_its_shard():
    from hmm_training_amd.engine import shard_bounds
    N, K = 8, 64
    rng = np.random.default_rng(51)
    pi, A, B = V.model(N, K, "dense", rng)
    obs = V.sequences(V.ragged_lengths(N, 8, rng), K, rng)
    lo, hi = shard_bounds([len(o) for o in obs], 2)[1]
    shard = obs[lo:hi]
    paths, logp = decode(shard, pi, A, B, "dense", rank=1, world_size=2, native_comm=False)
    V.check_decode(shard, pi, A, B, paths, logp, "dense")


def test_drop_in_equals_the_engine_call():
    import hmm_training_amd
    from hmm_training_amd.hmm_classes import HMMTrained
    N, K = 5, 16
    rng = np.random.default_rng(61)
    pi, A, B = V.model(N, K, "left_to_right", rng)
    obs = V.sequences(V.ragged_lengths(N, 7, rng), K, rng)
    paths, logp = hmm_training_amd.viterbi_decode(obs, HMMTrained(N, K, A, B, pi, "w"))
    epaths, elogp = decode(obs, pi, A, B, "left_to_right")
    assert logp.tobytes() == elogp.tobytes()
    assert all(np.array_equal(p, q) for p, q in zip(paths, epaths))
    V.check_decode(obs, pi, A, B, paths, logp, "left_to_right")
    assert hmm_training_amd.viterbi_decode([], None)[0] == []
