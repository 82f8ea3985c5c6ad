"""Connected-word decoding on the GPU (hmmbw_wordnet_decode, hmm_training_amd/csrc/wordnet.hip) against the NumPy
checker of tests/wordnet_ref.py.  Every case checks: 1. logp to rtol 1e-9; 2. every returned labelling is valid
(states in range, start[0] = 1, an entry step preceded by a last state) and re-scores arc by arc to the returned
logp (so it is optimal even where it differs from the checker's); 3. exact path and start equality wherever the
checker's margin exceeds 1e-8, after asserting from the checker alone that at least 95 % of the sequences clear it;
4. a scores-only decode returns the same logp bit for bit; 5. two calls return identical bytes."""
import numpy as np
import pytest

import viterbi_ref as V
import wordnet_ref as WR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: the GPU tests need an MI355X")


def decode(obs, bank, end_final=False, dense=False, engine_kw=None):
    from hmm_training_amd.engine import BaumWelchEngine
    pi, A, B, init, G = bank
    W, N = pi.shape
    with BaumWelchEngine(N, B.shape[2], **(engine_kw or {})) as e:
        e.set_observations(obs)
        paths, starts, logp = e.wordnet_decode(pi, A, B, init, G, end_final=end_final, dense=dense)
        none, none2, logp2 = e.wordnet_decode(pi, A, B, init, G, end_final=end_final, dense=dense, paths=False)
        paths3, starts3, logp3 = e.wordnet_decode(pi, A, B, init, G, end_final=end_final, dense=dense)
    assert none is None and none2 is None
    assert logp.tobytes() == logp2.tobytes()                                                     # 4
    assert logp.tobytes() == logp3.tobytes()                                                     # 5
    assert all(p.tobytes() == q.tobytes() for p, q in zip(paths, paths3))
    assert all(s.tobytes() == q.tobytes() for s, q in zip(starts, starts3))
    return paths, starts, logp


def run_case(W, N, K, topology, tmin, seed, with_g=True, end_final=False, **kw):
    rng = np.random.default_rng(seed)
    bank = WR.bank(W, N, K, topology, rng)
    if not with_g:
        bank = bank[:4] + (None,)
    obs = V.sequences(V.ragged_lengths(N, tmin, rng), K, rng)
    paths, starts, logp = decode(obs, bank, end_final=end_final, **kw)
    WR.check_decode(obs, bank, paths, starts, logp, end_final=end_final)                         # 1, 2, 3
    return obs, bank, paths, starts, logp


# every group width, each also just above its power of two; (64, 8, 256): the 1 MB table that stays in global memory
BANKS = [(1, 4, 8, "dense"), (3, 3, 8, "left_to_right"), (5, 4, 16, "dense"), (8, 8, 16, "left_to_right"),
         (9, 2, 16, "dense"), (10, 5, 32, "left_to_right"), (17, 8, 64, "dense"), (33, 1, 8, "dense"),
         (64, 8, 256, "left_to_right"), (3, 6, 16, "left_to_right"), (9, 7, 16, "dense")]


@pytest.mark.parametrize("with_g", [True, False])   # False: word_trans = None, the reduction path
@pytest.mark.parametrize("W,N,K,topology", BANKS)
def test_banks(W, N, K, topology, with_g):
    run_case(W, N, K, topology, 9, 500 + 7 * W + N + (0 if with_g else 1000), with_g=with_g)


@pytest.mark.parametrize("tmin", [1, 7, 8, 9, 17])
@pytest.mark.parametrize("W,N,K,topology,with_g", [(3, 3, 8, "left_to_right", True), (10, 5, 32, "left_to_right", False),
                                                   (17, 8, 64, "dense", True), (5, 4, 16, "dense", False)])
def test_lengths_around_the_chunk(tmin, W, N, K, topology, with_g):
    # the eight-step chunk boundary, R that is no multiple of the slots per wave, padding slots
    run_case(W, N, K, topology, tmin, 2000 + 13 * tmin + W, with_g=with_g, end_final=(tmin % 2 == 1))


@pytest.mark.parametrize("K", [256, 300])
def test_pack_forms(K):
    # N = 8, K = 256: the E-step's tables live in LDS and the packs hold scaled row offsets; K = 300: symbol ids
    run_case(5, 8, K, "left_to_right", 9, 3000 + K)


def test_single_sequence_and_single_step():
    for T in (1, 13):
        rng = np.random.default_rng(3100 + T)
        bank = WR.bank(10, 5, 32, "left_to_right", rng)
        obs = [rng.integers(0, 32, size=T)]
        paths, starts, logp = decode(obs, bank)
        WR.check_decode(obs, bank, paths, starts, logp, min_clear=0.0)


def words_of(path, start, N):
    return [int(path[t]) // N for t in np.flatnonzero(start)]


# 10 words x 5 states: with five states per word a spurious or a missed word needs a run of wrong symbols (each has
# probability 0.1) that also lines up with another word's states; at three states per word single wrong symbols at a
# word boundary already cost the checker itself a word in some draws.
RECOVERY = dict(W=10, N=5, n_seq=60, seed=4000)


def recovery_case():
    rng = np.random.default_rng(RECOVERY["seed"])
    obs, words = WR.word_sequences(RECOVERY["W"], RECOVERY["N"], RECOVERY["n_seq"], rng)
    return obs, words, WR.recovery_bank(RECOVERY["W"], RECOVERY["N"], rng)


@pytest.mark.parametrize("trans", ["ones", "uniform"])
def test_recovery_of_the_spoken_words(trans):
    W, N = RECOVERY["W"], RECOVERY["N"]
    obs, words, (pi, A, B) = recovery_case()
    assert any(a == b for ws in words for a, b in zip(ws, ws[1:]))  # immediate repeats of a word occur
    G = np.ones((W, W)) if trans == "ones" else np.full((W, W), 1.0 / W)
    bank = (pi, A, B, np.ones(W), G)
    paths, starts, logp = decode(obs, bank, end_final=True)
    rpaths, rstarts, _, _ = WR.check_decode(obs, bank, paths, starts, logp, end_final=True)
    assert all(words_of(p, s, N) == ws for p, s, ws in zip(rpaths, rstarts, words))  # the checker alone recovers all
    for r, (p, s) in enumerate(zip(paths, starts)):
        assert words_of(p, s, N) == words[r], r


def test_grammar_of_consecutive_words():
    W, N, K = 6, 3, 16
    rng = np.random.default_rng(4100)
    pi, A, B, init, _ = WR.bank(W, N, K, "dense", rng)
    G = np.zeros((W, W))
    G[np.arange(W - 1), np.arange(1, W)] = 1.0
    bank = (pi, A, B, init, G)
    obs = V.sequences(V.ragged_lengths(N, 9, rng), K, rng)
    paths, starts, logp = decode(obs, bank)
    WR.check_decode(obs, bank, paths, starts, logp)
    assert np.all(np.isfinite(logp))
    seen = 0
    for p, s in zip(paths, starts):
        ws = words_of(p, s, N)
        assert ws == list(range(ws[0], ws[0] + len(ws)))
        seen = max(seen, len(ws))
    assert seen > 1  # word transitions occurred


@pytest.mark.parametrize("W,N,K", [(3, 3, 8), (10, 5, 32)])
def test_dense_flag_on_a_left_to_right_bank(W, N, K):
    rng = np.random.default_rng(4200 + W)
    bank = WR.bank(W, N, K, "left_to_right", rng)
    obs = V.sequences(V.ragged_lengths(N, 9, rng), K, rng)
    paths, starts, logp = decode(obs, bank)
    dpaths, dstarts, dlogp = decode(obs, bank, dense=True)
    np.testing.assert_allclose(dlogp, logp, rtol=V.RTOL)
    _, _, _, margin = WR.check_decode(obs, bank, dpaths, dstarts, dlogp)
    for r in np.flatnonzero(margin > V.MARGIN):
        assert np.array_equal(paths[r], dpaths[r]) and np.array_equal(starts[r], dstarts[r]), r


def test_cross_check_against_the_state_decoder_on_the_composite():
    # hmmbw_viterbi on the 50-state composite model: no kernel in common with the word-loop decoder
    from hmm_training_amd.engine import BaumWelchEngine
    W, N, K = 10, 5, 32
    rng = np.random.default_rng(4300)
    bank = WR.bank(W, N, K, "left_to_right", rng)
    obs = V.sequences(V.ragged_lengths(N, 9, rng), K, rng)
    _, _, logp = decode(obs, bank)
    cpi, cA, cB = WR.composite(*bank)
    with BaumWelchEngine(W * N, K, topology="dense") as e:
        e.set_observations(obs)
        e.set_params(cpi, cA, cB)
        _, clogp = e.viterbi(paths=False)
    np.testing.assert_allclose(logp, clogp, rtol=V.RTOL)


def test_exact_ties_take_composite_state_zero():
    W, N, K = 5, 4, 4
    bank = (np.full((W, N), 1 / N), np.full((W, N, N), 1 / N), np.full((W, N, K), 1 / K), np.full(W, 1 / W),
            np.full((W, W), 1 / W))
    rng = np.random.default_rng(5)
    obs = V.sequences(V.ragged_lengths(N, 7, rng), K, rng)
    for b in (bank, bank[:4] + (None,)):
        paths, starts, logp = decode(obs, b)
        for p, s, o in zip(paths, starts, obs):
            assert p.shape == s.shape == (len(o),) and np.all(p == 0) and s[0] == 1 and np.all(s[1:] == 0)
        # every candidate ties whatever the arithmetic, so the margin is 0 and check 3 asks nothing: min_clear = 0
        WR.check_decode(obs, b, paths, starts, logp, min_clear=0.0)


def test_dead_sequences_beside_live_ones():
    # one symbol has a zero emission column in every word: the sequences that contain it have no path
    W, N, K, zero = 10, 5, 8, 4
    rng = np.random.default_rng(11)
    pi, A, B, init, G = WR.bank(W, N, K, "left_to_right", rng)
    B[:, :, zero] = 0.0
    B /= B.sum(axis=2, keepdims=True)
    bank = (pi, A, B, init, G)
    obs = V.sequences(rng.integers(1, 12, size=45), K, rng)
    obs[0] = np.array([0, 1, 2])          # one that certainly decodes
    obs[1] = np.array([0, zero, 2, 1])    # and one that certainly does not (four sequences share a wave)
    paths, starts, logp = decode(obs, bank)
    has_zero = np.array([np.any(o == zero) for o in obs])
    assert has_zero.any() and not has_zero.all()
    assert np.all(logp[has_zero] == -np.inf) and np.all(np.isfinite(logp[~has_zero]))
    for r in np.flatnonzero(has_zero):
        assert np.all(paths[r] == -1) and np.all(starts[r] == 0)
    WR.check_decode(obs, bank, paths, starts, logp)


@pytest.mark.parametrize("deterministic", [True, False])
def test_decode_does_not_disturb_training(deterministic):
    from hmm_training_amd.engine import BaumWelchEngine
    N, K, W = 8, 32, 5
    rng = np.random.default_rng(21)
    pi, A, B = V.model(N, K, "left_to_right", rng)
    obs = V.sequences(V.ragged_lengths(N, 17, rng), K, rng)
    bank = WR.bank(W, N, K, "left_to_right", rng)

    def run(with_decode):
        trace = []
        with BaumWelchEngine(N, K, topology="left_to_right", deterministic=deterministic) as e:
            e.set_observations(obs)
            e.set_params(pi, A, B)
            e.train(0.0, 2, lambda k, L, d: trace.append(L))
            ll = e.loglik()
            if with_decode:
                before = e.params(normalise=False)
                paths, starts, logp = e.wordnet_decode(*bank)
                assert np.array_equal(e.loglik(), ll)      # the E-step's log-likelihoods are untouched
                assert all(np.array_equal(x, y) for x, y in zip(e.params(normalise=False), before))
                WR.check_decode(obs, bank, paths, starts, logp)
            e.train(0.0, 2, lambda k, L, d: trace.append(L))
            return e.params(normalise=False), np.array(trace), ll

    (p1, t1, l1), (p0, t0, l0) = run(True), run(False)
    assert len(t1) == len(t0) == 4
    for x, y in list(zip(p1, p0)) + [(t1, t0), (l1, l0)]:
        if deterministic:
            assert np.array_equal(x, y)
        else:
            np.testing.assert_allclose(x, y, rtol=1e-12)


def test_errors():
    from hmm_training_amd import _lib
    from hmm_training_amd.engine import BaumWelchEngine
    W, N, K = 3, 4, 8
    rng = np.random.default_rng(41)
    pi, A, B, init, G = WR.bank(W, N, K, "dense", rng)
    obs = V.sequences([5, 3, 9], K, rng)
    logp = np.zeros(3)
    path = np.zeros(17, dtype=np.int32)
    start = np.zeros(17, dtype=np.uint8)
    big = WR.bank(65, N, K, "dense", rng)
    ptr = lambda x: None if x is None else x.ctypes.data  # noqa: E731

    def call(e, n_words, bank, path_, start_, n, lp=logp):
        p, a, b, i, g = bank
        return e._lib.hmmbw_wordnet_decode(e._ctx, n_words, ptr(p), ptr(a), ptr(b), ptr(i), ptr(g), 0, ptr(lp),
                                           ptr(path_), ptr(start_), n)

    good = (pi, A, B, init, G)
    with BaumWelchEngine(N, K) as e:
        assert call(e, W, good, path, start, 17) == _lib.HMMBW_E_STATE            # no observations
        e.set_observations(obs)
        assert call(e, 0, good, path, start, 17) == _lib.HMMBW_E_INVALID          # n_words < 1
        assert call(e, 65, big, path, start, 17) == _lib.HMMBW_E_UNSUPPORTED      # more than 64 words
        assert call(e, W, good, path, start, 16) == _lib.HMMBW_E_INVALID          # wrong path_len
        assert call(e, W, good, None, None, 16) == _lib.HMMBW_E_INVALID           # ... also without paths
        assert call(e, W, good, None, start, 17) == _lib.HMMBW_E_INVALID          # start_out without path_out
        assert call(e, W, (None, A, B, init, G), path, start, 17) == _lib.HMMBW_E_INVALID  # a NULL bank pointer
        assert call(e, W, good, path, start, 17, lp=None) == _lib.HMMBW_E_INVALID
        neg = G.copy()
        neg[1, 2] = -0.1
        assert call(e, W, (pi, A, B, init, neg), path, start, 17) == _lib.HMMBW_E_INVALID  # a negative weight
        nan = init.copy()
        nan[0] = np.nan
        assert call(e, W, (pi, A, B, nan, G), path, start, 17) == _lib.HMMBW_E_INVALID     # a NaN weight
        with pytest.raises(ValueError):
            e.wordnet_decode(pi, A, B, init, neg)
        # the context still works afterwards, without parameters of its own
        assert call(e, W, good, path, start, 17) == _lib.HMMBW_OK
        assert call(e, W, good, path, None, 17) == _lib.HMMBW_OK                  # paths without start flags
        paths, starts, lp = e.wordnet_decode(*good)
        assert np.array_equal(np.concatenate(paths), path) and np.array_equal(np.concatenate(starts), start)
        WR.check_decode(obs, good, paths, starts, lp, min_clear=0.0)
    nine = WR.bank(2, 9, K, "dense", rng)
    with BaumWelchEngine(9, K) as e:
        e.set_observations(obs)
        assert call(e, 2, nine, path, start, 17) == _lib.HMMBW_E_UNSUPPORTED      # a context with N = 9
        pi9, A9, B9 = V.model(9, K, "dense", rng)
        e.set_params(pi9, A9, B9)
        p9, l9 = e.viterbi()                                                      # the context still works
        V.check_decode(obs, pi9, A9, B9, p9, l9, "dense", min_clear=0.0)


def test_empty_observations_write_nothing():
    from hmm_training_amd.engine import BaumWelchEngine
    bank = WR.bank(3, 4, 8, "dense", np.random.default_rng(1))
    with BaumWelchEngine(4, 8) as e:
        e.set_observations([])
        paths, starts, lp = e.wordnet_decode(*bank)
        assert paths == [] and starts == [] and lp.shape == (0,)
        assert e.wordnet_decode(*bank, paths=False)[2].shape == (0,)


def test_multi_rank_context_decodes_its_shard():
    from hmm_training_amd.engine import shard_bounds
    W, N, K = 9, 2, 16
    rng = np.random.default_rng(51)
    bank = WR.bank(W, N, K, "dense", rng)
    obs = V.sequences(V.ragged_lengths(N, 8, rng), K, rng)
    lo, hi = shard_bounds([len(o) for o in obs], 2)[1]
    shard = obs[lo:hi]
    paths, starts, logp = decode(shard, bank, engine_kw=dict(rank=1, world_size=2, native_comm=False))
    WR.check_decode(shard, bank, paths, starts, logp)


def test_group_width_changes_between_calls():
    # one context, banks of 3 and then 20 and then 3 words: the back-pointer rows are planned again per group width
    from hmm_training_amd.engine import BaumWelchEngine
    N, K = 3, 8
    rng = np.random.default_rng(61)
    obs = V.sequences(V.ragged_lengths(N, 9, rng), K, rng)
    small, large = WR.bank(3, N, K, "left_to_right", rng), WR.bank(20, N, K, "left_to_right", rng)
    with BaumWelchEngine(N, K) as e:
        e.set_observations(obs)
        for bank in (small, large, small):
            paths, starts, logp = e.wordnet_decode(*bank)
            WR.check_decode(obs, bank, paths, starts, logp)


def test_decode_words_end_to_end():
    import hmm_training_amd
    from hmm_training_amd.hmm_classes import HMMTrained
    W, N = RECOVERY["W"], RECOVERY["N"]
    obs, words, (pi, A, B) = recovery_case()
    names = ["forward", "back", "left", "right", "stop", "go", "up", "down", "faster", "slower"]
    models = [HMMTrained(N, W * N, A[w], B[w], pi[w], names[w]) for w in range(W)]
    segments, logp = hmm_training_amd.decode_words(obs, models)
    assert logp.shape == (len(obs),) and np.all(np.isfinite(logp))
    for r, seg in enumerate(segments):
        assert [name for name, _, _ in seg] == [names[w] for w in words[r]], r
        assert seg[0][1] == 0 and seg[-1][2] == len(obs[r])
        assert all(a[2] == b[1] for a, b in zip(seg, seg[1:]))      # the segments tile the recording
        assert all(e - s >= N for _, s, e in seg)                   # a left-to-right word takes N frames at least
