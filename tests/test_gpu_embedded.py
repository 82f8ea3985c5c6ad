"""Embedded training on the GPU (hmmbw_embedded_train, hmm_training_amd/csrc/embedded.hip) against the NumPy checker
of tests/embedded_ref.py, and with one-word transcripts against the reference's own training (the oracle).  The
project's tolerances: log P and L at rtol 1e-9, parameters 1e-6 relative (+ 1e-15 absolute, which also covers an
entry that is the 1e-20 floor in one computation and a denormal quotient in the other).  The sums are floating-point
atomics, so no test compares two calls bit for bit."""
import os

import numpy as np
import pytest

import embedded_ref as ER
import viterbi_ref as V
import wordnet_ref as WR
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

LL_RTOL = ER.LL_RTOL


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: the GPU tests need an MI355X")


def gpu_train(obs, transcripts, bank, **kw):
    from hmm_training_amd.engine import BaumWelchEngine
    pi, A, B = bank
    with BaumWelchEngine(pi.shape[1], B.shape[2]) as e:
        e.set_observations(obs)
        return e.embedded_train(pi, A, B, transcripts, **kw)


def assert_no_nan(*arrays):
    for x in arrays:
        assert not np.any(np.isnan(np.asarray(x, dtype=float)))


def compare(got, ref):
    """GPU (pi, A, B, records, logp) against the checker's (pi, A, B, records, logp, stats)."""
    pi, A, B, recs, logp = got
    rpi, rA, rB, rrecs, rlogp = ref[:5]
    assert_no_nan(pi, A, B, logp, [L for L, _ in recs], [d for _, d in recs])
    assert len(recs) == len(rrecs)
    assert np.array_equal(logp == -np.inf, rlogp == -np.inf)
    np.testing.assert_allclose(logp, rlogp, rtol=LL_RTOL)
    np.testing.assert_allclose([L for L, _ in recs], [L for L, _ in rrecs], rtol=LL_RTOL)
    np.testing.assert_allclose([d for _, d in recs[1:]], [d for _, d in rrecs[1:]], rtol=1e-6, atol=1e-9)
    assert recs[0][1] == np.inf
    ER.close(pi, rpi, "pi")
    ER.close(A, rA, "A")
    ER.close(B, rB, "B")


# every dense / left-to-right kernel family; (64, 8, 256): the 1 MB emission table that stays in global memory
BANKS = [(1, 4, 8, "dense"), (3, 3, 8, "left_to_right"), (5, 4, 16, "dense"), (8, 8, 16, "left_to_right"),
         (10, 5, 32, "left_to_right"), (17, 8, 64, "dense"), (64, 8, 256, "left_to_right"),
         (3, 6, 16, "left_to_right"), (9, 7, 16, "dense")]
LONGEST = [1, 2, 8, 9, 16, 17, 33, 64]  # every group width, each also just above its power of two
_cases = {}


def case(W, N, K, topology, longest):
    """(obs, transcripts, bank), made once: R is no multiple of the 64 / GW slots of a wave; the first transcript has
    `longest` words, the others 1 .. longest, immediate repeats included; T from the transcript's length (the
    shortest an utterance can be) up to about 3 L N, the first ones just around the 8-step chunk."""
    key = (W, N, K, topology, longest)
    if key not in _cases:
        rng = np.random.default_rng(7000 + 131 * W + 17 * N + longest)
        pi, A, B, _, _ = WR.bank(W, N, K, topology, rng)
        GW = 8 if longest <= 8 else 16 if longest <= 16 else 32 if longest <= 32 else 64
        R = 2 * (64 // GW) + 3
        lens = [longest] + [int(x) for x in rng.integers(1, longest + 1, size=R - 1)]
        transcripts = ER.transcripts_for(W, lens, rng)
        T = [int(rng.integers(L, 3 * L * N + 1)) for L in lens]
        for r, t in zip(range(1, R), (7, 8, 9, 17)):
            T[r] = max(t, lens[r])
        T[0] = 3 * longest * N  # the longest chain at its longest
        _cases[key] = (V.sequences(T, K, rng), transcripts, (pi, A, B))
    return _cases[key]


@pytest.mark.parametrize("longest", LONGEST)
@pytest.mark.parametrize("W,N,K,topology", BANKS)
def test_one_iteration_at_every_group_width(W, N, K, topology, longest):
    obs, transcripts, bank = case(W, N, K, topology, longest)
    end_final = (W + longest) % 2 == 1
    ref = ER.train(obs, transcripts, *bank, 0.0, 1, end_final=end_final)
    assert np.isfinite(ref[4]).any()
    compare(gpu_train(obs, transcripts, bank, epsilon=0.0, max_iterations=1, end_final=end_final, normalise=False), ref)


@pytest.mark.parametrize("longest", LONGEST)
@pytest.mark.parametrize("W,N,K,topology", BANKS[:3] + BANKS[4:5])
def test_three_iterations_and_continuation(W, N, K, topology, longest):
    obs, transcripts, bank = case(W, N, K, topology, longest)
    ref = ER.train(obs, transcripts, *bank, 0.0, 3)
    three = gpu_train(obs, transcripts, bank, epsilon=0.0, max_iterations=3, normalise=False)
    compare(three, ref)
    two = gpu_train(obs, transcripts, bank, epsilon=0.0, max_iterations=2, normalise=False)
    one = gpu_train(obs, transcripts, two[:3], epsilon=0.0, max_iterations=1, normalise=False)
    for x, y, what in zip(one[:3], three[:3], ("pi", "A", "B")):
        ER.close(x, y, what)
    np.testing.assert_allclose([L for L, _ in two[3] + one[3]], [L for L, _ in three[3]], rtol=LL_RTOL)
    np.testing.assert_allclose(one[4], three[4], rtol=LL_RTOL)
    # normalise = 1 is the reference's return path on the same working parameters
    norm = gpu_train(obs, transcripts, bank, epsilon=0.0, max_iterations=3, normalise=True)
    for x, y, what in zip(norm[:3], ER.normalised(*ref[:3], ref[5].count), ("pi", "A", "B")):
        ER.close(x, y, what)


def test_stops_on_epsilon():
    obs, transcripts, bank = case(3, 3, 8, "left_to_right", 2)
    ref = ER.train(obs, transcripts, *bank, 1e-3, 40)
    assert 2 < len(ref[3]) < 40 and ref[3][-1][1] < 1e-3 <= ref[3][-2][1]  # the checker alone: it stops on epsilon
    got = gpu_train(obs, transcripts, bank, epsilon=1e-3, max_iterations=40, normalise=False)
    compare(got, ref)


# --------------------------------------------------------------------------------------------------------------
# one-word transcripts: the reference's own training
# --------------------------------------------------------------------------------------------------------------
def oracle_alone(oracle, obs, N, K, pi0, A0, B0, iters=5):
    off, sym = oracle.to_csr(obs)
    return oracle.hmm_training(off, sym, N, K, 0.0, iters, pi0, A0, B0)


def check_against_oracle(oracle, sets, N, K, models):
    """sets[w]: the utterances of word w; trained together, interleaved, each word is the oracle's run on its own."""
    W = len(sets)
    order = sorted((r, w) for w in range(W) for r in range(len(sets[w])))
    obs = [sets[w][r] for r, w in order]
    transcripts = [[w] for _, w in order]
    bank = tuple(np.stack([m[i] for m in models]) for i in range(3))
    pi, A, B, recs, logp = gpu_train(obs, transcripts, bank, epsilon=0.0, max_iterations=5, normalise=True)
    wpi, wA, wB, _, _ = gpu_train(obs, transcripts, bank, epsilon=0.0, max_iterations=5, normalise=False)
    assert_no_nan(pi, A, B, wpi, wA, wB, logp)
    refs = [oracle_alone(oracle, sets[w], N, K, *models[w]) for w in range(W)]
    assert len(recs) == 5 and all(ref.iterations == 5 for ref in refs)
    with np.errstate(invalid="ignore"):
        L = np.logaddexp.reduce(np.stack([ref.trace_L for ref in refs]), axis=0)  # LSE over all utterances
    np.testing.assert_allclose([x for x, _ in recs], L, rtol=LL_RTOL)
    for w, ref in enumerate(refs):
        mine = np.array([logp[i] for i, (_, v) in enumerate(order) if v == w])
        assert np.array_equal(mine == -np.inf, ref.logP == -np.inf)
        np.testing.assert_allclose(mine, ref.logP, rtol=LL_RTOL)
        ER.close(pi[w], ref.pi, "pi")
        ER.close(A[w], ref.A, "A")
        ER.close(B[w], ref.B, "B")
        ER.close(wpi[w], np.exp(ref.log_pi), "working pi")
        ER.close(wA[w], np.exp(ref.log_A), "working A")
        ER.close(wB[w], np.exp(ref.log_B), "working B")


@pytest.mark.parametrize("W,N,K,topology", [(1, 4, 16, "dense"), (3, 5, 32, "left_to_right"), (3, 4, 16, "dense")])
def test_one_word_transcripts_are_the_oracle(oracle, W, N, K, topology):
    rng = np.random.default_rng(8000 + W + N)
    models = []
    for _ in range(W):
        pi0, A0, B0 = V.model(N, K, topology, rng)
        models.append((rng.dirichlet(np.ones(N)) if topology == "dense" else pi0, A0, B0))
    sets = [V.sequences(rng.integers(6, 40, size=9 + 2 * w), K, rng) for w in range(W)]
    check_against_oracle(oracle, sets, N, K, models)


@pytest.mark.parametrize("golden", ["zero_prob_seq", "t1_edge", "empty_rows"])
def test_one_word_transcripts_on_the_goldens(oracle, golden):
    d = np.load(os.path.join(GOLDEN, f"bw_{golden}.npz"), allow_pickle=False)
    off, sym = d["offsets"], d["symbols"]
    obs = [sym[off[r]:off[r + 1]] for r in range(len(off) - 1)]
    check_against_oracle(oracle, [obs], int(d["N"]), int(d["M"]), [(d["init_pi"], d["init_A"], d["init_B"])])


# --------------------------------------------------------------------------------------------------------------
# edge cases
# --------------------------------------------------------------------------------------------------------------
def lr_bank(W, N, K, rng):
    pi, A, B, _, _ = WR.bank(W, N, K, "left_to_right", rng)
    pi[:] = 0.0
    pi[:, 0] = 1.0  # entered at state 0: an instance takes N frames at least
    return pi, A, B


def test_an_utterance_too_short_for_its_transcript():
    W, N, K = 4, 3, 8
    rng = np.random.default_rng(8100)
    bank = lr_bank(W, N, K, rng)
    transcripts = [[0, 1], [2, 2, 3], [1], [3, 0, 1, 2], [0]]
    # utterance 3: T = 9 < L N = 12, and below the (L - 1) N + 1 = 10 frames that reach the last word's first state
    obs = V.sequences([9, 14, 5, 9, 4], K, rng)
    for end_final in (False, True):
        ref = ER.train(obs, transcripts, *bank, 0.0, 1, end_final=end_final)
        assert (ref[4] == -np.inf).tolist() == [False, False, False, True, False]
        got = gpu_train(obs, transcripts, bank, epsilon=0.0, max_iterations=1, end_final=end_final, normalise=False)
        compare(got, ref)
        assert got[4][3] == -np.inf
        # the other utterances' statistics are what they are without it; only count, the divisor of pi, differs
        keep = [0, 1, 2, 4]
        alone = gpu_train([obs[r] for r in keep], [transcripts[r] for r in keep], bank, epsilon=0.0, max_iterations=1,
                          end_final=end_final, normalise=False)
        ER.close(got[1], alone[1], "A")
        ER.close(got[2], alone[2], "B")
        count = np.bincount(sum(transcripts, []), minlength=W)
        count_alone = np.bincount(sum((transcripts[r] for r in keep), []), minlength=W)
        ER.close(got[0] * count[:, None], alone[0] * count_alone[:, None], "entry")
        np.testing.assert_allclose(got[4][keep], alone[4], rtol=LL_RTOL)


def test_every_utterance_dead():
    W, N, K = 2, 3, 8
    rng = np.random.default_rng(8150)
    bank = lr_bank(W, N, K, rng)
    obs = V.sequences([3, 2], K, rng)  # fewer than the (L - 1) N + 1 = 4 frames that reach the second word
    pi, A, B, recs, logp = gpu_train(obs, [[0, 1], [1, 1]], bank, epsilon=0.0, max_iterations=2, normalise=True)
    assert_no_nan(pi, A, B)
    assert np.all(logp == -np.inf) and [L for L, _ in recs] == [-np.inf, -np.inf] and recs[0][1] == np.inf
    compare((pi, A, B, recs, logp), ER.train(obs, [[0, 1], [1, 1]], *bank, 0.0, 2, normalise=True))
    assert not pi.any() and not A.any() and not B.any()  # nothing was explained: the reference's rule gives zeros


@pytest.mark.parametrize("normalise", [False, True])
def test_a_word_without_an_instance_comes_back_bit_identical(normalise):
    W, N, K = 5, 4, 16
    rng = np.random.default_rng(8200)
    pi, A, B, _, _ = WR.bank(W, N, K, "dense", rng)
    pi[2], A[2], B[2] = 3.0 * pi[2], 0.5 * A[2], 7.0 * B[2]  # working parameters: not normalised
    transcripts = [[0, 1], [4, 4, 3], [1], [3, 0]]           # word 2 has no instance
    obs = V.sequences([9, 14, 5, 11], K, rng)
    got = gpu_train(obs, transcripts, (pi, A, B), epsilon=0.0, max_iterations=2, normalise=normalise)
    assert got[0][2].tobytes() == pi[2].tobytes() and got[1][2].tobytes() == A[2].tobytes()
    assert got[2][2].tobytes() == B[2].tobytes()
    compare(got, ER.train(obs, transcripts, pi, A, B, 0.0, 2, normalise=normalise))


@pytest.mark.parametrize("W,N,K,longest", [(3, 3, 8, 2), (10, 5, 32, 9), (8, 8, 16, 17)])
def test_dense_flag_on_a_left_to_right_bank(W, N, K, longest):
    obs, transcripts, bank = case(W, N, K, "left_to_right", longest)
    for end_final in (False, True):
        lr = gpu_train(obs, transcripts, bank, epsilon=0.0, max_iterations=2, end_final=end_final, normalise=False)
        dn = gpu_train(obs, transcripts, bank, epsilon=0.0, max_iterations=2, end_final=end_final, dense=True, normalise=False)
        for x, y in zip(lr[:3], dn[:3]):
            np.testing.assert_allclose(x, y, rtol=1e-12, atol=0)
        np.testing.assert_allclose(lr[4], dn[4], rtol=1e-12)
        np.testing.assert_allclose([L for L, _ in lr[3]], [L for L, _ in dn[3]], rtol=1e-12)


@pytest.mark.parametrize("K", [256, 300])
def test_pack_forms(K):
    # N = 8, K = 256: the E-step's tables live in LDS and the packs hold scaled row offsets; K = 300: symbol ids
    rng = np.random.default_rng(8300 + K)
    bank = WR.bank(5, 8, K, "left_to_right", rng)[:3]
    lens = [3, 1, 2, 3, 1, 2, 2]
    transcripts = ER.transcripts_for(5, lens, rng)
    obs = V.sequences([int(rng.integers(L, 3 * L * 8)) for L in lens], K, rng)
    compare(gpu_train(obs, transcripts, bank, epsilon=0.0, max_iterations=1, normalise=False),
            ER.train(obs, transcripts, *bank, 0.0, 1))


# --------------------------------------------------------------------------------------------------------------
# errors, and a context that is left as it was
# --------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_context_as_it_was(oracle):
    from hmm_training_amd import _lib
    from hmm_training_amd.engine import BaumWelchEngine
    W, N, K = 3, 4, 8
    rng = np.random.default_rng(8400)
    pi, A, B, _, _ = WR.bank(W, N, K, "dense", rng)
    obs = V.sequences([5, 3, 9], K, rng)
    off = np.array([0, 2, 3, 5], dtype=np.int64)
    ids = np.array([0, 1, 2, 2, 0], dtype=np.int32)
    ptr = lambda x: None if x is None else x.ctypes.data  # noqa: E731

    def call(e, n_words=W, bank=(pi, A, B), off_=off, ids_=ids, n=3, flags=0, eps=0.0, iters=1):
        p, a, b = (None if x is None else x.copy() for x in bank)
        return e._lib.hmmbw_embedded_train(e._ctx, n_words, ptr(p), ptr(a), ptr(b), ptr(off_), ptr(ids_), n, flags, eps,
                                           iters, 0, None, 0, None, None)

    def spoiled(x, value):
        y = x.copy()
        y.reshape(-1)[3] = value
        return y

    mpi, mA, mB = V.model(N, K, "dense", rng)
    with BaumWelchEngine(N, K) as e:
        assert call(e) == _lib.HMMBW_E_STATE                                           # no observations
        e.set_observations(obs)
        e.set_params(mpi, mA, mB)
        e.train(0.0, 2)
        before = (e.loglik().tobytes(), [x.tobytes() for x in e.params(normalise=False)], bytes(e.status()[0]))
        assert call(e, n_words=0) == _lib.HMMBW_E_INVALID
        for bank in ((None, A, B), (pi, None, B), (pi, A, None)):
            assert call(e, bank=bank) == _lib.HMMBW_E_INVALID                          # a NULL bank pointer
        assert call(e, off_=None) == _lib.HMMBW_E_INVALID and call(e, ids_=None) == _lib.HMMBW_E_INVALID
        assert call(e, n=2) == _lib.HMMBW_E_INVALID                                    # not the loaded count
        assert call(e, off_=np.array([0, 2, 2, 5], dtype=np.int64)) == _lib.HMMBW_E_INVALID   # an empty transcript
        assert call(e, ids_=np.array([0, 1, 3, 2, 0], dtype=np.int32)) == _lib.HMMBW_E_INVALID   # a word id = W
        assert call(e, ids_=np.array([0, -1, 2, 2, 0], dtype=np.int32)) == _lib.HMMBW_E_INVALID
        for bad in (-0.1, np.inf, np.nan):
            assert call(e, bank=(spoiled(pi, bad), A, B)) == _lib.HMMBW_E_INVALID
            assert call(e, bank=(pi, spoiled(A, bad), B)) == _lib.HMMBW_E_INVALID
            assert call(e, bank=(pi, A, spoiled(B, bad))) == _lib.HMMBW_E_INVALID
        assert call(e, iters=0) == _lib.HMMBW_E_INVALID
        assert call(e, eps=-1e-9) == _lib.HMMBW_E_INVALID and call(e, eps=np.nan) == _lib.HMMBW_E_INVALID
        assert call(e, flags=4) == _lib.HMMBW_E_INVALID                                # an unknown flag bit
        big = WR.bank(65, N, K, "dense", rng)[:3]
        assert call(e, n_words=65, bank=big) == _lib.HMMBW_E_UNSUPPORTED               # more than 64 words
        long_off = np.array([0, 65, 66, 67], dtype=np.int64)
        assert call(e, off_=long_off, ids_=np.zeros(67, dtype=np.int32)) == _lib.HMMBW_E_UNSUPPORTED  # a 65-word transcript
        with pytest.raises(ValueError):
            e.embedded_train(pi, A, B, [[0, 1], [], [2, 0]])
        # the context is as it was, byte for byte; a good call changes nothing of the context's own either
        assert (e.loglik().tobytes(), [x.tobytes() for x in e.params(normalise=False)], bytes(e.status()[0])) == before
        transcripts = [[0, 1], [2], [2, 0]]
        got = e.embedded_train(pi, A, B, transcripts, epsilon=0.0, max_iterations=2, normalise=False)
        compare(got, ER.train(obs, transcripts, pi, A, B, 0.0, 2))
        assert (e.loglik().tobytes(), [x.tobytes() for x in e.params(normalise=False)], bytes(e.status()[0])) == before
        # ... and it still decodes, scores and trains
        ep = e.params(normalise=False)
        paths, logp = e.viterbi()
        V.check_decode(obs, *ep, paths, logp, "dense", min_clear=0.0)
        off64, sym64 = oracle.to_csr(obs)
        np.testing.assert_allclose(e.score(), oracle.forward_loglik(off64, sym64, N, K, *ep), rtol=LL_RTOL)
        trace = []
        e.set_params(mpi, mA, mB)
        e.train(0.0, 3, lambda k, L, d: trace.append(L))
        np.testing.assert_allclose(trace, oracle.hmm_training(off64, sym64, N, K, 0.0, 3, mpi, mA, mB).trace_L, rtol=LL_RTOL)
        # an open iteration
        e.reset(0.0, 3)
        e.iterate_begin()
        assert call(e) == _lib.HMMBW_E_STATE
        e.iterate_end()
        assert call(e) == _lib.HMMBW_OK
    with BaumWelchEngine(9, K) as e:                                                   # a context with N = 9
        e.set_observations(obs)
        nine = WR.bank(2, 9, K, "dense", rng)[:3]
        assert call(e, n_words=2, bank=nine, ids_=np.array([0, 1, 1, 1, 0], dtype=np.int32)) == _lib.HMMBW_E_UNSUPPORTED
    with BaumWelchEngine(N, K, rank=0, world_size=2, native_comm=False) as e:          # no collective is built here
        e.set_observations(obs)
        assert call(e) == _lib.HMMBW_E_UNSUPPORTED
    with BaumWelchEngine(N, K, deterministic=True) as e:
        e.set_observations(obs)
        assert call(e) == _lib.HMMBW_E_UNSUPPORTED


def test_empty_observations_train_nothing():
    from hmm_training_amd.engine import BaumWelchEngine
    pi, A, B, _, _ = WR.bank(3, 4, 8, "dense", np.random.default_rng(1))
    with BaumWelchEngine(4, 8) as e:
        e.set_observations([])
        p, a, b, recs, logp = e.embedded_train(pi, A, B, [])
        assert recs == [] and logp.shape == (0,)
        assert np.array_equal(p, pi) and np.array_equal(a, A) and np.array_equal(b, B)


# --------------------------------------------------------------------------------------------------------------
# recovery from a near-flat start, and the Python layers
# --------------------------------------------------------------------------------------------------------------
RECOVERY = dict(W=6, N=3, n_seq=120, iters=12)


def recovery_case():
    W, N = RECOVERY["W"], RECOVERY["N"]
    rng = np.random.default_rng(1)
    obs, words = WR.word_sequences(W, N, RECOVERY["n_seq"], rng, max_words=4)
    return obs, words, ER.flat_start(W, N, W * N, rng)


def words_of(path, start, N):
    return [int(path[t]) // N for t in np.flatnonzero(start)]


def test_recovery_from_a_near_flat_start():
    import hmm_training_amd
    from hmm_training_amd.hmm_classes import HMMTrained
    W, N, iters = RECOVERY["W"], RECOVERY["N"], RECOVERY["iters"]
    obs, words, start = recovery_case()
    ref = ER.train(obs, words, *start, 0.0, iters, end_final=True)
    rpi, rA, rB, rrecs = ref[:4]
    # from the checker alone: training helps, and the trained bank finds the words
    assert rrecs[-1][0] - rrecs[0][0] > 5
    first = range(60)
    rdec = [WR.decode(obs[r], rpi, rA, rB, end_final=True) for r in first]
    exact = [words_of(p, s, N) == words[r] for r, (p, s, _, _) in zip(first, rdec)]
    assert np.mean(exact) >= 0.9
    got = gpu_train(obs, words, start, epsilon=0.0, max_iterations=iters, end_final=True, normalise=False)
    compare(got, ref)
    names = [f"w{w}" for w in range(W)]
    models = [HMMTrained(N, W * N, got[1][w], got[2][w], got[0][w], names[w]) for w in range(W)]
    segments, logp = hmm_training_amd.decode_words([obs[r] for r in first], models, end_final=True)
    for r, (p, s, _, margin) in zip(first, rdec):
        if margin > WR.MARGIN:
            assert [name for name, _, _ in segments[r]] == [names[w] for w in words_of(p, s, N)], r


def test_train_connected_round_trip():
    import hmm_training_amd
    from hmm_training_amd.hmm_classes import HMMTrained
    W, N = RECOVERY["W"], RECOVERY["N"]
    obs, words, (pi, A, B) = recovery_case()
    obs, words = obs[:40], words[:40]
    names = ["zero", "one", "two", "three", "four", "five"]
    models = [HMMTrained(N, W * N, A[w], B[w], pi[w], names[w]) for w in range(W)]
    trained, records = hmm_training_amd.train_connected(obs, [[names[w] for w in ws] for ws in words], models,
                                                        epsilon=0.0, max_iterations=4)
    ref = ER.train(obs, words, pi, A, B, 0.0, 4, end_final=True, normalise=True)
    assert [m.word for m in trained] == names and all(m.states == N and m.symbols == W * N for m in trained)
    np.testing.assert_allclose([L for L, _ in records], [L for L, _ in ref[3]], rtol=LL_RTOL)
    for w, m in enumerate(trained):
        ER.close(np.asarray(m.Pi).reshape(-1), ref[0][w], "pi")
        ER.close(m.A, ref[1][w], "A")
        ER.close(m.B, ref[2][w], "B")
    # what comes back goes straight into the decoder
    segments, _ = hmm_training_amd.decode_words(obs[:5], trained)
    assert all(seg and seg[0][1] == 0 and seg[-1][2] == len(o) for seg, o in zip(segments, obs[:5]))
    with pytest.raises(ValueError, match="no model carries"):
        hmm_training_amd.train_connected(obs, [["zero", "six"]] + [["one"]] * 39, models)
    odd = HMMTrained(N + 1, W * N, np.eye(N + 1), np.full((N + 1, W * N), 1.0 / (W * N)), np.eye(N + 1)[0], "odd")
    with pytest.raises(ValueError, match="one shape"):
        hmm_training_amd.train_connected(obs, [["zero"]] * 40, models + [odd])
