"""Forced alignment on the GPU (hmmbw_align, hmm_training_amd/csrc/align.hip) against the NumPy checker of
tests/align_ref.py.  Every case checks: 1. logp to rtol 1e-9; 2. every returned labelling is valid (positions
non-decreasing by steps of at most 1, an increase only from a last state, bounds consistent with the path) and
re-scores arc by arc to the returned logp (so it is optimal even where it differs from the checker's); 3. exact
path and bounds equality wherever the checker's margin exceeds 1e-8, after asserting from the checker alone that
at least 95 % of the finite sequences clear it; 4. a scores-only call returns the same logp bit for bit; 5. two
calls return identical bytes."""
import numpy as np
import pytest

import align_ref as AR
import embedded_ref as ER
import viterbi_ref as V
import wordnet_ref as WR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: the GPU tests need an MI355X")


def align(obs, transcripts, bank, end_final=False, dense=False, engine_kw=None):
    from hmm_training_amd.engine import BaumWelchEngine
    pi, A, B = bank
    with BaumWelchEngine(pi.shape[1], B.shape[2], **(engine_kw or {})) as e:
        e.set_observations(obs)
        paths, bounds, logp = e.align(pi, A, B, transcripts, end_final=end_final, dense=dense)
        none, none2, logp2 = e.align(pi, A, B, transcripts, end_final=end_final, dense=dense, paths=False)
        paths3, bounds3, logp3 = e.align(pi, A, B, transcripts, end_final=end_final, dense=dense)
    assert none is None and none2 is None
    assert logp.tobytes() == logp2.tobytes()                                                     # 4
    assert logp.tobytes() == logp3.tobytes()                                                     # 5
    assert all(p.tobytes() == q.tobytes() for p, q in zip(paths, paths3))
    assert all(b.tobytes() == q.tobytes() for b, q in zip(bounds, bounds3))
    return paths, bounds, logp


def run(obs, transcripts, bank, end_final=False, min_clear=0.95, **kw):
    paths, bounds, logp = align(obs, transcripts, bank, end_final=end_final, **kw)
    ref = AR.check_align(obs, transcripts, bank, paths, bounds, logp, end_final=end_final, min_clear=min_clear)  # 1, 2, 3
    return (paths, bounds, logp), ref


def has_repeat(transcripts):
    return any(a == b for ws in transcripts for a, b in zip(ws, ws[1:]))


# every group width, each also just above its power of two; every N from 1 to 8; both scans.  The last entry is the
# seed: one for which, from the checker alone, at least 95 % of the finite sequences clear the margin (two instances
# of the same word in a row leave the frame of the hand-over open whenever the path sits in the word's last state
# on both sides of it, so not every draw does)
WIDTHS = [(1, 3, 3, 8, "left_to_right", 9000), (3, 5, 2, 16, "dense", 9011), (8, 10, 5, 32, "left_to_right", 9001),
          (8, 3, 8, 16, "dense", 9005), (9, 4, 8, 16, "left_to_right", 9001), (16, 8, 1, 8, "dense", 9000),
          (17, 17, 3, 16, "left_to_right", 9000), (33, 6, 5, 32, "dense", 9004), (64, 9, 8, 64, "left_to_right", 9000),
          (64, 5, 2, 8, "dense", 9000), (3, 4, 6, 16, "dense", 9003), (9, 5, 7, 16, "left_to_right", 9003),
          (2, 3, 4, 8, "left_to_right", 9002)]


def waves_of(obs, spw):
    """The sequences of every decoding wave: the layout sorts by length, longest first, and a wave holds spw slots."""
    order = sorted(range(len(obs)), key=lambda r: -len(obs[r]))
    return [order[i:i + spw] for i in range(0, len(order), spw)]


@pytest.mark.parametrize("longest,W,N,K,topology,seed", WIDTHS)
def test_group_widths_and_both_scans(longest, W, N, K, topology, seed):
    obs, transcripts, bank = AR.case(W, N, K, topology, longest, seed)
    R, spw = len(obs), 64 // AR.gw_of(longest)
    assert max(len(t) for t in transcripts) == longest
    if spw > 1:
        assert R % spw != 0                                                  # R is no multiple of the slots per wave
    if longest >= 2 and N > 1:
        assert has_repeat(transcripts)                                       # immediate repeats of a word occur
    if longest >= 3 and spw > 1:                                             # unequal transcripts in one wave
        assert any(len({len(transcripts[r]) for r in wave}) > 1 for wave in waves_of(obs, spw))
    (_, _, logp), _ = run(obs, transcripts, bank, end_final=(W + longest) % 2 == 1)
    assert np.isfinite(logp).all()                                           # T >= L and every pi is positive


CHUNK_BANKS = [(3, 3, 8, "left_to_right", 3), (10, 5, 32, "left_to_right", 9), (17, 8, 64, "dense", 17), (5, 4, 16, "dense", 5)]
CHUNK_SEEDS = {1: (9500, 9500, 9501, 9501), 7: (9500, 9527, 9500, 9503), 8: (9500, 9504, 9500, 9501),
               9: (9500, 9502, 9502, 9501), 17: (9500, 9514, 9501, 9501)}   # chosen as those of WIDTHS


@pytest.mark.parametrize("tmin", [1, 7, 8, 9, 17])
@pytest.mark.parametrize("bank_no", range(len(CHUNK_BANKS)))
def test_lengths_around_the_chunk(tmin, bank_no):
    # the eight-step chunk boundary, R that is no multiple of the slots per wave, padding slots
    W, N, K, topology, longest = CHUNK_BANKS[bank_no]
    rng = np.random.default_rng(CHUNK_SEEDS[tmin][bank_no])
    pi, A, B, _, _ = WR.bank(W, N, K, topology, rng)
    T = V.ragged_lengths(N, tmin, rng)
    obs = V.sequences(T, K, rng)
    transcripts = ER.transcripts_for(W, [int(rng.integers(1, min(int(t), longest) + 1)) for t in T], rng)
    run(obs, transcripts, (pi, A, B), end_final=(tmin % 2 == 1))


def test_feasibility_edge():
    W, N, K = 4, 3, 8
    rng = np.random.default_rng(9600)
    dense = WR.bank(W, N, K, "dense", rng)[:3]
    lr = WR.bank(W, N, K, "left_to_right", rng)[:3]
    lr[0][:] = 0.0
    lr[0][:, 0] = 1.0                       # entered at state 0: an instance takes N frames at least
    transcripts = [[0, 1], [2, 2, 3], [1], [3, 0, 1, 2], [0, 0, 1], [2], [1, 3], [0, 1, 2, 3, 0], [3, 3], [2, 1, 0]]
    #              ok      T == L      ok   T < L         T == L     T=1  ok      T < L            ok      ok
    obs = V.sequences([9, 3, 5, 3, 3, 1, 14, 4, 7, 11], K, rng)
    short, exact = [3, 7], [1, 4, 5]
    for end_final in (False, True):
        (paths, bounds, logp), _ = run(obs, transcripts, dense, end_final=end_final)
        assert np.all(logp[short] == -np.inf) and np.isfinite(np.delete(logp, short)).all()
        for r in short:
            assert np.all(paths[r] == -1) and np.all(bounds[r] == -1)
        for r in exact:                     # one frame per instance: every bound is l
            assert bounds[r].tolist() == list(range(len(transcripts[r])))
            assert np.all(paths[r] // N == np.arange(len(transcripts[r])))
        (paths, bounds, logp), (_, _, rlogp, _) = run(obs, transcripts, lr, end_final=end_final)
        dead = short + [1, 4]               # T == L with L > 1 cannot pass through N > 1 states per word
        if end_final:
            dead = dead + [5]               # T = 1 ends in state 0
        assert np.all(logp[dead] == -np.inf)
        assert np.array_equal(logp == -np.inf, rlogp == -np.inf) and np.isfinite(logp[[0, 6]]).all()
    # a symbol that every state of one needed word forbids
    pi, A, B = (x.copy() for x in dense)
    B[1, :, 5] = 0.0
    obs2 = [o.copy() for o in obs]
    for o in obs2:
        o[o == 5] = 4
    obs2[0][:] = 5                          # transcript [0, 1] needs word 1 for one frame at least
    obs2[2][2] = 5                          # transcript [1]
    (paths, bounds, logp), _ = run(obs2, transcripts, (pi, A, B))
    assert logp[0] == -np.inf and logp[2] == -np.inf and np.isfinite(logp[[6, 8, 9]]).all()
    assert not np.any(np.isnan(logp))


@pytest.mark.parametrize("W,N,K", [(64, 8, 256), (5, 8, 256), (5, 8, 300)])
def test_table_placement_and_pack_forms(W, N, K):
    # (64, 8, 256): the 1 MB emission table stays in global memory.  N = 8, K = 256: the E-step's tables live in LDS
    # and the packs hold scaled row offsets; K = 300: symbol ids
    rng = np.random.default_rng(9700 + W + K)
    bank = WR.bank(W, N, K, "left_to_right", rng)[:3]
    lens = [3, 1, 2, 3, 1, 2, 2, 3, 1, 2, 3]
    transcripts = ER.transcripts_for(W, lens, rng)
    obs = V.sequences([int(rng.integers(L, 3 * L * N)) for L in lens], K, rng)
    run(obs, transcripts, bank)


@pytest.mark.parametrize("N,K,topology", [(4, 16, "dense"), (5, 32, "left_to_right")])
def test_one_word_transcripts_are_hmmbw_viterbi(N, K, topology):
    from hmm_training_amd.engine import BaumWelchEngine
    W = 3
    rng = np.random.default_rng(9800 + N)
    bank = WR.bank(W, N, K, topology, rng)[:3]
    obs = V.sequences(V.ragged_lengths(N, 9, rng), K, rng)
    for w in range(W):
        transcripts = [[w]] * len(obs)
        (paths, bounds, logp), _ = run(obs, transcripts, bank)
        assert all(b.tolist() == [0] for b in bounds)
        with BaumWelchEngine(N, K) as e:
            e.set_observations(obs)
            e.set_params(bank[0][w], bank[1][w], bank[2][w])
            vpaths, vlogp = e.viterbi()
        np.testing.assert_allclose(logp, vlogp, rtol=1e-12)
        _, _, margin = V.decode_all(obs, bank[0][w], bank[1][w], bank[2][w])
        assert (margin > V.MARGIN).mean() >= 0.95
        for r in np.flatnonzero(margin > V.MARGIN):
            assert np.array_equal(paths[r], vpaths[r]), r


def recovery_data():
    """The recovery data of the loop decoder's tests (WR.word_sequences, WR.recovery_bank) with the generating
    segmentation: the generator is replayed draw by draw and must give the same observations."""
    import test_gpu_wordnet as TW
    obs, words, bank = TW.recovery_case()
    W, N, n_seq, seed = (TW.RECOVERY[k] for k in ("W", "N", "n_seq", "seed"))
    rng = np.random.default_rng(seed)
    K = W * N
    truth = []
    for r in range(n_seq):
        n = int(rng.integers(1, 5 + 1))
        ws = [int(x) for x in rng.integers(0, W, size=n)]
        if n >= 2 and r % 2 == 0:
            ws[1] = ws[0]
        o, starts = [], []
        for w in ws:
            starts.append(len(o))
            for j in range(N):
                for _ in range(int(rng.integers(1, 5))):
                    k = w * N + j
                    if rng.random() >= 0.9:
                        k = int((k + rng.integers(1, K)) % K)
                    o.append(k)
        assert ws == words[r] and np.array_equal(o, obs[r])
        truth.append(np.array(starts))
    return obs, words, bank, truth


@pytest.mark.parametrize("end_final", [True, False])
def test_agreement_with_the_loop_decoder(end_final):
    from hmm_training_amd.engine import BaumWelchEngine
    obs, _, bank, _ = recovery_data()
    pi, A, B = bank
    W, N = pi.shape
    with BaumWelchEngine(N, B.shape[2]) as e:
        e.set_observations(obs)
        lpaths, lstarts, llogp = e.wordnet_decode(pi, A, B, None, None, end_final=end_final)
        found = [[int(p[t]) // N for t in np.flatnonzero(s)] for p, s in zip(lpaths, lstarts)]
        assert np.isfinite(llogp).all() and max(len(ws) for ws in found) > 1
        paths, bounds, logp = e.align(pi, A, B, found, end_final=end_final)
    np.testing.assert_allclose(logp, llogp, rtol=1e-12)
    _, _, _, lmargin = WR.decode_all(obs, pi, A, B, None, None, end_final)
    _, _, _, margin = AR.check_align(obs, found, bank, paths, bounds, logp, end_final=end_final)
    clear = (lmargin > V.MARGIN) & (margin > V.MARGIN)
    assert clear.mean() >= 0.95
    for r in np.flatnonzero(clear):
        ws = np.asarray(found[r])
        assert np.array_equal(ws[paths[r] // N] * N + paths[r] % N, lpaths[r]), r
        assert np.array_equal(bounds[r], np.flatnonzero(lstarts[r])), r


def test_recovery_of_the_generating_segmentation():
    obs, words, bank, truth = recovery_data()
    assert has_repeat(words)
    rpaths, rbounds, rlogp, margin = AR.align_all(obs, words, *bank, True)
    assert np.isfinite(rlogp).all()
    dev = np.concatenate([np.abs(b - t) for b, t in zip(rbounds, truth)])
    tol = int(dev.max())                      # what the checker itself achieves: not fixed beforehand
    assert tol < min(len(o) for o in obs) and np.median(dev) == 0
    paths, bounds, logp = align(obs, words, bank, end_final=True)
    AR.check_align(obs, words, bank, paths, bounds, logp, end_final=True)
    for r, (b, t) in enumerate(zip(bounds, truth)):
        assert np.all(np.abs(b - t) <= tol), r
        if margin[r] > V.MARGIN:
            assert np.array_equal(b, rbounds[r]), r


@pytest.mark.parametrize("W,N,K,longest,seed", [(3, 3, 8, 2, 9900), (10, 5, 32, 9, 9902), (8, 8, 16, 17, 9900)])
def test_dense_flag_on_a_left_to_right_bank(W, N, K, longest, seed):
    obs, transcripts, bank = AR.case(W, N, K, "left_to_right", longest, seed)
    for end_final in (False, True):
        (paths, bounds, logp), _ = run(obs, transcripts, bank, end_final=end_final)
        (dpaths, dbounds, dlogp), (_, _, _, margin) = run(obs, transcripts, bank, end_final=end_final, dense=True)
        np.testing.assert_allclose(dlogp, logp, rtol=V.RTOL)
        for r in np.flatnonzero(margin > V.MARGIN):
            assert np.array_equal(paths[r], dpaths[r]) and np.array_equal(bounds[r], dbounds[r]), r


@pytest.mark.parametrize("deterministic", [True, False])
def test_align_does_not_disturb_training(deterministic):
    from hmm_training_amd.engine import BaumWelchEngine
    N, K, W = 8, 32, 5
    rng = np.random.default_rng(9951)
    pi, A, B = V.model(N, K, "left_to_right", rng)
    T = V.ragged_lengths(N, 17, rng)
    obs = V.sequences(T, K, rng)
    bank = WR.bank(W, N, K, "left_to_right", rng)[:3]
    transcripts = ER.transcripts_for(W, [int(rng.integers(1, 4)) for _ in T], rng)

    def go(with_align):
        trace = []
        with BaumWelchEngine(N, K, topology="left_to_right", deterministic=deterministic) as e:
            e.set_observations(obs)
            e.set_params(pi, A, B)
            e.train(0.0, 2, lambda k, L, d: trace.append(L))
            ll = e.loglik()
            if with_align:
                before = (ll.tobytes(), [x.tobytes() for x in e.params(normalise=False)], bytes(e.status()[0]))
                paths, bounds, logp = e.align(*bank, transcripts)
                after = (e.loglik().tobytes(), [x.tobytes() for x in e.params(normalise=False)], bytes(e.status()[0]))
                assert after == before      # log-likelihoods, parameters and training status: bit for bit
                AR.check_align(obs, transcripts, bank, paths, bounds, logp)
            e.train(0.0, 2, lambda k, L, d: trace.append(L))
            return e.params(normalise=False), np.array(trace), ll

    (p1, t1, l1), (p0, t0, l0) = go(True), go(False)
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
    rng = np.random.default_rng(9960)
    pi, A, B, _, _ = WR.bank(W, N, K, "dense", rng)
    obs = V.sequences([5, 3, 9], K, rng)
    off = np.array([0, 2, 3, 5], dtype=np.int64)
    ids = np.array([0, 1, 2, 2, 0], dtype=np.int32)
    logp = np.zeros(3)
    path = np.zeros(17, dtype=np.int32)
    bounds = np.zeros(5, dtype=np.int32)
    ptr = lambda x: None if x is None else x.ctypes.data  # noqa: E731

    def call(e, n_words=W, bank=(pi, A, B), off_=off, ids_=ids, n=3, flags=0, lp=logp, path_=path, n_path=17,
             bounds_=bounds, n_bounds=5):
        p, a, b = bank
        return e._lib.hmmbw_align(e._ctx, n_words, ptr(p), ptr(a), ptr(b), ptr(off_), ptr(ids_), n, flags, ptr(lp),
                                  ptr(path_), n_path, ptr(bounds_), n_bounds)

    def spoiled(x, value):
        y = x.copy()
        y.reshape(-1)[3] = value
        return y

    mpi, mA, mB = V.model(N, K, "dense", rng)
    with BaumWelchEngine(N, K) as e:
        assert call(e) == _lib.HMMBW_E_STATE                                           # no observations
        e.set_observations(obs)
        assert call(e, n_words=0) == _lib.HMMBW_E_INVALID                              # n_words < 1
        for bank in ((None, A, B), (pi, None, B), (pi, A, None)):
            assert call(e, bank=bank) == _lib.HMMBW_E_INVALID                          # a NULL bank pointer
        assert call(e, off_=None) == _lib.HMMBW_E_INVALID and call(e, ids_=None) == _lib.HMMBW_E_INVALID
        assert call(e, lp=None) == _lib.HMMBW_E_INVALID                                # a NULL logp_out
        assert call(e, path_=None) == _lib.HMMBW_E_INVALID                             # bounds_out without path_out
        assert call(e, n=2) == _lib.HMMBW_E_INVALID                                    # not the loaded count
        assert call(e, n_path=16) == _lib.HMMBW_E_INVALID                              # a wrong path_len
        assert call(e, path_=None, bounds_=None, n_path=16) == _lib.HMMBW_E_INVALID    # ... also without paths
        assert call(e, n_bounds=4) == _lib.HMMBW_E_INVALID                             # a wrong bounds_len
        assert call(e, path_=None, bounds_=None, n_bounds=6) == _lib.HMMBW_E_INVALID   # ... also without bounds
        assert call(e, off_=np.array([0, 2, 2, 5], dtype=np.int64)) == _lib.HMMBW_E_INVALID   # an empty transcript
        assert call(e, ids_=np.array([0, 1, 3, 2, 0], dtype=np.int32)) == _lib.HMMBW_E_INVALID   # a word id = W
        assert call(e, ids_=np.array([0, -1, 2, 2, 0], dtype=np.int32)) == _lib.HMMBW_E_INVALID
        assert call(e, off_=np.array([1, 2, 3, 5], dtype=np.int64)) == _lib.HMMBW_E_INVALID      # bad offsets
        assert call(e, off_=np.array([0, 3, 2, 5], dtype=np.int64)) == _lib.HMMBW_E_INVALID
        for bad in (-0.1, np.inf, np.nan):
            assert call(e, bank=(spoiled(pi, bad), A, B)) == _lib.HMMBW_E_INVALID
            assert call(e, bank=(pi, spoiled(A, bad), B)) == _lib.HMMBW_E_INVALID
            assert call(e, bank=(pi, A, spoiled(B, bad))) == _lib.HMMBW_E_INVALID
        assert call(e, flags=4) == _lib.HMMBW_E_INVALID                                # an unknown flag bit
        big = WR.bank(65, N, K, "dense", rng)[:3]
        assert call(e, n_words=65, bank=big) == _lib.HMMBW_E_UNSUPPORTED               # more than 64 words
        long_off = np.array([0, 65, 66, 67], dtype=np.int64)
        assert call(e, off_=long_off, ids_=np.zeros(67, dtype=np.int32), bounds_=np.zeros(67, dtype=np.int32),
                    n_bounds=67) == _lib.HMMBW_E_UNSUPPORTED                           # a 65-word transcript
        with pytest.raises(ValueError):
            e.align(pi, A, B, [[0, 1], [], [2, 0]])
        with pytest.raises(ValueError):
            e.align(pi, A, B, [[0, 1], [2]])
        # the context still works afterwards, without parameters of its own
        transcripts = [[0, 1], [2], [2, 0]]
        assert call(e) == _lib.HMMBW_OK
        assert call(e, bounds_=None) == _lib.HMMBW_OK                                  # paths without bounds
        assert call(e, path_=None, bounds_=None) == _lib.HMMBW_OK                      # scores only
        paths, bnds, lp = e.align(pi, A, B, transcripts)
        assert np.array_equal(np.concatenate(paths), path) and np.array_equal(np.concatenate(bnds), bounds)
        assert np.array_equal(lp, logp)
        AR.check_align(obs, transcripts, (pi, A, B), paths, bnds, lp, min_clear=0.0)
        # an open iteration
        e.set_params(mpi, mA, mB)
        e.train(0.0, 2)
        e.reset(0.0, 3)
        e.iterate_begin()
        assert call(e) == _lib.HMMBW_E_STATE
        e.iterate_end()
        assert call(e) == _lib.HMMBW_OK
    with BaumWelchEngine(9, K) as e:                                                   # a context with N = 9
        e.set_observations(obs)
        nine = WR.bank(2, 9, K, "dense", rng)[:3]
        assert call(e, n_words=2, bank=nine, ids_=np.array([0, 1, 1, 1, 0], dtype=np.int32)) == _lib.HMMBW_E_UNSUPPORTED
        pi9, A9, B9 = V.model(9, K, "dense", rng)
        e.set_params(pi9, A9, B9)
        p9, l9 = e.viterbi()                                                           # the context still works
        V.check_decode(obs, pi9, A9, B9, p9, l9, "dense", min_clear=0.0)


def test_empty_observations_write_nothing():
    from hmm_training_amd.engine import BaumWelchEngine
    bank = WR.bank(3, 4, 8, "dense", np.random.default_rng(1))[:3]
    with BaumWelchEngine(4, 8) as e:
        e.set_observations([])
        paths, bounds, lp = e.align(*bank, [])
        assert paths == [] and bounds == [] and lp.shape == (0,)
        assert e.align(*bank, [], paths=False)[2].shape == (0,)


def test_multi_rank_context_aligns_its_shard():
    from hmm_training_amd.engine import shard_bounds
    W, N, K = 9, 2, 16
    rng = np.random.default_rng(9997)
    bank = WR.bank(W, N, K, "dense", rng)[:3]
    T = V.ragged_lengths(N, 8, rng)
    obs = V.sequences(T, K, rng)
    transcripts = ER.transcripts_for(W, [int(rng.integers(1, 4)) for _ in T], rng)
    lo, hi = shard_bounds([len(o) for o in obs], 2)[1]
    run(obs[lo:hi], transcripts[lo:hi], bank, engine_kw=dict(rank=1, world_size=2, native_comm=False))


def test_group_width_changes_between_calls():
    # one context, transcripts of up to 3, then 20, then 3 words: the back-pointer rows are planned again per width
    from hmm_training_amd.engine import BaumWelchEngine
    W, N, K = 6, 3, 8
    rng = np.random.default_rng(9980)
    bank = WR.bank(W, N, K, "left_to_right", rng)[:3]
    T = V.ragged_lengths(N, 20, rng)
    obs = V.sequences(T, K, rng)
    short = ER.transcripts_for(W, [int(rng.integers(1, 4)) for _ in T], rng)
    long_ = ER.transcripts_for(W, [20] + [int(rng.integers(1, 21)) for _ in T[1:]], rng)
    with BaumWelchEngine(N, K) as e:
        e.set_observations(obs)
        for transcripts in (short, long_, short):
            paths, bounds, logp = e.align(*bank, transcripts)
            AR.check_align(obs, transcripts, bank, paths, bounds, logp)


def test_align_words_end_to_end():
    import hmm_training_amd
    from hmm_training_amd.hmm_classes import HMMTrained
    obs, words, (pi, A, B), truth = recovery_data()
    W, N = pi.shape
    names = ["forward", "back", "left", "right", "stop", "go", "up", "down", "faster", "slower"]
    models = [HMMTrained(N, W * N, A[w], B[w], pi[w], names[w]) for w in range(W)]
    obs, words = list(obs[:20]), [list(ws) for ws in words[:20]]
    obs.append(obs[0][:3])
    words.append([0, 1, 2, 3])               # four left-to-right words in three frames: no path
    segments, logp = hmm_training_amd.align_words(obs, [[names[w] for w in ws] for ws in words], models)
    assert logp.shape == (21,) and np.isfinite(logp[:20]).all() and logp[20] == -np.inf and segments[20] == []
    for r, seg in enumerate(segments[:20]):
        assert [name for name, _, _ in seg] == [names[w] for w in words[r]], r      # one per position, in order
        assert seg[0][1] == 0 and seg[-1][2] == len(obs[r])
        assert all(a[2] == b[1] for a, b in zip(seg, seg[1:]))                     # the segments tile [0, T)
        assert all(e - s >= N for _, s, e in seg)                                  # a left-to-right word takes N frames


def test_align_words_after_train_connected():
    import hmm_training_amd
    from hmm_training_amd.hmm_classes import HMMTrained
    W, N = 3, 3
    rng = np.random.default_rng(2)
    obs, words = WR.word_sequences(W, N, 30, rng, max_words=3)
    pi, A, B = ER.flat_start(W, N, W * N, rng)
    names = ["one", "two", "three"]
    models = [HMMTrained(N, W * N, A[w], B[w], pi[w], names[w]) for w in range(W)]
    spoken = [[names[w] for w in ws] for ws in words]
    trained, _ = hmm_training_amd.train_connected(obs, spoken, models, epsilon=0.0, max_iterations=5)
    segments, logp = hmm_training_amd.align_words(obs, spoken, trained)
    assert np.isfinite(logp).all()
    for seg, ws, o in zip(segments, spoken, obs):
        assert [name for name, _, _ in seg] == ws and seg[0][1] == 0 and seg[-1][2] == len(o)
        assert all(a[2] == b[1] for a, b in zip(seg, seg[1:]))
