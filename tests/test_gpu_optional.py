"""Optional transcript positions on the GPU (hmmbw_align_optional, hmmbw_embedded_train_optional: align.hip and
embedded.hip with OPT) against the NumPy checker of tests/optional_ref.py, with the project's tolerances
(viterbi_ref.RTOL and MARGIN, embedded_ref.PARAM_RTOL, PARAM_ATOL and LL_RTOL).  Paths and bounds are compared
exactly where the checker's margin exceeds MARGIN, after asserting from the checker alone that at least 95 % of the
finite sequences clear it; the seeds were chosen on the CPU so that they do."""
import ctypes

import numpy as np
import pytest

import align_ref as AR
import embedded_ref as ER
import optional_ref as OR
import viterbi_ref as V
import wordnet_ref as WR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: the GPU tests need an MI355X")


def engine(bank, obs):
    from hmm_training_amd.engine import BaumWelchEngine
    e = BaumWelchEngine(bank[0].shape[1], bank[2].shape[2])
    e.set_observations(obs)
    return e


def csr(transcripts, optional=None):
    off = np.zeros(len(transcripts) + 1, dtype=np.int64)
    np.cumsum([len(t) for t in transcripts], out=off[1:])
    ids = np.concatenate([np.asarray(t, dtype=np.int32) for t in transcripts])
    flags = None if optional is None else np.concatenate([np.asarray(f, dtype=np.uint8) for f in optional])
    return off, ids, flags


ptr = lambda x: None if x is None else x.ctypes.data  # noqa: E731


def raw_align(e, bank, transcripts, flags, end_final=False, plain=False):
    """hmmbw_align (plain) or hmmbw_align_optional with the flag bytes given (None: a NULL pointer): (rc, logp, path,
    bounds) as flat arrays."""
    pi, A, B = (np.ascontiguousarray(x, dtype=np.float64) for x in bank)
    off, ids, _ = csr(transcripts)
    logp = np.zeros(len(transcripts))
    path = np.zeros(e.n_symbols_total, dtype=np.int32)
    bounds = np.zeros(len(ids), dtype=np.int32)
    head = (e._ctx, pi.shape[0], ptr(pi), ptr(A), ptr(B), ptr(off), ptr(ids))
    tail = (len(transcripts), 1 if end_final else 0, ptr(logp), ptr(path), len(path), ptr(bounds), len(bounds))
    rc = e._lib.hmmbw_align(*head, *tail) if plain else e._lib.hmmbw_align_optional(*head, ptr(flags), *tail)
    return rc, logp, path, bounds


def raw_train(e, bank, transcripts, flags, plain=False, max_iterations=1, normalise=0):
    pi, A, B = (np.array(x, dtype=np.float64, order="C") for x in bank)
    off, ids, _ = csr(transcripts)
    logp = np.zeros(len(transcripts))
    n = ctypes.c_int64()
    head = (e._ctx, pi.shape[0], ptr(pi), ptr(A), ptr(B), ptr(off), ptr(ids))
    tail = (len(transcripts), 0, 0.0, max_iterations, normalise, None, 0, ctypes.byref(n), ptr(logp))
    rc = (e._lib.hmmbw_embedded_train(*head, *tail) if plain
          else e._lib.hmmbw_embedded_train_optional(*head, ptr(flags), *tail))
    return rc, (pi, A, B), logp, n.value


# every group width and its edge.  longest: an odd length has the optional positions 0, 2, .., L - 1, an even one
# 1, 3, .., L - 1, so together they lie on both sides of lanes 7 / 8, 15 / 16 and 31 / 32, at 0 and at L - 1.  The
# last entry is the seed: one for which, from the checker alone, at least 95 % of the finite sequences clear the
# margin.  N = 1, N = 5 left-to-right and N = 8 dense (the full nibble word) occur
WIDTHS = [(8, 4, 1, 8, "dense", 7000), (8, 5, 5, 16, "left_to_right", 7000), (9, 5, 5, 16, "left_to_right", 7000),
          (9, 4, 8, 16, "dense", 7000), (16, 4, 8, 16, "dense", 7000), (16, 5, 1, 8, "dense", 7000),
          (17, 5, 1, 8, "dense", 7000), (17, 6, 5, 16, "left_to_right", 7000), (32, 6, 5, 16, "left_to_right", 7000),
          (33, 4, 8, 16, "dense", 7000), (33, 5, 1, 8, "dense", 7000), (64, 5, 5, 16, "left_to_right", 7019),
          (64, 6, 1, 8, "dense", 7000)]


def waves_of(obs, spw):
    order = sorted(range(len(obs)), key=lambda r: -len(obs[r]))
    return [order[i:i + spw] for i in range(0, len(order), spw)]


@pytest.mark.parametrize("longest,W,N,K,topology,seed", WIDTHS)
def test_alignment_at_every_group_width(longest, W, N, K, topology, seed):
    obs, transcripts, optional, bank = OR.case(W, N, K, topology, longest, seed)
    R, spw = len(obs), 64 // AR.gw_of(longest)
    assert max(len(t) for t in transcripts) == longest == len(transcripts[0])
    f0 = optional[0]
    assert f0[longest - 1] == 1 and (f0[0] == 1) == (longest % 2 == 1)
    assert [l for l, f in enumerate(f0) if f] == list(range(1 - longest % 2, longest, 2))
    if spw > 1:
        assert R % spw != 0                                           # R is no multiple of the slots per wave
        mixed = [{bool(sum(optional[r])) for r in wave} for wave in waves_of(obs, spw)]
        assert any(len(m) == 2 for m in mixed)                        # a wave with and without optional positions
    mand = [len(t) - sum(f) for t, f in zip(transcripts, optional)]
    T = [len(o) for o in obs]
    assert T[R - 1] == mand[R - 1] and {7, 8, 9, 17} <= {t for t in T} | {m for m in mand[1:5]}
    end_final = (W + longest) % 2 == 1
    with engine(bank, obs) as e:
        paths, bounds, logp = e.align(*bank, transcripts, end_final=end_final, optional=optional)
        none, none2, logp2 = e.align(*bank, transcripts, end_final=end_final, optional=optional, paths=False)
        paths3, bounds3, logp3 = e.align(*bank, transcripts, end_final=end_final, optional=optional)
    assert none is None and none2 is None and logp.tobytes() == logp2.tobytes() == logp3.tobytes()
    assert all(p.tobytes() == q.tobytes() for p, q in zip(paths + bounds, paths3 + bounds3))
    _, rbounds, rlogp, _ = OR.check_align(obs, transcripts, optional, bank, paths, bounds, logp, end_final=end_final)
    assert np.isfinite(rlogp).any()
    if N == 1:                          # one frame per mandatory position: every optional one is passed over
        assert np.array_equal(bounds[R - 1] >= 0, np.asarray(optional[R - 1]) == 0)
    assert any((b[np.asarray(f) == 1] >= 0).any() for b, f in zip(rbounds, optional))    # some are visited
    assert any((b[np.asarray(f) == 1] < 0).any() for b, f in zip(rbounds, optional))     # and some are not


@pytest.mark.parametrize("W,N,K,topology,longest,seed", [(4, 3, 8, "dense", 7, 7100), (5, 5, 16, "left_to_right", 12, 7101),
                                                         (4, 8, 16, "dense", 20, 7102)])
def test_null_and_all_zero_flags_are_the_plain_entry_points(W, N, K, topology, longest, seed):
    obs, transcripts, bank = AR.case(W, N, K, topology, longest, seed)
    zeros = np.zeros(sum(len(t) for t in transcripts), dtype=np.uint8)
    with engine(bank, obs) as e:
        for end_final in (False, True):
            rc, logp, path, bounds = raw_align(e, bank, transcripts, None, end_final, plain=True)
            assert rc == 0
            for flags in (None, zeros):
                rc2, logp2, path2, bounds2 = raw_align(e, bank, transcripts, flags, end_final)
                assert rc2 == 0 and logp2.tobytes() == logp.tobytes()
                assert path2.tobytes() == path.tobytes() and bounds2.tobytes() == bounds.tobytes()
        rc, ref, rlogp, n = raw_train(e, bank, transcripts, None, plain=True)
        assert rc == 0 and n == 1
        for flags in (None, zeros):
            rc2, got, logp2, n2 = raw_train(e, bank, transcripts, flags)
            assert rc2 == 0 and n2 == 1
            np.testing.assert_allclose(logp2, rlogp, rtol=ER.LL_RTOL)
            for x, y, what in zip(got, ref, ("pi", "A", "B")):
                ER.close(x, y, what)


@pytest.mark.parametrize("W,N,K,topology,seed", [(4, 2, 8, "dense", 7200), (5, 4, 12, "left_to_right", 7201)])
def test_max_identity_on_the_device(W, N, K, topology, seed):
    # the optional score is the largest of hmmbw_align's over the expansions, and the winner's bounds are ours
    rng = np.random.default_rng(seed)
    bank = WR.bank(W, N, K, topology, rng)[:3]
    keeps = [[1, 1, 1], [1, 0, 1], [0, 1, 1], [1, 1, 0], [1, 1], [0, 1], [1, 0], [0, 1, 0], [1, 0, 1, 1], [0, 0]]
    transcripts, optional = [], []
    for keep in keeps:
        ws = [int(x) for x in rng.integers(0, W - 1, size=len(keep) - 1)]
        for i in range(1, len(ws)):
            if ws[i] == ws[i - 1]:
                ws[i] = (ws[i] + 1) % (W - 1)
        t, f = OR.with_sil(ws, W - 1, keep)
        transcripts.append(t)
        optional.append(f)
    obs = V.sequences([int(rng.integers(len(t), 4 * len(t) * N)) for t in transcripts], K, rng)
    subs = [OR.expansions(f) for f in optional]
    assert max(len(s) for s in subs) == 8
    with engine(bank, obs) as e:
        _, bounds, logp = e.align(*bank, transcripts, optional=optional)
        exp = []
        for k in range(8):
            picked = [s[k % len(s)] for s in subs]
            _, b, lp = e.align(*bank, [[t[l] for l in s] for t, s in zip(transcripts, picked)])
            exp.append((picked, b, lp))
    best = np.max([x[2] for x in exp], axis=0)
    assert np.isfinite(best).all()
    np.testing.assert_allclose(logp, best, rtol=V.RTOL)
    _, _, _, margin = OR.align_all(obs, transcripts, optional, *bank)
    assert (margin > V.MARGIN).mean() >= 0.95
    for r in np.flatnonzero(margin > V.MARGIN):
        visited = [l for l in range(len(transcripts[r])) if bounds[r][l] >= 0]
        k = next(k for k in range(8) if exp[k][0][r] == visited)
        np.testing.assert_allclose(exp[k][2][r], best[r], rtol=V.RTOL)
        assert np.array_equal(bounds[r][visited], exp[k][1][r]), r


RECOVERY = dict(W=6, N=3, n_seq=60, seed=7300)


def recovery_case():
    W, N = RECOVERY["W"], RECOVERY["N"]
    obs, words, truth = OR.disjoint_case(W, N, RECOVERY["n_seq"], RECOVERY["seed"])
    return obs, words, truth, OR.disjoint_bank(W, N, np.random.default_rng(RECOVERY["seed"] + 1))


def test_exact_recovery_of_the_generating_segmentation():
    obs, words, truth, bank = recovery_case()
    W, N = bank[0].shape
    sil = W - 1
    pairs = [OR.with_sil(ws, sil, [True] * (len(ws) + 1)) for ws in words]
    transcripts, optional = [p[0] for p in pairs], [p[1] for p in pairs]
    present = [sum(1 for w, _, _ in seg if w == sil) for seg in truth]
    assert 0 in present and any(p == len(t) - len(ws) for p, t, ws in zip(present, transcripts, words))
    with engine(bank, obs) as e:
        paths, bounds, logp = e.align(*bank, transcripts, end_final=True, optional=optional)
    assert np.isfinite(logp).all()
    OR.check_align(obs, transcripts, optional, bank, paths, bounds, logp, end_final=True)
    for r, (b, seg, ws) in enumerate(zip(bounds, truth, words)):
        want = np.full(len(b), -1)
        gen = list(seg)
        for l, (w, f) in enumerate(zip(transcripts[r], optional[r])):     # a pause that was not generated stays -1
            if gen and gen[0][0] == w:
                want[l] = gen.pop(0)[1]
            else:
                assert f == 1, r
        assert not gen and np.array_equal(b, want), r


# embedded training: (longest, W, N, K, topology, seed), every group width
TRAIN = [(7, 4, 3, 8, "dense", 7400), (8, 5, 5, 16, "left_to_right", 7401), (15, 4, 8, 16, "dense", 7402),
         (17, 5, 2, 8, "left_to_right", 7403), (33, 5, 1, 8, "dense", 7404), (64, 4, 5, 16, "left_to_right", 7405)]


def close_bank(got, want, what):
    for x, y, name in zip(got, want, ("pi", "A", "B")):
        ER.close(x, y, f"{what} {name}")


@pytest.mark.parametrize("longest,W,N,K,topology,seed", TRAIN)
def test_one_iteration_against_the_checker(longest, W, N, K, topology, seed):
    obs, transcripts, optional, bank = OR.case(W, N, K, topology, longest, seed)
    end_final = seed % 2 == 1
    with engine(bank, obs) as e:
        pi, A, B, records, logp = e.embedded_train(*bank, transcripts, epsilon=0.0, max_iterations=1, normalise=False,
                                                   end_final=end_final, optional=optional)
    rpi, rA, rB, rrec, rlogp, touched = OR.train(obs, transcripts, optional, *bank, max_iterations=1, end_final=end_final)
    assert touched.all() and len(records) == 1
    assert np.array_equal(logp == -np.inf, rlogp == -np.inf) and not np.isnan(logp).any()
    fin = rlogp > -np.inf
    assert fin.any()
    np.testing.assert_allclose(logp[fin], rlogp[fin], rtol=ER.LL_RTOL)
    np.testing.assert_allclose(records[0][0], rrec[0][0], rtol=ER.LL_RTOL)
    close_bank((pi, A, B), (rpi, rA, rB), "one iteration")
    # the silence occurs only at optional positions: its pi is entry / present, a denominator below its instances
    _, _, mand, present = OR.estep(obs, transcripts, optional, *bank, end_final=end_final)
    n_sil = sum(t.count(W - 1) for t in transcripts)
    assert mand[W - 1] == 0 and 0.0 < present[W - 1] < n_sil


def test_three_iterations_and_a_continuation():
    obs, transcripts, optional, bank = OR.case(5, 3, 8, "left_to_right", 9, 7500)
    with engine(bank, obs) as e:
        kw = dict(epsilon=0.0, normalise=False, optional=optional)
        pi3, A3, B3, rec3, logp3 = e.embedded_train(*bank, transcripts, max_iterations=3, **kw)
        pi2, A2, B2, rec2, _ = e.embedded_train(*bank, transcripts, max_iterations=2, **kw)
        pi1, A1, B1, rec1, logp1 = e.embedded_train(pi2, A2, B2, transcripts, max_iterations=1, **kw)
        npi, nA, nB, _, _ = e.embedded_train(*bank, transcripts, epsilon=0.0, max_iterations=3, optional=optional)
    rpi, rA, rB, rrec, rlogp, touched = OR.train(obs, transcripts, optional, *bank, max_iterations=3)
    assert len(rec3) == 3 and len(rec2) == 2 and len(rec1) == 1
    np.testing.assert_allclose([r[0] for r in rec3], [r[0] for r in rrec], rtol=ER.LL_RTOL)
    np.testing.assert_allclose([r[1] for r in rec3[1:]], [r[1] for r in rrec[1:]], rtol=1e-6, atol=1e-9)
    close_bank((pi3, A3, B3), (rpi, rA, rB), "three iterations")
    close_bank((pi1, A1, B1), (rpi, rA, rB), "two and one")
    np.testing.assert_allclose(rec1[0][0], rrec[2][0], rtol=ER.LL_RTOL)
    close_bank((npi, nA, nB), ER.normalised(rpi, rA, rB, touched.astype(int)), "normalised")


def test_an_impossible_optional_word_and_a_short_utterance():
    W, N, K = 4, 3, 9
    rng = np.random.default_rng(7600)
    pi, A, B = WR.bank(W, N, K, "dense", rng)[:3]
    B[:, :, K - 1] = 0.0                     # symbol K - 1 never occurs, and the last word emits nothing else
    B[W - 1] = 0.0
    B[W - 1, :, K - 1] = 0.7                 # not normalised: a normalising return path would show
    pi[W - 1] *= 3.0
    words = [[0, 1], [2], [1, 0, 2], [2, 2, 1], [0], [1, 2]]
    pairs = [OR.with_sil(ws, W - 1, [True] * (len(ws) + 1)) for ws in words]
    transcripts, optional = [p[0] for p in pairs], [p[1] for p in pairs]
    obs = [rng.integers(0, K - 1, size=t) for t in (9, 5, 12, 2, 4, 8)]      # utterance 3: 2 frames for 3 words
    bank = (pi, A, B)
    for normalise in (False, True):
        with engine(bank, obs) as e:
            gpi, gA, gB, rec, logp = e.embedded_train(*bank, transcripts, epsilon=0.0, max_iterations=2,
                                                      normalise=normalise, optional=optional)
        rpi, rA, rB, rrec, rlogp, touched = OR.train(obs, transcripts, optional, *bank, max_iterations=2,
                                                     normalise=normalise)
        assert touched.tolist() == [True, True, True, False]
        assert logp[3] == -np.inf and rlogp[3] == -np.inf and np.isfinite(np.delete(logp, 3)).all()
        np.testing.assert_allclose(np.delete(logp, 3), np.delete(rlogp, 3), rtol=ER.LL_RTOL)
        close_bank((gpi, gA, gB), (rpi, rA, rB), "with a dead word")
        for got, start in zip((gpi, gA, gB), bank):      # bit for bit, whatever normalise says
            assert got[W - 1].tobytes() == start[W - 1].tobytes()
    # the short utterance adds nothing but its mandatory count: the same sums with its observations replaced
    st, _, mand, present = OR.estep(obs, transcripts, optional, *bank)
    obs2 = list(obs)
    obs2[3] = np.array([0])
    st2, _, mand2, present2 = OR.estep(obs2, transcripts, optional, *bank)
    assert np.array_equal(st.xi, st2.xi) and np.array_equal(present, present2) and np.array_equal(mand, mand2)


def test_errors_leave_the_context_as_it_was():
    from hmm_training_amd import _lib
    W, N, K = 3, 4, 8
    rng = np.random.default_rng(7700)
    bank = WR.bank(W, N, K, "dense", rng)[:3]
    obs = V.sequences([6, 3, 9], K, rng)
    transcripts = [[2, 0, 2], [1], [0, 2, 1, 2]]
    good = [[1, 0, 1], [0], [0, 1, 0, 1]]
    flat = lambda f: np.concatenate([np.asarray(x, dtype=np.uint8) for x in f])  # noqa: E731
    mpi, mA, mB = V.model(N, K, "dense", rng)
    with engine(bank, obs) as e:
        rc, logp, path, bounds = raw_align(e, bank, transcripts, flat(good))
        assert rc == 0
        rc, tb, tlogp, n = raw_train(e, bank, transcripts, flat(good))
        assert rc == 0 and n == 1
        for bad in ([[1, 0, 1], [0], [0, 1, 1, 0]],          # adjacent optional positions
                    [[1, 0, 1], [1], [0, 1, 0, 1]],          # a lone optional position
                    [[1, 0, 1], [0], [0, 2, 0, 1]]):         # a flag of 2
            assert raw_align(e, bank, transcripts, flat(bad))[0] == _lib.HMMBW_E_INVALID
            rc, after, _, n = raw_train(e, bank, transcripts, flat(bad))
            assert rc == _lib.HMMBW_E_INVALID and n == 0
            assert all(x.tobytes() == np.ascontiguousarray(y).tobytes() for x, y in zip(after, bank))
        with pytest.raises(ValueError):
            e.align(*bank, transcripts, optional=good[:2])
        with pytest.raises(ValueError):
            e.embedded_train(*bank, transcripts, optional=[[1, 0], [0], [0, 1, 0, 1]])
        e.set_params(mpi, mA, mB)
        e.train(0.0, 2)
        e.reset(0.0, 3)
        e.iterate_begin()
        assert raw_align(e, bank, transcripts, flat(good))[0] == _lib.HMMBW_E_STATE       # an open iteration
        assert raw_train(e, bank, transcripts, flat(good))[0] == _lib.HMMBW_E_STATE
        e.iterate_end()
        rc, logp2, path2, bounds2 = raw_align(e, bank, transcripts, flat(good))
        assert rc == 0 and logp2.tobytes() == logp.tobytes() and path2.tobytes() == path.tobytes()
        assert bounds2.tobytes() == bounds.tobytes()
        rc, tb2, tlogp2, n = raw_train(e, bank, transcripts, flat(good))
        assert rc == 0 and n == 1
        np.testing.assert_allclose(tlogp2, tlogp, rtol=ER.LL_RTOL)
        close_bank(tb2, tb, "after the errors")
    split = lambda x, t: np.split(x, np.cumsum([len(y) for y in t])[:-1])  # noqa: E731
    OR.check_align(obs, transcripts, good, bank, split(path, obs), split(bounds, transcripts), logp, min_clear=0.0)


def test_round_trip_through_the_drop_in_names():
    import hmm_training_amd
    from hmm_training_amd.hmm_classes import HMMTrained
    obs, words, truth, (pi, A, B) = recovery_case()
    W, N = pi.shape
    K = B.shape[2]
    names = ["one", "two", "three", "four", "five", "sil"]
    rng = np.random.default_rng(RECOVERY["seed"] + 2)
    Bp = 0.6 * B + 0.4 * rng.dirichlet(np.full(K, 5.0), size=(W, N))          # a perturbed bank: nothing is certain
    Ap = A.copy()
    for j in range(N):
        Ap[:, j, j] = 0.6
        if j + 1 < N:
            Ap[:, j, j + 1] = 0.4
    models = [HMMTrained(N, K, Ap[w], Bp[w], pi[w], names[w]) for w in range(W)]
    spoken, optional = hmm_training_amd.with_optional([[names[w] for w in ws] for ws in words], "sil")
    trained, records = hmm_training_amd.train_connected(obs, spoken, models, epsilon=0.0, max_iterations=6,
                                                        optional=optional)
    assert len(records) == 6 and records[-1][0] > records[0][0]
    segments, logp = hmm_training_amd.align_words(obs, spoken, trained, optional=optional)
    assert np.isfinite(logp).all()
    for r, (seg, gen) in enumerate(zip(segments, truth)):
        assert seg == [(names[w], s, e) for w, s, e in gen], r
