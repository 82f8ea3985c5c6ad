"""Optional transcript positions without a GPU: the NumPy checker of the GPU tests (tests/optional_ref.py) against
the existing checkers by the expansion identities (every complete path visits a definite subset of the optional
positions, so log P is the LSE and the Viterbi score the maximum over the 2^k plain transcripts); hand cases; the
transcript check and the plan of the new quantities through a stand-alone probe built with the address and
undefined-behaviour sanitizers; the two entry points in the header, the binding table and the built library; and
the Python layers' argument checks and with_optional."""
import os
import re
import subprocess

import numpy as np
import pytest

import align_ref as AR
import embedded_ref as ER
import optional_ref as OR
import wordnet_ref as WR
from conftest import ROOT
from test_lds_layout import _host_compiler


# --------------------------------------------------------------------------------------------------------------
# the checker against the existing checkers
# --------------------------------------------------------------------------------------------------------------
def sil_transcript(W, n, keep, rng):
    ws = [int(x) for x in rng.integers(0, W - 1, size=n)]
    return OR.with_sil(ws, W - 1, keep)


IDENTITY = [(3, 1, 8, "dense"), (3, 2, 6, "left_to_right"), (4, 3, 8, "dense"), (4, 5, 12, "left_to_right"),
            (4, 8, 16, "dense")]


@pytest.mark.parametrize("end_final", [False, True])
@pytest.mark.parametrize("W,N,K,topology", IDENTITY)
def test_expansion_identities(W, N, K, topology, end_final):
    rng = np.random.default_rng(500 + W * N + K)
    pi, A, B, _, _ = WR.bank(W, N, K, topology, rng)
    seen_skip = seen_dead = 0
    for n, keep in ((1, [1, 1]), (2, [1, 1, 1]), (2, [0, 1, 1]), (2, [1, 0, 1]), (2, [1, 1, 0]), (3, [0, 1, 0, 1]),
                    (1, [0, 1]), (1, [1, 0]), (3, [0, 0, 0, 0])):
        words, opt = sil_transcript(W, n, keep, rng)
        assert sum(opt) <= 3
        mand = len(words) - sum(opt)
        for T in (mand - 1, mand, mand + 1, len(words) * N + 3):
            if T < 1:
                continue
            obs = rng.integers(0, K, size=T)
            subs = OR.expansions(opt)
            assert len(subs) == 2 ** sum(opt)
            # the sums: log P is the LSE of the expansions' log P
            logp = OR.forward_backward(obs, words, opt, pi, A, B, end_final)[0]
            parts = [ER.forward_backward(obs, [words[l] for l in s], pi, A, B, end_final)[0] for s in subs]
            want = ER.lse(parts)
            if want == -np.inf:
                seen_dead += 1
                assert logp == -np.inf                              # T below the mandatory count, or too few frames
                assert T < mand or topology == "left_to_right"      # for the states of a left-to-right chain
            else:
                np.testing.assert_allclose(logp, want, rtol=1e-12)
            # the maxima: the Viterbi score is the largest of the expansions', and the winner's labelling is ours
            path, bounds, vlogp, margin = OR.align(obs, words, opt, pi, A, B, end_final)
            exp = [AR.align(obs, [words[l] for l in s], pi, A, B, end_final) for s in subs]
            best = max(e[2] for e in exp)
            assert vlogp == best                                   # the same additions in the same order
            if best == -np.inf:
                assert np.all(path == -1) and np.all(bounds == -1) and margin == np.inf
                continue
            np.testing.assert_allclose(OR.path_logp(path, obs, words, opt, pi, A, B), vlogp, rtol=1e-13)
            if margin > 1e-9:
                visited = [l for l in range(len(words)) if bounds[l] >= 0]
                k = subs.index(visited)
                assert exp[k][2] == best
                assert np.array_equal(bounds[visited], exp[k][1])
                assert np.array_equal(path % N, exp[k][0] % N)
                assert np.array_equal(np.asarray(visited)[exp[k][0] // N], path // N)
                seen_skip += len(visited) < len(words)
    assert seen_skip > 0 and seen_dead > 0


def test_no_optional_position_is_the_plain_checker():
    rng = np.random.default_rng(77)
    W, N, K = 4, 3, 8
    pi, A, B, _, _ = WR.bank(W, N, K, "dense", rng)
    for L, T in ((1, 1), (2, 7), (5, 19)):
        words = ER.transcripts_for(W, [L], rng)[0]
        obs = rng.integers(0, K, size=T)
        for end_final in (False, True):
            p, b, lp, m = OR.align(obs, words, [0] * L, pi, A, B, end_final)
            rp, rb, rlp, rm = AR.align(obs, words, pi, A, B, end_final)
            assert lp == rlp and np.array_equal(p, rp) and np.array_equal(b, rb)
            np.testing.assert_allclose(m, rm, rtol=1e-9, atol=1e-13)
    obs = [rng.integers(0, K, size=t) for t in (9, 4, 12)]
    transcripts = [[0, 1], [2], [3, 3, 0]]
    st, logp, mand, present = OR.estep(obs, transcripts, [[0] * len(t) for t in transcripts], pi, A, B)
    rst, rlogp = ER.estep(obs, transcripts, pi, A, B)
    assert np.array_equal(mand, rst.count) and not present.any()
    np.testing.assert_allclose(logp, rlogp, rtol=1e-13)
    for x, y in ((st.entry, rst.entry), (st.xi, rst.xi), (st.g_all, rst.g_all), (st.b_num, rst.b_num)):
        np.testing.assert_allclose(x, y, rtol=1e-12, atol=1e-300)


def test_statistics_are_the_expansions_posterior_mixture():
    # the pooled sums of the optional chain are the expansions' sums weighted by their posterior P_e / P
    rng = np.random.default_rng(78)
    W, N, K = 3, 2, 5
    pi, A, B, _, _ = WR.bank(W, N, K, "dense", rng)
    words, opt = [2, 0, 2, 1, 2], [1, 0, 1, 0, 1]
    obs = rng.integers(0, K, size=11)
    st, logp, mand, present = OR.estep([obs], [words], [opt], pi, A, B)
    mix = ER.Stats(W, N, K)
    vis = 0.0
    for s in OR.expansions(opt):
        sub = [words[l] for l in s]
        est, elp = ER.estep([obs], [sub], pi, A, B)
        wgt = np.exp(elp[0] - logp[0])
        for name in ("entry", "xi", "g_all", "b_num"):
            setattr(mix, name, getattr(mix, name) + wgt * getattr(est, name))
        vis += wgt * (len(s) - 2)                                       # the optional instances it visits
    for name in ("entry", "xi", "g_all", "b_num"):
        np.testing.assert_allclose(getattr(st, name), getattr(mix, name), rtol=1e-10, atol=1e-300)
    assert mand.tolist() == [1, 1, 0]
    np.testing.assert_allclose(present, [0.0, 0.0, vis], rtol=1e-10)
    np.testing.assert_allclose(st.entry.sum(axis=1), mand + present, rtol=1e-10)   # 1 per visited instance


def test_hand_cases():
    W, N, K = 2, 1, 2          # word 0 = a emits symbol 0, word 1 = sil emits symbol 1; one state each
    pi, A = np.ones((W, N)), np.full((W, N, N), 0.5)
    B = np.array([[[0.9, 0.1]], [[0.2, 0.8]]])
    words, opt = [1, 0, 1], [1, 0, 1]
    # sil? a sil? at T = 1: only a
    path, bounds, logp, margin = OR.align([0], words, opt, pi, A, B)
    assert path.tolist() == [1] and bounds.tolist() == [-1, 0, -1] and margin == np.inf
    np.testing.assert_allclose(logp, np.log(0.9), rtol=1e-15)
    np.testing.assert_allclose(OR.forward_backward([0], words, opt, pi, A, B)[0], np.log(0.9), rtol=1e-15)
    # T = 2, [sil, a]: the pause before is taken, the one after is not
    path, bounds, logp, _ = OR.align([1, 0], words, opt, pi, A, B)
    assert path.tolist() == [0, 1] and bounds.tolist() == [0, 1, -1]
    np.testing.assert_allclose(logp, np.log(0.8) + np.log(0.9), rtol=1e-15)
    # a b with sil? between, at T = mandatory count: every optional position is passed over
    pi3, A3 = np.ones((3, 1)), np.full((3, 1, 1), 0.5)
    B3 = np.array([[[0.8, 0.1, 0.1]], [[0.1, 0.8, 0.1]], [[0.1, 0.1, 0.8]]])
    words, opt = [2, 0, 2, 1, 2], [1, 0, 1, 0, 1]
    path, bounds, logp, _ = OR.align([0, 1], words, opt, pi3, A3, B3)
    assert path.tolist() == [1, 3] and bounds.tolist() == [-1, 0, -1, 1, -1]
    np.testing.assert_allclose(logp, 2 * np.log(0.8), rtol=1e-15)
    # ... and one frame below it there is no path
    path, bounds, logp, margin = OR.align([0], words, opt, pi3, A3, B3)
    assert logp == -np.inf and np.all(path == -1) and np.all(bounds == -1) and margin == np.inf
    assert OR.forward_backward([0], words, opt, pi3, A3, B3)[0] == -np.inf
    # ties, decided arc by arc as the back-trace meets them.  All emissions equal, stay = entry weight: every path
    # scores the same.  The end in L-1 beats L-2; the within-word arc beats an entry, so a position is entered at
    # the first frame it can be reached (position l at frame l - 1 here, with position 1 a start); and the entry
    # from l-1 beats the one from l-2 wherever l-1 is alive: position 2 is not at frame 0, so 3 is entered from 1
    flat = np.full((3, 1, 3), 1 / 3)
    pi1, A1 = np.ones((3, 1)), np.ones((3, 1, 1))
    path, bounds, logp, margin = OR.align([0, 1, 2, 0, 1], words, opt, pi1, A1, flat)
    assert margin == 0.0 and path.tolist() == [1, 3, 4, 4, 4] and bounds.tolist() == [-1, 0, -1, 1, 2]
    A1b = A1.copy()
    A1b[1, 0, 0] = 0.0                         # word 1 cannot stay: the last position is entered at the last frame,
    path, bounds, logp, margin = OR.align([0, 1, 2], [0, 2, 1], [0, 1, 0], pi1, A1b, flat)   # where l-1 beats l-2
    assert margin == 0.0 and path.tolist() == [0, 1, 2] and bounds.tolist() == [0, 1, 2]
    path, bounds, logp, margin = OR.align([0, 1], [0, 2], [0, 1], pi1, A1, flat)
    assert margin == 0.0 and path.tolist() == [0, 1] and bounds.tolist() == [0, 1]          # the end in L-1 beats L-2


def test_check_transcript_outcomes():
    assert OR.check_transcript([0, 1, 0]) == 0 and OR.check_transcript([1, 0, 1]) == 0 and OR.check_transcript([0]) == 0
    assert OR.check_transcript([0, 2, 0]) == 1
    assert OR.check_transcript([0, 1, 1, 0]) == 2
    assert OR.check_transcript([1]) == 3


# --------------------------------------------------------------------------------------------------------------
# the host-side plan, under the sanitizers (a stand-alone program: nothing is loaded into Python)
# --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("optional_plan") / "optional_plan_probe")
    src = os.path.join(ROOT, "tests", "native", "optional_plan_probe.cpp")
    subprocess.run([_host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", src, "-o", exe], check=True)
    return exe


def run_probe(exe, W, N, K, rows, transcripts, optional):
    args = [str(x) for x in (W, N, K, rows)] + [str(len(t)) for t in transcripts] + ["--"]
    args += [str(w) for t in transcripts for w in t]
    if optional is not None:
        args += ["--"] + [str(int(f)) for o in optional for f in o]
    out = subprocess.run([exe] + args, check=True, capture_output=True, text=True).stdout
    return {l.split()[0]: [int(x) for x in l.split()[1:]] for l in out.splitlines()}


@pytest.mark.parametrize("optional,code", [
    ([[1, 0, 1], [0], [0, 1, 0, 1]], 0),           # accepted
    (None, 0),                                     # no flags at all
    ([[1, 0, 1], [0], [0, 2, 0, 1]], 1),           # a flag of 2
    ([[1, 0, 1], [0], [0, 1, 1, 0]], 2),           # adjacent optional positions
    ([[1, 0, 1], [1], [0, 1, 0, 1]], 3),           # a lone optional position
    ([[0, 1, 0], [0], [1, 0, 0, 1]], 0),           # an optional last position of one transcript beside the first of the next
])
def test_transcript_check_and_plan(plan_probe, optional, code):
    W, N, K, rows = 4, 5, 12, 37
    transcripts = [[3, 0, 3], [1], [2, 3, 0, 3]]
    out = run_probe(plan_probe, W, N, K, rows, transcripts, optional)
    assert out["check"] == [code]
    flat = [f for o in optional for f in o] if optional else [0] * 8
    assert code == max([0] + [OR.check_transcript(o) for o in (optional or [])])
    count = np.bincount([w for t in transcripts for w in t], minlength=W)
    assert out["count"] == count.tolist()
    if code == 0:
        ids = [w for t in transcripts for w in t]
        assert out["mand"] == np.bincount([w for w, f in zip(ids, flat) if not f], minlength=W).tolist()
        if optional is None:
            assert out["mand"] == out["count"]
    NP = 8
    base = W * N + W * N * N + W * N + K * W * NP
    assert out["stats"] == [base, base + W, base + 2 * W, base]
    assert out["skip"] == [8, 8 * rows, 256 * rows]


# --------------------------------------------------------------------------------------------------------------
# the layers
# --------------------------------------------------------------------------------------------------------------
def test_entry_points_declared_bound_and_exported():
    from hmm_training_amd import _lib
    header = open(os.path.join(ROOT, "include", "hmmbw.h")).read()
    assert re.search(r"^int hmmbw_align_optional\(hmmbw_ctx \*ctx, int n_words,\s+const double \*pi, const double \*A, "
                     r"const double \*B,\s+const int64_t \*word_offsets, const int32_t \*word_ids, "
                     r"const uint8_t \*optional,\s+int64_t n_seq, int flags,\s+double \*logp_out, int32_t \*path_out, "
                     r"int64_t path_len,\s+int32_t \*bounds_out, int64_t bounds_len\);", header, flags=re.M)
    assert re.search(r"^int hmmbw_embedded_train_optional\(hmmbw_ctx \*ctx, int n_words,\s+double \*pi, double \*A, "
                     r"double \*B,\s+const int64_t \*word_offsets, const int32_t \*word_ids, const uint8_t \*optional,\s+"
                     r"int64_t n_seq,\s+int flags, double epsilon, int64_t max_iterations, int normalise,\s+"
                     r"hmmbw_iter_record \*records, int64_t records_cap, int64_t \*n_records,\s+double \*logp_out\);",
                     header, flags=re.M)
    assert re.search(r"^#define HMMBW_ABI_VERSION 5\b", header, flags=re.M) and _lib.ABI_VERSION == 5
    assert ("hmmbw_align_optional and hmmbw_embedded_train_optional are new entry points of version 5: an older "
            "library lacks the symbols") in re.sub(r"\s+", " ", header)
    for name in ("hmmbw_align_optional", "hmmbw_embedded_train_optional"):
        assert name in _lib.EXPORTED
        assert hasattr(_lib.lib(), name)
    # the plain entry points keep their declarations
    assert re.search(r"^int hmmbw_align\(hmmbw_ctx \*ctx, int n_words,", header, flags=re.M)
    assert re.search(r"^int hmmbw_embedded_train\(hmmbw_ctx \*ctx, int n_words,", header, flags=re.M)


def test_with_optional_and_argument_errors():
    import hmm_training_amd
    from hmm_training_amd import hmm_testing as HT
    from hmm_training_amd import hmm_training as HTR
    from hmm_training_amd.hmm_classes import HMMTrained
    assert hmm_training_amd.with_optional is HTR.with_optional and "with_optional" in hmm_training_amd.__all__
    t, f = hmm_training_amd.with_optional([["one", "two"], ["go"]], "sil")
    assert t == [["sil", "one", "sil", "two", "sil"], ["sil", "go", "sil"]]
    assert f == [[True, False, True, False, True], [True, False, True]]
    assert all(OR.check_transcript(x) == 0 for x in f)
    with pytest.raises(ValueError, match="is empty"):
        hmm_training_amd.with_optional([["one"], []], "sil")
    with pytest.raises(ValueError, match="already names"):
        hmm_training_amd.with_optional([["one", "sil"]], "sil")
    a = HMMTrained(2, 4, np.eye(2), np.full((2, 4), 0.25), np.array([1.0, 0.0]), "a")
    s = HMMTrained(2, 4, np.eye(2), np.full((2, 4), 0.25), np.array([1.0, 0.0]), "sil")
    obs = [np.array([0, 1, 2])]
    for fn in (HT.align_words, HTR.train_connected):
        with pytest.raises(ValueError, match="optional sequences for"):
            fn(obs, [["sil", "a"]], [a, s], optional=[[True, False], [False]])
        with pytest.raises(ValueError, match="entries for a transcript of"):
            fn(obs, [["sil", "a"]], [a, s], optional=[[True]])
    segments, logp = HT.align_words([], [], [a, s], optional=[])     # nothing to do: no device is touched
    assert segments == [] and logp.shape == (0,)
    models, records = HTR.train_connected([], [], [a, s], optional=[])
    assert models == [a, s] and records == []
    import inspect
    from hmm_training_amd.engine import BaumWelchEngine
    for fn in (BaumWelchEngine.align, BaumWelchEngine.embedded_train, HT.align_words, HTR.train_connected):
        assert inspect.signature(fn).parameters["optional"].default is None
