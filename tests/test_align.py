"""Forced alignment without a GPU: the NumPy checker of the GPU tests (tests/align_ref.py) against brute-force
enumeration of all complete paths of the chain and against the ordinary Viterbi checker on the composite model of
tests/embedded_ref.py; its tie rules and its labelling check; the new entry point in the header, the binding
table, the built library and the build's unit list; the Python layers' argument checks; and the host-side plan of
the aligner (hmm_training_amd/csrc/align_plan.hpp, plan_viterbi_group) through a stand-alone probe built with the
address and undefined-behaviour sanitizers."""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import align_ref as AR
import embedded_ref as ER
import viterbi_ref as V
import wordnet_ref as WR
from conftest import ROOT
from test_lds_layout import _host_compiler


# --------------------------------------------------------------------------------------------------------------
# the checker against enumeration
# --------------------------------------------------------------------------------------------------------------
def brute_force(obs, words, pi, A, B, end_final):
    """(best logp, second-best logp, best path or None) over all complete paths of the chain: a composite state
    (l, j) per step, from position 0 to position L - 1 (end_final: to (L - 1, N - 1)), positions moving by 0 or by 1
    from a last state.  Scored by AR.path_logp, which has no recursion in it."""
    N = pi.shape[1]
    L, T = len(words), len(obs)
    scored = []
    for states in itertools.product(range(L * N), repeat=T):
        pos = [s // N for s in states]
        if pos[0] != 0 or pos[-1] != L - 1 or (end_final and states[-1] % N != N - 1):
            continue
        if any(not (b == a or (b == a + 1 and s % N == N - 1)) for a, b, s in zip(pos, pos[1:], states)):
            continue
        scored.append((AR.path_logp(states, obs, words, pi, A, B), states))
    if not scored:
        return -np.inf, -np.inf, None
    scored.sort(key=lambda x: -x[0])
    second = scored[1][0] if len(scored) > 1 else -np.inf
    return scored[0][0], second, scored[0][1]


@pytest.mark.parametrize("end_final", [False, True])
@pytest.mark.parametrize("topology,zero_col", [("dense", None), ("left_to_right", None), ("dense", 1), ("left_to_right", 2)])
def test_checker_matches_brute_force(topology, zero_col, end_final):
    rng = np.random.default_rng(71)
    W, N, K = 2, 2, 3
    seen_inf = seen_fin = seen_short = 0
    for words in ([0], [1], [0, 1], [1, 1], [0, 0, 1], [1, 0, 0]):  # L <= 3, immediate repeats included
        for T in range(1, 6):
            pi = rng.dirichlet(np.ones(N), size=W)
            A = rng.dirichlet(np.ones(N), size=(W, N))
            if topology == "left_to_right":
                A = np.triu(np.tril(A, 1))
                pi[:] = [1.0, 0.0]
            B = rng.dirichlet(np.full(K, 2.0), size=(W, N))
            if zero_col is not None:
                B[:, :, zero_col] = 0.0
            obs = rng.integers(0, K, size=T)
            path, bounds, logp, margin = AR.align(obs, words, pi, A, B, end_final)
            best, second, bpath = brute_force(obs, words, pi, A, B, end_final)
            if T < len(words):
                seen_short += 1
                assert best == -np.inf  # every instance takes a frame
            if best == -np.inf:
                seen_inf += 1
                assert logp == -np.inf and np.all(path == -1) and np.all(bounds == -1) and margin == np.inf
                assert path.shape == (T,) and bounds.shape == (len(words),)
                continue
            seen_fin += 1
            np.testing.assert_allclose(logp, best, rtol=1e-13)
            np.testing.assert_allclose(AR.path_logp(path, obs, words, pi, A, B), logp, rtol=1e-13)
            AR.check_labelling(path, bounds, T, len(words), N)
            if second == -np.inf:
                assert margin == np.inf
            else:  # the margin is the gap to the second-best complete path
                np.testing.assert_allclose(margin, best - second, rtol=1e-9, atol=1e-13)
            if margin > 1e-12:
                assert tuple(path) == bpath
    assert seen_fin > 0 and seen_inf > 0 and seen_short > 0


@pytest.mark.parametrize("W,N,topology", [(1, 4, "dense"), (3, 3, "left_to_right"), (5, 4, "dense"),
                                          (10, 5, "left_to_right"), (17, 8, "dense"), (6, 1, "dense")])
@pytest.mark.parametrize("end_final", [False, True])
def test_checker_is_the_viterbi_of_the_composite_chain(W, N, topology, end_final):
    rng = np.random.default_rng(300 + W + N)
    K = 12
    pi, A, B, _, _ = WR.bank(W, N, K, topology, rng)
    for L, T in ((1, 1), (1, 9), (2, 2), (3, 11), (7, 23), (9, 9)):
        words = ER.transcripts_for(W, [L], rng)[0]
        obs = rng.integers(0, K, size=T)
        path, bounds, logp, margin = AR.align(obs, words, pi, A, B, end_final)
        init, trans, emis, end = ER.composite(words, pi, A, B, end_final)
        # an ordinary Viterbi over the L N states, its end restricted to the allowed states by one more step: a
        # sink state that only the allowed states reach and that emits a symbol of its own
        S = L * N
        cA = np.zeros((S + 1, S + 1))
        cA[:S, :S] = trans
        cA[:S, S] = end
        cB = np.zeros((S + 1, K + 1))
        cB[:S, :K] = emis
        cB[S, K] = 1.0
        cpath, clogp, _ = V.viterbi(np.append(obs, K), np.append(init, 0.0), cA, cB)
        assert np.isfinite(logp) and margin >= 0.0
        np.testing.assert_allclose(logp, clogp, rtol=1e-13)
        np.testing.assert_allclose(AR.path_logp(path, obs, words, pi, A, B), logp, rtol=1e-13)
        AR.check_labelling(path, bounds, T, L, N)
        if margin > 1e-9:
            assert np.array_equal(path, cpath[:-1])


def test_checker_tie_rules():
    # every complete path ties.  The end is the smallest j; the within-word arc wins its tie with the entry arc, so
    # the backtrace stays in a position for as long as that position was reachable one step earlier, and position l
    # was first reachable at frame l: it is entered there, from the last state of position l - 1
    W, N, K = 2, 2, 4
    pi, A, B = np.full((W, N), 1 / N), np.full((W, N, N), 1 / N), np.full((W, N, K), 1 / K)
    path, bounds, logp, margin = AR.align([0, 3, 1, 2, 2], [0, 1, 1], pi, A, B)
    assert bounds.tolist() == [0, 1, 2] and path.tolist() == [1, 3, 4, 4, 4] and margin == 0.0
    np.testing.assert_allclose(logp, 5 * np.log(1 / N / K), rtol=1e-13)
    # one-state words that cannot stay (a = 0): T == L is the only feasible length
    pi, A, B = np.ones((2, 1)), np.zeros((2, 1, 1)), np.array([[[0.9, 0.1]], [[0.1, 0.9]]])
    path, bounds, logp, margin = AR.align([0, 0, 1], [0, 0, 1], pi, A, B)
    assert path.tolist() == [0, 1, 2] and bounds.tolist() == [0, 1, 2] and margin == np.inf
    np.testing.assert_allclose(logp, 3 * np.log(0.9), rtol=1e-13)
    assert AR.align([0, 0, 1, 1], [0, 0, 1], pi, A, B)[2] == -np.inf
    assert AR.align([0, 0], [0, 0, 1], pi, A, B)[2] == -np.inf


def test_check_labelling_rejects_what_it_should():
    N = 3
    good, bounds = np.array([0, 1, 2, 3, 5, 8], dtype=np.int32), np.array([0, 3, 5], dtype=np.int32)
    AR.check_labelling(good, bounds, 6, 3, N)
    for bad_path, bad_bounds in ((np.array([0, 1, 1, 3, 5, 8], dtype=np.int32), bounds),      # an increase from state 1
                                 (np.array([0, 1, 2, 6, 6, 8], dtype=np.int32), bounds),      # a skipped position
                                 (np.array([0, 2, 3, 2, 5, 8], dtype=np.int32), bounds),      # a position that decreases
                                 (np.array([3, 4, 5, 5, 5, 8], dtype=np.int32), bounds),      # does not start in 0
                                 (np.array([0, 1, 2, 3, 5, 5], dtype=np.int32), bounds),      # does not reach L - 1
                                 (good, np.array([0, 3, 4], dtype=np.int32))):                # bounds beside the path
        with pytest.raises(AssertionError):
            AR.check_labelling(bad_path, bad_bounds, 6, 3, N)


# --------------------------------------------------------------------------------------------------------------
# the layers
# --------------------------------------------------------------------------------------------------------------
def test_entry_point_declared_bound_and_exported():
    from hmm_training_amd import _lib, build
    assert "hmmbw_align" in _lib.EXPORTED
    header = open(os.path.join(ROOT, "include", "hmmbw.h")).read()
    assert re.search(r"^int hmmbw_align\(hmmbw_ctx \*ctx, int n_words,\s+const double \*pi, const double \*A, "
                     r"const double \*B,\s+const int64_t \*word_offsets, const int32_t \*word_ids, int64_t n_seq,\s+"
                     r"int flags,\s+double \*logp_out, int32_t \*path_out, int64_t path_len,\s+"
                     r"int32_t \*bounds_out, int64_t bounds_len\);", header, flags=re.M)
    assert re.search(r"^#define HMMBW_ALIGN_END_FINAL 1$", header, flags=re.M)
    assert re.search(r"^#define HMMBW_ALIGN_DENSE\s+2\b", header, flags=re.M)
    assert re.search(r"^#define HMMBW_ABI_VERSION 5\b", header, flags=re.M)
    assert "hmmbw_align is a new entry point of version 5: an older library lacks the symbol" in re.sub(r"\s+", " ", header)
    assert (_lib.ALIGN_END_FINAL, _lib.ALIGN_DENSE) == (1, 2)
    assert hasattr(_lib.lib(), "hmmbw_align")
    assert any(os.path.basename(src) == "align.hip" for src, _, _ in build.units())


def test_drop_in_names_resolve_and_check_their_arguments():
    import hmm_training_amd
    from hmm_training_amd import hmm_testing as HT
    from hmm_training_amd.hmm_classes import HMMTrained
    assert hmm_training_amd.align_words is HT.align_words
    assert "align_words" in hmm_training_amd.__all__
    a = HMMTrained(2, 4, np.eye(2), np.full((2, 4), 0.25), np.array([1.0, 0.0]), "a")
    b = HMMTrained(3, 4, np.eye(3), np.full((3, 4), 0.25), np.array([1.0, 0.0, 0.0]), "b")
    a2 = HMMTrained(2, 4, np.eye(2), np.full((2, 4), 0.25), np.array([1.0, 0.0]), "a2")
    obs = [np.array([0, 1, 2])]
    with pytest.raises(ValueError, match="one shape"):
        HT.align_words(obs, [["a", "b"]], [a, b])
    with pytest.raises(ValueError, match="no model carries"):
        HT.align_words(obs, [["a", "c"]], [a, a2])
    with pytest.raises(ValueError, match="transcripts for"):
        HT.align_words(obs, [["a"], ["a2"]], [a, a2])
    with pytest.raises(ValueError, match="no word models"):
        HT.align_words(obs, [["a"]], [])
    segments, logp = HT.align_words([], [], [a, a2])  # nothing to align: no device is touched
    assert segments == [] and logp.shape == (0,)


# --------------------------------------------------------------------------------------------------------------
# the host-side plan, under the sanitizers (a stand-alone program: nothing is loaded into Python)
# --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("align_plan") / "align_plan_probe")
    src = os.path.join(ROOT, "tests", "native", "align_plan_probe.cpp")
    subprocess.run([_host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", src, "-o", exe], check=True)
    return exe


def run_plan(exe, W, N, K, U, longest, lens):
    out = subprocess.run([exe, str(W), str(N), str(K), str(U), str(longest)] + [str(t) for t in lens], check=True,
                         capture_output=True, text=True).stdout
    return {l.split()[0]: [int(x) for x in l.split()[1:]] for l in out.splitlines()}


@pytest.mark.parametrize("longest", [1, 8, 9, 16, 17, 32, 33, 64])
@pytest.mark.parametrize("W,N,K,U,lens", [(1, 4, 8, 16, [5, 9, 1, 30, 2, 2, 7, 8, 8, 40, 3]), (10, 5, 32, 8, list(range(1, 40))),
                                          (64, 8, 256, 8, [1]), (5, 8, 256, 8, [70] * 9), (4, 8, 256, 8, []),
                                          (3, 1, 7, 32, [4] * 33)])
def test_plan(plan_probe, longest, W, N, K, U, lens):
    rows = run_plan(plan_probe, W, N, K, U, longest, lens)
    GW = AR.gw_of(longest)
    NP = 1 if N <= 1 else 2 if N <= 2 else 4 if N <= 4 else 8
    spw = 64 // GW
    R = len(lens)
    gw, spw_, nslots, nvw, nrows, total = rows["fig"]
    assert (gw, spw_) == (GW, spw) and nslots == -(-R // U) * U and nvw == -(-nslots // spw) and total == sum(lens)
    slot_len, slot_out = rows.get("slot_len", []), rows.get("slot_out", [])
    order = sorted(range(R), key=lambda r: -lens[r])
    off = np.concatenate([[0], np.cumsum(lens)]).astype(int)
    assert slot_out == [int(off[r]) for r in order] + [-1] * (nslots - R)
    # back-pointer rows: each wave has as many as its longest slot has steps, one wave after the other, 256 B each
    tw = [max(slot_len[w * spw: (w + 1) * spw]) for w in range(nvw)]
    assert rows.get("psi_off", []) == [int(x) for x in np.concatenate([[0], np.cumsum(tw)])[:-1]]
    assert nrows == sum(tw)
    assert rows["bp"] == [256, 256 * nrows]
    # the trainer's tables, holding logarithms: one after the other, the emission rows 16-B aligned, W words
    pi, A, B, ttotal, np_, bank = rows["tab"]
    assert (pi, A, np_) == (0, W * NP, NP) and B % 2 == 0 and 0 <= B - (A + W * N * N) <= 1 and ttotal == B + K * W * NP
    assert bank == W * N + W * N * N + W * N * K
    nbytes = K * W * NP * 8
    assert rows["place"] == [1 if nbytes <= 65536 else 0, nbytes]
    assert rows["flags"] == [1, 1, 1, 1, 0, 0]
    assert rows["lengths"] == [0, 1, 2, 1, 1 if sum(lens) else 2]
