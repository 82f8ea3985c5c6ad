"""Connected-word decoding without a GPU: the NumPy checker of the GPU tests (tests/wordnet_ref.py) against
brute-force enumeration of all labelled paths and against the ordinary Viterbi checker on the composite model; the
pure segment builder; the new entry point in the header, the binding table, the built library and the build's
unit list; and the host-side plan of the decoder (hmm_training_amd/csrc/wordnet_plan.hpp, plan_viterbi_group)
through a stand-alone probe built with the address and undefined-behaviour sanitizers."""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import viterbi_ref as V
import wordnet_ref as WR
from conftest import ROOT
from test_lds_layout import _host_compiler


def small_bank(rng, W, N, K, topology, zero_col=None, zero_g=False):
    pi = rng.dirichlet(np.ones(N), size=W)
    A = rng.dirichlet(np.ones(N), size=(W, N))
    if topology == "left_to_right":
        A = np.triu(np.tril(A, 1))
        A /= A.sum(axis=2, keepdims=True)
    B = rng.dirichlet(np.full(K, 2.0), size=(W, N))
    if zero_col is not None:
        B[:, :, zero_col] = 0.0
        B /= B.sum(axis=2, keepdims=True)
    G = 0.3 * rng.dirichlet(np.ones(W), size=W)
    if zero_g:
        G[rng.integers(0, W), rng.integers(0, W)] = 0.0
    return pi, A, B, rng.dirichlet(np.ones(W)), G


def brute_force(obs, pi, A, B, init, G, end_final):
    """(best logp, second-best logp, best labelling) over all labelled paths: a composite state per step and an
    arc type (within-word or entry) per step after the first; an entry arc comes only from j_prev = N - 1, a
    within-word arc stays in the word.  The best labelling is the one the decoder's tie rules pick when it is
    unique; it is returned only for that case."""
    W, N = pi.shape
    T = len(obs)
    scored = []
    for states in itertools.product(range(W * N), repeat=T):
        if end_final and states[-1] % N != N - 1:
            continue
        for arcs in itertools.product((0, 1), repeat=T - 1):
            start = np.array((1,) + arcs, dtype=np.uint8)
            ok = all((states[t - 1] % N == N - 1) if arcs[t - 1] else (states[t - 1] // N == states[t] // N)
                     for t in range(1, T))
            if ok:
                scored.append((WR.path_logp(states, start, obs, pi, A, B, init, G), states, tuple(start)))
    scored.sort(key=lambda x: -x[0])
    best = scored[0][0]
    second = scored[1][0] if len(scored) > 1 else -np.inf
    return best, second, scored[0]


@pytest.mark.parametrize("W,N,Ts", [(2, 2, (1, 2, 3, 4)), (3, 2, (3,))])
@pytest.mark.parametrize("topology,zero_col,end_final", [("dense", None, False), ("left_to_right", None, True),
                                                         ("dense", 1, True), ("left_to_right", 2, False)])
def test_checker_matches_brute_force(W, N, Ts, topology, zero_col, end_final):
    rng = np.random.default_rng(17 + W)
    K = 3
    seen_inf = 0
    for T in Ts:
        for _ in range(4):
            pi, A, B, init, G = small_bank(rng, W, N, K, topology, zero_col, zero_g=True)
            obs = rng.integers(0, K, size=T)
            path, start, logp, margin = WR.decode(obs, pi, A, B, init, G, end_final)
            best, second, (_, bstates, bstart) = brute_force(obs, pi, A, B, init, G, end_final)
            if best == -np.inf:
                seen_inf += 1
                assert logp == -np.inf and np.all(path == -1) and np.all(start == 0) and margin == np.inf
                continue
            np.testing.assert_allclose(logp, best, rtol=1e-13)
            np.testing.assert_allclose(WR.path_logp(path, start, obs, pi, A, B, init, G), logp, rtol=1e-13)
            WR.check_labelling(path, start, obs, W, N)
            # the margin is the gap to the second-best labelled path
            if second == -np.inf:
                assert margin == np.inf
            else:
                np.testing.assert_allclose(margin, best - second, rtol=1e-9, atol=1e-13)
            if margin > 1e-12:
                assert tuple(path) == bstates and tuple(start) == bstart
    if zero_col is not None:
        assert seen_inf > 0  # sequences with the zero-probability symbol occurred


@pytest.mark.parametrize("W,N,topology", [(1, 4, "dense"), (3, 3, "left_to_right"), (5, 4, "dense"),
                                          (10, 5, "left_to_right"), (17, 8, "dense"), (64, 8, "left_to_right")])
@pytest.mark.parametrize("with_g", [True, False])
def test_checker_logp_is_the_composite_viterbi_score(W, N, topology, with_g):
    rng = np.random.default_rng(100 + W + N)
    K = 12
    pi, A, B, init, G = WR.bank(W, N, K, topology, rng)
    if not with_g:
        G = None
    cpi, cA, cB = WR.composite(pi, A, B, init, G)
    for T in (1, 2, 9, 23):
        obs = rng.integers(0, K, size=T)
        path, start, logp, margin = WR.decode(obs, pi, A, B, init, G)
        cpath, clogp, _ = V.viterbi(obs, cpi, cA, cB)
        np.testing.assert_allclose(logp, clogp, rtol=1e-13)
        np.testing.assert_allclose(WR.path_logp(path, start, obs, pi, A, B, init, G), logp, rtol=1e-13)
        WR.check_labelling(path, start, obs, W, N)
        assert margin >= 0.0


def test_checker_tie_rules():
    # every decision ties: composite state 0 throughout, a word start only at t = 0, margin 0
    W, N, K = 3, 2, 4
    pi, A, B = np.full((W, N), 1 / N), np.full((W, N, N), 1 / N), np.full((W, N, K), 1 / K)
    path, start, logp, margin = WR.decode([0, 3, 1, 2, 2], pi, A, B, np.full(W, 1 / W), np.full((W, W), 1.0))
    assert np.all(path == 0) and start.tolist() == [1, 0, 0, 0, 0] and margin == 0.0
    np.testing.assert_allclose(logp, np.log(1 / W / N / K) + 4 * np.log(1 / N / K), rtol=1e-13)
    # a word is left only from its last state, whatever that state's row of A holds: two one-state words that
    # cannot stay (a = 0) alternate or repeat through the entry arc alone
    pi, A, B = np.ones((2, 1)), np.zeros((2, 1, 1)), np.array([[[0.9, 0.1]], [[0.1, 0.9]]])
    path, start, logp, margin = WR.decode([0, 0, 1], pi, A, B)
    assert path.tolist() == [0, 0, 1] and start.tolist() == [1, 1, 1]
    np.testing.assert_allclose(logp, 3 * np.log(0.9), rtol=1e-13)
    np.testing.assert_allclose(margin, np.log(0.9) - np.log(0.1), rtol=1e-13)


def test_segments_from_path():
    from hmm_training_amd.hmm_testing import segments_from_path
    N, words = 3, ["go", "left", "stop"]
    #        go go go | go go      | stop stop stop stop | left
    path = [0, 1, 2, 0, 2, 6, 6, 7, 8, 3]
    start = [1, 0, 0, 1, 0, 1, 0, 0, 0, 1]
    assert segments_from_path(np.array(path, dtype=np.int32), np.array(start, dtype=np.uint8), N, words) == [
        ("go", 0, 3), ("go", 3, 5), ("stop", 5, 9), ("left", 9, 10)]
    assert segments_from_path(np.full(4, -1, dtype=np.int32), np.zeros(4, dtype=np.uint8), N, words) == []
    assert segments_from_path(np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.uint8), N, words) == []
    # a held word is one segment
    assert segments_from_path([3, 3, 4, 4, 5], [1, 0, 0, 0, 0], N, words) == [("left", 0, 5)]


def test_entry_point_declared_bound_and_exported():
    from hmm_training_amd import _lib, build
    assert "hmmbw_wordnet_decode" in _lib.EXPORTED
    header = open(os.path.join(ROOT, "include", "hmmbw.h")).read()
    assert re.search(r"^int hmmbw_wordnet_decode\(hmmbw_ctx \*ctx, int n_words, const double \*pi, const double \*A, "
                     r"const double \*B,\s+const double \*word_init, const double \*word_trans, int flags,\s+"
                     r"double \*logp_out, int32_t \*path_out, uint8_t \*start_out, int64_t path_len\);",
                     header, flags=re.M)
    assert re.search(r"^#define HMMBW_WORDNET_END_FINAL 1$", header, flags=re.M)
    assert re.search(r"^#define HMMBW_WORDNET_DENSE\s+2\b", header, flags=re.M)
    assert re.search(r"^#define HMMBW_ABI_VERSION 5\b", header, flags=re.M)
    assert (_lib.WORDNET_END_FINAL, _lib.WORDNET_DENSE) == (1, 2)
    assert hasattr(_lib.lib(), "hmmbw_wordnet_decode")
    assert any(os.path.basename(src) == "wordnet.hip" for src, _, _ in build.units())


def test_drop_in_names_resolve():
    import hmm_training_amd
    from hmm_training_amd import hmm_testing
    from hmm_training_amd.hmm_classes import HMMTrained
    assert hmm_training_amd.decode_words is hmm_testing.decode_words
    assert hmm_training_amd.segments_from_path is hmm_testing.segments_from_path
    assert "decode_words" in hmm_training_amd.__all__
    segments, logp = hmm_testing.decode_words([], [])
    assert segments == [] and logp.shape == (0,)
    a = HMMTrained(2, 4, np.eye(2), np.full((2, 4), 0.25), np.array([1.0, 0.0]), "a")
    b = HMMTrained(3, 4, np.eye(3), np.full((3, 4), 0.25), np.array([1.0, 0.0, 0.0]), "b")
    with pytest.raises(ValueError):
        hmm_testing.decode_words([np.array([0, 1])], [a, b])


# --------------------------------------------------------------------------------------------------------------
# the host-side plan, under the sanitizers (a stand-alone program: nothing is loaded into Python)
# --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("wordnet_plan") / "wordnet_plan_probe")
    src = os.path.join(ROOT, "tests", "native", "wordnet_plan_probe.cpp")
    subprocess.run([_host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", src, "-o", exe], check=True)
    return exe


def run_plan(exe, W, N, K, U, lens):
    out = subprocess.run([exe, str(W), str(N), str(K), str(U)] + [str(t) for t in lens], check=True,
                         capture_output=True, text=True).stdout
    return {l.split()[0]: [int(x) for x in l.split()[1:]] for l in out.splitlines()}


@pytest.mark.parametrize("W,N,K,U,lens", [(1, 4, 8, 16, [5, 9, 1, 30, 2, 2, 7, 8, 8, 40, 3]), (9, 2, 16, 32, [4] * 32 + [1]),
                                          (10, 5, 32, 8, list(range(1, 40))), (17, 8, 64, 8, [17, 3, 9]),
                                          (64, 8, 256, 8, [1]), (33, 1, 8, 32, [])])
def test_plan(plan_probe, W, N, K, U, lens):
    rows = run_plan(plan_probe, W, N, K, U, lens)
    GW = 8 if W <= 8 else 16 if W <= 16 else 32 if W <= 32 else 64
    NP = 1 if N <= 1 else 2 if N <= 2 else 4 if N <= 4 else 8
    spw = 64 // GW
    R = len(lens)
    assert rows["fig"][:2] == [GW, spw]
    nslots, nvw, total, psi_rows = rows["fig"][2:]
    assert nslots == -(-R // U) * U and nvw == -(-nslots // spw) and total == sum(lens)
    slot_len, slot_out = rows.get("slot_len", []), rows.get("slot_out", [])
    order = sorted(range(R), key=lambda r: -lens[r])
    off = np.concatenate([[0], np.cumsum(lens)]).astype(int)
    assert slot_out == [int(off[r]) for r in order] + [-1] * (nslots - R)
    # back-pointer rows: each decoding wave has as many as its longest slot, one after the other
    tw = [max(slot_len[w * spw: (w + 1) * spw]) for w in range(nvw)]
    assert rows.get("psi_off", []) == [int(x) for x in np.concatenate([[0], np.cumsum(tw)])[:-1]]
    assert psi_rows == sum(tw)
    # the state decoder's plan is the group plan of its own width, and both share slot_out
    assert rows["same"] == [1]
    # the tables: one after the other, the emission rows 16-B aligned
    pi, init, A, G, B, ttotal, np_, in_len = rows["tab"]
    assert (pi, init, A, G, np_) == (0, GW * NP, GW * NP + GW, GW * NP + GW + GW * N * N, NP)
    assert B % 2 == 0 and 0 <= B - (G + GW * GW) <= 1 and ttotal == B + K * GW * NP
    assert in_len == W * N + W * N * N + W * N * K + W + W * W
    in_lds, nbytes, row_bytes = rows["place"]
    assert nbytes == K * GW * NP * 8 and in_lds == (1 if nbytes <= 65536 else 0) and row_bytes == 320
    assert rows["lr"] == [1, 1 if N == 1 else 0, -1 if N < 3 else 0]  # a full 1 x 1 matrix is left-to-right
    assert rows["ok"] == [1, 0, 0, 0, 1]
