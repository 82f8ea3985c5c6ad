"""Embedded training without a GPU: the NumPy checker of the GPU tests (tests/embedded_ref.py) against brute-force
enumeration of all labelled paths of the composite chain, and, with one-word transcripts, against the reference's
own training (oracle.hmm_training) on random shapes and on the goldens with a zero-probability sequence, with empty
rows and with one-step sequences; the new entry point in the header, the binding table, the built library and the
build's unit list; the Python layers' argument checks; and the host-side plan of the trainer
(hmm_training_amd/csrc/embed_plan.hpp) through a stand-alone probe built with the address and
undefined-behaviour sanitizers."""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import embedded_ref as ER
from conftest import GOLDEN, ROOT
from test_lds_layout import _host_compiler


# --------------------------------------------------------------------------------------------------------------
# the checker against enumeration
# --------------------------------------------------------------------------------------------------------------
def brute_force(obs, words, pi, A, B, end_final):
    """(log P, Stats-like dict) of one utterance by enumerating every labelled path: a composite state (l, j) per
    step; a step either stays in its instance (within-word arc) or goes from (l, N-1) to (l+1, j) (entry arc)."""
    W, N = pi.shape
    K = B.shape[2]
    L, T = len(words), len(obs)
    S = L * N
    st = ER.Stats(W, N, K)
    total = 0.0
    for states in itertools.product(range(S), repeat=T):
        l0, j0 = divmod(states[0], N)
        if l0 != 0:
            continue
        lT, jT = divmod(states[-1], N)
        if lT != L - 1 or (end_final and jT != N - 1):
            continue
        p = pi[words[0], j0] * B[words[0], j0, obs[0]]
        arcs = []
        for t in range(1, T):
            (pl, pj), (l, j) = divmod(states[t - 1], N), divmod(states[t], N)
            if l == pl:
                p *= A[words[l], pj, j]
                arcs.append(("in", words[l], pj, j))
            elif l == pl + 1 and pj == N - 1:
                p *= pi[words[l], j]
                arcs.append(("entry", words[l], j))
            else:
                p = 0.0
            p *= B[words[l], j, obs[t]]
            if p == 0.0:
                break
        if p == 0.0:
            continue
        total += p
        st.entry[words[0], j0] += p
        for arc in arcs:
            if arc[0] == "in":
                st.xi[arc[1], arc[2], arc[3]] += p
            else:
                st.entry[arc[1], arc[2]] += p
        for t, s in enumerate(states):
            l, j = divmod(s, N)
            st.g_all[words[l], j] += p
            st.b_num[words[l], j, obs[t]] += p
    if total == 0.0:
        return -np.inf, None
    for x in (st.entry, st.xi, st.g_all, st.b_num):
        x /= total
    return float(np.log(total)), st


@pytest.mark.parametrize("end_final", [False, True])
@pytest.mark.parametrize("topology,zero_col", [("dense", None), ("left_to_right", None), ("dense", 1), ("left_to_right", 2)])
def test_checker_matches_brute_force(topology, zero_col, end_final):
    rng = np.random.default_rng(31)
    W, N, K = 2, 2, 3
    seen_inf = seen_fin = 0
    for words in ([0], [1], [0, 1], [1, 1], [0, 0, 1], [1, 0, 0]):  # 1 to 3 words, immediate repeats included
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
            logp, ref = brute_force(obs, words, pi, A, B, end_final)
            st, lp = ER.estep([obs], [words], pi, A, B, end_final)
            assert np.array_equal(st.count, np.bincount(words, minlength=W))
            if ref is None:
                seen_inf += 1
                assert lp[0] == -np.inf
                assert not st.entry.any() and not st.xi.any() and not st.g_all.any() and not st.b_num.any()
                continue
            seen_fin += 1
            np.testing.assert_allclose(lp[0], logp, rtol=1e-12, atol=1e-12)
            for name in ("entry", "xi", "g_all", "b_num"):
                np.testing.assert_allclose(getattr(st, name), getattr(ref, name), rtol=1e-12, atol=1e-12, err_msg=name)
            np.testing.assert_allclose(st.a_den, ref.xi.sum(axis=2), rtol=1e-12, atol=1e-12)
            np.testing.assert_allclose(st.entry.sum(), len(words), rtol=1e-12)  # 1 per instance
            np.testing.assert_allclose(st.g_all.sum(), T, rtol=1e-12)
    assert seen_fin > 0 and seen_inf > 0  # too short for the transcript, or the zero-probability symbol


def test_a_den_is_gamma_without_the_last_row_and_the_exits():
    # the second form the definition allows: sum_{t <= T-2} gamma_t(l, i) minus the exit arcs of i = N - 1
    rng = np.random.default_rng(5)
    W, N, K = 3, 3, 6
    pi, A, B = rng.dirichlet(np.ones(N), size=W), rng.dirichlet(np.ones(N), size=(W, N)), rng.dirichlet(np.ones(K), size=(W, N))
    words, obs = [2, 0, 0, 1], rng.integers(0, K, size=11)
    _, gamma, xi = ER.utterance(obs, words, pi, A, B)
    st, _ = ER.estep([obs], [words], pi, A, B)
    alt = np.zeros((W, N))
    for l, w in enumerate(words):
        alt[w] += gamma[:-1, l * N:(l + 1) * N].sum(axis=0)
        if l + 1 < len(words):
            alt[w, N - 1] -= xi[:, l * N + N - 1, (l + 1) * N:(l + 2) * N].sum()
    np.testing.assert_allclose(st.a_den, alt, rtol=1e-12, atol=1e-14)


# --------------------------------------------------------------------------------------------------------------
# the checker with one-word transcripts is the reference's training
# --------------------------------------------------------------------------------------------------------------
def against_oracle(oracle, obs, N, K, pi0, A0, B0, epsilon, max_iterations):
    off, sym = oracle.to_csr(obs)
    ref = oracle.hmm_training(off, sym, N, K, epsilon, max_iterations, pi0, A0, B0)
    transcripts = [[0]] * len(obs)
    pi, A, B, recs, logp, _ = ER.train(obs, transcripts, pi0[None], A0[None], B0[None], epsilon, max_iterations)
    assert len(recs) == ref.iterations
    np.testing.assert_allclose([L for L, _ in recs], ref.trace_L, rtol=1e-9)
    np.testing.assert_allclose(logp, ref.logP, rtol=1e-9)
    ER.close(pi[0], np.exp(ref.log_pi), "working pi")
    ER.close(A[0], np.exp(ref.log_A), "working A")
    ER.close(B[0], np.exp(ref.log_B), "working B")
    npi, nA, nB = ER.normalised(pi, A, B)
    ER.close(npi[0], ref.pi, "pi")
    ER.close(nA[0], ref.A, "A")
    ER.close(nB[0], ref.B, "B")


@pytest.mark.parametrize("N,K,topology", [(4, 16, "dense"), (5, 32, "left_to_right")])
def test_one_word_transcripts_are_the_reference(oracle, N, K, topology):
    import viterbi_ref as V
    rng = np.random.default_rng(1)
    pi0, A0, B0 = V.model(N, K, topology, rng)
    if topology == "dense":
        pi0 = rng.dirichlet(np.ones(N))
    obs = V.sequences(rng.integers(6, 40, size=12), K, rng)
    against_oracle(oracle, obs, N, K, pi0, A0, B0, 0.0, 6)


@pytest.mark.parametrize("case", ["zero_prob_seq", "empty_rows", "t1_edge"])
def test_one_word_transcripts_on_the_goldens(oracle, case):
    d = np.load(os.path.join(GOLDEN, f"bw_{case}.npz"), allow_pickle=False)
    off, sym = d["offsets"], d["symbols"]
    obs = [sym[off[r]:off[r + 1]] for r in range(len(off) - 1)]
    N, K = int(d["N"]), int(d["M"])
    against_oracle(oracle, obs, N, K, d["init_pi"], d["init_A"], d["init_B"], float(d["epsilon"]), int(d["max_iterations"]))
    # and the recorded reference run itself
    pi, A, B, recs, logp, _ = ER.train(obs, [[0]] * len(obs), d["init_pi"][None], d["init_A"][None], d["init_B"][None],
                                       float(d["epsilon"]), int(d["max_iterations"]), normalise=True)
    assert len(recs) == int(d["iterations"])
    np.testing.assert_allclose([L for L, _ in recs], d["trace_L"], rtol=1e-9)
    ER.close(pi[0], d["out_pi"], "pi")
    ER.close(A[0], d["out_A"], "A")
    ER.close(B[0], d["out_B"], "B")


def test_untrained_word_and_continuation():
    rng = np.random.default_rng(9)
    W, N, K = 3, 3, 8
    pi, A, B = rng.dirichlet(np.ones(N), size=W), rng.dirichlet(np.ones(N), size=(W, N)), rng.dirichlet(np.ones(K), size=(W, N))
    obs = [rng.integers(0, K, size=t) for t in (9, 4, 12, 7)]
    tr = [[0, 2], [2], [2, 2, 0], [0]]  # word 1 has no instance
    p3, a3, b3, r3, _, st = ER.train(obs, tr, pi, A, B, 0.0, 3)
    assert st.count.tolist() == [3, 0, 4]
    assert np.array_equal(p3[1], pi[1]) and np.array_equal(a3[1], A[1]) and np.array_equal(b3[1], B[1])
    p2, a2, b2, r2, _, _ = ER.train(obs, tr, pi, A, B, 0.0, 2)
    p1, a1, b1, r1, _, _ = ER.train(obs, tr, p2, a2, b2, 0.0, 1)
    assert np.array_equal(p1, p3) and np.array_equal(a1, a3) and np.array_equal(b1, b3)
    assert [L for L, _ in r2 + r1] == [L for L, _ in r3] and r1[0][1] == np.inf
    assert all(b >= a - 1e-12 for a, b in zip([L for L, _ in r3], [L for L, _ in r3][1:]))  # EM does not lose likelihood


# --------------------------------------------------------------------------------------------------------------
# the layers
# --------------------------------------------------------------------------------------------------------------
def test_entry_point_declared_bound_and_exported():
    from hmm_training_amd import _lib, build
    assert "hmmbw_embedded_train" in _lib.EXPORTED
    header = open(os.path.join(ROOT, "include", "hmmbw.h")).read()
    assert re.search(r"^int hmmbw_embedded_train\(hmmbw_ctx \*ctx, int n_words,\s+double \*pi, double \*A, double \*B,\s+"
                     r"const int64_t \*word_offsets, const int32_t \*word_ids, int64_t n_seq,\s+"
                     r"int flags, double epsilon, int64_t max_iterations, int normalise,\s+"
                     r"hmmbw_iter_record \*records, int64_t records_cap, int64_t \*n_records,\s+double \*logp_out\);",
                     header, flags=re.M)
    assert re.search(r"^#define HMMBW_EMBED_END_FINAL 1$", header, flags=re.M)
    assert re.search(r"^#define HMMBW_EMBED_DENSE\s+2\b", header, flags=re.M)
    assert re.search(r"^#define HMMBW_ABI_VERSION 5\b", header, flags=re.M)
    assert "hmmbw_embedded_train is a new entry point" in re.sub(r"\s+", " ", header)
    assert (_lib.EMBED_END_FINAL, _lib.EMBED_DENSE) == (1, 2)
    assert hasattr(_lib.lib(), "hmmbw_embedded_train")
    assert any(os.path.basename(src) == "embedded.hip" for src, _, _ in build.units())


def test_drop_in_names_resolve_and_check_their_arguments():
    import hmm_training_amd
    from hmm_training_amd import hmm_training as HT
    from hmm_training_amd.hmm_classes import HMMTrained
    assert hmm_training_amd.train_connected is HT.train_connected
    assert "train_connected" in hmm_training_amd.__all__
    a = HMMTrained(2, 4, np.eye(2), np.full((2, 4), 0.25), np.array([1.0, 0.0]), "a")
    b = HMMTrained(3, 4, np.eye(3), np.full((3, 4), 0.25), np.array([1.0, 0.0, 0.0]), "b")
    a2 = HMMTrained(2, 4, np.eye(2), np.full((2, 4), 0.25), np.array([1.0, 0.0]), "a2")
    obs = [np.array([0, 1, 2])]
    with pytest.raises(ValueError, match="one shape"):
        HT.train_connected(obs, [["a", "b"]], [a, b])
    with pytest.raises(ValueError, match="no model carries"):
        HT.train_connected(obs, [["a", "c"]], [a, a2])
    with pytest.raises(ValueError, match="transcripts for"):
        HT.train_connected(obs, [["a"], ["a2"]], [a, a2])
    with pytest.raises(ValueError, match="no word models"):
        HT.train_connected(obs, [["a"]], [])
    models, records = HT.train_connected([], [], [a, a2])  # nothing to train from: no device is touched
    assert models == [a, a2] and records == []


# --------------------------------------------------------------------------------------------------------------
# the host-side plan, under the sanitizers (a stand-alone program: nothing is loaded into Python)
# --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("embed_plan") / "embed_plan_probe")
    src = os.path.join(ROOT, "tests", "native", "embed_plan_probe.cpp")
    subprocess.run([_host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", src, "-o", exe], check=True)
    return exe


def run_plan(exe, W, N, K, U, longest, lens):
    out = subprocess.run([exe, str(W), str(N), str(K), str(U), str(longest)] + [str(t) for t in lens], check=True,
                         capture_output=True, text=True).stdout
    return {l.split()[0]: [int(x) for x in l.split()[1:]] for l in out.splitlines()}


@pytest.mark.parametrize("longest", [1, 8, 9, 16, 17, 32, 33, 64])
@pytest.mark.parametrize("W,N,K,U,lens", [(1, 4, 8, 16, [5, 9, 1, 30, 2, 2, 7, 8, 8, 40, 3]), (10, 5, 32, 8, list(range(1, 40))),
                                          (17, 8, 64, 8, [17, 3, 9]), (64, 8, 256, 8, [1]), (5, 8, 256, 8, [70] * 9),
                                          (4, 8, 256, 8, []), (3, 1, 7, 32, [4] * 33), (2, 2, 5, 32, [6, 6])])
def test_plan(plan_probe, longest, W, N, K, U, lens):
    rows = run_plan(plan_probe, W, N, K, U, longest, lens)
    GW = 8 if longest <= 8 else 16 if longest <= 16 else 32 if longest <= 32 else 64
    NP = 1 if N <= 1 else 2 if N <= 2 else 4 if N <= 4 else 8
    spw = 64 // GW
    R = len(lens)
    gw, spw_, nslots, nvw, nrows = rows["fig"]
    assert (gw, spw_) == (GW, spw) and nslots == -(-R // U) * U and nvw == -(-nslots // spw)
    slot_len = rows.get("slot_len", [])
    assert sorted(slot_len, reverse=True) == sorted(lens, reverse=True) + [0] * (nslots - R)
    # workspace rows: each wave has as many as its longest slot has steps, one wave after the other
    tw = [max(slot_len[w * spw: (w + 1) * spw]) for w in range(nvw)]
    assert rows.get("work_off", []) == [int(x) for x in np.concatenate([[0], np.cumsum(tw)])[:-1]]
    assert nrows == sum(tw)
    assert rows["work"] == [N * 64, nrows * N * 64 * 8]
    # the tables one after the other, the emission rows 16-B aligned; b_num indexed as the emission table
    pi, A, B, total, np_, bank = rows["tab"]
    assert (pi, A, np_) == (0, W * NP, NP) and B % 2 == 0 and 0 <= B - (A + W * N * N) <= 1 and total == B + K * W * NP
    assert bank == W * N + W * N * N + W * N * K
    assert rows["stats"] == [0, W * N, W * N + W * N * N, 2 * W * N + W * N * N, 2 * W * N + W * N * N + K * W * NP]
    nbytes = K * W * NP * 8
    assert rows["place"] == [1 if nbytes <= 65536 else 0, nbytes]
    assert rows["state"][0] == 6 * 8 + 2 * 4 + 2 * 16 * 8 and rows["state"][1] == 16
    assert rows["check"] == [0, 1, 2, 2, 3, 0]
    assert rows["longest"] == [max(longest, 2)]  # the probe's transcripts have `longest`, 1 and 2 words
    count = np.bincount(np.arange(longest + 3) % W, minlength=W)
    assert rows["count"] == count.tolist()
