"""Viterbi decoding without a GPU: the NumPy checker of the GPU tests (tests/viterbi_ref.py) against brute-force
enumeration, its tie rule and its margin; the new entry point in the header, the binding table and the built
library; and the host-side plan of the decoder (hmm_training_amd/csrc/viterbi_plan.hpp) through a stand-alone
probe built with the address and undefined-behaviour sanitizers."""
import os
import re
import subprocess

import numpy as np
import pytest

import viterbi_ref as V
from conftest import ROOT
from test_lds_layout import _host_compiler


def small_model(rng, topology, zero_col=None, N=3, K=4):
    pi = rng.dirichlet(np.ones(N))
    A = rng.dirichlet(np.ones(N), size=N)
    if topology == "left_to_right":
        A = np.triu(np.tril(A, 1))
        A /= A.sum(axis=1, keepdims=True)
    B = rng.dirichlet(np.full(K, 2.0), size=N)
    if zero_col is not None:
        B[:, zero_col] = 0.0
        B /= B.sum(axis=1, keepdims=True)
    return pi, A, B


@pytest.mark.parametrize("topology,zero_col", [("dense", None), ("left_to_right", None), ("dense", 2),
                                               ("left_to_right", 1)])
def test_checker_matches_brute_force(topology, zero_col):
    rng = np.random.default_rng(7)
    N, T, K = 3, 5, 4
    seen_inf = 0
    for _ in range(12):
        pi, A, B = small_model(rng, topology, zero_col)
        obs = rng.integers(0, K, size=T)
        path, logp, margin = V.viterbi(obs, pi, A, B)
        bpath, best, second = V.brute_force(obs, pi, A, B)
        if best == -np.inf:
            seen_inf += 1
            assert logp == -np.inf and np.all(path == -1) and margin == np.inf
            continue
        np.testing.assert_allclose(logp, best, rtol=1e-13)
        assert np.array_equal(path, bpath)
        np.testing.assert_allclose(V.path_logp(path, obs, pi, A, B), logp, rtol=1e-13)
        # the margin is the gap to the second-best whole path
        if second == -np.inf:
            assert margin == np.inf
        else:
            np.testing.assert_allclose(margin, best - second, rtol=1e-9, atol=1e-13)
    if zero_col is not None:
        assert seen_inf > 0  # sequences with the zero-probability symbol occurred


def test_checker_tie_rule_and_margin():
    # every candidate ties: the first maximum everywhere, so the path is all zeros and the margin is 0
    N, K = 4, 4
    pi, A, B = np.full(N, 1 / N), np.full((N, N), 1 / N), np.full((N, K), 1 / K)
    path, logp, margin = V.viterbi([0, 3, 1, 2, 2, 0], pi, A, B)
    assert np.all(path == 0) and margin == 0.0
    np.testing.assert_allclose(logp, 6 * np.log(1 / N / K), rtol=1e-13)  # one path's probability, not the sum
    # one decision only (T = 1): the margin is the gap between the two best states
    path, logp, margin = V.viterbi([1], [0.6, 0.3, 0.1], np.eye(3), np.full((3, 2), 0.5))
    assert path.tolist() == [0]
    np.testing.assert_allclose(margin, np.log(0.6) - np.log(0.3), rtol=1e-13)
    # two decisions: the predecessor of the end state by log(0.7 0.8 / (0.3 0.2)), the end state by the smaller
    # log(0.8 / 0.2) (the second-best whole path is [0, 1])
    path, logp, margin = V.viterbi([0, 0], [0.7, 0.3], [[0.5, 0.5], [0.5, 0.5]], [[0.8, 0.2], [0.2, 0.8]])
    assert path.tolist() == [0, 0]
    np.testing.assert_allclose(margin, np.log(0.8) - np.log(0.2), rtol=1e-13)


def test_entry_point_declared_bound_and_exported():
    from hmm_training_amd import _lib, build
    assert "hmmbw_viterbi" in _lib.EXPORTED
    header = open(os.path.join(ROOT, "include", "hmmbw.h")).read()
    assert re.search(r"^int hmmbw_viterbi\(hmmbw_ctx \*ctx, double \*logp_out, int32_t \*path_out, int64_t path_len\);",
                     header, flags=re.M)
    assert hasattr(_lib.lib(), "hmmbw_viterbi")
    assert any(os.path.basename(src) == "viterbi.hip" for src, _, _ in build.units())


def test_drop_in_name_resolves():
    import hmm_training_amd
    from hmm_training_amd import hmm_testing
    assert hmm_training_amd.viterbi_decode is hmm_testing.viterbi_decode
    assert "viterbi_decode" in hmm_training_amd.__all__
    assert hmm_testing.viterbi_decode([], None)[0] == [] and hmm_testing.viterbi_decode([], None)[1].shape == (0,)


# --------------------------------------------------------------------------------------------------------------
# the host-side plan, under the sanitizers (a stand-alone program: nothing is loaded into Python)
# --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("viterbi_plan") / "viterbi_plan_probe")
    src = os.path.join(ROOT, "tests", "native", "viterbi_plan_probe.cpp")
    subprocess.run([_host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", src, "-o", exe], check=True)
    return exe


def run_plan(exe, N, U, lens):
    out = subprocess.run([exe, str(N), str(U)] + [str(t) for t in lens], check=True, capture_output=True, text=True).stdout
    rows = {l.split()[0]: [int(x) for x in l.split()[1:]] for l in out.splitlines()}
    return rows


@pytest.mark.parametrize("N,U,lens", [(8, 8, [5, 9, 1, 30, 2, 2, 7, 8, 8, 40, 3]), (3, 16, [4] * 16 + [1]), (64, 16, [17, 3, 9]),
                                      (17, 16, list(range(1, 40))), (16, 4, [1]), (5, 8, [])])
def test_plan_offsets_and_rows(plan_probe, N, U, lens):
    rows = run_plan(plan_probe, N, U, lens)
    GV = 8 if N <= 8 else 16 if N <= 16 else 32 if N <= 32 else 64
    spw = 64 // GV
    R = len(lens)
    assert rows["fig"][:2] == [GV, spw]
    nslots, nvw, total, psi_rows = rows["fig"][2:]
    assert nslots == -(-R // U) * U and nvw == -(-nslots // spw) and total == sum(lens)
    slot_len, slot_seq, slot_out = rows.get("slot_len", [])[:], rows.get("slot_seq", []), rows.get("slot_out", [])
    # the layout: the stable length-descending order of the sequences, then padding
    order = sorted(range(R), key=lambda r: -lens[r])
    assert slot_seq == order + [-1] * (nslots - R)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(int)
    assert slot_out == [int(off[r]) for r in order] + [-1] * (nslots - R)
    # every entry of the path belongs to exactly one slot
    covered = np.zeros(total, dtype=int)
    for s in range(R):
        covered[slot_out[s]: slot_out[s] + slot_len[s]] += 1
    assert np.all(covered == 1)
    # back-pointer rows: each decoding wave has as many as its longest slot, one after the other
    tw = [max(slot_len[w * spw: (w + 1) * spw]) for w in range(nvw)]
    assert rows.get("psi_off", []) == [int(x) for x in np.concatenate([[0], np.cumsum(tw)])[:-1]]
    assert psi_rows == sum(tw)


def test_plan_table_placement_and_divisor(plan_probe):
    rows = run_plan(plan_probe, 8, 8, [3])
    # K GV: in LDS (1) or global (0)
    place = dict(zip(zip(rows["place"][0::3], rows["place"][1::3]), rows["place"][2::3]))
    assert place[(4, 8)] == 1 and place[(256, 8)] == 1 and place[(256, 16)] == 1 and place[(1024, 8)] == 1
    assert place[(1024, 64)] == 0 and place[(256, 64)] == 0 and place[(128, 64)] == 1
    # lds_tables G: divisor, shift
    div = {(a, g): (d, s) for a, g, d, s in zip(*[rows["div"][i::4] for i in range(4)])}
    assert div[(1, 8)] == (128, 7) and div[(1, 16)] == (256, 8) and div[(1, 2)] == (32, 5) and div[(0, 16)] == (1, 0)
    assert rows["shift"] == [-1, 0, -1, 4, -1]  # of 0, 1, 48, 16, -8
