"""State posteriors without a GPU: the NumPy checker of the GPU tests (tests/posterior_ref.py) against brute-force
enumeration of all N^T paths, and the new entry point in the header, the binding table, the built library and
the package."""
import os
import re

import numpy as np
import pytest

import posterior_ref as P
from conftest import ROOT
from test_viterbi import small_model


@pytest.mark.parametrize("topology,zero_col,N,T", [("dense", None, 3, 6), ("left_to_right", None, 3, 6), ("dense", 2, 3, 5),
                                                   ("left_to_right", 1, 3, 5), ("dense", None, 2, 1),
                                                   ("dense", None, 1, 4)])
def test_checker_matches_brute_force(topology, zero_col, N, T):
    rng = np.random.default_rng(17)
    K = 4
    dead = 0
    for _ in range(8):
        pi, A, B = small_model(rng, topology, zero_col, N=N, K=K)
        obs = rng.integers(0, K, size=T)
        gamma, path, logp, gap, la, lb = P.posterior(obs, pi, A, B)
        bgamma, prob = P.brute_force(obs, pi, A, B)
        assert gamma.shape == (T, N) and path.shape == (T,) and gap.shape == (T,)
        if bgamma is None:
            dead += 1
            assert logp == -np.inf and np.all(gamma == 0.0) and np.all(path == -1)
            continue
        np.testing.assert_allclose(logp, np.log(prob), rtol=1e-12)
        np.testing.assert_allclose(gamma, bgamma, rtol=1e-11, atol=1e-300)
        assert np.all(gamma[bgamma == 0.0] == 0.0)  # structural zeros stay exact
        np.testing.assert_allclose(gamma.sum(axis=1), 1.0, rtol=1e-12)
        assert np.array_equal(path, np.argmax(bgamma, axis=1)) or gap.min() < 1e-9
        if N > 1:
            top = np.sort(bgamma, axis=1)
            np.testing.assert_allclose(gap, top[:, -1] - top[:, -2], rtol=1e-9, atol=1e-12)
    if zero_col is not None:
        assert dead > 0  # sequences with the zero-probability symbol occurred


def test_checker_zero_pattern_and_ties():
    # left-to-right from state 0: alpha_t(i) = 0 for i > t, exactly, and the checker's gamma with it
    pi, A = np.array([1.0, 0.0, 0.0]), np.array([[0.5, 0.5, 0.0], [0.0, 0.5, 0.5], [0.0, 0.0, 1.0]])
    B = np.full((3, 2), 0.5)
    gamma, path, logp, gap, la, lb = P.posterior([0, 1, 1, 0], pi, A, B)
    assert np.all(np.isneginf(la[0, 1:])) and np.isneginf(la[1, 2]) and np.all(gamma[0] == [1.0, 0.0, 0.0])
    assert gamma[1, 2] == 0.0 and path[0] == 0
    # every state alike: every gamma is 1 / N, the first maximum is state 0 and the gap is 0
    N, K = 4, 3
    gamma, path, logp, gap, _, _ = P.posterior([0, 2, 1], np.full(N, 1 / N), np.full((N, N), 1 / N), np.full((N, K), 1 / K))
    np.testing.assert_allclose(gamma, 1 / N, rtol=1e-13)
    assert np.all(path == 0) and np.all(np.abs(gap) < 1e-15)
    np.testing.assert_allclose(logp, 3 * np.log(1 / K), rtol=1e-13)


def test_entry_point_declared_bound_and_exported():
    from hmm_training_amd import _lib, build
    assert "hmmbw_posterior" in _lib.EXPORTED
    header = open(os.path.join(ROOT, "include", "hmmbw.h")).read()
    assert re.search(r"^int hmmbw_posterior\(hmmbw_ctx \*ctx, double \*gamma_dev, int64_t gamma_len,\s*"
                     r"int32_t \*path_out, int64_t path_len, double \*logp_out\);", header, flags=re.M)
    assert "hmmbw_posterior is a new entry point of version 5: an older library" in re.sub(r"\s+", " ", header)
    assert hasattr(_lib.lib(), "hmmbw_posterior")
    assert any(os.path.basename(src) == "posterior.hip" for src, _, _ in build.units())


def test_kernels_compile_without_scratch(tmp_path):
    # every instantiation of k_posterior holds its 2 .. 64 transition coefficients in registers: the gfx950 code
    # object's metadata must show no private segment and no spills (GV = 64 would otherwise run from scratch memory)
    import subprocess
    import sys
    from hmm_training_amd import build
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_identity as isa
    src = os.path.join(build.CSRC, "posterior.hip")
    obj = os.path.join(build.PKG, "_obj", "release", "posterior.o")
    if not os.path.exists(obj) or os.path.getmtime(obj) < os.path.getmtime(src):
        obj = str(tmp_path / "posterior.o")
        subprocess.run([build.HIPCC, *build.FLAGS, "-c", src, "-o", obj], check=True)
    fig = isa.figures(isa.code_object(obj, str(tmp_path)))
    kernels = {k: dict(zip(isa.FIGURES, v)) for k, v in fig.items() if "k_posterior" in k}
    # 2 topologies x GV 8, 16 and dense GV 32, 64, each x {gamma, log P only} x {LDS, global table}, and the prep kernel
    assert len(kernels) == 6 * 4 + 1, sorted(kernels)
    for name, f in kernels.items():
        assert f["private_segment_fixed_size"] == "0", (name, f)
        assert f["vgpr_spill_count"] == "0" and f["sgpr_spill_count"] == "0", (name, f)


def test_drop_in_name_resolves():
    import hmm_training_amd
    from hmm_training_amd import hmm_testing
    assert hmm_training_amd.posterior_decode is hmm_testing.posterior_decode
    assert "posterior_decode" in hmm_training_amd.__all__
    gammas, paths, logp = hmm_testing.posterior_decode([], None)
    assert gammas == [] and paths == [] and logp.shape == (0,)
