"""The joined E-step on the class-split LDS emission tables (k_estep_join<.., 1>, lds_layout.hpp) against the
oracle on the same inputs: 3 EM iterations through the production path (the merged M-step prologue rebuilds
both classes' tables twice), every recorded L and every log P at rtol 1e-9, then one statistics pass (the
unmerged table build) with the complete statistics at rtol 1e-9 (tests/test_gpu_fullsize.py::assert_stats).
Every case asserts which layout the launch reports (HMMBW_INFO_LDS_LAYOUT).  The cases force the layout on
(HMMBW_OPT_LDS_LAYOUT = 1) since by default a context takes it only where it measured faster (long left-to-right
sweeps with extra groups: test_default_policy), far from the smallest shapes at which the kernel can go wrong.

With equal lengths the length-sorted slot assignment is the identity: sequence r sits in slot r % 8 of wave
r // 8 (G = 8), which is how the cases below aim symbols at slots."""
import numpy as np
import pytest

from test_gpu_fullsize import LL_RTOL, _params, assert_stats, statistics_pass

pytestmark = pytest.mark.gpu

ITERS = 3


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: the GPU tests need an MI355X")


def run_case(oracle, obs, N, K, topology, layout, joined=None, split_extra=None, option=1, params=None):
    """Train ITERS iterations on `obs`, check everything against the oracle, assert the reported layout (and map);
    returns (trace of L, log P, decoded statistics) for comparisons between contexts.  params: the starting
    (pi, A, B) instead of the seeded default."""
    from hmm_training_amd._lib import OPT_LDS_LAYOUT
    from hmm_training_amd.engine import BaumWelchEngine, to_csr
    off, sym = to_csr(obs)
    sym64 = sym.astype(np.int64)
    R, total = len(obs), int(off[-1])
    pi, A, B = _params(N, K, topology, 7) if params is None else params
    ref = oracle.hmm_training(off, sym64, N, K, 0.0, ITERS, pi, A, B)
    with BaumWelchEngine(N, K, topology=topology) as eng:
        if option is not None:
            eng.set_option(OPT_LDS_LAYOUT, option)
        eng.set_observations(obs)
        eng.set_params(pi, A, B)
        lm = eng.launch_map()
        assert lm["lds_layout"] == layout == eng.lds_layout, lm
        if joined is not None:
            assert lm["joined"] == joined, lm
        if split_extra is not None:
            assert lm["split_extra"] == split_extra, lm
        eng.reset(0.0, ITERS)
        eng.enqueue_iterations(ITERS)
        st, recs = eng.status(0, ITERS)
        assert st.iterations == ITERS
        trace = np.array([L for L, _ in recs])
        np.testing.assert_allclose(trace, ref.trace_L, rtol=LL_RTOL)
        ll_last = eng.loglik()
        np.testing.assert_allclose(ll_last, ref.logP, rtol=LL_RTOL)
        p_cur, A_cur, B_cur = eng.params(normalise=False)
        g, ll, _ = statistics_pass(eng, N, K, R)
        assert eng.lds_layout == layout
    s = oracle.estep_logstats(off, sym64, N, K, p_cur, A_cur, B_cur)
    np.testing.assert_allclose(ll, s.logP, rtol=LL_RTOL)
    assert_stats(g, s, R, total / R)
    return trace, ll, g


def uniform(R, T, K, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, K, size=T) for _ in range(R)]


@pytest.mark.parametrize("K", [256, 2, 255])
def test_joined_without_extra_groups(oracle, K):
    """R = 96, T = 9 (two chunks), N = 8: the joined kernel with idle waves 4-7.  K = 256 is the boundary: the
    largest pack entry, 65,280, and the last row of class 1's region (every symbol occurs, K - 1 forced in)."""
    obs = uniform(96, 9, K, seed=K)
    obs[5][3] = K - 1
    obs[2][8] = K - 1  # slot 2: class 1
    run_case(oracle, obs, 8, K, "left_to_right", layout=1, joined=True)


@pytest.mark.parametrize("N,layout", [(5, 1), (3, 0)])
def test_padding_states(oracle, N, layout):
    """N = 5: G = 8 with three padding lanes per slot, on the class-split tables.  N = 3: G = 4 stays on the row
    tables (two classes do not free its reads: tools/lds_banks.py)."""
    run_case(oracle, uniform(96, 9, 256, seed=N), N, 256, "left_to_right", layout=layout, joined=True)


def test_ragged(oracle):
    """R = 200 with lengths 1..40: masked chunks, sequences shorter than a chunk, padding slots (row 0)."""
    rng = np.random.default_rng(40)
    lens = rng.permutation(np.arange(200) % 40 + 1)
    obs = [rng.integers(0, 256, size=int(t)) for t in lens]
    run_case(oracle, obs, 8, 256, "left_to_right", layout=1, joined=True)


def _symbols_kind(kind, R, T, K):
    if kind == "uniform":
        return uniform(R, T, K, seed=T)
    if kind == "equal":  # the broadcast path: at every step all slots read one row (and add to it in both
        # histogram copies): every sequence is the same random symbol string (one constant symbol would train to
        # P = 1, where log P is rounding noise and no relative tolerance means anything)
        one = np.random.default_rng(T).integers(0, K, size=T)
        return [one.copy() for _ in range(R)]
    rng = np.random.default_rng(T)
    return [rng.choice(np.array([0, K - 1]), size=T) for _ in range(R)]


@pytest.mark.parametrize("topology", ["left_to_right", "dense"])
@pytest.mark.parametrize("kind", ["uniform", "equal", "two"])
@pytest.mark.parametrize("T", [9, 17])
def test_split_extra_waves(oracle_mt, topology, kind, T):
    """R = 10,000: the joined map with extra groups, whose idle waves run the split lower backward halves (B waves:
    the pre-sweep reads the class tables too)."""
    run_case(oracle_mt, _symbols_kind(kind, 10_000, T, 256), 8, 256, topology, layout=1, joined=True, split_extra=True)


@pytest.mark.parametrize("by", ["parity", "class"])
def test_histogram_merge(oracle, by):
    """Symbols 3 and 5 occur only in one half of the slots and 200 and 202 only in the other (by slot parity, and
    by the layout's own slot class, bit 1 of the slot index), so a symbol's histogram lives in one class's copy
    only ("class") or its two halves in different copies ("parity"): a flush that read one copy would lose them."""
    R, T = 96, 9
    rng = np.random.default_rng(11)
    obs = []
    for r in range(R):
        u = r % 8
        first = (u & 1) if by == "parity" else ((u >> 1) & 1)
        obs.append(rng.choice(np.array([3, 5] if first else [200, 202]), size=T))
    run_case(oracle, obs, 8, 256, "left_to_right", layout=1, joined=True)


def test_fallback_large_alphabet(oracle):
    """K = 300: the rows of a class no longer fit 64 KiB (nor do the row tables fit LDS): the old path, still right."""
    run_case(oracle, uniform(96, 9, 300, seed=300), 8, 300, "left_to_right", layout=0)


@pytest.mark.parametrize("R,T,topology,layout", [(10_000, 144, "left_to_right", 1), (10_000, 136, "left_to_right", 0),
                                                 (8_192, 200, "left_to_right", 0), (10_000, 200, "dense", 0)])
def test_default_policy(R, T, topology, layout):
    """With no option set the class-split tables serve the joined launch where they measured faster: left-to-right,
    more sequence groups than SIMDs, at least 144 steps per group on average (the table build costs more LDS stores
    per launch than shorter sweeps win back)."""
    from hmm_training_amd._lib import OPT_LDS_LAYOUT
    from hmm_training_amd.engine import BaumWelchEngine
    sym = np.random.default_rng(T).integers(0, 256, size=R * T).astype(np.int32)
    with BaumWelchEngine(8, 256, topology=topology) as eng:
        assert eng.get_option(OPT_LDS_LAYOUT) == -1
        eng.set_observations(offsets=np.arange(R + 1, dtype=np.int64) * T, symbols=sym)
        eng.set_params(*_params(8, 256, topology, 7))
        lm = eng.launch_map()
        assert lm["joined"] and lm["lds_layout"] == layout, lm


def test_switch(oracle_mt, monkeypatch):
    """HMMBW_OPT_LDS_LAYOUT = 0 (and the environment variable) keep the joined launch on the row tables; both
    layouts give the same results (rtol 1e-9: the histogram's atomic order differs)."""
    from hmm_training_amd._lib import OPT_LDS_LAYOUT
    from hmm_training_amd.engine import BaumWelchEngine
    obs = uniform(10_000, 17, 256, seed=1)
    new = run_case(oracle_mt, obs, 8, 256, "left_to_right", layout=1, joined=True, option=1)
    old = run_case(oracle_mt, obs, 8, 256, "left_to_right", layout=0, joined=True, option=0)
    np.testing.assert_allclose(new[0], old[0], rtol=1e-9)
    np.testing.assert_allclose(new[1], old[1], rtol=1e-9)
    for key in ("pi_num", "xi", "gamma_den_excl", "gamma_den_all", "B_num"):
        np.testing.assert_allclose(new[2][key], old[2][key], rtol=1e-9, atol=1e-300, err_msg=key)
    monkeypatch.setenv("HMMBW_LDS_LAYOUT", "0")
    with BaumWelchEngine(8, 256, topology="left_to_right") as eng:
        assert eng.get_option(OPT_LDS_LAYOUT) == 0
        eng.set_observations(obs[:96])
        eng.set_params(*_params(8, 256, "left_to_right", 7))
        assert eng.launch_map()["joined"] and eng.lds_layout == 0
        with pytest.raises(Exception):  # the observations are packed for the layout
            eng.set_option(OPT_LDS_LAYOUT, 1)
