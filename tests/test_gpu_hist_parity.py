"""The histogram parity halves of the class-split LDS tables (lds_layout.hpp: lay2_add_off, lay2_b_off) on the
GPU, against the oracle through test_gpu_lds_layout.run_case: 3 EM iterations on one context (every recorded L
is compared, so a histogram half or class that one launch left unzeroed shows in the next iteration's L), every
log P, then the complete statistics of one pass, all at that file's tolerances.  Every case asserts that the
launch is the joined one on layout 1 (but for the one dense shape that the map does not join, which asserts that).

The H entry of (class, symbol, state) is {h_even, h_odd}: sequence slot u of a wave adds gamma into half u & 1 of
its class (u >> 1) & 1, the flush sums the four pieces, and b_j(o), which the left-to-right forward needs for
pi_j b_j(o_0), comes from a compact table after the class tables.  With equal lengths sequence r sits in slot
r % 8 of wave r // 8 (G = 8), which is how the cases aim symbols at slots."""
import numpy as np
import pytest

from test_gpu_fullsize import _params
from test_gpu_lds_layout import _symbols_kind, run_case, uniform

pytestmark = pytest.mark.gpu

N, K = 8, 256
LR = "left_to_right"


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: the GPU tests need an MI355X")


def test_one_piece_per_symbol(oracle):
    """Slot u draws only from symbols 8u .. 8u + 7, so each of the four (class, half) pieces holds symbols that no
    other piece holds: a flush that drops a piece loses their B_num rows, one that counts a piece twice doubles them."""
    R, T = 96, 9
    rng = np.random.default_rng(21)
    obs = [rng.integers(8 * (r % 8), 8 * (r % 8) + 8, size=T) for r in range(R)]
    run_case(oracle, obs, N, K, LR, layout=1, joined=True)


def test_both_halves_of_one_entry(oracle):
    """Every sequence the same random string: at every step the two slots of an add group add to the two halves
    of one H entry, and every piece of that symbol's row is in use."""
    run_case(oracle, _symbols_kind("equal", 96, 9, K), N, K, LR, layout=1, joined=True)


@pytest.mark.parametrize("first", [0, K - 1])
def test_b00_source(oracle, first):
    """pi_j b_j(o_0) reads the b table: its first and last rows (o_0 = 0, K - 1), with a starting pi that has mass
    on every state so that the entries of the states j > 0 matter to log P and pi_num."""
    obs = uniform(96, 9, K, seed=first + 3)
    for o in obs:
        o[0] = first
    rng = np.random.default_rng(5)
    _, A, B = _params(N, K, LR, 7)
    pi = rng.dirichlet(np.full(N, 4.0))
    assert pi.min() > 0
    run_case(oracle, obs, N, K, LR, layout=1, joined=True, params=(pi, A, B))


def test_padding_lanes(oracle):
    """N = 5 (G = 8): the pad columns of the b table and of both halves stay zero and harmless."""
    run_case(oracle, uniform(96, 9, K, seed=55), 5, K, LR, layout=1, joined=True)


def test_ragged_lengths(oracle):
    """Lengths 1..40, R = 200: masked steps and padding slots add zeros into their own half (of row 0)."""
    rng = np.random.default_rng(41)
    lens = rng.permutation(np.arange(200) % 40 + 1)
    obs = [rng.integers(0, K, size=int(t)) for t in lens]
    run_case(oracle, obs, N, K, LR, layout=1, joined=True)


@pytest.mark.parametrize("kind", ["uniform", "two"])
@pytest.mark.parametrize("T", [9, 17])
def test_split_extra_groups(oracle_mt, kind, T):
    """R = 10,000: the A and B waves of the split extra groups add with the parity offset too."""
    run_case(oracle_mt, _symbols_kind(kind, 10_000, T, K), N, K, LR, layout=1, joined=True, split_extra=True)


@pytest.mark.parametrize("R", [8_200, 10_000])
def test_dense_forced_on(oracle_mt, R):
    """Dense with the layout forced on: b comes from the P entry, the adds and the flush are the new ones.  The
    dense E-step joins only where the map has extra groups (obs_plan.hpp, joined): R = 8,200 is the smallest such
    shape on 256 CUs (one extra group beyond 1,024 full waves), R = 10,000 the headline's count."""
    run_case(oracle_mt, uniform(R, 9, K, seed=R), N, K, "dense", layout=1, joined=True)


def test_dense_forced_on_without_extra_groups(oracle):
    """R = 96, dense, option 1: without extra groups the dense E-step is not the joined launch, so the option has
    nothing to act on and the launch reports the row tables (HMMBW_INFO_LDS_LAYOUT = 0); the results must not
    care that the context was asked for the layout (its packs and b table are then never built)."""
    run_case(oracle, uniform(96, 9, K, seed=96), N, K, "dense", layout=0, joined=False)
