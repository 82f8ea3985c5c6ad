"""Grouped launches (hmmbw_group_*, k_estep_small_group) at the shapes real use gives them: members of unequal
size, a member on the spread map, a member of more than 512 workgroups, per-member options, enqueues that span and
wrap the argument slabs, a score between two enqueues, members whose observations or topology change under the
group, a member without sequences, and the Python layers that are meant to group.

One contract throughout (include/hmmbw.h): a member of a group ends "exactly as if trained alone".  Every member is
compared with the oracle (oracle.hmm_training, oracle.forward_loglik) on its own data: the reference trains word by
word (HMM/main.py:147-152) and scores pair by pair (HMM/hmm_testing.py:139-161).  Tolerances as test_gpu_parity.py /
test_gpu_fuzz.py: parameters 1e-6 relative + 1e-15 absolute, L and log P 1e-9 relative with -inf matched exactly,
per-sequence log P also 1e-12 absolute (K = 1 makes log P zero; L of a member that holds one sequence is such a
log P, see l_atol), iteration counts and stop flags exact, no NaN.

Every case first asserts, from BaumWelchEngine.launch_map() and the member sizes, that it reaches the path it names
(slice lengths in workgroups, spread map, > 512 workgroups, number of grouped launches, a pending M-step), and prints
those facts; the CU count comes from the device."""
import contextlib
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PARAM_RTOL, PARAM_ATOL, LL_RTOL, LOGP_ATOL = 1e-6, 1e-15, 1e-9, 1e-12
WPB = 4  # waves of an E-step workgroup (kBlock / kWave, obs_plan.hpp)


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: the GPU tests need an MI355X")


def ncus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def lane_group(N):
    return 2 if N <= 2 else 4 if N <= 4 else 8 if N <= 8 else 16


# ------------------------------------------------------------------------------------------------ comparisons
def margin(err, tol):
    """(worst err - tol, worst err / tol): <= 0 and <= 1 within tolerance."""
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err > 0, err / tol, 0.0)
    return float((err - tol).max()), float(ratio.max())


def params_excess(mine, ref, what):
    """Parameters against 1e-6 |ref| + 1e-15: the worst excess over that bound and the worst error as a fraction
    of it."""
    mine, ref = np.asarray(mine, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert mine.shape == ref.shape, what
    assert not np.any(np.isnan(mine)), f"{what}: NaN"
    worst = margin(np.abs(mine - ref), PARAM_RTOL * np.abs(ref) + PARAM_ATOL)
    assert worst[0] <= 0, f"{what}: worst excess {worst[0]:.3e}"
    return worst


def ll_excess(mine, ref, what, atol=0.0):
    """L traces and log P: -inf where the oracle has -inf and nowhere else, the rest within 1e-9 relative (+ atol);
    the worst excess over that bound and the worst error as a fraction of it."""
    mine, ref = np.asarray(mine, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert mine.shape == ref.shape, f"{what}: {mine.shape} against {ref.shape}"
    assert not np.any(np.isnan(mine)), f"{what}: NaN"
    inf = np.isneginf(ref)
    assert np.all(np.isfinite(ref[~inf])), f"{what}: the oracle's own value is not finite"
    assert np.array_equal(np.isneginf(mine), inf), f"{what}: -inf in other places than the oracle's"
    if not np.any(~inf):
        return -np.inf, 0.0
    worst = margin(np.abs(mine[~inf] - ref[~inf]), LL_RTOL * np.abs(ref[~inf]) + atol)
    assert worst[0] <= 0, f"{what}: worst excess {worst[0]:.3e}"
    return worst


class Worst:
    """Per quantity, over everything a test compared: the worst excess over tolerance (negative: the margin left) and
    the worst error as a fraction of its tolerance; printed at the test's end."""

    def __init__(self):
        self.w = {}

    def add(self, key, v):
        old = self.w.get(key, (-np.inf, 0.0))
        self.w[key] = (max(old[0], v[0]), max(old[1], v[1]))

    def __str__(self):
        return ", ".join(f"{k} {e:+.3e} ({r:.2e} of tol)" for k, (e, r) in self.w.items())


# ------------------------------------------------------------------------------------------------ members
class Member:
    def __init__(self, name, obs, pi, A, B, **opts):
        self.name, self.obs, self.pi, self.A, self.B, self.opts = name, obs, pi, A, B, opts
        self.off = np.concatenate([[0], np.cumsum([len(o) for o in obs])]).astype(np.int64)
        self.sym = (np.concatenate(obs) if len(obs) else np.zeros(0)).astype(np.int64)

    def train_ref(self, oracle, N, K, eps, maxit, start=None):
        pi, A, B = start if start is not None else (self.pi, self.A, self.B)
        return oracle.hmm_training(self.off, self.sym, N, K, eps, maxit, pi, A, B)

    def score_ref(self, oracle, N, K, start=None):
        pi, A, B = start if start is not None else (self.pi, self.A, self.B)
        return oracle.forward_loglik(self.off, self.sym, N, K, pi, A, B)

    def engine(self, N, K, dense):
        from hmm_training_amd.engine import BaumWelchEngine
        e = BaumWelchEngine(N, K, device=0, topology="dense" if dense else "left_to_right", **self.opts)
        e.set_observations(self.obs)
        e.set_params(self.pi, self.A, self.B)
        return e


def model(rng, N, K, dense):
    """A random warm start without zero entries in B: dense (pi, A), or a left-to-right chain."""
    B = rng.dirichlet(np.full(K, 0.7), size=N) if K > 1 else np.ones((N, 1))
    B = np.maximum(B, 1e-6)
    B /= B.sum(1, keepdims=True)
    if dense:
        return rng.dirichlet(np.ones(N)), rng.dirichlet(np.ones(N), size=N), B
    A = np.zeros((N, N))
    for j in range(N):
        A[j, j] = rng.uniform(0.3, 0.9) if j + 1 < N else 1.0
        if j + 1 < N:
            A[j, j + 1] = 1.0 - A[j, j]
    pi = np.full(N, 0.2 / max(N - 1, 1))
    pi[0] = 0.8 if N > 1 else 1.0
    return pi, A, B


def ragged(rng, R, K, tmax, tmin=1):
    """R sequences over [0, K), lengths uniform in [tmin, tmax] with both ends present when R >= 2."""
    T = rng.integers(tmin, tmax + 1, size=R)
    T[0] = tmax
    if R > 1:
        T[-1] = tmin
    return [rng.integers(0, K, size=int(t)) for t in T]


def member(rng, name, N, K, dense, R, tmax=10, zero=False, **opts):
    """A member of R ragged sequences (T = 1 .. tmax).  zero: its sequence 1 (or its only one) has probability zero.
    K >= 2: the last symbol has b_j = 0 in every state and only that sequence carries it.  K = 1 (every sequence of
    one length has the same probability): A moves strictly upwards (no self-loops, last row zero), so A^N = 0, the
    sequences have T <= N and that one T = N + 1."""
    pi, A, B = model(rng, N, K, dense)
    if not zero:
        return Member(name, ragged(rng, R, K, tmax), pi, A, B, **opts)
    z = min(1, R - 1)
    if K >= 2:
        B[:, K - 1] = 0.0
        B /= B.sum(1, keepdims=True)
        obs = ragged(rng, R, K - 1, tmax)
        obs[z][-1] = K - 1
    else:
        A = np.triu(rng.uniform(0.2, 1.0, size=(N, N)), 1) if dense else np.diag(np.ones(N - 1), 1)
        s = A.sum(1, keepdims=True)
        A = np.divide(A, s, out=np.zeros_like(A), where=s > 0)
        obs = ragged(rng, R, K, N)
        obs[z] = np.zeros(N + 1, dtype=np.int64)
    m = Member(name, obs, pi, A, B, **opts)
    m.zero_seq = z
    return m


def l_atol(m):
    """L = LSE_r log P_r of a member that holds ONE sequence is that sequence's log P, so it takes the per-sequence
    bound: with K = 1 it is log 1 = 0 up to rounding (~1e-15), where a relative tolerance means nothing.  Every
    other member's L is compared at 1e-9 relative alone."""
    return LOGP_ATOL if len(m.obs) == 1 else 0.0


def check_member(W, e, m, ref, st, trace, tag):
    """Member m's engine e after training against its oracle run ref: count, flags, L, log P, parameters."""
    assert st.iterations == ref.iterations, f"{tag}: iterations"
    assert st.done == 1, f"{tag}: done"
    W.add("L", ll_excess(trace, ref.trace_L, f"{tag} L", l_atol(m)))
    W.add("logP", ll_excess(e.loglik(), ref.logP, f"{tag} log P", LOGP_ATOL))
    p2, A2, B2 = e.params(normalise=True)
    W.add("A", params_excess(A2, ref.A, f"{tag} A"))
    W.add("B", params_excess(B2, ref.B, f"{tag} B"))
    W.add("pi", params_excess(p2, ref.pi, f"{tag} pi"))


def trace_of(e, n):
    """Status and L of the first n iterations (of those made, if fewer: the caller compares the count)."""
    st, recs = e.status(0, min(n, e.status()[0].iterations))
    return st, [L for L, _ in recs]


def slices(engines):
    return [e.launch_map()["workgroups"] for e in engines]


# ------------------------------------------------------------------------------------------------ 1. unequal slices
# (N, K, dense): every lane-group width G = 2, 4, 8, 16 at an N below G and (but G = 4) at N = G, both topologies,
# K at the LDS-table limit of the width (K G 16 B = 32 KiB), a small K that is no power of two, and K = 1
SHAPES = [(1, 1, False), (1, 1024, True), (2, 7, True), (2, 1024, False),
          (3, 512, False), (3, 5, True),
          (5, 1, True), (5, 256, False), (7, 13, False), (7, 256, True), (8, 256, False), (8, 256, True), (8, 11, True),
          (9, 128, True), (9, 6, False), (12, 128, False), (12, 1, True), (16, 128, True), (16, 128, False),
          (16, 11, False)]
# member order -> where the largest slice sits
ORDERS = {"largest first": ["big", "single", "mid", "two", "part"],
          "largest last": ["single", "mid", "two", "part", "big"],
          "largest between two one-workgroup members": ["mid", "single", "big", "part", "two"]}
WANT = {"big": 7, "mid": 3, "two": 2, "part": 1, "single": 1}


@pytest.mark.parametrize("N,K,dense", SHAPES)
def test_unequal_slices_train_and_score(oracle, N, K, dense):
    """Five members with slices of 7, 3, 2, 1 and 1 workgroups, in three orders: scored before training and trained
    4 iterations in one group, every member against its own oracle run (computed once, shared by the orders).
    `big` and `part` end in a partly filled wave, `single` holds one sequence, `mid` holds a sequence of probability
    zero (checked on the oracle first)."""
    from hmm_training_amd.engine import EngineGroup
    G = lane_group(N)
    U = 64 // G        # sequences per wave
    S = WPB * U        # ... per workgroup
    rng = np.random.default_rng(1000 * N + K + int(dense))
    assert K * G * 16 <= 32768
    R = {"big": 6 * S + U + 1, "mid": 2 * S + 3 * U, "two": S + 1, "part": U + max(1, U // 2), "single": 1}
    assert R["big"] % U and R["part"] % U, "the last wave of big and part is partly filled"
    mem = {k: member(rng, k, N, K, dense, R[k], zero=(k == "mid")) for k in R}
    # 4 iterations: launch e adds into statistics buffer e % 3 and clears the next one over its slice, so the fourth
    # launch is the first to add into a buffer that a grouped launch has cleared
    maxit, eps = 4, 1e-6
    sref = {k: m.score_ref(oracle, N, K) for k, m in mem.items()}
    tref = {k: m.train_ref(oracle, N, K, eps, maxit) for k, m in mem.items()}
    z = mem["mid"].zero_seq
    assert np.isneginf(sref["mid"][z]) and np.isneginf(sref["mid"]).sum() == 1, "the oracle's log P of the zero sequence"
    assert all(np.all(np.isfinite(sref[k])) for k in R if k != "mid")
    W = Worst()
    for order, names in ORDERS.items():
        engines = [mem[k].engine(N, K, dense) for k in names]
        try:
            maps = [e.launch_map() for e in engines]
            got = [lm["workgroups"] for lm in maps]
            print(f"N={N} K={K} {'dense' if dense else 'lr'} G={G} | {order}: slices {got} workgroups, "
                  f"sequences {[R[k] for k in names]}, waves {[lm['waves'] for lm in maps]}")
            assert got == [WANT[k] for k in names]
            assert all(lm["full_workgroups"] == lm["workgroups"] for lm in maps), "no member on the spread map here"
            assert all(e.topology == ("dense" if dense else "left_to_right") for e in engines)
            with EngineGroup(engines) as grp:
                cols = grp.score()
                for e in engines:
                    e.reset(eps, maxit)
                # one call and no query in between: every M-step but the last runs in the next launch's prologue
                # (a status query would run it as its own kernel, which clears the statistics itself), and the
                # launches past a member's own stop are no-ops for it
                grp.enqueue_iterations(maxit)
            for i, k in enumerate(names):
                tag = f"{order}, member {i} ({k})"
                W.add("score", ll_excess(cols[i], sref[k], f"{tag} score", LOGP_ATOL))
                st, trace = trace_of(engines[i], tref[k].iterations)
                assert st.converged == int(tref[k].iterations < maxit), f"{tag}: converged"
                check_member(W, engines[i], mem[k], tref[k], st, trace, tag)
        finally:
            for e in engines:
                e.close()
    print(f"worst excess over tolerance: {W}")


# ------------------------------------------------------------------------------------------------ 2. the spread map
@pytest.mark.parametrize("dense,tlo,thi", [(True, 1, 6), (False, 1, 6), (True, 12, 12)],
                         ids=["dense", "left_to_right", "dense_split_halves"])
def test_member_on_the_spread_map(oracle, dense, tlo, thi):
    """N = 8: a member with 38 more sequence-group waves than the device has SIMDs, between two one-workgroup
    members.  In a group its plan is made with allow_join = false, so it runs the unjoined spread map: extra
    workgroups of xact active waves past the full ones (bid >= nfull), dense with the split extra waves switched on.
    Two grouped iterations and a grouped score against the oracle; the same member alone (for left-to-right: the
    joined map) against the oracle too.  No bitwise comparison of the two: the sums are floating-point atomics.
    T = 1 .. 6 never splits a group's backward (one chunk of 8 steps); the third case, equal T = 12, is the one in
    which the extra workgroups' B partner waves really take the lower half."""
    from hmm_training_amd.engine import EngineGroup
    N, K, U = 8, 64, 8
    ncu = ncus()
    rng = np.random.default_rng(77 + int(dense) + thi)
    Rbig = U * (WPB * ncu + 38) - 5  # the last wave partly filled
    pi, A, B = model(rng, N, K, dense)
    big = Member("big", ragged(rng, Rbig, K, thi, tlo), pi, A, B)
    mem = [member(rng, "left", N, K, dense, 5, tmax=6), big, member(rng, "right", N, K, dense, 20, tmax=6)]
    maxit, eps = 2, 1e-6
    W = Worst()
    engines = [m.engine(N, K, dense) for m in mem]
    lone = big.engine(N, K, dense)
    try:
        lm = engines[1].launch_map()
        print(f"{ncu} CUs; slices {slices(engines)} workgroups; big member: {Rbig} sequences, {lm}; alone: "
              f"joined={lone.launch_map()['joined']}")
        assert lm["waves"] > WPB * ncu
        assert lm["workgroups"] > lm["full_workgroups"], "the large member must be on the spread map"
        if dense:
            assert lm["split_extra"], "dense: the split extra waves must be on"
        assert slices(engines)[0] == 1 and slices(engines)[2] == 1
        with EngineGroup(engines) as grp:
            cols = grp.score()
            for e in engines:
                e.reset(eps, maxit)
            grp.enqueue_iterations(maxit)
            for i, m in enumerate(mem):
                ref = m.train_ref(oracle, N, K, eps, maxit)
                W.add("score", ll_excess(cols[i], m.score_ref(oracle, N, K), f"member {i} score", LOGP_ATOL))
                st, trace = trace_of(engines[i], ref.iterations)
                check_member(W, engines[i], m, ref, st, trace, f"member {i} ({m.name})")
                if m is big:
                    lone.reset(eps, maxit)
                    lone.enqueue_iterations(maxit)
                    st, trace = trace_of(lone, ref.iterations)
                    check_member(W, lone, m, ref, st, trace, "big member alone")
    finally:
        for e in engines + [lone]:
            e.close()
    print(f"worst excess over tolerance: {W}")


# ------------------------------------------------------------------------------------------------ 3. > 512 workgroups
@pytest.mark.parametrize("dense", [True, False], ids=["dense", "left_to_right"])
def test_member_of_more_than_512_workgroups(oracle, dense):
    """merged_mstep (hmmbw_device.hpp) holds PB = 2 log-likelihood pairs per thread in registers, PB * BLK = 2 * 256
    = 512 pairs per workgroup of a grouped launch, and folds the pairs past them in a separate loop.  A member of
    N = 16 (4 sequences per wave, 16 per workgroup) with 8,213 sequences writes 514 pairs; it trains two merged
    iterations beside two small members.  The only grouped check of that loop: L of every iteration and the
    returned parameters against the oracle."""
    from hmm_training_amd._lib import OPT_MERGE_MSTEP
    from hmm_training_amd.engine import EngineGroup
    N, K = 16, 32
    rng = np.random.default_rng(512 + int(dense))
    pi, A, B = model(rng, N, K, dense)
    big = Member("big", ragged(rng, 16 * 513 + 5, K, 4), pi, A, B)
    mem = [member(rng, "left", N, K, dense, 3, tmax=4), big, member(rng, "right", N, K, dense, 21, tmax=4)]
    maxit, eps = 2, 0.0
    W = Worst()
    engines = [m.engine(N, K, dense) for m in mem]
    try:
        print(f"{ncus()} CUs; slices {slices(engines)} workgroups; big member: {engines[1].launch_map()}")
        assert slices(engines)[1] > 512, "the large member must write more than PB * BLK = 512 pairs"
        assert slices(engines)[0] == 1 and slices(engines)[2] == 2
        assert all(e.get_option(OPT_MERGE_MSTEP) == 1 for e in engines)
        with EngineGroup(engines) as grp:
            for e in engines:
                e.reset(eps, maxit)
            grp.enqueue_iterations(maxit)
            # the second launch ran the first iteration's M-step in its prologue; the second M-step is pending
            assert all(e.wait_status(e.post_status())[0].iterations == maxit - 1 for e in engines)
            for i, m in enumerate(mem):
                ref = m.train_ref(oracle, N, K, eps, maxit)
                assert ref.iterations == maxit
                st, trace = trace_of(engines[i], maxit)
                assert st.converged == 0
                check_member(W, engines[i], m, ref, st, trace, f"member {i} ({m.name})")
    finally:
        for e in engines:
            e.close()
    print(f"worst excess over tolerance: {W}")


# ------------------------------------------------------------------------------------------------ 4. per-member options
@pytest.mark.parametrize("dense", [True, False], ids=["dense", "left_to_right"])
@pytest.mark.parametrize("merge", ["mixed", "none"])
def test_options_differ_between_members(oracle, dense, merge):
    """stat_copies 1, 2, 3, safe_scaling on and off, and merge_mstep on for some members only (`mixed`) or for none:
    hmmbw_group_iterate then goes one launch at a time, with the separate M-step kernels of the members that cannot
    merge between two grouped launches.  Unequal slices (2, 1, 3, 2, 1 workgroups)."""
    from hmm_training_amd._lib import OPT_MERGE_MSTEP, OPT_SAFE_SCALING, OPT_STAT_COPIES
    from hmm_training_amd.engine import EngineGroup
    N, K = 8, 64
    rng = np.random.default_rng(40 + int(dense))
    spec = [(40, 1, False, True), (7, 2, True, False), (70, 3, False, False), (33, 3, True, True), (1, 1, True, False)]
    mem = [member(rng, f"m{i}", N, K, dense, R, stat_copies=c, safe_scaling=s, merge_mstep=(mg and merge == "mixed"))
           for i, (R, c, s, mg) in enumerate(spec)]
    maxit, eps = 4, 1e-6  # 4: the fourth launch adds into a statistics buffer that the third cleared
    W = Worst()
    engines = [m.engine(N, K, dense) for m in mem]
    try:
        opts = [(e.get_option(OPT_STAT_COPIES), e.get_option(OPT_SAFE_SCALING), e.get_option(OPT_MERGE_MSTEP))
                for e in engines]
        print(f"slices {slices(engines)} workgroups; (stat_copies, safe_scaling, merge_mstep) {opts}")
        assert slices(engines) == [2, 1, 3, 2, 1]
        assert opts == [(c, int(s), int(mg and merge == "mixed")) for _, c, s, mg in spec]
        assert {o[2] for o in opts} == ({0, 1} if merge == "mixed" else {0})
        with EngineGroup(engines) as grp:
            cols = grp.score()
            for e in engines:
                e.reset(eps, maxit)
            grp.enqueue_iterations(maxit)  # one call: the members that merge keep their M-steps in the prologues
        for i, m in enumerate(mem):
            ref = m.train_ref(oracle, N, K, eps, maxit)
            W.add("score", ll_excess(cols[i], m.score_ref(oracle, N, K), f"member {i} score", LOGP_ATOL))
            st, trace = trace_of(engines[i], ref.iterations)
            check_member(W, engines[i], m, ref, st, trace, f"member {i} {opts[i]}")
    finally:
        for e in engines:
            e.close()
    print(f"worst excess over tolerance: {W}")


# ------------------------------------------------------------------------------------------------ 5. argument slabs
def tiny_members(dense, seed):
    """N = 3, K = 8: members of 3, 4 and 5 sequences of T <= 10."""
    rng = np.random.default_rng(seed)
    return [member(rng, f"m{i}", 3, 8, dense, R) for i, R in enumerate([3, 4, 5])]


@pytest.mark.parametrize("dense,seed", [(True, 5), (False, 6)], ids=["dense", "left_to_right"])
def test_one_enqueue_spans_three_argument_slabs(oracle, dense, seed):
    """enqueue_iterations(130) in one call: hmmbw_group_iterate fills an argument slab per kBatch = 64 launches, so
    64 + 64 + 2.  Epsilon 0 keeps every member running to max_iterations = 130; all 130 values of L and the final
    parameters against the oracle, whose own trace is checked to be finite first."""
    from hmm_training_amd.engine import EngineGroup
    N, K, n = 3, 8, 130
    mem = tiny_members(dense, seed)
    refs = [m.train_ref(oracle, N, K, 0.0, n) for m in mem]
    for r in refs:
        assert r.iterations == n and np.all(np.isfinite(r.trace_L)), "pick a seed with a finite oracle trace"
    W = Worst()
    engines = [m.engine(N, K, dense) for m in mem]
    try:
        print(f"slices {slices(engines)} workgroups, sequences {[e.n_seq for e in engines]}")
        assert slices(engines) == [1, 1, 1] and len({e.n_seq for e in engines}) == 3
        with EngineGroup(engines) as grp:
            for e in engines:
                e.reset(0.0, n)
            grp.timing(1)
            grp.enqueue_iterations(n)
            _, launches = grp.timing(0)
            print(f"{launches} grouped launches from one call (64 per argument slab)")
            assert launches == n > 2 * 64
            for i, m in enumerate(mem):
                st, trace = trace_of(engines[i], n)
                assert st.converged == 0
                check_member(W, engines[i], m, refs[i], st, trace, f"member {i}")
    finally:
        for e in engines:
            e.close()
    print(f"worst excess over tolerance: {W}")


@pytest.mark.parametrize("dense,seed", [(True, 5), (False, 6)], ids=["dense", "left_to_right"])
def test_back_to_back_enqueues_wrap_the_slab_ring(oracle, dense, seed):
    """Seven enqueue_iterations(1) calls with no query between them: each takes the next of the group's four argument
    slabs, so the ring wraps and a slab is refilled while earlier launches may still be queued."""
    from hmm_training_amd.engine import EngineGroup
    N, K, n = 3, 8, 7
    mem = tiny_members(dense, seed)
    refs = [m.train_ref(oracle, N, K, 0.0, n) for m in mem]
    for r in refs:
        assert r.iterations == n and np.all(np.isfinite(r.trace_L))
    W = Worst()
    engines = [m.engine(N, K, dense) for m in mem]
    try:
        print(f"slices {slices(engines)} workgroups, sequences {[e.n_seq for e in engines]}")
        assert slices(engines) == [1, 1, 1] and len({e.n_seq for e in engines}) == 3
        with EngineGroup(engines) as grp:
            for e in engines:
                e.reset(0.0, n)
            grp.timing(1)
            for _ in range(n):
                grp.enqueue_iterations(1)
            _, launches = grp.timing(0)
            print(f"{launches} one-launch calls over a ring of 4 slabs")
            assert launches == n > 4
            for i, m in enumerate(mem):
                st, trace = trace_of(engines[i], n)
                check_member(W, engines[i], m, refs[i], st, trace, f"member {i}")
    finally:
        for e in engines:
            e.close()
    print(f"worst excess over tolerance: {W}")


# ------------------------------------------------------------------------------------------------ 6. score mid-way
@pytest.mark.parametrize("dense", [True, False], ids=["dense", "left_to_right"])
def test_score_between_two_enqueues(oracle, dense):
    """Two iterations, grp.score(), three more.  The score flushes every member's pending M-step (the second
    iteration's, which the third launch would have run in its prologue): the working parameters at the score are
    the oracle's after two iterations, the scores are the oracle's forward log P under them, and the run still ends
    where the oracle's five iterations end."""
    from hmm_training_amd.engine import EngineGroup
    N, K, n1, n = 8, 32, 2, 5
    rng = np.random.default_rng(60 + int(dense))
    mem = [member(rng, f"m{i}", N, K, dense, R) for i, R in enumerate([40, 7, 1])]
    W = Worst()
    engines = [m.engine(N, K, dense) for m in mem]
    try:
        print(f"slices {slices(engines)} workgroups")
        assert slices(engines) == [2, 1, 1]
        with EngineGroup(engines) as grp:
            for e in engines:
                e.reset(0.0, n)
            grp.enqueue_iterations(n1)
            recorded = [e.wait_status(e.post_status())[0].iterations for e in engines]
            print(f"iterations recorded before the score: {recorded} of {n1} enqueued (an M-step is pending)")
            assert recorded == [n1 - 1] * len(mem)
            cols = grp.score()
            for i, m in enumerate(mem):
                mid = m.train_ref(oracle, N, K, 0.0, n1)
                with np.errstate(under="ignore"):
                    work = np.exp(mid.log_pi), np.exp(mid.log_A), np.exp(mid.log_B)
                st, trace = trace_of(engines[i], n1)
                assert st.iterations == n1 and st.done == 0
                W.add("L", ll_excess(trace, mid.trace_L, f"member {i} L at the score", l_atol(m)))
                p, A, B = engines[i].params(normalise=False)
                W.add("pi", params_excess(p, work[0], f"member {i} working pi at the score"))
                W.add("A", params_excess(A, work[1], f"member {i} working A at the score"))
                W.add("B", params_excess(B, work[2], f"member {i} working B at the score"))
                W.add("score", ll_excess(cols[i], m.score_ref(oracle, N, K, work), f"member {i} score", LOGP_ATOL))
            grp.enqueue_iterations(n - n1)
            for i, m in enumerate(mem):
                ref = m.train_ref(oracle, N, K, 0.0, n)
                st, trace = trace_of(engines[i], n)
                check_member(W, engines[i], m, ref, st, trace, f"member {i} at the end")
    finally:
        for e in engines:
            e.close()
    print(f"worst excess over tolerance: {W}")


# ------------------------------------------------------------------------------------------------ 7. members that change
def test_member_gets_new_observations_under_the_group(oracle):
    """After one grouped run, member 1 gets a larger observation set (1 -> 4 workgroups) and fresh parameters; the
    others keep their data and go on from their working parameters.  The same group object then runs again: every
    member against the oracle on its current data and start."""
    from hmm_training_amd.engine import EngineGroup
    N, K, dense, n = 8, 32, False, 2
    rng = np.random.default_rng(70)
    mem = [member(rng, f"m{i}", N, K, dense, R) for i, R in enumerate([40, 9, 20])]
    W = Worst()
    engines = [m.engine(N, K, dense) for m in mem]
    try:
        with EngineGroup(engines) as grp:
            before = slices(engines)
            for e in engines:
                e.reset(0.0, n)
            grp.enqueue_iterations(n)
            for i, m in enumerate(mem):
                st, trace = trace_of(engines[i], n)
                check_member(W, engines[i], m, m.train_ref(oracle, N, K, 0.0, n), st, trace, f"run 1, member {i}")
            starts = [e.params(normalise=False) for e in engines]
            mem[1] = member(rng, "m1 again", N, K, dense, 3 * 32 + 11)
            engines[1].set_observations(mem[1].obs)
            engines[1].set_params(mem[1].pi, mem[1].A, mem[1].B)
            starts[1] = (mem[1].pi, mem[1].A, mem[1].B)
            print(f"slices {before} -> {slices(engines)} workgroups")
            assert before == [2, 1, 1] and slices(engines) == [2, 4, 1]
            for e in engines:
                e.reset(0.0, n)
            grp.enqueue_iterations(n)
            refs = [m.train_ref(oracle, N, K, 0.0, n, starts[i]) for i, m in enumerate(mem)]
            for i, m in enumerate(mem):
                st, trace = trace_of(engines[i], n)
                check_member(W, engines[i], m, refs[i], st, trace, f"run 2, member {i}")
            cols = grp.score()  # after the checks: it overwrites the last E-step's log P
            for i, m in enumerate(mem):
                with np.errstate(under="ignore"):
                    work = np.exp(refs[i].log_pi), np.exp(refs[i].log_A), np.exp(refs[i].log_B)
                W.add("score", ll_excess(cols[i], m.score_ref(oracle, N, K, work), f"run 2, member {i} score", LOGP_ATOL))
    finally:
        for e in engines:
            e.close()
    print(f"worst excess over tolerance: {W}")


def test_member_that_no_longer_fits_is_refused_and_nothing_changes(oracle):
    """topology="auto": one member of three left-to-right ones gets a dense A.  hmmbw_group_iterate and
    hmmbw_group_score must refuse (HMMBW_E_UNSUPPORTED) before they touch any member: the others' working
    parameters, log P and status are byte-identical before and after."""
    from hmm_training_amd._lib import HMMBW_E_UNSUPPORTED, HMMBWError
    from hmm_training_amd.engine import BaumWelchEngine, EngineGroup
    N, K, n = 8, 32, 2
    rng = np.random.default_rng(71)
    mem = [member(rng, f"m{i}", N, K, False, R) for i, R in enumerate([40, 9, 20])]
    engines = []
    for m in mem:
        e = BaumWelchEngine(N, K, device=0, topology="auto")
        e.set_observations(m.obs)
        e.set_params(m.pi, m.A, m.B)
        engines.append(e)

    def state(e):
        return tuple(x.tobytes() for x in e.params(normalise=False)) + (e.loglik().tobytes(), bytes(e.status()[0]))

    try:
        print(f"slices {slices(engines)} workgroups")
        assert slices(engines) == [2, 1, 1] and [e.topology for e in engines] == ["left_to_right"] * 3
        with EngineGroup(engines) as grp:
            for e in engines:
                e.reset(0.0, 2 * n)
            grp.enqueue_iterations(n)
            for which in (1, 0):  # a middle member, then the one the others are compared with
                keep = mem[which]
                engines[which].set_params(*model(rng, N, K, True))
                assert engines[which].topology == "dense"
                others = [e for i, e in enumerate(engines) if i != which]
                before = [state(e) for e in others]
                for call in (lambda: grp.enqueue_iterations(1), grp.score):
                    with pytest.raises(HMMBWError) as err:
                        call()
                    assert err.value.code == HMMBW_E_UNSUPPORTED
                assert [state(e) for e in others] == before
                engines[which].set_params(keep.pi, keep.A, keep.B)
            # the group works again once every member fits: member 2 goes on to the oracle's 2 n iterations
            grp.enqueue_iterations(n)
            ref = mem[2].train_ref(oracle, N, K, 0.0, 2 * n)
            st, trace = trace_of(engines[2], 2 * n)
            check_member(Worst(), engines[2], mem[2], ref, st, trace, "member 2 after the refusals")
    finally:
        for e in engines:
            e.close()


# ------------------------------------------------------------------------------------------------ 8. no sequences
@pytest.mark.parametrize("where", [0, 1, 2])
def test_member_without_sequences(oracle, where):
    """A member with set_observations([]) contributes no workgroup (start[m] == start[m + 1]) and cannot merge its
    M-step, so the group iterates one launch at a time.  It does exactly what the same engine does alone with
    enqueue_iterations(k) (the same status fields and parameters, bit for bit); its score is an empty array.  The
    other members match the oracle."""
    from hmm_training_amd.engine import BaumWelchEngine, EngineGroup
    N, K, dense, k = 8, 16, False, 3
    rng = np.random.default_rng(80 + where)
    mem = [member(rng, f"m{i}", N, K, dense, R) for i, R in enumerate([40, 5, 33])]
    mem[where] = Member("empty", [], *model(rng, N, K, dense))
    W = Worst()
    engines = [m.engine(N, K, dense) for m in mem]
    lone = mem[where].engine(N, K, dense)

    def state(e):
        return (tuple(x.tobytes() for x in e.params(normalise=False)) + tuple(x.tobytes() for x in e.params()) +
                (bytes(e.status()[0]),))

    try:
        lone.reset(1e-6, k)
        lone.enqueue_iterations(k)
        st = lone.status()[0]
        print(f"slices {slices(engines)} workgroups; an empty engine alone after {k} iterations: iterations "
              f"{st.iterations}, done {st.done}, converged {st.converged}, L {st.last_log_likelihood}, diff {st.last_diff}")
        assert slices(engines)[where] == 0 and engines[where].n_seq == 0
        assert st.iterations == k and st.done == 1 and st.converged == 0 and st.last_log_likelihood == -np.inf
        with EngineGroup(engines) as grp:
            cols = grp.score()
            assert cols[where].shape == (0,)
            for e in engines:
                e.reset(1e-6, k)
            grp.enqueue_iterations(k)
            assert state(engines[where]) == state(lone)
            assert engines[where].loglik().shape == (0,)
            for i, m in enumerate(mem):
                if i == where:
                    continue
                ref = m.train_ref(oracle, N, K, 1e-6, k)
                W.add("score", ll_excess(cols[i], m.score_ref(oracle, N, K), f"member {i} score", LOGP_ATOL))
                st, trace = trace_of(engines[i], ref.iterations)
                check_member(W, engines[i], m, ref, st, trace, f"member {i}")
    finally:
        for e in engines + [lone]:
            e.close()
    print(f"worst excess over tolerance: {W}")


# ------------------------------------------------------------------------------------------------ 9. the Python layers
def test_hmm_training_group_trains_all_words_in_one_group(tmp_path, monkeypatch):
    """Word sets of 3, 40 and 11 recordings (1, 2 and 1 workgroups at N = 8): the parameters and printed lines of
    hmm_training word by word, and one EngineGroup.train call over all three engines (not the one-by-one fallback)."""
    from hmm_training_amd.engine import EngineGroup
    from hmm_training_amd.hmm_training import hmm_training, hmm_training_group
    monkeypatch.chdir(tmp_path)
    N, K = 8, 32
    rng = np.random.default_rng(90)
    sets = [ragged(rng, R, K, 30, 5) for R in (3, 40, 11)]
    names = ["up", "down", "left"]
    out_seq, res_seq = io.StringIO(), []
    with contextlib.redirect_stdout(out_seq):
        for obs, name in zip(sets, names):
            res_seq.append(hmm_training(obs, N=N, M=K, max_iterations=12, word_name=name, device=0))
    calls, wgs = [], []
    train = EngineGroup.train

    def spy(self, *a, **kw):
        calls.append([e.n_seq for e in self.engines])
        wgs.append(slices(self.engines))
        return train(self, *a, **kw)

    monkeypatch.setattr(EngineGroup, "train", spy)
    out_grp = io.StringIO()
    with contextlib.redirect_stdout(out_grp):
        res_grp = hmm_training_group(sets, N=N, M=K, max_iterations=12, word_names=names, device=0)
    print(f"EngineGroup.train calls (sequences per member): {calls}, slices {wgs} workgroups")
    assert calls == [[3, 40, 11]] and wgs == [[1, 2, 1]], "one group must train all the words"
    assert out_grp.getvalue() == out_seq.getvalue() and "Iteration 1\n" in out_grp.getvalue()
    for w, ((A1, B1, p1), (A2, B2, p2)) in enumerate(zip(res_seq, res_grp)):
        params_excess(A2, A1, f"A[{w}]")
        params_excess(B2, B1, f"B[{w}]")
        params_excess(p2, p1, f"pi[{w}]")


def test_score_matrix_scores_each_shape_bucket_in_one_group(oracle, monkeypatch):
    """Models of two shapes (three N = 8 left-to-right, two N = 5 dense): one EngineGroup.score per shape bucket, and
    every column against the oracle."""
    from hmm_training_amd.engine import EngineGroup
    from hmm_training_amd.hmm_classes import HMMTrained
    from hmm_training_amd.hmm_testing import score_matrix
    K = 24
    rng = np.random.default_rng(91)
    shapes = [(8, False)] * 3 + [(5, True)] * 2
    models = []
    for i, (N, dense) in enumerate(shapes):
        pi, A, B = model(rng, N, K, dense)
        models.append(HMMTrained(states=N, symbols=K, A=A, B=B, Pi=pi, word=f"w{i}"))
    test = Member("test", ragged(rng, 45, K, 20), None, None, None)
    calls = []
    score = EngineGroup.score

    def spy(self):
        calls.append([(e.N, e.topology) for e in self.engines])
        print(f"EngineGroup.score: slices {slices(self.engines)} workgroups")
        return score(self)

    monkeypatch.setattr(EngineGroup, "score", spy)
    S = score_matrix(test.obs, models, device=0)
    print(f"EngineGroup.score calls: {calls}")
    assert calls == [[(8, "left_to_right")] * 3, [(5, "dense")] * 2], "one grouped score per shape bucket"
    for m, h in enumerate(models):
        ll_excess(S[:, m], test.score_ref(oracle, h.states, K, (h.Pi, h.A, h.B)), f"model {m}", LOGP_ATOL)
