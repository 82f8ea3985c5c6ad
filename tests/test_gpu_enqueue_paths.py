"""The four ways an EM iteration is enqueued, side by side on one small data set: hmmbw_iterate, hmmbw_estep +
hmmbw_mstep on one rank, hmmbw_iterate_begin / _end with in-process ranks (world 2, one shard empty: the
memset branch and the standalone M-step beside a merged rank) and a grouped launch of two members with unequal
sequence counts.  Each path picks other buffers for the same E-step launch (the statistics triple buffer, the
packed copy set, the fused all-reduce buffer) and hands the M-step its input in its own way, so each is held
against the oracle (hmm_training.py:351-514) with the tolerances of test_gpu_parity.py and test_gpu_group.py, with
the M-step merged into the next launch and as its own kernel.

About 70 sequences of 1..40 symbols: more than one workgroup, a partial last wave, a sequence of one symbol.
The wide shape (N = 20) has no grouped kernel: there the group is refused with HMMBW_E_UNSUPPORTED, as it is today."""
import ctypes

import numpy as np
import pytest

from test_gpu_group import assert_params as assert_params_group
from test_gpu_multirank import allreduce_in_process, hip  # noqa: F401  (hip: the fixture)
from test_gpu_parity import LL_RTOL, assert_ll, assert_params

pytestmark = pytest.mark.gpu

ITERS = 3
R, SPLIT = 70, 45  # the group's members hold sequences [0, 45) and [45, 70)
SHAPES = {"lr": (4, 16, "left_to_right"), "dense": (5, 32, "dense"), "wide": (20, 24, "dense")}
_cache = {}


def problem(oracle, shape):
    """(obs, initial parameters, oracle runs of: all sequences, the group's two members), made once per shape."""
    if shape not in _cache:
        from hmm_training_amd.engine import to_csr
        from hmm_training_amd.hmm_training import default_initial_params
        N, K, topology = SHAPES[shape]
        rng = np.random.default_rng(100 + N)
        lens = rng.integers(1, 41, size=R)
        lens[3], lens[SPLIT + 1] = 1, 1
        obs = [rng.integers(0, K, size=int(t)) for t in lens]
        pi, A, B = default_initial_params(N, K)
        if topology == "dense":
            A = 0.5 * A + 0.5 * rng.dirichlet(np.ones(N), size=N)
        B = rng.dirichlet(np.full(K, 2.0), size=N)
        refs = []
        for part in (obs, obs[:SPLIT], obs[SPLIT:]):
            off, sym = to_csr(part)
            refs.append(oracle.hmm_training(off, sym.astype(np.int64), N, K, 0.0, ITERS, pi, A, B))
        _cache[shape] = (obs, (pi, A, B), refs)
    return _cache[shape]


def engine(shape, merge, obs, init, n_seq_global=None, **kw):
    from hmm_training_amd.engine import BaumWelchEngine
    N, K, topology = SHAPES[shape]
    e = BaumWelchEngine(N, K, topology=topology, merge_mstep=merge, **kw)
    e.set_observations(obs, n_seq_global=n_seq_global)
    e.set_params(*init)
    e.reset(0.0, ITERS)
    return e


def result(e):
    st, recs = e.status(0, ITERS)
    return st, recs, e.params(normalise=True)


def check(res, ref, what, params=assert_params):
    st, recs, (pi, A, B) = res
    assert st.iterations == ITERS and st.done and len(recs) == ITERS, what
    assert_ll([L for L, _ in recs], ref.trace_L, LL_RTOL)
    params(A, ref.A, f"{what}: A")
    params(B, ref.B, f"{what}: B")
    params(pi, ref.pi, f"{what}: pi")


def run_iterate(shape, merge, obs, init):
    with engine(shape, merge, obs, init) as e:
        e.enqueue_iterations(ITERS)  # world 1: hmmbw_iterate
        return result(e)


def run_estep_mstep(shape, merge, obs, init):
    with engine(shape, merge, obs, init) as e:
        stats = e.make_stats_buffer()
        ptr = ctypes.c_void_p(stats.data_ptr())
        for _ in range(ITERS):
            assert e._lib.hmmbw_estep(e._ctx, ptr) == 0
            assert e._lib.hmmbw_mstep(e._ctx, ptr, len(obs)) == 0
        return result(e)


def run_split(hip, shape, merge, obs, init):
    engines = []
    try:
        for r, part in enumerate((obs, [])):
            engines.append(engine(shape, merge, part, init, n_seq_global=len(obs), rank=r, world_size=2))
        for _ in range(ITERS):
            bufs = [e.iterate_begin() for e in engines]
            allreduce_in_process(hip, bufs)
            for e in engines:
                e.iterate_end()
        return [result(e) for e in engines]
    finally:
        for e in engines:
            e.close()


def run_group(shape, merge, obs, init):
    from hmm_training_amd._lib import HMMBW_E_UNSUPPORTED, HMMBWError
    from hmm_training_amd.engine import EngineGroup
    engines = [engine(shape, merge, part, init) for part in (obs[:SPLIT], obs[SPLIT:])]
    try:
        if shape == "wide":
            with pytest.raises(HMMBWError) as ei:
                EngineGroup(engines)
            assert ei.value.code == HMMBW_E_UNSUPPORTED
            return None
        grp = EngineGroup(engines)
        try:
            grp.enqueue_iterations(ITERS)
            return [result(e) for e in engines]
        finally:
            grp.close()
    finally:
        for e in engines:
            e.close()


@pytest.mark.parametrize("merge", [True, False])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_enqueue_path_matches_the_oracle(hip, oracle, shape, merge):  # noqa: F811
    obs, init, (ref, ref_a, ref_b) = problem(oracle, shape)
    check(run_iterate(shape, merge, obs, init), ref, "hmmbw_iterate")
    check(run_estep_mstep(shape, merge, obs, init), ref, "hmmbw_estep + hmmbw_mstep")
    ranks = run_split(hip, shape, merge, obs, init)
    for r, res in enumerate(ranks):
        check(res, ref, f"iterate_begin / _end, rank {r}")
    assert ranks[0][1] == ranks[1][1], "the ranks' records differ"
    members = run_group(shape, merge, obs, init)
    if members is not None:
        check(members[0], ref_a, "group member 0", assert_params_group)
        check(members[1], ref_b, "group member 1", assert_params_group)
