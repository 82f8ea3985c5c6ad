"""The engine's launch map (BaumWelchEngine.launch_map, HMMBW_INFO_*) against the planner's own figures: what
hmmbw_set_observations stores must be what obs_plan.hpp's probe (tests/native/obs_plan_probe.cpp, test_obs_plan.py)
prints for the same shape, switches and the device's CU count.  Only set_observations and set_params run."""
import numpy as np
import pytest

from test_gpu_fullsize import _params
from test_obs_plan import DENSE, LR, geometry, probe_exe, run_map  # noqa: F401 (probe_exe: fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ncu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: the GPU tests need an MI355X")
    return torch.cuda.get_device_properties(0).multi_processor_count


# name, R, T, N, K, topology, engine keywords, LDS layout option, environment
CASES = [
    ("lr_t8", 10_000, 8, 8, 256, LR, {}, None, {}),
    ("lr_t144", 10_000, 144, 8, 256, LR, {}, None, {}),       # the class-split tables by default
    ("lr_t144_lay0", 10_000, 144, 8, 256, LR, {}, 0, {}),
    ("lr_t8_lay1", 10_000, 8, 8, 256, LR, {}, 1, {}),
    ("dense", 10_000, 8, 8, 256, DENSE, {}, None, {}),
    ("lr_12500", 12_500, 8, 8, 256, LR, {}, None, {}),
    ("lr_8192", 8_192, 8, 8, 256, LR, {}, None, {}),
    ("dense_8192", 8_192, 8, 8, 256, DENSE, {}, None, {}),
    ("det", 10_000, 8, 8, 256, LR, {"deterministic": True}, None, {}),
    ("wide", 150, 8, 40, 64, DENSE, {}, None, {}),
    ("lr_nojoin", 10_000, 8, 8, 256, LR, {}, None, {"HMMBW_JOIN": "0"}),
    ("dense_join0", 10_000, 8, 8, 256, DENSE, {}, None, {"HMMBW_JOIN": "0"}),
    ("dense_9000_join0", 9_000, 8, 8, 256, DENSE, {}, None, {"HMMBW_JOIN": "0"}),
    ("lr_9000_nojoin", 9_000, 8, 8, 256, LR, {}, None, {"HMMBW_JOIN": "0"}),
    ("dense_nojoin", 10_000, 8, 8, 256, DENSE, {}, None, {"HMMBW_JOIN_DENSE": "0"}),
    ("dense_nosplit", 10_000, 8, 8, 256, DENSE, {}, None, {"HMMBW_SPLIT_EXTRA": "0"}),
    ("lr_12500_nojoin", 12_500, 8, 8, 256, LR, {}, None, {"HMMBW_JOIN": "0"}),
    ("lr_8192_nojoin", 8_192, 8, 8, 256, LR, {}, None, {"HMMBW_JOIN": "0"}),
    ("lr_xact1", 9_000, 8, 8, 256, LR, {}, None, {"HMMBW_XACT": "1"}),
    ("lr_xact3", 9_000, 8, 8, 256, LR, {}, None, {"HMMBW_XACT": "3"}),
    ("lr_xact4", 9_000, 8, 8, 256, LR, {}, None, {"HMMBW_XACT": "4"}),
    ("lr_xact1_nojoin", 9_000, 8, 8, 256, LR, {}, None, {"HMMBW_XACT": "1", "HMMBW_JOIN": "0"}),
]


@pytest.mark.parametrize("name,R,T,N,K,topo,ekw,layout,env", CASES, ids=[c[0] for c in CASES])
def test_launch_map_is_the_planners(probe_exe, ncu, monkeypatch, name, R, T, N, K, topo, ekw, layout, env):  # noqa: F811
    from hmm_training_amd._lib import OPT_LDS_LAYOUT
    from hmm_training_amd.engine import BaumWelchEngine
    for k in ("HMMBW_JOIN", "HMMBW_JOIN_DENSE", "HMMBW_SPLIT_EXTRA", "HMMBW_XACT", "HMMBW_LDS_LAYOUT"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    fig, _, _ = run_map(probe_exe, R, T, N=N, K=K, ncu=ncu, topo=topo, det=bool(ekw.get("deterministic")),
                        split_extra=int(env.get("HMMBW_SPLIT_EXTRA", 1)), join=int(env.get("HMMBW_JOIN", 1)),
                        join_dense=int(env.get("HMMBW_JOIN_DENSE", 1)), lds_layout=-1 if layout is None else layout,
                        xact=int(env.get("HMMBW_XACT", 0)))
    g = geometry(N, K)
    wide = g["wide"]
    want = {"waves": fig["nblocks"] * (g["NP"] // 16) if wide else fig["waves"], "workgroups": fig["nblocks"],
            "waves_per_workgroup": g["NP"] // 16 if wide else 4,
            "full_workgroups": fig["nblocks"] if wide else min(fig["nfull"], fig["nblocks"]),
            "extra_waves": 0 if wide else fig["xact"], "joined": bool(fig["joined"]),
            "split_extra": bool(fig["split_extra"]), "lds_layout": fig["split_tables"]}
    rng = np.random.default_rng(R + T)
    sym = rng.integers(0, K, size=R * T).astype(np.int32)
    off = np.arange(R + 1, dtype=np.int64) * T
    topology = "dense" if topo == DENSE else "left_to_right"
    pi, A, B = _params(N, K, topology, 3)
    with BaumWelchEngine(N, K, topology=topology, **ekw) as eng:
        if layout is not None:
            eng.set_option(OPT_LDS_LAYOUT, layout)
        eng.set_observations(offsets=off, symbols=sym)
        eng.set_params(pi, A, B)
        lm = eng.launch_map()
        print(name, "ncu", ncu, "probe", fig, "engine", lm)
        assert {k: lm[k] for k in want} == want, (lm, want)
        assert eng.lds_layout == fig["split_tables"]
