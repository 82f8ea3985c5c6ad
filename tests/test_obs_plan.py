"""The observation layout and the launch map (hmm_training_amd/csrc/obs_plan.hpp) without a GPU, through a
host-compiled probe (tests/native/obs_plan_probe.cpp): the map's figures at 256 CUs, the contract between the map
and the kernel's wave_role over every (workgroup, wave) of a launch, and the layout on ragged input."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_lds_layout import _host_compiler

AUTO, DENSE, LR = 0, 1, 2  # HMMBW_TOPOLOGY_*
CHUNK, WAVE = 8, 64
NCU = 256


@pytest.fixture(scope="session")
def probe_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("obs_plan") / "obs_plan_probe")
    src = os.path.join(ROOT, "tests", "native", "obs_plan_probe.cpp")
    subprocess.run([_host_compiler(), "-std=c++17", "-O1", "-Wall", "-Werror", src, "-o", exe], check=True)
    return exe


def geometry(N, K):
    """What hmmbw_ctx_create derives from the shape: lane-group size, sequences per wave, wide, NP, LDS tables."""
    wide = N > 16
    NP = 16 * ((N + 15) // 16) if wide else 0
    G = NP if wide else (2 if N <= 2 else 4 if N <= 4 else 8 if N <= 8 else 16)
    U = 16 if wide else WAVE // G
    return {"G": G, "U": U, "wide": wide, "NP": NP, "lds_tables": not wide and K * G * 16 <= 32768}


def run_map(exe, R, T, *, N=8, K=256, ncu=NCU, topo=LR, topo_req=None, det=False, split_extra=1, join=1,
            join_dense=1, lds_layout=-1, xact=0):
    """The probe's map of R sequences of T steps each: (figures, role rows, role rows under the old planner's
    EArgs::split_extra); role columns: J, bid, wv, wave, slot, xblk, split, brole, active."""
    g = geometry(N, K)
    nwaves = -(-R // g["U"])
    steps = nwaves * (-(-T // CHUNK) * CHUNK)
    split_tables = (lds_layout != 0 and not g["wide"] and not det and g["G"] == 8 and g["lds_tables"]
                    and K * 2 * g["G"] * 16 <= 65536)
    args = [nwaves, steps, ncu, int(g["wide"]), int(det), int(g["lds_tables"]), int(split_tables),
            topo if topo_req is None else topo_req, topo, split_extra, join, join_dense, lds_layout, xact]
    out = subprocess.run([exe, "map"] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout
    lines = out.splitlines()
    head = lines[0].split()
    fig = {head[i]: int(head[i + 1]) for i in range(0, len(head), 2)}
    fig["waves"] = nwaves
    rows = {tag: np.array([[int(x) for x in l.split()[1:]] for l in lines[1:] if l.startswith(tag + " ")],
                          dtype=np.int64).reshape(-1, 9) for tag in ("role", "orole")}
    return fig, rows["role"], rows["orole"]


# (R, T, keywords) -> figures; the table of the map at 256 CUs, N = 8, K = 256, default switches
MAPS = [
    ("lr_t200", 10_000, 200, {}, dict(waves=1250, nfull=256, xact=2, nblocks=369, joined=1, split_extra=1, split_tables=1)),
    ("lr_t96", 10_000, 96, {}, dict(waves=1250, nfull=256, xact=2, nblocks=369, joined=1, split_extra=1, split_tables=0)),
    ("lr_t144", 10_000, 144, {}, dict(waves=1250, nblocks=369, joined=1, split_tables=1)),
    ("lr_t143", 10_000, 143, {}, dict(waves=1250, nblocks=369, joined=1, split_tables=1)),  # 144 steps in whole chunks
    ("lr_t136", 10_000, 136, {}, dict(waves=1250, nblocks=369, joined=1, split_tables=0)),
    ("dense", 10_000, 200, dict(topo=DENSE), dict(waves=1250, nfull=256, xact=1, nblocks=482, joined=1, split_extra=1,
                                                  split_tables=0)),
    ("lr_12500", 12_500, 200, {}, dict(waves=1563, nfull=256, xact=4, nblocks=391, joined=1, split_extra=0)),
    ("lr_8192", 8_192, 8, {}, dict(waves=1024, nfull=256, xact=4, nblocks=256, fits_cus=1, joined=1)),
    ("dense_8192", 8_192, 8, dict(topo=DENSE), dict(waves=1024, nfull=256, xact=4, nblocks=256, fits_cus=1, joined=0)),
    ("det", 10_000, 200, dict(det=True), dict(waves=1250, nblocks=313, nfull=313, xact=4, joined=0, split_extra=0)),
    ("wide", 150, 8, dict(N=40, K=64, topo=DENSE), dict(waves=10, nblocks=10, joined=0, split_extra=0)),
    # join = 0: the separate extra workgroups, no class-split tables; left-to-right then does not split
    ("lr_nojoin", 10_000, 200, dict(join=0), dict(nblocks=369, xact=2, joined=0, split_extra=0, split_tables=0)),
    ("dense_nojoin", 10_000, 200, dict(topo=DENSE, join_dense=0), dict(nblocks=482, xact=1, joined=0, split_extra=1,
                                                                      split_tables=0)),
    # join = 0 on the dense launch too (its own switch is join_dense): separate extra workgroups, which still split
    ("dense_join0", 10_000, 200, dict(topo=DENSE, join=0), dict(nblocks=482, xact=1, joined=0, split_extra=1,
                                                               split_tables=0)),
    ("lr_t96_nojoin", 10_000, 96, dict(join=0), dict(nblocks=369, xact=2, joined=0, split_extra=0, split_tables=0)),
    ("lr_9000_nojoin", 9_000, 160, dict(join=0), dict(waves=1125, nfull=256, xact=2, nblocks=307, joined=0, split_extra=0,
                                                      split_tables=0)),
    ("dense_9000_join0", 9_000, 160, dict(topo=DENSE, join=0), dict(waves=1125, nfull=256, xact=1, nblocks=357, joined=0,
                                                                    split_extra=1, split_tables=0)),
    ("dense_8192_join0", 8_192, 8, dict(topo=DENSE, join=0), dict(nblocks=256, joined=0, split_extra=0, split_tables=0)),
    ("lr_12500_nojoin", 12_500, 200, dict(join=0), dict(nblocks=391, nfull=391, xact=4, joined=0, split_extra=0)),
    ("lr_8192_nojoin", 8_192, 8, dict(join=0), dict(nblocks=256, joined=0, split_tables=0)),
    # HMMBW_XACT = 1, 3, 4 on 9,000 sequences = 1,125 waves, 101 past the SIMDs (test_gpu_fullsize's parametrisation)
    ("lr_xact_default", 9_000, 160, {}, dict(waves=1125, nfull=256, xact=2, nblocks=256 + 51, joined=1)),
    ("lr_xact1", 9_000, 160, dict(xact=1), dict(nfull=256, xact=1, nblocks=256 + 101, joined=1, split_extra=1)),
    ("lr_xact3", 9_000, 160, dict(xact=3), dict(nfull=256, xact=3, nblocks=256 + 34, joined=1, split_extra=0)),
    ("lr_xact4", 9_000, 160, dict(xact=4), dict(nfull=282, xact=4, nblocks=282, joined=0, split_extra=0)),
    ("lr_xact1_nojoin", 9_000, 160, dict(xact=1, join=0), dict(xact=1, nblocks=357, joined=0, split_extra=0)),
    ("dense_xact_default", 9_000, 160, dict(topo=DENSE), dict(xact=1, nblocks=357, joined=1, split_extra=1)),
    ("dense_nosplit", 10_000, 200, dict(topo=DENSE, split_extra=0), dict(xact=2, nblocks=369, joined=1, split_extra=0)),
    # HMMBW_OPT_LDS_LAYOUT: 0 never, 1 wherever split_tables() allows (not in deterministic mode)
    ("lr_t200_lay0", 10_000, 200, dict(lds_layout=0), dict(sym2=0, joined=1, split_tables=0)),
    ("lr_t96_lay1", 10_000, 96, dict(lds_layout=1), dict(sym2=1, joined=1, split_tables=1)),
    ("lr_8192_lay1", 8_192, 8, dict(lds_layout=1), dict(sym2=1, joined=1, split_tables=1)),
    ("dense_lay1", 10_000, 200, dict(topo=DENSE, lds_layout=1), dict(sym2=1, joined=1, split_tables=1)),
    ("det_lay1", 10_000, 200, dict(det=True, lds_layout=1), dict(sym2=0, split_tables=0)),
    ("lr_lay1_nojoin", 10_000, 200, dict(lds_layout=1, join=0), dict(sym2=1, joined=0, split_tables=0)),
]


@pytest.mark.parametrize("name,R,T,kw,want", MAPS, ids=[m[0] for m in MAPS])
def test_map_figures_and_kernel_contract(probe_exe, name, R, T, kw, want):
    fig, role, orole = run_map(probe_exe, R, T, **kw)
    assert {k: fig[k] for k in want} == want, fig
    if fig["xact"] == 4 and kw.get("topo", LR) == LR and not kw.get("det") and fig["nblocks"] == fig["nfull"]:
        assert fig["joined"] == (fig["fits_cus"] and kw.get("join", 1))  # the no-extra-groups rule
    # EArgs::split_extra from split_extra_on gives every wave the role the planner's earlier value gave it
    assert np.array_equal(role, orole)
    if kw.get("N", 8) > 16:
        assert len(role) == 0
        return
    nw, xact = fig["waves"], fig["xact"]
    launches = sorted(set(role[:, 0].tolist()))
    assert launches == ([0, 1] if fig["nblocks"] - fig["nfull"] <= fig["nfull"] else [0])
    if fig["joined"]:
        assert 1 in launches
    for J in launches:
        r = role[role[:, 0] == J]
        _, bid, wv, wave, slot, xblk, split, brole, active = r.T
        grid, wpg = (fig["nfull"], 8) if J else (fig["nblocks"], 4)
        assert len(r) == grid * wpg and np.array_equal(bid * wpg + wv, np.arange(grid * wpg))  # the whole grid
        run = (active == 1) & (wave < nw)  # what estep_small_body runs: wactive && wave < nwaves
        a = run & (brole == 0)
        # each wave exactly once among the non-B roles.  Active indices at or above the wave count (the tail of the
        # last workgroup; waves 4.. of a joined workgroup without an extra group) are what the kernel's guard
        # leaves out: they are distinct slots of the launch's capacity, never a second claim on a real wave
        assert np.array_equal(np.sort(wave[a]), np.arange(nw))
        cap = fig["nfull"] * (4 + xact) if J else fig["nfull"] * 4 + (fig["nblocks"] - fig["nfull"]) * xact
        anb = (active == 1) & (brole == 0)
        assert np.array_equal(np.sort(wave[anb]), np.arange(cap))
        if not J:
            assert cap - nw < 4
        assert np.all(xblk[brole == 1] == 1) and np.all(split[brole == 1] == 1) and np.all(active[brole == 1] == 1)
        # every B partner names the wave of exactly one A wave, in the same workgroup, in the same hand-over slot
        akey = {(int(b), int(w), int(s)) for b, w, s in zip(bid[a & (xblk == 1)], wave[a & (xblk == 1)], slot[a & (xblk == 1)])}
        bsel = run & (brole == 1)
        bkey = [(int(b), int(w), int(s)) for b, w, s in zip(bid[bsel], wave[bsel], slot[bsel])]
        assert len(set(bkey)) == len(bkey) and set(bkey) <= akey
        # the slots of a workgroup's extra groups are distinct and index the kernel's kBlock / kWave / 2 flags when split
        sa = (split == 1) & (active == 1)
        assert np.all((slot[sa] >= 0) & (slot[sa] < 2))
        # B partners appear only when 2 xact <= 4, and then with every A wave of an extra group when the split is on
        if 2 * xact > 4:
            assert not brole.any()
        if split.any():
            assert 2 * xact <= 4 and len(bkey) == int((a & (xblk == 1)).sum())
    # the split runs on the launch the info key speaks of
    Jrun = 1 if fig["joined"] else 0
    assert bool(role[(role[:, 0] == Jrun), 6].any()) == bool(fig["split_extra"])


# ---------------------------------------------------------------------------------------------------------------
# layout
# ---------------------------------------------------------------------------------------------------------------
def _ragged(R, K, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, K, size=int(t)) for t in rng.integers(1, 41, size=R)]


def run_layout(exe, tmp_path, obs, U, wide, NP, G):
    path = str(tmp_path / "obs.txt")
    with open(path, "w") as f:
        f.write(f"{len(obs)}\n")
        for o in obs:
            f.write(" ".join(str(x) for x in [len(o), *o.tolist()]) + "\n")
    out = subprocess.run([exe, "layout", path, str(U), str(int(wide)), str(NP), str(G)], check=True,
                         capture_output=True, text=True).stdout
    return {l.split()[0]: np.array(l.split()[1:], dtype=np.int64) for l in out.splitlines()}


@pytest.mark.parametrize("U,wide,NP,G", [(4, False, 0, 16), (8, False, 0, 8), (16, False, 0, 4), (16, True, 48, 8)])  # G: the packs' row scale only
@pytest.mark.parametrize("R", [1, 7, 8, 9, 65])
def test_layout_ragged(probe_exe, tmp_path, R, U, wide, NP, G):
    K = 64
    obs = _ragged(R, K, 1000 * U + R)
    L = run_layout(probe_exe, tmp_path, obs, U, wide, NP, G)
    lens = np.array([len(o) for o in obs])
    nw = -(-R // U)
    nwaves, symtot, cktot, sptot = L["tot"]
    assert nwaves == nw
    # the stable length-descending permutation in the slots, padding after it
    perm = np.argsort(-lens, kind="stable")
    assert np.array_equal(L["slot_seq"], np.concatenate([perm, -np.ones(nw * U - R, dtype=np.int64)]))
    assert np.array_equal(L["slot_len"], np.concatenate([lens[perm], np.zeros(nw * U - R, dtype=np.int64)]))
    # wave_T, wave_full (set exactly when all real slots share wave_T), offsets: running sums of chunk-rounded sizes
    sl = L["slot_len"].reshape(nw, U)
    real = L["slot_seq"].reshape(nw, U) >= 0
    assert np.array_equal(L["wave_T"], sl.max(1))
    assert np.array_equal(L["wave_full"], [int(np.all(sl[w][real[w]] == sl[w].max())) for w in range(nw)])
    nch = -(-L["wave_T"] // CHUNK)
    run = lambda per: np.concatenate([[0], np.cumsum(per)])
    sym_run = run(nch * U * CHUNK)
    ck_run = run(nch * CHUNK * NP * 16 if wide else nch * WAVE)
    sp_run = run(nch * CHUNK * 16 if wide else nch * U)
    assert np.array_equal(L["symoff"], sym_run[:-1]) and symtot == sym_run[-1]
    assert np.array_equal(L["ckoff"], ck_run[:-1]) and cktot == ck_run[-1]
    assert np.array_equal(L["spoff"], sp_run[:-1]) and sptot == sp_run[-1]
    # every (sequence, t) at a distinct pack position inside its wave's range; padding positions hold 0
    row_bytes = 16 * G
    want = np.zeros(max(symtot, 1), dtype=np.int64)
    seen = np.zeros(max(symtot, 1), dtype=bool)
    pos_of = {}
    for s in range(R):
        w, u, r = s // U, s % U, int(perm[s])
        for t in range(lens[r]):
            p = L["symoff"][w] + ((t // CHUNK) * U + u) * CHUNK + t % CHUNK
            assert sym_run[w] <= p < sym_run[w + 1] and not seen[p]
            seen[p] = True
            want[p] = obs[r][t] * row_bytes
            pos_of[(r, t)] = (p, ck_run[w] // NP + t * U + u if wide else p)
    assert np.array_equal(L["pack"], want) and np.all(L["pack"][~seen] == 0)
    # the class-split packs: symbol * lay2_row_bytes(G) = symbol * 2 G 16
    assert np.array_equal(L["pack2"], want // row_bytes * (2 * G * 16))
    # both gather indices: the real positions, grouped by symbol, in stable (slot, then time) order
    order = [(int(obs[int(perm[s])][t]), s, t) for s in range(R) for t in range(lens[perm[s]])]
    order.sort(key=lambda x: x[0])  # stable
    total = int(lens.sum())
    counts = np.bincount([o[0] for o in order], minlength=len(L["bptr"]) - 1)
    assert np.array_equal(L["bptr"], run(counts)) and L["bptr"][-1] == total
    assert np.array_equal(L["rows"], [pos_of[(int(perm[s]), t)][0] for _, s, t in order])
    assert len(set(L["rows"].tolist())) == total and np.all(seen[L["rows"]])
    prow = L["prow"]
    assert len(prow) == max(cktot // NP if wide else symtot, 1)
    real_pos = np.array([pos_of[(int(perm[s]), t)][1] for _, s, t in order])
    assert np.array_equal(prow[real_pos], np.arange(total))  # the inverse: position -> rank
    pad = np.ones(len(prow), dtype=bool)
    pad[real_pos] = False
    assert np.all(prow[pad] == total)  # padding rows: the scratch row past the real ones
