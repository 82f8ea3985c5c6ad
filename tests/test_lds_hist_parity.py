"""The histogram parity halves of the class-split LDS tables (hmm_training_amd/csrc/lds_layout.hpp: lay2_add_off,
lay2_b_off, lay2_total_bytes), without a GPU: the address functions through a host-compiled probe
(tests/native/lds_hist_parity_probe.cpp) and the bank-conflict model of tools/lds_banks.py ("parity")."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_lds_layout import _host_compiler

sys.path.insert(0, os.path.join(ROOT, "tools"))

G, K = 8, 256
U = 64 // G


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """(constants, add table [u, o, j, P offset, add offset], b table [o, j, offset]) at G = 8, K = 256."""
    exe = str(tmp_path_factory.mktemp("lds_hist_parity") / "lds_hist_parity_probe")
    src = os.path.join(ROOT, "tests", "native", "lds_hist_parity_probe.cpp")
    subprocess.run([_host_compiler(), "-std=c++17", "-O1", "-Wall", "-Werror", src, "-o", exe], check=True)
    out = subprocess.run([exe, str(G), str(K)], check=True, capture_output=True, text=True).stdout.splitlines()
    head = out[0].split()
    consts = {head[i]: int(head[i + 1]) for i in range(0, len(head), 2)}
    adds = np.array([[int(x) for x in l.split()[1:]] for l in out[1:] if l.startswith("a ")], dtype=np.int64)
    btab = np.array([[int(x) for x in l.split()[1:]] for l in out[1:] if l.startswith("b ")], dtype=np.int64)
    assert adds.shape == (U * K * G, 5) and btab.shape == (K * G, 3)
    return consts, adds, btab


@pytest.mark.parametrize("symbols", ["uniform", "equal", "two"])
def test_bank_model_parity_conflict_free(symbols):
    """ds_add_f64 on the parity halves: exactly one LDS cycle per 16-lane group whatever the symbols (the halves of
    the two slots of a group are disjoint bank pairs); the read is the class-split one, still conflict-free."""
    import lds_banks
    assert lds_banks.add_cycles(G, G, K, np.random.default_rng(1), trials=1000, layout="parity", symbols=symbols) == 1.0
    assert lds_banks.read_cycles(G, G, K, np.random.default_rng(1), trials=1000, layout="parity", symbols=symbols) == 1.0


def test_bank_model_what_the_halves_remove():
    """The same draws on the {h, b} entries: 2.00 cycles per group on uniform symbols, 1.50 on two-valued ones."""
    import lds_banks
    uni = lds_banks.add_cycles(G, G, K, np.random.default_rng(1), trials=2000, layout="split", symbols="uniform")
    two = lds_banks.add_cycles(G, G, K, np.random.default_rng(1), trials=2000, layout="split", symbols="two")
    assert round(uni, 2) == 2.00 and abs(two - 1.5) < 0.03


def test_add_addresses(probe):
    consts, adds, btab = probe
    u, o, j, p, a = adds.T
    import lds_banks
    assert np.all(a % 8 == 0)                                    # ds_add_f64
    assert np.all(p % 16 == 0)                                   # the read keeps its 16-B alignment
    # inside the H row of the slot's class: bytes [128, 256) of row o of class (u >> 1) & 1
    cls = (u >> 1) & 1
    row = cls * (65536 + 128) + o * 256
    assert np.all(a >= row + 128) and np.all(a + 8 <= row + 256)
    # the field is half u & 1 of the H entry of (o, j)
    assert np.array_equal(a, row + 128 + j * 16 + 8 * (u & 1))
    # the two slots of every add group (2i, 2i + 1), equal symbols: exactly 8 bytes apart
    t = adds.reshape(U, K, G, 5)
    for i in range(U // 2):
        assert np.all(t[2 * i + 1, :, :, 4] - t[2 * i, :, :, 4] == 8)
    # slots of one class and one parity share their piece; there are exactly four pieces per (o, j)
    assert len(np.unique(a)) == 4 * K * G
    # no add field overlaps a P entry or the b table
    pbytes = set()
    for c in (0, 1):
        for oo in range(K):
            base = c * (65536 + 128) + oo * 256
            pbytes.update(range(base // 8, (base + 128) // 8))
    abytes = set((a // 8).tolist())
    assert abytes.isdisjoint(pbytes)
    bo = btab[:, 2]
    assert abytes.isdisjoint(set((bo // 8).tolist()))
    assert a.max() + 8 <= consts["table_bytes"] <= bo.min()


def test_b_table(probe):
    consts, adds, btab = probe
    o, j, off = btab.T
    assert np.array_equal(off, consts["table_bytes"] + (o * G + j) * 8)   # compact [K][GP] fp64 after the class tables
    assert off.max() + 8 == consts["total_bytes"] == consts["table_bytes"] + consts["b_bytes"]
    assert consts["b_bytes"] == K * G * 8
    # a symbol's pack entry (its P/H row offset) shifted down is its b row offset
    packs = adds[(adds[:, 0] == 0) & (adds[:, 2] == 0)][:, 3]
    assert np.array_equal(packs >> consts["b_pack_shift"], np.arange(K) * G * 8)


def test_total_bytes_fit_a_cu(probe):
    consts, _, _ = probe
    assert consts["cu_bytes"] == 160 * 1024
    assert consts["total_bytes"] == 147584 <= 160 * 1024
    # with the reduction scratch of the widest instantiation (dense N = 8: [8 waves][8][11] + 16 doubles) and
    # 4 KiB of static LDS
    assert consts["other_bytes"] == 8 * (8 * 8 * 11 + 16) + 4096
    assert consts["total_bytes"] + consts["other_bytes"] <= consts["cu_bytes"]
    assert consts["fit"] == 1 and consts["first_unfit_K"] == K + 1   # K = 257 is refused


def test_tool_mirrors_header(probe):
    import lds_banks
    consts, adds, btab = probe
    assert lds_banks.parity_total_bytes(K, G) == consts["total_bytes"]
    for u, o, j, p, a in adds[::41]:
        assert lds_banks.parity_add_off(G, int(u)) == a - p
        assert lds_banks.parity_add_addr(G, int(u), int(o), int(j)) == a
    for o, j, off in btab[::29]:
        assert lds_banks.parity_b_off(K, G, int(o), int(j)) == off
