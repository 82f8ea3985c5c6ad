"""The class-split LDS emission tables of the joined map (hmm_training_amd/csrc/lds_layout.hpp), without a GPU:
the address function itself through a host-compiled probe (tests/native/lds_layout_probe.cpp), and the
bank-conflict model of tools/lds_banks.py on the row tables and on the class-split ones."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))

G, K = 8, 256


def _host_compiler():
    for cxx in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    pytest.fail("no host C++ compiler found for the layout probe")


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """(constants, classes, table) printed by the probe at G = 8, K = 256; table rows: class, o, j, P, H offsets."""
    exe = str(tmp_path_factory.mktemp("lds_layout") / "lds_layout_probe")
    src = os.path.join(ROOT, "tests", "native", "lds_layout_probe.cpp")
    subprocess.run([_host_compiler(), "-std=c++17", "-O1", "-Wall", "-Werror", src, "-o", exe], check=True)
    out = subprocess.run([exe, str(G), str(K)], check=True, capture_output=True, text=True).stdout.splitlines()
    head = out[0].split()
    consts = {head[i]: int(head[i + 1]) for i in range(0, len(head), 2)}
    classes = [int(x) for x in out[1].split()[1:]]
    table = np.array([[int(x) for x in l.split()] for l in out[2:]], dtype=np.int64)
    assert table.shape == (2 * K * G, 5)
    return consts, classes, table


def test_layout_constants(probe):
    consts, classes, _ = probe
    assert consts == {"row_bytes": 256, "hist_off": 128, "class_off": 65536 + 128, "table_bytes": 131200, "fit": 1}
    # the slots a ds_read_b128 lane group puts on the same states (0 with 3, 1 with 2) are in different classes,
    # the two slots of a ds_add_f64 lane group (2i, 2i + 1) in the same one
    assert len(classes) == 64 // G
    for base in (0, 4):
        assert classes[base] != classes[base + 3] and classes[base + 1] != classes[base + 2]
    assert all(classes[2 * i] == classes[2 * i + 1] for i in range(len(classes) // 2))
    assert set(classes) == {0, 1}


def test_layout_addresses(probe):
    consts, _, t = probe
    cls, o, j, p, h = t.T
    assert np.all(p % 16 == 0) and np.all(h % 16 == 0)            # ds_read_b128 / 16-B entries
    assert np.all(h - p == 128)                                   # one immediate offset for the add and H.b
    assert p.min() == 0 and np.all(h + 16 <= consts["table_bytes"])  # inside the declared table bytes
    # no two entries (P or H, either class) overlap: all 16-B entry indices distinct
    ent = np.concatenate([p, h]) // 16
    assert len(np.unique(ent)) == len(ent) == 4 * K * G
    # the ranges of the classes are disjoint as a whole, and P / H never share a 128-B half row
    c0 = t[cls == 0]
    c1 = t[cls == 1]
    assert c0[:, 4].max() + 16 <= c1[:, 3].min()
    assert set((p // 128).tolist()).isdisjoint((h // 128).tolist())
    # pack entries (the row offset of a symbol) fit uint16, the largest being 65,280
    packs = p[(cls == 0) & (j == 0)]
    assert np.array_equal(packs, np.arange(K) * 256) and packs.max() == 65280 <= 65535
    # the lane address is base + class offset + j 16 + pack: the class offset is one constant
    assert np.all(c1[:, 3] - c0[:, 3] == consts["class_off"])
    # bank quarters of the read's 64 banks: class 0's P rows on banks 0-31, class 1's on 32-63
    assert np.all((c0[:, 3] // 4) % 64 < 32) and np.all((c1[:, 3] // 4) % 64 >= 32)


def test_tool_mirrors_header(probe):
    import lds_banks
    consts, classes, t = probe
    assert lds_banks.split_row_bytes(G) == consts["row_bytes"] and lds_banks.split_hist_off(G) == consts["hist_off"]
    assert lds_banks.split_class_off(G) == consts["class_off"] and lds_banks.split_table_bytes(K, G) == consts["table_bytes"]
    assert [lds_banks.split_class(u) for u in range(64 // G)] == classes
    for c, o, j, p, h in t[:: 37]:
        assert lds_banks.split_p_off(G, int(c), int(o), int(j)) == p
    assert lds_banks.split_pack(G, K - 1) == 65280


@pytest.mark.parametrize("symbols", ["uniform", "equal"])
def test_bank_model_read_conflicts(symbols):
    """ds_read_b128 of the emission entry, LDS cycles per 16-lane group: the class-split tables are conflict-free
    on uniform and on all-equal symbols; the row tables pay 1.74 on uniform symbols."""
    import lds_banks
    rng = np.random.default_rng(0)
    split = lds_banks.read_cycles(G, G, K, rng, trials=2000, layout="split", symbols=symbols)
    assert split == 1.0
    rows = lds_banks.read_cycles(G, G, K, np.random.default_rng(0), trials=4000, layout="rows", symbols=symbols)
    if symbols == "uniform":
        assert round(rows, 2) == 1.74  # 1 + P(two of the colliding slot pairs share a parity) = 1.75 - O(1/K)
    else:
        assert rows == 1.0


def test_bank_model_adds_unchanged():
    """The histogram add's conflicts are out of the layout's reach, and it does not make them worse: the same
    cycles per group as the row tables on uniform, all-equal and two-valued symbols."""
    import lds_banks
    for symbols in ("uniform", "equal", "two"):
        a = lds_banks.add_cycles(G, G, K, np.random.default_rng(1), trials=500, layout="rows", symbols=symbols)
        b = lds_banks.add_cycles(G, G, K, np.random.default_rng(1), trials=500, layout="split", symbols=symbols)
        assert a == b, (symbols, a, b)


def test_bank_model_other_group_sizes():
    """Why G = 4 and G = 16 stay on the row tables: two classes leave G = 4 read conflicts, G = 16 has none."""
    import lds_banks
    rng = np.random.default_rng(0)
    assert lds_banks.read_cycles(4, 4, K, rng, trials=1000, layout="split") > 1.5
    assert lds_banks.read_cycles(16, 16, K, rng, trials=500, layout="rows") == 1.0
