#!/usr/bin/env python3
"""Is the device code of two builds the same?  CPU only: nothing here runs a kernel.

    tools/isa_identity.py PARENT NEW [--libs PARENT.so NEW.so] [-j JOBS]

PARENT and NEW are each an object directory (hmm_training_amd/_obj/<tag>, as build() leaves it) or a checkout;
a checkout is built first, with its own hmm_training_amd/build.py, into the tag `isa_identity` and a scratch
library.  From every object of both sides the gfx950 code object is unbundled (llvm-objcopy
--dump-section=.hip_fatbin, clang-offload-bundler --unbundle) and disassembled (llvm-objdump -d).  Compared per
kernel: the instruction text (operands and branch offsets included, addresses and encodings dropped) and, from the
code object's notes (llvm-readelf --notes), the agpr / vgpr / sgpr counts, the group (LDS) and private (scratch)
segment sizes and the spill counts.  A kernel is paired with the one of its name in the same unit; one that a unit
has on one side only (it moved to another unit, or its unit is new) is paired by name across the units.  Then the
exported hmmbw_ symbols of the two libraries (the objects linked as
build() links them, unless --libs names them).  Prints one line per translation unit, the differing kernels
under it, and exits 1 on any difference.  The text is only compared and hashed; what the instructions are is
not looked at.  profiles/r8/isa_identity.txt and profiles/r9/isa_identity.txt are this table.
"""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import glob
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
ARCH = os.environ.get("HMMBW_ARCH", "gfx950")
FIGURES = ("agpr_count", "vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
           "sgpr_spill_count", "vgpr_spill_count")


def tool(name: str) -> str:
    for d in ("llvm/bin", "lib/llvm/bin", "bin"):
        p = os.path.join(ROCM, d, name)
        if os.path.exists(p):
            return p
    return name


def run(cmd, **kw) -> subprocess.CompletedProcess:
    return subprocess.run(cmd, capture_output=True, text=True, **kw)


def code_object(obj: str, tmp: str):
    """The gfx950 code object of a host object, or None when the unit has no device code."""
    stem = os.path.join(tmp, os.path.basename(obj)[:-2])
    fat, co = stem + ".hipfb", stem + ".co"
    r = run([tool("llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", obj, stem + ".copy.o"])
    if r.returncode != 0 or not os.path.exists(fat) or os.path.getsize(fat) == 0:
        return None
    r = run([tool("clang-offload-bundler"), "--unbundle", "--type=o", f"--targets=hipv4-amdgcn-amd-amdhsa--{ARCH}",
             f"--input={fat}", f"--output={co}"])
    if r.returncode != 0:
        raise RuntimeError(f"{obj}: {r.stderr.strip()}")
    return co if os.path.getsize(co) else None


def streams(co: str) -> dict:
    """symbol -> its instruction lines, address and encoding comments dropped."""
    r = run([tool("llvm-objdump"), "-d", co])
    if r.returncode != 0:
        raise RuntimeError(f"{co}: {r.stderr.strip()}")
    out, cur = {}, None
    for line in r.stdout.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line[:1] in " \t" and line.strip():
            cur.append(line.split("//", 1)[0].strip())
    # the fill between a symbol's last instruction and the next symbol's alignment (the end of the code object
    # after the last one) depends on what follows it in the unit, not on the kernel
    for v in out.values():
        while v and v[-1] in ("s_nop 0", "s_code_end"):
            v.pop()
    return out


def figures(co: str) -> dict:
    """kernel -> its resource figures, from the amdhsa.kernels list of the code object's notes."""
    r = run([tool("llvm-readelf"), "--notes", co])
    if r.returncode != 0:
        raise RuntimeError(f"{co}: {r.stderr.strip()}")
    out, entry, indent, inside = {}, None, None, False
    for line in r.stdout.splitlines():
        if line.strip() == "amdhsa.kernels:":
            inside, indent = True, None
            continue
        if not inside:
            continue
        m = re.match(r"^(\s*)(- )?\.(\w+):\s*(.*)$", line)
        if m is None:
            if re.match(r"^\s*amdhsa\.", line):
                inside = False
            continue
        col = len(m.group(1)) + (2 if m.group(2) else 0)  # column of the key
        if m.group(2) and (indent is None or col == indent):
            indent = col
            entry = {}
            out[len(out)] = entry
        if entry is not None and col == indent and (m.group(3) in FIGURES or m.group(3) == "name"):
            entry[m.group(3)] = m.group(4).strip("'\"")
    return {e["name"]: tuple(e.get(k, "-") for k in FIGURES) for e in out.values() if "name" in e}


def unit(obj: str, tmp: str):
    co = code_object(obj, tmp)
    if co is None:
        return {}, {}
    return streams(co), figures(co)


def exported(lib: str) -> set:
    r = run([tool("llvm-readelf"), "--dyn-syms", "-W", lib])
    if r.returncode != 0:
        raise RuntimeError(f"{lib}: {r.stderr.strip()}")
    names = set()
    for line in r.stdout.splitlines():
        f = line.split()
        if len(f) == 8 and f[6] != "UND" and f[7].startswith("hmmbw_"):
            names.add(f[7].split("@")[0])
    return names


def resolve(path: str, tmp: str, side: str):
    """(object directory, library or None) of an object directory or a checkout."""
    if glob.glob(os.path.join(path, "*.o")):
        return path, None
    if not os.path.exists(os.path.join(path, "hmm_training_amd", "build.py")):
        sys.exit(f"{path}: neither an object directory nor a checkout")
    lib = os.path.join(tmp, f"libhmmbw_{side}.so")
    code = f"from hmm_training_amd.build import build; build(force=True, out={lib!r}, tag='isa_identity')"
    r = run([sys.executable, "-c", code], cwd=path)
    if r.returncode != 0:
        sys.exit(f"{path}: build failed\n{r.stderr}")
    return os.path.join(path, "hmm_training_amd", "_obj", "isa_identity"), lib


def link(objdir: str, out: str) -> str:
    hipcc = os.environ.get("HIPCC", os.path.join(ROCM, "bin", "hipcc"))
    r = run([hipcc, "-shared", "-fPIC", f"--offload-arch={ARCH}", *sorted(glob.glob(os.path.join(objdir, "*.o"))), "-o", out])
    if r.returncode != 0:
        sys.exit(f"{objdir}: link failed\n{r.stderr}")
    return out


def sha(lines) -> str:
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16]


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--libs", nargs=2, metavar=("PARENT.so", "NEW.so"), help="compare these libraries' exports")
    ap.add_argument("-j", type=int, default=max(1, min(16, os.cpu_count() or 1)))
    args = ap.parse_args()
    same = True
    with tempfile.TemporaryDirectory() as tmp:
        sides = []
        for side, path in (("parent", args.parent), ("new", args.new)):
            os.makedirs(os.path.join(tmp, side))
            sides.append(resolve(path, tmp, side))
        stems = sorted({os.path.basename(o)[:-2] for d, _ in sides for o in glob.glob(os.path.join(d, "*.o"))})
        jobs = [(os.path.join(d, s + ".o"), os.path.join(tmp, side)) for s in stems
                for side, (d, _) in zip(("parent", "new"), sides)]
        with cf.ThreadPoolExecutor(max_workers=args.j) as ex:
            res = list(ex.map(lambda j: unit(*j) if os.path.exists(j[0]) else None, jobs))
        print("# per translation unit: kernels, instructions, sha256 of all instruction text (parent == new?), "
              "resource figures equal?")
        # symbols a unit has on one side only (a kernel that moved unit, a unit that is new): paired by name below
        lost, found = {}, {}
        for i, s in enumerate(stems):
            (sa, fa), (sb, fb) = res[2 * i] or ({}, {}), res[2 * i + 1] or ({}, {})
            lost.update({k: (s, sa[k], fa.get(k)) for k in sa if k not in sb})
            found.update({k: (s, sb[k], fb.get(k)) for k in sb if k not in sa})
            if res[2 * i] is None or res[2 * i + 1] is None:
                print(f"{s:<18} only in {'new' if res[2 * i] is None else 'parent'}: {len(sa) + len(sb)} symbols, by name below")
                continue
            both = sorted(set(sa) & set(sb))
            text = [sha([f"{k}:"] + sa[k]) for k in both], [sha([f"{k}:"] + sb[k]) for k in both]
            ok_s = all(sa[k] == sb[k] for k in both)
            ok_f = all(fa.get(k) == fb.get(k) for k in both)
            same = same and ok_s and ok_f
            moved = f" ({len(sa) - len(both)} left, {len(sb) - len(both)} joined: by name below)" if len(sa) != len(both) or len(sb) != len(both) else ""
            print(f"{s:<18} kernels {sum(k in fa for k in both):4d} instructions {sum(len(sa[k]) for k in both):9d} "
                  f"sha {sha(text[0])} / {sha(text[1])} streams {'identical' if ok_s else 'DIFFER'} "
                  f"figures {'identical' if ok_f else 'DIFFER'}{moved}")
            for k in both:
                if sa[k] != sb[k] or fa.get(k) != fb.get(k):
                    na, nb = len(sa[k]), len(sb[k])
                    inplace = f" ({sum(x != y for x, y in zip(sa[k], sb[k]))} lines differ in place)" if na == nb else ""
                    print(f"    {k}: instructions {na} -> {nb}{inplace}"
                          + ("" if fa.get(k) == fb.get(k) else f"; {', '.join(FIGURES)}: {fa.get(k)} -> {fb.get(k)}"))
        if lost or found:
            print("# symbols whose unit changed, paired by name: parent unit -> new unit")
        for k in sorted(set(lost) | set(found)):
            if k not in lost or k not in found:
                same = False
                print(f"    {k}: only in {'parent ' + lost[k][0] if k in lost else 'new ' + found[k][0]}")
                continue
            (ua, xa, ga), (ub, xb, gb) = lost[k], found[k]
            ok_s, ok_f = xa == xb, ga == gb
            same = same and ok_s and ok_f
            print(f"    {k}: {ua} -> {ub} instructions {len(xa)} -> {len(xb)} streams {'identical' if ok_s else 'DIFFER'} "
                  f"figures {'identical' if ok_f else 'DIFFER'}" + ("" if ok_f else f"; {', '.join(FIGURES)}: {ga} -> {gb}"))
        libs = args.libs or [lib or link(d, os.path.join(tmp, f"libhmmbw_{side}.so"))
                             for side, (d, lib) in zip(("parent", "new"), sides)]
        ea, eb = exported(libs[0]), exported(libs[1])
        same = same and ea == eb
        print(f"# exported hmmbw_ symbols: parent {len(ea)}, new {len(eb)}, "
              + ("same set" if ea == eb else f"only parent {sorted(ea - eb)}, only new {sorted(eb - ea)}"))
    print("# every unit identical" if same else "# DIFFERENCES above")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
