#!/usr/bin/env python3
"""Kernel by kernel, is the gfx950 code of two builds the same?

    python scripts/compare_kernels.py <object dir A> <object dir B>          (e.g. the ldso_amd/_obj of two checkouts)

Takes the gfx950 code object out of every .o of both directories (the way ldso_amd/build.py's check_kernarg_segments does), and compares, for every kernel
symbol, whichever object it lives in: the instruction stream (mnemonic, operands and encoding of `llvm-objdump -d`, without the addresses) and the
.vgpr_count / .sgpr_count / .private_segment_fixed_size / .group_segment_fixed_size / .kernarg_segment_size notes.  Prints the compiler version, then one line
per kernel with its instruction count and `identical` or `differs`; exits 1 if any kernel differs or exists on one side only.  It compares and counts only."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
NOTES = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size", ".kernarg_segment_size")


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def code_object(obj, tmp):
    """The gfx950 code object inside a host object, or None (plain C++ units have no .hip_fatbin)."""
    fat, co = os.path.join(tmp, "k.fat"), os.path.join(tmp, "k.co")
    for f in (fat, co):
        if os.path.exists(f):
            os.remove(f)
    if subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", obj], capture_output=True).returncode != 0 or not os.path.exists(fat):
        return None
    run(f"{LLVM}/clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={co}", "--unbundle")
    return co if os.path.getsize(co) > 0 else None


def kernel_notes(co):
    """{kernel symbol: {note: value}} from the amdhsa.kernels records of the code object's metadata."""
    out, cur, indent = {}, None, None
    for line in run(f"{LLVM}/llvm-readelf", "--notes", co).splitlines():
        if line.strip() == "amdhsa.kernels:":
            indent = -1
            continue
        if indent is None:
            continue
        m = re.match(r"^(\s*)(- )?(\.\w+):\s*(.*)$", line)
        if not m:
            if line.strip() and not line.startswith(" "):
                indent = None          # left the list
            continue
        col = len(m.group(1))
        if indent == -1:
            indent = col
        if col == indent and m.group(2):          # a new kernel record
            cur = {}
        elif col != indent + 2:
            if col < indent:
                indent = None          # amdhsa.target / amdhsa.version follow the list
            continue                   # a field of an argument
        if cur is None:
            continue
        key, val = m.group(3), m.group(4).strip().strip("'")
        cur[key] = val
        if key == ".name":
            out[val] = cur
    return {k: {n: v.get(n) for n in NOTES} for k, v in out.items()}


def kernel_code(co, names):
    """{kernel symbol: [(instruction text, encoding), ...]} from the disassembly; the address column is dropped.  A kernel ends where its symbol's size says:
    the disassembler goes on to the next symbol, through the padding that aligns it (behind the last kernel of a unit: to the end of the section)."""
    size = {}
    for line in run(f"{LLVM}/llvm-readelf", "--symbols", "--wide", co).splitlines():          # Num: Value Size Type Bind Vis Ndx Name
        f = line.split()
        if len(f) == 8 and f[3] == "FUNC":
            size[f[7]] = int(f[2], 0)
    out, cur, end = {}, None, 0
    for line in run(f"{LLVM}/llvm-objdump", "-d", co).splitlines():
        m = re.match(r"^([0-9a-fA-F]+) <(.+)>:$", line)
        if m:
            cur = out.setdefault(m.group(2), []) if m.group(2) in names else None
            end = int(m.group(1), 16) + size.get(m.group(2), 0)
            continue
        if cur is None or "//" not in line:
            continue
        text, _, tail = line.partition("//")
        addr, _, enc = tail.partition(":")
        if int(addr, 16) < end:
            cur.append((" ".join(text.split()), enc.strip()))
    return out


def kernels(objdir):
    """{kernel symbol: (object file, notes, instructions)} over every object of a directory."""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for f in sorted(os.listdir(objdir)):
            if not f.endswith(".o"):
                continue
            co = code_object(os.path.join(objdir, f), tmp)
            if co is None:
                continue
            notes = kernel_notes(co)
            code = kernel_code(co, set(notes))
            for k, n in notes.items():
                out.setdefault(k, []).append((f, n, code.get(k, [])))
    # a kernel of internal linkage (_ZL...) may exist in several units under one name: those are told apart by their unit
    return {(k if len(v) == 1 else f"{k} @ {f}"): (f, n, c) for k, v in out.items() for f, n, c in v}


def main():
    if len(sys.argv) != 3:
        raise SystemExit(__doc__)
    print(run("hipcc", "--version").splitlines()[0] + " | " + run(f"{LLVM}/clang", "--version").splitlines()[0])
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b:
            print(f"{k}  only in {sys.argv[1] if k in a else sys.argv[2]} ({(a.get(k) or b.get(k))[0]})")
            bad += 1
            continue
        (fa, na, ca), (fb, nb, cb) = a[k], b[k]
        same = na == nb and ca == cb and len(ca) > 0
        bad += not same
        where = fa if fa == fb else f"{fa} -> {fb}"
        detail = "" if same else "  [" + ", ".join(([f"{len(ca)} -> {len(cb)} instructions" if len(ca) != len(cb) else "instruction stream"] if ca != cb else []) +
                                                      [f"{n} {na[n]} -> {nb[n]}" for n in NOTES if na[n] != nb[n]]) + "]"
        print(f"{k}  {where}  {len(cb)} instructions  vgpr {nb['.vgpr_count']} sgpr {nb['.sgpr_count']} scratch {nb['.private_segment_fixed_size']} lds {nb['.group_segment_fixed_size']} "
              f"kernarg {nb['.kernarg_segment_size']}  {'identical' if same else 'differs'}{detail}")
    print(f"{len(set(a) | set(b))} kernels, {bad} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
