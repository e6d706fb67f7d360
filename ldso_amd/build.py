"""Build libldso_hip.so (gfx950) in-tree with hipcc.  No JIT cache: the .so travels with the repo snapshot."""
from __future__ import annotations

import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(HERE, "libldso_hip.so")
SOURCES = ["ba_linearize.hip", "ba_linearize_batch.hip", "ba_reduce.hip", "ba_solve.hip", "ba_solve_batch.hip", "ba_step.hip", "ba_api.hip", "ba_window.hip", "ba_optimize.hip", "ba_batch.hip", "ba_dist.hip", "tracker.hip", "tracker_ref.hip", "tracker_api.hip", "tracker_group.hip", "tracker_hyp.cpp",
           "images.hip", "trace.hip", "trace_group.hip", "ba_activate.hip", "act_select.hip", "initializer.hip", "initializer_api.hip", "initializer_sched.cpp", "init_first.hip", "init_nn_tree.cpp", "features.hip", "pixel_select.hip", "undistort.hip"]
# -ffp-contract=off: elementwise arithmetic is IEEE and follows the reference's operation order (bit-identical
# energies / residual states); fused multiply-adds are spelled explicitly where they are wanted.
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wno-unused-result"]
if os.environ.get("LDSO_STAMPS"):          # device-side phase stamps for scripts/dbg_gn.py (debug builds only, see ba_dev.h)
    FLAGS.append("-DLDSO_STAMPS")


FLAGFILE = os.path.join(HERE, "_obj", "flags.txt")


def flags_changed() -> bool:
    """Objects built with other flags (e.g. a LDSO_STAMPS debug build) must not be reused."""
    try:
        return open(FLAGFILE).read() != " ".join(FLAGS)
    except OSError:
        return True


def needs_build() -> bool:
    if not os.path.exists(OUT) or flags_changed():
        return True
    t = os.path.getmtime(OUT)
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC)] + [os.path.join(HERE, "..", "include", f) for f in ("ldso_hip.h", "ldso_window.h")]
    return any(os.path.getmtime(d) > t for d in deps)


# ld_touch_kernarg<LINES>() (csrc/ba_dev.h) requests one dword of each of the first LINES 64-byte lines of a kernel's argument block at kernel entry.  The
# static_asserts beside the calls bound the EXPLICIT arguments only; two kernels (k_linearize_one: 16 lines, the argument-based k_linearize: 14) also reach into
# the hidden arguments behind them.  What actually bounds the loads is .kernarg_segment_size of the code object: checked here, from the objects that get linked,
# so that another code-object version / compiler that trims the hidden block fails the BUILD instead of reading past the segment.
KERNARG_TOUCH = {"k_linearize_one": 16, "k_linearize": 14, "k_reduce_solve": 12, "k_gn_solve": 10, "k_reduce": 8}


def check_kernarg_segments() -> None:
    import re
    import tempfile
    llvm = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(os.path.join(llvm, "llvm-readelf")):
        return
    seen = set()
    with tempfile.TemporaryDirectory() as tmp:
        for s in ("ba_linearize.hip", "ba_reduce.hip", "ba_solve.hip"):
            o, fat, co = os.path.join(HERE, "_obj", s + ".o"), os.path.join(tmp, "k.fat"), os.path.join(tmp, "k.co")
            if subprocess.run([f"{llvm}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", o], capture_output=True).returncode != 0:
                raise RuntimeError(f"kernarg check: no .hip_fatbin in {o}")
            subprocess.run([f"{llvm}/clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={co}", "--unbundle"],
                           check=True, capture_output=True)
            notes = subprocess.run([f"{llvm}/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
            size = None
            for line in notes.splitlines():
                m = re.search(r"\.kernarg_segment_size:\s*(\d+)", line)
                if m:
                    size = int(m.group(1))
                m = re.search(r"\.name:\s*(\S+)", line)          # .name follows .kernarg_segment_size inside a kernel's record (keys are sorted)
                if m and size is not None:
                    mangled = m.group(1)
                    for kn, lines in KERNARG_TOUCH.items():
                        if mangled.startswith(f"_Z{len(kn)}{kn}"):          # _Z<len><name>...: the length prefix makes this the exact kernel name (plain or template)
                            need = (lines - 1) * 64 + 4
                            if size < need:
                                raise RuntimeError(f"{mangled}: kernarg segment of {size} bytes, ld_touch_kernarg<{lines}> reads up to byte {need}")
                            seen.add(kn)
                    size = None
    missing = set(KERNARG_TOUCH) - seen
    if missing:
        raise RuntimeError(f"kernarg check: kernels not found in the code objects: {sorted(missing)}")


def build(force: bool = False, verbose: bool = False) -> str:
    if not force and not needs_build():
        return OUT
    objs = []
    os.makedirs(os.path.join(HERE, "_obj"), exist_ok=True)
    force = force or flags_changed()
    procs = []
    for s in SOURCES:
        src = os.path.join(CSRC, s)
        if not os.path.exists(src):
            continue
        o = os.path.join(HERE, "_obj", s + ".o")
        objs.append(o)
        if not force and os.path.exists(o) and all(os.path.getmtime(o) > os.path.getmtime(os.path.join(CSRC, f)) for f in os.listdir(CSRC) if f.endswith(".h") or f == s) \
                and os.path.getmtime(o) > os.path.getmtime(os.path.join(HERE, "..", "include", "ldso_hip.h")) \
                and os.path.getmtime(o) > os.path.getmtime(os.path.join(HERE, "..", "include", "ldso_window.h")):
            continue
        cmd = ["hipcc", *FLAGS, *(["-x", "c++", "-fvisibility-inlines-hidden"] if s.endswith(".cpp") else []), "-c", src, "-o", o]          # .cpp: host arithmetic only, plain C++
        if verbose:
            print(" ".join(cmd))
        procs.append((s, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    for s, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            sys.stderr.write(out)
            raise RuntimeError(f"hipcc failed on {s}")
        if verbose and out.strip():
            print(out)
    check_kernarg_segments()
    cmd = ["hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", *objs, "-o", OUT]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout)
        raise RuntimeError("link failed")
    with open(FLAGFILE, "w") as f:
        f.write(" ".join(FLAGS))
    return OUT


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
