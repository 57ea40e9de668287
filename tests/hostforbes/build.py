"""Build tests/hostforbes/_build/hostforbes (and hostforbes_asan): the Forbes surface step of
optiland_amd/csrc/forbes_device.h compiled for the HOST as a stand-alone program -- a checker
for boxes without a GPU.  See main.hip for what it is and is not.

    python tests/hostforbes/build.py [--sanitize]

main.hip is compiled with the flags of tests/hostmath/build.py and linked with the two objects
that build leaves behind (the host-only csrc/capi.hip and the stand-in HIP runtime of
tests/hostmath/harness.hip).  `sanitize=True`: all three with AddressSanitizer +
UndefinedBehaviorSanitizer, the runtime linked INTO the program -- it runs as an ordinary child
process, nothing is preloaded.
"""

from __future__ import annotations

import importlib.util
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "optiland_amd", "csrc")
OUT = os.path.join(HERE, "_build")


def _hostmath():
    spec = importlib.util.spec_from_file_location(
        "_hostmath_build", os.path.join(HERE, "..", "hostmath", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def available() -> bool:
    return _hostmath().available()


def build(force: bool = False, verbose: bool = False, sanitize: bool = False) -> str:
    hm = _hostmath()
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    os.makedirs(OUT, exist_ok=True)
    suffix = "_asan" if sanitize else ""
    exe = os.path.join(OUT, "hostforbes" + suffix)
    objs = [os.path.join(hm.OUT, f"{name}{suffix}.o") for name in ("capi", "harness")]
    src = os.path.join(HERE, "main.hip")
    # (the SOURCES decide, not the objects: a tree that travels without its object files keeps a
    # program that is up to date)
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")] + [
        src, os.path.join(CSRC, "capi.hip"), os.path.join(HERE, "..", "hostmath", "harness.hip"),
        os.path.join(ROOT, "include", "optiland_hip.h"), os.path.abspath(__file__)]
    if not force and os.path.exists(exe) and \
            all(os.path.getmtime(d) <= os.path.getmtime(exe) for d in deps):
        return exe
    hm.build(force=force, verbose=verbose, sanitize=sanitize)   # capi.o / harness.o up to date
    if not all(os.path.exists(o) for o in objs):   # (a library that travelled without its objects)
        hm.build(force=True, verbose=verbose, sanitize=sanitize)
    flags = ["--offload-host-only", "-std=c++17", "-fPIC", "-ffp-contract=on", "-fno-math-errno",
             "-Wall"] + (["-mfma"] if hm._cpu_has_fma() else [])
    flags += ["-O1", "-g1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
              "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    obj = os.path.join(OUT, f"main{suffix}.o")
    cmd = [hipcc, *flags, "-c", src, "-o", obj]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd, stderr=None if verbose else subprocess.DEVNULL)
    if sanitize:
        clang = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "lib", "llvm", "bin",
                             "clang++")
        if not os.path.exists(clang):
            clang = "/opt/rocm/lib/llvm/bin/clang++"
        cmd = [clang, "-fsanitize=address,undefined", obj, *objs, "-o", exe]
    else:
        cmd = ["g++", obj, *objs, "-o", exe]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return exe


if __name__ == "__main__":
    import sys
    print(build(force=True, verbose=True, sanitize="--sanitize" in sys.argv))
