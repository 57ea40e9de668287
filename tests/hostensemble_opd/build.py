"""Build tests/hostensemble_opd/_build/hostensemble_opd (and hostensemble_opd_asan): the wavefront
cells of optiland_amd/csrc/ensemble_opd_device.h compiled for the HOST as a stand-alone program --
a checker for boxes without a GPU.  See main.hip for what it is and is not.

    python tests/hostensemble_opd/build.py [--sanitize]

The recipe is `build_program` of tests/hostmath/build.py: main.hip with that build's flags, linked
with the two objects it leaves behind (the host-only csrc/capi.hip and the stand-in HIP runtime of
tests/hostmath/harness.hip), plain or with AddressSanitizer + UndefinedBehaviorSanitizer.
"""

from __future__ import annotations

import importlib.util
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def _hostmath():
    spec = importlib.util.spec_from_file_location(
        "_hostmath_build", os.path.join(HERE, "..", "hostmath", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def available() -> bool:
    return _hostmath().available()


def build(force: bool = False, verbose: bool = False, sanitize: bool = False) -> str:
    return _hostmath().build_program("hostensemble_opd", os.path.join(HERE, "main.hip"),
                                     force=force, verbose=verbose, sanitize=sanitize)


if __name__ == "__main__":
    import sys
    print(build(force=True, verbose=True, sanitize="--sanitize" in sys.argv))
