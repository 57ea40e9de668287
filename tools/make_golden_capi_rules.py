#!/usr/bin/env python
"""tests/golden/capi_rules.json: what the system-taking C entry points REFUSE, and in which order,
for the replay tests (tests/test_capi_rules_cpu.py, tests/test_gpu_capi_rules.py).  The cases, the
systems and the buffers are those of tests/_capi_rules.py; this tool runs them on a library built
from the commit whose behaviour is to be pinned -- the PARENT of a change to the argument rules,
before any source edit -- and writes down each return code and ol_last_error text.

    python tools/make_golden_capi_rules.py host     the entries of capi.hip, through the host-math
                                                    library (tests/hostmath; CPU only)
    python tools/make_golden_capi_rules.py device   ol_trace_forbes, ol_aim_rays and the
                                                    current-device rule, through the product
                                                    library on a GPU (OPTILAND_HIP_LIBRARY names
                                                    the library of the pinned commit)

    python tools/make_golden_capi_rules.py two_kinds  a range that holds rows of two one-launch
                                                    kinds (tests/_capi_rules.py: TWO_KINDS),
                                                    through the host-math library (CPU only)

    python tools/make_golden_capi_rules.py create   what staging refuses: single-fault calls of
                                                    ol_system_create and ol_system_update
                                                    (tests/_capi_rules.py: CREATE, UPDATE), through
                                                    the host-math library (CPU only)

Each run replaces its own section of the file and keeps the other.  `--commit HASH` names the
pinned commit (default: HEAD of a clean tree).
"""

from __future__ import annotations

import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)

from tests import _capi_rules as R  # noqa: E402


def _commit() -> str:
    if "--commit" in sys.argv:
        return sys.argv[sys.argv.index("--commit") + 1]
    dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain", "--", "optiland_amd", "include"],
                           capture_output=True, text=True, check=True).stdout.strip()
    if dirty:
        sys.exit(f"the sources differ from HEAD (name the pinned commit with --commit):\n{dirty}")
    return subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True,
                          check=True).stdout.strip()


def record(k: R.Context, entries: dict) -> dict:
    out = {}
    for name, entry in entries.items():
        cases = R.run(k, name, entry)
        accepted = set(entry["accepted"])
        for case, rc, text in cases:
            print(f"{name:24s} {case:40s} {rc:3d} {text}")
            assert text, (name, case, "empty text")
            if case.endswith(": accepted") or case in accepted:
                assert rc == 0, (name, case, rc, text)
            else:
                assert rc != 0, (name, case, "was accepted")
        assert len({c[0] for c in cases}) == len(cases), (name, "case names repeat")
        out[name] = cases
    return out


def main():
    section = sys.argv[1] if len(sys.argv) > 1 else ""
    if section not in ("host", "device", "two_kinds", "create"):
        sys.exit(__doc__)
    commit = _commit()
    if section == "host":
        from tests import _hostmath

        k = R.Context(_hostmath.load(), R.numpy_put)
        got = record(k, R.ENTRIES)
    elif section == "two_kinds":
        from tests import _hostmath

        k = R.Context(_hostmath.load(), R.numpy_put)
        got = R.two_kinds(k)
        for case, rc, text in got:
            print(f"{case:40s} {rc:3d} {text}")
            assert rc != 0 and text, (case, "was accepted")
    elif section == "create":
        from tests import _hostmath

        k = R.Context(_hostmath.load(), R.numpy_put)
        got = R.create(k.lib)
        assert [c[0] for c in got] == [c for c, _ in R.create_accepted()]
        assert len({c[0] for c in got}) == len(got), "case names repeat"
        for (case, rc, text), (_, accepted) in zip(got, R.create_accepted()):
            print(f"{case:48s} {rc:3d} {text}")
            assert text and (rc == 0) == accepted, (case, "accepted" if rc == 0 else "refused")
    else:
        import torch

        from optiland_amd import _capi

        assert torch.cuda.is_available(), "the device section needs a GPU"
        torch.zeros(1, device="cuda")
        k = R.Context(_capi.load(), R.torch_put)
        got = record(k, R.DEVICE_ENTRIES)
        if torch.cuda.device_count() >= 2:
            case = R.other_device(k)
            print(f"{'ol_trace_ex':24s} {case[0]:40s} {case[1]:3d} {case[2]}")
            assert case[1] != 0 and case[2]
            got["ol_trace_ex"] = [case]
        else:
            print("one device visible: the current-device rule is not recorded")
        torch.cuda.synchronize()
    k.close()
    doc = R.fixture() if os.path.exists(R.GOLD) else {}
    doc["n_rays"] = R.N
    doc.setdefault("parent", {})[section] = commit
    doc[section] = got
    with open(R.GOLD, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    cases = len(got) if section in ("two_kinds", "create") else sum(len(v) for v in got.values())
    print(f"{R.GOLD}: {cases} cases ({section}), commit {commit}")


if __name__ == "__main__":
    main()
