"""Records the ctypes signatures `_native.lib()` / `verify_lib()` set, the exported names and the header's constants into
tests/golden/abi_signatures.json (tests/test_abi_host.py compares the loaded libraries with it).

Recorded at the commit BEFORE the bindings were read from the headers, i.e. from the hand-written table that the parser replaced:
run it again only to add an entry point, and review the diff of the JSON line by line -- it is the second statement of the ABI.

The names are ctypes' class names on LP64 Linux (`c_ulong` for uint64_t and size_t, `c_long` for int64_t, `LP_c_ulong` for size_t *),
the only platform the library is built for: the comparison by name holds there.

    python tests/golden/gen_abi_signatures.py          (needs the built libraries, no GPU)
"""
import ctypes as C
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from scalable_collision_avoidance_rl_amd import _native  # noqa: E402

CONSTANTS = ("MAX_K", "MAX_AGENTS", "MAX_OBSTACLES", "MAX_SENSE", "STATS_SCRATCH_DOUBLES", "EPISODE_REDUCE_DOUBLES",
             "OK", "EINVAL", "EUNSUPPORTED", "ELAUNCH", "CONTROL_PROPORTIONAL", "CONTROL_GRADIENT")


def signature(fn):
    """(restype, argtypes) by ctypes class name; an unset restype is ctypes' default c_int, unset argtypes those of `(void)`."""
    restype = C.c_int if fn.restype is None or fn.restype is C.c_int else fn.restype
    return {"restype": restype.__name__, "argtypes": [t.__name__ for t in (fn.argtypes or [])]}


def streamless(path, names):
    """Entries whose parameter list does not end in `void *stream` (a reading of the header of its own, not the binding's parser)."""
    text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    return [n for n in names if not re.search(r"\b%s\s*\([^)]*\bvoid\s*\*\s*stream\s*\)\s*;" % n, text)]


def main():
    lib, vlib = _native.lib(), _native.verify_lib()
    out = {"lib": {n: signature(getattr(lib, n)) for n in _native.SYMBOLS},
           "verify_lib": {n: signature(getattr(vlib, n)) for n in _native.VERIFY_SYMBOLS},
           "constants": {n: getattr(_native, n) for n in CONSTANTS},
           "no_stream": {"lib": streamless(_native.HEADER_PATH, _native.SYMBOLS),
                         "verify_lib": streamless(_native.VERIFY_HEADER_PATH, _native.VERIFY_SYMBOLS)}}
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "abi_signatures.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(len(out["lib"]), "+", len(out["verify_lib"]), "entries;", len(out["no_stream"]["lib"]), "without a stream")


if __name__ == "__main__":
    main()
