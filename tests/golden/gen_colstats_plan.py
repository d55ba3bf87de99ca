#!/usr/bin/env python3
"""Record tests/golden/colstats_plan.npz: the workspace sizes `dronesim_standardize_workspace` and `dronesim_obsnorm_workspace`
return over the grid of tests/test_colstats_plan_host.py, from the library given on the command line -- the build of the commit
BEFORE csrc/colstats_common.hpp, when each of the two files planned for itself:

    python tests/golden/gen_colstats_plan.py <that build's libdronesim.so>

run from the repository root.  The queries make no HIP call, so this needs no GPU.  `rows`, `cols`: the grid; `bytes`
[2, rows, cols] int64: standardize, obsnorm."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import torch  # noqa: E402,F401  (the library binds to the HIP runtime torch ships, as in _native.lib())

from tests import test_colstats_plan_host as T  # noqa: E402

if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    out = T.workspaces(C.CDLL(os.path.abspath(sys.argv[1])))
    np.savez_compressed(T.GOLDEN, rows=np.array(T.ROWS, dtype=np.int64), cols=np.array(T.COLS, dtype=np.int64), bytes=out)
    print(f"{T.GOLDEN}: {out.size} sizes, {os.path.getsize(T.GOLDEN)} bytes")
