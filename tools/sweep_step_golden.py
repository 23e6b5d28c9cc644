#!/usr/bin/env python3
"""Writes tests/golden/sweep_step_parent.npz: x, y, iterations and status of the 12 + 12 + 12 seeded QPs
of tests/test_sweep_step.py (K = 8 with K = 9 in one grouped launch, K = 3 alone; default settings), as
the loaded library computes them on the GPU.  Run it with the library the results must not move away
from -- for a change to the stage sweeps, the parent commit built as a variant:

    make variant V=parent            (in a checkout of the parent commit; copy lib/libimpc_qp_parent.so here)
    IMPC_LIB_VARIANT=parent python tools/sweep_step_golden.py [out.npz]

The K = 8 / 9 launch is solved at three and at two teams per CU; the two must agree bit for bit before
anything is written."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tests", "", os.path.join("intent-mpc_amd", "python")):
    sys.path.insert(0, os.path.join(ROOT, p))

import impc  # noqa: E402
import test_sweep_step as t  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else t.GOLDEN
    ctx = impc.Context(0)
    arrays = {}
    try:
        for name in t.CASES:
            per = {}
            for n in (3, 2):
                os.environ[t.ENV] = str(n)
                res, _ = t.solve(ctx, t.cases()[name], impc.default_settings(verbose=0))
                per[n] = t.golden_arrays(name, res)
            for k in per[3]:
                if per[3][k].tobytes() != per[2][k].tobytes():
                    sys.exit(f"{k}: three and two teams per CU differ")
            arrays.update(per[3])
    finally:
        ctx.close()
    np.savez_compressed(out, **arrays)
    print(impc.lib.impc_build_id().decode(), out, os.path.getsize(out), "bytes", {k: v.shape for k, v in arrays.items()})


if __name__ == "__main__":
    main()
