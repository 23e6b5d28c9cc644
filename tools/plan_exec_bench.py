#!/usr/bin/env python3
"""Device time of the plan-execution calls next to the replan they follow: I planning instances on
the live loop (scenarios.live_loop: N = 30, K = 4 by default), a first plan and chained fan-out
replans as tools/live_loop.py runs them, and after every replan one impc_replan_target_device (the
yaw look-ahead, IMPC_YAW_SMOOTH) and one impc_replan_check_device (map + boxes), each between two HIP
events on the context stream (the context's step timer).  The boxes are the replan's current
obstacles with 0.8 m sizes, the map an empty 1 m grid around the flight, realTime spread over 0..1.2 s.
Every shape is warmed by the first replan, which is not counted.  Prints one JSON line; --out also
writes it to a file."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "intent-mpc_amd", "python")]
import impc  # noqa: E402
from impc import execution as E  # noqa: E402
from impc import perception as P  # noqa: E402
from impc import scenarios  # noqa: E402
from impc.replan import DeviceReplan  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=8192)
    ap.add_argument("--obstacles", type=int, default=4)
    ap.add_argument("--horizon", type=int, default=30)
    ap.add_argument("--replans", type=int, default=8)
    ap.add_argument("--calls", type=int, default=10, help="target / check calls timed after every replan")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    I, K, N, R = a.instances, a.obstacles, a.horizon, a.replans
    sc = scenarios.live_loop(I, K, R, N=N, seed=4100)
    p, pd, L = sc["params"], sc["pd"], sc["L"]
    ctx = impc.Context(0)
    rp = DeviceReplan(ctx, p, pd, I, K, L, impc.default_settings(verbose=0))
    paths = impc.ReferencePaths(ctx, list(sc["paths"]), pd["ts"], N)
    Dv, c = impc.DeviceArray, np.ascontiguousarray
    pos_d, vel_d, xref_d = Dv(ctx, c(sc["pos0"])), Dv(ctx, c(sc["vel0"])), Dv(ctx, (I, N, 8))
    psize_d, prob_d = Dv(ctx, c(sc["pred_size"])), Dv(ctx, c(sc["prob"]))
    pred_d, cur_d = Dv(ctx, c(sc["pred_pos"])), Dv(ctx, c(sc["dyn_cur"]))
    step_pred, step_cur = pred_d.nbytes // R, cur_d.nbytes // R
    allp = np.concatenate([sc["paths"].reshape(-1, 3), sc["dyn_cur"].reshape(-1, 3)])
    lo, hi = np.floor(allp.min(axis=0) - 20.0), np.ceil(allp.max(axis=0) + 20.0)
    dims = [int(v) for v in hi - lo]
    omap = P.occ_map(lo.tolist(), 1.0, dims)
    occ_d = Dv(ctx, np.zeros(int(np.prod(dims)), np.uint8))
    t_d = Dv(ctx, np.random.default_rng(1).uniform(0.0, 1.2, I))
    yaw_d = Dv(ctx, np.zeros(I))
    nobs_d = Dv(ctx, np.full(I, K, np.int32))
    size_d = Dv(ctx, np.full((I, K, 3), 0.8))
    tgt, chk = E.TargetBuffers(ctx, I), E.CheckBuffers(ctx, I)
    for r in range(R):
        paths.xref_device(pos_d.ptr, xref_d.ptr)
        ctx.timer_mark()
        rp.run_device(pos_d.ptr, vel_d.ptr, xref_d.ptr, cur_d.ptr + r * step_cur, pred_d.ptr + r * step_pred,
                      psize_d.ptr, prob_d.ptr)
        ctx.timer_mark()
        for _ in range(a.calls):
            ctx.timer_mark()
            E.target_device(rp, E.YAW_SMOOTH, t_d.ptr, pos_d.ptr, yaw_d.ptr, **tgt.ptrs())
            ctx.timer_mark()
            ctx.timer_mark()
            E.check_device(rp, t_d.ptr, pos_d.ptr, omap=omap, occ=occ_d.ptr, num_obs=nobs_d.ptr,
                           ob_pos=cur_d.ptr + r * step_cur, ob_size=size_d.ptr, **chk.ptrs())
            ctx.timer_mark()
        rp.advance_device(pd["ts"], pos_d.ptr, vel_d.ptr)
        ctx.synchronize()
    ms = ctx.timer_read(max_pairs=R * (1 + 2 * a.calls)).reshape(R, 1 + 2 * a.calls)
    replan_ms, target_ms, check_ms = ms[1:, 0], ms[1:, 1::2].reshape(-1), ms[1:, 2::2].reshape(-1)
    got, flags = tgt.get(), chk.get()
    _, _, _, valid = rp.plans()
    med = lambda v: float(np.median(v))  # noqa: E731
    line = json.dumps({
        "workload": f"plan execution after the live loop's replan: {I} instances, N={N}, K={K}, {R - 1} fan-out replans, "
                    f"{a.calls} target (IMPC_YAW_SMOOTH) and check (map + {K} boxes) calls after each",
        "instances": I, "horizon": N, "obstacles": K, "kernel_form": "one wavefront per instance",
        "target_ms_median": med(target_ms), "target_ms_min": float(target_ms.min()), "target_ms_max": float(target_ms.max()),
        "check_ms_median": med(check_ms), "check_ms_min": float(check_ms.min()), "check_ms_max": float(check_ms.max()),
        "replan_ms_median": med(replan_ms), "replan_ms": replan_ms.tolist(),
        "timing": "HIP events on the context stream around each call (impc_ctx_timer_mark); first replan not counted",
        "valid_plans": int(valid.sum()), "done": int(got["done"].sum()), "look_ahead_hits": int((got["yaw_step"] >= 0).sum()),
        "replan_flags": int(flags["replan_flag"].sum()),
        "thread_per_instance_form": "not measured", "build_id": impc.lib.impc_build_id().decode()})
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    for d in (pos_d, vel_d, xref_d, psize_d, prob_d, pred_d, cur_d, occ_d, t_d, yaw_d, nobs_d, size_d):
        d.free()
    tgt.free()
    chk.free()
    paths.close()
    rp.close()
    ctx.close()


if __name__ == "__main__":
    main()
