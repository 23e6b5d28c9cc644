#!/usr/bin/env python3
"""Device time of impc_cluster_run_device (include/impc_cluster.h): I planning instances with the
live launch's parameters (planner_param.yaml: cloud_res 0.2, region 6 x 4 m, z 0.5 .. 3.0) on a
seeded inflated map of boxes and pillars, each call between two HIP events on the context stream
(impc_ctx_timer_mark), the median of --calls calls after --warmup warm-up calls.  For scale, the
serial form of the same arithmetic (tests/native/cluster_harness.cpp, cluster_serial) on the same
inputs with --threads host threads, and how many instances agree with it on count, flags and boxes.
Prints one JSON line; --out also writes it to a file."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "intent-mpc_amd", "python")]
import impc  # noqa: E402
from impc import clustering as CL  # noqa: E402


def scene(seed, extent, height, res, boxes, pillars, inflate):
    """the inflated grid of a square map with random boxes and pillars (inflate voxels each way)"""
    rng = np.random.default_rng(seed)
    dims = (int(extent / res), int(extent / res), int(height / res))
    occ = np.zeros(dims, np.uint8)

    def put(lo, hi):
        a = [max(int(np.floor(lo[k] / res)) - inflate, 0) for k in range(3)]
        b = [min(int(np.ceil(hi[k] / res)) + inflate, dims[k]) for k in range(3)]
        occ[a[0]:b[0], a[1]:b[1], a[2]:b[2]] = 1

    for _ in range(boxes):
        c, s = rng.uniform(2.0, extent - 2.0, 2), rng.uniform(0.4, 2.5, 2)
        h = rng.uniform(1.0, height)
        put((c[0] - s[0] / 2, c[1] - s[1] / 2, 0.0), (c[0] + s[0] / 2, c[1] + s[1] / 2, h))
    for _ in range(pillars):
        c, r = rng.uniform(2.0, extent - 2.0, 2), rng.uniform(0.1, 0.3)
        put((c[0] - r, c[1] - r, 0.0), (c[0] + r, c[1] + r, height))
    return occ, dims, rng


def kernel_regs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), impc.LIB_PATH, "k_cluster"],
                         capture_output=True, text=True)
    return out.stdout.strip() if out.returncode == 0 and out.stdout.strip() else "not measured"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=8192)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--max-points", type=int, default=4096)
    ap.add_argument("--max-boxes", type=int, default=32)
    ap.add_argument("--boxes", type=int, default=24)
    ap.add_argument("--pillars", type=int, default=40)
    ap.add_argument("--seed", type=int, default=1400)
    ap.add_argument("--no-host", action="store_true", help="skip the host harness")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    I, P, S = a.instances, a.max_points, a.max_boxes
    extent, height, res = 60.0, 4.0, 0.1
    occ, dims, rng = scene(a.seed, extent, height, res, a.boxes, a.pillars, inflate=2)
    pr = CL.cluster_params(**CL.LIVE_PARAMS, max_points=P, max_boxes=S)
    omap = impc.OccMap(resolution=res)
    omap.dims[:] = dims
    map_max = [dims[k] * res for k in range(3)]
    pos = np.column_stack([rng.uniform(6.0, extent - 6.0, (I, 2)), rng.uniform(0.8, 1.6, I)])
    yaw, speed = rng.uniform(-np.pi, np.pi, I), rng.uniform(0.5, 2.0, I)
    vel = np.column_stack([speed * np.cos(yaw), speed * np.sin(yaw), np.zeros(I)])

    ctx = impc.Context(0)
    sc = CL.StaticClusters(ctx, pr, I, debug=("num_points", "num_initial"))
    D = impc.DeviceArray
    occ_d, pos_d, vel_d = D(ctx, occ), D(ctx, pos), D(ctx, vel)
    total = a.warmup + a.calls
    for _ in range(total):
        ctx.timer_mark()
        sc.run_device(pos_d.ptr, vel_d.ptr, omap, map_max, occ_d.ptr)
        ctx.timer_mark()
    ctx.synchronize()
    ms = ctx.timer_read(max_pairs=total)[a.warmup:]
    got = sc.get()
    ok = got["flags"] == 0

    host = dict(seconds="not measured", agree="not measured")
    if not a.no_host:
        lib = C.CDLL(os.path.join(ROOT, "tests", "native", "build", "libcluster_harness.so"))
        lib.cluster_serial.restype = C.c_int
        lib.cluster_serial.argtypes = [C.POINTER(CL.ClusterParams), C.c_int64, C.POINTER(CL.ClusterIn),
                                       C.POINTER(CL.ClusterOut), C.c_int]
        st = dict(heading=np.zeros(I), count=np.zeros(I, np.int32), centroid=np.zeros((I, S, 3)), size=np.zeros((I, S, 3)),
                  yaw=np.zeros((I, S)), flags=np.zeros(I, np.int32))
        ci = CL.ClusterIn(cur_pos=pos.ctypes.data, cur_vel=vel.ctypes.data, occ_inflated=occ.ctypes.data)
        ci.map = omap
        ci.map_max[:] = map_max
        co = CL.ClusterOut(**{k: v.ctypes.data for k, v in st.items()})
        t0 = time.perf_counter()
        assert lib.cluster_serial(C.byref(pr), I, C.byref(ci), C.byref(co), a.threads) == 0
        host["seconds"] = time.perf_counter() - t0
        same = (st["count"] == got["count"]) & (st["flags"] == got["flags"])
        for k in ("centroid", "size", "yaw"):
            same &= (st[k].reshape(I, -1) == got[k].reshape(I, -1)).all(axis=1)
        host["agree"] = int(same.sum())

    line = json.dumps({
        "workload": f"static-obstacle clustering: {I} instances, live parameters (cloud_res 0.2, region 6 x 4 m, z 0.5-3.0), "
                    f"{extent:.0f} m map at {res} m with {a.boxes} boxes and {a.pillars} pillars (seed {a.seed}), "
                    f"max_points {P}, max_boxes {S}",
        "instances": I, "kernel_form": "one 256-thread workgroup per instance, one wavefront per tree node",
        "device_ms_median": float(np.median(ms)), "device_ms_min": float(ms.min()), "device_ms_max": float(ms.max()),
        "calls": int(a.calls), "warmup": int(a.warmup),
        "timing": "HIP events on the context stream around each call (impc_ctx_timer_mark)",
        "points_mean": float(got["num_points"].mean()), "points_max": int(got["num_points"].max()),
        "initial_clusters_mean": float(got["num_initial"][ok].mean()) if ok.any() else 0.0,
        "boxes_mean": float(got["count"][ok].mean()) if ok.any() else 0.0, "boxes_max": int(got["count"].max()),
        "flagged": {"points": int((got["flags"] & 1 != 0).sum()), "boxes": int((got["flags"] & 2 != 0).sum()),
                    "empty": int((got["flags"] & 4 != 0).sum())},
        "host_serial_seconds": host["seconds"], "host_threads": a.threads,
        "host_agrees_on_instances": host["agree"],
        "kernel_registers": kernel_regs(), "build_id": impc.lib.impc_build_id().decode()})
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    for d in (occ_d, pos_d, vel_d):
        d.free()
    sc.close()
    ctx.close()


if __name__ == "__main__":
    main()
