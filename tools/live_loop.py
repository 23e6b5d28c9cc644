#!/usr/bin/env python3
"""The live replan loop's rate: I planning instances flying the reference's benchmark path
(ref_trajectory_dynus_benchmark.txt) at the live horizon N = 30 with up to K dynamic obstacles each,
R chained replans as mpcNavigation::mpcCB runs them -- per replan getXRef on the device
(impc_reference_traj_device), ONE impc_replan_run (makePlanWithPred for every instance) and the
vehicle following its plan for 0.1 s (impc_replan_advance_device).  Every replan's predictions are
resident on the device before the timed loop (the predictor's output, scenarios.live_loop); each
replan is timed from its first call to the end of its device work.  Prints one JSON line.

--mixed-k: every instance sees its own number of obstacles each replan (K_i in 0..K, seeded: a
synthetic stand-in for the detector keeping the obstacles in range and view, fakeDetector.cpp:493 ->
updatePredObstacles predPos.size(), mpcPlanner.cpp:343-373; K_i = 0 replans without predictions).

--statics S: every instance also carries S static obstacles (obclustering_->getStaticObstacles(),
mpcPlanner.cpp:594; impc_replan_config.num_static) -- boxes of 0.6-1.2 m beside its own reference
path, 0.8-1.6 m off it, at random yaw (seeded; the live planner has clustering off, :191-193, so this
is the dormant path at scale).

--gpus N: one process per GPU (started here with torch.distributed.run before anything touches a
GPU, or under the caller's torchrun); the instances are split in contiguous ranges, every rank
replans its own (the selection is per instance: no exchange inside a replan) and, after every replan,
each instance's record (impc_replan_record: what the replan decided and --plan-steps stage states of
the committed plan) reaches every rank: impc_replan_gather packs them on the device and moves them
with one in-place ncclAllGather on the context stream, inside the replan's timed span (on one GPU a
communicator of one rank runs the same path).  A barrier and the max over ranks bound each
replan's time.  With IMPC_RANK_DEVICE putting every rank on one device (a rehearsal; RCCL refuses
that) the records are packed on the device, copied to the host and gathered over gloo.  The rate is
all ranks' instances over that time.  The same loop at small I is checked replan by replan against the restatements in
tests/test_live_loop.py; the rank split in tests/test_distributed.py.

--detector [--range 30.0] [--hist 100]: the detector in the loop instead of baked predictions
(scenarios.live_world; defaults from fake_detector_param.yaml color_distance / history_size).  Every
instance has its own world of --world-obstacles M obstacles; per replan three history pushes
(impc_tracks_push_device: histCB's 0.033 s timer), ONE impc.perception.DeviceTick (range gate ->
intent probabilities -> predicted trajectories -> makePlanWithPred with num_pred = the gate's K_i)
and the vehicle following its plan, all queued on the context stream.  K_i changes only when an
obstacle crosses the sensor range.  The line gains, per replan, the histogram of K_i, the count of
truncated instances (more in range than the K slots), the branch counts and the device times of the
gate, the two predictor kernels and the replan (the context's step timer), and how many vehicles raised
`replan` (impc_replan_check_device on the fresh plan, the tick's map and the gate's boxes) and how
many were `done` (impc_replan_target_device one replan period into it); the two counts are also
printed per replan on stderr.  One GPU.  The same tick
at small I is checked replan by replan in tests/test_tick.py.

--cluster S [--out FILE]: the static-obstacle clustering in the loop (mpcPlanner::staticObstacleClusteringCB
feeding obclustering_->getStaticObstacles(), mpcPlanner.cpp:200-247, :594).  A seeded field of pillars
is laid over the flight (scenarios.live_loop's paths and baked predictions); per replan getXRef, ONE
impc_cluster_run_device with at most S boxes per vehicle, ONE impc_replan_run with the clustering's
count [I] bound (impc_replan_bind_static_count: vehicle i plans around its own s_i boxes, its QPs in
the shapes (k, s_i)) and its centroid / size / yaw passed in place, and the vehicle following its plan.
The same loop then runs again in the only form the replan had before counts could be bound: nothing
bound, every vehicle carrying all S rows (the rows past its count are the boxes it held earlier, or
zero-size boxes at the origin).  One JSON line: replans/s of both, the distribution of s_i per replan,
and the device memory of the replan object in both forms (the sum of its solver batches' device bytes;
the bound object holds S + 1 times the shapes).  One GPU.  --out also appends the line to FILE.
The same chain at small I is checked against the restatement in tests/test_replan_static_counts.py."""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "intent-mpc_amd", "python")]


def relaunch(n, argv):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + argv
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    return subprocess.call(cmd, env=env)


def detector_loop(a):
    import impc
    from impc import execution as E
    from impc import perception as P
    from impc import scenarios
    from impc.replan import DeviceReplan
    I, K, R, N, M, PUSHES = a.instances, a.obstacles, a.replans, a.horizon, a.world_obstacles, 3
    t0 = time.time()
    w = scenarios.live_world(I, M, R, pushes_per_replan=PUSHES, N=N, seed=4100)
    gen_s = time.time() - t0
    p, pd, L = w["params"], w["pd"], w["L"]
    ctx = impc.Context(0)
    rp = DeviceReplan(ctx, p, pd, I, K, L, impc.default_settings(verbose=0))
    paths = impc.ReferencePaths(ctx, list(w["paths"]), pd["ts"], N)
    tracks = P.Tracks(ctx, I, M, a.hist)
    tick = P.DeviceTick(ctx, rp, tracks, P.detect_params(a.range, P.FOV_ALL, (0.0, 0.0, 0.0), K), occ=w["occ"],
                        omap=w["map"])
    Dv = impc.DeviceArray
    c = np.ascontiguousarray
    pos_d, vel_d, xref_d = Dv(ctx, c(w["pos0"])), Dv(ctx, c(w["vel0"])), Dv(ctx, (I, N, 8))
    world_d, wvel_d, wsize_d = Dv(ctx, c(w["world_pos"])), Dv(ctx, c(w["world_vel"])), Dv(ctx, c(w["world_size"]))
    step = world_d.nbytes // (R * PUSHES)
    # what the caller does with each plan (impc.execution): the tracking target one replan period into
    # it and the "replan now" tests at its start, queued behind the replan
    t_target, t_check, yaw_d = Dv(ctx, np.full(I, pd["ts"])), Dv(ctx, np.zeros(I)), Dv(ctx, np.zeros(I))
    tgt = E.TargetBuffers(ctx, I)
    walls, branches, k_hist, truncated, raised, done = [], [], [], [], [], []
    for r in range(R):
        ctx.synchronize()
        t = time.perf_counter()
        for q in range(PUSHES):
            tracks.push_device(world_d.ptr + (r * PUSHES + q) * step, wvel_d.ptr, wsize_d.ptr)
        paths.xref_device(pos_d.ptr, xref_d.ptr)
        ctx.timer_mark()
        tick.gather(pos_d.ptr)
        ctx.timer_mark()
        ctx.timer_mark()
        tick.intent()
        ctx.timer_mark()
        ctx.timer_mark()
        tick.trajectories()
        ctx.timer_mark()
        ctx.timer_mark()
        tick.plan(pos_d.ptr, vel_d.ptr, xref_d.ptr)
        ctx.timer_mark()
        chk = tick.check(t_check.ptr, pos_d.ptr)
        tick.target(E.YAW_SMOOTH, t_target.ptr, pos_d.ptr, yaw_d.ptr, tgt.ptrs())
        rp.advance_device(pd["ts"], pos_d.ptr, vel_d.ptr)
        ctx.synchronize()
        walls.append(time.perf_counter() - t)
        raised.append(int(chk.get()["replan_flag"].sum()))
        done.append(int(tgt.get()["done"].sum()))
        print(f"replan {r}: {raised[-1]} of {I} vehicles raised replan, {done[-1]} done", file=sys.stderr, flush=True)
        st = rp.stats()
        branches.append([int(st["fanout"]), int(st["single_first"]), int(st["single_current"])])
        num, inr = tick.gate.num.get(), tick.gate.in_range.get()
        k_hist.append(np.bincount(num, minlength=K + 1).tolist())
        truncated.append(int((inr > K).sum()))
    ms = ctx.timer_read(max_pairs=4 * R).reshape(R, 4)  # per replan: gate, intent probabilities, trajectories, replan
    last = rp.results(values=False)
    its = np.concatenate([s["info"]["iter"] for s in last["shapes"].values()])
    sts = np.concatenate([s["info"]["status_val"] for s in last["shapes"].values()])
    _, _, _, valid = rp.plans()
    wl = np.array(walls)
    fan = wl[1:]
    med = lambda v: float(np.median(v))  # noqa: E731
    print(json.dumps({
        "workload": f"live loop with the detector: {I} instances on ref_trajectory_dynus_benchmark.txt, N={N}, worlds of "
                    f"{M} obstacles, sensor range {a.range} m, K={K} slots, history {a.hist}, {R} chained replans "
                    f"({PUSHES} history pushes + getXRef + gate + intent probabilities + predicted trajectories + "
                    f"makePlanWithPred + follow plan 0.1 s per replan)",
        "instances": I, "replans": R, "n_gpus": 1, "first_replan_s": float(wl[0]), "fanout_replan_s": fan.tolist(),
        "fanout_replan_s_median": med(fan), "replans_per_s": float(I / med(fan)),
        "device_ms_median": {"gate": med(ms[1:, 0]), "intent_prob": med(ms[1:, 1]), "predict_traj": med(ms[1:, 2]),
                             "replan": med(ms[1:, 3])},
        "device_ms": {"gate": ms[:, 0].tolist(), "intent_prob": ms[:, 1].tolist(), "predict_traj": ms[:, 2].tolist(),
                      "replan": ms[:, 3].tolist()},
        "k_hist": k_hist, "truncated": truncated, "branches": branches, "replan_raised": raised, "done": done,
        "last_replan_rank0": {"qps": int(its.size), "mean_iter": float(its.mean()), "p50_iter": float(np.median(its)),
                              "max_iter": int(its.max()),
                              "status_counts": {str(int(k)): int(v) for k, v in zip(*np.unique(sts, return_counts=True))},
                              "shapes": {str(k): int(s["x"].shape[0]) for k, s in last["shapes"].items()}},
        # QPs that ran all of settings.max_iter iterations, whatever status the final check gave them
        "at_iter_cap_last": int((its >= rp.settings.max_iter).sum()),
        "qp_solves_per_s_rank0": float(its.size / med(fan)), "valid_plans": int(valid.sum()),
        "ref_start_idx_mean": float(paths.last_idx().mean()), "gen_s": gen_s,
        "build_id": impc.lib.impc_build_id().decode()}), flush=True)
    for d in (pos_d, vel_d, xref_d, world_d, wvel_d, wsize_d, t_target, t_check, yaw_d):
        d.free()
    tgt.free()
    tick.close()
    tracks.close()
    paths.close()
    rp.close()
    ctx.close()


def pillar_field(paths, advance_m, seed, res=0.2, clear=0.9):
    """An inflated occupancy grid over the first advance_m metres of every path: pillars of 0.4-1.0 m
    on a jittered 3 m grid over the map's whole height.  Returns (map dict, map_max, occ uint8 [x][y][z])."""
    first = np.concatenate([np.asarray(p, np.float64).reshape(-1, 3)[:2] for p in paths])
    lo = np.floor(first.min(axis=0) - [advance_m + 8.0, advance_m + 8.0, 0.0])
    hi = np.ceil(first.max(axis=0) + [advance_m + 8.0, advance_m + 8.0, 0.0])
    lo[2], hi[2] = np.floor(first[:, 2].min() - 3.0), np.ceil(first[:, 2].max() + 3.0)
    dims = np.round((hi - lo) / res).astype(int)
    occ = np.zeros(dims, np.uint8)
    rng = np.random.default_rng(seed)
    for gx in np.arange(lo[0] + 1.5, hi[0] - 1.5, 3.0):
        for gy in np.arange(lo[1] + 1.5, hi[1] - 1.5, 3.0):
            if rng.random() < 0.45:
                continue
            c = np.array([gx, gy]) + rng.uniform(-0.9, 0.9, 2)
            h = rng.uniform(0.2, 0.5, 2)
            a = np.maximum(np.floor((c - h - lo[:2]) / res).astype(int), 0)
            b = np.minimum(np.ceil((c + h - lo[:2]) / res).astype(int), dims[:2])
            occ[a[0]:b[0], a[1]:b[1], :] = 1
    # a corridor of `clear` m around every path stays free: the vehicles fly between the pillars
    r = int(np.ceil(clear / res))
    free = np.zeros(dims[:2], bool)
    for p in paths:
        pts = np.asarray(p, np.float64).reshape(-1, 3)[:, :2]
        seg = np.concatenate([np.linspace(pts[k], pts[k + 1], 8, endpoint=False) for k in range(len(pts) - 1)])
        ij = np.floor((seg - lo[:2]) / res).astype(int)
        ij = ij[((ij >= 0) & (ij < dims[:2])).all(axis=1)]
        free[ij[:, 0], ij[:, 1]] = True
    grown = np.zeros_like(free)
    for dx in range(-r, r + 1):
        for dy in range(-r, r + 1):
            if dx * dx + dy * dy <= r * r:
                grown |= np.roll(np.roll(free, dx, axis=0), dy, axis=1)
    occ[grown] = 0
    m = dict(origin=lo.tolist(), res=res, dims=dims.tolist())
    return m, (lo + dims * res).tolist(), occ


def cluster_loop(a):
    import impc
    from impc import clustering as CL
    from impc import perception as P
    from impc import scenarios
    from impc.replan import DeviceReplan
    I, K, R, N, S = a.instances, a.obstacles, a.replans, a.horizon, a.cluster
    t0 = time.time()
    sc = scenarios.live_loop(I, K, R, N=N, seed=4100)
    m, map_max, occ = pillar_field(sc["paths"], 0.5 * R, 4103)
    gen_s = time.time() - t0
    p, pd, L = sc["params"], sc["pd"], sc["L"]
    ctx = impc.Context(0)
    Dv = impc.DeviceArray
    c = np.ascontiguousarray
    omap = P.occ_map(m["origin"], m["res"], m["dims"])
    occ_d = Dv(ctx, c(occ).reshape(-1))
    psize_d, prob_d = Dv(ctx, c(sc["pred_size"])), Dv(ctx, c(sc["prob"]))
    pred_d, cur_d = Dv(ctx, c(sc["pred_pos"])), Dv(ctx, c(sc["dyn_cur"]))
    step_pred, step_cur = pred_d.nbytes // R, cur_d.nbytes // R
    paths = impc.ReferencePaths(ctx, list(sc["paths"]), pd["ts"], N)
    cpar = CL.cluster_params(**CL.LIVE_PARAMS, max_points=a.cluster_points, max_boxes=S)

    def run(bound):
        rp = DeviceReplan(ctx, p, pd, I, K, L, impc.default_settings(verbose=0), num_static=S)
        cl = CL.StaticClusters(ctx, cpar, I)
        if bound:
            rp.bind_static_count(cl.arrays["count"].ptr)
        mem = sum(rp._stats_of(rp.shape_by_id(k)[0])["device_bytes"] for k in range(rp.num_shapes))
        pos_d, vel_d, xref_d = Dv(ctx, c(sc["pos0"])), Dv(ctx, c(sc["vel0"])), Dv(ctx, (I, N, 8))
        ar = cl.arrays
        walls, hist, flags, branches = [], [], [], []
        for r in range(R):
            ctx.synchronize()
            t = time.perf_counter()
            paths.xref_device(pos_d.ptr, xref_d.ptr)
            cl.run_device(pos_d.ptr, vel_d.ptr, omap, map_max, occ_d.ptr)
            rp.run_device(pos_d.ptr, vel_d.ptr, xref_d.ptr, cur_d.ptr + r * step_cur, pred_d.ptr + r * step_pred,
                          psize_d.ptr, prob_d.ptr, st_centroid=ar["centroid"].ptr, st_size=ar["size"].ptr,
                          st_yaw=ar["yaw"].ptr)
            rp.advance_device(pd["ts"], pos_d.ptr, vel_d.ptr)
            ctx.synchronize()
            walls.append(time.perf_counter() - t)
            hist.append(np.bincount(ar["count"].get(), minlength=S + 1).tolist())
            flags.append(int((ar["flags"].get() != 0).sum()))
            st = rp.stats()
            branches.append([int(st["fanout"]), int(st["single_first"]), int(st["single_current"])])
        last = rp.results(values=False)
        its = np.concatenate([s["info"]["iter"] for s in last["shapes"].values()])
        valid = int(rp.plans()[3].sum())
        fan = np.array(walls)[1:]
        out = {"replans_per_s": float(I / np.median(fan)), "fanout_replan_s_median": float(np.median(fan)),
               "first_replan_s": float(walls[0]), "fanout_replan_s": fan.tolist(), "replan_device_bytes": int(mem),
               "shapes": rp.num_shapes, "shapes_used_last": len(last["shapes"]), "branches": branches,
               "static_count_hist": hist, "cluster_flagged": flags, "qps_last": int(its.size),
               "mean_iter_last": float(its.mean()), "valid_plans": valid}
        if bound:
            rp.bind_static_count(None)
        for d in (pos_d, vel_d, xref_d):
            d.free()
        cl.close()
        rp.close()
        return out

    bound, fixed = run(True), run(False)
    line = json.dumps({
        "workload": f"live loop with the static-obstacle clustering: {I} instances on ref_trajectory_dynus_benchmark.txt, "
                    f"N={N}, K={K} dynamic obstacles, a pillar field of {int(occ.any(axis=2).sum())} occupied columns "
                    f"({m['res']} m voxels), at most {S} boxes per vehicle, {R} chained replans (getXRef + clustering + "
                    f"makePlanWithPred + follow plan 0.1 s per replan)",
        "instances": I, "replans": R, "n_gpus": 1, "num_static": S,
        "bound_counts": bound, "fixed_num_static": fixed,
        "memory_ratio": bound["replan_device_bytes"] / max(fixed["replan_device_bytes"], 1),
        "gen_s": gen_s, "build_id": impc.lib.impc_build_id().decode()})
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    for d in (occ_d, psize_d, prob_d, pred_d, cur_d):
        d.free()
    paths.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=8192)
    ap.add_argument("--obstacles", type=int, default=4)
    ap.add_argument("--replans", type=int, default=30)
    ap.add_argument("--horizon", type=int, default=30)
    ap.add_argument("--mixed-k", action="store_true", help="per-instance obstacle counts K_i in 0..K per replan")
    ap.add_argument("--statics", type=int, default=0, help="static obstacles per instance (num_static)")
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--plan-steps", type=int, default=None,
                    help="stage states of the plan in every gathered record (0..horizon; default: the horizon)")
    ap.add_argument("--detector", action="store_true", help="gate + predictor + replan per tick (DeviceTick)")
    ap.add_argument("--range", type=float, default=30.0, help="--detector: sensor range (color_distance)")
    ap.add_argument("--hist", type=int, default=100, help="--detector: history entries per track (history_size)")
    ap.add_argument("--world-obstacles", type=int, default=8, help="--detector: obstacles M in every instance's world")
    ap.add_argument("--cluster", type=int, default=0,
                    help="clustering every tick, at most this many boxes per vehicle, counts bound to the replan")
    ap.add_argument("--cluster-points", type=int, default=2048, help="--cluster: max_points of the clustering")
    ap.add_argument("--out", default=None, help="--cluster: also append the JSON line to this file")
    a = ap.parse_args()
    if a.cluster:
        if a.gpus != 1 or a.mixed_k or a.statics or a.detector:
            sys.exit("live_loop.py: --cluster runs on one GPU, without --mixed-k / --statics / --detector")
        return cluster_loop(a)
    if a.detector:
        if a.gpus != 1 or a.mixed_k or a.statics:
            sys.exit("live_loop.py: --detector runs on one GPU, without --mixed-k / --statics")
        return detector_loop(a)
    if "WORLD_SIZE" not in os.environ and a.gpus > 1:
        sys.exit(relaunch(a.gpus, sys.argv[1:]))
    import impc  # noqa: E402  (after a possible relaunch: nothing touched the GPU before it)
    from impc import distributed as D  # noqa: E402
    from impc import scenarios  # noqa: E402
    from impc.replan import DeviceReplan, record_dtype  # noqa: E402
    rank, local_rank, world = D.env()
    if world != a.gpus:
        sys.exit(f"live_loop.py: --gpus {a.gpus} but WORLD_SIZE={world}")
    dist = D.init("gloo", local_rank) if world > 1 else None
    Iall, K, R, N = a.instances, a.obstacles, a.replans, a.horizon
    t0 = time.time()
    sc = scenarios.live_loop(Iall, K, R, N=N, seed=4100)
    bounds = D.equal_instance_bounds(Iall, world)
    lo, hi = int(bounds[rank]), int(bounds[rank + 1])
    I = hi - lo
    num_pred = None
    if a.mixed_k:
        num_pred = np.random.default_rng(4101).integers(0, K + 1, (R, Iall)).astype(np.int32)[:, lo:hi]
    static = None
    if a.statics:
        rs = np.random.default_rng(4102)
        S = a.statics
        cen = np.empty((I, S, 3))
        for i in range(I):
            path = np.asarray(sc["paths"][lo + i], np.float64).reshape(-1, 3)
            at = path[np.linspace(1, min(len(path) - 1, 6), S).astype(int)]
            off = rs.uniform(0.8, 1.6, (S, 2)) * rs.choice([-1.0, 1.0], (S, 2))
            cen[i] = at + np.concatenate([off, np.zeros((S, 1))], axis=1)
        static = (cen, rs.uniform(0.6, 1.2, (I, S, 3)), rs.uniform(-np.pi, np.pi, (I, S)))
    gen_s = time.time() - t0
    p, pd, L = sc["params"], sc["pd"], sc["L"]
    # IMPC_RANK_DEVICE: every rank on that device (a rehearsal of the rank path on a one-GPU box)
    ctx = impc.Context(int(os.environ.get("IMPC_RANK_DEVICE", local_rank)))
    rp = DeviceReplan(ctx, p, pd, I, K, L, impc.default_settings(verbose=0), num_static=a.statics)
    paths = impc.ReferencePaths(ctx, list(sc["paths"][lo:hi]), pd["ts"], N)
    Dv = impc.DeviceArray
    c = np.ascontiguousarray
    pos_d, vel_d, xref_d = Dv(ctx, c(sc["pos0"][lo:hi])), Dv(ctx, c(sc["vel0"][lo:hi])), Dv(ctx, (I, N, 8))
    psize_d, prob_d = Dv(ctx, c(sc["pred_size"][lo:hi])), Dv(ctx, c(sc["prob"][lo:hi]))
    pred_d, cur_d = Dv(ctx, c(sc["pred_pos"][:, lo:hi])), Dv(ctx, c(sc["dyn_cur"][:, lo:hi]))
    np_d = Dv(ctx, c(num_pred)) if num_pred is not None else None
    st_d = [Dv(ctx, c(x)) for x in static] if static is not None else []
    st_ptr = dict(zip(("st_centroid", "st_size", "st_yaw"), (d.ptr for d in st_d)))
    step_pred, step_cur = pred_d.nbytes // R, cur_d.nbytes // R
    # every replan's per-instance records to every rank (impc_replan_gather: pack + ONE in-place
    # ncclAllGather on the context stream).  RCCL refuses several ranks on one device, so the
    # IMPC_RANK_DEVICE rehearsal packs on the device, copies the block to the host and gathers over gloo.
    counts = [int(bounds[k + 1] - bounds[k]) for k in range(world)]
    max_inst = max(counts)
    P = N if a.plan_steps is None else a.plan_steps
    rec_dt = record_dtype(P)
    rehearsal = world > 1 and "IMPC_RANK_DEVICE" in os.environ
    comm = None if rehearsal else D.make_comm(dist, ctx)
    recv_d = Dv(ctx, ((1 if rehearsal else world) * max_inst * rec_dt.itemsize,), np.uint8)
    walls, stats, gathered, allrec = [], [], [], None
    for r in range(R):
        ctx.synchronize()
        if dist is not None:
            dist.barrier()
        t = time.perf_counter()
        paths.xref_device(pos_d.ptr, xref_d.ptr)
        ctx.timer_mark()
        rp.run_device(pos_d.ptr, vel_d.ptr, xref_d.ptr, cur_d.ptr + r * step_cur, pred_d.ptr + r * step_pred,
                      psize_d.ptr, prob_d.ptr, num_pred=None if np_d is None else np_d.ptr + r * 4 * I, **st_ptr)
        ctx.timer_mark()
        rp.advance_device(pd["ts"], pos_d.ptr, vel_d.ptr)
        if rehearsal:
            rp.pack_device(rank, lo, P, max_inst, recv_d.ptr)
            block = recv_d.get()[: I * rec_dt.itemsize].reshape(I, rec_dt.itemsize)  # the one D2H of the rehearsal
            allrec = np.frombuffer(D.gather_costs(dist, block, counts).tobytes(), rec_dt)
        else:
            ctx.timer_mark()
            rp.gather_records(comm, lo, P, max_inst, recv_d.ptr)
            ctx.timer_mark()
        ctx.synchronize()
        if dist is not None:
            dist.barrier()
        walls.append(D.max_over_ranks(dist, time.perf_counter() - t))
        if not rehearsal:  # outside the timed replan: what this rank now holds
            allrec = D.unpad(np.frombuffer(recv_d.get().tobytes(), rec_dt), counts)
        gathered.append(int(np.count_nonzero(allrec["inst"] == np.arange(allrec.shape[0]))))
        st = rp.stats()
        stats.append((st["fanout"], st["single_first"], st["single_current"]))
    ms = ctx.timer_read(max_pairs=2 * R).reshape(R, -1)  # per replan: the replan, then (device path) the gather
    replan_ms, gather_ms = ms[:, 0].tolist(), [] if rehearsal else ms[:, 1].tolist()
    last = rp.results(values=False)
    its = np.concatenate([s["info"]["iter"] for s in last["shapes"].values()])
    sts = np.concatenate([s["info"]["status_val"] for s in last["shapes"].values()])
    st_all = D.gather_costs(dist, np.array([stats[-1]], np.float64), [1] * world)
    w = np.array(walls)
    fan = w[1:]  # replans 1..R-1: every instance past its first plan
    n_qps = int(its.size)
    if rank == 0:
        print(json.dumps({
            "workload": f"live loop: {Iall} instances on ref_trajectory_dynus_benchmark.txt, N={N}, "
                        f"{'K_i in 0..' + str(K) + ' per instance and replan' if a.mixed_k else 'K=' + str(K)} dynamic "
                        f"obstacles{', ' + str(a.statics) + ' static obstacles' if a.statics else ''}, {R} chained "
                        f"replans (getXRef + makePlanWithPred + follow plan 0.1 s per replan)",
            "instances": Iall, "replans": R, "n_gpus": world, "first_replan_s": float(w[0]),
            "fanout_replan_s": fan.tolist(), "fanout_replan_s_median": float(np.median(fan)),
            "replans_per_s": float(Iall / np.median(fan)), "branches_last": st_all.astype(int).sum(axis=0).tolist(),
            "last_replan_rank0": {"qps": n_qps, "mean_iter": float(its.mean()), "p50_iter": float(np.median(its)),
                                  "max_iter": int(its.max()),
                                  "status_counts": {str(int(k)): int(v) for k, v in zip(*np.unique(sts, return_counts=True))},
                                  "shapes": {str(k): int(s["x"].shape[0]) for k, s in last["shapes"].items()}},
            "qp_solves_per_s_rank0": float(n_qps / np.median(fan)),
            "valid_plans": int(allrec["valid"].sum()), "records_gathered": gathered[-1],
            "records": {"plan_steps": P, "bytes_per_record": rec_dt.itemsize,
                        "bytes_per_rank": max_inst * rec_dt.itemsize,
                        "transport": "gloo (one-device rehearsal)" if rehearsal else "rccl",
                        "gathered_per_replan": gathered, "gather_ms": gather_ms,
                        "gather_ms_median": float(np.median(gather_ms[1:])) if len(gather_ms) > 1 else None,
                        "replan_ms_median": float(np.median(replan_ms[1:])) if R > 1 else None},
            "ref_start_idx_mean": float(paths.last_idx().mean()), "gen_s": gen_s,
            "build_id": impc.lib.impc_build_id().decode()}), flush=True)
    if comm is not None:
        comm.close()
    for d in (pos_d, vel_d, xref_d, psize_d, prob_d, pred_d, cur_d, recv_d) + ((np_d,) if np_d is not None else ()) + tuple(st_d):
        d.free()
    paths.close()
    rp.close()
    ctx.close()
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
