"""TEST INFRASTRUCTURE ONLY -- pure-Python restatement of what mpcNavigation does with a committed
plan (the oracle for include/impc_exec.h).  Only tests/ may import it.

Follows the reference statement by statement, in Python floats (IEEE doubles, no contraction):
  trajectory_planner/include/trajectory_planner/mpcPlanner.cpp
    getPos  :1257-1273   empty currentStatesSol_ -> currPos_; idx = floor(t / ts_); dt = t - idx * ts_;
                         idx = max(0, min(idx, size - 1)); nextIdx = min(idx + 1, size - 1);
                         states(c) + (nextStates(c) - states(c)) / ts_ * dt, c = 0..2
    getVel  :1275-1290   empty -> zero; the same over states 3..5
    getAcc  :1292-1307   empty currentControlsSol_ -> zero; the same over the size - 1 controls
    getRef  :1309-1324   empty ref_ -> currPos_; the same over ref_ (rows 0..2 of the committed xref)
  autonomous_flight/include/autonomous_flight/mpcNavigation.cpp
    trajExeCB            :499-567  endTime = getHorizon() * getTs() (:508); leftTime <= 0: pos, zero
                                   velocity / acceleration, odometry yaw (:516-527); else the yaw of
                                   the mode (:530-554) -- the look-ahead is for (t = realTime; t <=
                                   endTime; t += dt) over getRef (:541-549) -- with pos, vel, acc
    mpcHasCollision      :631-647  startTime = min(1.0, realTime); endTime = min(startTime + 2.0,
                                   getHorizon() * dt); for (t = startTime; t <= endTime; t += dt):
                                   isInflatedOccupied(getPos(t))
    hasDynamicCollision  :669-703  endTime = min(startTime + 1.0, ...); p inside the closed box
                                   ob +- size / 2 on all three axes (:689-698)
  map_manager/include/map_manager/occupancyMap.h
    isInflatedOccupied   :257-269  posToIndex (:501-505: floor((pos - mapSizeMin_) / mapRes_)), isInMap
                                   (:490-499; outside -> occupied), indexToAddress
                                   (x * dims[1] * dims[2] + y * dims[2] + z)
The loops run on the running sum `t += dt`, as written.  std::min(a, b) is (b < a) ? b : a.  Eigen's
norm of a 3-vector is sqrt(x x + y y + z z) summed in that order.

A plan is a dict(states [N][8] lists or None/empty, controls [N-1][5], ref [N][3] or empty, cur_pos
[3], N, ts).  The step functions return the index of the first sample that collides, or -1 (the
reference returns whether one does).
"""
import math

YAW_FACING, YAW_HOLD, YAW_SMOOTH = 0, 1, 2


def plan(states, controls, ref, cur_pos, N, ts):
    return dict(states=[] if states is None else [[float(v) for v in s] for s in states],
                controls=[] if controls is None else [[float(v) for v in s] for s in controls],
                ref=[] if ref is None else [[float(v) for v in s] for s in ref],
                cur_pos=[float(v) for v in cur_pos], N=int(N), ts=float(ts))


def _interp(rows, off, ts, t):
    idx = math.floor(t / ts)
    dt = t - idx * ts
    idx = max(0, min(idx, len(rows) - 1))
    next_idx = min(idx + 1, len(rows) - 1)
    s, e = rows[idx], rows[next_idx]
    return [s[off + c] + (e[off + c] - s[off + c]) / ts * dt for c in range(3)]


def get_pos(p, t):
    if len(p["states"]) == 0:
        return list(p["cur_pos"])
    return _interp(p["states"], 0, p["ts"], t)


def get_vel(p, t):
    if len(p["states"]) == 0:
        return [0.0, 0.0, 0.0]
    return _interp(p["states"], 3, p["ts"], t)


def get_acc(p, t):
    if len(p["controls"]) == 0:
        return [0.0, 0.0, 0.0]
    return _interp(p["controls"], 0, p["ts"], t)


def get_ref(p, t):
    if len(p["ref"]) == 0:
        return list(p["cur_pos"])
    return _interp(p["ref"], 0, p["ts"], t)


def sample_times(start, end, dt):
    """for (double t = start; t <= end; t += dt)"""
    out = []
    t = start
    while t <= end:
        out.append(t)
        t += dt
    return out


def target(p, real_time, yaw_mode, odom_yaw, facing_yaw=0.0, forward_dist=1.0):
    """trajExeCB with mpcTrajectoryReady_: dict(pos, vel, acc, ref, yaw, done, yaw_step, dx, dy);
    yaw_step is the look-ahead sample whose point gave the yaw (-1: none, or another mode), dx / dy
    atan2's arguments."""
    end_time = p["N"] * p["ts"]
    pos = get_pos(p, real_time)
    vel = get_vel(p, real_time)
    acc = get_acc(p, real_time)
    ref_pos = get_ref(p, real_time)
    left_time = end_time - real_time
    out = dict(pos=pos, ref=ref_pos, yaw_step=-1, dx=0.0, dy=0.0)
    if left_time <= 0.0:
        out.update(vel=[0.0, 0.0, 0.0], acc=[0.0, 0.0, 0.0], yaw=odom_yaw, done=1)
        return out
    if yaw_mode == YAW_FACING:
        yaw = facing_yaw
    elif yaw_mode == YAW_HOLD:
        yaw = odom_yaw
    else:
        dt = p["ts"]
        no_yaw_change = True
        yaw = None
        t, k = real_time, 0
        while t <= end_time:
            q = get_ref(p, t)
            d = [q[0] - ref_pos[0], q[1] - ref_pos[1], q[2] - ref_pos[2]]
            if math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) >= forward_dist:
                yaw = math.atan2(q[1] - ref_pos[1], q[0] - ref_pos[0])
                out.update(yaw_step=k, dx=d[0], dy=d[1])
                no_yaw_change = False
                break
            t += dt
            k += 1
        if no_yaw_change:
            yaw = odom_yaw
    out.update(vel=vel, acc=acc, yaw=yaw, done=0)
    return out


def is_inflated_occupied(m, occ, pos):
    """m: dict(origin [3], res, dims [3]); occ: flat sequence, nonzero = occupied."""
    idx = [math.floor((pos[c] - m["origin"][c]) / m["res"]) for c in range(3)]
    d = m["dims"]
    if not all(0 <= idx[c] < d[c] for c in range(3)):
        return True
    return bool(occ[idx[0] * d[1] * d[2] + idx[1] * d[2] + idx[2]])


def _window(p, real_time, span):
    start_time = real_time if real_time < 1.0 else 1.0
    a, b = start_time + span, p["N"] * p["ts"]
    return start_time, (b if b < a else a)


def map_step(p, real_time, m, occ):
    """mpcHasCollision: the first sample inside the inflated map's occupied space, or -1."""
    dt = p["ts"]
    start_time, end_time = _window(p, real_time, 2.0)
    t, k = start_time, 0
    while t <= end_time:
        if is_inflated_occupied(m, occ, get_pos(p, t)):
            return k
        t += dt
        k += 1
    return -1


def in_box(q, ob, size):
    lower = [ob[c] - size[c] / 2 for c in range(3)]
    upper = [ob[c] + size[c] / 2 for c in range(3)]
    return (q[0] >= lower[0] and q[0] <= upper[0] and q[1] >= lower[1] and q[1] <= upper[1] and
            q[2] >= lower[2] and q[2] <= upper[2])


def dyn_step(p, real_time, obstacles_pos, obstacles_size):
    """hasDynamicCollision: the first sample inside any box, or -1."""
    dt = p["ts"]
    start_time, end_time = _window(p, real_time, 1.0)
    t, k = start_time, 0
    while t <= end_time:
        q = get_pos(p, t)
        for ob, size in zip(obstacles_pos, obstacles_size):
            if in_box(q, ob, size):
                return k
        t += dt
        k += 1
    return -1


# ---------------------------------------------------------------- the library's outputs, restated
def plans_from_arrays(plan_x, plan_ref, count, ref_count, cur_pos, N, ts):
    """One plan dict per instance from the replan object's arrays: plan_x [I][13 N - 5], plan_ref
    [I][N][3], count / ref_count [I] (0 = empty), cur_pos [I][3]."""
    out = []
    for i in range(len(plan_x)):
        x = [float(v) for v in plan_x[i]]
        st = [x[8 * k:8 * k + 8] for k in range(N)] if count[i] > 0 else []
        ct = [x[8 * N + 5 * k:8 * N + 5 * k + 5] for k in range(N - 1)] if count[i] > 0 else []
        rf = [[float(v) for v in r] for r in plan_ref[i]] if ref_count[i] > 0 else []
        out.append(dict(states=st, controls=ct, ref=rf, cur_pos=[float(v) for v in cur_pos[i]], N=N, ts=float(ts)))
    return out


def target_batch(plans, t, yaw_mode, odom_yaw, facing_yaw, forward_dist=1.0):
    """impc_replan_target_device for ready instances: dict of numpy arrays pos, vel, acc, ref [I][3],
    yaw [I], done [I] int8, yaw_step [I] int32, dxy [I][2]."""
    import numpy as np
    res = [target(p, float(t[i]), yaw_mode, float(odom_yaw[i]), float(facing_yaw[i]), forward_dist)
           for i, p in enumerate(plans)]
    out = {k: np.array([r[k] for r in res], np.float64).reshape(len(res), -1) for k in ("pos", "vel", "acc", "ref")}
    out["yaw"] = np.array([r["yaw"] for r in res], np.float64)
    out["done"] = np.array([r["done"] for r in res], np.int8)
    out["yaw_step"] = np.array([r["yaw_step"] for r in res], np.int32)
    out["dxy"] = np.array([[r["dx"], r["dy"]] for r in res], np.float64).reshape(len(res), 2)
    return out


def check_batch(plans, t, m, occ, num_obs, ob_pos, ob_size):
    """impc_replan_check_device for ready instances: (map_step, dyn_step, replan); m / occ None skips
    the map test, num_obs None the dynamic one."""
    import numpy as np
    I = len(plans)
    ms = np.full(I, -1, np.int32)
    ds = np.full(I, -1, np.int32)
    for i, p in enumerate(plans):
        if occ is not None:
            ms[i] = map_step(p, float(t[i]), m, occ)
        if num_obs is not None:
            n = int(num_obs[i])
            ds[i] = dyn_step(p, float(t[i]), [list(map(float, v)) for v in ob_pos[i][:n]],
                             [list(map(float, v)) for v in ob_size[i][:n]])
    return ms, ds, ((ms >= 0) | (ds >= 0)).astype(np.int8)
