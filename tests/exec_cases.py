"""TEST INFRASTRUCTURE ONLY -- seeded cases for include/impc_exec.h, shared by tests/test_exec_host.py
(the host-compiled functions) and tests/test_exec_gpu.py (the kernels), and classified with
tests/exec_ref.py alone.

make(I, N, ts, K, seed): I instances with a plan through an 8 x 6 x 5-voxel map (0.5 m voxels, about
an eighth of them occupied), K box slots and a reference each, built so that for the map test, the
dynamic test and the yaw look-ahead every outcome occurs: no hit, a hit at the loop's first sample,
a hit at a later sample.  Instance i is aimed at outcome (i + shift) % 3 of each where its window
admits it (a window of one sample cannot hit later; one of none cannot hit at all) -- plans are
redrawn until the restatement reports the wanted map outcome, boxes are placed on the plan's own
sample for the dynamic one, and the reference's length is scaled for the look-ahead.  classes()
reports what the restatement finally says, and the tests assert on that.

The times: t = 0, 0.05, 0.37, 1.0, 1.9, N ts, N ts + 0.1 for the first seven instances, then three in
four inside the plan and the rest past its end (leftTime <= 0).  Instance 7 has no plan at all
(getPos -> currPos_), instance 8 a plan and an empty ref_ (getRef -> currPos_), instances 9 and 40
are not ready.  Instance 10's first box has its lower x face exactly on the plan's first sample (the
closed comparison).  With N >= 100 (loops of more than 64 samples) instance 11's plan leaves the grid,
and instance 12's reference moves away, only after sample 64.
"""
import math

import numpy as np

import exec_ref as er

MAP = dict(origin=[-2.0, -1.5, -1.0], res=0.5, dims=[8, 6, 5])
NONE, FIRST, LATER = 0, 1, 2
FAR = 100.0  # a box nowhere near the map


def occupancy(seed=11):
    rng = np.random.default_rng(seed)
    return (rng.uniform(size=MAP["dims"]) < 0.125).astype(np.uint8)


def _cls(step):
    return NONE if step < 0 else FIRST if step == 0 else LATER


def _window_samples(p, t, span):
    start, end = er._window(p, t, span)
    return er.sample_times(start, end, p["ts"])


def _draw_plan(rng, N):
    lo = np.array(MAP["origin"])
    ext = np.array(MAP["dims"]) * MAP["res"]
    p0 = lo + rng.uniform(0.05, 0.95, 3) * ext
    d = rng.normal(size=3)
    d *= rng.choice([rng.uniform(0.2, 1.0), rng.uniform(1.0, 3.0), rng.uniform(3.0, 7.0)]) / np.linalg.norm(d)
    s = np.linspace(0.0, 1.0, N)[:, None]
    states = np.zeros((N, 8))
    states[:, :3] = p0 + s * d + rng.normal(scale=0.02, size=(N, 3))
    states[:, 3:6] = rng.normal(scale=1.5, size=(N, 3))
    states[:, 6:] = rng.uniform(0.0, 0.1, (N, 2))
    controls = np.concatenate([rng.normal(scale=3.0, size=(N - 1, 3)), rng.uniform(0.0, 0.1, (N - 1, 2))], axis=1)
    return states, controls


def make(I, N, ts, K=3, seed=0):
    rng = np.random.default_rng(seed)
    T = N * ts
    occ = occupancy()
    flat = occ.reshape(-1)
    t = np.empty(I)
    fixed = [0.0, 0.05, 0.37, 1.0, 1.9, T, T + 0.1]
    for i in range(I):
        t[i] = fixed[i] if i < len(fixed) else (rng.uniform(0.0, 0.9 * T) if i % 4 else rng.uniform(T, T + 0.5))
    long_loops = N >= 100 and T >= 2.0 and I > 12  # loops of more than 64 samples: instances 11 and 12
    if long_loops:
        t[11] = t[12] = 0.1
    count = np.full(I, N, np.int32)
    ref_count = np.full(I, N, np.int32)
    ready = np.ones(I, np.int8)
    if I > 8:
        count[7] = ref_count[7] = 0
        ref_count[8] = 0
    for i in (9, 40):
        if i < I:
            ready[i] = 0
    cur_pos = np.array(MAP["origin"]) + rng.uniform(0.1, 0.9, (I, 3)) * np.array(MAP["dims"]) * MAP["res"]
    plan_x = np.zeros((I, 13 * N - 5))
    plan_ref = np.zeros((I, N, 3))
    num_obs = np.zeros(I, np.int32)
    ob_pos = np.full((I, K, 3), FAR)
    ob_size = np.full((I, K, 3), 0.5)
    face = None
    for i in range(I):
        # ---- the plan, redrawn until the map test gives the wanted outcome
        probe = er.plan(np.zeros((N, 8)), None, None, cur_pos[i], N, ts)
        n_map = len(_window_samples(probe, float(t[i]), 2.0))
        want = min((i + 0) % 3, n_map) if count[i] else NONE
        for _ in range(300):
            states, controls = _draw_plan(rng, N)
            p = er.plan(states if count[i] else None, controls if count[i] else None, None, cur_pos[i], N, ts)
            if not count[i] or _cls(er.map_step(p, float(t[i]), MAP, flat)) == want:
                break
        if long_loops and i == 11:  # free until state 75, then out of the grid: a hit past sample 64
            free = np.argwhere(occ == 0)[len(np.argwhere(occ == 0)) // 2]
            states[:, :3] = np.array(MAP["origin"]) + (free + 0.5) * MAP["res"] + rng.normal(scale=0.02, size=(N, 3))
            states[75:, :3] = FAR
            p = er.plan(states, controls, None, cur_pos[i], N, ts)
        plan_x[i, :8 * N] = states.reshape(-1)
        plan_x[i, 8 * N:] = controls.reshape(-1)
        # ---- the boxes, on the plan's own samples
        times = _window_samples(p, float(t[i]), 1.0)
        want = min((i + 1) % 3, len(times))
        num_obs[i] = rng.integers(0, K + 1) if want == NONE else rng.integers(1, K + 1)
        if want != NONE:
            k = 0 if want == FIRST else int(rng.integers(1, len(times)))
            q = np.array(er.get_pos(p, times[k]))
            slot = int(rng.integers(0, num_obs[i]))
            size = rng.uniform(0.2, 0.6, 3) if want == FIRST else rng.uniform(1e-4, 4e-4, 3)
            ob_pos[i, slot] = q + rng.uniform(-0.4, 0.4, 3) * size
            ob_size[i, slot] = size
        if i == 10 and count[i] and times:  # the lower x face exactly on the first sample
            q = er.get_pos(p, times[0])
            for sx in [2.0 ** -k for k in range(12)]:  # q + sx / 2 is exact once sx / 2 is below |q|'s binade
                c = q[0] + sx / 2
                if c - sx / 2 == q[0]:
                    num_obs[i] = max(num_obs[i], 1)
                    ob_pos[i, 0] = [c, q[1], q[2]]
                    ob_size[i, 0] = [sx, 0.5, 0.5]
                    face = (i, q[0], c, sx)
                    break
        # ---- the reference: a line whose length decides how far ahead the look-ahead must go
        last = (N - 1) * ts
        frac = (last - t[i]) / last
        want = (i + 2) % 3
        if want == FIRST:  # only forward_dist <= 0 stops at the first sample: either other outcome
            want = NONE if i % 2 else LATER
        e = rng.normal(size=3)
        e[2] *= 0.2
        e /= np.linalg.norm(e)
        length = rng.uniform(0.0, 0.6) if (want == NONE or frac <= 0.05) else rng.uniform(1.5, 4.0) / frac
        s = np.linspace(0.0, 1.0, N)[:, None]
        plan_ref[i] = rng.uniform(-5, 5, 3) + s * (length * e) + rng.normal(scale=1e-3, size=(N, 3))
        if long_loops and i == 12:  # at rest until row 75, then 5 m away: the look-ahead stops past sample 64
            plan_ref[i] = plan_ref[i, 0] + rng.normal(scale=1e-3, size=(N, 3))
            plan_ref[i, 75:, 0] += 5.0
    return dict(I=I, N=N, ts=ts, K=K, map=MAP, occ=occ, t=t, ready=ready, count=count, ref_count=ref_count,
                cur_pos=cur_pos, plan_x=plan_x, plan_ref=plan_ref, num_obs=num_obs, ob_pos=ob_pos, ob_size=ob_size,
                odom_yaw=rng.uniform(-math.pi, math.pi, I), facing_yaw=rng.uniform(-math.pi, math.pi, I), face=face)


def plans(c, ref_count=None):
    return er.plans_from_arrays(c["plan_x"], c["plan_ref"], c["count"], c["ref_count"] if ref_count is None else ref_count,
                                c["cur_pos"], c["N"], c["ts"])


def reference(c, ref_count=None):
    """What the restatement gives for every instance as if ready: the targets of the three yaw modes
    (and IMPC_YAW_SMOOTH at forward_dist = 0) and the two collision tests."""
    pl = plans(c, ref_count)
    out = {m: er.target_batch(pl, c["t"], m, c["odom_yaw"], c["facing_yaw"]) for m in
           (er.YAW_FACING, er.YAW_HOLD, er.YAW_SMOOTH)}
    out["smooth0"] = er.target_batch(pl, c["t"], er.YAW_SMOOTH, c["odom_yaw"], c["facing_yaw"], forward_dist=0.0)
    out["map_step"], out["dyn_step"], out["replan"] = er.check_batch(pl, c["t"], c["map"], c["occ"].reshape(-1),
                                                                     c["num_obs"], c["ob_pos"], c["ob_size"])
    return out


def classes(ref):
    """Instances per outcome (none, first sample, later sample) of the map test, the dynamic test and
    the look-ahead at forward_dist = 1 and at 0, and the number with leftTime <= 0."""
    def count(steps):
        steps = np.asarray(steps)
        return [int((steps < 0).sum()), int((steps == 0).sum()), int((steps > 0).sum())]
    return dict(map=count(ref["map_step"]), dyn=count(ref["dyn_step"]), look=count(ref[er.YAW_SMOOTH]["yaw_step"]),
                look0=count(ref["smooth0"]["yaw_step"]), done=int(ref[er.YAW_SMOOTH]["done"].sum()))


def assert_classes(cl, I):
    """Every outcome of every loop holds at least a tenth of the instances.  The look-ahead's first
    sample is getRef(realTime) itself, at distance 0 from refPos, so with forward_dist = 1 (the
    reference's value) it can never stop there: that outcome is exercised at forward_dist = 0, where
    every instance with time left stops at sample 0, and counted there."""
    tenth = I / 10.0
    assert min(cl["map"]) >= tenth, cl
    assert min(cl["dyn"]) >= tenth, cl
    assert cl["look"][0] >= tenth and cl["look"][2] >= tenth and cl["look"][1] == 0, cl
    assert cl["look0"][1] >= tenth, cl
    assert cl["done"] >= 1, cl
