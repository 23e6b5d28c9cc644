"""The plan getters, trajExeCB's target and the two collision tests of csrc/plan_exec.hpp, compiled
for the host (tests/native/exec_harness.cpp: the same __host__ __device__ functions the kernels
k_target / k_check call) against the Python restatement tests/exec_ref.py, bit for bit -- positions,
velocities, accelerations, reference points, the yaw (both sides use the host's atan2) and every step
index.  Cases: tests/exec_cases.py at N in {5, 20} x ts in {0.1, 0.02}; their outcome classes are
asserted with the restatement alone, so a set of cases that exercises nothing fails.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

import exec_cases as ec
import exec_ref as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXEC_HARNESS = os.path.join(ROOT, "tests", "native", "build", "libexec_harness.so")
I, K = 67, 3


class OccMap(C.Structure):  # impc_occ_map (include/impc_predict.h)
    _fields_ = [("origin", C.c_double * 3), ("resolution", C.c_double), ("dims", C.c_int32 * 3), ("reserved", C.c_int32)]


def _map(m):
    om = OccMap(resolution=m["res"])
    om.origin[:] = m["origin"]
    om.dims[:] = m["dims"]
    return om


@pytest.fixture(scope="module")
def lib():
    h = C.CDLL(EXEC_HARNESS)
    h.exec_sample_count.restype = C.c_int32
    h.exec_sample_count.argtypes = [C.c_double, C.c_double, C.c_double, C.POINTER(C.c_double)]
    return h


_CASES = {}


def _case(N, ts):
    """The seeded cases of one (N, ts) and the restatement's results, computed once."""
    if (N, ts) not in _CASES:
        c = ec.make(I, N, ts, K, seed=1000 + N)
        _CASES[N, ts] = (c, ec.reference(c))
    return _CASES[N, ts]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def harness_target(lib, c, mode, forward_dist=1.0):
    n, N = c["I"], c["N"]
    out = dict(pos=np.empty((n, 3)), vel=np.empty((n, 3)), acc=np.empty((n, 3)), ref=np.empty((n, 3)), yaw=np.empty(n),
               done=np.empty(n, np.int8), yaw_step=np.empty(n, np.int32), dxy=np.empty((n, 2)))
    lib.exec_target(C.c_int64(n), C.c_int32(N), C.c_double(c["ts"]), _p(c["plan_x"]), _p(c["plan_ref"]), _p(c["count"]),
                    _p(c["ref_count"]), _p(c["cur_pos"]), _p(c["t"]), C.c_int32(mode), C.c_double(forward_dist),
                    _p(c["odom_yaw"]), _p(c["facing_yaw"]), *[_p(out[k]) for k in
                                                              ("pos", "vel", "acc", "ref", "yaw", "done", "yaw_step", "dxy")])
    return out


def harness_check(lib, c, with_map=True, with_boxes=True):
    n = c["I"]
    ms, ds = np.empty(n, np.int32), np.empty(n, np.int32)
    om = _map(c["map"])
    occ = np.ascontiguousarray(c["occ"].reshape(-1))
    lib.exec_check(C.c_int64(n), C.c_int32(c["N"]), C.c_double(c["ts"]), _p(c["plan_x"]), _p(c["count"]), _p(c["cur_pos"]),
                   _p(c["t"]), C.byref(om), _p(occ) if with_map else None, C.c_int32(c["K"]),
                   _p(c["num_obs"]) if with_boxes else None, _p(c["ob_pos"]), _p(c["ob_size"]), _p(ms), _p(ds))
    return ms, ds


CONFIGS = [(5, 0.1), (5, 0.02), (20, 0.1), (20, 0.02)]


@pytest.mark.parametrize("N,ts", CONFIGS)
def test_cases_exercise_every_outcome(N, ts):
    c, ref = _case(N, ts)
    cl = ec.classes(ref)
    print(f"N={N} ts={ts}: {cl}")
    ec.assert_classes(cl, I)
    assert c["count"][7] == 0 and c["ref_count"][8] == 0 and c["count"][8] == N
    # the box whose lower x face is exactly the plan's first sample: hit through the closed comparison
    i, q0, centre, sx = c["face"]
    assert centre - sx / 2 == q0 and c["ob_pos"][i, 0, 0] == centre and ref["dyn_step"][i] == 0
    open_box = c["ob_pos"][i].copy()
    open_box[0, 0] = np.nextafter(centre, np.inf)  # one ulp further and the sample is outside
    p = ec.plans(c)[i]
    assert er.dyn_step(p, float(c["t"][i]), open_box[:1].tolist(), c["ob_size"][i, :1].tolist()) != 0


@pytest.mark.parametrize("N,ts", CONFIGS)
def test_getters_match_restatement(lib, N, ts):
    c, _ = _case(N, ts)
    n = c["I"]
    got = [np.empty((n, 3)) for _ in range(4)]
    rng = np.random.default_rng(5)
    for t in (c["t"], rng.uniform(0.0, 1.5 * N * ts, n), np.arange(n) * ts, np.arange(n) * ts * 0.5):
        t = np.ascontiguousarray(t, np.float64)
        lib.exec_getters(C.c_int64(n), C.c_int32(N), C.c_double(ts), _p(c["plan_x"]), _p(c["plan_ref"]), _p(c["count"]),
                         _p(c["ref_count"]), _p(c["cur_pos"]), _p(t), *[_p(g) for g in got])
        pl = ec.plans(c)
        for g, f in zip(got, (er.get_pos, er.get_vel, er.get_acc, er.get_ref)):
            np.testing.assert_array_equal(g, np.array([f(pl[i], float(t[i])) for i in range(n)]), err_msg=f.__name__)
    # no plan: currPos_ and zeros; an empty ref_: currPos_
    np.testing.assert_array_equal(got[0][7], c["cur_pos"][7])
    assert not got[1][7].any() and not got[2][7].any()
    np.testing.assert_array_equal(got[3][8], c["cur_pos"][8])


@pytest.mark.parametrize("N,ts", CONFIGS)
def test_target_matches_restatement(lib, N, ts):
    c, ref = _case(N, ts)
    for mode, fd in ((er.YAW_FACING, 1.0), (er.YAW_HOLD, 1.0), (er.YAW_SMOOTH, 1.0), ("smooth0", 0.0)):
        got = harness_target(lib, c, er.YAW_SMOOTH if mode == "smooth0" else mode, fd)
        for k, v in ref[mode].items():
            np.testing.assert_array_equal(got[k], v, err_msg=f"mode {mode}: {k}")
    done = ref[er.YAW_HOLD]["done"] == 1
    np.testing.assert_array_equal(done, N * ts - c["t"] <= 0.0)
    assert not ref[er.YAW_SMOOTH]["vel"][done].any() and not ref[er.YAW_SMOOTH]["acc"][done].any()
    np.testing.assert_array_equal(ref[er.YAW_FACING]["yaw"], np.where(done, c["odom_yaw"], c["facing_yaw"]))
    np.testing.assert_array_equal(ref[er.YAW_HOLD]["yaw"], c["odom_yaw"])
    s = ref[er.YAW_SMOOTH]
    hit = s["yaw_step"] >= 0
    np.testing.assert_array_equal(s["yaw"][~hit], c["odom_yaw"][~hit])
    # (math.atan2, the C library's: numpy's vectorised arctan2 differs from it in the last bit)
    np.testing.assert_array_equal(s["yaw"][hit], [math.atan2(dy, dx) for dx, dy in s["dxy"][hit]])


@pytest.mark.parametrize("N,ts", CONFIGS)
def test_collision_steps_match_restatement(lib, N, ts):
    c, ref = _case(N, ts)
    ms, ds = harness_check(lib, c)
    np.testing.assert_array_equal(ms, ref["map_step"])
    np.testing.assert_array_equal(ds, ref["dyn_step"])
    ms, ds = harness_check(lib, c, with_map=False)
    assert (ms == -1).all()
    np.testing.assert_array_equal(ds, ref["dyn_step"])
    ms, ds = harness_check(lib, c, with_boxes=False)
    np.testing.assert_array_equal(ms, ref["map_step"])
    assert (ds == -1).all()
    # plans that leave the grid are stopped there: outside counts as occupied
    pl = ec.plans(c)
    lo, hi = np.array(c["map"]["origin"]), np.array(c["map"]["origin"]) + np.array(c["map"]["dims"]) * c["map"]["res"]
    left = 0
    for i in np.flatnonzero(ref["map_step"] >= 0):
        start, end = er._window(pl[i], float(c["t"][i]), 2.0)
        q = np.array(er.get_pos(pl[i], er.sample_times(start, end, ts)[ref["map_step"][i]]))
        left += bool(((q < lo) | (q >= hi)).any())
    assert left >= 3


def test_map_lookup_matches_restatement(lib):
    m, occ = ec.MAP, ec.occupancy()
    om, flat = _map(m), np.ascontiguousarray(occ.reshape(-1))
    rng = np.random.default_rng(3)
    lo = np.array(m["origin"])
    ext = np.array(m["dims"]) * m["res"]
    pts = lo + rng.uniform(-0.2, 1.2, (4000, 3)) * ext
    edge = lo + rng.integers(0, 9, (400, 3)) * m["res"]  # on voxel faces, the grid's outer faces included
    inside = 0
    for q in np.concatenate([pts, edge]):
        q = np.ascontiguousarray(q)
        want = er.is_inflated_occupied(m, flat, q.tolist())
        assert lib.exec_inflated_occupied(C.byref(om), _p(flat), _p(q)) == int(want)
        inside += not want
    assert inside >= 1000


def test_sample_counts_follow_the_running_sum(lib):
    """The loops run on t += dt: from 1.0 with ts = 0.1 the sum reaches 3.0 after 20 samples where
    1.0 + k * 0.1 would give 21, and from 0.0 the 21st value is 2.0000000000000004 > 2.0."""
    last = C.c_double()
    assert len(er.sample_times(1.0, 3.0, 0.1)) == 20 and lib.exec_sample_count(1.0, 3.0, 0.1, C.byref(last)) == 20
    assert last.value == er.sample_times(1.0, 3.0, 0.1)[-1] < 3.0
    assert sum(1.0 + k * 0.1 <= 3.0 for k in range(30)) == 21
    assert len(er.sample_times(0.0, 2.0, 0.1)) == 20 and lib.exec_sample_count(0.0, 2.0, 0.1, C.byref(last)) == 20
    t = 0.0
    for _ in range(20):
        t += 0.1
    assert t == 2.0000000000000004
    for start, end, dt in ((0.37, 2.0, 0.1), (0.0, 2.0, 0.02), (1.0, 2.2, 0.02), (0.05, 0.1, 0.02), (1.9, 0.5, 0.1)):
        want = er.sample_times(start, end, dt)
        assert lib.exec_sample_count(start, end, dt, C.byref(last)) == len(want)
        if want:
            assert last.value == want[-1]
    # the same counts through the collision windows of a plan at ts = 0.1, N = 30 (endTime 3.0)
    p = er.plan(np.zeros((30, 8)), np.zeros((29, 5)), None, [0.0, 0.0, 0.0], 30, 0.1)
    assert len(er.sample_times(*er._window(p, 1.0, 2.0), 0.1)) == 20
    assert len(er.sample_times(*er._window(p, 0.0, 2.0), 0.1)) == 20
    assert math.isclose(er._window(p, 5.0, 2.0)[0], 1.0)
