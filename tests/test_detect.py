"""The detector stage (include/impc_detect.h): the track store of fakeDetector's histCB and the
batched sensor-range gate of getDynamicObstaclesHist / getObstaclesInSensorRange
(fakeDetector.cpp:337-347, :482-556).

CPU: known answers of the restatement (tests/detect_ref.py) that follow from the cited statements
(the reference holds no tests for these functions, so parity of the restatement is unpinned), and
the kernel's predicate (csrc/detect_gate.hpp) compiled for the host against the restatement.
GPU: the gate against the restatement byte for byte -- its outputs are copies and integers, so
every array is compared with np.array_equal, the empty slots included.  The only floating-point
decisions are the two comparisons of isObstacleInSensorRange; the device's sqrt is correctly rounded
but its cos / sin / atan2 may differ from glibc's by an ulp, so the seeded inputs are asserted to
keep 1e-9 from both thresholds (distances of tens of metres and angles of radians carry ulps of
1e-14 and less)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import detect_ref as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DETECT_HARNESS = os.path.join(ROOT, "tests", "native", "build", "libdetect_harness.so")
MARGIN = 1e-9
ROBOT_SIZE = (0.3, 0.2, 0.1)


# ---------------------------------------------------------------- known answers (CPU)
def _det(boxes, rng_m=30.0, H=100, robot=(0.0, 0.0, 0.0), yaw=0.0):
    d = dr.FakeDetector(H, rng_m)
    d.obstacle_msg = [dr.box(p, (0.5, -0.25, 9.0), (1.0, 2.0, 3.0)) for p in boxes]
    d.robot_pos, d.robot_yaw = list(robot), yaw
    d.hist_cb()
    return d


def test_range_is_inclusive_and_z_does_not_count():
    d = _det([(30.0, 0.0, 0.0), (0.0, 30.0, 500.0), (math.nextafter(30.0, 31.0), 0.0, 0.0), (18.0, 24.0, -7.0)])
    got = [d.is_obstacle_in_sensor_range(b, 2 * math.pi) for b in d.obstacle_msg]
    assert got == [True, True, False, True]   # at exactly `range`: kept (<=); 18-24-30 triangle; z ignored


def test_field_of_view():
    deg = math.pi / 180
    at = lambda a, r=10.0: (r * math.cos(a), r * math.sin(a), 1.0)  # noqa: E731
    d = _det([at(0.0), at(44 * deg), at(46 * deg), at(-46 * deg), at(math.pi), at(0.0, 31.0)])
    got = [d.is_obstacle_in_sensor_range(b, math.pi / 2) for b in d.obstacle_msg]
    assert got == [True, True, False, False, False, False]
    # fov = 2 pi: everything within range, whatever the yaw
    for yaw in (0.0, 1.0, -2.5, math.pi):
        d.robot_yaw = yaw
        assert [d.is_obstacle_in_sensor_range(b, 2 * math.pi) for b in d.obstacle_msg] == [True] * 5 + [False]
    # the view turns with the yaw
    d.robot_yaw = math.pi
    assert [d.is_obstacle_in_sensor_range(b, math.pi / 2) for b in d.obstacle_msg] == [False] * 4 + [True, False]


def test_getters_keep_index_order_and_add_robot_size():
    d = _det([(50.0, 0.0, 0.0), (5.0, 0.0, 0.0), (0.0, 40.0, 0.0), (0.0, -7.0, 0.0), (1.0, 1.0, 1.0)])
    cur = d.get_obstacles_in_sensor_range(2 * math.pi, ROBOT_SIZE)
    assert [(b["x"], b["y"]) for b in cur] == [(5.0, 0.0), (0.0, -7.0), (1.0, 1.0)]
    assert all((b["x_width"], b["y_width"], b["z_width"]) == (1.0 + 0.3, 2.0 + 0.2, 3.0 + 0.1) for b in cur)
    ph, vh, sh = d.get_dynamic_obstacles_hist(ROBOT_SIZE)
    assert [h[0] for h in ph] == [[5.0, 0.0, 0.0], [0.0, -7.0, 0.0], [1.0, 1.0, 1.0]]
    assert vh[0] == [[0.5, -0.25, 0.0]]            # (Vx, Vy, 0)
    assert sh[0] == [[1.3, 2.2, 3.1]]
    assert d.obstacle_msg[1]["x_width"] == 1.0     # the getters copy: the stored boxes keep their size


def test_history_holds_the_last_H_newest_first():
    H = 4
    d = dr.FakeDetector(H, 30.0)
    for n in range(H + 2):
        d.obstacle_msg = [dr.box((float(n), 0.0, 0.0), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)),
                          dr.box((0.0, float(-n), 0.0), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))]
        d.hist_cb()
    assert [h["x"] for h in d.obstacle_hist[0]] == [5.0, 4.0, 3.0, 2.0]
    assert [h["y"] for h in d.obstacle_hist[1]] == [-5.0, -4.0, -3.0, -2.0]
    # the gate reads the NEWEST entry only: obstacle 0 left the range, its older entries do not count
    d.color_distance = 4.5
    ph, _, _ = d.get_dynamic_obstacles_hist((0.0, 0.0, 0.0))
    assert len(ph) == 0
    d.color_distance = 5.0
    ph, _, _ = d.get_dynamic_obstacles_hist((0.0, 0.0, 0.0))
    assert [len(h) for h in ph] == [H, H]


def test_gather_restates_the_empty_slot_convention():
    pushes = [(np.array([[1.0, 0, 0], [99.0, 0, 0], [2.0, 0, 0]]), np.ones((3, 3)), np.ones((3, 3)))]
    out = dr.gather([pushes], 2, 30.0, 2 * math.pi, ROBOT_SIZE, 4, np.zeros((1, 3)))
    assert out["num"].tolist() == [2] and out["in_range"].tolist() == [2]
    assert out["src"].tolist() == [[0, 2, -1, -1]] and out["hist_len"].tolist() == [[1, 1, 0, 0]]
    assert not out["pos_hist"][0, 2:].any() and not out["cur_size"][0, 2:].any()
    assert out["cur_vel"][0, 1].tolist() == [1.0, 1.0, 0.0]
    out = dr.gather([pushes], 2, 30.0, 2 * math.pi, ROBOT_SIZE, 1, np.zeros((1, 3)))   # K = 1 < 2 in range
    assert out["num"].tolist() == [1] and out["in_range"].tolist() == [2] and out["src"].tolist() == [[0]]


# ---------------------------------------------------------------- the kernel's predicate on the host
def test_host_compiled_predicate_matches_restatement():
    lib = C.CDLL(DETECT_HARNESS)
    n = 4000
    rng = np.random.default_rng(77)
    robot = rng.uniform(-10, 10, (n, 3))
    yaw = rng.uniform(-math.pi, math.pi, n)
    ob = rng.uniform(-40, 40, (n, 3))
    fov = np.where(rng.uniform(size=n) < 0.25, 2 * math.pi, rng.uniform(0.2, 2 * math.pi, n))
    rg = rng.uniform(5.0, 45.0, n)
    # a few tuples on the thresholds themselves (the discard rule's business)
    ob[:8, :2] = robot[:8, :2] + rg[:8, None] * np.stack([np.cos(yaw[:8]), np.sin(yaw[:8])], axis=1)
    out = np.zeros(n, np.int8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    lib.detect_in_range(C.c_int64(n), p(robot), p(yaw), p(ob), p(fov), p(rg), C.c_int32(1), p(out))
    det = dr.FakeDetector(1, 0.0)
    keep, ref = [], []
    for k in range(n):
        md, ma = dr.margins(robot[k], yaw[k], ob[k], fov[k], rg[k])
        if md <= MARGIN or ma <= MARGIN:
            continue
        det.robot_pos, det.robot_yaw, det.color_distance = robot[k].tolist(), float(yaw[k]), float(rg[k])
        keep.append(k)
        ref.append(det.is_obstacle_in_sensor_range(dr.box(ob[k], (0, 0, 0), (0, 0, 0)), float(fov[k])))
    assert n - len(keep) < n // 100, n - len(keep)   # the discard rule removes under 1 %
    np.testing.assert_array_equal(out[keep].astype(bool), ref)
    assert 0.2 < np.mean(ref) < 0.8                   # both decisions are exercised
    # the robot_yaw == NULL path (fov >= 2 pi: distance only)
    full = np.full(n, 2 * math.pi)
    lib.detect_in_range(C.c_int64(n), p(robot), p(yaw), p(ob), p(full), p(rg), C.c_int32(0), p(out))
    keep, ref = [], []
    for k in range(n):
        if dr.margins(robot[k], yaw[k], ob[k], 2 * math.pi, rg[k])[0] <= MARGIN:
            continue
        det.robot_pos, det.robot_yaw, det.color_distance = robot[k].tolist(), float(yaw[k]), float(rg[k])
        keep.append(k)
        ref.append(det.is_obstacle_in_sensor_range(dr.box(ob[k], (0, 0, 0), (0, 0, 0)), 2 * math.pi))
    assert n - len(keep) < n // 100
    np.testing.assert_array_equal(out[keep].astype(bool), ref)
    # NaN inputs fail the comparisons
    nan = np.array([[math.nan, 0.0, 0.0]])
    one = np.zeros(1, np.int8)
    z, f, r = np.zeros(1), np.array([2 * math.pi]), np.array([30.0])
    for rb, o_, y_ in ((nan, np.zeros((1, 3)), z), (np.zeros((1, 3)), nan, z), (np.zeros((1, 3)), np.ones((1, 3)), z + math.nan)):
        lib.detect_in_range(C.c_int64(1), p(rb), p(y_), p(o_), p(f), p(r), C.c_int32(1), p(one))
        assert one[0] == 0


# ---------------------------------------------------------------- the gate on the device
def _world(seed, I, M, worlds, pushes, spread=40.0):
    """Seeded pushes per world (time order) and robot poses."""
    rng = np.random.default_rng(seed)
    wp = []
    for _ in range(worlds):
        pos = rng.uniform(-spread, spread, (M, 3))
        vel = rng.uniform(-2.0, 2.0, (M, 3))       # a z velocity too: the store keeps (Vx, Vy, 0)
        size = rng.uniform(0.3, 1.5, (M, 3))
        wp.append([(pos + vel * (0.033 * n), vel + 0.01 * n, size + 0.001 * n) for n in range(pushes)])
    robot = rng.uniform(-10.0, 10.0, (I, 3))
    yaw = rng.uniform(-math.pi, math.pi, I)
    return wp, robot, yaw


def _assert_margins(wp, robot, yaw, fov, rng_m):
    for i in range(len(robot)):
        pushes = wp[0] if len(wp) == 1 else wp[i]
        if not pushes:
            continue
        for ob in pushes[-1][0]:
            md, ma = dr.margins(robot[i], 0.0 if yaw is None else yaw[i], ob, fov, rng_m)
            assert md > MARGIN, "seed puts a pair on the range threshold: pick another"
            assert fov >= 2 * math.pi or ma > MARGIN, "seed puts a pair on the angle threshold: pick another"


def _device_gather(ctx, wp, M, H, params, robot, yaw, buffers=None):
    from impc import DeviceArray, perception as P
    I = len(robot)
    tr = P.Tracks(ctx, len(wp), M, H)
    gb = buffers if buffers is not None else P.GateBuffers(ctx, I, params.max_out, H)
    rp_d = DeviceArray(ctx, np.ascontiguousarray(robot))
    ry_d = DeviceArray(ctx, np.ascontiguousarray(yaw)) if yaw is not None else None
    try:
        for n in range(len(wp[0])):
            tr.push(*[np.stack([w[n][k] for w in wp]) for k in range(3)])
        P.gather_device(tr, params, I, rp_d.ptr, ry_d.ptr if ry_d else None, gb.out)
        ctx.synchronize()
        return gb.get()
    finally:
        rp_d.free()
        if ry_d:
            ry_d.free()
        tr.close()
        if buffers is None:
            gb.free()


def _compare(got, ref):
    for k in ("num", "in_range", "src", "hist_len", "cur_pos", "cur_vel", "cur_size", "pos_hist", "vel_hist"):
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, k
        assert np.array_equal(got[k], ref[k]), (k, np.argwhere(got[k] != ref[k])[:5])


HALF = math.pi / 2
FULL = 2 * math.pi
# (I, M, K, worlds, H, pushes, fov, with_yaw, range): M over the ballot's chunk boundaries, K = 1 / 4 / M,
# more than one workgroup, one world and one per instance, an empty / partly filled / wrapped ring
CASES = [
    (1, 1, 1, 1, 1, 3, FULL, False, 30.0),       # H = 1: every push lands on the only entry
    (3, 63, 4, 1, 5, 3, FULL, False, 30.0),      # fov = 2 pi and robot_yaw = NULL
    (3, 64, 64, 3, 5, 7, FULL, True, 30.0),      # K = M, wrapped ring, a world per instance
    (70, 65, 4, 1, 5, 7, FULL, False, 30.0),
    (70, 130, 130, 70, 1, 3, FULL, False, 30.0),
    (3, 130, 4, 3, 5, 0, FULL, False, 30.0),     # nothing tracked: all num = 0
    (3, 65, 4, 1, 5, 3, FULL, False, 1e3),       # every obstacle in range, M > K: truncation
    (3, 64, 4, 3, 5, 3, FULL, False, 0.05),      # none in range
    (70, 130, 4, 1, 5, 3, HALF, True, 30.0),     # fov = pi / 2 and a yaw array
    (3, 63, 63, 3, 5, 7, HALF, True, 30.0),
    (1, 130, 1, 1, 5, 3, FULL, True, 30.0),
    (70, 1, 1, 70, 5, 3, HALF, True, 30.0),
    (3, 130, 70, 1, 5, 3, FULL, False, 1e3),     # truncation in the second chunk: 64 < K < in-range count
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: "I{}-M{}-K{}-W{}-H{}-p{}-fov{:.1f}-yaw{:d}-r{:g}".format(*c))
def test_gate_matches_restatement_byte_for_byte(ctx, case):
    from impc import perception as P
    I, M, K, worlds, H, pushes, fov, with_yaw, rng_m = case
    wp, robot, yaw = _world(900 + 7 * CASES.index(case), I, M, worlds, pushes)
    yaw = yaw if with_yaw else None
    _assert_margins(wp, robot, yaw, fov, rng_m)
    ref = dr.gather(wp, H, rng_m, fov, ROBOT_SIZE, K, robot, yaw)
    got = _device_gather(ctx, wp, M, H, P.detect_params(rng_m, fov, ROBOT_SIZE, K), robot, yaw)
    _compare(got, ref)
    if pushes == 0:
        assert not got["num"].any() and not got["in_range"].any()
    elif rng_m >= 1e3:
        assert (got["num"] == K).all() and (got["in_range"] == M).all()
        assert (got["src"] == np.arange(K)).all()
    elif rng_m < 1.0:
        assert not got["in_range"].any()
    elif I * M >= 60:
        assert 0 < got["in_range"].sum() < I * M      # the gate decides both ways
    if pushes > H and got["num"].any():
        assert got["hist_len"].max() == H


@pytest.mark.gpu
def test_second_gather_leaves_no_stale_data(ctx):
    from impc import perception as P
    I, M, K, H = 5, 70, 8, 5
    wp, robot, _ = _world(31, I, M, 1, 7)
    gb = P.GateBuffers(ctx, I, K, H)
    try:
        _assert_margins(wp, robot, None, FULL, 30.0)
        first = _device_gather(ctx, wp, M, H, P.detect_params(30.0, FULL, ROBOT_SIZE, K), robot, None, buffers=gb)
        assert (first["num"] == K).all() and first["pos_hist"].any()          # many detections
        second = _device_gather(ctx, wp, M, H, P.detect_params(0.05, FULL, ROBOT_SIZE, K), robot, None, buffers=gb)
        _assert_margins(wp, robot, None, FULL, 0.05)
        assert not second["num"].any() and not second["in_range"].any()
        assert (second["src"] == -1).all() and not second["hist_len"].any()
        for k in ("pos_hist", "vel_hist", "cur_pos", "cur_vel", "cur_size"):
            assert not second[k].any() and not np.signbit(second[k]).any(), k
        # a reset store tracks nothing either
        tr = P.Tracks(ctx, 1, M, H)
        tr.push(*[a[None] for a in wp[0][0]])
        tr.reset()
        got = P.gather(tr, P.detect_params(1e3, FULL, ROBOT_SIZE, K), robot)
        tr.close()
        assert not got["num"].any() and (got["src"] == -1).all()
    finally:
        gb.free()


@pytest.mark.gpu
def test_argument_errors(ctx):
    import impc
    from impc import perception as P
    I, M, K, H = 3, 4, 2, 3
    tr = P.Tracks(ctx, 1, M, H)
    gb = P.GateBuffers(ctx, I, K, H)
    rp_d = impc.DeviceArray(ctx, np.zeros((I, 3)))
    try:
        ctx.synchronize()
        before = {k: a.get() for k, a in gb.arrays.items()}
        for params in (P.detect_params(30.0, HALF, ROBOT_SIZE, K),      # fov < 2 pi without yaw
                       P.detect_params(30.0, FULL, ROBOT_SIZE, 0),      # max_out < 1
                       P.detect_params(30.0, FULL, ROBOT_SIZE, -3)):
            with pytest.raises(impc.ImpcError) as e:
                P.gather_device(tr, params, I, rp_d.ptr, None, gb.out)
            assert e.value.code == P.INVALID_ARGUMENT
            with pytest.raises(impc.ImpcError) as e:
                P.gather(tr, params, np.zeros((I, 3)))
            assert e.value.code == P.INVALID_ARGUMENT
        ctx.synchronize()
        for k, a in gb.arrays.items():                                   # no launch happened
            assert np.array_equal(a.get(), before[k], equal_nan=True), k
        tr2 = P.Tracks(ctx, 2, M, H)                                     # a store of 2 worlds, 3 instances
        try:
            with pytest.raises(impc.ImpcError) as e:
                P.gather_device(tr2, P.detect_params(30.0, FULL, ROBOT_SIZE, K), I, rp_d.ptr, None, gb.out)
        finally:
            tr2.close()
        assert e.value.code == P.INVALID_ARGUMENT
        for bad in ((0, M, H), (1, 0, H), (1, M, 0)):
            with pytest.raises(impc.ImpcError) as e:
                P.Tracks(ctx, *bad)
            assert e.value.code == P.INVALID_ARGUMENT
    finally:
        rp_d.free()
        gb.free()
        tr.close()


@pytest.mark.gpu
def test_host_array_variant_gives_the_same_bytes(ctx):
    from impc import perception as P
    I, M, K, H = 7, 65, 4, 5
    wp, robot, yaw = _world(55, I, M, I, 7)
    params = P.detect_params(30.0, HALF, ROBOT_SIZE, K)
    _assert_margins(wp, robot, yaw, HALF, 30.0)
    dev = _device_gather(ctx, wp, M, H, params, robot, yaw)
    tr = P.Tracks(ctx, I, M, H)
    try:
        for n in range(7):
            tr.push(*[np.stack([w[n][k] for w in wp]) for k in range(3)])
        host = P.gather(tr, params, robot, yaw)
        _compare(host, dev)
        some = P.gather(tr, params, robot, yaw, fields=("src", "cur_size"))   # optional outputs left out
        assert sorted(some) == ["cur_size", "num", "src"]
        assert np.array_equal(some["src"], dev["src"]) and np.array_equal(some["cur_size"], dev["cur_size"])
    finally:
        tr.close()
    assert dev["in_range"].any()


def test_struct_layouts_match_the_header(tmp_path):
    """impc_detect_params / impc_detect_out: the ctypes mirror's size and field offsets equal the C
    compiler's for include/impc_detect.h."""
    import subprocess
    from impc.perception import DetectOut, DetectParams
    structs = (("impc_detect_params", DetectParams), ("impc_detect_out", DetectOut))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "impc_detect.h"', "int main(void) {"]
    for cname, py in structs:
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        for f, _ in py._fields_:
            lines.append(f'printf("%zu\\n", offsetof({cname}, {f}));')
    lines.append("return 0; }")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = []
    for _, py in structs:
        want.append(C.sizeof(py))
        want += [getattr(py, f).offset for f, _ in py._fields_]
    assert got == want
