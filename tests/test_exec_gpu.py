"""impc_replan_target_device / impc_replan_check_device (include/impc_exec.h) and the replan's ref_
state on the device, against the Python restatement tests/exec_ref.py.

Isolated: a DeviceReplan with I = 67 instances (not a multiple of the wavefront), K = 3 box slots, its
state set from the host (set_state + set_ref, no solve) with tests/exec_cases.py's cases, at (N, ts) =
(20, 0.1), (5, 0.02) and (110, 0.02) -- the last has loops of 101 samples, more than one wavefront
round (a horizon the grouped solve does not take: the object only holds the state).  Positions, velocities, accelerations, reference points, done, the look-ahead's sample, both
collision steps and the replan flag are compared bit for bit, and so is the yaw wherever it is an
input passed through (HOLD, FACING, no look-ahead hit, leftTime <= 0).

The look-ahead's yaw is atan2 on the device, which is not the host's atan2.  The sample it stops at
is compared exactly (yaw_step), and its arguments are differences of values that are compared bit for
bit, so the only difference is the function's own.  No documented error bound of the device's atan2
was at hand, so the difference was measured on this test's own inputs (the look-ahead hits of all
three configurations, on an MI355X): the largest is
ATAN2_ULP_MEASURED = 1 ulp of the restatement's value (4.4e-16 rad), and the test allows twice that,
and never more than 1e-12 rad.

End to end: six vehicles on scenarios.live_world in tests/test_tick.py's set-up, two replans through
DeviceTick; after each, the committed ref_, the target one step into the fresh plan and the tick's
check against the restatement on the plans, gate outputs and map read back.
"""
import ctypes as C
import math

import numpy as np
import pytest

import impc
from impc import execution as E
from impc.replan import DeviceReplan

import exec_cases as ec
import exec_ref as er

pytestmark = pytest.mark.gpu

I, K, L = 67, 3, 3
INVALID_ARGUMENT, UNSUPPORTED = 101, 102
ATAN2_ULP_MEASURED = 1   # largest |device - host| atan2 difference seen, in ulp of the host's value
ATAN2_ULP_BOUND = 2 * ATAN2_ULP_MEASURED
SENT = -77.0
D = impc.DeviceArray


def _replan(ctx, N, ts, instances=I, k=K):
    p, pd = impc.mpc_params(horizon=N, ts=ts)
    return DeviceReplan(ctx, p, pd, instances, k, L, impc.default_settings(verbose=0))


class _Dev:
    """The cases' inputs on the device and sentinel-filled outputs."""

    def __init__(self, ctx, c):
        self.ctx, n = ctx, c["I"]
        self.inp = {k: D(ctx, np.ascontiguousarray(c[k])) for k in
                    ("t", "ready", "cur_pos", "odom_yaw", "facing_yaw", "num_obs", "ob_pos", "ob_size")}
        self.occ = D(ctx, np.ascontiguousarray(c["occ"].reshape(-1)))
        m = c["map"]
        self.omap = impc.OccMap(resolution=m["res"])
        self.omap.origin[:] = m["origin"]
        self.omap.dims[:] = m["dims"]
        self.tgt = E.TargetBuffers(ctx, n, fill=SENT)
        self.chk = E.CheckBuffers(ctx, n, fill=int(SENT))

    def refill(self):
        for b in (self.tgt, self.chk):
            for a in b.arrays.values():
                a.set(np.full(a.shape, SENT, a.dtype))

    def target(self, rp, mode, ready=True, forward_dist=1.0):
        self.refill()
        i = self.inp
        E.target_device(rp, mode, i["t"].ptr, i["cur_pos"].ptr, i["odom_yaw"].ptr, ready=i["ready"].ptr if ready else None,
                        facing_yaw=i["facing_yaw"].ptr, forward_dist=forward_dist, **self.tgt.ptrs())
        self.ctx.synchronize()
        return self.tgt.get()

    def check(self, rp, ready=True, with_map=True, with_boxes=True):
        self.refill()
        i = self.inp
        E.check_device(rp, i["t"].ptr, i["cur_pos"].ptr, ready=i["ready"].ptr if ready else None, omap=self.omap,
                       occ=self.occ.ptr if with_map else None, num_obs=i["num_obs"].ptr if with_boxes else None,
                       ob_pos=i["ob_pos"].ptr, ob_size=i["ob_size"].ptr, **self.chk.ptrs())
        self.ctx.synchronize()
        return self.chk.get()

    def free(self):
        for a in list(self.inp.values()) + [self.occ]:
            a.free()
        self.tgt.free()
        self.chk.free()


def _ulps(got, want):
    """|got - want| in units of want's ulp."""
    return np.abs(got - want) / np.spacing(np.abs(want))


def _cmp_target(got, ref, served, what, yaw_exact):
    """Bit for bit where served, the sentinel elsewhere; the yaw only where it is passed through."""
    worst = 0.0
    for k in ("pos", "vel", "acc", "ref", "done", "yaw_step"):
        np.testing.assert_array_equal(got[k][served], ref[k][served], err_msg=f"{what}: {k}")
        assert (got[k][~served] == np.asarray(SENT).astype(got[k].dtype)).all(), f"{what}: {k} of an instance not ready"
    assert (got["yaw"][~served] == SENT).all()
    through = served & (True if yaw_exact else ref["yaw_step"] < 0)
    np.testing.assert_array_equal(got["yaw"][through], ref["yaw"][through], err_msg=f"{what}: yaw")
    looked = served & ~through
    if looked.any():
        u = _ulps(got["yaw"][looked], ref["yaw"][looked])
        zero = ref["yaw"][looked] == 0.0   # atan2(0, 0) at forward_dist = 0
        assert (got["yaw"][looked][zero] == 0.0).all()
        worst = float(u[~zero].max()) if (~zero).any() else 0.0
        print(f"{what}: {int(looked.sum())} look-ahead yaws, largest device/host atan2 difference {worst:g} ulp, "
              f"{float(np.abs(got['yaw'][looked] - ref['yaw'][looked]).max()):.3e} rad")
        assert worst <= ATAN2_ULP_BOUND, (what, worst)
        assert np.abs(got["yaw"][looked] - ref["yaw"][looked]).max() <= 1e-12
    return worst


@pytest.mark.parametrize("N,ts", [(20, 0.1), (5, 0.02), (110, 0.02)])
def test_target_and_check_match_restatement(ctx, N, ts):
    c = ec.make(I, N, ts, K, seed=2000 + N)
    has_plan = c["count"] > 0
    rc_dev = np.where(has_plan, N, 0).astype(np.int32)   # set_ref: every instance with a plan has a ref_
    ref = ec.reference(c, ref_count=rc_dev)
    cl = ec.classes(ref)
    print(f"N={N} ts={ts}: {cl}")
    ec.assert_classes(cl, I)
    if N == 110:  # more samples than one wavefront round holds, with hits past the first round
        assert (ref["map_step"] >= 64).any() and (ref[er.YAW_SMOOTH]["yaw_step"] >= 64).any(), \
            (ref["map_step"].max(), ref[er.YAW_SMOOTH]["yaw_step"].max())
    rp = _replan(ctx, N, ts)
    dv = _Dev(ctx, c)
    try:
        if N == 110:  # 13 N - 5 variables are beyond the grouped solve's kernel: the object holds state only
            with pytest.raises(impc.ImpcError) as e:
                rp.run_device(*[dv.inp["t"].ptr] * 7)
            assert e.value.code == UNSUPPORTED
        x = c["plan_x"]
        rp.set_state(x[:, :8 * N].reshape(I, N, 8), (~has_plan).astype(np.int8), x[:, 8 * N:].reshape(I, N - 1, 5))
        ready = c["ready"] == 1
        # ---- before set_ref every ref_ is empty: getRef is currPos_, the look-ahead finds nothing
        pr, rc = rp.refs()
        assert not rc.any() and not pr.any()
        ref0 = ec.reference(c, ref_count=np.zeros(I, np.int32))[er.YAW_SMOOTH]
        assert (ref0["yaw_step"] == -1).all()
        np.testing.assert_array_equal(ref0["ref"], c["cur_pos"])
        _cmp_target(dv.target(rp, er.YAW_SMOOTH), ref0, ready, "empty ref_", yaw_exact=True)
        rp.set_ref(c["plan_ref"])
        pr, rc = rp.refs()
        np.testing.assert_array_equal(pr, c["plan_ref"])
        np.testing.assert_array_equal(rc, rc_dev)
        # ---- the target in the three yaw modes, and the look-ahead at forward_dist = 0
        _cmp_target(dv.target(rp, er.YAW_FACING), ref[er.YAW_FACING], ready, "FACING", yaw_exact=True)
        _cmp_target(dv.target(rp, er.YAW_HOLD), ref[er.YAW_HOLD], ready, "HOLD", yaw_exact=True)
        _cmp_target(dv.target(rp, er.YAW_SMOOTH), ref[er.YAW_SMOOTH], ready, "SMOOTH", yaw_exact=False)
        _cmp_target(dv.target(rp, er.YAW_SMOOTH, forward_dist=0.0), ref["smooth0"], ready, "SMOOTH fd=0", yaw_exact=False)
        # ready = NULL: the instances that hold a plan
        _cmp_target(dv.target(rp, er.YAW_HOLD, ready=False), ref[er.YAW_HOLD], has_plan, "HOLD, ready NULL", yaw_exact=True)
        # ---- the collision tests
        for kw, served in ((dict(), ready), (dict(ready=False), has_plan)):
            got = dv.check(rp, **kw)
            np.testing.assert_array_equal(got["map_step"], np.where(served, ref["map_step"], -1))
            np.testing.assert_array_equal(got["dyn_step"], np.where(served, ref["dyn_step"], -1))
            np.testing.assert_array_equal(got["replan_flag"], np.where(served, ref["replan"], 0))
        got = dv.check(rp, with_map=False)
        assert (got["map_step"] == -1).all()
        np.testing.assert_array_equal(got["dyn_step"], np.where(ready, ref["dyn_step"], -1))
        np.testing.assert_array_equal(got["replan_flag"], (got["dyn_step"] >= 0).astype(np.int8))
        got = dv.check(rp, with_boxes=False)
        assert (got["dyn_step"] == -1).all()
        np.testing.assert_array_equal(got["map_step"], np.where(ready, ref["map_step"], -1))
        # set_state empties every ref_ again
        rp.set_state(x[:, :8 * N].reshape(I, N, 8), (~has_plan).astype(np.int8))
        assert not rp.refs()[1].any()
    finally:
        dv.free()
        rp.close()


def test_two_replans_through_the_tick(ctx):
    from test_tick import _Loop, I as NV, K as KV, N as NT
    lp = _Loop(ctx, 2, 28.0, predictor=True)
    ts = lp.pd["ts"]
    n = 13 * NT - 5
    t_step, t_zero, yaw = D(ctx, np.full(NV, ts)), D(ctx, np.linspace(0.0, 1.2, NV)), D(ctx, np.linspace(-1.0, 1.0, NV))
    tgt = E.TargetBuffers(ctx, NV, fill=SENT)
    try:
        prev_ref, ever = np.zeros((NV, NT, 3)), np.zeros(NV, bool)
        for r in range(2):
            pos, vel, xref, out, gate = lp.replan(r)
            plan_x, _, pc, valid = lp.rp.plans()
            ok = valid == 1
            assert ok.any()
            ever |= ok
            # ---- ref_ of the commit
            plan_ref, ref_count = lp.rp.refs()
            np.testing.assert_array_equal(plan_ref, np.where(ok[:, None, None], xref[:, :, :3], prev_ref))
            np.testing.assert_array_equal(ref_count, np.where(ever, NT, 0))
            np.testing.assert_array_equal(pc > 0, ever)
            prev_ref = plan_ref
            # ---- one step into the plan: its state 1 and control 1
            lp.tick.target(E.YAW_HOLD, t_step.ptr, lp.pos_d.ptr, yaw.ptr, tgt.ptrs())
            ctx.synchronize()
            got = tgt.get()
            np.testing.assert_array_equal(got["pos"][ever], plan_x[ever, 8:11])
            np.testing.assert_array_equal(got["vel"][ever], plan_x[ever, 11:14])
            np.testing.assert_array_equal(got["acc"][ever], plan_x[ever, 8 * NT + 5:8 * NT + 8])
            assert (got["pos"][~ever] == SENT).all() and not got["done"][ever].any()
            # ---- the tick's check against the restatement on what the device holds
            chk = lp.tick.check(t_zero.ptr, lp.pos_d.ptr)
            ctx.synchronize()
            got = chk.get()
            plans = er.plans_from_arrays(plan_x, plan_ref, pc, ref_count, pos, NT, ts)
            ms, ds, flag = er.check_batch(plans, t_zero.get(), lp.w["map"], lp.w["occ"].reshape(-1), gate["num"],
                                          gate["cur_pos"], gate["cur_size"])
            np.testing.assert_array_equal(got["map_step"], np.where(ever, ms, -1))
            np.testing.assert_array_equal(got["dyn_step"], np.where(ever, ds, -1))
            np.testing.assert_array_equal(got["replan_flag"], np.where(ever, flag, 0))
            lp.rp.advance_device(ts, lp.pos_d.ptr, lp.vel_d.ptr)
        assert plan_x.shape == (NV, n) and gate["num"].max() <= KV
    finally:
        for d in (t_step, t_zero, yaw):
            d.free()
        tgt.free()
        lp.close()


def test_argument_errors_launch_nothing(ctx):
    n, N = 3, 5
    rp = _replan(ctx, N, 0.1, instances=n, k=1)
    bufs = dict(t=D(ctx, np.zeros(n)), cur_pos=D(ctx, np.zeros((n, 3))), odom_yaw=D(ctx, np.zeros(n)),
                facing_yaw=D(ctx, np.zeros(n)), num_obs=D(ctx, np.ones(n, np.int32)), ob=D(ctx, np.zeros((n, 1, 3))),
                occ=D(ctx, np.zeros(8, np.uint8)))
    tgt, chk = E.TargetBuffers(ctx, n, fill=SENT), E.CheckBuffers(ctx, n, fill=int(SENT))
    omap = impc.OccMap(resolution=1.0)
    omap.dims[:] = [2, 2, 2]

    def refused(call, *a, **kw):
        with pytest.raises(impc.ImpcError) as e:
            call(*a, **kw)
        assert e.value.code == INVALID_ARGUMENT, e.value

    def target(rp_=rp, mode=E.YAW_HOLD, **over):
        kw = dict(t=bufs["t"].ptr, cur_pos=bufs["cur_pos"].ptr, odom_yaw=bufs["odom_yaw"].ptr,
                  facing_yaw=bufs["facing_yaw"].ptr, **tgt.ptrs())
        kw.update(over)
        E.target_device(rp_, mode, **kw)

    def check(rp_=rp, **over):
        kw = dict(t=bufs["t"].ptr, cur_pos=bufs["cur_pos"].ptr, omap=omap, occ=bufs["occ"].ptr, num_obs=bufs["num_obs"].ptr,
                  ob_pos=bufs["ob"].ptr, ob_size=bufs["ob"].ptr, **chk.ptrs())
        kw.update(over)
        E.check_device(rp_, **kw)

    class _Null:
        h = None

    try:
        # no plan state yet: neither set_state nor a run on this object
        refused(target)
        refused(check)
        rp.set_state(np.zeros((n, N, 8)), np.zeros(n, np.int8))
        refused(target, _Null)
        refused(check, _Null)
        for k in ("t", "cur_pos", "odom_yaw", "pos", "vel", "acc", "yaw", "done"):
            refused(target, **{k: None})
        refused(target, mode=-1)
        refused(target, mode=3)
        refused(target, mode=E.YAW_FACING, facing_yaw=None)
        for k in ("t", "cur_pos", "map_step", "dyn_step", "replan_flag"):
            refused(check, **{k: None})
        refused(check, ob_pos=None)
        refused(check, ob_size=None)
        for res, dims in ((0.0, (2, 2, 2)), (-1.0, (2, 2, 2)), (float("nan"), (2, 2, 2)), (1.0, (0, 2, 2)), (1.0, (2, 2, -1))):
            bad = impc.OccMap(resolution=res)
            bad.dims[:] = dims
            refused(check, omap=bad)
        # null parameter blocks, straight through the C-ABI
        p, i, o = E.TargetParams(yaw_mode=E.YAW_HOLD, forward_dist=1.0), E.TargetIn(), E.TargetOut()
        assert impc.lib.impc_replan_target_device(rp.h, None, C.byref(i), C.byref(o)) == INVALID_ARGUMENT
        assert impc.lib.impc_replan_target_device(rp.h, C.byref(p), None, C.byref(o)) == INVALID_ARGUMENT
        assert impc.lib.impc_replan_target_device(rp.h, C.byref(p), C.byref(i), None) == INVALID_ARGUMENT
        assert impc.lib.impc_replan_check_device(rp.h, None, C.byref(E.CheckOut())) == INVALID_ARGUMENT
        assert impc.lib.impc_replan_check_device(rp.h, C.byref(E.CheckIn()), None) == INVALID_ARGUMENT
        assert impc.lib.impc_replan_set_ref(rp.h, None) == INVALID_ARGUMENT
        assert impc.lib.impc_replan_set_ref(None, None) == INVALID_ARGUMENT
        # nothing was launched: every output still holds the sentinel
        ctx.synchronize()
        for b in (tgt, chk):
            for k, a in b.get().items():
                assert (a == np.asarray(SENT).astype(a.dtype)).all(), k
        # and the same calls with every argument in place are accepted
        target(ref=None, yaw_step=None)
        check(occ=None)
        check(num_obs=None, ob_pos=None, ob_size=None)
        ctx.synchronize()
        assert (chk.get()["replan_flag"] == 0).all() and not math.isnan(tgt.get()["yaw"][0])
    finally:
        for d in bufs.values():
            d.free()
        tgt.free()
        chk.free()
        rp.close()
