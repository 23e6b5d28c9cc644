"""The whole planner tick on the device (impc.perception.DeviceTick): per replan three history
pushes (fakeDetector::histCB's 0.033 s timer against the 0.1 s replan), the sensor-range gate
(include/impc_detect.h), the predictor (impc_intent_prob_device / impc_predict_traj_device over all
I * K slots) and impc_replan_run with num_pred = the gate's K_i, then the vehicle following its plan
(impc_replan_advance_device) -- six vehicles on scenarios.live_world, five obstacles each, K = 4
slots, so K_i changes as the vehicles fly past and one vehicle sees more obstacles than it has slots.

Every replan is checked at the positions read back from the device: the gate's outputs against
tests/detect_ref.py byte for byte (every pair at least 1e-3 m from the range threshold; positions
carry solver differences of order 1e-5 at most), and the replan's records against
oracle/replan_ref.py fed the device's own predictions and the gate's K_i, with
tests/test_live_loop.py's rules (test_replan_branches._check_replan, unchanged).  At the replan with
the most detections the predictor's outputs of the occupied slots are compared with
oracle/predict_ref.py at tests/test_predict.py's tolerances.

The range and seed were chosen on the CPU with the restatement and the vehicles' obstacle-free
plans (3.85 m of advance over the ten replans): seed 4105 at 28 m gives K_i = (1 3 4 2 3 1) at the
first and (2 3 4 2 4 2) at the last replan, in_range = 5 for vehicle 2, and a smallest margin of
0.18 m; at 20 m the first three replans see (0 1 4 2 2 1), margin 0.26 m."""
import math

import numpy as np
import pytest

import impc
from impc import scenarios
from impc.replan import FANOUT, SINGLE_CURRENT, SINGLE_FIRST, DeviceReplan
from oracle import predict_ref as pr
from oracle.reftraj_ref import ReferencePath

import detect_ref as dr
from test_replan_branches import _check_replan

pytestmark = pytest.mark.gpu

I, M, K, N, H, PUSHES = 6, 5, 4, 30, 8, 3
SEED = 4105
ROBOT_SIZE = (0.4, 0.4, 0.2)
MIN_MARGIN = 1e-3


class _Loop:
    """The closed loop's device state and its host replay."""

    def __init__(self, ctx, replans, range_m, predictor):
        from impc import perception as P
        self.ctx, self.P, self.range_m = ctx, P, range_m
        self.w = w = scenarios.live_world(I, M, replans, pushes_per_replan=PUSHES, N=N, seed=SEED)
        self.pd, self.L = w["pd"], w["L"]
        self.s = impc.default_settings(verbose=0)
        self.rp = DeviceReplan(ctx, w["params"], self.pd, I, K, self.L, self.s)
        self.paths = impc.ReferencePaths(ctx, list(w["paths"]), self.pd["ts"], N)
        self.refs = [ReferencePath(p, self.pd["ts"], N) for p in w["paths"]]
        self.tracks = P.Tracks(ctx, I, M, H)
        self.params = P.detect_params(range_m, P.FOV_ALL, ROBOT_SIZE, K)
        self.tick = P.DeviceTick(ctx, self.rp, self.tracks, self.params, occ=w["occ"], omap=w["map"],
                                 predictor=predictor)
        D = impc.DeviceArray
        self.pos_d, self.vel_d, self.xref_d = D(ctx, w["pos0"]), D(ctx, w["vel0"]), D(ctx, (I, N, 8))
        self.world_d = D(ctx, np.ascontiguousarray(w["world_pos"]))
        self.wvel_d, self.wsize_d = D(ctx, np.ascontiguousarray(w["world_vel"])), D(ctx, w["world_size"])
        self.pushed = 0
        self.plan_x, self.ft = np.zeros((I, 13 * N - 5)), np.ones(I, np.int8)

    def replan(self, r):
        """Replan r on the device (pushes, xref, tick); returns (pos, vel, xref, out, gate) read back,
        the gate checked against the restatement at the positions read back."""
        step = I * M * 3 * 8
        for _ in range(PUSHES):
            self.tracks.push_device(self.world_d.ptr + self.pushed * step, self.wvel_d.ptr, self.wsize_d.ptr)
            self.pushed += 1
        self.paths.xref_device(self.pos_d.ptr, self.xref_d.ptr)
        self.tick.run_device(self.pos_d.ptr, self.vel_d.ptr, self.xref_d.ptr)
        self.ctx.synchronize()
        pos, vel, xref = self.pos_d.get(), self.vel_d.get(), self.xref_d.get()
        gate = self.tick.gate.get()
        w = self.w
        for i in range(I):
            for ob in w["world_pos"][self.pushed - 1][i]:
                md, _ = dr.margins(pos[i], 0.0, ob, 2 * math.pi, self.range_m)
                assert md >= MIN_MARGIN, (r, i, md)
        pushes = [[(w["world_pos"][n][i], w["world_vel"][i], w["world_size"][i]) for n in range(self.pushed)]
                  for i in range(I)]
        ref = dr.gather(pushes, H, self.range_m, 2 * math.pi, ROBOT_SIZE, K, pos)
        for k, v in ref.items():
            assert np.array_equal(gate[k], v), (r, k)
        np.testing.assert_array_equal(xref, np.array([self.refs[i].xref(pos[i]) for i in range(I)]))
        return pos, vel, xref, self.rp.results(), gate

    def commit(self, r, expect, expect_first):
        """The committed plans against the restatement's; the vehicles follow their plans."""
        plan_x, ft, _, valid = self.rp.plans()
        np.testing.assert_array_equal(plan_x, expect, err_msg=f"replan {r}: committed plans")
        np.testing.assert_array_equal(ft, expect_first)
        pos, vel = self.pos_d.get(), self.vel_d.get()
        self.rp.advance_device(self.pd["ts"], self.pos_d.ptr, self.vel_d.ptr)
        self.ctx.synchronize()
        # getPos / getVel(dt) of a fresh plan: its state 1
        np.testing.assert_array_equal(self.pos_d.get(), np.where(valid[:, None] == 1, plan_x[:, 8:11], pos))
        np.testing.assert_array_equal(self.vel_d.get(), np.where(valid[:, None] == 1, plan_x[:, 11:14], vel))
        self.plan_x, self.ft = plan_x, ft

    def close(self):
        for d in (self.pos_d, self.vel_d, self.xref_d, self.world_d, self.wvel_d, self.wsize_d):
            d.free()
        self.tick.close()
        self.tracks.close()
        self.paths.close()
        self.rp.close()


def test_closed_tick_loop_ten_replans(ctx):
    R, range_m = 10, 28.0
    lp = _Loop(ctx, R, range_m, predictor=True)
    nums, in_ranges, branches, most = [], [], [], None
    try:
        for r in range(R):
            pos, vel, xref, out, gate = lp.replan(r)
            pred_pos, pred_size, prob = lp.tick.pred_pos.get(), lp.tick.pred_size.get(), lp.tick.prob.get()
            try:
                expect, expect_first = _check_replan(out, (lp.plan_x, lp.ft, None, None), pos, vel, xref,
                                                     gate["cur_pos"], pred_pos, pred_size, prob, np.ones(I, bool),
                                                     None, np.zeros(I, np.int32), lp.pd, lp.s, num_pred=gate["num"])
            except AssertionError as e:
                raise AssertionError(f"replan {r}: {e}") from e
            lp.commit(r, expect, expect_first)
            nums.append(gate["num"].copy())
            in_ranges.append(gate["in_range"].copy())
            branches.append(out["branch"].copy())
            if most is None or gate["num"].sum() > most[0]["num"].sum():
                most = (gate, pred_pos, pred_size, prob)
        nums, in_ranges, br = np.array(nums), np.array(in_ranges), np.array(branches)
        print("K_i per replan:", nums.tolist(), "in_range max", in_ranges.max(axis=0).tolist())
        assert len(np.unique(nums)) >= 3                        # at least three distinct K_i over the run
        assert (nums[1:] != nums[:-1]).any()                    # a K_i changes between consecutive replans
        assert (in_ranges == M).any() and M > K                 # a vehicle sees more than it has slots
        assert (br[0] == SINGLE_FIRST).all()
        assert (br[1:] == np.where(nums[1:] > 0, FANOUT, SINGLE_FIRST)).all()
        assert (lp.pos_d.get()[:, 0] > lp.w["pos0"][:, 0] + 2.0).all()     # the vehicles advanced
        # the predictor at the replan with the most detections, occupied slots only
        gate, pred_pos, pred_size, prob = most
        ipar = pr.params_from_config(0.5, 10.0, 0.1, 5.0)       # predictor_param.yaml, as impc.intent_params()
        tp = dict(num_pred=lp.L - 1, dt=lp.pd["ts"], stop_vel=0.1, front_angle_deg=10.0, min_turning_time=2.0,
                  max_turning_time=3.0, z_score=0.674)
        m, flat = lp.w["map"], lp.w["occ"].reshape(-1)
        checked = 0
        for i in range(I):
            for s_ in range(gate["num"][i]):
                n = gate["hist_len"][i, s_]
                ref = pr.intent_prob(ipar, gate["pos_hist"][i, s_, :n].tolist(), gate["vel_hist"][i, s_, :n].tolist())
                np.testing.assert_allclose(prob[i, s_], ref, rtol=1e-13, atol=1e-15)
                rpp, rps = pr.predict_traj(tp, m, flat, gate["cur_pos"][i, s_].tolist(),
                                           gate["cur_vel"][i, s_].tolist(), gate["cur_size"][i, s_].tolist())
                np.testing.assert_allclose(pred_pos[i, s_], np.asarray(rpp), rtol=1e-12, atol=1e-12)
                np.testing.assert_allclose(pred_size[i, s_], np.asarray(rps), rtol=1e-12, atol=1e-12)
                checked += 1
            for s_ in range(gate["num"][i], K):                 # empty slots: uniform intents, a point at 0
                assert prob[i, s_].tolist() == [0.25] * 4
                assert not pred_pos[i, s_].any() and not pred_size[i, s_].any()
        assert checked == gate["num"].sum() >= 12
    finally:
        lp.close()


def test_no_predictor_mode_three_replans(ctx):
    R, range_m = 3, 20.0
    lp = _Loop(ctx, R, range_m, predictor=False)
    zeros = np.zeros((I, K, 4, lp.L, 3))
    prob = np.full((I, K, 4), 0.25)
    try:
        for r in range(R):
            pos, vel, xref, out, gate = lp.replan(r)
            Ki = gate["num"]
            if r == 0:
                assert (out["branch"] == SINGLE_FIRST).all()
            else:
                assert (out["branch"] == np.where(Ki >= 1, SINGLE_CURRENT, SINGLE_FIRST)).all()
                assert (out["num_obs"] == Ki).all()
                assert (Ki == 0).any() and (Ki >= 1).any()
            expect, expect_first = _check_replan(out, (lp.plan_x, lp.ft, None, None), pos, vel, xref, gate["cur_pos"],
                                                 zeros, zeros, prob, np.zeros(I, bool), gate["cur_size"], Ki, lp.pd,
                                                 lp.s)
            lp.commit(r, expect, expect_first)
    finally:
        lp.close()
