"""Per-instance static-obstacle counts in the device replan (impc_replan_bind_static_count,
include/impc_replan.h): obclustering_->getStaticObstacles() gives every vehicle its own number of
boxes, and makePlanWithPred passes exactly that many to solveTraj and getTrajectoryScore
(mpcPlanner.cpp:594, :615-620, :652).  With counts bound the QPs of a replan are grouped by the pair
(k dynamic, s static rows per stage); every instance is compared with the restatement
oracle/replan_ref.py given its own first s_i boxes, as tests/test_replan_branches.py compares the
fixed-count replan (its horizon, instance count, scenario seeds and rules; the static rows carry a
yaw, so the assembled values are held to 1e-13 and the oracle solves what the device assembled).

The draws of test 1 (seed 4646 / rng 46 as the fixed-count test, the counts s_i from rng 48) were
checked on the CPU before they were committed: at the first replan alone instances 5, 10, 15 and 20
are on a first plan with s_i > 0, not-first instances carry s_i = 0, 1, 2 and 3, and all three
branches occur; the test asserts each of these on what the device reports."""
import ctypes as C

import numpy as np
import pytest

import impc
from impc import DeviceArray, scenarios
from impc import replan as R
from impc.replan import FANOUT, SINGLE_CURRENT, SINGLE_FIRST, DeviceReplan
from oracle import replan_ref as ref

from test_replan_branches import _row, _solution_check, _statics

I, N = 24, 20
INVALID_ARGUMENT, UNSUPPORTED = 101, 102
COUNT_SEED = 48
VIEW_KEYS = ("branch", "best_cand", "ob_idx", "cand_type", "cand_slot", "valid", "num_obs", "slot_row", "shape",
             "weighted")


# ------------------------------------------------------------------ host helpers (no GPU)
def test_shape_ids_capacities_and_signatures():
    """The host mirror of the shape ids (K + 3 + s (K + 2) + k for s < S_st), their capacities, and
    the ctypes signatures of the three entry points."""
    K, S = 4, 3
    assert R.num_shapes(K, 0) == K + 2 and R.num_shapes(K, S) == K + 3
    assert R.num_shapes(K, S, True) == (K + 2) * (S + 1) + 1 and R.num_shapes(10, 8, True) == 109
    assert R.num_shapes(K, 0, True) == K + 2
    seen = set()
    for s in range(S + 1):
        for k in range(K + 2):
            sid = R.shape_id(K, S, k, s)
            assert sid == (k if s == S else K + 3 + s * (K + 2) + k)
            assert R.shape_pair(K, S, sid) == (k, s)
            assert R.shape_capacity(7, K, S, sid) == (7 if k == 0 else 28 if k <= K else 14)
            seen.add(sid)
    assert R.shape_id(K, S, 2) == 2 and R.shape_pair(K, S, K + 2) == (0, 0) and R.shape_capacity(7, K, S, K + 2) == 7
    assert seen | {K + 2} == set(range(R.num_shapes(K, S, True)))
    for bad in ((-1, 0), (K + 2, 0), (0, -1), (0, S + 1)):
        with pytest.raises(ValueError):
            R.shape_id(K, S, *bad)
    with pytest.raises(ValueError):
        R.shape_pair(K, S, R.num_shapes(K, S, True))
    P = C.c_void_p
    f = impc.lib.impc_replan_bind_static_count
    assert f.restype is C.c_int and f.argtypes == [P, P]
    f = impc.lib.impc_replan_shape_static
    assert f.restype is C.c_int and f.argtypes[:3] == [P, C.c_int32, C.c_int32] and len(f.argtypes) == 12
    assert f.argtypes[4] == C.POINTER(C.c_int64)
    f = impc.lib.impc_replan_static_count_device
    assert f.restype is C.c_int and f.argtypes == [P, C.POINTER(P)]
    # assemble() locates a fan-out instance's candidates in the shapes of (K_i, s_i) and (K_i + 1, s_i)
    per = dict(branch=np.array([FANOUT], np.int8), num_obs=np.array([2]), slot_row=np.arange(6)[None],
               shape=np.array([R.shape_id(K, S, 2, 1)]), cand_slot=np.array([[5, 0, 1, 2, 3, 4]]),
               static_count=np.array([1]), shape_dims=(K, S))
    out = R.assemble(per, {})
    assert out["cand_rows"][0][0] == (R.shape_id(K, S, 3, 1), 5) and out["cand_rows"][0][1] == (R.shape_id(K, S, 2, 1), 0)


# ------------------------------------------------------------------ the comparison with the restatement
def _check_replan(out, before, pos, vel, xref, dyn_cur, pred, pred_size, prob, cur_size, cur_count, pd, s, num_pred,
                  static, scount, S_st):
    """One replan with bound counts against the restatement, every instance with its first s_i boxes
    (test_replan_branches._check_replan's rules; the shapes are the pairs' ids).  Returns the plans
    and first-time flags the oracle's choice implies."""
    plan_x, first, _, _ = before
    nI, Kall = len(out["branch"]), pred.shape[1]
    kp, sc = np.asarray(num_pred), np.clip(np.asarray(scount), 0, S_st)
    stat = [[(static[0][i][j], static[1][i][j], float(static[2][i][j])) for j in range(sc[i])] for i in range(nI)]
    expect, expect_first = plan_x.copy(), first.copy()
    checked = np.zeros(nI, bool)

    def check_qp(vals, got, msg):
        for key, g in zip(("Px", "q", "Ax", "l", "u"), got):
            fin = np.isfinite(vals[key])
            np.testing.assert_array_equal(np.isfinite(g), fin, err_msg=f"{msg} {key}")
            np.testing.assert_allclose(g[fin], vals[key][fin], rtol=1e-13, atol=1e-13, err_msg=f"{msg} {key}")
        return dict(zip(("Px", "q", "Ax", "l", "u"), got))

    for i in range(nI):
        assert out["branch"][i] == ref.branch(first[i], kp[i] > 0, cur_count[i]), i
        assert out["static_count"][i] == (0 if first[i] else sc[i]), i
    for i in out["inst_fanout"]:
        Ki, px = int(kp[i]), plan_x[i]
        assert out["num_obs"][i] == Ki and out["shape"][i] == R.shape_id(Kall, S_st, Ki, sc[i]), i
        fo, qps = ref.fanout_qps(pd, 0, px, pos[i], vel[i], xref[i], dyn_cur[i][:Ki], pred[i][:Ki], pred_size[i][:Ki],
                                 prob[i][:Ki], stat[i])
        assert out["ob_idx"][i] == fo["ob_idx"], i
        np.testing.assert_array_equal(out["cand_type"][i], fo["types"])
        xs, oks = [], []
        for c in range(6):
            k, r = out["cand_rows"][i][c]
            assert k == R.shape_id(Kall, S_st, Ki + (1 if out["cand_slot"][i][c] >= 4 else 0), sc[i]), (i, c, k)
            assert out["shapes"][k]["row_inst"][r] == i
            x, y, info, vals = _row(out, k, r)
            sv = check_qp(qps[c][1], vals, f"instance {i} candidate {c}")
            xo, yo, io = ref.solve(qps[c][0], sv, qps[c][2], s)
            _solution_check(x, y, info, xo, yo, io, np.abs(px).max() >= 1e9)
            xs.append(x)
            oks.append(ref.solve_traj_ok(info))
        best = ref.select(pd, pd, 0, px, xref[i], fo, xs, oks, prob[i][fo["ob_idx"]], stat[i])
        assert out["best_cand"][i] == best, (i, out["best_cand"][i], best)
        if best >= 0:
            expect[i], expect_first[i] = xs[best], 0
        checked[i] = True
    for idx, br in ((out["inst_first"], SINGLE_FIRST), (out["inst_current"], SINGLE_CURRENT)):
        for i in idx:
            cur = br == SINGLE_CURRENT
            ci = int(cur_count[i]) if cur else 0
            pat, vals, ws = ref.single_qp(pd, first[i], plan_x[i], pos[i], vel[i], xref[i],
                                          dyn_cur[i][:ci] if cur else None, cur_size[i][:ci] if cur else None, stat[i])
            k, r = out["single_rows"][i]
            assert k == (Kall + 2 if first[i] else R.shape_id(Kall, S_st, ci, sc[i])), (i, k, ci)
            assert out["shape"][i] == k and out["num_obs"][i] == ci, i
            assert out["shapes"][k]["row_inst"][r] == i
            x, y, info, got_vals = _row(out, k, r)
            sv = check_qp(vals, got_vals, f"instance {i} single ({'current' if cur else 'first'})")
            xo, yo, io = ref.solve(pat, sv, ws, s)
            _solution_check(x, y, info, xo, yo, io, not first[i] and np.abs(plan_x[i]).max() >= 1e9)
            if ref.solve_traj_ok(info):
                expect[i], expect_first[i] = x, 0
            checked[i] = True
    assert checked.all()  # no instance is skipped
    return expect, expect_first


def _row_order(out, nI, K, S_st):
    """Inside every shape: single solves first, then candidates, each in ascending instance order
    (a fan-out instance's four single-intent slots, or its two two-intent slots, in slot order)."""
    for sid, sh in out["shapes"].items():
        inst, code = sh["row_inst"].astype(int), sh["row_code"].astype(int)
        single = code >= 6
        ns = int(single.sum())
        assert single[:ns].all() and not single[ns:].any(), sid
        assert (np.diff(inst[:ns]) > 0).all(), sid
        key = inst[ns:] * 8 + code[ns:]
        assert (np.diff(key) > 0).all(), sid
        assert len(inst) <= R.shape_capacity(nI, K, S_st, sid), sid
        assert sh["pair"] == R.shape_pair(K, S_st, sid)


class _Scene:
    """The fixed-count test's scenario (seed 4646, rng 46) with a count s_i per instance and replan."""

    def __init__(self, Kmax=4, S=3, nI=I, seed=4646, steps=3):
        buckets = scenarios.intent_config(N=N, K=Kmax, instances=nI, hyps=6, seed=seed)
        self.inst = inst = next(iter(buckets.values()))["instances"]
        self.p, self.pd = impc.mpc_params(horizon=N)
        self.pred_size = np.broadcast_to(inst["size"], inst["pred"].shape).copy()
        self.s = impc.default_settings(verbose=0)
        self.L = inst["pred"].shape[3]
        self.K, self.S, self.I, self.steps = Kmax, S, nI, steps
        idx = np.arange(nI)
        rng = np.random.default_rng(46)
        self.first = (idx % 5 == 0).astype(np.int8)
        self.num_pred = [rng.integers(0, Kmax + 1, nI) for _ in range(steps)]
        self.cur_count = rng.integers(0, Kmax + 1, nI).astype(np.int32)
        self.cur_size = np.broadcast_to(inst["size"], (nI, Kmax, 3)).copy()
        self.static = _statics(inst, S, 47, True)
        rs = np.random.default_rng(COUNT_SEED)
        self.scount = [rs.integers(0, S + 1, nI).astype(np.int32) for _ in range(steps)]

    def statics(self, step, poison):
        """the three static arrays, rows >= s_i NaN when poisoned"""
        if not poison:
            return self.static
        cen, size, yaw = (a.copy() for a in self.static)
        past = np.arange(self.S)[None, :] >= self.scount[step][:, None]
        cen[past], size[past], yaw[past] = np.nan, np.nan, np.nan
        return cen, size, yaw

    def chain(self, ctx, poison=False, check=False):
        """The chained replans; returns per replan the results dict and the committed state."""
        inst, K, S = self.inst, self.K, self.S
        rp = DeviceReplan(ctx, self.p, self.pd, self.I, K, self.L, self.s, num_static=S)
        rp.set_state(inst["prev"], self.first)
        pos, vel, pred = inst["pos"].copy(), inst["vel"].copy(), inst["pred"].copy()
        snaps = []
        try:
            for step in range(self.steps):
                before = rp.plans()
                dyn_cur = pred[:, :, 0, 0, :]
                out = rp.run(pos, vel, inst["xref"], dyn_cur=dyn_cur, pred_pos=pred, pred_size=self.pred_size,
                             prob=inst["prob_all"], num_pred=self.num_pred[step], cur_size=self.cur_size,
                             cur_count=self.cur_count, static=self.statics(step, poison),
                             static_count=self.scount[step])
                plans = rp.plans()
                if check:
                    for sid, sh in out["shapes"].items():  # each shape's constraint count
                        k, s_ = R.shape_pair(K, S, sid)
                        assert sh["y"].shape[1] == impc.mpc_dims(self.p, s_, k)[1], (sid, k, s_)
                    _row_order(out, self.I, K, S)
                    expect, expect_first = _check_replan(out, before, pos, vel, inst["xref"], dyn_cur, pred,
                                                         self.pred_size, inst["prob_all"], self.cur_size,
                                                         self.cur_count, self.pd, self.s, self.num_pred[step],
                                                         self.static, self.scount[step], S)
                    np.testing.assert_array_equal(plans[0], expect)  # the committed plans, bitwise
                    np.testing.assert_array_equal(plans[1], expect_first)
                snaps.append(dict(out=out, plans=plans, first_before=before[1]))
                plan_x, valid = plans[0], plans[3]
                pos = np.where(valid[:, None] == 1, plan_x[:, 8:11], pos)
                vel = np.where(valid[:, None] == 1, plan_x[:, 11:14], vel)
                pred = np.concatenate([pred[:, :, :, 1:], pred[:, :, :, -1:]], axis=3)
        finally:
            rp.close()
        return snaps


_CACHE = {}


def _plain_chain(ctx):
    """the unpoisoned chain, run and checked once for the tests that share it"""
    if "plain" not in _CACHE:
        sc = _Scene()
        _CACHE["plain"] = (sc, sc.chain(ctx, check=True))
    return _CACHE["plain"]


@pytest.mark.gpu
def test_counts_three_chained_replans(ctx):
    """K = 4, S_st = 3, s_i drawn per instance and redrawn each replan: every instance against the
    restatement with its own first s_i boxes, and the cases the draws must cover."""
    sc, snaps = _plain_chain(ctx)
    K, S = sc.K, sc.S
    pairs, branches = set(), set()
    first_with_statics = later_without = False
    for step, sn in enumerate(snaps):
        out = sn["out"]
        pairs.update(R.shape_pair(K, S, sid) for sid in out["shapes"] if sid != K + 2)
        branches.update(int(b) for b in out["branch"])
        ft = sn["first_before"] != 0
        first_with_statics |= bool((ft & (sc.scount[step] > 0)).any())
        later_without |= bool((~ft & (sc.scount[step] == 0)).any())
        assert (out["static_count"][ft] == 0).all()
        np.testing.assert_array_equal(out["static_count"][~ft], sc.scount[step][~ft])
    svals = {s_ for _, s_ in pairs}
    assert 0 in svals and S in svals and any(0 < s_ < S for s_ in svals), svals
    assert any(k >= 1 and s_ >= 1 for k, s_ in pairs)  # the isDyamic quirk's region
    assert first_with_statics and later_without
    assert branches == {FANOUT, SINGLE_FIRST, SINGLE_CURRENT}


def _same_bytes(a, b, msg):
    assert a.dtype == b.dtype and a.shape == b.shape, msg
    np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8),
                                  err_msg=msg)


def _same_results(got, want, msg, shapes=True):
    for key in VIEW_KEYS + (("static_count",) if "static_count" in want["out"] else ()):
        _same_bytes(got["out"][key], want["out"][key], f"{msg} {key}")
    for k, (a, b) in enumerate(zip(got["plans"], want["plans"])):
        _same_bytes(a, b, f"{msg} plans[{k}]")
    if shapes:
        assert set(got["out"]["shapes"]) == set(want["out"]["shapes"]), msg
        for sid, sh in want["out"]["shapes"].items():
            for key in ("x", "y", "info", "row_inst", "row_code"):
                _same_bytes(got["out"]["shapes"][sid][key], sh[key], f"{msg} shape {sid} {key}")


@pytest.mark.gpu
def test_rows_past_the_count_are_not_read(ctx):
    """The same chain with rows >= s_i of st_centroid / st_size / st_yaw set to NaN: byte-identical."""
    sc, snaps = _plain_chain(ctx)
    poisoned = sc.chain(ctx, poison=True)
    assert any((sc.scount[k] < sc.S).any() for k in range(sc.steps))
    for step, (a, b) in enumerate(zip(poisoned, snaps)):
        _same_results(a, b, f"replan {step}")


def _packed(ctx, rp, nI):
    buf = DeviceArray(ctx, np.zeros(nI * (64 + 64 * N), np.uint8))
    try:
        rp.pack_device(3, 100, N, nI, buf.ptr)
        ctx.synchronize()
        return buf.get()
    finally:
        buf.free()


@pytest.mark.gpu
def test_fixed_counts_unchanged(ctx):
    """count = S_st for every instance, counts above S_st (clamped), and NULL after a bind give the
    plans, view arrays, per-shape results and packed records of an object that never bound, byte for
    byte; a negative count clamps to 0."""
    sc = _Scene(steps=1)
    inst, K, S = sc.inst, sc.K, sc.S
    first = (np.arange(I) % 5 == 0).astype(np.int8)

    def one(counts, unbind=False):
        rp = DeviceReplan(ctx, sc.p, sc.pd, I, K, sc.L, sc.s, num_static=S)
        cd = None if counts is None else DeviceArray(ctx, np.asarray(counts, np.int32))
        try:
            rp.set_state(inst["prev"], first)
            if cd is not None:
                rp.bind_static_count(cd.ptr)
                if unbind:
                    rp.bind_static_count(None)
            out = rp.run(inst["pos"], inst["vel"], inst["xref"], dyn_cur=inst["pred"][:, :, 0, 0, :],
                         pred_pos=inst["pred"], pred_size=sc.pred_size, prob=inst["prob_all"],
                         num_pred=sc.num_pred[0], cur_size=sc.cur_size, cur_count=sc.cur_count, static=sc.static)
            return dict(out=out, plans=rp.plans(), packed=_packed(ctx, rp, I))
        finally:
            rp.close()
            if cd is not None:
                cd.free()

    base = one(None)
    assert "static_count" not in base["out"] and set(base["out"]["shapes"]) <= set(range(K + 3))
    for name, got in (("count = S_st", one(np.full(I, S))), ("count above S_st", one(np.full(I, S + 5))),
                      ("unbound again", one(np.zeros(I), unbind=True))):
        got["out"].pop("static_count", None)
        _same_results(got, base, name)
        _same_bytes(got["packed"], base["packed"], f"{name} records")
    neg, zero = one(np.full(I, -3)), one(np.zeros(I))
    _same_results(neg, zero, "negative counts clamp to 0")
    assert (zero["out"]["static_count"] == 0).all()
    assert all(R.shape_pair(K, S, sid)[1] == 0 for sid in zero["out"]["shapes"])
    assert not np.array_equal(zero["plans"][0], base["plans"][0])  # the statics of this scene bind


@pytest.mark.gpu
def test_many_shapes(ctx):
    """K = 10, S_st = 8, four instances: 109 shapes.  One replan against the restatement, and the row
    order inside the shapes."""
    Kmax, S, nI = 10, 8, 4
    sc = _Scene(Kmax=Kmax, S=S, nI=nI, seed=4747, steps=1)
    assert R.num_shapes(Kmax, S, True) == 109
    sc.first = np.array([0, 1, 0, 0], np.int8)
    sc.num_pred = [np.array([10, 3, 0, 2])]   # the two-intent candidates of K_i = K: shape (K + 1, s)
    sc.cur_count = np.array([0, 4, 7, 0], np.int32)
    sc.scount = [np.array([5, 2, 0, 8], np.int32)]
    snaps = sc.chain(ctx, check=True)
    out = snaps[0]["out"]
    want = {R.shape_id(Kmax, S, 10, 5), R.shape_id(Kmax, S, 11, 5), Kmax + 2, R.shape_id(Kmax, S, 7, 0), 2, 3}
    assert set(out["shapes"]) == want
    assert out["branch"].tolist() == [FANOUT, SINGLE_FIRST, SINGLE_CURRENT, FANOUT]


@pytest.mark.gpu
def test_bind_argument_errors(ctx):
    """Every error of the bind call, each leaving a working object: after the failed first bind the
    object runs unbound exactly as a fresh one."""
    sc = _Scene(steps=1)
    inst, K = sc.inst, sc.K
    cd = DeviceArray(ctx, np.zeros(I, np.int32))
    bind = impc.lib.impc_replan_bind_static_count
    first = (np.arange(I) % 5 == 0).astype(np.int8)

    def one(rp):
        rp.set_state(inst["prev"], first)
        out = rp.run(inst["pos"], inst["vel"], inst["xref"], dyn_cur=inst["pred"][:, :, 0, 0, :], pred_pos=inst["pred"],
                     pred_size=sc.pred_size, prob=inst["prob_all"], num_pred=sc.num_pred[0], cur_size=sc.cur_size,
                     cur_count=sc.cur_count)
        return dict(out=out, plans=rp.plans())

    try:
        assert bind(None, cd.ptr) == INVALID_ARGUMENT
        fresh = DeviceReplan(ctx, sc.p, sc.pd, I, K, sc.L, sc.s)
        rp = DeviceReplan(ctx, sc.p, sc.pd, I, K, sc.L, sc.s)  # num_static = 0
        try:
            assert bind(rp.h, cd.ptr) == INVALID_ARGUMENT and b"num_static" in impc.lib.impc_last_error()
            assert bind(rp.h, None) == INVALID_ARGUMENT
            with pytest.raises(Exception):
                rp.shape(0, 1)
            _same_results(one(rp), one(fresh), "after a failed bind")
            assert (rp.static_count() == 0).all()
        finally:
            rp.close()
            fresh.close()
        # an object without solver shapes (a horizon beyond the structured kernel): as impc_replan_run
        pb, pdb = impc.mpc_params(horizon=110)
        big = DeviceReplan(ctx, pb, pdb, 2, 2, 110, sc.s, num_static=2)
        try:
            assert bind(big.h, cd.ptr) == UNSUPPORTED and b"structured kernel" in impc.lib.impc_last_error()
            assert bind(big.h, None) == UNSUPPORTED
            b, cnt = C.c_void_p(), C.c_int64()
            assert impc.lib.impc_replan_shape_static(big.h, 0, 0, C.byref(b), C.byref(cnt), *([None] * 7)) == UNSUPPORTED
        finally:
            big.close()
        # the inspection call's own errors
        rp = DeviceReplan(ctx, sc.p, sc.pd, I, K, sc.L, sc.s, num_static=2)
        try:
            args = (C.byref(C.c_void_p()), C.byref(C.c_int64())) + (None,) * 7
            for k, s_ in ((-1, 0), (K + 2, 0), (0, -1), (0, 3)):
                assert impc.lib.impc_replan_shape_static(rp.h, k, s_, *args) == INVALID_ARGUMENT, (k, s_)
            assert impc.lib.impc_replan_shape_static(rp.h, 0, 1, *args) == INVALID_ARGUMENT  # nothing bound yet
            assert impc.lib.impc_replan_shape_static(rp.h, 0, 2, *args) == 0
            assert impc.lib.impc_replan_static_count_device(rp.h, None) == INVALID_ARGUMENT
            rp.bind_static_count(cd.ptr)
            assert impc.lib.impc_replan_shape_static(rp.h, 0, 1, *args) == 0
        finally:
            rp.close()
    finally:
        cd.free()


@pytest.mark.gpu
def test_clustering_chained_into_the_replan(ctx):
    """The device clustering feeding the replan inside the tick (DeviceTick(..., clusters=...)): the
    "main" scene of tests/cluster_cases.py (13 vehicles, max_boxes = S_st = 12, between 0 and 8 boxes
    each), two ticks at the scene's two poses with two tracked obstacles ahead of every vehicle (the
    second beyond the gate's range for every other vehicle).  The clustering's own boxes and counts,
    the gate's K_i and the predictor's trajectories are read back and given to the restatement:
    the comparison of test 1."""
    import cluster_cases as cases
    from impc import clustering as CL
    from impc import perception as P
    from test_cluster_host import c_map, c_params
    g = cases.group("main")
    nI, K, M, H, L = cases.I, 2, 2, 4, N + 1
    S = int(c_params(g["pr"]).max_boxes)
    p, pd = impc.mpc_params(horizon=N)
    s = impc.default_settings(verbose=0)
    ts = pd["ts"]
    rp = DeviceReplan(ctx, p, pd, nI, K, L, s, num_static=S)
    cl = CL.StaticClusters(ctx, c_params(g["pr"]), nI)
    tracks = P.Tracks(ctx, nI, M, H)
    tick = P.DeviceTick(ctx, rp, tracks, P.detect_params(5.0, P.FOV_ALL, (0.4, 0.4, 0.2), K),
                        occ=np.ascontiguousarray(g["occ"]), omap=c_map(g["map"]), clusters=cl, map_max=g["map_max"])
    tmp = []

    def dev(a, dt=np.float64):
        tmp.append(DeviceArray(ctx, np.ascontiguousarray(a, dt)))
        return tmp[-1]

    try:
        cl.set(**{k: v for k, v in cases.initial_state(g).items() if k in CL.StaticClusters.STATE})
        pos0 = g["calls"][0]["cur_pos"]
        # a third of the vehicles on a first plan; the others hold a plan along their reference
        first = (np.arange(nI) % 3 == 0).astype(np.int8)
        step = np.arange(N)[None, :, None] * ts
        prev = np.zeros((nI, N, 8))
        prev[:, :, :3] = pos0[:, None, :] + step * np.array([0.3, 0.25, 0.0])
        prev[:, :, 3:6] = [0.3, 0.25, 0.0]
        rp.set_state(prev, first)
        plan_x, ft = rp.plans()[:2]
        counts, pairs, pushed = [], set(), 0
        for r, call in enumerate(g["calls"]):
            pos, vel = call["cur_pos"], call["cur_vel"]
            xref = np.zeros((nI, N, 8))  # past the blocks on their left, at 0.3 m/s
            xref[:, :, :3] = pos[:, None, :] + step * np.array([0.3, 0.25, 0.0])
            xref[:, :, 3:6] = [0.3, 0.25, 0.0]
            wsize = np.full((nI, M, 3), 0.4)
            wvel = np.broadcast_to([-0.2, 0.05, 0.0], (nI, M, 3)).copy()
            for _ in range(3):  # histCB: three pushes per replan
                wpos = pos0[:, None, :] + np.array([[1.6, -0.7, 0.0], [2.0, 0.9, 0.0]])[None] + wvel * 0.033 * pushed
                wpos[1::2, 1, 0] += 6.0  # out of range
                tracks.push(wpos, wvel, wsize)
                pushed += 1
            pos_d, vel_d, xref_d = dev(pos), dev(vel), dev(xref)
            tick.run_device(pos_d.ptr, vel_d.ptr, xref_d.ptr, cluster_active=dev(call["active"], np.int8).ptr,
                            cluster_first=dev(call["first"], np.int8).ptr)
            ctx.synchronize()
            boxes, gate = cl.get(), tick.gate.get()
            np.testing.assert_array_equal(boxes["count"], g["ref"][r]["count"])  # (test_cluster_gpu's ground)
            out = rp.results()
            expect, expect_first = _check_replan(out, (plan_x, ft, None, None), pos, vel, xref, gate["cur_pos"],
                                                 tick.pred_pos.get(), tick.pred_size.get(), tick.prob.get(), None,
                                                 np.zeros(nI, np.int32), pd, s, gate["num"],
                                                 (boxes["centroid"], boxes["size"], boxes["yaw"]), boxes["count"], S)
            _row_order(out, nI, K, S)
            plan_x, ft = rp.plans()[:2]
            np.testing.assert_array_equal(plan_x, expect)
            np.testing.assert_array_equal(ft, expect_first)
            counts.append(boxes["count"].copy())
            pairs.update(out["shapes"])
        assert len(np.unique(counts[-1])) >= 4 and (np.asarray(counts) < S).all()  # 0, 1, 2 and 8 boxes
        assert len(np.unique(gate["num"])) == 2
        assert any(sid > K + 2 for sid in pairs)
    finally:
        tick.close()
        tracks.close()
        cl.close()
        rp.close()
        for d in tmp:
            d.free()
