"""impc_cluster_run_device (include/impc_cluster.h) on the device against the restatement
tests/cluster_ref.py over the scenes of tests/cluster_cases.py, I = 13 instances per object, two
chained calls each: count, flags, num_points, num_initial, cloud, dbscan_label, centroid, size and yaw
bit for bit, heading within 2 ulp (the device's atan2).  The scenes keep their lattice away from every
floor / ceil / half-plane decision and their 2-means distances apart (tests/test_cluster_host.py), so
an ulp in the device's atan2 / cos / sin or in a reduced sum decides nothing.  Every run is queued
behind the device copies that produce its inputs, without a synchronisation in between."""
import ctypes as C

import numpy as np
import pytest

import cluster_cases as cases
import cluster_ref as ref
import impc
from impc import DeviceArray as D
from impc import clustering as CL
from test_cluster_host import OUTPUTS, c_map, c_params

pytestmark = pytest.mark.gpu
INVALID_ARGUMENT = 101
EXACT = tuple(k for k in OUTPUTS if k != "heading")


def _queued(ctx, host, stream):
    """a device array whose content arrives by a copy queued on `stream` (not waited for)"""
    src, dst = D(ctx, np.ascontiguousarray(host)), D(ctx, np.zeros_like(host))
    row = host.dtype.itemsize * int(np.prod(host.shape[1:], dtype=np.int64))
    impc.copy_rows_device(ctx, dst.ptr, row, src.ptr, row, row, host.shape[0], stream=stream)
    return src, dst


def _compare(got, want, msg):
    for key in EXACT:
        np.testing.assert_array_equal(got[key].view(np.uint8), want[key].view(np.uint8), err_msg=f"{msg} {key}")
    ulps = np.abs(got["heading"] - want["heading"]) / np.spacing(np.abs(want["heading"]))
    assert ulps.max() <= 2, (msg, ulps)


@pytest.mark.parametrize("gname", list(cases.BUILDERS))
def test_device_equals_the_restatement(ctx, gname):
    g = cases.group(gname)
    sc = CL.StaticClusters(ctx, c_params(g["pr"]), cases.I, debug=True)
    own = impc.Stream(ctx) if gname == "quarter" else None  # one group on a caller's stream
    st = own.h if own is not None else None
    tmp = [D(ctx, np.ascontiguousarray(g["occ"]))]
    try:
        sc.set(**cases.initial_state(g))
        for k, call in enumerate(g["calls"]):
            bufs = {key: _queued(ctx, call[key], st) for key in ("cur_pos", "cur_vel", "active", "first")}
            tmp += [b for pair in bufs.values() for b in pair]
            sc.run_device(bufs["cur_pos"][1].ptr, bufs["cur_vel"][1].ptr, c_map(g["map"]), g["map_max"], tmp[0].ptr,
                          active=bufs["active"][1].ptr, first=bufs["first"][1].ptr, stream=st)
            own.synchronize() if own is not None else ctx.synchronize()
            got = sc.get()
            if k == 0:  # the debug outputs before the exact ones fail: where a stage went wrong
                np.testing.assert_array_equal(got["num_points"], g["ref"][k]["num_points"])
                np.testing.assert_array_equal(got["num_initial"], g["ref"][k]["num_initial"])
            _compare(got, g["ref"][k], f"{gname} call {k}")
    finally:
        sc.close()
        for b in tmp:
            b.free()
        if own is not None:
            own.close()


def test_null_flags_mean_all_active_and_none_first(ctx):
    """active = NULL runs every instance, first = NULL takes none as first; the optional outputs may
    be NULL; the host-array twin gives the same state."""
    g = cases.group("main")
    call = g["calls"][0]
    want = cases.initial_state(g)
    ref.run(g["pr"], g["map"], g["map_max"], g["occ"], call["cur_pos"], call["cur_vel"], want)
    sc = CL.StaticClusters(ctx, c_params(g["pr"]), cases.I)
    tmp = [D(ctx, np.ascontiguousarray(a)) for a in (g["occ"], call["cur_pos"], call["cur_vel"])]
    try:
        sc.run_device(tmp[1].ptr, tmp[2].ptr, c_map(g["map"]), g["map_max"], tmp[0].ptr)
        ctx.synchronize()
        got = sc.get()
        for key in CL.StaticClusters.STATE:
            if key != "heading":
                np.testing.assert_array_equal(got[key].view(np.uint8), want[key].view(np.uint8), err_msg=key)
        host = {k: v for k, v in cases.initial_state(g).items() if k in CL.StaticClusters.STATE}
        CL.run_host(ctx, c_params(g["pr"]), c_map(g["map"]), g["map_max"], g["occ"], call["cur_pos"], call["cur_vel"],
                    host)
        for key in CL.StaticClusters.STATE:
            np.testing.assert_array_equal(host[key].view(np.uint8), got[key].view(np.uint8), err_msg=key)
    finally:
        sc.close()
        for b in tmp:
            b.free()


def test_argument_errors_launch_nothing(ctx):
    g = cases.group("main")
    pr = c_params(g["pr"])
    sc = CL.StaticClusters(ctx, pr, cases.I, debug=True)
    sent = {k: np.full(a.shape, 77, a.dtype) for k, a in sc.get().items()}
    sc.set(**sent)
    call = g["calls"][0]
    tmp = [D(ctx, np.ascontiguousarray(a)) for a in (g["occ"], call["cur_pos"], call["cur_vel"])]

    def run(omap=None, null_in=None, null_out=None, handle=None):
        i = CL.ClusterIn(cur_pos=tmp[1].ptr, cur_vel=tmp[2].ptr, occ_inflated=tmp[0].ptr)
        i.map = omap if omap is not None else c_map(g["map"])
        i.map_max[:] = g["map_max"]
        o = CL.ClusterOut(**sc.ptrs())
        if null_in:
            setattr(i, null_in, None)
        if null_out:
            setattr(o, null_out, None)
        return impc.lib.impc_cluster_run_device(sc.h if handle is None else handle[0], C.byref(i), C.byref(o), None)

    try:
        for k in ("cur_pos", "cur_vel", "occ_inflated"):
            assert run(null_in=k) == INVALID_ARGUMENT, k
        for k in CL.StaticClusters.STATE:
            assert run(null_out=k) == INVALID_ARGUMENT, k
        for res, dims in ((0.0, (2, 2, 2)), (-1.0, (2, 2, 2)), (float("nan"), (2, 2, 2)), (1.0, (0, 2, 2)),
                          (1.0, (2, 2, -1))):
            bad = impc.OccMap(resolution=res)
            bad.dims[:] = dims
            assert run(omap=bad) == INVALID_ARGUMENT, (res, dims)
        assert run(handle=(None,)) == INVALID_ARGUMENT
        i, o = CL.ClusterIn(), CL.ClusterOut()
        assert impc.lib.impc_cluster_run_device(sc.h, None, C.byref(o), None) == INVALID_ARGUMENT
        assert impc.lib.impc_cluster_run_device(sc.h, C.byref(i), None, None) == INVALID_ARGUMENT
        assert impc.lib.impc_cluster_run(sc.h, None, C.byref(o)) == INVALID_ARGUMENT
        # create: null arguments, no instance, parameters out of range, per-point state past the LDS
        h = C.c_void_p()
        assert impc.lib.impc_cluster_create(ctx.h, None, 1, C.byref(h)) == INVALID_ARGUMENT
        assert impc.lib.impc_cluster_create(ctx.h, C.byref(pr), 0, C.byref(h)) == INVALID_ARGUMENT
        for over in (dict(cloud_res=0.0), dict(eps=-1.0), dict(angle_num=0), dict(angle_num=65), dict(max_boxes=0),
                     dict(max_points=0), dict(density_thresh=0.0), dict(region_x=5000.0)):
            bad = c_params(dict(g["pr"], **over))
            assert impc.lib.impc_cluster_create(ctx.h, C.byref(bad), 1, C.byref(h)) == INVALID_ARGUMENT, over
        big = c_params(dict(g["pr"], max_points=1 << 16))
        assert impc.lib.impc_cluster_create(ctx.h, C.byref(big), 1, C.byref(h)) == INVALID_ARGUMENT
        assert b"shared memory" in impc.lib.impc_last_error()
        # nothing was launched: the state still holds the sentinel
        ctx.synchronize()
        for k, a in sc.get().items():
            np.testing.assert_array_equal(a, sent[k], err_msg=k)
    finally:
        sc.close()
        for b in tmp:
            b.free()


def test_boxes_feed_a_replan_without_a_copy(ctx):
    """The object's box arrays as the st_centroid / st_size / st_yaw of a replan with num_static =
    max_boxes, queued on the same stream right behind the clustering: the replan (mixed branches, the
    shape of test_replan_branches' statics case) against oracle/replan_ref.py fed the restatement's
    boxes, under that test's own criteria."""
    from impc import scenarios
    from impc.replan import DeviceReplan
    from test_replan_branches import I as RI, N, _check_replan

    Kmax, S = 4, 3
    g = cases.three_boxes(RI)
    call = g["calls"][0]
    want = ref.new_state(RI, g["pr"])
    ref.run(g["pr"], g["map"], g["map_max"], g["occ"], call["cur_pos"], call["cur_vel"], want)
    assert (want["count"] == S).all() and not want["flags"].any()
    static = (want["centroid"], want["size"], want["yaw"])

    buckets = scenarios.intent_config(N=N, K=Kmax, instances=RI, hyps=6, seed=4646)
    inst = next(iter(buckets.values()))["instances"]
    p, pd = impc.mpc_params(horizon=N)
    pred_size = np.broadcast_to(inst["size"], inst["pred"].shape).copy()
    s = impc.default_settings(verbose=0)
    L = inst["pred"].shape[3]
    rng = np.random.default_rng(46)
    first = (np.arange(RI) % 5 == 0).astype(np.int8)
    num_pred = rng.integers(0, Kmax + 1, RI).astype(np.int32)
    cur_count = rng.integers(0, Kmax + 1, RI).astype(np.int32)
    cur_size = np.broadcast_to(inst["size"], (RI, Kmax, 3)).copy()
    dyn_cur = np.ascontiguousarray(inst["pred"][:, :, 0, 0, :])

    sc = CL.StaticClusters(ctx, c_params(g["pr"]), RI)
    rp = DeviceReplan(ctx, p, pd, RI, Kmax, L, s, num_static=S)
    tmp = {k: D(ctx, np.ascontiguousarray(a)) for k, a in dict(
        occ=g["occ"], cpos=call["cur_pos"], cvel=call["cur_vel"], pos=inst["pos"], vel=inst["vel"], xref=inst["xref"],
        dyn_cur=dyn_cur, pred_pos=inst["pred"], pred_size=pred_size, prob=inst["prob_all"], num_pred=num_pred,
        cur_size=cur_size, cur_count=cur_count).items()}
    try:
        rp.set_state(inst["prev"], first)
        before = rp.plans()
        sc.run_device(tmp["cpos"].ptr, tmp["cvel"].ptr, c_map(g["map"]), g["map_max"], tmp["occ"].ptr)
        box = sc.ptrs()
        rp.run_device(tmp["pos"].ptr, tmp["vel"].ptr, tmp["xref"].ptr, tmp["dyn_cur"].ptr, tmp["pred_pos"].ptr,
                      tmp["pred_size"].ptr, tmp["prob"].ptr, cur_size=tmp["cur_size"].ptr,
                      cur_count=tmp["cur_count"].ptr, num_pred=tmp["num_pred"].ptr, st_centroid=box["centroid"],
                      st_size=box["size"], st_yaw=box["yaw"])
        ctx.synchronize()
        got = sc.get()
        for key in ("count", "centroid", "size", "yaw"):
            np.testing.assert_array_equal(got[key].view(np.uint8), want[key].view(np.uint8), err_msg=key)
        out = rp.results(True)
        out["xref"] = inst["xref"]
        expect, expect_first = _check_replan(out, before, inst["pos"], inst["vel"], inst["xref"], dyn_cur, inst["pred"],
                                             pred_size, inst["prob_all"], np.ones(RI, bool), cur_size, cur_count, pd, s,
                                             num_pred=num_pred, static=static)
        plan_x, ft, _, _ = rp.plans()
        np.testing.assert_array_equal(plan_x, expect)
        np.testing.assert_array_equal(ft, expect_first)
        assert len(set(int(b) for b in out["branch"])) == 3  # fan-out, first plan and current-obstacle solves
    finally:
        rp.close()
        sc.close()
        for b in tmp.values():
            b.free()
