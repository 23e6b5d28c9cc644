"""The detector stage in front of the predictor and the replan: a ctypes mirror of
include/impc_detect.h (the device track store of fakeDetector's obstacleHist_ / histCB and the
batched sensor-range gate of getDynamicObstaclesHist / getObstaclesInSensorRange,
fakeDetector.cpp:337-347, :482-556), and DeviceTick, one whole planner tick queued on the context
stream with nothing on the host: gate -> intent probabilities -> predicted trajectories -> replan.
"""
import ctypes as C
import math

import numpy as np

from . import DeviceArray, IntentParams, OccMap, TrajParams, _check, _P, intent_params, lib

INVALID_ARGUMENT = 101  # IMPC_INVALID_ARGUMENT (include/impc_qp.h)
FOV_ALL = 2 * math.pi  # getDynamicObstaclesHist's fov (:533); mpcNavigation passes the same to getObstaclesInSensorRange


class DetectParams(C.Structure):
    """impc_detect_params."""
    _fields_ = [("range", C.c_double), ("fov", C.c_double), ("robot_size", C.c_double * 3), ("max_out", C.c_int32),
                ("reserved", C.c_int32)]


OUT_FIELDS = ("num", "in_range", "src", "hist_len", "pos_hist", "vel_hist", "cur_pos", "cur_vel", "cur_size")


class DetectOut(C.Structure):
    """impc_detect_out: device (gather_device) or host (gather) pointers."""
    _fields_ = [(k, C.c_void_p) for k in OUT_FIELDS]


def _sig(name, *args):
    f = getattr(lib, name)
    f.restype = C.c_int
    f.argtypes = list(args)


_sig("impc_tracks_create", _P, C.c_int64, C.c_int32, C.c_int32, C.POINTER(_P))
_sig("impc_tracks_destroy", _P)
_sig("impc_tracks_push_device", _P, _P, _P, _P, _P)
_sig("impc_tracks_reset", _P)
_sig("impc_detect_gather_device", _P, C.POINTER(DetectParams), C.c_int64, _P, _P, C.POINTER(DetectOut), _P)
_sig("impc_detect_gather", _P, C.POINTER(DetectParams), C.c_int64, _P, _P, C.POINTER(DetectOut))


def detect_params(range_m=30.0, fov=FOV_ALL, robot_size=(0.0, 0.0, 0.0), max_out=4):
    """impc_detect_params (defaults: fake_detector_param.yaml color_distance, the live callers' fov)."""
    p = DetectParams(range=float(range_m), fov=float(fov), max_out=int(max_out))
    p.robot_size[:] = [float(v) for v in robot_size]
    return p


def out_shapes(I, K, H):
    """Shape and dtype of every impc_detect_out array."""
    i32, f64 = np.int32, np.float64
    return dict(num=((I,), i32), in_range=((I,), i32), src=((I, K), i32), hist_len=((I, K), i32),
                pos_hist=((I, K, H, 3), f64), vel_hist=((I, K, H, 3), f64), cur_pos=((I, K, 3), f64),
                cur_vel=((I, K, 3), f64), cur_size=((I, K, 3), f64))


class Tracks:
    """impc_tracks: `worlds` worlds (1, or one per planning instance) of M obstacles with at most H
    history entries each, on the device."""

    def __init__(self, ctx, worlds, M, H):
        self.ctx, self.worlds, self.M, self.H = ctx, int(worlds), int(M), int(H)
        h = _P()
        _check(lib.impc_tracks_create(ctx.h, self.worlds, self.M, self.H, C.byref(h)), "impc_tracks_create")
        self.h = h

    def push_device(self, pos_ptr, vel_ptr, size_ptr, stream=None):
        """histCB: the newest boxes, device arrays [worlds][M][3]; asynchronous."""
        _check(lib.impc_tracks_push_device(self.h, _P(pos_ptr), _P(vel_ptr), _P(size_ptr),
                                           _P(stream) if stream else None), "impc_tracks_push_device")

    def push(self, pos, vel, size):
        """push_device from host arrays (test plumbing; synchronous)."""
        shp = (self.worlds, self.M, 3)
        tmp = [DeviceArray(self.ctx, np.ascontiguousarray(a, np.float64).reshape(shp)) for a in (pos, vel, size)]
        self.push_device(*[d.ptr for d in tmp])
        self.ctx.synchronize()
        for d in tmp:
            d.free()

    def reset(self):
        _check(lib.impc_tracks_reset(self.h), "impc_tracks_reset")

    def close(self):
        # a store is destroyed before its context (include/impc_detect.h); once the context is closed
        # the handle is only dropped -- impc_tracks_destroy would reach into the freed context
        if self.h and self.ctx.h:
            lib.impc_tracks_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GateBuffers:
    """Device arrays for every output of a gather over I instances with K slots (impc_detect_out)."""

    def __init__(self, ctx, I, K, H):
        self.ctx, self.I, self.K, self.H = ctx, int(I), int(K), int(H)
        self.arrays = {k: DeviceArray(ctx, shp, dt) for k, (shp, dt) in out_shapes(self.I, self.K, self.H).items()}
        self.out = DetectOut(**{k: a.ptr for k, a in self.arrays.items()})

    def __getattr__(self, name):  # gate.num, gate.cur_pos, ...: the DeviceArray
        try:
            return self.__dict__["arrays"][name]
        except KeyError:
            raise AttributeError(name) from None

    def get(self):
        """Host copies of every array (synchronises)."""
        return {k: a.get() for k, a in self.arrays.items()}

    def free(self):
        for a in self.arrays.values():
            a.free()


def gather_device(tracks, params, I, robot_pos_ptr, robot_yaw_ptr, out, stream=None):
    """impc_detect_gather_device: `out` a DetectOut of device pointers (GateBuffers.out); asynchronous."""
    _check(lib.impc_detect_gather_device(tracks.h, C.byref(params), int(I), _P(robot_pos_ptr),
                                         _P(robot_yaw_ptr) if robot_yaw_ptr else None, C.byref(out),
                                         _P(stream) if stream else None), "impc_detect_gather_device")


def gather(tracks, params, robot_pos, robot_yaw=None, fields=OUT_FIELDS):
    """impc_detect_gather from host arrays robot_pos [I][3], robot_yaw [I] or None: a dict of the
    output arrays named in `fields` (num always)."""
    rp = np.ascontiguousarray(robot_pos, np.float64).reshape(-1, 3)
    ry = None if robot_yaw is None else np.ascontiguousarray(robot_yaw, np.float64).reshape(rp.shape[0])
    I = rp.shape[0]
    # (a max_out < 1 is the library's to reject: the arrays only have to exist)
    res = {k: np.empty(shp, dt) for k, (shp, dt) in out_shapes(I, max(params.max_out, 1), tracks.H).items()
           if k == "num" or k in fields}
    out = DetectOut(**{k: a.ctypes.data for k, a in res.items()})
    _check(lib.impc_detect_gather(tracks.h, C.byref(params), I, rp.ctypes.data_as(_P),
                                  None if ry is None else ry.ctypes.data_as(_P), C.byref(out)), "impc_detect_gather")
    return res


def traj_params(num_pred, dt=0.1, stop_velocity=0.1, front_angle_deg=10.0, min_turning_time=2.0,
                max_turning_time=3.0, z_score=0.674):
    """impc_traj_params (defaults: the reference's predictor_param.yaml)."""
    return TrajParams(num_pred=int(num_pred), dt=dt, stop_velocity=stop_velocity, front_angle_deg=front_angle_deg,
                      min_turning_time=min_turning_time, max_turning_time=max_turning_time, z_score=z_score)


def occ_map(origin, res, dims):
    om = OccMap()
    om.origin[:] = [float(v) for v in origin]
    om.resolution = float(res)
    om.dims[:] = [int(v) for v in dims]
    return om


class DeviceTick:
    """One planner tick of I vehicles on the device, queued on the context stream without a host
    synchronisation: the range gate over `tracks` (impc_detect_gather_device), then -- the
    use_predictor path, mpcNavigation.cpp:290-322 -- the intent probabilities and predicted
    trajectories of all I * K slots (impc_intent_prob_device, impc_predict_traj_device with
    num_pred = L - 1; empty slots are defined inputs that nothing downstream reads) and the replan
    with num_pred = the gate's K_i.  predictor=False is the use_predictor: false path
    (mpcNavigation.cpp:301-311, :705-716: getObstaclesInSensorRange -> updateDynamicObstacles): the
    replan gets the gate's cur_pos / cur_size / num as dyn_cur / cur_size / cur_count and has_pred all
    zero, its SINGLE_CURRENT branch.  After the plan, target() and check() serve what the caller does
    with it (impc.execution: trajExeCB's tracking target, and mpcHasCollision / hasDynamicCollision
    against the tick's map and the gate's boxes), on the same stream.  Owns the gate's and the
    predictor's output buffers; `replan` is an impc.replan.DeviceReplan with K = params.max_out slots.

    clusters: an impc.clustering.StaticClusters over the same I vehicles with max_boxes = the replan's
    num_static (mpcPlanner::staticObstacleClusteringCB feeding makePlanWithPred's
    obclustering_->getStaticObstacles(), mpcPlanner.cpp:200-247, :594).  The tick then runs the
    clustering on its map before the plan, binds the clustering's count [I] to the replan
    (impc_replan_bind_static_count: each vehicle plans around its own s_i boxes) and hands its
    centroid / size / yaw to the replan in place -- still nothing on the host.  map_max: the map's
    upper corner for the clustering (default origin + dims * resolution)."""

    def __init__(self, ctx, replan, tracks, params, occ=None, omap=None, tp=None, ip=None, predictor=True,
                 clusters=None, map_max=None):
        I, K, L = replan.I, replan.K, replan.L
        if params.max_out != K:
            raise ValueError(f"DeviceTick: max_out {params.max_out} != the replan's num_obstacles {K}")
        self.ctx, self.replan, self.tracks, self.params, self.predictor = ctx, replan, tracks, params, bool(predictor)
        self.I, self.K, self.L, self.H = I, K, L, tracks.H
        self.gate = GateBuffers(ctx, I, K, tracks.H)
        # predictor=False: the replan still requires pred_pos / pred_size / prob (impc_replan_run rejects
        # NULL) and reads none of them with has_pred all zero; they keep their full size so that no kernel
        # of the replan is handed an array shorter than its [I][K][4][L][3] indexing, whatever it gates
        self.pred_pos = DeviceArray(ctx, np.zeros((I, K, 4, L, 3)))
        self.pred_size = DeviceArray(ctx, np.zeros((I, K, 4, L, 3)))
        self.prob = DeviceArray(ctx, np.full((I, K, 4), 0.25))
        self.no_pred = DeviceArray(ctx, np.zeros(I, np.int8))
        self._own_occ = self.omap = self.occ_ptr = self.check_out = None
        if self.predictor and (omap is None or occ is None):
            raise ValueError("DeviceTick: the predictor needs the occupancy map (omap, occ)")
        if omap is not None and occ is not None:  # the predictor's map, and check()'s
            self.omap = omap if isinstance(omap, OccMap) else occ_map(omap["origin"], omap["res"], omap["dims"])
            if isinstance(occ, np.ndarray):
                self._own_occ = DeviceArray(ctx, np.ascontiguousarray(occ, np.uint8).reshape(-1))
                self.occ_ptr = self._own_occ.ptr
            else:
                self.occ_ptr = int(occ)
        if self.predictor:
            self.tp = tp if tp is not None else traj_params(L - 1, dt=replan.pd["ts"])
            if self.tp.num_pred != L - 1:
                raise ValueError("DeviceTick: the predictor's num_pred must be the replan's pred_len - 1")
            self.ip = ip if ip is not None else intent_params()
        self.clusters = clusters
        if clusters is not None:
            if clusters.S != replan.S_st or clusters.I != I:
                raise ValueError(f"DeviceTick: the clustering's max_boxes {clusters.S} / instances {clusters.I} != "
                                 f"the replan's num_static {replan.S_st} / instances {I}")
            if self.omap is None:
                raise ValueError("DeviceTick: the clustering needs the occupancy map (omap, occ)")
            m = self.omap
            self.map_max = [float(v) for v in map_max] if map_max is not None else \
                [m.origin[k] + m.dims[k] * m.resolution for k in range(3)]
            replan.bind_static_count(clusters.arrays["count"].ptr)

    def cluster(self, pos_ptr, vel_ptr, active=None, first=None):
        """The static-obstacle clustering of every vehicle on the tick's map (impc_cluster_run_device)."""
        self.clusters.run_device(pos_ptr, vel_ptr, self.omap, self.map_max, self.occ_ptr, active=active, first=first)

    def gather(self, pos_ptr, yaw_ptr=None):
        gather_device(self.tracks, self.params, self.I, pos_ptr, yaw_ptr, self.gate.out)

    def intent(self):
        g = self.gate
        _check(lib.impc_intent_prob_device(self.ctx.h, C.byref(self.ip), self.I * self.K, self.H, _P(g.hist_len.ptr),
                                           _P(g.pos_hist.ptr), _P(g.vel_hist.ptr), _P(self.prob.ptr), None),
               "impc_intent_prob_device")

    def trajectories(self):
        g = self.gate
        _check(lib.impc_predict_traj_device(self.ctx.h, C.byref(self.tp), C.byref(self.omap), _P(self.occ_ptr),
                                            self.I * self.K, _P(g.cur_pos.ptr), _P(g.cur_vel.ptr),
                                            _P(g.cur_size.ptr), _P(self.pred_pos.ptr), _P(self.pred_size.ptr), None),
               "impc_predict_traj_device")

    def predict(self):
        self.intent()
        self.trajectories()

    def plan(self, pos_ptr, vel_ptr, xref_ptr, **kw):
        g = self.gate
        if self.clusters is not None:  # the clustering's boxes in place; their count is bound
            a = self.clusters.arrays
            kw = dict(kw, st_centroid=a["centroid"].ptr, st_size=a["size"].ptr, st_yaw=a["yaw"].ptr)
        if self.predictor:
            self.replan.run_device(pos_ptr, vel_ptr, xref_ptr, g.cur_pos.ptr, self.pred_pos.ptr, self.pred_size.ptr,
                                   self.prob.ptr, num_pred=g.num.ptr, **kw)
        else:
            self.replan.run_device(pos_ptr, vel_ptr, xref_ptr, g.cur_pos.ptr, self.pred_pos.ptr, self.pred_size.ptr,
                                   self.prob.ptr, has_pred=self.no_pred.ptr, cur_size=g.cur_size.ptr,
                                   cur_count=g.num.ptr, **kw)

    def run_device(self, pos_ptr, vel_ptr, xref_ptr, yaw_ptr=None, cluster_active=None, cluster_first=None, **kw):
        """The whole tick from device addresses: pos / vel [I][3], xref [I][N][8], yaw [I] (only with
        fov < 2 pi); kw: the replan's budget (solver_time_limit, elapsed_s).  With clusters:
        cluster_active / cluster_first [I] int8 device addresses or None (impc_cluster_in)."""
        if self.clusters is not None:
            self.cluster(pos_ptr, vel_ptr, cluster_active, cluster_first)
        self.gather(pos_ptr, yaw_ptr)
        if self.predictor:
            self.predict()
        self.plan(pos_ptr, vel_ptr, xref_ptr, **kw)

    def target(self, yaw_mode, t_ptr, pos_ptr, odom_yaw_ptr, out, ready_ptr=None, facing_yaw_ptr=None,
               forward_dist=1.0):
        """trajExeCB of every vehicle on its committed plan (impc_replan_target_device): t [I]
        (realTime), pos [I][3] (currPos_), odom_yaw [I]; out: the output addresses by name (pos, vel,
        acc, yaw, done, optionally ref, yaw_step -- impc.execution.TargetBuffers.ptrs())."""
        from . import execution as E
        E.target_device(self.replan, yaw_mode, t_ptr, pos_ptr, odom_yaw_ptr, ready=ready_ptr,
                        facing_yaw=facing_yaw_ptr, forward_dist=forward_dist, **out)

    def check(self, t_ptr, pos_ptr, ready_ptr=None):
        """The "replan now" tests of every vehicle (impc_replan_check_device): mpcHasCollision against
        the tick's own map (skipped without one) and hasDynamicCollision against the gate's boxes of
        the last gather (num / cur_pos / cur_size: getObstaclesInSensorRange, mpcNavigation.cpp:705-716).
        t [I] (realTime), pos [I][3] (currPos_).  Returns the tick's impc.execution.CheckBuffers
        (map_step, dyn_step, replan_flag on the device; allocated at the first call)."""
        from . import execution as E
        g = self.gate
        if self.check_out is None:
            self.check_out = E.CheckBuffers(self.ctx, self.I)
        E.check_device(self.replan, t_ptr, pos_ptr, ready=ready_ptr, omap=self.omap, occ=self.occ_ptr,
                       num_obs=g.num.ptr, ob_pos=g.cur_pos.ptr, ob_size=g.cur_size.ptr, **self.check_out.ptrs())
        return self.check_out

    def close(self):
        if self.clusters is not None and self.replan.h:
            self.replan.bind_static_count(None)  # the clustering's count array is its owner's to free
        self.gate.free()
        if self.check_out is not None:
            self.check_out.free()
            self.check_out = None
        for d in (self.pred_pos, self.pred_size, self.prob, self.no_pred, self._own_occ):
            if d is not None:
                d.free()
