"""The reference's static-obstacle producer on the device: a ctypes mirror of include/impc_cluster.h
-- impc_cluster_run_device (mpcPlanner::staticObstacleClusteringCB, mpcPlanner.cpp:200-247, over
obstacleClustering::run and getStaticObstacles, clustering/obstacleClustering.cpp:14-81, :305-315),
stream-ordered with nothing on the host.  Every pointer is a device address (an int, e.g.
impc.DeviceArray.ptr) or None.  StaticClusters holds the state arrays the call updates in place; its
centroid / size / yaw are what impc_replan_inputs' st_centroid / st_size / st_yaw take when max_boxes
equals the replan's num_static.
"""
import ctypes as C

import numpy as np

from . import DeviceArray, OccMap, _check, _P, lib

FLAG_POINTS, FLAG_BOXES, FLAG_EMPTY = 1, 2, 4  # IMPC_CLUSTER_*
NOISE = -2  # IMPC_CLUSTER_NOISE

# autonomous_flight cfg/mpc_navigation/planner_param.yaml:41-45 (the header's comments carry the class defaults)
LIVE_PARAMS = dict(cloud_res=0.2, region_x=6.0, region_y=4.0, ground_height=0.5, ceiling_height=3.0)


class ClusterParams(C.Structure):
    """impc_cluster_params."""
    _fields_ = [(k, C.c_double) for k in ("cloud_res", "region_x", "region_y", "ground_height", "ceiling_height",
                                          "offset", "min_speed", "eps", "density_thresh")] + \
               [(k, C.c_int32) for k in ("min_pts", "tree_level", "angle_num", "kmeans_iters", "max_points",
                                         "max_boxes")]


class ClusterIn(C.Structure):
    """impc_cluster_in."""
    _fields_ = [("active", C.c_void_p), ("first", C.c_void_p), ("cur_pos", C.c_void_p), ("cur_vel", C.c_void_p),
                ("map", OccMap), ("map_max", C.c_double * 3), ("occ_inflated", C.c_void_p)]


class ClusterOut(C.Structure):
    """impc_cluster_out."""
    _fields_ = [(k, C.c_void_p) for k in ("heading", "count", "centroid", "size", "yaw", "flags", "num_points",
                                          "num_initial", "cloud", "dbscan_label")]


lib.impc_cluster_default_params.restype = None
lib.impc_cluster_default_params.argtypes = [C.POINTER(ClusterParams)]
lib.impc_cluster_create.restype = C.c_int
lib.impc_cluster_create.argtypes = [_P, C.POINTER(ClusterParams), C.c_int64, C.POINTER(_P)]
lib.impc_cluster_destroy.restype = C.c_int
lib.impc_cluster_destroy.argtypes = [_P]
lib.impc_cluster_run_device.restype = C.c_int
lib.impc_cluster_run_device.argtypes = [_P, C.POINTER(ClusterIn), C.POINTER(ClusterOut), _P]
lib.impc_cluster_run.restype = C.c_int
lib.impc_cluster_run.argtypes = [_P, C.POINTER(ClusterIn), C.POINTER(ClusterOut)]


def cluster_params(**kw):
    """The reference's defaults (impc_cluster_default_params) with fields replaced."""
    p = ClusterParams()
    lib.impc_cluster_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


class StaticClusters:
    """impc_cluster_create over I instances with the state arrays heading [I], count [I] int32,
    centroid / size [I][S][3], yaw [I][S], flags [I] int32 on the device (zero to begin with); with
    debug=True also num_points, num_initial [I] int32, cloud [I][P][3] and dbscan_label [I][P] int32
    (debug may also name the ones wanted)."""
    STATE = ("heading", "count", "centroid", "size", "yaw", "flags")
    DEBUG = ("num_points", "num_initial", "cloud", "dbscan_label")

    def __init__(self, ctx, params, instances, debug=False):
        self.ctx, self.params, self.I = ctx, params, int(instances)
        self.P, self.S = int(params.max_points), int(params.max_boxes)
        h = _P()
        _check(lib.impc_cluster_create(ctx.h, C.byref(params), self.I, C.byref(h)), "impc_cluster_create")
        self.h = h
        I, P, S = self.I, self.P, self.S
        shapes = dict(heading=((I,), np.float64), count=((I,), np.int32), centroid=((I, S, 3), np.float64),
                      size=((I, S, 3), np.float64), yaw=((I, S), np.float64), flags=((I,), np.int32))
        extra = dict(num_points=((I,), np.int32), num_initial=((I,), np.int32), cloud=((I, P, 3), np.float64),
                     dbscan_label=((I, P), np.int32))
        shapes.update({k: extra[k] for k in (self.DEBUG if debug is True else debug or ())})
        self.arrays = {k: DeviceArray(ctx, np.zeros(s, dt)) for k, (s, dt) in shapes.items()}

    def run_device(self, cur_pos, cur_vel, omap, map_max, occ, active=None, first=None, stream=None):
        """impc_cluster_run_device: cur_pos / cur_vel [I][3], active / first [I] int8 or None, omap an
        impc.OccMap with map_max its upper corner and occ its device grid.  Asynchronous on `stream`
        (a raw stream handle; None = the context's)."""
        i = ClusterIn(active=active, first=first, cur_pos=cur_pos, cur_vel=cur_vel, occ_inflated=occ)
        i.map = omap
        i.map_max[:] = [float(v) for v in map_max]
        o = ClusterOut(**{k: a.ptr for k, a in self.arrays.items()})
        _check(lib.impc_cluster_run_device(self.h, C.byref(i), C.byref(o), _P(stream) if stream else None),
               "impc_cluster_run_device")

    def ptrs(self):
        return {k: a.ptr for k, a in self.arrays.items()}

    def get(self):
        return {k: a.get() for k, a in self.arrays.items()}

    def set(self, **state):
        for k, v in state.items():
            self.arrays[k].set(v)

    def close(self):
        if self.h:
            lib.impc_cluster_destroy(self.h)
            self.h = None
            for a in self.arrays.values():
                a.free()


def run_host(ctx, params, omap, map_max, occ, cur_pos, cur_vel, state, active=None, first=None, debug=False):
    """impc_cluster_run over numpy arrays: `state` maps StaticClusters.STATE names to arrays that are
    updated in place (debug adds the DEBUG arrays, created here).  Returns state."""
    I = cur_pos.shape[0]
    h = _P()
    _check(lib.impc_cluster_create(ctx.h, C.byref(params), I, C.byref(h)), "impc_cluster_create")
    try:
        if debug:
            P = params.max_points
            state.setdefault("num_points", np.zeros(I, np.int32))
            state.setdefault("num_initial", np.zeros(I, np.int32))
            state.setdefault("cloud", np.zeros((I, P, 3)))
            state.setdefault("dbscan_label", np.zeros((I, P), np.int32))
        keep = [np.ascontiguousarray(a) for a in (cur_pos, cur_vel, occ)]
        ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        i = ClusterIn(active=ptr(active), first=ptr(first), cur_pos=ptr(keep[0]), cur_vel=ptr(keep[1]),
                      occ_inflated=ptr(keep[2]))
        i.map = omap
        i.map_max[:] = [float(v) for v in map_max]
        o = ClusterOut(**{k: ptr(a) for k, a in state.items()})
        _check(lib.impc_cluster_run(h, C.byref(i), C.byref(o)), "impc_cluster_run")
    finally:
        lib.impc_cluster_destroy(h)
    return state
