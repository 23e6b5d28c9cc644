"""What the reference's caller does with a committed plan, on the device: a ctypes mirror of
include/impc_exec.h -- impc_replan_target_device (trajExeCB's tracking target, mpcNavigation.cpp:499-567)
and impc_replan_check_device (mpcHasCollision / hasDynamicCollision, :631-647, :669-703: the "replan
now" decision) over the replan object's own state, stream-ordered on the context stream with nothing
on the host.  Every pointer is a device address (an int, e.g. impc.DeviceArray.ptr) or None.
"""
import ctypes as C

import numpy as np

from . import DeviceArray, OccMap, _check, _P, lib

YAW_FACING, YAW_HOLD, YAW_SMOOTH = 0, 1, 2  # IMPC_YAW_*
FORWARD_DIST = 1.0  # trajExeCB's forwardDist (:538)


class TargetParams(C.Structure):
    """impc_target_params."""
    _fields_ = [("yaw_mode", C.c_int32), ("reserved", C.c_int32), ("forward_dist", C.c_double)]


class TargetIn(C.Structure):
    """impc_target_in."""
    _fields_ = [(k, C.c_void_p) for k in ("t", "ready", "cur_pos", "odom_yaw", "facing_yaw")]


class TargetOut(C.Structure):
    """impc_target_out."""
    _fields_ = [(k, C.c_void_p) for k in ("pos", "vel", "acc", "yaw", "ref", "done", "yaw_step")]


class CheckIn(C.Structure):
    """impc_check_in."""
    _fields_ = [("t", C.c_void_p), ("ready", C.c_void_p), ("cur_pos", C.c_void_p), ("map", OccMap),
                ("occ_inflated", C.c_void_p), ("num_obs", C.c_void_p), ("ob_pos", C.c_void_p), ("ob_size", C.c_void_p)]


class CheckOut(C.Structure):
    """impc_check_out."""
    _fields_ = [(k, C.c_void_p) for k in ("map_step", "dyn_step", "replan")]


lib.impc_replan_target_device.restype = C.c_int
lib.impc_replan_target_device.argtypes = [_P, C.POINTER(TargetParams), C.POINTER(TargetIn), C.POINTER(TargetOut)]
lib.impc_replan_check_device.restype = C.c_int
lib.impc_replan_check_device.argtypes = [_P, C.POINTER(CheckIn), C.POINTER(CheckOut)]


def target_device(replan, yaw_mode, t, cur_pos, odom_yaw, pos, vel, acc, yaw, done, ready=None, facing_yaw=None,
                  ref=None, yaw_step=None, forward_dist=FORWARD_DIST):
    """impc_replan_target_device on `replan` (an impc.replan.DeviceReplan): inputs t [I], cur_pos
    [I][3], odom_yaw [I], ready [I] int8 or None, facing_yaw [I] (IMPC_YAW_FACING); outputs pos, vel,
    acc [I][3], yaw [I], done [I] int8, ref [I][3] or None, yaw_step [I] int32 or None.  Asynchronous."""
    p = TargetParams(yaw_mode=int(yaw_mode), forward_dist=float(forward_dist))
    i = TargetIn(t=t, ready=ready, cur_pos=cur_pos, odom_yaw=odom_yaw, facing_yaw=facing_yaw)
    o = TargetOut(pos=pos, vel=vel, acc=acc, yaw=yaw, ref=ref, done=done, yaw_step=yaw_step)
    _check(lib.impc_replan_target_device(replan.h, C.byref(p), C.byref(i), C.byref(o)), "impc_replan_target_device")


def check_device(replan, t, cur_pos, map_step, dyn_step, replan_flag, ready=None, omap=None, occ=None, num_obs=None,
                 ob_pos=None, ob_size=None):
    """impc_replan_check_device: inputs t [I], cur_pos [I][3], ready or None, the inflated map (omap
    an impc.OccMap, occ its device grid; occ None skips the map test) and the boxes num_obs [I], ob_pos
    / ob_size [I][K][3] (num_obs None skips the dynamic test); outputs map_step, dyn_step [I] int32,
    replan_flag [I] int8.  Asynchronous."""
    i = CheckIn(t=t, ready=ready, cur_pos=cur_pos, occ_inflated=occ, num_obs=num_obs, ob_pos=ob_pos, ob_size=ob_size)
    if omap is not None:
        i.map = omap
    o = CheckOut(map_step=map_step, dyn_step=dyn_step, replan=replan_flag)
    _check(lib.impc_replan_check_device(replan.h, C.byref(i), C.byref(o)), "impc_replan_check_device")


class TargetBuffers:
    """Device arrays for every output of impc_replan_target_device over I instances."""
    SHAPES = dict(pos=(3, np.float64), vel=(3, np.float64), acc=(3, np.float64), yaw=(0, np.float64),
                  ref=(3, np.float64), done=(0, np.int8), yaw_step=(0, np.int32))

    def __init__(self, ctx, I, fill=None):
        self.arrays = {}
        for k, (w, dt) in self.SHAPES.items():
            shape = (I, w) if w else (I,)
            self.arrays[k] = DeviceArray(ctx, shape, dt) if fill is None else DeviceArray(ctx, np.full(shape, fill, dt))

    def ptrs(self):
        return {k: a.ptr for k, a in self.arrays.items()}

    def get(self):
        return {k: a.get() for k, a in self.arrays.items()}

    def free(self):
        for a in self.arrays.values():
            a.free()


class CheckBuffers:
    """Device arrays for every output of impc_replan_check_device over I instances."""

    def __init__(self, ctx, I, fill=None):
        mk = lambda dt: DeviceArray(ctx, (I,), dt) if fill is None else DeviceArray(ctx, np.full(I, fill, dt))  # noqa: E731
        self.arrays = dict(map_step=mk(np.int32), dyn_step=mk(np.int32), replan_flag=mk(np.int8))

    def ptrs(self):
        return {k: a.ptr for k, a in self.arrays.items()}

    def get(self):
        return {k: a.get() for k, a in self.arrays.items()}

    def free(self):
        for a in self.arrays.values():
            a.free()
