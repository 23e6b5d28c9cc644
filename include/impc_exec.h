/*
 * impc_exec.h -- C-ABI of what the reference's caller does with a committed plan, batched on the
 * device: the tracking target of trajExeCB (autonomous_flight mpcNavigation.cpp:499-567, 100 Hz)
 * and the "replan now" tests mpcHasCollision / hasDynamicCollision (:631-647, :669-703; called by
 * replanCheckCB :414-422, :474-479 and mpcCB :346, :355).  Both read the plan through
 * mpcPlanner::getPos / getVel / getAcc / getRef (trajectory_planner mpcPlanner.cpp:1257-1324) of
 * the replan object's own state (include/impc_replan.h): plan_x (currentStatesSol_ then
 * currentControlsSol_), prev_count (currentStatesSol_.size()), plan_ref / ref_count (ref_).
 *
 * Both entry points are stream-ordered on the replan's context stream, after whatever the replan
 * queued; neither synchronises nor allocates.  Every array is a DEVICE pointer, indexed by planning
 * instance (I = the replan's instances, N = its horizon, ts = its mpc.ts).
 *
 * An instance takes part when it is ready -- ready[i] != 0 (mpcTrajectoryReady_), or with ready =
 * NULL when it holds a plan (prev_count[i] > 0).  A ready instance without a plan is served as the
 * reference serves it: getPos and getRef return cur_pos (currPos_), getVel and getAcc zero.
 *
 * t [I] is realTime, (now - trajStartTime_).toSec() per instance: finite, >= 0 and below 2^31 ts.
 * It lives on the device and cannot be validated without a synchronisation: the caller keeps it in
 * that range.  (Every loop is finite whatever t holds -- a time the step no longer advances ends it --
 * and every array index is clamped, but the results of such a t are not the reference's.)
 *
 * Sample times are the reference's running sums (for (tt = start; tt <= end; tt += ts)), not
 * start + k ts, and none of this arithmetic is contracted into fused multiply-adds: positions,
 * voxel indices, box comparisons and sample counts are those of the reference built for a target
 * without FMA contraction.
 */
#ifndef IMPC_EXEC_H
#define IMPC_EXEC_H
#include <stdint.h>
#include "impc_replan.h"
#include "impc_predict.h"
#ifdef __cplusplus
extern "C" {
#endif

#define IMPC_YAW_FACING 0 /* useYawControl_ false: yaw = facing_yaw[i] (facingYaw_, :530-532) */
#define IMPC_YAW_HOLD 1   /* noYawTurning_: yaw = odom_yaw[i] (:533-535) */
#define IMPC_YAW_SMOOTH 2 /* the look-ahead over the reference (:536-554) */

typedef struct {
    int32_t yaw_mode;    /* IMPC_YAW_* */
    int32_t reserved;
    double forward_dist; /* forwardDist, 1.0 (:538) */
} impc_target_params;

typedef struct {
    const double *t;          /* [I] realTime */
    const int8_t *ready;      /* [I] mpcTrajectoryReady_; NULL = prev_count > 0 */
    const double *cur_pos;    /* [I][3] currPos_ */
    const double *odom_yaw;   /* [I] rpy_from_quaternion(odom_.pose.pose.orientation) */
    const double *facing_yaw; /* [I] facingYaw_; required with IMPC_YAW_FACING only */
} impc_target_in;

typedef struct {
    double *pos, *vel, *acc; /* [I][3] Target position / velocity / acceleration */
    double *yaw;             /* [I] Target yaw */
    double *ref;             /* [I][3] refPos = getRef(realTime); may be NULL */
    int8_t *done;            /* [I] 1 when leftTime = N ts - realTime <= 0 (:516), else 0 */
    int32_t *yaw_step;       /* [I] IMPC_YAW_SMOOTH: the look-ahead sample (0 = realTime) whose
                                reference point gave the yaw, -1 when none did (noYawChange) or the
                                yaw did not come from the look-ahead; may be NULL */
} impc_target_out;

/* trajExeCB for every ready instance (others keep every output untouched), statement by statement:
 * endTime = N ts (getHorizon() * getTs(), :508 -- the horizon, not the last state's time);
 * pos / vel / acc / refPos = getPos / getVel / getAcc / getRef(realTime) (:509-512; getAcc over the
 * N - 1 controls); with leftTime <= 0 the target is pos, zero velocity and acceleration and the
 * odometry yaw (:516-527); otherwise the yaw of yaw_mode -- the look-ahead is for (tt = realTime; tt
 * <= endTime; tt += ts): the first getRef(tt) at least forward_dist from refPos gives atan2(dy, dx),
 * none gives the odometry yaw (:538-553) -- with pos, vel, acc (:555-563).
 * IMPC_INVALID_ARGUMENT (nothing is launched): a null object, params, in or out; a null t, cur_pos,
 * odom_yaw, pos, vel, acc, yaw or done; yaw_mode out of range; IMPC_YAW_FACING without facing_yaw;
 * an object that has neither been given a state (impc_replan_set_state) nor run. */
int impc_replan_target_device(impc_replan rp, const impc_target_params *p, const impc_target_in *in,
                              const impc_target_out *out);

typedef struct {
    const double *t;             /* [I] realTime */
    const int8_t *ready;         /* [I]; NULL = prev_count > 0 */
    const double *cur_pos;       /* [I][3] currPos_ */
    impc_occ_map map;            /* map_manager's grid (include/impc_predict.h) */
    const uint8_t *occ_inflated; /* [dims[0] dims[1] dims[2]] occupancyInflated_ (nonzero =
                                    occupied); NULL skips the map test (map is not read) */
    const int32_t *num_obs;      /* [I] boxes of the instance, clamped to 0 .. K; NULL skips the
                                    dynamic test */
    const double *ob_pos;        /* [I][K][3] box centres, K = the replan's num_obstacles */
    const double *ob_size;       /* [I][K][3] box sizes: the range gate's num / cur_pos / cur_size are
                                    getObstaclesInSensorRange(2 pi, robotSize) (:705-716) */
} impc_check_in;

typedef struct {
    int32_t *map_step; /* [I] index of the first colliding sample of mpcHasCollision's loop, or -1 */
    int32_t *dyn_step; /* [I] the same for hasDynamicCollision's loop */
    int8_t *replan;    /* [I] map_step >= 0 || dyn_step >= 0 */
} impc_check_out;

/* mpcHasCollision and hasDynamicCollision for every instance: startTime = min(1.0, realTime);
 * samples for (tt = startTime; tt <= endTime; tt += ts) at p = getPos(tt), with endTime =
 * min(startTime + 2.0, N ts) for the map test -- isInflatedOccupied(p): voxel floor((p - origin) /
 * resolution), outside the grid occupied, address (x dims[1] + y) dims[2] + z (occupancyMap.h:257-269,
 * :490-502) -- and min(startTime + 1.0, N ts) for the dynamic test -- p inside the closed box ob +-
 * size / 2 on all three axes, for any of the instance's boxes (:689-698).  A skipped test reports
 * -1; an instance that is not ready gets (-1, -1, 0).
 * IMPC_INVALID_ARGUMENT (nothing is launched): a null object, in or out; a null t, cur_pos,
 * map_step, dyn_step or replan; num_obs without ob_pos and ob_size; occ_inflated with a non-positive
 * resolution or dimension; an object that has neither been given a state nor run. */
int impc_replan_check_device(impc_replan rp, const impc_check_in *in, const impc_check_out *out);

#ifdef __cplusplus
}
#endif
#endif
