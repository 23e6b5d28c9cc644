/*
 * impc_detect.h -- the detector stage in front of the predictor and the replan (libimpc_qp.so),
 * batched over planning instances on the device: the tracking histories of a world of obstacles,
 * the sensor-range gate of every vehicle, and the ordered compaction of the obstacles it keeps
 * into the K obstacle slots of the predictor's and the replan's per-instance inputs.  It is what
 * makes K_i = predPos.size() vary per vehicle and per replan (impc_replan.h num_pred).
 *
 * Replaces (reference onboard_detector/include/onboard_detector/fakeDetector.cpp):
 *   histCB                    :337-347  every 0.033 s (:69) the newest box of every obstacle is
 *                                        pushed to the front of its history obstacleHist_[i]; the
 *                                        oldest entry drops once histSize_ are held (:342-345)
 *   isObstacleInSensorRange   :482-500  diff = pObstacle - pRobot, diff(2) = 0, distance =
 *                                        diff.norm(), direction = (cos yaw, sin yaw, 0), angle =
 *                                        angleBetweenVectors(direction, diff) = atan2(|direction x
 *                                        diff|, direction . diff) (utils.h:58-60); in range when
 *                                        angle <= fov / 2 and distance <= colorDistance_ (:493)
 *   getObstaclesInSensorRange :513-523  the boxes of obstacleMsg_ in range, in index order, their
 *                                        sizes + robotSize (:517-519) -- the no-predictor path
 *                                        (mpcNavigation.cpp:705-716, use_predictor false :301-311)
 *   getDynamicObstaclesHist   :525-556  the obstacles whose NEWEST history entry obstacleHist_[i][0]
 *                                        is in range with fov = 2 pi (:533), in index order, each
 *                                        with its whole history: pos, vel = (Vx, Vy, 0) (:537), size
 *                                        + robotSize (:540) -- the predictor's input
 *                                        (dynamicPredictor.cpp:163-170)
 * Here both getters are one gather over the newest history entries (histCB pushes obstacleMsg_, so
 * after a push the newest entry is the current box).  The yaw-from-quaternion conversion
 * (rpy_from_quaternion, :489) is the caller's: robot_yaw is an input.
 */
#ifndef IMPC_DETECT_H
#define IMPC_DETECT_H
#include <stdint.h>
#include "impc_qp.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- Track store (obstacleHist_): `worlds` worlds of M obstacles each, at most H history entries
 * per obstacle, kept on the device as a ring with a head index (a push writes one entry per
 * obstacle and moves nothing).  worlds is 1 (one world seen by every vehicle) or the number of
 * planning instances (each with its own obstacles).  worlds >= 1, M >= 1, H >= 1. */
typedef struct impc_tracks_s *impc_tracks;

int impc_tracks_create(impc_ctx ctx, int64_t worlds, int32_t M, int32_t H, impc_tracks *out);
/* Waits for the context's stream and frees the store.  A store belongs to its context: destroy it
 * before impc_ctx_destroy (the store is not usable, and must not be destroyed, after it). */
int impc_tracks_destroy(impc_tracks tr);
/* histCB: the newest box of every obstacle to the front of its history.  DEVICE arrays pos, vel,
 * size [worlds][M][3]; the stored velocity is (vel[0], vel[1], 0) (:537).  Once H entries are held
 * the oldest drops.  Asynchronous on `stream` (NULL = the context's stream).  The head index and
 * the entry count live on the host, so pushes, resets and gathers of one store take effect in the
 * order of their calls and their device work must be queued in that order too (one stream, or
 * streams the caller orders). */
int impc_tracks_push_device(impc_tracks tr, const double *pos, const double *vel, const double *size, void *stream);
/* Empties every history (no device work). */
int impc_tracks_reset(impc_tracks tr);

/* ---- Gate and gather */
typedef struct {
    double range;          /* colorDistance_ (fake_detector_param.yaml color_distance: 30.0) */
    double fov;            /* field of view (rad); getDynamicObstaclesHist passes 2 pi */
    double robot_size[3];  /* robotSize added to the sizes (:517-519, :540) */
    int32_t max_out;       /* K >= 1: obstacle slots per instance (the replan's num_obstacles) */
    int32_t reserved;
} impc_detect_params;

/* Outputs of a gather, K = max_out.  All but `num` may be NULL.  Slots s >= num[i] of every array
 * are written on every call: src -1, hist_len 0, everything else 0.0 -- so the predictor may run
 * over all I * K slots with defined inputs (a zero-velocity slot takes its stationary path, a
 * zero-length history yields uniform intent probabilities); nothing downstream reads past K_i. */
typedef struct {
    int32_t *num;        /* [I] min(in-range count, K): the replan's num_pred / cur_count */
    int32_t *in_range;   /* [I] the uncapped in-range count (the reference has no cap; the first K
                            in index order are kept, in_range > K tells the truncation) */
    int32_t *src;        /* [I][K] index of slot s's obstacle in its world */
    int32_t *hist_len;   /* [I][K] history entries held */
    double *pos_hist;    /* [I][K][H][3] entry 0 the newest, entries >= hist_len 0.0 */
    double *vel_hist;    /* [I][K][H][3] (impc_intent_prob_device's input with count = I * K) */
    double *cur_pos;     /* [I][K][3] newest entry: impc_predict_traj_device's pos, the replan's dyn_cur */
    double *cur_vel;     /* [I][K][3] (Vx, Vy, 0) */
    double *cur_size;    /* [I][K][3] newest size + robot_size: the predictor's size, the replan's
                            cur_size on the no-predictor path */
} impc_detect_out;

/*
 * For instance i (world 0, or world i of a store with `worlds` = I), over the obstacles j = 0 ..
 * M - 1 in index order: obstacle j is in range when it has a history entry and its NEWEST entry
 * passes isObstacleInSensorRange (above) from robot_pos[i] / robot_yaw[i]; NaN inputs fail the
 * comparisons (not in range).  The obstacles in range fill the slots in index order.  DEVICE
 * arrays robot_pos [I][3], robot_yaw [I]; `out` holds DEVICE pointers.  With fov >= 2 pi the angle
 * test always holds (atan2 of a non-negative first argument lies in [0, pi]) and robot_yaw may be
 * NULL; otherwise it is required (IMPC_INVALID_ARGUMENT).  I must be `worlds` unless `worlds` is 1.
 * Asynchronous on `stream` (NULL = the context's stream).
 */
int impc_detect_gather_device(impc_tracks tr, const impc_detect_params *p, int64_t I, const double *robot_pos,
                              const double *robot_yaw, const impc_detect_out *out, void *stream);

/* Same with host arrays: robot_pos, robot_yaw and the arrays of `out` on the host (synchronous). */
int impc_detect_gather(impc_tracks tr, const impc_detect_params *p, int64_t I, const double *robot_pos,
                       const double *robot_yaw, const impc_detect_out *out);

#ifdef __cplusplus
}
#endif
#endif
