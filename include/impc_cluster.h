/*
 * impc_cluster.h -- C-ABI of the reference's static-obstacle producer, batched on the device:
 * mpcPlanner::staticObstacleClusteringCB (trajectory_planner mpcPlanner.cpp:200-247) scans the
 * inflated occupancy map on a lattice in a box ahead of the vehicle and obstacleClustering::run
 * (clustering/obstacleClustering.cpp:14-81) turns the cloud into oriented boxes -- DBSCAN
 * (clustering/DBSCAN.h:56-101), a tree of 2-means splits (obstacleClustering.cpp:129-228,
 * Kmeans.cpp:40-100) and a search over angle_num box orientations (:230-290) -- which
 * getStaticObstacles (:305-315) hands to makePlan / makePlanWithPred (mpcPlanner.cpp:551, :594).
 *
 * The run call is stream-ordered; it neither synchronises nor allocates.  Every array of the device
 * entry point is a DEVICE pointer indexed by planning instance (I = the object's instances).  The
 * output arrays are STATE that the call updates in place: an instance that is inactive, whose cloud
 * is empty (obstacleClustering::run does nothing then) or whose run raises a flag keeps its previous
 * boxes and count.  centroid / size / yaw have the layout of impc_replan_inputs' st_centroid /
 * st_size / st_yaw (include/impc_replan.h) when max_boxes equals the replan's num_static.
 *
 * Lattice coordinates are the reference's running sums (for (ix = xStart; ix <= xEnd; ix += res)),
 * never start + k res, and none of this arithmetic is contracted into fused multiply-adds.
 *
 * What the reference leaves undefined gets a defined result and a flag, the instance keeping its
 * previous boxes and count:
 *   IMPC_CLUSTER_POINTS  the cloud has more than max_points points (or the lattice more cells per
 *                        axis than the region can span: coordinates so large that the step no
 *                        longer advances the sum; num_points is -1 then)
 *   IMPC_CLUSTER_BOXES   more than max_boxes clusters at some level of the tree
 *   IMPC_CLUSTER_EMPTY   a 2-means child came out empty (the reference indexes points[0] of an
 *                        empty vector).  Two distinct seeds always keep a member each, so this is
 *                        the split of a one-point cluster, which has no seed (the reference reads
 *                        an uninitialised fpoint): its density is 1, so only a density_thresh above
 *                        1 ("always split") gets there
 * Within a level, an empty child is reported before the box count is looked at.
 */
#ifndef IMPC_CLUSTER_H
#define IMPC_CLUSTER_H
#include <stdint.h>
#include "impc_qp.h"
#include "impc_predict.h"
#ifdef __cplusplus
extern "C" {
#endif

#define IMPC_CLUSTER_POINTS 1
#define IMPC_CLUSTER_BOXES 2
#define IMPC_CLUSTER_EMPTY 4
#define IMPC_CLUSTER_NOISE (-2) /* DBSCAN_NOISE (DBSCAN.h:17) */

typedef struct {
    double cloud_res;       /* cloudRes_, 0.2 */
    double region_x;        /* regionSizeX_, 5.0 (live 6.0) */
    double region_y;        /* regionSizeY_, 2.0 (live 4.0) */
    double ground_height;   /* groundHeight_, 0.3 (live 0.5) */
    double ceiling_height;  /* ceilingHeight_, 2.0 (live 3.0) */
    double offset;          /* 2.0 (mpcPlanner.cpp:207) */
    double min_speed;       /* 0.3 (:210) */
    double eps;             /* eps_, 0.5 (obstacleClustering.h:72) */
    double density_thresh;  /* densityThresh_, 0.9 (:78); > 0 */
    int32_t min_pts;        /* minPts_, 15 (:73) */
    int32_t tree_level;     /* treeLevel_, 3 (:76) */
    int32_t angle_num;      /* angleDiscreteNum_, 20 (:77); 1 .. 64 */
    int32_t kmeans_iters;   /* kmeansIterNum_, 10 (:80) */
    int32_t max_points;     /* P: capacity of the cloud per instance */
    int32_t max_boxes;      /* S_max: capacity of the box arrays per instance */
} impc_cluster_params;

typedef struct impc_cluster_s *impc_cluster;

/* The reference's defaults above, max_points 4096, max_boxes 16. */
void impc_cluster_default_params(impc_cluster_params *p);

/* Allocates everything the run needs: the per-workgroup workspace (the lattice -> point map) and
 * the table of cos / sin (pi i / angle_num) and cos / sin (-pi i / angle_num), computed on the host
 * with libm (getOrientation's strict density comparison picks between angles whose boxes are often
 * equal up to rounding; only the host's own rotations keep its choice).
 * IMPC_INVALID_ARGUMENT: a null argument, instances < 1, a parameter out of range, or per-point
 * state that does not fit the device's shared memory per workgroup (the message says by how much). */
int impc_cluster_create(impc_ctx ctx, const impc_cluster_params *p, int64_t instances, impc_cluster *out);
int impc_cluster_destroy(impc_cluster c);

typedef struct {
    const int8_t *active;        /* [I] inputTraj_.size() != 0 and stateReceived_ (:203); NULL = all */
    const int8_t *first;         /* [I] firstTime_; NULL = none */
    const double *cur_pos;       /* [I][3] currPos_ */
    const double *cur_vel;       /* [I][3] currVel_ */
    impc_occ_map map;            /* map_manager's grid */
    double map_max[3];           /* mapSizeMax_ (isInMap(pos) is the closed box [origin, map_max]) */
    const uint8_t *occ_inflated; /* [dims[0] dims[1] dims[2]] occupancyInflated_ (nonzero = occupied) */
} impc_cluster_in;

typedef struct {
    double *heading;      /* [I] angle_ */
    int32_t *count;       /* [I] boxes of the instance */
    double *centroid;     /* [I][S_max][3] staticObstacle.centroid */
    double *size;         /* [I][S_max][3] staticObstacle.size */
    double *yaw;          /* [I][S_max] staticObstacle.yaw */
    int32_t *flags;       /* [I] IMPC_CLUSTER_* of an active instance's run, else untouched */
    /* optional (may be NULL), written by every active instance's run: */
    int32_t *num_points;  /* [I] points of the cloud (also when above max_points) */
    int32_t *num_initial; /* [I] DBSCAN clusters (cloud of 1 .. P points) */
    double *cloud;        /* [I][P][3] the first num_points rows (cloud of 1 .. P points) */
    int32_t *dbscan_label; /* [I][P] cluster index or IMPC_CLUSTER_NOISE, likewise */
} impc_cluster_out;

/* staticObstacleClusteringCB + obstacleClustering::run + getStaticObstacles for every active
 * instance; asynchronous on `stream` (NULL = the context's stream).
 * IMPC_INVALID_ARGUMENT (nothing is launched): a null object, in or out; a null cur_pos, cur_vel,
 * occ_inflated, heading, count, centroid, size, yaw or flags; a non-positive map resolution or
 * dimension. */
int impc_cluster_run_device(impc_cluster c, const impc_cluster_in *in, const impc_cluster_out *out, void *stream);

/* Same with HOST arrays in `in` (occ_inflated included) and `out`: copied to the device, run, and
 * copied back; synchronous.  The state arrays are read as well as written. */
int impc_cluster_run(impc_cluster c, const impc_cluster_in *in, const impc_cluster_out *out);

#ifdef __cplusplus
}
#endif
#endif
