// cluster.hpp -- the arithmetic of the static-obstacle producer (include/impc_cluster.h), statement
// for statement: the region and lattice of mpcPlanner::staticObstacleClusteringCB (mpcPlanner.cpp:
// 200-247), DBSCAN's neighbour test (clustering/DBSCAN.h:31-33, :91), the 2-means classifier
// (Kmeans.cpp:40-59) and its seeds (obstacleClustering.cpp:138-166), and getOrientation's rotation,
// density and box (:236-271, obstacleClustering.h:40-53).
//
// Everything is a __host__ __device__ function so that the kernel (cluster.hip) and a CPU harness
// (tests/native/cluster_harness.cpp) compile the same arithmetic.  As in plan_exec.hpp:
//   * lattice coordinates are the reference's running sums -- for (ix = xStart; ix <= xEnd; ix +=
//     res) -- never start + k res; the sums also decide where each loop ends;
//   * no statement is contracted into a fused multiply-add (fp contract(off) in every function).
// Eigen evaluates a fixed-size sum of three terms as t0 + (t1 + t2) (Redux.h's unroller halves the
// range); that is the order of norm3 below.  In the rotation and in the half-plane test the third
// term is a product with an exact zero, so either order gives the same value.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/impc_cluster.h"

namespace impc_clu {

constexpr int kAngleCols = 5;  // per angle: angle, cos, sin, cos(-angle), sin(-angle)

// What staticObstacleClusteringCB derives from the vehicle state (:209-228).
struct Region {
    double heading;            // angle_ after the update
    double face[3], org[3];    // faceDirection, pOrigin
    double x0, x1, y0, y1;     // xStart, xEnd, yStart, yEnd
    double fl[4];              // the arguments of the two floors and two ceils (for the tests' margins)
};

__host__ __device__ inline double norm3(double a, double b, double c) {
#pragma clang fp contract(off)
    return sqrt(a * a + (b * b + c * c));
}

__host__ __device__ inline double min4(double a, double b, double c, double d) {  // std::min({..}): first smallest
    double m = a;
    if (b < m) m = b;
    if (c < m) m = c;
    if (d < m) m = d;
    return m;
}
__host__ __device__ inline double max4(double a, double b, double c, double d) {  // std::max({..}): first largest
    double m = a;
    if (m < b) m = b;
    if (m < c) m = c;
    if (m < d) m = d;
    return m;
}

__host__ __device__ inline void region_of(const impc_cluster_params &pr, const double *pos, const double *vel, bool first,
                                          double heading, Region &r) {
#pragma clang fp contract(off)
    const double angle = atan2(vel[1], vel[0]);
    if (norm3(vel[0], vel[1], vel[2]) >= pr.min_speed || first) heading = angle;
    r.heading = heading;
    const double c = cos(heading), s = sin(heading);
    r.face[0] = c, r.face[1] = s, r.face[2] = 0.0;
    const double side[3] = {-s, c, 0.0};
    double p1[3], p2[3], p3[3], p4[3];
    const double reach = pr.region_x + pr.offset;
    for (int k = 0; k < 3; k++) {
        r.org[k] = pos[k] - pr.offset * r.face[k];
        p1[k] = r.org[k] + pr.region_y * side[k];
        p2[k] = r.org[k] - pr.region_y * side[k];
        p3[k] = p1[k] + reach * r.face[k];
        p4[k] = p2[k] + reach * r.face[k];
    }
    r.fl[0] = min4(p1[0], p2[0], p3[0], p4[0]) / pr.cloud_res;
    r.fl[1] = max4(p1[0], p2[0], p3[0], p4[0]) / pr.cloud_res;
    r.fl[2] = min4(p1[1], p2[1], p3[1], p4[1]) / pr.cloud_res;
    r.fl[3] = max4(p1[1], p2[1], p3[1], p4[1]) / pr.cloud_res;
    r.x0 = floor(r.fl[0]) * pr.cloud_res;
    r.x1 = ceil(r.fl[1]) * pr.cloud_res;
    r.y0 = floor(r.fl[2]) * pr.cloud_res;
    r.y1 = ceil(r.fl[3]) * pr.cloud_res;
}

// The values of for (v = start; v <= end; v += step) by successive additions.  Returns their
// number, or cap + 1 when there are more than cap (a sum that the step no longer advances included).
__host__ __device__ inline int axis_table(double start, double end, double step, int cap, double *out) {
#pragma clang fp contract(off)
    int n = 0;
    for (double v = start; v <= end; v += step) {
        if (n == cap || !(v + step > v)) return cap + 1;
        out[n++] = v;
    }
    return n;
}

// (p - pOrigin).dot(faceDirection) (:234); the point is scanned when it is >= 0
__host__ __device__ inline double face_dot(const Region &r, double x, double y, double z) {
#pragma clang fp contract(off)
    return (x - r.org[0]) * r.face[0] + ((y - r.org[1]) * r.face[1] + (z - r.org[2]) * r.face[2]);
}

// occMap::isInMap(pos) (occupancyMap.h:479-488): the closed box
__host__ __device__ inline bool in_map(const impc_occ_map &m, const double *map_max, double x, double y, double z) {
    return x >= m.origin[0] && x <= map_max[0] && y >= m.origin[1] && y <= map_max[1] && z >= m.origin[2] &&
           z <= map_max[2];
}

// occMap::isInflatedOccupied(pos) (occupancyMap.h:257-269, :490-505): outside the voxel grid is occupied
__host__ __device__ inline bool inflated_occupied(const impc_occ_map &m, const uint8_t *occ, double x, double y,
                                                  double z) {
#pragma clang fp contract(off)
    const int ix = (int)floor((x - m.origin[0]) / m.resolution);
    const int iy = (int)floor((y - m.origin[1]) / m.resolution);
    const int iz = (int)floor((z - m.origin[2]) / m.resolution);
    const int32_t *d = m.dims;
    if (ix < 0 || ix >= d[0] || iy < 0 || iy >= d[1] || iz < 0 || iz >= d[2]) return true;
    return occ[((int64_t)ix * d[1] + iy) * d[2] + iz] != 0;
}

__host__ __device__ inline bool in_cloud(const Region &r, const impc_occ_map &m, const double *map_max,
                                         const uint8_t *occ, double x, double y, double z) {
    return face_dot(r, x, y, z) >= 0 && in_map(m, map_max, x, y, z) && inflated_occupied(m, occ, x, y, z);
}

// Point::getDis (DBSCAN.h:31-33)
__host__ __device__ inline double dbscan_dist(const double *a, const double *b) {
#pragma clang fp contract(off)
    return sqrt((a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2]));
}

// Lattice offsets (i, j, k) that cannot be within eps are skipped before any coordinate is read: the
// running sums differ from k res by a few ulps, the bound leaves a relative 1e-6.
__host__ __device__ inline bool stencil_far(int m, double res, double eps) {  // m = i^2 + j^2 + k^2
    const double d2 = (double)m * res * res;
    return d2 > eps * eps * 1.000001 + 1e-12;
}
__host__ __device__ inline bool stencil_skip(int i, int j, int k, double res, double eps) {
    return stencil_far(i * i + j * j + k * k, res, eps);
}
__host__ __device__ inline int stencil_radius(double res, double eps) { return (int)ceil(eps / res) + 1; }

// KMeans::Classify over two centroids (Kmeans.cpp:40-59): min > distance is strict, a tie goes to 0.
// d[0], d[1]: the two distances (for the tests' margin).
__host__ __device__ inline int classify2(const double *p, const double *c0, const double *c1, double *d) {
#pragma clang fp contract(off)
    double a = 0, b = 0;
    for (int k = 0; k < 3; k++) a += (p[k] - c0[k]) * (p[k] - c0[k]);
    for (int k = 0; k < 3; k++) b += (p[k] - c1[k]) * (p[k] - c1[k]);
    d[0] = sqrt(a), d[1] = sqrt(b);
    return d[0] > d[1] ? 1 : 0;
}

// (diff).norm() of runKmeans' seed searches (obstacleClustering.cpp:139-141, :159-161)
__host__ __device__ inline double seed_dist(const double *p, const double *q) {
#pragma clang fp contract(off)
    return norm3(p[0] - q[0], p[1] - q[1], p[2] - q[2]);
}

// (clusterMin + clusterMax) / 2.0 (:124, :218; obstacleClustering.h:51 adds pmax + pmin, which is the same sum)
__host__ __device__ inline double mid(double lo, double hi) {
#pragma clang fp contract(off)
    return (lo + hi) / 2.0;
}

// pNew = rot * (p - centroid) + centroid (:238-243) with rot = [c -s 0; s c 0; 0 0 1].  A zero result
// is +0: min / max then do not depend on the order in which equal zeros of either sign are met.
__host__ __device__ inline void rotate(double c, double s, const double *p, const double *cen, double *out) {
#pragma clang fp contract(off)
    const double d0 = p[0] - cen[0], d1 = p[1] - cen[1], d2 = p[2] - cen[2];
    const double ms = -s;
    out[0] = (c * d0 + (ms * d1 + 0.0 * d2)) + cen[0] + 0.0;
    out[1] = (s * d0 + (c * d1 + 0.0 * d2)) + cen[1] + 0.0;
    out[2] = (0.0 * d0 + (0.0 * d1 + 1.0 * d2)) + cen[2] + 0.0;
}

// density of a rotated box (:268-271)
__host__ __device__ inline double density_of(int n, const double *lo, const double *hi, double res) {
#pragma clang fp contract(off)
    const double ln = (hi[0] - lo[0]) / res + 1, wn = (hi[1] - lo[1]) / res + 1, hn = (hi[2] - lo[2]) / res + 1;
    return (double)n / (ln * wn * hn);
}

// bboxVertex (obstacleClustering.h:50-52) as getStaticObstacles returns it (:309-311): centroid and
// dimension in the ROTATED frame, yaw = -angle
__host__ __device__ inline void box_of(const double *lo, const double *hi, double angle, double *centroid, double *size,
                                       double *yaw) {
#pragma clang fp contract(off)
    for (int k = 0; k < 3; k++) {
        size[k] = hi[k] - lo[k];
        centroid[k] = (hi[k] + lo[k]) / 2.0;
    }
    *yaw = -angle;
}

// The angle table of getOrientation (:236-238, :283), host libm only.
inline void angle_table(int angle_num, double *tab) {
#pragma clang fp contract(off)
    for (int i = 0; i < angle_num; i++) {
        const double angle = M_PI * double(i) / double(angle_num);
        double *t = tab + kAngleCols * i;
        t[0] = angle, t[1] = cos(angle), t[2] = sin(angle), t[3] = cos(-angle), t[4] = sin(-angle);
    }
}

}  // namespace impc_clu
