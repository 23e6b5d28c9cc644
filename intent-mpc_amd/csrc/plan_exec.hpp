// plan_exec.hpp -- what mpcNavigation does with a committed plan (include/impc_exec.h): the
// tracking target of trajExeCB (mpcNavigation.cpp:499-567) and the collision tests mpcHasCollision /
// hasDynamicCollision (:631-647, :669-703) over mpcPlanner::getPos / getVel / getAcc / getRef
// (mpcPlanner.cpp:1257-1324) and occMap::isInflatedOccupied (occupancyMap.h:257-269, :490-502).
//
// Everything per instance and per sample is a __host__ __device__ function, statement for
// statement, so the kernels below and a CPU harness (tests/native/exec_harness.cpp) compile the
// same arithmetic.  Two things decide whether the results are the reference's:
//   * sample times are its running sums -- for (tt = start; tt <= end; tt += ts) -- never start +
//     k ts: from 1.0 with ts = 0.1 the sum takes 20 samples to 3.0 where the product takes 21, and
//     from 0.0 its 21st value is 2.0000000000000004 > 2.0;
//   * no statement is contracted into a fused multiply-add (fp contract(off) in every function):
//     s + (e - s) / ts * dt, t - idx * ts, the voxel index and the box bounds round as written.
//
// The kernels run one wavefront per instance: the lanes take consecutive samples of a loop (sample x
// box pairs for the dynamic test), every lane forming its own running sum from the chunk's first
// time, a ballot finds the first sample whose predicate holds, and the sum is carried from chunk to
// chunk, so a loop of any length (N = 110 at ts = 0.02: 101 samples) costs ceil(samples / 64) rounds.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/impc_exec.h"

namespace impc_exec {

// One instance's planner state as the getters read it.
struct Plan {
    const double *x;    // plan_x row: currentStatesSol_ [N][8], then currentControlsSol_ [N - 1][5]
    const double *ref;  // plan_ref row: ref_ [N][3]
    const double *cur;  // currPos_ [3]
    int32_t N;          // horizon
    int32_t count;      // currentStatesSol_.size(): 0 or N
    int32_t ref_count;  // ref_.size(): 0 or N
    double ts;
};

// The getters' common statements (:1262-1271): idx = floor(t / ts); dt = t - idx * ts; idx and
// idx + 1 clamped to the `size` rows; s + (e - s) / ts * dt for the first three entries of a row.
__host__ __device__ inline void interp3(const double *rows, int stride, int size, double ts, double t, double *out) {
#pragma clang fp contract(off)
    int idx = (int)floor(t / ts);
    const double dt = t - idx * ts;
    idx = idx < size - 1 ? idx : size - 1;
    idx = idx > 0 ? idx : 0;
    const int nxt = idx + 1 < size - 1 ? idx + 1 : size - 1;
    const double *s = rows + (int64_t)stride * idx, *e = rows + (int64_t)stride * nxt;
    _Pragma("unroll") for (int c = 0; c < 3; c++) out[c] = s[c] + (e[c] - s[c]) / ts * dt;
}

__host__ __device__ inline void get_pos(const Plan &p, double t, double *out) {  // :1257-1273
    if (p.count <= 0) {
        _Pragma("unroll") for (int c = 0; c < 3; c++) out[c] = p.cur[c];
        return;
    }
    interp3(p.x, 8, p.count, p.ts, t, out);
}

__host__ __device__ inline void get_vel(const Plan &p, double t, double *out) {  // :1275-1290
    if (p.count <= 0) {
        _Pragma("unroll") for (int c = 0; c < 3; c++) out[c] = 0.0;
        return;
    }
    interp3(p.x + 3, 8, p.count, p.ts, t, out);
}

__host__ __device__ inline void get_acc(const Plan &p, double t, double *out) {  // :1292-1307
    if (p.count <= 1) {  // currentControlsSol_ (size() - 1 controls) is empty
        _Pragma("unroll") for (int c = 0; c < 3; c++) out[c] = 0.0;
        return;
    }
    interp3(p.x + 8 * (int64_t)p.N, 5, p.count - 1, p.ts, t, out);
}

__host__ __device__ inline void get_ref(const Plan &p, double t, double *out) {  // :1309-1324
    if (p.ref_count <= 0) {
        _Pragma("unroll") for (int c = 0; c < 3; c++) out[c] = p.cur[c];
        return;
    }
    interp3(p.ref, 3, p.ref_count, p.ts, t, out);
}

// getHorizon() * getTs() (mpcNavigation.cpp:508, :636, :686)
__host__ __device__ inline double end_time(const Plan &p) {
#pragma clang fp contract(off)
    return p.N * p.ts;
}

// occMap::isInflatedOccupied (occupancyMap.h:257-269): posToIndex (:501-505), isInMap (:490-499,
// mapVoxelMin_ = 0), indexToAddress
__host__ __device__ inline bool inflated_occupied(const impc_occ_map &m, const uint8_t *occ, const double *p) {
#pragma clang fp contract(off)
    const int ix = (int)floor((p[0] - m.origin[0]) / m.resolution);
    const int iy = (int)floor((p[1] - m.origin[1]) / m.resolution);
    const int iz = (int)floor((p[2] - m.origin[2]) / m.resolution);
    const int32_t *d = m.dims;
    if (ix < 0 || ix >= d[0] || iy < 0 || iy >= d[1] || iz < 0 || iz >= d[2]) return true;
    return occ[((int64_t)ix * d[1] + iy) * d[2] + iz] != 0;
}

// p inside the closed box ob +- size / 2 (mpcNavigation.cpp:690-696)
__host__ __device__ inline bool in_box(const double *p, const double *ob, const double *size) {
#pragma clang fp contract(off)
    _Pragma("unroll") for (int c = 0; c < 3; c++) {
        const double lower = ob[c] - size[c] / 2, upper = ob[c] + size[c] / 2;
        if (!(p[c] >= lower && p[c] <= upper)) return false;
    }
    return true;
}

// One step of the yaw look-ahead (:543-545): p = getRef(tt); (p - refPos).norm() >= forwardDist.
// dx, dy: atan2's arguments.  (Eigen sums the three squares left to right.)
__host__ __device__ inline bool far_from_ref(const Plan &p, const double *ref_pos, double tt, double forward_dist,
                                             double &dx, double &dy) {
#pragma clang fp contract(off)
    double q[3];
    get_ref(p, tt, q);
    dx = q[0] - ref_pos[0];
    dy = q[1] - ref_pos[1];
    const double dz = q[2] - ref_pos[2];
    return sqrt(dx * dx + dy * dy + dz * dz) >= forward_dist;
}

// The collision loops' window (:635-636, :685-686): startTime = std::min(1.0, realTime), endTime =
// std::min(startTime + span, N ts), span 2.0 (map) or 1.0 (boxes).
__host__ __device__ inline void check_window(const Plan &p, double t, double span, double &start, double &end) {
#pragma clang fp contract(off)
    start = t < 1.0 ? t : 1.0;
    const double a = start + span, b = end_time(p);
    end = b < a ? b : a;
}

// The reference's sample loop: the index of the first sample whose predicate holds, or -1.
template <class Pred>
__host__ __device__ inline int first_sample(double start, double end, double dt, Pred pred) {
#pragma clang fp contract(off)
    int k = 0;
    for (double tt = start; tt <= end; tt += dt, k++) {
        if (pred(k, tt)) return k;
        if (!(tt + dt > tt)) break;  // a time the step no longer advances (|t| >= 2^53 ts): not a realTime
    }
    return -1;
}

struct Target {
    double pos[3], vel[3], acc[3], ref[3];
    double yaw, dx, dy;  // dx, dy: the look-ahead's atan2 arguments (yaw_step >= 0)
    int32_t done, yaw_step;
};

// trajExeCB up to the look-ahead (:508-535, :555-563): everything but IMPC_YAW_SMOOTH's yaw, which is
// preset to the odometry yaw (noYawChange).  Returns true when the look-ahead has to run.
__host__ __device__ inline bool target_head(const Plan &p, double t, int yaw_mode, double odom_yaw, double facing_yaw,
                                            Target &o) {
#pragma clang fp contract(off)
    get_pos(p, t, o.pos);
    get_vel(p, t, o.vel);
    get_acc(p, t, o.acc);
    get_ref(p, t, o.ref);
    o.dx = o.dy = 0.0;
    o.yaw_step = -1;
    o.yaw = odom_yaw;
    const double left = end_time(p) - t;
    o.done = left <= 0.0 ? 1 : 0;
    if (o.done) {
        o.vel[0] = o.vel[1] = o.vel[2] = 0.0;
        o.acc[0] = o.acc[1] = o.acc[2] = 0.0;
        return false;
    }
    if (yaw_mode == IMPC_YAW_FACING) o.yaw = facing_yaw;
    return yaw_mode == IMPC_YAW_SMOOTH;
}

// ---- one instance, one thread: what the harness exports
__host__ __device__ inline void target_serial(const Plan &p, double t, int yaw_mode, double forward_dist, double odom_yaw,
                                              double facing_yaw, Target &o) {
    if (!target_head(p, t, yaw_mode, odom_yaw, facing_yaw, o)) return;
    double dx = 0.0, dy = 0.0;
    const int k = first_sample(t, end_time(p), p.ts,
                               [&](int, double tt) { return far_from_ref(p, o.ref, tt, forward_dist, dx, dy); });
    if (k >= 0) {
        o.yaw = atan2(dy, dx);
        o.dx = dx, o.dy = dy;
        o.yaw_step = k;
    }
}

__host__ __device__ inline int map_step_serial(const Plan &p, double t, const impc_occ_map &m, const uint8_t *occ) {
    double start, end;
    check_window(p, t, 2.0, start, end);
    return first_sample(start, end, p.ts, [&](int, double tt) {
        double q[3];
        get_pos(p, tt, q);
        return inflated_occupied(m, occ, q);
    });
}

__host__ __device__ inline int dyn_step_serial(const Plan &p, double t, int nobs, const double *ob_pos,
                                               const double *ob_size) {
    double start, end;
    check_window(p, t, 1.0, start, end);
    return first_sample(start, end, p.ts, [&](int, double tt) {
        double q[3];
        get_pos(p, tt, q);
        for (int o = 0; o < nobs; o++)
            if (in_box(q, ob_pos + 3 * o, ob_size + 3 * o)) return true;
        return false;
    });
}

#ifndef IMPC_EXEC_HOST_ONLY
// ---- one instance, one wavefront

// first_sample over a wavefront.  Each sample has `per` sub-tests (1 <= per <= 64): a round covers
// 64 / per samples, lane l testing sub-test l % per of the round's sample l / per.  The lane forms its
// sample's time by l / per successive additions to the round's first time, and the next round starts
// from the last sample's time plus dt -- the serial loop's sums exactly.  Times ascend, so the samples
// within the end form a prefix of the round and the lowest lane whose predicate holds belongs to the
// first such sample.  Returns that sample's index or -1, and the lane in *hit_lane; uniform over the
// wavefront, which must call it converged.
template <class Pred>
__device__ inline int wave_first_sample(double start, double end, double dt, int per, Pred pred, int *hit_lane) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, spl = 64 / per, ks = lane / per, sub = lane - ks * per;
    double base = start;
    for (int k0 = 0;; k0 += spl) {
        double tt = base;
        for (int j = 0; j < ks; j++) tt += dt;
        const bool in = ks < spl && tt <= end;
        const bool hit = in && pred(k0 + ks, sub, tt);
        const unsigned long long hits = __ballot(hit), ins = __ballot(in);
        if (hits) {
            const int l = __ffsll((long long)hits) - 1;
            *hit_lane = l;
            return k0 + l / per;
        }
        if (!(ins >> (spl * per - 1) & 1)) return -1;  // the loop ended inside this round
        const double last = __shfl(tt, (spl - 1) * per, 64);
        base = last + dt;
        if (!(base > last)) return -1;  // as first_sample: the step no longer advances the time
    }
}

// the replan object's state, as the kernels read it
struct State {
    int64_t I, n;
    int32_t N, K;
    double ts;
    const double *plan_x, *plan_ref;
    const int32_t *prev_count, *ref_count;
};

__device__ inline Plan plan_of(const State &s, const double *cur_pos, int64_t i) {
    return Plan{s.plan_x + i * s.n, s.plan_ref + i * (int64_t)s.N * 3, cur_pos + 3 * i, s.N,
                s.prev_count[i] > 0 ? s.N : 0, s.ref_count[i] > 0 ? s.N : 0, s.ts};
}

// trajExeCB of every ready instance (impc_replan_target_device)
__global__ __launch_bounds__(64) void k_target(State s, impc_target_params tp, impc_target_in in, impc_target_out out) {
    const int lane = threadIdx.x;
    for (int64_t i = blockIdx.x; i < s.I; i += gridDim.x) {
        if (!(in.ready ? in.ready[i] != 0 : s.prev_count[i] > 0)) continue;
        const Plan p = plan_of(s, in.cur_pos, i);
        const double t = in.t[i];
        Target o;
        const bool look = target_head(p, t, tp.yaw_mode, in.odom_yaw[i],
                                      tp.yaw_mode == IMPC_YAW_FACING ? in.facing_yaw[i] : 0.0, o);
        if (look) {
            const double ref_pos[3] = {o.ref[0], o.ref[1], o.ref[2]};
            double dx = 0.0, dy = 0.0;
            int hl = 0;
            const int k = wave_first_sample(
                t, end_time(p), p.ts, 1,
                [&](int, int, double tt) { return far_from_ref(p, ref_pos, tt, tp.forward_dist, dx, dy); }, &hl);
            if (k >= 0) {
                o.yaw = atan2(__shfl(dy, hl, 64), __shfl(dx, hl, 64));
                o.yaw_step = k;
            }
        }
        if (lane == 0) {  // (constant indices: the target stays in registers)
            const auto put3 = [i](double *dst, const double *v) {
                dst[3 * i] = v[0], dst[3 * i + 1] = v[1], dst[3 * i + 2] = v[2];
            };
            put3(out.pos, o.pos);
            put3(out.vel, o.vel);
            put3(out.acc, o.acc);
            if (out.ref) put3(out.ref, o.ref);
            out.yaw[i] = o.yaw;
            out.done[i] = (int8_t)o.done;
            if (out.yaw_step) out.yaw_step[i] = o.yaw_step;
        }
    }
}

// mpcHasCollision and hasDynamicCollision of every instance (impc_replan_check_device)
__global__ __launch_bounds__(64) void k_check(State s, impc_check_in in, impc_check_out out) {
    const int lane = threadIdx.x;
    for (int64_t i = blockIdx.x; i < s.I; i += gridDim.x) {
        int ms = -1, ds = -1, hl = 0;
        if (in.ready ? in.ready[i] != 0 : s.prev_count[i] > 0) {
            const Plan p = plan_of(s, in.cur_pos, i);
            const double t = in.t[i];
            double start, end;
            if (in.occ_inflated) {
                check_window(p, t, 2.0, start, end);
                ms = wave_first_sample(start, end, p.ts, 1, [&](int, int, double tt) {
                    double q[3];
                    get_pos(p, tt, q);
                    return inflated_occupied(in.map, in.occ_inflated, q);
                }, &hl);
            }
            const int nobs = in.num_obs ? min(max(in.num_obs[i], 0), s.K) : 0;
            if (nobs > 0) {
                check_window(p, t, 1.0, start, end);
                const double *ob = in.ob_pos + i * (int64_t)s.K * 3, *sz = in.ob_size + i * (int64_t)s.K * 3;
                ds = wave_first_sample(start, end, p.ts, nobs, [&](int, int o, double tt) {
                    double q[3];
                    get_pos(p, tt, q);
                    return in_box(q, ob + 3 * o, sz + 3 * o);
                }, &hl);
            }
        }
        if (lane == 0) {
            out.map_step[i] = ms;
            out.dyn_step[i] = ds;
            out.replan[i] = (ms >= 0 || ds >= 0) ? 1 : 0;
        }
    }
}

// ref_ after the commit (mpcPlanner.cpp:639, :657): rows 0..2 of the xref of every instance whose
// replan produced a plan
__global__ void k_commit_ref(int64_t I, int32_t N, const int8_t *__restrict__ valid, const double *__restrict__ xref,
                             double *__restrict__ plan_ref, int32_t *__restrict__ ref_count) {
    const int64_t per = (int64_t)N * 3, total = I * per;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = e / per, r = e - i * per;
        if (!valid[i]) continue;
        plan_ref[e] = xref[(i * N + r / 3) * 8 + r % 3];
        if (r == 0) ref_count[i] = N;
    }
}

// impc_replan_set_ref: ref_.size() of every instance that holds a plan
__global__ void k_ref_count(int64_t I, int32_t N, const int32_t *__restrict__ prev_count,
                            int32_t *__restrict__ ref_count) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < I; i += (int64_t)gridDim.x * blockDim.x)
        ref_count[i] = prev_count[i] > 0 ? N : 0;
}
#endif  // IMPC_EXEC_HOST_ONLY

}  // namespace impc_exec
