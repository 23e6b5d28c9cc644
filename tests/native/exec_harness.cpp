// exec_harness.cpp -- TEST ONLY: the per-instance functions of csrc/plan_exec.hpp (the __host__
// __device__ restatement of mpcPlanner's getters, trajExeCB's target and mpcNavigation's two collision
// tests that the kernels k_target / k_check call) compiled for the host, so tests/test_exec_host.py
// can compare them with the Python restatement (tests/exec_ref.py) on a machine without a GPU.
#include <hip/hip_runtime.h>

#include <cstdint>

#define IMPC_EXEC_HOST_ONLY
#include "../../intent-mpc_amd/csrc/plan_exec.hpp"

using namespace impc_exec;

namespace {
Plan plan(int64_t i, int32_t N, double ts, const double *plan_x, const double *plan_ref, const int32_t *count,
          const int32_t *ref_count, const double *cur_pos) {
    return Plan{plan_x + i * (13 * (int64_t)N - 5), plan_ref ? plan_ref + i * (int64_t)N * 3 : nullptr, cur_pos + 3 * i, N,
                count[i] > 0 ? N : 0, (plan_ref && ref_count[i] > 0) ? N : 0, ts};
}
}  // namespace

extern "C" {

// n instances: plan_x [n][13 N - 5], plan_ref [n][N][3], count / ref_count [n] (0 = empty), cur_pos
// [n][3], t [n] -> getPos / getVel / getAcc / getRef(t), each [n][3]
void exec_getters(int64_t n, int32_t N, double ts, const double *plan_x, const double *plan_ref, const int32_t *count,
                  const int32_t *ref_count, const double *cur_pos, const double *t, double *pos, double *vel,
                  double *acc, double *ref) {
    for (int64_t i = 0; i < n; i++) {
        const Plan p = plan(i, N, ts, plan_x, plan_ref, count, ref_count, cur_pos);
        get_pos(p, t[i], pos + 3 * i);
        get_vel(p, t[i], vel + 3 * i);
        get_acc(p, t[i], acc + 3 * i);
        get_ref(p, t[i], ref + 3 * i);
    }
}

// trajExeCB of n ready instances; dxy [n][2]: the look-ahead's atan2 arguments (dx, dy), zero
// when yaw_step is -1
void exec_target(int64_t n, int32_t N, double ts, const double *plan_x, const double *plan_ref, const int32_t *count,
                 const int32_t *ref_count, const double *cur_pos, const double *t, int32_t yaw_mode, double forward_dist,
                 const double *odom_yaw, const double *facing_yaw, double *pos, double *vel, double *acc, double *ref,
                 double *yaw, int8_t *done, int32_t *yaw_step, double *dxy) {
    for (int64_t i = 0; i < n; i++) {
        const Plan p = plan(i, N, ts, plan_x, plan_ref, count, ref_count, cur_pos);
        Target o;
        target_serial(p, t[i], yaw_mode, forward_dist, odom_yaw[i], facing_yaw ? facing_yaw[i] : 0.0, o);
        for (int c = 0; c < 3; c++) {
            pos[3 * i + c] = o.pos[c];
            vel[3 * i + c] = o.vel[c];
            acc[3 * i + c] = o.acc[c];
            ref[3 * i + c] = o.ref[c];
        }
        yaw[i] = o.yaw;
        done[i] = (int8_t)o.done;
        yaw_step[i] = o.yaw_step;
        dxy[2 * i] = o.dx;
        dxy[2 * i + 1] = o.dy;
    }
}

// mpcHasCollision / hasDynamicCollision of n ready instances: occ NULL or num_obs NULL skips a test
// (-1); ob_pos, ob_size [n][K][3]
void exec_check(int64_t n, int32_t N, double ts, const double *plan_x, const int32_t *count, const double *cur_pos,
                const double *t, const impc_occ_map *map, const uint8_t *occ, int32_t K, const int32_t *num_obs,
                const double *ob_pos, const double *ob_size, int32_t *map_step, int32_t *dyn_step) {
    for (int64_t i = 0; i < n; i++) {
        const Plan p = plan(i, N, ts, plan_x, nullptr, count, nullptr, cur_pos);
        map_step[i] = occ ? map_step_serial(p, t[i], *map, occ) : -1;
        const int nobs = num_obs ? (num_obs[i] < 0 ? 0 : num_obs[i] > K ? K : num_obs[i]) : 0;
        dyn_step[i] = nobs > 0 ? dyn_step_serial(p, t[i], nobs, ob_pos + i * (int64_t)K * 3, ob_size + i * (int64_t)K * 3) : -1;
    }
}

// the number of samples of for (tt = start; tt <= end; tt += dt), and the last one taken
int32_t exec_sample_count(double start, double end, double dt, double *last) {
    int32_t count = 0;
    first_sample(start, end, dt, [&](int, double tt) {
        count++;
        *last = tt;
        return false;
    });
    return count;
}

int exec_inflated_occupied(const impc_occ_map *map, const uint8_t *occ, const double *p) {
    return inflated_occupied(*map, occ, p) ? 1 : 0;
}

}  // extern "C"
