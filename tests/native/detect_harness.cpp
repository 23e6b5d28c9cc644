// detect_harness.cpp -- TEST ONLY: the range gate's predicate (csrc/detect_gate.hpp, the
// __host__ __device__ restatement of fakeDetector::isObstacleInSensorRange the kernel k_gate calls)
// compiled for the host, so tests/test_detect.py can compare its decisions with the Python
// restatement on a machine without a GPU.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../intent-mpc_amd/csrc/detect_gate.hpp"

// n tuples: robot [n][3], yaw [n], ob [n][3], fov [n], range [n] -> out [n] (1 = in range).
// with_yaw = 0 evaluates the kernel's robot_yaw == NULL path (distance only).
extern "C" void detect_in_range(int64_t n, const double *robot, const double *yaw, const double *ob,
                                const double *fov, const double *range, int32_t with_yaw, int8_t *out) {
    for (int64_t k = 0; k < n; k++)
        out[k] = impc_detect::in_sensor_range(ob + 3 * k, robot + 3 * k, with_yaw != 0, yaw[k], fov[k], range[k]) ? 1 : 0;
}
