// detect_gate.hpp -- fakeDetector::isObstacleInSensorRange (fakeDetector.cpp:482-500) as one
// host / device function, term for term, so the gate kernel (detect.hip) and a CPU harness
// (tests/native/detect_harness.cpp) compile the same statements.
#pragma once
#include <math.h>

namespace impc_detect {

// ob, robot: positions [3]; with_yaw false skips the angle test (fov >= 2 pi: atan2 of a
// non-negative first argument never exceeds pi).  NaN inputs fail the comparisons.
__host__ __device__ inline bool in_sensor_range(const double *ob, const double *robot, bool with_yaw, double yaw,
                                                double fov, double range) {
#pragma clang fp contract(off)
    const double dx = ob[0] - robot[0], dy = ob[1] - robot[1], dz = 0.0;  // diff(2) = 0 (:487)
    const double distance = sqrt(dx * dx + dy * dy + dz * dz);            // diff.norm() (:488)
    if (!(distance <= range)) return false;
    if (!with_yaw) return true;
    const double ax = cos(yaw), ay = sin(yaw), az = 0.0;                  // direction (:490)
    // angleBetweenVectors (utils.h:58-60): atan2(a.cross(b).norm(), a.dot(b))
    const double cx = ay * dz - az * dy, cy = az * dx - ax * dz, cz = ax * dy - ay * dx;
    const double angle = atan2(sqrt(cx * cx + cy * cy + cz * cz), ax * dx + ay * dy + az * dz);
    return angle <= fov / 2;                                              // :493
}

}  // namespace impc_detect
