// p2c_carla_dev.h -- the arithmetic of one exported CARLA row (shared by p2c_carla_pose.hip, K30, and p2c_lift.hip, K32).
// See p2c_carla_pose.hip for the definitions and the reference citations.
#pragma once
#include <hip/hip_runtime.h>

namespace p2c_carla {

constexpr float kDeg = 57.29577951308232f, kRad = 0.017453292519943295f;

__device__ __forceinline__ float clamp_unit(float v) {            // comparisons, not fminf / fmaxf: a NaN stays a NaN
  return v > 1.0f ? 1.0f : (v < -1.0f ? -1.0f : v);
}

// (x, y, z) and the five entries of R the 'XYZ' Euler angles read -> o[0..5] = (x, y, -z, pitch, yaw, roll)
__device__ __forceinline__ void carla_row(float x, float y, float z, float r00, float r01, float r02, float r12, float r22,
                                          float *o) {
  const float e1 = asinf(clamp_unit(r02));
  const float e0 = atan2f(-r12, r22);
  const float e2 = atan2f(-r01, r00);
  o[0] = x, o[1] = y, o[2] = -z;
  o[3] = -(e1 * kDeg), o[4] = -(e2 * kDeg), o[5] = -(e0 * kDeg);
}

}  // namespace p2c_carla
