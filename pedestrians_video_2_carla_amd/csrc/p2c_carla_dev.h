// p2c_carla_dev.h -- shared by p2c_carla_pose.hip (K30) and p2c_lift.hip (K32): carla_row; by p2c_resample.hip (K37) and p2c_smooth.hip (K39):
// carla_row and row_quat; by p2c_smpl.hip (K35) and p2c_ik.hip (K36): all of it; by p2c_root_motion.hip (K40): row_pose (K30's too) and
// the frame front end.
// The arithmetic of one exported CARLA row (definitions and reference citations: p2c_carla_pose.hip) and the frame front end, rows
// tail and argument checks of the per-frame converters.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/p2c.h"

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

// row (x, y, z, pitch, yaw, roll) -> l[0..2] = (x, y, -z), r[0..8] = Rx(a0) Ry(a1) Rz(a2) row-major, (a0, a1, a2) = rad(-roll, -pitch,
// -yaw): K30's inverse (p2c_carla_pose.hip) and the frame phase of K40 (p2c_root_motion.hip)
__device__ __forceinline__ void row_pose(float x, float y, float z, float pitch, float yaw, float roll, float *l, float *r) {
  float s0, c0, s1, c1, s2, c2;
  sincosf(-roll * kRad, &s0, &c0);
  sincosf(-pitch * kRad, &s1, &c1);
  sincosf(-yaw * kRad, &s2, &c2);
  l[0] = x, l[1] = y, l[2] = -z;
  r[0] = c1 * c2;
  r[1] = -(c1 * s2);
  r[2] = s1;
  r[3] = c0 * s2 + (s0 * s1) * c2;
  r[4] = c0 * c2 - (s0 * s1) * s2;
  r[5] = -(s0 * c1);
  r[6] = s0 * s2 - (c0 * s1) * c2;
  r[7] = s0 * c2 + (c0 * s1) * s2;
  r[8] = c0 * c1;
}

// rows (x, y, z, pitch, yaw, roll) -> unit quaternion (w, x, y, z) of Rx(e0) Ry(e1) Rz(e2)
__device__ __forceinline__ void row_quat(float pitch, float yaw, float roll, float &w, float &x, float &y, float &z) {
  float s0, c0, s1, c1, s2, c2;
  sincosf(-roll * kRad * 0.5f, &s0, &c0);
  sincosf(-pitch * kRad * 0.5f, &s1, &c1);
  sincosf(-yaw * kRad * 0.5f, &s2, &c2);
  const float w1 = c0 * c1, x1 = s0 * c1, y1 = c0 * s1, z1 = s0 * s1;   // qx qy
  w = w1 * c2 - z1 * s2;
  x = x1 * c2 + y1 * s2;
  y = y1 * c2 - x1 * s2;
  z = w1 * s2 + z1 * c2;
}

// ---- a frame per 32-lane group (K35, K36): lanes 0..25 the bones in CARLA_SKELETON (= DFS) order, lane 26 the spare, the rest idle
constexpr int kBones = P2C_JOINTS, kSpare = 26, kTypes = 4;
constexpr int kFrameThreads = 256, kFrameMaxBlocks = 2048;   // 8 workgroups per CU on 256 CUs

struct FrameLane {
  int lane, j, base, jb;           // lane of the wavefront, of the group, the group's first lane, the table row (idle lanes: row 0, unused)
  bool bone, spare;
};
__device__ __forceinline__ FrameLane frame_lane() {
  const int lane = threadIdx.x & 63, j = lane & 31;
  return FrameLane{lane, j, lane & 32, j < kBones ? j : 0, j < kBones, j == kSpare};
}

// the skeleton type of frame n, frames_per_type consecutive frames to an entry; a type outside [0, kTypes) is clamped, never followed
__device__ __forceinline__ int frame_type(const int32_t *skel_type, int64_t n, int32_t frames_per_type) {
  const int64_t clip = frames_per_type == 1 ? n
                       : (n <= 0xffffffffll ? (int64_t)((uint32_t)n / (uint32_t)frames_per_type) : n / frames_per_type);
  const int st = skel_type[clip];
  return st < 0 ? 0 : (st >= kTypes ? kTypes - 1 : st);
}

// row (type * 26 + bone) of the relative reference tables -> q the rotation (row-major), l0..l2 the offset
__device__ __forceinline__ void load_ref(const float *ref_rel_rot, const float *ref_rel_loc, size_t row, float (&q)[9], float &l0,
                                         float &l1, float &l2) {
  const float *pr = ref_rel_rot + row * 9, *pl = ref_rel_loc + row * 3;
#pragma unroll
  for (int i = 0; i < 9; ++i) q[i] = pr[i];
  l0 = pl[0], l1 = pl[1], l2 = pl[2];
}

// The rows tail of frame n: bones by their lanes (the row of the bone's reference offset and relative rotation), the root row by
// the spare lane from world_loc / world_rot. Floats by value: behind a pointer or in a struct they are also written to scratch.
__device__ __forceinline__ void store_rows(float *bones, float *root, const float *world_loc, const float *world_rot, int64_t n,
                                           const FrameLane &L, float x, float y, float z, float r00, float r01, float r02,
                                           float r12, float r22) {
  if (!bones && !root) return;
  const bool is_root = L.spare && root;
  if (is_root) {
    const float *w = world_loc + n * 3, *r = world_rot + n * 9;
    x = w[0], y = w[1], z = w[2];
    r00 = r[0], r01 = r[1], r02 = r[2], r12 = r[5], r22 = r[8];
  }
  float o[6];
  carla_row(x, y, z, r00, r01, r02, r12, r22, o);
  float *dst = nullptr;
  if (L.bone && bones) dst = bones + ((size_t)n * kBones + L.j) * 6;
  if (is_root) dst = root + (size_t)n * 6;
  if (dst) {
#pragma unroll
    for (int i = 0; i < 6; ++i) dst[i] = o[i];
  }
}

// ---- host side: what an entry point of such a converter refuses, in this order, before N == 0 returns without a launch
inline int check_frames_call(int64_t N, int64_t frames_per_type, int32_t max_blocks, bool all_inputs, bool any_output,
                             const float *world_loc, const float *world_rot, const float *root) {
  if (N < 0 || N > ((int64_t)1 << 40) || frames_per_type < 1 || frames_per_type > 0x7fffffff || max_blocks < 0) return P2C_E_SHAPE;
  if (!all_inputs || !any_output) return P2C_E_NULL;
  if ((world_loc == nullptr) != (world_rot == nullptr)) return P2C_E_NULL;      // both or neither
  return root && !world_loc ? P2C_E_NULL : 0;
}

}  // namespace p2c_carla
