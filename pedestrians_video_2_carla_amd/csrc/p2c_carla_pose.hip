// p2c_carla_pose.hip -- K30: predicted poses <-> CARLA bone transforms, one launch each way (gfx950).
//
// Reference: walker_control/p3d_pose.py:56-96 (tensors_to_pose), :34-54 (pose_to_tensors) and the root conversion of
// renderers/carla_renderer.py:165-183, which run per frame on the host behind a .cpu().numpy() each. Here a whole batch of
// (frame, bone) elements -- and, in the same launch, the per-frame root rows -- is converted on the device.
//
// Forward, per element: (x, y, z), R (3x3, row-major)  ->  (x, y, -z, pitch, yaw, roll) with
//   e = matrix_to_euler_angles(R, 'XYZ'):  e1 = asin(clamp(R[0,2])), e0 = atan2(-R[1,2], R[2,2]), e2 = atan2(-R[0,1], R[0,0]),
//   pitch = -deg(e1), yaw = -deg(e2), roll = -deg(e0).
//   The clamp to [-1, 1] keeps an orthonormalised fp32 matrix whose R[0,2] lands one ulp outside the range at +-90 degrees
//   (pytorch3d returns NaN there); it is written with comparisons, which let a NaN through.
// Inverse, per element: (x, y, z, pitch, yaw, roll)  ->  (x, y, -z), R = Rx(a0) Ry(a1) Rz(a2) with (a0, a1, a2) =
//   rad(-roll, -pitch, -yaw): the closed form of the product euler_xyz_to_matrix (data/carla/reference.py) forms.
// No masking: a NaN operand reaches exactly the outputs computed from it. Only R[0,0], R[0,1], R[0,2], R[1,2], R[2,2] enter the
// forward conversion; the other four entries of a row are not read.
//
// Mapping. One lane per element; element e < N J is bone row e, element N J + n is root row n (forward, world inputs given).
// A lane reads its own 12- and 36-byte rows (4-byte aligned: 36 = 4 * 9): the 64 lanes of a wavefront cover one contiguous span
// of 768 / 2304 bytes, so every 128-byte line that is fetched is used whole, by the neighbouring lanes of the same wavefront, and
// comes from HBM once; a lane's loads are independent and all in flight before the first transcendental. A cooperative copy through LDS would make each instruction fully coalesced, but it
// costs a barrier and a bank-conflicted 9-dword-stride read for a kernel whose whole working set at B = 256, T = 16 is 8.0 MB:
// the lane-per-row form has no LDS, no barrier and no cross-lane traffic. The 24-byte output rows are written by their lane in
// the same way (gfx950 takes multi-dword vector accesses at 4-byte alignment: the compiler merges a row's neighbouring dwords).
// The grid is capped at kMaxBlocks workgroups of 256 lanes (max_blocks lowers the cap); lanes stride over the elements beyond it.
// Every output element is written by exactly one lane and nothing is reduced: the result is fixed by the inputs.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/p2c.h"
#include "p2c_host.h"

#include "p2c_carla_dev.h"   // kDeg, kRad, clamp_unit, carla_row: shared with K32 (p2c_lift.hip); row_pose: with K40 (p2c_root_motion.hip)

namespace p2c_carla {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;   // 8 workgroups per CU on 256 CUs

struct FwdArgs {
  const float *rel_loc, *rel_rot, *world_loc, *world_rot;
  float *bones, *root;
  int64_t n_bones, n_total;        // N J, and N J + N when the root rows are converted too
};

struct InvArgs {
  const float *bones;
  float *loc, *rot;
  int64_t n_bones;
};

__global__ __launch_bounds__(kThreads) void carla_pose_fwd_kernel(FwdArgs a) {
  const int64_t step = (int64_t)gridDim.x * kThreads;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < a.n_total; e += step) {
    const bool is_root = e >= a.n_bones;
    const int64_t row = is_root ? e - a.n_bones : e;
    const float *p = (is_root ? a.world_loc : a.rel_loc) + row * 3;
    const float *r = (is_root ? a.world_rot : a.rel_rot) + row * 9;
    const float x = p[0], y = p[1], z = p[2];
    const float r00 = r[0], r01 = r[1], r02 = r[2], r12 = r[5], r22 = r[8];
    carla_row(x, y, z, r00, r01, r02, r12, r22, (is_root ? a.root : a.bones) + row * 6);
  }
}

__global__ __launch_bounds__(kThreads) void carla_pose_inv_kernel(InvArgs a) {
  const int64_t step = (int64_t)gridDim.x * kThreads;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < a.n_bones; e += step) {
    const float *b = a.bones + e * 6;
    const float x = b[0], y = b[1], z = b[2], pitch = b[3], yaw = b[4], roll = b[5];
    row_pose(x, y, z, pitch, yaw, roll, a.loc + e * 3, a.rot + e * 9);
  }
}

// N J (+ N) elements as 64-bit counts: refused only where the byte offsets of the 36-byte rows would leave int64
static int check_shape(int64_t N, int32_t J, int32_t max_blocks) {
  if (N < 0 || J < 1 || max_blocks < 0) return P2C_E_SHAPE;
  if (N > (((int64_t)1 << 56) / J)) return P2C_E_SHAPE;
  return 0;
}

static int blocks_for(int64_t elements, int32_t max_blocks) {
  const int cap = max_blocks > 0 && max_blocks < kMaxBlocks ? max_blocks : kMaxBlocks;
  const int64_t want = (elements + kThreads - 1) / kThreads;
  return (int)(want < cap ? want : cap);
}

}  // namespace p2c_carla

using namespace p2c_carla;

extern "C" int p2c_carla_pose_fwd(const float *rel_loc, const float *rel_rot, const float *world_loc, const float *world_rot,
                                  float *bones, float *root, int64_t N, int32_t J, int32_t max_blocks, void *stream) {
  const int rc = check_shape(N, J, max_blocks);
  if (rc) return rc;
  if (!rel_loc || !rel_rot || !bones) return P2C_E_NULL;
  if ((world_loc == nullptr) != (world_rot == nullptr)) return P2C_E_NULL;      // both or neither
  if (world_loc && !root) return P2C_E_NULL;
  if (N == 0) return 0;
  FwdArgs a{};
  a.rel_loc = rel_loc, a.rel_rot = rel_rot, a.world_loc = world_loc, a.world_rot = world_rot;
  a.bones = bones, a.root = world_loc ? root : nullptr;
  a.n_bones = N * J;
  a.n_total = a.n_bones + (world_loc ? N : 0);
  hipLaunchKernelGGL(carla_pose_fwd_kernel, dim3(blocks_for(a.n_total, max_blocks)), dim3(kThreads), 0, (hipStream_t)stream, a);
  return p2c_host::launch_status();
}

extern "C" int p2c_carla_pose_inv(const float *bones, float *loc, float *rot, int64_t N, int32_t J, int32_t max_blocks,
                                  void *stream) {
  const int rc = check_shape(N, J, max_blocks);
  if (rc) return rc;
  if (!bones || !loc || !rot) return P2C_E_NULL;
  if (N == 0) return 0;
  InvArgs a{};
  a.bones = bones, a.loc = loc, a.rot = rot;
  a.n_bones = N * J;
  hipLaunchKernelGGL(carla_pose_inv_kernel, dim3(blocks_for(a.n_bones, max_blocks)), dim3(kThreads), 0, (hipStream_t)stream, a);
  return p2c_host::launch_status();
}
