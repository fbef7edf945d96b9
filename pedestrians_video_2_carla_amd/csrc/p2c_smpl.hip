// p2c_smpl.hip -- K35: SMPL body poses (AMASS) -> CARLA bone transforms in one launch (gfx950).
//
// Reference: data/smpl/smpl_dataset.py:103-142 (SMPLDataset.convert_smpl_to_carla, per clip on a DataLoader worker: 26 small bmm,
// a batched linalg.solve, a recursive FK) with data/smpl/utils.py:53-58 and data/smpl/skeleton.py:9-34,133-142; restated on
// tensors in data/smpl/retarget.py. Per frame with skeleton type t:
//   p (22,3) = the frame's 66 values in ORIGINAL SMPL joint order;  M[s] = Rx Ry Rz of (-p[s][0], p[s][1], p[s][2]);
//   C[bone] = M[its SMPL joint], C[spine01] = M[Spine3] @ M[Spine2];  L = abs_ref_rot[t][bone] @ K, K = [[1,0,0],[0,0,-1],[0,1,0]]:
//   the columns (a0, a2, -a1) of abs_ref_rot, formed while the row is read;  local = (L^T C) L;
//   relative_pose_rot = local @ ref_rel_rot[t][bone]; the five bones without an SMPL joint keep ref_rel_rot[t][bone] itself;
//   absolute_pose_* = forward kinematics of (ref_rel_loc[t], relative_pose_rot), row-vector convention;
//   bones = the K30 row of (ref_rel_loc[t], relative_pose_rot), root = the K30 row of (world_loc, world_rot).
// No masking: a NaN joint reaches its bone and the bone's descendants. Nothing accumulates over frames.
//
// Mapping. The frame group of p2c_carla_dev.h (frame_lane: a bone per lane, 32 lanes per frame), two frames per wavefront, eight
// per workgroup; groups stride over the frames (grid capped at kFrameMaxBlocks workgroups, max_blocks lowers the cap). The group's
// spare lane converts Spine2 -- the SMPL joint no bone owns -- and, with world inputs, writes the root row (store_rows); for the
// forward kinematics it is the identity lane of the pose head's tree walk.
//   * Frame loads. Every one of the 22 SMPL joints belongs to exactly one lane (21 bones + the spare), which reads its own 12
//     bytes: the 22 loads of a group cover the frame's 264 bytes once and a wavefront's two frames are one 528-byte span. No
//     staging: nothing is read twice. Only M[Spine2] changes lanes (spare -> spine01, nine ds_bpermute).
//   * Tables. A lane reads its bone's 21 floats of the three (4,26,..) reference tables (8.7 KB in all: cache resident) after
//     the frame's skeleton type (frame_type: one broadcast load per group, clamped, never followed).
//   * Forward kinematics. fk_doubling of p2c_pose_head_dev.h: pointer doubling in three rounds instead of eight dependent
//     levels -- DPP row_shr:1 where the parent is the previous lane, ds_bpermute for the two ancestor rounds. Both stay in
//     registers: no LDS allocation, no barrier (a frame's lanes sit in one wavefront), and no LDS for the poison audit to find.
//   * Stores. The lane-per-row form of K30 (see p2c_carla_pose.hip): a lane writes its own 36-, 12- and 24-byte rows, 4-byte
//     aligned, which the compiler merges into multi-dword stores; the 52 rows of a wavefront are one contiguous span of 1872 /
//     624 / 1248 bytes per tensor, so every 128-byte line it touches leaves the wavefront whole, bar the two at the span's ends,
//     which the neighbouring wavefronts complete in L2.
//   * Arithmetic. sincosf, the closed form of carla_pose_inv_kernel; mul / mulTN / vmul of the pose head; carla_row unchanged.
// Every output element has one writer and nothing is reduced; what is computed does not depend on which outputs are asked
// for (the stores are behind wave-uniform tests, the forward kinematics runs only when an absolute tensor is wanted).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/p2c.h"
#include "p2c_host.h"

#include "p2c_pose_head_dev.h"
#include "p2c_carla_dev.h"

namespace p2c_smpl {

namespace ph = p2c;
namespace pc = p2c_carla;
constexpr int J = ph::J;
constexpr int kFramesPerBlock = pc::kFrameThreads / ph::GROUP;
constexpr int kSmplValues = 66;

// lane -> the ORIGINAL-order SMPL joint it converts (-1: none). Lanes 0..25: the 21 pairs of get_common_indices(SMPL_SKELETON);
// lane 26: Spine2. Every joint 0..21 appears once.
static __constant__ int c_smpl_joint[ph::GROUP] = {-1, 0, 3, 9, 13, 16, 18, 20, 12, 15, -1, -1, 14, 17, 19, 21, 2, 5, 8, 11, -1,
                                                   1, 4, 7, 10, -1, 6, -1, -1, -1, -1, -1};
constexpr int kSpine01 = 3;        // CARLA_SKELETON.crl_spine01__C

struct Args {
  const float *body_pose;
  const int32_t *skel_type;
  const float *ref_rel_loc, *ref_rel_rot, *ref_abs_rot, *world_loc, *world_rot;
  float *rel_rot, *abs_loc, *abs_rot, *bones, *root;
  int64_t N;
  int32_t frames_per_type;
};

__global__ __launch_bounds__(pc::kFrameThreads) void smpl_to_carla_kernel(const Args a) {
  const pc::FrameLane F = pc::frame_lane();
  ph::LaneCtx L;
  L.lane = F.lane, L.j = F.j, L.base = F.base;
  L.anc0 = ph::c_parent[L.j], L.anc1 = ph::c_anc_r2[L.j], L.anc2 = ph::c_anc_r3[L.j];
  L.interior = (ph::kInteriorMask >> L.j) & 1u;
  const bool bone = F.bone;
  const int sj = c_smpl_joint[L.j];
  const bool want_fk = a.abs_loc || a.abs_rot;

  const int64_t step = (int64_t)gridDim.x * kFramesPerBlock;
  for (int64_t n = (int64_t)blockIdx.x * kFramesPerBlock + (threadIdx.x >> 5); n < a.N; n += step) {
    // ---- the frame's joint of this lane, its skeleton type, the bone's reference rows ----
    float p0 = 0.f, p1 = 0.f, p2 = 0.f;
    if (sj >= 0) {
      const float *p = a.body_pose + n * kSmplValues + sj * 3;
      p0 = p[0], p1 = p[1], p2 = p[2];
    }
    const size_t row = (size_t)pc::frame_type(a.skel_type, n, a.frames_per_type) * J + F.jb;
    ph::M3 R0, Lm;
    ph::V3 l0;
    pc::load_ref(a.ref_rel_rot, a.ref_rel_loc, row, R0.m, l0.x, l0.y, l0.z);
    {
      const float *pa = a.ref_abs_rot + row * 9;
#pragma unroll
      for (int i = 0; i < 3; ++i) Lm.m[i * 3 + 0] = pa[i * 3 + 0], Lm.m[i * 3 + 1] = pa[i * 3 + 2], Lm.m[i * 3 + 2] = -pa[i * 3 + 1];
    }

    // ---- M = Rx Ry Rz of (-p0, p1, p2) ----
    float s0, c0, s1, c1, s2, c2;
    sincosf(-p0, &s0, &c0);
    sincosf(p1, &s1, &c1);
    sincosf(p2, &s2, &c2);
    ph::M3 M;
    M.m[0] = c1 * c2;
    M.m[1] = -(c1 * s2);
    M.m[2] = s1;
    M.m[3] = c0 * s2 + (s0 * s1) * c2;
    M.m[4] = c0 * c2 - (s0 * s1) * s2;
    M.m[5] = -(s0 * c1);
    M.m[6] = s0 * s2 - (c0 * s1) * c2;
    M.m[7] = s0 * c2 + (c0 * s1) * s2;
    M.m[8] = c0 * c1;
    {   // spine01: M[Spine3] @ M[Spine2], the latter from the spare lane
      const ph::M3 M2 = ph::shfl(M, L.base + ph::IDL);
      const ph::M3 C2 = ph::mul(M, M2);
      if (L.j == kSpine01) M = C2;
    }
    // ---- local = (L^T C) L, relative_pose_rot = local @ ref_rel_rot ----
    ph::M3 R = ph::mul(ph::mul(ph::mulTN(Lm, M), Lm), R0);
    if (sj < 0) R = R0;
    if (bone && a.rel_rot) ph::store_m3(a.rel_rot, (size_t)n * J + L.j, R);

    // ---- rows: bones by their lanes, the root row by the spare lane ----
    pc::store_rows(a.bones, a.root, a.world_loc, a.world_rot, n, F, l0.x, l0.y, l0.z, R.m[0], R.m[1], R.m[2], R.m[5], R.m[8]);

    // ---- forward kinematics over the group ----
    if (want_fk) {
      if (!bone) R = ph::identity(), l0 = ph::v3(0.f, 0.f, 0.f);
      ph::fk_doubling(L, R, l0);
      if (bone && a.abs_rot) ph::store_m3(a.abs_rot, (size_t)n * J + L.j, R);
      if (bone && a.abs_loc) {
        float *o = a.abs_loc + ((size_t)n * J + L.j) * 3;
        o[0] = l0.x, o[1] = l0.y, o[2] = l0.z;
      }
    }
  }
}

}  // namespace p2c_smpl

using namespace p2c_smpl;

extern "C" int p2c_smpl_to_carla_fwd(const float *body_pose, const int32_t *skel_type, int64_t frames_per_type,
                                     const float *ref_rel_loc, const float *ref_rel_rot, const float *ref_abs_rot,
                                     const float *world_loc, const float *world_rot, float *relative_pose_rot,
                                     float *absolute_pose_loc, float *absolute_pose_rot, float *bones, float *root, int64_t N,
                                     int32_t max_blocks, void *stream) {
  const int rc = pc::check_frames_call(N, frames_per_type, max_blocks, body_pose && skel_type && ref_rel_loc && ref_rel_rot && ref_abs_rot,
                                       relative_pose_rot || absolute_pose_loc || absolute_pose_rot || bones || root, world_loc,
                                       world_rot, root);
  if (rc || N == 0) return rc;
  Args a{};
  a.body_pose = body_pose, a.skel_type = skel_type;
  a.ref_rel_loc = ref_rel_loc, a.ref_rel_rot = ref_rel_rot, a.ref_abs_rot = ref_abs_rot;
  a.world_loc = world_loc, a.world_rot = world_rot;
  a.rel_rot = relative_pose_rot, a.abs_loc = absolute_pose_loc, a.abs_rot = absolute_pose_rot, a.bones = bones, a.root = root;
  a.N = N, a.frames_per_type = (int32_t)frames_per_type;
  const unsigned grid = p2c_host::grid_for((N + kFramesPerBlock - 1) / kFramesPerBlock, max_blocks, pc::kFrameMaxBlocks);
  hipLaunchKernelGGL(smpl_to_carla_kernel, dim3(grid), dim3(pc::kFrameThreads), 0, (hipStream_t)stream, a);
  return p2c_host::launch_status();
}
