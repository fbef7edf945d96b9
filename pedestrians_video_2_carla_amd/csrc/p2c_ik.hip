// p2c_ik.hip -- K36: 3-D joint locations -> CARLA bone rotations (inverse kinematics over the 26-bone tree) in one launch (gfx950).
//
// No counterpart in the reference, which cannot play a model that outputs absolute locations. The definition is
// walker_control/inverse_kinematics.py (fit_carla_rotations), row-vector convention. Per frame with skeleton type t, X the frame's
// 26 locations, R_ref / r the relative reference tables of t, A[j] the fitted absolute rotation (A[parent(root)] = I), parents first:
//   P = R_ref[j] A[parent]                                    the prior: the bone keeps its reference relative rotation;
//   a child c is usable when neither |r_c| nor |X[c] - X[j]| is zero (a NaN length is not zero: nothing is masked);
//   no usable child (leaves, root, coincident joints):         A[j] = P,  relative_pose_rot[j] = R_ref[j], the table row itself;
//   one child in the tree, usable:                             u = unit(r_c P), v = unit(X[c] - X[j]), A[j] = P S with S the
//     shortest arc u S = v: h = unit(u + v), the transposed matrix of the quaternion (u.h, u x h); when |u + v|^2 <= 2^-40 the half
//     turn 2 a^T a - I, a = unit(u x e_k), k the index of the smallest |u_k| (lowest on ties);
//   several children in the tree (hips, spine01, head), >= 1 usable: A[j] = p2c_procrustes::solve of H[a][b] = sum d_c[a] r_c[b]
//     over the usable children's unit vectors (NaN when H is not finite);
//   where a fit happened relative_pose_rot[j] = A[j] A[parent]^T;
//   absolute_pose_rot = A, absolute_pose_loc = forward kinematics of (r, A), bones = the K30 row of (r, relative_pose_rot),
//   root = the K30 row of (world_loc, world_rot).
// Only differences of X are read: a fit of directions. Nothing accumulates over frames.
//
// Mapping. The frame group of p2c_carla_dev.h (frame_lane: a bone per lane, 32 lanes per frame), two frames (a pair) per
// wavefront at a time. The group's spare lane holds the identity the root composes with and, with world inputs, writes the root
// row (store_rows). A wavefront takes a chunk of `pairs` consecutive pairs (1 .. 10, chosen on the host from N alone);
// chunks stride over the frames (grid capped at kFrameMaxBlocks workgroups of four wavefronts, max_blocks lowers the cap).
//   * Loads. A lane reads its own joint's 12 bytes (a pair is one 624-byte span) and its bone's 12 floats of the two (4,26,..)
//     tables (load_ref; 5 KB in all: cache resident) after the frame's skeleton type (frame_type: one broadcast load per group,
//     clamped, never followed).
//   * Children. Up to three per bone; their locations and reference offsets come across lanes (ds_bpermute, fp32, 18 moves).
//   * Procrustes first, and together. The absolute rotation of a bone with several children does not depend on its parent, so
//     the solves come out of the tree walk; and only 3 lanes in 32 have one, so a chunk gathers them: phase 1 forms H for every
//     pair of the chunk and moves it to a slot lane (pair * 6 + group * 3 + {hips, spine01, head}), phase 2 is ONE pass of
//     p2c_procrustes::solve on up to 60 lanes, phase 3 hands every R back and walks the trees. Phase 3 reads the chunk's frames a
//     second time (a 6 KB span, cache resident) instead of holding ten pairs in registers. The solve is some thousand fp64
//     instructions, the rest of a frame a few hundred: with one pass per pair the call was bound by three lanes' arithmetic
//     (DESIGN section 5.24). Up to kSpreadFrames frames a chunk is one pair, so that a small call spreads over the SIMDs
//     instead of queueing pairs behind each other; what a frame's result is does not depend on the chunking (tested).
//   * Tree walk. Eight levels, each one round: every lane fetches its parent's A and absolute location (ds_bpermute, 24 dwords),
//     the lanes of that level form the prior and fit. The prior makes a bone wait for its parent: the walk cannot be doubled as
//     K35's forward kinematics is. No LDS, no barrier: a wavefront's lanes run every cross-lane move together (the chunk and
//     pair loops are wavefront-uniform; a frame past the end computes on zeros and stores nothing).
//   * Stores. K35's lane-per-row form: a lane writes its own 36-, 12- and 24-byte rows.
//   * Arithmetic. All of the fit runs in fp64 -- the solve has to, the half-vector form and the eight-deep chain of priors are
//     cheap next to it (fp64 FMA issues at the fp32 rate here) -- on the fp32 inputs and tables. Each output is rounded to fp32
//     once; the rows are carla_row of p2c_carla_dev.h on the rounded relative rotations and the fp32 table offsets: K30's rows on
//     K36's rotations, bit for bit.
// Every output element has one writer and nothing is reduced; what is computed does not depend on which outputs are asked for
// (everything is computed, the stores are behind wave-uniform tests).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "../../include/p2c.h"
#include "p2c_host.h"

#include "p2c_pose_head_dev.h"
#include "p2c_carla_dev.h"
#include "p2c_procrustes_dev.h"

namespace p2c_ik {

namespace ph = p2c;
namespace pc = p2c_carla;
constexpr int J = ph::J;
constexpr int kThreads = pc::kFrameThreads;
constexpr int kMaxPairs = 10;      // frame pairs per wavefront and pass: 6 Procrustes solves each, 60 of the 64 lanes
constexpr int kSpreadFrames = 2048;   // one wavefront per SIMD (1024) times two frames
constexpr int kLevels = 8;        // root .. hand
constexpr double kAntiparallel = 0x1p-40;

// depth of each bone in the tree (idle lanes: no level), its number of children, and the children's lanes (-1: none)
static __constant__ int c_depth[ph::GROUP] = {0, 1, 2, 3, 4, 5, 6, 7, 4, 5, 6, 6, 4, 5, 6, 7, 2, 3, 4, 5, 6, 2, 3, 4, 5, 6,
                                              99, 99, 99, 99, 99, 99};
static __constant__ int c_child[3][ph::GROUP] = {
    {1, 2, 3, 4, 5, 6, 7, -1, 9, 10, -1, -1, 13, 14, 15, -1, 17, 18, 19, 20, -1, 22, 23, 24, 25, -1, -1, -1, -1, -1, -1, -1},
    {-1, 16, -1, 8, -1, -1, -1, -1, -1, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {-1, 21, -1, 12, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}};

struct D3 {
  double x, y, z;
};
struct DM {
  double m[9];  // row-major
};

__device__ __forceinline__ double ddot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ D3 dcross(D3 a, D3 b) { return D3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ D3 dscale(D3 a, double s) { return D3{a.x * s, a.y * s, a.z * s}; }
// a / |a| and whether |a| is not zero (a NaN length is not zero); a zero vector stays zero
__device__ __forceinline__ D3 dunit(D3 a, bool &ok) {
  const double n = sqrt(ddot(a, a));
  ok = !(n == 0.0);
  return dscale(a, 1.0 / (ok ? n : 1.0));
}
__device__ __forceinline__ DM dmul(const DM &a, const DM &b) {             // A @ B
  DM c;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int k = 0; k < 3; ++k) c.m[i * 3 + k] = a.m[i * 3] * b.m[k] + a.m[i * 3 + 1] * b.m[3 + k] + a.m[i * 3 + 2] * b.m[6 + k];
  return c;
}
__device__ __forceinline__ DM dmulNT(const DM &a, const DM &b) {           // A @ B^T
  DM c;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int k = 0; k < 3; ++k)
      c.m[i * 3 + k] = a.m[i * 3] * b.m[k * 3] + a.m[i * 3 + 1] * b.m[k * 3 + 1] + a.m[i * 3 + 2] * b.m[k * 3 + 2];
  return c;
}
__device__ __forceinline__ D3 dvmul(D3 v, const DM &a) {                   // row vector times matrix
  return D3{v.x * a.m[0] + v.y * a.m[3] + v.z * a.m[6], v.x * a.m[1] + v.y * a.m[4] + v.z * a.m[7],
            v.x * a.m[2] + v.y * a.m[5] + v.z * a.m[8]};
}
__device__ __forceinline__ double dshfl(double v, int src_lane) { return __shfl(v, src_lane, 64); }

// the shortest-arc rotation S with u S = v, for unit u and v
__device__ __forceinline__ DM shortest_arc(D3 u, D3 v) {
  const D3 s = D3{u.x + v.x, u.y + v.y, u.z + v.z};
  const double s2 = ddot(s, s);
  DM S;
  if (s2 <= kAntiparallel) {       // false for NaN: a NaN runs the half-vector form and comes out as NaN
    const double m0 = fabs(u.x), m1 = fabs(u.y), m2 = fabs(u.z);
    const int k = (m0 <= m1 && m0 <= m2) ? 0 : (m1 <= m2 ? 1 : 2);
    D3 a = k == 0 ? D3{0.0, u.z, -u.y} : (k == 1 ? D3{-u.z, 0.0, u.x} : D3{u.y, -u.x, 0.0});      // u x e_k
    a = dscale(a, 1.0 / sqrt(ddot(a, a)));
    const double av[3] = {a.x, a.y, a.z};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int k2 = 0; k2 < 3; ++k2) S.m[i * 3 + k2] = 2.0 * av[i] * av[k2] - (i == k2 ? 1.0 : 0.0);
  } else {
    const D3 h = dscale(s, 1.0 / sqrt(s2));
    const double q0 = ddot(u, h);
    const D3 q = dcross(u, h);
    const double qx = q.x, qy = q.y, qz = q.z;
    S.m[0] = q0 * q0 + qx * qx - qy * qy - qz * qz, S.m[1] = 2.0 * (qy * qx + q0 * qz), S.m[2] = 2.0 * (qz * qx - q0 * qy);
    S.m[3] = 2.0 * (qx * qy - q0 * qz), S.m[4] = q0 * q0 - qx * qx + qy * qy - qz * qz, S.m[5] = 2.0 * (qz * qy + q0 * qx);
    S.m[6] = 2.0 * (qx * qz + q0 * qy), S.m[7] = 2.0 * (qy * qz - q0 * qx), S.m[8] = q0 * q0 - qx * qx - qy * qy + qz * qz;
  }
  return S;
}

struct Args {
  const float *loc;
  const int32_t *skel_type;
  const float *ref_rel_loc, *ref_rel_rot, *world_loc, *world_rot;
  float *rel_rot, *abs_loc, *abs_rot, *bones, *root;
  int64_t N;
  int32_t frames_per_type;
  int32_t pairs;                 // frame pairs a wavefront takes at a time: 1 .. kMaxPairs
};

struct LaneConsts : pc::FrameLane {
  int parent, depth, ch[3];
  bool multi;
};

// this lane's joint, the frame's skeleton type, the bone's reference rows, the children's unit offsets (every lane of the
// wavefront calls this together: the children come across lanes)
// Out: l0..l2 the bone's reference offset, q its reference relative rotation (row-major), rh0 / dh0 the unit reference / observed offset
// of the first child, any_usable, and for the bones with several children H = the sum over the usable children of d^T r.
// (Plain out-parameters: returned as a struct, the floats are also written to scratch memory that nothing reads.)
__device__ __forceinline__ void read_frame(const Args &a, const LaneConsts &L, int64_t n, bool valid, float &l0, float &l1, float &l2,
                                           float (&q)[9], D3 &rh0, D3 &dh0, bool &any_usable, double (&H)[9]) {
  float x0 = 0.f, x1 = 0.f, x2 = 0.f;
  int st = 0;
  if (valid) {
    if (L.bone) {
      const float *p = a.loc + (n * J + L.j) * 3;
      x0 = p[0], x1 = p[1], x2 = p[2];
    }
    st = pc::frame_type(a.skel_type, n, a.frames_per_type);
  }
  pc::load_ref(a.ref_rel_rot, a.ref_rel_loc, (size_t)st * J + L.jb, q, l0, l1, l2);

#pragma unroll
  for (int i = 0; i < 9; ++i) H[i] = 0.0;
  any_usable = false;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int src = L.base + (L.ch[k] >= 0 ? L.ch[k] : L.j);
    const float c0 = ph::shfl(x0, src), c1 = ph::shfl(x1, src), c2 = ph::shfl(x2, src);
    const float r0 = ph::shfl(l0, src), r1 = ph::shfl(l1, src), r2 = ph::shfl(l2, src);
    bool r_ok, d_ok;
    const D3 rh = dunit(D3{(double)r0, (double)r1, (double)r2}, r_ok);
    const D3 dh = dunit(D3{(double)c0 - (double)x0, (double)c1 - (double)x1, (double)c2 - (double)x2}, d_ok);
    const bool usable = L.bone && L.ch[k] >= 0 && r_ok && d_ok;
    any_usable = any_usable || usable;
    if (k == 0) rh0 = rh, dh0 = dh;
    const double d[3] = {dh.x, dh.y, dh.z}, r[3] = {rh.x, rh.y, rh.z};
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int q = 0; q < 3; ++q) H[p * 3 + q] += usable ? d[p] * r[q] : 0.0;
  }
}

__global__ __launch_bounds__(kThreads) void loc_to_carla_kernel(const Args a) {
  LaneConsts L;
  static_cast<pc::FrameLane &>(L) = pc::frame_lane();
  L.parent = L.base + ph::c_parent[L.j];               // root and idle lanes: the identity lane / themselves
  L.depth = c_depth[L.j];
  L.ch[0] = c_child[0][L.j], L.ch[1] = c_child[1][L.j], L.ch[2] = c_child[2][L.j];
  L.multi = L.ch[1] >= 0;
  const int j = L.j, group = L.lane >> 5;
  // Procrustes slots: lane s < 6 * pairs solves for pair s / 6, group (s % 6) / 3, bone {hips, spine01, head}[s % 3]
  const int slot_bone = (L.lane % 3) == 0 ? 1 : ((L.lane % 3) == 1 ? 3 : 9);
  const int slot_src = L.lane < 6 * kMaxPairs ? ((L.lane % 6) / 3) * 32 + slot_bone : L.lane;
  const int slot_pair = L.lane / 6;
  const int my_slot = group * 3 + (j == 1 ? 0 : (j == 3 ? 1 : 2));      // + 6 * pair: where a bone with several children finds its fit

  const int64_t chunk_frames = 2 * (int64_t)a.pairs;
  const int64_t waves = (int64_t)gridDim.x * (kThreads / 64);
  for (int64_t c = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6); c * chunk_frames < a.N; c += waves) {
    const int64_t n0 = c * chunk_frames;
    // ---- phase 1: the Procrustes matrices of the chunk's frames, gathered one per lane ----
    double S[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < a.pairs && n0 + 2 * i < a.N; ++i) {
      const int64_t n = n0 + 2 * i + group;
      float l0, l1, l2, q[9];
      D3 rh0, dh0;
      bool any_usable;
      double H[9];
      read_frame(a, L, n, n < a.N, l0, l1, l2, q, rh0, dh0, any_usable, H);
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        const double t = dshfl(H[k], slot_src);
        S[k] = slot_pair == i ? t : S[k];
      }
    }
    // ---- phase 2: every slot solves its own (a slot without a frame solves zeros and is never read) ----
    if (L.lane < 6 * a.pairs) {
      double H[3][3], R[3][3], sum;
      bool finite = true;
#pragma unroll
      for (int k = 0; k < 9; ++k) H[k / 3][k % 3] = S[k], finite = finite && isfinite(S[k]);
      p2c_procrustes::solve(H, R, sum);
#pragma unroll
      for (int k = 0; k < 9; ++k) S[k] = finite ? R[k / 3][k % 3] : (double)__builtin_nanf("");
    }
    // ---- phase 3: the tree of every frame, level by level ----
    for (int i = 0; i < a.pairs && n0 + 2 * i < a.N; ++i) {
      const int64_t n = n0 + 2 * i + group;
      const bool valid = n < a.N;
      float l0, l1, l2, q[9];
      D3 rh0, dh0;
      bool any_usable;
      double H[9];
      read_frame(a, L, n, valid, l0, l1, l2, q, rh0, dh0, any_usable, H);
      DM A;
      {
        const int from = L.multi ? 6 * i + my_slot : L.lane;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          const double t = dshfl(S[k], from);
          A.m[k] = (L.multi && any_usable) ? t : ((k % 4 == 0) ? 1.0 : 0.0);
        }
      }
      DM rel;
#pragma unroll
      for (int k = 0; k < 9; ++k) rel.m[k] = (double)q[k];
      D3 al = D3{0.0, 0.0, 0.0};
      for (int level = 0; level < kLevels; ++level) {
        DM Ap;
#pragma unroll
        for (int k = 0; k < 9; ++k) Ap.m[k] = dshfl(A.m[k], L.parent);
        const D3 lp = D3{dshfl(al.x, L.parent), dshfl(al.y, L.parent), dshfl(al.z, L.parent)};
        if (L.depth == level) {
          const D3 moved = dvmul(D3{(double)l0, (double)l1, (double)l2}, Ap);
          al = D3{moved.x + lp.x, moved.y + lp.y, moved.z + lp.z};
          const DM P = dmul(rel, Ap);                   // rel still holds the reference row
          if (!any_usable) {
            A = P;
          } else {
            if (!L.multi) {
              bool ok;
              const D3 u = dunit(dvmul(rh0, P), ok);
              A = dmul(P, shortest_arc(u, dh0));
            }
            rel = dmulNT(A, Ap);
          }
        }
      }

      // ---- stores: every output rounded to fp32 once ----
      if (!valid) continue;
      const float f0 = (float)rel.m[0], f1 = (float)rel.m[1], f2 = (float)rel.m[2], f3 = (float)rel.m[3], f4 = (float)rel.m[4],
                  f5 = (float)rel.m[5], f6 = (float)rel.m[6], f7 = (float)rel.m[7], f8 = (float)rel.m[8];
      if (L.bone && a.rel_rot) {
        float *o = a.rel_rot + ((size_t)n * J + j) * 9;
        o[0] = f0, o[1] = f1, o[2] = f2, o[3] = f3, o[4] = f4, o[5] = f5, o[6] = f6, o[7] = f7, o[8] = f8;
      }
      if (L.bone && a.abs_rot) {
        float *o = a.abs_rot + ((size_t)n * J + j) * 9;
#pragma unroll
        for (int k = 0; k < 9; ++k) o[k] = (float)A.m[k];
      }
      if (L.bone && a.abs_loc) {
        float *o = a.abs_loc + ((size_t)n * J + j) * 3;
        o[0] = (float)al.x, o[1] = (float)al.y, o[2] = (float)al.z;
      }
      // rows: p2c_carla::carla_row(table offset, rounded relative rotation) by the bone lanes, the world's by the spare lane
      pc::store_rows(a.bones, a.root, a.world_loc, a.world_rot, n, L, l0, l1, l2, f0, f1, f2, f5, f8);
    }
  }
}

}  // namespace p2c_ik

using namespace p2c_ik;

extern "C" int p2c_loc_to_carla_fwd(const float *loc, const int32_t *skel_type, int64_t frames_per_type, const float *ref_rel_loc,
                                    const float *ref_rel_rot, const float *world_loc, const float *world_rot,
                                    float *relative_pose_rot, float *absolute_pose_loc, float *absolute_pose_rot, float *bones,
                                    float *root, int64_t N, int32_t max_blocks, void *stream) {
  const int rc = pc::check_frames_call(N, frames_per_type, max_blocks, loc && skel_type && ref_rel_loc && ref_rel_rot,
                                       relative_pose_rot || absolute_pose_loc || absolute_pose_rot || bones || root, world_loc,
                                       world_rot, root);
  if (rc || N == 0) return rc;
  Args a{};
  a.loc = loc, a.skel_type = skel_type;
  a.ref_rel_loc = ref_rel_loc, a.ref_rel_rot = ref_rel_rot;
  a.world_loc = world_loc, a.world_rot = world_rot;
  a.rel_rot = relative_pose_rot, a.abs_loc = absolute_pose_loc, a.abs_rot = absolute_pose_rot, a.bones = bones, a.root = root;
  a.N = N, a.frames_per_type = (int32_t)frames_per_type;
  // up to kSpreadFrames frames every pair of frames has a wavefront of its own (the shortest call); beyond, a wavefront takes
  // more pairs at a time and their Procrustes solves share one pass
  const int64_t pairs = (N + kSpreadFrames - 1) / kSpreadFrames;
  a.pairs = (int32_t)(pairs < 1 ? 1 : (pairs > kMaxPairs ? kMaxPairs : pairs));
  const int64_t chunks = (N + 2 * a.pairs - 1) / (2 * a.pairs);
  const unsigned grid = p2c_host::grid_for((chunks + kThreads / 64 - 1) / (kThreads / 64), max_blocks, pc::kFrameMaxBlocks);
  hipLaunchKernelGGL(loc_to_carla_kernel, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, a);
  return p2c_host::launch_status();
}
