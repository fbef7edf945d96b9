// p2c_lift.hip -- K32: 2-D keypoint clips -> CARLA bone transforms in one launch (gfx950).
//
// What a user with a trained LitPoseLiftingFlow(LinearAE) runs to feed a CARLA walker, as three calls: LinearAE.forward
// (K8, p2c_mlp_fwd) -> the materialising pose head (pose_head_rot_fwd<KIND, true>: forward kinematics, projection, eight tensors,
// of which the export reads two) -> p2c_carla_pose_fwd (K30). Here the model output y (B,T,26,6) and the relative rotations
// (B,T,26,3,3) never leave LDS, nothing the export does not read is computed, and relative_pose_loc is the row of the
// reference table of the clip's skeleton type. The running rotation of the pose_changes kind may start from a caller's
// (B,26,3,3) instead of the reference pose, and its last value is handed back: a video cut into clips continues its pose.
//
// Structure (the bits of the three calls depend on it):
//   * one workgroup of eight waves per clip, min(B, 256) workgroups striding over the clips; the 84 KB weight image is staged
//     into LDS once per workgroup, during its first tile (mlp_fwd_kernel's schedule: stage_issue / stage_commit per layer);
//   * a clip is walked in tiles of 16 frames = one MFMA sample tile. A tile runs the LinearAE forward with the cooperative-tile
//     code of p2c_mlp_dev.h exactly as mlp_fwd_kernel / train_clip_kernel do (fp32 MFMA = an fmaf chain in k order: a frame's
//     column does not depend on which tile or which wave computes it); the last layer leaves y^T in LDS. Frames beyond the clip
//     in a partial last tile are zero columns: computed, never written out;
//   * phase A, one lane per (frame, joint) of the tile: c = rot6d_fwd(y) -> the tile's rotation plane RT[t][j][9] in LDS. The
//     orthonormalisation of a frame does not depend on any other frame: its 416 instances run side by side;
//   * phase B (pose_changes only), lane j of wave 0: R = mul(c_t, R) for t in frame order, R in registers across the tiles of the
//     clip, each R_t written over c_t. This is the sequential product of pose_head_rot_fwd (not the time-parallel scan of K13,
//     whose rounding order differs): the same functions on the same operands in the same order;
//   * phase C, one lane per (frame, joint) again: the row of carla_pose_fwd_kernel (p2c_carla_dev.h) from RT and the reference
//     location; sixteen more lanes convert the tile's root rows; RT, whose layout is that of (T,26,3,3), is copied out as it is
//     when relative_pose_rot is wanted.
// Every output element has one writer and nothing is reduced: no atomics, no workspace, two runs give the same bits.
//
// LDS: image 83.7 KB | H_0 .. H_5, y^T (528 rows of pitch 17) 35.9 KB | RT 15.0 KB = 134.6 KB of 160 KB. Banks (64 x 4 B): phase A
// reads y^T at (6 j + i) * 17 + t, a lane stride of 102 floats = 2-way; RT is touched at a lane stride of 9 floats (odd):
// conflict-free; the copy-out and the layers' accesses are those of K8.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "../../include/p2c.h"
#include "p2c_host.h"

#include "p2c_mlp_dev.h"
#include "p2c_pose_head_dev.h"
#include "p2c_carla_dev.h"

namespace p2c_lift {

using namespace p2c_mlp;
namespace ph = p2c;
using S = LinearAE156;
constexpr int NLAY = S::NLAY;
constexpr int J = ph::J;
constexpr int ELEMS = TS * J;                 // (frame, joint) elements of a tile
constexpr int RT_FLOATS = ELEMS * 9;
constexpr int LDS_FLOATS = S::w_total() + S::act_rows() * TP + RT_FLOATS;
constexpr int kMaxBlocks = 256;               // one 135 KB-LDS workgroup per CU
static_assert((size_t)LDS_FLOATS * sizeof(float) <= 160 * 1024, "image + activations + rotation plane must fit the LDS");
static_assert(ELEMS + TS <= NTH, "one lane per (frame, joint) of a tile, sixteen more for the root rows");
static_assert(S::dims(NLAY) == J * 6, "the model emits one 6-D rotation per joint");

struct LiftArgs {
  const float *x, *w_image;
  const int32_t *skel_type;
  const float *ref_rel_loc, *ref_rel_rot, *world_loc, *world_rot, *initial_rel_rot;
  float *bones, *root, *final_rel_rot, *out_rot;
  int32_t B, T, vec_x;
};

template <int KIND>
__global__ __launch_bounds__(NTH) void lift_kernel(const LiftArgs a) {
  using K = ph::KindTraits<KIND>;
  static_assert(K::SIXD, "the lift kernel is for the 6-D kinds");
  extern __shared__ float lds[];
  const S sh;
  Lane L;
  L.lane = threadIdx.x & 63, L.c = L.lane & 15, L.g = L.lane >> 4;
  L.wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  constexpr int total4 = S::w_total() >> 2;
  float *H = lds + S::w_total();
  float *Y = H + S::h_off(NLAY) * TP;          // y^T[6 j + i][frame]
  float *RT = H + S::act_rows() * TP;          // [frame][joint][9]
  const int T = a.T, n_tiles = (T + TS - 1) / TS;
  const bool vec = a.vec_x != 0;

  // this lane's (frame, joint) of a tile in phases A and C; lanes ELEMS .. ELEMS + 15 take the root rows
  const int e = threadIdx.x;
  const bool elem = e < ELEMS;
  const int et = elem ? e / J : 0, ej = elem ? e - et * J : 0;
  const bool chain = K::SCAN && L.wave == 0 && L.lane < J;      // phase B: lane = joint

  TileRegs xr;
  ImageRegs wr;
  tile_issue<NTH>(a.x, (int64_t)blockIdx.x * T, (int64_t)blockIdx.x * T + T, S::dims(0), vec, xr);   // grid <= B: a real clip
  stage_issue(a.w_image, total4, wr, 0, 0, issue_mark<S>(1));
  init_rows<NTH>(H, S::h_off(0) + S::dims(0), S::h_off(0) + k_rows(S::dims(0)), S::h_off(0) + S::dims(0));

  ph::M3 R = ph::identity();       // running relative rotation of joint `lane` (phase B lanes)
  float lraw[3] = {0.f, 0.f, 0.f};   // reference location of joint ej for this clip's skeleton type

  auto one_tile = [&](const int clip, const int tile, auto first_c) {
    constexpr bool first = decltype(first_c)::value;
    const int t0 = tile * TS;
    const int n_valid = T - t0 < TS ? T - t0 : TS;
    if (tile == 0) {   // per clip: the reference rows (consumed behind the six layers)
      const int st = a.skel_type[clip];
      if (elem) {
        const float *pl = a.ref_rel_loc + ((size_t)st * J + ej) * 3;
        lraw[0] = pl[0], lraw[1] = pl[1], lraw[2] = pl[2];
      }
      if (chain) {
        const float *pr = a.initial_rel_rot ? a.initial_rel_rot + ((size_t)clip * J + L.lane) * 9
                                            : a.ref_rel_rot + ((size_t)st * J + L.lane) * 9;
#pragma unroll
        for (int i = 0; i < 9; ++i) R.m[i] = pr[i];
      }
    }
    // ---- LinearAE forward of the tile's frames (mlp_fwd_kernel's schedule); the last layer writes y^T to LDS ----
    tile_commit<NTH>(S::dims(0), vec, xr, H + S::h_off(0) * TP);
    {   // this workgroup's next tile waits in registers: the clip's next 16 frames, or the first of its next clip
      const bool same = tile + 1 < n_tiles;
      const int64_t nclip = same ? clip : (int64_t)clip + gridDim.x;
      const int64_t row0 = nclip * T + (same ? t0 + TS : 0);
      tile_issue<NTH>(a.x, row0, nclip < a.B ? nclip * T + T : 0, S::dims(0), vec, xr);
    }
    for_layers(sh, 0, NLAY, [&](int l) {
      if constexpr (first) stage_commit(total4, wr, lds, 0, l == 0 ? 0 : rounds_upto<S>(l - 1), rounds_upto<S>(l));
      lds_barrier();
      if constexpr (first) stage_issue(a.w_image, total4, wr, 0, issue_mark<S>(l + 1), issue_mark<S>(l + 2));
      const bool last = (l == NLAY - 1);
      layer_forward<P2C_PREC_F32, true>(L, lds + S::w_off(l), S::ld(l), S::dims(l), S::dims(l + 1), !last, H + S::h_off(l) * TP,
                                        last ? Y : H + S::h_off(l + 1) * TP, nullptr, false, false);
    });
    lds_barrier();
    // ---- phase A: c = rot6d_fwd(y) per (frame, joint) ----
    if (elem) {
      float y6[6];
#pragma unroll
      for (int i = 0; i < 6; ++i) y6[i] = Y[(ej * 6 + i) * TP + et];
      y6[0] += 0.f, y6[4] += 0.f;            // as rotation_input() of the pose head consumes a frame (a -0 becomes +0)
      ph::SixD s;
      const ph::M3 c = ph::rot6d_fwd(y6, s);
#pragma unroll
      for (int i = 0; i < 9; ++i) RT[e * 9 + i] = c.m[i];
    }
    lds_barrier();
    // ---- phase B: the sequential product over the frames of the tile ----
    if constexpr (K::SCAN) {
      if (chain) {
        for (int t = 0; t < n_valid; ++t) {
          float *p = RT + (t * J + L.lane) * 9;
          ph::M3 c;
#pragma unroll
          for (int i = 0; i < 9; ++i) c.m[i] = p[i];
          R = ph::mul(c, R);
#pragma unroll
          for (int i = 0; i < 9; ++i) p[i] = R.m[i];
        }
        if (tile == n_tiles - 1 && a.final_rel_rot) ph::store_m3(a.final_rel_rot, (size_t)clip * J + L.lane, R);
      }
      lds_barrier();
    }
    // ---- phase C: the rows ----
    const size_t frame0 = (size_t)clip * T + t0;
    if (elem && et < n_valid) {
      const float *r = RT + e * 9;
      p2c_carla::carla_row(lraw[0], lraw[1], lraw[2], r[0], r[1], r[2], r[5], r[8], a.bones + (frame0 * J + e) * 6);
    }
    if (a.root && e >= ELEMS && e - ELEMS < n_valid) {
      const size_t frame = frame0 + (e - ELEMS);
      float x = 0.f, y = 0.f, z = 0.f, r00 = 1.f, r01 = 0.f, r02 = 0.f, r12 = 0.f, r22 = 1.f;   // the identity world
      if (a.world_loc) {
        const float *p = a.world_loc + frame * 3, *r = a.world_rot + frame * 9;
        x = p[0], y = p[1], z = p[2];
        r00 = r[0], r01 = r[1], r02 = r[2], r12 = r[5], r22 = r[8];
      }
      asm volatile("" : "+v"(x), "+v"(y), "+v"(z), "+v"(r00), "+v"(r01), "+v"(r02), "+v"(r12), "+v"(r22));   // run-time values either way
      p2c_carla::carla_row(x, y, z, r00, r01, r02, r12, r22, a.root + frame * 6);
    }
    if (a.out_rot) {
      float *dst = a.out_rot + frame0 * (J * 9);
      for (int i = e; i < n_valid * J * 9; i += NTH) dst[i] = RT[i];
    }
  };

  int clip = blockIdx.x, tile = 0;
  one_tile(clip, tile, std::true_type{});
  for (;;) {
    if (++tile == n_tiles) tile = 0, clip += gridDim.x;
    if (clip >= a.B) break;
    one_tile(clip, tile, std::false_type{});
  }
}

static bool geometry_ok(const p2c_mlp_desc &m) {
  if (m.n_layers != NLAY) return false;
  for (int l = 0; l <= NLAY; ++l)
    if (m.dims[l] != S::dim_at(l)) return false;
  return true;
}
static bool kind_ok(int32_t kind) { return kind == P2C_KIND_POSE_CHANGES_6D || kind == P2C_KIND_RELATIVE_ROT_6D; }

}  // namespace p2c_lift

using namespace p2c_lift;

extern "C" int p2c_lift_supported(const p2c_lift_desc *d) {
  return d && geometry_ok(d->mlp) && kind_ok(d->kind) && d->mlp.precision == P2C_PREC_F32 ? 1 : 0;
}

extern "C" int p2c_lift_fwd(const p2c_lift_desc *d, void *stream) {
  if (!d) return P2C_E_NULL;
  if (d->B < 0 || d->T < 0 || d->max_blocks < 0) return P2C_E_SHAPE;
  if (!kind_ok(d->kind) || d->mlp.precision != P2C_PREC_F32) return P2C_E_ENUM;
  if (!geometry_ok(d->mlp)) return P2C_E_SHAPE;
  if ((int64_t)d->B * d->T > ((int64_t)1 << 40) || d->mlp.N != (int64_t)d->B * d->T) return P2C_E_SHAPE;
  if (!d->mlp.x || !d->mlp.w_image || !d->skel_type || !d->ref_rel_loc || !d->ref_rel_rot || !d->bones) return P2C_E_NULL;
  if ((d->world_loc == nullptr) != (d->world_rot == nullptr)) return P2C_E_NULL;      // both or neither
  if (d->world_loc && !d->root) return P2C_E_NULL;
  if (!d->mlp.skip_pack)
    for (int l = 0; l < NLAY; ++l)
      if (!d->mlp.W[l] || !d->mlp.b[l]) return P2C_E_NULL;
  if (d->B == 0 || d->T == 0) return 0;
  if (!d->mlp.skip_pack) {
    const int rc = p2c_mlp_pack(&d->mlp, stream);
    if (rc) return rc;
  }
  LiftArgs a{};
  a.x = d->mlp.x, a.w_image = d->mlp.w_image, a.skel_type = d->skel_type;
  a.ref_rel_loc = d->ref_rel_loc, a.ref_rel_rot = d->ref_rel_rot, a.world_loc = d->world_loc, a.world_rot = d->world_rot;
  a.initial_rel_rot = d->initial_rel_rot;
  a.bones = d->bones, a.root = d->root, a.final_rel_rot = d->final_rel_rot, a.out_rot = d->out_relative_pose_rot;
  a.B = d->B, a.T = d->T;
  a.vec_x = (reinterpret_cast<uintptr_t>(a.x) & 15) == 0;      // a frame is 208 bytes: every tile starts 16-byte aligned with x
  const bool scan = d->kind == P2C_KIND_POSE_CHANGES_6D;
  auto kernel = scan ? lift_kernel<P2C_KIND_POSE_CHANGES_6D> : lift_kernel<P2C_KIND_RELATIVE_ROT_6D>;
  static bool big_lds = false;
  if (!big_lds) {
    (void)hipFuncSetAttribute((const void *)lift_kernel<P2C_KIND_POSE_CHANGES_6D>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute((const void *)lift_kernel<P2C_KIND_RELATIVE_ROT_6D>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    big_lds = true;
  }
  const int cap = d->max_blocks > 0 && d->max_blocks < kMaxBlocks ? d->max_blocks : kMaxBlocks;
  const int grid = d->B < cap ? d->B : cap;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(NTH), (size_t)LDS_FLOATS * sizeof(float), (hipStream_t)stream, a);
  return p2c_host::launch_status();
}
