// p2c_generate.hip -- K38: Carla2D3D training batches generated on the device in one launch (gfx950).
//
// Reference: Carla2D3DIterableDataset.generate_batch (data/carla/datasets/carla_2d3d_dataset.py:145-210): per frame k random joints
// are turned by U(-max, max) per Euler axis, the world yaws, the changes go through the projection layer
// (modules/layers/projection.py) and the result through Projection2DMixin.process_projection_2d (deform + two normalisations).
// The random part is defined once, in data/carla/generator.py (key schedule, element layout, what is made of a word); this file
// restates it on the device and must equal it to the bit. Per clip n, frame t, bone j:
//   C[t][j] = Rx Ry Rz of the joint's angles (identity when the joint is not picked);  rel[t] = C[t] @ rel[t-1], rel[-1] = the
//   clip's ref_rel_rot row (oracle/pose_head.py:319-321);  abs = forward kinematics of (ref_rel_loc, rel[t]);
//   wrot[t] = wrot[t-1] @ Rz(yaw[t]) (only with a world parameter set: else the identity, and no multiply);
//   projection_2d = the pinhole projection of the pose head (project_joint, p2c_pose_head_dev.h);  projection_2d_deformed = + noise, (0, 0) where
//   miss_u < miss_prob[j];  frames = normalise(deformed);  projection_2d_transformed, shift, scale = normalise(projection_2d).
//
// Mapping. The frame group of p2c_carla_dev.h (a bone per lane, 32 lanes, two groups per wavefront, eight per workgroup); groups
// stride over work items (grid capped at kFrameMaxBlocks, max_blocks lowers the cap). Two mappings, one loop:
//   sequential      an item is a clip: the group walks t = 0 .. T-1, carrying rel and wrot, and writes every frame;
//   frame parallel  an item is a (clip, frame): the group replays the draws and the running products of frames 0 .. t (no
//                   forward kinematics, no stores) and writes frame t only. O(T^2) cheap work that fills the machine at small B.
// Both run the same instructions on the same values for a frame they write, so they give the same bits.
//   * No LDS, no atomics, no barrier: the pick rank is 26 readlane pairs, the tree walk fk_doubling, the normaliser shuffles.
//   * The only HBM reads are a bone's 12 reference floats per item (8.7 KB of tables in all: cache resident).
//   * Every output is optional, written behind a wave-uniform test by one lane per element; what is computed does not depend on
//     what is asked for, except that the forward kinematics and everything behind it run only when something behind them is wanted
//     (they feed nothing that comes before).
//   * Clip and frame indices are 64-bit; the element counter of a clip is 32-bit (T <= 2^16).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/p2c.h"
#include "p2c_host.h"

#include "p2c_pose_head_dev.h"
#include "p2c_carla_dev.h"
#include "p2c_collate_dev.h"
#include "p2c_rec_dev.h"

namespace p2c_generate {

namespace ph = p2c;
namespace pc = p2c_carla;
namespace co = p2c_collate;
using p2c_rec::mix32;
constexpr int J = ph::J;
constexpr int kGroupsPerBlock = pc::kFrameThreads / ph::GROUP;
constexpr uint32_t kPhi = 0x9E3779B1u, kClipWord = 0xFFFFFFFFu;
constexpr int kYawSlot = 31;
enum { CH_PICK = 0, CH_X, CH_Y, CH_Z, CH_MISS, CH_NOISE_X, CH_NOISE_Y };
constexpr int kHips = 1, kNeck = 8;      // CARLA_SKELETON.crl_hips__C, crl_neck__C

struct Args {
  const float *ref_rel_loc, *ref_rel_rot;
  float *frames, *proj, *deformed, *transformed, *shift, *scale, *pose_changes, *rel_loc, *rel_rot, *abs_loc, *abs_rot;
  float *world_loc, *world_rot, *world_loc_changes, *world_rot_changes;
  int32_t *skel_type;
  int64_t B, first_clip, items;
  int32_t T, k, transform, noise, has_miss, frame_parallel, world_on;
  uint32_t k0, k1;
  float max_change, max_world, max_initial, noise_param, near_zero;
  float cam_f, cam_cx, cam_cy, cam_dist, cam_elev;
  float miss_prob[ph::GROUP];
};

struct ClipKeys {
  uint32_t c0, c1;
};
__device__ __forceinline__ ClipKeys clip_keys(const Args &a, int64_t n) {
  const uint32_t n_lo = (uint32_t)((uint64_t)n & 0xFFFFFFFFull), n_hi = (uint32_t)((uint64_t)n >> 32);
  const uint32_t x = mix32(n_lo ^ a.k0), b = mix32(x + n_hi);
  ClipKeys c;
  c.c0 = mix32(b ^ a.k1);
  c.c1 = mix32(c.c0 + x + 0x85EBCA6Bu);
  return c;
}
__device__ __forceinline__ uint32_t word(const ClipKeys &c, uint32_t e) { return mix32(mix32(c.c0 + e * kPhi) + c.c1); }
__device__ __forceinline__ float uniform(uint32_t w) { return (float)(w >> 8) * 5.9604644775390625e-08f; }   // 2^-24: exact
// The definition rounds after every operation. Contraction is off in these two, so that the product is rounded before anything
// consumes it: the compiler otherwise fuses u * p - p / 2 into one fma (one ulp off the definition in about 1 value of 50).
__device__ __forceinline__ float signed_draw(uint32_t w, float amplitude) {
#pragma clang fp contract(off)
  const float centred = fmaf(uniform(w), 2.0f, -1.0f);                   // 2u - 1 is exact: one rounding
  return centred * amplitude;
}
__device__ __forceinline__ float noise_draw(uint32_t w, float noise_param) {
#pragma clang fp contract(off)
  const float scaled = uniform(w) * noise_param;
  return scaled - noise_param / 2.0f;
}

// Rx Ry Rz of (a0, a1, a2): the closed form of carla_pose_inv_kernel and K35
__device__ __forceinline__ ph::M3 euler_xyz(float a0, float a1, float a2) {
  float s0, c0, s1, c1, s2, c2;
  sincosf(a0, &s0, &c0);
  sincosf(a1, &s1, &c1);
  sincosf(a2, &s2, &c2);
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
  return M;
}

__device__ __forceinline__ void store3(float *base, size_t idx, float x, float y, float z) {
  float *o = base + idx * 3;
  o[0] = x, o[1] = y, o[2] = z;
}

__global__ __launch_bounds__(pc::kFrameThreads) void generate_kernel(const Args a) {
  const pc::FrameLane F = pc::frame_lane();
  ph::LaneCtx L;
  L.lane = F.lane, L.j = F.j, L.base = F.base;
  L.anc0 = ph::c_parent[L.j], L.anc1 = ph::c_anc_r2[L.j], L.anc2 = ph::c_anc_r3[L.j];
  L.interior = (ph::kInteriorMask >> L.j) & 1u;
  const bool bone = F.bone, upper = F.base != 0;
  const float mp = a.miss_prob[F.j];
  const bool want_2d = a.frames || a.proj || a.deformed || a.transformed || a.shift || a.scale;
  const bool want_fk = want_2d || a.abs_loc || a.abs_rot;
  const bool want_world = a.world_loc || a.world_rot || a.world_loc_changes || a.world_rot_changes;

  co::View v{};
  v.Jd = v.Jn = J, v.C = 2, v.transform = a.transform, v.n_hips = v.n_neck = 1;
  v.hips_idx[0] = v.hips_idx[1] = kHips, v.neck_idx[0] = v.neck_idx[1] = kNeck;

  const int64_t step = (int64_t)gridDim.x * kGroupsPerBlock;
  for (int64_t it0 = (int64_t)blockIdx.x * kGroupsPerBlock; it0 < a.items; it0 += step) {
    // the trip count is a workgroup's, not a group's: a group past the last item goes through the motions of the last one (its
    // shuffles stay defined) and stores nothing
    const int64_t mine = it0 + (threadIdx.x >> 5);
    const bool live = mine < a.items;
    const int64_t item = live ? mine : a.items - 1;
    int64_t n = item;
    int t_emit = -1, t_last = a.T - 1;              // sequential: every frame is written
    if (a.frame_parallel) {
      n = item <= 0xffffffffll ? (int64_t)((uint32_t)item / (uint32_t)a.T) : item / a.T;
      t_emit = t_last = (int)(item - n * a.T);
    }
    const ClipKeys ck = clip_keys(a, a.first_clip + n);
    int st = (int)(word(ck, kClipWord) >> 30);
    if (live && a.skel_type && F.j == 0 && (t_emit <= 0)) a.skel_type[n] = st;
    const size_t row = (size_t)st * J + F.jb;
    ph::M3 R;
    ph::V3 l0;
    pc::load_ref(a.ref_rel_rot, a.ref_rel_loc, row, R.m, l0.x, l0.y, l0.z);
    ph::M3 W = ph::identity();

    // both halves of a wavefront walk the same number of frames: the longer of the two (the cross-lane steps need every lane)
    const int t_other = __shfl_xor(t_last, 32, 64);
    const int t_walk = t_last > t_other ? t_last : t_other;
    for (int t = 0; t <= t_walk; ++t) {
      const bool emit = live && t <= t_last && (t_emit < 0 || t == t_emit);
      const uint32_t e = (uint32_t)t * 256u + (uint32_t)F.j * 8u;
      // ---- draws: which joints change, by how much ----
      bool picked = a.k >= J;
      if (a.k > 0 && a.k < J) {
        const uint32_t key = bone ? ((word(ck, e + CH_PICK) & 0xFFFFFFE0u) | (uint32_t)F.j) : 0xFFFFFFFFu;
        int rank = 0;
#pragma unroll
        for (int i = 0; i < J; ++i) {
          const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)key, i), hi = (uint32_t)__builtin_amdgcn_readlane((int)key, i + 32);
          rank += ((upper ? hi : lo) < key) ? 1 : 0;
        }
        picked = rank < a.k;
      }
      picked = picked && bone;
      const float a0 = picked ? signed_draw(word(ck, e + CH_X), a.max_change) : 0.f;
      const float a1 = picked ? signed_draw(word(ck, e + CH_Y), a.max_change) : 0.f;
      const float a2 = picked ? signed_draw(word(ck, e + CH_Z), a.max_change) : 0.f;
      const ph::M3 C = euler_xyz(a0, a1, a2);
      if (t <= t_last) R = ph::mul(C, R);
      // ---- world: only the yaw changes (wave-uniform per group, computed by every lane) ----
      ph::M3 dW = ph::identity();
      if (a.world_on) {
        const float amp = t == 0 ? (a.max_initial > 0.f ? a.max_initial : 0.f) : a.max_world;
        const float yaw = amp != 0.f ? signed_draw(word(ck, (uint32_t)t * 256u + (uint32_t)kYawSlot * 8u), amp) : 0.f;
        float sn, cs;
        sincosf(yaw, &sn, &cs);
        dW.m[0] = cs, dW.m[1] = -sn, dW.m[3] = sn, dW.m[4] = cs;
        if (t <= t_last) W = ph::mul(W, dW);
      }
      if (a.frame_parallel && t < t_walk && __all(t != t_last)) continue;       // nothing of this frame is written by this wavefront

      const size_t frame = (size_t)n * a.T + (size_t)(t <= t_last ? t : t_last);
      const size_t o = frame * J + F.j;
      if (emit && bone) {
        if (a.pose_changes) ph::store_m3(a.pose_changes, o, C);
        if (a.rel_rot) ph::store_m3(a.rel_rot, o, R);
        if (a.rel_loc) store3(a.rel_loc, o, l0.x, l0.y, l0.z);
      }
      if (emit && F.spare && want_world) {
        if (a.world_rot) ph::store_m3(a.world_rot, frame, W);
        if (a.world_rot_changes) ph::store_m3(a.world_rot_changes, frame, dW);
        if (a.world_loc) store3(a.world_loc, frame, 0.f, 0.f, 0.f);
        if (a.world_loc_changes) store3(a.world_loc_changes, frame, 0.f, 0.f, 0.f);
      }
      if (!want_fk) continue;

      // ---- forward kinematics over the group ----
      ph::M3 A = bone ? R : ph::identity();
      ph::V3 x = bone ? l0 : ph::v3(0.f, 0.f, 0.f);
      ph::fk_doubling(L, A, x);
      if (emit && bone) {
        if (a.abs_rot) ph::store_m3(a.abs_rot, o, A);
        if (a.abs_loc) store3(a.abs_loc, o, x.x, x.y, x.z);
      }
      if (!want_2d) continue;

      // ---- projection: frame_head's own (project_joint, p2c_pose_head_dev.h); the world does not move ----
      ph::World Wd;
      Wd.rot = W, Wd.loc = ph::v3(0.f, 0.f, 0.f), Wd.on = a.world_on != 0;
      ph::V3 p;
      float invZ, pu, pv;
      ph::project_joint(a, x, Wd, p, invZ, pu, pv);
      if (!bone) { pu = 0.f; pv = 0.f; }

      // ---- apply_deform, apply_transform twice: the tail of collate_frame (p2c_collate.hip) ----
      float dx = pu, dy = pv;
      if (bone) {
        if (a.noise) {
          dx += noise_draw(word(ck, e + CH_NOISE_X), a.noise_param);
          dy += noise_draw(word(ck, e + CH_NOISE_Y), a.noise_param);
        }
        if (a.has_miss && uniform(word(ck, e + CH_MISS)) < mp) dx = 0.f, dy = 0.f;
      }
      float ix = dx, iy = dy, ic = 0.f, tx = pu, ty = pv, s[2] = {0.f, 0.f}, scale = 1.f;
      if (a.transform != P2C_TRANSFORM_NONE) {
        float s0[2], sc0, tc;
        co::normalise<32>(v, a.near_zero, F.base, bone, dx, dy, 0.f, ix, iy, ic, s0, sc0);
        co::normalise<32>(v, a.near_zero, F.base, bone, pu, pv, 0.f, tx, ty, tc, s, scale);
      }
      if (!emit) continue;
      if (F.j == 0) {
        if (a.shift) a.shift[frame * 2] = s[0], a.shift[frame * 2 + 1] = s[1];
        if (a.scale) a.scale[frame] = scale;
      }
      if (!bone) continue;
      if (a.frames) a.frames[2 * o] = ix, a.frames[2 * o + 1] = iy;
      if (a.proj) a.proj[2 * o] = pu, a.proj[2 * o + 1] = pv;
      if (a.deformed) a.deformed[2 * o] = dx, a.deformed[2 * o + 1] = dy;
      if (a.transformed) a.transformed[2 * o] = tx, a.transformed[2 * o + 1] = ty;
    }
  }
}

// the launch keys of data/carla/generator.py
inline uint32_t host_mix32(uint32_t x) {
  x ^= x >> 16, x *= 0x7feb352du;
  x ^= x >> 15, x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

}  // namespace p2c_generate

using namespace p2c_generate;

extern "C" int p2c_carla_generate_fwd(int64_t seed, int32_t draw_stream, int64_t first_clip, int64_t B, int32_t T,
                                      int32_t random_changes_each_frame, float max_change_rad, float max_world_rot_change_rad,
                                      float max_initial_world_rot_change_rad, int32_t transform, int32_t noise, float noise_param,
                                      const float *miss_prob, float near_zero, const float *camera, const float *ref_rel_loc,
                                      const float *ref_rel_rot, float *frames, float *projection_2d, float *projection_2d_deformed,
                                      float *projection_2d_transformed, float *projection_2d_shift, float *projection_2d_scale,
                                      float *pose_changes, float *relative_pose_loc, float *relative_pose_rot,
                                      float *absolute_pose_loc, float *absolute_pose_rot, float *world_loc, float *world_rot,
                                      float *world_loc_changes, float *world_rot_changes, int32_t *skel_type, int32_t mapping,
                                      int32_t max_blocks, void *stream) {
  if (B < 0 || T < 1 || T > P2C_GENERATE_MAX_T || first_clip < 0 || B > ((int64_t)1 << 40) / T ||
      first_clip > INT64_MAX - B || random_changes_each_frame < 0 || random_changes_each_frame > J || max_blocks < 0)
    return P2C_E_SHAPE;
  if (transform < P2C_TRANSFORM_NONE || transform > P2C_TRANSFORM_HIPS_NECK_BBOX || noise < P2C_GENERATE_NOISE_ZERO ||
      noise > P2C_GENERATE_NOISE_UNIFORM || mapping < P2C_GENERATE_AUTO || mapping > P2C_GENERATE_FRAME_PARALLEL)
    return P2C_E_ENUM;
  if ((projection_2d_transformed || projection_2d_shift || projection_2d_scale) && transform == P2C_TRANSFORM_NONE) return P2C_E_ENUM;
  if (!camera || !ref_rel_loc || !ref_rel_rot) return P2C_E_NULL;
  if (!(frames || projection_2d || projection_2d_deformed || projection_2d_transformed || projection_2d_shift ||
        projection_2d_scale || pose_changes || relative_pose_loc || relative_pose_rot || absolute_pose_loc || absolute_pose_rot ||
        world_loc || world_rot || world_loc_changes || world_rot_changes || skel_type))
    return P2C_E_NULL;
  if (B == 0) return 0;
  Args a{};
  a.ref_rel_loc = ref_rel_loc, a.ref_rel_rot = ref_rel_rot;
  a.frames = frames, a.proj = projection_2d, a.deformed = projection_2d_deformed, a.transformed = projection_2d_transformed;
  a.shift = projection_2d_shift, a.scale = projection_2d_scale, a.pose_changes = pose_changes;
  a.rel_loc = relative_pose_loc, a.rel_rot = relative_pose_rot, a.abs_loc = absolute_pose_loc, a.abs_rot = absolute_pose_rot;
  a.world_loc = world_loc, a.world_rot = world_rot, a.world_loc_changes = world_loc_changes, a.world_rot_changes = world_rot_changes;
  a.skel_type = skel_type;
  a.B = B, a.first_clip = first_clip, a.T = T, a.k = random_changes_each_frame, a.transform = transform;
  a.noise = noise == P2C_GENERATE_NOISE_UNIFORM;
  a.frame_parallel = mapping == P2C_GENERATE_AUTO ? (B * T <= P2C_GENERATE_FRAME_PARALLEL_MAX_FRAMES)
                                                  : (mapping == P2C_GENERATE_FRAME_PARALLEL);
  a.items = a.frame_parallel ? B * T : B;
  a.world_on = max_world_rot_change_rad != 0.f || max_initial_world_rot_change_rad != 0.f;
  {
    const uint64_t s = (uint64_t)seed;
    const uint32_t lo = (uint32_t)(s & 0xFFFFFFFFull), hi = (uint32_t)(s >> 32), st = (uint32_t)draw_stream;
    a.k0 = host_mix32(host_mix32(host_mix32(lo + 0x9E3779B9u) ^ hi) + st * 0x632BE59Bu);
    a.k1 = host_mix32(host_mix32(host_mix32(hi + 0x85EBCA6Bu) ^ st) + lo * 0xC2B2AE35u);
  }
  a.max_change = max_change_rad, a.max_world = max_world_rot_change_rad, a.max_initial = max_initial_world_rot_change_rad;
  a.noise_param = noise_param, a.near_zero = near_zero;
  a.cam_f = camera[0], a.cam_cx = camera[1], a.cam_cy = camera[2], a.cam_dist = camera[3], a.cam_elev = camera[4];
  for (int j = 0; j < ph::GROUP; ++j) a.miss_prob[j] = (miss_prob && j < J) ? miss_prob[j] : 0.f;
  a.has_miss = miss_prob != nullptr;
  const unsigned grid = p2c_host::grid_for((a.items + kGroupsPerBlock - 1) / kGroupsPerBlock, max_blocks, pc::kFrameMaxBlocks);
  hipLaunchKernelGGL(generate_kernel, dim3(grid), dim3(pc::kFrameThreads), 0, (hipStream_t)stream, a);
  return p2c_host::launch_status();
}
