// p2c_root_motion.hip -- K40: root motion of a CARLA animation from its planted feet (gfx950).
//
// Definition: walker_control/root_motion.py (the reference has no counterpart: its only trajectory model is ZeroTrajectory, so an
// exported walker swings its legs on its spawn point). Per video n and global frame g = first_frame + t:
//   (l_j, R_j) = row_pose(bones[n, t, j]); (x_j, A_j) the forward kinematics over the 26-bone tree (row vectors);
//   (r, W) = row_pose(root[n, t]) (no root: r = 0, W = 1); p_k = x_{C_k} W + r for the contact candidates C = (foot R, toe R,
//   foot L, toe L) = bones (18, 19, 23, 24); h_k = -p_k[2], CARLA's world z.
//   g >= 1: m_k = max(h_k(g - 1), h_k(g)), s = the smallest k with minimal m_k, d = p_s(g - 1)[0:2] - p_s(g)[0:2],
//   step(g) = rint(d 2^10) as two int32, contact(g) = s; a non-finite height (of the eight) or coordinate (of the four), or
//   |d 2^10| >= 2^31: step = (0, 0), contact = -1. g == 0: step = (0, 0), contact = argmin_k h_k, -1 with a non-finite height.
//   S(g) = S(g - 1) + step(g) in int64: an integer sum, exact in any order, which is what lets the two mappings, every grid, every
//   tiling and every cut of a video give the same bits. No floating-point value is summed across frames.
//   out_root = (fp32(fp64(x) + S_x 2^-10), likewise y, z [+ (ground - min_k h_k(g)) with a ground plane], the angles bit for bit).
// Every height comparison is a comparison (never fminf / fmaxf) and every finiteness test explicit: a NaN is seen.
//
// Frame phase (both mappings). The 32-lanes-per-frame front end of p2c_carla_dev.h: a bone per lane reads its 24-byte row (the 26
// rows of a frame are one 624-byte span) and runs row_pose, K30's inverse; the spare lane does the same for the root row and keeps
// (r, W) aside, because for the tree walk it is the identity lane. fk_doubling (three rounds, DPP and ds_bpermute, registers only),
// then lane k < 4 of the group fetches x_{C_k} and all of (r, W) across lanes and writes p_k into the tile's LDS image: 13 floats
// a frame (12 used; the odd stride keeps the per-frame readers of the step phase on different banks).
//
// Mapping A (root_motion_video_kernel), a workgroup per video: the workgroup walks its tiles of kTile frames in order. Frame phase
// (eight frames at a time) -> barrier -> a lane per frame forms the step from image slots i (frame g - 1) and i + 1 (frame g) ->
// block-wide inclusive scan of the int64 pairs (six __shfl_up rounds inside a wavefront, the four wavefront totals through LDS,
// behind one barrier) -> the carry, held in registers by every lane, is added, the rows are written. The lane of the tile's last
// frame puts that frame's points into slot 0, the next tile's halo: each frame's kinematics runs once. Two barriers a tile.
// Mapping B, frame-parallel, for few long videos. Launch 1 (root_motion_steps_kernel) over (video, tile): the same two phases with
// the tile's one halo frame recomputed, steps, contact and lowest height to the workspace, the tile's int64 total behind them.
// Launch 2 (root_motion_rows_kernel) over (video, tile): sums the totals of the tiles before its own (lanes stride over them, one
// block reduction), redoes the in-tile scan from the stored steps, writes the rows. No atomics, no tickets, no look-back: the
// kernel boundary is the only hand-off. Both mappings run the same device functions on the same operands.
// LDS: (kTile + 1) * 13 floats + 8 int64 = 6.8 KB, static. Every slot that is read was written in the same tile (slot 0 is not read
// at g == 0); every workspace word launch 2 reads was written by launch 1.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "../../include/p2c.h"
#include "p2c_host.h"

#include "p2c_pose_head_dev.h"
#include "p2c_carla_dev.h"

namespace p2c_root_motion {

namespace ph = p2c;
namespace pc = p2c_carla;

constexpr int kThreads = pc::kFrameThreads;                 // 256: eight frame groups
constexpr int kGroups = kThreads / ph::GROUP;
constexpr int kTile = P2C_ROOT_MOTION_TILE;                 // frames of a tile: a lane per frame in the step phase
constexpr int kMaxBlocks = pc::kFrameMaxBlocks;
constexpr int kSlot = 13;                                   // floats of a frame in the image: 4 points of 3, one pad
constexpr int kResident = 256 * 4;                          // MI355X: 256 CUs, four of mapping A's workgroups each (111 VGPRs)
constexpr float kQuantum = 1024.0f;                         // steps per length unit: the quantum is 2^-10
constexpr int64_t kMaxCount = (int64_t)1 << 40;
static_assert(kTile <= kThreads && kTile % kGroups == 0, "a lane per frame of a tile");

// the contact candidates: crl_foot__R, crl_toe__R, crl_foot__L, crl_toe__L in CARLA_SKELETON order
static __constant__ int c_contact[4] = {18, 19, 23, 24};

struct I2 {
  long long x, y;
};

struct Args {
  const float *bones, *root, *in_points;
  const long long *in_offset;
  float *out_root, *out_points;
  int32_t *out_steps;
  int8_t *out_contact;
  long long *out_offset;
  long long *ws_totals;                                      // mapping B: (N, tiles, 2)
  int32_t *ws_steps;                                         //            (N, T, 2)
  float *ws_low;                                             //            (N, T): the lowest contact height of the frame
  int8_t *ws_contact;                                        //            (N, T)
  int64_t N, T, first_frame, tiles;
  float ground;
  int32_t has_ground;
};

struct Step {
  int32_t sx, sy, contact;
  float low;                                                 // min_k h_k(g); NaN when a height is not finite
};

__device__ __forceinline__ bool finite(float v) { return fabsf(v) <= 3.402823466e+38f; }   // false for a NaN

// ---- frame phase: the four contact points of frame (n, t) into `slot`, by the 32 lanes of one frame group
__device__ __forceinline__ void frame_points(const Args &a, const ph::LaneCtx &L, const pc::FrameLane &F, int64_t n, int64_t t,
                                             float *slot) {
  const int64_t f = n * a.T + t;
  ph::M3 R = ph::identity();
  ph::V3 l = ph::v3(0.f, 0.f, 0.f);
  const float *p = nullptr;
  if (F.bone) p = a.bones + (f * pc::kBones + F.j) * 6;
  if (F.spare && a.root) p = a.root + f * 6;
  if (p) {
    const float x = p[0], y = p[1], z = p[2], pitch = p[3], yaw = p[4], roll = p[5];
    float lv[3];
    pc::row_pose(x, y, z, pitch, yaw, roll, lv, R.m);
    l = ph::v3(lv[0], lv[1], lv[2]);
  }
  // the actor's transform leaves the spare lane before that lane becomes the identity of the tree walk
  const ph::M3 W = ph::shfl(R, L.base + pc::kSpare);
  const ph::V3 r = ph::shfl(l, L.base + pc::kSpare);
  if (!F.bone) R = ph::identity(), l = ph::v3(0.f, 0.f, 0.f);
  ph::fk_doubling<false>(L, R, l);
  const int k = F.j < 4 ? F.j : 0;
  const ph::V3 x = ph::shfl(l, L.base + c_contact[k]);
  const ph::V3 pk = ph::vmul(x, W) + r;
  if (F.j < 4) slot[k * 3 + 0] = pk.x, slot[k * 3 + 1] = pk.y, slot[k * 3 + 2] = pk.z;
}

// ---- step phase: one lane, one frame. prev / cur: the image slots of frames g - 1 and g; prev is not read at g == 0
__device__ __forceinline__ Step frame_step(const float *prev, const float *cur, bool first) {
  Step s;
  float c[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) c[i] = cur[i];
  bool ok = true;
  float low = -c[2];
  int at = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float h = -c[k * 3 + 2];
    ok = ok && finite(h);
    if (h < low) low = h, at = k;
  }
  s.low = ok ? low : __builtin_nanf("");
  s.sx = 0, s.sy = 0, s.contact = ok ? at : -1;
  if (first) return s;
  float q[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) q[i] = prev[i];
  float best = 0.f, px = 0.f, py = 0.f, cx = 0.f, cy = 0.f;
  at = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float hp = -q[k * 3 + 2], hc = -c[k * 3 + 2];
    ok = ok && finite(hp);
    const float m = hp > hc ? hp : hc;
    if (k == 0 || m < best) best = m, at = k, px = q[k * 3], py = q[k * 3 + 1], cx = c[k * 3], cy = c[k * 3 + 1];
  }
  ok = ok && finite(px) && finite(py) && finite(cx) && finite(cy);
  const float vx = (px - cx) * kQuantum, vy = (py - cy) * kQuantum;
  ok = ok && fabsf(vx) < 2147483648.0f && fabsf(vy) < 2147483648.0f;
  s.contact = ok ? at : -1;
  if (ok) s.sx = (int32_t)rintf(vx), s.sy = (int32_t)rintf(vy);
  return s;
}

// ---- inclusive scan of an int64 pair over the workgroup's kThreads lanes; `total` the sum over all of them. `tot`: 8 int64 of
// LDS, rewritten by the next call: a barrier lies between two calls (the callers' tile barrier)
__device__ __forceinline__ I2 block_scan(I2 v, long long *tot, I2 &total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const long long ox = __shfl_up(v.x, d, 64), oy = __shfl_up(v.y, d, 64);
    if (lane >= d) v.x += ox, v.y += oy;
  }
  if (lane == 63) tot[w * 2] = v.x, tot[w * 2 + 1] = v.y;
  __syncthreads();
  total = I2{0, 0};
#pragma unroll
  for (int k = 0; k < kThreads / 64; ++k) {
    const long long tx = tot[k * 2], ty = tot[k * 2 + 1];
    if (k < w) v.x += tx, v.y += ty;
    total.x += tx, total.y += ty;
  }
  return v;
}

// ---- the output row of frame (n, t) with offset S(g), and the frame's step and contact where they are asked for
__device__ __forceinline__ void write_frame(const Args &a, int64_t n, int64_t t, I2 S, int32_t sx, int32_t sy, int32_t contact,
                                            float low) {
  const int64_t f = n * a.T + t;
  float x = 0.f, y = 0.f, z = 0.f, pitch = 0.f, yaw = 0.f, roll = 0.f;
  if (a.root) {
    const float *p = a.root + f * 6;
    x = p[0], y = p[1], z = p[2], pitch = p[3], yaw = p[4], roll = p[5];
  }
  x = (float)((double)x + (double)S.x * 0x1p-10);
  y = (float)((double)y + (double)S.y * 0x1p-10);
  if (a.has_ground) z = z + (a.ground - low);
  float *o = a.out_root + f * 6;
  o[0] = x, o[1] = y, o[2] = z, o[3] = pitch, o[4] = yaw, o[5] = roll;
  if (a.out_steps) a.out_steps[f * 2] = sx, a.out_steps[f * 2 + 1] = sy;
  if (a.out_contact) a.out_contact[f] = (int8_t)contact;
}

__device__ __forceinline__ ph::LaneCtx tree_lane(const pc::FrameLane &F) {
  ph::LaneCtx L;
  L.lane = F.lane, L.j = F.j, L.base = F.base;
  L.anc0 = ph::c_parent[L.j], L.anc1 = ph::c_anc_r2[L.j], L.anc2 = ph::c_anc_r3[L.j];
  L.interior = (ph::kInteriorMask >> L.j) & 1u;
  return L;
}

// the carried points of video n into slot 0 (the frame before the first one given)
__device__ __forceinline__ void load_halo(const Args &a, int64_t n, float *pts) {
  if (threadIdx.x < 12) pts[threadIdx.x] = a.in_points[n * 12 + threadIdx.x];
}

__global__ __launch_bounds__(kThreads) void root_motion_video_kernel(const Args a) {
  __shared__ float pts[(kTile + 1) * kSlot];
  __shared__ long long tot[2 * kThreads / 64];
  const pc::FrameLane F = pc::frame_lane();
  const ph::LaneCtx L = tree_lane(F);
  const int tid = threadIdx.x, grp = tid >> 5;
  const bool continued = a.first_frame > 0;
  for (int64_t n = blockIdx.x; n < a.N; n += gridDim.x) {
    I2 carry{0, 0};
    if (continued) {
      carry = I2{a.in_offset[n * 2], a.in_offset[n * 2 + 1]};
      load_halo(a, n, pts);
    }
    for (int64_t t0 = 0; t0 < a.T; t0 += kTile) {
      const int fa = (int)(a.T - t0 < kTile ? a.T - t0 : kTile);
      for (int i = grp; i < fa; i += kGroups) frame_points(a, L, F, n, t0 + i, pts + (i + 1) * kSlot);
      __syncthreads();
      Step s{0, 0, -1, 0.f};
      float last[12] = {};
      if (tid < fa) {
        s = frame_step(pts + tid * kSlot, pts + (tid + 1) * kSlot, a.first_frame + t0 + tid == 0);
        if (tid == fa - 1) {
#pragma unroll
          for (int i = 0; i < 12; ++i) last[i] = pts[(tid + 1) * kSlot + i];
        }
      }
      I2 total;
      I2 S = block_scan(I2{s.sx, s.sy}, tot, total);          // its barrier: every read of the image lies before it
      S.x += carry.x, S.y += carry.y;
      carry.x += total.x, carry.y += total.y;
      if (tid < fa) write_frame(a, n, t0 + tid, S, s.sx, s.sy, s.contact, s.low);
      if (tid == fa - 1) {
#pragma unroll
        for (int i = 0; i < 12; ++i) pts[i] = last[i];        // the next tile's halo
        if (t0 + fa == a.T && a.out_offset) {
          a.out_offset[n * 2] = S.x, a.out_offset[n * 2 + 1] = S.y;
#pragma unroll
          for (int i = 0; i < 12; ++i) a.out_points[n * 12 + i] = last[i];
        }
      }
    }
    __syncthreads();                                           // slot 0 belongs to the next video
  }
}

__global__ __launch_bounds__(kThreads) void root_motion_steps_kernel(const Args a) {
  __shared__ float pts[(kTile + 1) * kSlot];
  __shared__ long long tot[2 * kThreads / 64];
  const pc::FrameLane F = pc::frame_lane();
  const ph::LaneCtx L = tree_lane(F);
  const int tid = threadIdx.x, grp = tid >> 5;
  const int64_t units = a.N * a.tiles;
  for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
    const int64_t n = u / a.tiles, t0 = (u - n * a.tiles) * kTile;
    const int fa = (int)(a.T - t0 < kTile ? a.T - t0 : kTile);
    if (t0 == 0 && a.first_frame > 0) load_halo(a, n, pts);
    for (int i = grp - 1; i < fa; i += kGroups) {              // i == -1: the tile's halo frame, recomputed
      if (i >= 0 || t0 > 0) frame_points(a, L, F, n, t0 + i, pts + (i + 1) * kSlot);
    }
    __syncthreads();
    Step s{0, 0, -1, 0.f};
    if (tid < fa) {
      s = frame_step(pts + tid * kSlot, pts + (tid + 1) * kSlot, a.first_frame + t0 + tid == 0);
      const int64_t f = n * a.T + t0 + tid;
      a.ws_steps[f * 2] = s.sx, a.ws_steps[f * 2 + 1] = s.sy;
      a.ws_low[f] = s.low;
      a.ws_contact[f] = (int8_t)s.contact;
      if (tid == fa - 1 && t0 + fa == a.T && a.out_points) {
#pragma unroll
        for (int i = 0; i < 12; ++i) a.out_points[n * 12 + i] = pts[(tid + 1) * kSlot + i];
      }
    }
    I2 total;
    block_scan(I2{s.sx, s.sy}, tot, total);
    if (tid == 0) a.ws_totals[u * 2] = total.x, a.ws_totals[u * 2 + 1] = total.y;
    __syncthreads();                                           // the image and the totals belong to the next unit
  }
}

__global__ __launch_bounds__(kThreads) void root_motion_rows_kernel(const Args a) {
  __shared__ long long tot[2 * kThreads / 64];
  const int tid = threadIdx.x;
  const int64_t units = a.N * a.tiles;
  for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
    const int64_t n = u / a.tiles, tile = u - n * a.tiles, t0 = tile * kTile;
    const int fa = (int)(a.T - t0 < kTile ? a.T - t0 : kTile);
    I2 part{0, 0};
    for (int64_t k = tid; k < tile; k += kThreads) {
      const long long *p = a.ws_totals + (n * a.tiles + k) * 2;
      part.x += p[0], part.y += p[1];
    }
    I2 before;
    block_scan(part, tot, before);
    if (a.first_frame > 0) before.x += a.in_offset[n * 2], before.y += a.in_offset[n * 2 + 1];
    __syncthreads();                                           // the totals of the first scan were read
    const int64_t f = n * a.T + t0 + tid;
    int32_t sx = 0, sy = 0;
    if (tid < fa) sx = a.ws_steps[f * 2], sy = a.ws_steps[f * 2 + 1];
    I2 total;
    I2 S = block_scan(I2{sx, sy}, tot, total);
    S.x += before.x, S.y += before.y;
    if (tid < fa) {
      write_frame(a, n, t0 + tid, S, sx, sy, a.ws_contact[f], a.ws_low[f]);
      if (tid == fa - 1 && t0 + fa == a.T && a.out_offset) a.out_offset[n * 2] = S.x, a.out_offset[n * 2 + 1] = S.y;
    }
    __syncthreads();                                           // the totals belong to the next unit
  }
}

static int64_t tiles_of(int64_t T) { return (T + kTile - 1) / kTile; }

// mapping = 0, as measured on the MI355X: A where a video is one tile (B's second launch buys nothing: 22 against 26 us
// at 256 x 16, 28 against 41 at 4 096 x 16) or where the videos alone fill every workgroup slot of the chip (146 against 156 us at
// 2 048 x 256, 292 against 306 at 1 024 x 1 024); B below that (30 against 42 us at 256 x 256, 76 against 161 at 256 x 1 024, 27
// against 2 507 at 1 x 16 384). Between 256 and 1 024 videos of several tiles the crossover was not measured.
static int resolve_mapping(int32_t mapping, int64_t N, int64_t T) {
  if (mapping != P2C_ROOT_MOTION_AUTO) return mapping;
  return N >= kResident || T <= kTile ? P2C_ROOT_MOTION_PER_VIDEO : P2C_ROOT_MOTION_FRAME_PARALLEL;
}

static bool sizes_ok(int64_t N, int64_t T) {
  return N >= 0 && T >= 0 && N <= kMaxCount && T <= kMaxCount && !(N > 0 && T > 0 && N > kMaxCount / T / (pc::kBones + 1));
}

static int64_t round16(int64_t v) { return (v + 15) / 16 * 16; }

}  // namespace p2c_root_motion

using namespace p2c_root_motion;

extern "C" int32_t p2c_carla_root_motion_tile(void) { return kTile; }

extern "C" int64_t p2c_carla_root_motion_workspace(int64_t N, int64_t T, int32_t mapping) {
  if (!sizes_ok(N, T) || mapping < P2C_ROOT_MOTION_AUTO || mapping > P2C_ROOT_MOTION_FRAME_PARALLEL) return -1;
  if (N == 0 || T == 0 || resolve_mapping(mapping, N, T) == P2C_ROOT_MOTION_PER_VIDEO) return 0;
  // totals (N, tiles, 2) int64 | steps (N, T, 2) int32 | lowest height (N, T) fp32 | contact (N, T) int8, each 16-byte aligned
  return round16(N * tiles_of(T) * 16) + round16(N * T * 8) + round16(N * T * 4) + round16(N * T);
}

extern "C" int p2c_carla_root_motion_fwd(const float *bones, const float *root, const int64_t *state_in_offset,
                                         const float *state_in_points, float *out_root, int32_t *out_steps, int8_t *out_contact,
                                         int64_t *state_out_offset, float *state_out_points, int64_t N, int64_t T,
                                         int64_t first_frame, double ground, int32_t has_ground, int32_t mapping,
                                         int32_t max_blocks, void *workspace, void *stream) {
  if (!sizes_ok(N, T) || first_frame < 0 || first_frame > kMaxCount - T || max_blocks < 0 || (has_ground != 0 && has_ground != 1))
    return P2C_E_SHAPE;
  if (has_ground && !(std::isfinite(ground) && std::isfinite((double)(float)ground))) return P2C_E_SHAPE;
  if (mapping < P2C_ROOT_MOTION_AUTO || mapping > P2C_ROOT_MOTION_FRAME_PARALLEL) return P2C_E_ENUM;
  if (!bones || !out_root) return P2C_E_NULL;
  if ((state_in_offset == nullptr) != (state_in_points == nullptr)) return P2C_E_NULL;      // both or neither
  if ((state_out_offset == nullptr) != (state_out_points == nullptr)) return P2C_E_NULL;
  if (first_frame > 0 && !state_in_offset) return P2C_E_NULL;                               // frames that continue a video
  const int map = resolve_mapping(mapping, N, T);
  if (map == P2C_ROOT_MOTION_FRAME_PARALLEL && N > 0 && T > 0 && !workspace) return P2C_E_NULL;
  if (N == 0 || T == 0) return 0;
  Args a{};
  a.bones = bones, a.root = root, a.out_root = out_root, a.out_steps = out_steps, a.out_contact = out_contact;
  a.in_offset = (const long long *)state_in_offset, a.in_points = state_in_points;           // read with first_frame > 0 only
  a.out_offset = (long long *)state_out_offset, a.out_points = state_out_points;
  a.N = N, a.T = T, a.first_frame = first_frame, a.tiles = tiles_of(T);
  a.ground = has_ground ? (float)ground : 0.f, a.has_ground = has_ground;
  if (map == P2C_ROOT_MOTION_PER_VIDEO) {
    const unsigned grid = p2c_host::grid_for(N, max_blocks, kMaxBlocks);
    hipLaunchKernelGGL(root_motion_video_kernel, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, a);
    return p2c_host::launch_status();
  }
  char *ws = (char *)workspace;
  a.ws_totals = (long long *)ws, ws += round16(N * a.tiles * 16);
  a.ws_steps = (int32_t *)ws, ws += round16(N * T * 8);
  a.ws_low = (float *)ws, ws += round16(N * T * 4);
  a.ws_contact = (int8_t *)ws;
  const unsigned grid = p2c_host::grid_for(N * a.tiles, max_blocks, kMaxBlocks);
  hipLaunchKernelGGL(root_motion_steps_kernel, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, a);
  const int rc = p2c_host::launch_status();
  if (rc) return rc;
  hipLaunchKernelGGL(root_motion_rows_kernel, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, a);
  return p2c_host::launch_status();
}
