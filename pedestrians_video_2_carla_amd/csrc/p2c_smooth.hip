// p2c_smooth.hip -- K39: CARLA rows smoothed along time, one launch for the bones and root of a batch (gfx950).
//
// Definition: walker_control/smooth.py (the reference has no counterpart: its players show every frame as it was predicted).
// Rows are (x, y, z, pitch, yaw, roll); rotations are handled as the unit quaternions row_quat makes of them (K37's), never as
// Euler angles, and written back through carla_row on the five matrix entries it reads. Every comparison lets a NaN through.
//
// Gaussian (p2c_carla_smooth_gauss_fwd): output frame t (a global index, counted from the start of the video) combines the source
// frames max(0, t - R) .. min(t + R, last_frame) with weights[|g - t|]: locations sum(w x) / sum(w), rotations the normalised sum
// of the neighbours' quaternions, each negated when its dot product with the centre frame's is < 0; all sums in ascending frame
// order. R == 0 copies the rows.
// Mapping: a workgroup takes a unit = (video, tile of up to F output frames, chunk of up to kRows rows of a frame; the root is row
// J). It converts the rows of the tile's F + 2R source frames ONCE into (loc 3, quat 4) in LDS -- 7 floats a row, an odd stride,
// so the lanes of a wavefront fall into different banks -- barriers, and each lane then forms output rows from LDS: 2R + 1 reads
// of 7 floats instead of 2R + 1 conversions (three sincosf each). F = min(32, what 64 KB hold - 2R): 22 at R = 32 with 27 rows.
// The image is written for exactly the frames [s_lo, s_hi] the tile's windows read, and a window is clamped into them: tiles at
// the ends of a video read nothing that was not written. A row's bits depend on its window's source rows and the table only:
// the sequence of operations is the same in every tile, grid, chunk and cut of the video. One writer per element, no atomics.
//
// One-euro (p2c_carla_smooth_euro_fwd): a causal low-pass whose cutoff grows with the filtered speed, sequential along time. One
// lane per (video, row) chain walks its T frames with the state (x^ 3, v^ 3, q^ 4, w^ 1; 12 floats with the pad) in registers;
// neighbouring lanes are neighbouring rows of the same frame, so the fetched lines are used whole, and the next frame's row is
// requested before this frame's arithmetic. No LDS, no atomics. The constants alpha(d_cutoff) and fps / 2 pi are formed on the
// host in fp64 and rounded once, as the definition forms them.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <initializer_list>

#include "../../include/p2c.h"
#include "p2c_host.h"

#include "p2c_carla_dev.h"   // carla_row, row_quat

namespace p2c_smooth {

using p2c_carla::carla_row;
using p2c_carla::row_quat;

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;
constexpr int kRows = 27;                         // rows of a frame to a unit: the 26 bones and the root
constexpr int kMaxTile = 32;                      // output frames to a unit at the most
constexpr int kTable = P2C_SMOOTH_MAX_RADIUS + 1;
constexpr int kLdsFloats = 64 * 1024 / 4 - kTable - 7;   // the image; the table sits behind it
constexpr int kEuroThreads = 64;
constexpr int kEuroMaxBlocks = 8192;

// q (w, x, y, z), unit -> the five matrix entries carla_row reads, and the row; z is a stored value (carla_row negates it)
__device__ __forceinline__ void quat_row(float lx, float ly, float lz, float w, float x, float y, float z, float *o) {
  const float r00 = 1.0f - 2.0f * (y * y + z * z), r01 = 2.0f * (x * y - w * z), r02 = 2.0f * (x * z + w * y);
  const float r12 = 2.0f * (y * z - w * x), r22 = 1.0f - 2.0f * (x * x + y * y);
  carla_row(lx, ly, -lz, r00, r01, r02, r12, r22, o);
}

struct GaussArgs {
  const float *bones, *root, *weights;
  float *out_bones, *out_root;
  int64_t S, K, first_frame, first_output, hi_all;   // hi_all: the last source frame a window may read
  int64_t tiles, chunks, units;
  int32_t J, W, R, F, rows;                          // W = J + root rows of a frame, rows = min(W, kRows) of a unit
};

__device__ __forceinline__ const float *src_row(const GaussArgs &a, int64_t n, int64_t g, int r) {
  const int64_t f = n * a.S + (g - a.first_frame);
  return r < a.J ? a.bones + (f * a.J + r) * 6 : a.root + f * 6;
}
__device__ __forceinline__ float *dst_row(const GaussArgs &a, int64_t n, int64_t k, int r) {
  const int64_t f = n * a.K + k;
  return r < a.J ? a.out_bones + (f * a.J + r) * 6 : a.out_root + f * 6;
}

__global__ __launch_bounds__(kThreads) void carla_smooth_gauss_kernel(GaussArgs a) {
  extern __shared__ float lds[];
  const int tid = threadIdx.x;
  float *table = lds + (a.F + 2 * a.R) * a.rows * 7;
  if (a.R > 0 && tid <= a.R) table[tid] = a.weights[tid];            // read after the first barrier only
  for (int64_t u = blockIdx.x; u < a.units; u += gridDim.x) {
    const int64_t per_video = a.tiles * a.chunks;
    const int64_t n = u / per_video, rest = u - n * per_video;
    const int64_t tile = rest / a.chunks;
    const int r0 = (int)(rest - tile * a.chunks) * kRows;
    const int rows = a.W - r0 < a.rows ? a.W - r0 : a.rows;
    const int64_t k0 = tile * a.F;                                     // the tile's first output, counted from first_output
    const int fa = (int)(a.K - k0 < a.F ? a.K - k0 : a.F);
    const int64_t t0 = a.first_output + k0;
    const int64_t last_src = a.first_frame + a.S - 1;
    const int64_t hi_all = a.hi_all < last_src ? a.hi_all : last_src;
    if (a.R == 0) {                                                    // copies; a frame outside the given ones is clamped
      for (int i = tid; i < fa * rows; i += kThreads) {
        const int fo = i / rows, r = r0 + i - fo * rows;
        int64_t g = t0 + fo;
        g = g < a.first_frame ? a.first_frame : (g > last_src ? last_src : g);
        const float *p = src_row(a, n, g, r);
        float *o = dst_row(a, n, k0 + fo, r);
        const float v0 = p[0], v1 = p[1], v2 = p[2], v3 = p[3], v4 = p[4], v5 = p[5];
        o[0] = v0, o[1] = v1, o[2] = v2, o[3] = v3, o[4] = v4, o[5] = v5;
      }
      continue;
    }
    // the source frames the tile's windows read: [s_lo, s_hi], at most fa + 2R of them, all inside the given frames
    const int64_t s_lo = t0 - a.R > a.first_frame ? t0 - a.R : a.first_frame;
    const int64_t s_hi = t0 + fa - 1 + a.R < hi_all ? t0 + fa - 1 + a.R : hi_all;
    const int ns = s_hi >= s_lo ? (int)(s_hi - s_lo + 1) : 0;
    for (int i = tid; i < ns * rows; i += kThreads) {
      const int f = i / rows, rr = i - f * rows;
      const float *p = src_row(a, n, s_lo + f, r0 + rr);
      const float x = p[0], y = p[1], z = p[2], pitch = p[3], yaw = p[4], roll = p[5];
      float qw, qx, qy, qz;
      row_quat(pitch, yaw, roll, qw, qx, qy, qz);
      float *l = lds + i * 7;
      l[0] = x, l[1] = y, l[2] = z, l[3] = qw, l[4] = qx, l[5] = qy, l[6] = qz;
    }
    __syncthreads();
    for (int i = tid; i < fa * rows; i += kThreads) {
      const int fo = i / rows, rr = i - fo * rows;
      const int64_t t = t0 + fo;
      float *o = dst_row(a, n, k0 + fo, r0 + rr);
      const int64_t w_lo = t - a.R > s_lo ? t - a.R : s_lo, w_hi = t + a.R < s_hi ? t + a.R : s_hi;
      if (t < s_lo || t > s_hi) {                                      // the centre frame is not given: the caller's mistake
        const float nan = __builtin_nanf("");
        o[0] = nan, o[1] = nan, o[2] = nan, o[3] = nan, o[4] = nan, o[5] = nan;
        continue;
      }
      const float *c = lds + ((int)(t - s_lo) * rows + rr) * 7;
      const float cw = c[3], cx = c[4], cy = c[5], cz = c[6];
      float sx = 0.0f, sy = 0.0f, sz = 0.0f, sw = 0.0f, aw = 0.0f, ax = 0.0f, ay = 0.0f, az = 0.0f;
      for (int64_t g = w_lo; g <= w_hi; ++g) {
        const int d = (int)(g - t);
        const float w = table[d < 0 ? -d : d];
        const float *l = lds + ((int)(g - s_lo) * rows + rr) * 7;
        const float qw = l[3], qx = l[4], qy = l[5], qz = l[6];
        const float dot = qw * cw + qx * cx + qy * cy + qz * cz;
        const float ws = dot < 0.0f ? -w : w;                         // the neighbour on the centre's hemisphere
        sx += w * l[0], sy += w * l[1], sz += w * l[2], sw += w;
        aw += ws * qw, ax += ws * qx, ay += ws * qy, az += ws * qz;
      }
      const float rn = 1.0f / sqrtf(aw * aw + ax * ax + ay * ay + az * az);
      quat_row(sx / sw, sy / sw, sz / sw, aw * rn, ax * rn, ay * rn, az * rn, o);
    }
    __syncthreads();                                                   // the next unit overwrites the image
  }
}

struct EuroArgs {
  const float *bones, *root;
  float *state_bones, *state_root, *out_bones, *out_root;
  int64_t T, chains;
  int32_t J, W, has_state;
  float fps, min_cutoff, beta_loc, beta_rot, alpha_d, k;   // k = fps / 2 pi: alpha(fc) = 1 / (1 + k / fc)
};

__global__ __launch_bounds__(kEuroThreads) void carla_smooth_euro_kernel(EuroArgs a) {
  const int64_t step = (int64_t)gridDim.x * kEuroThreads;
  for (int64_t e = (int64_t)blockIdx.x * kEuroThreads + threadIdx.x; e < a.chains; e += step) {
    const int64_t n = e / a.W;
    const int r = (int)(e - n * a.W);
    const bool is_root = r >= a.J;
    const int64_t stride = is_root ? 6 : (int64_t)a.J * 6;             // floats from a frame's row to the next frame's
    const int64_t first = is_root ? n * a.T * 6 : (n * a.T * a.J + r) * 6;
    const float *src = (is_root ? a.root : a.bones) + first;
    float *dst = (is_root ? a.out_root : a.out_bones) + first;
    float *state = is_root ? (a.state_root ? a.state_root + n * 12 : nullptr)
                           : (a.state_bones ? a.state_bones + (n * a.J + r) * 12 : nullptr);
    float hx = 0.0f, hy = 0.0f, hz = 0.0f, vx = 0.0f, vy = 0.0f, vz = 0.0f, hw = 0.0f, hqx = 0.0f, hqy = 0.0f, hqz = 0.0f, om = 0.0f;
    if (a.has_state) {
      hx = state[0], hy = state[1], hz = state[2], vx = state[3], vy = state[4], vz = state[5];
      hw = state[6], hqx = state[7], hqy = state[8], hqz = state[9], om = state[10];
    }
    float x = src[0], y = src[1], z = src[2], pitch = src[3], yaw = src[4], roll = src[5];
    for (int64_t t = 0; t < a.T; ++t) {
      const float cx = x, cy = y, cz = z, cp = pitch, cyw = yaw, cr = roll;
      if (t + 1 < a.T) {                                               // the next row, asked for before this one's arithmetic
        const float *p = src + (t + 1) * stride;
        x = p[0], y = p[1], z = p[2], pitch = p[3], yaw = p[4], roll = p[5];
      }
      float *o = dst + t * stride;
      float qw, qx, qy, qz;
      row_quat(cp, cyw, cr, qw, qx, qy, qz);
      if (t == 0 && !a.has_state) {                                    // a video's first frame: the state starts, the row is copied
        hx = cx, hy = cy, hz = cz, hw = qw, hqx = qx, hqy = qy, hqz = qz;
        o[0] = cx, o[1] = cy, o[2] = cz, o[3] = cp, o[4] = cyw, o[5] = cr;
        continue;
      }
      const float dx = cx - hx, dy = cy - hy, dz = cz - hz;
      vx = vx + a.alpha_d * (dx * a.fps - vx), vy = vy + a.alpha_d * (dy * a.fps - vy), vz = vz + a.alpha_d * (dz * a.fps - vz);
      const float fc_loc = a.min_cutoff + a.beta_loc * sqrtf(vx * vx + vy * vy + vz * vz);
      const float al = 1.0f / (1.0f + a.k / fc_loc);
      hx = hx + al * dx, hy = hy + al * dy, hz = hz + al * dz;
      float d = hw * qw + hqx * qx + hqy * qy + hqz * qz;
      if (d < 0.0f) qw = -qw, qx = -qx, qy = -qy, qz = -qz, d = -d;   // the shortest arc
      d = d > 1.0f ? 1.0f : d;                                         // a comparison: a NaN stays a NaN
      const float theta = acosf(d);
      om = om + a.alpha_d * (2.0f * theta * a.fps - om);
      const float fc_rot = a.min_cutoff + a.beta_rot * om;
      const float ar = 1.0f / (1.0f + a.k / fc_rot);
      float wa = 1.0f - ar, wb = ar;
      if (!(d > 0.99999f)) {
        const float inv = 1.0f / sinf(theta);
        wa = sinf((1.0f - ar) * theta) * inv;
        wb = sinf(ar * theta) * inv;
      }
      const float sw = wa * hw + wb * qw, sx = wa * hqx + wb * qx, sy = wa * hqy + wb * qy, sz = wa * hqz + wb * qz;
      const float rn = 1.0f / sqrtf(sw * sw + sx * sx + sy * sy + sz * sz);
      hw = sw * rn, hqx = sx * rn, hqy = sy * rn, hqz = sz * rn;
      quat_row(hx, hy, hz, hw, hqx, hqy, hqz, o);
    }
    if (state) {
      state[0] = hx, state[1] = hy, state[2] = hz, state[3] = vx, state[4] = vy, state[5] = vz;
      state[6] = hw, state[7] = hqx, state[8] = hqy, state[9] = hqz, state[10] = om, state[11] = 0.0f;
    }
  }
}

constexpr int64_t kMaxCount = (int64_t)1 << 40;

static bool rows_fit(int64_t N, int64_t frames, int32_t J) {          // N frames (J + 1) <= 2^40
  return !(N > 0 && frames > 0 && N > kMaxCount / frames / ((int64_t)J + 1));
}

static bool positive(double v) { return std::isfinite(v) && v > 0.0; }

}  // namespace p2c_smooth

using namespace p2c_smooth;

extern "C" int p2c_carla_smooth_gauss_fwd(const float *bones, const float *root, float *out_bones, float *out_root,
                                          const float *weights, int64_t N, int64_t S, int32_t J, int64_t K, int64_t first_frame,
                                          int64_t first_output, int64_t last_frame, int32_t R, int32_t max_blocks, void *stream) {
  if (N < 0 || S < 0 || K < 0 || J < 1 || first_frame < 0 || first_output < 0 || last_frame < -1 || max_blocks < 0) return P2C_E_SHAPE;
  if (R < 0 || R > P2C_SMOOTH_MAX_RADIUS) return P2C_E_SHAPE;
  if (N > kMaxCount || S > kMaxCount || K > kMaxCount || last_frame > kMaxCount || first_output > kMaxCount - K ||
      first_frame > kMaxCount - S)
    return P2C_E_SHAPE;
  if (!rows_fit(N, K, J) || !rows_fit(N, S, J)) return P2C_E_SHAPE;
  if (S == 0 && K > 0 && N > 0) return P2C_E_SHAPE;                    // outputs of no frames
  if (!bones || !out_bones) return P2C_E_NULL;
  if ((root == nullptr) != (out_root == nullptr)) return P2C_E_NULL;   // both or neither
  if (R > 0 && !weights) return P2C_E_NULL;
  if (N == 0 || K == 0) return 0;
  GaussArgs a{};
  a.bones = bones, a.root = root, a.weights = weights, a.out_bones = out_bones, a.out_root = out_root;
  a.S = S, a.K = K, a.first_frame = first_frame, a.first_output = first_output;
  a.hi_all = last_frame >= 0 ? last_frame : kMaxCount * 2;
  a.J = J, a.W = J + (root ? 1 : 0), a.R = R;
  a.rows = a.W < kRows ? a.W : kRows;
  const int room = kLdsFloats / (7 * a.rows) - 2 * R;                  // frames of output the image has room for: >= 22
  a.F = room < kMaxTile ? room : kMaxTile;
  a.tiles = (K + a.F - 1) / a.F;
  a.chunks = (a.W + kRows - 1) / kRows;
  a.units = N * a.tiles * a.chunks;
  const size_t lds_bytes = R > 0 ? ((size_t)(a.F + 2 * R) * a.rows * 7 + kTable) * sizeof(float) : 0;
  const unsigned grid = p2c_host::grid_for(a.units, max_blocks, kMaxBlocks);
  hipLaunchKernelGGL(carla_smooth_gauss_kernel, dim3(grid), dim3(kThreads), lds_bytes, (hipStream_t)stream, a);
  return p2c_host::launch_status();
}

extern "C" int p2c_carla_smooth_euro_fwd(const float *bones, const float *root, float *state_bones, float *state_root,
                                         float *out_bones, float *out_root, int64_t N, int64_t T, int32_t J, int32_t has_state,
                                         double fps, double min_cutoff, double beta_loc, double beta_rot, double d_cutoff,
                                         int32_t max_blocks, void *stream) {
  if (N < 0 || T < 0 || J < 1 || max_blocks < 0 || (has_state != 0 && has_state != 1)) return P2C_E_SHAPE;
  if (N > kMaxCount || T > kMaxCount || !rows_fit(N, T, J)) return P2C_E_SHAPE;
  // the kernel uses the fp32 values: a rate or cutoff that rounds to 0 or to infinity is refused as well
  for (const double v : {fps, min_cutoff, d_cutoff})
    if (!positive(v) || !positive((double)(float)v)) return P2C_E_SHAPE;
  for (const double v : {beta_loc, beta_rot})
    if (!(std::isfinite(v) && v >= 0.0 && std::isfinite((double)(float)v))) return P2C_E_SHAPE;
  if (!bones || !out_bones) return P2C_E_NULL;
  if ((root == nullptr) != (out_root == nullptr)) return P2C_E_NULL;   // both or neither
  if (has_state && (!state_bones || (root && !state_root))) return P2C_E_NULL;
  if (N == 0 || T == 0) return 0;
  const double two_pi = 6.283185307179586;
  EuroArgs a{};
  a.bones = bones, a.root = root, a.state_bones = state_bones, a.state_root = root ? state_root : nullptr;
  a.out_bones = out_bones, a.out_root = out_root;
  a.T = T, a.J = J, a.W = J + (root ? 1 : 0), a.has_state = has_state;
  a.chains = N * a.W;
  a.fps = (float)fps, a.min_cutoff = (float)min_cutoff, a.beta_loc = (float)beta_loc, a.beta_rot = (float)beta_rot;
  a.alpha_d = (float)(1.0 / (1.0 + fps / (two_pi * d_cutoff)));
  a.k = (float)(fps / two_pi);
  const unsigned grid = p2c_host::grid_for((a.chains + kEuroThreads - 1) / kEuroThreads, max_blocks, kEuroMaxBlocks);
  hipLaunchKernelGGL(carla_smooth_euro_kernel, dim3(grid), dim3(kEuroThreads), 0, (hipStream_t)stream, a);
  return p2c_host::launch_status();
}
