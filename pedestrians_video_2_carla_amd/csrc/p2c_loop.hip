// p2c_loop.hip -- K41: the cycle of a CARLA animation that closes best, and that cycle played for any number of frames (gfx950).
//
// Definition: walker_control/loop.py (the reference has no counterpart: its players stop where the clip stops).
// Rows are (x, y, z, pitch, yaw, roll); q[t, j] is the unit quaternion row_quat makes of bone row (t, j) (K37's).
//
// Search (p2c_carla_loop_find_fwd). d(a, b) = sum_j w_j (1 - <q[a,j], q[b,j]>^2), j ascending, the four products of a dot product
// added from the first to the last; C(s, e) = sum_{k = -blend .. 0} d(s + k, e + k), k ascending, for the admissible pairs
// blend <= s, s + min_period <= e <= min(s + max_period, T - 1), +inf elsewhere. Per video the admissible pair with the smallest
// finite cost wins, ties to the smallest s, then the smallest e; none: (-1, -1) and NaN.
// Mapping: a workgroup takes a unit = (video, 32 x 32 tile of (s, e)). Only the tile columns the band min_period <= e - s <=
// max_period of a tile row can reach are enumerated; when the whole matrix is asked for, every column is, and a tile without an
// admissible pair costs one test and its +inf stores. It converts the rows of frames s0 - blend .. s0 + 31 and e0 - blend ..
// e0 + 31 ONCE into quaternions in LDS (bone-major, so the lanes of a wavefront read neighbouring 16-byte slots), forms the
// F x F tile of d there (F = 32 + blend), and each lane then sums the diagonals of its pairs in ascending k. The bones are taken in
// chunks when 2 F J quaternions and the tile do not fit 64 KB (J > 23 at blend = 32), a d entry accumulating over the chunks in
// the same ascending order. A frame outside the video is never read: its quaternions are zero and reach inadmissible pairs only.
// The tile's best pair is the minimum of 64-bit keys (the cost's bits mapped to an order-preserving integer, then s, then e) over
// an LDS tree, and one integer atomic minimum per tile puts it into the video's word of the workspace: integer minima are exact
// and do not depend on the order of arrival, and the key carries the tie-break. Two one-lane-per-video launches set the words
// before and read them back after. No floating-point atomics. Each C(s, e) is the work of one lane in a fixed order: its bits
// do not depend on the grid, on which outputs are asked for, or on the batch around the video.
//
// Play (p2c_carla_loop_play_fwd), K37's shape: one lane per output row, at most two source rows in, one row out, no LDS. Output
// g = first_output + i of a video with loop (s, e), P = e - s: c = g div P, phi = g mod P, a = s + phi. phi < P - blend copies row a.
// Otherwise u = (float)((phi - (P - blend) + 1) / (double)(blend + 1)), b = a - P, and the row is K37's interpolation of rows a and
// b at u. Root x and y are formed in fp64 -- m = (1 - u) root[a] + u (root[b] + delta) inside the window, root[a] outside,
// delta = root[e] - root[s], out = (float)(m + c delta), every product and sum rounded on its own -- and cycle 0 outside the
// window copies them. A loop that is not blend <= s < e <= T - 1 is never followed: its video plays NaN rows.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/p2c.h"
#include "p2c_host.h"

#include "p2c_carla_dev.h"   // carla_row, row_quat

namespace p2c_loop {

using p2c_carla::carla_row;
using p2c_carla::row_quat;

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;                  // 8 workgroups per CU on 256 CUs
constexpr int kTile = 32;                         // (s, e) pairs to a unit: kTile x kTile
constexpr int kLdsBytes = 64 * 1024;
constexpr int kKeyBytes = kThreads * 8;           // the reduction's keys, in front of the image
constexpr uint64_t kNoKey = ~(uint64_t)0;

struct FindArgs {
  const float *bones, *weights;
  float *out_cost;
  unsigned long long *best;                       // (N) keys
  int64_t T, tiles, width, units, min_period, max_period;   // width: tile columns of a tile row that are enumerated
  int32_t J, blend, F, chunk, full;               // F = kTile + blend frames a side, chunk bones to an image, full: every column
};

// cost bits -> an unsigned integer with the order of the floats (finite values only come here)
__device__ __forceinline__ uint32_t ordered_bits(float v) {
  const uint32_t b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float unordered_bits(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__global__ __launch_bounds__(kThreads) void carla_loop_init_kernel(unsigned long long *best, int64_t N) {
  const int64_t step = (int64_t)gridDim.x * kThreads;
  for (int64_t n = (int64_t)blockIdx.x * kThreads + threadIdx.x; n < N; n += step) best[n] = kNoKey;
}

__global__ __launch_bounds__(kThreads) void carla_loop_finish_kernel(const unsigned long long *best, int64_t *out_loop,
                                                                     float *out_loop_cost, int64_t N) {
  const int64_t step = (int64_t)gridDim.x * kThreads;
  for (int64_t n = (int64_t)blockIdx.x * kThreads + threadIdx.x; n < N; n += step) {
    const uint64_t key = best[n];
    const bool found = key != kNoKey;
    out_loop[n * 2] = found ? (int64_t)((key >> 16) & 0xffffu) : -1;
    out_loop[n * 2 + 1] = found ? (int64_t)(key & 0xffffu) : -1;
    out_loop_cost[n] = found ? unordered_bits((uint32_t)(key >> 32)) : __builtin_nanf("");
  }
}

__global__ __launch_bounds__(kThreads) void carla_loop_find_kernel(FindArgs a) {
  extern __shared__ __attribute__((aligned(16))) char lds_raw[];
  unsigned long long *keys = reinterpret_cast<unsigned long long *>(lds_raw);
  float *dist = reinterpret_cast<float *>(lds_raw + kKeyBytes);      // (F, F): d(s0 - blend + ia, e0 - blend + ib)
  const int F = a.F;
  const int dist_floats = (F * F + 3) & ~3;                           // the quaternions start on a 16-byte slot
  float4 *quat_s = reinterpret_cast<float4 *>(dist + dist_floats);    // (chunk, F) each
  float4 *quat_e = quat_s + a.chunk * F;
  const int tid = threadIdx.x;
  const float inf = __builtin_inff();
  for (int64_t u = blockIdx.x; u < a.units; u += gridDim.x) {
    const int64_t per_video = a.tiles * a.width;
    const int64_t n = u / per_video, rest = u - n * per_video;
    const int64_t ts = rest / a.width, s0 = ts * kTile;
    // without the matrix only the columns the band of this tile row can reach: from the one that holds e = s0 + min_period on
    const int64_t te = rest - ts * a.width + (a.full ? 0 : (s0 + a.min_period) / kTile);
    if (te >= a.tiles) continue;                                      // the same test in every lane
    const int64_t e0 = te * kTile;
    // the tile's pairs with the largest and the smallest e - s: (s0 + 31, e0) and (s0, e0 + 31); s <= T - 1 - min_period, s >= blend
    const int64_t s_hi = s0 + kTile - 1, e_hi = e0 + kTile - 1 < a.T - 1 ? e0 + kTile - 1 : a.T - 1;
    const bool on_band = e_hi - s0 >= a.min_period && e0 - s_hi <= a.max_period && s_hi >= a.blend;
    float *cost = a.out_cost ? a.out_cost + n * a.T * a.T : nullptr;
    if (!on_band) {                                                   // the same test in every lane
      if (cost)
        for (int i = tid; i < kTile * kTile; i += kThreads) {
          const int64_t s = s0 + (i >> 5), e = e0 + (i & 31);
          if (s < a.T && e < a.T) cost[s * a.T + e] = inf;
        }
      continue;
    }
    for (int i = tid; i < F * F; i += kThreads) dist[i] = 0.0f;
    for (int j0 = 0; j0 < a.J; j0 += a.chunk) {
      const int nj = a.J - j0 < a.chunk ? a.J - j0 : a.chunk;
      // both sides of the tile, frames in the outer position: neighbouring lanes read neighbouring bones of a frame
      for (int i = tid; i < 2 * F * nj; i += kThreads) {
        const int side = i >= F * nj, r = i - side * F * nj;
        const int f = r / nj, jj = r - f * nj;
        const int64_t t = (side ? e0 : s0) - a.blend + f;
        float4 q = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (t >= 0 && t < a.T) {
          const float *p = a.bones + ((n * a.T + t) * a.J + j0 + jj) * 6;
          row_quat(p[3], p[4], p[5], q.x, q.y, q.z, q.w);              // (w, x, y, z) in (x, y, z, w)
        }
        (side ? quat_e : quat_s)[jj * F + f] = q;
      }
      __syncthreads();
      for (int i = tid; i < F * F; i += kThreads) {
        const int ia = i / F, ib = i - ia * F;
        float acc = dist[i];
        for (int jj = 0; jj < nj; ++jj) {
          const float4 qa = quat_s[jj * F + ia], qb = quat_e[jj * F + ib];
          const float dot = ((qa.x * qb.x + qa.y * qb.y) + qa.z * qb.z) + qa.w * qb.w;
          const float term = 1.0f - dot * dot;
          acc += a.weights ? a.weights[j0 + jj] * term : term;
        }
        dist[i] = acc;
      }
      __syncthreads();                                                 // the next chunk overwrites the quaternions
    }
    uint64_t key = kNoKey;
    for (int i = tid; i < kTile * kTile; i += kThreads) {
      const int si = i >> 5, ei = i & 31;
      const int64_t s = s0 + si, e = e0 + ei;
      if (s >= a.T || e >= a.T) continue;
      float c = inf;
      if (s >= a.blend && e - s >= a.min_period && e - s <= a.max_period) {
        c = 0.0f;
        for (int k = 0; k <= a.blend; ++k) c += dist[(si + k) * F + (ei + k)];   // local frame si + blend + (k - blend)
        if (c < inf && c > -inf) {                                     // a NaN passes neither comparison
          const uint64_t mine = ((uint64_t)ordered_bits(c) << 32) | ((uint64_t)s << 16) | (uint64_t)e;
          key = mine < key ? mine : key;
        }
      }
      if (cost) cost[s * a.T + e] = c;
    }
    keys[tid] = key;
    __syncthreads();
    for (int half = kThreads / 2; half > 0; half >>= 1) {
      if (tid < half) {
        const uint64_t other = keys[tid + half];
        if (other < keys[tid]) keys[tid] = other;
      }
      __syncthreads();
    }
    if (tid == 0 && keys[0] != kNoKey) atomicMin(a.best + n, (unsigned long long)keys[0]);
    __syncthreads();                                                   // the next unit overwrites the keys and the tile
  }
}

struct PlayArgs {
  const float *bones, *root;
  const int64_t *loop;
  float *out_bones, *out_root;
  int64_t T, K, n_bones, n_total, first_output;   // n_bones = N K J output rows of bones, n_total adds the N K root rows
  int32_t J, blend;
};

__global__ __launch_bounds__(kThreads) void carla_loop_play_kernel(PlayArgs a) {
  const int64_t step = (int64_t)gridDim.x * kThreads;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < a.n_total; i += step) {
    const bool is_root = i >= a.n_bones;
    const uint32_t width = is_root ? 1u : (uint32_t)a.J;              // rows per frame; row counts are below 2^31
    const uint32_t row = (uint32_t)(is_root ? i - a.n_bones : i);
    const uint32_t frame = row / width, j = row - frame * width;      // frame = n K + k
    const uint32_t n = frame / (uint32_t)a.K, k = frame - n * (uint32_t)a.K;
    const float *src = is_root ? a.root : a.bones;
    float *o = (is_root ? a.out_root : a.out_bones) + (int64_t)row * 6;
    const int64_t s = a.loop[(int64_t)n * 2], e = a.loop[(int64_t)n * 2 + 1];
    if (!(s >= a.blend && s < e && e <= a.T - 1)) {                    // no loop, or one that cannot be followed
      const float nan = __builtin_nanf("");
      o[0] = nan, o[1] = nan, o[2] = nan, o[3] = nan, o[4] = nan, o[5] = nan;
      continue;
    }
    const int64_t P = e - s, g = a.first_output + k;
    const int64_t c = g / P, phi = g - c * P;
    const int64_t fa = s + phi;
    const float *pa = src + (((int64_t)n * a.T + fa) * width + j) * 6;
    const float ax = pa[0], ay = pa[1], az = pa[2], ap = pa[3], aw = pa[4], ar = pa[5];
    const bool inside = phi >= P - a.blend;
    if (!inside && (!is_root || c == 0)) {
      o[0] = ax, o[1] = ay, o[2] = az, o[3] = ap, o[4] = aw, o[5] = ar;
      continue;
    }
    double dx = 0.0, dy = 0.0;
    if (is_root) {
      const float *ps = src + ((int64_t)n * a.T + s) * 6, *pe = src + ((int64_t)n * a.T + e) * 6;
      dx = (double)pe[0] - (double)ps[0], dy = (double)pe[1] - (double)ps[1];
    }
    if (!inside) {                                                     // a later cycle of the root: moved, the rest copied
      o[0] = (float)__dadd_rn((double)ax, __dmul_rn((double)c, dx));
      o[1] = (float)__dadd_rn((double)ay, __dmul_rn((double)c, dy));
      o[2] = az, o[3] = ap, o[4] = aw, o[5] = ar;
      continue;
    }
    const float u = (float)((double)(phi - (P - a.blend) + 1) / (double)(a.blend + 1));
    const float *pb = pa - P * (int64_t)width * 6;                     // frame a - P >= s - blend >= 0
    const float bx = pb[0], by = pb[1], bz = pb[2], bp = pb[3], bw = pb[4], br = pb[5];
    float qaw, qax, qay, qaz, qbw, qbx, qby, qbz;
    row_quat(ap, aw, ar, qaw, qax, qay, qaz);
    row_quat(bp, bw, br, qbw, qbx, qby, qbz);
    float d = qaw * qbw + qax * qbx + qay * qby + qaz * qbz;
    if (d < 0.0f) qbw = -qbw, qbx = -qbx, qby = -qby, qbz = -qbz, d = -d;   // the shortest arc
    d = d > 1.0f ? 1.0f : d;                                                   // a comparison: a NaN stays a NaN
    float wa = 1.0f - u, wb = u;
    if (!(d > 0.99999f)) {
      const float theta = acosf(d), inv = 1.0f / sinf(theta);
      wa = sinf((1.0f - u) * theta) * inv;
      wb = sinf(u * theta) * inv;
    }
    float w = wa * qaw + wb * qbw, x = wa * qax + wb * qbx, y = wa * qay + wb * qby, z = wa * qaz + wb * qbz;
    const float rn = 1.0f / sqrtf(w * w + x * x + y * y + z * z);
    w *= rn, x *= rn, y *= rn, z *= rn;
    const float r00 = 1.0f - 2.0f * (y * y + z * z), r01 = 2.0f * (x * y - w * z), r02 = 2.0f * (x * z + w * y);
    const float r12 = 2.0f * (y * z - w * x), r22 = 1.0f - 2.0f * (x * x + y * y);
    float row_out[6];
    // locations are stored values: carla_row negates z, so it is given -z
    carla_row(ax + u * (bx - ax), ay + u * (by - ay), -(az + u * (bz - az)), r00, r01, r02, r12, r22, row_out);
    if (is_root) {
      const double ud = (double)u, one_u = 1.0 - ud;
      const double mx = __dadd_rn(__dmul_rn(one_u, (double)ax), __dmul_rn(ud, (double)bx + dx));
      const double my = __dadd_rn(__dmul_rn(one_u, (double)ay), __dmul_rn(ud, (double)by + dy));
      row_out[0] = (float)__dadd_rn(mx, __dmul_rn((double)c, dx));
      row_out[1] = (float)__dadd_rn(my, __dmul_rn((double)c, dy));
    }
    o[0] = row_out[0], o[1] = row_out[1], o[2] = row_out[2], o[3] = row_out[3], o[4] = row_out[4], o[5] = row_out[5];
  }
}

constexpr int64_t kMaxRows = (int64_t)1 << 31;

// N frames rows_per_frame < 2^31
static bool rows_fit(int64_t N, int64_t frames, int64_t rows_per_frame) {
  return !(N > 0 && frames > 0 && N > (kMaxRows - 1) / frames / rows_per_frame);
}

static bool find_shape_ok(int64_t N, int64_t T, int32_t J, int32_t blend, int64_t min_period, int64_t max_period) {
  if (N < 0 || N >= kMaxRows || T < 2 || T > P2C_LOOP_MAX_T || J < 1 || J > P2C_LOOP_MAX_J) return false;
  if (blend < 0 || blend > P2C_LOOP_MAX_BLEND || min_period < 1 || max_period < min_period) return false;
  return rows_fit(N, T, J);
}

// bones of an image: what 64 KB hold next to the keys and the F x F tile, J at the most
static int chunk_for(int32_t J, int32_t blend) {
  const int F = kTile + blend;
  const int room = (kLdsBytes - kKeyBytes - ((F * F + 3) & ~3) * 4) / (2 * F * 16);   // >= 23
  return J < room ? J : room;
}

}  // namespace p2c_loop

using namespace p2c_loop;

extern "C" int64_t p2c_carla_loop_find_workspace(int64_t N, int64_t T, int32_t J, int32_t blend) {
  if (!find_shape_ok(N, T, J, blend, 1, 1)) return -1;
  return N * 8;
}

extern "C" int p2c_carla_loop_find_fwd(const float *bones, const float *weights, int64_t *out_loop, float *out_loop_cost,
                                       float *out_cost, int64_t N, int64_t T, int32_t J, int32_t blend, int64_t min_period,
                                       int64_t max_period, int32_t max_blocks, void *workspace, void *stream) {
  if (max_blocks < 0 || !find_shape_ok(N, T, J, blend, min_period, max_period)) return P2C_E_SHAPE;
  if (!bones || !out_loop || !out_loop_cost) return P2C_E_NULL;
  if (N > 0 && !workspace) return P2C_E_NULL;
  if (N == 0) return 0;
  FindArgs a{};
  a.bones = bones, a.weights = weights, a.out_cost = out_cost, a.best = static_cast<unsigned long long *>(workspace);
  // e - s <= T - 1: periods from T on admit the same pairs as T does, and sums with them stay small
  a.T = T, a.J = J, a.blend = blend, a.min_period = min_period < T ? min_period : T, a.max_period = max_period < T ? max_period : T;
  a.F = kTile + blend;
  a.chunk = chunk_for(J, blend);
  a.tiles = (T + kTile - 1) / kTile;
  // e of tile row s0 .. s0 + 31 lies in s0 + min_period .. s0 + 31 + max_period: at most this many tile columns
  const int64_t reach = (kTile - 1 + (a.max_period - a.min_period)) / kTile + 2;
  a.full = out_cost != nullptr;                   // the matrix is written everywhere, +inf off the band
  a.width = a.full || reach > a.tiles ? a.tiles : reach;
  a.units = N * a.tiles * a.width;
  const size_t lds_bytes = (size_t)kKeyBytes + (size_t)((a.F * a.F + 3) & ~3) * 4 + (size_t)2 * a.chunk * a.F * 16;
  const unsigned lanes = p2c_host::grid_for((N + kThreads - 1) / kThreads, max_blocks, kMaxBlocks);
  hipLaunchKernelGGL(carla_loop_init_kernel, dim3(lanes), dim3(kThreads), 0, (hipStream_t)stream, a.best, N);
  const unsigned grid = p2c_host::grid_for(a.units, max_blocks, kMaxBlocks);
  hipLaunchKernelGGL(carla_loop_find_kernel, dim3(grid), dim3(kThreads), lds_bytes, (hipStream_t)stream, a);
  hipLaunchKernelGGL(carla_loop_finish_kernel, dim3(lanes), dim3(kThreads), 0, (hipStream_t)stream, a.best, out_loop,
                     out_loop_cost, N);
  return p2c_host::launch_status();
}

extern "C" int p2c_carla_loop_play_fwd(const float *bones, const float *root, const int64_t *loop, float *out_bones,
                                       float *out_root, int64_t N, int64_t T, int32_t J, int64_t frames, int64_t first_output,
                                       int32_t blend, int32_t max_blocks, void *stream) {
  if (N < 0 || T < 0 || frames < 0 || first_output < 0 || max_blocks < 0) return P2C_E_SHAPE;
  if (N >= kMaxRows || T > P2C_LOOP_MAX_T || J < 1 || J > P2C_LOOP_MAX_J || blend < 0 || blend > P2C_LOOP_MAX_BLEND) return P2C_E_SHAPE;
  if (first_output > ((int64_t)1 << 40) || !rows_fit(N, T, (int64_t)J + 1) || !rows_fit(N, frames, (int64_t)J + 1)) return P2C_E_SHAPE;
  if (N > 0 && frames > 0 && T < 2) return P2C_E_SHAPE;                // outputs of a video too short for any loop
  if (!bones || !loop || !out_bones) return P2C_E_NULL;
  if ((root == nullptr) != (out_root == nullptr)) return P2C_E_NULL;   // both or neither
  if (N == 0 || frames == 0) return 0;
  PlayArgs a{};
  a.bones = bones, a.root = root, a.loop = loop, a.out_bones = out_bones, a.out_root = out_root;
  a.T = T, a.K = frames, a.J = J, a.blend = blend, a.first_output = first_output;
  a.n_bones = N * frames * J;
  a.n_total = a.n_bones + (root ? N * frames : 0);
  const unsigned grid = p2c_host::grid_for((a.n_total + kThreads - 1) / kThreads, max_blocks, kMaxBlocks);
  hipLaunchKernelGGL(carla_loop_play_kernel, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, a);
  return p2c_host::launch_status();
}
