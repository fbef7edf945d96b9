// p2c_resample.hip -- K37: CARLA rows resampled to another frame rate, one launch for the bones and root of a batch (gfx950).
//
// Definition: walker_control/resample.py (the reference has no counterpart: its players set whatever rate the clip has).
// Output sample k (a global index, counted from the start of the video) sits at source position p = fl64(k * ratio),
// ratio = src_fps / dst_fps; i0 = floor(p), frac = (float)(p - i0). frac == 0 copies source row i0 bit for bit and reads no other
// row; otherwise rows a = i0 and b = i0 + 1 are combined: locations a + frac (b - a), rotations by the shortest-arc spherical
// interpolation of the rows' unit quaternions (w first, q = qx(e0) qy(e1) qz(e2) with (e0, e1, e2) = rad(-roll, -pitch, -yaw):
// the quaternion of the matrix K30's inverse forms), lerp weights above a dot product of 0.99999, normalised, and written back
// through carla_row on the five matrix entries it reads. mode HOLD copies row i0. Every comparison lets a NaN through: a NaN in a
// neighbour reaches the outputs computed from it and nothing else.
//
// Mapping, as K30's: one lane per output row; row e < N K J is bone row ((n K + k) J + j), row N K J + r is root row (n K + k).
// A lane reads two 24-byte source rows (the 64 lanes of a wavefront read neighbouring bones of the same one or two frames, so the
// 128-byte lines that are fetched are used whole; when upsampling, neighbouring outputs re-read the same frames from cache) and
// writes one 24-byte row (4-byte aligned multi-dword stores, merged by the compiler). No LDS, no barrier, no cross-lane traffic,
// one writer per element. The position is formed per lane in fp64 -- one multiply (__dmul_rn: never contracted with the
// subtraction that follows, so the host's fl64(k * ratio) is what the lane sees), a floor, a subtract -- and everything else is
// fp32. A lane's result is a function of its two source rows and frac only: not of the grid, of which outputs are asked for, or
// of where a streaming caller cut the video (source frame first_frame - 1 then comes from the carry row).
// A source index outside [first_frame - has_carry, first_frame + T - 1] is clamped, never followed: the caller checks the range.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "../../include/p2c.h"
#include "p2c_host.h"

#include "p2c_carla_dev.h"   // carla_row, row_quat

namespace p2c_resample {

using p2c_carla::carla_row;
using p2c_carla::row_quat;

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;   // 8 workgroups per CU on 256 CUs

struct Args {
  const float *bones, *root, *carry_bones, *carry_root;
  float *out_bones, *out_root;
  int64_t T, K, n_bones, n_total;  // n_bones = N K J output rows of bones, n_total adds the N K root rows
  int64_t first_output, first_frame, lo;   // lo: the smallest source index that can be read (first_frame - 1 with a carry)
  double ratio;
  int32_t J, mode;
};

// a / b and a % b for 0 <= a, 0 < b: in 32 bits where both fit
__device__ __forceinline__ void divmod(int64_t a, int64_t b, int64_t &q, int64_t &r) {
  if (((uint64_t)a | (uint64_t)b) <= 0xffffffffull) {
    const uint32_t q32 = (uint32_t)a / (uint32_t)b;
    q = q32, r = (uint32_t)a - q32 * (uint32_t)b;
  } else {
    q = a / b, r = a - q * b;
  }
}

__global__ __launch_bounds__(kThreads) void carla_resample_kernel(Args a) {
  const int64_t step = (int64_t)gridDim.x * kThreads;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < a.n_total; e += step) {
    const bool is_root = e >= a.n_bones;
    int64_t frame, j = 0;            // frame = n K + k
    int64_t width = 1;               // rows per frame
    if (is_root) {
      frame = e - a.n_bones;
    } else {
      width = a.J;
      divmod(e, width, frame, j);
    }
    int64_t n, k;
    divmod(frame, a.K, n, k);
    const double p = __dmul_rn((double)(a.first_output + k), a.ratio);
    const double fl = floor(p);
    const float frac = (float)(p - fl);
    const int64_t hi = a.first_frame + a.T - 1;
    int64_t i0 = (int64_t)fl;
    i0 = i0 < a.lo ? a.lo : (i0 > hi ? hi : i0);
    const int64_t i1 = i0 < hi ? i0 + 1 : hi;
    const float *src = is_root ? a.root : a.bones, *carry = is_root ? a.carry_root : a.carry_bones;
    const float *pa = i0 < a.first_frame ? carry + (n * width + j) * 6 : src + ((n * a.T + (i0 - a.first_frame)) * width + j) * 6;
    float *o = (is_root ? a.out_root : a.out_bones) + e * 6 - (is_root ? a.n_bones * 6 : 0);
    const float ax = pa[0], ay = pa[1], az = pa[2], ap = pa[3], aw = pa[4], ar = pa[5];
    if (frac == 0.0f || a.mode == P2C_RESAMPLE_HOLD) {
      o[0] = ax, o[1] = ay, o[2] = az, o[3] = ap, o[4] = aw, o[5] = ar;
      continue;
    }
    const float *pb = i1 < a.first_frame ? carry + (n * width + j) * 6 : src + ((n * a.T + (i1 - a.first_frame)) * width + j) * 6;
    const float bx = pb[0], by = pb[1], bz = pb[2], bp = pb[3], bw = pb[4], br = pb[5];
    float qaw, qax, qay, qaz, qbw, qbx, qby, qbz;
    row_quat(ap, aw, ar, qaw, qax, qay, qaz);
    row_quat(bp, bw, br, qbw, qbx, qby, qbz);
    float d = qaw * qbw + qax * qbx + qay * qby + qaz * qbz;
    if (d < 0.0f) qbw = -qbw, qbx = -qbx, qby = -qby, qbz = -qbz, d = -d;   // the shortest arc
    d = d > 1.0f ? 1.0f : d;                                                   // a comparison: a NaN stays a NaN
    float wa = 1.0f - frac, wb = frac;
    if (!(d > 0.99999f)) {
      const float theta = acosf(d), inv = 1.0f / sinf(theta);
      wa = sinf((1.0f - frac) * theta) * inv;
      wb = sinf(frac * theta) * inv;
    }
    float w = wa * qaw + wb * qbw, x = wa * qax + wb * qbx, y = wa * qay + wb * qby, z = wa * qaz + wb * qbz;
    const float rn = 1.0f / sqrtf(w * w + x * x + y * y + z * z);
    w *= rn, x *= rn, y *= rn, z *= rn;
    const float r00 = 1.0f - 2.0f * (y * y + z * z), r01 = 2.0f * (x * y - w * z), r02 = 2.0f * (x * z + w * y);
    const float r12 = 2.0f * (y * z - w * x), r22 = 1.0f - 2.0f * (x * x + y * y);
    // locations are stored values: carla_row negates z, so it is given -z
    carla_row(ax + frac * (bx - ax), ay + frac * (by - ay), -(az + frac * (bz - az)), r00, r01, r02, r12, r22, o);
  }
}

constexpr int64_t kMaxRows = (int64_t)1 << 40;

static int check_shape(int64_t N, int64_t T, int32_t J, int64_t K, int64_t first_output, int64_t first_frame, double ratio,
                       int32_t mode, int32_t max_blocks) {
  if (N < 0 || T < 0 || K < 0 || J < 1 || first_output < 0 || first_frame < 0 || max_blocks < 0) return P2C_E_SHAPE;
  if (N > kMaxRows || T > kMaxRows || K > kMaxRows || first_output > kMaxRows - K || first_frame > kMaxRows - T) return P2C_E_SHAPE;
  if (N > 0 && K > 0 && N > kMaxRows / K / ((int64_t)J + 1)) return P2C_E_SHAPE;          // N K (J + 1) output rows
  if (N > 0 && T > 0 && N > kMaxRows / T / ((int64_t)J + 1)) return P2C_E_SHAPE;          // and as many source rows at the most
  if (!std::isfinite(ratio) || ratio < 1.0 / 1024.0 || ratio > 1024.0) return P2C_E_SHAPE;
  if (mode != P2C_RESAMPLE_SLERP && mode != P2C_RESAMPLE_HOLD) return P2C_E_SHAPE;
  if (T == 0 && K > 0 && N > 0) return P2C_E_SHAPE;                                       // outputs of no frames
  return 0;
}

}  // namespace p2c_resample

using namespace p2c_resample;

extern "C" int p2c_carla_resample_fwd(const float *bones, const float *root, const float *carry_bones, const float *carry_root,
                                      float *out_bones, float *out_root, int64_t N, int64_t T, int32_t J, int64_t K,
                                      int64_t first_output, int64_t first_frame, double ratio, int32_t mode, int32_t max_blocks,
                                      void *stream) {
  const int rc = check_shape(N, T, J, K, first_output, first_frame, ratio, mode, max_blocks);
  if (rc) return rc;
  if (!bones || !out_bones) return P2C_E_NULL;
  if ((root == nullptr) != (out_root == nullptr)) return P2C_E_NULL;            // both or neither
  if (carry_root && !carry_bones) return P2C_E_NULL;
  if (root && carry_bones && !carry_root) return P2C_E_NULL;
  if (N == 0 || K == 0) return 0;
  Args a{};
  a.bones = bones, a.root = root, a.carry_bones = carry_bones, a.carry_root = root ? carry_root : nullptr;
  a.out_bones = out_bones, a.out_root = out_root;
  a.T = T, a.K = K, a.J = J, a.mode = mode;
  a.n_bones = N * K * J;
  a.n_total = a.n_bones + (root ? N * K : 0);
  a.first_output = first_output, a.first_frame = first_frame;
  a.lo = carry_bones && first_frame > 0 ? first_frame - 1 : first_frame;
  a.ratio = ratio;
  const unsigned grid = p2c_host::grid_for((a.n_total + kThreads - 1) / kThreads, max_blocks, kMaxBlocks);
  hipLaunchKernelGGL(carla_resample_kernel, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, a);
  return p2c_host::launch_status();
}
