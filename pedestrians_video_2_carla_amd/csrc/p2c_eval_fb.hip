// p2c_eval_fb.hip -- K22: the five FB_* validation metrics of the pose-lifting flow in one launch (gfx950).
//
// metrics/extra_metrics.py restates them as tensor reductions (mpjpe, weighted_mpjpe, n_mpjpe, mean_velocity_error, p_mpjpe):
// five passes over absolute_pose_loc, full-size temporaries, and for PA-MPJPE a batched library SVD of B*T 3x3 matrices in
// fp64. Here one G-lane group owns one frame, lane = joint: the frame (and its successor, for the velocity) is read once, every
// reduction over joints is a wave shuffle, and the 3x3 problem is solved in registers (p2c_procrustes_dev.h). All arithmetic is
// fp64 -- the tensor path it is pinned against is fp64 where it matters, and at one tiny problem per frame the rate does not.
// A one-workgroup fixed-order pass then ADDS the selected columns into the persistent (sum, count) state, as p2c_eval.hip does.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "../../include/p2c.h"
#include "p2c_host.h"
#include "p2c_lane_dev.h"
#include "p2c_procrustes_dev.h"

namespace p2c_fb {

constexpr int COLS = 5;                          // MPJPE, weighted, N-MPJPE, MPJVE, PA-MPJPE: the bits of `which`
enum { M_MPJPE = 1, M_WEIGHTED = 2, M_N = 4, M_V = 8, M_PA = 16, M_ALL = 31 };

struct Args {
  const float *pred, *gt, *w;                    // (N,J,3), (N,J,3), J weights or NULL
  float *partials;                               // (launched wavefronts, COLS)
  int64_t N;
  int32_t J, which;
};

using p2c_lane::xor_sum;

__device__ __forceinline__ double norm3(double x, double y, double z) { return sqrt(x * x + y * y + z * z); }

template <int G>
__global__ __launch_bounds__(256) void fb_kernel(const Args a) {
  const int lane = threadIdx.x & 63, j = lane & (G - 1);
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t n = wave * (64 / G) + lane / G;
  const bool frame_ok = n < a.N, joint_ok = frame_ok && j < a.J;
  const double invJ = 1.0 / (double)a.J;
  double p[3] = {0.0, 0.0, 0.0}, g[3] = {0.0, 0.0, 0.0};
  if (joint_ok) {
    const float *pp = a.pred + ((size_t)n * a.J + j) * 3, *gp = a.gt + ((size_t)n * a.J + j) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = (double)pp[k], g[k] = (double)gp[k];
  }
  double m[COLS] = {0.0, 0.0, 0.0, 0.0, 0.0};        // the frame's sums over joints (lanes past J add exact zeros)

  if (a.which & (M_MPJPE | M_WEIGHTED)) {
    const double d = norm3(p[0] - g[0], p[1] - g[1], p[2] - g[2]);
    if (a.which & M_MPJPE) m[0] = xor_sum<G>(d);
    if (a.which & M_WEIGHTED) m[1] = xor_sum<G>((a.w && joint_ok) ? (double)a.w[j] * d : d);
  }
  if (a.which & M_N) {                             // n_mpjpe: s = <g, p> / <p, p> over the frame (the two joint means cancel)
    const double gp = xor_sum<G>(g[0] * p[0] + g[1] * p[1] + g[2] * p[2]);
    const double pp = xor_sum<G>(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
    const double s = gp / pp;                      // 0/0 for an all-zero prediction: NaN, as in the tensor path
    const double d = norm3(s * p[0] - g[0], s * p[1] - g[1], s * p[2] - g[2]);
    m[2] = xor_sum<G>(joint_ok ? d : 0.0);            // (a NaN scale must not leak in through the lanes past J of a finite frame)
  }
  if (a.which & M_V) {                             // mean_velocity_error over the flattened (clip x frame) axis
    double d = 0.0;
    if (joint_ok && n + 1 < a.N) {
      const float *pp = a.pred + ((size_t)(n + 1) * a.J + j) * 3, *gp = a.gt + ((size_t)(n + 1) * a.J + j) * 3;
      d = norm3(((double)pp[0] - p[0]) - ((double)gp[0] - g[0]), ((double)pp[1] - p[1]) - ((double)gp[1] - g[1]),
                ((double)pp[2] - p[2]) - ((double)gp[2] - g[2]));
    }
    m[3] = xor_sum<G>(d);
  }
  if (a.which & M_PA) {                            // p_mpjpe, step for step
    double x0[3], y0[3];                           // centred, then scaled to unit Frobenius norm
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double mux = xor_sum<G>(g[k]) * invJ, muy = xor_sum<G>(p[k]) * invJ;
      x0[k] = joint_ok ? g[k] - mux : 0.0, y0[k] = joint_ok ? p[k] - muy : 0.0;
    }
    const double normX = sqrt(xor_sum<G>(x0[0] * x0[0] + x0[1] * x0[1] + x0[2] * x0[2]));
    const double normY = sqrt(xor_sum<G>(y0[0] * y0[0] + y0[1] * y0[1] + y0[2] * y0[2]));
#pragma unroll
    for (int k = 0; k < 3; ++k) {                  // coincident joints: 0/0 on the real lanes, NaN as in the tensor path
      x0[k] = joint_ok ? x0[k] / normX : 0.0, y0[k] = joint_ok ? y0[k] / normY : 0.0;
    }
    double H[3][3], R[3][3], ssum;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) H[r][c] = xor_sum<G>(x0[r] * y0[c]);
    p2c_procrustes::solve(H, R, ssum);
    // a (Y R) + t - X with a = ssum normX / normY and t = muX - a muY R  ==  normX (ssum (Y0 R) - X0), the offsets cancelled
    double e[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) e[c] = ssum * (y0[0] * R[0][c] + y0[1] * R[1][c] + y0[2] * R[2][c]) - x0[c];
    m[4] = xor_sum<G>(joint_ok ? normX * norm3(e[0], e[1], e[2]) : 0.0);
  }
  // empty groups hold 0/0 here: selected away, not multiplied away. Every launched wavefront writes its row.
#pragma unroll
  for (int k = 0; k < COLS; ++k) {
    double v = frame_ok ? m[k] : 0.0;
    if (G == 32) v += __shfl_xor(v, 32, 64);
    if (lane == 0) a.partials[wave * COLS + k] = (float)v;
  }
}

// state[2k] += scale_k * (column k of the partials, summed in fixed order), state[2k+1] += count, for the selected k only
__global__ __launch_bounds__(256) void fb_accumulate_kernel(const float *partials, int64_t rows, int32_t which, double *state,
                                                            double scale, double scale_v, double count) {
  __shared__ double sh[256];
  for (int k = 0; k < COLS; ++k) {
    if (!((which >> k) & 1)) continue;
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < rows; i += 256) s += (double)partials[i * COLS + k];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
      if ((int)threadIdx.x < st) sh[threadIdx.x] += sh[threadIdx.x + st];
      __syncthreads();
    }
    if (threadIdx.x == 0) state[2 * k] += sh[0] * (k == 3 ? scale_v : scale), state[2 * k + 1] += count;
    __syncthreads();
  }
}

static int64_t launched_waves(int64_t N, int32_t J) {
  const int per_wave = J <= 32 ? 2 : 1;
  const int64_t waves = (N + per_wave - 1) / per_wave;
  return (waves + 3) / 4 * 4;                    // whole 256-thread workgroups
}

}  // namespace p2c_fb

using namespace p2c_fb;

extern "C" int64_t p2c_eval_fb_workspace_floats(int64_t N) {
  if (N <= 0) return 0;
  return COLS * launched_waves(N, 64);            // one row per launched wavefront; one frame per wavefront is the most
}

extern "C" int p2c_eval_fb(const float *pred, const float *gt, const float *w, int64_t N, int32_t J, int32_t which,
                           float *partials, double *state, void *stream_) {
  if (!pred || !gt || !partials || !state) return P2C_E_NULL;
  if (N < 0 || J < 1 || J > 64 || which < 1 || which > M_ALL) return P2C_E_SHAPE;
  if (N == 0) return 0;
  if ((which & M_V) && N < 2) return P2C_E_SHAPE;
  const int64_t waves = launched_waves(N, J);
  if (waves / 4 > 0x7fffffffLL) return P2C_E_SHAPE;
  Args a{};
  a.pred = pred, a.gt = gt, a.w = w, a.partials = partials, a.N = N, a.J = J, a.which = which;
  hipStream_t stream = (hipStream_t)stream_;
  const dim3 grid((unsigned)(waves / 4));
  if (J <= 32) hipLaunchKernelGGL(fb_kernel<32>, grid, dim3(256), 0, stream, a);
  else hipLaunchKernelGGL(fb_kernel<64>, grid, dim3(256), 0, stream, a);
  // _FBMetric.update: state[2k] += N * (batch mean), state[2k+1] += N; the velocity has N - 1 frames in its mean
  const double scale = 1.0 / (double)J;
  const double scale_v = N > 1 ? (double)N / ((double)(N - 1) * (double)J) : 0.0;
  hipLaunchKernelGGL(fb_accumulate_kernel, dim3(1), dim3(256), 0, stream, (const float *)partials, waves, which, state, scale,
                     scale_v, (double)N);
  return p2c_host::launch_status();
}
