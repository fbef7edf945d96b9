// p2c_train_dev.h -- geometry shared by the two forms of the fused train step's first launch: train_clip_kernel (p2c_train.hip:
// one workgroup of eight wavefronts per clip, the latency form for about one clip per CU) and train_stream_kernel
// (p2c_train_stream.hip: a pair of wavefronts per clip, four pairs per workgroup: the throughput form for several clips per CU). Both leave the same factor
// blocks and per-clip loss sums for train_wgrad_kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/p2c.h"
#include "p2c_mlp_dev.h"
#include "p2c_pose_head_dev.h"

namespace p2c_train {

using namespace p2c_mlp;
namespace ph = p2c;

using S = LinearAE156;                       // 52 -> 26 -> 13 -> 6 -> 39 -> 78 -> 156 (linear_ae.py:25-40, 6-D output)
constexpr int NLAY = S::NLAY;
// factor block of one clip: rows [H_0 .. H_{L-1} | G_1 .. G_L], 16 samples (64 B) per row
__host__ __device__ constexpr int f_h_off(int l) {
  int r = 0;
  for (int i = 0; i < l; ++i) r += S::dim_at(i);
  return r;
}
constexpr int F_HALF = f_h_off(NLAY);
__host__ __device__ constexpr int f_g_off(int l) {
  int r = F_HALF;
  for (int i = 1; i < l; ++i) r += S::dim_at(i);
  return r;
}
constexpr int F_ROWS = f_g_off(NLAY) + S::dim_at(NLAY);

struct ClipArgs {
  const float *x;          // (B*T, 52) model input
  const float *w_image;    // packed weight image (p2c_mlp_pack layout), current
  const float *counts;     // (B) unmasked 2-D target pairs per clip
  float *factors;          // (B, F_ROWS, 16)
  int32_t *counters;       // arrival tickets of the second launch: zeroed here
  int32_t n_counters;
  int32_t identity_maps;   // gmap2d[j] == gmap3d[j] == j for every joint (host-checked)
  float n3_elems;          // the loc_3d denominator B (t1 - t0) n_common3d 3 (= p2c::n3_elems, worked out on the host)
};

// Row of the activation area (counted from H_0's first row, pitch TP) that holds factor row r: the twelve segments H_0 .. H_{L-1},
// G_1 .. G_L are dense in the factor block and padded in LDS. A caller that knows r lies in [lo, hi] pays one compare and select
// per segment boundary inside that range; the boundaries are compile-time constants.
__host__ __device__ constexpr int f_seg_start(int s) { return s < NLAY ? f_h_off(s) : f_g_off(s - NLAY + 1); }
__host__ __device__ constexpr int f_seg_lds_row(int s) {
  return s < NLAY ? S::h_off(s) : S::h_off(NLAY) - S::h_off(1) + S::h_off(s - NLAY + 1);
}
__device__ __forceinline__ int f_lds_row(int r, int lo, int hi) {
  int shift = 0;
#pragma unroll
  for (int s = 1; s < 2 * NLAY; ++s) {
    const int d = f_seg_lds_row(s) - f_seg_start(s);
    if (f_seg_start(s) <= lo) shift = d;
    else if (f_seg_start(s) <= hi) shift = r >= f_seg_start(s) ? d : shift;
  }
  return r + shift;
}

// ---- how a clip's factor block leaves the CU (both forms; DESIGN 5.20, profiles/k13_handoff) -----------------------------------
// Placement (train_clip_kernel): P2C_TRAIN_FACTOR_EARLY=1 stores each segment from waves that idle behind the barrier that
// publishes it, only G_1 at the end; 0 = the whole block behind the last barrier (the parent's tail).
// Policy: P2C_TRAIN_FACTOR_SC1=1 stores write-through (sc1: the line leaves the XCD's L2 with the store, nothing of it is left
// for the kernel-end write-back), 0 = plain stores (the line stays dirty in L2 until the kernel ends), 2 = write-through for the
// H half only. P2C_STREAM_FACTOR_SC1 is the same policy switch for train_stream_kernel. A/B builds: EXTRA=-DP2C_TRAIN_FACTOR_...=n.
#ifndef P2C_TRAIN_FACTOR_EARLY
#define P2C_TRAIN_FACTOR_EARLY 1
#endif
#ifndef P2C_TRAIN_FACTOR_SC1
#define P2C_TRAIN_FACTOR_SC1 1
#endif
#ifndef P2C_STREAM_FACTOR_SC1
#define P2C_STREAM_FACTOR_SC1 1
#endif
constexpr int F_SEGS = 2 * NLAY;             // H_0 .. H_{L-1}, G_1 .. G_L
__host__ __device__ constexpr int f_seg_end(int s) { return s + 1 < F_SEGS ? f_seg_start(s + 1) : F_ROWS; }
__host__ __device__ constexpr bool f_seg_sc1(int s) { return P2C_TRAIN_FACTOR_SC1 == 1 || (P2C_TRAIN_FACTOR_SC1 == 2 && s < NLAY); }

typedef unsigned fu32x4 __attribute__((ext_vector_type(4)));
// the clip's factor block as a raw buffer (sixteen-byte stores by byte offset; aux 16 = sc1, as train_wgrad_kernel publishes its slices)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t factor_rsrc(float *factors, int clip) {
  return __builtin_amdgcn_make_buffer_rsrc(factors + (size_t)clip * F_ROWS * 16, 0, F_ROWS * 64, 0x00020000);
}
// Segments [S0, S1) of the clip's factor block, as they sit in LDS (act = H_0's first row, pitch TP), carried by waves [W0, W1) of the
// workgroup: item i = sixteen bytes i of the dense block, the same flat index whoever carries it. Every LDS read of the lane first
// (from the padded row that holds factor row i / 4), then its stores back to back. The caller stands behind the barrier that publishes
// the segments; waves outside the range pass through.
template <int S0, int S1, int W0, int W1>
__device__ __forceinline__ void factor_store(const float *act, const __amdgpu_buffer_rsrc_t rs, int wave, int lane) {
  static_assert(0 <= S0 && S0 < S1 && S1 <= F_SEGS && 0 <= W0 && W0 < W1 && W1 <= WAVES, "segment and wave ranges");
  static_assert(f_seg_sc1(S0) == f_seg_sc1(S1 - 1), "one store policy per call");
  constexpr int I0 = f_seg_start(S0) * 4, I1 = f_seg_end(S1 - 1) * 4, LANES = 64 * (W1 - W0), ROUNDS = (I1 - I0 + LANES - 1) / LANES;
  constexpr int R_LAST = f_seg_end(S1 - 1) - 1;
  if (wave < W0 || wave >= W1) return;
  const int me = (wave - W0) * 64 + lane;
  f32x4 fv[ROUNDS];
#pragma unroll
  for (int k = 0; k < ROUNDS; ++k) {
    int i = I0 + k * LANES + me;
    if (I0 + (k + 1) * LANES > I1) i = i < I1 ? i : I1 - 1;               // (the last round is partial: read a valid row, store nothing)
    const int hi = (I0 + (k + 1) * LANES - 1) >> 2;
    const int o = f_lds_row(i >> 2, (I0 + k * LANES) >> 2, hi < R_LAST ? hi : R_LAST) * TP + (i & 3) * 4;
    fv[k] = (f32x4){act[o], act[o + 1], act[o + 2], act[o + 3]};
  }
#pragma unroll
  for (int k = 0; k < ROUNDS; ++k) {
    const int i = I0 + k * LANES + me;
    if (I0 + (k + 1) * LANES <= I1 || i < I1)
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(fu32x4, fv[k]), rs, i * 16, 0, f_seg_sc1(S0) ? 16 : 0);
  }
}

}  // namespace p2c_train

// p2c_train_stream.hip: the throughput form of the first launch. *_supported: the descriptor is one the kernel implements
// (identity joint maps, CARLA targets with two channels, hips / neck = joints 1 / 8, no world motion).
bool p2c_internal_train_stream_supported(const p2c_pose_head_desc &d);
int p2c_internal_train_stream_launch(const p2c_pose_head_desc &d, const p2c::GradLosses &gl, const p2c_train::ClipArgs &m, hipStream_t stream);
