// p2c_heatmaps.hip -- K28: the heatmap head of the pose-estimation flow (gfx950): target maps, their loss, the decode.
//
// Reference: data/base/mixins/dataset/video_mixin.py:186-225 (_add_heatmaps_to_targets / _get_heatmap: a Python loop over joints,
// each a full-resolution np.mgrid Gaussian of utils/gaussian_kernel.py:5-14, background = 1 - max), the target resize of
// modules/flow/pose_estimation.py:96-107 (avg_pool2d(9, 8, 1)), loss/heatmaps_loss.py:9-48 over loss/base_pose_loss.py:68-86
// (sum_per_frame: a Python loop over frames with boolean gathers and an isnan host sync each), and
// modules/flow/pose_estimation.py:113-134 (_keypoints_from_heatmaps: a triple loop with a .max() host sync per map).
//
// K28a  heatmap_targets_kernel. One lane per output cell of one frame, every channel of that cell. The frame's J centres
//   c = rint((kp - shift) * scale) are formed once per workgroup into LDS, next to the Gaussian table g[d2] the host built in
//   fp64 (both clamps of the reference applied, then the cast): sigma is an integer, so d2 is one, and g[d2] is the reference's
//   value bit for bit. A joint whose support box (|dx|, |dy| <= r, r = isqrt(table entries - 1)) misses the cell's window is
//   skipped: its cell is the literal 0.0f. The others add g over window x support x frame in (row, column) order; the
//   background adds 1 - max_j g_j over the window's in-frame pixels; both are divided by k k (padding counts, contributes 0).
//   Full resolution is the k = 1, stride 1, padding 0 pool: 0 + g, divided by 1 -- the table's bits. The full-resolution
//   tensor is never formed.
// K28b  heatmaps_loss_{maps,finish,bwd}_kernel. (1) one wavefront per (b, t, k) pair: the selection flag (mask off, or
//   k == forced, or every cell of the target map != 0) and the pair's sum of squares, lanes over cells, xor tree. (2) one
//   workgroup: wavefront w takes frames w, w + 4, ...: S_t and n_t over the selected (b, k) in fp64, lane l adding entries
//   l, l + 64, ... in order, then the tree; term_t = S_t / (n_t h w) unless n_t = 0 or S_t is NaN (the reference's isnan
//   skip), coefficient_t = 2 / (n_t h w) or 0; the four wavefronts' running sums are added in wavefront order. Fixed order
//   everywhere, no float atomics. (3) backward: one workgroup per (b, t, channel) map of the prediction; it walks the pair
//   list (a kernel argument), adds pred - gt of every selected pair that names this channel and scales by
//   grad_loss coefficient_t; a zero coefficient writes the literal 0 (a skipped frame's NaN must not come back as 0 * NaN).
// K28c  heatmap_keypoints_kernel. One wavefront per map of channels 1..P-1: each lane keeps (max, first index, saw-a-NaN)
//   over its cells, the tree combines them (greater value, then smaller index); c > 0 and no NaN writes
//   (col sw, row sh, c), anything else zeros.
// Bounds: every load is indexed from a counter compared against the map's own size; element offsets are 64-bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/p2c.h"
#include "p2c_lane_dev.h"
#include "p2c_host.h"

namespace p2c_hm {

constexpr int kMaxMaps = P2C_HEATMAPS_MAX_MAPS;      // 64: channels per frame, and pairs of the loss
constexpr int kMaxTable = P2C_HEATMAPS_MAX_TABLE;    // 1024 entries of g[d2]
constexpr int kMaxPool = P2C_HEATMAPS_MAX_POOL;      // 32
constexpr int kFar = 1 << 30;                        // a centre nobody's window reaches (non-finite or huge keypoints)

__device__ __forceinline__ int centre(float kp, float shift, float scale) {
  const float v = rintf(__fmul_rn(__fsub_rn(kp, shift), scale));   // fp32, in the reference's order, round-half-even
  if (!(v > -(float)kFar && v < (float)kFar)) return -kFar;        // NaN lands here too
  return (int)v;
}

struct TargetArgs {
  const float *kp, *shift, *table;
  float *out;
  int64_t N;
  int32_t J, H, W, k, s, p, oh, ow, n_table, r, blocks_per_frame;
  float scale_x, scale_y, kk;
};

__global__ __launch_bounds__(256) void heatmap_targets_kernel(const TargetArgs a) {
  __shared__ float g[kMaxTable];
  __shared__ int cx[kMaxMaps], cy[kMaxMaps];
  const int64_t frame = (int64_t)blockIdx.x / a.blocks_per_frame;
  const int chunk = (int)((int64_t)blockIdx.x - frame * a.blocks_per_frame);
  for (int i = threadIdx.x; i < a.n_table; i += 256) g[i] = a.table[i];
  if ((int)threadIdx.x < a.J) {
    const float *kp = a.kp + ((size_t)frame * a.J + threadIdx.x) * 2, *sh = a.shift + (size_t)frame * 2;
    cx[threadIdx.x] = centre(kp[0], sh[0], a.scale_x);
    cy[threadIdx.x] = centre(kp[1], sh[1], a.scale_y);
  }
  __syncthreads();
  const int cells = a.oh * a.ow, cell = chunk * 256 + (int)threadIdx.x;
  if (cell >= cells) return;
  const int orow = cell / a.ow, ocol = cell - orow * a.ow;
  // the window, clipped to the frame (never empty: p < k)
  const int y0 = max(orow * a.s - a.p, 0), y1 = min(orow * a.s - a.p + a.k, a.H);
  const int x0 = max(ocol * a.s - a.p, 0), x1 = min(ocol * a.s - a.p + a.k, a.W);
  float *out = a.out + (size_t)frame * (a.J + 1) * cells + cell;
  uint64_t near = 0;                                               // joints whose support box meets the window
  for (int j = 0; j < a.J; ++j) {
    const int jx0 = max(x0, cx[j] - a.r), jx1 = min(x1, cx[j] + a.r + 1);
    const int jy0 = max(y0, cy[j] - a.r), jy1 = min(y1, cy[j] + a.r + 1);
    float acc = 0.f;
    if (jx0 < jx1 && jy0 < jy1) {
      near |= (uint64_t)1 << j;
      for (int y = jy0; y < jy1; ++y) {
        const int dy2 = (y - cy[j]) * (y - cy[j]);
        for (int x = jx0; x < jx1; ++x) {
          const int d2 = dy2 + (x - cx[j]) * (x - cx[j]);
          if (d2 < a.n_table) acc += g[d2];
        }
      }
      if (a.k != 1) acc /= a.kk;                                   // k = 1: one addend, 0 + g -- the table's bits
    }
    out[(size_t)(j + 1) * cells] = acc;
  }
  float bg = 0.f;
  for (int y = y0; y < y1; ++y)
    for (int x = x0; x < x1; ++x) {
      float m = 0.f;
      for (uint64_t left = near; left; left &= left - 1) {
        const int j = __builtin_ctzll(left);
        const int dx = x - cx[j], dy = y - cy[j];
        if (dx >= -a.r && dx <= a.r && dy >= -a.r && dy <= a.r) {
          const int d2 = dx * dx + dy * dy;
          if (d2 < a.n_table) m = fmaxf(m, g[d2]);
        }
      }
      bg += 1.f - m;
    }
  out[0] = a.k == 1 ? bg : bg / a.kk;
}

// ---- K28b ---------------------------------------------------------------------------------------------------------------------
struct LossArgs {
  const float *pred, *gt;
  float *partials, *coef, *loss, *grad_pred;
  int32_t *flags;
  const float *grad_loss;
  int64_t B;
  int32_t T, Pp, Pg, cells, K, forced, mask;
  int32_t pred_channels[kMaxMaps], gt_channels[kMaxMaps];
};


__global__ __launch_bounds__(64) void heatmaps_loss_maps_kernel(const LossArgs a) {
  const int64_t pair = blockIdx.x;                                 // (b, t, k), k fastest
  const int k = (int)(pair % a.K);
  const int64_t bt = pair / a.K;
  const float *p = a.pred + ((size_t)bt * a.Pp + a.pred_channels[k]) * a.cells;
  const float *q = a.gt + ((size_t)bt * a.Pg + a.gt_channels[k]) * a.cells;
  float acc = 0.f;
  int zeros = 0;
  for (int i = threadIdx.x; i < a.cells; i += 64) {
    const float t = q[i], d = p[i] - t;
    acc = fmaf(d, d, acc);
    zeros |= !(t != 0.f);                                          // a NaN target cell is != 0, as in the reference
  }
  acc = p2c_lane::xor_sum<64>(acc);
  const int any_zero = __any(zeros);
  if (threadIdx.x == 0) {
    a.partials[pair] = acc;
    a.flags[pair] = (!a.mask || k == a.forced || !any_zero) ? 1 : 0;
  }
}

__global__ __launch_bounds__(256) void heatmaps_loss_finish_kernel(const LossArgs a) {
  __shared__ double part[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t per_frame = a.B * a.K;                             // entries of one frame: (b, k)
  double total = 0.0;
  for (int t = wave; t < a.T; t += 4) {
    double s = 0.0, n = 0.0;
    for (int64_t e = lane; e < per_frame; e += 64) {
      const int64_t b = e / a.K, pair = (b * a.T + t) * a.K + (e - b * a.K);
      if (a.flags[pair]) s += (double)a.partials[pair], n += 1.0;
    }
    s = p2c_lane::xor_sum<64>(s), n = p2c_lane::xor_sum<64>(n);
    const bool use = n > 0.0 && !(s != s);
    const double div = n * (double)a.cells;
    if (use) total += s / div;
    if (lane == 0) a.coef[t] = use ? (float)(2.0 / div) : 0.f;
  }
  if (lane == 0) part[wave] = total;
  __syncthreads();
  if (threadIdx.x == 0) *a.loss = (float)(((part[0] + part[1]) + part[2]) + part[3]);
}

__global__ __launch_bounds__(256) void heatmaps_loss_bwd_kernel(const LossArgs a) {
  const int64_t map = blockIdx.x;                                  // (b, t, c) of the prediction
  const int c = (int)(map % a.Pp);
  const int64_t bt = map / a.Pp;
  const int t = (int)(bt % a.T);
  float *gp = a.grad_pred + (size_t)map * a.cells;
  const float coef = a.coef[t];
  const float *p = a.pred + (size_t)map * a.cells;
  uint64_t sel = 0;                                                // workgroup-uniform: the selected pairs that name this channel
  if (coef != 0.f)
    for (int k = 0; k < a.K; ++k)
      if (a.pred_channels[k] == c && a.flags[bt * a.K + k]) sel |= (uint64_t)1 << k;
  if (sel == 0) {
    for (int i = threadIdx.x; i < a.cells; i += 256) gp[i] = 0.f;
    return;
  }
  const float scale = coef * *a.grad_loss;
  const float *g0 = a.gt + (size_t)bt * a.Pg * a.cells;
  for (int i = threadIdx.x; i < a.cells; i += 256) {
    const float v = p[i];
    float d = 0.f;
    for (uint64_t left = sel; left; left &= left - 1)              // in pair order
      d += v - g0[(size_t)a.gt_channels[__builtin_ctzll(left)] * a.cells + i];
    gp[i] = d * scale;
  }
}

// ---- K28c ---------------------------------------------------------------------------------------------------------------------
struct DecodeArgs {
  const float *maps;
  float *out;
  int32_t P, h, w;
  float sw, sh;
};

__global__ __launch_bounds__(64) void heatmap_keypoints_kernel(const DecodeArgs a) {
  const int64_t item = blockIdx.x;                                 // (frame, joint)
  const int64_t frame = item / (a.P - 1);
  const int joint = (int)(item - frame * (a.P - 1));
  const int cells = a.h * a.w;
  const float *m = a.maps + ((size_t)frame * a.P + joint + 1) * cells;
  float best = -INFINITY;
  int idx = 0, nan = 0;
  for (int i = threadIdx.x; i < cells; i += 64) {
    const float v = m[i];
    nan |= v != v;
    if (v > best) best = v, idx = i;                               // strict: the lane's first index of its maximum
  }
  if (best == -INFINITY) idx = 0x7fffffff;                         // a lane that saw nothing above -inf yields to any other
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const float ob = __shfl_xor(best, d, 64);
    const int oi = __shfl_xor(idx, d, 64);
    if (ob > best || (ob == best && oi < idx)) best = ob, idx = oi;
  }
  const int any_nan = __any(nan);
  if (threadIdx.x == 0) {
    float *o = a.out + (size_t)item * 3;
    if (!any_nan && best > 0.f) {
      const int row = idx / a.w, col = idx - row * a.w;
      o[0] = (float)col * a.sw, o[1] = (float)row * a.sh, o[2] = best;
    } else {
      o[0] = 0.f, o[1] = 0.f, o[2] = 0.f;
    }
  }
}

constexpr int64_t kMaxElems = ((int64_t)1 << 31) - 1;              // grids are one-dimensional: < 2^31 workgroups

static int isqrt_floor(int v) {
  int r = 0;
  while ((r + 1) * (r + 1) <= v) ++r;
  return r;
}

static int check_targets(const p2c_heatmap_targets_desc *d, TargetArgs &a) {
  if (!d) return P2C_E_NULL;
  if (d->N < 0 || d->J < 1 || d->J > kMaxMaps - 1 || d->H < 1 || d->W < 1 || d->H > (1 << 20) || d->W > (1 << 20))
    return P2C_E_SHAPE;
  if (d->n_table < 1 || d->n_table > kMaxTable) return P2C_E_SHAPE;
  if (d->k < 1 || d->k > kMaxPool || d->s < 1 || d->p < 0 || 2 * d->p > d->k) return P2C_E_SHAPE;   // avg_pool2d's own rule
  if (d->H + 2 * d->p < d->k || d->W + 2 * d->p < d->k) return P2C_E_SHAPE;
  const int oh = (d->H + 2 * d->p - d->k) / d->s + 1, ow = (d->W + 2 * d->p - d->k) / d->s + 1;
  if (d->oh != oh || d->ow != ow) return P2C_E_SHAPE;
  const int64_t cells = (int64_t)oh * ow, bpf = (cells + 255) / 256;
  if (cells > kMaxElems || (d->N > 0 && bpf > kMaxElems / d->N)) return P2C_E_SHAPE;
  if (d->N > 0 && (!d->kp || !d->shift || !d->table || !d->out)) return P2C_E_NULL;
  a.kp = d->kp, a.shift = d->shift, a.table = d->table, a.out = d->out, a.N = d->N;
  a.J = d->J, a.H = d->H, a.W = d->W, a.k = d->k, a.s = d->s, a.p = d->p, a.oh = oh, a.ow = ow, a.n_table = d->n_table;
  a.r = isqrt_floor(d->n_table - 1), a.blocks_per_frame = (int)bpf;
  a.scale_x = d->scale_x, a.scale_y = d->scale_y, a.kk = (float)(d->k * d->k);
  return 0;
}

static int check_loss(const p2c_heatmaps_loss_desc *d, bool bwd, LossArgs &a) {
  if (!d) return P2C_E_NULL;
  if ((d->mask | 1) != 1) return P2C_E_ENUM;
  if (d->B < 0 || d->T < 1 || d->Pp < 1 || d->Pp > kMaxMaps || d->Pg < 1 || d->Pg > kMaxMaps || d->h < 1 || d->w < 1 ||
      d->K < 1 || d->K > kMaxMaps || d->forced < -1 || d->forced >= d->K)
    return P2C_E_SHAPE;
  for (int k = 0; k < d->K; ++k)
    if (d->pred_channels[k] < 0 || d->pred_channels[k] >= d->Pp || d->gt_channels[k] < 0 || d->gt_channels[k] >= d->Pg)
      return P2C_E_SHAPE;
  const int64_t cells = (int64_t)d->h * d->w, maps = (int64_t)d->T * (d->Pp > d->K ? d->Pp : d->K);
  if (cells > kMaxElems || (d->B > 0 && maps > kMaxElems / d->B)) return P2C_E_SHAPE;
  if (!d->pred || !d->gt || !d->partials || !d->flags || !d->coef) return P2C_E_NULL;
  if (bwd ? (!d->grad_pred || !d->grad_loss) : !d->loss) return P2C_E_NULL;
  a.pred = d->pred, a.gt = d->gt, a.partials = d->partials, a.flags = d->flags, a.coef = d->coef, a.loss = d->loss;
  a.grad_pred = d->grad_pred, a.grad_loss = d->grad_loss;
  a.B = d->B, a.T = d->T, a.Pp = d->Pp, a.Pg = d->Pg, a.cells = (int)cells, a.K = d->K, a.forced = d->forced, a.mask = d->mask;
  for (int k = 0; k < d->K; ++k) a.pred_channels[k] = d->pred_channels[k], a.gt_channels[k] = d->gt_channels[k];
  return 0;
}

}  // namespace p2c_hm

using namespace p2c_hm;

static int launched() {
  return p2c_host::launch_status();
}

extern "C" int p2c_heatmap_targets_fwd(const p2c_heatmap_targets_desc *d, void *stream) {
  TargetArgs a{};
  const int rc = check_targets(d, a);
  if (rc) return rc;
  if (d->N == 0) return 0;
  hipLaunchKernelGGL(heatmap_targets_kernel, dim3((unsigned)(a.N * a.blocks_per_frame)), dim3(256), 0, (hipStream_t)stream, a);
  return launched();
}

extern "C" int p2c_heatmaps_loss_fwd(const p2c_heatmaps_loss_desc *d, void *stream) {
  LossArgs a{};
  const int rc = check_loss(d, false, a);
  if (rc) return rc;
  if (d->B > 0) {
    hipLaunchKernelGGL(heatmaps_loss_maps_kernel, dim3((unsigned)(a.B * a.T * a.K)), dim3(64), 0, (hipStream_t)stream, a);
    const int e = launched();
    if (e) return e;
  }
  hipLaunchKernelGGL(heatmaps_loss_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a);   // B = 0: loss 0, coefficients 0
  return launched();
}

extern "C" int p2c_heatmaps_loss_bwd(const p2c_heatmaps_loss_desc *d, void *stream) {
  LossArgs a{};
  const int rc = check_loss(d, true, a);
  if (rc) return rc;
  if (d->B == 0) return 0;
  hipLaunchKernelGGL(heatmaps_loss_bwd_kernel, dim3((unsigned)(a.B * a.T * a.Pp)), dim3(256), 0, (hipStream_t)stream, a);
  return launched();
}

extern "C" int p2c_heatmap_keypoints_fwd(const p2c_heatmap_keypoints_desc *d, void *stream) {
  if (!d) return P2C_E_NULL;
  if (d->N < 0 || d->P < 2 || d->P > kMaxMaps || d->h < 1 || d->w < 1) return P2C_E_SHAPE;
  const int64_t cells = (int64_t)d->h * d->w;
  if (cells > kMaxElems || (d->N > 0 && (int64_t)(d->P - 1) > kMaxElems / d->N)) return P2C_E_SHAPE;
  if (d->N == 0) return 0;
  if (!d->maps || !d->out) return P2C_E_NULL;
  DecodeArgs a{d->maps, d->out, d->P, d->h, d->w, d->sw, d->sh};
  hipLaunchKernelGGL(heatmap_keypoints_kernel, dim3((unsigned)(d->N * (d->P - 1))), dim3(64), 0, (hipStream_t)stream, a);
  return launched();
}
