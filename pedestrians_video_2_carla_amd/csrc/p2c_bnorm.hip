// p2c_bnorm.hip -- K19: BatchNorm1d (training or eval) + ReLU + dropout (+ residual add) over a row-major (N, C) fp32 activation,
// forward and backward (gfx950).
//
// The pose-lifting baseline (modules/movements/baseline_3d_pose/linear_model.py) normalises the output of every hidden Linear
// layer over the N = B T frames of a batch, then applies ReLU and dropout; a residual block adds its input. The framework runs
// that as four to six kernels per layer, each a full pass over the (N, C) activation, and a dropout mask tensor. Here:
//   forward (train):  K19a  per (column tile, row slab): shifted sums of y over the slab's rows -> slab (mean, M2);
//                     K19b  per column: the slabs' (mean, M2) combined in slab order (Chan et al.) -> mean, rstd; running
//                           statistics updated in place (momentum, unbiased variance, as nn.BatchNorm1d);
//                     K19c  z = relu(gamma (y - mean) rstd + beta) keep(e) / (1 - p) [+ residual]: one read of y, one write of z.
//   forward (eval):   K19c alone, with the running statistics and no dropout (its first row slab copies them to mean / rstd).
//   backward:         K19d  per (column tile, row slab): sum g and sum g xh, g = dz keep / (1 - p) [pre > 0], xh = (y - mean) rstd;
//                     K19e  per column: the slab partials in slab order -> d beta = sum g, d gamma = sum g xh (written to the
//                           workspace and stored or ADDED into the caller's gradients);
//                     K19f  dy = gamma rstd (g - d beta / N - xh d gamma / N)  (eval statistics: dy = gamma rstd g).
// Nothing but y, mean and rstd is kept for the backward: the ReLU gate is the sign of pre = gamma xh + beta, recomputed with the
// same operations as in the forward (bitwise the same), and the dropout mask comes from the hashed generator of p2c_rec_dev.h
// (element e = r C + c, one site per layer; the forward reads `step`, the backward `next - 1`). No float atomics: every sum has one
// fixed order (a thread's rows in sequence, the four waves of a workgroup in wave order, the slabs in slab order), so results are
// bitwise reproducible from run to run.
// Columns: 64 lanes of a wave cover 64 x VEC consecutive columns (VEC = 4: 16-byte loads and stores, when C % 4 == 0 and the
// row tensors are 16-byte aligned; VEC = 1 otherwise). gamma / beta / statistics are read per column, 4 bytes at a time (they
// may live inside a flat parameter buffer). Row offsets are 64-bit; the host refuses N C >= 2^31 (the hash's element index is 32-bit).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/p2c.h"
#include "p2c_host.h"
#include "p2c_rec_dev.h"

namespace p2c_bnorm {

using p2c_rec::DropRng;
typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int THREADS = 256, WAVES = THREADS / 64;
constexpr int TARGET_BLOCKS = 512;       // (column tile, row slab) workgroups of the reduction passes: 2 per CU
constexpr int MIN_SLAB_ROWS = 32;

struct Plan {
  int vec, tiles, slabs, slab_rows;
};

// The slab split depends on N and C only (the workspace size may not depend on pointer alignment).
__host__ __device__ inline int slab_rows_for(int64_t N, int C) {
  const int64_t tiles256 = (C + 255) / 256;
  const int64_t want = TARGET_BLOCKS / tiles256 > 1 ? TARGET_BLOCKS / tiles256 : 1;
  int64_t rows = (N + want - 1) / want;
  if (rows < MIN_SLAB_ROWS) rows = MIN_SLAB_ROWS;
  return (int)rows;
}
inline Plan plan_for(int64_t N, int C, bool vec4) {
  Plan p;
  p.vec = vec4 ? 4 : 1;
  p.tiles = (C + 64 * p.vec - 1) / (64 * p.vec);
  p.slab_rows = slab_rows_for(N, C);
  p.slabs = (int)((N + p.slab_rows - 1) / p.slab_rows);
  return p;
}

struct Args {
  const float *y, *gamma, *beta, *residual, *g_z, *stat_mean, *stat_b;   // stat_b: rstd (train) or running_var (eval)
  float *z, *g_y, *g_gamma, *g_beta, *mean, *rstd, *running_mean, *running_var, *part, *sums;
  int64_t N;
  int32_t C, tiles, slabs, slab_rows, relu, from_var, accumulate;
  float eps, momentum;
  DropRng drop;
};

template <int VEC>
struct Vec {
  float v[VEC];
};
template <int VEC>
__device__ __forceinline__ Vec<VEC> load_row(const float *base, int64_t r, int C, int c) {
  Vec<VEC> o;
  const float *p = base + r * (int64_t)C + c;
  if constexpr (VEC == 4) {
    const f32x4 t = *reinterpret_cast<const f32x4 *>(p);
    o.v[0] = t[0], o.v[1] = t[1], o.v[2] = t[2], o.v[3] = t[3];
  } else {
    o.v[0] = *p;
  }
  return o;
}
template <int VEC>
__device__ __forceinline__ void store_row(float *base, int64_t r, int C, int c, const Vec<VEC> &o) {
  float *p = base + r * (int64_t)C + c;
  if constexpr (VEC == 4)
    *reinterpret_cast<f32x4 *>(p) = (f32x4){o.v[0], o.v[1], o.v[2], o.v[3]};
  else
    *p = o.v[0];
}
template <int VEC>
__device__ __forceinline__ Vec<VEC> drop_row(const DropRng &d, uint32_t e) {
  Vec<VEC> o;
#pragma unroll
  for (int j = 0; j < VEC; ++j) o.v[j] = d.state ? p2c_rec::drop_value(d, e + j) : 1.f;
  return o;
}

// Per-column affine of the normalisation: pre = y a + b with a = gamma rstd, b = beta - mean a. The forward and the backward
// form pre with these exact operations (explicit fma, nothing for the compiler to contract differently), so the ReLU gate the
// backward recomputes is the forward's, bit for bit.
__device__ __forceinline__ float col_a(float gamma, float rstd) { return gamma * rstd; }
__device__ __forceinline__ float col_b(float beta, float mean, float a) { return fmaf(-mean, a, beta); }
__device__ __forceinline__ float pre_of(float y, float a, float b) { return fmaf(y, a, b); }

__device__ __forceinline__ void tile_of(const Args &a, int VEC, int &c, int64_t &r0, int64_t &r1) {
  const int tile = blockIdx.x % a.tiles, slab = blockIdx.x / a.tiles;
  c = (tile * 64 + (threadIdx.x & 63)) * VEC;
  r0 = (int64_t)slab * a.slab_rows;
  r1 = r0 + a.slab_rows < a.N ? r0 + a.slab_rows : a.N;
}

// ---- K19a: slab statistics. Sums of (y - k) with k = y[r0, c] (the slab's first row: no cancellation for large means) ----------
template <int VEC>
__global__ __launch_bounds__(THREADS) void stats_kernel(const Args a) {
  __shared__ float lds[2][WAVES][64 * VEC];
  int c;
  int64_t r0, r1;
  tile_of(a, VEC, c, r0, r1);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const bool on = c < a.C;
  float s1[VEC], s2[VEC];
  Vec<VEC> k;
#pragma unroll
  for (int j = 0; j < VEC; ++j) s1[j] = s2[j] = 0.f, k.v[j] = 0.f;
  if (on) {
    k = load_row<VEC>(a.y, r0, a.C, c);
#pragma unroll 4
    for (int64_t r = r0 + wave; r < r1; r += WAVES) {
      const Vec<VEC> v = load_row<VEC>(a.y, r, a.C, c);
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const float d = v.v[j] - k.v[j];
        s1[j] += d, s2[j] = fmaf(d, d, s2[j]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < VEC; ++j) lds[0][wave][lane * VEC + j] = s1[j], lds[1][wave][lane * VEC + j] = s2[j];
  __syncthreads();
  if (wave != 0 || !on) return;
  const float n = (float)(r1 - r0);
  const int slab = blockIdx.x / a.tiles;
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    float t1 = 0.f, t2 = 0.f;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) t1 += lds[0][w][lane * VEC + j], t2 += lds[1][w][lane * VEC + j];
    const float m = t1 / n;
    a.part[(int64_t)slab * a.C + c + j] = k.v[j] + m;                                   // slab mean
    a.part[((int64_t)a.slabs + slab) * a.C + c + j] = fmaxf(fmaf(-t1, m, t2), 0.f);     // slab M2 = S2 - S1^2 / n
  }
}

// ---- K19b: per column, the slabs combined in slab order; wave w takes slabs w, w + 4, ..., then the four in wave order -----------
__global__ __launch_bounds__(THREADS) void stats_finalize_kernel(const Args a) {
  __shared__ float lds[3][WAVES][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, c = blockIdx.x * 64 + lane;
  const bool on = c < a.C;
  float n = 0.f, mean = 0.f, m2 = 0.f;
  if (on)
    for (int s = wave; s < a.slabs; s += WAVES) {
      const float nb = (float)((int64_t)s * a.slab_rows + a.slab_rows <= a.N ? a.slab_rows : a.N - (int64_t)s * a.slab_rows);
      const float mb = a.part[(int64_t)s * a.C + c], m2b = a.part[((int64_t)a.slabs + s) * a.C + c];
      if (n == 0.f) {      // a wave's first slab is taken as it is: combined with the empty (0, 0, 0), (mb - 0)^2 * 0 is inf * 0 once
        n = nb, mean = mb, m2 = m2b;      // mb^2 leaves fp32 (|mean| > 1.8e19); the same bits otherwise
        continue;
      }
      const float nn = n + nb, d = mb - mean;
      mean = fmaf(d, nb / nn, mean);
      m2 = m2 + m2b + d * d * (n * nb / nn);
      n = nn;
    }
  lds[0][wave][lane] = n, lds[1][wave][lane] = mean, lds[2][wave][lane] = m2;
  __syncthreads();
  if (wave != 0 || !on) return;
  n = lds[0][0][lane], mean = lds[1][0][lane], m2 = lds[2][0][lane];
#pragma unroll
  for (int w = 1; w < WAVES; ++w) {
    const float nb = lds[0][w][lane];
    if (nb == 0.f) continue;
    const float mb = lds[1][w][lane], m2b = lds[2][w][lane];
    const float nn = n + nb, d = mb - mean;
    mean = fmaf(d, nb / nn, mean);
    m2 = m2 + m2b + d * d * (n * nb / nn);
    n = nn;
  }
  const float N = (float)a.N;
  a.mean[c] = mean;
  a.rstd[c] = 1.f / sqrtf(m2 / N + a.eps);
  if (a.running_mean) {
    const float mo = a.momentum;
    a.running_mean[c] = (1.f - mo) * a.running_mean[c] + mo * mean;
    a.running_var[c] = (1.f - mo) * a.running_var[c] + mo * (m2 / (N - 1.f));
  }
}

// ---- K19c: the element-wise pass ----------------------------------------------------------------------------------------------
template <int VEC>
__global__ __launch_bounds__(THREADS) void apply_fwd_kernel(Args a) {
  p2c_rec::drop_begin(a.drop, false);
  int c;
  int64_t r0, r1;
  tile_of(a, VEC, c, r0, r1);
  const int wave = threadIdx.x >> 6;
  float ca[VEC], cb[VEC];
  const bool on = c < a.C;
  const bool keep_stats = a.from_var && on && wave == 0 && blockIdx.x < a.tiles;    // eval: slab 0 leaves mean / rstd for a backward
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    const float sb = on ? a.stat_b[c + j] : 1.f, m = on ? a.stat_mean[c + j] : 0.f;
    const float rstd = a.from_var ? 1.f / sqrtf(sb + a.eps) : sb;
    ca[j] = on ? col_a(a.gamma[c + j], rstd) : 0.f;
    cb[j] = on ? col_b(a.beta[c + j], m, ca[j]) : 0.f;
    if (keep_stats) a.mean[c + j] = m, a.rstd[c + j] = rstd;
  }
  p2c_rec::drop_keys(a.drop, false);
  if (!on) return;
#pragma unroll 4
  for (int64_t r = r0 + wave; r < r1; r += WAVES) {
    Vec<VEC> v = load_row<VEC>(a.y, r, a.C, c);
    const Vec<VEC> k = drop_row<VEC>(a.drop, (uint32_t)(r * a.C + c));
    Vec<VEC> res;
    if (a.residual) res = load_row<VEC>(a.residual, r, a.C, c);
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      float p = pre_of(v.v[j], ca[j], cb[j]);
      if (a.relu) p = fmaxf(p, 0.f);
      v.v[j] = p * k.v[j];
      if (a.residual) v.v[j] += res.v[j];
    }
    store_row<VEC>(a.z, r, a.C, c, v);
  }
}

// g = dz keep / (1 - p) [pre > 0] and xh = (y - mean) rstd of one row's columns
template <int VEC>
__device__ __forceinline__ void grad_row(const Args &a, int64_t r, int c, const float *ca, const float *cb, const float *mean,
                                         const float *rstd, float *g, float *xh) {
  const Vec<VEC> v = load_row<VEC>(a.y, r, a.C, c);
  const Vec<VEC> dz = load_row<VEC>(a.g_z, r, a.C, c);
  const Vec<VEC> k = drop_row<VEC>(a.drop, (uint32_t)(r * a.C + c));
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    const bool pass = !a.relu || pre_of(v.v[j], ca[j], cb[j]) > 0.f;
    g[j] = pass ? dz.v[j] * k.v[j] : 0.f;
    xh[j] = (v.v[j] - mean[j]) * rstd[j];
  }
}

template <int VEC>
__device__ __forceinline__ bool load_cols(const Args &a, int c, float *ca, float *cb, float *mean, float *rstd) {
  const bool on = c < a.C;
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    mean[j] = on ? a.mean[c + j] : 0.f;
    rstd[j] = on ? a.rstd[c + j] : 0.f;
    ca[j] = on ? col_a(a.gamma[c + j], rstd[j]) : 0.f;
    cb[j] = on ? col_b(a.beta[c + j], mean[j], ca[j]) : 0.f;
  }
  return on;
}

// ---- K19d: slab partials of sum g, sum g xh --------------------------------------------------------------------------------------
template <int VEC>
__global__ __launch_bounds__(THREADS) void reduce_bwd_kernel(Args a) {
  __shared__ float lds[2][WAVES][64 * VEC];
  p2c_rec::drop_begin(a.drop, true);
  int c;
  int64_t r0, r1;
  tile_of(a, VEC, c, r0, r1);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float ca[VEC], cb[VEC], mean[VEC], rstd[VEC], sg[VEC], sx[VEC];
  const bool on = load_cols<VEC>(a, c, ca, cb, mean, rstd);
  p2c_rec::drop_keys(a.drop, true);
#pragma unroll
  for (int j = 0; j < VEC; ++j) sg[j] = sx[j] = 0.f;
  if (on) {
#pragma unroll 4
    for (int64_t r = r0 + wave; r < r1; r += WAVES) {
      float g[VEC], xh[VEC];
      grad_row<VEC>(a, r, c, ca, cb, mean, rstd, g, xh);
#pragma unroll
      for (int j = 0; j < VEC; ++j) sg[j] += g[j], sx[j] = fmaf(g[j], xh[j], sx[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < VEC; ++j) lds[0][wave][lane * VEC + j] = sg[j], lds[1][wave][lane * VEC + j] = sx[j];
  __syncthreads();
  if (wave != 0 || !on) return;
  const int slab = blockIdx.x / a.tiles;
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    float t1 = 0.f, t2 = 0.f;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) t1 += lds[0][w][lane * VEC + j], t2 += lds[1][w][lane * VEC + j];
    a.part[(int64_t)slab * a.C + c + j] = t1;
    a.part[((int64_t)a.slabs + slab) * a.C + c + j] = t2;
  }
}

// ---- K19e: per column, the slab partials in slab order -> d beta, d gamma ------------------------------------------------------
__global__ __launch_bounds__(THREADS) void reduce_finalize_kernel(const Args a) {
  __shared__ float lds[2][WAVES][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, c = blockIdx.x * 64 + lane;
  const bool on = c < a.C;
  float sb = 0.f, sg = 0.f;
  if (on)
    for (int s = wave; s < a.slabs; s += WAVES)
      sb += a.part[(int64_t)s * a.C + c], sg += a.part[((int64_t)a.slabs + s) * a.C + c];
  lds[0][wave][lane] = sb, lds[1][wave][lane] = sg;
  __syncthreads();
  if (wave != 0 || !on) return;
  sb = sg = 0.f;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) sb += lds[0][w][lane], sg += lds[1][w][lane];
  a.sums[c] = sb;
  a.sums[a.C + c] = sg;
  if (a.accumulate)
    a.g_beta[c] += sb, a.g_gamma[c] += sg;
  else
    a.g_beta[c] = sb, a.g_gamma[c] = sg;
}

// ---- K19f: dy = gamma rstd (g - d beta / N - xh d gamma / N) -------------------------------------------------------------------
template <int VEC>
__global__ __launch_bounds__(THREADS) void apply_bwd_kernel(Args a) {
  p2c_rec::drop_begin(a.drop, true);
  int c;
  int64_t r0, r1;
  tile_of(a, VEC, c, r0, r1);
  const int wave = threadIdx.x >> 6;
  float ca[VEC], cb[VEC], mean[VEC], rstd[VEC], mb[VEC], mg[VEC];
  const bool on = load_cols<VEC>(a, c, ca, cb, mean, rstd);
  const float inv_n = a.from_var ? 0.f : 1.f / (float)a.N;     // eval statistics are constants: no batch-statistics terms
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    mb[j] = on ? a.sums[c + j] * inv_n : 0.f;
    mg[j] = on ? a.sums[a.C + c + j] * inv_n : 0.f;
  }
  p2c_rec::drop_keys(a.drop, true);
  if (!on) return;
#pragma unroll 4
  for (int64_t r = r0 + wave; r < r1; r += WAVES) {
    float g[VEC], xh[VEC];
    grad_row<VEC>(a, r, c, ca, cb, mean, rstd, g, xh);
    Vec<VEC> o;
#pragma unroll
    for (int j = 0; j < VEC; ++j) o.v[j] = ca[j] * (g[j] - mb[j] - xh[j] * mg[j]);
    store_row<VEC>(a.g_y, r, a.C, c, o);
  }
}

inline bool shape_ok(int64_t N, int32_t C) { return N >= 1 && C >= 1 && N * (int64_t)C < ((int64_t)1 << 31); }

inline void set_drop(Args &a, const p2c_bnorm_desc *d) {
  a.drop = (d->drop_state && d->drop_p > 0.f) ? DropRng(d->drop_state, d->drop_p, d->drop_site) : DropRng{};
}

#define P2C_BN_LAUNCH(kernel, vec, grid)                                                                                  \
  do {                                                                                                                    \
    if ((vec) == 4)                                                                                                       \
      hipLaunchKernelGGL(kernel<4>, grid, dim3(THREADS), 0, (hipStream_t)stream, a);                                      \
    else                                                                                                                  \
      hipLaunchKernelGGL(kernel<1>, grid, dim3(THREADS), 0, (hipStream_t)stream, a);                                      \
  } while (0)

}  // namespace p2c_bnorm

extern "C" int64_t p2c_bnorm_workspace_floats(int64_t N, int32_t C) {
  using namespace p2c_bnorm;
  if (!shape_ok(N, C)) return 0;
  const int64_t slabs = (N + slab_rows_for(N, C) - 1) / slab_rows_for(N, C);
  return 2 * slabs * C + 2 * (int64_t)C;
}

extern "C" int p2c_bnorm_fwd(const p2c_bnorm_desc *d, float *workspace, void *stream) {
  using namespace p2c_bnorm;
  if (!d) return P2C_E_NULL;
  if (!shape_ok(d->N, d->C) || (d->training && d->N < 2)) return P2C_E_SHAPE;
  if (!d->y || !d->gamma || !d->beta || !d->z || !d->mean || !d->rstd) return P2C_E_NULL;
  if (d->training ? !workspace : (!d->running_mean || !d->running_var)) return P2C_E_NULL;
  if ((d->running_mean == nullptr) != (d->running_var == nullptr)) return P2C_E_NULL;
  const bool vec4 = d->C % 4 == 0 && p2c_host::aligned16(d->y, d->z, d->residual);
  const Plan p = plan_for(d->N, d->C, vec4);
  Args a{};
  a.y = d->y, a.gamma = d->gamma, a.beta = d->beta, a.residual = d->residual, a.z = d->z;
  a.mean = d->mean, a.rstd = d->rstd, a.part = workspace, a.N = d->N, a.C = d->C, a.tiles = p.tiles, a.slabs = p.slabs;
  a.slab_rows = p.slab_rows, a.relu = d->relu, a.eps = d->eps, a.momentum = d->momentum;
  const dim3 grid((unsigned)((int64_t)p.tiles * p.slabs));
  if (d->training) {
    a.running_mean = d->running_mean, a.running_var = d->running_var;
    P2C_BN_LAUNCH(stats_kernel, p.vec, grid);
    hipLaunchKernelGGL(stats_finalize_kernel, dim3((unsigned)((d->C + 63) / 64)), dim3(THREADS), 0, (hipStream_t)stream, a);
    a.stat_mean = d->mean, a.stat_b = d->rstd, a.from_var = 0;
    set_drop(a, d);
  } else {
    // eval: the running statistics, no dropout; the element-wise pass also leaves them in mean / rstd for a backward
    a.stat_mean = d->running_mean, a.stat_b = d->running_var, a.from_var = 1;
    a.drop = DropRng{};
  }
  P2C_BN_LAUNCH(apply_fwd_kernel, p.vec, grid);
  return p2c_host::launch_status();
}

extern "C" int p2c_bnorm_bwd(const p2c_bnorm_desc *d, float *workspace, void *stream) {
  using namespace p2c_bnorm;
  if (!d) return P2C_E_NULL;
  if (!shape_ok(d->N, d->C) || (d->training && d->N < 2)) return P2C_E_SHAPE;
  if (!d->y || !d->gamma || !d->beta || !d->mean || !d->rstd || !d->g_z || !d->g_y || !d->g_gamma || !d->g_beta || !workspace)
    return P2C_E_NULL;
  const bool vec4 = d->C % 4 == 0 && p2c_host::aligned16(d->y, d->g_z, d->g_y);
  const Plan p = plan_for(d->N, d->C, vec4);
  Args a{};
  a.y = d->y, a.gamma = d->gamma, a.beta = d->beta, a.g_z = d->g_z, a.g_y = d->g_y, a.g_gamma = d->g_gamma, a.g_beta = d->g_beta;
  a.mean = d->mean, a.rstd = d->rstd, a.part = workspace, a.sums = workspace + 2 * (int64_t)p.slabs * d->C;
  a.N = d->N, a.C = d->C, a.tiles = p.tiles, a.slabs = p.slabs, a.slab_rows = p.slab_rows, a.relu = d->relu;
  a.accumulate = d->accumulate, a.from_var = !d->training;
  if (d->training)
    set_drop(a, d);
  const dim3 grid((unsigned)((int64_t)p.tiles * p.slabs));
  P2C_BN_LAUNCH(reduce_bwd_kernel, p.vec, grid);
  hipLaunchKernelGGL(reduce_finalize_kernel, dim3((unsigned)((d->C + 63) / 64)), dim3(THREADS), 0, (hipStream_t)stream, a);
  P2C_BN_LAUNCH(apply_bwd_kernel, p.vec, grid);
  return p2c_host::launch_status();
}
