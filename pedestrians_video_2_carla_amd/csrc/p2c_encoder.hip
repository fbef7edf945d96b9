// p2c_encoder.hip -- K20: the two element-wise / small-matrix halves of a post-norm nn.TransformerEncoderLayer that no other kernel
// of the build covers, forward and backward (gfx950).
//
// SimpleTransformer (modules/movements/transformers.py) runs six torch.nn.TransformerEncoderLayer (post-norm, ReLU, dropout 0.1)
// over B clips of T frame tokens of width d = 2 J: d = 52 for CARLA (4 heads of 13), d = 50 for BODY_25. K14 (p2c_attn.hip) has no
// dropout and K15 (p2c_norm.hip) needs d % 4 == 0; the GEMMs are K16 with the ReLU + dropout epilogues (act 3 / 4).
//
// K20a  attention with dropout on the probabilities, any head width: one workgroup per (sequence, head), N <= 64 tokens.
//       forward : P = softmax(scale q k^T) per row, P' = P keep / (1 - p), out = P' v;
//       backward: P recomputed (same code, same bits), dP' = g_out v^T, dP = dP' keep / (1 - p), dS = P (dP - rowsum(P dP)),
//                 dq = scale dS k, dk = scale dS^T q, dv = P'^T g_out. The scores / probabilities live in LDS (3 x 64 x 65 floats);
//                 q, k, v, g_out are read from global memory (a head's rows are a few KB: L1 / L2 hits after the first touch).
//       Mask element e = ((s heads + h) N + i) N + j of the (S, heads, N, N) probabilities.
// K20b  post-norm residual: z = LayerNorm(x + s keep / (1 - p)), s = the out_proj / linear2 output, any 2 <= D <= 1024.
//       forward : mean, rstd (rows) are saved; the sum u = x + s keep / (1 - p) is not: the backward forms it again (same fma).
//                 u, the row mean and u - mean are formed in fp64 (forward and backward alike, the backward summing the row
//                 again: the saved fp32 mean serves callers only): a row whose elements lie within 1e-3 of each other -- any
//                 row at D = 2 with x1 + s1 ~ x2 + s2 -- loses u - mean to the rounding of u and of the mean in fp32 (seen:
//                 dx 3e-4 of the cancellation scale off, z 2e-5). The squares, rstd and everything behind them stay fp32.
//       backward: dz_pre = rstd (gg - mean(gg) - xh mean(gg xh)), gg = dz gamma, xh = (u - mean) rstd;
//                 dx = dz_pre (the residual branch), ds = dz_pre keep / (1 - p); d gamma = sum_rows dz xh, d beta = sum_rows dz in
//                 per-workgroup partials added in a fixed order by a second launch (K15's scheme: bitwise reproducible).
//       A row belongs to G lanes of a wave, lane l of the row owning columns l, l + G, l + 2 G, ... (every D, 4-byte loads that
//       the G lanes of a row turn into contiguous wave accesses). Mask element e = r D + c.
// Dropout: the hashed stream of p2c_rec_dev.h (state {seed_lo, seed_hi, step, next}); forward launches read `step` and leave
// next = step + 1, backward launches read next - 1 and leave step = next. Indices are 32-bit: the host refuses S heads N^2 >= 2^31
// (K20a) and rows D >= 2^31 (K20b) when a mask is drawn.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/p2c.h"
#include "p2c_host.h"
#include "p2c_lane_dev.h"
#include "p2c_rec_dev.h"

namespace p2c_encoder {

using p2c_lane::xor_max;
using p2c_lane::xor_sum;
using p2c_rec::DropRng;
constexpr int THREADS = 256, WAVES = THREADS / 64, MAXN = 64, PITCH = MAXN + 1;


// ---- K20a ------------------------------------------------------------------------------------------------------------------------
struct AttnArgs {
  const float *qkv, *g_out;
  float *out, *g_qkv;
  int32_t S, N, heads, hd;
  float scale;
  DropRng drop;
};

// P[i][j] = softmax_j(scale q_i . k_j) for the workgroup's (sequence, head); the same operations forward and backward
__device__ __forceinline__ void probabilities(const AttnArgs &a, const float *q, const float *k, int ld, float (*P)[PITCH]) {
  const int N = a.N, hd = a.hd;
  for (int idx = threadIdx.x; idx < N * N; idx += THREADS) {
    const int i = idx / N, j = idx - i * N;
    const float *qi = q + (int64_t)i * ld, *kj = k + (int64_t)j * ld;
    float acc = 0.f;
    for (int c = 0; c < hd; ++c) acc = fmaf(qi[c], kj[c], acc);
    P[i][j] = acc * a.scale;
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int i = wave; i < N; i += WAVES) {
    const float x = lane < N ? P[i][lane] : -INFINITY;
    const float mx = xor_max<64>(x);
    const float e = lane < N ? expf(x - mx) : 0.f;
    const float sum = xor_sum<64>(e);
    if (lane < N) P[i][lane] = e / sum;
  }
  __syncthreads();
}

__global__ __launch_bounds__(THREADS) void attn_fwd_kernel(AttnArgs a) {
  __shared__ float P[MAXN][PITCH];
  const int seq = blockIdx.x / a.heads, h = blockIdx.x - seq * a.heads;
  const int N = a.N, hd = a.hd, d = a.heads * hd, ld = 3 * d;
  p2c_rec::drop_begin(a.drop, false);
  p2c_rec::drop_keys(a.drop, false);
  const float *q = a.qkv + (int64_t)seq * N * ld + h * hd, *k = q + d, *v = q + 2 * d;
  probabilities(a, q, k, ld, P);
  if (a.drop.state) {
    const uint32_t e0 = (uint32_t)blockIdx.x * (uint32_t)(N * N);
    for (int idx = threadIdx.x; idx < N * N; idx += THREADS) {
      const int i = idx / N, j = idx - i * N;
      P[i][j] *= p2c_rec::drop_value(a.drop, e0 + (uint32_t)idx);
    }
    __syncthreads();
  }
  float *o = a.out + (int64_t)seq * N * d + h * hd;
  for (int idx = threadIdx.x; idx < N * hd; idx += THREADS) {
    const int i = idx / hd, c = idx - i * hd;
    float acc = 0.f;
    for (int j = 0; j < N; ++j) acc = fmaf(P[i][j], v[(int64_t)j * ld + c], acc);
    o[(int64_t)i * d + c] = acc;
  }
}

__global__ __launch_bounds__(THREADS) void attn_bwd_kernel(AttnArgs a) {
  __shared__ float P[MAXN][PITCH], Pd[MAXN][PITCH], G[MAXN][PITCH];      // P, P' (dropped), dP -> dS
  const int seq = blockIdx.x / a.heads, h = blockIdx.x - seq * a.heads;
  const int N = a.N, hd = a.hd, d = a.heads * hd, ld = 3 * d;
  p2c_rec::drop_begin(a.drop, true);
  p2c_rec::drop_keys(a.drop, true);
  const float *q = a.qkv + (int64_t)seq * N * ld + h * hd, *k = q + d, *v = q + 2 * d;
  const float *go = a.g_out + (int64_t)seq * N * d + h * hd;
  probabilities(a, q, k, ld, P);
  const uint32_t e0 = (uint32_t)blockIdx.x * (uint32_t)(N * N);
  for (int idx = threadIdx.x; idx < N * N; idx += THREADS) {
    const int i = idx / N, j = idx - i * N;
    const float m = a.drop.state ? p2c_rec::drop_value(a.drop, e0 + (uint32_t)idx) : 1.f;
    const float *gi = go + (int64_t)i * d, *vj = v + (int64_t)j * ld;
    float acc = 0.f;
    for (int c = 0; c < hd; ++c) acc = fmaf(gi[c], vj[c], acc);
    G[i][j] = acc * m;
    Pd[i][j] = P[i][j] * m;
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int i = wave; i < N; i += WAVES) {
    const float pg = lane < N ? P[i][lane] * G[i][lane] : 0.f;
    const float rd = xor_sum<64>(pg);
    if (lane < N) G[i][lane] = P[i][lane] * (G[i][lane] - rd);
  }
  __syncthreads();
  float *gq = a.g_qkv + (int64_t)seq * N * ld + h * hd, *gk = gq + d, *gv = gq + 2 * d;
  for (int idx = threadIdx.x; idx < N * hd; idx += THREADS) {
    const int i = idx / hd, c = idx - i * hd;                 // i: the query row of dq, the key / value row of dk, dv
    float sq = 0.f, sk = 0.f, sv = 0.f;
    for (int j = 0; j < N; ++j) {
      sq = fmaf(G[i][j], k[(int64_t)j * ld + c], sq);
      sk = fmaf(G[j][i], q[(int64_t)j * ld + c], sk);
      sv = fmaf(Pd[j][i], go[(int64_t)j * d + c], sv);
    }
    gq[(int64_t)i * ld + c] = sq * a.scale;
    gk[(int64_t)i * ld + c] = sk * a.scale;
    gv[(int64_t)i * ld + c] = sv;
  }
}

// ---- K20b ------------------------------------------------------------------------------------------------------------------------
struct NormArgs {
  const float *x, *s, *gamma, *beta, *gz;
  float *z, *mean, *rstd, *gx, *gs, *g_gamma, *g_beta, *partials;
  int64_t rows;
  int32_t D, accumulate, n_blocks;
  float eps;
  DropRng drop;
};

__device__ __forceinline__ float keep_of(const DropRng &d, int64_t r, int D, int col) {
  return d.state ? p2c_rec::drop_value(d, (uint32_t)(r * D + col)) : 1.f;
}

// G lanes per row, KV columns per lane: column of (k, l) = k G + l
template <int G, int KV>
__global__ __launch_bounds__(THREADS) void postnorm_fwd_kernel(NormArgs a) {
  constexpr int RPW = 64 / G, RPB = RPW * WAVES;
  const int lane = threadIdx.x & 63, l = lane % G, slot = (threadIdx.x >> 6) * RPW + lane / G;
  const int D = a.D;
  p2c_rec::drop_begin(a.drop, false);
  p2c_rec::drop_keys(a.drop, false);
  float gm[KV], bt[KV];
#pragma unroll
  for (int k = 0; k < KV; ++k) {
    const int col = k * G + l;
    gm[k] = col < D ? a.gamma[col] : 0.f, bt[k] = col < D ? a.beta[col] : 0.f;
  }
  const float inv_d = 1.f / (float)D;
  const double inv_d64 = 1.0 / (double)D;
  for (int64_t r0 = (int64_t)blockIdx.x * RPB; r0 < a.rows; r0 += (int64_t)gridDim.x * RPB) {
    const int64_t r = r0 + slot;
    const bool live = r < a.rows;
    double u[KV], s1 = 0.0;
#pragma unroll
    for (int k = 0; k < KV; ++k) {
      const int col = k * G + l;
      u[k] = 0.0;
      if (live && col < D) u[k] = fma((double)a.s[r * D + col], (double)keep_of(a.drop, r, D, col), (double)a.x[r * D + col]);
      s1 += u[k];
    }
    const double mean = xor_sum<G>(s1) * inv_d64;
    float t[KV], q = 0.f;
#pragma unroll
    for (int k = 0; k < KV; ++k) {
      t[k] = (k * G + l < D) ? (float)(u[k] - mean) : 0.f;
      q = fmaf(t[k], t[k], q);
    }
    const float rstd = rsqrtf(xor_sum<G>(q) * inv_d + a.eps);
    if (!live) continue;
#pragma unroll
    for (int k = 0; k < KV; ++k) {
      const int col = k * G + l;
      if (col < D) a.z[r * D + col] = fmaf(t[k] * rstd, gm[k], bt[k]);
    }
    if (l == 0) a.mean[r] = (float)mean, a.rstd[r] = rstd;
  }
}

template <int G, int KV>
__global__ __launch_bounds__(THREADS) void postnorm_bwd_kernel(NormArgs a) {
  constexpr int RPW = 64 / G, RPB = RPW * WAVES, SLOTS = RPB;
  __shared__ float red[SLOTS][G * KV * 2 + 1];
  const int lane = threadIdx.x & 63, l = lane % G, slot = (threadIdx.x >> 6) * RPW + lane / G;
  const int D = a.D;
  p2c_rec::drop_begin(a.drop, true);
  p2c_rec::drop_keys(a.drop, true);
  float gm[KV], dg[KV], db[KV];
#pragma unroll
  for (int k = 0; k < KV; ++k) {
    const int col = k * G + l;
    gm[k] = col < D ? a.gamma[col] : 0.f;
    dg[k] = db[k] = 0.f;
  }
  const float inv_d = 1.f / (float)D;
  const double inv_d64 = 1.0 / (double)D;
  for (int64_t r0 = (int64_t)blockIdx.x * RPB; r0 < a.rows; r0 += (int64_t)gridDim.x * RPB) {
    const int64_t r = r0 + slot;
    const bool live = r < a.rows;
    const float rstd = live ? a.rstd[r] : 0.f;
    float xh[KV], gg[KV], keep[KV], s1 = 0.f, s2 = 0.f;
    double u[KV], s0 = 0.0;
#pragma unroll
    for (int k = 0; k < KV; ++k) {
      const int col = k * G + l;
      const bool ok = live && col < D;
      keep[k] = ok ? keep_of(a.drop, r, D, col) : 0.f;
      u[k] = ok ? fma((double)a.s[r * D + col], (double)keep[k], (double)a.x[r * D + col]) : 0.0;
      s0 += u[k];
    }
    const double mean = xor_sum<G>(s0) * inv_d64;       // (the forward's operations: the same bits)
#pragma unroll
    for (int k = 0; k < KV; ++k) {
      const int col = k * G + l;
      const bool ok = live && col < D;
      const float g = ok ? a.gz[r * D + col] : 0.f;
      xh[k] = ok ? (float)(u[k] - mean) * rstd : 0.f;
      gg[k] = g * gm[k];
      s1 += gg[k];
      s2 = fmaf(gg[k], xh[k], s2);
      dg[k] = fmaf(g, xh[k], dg[k]);
      db[k] += g;
    }
    const float m1 = xor_sum<G>(s1) * inv_d, m2 = xor_sum<G>(s2) * inv_d;
    if (!live) continue;
#pragma unroll
    for (int k = 0; k < KV; ++k) {
      const int col = k * G + l;
      if (col < D) {
        const float o = rstd * (gg[k] - m1 - xh[k] * m2);
        a.gx[r * D + col] = o;
        a.gs[r * D + col] = o * keep[k];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < KV; ++k) {
    red[slot][(k * G + l) * 2] = dg[k];
    red[slot][(k * G + l) * 2 + 1] = db[k];
  }
  __syncthreads();
  float *out = a.partials + (size_t)blockIdx.x * 2 * D;
  for (int i = threadIdx.x; i < 2 * D; i += THREADS) {
    const int which = i / D, col = i - which * D;
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < SLOTS; ++q) s += red[q][col * 2 + which];
    out[i] = s;
  }
}

static int norm_shape_ok(int64_t rows, int32_t D) { return rows >= 0 && D >= 2 && D <= 1024; }

#define P2C_PN_DISPATCH(KERNEL, grid)                                                                           \
  if (D <= 32) hipLaunchKernelGGL((KERNEL<8, 4>), grid, dim3(THREADS), 0, (hipStream_t)stream, a);              \
  else if (D <= 64) hipLaunchKernelGGL((KERNEL<16, 4>), grid, dim3(THREADS), 0, (hipStream_t)stream, a);        \
  else if (D <= 128) hipLaunchKernelGGL((KERNEL<32, 4>), grid, dim3(THREADS), 0, (hipStream_t)stream, a);       \
  else if (D <= 256) hipLaunchKernelGGL((KERNEL<64, 4>), grid, dim3(THREADS), 0, (hipStream_t)stream, a);       \
  else if (D <= 512) hipLaunchKernelGGL((KERNEL<64, 8>), grid, dim3(THREADS), 0, (hipStream_t)stream, a);       \
  else hipLaunchKernelGGL((KERNEL<64, 16>), grid, dim3(THREADS), 0, (hipStream_t)stream, a);

}  // namespace p2c_encoder

using namespace p2c_encoder;

extern "C" int p2c_attn_drop_supported(int32_t N, int32_t heads, int32_t head_dim) {
  return N >= 1 && N <= MAXN && heads >= 1 && head_dim >= 1 && (int64_t)heads * head_dim <= 256;
}

static int attn_check(const float *qkv, int32_t S, int32_t N, int32_t heads, int32_t head_dim, void *drop_state, float drop_p) {
  if (!p2c_attn_drop_supported(N, heads, head_dim) || S < 0) return P2C_E_SHAPE;
  if (!(drop_p >= 0.f && drop_p < 1.f)) return P2C_E_SHAPE;
  if ((int64_t)S * heads > 0x7fffffffll) return P2C_E_SHAPE;
  if (drop_state && drop_p > 0.f && (int64_t)S * heads * N * N >= (1ll << 31)) return P2C_E_SHAPE;
  return 0;
}

extern "C" int p2c_attn_drop_fwd(const float *qkv, float *out, float scale, int32_t S, int32_t N, int32_t heads, int32_t head_dim,
                                 void *drop_state, float drop_p, int32_t drop_site, void *stream) {
  if (!qkv || !out) return P2C_E_NULL;
  if (int rc = attn_check(qkv, S, N, heads, head_dim, drop_state, drop_p)) return rc;
  if (S == 0) return 0;
  AttnArgs a{};
  a.qkv = qkv, a.out = out, a.S = S, a.N = N, a.heads = heads, a.hd = head_dim, a.scale = scale;
  a.drop = DropRng(drop_p > 0.f ? drop_state : nullptr, drop_p, drop_site);
  hipLaunchKernelGGL(attn_fwd_kernel, dim3((unsigned)(S * heads)), dim3(THREADS), 0, (hipStream_t)stream, a);
  return p2c_host::launch_status();
}

extern "C" int p2c_attn_drop_bwd(const float *qkv, const float *g_out, float *g_qkv, float scale, int32_t S, int32_t N,
                                 int32_t heads, int32_t head_dim, void *drop_state, float drop_p, int32_t drop_site, void *stream) {
  if (!qkv || !g_out || !g_qkv) return P2C_E_NULL;
  if (int rc = attn_check(qkv, S, N, heads, head_dim, drop_state, drop_p)) return rc;
  if (S == 0) return 0;
  AttnArgs a{};
  a.qkv = qkv, a.g_out = g_out, a.g_qkv = g_qkv, a.S = S, a.N = N, a.heads = heads, a.hd = head_dim, a.scale = scale;
  a.drop = DropRng(drop_p > 0.f ? drop_state : nullptr, drop_p, drop_site);
  hipLaunchKernelGGL(attn_bwd_kernel, dim3((unsigned)(S * heads)), dim3(THREADS), 0, (hipStream_t)stream, a);
  return p2c_host::launch_status();
}

extern "C" int p2c_postnorm_supported(int32_t D) { return norm_shape_ok(0, D); }

extern "C" int64_t p2c_postnorm_workspace_floats(int64_t rows, int32_t D) {
  if (!norm_shape_ok(rows, D)) return 0;
  return (int64_t)p2c_internal_norm_blocks(rows, D) * 2 * D;
}

static int norm_check(int64_t rows, int32_t D, void *drop_state, float drop_p) {
  if (!norm_shape_ok(rows, D)) return P2C_E_SHAPE;
  if (!(drop_p >= 0.f && drop_p < 1.f)) return P2C_E_SHAPE;
  if (drop_state && drop_p > 0.f && rows * D >= (1ll << 31)) return P2C_E_SHAPE;
  return 0;
}

extern "C" int p2c_postnorm_fwd(const float *x, const float *s, const float *gamma, const float *beta, float *z, float *mean,
                                float *rstd, int64_t rows, int32_t D, float eps, void *drop_state, float drop_p, int32_t drop_site,
                                void *stream) {
  if (!x || !s || !gamma || !beta || !z || !mean || !rstd) return P2C_E_NULL;
  if (int rc = norm_check(rows, D, drop_state, drop_p)) return rc;
  if (rows == 0) return 0;
  NormArgs a{};
  a.x = x, a.s = s, a.gamma = gamma, a.beta = beta, a.z = z, a.mean = mean, a.rstd = rstd, a.rows = rows, a.D = D, a.eps = eps;
  a.drop = DropRng(drop_p > 0.f ? drop_state : nullptr, drop_p, drop_site);
  const dim3 grid((unsigned)p2c_internal_norm_blocks(rows, D));
  P2C_PN_DISPATCH(postnorm_fwd_kernel, grid)
  return p2c_host::launch_status();
}

extern "C" int p2c_postnorm_bwd(const float *x, const float *s, const float *gamma, const float *mean, const float *rstd,
                                const float *g_z, float *g_x, float *g_s, float *g_gamma, float *g_beta, int32_t accumulate,
                                float *workspace, int64_t rows, int32_t D, void *drop_state, float drop_p, int32_t drop_site,
                                void *stream) {
  if (!x || !s || !gamma || !mean || !rstd || !g_z || !g_x || !g_s || !g_gamma || !g_beta || !workspace) return P2C_E_NULL;
  if (int rc = norm_check(rows, D, drop_state, drop_p)) return rc;
  NormArgs a{};
  a.x = x, a.s = s, a.gamma = gamma, a.mean = const_cast<float *>(mean), a.rstd = const_cast<float *>(rstd), a.gz = g_z;
  a.gx = g_x, a.gs = g_s, a.g_gamma = g_gamma, a.g_beta = g_beta, a.partials = workspace, a.rows = rows, a.D = D;
  a.accumulate = accumulate;
  a.drop = DropRng(drop_p > 0.f ? drop_state : nullptr, drop_p, drop_site);
  a.n_blocks = rows > 0 ? p2c_internal_norm_blocks(rows, D) : 0;
  if (rows > 0) {
    const dim3 grid((unsigned)a.n_blocks);
    P2C_PN_DISPATCH(postnorm_bwd_kernel, grid)
  }
  return p2c_internal_norm_finish(workspace, a.n_blocks, D, g_gamma, g_beta, accumulate, (hipStream_t)stream);   // K15's second launch
}
