// p2c_gru_step.hip -- K23: the recurrent half of a GRU layer for any hidden size (1 <= H <= 1024), one launch per time step
// (gfx950, fp32 MFMA). The tiling, the staging and the launch-per-step seam are K18's (p2c_lstm_step.hip).
//
// torch.nn.GRU, gate order r, z, n, with gx[t] = x[t] W_ih^T + b_ih from the caller (one dense GEMM for all t):
//   r = sigmoid(gx_r + W_hr h + b_hr)     z = sigmoid(gx_z + W_hz h + b_hz)     n = tanh(gx_n + r (W_hn h + b_hn))
//   h' = (1 - z) n + z h
// b_hn sits INSIDE the reset gate's product, so bias_hh cannot be folded into the input projection's bias (the kernel takes it)
// and the gradient of the recurrent pre-activation gh = W_hh h + b_hh differs from the gradient of gx in the n block by the
// factor r: the backward writes both, g_gx (-> dW_ih, db_ih, dx) and g_gh (-> dW_hh, db_hh and the dh of the step before).
//
// Forward, step t: a workgroup owns BM sequences x 16 hidden units with the three gates of those units: wave w takes sequences
// [16w, 16w + 16) of the tile, the 3 x 16 rows {qH + u} of W_hh and the tile's h[t-1] rows are staged through LDS in K-chunks of
// KC (zero-padded past H), three v_mfma_f32_16x16x4f32 accumulators leave lane (c, g) holding the r, z and n recurrent terms of
// (sequence c, units 4g .. 4g + 3), and the state update happens in registers. h[t-1] is out[t-1] (or h0; a NULL h0 is the
// zero state: no product at t = 0). It saves acts (T,B,4H) = r, z, n and hn = W_hn h + b_hn.
// Backward, step t (descending): dh = g_out[t] (+ g_hT at T - 1) + z[t+1] dh[t+1] (carried through a (B, H) workspace that only
// the owning lane touches) + g_gh[t+1] W_hh[:, units] (K = 3H, staged the same way); it writes g_gx[t], g_gh[t] and the carry.
// One more launch forms g_h0 = carry + g_gh[0] W_hh. The weight gradients are the caller's (K12 over all (t, b)).
// Addresses are 64-bit; rows past B / H are range-checked (loads are clamped, stores are skipped). The staging loads of a chunk
// are all issued first, unconditionally, from clamped (always valid) addresses; the zero padding is a select on the LDS write.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/p2c.h"
#include "p2c_rec_dev.h"

namespace p2c_gru_step {

using namespace p2c_rec;
constexpr int BM = 32;            // sequences per workgroup (16 per wave)
constexpr int NT = 64 * BM / 16;  // threads per workgroup
constexpr int KC = 64;            // K chunk staged in LDS
constexpr int KP = KC + 4;        // LDS pitch: the 16 rows x 4 k of a fragment read fall in distinct banks (two passes)

// a value loaded from global memory made resident here: the load cannot be sunk under the select that follows
__device__ __forceinline__ void pin1(float &v) { asm volatile("" : "+v"(v)); }

struct Args {
  const float *gx, *h0, *w_hh, *bias_hh;
  float *out, *hT, *acts;
  const float *g_out, *g_hT;
  float *g_gx, *g_gh, *g_h0, *dh;
  int32_t T, B, H;
};

// ---- forward ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void gru_step_fwd_kernel(const Args a, const int t) {
  __shared__ float wl[48 * KP];   // rows q * 16 + i: W_hh row q H + ub + i, columns k0 .. k0 + KC
  __shared__ float hl[BM * KP];   // rows s: h[t-1] of sequence b0 + s
  const int H = a.H, B = a.B, T = a.T;
  const int64_t G = 3 * (int64_t)H;
  const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4, w = threadIdx.x >> 6;
  const int b0 = blockIdx.x * BM, ub = blockIdx.y * 16;
  const int b = b0 + w * 16 + c, u0 = ub + 4 * g;         // this lane: sequence b, units u0 .. u0 + 3
  const bool bok = b < B;

  const float *hp = t > 0 ? a.out + ((int64_t)(t - 1) * B) * H : a.h0;   // NULL at t = 0 with the zero state: no product
  // per-lane rows: unconditional loads from clamped addresses (one round trip for all of them)
  const int bc = min(b, B - 1);
  f32x4 acc[3], xn, hprev;        // acc[0], acc[1]: the r and z pre-activations; acc[2]: hn = W_hn h + b_hn; xn: gx_n
  {
    const float *gxr = a.gx + ((int64_t)t * B + bc) * G;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int uc = min(u0 + r, H - 1);
      acc[0][r] = gxr[uc], acc[1][r] = gxr[H + uc], xn[r] = gxr[2 * H + uc];
      acc[2][r] = 0.f;
      hprev[r] = hp ? hp[(int64_t)bc * H + uc] : 0.f;
    }
    if (a.bias_hh) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int uc = min(u0 + r, H - 1);
#pragma unroll
        for (int q = 0; q < 3; ++q) acc[q][r] += a.bias_hh[q * H + uc];
      }
    }
  }

  if (hp) {
    for (int k0 = 0; k0 < H; k0 += KC) {
      constexpr int NW_ = 48 * KC / NT, NH_ = BM * KC / NT;
      float vw[NW_], vh[NH_];
#pragma unroll
      for (int j = 0; j < NW_; ++j) {
        const int e = threadIdx.x + j * NT, row = e / KC, k = e % KC, u = ub + (row & 15), kk = k0 + k;
        vw[j] = a.w_hh[((int64_t)(row >> 4) * H + min(u, H - 1)) * H + min(kk, H - 1)];
      }
#pragma unroll
      for (int j = 0; j < NH_; ++j) {
        const int e = threadIdx.x + j * NT, s = e / KC, k = e % KC, kk = k0 + k;
        vh[j] = hp[(int64_t)min(b0 + s, B - 1) * H + min(kk, H - 1)];
      }
#pragma unroll
      for (int j = 0; j < NW_; ++j) {
        pin1(vw[j]);
        const int e = threadIdx.x + j * NT, row = e / KC, k = e % KC, u = ub + (row & 15), kk = k0 + k;
        wl[row * KP + k] = (u < H && kk < H) ? vw[j] : 0.f;
      }
#pragma unroll
      for (int j = 0; j < NH_; ++j) {
        pin1(vh[j]);
        const int e = threadIdx.x + j * NT, s = e / KC, k = e % KC, kk = k0 + k;
        hl[s * KP + k] = (b0 + s < B && kk < H) ? vh[j] : 0.f;
      }
      __syncthreads();
      const int nks = (min(KC, H - k0) + 3) / 4;            // k-steps that touch a real column (the rest of the chunk is 0)
      const float *wa = wl + c * KP + g, *hb = hl + (w * 16 + c) * KP + g;
      for (int ks = 0; ks < nks; ++ks) {
        const float bv = hb[4 * ks];
#pragma unroll
        for (int q = 0; q < 3; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[q * 16 * KP + 4 * ks], bv, acc[q], 0, 0, 0);
      }
      __syncthreads();                                      // the chunk has been read before the next one is staged
    }
  }

  if (!bok) return;
  const int64_t row1 = ((int64_t)t * B + b) * H, row4 = ((int64_t)t * B + b) * 4 * (int64_t)H;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int u = u0 + r;
    if (u >= H) continue;
    const float ar = sigmoidf_(acc[0][r]), az = sigmoidf_(acc[1][r]), hn = acc[2][r];
    const float an = tanhf_(xn[r] + ar * hn);
    const float h = an + az * (hprev[r] - an);
    a.out[row1 + u] = h;
    if (a.acts) a.acts[row4 + u] = ar, a.acts[row4 + H + u] = az, a.acts[row4 + 2 * H + u] = an, a.acts[row4 + 3 * H + u] = hn;
    if (t == T - 1 && a.hT) a.hT[(int64_t)b * H + u] = h;
  }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------
// t >= 0: step t of the backward; t = -1: g_h0 = carry + g_gh[0] W_hh only.
__global__ __launch_bounds__(NT) void gru_step_bwd_kernel(const Args a, const int t) {
  __shared__ float wl[16 * KP];   // rows i: W_hh[k0 + k][ub + i] (the transposed column block of the tile's units)
  __shared__ float gl[BM * KP];   // rows s: g_gh[t+1] of sequence b0 + s
  const int H = a.H, B = a.B, T = a.T;
  const int64_t G = 3 * (int64_t)H;
  const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4, w = threadIdx.x >> 6;
  const int b0 = blockIdx.x * BM, ub = blockIdx.y * 16;
  const int b = b0 + w * 16 + c, u0 = ub + 4 * g;
  const bool bok = b < B;
  const int bc = min(b, B - 1);

  // the saved rows of the step: requested before the product, used after it (lanes past B / H compute values that are never stored)
  f32x4 ar, az, an, hn, hprev, go;
#pragma unroll
  for (int r = 0; r < 4; ++r) ar[r] = az[r] = an[r] = hn[r] = hprev[r] = go[r] = 0.f;
  if (t + 1 < T) {                                           // the carry z[t+1] dh[t+1], left by the launch of step t + 1
#pragma unroll
    for (int r = 0; r < 4; ++r) go[r] = a.dh[(int64_t)bc * H + min(u0 + r, H - 1)];
  }
  if (t >= 0) {
    const int64_t row1 = ((int64_t)t * B + bc) * H, row4 = ((int64_t)t * B + bc) * 4 * (int64_t)H;
    const float *hp = t > 0 ? a.out + ((int64_t)(t - 1) * B) * H : a.h0;
    const float *ghT = t == T - 1 ? a.g_hT : nullptr;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int uc = min(u0 + r, H - 1);
      ar[r] = a.acts[row4 + uc], az[r] = a.acts[row4 + H + uc], an[r] = a.acts[row4 + 2 * H + uc], hn[r] = a.acts[row4 + 3 * H + uc];
      hprev[r] = hp ? hp[(int64_t)bc * H + uc] : 0.f;
      if (a.g_out) go[r] += a.g_out[row1 + uc];
      if (ghT) go[r] += ghT[(int64_t)bc * H + uc];
    }
  }

  // g_gh[t+1] W_hh[:, units]: four accumulators over the k-steps break the dependent MFMA chain
  f32x4 e[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) e[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  if (t + 1 < T) {
    const float *gn = a.g_gh + ((int64_t)(t + 1) * B) * G;
    for (int64_t k0 = 0; k0 < G; k0 += KC) {
      constexpr int NW_ = 16 * KC / NT, NG_ = BM * KC / NT;
      float vw[NW_], vg[NG_];
#pragma unroll
      for (int j = 0; j < NW_; ++j) {
        const int x = threadIdx.x + j * NT, k = x / 16, i = x % 16;
        vw[j] = a.w_hh[min(k0 + k, G - 1) * H + min(ub + i, H - 1)];
      }
#pragma unroll
      for (int j = 0; j < NG_; ++j) {
        const int x = threadIdx.x + j * NT, s = x / KC, k = x % KC;
        vg[j] = gn[(int64_t)min(b0 + s, B - 1) * G + min(k0 + k, G - 1)];
      }
#pragma unroll
      for (int j = 0; j < NW_; ++j) {
        pin1(vw[j]);
        const int x = threadIdx.x + j * NT, k = x / 16, i = x % 16;
        wl[i * KP + k] = (ub + i < H && k0 + k < G) ? vw[j] : 0.f;
      }
#pragma unroll
      for (int j = 0; j < NG_; ++j) {
        pin1(vg[j]);
        const int x = threadIdx.x + j * NT, s = x / KC, k = x % KC;
        gl[s * KP + k] = (b0 + s < B && k0 + k < G) ? vg[j] : 0.f;
      }
      __syncthreads();
      const int n16 = (int)((min((int64_t)KC, G - k0) + 15) / 16);   // groups of four k-steps that touch a real row of W_hh
      const float *wa = wl + c * KP + g, *gb = gl + (w * 16 + c) * KP + g;
      for (int j = 0; j < n16; ++j) {
#pragma unroll
        for (int q = 0; q < 4; ++q) e[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[16 * j + 4 * q], gb[16 * j + 4 * q], e[q], 0, 0, 0);
      }
      __syncthreads();
    }
  }
  const f32x4 dhr = (e[0] + e[1]) + (e[2] + e[3]);
  if (!bok) return;

  if (t < 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (u0 + r < H) a.g_h0[(int64_t)b * H + u0 + r] = go[r] + dhr[r];
    return;
  }
  const int64_t row3 = ((int64_t)t * B + b) * G;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int u = u0 + r;
    if (u >= H) continue;
    const float dht = go[r] + dhr[r];
    const float dnp = dht * (1.f - az[r]) * (1.f - an[r] * an[r]);        // d (gx_n + r hn)
    const float pz = dht * (hprev[r] - an[r]) * az[r] * (1.f - az[r]);
    const float pr = dnp * hn[r] * ar[r] * (1.f - ar[r]);
    a.g_gx[row3 + u] = pr, a.g_gx[row3 + H + u] = pz, a.g_gx[row3 + 2 * H + u] = dnp;
    a.g_gh[row3 + u] = pr, a.g_gh[row3 + H + u] = pz, a.g_gh[row3 + 2 * H + u] = dnp * ar[r];
    if (t > 0 || a.g_h0) a.dh[(int64_t)b * H + u] = dht * az[r];
  }
}

}  // namespace p2c_gru_step

using namespace p2c_gru_step;

static int check_steps(const p2c_gru_desc *d, Args &a) {
  if (!d || !d->w_hh) return P2C_E_NULL;
  if (d->T < 0 || d->B < 0 || d->B > (1 << 20) || d->H < 1 || d->H > 1024) return P2C_E_SHAPE;
  // fields this form does not implement are refused, not ignored
  if (d->gx_bt || d->out_drop || d->drop_state) return P2C_E_SHAPE;
  a = Args{};
  a.gx = d->gx, a.h0 = d->h0, a.w_hh = d->w_hh, a.bias_hh = d->bias_hh;
  a.out = d->out, a.hT = d->hT, a.acts = d->acts;
  a.g_out = d->g_out, a.g_hT = d->g_hT, a.g_gx = d->g_gx, a.g_gh = d->g_gh, a.g_h0 = d->g_h0;
  a.T = d->T, a.B = d->B, a.H = d->H;
  return 0;
}

static dim3 steps_grid(const Args &a) { return dim3((unsigned)((a.B + BM - 1) / BM), (unsigned)((a.H + 15) / 16)); }

extern "C" int64_t p2c_gru_steps_workspace_floats(int32_t B, int32_t H) {
  return (B < 0 || H < 0) ? 0 : (int64_t)B * H;
}

extern "C" int p2c_gru_steps_fwd(const p2c_gru_desc *d, void *stream) {
  Args a;
  int rc = check_steps(d, a);
  if (rc) return rc;
  if (!a.gx || !a.out) return P2C_E_NULL;                        // out carries the state from one launch to the next
  if (a.B == 0) return 0;
  for (int t = 0; t < a.T; ++t) hipLaunchKernelGGL(gru_step_fwd_kernel, steps_grid(a), dim3(NT), 0, (hipStream_t)stream, a, t);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

extern "C" int p2c_gru_steps_bwd(const p2c_gru_desc *d, float *workspace, void *stream) {
  Args a;
  int rc = check_steps(d, a);
  if (rc) return rc;
  if (!a.acts || !a.g_gx || !a.g_gh) return P2C_E_NULL;
  if (a.T > 1 && !a.out) return P2C_E_NULL;                      // h[t-1] of the steps after the first
  if ((a.T > 1 || a.g_h0) && !workspace) return P2C_E_NULL;
  a.dh = workspace;
  if (a.B == 0 || a.T == 0) return 0;
  for (int t = a.T - 1; t >= 0; --t) hipLaunchKernelGGL(gru_step_bwd_kernel, steps_grid(a), dim3(NT), 0, (hipStream_t)stream, a, t);
  if (a.g_h0) hipLaunchKernelGGL(gru_step_bwd_kernel, steps_grid(a), dim3(NT), 0, (hipStream_t)stream, a, -1);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}
