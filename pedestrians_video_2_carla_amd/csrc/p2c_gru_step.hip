// p2c_gru_step.hip -- K23: the recurrent half of a GRU layer for any hidden size (1 <= H <= 1024), one launch per time step
// (gfx950, fp32 MFMA). The launch-per-step seam is K18's (p2c_lstm_step.hip); the tile (its constants, the staging and both MFMA
// loops) is p2c_rec_step_dev.h's, shared with K18.
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
// Addresses are 64-bit; rows past B / H are range-checked (loads are clamped, stores are skipped).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/p2c.h"
#include "p2c_host.h"
#include "p2c_rec_step_dev.h"

namespace p2c_gru_step {

using namespace p2c_rec_step;

struct Args {
  const float *gx, *h0, *w_hh, *bias_hh;
  float *out, *hT, *acts;
  const float *g_out, *g_hT;
  float *g_gx, *g_gh, *g_h0, *dh;
  int32_t T, B, H;
};

// ---- forward ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void gru_step_fwd_kernel(const Args a, const int t) {
  __shared__ float wl[3 * 16 * KP], hl[BM * KP];             // gates_product's
  const int H = a.H, B = a.B, T = a.T;
  const int64_t G = 3 * (int64_t)H;
  const Lane l(B);
  const int b = l.b, u0 = l.u0, bc = l.bc;                    // this lane: sequence b, units u0 .. u0 + 3
  const bool bok = l.bok;

  const float *hp = t > 0 ? a.out + ((int64_t)(t - 1) * B) * H : a.h0;   // NULL at t = 0 with the zero state: no product
  // per-lane rows: unconditional loads from clamped addresses (one round trip for all of them)
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

  if (hp) gates_product<3>(acc, wl, hl, a.w_hh, hp, H, B, l);

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
  __shared__ float wl[16 * KP], gl[BM * KP];                  // state_grad_product's
  const int H = a.H, B = a.B, T = a.T;
  const int64_t G = 3 * (int64_t)H;
  const Lane l(B);
  const int b = l.b, u0 = l.u0, bc = l.bc;
  const bool bok = l.bok;

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

  // g_gh[t+1] W_hh[:, units]
  const f32x4 dhr = state_grad_product(wl, gl, a.w_hh, t + 1 < T ? a.g_gh + ((int64_t)(t + 1) * B) * G : nullptr, G, H, B, l);
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
  if (int rc = check_tbh(d->T, d->B, d->H)) return rc;
  // fields this form does not implement are refused, not ignored
  if (d->gx_bt || d->out_drop || d->drop_state) return P2C_E_SHAPE;
  a = Args{};
  a.gx = d->gx, a.h0 = d->h0, a.w_hh = d->w_hh, a.bias_hh = d->bias_hh;
  a.out = d->out, a.hT = d->hT, a.acts = d->acts;
  a.g_out = d->g_out, a.g_hT = d->g_hT, a.g_gx = d->g_gx, a.g_gh = d->g_gh, a.g_h0 = d->g_h0;
  a.T = d->T, a.B = d->B, a.H = d->H;
  return 0;
}

extern "C" int64_t p2c_gru_steps_workspace_floats(int32_t B, int32_t H) { return workspace_floats(B, H); }

extern "C" int p2c_gru_steps_fwd(const p2c_gru_desc *d, void *stream) {
  Args a;
  int rc = check_steps(d, a);
  if (rc) return rc;
  if (!a.gx || !a.out) return P2C_E_NULL;                        // out carries the state from one launch to the next
  if (a.B == 0) return 0;
  for (int t = 0; t < a.T; ++t) hipLaunchKernelGGL(gru_step_fwd_kernel, steps_grid(a.B, a.H), dim3(NT), 0, (hipStream_t)stream, a, t);
  return p2c_host::launch_status();
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
  for (int t = a.T - 1; t >= 0; --t) hipLaunchKernelGGL(gru_step_bwd_kernel, steps_grid(a.B, a.H), dim3(NT), 0, (hipStream_t)stream, a, t);
  if (a.g_h0) hipLaunchKernelGGL(gru_step_bwd_kernel, steps_grid(a.B, a.H), dim3(NT), 0, (hipStream_t)stream, a, -1);
  return p2c_host::launch_status();
}
