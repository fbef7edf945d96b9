// p2c_lstm_step.hip -- K18: the recurrent half of an LSTM layer for ANY hidden size (1 <= H <= 1024), one launch per time step
// (gfx950, fp32 MFMA).
//
// K7b (p2c_lstm.hip) keeps W_hh in registers for the whole sequence: H / 16 waves of H VGPRs each, which stops at H = 128
// (from H = 256 on the whole W_hh, 4H x H fp32, is larger than a CU's register file and LDS together). The reference's LSTM
// movements model draws H from 64 ... 512 as any integer. Here the time loop is cut at its all-to-all seam instead: h[t] of every
// unit feeds every gate of step t + 1, so each step is one launch and the launch boundary is the synchronisation between steps
// (no waits between workgroups, no grid barrier).
//
// Forward, step t: gates = gx[t] (+ bias_a + bias_b) + h[t-1] W_hh^T, then c[t] = f c[t-1] + i g, h[t] = o tanh(c[t]) (gate order
// i, f, g, o). A workgroup owns BM sequences x 16 hidden units with all four gates of those units: wave w takes sequences
// [16w, 16w + 16) of the tile, the 4 x 16 rows {qH + u} of W_hh and the tile's h[t-1] rows are staged through LDS in K-chunks of
// KC (zero-padded past H), and four v_mfma_f32_16x16x4f32 accumulators -- one per gate, started from gx[t] -- leave lane (c, g)
// holding i, f, g, o of (sequence c, units 4g .. 4g + 3): the cell update happens in registers, as in K7b. h[t-1] is out[t-1]
// (or h0), c[t-1] is cs[t-1] (or c0): the saved tensors carry the state from one launch to the next. The tile (its constants, the
// staging and both MFMA loops) is p2c_rec_step_dev.h's, shared with the GRU (K23).
// Backward, step t (descending): dh = g_out[t] (+ g_hT at T - 1) + dgates[t+1] W_hh[:, units] (K = 4H, staged the same way), then
// the cell backward with the carried dc, read and written through a (B, H) workspace that only the owning lane touches; it writes
// g_gx[t] (= d gates) and dc for step t - 1 (g_c0 at t = 0). One more launch forms g_h0 = dgates[0] W_hh. The weight gradients
// are the caller's (dW_hh = sum_t dgates[t]^T h[t-1], one K12 launch over all (t, b)).
// Addresses are 64-bit; rows past B / H are range-checked (loads are clamped, stores are skipped).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/p2c.h"
#include "p2c_host.h"
#include "p2c_rec_step_dev.h"

namespace p2c_lstm_step {

using namespace p2c_rec_step;

struct Args {
  const float *gx, *h0, *c0, *w_hh, *bias_a, *bias_b;
  float *out, *hT, *cT, *acts, *cs;
  const float *g_out, *g_hT, *g_cT;
  float *g_gx, *g_h0, *g_c0, *dc;
  int32_t T, B, H;
};

// ---- forward ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void lstm_step_fwd_kernel(const Args a, const int t) {
  __shared__ float wl[4 * 16 * KP], hl[BM * KP];             // gates_product's
  const int H = a.H, B = a.B, T = a.T;
  const int64_t G = 4 * (int64_t)H;
  const Lane l(B);
  const int b = l.b, u0 = l.u0, bc = l.bc;                    // this lane: sequence b, units u0 .. u0 + 3
  const bool bok = l.bok;

  const float *cprev = t > 0 ? a.cs + ((int64_t)(t - 1) * B) * H : a.c0;
  // per-lane rows: unconditional loads from clamped addresses (one round trip for all of them), then selects
  f32x4 acc[4], cp;
  {
    const float *gxr = a.gx + ((int64_t)t * B + bc) * G;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int uc = min(u0 + r, H - 1);
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q][r] = gxr[q * H + uc];
      cp[r] = cprev ? cprev[(int64_t)bc * H + uc] : 0.f;
    }
    if (a.bias_a || a.bias_b) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int uc = min(u0 + r, H - 1);
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q][r] += (a.bias_a ? a.bias_a[q * H + uc] : 0.f) + (a.bias_b ? a.bias_b[q * H + uc] : 0.f);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool ok = bok && u0 + r < H;           // (padding lanes: zero pre-activations, as the zero-padded operands give)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q][r] = ok ? acc[q][r] : 0.f;
    }
  }

  const float *hp = t > 0 ? a.out + ((int64_t)(t - 1) * B) * H : a.h0;   // NULL at t = 0 with the zero state: no product
  if (hp) gates_product<4>(acc, wl, hl, a.w_hh, hp, H, B, l);

  if (!bok) return;
  const int64_t row1 = ((int64_t)t * B + b) * H, row4 = ((int64_t)t * B + b) * G;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int u = u0 + r;
    if (u >= H) continue;
    const float ai = sigmoidf_(acc[0][r]), af = sigmoidf_(acc[1][r]), ag = tanhf_(acc[2][r]), ao = sigmoidf_(acc[3][r]);
    const float ig = ai * ag;
    const float cn = af * cp[r] + ig;
    const float h = ao * tanhf_(cn);
    a.out[row1 + u] = h;
    a.cs[row1 + u] = cn;
    a.acts[row4 + u] = ai, a.acts[row4 + H + u] = af, a.acts[row4 + 2 * H + u] = ag, a.acts[row4 + 3 * H + u] = ao;
    if (t == T - 1) {
      if (a.hT) a.hT[(int64_t)b * H + u] = h;
      if (a.cT) a.cT[(int64_t)b * H + u] = cn;
    }
  }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------
// t >= 0: step t of the backward; t = -1: g_h0 = dgates[0] W_hh only.
__global__ __launch_bounds__(NT) void lstm_step_bwd_kernel(const Args a, const int t) {
  __shared__ float wl[16 * KP], gl[BM * KP];                  // state_grad_product's
  const int H = a.H, B = a.B, T = a.T;
  const int64_t G = 4 * (int64_t)H;
  const Lane l(B);
  const int b = l.b, u0 = l.u0, bc = l.bc;
  const bool bok = l.bok;

  // the saved rows of the step: requested before the product, used after it
  f32x4 ai, af, ag, ao, ct, cp, go, dc;
  if (t >= 0) {   // unconditional loads from clamped addresses (lanes past B / H compute values that are never stored)
    const int64_t row1 = ((int64_t)t * B + bc) * H, row4 = ((int64_t)t * B + bc) * G;
    const float *cprev = t > 0 ? a.cs + ((int64_t)(t - 1) * B) * H : a.c0;
    const float *dcin = t == T - 1 ? a.g_cT : a.dc;          // the carry: g_cT at the last step, then what step t + 1 left
    const float *ghT = t == T - 1 ? a.g_hT : nullptr;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int uc = min(u0 + r, H - 1);
      ai[r] = a.acts[row4 + uc], af[r] = a.acts[row4 + H + uc], ag[r] = a.acts[row4 + 2 * H + uc], ao[r] = a.acts[row4 + 3 * H + uc];
      ct[r] = a.cs[row1 + uc];
      cp[r] = cprev ? cprev[(int64_t)bc * H + uc] : 0.f;
      go[r] = a.g_out ? a.g_out[row1 + uc] : 0.f;
      dc[r] = dcin ? dcin[(int64_t)bc * H + uc] : 0.f;
    }
    if (ghT) {
#pragma unroll
      for (int r = 0; r < 4; ++r) go[r] += ghT[(int64_t)bc * H + min(u0 + r, H - 1)];
    }
  }

  // dh = dgates[t+1] W_hh[:, units]
  const f32x4 dhr = state_grad_product(wl, gl, a.w_hh, t + 1 < T ? a.g_gx + ((int64_t)(t + 1) * B) * G : nullptr, G, H, B, l);
  if (!bok) return;

  if (t < 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (u0 + r < H) a.g_h0[(int64_t)b * H + u0 + r] = dhr[r];
    return;
  }
  const int64_t row4 = ((int64_t)t * B + b) * G;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int u = u0 + r;
    if (u >= H) continue;
    const float dht = go[r] + dhr[r];
    const float tc = tanhf_(ct[r]);
    const float dct = dc[r] + dht * ao[r] * (1.f - tc * tc);
    const float po = dht * tc * ao[r] * (1.f - ao[r]);
    const float pi = dct * ag[r] * ai[r] * (1.f - ai[r]);
    const float pf = dct * cp[r] * af[r] * (1.f - af[r]);
    const float pg = dct * ai[r] * (1.f - ag[r] * ag[r]);
    a.g_gx[row4 + u] = pi, a.g_gx[row4 + H + u] = pf, a.g_gx[row4 + 2 * H + u] = pg, a.g_gx[row4 + 3 * H + u] = po;
    const float dcn = dct * af[r];
    if (t > 0) a.dc[(int64_t)b * H + u] = dcn;
    else if (a.g_c0) a.g_c0[(int64_t)b * H + u] = dcn;
  }
}

}  // namespace p2c_lstm_step

using namespace p2c_lstm_step;

static int check_steps(const p2c_lstm_desc *d, Args &a) {
  if (!d || !d->w_hh) return P2C_E_NULL;
  if (int rc = check_tbh(d->T, d->B, d->H)) return rc;
  // fields this form does not implement are refused, not ignored
  if (d->gx_bt || d->g_gx_bt || d->out_drop || d->drop_state) return P2C_E_SHAPE;
  a = Args{};
  a.gx = d->gx, a.h0 = d->h0, a.c0 = d->c0, a.w_hh = d->w_hh, a.bias_a = d->bias_a, a.bias_b = d->bias_b;
  a.out = d->out, a.hT = d->hT, a.cT = d->cT, a.acts = d->acts, a.cs = d->cs;
  a.g_out = d->g_out, a.g_hT = d->g_hT, a.g_cT = d->g_cT, a.g_gx = d->g_gx, a.g_h0 = d->g_h0, a.g_c0 = d->g_c0;
  a.T = d->T, a.B = d->B, a.H = d->H;
  return 0;
}

// T = 0 (p2c.h): no step runs, so the final state is the initial one and the gradient of the initial state is that of the final one --
// copied on the stream, or zero-filled where the source is NULL.
static int pass_state(float *dst, const float *src, const Args &a, hipStream_t stream) {
  if (!dst || dst == src) return 0;
  const size_t bytes = (size_t)a.B * a.H * sizeof(float);
  const hipError_t e = src ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, stream) : hipMemsetAsync(dst, 0, bytes, stream);
  return e == hipSuccess ? 0 : (int)e;
}

extern "C" int64_t p2c_lstm_steps_workspace_floats(int32_t B, int32_t H) { return workspace_floats(B, H); }

extern "C" int p2c_lstm_steps_fwd(const p2c_lstm_desc *d, void *stream) {
  Args a;
  int rc = check_steps(d, a);
  if (rc) return rc;
  if (!a.gx || !a.out || !a.acts || !a.cs) return P2C_E_NULL;   // cs carries the cell state from one launch to the next
  if (a.B == 0) return 0;
  if (a.T == 0) {
    if (int e = pass_state(a.hT, a.h0, a, (hipStream_t)stream)) return e;
    return pass_state(a.cT, a.c0, a, (hipStream_t)stream);
  }
  for (int t = 0; t < a.T; ++t) hipLaunchKernelGGL(lstm_step_fwd_kernel, steps_grid(a.B, a.H), dim3(NT), 0, (hipStream_t)stream, a, t);
  return p2c_host::launch_status();
}

extern "C" int p2c_lstm_steps_bwd(const p2c_lstm_desc *d, float *workspace, void *stream) {
  Args a;
  int rc = check_steps(d, a);
  if (rc) return rc;
  if (!a.acts || !a.cs || !a.g_gx) return P2C_E_NULL;
  if (a.T > 1 && !workspace) return P2C_E_NULL;
  a.dc = workspace;
  if (a.B == 0) return 0;
  if (a.T == 0) {
    if (int e = pass_state(a.g_h0, a.g_hT, a, (hipStream_t)stream)) return e;
    return pass_state(a.g_c0, a.g_cT, a, (hipStream_t)stream);
  }
  for (int t = a.T - 1; t >= 0; --t) hipLaunchKernelGGL(lstm_step_bwd_kernel, steps_grid(a.B, a.H), dim3(NT), 0, (hipStream_t)stream, a, t);
  if (a.g_h0) hipLaunchKernelGGL(lstm_step_bwd_kernel, steps_grid(a.B, a.H), dim3(NT), 0, (hipStream_t)stream, a, -1);
  return p2c_host::launch_status();
}
