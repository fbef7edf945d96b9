// p2c_pose_change_loss.hip -- K27: the pose_changes / cum_pose_changes training losses, one launch each way (gfx950).
//
// Reference: loss/pose_changes.py:7-28 (criterion(pose_inputs, targets['pose_changes'])) and loss/cum_pose_changes.py:9-56
// (prev = bmm(prev, change[t]) for prediction and target, T steps each, then the criterion on the stacked products), both with
// nn.MSELoss; for a model that emits 6-D rotations the reference's mixin has converted them first
// (modules/movements/movements.py:105-118), so the comparison -- and the divisor of the mean, B T J 9 -- is over matrices.
//
// Mapping. Every (clip, joint) pair is an independent chain of T 3x3 products; the B J chains are flattened densely over
// lanes (chain = b J + j), so a wavefront reads 64 neighbouring joints of a frame -- whole clips of 24 J or 36 J contiguous
// bytes. One lane walks its chain in frame order with the next frame's operands requested before the current frame's
// products (the T loop is a dependent chain: the loads are what can overlap). Workgroups are ONE wavefront: B = 256 has only
// 6 656 chains, 104 wavefronts that the dispatcher spreads over 104 CUs; no LDS, no barrier. The grid is capped at kMaxBlocks
// (desc.max_blocks lowers the cap); lanes stride over the chains beyond it.
// The direct form (cumulative = 0) is the same kernel on B chains-of-one: T' = 1, J' = T J.
//
// Forward: C_t = C_{t-1} M_t (C_0 = M_0: the reference's I M_0), likewise the target's running product, E_t = C_t - Gc_t,
//   loss = sum E^2 [/ N]. The lane adds its squares in (chain, t, element) order, the wavefront by xor-shuffles, and the
//   workgroup publishes one float. The LAST workgroup to arrive (an integer ticket; nobody waits) adds the published floats
//   in workgroup order in fp64 and writes the loss: fixed order, no float atomics, two runs give the same bits. Hand-off as in
//   the train step's weight gradient (p2c_train.hip): write-through store, drained by the storing wave, agent-scope integer
//   add by one lane, the last adder reads past its L1. The ticket word is zeroed by a 16-byte memset node in front of the launch.
// Backward: reads what the forward left in the workspace -- E_t and C_{t-1}, both (frame, element, chain) so that a wavefront
//   stores and loads 256 contiguous bytes per element -- and M_t again from the prediction. A_t = D_t + A_{t+1} M_{t+1}^T with
//   D_t = E_t (2 grad_loss / N), dM_t = C_{t-1}^T A_t (dM_0 = A_0). C_{t-1} is the stored product, never C_t M_t^{-1}: matrix
//   predictions need not be orthonormal. No reduction: every lane writes its own chain's gradient.
// 6-D input goes through rot6d_fwd / rot6d_bwd of the pose head (the same norm clamps and 1-ulp rcp / sqrt).
// No masking anywhere: a NaN in either operand reaches the loss.
//
// Element indices are 32-bit: B T J 9 >= 2^31 is refused (P2C_E_SHAPE) before anything is launched, as K19 / K20 do.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "p2c_lane_dev.h"
#include "p2c_host.h"
#include "p2c_pose_head_dev.h"

namespace p2c_pcl {

using p2c::M3;
using p2c::SixD;

constexpr int kMaxBlocks = 4096;   // one float of the workspace per workgroup; 16 wavefronts per CU on 256 CUs
constexpr int kHeader = 16;        // floats in front of the partials: word 0 is the arrival ticket (a 16-byte memset zeroes it)

struct Args {
  const float *pred, *target;
  float *ws_e, *ws_c;              // (T, 9, n) each: E_t and C_t (C_{T-1} is never read and not stored)
  float *partials;                 // (gridDim.x)
  unsigned *ticket;
  float *loss, *grad_pred;
  const float *grad_loss;
  int32_t n, T, J;                 // chains, frames per chain, chains per clip
  float scale;                     // backward: 2 / N (mean) or 2 (sum)
  double inv_n;                    // forward: 1 / N (mean) or 1 (sum)
};

template <bool SIXD>
struct Operand {                   // one frame of one chain as it comes from memory
  float p[SIXD ? 6 : 9];
};

template <bool SIXD>
__device__ __forceinline__ Operand<SIXD> load_pred(const float *pred, int elem) {
  Operand<SIXD> o;
  const float *p = pred + (size_t)elem * (SIXD ? 6 : 9);
  if (SIXD) {                      // 24-byte rows: 8-byte aligned
    const float2 *q = reinterpret_cast<const float2 *>(p);
    const float2 a = q[0], b = q[1], c = q[2];
    o.p[0] = a.x, o.p[1] = a.y, o.p[2] = b.x, o.p[3] = b.y, o.p[4] = c.x, o.p[5] = c.y;
  } else {
#pragma unroll
    for (int k = 0; k < 9; ++k) o.p[k] = p[k];
  }
  return o;
}
__device__ __forceinline__ M3 load_m3(const float *base, int elem) {
  M3 m;
  const float *p = base + (size_t)elem * 9;
#pragma unroll
  for (int k = 0; k < 9; ++k) m.m[k] = p[k];
  return m;
}
template <bool SIXD>
__device__ __forceinline__ M3 to_matrix(const Operand<SIXD> &o, SixD &s) {
  if (SIXD) return p2c::rot6d_fwd(o.p, s);
  M3 m;
#pragma unroll
  for (int k = 0; k < (SIXD ? 6 : 9); ++k) m.m[k] = o.p[k];
  return m;
}

template <bool SIXD>
__global__ __launch_bounds__(64) void pose_change_loss_fwd_kernel(const Args a) {
  const int lane = threadIdx.x, stride = (int)gridDim.x * 64;
  const size_t n = (size_t)a.n;
  float acc = 0.f;
  for (int64_t c64 = (int64_t)blockIdx.x * 64 + lane; c64 < a.n; c64 += stride) {
    const int c = (int)c64, b = c / a.J, e0 = b * a.T * a.J + (c - b * a.J);   // element (b, 0, j); frame t is e0 + t J
    Operand<SIXD> cur = load_pred<SIXD>(a.pred, e0), nxt = cur;
    M3 g = load_m3(a.target, e0), gn = g;
    M3 C, Gc;
    for (int t = 0; t < a.T; ++t) {
      if (t + 1 < a.T) {                       // next frame's operands are in flight during this frame's products
        nxt = load_pred<SIXD>(a.pred, e0 + (t + 1) * a.J);
        gn = load_m3(a.target, e0 + (t + 1) * a.J);
      }
      SixD s;
      const M3 m = to_matrix<SIXD>(cur, s);
      if (t == 0) C = m, Gc = g;
      else C = p2c::mul(C, m), Gc = p2c::mul(Gc, g);
      float *we = a.ws_e + (size_t)t * 9 * n + c, *wc = a.ws_c + (size_t)t * 9 * n + c;
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        const float e = C.m[k] - Gc.m[k];
        acc = fmaf(e, e, acc);
        we[(size_t)k * n] = e;
      }
      if (t + 1 < a.T) {
#pragma unroll
        for (int k = 0; k < 9; ++k) wc[(size_t)k * n] = C.m[k];
      }
      cur = nxt, g = gn;
    }
  }
  // ---- wavefront sum (fixed xor tree), publish, draw the ticket -------------------------------------------------------------
  acc = p2c::wave_sum(acc);
  if (lane == 0)                                                   // write-through (sc1): the last arriver sits on another CU
    __hip_atomic_store(reinterpret_cast<unsigned *>(a.partials) + blockIdx.x, __float_as_uint(acc), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                 // the storing wave drains before it signals
  unsigned ticket = 0;
  if (lane == 0) ticket = __hip_atomic_fetch_add(a.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  ticket = __builtin_amdgcn_readfirstlane(ticket);                 // (the returned value is used: the add has completed)
  if (ticket != gridDim.x - 1) return;
  // ---- last arriver: every partial is published. Lane l adds l, l + 64, ... in order, then the xor tree, in fp64 ----------
  double s = 0.0;
  for (int i = lane; i < (int)gridDim.x; i += 64)
    s += (double)__uint_as_float(__hip_atomic_load(reinterpret_cast<unsigned *>(a.partials) + i, __ATOMIC_RELAXED,
                                                   __HIP_MEMORY_SCOPE_AGENT));
  s = p2c_lane::xor_sum<64>(s);
  if (lane == 0) *a.loss = (float)(s * a.inv_n);
}

template <bool SIXD>
struct BwdFrame {
  Operand<SIXD> p;
  float e[9], c[9];                // E_t and C_{t-1}
};
template <bool SIXD>
__device__ __forceinline__ BwdFrame<SIXD> load_bwd(const Args &a, int e0, int c, int t) {
  BwdFrame<SIXD> f;
  const size_t n = (size_t)a.n;
  f.p = load_pred<SIXD>(a.pred, e0 + t * a.J);
  const float *we = a.ws_e + (size_t)t * 9 * n + c;
#pragma unroll
  for (int k = 0; k < 9; ++k) f.e[k] = we[(size_t)k * n];
  if (t > 0) {
    const float *wc = a.ws_c + (size_t)(t - 1) * 9 * n + c;
#pragma unroll
    for (int k = 0; k < 9; ++k) f.c[k] = wc[(size_t)k * n];
  } else {
#pragma unroll
    for (int k = 0; k < 9; ++k) f.c[k] = 0.f;
  }
  return f;
}

template <bool SIXD>
__global__ __launch_bounds__(64) void pose_change_loss_bwd_kernel(const Args a) {
  const int lane = threadIdx.x, stride = (int)gridDim.x * 64;
  const float scale = a.scale * *a.grad_loss;                      // D_t = E_t (2 grad_loss / N)
  constexpr int W = SIXD ? 6 : 9;
  for (int64_t c64 = (int64_t)blockIdx.x * 64 + lane; c64 < a.n; c64 += stride) {
    const int c = (int)c64, b = c / a.J, e0 = b * a.T * a.J + (c - b * a.J);
    BwdFrame<SIXD> cur = load_bwd<SIXD>(a, e0, c, a.T - 1), nxt = cur;
    M3 A = p2c::zero3(), Mn = p2c::zero3();                        // A_{t+1} and M_{t+1}: zero beyond the last frame
    for (int t = a.T - 1; t >= 0; --t) {
      if (t > 0) nxt = load_bwd<SIXD>(a, e0, c, t - 1);            // the earlier frame is in flight during this one
      SixD s;
      const M3 m = to_matrix<SIXD>(cur.p, s);
      const M3 AM = p2c::mulNT(A, Mn);
#pragma unroll
      for (int k = 0; k < 9; ++k) A.m[k] = fmaf(cur.e[k], scale, AM.m[k]);
      M3 dM = A;
      if (t > 0) {
        M3 Cp;
#pragma unroll
        for (int k = 0; k < 9; ++k) Cp.m[k] = cur.c[k];
        dM = p2c::mulTN(Cp, A);
      }
      float *gp = a.grad_pred + (size_t)(e0 + t * a.J) * W;
      if (SIXD) {
        float gy6[6];
        p2c::rot6d_bwd(s, dM, gy6);
        float2 *q = reinterpret_cast<float2 *>(gp);
        q[0] = make_float2(gy6[0], gy6[1]), q[1] = make_float2(gy6[2], gy6[3]), q[2] = make_float2(gy6[4], gy6[5]);
      } else {
#pragma unroll
        for (int k = 0; k < 9; ++k) gp[k] = dM.m[k];
      }
      Mn = m;
      cur = nxt;
    }
  }
}

// everything that can be refused, in two steps: nothing is launched unless both return 0
static int check_shape(const p2c_pose_change_loss_desc *d) {
  if (!d) return P2C_E_NULL;
  if ((d->pred_is_6d | 1) != 1 || (d->cumulative | 1) != 1 || (d->mean | 1) != 1) return P2C_E_ENUM;
  if (d->B < 0 || d->T < 1 || d->J < 1 || d->max_blocks < 0) return P2C_E_SHAPE;
  const int64_t lim = (((int64_t)1 << 31) - 1) / 9, tj = (int64_t)d->T * d->J;   // B T J 9 < 2^31, formed without overflow
  if (tj > lim || d->B > lim / tj) return P2C_E_SHAPE;
  return 0;
}
static int check(const p2c_pose_change_loss_desc *d, bool bwd, Args &a, int &blocks) {
  const int rc = check_shape(d);
  if (rc) return rc;
  if (!d->pred || !d->target || !d->workspace) return P2C_E_NULL;
  if (bwd ? (!d->grad_pred || !d->grad_loss) : !d->loss) return P2C_E_NULL;
  if (reinterpret_cast<uintptr_t>(d->workspace) & 15) return P2C_E_SHAPE;
  if (d->pred_is_6d && ((reinterpret_cast<uintptr_t>(d->pred) & 7) || (bwd && (reinterpret_cast<uintptr_t>(d->grad_pred) & 7))))
    return P2C_E_SHAPE;                                            // the 24-byte rows move as three 8-byte words
  const int64_t elems = d->B * d->T * d->J;
  // the direct form is the cumulative one over chains of a single frame
  a.T = d->cumulative ? d->T : 1;
  a.J = d->cumulative ? d->J : d->T * d->J;
  a.n = (int32_t)(d->B * a.J);
  a.pred = d->pred, a.target = d->target, a.loss = d->loss, a.grad_pred = d->grad_pred, a.grad_loss = d->grad_loss;
  a.ticket = reinterpret_cast<unsigned *>(d->workspace);
  a.partials = d->workspace + kHeader;
  a.ws_e = d->workspace + kHeader + kMaxBlocks;
  a.ws_c = a.ws_e + elems * 9;
  const double N = (double)elems * 9.0;
  a.inv_n = d->mean && elems > 0 ? 1.0 / N : 1.0;
  a.scale = (float)(d->mean && elems > 0 ? 2.0 / N : 2.0);
  const int cap = d->max_blocks > 0 && d->max_blocks < kMaxBlocks ? d->max_blocks : kMaxBlocks;
  const int64_t want = ((int64_t)a.n + 63) / 64;
  blocks = (int)(want < cap ? want : cap);
  return 0;
}

}  // namespace p2c_pcl

using namespace p2c_pcl;

extern "C" int64_t p2c_pose_change_loss_workspace_floats(const p2c_pose_change_loss_desc *d) {
  const int rc = check_shape(d);                                   // the size depends on the shape alone
  if (rc) return rc;
  return kHeader + kMaxBlocks + 2 * 9 * (d->B * d->T * d->J);      // [ticket | partials | E | C]
}

extern "C" int p2c_pose_change_loss_fwd(const p2c_pose_change_loss_desc *d, void *stream_) {
  Args a{};
  int blocks = 0;
  const int rc = check(d, false, a, blocks);
  if (rc) return rc;
  if (d->B == 0) return 0;
  hipStream_t stream = (hipStream_t)stream_;
  hipError_t e = hipMemsetAsync(d->workspace, 0, 16, stream);      // the arrival ticket
  if (e != hipSuccess) return (int)e;
  if (d->pred_is_6d) hipLaunchKernelGGL(pose_change_loss_fwd_kernel<true>, dim3(blocks), dim3(64), 0, stream, a);
  else hipLaunchKernelGGL(pose_change_loss_fwd_kernel<false>, dim3(blocks), dim3(64), 0, stream, a);
  return p2c_host::launch_status();
}

extern "C" int p2c_pose_change_loss_bwd(const p2c_pose_change_loss_desc *d, void *stream_) {
  Args a{};
  int blocks = 0;
  const int rc = check(d, true, a, blocks);
  if (rc) return rc;
  if (d->B == 0) return 0;
  hipStream_t stream = (hipStream_t)stream_;
  if (d->pred_is_6d) hipLaunchKernelGGL(pose_change_loss_bwd_kernel<true>, dim3(blocks), dim3(64), 0, stream, a);
  else hipLaunchKernelGGL(pose_change_loss_bwd_kernel<false>, dim3(blocks), dim3(64), 0, stream, a);
  return p2c_host::launch_status();
}
