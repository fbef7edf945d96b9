// p2c_rec_step_dev.h -- the tile of the one-launch-per-step recurrences (K18 p2c_lstm_step.hip, K23 p2c_gru_step.hip): its
// constants, the two W_hh products and the host-side pieces that depend on the tile alone.
//
// A workgroup owns BM sequences x 16 hidden units with all NQ gates of those units; wave w takes sequences [16w, 16w + 16) of the
// tile, and lane (c, g) ends up with (sequence c, units 4g .. 4g + 3) of every accumulator. Both products stage their operands
// through LDS in K-chunks of KC, zero-padded. The staging loads of a chunk are all issued first, unconditionally, from clamped
// (always valid) addresses, and the zero padding is a select on the LDS write: loads under per-element branches were waited for
// one by one (measured: 107 / 221 us per forward / backward step at B = 256, H = 512). The LDS arrays are the calling kernel's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/p2c.h"
#include "p2c_rec_dev.h"

namespace p2c_rec_step {

using namespace p2c_rec;
constexpr int BM = 32;            // sequences per workgroup (16 per wave)
constexpr int NT = 64 * BM / 16;  // threads per workgroup
constexpr int KC = 64;            // K chunk staged in LDS
constexpr int KP = KC + 4;        // LDS pitch: the 16 rows x 4 k of a fragment read fall in distinct banks (two passes)

// a value loaded from global memory made resident here: the load cannot be sunk under the select that follows (a load under a
// branch makes the compiler wait for each one at the join)
__device__ __forceinline__ void pin1(float &v) { asm volatile("" : "+v"(v)); }

// where a lane stands: fragment column c and row group g of wave w; the tile starts at sequence b0 and unit ub; the lane's own
// sequence b (bc: clamped to a valid row, bok: it exists) and first unit u0
struct Lane {
  int c, g, w, b0, ub, b, u0, bc;
  bool bok;
  __device__ __forceinline__ explicit Lane(const int B) {
    const int lane = threadIdx.x & 63;
    c = lane & 15, g = lane >> 4, w = threadIdx.x >> 6;
    b0 = blockIdx.x * BM, ub = blockIdx.y * 16;
    b = b0 + w * 16 + c, u0 = ub + 4 * g;
    bc = min(b, B - 1), bok = b < B;
  }
};

// Forward: acc[q] += h[t-1] W_hh[qH + units]^T for the NQ gates. wl (NQ * 16 * KP floats), rows q * 16 + i: W_hh row q H + ub + i,
// columns k0 .. k0 + KC; hl (BM * KP floats), rows s: h[t-1] (hp, not NULL) of sequence b0 + s.
template <int NQ>
__device__ __forceinline__ void gates_product(f32x4 (&acc)[NQ], float *wl, float *hl, const float *w_hh, const float *hp,
                                              const int H, const int B, const Lane &l) {
  const int b0 = l.b0, ub = l.ub;
  for (int k0 = 0; k0 < H; k0 += KC) {
    constexpr int NW_ = NQ * 16 * KC / NT, NH_ = BM * KC / NT;
    float vw[NW_], vh[NH_];
#pragma unroll
    for (int j = 0; j < NW_; ++j) {
      const int e = threadIdx.x + j * NT, row = e / KC, k = e % KC, u = ub + (row & 15), kk = k0 + k;
      vw[j] = w_hh[((int64_t)(row >> 4) * H + min(u, H - 1)) * H + min(kk, H - 1)];
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
    const float *wa = wl + l.c * KP + l.g, *hb = hl + (l.w * 16 + l.c) * KP + l.g;
    for (int ks = 0; ks < nks; ++ks) {
      const float bv = hb[4 * ks];
#pragma unroll
      for (int q = 0; q < NQ; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[q * 16 * KP + 4 * ks], bv, acc[q], 0, 0, 0);
    }
    __syncthreads();                                      // the chunk has been read before the next one is staged
  }
}

// Backward: gn W_hh[:, units] (K = G), gn = the (B, G) gate gradients of step t + 1 (NULL: there is none, the product is 0). wl
// (16 * KP floats), rows i: W_hh[k0 + k][ub + i] (the transposed column block of the tile's units); gl (BM * KP floats), rows s:
// gn of sequence b0 + s. Four accumulators over the k-steps break the dependent MFMA chain.
__device__ __forceinline__ f32x4 state_grad_product(float *wl, float *gl, const float *w_hh, const float *gn, const int64_t G,
                                                    const int H, const int B, const Lane &l) {
  const int b0 = l.b0, ub = l.ub;
  f32x4 e[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) e[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  if (gn) {
    for (int64_t k0 = 0; k0 < G; k0 += KC) {
      constexpr int NW_ = 16 * KC / NT, NG_ = BM * KC / NT;
      float vw[NW_], vg[NG_];
#pragma unroll
      for (int j = 0; j < NW_; ++j) {
        const int x = threadIdx.x + j * NT, k = x / 16, i = x % 16;
        vw[j] = w_hh[min(k0 + k, G - 1) * H + min(ub + i, H - 1)];
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
      const float *wa = wl + l.c * KP + l.g, *gb = gl + (l.w * 16 + l.c) * KP + l.g;
      for (int j = 0; j < n16; ++j) {
#pragma unroll
        for (int q = 0; q < 4; ++q) e[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[16 * j + 4 * q], gb[16 * j + 4 * q], e[q], 0, 0, 0);
      }
      __syncthreads();
    }
  }
  return (e[0] + e[1]) + (e[2] + e[3]);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
inline int check_tbh(const int32_t T, const int32_t B, const int32_t H) {
  return (T < 0 || B < 0 || B > (1 << 20) || H < 1 || H > 1024) ? P2C_E_SHAPE : 0;
}
inline dim3 steps_grid(const int32_t B, const int32_t H) { return dim3((unsigned)((B + BM - 1) / BM), (unsigned)((H + 15) / 16)); }
// the (B, H) carry of the backward, which only the owning lane touches
inline int64_t workspace_floats(const int32_t B, const int32_t H) { return (B < 0 || H < 0) ? 0 : (int64_t)B * H; }

}  // namespace p2c_rec_step
