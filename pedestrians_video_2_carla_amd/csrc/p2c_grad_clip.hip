// p2c_grad_clip.hip -- K29: gradient clipping inside the optimizer launch of the flat parameter buffer (gfx950).
//
// The reference builds its trainer from Lightning's argparse arguments (modeling.py:275, 353), so every run of it accepts
// --gradient_clip_val / --gradient_clip_algorithm norm|value: torch.nn.utils.clip_grad_norm_ / clip_grad_value_ between
// backward and optimizer.step(). Here the gradient is ONE flat buffer that the optimizer launch already walks, so the clip
// rides on that launch: no host sync, graph-capturable, one extra read of the gradient (norm mode) and nothing extra at all
// (value mode).
//
//   grad_sqnorm_kernel         reads the flat gradient once (float4 + scalar tail), sums (double)g * (double)g per lane ->
//                              wave -> workgroup, writes ONE double per workgroup to `partials`. Grid = sqnorm_blocks(n):
//                              ceil(ceil(n / 4) / 256) workgroups of 256 threads, at least 1, at most 1024 -- a function of n
//                              alone, so the summation order depends on n alone and two calls on the same data give the same
//                              bits. No atomics, no tickets. Every workgroup writes its slot, also one without any float4 of
//                              its own (n < 4: one workgroup, tail only).
//   adamw_clipped_kernel       adamw_kernel (p2c_optim.hip) with the clip in front of update<>: same grid, float4 body, scalar
//                              tail, zero_grad, scatter, step ticket. Norm mode: every workgroup first sums the partials in one
//                              fixed order (the kernel boundary is the only synchronisation), forms
//                                total_norm = (float)((double)grad_scale * sqrt(sum)),  coef = bound / (total_norm + 1e-6f)
//                              clamped to 1 with NaN kept (torch.clamp(max=1) keeps it, fminf would not); workgroup 0 stores
//                              total_norm. Per element g' = (g * grad_scale) * coef -- torch's order in a data-parallel step:
//                              average, then clip. Value mode: g' = clamp(g * grad_scale, -bound, bound) by compare-select,
//                              which keeps NaN as clamp_ does. update<> then runs with grad_scale = 1 (an exact product).
// p2c_optim.hip is untouched: the unclipped step keeps its bits, and a clipped step equals, bit for bit, that kernel fed
// with g' and grad_scale = 1 (tests/test_grad_clip_gpu.py).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/p2c.h"
#include "p2c_lane_dev.h"
#include "p2c_host.h"
#include "p2c_adam_math.h"

namespace p2c_grad_clip {

using p2c_optim::Coefs;
using p2c_optim::coefs;
using p2c_optim::update;

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256, kWaves = kThreads / 64, kMaxBlocks = 1024;

static int64_t sqnorm_blocks(int64_t n) {
  if (n <= 0) return 0;
  const int64_t n4 = (n + 3) >> 2;
  int64_t blocks = (n4 + kThreads - 1) / kThreads;
  return blocks > kMaxBlocks ? kMaxBlocks : blocks;
}

// lanes -> wave (xor butterfly: every lane ends with the same sum) -> workgroup (the four wave sums added in wave order by
// every thread that asks): one fixed order, the same in every workgroup
__device__ __forceinline__ double block_sum(double v, double *sw) {
  v = p2c_lane::xor_sum<64>(v);
  if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = sw[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) s += sw[w];
  return s;
}

__global__ __launch_bounds__(kThreads) void grad_sqnorm_kernel(const float *__restrict__ g, int64_t n,
                                                               double *__restrict__ partials) {
  __shared__ double sw[kWaves];
  const int64_t n4 = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const f32x4 *G = reinterpret_cast<const f32x4 *>(g);
  double acc = 0.0;
  for (int64_t i = t; i < n4; i += stride) {
    const f32x4 v = G[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) acc += (double)v[k] * (double)v[k];
  }
  const int64_t j = (n4 << 2) + t;           // the (at most three) tail elements: the first threads of workgroup 0
  if (j < n) acc += (double)g[j] * (double)g[j];
  const double s = block_sum(acc, sw);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

struct ClipArgs {
  float bound;
  int32_t n_partials;
  const double *partials;
  float *total_norm;
};

template <int MODE>
__device__ __forceinline__ float clipped(float g, float grad_scale, float k) {
#pragma clang fp contract(off)
  const float x = g * grad_scale;
  if (MODE == P2C_CLIP_NORM) return x * k;                     // k = clip coefficient
  return x < -k ? -k : (x > k ? k : x);                        // k = bound; a NaN fails both compares and stays
}

template <bool ADAMW, int MODE>
__global__ __launch_bounds__(kThreads) void adamw_clipped_kernel(const p2c_adamw_desc d, const ClipArgs a) {
  const float step = *d.step + 1.f;      // every workgroup reads the counter before it takes its completion ticket
  __shared__ Coefs sc;
  __shared__ float sk;
  __shared__ double sw[kWaves];
  double sum = 0.0;
  if (MODE == P2C_CLIP_NORM) {
    double acc = 0.0;
    for (int j = threadIdx.x; j < a.n_partials; j += kThreads) acc += a.partials[j];
    sum = block_sum(acc, sw);
  }
  if (threadIdx.x == 0) {
    Coefs c = coefs(d, step);
    float k = a.bound;
    if (MODE == P2C_CLIP_NORM) {
      const float total_norm = (float)((double)c.grad_scale * sqrt(sum));
      float coef = __fdiv_rn(a.bound, total_norm + 1e-6f);
      coef = coef < 1.f ? coef : (coef != coef ? coef : 1.f);
      if (blockIdx.x == 0) *a.total_norm = total_norm;
      k = coef;
    }
    sc = c, sk = k;
  }
  __syncthreads();
  Coefs c = sc;
  const float gs = c.grad_scale, k = sk;
  c.grad_scale = 1.f;                    // the scale is applied with the clip, in front of update<>
  const int64_t n4 = d.n >> 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  f32x4 *P = reinterpret_cast<f32x4 *>(d.param), *G = reinterpret_cast<f32x4 *>(d.grad);
  f32x4 *M = reinterpret_cast<f32x4 *>(d.exp_avg), *V = reinterpret_cast<f32x4 *>(d.exp_avg_sq);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    f32x4 p = P[i], g = G[i], m = M[i], v = V[i];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float pk = p[q], mk = m[q], vk = v[q];
      update<ADAMW>(c, pk, clipped<MODE>(g[q], gs, k), mk, vk);
      p[q] = pk, m[q] = mk, v[q] = vk;
    }
    P[i] = p, M[i] = m, V[i] = v;
    if (d.zero_grad) G[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (d.scatter_idx) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int j = d.scatter_idx[4 * i + q];
        if (j >= 0) d.scatter_dst[j] = p[q];
      }
    }
  }
  for (int64_t i = (n4 << 2) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < d.n; i += stride) {
    float p = d.param[i], m = d.exp_avg[i], v = d.exp_avg_sq[i];
    update<ADAMW>(c, p, clipped<MODE>(d.grad[i], gs, k), m, v);
    d.param[i] = p, d.exp_avg[i] = m, d.exp_avg_sq[i] = v;
    if (d.zero_grad) d.grad[i] = 0.f;
    if (d.scatter_idx) {
      const int j = d.scatter_idx[i];
      if (j >= 0) d.scatter_dst[j] = p;
    }
  }
  // step ticket: as in adamw_kernel (p2c_optim.hip)
  __syncthreads();
  if (threadIdx.x == 0) {
    if (atomicAdd(d.ticket, 1) == (int)gridDim.x - 1) {
      *d.step = step;
      *d.ticket = 0;
    }
  }
}

template <int MODE>
static void launch_step(const p2c_adamw_desc &d, const ClipArgs &a, unsigned blocks, hipStream_t stream) {
  if (d.adamw)
    hipLaunchKernelGGL((adamw_clipped_kernel<true, MODE>), dim3(blocks), dim3(kThreads), 0, stream, d, a);
  else
    hipLaunchKernelGGL((adamw_clipped_kernel<false, MODE>), dim3(blocks), dim3(kThreads), 0, stream, d, a);
}

}  // namespace p2c_grad_clip

extern "C" int64_t p2c_grad_clip_partials(int64_t n) { return p2c_grad_clip::sqnorm_blocks(n); }

extern "C" int p2c_adamw_step_clipped(const p2c_adamw_desc *desc, const p2c_clip_desc *clip, void *stream_) {
  using namespace p2c_grad_clip;
  if (!desc || !clip || !desc->param || !desc->grad || !desc->exp_avg || !desc->exp_avg_sq || !desc->step || !desc->ticket ||
      !desc->hyper)
    return P2C_E_NULL;
  if (desc->n < 0) return P2C_E_SHAPE;
  if ((desc->scatter_idx == nullptr) != (desc->scatter_dst == nullptr)) return P2C_E_NULL;
  if (clip->mode != P2C_CLIP_NORM && clip->mode != P2C_CLIP_VALUE) return P2C_E_ENUM;
  if (!(clip->bound > 0.f) || !std::isfinite(clip->bound)) return P2C_E_SHAPE;
  const bool norm = clip->mode == P2C_CLIP_NORM;
  if (norm && (!clip->partials || !clip->total_norm)) return P2C_E_NULL;
  if (desc->n == 0) return 0;
  for (const void *p : {(const void *)desc->param, (const void *)desc->grad, (const void *)desc->exp_avg,
                        (const void *)desc->exp_avg_sq})
    if (reinterpret_cast<uintptr_t>(p) & 15) return P2C_E_SHAPE;       // flat buffers are 16-byte aligned
  if (norm && (reinterpret_cast<uintptr_t>(clip->partials) & 7)) return P2C_E_SHAPE;
  hipStream_t stream = (hipStream_t)stream_;
  ClipArgs a;
  a.bound = clip->bound, a.n_partials = 0, a.partials = nullptr, a.total_norm = nullptr;
  if (norm) {
    const int64_t nb = sqnorm_blocks(desc->n);
    a.n_partials = (int32_t)nb, a.partials = clip->partials, a.total_norm = clip->total_norm;
    hipLaunchKernelGGL(grad_sqnorm_kernel, dim3((unsigned)nb), dim3(kThreads), 0, stream, (const float *)desc->grad, desc->n,
                       clip->partials);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  const int64_t n4 = (desc->n + 3) >> 2;                               // the grid of p2c_adamw_step
  int64_t blocks = (n4 + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (norm) launch_step<P2C_CLIP_NORM>(*desc, a, (unsigned)blocks, stream);
  else launch_step<P2C_CLIP_VALUE>(*desc, a, (unsigned)blocks, stream);
  return p2c_host::launch_status();
}
