// p2c_relu_stack.hip -- K21: fused ReLU stack h_{l+1} = relu(W_l h_l + b_l), l = 0 .. L-1 (1 <= L <= 5), over N = B T frame rows,
// for gfx950 on fp32 MFMA (v_mfma_f32_16x16x4_f32). The front end of Seq2SeqFlatEmbeddings (reference
// modules/movements/seq2seq/seq2seq_flat_embeddings.py:39-44 and 62-73, default 52 -> 128 -> 64): Linear + ReLU pairs over the
// flattened frame whose output feeds the encoder LSTM sequence-first, optionally time-reversed.
//
// As framework ops that is 2 L launches forward, about 5 L backward, a permute copy and a flip copy. Here it is ONE launch
// forward and ONE backward plus a fixed-order reduction of the per-workgroup weight-gradient partials.
//
// Structure: the cooperative 16-sample tile of K8 (p2c_mlp.hip), whose device functions (p2c_mlp_dev.h) are used as they are:
//   * a workgroup of eight wavefronts walks over tiles of 16 frame rows (grid-stride, ragged last tile, 64-bit row offsets);
//     activations live transposed in LDS, H_l^T[feature][sample], so the MFMA output tile of layer l is the B operand of layer
//     l + 1; the 16-row output tiles of a layer are dealt round-robin to the waves, one LDS barrier per layer;
//   * the weights are staged ONCE per workgroup, straight from the nn.Linear tensors (row-major (out, in)), into the zero-padded
//     LDS image of K8: rows 0 .. n_out, pitch ld_of(n_in) == 2 (mod 4), the bias in column n_in, a unit row n_out that hands the
//     constant-one activation row on to the next layer. No pack kernel: the forward is one launch;
//   * every product is exact fp32: the MFMA is an fmaf chain in k order;
//   * the last layer's ReLU is applied in its epilogue and the tile goes straight from the accumulators to y, SEQUENCE-FIRST:
//     input row b T + t is output row t' B + b with t' = flip ? T - 1 - t : t -- the encoder's layout, no permute / flip copy;
//   * backward: the hidden activations H_1 .. H_{L-1} are RECOMPUTED from x (no saved buffer: the recomputation is L - 1 of the
//     2 L - 1 products of a tile and spares an HBM round trip of 16 x sum(dims[1..L-1]) floats per tile each way); the last
//     layer's ReLU mask comes from y itself, applied to gy as the two tiles are loaded (same permuted rows). Then the dgrad
//     chain G_l = [H_l > 0] W_l^T G_{l+1}, l = L-1 .. 1, and the waves split the 16x16 tiles of dW_aug_l = G_{l+1}^T [H_l | 1]
//     (the bias gradient is the last column), held in MFMA accumulators across the workgroup's tiles. Every workgroup writes one
//     partial per tile (partials[block][tile][lane][4]); relu_stack_reduce_kernel adds them in workgroup order and writes, or
//     with `accumulate` adds to, gW / gb. No float atomics: two runs give the same bits. x is data: no dx is formed.
//
// Coverage (p2c_relu_stack_supported): 1 <= L <= 5, every width >= 1, and BOTH
//   (a) the LDS of the backward workgroup fits 160 KiB:
//         4 B x ( sum_l img_rows_of(dims[l+1]) x ld_of(dims[l])                      weight images, img_rows_of(n) = (n + 16) & ~15
//               + 17 x ( sum_{l=0}^{L-1} act_rows_of(dims[l])                        H_0 .. H_{L-1},   act_rows_of(n) = pad16(n) + 16
//                      + sum_{l=1}^{L} act_rows_of(dims[l]) ) )  <= 163 840          G_1 .. G_L
//       (the forward needs the images and H_0 .. H_{L-1} only);
//   (b) sum_l ceil(dims[l+1] / 16) x ceil((dims[l] + 1) / 16) <= 96: the weight-gradient tiles a workgroup holds in accumulators
//       (12 per wave).
// (52,128,64): 85 KB of images + 30 KB of activations, 68 tiles. (52,512,256) fails (a) with 660 KB of images.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/p2c.h"
#include "p2c_host.h"
#include "p2c_mlp_dev.h"

namespace p2c_relu_stack {

using namespace p2c_mlp;

constexpr int SL = P2C_RELU_STACK_MAX_LAYERS;
constexpr int MAX_BLOCKS = 256;            // persistent: one workgroup per CU
constexpr size_t LDS_LIMIT = 160 * 1024;
constexpr int RG = 16, RL = 16;            // reduction: RG groups of workgroup partials in parallel, RL lanes of a tile per workgroup

struct StackArgs {
  int32_t n_layers, dims[SL + 1];
  int32_t B, T, flip, accumulate;
  int64_t N;
  const float *x, *W[SL], *b[SL], *gy;
  float *y;                      // written by the forward, read (ReLU mask) by the backward
  float *gW[SL], *gb[SL], *partials;
  int32_t ld[SL], w_off[SL], w_total;
  int32_t h_off[SL + 2];         // row offset of H_l^T in the activation area (rows = act_rows_of(dims[l]))
  int32_t n_tiles_w, vec_y;
  int32_t tab[2 * MAX_SLOTS * WAVES];   // dW tile t: LDS float offsets (relative to H) of its G rows and its H rows
};

// 16 frame rows of a row-major (rows, n) tensor -> LDS transposed dst[k * TP + sample]; rows beyond N read as zero. Thread
// (sample = tid / 32, k = tid % 32 + 32 j): 32 consecutive floats of a row per half wave. PERMUTED: the tensor is sequence-first
// (y, gy), row b T + t of the stack lives at row t' B + b. MASK: dst = mask > 0 ? src : 0 (gy under the last layer's ReLU).
template <bool PERMUTED, bool MASK>
__device__ __forceinline__ void load_tile(const StackArgs &a, const float *src, const float *mask, int n, int64_t row0, float *dst) {
  const int s = threadIdx.x >> 5, k0 = threadIdx.x & 31;
  const int64_t row = row0 + s;
  const bool ok = row < a.N;
  int64_t srow = row;
  if (PERMUTED && ok) {
    const int64_t bi = row / a.T, t = row - bi * a.T;
    srow = (a.flip ? (a.T - 1 - t) : t) * (int64_t)a.B + bi;
  }
  const float *p = src + srow * n, *m = MASK ? mask + srow * n : nullptr;
  for (int k = k0; k < n; k += 32) {
    float v = ok ? p[k] : 0.f;
    if (MASK) v = (ok && m[k] > 0.f) ? v : 0.f;
    dst[k * TP + s] = v;
  }
}
static_assert(64 * WAVES == 32 * TS, "load_tile: 32 threads per sample");

// the zero-padded image of every [W_l | b_l] (see p2c_mlp.hip, mlp_pack_kernel), written straight into LDS
__device__ __forceinline__ void stage_images(const StackArgs &a, float *lds) {
  for (int l = 0; l < a.n_layers; ++l) {
    const int n_in = a.dims[l], n_out = a.dims[l + 1], ld = a.ld[l];
    const int total = (l + 1 < a.n_layers ? a.w_off[l + 1] : a.w_total) - a.w_off[l];
    const float *W = a.W[l], *b = a.b[l];
    float *img = lds + a.w_off[l];
    for (int i = threadIdx.x; i < total; i += blockDim.x) {
      const int n = i / ld, k = i - n * ld;
      float v = 0.f;
      if (n < n_out) {
        if (k < n_in) v = W[(size_t)n * n_in + k];
        else if (k == n_in) v = b[n];
      } else if (n == n_out && k == n_in) {
        v = 1.f;
      }
      img[i] = v;
    }
  }
}

__device__ __forceinline__ Lane make_lane() {
  Lane L;
  L.lane = threadIdx.x & 63, L.c = L.lane & 15, L.g = L.lane >> 4;
  L.wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  return L;
}

// LDS: [weight images | H_0 .. H_{L-1}]
__global__ __launch_bounds__(64 * WAVES) void relu_stack_fwd_kernel(const StackArgs a) {
  extern __shared__ float lds[];
  const Lane L = make_lane();
  const int nl = a.n_layers, n0 = a.dims[0], nL = a.dims[nl];
  float *H = lds + a.w_total;
  stage_images(a, lds);
  init_rows<NTH>(H, a.h_off[0] + n0, a.h_off[0] + k_rows(n0), a.h_off[0] + n0);     // the ones row and the k rounding behind the x tile
  const int64_t n_tiles = (a.N + TS - 1) / TS;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t row0 = tile * TS, row = row0 + L.c;
    const bool row_ok = row < a.N;
    int64_t orow = 0;
    if (row_ok) {
      const int64_t bi = row / a.T, t = row - bi * a.T;
      orow = (a.flip ? (a.T - 1 - t) : t) * (int64_t)a.B + bi;
    }
    lds_barrier();                          // the previous tile's layers have consumed H (first tile: nothing to wait for)
    load_tile<false, false>(a, a.x, nullptr, n0, row0, H + a.h_off[0] * TP);
    for (int l = 0; l < nl; ++l) {
      lds_barrier();                        // H_l (and, on the first tile, the images) complete
      const bool last = (l == nl - 1);
      layer_forward<P2C_PREC_F32>(L, lds + a.w_off[l], a.ld[l], a.dims[l], a.dims[l + 1], true, H + a.h_off[l] * TP,
                                  last ? nullptr : H + a.h_off[l + 1] * TP, last ? a.y + orow * nL : nullptr, row_ok,
                                  a.vec_y != 0);
    }
  }
}

// LDS: [weight images | H_0 .. H_{L-1} | G_1 .. G_L]
__global__ __launch_bounds__(64 * WAVES) void relu_stack_bwd_kernel(const StackArgs a) {
  extern __shared__ float lds[];
  const Lane L = make_lane();
  const int nl = a.n_layers, n0 = a.dims[0], nL = a.dims[nl];
  float *H = lds + a.w_total;
  float *G = H + (a.h_off[nl] - a.h_off[1]) * TP;            // G_l lives at row h_off[l] of this base (l = 1 .. L)
  stage_images(a, lds);
  init_rows<NTH>(H, a.h_off[0] + n0, a.h_off[0] + k_rows(n0), a.h_off[0] + n0);
  init_rows<NTH>(G, a.h_off[nl] + nL, a.h_off[nl] + pad16(nL), -1);   // rows of G_L the dgrad / dW phases read beyond the gy tile
  const int lane_off = L.c * TP + L.g;
  f32x4 acc[MAX_SLOTS];
#pragma unroll
  for (int i = 0; i < MAX_SLOTS; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int64_t n_tiles = (a.N + TS - 1) / TS;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t row0 = tile * TS;
    lds_barrier();                          // the previous tile's dW phase has consumed H and G
    load_tile<false, false>(a, a.x, nullptr, n0, row0, H + a.h_off[0] * TP);
    load_tile<true, true>(a, a.gy, a.y, nL, row0, G + a.h_off[nl] * TP);       // G_L = [y > 0] gy
    // ---- the hidden activations H_1 .. H_{L-1}, recomputed
    for (int l = 0; l < nl - 1; ++l) {
      lds_barrier();
      layer_forward<P2C_PREC_F32>(L, lds + a.w_off[l], a.ld[l], a.dims[l], a.dims[l + 1], true, H + a.h_off[l] * TP,
                                  H + a.h_off[l + 1] * TP, nullptr, false, false);
    }
    // ---- G_l = [H_l > 0] W_l^T G_{l+1}, l = L-1 .. 1
    for (int l = nl - 1; l >= 1; --l) {
      lds_barrier();
      layer_dgrad<P2C_PREC_F32>(L, lds + a.w_off[l], a.ld[l], a.dims[l], a.dims[l + 1], G + a.h_off[l + 1] * TP,
                                H + a.h_off[l] * TP, G + a.h_off[l] * TP);
    }
    lds_barrier();
    // ---- dW_aug_l[n][m] += sum_s G_{l+1}^T[n][s] H_l^T_aug[m][s]; tile t = slot * WAVES + wave. Slots past the last tile alias
    // tile 0 and are never written out. Samples beyond N carry G = 0.
#pragma unroll
    for (int slot = 0; slot < MAX_SLOTS; ++slot) {
      const int t = slot * WAVES + L.wave;
      const float *gp = H + a.tab[2 * t] + lane_off;       // A[n][k = sample]
      const float *hp = H + a.tab[2 * t + 1] + lane_off;   // B[k = sample][m]
      float av[4], bv[4];
#pragma unroll
      for (int s = 0; s < TS / 4; ++s) av[s] = gp[4 * s], bv[s] = hp[4 * s];
      acc[slot] = mfma_k16<P2C_PREC_F32>(av, bv, acc[slot]);
    }
  }
  f32x4 *part = reinterpret_cast<f32x4 *>(a.partials) + (size_t)blockIdx.x * a.n_tiles_w * 64;
#pragma unroll
  for (int slot = 0; slot < MAX_SLOTS; ++slot) {
    const int t = slot * WAVES + L.wave;
    if (t < a.n_tiles_w) __builtin_nontemporal_store(acc[slot], &part[t * 64 + L.lane]);   // read once, by the reduction
  }
}

// grad (+)= sum over workgroups of their partial tiles, in a fixed order, scattered to the per-layer gradient tensors. Four
// workgroups per dW tile (RL lanes each); group q adds workgroups q, q + RG, ..., the groups are added in order through LDS.
__global__ __launch_bounds__(RL * RG) void relu_stack_reduce_kernel(const StackArgs a, int n_blocks) {
  __shared__ f32x4 red[RG][RL];
  const int t = blockIdx.x / (64 / RL), li = threadIdx.x % RL, q = threadIdx.x / RL;
  const int lane = (blockIdx.x % (64 / RL)) * RL + li;        // lane of the MFMA C tile this thread reduces
  const size_t stride = (size_t)a.n_tiles_w * 64;
  const f32x4 *p = reinterpret_cast<const f32x4 *>(a.partials) + (size_t)t * 64 + lane;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  int w = q;
  for (; w + 3 * RG < n_blocks; w += 4 * RG) {      // four loads in flight, added in workgroup order
    f32x4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = __builtin_nontemporal_load(&p[(size_t)(w + u * RG) * stride]);
#pragma unroll
    for (int u = 0; u < 4; ++u) s += v[u];
  }
  for (; w < n_blocks; w += RG) s += __builtin_nontemporal_load(&p[(size_t)w * stride]);
  red[q][li] = s;
  __syncthreads();
  if (q != 0) return;
#pragma unroll
  for (int i = 1; i < RG; ++i) s += red[i][li];
  const TileRef tr = locate_tile(a.dims, t);
  const int n_in = a.dims[tr.l], n_out = a.dims[tr.l + 1];
  const int m = tr.mtile * 16 + (lane & 15);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int n = tr.ntile * 16 + 4 * (lane >> 4) + r;
    if (n >= n_out || m > n_in) continue;
    float *g = (m < n_in) ? a.gW[tr.l] + (size_t)n * n_in + m : a.gb[tr.l] + n;
    *g = a.accumulate ? *g + s[r] : s[r];
  }
}

using p2c_host::aligned16;

// geometry only (no pointer is looked at): 0, or P2C_E_SHAPE for widths the kernel does not cover
static int fill_shape(StackArgs &a, const p2c_relu_stack_desc *d) {
  a = StackArgs{};
  if (d->n_layers < 1 || d->n_layers > SL) return P2C_E_SHAPE;
  const int nl = a.n_layers = d->n_layers;
  int rows = 0, tiles = 0;
  int64_t wtot = 0;
  for (int l = 0; l <= nl; ++l) {
    if (d->dims[l] < 1 || d->dims[l] > (1 << 14)) return P2C_E_SHAPE;
    a.dims[l] = d->dims[l];
    a.h_off[l] = rows;
    rows += act_rows_of(a.dims[l]);
  }
  a.h_off[nl + 1] = rows;
  for (int l = 0; l < nl; ++l) {
    tiles += ((a.dims[l + 1] + 15) / 16) * ((a.dims[l] + 1 + 15) / 16);
    a.ld[l] = ld_of(a.dims[l]);
    if (wtot > (int64_t)LDS_LIMIT) return P2C_E_SHAPE;
    a.w_off[l] = (int32_t)wtot;
    wtot += (int64_t)img_rows_of(a.dims[l + 1]) * a.ld[l];
  }
  if (wtot > (int64_t)LDS_LIMIT || tiles > MAX_SLOTS * WAVES) return P2C_E_SHAPE;
  a.w_total = ((int32_t)wtot + 3) & ~3;
  a.n_tiles_w = tiles;
  int t = 0;
  for (int l = 0; l < nl; ++l) {
    const int ntl = (a.dims[l + 1] + 15) / 16, mtl = (a.dims[l] + 1 + 15) / 16;
    for (int nt = 0; nt < ntl; ++nt)
      for (int mt = 0; mt < mtl; ++mt, ++t) {
        a.tab[2 * t] = (a.h_off[nl] - a.h_off[1] + a.h_off[l + 1] + nt * 16) * TP;     // G rows live behind the H area
        a.tab[2 * t + 1] = (a.h_off[l] + mt * 16) * TP;
      }
  }
  for (; t < MAX_SLOTS * WAVES; ++t) a.tab[2 * t] = a.tab[0], a.tab[2 * t + 1] = a.tab[1];
  return 0;
}
static size_t lds_fwd(const StackArgs &a) { return ((size_t)a.w_total + (size_t)a.h_off[a.n_layers] * TP) * sizeof(float); }
static size_t lds_bwd(const StackArgs &a) {
  return ((size_t)a.w_total + (size_t)(a.h_off[a.n_layers] + a.h_off[a.n_layers + 1] - a.h_off[1]) * TP) * sizeof(float);
}

static int fill(StackArgs &a, const p2c_relu_stack_desc *d) {
  if (!d || !d->x) return P2C_E_NULL;
  int rc = fill_shape(a, d);
  if (rc) return rc;
  if (lds_bwd(a) > LDS_LIMIT || d->B < 0 || d->T < 1) return P2C_E_SHAPE;
  a.B = d->B, a.T = d->T, a.flip = d->flip != 0, a.accumulate = d->accumulate != 0;
  a.N = (int64_t)d->B * d->T;
  a.x = d->x, a.y = d->y, a.gy = d->gy, a.partials = d->workspace;
  for (int l = 0; l < a.n_layers; ++l) {
    if (!d->W[l] || !d->b[l]) return P2C_E_NULL;
    a.W[l] = d->W[l], a.b[l] = d->b[l], a.gW[l] = d->gW[l], a.gb[l] = d->gb[l];
  }
  a.vec_y = (a.dims[a.n_layers] % 4 == 0) && aligned16(a.y);
  return 0;
}

static inline int n_blocks(int64_t N) {
  const int64_t n_tiles = (N + TS - 1) / TS;
  return (int)(n_tiles < MAX_BLOCKS ? (n_tiles < 1 ? 1 : n_tiles) : MAX_BLOCKS);
}
static void allow_big_lds() {
  static bool done = false;
  if (done) return;
  (void)hipFuncSetAttribute((const void *)relu_stack_fwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_LIMIT);
  (void)hipFuncSetAttribute((const void *)relu_stack_bwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_LIMIT);
  done = true;
}

}  // namespace p2c_relu_stack

using namespace p2c_relu_stack;

extern "C" int p2c_relu_stack_supported(const p2c_relu_stack_desc *d) {
  StackArgs a;
  if (!d || fill_shape(a, d)) return 0;
  return lds_bwd(a) <= LDS_LIMIT ? 1 : 0;
}

extern "C" int64_t p2c_relu_stack_workspace_floats(const p2c_relu_stack_desc *d) {
  StackArgs a;
  if (!d || fill_shape(a, d) || d->B < 0 || d->T < 1) return 0;
  return (int64_t)n_blocks((int64_t)d->B * d->T) * a.n_tiles_w * 256;
}

extern "C" int p2c_relu_stack_fwd(const p2c_relu_stack_desc *d, void *stream_) {
  StackArgs a;
  int rc = fill(a, d);
  if (rc) return rc;
  if (!a.y) return P2C_E_NULL;
  if (a.N == 0) return 0;
  allow_big_lds();
  hipLaunchKernelGGL(relu_stack_fwd_kernel, dim3(n_blocks(a.N)), dim3(64 * WAVES), lds_fwd(a), (hipStream_t)stream_, a);
  return p2c_host::launch_status();
}

extern "C" int p2c_relu_stack_bwd(const p2c_relu_stack_desc *d, void *stream_) {
  StackArgs a;
  int rc = fill(a, d);
  if (rc) return rc;
  if (!a.y || !a.gy || !a.partials) return P2C_E_NULL;
  for (int l = 0; l < a.n_layers; ++l)
    if (!a.gW[l] || !a.gb[l]) return P2C_E_NULL;
  allow_big_lds();
  const int blocks = n_blocks(a.N);           // N == 0: one workgroup writes a zero partial, the gradients are zero
  hipLaunchKernelGGL(relu_stack_bwd_kernel, dim3(blocks), dim3(64 * WAVES), lds_bwd(a), (hipStream_t)stream_, a);
  hipLaunchKernelGGL(relu_stack_reduce_kernel, dim3(a.n_tiles_w * (64 / RL)), dim3(RL * RG), 0, (hipStream_t)stream_, a, blocks);
  return p2c_host::launch_status();
}
