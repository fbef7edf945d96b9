// p2c_cls_head.hip -- K24: the classification head's loss, its gradient, the predicted class and the confusion counts of one batch
// in ONE launch (gfx950).
//
// Multiclass (torch.nn.CrossEntropyLoss, mean reduction): logits (B, C), 2 <= C <= 32, int64 targets (B):
//   loss = 1 / n_valid  sum_b  [ (max_b - x_b,target) + log1p(sum_{c != argmax} exp(x_bc - max_b)) ]
//   g_logits[b][c] = (softmax(x_b)[c] - [c == target_b]) / n_valid            predicted_b = first maximal logit (torch.argmax)
//   confusion[target_b][predicted_b] += 1      (caller-owned (C, C) int32, ADDED to)
// Binary (torch.nn.BCEWithLogitsLoss): logits (B), targets 0 / 1, loss_b = max(x, 0) - x y + log1p(exp(-|x|)),
//   g = (sigmoid(x) - y) / n_valid, predicted = x > 0, a 2 x 2 matrix.
// A row whose target lies outside [0, C) -- CrossEntropyLoss's ignore_index = -100, or any bad label -- is ignored everywhere: no
// loss, a zero gradient row, not in n_valid, not in the matrix; nothing is indexed with it. All rows ignored: loss = 0 / 0 = NaN.
// B is a classification batch, so ONE workgroup strides over the rows: thread i takes rows i, i + NT, ... in that order and the NT
// partial sums meet in a fixed LDS tree, so two runs give the same bits. The matrix is counted in LDS with integer atomics (the
// order does not matter for integers) and added to the caller's with one atomic per non-zero cell.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/p2c.h"
#include "p2c_host.h"

namespace p2c_cls {

constexpr int NT = 256;
constexpr int CMAX = 32;

__global__ __launch_bounds__(NT) void cls_head_kernel(const float *__restrict__ logits, const int64_t *__restrict__ targets,
                                                      const int64_t B, const int C, const int binary, const int count_only,
                                                      float *__restrict__ loss, float *__restrict__ g_logits,
                                                      int32_t *__restrict__ confusion) {
  __shared__ int cm[CMAX * CMAX];
  __shared__ float part[NT];
  __shared__ int nval[NT];
  const int tid = threadIdx.x;
  const int K = binary ? 2 : C;                  // classes of the matrix
  for (int i = tid; i < K * K; i += NT) cm[i] = 0;

  // pass 1: the number of rows that count (the gradient is divided by it)
  int nv = 0;
  for (int64_t b = tid; b < B; b += NT) {
    const int64_t y = targets[b];
    nv += (y >= 0 && y < K) ? 1 : 0;
  }
  nval[tid] = nv;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (tid < s) nval[tid] += nval[tid + s];
    __syncthreads();
  }
  const float inv = 1.f / (float)nval[0];        // (no valid row: inf, and the loss below is 0 * inf = NaN)

  // pass 2: loss, gradient, prediction, counts
  float sum = 0.f;
  for (int64_t b = tid; b < B; b += NT) {
    const int64_t y = targets[b];
    const bool ok = y >= 0 && y < K;
    if (binary) {
      const float x = logits[b];
      if (ok) atomicAdd(&cm[(int)y * 2 + (x > 0.f ? 1 : 0)], 1);
      if (count_only) continue;
      // e = exp(-|x|) <= 1; sigmoid(-|x|) = e / (1 + e) and sigmoid(|x|) = 1 / (1 + e): sigmoid(x) - y is formed without the
      // cancellation of a sigmoid near 1 against y = 1 (a confident correct row would keep no digit of its gradient)
      const float e = expf(-fabsf(x)), lo = e / (1.f + e), hi = 1.f / (1.f + e);
      if (ok) sum += fmaxf(x, 0.f) - x * (float)y + log1pf(e);
      if (g_logits) g_logits[b] = ok ? (y == 1 ? -(x >= 0.f ? lo : hi) : (x >= 0.f ? hi : lo)) * inv : 0.f;
      continue;
    }
    const float *row = logits + b * C;
    float m = row[0];
    int am = 0;
    for (int c = 1; c < C; ++c) {
      const float v = row[c];
      if (v > m) m = v, am = c;                  // strict: the FIRST maximal logit
    }
    if (ok) atomicAdd(&cm[(int)y * C + am], 1);
    if (count_only) continue;
    // sum_c exp(x_c - m) = 1 + sm, sm over the classes other than the (first) maximal one: log1p(sm) keeps the loss of a
    // confident row, and the target's gradient is -(sum of the OTHER classes) / sum rather than softmax - 1
    float sm = 0.f;
    for (int c = 0; c < C; ++c) sm += c == am ? 0.f : expf(row[c] - m);
    if (ok) sum += (m - row[(int)y]) + log1pf(sm);
    if (g_logits) {
      float *grow = g_logits + b * C;
      const float rs = 1.f / (1.f + sm);
      for (int c = 0; c < C; ++c) {
        const float e = expf(row[c] - m);
        grow[c] = ok ? (c == (int)y ? -(c == am ? sm : (1.f + sm) - e) : e) * rs * inv : 0.f;
      }
    }
  }
  if (!count_only) {
    part[tid] = sum;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
      if (tid < s) part[tid] += part[tid + s];
      __syncthreads();
    }
    if (tid == 0 && loss) loss[0] = nval[0] > 0 ? part[0] * inv : NAN;
  }
  __syncthreads();                               // every row has been counted
  if (confusion)
    for (int i = tid; i < K * K; i += NT)
      if (cm[i]) atomicAdd(&confusion[i], cm[i]);
}

}  // namespace p2c_cls

extern "C" int p2c_cls_head(const float *logits, const int64_t *targets, int64_t B, int32_t C, int32_t flags, float *loss,
                            float *g_logits, int32_t *confusion, void *stream) {
  const int binary = flags & P2C_CLS_BINARY, count_only = flags & P2C_CLS_COUNT_ONLY;
  if (flags & ~(P2C_CLS_BINARY | P2C_CLS_COUNT_ONLY)) return P2C_E_ENUM;
  if (B < 0 || B > ((int64_t)1 << 31) || (binary ? C != 1 : (C < 2 || C > p2c_cls::CMAX))) return P2C_E_SHAPE;
  if (B == 0 && count_only) return 0;
  if ((B > 0 && (!logits || !targets)) || (!count_only && !loss) || (count_only && !confusion)) return P2C_E_NULL;
  hipLaunchKernelGGL(p2c_cls::cls_head_kernel, dim3(1), dim3(p2c_cls::NT), 0, (hipStream_t)stream, logits, targets, B,
                     (int)C, binary ? 1 : 0, count_only ? 1 : 0, loss, g_logits, confusion);
  return p2c_host::launch_status();
}
