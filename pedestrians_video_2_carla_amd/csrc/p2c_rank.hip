// p2c_rank.hip -- K25: the ranking behind AUROC, the ROC curve and the precision / recall curve (gfx950).
//
// scores (N, C) float, targets (N) int32. Class c is ranked one-vs-rest (a row is positive when target == c; with ONE column the
// labels are 0 / 1 and a row is positive when target == 1). A row whose target lies outside the label range, or that holds a NaN
// score in any column, is dropped everywhere. Per class: the kept rows sorted by score, descending; rows with equal scores (-0.0 and
// +0.0 are equal) form one group; for every group, in order, its score (thresholds), the number of positives (tps) and of negatives
// (fps) ranked at or above it -- scikit-learn's _binary_clf_curve -- and from those the integer trapezoid
//   num = sum_k (fps[k] - fps[k-1]) (tps[k] + tps[k-1]),    AUROC = num / (2 P Q),  P = tps[last], Q = fps[last]
// in 64-bit integers with ONE fp64 division (both sides < 2^53 for N <= 2^24: the correctly rounded value).
//
// The sorted element is 64 bits: [63:32] an order-preserving image of the float, inverted, so that an ASCENDING integer sort is a
// DESCENDING score; [0] the positive bit. Kept scores are not NaN, so the largest image a kept row can have is -inf's 0xFF800000;
// dropped rows and padding carry 0xFFFFFFFF and sort behind every kept row without ever sharing its group.
//
// Two regimes, the same output bits (everything after the sort is integer arithmetic on a uniquely defined order of groups, and no
// output depends on the order of rows inside a group):
//   LDS     N <= 16384 (16384 x 8 B = 128 KiB + 16 KiB of scan scratch in the CU's 160 KiB): one workgroup per class, bitonic sort
//           over the next power of two, group ends, prefix counts, compaction and the AUROC sum in the same launch.
//   global  any N <= 2^24 (or P2C_RANK_GLOBAL): one launch forms the elements, then a least-significant-digit radix sort in the
//           workspace, 4-bit digits over the 32 image bits = 8 passes of 3 launches (tile digit counts, scan, scatter). Every thread
//           owns a contiguous run of its tile, and its digit counts sit in an LDS table scanned bin-major, so a pass is stable with
//           no sort inside the tile. Then tile counts, their scan, the compacting write and the AUROC sum: 29 launches.
// Sums here are integers, so their order cannot change a bit; two runs give the same bits.
//
// p2c_rank_scores: logits (B, C) + int64 targets -> fp32 softmax (maximum subtracted) or, with P2C_CLS_BINARY, sigmoid scores formed
// from exp(-|x|) as K24 forms them, and int32 targets (-1 for a label outside the range), written at a row offset of the epoch buffers.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/p2c.h"
#include "p2c_host.h"

namespace p2c_rank {

typedef unsigned long long u64;

constexpr int CMAX = 32;
constexpr int LDS_MAX_N = 16384;
constexpr int64_t MAX_N = (int64_t)1 << 24;
constexpr int NT_LDS = 1024;                     // the LDS regime's workgroup
constexpr int NT = 256, ITEMS = 16, TILE = NT * ITEMS;   // the global regime's tile: every thread owns ITEMS contiguous elements
constexpr int RADIX = 16, PASSES = 8;
constexpr uint32_t PAD_KEY = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t key_of(float s) {
  const uint32_t b = s == 0.f ? 0u : __float_as_uint(s);         // -0.0 ties with +0.0
  const uint32_t u = (b & 0x80000000u) ? ~b : (b | 0x80000000u);  // ascending u = ascending float
  return ~u;                                                       // ascending key = descending float
}

__device__ __forceinline__ float score_of(uint32_t key) {
  const uint32_t u = ~key;
  return __uint_as_float((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u);
}

// the element of (row i, class c); a dropped row gives the padding element
__device__ __forceinline__ u64 element(const float *__restrict__ scores, const int32_t *__restrict__ targets, int64_t i, int C, int c) {
  const int t = targets[i];
  bool ok = t >= 0 && t < (C == 1 ? 2 : C);
  const float *row = scores + i * C;
  for (int k = 0; k < C; ++k) ok = ok && !(row[k] != row[k]);
  if (!ok) return (u64)PAD_KEY << 32;
  return ((u64)key_of(row[c]) << 32) | (u64)(t == (C == 1 ? 1 : c) ? 1 : 0);
}

// Exclusive prefix sum of one u64 per thread over the workgroup (Hillis-Steele on two LDS buffers of NTH each); total = the sum.
template <int NTH>
__device__ __forceinline__ u64 block_scan(u64 v, u64 *buf, u64 *total) {
  const int tid = threadIdx.x;
  u64 *a = buf, *b = buf + NTH;
  __syncthreads();                               // the buffers may still be read from an earlier use
  a[tid] = v;
  __syncthreads();
  for (int d = 1; d < NTH; d <<= 1) {
    b[tid] = tid >= d ? a[tid] + a[tid - d] : a[tid];
    __syncthreads();
    u64 *t = a;
    a = b, b = t;
  }
  *total = a[NTH - 1];
  return a[tid] - v;
}

// AUROC sum of class c from its written curve, by one workgroup; thread 0 writes the per-class results
template <int NTH>
__device__ __forceinline__ void finish_class(const int32_t *tps, const int32_t *fps, int npts, int P, int nvalid,
                                             int c, u64 *buf, int32_t *n_points, int32_t *n_pos, double *auroc, int32_t *n_valid) {
  const int tid = threadIdx.x;
  u64 acc = 0;
  for (int k = tid; k < npts; k += NTH) {
    const u64 t1 = (u64)tps[k], f1 = (u64)fps[k], t0 = k ? (u64)tps[k - 1] : 0, f0 = k ? (u64)fps[k - 1] : 0;
    acc += (f1 - f0) * (t1 + t0);
  }
  u64 num;
  block_scan<NTH>(acc, buf, &num);
  if (tid == 0) {
    const int Q = nvalid - P;
    n_points[c] = npts;
    n_pos[c] = P;
    auroc[c] = (P > 0 && Q > 0) ? (double)num / (2.0 * (double)P * (double)Q) : (double)NAN;
    if (c == 0) n_valid[0] = nvalid;
  }
}

// ---------------------------------------------------------------------------------------------------------------- LDS regime
__global__ __launch_bounds__(NT_LDS) void rank_lds_kernel(const float *__restrict__ scores, const int32_t *__restrict__ targets,
                                                          const int N, const int C, const int M, float *__restrict__ thresholds,
                                                          int32_t *tps, int32_t *fps,   // read back after the barrier: not restrict
                                                          int32_t *__restrict__ n_points, int32_t *__restrict__ n_pos,
                                                          double *__restrict__ auroc, int32_t *__restrict__ n_valid) {
  extern __shared__ __attribute__((aligned(16))) u64 lds[];
  u64 *el = lds, *buf = lds + M;                 // M elements, then 2 * NT_LDS of scan scratch
  const int tid = threadIdx.x, c = blockIdx.x;
  for (int i = tid; i < M; i += NT_LDS) el[i] = i < N ? element(scores, targets, i, C, c) : (u64)PAD_KEY << 32;
  __syncthreads();
  // bitonic sort, ascending, of M = 2^m elements
  for (int k = 2; k <= M; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (M >> 1); t += NT_LDS) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
        const u64 a = el[i], b = el[p];
        if ((a > b) == ((i & k) == 0)) el[i] = b, el[p] = a;
      }
      __syncthreads();
    }
  // every thread owns a contiguous run: counts of positives, group ends and kept rows, packed 20 bits apart (each <= 16384)
  const int per = M >= NT_LDS ? M / NT_LDS : 1, lo = tid * per, hi = lo + per <= M ? lo + per : (lo < M ? M : lo);
  u64 cnt = 0;
  for (int i = lo; i < hi; ++i) {
    const u64 e = el[i];
    const uint32_t key = (uint32_t)(e >> 32);
    if (key == PAD_KEY) continue;
    const uint32_t next = i + 1 < M ? (uint32_t)(el[i + 1] >> 32) : PAD_KEY;
    cnt += (e & 1) + ((u64)(next != key) << 20) + ((u64)1 << 40);
  }
  u64 total;
  const u64 before = block_scan<NT_LDS>(cnt, buf, &total);
  int tp = (int)(before & 0xFFFFF), g = (int)((before >> 20) & 0xFFFFF);
  const size_t base = (size_t)c * N;
  for (int i = lo; i < hi; ++i) {
    const u64 e = el[i];
    const uint32_t key = (uint32_t)(e >> 32);
    if (key == PAD_KEY) continue;
    const uint32_t next = i + 1 < M ? (uint32_t)(el[i + 1] >> 32) : PAD_KEY;
    tp += (int)(e & 1);
    if (next != key) {
      thresholds[base + g] = score_of(key);
      tps[base + g] = tp;
      fps[base + g] = i + 1 - tp;                // kept rows are a prefix of the sorted order
      ++g;
    }
  }
  __threadfence_block();
  __syncthreads();                               // the curve is written: read it back for the sum
  finish_class<NT_LDS>(tps + base, fps + base, (int)((total >> 20) & 0xFFFFF), (int)(total & 0xFFFFF), (int)(total >> 40), c, buf,
                       n_points, n_pos, auroc, n_valid);
}

// ------------------------------------------------------------------------------------------------------------- global regime
__global__ __launch_bounds__(NT) void build_kernel(const float *__restrict__ scores, const int32_t *__restrict__ targets, const int N,
                                                   const int C, u64 *__restrict__ el) {
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i >= N) return;
  const int t = targets[i];
  bool ok = t >= 0 && t < (C == 1 ? 2 : C);
  const float *row = scores + (size_t)i * C;
  for (int k = 0; k < C; ++k) ok = ok && !(row[k] != row[k]);
  for (int c = 0; c < C; ++c)
    el[(size_t)c * N + i] = ok ? ((u64)key_of(row[c]) << 32) | (u64)(t == (C == 1 ? 1 : c) ? 1 : 0) : (u64)PAD_KEY << 32;
}

// table[d * NT + tid] = how many elements of this thread's run have digit d
__device__ __forceinline__ void digit_table(const u64 *__restrict__ src, int lo, int hi, int shift, int *table) {
  const int tid = threadIdx.x;
  for (int d = 0; d < RADIX; ++d) table[d * NT + tid] = 0;
  for (int i = lo; i < hi; ++i) table[(int)((src[i] >> shift) & (RADIX - 1)) * NT + tid] += 1;
  __syncthreads();
}

__global__ __launch_bounds__(NT) void radix_count_kernel(const u64 *__restrict__ el, const int N, const int tiles, const int shift,
                                                         int *__restrict__ hist) {
  __shared__ int table[RADIX * NT];
  __shared__ int part[NT];
  const int tid = threadIdx.x, tile = blockIdx.x, c = blockIdx.y;
  const int lo0 = tile * TILE + tid * ITEMS, lo = lo0 < N ? lo0 : N, hi = lo + ITEMS < N ? lo + ITEMS : N;
  digit_table(el + (size_t)c * N, lo, hi, shift, table);
  // thread (d, q) sums 16 columns of digit d; then thread d < 16 sums its 16 parts
  int s = 0;
  for (int k = 0; k < NT / RADIX; ++k) s += table[tid * (NT / RADIX) + k];       // = table[d * NT + q * 16 + k], d = tid / 16, q = tid % 16
  part[tid] = s;
  __syncthreads();
  if (tid < RADIX) {
    int tot = 0;
    for (int q = 0; q < NT / RADIX; ++q) tot += part[tid * (NT / RADIX) + q];
    hist[((size_t)c * RADIX + tid) * tiles + tile] = tot;
  }
}

// exclusive scan, in place, of the L ints of class blockIdx.x (digit-major, tile-minor)
__global__ __launch_bounds__(NT_LDS) void radix_scan_kernel(int *__restrict__ hist, const int L) {
  __shared__ u64 buf[2 * NT_LDS];
  const int tid = threadIdx.x;
  int *h = hist + (size_t)blockIdx.x * L;
  const int per = (L + NT_LDS - 1) / NT_LDS, lo = tid * per < L ? tid * per : L, hi = lo + per < L ? lo + per : L;
  u64 s = 0;
  for (int i = lo; i < hi; ++i) s += (u64)h[i];
  u64 total;
  int run = (int)block_scan<NT_LDS>(s, buf, &total);
  for (int i = lo; i < hi; ++i) {
    const int v = h[i];
    h[i] = run;
    run += v;
  }
}

__global__ __launch_bounds__(NT) void radix_scatter_kernel(const u64 *__restrict__ src_all, u64 *__restrict__ dst_all, const int N,
                                                           const int tiles, const int shift, const int *__restrict__ hist) {
  __shared__ int table[RADIX * NT];
  __shared__ u64 buf[2 * NT];
  __shared__ int first[RADIX], goff[RADIX];
  const int tid = threadIdx.x, tile = blockIdx.x, c = blockIdx.y;
  const u64 *src = src_all + (size_t)c * N;
  u64 *dst = dst_all + (size_t)c * N;
  const int lo0 = tile * TILE + tid * ITEMS, lo = lo0 < N ? lo0 : N, hi = lo + ITEMS < N ? lo + ITEMS : N;
  digit_table(src, lo, hi, shift, table);
  // exclusive scan of the table bin-major: thread t owns entries [16 t, 16 t + 16)
  int s = 0;
  for (int k = 0; k < RADIX; ++k) s += table[tid * RADIX + k];
  u64 total;
  int run = (int)block_scan<NT>((u64)s, buf, &total);
  for (int k = 0; k < RADIX; ++k) {
    const int v = table[tid * RADIX + k];
    table[tid * RADIX + k] = run;
    run += v;
  }
  __syncthreads();
  if (tid < RADIX) {
    first[tid] = table[tid * NT];                // elements of the tile with a smaller digit
    goff[tid] = hist[((size_t)c * RADIX + tid) * tiles + tile];   // where (digit, tile) starts in the class's output
  }
  __syncthreads();
  for (int i = lo; i < hi; ++i) {                // in order: equal digits keep their order (stable)
    const u64 e = src[i];
    const int d = (int)((e >> shift) & (RADIX - 1));
    const int at = table[d * NT + tid];          // this thread's own column: no other thread touches it
    table[d * NT + tid] = at + 1;
    const int to = goff[d] + (at - first[d]);
    if (to >= 0 && to < N) dst[to] = e;
  }
}

// per tile: positives and group ends (packed 32 bits apart) and kept rows
__device__ __forceinline__ u64 run_counts(const u64 *__restrict__ el, int lo, int hi, int N, int *kept) {
  u64 cnt = 0;
  int k = 0;
  for (int i = lo; i < hi; ++i) {
    const u64 e = el[i];
    const uint32_t key = (uint32_t)(e >> 32);
    if (key == PAD_KEY) continue;
    const uint32_t next = i + 1 < N ? (uint32_t)(el[i + 1] >> 32) : PAD_KEY;
    cnt += (e & 1) + ((u64)(next != key) << 32);
    ++k;
  }
  *kept = k;
  return cnt;
}

__global__ __launch_bounds__(NT) void tile_count_kernel(const u64 *__restrict__ el_all, const int N, const int tiles,
                                                        u64 *__restrict__ tcnt, int *__restrict__ tkept) {
  __shared__ u64 buf[2 * NT];
  const int tid = threadIdx.x, tile = blockIdx.x, c = blockIdx.y;
  const int lo0 = tile * TILE + tid * ITEMS, lo = lo0 < N ? lo0 : N, hi = lo + ITEMS < N ? lo + ITEMS : N;
  int kept;
  const u64 cnt = run_counts(el_all + (size_t)c * N, lo, hi, N, &kept);
  u64 total, tk;
  block_scan<NT>(cnt, buf, &total);
  block_scan<NT>((u64)kept, buf, &tk);
  if (tid == 0) {
    tcnt[(size_t)c * tiles + tile] = total;
    tkept[(size_t)c * tiles + tile] = (int)tk;
  }
}

// exclusive scan of the tile counts of class blockIdx.x; totals[c] = {positives, groups, kept rows}
__global__ __launch_bounds__(NT_LDS) void tile_scan_kernel(u64 *__restrict__ tcnt, const int *__restrict__ tkept, const int tiles,
                                                           int *__restrict__ totals) {
  __shared__ u64 buf[2 * NT_LDS];
  const int tid = threadIdx.x, c = blockIdx.x;
  u64 *t = tcnt + (size_t)c * tiles;
  const int *tk = tkept + (size_t)c * tiles;
  const int per = (tiles + NT_LDS - 1) / NT_LDS, lo = tid * per < tiles ? tid * per : tiles, hi = lo + per < tiles ? lo + per : tiles;
  u64 s = 0, k = 0;
  for (int i = lo; i < hi; ++i) s += t[i], k += (u64)tk[i];
  u64 total, ktotal;
  u64 run = block_scan<NT_LDS>(s, buf, &total);
  block_scan<NT_LDS>(k, buf, &ktotal);
  for (int i = lo; i < hi; ++i) {
    const u64 v = t[i];
    t[i] = run;
    run += v;
  }
  if (tid == 0) {
    totals[c * 3 + 0] = (int)(total & 0xFFFFFFFFu);
    totals[c * 3 + 1] = (int)(total >> 32);
    totals[c * 3 + 2] = (int)ktotal;
  }
}

__global__ __launch_bounds__(NT) void tile_write_kernel(const u64 *__restrict__ el_all, const int N, const int tiles,
                                                        const u64 *__restrict__ tcnt, float *__restrict__ thresholds,
                                                        int32_t *__restrict__ tps, int32_t *__restrict__ fps) {
  __shared__ u64 buf[2 * NT];
  const int tid = threadIdx.x, tile = blockIdx.x, c = blockIdx.y;
  const u64 *el = el_all + (size_t)c * N;
  const int lo0 = tile * TILE + tid * ITEMS, lo = lo0 < N ? lo0 : N, hi = lo + ITEMS < N ? lo + ITEMS : N;
  int kept;
  const u64 cnt = run_counts(el, lo, hi, N, &kept);
  u64 total;
  const u64 before = block_scan<NT>(cnt, buf, &total) + tcnt[(size_t)c * tiles + tile];
  int tp = (int)(before & 0xFFFFFFFFu), g = (int)(before >> 32);
  const size_t base = (size_t)c * N;
  for (int i = lo; i < hi; ++i) {
    const u64 e = el[i];
    const uint32_t key = (uint32_t)(e >> 32);
    if (key == PAD_KEY) continue;
    const uint32_t next = i + 1 < N ? (uint32_t)(el[i + 1] >> 32) : PAD_KEY;
    tp += (int)(e & 1);
    if (next != key && g < N) {
      thresholds[base + g] = score_of(key);
      tps[base + g] = tp;
      fps[base + g] = i + 1 - tp;
      ++g;
    }
  }
}

__global__ __launch_bounds__(NT_LDS) void finish_kernel(const int32_t *__restrict__ tps, const int32_t *__restrict__ fps, const int N,
                                                        const int *__restrict__ totals, int32_t *__restrict__ n_points,
                                                        int32_t *__restrict__ n_pos, double *__restrict__ auroc,
                                                        int32_t *__restrict__ n_valid) {
  __shared__ u64 buf[2 * NT_LDS];
  const int c = blockIdx.x;
  const size_t base = (size_t)c * N;
  finish_class<NT_LDS>(tps + base, fps + base, totals[c * 3 + 1], totals[c * 3 + 0], totals[c * 3 + 2], c, buf, n_points, n_pos, auroc,
                       n_valid);
}

// ------------------------------------------------------------------------------------------------------------------- scores
__global__ __launch_bounds__(NT) void rank_scores_kernel(const float *__restrict__ logits, const int64_t *__restrict__ targets,
                                                         const int64_t B, const int C, const int binary, float *__restrict__ out_scores,
                                                         int32_t *__restrict__ out_targets, const int64_t offset) {
  const int K = binary ? 2 : C;
  for (int64_t b = (int64_t)blockIdx.x * NT + threadIdx.x; b < B; b += (int64_t)gridDim.x * NT) {
    const int64_t y = targets[b];
    out_targets[offset + b] = (y >= 0 && y < K) ? (int32_t)y : -1;
    if (binary) {
      const float x = logits[b], e = expf(-fabsf(x));
      out_scores[offset + b] = x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
      continue;
    }
    const float *row = logits + b * C;
    float *out = out_scores + (offset + b) * C;
    float m = row[0];
    for (int c = 1; c < C; ++c) m = fmaxf(m, row[c]);
    float sum = 0.f;                             // (fmaxf skips a NaN logit, the sum does not: the whole row becomes NaN and is dropped)
    for (int c = 0; c < C; ++c) sum += expf(row[c] - m);
    for (int c = 0; c < C; ++c) out[c] = expf(row[c] - m) / sum;
  }
}

static int64_t tiles_of(int64_t N) { return (N + TILE - 1) / TILE; }
static int64_t up16(int64_t v) { return (v + 15) & ~(int64_t)15; }
static bool use_lds(int64_t N, int32_t flags) { return N <= LDS_MAX_N && !(flags & P2C_RANK_GLOBAL); }

static int check_shape(int64_t N, int32_t C, int32_t flags) {
  if (flags & ~P2C_RANK_GLOBAL) return P2C_E_ENUM;
  if (N < 0 || N > MAX_N || C < 1 || C > CMAX) return P2C_E_SHAPE;
  return 0;
}

}  // namespace p2c_rank

extern "C" int64_t p2c_rank_workspace_bytes(int64_t N, int32_t C, int32_t flags) {
  using namespace p2c_rank;
  const int rc = check_shape(N, C, flags);
  if (rc) return rc;
  if (N == 0 || use_lds(N, flags)) return 0;
  const int64_t tiles = tiles_of(N);
  // two element buffers, the digit histogram, the tile counts (u64), the kept counts, the totals
  return 2 * up16((int64_t)C * N * 8) + up16((int64_t)C * RADIX * tiles * 4) + up16((int64_t)C * tiles * 8) + up16((int64_t)C * tiles * 4)
         + up16((int64_t)C * 3 * 4);
}

extern "C" int p2c_rank_curves(const p2c_rank_desc *d, void *workspace, void *stream) {
  using namespace p2c_rank;
  if (!d) return P2C_E_NULL;
  const int rc = check_shape(d->N, d->C, d->flags);
  if (rc) return rc;
  if (!d->n_points || !d->n_pos || !d->auroc || !d->n_valid) return P2C_E_NULL;
  const int N = (int)d->N, C = d->C;
  hipStream_t st = (hipStream_t)stream;
  if (N == 0) {                                  // answered without a launch (the outputs are device memory: two small fills)
    // n_points, n_pos, n_valid = 0; AUROC = NaN (all-ones bytes are a quiet NaN)
    hipError_t e = hipMemsetAsync(d->n_points, 0, sizeof(int32_t) * C, st);
    if (e == hipSuccess) e = hipMemsetAsync(d->n_pos, 0, sizeof(int32_t) * C, st);
    if (e == hipSuccess) e = hipMemsetAsync(d->n_valid, 0, sizeof(int32_t), st);
    if (e == hipSuccess) e = hipMemsetAsync(d->auroc, 0xFF, sizeof(double) * C, st);
    return e == hipSuccess ? 0 : (int)e;
  }
  if (!d->scores || !d->targets || !d->thresholds || !d->tps || !d->fps) return P2C_E_NULL;
  if (use_lds(N, d->flags)) {
    int M = 2;
    while (M < N) M <<= 1;
    const size_t lds = (size_t)M * 8 + 2 * NT_LDS * 8;
    static bool allowed = false;
    if (!allowed) {
      (void)hipFuncSetAttribute((const void *)rank_lds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                LDS_MAX_N * 8 + 2 * NT_LDS * 8);
      allowed = true;
    }
    hipLaunchKernelGGL(rank_lds_kernel, dim3(C), dim3(NT_LDS), lds, st, d->scores, d->targets, N, C, M, d->thresholds, d->tps, d->fps,
                       d->n_points, d->n_pos, d->auroc, d->n_valid);
    return p2c_host::launch_status();
  }
  if (!workspace) return P2C_E_NULL;
  const int tiles = (int)tiles_of(N);
  char *w = (char *)workspace;
  u64 *A = (u64 *)w;
  w += up16((int64_t)C * N * 8);
  u64 *Bf = (u64 *)w;
  w += up16((int64_t)C * N * 8);
  int *hist = (int *)w;
  w += up16((int64_t)C * RADIX * tiles * 4);
  u64 *tcnt = (u64 *)w;
  w += up16((int64_t)C * tiles * 8);
  int *tkept = (int *)w;
  w += up16((int64_t)C * tiles * 4);
  int *totals = (int *)w;
  const dim3 grid(tiles, C);
  hipLaunchKernelGGL(build_kernel, dim3((N + NT - 1) / NT), dim3(NT), 0, st, d->scores, d->targets, N, C, A);
  u64 *src = A, *dst = Bf;
  for (int p = 0; p < PASSES; ++p) {
    const int shift = 32 + 4 * p;
    hipLaunchKernelGGL(radix_count_kernel, grid, dim3(NT), 0, st, (const u64 *)src, N, tiles, shift, hist);
    hipLaunchKernelGGL(radix_scan_kernel, dim3(C), dim3(NT_LDS), 0, st, hist, RADIX * tiles);
    hipLaunchKernelGGL(radix_scatter_kernel, grid, dim3(NT), 0, st, (const u64 *)src, dst, N, tiles, shift, (const int *)hist);
    u64 *t = src;
    src = dst, dst = t;
  }
  hipLaunchKernelGGL(tile_count_kernel, grid, dim3(NT), 0, st, (const u64 *)src, N, tiles, tcnt, tkept);
  hipLaunchKernelGGL(tile_scan_kernel, dim3(C), dim3(NT_LDS), 0, st, tcnt, (const int *)tkept, tiles, totals);
  hipLaunchKernelGGL(tile_write_kernel, grid, dim3(NT), 0, st, (const u64 *)src, N, tiles, (const u64 *)tcnt, d->thresholds, d->tps,
                     d->fps);
  hipLaunchKernelGGL(finish_kernel, dim3(C), dim3(NT_LDS), 0, st, (const int32_t *)d->tps, (const int32_t *)d->fps, N,
                     (const int *)totals, d->n_points, d->n_pos, d->auroc, d->n_valid);
  return p2c_host::launch_status();
}

extern "C" int p2c_rank_scores(const float *logits, const int64_t *targets, int64_t B, int32_t C, int32_t flags, float *out_scores,
                               int32_t *out_targets, int64_t row_offset, int64_t capacity, void *stream) {
  using namespace p2c_rank;
  const int binary = flags & P2C_CLS_BINARY;
  if (flags & ~P2C_CLS_BINARY) return P2C_E_ENUM;
  if (B < 0 || B > MAX_N || row_offset < 0 || capacity < 0 || row_offset + B > capacity || (binary ? C != 1 : (C < 2 || C > CMAX)))
    return P2C_E_SHAPE;
  if (B == 0) return 0;
  if (!logits || !targets || !out_scores || !out_targets) return P2C_E_NULL;
  int64_t grid = (B + NT - 1) / NT;
  if (grid > 1024) grid = 1024;
  hipLaunchKernelGGL(rank_scores_kernel, dim3((unsigned)grid), dim3(NT), 0, (hipStream_t)stream, logits, targets, B, (int)C,
                     binary ? 1 : 0, out_scores, out_targets, row_offset);
  return p2c_host::launch_status();
}
