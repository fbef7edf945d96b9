// p2c_frames.hip -- K33: decoded video clips -> the input frames of the pose-estimation flow (gfx950).
//
// Reference: data/base/mixins/dataset/video_mixin.py:143-184 (crop_bbox / extract_bbox_from_frame: a zero canvas and one paste per
// frame in a Python loop) and transforms/video/video_to_resnet.py:14-56 (torchvision equalize -- a histogram and a look-up table per
// frame and channel --, an antialiased bilinear resize per frame in a second loop, / 255, ImageNet mean / std, stack).
//
// The image of a frame is either the frame itself or, under the bbox crop, the canvas x canvas square the reference pastes the frame
// into; the canvas is never formed: image pixel (y, x) is frame pixel (y - cys + fy0, x - cxs + fx0) inside the pasted window
// [cys, cys + fh) x [cxs, cxs + fw) and level 0 outside it (geometry(), extract_bbox_from_frame's integer arithmetic).
//
// Launch A  frames_hist_kernel. One workgroup per 32 rows of a frame's pasted window (the grid is sized for the largest window a
//   frame can have; a workgroup past its frame's window leaves). A wavefront walks a row's fw * 3 bytes as aligned dwords (byte
//   loads for the <= 3 bytes in front and behind), channel = byte index mod 3, and counts into its own 3 x 256 LDS table with LDS
//   atomics; the four tables are added and the non-zero sums go to the frame's (3, 256) int32 counts with global atomics. Integer
//   sums: exact in any order. The counts are zeroed by a memset node in front.
// Launch B  frames_out_kernel. Every workgroup first rebuilds its frame's three look-up tables from the 768 counts (+ the zero
//   padding, image pixels - window pixels, on bin 0): a wavefront scan, four wavefront totals through LDS, then the integer formula
//   of torchvision's _scale_channel; the tables are kept in LDS as the fp32 level. Then
//     no resampling: 256 consecutive pixels of the image, lut -> normalise -> three plane stores (coalesced along w);
//     resampling: one 8 x 64 output tile. 64 lanes = 64 output columns. The tile's source rows are walked in chunks of 16: wavefront
//       w forms the horizontal sums of rows w, w + 4, ... for its column and the three channels (taps over the lut of the source
//       bytes) into LDS, then adds the chunk's rows into the vertical sums of its two output rows (w, w + 4) -- any tap count fits.
//   Tap windows and the weights' centre come from fp64 (scale = in / out, centre = scale (i + 0.5)), relative to the window's first
//   tap, so the fp32 weights max(0, 1 - |j - c| / support) / total keep full precision at any coordinate. round half-even, then
//   (level / 255 - mean) / std with two IEEE divisions.
// Bounds: a source address is formed only from (row, column) tested against the pasted window, which geometry() clips to the frame;
// the host checks every clip block against src_bytes; output indices are tested against (out_h, out_w).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/p2c.h"
#include "p2c_host.h"

namespace p2c_fr {

constexpr int kMaxClips = P2C_FRAMES_MAX_CLIPS;
constexpr int kMaxSide = P2C_FRAMES_MAX_SIDE;
constexpr int kHistRows = 32;                 // window rows per workgroup of launch A
constexpr int kTileW = 64, kTileH = 8;        // output tile of launch B
constexpr int kChunk = 16;                    // source rows per pass through LDS
constexpr int kFarCentre = 1 << 20;           // centres are clamped here: beyond it the window is empty anyway (sides <= 8192)

struct Clip {
  int64_t src_off, out_off;                   // bytes into src; floats into out
  int32_t H, W, canvas, oh, ow;
  int32_t first_block, blocks_per_frame, pad;
};

struct Args {
  const uint8_t *src;
  const int32_t *centres;
  int32_t *counts;
  float *out;
  int32_t N, T;
  Clip clips[kMaxClips];
};

struct Geo {
  int vh, vw;                                 // the image: the frame, or the canvas
  int cys, cxs, fy0, fx0, fh, fw;             // pasted window: image origin, frame origin, size (fh, fw >= 0)
};

__device__ __forceinline__ Geo geometry(const Clip &c, const int32_t *centres, int64_t frame) {
  Geo g;
  if (c.canvas == 0) {
    g.vh = c.H, g.vw = c.W, g.cys = 0, g.cxs = 0, g.fy0 = 0, g.fx0 = 0, g.fh = c.H, g.fw = c.W;
    return g;
  }
  const int half = c.canvas / 2;
  const int cx = min(max(centres[frame * 2], -kFarCentre), kFarCentre);
  const int cy = min(max(centres[frame * 2 + 1], -kFarCentre), kFarCentre);
  g.vh = c.canvas, g.vw = c.canvas;
  g.fx0 = max(0, cx - half), g.fy0 = max(0, cy - half);
  g.fw = max(min(c.W, cx + half) - g.fx0, 0), g.fh = max(min(c.H, cy + half) - g.fy0, 0);
  g.cxs = max(0, half - cx), g.cys = max(0, half - cy);
  if (g.fw == 0 || g.fh == 0) g.fw = 0, g.fh = 0, g.fx0 = 0, g.fy0 = 0, g.cxs = 0, g.cys = 0;
  return g;
}

// the clip a workgroup belongs to: first_block is ascending, N <= 64 entries in the kernel arguments (a scalar loop)
__device__ __forceinline__ int find_clip(const Args &a, int block) {
  int ci = 0;
  for (int i = 1; i < a.N; ++i)
    if (block >= a.clips[i].first_block) ci = i;
  return ci;
}

__global__ __launch_bounds__(256) void frames_hist_kernel(const Args a) {
  __shared__ int hist[4][768];
  const int ci = find_clip(a, (int)blockIdx.x);
  const Clip &c = a.clips[ci];
  const int local = (int)blockIdx.x - c.first_block;
  const int t = local / c.blocks_per_frame, part = local - t * c.blocks_per_frame;
  if (t >= a.T) return;
  const int64_t frame = (int64_t)ci * a.T + t;
  const Geo g = geometry(c, a.centres, frame);
  const int r0 = part * kHistRows, r1 = min(r0 + kHistRows, g.fh);
  if (r0 >= r1) return;                                              // workgroup-uniform
  for (int i = threadIdx.x; i < 4 * 768; i += 256) (&hist[0][0])[i] = 0;
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int *h = hist[wave];
  const uint8_t *img = a.src + c.src_off + (int64_t)t * c.H * c.W * 3;
  const int nbytes = g.fw * 3;
  for (int r = r0 + wave; r < r1; r += 4) {
    const uint8_t *p = img + ((int64_t)(g.fy0 + r) * c.W + g.fx0) * 3;
    const int head = min((int)((4 - ((uintptr_t)p & 3)) & 3), nbytes);
    const int body = (nbytes - head) >> 2, tail = nbytes - head - 4 * body;
    const uint32_t *q = (const uint32_t *)(p + head);
    for (int i = lane; i < body; i += 64) {
      const uint32_t v = q[i];
      const int m = (head + 4 * i) % 3;                              // channel of the dword's first byte
      const int m1 = m == 2 ? 0 : m + 1, m2 = m1 == 2 ? 0 : m1 + 1;
      atomicAdd(&h[m * 256 + (v & 255)], 1);
      atomicAdd(&h[m1 * 256 + ((v >> 8) & 255)], 1);
      atomicAdd(&h[m2 * 256 + ((v >> 16) & 255)], 1);
      atomicAdd(&h[m * 256 + (v >> 24)], 1);
    }
    if (lane < head) {
      atomicAdd(&h[(lane % 3) * 256 + p[lane]], 1);
    } else if (lane >= 8 && lane - 8 < tail) {
      const int idx = head + 4 * body + lane - 8;
      atomicAdd(&h[(idx % 3) * 256 + p[idx]], 1);
    }
  }
  __syncthreads();
  int *counts = a.counts + frame * 768;
  for (int i = threadIdx.x; i < 768; i += 256) {
    const int s = (hist[0][i] + hist[1][i]) + (hist[2][i] + hist[3][i]);
    if (s) atomicAdd(&counts[i], s);
  }
}

__device__ __forceinline__ float normalise(float level, int c) {
  const float mean = c == 0 ? 0.485f : c == 1 ? 0.456f : 0.406f;
  const float sd = c == 0 ? 0.229f : c == 1 ? 0.224f : 0.225f;
  return __fdiv_rn(__fsub_rn(__fdiv_rn(level, 255.0f), mean), sd);
}

__device__ __forceinline__ float triangle(float x) {
  return fmaxf(1.0f - fabsf(x), 0.0f);
}

// torch's antialias window of output index i: first tap, tap count, the centre relative to the first tap's pixel centre, 1 / sum
__device__ __forceinline__ void tap_window(int i, int in, int out, float invscale, int &first, int &count, float &cf, float &inv_total) {
  const double scale = (double)in / (double)out, support = scale >= 1.0 ? scale : 1.0;
  const double centre = scale * ((double)i + 0.5);
  first = max((int)(centre - support + 0.5), 0);
  count = min((int)(centre + support + 0.5), in) - first;
  cf = (float)(centre - 0.5 - (double)first);
  float total = 0.f;
  for (int j = 0; j < count; ++j) total += triangle(((float)j - cf) * invscale);
  inv_total = 1.0f / total;
}

__global__ __launch_bounds__(256) void frames_out_kernel(const Args a) {
  __shared__ float lut[3][256];
  __shared__ int cum[3][256];
  __shared__ int wave_total[3][4], wave_last[3][4];
  __shared__ float inter[kChunk][3][kTileW];
  __shared__ int x_first[kTileW], x_count[kTileW], y_first[kTileH], y_count[kTileH];
  __shared__ float x_cf[kTileW], x_inv[kTileW], y_cf[kTileH], y_inv[kTileH];

  const int ci = find_clip(a, (int)blockIdx.x);
  const Clip &c = a.clips[ci];
  const int local = (int)blockIdx.x - c.first_block;
  const int t = local / c.blocks_per_frame, tile = local - t * c.blocks_per_frame;
  if (t >= a.T) return;
  const int64_t frame = (int64_t)ci * a.T + t;
  const Geo g = geometry(c, a.centres, frame);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, tid = threadIdx.x;
  const bool resample = c.oh != g.vh || c.ow != g.vw;

  // ---- the frame's three look-up tables ----
  {
    const int32_t *counts = a.counts + frame * 768;
    const int padding = g.vh * g.vw - g.fh * g.fw;                   // <= 8192^2
    int incl[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const int n = counts[ch * 256 + tid] + (tid == 0 ? padding : 0);
      int s = n, last = n ? tid : -1;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(s, d, 64);
        if (lane >= d) s += o;
      }
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) last = max(last, __shfl_xor(last, d, 64));
      incl[ch] = s;
      if (lane == 63) wave_total[ch][wave] = s;
      if (lane == 0) wave_last[ch][wave] = last;
    }
    __syncthreads();
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      int off = 0;
      for (int w = 0; w < wave; ++w) off += wave_total[ch][w];
      cum[ch][tid] = incl[ch] + off;
    }
    __syncthreads();
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      // the last non-empty bin (an image has >= 1 pixel; the clamp keeps the index in the table whatever the counts hold)
      const int last = max(max(max(wave_last[ch][0], wave_last[ch][1]), max(wave_last[ch][2], wave_last[ch][3])), 0);
      const int in_last = cum[ch][last] - (last > 0 ? cum[ch][last - 1] : 0);
      const int step = (cum[ch][255] - in_last) / 255;
      int v = tid;
      if (step != 0) v = tid == 0 ? 0 : min((cum[ch][tid - 1] + step / 2) / step, 255);
      lut[ch][tid] = (float)v;
    }
  }
  const uint8_t *img = a.src + c.src_off + (int64_t)t * c.H * c.W * 3;
  float *out = a.out + c.out_off + (int64_t)t * 3 * c.oh * c.ow;
  const int plane = c.oh * c.ow;

  if (!resample) {
    __syncthreads();
    const int p = tile * 256 + tid;
    if (p >= plane) return;
    const int y = p / g.vw, x = p - y * g.vw;
    const int sy = y - g.cys, sx = x - g.cxs;
    int v0 = 0, v1 = 0, v2 = 0;
    if (sy >= 0 && sy < g.fh && sx >= 0 && sx < g.fw) {
      const uint8_t *s = img + ((int64_t)(sy + g.fy0) * c.W + (sx + g.fx0)) * 3;
      v0 = s[0], v1 = s[1], v2 = s[2];
    }
    out[p] = normalise(lut[0][v0], 0);
    out[plane + p] = normalise(lut[1][v1], 1);
    out[2 * plane + p] = normalise(lut[2][v2], 2);
    return;
  }

  // ---- one 8 x 64 output tile ----
  const int tiles_x = (c.ow + kTileW - 1) / kTileW;
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int ox = tx * kTileW + lane, oy0 = ty * kTileH;
  const float inv_sx = g.vw >= c.ow ? (float)((double)c.ow / (double)g.vw) : 1.0f;
  const float inv_sy = g.vh >= c.oh ? (float)((double)c.oh / (double)g.vh) : 1.0f;
  if (tid < kTileW) {
    int first = 0, count = 0;
    float cf = 0.f, inv = 0.f;
    if (ox < c.ow) tap_window(ox, g.vw, c.ow, inv_sx, first, count, cf, inv);
    x_first[tid] = first, x_count[tid] = count, x_cf[tid] = cf, x_inv[tid] = inv;
  } else if (tid < kTileW + kTileH) {
    const int r = tid - kTileW;
    int first = 0, count = 0;
    float cf = 0.f, inv = 0.f;
    if (oy0 + r < c.oh) tap_window(oy0 + r, g.vh, c.oh, inv_sy, first, count, cf, inv);
    y_first[r] = first, y_count[r] = count, y_cf[r] = cf, y_inv[r] = inv;
  }
  __syncthreads();
  const int rows = min(kTileH, c.oh - oy0);                          // >= 1
  const int y_lo = y_first[0], y_hi = y_first[rows - 1] + y_count[rows - 1];   // first + count is non-decreasing in the row
  const int xf = x_first[lane], xn = x_count[lane];
  const float xc = x_cf[lane], xi = x_inv[lane];
  float acc[2][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
  for (int y0 = y_lo; y0 < y_hi; y0 += kChunk) {
    const int n = min(kChunk, y_hi - y0);
    for (int r = wave; r < n; r += 4) {
      const int sy = y0 + r - g.cys;
      float s0 = 0.f, s1 = 0.f, s2 = 0.f;
      if (sy >= 0 && sy < g.fh) {                                    // outside the window the level is 0 and lut[0] = 0
        const uint8_t *row = img + ((int64_t)(sy + g.fy0) * c.W + g.fx0) * 3;
        for (int j = 0; j < xn; ++j) {
          const int sx = xf + j - g.cxs;
          if (sx >= 0 && sx < g.fw) {
            const float w = triangle(((float)j - xc) * inv_sx) * xi;
            const uint8_t *s = row + sx * 3;
            s0 = fmaf(w, lut[0][s[0]], s0);
            s1 = fmaf(w, lut[1][s[1]], s1);
            s2 = fmaf(w, lut[2][s[2]], s2);
          }
        }
      }
      inter[r][0][lane] = s0, inter[r][1][lane] = s1, inter[r][2][lane] = s2;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int r = wave + 4 * k;
      if (r < rows) {
        const int first = y_first[r];
        const int lo = max(first, y0), hi = min(first + y_count[r], y0 + n);
        const float yc = y_cf[r], yi = y_inv[r];
        for (int y = lo; y < hi; ++y) {
          const float w = triangle(((float)(y - first) - yc) * inv_sy) * yi;
          acc[k][0] = fmaf(w, inter[y - y0][0][lane], acc[k][0]);
          acc[k][1] = fmaf(w, inter[y - y0][1][lane], acc[k][1]);
          acc[k][2] = fmaf(w, inter[y - y0][2][lane], acc[k][2]);
        }
      }
    }
    __syncthreads();
  }
  if (ox < c.ow) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int r = wave + 4 * k;
      if (r < rows) {
        float *o = out + (int64_t)(oy0 + r) * c.ow + ox;
        o[0] = normalise(rintf(acc[k][0]), 0);
        o[plane] = normalise(rintf(acc[k][1]), 1);
        o[2 * plane] = normalise(rintf(acc[k][2]), 2);
      }
    }
  }
}

constexpr int64_t kMaxBlocks = ((int64_t)1 << 31) - 1;

static int check(const p2c_clip_frames_desc *d, Args &a) {
  if (!d) return P2C_E_NULL;
  if (d->N < 1 || d->N > kMaxClips || d->T < 1 || d->src_bytes < 0) return P2C_E_SHAPE;
  bool crops = false;
  int64_t out_off = 0;
  for (int i = 0; i < d->N; ++i) {
    const p2c_clip_frames_clip &s = d->clips[i];
    if (s.H < 1 || s.H > kMaxSide || s.W < 1 || s.W > kMaxSide || s.canvas < 0 || s.canvas > kMaxSide || s.out_h < 1 ||
        s.out_h > kMaxSide || s.out_w < 1 || s.out_w > kMaxSide)
      return P2C_E_SHAPE;
    const int64_t bytes = (int64_t)d->T * s.H * s.W * 3;
    if (s.offset < 0 || s.offset > d->src_bytes || bytes > d->src_bytes - s.offset) return P2C_E_SHAPE;
    crops |= s.canvas > 0;
    Clip &c = a.clips[i];
    c.src_off = s.offset, c.out_off = out_off, c.H = s.H, c.W = s.W, c.canvas = s.canvas, c.oh = s.out_h, c.ow = s.out_w;
    c.first_block = 0, c.blocks_per_frame = 0, c.pad = 0;
    out_off += (int64_t)d->T * 3 * s.out_h * s.out_w;
  }
  if (!d->src || !d->workspace || !d->out || (crops && !d->centres)) return P2C_E_NULL;
  if (((uintptr_t)d->workspace & 3) != 0) return P2C_E_SHAPE;
  a.src = d->src, a.centres = d->centres, a.counts = d->workspace, a.out = d->out, a.N = d->N, a.T = d->T;
  return 0;
}

// blocks_per_frame / first_block of every clip for one launch; the grid, or -1 beyond 2^31 - 1 workgroups
template <class F>
static int64_t plan(Args &a, F blocks_per_frame) {
  int64_t total = 0;
  for (int i = 0; i < a.N; ++i) {
    Clip &c = a.clips[i];
    c.first_block = (int32_t)total, c.blocks_per_frame = blocks_per_frame(c);
    total += (int64_t)a.T * c.blocks_per_frame;
    if (total > kMaxBlocks) return -1;
  }
  return total;
}

}  // namespace p2c_fr

using namespace p2c_fr;

extern "C" int64_t p2c_clip_frames_workspace_bytes(int64_t frames) {
  return frames < 0 ? P2C_E_SHAPE : frames * 3 * 256 * (int64_t)sizeof(int32_t);
}

extern "C" int p2c_clip_frames_fwd(const p2c_clip_frames_desc *d, void *stream) {
  Args a{};
  const int rc = check(d, a);
  if (rc) return rc;
  Args b = a;
  // launch A: the tallest window a frame of the clip can have is min(H, canvas) rows
  const int64_t grid_a = plan(a, [](const Clip &c) {
    const int rows = c.canvas ? (c.canvas < c.H ? c.canvas : c.H) : c.H;
    return (rows + kHistRows - 1) / kHistRows;
  });
  const int64_t grid_b = plan(b, [](const Clip &c) {
    const int vh = c.canvas ? c.canvas : c.H, vw = c.canvas ? c.canvas : c.W;
    if (c.oh == vh && c.ow == vw) return (c.oh * c.ow + 255) / 256;
    return ((c.ow + kTileW - 1) / kTileW) * ((c.oh + kTileH - 1) / kTileH);
  });
  if (grid_a < 0 || grid_b < 0) return P2C_E_SHAPE;
  const hipError_t e = hipMemsetAsync(a.counts, 0, (size_t)p2c_clip_frames_workspace_bytes((int64_t)a.N * a.T), (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(frames_hist_kernel, dim3((unsigned)grid_a), dim3(256), 0, (hipStream_t)stream, a);
  hipError_t l = hipGetLastError();
  if (l != hipSuccess) return (int)l;
  hipLaunchKernelGGL(frames_out_kernel, dim3((unsigned)grid_b), dim3(256), 0, (hipStream_t)stream, b);
  return p2c_host::launch_status();
}
