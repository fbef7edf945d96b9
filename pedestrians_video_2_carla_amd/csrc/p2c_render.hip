// p2c_render.hip -- K34: skeleton clips -> the video logger's uint8 frames in one launch (gfx950).
//
// The reference's PedestrianWriter renders on the host inside the training loop: per logged clip, panel and frame a PIL canvas and
// one ellipse call per joint, then numpy concatenations that merge the panels (loggers/pedestrian/pedestrian_writer.py:241-289).
// Here the panels of a logged batch -- what the model saw next to what it projected -- are one launch over (cell, video, frame,
// tile); the merged frames leave the device in one copy. The rules (include/p2c.h, K34) are integer arithmetic behind one rintf per
// coordinate, so the tensor restatement in ops.py (_render_points_tensor) gives the same bytes and tests compare with torch.equal.
//
// Structure:
//   * a workgroup of four waves owns a 16 x 64 pixel tile of one cell of one frame and strides over the tiles (no memset in front:
//     a zero cell, a None panel and a tile nothing reaches are stores of zero; every output byte has one writer, written once);
//   * lanes j < J round the frame's centres into LDS (an invalid joint is a sentinel);
//   * wave 0 takes the bones (lane = edge), wave 1 the joints (lane = joint): a primitive whose bounding box, grown by
//     ceil(L / 2) or the radius, meets the tile is kept; a ballot and a prefix popcount compact the kept ones in draw order;
//   * each lane then walks the two lists for four consecutive pixels of a row (LDS broadcasts: every lane reads the same entry), the
//     last covering primitive wins, and stores 12 bytes as three dwords (W % 4 == 0: a group of four never straddles the canvas edge,
//     and (row pitch, x) * 3 is a multiple of 12, so the dwords are aligned with the allocation).
// Most tiles of an 800 x 600 canvas meet no primitive: the kernel is write-bound (1.44 MB per panel frame).
// A bone's three cover tests all imply a distance of at most L / 2 from the segment, so the grown bounding box loses nothing.
// Ranges: |c| <= 16383 and 0 <= p < 8192 give |q| components below 2^15 and |d| components below 2^15; s and n stay below 2^31, the
// cross product is twice the area of a triangle inside the 32766-square, <= 2^30.1, so 4 (q x d)^2 < 2^63: int64 is exact.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/p2c.h"
#include "p2c_host.h"

namespace p2c_render {

constexpr int NTH = 256;
constexpr int TW = 64, TH = 16;               // tile: 16 lanes x 4 pixels wide, 16 rows
constexpr int MAXP = P2C_RENDER_MAX_PRIMS;
constexpr int kMaxBlocks = 2048;              // eight small workgroups per CU
constexpr int INVALID = INT32_MIN;
static_assert(MAXP <= 64, "one wave compacts a panel's bones, one its joints");
static_assert(TW / 4 * TH == NTH, "one lane per group of four pixels");

struct Dwords3 {
  uint32_t w[3];
};

__device__ __forceinline__ bool bone_covers(int px, int py, int ax, int ay, int bx, int by, long long L2) {
  const long long dx = bx - ax, dy = by - ay, qx = px - ax, qy = py - ay;
  const long long s = qx * dx + qy * dy, n = dx * dx + dy * dy;
  if (s <= 0) return 4 * (qx * qx + qy * qy) <= L2;
  if (s >= n) {
    const long long rx = px - bx, ry = py - by;
    return 4 * (rx * rx + ry * ry) <= L2;
  }
  const long long cr = qx * dy - qy * dx;
  return 4 * cr * cr <= L2 * n;
}

__global__ __launch_bounds__(NTH) void render_points_kernel(const p2c_render_points_desc d) {
  __shared__ int s_cx[MAXP], s_cy[MAXP];
  __shared__ int s_bone[MAXP][5];             // ax, ay, bx, by, rgb -- the bones that reach the tile, in edge order
  __shared__ int s_joint[MAXP][3];            // cx, cy, rgb -- the joints that reach the tile, in index order
  __shared__ int s_count[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int H = d.H, W = d.W, L = d.line_width, radius = d.radius;
  const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH, cells = d.rows * d.cols;
  const int64_t total = (int64_t)d.V * d.T * cells * tiles_y * tiles_x;
  const int64_t row_bytes = (int64_t)d.cols * W * 3;
  const int ly = tid >> 4, lx = (tid & 15) * 4;
  const long long L2 = (long long)L * L;
  const int r2 = radius * radius, grow = (L + 1) >> 1;

  for (int64_t tile = blockIdx.x; tile < total; tile += gridDim.x) {
    const int tx = (int)(tile % tiles_x);
    int64_t rest = tile / tiles_x;
    const int ty = (int)(rest % tiles_y);
    rest /= tiles_y;
    const int cell = (int)(rest % cells);
    const int64_t frame = rest / cells;
    const int x0 = tx * TW, y0 = ty * TH;
    const int x = x0 + lx, y = y0 + ly;
    const bool inside = x < W && y < H;
    uint32_t c[4] = {0u, 0u, 0u, 0u};

    if (cell < d.n_panels && d.panels[cell].points != nullptr) {      // the same answer on every lane of the workgroup
      const p2c_render_panel &P = d.panels[cell];
      const int J = P.J, E = L > 0 ? P.E : 0;
      if (tid < J) {
        const float *p = P.points + ((int64_t)frame * J + tid) * P.C;
        const float fx = rintf(p[0]), fy = rintf(p[1]);
        const bool ok = fabsf(fx) <= (float)P2C_RENDER_MAX_COORD && fabsf(fy) <= (float)P2C_RENDER_MAX_COORD;   // false for NaN / inf
        s_cx[tid] = ok ? (int)fx : INVALID;
        s_cy[tid] = ok ? (int)fy : 0;
      }
      __syncthreads();
      const int x1 = (x0 + TW < W ? x0 + TW : W) - 1, y1 = (y0 + TH < H ? y0 + TH : H) - 1;
      if (wave == 0) {
        bool reach = false;
        int ax = 0, ay = 0, bx = 0, by = 0, rgb = 0;
        if (lane < E) {
          const int a = P.edges[2 * lane], b = P.edges[2 * lane + 1];
          if ((unsigned)a < (unsigned)J && (unsigned)b < (unsigned)J) {
            ax = s_cx[a], ay = s_cy[a], bx = s_cx[b], by = s_cy[b];
            if (ax != INVALID && bx != INVALID) {
              const int lo_x = ax < bx ? ax : bx, hi_x = ax < bx ? bx : ax, lo_y = ay < by ? ay : by, hi_y = ay < by ? by : ay;
              reach = lo_x - grow <= x1 && hi_x + grow >= x0 && lo_y - grow <= y1 && hi_y + grow >= y0;
              const uint8_t *col = P.colors + 3 * b;
              rgb = col[0] | col[1] << 8 | col[2] << 16;
            }
          }
        }
        const unsigned long long kept = __ballot(reach);
        if (reach) {
          int *e = s_bone[__popcll(kept & ((1ull << lane) - 1))];
          e[0] = ax, e[1] = ay, e[2] = bx, e[3] = by, e[4] = rgb;
        }
        if (lane == 0) s_count[0] = __popcll(kept);
      } else if (wave == 1) {
        bool reach = false;
        int cx = 0, cy = 0;
        if (lane < J) {
          cx = s_cx[lane], cy = s_cy[lane];
          reach = cx != INVALID && cx - radius <= x1 && cx + radius >= x0 && cy - radius <= y1 && cy + radius >= y0;
        }
        const unsigned long long kept = __ballot(reach);
        if (reach) {
          const uint8_t *col = P.colors + 3 * lane;
          int *e = s_joint[__popcll(kept & ((1ull << lane) - 1))];
          e[0] = cx, e[1] = cy, e[2] = col[0] | col[1] << 8 | col[2] << 16;
        }
        if (lane == 0) s_count[1] = __popcll(kept);
      }
      __syncthreads();
      // (the next tile's centres are written behind this barrier by lanes that have read theirs, its lists and counts behind the
      // next tile's first barrier, which no lane passes before every lane has left the loops below)
      const int nb = s_count[0], nj = s_count[1];
      if (inside) {
        for (int i = 0; i < nb; ++i) {
          const int ax = s_bone[i][0], ay = s_bone[i][1], bx = s_bone[i][2], by = s_bone[i][3];
          const uint32_t rgb = (uint32_t)s_bone[i][4];
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (bone_covers(x + k, y, ax, ay, bx, by, L2)) c[k] = rgb;
        }
        for (int i = 0; i < nj; ++i) {
          const int ex = x - s_joint[i][0], ey = y - s_joint[i][1];
          const uint32_t rgb = (uint32_t)s_joint[i][2];
          const int ey2 = ey * ey;
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if ((ex + k) * (ex + k) + ey2 <= r2) c[k] = rgb;
        }
      }
    }
    if (inside) {
      const int crow = cell / d.cols, ccol = cell - crow * d.cols;
      uint8_t *dst = d.out + ((frame * d.rows + crow) * H + y) * row_bytes + ((int64_t)ccol * W + x) * 3;
      Dwords3 v;      // bytes r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
      v.w[0] = c[0] | c[1] << 24;
      v.w[1] = c[1] >> 8 | c[2] << 16;
      v.w[2] = c[2] >> 16 | c[3] << 8;
      *reinterpret_cast<Dwords3 *>(dst) = v;
    }
  }
}

static bool shapes_ok(const p2c_render_points_desc &d) {
  if (d.V < 1 || d.T < 1 || d.rows < 1 || d.cols < 1) return false;
  if (d.H < 1 || d.W < 1 || d.H > P2C_RENDER_MAX_SIDE || d.W > P2C_RENDER_MAX_SIDE || d.W % 4 != 0) return false;
  if (d.radius < 0 || d.radius > P2C_RENDER_MAX_REACH || d.line_width < 0 || d.line_width > P2C_RENDER_MAX_REACH) return false;
  if (d.n_panels < 0 || d.n_panels > P2C_RENDER_MAX_PANELS || d.n_panels > (int64_t)d.rows * d.cols) return false;
  if ((int64_t)d.rows * d.cols > (1 << 20)) return false;
  const int64_t frame_bytes = (int64_t)d.rows * d.cols * d.H * d.W * 3;                  // < 2^48
  if ((int64_t)d.V * d.T > ((int64_t)1 << 44) / frame_bytes) return false;               // the output's byte offsets stay far inside int64
  for (int k = 0; k < d.n_panels; ++k) {
    const p2c_render_panel &p = d.panels[k];
    if (!p.points) continue;
    if (p.J < 0 || p.J > P2C_RENDER_MAX_PRIMS || p.E < 0 || p.E > P2C_RENDER_MAX_PRIMS || p.C < 2) return false;
  }
  return true;
}

}  // namespace p2c_render

using namespace p2c_render;

extern "C" int p2c_render_points_supported(const p2c_render_points_desc *d) { return d && shapes_ok(*d) ? 1 : 0; }

extern "C" int p2c_render_points_fwd(const p2c_render_points_desc *d, void *stream) {
  if (!d) return P2C_E_NULL;
  if (!shapes_ok(*d) || d->max_blocks < 0) return P2C_E_SHAPE;
  if (!d->out) return P2C_E_NULL;
  for (int k = 0; k < d->n_panels; ++k) {
    const p2c_render_panel &p = d->panels[k];
    if (p.points && (!p.colors || (p.E > 0 && !p.edges))) return P2C_E_NULL;
  }
  const int64_t tiles_x = (d->W + TW - 1) / TW, tiles_y = (d->H + TH - 1) / TH;
  const int64_t total = (int64_t)d->V * d->T * d->rows * d->cols * tiles_y * tiles_x;
  const int cap = d->max_blocks > 0 && d->max_blocks < kMaxBlocks ? d->max_blocks : kMaxBlocks;
  const int grid = total < cap ? (int)total : cap;
  hipLaunchKernelGGL(render_points_kernel, dim3(grid), dim3(NTH), 0, (hipStream_t)stream, *d);
  return p2c_host::launch_status();
}
