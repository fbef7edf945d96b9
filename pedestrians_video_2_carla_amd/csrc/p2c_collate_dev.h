// p2c_collate_dev.h -- shared by p2c_collate.hip (K11, K26) and p2c_generate.hip (K38): what a lane group knows about the source of
// its frame (View) and the data-side normaliser of one frame (normalise). Both files run the same instructions on the same inputs,
// so the model input and the projection_2d_transformed target come out with the same bits whichever kernel formed them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "../../include/p2c.h"
#include "p2c_lane_dev.h"

namespace p2c_collate {

// What one lane group needs to know about the source of its frame. K11 fills it from Args (every field wave-uniform, so it
// stays in SGPRs); K26 fills it per lane group from the table of its clip's source.
struct View {
  const float *raw, *noise, *miss_u, *bboxes;   // nullptr = that step is off for this source
  int64_t rf;                                   // frame index in raw (K11: the batch frame)
  int32_t Jd, Jn, C, transform, n_hips, n_neck; // Jn: joints per frame of noise / miss_u
  int32_t hips_idx[2], neck_idx[2];
  float mp;                                     // this lane's miss_prob, flip source joint and node-map source joint
  int32_t perm_j, inv_j;
};

using p2c_lane::xor_max;
using p2c_lane::xor_min;
__device__ __forceinline__ float finite_or_zero(float v) { return isfinite(v) ? v : 0.f; }   // nan_to_zero

// Normalizer.__call__ (normalizer.py:20-41), dim = 2, for the frame of this lane group: (x, y[, conf]) -> normalised
// (x, y), conf through nan_to_zero; shift / scale of the frame. Same arithmetic as p2c_aux::normalize_kernel.
// The shuffles sit under conditions on the source's transform: uniform over a lane group, which is all they read.
template <int G>
__device__ __forceinline__ void normalise(const View &v, float near_zero, int base, bool active, float x, float y,
                                          float conf, float &ox, float &oy, float &oconf, float (&s)[2], float &scale) {
  const int tr = v.transform;
  float k[2] = {0.f, 0.f};
  s[0] = s[1] = 0.f;
  scale = 1.f;
  const float p[2] = {x, y};
  if (tr != P2C_TRANSFORM_BBOX) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      float h = __shfl(p[c], base + v.hips_idx[0], 64);
      if (v.n_hips == 2) h = 0.5f * (h + __shfl(p[c], base + v.hips_idx[1], 64));
      float q = __shfl(p[c], base + v.neck_idx[0], 64);
      if (v.n_neck == 2) q = 0.5f * (q + __shfl(p[c], base + v.neck_idx[1], 64));
      s[c] = h, k[c] = q;
    }
    scale = sqrtf(fmaf(k[1] - s[1], k[1] - s[1], (k[0] - s[0]) * (k[0] - s[0])));
  }
  bool use_bb = false;
  if (tr == P2C_TRANSFORM_HIPS_NECK_BBOX)
    use_bb = (s[0] < near_zero && s[1] < near_zero) || (k[0] < near_zero && k[1] < near_zero);
  if (__any(tr == P2C_TRANSFORM_BBOX || use_bb)) {
    const bool missing = !active || (x < near_zero && y < near_zero);
    const float inf = __builtin_inff();
    const float mn0 = xor_min<G>(missing ? inf : x), mn1 = xor_min<G>(missing ? inf : y);
    const float mx0 = xor_max<G>(missing ? -inf : x), mx1 = xor_max<G>(missing ? -inf : y);
    const float cu = 0.5f * (mn0 + mx0), cv = 0.5f * (mn1 + mx1);
    const float dx = cu - cu, dy = fminf(mn1, mx1) - cv;
    const float bb_scale = sqrtf(fmaf(dx, dx, dy * dy));
    if (tr == P2C_TRANSFORM_BBOX) s[0] = cu, s[1] = cv, scale = bb_scale;
    else if (use_bb) scale = bb_scale * 0.5748f;
  }
  ox = finite_or_zero((x - s[0]) / scale), oy = finite_or_zero((y - s[1]) / scale);
  oconf = finite_or_zero(conf);
  if (v.C > 2 && !(oconf >= near_zero)) ox = 0.f, oy = 0.f;     // normalizer.py:35-37
}

}  // namespace p2c_collate
