// p2c_lane_dev.h -- the xor-butterfly reductions over the lanes of a wave, shared by every kernel file.
//
// A group is G consecutive lanes of a 64-lane wave (G a power of two, aligned at a multiple of G). Lane i meets lane i ^ o for
// o = G/2, G/4, ..., 1 through __shfl_xor (ds_bpermute_b32), so after log2(G) rounds every lane of the group holds the
// reduction over the group, in one fixed order: bitwise the same in every lane and in every launch. G = 64 is the whole wave.
// T is float or double. The pose head's DPP / permlane forms (p2c_pose_head_dev.h) meet the same partners in the same order
// without the LDS crossbar; they stay where they are.
#pragma once
#include <hip/hip_runtime.h>

namespace p2c_lane {

template <int G, typename T>
__device__ __forceinline__ T xor_sum(T v) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
template <int G>
__device__ __forceinline__ float xor_min(float v) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}
template <int G>
__device__ __forceinline__ float xor_max(float v) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

}  // namespace p2c_lane
