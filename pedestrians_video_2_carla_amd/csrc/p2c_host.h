// p2c_host.h -- host-side helpers shared by the C-ABI entry points of every kernel file.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace p2c_host {

// What an entry point returns after its last launch: 0, or the HIP error the launch left behind (include/p2c.h: rc > 0).
inline int launch_status() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

// The grid of a kernel whose workgroups stride over `want` units of work: capped at `limit`, which max_blocks > 0 lowers.
inline unsigned grid_for(int64_t want, int32_t max_blocks, int limit) {
  const int cap = max_blocks > 0 && max_blocks < limit ? max_blocks : limit;
  return (unsigned)(want < cap ? want : cap);
}

// Every pointer is 16-byte aligned (float4 loads and stores). A null pointer passes: an optional tensor that is absent.
template <class... P>
inline bool aligned16(const P *...p) {
  return ((reinterpret_cast<uintptr_t>(p) | ... | uintptr_t(0)) & 15) == 0;
}

}  // namespace p2c_host

// K15's reduction of per-workgroup (d gamma | d beta) partial rows, used by K20b as well (p2c_norm.hip).
int p2c_internal_norm_blocks(int64_t rows, int32_t D);     // workgroups of a row pass: one partial row of 2 D floats each
int p2c_internal_norm_finish(const float *partials, int32_t n_blocks, int32_t D, float *g_gamma, float *g_beta, int32_t accumulate,
                             hipStream_t stream);          // adds the rows in a fixed order; returns launch_status()
