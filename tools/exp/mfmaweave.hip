// experiment: what does a dependent chain of v_mfma_f32_16x16x4_f32 cost per k-step when its operands come from LDS the way dgrad
// step 5 of the LinearAE reads them (A rows ld = 82 floats apart, B rows TP = 17 apart, four rows per k-step), with the operand
// reads of the next group standing as a BLOCK between two groups of four MFMAs (layer_dgrad before the weave) or WOVEN one
// position at a time into the gaps behind the MFMAs. One wave on the CU, two waves on one SIMD, eight waves (two per SIMD).
// build: hipcc -O3 --offload-arch=gfx950 -o mfmaweave mfmaweave.hip
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("hip error %d at %d\n", (int)e, __LINE__); return 1; } } while (0)
typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int KS = 40, ROUNDS = 32, LD = 82, TP = 17, MT = 5;        // layer 5: 78 inputs (five m-tiles), 156 outputs padded to 160
constexpr int A_FLOATS = 4 * KS * LD, B_FLOATS = 4 * KS * TP;
constexpr int LDS_BYTES = 100 * 1024;                                // more than half a CU's LDS: one workgroup per CU

// form 0: the block form (ping-pong over groups of four steps)
__device__ __forceinline__ f32x4 chain_block(const float *ap, const float *bp, f32x4 c) {
  float b0[4], a0[4], b1[4], a1[4];
  auto load = [&](float (&bv)[4], float (&av)[4], int s) {
#pragma unroll
    for (int u = 0; u < 4; ++u) bv[u] = bp[(s + u) * 4 * TP], av[u] = ap[(s + u) * 4 * LD];
  };
  auto fma4 = [&](const float (&bv)[4], const float (&av)[4]) {
#pragma unroll
    for (int u = 0; u < 4; ++u) c = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], bv[u], c, 0, 0, 0);
  };
  load(b0, a0, 0);
#pragma unroll
  for (int s = 4;; s += 8) {
    if (s < KS) load(b1, a1, s);
    __builtin_amdgcn_sched_barrier(0);
    fma4(b0, a0);
    __builtin_amdgcn_sched_barrier(0);
    if (s >= KS) break;
    if (s + 4 < KS) load(b0, a0, s + 4);
    __builtin_amdgcn_sched_barrier(0);
    fma4(b1, a1);
    __builtin_amdgcn_sched_barrier(0);
    if (s + 4 >= KS) break;
  }
  return c;
}
// woven: AHEAD steps in flight in front of the first MFMA; behind MFMA k the reads of step k + AHEAD. PAIR: the B reads of two steps
// stand together in every second gap (one ds_read2_b32), otherwise every gap has one A and one B read.
template <int AHEAD, bool PAIR>
__device__ __forceinline__ f32x4 chain_woven(const float *ap, const float *bp, f32x4 c) {
  float a[8], b[8];
#pragma unroll
  for (int k = 0; k < AHEAD; ++k) a[k] = ap[k * 4 * LD], b[k] = bp[k * 4 * TP];
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int k = 0; k < KS; ++k) {
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[k & 7], b[k & 7], c, 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
    const int n = k + AHEAD;
    if (n < KS) a[n & 7] = ap[n * 4 * LD];
    if constexpr (!PAIR) {
      if (n < KS) b[n & 7] = bp[n * 4 * TP];
    } else if constexpr (AHEAD == 4) {       // slots of steps n, n + 1 were used by MFMAs k - 4, k - 3
      if ((k & 1) == 0) {
        if (n < KS) b[n & 7] = bp[n * 4 * TP];
        if (n + 1 < KS) b[(n + 1) & 7] = bp[(n + 1) * 4 * TP];
      }
    } else {                                 // in-place refill: the slots of steps n - 1, n are free behind MFMA k only
      if ((k & 1) == 1) {
        if (n - 1 < KS) b[(n - 1) & 7] = bp[(n - 1) * 4 * TP];
        if (n < KS) b[n & 7] = bp[n * 4 * TP];
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  return c;
}

template <int FORM>
__global__ __launch_bounds__(512) void k(unsigned long long *cyc, unsigned *simd, float *out, unsigned mask) {
  extern __shared__ float lds[];
  for (int i = threadIdx.x; i < A_FLOATS + B_FLOATS; i += blockDim.x) lds[i] = (float)((i * 7 + 3) % 5 - 2);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  if (!((mask >> wave) & 1)) return;
  const float *ap = lds + g * LD + (wave % MT) * 16 + c, *bp = lds + A_FLOATS + g * TP + c;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const unsigned long long t0 = __builtin_readcyclecounter();
#pragma unroll 1
  for (int r = 0; r < ROUNDS; ++r) {
    asm volatile("" ::: "memory");           // a round reads its operands again, as a layer step does
    if constexpr (FORM == 0) acc = chain_block(ap, bp, acc);
    if constexpr (FORM == 1) acc = chain_woven<8, false>(ap, bp, acc);
    if constexpr (FORM == 2) acc = chain_woven<4, false>(ap, bp, acc);
    if constexpr (FORM == 3) acc = chain_woven<8, true>(ap, bp, acc);
    if constexpr (FORM == 4) acc = chain_woven<4, true>(ap, bp, acc);
  }
  const unsigned long long t1 = __builtin_readcyclecounter();
  if (acc[0] + acc[1] + acc[2] + acc[3] == 12345.678f) out[0] = acc[0];
  if (lane == 0) {
    cyc[blockIdx.x * 8 + wave] = t1 - t0;
    simd[blockIdx.x * 8 + wave] = (__builtin_amdgcn_s_getreg(4 | (4 << 6) | (1 << 11)));   // HW_ID bits 5:4 = SIMD
  }
}

int main() {
  constexpr int BLOCKS = 256;
  unsigned long long *cyc;
  unsigned *simd;
  float *out;
  CK(hipMalloc(&cyc, BLOCKS * 8 * 8));
  CK(hipMalloc(&simd, BLOCKS * 8 * 4));
  CK(hipMalloc(&out, 64));
  std::vector<unsigned long long> h(BLOCKS * 8);
  std::vector<unsigned> hs(BLOCKS * 8);
  const char *names[5] = {"block", "woven, 8 ahead, A + B per gap", "woven, 4 ahead, A + B per gap", "woven, 8 ahead, B paired",
                          "woven, 4 ahead, B paired"};
  struct Setup { const char *name; int threads; unsigned mask; } setups[3] = {
      {"1 wave on the CU", 64, 0x01}, {"2 waves on one SIMD", 512, 0x11}, {"8 waves (2 per SIMD)", 512, 0xff}};
  auto launch = [&](int form, const Setup &s) {
    void (*fn)(unsigned long long *, unsigned *, float *, unsigned) =
        form == 0 ? k<0> : form == 1 ? k<1> : form == 2 ? k<2> : form == 3 ? k<3> : k<4>;
    hipError_t e = hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fn, dim3(BLOCKS), dim3(s.threads), LDS_BYTES, 0, cyc, simd, out, s.mask);
    return hipDeviceSynchronize();
  };
  printf("cycles per k-step of a dependent chain of %d v_mfma_f32_16x16x4_f32, %d rounds, mean over the active waves of %d workgroups\n",
         KS, ROUNDS, BLOCKS);
  for (const Setup &s : setups) {
    for (int form = 0; form < 5; ++form) {
      for (int rep = 0; rep < 2; ++rep) CK(launch(form, s));
      CK(hipMemcpy(h.data(), cyc, BLOCKS * 8 * 8, hipMemcpyDeviceToHost));
      CK(hipMemcpy(hs.data(), simd, BLOCKS * 8 * 4, hipMemcpyDeviceToHost));
      double sum = 0, mx = 0;
      int n = 0;
      for (int b = 0; b < BLOCKS; ++b)
        for (int w = 0; w < 8; ++w)
          if ((s.mask >> w) & 1) {
            const double v = (double)h[b * 8 + w] / (ROUNDS * KS);
            sum += v, ++n;
            if (v > mx) mx = v;
          }
      printf("%-22s %-32s %6.1f (max %6.1f)  SIMDs of workgroup 0:", s.name, names[form], sum / n, mx);
      for (int w = 0; w < 8; ++w)
        if ((s.mask >> w) & 1) printf(" %u", hs[w]);
      printf("\n");
    }
  }
  return 0;
}
