// p2c_s2s_wide.h -- K7c for 64 < O <= 160 (absolute_loc: 78, pose_changes / relative_rot: 156). Included by p2c_s2s.hip inside
// namespace p2c_s2s: same Args, same cell functions, same buffer-resource rows, same three barriers per step.
//
// The 16-clip tiling of decoder_fwd_kernel / decoder_bwd_kernel with the output features spread over the waves in 16-feature
// blocks: wave w owns blocks w, w + 4, w + 8 (NB = 2 up to O = 80, 3 up to 160), i.e. features (w + 4 j) 16 + [0, 16).
//   forward   A fragments per lane: W_ih0 4 x KS0 (KS0 = ceil(O / 4) rounded to 20 or 40), W_ih1 64, W_fc 16 NB   (<= 272 at O = 160)
//   backward  W_ih0^T 64 NB in registers (<= 192); W_fc^T and W_ih1^T resident in LDS (see above the kernel)
// One wave per SIMD (__launch_bounds__(256)): the 512 registers of a lane hold them for all T steps.
// W_ih0 (4H x O) does not fit the staging image (256 x 161 floats = 165 KB): it is staged one GATE at a time -- rows
// [64 q, 64 q + 64) are one contiguous block of 64 O floats, at most 64 x 161 x 4 = 41 KB -- so the image is no larger than
// the one the O <= 64 kernels use. LDS: x^T / d out^T grow to 64 NB rows of 17 floats.
// Summation order: every product walks k ascending, 4 per MFMA, exactly as the O <= 64 kernels of this tiling do (one chain per
// gate in layer 0, two interleaved chains in the other products); it depends on neither B nor the grid.
// There is no 4-clip form for these widths: P2C_REC_TILE is not read for O > 64.

constexpr int OWIDE = 160;

// `rows` whole rows of `cols` floats, contiguous from src, -> LDS image [rows][cols + 1]. 16-byte loads over the flat block
// whatever cols is (a row may start inside a load); a block that does not start on 16 bytes or does not end on a multiple of
// four floats is copied float by float.
__device__ __forceinline__ void stage_flat(const float *src, int rows, int cols, float *img) {
  __syncthreads();                                   // previous users of the image region are done
  const int n = rows * cols;
  if ((n & 3) == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
    const f32x4 *s4 = reinterpret_cast<const f32x4 *>(src);
    constexpr int SB = 10;                           // 64 x 160 floats = 2 560 loads = 10 per thread: one round trip per gate
    const int n4 = n >> 2, nt = blockDim.x;
    for (int i0 = threadIdx.x; i0 < n4; i0 += nt * SB) {
      f32x4 v[SB];
#pragma unroll
      for (int r = 0; r < SB; ++r) v[r] = (i0 + r * nt < n4) ? s4[i0 + r * nt] : zero4();
#pragma unroll
      for (int r = 0; r < SB; ++r) {
        const int i = i0 + r * nt;
        if (i >= n4) continue;
        int rr = (i * 4) / cols, cc = i * 4 - rr * cols;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          img[rr * (cols + 1) + cc] = v[r][j];
          if (++cc == cols) cc = 0, ++rr;
        }
      }
    }
  } else {
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      const int r = i / cols, cc = i - r * cols;
      img[r * (cols + 1) + cc] = src[i];
    }
  }
  __syncthreads();
}

// ---- forward -----------------------------------------------------------------------------------------------------------
template <int KS0, int NB>
__global__ __launch_bounds__(256) void decoder_fwd_wide_kernel(const Args a) {
  DropRng rng = a.rng;
  const bool hashed = !a.drop && rng.state != nullptr;
  if (hashed) drop_begin(rng, false);
  extern __shared__ float img[];                    // staging image of one weight block at a time
  __shared__ float xT[NB * 64 * TP], h0T[H * TP], h1T[H * TP];
  const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = blockIdx.x * TS + c;
  const bool ok = b < a.B;
  const int u0 = w * 16 + 4 * g;                    // first of this lane's four hidden units; its features are u0 + 64 j + r
  const int O = a.O, B = a.B, T = a.T;
  const int off4 = (b * G4 + u0) * 4, off1 = (b * H + u0) * 4;

  float fa0[4][KS0], fa1[4][H / 4], ffc[NB][H / 4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {                     // W_ih0, one gate (64 contiguous rows) per image
    stage_flat(a.w_ih0 + (size_t)q * H * O, H, O, img);
#pragma unroll
    for (int ks = 0; ks < KS0; ++ks) {
      const int k = 4 * ks + g;
      fa0[q][ks] = (k < O) ? img[(w * 16 + c) * (O + 1) + k] : 0.f;
    }
  }
  stage(a.w_ih1, G4, H, img);
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int ks = 0; ks < H / 4; ++ks) fa1[q][ks] = img[(q * H + w * 16 + c) * (H + 1) + 4 * ks + g];
  stage(a.w_fc, O, H, img);
#pragma unroll
  for (int j = 0; j < NB; ++j)
#pragma unroll
    for (int ks = 0; ks < H / 4; ++ks) {
      const int f = (w + 4 * j) * 16 + c;
      ffc[j][ks] = (f < O) ? img[f * (H + 1) + 4 * ks + g] : 0.f;
    }

  f32x4 k0r[4], k1r[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    k0r[q] = load4(a.k0 + (size_t)b * G4 + q * H + u0, ok);
    k1r[q] = load4(a.k1 + (size_t)b * G4 + q * H + u0, ok);
  }
  const f32x4 c0r = load4(a.c0 + (size_t)b * H + u0, ok), c1r = load4(a.c1 + (size_t)b * H + u0, ok);
  f32x4 bfc[NB];
  int offo[NB][4], offb[NB][4];                      // byte offsets of this lane's output features (OOB beyond O)
#pragma unroll
  for (int j = 0; j < NB; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int f = u0 + 64 * j + r;
      bfc[j][r] = (f < O) ? a.b_fc[f] : 0.f;
      offo[j][r] = (f < O) ? (b * O + f) * 4 : OOB;
      offb[j][r] = (f < O) ? (b * T * O + f) * 4 : OOB;
      // x_0 (rows >= O stay zero: they only ever meet zero weight fragments)
      xT[f * TP + c] = (a.x0 && ok && f < O) ? a.x0[(size_t)b * O + f] : 0.f;
    }
  if (hashed) drop_keys(rng, false);
  // the step's dropout mask, requested / drawn one step ahead (see decoder_fwd_kernel)
  auto mask_of = [&](const int t) -> f32x4 { return bload4(step_rows(a.drop, t, B, H), off1); };
  auto hash_of = [&](const int t) -> f32x4 {
    f32x4 m = {1.f, 1.f, 1.f, 1.f};
    if (hashed) m = drop_value4(rng, (uint32_t)((t * B + b) * H + u0));
    return m;
  };
  f32x4 maskh = hash_of(0);
  f32x4 mask = mask_of(0);
  __syncthreads();
  pin(mask);
  const bool has_drop = a.drop != nullptr || hashed;

  for (int t = 0; t < T; ++t) {
    f32x4 acc[4], ai, af, ag, ao, h;
    const f32x4 m = hashed ? maskh : mask;
    mask = mask_of((t + 1 < T) ? t + 1 : t), maskh = hash_of((t + 1 < T) ? t + 1 : t);
    // teacher forcing: flag and target features of this step, requested now, used behind the fc product (NULL: zeros)
    const float forced = bload1(step_rows(a.force, t, B, 1), b * 4);
    f32x4 tgt[NB];
    {
      const __amdgpu_buffer_rsrc_t rtg = step_rows(a.target, t, B, O);
#pragma unroll
      for (int j = 0; j < NB; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) tgt[j][r] = bload1(rtg, offo[j][r]);
    }
    // ---- layer 0
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = k0r[q];
#pragma unroll
    for (int ks = 0; ks < KS0; ++ks) {
      const float bv = xT[(4 * ks + g) * TP + c];
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa0[q][ks], bv, acc[q], 0, 0, 0);
    }
    cell_fwd(acc, c0r, ai, af, ag, ao, h);
    if (has_drop) h *= m;
#pragma unroll
    for (int r = 0; r < 4; ++r) h0T[(u0 + r) * TP + c] = h[r];
    pin(mask);                                       // before the stores: the wait covers the one load only
    store_gates(step_rows(a.acts0, t, B, G4), off4, ai, af, ag, ao);
    bstore4(step_rows(a.h0d, t, B, H), off1, h);
    lds_barrier();
    // ---- layer 1
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = k1r[q];
#pragma unroll
    for (int ks = 0; ks < H / 4; ++ks) {
      const float bv = h0T[(4 * ks + g) * TP + c];
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa1[q][ks], bv, acc[q], 0, 0, 0);
    }
    cell_fwd(acc, c1r, ai, af, ag, ao, h);
#pragma unroll
    for (int r = 0; r < 4; ++r) h1T[(u0 + r) * TP + c] = h[r];
    store_gates(step_rows(a.acts1, t, B, G4), off4, ai, af, ag, ao);
    bstore4(step_rows(a.h1, t, B, H), off1, h);
    lds_barrier();
    // ---- fc: this wave's NB blocks of 16 output features (two accumulators per block, as in the O <= 64 kernel)
    f32x4 o[NB], o2[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) o[j] = bfc[j], o2[j] = zero4();
#pragma unroll
    for (int ks = 0; ks < H / 4; ks += 2) {
      const float b0 = h1T[(4 * ks + g) * TP + c], b1 = h1T[(4 * ks + 4 + g) * TP + c];
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        o[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(ffc[j][ks], b0, o[j], 0, 0, 0);
        o2[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(ffc[j][ks + 1], b1, o2[j], 0, 0, 0);
      }
    }
    const __amdgpu_buffer_rsrc_t ro = step_rows(a.out, t, B, O), rb = bt_rows(a.out_bt, t, B, T, O);
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      o[j] += o2[j];
      if (forced != 0.f) o[j] = tgt[j];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        xT[(u0 + 64 * j + r) * TP + c] = o[j][r];    // next step's input (features >= O are exactly zero)
        bstore1(ro, offo[j][r], o[j][r]);
        bstore1(rb, offb[j][r], o[j][r]);
      }
    }
    lds_barrier();
  }
}

// ---- backward ----------------------------------------------------------------------------------------------------------
// Only W_ih0^T (64 NB fragments) lives in registers here. With W_fc^T (KS0) and W_ih1^T (64) beside it and the rows prefetched one
// step ahead the allocator spilled at NB = 3 (164 bytes per lane; 124 with W_fc^T alone moved out), so those two stay in LDS for all
// T steps and are read as the A operands of their products: [unit][k] with pitches FP = 164 and GPW = 260 (= 4 mod 64 banks: the
// 16 units x 4 k of one operand read fall into 64 different banks). The staging image of the prologue (one gate of W_ih0) lies over
// d out^T | d gates1^T | d gates0^T, which the loop writes only after it. One dynamic LDS block: 153 KB at NB = 3, 149 KB at NB = 2.
constexpr int FP = OWIDE + 4, GPW = G4 + 4;
template <int NB> constexpr int bwd_wide_floats() { return (NB * 64 + 2 * G4) * TP + H * FP + H * GPW; }
template <int KS0, int NB>
__global__ __launch_bounds__(256) void decoder_bwd_wide_kernel(const Args a) {
  static_assert((NB * 64 + 2 * G4) * TP >= H * (4 * KS0 + 1), "the staging image of one W_ih0 gate lies over the step buffers");
  DropRng rng = a.rng;
  const bool hashed = !a.drop && rng.state != nullptr;
  if (hashed) drop_begin(rng, true);
  extern __shared__ float img[];                     // staging image during the prologue, then:
  float *const doT = img, *const dg1T = doT + NB * 64 * TP, *const dg0T = dg1T + G4 * TP;
  float *const wfcT = dg0T + G4 * TP, *const w1T = wfcT + H * FP;      // W_fc^T [unit][o], W_ih1^T [unit][gate row]
  const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = blockIdx.x * TS + c;
  const bool ok = b < a.B;
  const int u0 = w * 16 + 4 * g;
  const int O = a.O, B = a.B, T = a.T;
  const int off4 = (b * G4 + u0) * 4, off1 = (b * H + u0) * 4;

  // dh1 = W_fc^T dout:  A[unit][k = o] = W_fc[o][unit]; columns O .. 4 KS0 - 1 are zero (they meet the zero rows of d out^T)
  // (256 threads, constant trip counts, unrolled: the loads of ten / sixteen rows are in flight together)
#pragma unroll 10
  for (int i = threadIdx.x; i < 4 * KS0 * H; i += 256) {
    const int k = i >> 6, u = i & 63;
    wfcT[u * FP + k] = (k < O) ? a.w_fc[i] : 0.f;
  }
  // dh0 = W_ih1^T dgates1:  A[unit][k = gate row] = W_ih1[k][unit]
#pragma unroll 16
  for (int i = threadIdx.x; i < G4 * H; i += 256) {
    const int k = i >> 6, u = i & 63;
    w1T[u * GPW + k] = a.w_ih1[i];
  }
  const float *const wfc_row = wfcT + (w * 16 + c) * FP + g, *const w1_row = w1T + (w * 16 + c) * GPW + g;
  // dx = W_ih0^T dgates0:  A[o][k = gate row] = W_ih0[k][o]: rows = a block of 16 output features, one gate per image
  float f0T[NB][G4 / 4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    stage_flat(a.w_ih0 + (size_t)q * H * O, H, O, img);
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int kk = 0; kk < H / 4; ++kk) {
        const int f = (w + 4 * j) * 16 + c;
        f0T[j][q * (H / 4) + kk] = (f < O) ? img[(4 * kk + g) * (O + 1) + f] : 0.f;
      }
  }
  __syncthreads();                                   // the image is read: the loop may write the step buffers that lie under it

  const f32x4 c0r = load4(a.c0 + (size_t)b * H + u0, ok), c1r = load4(a.c1 + (size_t)b * H + u0, ok);
  f32x4 dc0 = zero4(), dc1 = zero4(), dx[NB];
  int offo[NB][4], offi[NB][4];                      // d out_total rows (T,B,O); g_out rows in the layout the caller has
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    dx[j] = zero4();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int f = u0 + 64 * j + r;
      offo[j][r] = (f < O) ? (b * O + f) * 4 : OOB;
      offi[j][r] = (f < O) ? ((a.g_out_bt ? b * T * O : b * O) + f) * 4 : OOB;
    }
  }
  if (hashed) drop_keys(rng, true);
  const bool has_drop = a.drop != nullptr || hashed;

  // the rows a step reads are requested at the top of the previous step and pinned at its end (see decoder_bwd_kernel)
  struct Saved { f32x4 go[NB], a1[4], a0[4], m; float forced; };
  auto fetch = [&](int t, Saved &s) {
    s.forced = bload1(step_rows(a.force, t, B, 1), b * 4);
    const __amdgpu_buffer_rsrc_t rg = a.g_out_bt ? bt_rows(a.g_out, t, B, T, O) : step_rows(a.g_out, t, B, O);
    const __amdgpu_buffer_rsrc_t r1 = step_rows(a.acts1, t, B, G4), r0 = step_rows(a.acts0, t, B, G4);
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) s.go[j][r] = bload1(rg, offi[j][r]);
#pragma unroll
    for (int q = 0; q < 4; ++q) s.a1[q] = bload4(r1, off4 + q * H * 4), s.a0[q] = bload4(r0, off4 + q * H * 4);
    s.m = bload4(step_rows(a.drop, t, B, H), off1);
  };
  auto pin_all = [&](Saved &s) {
    pin(s.m);
    asm volatile("" : "+v"(s.forced));
#pragma unroll
    for (int j = 0; j < NB; ++j) pin(s.go[j]);
#pragma unroll
    for (int q = 0; q < 4; ++q) pin(s.a1[q]), pin(s.a0[q]);
  };
  Saved nx = {};
  if (T > 0) fetch(T - 1, nx);
  pin_all(nx);

  for (int t = T - 1; t >= 0; --t) {
    const Saved sv = nx;
    fetch(t > 0 ? t - 1 : 0, nx);                    // (the last step re-reads its own rows: no branch in the body)
    // ---- d out_t (loss + the next step's input gradient), this wave's NB blocks of 16 output features
    const __amdgpu_buffer_rsrc_t rt = step_rows(a.g_outtot, t, B, O);
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      f32x4 dout = dx[j] + sv.go[j];                 // (features >= O: zero fragments gave dx = 0, the OOB load gave 0)
      if (sv.forced != 0.f) dout = zero4();          // a forced frame is the target: no gradient reaches the decoder through it
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        doT[(u0 + 64 * j + r) * TP + c] = dout[r];
        bstore1(rt, offo[j][r], dout[r]);
      }
    }
    lds_barrier();
    // ---- fc backward: dh1 for this wave's 16 hidden units
    f32x4 dh = zero4();
#pragma unroll
    for (int ks = 0; ks < KS0; ++ks) dh = __builtin_amdgcn_mfma_f32_16x16x4f32(wfc_row[4 * ks], doT[(4 * ks + g) * TP + c], dh, 0, 0, 0);
    f32x4 pi, pf, pg, po;
    cell_bwd(dh, sv.a1[0], sv.a1[1], sv.a1[2], sv.a1[3], c1r, pi, pf, pg, po, dc1);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      dg1T[(u0 + r) * TP + c] = pi[r], dg1T[(H + u0 + r) * TP + c] = pf[r];
      dg1T[(2 * H + u0 + r) * TP + c] = pg[r], dg1T[(3 * H + u0 + r) * TP + c] = po[r];
    }
    store_gates(step_rows(a.g_gates1, t, B, G4), off4, pi, pf, pg, po);
    lds_barrier();
    // ---- layer-1 input gradient: dh0 (two accumulators halve the dependent chain)
    f32x4 e0 = zero4(), e1 = zero4();
#pragma unroll
    for (int ks = 0; ks < G4 / 4; ks += 2) {
      e0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w1_row[4 * ks], dg1T[(4 * ks + g) * TP + c], e0, 0, 0, 0);
      e1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w1_row[4 * ks + 4], dg1T[(4 * ks + 4 + g) * TP + c], e1, 0, 0, 0);
    }
    dh = e0 + e1;
    // (the hashed mask is drawn here, not a step ahead: ~50 integer instructions beside 300 MFMAs, and four registers less to carry)
    if (has_drop) dh *= hashed ? drop_value4(rng, (uint32_t)((t * B + b) * H + u0)) : sv.m;
    cell_bwd(dh, sv.a0[0], sv.a0[1], sv.a0[2], sv.a0[3], c0r, pi, pf, pg, po, dc0);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      dg0T[(u0 + r) * TP + c] = pi[r], dg0T[(H + u0 + r) * TP + c] = pf[r];
      dg0T[(2 * H + u0 + r) * TP + c] = pg[r], dg0T[(3 * H + u0 + r) * TP + c] = po[r];
    }
    store_gates(step_rows(a.g_gates0, t, B, G4), off4, pi, pf, pg, po);
    lds_barrier();
    // ---- layer-0 input gradient = gradient of the previous step's output, NB blocks against one pass over d gates0
    f32x4 x0a[NB], x1a[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) x0a[j] = zero4(), x1a[j] = zero4();
#pragma unroll
    for (int ks = 0; ks < G4 / 4; ks += 2) {
      const float b0 = dg0T[(4 * ks + g) * TP + c], b1 = dg0T[(4 * ks + 4 + g) * TP + c];
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        x0a[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(f0T[j][ks], b0, x0a[j], 0, 0, 0);
        x1a[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(f0T[j][ks + 1], b1, x1a[j], 0, 0, 0);
      }
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) dx[j] = x0a[j] + x1a[j];
    pin_all(nx);
  }
  if (ok) {
    *reinterpret_cast<f32x4 *>(a.g_c0 + (size_t)b * H + u0) = dc0;
    *reinterpret_cast<f32x4 *>(a.g_c1 + (size_t)b * H + u0) = dc1;
  }
}
