// mfma_mlp.h -- building blocks of the fused tiny-MLP kernels on the gfx950 matrix cores: the NeuS SDF + radiance field
// (field.hip), the NeRF++ distant model and the close-range NGP model (nerf_field.hip), the sky MLP (sky.hip).
//
// Activation-register convention (one wave = 32 points): lane (j = l&31, hi = l>>5) owns point j and the units
// U(m,r,hi) = 32m + (r&3) + 8(r>>2) + 4hi of every M-tile m -- the C/D fragment of v_mfma_f32_32x32x*.  Layers are
// computed transposed (Out^T = W . In^T, weights = A operand), so a lane's accumulator registers are its B fragment for
// the next layer.  Weight gradients contract over points and go through an LDS transpose ([unit][point]).
//
// Weight-pack format: every decoder hands its matrices to contract / contract16 as pre-packed A fragments and its biases
// as per-lane vectors.  That format is stated HERE and nowhere else: the readers are contract / contract16, the writers
// the frag*_ coordinate functions right below each of them (their inverses), vec_unit, and pack_matrices, the one walk
// over a pack's matrices.  A decoder's pack kernel supplies its list of matrices (PackShape), where they go (its
// *Layout) and where an element comes from (its source function); tests/golden/wpack_sha256.json pins the bytes.
#pragma once
#include "nsim_common.h"

__host__ __device__ __forceinline__ int unit_of(int m, int r, int hi) { return 32 * m + (r & 3) + 8 * (r >> 2) + 4 * hi; }

// ------------------------------------------------------------------------------------- MFMA helpers
// (wave_sync_lds: nsim_prims.h)

__device__ __forceinline__ f32x16 zero16() {
  f32x16 z;
#pragma unroll
  for (int r = 0; r < 16; ++r) z[r] = 0.f;
  return z;
}

// exact power-of-two scale bringing the wave-wide max |v| to ~16 (1 when PREC==1 or all-zero)
template <int PREC, int N>
__device__ __forceinline__ float dyn_scale(const float (&v)[N]) {
  if constexpr (PREC == 1) {
    return 1.0f;
  } else {
    float m = 0.f;
#pragma unroll
    for (int i = 0; i < N; ++i) m = fmaxf(m, fabsf(v[i]));
    m = wave_max(m);
    if (!(m > 0.f) || !(m < 3.0e38f)) return 1.0f;
    uint32_t bits;
    memcpy(&bits, &m, 4);
    const int ex = (int)((bits >> 23) & 0xffu) - 126;  // m = f * 2^ex, f in [0.5,1)
    int k = 4 - ex;
    k = k > 60 ? 60 : (k < -60 ? -60 : k);
    const uint32_t sb = (uint32_t)(127 + k) << 23;
    float sc;
    memcpy(&sc, &sb, 4);
    return sc;
  }
}

// acc[mo] += W[32mo.., :] . In^T   with In given in activation-register order (NI M-tiles of 16 regs),
// multiplied by in_scale before the f16 conversion.  Caller multiplies the result by 1/in_scale.
template <int PREC, int MO, int NI>
__device__ __forceinline__ void contract(f32x16 (&acc)[MO], const char* wmat, const float (&in)[NI * 16],
                                         float in_scale) {
  const int lane = nsim_lane();
  if constexpr (PREC == 0) {
    const f16x8* A = reinterpret_cast<const f16x8*>(wmat);
#pragma unroll
    for (int s = 0; s < 2 * NI; ++s) {
      f16x8 b;
#pragma unroll
      for (int e = 0; e < 8; ++e) b[e] = (f16)(in[(s >> 1) * 16 + 8 * (s & 1) + e] * in_scale);
#pragma unroll
      for (int mo = 0; mo < MO; ++mo) acc[mo] = mfma_32x32x16_f16(A[(mo * 2 * NI + s) * 64 + lane], b, acc[mo]);
    }
  } else {
    const float* A = reinterpret_cast<const float*>(wmat);
#pragma unroll
    for (int mi = 0; mi < NI; ++mi) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float b = in[mi * 16 + r];
#pragma unroll
        for (int mo = 0; mo < MO; ++mo)
          acc[mo] = mfma_32x32x2_f32(A[((mo * NI + mi) * 16 + r) * 64 + lane], b, acc[mo]);
      }
    }
  }
}

// The inverses of the A-fragment indexing of contract just above: element k of a packed [Uo x Ui] matrix -> (row, col).
// f16 (also each half of the split form): k = ((mo * (Ui / 16) + s) * 64 + lane) * 8 + e
struct FragRC {
  int row, col;
};
__host__ __device__ inline FragRC frag32_f16(int64_t k, int Ui) {
  const int e = (int)(k & 7), lane = (int)((k >> 3) & 63), fs = (int)(k >> 9), nS = Ui / 16;
  return FragRC{32 * (fs / nS) + (lane & 31), 16 * (fs % nS) + mfma_row(e, lane >> 5)};
}
// f32: k = ((mo * (Ui / 32) + mi) * 16 + r) * 64 + lane.  This one and vec_unit go through unit_of, with an M-tile that is
// not bounded at compile time, on purpose: the device link step derives value ranges for unit_of's arguments from ALL its
// callers in a source file, and without such a caller the sin / cos kernels of sky.hip and field.hip (k_sky_fwd, k_field,
// k_field_bwd_j) compile differently.  The pack tests cannot catch that -- the packed bytes stay the same; only a
// comparison of those kernels' assembly shows it.
__host__ __device__ inline FragRC frag32_f32(int64_t k, int Ui) {
  const int lane = (int)(k & 63), fr = (int)(k >> 6), fm = fr >> 4, nMi = Ui / 32;
  return FragRC{32 * (fm / nMi) + (lane & 31), unit_of(fm % nMi, fr & 15, lane >> 5)};
}
// slot k of an n-long per-lane vector (order [hi][m * 16 + r]: lane-half hi reads its n / 2 floats contiguously) -> unit
__host__ __device__ inline int vec_unit(int k, int n) {
  const int hi = k / (n / 2), q = k % (n / 2);
  return unit_of(q >> 4, q & 15, hi);
}

// out[m*16+r] = (W . In^T)[unit(m,r,hi)][pt]
template <int PREC, int MO, int NI>
__device__ __forceinline__ void dense(float (&out)[MO * 16], const char* wmat, const float (&in)[NI * 16],
                                      bool dynamic) {
  f32x16 acc[MO];
#pragma unroll
  for (int mo = 0; mo < MO; ++mo) acc[mo] = zero16();
  const float sc = dynamic ? dyn_scale<PREC, NI * 16>(in) : 1.0f;
  contract<PREC, MO, NI>(acc, wmat, in, sc);
  const float inv = 1.0f / sc;
#pragma unroll
  for (int mo = 0; mo < MO; ++mo)
#pragma unroll
    for (int r = 0; r < 16; ++r) out[mo * 16 + r] = acc[mo][r] * inv;
}

// ---- LDS staging [unit][point] for the weight-gradient contractions (contract over the tile's 32 points)
template <int PREC>
struct StageT {
  typedef f16 T;
  static constexpr int PITCH = 40;
};
template <>
struct StageT<1> {
  typedef float T;
  static constexpr int PITCH = 33;
};

// bytes of the two per-wave staging arrays (A side + B side, 64 rows each)
template <int PREC>
__host__ __device__ constexpr int stage_bytes_per_wave() {
  return 2 * 64 * StageT<PREC>::PITCH * (int)sizeof(typename StageT<PREC>::T);
}

template <int PREC, int NM>
__device__ __forceinline__ void stage(void* st, const float (&v)[NM * 16], float scale) {
  typedef typename StageT<PREC>::T T;
  T* p = reinterpret_cast<T*>(st);
  const int lane = nsim_lane(), j = lane & 31, hi = lane >> 5;
#pragma unroll
  for (int m = 0; m < NM; ++m)
#pragma unroll
    for (int r = 0; r < 16; ++r) p[unit_of(m, r, hi) * StageT<PREC>::PITCH + j] = (T)(v[m * 16 + r] * scale);
}

// C[32mo + row][32no + col] = sum_pt A[32mo+row][pt] * B[32no+col][pt]
template <int PREC>
__device__ __forceinline__ f32x16 dw_tile(const void* stA, int mo, const void* stB, int no) {
  typedef typename StageT<PREC>::T T;
  constexpr int P = StageT<PREC>::PITCH;
  const T* a = reinterpret_cast<const T*>(stA);
  const T* b = reinterpret_cast<const T*>(stB);
  const int lane = nsim_lane(), i = lane & 31, hi = lane >> 5;
  f32x16 acc = zero16();
  if constexpr (PREC == 0) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const f16x8 av = *reinterpret_cast<const f16x8*>(a + (32 * mo + i) * P + 16 * s + 8 * hi);
      const f16x8 bv = *reinterpret_cast<const f16x8*>(b + (32 * no + i) * P + 16 * s + 8 * hi);
      acc = mfma_32x32x16_f16(av, bv, acc);
    }
  } else {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const float av = a[(32 * mo + i) * P + 2 * q + hi];
      const float bv = b[(32 * no + i) * P + 2 * q + hi];
      acc = mfma_32x32x2_f32(av, bv, acc);
    }
  }
  return acc;
}

// accumulate a dW tile into an LDS accumulator: dst[(32mo+row)*ld + 32no + col].
// PRIV = the accumulator belongs to THIS wave alone -> plain read-add-write.  Measured on MI355X: ds_add_f32 costs
// ~800 cycles per wave instruction (the 192 LDS float atomics per 32-point tile were 80 % of the SDF-branch backward),
// a ds_read / v_add / ds_write triple a few tens.  PRIV = false keeps the shared accumulator + atomics (f32 test mode).
template <bool PRIV = false>
__device__ __forceinline__ void dw_flush(float* dst, int ld, int rows, int cols, int mo, int no, const f32x16& acc,
                                         float unscale) {
  const int lane = nsim_lane(), col = 32 * no + (lane & 31), hi = lane >> 5;
  if (col >= cols) return;
  if constexpr (PRIV) {
    float cur[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = 32 * mo + mfma_row(r, hi);
      cur[r] = row < rows ? dst[row * ld + col] : 0.f;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = 32 * mo + mfma_row(r, hi);
      if (row < rows) dst[row * ld + col] = cur[r] + acc[r] * unscale;
    }
  } else {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = 32 * mo + mfma_row(r, hi);
      if (row < rows) atomicAdd(&dst[row * ld + col], acc[r] * unscale);
    }
  }
}

// dW[rows x cols] += A (NMA m-tiles) (x) B (NMB m-tiles) over the tile's points; db[rows] += rowsum(A)
template <int PREC, int NMA, int NMB, bool PRIV = false>
__device__ __forceinline__ void dw_product(void* stA, void* stB, const float (&A)[NMA * 16], const float (&B)[NMB * 16],
                                           float* dW, int ld, int rows, int cols, float* db) {
  const float sa = dyn_scale<PREC, NMA * 16>(A), sb = dyn_scale<PREC, NMB * 16>(B);
  wave_sync_lds();
  stage<PREC, NMA>(stA, A, sa);
  stage<PREC, NMB>(stB, B, sb);
  wave_sync_lds();
  const float un = 1.0f / (sa * sb);
#pragma unroll
  for (int mo = 0; mo < NMA; ++mo)
#pragma unroll
    for (int no = 0; no < NMB; ++no) {
      const f32x16 acc = dw_tile<PREC>(stA, mo, stB, no);
      dw_flush<PRIV>(dW, ld, rows, cols, mo, no, acc, un);
    }
  if (db) {
    typedef typename StageT<PREC>::T T;
    const T* a = reinterpret_cast<const T*>(stA);
    const int lane = nsim_lane();
    if (lane < NMA * 32 && lane < rows) {
      float s = 0.f;
      for (int j = 0; j < 32; ++j) s += (float)a[lane * StageT<PREC>::PITCH + j];
      if constexpr (PRIV) db[lane] = db[lane] + s / sa;
      else atomicAdd(&db[lane], s / sa);
    }
  }
}

// row sums of an activation (for vector-shaped gradients such as the SDF head weights)
template <int PREC, int NM, bool PRIV = false>
__device__ __forceinline__ void rowsum_acc(void* stA, const float (&A)[NM * 16], float* dst, int rows) {
  const float sa = dyn_scale<PREC, NM * 16>(A);
  wave_sync_lds();
  stage<PREC, NM>(stA, A, sa);
  wave_sync_lds();
  typedef typename StageT<PREC>::T T;
  const T* a = reinterpret_cast<const T*>(stA);
  const int lane = nsim_lane();
  if (lane < NM * 32 && lane < rows) {
    float s = 0.f;
    for (int j = 0; j < 32; ++j) s += (float)a[lane * StageT<PREC>::PITCH + j];
    if constexpr (PRIV) dst[lane] = dst[lane] + s / sa;
    else atomicAdd(&dst[lane], s / sa);
  }
}


// ===================================================================== workgroup-joint weight-gradient products
// The weight gradients contract over POINTS.  Instead of one 32-point product per wave and tile (with its accumulator
// read-add-written in LDS after every tile: 16 ds_read + 16 ds_write per lane and output tile, four private 25 KB
// accumulator copies -> one workgroup per CU), the NW waves of a workgroup stage their activations side by side
// ([unit][32 NW points]) and every wave owns a FIXED subset of the output tiles, which it keeps in MFMA accumulator
// registers for the whole launch: no read-modify-write at all, no accumulators in LDS, one flush per wave at the end.
// fp16 mode stages bf16 (v_mfma_f32_32x32x16_bf16, same rate as f16 on gfx950): the f32 exponent range makes the
// per-tile power-of-two re-scaling of the f16 operands unnecessary, which is what allows the accumulation to run
// ACROSS tiles; the operands keep 8 significant bits, the sum is f32.  f32 mode stages f32 (exact, validation).
#ifndef NSIM_STAGE_PAIRS
#define NSIM_STAGE_PAIRS 1      // jstage, bf16: v_cvt_pk_bf16_f32 converts two staged values per instruction
#endif
#define JOINT_WAVES 4
#define JOINT_PTS (32 * JOINT_WAVES)

template <int PREC>
struct JStageT {
  typedef bf16 T;
  static constexpr int PITCH = JOINT_PTS + 8;     // 272 B rows: 16-byte aligned, conflict-free ds_read_b128
};
template <>
struct JStageT<1> {
  typedef float T;
  static constexpr int PITCH = JOINT_PTS + 1;
};

template <int PREC>
__host__ __device__ constexpr int jstage_row_bytes() {
  return JStageT<PREC>::PITCH * (int)sizeof(typename JStageT<PREC>::T);
}

// write this wave's 32 points of an activation (NM m-tiles in activation-register order) into rows [0, 32 NM) of ``st``
// PAIRS (bf16): two values per conversion instruction (nsim_cvt2_bf16; MI355X: nsim_field_bwd_sdf 0.1216 -> 0.1135 ms on the bench
// step -- but the 17..32-level one-hidden-layer backward of the street step got 5 % slower, its register allocation moved 78 more
// values through AGPRs: that instantiation passes PAIRS = false)
template <int PREC, int NM, bool PAIRS = true>
__device__ __forceinline__ void jstage(void* st, const float (&v)[NM * 16], int wave) {
  typedef typename JStageT<PREC>::T T;
  T* p = reinterpret_cast<T*>(st);
  const int lane = nsim_lane(), j = lane & 31, hi = lane >> 5;
  if constexpr (PREC == 0 && NSIM_STAGE_PAIRS && PAIRS) {
#pragma unroll
    for (int m = 0; m < NM; ++m)
#pragma unroll
      for (int r = 0; r < 16; r += 2) {
        bf16 lo, hi16;
        nsim_cvt2_bf16(v[m * 16 + r], v[m * 16 + r + 1], lo, hi16);
        p[unit_of(m, r, hi) * JStageT<PREC>::PITCH + 32 * wave + j] = lo;
        p[unit_of(m, r + 1, hi) * JStageT<PREC>::PITCH + 32 * wave + j] = hi16;
      }
    return;
  }
#pragma unroll
  for (int m = 0; m < NM; ++m)
#pragma unroll
    for (int r = 0; r < 16; ++r) p[unit_of(m, r, hi) * JStageT<PREC>::PITCH + 32 * wave + j] = (T)v[m * 16 + r];
}

// the same for v * scale (a chain carried in scaled form is un-scaled where it is staged: no second copy of it in registers)
template <int PREC, int NM>
__device__ __forceinline__ void jstage_scaled(void* st, const float (&v)[NM * 16], float scale, int wave) {
  typedef typename JStageT<PREC>::T T;
  T* p = reinterpret_cast<T*>(st);
  const int lane = nsim_lane(), j = lane & 31, hi = lane >> 5;
  if constexpr (PREC == 0 && NSIM_STAGE_PAIRS) {
#pragma unroll
    for (int m = 0; m < NM; ++m)
#pragma unroll
      for (int r = 0; r < 16; r += 2) {
        bf16 lo, hi16;
        nsim_cvt2_bf16(v[m * 16 + r] * scale, v[m * 16 + r + 1] * scale, lo, hi16);
        p[unit_of(m, r, hi) * JStageT<PREC>::PITCH + 32 * wave + j] = lo;
        p[unit_of(m, r + 1, hi) * JStageT<PREC>::PITCH + 32 * wave + j] = hi16;
      }
    return;
  }
#pragma unroll
  for (int m = 0; m < NM; ++m)
#pragma unroll
    for (int r = 0; r < 16; ++r) p[unit_of(m, r, hi) * JStageT<PREC>::PITCH + 32 * wave + j] = (T)(v[m * 16 + r] * scale);
}

// acc += A[32 mo + row][:] . B[32 no + col][:]^T over the staged points [16 S0, 16 S1)  (default: all JOINT_PTS)
template <int PREC, int S0 = 0, int S1 = JOINT_PTS / 16>
__device__ __forceinline__ f32x16 jdw_tile(const void* stA, int mo, const void* stB, int no, f32x16 acc) {
  typedef typename JStageT<PREC>::T T;
  constexpr int P = JStageT<PREC>::PITCH;
  const T* a = reinterpret_cast<const T*>(stA);
  const T* b = reinterpret_cast<const T*>(stB);
  const int lane = nsim_lane(), i = lane & 31, hi = lane >> 5;
  if constexpr (PREC == 0) {
#pragma unroll
    for (int s = S0; s < S1; ++s) {
      const bf16x8 av = *reinterpret_cast<const bf16x8*>(a + (32 * mo + i) * P + 16 * s + 8 * hi);
      const bf16x8 bv = *reinterpret_cast<const bf16x8*>(b + (32 * no + i) * P + 16 * s + 8 * hi);
      acc = mfma_32x32x16_bf16(av, bv, acc);
    }
  } else {
#pragma unroll 8
    for (int q = 8 * S0; q < 8 * S1; ++q) {
      const float av = a[(32 * mo + i) * P + 2 * q + hi];
      const float bv = b[(32 * no + i) * P + 2 * q + hi];
      acc = mfma_32x32x2_f32(av, bv, acc);
    }
  }
  return acc;
}

// sum of row ``lane`` over THIS wave's 32 staged points (bias gradients; every wave keeps its own partial sum, so no
// wave becomes the straggler of the next barrier).  bf16: v_dot2c_f32_bf16 against (1, 1) adds two points per issue.
template <int PREC>
__device__ __forceinline__ float jrow_sum(const void* stA, int rows, int wave) {
  typedef typename JStageT<PREC>::T T;
  constexpr int P = JStageT<PREC>::PITCH;
  const T* a = reinterpret_cast<const T*>(stA);
  const int lane = nsim_lane();
  float s = 0.f;
  if (lane < rows) {
    if constexpr (PREC == 0) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const bf16x8 v = *reinterpret_cast<const bf16x8*>(a + lane * P + 32 * wave + 8 * q);
        s = nsim_bf16x8_sum(v, s);
      }
    } else {
      for (int q = 0; q < 32; ++q) s += a[lane * P + 32 * wave + q];
    }
  }
  return s;
}

// flush an accumulator tile with global atomics: dst[(32 mo + row) * ld + 32 no + col], rows < rows, cols < cols
__device__ __forceinline__ void jflush_tile(float* dst, int ld, int rows, int cols, int mo, int no, const f32x16& acc) {
  const int lane = nsim_lane(), col = 32 * no + (lane & 31), hi = lane >> 5;
  if (col >= cols) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = 32 * mo + mfma_row(r, hi);
    if (row < rows && acc[r] != 0.f) atomicAdd(&dst[row * ld + col], acc[r]);
  }
}

// Sum v0 / v1 over the runs of equal ``key`` among the 32 lanes of each wave half (keys arrive grouped: consecutive
// samples of a ray are neighbouring lanes); the run total is valid on the LAST lane of the run, for which the function
// returns true.  Used to issue ONE atomic per (ray, channel) and wave instead of one per sample: same-address atomics of
// one instruction are separate requests to the atomic unit (21 G requests/s chip-wide) and serialise in L2.
__device__ __forceinline__ bool halfwave_run_sum2(int64_t key, bool valid, float& v0, float& v1) {
  const int lane = nsim_lane();
  const int64_t k = valid ? key : (int64_t)-1 - lane;          // invalid lanes: runs of their own
  const int64_t pk = wave_shfl(k, lane - 1);
  const unsigned long long heads = wave_ballot((lane & 31) == 0 || pk != k);
  const unsigned long long below = heads & ((2ull << lane) - 1ull);
  const int run_start = 63 - __builtin_clzll(below);
#pragma unroll
  for (int d = 1; d < 32; d <<= 1) {
    const float o0 = wave_shfl(v0, lane - d), o1 = wave_shfl(v1, lane - d);
    if (lane - d >= run_start) {
      v0 += o0;
      v1 += o1;
    }
  }
  return valid && ((lane & 31) == 31 || ((heads >> (lane + 1)) & 1ull));
}


// ===================================================================== 16-point tiles (v_mfma_f32_16x16x32_*)
// Activation-register convention (one wave = 16 points): lane l (p = l & 15, g = l >> 4) owns point p and the units
// 16m + 4g + r (register 4m + r) of a layer -- the C/D fragment of v_mfma_f32_16x16x32.  The B operand of K-step c is
// registers 8c .. 8c + 7 as they stand: K index 8g + e <-> unit 16(2c + (e >> 2)) + 4g + (e & 3), and the weight pack (the A
// operand, frag16_f16 below) uses the same permutation, so layers chain in registers as in the 32-point convention.  Half
// the activation registers per lane: the with-grad backward fits 256 registers and runs two waves per SIMD.
// Weight gradients: the waves of a workgroup stage their activations side by side as [point][unit] rows (one 8-byte store
// per m-tile and lane) and read them back column-wise with ds_read_b64_tr_b16 (J16_ROW below).
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4 zero4() {
  f32x4 z;
#pragma unroll
  for (int r = 0; r < 4; ++r) z[r] = 0.f;
  return z;
}

// D = A . B + C on v_mfma_f32_16x16x32_{f16,bf16}: A lane l -> row l & 15, B lane l -> col l & 15, K index 8(l >> 4) + e;
// C/D: col = l & 15, row = 4(l >> 4) + r.  Outside a HIP compile (the host emulator of the tests) the same product is
// formed from wave_shfl, in the layout the CDNA4 guide states.
#if defined(__HIP__)
__device__ __forceinline__ f32x4 mfma_16x16x32_f16(f16x8 a, f16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma_16x16x32_bf16(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
#else
template <class V>
inline f32x4 mfma_16x16x32_portable(V a, V b, f32x4 c) {
  const int lane = nsim_lane(), col = lane & 15, g = lane >> 4;
  f32x4 d = c;
  for (int G = 0; G < 4; ++G) {
    const V bs = wave_shfl(b, 16 * G + col);
    for (int r = 0; r < 4; ++r) {
      const V as = wave_shfl(a, 16 * G + 4 * g + r);
      float s = 0.f;
      for (int e = 0; e < 8; ++e) s += (float)as[e] * (float)bs[e];
      d[r] += s;
    }
  }
  return d;
}
inline f32x4 mfma_16x16x32_f16(f16x8 a, f16x8 b, f32x4 c) { return mfma_16x16x32_portable(a, b, c); }
inline f32x4 mfma_16x16x32_bf16(bf16x8 a, bf16x8 b, f32x4 c) { return mfma_16x16x32_portable(a, b, c); }
#endif

// ds_read_b64_tr_b16: per group of 16 lanes, lane 4q + p names 4 consecutive 16-bit elements of row q of a 4 x 16 block;
// lane i of the group receives column i of the 4 rows (row q in element q).  Every lane of the wave must execute it.
__device__ __forceinline__ bf16x4 lds_read_tr16(const bf16* p) {
#if defined(__HIP__)
  return __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)p);
#else
  const int lane = nsim_lane(), G = lane >> 4, i = lane & 15;
  const unsigned long long me = (unsigned long long)(uintptr_t)p;
  bf16x4 r;
  for (int q = 0; q < 4; ++q) {
    const unsigned long long src = wave_shfl(me, 16 * G + 4 * q + (i >> 2));
    r[q] = reinterpret_cast<const bf16*>((uintptr_t)src)[i & 3];
  }
  return r;
#endif
}

// acc[mo] += W16[16 mo.., :] . In^T, In in 16-point register order (NT 16-unit tiles, NT even), scaled by in_scale before
// the f16 conversion
template <int MO, int NT>
__device__ __forceinline__ void contract16(f32x4 (&acc)[MO], const char* wmat, const float (&in)[NT * 4], float in_scale) {
  static_assert(NT % 2 == 0, "contract16: whole K-steps of 32 inputs");
  const int lane = nsim_lane();
  const f16x8* A = reinterpret_cast<const f16x8*>(wmat);
#pragma unroll
  for (int c = 0; c < NT / 2; ++c) {
    f16x8 b;
#pragma unroll
    for (int e = 0; e < 8; ++e) b[e] = (f16)(in[8 * c + e] * in_scale);
#pragma unroll
    for (int mo = 0; mo < MO; ++mo) acc[mo] = mfma_16x16x32_f16(A[(mo * (NT / 2) + c) * 64 + lane], b, acc[mo]);
  }
}

// The inverse of the A-fragment indexing of contract16 just above: k = ((mo * (Ui / 32) + c) * 64 + lane) * 8 + e
__host__ __device__ inline FragRC frag16_f16(int64_t k, int Ui) {
  const int e = (int)(k & 7), lane = (int)((k >> 3) & 63), fs = (int)(k >> 9), nS = Ui / 32;
  return FragRC{16 * (fs / nS) + (lane & 15), 32 * (fs % nS) + 16 * (e >> 2) + 4 * (lane >> 4) + (e & 3)};
}

// out[4 mo + r] = (W16 . In^T)[16 mo + 4g + r][pt]   (fp16, dynamic: power-of-two re-scaling of In, as dense)
template <int MO, int NT>
__device__ __forceinline__ void dense16(float (&out)[MO * 4], const char* wmat, const float (&in)[NT * 4], bool dynamic) {
  f32x4 acc[MO];
#pragma unroll
  for (int mo = 0; mo < MO; ++mo) acc[mo] = zero4();
  const float sc = dynamic ? dyn_scale<0, NT * 4>(in) : 1.0f;
  contract16<MO, NT>(acc, wmat, in, sc);
  const float inv = 1.0f / sc;
#pragma unroll
  for (int mo = 0; mo < MO; ++mo)
#pragma unroll
    for (int r = 0; r < 4; ++r) out[mo * 4 + r] = acc[mo][r] * inv;
}

// ------------------------------------------------------------------------------------- writing a weight pack
// precision 2 ("split"): an f32 value travels through the f16 matrix cores as v = hi + lo / SPLIT_LO_SCALE with
// hi = f16(v), lo = f16((v - hi) * SPLIT_LO_SCALE) -- 22 significant bits; a product W . x is three MFMAs (hi.hi into the
// main accumulator, hi.lo + lo.hi into a correction accumulator that is folded in with 1 / SPLIT_LO_SCALE), the
// dropped lo.lo term is 2^-22 relative.  The scale keeps the residuals out of the f16 subnormals.
#define SPLIT_LO_SCALE 2048.0f

// fragment form of a packed matrix: 32-point f16 | 32-point f32 | split (the f16 form twice: hi, then lo at + Uo Ui) |
// 16-point f16
enum { PACK_F16 = 0, PACK_F32, PACK_SPLIT, PACK_F16_16 };
__host__ __device__ inline int pack_form(int elt, int split = 0) { return split ? PACK_SPLIT : (elt == 2 ? PACK_F16 : PACK_F32); }

// the matrices of a pack, in the order of its layout
#define PACK_MAX_MATS 10       // (every decoder asserts its matrix count against it)
struct PackShape {
  int uo[PACK_MAX_MATS], ui[PACK_MAX_MATS];
};
static inline PackShape pack_shape(int n, const int* uo, const int* ui) {
  PackShape sh;
  for (int m = 0; m < n; ++m) {
    sh.uo[m] = uo[m];
    sh.ui[m] = ui[m];
  }
  return sh;
}
// threads of a pack launch: one per element of the first n matrices + ``extra`` (vector slots, further fragment sets)
static inline int64_t pack_elems(const PackShape& sh, int n, int64_t extra) {
  for (int m = 0; m < n; ++m) extra += (int64_t)sh.uo[m] * sh.ui[m];
  return extra;
}

// One thread per matrix element: thread ``tid`` finds the matrix m < n and the element k of it that are its own, and
// stores src(m, row, col) at byte offset off[m] of ``wpack``, element k, in fragment form ``form``.  Returns false for a
// thread past the matrices, with their element count taken off ``tid``.
template <class Src>
__device__ __forceinline__ bool pack_matrices(const PackShape& sh, int n, const int64_t* off, int form, char* wpack,
                                              int64_t& tid, Src src) {
  for (int m = 0; m < n; ++m) {
    const int Ui = sh.ui[m];
    const int64_t cnt = (int64_t)sh.uo[m] * Ui;
    if (tid < cnt) {
      const int64_t k = tid;
      const FragRC rc = form == PACK_F32 ? frag32_f32(k, Ui) : (form == PACK_F16_16 ? frag16_f16(k, Ui) : frag32_f16(k, Ui));
      const float w = src(m, rc.row, rc.col);
      if (form == PACK_F32) {
        ((float*)(wpack + off[m]))[k] = w;
      } else {
        const f16 whi = (f16)w;
        ((f16*)(wpack + off[m]))[k] = whi;
        if (form == PACK_SPLIT) ((f16*)(wpack + off[m]))[cnt + k] = (f16)((w - (float)whi) * SPLIT_LO_SCALE);
      }
      return true;
    }
    tid -= cnt;
  }
  return false;
}

// ------------------------------------------------------------------------------------- SH-4 of a view direction
__device__ __forceinline__ void sh4_eval(const float d[3], float (&o)[16]) {
  const float x = d[0], y = d[1], z = d[2];
  const float xy = x * y, xz = x * z, yz = y * z, x2 = x * x, y2 = y * y, z2 = z * z;
  o[0] = 0.28209479177387814f;
  o[1] = -0.48860251190291987f * y;
  o[2] = 0.48860251190291987f * z;
  o[3] = -0.48860251190291987f * x;
  o[4] = 1.0925484305920792f * xy;
  o[5] = -1.0925484305920792f * yz;
  o[6] = 0.94617469575755997f * z2 - 0.31539156525251999f;
  o[7] = -1.0925484305920792f * xz;
  o[8] = 0.54627421529603959f * x2 - 0.54627421529603959f * y2;
  o[9] = 0.59004358992664352f * y * (-3.0f * x2 + y2);
  o[10] = 2.8906114426405538f * xy * z;
  o[11] = 0.45704579946446572f * y * (1.0f - 5.0f * z2);
  o[12] = 0.3731763325901154f * z * (5.0f * z2 - 3.0f);
  o[13] = 0.45704579946446572f * x * (1.0f - 5.0f * z2);
  o[14] = 1.4453057213202769f * z * (x2 - y2);
  o[15] = 0.59004358992664352f * x * (-x2 + 3.0f * y2);
}

// out[c] = sum_k g[k] * d sh4_k / d d_c   (pose refinement: gradient w.r.t. the view direction)
__device__ __forceinline__ void sh4_grad(const float d[3], const float (&g)[16], float (&out)[3]) {
  const float x = d[0], y = d[1], z = d[2];
  const float x2 = x * x, y2 = y * y, z2 = z * z;
  const float a1 = 0.48860251190291987f, b = 1.0925484305920792f, c1 = 0.94617469575755997f;
  const float e = 0.54627421529603959f, f = 0.59004358992664352f, gg = 2.8906114426405538f;
  const float h = 0.45704579946446572f, i3 = 0.3731763325901154f, jj = 1.4453057213202769f;
  out[0] = -a1 * g[3] + b * y * g[4] - b * z * g[7] + 2.0f * e * x * g[8] - 6.0f * f * x * y * g[9] + gg * y * z * g[10] +
           h * (1.0f - 5.0f * z2) * g[13] + 2.0f * jj * z * x * g[14] + f * (-3.0f * x2 + 3.0f * y2) * g[15];
  out[1] = -a1 * g[1] + b * x * g[4] - b * z * g[5] - 2.0f * e * y * g[8] + f * (-3.0f * x2 + 3.0f * y2) * g[9] +
           gg * x * z * g[10] + h * (1.0f - 5.0f * z2) * g[11] - 2.0f * jj * z * y * g[14] + 6.0f * f * x * y * g[15];
  out[2] = a1 * g[2] - b * y * g[5] + 2.0f * c1 * z * g[6] - b * x * g[7] + gg * x * y * g[10] - 10.0f * h * y * z * g[11] +
           i3 * (15.0f * z2 - 3.0f) * g[12] - 10.0f * h * x * z * g[13] + jj * (x2 - y2) * g[14];
}

// ---- LDS staging [point][unit] bf16 for the workgroup-joint weight gradients: J16_PTS rows of 128 bytes (<= 64 units).
// The 8-byte chunk ch (units 4ch .. 4ch + 3) of row ``row`` sits at chunk ch ^ j16_swz(row): the 16 lanes of a
// ds_write_b64 (16 consecutive rows, one chunk) hit 16 distinct chunk slots, and each 32-lane half of a transposed read
// (8 consecutive rows, 4 chunks) covers the 64 banks once -- both conflict-free.
#define J16_PTS (16 * JOINT_WAVES)
#define J16_ROW 128
#define J16_STAGE_BYTES (J16_PTS * J16_ROW)

__device__ __forceinline__ int j16_swz(int row) { return (((row >> 1) & 3) << 2) | (row & 1) | ((row >> 2) & 2); }

// write this wave's 16 points of an activation (NT 16-unit tiles in 16-point register order) into rows 16 wave + p
template <int NT>
__device__ __forceinline__ void jstage16(void* st, const float (&v)[NT * 4], int wave) {
  const int lane = nsim_lane(), p = lane & 15, g = lane >> 4;
  const int row = 16 * wave + p;
  char* base = reinterpret_cast<char*>(st) + row * J16_ROW;
  const int swz = j16_swz(row);
#pragma unroll
  for (int m = 0; m < NT; ++m) {
    bf16x4 w;
    bf16 b0, b1, b2, b3;
    nsim_cvt2_bf16(v[4 * m], v[4 * m + 1], b0, b1);
    nsim_cvt2_bf16(v[4 * m + 2], v[4 * m + 3], b2, b3);
    w[0] = b0; w[1] = b1; w[2] = b2; w[3] = b3;
    *reinterpret_cast<bf16x4*>(base + 8 * ((4 * m + g) ^ swz)) = w;
  }
}

// the 16x16x32 operand of units 16 t + (l & 15) over K-step c of the staged points: K index 8G + e (G = l >> 4) <-> staged
// row 32 c + 16 (e >> 2) + 4 G + (e & 3) -- the same for the A and the B side, so the product sums over the points
__device__ __forceinline__ bf16x8 j16_operand(const void* st, int t, int c) {
  const int lane = nsim_lane(), G = lane >> 4, q = (lane >> 2) & 3, pc = lane & 3;
  const char* base = reinterpret_cast<const char*>(st);
  bf16x8 o;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int row = 32 * c + 16 * h + 4 * G + q;
    const bf16x4 v = lds_read_tr16(reinterpret_cast<const bf16*>(base + row * J16_ROW + 8 * ((4 * t + pc) ^ j16_swz(row))));
#pragma unroll
    for (int e = 0; e < 4; ++e) o[4 * h + e] = v[e];
  }
  return o;
}

// acc[n] += A[16 ta + row][:] . B[16 tb_n + col][:]^T over all staged points, tb_n = TB0 + n; rs (optional) += the sum of
// this lane's share of A's row 16 ta + (l & 15) (summed over the four lane groups at the flush: a bias gradient for free)
template <int NB>
__device__ __forceinline__ void jdw16_tiles(const void* stA, int ta, const void* stB, int tb0, f32x4 (&acc)[NB], float* rs) {
#pragma unroll
  for (int c = 0; c < J16_PTS / 32; ++c) {
    const bf16x8 av = j16_operand(stA, ta, c);
    if (rs) *rs = nsim_bf16x8_sum(av, *rs);
#pragma unroll
    for (int n = 0; n < NB; ++n) acc[n] = mfma_16x16x32_bf16(av, j16_operand(stB, tb0 + n, c), acc[n]);
  }
}

// the same row share without a product (a staged vector whose gradient is a plain sum over points)
__device__ __forceinline__ float j16_row_share(const void* st, int t) {
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < J16_PTS / 32; ++c) s = nsim_bf16x8_sum(j16_operand(st, t, c), s);
  return s;
}

// flush a 16x16 accumulator tile: dst[(16 to + 4 (l >> 4) + r) * ld + 16 tn + (l & 15)], columns < cols
__device__ __forceinline__ void jflush16(float* dst, int ld, int cols, int to, int tn, const f32x4& acc) {
  const int lane = nsim_lane(), col = 16 * tn + (lane & 15);
  if (col >= cols) return;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = 16 * to + 4 * (lane >> 4) + r;
    if (acc[r] != 0.f) atomicAdd(&dst[row * ld + col], acc[r]);
  }
}
