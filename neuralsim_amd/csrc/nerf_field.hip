// nerf_field.hip -- the NeRF++ distant-view model (``LoTDNeRFDistant``) on gfx950: inverse-radius cuboid-shell
// sampling, 4-D LoTD (quadrilinear, 16 corners per level) gather / scatter, density MLP (F -> 64 -> 1, softplus
// output) and radiance MLP ([features, SH-4 view dir, appearance-4] -> 64 -> 64 -> 3) forward + backward on the
// matrix cores, and sigma -> alpha.
//
// Replaces the native half of nr3d_lib.models.fields_distant.nerf.LoTDNeRFDistantModel as the reference drives it
// (app/models/single/nerf.py:145-196; call site app/renderers/single_volume_renderer.py:281-309; config
// code_single/configs/object_centric/lotd_neus.dtu.230814.yaml:186-247).  Executable spec: oracle/distant.py.
// Same register-resident transposed-MFMA scheme as field.hip (mfma_mlp.h); no second-order terms are needed here
// (the distant model has ``use_nablas: false``).
#include "mfma_mlp.h"
#include "lotd_dev.h"
#include <stdlib.h>

#define D4_MAX_LEVELS 16

struct Lotd4Dev {
  int num_levels;
  int res_xyz[D4_MAX_LEVELS], res_y[D4_MAX_LEVELS], res_z[D4_MAX_LEVELS], res_w[D4_MAX_LEVELS], type[D4_MAX_LEVELS];
  uint32_t size[D4_MAX_LEVELS];
  int64_t offset[D4_MAX_LEVELS];
};

static inline Lotd4Dev lotd4_dev(const NsimLotd4Meta* m) {
  Lotd4Dev d;
  d.num_levels = m->num_levels;
  for (int l = 0; l < D4_MAX_LEVELS; ++l) {
    const bool ok = l < m->num_levels;
    d.res_xyz[l] = ok ? m->res_xyz[l] : 2;
    d.res_y[l] = ok ? (m->res_y[l] > 0 ? m->res_y[l] : m->res_xyz[l]) : 2;      // 0: cubic level
    d.res_z[l] = ok ? (m->res_z[l] > 0 ? m->res_z[l] : m->res_xyz[l]) : 2;
    d.res_w[l] = ok ? m->res_w[l] : 2;
    d.type[l] = ok ? m->type[l] : 0;
    d.size[l] = ok ? m->size[l] : 16;
    d.offset[l] = ok ? m->offset[l] : 0;
  }
  return d;
}

static int lotd4_meta_check(const NsimLotd4Meta* m) {
  if (!m) return 10;
  if (m->num_levels < 1 || m->num_levels > D4_MAX_LEVELS) return 12;
  for (int l = 0; l < m->num_levels; ++l) {
    if (m->res_xyz[l] < 2 || m->res_w[l] < 2) return 13;
    if (m->res_y[l] == 1 || m->res_z[l] == 1 || m->res_y[l] < 0 || m->res_z[l] < 0) return 13;
    const uint64_t ry = m->res_y[l] > 0 ? m->res_y[l] : m->res_xyz[l], rz = m->res_z[l] > 0 ? m->res_z[l] : m->res_xyz[l];
    if (m->type[l] == NSIM_LOTD_DENSE) {
      if ((uint64_t)m->res_xyz[l] * ry * rz * m->res_w[l] != (uint64_t)m->size[l]) return 14;
    } else if (m->type[l] == NSIM_LOTD_HASH) {
      if (m->size[l] == 0 || (m->size[l] & (m->size[l] - 1)) != 0) return 17;
    } else {
      return 15;
    }
    if (m->offset[l] & 1) return 16;
  }
  return 0;
}

struct Cell4 {
  int c0[4];
  float w[4];
};

__device__ __forceinline__ Cell4 lotd4_cell(const float u[4], int Rx, int Ry, int Rz, int Rw) {
  Cell4 c;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int R = a == 0 ? Rx : (a == 1 ? Ry : (a == 2 ? Rz : Rw));
    const float pos = u[a] * (float)(R - 1);
    float f = floorf(pos);
    f = fminf(fmaxf(f, 0.f), (float)(R - 2));
    c.c0[a] = (int)f;
    c.w[a] = pos - f;
  }
  return c;
}

__device__ __forceinline__ uint32_t lotd4_index(int cx, int cy, int cz, int cw, int Rx, int Ry, int Rz, int type,
                                                uint32_t T) {
  if (type == NSIM_LOTD_DENSE)
    return (uint32_t)cx + (uint32_t)Rx * ((uint32_t)cy + (uint32_t)Ry * ((uint32_t)cz + (uint32_t)Rz * (uint32_t)cw));
  const uint32_t h = (uint32_t)cx ^ ((uint32_t)cy * 2654435761u) ^ ((uint32_t)cz * 805459861u) ^
                     ((uint32_t)cw * 3674653429u);
  return h & (T - 1u);
}

// vertex order of the 4-D gathers: slot k reads the vertex with the coordinate parities of k's bits (lotd_dev.h, NSIM_GATHER_PARITY)
__device__ __forceinline__ int lotd4_slot_mask(const Cell4& c) {
  return NSIM_GATHER_PARITY ? ((c.c0[0] & 1) | ((c.c0[1] & 1) << 1) | ((c.c0[2] & 1) << 2) | ((c.c0[3] & 1) << 3)) : 0;
}

__device__ __forceinline__ float lotd4_weight(const Cell4& c, int corner) {
  float w = 1.0f;
#pragma unroll
  for (int a = 0; a < 4; ++a) w = w * (((corner >> a) & 1) ? c.w[a] : 1.0f - c.w[a]);
  return w;
}

__device__ __forceinline__ void lotd4_load2(const f16* grid, int64_t off, uint32_t idx, float& f0, float& f1) {
  const uint32_t raw = *reinterpret_cast<const uint32_t*>(grid + off + 2 * (int64_t)idx);
  union {
    uint32_t u;
    f16 h[2];
  } cv;
  cv.u = raw;
  f0 = (float)cv.h[0];
  f1 = (float)cv.h[1];
}

// ----------------------------------------------------------------------------------------- sampling
// One thread per (ray, shell): 1/r uniform in [1/r_max, 1/r_min]; the sample sits where the ray leaves the AABB
// scaled by r about its centre.
__global__ void __launch_bounds__(256) k_distant_shells(const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                                         const float* __restrict__ near, const float* __restrict__ jitter,
                                                         int64_t N, int K, float cx, float cy, float cz, float hx, float hy, float hz, float r_min,
                                                         float r_max, float* __restrict__ t_out,
                                                         float* __restrict__ u4_out, uint8_t* __restrict__ valid_out) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= N * K) return;
  const int64_t ray = s / K;
  const int k = (int)(s % K);
  const float u = jitter ? jitter[s] : 0.5f;
  const float inv_r = 1.0f / r_min + (((float)k + u) / (float)K) * (1.0f / r_max - 1.0f / r_min);
  const float r = 1.0f / inv_r;
  const float c[3] = {cx, cy, cz}, hf[3] = {hx, hy, hz};
  float tmin = -INFINITY, tmax = INFINITY, o[3], d[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    o[a] = rays_o[3 * ray + a] - c[a];
    d[a] = rays_d[3 * ray + a];
    float ds = d[a];
    if (fabsf(ds) < 1e-12f) ds = (ds < 0.f) ? -1e-12f : 1e-12f;
    const float inv = 1.0f / ds;
    const float hr = hf[a] * r;
    const float t1 = (-hr - o[a]) * inv, t2 = (hr - o[a]) * inv;
    tmin = fmaxf(tmin, fminf(t1, t2));
    tmax = fminf(tmax, fmaxf(t1, t2));
  }
  const bool valid = (tmax > tmin) && (tmax > near[ray]);
  t_out[s] = tmax;
  valid_out[s] = valid ? 1 : 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float x = rays_o[3 * ray + a] + tmax * d[a];
    float un = (x - c[a]) / hf[a] * inv_r;
    un = un * 0.5f + 0.5f;
    u4_out[4 * s + a] = fminf(fmaxf(un, 0.f), 1.f);
  }
  u4_out[4 * s + 3] = fminf(fmaxf(inv_r, 0.f), 1.f);
}

// alpha_k = 1 - exp(-sigma_k * delta_k), delta = t_{k+1} - t_k; the last shell reaches to infinity (1e10,
// ``include_inf_distance: true``, object-centric configs) or repeats the previous interval (``false``: the street
// config, whose sky model takes the remaining transmittance); 0 on invalid shells
__device__ __forceinline__ float shell_delta(const float* t, const uint8_t* valid, int64_t s, int k, int K, int include_inf) {
  if (k + 1 < K) return t[s + 1] - t[s];
  if (include_inf) return 1e10f;
  return (k > 0 && valid[s - 1]) ? t[s] - t[s - 1] : 0.f;
}

__global__ void __launch_bounds__(256) k_density_alpha_fwd(const float* __restrict__ sigma, const float* __restrict__ t,
                                                            const uint8_t* __restrict__ valid, int64_t N, int K,
                                                            int include_inf, float* __restrict__ alpha) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= N * K) return;
  const int k = (int)(s % K);
  const float delta = shell_delta(t, valid, s, k, K, include_inf);
  alpha[s] = valid[s] ? 1.0f - expf(-sigma[s] * delta) : 0.f;
}

__global__ void __launch_bounds__(256) k_density_alpha_bwd(const float* __restrict__ sigma, const float* __restrict__ t,
                                                            const uint8_t* __restrict__ valid,
                                                            const float* __restrict__ dalpha, int64_t N, int K,
                                                            int include_inf, float* __restrict__ dsigma) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= N * K) return;
  const int k = (int)(s % K);
  const float delta = shell_delta(t, valid, s, k, K, include_inf);
  dsigma[s] = valid[s] ? dalpha[s] * delta * expf(-sigma[s] * delta) : 0.f;
}

// ----------------------------------------------------------------------------------------- weight pack
enum { N_D1 = 0, N_D1T, N_Q1, N_Q2, N_Q3, N_Q3T, N_Q2T, N_Q1T, N_MCOUNT };
enum { NV_DB1 = 0, NV_DWH, NV_RB1, NV_RB2, NV_RB3, NV_SCAL, NV_COUNT };
static_assert(N_MCOUNT <= PACK_MAX_MATS, "PackShape holds the distant model's matrices");
static const int kNUo[N_MCOUNT] = {64, 32, 64, 64, 32, 64, 64, 64};
static const int kNUi[N_MCOUNT] = {32, 64, 64, 64, 64, 32, 64, 64};

struct NerfLayout {
  int64_t mat[N_MCOUNT], vec[NV_COUNT], total;
  int elt;
};
static inline NerfLayout nerf_layout(int precision) {
  NerfLayout L;
  L.elt = precision == 0 ? 2 : 4;
  int64_t off = 0;
  for (int m = 0; m < N_MCOUNT; ++m) {
    L.mat[m] = off;
    off += (int64_t)kNUo[m] * kNUi[m] * L.elt;
  }
  for (int v = 0; v < NV_COUNT; ++v) {
    L.vec[v] = off;
    off += 64 * 4;
  }
  L.total = off;
  return L;
}

// radiance input slot (0..63) -> column of the [64 x (F+20)] first radiance layer, or -1
__host__ __device__ inline int q1_col(int slot, int F) {
  if (slot < 32) return slot < F ? slot : -1;
  if (slot < 48) return F + (slot - 32);
  if (slot < 52) return F + 16 + (slot - 48);
  return -1;
}

__device__ __forceinline__ float nerf_src(int mat, int row, int col, int F, const float* den_w, const float* rad_w) {
  const int K1 = F + 20;
  const int q2 = 64 * K1, q3 = q2 + 4096;
  switch (mat) {
    case N_D1: return col < F ? den_w[row * F + col] : 0.f;
    case N_D1T: return row < F ? den_w[col * F + row] : 0.f;
    case N_Q1: { const int c = q1_col(col, F); return c >= 0 ? rad_w[row * K1 + c] : 0.f; }
    case N_Q1T: { const int c = q1_col(row, F); return c >= 0 ? rad_w[col * K1 + c] : 0.f; }
    case N_Q2: return rad_w[q2 + row * 64 + col];
    case N_Q2T: return rad_w[q2 + col * 64 + row];
    case N_Q3: return row < 3 ? rad_w[q3 + row * 64 + col] : 0.f;
    case N_Q3T: return col < 3 ? rad_w[q3 + col * 64 + row] : 0.f;
  }
  return 0.f;
}

__global__ void __launch_bounds__(256) k_nerf_pack(NerfLayout L, PackShape sh, int F, const float* __restrict__ den_w,
                                                    const float* __restrict__ den_b, const float* __restrict__ rad_w,
                                                    const float* __restrict__ rad_b, char* __restrict__ wpack) {
  int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const auto src = [&](int m, int row, int col) { return nerf_src(m, row, col, F, den_w, rad_w); };
  if (pack_matrices(sh, N_MCOUNT, L.mat, pack_form(L.elt), wpack, tid, src)) return;
  if (tid < (int64_t)NV_COUNT * 64) {
    const int v = (int)(tid >> 6), k = (int)(tid & 63), u = vec_unit(k, 64);
    float val = 0.f;
    switch (v) {
      case NV_DB1: val = den_b[u]; break;
      case NV_DWH: val = den_w[64 * F + u]; break;
      case NV_RB1: val = rad_b[u]; break;
      case NV_RB2: val = rad_b[64 + u]; break;
      case NV_RB3: val = u < 3 ? rad_b[128 + u] : 0.f; break;
      case NV_SCAL: val = (k == 0) ? den_b[64] : 0.f; break;
    }
    ((float*)(wpack + L.vec[v]))[k] = val;
  }
}

// ----------------------------------------------------------------------------------------- MLP kernels
struct NerfArgs {
  Lotd4Dev lotd;
  NerfLayout lay;
  int F;                                  // real feature count = 2 * num_levels (<= 32)
  const f16* grid;
  const char* wpack;
  const float* u4;                        // [S,4] in [0,1]
  const float* rays_d;                    // [N,3]
  const float* h_appear;                  // [N,4] or NULL
  const uint8_t* valid;                   // [S]
  int64_t S;
  int K;                                  // shells per ray (ray = s / K)
  float *sigma, *rgb;                     // forward outputs
  float* h_pl;                            // [16][S][2] saved features
  int h_from_planes;                      // forward: the features were gathered level-major (k_lotd4_gather_lm)
  const float *sigma_fwd, *rgb_fwd;       // saved forward outputs
  const float *dsigma, *drgb;             // upstream
  float* dh_pl;                           // [16][S][2] hand-off to the scatter
  float *dden_w, *dden_b, *drad_w, *drad_b, *dh_appear;
};

#define NERF_WAVES 4

// Stage the pack into LDS (fp16 mode): everything, or -- VEC_ONLY -- just the per-lane vectors (the matrices are then
// read from L2, which frees LDS for private weight-gradient accumulators).  Returns the base the VECTORS are addressed
// from: nvec() uses offsets relative to lay.vec[0].
template <int PREC, bool VEC_ONLY>
__device__ __forceinline__ const char* nerf_stage_weights(char* smem, const NerfArgs& a, int& used, const char*& WM) {
  if constexpr (PREC == 0) {
    const int64_t first = VEC_ONLY ? a.lay.vec[0] : 0;
    const int n16 = (int)((a.lay.total - first + 15) >> 4);
    const f16x8* src = reinterpret_cast<const f16x8*>(a.wpack + first);
    f16x8* dst = reinterpret_cast<f16x8*>(smem);
    for (int i = threadIdx.x; i < n16; i += blockDim.x) dst[i] = src[i];
    used = n16 << 4;
    __syncthreads();
    WM = VEC_ONLY ? a.wpack : smem;
    return VEC_ONLY ? smem : smem + a.lay.vec[0];
  } else {
    used = 0;
    WM = a.wpack;
    return a.wpack + a.lay.vec[0];
  }
}

__device__ __forceinline__ float nvec(const char* WV, const NerfLayout& L, int v, int hi, int k) {
  return reinterpret_cast<const float*>(WV + (L.vec[v] - L.vec[0]))[hi * 32 + k];
}

// radiance input, second M-tile (slots 32..63): SH-4 of the view direction, appearance code, zero padding
__device__ __forceinline__ void nerf_rin_tail(float (&rin)[32], const float vd[3], const float ha[4], int hi) {
  float sh[16];
  sh4_eval(vd, sh);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int slot = unit_of(0, r, hi);  // position inside the second M-tile
    float v = 0.f;
    if (slot < 16) v = sh[slot];
    else if (slot < 20) v = ha[slot - 16];
    rin[16 + r] = v;
  }
}

struct NerfPoint {
  int64_t s, ray;
  bool valid;
  float vd[3], ha[4];
};
__device__ __forceinline__ NerfPoint nerf_point(const NerfArgs& a, int64_t tile, int j) {
  NerfPoint p;
  p.s = tile * 32 + j;
  p.valid = p.s < a.S;
  p.ray = p.valid ? p.s / a.K : 0;
  p.vd[0] = p.vd[1] = 0.f;
  p.vd[2] = 1.f;
  p.ha[0] = p.ha[1] = p.ha[2] = p.ha[3] = 0.f;
  if (p.valid) {
#pragma unroll
    for (int c = 0; c < 3; ++c) p.vd[c] = a.rays_d[3 * p.ray + c];
    if (a.h_appear) {
#pragma unroll
      for (int c = 0; c < 4; ++c) p.ha[c] = a.h_appear[4 * p.ray + c];
    }
  }
  return p;
}

__device__ __forceinline__ float softplus1(float x) { return x > 20.f ? x : log1pf(expf(x)); }

// fp16 backward: three waves per workgroup, each with a PRIVATE copy of the weight-gradient accumulators in LDS
// (plain read-add-write -- LDS float atomics cost ~800 cycles per instruction, mfma_mlp.h:dw_flush), matrices from L2.
#define NERF_WAVES_PRIV 3
template <int PREC, int BWD>
__global__ void __launch_bounds__(64 * ((PREC == 0 && BWD) ? NERF_WAVES_PRIV : NERF_WAVES)) k_nerf(NerfArgs a) {
  NSIM_DYN_SMEM(smem);
  constexpr bool PRIV = (PREC == 0 && BWD);
  constexpr int NW = PRIV ? NERF_WAVES_PRIV : NERF_WAVES;
  const int lane = nsim_lane(), j = lane & 31, hi = lane >> 5;
  const int wave = (int)(threadIdx.x >> 6);
  const NerfLayout& L = a.lay;
  int wbytes;
  const char* WM;
  const char* W = nerf_stage_weights<PREC, PRIV>(smem, a, wbytes, WM);
  // LDS accumulators (backward): D1 [64x32], DWH [64], DB1 [64], bd [4], Q1 [64x64], Q2 [64x64], Q3 [3x64], RB1, RB2, RB3
  constexpr int A_D1 = 0, A_DWH = 2048, A_DB1 = 2112, A_BD = 2176, A_Q1 = 2180, A_Q2 = A_Q1 + 4096, A_Q3 = A_Q2 + 4096,
                A_RB1 = A_Q3 + 192, A_RB2 = A_RB1 + 64, A_RB3 = A_RB2 + 64, A_TOTAL = A_RB3 + 4;
  float* accum = nullptr;
  char* stA = nullptr;
  char* stB = nullptr;
  if constexpr (BWD) {
    constexpr int ACC_BYTES = (A_TOTAL * 4 + 15) & ~15;
    accum = reinterpret_cast<float*>(smem + wbytes + (PRIV ? wave * ACC_BYTES : 0));
    char* stbase = smem + wbytes + (PRIV ? NW : 1) * ACC_BYTES + wave * stage_bytes_per_wave<PREC>();
    stA = stbase;
    stB = stbase + stage_bytes_per_wave<PREC>() / 2;
    if constexpr (PRIV) {
      for (int i = lane; i < A_TOTAL; i += 64) accum[i] = 0.f;
    } else {
      for (int i = threadIdx.x; i < A_TOTAL; i += blockDim.x) accum[i] = 0.f;
    }
    __syncthreads();
  }
  const float b_d = reinterpret_cast<const float*>(W + (L.vec[NV_SCAL] - L.vec[0]))[0];
  const int64_t ntiles = (a.S + 31) / 32;
  const int64_t wstride = (int64_t)gridDim.x * NW;
  for (int64_t tile = (int64_t)blockIdx.x * NW + wave; tile < ntiles; tile += wstride) {
    const NerfPoint p = nerf_point(a, tile, j);
    const int64_t s = p.s;
    if constexpr (BWD) {
      // a tile without a single live shell (behind an opaque foreground: the renderer's transmittance mask, folded into
      // ``valid`` by the host) contributes nothing -- its planes are not read, its dh rows not written (the scatter
      // skips the same shells)
      if (wave_ballot(p.valid && a.valid[s] != 0) == 0ull) continue;
    }
    // -------------------------------------------------------------- features: gather (forward) or planes (backward)
    float rin[32];  // [0,16): own features (first M-tile of the radiance input), [16,32): SH / appearance slots
    if (!BWD && a.h_from_planes) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const int l = 4 * q + 2 * hi + b;
          float f0 = 0.f, f1 = 0.f;
          if (p.valid && l < a.lotd.num_levels) {
            const float* hp = a.h_pl + ((int64_t)l * a.S + s) * 2;
            f0 = hp[0];
            f1 = hp[1];
          }
          rin[4 * q + 2 * b] = f0;
          rin[4 * q + 2 * b + 1] = f1;
        }
      }
    } else if constexpr (!BWD) {
      float u[4] = {0.f, 0.f, 0.f, 0.f};
      if (p.valid) {
#pragma unroll
        for (int c = 0; c < 4; ++c) u[c] = a.u4[4 * s + c];
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const int l = 4 * q + 2 * hi + b;   // level slot; slots >= num_levels are padding
          float f0 = 0.f, f1 = 0.f;
          if (l < a.lotd.num_levels) {
            const int Rx = a.lotd.res_xyz[l], Ry = a.lotd.res_y[l], Rz = a.lotd.res_z[l], Rw = a.lotd.res_w[l];
            const Cell4 c = lotd4_cell(u, Rx, Ry, Rz, Rw);
            const int pm4 = lotd4_slot_mask(c);
#pragma unroll
            for (int slot = 0; slot < 16; ++slot) {
              const int corner = slot ^ pm4;
              const float w = lotd4_weight(c, corner);
              const uint32_t idx = lotd4_index(c.c0[0] + (corner & 1), c.c0[1] + ((corner >> 1) & 1),
                                               c.c0[2] + ((corner >> 2) & 1), c.c0[3] + ((corner >> 3) & 1), Rx, Ry, Rz,
                                               a.lotd.type[l], a.lotd.size[l]);
              float g0, g1;
              lotd4_load2(a.grid, a.lotd.offset[l], idx, g0, g1);
              f0 = f0 + w * g0;
              f1 = f1 + w * g1;
            }
          }
          rin[4 * q + 2 * b] = f0;
          rin[4 * q + 2 * b + 1] = f1;
          if (a.h_pl && p.valid) {
            float* hp = a.h_pl + ((int64_t)l * a.S + s) * 2;
            hp[0] = f0;
            hp[1] = f1;
          }
        }
      }
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const int l = 4 * q + 2 * hi + b;
          float f0 = 0.f, f1 = 0.f;
          if (p.valid && l < a.lotd.num_levels) {      // (the level-major gather writes the pyramid's own levels only)
            const float* hp = a.h_pl + ((int64_t)l * a.S + s) * 2;
            f0 = hp[0];
            f1 = hp[1];
          }
          rin[4 * q + 2 * b] = f0;
          rin[4 * q + 2 * b + 1] = f1;
        }
      }
    }
    float h[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) h[r] = rin[r];
    nerf_rin_tail(rin, p.vd, p.ha, hi);
    // -------------------------------------------------------------- density + radiance forward
    float a1[32];
    dense<PREC, 2, 1>(a1, WM + L.mat[N_D1], h, true);
#pragma unroll
    for (int k = 0; k < 32; ++k) a1[k] = fmaxf(a1[k] + nvec(W, L, NV_DB1, hi, k), 0.f);
    float r1[32], r2[32];
    dense<PREC, 2, 2>(r1, WM + L.mat[N_Q1], rin, true);
#pragma unroll
    for (int k = 0; k < 32; ++k) r1[k] = fmaxf(r1[k] + nvec(W, L, NV_RB1, hi, k), 0.f);
    dense<PREC, 2, 2>(r2, WM + L.mat[N_Q2], r1, false);
#pragma unroll
    for (int k = 0; k < 32; ++k) r2[k] = fmaxf(r2[k] + nvec(W, L, NV_RB2, hi, k), 0.f);
    if constexpr (!BWD) {
      float raw = 0.f;
#pragma unroll
      for (int k = 0; k < 32; ++k) raw = raw + nvec(W, L, NV_DWH, hi, k) * a1[k];
      raw = raw + wave_shfl_xor(raw, 32) + b_d;
      float o3[16];
      dense<PREC, 1, 2>(o3, WM + L.mat[N_Q3], r2, false);
      if (p.valid && hi == 0) {
        a.sigma[s] = softplus1(raw);
#pragma unroll
        for (int c = 0; c < 3; ++c) a.rgb[3 * s + c] = 1.0f / (1.0f + nsim_fast_exp(-(o3[c] + nvec(W, L, NV_RB3, hi, c))));
      }
      continue;
    }
    if constexpr (BWD) {
      float gs = 0.f, sg = 0.f, gr[3] = {0.f, 0.f, 0.f}, rgbv[3] = {0.f, 0.f, 0.f};
      if (p.valid && a.valid[s]) {
        gs = a.dsigma ? a.dsigma[s] : 0.f;
        sg = a.sigma_fwd[s];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          gr[c] = a.drgb ? a.drgb[3 * s + c] : 0.f;
          rgbv[c] = a.rgb_fwd[3 * s + c];
        }
      }
      // ---- radiance branch
      float dout[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) dout[r] = 0.f;
      if (hi == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) dout[c] = gr[c] * rgbv[c] * (1.0f - rgbv[c]);
      }
      dw_product<PREC, 1, 2, PRIV>(stA, stB, dout, r2, accum + A_Q3, 64, 3, 64, accum + A_RB3);
      float dr2[32];
      dense<PREC, 2, 1>(dr2, WM + L.mat[N_Q3T], dout, true);
#pragma unroll
      for (int k = 0; k < 32; ++k) dr2[k] = r2[k] > 0.f ? dr2[k] : 0.f;
      dw_product<PREC, 2, 2, PRIV>(stA, stB, dr2, r1, accum + A_Q2, 64, 64, 64, accum + A_RB2);
      float dr1[32];
      dense<PREC, 2, 2>(dr1, WM + L.mat[N_Q2T], dr2, true);
#pragma unroll
      for (int k = 0; k < 32; ++k) dr1[k] = r1[k] > 0.f ? dr1[k] : 0.f;
      dw_product<PREC, 2, 2, PRIV>(stA, stB, dr1, rin, accum + A_Q1, 64, 64, 64, accum + A_RB1);
      float din[32];
      dense<PREC, 2, 2>(din, WM + L.mat[N_Q1T], dr1, true);
      // appearance slots 48..51 = second M-tile local 16..19: (hi0: r8..11 -> 16..19)
      // (summed over the shells of a ray inside the wave first: one atomic per ray and channel, not one per sample)
      if (a.dh_appear) {
        float c0 = din[16 + 8], c1 = din[16 + 9], c2 = din[16 + 10], c3 = din[16 + 11];
        const bool v = p.valid && hi == 0;
        const bool last = halfwave_run_sum2(p.ray, v, c0, c1);
        halfwave_run_sum2(p.ray, v, c2, c3);
        if (last) {
          float* dst = a.dh_appear + 4 * p.ray;
          atomicAdd(dst, c0);
          atomicAdd(dst + 1, c1);
          atomicAdd(dst + 2, c2);
          atomicAdd(dst + 3, c3);
        }
      }
      // ---- density branch: sigma = softplus(raw) -> d raw = d sigma * (1 - exp(-sigma))
      const float draw = gs * (1.0f - nsim_fast_exp(-sg));
      float da[32], whv[32];
#pragma unroll
      for (int k = 0; k < 32; ++k) {
        whv[k] = draw * a1[k];
        da[k] = a1[k] > 0.f ? draw * nvec(W, L, NV_DWH, hi, k) : 0.f;
      }
      rowsum_acc<PREC, 2, PRIV>(stA, whv, accum + A_DWH, 64);
      {
        float v = (hi == 0) ? draw : 0.f;
        v = wave_sum(v);
        if (lane == 0 && v != 0.f) {
          if constexpr (PRIV) accum[A_BD] = accum[A_BD] + v;
          else atomicAdd(&accum[A_BD], v);
        }
      }
      dw_product<PREC, 2, 1, PRIV>(stA, stB, da, h, accum + A_D1, 32, 64, 32, accum + A_DB1);
      float dh[16];
      dense<PREC, 1, 2>(dh, WM + L.mat[N_D1T], da, true);
      if (p.valid && a.dh_pl) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
#pragma unroll
          for (int b = 0; b < 2; ++b) {
            const int l = 4 * q + 2 * hi + b;
            if (l >= a.lotd.num_levels) continue;      // (the scatter reads the pyramid's own levels only)
            float* dp = a.dh_pl + ((int64_t)l * a.S + s) * 2;
            dp[0] = dh[4 * q + 2 * b] + din[4 * q + 2 * b];
            dp[1] = dh[4 * q + 2 * b + 1] + din[4 * q + 2 * b + 1];
          }
        }
      }
    }
  }
  if constexpr (BWD) {
    __syncthreads();
    const int F = a.F, K1 = a.F + 20;
    for (int i = threadIdx.x; i < A_TOTAL; i += blockDim.x) {
      float v;
      if constexpr (PRIV) {
        constexpr int ACC_FLOATS = ((A_TOTAL * 4 + 15) & ~15) / 4;
        const float* a0 = reinterpret_cast<const float*>(smem + wbytes);
        v = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) v += a0[w * ACC_FLOATS + i];
      } else {
        v = accum[i];
      }
      if (v == 0.f) continue;
      float* dst = nullptr;
      if (i < A_DWH) {
        const int row = i >> 5, col = i & 31;
        if (col < F) dst = a.dden_w + row * F + col;
      } else if (i < A_DB1) dst = a.dden_w + 64 * F + (i - A_DWH);
      else if (i < A_BD) dst = a.dden_b + (i - A_DB1);
      else if (i < A_Q1) dst = (i == A_BD) ? a.dden_b + 64 : nullptr;
      else if (i < A_Q2) {
        const int row = (i - A_Q1) >> 6, c = q1_col((i - A_Q1) & 63, F);
        if (c >= 0) dst = a.drad_w + row * K1 + c;
      } else if (i < A_Q3) dst = a.drad_w + 64 * K1 + (i - A_Q2);
      else if (i < A_RB1) dst = a.drad_w + 64 * K1 + 4096 + (i - A_Q3);
      else if (i < A_RB2) dst = a.drad_b + (i - A_RB1);
      else if (i < A_RB3) dst = a.drad_b + 64 + (i - A_RB2);
      else dst = (i - A_RB3 < 3) ? a.drad_b + 128 + (i - A_RB3) : nullptr;
      if (dst) atomicAdd(dst, v);
    }
  }
}

// ----------------------------------------------------------------------------------------- 4-D level-major gather
// The forward's table reads as their own launch, in the form of field.hip's k_lotd_gather_lm: every wave owns
// G4_PTS x 64 shell points and walks the levels dealt to ITS XCD (block b runs on XCD b % 8 -- used for speed only), so
// at any moment an XCD streams one or two tables (<= 2 MB each at T = 2^19) through its 4 MB L2 instead of all 16-32 MB
// of the pyramid at once, with G4_PTS x 16 independent 4-byte loads in flight per lane.  The 64 lanes are consecutive
// shells of one ray: on the coarse levels they share cells (same lines: coalesced by the texture unit), the fine hashed
// levels cost one line per x-pair.  Output: the f32 planes h [16][S][2] the decoders (forward AND backward) read.
#ifndef G4_PTS
#define G4_PTS 2
#endif
struct Gather4Args {
  Lotd4Dev lotd;
  const f16* grid;
  const float* u4;
  int64_t S;
  float* h_pl;
  signed char n[8], lv[8][D4_MAX_LEVELS], half[8][D4_MAX_LEVELS];
};

__global__ void __launch_bounds__(64) k_lotd4_gather_lm(Gather4Args a) {
  const int lane = nsim_lane();
  const int xcd = (int)(blockIdx.x & 7u);
  const int64_t s0 = (int64_t)(blockIdx.x >> 3) * (64 * G4_PTS) + lane;
  float u[G4_PTS][4];
#pragma unroll
  for (int q = 0; q < G4_PTS; ++q) {
    const int64_t s = s0 + 64 * q;
#pragma unroll
    for (int c = 0; c < 4; ++c) u[q][c] = s < a.S ? a.u4[4 * s + c] : 0.f;
  }
  const bool second_half = (blockIdx.x >> 3) >= ((gridDim.x >> 3) + 1) / 2;
  const int nl = a.n[xcd];
#pragma unroll 1
  for (int k = 0; k < nl; ++k) {
    const int l = a.lv[xcd][k];
    const int hf = a.half[xcd][k];
    if ((hf == 1 && second_half) || (hf == 2 && !second_half)) continue;
    const int Rx = a.lotd.res_xyz[l], Ry = a.lotd.res_y[l], Rz = a.lotd.res_z[l], Rw = a.lotd.res_w[l];
    const int type = a.lotd.type[l];
    const uint32_t T = a.lotd.size[l];
    const int64_t off = a.lotd.offset[l];
    float f0[G4_PTS], f1[G4_PTS];
#pragma unroll
    for (int q = 0; q < G4_PTS; ++q) {
      const Cell4 c = lotd4_cell(u[q], Rx, Ry, Rz, Rw);
      f0[q] = f1[q] = 0.f;
      const int pm4 = lotd4_slot_mask(c);
#pragma unroll
      for (int slot = 0; slot < 16; ++slot) {
        const int corner = slot ^ pm4;
        const float w = lotd4_weight(c, corner);
        const uint32_t idx = lotd4_index(c.c0[0] + (corner & 1), c.c0[1] + ((corner >> 1) & 1), c.c0[2] + ((corner >> 2) & 1),
                                         c.c0[3] + ((corner >> 3) & 1), Rx, Ry, Rz, type, T);
        float g0, g1;
        lotd4_load2(a.grid, off, idx, g0, g1);
        f0[q] = f0[q] + w * g0;
        f1[q] = f1[q] + w * g1;
      }
    }
#pragma unroll
    for (int q = 0; q < G4_PTS; ++q) {
      const int64_t s = s0 + 64 * q;
      if (s < a.S) {
        float* hp = a.h_pl + ((int64_t)l * a.S + s) * 2;
        hp[0] = f0[q];
        hp[1] = f1[q];
      }
    }
  }
}

// hashed levels cost 1, dense ones ~0.35 (their lines mostly hit L1): most expensive first onto the least loaded XCD,
// split into two halves of the point range when a whole level would overload it (field.hip deal_levels)
static void deal_levels4(const NsimLotd4Meta* m, Gather4Args& a) {
  const int NL = m->num_levels;
  float cost[D4_MAX_LEVELS], load[8] = {0, 0, 0, 0, 0, 0, 0, 0}, total = 0.f;
  bool used[D4_MAX_LEVELS] = {false};
  for (int l = 0; l < NL; ++l) {
    cost[l] = m->type[l] == NSIM_LOTD_HASH ? 1.0f : 0.35f;
    total += cost[l];
  }
  const float limit = total / 8.0f * 1.08f;
  for (int xc = 0; xc < 8; ++xc) a.n[xc] = 0;
  auto least = [&]() {
    int tx = 0;
    for (int xc = 1; xc < 8; ++xc)
      if (load[xc] < load[tx]) tx = xc;
    return tx;
  };
  auto put = [&](int xc, int l, int hf, float c) {
    a.lv[xc][(int)a.n[xc]] = (signed char)l;
    a.half[xc][(int)a.n[xc]++] = (signed char)hf;
    load[xc] += c;
  };
  for (int it = 0; it < NL; ++it) {
    int best = -1;
    for (int l = 0; l < NL; ++l)
      if (!used[l] && (best < 0 || cost[l] > cost[best] || (cost[l] == cost[best] && m->size[l] > m->size[best]))) best = l;
    used[best] = true;
    const int x0 = least();
    if (load[x0] + cost[best] <= limit || load[x0] == 0.f) {
      put(x0, best, 0, cost[best]);
    } else {
      put(x0, best, 1, 0.5f * cost[best]);
      put(least(), best, 2, 0.5f * cost[best]);
    }
  }
}

// ----------------------------------------------------------------------------------------- 4-D scatter
// dgrid[level][vertex][f] += w_c * dh[f]; level-major, one lane per sample, x-adjacent corner pairs issued
// quad-transposed so {x0.f0,x0.f1,x1.f0,x1.f1} leave as one request (see field.hip / tools/atomic_bench2.hip).
struct Scatter4Args {
  Lotd4Dev lotd;
  const float* u4;
  const uint8_t* valid;
  int64_t S;
  const float* dh_pl;
  float* dgrid;
  int dedup_max_rw;     // 1 << 30: every level is folded (3.62 -> 1.73 ms per 0.52 M shell points; levels with Rw <= 16 / 64 only: 2.07 / 1.76)
  int parity_slots;     // 1.  Both stay run-time values: as constants the kernel needs 87-88 instead of 86 registers
};

// Issue I of the quad transposition carries the 16 consecutive shells 16 I + q (not the shells 4q + I); with the parity slots
// the street step's 4-D scatter went 2.15 -> 1.99 (parity slots) -> 1.74 ms (+ consecutive issue), see k_lotd_scatter in field.hip
__global__ void __launch_bounds__(256) k_lotd4_scatter(Scatter4Args a) {
  const int lane = nsim_lane();
  const int l = blockIdx.y;
  const int Rx = a.lotd.res_xyz[l], Ry = a.lotd.res_y[l], Rz = a.lotd.res_z[l], Rw = a.lotd.res_w[l];
  // K = 64 shells per ray: a wave holds consecutive shells of (mostly) ONE ray.  Far shells converge to a fixed
  // (x/r) direction and step through few 1/r cells on the coarser levels, so runs of lanes hit the same vertex:
  // collapse them (run heads by ballot, segmented shuffle scan) before the atomics -- the kernel is bound by the
  // atomic request rate, the extra shuffles are free.
  const bool dedup = Rw <= a.dedup_max_rw;
  const int rq = lane & 3;
  float* base = a.dgrid + a.lotd.offset[l];
  const int64_t nchunks = (a.S + 63) / 64;
  const int64_t wstride = (int64_t)gridDim.x * 4;
  for (int64_t chunk = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); chunk < nchunks; chunk += wstride) {
    const int64_t s = chunk * 64 + lane;
    const bool valid = s < a.S && a.valid[s];
    float u[4] = {0.f, 0.f, 0.f, 0.f}, dh0 = 0.f, dh1 = 0.f;
    if (valid) {
#pragma unroll
      for (int c = 0; c < 4; ++c) u[c] = a.u4[4 * s + c];
      const float* dp = a.dh_pl + ((int64_t)l * a.S + s) * 2;
      dh0 = dp[0];
      dh1 = dp[1];
    }
    const Cell4 c = lotd4_cell(u, Rx, Ry, Rz, Rw);
    const int pmask = a.parity_slots ? ((c.c0[0] & 1) | ((c.c0[1] & 1) << 1) | ((c.c0[2] & 1) << 2) | ((c.c0[3] & 1) << 3)) : 0;
#pragma unroll
    for (int yzw = 0; yzw < 8; ++yzw) {
      uint32_t idx[2];
      float v0[2], v1[2];
      int emit[2];
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        // parity slots (see k_lotd_scatter, field.hip): slot (dx, yzw) holds the vertex with those coordinate parities, so the
        // vertices two consecutive shells' cells share sit in the same slot and the run merge below folds them
        const int corner = (dx | (yzw << 1)) ^ pmask;
        const float w = lotd4_weight(c, corner);
        idx[dx] = lotd4_index(c.c0[0] + (corner & 1), c.c0[1] + ((corner >> 1) & 1), c.c0[2] + ((corner >> 2) & 1), c.c0[3] + (corner >> 3), Rx,
                              Ry, Rz, a.lotd.type[l], a.lotd.size[l]);
        v0[dx] = w * dh0;
        v1[dx] = w * dh1;
        emit[dx] = valid;
        if (dedup) {
          const uint32_t key = valid ? idx[dx] : 0xffffffffu;
          const uint32_t pk = wave_shfl(key, lane - 1);
          const unsigned long long heads = wave_ballot(lane == 0 || pk != key);
          const unsigned long long below = heads & ((2ull << lane) - 1ull);
          const int run_start = 63 - __builtin_clzll(below);
#pragma unroll
          for (int d = 1; d < 64; d <<= 1) {
            // (wave-uniform early exit: no run of this slot reaches d lanes back -- at the fine levels runs are 1-3 lanes long
            // and two of the six rounds do all the work)
            if (!wave_ballot(lane - d >= run_start)) break;
            const float o0 = wave_shfl(v0[dx], lane - d), o1 = wave_shfl(v1[dx], lane - d);
            if (lane - d >= run_start) {
              v0[dx] += o0;
              v1[dx] += o1;
            }
          }
          emit[dx] = valid && (lane == 63 || ((heads >> (lane + 1)) & 1ull));   // last lane of the run
        }
      }
      const uint32_t k0 = emit[0] ? idx[0] : 0xffffffffu, k1 = emit[1] ? idx[1] : 0xffffffffu;
#pragma unroll
      for (int I = 0; I < 4; ++I) {
        const int src = 16 * I + (lane >> 2);
        const uint32_t i0 = wave_shfl(k0, src), i1 = wave_shfl(k1, src);
        const float a0 = wave_shfl(v0[0], src), a1 = wave_shfl(v1[0], src);
        const float b0 = wave_shfl(v0[1], src), b1 = wave_shfl(v1[1], src);
        const uint32_t ii = rq < 2 ? i0 : i1;
        const float vv = rq == 0 ? a0 : (rq == 1 ? a1 : (rq == 2 ? b0 : b1));
        if (ii != 0xffffffffu) atomicAdd(base + 2 * (int64_t)ii + (rq & 1), vv);
      }
    }
  }
}

// ================================================================================== close-range NGP NeRF
// ``LoTDNeRFModel`` (app/models/single/nerf.py:33-143 LoTDNeRFObj / LoTDNeRFStreet; config
// code_single/configs/waymo/ngp_withlidar.230814.yaml:100-158): 3-D LoTD features (gathered level-major by field.hip) ->
// density decoder [h (F <= 32) | x_n (3)] -> 64 (relu) -> 32 (linear): output 0 = raw density (sigma = exp(raw - 1)),
// outputs 1..31 = geometry feature -> radiance decoder [geo (31) | SH-4 (16) | h_appear (0 | 4)] -> 64 -> 64 -> 3 (sigmoid).
// Same 32-point register-resident transposed-MFMA scheme as k_nerf above.  The three-position block of the first density
// layer is a rank-3 update on the VALU in f32 (forward) and a 3-column weight-gradient product (backward): it never
// enters an MFMA chunk, so 2 num_levels = 32 needs no second 32-input chunk and x_n is not rounded to fp16.
#include "occ_dev.h"

enum { G_D1 = 0, G_D2, G_Q1, G_Q2, G_Q3, G_D1T, G_D2T, G_Q3T, G_Q2T, G_Q1T, G_MCOUNT };
enum { GV_DB1 = 0, GV_DX0, GV_DX1, GV_DX2, GV_DB2, GV_RB1, GV_RB2, GV_RB3, GV_COUNT };
static_assert(G_MCOUNT <= PACK_MAX_MATS, "PackShape holds the NGP model's matrices");
static const int kGUo[G_MCOUNT] = {64, 32, 64, 64, 32, 32, 64, 64, 64, 64};
static const int kGUi[G_MCOUNT] = {32, 64, 64, 64, 64, 64, 32, 32, 64, 64};

// pack: [vectors | forward matrices | transposed matrices] -- the forward stages [0, fwd_end) into LDS, the fp16 backward
// the vectors alone
struct NgpLayout {
  int64_t mat[G_MCOUNT], vec[GV_COUNT], fwd_end, total;
  int elt;
};
static inline NgpLayout ngp_layout(int precision) {
  NgpLayout L;
  L.elt = precision == 0 ? 2 : 4;
  int64_t off = 0;
  for (int v = 0; v < GV_COUNT; ++v) {
    L.vec[v] = off;
    off += 64 * 4;
  }
  L.fwd_end = 0;
  for (int m = 0; m < G_MCOUNT; ++m) {
    L.mat[m] = off;
    off += (int64_t)kGUo[m] * kGUi[m] * L.elt;
    if (m == G_Q3) L.fwd_end = off;
  }
  L.total = off;
  return L;
}

// radiance input slot (0..63) -> column of the [64 x (31 + 16 + NA)] first radiance layer, or -1.  Slot 0 is the raw
// density (not an input of the radiance net), slots 1..31 the geometry feature, 32..47 SH-4, 48..51 the appearance code.
__host__ __device__ inline int ngp_q1_col(int slot, int NA) {
  if (slot < 1) return -1;
  if (slot < 32) return slot - 1;
  if (slot < 48) return 31 + (slot - 32);
  if (slot < 52) return NA == 4 ? 47 + (slot - 48) : -1;
  return -1;
}

__device__ __forceinline__ float ngp_src(int mat, int row, int col, int F, int NA, const float* den_w, const float* rad_w) {
  const int FI = F + 3, K1 = 47 + NA;
  const int d2 = 64 * FI, q2 = 64 * K1, q3 = q2 + 4096;
  switch (mat) {
    case G_D1: return col < F ? den_w[row * FI + col] : 0.f;
    case G_D1T: return row < F ? den_w[col * FI + row] : 0.f;
    case G_D2: return den_w[d2 + row * 64 + col];
    case G_D2T: return den_w[d2 + col * 64 + row];
    case G_Q1: { const int c = ngp_q1_col(col, NA); return c >= 0 ? rad_w[row * K1 + c] : 0.f; }
    case G_Q1T: { const int c = ngp_q1_col(row, NA); return c >= 0 ? rad_w[col * K1 + c] : 0.f; }
    case G_Q2: return rad_w[q2 + row * 64 + col];
    case G_Q2T: return rad_w[q2 + col * 64 + row];
    case G_Q3: return row < 3 ? rad_w[q3 + row * 64 + col] : 0.f;
    case G_Q3T: return col < 3 ? rad_w[q3 + col * 64 + row] : 0.f;
  }
  return 0.f;
}

__global__ void __launch_bounds__(256) k_ngp_pack(NgpLayout L, PackShape sh, int F, int NA, const float* __restrict__ den_w,
                                                   const float* __restrict__ den_b, const float* __restrict__ rad_w,
                                                   const float* __restrict__ rad_b, char* __restrict__ wpack) {
  int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const auto src = [&](int m, int row, int col) { return ngp_src(m, row, col, F, NA, den_w, rad_w); };
  if (pack_matrices(sh, G_MCOUNT, L.mat, pack_form(L.elt), wpack, tid, src)) return;
  if (tid < (int64_t)GV_COUNT * 64) {
    const int v = (int)(tid >> 6), k = (int)(tid & 63), u = vec_unit(k, 64);
    const int FI = F + 3;
    float val = 0.f;
    switch (v) {
      case GV_DB1: val = den_b[u]; break;
      case GV_DX0: val = den_w[u * FI + F]; break;
      case GV_DX1: val = den_w[u * FI + F + 1]; break;
      case GV_DX2: val = den_w[u * FI + F + 2]; break;
      case GV_DB2: val = u < 32 ? den_b[64 + u] : 0.f; break;
      case GV_RB1: val = rad_b[u]; break;
      case GV_RB2: val = rad_b[64 + u]; break;
      case GV_RB3: val = u < 3 ? rad_b[128 + u] : 0.f; break;
    }
    ((float*)(wpack + L.vec[v]))[k] = val;
  }
}

struct NgpArgs {
  NgpLayout lay;
  int F, NL, n_active, NA;                // features = 2 NL; levels >= n_active are masked (hardmask annealing)
  float xs[3], xb[3];                     // u = x * xs + xb in [0,1]; x_n = 2 u - 1
  const char* wpack;
  const float *x, *rays_o, *rays_d, *t;   // points: x [S,3], or rays_o[ridx] + t rays_d[ridx]
  const int64_t* ridx;
  const float* h_appear;                  // [R,4] or NULL
  int64_t S, PS;                          // points; pitch of h_pl
  float step;                             // alpha = 1 - exp(-sigma step)
  const float* h_pl;                      // [16][PS][2] gathered features
  float *sigma, *alpha, *rgb;             // forward outputs (rgb NULL: density only)
  const float *sigma_fwd, *rgb_fwd;       // saved forward outputs
  const float *dsigma, *dalpha, *drgb;    // upstream (each may be NULL)
  float* dh_pl;                           // [16][S][2] hand-off to nsim_lotd_scatter (may be NULL)
  float* dst[4];                          // dden_w, dden_b, drad_w, drad_b -- or replica 0 of the registered scratch
  int64_t rep_stride;                     // floats between replicas (workgroup b adds into replica b & rep_mask)
  int rep_mask;
  float* dh_appear;
  float *dx, *dv;                         // POSE: per-sample gradients to the position / the un-normalised ray direction
};

#define NGP_WAVES 4
#define NGP_WAVES_BWD 2       // the weight-gradient accumulators are 51.6 KB per private copy: two fit next to the staging

__device__ __forceinline__ float ngp_vec(const char* WV, const NgpLayout& L, int v, int hi, int k) {
  return reinterpret_cast<const float*>(WV + L.vec[v])[hi * 32 + k];
}

struct NgpPoint {
  int64_t s, ray;
  bool valid;
  float xn[3], vd[3], ha[4];
};
__device__ __forceinline__ NgpPoint ngp_point(const NgpArgs& a, int64_t tile, int j, bool with_rad) {
  NgpPoint p;
  p.s = tile * 32 + j;
  p.valid = p.s < a.S;
  p.ray = 0;
  p.xn[0] = p.xn[1] = p.xn[2] = 0.f;
  p.vd[0] = p.vd[1] = 0.f;
  p.vd[2] = 1.f;
  p.ha[0] = p.ha[1] = p.ha[2] = p.ha[3] = 0.f;
  if (p.valid) {
    p.ray = a.ridx ? a.ridx[p.s] : p.s;
    float xx[3];
    if (a.x) {
#pragma unroll
      for (int c = 0; c < 3; ++c) xx[c] = a.x[3 * p.s + c];
    } else {
      const float tt = a.t[p.s];
#pragma unroll
      for (int c = 0; c < 3; ++c) xx[c] = a.rays_o[3 * p.ray + c] + tt * a.rays_d[3 * p.ray + c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) p.xn[c] = 2.0f * (xx[c] * a.xs[c] + a.xb[c]) - 1.0f;
    if (with_rad) {
      float d[3], n2 = 0.f;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        d[c] = a.rays_d[3 * p.ray + c];
        n2 = n2 + d[c] * d[c];
      }
      const float inv = n2 > 0.f ? 1.0f / sqrtf(n2) : 0.f;
#pragma unroll
      for (int c = 0; c < 3; ++c) p.vd[c] = d[c] * inv;
      if (a.h_appear && a.NA == 4) {
#pragma unroll
        for (int c = 0; c < 4; ++c) p.ha[c] = a.h_appear[4 * p.ray + c];
      }
    }
  }
  return p;
}

// BWD = 0: sigma / alpha / rgb.  BWD = 1: recomputes the activations from the saved feature planes and accumulates the
// weight gradients (per-wave private LDS accumulators in fp16 mode, as k_nerf), dh planes, dh_appear.
// POSE (backward only; pose refinement, the rays or points carry gradients): also dx [S,3], the first density layer's
// direct position input pulled back to object coordinates (W1[:, F:]^T da1 . 2 xs -- the table's share is added by
// k_lotd_dx_lm from the dh planes), and dv [S,3] (NULL without a colour gradient), the SH-4 slots of the radiance input
// gradient through sh4_grad and the normalisation n = d / |d|: dv = (I - n n^T) g / |d|.
template <int PREC, int BWD, bool POSE = false>
__global__ void __launch_bounds__(64 * (BWD ? NGP_WAVES_BWD : NGP_WAVES)) k_ngp(NgpArgs a) {
  static_assert(!POSE || BWD, "the ray gradients are outputs of the backward");
  NSIM_DYN_SMEM(smem);
  constexpr bool PRIV = (PREC == 0 && BWD);
  constexpr int NW = BWD ? NGP_WAVES_BWD : NGP_WAVES;
  const int lane = nsim_lane(), j = lane & 31, hi = lane >> 5;
  const int wave = (int)(threadIdx.x >> 6);
  const NgpLayout& L = a.lay;
  const bool with_rad = BWD ? (a.drgb != nullptr) : (a.rgb != nullptr);
  // ---- weights: fp16 stages the vectors (+ the forward matrices in the forward) into LDS; f32 reads the pack from L2
  const char* W = a.wpack;        // base the vectors AND matrices are addressed from
  const char* WM = a.wpack;
  int wbytes = 0;
  if constexpr (PREC == 0) {
    const int64_t nbytes = BWD ? L.mat[0] : L.fwd_end;
    const int n16 = (int)((nbytes + 15) >> 4);
    const f16x8* src = reinterpret_cast<const f16x8*>(a.wpack);
    f16x8* dst = reinterpret_cast<f16x8*>(smem);
    for (int i = threadIdx.x; i < n16; i += blockDim.x) dst[i] = src[i];
    wbytes = n16 << 4;
    __syncthreads();
    W = smem;
    if constexpr (!BWD) WM = smem;
  }
  constexpr int A_D1 = 0, A_DX = 2048, A_DB1 = A_DX + 192, A_D2 = A_DB1 + 64, A_DB2 = A_D2 + 2048, A_Q1 = A_DB2 + 32,
                A_Q2 = A_Q1 + 4096, A_Q3 = A_Q2 + 4096, A_RB1 = A_Q3 + 192, A_RB2 = A_RB1 + 64, A_RB3 = A_RB2 + 64,
                A_TOTAL = A_RB3 + 4;
  constexpr int ACC_BYTES = (A_TOTAL * 4 + 15) & ~15;
  float* accum = nullptr;
  char* stA = nullptr;
  char* stB = nullptr;
  if constexpr (BWD) {
    accum = reinterpret_cast<float*>(smem + wbytes + (PRIV ? wave * ACC_BYTES : 0));
    char* stbase = smem + wbytes + (PRIV ? NW : 1) * ACC_BYTES + wave * stage_bytes_per_wave<PREC>();
    stA = stbase;
    stB = stbase + stage_bytes_per_wave<PREC>() / 2;
    if constexpr (PRIV) {
      for (int i = lane; i < A_TOTAL; i += 64) accum[i] = 0.f;
    } else {
      for (int i = threadIdx.x; i < A_TOTAL; i += blockDim.x) accum[i] = 0.f;
    }
    __syncthreads();
  }
  const int64_t ntiles = (a.S + 31) / 32;
  const int64_t wstride = (int64_t)gridDim.x * NW;
  for (int64_t tile = (int64_t)blockIdx.x * NW + wave; tile < ntiles; tile += wstride) {
    const NgpPoint p = ngp_point(a, tile, j, with_rad);
    const int64_t s = p.s;
    // -------------------------------------------------------------- features from the level-major planes
    float h[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int l = 4 * q + 2 * hi + b;
        float f0 = 0.f, f1 = 0.f;
        if (p.valid && l < a.n_active) {      // (masked and padding levels: zero features, their planes are never read)
          const float* hp = a.h_pl + ((int64_t)l * a.PS + s) * 2;
          f0 = hp[0];
          f1 = hp[1];
        }
        h[4 * q + 2 * b] = f0;
        h[4 * q + 2 * b + 1] = f1;
      }
    }
    // -------------------------------------------------------------- density decoder
    float a1[32];
    dense<PREC, 2, 1>(a1, WM + L.mat[G_D1], h, true);
#pragma unroll
    for (int k = 0; k < 32; ++k) {
      float z = a1[k] + ngp_vec(W, L, GV_DB1, hi, k);
      z = z + ngp_vec(W, L, GV_DX0, hi, k) * p.xn[0];
      z = z + ngp_vec(W, L, GV_DX1, hi, k) * p.xn[1];
      z = z + ngp_vec(W, L, GV_DX2, hi, k) * p.xn[2];
      a1[k] = fmaxf(z, 0.f);
    }
    float rin[32];      // [0,16): density outputs (slot 0 = raw, zeroed: not a radiance input), [16,32): SH / appearance
    {
      float o16[16];
      dense<PREC, 1, 2>(o16, WM + L.mat[G_D2], a1, true);
#pragma unroll
      for (int r = 0; r < 16; ++r) rin[r] = o16[r] + ngp_vec(W, L, GV_DB2, hi, r);
    }
    if constexpr (!BWD) {
      const float raw = wave_shfl(rin[0], j);       // unit 0 lives in register 0 of the lower half-wave
      const float sg = expf(raw - 1.0f);
      if (p.valid && hi == 0) {
        a.sigma[s] = sg;
        if (a.alpha) a.alpha[s] = 1.0f - expf(-sg * a.step);
      }
    }
    if (hi == 0) rin[0] = 0.f;
    float r1[32], r2[32];
    if (with_rad) {
      nerf_rin_tail(rin, p.vd, p.ha, hi);
      dense<PREC, 2, 2>(r1, WM + L.mat[G_Q1], rin, true);
#pragma unroll
      for (int k = 0; k < 32; ++k) r1[k] = fmaxf(r1[k] + ngp_vec(W, L, GV_RB1, hi, k), 0.f);
      dense<PREC, 2, 2>(r2, WM + L.mat[G_Q2], r1, false);
#pragma unroll
      for (int k = 0; k < 32; ++k) r2[k] = fmaxf(r2[k] + ngp_vec(W, L, GV_RB2, hi, k), 0.f);
    }
    if constexpr (!BWD) {
      if (with_rad) {
        float o3[16];
        dense<PREC, 1, 2>(o3, WM + L.mat[G_Q3], r2, false);
        if (p.valid && hi == 0) {
#pragma unroll
          for (int c = 0; c < 3; ++c) a.rgb[3 * s + c] = 1.0f / (1.0f + nsim_fast_exp(-(o3[c] + ngp_vec(W, L, GV_RB3, hi, c))));
        }
      }
    }
    if constexpr (BWD) {
      float dO[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) dO[r] = 0.f;
      if (with_rad) {
        float gr[3] = {0.f, 0.f, 0.f}, rgbv[3] = {0.f, 0.f, 0.f};
        if (p.valid) {
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            gr[c] = a.drgb[3 * s + c];
            rgbv[c] = a.rgb_fwd[3 * s + c];
          }
        }
        float dout[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) dout[r] = 0.f;
        if (hi == 0) {
#pragma unroll
          for (int c = 0; c < 3; ++c) dout[c] = gr[c] * rgbv[c] * (1.0f - rgbv[c]);
        }
        dw_product<PREC, 1, 2, PRIV>(stA, stB, dout, r2, accum + A_Q3, 64, 3, 64, accum + A_RB3);
        float dr2[32];
        dense<PREC, 2, 1>(dr2, WM + L.mat[G_Q3T], dout, true);
#pragma unroll
        for (int k = 0; k < 32; ++k) dr2[k] = r2[k] > 0.f ? dr2[k] : 0.f;
        dw_product<PREC, 2, 2, PRIV>(stA, stB, dr2, r1, accum + A_Q2, 64, 64, 64, accum + A_RB2);
        float dr1[32];
        dense<PREC, 2, 2>(dr1, WM + L.mat[G_Q2T], dr2, true);
#pragma unroll
        for (int k = 0; k < 32; ++k) dr1[k] = r1[k] > 0.f ? dr1[k] : 0.f;
        dw_product<PREC, 2, 2, PRIV>(stA, stB, dr1, rin, accum + A_Q1, 64, 64, 64, accum + A_RB1);
        float din[32];
        dense<PREC, 2, 2>(din, WM + L.mat[G_Q1T], dr1, true);
        // appearance slots 48..51 = second M-tile local 16..19 (lower half-wave, registers 8..11); one atomic per ray and
        // channel: the samples of a ray are neighbouring lanes
        if (a.dh_appear && a.NA == 4) {
          float c0 = din[16 + 8], c1 = din[16 + 9], c2 = din[16 + 10], c3 = din[16 + 11];
          const bool v = p.valid && hi == 0;
          const bool last = halfwave_run_sum2(p.ray, v, c0, c1);
          halfwave_run_sum2(p.ray, v, c2, c3);
          if (last) {
            float* dst = a.dh_appear + 4 * p.ray;
            atomicAdd(dst, c0);
            atomicAdd(dst + 1, c1);
            atomicAdd(dst + 2, c2);
            atomicAdd(dst + 3, c3);
          }
        }
        if constexpr (POSE) {
          if (a.dv) {     // SH slot k of the second M-tile: half-wave (k >> 2) & 1, register (k & 3) + 4 (k >> 3)
            float gsh[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) {
              const float v = (hi == ((k >> 2) & 1)) ? din[16 + (k & 3) + 4 * (k >> 3)] : 0.f;
              gsh[k] = v + wave_shfl_xor(v, 32);
            }
            float gv[3];
            sh4_grad(p.vd, gsh, gv);
            if (p.valid && hi == 0) {
              float n2 = 0.f;
#pragma unroll
              for (int c = 0; c < 3; ++c) {
                const float dc = a.rays_d[3 * p.ray + c];
                n2 = n2 + dc * dc;
              }
              const float inv = n2 > 0.f ? 1.0f / sqrtf(n2) : 0.f;
              const float ng = p.vd[0] * gv[0] + p.vd[1] * gv[1] + p.vd[2] * gv[2];
#pragma unroll
              for (int c = 0; c < 3; ++c) a.dv[3 * s + c] = (gv[c] - p.vd[c] * ng) * inv;
            }
          }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) dO[r] = din[r];      // geometry feature (slot 0: the packed row is zero)
      }
      // ---- sigma = exp(raw - 1): d raw = (d sigma + d alpha step exp(-sigma step)) exp(min(raw - 1, 15))
      if (hi == 0) {
        float g = 0.f;
        if (p.valid) {
          const float sg = a.sigma_fwd[s];
          if (a.dsigma) g = g + a.dsigma[s];
          if (a.dalpha) g = g + a.dalpha[s] * (a.step * expf(-sg * a.step));
          g = g * fminf(sg, 3269017.3724721107f);       // exp(15)
        }
        dO[0] = g;
      }
      dw_product<PREC, 1, 2, PRIV>(stA, stB, dO, a1, accum + A_D2, 64, 32, 64, accum + A_DB2);
      float da[32];
      dense<PREC, 2, 1>(da, WM + L.mat[G_D2T], dO, true);
#pragma unroll
      for (int k = 0; k < 32; ++k) da[k] = a1[k] > 0.f ? da[k] : 0.f;
      dw_product<PREC, 2, 1, PRIV>(stA, stB, da, h, accum + A_D1, 32, 64, 32, accum + A_DB1);
      {
        float xt[16];     // the position block as an input tile: units 0..2 = registers 0..2 of the lower half-wave
#pragma unroll
        for (int r = 0; r < 16; ++r) xt[r] = (hi == 0 && r < 3) ? p.xn[r < 3 ? r : 0] : 0.f;
        dw_product<PREC, 2, 1, PRIV>(stA, stB, da, xt, accum + A_DX, 3, 64, 3, nullptr);
      }
      if constexpr (POSE) {     // x_n = 2 (x xs + xb) - 1: d x_c = 2 xs_c sum_u W1[u][F + c] da[u]
        float gx[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 32; ++k) {
          gx[0] = gx[0] + ngp_vec(W, L, GV_DX0, hi, k) * da[k];
          gx[1] = gx[1] + ngp_vec(W, L, GV_DX1, hi, k) * da[k];
          gx[2] = gx[2] + ngp_vec(W, L, GV_DX2, hi, k) * da[k];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) gx[c] = gx[c] + wave_shfl_xor(gx[c], 32);
        if (p.valid && hi == 0) {
#pragma unroll
          for (int c = 0; c < 3; ++c) a.dx[3 * s + c] = gx[c] * (2.0f * a.xs[c]);
        }
      }
      if (a.dh_pl) {
        float dh[16];
        dense<PREC, 1, 2>(dh, WM + L.mat[G_D1T], da, true);
        if (p.valid) {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
#pragma unroll
            for (int b = 0; b < 2; ++b) {
              const int l = 4 * q + 2 * hi + b;
              if (l >= a.NL) continue;                      // (the scatter reads the pyramid's own levels only)
              const bool on = l < a.n_active;
              float* dp = a.dh_pl + ((int64_t)l * a.S + s) * 2;
              dp[0] = on ? dh[4 * q + 2 * b] : 0.f;
              dp[1] = on ? dh[4 * q + 2 * b + 1] : 0.f;
            }
          }
        }
      }
    }
  }
  if constexpr (BWD) {
    __syncthreads();
    const int F = a.F, FI = a.F + 3, K1 = 47 + a.NA;
    const int64_t rep = (int64_t)(blockIdx.x & (unsigned)a.rep_mask) * a.rep_stride;
    for (int i = threadIdx.x; i < A_TOTAL; i += blockDim.x) {
      float v;
      if constexpr (PRIV) {
        constexpr int ACC_FLOATS = ACC_BYTES / 4;
        const float* a0 = reinterpret_cast<const float*>(smem + wbytes);
        v = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) v += a0[w * ACC_FLOATS + i];
      } else {
        v = accum[i];
      }
      if (v == 0.f) continue;
      int d = -1;
      int64_t off = 0;
      if (i < A_DX) {
        const int row = i >> 5, col = i & 31;
        if (col < F) { d = 0; off = row * FI + col; }
      } else if (i < A_DB1) {
        const int k = i - A_DX;
        d = 0; off = (k / 3) * FI + F + (k % 3);
      } else if (i < A_D2) { d = 1; off = i - A_DB1; }
      else if (i < A_DB2) { d = 0; off = 64 * FI + (i - A_D2); }
      else if (i < A_Q1) { d = 1; off = 64 + (i - A_DB2); }
      else if (i < A_Q2) {
        const int row = (i - A_Q1) >> 6, c = ngp_q1_col((i - A_Q1) & 63, a.NA);
        if (c >= 0) { d = 2; off = row * K1 + c; }
      } else if (i < A_Q3) { d = 2; off = 64 * K1 + (i - A_Q2); }
      else if (i < A_RB1) { d = 2; off = 64 * K1 + 4096 + (i - A_Q3); }
      else if (i < A_RB2) { d = 3; off = i - A_RB1; }
      else if (i < A_RB3) { d = 3; off = 64 + (i - A_RB2); }
      else if (i - A_RB3 < 3) { d = 3; off = 128 + (i - A_RB3); }
      if (d >= 0) atomicAdd(a.dst[d] + rep + off, v);
    }
  }
}

// ----------------------------------------------------------------------------------------- pose refinement
// The position gradient of the level-major 3-D gather (the LoTD counterpart of permuto.hip's k_permuto_dx_pts):
//   dx[s][c] = dx_add[s][c] + sum_{l < n_active} dscale_l,c sum_slot (d w_slot / d pos_c) (dh[l][s][0] g0 + dh[l][s][1] g1)
// with dh the planes [16][pitch][2] the decoder backward leaves for the scatter, (g0, g1) the fp16 table entry of the slot's
// vertex (lotd_dev.h: the parity enumeration of every gather) and dscale = xs (R - 1), so dx is in object coordinates.  The
// model saves no dh/dx planes in the forward (they are 6 floats per level and sample and only this launch would read them):
// the eight vertices are fetched again.  One lane per sample over all active levels: every dx row has one writer; masked
// levels touch neither their table nor their plane.
struct LotdDxArgs {
  LotdDev lotd;
  const f16* grid;
  const float *x, *rays_o, *rays_d, *t;
  const int64_t* ridx;
  int64_t S, PS;
  const float *dh_pl, *dx_add;
  float* dx;
};

__global__ void __launch_bounds__(256) k_lotd_dx_lm(LotdDxArgs a) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= a.S) return;
  float xx[3];
  if (a.x) {
    xx[0] = a.x[3 * s]; xx[1] = a.x[3 * s + 1]; xx[2] = a.x[3 * s + 2];
  } else {
    const int64_t ray = a.ridx[s];
    const float tt = a.t[s];
#pragma unroll
    for (int c = 0; c < 3; ++c) xx[c] = a.rays_o[3 * ray + c] + tt * a.rays_d[3 * ray + c];
  }
  const GridRef gref = grid_ref(a.grid);
  float acc[3] = {0.f, 0.f, 0.f};
  if (a.dx_add) {
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] = a.dx_add[3 * s + c];
  }
  for (int l = 0; l < a.lotd.n_active; ++l) {
    const LotdRes R = a.lotd.res[l];
    const int type = a.lotd.type[l];
    const uint32_t T = a.lotd.size[l], off = (uint32_t)a.lotd.offset[l];
    const LotdCell c = lotd_cell(xx, R, a.lotd);
    const LotdSlots SL = lotd_slots(c);
    const float* dp = a.dh_pl + ((int64_t)l * a.PS + s) * 2;
    const float d0 = dp[0], d1 = dp[1];
    float j[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int slot = 0; slot < 8; ++slot) {
      float w, dw[3], g0, g1;
      lotd_slot_w(SL, slot, w, dw);
      lotd_load2(gref, off + 2u * lotd_slot_index(SL, slot, R, type, T), g0, g1);
      const float v = d0 * g0 + d1 * g1;
#pragma unroll
      for (int c3 = 0; c3 < 3; ++c3) j[c3] = j[c3] + dw[c3] * v;
    }
#pragma unroll
    for (int c3 = 0; c3 < 3; ++c3) acc[c3] = acc[c3] + j[c3] * c.dscale[c3];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) a.dx[3 * s + c] = acc[c];
}

// ----------------------------------------------------------------------------------------- density occupancy
// ``accel_cfg{type: occ_grid}`` of a density field (ngp_withlidar.230814.yaml:138-152; no ``occ_val_fn_cfg``: the value IS
// the density): val[voxel(p)] = max(val[voxel(p)], sigma(p)).  sigma >= 0: the integer atomicMax on the bit pattern is
// exact (occ_dev.h: occ_max_wave).
__global__ void __launch_bounds__(256) k_occ_max_density(float* __restrict__ val, const float* __restrict__ x,
                                                          const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                                          const float* __restrict__ t, const int64_t* __restrict__ ridx,
                                                          const float* __restrict__ sigma, int64_t n, OccDev m) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool ok = i < n;
  float px = 0.f, py = 0.f, pz = 0.f, v = 0.f;
  if (ok) {
    if (x) {
      px = x[3 * i]; py = x[3 * i + 1]; pz = x[3 * i + 2];
    } else {
      const int64_t r = ridx[i];
      const float tt = t[i];
      px = rays_o[3 * r] + tt * rays_d[3 * r];
      py = rays_o[3 * r + 1] + tt * rays_d[3 * r + 1];
      pz = rays_o[3 * r + 2] + tt * rays_d[3 * r + 2];
    }
    v = fmaxf(sigma[i], 0.f);
    if (!(v == v)) v = 0.f;
  }
  occ_max_wave(val, m, ok, px, py, pz, v);
}

__global__ void __launch_bounds__(256) k_occ_scale(float* __restrict__ val, int64_t n, float decay) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) val[i] = val[i] * decay;
}

// partial sums of the value grid: block b -> part[b] (fixed grid, fixed order: the threshold is reproducible)
#define OCC_MEAN_BLOCKS 64
__global__ void __launch_bounds__(256) k_occ_partial_sum(const float* __restrict__ val, int64_t nvox, float* __restrict__ part) {
  __shared__ float sh[4];
  float s = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvox; i += (int64_t)gridDim.x * blockDim.x) s += val[i];
  s = wave_sum(s);
  if (nsim_lane() == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// thre = min(occ_thre, mean(val)) (``occ_thre_consider_mean``) from the partial sums; bits; thre_out[0] = the threshold used
__global__ void __launch_bounds__(256) k_occ_pack_bits_mean(const float* __restrict__ val, int64_t nvox, float occ_thre,
                                                             int consider_mean, const float* __restrict__ part,
                                                             uint32_t* __restrict__ bits, float* __restrict__ thre_out) {
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  float thre = occ_thre;
  if (consider_mean) {
    float s = 0.f;
    for (int b = 0; b < OCC_MEAN_BLOCKS; ++b) s += part[b];
    thre = fminf(occ_thre, s / (float)nvox);
  }
  if (w == 0 && thre_out) thre_out[0] = thre;
  const int64_t nwords = (nvox + 31) / 32;
  if (w >= nwords) return;
  uint32_t b = 0;
  for (int k = 0; k < 32; ++k) {
    const int64_t v = w * 32 + k;
    if (v < nvox && val[v] > thre) b |= (1u << k);
  }
  bits[w] = b;
}

// ================================================================================== dynamic-only EmerNeRF
// ``EmerNeRFOnlyDynamicModel`` (app/models/single/dynamic_nerf.py EmerNerfStreetOnlyDynamic; config
// code_multi/configs/exps/fg_neus=permuto_emernerf/with_gtbox.240212.yaml:277-360): features of a 4-D permutohedral lattice
// over (x, y, z, time) (gathered level-major by permuto.hip: nsim_permuto_gather_pts) -> dynamic decoder h (F = 2 L <= 32) ->
// 64 (relu) -> 1 + 64 (linear): output 0 = raw density (sigma = softplus(raw)), outputs 1..64 = geometry feature ->
// radiance decoder [geo (64) | SH-4 (16) | h_appear (0 | 4)] -> 64 -> 64 (relu) -> 3 (sigmoid).
// Tiling on the 32-unit tiles of mfma_mlp.h: the density row of the second layer is a 64-long dot product on the VALU in
// f32 (a per-lane vector of the pack, as the head of k_nerf) and never enters an MFMA chunk, so the geometry feature is
// exactly two M-tiles; the first radiance layer takes three input tiles (geo 0..63 | SH 64..79 | appearance 80..83 | zero
// padding to 96).  Its weight gradient is two products (geo block, tail block): the staging arrays hold 64 rows.
enum { Y_D1 = 0, Y_D2, Y_Q1, Y_Q2, Y_Q3, Y_D1T, Y_D2T, Y_Q3T, Y_Q2T, Y_Q1T, Y_MCOUNT };
enum { YV_DB1 = 0, YV_DWH, YV_DB2, YV_RB1, YV_RB2, YV_RB3, YV_SCAL, YV_COUNT };
static_assert(Y_MCOUNT <= PACK_MAX_MATS && Y_MCOUNT == G_MCOUNT && YV_COUNT <= GV_COUNT, "the dynamic model's pack fits NgpLayout");
static const int kYUo[Y_MCOUNT] = {64, 64, 64, 64, 32, 32, 64, 64, 64, 96};
static const int kYUi[Y_MCOUNT] = {32, 64, 96, 64, 64, 64, 64, 32, 64, 64};

// pack: [vectors | forward matrices | transposed matrices], as the NGP model's
static inline NgpLayout dyn_layout(int precision) {
  NgpLayout L;
  L.elt = precision == 0 ? 2 : 4;
  int64_t off = 0;
  for (int v = 0; v < GV_COUNT; ++v) {
    L.vec[v] = off;
    if (v < YV_COUNT) off += 64 * 4;
  }
  L.fwd_end = 0;
  for (int m = 0; m < Y_MCOUNT; ++m) {
    L.mat[m] = off;
    off += (int64_t)kYUo[m] * kYUi[m] * L.elt;
    if (m == Y_Q3) L.fwd_end = off;
  }
  L.total = off;
  return L;
}

// radiance input slot (0..95) -> column of the [64 x (80 + NA)] first radiance layer, or -1 (padding)
__host__ __device__ inline int dyn_q1_col(int slot, int NA) { return slot < 80 + NA ? slot : -1; }

__device__ __forceinline__ float dyn_src(int mat, int row, int col, int F, int NA, const float* den_w, const float* rad_w) {
  const int K1 = 80 + NA;
  const int d2 = 64 * F + 64, q2 = 64 * K1, q3 = q2 + 4096;      // d2: row 1 of the [65 x 64] second density layer
  switch (mat) {
    case Y_D1: return col < F ? den_w[row * F + col] : 0.f;
    case Y_D1T: return row < F ? den_w[col * F + row] : 0.f;
    case Y_D2: return den_w[d2 + row * 64 + col];
    case Y_D2T: return den_w[d2 + col * 64 + row];
    case Y_Q1: { const int c = dyn_q1_col(col, NA); return c >= 0 ? rad_w[row * K1 + c] : 0.f; }
    case Y_Q1T: { const int c = dyn_q1_col(row, NA); return c >= 0 ? rad_w[col * K1 + c] : 0.f; }
    case Y_Q2: return rad_w[q2 + row * 64 + col];
    case Y_Q2T: return rad_w[q2 + col * 64 + row];
    case Y_Q3: return row < 3 ? rad_w[q3 + row * 64 + col] : 0.f;
    case Y_Q3T: return col < 3 ? rad_w[q3 + col * 64 + row] : 0.f;
  }
  return 0.f;
}

__global__ void __launch_bounds__(256) k_dyn_pack(NgpLayout L, PackShape sh, int F, int NA, const float* __restrict__ den_w,
                                                   const float* __restrict__ den_b, const float* __restrict__ rad_w,
                                                   const float* __restrict__ rad_b, char* __restrict__ wpack) {
  int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const auto src = [&](int m, int row, int col) { return dyn_src(m, row, col, F, NA, den_w, rad_w); };
  if (pack_matrices(sh, Y_MCOUNT, L.mat, pack_form(L.elt), wpack, tid, src)) return;
  if (tid < (int64_t)YV_COUNT * 64) {
    const int v = (int)(tid >> 6), k = (int)(tid & 63), u = vec_unit(k, 64);
    float val = 0.f;
    switch (v) {
      case YV_DB1: val = den_b[u]; break;
      case YV_DWH: val = den_w[64 * F + u]; break;
      case YV_DB2: val = den_b[65 + u]; break;
      case YV_RB1: val = rad_b[u]; break;
      case YV_RB2: val = rad_b[64 + u]; break;
      case YV_RB3: val = u < 3 ? rad_b[128 + u] : 0.f; break;
      case YV_SCAL: val = (k == 0) ? den_b[64] : 0.f; break;
    }
    ((float*)(wpack + L.vec[v]))[k] = val;
  }
}

struct DynArgs {
  NgpLayout lay;
  int F, NL, n_active, NA;                // features = 2 NL; levels >= n_active are masked
  const char* wpack;
  const float* rays_d;                    // [R,3] (radiance only)
  const int64_t* ridx;                    // [S] (radiance only)
  const float* h_appear;                  // [R,4] or NULL
  int64_t S, PS;                          // points; pitch of h_pl
  float step;                             // alpha = 1 - exp(-sigma step)
  const float* h_pl;                      // [16][PS][2] gathered features
  float *sigma, *alpha, *rgb;             // forward outputs (rgb NULL: density only)
  const float *sigma_fwd, *rgb_fwd;       // saved forward outputs
  const float *dsigma, *dalpha, *drgb;    // upstream (each may be NULL)
  float* dh_pl;                           // [16][S][2] hand-off to nsim_permuto_scatter_pts (may be NULL)
  float* dst[4];                          // dden_w, dden_b, drad_w, drad_b -- or replica 0 of the registered scratch
  int64_t rep_stride;
  int rep_mask;
  float* dh_appear;
  float* dv;                              // POSE: per-sample gradient to the un-normalised ray direction (radiance only)
};

#define DYN_WAVES 4
#define DYN_WAVES_BWD 2       // the weight-gradient accumulators are 67.6 KB per private copy: two fit next to the staging

// sigma = softplus(raw) = log1p(exp(raw)); past 30 the difference to raw is below half an ulp
__device__ __forceinline__ float dyn_softplus(float raw) { return raw > 30.f ? raw : log1pf(expf(raw)); }

// radiance input, third M-tile (slots 64..95): SH-4 of the view direction, appearance code, zero padding
__device__ __forceinline__ void dyn_rin_tail(float (&tail)[16], const float vd[3], const float ha[4], int hi) {
  float sh[16];
  sh4_eval(vd, sh);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int slot = unit_of(0, r, hi);
    float v = 0.f;
    if (slot < 16) v = sh[slot];
    else if (slot < 20) v = ha[slot - 16];
    tail[r] = v;
  }
}

// features of sample s from the level-major planes (masked and padding levels: zero features, their planes are never read)
__device__ __forceinline__ void dyn_load_h(const DynArgs& a, int64_t row, bool valid, int hi, float (&h)[16]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int l = 4 * q + 2 * hi + b;
      float f0 = 0.f, f1 = 0.f;
      if (valid && l < a.n_active) {
        const float* hp = a.h_pl + ((int64_t)l * a.PS + row) * 2;
        f0 = hp[0];
        f1 = hp[1];
      }
      h[4 * q + 2 * b] = f0;
      h[4 * q + 2 * b + 1] = f1;
    }
  }
}

// EmerNeRF's temporal aggregation (the with-flow model): the hidden layer of the density decoder is blended over the sample and
// its two flow-warped neighbours, a = 1/2 relu(W1 h(x, w) + b1) + 1/4 relu(W1 h(x+, w+) + b1) + 1/4 relu(W1 h(x-, w-) + b1); the
// second layer is affine and the weights sum to 1, so this is the weighted mean of the three decoder outputs.
__device__ __forceinline__ float dyn_agg_weight(int p) { return p == 0 ? 0.5f : 0.25f; }

// BWD = 0: sigma / alpha / rgb.  BWD = 1: recomputes the activations from the saved feature planes and accumulates the weight
// gradients (per-wave private LDS accumulators in fp16 mode, as k_ngp), dh planes, dh_appear.
// AGG: the three plane sets of a sample lie at rows s, s + S, s + 2S of ONE buffer of pitch PS = 3S; the first layer runs three
// times, one after the other over the same registers and staging (no LDS beyond the plain kernel's), the backward writes three dh
// plane sets (pitch 3S).  AGG = false is the kernel as it was: every AGG branch is an ``if constexpr``.
// POSE (backward with a colour gradient only; pose refinement): also dv [S,3], the SH-4 slots of the radiance input gradient
// through sh4_grad and n = d / |d|: dv = (I - n n^T) g / |d|.  This model has no direct position input: the position gradient
// comes from the lattice alone (nsim_permuto_dx_pts on the dh planes).  Every POSE branch is an ``if constexpr``.
template <int PREC, int BWD, bool AGG = false, bool POSE = false>
__global__ void __launch_bounds__(64 * (BWD ? DYN_WAVES_BWD : DYN_WAVES)) k_dyn(DynArgs a) {
  static_assert(!POSE || BWD, "the ray gradients are outputs of the backward");
  NSIM_DYN_SMEM(smem);
  constexpr bool PRIV = (PREC == 0 && BWD);
  constexpr int NW = BWD ? DYN_WAVES_BWD : DYN_WAVES;
  const int lane = nsim_lane(), j = lane & 31, hi = lane >> 5;
  const int wave = (int)(threadIdx.x >> 6);
  const NgpLayout& L = a.lay;
  const bool with_rad = BWD ? (a.drgb != nullptr) : (a.rgb != nullptr);
  const char* W = a.wpack;
  const char* WM = a.wpack;
  int wbytes = 0;
  if constexpr (PREC == 0) {
    const int64_t nbytes = BWD ? L.mat[0] : L.fwd_end;
    const int n16 = (int)((nbytes + 15) >> 4);
    const f16x8* src = reinterpret_cast<const f16x8*>(a.wpack);
    f16x8* dst = reinterpret_cast<f16x8*>(smem);
    for (int i = threadIdx.x; i < n16; i += blockDim.x) dst[i] = src[i];
    wbytes = n16 << 4;
    __syncthreads();
    W = smem;
    if constexpr (!BWD) WM = smem;
  }
  constexpr int A_D1 = 0, A_DWH = 2048, A_DB1 = A_DWH + 64, A_BD = A_DB1 + 64, A_D2 = A_BD + 4, A_DB2 = A_D2 + 4096,
                A_Q1 = A_DB2 + 64, A_Q2 = A_Q1 + 6144, A_Q3 = A_Q2 + 4096, A_RB1 = A_Q3 + 192, A_RB2 = A_RB1 + 64,
                A_RB3 = A_RB2 + 64, A_TOTAL = A_RB3 + 4;
  static_assert(A_TOTAL == 16904, "nsim_dyn_bwd sizes the LDS from this count");
  constexpr int ACC_BYTES = (A_TOTAL * 4 + 15) & ~15;
  float* accum = nullptr;
  char* stA = nullptr;
  char* stB = nullptr;
  if constexpr (BWD) {
    accum = reinterpret_cast<float*>(smem + wbytes + (PRIV ? wave * ACC_BYTES : 0));
    char* stbase = smem + wbytes + (PRIV ? NW : 1) * ACC_BYTES + wave * stage_bytes_per_wave<PREC>();
    stA = stbase;
    stB = stbase + stage_bytes_per_wave<PREC>() / 2;
    if constexpr (PRIV) {
      for (int i = lane; i < A_TOTAL; i += 64) accum[i] = 0.f;
    } else {
      for (int i = threadIdx.x; i < A_TOTAL; i += blockDim.x) accum[i] = 0.f;
    }
    __syncthreads();
  }
  const float b_d = reinterpret_cast<const float*>(W + L.vec[YV_SCAL])[0];
  const int64_t ntiles = (a.S + 31) / 32;
  const int64_t wstride = (int64_t)gridDim.x * NW;
  for (int64_t tile = (int64_t)blockIdx.x * NW + wave; tile < ntiles; tile += wstride) {
    const int64_t s = tile * 32 + j;
    const bool valid = s < a.S;
    int64_t ray = 0;
    float vd[3] = {0.f, 0.f, 1.f}, ha[4] = {0.f, 0.f, 0.f, 0.f};
    if (valid && with_rad) {
      ray = a.ridx[s];
      float d[3], n2 = 0.f;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        d[c] = a.rays_d[3 * ray + c];
        n2 = n2 + d[c] * d[c];
      }
      const float inv = n2 > 0.f ? 1.0f / sqrtf(n2) : 0.f;
#pragma unroll
      for (int c = 0; c < 3; ++c) vd[c] = d[c] * inv;
      if (a.h_appear && a.NA == 4) {
#pragma unroll
        for (int c = 0; c < 4; ++c) ha[c] = a.h_appear[4 * ray + c];
      }
    }
    // -------------------------------------------------------------- features from the level-major planes
    float h[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int l = 4 * q + 2 * hi + b;
        float f0 = 0.f, f1 = 0.f;
        if (valid && l < a.n_active) {      // (masked and padding levels: zero features, their planes are never read)
          const float* hp = a.h_pl + ((int64_t)l * a.PS + s) * 2;
          f0 = hp[0];
          f1 = hp[1];
        }
        h[4 * q + 2 * b] = f0;
        h[4 * q + 2 * b + 1] = f1;
      }
    }
    // -------------------------------------------------------------- dynamic (density) decoder
    float a1[32];
    if constexpr (!AGG) {
      dense<PREC, 2, 1>(a1, WM + L.mat[Y_D1], h, true);
#pragma unroll
      for (int k = 0; k < 32; ++k) a1[k] = fmaxf(a1[k] + ngp_vec(W, L, YV_DB1, hi, k), 0.f);
    } else {
#pragma unroll
      for (int k = 0; k < 32; ++k) a1[k] = 0.f;
#pragma unroll 1
      for (int p = 0; p < 3; ++p) {
        float hp_[16], t1[32];
        dyn_load_h(a, s + p * a.S, valid, hi, hp_);
        dense<PREC, 2, 1>(t1, WM + L.mat[Y_D1], hp_, true);
        const float wp = dyn_agg_weight(p);
#pragma unroll
        for (int k = 0; k < 32; ++k) a1[k] = a1[k] + wp * fmaxf(t1[k] + ngp_vec(W, L, YV_DB1, hi, k), 0.f);
      }
    }
    float raw = 0.f;
#pragma unroll
    for (int k = 0; k < 32; ++k) raw = raw + ngp_vec(W, L, YV_DWH, hi, k) * a1[k];
    raw = raw + wave_shfl_xor(raw, 32) + b_d;
    if constexpr (!BWD) {
      const float sg = dyn_softplus(raw);
      if (valid && hi == 0) {
        a.sigma[s] = sg;
        if (a.alpha) a.alpha[s] = 1.0f - expf(-sg * a.step);
      }
    }
    float geo[32], tail[16], r1[32], r2[32];
    if (with_rad) {
      dense<PREC, 2, 2>(geo, WM + L.mat[Y_D2], a1, true);
      float rin[48];
#pragma unroll
      for (int k = 0; k < 32; ++k) {
        geo[k] = geo[k] + ngp_vec(W, L, YV_DB2, hi, k);
        rin[k] = geo[k];
      }
      dyn_rin_tail(tail, vd, ha, hi);
#pragma unroll
      for (int k = 0; k < 16; ++k) rin[32 + k] = tail[k];
      dense<PREC, 2, 3>(r1, WM + L.mat[Y_Q1], rin, true);
#pragma unroll
      for (int k = 0; k < 32; ++k) r1[k] = fmaxf(r1[k] + ngp_vec(W, L, YV_RB1, hi, k), 0.f);
      dense<PREC, 2, 2>(r2, WM + L.mat[Y_Q2], r1, false);
#pragma unroll
      for (int k = 0; k < 32; ++k) r2[k] = fmaxf(r2[k] + ngp_vec(W, L, YV_RB2, hi, k), 0.f);
    }
    if constexpr (!BWD) {
      if (with_rad) {
        float o3[16];
        dense<PREC, 1, 2>(o3, WM + L.mat[Y_Q3], r2, false);
        if (valid && hi == 0) {
#pragma unroll
          for (int c = 0; c < 3; ++c) a.rgb[3 * s + c] = 1.0f / (1.0f + nsim_fast_exp(-(o3[c] + ngp_vec(W, L, YV_RB3, hi, c))));
        }
      }
    }
    if constexpr (BWD) {
      float da[32];
#pragma unroll
      for (int k = 0; k < 32; ++k) da[k] = 0.f;
      if (with_rad) {
        float gr[3] = {0.f, 0.f, 0.f}, rgbv[3] = {0.f, 0.f, 0.f};
        if (valid) {
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            gr[c] = a.drgb[3 * s + c];
            rgbv[c] = a.rgb_fwd[3 * s + c];
          }
        }
        float dout[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) dout[r] = 0.f;
        if (hi == 0) {
#pragma unroll
          for (int c = 0; c < 3; ++c) dout[c] = gr[c] * rgbv[c] * (1.0f - rgbv[c]);
        }
        dw_product<PREC, 1, 2, PRIV>(stA, stB, dout, r2, accum + A_Q3, 64, 3, 64, accum + A_RB3);
        float dr2[32];
        dense<PREC, 2, 1>(dr2, WM + L.mat[Y_Q3T], dout, true);
#pragma unroll
        for (int k = 0; k < 32; ++k) dr2[k] = r2[k] > 0.f ? dr2[k] : 0.f;
        dw_product<PREC, 2, 2, PRIV>(stA, stB, dr2, r1, accum + A_Q2, 64, 64, 64, accum + A_RB2);
        float dr1[32];
        dense<PREC, 2, 2>(dr1, WM + L.mat[Y_Q2T], dr2, true);
#pragma unroll
        for (int k = 0; k < 32; ++k) dr1[k] = r1[k] > 0.f ? dr1[k] : 0.f;
        // the first radiance layer's gradient [64 x 96] in two products: columns 0..63 (geo), 64..95 (SH | appearance | padding)
        dw_product<PREC, 2, 2, PRIV>(stA, stB, dr1, geo, accum + A_Q1, 96, 64, 64, accum + A_RB1);
        dw_product<PREC, 2, 1, PRIV>(stA, stB, dr1, tail, accum + A_Q1 + 64, 96, 64, 32, nullptr);
        float din[48];
        dense<PREC, 3, 2>(din, WM + L.mat[Y_Q1T], dr1, true);
        // appearance slots 80..83 = third M-tile local 16..19 (lower half-wave, registers 8..11); one atomic per ray and channel
        if (a.dh_appear && a.NA == 4) {
          float c0 = din[32 + 8], c1 = din[32 + 9], c2 = din[32 + 10], c3 = din[32 + 11];
          const bool v = valid && hi == 0;
          const bool last = halfwave_run_sum2(ray, v, c0, c1);
          halfwave_run_sum2(ray, v, c2, c3);
          if (last) {
            float* dst = a.dh_appear + 4 * ray;
            atomicAdd(dst, c0);
            atomicAdd(dst + 1, c1);
            atomicAdd(dst + 2, c2);
            atomicAdd(dst + 3, c3);
          }
        }
        if constexpr (POSE) {     // SH slot k of the third M-tile: half-wave (k >> 2) & 1, register (k & 3) + 4 (k >> 3)
          float gsh[16];
#pragma unroll
          for (int k = 0; k < 16; ++k) {
            const float v = (hi == ((k >> 2) & 1)) ? din[32 + (k & 3) + 4 * (k >> 3)] : 0.f;
            gsh[k] = v + wave_shfl_xor(v, 32);
          }
          float gv[3];
          sh4_grad(vd, gsh, gv);
          if (valid && hi == 0) {
            float n2 = 0.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              const float dc = a.rays_d[3 * ray + c];
              n2 = n2 + dc * dc;
            }
            const float inv = n2 > 0.f ? 1.0f / sqrtf(n2) : 0.f;
            const float ng = vd[0] * gv[0] + vd[1] * gv[1] + vd[2] * gv[2];
#pragma unroll
            for (int c = 0; c < 3; ++c) a.dv[3 * s + c] = (gv[c] - vd[c] * ng) * inv;
          }
        }
        float dgeo[32];
#pragma unroll
        for (int k = 0; k < 32; ++k) dgeo[k] = valid ? din[k] : 0.f;
        dw_product<PREC, 2, 2, PRIV>(stA, stB, dgeo, a1, accum + A_D2, 64, 64, 64, accum + A_DB2);
        dense<PREC, 2, 2>(da, WM + L.mat[Y_D2T], dgeo, true);
      }
      // ---- sigma = softplus(raw): d raw = (d sigma + d alpha step exp(-sigma step)) sigmoid(min(raw, 15))
      float draw = 0.f;
      if (valid) {
        const float sg = a.sigma_fwd[s];
        if (a.dsigma) draw = draw + a.dsigma[s];
        if (a.dalpha) draw = draw + a.dalpha[s] * (a.step * expf(-sg * a.step));
        draw = draw * (1.0f / (1.0f + expf(-fminf(raw, 15.0f))));
      }
      float whv[32];
#pragma unroll
      for (int k = 0; k < 32; ++k) {
        whv[k] = draw * a1[k];
        if constexpr (!AGG) da[k] = a1[k] > 0.f ? da[k] + draw * ngp_vec(W, L, YV_DWH, hi, k) : 0.f;
        else da[k] = da[k] + draw * ngp_vec(W, L, YV_DWH, hi, k);      // (d a: the relu masks are the three passes' own)
      }
      rowsum_acc<PREC, 2, PRIV>(stA, whv, accum + A_DWH, 64);
      {
        float v = (hi == 0) ? draw : 0.f;
        v = wave_sum(v);
        if (lane == 0 && v != 0.f) {
          if constexpr (PRIV) accum[A_BD] = accum[A_BD] + v;
          else atomicAdd(&accum[A_BD], v);
        }
      }
      if constexpr (!AGG) {
      dw_product<PREC, 2, 1, PRIV>(stA, stB, da, h, accum + A_D1, 32, 64, 32, accum + A_DB1);
      if (a.dh_pl) {
        float dh[16];
        dense<PREC, 1, 2>(dh, WM + L.mat[Y_D1T], da, true);
        if (valid) {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
#pragma unroll
            for (int b = 0; b < 2; ++b) {
              const int l = 4 * q + 2 * hi + b;
              if (l >= a.NL) continue;                      // (the scatter reads the lattice's own levels only)
              const bool on = l < a.n_active;
              float* dp = a.dh_pl + ((int64_t)l * a.S + s) * 2;
              dp[0] = on ? dh[4 * q + 2 * b] : 0.f;
              dp[1] = on ? dh[4 * q + 2 * b + 1] : 0.f;
            }
          }
        }
      }
      } else {
        // the three first-layer passes again, one after the other: pre-activation, its relu mask on the weighted d a, the
        // weight-gradient product and the pass's dh plane set (row s + p S of pitch 3S)
#pragma unroll 1
        for (int p = 0; p < 3; ++p) {
          float hp_[16], t1[32];
          dyn_load_h(a, s + p * a.S, valid, hi, hp_);
          dense<PREC, 2, 1>(t1, WM + L.mat[Y_D1], hp_, true);
          const float wp = dyn_agg_weight(p);
#pragma unroll
          for (int k = 0; k < 32; ++k) t1[k] = (t1[k] + ngp_vec(W, L, YV_DB1, hi, k)) > 0.f ? wp * da[k] : 0.f;
          dw_product<PREC, 2, 1, PRIV>(stA, stB, t1, hp_, accum + A_D1, 32, 64, 32, accum + A_DB1);
          if (a.dh_pl) {
            float dh[16];
            dense<PREC, 1, 2>(dh, WM + L.mat[Y_D1T], t1, true);
            if (valid) {
#pragma unroll
              for (int q = 0; q < 4; ++q) {
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                  const int l = 4 * q + 2 * hi + b;
                  if (l >= a.NL) continue;
                  const bool on = l < a.n_active;
                  float* dp = a.dh_pl + ((int64_t)l * a.PS + s + p * a.S) * 2;
                  dp[0] = on ? dh[4 * q + 2 * b] : 0.f;
                  dp[1] = on ? dh[4 * q + 2 * b + 1] : 0.f;
                }
              }
            }
          }
        }
      }
    }
  }
  if constexpr (BWD) {
    __syncthreads();
    const int F = a.F, K1 = 80 + a.NA;
    const int64_t rep = (int64_t)(blockIdx.x & (unsigned)a.rep_mask) * a.rep_stride;
    for (int i = threadIdx.x; i < A_TOTAL; i += blockDim.x) {
      float v;
      if constexpr (PRIV) {
        constexpr int ACC_FLOATS = ACC_BYTES / 4;
        const float* a0 = reinterpret_cast<const float*>(smem + wbytes);
        v = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) v += a0[w * ACC_FLOATS + i];
      } else {
        v = accum[i];
      }
      if (v == 0.f) continue;
      int d = -1;
      int64_t off = 0;
      if (i < A_DWH) {
        const int row = i >> 5, col = i & 31;
        if (col < F) { d = 0; off = row * F + col; }
      } else if (i < A_DB1) { d = 0; off = 64 * F + (i - A_DWH); }
      else if (i < A_BD) { d = 1; off = i - A_DB1; }
      else if (i < A_D2) { if (i == A_BD) { d = 1; off = 64; } }
      else if (i < A_DB2) { d = 0; off = 64 * F + 64 + (i - A_D2); }
      else if (i < A_Q1) { d = 1; off = 65 + (i - A_DB2); }
      else if (i < A_Q2) {
        const int row = (i - A_Q1) / 96, c = dyn_q1_col((i - A_Q1) % 96, a.NA);
        if (c >= 0) { d = 2; off = row * K1 + c; }
      } else if (i < A_Q3) { d = 2; off = 64 * K1 + (i - A_Q2); }
      else if (i < A_RB1) { d = 2; off = 64 * K1 + 4096 + (i - A_Q3); }
      else if (i < A_RB2) { d = 3; off = i - A_RB1; }
      else if (i < A_RB3) { d = 3; off = 64 + (i - A_RB2); }
      else if (i - A_RB3 < 3) { d = 3; off = 128 + (i - A_RB3); }
      if (d >= 0) atomicAdd(a.dst[d] + rep + off, v);
    }
  }
}

// ----------------------------------------------------------------------------------------- scene-flow decoder
// ``flow_decoder_cfg{type: mlp, D: 2, W: 64}`` of the with-flow EmerNeRF model (code_multi/configs/exps/fg_emernerf/
// no_gtbox_with_flow.240208.yaml): features of the flow lattice h_f (F = 2 L_f <= 32, level-major planes of
// nsim_permuto_gather_pts) -> 64 (relu) -> 64 (relu) -> 6 (linear): outputs 0..2 = flow_fwd, 3..5 = flow_bwd.  The two hidden
// layers run on the 32-unit tiles of mfma_mlp.h; the six output rows are 64-long dot products on the VALU in f32 (per-lane
// vectors of the pack, as the density row of k_dyn), so the displacements are not rounded to fp16 on the way out.  Flat
// parameters: flow_w = [W1 64 x F | W2 64 x 64 | W3 6 x 64], flow_b = [b1 64 | b2 64 | b3 6], row-major.
enum { F_W1 = 0, F_W2, F_W3T, F_W2T, F_W1T, F_MCOUNT };
enum { FV_B1 = 0, FV_B2, FV_W3, FV_SCAL = FV_W3 + 6, FV_COUNT };
static_assert(F_MCOUNT <= PACK_MAX_MATS, "PackShape holds the flow decoder's matrices");
static const int kFUo[F_MCOUNT] = {64, 64, 64, 64, 32};
static const int kFUi[F_MCOUNT] = {32, 64, 32, 64, 64};

// pack: [vectors | forward matrices (W1, W2) | backward matrices (W3^T padded to 32 inputs, W2^T, W1^T)]
struct FlowLayout {
  int64_t mat[F_MCOUNT], vec[FV_COUNT], fwd_end, total;
  int elt;
};
static inline FlowLayout flow_layout(int precision) {
  FlowLayout L;
  L.elt = precision == 0 ? 2 : 4;
  int64_t off = 0;
  for (int v = 0; v < FV_COUNT; ++v) {
    L.vec[v] = off;
    off += 64 * 4;
  }
  L.fwd_end = 0;
  for (int m = 0; m < F_MCOUNT; ++m) {
    L.mat[m] = off;
    off += (int64_t)kFUo[m] * kFUi[m] * L.elt;
    if (m == F_W2) L.fwd_end = off;
  }
  L.total = off;
  return L;
}

__device__ __forceinline__ float flow_src(int mat, int row, int col, int F, const float* w) {
  const int w2 = 64 * F, w3 = w2 + 4096;
  switch (mat) {
    case F_W1: return col < F ? w[row * F + col] : 0.f;
    case F_W1T: return row < F ? w[col * F + row] : 0.f;
    case F_W2: return w[w2 + row * 64 + col];
    case F_W2T: return w[w2 + col * 64 + row];
    case F_W3T: return col < 6 ? w[w3 + col * 64 + row] : 0.f;
  }
  return 0.f;
}

__global__ void __launch_bounds__(256) k_flow_pack(FlowLayout L, PackShape sh, int F, const float* __restrict__ flow_w,
                                                    const float* __restrict__ flow_b, char* __restrict__ wpack) {
  int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const auto src = [&](int m, int row, int col) { return flow_src(m, row, col, F, flow_w); };
  if (pack_matrices(sh, F_MCOUNT, L.mat, pack_form(L.elt), wpack, tid, src)) return;
  if (tid < (int64_t)FV_COUNT * 64) {
    const int v = (int)(tid >> 6), k = (int)(tid & 63), u = vec_unit(k, 64);
    float val = 0.f;
    if (v == FV_B1) val = flow_b[u];
    else if (v == FV_B2) val = flow_b[64 + u];
    else if (v < FV_SCAL) val = flow_w[64 * F + 4096 + (v - FV_W3) * 64 + u];
    else val = k < 6 ? flow_b[128 + k] : 0.f;
    ((float*)(wpack + L.vec[v]))[k] = val;
  }
}

struct FlowArgs {
  FlowLayout lay;
  int F, NL, n_active;
  const char* wpack;
  int64_t S, PS;                          // points; pitch of h_pl and dh_pl
  const float* h_pl;                      // [16][PS][2] gathered flow features
  float* flow6;                           // [S,6] forward output
  const float* dflow6;                    // [S,6] upstream
  float* dh_pl;                           // [16][PS][2] hand-off to nsim_permuto_scatter_pts / _dx_pts (may be NULL)
  float* dst[2];                          // dflow_w, dflow_b -- or replica 0 of the registered scratch
  int64_t rep_stride;
  int rep_mask;
};

#define FLOW_WAVES 4
#define FLOW_WAVES_BWD 2      // the weight-gradient accumulators are 26.7 KB per private copy

__device__ __forceinline__ float flow_vec(const char* WV, const FlowLayout& L, int v, int hi, int k) {
  return reinterpret_cast<const float*>(WV + L.vec[v])[hi * 32 + k];
}

template <int PREC, int BWD>
__global__ void __launch_bounds__(64 * (BWD ? FLOW_WAVES_BWD : FLOW_WAVES)) k_flow(FlowArgs a) {
  NSIM_DYN_SMEM(smem);
  constexpr bool PRIV = (PREC == 0 && BWD);
  constexpr int NW = BWD ? FLOW_WAVES_BWD : FLOW_WAVES;
  const int lane = nsim_lane(), j = lane & 31, hi = lane >> 5;
  const int wave = (int)(threadIdx.x >> 6);
  const FlowLayout& L = a.lay;
  const char* W = a.wpack;
  const char* WM = a.wpack;
  int wbytes = 0;
  if constexpr (PREC == 0) {
    const int64_t nbytes = BWD ? L.mat[0] : L.fwd_end;
    const int n16 = (int)((nbytes + 15) >> 4);
    const f16x8* src = reinterpret_cast<const f16x8*>(a.wpack);
    f16x8* dst = reinterpret_cast<f16x8*>(smem);
    for (int i = threadIdx.x; i < n16; i += blockDim.x) dst[i] = src[i];
    wbytes = n16 << 4;
    __syncthreads();
    W = smem;
    if constexpr (!BWD) WM = smem;
  }
  constexpr int A_W1 = 0, A_B1 = 2048, A_W2 = A_B1 + 64, A_B2 = A_W2 + 4096, A_W3 = A_B2 + 64, A_B3 = A_W3 + 384,
                A_TOTAL = A_B3 + 8;
  static_assert(A_TOTAL == 6664, "nsim_flow_bwd sizes the LDS from this count");
  constexpr int ACC_BYTES = (A_TOTAL * 4 + 15) & ~15;
  float* accum = nullptr;
  char* stA = nullptr;
  char* stB = nullptr;
  if constexpr (BWD) {
    accum = reinterpret_cast<float*>(smem + wbytes + (PRIV ? wave * ACC_BYTES : 0));
    char* stbase = smem + wbytes + (PRIV ? NW : 1) * ACC_BYTES + wave * stage_bytes_per_wave<PREC>();
    stA = stbase;
    stB = stbase + stage_bytes_per_wave<PREC>() / 2;
    if constexpr (PRIV) {
      for (int i = lane; i < A_TOTAL; i += 64) accum[i] = 0.f;
    } else {
      for (int i = threadIdx.x; i < A_TOTAL; i += blockDim.x) accum[i] = 0.f;
    }
    __syncthreads();
  }
  const int64_t ntiles = (a.S + 31) / 32;
  const int64_t wstride = (int64_t)gridDim.x * NW;
  for (int64_t tile = (int64_t)blockIdx.x * NW + wave; tile < ntiles; tile += wstride) {
    const int64_t s = tile * 32 + j;
    const bool valid = s < a.S;
    float h[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int l = 4 * q + 2 * hi + b;
        float f0 = 0.f, f1 = 0.f;
        if (valid && l < a.n_active) {      // (masked and padding levels: zero features, their planes are never read)
          const float* hp = a.h_pl + ((int64_t)l * a.PS + s) * 2;
          f0 = hp[0];
          f1 = hp[1];
        }
        h[4 * q + 2 * b] = f0;
        h[4 * q + 2 * b + 1] = f1;
      }
    }
    float a1[32], a2[32];
    dense<PREC, 2, 1>(a1, WM + L.mat[F_W1], h, true);
#pragma unroll
    for (int k = 0; k < 32; ++k) a1[k] = fmaxf(a1[k] + flow_vec(W, L, FV_B1, hi, k), 0.f);
    dense<PREC, 2, 2>(a2, WM + L.mat[F_W2], a1, true);
#pragma unroll
    for (int k = 0; k < 32; ++k) a2[k] = fmaxf(a2[k] + flow_vec(W, L, FV_B2, hi, k), 0.f);
    if constexpr (!BWD) {
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        float o = 0.f;
#pragma unroll
        for (int k = 0; k < 32; ++k) o = o + flow_vec(W, L, FV_W3 + c, hi, k) * a2[k];
        o = o + wave_shfl_xor(o, 32) + reinterpret_cast<const float*>(W + L.vec[FV_SCAL])[c];
        if (valid && hi == 0) a.flow6[6 * s + c] = o;
      }
    } else {
      // upstream gradient as the first M-tile's units 0..5: unit u < 4 is register u of the lower half-wave, 4 and 5 are
      // registers 0 and 1 of the upper one (unit_of)
      float dout[16], g6[6];
#pragma unroll
      for (int r = 0; r < 16; ++r) dout[r] = 0.f;
#pragma unroll
      for (int c = 0; c < 6; ++c) g6[c] = valid ? a.dflow6[6 * s + c] : 0.f;
      if (hi == 0) {
#pragma unroll
        for (int c = 0; c < 4; ++c) dout[c] = g6[c];
      } else {
        dout[0] = g6[4];
        dout[1] = g6[5];
      }
      dw_product<PREC, 1, 2, PRIV>(stA, stB, dout, a2, accum + A_W3, 64, 6, 64, accum + A_B3);
      float da2[32];
      dense<PREC, 2, 1>(da2, WM + L.mat[F_W3T], dout, true);
#pragma unroll
      for (int k = 0; k < 32; ++k) da2[k] = a2[k] > 0.f ? da2[k] : 0.f;
      dw_product<PREC, 2, 2, PRIV>(stA, stB, da2, a1, accum + A_W2, 64, 64, 64, accum + A_B2);
      float da1[32];
      dense<PREC, 2, 2>(da1, WM + L.mat[F_W2T], da2, true);
#pragma unroll
      for (int k = 0; k < 32; ++k) da1[k] = a1[k] > 0.f ? da1[k] : 0.f;
      dw_product<PREC, 2, 1, PRIV>(stA, stB, da1, h, accum + A_W1, 32, 64, 32, accum + A_B1);
      if (a.dh_pl) {
        float dh[16];
        dense<PREC, 1, 2>(dh, WM + L.mat[F_W1T], da1, true);
        if (valid) {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
#pragma unroll
            for (int b = 0; b < 2; ++b) {
              const int l = 4 * q + 2 * hi + b;
              if (l >= a.NL) continue;                      // (the scatter reads the lattice's own levels only)
              const bool on = l < a.n_active;
              float* dp = a.dh_pl + ((int64_t)l * a.PS + s) * 2;
              dp[0] = on ? dh[4 * q + 2 * b] : 0.f;
              dp[1] = on ? dh[4 * q + 2 * b + 1] : 0.f;
            }
          }
        }
      }
    }
  }
  if constexpr (BWD) {
    __syncthreads();
    const int F = a.F;
    const int64_t rep = (int64_t)(blockIdx.x & (unsigned)a.rep_mask) * a.rep_stride;
    for (int i = threadIdx.x; i < A_TOTAL; i += blockDim.x) {
      float v;
      if constexpr (PRIV) {
        constexpr int ACC_FLOATS = ACC_BYTES / 4;
        const float* a0 = reinterpret_cast<const float*>(smem + wbytes);
        v = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) v += a0[w * ACC_FLOATS + i];
      } else {
        v = accum[i];
      }
      if (v == 0.f) continue;
      int d = -1;
      int64_t off = 0;
      if (i < A_B1) {
        const int row = i >> 5, col = i & 31;
        if (col < F) { d = 0; off = row * F + col; }
      } else if (i < A_W2) { d = 1; off = i - A_B1; }
      else if (i < A_B2) { d = 0; off = 64 * F + (i - A_W2); }
      else if (i < A_W3) { d = 1; off = 64 + (i - A_B2); }
      else if (i < A_B3) { d = 0; off = 64 * F + 4096 + (i - A_W3); }
      else if (i - A_B3 < 6) { d = 1; off = 128 + (i - A_B3); }
      if (d >= 0) atomicAdd(a.dst[d] + rep + off, v);
    }
  }
}

// warped lattice points of the flow field: x4w [2S,4] = (x + flow_fwd, w+) | (x + flow_bwd, w-) from the lattice points x4 [S,4]
// (object coordinates: the AABB normalisation is part of the lattice's scale, so a displacement in object coordinates moves the
// normalised position by flow / half-extent), w+ = min(w + delta, hi), w- = max(w - delta, lo) (the ends clamp, as k_dyn_time does)
__global__ void __launch_bounds__(256) k_dyn_warp_fwd(const float* __restrict__ x4, const float* __restrict__ flow6, int64_t S,
                                                       float delta, float lo, float hi, float* __restrict__ x4w) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const float w = x4[4 * s + 3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float x = x4[4 * s + c];
    x4w[4 * s + c] = x + flow6[6 * s + c];
    x4w[4 * (S + s) + c] = x + flow6[6 * s + 3 + c];
  }
  x4w[4 * s + 3] = fminf(w + delta, hi);
  x4w[4 * (S + s) + 3] = fmaxf(w - delta, lo);
}

// dflow6[s][0..2] += dx4w[s][0..2], dflow6[s][3..5] += dx4w[S + s][0..2] (the time parts carry no gradient)
__global__ void __launch_bounds__(256) k_dyn_warp_bwd(const float* __restrict__ dx4w, int64_t S, float* __restrict__ dflow6) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    dflow6[6 * s + c] = dflow6[6 * s + c] + dx4w[4 * s + c];
    dflow6[6 * s + 3 + c] = dflow6[6 * s + 3 + c] + dx4w[4 * (S + s) + c];
  }
}

// Pose refinement: the position gradient of sample s from the lattice launches' [.,4] outputs -- dx[s][c] = the position parts of
// dx4_dyn[s] + dx4_flow[s] (nsim_permuto_dx_pts at the sample, dynamic / flow lattice) + dx4w_dyn[s] + dx4w_dyn[S + s] + dx4w_flow[s]
// + dx4w_flow[S + s] (at its two warped points: x+- = x +- flow, d x+- / d x = I); the time components are dropped.  Each input
// may be NULL; every dx row is written.
__global__ void __launch_bounds__(256) k_dyn_pose_dx(const float* __restrict__ dx4_dyn, const float* __restrict__ dx4_flow,
                                                      const float* __restrict__ dx4w_dyn, const float* __restrict__ dx4w_flow,
                                                      int64_t S, float* __restrict__ dx) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float v = 0.f;
    if (dx4_dyn) v = v + dx4_dyn[4 * s + c];
    if (dx4w_dyn) v = v + dx4w_dyn[4 * s + c] + dx4w_dyn[4 * (S + s) + c];
    if (dx4w_flow) v = v + dx4w_flow[4 * s + c] + dx4w_flow[4 * (S + s) + c];
    if (dx4_flow) v = v + dx4_flow[4 * s + c];
    dx[3 * s + c] = v;
  }
}

// ----------------------------------------------------------------------------------------- time input
// w = SeqEmbedding(tk, v)(ts, 'interp') (piecewise linear, the ends clamp, T == 1: v[0]) and the slice of a time: the nearest of
// the T keyframes tk, a tie to the lower index, times outside the range clamp.
__global__ void __launch_bounds__(256) k_dyn_time(const float* __restrict__ tk, const float* __restrict__ v, int T,
                                                   const float* __restrict__ ts, int64_t n, int64_t words_per_slice,
                                                   float* __restrict__ w_out, int64_t* __restrict__ slice_out,
                                                   int64_t* __restrict__ word_off_out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float t = ts[i];
  if (w_out) {
    float w = v[0];
    if (T > 1) {
      int lo = 0, hi = T;                   // first index with tk[idx] > t (searchsorted right), clamped to [1, T - 1]
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (tk[mid] > t) hi = mid;
        else lo = mid + 1;
      }
      const int idx = lo < 1 ? 1 : (lo > T - 1 ? T - 1 : lo);
      const float t0 = tk[idx - 1], t1 = tk[idx];
      float f = (t - t0) / fmaxf(t1 - t0, 1e-12f);
      f = fminf(fmaxf(f, 0.f), 1.f);
      w = v[idx - 1] + f * (v[idx] - v[idx - 1]);
    }
    w_out[i] = w;
  }
  if (slice_out || word_off_out) {
    int lo = 0, hi = T;                     // first keyframe >= t
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (tk[mid] >= t) hi = mid;
      else lo = mid + 1;
    }
    int k = lo;
    if (k >= T) k = T - 1;
    else if (k > 0 && !(tk[k] - t < t - tk[k - 1])) k = k - 1;      // tie: lower index
    if (slice_out) slice_out[i] = k;
    if (word_off_out) word_off_out[i] = (int64_t)k * words_per_slice;
  }
}

// lattice points [S,4] = (position, time coordinate): position x [S,3] with w per point, or rays_o[ridx] + t rays_d[ridx] with w
// per ray
__global__ void __launch_bounds__(256) k_dyn_points(const float* __restrict__ x, const float* __restrict__ rays_o,
                                                     const float* __restrict__ rays_d, const float* __restrict__ t,
                                                     const int64_t* __restrict__ ridx, const float* __restrict__ w, int64_t S,
                                                     float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= S) return;
  float p[4];
  if (x) {
    p[0] = x[3 * i]; p[1] = x[3 * i + 1]; p[2] = x[3 * i + 2];
    p[3] = w[i];
  } else {
    const int64_t r = ridx[i];
    const float tt = t[i];
    p[0] = rays_o[3 * r] + tt * rays_d[3 * r];
    p[1] = rays_o[3 * r + 1] + tt * rays_d[3 * r + 1];
    p[2] = rays_o[3 * r + 2] + tt * rays_d[3 * r + 2];
    p[3] = w[r];
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) out[4 * i + c] = p[c];
}

// ----------------------------------------------------------------------------------------- time-sliced density occupancy
// ``accel_cfg{type: occ_grid_dynamic}``: K value grids of one resolution, ``stride`` floats apart; every point is folded into
// the grid of ITS slice (per point with x, per ray with rays).  occ_max_wave with the slice in the run key: equal voxels of
// neighbouring lanes merge only inside one slice.
__global__ void __launch_bounds__(256) k_occ_max_density_sliced(float* __restrict__ val, int64_t stride, int K,
                                                                 const float* __restrict__ x, const float* __restrict__ rays_o,
                                                                 const float* __restrict__ rays_d, const float* __restrict__ t,
                                                                 const int64_t* __restrict__ ridx,
                                                                 const int64_t* __restrict__ slice, const float* __restrict__ sigma,
                                                                 int64_t n, OccDev m) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = nsim_lane();
  bool ok = i < n;
  float px = 0.f, py = 0.f, pz = 0.f, v = 0.f;
  int64_t k = 0;
  if (ok) {
    if (x) {
      px = x[3 * i]; py = x[3 * i + 1]; pz = x[3 * i + 2];
      k = slice[i];
    } else {
      const int64_t r = ridx[i];
      const float tt = t[i];
      px = rays_o[3 * r] + tt * rays_d[3 * r];
      py = rays_o[3 * r + 1] + tt * rays_d[3 * r + 1];
      pz = rays_o[3 * r + 2] + tt * rays_d[3 * r + 2];
      k = slice[r];
    }
    v = fmaxf(sigma[i], 0.f);
    if (!(v == v)) v = 0.f;
    ok = k >= 0 && k < K;               // (a slice outside the grids is dropped, never written)
  }
  int64_t flat = -1 - lane;
  if (ok) {
    int64_t f;
    ok = occ_voxel(m, px, py, pz, f);
    if (ok) flat = k * stride + f;
  }
  if (!ok) v = 0.f;
  const int64_t pk = wave_shfl(flat, lane - 1);
  const unsigned long long heads = wave_ballot(lane == 0 || pk != flat);
  const unsigned long long below = heads & ((2ull << lane) - 1ull);
  const int run_start = 63 - __builtin_clzll(below);
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const float o = wave_shfl(v, lane - d);
    if (lane - d >= run_start) v = fmaxf(v, o);
  }
  const bool last = lane == 63 || ((heads >> (lane + 1)) & 1ull);
  if (!ok || !last) return;
  if (val[flat] >= v) return;
  int iv;
  memcpy(&iv, &v, 4);
  atomicMax((int*)val + flat, iv);
}

// k_occ_partial_sum / k_occ_pack_bits_mean for all K slices in one launch each (blockIdx.y = slice): the same sums in the same
// order, so a slice's threshold equals that of a single grid holding its values.  Slice k: values val + k stride, words
// bits + k ceil(nvox / 32), workspace ws + 65 k (64 partial sums, then the threshold used).
__global__ void __launch_bounds__(256) k_occ_partial_sum_sliced(const float* __restrict__ val, int64_t stride, int64_t nvox,
                                                                 float* __restrict__ ws) {
  __shared__ float sh[4];
  const float* vk = val + (int64_t)blockIdx.y * stride;
  float s = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvox; i += (int64_t)gridDim.x * blockDim.x) s += vk[i];
  s = wave_sum(s);
  if (nsim_lane() == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) ws[(int64_t)blockIdx.y * (OCC_MEAN_BLOCKS + 1) + blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

__global__ void __launch_bounds__(256) k_occ_pack_bits_mean_sliced(const float* __restrict__ val, int64_t stride, int64_t nvox,
                                                                    float occ_thre, int consider_mean, float* __restrict__ ws,
                                                                    uint32_t* __restrict__ bits) {
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t k = blockIdx.y;
  const float* vk = val + k * stride;
  float* wk = ws + k * (OCC_MEAN_BLOCKS + 1);
  float thre = occ_thre;
  if (consider_mean) {
    float s = 0.f;
    for (int b = 0; b < OCC_MEAN_BLOCKS; ++b) s += wk[b];
    thre = fminf(occ_thre, s / (float)nvox);
  }
  const int64_t nwords = (nvox + 31) / 32;
  if (w == 0) wk[OCC_MEAN_BLOCKS] = thre;      // (word 64 of the slice's workspace: no thread reads it)
  if (w >= nwords) return;
  uint32_t b = 0;
  for (int q = 0; q < 32; ++q) {
    const int64_t vx = w * 32 + q;
    if (vx < nvox && vk[vx] > thre) b |= (1u << q);      // (padding bits of the last word are never set)
  }
  bits[k * nwords + w] = b;
}

// ================================================================================== C ABI
static int nerf_meta_check(const NsimDistantMeta* m) {
  if (!m) return 20;
  const int rc = lotd4_meta_check(&m->lotd);
  if (rc) return rc;
  if (m->precision != 0 && m->precision != 1) return 23;
  return 0;
}

static NerfArgs nerf_args(const NsimDistantMeta* meta) {
  NerfArgs a = NerfArgs();
  a.lotd = lotd4_dev(&meta->lotd);
  a.lay = nerf_layout(meta->precision);
  a.F = 2 * meta->lotd.num_levels;
  return a;
}

static unsigned nerf_grid(int64_t S, int64_t cap) {
  const int64_t tiles = (S + 31) / 32;
  int64_t b = (tiles + NERF_WAVES - 1) / NERF_WAVES;
  b = b > cap ? cap : (b < 1 ? 1 : b);
  return (unsigned)b;
}

// forward decoders (k_nerf) of the distant model: on the gathered planes (a.h_from_planes) or with the 4-D gather fused in
static int nerf_launch_fwd(const NsimDistantMeta* meta, const NerfArgs& a, hipStream_t stream) {
  const size_t shmem = meta->precision == 0 ? (size_t)((a.lay.total + 15) & ~15) : 0;
  // persistent workgroups, one per CU (decoder part of nsim_distant_fwd per 0.52 M shells: 0.125 ms at 1024, 0.113 at 256)
  static const int fwd_grid = getenv("NSIM_NERF_FWD_GRID") ? atoi(getenv("NSIM_NERF_FWD_GRID")) : 256;
  const dim3 grid(nerf_grid(a.S, fwd_grid)), block(64 * NERF_WAVES);
  if (meta->precision == 0) hipLaunchKernelGGL((k_nerf<0, 0>), grid, block, shmem, stream, a);
  else hipLaunchKernelGGL((k_nerf<1, 0>), grid, block, shmem, stream, a);
  NSIM_CHECK_LAUNCH();
  return 0;
}

extern "C" {

int64_t nsim_distant_wpack_bytes(const NsimDistantMeta* meta) {
  if (nerf_meta_check(meta)) return -1;
  return nerf_layout(meta->precision).total;
}

int nsim_distant_pack_weights(const NsimDistantMeta* meta, const float* den_w, const float* den_b, const float* rad_w,
                              const float* rad_b, void* wpack, void* stream) {
  const int rc = nerf_meta_check(meta);
  if (rc) return rc;
  const NerfLayout L = nerf_layout(meta->precision);
  const PackShape sh = pack_shape(N_MCOUNT, kNUo, kNUi);
  const int64_t total = pack_elems(sh, N_MCOUNT, (int64_t)NV_COUNT * 64);
  hipLaunchKernelGGL(k_nerf_pack, dim3(nsim_blocks(total, 256)), dim3(256), 0, (hipStream_t)stream, L, sh,
                     2 * meta->lotd.num_levels, den_w, den_b, rad_w, rad_b, (char*)wpack);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_distant_shells(const float* rays_o, const float* rays_d, const float* near, const float* jitter, int64_t N,
                        int K, const float* aabb /* host [6]: min, max */, float r_min, float r_max, float* t,
                        float* u4, uint8_t* valid, void* stream) {
  if (N <= 0 || K <= 0) return 0;
  if (!aabb || !(r_min > 0.f) || !(r_max > r_min)) return 5;
  hipLaunchKernelGGL(k_distant_shells, dim3(nsim_blocks(N * K, 256)), dim3(256), 0, (hipStream_t)stream, rays_o, rays_d,
                     near, jitter, N, K, (aabb[0] + aabb[3]) * 0.5f, (aabb[1] + aabb[4]) * 0.5f, (aabb[2] + aabb[5]) * 0.5f,
                     (aabb[3] - aabb[0]) * 0.5f, (aabb[4] - aabb[1]) * 0.5f, (aabb[5] - aabb[2]) * 0.5f, r_min, r_max, t, u4,
                     valid);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_density_alpha_fwd(const float* sigma, const float* t, const uint8_t* valid, int64_t N, int K,
                           int include_inf_distance, float* alpha, void* stream) {
  if (N <= 0 || K <= 0) return 0;
  hipLaunchKernelGGL(k_density_alpha_fwd, dim3(nsim_blocks(N * K, 256)), dim3(256), 0, (hipStream_t)stream, sigma, t,
                     valid, N, K, include_inf_distance, alpha);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_density_alpha_bwd(const float* sigma, const float* t, const uint8_t* valid, const float* dalpha, int64_t N,
                           int K, int include_inf_distance, float* dsigma, void* stream) {
  if (N <= 0 || K <= 0) return 0;
  hipLaunchKernelGGL(k_density_alpha_bwd, dim3(nsim_blocks(N * K, 256)), dim3(256), 0, (hipStream_t)stream, sigma, t,
                     valid, dalpha, N, K, include_inf_distance, dsigma);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_distant_fwd(const NsimDistantMeta* meta, const void* grid_f16, const void* wpack, const float* u4,
                     const float* rays_d, const float* h_appear, int64_t S, int K, float* sigma, float* rgb,
                     float* h_planes, void* stream) {
  const int rc = nerf_meta_check(meta);
  if (rc) return rc;
  if (S <= 0) return 0;
  if (!u4 || !rays_d || !sigma || !rgb || K <= 0) return 4;
  NerfArgs a = nerf_args(meta);
  a.grid = (const f16*)grid_f16;
  a.wpack = (const char*)wpack;
  a.u4 = u4; a.rays_d = rays_d; a.h_appear = h_appear;
  a.S = S; a.K = K;
  a.sigma = sigma; a.rgb = rgb; a.h_pl = h_planes;
  if (h_planes) {        // training: the table reads as their own level-major launch, decoders on the planes
    Gather4Args g;
    g.lotd = a.lotd;
    g.grid = a.grid;
    g.u4 = u4;
    g.S = S;
    g.h_pl = h_planes;
    deal_levels4(&meta->lotd, g);
    const dim3 gg((unsigned)(8 * nsim_blocks(S, 64 * G4_PTS)));
    hipLaunchKernelGGL(k_lotd4_gather_lm, gg, dim3(64), 0, (hipStream_t)stream, g);
    NSIM_CHECK_LAUNCH();
    a.h_from_planes = 1;
  }
  return nerf_launch_fwd(meta, a, (hipStream_t)stream);
}

// The decoders alone, on planes another encoding has filled (nsim_permuto_gather_pts: PermutoNeRFDistant) -- the launch of
// nsim_distant_fwd's training path without its gather.
int nsim_distant_fwd_planes(const NsimDistantMeta* meta, const void* wpack, const float* h_planes, const float* rays_d,
                            const float* h_appear, int64_t S, int K, float* sigma, float* rgb, void* stream) {
  const int rc = nerf_meta_check(meta);
  if (rc) return rc;
  if (S <= 0) return 0;
  if (!wpack || !h_planes || !rays_d || !sigma || !rgb || K <= 0) return 4;
  NerfArgs a = nerf_args(meta);
  a.wpack = (const char*)wpack;
  a.rays_d = rays_d; a.h_appear = h_appear;
  a.S = S; a.K = K;
  a.sigma = sigma; a.rgb = rgb; a.h_pl = const_cast<float*>(h_planes);
  a.h_from_planes = 1;
  return nerf_launch_fwd(meta, a, (hipStream_t)stream);
}

int nsim_distant_bwd(const NsimDistantMeta* meta, const void* wpack, const float* h_planes, const float* sigma_fwd,
                     const float* rgb_fwd, const float* rays_d, const float* h_appear, const uint8_t* valid, int64_t S,
                     int K, const float* dsigma, const float* drgb, float* dh_planes, float* dden_w, float* dden_b,
                     float* drad_w, float* drad_b, float* dh_appear, void* stream) {
  const int rc = nerf_meta_check(meta);
  if (rc) return rc;
  if (S <= 0) return 0;
  if (!h_planes || !sigma_fwd || !rgb_fwd || !rays_d || !valid) return 28;
  if (!dden_w || !dden_b || !drad_w || !drad_b) return 26;
  NerfArgs a = nerf_args(meta);
  a.wpack = (const char*)wpack;
  a.rays_d = rays_d; a.h_appear = h_appear; a.valid = valid;
  a.S = S; a.K = K;
  a.h_pl = const_cast<float*>(h_planes);
  a.sigma_fwd = sigma_fwd; a.rgb_fwd = rgb_fwd;
  a.dsigma = dsigma; a.drgb = drgb;
  a.dh_pl = dh_planes;
  a.dden_w = dden_w; a.dden_b = dden_b; a.drad_w = drad_w; a.drad_b = drad_b; a.dh_appear = dh_appear;
  const size_t st = meta->precision == 0 ? stage_bytes_per_wave<0>() : stage_bytes_per_wave<1>();
  const size_t acc = (10700 * 4 + 15) & ~15;
  const bool priv = meta->precision == 0;
  const int nw = priv ? NERF_WAVES_PRIV : NERF_WAVES;
  const size_t vec_bytes = (size_t)((a.lay.total - a.lay.vec[0] + 15) & ~15);
  const size_t shmem = priv ? vec_bytes + nw * acc + nw * st : acc + nw * st;
  const int64_t tiles = (S + 31) / 32;
  int64_t nb = (tiles + nw - 1) / nw;
  nb = nb > 256 ? 256 : (nb < 1 ? 1 : nb);
  const dim3 grid((unsigned)nb), block(64 * nw);
  if (meta->precision == 0) hipLaunchKernelGGL((k_nerf<0, 1>), grid, block, shmem, (hipStream_t)stream, a);
  else hipLaunchKernelGGL((k_nerf<1, 1>), grid, block, shmem, (hipStream_t)stream, a);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_lotd4_scatter(const NsimLotd4Meta* meta, const float* u4, const uint8_t* valid, int64_t S,
                       const float* dh_planes, float* dgrid, void* stream) {
  const int rc = lotd4_meta_check(meta);
  if (rc) return rc;
  if (S <= 0) return 0;
  if (!u4 || !valid || !dh_planes || !dgrid) return 28;
  Scatter4Args sa;
  sa.lotd = lotd4_dev(meta);
  sa.u4 = u4; sa.valid = valid; sa.S = S; sa.dh_pl = dh_planes; sa.dgrid = dgrid;
  sa.dedup_max_rw = 1 << 30;
  sa.parity_slots = 1;
  const dim3 grid(nsim_blocks((S + 63) / 64, 4, 4096), meta->num_levels);
  hipLaunchKernelGGL(k_lotd4_scatter, grid, dim3(256), 0, (hipStream_t)stream, sa);
  NSIM_CHECK_LAUNCH();
  return 0;
}


// ------------------------------------------------------------------------------ close-range NGP NeRF (LoTDNeRFModel)
static int ngp_meta_check(const NsimNgpMeta* m) {
  if (!m) return 20;
  const int rc = lotd_meta_check(&m->lotd);
  if (rc) return rc;
  if (m->lotd.num_levels > 16) return 38;
  if (m->precision != 0 && m->precision != 1) return 23;
  if (m->n_appear != 0 && m->n_appear != 4) return 39;
  return 0;
}

static NgpArgs ngp_args(const NsimNgpMeta* meta) {
  NgpArgs a = NgpArgs();
  const LotdDev d = lotd_dev(&meta->lotd);
  a.lay = ngp_layout(meta->precision);
  a.NL = meta->lotd.num_levels;
  a.F = 2 * a.NL;
  a.n_active = d.n_active;
  a.NA = meta->n_appear;
  for (int c = 0; c < 3; ++c) {
    a.xs[c] = d.xs[c];
    a.xb[c] = d.xb[c];
  }
  return a;
}

// the replica scratch of nsim_set_grad_scratch (field.hip), for a launch of nb workgroups adding n floats
float* nsim_grad_scratch_acquire(void* stream, int64_t n, int64_t nb, int* R);
void nsim_grad_scratch_fold(float* sc, int R, int64_t stride, int64_t n_w, int64_t n_b, float* dst_w, float* dst_b, void* stream);

int64_t nsim_ngp_wpack_bytes(const NsimNgpMeta* meta) {
  if (ngp_meta_check(meta)) return -1;
  return ngp_layout(meta->precision).total;
}

int nsim_ngp_pack_weights(const NsimNgpMeta* meta, const float* den_w, const float* den_b, const float* rad_w,
                          const float* rad_b, void* wpack, void* stream) {
  const int rc = ngp_meta_check(meta);
  if (rc) return rc;
  if (!den_w || !den_b || !rad_w || !rad_b || !wpack) return 4;
  const NgpLayout L = ngp_layout(meta->precision);
  const PackShape sh = pack_shape(G_MCOUNT, kGUo, kGUi);
  const int64_t total = pack_elems(sh, G_MCOUNT, (int64_t)GV_COUNT * 64);
  hipLaunchKernelGGL(k_ngp_pack, dim3(nsim_blocks(total, 256)), dim3(256), 0, (hipStream_t)stream, L, sh,
                     2 * meta->lotd.num_levels, meta->n_appear, den_w, den_b, rad_w, rad_b, (char*)wpack);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_ngp_fwd(const NsimNgpMeta* meta, const void* wpack, const float* h_planes, int64_t plane_pitch, const float* x,
                 const float* rays_o, const float* rays_d, const float* t, const int64_t* ridx, const float* h_appear,
                 int64_t S, float step, float* sigma, float* alpha, float* rgb, void* stream) {
  const int rc = ngp_meta_check(meta);
  if (rc) return rc;
  if (S <= 0) return 0;
  if (!wpack || !sigma) return 4;
  if (!h_planes) return 28;
  if (!x && !(rays_o && rays_d && t && ridx)) return 24;
  if (rgb && !(rays_d && ridx)) return 25;
  NgpArgs a = ngp_args(meta);
  a.wpack = (const char*)wpack;
  a.h_pl = h_planes;
  a.PS = plane_pitch > 0 ? plane_pitch : NSIM_PLANE_PITCH(S);
  a.x = x; a.rays_o = rays_o; a.rays_d = rays_d; a.t = t; a.ridx = ridx; a.h_appear = h_appear;
  a.S = S; a.step = step;
  a.sigma = sigma; a.alpha = alpha; a.rgb = rgb;
  const size_t shmem = meta->precision == 0 ? (size_t)((a.lay.fwd_end + 15) & ~15) : 0;
  const int64_t tiles = (S + 31) / 32;
  int64_t nb = (tiles + NGP_WAVES - 1) / NGP_WAVES;
  nb = nb > 512 ? 512 : (nb < 1 ? 1 : nb);       // persistent workgroups: 31 KB of LDS each, two per CU
  const dim3 grid((unsigned)nb), block(64 * NGP_WAVES);
  if (meta->precision == 0) hipLaunchKernelGGL((k_ngp<0, 0>), grid, block, shmem, (hipStream_t)stream, a);
  else hipLaunchKernelGGL((k_ngp<1, 0>), grid, block, shmem, (hipStream_t)stream, a);
  NSIM_CHECK_LAUNCH();
  return 0;
}

// nsim_ngp_bwd (pose == false) | nsim_ngp_bwd_pose (pose: dx [S,3] and, with a colour gradient, dv [S,3] as well)
static int ngp_bwd(const NsimNgpMeta* meta, const void* wpack, const float* h_planes, int64_t plane_pitch, const float* x,
                   const float* rays_o, const float* rays_d, const float* t, const int64_t* ridx, const float* h_appear,
                   int64_t S, float step, const float* sigma_fwd, const float* rgb_fwd, const float* dsigma,
                   const float* dalpha, const float* drgb, float* dh_planes, float* dden_w, float* dden_b, float* drad_w,
                   float* drad_b, float* dh_appear, bool pose, float* dx, float* dv, void* stream) {
  const int rc = ngp_meta_check(meta);
  if (rc) return rc;
  if (S <= 0) return 0;
  if (!wpack || !h_planes || !sigma_fwd) return 28;
  if (pose && (!dx || (dv && !drgb))) return 4;
  if (pose && !dh_planes) return 28;          // the next launch (nsim_lotd_dx_lm) reads them
  if (!x && !(rays_o && rays_d && t && ridx)) return 24;
  if (drgb && !(rays_d && ridx && rgb_fwd)) return 25;
  if (!dden_w || !dden_b || (drgb && (!drad_w || !drad_b))) return 26;
  NgpArgs a = ngp_args(meta);
  a.wpack = (const char*)wpack;
  a.h_pl = h_planes;
  a.PS = plane_pitch > 0 ? plane_pitch : NSIM_PLANE_PITCH(S);
  a.x = x; a.rays_o = rays_o; a.rays_d = rays_d; a.t = t; a.ridx = ridx; a.h_appear = h_appear;
  a.S = S; a.step = step;
  a.sigma_fwd = sigma_fwd; a.rgb_fwd = rgb_fwd;
  a.dsigma = dsigma; a.dalpha = dalpha; a.drgb = drgb;
  a.dh_pl = dh_planes;
  a.dh_appear = dh_appear;
  a.dx = dx; a.dv = dv;
  const bool priv = meta->precision == 0;
  const size_t st = priv ? stage_bytes_per_wave<0>() : stage_bytes_per_wave<1>();
  const size_t acc = (12900 * 4 + 15) & ~15;
  const size_t vec_bytes = (size_t)((a.lay.mat[0] + 15) & ~15);
  const size_t shmem = priv ? vec_bytes + NGP_WAVES_BWD * acc + NGP_WAVES_BWD * st : acc + NGP_WAVES_BWD * st;
  const int64_t tiles = (S + 31) / 32;
  int64_t nb = (tiles + NGP_WAVES_BWD - 1) / NGP_WAVES_BWD;
  nb = nb > 256 ? 256 : (nb < 1 ? 1 : nb);       // one workgroup per CU (125 KB of LDS)
  const int FI = 2 * meta->lotd.num_levels + 3, K1 = 47 + meta->n_appear;
  const int64_t n[4] = {64 * FI + 2048, 96, drgb ? 64 * K1 + 4096 + 192 : 0, drgb ? 131 : 0};
  const int64_t n_all = n[0] + n[1] + n[2] + n[3];
  int R = 1;
  float* sc = nsim_grad_scratch_acquire(stream, n_all, nb, &R);
  if (sc) {        // workgroup b adds into replica b % R of the registered scratch; k_ngp_fold sums them up
    a.dst[0] = sc; a.dst[1] = sc + n[0]; a.dst[2] = sc + n[0] + n[1]; a.dst[3] = sc + n[0] + n[1] + n[2];
    a.rep_stride = n_all;
    a.rep_mask = R - 1;
  } else {
    a.dst[0] = dden_w; a.dst[1] = dden_b; a.dst[2] = drad_w; a.dst[3] = drad_b;
    a.rep_stride = 0;
    a.rep_mask = 0;
  }
  const dim3 grid((unsigned)nb), block(64 * NGP_WAVES_BWD);
  if (pose) {
    if (priv) hipLaunchKernelGGL((k_ngp<0, 1, true>), grid, block, shmem, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((k_ngp<1, 1, true>), grid, block, shmem, (hipStream_t)stream, a);
  } else {
    if (priv) hipLaunchKernelGGL((k_ngp<0, 1>), grid, block, shmem, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((k_ngp<1, 1>), grid, block, shmem, (hipStream_t)stream, a);
  }
  NSIM_CHECK_LAUNCH();
  if (sc) {      // the replicas of [den_w | den_b] and of [rad_w | rad_b] folded by field.hip's reduction (which zeroes them again)
    nsim_grad_scratch_fold(sc, R, n_all, n[0], n[1], dden_w, dden_b, stream);
    if (drgb) nsim_grad_scratch_fold(sc + n[0] + n[1], R, n_all, n[2], n[3], drad_w, drad_b, stream);
    NSIM_CHECK_LAUNCH();
  }
  return 0;
}

int nsim_ngp_bwd(const NsimNgpMeta* meta, const void* wpack, const float* h_planes, int64_t plane_pitch, const float* x,
                 const float* rays_o, const float* rays_d, const float* t, const int64_t* ridx, const float* h_appear,
                 int64_t S, float step, const float* sigma_fwd, const float* rgb_fwd, const float* dsigma,
                 const float* dalpha, const float* drgb, float* dh_planes, float* dden_w, float* dden_b, float* drad_w,
                 float* drad_b, float* dh_appear, void* stream) {
  return ngp_bwd(meta, wpack, h_planes, plane_pitch, x, rays_o, rays_d, t, ridx, h_appear, S, step, sigma_fwd, rgb_fwd, dsigma,
                 dalpha, drgb, dh_planes, dden_w, dden_b, drad_w, drad_b, dh_appear, false, nullptr, nullptr, stream);
}

int nsim_ngp_bwd_pose(const NsimNgpMeta* meta, const void* wpack, const float* h_planes, int64_t plane_pitch, const float* x,
                      const float* rays_o, const float* rays_d, const float* t, const int64_t* ridx, const float* h_appear,
                      int64_t S, float step, const float* sigma_fwd, const float* rgb_fwd, const float* dsigma,
                      const float* dalpha, const float* drgb, float* dh_planes, float* dden_w, float* dden_b, float* drad_w,
                      float* drad_b, float* dh_appear, float* dx, float* dv, void* stream) {
  return ngp_bwd(meta, wpack, h_planes, plane_pitch, x, rays_o, rays_d, t, ridx, h_appear, S, step, sigma_fwd, rgb_fwd, dsigma,
                 dalpha, drgb, dh_planes, dden_w, dden_b, drad_w, drad_b, dh_appear, true, dx, dv, stream);
}

int nsim_lotd_dx_lm(const NsimLotdMeta* meta, const void* grid_f16, const float* x, const float* rays_o, const float* rays_d,
                    const float* t, const int64_t* ridx, int64_t S, const float* dh_planes, int64_t plane_pitch,
                    const float* dx_add, float* dx, void* stream) {
  const int rc = lotd_meta_check(meta);
  if (rc) return rc;
  if (meta->num_levels > 16) return 38;           // the planes hold 16 levels
  if (S <= 0) return 0;
  if (!x && !(rays_o && rays_d && t && ridx)) return 24;
  if (!grid_f16 || !dx) return 4;
  if (!dh_planes || (plane_pitch != 0 && plane_pitch < S)) return 28;
  LotdDxArgs a;
  a.lotd = lotd_dev(meta);
  a.grid = (const f16*)grid_f16;
  a.x = x; a.rays_o = rays_o; a.rays_d = rays_d; a.t = t; a.ridx = ridx;
  a.S = S;
  a.PS = plane_pitch ? plane_pitch : S;
  a.dh_pl = dh_planes; a.dx_add = dx_add; a.dx = dx;
  hipLaunchKernelGGL(k_lotd_dx_lm, dim3(nsim_blocks(S, 256)), dim3(256), 0, (hipStream_t)stream, a);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_occ_update_density(float* val, int64_t nvox, float decay, const float* pts, const float* sigma, int64_t n,
                            const NsimOccMeta* meta, void* stream) {
  if (nvox <= 0) return 0;
  if (!meta || !val) return 5;
  hipLaunchKernelGGL(k_occ_scale, dim3(nsim_blocks(nvox, 256)), dim3(256), 0, (hipStream_t)stream, val, nvox, decay);
  NSIM_CHECK_LAUNCH();
  if (n <= 0) return 0;
  if (!pts || !sigma) return 4;
  hipLaunchKernelGGL(k_occ_max_density, dim3(nsim_blocks(n, 256)), dim3(256), 0, (hipStream_t)stream, val, pts,
                     (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, (const int64_t*)nullptr, sigma, n,
                     occ_dev(meta));
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_occ_collect_density(float* val, const float* x, const float* rays_o, const float* rays_d, const float* t,
                             const int64_t* ridx, const float* sigma, int64_t n, const NsimOccMeta* meta, void* stream) {
  if (n <= 0) return 0;
  if (!meta || !val) return 5;
  if (!sigma) return 4;
  if (!x && !(rays_o && rays_d && t && ridx)) return 24;
  hipLaunchKernelGGL(k_occ_max_density, dim3(nsim_blocks(n, 256)), dim3(256), 0, (hipStream_t)stream, val, x, rays_o,
                     rays_d, t, ridx, sigma, n, occ_dev(meta));
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_occ_pack_bits_mean(const float* val, int64_t nvox, float occ_thre, int consider_mean, float* workspace,
                            uint32_t* bits, void* stream) {
  if (nvox <= 0) return 0;
  if (!val || !bits || !workspace) return 4;
  if (consider_mean) {
    hipLaunchKernelGGL(k_occ_partial_sum, dim3(OCC_MEAN_BLOCKS), dim3(256), 0, (hipStream_t)stream, val, nvox, workspace);
    NSIM_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(k_occ_pack_bits_mean, dim3(nsim_blocks((nvox + 31) / 32, 256)), dim3(256), 0, (hipStream_t)stream, val,
                     nvox, occ_thre, consider_mean, workspace, bits, workspace + OCC_MEAN_BLOCKS);
  NSIM_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------ dynamic-only EmerNeRF
static DynArgs dyn_args(const NsimNgpMeta* meta) {
  DynArgs a = DynArgs();
  a.lay = dyn_layout(meta->precision);
  a.NL = meta->lotd.num_levels;
  a.F = 2 * a.NL;
  a.n_active = (meta->lotd.n_active_levels > 0 && meta->lotd.n_active_levels < a.NL) ? meta->lotd.n_active_levels : a.NL;
  a.NA = meta->n_appear;
  return a;
}

int64_t nsim_dyn_wpack_bytes(const NsimNgpMeta* meta) {
  if (ngp_meta_check(meta)) return -1;
  return dyn_layout(meta->precision).total;
}

int nsim_dyn_pack_weights(const NsimNgpMeta* meta, const float* den_w, const float* den_b, const float* rad_w,
                          const float* rad_b, void* wpack, void* stream) {
  const int rc = ngp_meta_check(meta);
  if (rc) return rc;
  if (!den_w || !den_b || !rad_w || !rad_b || !wpack) return 4;
  const NgpLayout L = dyn_layout(meta->precision);
  const PackShape sh = pack_shape(Y_MCOUNT, kYUo, kYUi);
  const int64_t total = pack_elems(sh, Y_MCOUNT, (int64_t)YV_COUNT * 64);
  hipLaunchKernelGGL(k_dyn_pack, dim3(nsim_blocks(total, 256)), dim3(256), 0, (hipStream_t)stream, L, sh,
                     2 * meta->lotd.num_levels, meta->n_appear, den_w, den_b, rad_w, rad_b, (char*)wpack);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_dyn_fwd(const NsimNgpMeta* meta, const void* wpack, const float* h_planes, int64_t plane_pitch, const float* rays_d,
                 const int64_t* ridx, const float* h_appear, int64_t S, float step, float* sigma, float* alpha, float* rgb,
                 void* stream) {
  const int rc = ngp_meta_check(meta);
  if (rc) return rc;
  if (S <= 0) return 0;
  if (!wpack || !sigma) return 4;
  if (!h_planes) return 28;
  if (rgb && !(rays_d && ridx)) return 25;
  DynArgs a = dyn_args(meta);
  a.wpack = (const char*)wpack;
  a.h_pl = h_planes;
  a.PS = plane_pitch > 0 ? plane_pitch : S;
  a.rays_d = rays_d; a.ridx = ridx; a.h_appear = h_appear;
  a.S = S; a.step = step;
  a.sigma = sigma; a.alpha = alpha; a.rgb = rgb;
  const size_t shmem = meta->precision == 0 ? (size_t)((a.lay.fwd_end + 15) & ~15) : 0;
  const int64_t tiles = (S + 31) / 32;
  int64_t nb = (tiles + DYN_WAVES - 1) / DYN_WAVES;
  nb = nb > 512 ? 512 : (nb < 1 ? 1 : nb);       // persistent workgroups: 38 KB of LDS each, two per CU
  const dim3 grid((unsigned)nb), block(64 * DYN_WAVES);
  if (meta->precision == 0) hipLaunchKernelGGL((k_dyn<0, 0>), grid, block, shmem, (hipStream_t)stream, a);
  else hipLaunchKernelGGL((k_dyn<1, 0>), grid, block, shmem, (hipStream_t)stream, a);
  NSIM_CHECK_LAUNCH();
  return 0;
}

// nsim_dyn_bwd | nsim_dyn_bwd_agg (agg: the three plane sets at pitch 3S) | their _pose forms (dv [S,3]; needs drgb)
static int dyn_bwd(const NsimNgpMeta* meta, const void* wpack, const float* h_planes, int64_t plane_pitch, const float* rays_d,
                   const int64_t* ridx, const float* h_appear, int64_t S, float step, const float* sigma_fwd, const float* rgb_fwd,
                   const float* dsigma, const float* dalpha, const float* drgb, float* dh_planes, float* dden_w, float* dden_b,
                   float* drad_w, float* drad_b, float* dh_appear, bool agg, float* dv, void* stream) {
  const int rc = ngp_meta_check(meta);
  if (rc) return rc;
  if (S <= 0) return 0;
  if (!wpack || !h_planes || !sigma_fwd) return 28;
  if (drgb && !(rays_d && ridx && rgb_fwd)) return 25;
  if (!dden_w || !dden_b || (drgb && (!drad_w || !drad_b))) return 26;
  if (dv && !drgb) return 25;
  if (dv && !dh_planes) return 28;            // the pose forms hand the planes to nsim_permuto_dx_pts
  DynArgs a = dyn_args(meta);
  a.wpack = (const char*)wpack;
  a.h_pl = h_planes;
  a.PS = agg ? 3 * S : (plane_pitch > 0 ? plane_pitch : S);
  a.rays_d = rays_d; a.ridx = ridx; a.h_appear = h_appear;
  a.S = S; a.step = step;
  a.sigma_fwd = sigma_fwd; a.rgb_fwd = rgb_fwd;
  a.dsigma = dsigma; a.dalpha = dalpha; a.drgb = drgb;
  a.dh_pl = dh_planes;
  a.dh_appear = dh_appear;
  a.dv = dv;
  const bool priv = meta->precision == 0;
  const size_t st = priv ? stage_bytes_per_wave<0>() : stage_bytes_per_wave<1>();
  const size_t acc = (16904 * 4 + 15) & ~15;
  const size_t vec_bytes = (size_t)((a.lay.mat[0] + 15) & ~15);
  const size_t shmem = priv ? vec_bytes + DYN_WAVES_BWD * acc + DYN_WAVES_BWD * st : acc + DYN_WAVES_BWD * st;
  const int64_t tiles = (S + 31) / 32;
  int64_t nb = (tiles + DYN_WAVES_BWD - 1) / DYN_WAVES_BWD;
  nb = nb > 256 ? 256 : (nb < 1 ? 1 : nb);       // one workgroup per CU (154 KB of LDS in fp16 mode)
  const int F = 2 * meta->lotd.num_levels, K1 = 80 + meta->n_appear;
  const int64_t n[4] = {64 * F + 65 * 64, 129, drgb ? 64 * K1 + 4096 + 192 : 0, drgb ? 131 : 0};
  const int64_t n_all = n[0] + n[1] + n[2] + n[3];
  int R = 1;
  float* sc = nsim_grad_scratch_acquire(stream, n_all, nb, &R);
  if (sc) {        // workgroup b adds into replica b % R of the registered scratch, folded below
    a.dst[0] = sc; a.dst[1] = sc + n[0]; a.dst[2] = sc + n[0] + n[1]; a.dst[3] = sc + n[0] + n[1] + n[2];
    a.rep_stride = n_all;
    a.rep_mask = R - 1;
  } else {
    a.dst[0] = dden_w; a.dst[1] = dden_b; a.dst[2] = drad_w; a.dst[3] = drad_b;
    a.rep_stride = 0;
    a.rep_mask = 0;
  }
  const dim3 grid((unsigned)nb), block(64 * DYN_WAVES_BWD);
  switch ((dv ? 4 : 0) + (agg ? 2 : 0) + (priv ? 0 : 1)) {
    case 0: hipLaunchKernelGGL((k_dyn<0, 1>), grid, block, shmem, (hipStream_t)stream, a); break;
    case 1: hipLaunchKernelGGL((k_dyn<1, 1>), grid, block, shmem, (hipStream_t)stream, a); break;
    case 2: hipLaunchKernelGGL((k_dyn<0, 1, true>), grid, block, shmem, (hipStream_t)stream, a); break;
    case 3: hipLaunchKernelGGL((k_dyn<1, 1, true>), grid, block, shmem, (hipStream_t)stream, a); break;
    case 4: hipLaunchKernelGGL((k_dyn<0, 1, false, true>), grid, block, shmem, (hipStream_t)stream, a); break;
    case 5: hipLaunchKernelGGL((k_dyn<1, 1, false, true>), grid, block, shmem, (hipStream_t)stream, a); break;
    case 6: hipLaunchKernelGGL((k_dyn<0, 1, true, true>), grid, block, shmem, (hipStream_t)stream, a); break;
    case 7: hipLaunchKernelGGL((k_dyn<1, 1, true, true>), grid, block, shmem, (hipStream_t)stream, a); break;
  }
  NSIM_CHECK_LAUNCH();
  if (sc) {
    nsim_grad_scratch_fold(sc, R, n_all, n[0], n[1], dden_w, dden_b, stream);
    if (drgb) nsim_grad_scratch_fold(sc + n[0] + n[1], R, n_all, n[2], n[3], drad_w, drad_b, stream);
    NSIM_CHECK_LAUNCH();
  }
  return 0;
}

int nsim_dyn_bwd(const NsimNgpMeta* meta, const void* wpack, const float* h_planes, int64_t plane_pitch, const float* rays_d,
                 const int64_t* ridx, const float* h_appear, int64_t S, float step, const float* sigma_fwd, const float* rgb_fwd,
                 const float* dsigma, const float* dalpha, const float* drgb, float* dh_planes, float* dden_w, float* dden_b,
                 float* drad_w, float* drad_b, float* dh_appear, void* stream) {
  return dyn_bwd(meta, wpack, h_planes, plane_pitch, rays_d, ridx, h_appear, S, step, sigma_fwd, rgb_fwd, dsigma, dalpha, drgb,
                 dh_planes, dden_w, dden_b, drad_w, drad_b, dh_appear, false, nullptr, stream);
}

int nsim_dyn_bwd_pose(const NsimNgpMeta* meta, const void* wpack, const float* h_planes, int64_t plane_pitch, const float* rays_d,
                      const int64_t* ridx, const float* h_appear, int64_t S, float step, const float* sigma_fwd,
                      const float* rgb_fwd, const float* dsigma, const float* dalpha, const float* drgb, float* dh_planes,
                      float* dden_w, float* dden_b, float* drad_w, float* drad_b, float* dh_appear, float* dv, void* stream) {
  if (S > 0 && !dv) return 4;
  return dyn_bwd(meta, wpack, h_planes, plane_pitch, rays_d, ridx, h_appear, S, step, sigma_fwd, rgb_fwd, dsigma, dalpha, drgb,
                 dh_planes, dden_w, dden_b, drad_w, drad_b, dh_appear, false, dv, stream);
}

// the aggregating variants (the with-flow model): h_planes [16][3S][2] holds the plane sets of the samples (rows 0..S), of their
// forward-warped (S..2S) and backward-warped (2S..3S) neighbours; dh_planes is written in the same layout
int nsim_dyn_fwd_agg(const NsimNgpMeta* meta, const void* wpack, const float* h_planes, const float* rays_d, const int64_t* ridx,
                     const float* h_appear, int64_t S, float step, float* sigma, float* alpha, float* rgb, void* stream) {
  const int rc = ngp_meta_check(meta);
  if (rc) return rc;
  if (S <= 0) return 0;
  if (!wpack || !sigma) return 4;
  if (!h_planes) return 28;
  if (rgb && !(rays_d && ridx)) return 25;
  DynArgs a = dyn_args(meta);
  a.wpack = (const char*)wpack;
  a.h_pl = h_planes;
  a.PS = 3 * S;
  a.rays_d = rays_d; a.ridx = ridx; a.h_appear = h_appear;
  a.S = S; a.step = step;
  a.sigma = sigma; a.alpha = alpha; a.rgb = rgb;
  const size_t shmem = meta->precision == 0 ? (size_t)((a.lay.fwd_end + 15) & ~15) : 0;
  const int64_t tiles = (S + 31) / 32;
  int64_t nb = (tiles + DYN_WAVES - 1) / DYN_WAVES;
  nb = nb > 512 ? 512 : (nb < 1 ? 1 : nb);
  const dim3 grid((unsigned)nb), block(64 * DYN_WAVES);
  if (meta->precision == 0) hipLaunchKernelGGL((k_dyn<0, 0, true>), grid, block, shmem, (hipStream_t)stream, a);
  else hipLaunchKernelGGL((k_dyn<1, 0, true>), grid, block, shmem, (hipStream_t)stream, a);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_dyn_bwd_agg(const NsimNgpMeta* meta, const void* wpack, const float* h_planes, const float* rays_d, const int64_t* ridx,
                     const float* h_appear, int64_t S, float step, const float* sigma_fwd, const float* rgb_fwd,
                     const float* dsigma, const float* dalpha, const float* drgb, float* dh_planes, float* dden_w, float* dden_b,
                     float* drad_w, float* drad_b, float* dh_appear, void* stream) {
  return dyn_bwd(meta, wpack, h_planes, 0, rays_d, ridx, h_appear, S, step, sigma_fwd, rgb_fwd, dsigma, dalpha, drgb, dh_planes,
                 dden_w, dden_b, drad_w, drad_b, dh_appear, true, nullptr, stream);
}

int nsim_dyn_bwd_agg_pose(const NsimNgpMeta* meta, const void* wpack, const float* h_planes, const float* rays_d,
                          const int64_t* ridx, const float* h_appear, int64_t S, float step, const float* sigma_fwd,
                          const float* rgb_fwd, const float* dsigma, const float* dalpha, const float* drgb, float* dh_planes,
                          float* dden_w, float* dden_b, float* drad_w, float* drad_b, float* dh_appear, float* dv, void* stream) {
  if (S > 0 && !dv) return 4;
  return dyn_bwd(meta, wpack, h_planes, 0, rays_d, ridx, h_appear, S, step, sigma_fwd, rgb_fwd, dsigma, dalpha, drgb, dh_planes,
                 dden_w, dden_b, drad_w, drad_b, dh_appear, true, dv, stream);
}

// ------------------------------------------------------------------------------ scene-flow decoder, warp
static int flow_check(int num_levels, int precision) {
  if (num_levels < 1 || num_levels > 16) return 42;
  if (precision != 0 && precision != 1) return 21;
  return 0;
}

static FlowArgs flow_args(int num_levels, int precision) {
  FlowArgs a = FlowArgs();
  a.lay = flow_layout(precision);
  a.NL = num_levels;
  a.F = 2 * num_levels;
  a.n_active = num_levels;
  return a;
}

int64_t nsim_flow_wpack_bytes(int precision) {
  if (precision != 0 && precision != 1) return -1;
  return flow_layout(precision).total;
}

int nsim_flow_pack_weights(int num_levels, int precision, const float* flow_w, const float* flow_b, void* wpack, void* stream) {
  const int rc = flow_check(num_levels, precision);
  if (rc) return rc;
  if (!flow_w || !flow_b || !wpack) return 4;
  const FlowLayout L = flow_layout(precision);
  const PackShape sh = pack_shape(F_MCOUNT, kFUo, kFUi);
  const int64_t total = pack_elems(sh, F_MCOUNT, (int64_t)FV_COUNT * 64);
  hipLaunchKernelGGL(k_flow_pack, dim3(nsim_blocks(total, 256)), dim3(256), 0, (hipStream_t)stream, L, sh, 2 * num_levels, flow_w,
                     flow_b, (char*)wpack);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_flow_fwd(int num_levels, int precision, const void* wpack, const float* h_planes, int64_t plane_pitch, int64_t S,
                  float* flow6, void* stream) {
  const int rc = flow_check(num_levels, precision);
  if (rc) return rc;
  if (S <= 0) return 0;
  if (!wpack || !flow6) return 4;
  if (!h_planes) return 28;
  if (plane_pitch != 0 && plane_pitch < S) return 2;
  FlowArgs a = flow_args(num_levels, precision);
  a.wpack = (const char*)wpack;
  a.h_pl = h_planes;
  a.PS = plane_pitch > 0 ? plane_pitch : S;
  a.S = S;
  a.flow6 = flow6;
  const size_t shmem = precision == 0 ? (size_t)((a.lay.fwd_end + 15) & ~15) : 0;
  const int64_t tiles = (S + 31) / 32;
  int64_t nb = (tiles + FLOW_WAVES - 1) / FLOW_WAVES;
  nb = nb > 1024 ? 1024 : (nb < 1 ? 1 : nb);     // persistent workgroups: 15 KB of LDS each
  const dim3 grid((unsigned)nb), block(64 * FLOW_WAVES);
  if (precision == 0) hipLaunchKernelGGL((k_flow<0, 0>), grid, block, shmem, (hipStream_t)stream, a);
  else hipLaunchKernelGGL((k_flow<1, 0>), grid, block, shmem, (hipStream_t)stream, a);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_flow_bwd(int num_levels, int precision, const void* wpack, const float* h_planes, int64_t plane_pitch, int64_t S,
                  const float* dflow6, float* dh_planes, float* dflow_w, float* dflow_b, void* stream) {
  const int rc = flow_check(num_levels, precision);
  if (rc) return rc;
  if (S <= 0) return 0;
  if (!wpack || !h_planes || !dflow6) return 28;
  if (!dflow_w || !dflow_b) return 26;
  if (plane_pitch != 0 && plane_pitch < S) return 2;
  FlowArgs a = flow_args(num_levels, precision);
  a.wpack = (const char*)wpack;
  a.h_pl = h_planes;
  a.PS = plane_pitch > 0 ? plane_pitch : S;
  a.S = S;
  a.dflow6 = dflow6;
  a.dh_pl = dh_planes;
  const bool priv = precision == 0;
  const size_t st = priv ? stage_bytes_per_wave<0>() : stage_bytes_per_wave<1>();
  const size_t acc = (6664 * 4 + 15) & ~15;
  const size_t vec_bytes = (size_t)((a.lay.mat[0] + 15) & ~15);
  const size_t shmem = priv ? vec_bytes + FLOW_WAVES_BWD * acc + FLOW_WAVES_BWD * st : acc + FLOW_WAVES_BWD * st;
  const int64_t tiles = (S + 31) / 32;
  int64_t nb = (tiles + FLOW_WAVES_BWD - 1) / FLOW_WAVES_BWD;
  nb = nb > 512 ? 512 : (nb < 1 ? 1 : nb);       // two workgroups per CU (76 KB of LDS in fp16 mode)
  const int F = 2 * num_levels;
  const int64_t n[2] = {64 * F + 4096 + 384, 134};
  const int64_t n_all = n[0] + n[1];
  int R = 1;
  float* sc = nsim_grad_scratch_acquire(stream, n_all, nb, &R);
  if (sc) {        // workgroup b adds into replica b % R of the registered scratch, folded below
    a.dst[0] = sc; a.dst[1] = sc + n[0];
    a.rep_stride = n_all;
    a.rep_mask = R - 1;
  } else {
    a.dst[0] = dflow_w; a.dst[1] = dflow_b;
    a.rep_stride = 0;
    a.rep_mask = 0;
  }
  const dim3 grid((unsigned)nb), block(64 * FLOW_WAVES_BWD);
  if (priv) hipLaunchKernelGGL((k_flow<0, 1>), grid, block, shmem, (hipStream_t)stream, a);
  else hipLaunchKernelGGL((k_flow<1, 1>), grid, block, shmem, (hipStream_t)stream, a);
  NSIM_CHECK_LAUNCH();
  if (sc) {
    nsim_grad_scratch_fold(sc, R, n_all, n[0], n[1], dflow_w, dflow_b, stream);
    NSIM_CHECK_LAUNCH();
  }
  return 0;
}

int nsim_dyn_warp_fwd(const float* x4, const float* flow6, int64_t S, float delta, float code_lo, float code_hi, float* x4w,
                      void* stream) {
  if (S <= 0) return 0;
  if (!x4 || !flow6 || !x4w) return 4;
  hipLaunchKernelGGL(k_dyn_warp_fwd, dim3(nsim_blocks(S, 256)), dim3(256), 0, (hipStream_t)stream, x4, flow6, S, delta, code_lo,
                     code_hi, x4w);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_dyn_warp_bwd(const float* dx4w, int64_t S, float* dflow6, void* stream) {
  if (S <= 0) return 0;
  if (!dx4w || !dflow6) return 4;
  hipLaunchKernelGGL(k_dyn_warp_bwd, dim3(nsim_blocks(S, 256)), dim3(256), 0, (hipStream_t)stream, dx4w, S, dflow6);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_dyn_pose_dx(const float* dx4_dyn, const float* dx4_flow, const float* dx4w_dyn, const float* dx4w_flow, int64_t S,
                     float* dx, void* stream) {
  if (S <= 0) return 0;
  if (!dx) return 4;
  hipLaunchKernelGGL(k_dyn_pose_dx, dim3(nsim_blocks(S, 256)), dim3(256), 0, (hipStream_t)stream, dx4_dyn, dx4_flow, dx4w_dyn,
                     dx4w_flow, S, dx);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_dyn_time(const float* keyframes, const float* codes, int T, const float* ts, int64_t n, int64_t words_per_slice,
                  float* w, int64_t* slice, int64_t* word_off, void* stream) {
  if (n <= 0) return 0;
  if (!keyframes || !ts || T < 1) return 4;
  if (w && !codes) return 4;
  hipLaunchKernelGGL(k_dyn_time, dim3(nsim_blocks(n, 256)), dim3(256), 0, (hipStream_t)stream, keyframes, codes, T, ts, n,
                     words_per_slice, w, slice, word_off);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_dyn_points(const float* x, const float* rays_o, const float* rays_d, const float* t, const int64_t* ridx,
                    const float* w, int64_t S, float* x4, void* stream) {
  if (S <= 0) return 0;
  if (!w || !x4) return 4;
  if (!x && !(rays_o && rays_d && t && ridx)) return 24;
  hipLaunchKernelGGL(k_dyn_points, dim3(nsim_blocks(S, 256)), dim3(256), 0, (hipStream_t)stream, x, rays_o, rays_d, t, ridx, w,
                     S, x4);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_occ_update_density_sliced(float* val, int64_t nvox, int64_t slice_stride, int K, float decay, const float* pts,
                                   const float* sigma, const int64_t* slice, int64_t n, const NsimOccMeta* meta,
                                   void* stream) {
  if (nvox <= 0 || K <= 0) return 0;
  if (!meta || !val || slice_stride < nvox) return 5;
  // (one decay of all K slices: the padding between slices, if any, is scaled too and never read)
  const int64_t span = (int64_t)(K - 1) * slice_stride + nvox;
  hipLaunchKernelGGL(k_occ_scale, dim3(nsim_blocks(span, 256)), dim3(256), 0, (hipStream_t)stream, val, span, decay);
  NSIM_CHECK_LAUNCH();
  if (n <= 0) return 0;
  if (!pts || !sigma || !slice) return 4;
  hipLaunchKernelGGL(k_occ_max_density_sliced, dim3(nsim_blocks(n, 256)), dim3(256), 0, (hipStream_t)stream, val,
                     slice_stride, K, pts, (const float*)nullptr, (const float*)nullptr, (const float*)nullptr,
                     (const int64_t*)nullptr, slice, sigma, n, occ_dev(meta));
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_occ_collect_density_sliced(float* val, int64_t slice_stride, int K, const float* x, const float* rays_o,
                                    const float* rays_d, const float* t, const int64_t* ridx, const int64_t* slice,
                                    const float* sigma, int64_t n, const NsimOccMeta* meta, void* stream) {
  if (n <= 0 || K <= 0) return 0;
  if (!meta || !val) return 5;
  if (!sigma || !slice) return 4;
  if (!x && !(rays_o && rays_d && t && ridx)) return 24;
  hipLaunchKernelGGL(k_occ_max_density_sliced, dim3(nsim_blocks(n, 256)), dim3(256), 0, (hipStream_t)stream, val,
                     slice_stride, K, x, rays_o, rays_d, t, ridx, slice, sigma, n, occ_dev(meta));
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_occ_pack_bits_mean_sliced(const float* val, int64_t nvox, int64_t slice_stride, int K, float occ_thre,
                                   int consider_mean, float* workspace, uint32_t* bits, void* stream) {
  if (nvox <= 0 || K <= 0) return 0;
  if (!val || !bits || !workspace || slice_stride < nvox) return 4;
  if (consider_mean) {
    hipLaunchKernelGGL(k_occ_partial_sum_sliced, dim3(OCC_MEAN_BLOCKS, K), dim3(256), 0, (hipStream_t)stream, val,
                       slice_stride, nvox, workspace);
    NSIM_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(k_occ_pack_bits_mean_sliced, dim3(nsim_blocks((nvox + 31) / 32, 256), K), dim3(256), 0,
                     (hipStream_t)stream, val, slice_stride, nvox, occ_thre, consider_mean, workspace, bits);
  NSIM_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
