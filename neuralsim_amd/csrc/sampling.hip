// sampling.hip -- ray generation, AABB ray test, occupancy-grid marching and NeuS up-sampling for gfx950.
//
// Replaces the native half of Camera.get_selected_rays (app/resources/observers/cameras.py:281-310),
// AABBSpace.ray_test, OccGridAccel.ray_march / OccGridEma (accel_cfg, march_cfg in
// code_single/configs/object_centric/lotd_neus.dtu.230814.yaml:140-173) and the multi-stage inverse-CDF
// up-sampler of NeusRendererMixin (num_fine, upsample_inv_s, upsample_use_estimate_alpha).
//
// Design: one wavefront per ray.  Marching tests 64 lattice steps per wave instruction against the
// occupancy BITFIELD (64^3 bits = 32 KiB: L1/LDS resident), ballots the hits and emits them already
// sorted; up-sampling is a chunked wave scan (alpha -> transmittance -> cdf) followed by one binary search
// per new sample.  All arithmetic that decides sample membership is written mul-then-add (the library is
// built with -ffp-contract=off) so the sample set is bit-identical to the oracle's.
#include "nsim_common.h"
#include "occ_dev.h"

#define SMP_WAVES_PER_BLOCK 4
#define SMP_BLOCK (64 * SMP_WAVES_PER_BLOCK)
#define SMP_LDS_FLOATS 512   // per-wave LDS window of the up-sampling / merge kernels (longer rays: global memory)

__device__ __forceinline__ int64_t smp_wave_id() {
  return (int64_t)blockIdx.x * SMP_WAVES_PER_BLOCK + (threadIdx.x >> 6);
}
static inline dim3 smp_grid(int64_t R) { return dim3(nsim_blocks(R, SMP_WAVES_PER_BLOCK)); }

// ``upsample_on_marched_only`` (nsim_live_rank, pack_ops.hip): live_rank[r] = q >= 0 -- ray r is the q-th ray whose march found
// occupied voxels ("live"); ~q < 0 -- it found none (q live rays precede it).  Only live rays get coarse and fine samples; every
// per-live-ray array ([R', C] coarse depths, [R', n_fine] draws and their positions / SDFs) is indexed by q, so the points of the
// SDF queries are compact: R' n instead of R n.  live_rank == NULL: every ray is live and q = r (the dense layout).
__device__ __forceinline__ bool smp_live(const int64_t* __restrict__ live_rank, int64_t r, int64_t& q) {
  if (!live_rank) {
    q = r;
    return true;
  }
  const int64_t e = live_rank[r];
  q = e >= 0 ? e : ~e;
  return e >= 0;
}

// ----------------------------------------------------------------------------------- ray generation
// ``intr.lift(u, v, 1)``: pixel -> direction in the camera frame.  Pinhole: ((u - cx) / fx, (v - cy) / fy, 1).  OpenCV
// model (camera_model 'opencv', app/resources/observers/cameras.py:84-87; Waymo's calibration, ``consider_distortion:
// true`` in the street configs): the pinhole coordinates are the DISTORTED ones, x_d = x (1 + k1 r2 + k2 r4 + k3 r6) +
// 2 p1 x y + p2 (r2 + 2 x2) (y alike), dist = (k1, k2, p1, p2, k3); the undistorted (x, y) come from the fixed-point
// iteration of cv::undistortPoints, n_iters rounds (OpenCV runs 5).  nr3d_lib's OpenCVCameraMatHW is absent: the
// iteration and its count are fixed here.  Written mul-then-add (no contraction) so that the oracle reproduces it.
// Fisheye model (camera_model 'fisheye', cameras.py:88-92; the OpenCV fisheye / Kannala-Brandt equidistant model the
// reference's app/resources/observers/fisheye.py:36-42 applies: theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 +
// k4 theta^8), pixel = f (x_d, y_d) + c with (x_d, y_d) = theta_d (a, b) / r): n_iters < 0 selects it, dist = (k1..k4) with
// stride 4, -n_iters Newton rounds on theta (cv::fisheye::undistortPoints runs 10) from theta = theta_d.  The lifted
// direction is (sin theta x_d / theta_d, sin theta y_d / theta_d, cos theta) -- (a, b, 1) cos theta, valid past 90 degrees.
__device__ __forceinline__ void raygen_lift_fisheye(const float* K, const float* dist, int n_iters, float w, float h, float l[3]) {
  const float xd = (w - K[2]) / K[0], yd = (h - K[5]) / K[4];
  const float td = sqrtf(xd * xd + yd * yd);
  const float k1 = dist[0], k2 = dist[1], k3 = dist[2], k4 = dist[3];
  float th = td;
  for (int it = 0; it < n_iters; ++it) {
    const float t2 = th * th;
    const float f = th * (1.0f + (((k4 * t2 + k3) * t2 + k2) * t2 + k1) * t2) - td;
    const float fp = 1.0f + (((9.0f * k4 * t2 + 7.0f * k3) * t2 + 5.0f * k2) * t2 + 3.0f * k1) * t2;
    th = th - f / fp;
  }
  const float sc = td > 1e-8f ? sinf(th) / td : 1.0f;
  l[0] = xd * sc;
  l[1] = yd * sc;
  l[2] = cosf(th);
}

__device__ __forceinline__ void raygen_lift(const float* K, const float* dist, int n_iters, float w, float h, float l[3]) {
  if (n_iters < 0) {
    raygen_lift_fisheye(K, dist, -n_iters, w, h, l);
    return;
  }
  const float x0 = (w - K[2]) / K[0], y0 = (h - K[5]) / K[4];
  float x = x0, y = y0;
  if (dist) {
    const float k1 = dist[0], k2 = dist[1], p1 = dist[2], p2 = dist[3], k3 = dist[4];
    for (int it = 0; it < n_iters; ++it) {
      const float r2 = x * x + y * y;
      const float icd = 1.0f / (1.0f + ((k3 * r2 + k2) * r2 + k1) * r2);
      const float dx = 2.0f * p1 * x * y + p2 * (r2 + 2.0f * x * x);
      const float dy = p1 * (r2 + 2.0f * y * y) + 2.0f * p2 * x * y;
      x = (x0 - dx) * icd;
      y = (y0 - dy) * icd;
    }
  }
  l[0] = x;
  l[1] = y;
  l[2] = 1.0f;
}

__global__ void __launch_bounds__(256) k_raygen_pinhole(const float* __restrict__ xy,
                                                         const int64_t* __restrict__ fidx,
                                                         const float* __restrict__ intr,
                                                         const float* __restrict__ c2w,
                                                         const int64_t* __restrict__ WH, int64_t N, int snap,
                                                         float* __restrict__ rays_o, float* __restrict__ rays_d,
                                                         const float* __restrict__ dist, int n_iters) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int64_t f = fidx[i];
  const float W = (float)WH[2 * f], H = (float)WH[2 * f + 1];
  float w = xy[2 * i] * W, h = xy[2 * i + 1] * H;
  if (snap) {  // (xy*WH).long().clamp(0, WH-1) + 0.5   (cameras.py:302-303)
    float wi = truncf(w), hi = truncf(h);
    wi = fminf(fmaxf(wi, 0.f), W - 1.f);
    hi = fminf(fmaxf(hi, 0.f), H - 1.f);
    w = wi + 0.5f;
    h = hi + 0.5f;
  }
  float l[3];
  raygen_lift(intr + f * 9, dist ? dist + f * (n_iters < 0 ? 4 : 5) : nullptr, n_iters, w, h, l);
  const float dx = l[0], dy = l[1], dz = l[2];      // (dz == 1.0f for the pinhole / OpenCV models)
  const float* M = c2w + f * 16;
  // broadcast-multiply-sum, never a reduced-precision matmul (cameras.py:355-359)
  float d0 = M[0] * dx + M[1] * dy + M[2] * dz;
  float d1 = M[4] * dx + M[5] * dy + M[6] * dz;
  float d2 = M[8] * dx + M[9] * dy + M[10] * dz;
  const float nrm = fmaxf(sqrtf(d0 * d0 + d1 * d1 + d2 * d2), 1e-12f);
  rays_d[3 * i + 0] = d0 / nrm;
  rays_d[3 * i + 1] = d1 / nrm;
  rays_d[3 * i + 2] = d2 / nrm;
  rays_o[3 * i + 0] = M[3];
  rays_o[3 * i + 1] = M[7];
  rays_o[3 * i + 2] = M[11];
}

// Backward of the ray generation w.r.t. the camera poses (pose refinement: the reference's LearnableParams feed refined
// c2w matrices into Camera.get_selected_rays, withmask_withlidar_joint.240219.yaml:338-352):
//   rays_o = T,  rays_d = R l / |R l|   =>   dT[f] += d_o,  dR[f] += ((I - d d^T) d_d / |R l|) (x) l
// d_c2w [V,4,4] is accumulated with atomics (a few thousand rays onto a few hundred poses; the bottom row stays zero).
__global__ void __launch_bounds__(256) k_raygen_pinhole_bwd(const float* __restrict__ xy,
                                                             const int64_t* __restrict__ fidx,
                                                             const float* __restrict__ intr,
                                                             const float* __restrict__ c2w,
                                                             const int64_t* __restrict__ WH, int64_t N, int snap,
                                                             const float* __restrict__ d_o,
                                                             const float* __restrict__ d_d,
                                                             float* __restrict__ d_c2w,
                                                             const float* __restrict__ dist, int n_iters) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int64_t f = fidx[i];
  const float W = (float)WH[2 * f], H = (float)WH[2 * f + 1];
  float w = xy[2 * i] * W, h = xy[2 * i + 1] * H;
  if (snap) {
    float wi = truncf(w), hi = truncf(h);
    wi = fminf(fmaxf(wi, 0.f), W - 1.f);
    hi = fminf(fmaxf(hi, 0.f), H - 1.f);
    w = wi + 0.5f;
    h = hi + 0.5f;
  }
  float l[3];
  raygen_lift(intr + f * 9, dist ? dist + f * (n_iters < 0 ? 4 : 5) : nullptr, n_iters, w, h, l);
  const float* M = c2w + f * 16;
  float dw[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) dw[r] = M[4 * r] * l[0] + M[4 * r + 1] * l[1] + M[4 * r + 2] * l[2];
  const float nrm = fmaxf(sqrtf(dw[0] * dw[0] + dw[1] * dw[1] + dw[2] * dw[2]), 1e-12f);
  float* G = d_c2w + f * 16;
  if (d_d) {
    const float u[3] = {dw[0] / nrm, dw[1] / nrm, dw[2] / nrm};
    const float g[3] = {d_d[3 * i], d_d[3 * i + 1], d_d[3 * i + 2]};
    const float dot = g[0] * u[0] + g[1] * u[1] + g[2] * u[2];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const float gr = (g[r] - dot * u[r]) / nrm;
#pragma unroll
      for (int c = 0; c < 3; ++c) atomicAdd(&G[4 * r + c], gr * l[c]);
    }
  }
  if (d_o) {
#pragma unroll
    for (int r = 0; r < 3; ++r) atomicAdd(&G[4 * r + 3], d_o[3 * i + r]);
  }
}

// ------------------------------------------------------------------------------------ AABB ray test
__global__ void __launch_bounds__(256) k_aabb_ray_test(const float* __restrict__ rays_o,
                                                        const float* __restrict__ rays_d, int64_t N, OccDev m,
                                                        float near, float far, float* __restrict__ near_out,
                                                        float* __restrict__ far_out, uint8_t* __restrict__ hit) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  float tmin = -INFINITY, tmax = INFINITY;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float o = rays_o[3 * i + a];
    float d = rays_d[3 * i + a];
    if (fabsf(d) < 1e-12f) d = (d < 0.f) ? -1e-12f : 1e-12f;
    const float inv = 1.0f / d;
    const float t1 = (m.mn[a] - o) * inv, t2 = (m.mx[a] - o) * inv;
    tmin = fmaxf(tmin, fminf(t1, t2));
    tmax = fminf(tmax, fmaxf(t1, t2));
  }
  const float n = fmaxf(tmin, near);
  const float f = (far >= 0.f) ? fminf(tmax, far) : tmax;
  near_out[i] = n;
  far_out[i] = f;
  hit[i] = (f > n) ? 1 : 0;
}

// ----------------------------------------------------------------------------------- occupancy grid
__global__ void __launch_bounds__(256) k_occ_decay(float* __restrict__ val, int64_t n, float decay) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) val[i] = val[i] * decay;
}

// scatter-max of f(sdf) = 4 sig(s x)(1 - sig(s x)) >= 0: integer atomicMax on the bit pattern is exact
// n_dev (may be NULL): the number of valid points is min(n, *n_dev + n_add) -- 0 when that exceeds n (a speculatively
// sized sampling pass that overflowed: the caller redoes it, see k_lotd_gather_lm)
__global__ void __launch_bounds__(256) k_occ_update(float* __restrict__ val, const float* __restrict__ pts,
                                                     const float* __restrict__ sdf, int64_t n, OccDev m,
                                                     float inv_s, const int64_t* __restrict__ n_dev, int64_t n_add) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n_dev) {
    const int64_t nd = n_dev[0] + n_add;
    n = nd <= n ? nd : 0;
  }
  const bool ok = i < n;
  occ_collect_wave(val, m, ok, ok ? pts[3 * i] : 0.f, ok ? pts[3 * i + 1] : 0.f, ok ? pts[3 * i + 2] : 0.f, ok ? sdf[i] : 0.f,
                   inv_s);
}

// one lane per voxel (coalesced reads), a ballot packs the 64 voxels of a wave into two words; a grid of any size covers the array
__global__ void __launch_bounds__(256) k_occ_pack_bits(const float* __restrict__ val, int64_t nvox, float thre,
                                                        uint32_t* __restrict__ bits) {
  const int lane = nsim_lane();
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t end = (nvox + 63) & ~(int64_t)63;            // whole waves take part in every ballot
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < end; v += stride) {
    const unsigned long long b = wave_ballot(v < nvox && val[v] > thre);
    if ((lane & 31) == 0 && v < nvox) bits[v >> 5] = (uint32_t)(b >> (lane & 32));
  }
}

// ------------------------------------------------------------------------------------------ marching
// (MarchRay / march_load / march_test: occ_dev.h -- the sphere tracer of field.hip skips empty space on the same lattice)
__global__ void __launch_bounds__(SMP_BLOCK) k_march_count(
    const float* __restrict__ rays_o, const float* __restrict__ rays_d, const float* __restrict__ near,
    const float* __restrict__ far, const float* __restrict__ jitter, int64_t R, const uint32_t* __restrict__ bits,
    const int64_t* __restrict__ ray_word_off, OccDev occ, float step, int max_steps, int64_t* __restrict__ counts) {
  const int64_t r = smp_wave_id();
  if (r >= R) return;
  const int lane = nsim_lane();
  if (ray_word_off) bits += ray_word_off[r];      // batched occupancy grid: this ray's instance
  const MarchRay m = march_load(rays_o, rays_d, near, far, jitter, r, step, max_steps);
  int cnt = 0;
  for (int base = 0; base < m.K; base += 64) {
    float t;
    const bool hit = march_test(m, occ, bits, base + lane, step, t);
    cnt += __popcll(wave_ballot(hit));
  }
  if (lane == 0) counts[r] = cnt;
}

__global__ void __launch_bounds__(SMP_BLOCK) k_march_emit(
    const float* __restrict__ rays_o, const float* __restrict__ rays_d, const float* __restrict__ near,
    const float* __restrict__ far, const float* __restrict__ jitter, int64_t R, const uint32_t* __restrict__ bits,
    const int64_t* __restrict__ ray_word_off, OccDev occ, float step, int max_steps, const int64_t* __restrict__ pi,
    float* __restrict__ t_out) {
  const int64_t r = smp_wave_id();
  if (r >= R) return;
  const int lane = nsim_lane();
  if (ray_word_off) bits += ray_word_off[r];
  if (pi[2 * r + 1] == 0) return;      // nothing to emit (or a pack emptied by a speculative capacity, pack_ops.hip)
  const MarchRay m = march_load(rays_o, rays_d, near, far, jitter, r, step, max_steps);
  const int64_t st = pi[2 * r];
  int cnt = 0;
  for (int base = 0; base < m.K; base += 64) {
    float t;
    const bool hit = march_test(m, occ, bits, base + lane, step, t);
    const unsigned long long mask = wave_ballot(hit);
    if (hit) {
      const int before = __popcll(mask & ((1ull << lane) - 1ull));
      t_out[st + cnt + before] = t;
    }
    cnt += __popcll(mask);
  }
}

__global__ void __launch_bounds__(256) k_coarse_depths(const float* __restrict__ near, const float* __restrict__ far,
                                                        const float* __restrict__ jc, int64_t R, int C,
                                                        float* __restrict__ out, const int64_t* __restrict__ live_rank) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= R * C) return;
  const int64_t r = j / C;
  const int i = (int)(j % C);
  int64_t q;
  if (!smp_live(live_rank, r, q)) return;
  const float u = jc ? jc[j] : 0.5f;
  out[q * C + i] = near[r] + (far[r] - near[r]) * (((float)i + u) / (float)C);
}

// ---------------------------------------------------------------------------------------- up-sampling
__device__ __forceinline__ float smp_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// interval opacity used for up-sampling (NeuS `up_sample`, or the plain consecutive-sdf form)
__device__ __forceinline__ float upsample_alpha(const float* t, const float* sdf, int64_t i, float inv_s,
                                                int use_est) {
  const float s0 = sdf[i], s1 = sdf[i + 1];
  if (use_est) {
    const float t0 = t[i], t1 = t[i + 1];
    const float dist = t1 - t0;
    float cs = (s1 - s0) / (dist + 1e-5f);
    float prev = 0.f;
    if (i > 0) prev = (s0 - sdf[i - 1]) / ((t0 - t[i - 1]) + 1e-5f);
    cs = fminf(prev, cs);
    cs = fminf(fmaxf(cs, -1e3f), 0.f);
    const float mid = (s0 + s1) * 0.5f;
    const float half = cs * dist * 0.5f;
    const float pc = smp_sigmoid((mid - half) * inv_s), nc = smp_sigmoid((mid + half) * inv_s);
    return (pc - nc + 1e-5f) / (pc + 1e-5f);
  } else {
    const float c0 = smp_sigmoid(s0 * inv_s), c1 = smp_sigmoid(s1 * inv_s);
    const float a = (c0 - c1 + 1e-5f) / (c0 + 1e-5f);
    return fminf(fmaxf(a, 0.f), 1.f);
  }
}

// one ray (one wave): n_fine new depths drawn from the interval weights of the ray's samples tt / ss [n]; ``lds`` holds the
// running sums when the ray fits (SMP_LDS_FLOATS intervals), the global scratch ``cs_glob`` otherwise
__device__ __forceinline__ void upsample_ray(const float* tt, const float* ss, int64_t n, int64_t r, int64_t q, float inv_s, int n_fine,
                                             int use_est, float* lds, float* cs_glob, float* __restrict__ t_new,
                                             const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                             float* __restrict__ x_new) {
  const int lane = nsim_lane();
  const int64_t ni = n - 1;  // intervals
  float ro[3] = {0.f, 0.f, 0.f}, rd[3] = {0.f, 0.f, 0.f};
  if (x_new) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      ro[c] = rays_o[3 * r + c];
      rd[c] = rays_d[3 * r + c];
    }
  }
  auto body = [&](auto cs) {
    float carry_T = 1.0f, carry_S = 0.f;
    for (int64_t base = 0; base < ni; base += 64) {
      const int64_t i = base + lane;
      const bool valid = i < ni;
      const float a = valid ? upsample_alpha(tt, ss, i, inv_s, use_est) : 0.f;
      const float f = valid ? (1.0f - a + 1e-7f) : 1.0f;
      const float incl = wave_incl_prod(f);
      float excl = wave_shfl(incl, lane - 1);
      if (lane == 0) excl = 1.0f;
      const float T = carry_T * excl;
      carry_T = carry_T * wave_shfl(incl, 63);
      const float w = valid ? (a * T + 1e-5f) : 0.f;
      const float ws = wave_incl_sum(w);
      if (valid) cs[i] = carry_S + ws;
      carry_S = carry_S + wave_shfl(ws, 63);
    }
    nsim_wave_fence();
    const float wsum = carry_S;
    for (int kb = 0; kb < n_fine; kb += 64) {
      const int k = kb + lane;
      if (k >= n_fine) continue;
      float tn = (n > 0) ? tt[0] : 0.f;
      if (ni > 0) {
        const float u = ((float)k + 0.5f) / (float)n_fine;
        // first interval i with cdf[i+1] = cs[i]/wsum > u, clamped to the last interval
        int64_t lo = 0, hi = ni;
        while (lo < hi) {
          const int64_t mid = (lo + hi) >> 1;
          if (cs[mid] / wsum <= u) lo = mid + 1; else hi = mid;
        }
        if (lo > ni - 1) lo = ni - 1;
        const float c_lo = (lo == 0) ? 0.f : cs[lo - 1] / wsum;
        const float c_hi = cs[lo] / wsum;
        float den = c_hi - c_lo;
        if (den < 1e-5f) den = 1.0f;
        float frac = (u - c_lo) / den;
        frac = fminf(fmaxf(frac, 0.f), 1.f);
        const float b_lo = tt[lo], b_hi = tt[lo + 1];
        tn = b_lo + frac * (b_hi - b_lo);
      }
      t_new[q * n_fine + k] = tn;
      if (x_new) {   // the sample's position, so that the level-major query loads 12 B instead of re-deriving it per XCD
#pragma unroll
        for (int c = 0; c < 3; ++c) x_new[(q * n_fine + k) * 3 + c] = ro[c] + tn * rd[c];
      }
    }
  };
  if (ni <= SMP_LDS_FLOATS) body(lds);
  else body(cs_glob);
}

__global__ void __launch_bounds__(SMP_BLOCK) k_upsample_stage(const float* __restrict__ t,
                                                                const float* __restrict__ sdf,
                                                                const int64_t* __restrict__ pi, int64_t R,
                                                                float inv_s, int n_fine, int use_est,
                                                                float* __restrict__ csum,
                                                                float* __restrict__ t_new,
                                                                const float* __restrict__ rays_o,
                                                                const float* __restrict__ rays_d,
                                                                float* __restrict__ x_new,
                                                                const int64_t* __restrict__ live_rank) {
  // the running sums of a ray's interval weights live in LDS (<= SMP_LDS_FLOATS intervals; longer rays use the global
  // scratch): the inverse-CDF search below is eight DEPENDENT reads per new sample -- 13 us per launch from L2
  __shared__ float smp_lds[SMP_WAVES_PER_BLOCK][SMP_LDS_FLOATS];
  const int64_t r = smp_wave_id();
  if (r >= R) return;
  int64_t q;
  if (!smp_live(live_rank, r, q)) return;      // no marched samples: no draws
  const int64_t st = pi[2 * r], n = pi[2 * r + 1];
  upsample_ray(t + st, sdf + st, n, r, q, inv_s, n_fine, use_est, &smp_lds[threadIdx.x >> 6][0], csum + st, t_new, rays_o, rays_d,
               x_new);
}

// -------------------------------------------------------------------------------- sorted merge
__device__ __forceinline__ int64_t smp_lower_bound(const float* a, int64_t n, float v) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (a[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ int64_t smp_upper_bound(const float* a, int64_t n, float v) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (a[mid] <= v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// one ray (one wave): merge its sorted depth lists a [na] (values v_a) and b [nb] (values v_b) into the packed output at
// ``so``; ``lds`` holds both lists when they fit
__device__ __forceinline__ void merge_ray(const float* __restrict__ t_a, const float* __restrict__ v_a, int64_t sa, int64_t na,
                                          const float* __restrict__ t_b, const float* __restrict__ v_b, int64_t r, int64_t q, int nb,
                                          int64_t so, float* lds, float* __restrict__ t_out, float* __restrict__ v_out,
                                          int64_t* __restrict__ ridx_out, const float* __restrict__ rays_o,
                                          const float* __restrict__ rays_d, float* __restrict__ x_out) {
  const int lane = nsim_lane();
  float ro[3] = {0.f, 0.f, 0.f}, rd[3] = {0.f, 0.f, 0.f};
  if (x_out) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      ro[c] = rays_o[3 * r + c];
      rd[c] = rays_d[3 * r + c];
    }
  }
  // both depth lists of the ray in LDS when they fit (a first, then b): the rank searches are 6-8 DEPENDENT reads each
  const bool in_lds = na + nb <= SMP_LDS_FLOATS;
  float* la = lds;
  float* lb = la + na;
  if (in_lds) {
    for (int64_t i = lane; i < na; i += 64) la[i] = t_a[sa + i];
    for (int64_t j = lane; j < nb; j += 64) lb[j] = t_b[q * (int64_t)nb + j];
    nsim_wave_fence();
  }
  auto body = [&](auto a, auto b) {
    for (int64_t i = lane; i < na; i += 64) {  // a first on ties: b elements strictly smaller precede
      const float v = a[i];
      const int64_t pos = i + smp_lower_bound(b, nb, v);
      t_out[so + pos] = v;
      if (v_out) v_out[so + pos] = v_a ? v_a[sa + i] : 0.f;
      if (ridx_out) ridx_out[so + pos] = r;
      if (x_out) {
#pragma unroll
        for (int c = 0; c < 3; ++c) x_out[(so + pos) * 3 + c] = ro[c] + v * rd[c];
      }
    }
    for (int64_t j = lane; j < nb; j += 64) {
      const float v = b[j];
      const int64_t pos = j + smp_upper_bound(a, na, v);
      t_out[so + pos] = v;
      if (v_out) v_out[so + pos] = v_b ? v_b[q * (int64_t)nb + j] : 0.f;
      if (ridx_out) ridx_out[so + pos] = r;
      if (x_out) {
#pragma unroll
        for (int c = 0; c < 3; ++c) x_out[(so + pos) * 3 + c] = ro[c] + v * rd[c];
      }
    }
  };
  if (in_lds) body((const float*)la, (const float*)lb);
  else body(t_a + sa, t_b + q * (int64_t)nb);
}

__global__ void __launch_bounds__(SMP_BLOCK) k_merge_sorted(const float* __restrict__ t_a,
                                                              const float* __restrict__ v_a,
                                                              const int64_t* __restrict__ pia,
                                                              const float* __restrict__ t_b,
                                                              const float* __restrict__ v_b, int64_t R, int nb,
                                                              float* __restrict__ t_out, float* __restrict__ v_out,
                                                              int64_t* __restrict__ pio, int64_t* __restrict__ ridx_out,
                                                              const float* __restrict__ rays_o,
                                                              const float* __restrict__ rays_d,
                                                              float* __restrict__ x_out,
                                                              const int64_t* __restrict__ live_rank) {
  __shared__ float smp_lds[SMP_WAVES_PER_BLOCK][SMP_LDS_FLOATS];
  const int64_t r = smp_wave_id();
  if (r >= R) return;
  int64_t q;
  const bool live = smp_live(live_rank, r, q);
  const int64_t sa = pia[2 * r], na = live ? pia[2 * r + 1] : 0;
  const int64_t so = sa + q * (int64_t)nb;       // q live rays precede r, each with nb list-b samples
  const int nb_r = live ? nb : 0;
  if (nsim_lane() == 0) {
    pio[2 * r] = so;
    pio[2 * r + 1] = na + nb_r;
  }
  if (!live) return;
  merge_ray(t_a, v_a, sa, na, t_b, v_b, r, q, nb, so, &smp_lds[threadIdx.x >> 6][0], t_out, v_out, ridx_out, rays_o, rays_d, x_out);
}

// merge of up-sampling stage k AND the draw of stage k + 1 in one launch (round 4): both are one-wave-per-ray; the merged
// samples of a ray are handed from the merge to the draw through t_out / v_out (written and read by the SAME wave, ordered by
// the wave-level fence), the LDS row is used by the merge first and by the draw's running sums afterwards
__global__ void __launch_bounds__(SMP_BLOCK) k_merge_upsample(const float* __restrict__ t_a, const float* __restrict__ v_a,
                                                                const int64_t* __restrict__ pia, const float* __restrict__ t_b,
                                                                const float* __restrict__ v_b, int64_t R, int nb,
                                                                float* __restrict__ t_out, float* __restrict__ v_out,
                                                                int64_t* __restrict__ pio, int64_t* __restrict__ ridx_out,
                                                                float inv_s, int n_fine, int use_est, float* __restrict__ csum,
                                                                float* __restrict__ t_new, const float* __restrict__ rays_o,
                                                                const float* __restrict__ rays_d, float* __restrict__ x_new,
                                                                const int64_t* __restrict__ live_rank) {
  __shared__ float smp_lds[SMP_WAVES_PER_BLOCK][SMP_LDS_FLOATS];
  const int64_t r = smp_wave_id();
  if (r >= R) return;
  int64_t q;
  const bool live = smp_live(live_rank, r, q);
  const int64_t sa = pia[2 * r], na = live ? pia[2 * r + 1] : 0;
  const int64_t so = sa + q * (int64_t)nb;
  const int nb_r = live ? nb : 0;
  if (nsim_lane() == 0) {
    pio[2 * r] = so;
    pio[2 * r + 1] = na + nb_r;
  }
  if (!live) return;
  float* lds = &smp_lds[threadIdx.x >> 6][0];
  merge_ray(t_a, v_a, sa, na, t_b, v_b, r, q, nb, so, lds, t_out, v_out, ridx_out, nullptr, nullptr, nullptr);
  nsim_wave_fence();
  upsample_ray(t_out + so, v_out + so, na + nb, r, q, inv_s, n_fine, use_est, lds, csum + so, t_new, rays_o, rays_d, x_new);
}

// ------------------------------------------------------------------ compressed query mode
// ``query_mode: march_occ_multi_upsample_compressed`` (lotd_neus.dtu.230814.yaml:157): after up-sampling every
// sample carries a no-grad SDF; samples whose visibility weight is negligible are dropped before the expensive
// with-grad query.  A sample is kept iff one of the two intervals it bounds has vw > thre; surviving neighbours
// form merged intervals (the NeuS opacity telescopes: 1 - alpha(i,j) = Phi(s_j)/Phi(s_i)).
// One wave per ray: alpha -> transmittance scan -> keep flags -> ballot compaction.
__device__ __forceinline__ float compress_alpha(const float* sdf, int64_t i, int64_t n, float s) {
  if (i + 1 >= n) return 0.f;
  const float c0 = smp_sigmoid(sdf[i] * s), c1 = smp_sigmoid(sdf[i + 1] * s);
  const float a = (c0 - c1 + 1e-5f) / (c0 + 1e-5f);
  return fminf(fmaxf(a, 0.f), 1.f);
}

template <bool EMIT>
__global__ void __launch_bounds__(SMP_BLOCK) k_compress(const float* __restrict__ sdf, const float* __restrict__ t,
                                                         const int64_t* __restrict__ pi, int64_t R,
                                                         const float* __restrict__ ln_inv_s, float factor,
                                                         float forward_inv_s, float thre, int64_t* __restrict__ counts,
                                                         const int64_t* __restrict__ pi_out, float* __restrict__ t_out,
                                                         int64_t* __restrict__ ridx_out, int64_t tail_n) {
  const int64_t r = smp_wave_id();
  if (r >= R) return;
  const int lane = nsim_lane();
  if (EMIT && tail_n > 0) {  // tail_n zero-length samples on the pseudo-rays R, R+1, ... behind the kept set
    const int64_t S = pi_out[2 * (R - 1)] + pi_out[2 * (R - 1) + 1];
    for (int64_t i = r * 64 + lane; i < tail_n; i += R * 64) {
      t_out[S + i] = 0.f;
      ridx_out[S + i] = R + i;
    }
  }
  const int64_t st = pi[2 * r], n = pi[2 * r + 1];
  const float s = forward_inv_s > 0.f ? forward_inv_s : expf(ln_inv_s[0] * factor);
  const float* ss = sdf + st;
  float carry = 1.0f;
  bool prev_sig = false;  // significance of the interval ending at the first sample of the chunk
  int cnt = 0;
  const int64_t ost = EMIT ? pi_out[2 * r] : 0;
  for (int64_t base = 0; base < n; base += 64) {
    const int64_t i = base + lane;
    const bool valid = i < n;
    const float a = valid ? compress_alpha(ss, i, n, s) : 0.f;
    const float f = valid ? (1.0f - a + 1e-10f) : 1.0f;
    const float incl = wave_incl_prod(f);
    float excl = wave_shfl(incl, lane - 1);
    if (lane == 0) excl = 1.0f;
    const float vw = a * (carry * excl);
    carry = carry * wave_shfl(incl, 63);
    const bool sig = valid && (vw > thre);
    int psig = wave_shfl((int)sig, lane - 1);
    if (lane == 0) psig = prev_sig ? 1 : 0;
    prev_sig = wave_shfl((int)sig, 63) != 0;
    const bool keep = valid && (sig || psig != 0);
    const unsigned long long m = wave_ballot(keep);
    if (EMIT && keep) {
      const int before = __popcll(m & ((1ull << lane) - 1ull));
      t_out[ost + cnt + before] = t[st + i];
      ridx_out[ost + cnt + before] = r;
    }
    cnt += __popcll(m);
  }
  if (!EMIT && lane == 0) counts[r] = cnt;
}

// ================================================================================== C ABI
extern "C" {

int nsim_raygen_pinhole(const float* xy, const int64_t* fidx, const float* intr, const float* c2w,
                        const int64_t* WH, int64_t N, int snap, float* rays_o, float* rays_d, void* stream) {
  if (N <= 0) return 0;
  hipLaunchKernelGGL(k_raygen_pinhole, dim3(nsim_blocks(N, 256)), dim3(256), 0, (hipStream_t)stream, xy, fidx, intr, c2w,
                     WH, N, snap, rays_o, rays_d, (const float*)nullptr, 0);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_raygen_opencv(const float* xy, const int64_t* fidx, const float* intr, const float* distortion, int n_iters,
                       const float* c2w, const int64_t* WH, int64_t N, int snap, float* rays_o, float* rays_d,
                       void* stream) {
  if (N <= 0) return 0;
  if (!distortion || n_iters < 0 || n_iters > 64) return 4;
  hipLaunchKernelGGL(k_raygen_pinhole, dim3(nsim_blocks(N, 256)), dim3(256), 0, (hipStream_t)stream, xy, fidx, intr, c2w,
                     WH, N, snap, rays_o, rays_d, distortion, n_iters);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_raygen_fisheye(const float* xy, const int64_t* fidx, const float* intr, const float* distortion, int n_iters,
                        const float* c2w, const int64_t* WH, int64_t N, int snap, float* rays_o, float* rays_d,
                        void* stream) {
  if (N <= 0) return 0;
  if (!distortion || n_iters < 1 || n_iters > 64) return 4;
  hipLaunchKernelGGL(k_raygen_pinhole, dim3(nsim_blocks(N, 256)), dim3(256), 0, (hipStream_t)stream, xy, fidx, intr, c2w,
                     WH, N, snap, rays_o, rays_d, distortion, -n_iters);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_raygen_fisheye_bwd(const float* xy, const int64_t* fidx, const float* intr, const float* distortion, int n_iters,
                            const float* c2w, const int64_t* WH, int64_t N, int snap, const float* d_rays_o,
                            const float* d_rays_d, float* d_c2w, void* stream) {
  if (N <= 0) return 0;
  if (!d_c2w || !distortion || n_iters < 1 || n_iters > 64) return 4;
  hipLaunchKernelGGL(k_raygen_pinhole_bwd, dim3(nsim_blocks(N, 256)), dim3(256), 0, (hipStream_t)stream, xy, fidx, intr,
                     c2w, WH, N, snap, d_rays_o, d_rays_d, d_c2w, distortion, -n_iters);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_raygen_pinhole_bwd(const float* xy, const int64_t* fidx, const float* intr, const float* c2w,
                            const int64_t* WH, int64_t N, int snap, const float* d_rays_o, const float* d_rays_d,
                            float* d_c2w, void* stream) {
  if (N <= 0) return 0;
  if (!d_c2w) return 4;
  hipLaunchKernelGGL(k_raygen_pinhole_bwd, dim3(nsim_blocks(N, 256)), dim3(256), 0, (hipStream_t)stream, xy, fidx, intr,
                     c2w, WH, N, snap, d_rays_o, d_rays_d, d_c2w, (const float*)nullptr, 0);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_raygen_opencv_bwd(const float* xy, const int64_t* fidx, const float* intr, const float* distortion, int n_iters,
                           const float* c2w, const int64_t* WH, int64_t N, int snap, const float* d_rays_o,
                           const float* d_rays_d, float* d_c2w, void* stream) {
  if (N <= 0) return 0;
  if (!d_c2w || !distortion || n_iters < 0 || n_iters > 64) return 4;
  hipLaunchKernelGGL(k_raygen_pinhole_bwd, dim3(nsim_blocks(N, 256)), dim3(256), 0, (hipStream_t)stream, xy, fidx, intr,
                     c2w, WH, N, snap, d_rays_o, d_rays_d, d_c2w, distortion, n_iters);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_aabb_ray_test(const float* rays_o, const float* rays_d, int64_t N, const NsimOccMeta* meta, float near,
                       float far, float* near_out, float* far_out, uint8_t* hit, void* stream) {
  if (N <= 0) return 0;
  if (!meta) return 5;
  hipLaunchKernelGGL(k_aabb_ray_test, dim3(nsim_blocks(N, 256)), dim3(256), 0, (hipStream_t)stream, rays_o, rays_d, N,
                     occ_dev(meta), near, far, near_out, far_out, hit);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_occ_decay(float* val, int64_t nvox, float decay, void* stream) {
  if (nvox <= 0) return 0;
  hipLaunchKernelGGL(k_occ_decay, dim3(nsim_blocks(nvox, 256)), dim3(256), 0, (hipStream_t)stream, val, nvox, decay);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_occ_update(float* val, const float* pts, const float* sdf, int64_t n, const NsimOccMeta* meta,
                    float inv_s, void* stream) {
  if (n <= 0) return 0;
  if (!meta) return 5;
  hipLaunchKernelGGL(k_occ_update, dim3(nsim_blocks(n, 256)), dim3(256), 0, (hipStream_t)stream, val, pts, sdf, n,
                     occ_dev(meta), inv_s, (const int64_t*)nullptr, (int64_t)0);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_occ_collect(float* val, const float* pts, const float* sdf, int64_t n, const int64_t* n_dev, int64_t n_add,
                     const NsimOccMeta* meta, float inv_s, void* stream) {
  if (n <= 0) return 0;
  if (!meta) return 5;
  hipLaunchKernelGGL(k_occ_update, dim3(nsim_blocks(n, 256)), dim3(256), 0, (hipStream_t)stream, val, pts, sdf, n,
                     occ_dev(meta), inv_s, n_dev, n_add);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_occ_pack_bits(const float* val, int64_t nvox, float thre, uint32_t* bits, void* stream) {
  if (nvox <= 0) return 0;
  hipLaunchKernelGGL(k_occ_pack_bits, dim3(nsim_blocks(nvox, 256)), dim3(256), 0, (hipStream_t)stream, val,
                     nvox, thre, bits);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_march_count(const float* rays_o, const float* rays_d, const float* near, const float* far,
                     const float* jitter, int64_t R, const uint32_t* bits, const int64_t* ray_word_off,
                     const NsimOccMeta* meta, float step, int max_steps, int64_t* counts, void* stream) {
  if (R <= 0) return 0;
  if (!meta || !(step > 0.f)) return 5;
  hipLaunchKernelGGL(k_march_count, smp_grid(R), dim3(SMP_BLOCK), 0, (hipStream_t)stream, rays_o, rays_d, near, far,
                     jitter, R, bits, ray_word_off, occ_dev(meta), step, max_steps, counts);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_march_emit(const float* rays_o, const float* rays_d, const float* near, const float* far,
                    const float* jitter, int64_t R, const uint32_t* bits, const int64_t* ray_word_off,
                    const NsimOccMeta* meta, float step, int max_steps, const int64_t* pack_infos, float* t_out,
                    void* stream) {
  if (R <= 0) return 0;
  if (!meta || !(step > 0.f)) return 5;
  hipLaunchKernelGGL(k_march_emit, smp_grid(R), dim3(SMP_BLOCK), 0, (hipStream_t)stream, rays_o, rays_d, near, far, jitter,
                     R, bits, ray_word_off, occ_dev(meta), step, max_steps, pack_infos, t_out);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_coarse_depths(const float* near, const float* far, const float* jitter_c, int64_t R, int C, float* out,
                       const int64_t* live_rank, void* stream) {
  if (R <= 0 || C <= 0) return 0;
  hipLaunchKernelGGL(k_coarse_depths, dim3(nsim_blocks(R * C, 256)), dim3(256), 0, (hipStream_t)stream, near, far,
                     jitter_c, R, C, out, live_rank);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_upsample_stage(const float* t, const float* sdf, const int64_t* pack_infos, int64_t R, float inv_s,
                        int n_fine, int use_estimate_alpha, float* scratch, float* t_new, const float* rays_o,
                        const float* rays_d, float* x_new, const int64_t* live_rank, void* stream) {
  if (R <= 0 || n_fine <= 0) return 0;
  if (x_new && !(rays_o && rays_d)) return 24;
  hipLaunchKernelGGL(k_upsample_stage, smp_grid(R), dim3(SMP_BLOCK), 0, (hipStream_t)stream, t, sdf, pack_infos, R, inv_s,
                     n_fine, use_estimate_alpha, scratch, t_new, rays_o, rays_d, x_new, live_rank);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_merge_sorted(const float* t_a, const float* v_a, const int64_t* pack_infos_a, const float* t_b,
                      const float* v_b, int64_t R, int nb, float* t_out, float* v_out, int64_t* pack_infos_out,
                      int64_t* ridx_out, const float* rays_o, const float* rays_d, float* x_out, const int64_t* live_rank,
                      void* stream) {
  if (R <= 0) return 0;
  if (x_out && !(rays_o && rays_d)) return 24;
  hipLaunchKernelGGL(k_merge_sorted, smp_grid(R), dim3(SMP_BLOCK), 0, (hipStream_t)stream, t_a, v_a, pack_infos_a, t_b, v_b,
                     R, nb, t_out, v_out, pack_infos_out, ridx_out, rays_o, rays_d, x_out, live_rank);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_merge_upsample(const float* t_a, const float* v_a, const int64_t* pack_infos_a, const float* t_b, const float* v_b,
                        int64_t R, int nb, float* t_out, float* v_out, int64_t* pack_infos_out, int64_t* ridx_out, float inv_s,
                        int n_fine, int use_estimate_alpha, float* scratch, float* t_new, const float* rays_o,
                        const float* rays_d, float* x_new, const int64_t* live_rank, void* stream) {
  if (R <= 0) return 0;
  if (n_fine <= 0 || !v_a || !v_b || !v_out || !scratch || !t_new) return 4;
  if (x_new && !(rays_o && rays_d)) return 24;
  hipLaunchKernelGGL(k_merge_upsample, smp_grid(R), dim3(SMP_BLOCK), 0, (hipStream_t)stream, t_a, v_a, pack_infos_a, t_b, v_b, R,
                     nb, t_out, v_out, pack_infos_out, ridx_out, inv_s, n_fine, use_estimate_alpha, scratch, t_new, rays_o,
                     rays_d, x_new, live_rank);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_compress_count(const float* sdf, const int64_t* pack_infos, int64_t R, const float* ln_inv_s,
                        float ln_inv_s_factor, float forward_inv_s, float thre, int64_t* counts, void* stream) {
  if (R <= 0) return 0;
  hipLaunchKernelGGL((k_compress<false>), smp_grid(R), dim3(SMP_BLOCK), 0, (hipStream_t)stream, sdf, nullptr, pack_infos, R,
                     ln_inv_s, ln_inv_s_factor, forward_inv_s, thre, counts, nullptr, nullptr, nullptr, (int64_t)0);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_compress_emit(const float* sdf, const float* t, const int64_t* pack_infos, int64_t R, const float* ln_inv_s,
                       float ln_inv_s_factor, float forward_inv_s, float thre, const int64_t* pack_infos_out,
                       float* t_out, int64_t* ridx_out, int64_t tail_n, void* stream) {
  if (R <= 0) return 0;
  hipLaunchKernelGGL((k_compress<true>), smp_grid(R), dim3(SMP_BLOCK), 0, (hipStream_t)stream, sdf, t, pack_infos, R,
                     ln_inv_s, ln_inv_s_factor, forward_inv_s, thre, nullptr, pack_infos_out, t_out, ridx_out, tail_n);
  NSIM_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"

// ----------------------------------------------------------------------------------- simulated LiDAR: beam-pattern rays
// Lidar.get_all_rays (app/resources/observers/lidars.py:208-232): the reference builds meshgrid tensors of both angles, four
// sin / cos tensors, three broadcast products, a normalize and a tile; here it is one pass over the outputs.
//   grid   ray r = i n_beams + j takes phis[i], thetas[j] (the flatten order of meshgrid(thetas, phis, indexing='xy'): beam
//          fastest); a workgroup owns LG_TILE consecutive rays, i.e. at most LG_TILE / n_beams + 2 azimuths and min(n_beams,
//          LG_TILE) beams: their sines and cosines are staged in LDS once, the per-ray work is multiplies, adds and the normalise
//          (sensors with more than LG_TILE beams -- none known -- take the sines of their thetas per ray);
//   paired ray r takes (thetas[r], phis[r]) (solid-state / Risley scan patterns, lidars.py:494-504, 566-588).
// d = normalize((a X + b Y) + c Z), X, Y, Z the columns of l2w [3,4] (products and sums rounded on their own, as the separate
// tensor operations are), (a, b, c) = (sinT cosP, sinT sinP, cosT), for axis 1 (lidars.py:221-224) (cosT, sinT sinP, -(sinT
// cosP)); normalize = d / max(|d|, 1e-12) with IEEE sqrt and division (torch.nn.functional.normalize).  sinf / cosf are the
// precise library functions: the hardware sine of nsim_sin is outside the accuracy bound of tests/test_lidar_sim.py.
#define LG_THREADS 256
#define LG_PER 4
#define LG_TILE (LG_THREADS * LG_PER)

__device__ __forceinline__ void lg_store_ray(const float* __restrict__ M, int axis, float sT, float cT, float sP, float cP, int64_t r,
                                             float* __restrict__ rays_o, float* __restrict__ rays_d) {
  const float sc = sT * cP, ss = sT * sP;
  const float a = axis ? cT : sc, b = ss, c = axis ? -sc : cT;
  const float d0 = (a * M[0] + b * M[1]) + c * M[2];
  const float d1 = (a * M[4] + b * M[5]) + c * M[6];
  const float d2 = (a * M[8] + b * M[9]) + c * M[10];
  const float nrm = fmaxf(sqrtf((d0 * d0 + d1 * d1) + d2 * d2), 1e-12f);
  rays_d[3 * r + 0] = d0 / nrm;
  rays_d[3 * r + 1] = d1 / nrm;
  rays_d[3 * r + 2] = d2 / nrm;
  rays_o[3 * r + 0] = M[3];
  rays_o[3 * r + 1] = M[7];
  rays_o[3 * r + 2] = M[11];
}

__global__ void __launch_bounds__(LG_THREADS) k_lidar_raygen_grid(const float* __restrict__ thetas, const float* __restrict__ phis,
                                                                  int64_t n_beams, int64_t N, int axis,
                                                                  const float* __restrict__ l2w, float* __restrict__ rays_o,
                                                                  float* __restrict__ rays_d, float* __restrict__ theta_phi) {
  __shared__ float s_sT[LG_TILE], s_cT[LG_TILE], s_sP[LG_TILE + 2], s_cP[LG_TILE + 2];
  const int tid = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * LG_TILE;
  const int64_t r_last = (r0 + LG_TILE < N ? r0 + LG_TILE : N) - 1;
  const int64_t i0 = r0 / n_beams;
  const int n_i = (int)(r_last / n_beams - i0) + 1;                     // <= LG_TILE / n_beams + 2 <= LG_TILE + 2
  const bool staged = n_beams <= LG_TILE;
  if (staged)
    for (int j = tid; j < (int)n_beams; j += LG_THREADS) {
      const float t = thetas[j];
      s_sT[j] = sinf(t);
      s_cT[j] = cosf(t);
    }
  for (int k = tid; k < n_i; k += LG_THREADS) {
    const float p = phis[i0 + k];
    s_sP[k] = sinf(p);
    s_cP[k] = cosf(p);
  }
  __syncthreads();
  float M[12];
#pragma unroll
  for (int q = 0; q < 12; ++q) M[q] = l2w[q];
#pragma unroll
  for (int q = 0; q < LG_PER; ++q) {
    const int64_t r = r0 + q * LG_THREADS + tid;
    if (r >= N) break;
    const int64_t i = r / n_beams, j = r - i * n_beams;
    float sT, cT;
    if (staged) {
      sT = s_sT[j];
      cT = s_cT[j];
    } else {
      const float t = thetas[j];
      sT = sinf(t);
      cT = cosf(t);
    }
    lg_store_ray(M, axis, sT, cT, s_sP[i - i0], s_cP[i - i0], r, rays_o, rays_d);
    if (theta_phi) {
      theta_phi[2 * r + 0] = thetas[j];
      theta_phi[2 * r + 1] = phis[i];
    }
  }
}

__global__ void __launch_bounds__(LG_THREADS) k_lidar_raygen_paired(const float* __restrict__ thetas, const float* __restrict__ phis,
                                                                    int64_t N, int axis, const float* __restrict__ l2w,
                                                                    float* __restrict__ rays_o, float* __restrict__ rays_d,
                                                                    float* __restrict__ theta_phi) {
  const int64_t r = (int64_t)blockIdx.x * LG_THREADS + threadIdx.x;
  if (r >= N) return;
  float M[12];
#pragma unroll
  for (int q = 0; q < 12; ++q) M[q] = l2w[q];
  const float t = thetas[r], p = phis[r];
  lg_store_ray(M, axis, sinf(t), cosf(t), sinf(p), cosf(p), r, rays_o, rays_d);
  if (theta_phi) {
    theta_phi[2 * r + 0] = t;
    theta_phi[2 * r + 1] = p;
  }
}

extern "C" {

int nsim_lidar_raygen(const float* thetas, const float* phis, int64_t n_beams, int64_t n_az, int mode, int axis, const float* l2w,
                      float* rays_o, float* rays_d, float* theta_phi, void* stream) {
  if (n_beams < 0 || n_az < 0) return 2;
  if (mode != 0 && mode != 1) return 3;
  if (axis != 0 && axis != 1) return 3;
  if (mode == 1 && n_beams != n_az) return 60;
  if (n_beams >= ((int64_t)1 << 31) || n_az >= ((int64_t)1 << 31)) return 60;
  const int64_t N = mode == 0 ? n_beams * n_az : n_beams;
  if (N == 0) return 0;
  if (N >= ((int64_t)1 << 39)) return 60;
  if (!rays_o || !rays_d) return 4;
  if (!thetas || !phis || !l2w) return 60;
  if (mode == 0)
    hipLaunchKernelGGL(k_lidar_raygen_grid, dim3((unsigned)((N + LG_TILE - 1) / LG_TILE)), dim3(LG_THREADS), 0, (hipStream_t)stream,
                       thetas, phis, n_beams, N, axis, l2w, rays_o, rays_d, theta_phi);
  else
    hipLaunchKernelGGL(k_lidar_raygen_paired, dim3((unsigned)((N + LG_THREADS - 1) / LG_THREADS)), dim3(LG_THREADS), 0,
                       (hipStream_t)stream, thetas, phis, N, axis, l2w, rays_o, rays_d, theta_phi);
  NSIM_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"

// ----------------------------------------------------------------------------------- error-map importance sampling
// The pixel sampler of the reference's trainer (``ImpSampler`` / ``ErrorMap``: code_single/tools/train.py:105-138 builds them,
// dataio/data_loader/pixel_loader.py:157-171, 280-302 draws (frame, pixel) from them once per iteration, train.py:619-621,
// 678-688 scatters the batch's per-ray photometric error back; config block ``training.error_map``).  Four entry points:
//   accumulate  per ray: cell of (frame, xy), f32 atomics into the scratch planes sum / cnt, a flag per touched image
//   blend       per cell with cnt > 0: em = 0.5 em + 0.5 sum / cnt; the consumed scratch is zeroed again, n_steps counted
//   cdf         per image (one workgroup): the clamped, twice-normalised pdf and its inclusive scan; then the image level
//   draw        per row: two binary searches (image, cell) + the jitter inside the cell, or the uniform formula
// The scan runs on 48-bit fixed point (int64 sums are associative): every CDF is non-decreasing whatever the order of the
// partial sums, and the device and the host emulator produce the same bits.  The normalising sums are f64 -- a few
// thousand cells per image, the kernels are latency bound.
#define EM_THREADS 256
#define EM_PER 8
#define EM_FIX 281474976710656.0        // 2^48

__device__ __forceinline__ int em_cell_axis(float x, int n) {        // clamp(int(x n), 0, n - 1), NaN -> 0
  const float s = x * (float)n;
  if (!(s >= 1.0f)) return 0;
  if (s >= (float)n) return n - 1;
  return (int)s;
}

__global__ void __launch_bounds__(256) k_errmap_accumulate(const int64_t* __restrict__ fidx, int64_t fidx_stride,
                                                            const float* __restrict__ xy, const float* __restrict__ val,
                                                            const float* __restrict__ pred, const float* __restrict__ gt,
                                                            int fn, int64_t N, int64_t V, int h, int w,
                                                            float* __restrict__ sum, float* __restrict__ cnt,
                                                            int32_t* __restrict__ touched, float* __restrict__ err_out) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= N) return;
  float e;
  if (val) {
    e = val[r];
  } else {       // mean_c fn(pred - gt): ``mse`` (fn 0) or ``l1`` (fn 1), app/loss/photometric.py:111-112
    const float d0 = pred[3 * r] - gt[3 * r], d1 = pred[3 * r + 1] - gt[3 * r + 1], d2 = pred[3 * r + 2] - gt[3 * r + 2];
    e = fn == 1 ? ((fabsf(d0) + fabsf(d1)) + fabsf(d2)) / 3.0f : ((d0 * d0 + d1 * d1) + d2 * d2) / 3.0f;
  }
  if (err_out) err_out[r] = e;
  const int64_t i = fidx[r * fidx_stride];
  if (i < 0 || i >= V) return;          // a frame outside the map: nothing to account it to
  const int cx = em_cell_axis(xy[2 * r], w), cy = em_cell_axis(xy[2 * r + 1], h);
  const int64_t flat = (i * h + cy) * w + cx;
  atomicAdd(sum + flat, e);
  atomicAdd(cnt + flat, 1.0f);
  touched[i] = 1;                       // (every writer stores the same word)
}

__global__ void __launch_bounds__(256) k_errmap_blend(float* __restrict__ em, float* __restrict__ sum, float* __restrict__ cnt,
                                                       int32_t* __restrict__ touched, int64_t* __restrict__ n_steps,
                                                       int64_t V, int64_t n_cells) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n_cells; c += stride) {
    const float k = cnt[c];
    if (k > 0.0f) {
      em[c] = 0.5f * em[c] + 0.5f * (sum[c] / k);
      sum[c] = 0.0f;
      cnt[c] = 0.0f;
    }
  }
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < V; i += stride) {
    if (touched[i]) {
      n_steps[i] += 1;
      touched[i] = 0;
    }
  }
}

// sum of v over the workgroup, returned to every thread (sh: EM_THREADS / 64 words; two barriers)
__device__ __forceinline__ double em_block_sum(double v, double* sh) {
  const double ws = wave_sum(v);
  __syncthreads();                      // (the previous use of sh is over)
  if (nsim_lane() == 0) sh[threadIdx.x >> 6] = ws;
  __syncthreads();
  double t = 0.0;
#pragma unroll
  for (int k = 0; k < EM_THREADS / 64; ++k) t += sh[k];
  return t;
}

// the pdf of one cell before its last normalisation (ErrorMap.get_pdf): max(em, 0) + 1e-12, / S1, clamped from below to
// min_pdf / (h w) and -- hi > 0 -- from above to hi
__device__ __forceinline__ double em_clamped(float e, double inv_s1, double lo, double hi) {
  double p = ((double)fmaxf(e, 0.0f) + 1e-12) * inv_s1;
  p = p > lo ? p : lo;
  if (hi > 0.0) p = p < hi ? p : hi;
  return p;
}

// One workgroup per image; thread t owns EM_PER consecutive cells of every chunk of EM_THREADS * EM_PER (the arrangement of
// k_pack_infos_from_n: one serial prefix per thread, one wave scan, the wave totals through LDS), chunks chained by a
// carried running sum, so any h w >= 1 is covered.
__global__ void __launch_bounds__(EM_THREADS) k_errmap_cdf(const float* __restrict__ em, int hw, float min_pdf, float max_pdf,
                                                            float* __restrict__ cdf_cell, float* __restrict__ pdf_cell,
                                                            float* __restrict__ mass) {
  __shared__ double sh[EM_THREADS / 64];
  __shared__ int64_t wtot[EM_THREADS / 64];
  const int tid = threadIdx.x, lane = nsim_lane(), wave = tid >> 6;
  const int64_t img = blockIdx.x;
  const float* e = em + img * hw;
  double s1 = 0.0, m = 0.0;
  for (int c = tid; c < hw; c += EM_THREADS) {
    const float v = e[c];
    s1 += (double)fmaxf(v, 0.0f) + 1e-12;
    m += (double)v;
  }
  s1 = em_block_sum(s1, sh);
  m = em_block_sum(m, sh);
  if (tid == 0) mass[img] = (float)m;
  const double inv_s1 = 1.0 / s1, lo = (double)min_pdf / (double)hw;
  const double hi = max_pdf >= 0.0f ? (double)fmaxf(max_pdf, 1.0f) : -1.0;
  double s2 = 0.0;
  for (int c = tid; c < hw; c += EM_THREADS) s2 += em_clamped(e[c], inv_s1, lo, hi);
  s2 = em_block_sum(s2, sh);
  const double inv_s2 = 1.0 / s2;
  int64_t carry = 0;
  for (int base = 0; base < hw; base += EM_THREADS * EM_PER) {
    const int c0 = base + tid * EM_PER;
    int64_t v[EM_PER];
    int64_t mine = 0;
#pragma unroll
    for (int k = 0; k < EM_PER; ++k) {
      v[k] = 0;
      if (c0 + k < hw) {
        const double p = em_clamped(e[c0 + k], inv_s1, lo, hi) * inv_s2;
        if (pdf_cell) pdf_cell[img * hw + c0 + k] = (float)p;
        v[k] = (int64_t)(p * EM_FIX + 0.5);
      }
      mine += v[k];
    }
    const int64_t incl = wave_incl_sum(mine);
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    int64_t before = 0, chunk = 0;
#pragma unroll
    for (int k = 0; k < EM_THREADS / 64; ++k) {
      const int64_t x = wtot[k];
      before += (k < wave) ? x : 0;
      chunk += x;
    }
    int64_t run = carry + before + incl - mine;
#pragma unroll
    for (int k = 0; k < EM_PER; ++k) {
      run += v[k];
      if (c0 + k < hw) cdf_cell[img * hw + c0 + k] = (c0 + k == hw - 1) ? 1.0f : fminf((float)((double)run * (1.0 / EM_FIX)), 1.0f);
    }
    carry += chunk;
    __syncthreads();
  }
}

// image level: pdf_img = mass / max(sum mass, 1e-12) (ErrorMap.get_pdf_image) and its inclusive scan, last entry 1.  One
// workgroup.  The scan takes max(mass, 0); when no image carries mass every image gets the same share.
__global__ void __launch_bounds__(EM_THREADS) k_errmap_cdf_img(const float* __restrict__ mass, int64_t V,
                                                                float* __restrict__ cdf_img, float* __restrict__ pdf_img) {
  __shared__ double sh[EM_THREADS / 64];
  __shared__ int64_t wtot[EM_THREADS / 64];
  const int tid = threadIdx.x, lane = nsim_lane(), wave = tid >> 6;
  double tot = 0.0, pos = 0.0;
  for (int64_t i = tid; i < V; i += EM_THREADS) {
    tot += (double)mass[i];
    pos += (double)fmaxf(mass[i], 0.0f);
  }
  tot = em_block_sum(tot, sh);
  pos = em_block_sum(pos, sh);
  const double inv_tot = 1.0 / (tot > 1e-12 ? tot : 1e-12);
  const bool flat = !(pos > 0.0);
  const double inv_pos = flat ? 0.0 : 1.0 / pos, share = 1.0 / (double)V;
  int64_t carry = 0;
  for (int64_t base = 0; base < V; base += EM_THREADS) {
    const int64_t i = base + tid;
    int64_t mine = 0;
    if (i < V) {
      const float mi = mass[i];
      pdf_img[i] = (float)((double)mi * inv_tot);
      mine = (int64_t)((flat ? share : (double)fmaxf(mi, 0.0f) * inv_pos) * EM_FIX + 0.5);
    }
    const int64_t incl = wave_incl_sum(mine);
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    int64_t before = 0, chunk = 0;
#pragma unroll
    for (int k = 0; k < EM_THREADS / 64; ++k) {
      const int64_t x = wtot[k];
      before += (k < wave) ? x : 0;
      chunk += x;
    }
    if (i < V) cdf_img[i] = (i == V - 1) ? 1.0f : fminf((float)((double)(carry + before + incl) * (1.0 / EM_FIX)), 1.0f);
    carry += chunk;
    __syncthreads();
  }
}

// the first index in [0, n) whose entry is > u, clamped to n - 1 (cdf non-decreasing)
__device__ __forceinline__ int64_t em_upper(const float* __restrict__ cdf, int64_t n, float u) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (cdf[mid] > u) hi = mid;
    else lo = mid + 1;
  }
  return lo < n - 1 ? lo : n - 1;
}

// (c + u) / n, moved by single ulps until int(x n) == c again (c + u may round up to c + 1, c / n may round below the border):
// the cell a pixel was drawn from is the cell its error is accounted to
__device__ __forceinline__ float em_in_cell(int c, float u, int n, float lo, float hi) {
  float x = ((float)c + u) / (float)n;
  for (int it = 0; it < 4; ++it) {
    const int k = (int)(x * (float)n);
    if (k == c) break;
    x = nextafterf(x, k < c ? 2.0f : -1.0f);
  }
  return fminf(fmaxf(x, lo), hi);
}

__global__ void __launch_bounds__(256) k_errmap_draw(const float* __restrict__ cdf_img, const float* __restrict__ cdf_cell,
                                                      int64_t V, int h, int w, const float* __restrict__ u, int64_t n,
                                                      int64_t n_uni, int64_t fixed_frame, int64_t row0,
                                                      int64_t* __restrict__ fidx_out, float* __restrict__ xy_out) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int64_t r = row0 + j;
  const float u0 = u[4 * r], u1 = u[4 * r + 1], u2 = u[4 * r + 2], u3 = u[4 * r + 3];
  const float lo = (float)1e-6, hi = (float)(1.0 - 1e-6);        // cameras.py:247 ``clamp_(1e-6, 1 - 1e-6)``
  int64_t f;
  float x, y;
  if (j < n_uni) {
    if (fixed_frame >= 0) {
      f = fixed_frame;
    } else {
      const float s = u0 * (float)V;
      f = s >= (float)V ? V - 1 : (s >= 0.0f ? (int64_t)s : 0);
    }
    x = fminf(fmaxf(u2, lo), hi);
    y = fminf(fmaxf(u3, lo), hi);
  } else {
    f = fixed_frame >= 0 ? fixed_frame : em_upper(cdf_img, V, u0);
    const int64_t hw = (int64_t)h * w;
    const int64_t c = em_upper(cdf_cell + f * hw, hw, u1);
    const int cy = (int)(c / w), cx = (int)(c - (int64_t)cy * w);
    x = em_in_cell(cx, u2, w, lo, hi);
    y = em_in_cell(cy, u3, h, lo, hi);
  }
  if (fidx_out) fidx_out[r] = f;
  xy_out[2 * r] = x;
  xy_out[2 * r + 1] = y;
}

extern "C" {

static inline int em_check_sizes(int64_t V, int h, int w) {
  if (V < 1 || h < 1 || w < 1) return 54;
  if ((double)V * (double)h * (double)w >= 2147483648.0) return 54;
  return 0;
}

int nsim_errmap_accumulate(const int64_t* fidx, int64_t fidx_stride, const float* xy, const float* val, const float* pred,
                           const float* gt, int fn, int64_t N, int64_t n_images, int h, int w, float* sum, float* cnt,
                           int32_t* touched, float* err_out, void* stream) {
  if (N <= 0) return 0;
  if (int rc = em_check_sizes(n_images, h, w)) return rc;
  if (!fidx || !xy || !sum || !cnt || !touched || (!val && !(pred && gt))) return 4;
  if ((fidx_stride != 0 && fidx_stride != 1) || (fn != 0 && fn != 1)) return 3;
  hipLaunchKernelGGL(k_errmap_accumulate, dim3(nsim_blocks(N, 256)), dim3(256), 0, (hipStream_t)stream, fidx, fidx_stride, xy,
                     val, pred, gt, fn, N, n_images, h, w, sum, cnt, touched, err_out);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_errmap_blend(float* em, float* sum, float* cnt, int32_t* touched, int64_t* n_steps, int64_t n_images, int h, int w,
                      void* stream) {
  if (int rc = em_check_sizes(n_images, h, w)) return rc;
  if (!em || !sum || !cnt || !touched || !n_steps) return 4;
  const int64_t n_cells = n_images * h * w;
  hipLaunchKernelGGL(k_errmap_blend, dim3(nsim_blocks(n_cells > n_images ? n_cells : n_images, 256, 4096)), dim3(256), 0,
                     (hipStream_t)stream, em, sum, cnt, touched, n_steps, n_images, n_cells);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_errmap_cdf(const float* em, int64_t n_images, int h, int w, float min_pdf, float max_pdf, float* cdf_cell,
                    float* pdf_cell, float* mass, float* cdf_img, float* pdf_img, void* stream) {
  if (int rc = em_check_sizes(n_images, h, w)) return rc;
  if (!em || !cdf_cell || !mass || !cdf_img || !pdf_img) return 4;
  hipLaunchKernelGGL(k_errmap_cdf, dim3((unsigned)n_images), dim3(EM_THREADS), 0, (hipStream_t)stream, em, h * w, min_pdf,
                     max_pdf, cdf_cell, pdf_cell, mass);
  NSIM_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_errmap_cdf_img, dim3(1), dim3(EM_THREADS), 0, (hipStream_t)stream, (const float*)mass, n_images, cdf_img,
                     pdf_img);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_errmap_draw(const float* cdf_img, const float* cdf_cell, int64_t n_images, int h, int w, const float* u, int64_t n,
                     int64_t n_uni, int64_t fixed_frame, int64_t row0, int64_t* fidx_out, float* xy_out, void* stream) {
  if (n <= 0) return 0;
  if (int rc = em_check_sizes(n_images, h, w)) return rc;
  if (n_uni < 0 || row0 < 0) return 2;
  if (fixed_frame >= n_images) return 54;
  if (!u || !xy_out || (n_uni < n && (!cdf_cell || (fixed_frame < 0 && !cdf_img)))) return 4;
  hipLaunchKernelGGL(k_errmap_draw, dim3(nsim_blocks(n, 256)), dim3(256), 0, (hipStream_t)stream, cdf_img, cdf_cell, n_images, h,
                     w, u, n, n_uni, fixed_frame, row0, fidx_out, xy_out);
  NSIM_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
