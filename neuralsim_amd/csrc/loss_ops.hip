// loss_ops.hip -- fused reductions of the losses the training step evaluates on the path's outputs (SURVEY sec. 8 row
// a18) and the gradient of the per-frame appearance-embedding lookup.
//   * eikonal: mean((|nablas| - 1)^2)                 (app/loss/eikonal.py:96-105 with safe_mse off, alpha_reg_zero 0)
//   * photometric mse: mean((pred - gt)^2)            (app/loss/photometric.py:88-146, fn_type mse, no mask)
//   * rows_scatter_add: d embed[idx[i], :] += g[i, :]  (app/models/scene/image_embeddings.py:23-80: ``embed[fidx]``)
//   * sdf curvature: acos(n0^ . n1^) / pi of the nablas at a point and at its tangentially shifted neighbour, the shift
//     itself, and mean(min(curvature, clamp_max))     (model.get_sdf_curvature_1d + SDFCurvatureRegLoss.fn,
//     app/loss/sdf_curvature.py:42,69,75; the regulariser of PermutoSDF, Rosu & Behnke 2023)
//   * ssim / s3im: mean SSIM of two images, planar or gathered through an index from [N,3] rows (the virtual image of S3IM,
//     Xie et al. 2023), gradient to the first    (nr3d_lib.models.loss.ssim.ssim_module under app/loss/perceptual.py:61-70, 142-157)
// The reference evaluates these with a handful of torch ops each; here one launch per direction, because at 8192
// rays per iteration the step is bounded by launch count, not by bytes.
#include "nsim_common.h"

#define LOSS_BLOCK 256
#define LOSS_MAX_BLOCKS 256

__device__ __forceinline__ void block_sum_atomic(float v, float scale, float* out) {
  __shared__ float red[LOSS_BLOCK / 64];
  v = wave_sum(v);
  if (nsim_lane() == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    float tot = 0.f;
    for (int w = 0; w < LOSS_BLOCK / 64; ++w) tot += red[w];
    if (tot != 0.f) atomicAdd(out, tot * scale);
  }
}

__global__ void __launch_bounds__(LOSS_BLOCK) k_eikonal_fwd(const float* __restrict__ nab, int64_t S, float inv_S,
                                                            float* __restrict__ out) {
  float acc = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * LOSS_BLOCK + threadIdx.x; i < S; i += (int64_t)gridDim.x * LOSS_BLOCK) {
    const float a = nab[3 * i], b = nab[3 * i + 1], c = nab[3 * i + 2];
    const float e = sqrtf(a * a + b * b + c * c) - 1.0f;
    acc += e * e;
  }
  block_sum_atomic(acc, inv_S, out);
}

__global__ void __launch_bounds__(LOSS_BLOCK) k_eikonal_bwd(const float* __restrict__ nab, int64_t S, float inv_S,
                                                            const float* __restrict__ gout, float* __restrict__ dnab) {
  const int64_t i = (int64_t)blockIdx.x * LOSS_BLOCK + threadIdx.x;
  if (i >= S) return;
  const float a = nab[3 * i], b = nab[3 * i + 1], c = nab[3 * i + 2];
  const float nrm = sqrtf(a * a + b * b + c * c);
  // d/dn (|n|-1)^2 = 2 (|n|-1) n/|n|; the sub-gradient at n = 0 is 0 (as torch.norm's backward)
  const float k = nrm > 0.f ? gout[0] * inv_S * 2.0f * (nrm - 1.0f) / nrm : 0.f;
  dnab[3 * i] = k * a;
  dnab[3 * i + 1] = k * b;
  dnab[3 * i + 2] = k * c;
}

__global__ void __launch_bounds__(LOSS_BLOCK) k_mse_fwd(const float* __restrict__ a, const float* __restrict__ b,
                                                        int64_t n, float inv_n, float* __restrict__ out) {
  float acc = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * LOSS_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * LOSS_BLOCK) {
    const float e = a[i] - b[i];
    acc += e * e;
  }
  block_sum_atomic(acc, inv_n, out);
}

__global__ void __launch_bounds__(LOSS_BLOCK) k_mse_bwd(const float* __restrict__ a, const float* __restrict__ b,
                                                        int64_t n, float inv_n, const float* __restrict__ gout,
                                                        float* __restrict__ da) {
  const int64_t i = (int64_t)blockIdx.x * LOSS_BLOCK + threadIdx.x;
  if (i >= n) return;
  da[i] = gout[0] * inv_n * 2.0f * (a[i] - b[i]);
}

// The training step's loss head in ONE launch (six otherwise): acc[0] += mse(pred, gt), acc[1] += eikonal(nab[:S]),
// acc[2] += eikonal(nab[S:S+M]) and the gradients of  mse + w_eik (eik + eik)  -- d_img = 2 (pred - gt) / n and
// dnab = w_eik 2 (|n| - 1) n / (|n| count).  None of the gradients needs the loss VALUE, so there is no second pass.
__global__ void __launch_bounds__(LOSS_BLOCK) k_loss_head(const float* __restrict__ pred, const float* __restrict__ gt,
                                                          int64_t n_img, const float* __restrict__ nab, int64_t S,
                                                          int64_t M, float w_eik, float* __restrict__ acc,
                                                          float* __restrict__ d_img, float* __restrict__ dnab) {
  __shared__ float red[3][LOSS_BLOCK / 64];
  const float inv_n = 1.0f / (float)n_img, inv_S = 1.0f / (float)(S > 0 ? S : 1), inv_M = 1.0f / (float)(M > 0 ? M : 1);
  const int64_t St = S + M, top = n_img > St ? n_img : St;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * LOSS_BLOCK + threadIdx.x; i < top; i += (int64_t)gridDim.x * LOSS_BLOCK) {
    if (i < n_img) {
      const float e = pred[i] - gt[i];
      a0 += e * e;
      d_img[i] = inv_n * 2.0f * e;
    }
    if (i < St) {
      const float a = nab[3 * i], b = nab[3 * i + 1], c = nab[3 * i + 2];
      const float nrm = sqrtf(a * a + b * b + c * c);
      const float e = nrm - 1.0f;
      const bool ren = i < S;
      if (ren) a1 += e * e;
      else a2 += e * e;
      const float k = nrm > 0.f ? w_eik * (ren ? inv_S : inv_M) * 2.0f * (nrm - 1.0f) / nrm : 0.f;
      dnab[3 * i] = k * a;
      dnab[3 * i + 1] = k * b;
      dnab[3 * i + 2] = k * c;
    }
  }
  a0 = wave_sum(a0);
  a1 = wave_sum(a1);
  a2 = wave_sum(a2);
  if (nsim_lane() == 0) {
    red[0][threadIdx.x >> 6] = a0;
    red[1][threadIdx.x >> 6] = a1;
    red[2][threadIdx.x >> 6] = a2;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    float tot = 0.f;
    for (int w = 0; w < LOSS_BLOCK / 64; ++w) tot += red[threadIdx.x][w];
    const float sc = threadIdx.x == 0 ? inv_n : (threadIdx.x == 1 ? inv_S : inv_M);
    if (tot != 0.f) atomicAdd(acc + threadIdx.x, tot * sc);
  }
}

// rows * C <= ROWS_LDS_MAX: per-block LDS histogram (the few hundred frame embeddings are hit by thousands of rays),
// flushed with one global atomic per touched entry; larger tables go straight to global atomics.
#define ROWS_LDS_MAX 4096
__global__ void __launch_bounds__(LOSS_BLOCK) k_rows_scatter_add(const float* __restrict__ g,
                                                                 const int64_t* __restrict__ idx, int64_t n, int C,
                                                                 int64_t rows, float* __restrict__ out) {
  __shared__ float acc[ROWS_LDS_MAX];
  const int64_t tot = rows * C;
  const bool use_lds = tot <= ROWS_LDS_MAX;
  if (use_lds) {
    for (int j = threadIdx.x; j < tot; j += LOSS_BLOCK) acc[j] = 0.f;
    __syncthreads();
  }
  const int64_t nC = n * C;
  for (int64_t i = (int64_t)blockIdx.x * LOSS_BLOCK + threadIdx.x; i < nC; i += (int64_t)gridDim.x * LOSS_BLOCK) {
    const int64_t r = idx[i / C];
    if (r < 0 || r >= rows) continue;
    const int64_t j = r * C + (i % C);
    if (use_lds) atomicAdd(&acc[j], g[i]);
    else atomicAdd(&out[j], g[i]);
  }
  if (use_lds) {
    __syncthreads();
    for (int j = threadIdx.x; j < tot; j += LOSS_BLOCK) {
      const float v = acc[j];
      if (v != 0.f) atomicAdd(&out[j], v);
    }
  }
}

// analytic image of a sphere at the origin along unit rays: 0.5 + 0.5 n at the first hit, black elsewhere
// (synthetic multi-view-consistent supervision of bench.py; one launch instead of ~10 elementwise torch ops)
__global__ void __launch_bounds__(LOSS_BLOCK) k_sphere_image(const float* __restrict__ o, const float* __restrict__ d,
                                                             int64_t N, float radius, float* __restrict__ rgb) {
  const int64_t i = (int64_t)blockIdx.x * LOSS_BLOCK + threadIdx.x;
  if (i >= N) return;
  const float ox = o[3 * i], oy = o[3 * i + 1], oz = o[3 * i + 2];
  const float dx = d[3 * i], dy = d[3 * i + 1], dz = d[3 * i + 2];
  const float b = ox * dx + oy * dy + oz * dz;
  const float c = ox * ox + oy * oy + oz * oz - radius * radius;
  const float disc = b * b - c;
  const float t = -b - sqrtf(fmaxf(disc, 0.f));
  const bool hit = disc > 0.f && t > 0.f;
  const float inv = 1.0f / radius;
  rgb[3 * i] = hit ? 0.5f + 0.5f * (ox + t * dx) * inv : 0.f;
  rgb[3 * i + 1] = hit ? 0.5f + 0.5f * (oy + t * dy) * inv : 0.f;
  rgb[3 * i + 2] = hit ? 0.5f + 0.5f * (oz + t * dz) * inv : 0.f;
}

// compaction of the AABB-tested rays: (o, d, near, far)[idx] in one launch (model.ray_test)
__global__ void __launch_bounds__(LOSS_BLOCK) k_gather_rays(const float* __restrict__ o, const float* __restrict__ d,
                                                            const float* __restrict__ near, const float* __restrict__ far,
                                                            const int64_t* __restrict__ idx, int64_t R,
                                                            float* __restrict__ o_out, float* __restrict__ d_out,
                                                            float* __restrict__ near_out, float* __restrict__ far_out) {
  const int64_t i = (int64_t)blockIdx.x * LOSS_BLOCK + threadIdx.x;
  if (i >= R) return;
  const int64_t r = idx[i];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    o_out[3 * i + c] = o[3 * r + c];
    d_out[3 * i + c] = d[3 * r + c];
  }
  near_out[i] = near[r];
  far_out[i] = far[r];
}

// ---------------------------------------------------------------------------------------------- sdf curvature
// A lane owns one point: its three floats are one 12-byte load (the wave reads 768 contiguous bytes, every byte of every cache
// line it touches is used), as k_eikonal_* read their nablas.  Plain f32, no LDS beyond the block reduction.
#define CURV_MAX_BLOCKS 2048          // elementwise kernels: 8 blocks per CU, the rest by grid stride
#define CURV_NORM_MIN 1e-12f          // n^ = n / max(|n|, 1e-12); a shorter vector gets NO gradient (departs from F.normalize)
#define CURV_DOT_MAX 0x1.ffffdep-1f   // f32(1 - 1e-6) = 1 - 1.0133e-6: the clamp of the dot product
#define CURV_AT_DOT_MAX 0x1.db2614p-12f   // f32(acos( CURV_DOT_MAX) / pi) = 4.5313715e-4
#define CURV_AT_DOT_MIN 0x1.ffc49cp-1f    // f32(acos(-CURV_DOT_MAX) / pi) = 1 - 4.5313715e-4
#define CURV_ANGLE_MIN 0x1.752e52p-10f     // f32(acos(CURV_DOT_MAX)) = 1.4235723e-3 rad
#define CURV_PI 3.14159265358979f

struct CurvUnit {
  float x, y, z, len;
};

__device__ __forceinline__ CurvUnit curv_unit(const float* __restrict__ v, int64_t i) {
  const float a = v[3 * i], b = v[3 * i + 1], c = v[3 * i + 2];
  CurvUnit u;
  u.len = sqrtf(a * a + b * b + c * c);
  const float inv = 1.0f / fmaxf(u.len, CURV_NORM_MIN);
  u.x = a * inv;
  u.y = b * inv;
  u.z = c * inv;
  return u;
}

// curvature of one pair of normalised vectors and d curvature / d dot (0 where the clamp of the dot product is active -- there the
// curvature is one of two constants).  The ONE angle function of the elementwise and the fused kernels.
// The angle is taken as atan2(|n0^ x n1^|, |n0^ . n1^|), not as acos of the dot product: just inside the clamp d acos / d dot is
// 1 / sqrt(2e-6) = 700, which turns the 6e-8 rounding of an f32 dot product near 1 into 1.3e-5 of curvature per ulp; the cross
// product keeps its relative precision down to the clamp angle (1.4e-3 rad), so does the gradient's 1 / sin.
__device__ __forceinline__ float curv_angle(const CurvUnit& u0, const CurvUnit& u1, float* dot_out, float* dcurv_ddot) {
  const float dot = u0.x * u1.x + u0.y * u1.y + u0.z * u1.z;
  *dot_out = dot;
  *dcurv_ddot = 0.f;
  if (u0.len < CURV_NORM_MIN || u1.len < CURV_NORM_MIN) {
    // a vector below the norm floor is not a unit vector: the formula as it stands, acos(clamp(dot)) / pi (|dot| < 1 here)
    if (dot >= CURV_DOT_MAX) return CURV_AT_DOT_MAX;
    if (dot <= -CURV_DOT_MAX) return CURV_AT_DOT_MIN;
    *dcurv_ddot = -1.0f / (CURV_PI * sqrtf((1.0f - dot) * (1.0f + dot)));
    return acosf(dot) / CURV_PI;
  }
  const float cx = u0.y * u1.z - u0.z * u1.y, cy = u0.z * u1.x - u0.x * u1.z, cz = u0.x * u1.y - u0.y * u1.x;
  const float sn = sqrtf(cx * cx + cy * cy + cz * cz);
  const float th = atan2f(sn, fabsf(dot));            // angle to the nearer of +-n1^, in [0, pi/2]
  if (th <= CURV_ANGLE_MIN) return dot > 0.f ? CURV_AT_DOT_MAX : CURV_AT_DOT_MIN;
  *dcurv_ddot = -1.0f / (CURV_PI * sn);
  const float c = th / CURV_PI;
  return dot >= 0.f ? c : 1.0f - c;
}

// d n [3] = k (d dot / d n) with d dot / d n = (other^ - dot n^) / |n| through the normalisation; 0 below CURV_NORM_MIN
__device__ __forceinline__ void curv_store_grad(float* __restrict__ dn, int64_t i, float k, float dot, const CurvUnit& u,
                                                const CurvUnit& o) {
  const float s = u.len >= CURV_NORM_MIN ? k / u.len : 0.f;
  dn[3 * i] = s * (o.x - dot * u.x);
  dn[3 * i + 1] = s * (o.y - dot * u.y);
  dn[3 * i + 2] = s * (o.z - dot * u.z);
}

// x_out = clamp(x + eps (n^ x r^), aabb): the tangential neighbour the second query runs at (|shift| = eps sin(n^, r^) <= eps)
__global__ void __launch_bounds__(LOSS_BLOCK) k_curv_shift(const float* __restrict__ nab, const float* __restrict__ x,
                                                           const float* __restrict__ dirs, const float* __restrict__ lo,
                                                           const float* __restrict__ hi, float eps, int64_t n,
                                                           float* __restrict__ x_out) {
  const float lx = lo[0], ly = lo[1], lz = lo[2], hx = hi[0], hy = hi[1], hz = hi[2];
  for (int64_t i = (int64_t)blockIdx.x * LOSS_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * LOSS_BLOCK) {
    const CurvUnit u = curv_unit(nab, i), r = curv_unit(dirs, i);
    const float tx = u.y * r.z - u.z * r.y, ty = u.z * r.x - u.x * r.z, tz = u.x * r.y - u.y * r.x;
    x_out[3 * i] = fminf(fmaxf(x[3 * i] + eps * tx, lx), hx);
    x_out[3 * i + 1] = fminf(fmaxf(x[3 * i + 1] + eps * ty, ly), hy);
    x_out[3 * i + 2] = fminf(fmaxf(x[3 * i + 2] + eps * tz, lz), hz);
  }
}

__global__ void __launch_bounds__(LOSS_BLOCK) k_curv_angle_fwd(const float* __restrict__ n0, const float* __restrict__ n1,
                                                               int64_t n, float* __restrict__ curv) {
  for (int64_t i = (int64_t)blockIdx.x * LOSS_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * LOSS_BLOCK) {
    float dot, dc;
    curv[i] = curv_angle(curv_unit(n0, i), curv_unit(n1, i), &dot, &dc);
  }
}

// recomputes the dot product from the inputs (the forward's output is the caller's to modify in place); dn0 / dn1 may be NULL
__global__ void __launch_bounds__(LOSS_BLOCK) k_curv_angle_bwd(const float* __restrict__ n0, const float* __restrict__ n1,
                                                               const float* __restrict__ gcurv, int64_t n,
                                                               float* __restrict__ dn0, float* __restrict__ dn1) {
  for (int64_t i = (int64_t)blockIdx.x * LOSS_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * LOSS_BLOCK) {
    const CurvUnit u0 = curv_unit(n0, i), u1 = curv_unit(n1, i);
    float dot, dc;
    curv_angle(u0, u1, &dot, &dc);
    const float k = gcurv[i] * dc;
    if (dn0) curv_store_grad(dn0, i, k, dot, u0, u1);
    if (dn1) curv_store_grad(dn1, i, k, dot, u1, u0);
  }
}

__global__ void __launch_bounds__(LOSS_BLOCK) k_curv_loss_fwd(const float* __restrict__ n0, const float* __restrict__ n1,
                                                              int64_t n, float inv_n, float clamp_max,
                                                              float* __restrict__ out) {
  float acc = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * LOSS_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * LOSS_BLOCK) {
    float dot, dc;
    acc += fminf(curv_angle(curv_unit(n0, i), curv_unit(n1, i), &dot, &dc), clamp_max);
  }
  block_sum_atomic(acc, inv_n, out);
}

// d mean(min(curvature, clamp_max)): the min passes the gradient where curvature <= clamp_max (torch's clamp_max_)
__global__ void __launch_bounds__(LOSS_BLOCK) k_curv_loss_bwd(const float* __restrict__ n0, const float* __restrict__ n1,
                                                              int64_t n, float inv_n, float clamp_max,
                                                              const float* __restrict__ gout, float* __restrict__ dn0,
                                                              float* __restrict__ dn1) {
  const float g = gout[0] * inv_n;
  for (int64_t i = (int64_t)blockIdx.x * LOSS_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * LOSS_BLOCK) {
    const CurvUnit u0 = curv_unit(n0, i), u1 = curv_unit(n1, i);
    float dot, dc;
    const float c = curv_angle(u0, u1, &dot, &dc);
    const float k = c <= clamp_max ? g * dc : 0.f;
    if (dn0) curv_store_grad(dn0, i, k, dot, u0, u1);
    if (dn1) curv_store_grad(dn1, i, k, dot, u1, u0);
  }
}

// ---------------------------------------------------------------------------------------------- ssim / s3im
// SSIM of two images under a k x k Gaussian window (sigma 1.5, zero padding (k - 1) / 2, stride s, per channel) and its gradient
// with respect to the first image, in two addressings of ONE kernel family (the template argument CH):
//   CH = 1  planar: BC = B * C independent single-channel images [BC, H, W];
//   CH = 3  indexed: ONE three-channel image [3, H, W] whose pixel (i, j) is row index[i * W + j] of the [n_rows, 3] arrays -- the
//           virtual image of S3IM (app/loss/perceptual.py:151-156), never materialised.  An index outside [0, n_rows) is a zero
//           pixel that receives no gradient.
// Forward: one thread per window position (its CH channels in turn), two passes over the window -- the weighted means, then the
// moments ABOUT the means -- and three coefficients per window for the backward.  Backward: one thread per pixel, a gather over
// the windows that cover it (at most ceil(k / s)^2: one for s >= k, 121 for k = 11, s = 1), stored (planar) or added atomically
// into the pixel's row (indexed: a row occurs once per repeat of the virtual image).
//
// With dm = mu2 - mu1, sdd = sum g ((x - mu1) - (y - mu2))^2 = s11 + s22 - 2 s12, B1 = mu1^2 + mu2^2 + C1, B2 = s11 + s22 + C2:
//   ssim = (1 - dm^2 / B1) (1 - sdd / B2)                  [2 mu1 mu2 + C1 = B1 - dm^2,  2 s12 + C2 = B2 - sdd]
//   d ssim / d x_v = g_v (alpha + beta x_v + gamma (y_v - x_v)),
//   gamma = d ssim / d s12 = 2 (1 - dm^2 / B1) / B2,   beta = 2 d ssim / d s11 + gamma = gamma sdd / B2,
//   alpha = d ssim / d mu1 - beta mu1 - gamma dm,      d ssim / d mu1 = (2 / B1) (1 - sdd / B2) (dm + mu1 dm^2 / B1).
// Every difference of nearly equal numbers is taken between INPUTS (y_v - x_v, x_v - mu1), never between products of the size of
// 1 / C2: on flat bright images the textbook form E[x^2] - mu^2 loses 2e-5 of the value and 8e-4 of the gradient in f32.
#define SSIM_MAX_WIN 11
#define SSIM_C1 ((float)(0.01 * 0.01))
#define SSIM_C2 ((float)(0.03 * 0.03))

struct SsimArgs {
  const float* x;
  const float* y;
  const int64_t* index;      // CH = 3 only
  int64_t n_rows;            // CH = 3 only
  int64_t BC;
  int H, W, Ho, Wo, k, s, p;
  float g[SSIM_MAX_WIN];     // the 1-D window, normalised to sum 1 in double on the host
};

// offset of channel 0 of pixel (iy, ix) of image bc, -1 for an index outside the rows (CH = 3)
template <int CH>
__device__ __forceinline__ int64_t ssim_base(const SsimArgs& a, int64_t bc, int iy, int ix) {
  if (CH == 1) return (bc * a.H + iy) * (int64_t)a.W + ix;
  const int64_t r = a.index[(int64_t)iy * a.W + ix];
  return (r >= 0 && r < a.n_rows) ? 3 * r : -1;
}

// coef [3, nW] (alpha, beta, gamma), nW = BC * CH * Ho * Wo, window id = ((bc * CH + c) * Ho + oy) * Wo + ox
template <int CH>
__global__ void __launch_bounds__(LOSS_BLOCK) k_ssim_fwd(SsimArgs a, float inv_nw, float* __restrict__ out,
                                                         float* __restrict__ coef) {
  __shared__ float g[SSIM_MAX_WIN];
  if (threadIdx.x < SSIM_MAX_WIN) g[threadIdx.x] = threadIdx.x < a.k ? a.g[threadIdx.x] : 0.f;
  __syncthreads();
  const int64_t plane = (int64_t)a.Ho * a.Wo, sites = a.BC * plane, nW = sites * CH;
  float acc = 0.f;
  for (int64_t w = (int64_t)blockIdx.x * LOSS_BLOCK + threadIdx.x; w < sites; w += (int64_t)gridDim.x * LOSS_BLOCK) {
    const int64_t bc = w / plane;
    const int oy = (int)((w - bc * plane) / a.Wo), ox = (int)((w - bc * plane) % a.Wo);
    const int y0 = oy * a.s - a.p, x0 = ox * a.s - a.p;
    float m1[CH], dm[CH], s11[CH], s22[CH], sdd[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) m1[c] = dm[c] = s11[c] = s22[c] = sdd[c] = 0.f;
    // a pixel of the zero padding adds nothing to the means ...
    for (int i = 0; i < a.k; ++i) {
      const int iy = y0 + i;
      if (iy < 0 || iy >= a.H) continue;
      for (int j = 0; j < a.k; ++j) {
        const int ix = x0 + j;
        if (ix < 0 || ix >= a.W) continue;
        const int64_t b = ssim_base<CH>(a, bc, iy, ix);
        if (b < 0) continue;
        const float wg = g[i] * g[j];
#pragma unroll
        for (int c = 0; c < CH; ++c) {
          const float xv = a.x[b + c], yv = a.y[b + c];
          m1[c] += wg * xv;
          dm[c] += wg * (yv - xv);
        }
      }
    }
    // ... but its deviation from them counts
    for (int i = 0; i < a.k; ++i) {
      const int iy = y0 + i;
      const bool row_in = iy >= 0 && iy < a.H;
      for (int j = 0; j < a.k; ++j) {
        const int ix = x0 + j;
        const int64_t b = (row_in && ix >= 0 && ix < a.W) ? ssim_base<CH>(a, bc, iy, ix) : -1;
        const float wg = g[i] * g[j];
#pragma unroll
        for (int c = 0; c < CH; ++c) {
          const float xv = b >= 0 ? a.x[b + c] : 0.f, yv = b >= 0 ? a.y[b + c] : 0.f;
          const float dx = xv - m1[c], dd = (yv - xv) - dm[c], dy = dx + dd;
          s11[c] += wg * dx * dx;
          s22[c] += wg * dy * dy;
          sdd[c] += wg * dd * dd;
        }
      }
    }
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const float m2 = m1[c] + dm[c];
      const float B1 = m1[c] * m1[c] + m2 * m2 + SSIM_C1, B2 = s11[c] + s22[c] + SSIM_C2;
      const float lum = 1.0f - dm[c] * dm[c] / B1, cs = 1.0f - sdd[c] / B2;
      acc += lum * cs;
      const float gamma = 2.0f * lum / B2, beta = gamma * sdd[c] / B2;
      const float dmu1 = 2.0f / B1 * cs * (dm[c] + m1[c] * dm[c] * dm[c] / B1);
      const int64_t wid = (bc * CH + c) * plane + (int64_t)oy * a.Wo + ox;
      coef[wid] = dmu1 - beta * m1[c] - gamma * dm[c];
      coef[nW + wid] = beta;
      coef[2 * nW + wid] = gamma;
    }
  }
  block_sum_atomic(acc, inv_nw, out);
}

// dx: planar [BC, H, W], every element written (zero where no window covers the pixel); indexed [n_rows, 3], zero on entry
template <int CH>
__global__ void __launch_bounds__(LOSS_BLOCK) k_ssim_bwd(SsimArgs a, float inv_nw, const float* __restrict__ coef,
                                                         const float* __restrict__ gout, float* __restrict__ dx) {
  __shared__ float g[SSIM_MAX_WIN];
  if (threadIdx.x < SSIM_MAX_WIN) g[threadIdx.x] = threadIdx.x < a.k ? a.g[threadIdx.x] : 0.f;
  __syncthreads();
  const int64_t plane = (int64_t)a.Ho * a.Wo, nW = a.BC * plane * CH, img = (int64_t)a.H * a.W, npix = a.BC * img;
  const float sc = gout[0] * inv_nw;
  for (int64_t v = (int64_t)blockIdx.x * LOSS_BLOCK + threadIdx.x; v < npix; v += (int64_t)gridDim.x * LOSS_BLOCK) {
    const int64_t bc = v / img;
    const int iy = (int)((v - bc * img) / a.W), ix = (int)((v - bc * img) % a.W);
    const int64_t b = ssim_base<CH>(a, bc, iy, ix);
    if (b < 0) continue;
    // window oy holds row iy at tap iy + p - oy s in [0, k)
    int oy_lo = iy + a.p - a.k + 1, ox_lo = ix + a.p - a.k + 1;
    oy_lo = oy_lo > 0 ? (oy_lo + a.s - 1) / a.s : 0;
    ox_lo = ox_lo > 0 ? (ox_lo + a.s - 1) / a.s : 0;
    int oy_hi = (iy + a.p) / a.s, ox_hi = (ix + a.p) / a.s;
    oy_hi = oy_hi < a.Ho - 1 ? oy_hi : a.Ho - 1;
    ox_hi = ox_hi < a.Wo - 1 ? ox_hi : a.Wo - 1;
    float sa[CH], sb[CH], sg[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) sa[c] = sb[c] = sg[c] = 0.f;
    for (int oy = oy_lo; oy <= oy_hi; ++oy) {
      const float gy = g[iy + a.p - oy * a.s];
      for (int ox = ox_lo; ox <= ox_hi; ++ox) {
        const float wg = gy * g[ix + a.p - ox * a.s];
#pragma unroll
        for (int c = 0; c < CH; ++c) {
          const int64_t wid = (bc * CH + c) * plane + (int64_t)oy * a.Wo + ox;
          sa[c] += wg * coef[wid];
          sb[c] += wg * coef[nW + wid];
          sg[c] += wg * coef[2 * nW + wid];
        }
      }
    }
    const bool covered = oy_lo <= oy_hi && ox_lo <= ox_hi;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const float xv = a.x[b + c], yv = a.y[b + c];
      const float d = sc * (sa[c] + sb[c] * xv + sg[c] * (yv - xv));
      if (CH == 1) dx[b] = covered ? d : 0.f;
      else if (covered) atomicAdd(&dx[b + c], d);
    }
  }
}

// sizes of one call; 0 or the error code
static inline int ssim_args(SsimArgs* a, const float* x, const float* y, const int64_t* index, int64_t n_rows, int64_t BC, int H,
                            int W, int k, int s) {
  if (BC < 1 || H < 1 || W < 1 || k < 1 || k > SSIM_MAX_WIN || s < 1 || (int64_t)H * W >= ((int64_t)1 << 31)) return 55;
  if (index && (BC != 1 || n_rows < 0)) return 55;
  const int p = (k - 1) / 2;
  if (H + 2 * p - k < 0 || W + 2 * p - k < 0) return 55;        // no window fits (an even window on one row / column)
  a->x = x, a->y = y, a->index = index, a->n_rows = n_rows, a->BC = BC;
  a->H = H, a->W = W, a->k = k, a->s = s, a->p = p;
  a->Ho = (H + 2 * p - k) / s + 1, a->Wo = (W + 2 * p - k) / s + 1;
  double g[SSIM_MAX_WIN], tot = 0.0;
  for (int i = 0; i < k; ++i) {
    g[i] = exp(-(double)((i - k / 2) * (i - k / 2)) / (2.0 * 1.5 * 1.5));
    tot += g[i];
  }
  for (int i = 0; i < SSIM_MAX_WIN; ++i) a->g[i] = i < k ? (float)(g[i] / tot) : 0.f;
  return 0;
}

static inline dim3 loss_grid(int64_t n) {
  int64_t b = nsim_blocks(n, LOSS_BLOCK);
  return dim3((unsigned)(b > LOSS_MAX_BLOCKS ? LOSS_MAX_BLOCKS : b));
}

extern "C" {

// out[0] must be zero on entry (the caller's memset is part of the op); out[0] += mean((|nab_i| - 1)^2)
int nsim_eikonal_loss_fwd(const float* nablas, int64_t S, float* out, void* stream) {
  if (S < 0) return 2;
  if (!out) return 4;
  if (S == 0) return 0;
  hipLaunchKernelGGL(k_eikonal_fwd, loss_grid(S), dim3(LOSS_BLOCK), 0, (hipStream_t)stream, nablas, S,
                     1.0f / (float)S, out);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_eikonal_loss_bwd(const float* nablas, int64_t S, const float* gout, float* dnablas, void* stream) {
  if (S < 0) return 2;
  if (S == 0) return 0;
  if (!dnablas || !gout) return 26;
  hipLaunchKernelGGL(k_eikonal_bwd, dim3(nsim_blocks(S, LOSS_BLOCK)), dim3(LOSS_BLOCK), 0, (hipStream_t)stream, nablas,
                     S, 1.0f / (float)S, gout, dnablas);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_mse_loss_fwd(const float* pred, const float* gt, int64_t n, float* out, void* stream) {
  if (n < 0) return 2;
  if (!out) return 4;
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_mse_fwd, loss_grid(n), dim3(LOSS_BLOCK), 0, (hipStream_t)stream, pred, gt, n, 1.0f / (float)n,
                     out);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_mse_loss_bwd(const float* pred, const float* gt, int64_t n, const float* gout, float* dpred, void* stream) {
  if (n < 0) return 2;
  if (n == 0) return 0;
  if (!dpred || !gout) return 26;
  hipLaunchKernelGGL(k_mse_bwd, dim3(nsim_blocks(n, LOSS_BLOCK)), dim3(LOSS_BLOCK), 0, (hipStream_t)stream, pred, gt, n,
                     1.0f / (float)n, gout, dpred);
  NSIM_CHECK_LAUNCH();
  return 0;
}

static inline dim3 curv_grid(int64_t n) {
  return dim3(nsim_blocks(n, LOSS_BLOCK, CURV_MAX_BLOCKS));
}

// x_out [n,3] = clamp(x + eps (nablas^ x dirs^), aabb_lo, aabb_hi); aabb_lo / aabb_hi: 3 device floats each
int nsim_curv_shift(const float* nablas, const float* x, const float* dirs, const float* aabb_lo, const float* aabb_hi,
                    float eps, int64_t n, float* x_out, void* stream) {
  if (n < 0) return 2;
  if (n == 0) return 0;
  if (!nablas || !x || !dirs || !aabb_lo || !aabb_hi || !x_out) return 4;
  hipLaunchKernelGGL(k_curv_shift, curv_grid(n), dim3(LOSS_BLOCK), 0, (hipStream_t)stream, nablas, x, dirs, aabb_lo, aabb_hi,
                     eps, n, x_out);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_curv_angle_fwd(const float* n0, const float* n1, int64_t n, float* curv, void* stream) {
  if (n < 0) return 2;
  if (n == 0) return 0;
  if (!n0 || !n1 || !curv) return 4;
  hipLaunchKernelGGL(k_curv_angle_fwd, curv_grid(n), dim3(LOSS_BLOCK), 0, (hipStream_t)stream, n0, n1, n, curv);
  NSIM_CHECK_LAUNCH();
  return 0;
}

// dn0 / dn1 [n,3]: either may be NULL (gradient not wanted)
int nsim_curv_angle_bwd(const float* n0, const float* n1, const float* gcurv, int64_t n, float* dn0, float* dn1,
                        void* stream) {
  if (n < 0) return 2;
  if (n == 0 || (!dn0 && !dn1)) return 0;
  if (!n0 || !n1 || !gcurv) return 26;
  hipLaunchKernelGGL(k_curv_angle_bwd, curv_grid(n), dim3(LOSS_BLOCK), 0, (hipStream_t)stream, n0, n1, gcurv, n, dn0, dn1);
  NSIM_CHECK_LAUNCH();
  return 0;
}

// out[0] must be zero on entry; out[0] += mean(min(curvature_i, clamp_max))
int nsim_curv_loss_fwd(const float* n0, const float* n1, int64_t n, float clamp_max, float* out, void* stream) {
  if (n < 0) return 2;
  if (!out) return 4;
  if (n == 0) return 0;
  if (!n0 || !n1) return 4;
  hipLaunchKernelGGL(k_curv_loss_fwd, loss_grid(n), dim3(LOSS_BLOCK), 0, (hipStream_t)stream, n0, n1, n, 1.0f / (float)n,
                     clamp_max, out);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_curv_loss_bwd(const float* n0, const float* n1, int64_t n, float clamp_max, const float* gout, float* dn0,
                       float* dn1, void* stream) {
  if (n < 0) return 2;
  if (n == 0 || (!dn0 && !dn1)) return 0;
  if (!n0 || !n1 || !gout) return 26;
  hipLaunchKernelGGL(k_curv_loss_bwd, curv_grid(n), dim3(LOSS_BLOCK), 0, (hipStream_t)stream, n0, n1, n, 1.0f / (float)n,
                     clamp_max, gout, dn0, dn1);
  NSIM_CHECK_LAUNCH();
  return 0;
}

// out[0] must be zero on entry; out[0] += mean SSIM over the BC CH Ho Wo windows.  index NULL: planar [BC, H, W]; else the [3, H, W]
// image gathered from rows index[i W + j] of x, y [n_rows, 3] (BC = 1).  coef [3, BC CH Ho Wo]: handed to nsim_ssim_bwd
int nsim_ssim_fwd(const float* x, const float* y, const int64_t* index, int64_t n_rows, int64_t BC, int H, int W, int k, int s,
                  float* out, float* coef, void* stream) {
  SsimArgs a;
  const int rc = ssim_args(&a, x, y, index, n_rows, BC, H, W, k, s);
  if (rc) return rc;
  if (!x || !y || !out || !coef) return 4;
  const int64_t sites = BC * a.Ho * a.Wo;
  if (index)
    hipLaunchKernelGGL((k_ssim_fwd<3>), loss_grid(sites), dim3(LOSS_BLOCK), 0, (hipStream_t)stream, a,
                       1.0f / (float)(3 * sites), out, coef);
  else
    hipLaunchKernelGGL((k_ssim_fwd<1>), loss_grid(sites), dim3(LOSS_BLOCK), 0, (hipStream_t)stream, a, 1.0f / (float)sites,
                       out, coef);
  NSIM_CHECK_LAUNCH();
  return 0;
}

// dx = gout[0] d (mean SSIM) / d x: planar [BC, H, W], every element written; indexed [n_rows, 3], ADDED to (the caller's zero
// fill is part of the op: rows no index names stay zero)
int nsim_ssim_bwd(const float* x, const float* y, const int64_t* index, int64_t n_rows, int64_t BC, int H, int W, int k, int s,
                  const float* coef, const float* gout, float* dx, void* stream) {
  SsimArgs a;
  const int rc = ssim_args(&a, x, y, index, n_rows, BC, H, W, k, s);
  if (rc) return rc;
  if (!dx || !gout) return 26;
  if (!x || !y || !coef) return 4;
  const int64_t sites = BC * a.Ho * a.Wo, npix = BC * H * W;
  if (index)
    hipLaunchKernelGGL((k_ssim_bwd<3>), curv_grid(npix), dim3(LOSS_BLOCK), 0, (hipStream_t)stream, a,
                       1.0f / (float)(3 * sites), coef, gout, dx);
  else
    hipLaunchKernelGGL((k_ssim_bwd<1>), curv_grid(npix), dim3(LOSS_BLOCK), 0, (hipStream_t)stream, a, 1.0f / (float)sites, coef,
                       gout, dx);
  NSIM_CHECK_LAUNCH();
  return 0;
}

// acc [3] must be zero on entry.  n_img = number of image VALUES (rays * 3); nablas [S + M, 3]
int nsim_train_loss_head(const float* pred, const float* gt, int64_t n_img, const float* nablas, int64_t S, int64_t M,
                         float w_eikonal, float* acc, float* d_pred, float* d_nablas, void* stream) {
  if (n_img <= 0 || S < 0 || M < 0) return 2;
  if (!pred || !gt || !acc || !d_pred || (S + M > 0 && (!nablas || !d_nablas))) return 4;
  const int64_t top = n_img > S + M ? n_img : S + M;
  int64_t b = nsim_blocks(top, LOSS_BLOCK);
  if (b > LOSS_MAX_BLOCKS) b = LOSS_MAX_BLOCKS;     // three single-address atomics per block: they serialise at L2
  hipLaunchKernelGGL(k_loss_head, dim3((unsigned)b), dim3(LOSS_BLOCK), 0, (hipStream_t)stream, pred, gt, n_img, nablas, S,
                     M, w_eikonal, acc, d_pred, d_nablas);
  NSIM_CHECK_LAUNCH();
  return 0;
}

// out [rows, C] must be initialised by the caller (zeros for a plain gradient)
int nsim_rows_scatter_add(const float* g, const int64_t* idx, int64_t n, int C, int64_t rows, float* out, void* stream) {
  if (n < 0 || rows < 0) return 2;
  if (C <= 0) return 3;
  if (n == 0) return 0;
  if (!out) return 4;
  hipLaunchKernelGGL(k_rows_scatter_add, loss_grid(n * C), dim3(LOSS_BLOCK), 0, (hipStream_t)stream, g, idx, n, C, rows,
                     out);
  NSIM_CHECK_LAUNCH();
  return 0;
}

// out[i, :] = table[idx[i], :] for i < n, zeros for n <= i < n + tail (the forward of ``embed[fidx]`` with the zero rows of
// the step's appended free points in the same launch)
__global__ void __launch_bounds__(LOSS_BLOCK) k_rows_gather(const float* __restrict__ table, const int64_t* __restrict__ idx,
                                                            int64_t n, int C, int64_t rows, int64_t tail, float* __restrict__ out) {
  const int64_t tot = (n + tail) * C;
  for (int64_t i = (int64_t)blockIdx.x * LOSS_BLOCK + threadIdx.x; i < tot; i += (int64_t)gridDim.x * LOSS_BLOCK) {
    const int64_t r = i / C;
    float v = 0.f;
    if (r < n) {
      const int64_t k = idx[r];
      if (k >= 0 && k < rows) v = table[k * C + (i % C)];
    }
    out[i] = v;
  }
}

int nsim_rows_gather(const float* table, const int64_t* idx, int64_t n, int C, int64_t rows, int64_t tail, float* out,
                     void* stream) {
  if (n < 0 || tail < 0 || C <= 0) return 2;
  if (n + tail == 0) return 0;
  if (!out || (n > 0 && (!table || !idx))) return 4;
  hipLaunchKernelGGL(k_rows_gather, loss_grid((n + tail) * C), dim3(LOSS_BLOCK), 0, (hipStream_t)stream, table, idx, n, C, rows,
                     tail, out);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_sphere_image(const float* rays_o, const float* rays_d, int64_t N, float radius, float* rgb, void* stream) {
  if (N < 0) return 2;
  if (N == 0) return 0;
  if (!rgb || !(radius > 0.f)) return 4;
  hipLaunchKernelGGL(k_sphere_image, dim3(nsim_blocks(N, LOSS_BLOCK)), dim3(LOSS_BLOCK), 0, (hipStream_t)stream, rays_o,
                     rays_d, N, radius, rgb);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_gather_rays(const float* rays_o, const float* rays_d, const float* near, const float* far, const int64_t* idx,
                     int64_t R, float* o_out, float* d_out, float* near_out, float* far_out, void* stream) {
  if (R < 0) return 2;
  if (R == 0) return 0;
  if (!o_out || !d_out || !near_out || !far_out) return 4;
  hipLaunchKernelGGL(k_gather_rays, dim3(nsim_blocks(R, LOSS_BLOCK)), dim3(LOSS_BLOCK), 0, (hipStream_t)stream, rays_o,
                     rays_d, near, far, idx, R, o_out, d_out, near_out, far_out);
  NSIM_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
