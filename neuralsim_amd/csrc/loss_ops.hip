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
//   * the street configs' supervision: occupancy-mask BCE, mask entropy, sparsity, clearance, the lidar depth + line-of-sight loss
//     with its median outlier gate (an exact order statistic by radix select)   (app/loss/{mask, mask_entropy, sparsity, clearance,
//     lidar}.py)
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

// elementwise kernels without a reduction: 8 blocks per CU, the rest by grid stride
static inline dim3 elem_grid(int64_t n) {
  return dim3(nsim_blocks(n, LOSS_BLOCK, CURV_MAX_BLOCKS));
}

// ---------------------------------------------------------------------------------------------- street supervision losses
// The loss blocks of the street configs beside rgb and eikonal (withmask_withlidar_joint.240219.yaml:438-500): occupancy-mask BCE,
// mask entropy, sparsity, clearance and the lidar loss with its median outlier gate.  Every forward launch also writes the
// UNSCALED gradient (as k_loss_head: none of them needs the loss value), so a backward is one scale by gout -- except the mask
// entropy, whose two sums have upstream gradients of their own: its backward re-evaluates the term table.

// several partial sums of one block into out[0..K): one atomic per non-zero sum and block
template <int K>
__device__ __forceinline__ void block_sums_atomic(const float (&v)[K], float* out) {
  __shared__ float red[K][LOSS_BLOCK / 64];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float s = wave_sum(v[k]);
    if (nsim_lane() == 0) red[k][threadIdx.x >> 6] = s;
  }
  __syncthreads();
  if (threadIdx.x < K) {
    float tot = 0.f;
    for (int w = 0; w < LOSS_BLOCK / 64; ++w) tot += red[threadIdx.x][w];
    if (tot != 0.f) atomicAdd(out + threadIdx.x, tot);
  }
}

// d[i] = gout[0] g[i]: the backward of every loss whose forward left its unscaled gradient
__global__ void __launch_bounds__(LOSS_BLOCK) k_loss_scale(const float* __restrict__ g, int64_t n, const float* __restrict__ gout,
                                                           float* __restrict__ d) {
  const float s = gout[0];
  for (int64_t i = (int64_t)blockIdx.x * LOSS_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * LOSS_BLOCK) d[i] = s * g[i];
}

// mode 0: gt as given; 1 always_occupied: gt = 1; 2 only_cull_non_occupied: rays with gt < 0.5 against 0; 3 only_preserve_occupied:
// rays with gt > 0.5 against 1.  The unselected rays of modes 2, 3 add nothing, get no gradient and err 0; the divisor stays N.
__global__ void __launch_bounds__(LOSS_BLOCK) k_mask_bce(const float* __restrict__ pred, const float* __restrict__ gt, int64_t N,
                                                         float lo, float hi, int mode, float scale, float* __restrict__ out,
                                                         float* __restrict__ err, float* __restrict__ grad) {
  float acc = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * LOSS_BLOCK + threadIdx.x; i < N; i += (int64_t)gridDim.x * LOSS_BLOCK) {
    const float x = pred[i];
    float y = mode == 1 ? 1.0f : gt[i];
    bool sel = true;
    if (mode == 2) sel = y < 0.5f, y = 0.f;
    if (mode == 3) sel = y > 0.5f, y = 1.0f;
    float e = 0.f, g = 0.f;
    if (sel) {
      const float p = fminf(fmaxf(x, lo), hi);
      // F.binary_cross_entropy: both logs floored at -100; its backward (p - y) / max(p (1 - p), 1e-12)
      acc += -(y * fmaxf(logf(p), -100.0f) + (1.0f - y) * fmaxf(logf(1.0f - p), -100.0f));
      if (x >= lo && x <= hi) g = scale * (p - y) / fmaxf((1.0f - p) * p, 1e-12f);
      e = fabsf(x - y);
    }
    err[i] = e;
    grad[i] = g;
  }
  block_sum_atomic(acc, scale, out);
}

// One term of a mask-entropy mode: coef * A * log(max(B, eps)) with A, B each one of the three masks m or its complement 1 - m,
// summed into out[term.out]; a detached factor is a constant of the backward.
#define ENT_MAX_TERMS 4
struct EntropyTerm {
  int32_t a_src, a_neg, a_detach, b_src, b_neg, b_detach, out;
  float coef;
};
struct EntropyTable {
  int32_t n_terms;
  EntropyTerm t[ENT_MAX_TERMS];
};

__device__ __forceinline__ float ent_pick(float v0, float v1, float v2, int src, int neg) {
  const float v = src == 0 ? v0 : (src == 1 ? v1 : v2);
  return neg ? 1.0f - v : v;
}

__global__ void __launch_bounds__(LOSS_BLOCK) k_mask_entropy_fwd(EntropyTable tab, const float* __restrict__ m0,
                                                                 const float* __restrict__ m1, const float* __restrict__ m2,
                                                                 int64_t N, float eps, float inv_n, float* __restrict__ out) {
  float acc[2] = {0.f, 0.f};
  for (int64_t i = (int64_t)blockIdx.x * LOSS_BLOCK + threadIdx.x; i < N; i += (int64_t)gridDim.x * LOSS_BLOCK) {
    const float v0 = m0 ? m0[i] : 0.f, v1 = m1 ? m1[i] : 0.f, v2 = m2 ? m2[i] : 0.f;
    for (int k = 0; k < tab.n_terms; ++k) {
      const EntropyTerm& t = tab.t[k];
      const float a = ent_pick(v0, v1, v2, t.a_src, t.a_neg), b = ent_pick(v0, v1, v2, t.b_src, t.b_neg);
      const float term = t.coef * inv_n * (a * logf(fmaxf(b, eps)));
      if (t.out) acc[1] += term;
      else acc[0] += term;
    }
  }
  block_sums_atomic<2>(acc, out);
}

// d0 / d1 / d2 [N] (NULL: not wanted) = gout_k d out[k] / d mask; clamp_min passes the gradient where its argument >= eps
__global__ void __launch_bounds__(LOSS_BLOCK) k_mask_entropy_bwd(EntropyTable tab, const float* __restrict__ m0,
                                                                 const float* __restrict__ m1, const float* __restrict__ m2,
                                                                 int64_t N, float eps, float inv_n, const float* __restrict__ gout0,
                                                                 const float* __restrict__ gout1, float* __restrict__ d0,
                                                                 float* __restrict__ d1, float* __restrict__ d2) {
  const float go0 = gout0 ? gout0[0] * inv_n : 0.f, go1 = gout1 ? gout1[0] * inv_n : 0.f;
  for (int64_t i = (int64_t)blockIdx.x * LOSS_BLOCK + threadIdx.x; i < N; i += (int64_t)gridDim.x * LOSS_BLOCK) {
    const float v0 = m0 ? m0[i] : 0.f, v1 = m1 ? m1[i] : 0.f, v2 = m2 ? m2[i] : 0.f;
    float e0 = 0.f, e1 = 0.f, e2 = 0.f;
    for (int k = 0; k < tab.n_terms; ++k) {
      const EntropyTerm& t = tab.t[k];
      const float a = ent_pick(v0, v1, v2, t.a_src, t.a_neg), b = ent_pick(v0, v1, v2, t.b_src, t.b_neg);
      const float c = (t.out ? go1 : go0) * t.coef;
      if (!t.a_detach) {
        const float g = (t.a_neg ? -c : c) * logf(fmaxf(b, eps));
        e0 += t.a_src == 0 ? g : 0.f, e1 += t.a_src == 1 ? g : 0.f, e2 += t.a_src == 2 ? g : 0.f;
      }
      if (!t.b_detach && b >= eps) {
        const float g = (t.b_neg ? -c : c) * a / b;
        e0 += t.b_src == 0 ? g : 0.f, e1 += t.b_src == 1 ? g : 0.f, e2 += t.b_src == 2 ? g : 0.f;
      }
    }
    if (d0) d0[i] = e0;
    if (d1) d1[i] = e1;
    if (d2) d2[i] = e2;
  }
}

// type 0 normalized_logistic_density 4 s(1 - s), s = sigmoid(param x); 1 normal exp(-x^param); 2 density_reg |1 - exp(-param x)|
__global__ void __launch_bounds__(LOSS_BLOCK) k_sparsity(const float* __restrict__ x, int64_t M, int type, float param, float scale,
                                                         float* __restrict__ out, float* __restrict__ grad) {
  float acc = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * LOSS_BLOCK + threadIdx.x; i < M; i += (int64_t)gridDim.x * LOSS_BLOCK) {
    const float v = x[i];
    float f, g;
    if (type == 0) {
      const float s = 1.0f / (1.0f + expf(-param * v));
      f = 4.0f * s * (1.0f - s);
      g = param * f * (1.0f - 2.0f * s);
    } else if (type == 1) {
      f = expf(-powf(v, param));
      g = param == 0.f ? 0.f : -param * powf(v, param - 1.0f) * f;      // torch.pow's backward: 0 for a zero exponent
    } else {
      const float e = expf(-param * v), r = 1.0f - e;
      f = fabsf(r);
      g = r > 0.f ? param * e : (r < 0.f ? -param * e : 0.f);          // abs: sub-gradient 0 at 0
    }
    acc += f;
    grad[i] = scale * g;
  }
  block_sum_atomic(acc, scale, out);
}

// sum over near_sdf < thresh of exp(-beta (near_sdf - thresh)) / M: no point below the threshold adds nothing to the caller's zero
__global__ void __launch_bounds__(LOSS_BLOCK) k_clearance(const float* __restrict__ x, int64_t M, float beta, float thresh,
                                                          float scale, float* __restrict__ out, float* __restrict__ grad) {
  float acc = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * LOSS_BLOCK + threadIdx.x; i < M; i += (int64_t)gridDim.x * LOSS_BLOCK) {
    const float v = x[i];
    float g = 0.f;
    if (v < thresh) {
      const float e = expf(-beta * (v - thresh));
      acc += e;
      g = -beta * scale * e;
    }
    grad[i] = g;
  }
  block_sum_atomic(acc, scale, out);
}

// The k-th smallest of x [N] (0-based), exactly: a radix select over the bit pattern, which orders non-negative floats as their
// values.  ONE workgroup, four passes of eight bits from the top: an LDS histogram of the digit among the elements that share the
// digits fixed so far, then thread 0 walks its 256 bins to the one that holds rank k.  Every loop is bounded by N or 256.
__global__ void __launch_bounds__(LOSS_BLOCK) k_kth_value(const float* __restrict__ x, int64_t N, int64_t k, float* __restrict__ out) {
  __shared__ unsigned hist[256];
  __shared__ unsigned s_prefix, s_k;
  if (threadIdx.x == 0) s_prefix = 0u, s_k = (unsigned)k;
  for (int shift = 24; shift >= 0; shift -= 8) {
    hist[threadIdx.x] = 0u;                       // LOSS_BLOCK == 256 bins
    __syncthreads();
    const unsigned prefix = s_prefix;
    const unsigned fixed = shift == 24 ? 0u : (0xffffffffu << (shift + 8));
    for (int64_t i = threadIdx.x; i < N; i += LOSS_BLOCK) {
      unsigned b;
      const float v = x[i];
      __builtin_memcpy(&b, &v, 4);
      if ((b & fixed) == prefix) atomicAdd(&hist[(b >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned left = s_k, bin = 255u;
      for (unsigned j = 0; j < 256u; ++j) {
        if (left < hist[j]) {
          bin = j;
          break;
        }
        left -= hist[j];
      }
      s_k = left;
      s_prefix = prefix | (bin << shift);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const unsigned b = s_prefix;
    float v;
    __builtin_memcpy(&v, &b, 4);
    out[0] = v;
  }
}

// per beam: is it a return the rendering saw, and its absolute depth error (0 for the others) -- the input of the median
__global__ void __launch_bounds__(LOSS_BLOCK) k_lidar_valid(const float* __restrict__ depth, const float* __restrict__ mask,
                                                            const float* __restrict__ ranges, int64_t N, float mask_thresh,
                                                            float toofar, int replaces, uint8_t* __restrict__ valid,
                                                            float* __restrict__ err) {
  for (int64_t i = (int64_t)blockIdx.x * LOSS_BLOCK + threadIdx.x; i < N; i += (int64_t)gridDim.x * LOSS_BLOCK) {
    const float r = ranges[i];
    bool v = mask[i] > mask_thresh && r > 0.f;
    if (toofar > 0.f) v = replaces ? r <= toofar : (v && r <= toofar);
    valid[i] = v ? 1 : 0;
    err[i] = fabsf(depth[i] - r) * (v ? 1.0f : 0.f);
  }
}

struct LidarArgs {
  const float* depth;          // [N]
  const float* ranges;         // [N]
  const uint8_t* valid;        // [N]
  const float* err;            // [N]
  const float* median;         // [1], read when factor > 0
  int64_t N;
  float factor;                // discard_outliers_median
  int depth_fn;                // -1 none, 0 l1, 1 l1_log, 2 l2, 3 l2_relative, 4 l2_normalized, 5 huber
  float depth_param;           // far (4), alpha (5)
  float w_depth;
  int los_fn;                  // 0 none, 1 nerf / neus_urban, 2 neus_unisim
  float bound;                 // sigma (1), epsilon (2)
  float std;                   // sigma / sigma_scale_factor (1)
  float w_los;
  const float* t;              // [S]
  const float* vw;             // [S]
  const int64_t* rays_inds;    // [R]
  const int64_t* pack_infos;   // [R, 2]
  int64_t R, S;
  float* acc;                  // [3]: depth, los.neighbor, los.empty (weighted)
  uint8_t* keep;               // [N]: the final mask
  float* g_depth;              // [N]
  float* g_vw;                 // [S]
  uint8_t* member;             // [S]: 0 no term, 1 neighbor, 2 empty
};

__device__ __forceinline__ bool lidar_keep(const LidarArgs& a, int64_t i, float thr) {
  return a.valid[i] && !(a.factor > 0.f && a.err[i] > thr);
}

// Blocks [0, depth_blocks) walk the beams, the others the packs of the line-of-sight buffer, one wave per pack.  Both halves form
// the final mask of a beam from (valid, err, median) themselves, so neither waits for the other.
__global__ void __launch_bounds__(LOSS_BLOCK) k_lidar_loss(LidarArgs a, int depth_blocks) {
  const float thr = a.factor > 0.f ? a.median[0] * a.factor : 0.f;        // the product in f32, as the reference forms it
  float acc[3] = {0.f, 0.f, 0.f};
  if ((int)blockIdx.x < depth_blocks) {
    const float sc = a.w_depth / (float)a.N;
    for (int64_t i = (int64_t)blockIdx.x * LOSS_BLOCK + threadIdx.x; i < a.N; i += (int64_t)depth_blocks * LOSS_BLOCK) {
      const bool m = lidar_keep(a, i, thr);
      a.keep[i] = m ? 1 : 0;
      if (a.depth_fn < 0) continue;
      const float mf = m ? 1.0f : 0.f, p = a.depth[i], g = a.ranges[i];
      float f, df;
      switch (a.depth_fn) {
        case 0: {
          const float d = p - g;
          f = fabsf(d), df = d > 0.f ? 1.0f : (d < 0.f ? -1.0f : 0.f);
        } break;
        case 1: {
          // log(p + 1) - log(g + 1) as log1p((p - g) / (g + 1)): the difference is taken between the INPUTS -- two logs of ~3
          // that differ by ~1e-2 lose 1e-5 of the term in f32 (p, g >= 0: the same real number)
          const float d = log1pf((p - g) / (g + 1.0f));
          f = fabsf(d), df = (d > 0.f ? 1.0f : (d < 0.f ? -1.0f : 0.f)) / (p + 1.0f);
        } break;
        case 2: {
          const float d = p - g;
          f = d * d, df = 2.0f * d;
        } break;
        case 3: {
          const float d = p - g, q = g * g + 1e-2f;
          f = d * d / q, df = 2.0f * d / q;
        } break;
        case 4: {
          const float d = (p - g) / a.depth_param;        // p / far - g / far, the difference taken between the inputs
          f = d * d, df = 2.0f * d / a.depth_param;
        } break;
        default: {
          const float d = p - g, ad = fabsf(d), al = a.depth_param;
          f = ad < al ? 0.5f * d * d : al * (ad - 0.5f * al);
          df = ad < al ? d : (d > 0.f ? al : -al);
        } break;
      }
      acc[0] += f * mf;
      a.g_depth[i] = sc * df * mf;
    }
    acc[0] *= sc;
  } else if (a.los_fn != 0) {
    const float sc = a.w_los / (float)a.R;
    const int lane = nsim_lane();
    const int64_t wave = (int64_t)((int)blockIdx.x - depth_blocks) * (LOSS_BLOCK / 64) + (threadIdx.x >> 6);
    const int64_t n_waves = (int64_t)((int)gridDim.x - depth_blocks) * (LOSS_BLOCK / 64);
    const float inv_norm = 1.0f / (a.std * 2.5066282746310002f);           // 1 / (std sqrt(2 pi))
    for (int64_t r = wave; r < a.R; r += n_waves) {
      const int64_t ray = a.rays_inds[r], begin = a.pack_infos[2 * r], cnt = a.pack_infos[2 * r + 1];
      const bool in = ray >= 0 && ray < a.N;
      const float g = in ? a.ranges[ray] : 0.f;
      const float mf = (in && lidar_keep(a, ray, thr)) ? 1.0f : 0.f;
      for (int64_t j = begin + lane; j < begin + cnt; j += 64) {
        if (j < 0 || j >= a.S) continue;
        const float t = a.t[j], w = a.vw[j];
        uint8_t mem = 0;
        float gv = 0.f;
        if (a.los_fn == 1) {
          if (t <= g + a.bound && t >= g - a.bound) {
            const float z = (t - g) / a.std, d = w - inv_norm * expf(-0.5f * z * z);
            mem = 1, acc[1] += d * d * mf, gv = 2.0f * d;
          } else if (t < g - a.bound) {
            mem = 2, acc[2] += w * w * mf, gv = 2.0f * w;
          }
        } else if (fabsf(t - g) > a.bound) {
          mem = 2, acc[2] += w * w * mf, gv = 2.0f * w;
        }
        a.member[j] = mem;
        a.g_vw[j] = sc * gv * mf;
      }
    }
    acc[1] *= sc;
    acc[2] *= sc;
  }
  block_sums_atomic<3>(acc, a.acc);
}

// d_depth = gout[0] g_depth; d_vw = gout[member] g_vw (a NULL gout: that term is not part of the graph)
__global__ void __launch_bounds__(LOSS_BLOCK) k_lidar_loss_bwd(const float* __restrict__ g_depth, int64_t N,
                                                               const float* __restrict__ g_vw, const uint8_t* __restrict__ member,
                                                               int64_t S, const float* __restrict__ go_depth,
                                                               const float* __restrict__ go_nb, const float* __restrict__ go_em,
                                                               float* __restrict__ d_depth, float* __restrict__ d_vw) {
  const float s0 = go_depth ? go_depth[0] : 0.f, s1 = go_nb ? go_nb[0] : 0.f, s2 = go_em ? go_em[0] : 0.f;
  const int64_t top = N > S ? N : S;
  for (int64_t i = (int64_t)blockIdx.x * LOSS_BLOCK + threadIdx.x; i < top; i += (int64_t)gridDim.x * LOSS_BLOCK) {
    if (d_depth && i < N) d_depth[i] = s0 * g_depth[i];
    if (d_vw && i < S) {
      const uint8_t m = member[i];
      d_vw[i] = m == 1 ? s1 * g_vw[i] : (m == 2 ? s2 * g_vw[i] : 0.f);
    }
  }
}

extern "C" {

// d [n] = gout[0] g [n]
int nsim_loss_scale_bwd(const float* g, int64_t n, const float* gout, float* d, void* stream) {
  if (n < 0) return 2;
  if (n == 0) return 0;
  if (!g || !gout || !d) return 26;
  hipLaunchKernelGGL(k_loss_scale, elem_grid(n), dim3(LOSS_BLOCK), 0, (hipStream_t)stream, g, n, gout, d);
  NSIM_CHECK_LAUNCH();
  return 0;
}

// out[0] must be zero on entry; out[0] += w / N sum of the selected rays' BCE; err [N], grad [N] = w d mean / d pred are written
int nsim_mask_bce_fwd(const float* pred, const float* gt, int64_t N, float lo, float hi, int mode, float w, float* out, float* err,
                      float* grad, void* stream) {
  if (N < 0) return 2;
  if (mode < 0 || mode > 3 || !(lo <= hi)) return 58;
  if (!out) return 4;
  if (N == 0) return 0;
  if (!pred || (!gt && mode != 1) || !err || !grad) return 4;
  hipLaunchKernelGGL(k_mask_bce, loss_grid(N), dim3(LOSS_BLOCK), 0, (hipStream_t)stream, pred, gt, N, lo, hi, mode, w / (float)N,
                     out, err, grad);
  NSIM_CHECK_LAUNCH();
  return 0;
}

static inline int entropy_table(EntropyTable* t, const NsimEntropyTable* tab, const float* const* m) {
  if (!tab || tab->n_terms < 0 || tab->n_terms > ENT_MAX_TERMS) return 58;
  t->n_terms = tab->n_terms;
  for (int k = 0; k < tab->n_terms; ++k) {
    const NsimEntropyTerm& s = tab->t[k];
    if (s.a_src < 0 || s.a_src > 2 || s.b_src < 0 || s.b_src > 2 || s.out < 0 || s.out > 1) return 58;
    if (!m[s.a_src] || !m[s.b_src]) return 4;
    EntropyTerm& d = t->t[k];
    d.a_src = s.a_src, d.a_neg = s.a_neg, d.a_detach = s.a_detach, d.b_src = s.b_src, d.b_neg = s.b_neg, d.b_detach = s.b_detach;
    d.out = s.out, d.coef = s.coef;
  }
  return 0;
}

// out [2] must be zero on entry; masks a table term does not name may be NULL
int nsim_mask_entropy_fwd(const NsimEntropyTable* tab, const float* mask_pred, const float* mask_cr, const float* mask_dv,
                          int64_t N, float eps, float* out, void* stream) {
  if (N < 0) return 2;
  const float* m[3] = {mask_pred, mask_cr, mask_dv};
  EntropyTable t;
  const int rc = entropy_table(&t, tab, m);
  if (rc) return rc;
  if (!out) return 4;
  if (N == 0 || t.n_terms == 0) return 0;
  hipLaunchKernelGGL(k_mask_entropy_fwd, loss_grid(N), dim3(LOSS_BLOCK), 0, (hipStream_t)stream, t, m[0], m[1], m[2], N, eps,
                     1.0f / (float)N, out);
  NSIM_CHECK_LAUNCH();
  return 0;
}

// gout0 / gout1 [1]: the upstream gradients of out[0] / out[1] (NULL: zero); d_pred / d_cr / d_dv [N]: any may be NULL
int nsim_mask_entropy_bwd(const NsimEntropyTable* tab, const float* mask_pred, const float* mask_cr, const float* mask_dv,
                          int64_t N, float eps, const float* gout0, const float* gout1, float* d_pred, float* d_cr, float* d_dv,
                          void* stream) {
  if (N < 0) return 2;
  const float* m[3] = {mask_pred, mask_cr, mask_dv};
  EntropyTable t;
  const int rc = entropy_table(&t, tab, m);
  if (rc) return rc;
  if (N == 0 || (!d_pred && !d_cr && !d_dv)) return 0;
  hipLaunchKernelGGL(k_mask_entropy_bwd, elem_grid(N), dim3(LOSS_BLOCK), 0, (hipStream_t)stream, t, m[0], m[1], m[2], N, eps,
                     1.0f / (float)N, gout0, gout1, d_pred, d_cr, d_dv);
  NSIM_CHECK_LAUNCH();
  return 0;
}

// out[0] must be zero on entry; out[0] += w mean(f(x)); grad [M] = w d mean / d x
int nsim_sparsity_fwd(const float* x, int64_t M, int type, float param, float w, float* out, float* grad, void* stream) {
  if (M < 0) return 2;
  if (type < 0 || type > 2) return 58;
  if (!out) return 4;
  if (M == 0) return 0;
  if (!x || !grad) return 4;
  hipLaunchKernelGGL(k_sparsity, loss_grid(M), dim3(LOSS_BLOCK), 0, (hipStream_t)stream, x, M, type, param, w / (float)M, out,
                     grad);
  NSIM_CHECK_LAUNCH();
  return 0;
}

// out[0] must be zero on entry; out[0] += w / M sum over near_sdf < thresh of exp(-beta (near_sdf - thresh)); grad [M] written
int nsim_clearance_fwd(const float* near_sdf, int64_t M, float beta, float thresh, float w, float* out, float* grad, void* stream) {
  if (M < 0) return 2;
  if (!out) return 4;
  if (M == 0) return 0;
  if (!near_sdf || !grad) return 4;
  hipLaunchKernelGGL(k_clearance, loss_grid(M), dim3(LOSS_BLOCK), 0, (hipStream_t)stream, near_sdf, M, beta, thresh,
                     w / (float)M, out, grad);
  NSIM_CHECK_LAUNCH();
  return 0;
}

// out[0] = sort(x)[k] for finite non-negative x [N], 0 <= k < N < 2^32; one workgroup, the value stays on the device
int nsim_kth_value_f32(const float* x, int64_t N, int64_t k, float* out, void* stream) {
  if (N < 0) return 2;
  if (N == 0 || k < 0 || k >= N || N >= ((int64_t)1 << 32)) return 58;
  if (!x || !out) return 4;
  hipLaunchKernelGGL(k_kth_value, dim3(1), dim3(LOSS_BLOCK), 0, (hipStream_t)stream, x, N, k, out);
  NSIM_CHECK_LAUNCH();
  return 0;
}

// valid [N] uint8, err [N] = |depth_pred - ranges| valid.  discard_toofar <= 0: no range gate
int nsim_lidar_valid(const float* depth_pred, const float* mask_pred, const float* ranges, int64_t N, float mask_pred_thresh,
                     float discard_toofar, int toofar_replaces_mask, uint8_t* valid, float* err, void* stream) {
  if (N < 0) return 2;
  if (N == 0) return 0;
  if (!depth_pred || !mask_pred || !ranges || !valid || !err) return 4;
  hipLaunchKernelGGL(k_lidar_valid, loss_grid(N), dim3(LOSS_BLOCK), 0, (hipStream_t)stream, depth_pred, mask_pred, ranges, N,
                     mask_pred_thresh, discard_toofar, toofar_replaces_mask, valid, err);
  NSIM_CHECK_LAUNCH();
  return 0;
}

// acc [3] must be zero on entry.  The packs of pack_infos_hit tile [0, S): every element of g_vw / member is written.
int nsim_lidar_loss_fwd(const NsimLidarLoss* cfg, const float* depth_pred, const float* ranges, const uint8_t* valid,
                        const float* err, const float* median, int64_t N, const float* t, const float* vw,
                        const int64_t* rays_inds_hit, const int64_t* pack_infos_hit, int64_t R, int64_t S, float* acc,
                        uint8_t* keep, float* g_depth, float* g_vw, uint8_t* member, void* stream) {
  if (N < 0 || R < 0 || S < 0) return 2;
  if (!cfg || cfg->depth_fn < -1 || cfg->depth_fn > 5 || cfg->los_fn < 0 || cfg->los_fn > 2) return 58;
  if (cfg->depth_fn == 4 && !(cfg->depth_param > 0.f)) return 58;
  if (cfg->los_fn == 1 && !(cfg->std > 0.f)) return 58;
  if (!acc) return 4;
  if (N == 0) return 0;
  if (!depth_pred || !ranges || !valid || !err || !keep || (cfg->factor > 0.f && !median)) return 4;
  if (cfg->depth_fn >= 0 && !g_depth) return 4;
  const bool los = cfg->los_fn != 0 && R > 0 && S > 0;
  if (los && (!t || !vw || !rays_inds_hit || !pack_infos_hit || !g_vw || !member)) return 4;
  LidarArgs a;
  a.depth = depth_pred, a.ranges = ranges, a.valid = valid, a.err = err, a.median = median, a.N = N;
  a.factor = cfg->factor, a.depth_fn = cfg->depth_fn, a.depth_param = cfg->depth_param, a.w_depth = cfg->w_depth;
  a.los_fn = los ? cfg->los_fn : 0, a.bound = cfg->bound, a.std = cfg->std, a.w_los = cfg->w_los;
  a.t = t, a.vw = vw, a.rays_inds = rays_inds_hit, a.pack_infos = pack_infos_hit, a.R = R, a.S = S;
  a.acc = acc, a.keep = keep, a.g_depth = g_depth, a.g_vw = g_vw, a.member = member;
  const int db = (int)loss_grid(N).x;
  const int lb = los ? (int)loss_grid(R * 64).x : 0;
  hipLaunchKernelGGL(k_lidar_loss, dim3((unsigned)(db + lb)), dim3(LOSS_BLOCK), 0, (hipStream_t)stream, a, db);
  NSIM_CHECK_LAUNCH();
  return 0;
}

// d_depth [N] / d_vw [S] (either may be NULL) from the forward's g_depth, g_vw, member and the three upstream gradients (NULL: 0)
int nsim_lidar_loss_bwd(const float* g_depth, int64_t N, const float* g_vw, const uint8_t* member, int64_t S,
                        const float* gout_depth, const float* gout_neighbor, const float* gout_empty, float* d_depth, float* d_vw,
                        void* stream) {
  if (N < 0 || S < 0) return 2;
  if (d_depth && !g_depth) return 26;
  if (d_vw && (!g_vw || !member)) return 26;
  const int64_t top = (d_depth ? N : 0) > (d_vw ? S : 0) ? N : (d_vw ? S : 0);
  if (top == 0) return 0;
  hipLaunchKernelGGL(k_lidar_loss_bwd, elem_grid(top), dim3(LOSS_BLOCK), 0, (hipStream_t)stream, g_depth, d_depth ? N : 0, g_vw,
                     member, d_vw ? S : 0, gout_depth, gout_neighbor, gout_empty, d_depth, d_vw);
  NSIM_CHECK_LAUNCH();
  return 0;
}

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
