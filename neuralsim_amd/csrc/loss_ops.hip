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
//   * the monocular depth / normal cue losses with their remain mask, and an object's share of the joint rendering (app/loss/mono.py,
//     app/renderers/single_volume_renderer.py:104-120): the last section of this file
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

// ---------------------------------------------------------------------------------------------- monocular depth / normal cues
// The monocular depth / normal cue losses (app/loss/mono.py) and an object's share of the joint rendering:
//   * remain mask: the ignore list of MonoDepthLoss / MonoNormalLoss (mono.py:358-391, 510-524) evaluated into an LDS tile with
//     halo and eroded by a flat 2e x 2e window of ones (kornia.morphology.erosion, geodesic border: mono.py:393-395) -- one launch
//   * scale-and-shift-invariant depth (MonoSDFDepthLoss.forward, mono.py:136-158): five masked moments, the 2x2 solve, one of nine
//     regressions and the multi-scale depth-gradient regulariser, with the gradient THROUGH the solve
//   * Pearson depth (PearsonCorrDepthLoss.forward, mono.py:222-246, reverse_gt False) with its gradient-correlation regulariser
//   * normal cue (MonoNormalLoss.fn, mono.py:479-484) with the world -> camera rotation of mono.py:507
// The reference composes each of these from tens of torch ops on a 64x64 / 80x120 patch; here at most two launches forward and
// one backward.  Every sum is taken in f64 (per thread, per workgroup, one f64 atomic per workgroup and quantity): the determinant
// a00 a11 - a01^2 of the solve and the centred moments of the correlation cancel badly in f32.  The LAST workgroup to finish (a
// ticket counter in the zeroed workspace) turns the f64 totals into the f32 losses, so nothing is converted by a further launch.

#define MONO_BLOCK 256
#define MONO_MAX_BLOCKS 256
#define MONO_TILE 32
#define MONO_MAX_ERODE 32
#define MONO_REGION (MONO_TILE + 2 * MONO_MAX_ERODE - 1)
#define MONO_MAX_SCALES 8
#define MONO_MAX_SETS (1 + 2 * MONO_MAX_SCALES)

static inline dim3 mono_grid(int64_t n) {
  return dim3(nsim_blocks(n, MONO_BLOCK, MONO_MAX_BLOCKS));
}

// K partial sums of one block added into acc[0..K) (f64 atomics, one per non-zero sum)
template <int K>
__device__ __forceinline__ void mono_block_sums(const double (&v)[K], double* acc) {
  __shared__ double red[K][MONO_BLOCK / 64];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double s = wave_sum(v[k]);
    if (nsim_lane() == 0) red[k][threadIdx.x >> 6] = s;
  }
  __syncthreads();
  if (threadIdx.x < K) {
    double tot = 0.0;
    for (int w = 0; w < MONO_BLOCK / 64; ++w) tot += red[threadIdx.x][w];
    if (tot != 0.0) atomicAdd(acc + threadIdx.x, tot);
  }
  __syncthreads();
}

// Outside a HIP compile (the host emulator of the tests) workgroups run one after another: nothing to order.
#if defined(__HIP__)
__device__ __forceinline__ void mono_release() { nsim_release_agent(); }
#else
inline void mono_release() {}
#endif

// true in thread 0 of the block that finishes last (its view of every other block's atomics is complete)
__device__ __forceinline__ bool mono_last_block(unsigned* ticket) {
  if (threadIdx.x != 0) return false;
  mono_release();                // the sums above left through atomics of THIS wave (threads 0..K-1): complete before the ticket
  return atomicAdd(ticket, 1u) == gridDim.x - 1;
}

__device__ __forceinline__ double mono_read(double* p) { return atomicAdd(p, 0.0); }

// ---------------------------------------------------------------------------------------------- remain mask
struct MonoMaskArgs {
  const float *mask_pred, *depth_pred0, *depth_pred, *depth_gt;
  const uint8_t *occ, *dyn, *human;
  const double* gt_sum;     // sum of depth_gt (mono_distant)
  float thresh, far, far08;
  int flags;                // bit 0 toofar, 1 pred_not_occupied, 2 not_occupied, 3 dynamic, 4 human, 5 pred_distant, 6 mono_distant
  int keep_all;             // the depth loss with an empty list: every pixel remains (mono.py:396-397)
  int H, W, e;
  int64_t n;
};

__device__ __forceinline__ uint8_t mono_remain(const MonoMaskArgs& a, int64_t i, float gt_gate) {
  if (a.keep_all) return 1;
  bool ign = false;
  if (a.flags & 1) ign |= a.depth_pred0[i] > a.far;
  if (a.flags & 2) ign |= !(a.mask_pred[i] > a.thresh);
  if (a.flags & 4) ign |= !a.occ[i];
  if (a.flags & 8) ign |= a.dyn[i] != 0;
  if (a.flags & 16) ign |= a.human[i] != 0;
  if (a.flags & 32) ign |= a.depth_pred[i] > a.far08;
  if (a.flags & 64) ign |= a.depth_gt[i] > gt_gate;
  return ign ? 0 : 1;
}

__device__ __forceinline__ float mono_gt_gate(const MonoMaskArgs& a) {
  // depth_gt.mean() - 1e-5 in f32 (mono.py:388); the mean itself from the f64 sum
  return (a.flags & 64) ? (float)(a.gt_sum[0] / (double)a.n) - 1e-5f : 0.f;
}

__global__ void __launch_bounds__(MONO_BLOCK) k_mono_mask_flat(MonoMaskArgs a, uint8_t* __restrict__ out) {
  const float gate = mono_gt_gate(a);
  for (int64_t i = (int64_t)blockIdx.x * MONO_BLOCK + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * MONO_BLOCK)
    out[i] = mono_remain(a, i, gate);
}

// one 32 x 32 tile of the output per block: the predicates of the tile and its halo (e before, e - 1 after; a pixel outside the
// image is 1: it does not erode) into LDS, the row minimum over 2e columns, then the column minimum over 2e rows
__global__ void __launch_bounds__(MONO_BLOCK) k_mono_mask_erode(MonoMaskArgs a, uint8_t* __restrict__ out) {
  __shared__ uint8_t P[MONO_REGION * MONO_REGION];
  __shared__ uint8_t R[MONO_REGION * MONO_TILE];
  const float gate = mono_gt_gate(a);
  const int e = a.e, k = 2 * e, reg = MONO_TILE + k - 1;
  const int y0 = (int)blockIdx.y * MONO_TILE - e, x0 = (int)blockIdx.x * MONO_TILE - e;
  for (int j = threadIdx.x; j < reg * reg; j += MONO_BLOCK) {
    const int y = y0 + j / reg, x = x0 + j % reg;
    P[j] = (y >= 0 && y < a.H && x >= 0 && x < a.W) ? mono_remain(a, (int64_t)y * a.W + x, gate) : 1;
  }
  __syncthreads();
  for (int j = threadIdx.x; j < reg * MONO_TILE; j += MONO_BLOCK) {
    const int r = j / MONO_TILE, c = j % MONO_TILE;
    uint8_t m = 1;
    for (int d = 0; d < k; ++d) m &= P[r * reg + c + d];
    R[j] = m;
  }
  __syncthreads();
  for (int j = threadIdx.x; j < MONO_TILE * MONO_TILE; j += MONO_BLOCK) {
    const int r = j / MONO_TILE, c = j % MONO_TILE;
    const int y = (int)blockIdx.y * MONO_TILE + r, x = (int)blockIdx.x * MONO_TILE + c;
    if (y >= a.H || x >= a.W) continue;
    uint8_t m = 1;
    for (int d = 0; d < k; ++d) m &= R[(r + d) * MONO_TILE + c];
    out[(int64_t)y * a.W + x] = m;
  }
}

__global__ void __launch_bounds__(MONO_BLOCK) k_mono_sum_f64(const float* __restrict__ x, int64_t n, double* __restrict__ out) {
  double acc[1] = {0.0};
  for (int64_t i = (int64_t)blockIdx.x * MONO_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * MONO_BLOCK) acc[0] += (double)x[i];
  mono_block_sums<1>(acc, out);
}

// ---------------------------------------------------------------------------------------------- scale-and-shift-invariant depth
// workspace (f64, zero on entry): [0..5) a00 a01 a11 b0 b1, [5] sum m f, [6] sum of the regulariser's |differences|,
// [7..11) d depth / d scale, d depth / d shift, d reg / d scale, d reg / d shift, [11] the ticket (its first 4 bytes)
#define SSI_WS 12
struct SsiArgs {
  const float *pred, *gt;
  const uint8_t* mask;
  int H, W;
  int fn;                   // 0 mse, 1 l1, 2 log_l1, 3 smooth_l1 (beta), 4 relative_l1 / mape (eps), 5 smape (eps), 6 relative_l2 (eps),
  double param;             // 7 huber (alpha)
  double pre_scale, pre_shift;
  int gt_to_pred, detach, n_scales;
  double w_depth, w_reg;    // w / (H W), w alpha_grad_reg
};

__device__ __forceinline__ double ssi_target(const SsiArgs& a, int64_t i) {
  return a.pre_scale * (double)a.gt[i] + a.pre_shift;
}

struct SsiSolve {
  double scale, shift, det;
};

// (the moments are a previous launch's: plain reads)
__device__ __forceinline__ SsiSolve ssi_solve(const double* ws) {
  const double a00 = ws[0], a01 = ws[1], a11 = ws[2], b0 = ws[3], b1 = ws[4];
  SsiSolve s;
  s.det = a00 * a11 - a01 * a01;
  s.scale = s.det != 0.0 ? (a11 * b0 - a01 * b1) / s.det : 0.0;
  s.shift = s.det != 0.0 ? (-a01 * b0 + a00 * b1) / s.det : 0.0;
  return s;
}

__device__ __forceinline__ double mono_sign(double x) { return x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : 0.0); }

// f(a, b) of nr3d_lib/models/loss/recon.py (log_l1: mono.py:64) and its derivatives to both arguments
__device__ __forceinline__ double ssi_fn(int fn, double prm, double a, double b, double& fa, double& fb) {
  const double d = a - b, sd = mono_sign(d), ad = fabs(d);
  switch (fn) {
    case 0:
      fa = 2.0 * d, fb = -fa;
      return d * d;
    case 1:
      fa = sd, fb = -sd;
      return ad;
    case 2: {
      const double ac = a + 1.0 > 1e-3 ? a + 1.0 : 1e-3;
      const double u = log(ac) - log(b + 1.0), su = mono_sign(u);
      fa = a + 1.0 >= 1e-3 ? su / ac : 0.0;
      fb = -su / (b + 1.0);
      return fabs(u);
    }
    case 3:
      if (ad < prm) {
        fa = d / prm, fb = -fa;
        return 0.5 * d * d / prm;
      }
      fa = sd, fb = -sd;
      return ad - 0.5 * prm;
    case 4: {
      const double q = fabs(b) + prm;
      fa = sd / q;
      fb = -sd / q - ad * mono_sign(b) / (q * q);
      return ad / q;
    }
    case 5: {
      const double q = 0.5 * (fabs(a) + fabs(b)) + prm;
      fa = sd / q - ad * 0.5 * mono_sign(a) / (q * q);
      fb = -sd / q - ad * 0.5 * mono_sign(b) / (q * q);
      return ad / q;
    }
    case 6: {
      const double q = b * b + prm;
      fa = 2.0 * d / q;
      fb = -fa - d * d * 2.0 * b / (q * q);
      return d * d / q;
    }
    default:
      if (ad < prm) {
        fa = d, fb = -d;
        return 0.5 * d * d;
      }
      fa = prm * sd, fb = -fa;
      return prm * (ad - 0.5 * prm);
  }
}

__global__ void __launch_bounds__(MONO_BLOCK) k_ssi_moments(SsiArgs a, double* __restrict__ ws) {
  double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  const int64_t n = (int64_t)a.H * a.W;
  for (int64_t i = (int64_t)blockIdx.x * MONO_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * MONO_BLOCK) {
    if (!a.mask[i]) continue;
    const double p = (double)a.pred[i], t = ssi_target(a, i);
    acc[0] += p * p, acc[1] += p, acc[2] += 1.0, acc[3] += p * t, acc[4] += t;
  }
  mono_block_sums<5>(acc, ws);
}

// the two compared images at pixel i: (scale pred + shift, target) or (pred, (target - shift) / scale)
__device__ __forceinline__ void ssi_pair(const SsiArgs& a, const SsiSolve& s, int64_t i, double& pa, double& pb) {
  const double p = (double)a.pred[i], t = ssi_target(a, i);
  if (a.gt_to_pred) pa = p, pb = (t - s.shift) / s.scale;
  else pa = s.scale * p + s.shift, pb = t;
}

__global__ void __launch_bounds__(MONO_BLOCK) k_ssi_main(SsiArgs a, double* __restrict__ ws, float* __restrict__ out,
                                                         float* __restrict__ g_depth, float* __restrict__ g_reg) {
  __shared__ SsiSolve sol;
  if (threadIdx.x == 0) sol = ssi_solve(ws);
  __syncthreads();
  const SsiSolve s = sol;
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const int64_t n = (int64_t)a.H * a.W;
  for (int64_t i = (int64_t)blockIdx.x * MONO_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * MONO_BLOCK) {
    float gd = 0.f, gr = 0.f;
    if (a.mask[i]) {      // a masked-out pixel is not evaluated (the reference multiplies its value by 0)
      const int y = (int)(i / a.W), x = (int)(i % a.W);
      const double p = (double)a.pred[i];
      double pa, pb, fa, fb;
      ssi_pair(a, s, i, pa, pb);
      acc[0] += ssi_fn(a.fn, a.param, pa, pb, fa, fb);
      // the regulariser: L1 of the x- and y-differences of (pa - pb) on the ::2^k sub-images, pairs with both mask pixels set
      // (mono.py:115-134).  G = d (sum) / d (pa - pb) at this pixel; the pair's value is counted by its left / upper pixel.
      double G = 0.0;
      if (a.w_reg != 0.0) {
        const double D = pa - pb;
        for (int k = 0; k < a.n_scales; ++k) {
          const int step = 1 << k;
          if ((y & (step - 1)) || (x & (step - 1))) break;
          const int64_t nb[4] = {x + step < a.W ? i + step : -1, y + step < a.H ? i + (int64_t)step * a.W : -1,
                                 x - step >= 0 ? i - step : -1, y - step >= 0 ? i - (int64_t)step * a.W : -1};
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            if (nb[q] < 0 || !a.mask[nb[q]]) continue;
            double qa, qb;
            ssi_pair(a, s, nb[q], qa, qb);
            const double df = q < 2 ? (qa - qb) - D : D - (qa - qb);
            if (q < 2) acc[1] += fabs(df), G -= mono_sign(df);
            else G += mono_sign(df);
          }
        }
      }
      // direct gradients to pred, and the chain sums d L / d scale, d L / d shift (the backward multiplies them by d scale /
      // d pred, d shift / d pred: closed-form from the moments)
      const double wd = a.w_depth, wr = a.w_reg;
      if (a.gt_to_pred) {
        gd = (float)(wd * fa), gr = (float)(wr * G);
        const double b_s = -pb / s.scale, b_h = -1.0 / s.scale;
        acc[2] += fb * b_s, acc[3] += fb * b_h, acc[4] += -G * b_s, acc[5] += -G * b_h;
      } else {
        gd = (float)(wd * fa * s.scale), gr = (float)(wr * G * s.scale);
        acc[2] += fa * p, acc[3] += fa, acc[4] += G * p, acc[5] += G;
      }
    }
    g_depth[i] = gd;
    g_reg[i] = gr;
  }
  acc[0] *= a.w_depth, acc[2] *= a.w_depth, acc[3] *= a.w_depth;
  acc[1] *= a.w_reg, acc[4] *= a.w_reg, acc[5] *= a.w_reg;
  mono_block_sums<6>(acc, ws + 5);
  if (mono_last_block(reinterpret_cast<unsigned*>(ws + 11))) {
    out[0] = (float)mono_read(ws + 5);
    out[1] = (float)mono_read(ws + 6);
  }
}

__global__ void __launch_bounds__(MONO_BLOCK) k_ssi_bwd(SsiArgs a, double* __restrict__ ws, const float* __restrict__ g_depth,
                                                        const float* __restrict__ g_reg, const float* __restrict__ gout0,
                                                        const float* __restrict__ gout1, float* __restrict__ d_pred) {
  const double a01 = ws[1], a11 = ws[2], b0 = ws[3], b1 = ws[4];
  const SsiSolve s = ssi_solve(ws);
  const double det = s.det, scale = s.scale, shift = s.shift;
  const bool chain = det != 0.0 && !a.detach;
  const double g0 = gout0 ? (double)gout0[0] : 0.0, g1 = gout1 ? (double)gout1[0] : 0.0;
  const double c_s = g0 * ws[7] + g1 * ws[9], c_h = g0 * ws[8] + g1 * ws[10];
  const int64_t n = (int64_t)a.H * a.W;
  for (int64_t i = (int64_t)blockIdx.x * MONO_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * MONO_BLOCK) {
    double d = g0 * (double)g_depth[i] + g1 * (double)g_reg[i];
    if (chain && a.mask[i]) {
      const double p = (double)a.pred[i], t = ssi_target(a, i);
      const double ddet = 2.0 * (p * a11 - a01);
      d += (c_s * ((a11 * t - b1) - scale * ddet) + c_h * ((2.0 * p * b1 - b0 - a01 * t) - shift * ddet)) / det;
    }
    d_pred[i] = (float)d;
  }
}

// ---------------------------------------------------------------------------------------------- Pearson depth
// set 0: (pred, gt) over the masked pixels; set 1 + 2k / 2 + 2k: their x- / y-differences on the ::2^k sub-image over the pairs
// with both mask pixels set.  workspace (f64, zero on entry): per set n, Sx, Sy, Sxx, Syy, Sxy; then the ticket.
#define PEARSON_WS (6 * MONO_MAX_SETS + 1)
struct PearsonArgs {
  const float *pred, *gt;
  const uint8_t* mask;
  int H, W, n_scales;       // n_scales 0: no regulariser
  double w_depth, w_reg;    // w, w alpha_grad_reg
};

// the pair (x, y) pixel i adds to ``set``, false when it adds none
__device__ __forceinline__ bool pearson_sample(const PearsonArgs& a, int set, int64_t i, double& x, double& y) {
  if (!a.mask[i]) return false;
  if (set == 0) {
    x = (double)a.pred[i], y = (double)a.gt[i];
    return true;
  }
  const int k = (set - 1) >> 1, step = 1 << k, py = (int)(i / a.W), px = (int)(i % a.W);
  if ((py & (step - 1)) || (px & (step - 1))) return false;
  int64_t j;
  if ((set - 1) & 1) {
    if (py + step >= a.H) return false;
    j = i + (int64_t)step * a.W;
  } else {
    if (px + step >= a.W) return false;
    j = i + step;
  }
  if (!a.mask[j]) return false;
  x = (double)a.pred[j] - (double)a.pred[i], y = (double)a.gt[j] - (double)a.gt[i];
  return true;
}

struct PearsonSet {
  double mx, my, inv_d, c_over_a, r;
  int valid;
};

// centred moments from the raw f64 sums; r = C / max(sqrt(A) sqrt(B), 1e-12)
__device__ __forceinline__ PearsonSet pearson_set(const double* s) {
  PearsonSet o;
  o.valid = s[0] > 0.0;
  o.mx = o.my = o.inv_d = o.c_over_a = o.r = 0.0;
  if (!o.valid) return o;
  o.mx = s[1] / s[0], o.my = s[2] / s[0];
  const double A = fmax(s[3] - s[1] * o.mx, 0.0), B = fmax(s[4] - s[2] * o.my, 0.0), C = s[5] - s[1] * o.my;
  const double den = sqrt(A) * sqrt(B);
  if (den >= 1e-12) o.inv_d = 1.0 / den, o.c_over_a = C / A;
  else o.inv_d = 1e12;
  o.r = C * o.inv_d;
  return o;
}

__global__ void __launch_bounds__(MONO_BLOCK) k_pearson_fwd(PearsonArgs a, double* __restrict__ ws, float* __restrict__ out) {
  const int64_t n = (int64_t)a.H * a.W;
  const int n_sets = 1 + 2 * a.n_scales;
  for (int set = 0; set < n_sets; ++set) {
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * MONO_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * MONO_BLOCK) {
      double x, y;
      if (!pearson_sample(a, set, i, x, y)) continue;
      acc[0] += 1.0, acc[1] += x, acc[2] += y, acc[3] += x * x, acc[4] += y * y, acc[5] += x * y;
    }
    mono_block_sums<6>(acc, ws + 6 * set);
  }
  if (mono_last_block(reinterpret_cast<unsigned*>(ws + 6 * MONO_MAX_SETS))) {
    double reg = 0.0, dep = 0.0;
    for (int set = 0; set < n_sets; ++set) {
      double s[6];
      for (int q = 0; q < 6; ++q) s[q] = mono_read(ws + 6 * set + q);
      const PearsonSet ps = pearson_set(s);
      if (!ps.valid) continue;       // no pixel / no valid pair: the term is 0 (mono.py:181-194), decided here
      if (set == 0) dep = 1.0 - ps.r;
      else reg += 1.0 - ps.r;
    }
    out[0] = (float)(a.w_depth * dep);
    out[1] = (float)(a.w_reg * reg);
  }
}

__global__ void __launch_bounds__(MONO_BLOCK) k_pearson_bwd(PearsonArgs a, const double* __restrict__ ws, const float* __restrict__ gout0,
                                                            const float* __restrict__ gout1, float* __restrict__ d_pred) {
  __shared__ PearsonSet sets[MONO_MAX_SETS];
  const int n_sets = 1 + 2 * a.n_scales;
  if ((int)threadIdx.x < n_sets) sets[threadIdx.x] = pearson_set(ws + 6 * threadIdx.x);
  __syncthreads();
  const double g0 = (gout0 ? (double)gout0[0] : 0.0) * a.w_depth, g1 = (gout1 ? (double)gout1[0] : 0.0) * a.w_reg;
  const int64_t n = (int64_t)a.H * a.W;
  for (int64_t i = (int64_t)blockIdx.x * MONO_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * MONO_BLOCK) {
    double d = 0.0;
    if (a.mask[i]) {
      // d (1 - r) / d x_j = -((y_j - my) - (C / A) (x_j - mx)) / den; a difference x = pred[j] - pred[i] hands it to j and, negated, to i
      const int py = (int)(i / a.W), px = (int)(i % a.W);
      for (int set = 0; set < n_sets; ++set) {
        const PearsonSet& ps = sets[set];
        if (!ps.valid) continue;
        double x, y;
        const double g = set == 0 ? g0 : g1;
        if (pearson_sample(a, set, i, x, y)) {
          const double t = -((y - ps.my) - ps.c_over_a * (x - ps.mx)) * ps.inv_d;
          d += set == 0 ? g * t : -g * t;
        }
        if (set > 0) {           // the pair this pixel closes (its left / upper neighbour opens it)
          const int step = 1 << ((set - 1) >> 1);
          const bool vert = (set - 1) & 1;
          if ((py & (step - 1)) || (px & (step - 1))) continue;
          if (vert ? py - step < 0 : px - step < 0) continue;
          const int64_t j = vert ? i - (int64_t)step * a.W : i - step;
          if (pearson_sample(a, set, j, x, y)) d += g * -((y - ps.my) - ps.c_over_a * (x - ps.mx)) * ps.inv_d;
        }
      }
    }
    d_pred[i] = (float)d;
  }
}

// ---------------------------------------------------------------------------------------------- normal cue
// rot_mode 0: none; 1: one [3,3]; 2: per row [N,3,3] -- n' = rot n (world -> camera), a constant of the backward.
// workspace (f64, zero on entry): the two sums, the ticket.
#define NORMAL_WS 3
__device__ __forceinline__ void mono_normalize(const double v[3], double y[3], double& len) {
  len = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  const double dnm = len > 1e-12 ? len : 1e-12;      // F.normalize: v / max(|v|, eps)
  y[0] = v[0] / dnm, y[1] = v[1] / dnm, y[2] = v[2] / dnm;
}

__global__ void __launch_bounds__(MONO_BLOCK) k_normal_cue_fwd(const float* __restrict__ np, const float* __restrict__ ng,
                                                               const uint8_t* __restrict__ mask, const float* __restrict__ rot,
                                                               int rot_mode, int64_t N, double w_l1, double w_cos, double* __restrict__ ws,
                                                               float* __restrict__ out, float* __restrict__ g_l1,
                                                               float* __restrict__ g_cos) {
  double acc[2] = {0.0, 0.0};
  const double s1 = w_l1 / (double)N, s2 = w_cos / (double)N;
  for (int64_t i = (int64_t)blockIdx.x * MONO_BLOCK + threadIdx.x; i < N; i += (int64_t)gridDim.x * MONO_BLOCK) {
    double d1[3] = {0.0, 0.0, 0.0}, d2[3] = {0.0, 0.0, 0.0};
    if (!mask || mask[i]) {
      double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
      if (rot_mode) {
        const float* r = rot + (rot_mode == 2 ? 9 * i : 0);
        for (int q = 0; q < 9; ++q) R[q] = (double)r[q];
      }
      const double v[3] = {(double)np[3 * i], (double)np[3 * i + 1], (double)np[3 * i + 2]};
      const double u[3] = {R[0] * v[0] + R[1] * v[1] + R[2] * v[2], R[3] * v[0] + R[4] * v[1] + R[5] * v[2],
                           R[6] * v[0] + R[7] * v[1] + R[8] * v[2]};
      const double gt[3] = {(double)ng[3 * i], (double)ng[3 * i + 1], (double)ng[3 * i + 2]};
      double yp[3], yg[3], lp, lg;
      mono_normalize(u, yp, lp);
      mono_normalize(gt, yg, lg);
      double a1[3], a2[3];       // d l1 / d yp, d cos-term / d yp
      for (int c = 0; c < 3; ++c) {
        const double df = yp[c] - yg[c];
        acc[0] += fabs(df);
        a1[c] = mono_sign(df), a2[c] = -yg[c];
      }
      acc[1] += 1.0 - (yp[0] * yg[0] + yp[1] * yg[1] + yp[2] * yg[2]);
      // through the normalisation: (a - y (y . a)) / |u|, or a / eps where the clamp holds; then through the rotation: R^T
      double b1[3], b2[3];
      if (lp > 1e-12) {
        const double p1 = yp[0] * a1[0] + yp[1] * a1[1] + yp[2] * a1[2], p2 = yp[0] * a2[0] + yp[1] * a2[1] + yp[2] * a2[2];
        for (int c = 0; c < 3; ++c) b1[c] = (a1[c] - yp[c] * p1) / lp, b2[c] = (a2[c] - yp[c] * p2) / lp;
      } else {
        for (int c = 0; c < 3; ++c) b1[c] = a1[c] * 1e12, b2[c] = a2[c] * 1e12;
      }
      for (int c = 0; c < 3; ++c) {
        d1[c] = s1 * (R[c] * b1[0] + R[3 + c] * b1[1] + R[6 + c] * b1[2]);
        d2[c] = s2 * (R[c] * b2[0] + R[3 + c] * b2[1] + R[6 + c] * b2[2]);
      }
    }
    for (int c = 0; c < 3; ++c) g_l1[3 * i + c] = (float)d1[c], g_cos[3 * i + c] = (float)d2[c];
  }
  acc[0] *= s1, acc[1] *= s2;
  mono_block_sums<2>(acc, ws);
  if (mono_last_block(reinterpret_cast<unsigned*>(ws + 2))) {
    out[0] = (float)mono_read(ws);
    out[1] = (float)mono_read(ws + 1);
  }
}

// d [n] = gout0[0] g0 [n] + gout1[0] g1 [n] (a NULL upstream gradient is 0)
__global__ void __launch_bounds__(MONO_BLOCK) k_mono_scale2(const float* __restrict__ g0, const float* __restrict__ g1, int64_t n,
                                                            const float* __restrict__ gout0, const float* __restrict__ gout1,
                                                            float* __restrict__ d) {
  const float s0 = gout0 ? gout0[0] : 0.f, s1 = gout1 ? gout1[0] : 0.f;
  for (int64_t i = (int64_t)blockIdx.x * MONO_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * MONO_BLOCK)
    d[i] = s0 * g0[i] + s1 * g1[i];
}

// ---------------------------------------------------------------------------------------------- an object's share of the joint rendering
// _volume_integration_in_total (app/renderers/single_volume_renderer.py:104-120): per pack of one object's buffer the sums of its
// samples weighted by vw_in_total, placed at the pack's ray.  One wave per pack, f64 partial sums.
struct ShareArgs {
  const float *vw, *t, *rgb, *nab;
  const int64_t *pack_infos, *rays_inds;
  int64_t P, N;
  int norm_depth, norm_nablas;
};

// the integrated normal of a sample: the nabla itself (training) or normalize(clamp(nabla, -1, 1)) (mono.py's eval branch, :118)
__device__ __forceinline__ void share_normal(const ShareArgs& a, int64_t j, double y[3], double c[3], double& len) {
  for (int q = 0; q < 3; ++q) y[q] = c[q] = (double)a.nab[3 * j + q];
  len = 1.0;
  if (!a.norm_nablas) return;
  for (int q = 0; q < 3; ++q) c[q] = fmin(fmax(c[q], -1.0), 1.0);
  mono_normalize(c, y, len);
}

__global__ void __launch_bounds__(MONO_BLOCK) k_packed_share_fwd(ShareArgs a, float* __restrict__ mask, float* __restrict__ depth,
                                                                 float* __restrict__ rgb, float* __restrict__ nrm) {
  const int lane = nsim_lane();
  for (int64_t r = (int64_t)blockIdx.x * (MONO_BLOCK / 64) + (threadIdx.x >> 6); r < a.P; r += (int64_t)gridDim.x * (MONO_BLOCK / 64)) {
    const int64_t b = a.pack_infos[2 * r], n = a.pack_infos[2 * r + 1], ray = a.rays_inds[r];
    double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t j = b + lane; j < b + n; j += 64) {
      const double w = (double)a.vw[j];
      acc[0] += w, acc[1] += w * (double)a.t[j];
      if (a.rgb)
        for (int q = 0; q < 3; ++q) acc[2 + q] += w * (double)a.rgb[3 * j + q];
      if (a.nab) {
        double y[3], c[3], len;
        share_normal(a, j, y, c, len);
        for (int q = 0; q < 3; ++q) acc[5 + q] += w * y[q];
      }
    }
    for (int q = 0; q < 8; ++q) acc[q] = wave_sum(acc[q]);
    if (lane == 0 && ray >= 0 && ray < a.N) {
      mask[ray] = (float)acc[0];
      depth[ray] = (float)(a.norm_depth ? acc[1] / (acc[0] + 1e-10) : acc[1]);
      if (a.rgb)
        for (int q = 0; q < 3; ++q) rgb[3 * ray + q] = (float)acc[2 + q];
      if (a.nab)
        for (int q = 0; q < 3; ++q) nrm[3 * ray + q] = (float)acc[5 + q];
    }
  }
}

// mask / depth: the forward's outputs (the normalised depth's derivative is (t - depth) / (mask + 1e-10)); a NULL g_* is 0
__global__ void __launch_bounds__(MONO_BLOCK) k_packed_share_bwd(ShareArgs a, const float* __restrict__ mask,
                                                                 const float* __restrict__ depth, const float* __restrict__ g_mask,
                                                                 const float* __restrict__ g_depth, const float* __restrict__ g_rgb,
                                                                 const float* __restrict__ g_nrm, float* __restrict__ d_vw,
                                                                 float* __restrict__ d_rgb, float* __restrict__ d_nab) {
  const int lane = nsim_lane();
  for (int64_t r = (int64_t)blockIdx.x * (MONO_BLOCK / 64) + (threadIdx.x >> 6); r < a.P; r += (int64_t)gridDim.x * (MONO_BLOCK / 64)) {
    const int64_t b = a.pack_infos[2 * r], n = a.pack_infos[2 * r + 1], ray = a.rays_inds[r];
    const bool ok = ray >= 0 && ray < a.N;
    const double gm = ok && g_mask ? (double)g_mask[ray] : 0.0, gd = ok && g_depth ? (double)g_depth[ray] : 0.0;
    const double m = ok ? (double)mask[ray] : 0.0, dep = ok ? (double)depth[ray] : 0.0;
    double gc[3] = {0.0, 0.0, 0.0}, gn[3] = {0.0, 0.0, 0.0};
    for (int q = 0; q < 3; ++q) {
      if (ok && g_rgb) gc[q] = (double)g_rgb[3 * ray + q];
      if (ok && g_nrm) gn[q] = (double)g_nrm[3 * ray + q];
    }
    for (int64_t j = b + lane; j < b + n; j += 64) {
      const double w = (double)a.vw[j], t = (double)a.t[j];
      double d = gm + gd * (a.norm_depth ? (t - dep) / (m + 1e-10) : t);
      if (a.rgb) {
        for (int q = 0; q < 3; ++q) d += gc[q] * (double)a.rgb[3 * j + q];
        if (d_rgb)
          for (int q = 0; q < 3; ++q) d_rgb[3 * j + q] = (float)(w * gc[q]);
      }
      if (a.nab) {
        double y[3], c[3], len;
        share_normal(a, j, y, c, len);
        for (int q = 0; q < 3; ++q) d += gn[q] * y[q];
        if (d_nab) {
          double o[3] = {w * gn[0], w * gn[1], w * gn[2]};
          if (a.norm_nablas) {       // through normalize (v / max(|v|, 1e-12)) and the clamp (passes inside [-1, 1])
            const double dot = y[0] * o[0] + y[1] * o[1] + y[2] * o[2];
            for (int q = 0; q < 3; ++q) {
              o[q] = len > 1e-12 ? (o[q] - y[q] * dot) / len : o[q] * 1e12;
              const double v = (double)a.nab[3 * j + q];
              if (v < -1.0 || v > 1.0) o[q] = 0.0;
            }
          }
          for (int q = 0; q < 3; ++q) d_nab[3 * j + q] = (float)o[q];
        }
      }
      if (d_vw) d_vw[j] = (float)d;
    }
  }
}

// ---------------------------------------------------------------------------------------------- scene-flow losses
// FlowLoss.fn_cycle / fn_sparsity (app/loss/flow.py:35-55) on the four [S,3] flow tensors of a with-flow EmerNeRF query, both terms
// in one launch per direction:
//   cycle    = w_cycle 1/2 mean over S 3 of (sg(flow_fwd) + flow_fwd_pred_bwd)^2 + (sg(flow_bwd) + flow_bwd_pred_fwd)^2
//   sparsity = w_sparsity 1/4 mean over S of |flow_fwd| + |flow_fwd_pred_bwd| + |flow_bwd| + |flow_bwd_pred_fwd|
// sg = stop-gradient: the cycle term differentiates the two predictions only.  The gradient of a norm at zero is zero (as torch's).
// workspace (f64, zero on entry): the two sums, the ticket.
#define FLOW_WS 3
struct FlowLossArgs {
  const float *ff, *fpb, *fb, *bpf;      // flow_fwd, flow_fwd_pred_bwd, flow_bwd, flow_bwd_pred_fwd
  int64_t S;
  double s_cycle, s_sparsity;            // w_cycle / (2 S 3), w_sparsity / (4 S)
};

__device__ __forceinline__ double flow_row(const float* p, int64_t i, double v[3]) {
  v[0] = (double)p[3 * i], v[1] = (double)p[3 * i + 1], v[2] = (double)p[3 * i + 2];
  return sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
}

__global__ void __launch_bounds__(MONO_BLOCK) k_flow_loss_fwd(FlowLossArgs a, double* __restrict__ ws, float* __restrict__ out) {
  double acc[2] = {0.0, 0.0};
  for (int64_t i = (int64_t)blockIdx.x * MONO_BLOCK + threadIdx.x; i < a.S; i += (int64_t)gridDim.x * MONO_BLOCK) {
    double ff[3], fpb[3], fb[3], bpf[3];
    const double n = flow_row(a.ff, i, ff) + flow_row(a.fpb, i, fpb) + flow_row(a.fb, i, fb) + flow_row(a.bpf, i, bpf);
    double c = 0.0;
    for (int q = 0; q < 3; ++q) {
      const double u = ff[q] + fpb[q], v = fb[q] + bpf[q];
      c += u * u + v * v;
    }
    acc[0] += c, acc[1] += n;
  }
  acc[0] *= a.s_cycle, acc[1] *= a.s_sparsity;
  mono_block_sums<2>(acc, ws);
  if (mono_last_block(reinterpret_cast<unsigned*>(ws + 2))) {
    out[0] = (float)mono_read(ws);
    out[1] = (float)mono_read(ws + 1);
  }
}

// d_* [S,3] are written (a NULL upstream gradient is 0; a NULL d_* is not wanted)
__global__ void __launch_bounds__(MONO_BLOCK) k_flow_loss_bwd(FlowLossArgs a, const float* __restrict__ gout_cycle,
                                                              const float* __restrict__ gout_sparsity, float* __restrict__ d_ff,
                                                              float* __restrict__ d_fpb, float* __restrict__ d_fb,
                                                              float* __restrict__ d_bpf) {
  const double gc = gout_cycle ? 2.0 * a.s_cycle * (double)gout_cycle[0] : 0.0;
  const double gs = gout_sparsity ? a.s_sparsity * (double)gout_sparsity[0] : 0.0;
  for (int64_t i = (int64_t)blockIdx.x * MONO_BLOCK + threadIdx.x; i < a.S; i += (int64_t)gridDim.x * MONO_BLOCK) {
    double ff[3], fpb[3], fb[3], bpf[3];
    const double nff = flow_row(a.ff, i, ff), nfpb = flow_row(a.fpb, i, fpb), nfb = flow_row(a.fb, i, fb), nbpf = flow_row(a.bpf, i, bpf);
    const double rff = nff > 0.0 ? gs / nff : 0.0, rfpb = nfpb > 0.0 ? gs / nfpb : 0.0;
    const double rfb = nfb > 0.0 ? gs / nfb : 0.0, rbpf = nbpf > 0.0 ? gs / nbpf : 0.0;
    for (int q = 0; q < 3; ++q) {
      if (d_ff) d_ff[3 * i + q] = (float)(rff * ff[q]);
      if (d_fpb) d_fpb[3 * i + q] = (float)(gc * (ff[q] + fpb[q]) + rfpb * fpb[q]);
      if (d_fb) d_fb[3 * i + q] = (float)(rfb * fb[q]);
      if (d_bpf) d_bpf[3 * i + q] = (float)(gc * (fb[q] + bpf[q]) + rbpf * bpf[q]);
    }
  }
}

extern "C" {

int nsim_mono_sum_f64(const float* x, int64_t n, double* out, void* stream) {
  if (n < 0) return 2;
  if (!out) return 4;
  if (n == 0) return 0;
  if (!x) return 4;
  hipLaunchKernelGGL(k_mono_sum_f64, mono_grid(n), dim3(MONO_BLOCK), 0, (hipStream_t)stream, x, n, out);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_mono_remain_mask(const float* mask_pred, const float* depth_pred0, const float* depth_pred, const float* depth_gt,
                          const uint8_t* occupancy_gt, const uint8_t* dynamic_gt, const uint8_t* human_gt, const double* depth_gt_sum,
                          int64_t H, int64_t W, float mask_pred_thresh, float far, float far08, int flags, int keep_all, int erode,
                          uint8_t* out, void* stream) {
  if (H < 0 || W < 0 || H * W > ((int64_t)1 << 30)) return 2;
  if (erode < 0 || erode > MONO_MAX_ERODE || (flags & ~127)) return 58;
  if (H * W == 0) return 0;
  if (!out) return 4;
  if (!keep_all) {
    if (((flags & 1) && !depth_pred0) || ((flags & 2) && !mask_pred) || ((flags & 4) && !occupancy_gt) || ((flags & 8) && !dynamic_gt) ||
        ((flags & 16) && !human_gt) || ((flags & 32) && !depth_pred) || ((flags & 64) && (!depth_gt || !depth_gt_sum)))
      return 4;
  }
  MonoMaskArgs a;
  a.mask_pred = mask_pred, a.depth_pred0 = depth_pred0, a.depth_pred = depth_pred, a.depth_gt = depth_gt;
  a.occ = occupancy_gt, a.dyn = dynamic_gt, a.human = human_gt, a.gt_sum = depth_gt_sum;
  a.thresh = mask_pred_thresh, a.far = far, a.far08 = far08, a.flags = keep_all ? 0 : flags, a.keep_all = keep_all;
  a.H = (int)H, a.W = (int)W, a.e = erode, a.n = H * W;
  if (erode == 0) {
    hipLaunchKernelGGL(k_mono_mask_flat, mono_grid(a.n), dim3(MONO_BLOCK), 0, (hipStream_t)stream, a, out);
  } else {
    const dim3 grid((unsigned)((W + MONO_TILE - 1) / MONO_TILE), (unsigned)((H + MONO_TILE - 1) / MONO_TILE));
    if (grid.y > 65535u) return 2;
    hipLaunchKernelGGL(k_mono_mask_erode, grid, dim3(MONO_BLOCK), 0, (hipStream_t)stream, a, out);
  }
  NSIM_CHECK_LAUNCH();
  return 0;
}

static inline int ssi_args(SsiArgs* a, const NsimMonoSsi* cfg, const float* pred, const float* gt, const uint8_t* mask, int64_t H,
                           int64_t W) {
  if (!cfg) return 4;
  if (H < 1 || W < 1 || H * W > ((int64_t)1 << 30)) return 2;
  if (cfg->fn < 0 || cfg->fn > 7 || cfg->grad_reg_scales < 0 || cfg->grad_reg_scales > MONO_MAX_SCALES) return 58;
  if (!pred || !gt || !mask) return 4;
  a->pred = pred, a->gt = gt, a->mask = mask, a->H = (int)H, a->W = (int)W;
  a->fn = cfg->fn, a->param = cfg->fn_param, a->pre_scale = cfg->gt_pre_scale, a->pre_shift = cfg->gt_pre_shift;
  a->gt_to_pred = cfg->scale_gt_to_pred != 0, a->detach = cfg->detach_scale_shift != 0;
  a->n_scales = cfg->alpha_grad_reg != 0.0 ? cfg->grad_reg_scales : 0;
  a->w_depth = cfg->w / (double)(H * W);
  a->w_reg = a->n_scales ? cfg->w * cfg->alpha_grad_reg : 0.0;
  return 0;
}

int nsim_mono_ssi_moments(const NsimMonoSsi* cfg, const float* pred, const float* gt, const uint8_t* mask, int64_t H, int64_t W,
                          double* ws, void* stream) {
  SsiArgs a;
  if (int rc = ssi_args(&a, cfg, pred, gt, mask, H, W)) return rc;
  if (!ws) return 4;
  hipLaunchKernelGGL(k_ssi_moments, mono_grid(H * W), dim3(MONO_BLOCK), 0, (hipStream_t)stream, a, ws);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_mono_ssi_fwd(const NsimMonoSsi* cfg, const float* pred, const float* gt, const uint8_t* mask, int64_t H, int64_t W,
                      double* ws, float* out, float* g_depth, float* g_reg, void* stream) {
  SsiArgs a;
  if (int rc = ssi_args(&a, cfg, pred, gt, mask, H, W)) return rc;
  if (!ws || !out || !g_depth || !g_reg) return 4;
  hipLaunchKernelGGL(k_ssi_main, mono_grid(H * W), dim3(MONO_BLOCK), 0, (hipStream_t)stream, a, ws, out, g_depth, g_reg);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_mono_ssi_bwd(const NsimMonoSsi* cfg, const float* pred, const float* gt, const uint8_t* mask, int64_t H, int64_t W,
                      double* ws, const float* g_depth, const float* g_reg, const float* gout_depth, const float* gout_reg,
                      float* d_pred, void* stream) {
  SsiArgs a;
  if (int rc = ssi_args(&a, cfg, pred, gt, mask, H, W)) return rc;
  if (!ws || !g_depth || !g_reg || !d_pred) return 4;
  hipLaunchKernelGGL(k_ssi_bwd, mono_grid(H * W), dim3(MONO_BLOCK), 0, (hipStream_t)stream, a, ws, g_depth, g_reg, gout_depth,
                     gout_reg, d_pred);
  NSIM_CHECK_LAUNCH();
  return 0;
}

static inline int pearson_args(PearsonArgs* a, const float* pred, const float* gt, const uint8_t* mask, int64_t H, int64_t W,
                               double alpha_grad_reg, int grad_reg_scales, double w) {
  if (H < 1 || W < 1 || H * W > ((int64_t)1 << 30)) return 2;
  if (grad_reg_scales < 0 || grad_reg_scales > MONO_MAX_SCALES) return 58;
  if (!pred || !gt || !mask) return 4;
  a->pred = pred, a->gt = gt, a->mask = mask, a->H = (int)H, a->W = (int)W;
  a->n_scales = alpha_grad_reg != 0.0 ? grad_reg_scales : 0;
  a->w_depth = w, a->w_reg = w * alpha_grad_reg;
  return 0;
}

int nsim_mono_pearson_fwd(const float* pred, const float* gt, const uint8_t* mask, int64_t H, int64_t W, double alpha_grad_reg,
                          int grad_reg_scales, double w, double* ws, float* out, void* stream) {
  PearsonArgs a;
  if (int rc = pearson_args(&a, pred, gt, mask, H, W, alpha_grad_reg, grad_reg_scales, w)) return rc;
  if (!ws || !out) return 4;
  hipLaunchKernelGGL(k_pearson_fwd, mono_grid(H * W), dim3(MONO_BLOCK), 0, (hipStream_t)stream, a, ws, out);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_mono_pearson_bwd(const float* pred, const float* gt, const uint8_t* mask, int64_t H, int64_t W, double alpha_grad_reg,
                          int grad_reg_scales, double w, const double* ws, const float* gout_depth, const float* gout_reg,
                          float* d_pred, void* stream) {
  PearsonArgs a;
  if (int rc = pearson_args(&a, pred, gt, mask, H, W, alpha_grad_reg, grad_reg_scales, w)) return rc;
  if (!ws || !d_pred) return 4;
  hipLaunchKernelGGL(k_pearson_bwd, mono_grid(H * W), dim3(MONO_BLOCK), 0, (hipStream_t)stream, a, ws, gout_depth, gout_reg, d_pred);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_mono_normal_fwd(const float* normals_pred, const float* normals_gt, const uint8_t* mask, const float* rot, int rot_mode,
                         int64_t N, double w_l1, double w_cos, double* ws, float* out, float* g_l1, float* g_cos, void* stream) {
  if (N < 1) return 2;
  if (rot_mode < 0 || rot_mode > 2) return 58;
  if (!normals_pred || !normals_gt || (rot_mode && !rot) || !ws || !out || !g_l1 || !g_cos) return 4;
  hipLaunchKernelGGL(k_normal_cue_fwd, mono_grid(N), dim3(MONO_BLOCK), 0, (hipStream_t)stream, normals_pred, normals_gt, mask, rot,
                     rot_mode, N, w_l1, w_cos, ws, out, g_l1, g_cos);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_mono_scale2_bwd(const float* g0, const float* g1, int64_t n, const float* gout0, const float* gout1, float* d, void* stream) {
  if (n < 0) return 2;
  if (n == 0) return 0;
  if (!g0 || !g1 || !d) return 4;
  hipLaunchKernelGGL(k_mono_scale2, mono_grid(n), dim3(MONO_BLOCK), 0, (hipStream_t)stream, g0, g1, n, gout0, gout1, d);
  NSIM_CHECK_LAUNCH();
  return 0;
}

static inline int share_args(ShareArgs* a, const float* vw, const float* t, const float* rgb, const float* nablas,
                             const int64_t* pack_infos, const int64_t* rays_inds, int64_t P, int64_t N, int norm_depth, int norm_nablas) {
  if (P < 0 || N < 0) return 2;
  if (P && (!vw || !t || !pack_infos || !rays_inds)) return 4;
  a->vw = vw, a->t = t, a->rgb = rgb, a->nab = nablas, a->pack_infos = pack_infos, a->rays_inds = rays_inds;
  a->P = P, a->N = N, a->norm_depth = norm_depth != 0, a->norm_nablas = norm_nablas != 0;
  return 0;
}

int nsim_packed_share_fwd(const float* vw_in_total, const float* t, const float* rgb, const float* nablas, const int64_t* pack_infos,
                          const int64_t* rays_inds, int64_t P, int64_t N, int normalized_depth, int normalize_nablas, float* mask,
                          float* depth, float* rgb_out, float* normals_out, void* stream) {
  ShareArgs a;
  if (int rc = share_args(&a, vw_in_total, t, rgb, nablas, pack_infos, rays_inds, P, N, normalized_depth, normalize_nablas)) return rc;
  if (P == 0) return 0;
  if (!mask || !depth || (rgb && !rgb_out) || (nablas && !normals_out)) return 4;
  hipLaunchKernelGGL(k_packed_share_fwd, dim3(nsim_blocks(P, MONO_BLOCK / 64, 2048)), dim3(MONO_BLOCK), 0, (hipStream_t)stream, a, mask,
                     depth, rgb_out, normals_out);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_packed_share_bwd(const float* vw_in_total, const float* t, const float* rgb, const float* nablas, const int64_t* pack_infos,
                          const int64_t* rays_inds, int64_t P, int64_t N, int normalized_depth, int normalize_nablas, const float* mask,
                          const float* depth, const float* g_mask, const float* g_depth, const float* g_rgb, const float* g_normals,
                          float* d_vw, float* d_rgb, float* d_nablas, void* stream) {
  ShareArgs a;
  if (int rc = share_args(&a, vw_in_total, t, rgb, nablas, pack_infos, rays_inds, P, N, normalized_depth, normalize_nablas)) return rc;
  if (P == 0) return 0;
  if (!mask || !depth) return 4;
  hipLaunchKernelGGL(k_packed_share_bwd, dim3(nsim_blocks(P, MONO_BLOCK / 64, 2048)), dim3(MONO_BLOCK), 0, (hipStream_t)stream, a, mask,
                     depth, g_mask, g_depth, g_rgb, g_normals, d_vw, d_rgb, d_nablas);
  NSIM_CHECK_LAUNCH();
  return 0;
}

static inline int flow_loss_args(FlowLossArgs* a, const float* flow_fwd, const float* flow_fwd_pred_bwd, const float* flow_bwd,
                                 const float* flow_bwd_pred_fwd, int64_t S, double w_cycle, double w_sparsity) {
  if (S < 1 || S > ((int64_t)1 << 40)) return 2;
  if (!flow_fwd || !flow_fwd_pred_bwd || !flow_bwd || !flow_bwd_pred_fwd) return 4;
  a->ff = flow_fwd, a->fpb = flow_fwd_pred_bwd, a->fb = flow_bwd, a->bpf = flow_bwd_pred_fwd, a->S = S;
  a->s_cycle = w_cycle / (6.0 * (double)S), a->s_sparsity = w_sparsity / (4.0 * (double)S);
  return 0;
}

int nsim_flow_loss_fwd(const float* flow_fwd, const float* flow_fwd_pred_bwd, const float* flow_bwd, const float* flow_bwd_pred_fwd,
                       int64_t S, double w_cycle, double w_sparsity, double* ws, float* out, void* stream) {
  FlowLossArgs a;
  if (int rc = flow_loss_args(&a, flow_fwd, flow_fwd_pred_bwd, flow_bwd, flow_bwd_pred_fwd, S, w_cycle, w_sparsity)) return rc;
  if (!ws || !out) return 4;
  hipLaunchKernelGGL(k_flow_loss_fwd, mono_grid(S), dim3(MONO_BLOCK), 0, (hipStream_t)stream, a, ws, out);
  NSIM_CHECK_LAUNCH();
  return 0;
}

int nsim_flow_loss_bwd(const float* flow_fwd, const float* flow_fwd_pred_bwd, const float* flow_bwd, const float* flow_bwd_pred_fwd,
                       int64_t S, double w_cycle, double w_sparsity, const float* gout_cycle, const float* gout_sparsity,
                       float* d_flow_fwd, float* d_flow_fwd_pred_bwd, float* d_flow_bwd, float* d_flow_bwd_pred_fwd, void* stream) {
  FlowLossArgs a;
  if (int rc = flow_loss_args(&a, flow_fwd, flow_fwd_pred_bwd, flow_bwd, flow_bwd_pred_fwd, S, w_cycle, w_sparsity)) return rc;
  hipLaunchKernelGGL(k_flow_loss_bwd, mono_grid(S), dim3(MONO_BLOCK), 0, (hipStream_t)stream, a, gout_cycle, gout_sparsity, d_flow_fwd,
                     d_flow_fwd_pred_bwd, d_flow_bwd, d_flow_bwd_pred_fwd);
  NSIM_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
