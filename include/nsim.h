/* nsim.h -- C ABI of libnsim_hip.so, the MI355X (gfx950) implementation of the NeuS / StreetSurf
 * volume-render hot path of PJLab-ADG/neuralsim.
 *
 * The reference has no C/FFI plugin interface: its extension mechanism is Python class substitution
 * (``import_str(cfg.model_class)(**cfg.model_params)``, app/resources/asset_bank.py:129-138) and the
 * native work sits behind the Python API of the (un-vendored) nr3d_lib.  Every entry point below
 * therefore names the nr3d_lib Python symbol / reference call site whose native half it replaces; the
 * binding a maintainer adds is the ctypes stub shown in INTEGRATION.md (neuralsim_amd/_lib.py).
 *
 * Conventions:
 *   - plain pointers + sizes, no C++/torch types; all pointers are DEVICE pointers unless marked host;
 *   - never allocates, never synchronises; work is enqueued on ``stream`` (a hipStream_t);
 *   - returns 0 on success, a positive code otherwise (1000 + hipError_t for launch failures,
 *     1..99 for argument errors); nsim_strerror() explains argument errors;
 *   - "packed" arrays: ``pack_infos`` is int64 [P,2] = (first index, count) per ray
 *     (nr3d_lib.graphics.pack_ops.get_pack_infos_from_n; buffer_compose_renderer.py:991).
 */
#ifndef NSIM_H
#define NSIM_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NSIM_MAX_LEVELS 32
#define NSIM_LOTD_DENSE 0
#define NSIM_LOTD_HASH 1

/* LoTD level table (host struct, passed by pointer, copied by value into the launch).
 * nr3d_lib.models.grid_encodings.lotd ``lotd_cfg{lod_res, lod_n_feats, lod_types, hashmap_size}``
 * (code_single/configs/object_centric/lotd_neus.dtu.230814.yaml:96-101). n_feats is 2 for every level. */
typedef struct NsimLotdMeta {
  int32_t num_levels;
  int32_t n_feats;                     /* must be 2 */
  int32_t n_active_levels;             /* hardmask level annealing (encoding_cfg.anneal_cfg{type: hardmask},
                                        * lotd_neus.dtu.230814.yaml:104-108): levels >= n_active_levels yield zero
                                        * features and receive no gradient; 0 or >= num_levels = all active */
  int32_t res[NSIM_MAX_LEVELS][3];     /* vertices per axis (x, y, z); equal for cubic levels, per-axis for
                                        * ``lotd_use_cuboid`` (withmask_withlidar_joint.240219.yaml:160) */
  int32_t type[NSIM_MAX_LEVELS];       /* NSIM_LOTD_DENSE | NSIM_LOTD_HASH */
  uint32_t size[NSIM_MAX_LEVELS];      /* entries (vertices or hash slots) */
  int64_t offset[NSIM_MAX_LEVELS];     /* offset of the level in the flat param tensor, in scalars */
  float x_scale[3];                    /* position -> unit coordinate of the pyramid, per axis: u = x * x_scale + x_shift */
  float x_shift[3];                    /* = the model's AABB normalisation (nr3d_lib AABBSpace: lo -> 0, hi -> 1);
                                        * x_scale all zero = the [-1,1]^3 cube (0.5, 0.5) */
} NsimLotdMeta;

/* Occupancy-grid / AABB description (host struct). nr3d_lib.models.accelerations.OccGridAccel +
 * nr3d_lib.models.spatial.AABBSpace (``accel_cfg{type: occ_grid, resolution: [64,64,64]}``,
 * lotd_neus.dtu.230814.yaml:140-155). scale = res / (aabb_max - aabb_min). */
typedef struct NsimOccMeta {
  float aabb_min[3];
  float aabb_max[3];
  float scale[3];
  int32_t res[3];
} NsimOccMeta;

const char* nsim_strerror(int code);
int nsim_version(void);

/* ---------------------------------------------------------------- pack ops (graphics.pack_ops) */
/* get_pack_infos_from_n(n) ; total (device int64[1], may be NULL) receives sum(n).
 * cap < 0: plain.  cap >= 0: the caller sized its sample buffers for cap elements WITHOUT knowing sum(n); a pack
 * that would end beyond cap gets count 0 (its start is kept), so consumers stay in bounds; total still receives the
 * true sum and the caller redoes the pass when it later reads total > cap. */
int nsim_pack_infos_from_n(const int64_t* n, int64_t P, int64_t* pack_infos, int64_t* total, int64_t cap,
                           void* stream);
/* The same, and the kernel also stores (sum(n), seq) to ``notify`` [2] -- HOST-MAPPED pinned words (system-scope
 * stores, seq last with release order): the host polls notify[1] == seq and reads the size without a stream
 * synchronisation or a copy, so work queued behind this launch is not drained by the size read.  P > 0. */
int nsim_pack_infos_from_n_notify(const int64_t* n, int64_t P, int64_t* pack_infos, int64_t* total, int64_t cap,
                                  int64_t* notify, int64_t seq, void* stream);
/* ``ray_query_cfg.query_param.upsample_on_marched_only`` (the [R'] hit set of the reference's volume buffers,
 * single_volume_renderer.py:209-220,289-300: ``rays_inds_hit`` / ``pack_infos_hit`` cover the rays that produced samples): from
 * the occupancy-march counts n [R]: live_rank [R] = q >= 0 for the q-th ray with n > 0 ("live"), ~q < 0 for a ray with n == 0
 * (q live rays precede it); live_idx [R] (may be NULL) = the live rays in order, zero-filled past R'; cnts [8] (device) =
 * {R', sum(n) + R' C, R' nf0, R' nf1, R' nf2, R' nf3, sum(n), 0} -- the device-side point counts of the sampling pass's SDF
 * queries; notify (may be NULL): host-mapped words receiving (R', seq) as nsim_pack_infos_from_n_notify.  pack_infos [R,2]
 * (may be NULL) + total + cap + notify_total / seq_total: the outputs of nsim_pack_infos_from_n[_notify](n, cap) from the same
 * launch (the sampling pass needs both scans of the same counts). */
int nsim_live_rank(const int64_t* n, int64_t R, int C, int nf0, int nf1, int nf2, int nf3, int64_t* live_rank,
                   int64_t* live_idx, int64_t* cnts, int64_t* notify, int64_t seq, int64_t* pack_infos, int64_t* total,
                   int64_t cap, int64_t* notify_total, int64_t seq_total, void* stream);
/* packed_sum(x [S,C], pack_infos) -> out [P,C]   (single_volume_renderer.py:84-101) */
int nsim_packed_sum(const float* x, int C, const int64_t* pack_infos, int64_t P, float* out, void* stream);
/* out[s,c] = x[s,c] (op) per_pack[p, c or 0]; op 0 mul, 1 div, 2 add, 3 sub; x may be NULL (treated as 1 for
 * mul => broadcast, the backward of packed_sum).  packed_div: single_volume_renderer.py:86 */
int nsim_packed_binary(const float* x, int C, const float* per_pack, int Cp, const int64_t* pack_infos,
                       int64_t P, int op, float* out, void* stream);
/* packed_geq / packed_leq / packed_lt / packed_gt (op 0..3) -> uint8 mask (app/loss/lidar.py:102-110) */
int nsim_packed_cmp(const float* x, const float* per_pack, const int64_t* pack_infos, int64_t P, int op,
                    uint8_t* out, void* stream);
/* packed_matmul(x [S,3], rot [P,3,3]) : out[s] = rot[p] @ x[s] (transpose != 0: rot[p]^T @ x[s], the backward)
 * (app/renderers/utils.py:25) */
int nsim_packed_matmul3(const float* x, const float* rot, const int64_t* pack_infos, int64_t P,
                        int transpose, float* out, void* stream);
/* packed_sort(x, pack_infos) -> (sorted, GLOBAL indices)  (buffer_compose_renderer.py:1043-1047) */
int nsim_packed_sort(const float* x, const int64_t* pack_infos, int64_t P, float* sorted,
                     int64_t* indices, void* stream);
/* The collect + sort steps of BufferComposeRenderer.ray_query (code_multi/app/renderers/buffer_compose_renderer.py:648-695) in
 * one launch.  K <= 64 sources (the per-object volume buffers, in the reference's collect order); source k: depths t [S_k] in
 * packs ``pack_infos`` [P_k, 2] that live on the rays ``rays_inds`` [P_k] (ascending, one pack per ray: the reference's
 * ``rays_inds_collect`` / ``pack_infos_collect``).  total_pack_infos [N, 2]: (start, count) of every one of the N rays in the merged
 * buffer (count = the ray's samples over all sources; 0: no samples).  Outputs: t_sorted [S] -- every ray's samples ordered
 * by depth, ties in collect order (the reference's stable packed_sort of the concatenation) -- and, per source, dst [S_k]: the
 * position of each of its samples in that order (= ranks[pidx_in_total] of the reference's bookkeeping), so an attribute is
 * placed with ONE indexed store per source and an object's weights in the scene are vw[dst]. */
typedef struct NsimComposeSrc {
  const float* t;
  const int64_t* rays_inds;
  const int64_t* pack_infos;
  int64_t P;
  int64_t* dst;
} NsimComposeSrc;
int nsim_compose_collect_sort(const NsimComposeSrc* src, int32_t K, const int64_t* total_pack_infos, int64_t N,
                              float* t_sorted, void* stream);
/* The instance / class segmentation z-buffer of BufferComposeRenderer.ray_query(render_per_obj_individual=True)
 * (code_multi/app/renderers/buffer_compose_renderer.py:186-188 the three buffers, :268-311 a batched group, :427-450 and :549-572
 * a single model) for ALL drawable groups of a render in one call.  K <= 64 sources in the renderer's processing order; source
 * k: M candidates on the rays ``rays_inds`` [M] (the group's tested rays) with the object's INDIVIDUAL mask / depth -- pair form
 * (B == 0): ``mask`` / ``depth`` [M]; image form (B >= 1): ``mask`` / ``depth`` are [B, N] images read at (bidx[j], rays_inds[j]),
 * row 0 when bidx is NULL (a single model's [N] image) --,
 * the instance index per candidate (``ins`` [M]) or one for all (ins NULL: ins_scalar), and the class index.  Per ray: the
 * candidates are the entries with mask > threshold (strict) and depth < +inf (a NaN never wins; -0.0 counts as 0.0); the one of
 * smallest depth wins, among equal depths the earliest in processing order (source order, then position; the reference's strict
 * ``depth < z_buffer`` across groups -- inside a batched group its scatter_min leaves ties unspecified).  Outputs, written for every
 * ray: ins_seg / class_seg [N] (-1: no candidate) and z_buffer [N] (+inf: no candidate).  ``keys`` [N]: workspace of the caller,
 * initialised here when ordinal_base == 0.  More than 64 sources: further calls with the SAME keys and outputs and ordinal_base =
 * the candidates of the calls before (all ordinals < 2^32 - 1).  No host read, no synchronisation. */
typedef struct NsimSegSrc {
  const int64_t* rays_inds;
  int64_t M;
  const float* mask;
  const float* depth;
  const int64_t* bidx;
  int64_t B;
  const int64_t* ins;
  int64_t ins_scalar;
  int64_t class_ind;
} NsimSegSrc;
int nsim_seg_zbuffer(const NsimSegSrc* src, int32_t K, int64_t N, float threshold, int64_t ordinal_base, uint64_t* keys,
                     int64_t* ins_seg, int64_t* class_seg, float* z_buffer, void* stream);
/* interleave_linstep(start [P], n [P], step): pack_infos = get_pack_infos_from_n(n)  (buffer_compose_renderer.py:1036) */
int nsim_interleave_linstep(const int64_t* start, const int64_t* pack_infos, int64_t P, int64_t step,
                            int64_t* out, void* stream);
/* merge_two_packs_sorted (single_volume_renderer.py:341-344): packs of a / b live on rays slot_a / slot_b
 * (index into the union ray list, ascending); pack_infos_out [U,2] given (from the summed counts).
 * a-first on ties. */
int nsim_merge_two_packs(const float* va, const int64_t* pia, const int64_t* slot_a, int64_t Pa,
                         const float* vb, const int64_t* pib, const int64_t* slot_b, int64_t Pb,
                         const int64_t* pack_infos_out, int64_t U, int64_t* pidx_a, int64_t* pidx_b,
                         void* stream);

/* --------------------------------------------------------------- graphics.nerf / compositing */
/* packed_alpha_to_vw (single_volume_renderer.py:79-83): vw_i = alpha_i * prod_{j<i}(1-alpha_j+1e-10).
 * trans (may be NULL) receives the transmittance T_i, saved for the backward. */
int nsim_alpha_to_vw_fwd(const float* alpha, const int64_t* pack_infos, int64_t P, float* vw, float* trans,
                         void* stream);
int nsim_alpha_to_vw_bwd(const float* alpha, const float* trans, const float* vw, const float* dvw,
                         const int64_t* pack_infos, int64_t P, float* dalpha, void* stream);
/* The differentiable tail of a training step in ONE launch (no reference counterpart: the reference evaluates these with a
 * dozen torch / nr3d_lib calls -- ``_volume_integration`` app/renderers/single_volume_renderer.py:73-102, the photometric mse
 * app/loss/photometric.py:88-146, the eikonal term app/loss/eikonal.py:185-253 -- and autograd's backward of each): for the P
 * hit rays (packs ``pack_infos``, image row ``out_idx[p]`` or p) sdf -> alpha -> visibility weights -> mask / depth / rgb / normal
 * images; loss = mean((rgb image - gt)^2) over ALL N rays (rays outside the packs render black) + w_eikonal (mean over the S
 * render samples + mean over the M free points of (|nablas| - 1)^2); acc[0..2] += (mse, eikonal_render, eikonal_free) -- the mse
 * as a sum of squares only (e^2 of the pack rays + gt^2 of the others; out_idx must be ASCENDING: membership by search); and the
 * backward of all of it: dalpha [S], dsdf [S] (rows S.. are the caller's zeros), drgb [S,3], dnablas [S+M,3] (eikonal part
 * only), d_ln_inv_s += (may be NULL).  alpha / vw / trans [S] are written (the later backward launches read them). */
int nsim_render_head(const float* sdf, const float* ln_inv_s, float ln_inv_s_factor, float forward_inv_s, const float* t,
                     const float* rgb, const float* nablas, const int64_t* pack_infos, int64_t P, int normalized_depth,
                     const float* gt, int64_t N, int64_t S, int64_t M, float w_eikonal, const int64_t* out_idx, float* alpha,
                     float* vw, float* trans, float* mask, float* depth, float* rgb_out, float* nrm_out, float* acc,
                     float* dalpha, float* dsdf, float* drgb, float* dnablas, float* d_ln_inv_s, void* stream);
/* Fused SingleVolumeRenderer._volume_integration (single_volume_renderer.py:73-102): alpha -> vw -> mask,
 * depth (optionally normalised), rgb, normals per ray.  rgb / nrm (and their outputs) may be NULL.
 * out_idx [P] (may be NULL): row of the per-ray outputs that pack p writes / reads -- the scatter of the hit rays into
 * the all-rays images (``rendered[k][rays_inds_hit] = ...``, :88-101) fused into the same launch; the caller zeroes
 * the images. */
int nsim_composite_fwd(const float* alpha, const float* t, const float* rgb, const float* nrm,
                       const int64_t* pack_infos, int64_t P, int normalized_depth, float* vw, float* trans,
                       float* mask, float* depth, float* rgb_out, float* nrm_out, const int64_t* out_idx,
                       void* stream);
int nsim_composite_bwd(const float* alpha, const float* trans, const float* vw, const float* t,
                       const float* rgb, const float* nrm, const int64_t* pack_infos, int64_t P,
                       int normalized_depth, const float* mask, const float* depth, const float* dmask,
                       const float* ddepth, const float* drgb_out, const float* dnrm_out,
                       const float* dvw_ext, float* dalpha, float* drgb, float* dnrm, const int64_t* out_idx,
                       void* stream);
/* NeuS sdf -> opacity (NeusRendererMixin): alpha_i for interval (i,i+1), 0 at the
 * last sample of each pack.  inv_s = exp(ln_inv_s[0] * ln_inv_s_factor) unless forward_inv_s > 0. */
int nsim_neus_alpha_fwd(const float* sdf, const int64_t* pack_infos, int64_t P, const float* ln_inv_s,
                        float ln_inv_s_factor, float forward_inv_s, float* alpha, void* stream);
int nsim_neus_alpha_bwd(const float* sdf, const float* dalpha, const int64_t* pack_infos, int64_t P,
                        const float* ln_inv_s, float ln_inv_s_factor, float forward_inv_s, float* dsdf,
                        float* d_ln_inv_s, void* stream);
/* nsim_neus_alpha_fwd + nsim_composite_fwd in one launch (identical arithmetic; alpha [S] is written for the
 * backward passes above). */
int nsim_neus_composite_fwd(const float* sdf, const float* ln_inv_s, float ln_inv_s_factor, float forward_inv_s,
                            const float* t, const float* rgb, const float* nrm, const int64_t* pack_infos, int64_t P,
                            int normalized_depth, float* alpha, float* vw, float* trans, float* mask, float* depth,
                            float* rgb_out, float* nrm_out, const int64_t* out_idx, void* stream);

/* ------------------------------------------------------------------------------ ray generation */
/* Camera._get_selected_rays_from_ixy (app/resources/observers/cameras.py:281-310) */
int nsim_raygen_pinhole(const float* xy, const int64_t* fidx, const float* intr /*[V,3,3]*/,
                        const float* c2w /*[V,4,4]*/, const int64_t* WH /*[V,2]*/, int64_t N, int snap,
                        float* rays_o, float* rays_d, void* stream);
/* Its backward w.r.t. the poses (pose refinement, LearnableParams -> refined c2w,
 * withmask_withlidar_joint.240219.yaml:338-352): d_c2w [V,4,4] (initialised by the caller) += the gradients of
 * rays_o = T and rays_d = R l / |R l|; d_rays_o / d_rays_d [N,3] may each be NULL. */
int nsim_raygen_pinhole_bwd(const float* xy, const int64_t* fidx, const float* intr, const float* c2w,
                            const int64_t* WH, int64_t N, int snap, const float* d_rays_o, const float* d_rays_d,
                            float* d_c2w, void* stream);
/* The same two with the OpenCV camera model (``camera_model: opencv`` -> ``OpenCVCameraMatHW.lift``,
 * app/resources/observers/cameras.py:84-87; the street configs' ``consider_distortion: true``,
 * withmask_withlidar_joint.240219.yaml:141, Waymo calibration (k1, k2, p1, p2, k3),
 * dataio/autonomous_driving/waymo/preprocess.py:172): distortion [V,5]; the undistorted direction comes from n_iters
 * rounds of the fixed-point iteration of cv::undistortPoints (5 there).  Implementation in the absent nr3d_lib:
 * semantics fixed here. */
int nsim_raygen_opencv(const float* xy, const int64_t* fidx, const float* intr, const float* distortion /*[V,5]*/,
                       int n_iters, const float* c2w, const int64_t* WH, int64_t N, int snap, float* rays_o,
                       float* rays_d, void* stream);
int nsim_raygen_opencv_bwd(const float* xy, const int64_t* fidx, const float* intr, const float* distortion, int n_iters,
                           const float* c2w, const int64_t* WH, int64_t N, int snap, const float* d_rays_o,
                           const float* d_rays_d, float* d_c2w, void* stream);
/* ... and with the fisheye camera model (``camera_model: fisheye`` -> ``FisheyeCameraMatHW.lift``,
 * app/resources/observers/cameras.py:88-92; dataio/autonomous_driving/custom/custom_autodrive_dataset.py:512,581): the
 * OpenCV fisheye (Kannala-Brandt equidistant) model theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8)
 * the reference applies in app/resources/observers/fisheye.py:36-42; distortion [V,4]; theta from n_iters Newton rounds
 * (cv::fisheye::undistortPoints runs 10), direction (sin theta x_d / theta_d, sin theta y_d / theta_d, cos theta).
 * Implementation in the absent nr3d_lib: semantics fixed here. */
int nsim_raygen_fisheye(const float* xy, const int64_t* fidx, const float* intr, const float* distortion /*[V,4]*/,
                        int n_iters, const float* c2w, const int64_t* WH, int64_t N, int snap, float* rays_o,
                        float* rays_d, void* stream);
int nsim_raygen_fisheye_bwd(const float* xy, const int64_t* fidx, const float* intr, const float* distortion, int n_iters,
                            const float* c2w, const int64_t* WH, int64_t N, int snap, const float* d_rays_o,
                            const float* d_rays_d, float* d_c2w, void* stream);
/* AABBSpace.ray_test (call site single_volume_renderer.py:235-238): far < 0 means "no far". */
int nsim_aabb_ray_test(const float* rays_o, const float* rays_d, int64_t N, const NsimOccMeta* meta,
                       float near, float far, float* near_out, float* far_out, uint8_t* hit, void* stream);

/* ------------------------------------------------------------------------ occupancy + sampling */
/* OccGridEma update (lotd_neus.dtu.230814.yaml:140-155): val = max(val*decay, 4 sig(s sdf)(1-sig)) */
int nsim_occ_decay(float* val, int64_t nvox, float decay, void* stream);
int nsim_occ_update(float* val, const float* pts, const float* sdf, int64_t n, const NsimOccMeta* meta,
                    float inv_s, void* stream);
int nsim_occ_pack_bits(const float* val, int64_t nvox, float thre, uint32_t* bits, void* stream);
/* ``accel_cfg.update_from_samples_cfg: {}`` (lotd_neus.dtu.230814.yaml:158; hook app/resources/asset_bank.py:291-298): the
 * SDFs the sampling pass of a training step computes anyway are max-folded into the value grid (no decay: the periodic
 * refresh decays and re-thresholds).  n_dev (may be NULL): valid points = min(n, *n_dev + n_add), 0 if that exceeds n. */
int nsim_occ_collect(float* val, const float* pts, const float* sdf, int64_t n, const int64_t* n_dev, int64_t n_add,
                     const NsimOccMeta* meta, float inv_s, void* stream);
/* OccGridAccel.ray_march (march_cfg{step_size,max_steps}): lattice t_k = near + (k + jitter) * step.
 * ray_word_off (may be NULL): batched occupancy grid (``accel_cfg{type: occ_grid_batched}``,
 * code_multi/.../no_fg_occ.221218.yaml:369-377) -- offset in 32-bit words of ray r's instance inside ``bits``. */
int nsim_march_count(const float* rays_o, const float* rays_d, const float* near, const float* far,
                     const float* jitter, int64_t R, const uint32_t* bits, const int64_t* ray_word_off,
                     const NsimOccMeta* meta, float step, int max_steps, int64_t* counts, void* stream);
int nsim_march_emit(const float* rays_o, const float* rays_d, const float* near, const float* far,
                    const float* jitter, int64_t R, const uint32_t* bits, const int64_t* ray_word_off,
                    const NsimOccMeta* meta, float step, int max_steps, const int64_t* pack_infos, float* t_out,
                    void* stream);
/* coarse_step_cfg{step_mode: linear}: t = near + (far-near) * ((i + u)/C); jitter_c NULL => u = 0.5 */
/* live_rank (here and in the three entry points below; may be NULL = every ray is live, dense [R, n] layout): the ranks of
 * nsim_live_rank -- only live rays get samples, and every per-live-ray array (out here; t_b / v_b, t_new, x_new below) is
 * indexed by the rank q instead of r, i.e. holds R' n compact entries. */
int nsim_coarse_depths(const float* near, const float* far, const float* jitter_c, int64_t R, int C,
                       float* out, const int64_t* live_rank, void* stream);
/* One NeuS up-sampling stage (num_fine[i], upsample_inv_s * factor[i], upsample_use_estimate_alpha).
 * scratch: float [S]. t_new: [R, n_fine] ascending.  x_new [R, n_fine, 3] (may be NULL; needs rays_o / rays_d [R,3]):
 * positions o + t d of the new samples, so that the level-major query reads 12 B per point instead of re-deriving
 * the point from (ridx, t, o, d) once per XCD. */
int nsim_upsample_stage(const float* t, const float* sdf, const int64_t* pack_infos, int64_t R, float inv_s,
                        int n_fine, int use_estimate_alpha, float* scratch, float* t_new, const float* rays_o,
                        const float* rays_d, float* x_new, const int64_t* live_rank, void* stream);
/* Sorted merge of packed (t_a, v_a) with batched (t_b, v_b) [R,nb]; packs must tile the arrays in order.
 * v_a / v_b / v_out may be NULL. pack_infos_out [R,2] is written; ridx_out [S_out] (may be NULL) receives the
 * ray (pack) index of every merged sample; x_out [S_out, 3] (may be NULL; needs rays_o / rays_d) their positions. */
int nsim_merge_sorted(const float* t_a, const float* v_a, const int64_t* pack_infos_a, const float* t_b,
                      const float* v_b, int64_t R, int nb, float* t_out, float* v_out,
                      int64_t* pack_infos_out, int64_t* ridx_out, const float* rays_o, const float* rays_d,
                      float* x_out, const int64_t* live_rank, void* stream);
/* nsim_merge_sorted of up-sampling stage k followed, in the same launch, by nsim_upsample_stage of stage k + 1 on the merged
 * samples (both one wave per ray; v_a / v_b / v_out = the no-grad SDFs, required): t_new [R, n_fine] (+ x_new) are the next
 * stage's draws; scratch [>= merged sample count] as nsim_upsample_stage.  Same values as the two calls. */
int nsim_merge_upsample(const float* t_a, const float* v_a, const int64_t* pack_infos_a, const float* t_b, const float* v_b,
                        int64_t R, int nb, float* t_out, float* v_out, int64_t* pack_infos_out, int64_t* ridx_out, float inv_s,
                        int n_fine, int use_estimate_alpha, float* scratch, float* t_new, const float* rays_o,
                        const float* rays_d, float* x_new, const int64_t* live_rank, void* stream);

/* ``query_mode: march_occ_multi_upsample_compressed`` (lotd_neus.dtu.230814.yaml:157): from the no-grad SDF of all
 * samples keep those that bound an interval with visibility weight > thre.  count -> counts [R]; emit (given
 * pack_infos_out from the counts) -> compacted t_out / ridx_out; emit also appends ``tail_n`` (>= 0) zero-depth samples
 * on the pseudo-rays R .. R+tail_n-1 behind the kept set (the free eikonal points of the with-grad query), so
 * t_out / ridx_out hold total + tail_n entries. */
int nsim_compress_count(const float* sdf, const int64_t* pack_infos, int64_t R, const float* ln_inv_s,
                        float ln_inv_s_factor, float forward_inv_s, float thre, int64_t* counts, void* stream);
int nsim_compress_emit(const float* sdf, const float* t, const int64_t* pack_infos, int64_t R, const float* ln_inv_s,
                       float ln_inv_s_factor, float forward_inv_s, float thre, const int64_t* pack_infos_out,
                       float* t_out, int64_t* ridx_out, int64_t tail_n, void* stream);

/* ------------------------------------------------------------------- LoTD encoding (standalone) */
/* LoTDEncoding.forward / forward_dydx (inspect_rendering.py:468-474): x [S,3] in [-1,1], grid fp16.
 * out f32 [S, L*2]; dydx (may be NULL) f32 [S, L*2, 3] = d out / d x. */
int nsim_lotd_fwd(const float* x, const void* grid_f16, const NsimLotdMeta* meta, int64_t S, float* out,
                  float* dydx, void* stream);
/* LoTD backward: dgrid (f32 [n_params], accumulated with atomics) += d L/d out . d out/d grid
 *   + (if dL_ddydx != NULL) d L / d dydx . d dydx / d grid  (the second-order path used by nablas). */
int nsim_lotd_bwd(const float* x, const float* dL_dout, const float* dL_ddydx, const NsimLotdMeta* meta,
                  int64_t S, float* dgrid, void* stream);

/* ------------------------------------------------------- permutohedral-lattice encoding */
/* nr3d_lib.models.grid_encodings.permuto.PermutoEncoding(in_dim, permuto_auto_compute_cfg{type: multi_res, coarsest_res,
 * finest_res, n_levels, n_feats, log2_hashmap_size, apply_random_shifts_per_level}) -- call sites
 * app/models/single/neus.py:64-76 (PermutoNeuSObj), docs/exps/exp_permuto_3d_modulated.py:52-60,
 * code_multi/configs/exps/fg_neus=permuto/all_occ.240201.yaml:438-446.  The implementation is in the absent nr3d_lib; the
 * kernels follow the published algorithm (Adams et al. 2010, Rosu & Behnke 2023) as restated in oracle/permuto.py:
 * level l: cf_i = (x_i + shift[l][i]) * scale[l][i] with scale[l][i] = res_l / sqrt((i+1)(i+2)), elevation, nearest
 * remainder-0 point, ranks, barycentric weights of the in_dim + 1 simplex vertices, vertex hash
 * k <- (k + key_i) * 2531011 (uint32) over the first in_dim key coordinates, modulo hashmap_size.
 * Table: fp16, level l at [l * hashmap_size * 2, (l+1) * hashmap_size * 2), two features per entry. */
typedef struct NsimPermutoMeta {
  int32_t in_dim;                      /* 2..8 (3 = positions; 3 + k = positions with a k-dim condition concatenated) */
  int32_t num_levels;                  /* 1..32 */
  int32_t n_feats;                     /* must be 2 */
  uint32_t hashmap_size;               /* entries per level, a power of two */
  float scale[NSIM_MAX_LEVELS][8];
  float shift[NSIM_MAX_LEVELS][8];     /* ``apply_random_shifts_per_level`` (zeros when off) */
  int32_t n_active_levels;             /* hardmask level annealing (encoding_cfg.anneal_cfg{type: hardmask},
                                        * permuto_neus.bmvs.230814.yaml:118-122 and :212-216), as NsimLotdMeta: levels
                                        * >= n_active_levels yield zero features, zero d features / d x, no gradient and
                                        * no memory access to their tables; 0 or >= num_levels = all levels */
} NsimPermutoMeta;
/* PermutoEncoding.forward / forward_dydx: x [S,in_dim] -> out f32 [S, L*2]; dydx (may be NULL) f32 [S, L*2, in_dim]. */
int nsim_permuto_fwd(const NsimPermutoMeta* meta, const void* grid_f16, const float* x, int64_t S, float* out, float* dydx,
                     void* stream);
/* backward w.r.t. the table: dgrid (f32 [L * hashmap_size * 2], accumulated with atomics) += dL/dout . dout/dgrid.
 * (dL/dx = sum dL/dout . dydx is a host-side contraction of the forward's dydx.) */
int nsim_permuto_bwd(const NsimPermutoMeta* meta, const float* x, int64_t S, const float* dL_dout, float* dgrid,
                     void* stream);
/* The NeuS field's front end (PermutoNeuSObj; GenerativePermutoConcat with z): positions x [S,3] or rays
 * (rays_o, rays_d [R,3], t [S], ridx [S]); z [R, in_dim - 3] (may be NULL = zeros; needs ridx) is the per-ray condition
 * concatenated to the position.  Writes LEVEL-MAJOR planes in the layout of nsim_lotd_gather_lm / nsim_field_fwd, so
 * that nsim_field_sdf (feat_planes) and nsim_field_fwd / _bwd_sdf (h_planes, J_planes; pass grid_f16 = NULL there: "the
 * planes are already gathered") run unchanged on a permutohedral model: exactly one of
 *   feat_planes [NL][P] (f16x2 scaled by 1024 when feat_f32 = 0, f32x2 when 1)      -- no-grad query, or
 *   h_planes [NL][P][2] + J_planes [NL][P][2][3], P = NSIM_PLANE_PITCH(S)            -- with-grad query; J_planes in the
 *       element type the decoders' meta asks for (nsim_jplane_elem_bytes): feat_f32 = 0 writes f16 (2 bytes), 1 writes f32
 * (NL = 16 for <= 16 levels, else 32; levels past num_levels are not written).  n_dev / n_add as nsim_lotd_gather_lm. */
int nsim_permuto_gather(const NsimPermutoMeta* meta, const void* grid_f16, const float* x, const float* rays_o,
                        const float* rays_d, const float* t, const int64_t* ridx, const float* z, int64_t S,
                        const int64_t* n_dev, int64_t n_add, void* feat_planes, int feat_f32, float* h_planes,
                        void* J_planes, void* stream);
/* Backward to the table from the decoders' hand-off planes (nsim_field_bwd_sdf): dgrid[v][f] += w_v dL/dh[f]
 * + g[f] (dw_v/dx . gn)  -- gn [S,3] (may be NULL, then g_planes may be NULL too) is the total dL/dnablas; the weights
 * are piecewise linear in x, so this is the whole second-order term. */
int nsim_permuto_scatter(const NsimPermutoMeta* meta, const float* x, const float* rays_o, const float* rays_d,
                         const float* t, const int64_t* ridx, const float* z, int64_t S, const float* dh_planes,
                         const float* g_planes, const float* gn, float* dgrid, void* stream);
/* Backward to the CONDITION of a conditioned field (in_dim > 3; GenerativePermutoConcat's learned per-instance codes,
 * app/models/shared/batched_neus.py:295-407 ``z_ins_all``): dz[ray][c] += sum over the ray's samples, levels and features of
 * dL/dh . dh/dz_c (dz [R, in_dim - 3], caller-zeroed; z and ridx required).  The normals carry no z term: dh/dx is constant
 * inside a simplex. */
int nsim_permuto_dz(const NsimPermutoMeta* meta, const void* grid_f16, const float* x, const float* rays_o,
                    const float* rays_d, const float* t, const int64_t* ridx, const float* z, int64_t S,
                    const float* dh_planes, float* dz, void* stream);
/* Point-mode front end for decoders without normals (PermutoNeRFDistant: the NeRF++ background on a 4-D lattice):
 * x [S,in_dim] carries every input per point (in_dim 2..8, num_levels <= 16).  Writes ONLY h_planes [16][S][2] f32,
 * level-major with pitch S -- the layout nsim_distant_fwd_planes / nsim_distant_bwd read -- all 16 rows (zeros for masked
 * levels and past the pyramid); no d features / d x. */
int nsim_permuto_gather_pts(const NsimPermutoMeta* meta, const void* grid_f16, const float* x, int64_t S, float* h_planes,
                            void* stream);
/* ... and its backward to the table: dgrid[v][f] += w_v dh_planes[l][s][f] over the in_dim + 1 vertices per level of the
 * points with valid[s] != 0 (the others are skipped before the simplex; their dh rows are never read). */
int nsim_permuto_scatter_pts(const NsimPermutoMeta* meta, const float* x, const uint8_t* valid, int64_t S,
                             const float* dh_planes, float* dgrid, void* stream);
/* ... and its backward to the POINTS, for callers whose lattice points are network outputs (positions warped by a predicted
 * scene flow, EmerNeRF's flow field): dx[s][c] = sum over the active levels and the features of dh_planes[l][s][f] . dh[l][f] /
 * dx_c for ALL in_dim inputs (inside a simplex the features are affine in x: the derivative of the barycentric weights times the
 * vertex features).  dh_planes [16][plane_pitch][2] (plane_pitch 0 = S; a caller that gathered several point sets into one buffer
 * passes the set's first row and the buffer's pitch), dx [S,in_dim] is WRITTEN (one writer per row, no atomics, need not be
 * zeroed).  valid [S] or NULL (every point): a cleared point gets a zero row, none of its dh rows or table entries is read.
 * Masked levels (n_active_levels) contribute nothing and their tables are not read. */
int nsim_permuto_dx_pts(const NsimPermutoMeta* meta, const void* grid_f16, const float* x, const uint8_t* valid, int64_t S,
                        const float* dh_planes, int64_t plane_pitch, float* dx, void* stream);

/* ------------------------------------------------------- fused NeuS field (LoTD + MLPs, MFMA) */
/* Network description (host struct).  LoTDNeuSModel = LoTDSDF + RadianceNet
 * (app/models/single/neus.py:24-62; lotd_neus.dtu.230814.yaml:92-139). */
typedef struct NsimFieldMeta {
  NsimLotdMeta lotd;     /* 1..32 levels x 2 feats (<= 64 input features; W1 is [64 x 2 num_levels]); more than 16
                          * levels: level-major planes of 32 levels, the planes arguments are then mandatory */
  int32_t sdf_D;         /* hidden layers of the SDF decoder: 1 or 2 (width 64, softplus beta) */
  int32_t precision;     /* 0: fp16 MFMA (v_mfma_f32_32x32x16_f16), 1: exact f32 MFMA (32x32x2 f32) */
  float softplus_beta;   /* 100; a negative value selects relu (decoder_cfg.activation: relu) */
  int32_t embed_E;       /* width of the embedded-position block appended to the SDF decoder's input: 0 = none, else
                          * 3 + 6 n_frequencies <= 63 (``surface_cfg.extra_pos_embed_cfg{type: sinusoidal_legacy}`` of the
                          * StyleLoTD Vehicle block, code_multi/configs/exps/fg_neus=hyper_lotd/no_fg_occ.221218.yaml:319-321).
                          * W1 is then [64 x (2 num_levels + embed_E)] and the packed first-layer matrices carry two more
                          * 32-input MFMA chunks; nsim_field_fwd (level-major path) and nsim_wide_bwd_sdf read it */
} NsimFieldMeta;

/* size in bytes of the packed-fragment weight buffer for a given meta */
int64_t nsim_field_wpack_bytes(const NsimFieldMeta* meta);
/* Re-pack f32 master weights into MFMA A-fragment order (once per optimizer step).
 * sdf_w: [W1 (64 x 2 num_levels), (W2 (64x64)), Wout (1x64)] concatenated row-major; sdf_b likewise [64,(64),1];
 * rad_w: [Wr1 (64x26), Wr2 (64x64), Wr3 (3x64)], rad_b [64,64,3]. */
int nsim_field_pack_weights(const NsimFieldMeta* meta, const float* sdf_w, const float* sdf_b,
                            const float* rad_w, const float* rad_b, void* wpack, void* stream);
/* Two packs of the same master weights in ONE launch (a model whose sampling pass runs at another precision than its field
 * keeps two: every optimizer step re-packs both). */
int nsim_field_pack_weights2(const NsimFieldMeta* meta_a, void* wpack_a, const NsimFieldMeta* meta_b, void* wpack_b,
                             const float* sdf_w, const float* sdf_b, const float* rad_w, const float* rad_b, void* stream);
/* No-grad SDF query (model.query_sdf / forward_sdf; inspect_rendering.py:120-128).
 * Points are x[s] (if x != NULL) or rays_o[ridx[s]] + t[s] * rays_d[ridx[s]].
 * feat_planes == NULL: one fused point-major kernel (gather + decoder).
 * feat_planes != NULL: decoder only, on the level-major feature planes written by nsim_lotd_gather_lm for the same
 * points (x / rays / grid are then unused and may be NULL).  Same values either way.
 * Speculatively sized buffers (level-major path): S is the CAPACITY (the plane pitch is NSIM_PLANE_PITCH(S)); when n_dev != NULL the
 * number of valid points is *n_dev + n_add, read on the device (0 if that exceeds S: the caller under-sized its
 * buffers and redoes the pass) -- the host never learns the size of the marched sample set before launching its
 * first query (one host sync less per step).
 * occ_val != NULL (needs x and occ_meta): the SDFs are also folded into the occupancy value grid in the same launch --
 * nsim_occ_collect's update (``update_from_samples_cfg``) without a pass of its own. */
int nsim_field_sdf(const NsimFieldMeta* meta, const void* grid_f16, const void* wpack, const float* x,
                   const float* rays_o, const float* rays_d, const float* t, const int64_t* ridx,
                   const int64_t* ray_goff, int64_t S, const int64_t* n_dev, int64_t n_add, float* sdf,
                   const void* feat_planes, float* occ_val, const NsimOccMeta* occ_meta, float occ_inv_s, void* stream);
/* Sphere tracing of R rays against the SDF (``query_mode: sphere_trace`` + ``model.tracer.trace``: the library's
 * csrc/sphere_trace extension behind app/visualizer/gui_runner_single_cuboid.py:76-104 and
 * code_single/tools/inspect_rendering.py:71-73,262-287; its source is absent, the semantics are fixed in DESIGN sec. 7).
 * One persistent launch; the SDF is the fused point-major query of nsim_field_sdf (same meta / grid / weight pack, <= 16
 * levels), empty space is skipped on the marching lattice of nsim_march_* with jitter 0 (bits / meta / step / max_steps as
 * there).  Per ray, from t = near: [skip to the next occupied lattice point, OUT if none] -> s = sdf(o + t d), n_steps += 1
 * -> HIT if s <= hit_threshold -> t += max(distance_scale s, min_step) -> OUT if t > far -> ALIVE if n_steps == max_iters.
 * Outputs by ray: status (0 ALIVE, 1 HIT, 2 OUT; inspect_rendering.py:285), n_steps, and (t_out, sdf_out) = depth and value of
 * the ray's LAST query -- the hit point of a HIT ray; (near, NaN) for a ray that never queried.  Results do not depend on
 * the schedule.  workspace: nsim_sphere_trace_workspace_bytes() bytes of device memory, contents irrelevant (the ray cursor). */
int64_t nsim_sphere_trace_workspace_bytes(void);
int nsim_sphere_trace(const NsimFieldMeta* meta, const void* grid_f16, const void* wpack, const float* rays_o,
                      const float* rays_d, const float* near, const float* far, int64_t R, const uint32_t* occ_bits,
                      const NsimOccMeta* occ_meta, float march_step, int max_steps, float distance_scale, float min_step,
                      float hit_threshold, int max_iters, float* t_out, float* sdf_out, uint8_t* status_out,
                      int32_t* n_steps_out, void* workspace, void* stream);
/* Level-major LoTD gather of the no-grad query (the encoding half of forward_sdf): feat_planes [NLP][P] (NLP = 16 for <= 16 levels, 32 above;
 * P = NSIM_PLANE_PITCH(S): a 32-point tile of a level is one aligned 128 B | 256 B piece, which nsim_field_sdf copies
 * straight into LDS, global_load_lds_dwordx4, one tile ahead) of
 * (fp16 x 2, pre-scaled for the fp16 MFMA decoder | f32 x 2) = NLP * P * (4 | 8) bytes, caller-owned.  Every wave
 * walks the levels in one order and the levels are dealt to the XCDs, so a level's table is read through ONE L2. */
int nsim_lotd_gather_lm(const NsimFieldMeta* meta, const void* grid_f16, const float* x, const float* rays_o,
                        const float* rays_d, const float* t, const int64_t* ridx, const int64_t* ray_goff, int64_t S,
                        const int64_t* n_dev, int64_t n_add, void* feat_planes, void* stream);
/* Batched / multi-instance models (``batched_ray_query`` + ``set_condition``,
 * app/renderers/buffer_compose_renderer.py:222-265, app/models/shared/batched_neus.py:380-407): the tables of all
 * instances live in ONE flat tensor and ``ray_goff[r]`` (may be NULL) is the offset, in scalars (even), of ray r's
 * instance; every kernel that touches the table takes it next to ``ridx`` (required then, also with ``x``).
 *
 * With-grad query: forward_sdf_nablas + radiance. v: view dirs per sample taken from
 * rays_d[ridx]; h_appear [R,4] per ray (may be NULL => zeros). Outputs sdf [S], nablas [S,3], rgb [S,3]
 * (rgb may be NULL: with_rgb=False, code_single/tools/train.py:896-902).
 * h_planes [NLP,P,2] (f32) / J_planes [NLP,P,2,3] (f16 | f32: nsim_jplane_elem_bytes) with the pitch P = NSIM_PLANE_PITCH(S) = S rounded up to 32 -- every 32-point
 * tile of a level is then one 16-byte-aligned 256 B / 768 B piece, which the decoder kernels prefetch straight into LDS
 * (global_load_lds_dwordx4) -- (both or neither; NLP = 16 for <= 16 levels, 32 above): when given, the gathered features and their
 * derivative w.r.t. x are saved level-major for the backward launches (which then never gather again).
 * n_dev (may be NULL; needs the planes): the launch is sized for a CAPACITY S while the number of valid points,
 * n_dev[0] + n_add <= S, is read on the device -- the training step queues this launch before the host has read the
 * size of the kept sample set (a count above the capacity touches nothing; the caller redoes the launch).
 * wpack == NULL (needs grid_f16 and the planes): GATHER ONLY -- the planes are written, no decoder runs (the caller's
 * decoder is another one: nsim_wide_fwd); sdf / nablas / rgb are then unused. */
#define NSIM_PLANE_PITCH(S) ((((int64_t)(S)) + 31) & ~(int64_t)31)
int nsim_field_fwd(const NsimFieldMeta* meta, const void* grid_f16, const void* wpack, const float* x,
                   const float* rays_o, const float* rays_d, const float* t, const int64_t* ridx,
                   const int64_t* ray_goff, const float* h_appear, int64_t S, float* sdf, float* nablas, float* rgb,
                   float* h_planes, void* J_planes, const int64_t* n_dev, int64_t n_add, void* stream);
/* Element size of the dh/dx planes (J_planes) for this meta: 2 (f16: the fp16 field mode -- 192 B per point instead of 384,
 * the dominant plane traffic of the with-grad gather and of the two decoders that read them) or 4 (f32: the f32 mode).
 * J_planes holds NLP * P * 6 such elements. */
int nsim_jplane_elem_bytes(const NsimFieldMeta* meta);
/* Optional scratch for the weight-gradient flush of the backward launches (1) and (2) below.  Every workgroup of those
 * launches ends by adding its partial dW / db into the same few thousand floats; hundreds of same-address atomics per
 * address serialise in L2 (measured: ~55 us of a 100 us radiance backward).  With a caller-owned, ZEROED buffer of
 * ``floats`` floats registered for (the calling thread's current device, ``stream``) (>= 16 x 8448 covers every decoder shape), workgroup b adds into replica
 * b % 16 of it and a small second launch folds the replicas into dW / db and zeroes the buffer again: the buffer is zero
 * whenever no launch of that stream is in flight.  buf = NULL unregisters.  Without a registration (or with
 * NSIM_GRAD_REPLICAS=1) the launches add into dW / db directly, as before.  The reference has no counterpart: its
 * autograd backward of the tcnn-style MLP reduces weight gradients inside one GEMM. */
int nsim_set_grad_scratch(float* buf, int64_t floats, void* stream);
/* Backward of nsim_field_fwd = three launches (each its own entry point so that callers can time / overlap them):
 *
 * (1) radiance branch: given dL/drgb [S,3], the saved forward nablas_fwd / rgb_fwd [S,3] and the upstream
 *     dL/dnablas (may be NULL): accumulates drad_w / drad_b (layouts of nsim_field_pack_weights), dh_appear [R,4]
 *     (may be NULL) and writes gn_out [S,3] = dL/dnablas + d(radiance)/d nablas.
 *     Pose refinement (LearnableParams, withmask_withlidar_joint.240219.yaml:338-352 -- the rays carry gradients):
 *     dx [S,3] (may be NULL) is SET to the radiance net's gradient w.r.t. the sample position, dv [S,3] (may be
 *     NULL) to its gradient w.r.t. the view direction (through SH-4). */
int nsim_field_bwd_rad(const NsimFieldMeta* meta, const void* wpack, const float* nablas_fwd, const float* rgb_fwd,
                       const float* x, const float* rays_o, const float* rays_d, const float* t, const int64_t* ridx,
                       const float* h_appear, int64_t S, const float* dnablas, const float* drgb, float* gn_out,
                       float* drad_w, float* drad_b, float* dh_appear, float* dx, float* dv, void* stream);
/* (2) SDF-decoder branch on the saved h / J planes: given dL/dsdf [S] and the total dL/dnablas gn [S,3] (either may
 *     be NULL) accumulates dsdf_w / dsdf_b -- including the double-backward terms of nablas w.r.t. the decoder
 *     weights (app/loss/eikonal.py:216-251) -- and writes the hand-off planes dh_planes = dL/dh and
 *     g_planes = d sdf/d h, both [NLP,S,2] (both or neither).  dx [S,3] (may be NULL; initialised by the caller or
 *     by (1)) += (dh/dx)^T dL/dh, the first-order position gradient (LoTD ``dL/dx``).
 *     plane_pitch: pitch of h_planes / J_planes when the forward ran at a capacity above S (0 = NSIM_PLANE_PITCH(S)). */
int nsim_field_bwd_sdf(const NsimFieldMeta* meta, const void* wpack, const float* h_planes, const void* J_planes,
                       int64_t S, const float* dsdf, const float* gn, float* dh_planes, float* g_planes,
                       float* dsdf_w, float* dsdf_b, float* dx, int64_t plane_pitch, void* stream);
/* The SDF decoder with an embedded-position block appended to its input (meta->embed_E > 0):
 * ``surface_cfg.extra_pos_embed_cfg{type: sinusoidal_legacy, n_frequencies: N}`` of the StyleLoTD Vehicle block
 * (code_multi/configs/exps/fg_neus=hyper_lotd/no_fg_occ.221218.yaml:319-321).  Input = [2 num_levels features | x_n (3),
 * sin(2^k x_n) (3), cos(2^k x_n) (3), k = 0..N-1], x_n = the AABB-normalised position in [-1, 1] (meta->lotd.x_scale /
 * x_shift); sdf_w = [W1 (64 x FIN), (W2 (64 x 64)), w_head (64)], FIN = 2 num_levels + 3 + 6 N.
 *   with-grad forward: nsim_field_fwd on the level-major planes (h_planes / J_planes given) with the meta's wpack -- the first
 *     layer contracts over the feature chunks + two embedding chunks on the matrix cores (k_field<.., NE = 2>, csrc/field.hip);
 *   backward of the SDF branch: nsim_wide_bwd_sdf = nsim_field_bwd_sdf + the sample positions (the embedding and its
 *     x-derivative are regenerated in the kernel): k_field_bwd_j<.., NE = 2>; no dL/dx output;
 *   no-grad query (sampling, occupancy): nsim_wide_sdf on the f32 MASTER weights, f32 arithmetic on the VALU
 *     (csrc/wide_field.hip; meta->precision is not read) over f32 feature planes of nsim_lotd_gather_lm.
 * The hand-off planes of the backward feed nsim_lotd_scatter, the radiance backward is nsim_field_bwd_rad.  Points, n_dev /
 * n_add, plane pitches: as for nsim_field_sdf / _fwd / _bwd_sdf. */
int nsim_wide_sdf(const NsimFieldMeta* meta, int32_t n_freq, const float* sdf_w, const float* sdf_b, const float* x,
                  const float* rays_o, const float* rays_d, const float* t, const int64_t* ridx, int64_t S,
                  const int64_t* n_dev, int64_t n_add, const float* feat_planes, float* sdf, void* stream);
int nsim_wide_bwd_sdf(const NsimFieldMeta* meta, const void* wpack, const float* x, const float* rays_o,
                      const float* rays_d, const float* t, const int64_t* ridx, int64_t S, const float* h_planes,
                      const void* J_planes, int64_t plane_pitch, const float* dsdf, const float* gn, float* dh_planes,
                      float* g_planes, float* dsdf_w, float* dsdf_b, void* stream);
/* (3) LoTD scatter (LoTD backward incl. the dy/dx path): dgrid[level][vertex][f] (f32, atomics) +=
 *     w_c * dh[f] + g[f] * (d w_c/d x . gn).  gn may be NULL (no second-order term); g_planes is required (code 28) and
 *     READ even then -- it must be readable [NLP,S,2] memory holding FINITE values (g * 0 is added: a NaN or Inf there
 *     poisons the gradient); a caller without a g passes dh_planes in its place (fields/nerf.py).
 *     Levels [level_begin, level_begin + level_count) only (level_count <= 0: all) -- a data-parallel caller scatters
 *     the pyramid in two halves and starts the all-reduce of the first half's gradient while the second is computed. */
int nsim_lotd_scatter(const NsimLotdMeta* meta, const float* x, const float* rays_o, const float* rays_d,
                      const float* t, const int64_t* ridx, const int64_t* ray_goff, int64_t S,
                      const float* dh_planes, const float* g_planes, const float* gn, float* dgrid, int level_begin,
                      int level_count, void* stream);
/* (4, pose refinement only) position gradient of the normals' own dependence on x: nablas = (d sdf/d h) . dh/dx(x), and
 *     inside a cell the trilinear interpolant has mixed second derivatives:
 *     dx[s][c] += sum_{l,f} g[l][s][f] sum_{c' != c} gn[s][c'] d2 h_{l,f} / dx_c' dx_c.   g_planes from (2), gn from (1). */
int nsim_lotd_hess_dx(const NsimLotdMeta* meta, const void* grid_f16, const float* x, const float* rays_o,
                      const float* rays_d, const float* t, const int64_t* ridx, const int64_t* ray_goff, int64_t S,
                      const float* g_planes, const float* gn, float* dx, void* stream);
/* (5, pose refinement only) x_s = o_r + t_s d_r, v_s = d_r  =>  d_rays_o[r] += dx_s, d_rays_d[r] += t_s dx_s + dv_s
 *     (dv, d_rays_o, d_rays_d may each be NULL); the outputs [R,3] are initialised by the caller. */
int nsim_ray_grad_reduce(const float* dx, const float* dv, const float* t, const int64_t* ridx, int64_t S,
                         float* d_rays_o, float* d_rays_d, void* stream);

/* ------------------------------------------------ NeRF++ distant-view model (LoTDNeRFDistant) */
/* 4-D LoTD level table of ``lotd_auto_compute_cfg{type: ngp4d}`` (lotd_neus.dtu.230814.yaml:193-200): level l has
 * res_xyz^3 * res_w vertices (Dense) or a 2^k-entry hash table; 2 features per level; <= 16 levels.
 * ``lotd_use_cuboid: true`` (withmask_withlidar_joint.240219.yaml:256): per-axis vertex counts -- res_xyz is the x
 * count, res_y / res_z the other two; 0 in res_y / res_z means "same as res_xyz" (cubic level). */
typedef struct NsimLotd4Meta {
  int32_t num_levels;
  int32_t res_xyz[16];
  int32_t res_w[16];
  int32_t type[16];
  uint32_t size[16];
  int64_t offset[16];
  int32_t res_y[16];
  int32_t res_z[16];
} NsimLotd4Meta;

typedef struct NsimDistantMeta {
  NsimLotd4Meta lotd;
  int32_t precision;     /* 0: fp16 MFMA, 1: exact f32 MFMA */
} NsimDistantMeta;

int64_t nsim_distant_wpack_bytes(const NsimDistantMeta* meta);
/* den_w: [D1 (64 x F), Dhead (1 x 64)], den_b: [64, 1]; rad_w: [Q1 (64 x (F+20)), Q2 (64x64), Q3 (3x64)], rad_b [64,64,3];
 * F = 2 * num_levels; radiance input = [features F, SH-4 (16), appearance (4)]  (yaml :221-234). */
int nsim_distant_pack_weights(const NsimDistantMeta* meta, const float* den_w, const float* den_b, const float* rad_w,
                              const float* rad_b, void* wpack, void* stream);
/* ``ray_query_cfg{query_mode: march, march_cfg{sample_mode: box, max_steps: K}}`` with ``radius_scale_min/max``:
 * K shells per ray, 1/r uniform; t [N,K] = exit depth of the AABB (host float[6] = min,max) scaled by r about its
 * centre, u4 [N,K,4] = network input in [0,1]^4, valid [N,K] (shell crossed beyond near[ray]). jitter [N,K] or NULL. */
int nsim_distant_shells(const float* rays_o, const float* rays_d, const float* near, const float* jitter, int64_t N,
                        int K, const float* aabb, float r_min, float r_max, float* t, float* u4, uint8_t* valid,
                        void* stream);
/* alpha = 1 - exp(-sigma * delta), delta = t[k+1]-t[k]; last shell: 1e10 when include_inf_distance (object-centric
 * configs, lotd_neus.dtu.230814.yaml:236) else the previous interval repeated (street config with a sky model,
 * withmask_withlidar_joint.240219.yaml:294); 0 if !valid */
int nsim_density_alpha_fwd(const float* sigma, const float* t, const uint8_t* valid, int64_t N, int K,
                           int include_inf_distance, float* alpha, void* stream);
int nsim_density_alpha_bwd(const float* sigma, const float* t, const uint8_t* valid, const float* dalpha, int64_t N,
                           int K, int include_inf_distance, float* dsigma, void* stream);
/* fused 4-D gather + density MLP + radiance MLP on S = N*K points (ray = s / K): sigma [S], rgb [S,3];
 * h_planes [16,S,2] (may be NULL) saves the features for the backward. */
int nsim_distant_fwd(const NsimDistantMeta* meta, const void* grid_f16, const void* wpack, const float* u4,
                     const float* rays_d, const float* h_appear, int64_t S, int K, float* sigma, float* rgb,
                     float* h_planes, void* stream);
/* The decoders of nsim_distant_fwd on h_planes [16,S,2] the caller has ALREADY filled (nsim_permuto_gather_pts): no table
 * is read; meta->lotd.num_levels gives F (a stub pyramid of that many levels serves as the meta). */
int nsim_distant_fwd_planes(const NsimDistantMeta* meta, const void* wpack, const float* h_planes, const float* rays_d,
                            const float* h_appear, int64_t S, int K, float* sigma, float* rgb, void* stream);
/* backward of nsim_distant_fwd: accumulates dden_w/dden_b/drad_w/drad_b (layouts above), dh_appear [N,4] (may be
 * NULL) and writes dh_planes [16,S,2] for nsim_lotd4_scatter. */
int nsim_distant_bwd(const NsimDistantMeta* meta, const void* wpack, const float* h_planes, const float* sigma_fwd,
                     const float* rgb_fwd, const float* rays_d, const float* h_appear, const uint8_t* valid,
                     int64_t S, int K, const float* dsigma, const float* drgb, float* dh_planes, float* dden_w,
                     float* dden_b, float* drad_w, float* drad_b, float* dh_appear, void* stream);
int nsim_lotd4_scatter(const NsimLotd4Meta* meta, const float* u4, const uint8_t* valid, int64_t S,
                       const float* dh_planes, float* dgrid, void* stream);

/* ------------------------------------------------ close-range NGP NeRF (LoTDNeRFObj / LoTDNeRFStreet: LoTDNeRFModel) */
/* InstantNGP + UrbanNeRF (docs/methods/ngp_lidar.md; code_single/configs/waymo/ngp_withlidar.230814.yaml:100-158; wrappers
 * app/models/single/nerf.py:33-143).  The implementation is in the absent nr3d_lib: semantics fixed in DESIGN sec. 7.
 *   encoding_cfg (yaml :103-118): the 3-D LoTD pyramid, <= 16 levels x 2 features, gathered LEVEL-MAJOR by the existing entry
 *     points (nsim_field_fwd with wpack == NULL for a with-grad query, nsim_lotd_gather_lm on an f32 meta otherwise) into
 *     h_planes [16][P][2] f32; ``anneal_cfg{type: hardmask}``: lotd.n_active_levels (masked levels are neither read nor given
 *     a gradient).
 *   density_decoder_cfg{D: 1, W: 64, output_activation{trunc_exp, offset: -1}} + extra_pos_embed_cfg{identity} +
 *     n_extra_feat_from_output: 31 (yaml :119-128): [h (2 num_levels) | x_n (3)] -> 64 (relu) -> 32 (linear), x_n = the
 *     AABB-normalised position 2 (x * x_scale + x_shift) - 1; output 0 = raw, sigma = exp(raw - 1), outputs 1..31 = geometry
 *     feature.  den_w = [W1 (64 x (2 num_levels + 3)), W2 (32 x 64)] row-major, den_b = [64, 32].
 *   radiance_decoder_cfg{use_pos: false, use_view_dirs: true, use_nablas: false, dir_embed_cfg{spherical, 4}, D: 2, W: 64}
 *     (yaml :129-137): [geo (31) | SH-4 of the normalised rays_d (16) | h_appear (n_appear = 0 | 4)] -> 64 -> 64 (relu) -> 3
 *     (sigmoid).  rad_w = [Q1 (64 x (47 + n_appear)), Q2 (64 x 64), Q3 (3 x 64)], rad_b = [64, 64, 3]. */
typedef struct NsimNgpMeta {
  NsimLotdMeta lotd;     /* 1..16 levels */
  int32_t precision;     /* 0: fp16 MFMA, 1: exact f32 MFMA */
  int32_t n_appear;      /* radiance_decoder_cfg.n_appear_embedding: 0 or 4 */
} NsimNgpMeta;
/* MFMA-fragment pack of the f32 master weights (once per optimizer step), as nsim_distant_pack_weights. */
int64_t nsim_ngp_wpack_bytes(const NsimNgpMeta* meta);
int nsim_ngp_pack_weights(const NsimNgpMeta* meta, const float* den_w, const float* den_b, const float* rad_w,
                          const float* rad_b, void* wpack, void* stream);
/* Fused decoders over the feature planes (pitch plane_pitch; 0 = NSIM_PLANE_PITCH(S)) of S points x [S,3] or
 * rays_o[ridx] + t rays_d[ridx] (``ray_query_cfg{query_mode: march_occ}``, yaml :153-158: the samples of nsim_march_*).
 * Writes sigma [S], alpha [S] = 1 - exp(-sigma step) (may be NULL) and rgb [S,3].  rgb == NULL: the density decoder alone
 * (lidar rays -- with_rgb=False --, the occupancy refresh, sample_pts_uniform); rays_d / ridx are then not needed with x. */
int nsim_ngp_fwd(const NsimNgpMeta* meta, const void* wpack, const float* h_planes, int64_t plane_pitch, const float* x,
                 const float* rays_o, const float* rays_d, const float* t, const int64_t* ridx, const float* h_appear,
                 int64_t S, float step, float* sigma, float* alpha, float* rgb, void* stream);
/* Backward on the saved planes and forward outputs: dsigma / dalpha [S], drgb [S,3] (each may be NULL; drgb == NULL skips the
 * radiance decoder, drad_w / drad_b are then untouched).  Accumulates dden_w / dden_b / drad_w / drad_b (layouts above; through
 * the replicas of nsim_set_grad_scratch when a scratch of 16 x 16384 floats is registered), dh_appear [R,4] (may be NULL)
 * and writes dh_planes [16][S][2] (may be NULL) for nsim_lotd_scatter (g_planes = gn = NULL).  trunc_exp: d sigma / d raw =
 * exp(min(raw - 1, 15)).  The rays get no gradient. */
int nsim_ngp_bwd(const NsimNgpMeta* meta, const void* wpack, const float* h_planes, int64_t plane_pitch, const float* x,
                 const float* rays_o, const float* rays_d, const float* t, const int64_t* ridx, const float* h_appear,
                 int64_t S, float step, const float* sigma_fwd, const float* rgb_fwd, const float* dsigma,
                 const float* dalpha, const float* drgb, float* dh_planes, float* dden_w, float* dden_b, float* drad_w,
                 float* drad_b, float* dh_appear, void* stream);
/* Pose refinement (``LearnableParams{refine_ego_motion, enable_after}``: the rays, or the points x, carry gradients; the model
 * opts in with ``ray_query_cfg.query_param.rays_has_grad``).  The sample depths t are constants of the step:
 * x_s = o_r + t_s d_r, v_s = d_r.  nsim_ngp_bwd_pose is nsim_ngp_bwd (same arguments, same weight / table / appearance
 * gradients; dh_planes is required) that also WRITES, one row per sample,
 *   dx [S,3] (required): the share of the first density layer's direct position input, W1[:, F:]^T da1 . 2 x_scale (object
 *     coordinates) -- the table's share is added by nsim_lotd_dx_lm below;
 *   dv [S,3] (NULL, or with drgb != NULL): the gradient to the UN-NORMALISED rays_d[ridx]: the SH-4 slots of the radiance
 *     input gradient through d sh4 / d n and n = d / |d|, i.e. (I - n n^T) g / |d|.
 * Launch order of a backward with ray gradients: (1) nsim_ngp_bwd_pose, (2) nsim_lotd_dx_lm (dx_add = dx, in place),
 * (3) nsim_ray_grad_reduce (or dx is the gradient to x), (4) nsim_lotd_scatter. */
int nsim_ngp_bwd_pose(const NsimNgpMeta* meta, const void* wpack, const float* h_planes, int64_t plane_pitch, const float* x,
                      const float* rays_o, const float* rays_d, const float* t, const int64_t* ridx, const float* h_appear,
                      int64_t S, float step, const float* sigma_fwd, const float* rgb_fwd, const float* dsigma,
                      const float* dalpha, const float* drgb, float* dh_planes, float* dden_w, float* dden_b, float* drad_w,
                      float* drad_b, float* dh_appear, float* dx, float* dv, void* stream);
/* Position gradient of the level-major 3-D gather (the LoTD counterpart of nsim_permuto_dx_pts), at x [S,3] or
 * rays_o[ridx] + t rays_d[ridx]:  dx[s][c] = dx_add[s][c] + sum_{l < n_active} sum_f dh_planes[l][s][f] d h[l][f] / d x_c,
 * the derivative of the trilinear weights times the eight vertex entries of the fp16 table (Dense and Hash levels), scaled
 * by x_scale (R - 1): object coordinates.  dh_planes [16][plane_pitch][2] (0 = S: what nsim_ngp_bwd writes); dx_add [S,3]
 * may be NULL or dx itself.  Every row of dx [S,3] is written by one lane: no atomics, no zero-fill; masked levels'
 * tables and planes are not read.  At most 16 levels. */
int nsim_lotd_dx_lm(const NsimLotdMeta* meta, const void* grid_f16, const float* x, const float* rays_o, const float* rays_d,
                    const float* t, const int64_t* ridx, int64_t S, const float* dh_planes, int64_t plane_pitch,
                    const float* dx_add, float* dx, void* stream);
/* ``accel_cfg{type: occ_grid, occ_thre, occ_thre_consider_mean, ema_decay, update_from_net_cfg, update_from_samples_cfg: {}}``
 * of a density field (yaml :138-152): the value grid holds densities.  update: val = max(val * decay, sigma(p)) over pts [n,3];
 * collect (a training step's own samples: x [n,3] or rays + t + ridx): the max-fold without decay; pack_bits_mean: a voxel is
 * occupied when val > thre, thre = consider_mean ? min(occ_thre, mean(val)) : occ_thre, the mean taken on the device.
 * workspace: 65 floats, contents irrelevant; workspace[64] receives the threshold used. */
int nsim_occ_update_density(float* val, int64_t nvox, float decay, const float* pts, const float* sigma, int64_t n,
                            const NsimOccMeta* meta, void* stream);
int nsim_occ_collect_density(float* val, const float* x, const float* rays_o, const float* rays_d, const float* t,
                             const int64_t* ridx, const float* sigma, int64_t n, const NsimOccMeta* meta, void* stream);
int nsim_occ_pack_bits_mean(const float* val, int64_t nvox, float occ_thre, int consider_mean, float* workspace,
                            uint32_t* bits, void* stream);

/* ------------------------------------------------ dynamic-only EmerNeRF (EmerNerfStreetOnlyDynamic: EmerNeRFOnlyDynamicModel) */
/* A density NeRF over (x, y, z, time) (code_multi/configs/exps/fg_neus=permuto_emernerf/with_gtbox.240212.yaml:277-360; wrapper
 * app/models/single/dynamic_nerf.py).  The implementation is in the absent nr3d_lib: semantics fixed in DESIGN sec. 7.
 *   dynamic_encoding_cfg{type: permuto} (yaml :290-300): a 4-D permutohedral lattice, <= 16 levels x 2 features, gathered
 *     LEVEL-MAJOR by nsim_permuto_gather_pts from the lattice points of nsim_dyn_points into h_planes [16][P][2] f32.  The meta is
 *     NsimNgpMeta: lotd.num_levels / lotd.n_active_levels give the level count and the hardmask (the pyramid itself is not read).
 *   dynamic_decoder_cfg{D: 1, W: 64, relu} + n_geometry_feat: 64 (yaml :281, :301-305): h (2 num_levels) -> 64 (relu) -> 65
 *     (linear); output 0 = raw, sigma = softplus(raw) = log1p(exp(raw)) (``trunc_softplus``: d sigma / d raw =
 *     sigmoid(min(raw, 15))), outputs 1..64 = geometry feature.  den_w = [W1 (64 x 2 num_levels), W2 (65 x 64)] row-major,
 *     den_b = [64, 65].
 *   radiance_cfg{use_pos: false, use_view_dirs: true, use_nablas: false, dir_embed_cfg{spherical, 4}, D: 2, W: 64} (yaml
 *     :329-338): [geo (64) | SH-4 of the normalised rays_d (16) | h_appear (n_appear = 0 | 4)] -> 64 -> 64 (relu) -> 3 (sigmoid).
 *     rad_w = [Q1 (64 x (80 + n_appear)), Q2 (64 x 64), Q3 (3 x 64)], rad_b = [64, 64, 3]. */
int64_t nsim_dyn_wpack_bytes(const NsimNgpMeta* meta);
int nsim_dyn_pack_weights(const NsimNgpMeta* meta, const float* den_w, const float* den_b, const float* rad_w,
                          const float* rad_b, void* wpack, void* stream);
/* Fused decoders over the feature planes (pitch plane_pitch; 0 = S, the pitch nsim_permuto_gather_pts writes) of S samples.
 * Writes sigma [S], alpha [S] = 1 - exp(-sigma step) (may be NULL) and rgb [S,3] from rays_d [R,3], ridx [S] and h_appear [R,4].
 * rgb == NULL: the density decoder alone (occupancy refresh, forward_density); rays_d / ridx are then not read. */
int nsim_dyn_fwd(const NsimNgpMeta* meta, const void* wpack, const float* h_planes, int64_t plane_pitch, const float* rays_d,
                 const int64_t* ridx, const float* h_appear, int64_t S, float step, float* sigma, float* alpha, float* rgb,
                 void* stream);
/* Backward on the saved planes and forward outputs: dsigma / dalpha [S], drgb [S,3] (each may be NULL; drgb == NULL skips the
 * radiance decoder and the geometry rows, drad_w / drad_b are then untouched).  Accumulates dden_w / dden_b / drad_w / drad_b
 * (layouts above; through the replicas of nsim_set_grad_scratch when the registered scratch holds them), dh_appear [R,4] (may
 * be NULL) and writes dh_planes [16][S][2] (may be NULL) for nsim_permuto_scatter_pts.  Neither rays nor times get a gradient. */
int nsim_dyn_bwd(const NsimNgpMeta* meta, const void* wpack, const float* h_planes, int64_t plane_pitch, const float* rays_d,
                 const int64_t* ridx, const float* h_appear, int64_t S, float step, const float* sigma_fwd, const float* rgb_fwd,
                 const float* dsigma, const float* dalpha, const float* drgb, float* dh_planes, float* dden_w, float* dden_b,
                 float* drad_w, float* drad_b, float* dh_appear, void* stream);
/* The aggregating variants of the with-flow model (EmerNeRF's 1/2, 1/4, 1/4 temporal aggregation): h_planes [16][3S][2] holds, per
 * level, the features of the S samples, then of their forward-warped, then of their backward-warped neighbours (one
 * nsim_permuto_gather_pts over the 3S lattice points).  The first density layer runs on each set, the hidden activations are
 * blended a = 1/2 relu(.) + 1/4 relu(.) + 1/4 relu(.), everything after is nsim_dyn_fwd's.  bwd writes dh_planes [16][3S][2] in the
 * same layout (for nsim_permuto_scatter_pts over the 3S points and nsim_permuto_dx_pts over the 2S warped ones). */
int nsim_dyn_fwd_agg(const NsimNgpMeta* meta, const void* wpack, const float* h_planes, const float* rays_d, const int64_t* ridx,
                     const float* h_appear, int64_t S, float step, float* sigma, float* alpha, float* rgb, void* stream);
int nsim_dyn_bwd_agg(const NsimNgpMeta* meta, const void* wpack, const float* h_planes, const float* rays_d, const int64_t* ridx,
                     const float* h_appear, int64_t S, float step, const float* sigma_fwd, const float* rgb_fwd,
                     const float* dsigma, const float* dalpha, const float* drgb, float* dh_planes, float* dden_w, float* dden_b,
                     float* drad_w, float* drad_b, float* dh_appear, void* stream);
/* Pose refinement (the rays carry gradients; ``ray_query_cfg.query_param.rays_has_grad``): nsim_dyn_bwd / nsim_dyn_bwd_agg with a
 * colour gradient (drgb, dh_planes and dv required) that also WRITE dv [S,3], one row per sample: the gradient to the
 * UN-NORMALISED rays_d[ridx] -- the SH-4 slots of the radiance input gradient through d sh4 / d n and n = d / |d|, i.e.
 * (I - n n^T) g / |d|.  The model has no direct position input: the position gradient of a sample is nsim_permuto_dx_pts on the
 * dh planes (components 0..2; the time component is dropped -- times get no gradient); with flow, plus the position parts of
 * dx4w at the two warped points (both lattices) and nsim_permuto_dx_pts on the flow lattice at x with the dh planes nsim_flow_bwd
 * leaves for the total dflow6.  Without a colour gradient there is no dv: the plain entry points serve.  Then
 * nsim_ray_grad_reduce. */
int nsim_dyn_bwd_pose(const NsimNgpMeta* meta, const void* wpack, const float* h_planes, int64_t plane_pitch, const float* rays_d,
                      const int64_t* ridx, const float* h_appear, int64_t S, float step, const float* sigma_fwd,
                      const float* rgb_fwd, const float* dsigma, const float* dalpha, const float* drgb, float* dh_planes,
                      float* dden_w, float* dden_b, float* drad_w, float* drad_b, float* dh_appear, float* dv, void* stream);
int nsim_dyn_bwd_agg_pose(const NsimNgpMeta* meta, const void* wpack, const float* h_planes, const float* rays_d,
                          const int64_t* ridx, const float* h_appear, int64_t S, float step, const float* sigma_fwd,
                          const float* rgb_fwd, const float* dsigma, const float* dalpha, const float* drgb, float* dh_planes,
                          float* dden_w, float* dden_b, float* drad_w, float* drad_b, float* dh_appear, float* dv, void* stream);
/* dx [S,3] (every row written) = the position parts of dx4_dyn[s] + dx4_flow[s] (nsim_permuto_dx_pts at the samples on the dynamic
 * / the flow lattice, [S,4]) + dx4w_dyn[s] + dx4w_dyn[S + s] + dx4w_flow[s] + dx4w_flow[S + s] (at the 2S warped points, [2S,4]:
 * x+- = x +- flow, so d x+- / d x = I).  Each input may be NULL.  The time components are dropped. */
int nsim_dyn_pose_dx(const float* dx4_dyn, const float* dx4_flow, const float* dx4w_dyn, const float* dx4w_flow, int64_t S,
                     float* dx, void* stream);
/* The scene-flow decoder of the with-flow EmerNeRF model (``flow_decoder_cfg{type: mlp, D: 2, W: 64}``, code_multi/configs/exps/
 * fg_emernerf/no_gtbox_with_flow.240208.yaml): features of the flow lattice (num_levels <= 16 levels x 2, level-major planes
 * [16][plane_pitch][2] of nsim_permuto_gather_pts, plane_pitch 0 = S) -> 64 (relu) -> 64 (relu) -> 6 (linear): flow6 [S,6] f32,
 * columns 0..2 flow_fwd, 3..5 flow_bwd.  The hidden layers run on the MFMA tiles of csrc/mfma_mlp.h (precision 0: fp16 operands,
 * 1: f32), the six output rows as f32 dot products.  Flat row-major parameters flow_w [64 x 2 num_levels | 64 x 64 | 6 x 64],
 * flow_b [64 | 64 | 6]; wpack (nsim_flow_wpack_bytes) is written by nsim_flow_pack_weights.
 * bwd: dflow6 [S,6] -> dflow_w / dflow_b ACCUMULATED (caller-zeroed; through the replicas of nsim_set_grad_scratch when
 * registered) and dh_planes [16][plane_pitch][2] (rows of the lattice's own levels written; may be NULL) for
 * nsim_permuto_scatter_pts / nsim_permuto_dx_pts. */
int64_t nsim_flow_wpack_bytes(int precision);
int nsim_flow_pack_weights(int num_levels, int precision, const float* flow_w, const float* flow_b, void* wpack, void* stream);
int nsim_flow_fwd(int num_levels, int precision, const void* wpack, const float* h_planes, int64_t plane_pitch, int64_t S,
                  float* flow6, void* stream);
int nsim_flow_bwd(int num_levels, int precision, const void* wpack, const float* h_planes, int64_t plane_pitch, int64_t S,
                  const float* dflow6, float* dh_planes, float* dflow_w, float* dflow_b, void* stream);
/* The flow-warped lattice points: x4w [2S,4] = (x + flow_fwd, min(w + delta, code_hi)) | (x + flow_bwd, max(w - delta, code_lo))
 * from x4 [S,4] (object coordinates and time code, nsim_dyn_points) and flow6 [S,6]; delta = the spacing of the keyframe codes.
 * bwd: dflow6 [S,6] += the position parts of dx4w [2S,4] (nsim_permuto_dx_pts at the warped points). */
int nsim_dyn_warp_fwd(const float* x4, const float* flow6, int64_t S, float delta, float code_lo, float code_hi, float* x4w,
                      void* stream);
int nsim_dyn_warp_bwd(const float* dx4w, int64_t S, float* dflow6, void* stream);
/* The time input.  keyframes [T] ascending (the model's ``ts_keyframes`` for w, the accelerator's for the slices), ts [n]:
 *   w [n] (may be NULL) = SeqEmbedding(keyframes, codes)(ts, 'interp') for codes [T] (``time_embedding_cfg{dim: 1}``):
 *     v[i-1] + f (v[i] - v[i-1]) on the interval that holds ts, f clamped to [0,1] (the ends clamp), v[0] when T == 1;
 *   slice [n] (may be NULL) = the index of the nearest keyframe, a tie to the lower index, times outside the range to the
 *     first / last; word_off [n] (may be NULL) = slice * words_per_slice, the ray_word_off of nsim_march_count / _emit. */
int nsim_dyn_time(const float* keyframes, const float* codes, int T, const float* ts, int64_t n, int64_t words_per_slice,
                  float* w, int64_t* slice, int64_t* word_off, void* stream);
/* Lattice points x4 [S,4] = (position, time coordinate): x [S,3] with w [S], or rays_o[ridx] + t rays_d[ridx] with w [R]. */
int nsim_dyn_points(const float* x, const float* rays_o, const float* rays_d, const float* t, const int64_t* ridx,
                    const float* w, int64_t S, float* x4, void* stream);
/* ``accel_cfg{type: occ_grid_dynamic}`` (yaml :339-354): K value grids of nvox voxels, slice_stride floats apart, one per
 * accelerator keyframe.  slice: the grid of every point (pts / x: [n]) or of every ray (rays + t + ridx: [R]); an index outside
 * [0, K) drops the point.  update: ALL slices decay once, then every point is max-folded into its own slice; collect: the
 * max-fold alone; pack_bits_mean: slice k's bits (ceil(nvox / 32) words each, padding bits clear) from slice k's own mean.
 * workspace: 65 K floats, contents irrelevant; workspace[65 k + 64] receives slice k's threshold. */
int nsim_occ_update_density_sliced(float* val, int64_t nvox, int64_t slice_stride, int K, float decay, const float* pts,
                                   const float* sigma, const int64_t* slice, int64_t n, const NsimOccMeta* meta,
                                   void* stream);
int nsim_occ_collect_density_sliced(float* val, int64_t slice_stride, int K, const float* x, const float* rays_o,
                                    const float* rays_d, const float* t, const int64_t* ridx, const int64_t* slice,
                                    const float* sigma, int64_t n, const NsimOccMeta* meta, void* stream);
int nsim_occ_pack_bits_mean_sliced(const float* val, int64_t nvox, int64_t slice_stride, int K, float occ_thre,
                                   int consider_mean, float* workspace, uint32_t* bits, void* stream);

/* ------------------------------------------------------------------------------- sky MLP (row a16) */
/* ``SimpleSky`` (app/models/env/sky.py:16-51) as configured by the street configs
 * (code_single/configs/waymo/streetsurf/withmask_withlidar_joint.240219.yaml:312-322): sinusoidal embedding of the
 * unit view direction [v, {sin(2^f v), cos(2^f v)}_{f<F}] (3 + 6F dims) ++ h_appear (A dims) -> 256 -> 256 -> 3,
 * ReLU hidden, sigmoid output (D = 2, W = 256 are fixed; 3 + 6F + A <= 96).  One query per RAY
 * (call site app/renderers/single_volume_renderer.py:449-457).
 * Flat weights in layer order: w = [W1 (256 x IN), W2 (256 x 256), W3 (3 x 256)] row-major, b = [256, 256, 3],
 * IN = 3 + 6F + A.  planes_fwd: [(96 + 256 + 256) * pitch] floats, planes_bwd: [(32 + 256 + 256) * pitch] floats
 * scratch, pitch = nsim_sky_plane_pitch(N) (N rounded up to 128). */
typedef struct NsimSkyMeta {
  int32_t n_frequencies;  /* F */
  int32_t n_appear;       /* A */
  int32_t precision;      /* 0: fp16 MFMA, 1: exact f32 MFMA */
} NsimSkyMeta;

int64_t nsim_sky_wpack_bytes(const NsimSkyMeta* meta);
int64_t nsim_sky_plane_pitch(int64_t N);
int nsim_sky_pack_weights(const NsimSkyMeta* meta, const float* w, const float* b, void* wpack, void* stream);
/* rgb [N,3] = sky(v [N,3], h_appear [N,A] (NULL iff A == 0)); planes_fwd (may be NULL) saves the activations. */
int nsim_sky_fwd(const NsimSkyMeta* meta, const void* wpack, const float* v, const float* h_appear, int64_t N,
                 float* rgb, float* planes_fwd, void* stream);
/* accumulates dw / db (layouts above, caller zeroes) and writes dh_appear [N,A] (may be NULL). */
int nsim_sky_bwd(const NsimSkyMeta* meta, const void* wpack, const float* rgb_fwd, const float* drgb, int64_t N,
                 const float* planes_fwd, float* planes_bwd, float* dw, float* db, float* dh_appear, void* stream);

/* ------------------------------------------------------------------------------- losses (row a18) */
/* Fused reductions of the two losses of the object-centric configs and the gradient of the appearance-embedding
 * lookup.  *out is a device scalar the caller zeroes; the kernels ADD the mean into it.
 *   eikonal: mean((|nablas_i| - 1)^2), nablas [S,3]          replaces app/loss/eikonal.py:96-105 (fn, plain mse) + .mean()
 *   mse:     mean((pred - gt)^2) over n floats               replaces app/loss/photometric.py:88-146 (fn_type mse)
 *   rows_scatter_add: out[idx[i], :] += g[i, :], g [n,C], out [rows,C]
 *                                                            backward of ``embed[fidx]``, app/models/scene/image_embeddings.py:23-80 */
int nsim_eikonal_loss_fwd(const float* nablas, int64_t S, float* out, void* stream);
int nsim_eikonal_loss_bwd(const float* nablas, int64_t S, const float* gout, float* dnablas, void* stream);
int nsim_mse_loss_fwd(const float* pred, const float* gt, int64_t n, float* out, void* stream);
int nsim_mse_loss_bwd(const float* pred, const float* gt, int64_t n, const float* gout, float* dpred, void* stream);
int nsim_rows_scatter_add(const float* g, const int64_t* idx, int64_t n, int C, int64_t rows, float* out, void* stream);
/* its forward: out[i, :] = table[idx[i], :] (i < n; an index outside [0, rows) gives zeros), followed by ``tail`` zero rows
 * (the free points a training step appends to its rays carry no appearance code) -- out [n + tail, C]. */
int nsim_rows_gather(const float* table, const int64_t* idx, int64_t n, int C, int64_t rows, int64_t tail, float* out,
                     void* stream);
/* The SDF curvature regulariser (PermutoSDF, Rosu & Behnke 2023): the pointwise part of ``model.get_sdf_curvature_1d(net_x,
 * nablas, eps=)``, app/loss/sdf_curvature.py:69,75 (the method itself lives in the absent nr3d_lib; semantics: DESIGN.md sec. 7).
 *   curv_shift:     x_out = clamp(x + eps (n^ x r^), aabb_lo, aabb_hi) with n^ = nablas / max(|nablas|, 1e-12), r^ = dirs
 *                   normalised alike; the cross product is NOT renormalised.  aabb_lo / aabb_hi: 3 device floats each.
 *   curv_angle_fwd: curv[i] = acos(clamp(n0^ . n1^, -(1 - 1e-6), 1 - 1e-6)) / pi      (the bound as its nearest f32)
 *   curv_angle_bwd: dn0 / dn1 [n,3] (either may be NULL) from gcurv [n], recomputed from n0, n1 -- the forward's output is not
 *                   read, so the caller may modify it in place (``curvature.clamp_max_(0.5)``, sdf_curvature.py:42).  Zero where
 *                   the clamp is active and for a vector shorter than 1e-12.
 *   curv_loss_fwd:  out[0] += mean(min(curv_i, clamp_max)) in one launch (out zeroed by the caller, as eikonal_loss_fwd)
 *   curv_loss_bwd:  its gradient given gout [1]; dn0 / dn1 as above. */
int nsim_curv_shift(const float* nablas, const float* x, const float* dirs, const float* aabb_lo, const float* aabb_hi,
                    float eps, int64_t n, float* x_out, void* stream);
int nsim_curv_angle_fwd(const float* n0, const float* n1, int64_t n, float* curv, void* stream);
int nsim_curv_angle_bwd(const float* n0, const float* n1, const float* gcurv, int64_t n, float* dn0, float* dn1,
                        void* stream);
int nsim_curv_loss_fwd(const float* n0, const float* n1, int64_t n, float clamp_max, float* out, void* stream);
int nsim_curv_loss_bwd(const float* n0, const float* n1, int64_t n, float clamp_max, const float* gout, float* dn0,
                       float* dn1, void* stream);
/* SSIM and S3IM (Xie et al., ICCV 2023): replaces ``nr3d_lib.models.loss.ssim.ssim_module`` (absent; the pytorch-ssim form: five
 * grouped conv2d + ~20 elementwise ops and their backward) under ``PerceptualLoss(loss_type='ssim')`` and ``S3IMLoss``,
 * app/loss/perceptual.py:61-70, 142-157.  Window g gT with g[i] ~ exp(-(i - k/2)^2 / (2 1.5^2)) normalised to sum 1, zero
 * padding (k - 1) / 2, stride s, per channel; C1 = 0.01^2, C2 = 0.03^2; 1 <= k <= 11; Ho = (H + 2p - k) / s + 1, Wo alike.
 *   index == NULL  planar: x, y [BC, H, W], BC = B C single-channel images;
 *   index != NULL  indexed: x, y [n_rows, 3]; pixel (i, j) of the ONE image [3, H, W] is row index[i W + j] (index [H W] int64,
 *                  BC = 1; an index outside [0, n_rows) is a zero pixel without gradient) -- S3IM's virtual image
 *                  (perceptual.py:151-156), not materialised.
 *   ssim_fwd: out[0] += mean of the SSIM map over all windows (out zeroed by the caller); coef [3, n_windows] f32 is written for
 *             the backward (n_windows = BC Ho Wo, times 3 in the indexed form).
 *   ssim_bwd: dx = gout[0] d out / d x.  Planar: every element of dx [BC, H, W] is written.  Indexed: ADDED into dx [n_rows, 3],
 *             which the caller zeroes (rows the index does not name stay zero).  No gradient to y. */
int nsim_ssim_fwd(const float* x, const float* y, const int64_t* index, int64_t n_rows, int64_t BC, int H, int W, int k, int s,
                  float* out, float* coef, void* stream);
int nsim_ssim_bwd(const float* x, const float* y, const int64_t* index, int64_t n_rows, int64_t BC, int H, int W, int k, int s,
                  const float* coef, const float* gout, float* dx, void* stream);
/* The loss head of one training step in a single launch (the reference's total = mse + w (eikonal(render samples) +
 * eikonal(uniform points)), code_single/tools/train.py:1411-1423 with app/loss/photometric.py + eikonal.py):
 *   acc[0] += mse(pred, gt) over n_img floats; acc[1] += eikonal(nablas[:S]); acc[2] += eikonal(nablas[S:S+M]);
 *   d_pred = d total / d pred;  d_nablas [S+M,3] = d total / d nablas.   acc [3] zero on entry. */
int nsim_train_loss_head(const float* pred, const float* gt, int64_t n_img, const float* nablas, int64_t S, int64_t M,
                         float w_eikonal, float* acc, float* d_pred, float* d_nablas, void* stream);
/* The supervision losses of the street configs beside rgb and eikonal (withmask_withlidar_joint.240219.yaml:438-500).  Each
 * reduction adds into an ``out`` the caller zeroes (as eikonal_loss_fwd) and carries its weight ``w``; each forward also writes
 * the UNSCALED gradient d out / d input, so its backward is ``loss_scale_bwd``: d [n] = gout[0] g [n].
 *   mask_bce_fwd   replaces MaskOccupancyLoss.forward, app/loss/mask.py:57-103 (F.binary_cross_entropy on the clamped
 *                  prediction, nr3d_lib's safe_binary_cross_entropy): p = clamp(pred, lo, hi); out[0] += w / N sum of
 *                  -(gt max(log p, -100) + (1 - gt) max(log(1 - p), -100)) over the rays of ``mode`` -- 0: all, gt as given;
 *                  1 always_occupied: gt = 1 (gt may be NULL); 2 only_cull_non_occupied: gt < 0.5, against 0; 3
 *                  only_preserve_occupied: gt > 0.5, against 1.  err [N] = |pred - gt| (0 outside the selection); grad [N]: the
 *                  clamp passes the gradient where lo <= pred <= hi.
 *   mask_entropy_* replaces MaskEntropyRegLoss.forward_code_single, app/loss/mask_entropy.py:77-160, for every mode: a mode is a
 *                  table of up to 4 terms coef A log(max(B, eps)), A and B each one of the masks (source 0 mask_pred, 1 mask_cr,
 *                  2 mask_dv) or its complement, a detached factor gets no gradient; out[term.out] += mean over N.  The backward
 *                  re-evaluates the table (two sums, two upstream gradients); max(., eps) passes the gradient where B >= eps.
 *   sparsity_fwd   replaces SparsityLoss.fn_nld / fn_normal / fn_density_reg, app/loss/sparsity.py:47-54: out[0] += w mean of
 *                  type 0: 4 s (1 - s), s = sigmoid(param x) | 1: exp(-x^param) | 2: |1 - exp(-param x)| (sub-gradient 0 at 0).
 *   clearance_fwd  replaces ClearanceLoss.fn_penalty_sdf, app/loss/clearance.py:51-56, without its host read: out[0] += w / M sum
 *                  over near_sdf < thresh of exp(-beta (near_sdf - thresh)); nothing below the threshold: out stays 0, grad is 0.
 *   kth_value_f32  out[0] = torch.sort(x).values[k], bit for bit, for finite non-negative x (their bit patterns order as the
 *                  values): a radix select in ONE workgroup, four 8-bit passes over LDS histograms; replaces the full sort of
 *                  app/loss/lidar.py:281-283.
 *   lidar_valid    app/loss/lidar.py:264-266, 280: valid = (mask_pred > mask_pred_thresh) & (ranges > 0), and with discard_toofar >
 *                  0 additionally & (ranges <= discard_toofar) -- or, toofar_replaces_mask, the reference's literal line :266,
 *                  valid = ranges <= discard_toofar alone; err = |depth_pred - ranges| valid.
 *   lidar_loss_fwd app/loss/lidar.py:284-292 with DepthLoss :34-53 and LineOfSightLoss :81-210 (packed buffers): keep = valid &
 *                  !(err > median[0] * factor) (factor <= 0: keep = valid); acc[0] += w_depth mean over N of fn(pred, ranges) keep;
 *                  per pack r of the buffer, with g = ranges[rays_inds_hit[r]]: los_fn 1 (nerf, neus_urban) acc[1] += w_los / R
 *                  keep sum over g - bound <= t <= g + bound of (vw - Normal(t - g; 0, std))^2, acc[2] += ... sum over t < g - bound
 *                  of vw^2; los_fn 2 (neus_unisim) acc[2] += w_los / R keep sum over |t - g| > bound of vw^2.  member [S]: 0 / 1
 *                  neighbor / 2 empty.  g_depth [N], g_vw [S]: the unscaled gradients; the packs tile [0, S).
 *   lidar_loss_bwd d_depth = gout_depth g_depth; d_vw = (gout_neighbor | gout_empty by member) g_vw. */
typedef struct NsimEntropyTerm {
  int32_t a_src, a_neg, a_detach;   /* A: source, 1 - source?, detached? */
  int32_t b_src, b_neg, b_detach;   /* B, inside the log */
  int32_t out;                      /* 0 or 1 */
  float coef;
} NsimEntropyTerm;
typedef struct NsimEntropyTable {
  int32_t n_terms;                  /* 0..4 */
  NsimEntropyTerm t[4];
} NsimEntropyTable;
typedef struct NsimLidarLoss {
  float factor;                     /* discard_outliers_median; <= 0: off */
  int32_t depth_fn;                 /* -1 none, 0 l1, 1 l1_log, 2 l2, 3 l2_relative, 4 l2_normalized, 5 huber */
  float depth_param;                /* far (4), alpha (5) */
  float w_depth;
  int32_t los_fn;                   /* 0 none, 1 nerf / neus_urban, 2 neus_unisim */
  float bound;                      /* sigma (1), epsilon (2) */
  float std;                        /* sigma / sigma_scale_factor (1) */
  float w_los;
} NsimLidarLoss;
int nsim_loss_scale_bwd(const float* g, int64_t n, const float* gout, float* d, void* stream);
int nsim_mask_bce_fwd(const float* pred, const float* gt, int64_t N, float lo, float hi, int mode, float w, float* out, float* err,
                      float* grad, void* stream);
int nsim_mask_entropy_fwd(const NsimEntropyTable* tab, const float* mask_pred, const float* mask_cr, const float* mask_dv,
                          int64_t N, float eps, float* out, void* stream);
int nsim_mask_entropy_bwd(const NsimEntropyTable* tab, const float* mask_pred, const float* mask_cr, const float* mask_dv,
                          int64_t N, float eps, const float* gout0, const float* gout1, float* d_pred, float* d_cr, float* d_dv,
                          void* stream);
int nsim_sparsity_fwd(const float* x, int64_t M, int type, float param, float w, float* out, float* grad, void* stream);
int nsim_clearance_fwd(const float* near_sdf, int64_t M, float beta, float thresh, float w, float* out, float* grad, void* stream);
int nsim_kth_value_f32(const float* x, int64_t N, int64_t k, float* out, void* stream);
int nsim_lidar_valid(const float* depth_pred, const float* mask_pred, const float* ranges, int64_t N, float mask_pred_thresh,
                     float discard_toofar, int toofar_replaces_mask, uint8_t* valid, float* err, void* stream);
int nsim_lidar_loss_fwd(const NsimLidarLoss* cfg, const float* depth_pred, const float* ranges, const uint8_t* valid,
                        const float* err, const float* median, int64_t N, const float* t, const float* vw,
                        const int64_t* rays_inds_hit, const int64_t* pack_infos_hit, int64_t R, int64_t S, float* acc,
                        uint8_t* keep, float* g_depth, float* g_vw, uint8_t* member, void* stream);
int nsim_lidar_loss_bwd(const float* g_depth, int64_t N, const float* g_vw, const uint8_t* member, int64_t S,
                        const float* gout_depth, const float* gout_neighbor, const float* gout_empty, float* d_depth, float* d_vw,
                        void* stream);
/* The monocular depth / normal cue losses (app/loss/mono.py; the ``mono_depth`` / ``mono_normals`` blocks of
 * lotd_neus.replica.230814.yaml:272-288 and withmask_nolidar.240219.yaml:463-483).  Masks are uint8 (0 / non-zero).  Every sum is
 * taken in f64 into a workspace ``ws`` the caller zeroes; the workgroup that finishes last writes the f32 losses ``out``, so no
 * value is converted or read back by a further launch.  Weights are folded in.
 *   mono_remain_mask  replaces the ignore list and erosion of MonoDepthLoss.forward / MonoNormalLoss.forward (mono.py:358-397,
 *                     510-528): out [H,W] = 1 where no selected rule ignores the pixel.  flags: bit 0 toofar (depth_pred0 > far),
 *                     1 pred_not_occupied (!(mask_pred > mask_pred_thresh)), 2 not_occupied (!occupancy_gt), 3 dynamic, 4 human,
 *                     5 pred_distant (depth_pred > far08), 6 mono_distant (depth_gt > f32(depth_gt_sum / (H W)) - 1e-5; the sum by
 *                     mono_sum_f64); a map no set bit needs may be NULL.  keep_all: every pixel remains (the depth loss with an
 *                     empty list, :396-397).  erode e in 0..32: kornia.morphology.erosion with a flat 2e x 2e kernel of ones --
 *                     out[y,x] = min over rows y-e .. y+e-1, columns x-e .. x+e-1, pixels outside the image not eroding.
 *   mono_sum_f64      out[0] += sum of x [n] (the mean of depth_gt for mono_distant)
 *   mono_ssi_*        replace MonoSDFDepthLoss.forward (mono.py:136-158) on pred, gt, mask [H,W].  ws [12]:
 *                     moments: ws[0..5) += a00 a01 a11 b0 b1 of compute_scale_and_shift (:88-113), target = gt_pre_scale gt + gt_pre_shift;
 *                     fwd:     the solve (det == 0: scale = shift = 0), out[0] = w mean over H W of mask f, out[1] = w alpha_grad_reg
 *                              image-gradient regulariser (:115-134; alpha 0: 0), g_depth / g_reg [H,W] = the direct gradients
 *                              of the two to pred, ws[7..11) = d out / d (scale, shift);
 *                     bwd:     d_pred = gout_depth (g_depth + chain) + gout_reg (g_reg + chain), the chain through the solve in
 *                              closed form from the moments (none with detach_scale_shift or det == 0); a NULL gout is 0.
 *   mono_pearson_*    replace PearsonCorrDepthLoss.forward (mono.py:222-240, reverse_gt False): out[0] = w (1 - r) over the masked
 *                     pixels, out[1] = w alpha sum over scales of (1 - r_x) + (1 - r_y) of the finite differences over the pairs
 *                     with both mask pixels set (a set without a sample adds 0), r = C / max(sqrt(A) sqrt(B), 1e-12) of the
 *                     centred moments.  ws [103]: six raw sums per set, the ticket.  One launch per direction.
 *   mono_normal_fwd   replaces MonoNormalLoss.fn (mono.py:479-484) behind the rotation of :507: n' = rot n (rot_mode 0 none,
 *                     1 one [3,3], 2 per row [N,3,3]), both sides v / max(|v|, 1e-12); out[0] = w_l1 mean over N of mask sum_c |.|,
 *                     out[1] = w_cos mean of mask (1 - dot); mask NULL: all rows.  g_l1 / g_cos [N,3] = d out / d normals_pred; ws [3].
 *   mono_scale2_bwd   d [n] = gout0[0] g0 [n] + gout1[0] g1 [n]: the backward of mono_normal_fwd (a NULL gout is 0). */
typedef struct NsimMonoSsi {
  int32_t fn;                       /* 0 mse | l2, 1 l1, 2 log_l1, 3 smooth_l1, 4 relative_l1 | mape, 5 smape, 6 relative_l2, 7 huber */
  int32_t scale_gt_to_pred, detach_scale_shift, grad_reg_scales;
  double fn_param;                  /* beta (3), eps (4, 5, 6), alpha (7) */
  double gt_pre_scale, gt_pre_shift, alpha_grad_reg, w;
} NsimMonoSsi;
int nsim_mono_remain_mask(const float* mask_pred, const float* depth_pred0, const float* depth_pred, const float* depth_gt,
                          const uint8_t* occupancy_gt, const uint8_t* dynamic_gt, const uint8_t* human_gt, const double* depth_gt_sum,
                          int64_t H, int64_t W, float mask_pred_thresh, float far, float far08, int flags, int keep_all, int erode,
                          uint8_t* out, void* stream);
int nsim_mono_sum_f64(const float* x, int64_t n, double* out, void* stream);
int nsim_mono_ssi_moments(const NsimMonoSsi* cfg, const float* pred, const float* gt, const uint8_t* mask, int64_t H, int64_t W,
                          double* ws, void* stream);
int nsim_mono_ssi_fwd(const NsimMonoSsi* cfg, const float* pred, const float* gt, const uint8_t* mask, int64_t H, int64_t W,
                      double* ws, float* out, float* g_depth, float* g_reg, void* stream);
int nsim_mono_ssi_bwd(const NsimMonoSsi* cfg, const float* pred, const float* gt, const uint8_t* mask, int64_t H, int64_t W,
                      double* ws, const float* g_depth, const float* g_reg, const float* gout_depth, const float* gout_reg,
                      float* d_pred, void* stream);
int nsim_mono_pearson_fwd(const float* pred, const float* gt, const uint8_t* mask, int64_t H, int64_t W, double alpha_grad_reg,
                          int grad_reg_scales, double w, double* ws, float* out, void* stream);
int nsim_mono_pearson_bwd(const float* pred, const float* gt, const uint8_t* mask, int64_t H, int64_t W, double alpha_grad_reg,
                          int grad_reg_scales, double w, const double* ws, const float* gout_depth, const float* gout_reg,
                          float* d_pred, void* stream);
int nsim_mono_normal_fwd(const float* normals_pred, const float* normals_gt, const uint8_t* mask, const float* rot, int rot_mode,
                         int64_t N, double w_l1, double w_cos, double* ws, float* out, float* g_l1, float* g_cos, void* stream);
int nsim_mono_scale2_bwd(const float* g0, const float* g1, int64_t n, const float* gout0, const float* gout1, float* d, void* stream);
/* The scene-flow losses of a with-flow EmerNeRF query (app/loss/flow.py:35-55 FlowLoss.fn_cycle / fn_sparsity; the ``flow`` block of
 * code_multi/configs/exps/fg_emernerf/no_gtbox_with_flow.240208.yaml) on the four [S,3] tensors flow_fwd, flow_fwd_pred_bwd,
 * flow_bwd, flow_bwd_pred_fwd (S >= 1), both terms in one launch per direction:
 *   out[0] = w_cycle 1/2 mean_{S 3}[(sg(flow_fwd) + flow_fwd_pred_bwd)^2 + (sg(flow_bwd) + flow_bwd_pred_fwd)^2]   (sg: stop-gradient)
 *   out[1] = w_sparsity 1/4 mean_S[|flow_fwd| + |flow_fwd_pred_bwd| + |flow_bwd| + |flow_bwd_pred_fwd|]
 * f64 sums (per thread, per workgroup, one f64 atomic per workgroup; ws [3] f64 zeroed by the caller, the last workgroup writes
 * out [2] f32).  bwd recomputes from the inputs: d_* [S,3] written (a NULL d_* is skipped), gout_* the upstream gradients of out[0]
 * / out[1] on the device (NULL = 0); the gradient of a norm at zero is zero. */
int nsim_flow_loss_fwd(const float* flow_fwd, const float* flow_fwd_pred_bwd, const float* flow_bwd, const float* flow_bwd_pred_fwd,
                       int64_t S, double w_cycle, double w_sparsity, double* ws, float* out, void* stream);
int nsim_flow_loss_bwd(const float* flow_fwd, const float* flow_fwd_pred_bwd, const float* flow_bwd, const float* flow_bwd_pred_fwd,
                       int64_t S, double w_cycle, double w_sparsity, const float* gout_cycle, const float* gout_sparsity,
                       float* d_flow_fwd, float* d_flow_fwd_pred_bwd, float* d_flow_bwd, float* d_flow_bwd_pred_fwd, void* stream);
/* One object's share of the joint rendering: replaces SingleVolumeRenderer._volume_integration_in_total
 * (app/renderers/single_volume_renderer.py:104-120; the ``cr_only`` depth of the mono losses reads it).  Per pack r of the object's
 * buffer (pack_infos [P,2] = begin, count; rays_inds [P]; samples vw_in_total, t [S], rgb / nablas [S,3] or NULL):
 *   mask[ray] = sum vw, depth[ray] = sum vw t / (mask + 1e-10) (normalized_depth) or sum vw t, rgb / normals[ray] = sum vw x;
 *   normalize_nablas: the integrated normal is normalize(clamp(nabla, -1, 1)) (the reference outside training).
 * The outputs [N(,3)] are zeroed by the caller (rays the object does not hit keep the zeros).  bwd: mask / depth are the forward's
 * outputs; every g_* [N(,3)] and every d_* [S(,3)] may be NULL; no gradient to t. */
int nsim_packed_share_fwd(const float* vw_in_total, const float* t, const float* rgb, const float* nablas, const int64_t* pack_infos,
                          const int64_t* rays_inds, int64_t P, int64_t N, int normalized_depth, int normalize_nablas, float* mask,
                          float* depth, float* rgb_out, float* normals_out, void* stream);
int nsim_packed_share_bwd(const float* vw_in_total, const float* t, const float* rgb, const float* nablas, const int64_t* pack_infos,
                          const int64_t* rays_inds, int64_t P, int64_t N, int normalized_depth, int normalize_nablas, const float* mask,
                          const float* depth, const float* g_mask, const float* g_depth, const float* g_rgb, const float* g_normals,
                          float* d_vw, float* d_rgb, float* d_nablas, void* stream);
/* Compaction of the AABB-tested rays, (o, d, near, far)[idx] -> [R,...] in one launch
 * (model.ray_test, app/renderers/single_volume_renderer.py:235-238). */
int nsim_gather_rays(const float* rays_o, const float* rays_d, const float* near, const float* far, const int64_t* idx,
                     int64_t R, float* o_out, float* d_out, float* near_out, float* far_out, void* stream);
/* Synthetic supervision of bench.py (no dataset in this environment): analytic image of a sphere of ``radius`` at the
 * origin along unit rays -- rgb = 0.5 + 0.5 normal at the first hit, 0 elsewhere. */
int nsim_sphere_image(const float* rays_o, const float* rays_d, int64_t N, float radius, float* rgb, void* stream);

/* ------------------------------------------------------------------------------- optimizer */
/* Adam (training_cfg{eps 1e-15, betas [.9,.99]}, lotd_neus.dtu.230814.yaml:178-184) on f32 master params;
 * p16 (may be NULL) receives the fp16 copy used by the kernels; grad is scaled by grad_scale; zero_grad bit 0: the gradient is
 * zeroed; bit 1 (opt-in, SURVEY sec. 8f-3 "Adam only on touched hash entries"): entries whose gradient is exactly 0 this step
 * are skipped entirely -- no moment decay, no update (torch.optim.SparseAdam's rule; NOT the reference's dense optimizer). */
int nsim_adam_step(float* p, void* p16, float* grad, float* m, float* v, int64_t n, float lr, float beta1,
                   float beta2, float eps, float bias1, float bias2, float grad_scale, int zero_grad,
                   void* stream);

/* The same update for up to NSIM_ADAM_MULTI_MAX small tensors in one launch (the decoder weights / biases, inv_s and
 * appearance codes of a step); per tensor: its own betas / bias corrections and a learning-rate factor. */
#define NSIM_ADAM_MULTI_MAX 12
typedef struct {
  float* p;
  void* p16;        /* may be NULL */
  float* grad;
  float* m;
  float* v;
  int64_t n;
  float beta1, beta2, bias1, bias2, lr_scale;
} NsimAdamTensor;
int nsim_adam_multi(const NsimAdamTensor* tensors, int n_tensors, float lr, float eps, float grad_scale, int zero_grad,
                    void* stream);

/* ------------------------------------------------------------------------------- marching cubes */
/* nr3d_lib.graphics.trianglemesh.extract_mesh (code_single/tools/extract_mesh.py:124): the surface {value = level} of a lattice
 * of SDF values, one z-slab at a time (neuralsim_amd/mesh.py; conventions in csrc/misc.hip).  A slab is lat f32
 * [nzs + 1][ny][nx] (x fastest), lattice point (i, j, k) at (bx, by, bz) + h (i, j, k0 + k); below / above (may be NULL) are
 * the single planes next to it.  bpp = ceil(nx ny / 256) blocks per plane.
 *   count:      cnt_v int32 [(nzs + 1) 2 bpp] (plane k: x/y-edge vertices of its blocks, then z-edge vertices),
 *               cnt_t int32 [(nzs + 1) bpp] (triangles of the cubes with their origin in the block);
 *   scan:       both in place -> exclusive offsets; totals int32 [3] = {vertices before plane nzs's x/y edges,
 *               all vertices of the slab, triangles};
 *   emit_verts: vid int32 [3][nzs + 1][ny nx] = vbase + slab-local id of the x / y / z edge vertex of every point (-1: none);
 *               verts / normals f32 [totals[0] (+ plane nzs's x/y vertices when emit_top)][3];
 *   emit_tris:  faces int32 [totals[2]][3] (global vertex ids from vid). */
int nsim_mc_count(const float* lat, int64_t nx, int64_t ny, int64_t nzs, float level, int32_t* cnt_v, int32_t* cnt_t,
                  void* stream);
int nsim_mc_scan(int32_t* cnt_v, int32_t* cnt_t, int64_t nx, int64_t ny, int64_t nzs, int32_t* totals, void* stream);
int nsim_mc_emit_verts(const float* lat, const float* below, const float* above, int64_t nx, int64_t ny, int64_t nzs,
                       float level, float bx, float by, float bz, float h, int64_t k0, int64_t vbase, int emit_top,
                       const int32_t* off_v, int32_t* vid, float* verts, float* normals, void* stream);
int nsim_mc_emit_tris(const float* lat, int64_t nx, int64_t ny, int64_t nzs, float level, const int32_t* off_t,
                      const int32_t* vid, int32_t* faces, void* stream);

/* --------------------------------------------------------------------------- nearest neighbours */
/* nr3d_lib.maths.chamfer_distance (code_single/tools/eval_lidar.py:417-421): exact nearest neighbour of every x[i] in y, both f32
 * [.][3] (neuralsim_amd/pointcloud.py; conventions in csrc/misc.hip).  d2[i] = min_j ((dx dx + dy dy) + dz dz) in f32,
 * idx[i] = the lowest j that attains it; non-finite points of y are never selected; a non-finite query or an empty y gives
 * d2 = +inf, idx = -1.  Both paths return the same bits.
 *   brute:      exhaustive.  qlist (may be NULL: all N queries) = int32 indices of the queries to search, their number read
 *               from *nq on the device.  nsplit > 1 spreads y over that many workgroups per query block; part_d2 f32 /
 *               part_idx int32 [nsplit][N] then hold the partial results, combined by a second launch.
 *   grid_count: hdr int32 [32] (written here: bounding box, cell size and resolution, counters; hdr[7] = the number of queries
 *               grid_query handed to the exhaustive pass), cell_cnt int32 [max_cells + 1] (points per cell), cell_of / rank
 *               int32 [M] (cell of every point, -1 when not finite, and its rank inside the cell).  target_occ = the mean
 *               number of points per occupied cell the cell size aims at.
 *   grid_scan:  cell_cnt in place -> exclusive offsets.
 *   grid_fill:  rec [M][4] 16-byte records (x, y, z f32, index int32) of y's finite points in cell order.
 *   grid_query: rings of cells around each query's cell until the best distance is strictly below the distance to the
 *               unvisited cells, at most max_rings rings; the queries still open are appended to left_list int32 [N]
 *               (count in hdr[7]) for nsim_nn_brute(..., qlist = left_list, nq = hdr + 7, ...). */
int nsim_nn_brute(const float* x, int64_t N, const float* y, int64_t M, const int32_t* qlist, const int32_t* nq, int64_t nsplit,
                  float* part_d2, int32_t* part_idx, float* d2, int32_t* idx, void* stream);
int nsim_nn_grid_count(const float* y, int64_t M, float target_occ, int64_t max_cells, int32_t* hdr, int32_t* cell_cnt,
                       int32_t* cell_of, int32_t* rank, void* stream);
int nsim_nn_grid_scan(const int32_t* hdr, int32_t* cell_cnt, void* stream);
int nsim_nn_grid_fill(const float* y, int64_t M, const int32_t* cell_off, const int32_t* cell_of, const int32_t* rank, float* rec,
                      void* stream);
int nsim_nn_grid_query(const float* x, int64_t N, const float* rec, const int32_t* cell_off, int32_t* hdr, int max_rings, float* d2,
                       int32_t* idx, int32_t* left_list, void* stream);

/* ------------------------------------------------------------- error-map importance sampling of training pixels */
/* nr3d_lib.models.importance ``ErrorMap`` / ``ImpSampler`` (built per camera by code_single/tools/train.py:105-138; config block
 * ``training.error_map{error_map_hw, frac_uniform, min_pdf, max_pdf, n_steps_max}``, lotd_neus.dtu.230814.yaml:316-320).  The map
 * is em f32 [n_images, h, w]; every entry point rejects n_images h w >= 2^31.
 *
 * ErrorMap.step_error_map(i, xy, val) (train.py:678-688; the error is the per-ray photometric term of
 * app/loss/photometric.py:111-112, 146), first half: ray r falls into the cell cx = clamp(int(x w), 0, w - 1), cy = clamp(int(y h),
 * 0, h - 1) of frame fidx[r * fidx_stride] (fidx_stride 0: one frame for every ray, 1: per ray); its error is added to
 * sum [n_images h w] and 1 to cnt [n_images h w] with f32 atomics (both zero on entry) and touched [n_images] (int32, zero on
 * entry) is set for its frame.  The error is val [N], or -- val NULL -- mean_c fn(pred - gt) of pred / gt [N,3] with fn 0 = mse,
 * 1 = l1, computed here so that a training chain needs no launch of its own for it; err_out [N] (may be NULL) receives it.  Rays
 * of a frame outside [0, n_images) are not accounted. */
int nsim_errmap_accumulate(const int64_t* fidx, int64_t fidx_stride, const float* xy, const float* val, const float* pred,
                           const float* gt, int fn, int64_t N, int64_t n_images, int h, int w, float* sum, float* cnt,
                           int32_t* touched, float* err_out, void* stream);
/* ... second half: cells with cnt > 0 become 0.5 em + 0.5 sum / cnt, every other cell keeps its bits; the consumed cells of sum /
 * cnt are zeroed again, n_steps [n_images] (int64) is incremented for every touched image and the flags are cleared. */
int nsim_errmap_blend(float* em, float* sum, float* cnt, int32_t* touched, int64_t* n_steps, int64_t n_images, int h, int w,
                      void* stream);
/* ErrorMap.get_pdf + get_pdf_image, as the tables ImpSampler.sample_img_pixel / sample_pixel (dataio/data_loader/
 * pixel_loader.py:157-171, 280-302) draw from.  Per image: p = max(em, 0) + 1e-12; p /= sum p; p = max(p, min_pdf / (h w));
 * max_pdf >= 0: p = min(p, max(max_pdf, 1)); p /= sum p -> pdf_cell [n_images, h w] (may be NULL) and its inclusive scan
 * cdf_cell [n_images, h w], non-decreasing, last entry of every image exactly 1.  mass [n_images] = sum of em per image;
 * pdf_img [n_images] = mass / max(sum mass, 1e-12); cdf_img [n_images] = the inclusive scan of max(mass, 0) / sum max(mass, 0)
 * (equal shares when no image has mass), last entry exactly 1.  Any h w >= 1.  max_pdf < 0: no upper clamp. */
int nsim_errmap_cdf(const float* em, int64_t n_images, int h, int w, float min_pdf, float max_pdf, float* cdf_cell,
                    float* pdf_cell, float* mass, float* cdf_img, float* pdf_img, void* stream);
/* ImpSampler.sample_img_pixel (fixed_frame < 0) / sample_pixel (fixed_frame = the frame) from uniforms u f32 [., 4]: rows row0 ..
 * row0 + n - 1 of u, fidx_out (int64, may be NULL) and xy_out (f32 [., 2]) are served, so that several maps fill one batch.  The
 * first n_uni of them are uniform: fidx = min(int(u0 n_images), n_images - 1), xy = (u2, u3).  The others: image = the first i with
 * cdf_img[i] > u0, cell = the first c with cdf_cell[i][c] > u1 (both clamped to the last index), xy = ((cx + u2) / w,
 * (cy + u3) / h), kept inside its cell: int(x w) == cx and int(y h) == cy.  All xy are clamped to [1e-6, 1 - 1e-6]. */
int nsim_errmap_draw(const float* cdf_img, const float* cdf_cell, int64_t n_images, int h, int w, const float* u, int64_t n,
                     int64_t n_uni, int64_t fixed_frame, int64_t row0, int64_t* fidx_out, float* xy_out, void* stream);

/* ------------------------------------------------------------------------------- occupancy grids */
/* code_single/tools/extract_occgrid.py:93-147 (sign-change detection on sub-sampled voxels), on the lattice the voxels share
 * (neuralsim_amd/occgrid.py; conventions in csrc/misc.hip).  Voxel (ix, iy, iz) of a grid of res[3] voxels owns the (s + 1)^3
 * lattice points of per-axis indices i s .. i s + s; the lattice is f32 [res[0] s + 1][res[1] s + 1][res[2] s + 1], z fastest,
 * walked in slabs of nxs voxel layers in x (nxs s + 1 lattice planes).  1 <= s <= 4.
 *   points: replaces :123-135 and :106 -- object-space coordinates x_obj f32 [n_planes][LY][LZ][3] of the lattice planes j0 ..
 *           j0 + n_planes - 1, c = float(j / s) + float(j % s) / float(s), cn = (c / float(res)) * 2 - 1, x_world = cn * radius +
 *           center, x_obj = (R^T (x_world - trans)) / scale with the three products of a row added left to right, every
 *           operation rounded on its own, and state uint8 per point:
 *           0 inside [obj_min, obj_max] (to be queried), 1 outside (the tool's invalid_sdf = +inf), 2 pruned -- only with
 *           occ_bits (the bit-packed occupancy grid of occ, which spans the object box): the cell containing the point and its 26
 *           neighbours, clamped at the border, are all empty;
 *   flags:  replaces :137, :142 -- uint8 [nxs s + 1][ry][rz], the OR over the (s + 1)^2 points in y and z of: 1 = a value > 0,
 *           2 = a value that is not, 4 = an infinite value or (state, may be NULL) a point whose state is not 0 (its value is not
 *           read);
 *   count:  replaces :138-145 -- a voxel is occupied iff the OR of its s + 1 flag bytes along x is exactly 3; cnt int32
 *           [ceil(nxs ry rz / 256)] occupied voxels per block of 256 voxels (z fastest);
 *   scan:   cnt in place -> exclusive offsets, *total = their sum, also stored as (total, seq) to the host-mapped words notify
 *           (may be NULL) so that the host reads the size without a stream synchronisation;
 *   emit:   replaces :145-147 -- out int32 [total][3] = (ix0 + ix, iy, iz) in ascending (ix, iy, iz). */
typedef struct NsimOccgridFrame {
  int32_t res[3];
  int32_t s;
  float center[3], radius[3]; /* of the world box: (max + min) / 2, (max - min) / 2 */
  float rot[9];               /* object -> world rotation, row-major */
  float trans[3];
  float scale[3];
  float obj_min[3], obj_max[3];
} NsimOccgridFrame;
int nsim_occgrid_points(const NsimOccgridFrame* frame, int64_t j0, int64_t n_planes, const int32_t* occ_bits,
                        const NsimOccMeta* occ, float* x_obj, uint8_t* state, void* stream);
int nsim_occgrid_flags(const float* lat, const uint8_t* state, int64_t nxs, int64_t ry, int64_t rz, int s, uint8_t* flags,
                       void* stream);
int nsim_occgrid_count(const uint8_t* flags, int64_t nxs, int64_t ry, int64_t rz, int s, int32_t* cnt, void* stream);
int nsim_occgrid_scan(int32_t* cnt, int64_t n_blocks, int32_t* total, int64_t* notify, int64_t seq, void* stream);
int nsim_occgrid_emit(const uint8_t* flags, int64_t nxs, int64_t ry, int64_t rz, int s, int64_t ix0, const int32_t* off,
                      int32_t* out, void* stream);

/* --------------------------------------------------------------------------------- visible grids */
/* app/visible_grid.py (VisibleGrid) and code_multi/tools/extract_visible_grid.py:205-235: the voxels the cameras saw
 * (neuralsim_amd/visible_grid.py; conventions in csrc/misc.hip).  The grid is the cube [origin, origin + G voxel], G = 2^depth,
 * 32 <= G <= 1024; voxel index = ix G G + iy G + iz (visible_grid.py:28-30, z fastest), int64.  hits: int32 [G^3] in that order;
 * bit sets: uint32 [G^3 / 32] stored as int32, bit (v & 31) of word (v >> 5).
 *   mark_samples: replaces extract_visible_grid.py:221-226 and visible_grid.py:88-89,119-121 in one pass -- for every sample s
 *           with w[s] > thre (strict; NaN is not greater) of pack row p (pack_infos_hit int64 [n_packs][2] = (start, length),
 *           starts non-decreasing) the point rays_o[r] + rays_d[r] * t[s], r = rays_inds_hit[p] (NULL: r = p; rows outside
 *           [0, n_rays) are skipped), counts iff box_min <= point <= box_max; hits[voxel] += 1 with voxel coordinate
 *           int((point - origin) / voxel) clamped to G - 1, every operation rounded on its own;
 *   mark_points: the same for points f32 [n][3] (visible_grid.py:83-91);
 *           stats (may be NULL): int64 [2] += (points counted, atomics issued after the in-wave run merge);
 *   bits:   bit v = hits[v] > 0;   set_bits: bit idx[i] = 1 for 0 <= idx[i] < G^3 (visible_grid.py:149);
 *   morph:  out = op(in) | keep (keep may be NULL or out; in != out), op 0 = 3x3x3 dilation with out-of-grid neighbours dropped,
 *           1 = 3x3x3 erosion with out-of-grid neighbours empty (visible_grid.py:166-215 on the 26-neighbourhood of :236-245);
 *   count:  cnt[b] = set bits of the 256 words of block b, ceil(G^3 / 8192) blocks -> nsim_occgrid_scan -> emit: out_idx int64
 *           [total] ascending (visible_grid.py:157-164), out_hits (may be NULL) = hits at them (hits NULL: 0);
 *   occ_val: f32 [G^3] in the occupancy grids' order (x fastest) = 1.0 where the bit is set, 0.0 elsewhere. */
typedef struct NsimVgridFrame {
  float origin[3], voxel[3];
  float box_min[3], box_max[3]; /* the space's box: ``space.contains`` */
  int32_t G;
} NsimVgridFrame;
int nsim_vgrid_mark_samples(const NsimVgridFrame* frame, const float* rays_o, const float* rays_d, int64_t n_rays,
                            const int64_t* rays_inds_hit, const int64_t* pack_infos_hit, int64_t n_packs, const float* t,
                            const float* w, int64_t S, float thre, int32_t* hits, int64_t* stats, void* stream);
int nsim_vgrid_mark_points(const NsimVgridFrame* frame, const float* pts, int64_t n, int32_t* hits, int64_t* stats, void* stream);
int nsim_vgrid_bits(const int32_t* hits, int64_t G, int32_t* bits, void* stream);
int nsim_vgrid_set_bits(const int64_t* idx, int64_t n, int64_t G, int32_t* bits, void* stream);
int nsim_vgrid_morph(const int32_t* in, const int32_t* keep, int64_t G, int op, int32_t* out, void* stream);
int nsim_vgrid_count(const int32_t* bits, int64_t G, int32_t* cnt, void* stream);
int nsim_vgrid_emit(const int32_t* bits, int64_t G, const int32_t* off, const int32_t* hits, int64_t* out_idx, int64_t* out_hits,
                    void* stream);
int nsim_vgrid_occ_val(const int32_t* bits, int64_t G, float* occ_val, void* stream);

/* --------------------------------------------------------------------------------- simulated LiDAR sensors */
/* The ``Lidar`` observer node and the tools that render its sweeps (neuralsim_amd/lidar_sim.py).
 *   raygen: replaces Lidar.get_all_rays, app/resources/observers/lidars.py:208-232 (meshgrid, four sin / cos tensors, three
 *           broadcast products, normalize, tile).  mode 0 (grid): N = n_beams n_az rays, ray r = i n_beams + j takes phis[i]
 *           and thetas[j] -- the flatten order of meshgrid(thetas, phis, indexing='xy'), lidars.py:218, 432, beam fastest;
 *           mode 1 (paired, n_beams == n_az == N): ray r takes (thetas[r], phis[r]), lidars.py:494-504, 566-588.
 *           l2w f32 [3][4] row-major ON THE DEVICE = the caller's world_transform x carla_to_opencv (lidars.py:188-192, 211),
 *           columns X, Y, Z, T; it may carry a scale.  rays_d[r] = normalize((a X + b Y) + c Z), every product and sum rounded on
 *           its own, normalize = d / max(|d|, 1e-12); (a, b, c) = (sinT cosP, sinT sinP, cosT) for axis 0 (lidars.py:226-227),
 *           (cosT, sinT sinP, -(sinT cosP)) for axis 1 (lidars.py:221-224); rays_o[r] = T; theta_phi (may be NULL) f32 [N][2] =
 *           the two angles of ray r.  N = 0 launches nothing.  60: see nsim_strerror.
 *   returns_count / nsim_occgrid_scan / returns_emit: replace the mask and the masked gathers of code_multi/tools/render.py:
 *           331-346 (and :298-313) by a stable compaction.  Ray r is a return iff acc[r] > thresh (strict, f32; NaN is not).
 *           count: cnt[b] = returns among the 256 rays of block b, ceil(N / 256) blocks; the scan turns cnt into offsets (and
 *           stores the total M to its host-mapped notify words); emit writes, for the M returns in ray order: ray_inds int64,
 *           ranges = depth[r], mask = acc[r], pts_world [M][3] = rays_o[r] + rays_d[r] * depth[r] (one multiply, then one add),
 *           pts_local [M][3] (may be NULL) with w2l f32 [3][4] row-major on the device, component k summed in the FIXED order
 *           ((w2l[k][0] x + w2l[k][1] y) + w2l[k][2] z) + w2l[k][3], (x, y, z) = pts_world; out_rgb [M][3] = rgb[r] and out_ids
 *           int64 [M] = ids[r] (``ins_seg_mask_buffer``) when non-NULL; range_image (may be NULL) f32 [N] = depth[r] on a
 *           return, 0 elsewhere.  Nothing past row M is written.  61: see nsim_strerror. */
int nsim_lidar_raygen(const float* thetas, const float* phis, int64_t n_beams, int64_t n_az, int mode, int axis, const float* l2w,
                      float* rays_o, float* rays_d, float* theta_phi, void* stream);
int nsim_lidar_returns_count(const float* acc, int64_t N, float thresh, int32_t* cnt, void* stream);
int nsim_lidar_returns_emit(const float* acc, const float* depth, const float* rays_o, const float* rays_d, int64_t N, float thresh,
                            const int32_t* off, const float* w2l, const float* rgb, const int64_t* ids, int64_t* ray_inds,
                            float* ranges, float* mask, float* pts_world, float* pts_local, float* out_rgb, int64_t* out_ids,
                            float* range_image, void* stream);

/* --------------------------------------------------------------------------------- LiDAR ground-truth filter */
/* SceneDataLoader.filter_lidar_gts / _filter_lidar_gts (dataio/data_loader/base_loader.py:649-844) and Camera / MultiCamBundle
 * .project_pts_in_image (app/resources/observers/cameras.py:397-446, 537-538), behind neuralsim_amd/lidar_filter.py.  The
 * reference's four sequential filters (each a mask, a nonzero and a gather of every column) are one conjunction per point.
 * Every product is rounded before its sum and every 3-term sum runs left to right.
 *   world point   p_local = rays_o + rays_d * range (one multiply, one add: torch.addcmul, base_loader.py:700, 709);
 *                 p[k] = ((R[k][0] x + R[k][1] y) + R[k][2] z) + t[k] with (R, t) = l2w[fi[r]][li[r]], l2w f32 [F][L][3][4];
 *                 li, fi int64 [N] (NULL: 0).  A point whose index is outside [0, L) / [0, F) is not kept and reads no table.
 *   filter_valid  (non-zero) keep iff range > 0 (base_loader.py:748-751; NaN and -0.0 are not kept).
 *   cameras       (C > 0; base_loader.py:753-787) cams f32 [F][C][24] on the device, a record = c2w [3][4], fx, skew, cx, fy,
 *                 cy, W, H (as floats, after any downscale), five distortion coefficients; cam_models int32 [C] ON THE HOST, one
 *                 id per camera of the rig (0 pinhole, 1 OpenCV k1 k2 p1 p2 k3, 2 fisheye k1..k4), C <= 32.  q = p - t_c,
 *                 cam[k] = (R_c[0][k] q0 + R_c[1][k] q1) + R_c[2][k] q2; (u, v, d) operation for operation as the ``proj`` of
 *                 nr3d_lib/models/attributes (pinhole :511-520, OpenCV :565-579, fisheye :619-632: the |z| < 1e-9 -> 1e-9 guard
 *                 and the skew term included); in view iff d > near_clip and 0 <= u < W and 0 <= v < H; with ignore u8
 *                 [F][C][Hm][Wm] (non-zero: ignored; padded bottom / right with 0) additionally ignore[(int)v][(int)u] == 0,
 *                 read only after the view test passed (a pixel outside [Hm][Wm] counts as padding).  Keep iff any camera of
 *                 the point's frame has it in view.
 *   aabb          (non-NULL; base_loader.py:789-800) f32 [2][3] on the device: keep iff min[k] <= p[k] <= max[k] for all k.
 *   boxes         (B > 0; base_loader.py:802-842) f32 [B][15] = a [3][4] transform and 3 sizes; the boxes of frame f are rows
 *                 box_offsets[f] .. box_offsets[f + 1] (int32 [F + 1] on the device); b = R_b^T (p - t_b) as above; inside iff
 *                 -s[k] / 2 <= b[k] <= s[k] / 2 for all k; keep iff inside no box.
 *   count: keep u8 [N] and cnt[b] = kept among the 256 points of block b, ceil(N / 256) blocks; nsim_occgrid_scan turns cnt
 *   into offsets; emit compacts, in point order, rays_o, rays_d, ranges and (where the output is non-NULL) li, fi, keep_inds
 *   int64 (the kept points' indices) and pts_world [M][3] (the world point above).  project: the dense projection of N world
 *   points into C cameras of ONE frame through the same device function as the filter: mask u8, u, v, d f32, all [C][N]
 *   (ignore u8 [C][Hm][Wm] or NULL).  N = 0 (and C = 0 for project) launch nothing.  62: see nsim_strerror. */
int nsim_lidar_filter_count(const float* rays_o, const float* rays_d, const float* ranges, const int64_t* li, const int64_t* fi,
                            int64_t N, const float* l2w, int64_t L, int64_t F, int filter_valid, const float* cams,
                            const int32_t* cam_models, int64_t C, float near_clip, const uint8_t* ignore, int64_t Hm, int64_t Wm,
                            const float* aabb, const float* boxes, const int32_t* box_offsets, int64_t B, uint8_t* keep,
                            int32_t* cnt, void* stream);
int nsim_lidar_filter_emit(const uint8_t* keep, const int32_t* off, const float* rays_o, const float* rays_d, const float* ranges,
                           const int64_t* li, const int64_t* fi, int64_t N, const float* l2w, int64_t L, int64_t F,
                           float* out_rays_o, float* out_rays_d, float* out_ranges, int64_t* out_li, int64_t* out_fi,
                           int64_t* keep_inds, float* pts_world, void* stream);
int nsim_cam_project(const float* pts, int64_t N, const float* cams, const int32_t* cam_models, int64_t C, float near_clip,
                     const uint8_t* ignore, int64_t Hm, int64_t Wm, uint8_t* mask, float* u, float* v, float* d, void* stream);

/* MFMA layout self-test (tests only): writes D = A(32x16 f16) * B(16x32 f16) with the wrappers used by the
 * field kernels; a, b given in plain row-major. d is 32x32 f32 row-major. */
int nsim_selftest_mfma(const float* a, const float* b, float* d, int use_f32, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NSIM_H */
