/*
 * jt_render.h -- C ABI of the MI355X (gfx950) TensoRF-VM joint pose + radiance-field renderer.
 *
 * The reference (Nemo1999/Joint-TensoRF) is pure Python/PyTorch and has no FFI of its own
 * (SURVEY.md §8(b)); its seam is the duck-typed scene class reached through
 * `getattr(tensorf_repr, opt.arch.tensorf.model)` (model/tensorf.py:375-397) and its
 * `forward(...)` (model/tensorf_repr/batBase.py:44-165).  This header is the boundary a
 * maintainer binds instead of the stock torch ops on that path; every entry point names the
 * reference code it replaces (paths relative to the reference repo root).
 *
 * Conventions
 *   - plain C: raw DEVICE pointers, sizes, a hipStream_t passed as void*; no torch types.
 *   - every function returns 0 on success, JT_ERR_* (>0) on bad arguments, or the negated
 *     hipError_t of a failed launch.  No exceptions, no hidden allocation, no internal
 *     threads, no host synchronisation: re-entrant per stream and hipGraph-capturable.
 *   - VM factors are CHANNEL-LAST: plane i is [H_i][W_i][C] floats (logical torch tensor
 *     [1,C,H,W] = [1,C,g[m1],g[m0]], tensoRF.py:165), line i is [L_i][C] (logical [1,C,g[v],1]).
 *     matMode = {{0,1},{0,2},{1,2}}, vecMode = {2,1,0} (tensorBase.py:405-406).
 *   - rays are [R][3] fp32 (origins, un-normalised directions), outputs [R][3] / [R].
 *   - gradient buffers are ACCUMULATED into (atomics); the caller zeroes them.
 */
#ifndef JT_RENDER_H
#define JT_RENDER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever a struct layout, an argument list or what an argument must point to changes (round 4 added
 * JtScene.near_plane_dev and grew the regulariser scratch to 640 floats without bumping it: a caller built against the old
 * header would have handed over a shorter struct).  jt_version() returns the value the LIBRARY was built with; the Python
 * binding refuses to load a library whose version differs from the one it was written against (joint_tensorf_amd/_lib.py:
 * JT_ABI_VERSION).  include/jt_render.abi holds a hash of every prototype, struct and constant of this header next to the
 * version it was taken at: tests/test_abi.py fails when the hash changes without this number changing (round 5 added
 * jt_reg_losses_fused, removed jt_pose_fused* and redefined matrix-mode bit 2 at version 1100; 1200 = round 6: those changes,
 * jt_shade_lean_tape / jt_shade_set_lean_tape, the workspace no longer carries the tile lists unless that variant is selected;
 * 1201: + jt_chip_geometry; 1202: + jt_shade_workspace_layout; 1203: + jt_march_forward_pose / jt_march_backward_pose; 1204: +
 * jt_lattice_indices; 1205: + jt_ssim_forward / jt_ssim_workspace_bytes; 1206: +
 * jt_image_ingest / jt_image_ingest_workspace_bytes; 1207: + jt_shade_backward_plan / jt_march_backward_plan; 1208: + jt_mesh_count / jt_mesh_emit;
 * 1209: + jt_components_init / jt_components_sweep / jt_component_sizes, jt_density_gradient, JT_COMPONENTS_TILE; 1210: +
 * jt_raster_project / jt_raster_draw / jt_raster_resolve, JT_RASTER_*; 1211: + jt_mesh_unwarp_ndc / jt_mesh_filter_count / jt_mesh_filter_emit,
 * JT_UNWARP_*; 1212: + jt_simplify_keys / jt_simplify_clusters / jt_simplify_triangles, JT_SIMPLIFY_*; 1213: + jt_texture_texels /
 * jt_texture_pack / jt_raster_resolve_texture, JT_TEXTURE_*; 1214: + jt_visible_tally / jt_visible_fold / jt_visible_mark /
 * jt_visible_spread / jt_mesh_select_count; 1215: + jt_conv_packed_floats / jt_conv_pack_weights / jt_conv2d_relu_forward /
 * jt_maxpool_3x3s2_forward / jt_lpips_workspace_bytes / jt_lpips_feature_layout / jt_lpips_forward, JtLpipsWeights, JT_CONV_*;
 * 1216: + jt_fusion_integrate / jt_fusion_finish.  Additions bump the last two digits, anything a caller built against the old header
 * would get wrong bumps the hundreds). */
#define JT_VERSION 1216

#define JT_OK 0
#define JT_ERR_ARG 1         /* null pointer / bad size */
#define JT_ERR_UNSUPPORTED 2 /* shape outside what the kernels are instantiated for */

#define JT_ACT_SOFTPLUS 0 /* softplus(x + shift)  tensorBase.py:696-698 */
#define JT_ACT_RELU 1     /* relu(x + shift)      tensorBase.py:699-700 */

#define JT_MLP_FEA 0      /* MLPRender_Fea          tensorBase.py:101-126 */
#define JT_MLP_WEAKVIEW 1 /* MLPRender_Fea_WeakView tensorBase.py:180-214 */

#define JT_SHADE_POSE_ONLY 2  /* jt_shade_forward flags: the backward of this forward will be called without
                                 g_factors and g_mlp (test-time pose optimisation); only the records that
                                 backward reads are written */
#define JT_SHADE_SKIP_WGRAD 1 /* jt_shade_backward flags: leave out the MLP/basis weight-gradient pass
                                 (kernel timing probes only; g_mlp is then not written) */

/* Scene / call description: 4-byte fields only (mirrored 1:1 by ctypes in joint_tensorf_amd/_lib.py).
 * Replaces the TensorBase attributes set in tensorBase.py:430-488 plus the per-call keyword
 * arguments of BatBase.forward (batBase.py:44). */
typedef struct JtScene {
  float aabb_lo[3];
  float aabb_hi[3];
  int32_t plane_h[3];   /* rows  of plane i as stored (g[m1]; swapped when the reference's    */
  int32_t plane_w[3];   /* cols  non-cubic blur quirk is reproduced)         */
  int32_t line_len[3];  /* g[v]                                                               */
  int32_t n_comp_density; /* channels of every density plane/line (16 in both BAT yamls)      */
  int32_t n_comp_app;     /* channels of every appearance plane/line (48 Blender, 20 LLFF)    */
  float step_size;      /* tensorBase.py:484                                                  */
  float near_plane;     /* near_far[0]                                                        */
  float far_plane;      /* near_far[1]                                                        */
  float distance_scale; /* batBase.py:122                                                     */
  float density_shift;
  int32_t density_act;  /* JT_ACT_*                                                           */
  float weight_thres;   /* rayMarch_weight_thres, batBase.py:127                              */
  int32_t n_samples;    /* N_samples                                                          */
  int32_t ndc;          /* 1: sample_ray_ndc semantics (tensorBase.py:554-571, batBase.py:61-66) */
  int32_t white_bg;     /* resolved `white_bg or (is_train and coin<0.5)` batBase.py:154      */
  int32_t app_dim;      /* basis_mat rows (27 / 20)                                           */
  int32_t mlp_kind;     /* JT_MLP_*                                                           */
  int32_t mlp_hidden;   /* featureC (64 / 32)                                                 */
  int32_t view_pe;
  int32_t fea_pe;
  float view_pe_progress;
  float fea_pe_progress;
  /* alpha-mask volume (AlphaGridMask, tensorBase.py:80-98), used when JtFactors.alpha_volume != NULL:
   * samples whose trilinear mask value is not > 0 are dropped (batBase.py:76-82). */
  int32_t mask_dims[3]; /* the volume's gridSize (x, y, z); the tensor is [z][y][x]                      */
  float mask_lo[3];     /* its own box: aabb[0]                                                         */
  float mask_inv[3];    /* 1.0 / (aabb[1] - aabb[0]) * 2, rounded like AlphaGridMask.invgridSize        */
  /* optional (NULL = use near_plane): one float in DEVICE memory holding near_far[0] for the depth map's
   * "- near_far[0] + 0.05" (batBase.py:147-150).  A launch captured into a hipGraph keeps reading the current
   * value while tensorf_near_plane_schedule (model/tensorf.py:230-232) moves the near plane between replays. */
  const float* near_plane_dev;
} JtScene;

/* the 12 VM factor tensors (or their gradients) */
typedef struct JtFactors {
  float* density_plane[3];
  float* density_line[3];
  float* app_plane[3];
  float* app_line[3];
  const float* alpha_volume; /* optional alpha-mask volume [z][y][x] (0 / 1 floats); NULL = no mask; ignored in
                                gradient structs */
} JtFactors;

/* basis_mat.weight [app_dim][3*n_comp_app] and the render MLP (torch Linear layout [out][in]) */
typedef struct JtMlp {
  float* basis;
  float* w1;
  float* b1;
  float* w2;
  float* b2;
  float* w3;
  float* b3;
} JtMlp;

int jt_version(void);
/* {compute units, XCDs} of the current device as the library sees them (hipDeviceGetAttribute, once per device).  The
 * persistent kernels -- shade forward / backward chain / scatter, the density walk -- run one workgroup per CU or a fixed
 * fraction of the CUs: their grids are derived from these two numbers (256 and 8 on a full MI355X; 32 and 1 on a CPX
 * partition), not from constants. */
int jt_chip_geometry(int32_t* out2);

/* ---------------------------------------------------------------------------------------------
 * Ray generation for the SAMPLED pixels only.
 * Replaces camera.get_center_and_ray (camera.py:231-261) + `[:,ray_idx]` (model/tensorf.py:159-161)
 * and, when `ndc` != 0, camera.convert_NDC (camera.py:303-340).
 *   pose [B][12] (3x4 row-major, world->camera), intr_inv [B][9], intr [B][9] (NDC only, may be
 *   NULL otherwise), ray_idx [r] int64 flat pixel index y*W+x (same lattice for every view).
 *   out: rays_o, rays_d [B*r][3].
 * backward: g_rays_o/g_rays_d [B*r][3] -> g_pose [B][12] (overwritten, deterministic per view). */
int jt_raygen_forward(const float* pose, const float* intr_inv, const float* intr, const int64_t* ray_idx,
                      int n_views, int rays_per_view, int image_w, int ndc, float ndc_near,
                      float* rays_o, float* rays_d, void* stream);
int jt_raygen_backward(const float* pose, const float* intr_inv, const float* intr, const int64_t* ray_idx,
                       int n_views, int rays_per_view, int image_w, int ndc, float ndc_near,
                       const float* g_rays_o, const float* g_rays_d, float* g_pose, void* stream);
/* Flat pixel indices of the `all_view_rand_grid` lattice (model/nerf.py:660-667: x = ox + i * step, y = oy + j * step, index
 * y * image_w + x, row-major over (j, i)) with the two offsets read from DEVICE memory (offsets: int32[2]) -- the form a replayed
 * hipGraph needs: the host draws ox, oy per iteration and pokes them in front of the replay.  ray_idx: [ny * nx] int64. */
int jt_lattice_indices(const int32_t* offsets, int step, int nx, int ny, int image_w, int64_t* ray_idx, void* stream);
/* The same for a RAGGED batch of views (batched test-time pose optimisation of model/bat.py:265-292: every held-out view on its own
 * pixel lattice): ray_idx [n_rays] is the concatenation of the views' pixel lists, view b owns rays view_offset[b] ..
 * view_offset[b + 1] - 1 (view_offset [n_views + 1], int32, device memory).  Per ray / per view the arithmetic and the order of
 * the sums are those of a single-view call: a view's rays and pose gradient do not depend on what else is in the batch. */
int jt_raygen_forward_ragged(const float* pose, const float* intr_inv, const float* intr, const int64_t* ray_idx,
                             const int32_t* view_offset, int n_views, int n_rays, int image_w, int ndc, float ndc_near,
                             float* rays_o, float* rays_d, void* stream);
int jt_raygen_backward_ragged(const float* pose, const float* intr_inv, const float* intr, const int64_t* ray_idx,
                              const int32_t* view_offset, int n_views, int n_rays, int image_w, int ndc, float ndc_near,
                              const float* g_rays_o, const float* g_rays_d, float* g_pose, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Learnable pose: pose = exp(se3) o noise o gt.
 * Replaces bat.Graph.get_pose train branch (model/bat.py:341-353), Lie.se3_to_SE3 with the
 * nth=8 Taylor series (camera.py:81-99,122-145) and Pose.compose_pair (camera.py:50-57).
 *   se3 [B][6]; noise [B][12] or NULL; gt [B][12] (gt_stride 12) or one [12] shared (gt_stride 0).
 * backward: g_pose [B][12] -> g_se3 [B][6] (overwritten). */
int jt_pose_forward(const float* se3, const float* noise, const float* gt, int gt_stride, int n_views,
                    float* pose, void* stream);
int jt_pose_backward(const float* se3, const float* noise, const float* gt, int gt_stride, int n_views,
                     const float* g_pose, float* g_se3, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Separable 1-D blur of a channel-last factor, replicate padding, cross-correlation.
 * Replaces BAT_VMSplit.convolute_plane / convolute_line (bateRF.py:8-39); taps come from
 * kernels.get_gaussian_kernel (kernels.py:16-22), n_taps odd (65 for c2f_kernel_size 64).
 *   in/out [H][W][C]; a line is H = L, W = 1 (only the H pass runs).  tmp: H*W*C floats scratch.
 * backward is the exact adjoint (g_out -> g_in, overwritten). */
int jt_blur_forward(const float* in, float* out, float* tmp, int H, int W, int C, const float* taps, int n_taps,
                    void* stream);
int jt_blur_backward(const float* g_out, float* g_in, float* tmp, int H, int W, int C, const float* taps,
                     int n_taps, void* stream);

/* The same for up to 12 factors at once (all VM factors of a scene: BAT_VMSplit.forward blurs every plane and
 * line before rendering, bateRF.py:41-130): two launches per direction instead of three per factor.  For the
 * backward `in` is g_out and `out` is g_in. */
typedef struct JtBlurItem {
  const float* in;
  float* out;
  float* tmp;        /* H*W*C floats scratch for planes, may be NULL for lines */
  const float* taps;
  int32_t H, W, C, n_taps;
} JtBlurItem;
int jt_blur_batch_forward(const JtBlurItem* items, int n_items, void* stream);
int jt_blur_batch_backward(const JtBlurItem* items, int n_items, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Staged renderer (forward).  Replaces BatBase.forward (batBase.py:44-165) and everything it
 * calls: sample_ray / sample_ray_ndc (tensorBase.py:554-612), compute_densityfeature
 * (bateRF.py:41-94), feature2density (tensorBase.py:696-700), raw2alpha (tensorBase.py:57-65),
 * compute_appfeature (bateRF.py:97-130), basis_mat (tensoRF.py:156), MLPRender_Fea[_WeakView]
 * (tensorBase.py:101-126,180-214) and the compositing tail (batBase.py:142-165).
 *
 * jt_march_forward: sampling + density + transmittance scan.
 *   jitter: [R] one uniform draw per ray (tensorBase.py:592-596) or NULL; NDC: zvals [S] holds the
 *   (jittered) linspace row shared by all rays (tensorBase.py:557-559), jitter ignored.
 *   out: sigma_feat [R][S], weight [R][S], tmin [R], shade_count [R], shade_offset [R+1]
 *   (exclusive scan; [R] = number of shaded samples), shade_idx [R][S] uint16 (sample indices with
 *   weight > thres, in order), opacity [R], depth [R] (batBase.py:147-151).
 * jt_shade_list: entry -> (ray, sample) map + the positions the appearance path needs.
 *   out: entry_ray [n], entry_smp [n] (int32), viewdirs [n][3] (normalised when ndc).
 * jt_shade_forward (fused, MFMA): prod -> basis -> MLP -> sigmoid, rgb_s [n][3].
 * jt_composite_forward: rgb [R][3] = sum_k w_k c_k (+ white bg) clamped, clamp_mask [R] bit ch
 *   set when the un-clamped value lies in [0,1]. */
/* Opacity 1 - exp(-sigma * length) of one step at n arbitrary world points xyz [n][3] (masked points: 0).
 * Replaces BatBase.compute_alpha (batBase.py:27-41) under TensorBase.getDenseAlpha (tensorBase.py:618-634). */
int jt_dense_alpha(const JtScene* scene, const JtFactors* factors, const float* xyz, long n, float length,
                   float* alpha, void* stream);
/* Density feature and its WORLD-space gradient at n arbitrary world points xyz [n][3]: feat [n] (may be NULL) = the feature
 * before the shift and the activation, grad [n][3] = d feat / d xyz = (d feat / d normalised coordinate) * 2 / (hi - lo) per
 * axis.  The field of the factors themselves: the alpha mask is ignored, and a point beyond the box meets grid_sample's zero
 * padding (taps outside a factor count as zero values, the fractional weights stay).  One thread per point, one launch. */
int jt_density_gradient(const JtScene* scene, const JtFactors* factors, const float* xyz, long n, float* feat, float* grad,
                        void* stream);
int jt_march_forward(const JtScene* scene, const JtFactors* factors, const float* rays_o, const float* rays_d,
                     const float* jitter, const float* zvals, int n_rays, float* sigma_feat, float* weight,
                     float* tmin, int32_t* shade_count, int32_t* shade_offset, uint16_t* shade_idx,
                     float* opacity, float* depth, void* stream);
int jt_shade_list(const JtScene* scene, const float* rays_d, int n_rays, const int32_t* shade_offset,
                  const uint16_t* shade_idx, int32_t* entry_ray, int32_t* entry_smp, float* viewdirs,
                  int n_entries_max, void* stream);
int jt_composite_forward(const JtScene* scene, int n_rays, const int32_t* shade_offset,
                         const uint16_t* shade_idx, const float* weight, const float* rgb_s,
                         const float* opacity, float* rgb, int32_t* clamp_mask, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Staged renderer (backward) -- replaces autograd of all of the above (loss.all.backward(),
 * model/base.py:162; the scatter-adds of grid_sampler_2d_backward).
 * jt_composite_backward: g_rgb [R][3] -> g_rgb_s [n][3] (= weight * g_rgb masked by clamp).
 * jt_march_backward: density + transmittance backward:
 *   += g_factors.density_* (g_factors may be NULL: gradients w.r.t. the rays only); g_rays_o, g_rays_d
 *   [R][3] overwritten (include the app path's
 *   coordinate gradients read from g_xyz_app).  g_opacity [R] may be NULL.  workspace: caller-provided,
 *   jt_march_backward_workspace_bytes(scene, n_rays) bytes (per-sample density gradients + run lists + the rays'
 *   gradient sums in 2^48 fixed point: the runs of a ray meet in integer atomics, so g_rays_o / g_rays_d do not depend
 *   on the order in which they arrive -- the density part of a pose gradient is bit-reproducible in every mode). */
int jt_composite_backward(const JtScene* scene, int n_rays, const int32_t* shade_offset,
                          const int32_t* entry_ray, const int32_t* entry_smp, const float* weight,
                          const int32_t* clamp_mask, const float* g_rgb, float* g_rgb_s, int n_entries_max,
                          void* stream);
int jt_march_backward(const JtScene* scene, const JtFactors* factors, const float* rays_o, const float* rays_d,
                      const float* jitter, const float* zvals, int n_rays, const float* sigma_feat,
                      const float* weight, const float* tmin, const int32_t* shade_offset,
                      const uint16_t* shade_idx, const float* rgb_s, const int32_t* clamp_mask,
                      const float* g_rgb, const float* g_opacity, const float* g_xyz_app,
                      const JtFactors* g_factors, float* g_rays_o, float* g_rays_d, void* workspace,
                      size_t workspace_bytes, void* stream);
size_t jt_march_backward_workspace_bytes(const JtScene* scene, int n_rays);
/* The pair for a render of which only the RAYS want a gradient (test-time pose optimisation, model/bat.py:265-292: the scene is
 * frozen).  jt_march_forward_pose is jt_march_forward that also leaves d(density feature) / d(normalised coordinates) of every
 * in-box sample in dfeat_dn -- three planes of [n_rays * n_samples] floats (x, y, z), written while the taps of
 * compute_densityfeature (bateRF.py:41-94) are in registers; jt_march_backward_pose is jt_march_backward with g_factors = NULL
 * that reads them back instead of gathering the density factors a second time (same sums, same order per ray). */
int jt_march_forward_pose(const JtScene* scene, const JtFactors* factors, const float* rays_o, const float* rays_d,
                          const float* jitter, const float* zvals, int n_rays, float* sigma_feat, float* weight,
                          float* tmin, int32_t* shade_count, int32_t* shade_offset, uint16_t* shade_idx,
                          float* opacity, float* depth, float* dfeat_dn, void* stream);
int jt_march_backward_pose(const JtScene* scene, const JtFactors* factors, const float* rays_o, const float* rays_d,
                           const float* jitter, const float* zvals, int n_rays, const float* sigma_feat,
                           const float* weight, const float* tmin, const int32_t* shade_offset,
                           const uint16_t* shade_idx, const float* rgb_s, const int32_t* clamp_mask,
                           const float* g_rgb, const float* g_opacity, const float* g_xyz_app,
                           const float* dfeat_dn, float* g_rays_o, float* g_rays_d, void* workspace,
                           size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fused appearance path on the matrix cores (fp32 accuracy: fp32 MFMA, or bf16 MFMA on three-piece operands, see
 * jt_shade_matrix_mode):
 * gather(app planes/lines) -> outer product -> basis_mat -> PE -> MLP -> sigmoid, per shaded
 * sample, without materialising the [n][3*Ca] product matrix.
 * Replaces compute_appfeature + basis_mat + MLPRender_Fea[_WeakView].forward and their autograd.
 *   forward : rgb_s [n][3]; with workspace != NULL (training) it also leaves the per-sample layer inputs
 *             (products, basis output, hidden activations, ReLU masks, sample coordinates) in the workspace
 *   backward: g_rgb_s [n][3] -> += g_factors.app_*, += g_mlp.*, g_xyz_app [n][3] (overwritten); g_factors and /
 *             or g_mlp may be NULL when that group of gradients is not wanted (test-time pose optimisation,
 *             model/bat.py:265-292, only needs g_xyz_app); consumes the
 *             records the forward of the SAME samples left in `workspace` (the autograd tape of the chain:
 *             nothing is gathered or evaluated twice) and the forward's rgb_s
 * workspace: jt_shade_workspace_bytes(scene, n_entries_max) bytes, caller-provided; forward with
 *            workspace == NULL is the inference path (no records).
 * aux_stream / ev_fork / ev_join (hipStream_t / hipEvent_t, all three or none): when given, the MLP / basis
 * weight-gradient GEMMs are enqueued on aux_stream behind ev_fork (recorded on `stream` after the per-sample
 * kernels) and ev_join is recorded on aux_stream at their end; the caller makes whoever consumes g_mlp wait
 * for ev_join.  This lets the MFMA-bound GEMMs overlap the atomics-bound density backward.  ev_fork alone (no
 * aux_stream): recorded on `stream` behind the per-sample backward kernels, in front of the weight-gradient GEMMs
 * (a timing mark). */
size_t jt_shade_workspace_bytes(const JtScene* scene, int n_entries_max);
/* Where the pieces of that workspace sit under the library's current modes (chunk size, split mode, lean tape): byte offsets
 * from the workspace base and byte sizes, out23[0] = the total jt_shade_workspace_bytes reports, [1] the record array (offset
 * 0), [2] / [3] / [4] offset of the per-chunk weight-gradient slabs, bytes per chunk, chunks, [5] rows of a tile's record block,
 * [6] / [7] offset inside a chunk's slabs and maximal size of what the scatter's workgroups write when dBasis is formed there,
 * [8] whether the tile-owned scatter's lists are part of the workspace and, if so, (offset, bytes) of its seven pieces in
 * [9..22].  A diagnostic for tests (every piece must lie inside the total for any capacity); JT_ERR_ARG for n_entries_max < 1. */
int jt_shade_workspace_layout(const JtScene* scene, int n_entries_max, int64_t* out23);
/* Shaded samples per backward launch ("chunk": batBase.py has no counterpart, it is how the build bounds the
 * per-launch record block).  jt_shade_chunk_entries() = the current value (2^22 unless JT_SHADE_CHUNK_LOG2 says
 * otherwise); jt_shade_set_chunk_log2(l) sets 2^l for l in 16..22 and returns the previous log2 (any other l only
 * queries).  jt_shade_workspace_bytes depends on it: re-query after a change, never change it between a forward
 * and its backward. */
/* Where the training forward leaves the ReLU sign words of the two hidden layers inside `workspace` (test / debug
 * readers): out[0] = record rows per 32-sample tile, out[1] = first of the four sign rows (2 * layer + lane half),
 * out[2] = hidden width, out[3] = samples per tile.  Bit mt * 16 + r of the word of half h stands for hidden unit
 * mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * h (tensorBase.py:101-126: the ReLUs of MLPRender_Fea). */
int jt_shade_record_layout(const JtScene* scene, int32_t* out);
/* JT_DETERMINISTIC mode (also the environment variable of that name, read once): bit-reproducible gradients.  While
 * it is on, the g_factors pointers handed to jt_shade_backward / jt_march_backward must be INT64 shadow buffers with
 * the element count and indexing of the float gradient buffers (zero-initialised; sums arrive as 2^56 fixed point: value
 * = word / 2^56), the cross-block sums of jt_render_loss_forward / jt_reg_losses_forward / the weight gradients run in
 * a fixed order, and the ray gradients of jt_march_backward are combined in fixed point inside its workspace.  Returns
 * the previous setting; any argument other than 0 / 1 only queries.  A debugging aid (race detection), slower. */
int jt_set_deterministic(int on);
/* Device-side failure reporting of the gradient scatters (the reference's NaN checks, model/tensorf.py:43-44,147-151).  The
 * ray (pose) gradients of jt_march_backward, and in JT_DETERMINISTIC mode the factor gradients, are summed in 2^48 fixed
 * point; an addend that is NaN, infinite or >= 8 192 in magnitude is dropped and raises a sticky flag inside the library.
 * While the flag is up jt_march_backward writes NaN into g_rays_o / g_rays_d (as the float sums it replaces would have
 * carried it) and ORs JT_STATUS_FINITE_GRAD into the int32 status word bound with jt_status_bind (device memory, may be
 * NULL: nothing is reported then).  jt_status_clear zeroes the flag and the bound word on `stream`. */
#define JT_STATUS_FINITE_GRAD 8
int jt_status_bind(int32_t* status_word);
int jt_status_clear(void* stream);
int jt_shade_chunk_entries(void);
/* Which matrix stages of the appearance path run on the bf16 matrix cores with every fp32 operand split into three bf16
 * pieces and six products accumulated per K step (fp32-level accuracy; the reference's fp32 torch.nn.Linear chain,
 * tensorBase.py:43-131, is what both variants are held to): bit 0 the forward chain (basis product, layers 1 and 2),
 * bit 1 the weight-gradient GEMMs, bit 2 (round 5) layers 2 and 1 of the backward chain where the backward runs SPLIT
 * (chain kernel + scatter: the 20-channel scene, the tile-owned variant, the pose-only backward; the fused VM-48 kernel's LDS
 * has no room for the pre-split transposed weights).  0 = everything on the fp32 matrix cores; build default 7.  The
 * environment variable JT_BF16X3 (read once) overrides the build default; jt_shade_set_matrix_mode(mode) sets it for the
 * launches that follow and returns the previous value (a mode outside 0..7 only queries).  A forward and its backward may run under different modes: the
 * records they exchange are the same fp32 values in the same layout. */
int jt_shade_matrix_mode(void);
int jt_shade_set_matrix_mode(int mode);
int jt_shade_set_chunk_log2(int log2_entries);
/* How jt_shade_backward runs the per-sample part of the appearance backward (the autograd of bateRF.py:97-130 +
 * tensorBase.py:116-126): 0 = one kernel (MLP backward chain and the factor-gradient scatter of a 32-sample tile in the same
 * wave); 8 / 16 = two launches, the chain (which leaves the feature gradients in the record rows) and a scatter kernel whose
 * 16-lane groups walk runs of that many consecutive samples and which sums the LINE gradients in a workgroup-private LDS copy;
 * 1 (round 5) = the chain and the TILE-OWNED scatter (pairs counting-sorted by 4 x 4-texel tile, one wave per tile, the gradient
 * slice accumulated in matrix-core registers; needs factor gradients, float accumulation and at most 131 072 tiles per plane,
 * otherwise the default takes over);
 * -1 (the default) = chosen per scene kind: split 16 whenever the chain runs on the bf16 matrix cores (matrix-mode bit 2: the
 * build default) or the scene has fewer than 48 appearance channels, one kernel otherwise.  Same gradients
 * up to the order of the float sums.  The environment variable JT_BWD_SPLIT (read once) overrides the default; the setter
 * returns the previous value (any other argument only queries). */
int jt_shade_bwd_split(void);
int jt_shade_set_bwd_split(int run);
/* "Lean tape" (round 6; default 1, environment variable JT_LEAN_TAPE read once): whenever the backward is the split form with
 * the walker scatter (jt_shade_bwd_split() 8, 16, or -1 resolving to 16), the training forward does NOT record the 3 Ca
 * plane x line products of a shaded sample (bateRF.py:112-116) -- 576 of the 1 920 record bytes for VM-48, 240 of 1 104 for the
 * 20-channel scene -- and dBasis (the gradient of tensoRF.py:156's basis_mat) is formed inside the scatter kernel from the
 * products its walkers hold, instead of by a GEMM over recorded rows.  Same gradients up to the order of the float sums.
 * jt_shade_workspace_bytes / jt_shade_record_layout follow the mode; like the chunk size and the split mode it must not change
 * between a jt_shade_forward and its jt_shade_backward (all of them take the tape from one function of the modes).  The setter
 * returns the previous value; any argument other than 0 / 1 only queries. */
int jt_shade_lean_tape(void);
int jt_shade_set_lean_tape(int on);
/* Which kernels jt_shade_backward would launch for this scene under the library's CURRENT modes (matrix mode, split, lean tape,
 * deterministic mode, the JT_* environment switches) -- the launcher executes exactly this plan.  A diagnostic like
 * jt_shade_workspace_layout: no device memory, no stream, nothing is launched.  want_factor_grads / want_mlp_grads: g_factors /
 * g_mlp would be given; flags as for jt_shade_backward; have_aux: aux_stream and both events would be given.  out16:
 *   [0]  split mode as requested, -1 resolved per scene kind (the tape and the caller's choice of streams follow this one)
 *   [1]  split that runs: after the tile-owned scatter's fallback, the pose-only override (16) and the twelve-wave choice (8)
 *   [2]  chain kernel k_shade_bwd<C, DET, SPLIT, B16>: 0 <C, false> (fused), 1 <C, true> (fused, deterministic),
 *        2 <C, false, true> (split, fp32 matrix cores), 3 <C, false, true, true> (split, bf16 matrix cores)
 *   [3]  second kernel: 0 none, 1 k_shade_scatter, 2 the tile-owned scatter, 3 k_pose_gather<C, false>, 4 k_pose_gather<C, true>
 *   [4] [5] [6] [7]  DET, RUN, WAVES, FLAGS of k_shade_scatter<C, DET, RUN, WAVES, FLAGS> (0 unless [3] == 1)
 *   [8]  its dynamic LDS bytes   [9] its workgroups at most (also the slab count k_dbasis_reduce sums)
 *   [10] lean tape   [11] rows of a tile's record block (= jt_shade_record_layout out[0])
 *   [12] dBasis is formed in the scatter
 *   [13] weight-gradient GEMMs k_wgrad<.., B16>: 0 <.., false> (fp32), 1 <.., true> (bf16)   [14] GEMMs per chunk (0, 3 or 4)   [15] on the auxiliary stream
 * JT_ERR_UNSUPPORTED for a NULL argument, a scene kind the shade kernels are not built for, or a plan without an instantiation. */
int jt_shade_backward_plan(const JtScene* scene, int want_factor_grads, int want_mlp_grads, int flags, int have_aux,
                           int32_t* out16);
/* The same for jt_march_backward (want_factor_grads: g_factors given) / jt_march_backward_pose (have_dfeat = 1) on n_rays rays.
 * out8:
 *   [0] scan kernel k_march_bwd_scan<0 | 1 | 2>   [1] whether k_march_bwd_walk<Cd, DET, LINE, WAVES> runs behind it, and then
 *   [2] runs per (ray, plane)   [3] LINE: 0 no LDS line, 1 a float copy, 2 doubles   [4] WAVES per workgroup
 *   [5] the prefix table of the rays' item counts is kept in LDS (a run-time argument, no part of the kernel's name)
 *   [6] dynamic LDS bytes   [7] workgroups */
int jt_march_backward_plan(const JtScene* scene, int n_rays, int want_factor_grads, int have_dfeat, int32_t* out8);
int jt_shade_forward(const JtScene* scene, const JtFactors* factors, const JtMlp* mlp, const float* rays_o,
                     const float* rays_d, const float* jitter, const float* zvals, const float* tmin,
                     const int32_t* shade_offset, int n_rays, const int32_t* entry_ray,
                     const int32_t* entry_smp, const float* viewdirs, float* rgb_s, int n_entries_max,
                     void* workspace, size_t workspace_bytes, int flags, void* stream);
int jt_shade_backward(const JtScene* scene, const JtFactors* factors, const JtMlp* mlp, const float* rays_o,
                      const float* rays_d, const float* jitter, const float* zvals, const float* tmin,
                      const int32_t* shade_offset, int n_rays, const int32_t* entry_ray,
                      const int32_t* entry_smp, const float* viewdirs, const float* rgb_s, const float* g_rgb_s,
                      const JtFactors* g_factors, const JtMlp* g_mlp, float* g_xyz_app, int n_entries_max,
                      void* workspace, size_t workspace_bytes, int flags, void* stream, void* aux_stream,
                      void* ev_fork, void* ev_join);

/* (The single-launch test-time kernel jt_pose_fused lives in an OPTIONAL module of its own since round 5: include/jt_fused.h,
 * libjt_fused.so -- it is slower than the staged kernels it would replace and no default path uses it.) */

/* ---------------------------------------------------------------------------------------------
 * Regularisers over one channel-last factor [H][W][C] (a line is W = 1) in a single pass.
 * Replaces TensorVMSplit.density_L1 (tensoRF.py:212-216) and TVLoss.forward (tensorBase.py:16-41) and
 * their autograd:
 *   forward : out3[0] += sum |x|, out3[1] += sum_{y} (x[y+1,x]-x[y,x])^2, out3[2] += sum_{x} (x[y,x+1]-x[y,x])^2
 *             (out3 zeroed by the caller; the means / weights are applied by the caller)
 *   backward: g (+)= coef3[0]*sign(x) + coef3[1]*d(out3[1])/dx + coef3[2]*d(out3[2])/dx, coef3 on the device;
 *             accumulate != 0 adds to g, 0 overwrites it. */
int jt_factor_reg_forward(const float* x, int H, int W, int C, float* out3, void* stream);
int jt_factor_reg_backward(const float* x, int H, int W, int C, const float* coef3, float* g, int accumulate,
                           void* stream);

/* ---------------------------------------------------------------------------------------------
 * Photometric loss.  Replaces the render term of tensorf.Graph.compute_loss (model/tensorf.py:96-124) with
 * Graph.MSE_loss = nanmean of the squared error (model/base.py:259-261), including the `image[:, ray_idx]`
 * gather: rgb [B][r][3], image [B][3][n_pixels], ray_idx [r] int64; edge_mask [B][n_pixels] u8 or NULL.
 *   edge_mask == NULL: loss = nanmean((rgb - img)^2)
 *   else             : loss = edge_factor * nanmean((rgb*m - img*m)^2) + non_edge_factor * nanmean((rgb*(1-m) - img*(1-m))^2)
 * acc4: 4 floats of device scratch shared by forward and backward; g_loss: dL/dloss on the device.
 * The kernels index colours with 32 bits: 3 * n_views * rays_per_view >= 2^31 is JT_ERR_UNSUPPORTED, forward and backward, direct
 * and _ind. */
int jt_render_loss_forward(const float* rgb, const float* image, const int64_t* ray_idx, const uint8_t* edge_mask,
                           int n_views, int rays_per_view, int n_pixels, float edge_factor, float non_edge_factor,
                           float* acc4, float* loss, void* stream);
int jt_render_loss_backward(const float* rgb, const float* image, const int64_t* ray_idx, const uint8_t* edge_mask,
                            int n_views, int rays_per_view, int n_pixels, float edge_factor, float non_edge_factor,
                            const float* acc4, const float* g_loss, float* g_rgb, void* stream);
/* One photometric nanmean PER VIEW over a ragged batch (layout as jt_raygen_forward_ragged; image [n_views][3][n_pixels], no edge
 * mask): loss [n_views], acc2 [n_views][2] = (sum of squares, count) kept for the backward, g_rgb[i] = g_loss[view of i] * 2 (rgb -
 * gt) / count -- the single-view jt_render_loss_forward / backward bit for bit.  The same 32-bit limit: the backward returns
 * JT_ERR_UNSUPPORTED for 3 * n_rays >= 2^31; the forward cannot see the counts (view_offset is device memory), so a caller
 * that has not been through the backward's check must keep every view below 2^31 / 3 rays itself. */
int jt_render_loss_views_forward(const float* rgb, const float* image, const int64_t* ray_idx, const int32_t* view_offset,
                                 int n_views, int n_pixels, float* acc2, float* loss, void* stream);
int jt_render_loss_views_backward(const float* rgb, const float* image, const int64_t* ray_idx, const int32_t* view_offset,
                                  int n_views, int n_rays, int n_pixels, const float* acc2, const float* g_loss, float* g_rgb,
                                  void* stream);
/* The same with the supervising buffers named by DEVICE memory: slots[0] = address of the image buffer, slots[1] = address
 * of the edge-mask buffer (read only when with_edge_mask != 0).  The reference picks one of five blur scales of the
 * ground-truth images per iteration (model/nerf.py:209-227); a captured hipGraph stays the same for all of them when the
 * caller rewrites `slots` with jt_poke in front of a replay. */
int jt_render_loss_forward_ind(const float* rgb, const uint64_t* slots, const int64_t* ray_idx, int with_edge_mask,
                               int n_views, int rays_per_view, int n_pixels, float edge_factor, float non_edge_factor,
                               float* acc4, float* loss, void* stream);
int jt_render_loss_backward_ind(const float* rgb, const uint64_t* slots, const int64_t* ray_idx, int with_edge_mask,
                                int n_views, int rays_per_view, int n_pixels, float edge_factor, float non_edge_factor,
                                const float* acc4, const float* g_loss, float* g_rgb, void* stream);

/* Non-finite guard without a host sync: ORs items[k].bit into *status_word (device memory, caller-owned, cleared by
 * the caller) for every item whose `data[0..n)` holds a NaN or an infinity; one launch for up to JT_FINITE_MAX
 * tensors.  Stands in for the per-iteration `pose.isnan().any()` / `assert not torch.isnan(loss[key])` host reads of
 * model/tensorf.py:43-44,147-151; the host reads the word when it wants to. */
#define JT_FINITE_MAX 8
typedef struct JtFiniteItem {
  const float* data;
  int64_t n;
  int32_t bit;
  int32_t pad_;
} JtFiniteItem;
int jt_finite_check(const JtFiniteItem* items, int n_items, int32_t* status_word, void* stream);

/* TV of the rendered depth over the pixel lattice (model/tensorf.py:126-135, `TV_depth`), VALUE only: out[0] = sum over views of
 * sum_h (d[h+1][w] - d[h][w])^2 / grid_h + sum_w (d[h][w+1] - d[h][w])^2 / grid_w for depth [n_views][grid_h][grid_w].  The BAT
 * yamls weight the term 0.0 and only log it; a non-zero weight goes through the host mirror's differentiable ops. */
int jt_tv_depth_forward(const float* depth, int n_views, int grid_h, int grid_w, float* out, void* stream);

/* SSIM of n_views image pairs, the `pytorch_ssim.ssim(rgb_map, var.image)` of the evaluation loop (model/nerf.py:550; as stock
 * ops: five grouped conv2d calls and ~20 element-wise launches per image, in fp32).  pred, target: [n_views][n_channels][height]
 * [width] fp32.  Window: the outer product of g[k] = exp(-(k - 5)^2 / (2 * 1.5^2)), k = 0..10, normalised to sum 1 and rounded
 * to fp32.  Per channel, with ZERO padding of 5 (the window is not renormalised at the border): mu1 = g*x, mu2 = g*y, s1 =
 * g*(x x) - mu1^2, s2 = g*(y y) - mu2^2, s12 = g*(x y) - mu1 mu2, ssim_map = (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)
 * (s1 + s2 + C2)), C1 = 0.01^2, C2 = 0.03^2.  ssim[v] (fp64) = mean of view v's map over channels and pixels; ssim_map (fp32,
 * same shape as the inputs) may be NULL.  The moments, the formula and the sums are fp64; the per-view sum has ONE order (no
 * atomics): the same bits run to run, with JT_DETERMINISTIC on or off.  Any height, width >= 1.  workspace:
 * jt_ssim_workspace_bytes(...) bytes, caller-provided, 8-byte aligned, overwritten.  JT_ERR_UNSUPPORTED when n_views *
 * n_channels * height * width reaches 2^31 (or n_views * n_channels exceeds 65 535). */
int jt_ssim_forward(const float* pred, const float* target, int n_views, int n_channels, int height, int width, double* ssim,
                    float* ssim_map, void* workspace, size_t workspace_bytes, void* stream);
size_t jt_ssim_workspace_bytes(int n_views, int n_channels, int height, int width);

/* Picture preprocessing of the dataset loaders (data/base.py:92-107 `preprocess_image`, data/blender.py:71-76): n_images decoded
 * pictures, uint8 [n_images][in_h][in_w][channels] (channels 3 or 4, device memory, 4-byte aligned when channels is 4) -> fp32
 * [n_images][3][out_h][out_w] at `out`, EQUAL BIT FOR BIT to PIL.Image.resize((out_w, out_h), LANCZOS) of an 8-bit RGB / RGBA
 * picture, torchvision's to_tensor (byte / 255 in fp32, IEEE division) and, for channels = 4 with `composite` set,
 * rgb * mask + bgcolor * (1 - mask) in fp32, every operation rounded on its own (mask = the resampled alpha / 255); channels = 4
 * without `composite` returns the resampled colour.  Pillow's arithmetic: RGBA is premultiplied ((t >> 8) + t) >> 8, t = c * a +
 * 128, resampled, and divided out (c where a is 0 or 255, else min(255, 255 c / a)); each axis is a table of int32 weights in
 * 2^22 fixed point, one output byte = clamp((2^21 + sum_i k_i in[first + i]) >> 22, 0, 255) in 32-bit integers; the horizontal
 * pass first, rounded to bytes, then the vertical pass.  An axis whose sizes agree is skipped, and with both equal the picture
 * is not premultiplied at all.  table_x / table_y (device, int32): [(2 + taps)][n_out], row 0 the first source index of every
 * output index, row 1 its tap count (<= taps), row 2 + i the weight of tap i; built on the host in double precision
 * (joint_tensorf_amd/datasets.py: resample_table); may be NULL for an axis whose sizes agree.  The kernels clamp every window to
 * the picture.  workspace: jt_image_ingest_workspace_bytes(...) bytes (the byte intermediate of the horizontal pass; 0 when
 * in_w == out_w), caller-provided, 4-byte aligned, overwritten.  One or two launches on `stream`, nothing else.  JT_ERR_ARG
 * for channels outside {3, 4}, a size below 1, a missing table or a short workspace; JT_ERR_UNSUPPORTED for n_images > 65 535
 * or more than 262 140 rows. */
int jt_image_ingest(const uint8_t* images, int n_images, int in_h, int in_w, int channels, const int32_t* table_x, int taps_x,
                    const int32_t* table_y, int taps_y, int out_h, int out_w, int composite, float bgcolor, float* out,
                    void* workspace, size_t workspace_bytes, void* stream);
size_t jt_image_ingest_workspace_bytes(int n_images, int in_h, int in_w, int channels, int out_h, int out_w);

/* The weighted sum of Model.summarize_loss (model/tensorf.py:31-47) over the photometric term and the three
 * regularisers, one launch each way:  total = w_render render[0] + w_l1 reg3[0] + w_tv_density reg3[1] +
 * w_tv_color reg3[2]  (reg3 = the out3 of jt_reg_losses_forward; a term with weight 0 is left out, as the reference
 * leaves it out);  backward: g_render[0] = g_total[0] w_render, g_reg3[k] = g_total[0] w_k. */
int jt_loss_sum_forward(const float* render, const float* reg3, float w_render, float w_l1, float w_tv_density,
                        float w_tv_color, float* total, void* stream);
int jt_loss_sum_backward(const float* g_total, float w_render, float w_l1, float w_tv_density, float w_tv_color,
                         float* g_render, float* g_reg3, void* stream);
/* The same with w4 = {w_render, w_l1, w_tv_density, w_tv_color} in DEVICE memory: a captured hipGraph keeps working while
 * the host schedule changes the weights every iteration (LLFF: the TV weights decay per iteration, model/tensorf.py:441-447);
 * the caller rewrites w4 with jt_poke in front of a replay. */
int jt_loss_sum_forward_dyn(const float* render, const float* reg3, const float* w4, float* total, void* stream);
/* jt_loss_sum_forward (w4_host: the four weights as host floats) or _dyn (w4_dev, used when w4_host is NULL) AND
 * jt_finite_check of `items` in ONE launch; the total itself is checked as well and reports `loss_bit`. */
int jt_loss_sum_check_forward(const float* render, const float* reg3, const float* w4_host, const float* w4_dev,
                              float* total, const JtFiniteItem* items, int n_items, int32_t loss_bit,
                              int32_t* status_word, void* stream);
int jt_loss_sum_backward_dyn(const float* g_total, const float* w4, float* g_render, float* g_reg3, void* stream);

/* All regularisers of one scene in one call (replaces the loop bodies of model/tensorf.py:127-130):
 *   out3 = { density_L1(), TV_loss_density(TVLoss()), TV_loss_app(TVLoss()) }   (tensoRF.py:212-228).
 * plane_hw_line[9] = {H_i, W_i, L_i} for i = 0..2; scratch640 (forward): 640 floats of device scratch that must be ZERO when the
 * first call sees them and are left zero by every call (the one launch sums into them and its last workgroup combines and resets
 * them: no zero fill and no combine launch per iteration); not to be shared by calls that run concurrently.
 * with_tv_density / with_tv_app == 0: that TV term has weight zero in the run; it is not evaluated and out3
 * carries 0 for it (the L1 term is always evaluated).
 * backward: g3 = dL/d out3 on the device; writes (accumulate == 0) or adds (accumulate != 0) the gradients of
 * the density planes + lines, and of the appearance planes when with_tv_app != 0, into g_factors. */
int jt_reg_losses_forward(const JtFactors* factors, const int32_t* plane_hw_line, int n_comp_density,
                          int n_comp_app, int with_tv_density, int with_tv_app, float* scratch640, float* out3,
                          void* stream);
int jt_reg_losses_backward(const JtFactors* factors, const int32_t* plane_hw_line, int n_comp_density,
                           int n_comp_app, const float* g3, int with_tv_density, int with_tv_app,
                           const JtFactors* g_factors, int accumulate, float* scratch640, void* stream);
/* Value AND gradient in ONE launch (round 5): out3 as jt_reg_losses_forward, and the gradients that jt_reg_losses_backward
 * (accumulate == 0) would WRITE for the upstream gradients w3 = dL/d out3 -- in a training step the loss weights of
 * Model.summarize_loss (model/tensorf.py:31-47), known before the forward: three host floats (w3_host) or, when w3_host is
 * NULL, three floats in device memory (w3_dev: a replayed hipGraph reads this iteration's weights from there).  Every factor
 * is read once instead of twice.  scratch640 as for the forward.  JT_ERR_UNSUPPORTED in deterministic mode. */
int jt_reg_losses_fused(const JtFactors* factors, const int32_t* plane_hw_line, int n_comp_density, int n_comp_app,
                        int with_tv_density, int with_tv_app, const float* w3_host, const float* w3_dev,
                        const JtFactors* g_factors, float* scratch640, float* out3, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Dense Adam step over all tensors of an optimizer in one launch.  Replaces torch.optim.Adam.step of the
 * optimizer built by tensorf.NeRF._get_optimizer (model/tensorf.py:463-478, betas (0.9, 0.99)):
 *   m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;  p -= lr / bias_correction1 * m / (sqrt(v) / sqrt(bias_correction2) + eps)
 * p, g, m, v: n floats each in the same (dense) layout, 16-byte aligned; updated in place. */
typedef struct JtAdamItem {
  float* p;
  const float* g;
  float* m;
  float* v;
  int64_t n;
  float lr;
  float bias_correction1; /* 1 - beta1^step */
  float bias_correction2; /* 1 - beta2^step */
  int32_t pad_;
} JtAdamItem;
int jt_adam_step(const JtAdamItem* items, int n_items, float beta1, float beta2, float eps, void* stream);

/* The same step with the two per-tensor coefficients that change every iteration read from DEVICE memory:
 * dyn[2 i] = lr_i / (1 - beta1^step_i), dyn[2 i + 1] = 1 / sqrt(1 - beta2^step_i) for item i (the lr /
 * bias_correction fields of the items are ignored).  A hipGraph that captured this launch (the whole steady-state
 * iteration is captured, joint_tensorf_amd/graphed.py) is replayed with new coefficients written by jt_poke. */
int jt_adam_step_dyn(const JtAdamItem* items, int n_items, float beta1, float beta2, float eps, const float* dyn,
                     void* stream);
/* The same step with the SAME two coefficients per item given as floats in HOST memory (coefs_host[2 i], [2 i + 1]; the
 * lr / bias_correction fields are ignored): they travel as launch arguments.  An eager iteration steps with exactly the
 * float values a replayed one reads from `dyn`, without the jt_poke launch in front. */
int jt_adam_step_coefs(const JtAdamItem* items, int n_items, float beta1, float beta2, float eps,
                       const float* coefs_host, void* stream);

/* Write n_words (1..256) 32-bit words from HOST memory `words` to device memory `dst` on `stream`: the values
 * travel as launch arguments (no host staging buffer, no synchronisation, the host array may be reused at once).
 * The per-iteration host scalars of the reference's loop -- lattice offsets (model/nerf.py:663), Adam coefficients
 * (model/tensorf.py:441-447 decays the lr every iteration) -- reach a replayed hipGraph this way. */
int jt_poke(void* dst, const uint32_t* words, int n_words, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Iso-surface of a scalar lattice as a triangle mesh (csrc/jt_mesh.hip): marching tetrahedra on the Kuhn triangulation of every
 * lattice cell -- six tetrahedra per cell, one per permutation (a, b, c) of the axes, corners c0 = (0,0,0), c1 = c0 + e_a, c2 = c1 +
 * e_b, c3 = (1,1,1).  The upstream TensoRF exports its mesh with skimage's marching cubes on the host; the reference kept only
 * the `trimesh:` option block.  lattice: [nx][ny][nz] fp32, z fastest (what getDenseAlpha returns); a point is inside iff its
 * value > level, so a NaN is outside.  Every tetrahedron edge is owned by its lower lattice point p and is one of seven kinds,
 * bits 0..6 = +x, +y, +z, +x+y, +x+z, +y+z, +x+y+z.  Two passes, no atomics, the same bits on every run:
 *   jt_mesh_count: edge_flags[p] bit k = owned edge k exists (its upper end is a lattice point) and its ends differ in `inside`
 *     (popcount = the vertices p owns); tri_count[p] (0..12) = triangles of the cell whose minimum corner is p, 0 without a cell.
 *   the caller scans both exclusively into int64 (vert_offset[p], tri_offset[p]) and reads the two totals;
 *   jt_mesh_emit: vertex vert_offset[p] + popcount(edge_flags[p] & ((1 << k) - 1)) lies on owned edge k of p at P(a) + t (P(b) -
 *     P(a)) per axis, a the owner, b the upper end, t = (level - v_a) / (v_b - v_a) in fp32 clamped to [0, 1] (a NaN t is 0.5),
 *     P_axis(i) = lo (1 - s) + hi s with s = float(i) / float(n - 1); lo3 / hi3 are HOST pointers.  The triangles of cell p start
 *     at tri_offset[p], tetrahedra in the order of the permutations (012, 021, 102, 120, 201, 210); two inside corners I0 < I1
 *     and outside corners O0 < O1 make the quad a = (I0,O0), b = (I0,O1), c = (I1,O1), d = (I1,O0), split along a-c.  The
 *     winding comes from the case and the permutation's parity alone, normals (right-hand rule) from inside to outside.
 * vertices [n_vertices][3] fp32, triangles [n_triangles][3] int32 vertex ids.  One launch each on `stream`, nothing else.
 * JT_ERR_ARG for a NULL pointer, any n < 2 or a non-finite level; JT_ERR_UNSUPPORTED when nx ny nz > 2^27 or when n_vertices
 * or 3 n_triangles reaches 2^31; n_vertices == 0 launches nothing (vertices / triangles may then be NULL) and is JT_OK.  Stores
 * past n_vertices / n_triangles are dropped, whatever the offsets say. */
int jt_mesh_count(const float* lattice, int nx, int ny, int nz, float level, uint8_t* edge_flags, uint8_t* tri_count,
                  void* stream);
int jt_mesh_emit(const float* lattice, int nx, int ny, int nz, float level, const float* lo3, const float* hi3,
                 const uint8_t* edge_flags, const int64_t* vert_offset, const int64_t* tri_offset, long n_vertices,
                 long n_triangles, float* vertices, int32_t* triangles, void* stream);

/* ---------------------------------------------------------------------------------------------
 * NDC meshes in world space (csrc/jt_mesh.hip).  A `camera.ndc` scene lives in the NDC coordinates of the ray generator
 * (camera.py:303-340; the centre shift moves ray origins only and does not enter): with n = ndc_near, sx = fx / cx, sy = fy / cy
 *     xn = sx x / z,   yn = sy y / z,   zn = 1 - 2 n / z            (world, camera-like frame, z forward -> NDC)
 *     u = 1 - zn,   z = 2 n / u,   x = xn z / sx,   y = yn z / sy   (NDC -> world), defined for u > 0:
 * zn = 1 is infinity and zn > 1 lies behind it.  The map is projective (planes go to planes) with det J = 2 n sx sy / z^4 > 0, so
 * the winding of a triangle is preserved.  A normal is a gradient direction and transforms by J^T; scaled by the positive z,
 *     n_world ~ (sx nx, sy ny, (1 - zn) nz - xn nx - yn ny), then normalised; (0, 0, 0) stays (0, 0, 0).
 *
 *   jt_mesh_unwarp_ndc: one launch, one lane per vertex of vertices [n][3] (NDC) and, when not NULL, normals [n][3] -> world
 *     [n][3], world_normals [n][3] (not touched without normals) and status [n] uint8, the first that applies of
 *       JT_UNWARP_BEYOND 1: a non-finite input coordinate, u <= 0, or a non-finite result;
 *       JT_UNWARP_FAR 2: max_depth > 0 and z > max_depth (z == max_depth is kept; max_depth <= 0: no limit);
 *       JT_UNWARP_KEPT 0.
 *     A vertex that is not kept is written as zeros, position and normal.  Every component is a chain of correctly rounded fp32
 *     operations on the one u = 1 - zn: z = (2 n) / u, x = (xn z) / sx, y = (yn z) / sy -- at most four roundings each, whatever
 *     the compiler contracts; the normal's third component is fma(u, nz, -fma(xn, nx, yn ny)), its length one fma chain and a
 *     square root, each component one division; a length that is zero or not finite gives (0, 0, 0).
 *   jt_mesh_filter_count: per triangle of triangles [n_triangles][3] keep[t] = 1 iff its three ids lie in [0, n_vertices) and
 *     their statuses are 0, and cause[t] = 0 for a kept one, else the first that applies of 1 (an id out of range, a vertex
 *     beyond) and 2 (a vertex far); used[v] = 1 for every vertex of a kept triangle (used [n_vertices], zeroed by the caller;
 *     several lanes may store the same 1; no atomics).
 *   the caller scans keep and used exclusively into int64 (tri_offset[t], vert_offset[v]) and reads the two totals;
 *   jt_mesh_filter_emit: kept triangle t becomes row tri_offset[t] of triangles_out with ids vert_offset[id]; used vertex v becomes
 *     row vert_offset[v] of vertices_out and, for normals / colors [n_vertices][3] fp32 that are not NULL, of normals_out /
 *     colors_out.  Both keep their original order; two runs give the same bits.  Stores past n_vertices_out / n_triangles_out are
 *     dropped; n_vertices_out == 0 launches nothing.
 * One launch each on `stream`, nothing else.  JT_ERR_ARG for a NULL pointer, a count below 1, an out count above its in count, a
 * NaN max_depth or an sx, sy or ndc_near that is not a positive finite number; JT_ERR_UNSUPPORTED when n (n_vertices) or 3
 * n_triangles reaches 2^31. */
#define JT_UNWARP_KEPT 0
#define JT_UNWARP_BEYOND 1
#define JT_UNWARP_FAR 2
int jt_mesh_unwarp_ndc(const float* vertices, const float* normals, long n, float sx, float sy, float ndc_near, float max_depth,
                       float* world, float* world_normals, uint8_t* status, void* stream);
int jt_mesh_filter_count(const int32_t* triangles, long n_triangles, const uint8_t* status, long n_vertices, uint8_t* keep,
                         uint8_t* cause, uint8_t* used, void* stream);
int jt_mesh_filter_emit(const float* vertices, const float* normals, const float* colors, long n_vertices,
                        const int32_t* triangles, long n_triangles, const uint8_t* keep, const uint8_t* used,
                        const int64_t* vert_offset, const int64_t* tri_offset, long n_vertices_out, long n_triangles_out,
                        float* vertices_out, float* normals_out, float* colors_out, int32_t* triangles_out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Mesh simplification (csrc/jt_simplify.hip): vertex clustering with a quadric (Hermite) representative.  Vertices are binned
 * into a uniform grid of cells3 = (cx, cy, cz) cells over the box lo3 .. hi3 (HOST pointers, as jt_mesh_emit takes them; cells3 a
 * HOST pointer to three ints); every occupied cell becomes ONE vertex, placed where the planes (position, normal) of its members
 * meet in the least-squares sense, regularised towards their mean; triangles are re-indexed and the collapsed ones dropped.  No
 * atomics, the same bits on every run, and every number below is a fixed sequence of correctly rounded operations (no
 * contraction): a NumPy statement of this comment reproduces the kernels bit for bit (tests/simplify_ref.py).
 *
 *   jt_simplify_keys: keys [n] int64 of vertices [n][3] fp32.  Per axis, in fp32, four operations each rounded once:
 *       d = x - lo,  w = hi - lo,  s = d / w,  f = s * float(cells);   i = cells - 1 if f >= cells, 0 if f < 0, else floorf(f);
 *     key = (ix * cy + iy) * cz + iz.  A vertex with a non-finite coordinate gets key cx * cy * cz, the "none" cluster, which owns
 *     no output vertex.
 *   the caller sorts the keys STABLY (members of a cluster stay in ascending vertex id) into order [n] int64, the vertex ids in
 *     sorted order; cluster j is the j-th distinct key below cx cy cz in ascending order and seg_start [n_clusters + 1] int64 the
 *     positions in `order` where the clusters begin, seg_start[n_clusters] = the number of vertices with a key below cx cy cz.
 *   jt_simplify_clusters: one lane per cluster, walking its members v_1 < ... < v_m = order[seg_start[j] .. seg_start[j + 1]) in
 *     that order (a wave per cluster would sum in another order: the order IS the contract).  Everything in fp64 from the fp32
 *     inputs, every sum sequential from 0.0 in member order, p = position, n = normal with (0, 0, 0) for one that has a non-finite
 *     component:
 *       c = (sum p_v) / m                                           per axis;
 *       per member  d = p_v - c,  e = (n_x d_x + n_y d_y) + n_z d_z,
 *                   a00 += n_x n_x, a01 += n_x n_y, a02 += n_x n_z, a11 += n_y n_y, a12 += n_y n_z, a22 += n_z n_z,
 *                   b += n e  and  sn += n                          per axis;
 *       r = double(lambda) * m;  a00 += r, a11 += r, a22 += r;
 *       k00 = a11 a22 - a12 a12,  k01 = a02 a12 - a01 a22,  k02 = a01 a12 - a02 a11,
 *       k11 = a00 a22 - a02 a02,  k12 = a01 a02 - a00 a12,  k22 = a00 a11 - a01 a01     (each: two products, one difference),
 *       det = (a00 k00 + a01 k01) + a02 k02,
 *       x0 = ((k00 b0 + k01 b1) + k02 b2) / det,  x1 = ((k01 b0 + k11 b1) + k12 b2) / det,  x2 = ((k02 b0 + k12 b1) + k22 b2) / det;
 *       positions[j] = min(max(fp32(c + x), lowest member coordinate), highest member coordinate)   per axis, min / max in fp32.
 *     A is positive definite with a condition number of at most (1 + lambda) / lambda for unit normals: no pivoting.  With unit
 *     normals this is the dual-contouring QEF regularised towards the mean: flat, zero-normal and single-normal clusters give the
 *     mean (along the directions the normals do not fix).  A representative never leaves the bounding box of what it replaces,
 *     and a cluster of one member returns its vertex exactly.  normals_out[j] = fp32(sn / sqrt((sn_x sn_x + sn_y sn_y) + sn_z
 *     sn_z)) per axis, (0, 0, 0) when the length is zero or not finite; counts[j] = m (int32).  An `order` entry outside [0, n)
 *     is no member and seg_start is clamped to [0, n]: nothing is read out of bounds; an empty cluster is written as zeros.
 *   the caller scatters the cluster index over `order` into cluster [n] int32, -1 for the none cluster;
 *   jt_simplify_triangles: per triangle of triangles [n_triangles][3] triangles_out[t] = (cluster[a], cluster[b], cluster[c]), -1
 *     for an id outside [0, n_vertices) or a cluster outside [0, n_clusters); cause[t] = the first that applies of
 *       JT_SIMPLIFY_INVALID 1: an id out of range or a vertex of the none cluster;
 *       JT_SIMPLIFY_COLLAPSED 2: two of the three clusters equal;
 *       JT_SIMPLIFY_KEPT 0;
 *     keep[t] = 1 for a kept one, and used[j] = 1 for the clusters of kept triangles (used [n_clusters], zeroed by the caller;
 *     several lanes may store the same 1; no atomics).  Duplicate triangles and opposite pairs are NOT removed, deliberately: the
 *     vertex map is simplicial, so every directed edge of the result occurs as often as its reverse whenever that held for the
 *     input, and removing same-orientation duplicates would break it.
 *   the caller scans keep and used and compacts with jt_mesh_filter_emit (vertices = positions, triangles = triangles_out): kept
 *     triangles in their original order, used clusters in key order.
 * One launch each on `stream`, nothing else; every argument is checked before the launch.  JT_ERR_ARG for a NULL pointer, a count
 * below 1, n_clusters above the vertex count, a cell count outside 1 .. 2^20, hi <= lo on an axis, a non-finite box (or fp32
 * extent), or a lambda that is not a positive finite number; JT_ERR_UNSUPPORTED when n (n_vertices) or 3 n_triangles reaches 2^31. */
#define JT_SIMPLIFY_KEPT 0
#define JT_SIMPLIFY_INVALID 1
#define JT_SIMPLIFY_COLLAPSED 2
int jt_simplify_keys(const float* vertices, long n, const float* lo3, const float* hi3, const int* cells3, int64_t* keys,
                     void* stream);
int jt_simplify_clusters(const float* vertices, const float* normals, long n, const int64_t* order, const int64_t* seg_start,
                         long n_clusters, float lambda, float* positions, float* normals_out, int32_t* counts, void* stream);
int jt_simplify_triangles(const int32_t* triangles, long n_triangles, const int32_t* cluster, long n_vertices, long n_clusters,
                          int32_t* triangles_out, uint8_t* keep, uint8_t* cause, uint8_t* used, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Connected components of a lattice's inside points (csrc/jt_components.hip), with the connectivity of the mesh above: two
 * points are adjacent iff both are inside (value > level; a NaN is outside) and they differ by + or - one of the seven edge
 * kinds -- 14 neighbours; (+x, -y) is no edge.  Every tetrahedron's inside corners then lie in one component, and the surface
 * splits exactly along components.  labels [nx][ny][nz] int32, z fastest: -1 outside, else the SMALLEST flat index of the
 * point's component -- a function of the lattice alone, the same bits on every run.
 *   jt_components_init: labels[p] = p inside, -1 outside.
 *   jt_components_sweep: one sweep of min-label propagation; a workgroup owns a tile of JT_COMPONENTS_TILE^3 points, lowers
 *     its labels over the 14 neighbours (a one-point halo read from its neighbours' tiles) until the tile is stable and stores
 *     only into its own tile; *lowered (a device word, zeroed by the caller) is set to 1 when any label fell.  With jump != 0 a
 *     second launch follows: labels[p] = labels[labels[...]] down the chain.  No workgroup waits for another: a halo word a
 *     neighbour lowers during the same launch may or may not be seen.  The caller repeats until a sweep leaves *lowered at 0;
 *     the labels are then final (and only then).
 *   jt_component_sizes: sizes[l] += 1 for every point with label l >= 0; sizes [nx ny nz] int32, zeroed by the caller
 *     (integer atomics: the sums do not depend on the order).
 * JT_ERR_ARG for a NULL pointer, any n < 2 or a non-finite level; JT_ERR_UNSUPPORTED when nx ny nz > 2^27. */
#define JT_COMPONENTS_TILE 8
int jt_components_init(const float* lattice, int nx, int ny, int nz, float level, int32_t* labels, void* stream);
int jt_components_sweep(int32_t* labels, int nx, int ny, int nz, int32_t* lowered, int jump, void* stream);
int jt_component_sizes(const int32_t* labels, int nx, int ny, int nz, int32_t* sizes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * A triangle rasteriser (csrc/jt_raster.hip): an exported mesh seen from its cameras.  Three calls, one launch each on `stream`,
 * nothing else, no host read between them; every argument is checked before anything launches.
 *
 *   jt_raster_project: screen [n_views][n_vertices][4] = (x, y, 1/w, w) of vertices [n_vertices][3] under proj [n_views][12], one
 *     3 x 4 row-major matrix per view that takes a homogeneous mesh-space point to (x w, y w, w) in pixel units.  x is the column
 *     and y the row; the pixel of column i and row j has its centre at (i + 0.5, j + 0.5), as the ray generator has it
 *     (camera.py:236-237), so proj = intr @ [R | t] puts a vertex where the field's rays see it.  Each of the three sums is a
 *     chain of three fmaf from the constant term, each quotient one division.  A vertex with a non-finite coordinate, with w <
 *     near (or a NaN w) or whose 1/w is not a positive finite number is written as (0, 0, 0, w).
 *   jt_raster_draw: every triangle [n_triangles][3] (int32 vertex ids) of every view into zbuf [n_views][H][W] uint64, which the
 *     caller has filled with all-ones bits.  Coverage is decided in integers: a vertex is snapped to 1/256 pixel (rintf(x *
 *     256)), the three edge functions are evaluated at the pixel centre in int64 with the top-left fill rule -- two triangles
 *     that share an edge cover every pixel of their union exactly once.  At a covered pixel q = (b0 q0 + b1 q1 + b2 q2) / (b0 +
 *     b1 + b2) in fp32, b the integer edge values and q_i = 1/w_i; the nearest triangle (largest q) wins, at equal q the lower
 *     index: ONE 64-bit atomic minimum per covered pixel on (~bits(q)) << 32 | index, so the result does not depend on the order
 *     of execution.  status [n_views][n_triangles] uint8 says what became of every triangle, the first that applies of
 *       JT_RASTER_DRAWN 0;
 *       JT_RASTER_NEAR 1: a vertex with 1/w = 0 in `screen` (behind near or non-finite), or a vertex id outside [0, n_vertices):
 *         the whole triangle is dropped, not clipped;
 *       JT_RASTER_GUARD 2: a snapped coordinate beyond +-2^22 sub-pixels (or not a number);
 *       JT_RASTER_EMPTY 3: zero area after snapping;
 *       JT_RASTER_CULLED 4: cull != 0 and the screen-space winding of a back face, (x1 - x0)(y2 - y0) - (y1 - y0)(x2 - x0) > 0 --
 *         what a triangle whose right-hand normal points away from the camera projects to under a proj with positive focal
 *         lengths (x right, y down, z forward).
 *     A drawn triangle need not cover a pixel.  No lane walks more than 64 pixels of a bounding box alone: larger boxes are
 *     walked by the whole wave.
 *   jt_raster_resolve: per pixel tri [n_views][H][W] int32 (the winner, -1 where nothing was drawn), depth fp32 (1 / q of the
 *     key, +inf where nothing was drawn) and, with attrs [n_vertices][n_attrs] fp32 (n_attrs <= 8), out [n_views][H][W][n_attrs]:
 *     attrs interpolated perspective-correctly, sum b_i q_i a_i / sum b_i q_i with the barycentrics recomputed from the same
 *     integers as in draw, evaluated as a0 + l1 (a1 - a0) + l2 (a2 - a0) with l_i = b_i q_i / sum b q (a constant attribute comes
 *     back exactly); background [n_attrs] (a HOST pointer) elsewhere.  n_attrs == 0: attrs, background and out are not read.
 *
 * JT_ERR_ARG for a NULL pointer, a size below 1 or a non-finite near; JT_ERR_UNSUPPORTED when n_views * H * W or n_triangles
 * reaches 2^31, H or W exceeds 16384, n_views exceeds 65535 or n_attrs exceeds 8. */
#define JT_RASTER_DRAWN 0
#define JT_RASTER_NEAR 1
#define JT_RASTER_GUARD 2
#define JT_RASTER_EMPTY 3
#define JT_RASTER_CULLED 4
int jt_raster_project(const float* vertices, int n_vertices, const float* proj, int n_views, float near, float* screen,
                      void* stream);
int jt_raster_draw(const float* screen, int n_vertices, const int32_t* triangles, long n_triangles, int n_views, int H, int W,
                   int cull, uint64_t* zbuf, uint8_t* status, void* stream);
int jt_raster_resolve(const uint64_t* zbuf, const float* screen, int n_vertices, const int32_t* triangles, long n_triangles,
                      int n_views, int H, int W, const float* attrs, int n_attrs, const float* background, int32_t* tri,
                      float* depth, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Texture atlas (csrc/jt_texture.hip, and jt_raster_resolve_texture in csrc/jt_raster.hip): colour decoupled from the vertex
 * count.  The atlas is a grid of square blocks of S x S texels (S from 4 to 64), `cols` blocks to a row, block b at column
 * b % cols and row b / cols; every block holds the charts of the two triangles 2b and 2b + 1, right-isosceles with legs of
 * L = S - 3 texels.  Texel (i, j) of a block -- column and row, 0 .. S - 1, centre at (i + 0.5, j + 0.5) -- belongs to triangle
 * 2b (the lower chart, chart coordinates (i, j)) when i + j <= S - 1 and to triangle 2b + 1 (the upper chart, the lower one
 * turned by 180 degrees: chart coordinates (S - 1 - i, S - 1 - j)) otherwise.  At chart coordinates (i, j) the barycentric weights
 * are a = i / L for vertex 1, b = j / L for vertex 2 and 1 - a - b for vertex 0: vertex 0 sits on texel (0, 0), vertex 1 on (L, 0),
 * vertex 2 on (0, L), and the texels beyond the hypotenuse (down to -2 / L for vertex 0) are extrapolated, not left empty.  A
 * bilinear sample at a point of a chart then reads only texels of chart coordinates i + j <= S - 2: never the other triangle's,
 * never another block's.  Texel (i, j) of block b is entry e = b S S + j S + i; atlas [H_atlas][W_atlas][3] uint8 with W_atlas =
 * cols S and H_atlas = rows S holds entry e at pixel (column (b % cols) S + i, row (b / cols) S + j).
 *
 *   jt_texture_texels: for the entries [start, start + count) -- any range, not aligned to blocks; slabs compose to the bits of
 *     one call -- where the appearance branch is to be asked: xyz [count][3], dirs [count][3] fp32 and valid [count] uint8, from
 *     vertices [n_vertices][3], normals [n_vertices][3] fp32 and triangles [n_triangles][3] int32.  With (v0, v1, v2) the
 *     triangle's vertices and a = float(i) / float(L), b = float(j) / float(L) at the entry's chart coordinates, in fp32, every
 *     operation rounded on its own (no contraction), per axis:
 *       p = (v0 + a (v1 - v0)) + b (v2 - v0),      m = (n0 + a (n1 - n0)) + b (n2 - n0)      the same way from the normals;
 *       dir = fp32(double(-m) / sqrt((m_x m_x + m_y m_y) + m_z m_z)) per axis, the square root and its argument in fp64;
 *       dir = (0, 0, -1) when that length is zero or not finite.
 *     An entry whose triangle id is >= n_triangles (the empty upper half of the last block of an odd count) or whose triangle
 *     names a vertex outside [0, n_vertices) is invalid: valid = 0, xyz = (0, 0, 0), dir = (0, 0, -1); nothing is read out of
 *     bounds.  `cols` only has to describe an atlas within the limits below.
 *   jt_texture_pack: rgb [count][3] fp32 and valid [count] of the same entry range into atlas, which the caller has zeroed:
 *     floor(255 c + 0.5) in fp64 clamped to 0 .. 255, 0 for a NaN; an invalid entry writes nothing.  Distinct entries write
 *     distinct bytes: no atomics, the same bits on every run.
 *   jt_raster_resolve_texture: jt_raster_resolve with the atlas in place of vertex attributes.  tri and depth are the bits
 *     jt_raster_resolve writes; out [n_views][H][W][3] fp32 is, at a pixel whose winner is t, the bilinear sample of chart t & 1 of
 *     block t >> 1 at (s, u) = (l1 L, l2 L), l the perspective-correct weights of jt_raster_resolve: i0 = min(max(int(floorf(s)),
 *     0), S - 2), fx = s - i0 (j0, fy likewise from u), the four texels (i0 + di, j0 + dj) in chart coordinates fetched as
 *     float(byte) / 255.f, out = lerp(lerp(c00, c10, fx), lerp(c01, c11, fx), fy) with lerp(p, q, f) = fmaf(f, q - p, p) -- a
 *     constant texture comes back exactly; background [3] (a HOST pointer) where nothing was drawn.
 * One launch each on `stream`, nothing else; every argument is checked before the launch.  JT_ERR_ARG for a NULL pointer, a size
 * or count below 1, a negative start, an entry range beyond the atlas, W_atlas != cols S, H_atlas no multiple of S, or an atlas
 * of fewer charts than triangles; JT_ERR_UNSUPPORTED for S outside 4 .. 64, an atlas side beyond 16384, ceil(n_triangles / 2) S S,
 * n_vertices or 3 n_triangles reaching 2^31, and what jt_raster_resolve refuses. */
#define JT_TEXTURE_MIN_BLOCK 4
#define JT_TEXTURE_MAX_BLOCK 64
#define JT_TEXTURE_MAX_SIDE 16384
int jt_texture_texels(const float* vertices, const float* normals, long n_vertices, const int32_t* triangles, long n_triangles,
                      int S, int cols, long start, long count, float* xyz, float* dirs, uint8_t* valid, void* stream);
int jt_texture_pack(const float* rgb, const uint8_t* valid, int S, int cols, long start, long count, uint8_t* atlas, int H_atlas,
                    int W_atlas, void* stream);
int jt_raster_resolve_texture(const uint64_t* zbuf, const float* screen, int n_vertices, const int32_t* triangles,
                              long n_triangles, int n_views, int H, int W, const uint8_t* atlas, int S, int cols, int H_atlas,
                              int W_atlas, const float* background, int32_t* tri, float* depth, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Visible surface (csrc/jt_visible.hip): which triangles of a mesh its cameras see, decided from what jt_raster_draw leaves --
 * the index of the nearest triangle in the low word of every pixel's 64-bit key, decided in integers, the same bits on every run.
 * Integer work throughout; the only atomics are integer additions, so no result depends on the order of execution and a NumPy
 * statement of this comment reproduces the kernels bit for bit (tests/visible_ref.py).  No resolve is needed.
 *
 *   jt_visible_tally: zbuf [n_views][H][W] uint64 as jt_raster_draw leaves it -> pix [n_views][n_triangles] uint32, zeroed by the
 *     caller: for every pixel whose key is not all-ones, pix[view][key & 0xffffffff] += 1.  A low word >= n_triangles is skipped,
 *     never used as an index.  Lanes take consecutive pixels and a wave adds a run of equal (view, index) once, with the run's
 *     length, from its first lane; a run ends at a view boundary (H W need not be a multiple of 64).  With JT_VISIBLE_RUNS=0 in
 *     the environment (read at every call) one atomic per counted pixel instead: the same sums.
 *   jt_visible_fold: one lane per triangle, no atomics: views[t] += #{v : pix[v][t] >= min_pixels} (int32) and pixels[t] += sum_v
 *     pix[v][t] (int64), both read and written: slabs of views compose by one call per slab.  min_pixels >= 1.
 *   jt_visible_mark: flag[v] = 1 for the three vertices of every triangle with visible[t] != 0 whose ids all lie in [0, n_vertices)
 *     (flag [n_vertices] uint8, zeroed by the caller; several lanes may store the same 1; no atomics);
 *   jt_visible_spread: visible_out[t] = visible_in[t] | (ids in range and a flag set on one of them).  The step between the two is
 *     a grid-wide dependency, hence two launches; `rings` applications of the pair grow the set by `rings` rings of vertex
 *     neighbours.  visible_out may not alias visible_in.
 *   jt_mesh_select_count: the per-triangle counterpart of jt_mesh_filter_count: keep_out[t] = 1 iff keep_in[t] != 0 and the three
 *     ids lie in [0, n_vertices), used[v] = 1 for every vertex of a kept triangle (used [n_vertices], zeroed by the caller; no
 *     atomics).  The caller scans keep_out and used and compacts with jt_mesh_filter_emit, as after jt_mesh_filter_count.
 * One launch each on `stream`, nothing else; every argument is checked before the launch.  JT_ERR_ARG for a NULL pointer, a size
 * or count below 1 or min_pixels < 1; JT_ERR_UNSUPPORTED when n_views H W, n_vertices or 3 n_triangles reaches 2^31. */
int jt_visible_tally(const uint64_t* zbuf, int n_views, int H, int W, long n_triangles, uint32_t* pix, void* stream);
int jt_visible_fold(const uint32_t* pix, int n_views, long n_triangles, int min_pixels, int32_t* views, int64_t* pixels,
                    void* stream);
int jt_visible_mark(const int32_t* triangles, long n_triangles, long n_vertices, const uint8_t* visible, uint8_t* flag,
                    void* stream);
int jt_visible_spread(const int32_t* triangles, long n_triangles, long n_vertices, const uint8_t* visible_in, const uint8_t* flag,
                      uint8_t* visible_out, void* stream);
int jt_mesh_select_count(const int32_t* triangles, long n_triangles, long n_vertices, const uint8_t* keep_in, uint8_t* keep_out,
                         uint8_t* used, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Depth-map fusion (csrc/jt_fusion.hip): the depth maps a field RENDERS from its cameras fused into a truncated signed distance
 * volume on the lattice jt_mesh_count / jt_mesh_emit extract.  The reference exports no geometry (it kept only the `trimesh:`
 * option block); the maps are those of its render, batBase.py:147-150, with the background term and the offset undone by the
 * caller.  One lane per lattice point, no atomics, no LDS; every fp32 operation is rounded on its own (no fused multiply-add), so
 * a NumPy float32 statement of this comment reproduces the kernels bit for bit (tests/fusion_ref.py).
 *
 *   jt_fusion_integrate: adds the n_views views of the call, in ascending order, into the running state sum [nx][ny][nz] fp32 and
 *     count [nx][ny][nz] int32 (z fastest; zeroed by the caller before the first call; read and written once per call, so slabs of
 *     views compose to the bits of one call).  depth, opacity: [n_views][H][W] fp32, depth along the camera axis; proj: [n_views][3]
 *     [4] fp32 as jt_raster_project takes it (intr @ [R|t]: the third row gives the camera-axis depth w).  lo3 / hi3 are HOST
 *     pointers.  Per point (i, j, k) and view:
 *       x, y, z = P_axis(index) = lo (1 - s) + hi s with s = float(index) / float(n - 1): jt_mesh_emit's lattice positions;
 *       xw = ((p00 x + p01 y) + p02 z) + p03, left to right, likewise yw (row 1) and w (row 2);
 *       skipped unless w > near; u = xw / w, v = yw / w; skipped unless 0 <= u < W and 0 <= v < H (a NaN fails every test);
 *       col = (int)u, row = (int)v: the nearest pixel, centres at half-integers, no filtering;
 *       d = depth[view][row][col], a = opacity[view][row][col]; the ray found a surface iff d is finite, d > 0 and a >=
 *       min_opacity.  Without one: carve != 0 counts the point as seen empty (sum += 1, count += 1), carve == 0 skips the view.
 *       With one: s = d - w; s < -trunc skips the view (the point is occluded); else t = s / trunc, 1 where t > 1; sum += t,
 *       count += 1.
 *   jt_fusion_finish: per point of the n: count >= min_views gives lattice = 0.5 (1 - sum / float(count)) and seen = 1, else
 *     lattice = 0 and seen = 0 (lattice [n] fp32, seen [n] uint8).  The lattice is occupancy-like: 1 deep inside, 0 outside or
 *     unknown, the surface at level 0.5.
 * One launch each on `stream`, nothing else; every argument is checked before the launch.  JT_ERR_ARG for a NULL pointer, any n <
 * 2, n_views < 0, H or W < 1, trunc not a positive finite number, a NaN min_opacity or near, min_views < 1; JT_ERR_UNSUPPORTED when
 * nx ny nz > 2^27 or n_views H W reaches 2^31; n_views == 0 launches nothing (depth, opacity and proj may then be NULL) and is
 * JT_OK. */
int jt_fusion_integrate(const float* depth, const float* opacity, const float* proj, int n_views, int H, int W, int nx, int ny,
                        int nz, const float* lo3, const float* hi3, float trunc, float min_opacity, int carve, float near,
                        float* sum, int32_t* count, void* stream);
int jt_fusion_finish(const float* sum, const int32_t* count, long n, int min_views, float* lattice, uint8_t* seen, void* stream);

/* LPIPS with the AlexNet backbone: the `self.lpips_loss = lpips.LPIPS(net="alex")` of model/nerf.py:33 and its call
 * `self.lpips_loss(rgb_map * 2 - 1, var.image * 2 - 1)` of model/nerf.py:551, as launches on `stream` (csrc/jt_lpips.hip).  Stock
 * ops run the five convolutions through a vendor convolution library; here they are implicit GEMMs on the fp32-input matrix
 * cores (v_mfma_f32_32x32x2_f32), whose result is bit for bit a k-ordered fmaf chain.
 *
 *   jt_conv_pack_weights: (model/nerf.py:33, the weights the package loads) w [c_out][c_in][kh][kw] fp32, torch's layout ->
 *     packed [Kpad][c_out], K = c_in kh kw, Kpad = K rounded up to JT_CONV_K_STEP, packed[k][m] = w[m][k] with k = (ci kh + ky) kw
 *     + kx and zero rows behind K: the K-major image the kernel reads.  Done once per weight file.  jt_conv_packed_floats = Kpad
 *     c_out (0 for sizes below 1 or at 2^31 elements).
 *   jt_conv2d_relu_forward: (model/nerf.py:551, one layer of the backbone) out = relu(conv2d(x, w, stride, pad) + bias), x [batch]
 *     [c_in][h][w], out [batch][c_out][oh][ow], oh = (h + 2 pad - kh) / stride + 1.  GEMM M = c_out, N = batch oh ow (the pixels of
 *     all pictures flattened; a tile may straddle two pictures), K as above; the operand of the activation is gathered on the
 *     fly, taps outside the picture read as zero.  Every output element is ONE fp32 accumulator chain over k ascending from 0,
 *     then one fp32 add of the bias, then ReLU: the same bits for every `variant` (JT_CONV_TILE_*: the workgroup's tile, channels x
 *     pixels; AUTO picks by the layer's size), for every batch the picture is part of, and run to run.  Against the exact
 *     result: |out - exact| <= (K + 2) 2^-24 (conv(|x|, |w|) + |bias|).  Instantiated for (kh, kw, stride, pad) = (11, 11, 4, 2),
 *     (5, 5, 1, 2), (3, 3, 1, 1) and c_out a multiple of 32 (of 64 for JT_CONV_TILE_64X64): anything else, and an input, output
 *     or weight tensor of 2^31 elements or more, is JT_ERR_UNSUPPORTED.
 *   jt_maxpool_3x3s2_forward: (model/nerf.py:551, the two 3x3 stride-2 max-pools of the backbone) x [planes][h][w] -> out [planes][(h - 3) / 2 + 1][(w - 3)
 *     / 2 + 1], floor mode, no padding; h, w >= 3.
 *   jt_lpips_forward: (model/nerf.py:551) pred, target [n_views][3][height][width] fp32 in [0, 1] (NOT clamped: the reference
 *     passes the render as it is) -> out [n_views] fp64 and, unless NULL, layers [n_views][5] fp64 with out[v] = the sum of
 *     layers[v][0..4] in ascending order.  Steps: both pictures through ((2 x - 1) - shift_c) / scale_c (fp32, the order of
 *     operations stated in csrc/jt_lpips.hip) into ONE batch of 2 n_views; conv 3->64 11x11/4/2 + ReLU; pool, conv 64->192 5x5/1/2
 *     + ReLU; pool, conv 192->384 3x3/1/1 + ReLU; conv 384->256 + ReLU; conv 256->256 + ReLU; after each ReLU, per pixel in fp64:
 *     n_i = sqrt(sum_c f_i^2) + 1e-10, sum_c lin_c (f0_c / n0 - f1_c / n1)^2, and the mean over the layer's pixels.  Every sum
 *     has one order (no atomics): the same bits run to run, and a view's value does not depend on the other views.  Identical
 *     pictures give exactly 0.  weights: a HOST struct of device pointers: conv[l] packed by jt_conv_pack_weights, bias[l]
 *     [c_out], lin[l] [c_out] fp32 (the package's lin<l>.model.1.weight).  workspace: jt_lpips_workspace_bytes(...) bytes,
 *     caller-provided, 256-byte aligned, overwritten; jt_lpips_feature_layout writes table[l] = {offset in floats of layer l's
 *     features [2 n_views][C][h][w] inside the workspace (pictures 0..n_views-1 = pred), C, h, w}, l = 0..4.  Decided before any
 *     launch: JT_ERR_ARG for a NULL pointer, a size below 1 or a short workspace; JT_ERR_UNSUPPORTED for height or width below
 *     31 (the second pool needs 3 rows) and for any activation of the 2 n_views batch with 2^31 elements or more (workspace
 *     bytes: 0 then). */
#define JT_CONV_K_STEP 32
#define JT_CONV_TILE_AUTO 0
#define JT_CONV_TILE_64X64 1  /* 4 waves, 2 x 2 */
#define JT_CONV_TILE_32X32 2 /* 1 wave */
typedef struct JtLpipsWeights {
  const float* conv[5];
  const float* bias[5];
  const float* lin[5];
} JtLpipsWeights;
size_t jt_conv_packed_floats(int c_out, int c_in, int kh, int kw);
int jt_conv_pack_weights(const float* w, int c_out, int c_in, int kh, int kw, float* packed, void* stream);
int jt_conv2d_relu_forward(const float* x, const float* packed, const float* bias, int batch, int c_in, int h, int w, int c_out,
                           int kh, int kw, int stride, int pad, int variant, float* out, void* stream);
int jt_maxpool_3x3s2_forward(const float* x, int planes, int h, int w, float* out, void* stream);
size_t jt_lpips_workspace_bytes(int n_views, int height, int width);
int jt_lpips_feature_layout(int n_views, int height, int width, int64_t* table);
int jt_lpips_forward(const float* pred, const float* target, int n_views, int height, int width, const JtLpipsWeights* weights,
                     double* out, double* layers, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* JT_RENDER_H */
