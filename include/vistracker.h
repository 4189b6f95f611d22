/*
 * vistracker.h -- C ABI of libvistracker_hip.so: the MI355X (gfx950) implementation of the VisTracker
 * per-frame SMPL-H / object fitting hot path.
 *
 * The reference has no FFI: its "operator API" for this path is the set of duck-typed Python callables the
 * fitters invoke.  Each entry point below names the reference callable it replaces
 * (paths relative to the reference tree).  The Python shims in vistracker_amd/ bind these with ctypes and
 * re-expose the reference's call signatures (smpl(), get_landmarks(), model.query()/get_preds(),
 * SilLossROI(...), chamfer_distance(...)).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to a contiguous row-major array (float = fp32, int = int32)
 *     unless the parameter is documented "host".
 *   - the library never allocates outputs or scratch: the caller passes them (sizes documented per call);
 *     handles own only immutable constants uploaded at creation.
 *   - every call enqueues on the caller's HIP stream (`stream` = hipStream_t cast to void*) and returns
 *     without synchronising; no global mutable state besides the per-thread error string.
 *   - return value: 0 = ok, negative = error (see vt_last_error()).
 */
#ifndef VISTRACKER_H
#define VISTRACKER_H

#include <stddef.h>     /* size_t (vt_grad_rank_mean) */

#ifdef __cplusplus
extern "C" {
#endif

#define VT_OK 0
#define VT_ERR_ARG -1
#define VT_ERR_HIP -2
#define VT_ERR_BUSY -3     /* the resource is already held by the same thread (vt_stream_set_skip_flag: another stop flag registered for the stream) */

#define VT_SMPL_V 6890
#define VT_SMPL_J 52
#define VT_SMPL_NB 10
#define VT_SMPL_NP 459
#define VT_FEAT 611
#define VT_HID 128

const char *vt_last_error(void);
int vt_version(void);

/* ---------------------------------------------------------------------------------------------------
 * SMPL-H layer.  Replaces SMPL_Layer.forward (lib_smpl/smplpytorch/smplpytorch/pytorch/smpl_layer.py:73-176),
 * th_posemap_axisang / batch_rodrigues (tensutils.py:6-19, rodrigues_layer.py:38-52) and its autograd backward.
 * ------------------------------------------------------------------------------------------------- */
typedef struct vt_smplh vt_smplh;

/* HOST pointers: v_template (V,3), shapedirs (V,3,NB), posedirs (V,3,NP), J_regressor (J,V) dense,
 * weights (V,J), parents (J) [parents[0] ignored].  smpl_layer.py:46-71. */
int vt_smplh_create(vt_smplh **out, const float *v_template, const float *shapedirs, const float *posedirs,
                    const float *J_regressor, const float *weights, const int *parents, void *stream);
void vt_smplh_destroy(vt_smplh *h);

/* floats of per-call workspace `ws` for batch B (kept by the caller between forward and backward) */
long vt_smplh_workspace_floats(int B);

/* pose (B,156) betas (B,10) trans (B,3) -> verts (B,6890,3), jtr (B,52,3), v_posed (B,6890,3)  */
int vt_smplh_forward(const vt_smplh *h, const float *pose, const float *betas, const float *trans, int B,
                     float *verts, float *jtr, float *v_posed, float *ws, void *stream);

/* dverts (B,6890,3), djtr (B,52,3) or NULL -> dpose (B,156), dbetas (B,10), dtrans (B,3)  (overwritten).
 * `ws` and `v_posed` must be the buffers the matching forward filled.  scratch: vt_smplh_bwd_scratch_floats(B). */
long vt_smplh_bwd_scratch_floats(int B);
int vt_smplh_backward(const vt_smplh *h, const float *pose, const float *betas, int B, const float *dverts,
                      const float *djtr, const float *v_posed, const float *ws, float *scratch,
                      float *dpose, float *dbetas, float *dtrans, void *stream);

/* The same layer for a fit that keeps the hand joints fixed: SMPLHFitter's optimisers (lib_smpl/fit_SMPLH_30fps.py init_globalpose_optimizer /
 * init_allpose_optimizer; recon/recon_fit_behave.py:430-451) hold trans, pose[:, :66] and betas only, so pose[:, 66:] (joints 22..51) is the same
 * at every step of a fit and what SMPL_Layer.forward computes from it can be done once.
 *   vt_smplh_prefix            pose (B,156) -> the rotations of joints 22..51 in `ws` and the blend-shape accumulators after the hand
 *                              pose-map rows in `prefix` (vt_smplh_prefix_floats(B) floats, layout private to the library).
 *   vt_smplh_forward_prefixed  vt_smplh_forward on top of (`ws`, `prefix`): the SAME `ws` the prefix call filled; it reads pose[:, :66] only.
 *                              Outputs are bit-identical to vt_smplh_forward's as long as pose[:, 66:] is what the prefix call saw.
 *   vt_smplh_backward_free     vt_smplh_backward for the first n_free_pose_cols pose columns (a multiple of 3, at most 66): dpose[:, :n], dbetas and
 *                              dtrans are bit-identical to vt_smplh_backward's, dpose[:, n:] is NOT written.  Works behind either forward. */
long vt_smplh_prefix_floats(int B);
int vt_smplh_prefix(const vt_smplh *h, const float *pose, int B, float *ws, float *prefix, void *stream);
int vt_smplh_forward_prefixed(const vt_smplh *h, const float *pose, const float *betas, const float *trans, int B, const float *prefix,
                              float *verts, float *jtr, float *v_posed, float *ws, void *stream);
int vt_smplh_backward_free(const vt_smplh *h, const float *pose, int B, const float *dverts, const float *djtr, const float *v_posed,
                           const float *ws, float *scratch, int n_free_pose_cols, float *dpose, float *dbetas, float *dtrans, void *stream);

/* batch_rodrigues alone: aa (n,3) -> R (n,9); and its VJP */
int vt_rodrigues_forward(const float *aa, int n, float *R, void *stream);
int vt_rodrigues_backward(const float *aa, int n, const float *dR, float *daa, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * Sparse landmark regressors.  Replaces load_regressors + batch_sparse_dense_matmul
 * (lib_smpl/body_landmark.py:16-28, lib_smpl/torch_functions.py:52-76).
 * ------------------------------------------------------------------------------------------------- */
typedef struct vt_landmarks vt_landmarks;
/* HOST CSR of the (K x V) regressor */
int vt_landmarks_create(vt_landmarks **out, const int *indptr, const int *indices, const float *data, int K, int V,
                        void *stream);
void vt_landmarks_destroy(vt_landmarks *h);
/* verts (B,V,3) -> out (B,K,3) */
int vt_landmarks_forward(const vt_landmarks *h, const float *verts, int B, float *out, void *stream);
/* dout (B,K,3) -> dverts (B,V,3) += (accumulate != 0) or = (accumulate == 0; rows without entries zeroed) */
int vt_landmarks_backward(const vt_landmarks *h, const float *dout, int B, float *dverts, int accumulate, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * Mahalanobis priors.  Replaces th_Mahalanobis.__call__ (lib_smpl/th_smpl_prior.py:30-38) and
 * HandPrior.__call__ (lib_smpl/th_hand_prior.py:57-72):  value[b] = | (x[b, off:off+n] - mean) @ prec |^2.
 * dx (B,stride) += gscale * d value[b] / dx  when dx != NULL.   mean (n), prec (n,n) device, n <= 64.
 * ------------------------------------------------------------------------------------------------- */
int vt_mahalanobis(const float *x, int B, int stride, int off, int n, const float *mean, const float *prec,
                   float *value, float *dx, float gscale, void *stream);

/* Loss-term accumulators: every `double *term` below is a DEVICE fp64 scalar the kernels add to with atomics
 * (fp64 keeps the sum order-independent to ~1e-16, so step losses and the early-stop decision are reproducible).
 * Zero them (vt_fill_f64) before the step. */
int vt_fill_f64(double *p, long n, double value, void *stream);
/* *term += scale * sum(value[0..n)) */
int vt_sum_to_term(const float *value, int n, float scale, double *term, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * SIF-Net point query.  Replaces CHORETriplane.query + CHORETriplaneVisibility.decode + get_preds
 * (model/chore_triplane.py:97-164,207-251; model/chore_tri_vis.py:17-50; model/camera.py:45-90;
 * model/geometry.py:4-14) and the autograd backward to the query coordinates.
 * Heads (bit index in head masks): 0 df(2) 1 pca(9) 2 parts(14) 3 centers(3) 4 vis(1).
 * ------------------------------------------------------------------------------------------------- */
typedef struct vt_sifnet vt_sifnet;
/* HOST weights: w[h*4+l] is (out,in) row-major (torch Conv1d.weight[:, :, 0]), b[h*4+l] is (out);
 * cam (host, 5 floats) = {fx_px, fy_px, cx_px, cy_px, crop_size} (camera.py:26-41). */
int vt_sifnet_create(vt_sifnet **out, const float *const *w, const float *const *b, const float *cam, void *stream);
void vt_sifnet_destroy(vt_sifnet *h);

/* Feature maps are consumed channel-last.  Converts one NCHW map (B,C,H,W) to NHWC (B,H,W,C). */
int vt_nchw_to_nhwc(const float *src, int B, int C, int H, int W, float *dst, void *stream);

/* maps (host array of 8 device pointers, NHWC) in the order im_feat(256) tmpx(64) tri_tmpx{right,back,top}(32)
 * tri_feat{right,back,top}(64); res (host, 8 ints) = H (=W) of each map. */
typedef struct {
    const float *maps[8];
    int res[8];
    /* optional: hoisted layer-1 projection of im_feat, (B, res[0], res[0], proj_cols) floats written by vt_query_build_projection for THESE
     * maps and THIS network (NULL = not available).  Layer 1 of the decoders (Conv1d(611,128), chore.py:113-126) is linear in the features
     * and the features are bilinear blends of texels (geometry.py:4-14), so its im_feat part can be applied to the texels once per batch
     * instead of to every query point at every optimisation step; the fused objective / projection-step entry points then blend rows of
     * this array instead of gathering the 256 im_feat channels and multiplying them by W1.  Results agree to fp32 round-off. */
    const float *proj;
    int proj_cols;
    /* operand-range level of the split-f16 decoders for the calls that pass THESE maps: level k runs the last hidden layer at the operand scale
     * 2^(6 - 4 k) (representable |activation| < 1023, 16 368, 262 016 for k = 0, 1, 2; the earlier layers have at least that range -- the decoders
     * of model/chore.py:113-126 have no such bound); beyond it a call yields NaN, loudly.  Same weights, exact power-of-two rescaling of biases /
     * features / outputs, so a checkpoint with large activations costs one repeated launch at the next level, not the 5x slower fp32 route.
     * proj_level = the level `proj` was built for (vt_query_build_projection uses act_level; a projection of another level is ignored).
     * Zero-initialised = level 0. */
    int act_level;
    int proj_level;
    /* non-zero: these calls run on the strict-fp32 kernels whatever the handle's precision (per batch, so concurrent fits through one handle do
     * not see each other's switch) */
    int force_fp32;
} vt_maps;

/* pts (B,N,3), crop_center (B,2), body_center (B,3).  Outputs may be NULL (head skipped); layout as the
 * reference: df (B,2,N), pca (B,9,N), parts (B,14,N), centers (B,3,N), vis (B,1,N). */
int vt_query_forward(const vt_sifnet *h, const vt_maps *maps, const float *pts, const float *crop_center,
                     const float *body_center, int B, int N,
                     float *df, float *pca, float *parts, float *centers, float *vis, void *stream);
/* upstream gradients in the same layouts (NULL = zero) -> dpts (B,N,3) (overwritten) */
int vt_query_backward(const vt_sifnet *h, const vt_maps *maps, const float *pts, const float *crop_center,
                      const float *body_center, int B, int N,
                      const float *d_df, const float *d_pca, const float *d_parts, const float *d_centers,
                      const float *d_vis, float *dpts, void *stream);

/* floats of the projection array for a batch of B frames, and its construction (one fp32 GEMM over all im_feat texels; heads df | parts) */
long vt_query_projection_floats(const vt_maps *maps, int B);
int vt_query_build_projection(const vt_sifnet *h, const vt_maps *maps, int B, float *proj, void *stream);

/* Fused objective kernels of the two fit loops (no autograd tape, one launch per step):
 *  human:  loss += w_dfh * mean_{B,N} clamp(df[:,0], max=.1) + w_part * mean_B sum_N CE(parts, labels)
 *          (recon_fit_base.py:640-647, recon_fit_behave.py:486); labels (N) int32
 *  object: loss += w_obj * mean_B( mean_N clamp(df[:,1], max=.8) * occ[b] )   (recon_fit_trivis_full.py:155-162)
 * dpts (B,N,3) is overwritten with the weighted gradient; terms[0..1] (device fp64) receive the UNWEIGHTED term
 * values (df_h, part) or (object, -) accumulated with atomics -- zero them before the call. */
/* order (N) int32 or NULL: a permutation of the point indices -- workgroup slot n processes point order[n] (inputs read, labels looked
 * up and dpts written at the ORIGINAL index, so results do not depend on it); a locality-preserving order (e.g. the Morton order of the
 * template vertices) makes the 64 points of a workgroup gather from neighbouring texels. */
int vt_query_human_loss(const vt_sifnet *h, const vt_maps *maps, const float *pts, const float *crop_center,
                        const float *body_center, int B, int N, const int *labels, const int *order, float w_dfh, float w_part,
                        float *dpts, double *terms, void *stream);
int vt_query_object_loss(const vt_sifnet *h, const vt_maps *maps, const float *pts, const float *crop_center,
                         const float *body_center, int B, int N, const float *occ, float w_obj,
                         float *dpts, double *terms, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * 3x3 / stride 1 / pad 1 bias-free convolution of the HGFilter encoders (model/HGFilters.py:56-203, model/net_util.py:346-396 ConvBlock) as a
 * split-f16 implicit GEMM (fp32 accumulate, same operand format as the point query).  weight (Cout, Cin, 3, 3) fp32 host, Cout in {32, 64, 128} (32: the 64-channel kernel with zero rows, half its waves idle in the MFMA phase),
 * Cin a multiple of 32.  in (B,H,W,Cin) NHWC fp32 device, H % 8 == 0, W % 16 == 0; the result goes to channels [out_coff, out_coff + Cout) of an
 * NHWC tensor with out_cstride channels (a ConvBlock's concatenation can be written in place).  A value beyond the operand range yields NaN.
 * ------------------------------------------------------------------------------------------------- */
typedef struct vt_conv3x3 vt_conv3x3;
int vt_conv3x3_create(vt_conv3x3 **out, const float *weight, int cout, int cin, void *stream);
void vt_conv3x3_destroy(vt_conv3x3 *h);
int vt_conv3x3_forward(const vt_conv3x3 *h, const float *in, int B, int H, int W, float *out, int out_cstride, int out_coff, void *stream);
/* The pre-activated form of the ConvBlock (GroupNorm -> ReLU -> conv, model/net_util.py:374-388) in one pass: the input is channels
 * [in_coff, in_coff + Cin) of an NHWC tensor with in_cstride channels; with gn_stats != NULL (the (B, groups) {mean, rstd} pairs of
 * vt_groupnorm_stats) max((x - mean) rstd gamma + beta, 0) is applied while the operand planes are staged (zero padding pads the rectified value). */
int vt_conv3x3_forward_gn(const vt_conv3x3 *h, const float *in, int in_cstride, int in_coff, const float *gn_stats, const float *gamma,
                          const float *beta, int groups, int B, int H, int W, float *out, int out_cstride, int out_coff, void *stream);
/* The same with the GroupNorm partial sums of the OUTPUT as a by-product (per 8 x 16 pixel tile, vt_conv3x3_tiles(H, W) of them, at
 * stats_ws + B * stats_groups doubles): vt_groupnorm_finalize(stats_ws, tiles, B, H * W, Cout, stats_groups, eps) turns them into the {mean, rstd}
 * pairs at the start of stats_ws -- the statistics the next convolution of a ConvBlock needs, without a pass over the tensor.
 * stats_ws >= B stats_groups + tiles B Cout 2 doubles (NULL: no statistics). */
int vt_conv3x3_forward_gn_stats(const vt_conv3x3 *h, const float *in, int in_cstride, int in_coff, const float *gn_stats, const float *gamma,
                                const float *beta, int groups, int B, int H, int W, float *out, int out_cstride, int out_coff, double *stats_ws,
                                int stats_groups, void *stream);
/* The general form (one ConvBlock step): out (or NULL) <- convolution, fin (or NULL) <- convolution + res, the block's result for these channels
 * (model/net_util.py:390-394: the residual add without a pass of its own). */
int vt_conv3x3_forward_block(const vt_conv3x3 *h, const float *in, int in_cstride, int in_coff, const float *gn_stats, const float *gamma,
                             const float *beta, int groups, int B, int H, int W, float *out, int out_cstride, int out_coff,
                             const float *res, int res_cstride, int res_coff, float *fin, int fin_cstride, int fin_coff,
                             double *stats_ws, int stats_groups, void *stream);
int vt_conv3x3_tiles(int H, int W);
/* The 7 x 7 / stride 2 / pad 3 convolution at the head of an encoder (model/HGFilters.py:118-130: self.conv1 = nn.Conv2d(in_ch, 64, kernel_size=7, stride=2,
 * padding=3), applied at HGFilters.py:166 `x = F.relu(self.bn1(self.conv1(x)), True)`): plain fp32 multiply-adds like the reference's, weights as scalar
 * operands (csrc/stem.hip).  weight (Cout, Cin, 7, 7) fp32 host, bias (Cout) fp32 host or NULL, Cout in {32, 64} (triplane / image encoder), Cin in 1..8.
 * forward: the input is channels [in_coff, in_coff + Cin) of an NHWC tensor (B, H, W, in_cstride), the result (B, ceil(H / 2), ceil(W / 2), Cout) goes to channels [out_coff, out_coff + Cout)
 * of an NHWC tensor with out_cstride channels (both multiples of 4).  Replaces the encoder's last MIOpen call (round 6). */
typedef struct vt_stem7x7 vt_stem7x7;
int vt_stem7x7_create(vt_stem7x7 **out, const float *weight, const float *bias, int cout, int cin, void *stream);
void vt_stem7x7_destroy(vt_stem7x7 *h);
int vt_stem7x7_forward(const vt_stem7x7 *h, const float *in, int in_cstride, int in_coff, int B, int H, int W, float *out, int out_cstride, int out_coff, void *stream);
/* The 1 x 1 convolutions of the same encoders (conv_last / l / bl / al of a stack, the ConvBlock's down-sampling projection: model/HGFilters.py:150-203,
 * model/net_util.py:364-372) on the same split-f16 kernel (one tap, the 8 x 16 tile as the patch).  weight (Cout, Cin) fp32 host, bias (Cout) or NULL,
 * Cout in {64, 128, 256} (256 runs as two launches of 128), Cin in {32, 64, 128, 256}.  forward: out <- conv(in) + bias [+ res]; gn_stats != NULL applies
 * max((x - mean) rstd gamma + beta, 0) to the input while it is staged (the GroupNorm -> ReLU in front of l / bl / the projection); stats_ws != NULL
 * leaves the GroupNorm partial sums of conv(in) + bias behind like vt_conv3x3_forward_gn_stats (finalize with C = Cout). */
typedef struct vt_conv1x1 vt_conv1x1;
int vt_conv1x1_create(vt_conv1x1 **out, const float *weight, const float *bias, int cout, int cin, void *stream);
void vt_conv1x1_destroy(vt_conv1x1 *h);
int vt_conv1x1_forward(const vt_conv1x1 *h, const float *in, int in_cstride, int in_coff, const float *gn_stats, const float *gamma, const float *beta, int groups,
                       int B, int H, int W, float *out, int out_cstride, int out_coff, const float *res, int res_cstride, int res_coff,
                       double *stats_ws, int stats_groups, void *stream);
int vt_groupnorm_finalize(double *ws, int nblk, int B, int HW, int C, int groups, float eps, void *stream);
/* vt_conv3x3_forward_block + the GroupNorm partial sums of `fin` (convolution + residual: the ConvBlock's result, model/net_util.py:390-394) for the
 * ConvBlock that reads it next: every launch of a block writes the partials of its channel slice [fin_coff, fin_coff + Cout) into one block of
 * fin_cstride channels per 8 x 16 pixel tile at fin_stats_ws + B * fin_stats_groups doubles; after the block's last launch
 * vt_groupnorm_finalize(fin_stats_ws, vt_conv3x3_tiles(H, W), B, H * W, fin_cstride, fin_stats_groups, eps) yields what vt_groupnorm_stats(fin) would. */
int vt_conv3x3_forward_block_stats(const vt_conv3x3 *h, const float *in, int in_cstride, int in_coff, const float *gn_stats, const float *gamma,
                                   const float *beta, int groups, int B, int H, int W, float *out, int out_cstride, int out_coff,
                                   const float *res, int res_cstride, int res_coff, float *fin, int fin_cstride, int fin_coff,
                                   double *stats_ws, int stats_groups, double *fin_stats_ws, int fin_stats_groups, void *stream);
/* 2 x 2 average pooling of an NHWC tensor (F.avg_pool2d(x, 2, stride=2): model/HGFilters.py:33,131-136), x (B, H, W, C) -> out (B, H/2, W/2, C), and
 * -- stats_ws != NULL -- the GroupNorm partial sums of the OUTPUT: vt_sweep_blocks(H/2 * W/2) blocks at stats_ws + B * stats_groups doubles, for
 * vt_groupnorm_finalize(stats_ws, vt_sweep_blocks(..), B, H/2 * W/2, C, stats_groups, eps) in place of a statistics pass by the consumer. */
int vt_avgpool2x2_stats(const float *x, int B, int H, int W, int C, float *out, double *stats_ws, int stats_groups, void *stream);
int vt_sweep_blocks(int HW);
/* GroupNorm statistics of a channel slice: ws >= vt_groupnorm_workspace_doubles(B, HW, C, groups) doubles; the (B, groups) {mean, rstd} float pairs
 * are written at the START of ws (pass `(const float *)ws` as gn_stats) */
int vt_groupnorm_stats(const float *x, int cstride, int coff, int B, int HW, int C, int groups, float eps, double *ws, void *stream);

/* Arithmetic of the decoder GEMMs behind every vt_query_* call of a handle:
 *   VT_PRECISION_SPLIT_F16 (default): 22-bit split-f16 operands on the f16 MFMA, fp32 accumulate (5.3x the f32-input MFMA rate; forward within
 *       ~1e-6 of the fp32 reference); activations must satisfy |x| < 1023 * 16^(vt_maps::act_level), beyond that the result is NaN;
 *   VT_PRECISION_FP32: exact fp32 products on the f32-input MFMA (the reference's nn.Conv1d arithmetic, model/chore.py:113-126), any magnitude,
 *       ~1/5 of the speed; the hoisted projection of the maps is ignored.
 * The fused fit loops of the host layer switch a handle to VT_PRECISION_FP32 and re-run the batch when the split route produced a non-finite
 * loss.  Per handle, may be changed between calls. */
#define VT_PRECISION_SPLIT_F16 0
#define VT_PRECISION_FP32 1
int vt_sifnet_set_precision(vt_sifnet *h, int mode);
int vt_sifnet_get_precision(const vt_sifnet *h);

/* Kernel selection for vt_query_human_loss when the maps carry the hoisted projection.  The product library holds ONE kernel (256: the two-workgroups-per-CU
 * kernel all query entry points use) and refuses anything else with VT_ERR_ARG.  The experiments build (csrc/experiments, `make experiments`, never shipped)
 * additionally accepts 512 (one 512-thread workgroup per 64-point tile, thin waves) and 128 (producer / consumer waves, 128 points per workgroup): measured
 * 52 % / 22 % slower, kept for A/B measurements and as independently written cross-checks of the same arithmetic.  Process-wide. */
int vt_query_set_human_kernel(int threads);

/* One projection step of the SIF-Net surface-point generator, fused.  Replaces one iteration of
 * Generator.approx_surface (recon/gen/generator.py:72-103): query -> target = clamp(df[:, df_idx], max = threshold) ->
 * autograd of sum(target) to the samples -> samples - F.normalize(grad, dim=2) * target.  df_idx 0 = human, 1 = object.
 * pts_out (B,N,3) may alias pts (every point is read and written by exactly one workgroup); df_target (B,N) or NULL receives
 * the clamped distance at the INPUT positions (what the caller thresholds with filter_val). */
int vt_query_project_step(const vt_sifnet *h, const vt_maps *maps, const float *pts, const float *crop_center,
                          const float *body_center, int B, int N, int df_idx, float threshold, float *pts_out,
                          float *df_target, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * Fused heads / tails of one Adam step of the two fit loops (the vt_objfit_step / vt_smplfit_step of SURVEY.md 8(b)): the arithmetic of the
 * single-purpose entry points below, element for element and in the same order, in 4 launches per object-stage step (head, query, stencils,
 * tail) and one tail per SMPL-stage step.  `terms` (device fp64), `w` (host, per-term weights), `state`, `stop_flag`, `history`, `slot`, `tol`,
 * `armed` as in vt_loss_reduce_and_stop; `ticket`: one zero-initialised device int per fit loop; the workgroup that finishes last closes the step
 * (loss, history, the reference's stop rule recon_fit_trivis_full.py:372 / recon_fit_behave.py:447) and zeroes terms[0, nzero).
 *   vt_objstep_head   R = project_so3(M0 + 1e-4 noise) (recon_fit_base.py:179-199,462-469); X = (X0 R + t) s for the surface points and, if X_verts
 *                     != NULL, the template vertices (recon_fit_base.py:455-459); terms[0, nzero) = 0
 *   vt_temporal_loss2 vt_accel_loss then vt_velocity_loss of (B, D) in one pass; init_zero: dv is written, not accumulated
 *   vt_objstep_tail   rigid VJP over the vertex set (dX_verts != NULL: phase 'sil') and the points, the translation regulariser
 *                     mean (t - t_init)^2 (t_init != NULL; recon_fit_trivis_full.py:227), SO(3) VJP, Adam (torch.optim.Adam) on pR (B,9) / pT (B,3)
 *                     (NULL: that group is not optimised), step end
 *   svd_ws            (B, 22) floats or NULL: vt_objstep_head leaves the SVD of M0 + 1e-4 noise there (U, V, s, det sign) and the tail of the SAME step takes
 *                     it from there instead of decomposing the matrix a second time (the same numbers; ~10 us of one thread per step)
 *   vt_smplstep_tail  body-pose prior th_Mahalanobis on pose[:, 3:66] (th_smpl_prior.py:30-38; gscale_prior = w / B), pinit term mean_B sum
 *                     (pose[:, 3:72] - pose_init)^2 (recon_fit_behave.py:500-503), Adam on up to three column slices (p, stride, g, stride, m, v,
 *                     columns, lr; p == NULL: unused), step end
 * ------------------------------------------------------------------------------------------------- */
/* SMPL-stage step forms: vt_kpts_step = vt_landmarks_forward + vt_kpts_loss + vt_landmarks_backward in one launch (J (B,K,3) or NULL receives the joints; dverts
 * is written -- accumulate = 0 -- or accumulated); vt_query_human_step = vt_query_human_loss whose gradient is ADDED to dpts (accumulate != 0: after vt_kpts_step)
 * and, with term_accel != NULL, the vertex acceleration stencil vt_accel_loss(pts, B, 3 N, NULL, w_accel, term_accel, dpts) in the same launch.  Same values as the
 * separate launches (float additions in the same order).  Split-f16 route only. */
int vt_kpts_step(const vt_landmarks *h, const float *verts, const float *kpts, const float *crop_center, int B, int mode, const float *cam, float net_size,
                 float gscale, double *term, float *J, float *dverts, int accumulate, void *stream);
int vt_query_human_step(const vt_sifnet *h, const vt_maps *maps, const float *pts, const float *crop_center, const float *body_center,
                        int B, int N, const int *labels, const int *order, float w_dfh, float w_part, int accumulate, float w_accel,
                        double *term_accel, float *dpts, double *terms, void *stream);
int vt_objstep_head(const float *M0, const float *noise, const float *t, const float *s, int B, const float *X0_points, int N, float *X_points,
                    const float *X0_verts, int NV, float *X_verts, float *R, double *terms, int nzero, float *svd_ws, void *stream);
int vt_temporal_loss2(const float *v, int B, int D, float gscale_accel, double *term_accel, float gscale_velocity, double *term_velocity, float *dv,
                      int init_zero, void *stream);
int vt_objstep_tail(const float *X0_verts, int NV, const float *dX_verts, const float *X0_points, int N, const float *dX_points, const float *s, int B,
                    const float *M0, const float *noise, const float *t, const float *t_init, float w_trans, double *term_trans,
                    float *dR, float *dt, float *dM,
                    float *pR, float *mR, float *vR, float lrR, float *pT, float *mT, float *vT, float lrT, int adam_step, float beta1, float beta2, float eps,
                    double *terms, const float *w, int nterms, float tol, int armed, float *state, int *stop_flag, float *history, int slot, int *ticket, int nzero,
                    float *svd_ws, void *stream);
/* vt_objstep_tail with the stencils of vt_temporal_loss2(X_points, B, 3 N, ...) evaluated inside it (the same float additions in the same order: bit-identical
 * parameters, one launch less per step); init_zero as there (dX_points is then not read).  For the phases in which nothing else adds to dX_points between the
 * stencils and the tail ('object only', 'sil'). */
int vt_objstep_tail_temporal(const float *X_points, float gscale_accel, double *term_accel, float gscale_velocity, double *term_velocity, int init_zero,
                             const float *X0_verts, int NV, const float *dX_verts, const float *X0_points, int N, const float *dX_points, const float *s, int B,
                             const float *M0, const float *noise, const float *t, const float *t_init, float w_trans, double *term_trans,
                             float *dR, float *dt, float *dM,
                             float *pR, float *mR, float *vR, float lrR, float *pT, float *mT, float *vT, float lrT, int adam_step, float beta1, float beta2, float eps,
                             double *terms, const float *w, int nterms, float tol, int armed, float *state, int *stop_flag, float *history, int slot, int *ticket, int nzero,
                             float *svd_ws, void *stream);
int vt_smplstep_tail(float *pose, const float *pose_init, float *dpose, int B, const float *prior_mean, const float *prior_prec, float gscale_prior,
                     double *term_prior, float w_pinit, double *term_pinit,
                     float *p0, int ps0, const float *g0, int gs0, float *m0, float *v0, int n0, float lr0,
                     float *p1, int ps1, const float *g1, int gs1, float *m1, float *v1, int n1, float lr1,
                     float *p2, int ps2, const float *g2, int gs2, float *m2, float *v2, int n2, float lr2,
                     int adam_step, float beta1, float beta2, float eps,
                     double *terms, const float *w, int nterms, float tol, int armed, float *state, int *stop_flag, float *history, int slot, int *ticket, int nzero,
                     void *stream);

/* ---------------------------------------------------------------------------------------------------
 * SO(3) projection.  Replaces ReconFitterBase.project_so3 / decopose_axis (recon/recon_fit_base.py:179-199,
 * 462-469): R = U diag(1,1,det(U V^T)) V^T of M; noise (B,3,3) or NULL is the U[0,1) sample, M = M0 + 1e-4*noise.
 * ------------------------------------------------------------------------------------------------- */
int vt_so3_project_forward(const float *M0, const float *noise, int B, float *R, void *stream);
int vt_so3_project_backward(const float *M0, const float *noise, int B, const float *dR, float *dM, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * Rigid transform.  Replaces transform_obj_verts (recon/recon_fit_base.py:455-459): X = (X0 @ R + t) * s.
 * X0 (N,3) shared by all frames if shared_x0 != 0 else (B,N,3).
 * ------------------------------------------------------------------------------------------------- */
int vt_rigid_forward(const float *X0, int shared_x0, const float *R, const float *t, const float *s, int B, int N,
                     float *X, void *stream);
/* dX (B,N,3) -> dR (B,3,3), dt (B,3)  (+= if accumulate) */
int vt_rigid_backward(const float *X0, int shared_x0, const float *s, int B, int N, const float *dX,
                      float *dR, float *dt, int accumulate, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * Temporal stencils (recon/recon_fit_trivis_full.py:170-177,379-391; preprocess/fit_SMPLH_30fps.py:189-200).
 *   accel:    mse(v[1:-1]-v[:-2], v[2:]-v[1:-1]) (optionally weighted per element by elem_w (D))
 *   velocity: mse(v[1:], v[:-1])
 * v (B,D).  *term (device scalar) += value;  dv (B,D) += gscale * gradient (dv may be NULL).
 * ------------------------------------------------------------------------------------------------- */
int vt_accel_loss(const float *v, int B, int D, const float *elem_w, float gscale, double *term, float *dv, void *stream);
/* same on the first D columns of a row-strided matrix (v, dv have `stride` floats per frame): pose accelerations */
int vt_accel_loss_strided(const float *v, int B, int D, int stride, const float *elem_w, float gscale, double *term,
                          float *dv, void *stream);
int vt_velocity_loss(const float *v, int B, int D, float gscale, double *term, float *dv, void *stream);

/* 2D keypoint terms.  mode 0: BaseFitter.compute_loss 'kpts' (preprocess/fit_SMPLH_kpts.py:280-310):
 *   mean_{B,25,2}((proj - k_xy)^2 * conf), full-image pinhole.
 * mode 1: projection_loss 'j2d' (recon/recon_fit_base.py:781-802): mean_{B,25}(sum_xy(proj - k)^2 * conf) with the
 *   crop-space projection scaled by net_size / crop_size; crop_center (B,2).
 * J (B,K,3), kpts (B,K,3);  *term += value;  dJ (B,K,3) = gscale * gradient (overwritten). cam (host,5). */
int vt_kpts_loss(const float *J, const float *kpts, const float *crop_center, int B, int K, int mode,
                 const float *cam, float net_size, float gscale, double *term, float *dJ, void *stream);

/* sum_i w_i (a_i - b_i)^2 / denom  over n elements laid out with row strides (rows x cols):
 * pinit terms (fit_SMPLH_30fps.py:178; recon_fit_behave.py:493-495) and 'trans' (recon_fit_trivis_full.py:223). */
int vt_sqdiff_loss(const float *a, int a_stride, const float *b, int b_stride, int rows, int cols, float denom,
                   float gscale, double *term, float *da, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * Human / object interpenetration ("collide", weight 3^2 / (1 + decay) in phase 'joint').  Replaces RegistrationBase.smpl_obj_collision /
 * compute_collision_loss (recon/recon_fit_base.py:97-100,736-765; recon_fit_trivis_full.py:260-264): mesh_intersection's BVH(max_collisions=8)
 * + DistanceFieldPenetrationLoss(sigma=0.5, point2plane=False) -- un-vendored, PARITY UNPINNED, restated from Tzionas et al. 2016.
 * smpl_verts (B,NVs,3), smpl_faces (NFs,3) int32, obj_verts (B,NVo,3) = the TRANSFORMED template, obj_faces (NFo,3) int32, all device.
 * *term += mean over frames of the penetration of the human-object triangle pairs (first max_collisions colliding SMPL faces per object face);
 * d_obj_t (B,3) += gscale * d value / d(object translation)  (the parameter phase 'joint' optimises; NULL to skip);
 * pairs_per_frame (B) int32 device, optional.  workspace: vt_collision_workspace_bytes(B, NFs) bytes, 8-byte aligned.
 * ------------------------------------------------------------------------------------------------- */
long vt_collision_workspace_bytes(int B, int n_smpl_faces);
int vt_collision_loss(const float *smpl_verts, int n_smpl_verts, const int *smpl_faces, int n_smpl_faces, const float *obj_verts, int n_obj_verts,
                      const int *obj_faces, int n_obj_faces, int B, float sigma, int max_collisions, float gscale, double *term,
                      float *d_obj_t, int *pairs_per_frame, void *workspace, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * Ragged contact Chamfer.  Replaces pytorch3d.loss.chamfer_distance(Pointclouds, Pointclouds)[0]
 * (recon/recon_fit_trivis_full.py:454-457; pytorch3d defaults, see DESIGN.md "unpinned").
 * x (nx_total,3), y (ny_total,3), offx/offy (P+1) int32 device.  *term += value.
 * dx, dy (+=, may be NULL) receive gscale * gradient.  Nearest neighbour: smallest index among equal distances.  No float atomics on the gradients, and the
 * pairs' shares of the term are added in pair order (stream-ordered scratch of P doubles, hipMallocAsync): the same bits on every run, in all three forms.
 * ------------------------------------------------------------------------------------------------- */
int vt_chamfer_ragged(const float *x, const int *offx, const float *y, const int *offy, int P, float gscale,
                      double *term, float *dx, float *dy, void *stream);
/* The same term and gradients with every pair split over several workgroups (one workgroup per pair makes the largest contact sets the launch's critical
 * path): total_x / total_y = offx[P] / offy[P] (rows of x / y), ws = vt_chamfer_ws_bytes(total_x, total_y, P) bytes of device scratch.  Gradients are still
 * accumulated without float atomics (run-to-run reproducible); the far-side sums associate differently from vt_chamfer_ragged (last-bit differences). */
long vt_chamfer_ws_bytes(long total_x, long total_y, int P);
int vt_chamfer_ragged_ws(const float *x, const int *offx, long total_x, const float *y, const int *offy, long total_y, int P, float gscale,
                         double *term, float *dx, float *dy, void *ws, void *stream);

/* The same with the y clouds taken THROUGH AN INDEX LIST out of one big array (the contact term of phase 'joint', recon_fit_trivis_full.py:393-457: the
 * object-side contact points are rows idx_y[r] of the transformed surface samples (B * N, 3) of the batch): y row r = y_base[idx_y[r]], and the gradient of
 * row r is ADDED to dy_base[idx_y[r]] -- the additions of "index_select, vt_chamfer_ragged_ws on the compact list, index_add_" in their order (bit-identical
 * results), without the three gather / zero / scatter launches around it.  idx_y must not repeat a row (a surface point belongs to one (frame, part) pair).
 * run_plan = 0 reuses the work-item plan a previous call left in ws for the SAME offx / offy (the contact set is computed once per batch). */
int vt_chamfer_ragged_idx(const float *x, const int *offx, long total_x, const float *y_base, const int *idx_y, const int *offy, long total_y, int P,
                          float gscale, double *term, float *dy_base, void *ws, int run_plan, void *stream);

/* Evaluation Chamfer, one direction (recon/eval/chamfer_distance.py:10-52, sklearn NearestNeighbors(k=1, metric='l2')): for each of
 * the nq points of cloud pair p the Euclidean distance to the nearest of the ns points of `search`; query (P,nq,3), search (P,ns,3),
 * dist (P,nq).  The bidirectional Chamfer of the reference is mean(dist(x->y)) + mean(dist(y->x)). */
int vt_nn_distance(const float *query, int nq, const float *search, int ns, int P, float *dist, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * Silhouette.  Replaces neural_renderer.Renderer(K, R=I, t=0, orig_size=1, anti_aliasing=False)(verts, faces,
 * mode='silhouettes') and its backward as used by SilLossROI.forward (recon/obj_pose_roi.py:77-94,183-207).
 * verts (B,NV,3) camera space, faces (NF,3) int32 shared, K (B,9), image (B,size,size) row 0 = top.
 * face_index (B,size,size) int32 (face id in [0,2*NF) of the doubled fill_back list, -1 = background) and the workspace
 * `ws` (vt_sil_workspace_floats(B,NV,NF,size) floats: depth keys, sweep masks, projected vertices, face corners, pixel boxes,
 * visibility flags) are
 * written by the forward and read again by the backward.
 * ------------------------------------------------------------------------------------------------- */
long vt_sil_workspace_floats(int B, int NV, int NF, int size);
int vt_sil_forward(const float *verts, int B, int NV, const int *faces, int NF, const float *K, int size,
                   float *image, int *face_index, float *ws, void *stream);
/* d_image (B,size,size) -> dverts (B,NV,3) (overwritten). eps = NMR's 1e-4. */
int vt_sil_backward(const float *verts, int B, int NV, const int *faces, int NF, const float *K, int size,
                    const int *face_index, const float *d_image, float eps, float *ws, float *dverts, void *stream);
/* SilLossROI's per-batch set-up on the device (recon/obj_pose_roi.py:39-75 __init__; :111-121 to_original_bbox; :123-155 compute_K_roi; :157-181 cvt_masks;
 * recon/bbox.py:26-48 make_bbox_square; recon/opt_utils.py:148-153 mask2bbox).  mask_h / mask_o (B,H,W) person / object masks of the network input in [0,1];
 * crop_centers (B,2) full-image pixels; expansion 0.3; out = render size (256); crop_size 1200, net_size 512; cam_norm = {fx, fy, cx, cy} / image_width (host
 * doubles).  Writes image_ref, keep_mask (B,out,out) and K (B,9) = normalised intrinsics of the square ROI; boxes_ws: 4 B doubles of scratch.  An empty
 * object mask gives the reference's degenerate box and all-zero crops (image_ref = 0, keep_mask = 1).  The ROIAlign underneath (detectron2
 * BitMasks.crop_and_resize: aligned, adaptive sampling ratio, >= 0.5) is third-party: PARITY UNPINNED beyond the restatement in silhouette.py. */
int vt_sil_setup(const float *mask_h, const float *mask_o, int B, int H, int W, const float *crop_centers, double expansion, int out, double crop_size,
                 double net_size, const double *cam_norm, double image_width, float *image_ref, float *keep_mask, float *K, double *boxes_ws, void *stream);

/* fused occlusion-aware mask term (obj_pose_roi.py:191-198; recon_fit_trivis_full.py:164-168):
 * per[b] = sum_px (keep*sil - ref)^2 ; *term += mean_b(per[b]*occ[b]); d_image = gscale * d/d sil */
int vt_sil_mask_loss(const float *image, const float *keep, const float *ref, const float *occ, int B, int size,
                     float gscale, double *term, float *per_frame, float *d_image, void *stream);

/* The silhouette term of ONE Adam step of phase 'sil' (recon_fit_trivis_full.py:164-168, 329-375; SilLossROI.forward, obj_pose_roi.py:183-207, and its backward):
 * vt_sil_forward + vt_sil_mask_loss + vt_sil_backward as 5 launches instead of 10 -- the same arithmetic, operation for operation (owner map, d_image, vertex
 * gradients bit-identical; *term += mean_b(sum_px (keep sil - ref)^2 occ[b]) accumulated in 2^-34 fixed point, frame order).  face_index, d_image: (B,size,size)
 * outputs; dverts (B,NV,3); ws: vt_sil_workspace_floats(B,NV,NF,size) floats. */
int vt_sil_step(const float *verts, int B, int NV, const int *faces, int NF, const float *K, int size, const float *keep, const float *ref,
                const float *occ, float gscale, float eps, double *term, int *face_index, float *d_image, float *ws, float *dverts, void *stream);

/* Triplane masks of the SMPL mesh.  Replaces TriplaneNrRenderer.render_3views
 * (render/render_triplane_nr.py:86-139): the mesh centred on `center` (B,3) (the SMPL centre, body25 joint 8) is rendered
 * orthographically from the right (x' = z, y' = -y, depth -x + 10), the back (-x, -y, -z + 10) and the top (x, z, y + 10);
 * mask = a face covers the pixel with 0.1 < depth < 100.  masks (B,3,size,size) in {0,1}, row 0 = top; face_index (B,3,size,size)
 * int32 scratch output (front face id or -1); ws >= vt_sil_workspace_floats(3 B, NV, NF, size) floats.  PARITY UNPINNED for the
 * rasterisation rule (neural_renderer, see vt_sil_forward); the view transforms are pinned (tests/golden/triplane_views.npz). */
int vt_triplane_render(const float *verts, const float *center, int B, int NV, const int *faces, int NF, int size,
                       float *masks, int *face_index, float *ws, void *stream);

/* Hourglass up-path of the image encoder: out = skip + bicubic x2 upsampling of low, NHWC fp32.  Replaces
 * `up1 + F.interpolate(low3, scale_factor=2, mode='bicubic', align_corners=True)` (model/HGFilters.py:45-47): cubic convolution with
 * A = -0.75, source coordinate dst * (h-1)/(2h-1), taps clamped to the border.  low (B,h,w,C), skip (B,2h,2w,C) or NULL, out (B,2h,2w,C);
 * C must be a multiple of 4.  (The convolutions and group norms of the encoder run on MIOpen through PyTorch.) */
int vt_upsample2x_bicubic_add(const float *low, const float *skip, int B, int h, int w, int C, float *out, void *stream);
/* the same arithmetic + the GroupNorm partial sums of the output (vt_sweep_blocks(4 h w) blocks, see vt_avgpool2x2_stats) */
int vt_upsample2x_bicubic_add_stats(const float *low, const float *skip, int B, int h, int w, int C, float *out, double *stats_ws, int stats_groups,
                                    void *stream);

/* GroupNorm (+ ReLU) of an NHWC fp32 tensor, the `bnK -> F.relu` prologue of every pre-activated convolution of the encoder
 * (model/net_util.py:374-388, model/HGFilters.py:176,192-193): y = [relu]((x - mean_g) / sqrt(var_g + eps) * gamma + beta) with the
 * biased variance over (H, W, C/groups), exactly torch.nn.functional.group_norm.  x, y (B,HW,C); gamma, beta (C); ws >= vt_groupnorm_workspace_doubles(B, HW, C, groups) doubles
 * ((B, groups) float pairs {mean, rstd} first, then per-block fp64 partial sums: no atomics, deterministic). */
long vt_groupnorm_workspace_doubles(int B, int HW, int C, int groups);
int vt_groupnorm_nhwc(const float *x, const float *gamma, const float *beta, int B, int HW, int C, int groups, float eps,
                      int relu, double *ws, float *y, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * Adam.  Replaces torch.optim.Adam(...).step() (defaults betas=(.9,.999), eps=1e-8) on one parameter tensor.
 * `stop_flag` (device int, may be NULL): when *stop_flag != 0 the update is skipped (device-side early stop).
 * ------------------------------------------------------------------------------------------------- */
int vt_adam_step(float *p, const float *g, float *m, float *v, long n, int step, float lr, float beta1, float beta2,
                 float eps, const int *stop_flag, void *stream);

/* the same update on the first `cols` columns of row-strided p/g (m, v are (rows, cols) contiguous): lets one pose
 * tensor (B,156) be optimised on its [0:66) slice, i.e. global_pose + body_pose of SMPLPyTorchWrapperBatchSplitParams */
int vt_adam_step_2d(float *p, long p_stride, const float *g, long g_stride, float *m, float *v, int rows, int cols,
                    int step, float lr, float beta1, float beta2, float eps, const int *stop_flag, void *stream);

/* Early-stop rule of the fit loops evaluated on the device (recon_fit_behave.py:447-455,
 * recon_fit_trivis_full.py:372-373, fit_SMPLH_kpts.py:161):
 *   loss = sum_k w[k]*terms[k];  if (armed && |prev-loss|/prev < prev*tol) *stop_flag = 1;  prev = loss;
 * terms (nterms) device, w (host, nterms), state (device, 2 floats: prev_loss, last_loss), history (device) or NULL
 * receives loss at index `slot`. */
int vt_loss_reduce_and_stop(const double *terms, const float *w, int nterms, float tol, int armed, float *state,
                            int *stop_flag, float *history, int slot, void *stream);

/* small utilities */
int vt_fill(float *p, long n, float value, void *stream);

/* Device-side early stop.  The fits evaluate their stop rules on the device (the reference breaks out of its inner loop on the host:
 * recon_fit_behave.py:447, recon_fit_trivis_full.py:372, fit_SMPLH_kpts.py:161) and the host reads the flag once per outer iteration of 10 steps; with
 * `flag` registered for `stream` the query and SMPL-H launches queued behind the stopping step return at once when *flag != 0 (the Adam / loss-history
 * launches ignore those steps already).  flag = NULL removes the registration; the owner must remove it before the flag's memory is released.
 * The registration belongs to the CALLING HOST THREAD: only launches issued by that thread on `stream` see the flag (two fits driven by two threads
 * through one stream do not interfere); registering a second, different flag for the same stream from the same thread is refused with VT_ERR_BUSY. */
int vt_stream_set_skip_flag(void *stream, const int *flag);

/* ---- bookkeeping of one round of the surface-point generator (recon/gen/generator.py:149-212, Generator.gen_pc_batch) ----------------------------------
 * vt_gen_round_compact: surface (B,S,3) projected samples, df_target (B,S) clamped distance of the last query, pre (B,S,3) positions of that query (or NULL),
 *   active (B) bytes.  A sample is kept when df_target < filter_val and z > zmin and its frame is active (generator.py:160-166).  order (B,S) int32 receives the
 *   kept sample indices in sample order (first cnt[b] entries: torch.argsort(~mask, stable=True)'s prefix); kept_pre (B,S,3) (or NULL) the positions `pre` at
 *   them; with write != 0 the kept points are appended to buf_points (B,cap+1,3) at row fill[b] (rows >= cap dropped: the reference cuts every frame to the common
 *   count anyway); cnt (B), fill_out (B) = min(fill + cnt, cap) (= fill without write) as int64.
 * vt_gen_scatter_heads: pred (B,C,kmax) predictions at the kept points -> buf (B,cap+1,C) rows fill_old[b] + k, k < cnt[b].
 * vt_gen_resample: the next round's M samples per frame (generator.py:190-210): samples[order[floor(u * cnt)]] + near_scale * pert where cnt > 1, else a
 *   restart init[floor(u * S0)] + 0.5 * pert; u (B,M) uniform, pert (B,M,3) normal (drawn by the caller's seeded generator). */
int vt_gen_round_compact(const float *surface, const float *df_target, const float *pre, const unsigned char *active, int B, int S, float filter_val,
                         float zmin, const long long *fill, int cap, int write, float *buf_points, int *order, float *kept_pre, long long *cnt,
                         long long *fill_out, void *stream);
int vt_gen_scatter_heads(const float *pred, int B, int C, int kmax, const long long *fill_old, const long long *cnt, int cap, float *buf, void *stream);
int vt_gen_resample(const float *samples, const int *order, const long long *cnt, const float *init, int B, int S, int S0, const float *u,
                    const float *pert, int M, float near_scale, float *out, void *stream);

/* ---- shaded rendering of the fitted meshes (demo.sh step 7: render/render_side_comp.py:71-98 RendererSide2side.render_recon ->
 * render/nr_utils.py:681-702 NrWrapper.render / render_meshes -> neural_renderer.Renderer.render, RGB mode) ---------------------------------------------
 * PARITY UNPINNED: neural_renderer is third-party; the rule (restated in render.hip's header, held to an independent float64 renderer in
 * tests/test_gpu_render.py): fill_back doubling (reversed copy [i2,i1,i0], same colour; doubled id f / F + f of an F-face scene), per-face lighting on the
 * camera-space vertices n = normalize(cross(v0 - v1, v2 - v1), eps 1e-5), light = I_amb c_amb + I_dir c_dir relu(n . d), colour = face colour * light;
 * projection x/(z+1e-9), y/(z+1e-9), K, v = orig_size - v, 2 (. - orig_size/2) / orig_size; vt_sil_forward's coverage rule (pixel centres, front faces,
 * perspective-correct depth, 0.1 < z < 100, nearest face, ties to the smaller doubled id, row 0 = top); uncovered pixels = background, alpha 0, depth 100;
 * anti_aliasing draws at 2 size and averages rgb, alpha and depth over 2 x 2 blocks.
 *
 * vt_render_rgb: verts (B,NV,3) camera coordinates, faces (NF,3) int32 and face_colors (NF,3) shared by the B views, K (B,9) (k_per_view != 0) or (9) shared,
 *   orig_size (nr_utils.py:568-570: w * ratio); light = host {I_amb, I_dir, c_amb[3], c_dir[3], direction[3]} (11 floats; nr_utils.py:572-575:
 *   0.4, 0.3, 1 1 1, 1 1 1, 1 0.5 1), background = host rgb[3].  static_layer: NULL, or a layer from vt_render_static_create built for the same K, orig_size,
 *   light, size and anti_aliasing; the views then show the concatenated scene [mesh faces, layer faces] (nr_utils.py:801-808 add_checker), with doubled ids
 *   numbered in that scene.  Outputs: rgb (B,size,size,3), alpha (B,size,size), depth (B,size,size) or NULL, face_index (B,is,is) int32 or NULL (owner's
 *   doubled id, -1 = background; is = 2 size with anti-aliasing: the owners of the full-resolution raster).  ws: ws_bytes >= vt_render_workspace_bytes(B, NF,
 *   size, anti_aliasing, L) bytes, where L is the batch's tile-list length.  The call synchronises `stream` once (after binning) to read L: it is written
 *   to *list_entries (host, or NULL), and a workspace too small for it returns VT_ERR_ARG before anything is rasterised (grow it to L and call again).
 * vt_render_static_create: a scene part shared by every view (render_recon.py:58-62, the xz ground checkerboard, already in camera coordinates: verts (NV,3),
 *   faces (NS,3), face_colors (NS,3), K (9)), set up, binned and resolved once; owns its lit face records and a per-pixel depth / owner map (device memory,
 *   allocated here; the temporary binning workspace is freed before it returns).  Synchronises `stream`.
 * vt_render_panel_u8: (clip(rgb, 0, 1) * 255).astype(uint8) -- truncation -- of rows [row0, row0 + nrows) x columns [col0, col0 + ncols) of each (B,size,size,3)
 *   view (render_side_comp.py:94, [:int(0.75 * 1200), 240:960]), written to out + view_off[b] (device int64 byte offsets) with out_row_stride bytes per row:
 *   panels go straight into their place of the frame strip (render_recon.py:155-158). */
long vt_render_workspace_bytes(int B, int NF, int size, int anti_aliasing, long list_entries);
int vt_render_static_create(void **layer, const float *verts, int NV, const int *faces, int NS, const float *face_colors, const float *K, float orig_size,
                            const float *light, int size, int anti_aliasing, void *stream);
void vt_render_static_destroy(void *layer);
int vt_render_rgb(const float *verts, int B, int NV, const int *faces, int NF, const float *face_colors, const float *K, int k_per_view, float orig_size,
                  const float *light, const float *background, const void *static_layer, int size, int anti_aliasing, float *rgb, float *alpha, float *depth,
                  int *face_index, void *ws, long ws_bytes, long *list_entries, void *stream);
int vt_render_panel_u8(const float *rgb, int B, int size, int row0, int nrows, int col0, int ncols, unsigned char *out, const long long *view_off,
                       long long out_row_stride, void *stream);
/* vt_render_rgb_pv: vt_render_rgb with face_colors (B,NF,3), one table per view, when colors_per_view != 0 (render/nr_utils.py:527-535: with
 *   contact_viz_type 'face' the object's colours depend on the frame); with colors_per_view == 0 it IS vt_render_rgb, which forwards here. */
int vt_render_rgb_pv(const float *verts, int B, int NV, const int *faces, int NF, const float *face_colors, int colors_per_view, const float *K, int k_per_view,
                     float orig_size, const float *light, const float *background, const void *static_layer, int size, int anti_aliasing, float *rgb,
                     float *alpha, float *depth, int *face_index, void *ws, long ws_bytes, long *list_entries, void *stream);

/* ---- contacts between body and object (demo.sh step 7 with viz_contact: render/nr_utils.py:380-404 ContactVisualizer.get_contact_spheres, :100-122
 * color_contact_faces / color_contact_faces_all, :504-535 NrWrapper.prepare_render) ------------------------------------------------------------------------
 * The reference queries a scipy cKDTree of the SMPL vertices with the object's vertices, per frame, on the host; here: brute force on the device, B frames a
 * call, no float atomics, results bit-identical from run to run and independent of B and of a frame's place in the batch (contact.hip's header).
 * PARITY UNPINNED: psbody.mesh.sphere.Sphere.to_mesh is not installed; the sphere tessellation is this project's icosphere (visualize.icosphere).
 *
 * vt_contact_regions: smpl_verts (B,NVs,3), labels (NVs) int32 in [0,P) (P <= 32; nr_utils.py:367-372), obj_verts (B,NVo,3), thres (nr_utils.py:384, 0.04 in
 *   NrWrapper) -> nn_idx (B,NVo) int32 nearest SMPL vertex on the squared fp32 distance, exact ties to the smaller index; nn_dist (B,NVo) its sqrtf; part (B,NVo)
 *   int32 labels[nn_idx] where nn_dist < thres, else -1; count (B,P) int32; centre (B,P,3) mean of the object vertices of the part (nr_utils.py:398-399),
 *   accumulated in fp64 in a fixed order and rounded once, 0 where count == 0.
 * vt_contact_spheres: unit_verts (NSV,3) sphere template -> out (B, P NSV, 3): centre + radius * unit per (frame, part) (nr_utils.py:400), every vertex at the
 *   centre (0) where count == 0: such faces have three identical corners and are culled by vt_render_rgb's set-up (zero area) before binning.
 * vt_contact_face_colors: out (B,NF,3) = base_colors (NF,3), except faces face_off + g, g < NFo, of the object (obj_faces (NFo,3) int32 into its NVo vertices) with
 *   a corner in contact: palette[highest part among the corners] (nr_utils.py:114-122: parts in ascending order, each overwriting).  Feeds vt_render_rgb_pv. */
int vt_contact_regions(const float *smpl_verts, const int *labels, const float *obj_verts, int B, int NVs, int NVo, int P, float thres, int *nn_idx,
                       float *nn_dist, int *part, int *count, float *centre, void *stream);
int vt_contact_spheres(const float *centre, const int *count, int B, int P, const float *unit_verts, int NSV, float radius, float *out, void *stream);
int vt_contact_face_colors(const int *part, int B, int NVo, const int *obj_faces, int NFo, int face_off, const float *base_colors, int NF, const float *palette,
                           int P, float *out, void *stream);

/* ---- Motion-JPEG video of demo step 7 (render/render_side_comp.py:71-72 drives render/render_recon.py, which appends every frame to an imageio FFMPEG
 * writer: render_recon.py:113-115 imageio.get_writer(..., format='FFMPEG', fps), :169 and :188 writer.append_data(frame)) --------------------------------
 * Baseline sequential JPEG of uint8 RGB frames already in device memory; the contract (JFIF BT.601 colour in fp32, 4:2:0 = mean of 2 x 2 or 4:4:4,
 * orthonormal fp32 DCT, IJG quality tables, Annex K Huffman tables, restart interval of one MCU row) is written in jpeg.hip's header and restated in float64 by
 * tests/jpeg_model.py.  vistracker_amd/video.py builds the per-size header (SOI .. SOS) and the AVI file.
 *
 * vt_jpeg_workspace_bytes: device workspace bytes of a call on n frames of H x W (subsampling 420 or 444), -1 on bad sizes; *max_out_bytes (host, or NULL)
 *   receives the worst case of the call's output (1660 bits per block before stuffing, stuffing doubling, two marker bytes per MCU row).
 * vt_jpeg_encode: frame f at rgb + f * frame_stride (bytes), rows row_stride bytes apart (>= 3 W), pixels packed: a (n,H,W,3) tensor or a strided view of one
 *   with packed pixels.  quality 1..100.  Writes, per frame, the entropy-coded data that follows SOS (segments separated by RSTm markers, EOI at the end)
 *   into the HOST buffer out, frames back to back: frame f is out[offsets[f], offsets[f + 1]) (offsets: host, n + 1 entries).  out_cap must hold the worst
 *   case (*max_out_bytes) and ws_bytes the workspace: both are checked before anything is launched (VT_ERR_ARG, the needed size in the message).  The call
 *   synchronises `stream`: once to read the n + 1 offsets, once after the one device-to-host copy of exactly the used bytes. */
long vt_jpeg_workspace_bytes(int n, int H, int W, int subsampling, long long *max_out_bytes);
int vt_jpeg_encode(const unsigned char *rgb, int n, int H, int W, long long frame_stride, long long row_stride, int quality, int subsampling, void *ws,
                   long ws_bytes, unsigned char *out, long long out_cap, long long *offsets, void *stream);

/* ---- SIF-Net input crops from decoded frames (data/train_data.py:143-162 prepare_image_crop; vistracker_amd/sequence_io.py prepare_crops) -------------------
 * uint8 frames in device memory in, channels 0..4 of the (B,8,S,S) fp32 network tensor out; the arithmetic contract is written in inputs.hip's header and
 * restated with integers in tests/inputs_model.py.  Both calls reproduce the host path (sequence_io.masks2bbox, crop, resize_bilinear, the compose of
 * SequenceLoader.load_crop) bit for bit; integer atomics only, results independent of scheduling, of B and of a frame's place in the batch.
 *
 * vt_mask_bbox (data/base_data.py:139-157 masks2bbox): pm, om (B,H,W) uint8; a pixel counts when (uint8)(pm + om) > thres, the sum wrapping in uint8 as the
 *   reference's accumulator does.  box (B,4) int32 = xmin, ymin, xmax, ymax, inclusive; (W, H, -1, -1) for a frame without such a pixel (the caller maps it
 *   to EMPTY_BBOX).  H * W <= 2^30, B <= 65535.
 * vt_crop_resize_compose (data/train_data.py:143-162, data/base_data.py:204-233 crop, :252-265 compose_images): rgb (B,H,W,3), pm, om (B,H,W) uint8;
 *   corners (B,4) int32 on the device = tl.x, tl.y, br.x, br.y of each frame's crop, rounded on the host as crop() rounds them (each extent br - tl is
 *   crop_size, or crop_size +- 1 for an odd crop_size: numpy rounds halves to even); a frame whose extents are not within 1 of crop_size, or with a corner beyond
 *   +-2^29, is written as zeros and reads nothing (crop_size < 2^28).  Only image pixels x in [max(0, tl.x), min(W - 1, br.x)) (likewise y) are read, the rest of the crop is 0.  Bilinear resize of the crop to
 *   out_size x out_size with half-pixel centres in fp32, q = clip(floor(x + 0.5), 0, 255), value = table[q] with table = 256 device floats
 *   float32(q / 255.0); rgb channels are zeroed where neither resized mask reaches 128.  Frame b is written at out + b * frame_stride floats
 *   (frame_stride >= 5 out_size^2; 8 out_size^2 for the network tensor), channels 0..4 only.
 * vt_resize_panel_u8 (render/render_recon.py:157-159: the camera image resized to the frame's height, the left panel of every step-7 frame): n decoded uint8 RGB
 *   images behind src (device, src_bytes bytes), frame k described by six HOST integers frames[6 k ..] = byte offset into src, full height h, full width w, first
 *   staged column x0, staged width sw, row stride in bytes: only columns [x0, x0 + sw) of the image are there, 3 sw packed bytes per row.  Frames of different
 *   sizes share a call.  Writes, for frame k, rows [0, H) x panel columns [0, pw) = columns [col0, col0 + pw) of the bilinear H x size resize (half-pixel centres,
 *   fp32, q = clip(floor(v + 0.5), 0, 255): inputs.hip's header; sequence_io.resize_bilinear_hw(img, H, size)[:, col0:col0 + pw]) at out + out_off[k] (DEVICE int64
 *   byte offsets, as vt_render_panel_u8 takes them) with out_row_stride bytes per row; no other byte of out is touched and no full-size image exists.  VT_ERR_ARG,
 *   before anything is launched, for null pointers, non-positive sizes, rows that leave [0, src_bytes) and staged columns that do not hold every tap of the
 *   panel's columns. */
int vt_mask_bbox(const unsigned char *pm, const unsigned char *om, int B, int H, int W, int thres, int *box, void *stream);
int vt_crop_resize_compose(const unsigned char *rgb, const unsigned char *pm, const unsigned char *om, int B, int H, int W, const int *corners, int crop_size,
                           int out_size, const float *table, float *out, long long frame_stride, void *stream);
int vt_resize_panel_u8(const unsigned char *src, long long src_bytes, const long long *frames, int n, int H, int size, int col0, int pw, unsigned char *out,
                       const long long *out_off, long long out_row_stride, void *stream);

/* ---- the fit on the camera image and its score on the masks (demo step 7; overlay.hip's header holds both contracts, tests/overlay_model.py restates them) -----
 * The reference declares -am / --add_mask (render/render_recon.py:346) and never reads it; it has no ground-truth-free score.  Both rules are this project's.
 *
 * vt_overlay_panel_u8: rgb (B,S,S,3), alpha (B,S,S) of a vt_render_rgb call without a static layer and with background (0,0,0) (rgb premultiplied by coverage);
 *   crop rows [row0, row0 + nrows) x columns [col0, col0 + ncols) as in vt_render_panel_u8.  View b reads the uint8 panel at out + src_off[b] and writes the panel
 *   at out + dst_off[b] (DEVICE int64 byte offsets, rows out_row_stride bytes apart; src_off[b] == dst_off[b] is allowed, no other overlap is).  Per pixel and
 *   channel c in fp32, in this order: a = opacity * alpha, v = (255 * opacity) * min(max(rgb_c, 0), 1) + (1 - a) * p, q = clip(floor(v + 0.5), 0, 255) with p the
 *   source byte: q == p bit for bit where alpha == 0 and rgb == 0, and for opacity == 0.  No byte outside the destination panels is written.  VT_ERR_ARG before
 *   any launch for null pointers, non-positive sizes, a crop outside [0, S), out_row_stride < 3 ncols, opacity outside [0, 1].
 * vt_mask_score: fidx (B,is,is) int32 = face_index of a vt_render_rgb call without a static layer over F faces: doubled id d -> face d < F ? d : d - F, -1 and
 *   ids >= 2 F -> none; faces < nf_body are body, faces < nf_body + nf_obj object, later ones (contact spheres) neither.  Masks: uint8 behind pm (person) and om
 *   (object; may be the same buffer), view b described by eight HOST integers frames[8 b ..] = byte offset of its person mask in pm, of its object mask in om, h,
 *   w, pixel stride and row stride of the person mask, pixel stride and row stride of the object mask (pixel stride C reads channel 0 of an (h,w,C) mask); all
 *   checked against pm_bytes / om_bytes before anything is launched.  A pixel is on when its value > thres.  Raster sample (yi, xi), yi < rows, xi < is, reads
 *   mask pixel sy = ((2 yi + 1) h) / (2 rows), sx = ((2 xi + 1) w) / (2 is) (integer division: nearest neighbour at half-pixel centres).  count (B,2,4) int32,
 *   zeroed by the call on the stream; class 0 = body against pm, class 1 = object against om: [0] owner is the class and the mask is on, [1] owner is the class,
 *   [2] the mask is on, [3] the mask is on and the owner is the other class.  Integer arithmetic and integer atomics only (at most 8 per workgroup, at most 64
 *   workgroups per view): bit-identical from run to run, independent of B and of a view's place in the batch. */
int vt_overlay_panel_u8(const float *rgb, const float *alpha, int B, int size, int row0, int nrows, int col0, int ncols, unsigned char *out,
                        const long long *src_off, const long long *dst_off, long long out_row_stride, float opacity, void *stream);
int vt_mask_score(const int *fidx, int B, int is, int rows, int F, int nf_body, int nf_obj, const unsigned char *pm, long long pm_bytes, const unsigned char *om,
                  long long om_bytes, const long long *frames, int thres, int *count, void *stream);

/* ---- labels of SIF-Net's training samples: exact point-to-mesh distance and nearest vertex (preprocess/boundary_sampler.py:75-100 compute_labels:
 * igl.signed_distance -> |distance| and closest surface point per mesh, trimesh.proximity.ProximityQuery.vertex -> nearest SMPL vertex) ---------------------
 * PARITY UNPINNED, RESTATED FROM THE GEOMETRIC DEFINITION: igl, trimesh and psbody are not installed, so nothing is recorded from them; the pin is the float64
 * brute force of tests/pmdist_model.py.  The arithmetic contract (closest point of a triangle by Voronoi region in fp32, the triangles as near as the minimum
 * within fp32 rounding re-evaluated in fp64 to decide the winner, zero-area triangles as their longest edge, bounding-sphere culling that changes no result) is
 * written in pmdist.hip's header, with the coordinate range the fp64 decision is guaranteed for (corners not much farther out than ~10 |p|_1).  INPUTS ARE FINITE BY CONTRACT: a NaN or infinite coordinate gives
 * unspecified (but in-bounds) results.  Results do not depend on B or on a frame's place in the batch; no float atomics.
 *
 * vt_point_mesh_distance (boundary_sampler.py:75-100): points (B,N,3), verts (B,NV,3) one mesh pose per frame, faces (NF,3) int32 shared by the frames, every
 *   index in [0,NV) (indices outside are clamped into it, for memory safety only) -> dist (B,N) unsigned distance = |p - closest| of the fp32 point written
 *   to closest (B,N,3; may be NULL); face_id (B,N; may be NULL) int32 = the smallest index among the faces attaining the (fp64-arbitrated) minimum.  workspace:
 *   vt_point_mesh_workspace_bytes(B, NF) bytes (-1 on bad sizes), 16-byte aligned, overwritten by every call.  B <= 65535.
 * vt_point_mesh_distance_ex: the same with flags (bit 0: culling off, every triangle is evaluated; results are bit-identical either way) and n_tests (one
 *   device-side 64-bit word, or NULL): the call ADDS the number of point-triangle evaluations it executed (the caller zeroes it).  Measurement and tests.
 * vt_nearest_vertex (boundary_sampler.py:87,97 ProximityQuery.vertex): vert_id (B,N) int32 = argmin_j |p - v_j|^2 on the squared fp32 distance
 *   ((dx dx + dy dy) + dz dz), exact ties to the smaller index; vert_dist (B,N; may be NULL) its sqrtf. */
long vt_point_mesh_workspace_bytes(int B, int n_faces);
int vt_point_mesh_distance(const float *points, int n_points, const float *verts, int n_verts, const int *faces, int n_faces, int B, float *dist, float *closest,
                           int *face_id, void *workspace, void *stream);
int vt_point_mesh_distance_ex(const float *points, int n_points, const float *verts, int n_verts, const int *faces, int n_faces, int B, float *dist,
                              float *closest, int *face_id, void *workspace, int flags, unsigned long long *n_tests, void *stream);
int vt_nearest_vertex(const float *points, int n_points, const float *verts, int n_verts, int B, int *vert_id, float *vert_dist, void *stream);

/* ---- SIF-Net's training objective at labelled points (model/chore_tri_vis.py:52-99 CHORETriplaneVisibility.get_errors, model/chore.py:312-325 get_df_loss;
 * called by every training step and validation pass: trainer/trainer.py:108-150,321-346).  losshead.hip's header holds the arithmetic contract, the float64
 * model tests/losshead_model.py restates it, tests/golden/losshead.npz records the reference's own values and autograd gradients.
 *
 * vt_sifnet_loss_head: predictions of S >= 1 stacks in the reference layout with a leading stack axis: df (S,B,2,N), pca (S,B,9,N), parts (S,B,14,N), centers
 *   (S,B,3,N), vis (S,B,1,N).  Labels: df_h, df_o (B,N); parts_gt (B,N) int32 (a value outside [0,14) is clamped, for definedness only); pca_gt, obj_center,
 *   visibility per point ((B,9,N), (B,3,N), (B,N); per_frame = 0) or per frame ((B,9), (B,3), (B); per_frame = 1), with identical bits.  weights: six HOST doubles
 *   in the order of loss_weights (dfh, dfo, parts, pca, obj_center, vis); vis_loss 0 = l1, 1 = l2.  terms: six device doubles, the entries of the reference's
 *   losses_all in ITS slot order (df_h, df_o, parts, pca, vis, obj_center), averaged over the stacks and UNWEIGHTED; error = terms[0] w0 + terms[1] w1 + terms[2] w2
 *   + terms[3] w3 + terms[4] w5 + terms[5] w4.  d_df .. d_vis: gradients of gscale * error in the layouts of the predictions, overwritten; each may be NULL.
 *   workspace: vt_sifnet_loss_head_ws_bytes(B, N) bytes (-1 on bad sizes), 8-byte aligned.  Two launches on the stream, no atomics: the same inputs give the same
 *   bits on every call, with or without gradient pointers.  B <= 65535. */
long vt_sifnet_loss_head_ws_bytes(int B, int n_points);
int vt_sifnet_loss_head(const float *df, const float *pca, const float *parts, const float *centers, const float *vis, int S, int B, int n_points,
                        const float *df_h, const float *df_o, const int *parts_gt, const float *pca_gt, const float *obj_center, const float *visibility,
                        int per_frame, float max_dist, const double *weights, int vis_loss, float gscale, double *terms, float *d_df, float *d_pca,
                        float *d_parts, float *d_centers, float *d_vis, void *workspace, void *stream);

/* ---- training SIF-Net's five point decoders with the feature maps frozen (dectrain.hip): a forward from PLAIN device weights and the gradient of the objective
 * to every weight and bias -- what loss.backward() leaves in the decoders of the reference's train step.  dectrain.hip's header holds the arithmetic contract
 * (exact fp32 products, fp32 accumulation on the f32-input MFMA; chunk partials added in fp64 in a fixed order; no atomics), tests/dectrain_model.py restates
 * it in float64, tests/golden/dectrain.npz records the reference's own predictions and autograd gradients.
 *
 * PARAMETERS: one flat fp32 device buffer of vt_decoder_param_floats() floats.  For head h in the head order above (df 2, pca 9, parts 14, centers 3, vis 1) and
 *   layer l = 0..3 it holds W_hl (out,in) row-major (torch's Conv1d.weight[:, :, 0]) and then b_hl (out): the decoders of model/chore.py:113-126 make_decoder.
 *   The `in` axis of layer 0 is the reference's 611-channel order (model/chore_triplane.py:139-151): im_feat 256, z_feat 3, tmpx 64, tri_tmpx 3 x 32, tri_feat
 *   3 x 64.  vt_decoder_param_offset(head, layer, is_bias) is the offset (in floats) of W_hl or b_hl; -1 for a head or layer that does not exist.
 * cam: HOST, the five floats of vt_sifnet_create.  maps: as vt_query_forward (its proj, act_level and force_fp32 fields are ignored).  B <= 65535.
 *
 * vt_decoder_train_forward (model/chore_triplane.py:97-164 query, model/geometry.py:4-14 index, model/chore.py:113-126): the projection, the eight bilinear
 *   gathers (grid_sample, align_corners=True, zeros padding), z_feat and the five decoders from `params`.  Outputs as vt_query_forward (NULL skips a head);
 *   df is OUT_DIST = 5.0 where the point projects outside the image (chore_triplane.py:155-159); vis carries its sigmoid.
 * vt_decoder_weight_grads (trainer/trainer.py:97-106: the loss.backward() of train_step, decoder parameters only): d_df .. d_vis are the upstream gradients in
 *   the prediction layouts; NULL = zero, and that head's slice of dparams is then exactly zero.  d_df of an out-of-image point counts as zero.  dparams has the
 *   layout of params; overwritten when accumulate == 0, added to otherwise (S stacks of maps share one buffer).  Sums over points: fp32 on the MFMA over at most
 *   chunk_points points of one frame (0 = the default, 2048; otherwise a multiple of 64 up to 16384), the chunk partials then in fp64 in the order (frame,
 *   chunk) and rounded to fp32 once.  The same inputs give the same bits on every call.  workspace: vt_decoder_weight_grads_ws_bytes(B, N, chunk_points) bytes
 *   (-1 on bad sizes), 16-byte aligned; nothing in it needs initialising, all of it is overwritten.  Nothing is computed for points or feature maps (vt_decoder_grads below adds the maps). */
long vt_decoder_param_floats(void);
long vt_decoder_param_offset(int head, int layer, int is_bias);
int vt_decoder_train_forward(const float *params, const float *cam, const vt_maps *maps, const float *pts, const float *crop_center, const float *body_center,
                             int B, int N, float *df, float *pca, float *parts, float *centers, float *vis, void *stream);
long vt_decoder_weight_grads_ws_bytes(int B, int N, int chunk_points);
int vt_decoder_weight_grads(const float *params, const float *cam, const vt_maps *maps, const float *pts, const float *crop_center, const float *body_center,
                            int B, int N, const float *d_df, const float *d_pca, const float *d_parts, const float *d_centers, const float *d_vis,
                            float *dparams, int accumulate, int chunk_points, void *workspace, void *stream);

/* ---- the gradient to the eight feature maps, with or without the weight gradients (dectrain.hip, section 5): what loss.backward() of the reference's train step
 * (trainer/trainer.py:97-106) sends on to the encoders through the sampled maps, i.e. the backward of model/geometry.py:4-14 (grid_sample, align_corners=True,
 * zeros padding) applied to d_a0 = sum over the heads of W_h0^T delta_h1.  The map gradient is the only tensor that crosses from the decoders to the encoders.
 *
 * vt_decoder_grads takes the arguments of vt_decoder_weight_grads and, in addition, d_maps and accumulate_maps.  d_maps: eight NHWC gradient buffers in the
 *   layout of `maps` (only maps[] and res[] are read); a NULL pointer skips that map, d_maps->res must equal maps->res (VT_ERR_ARG otherwise), the whole
 *   argument may be NULL.  dparams may be NULL: then no weight gradient is computed.  Both NULL (or all eight pointers NULL with dparams NULL) is VT_ERR_ARG.
 *   With d_maps NULL the call is vt_decoder_weight_grads, bit for bit (that entry is a call of this one).
 * ARITHMETIC: d_a0 per point in exact fp32 products accumulated in fp32 on the f32-input MFMA, K = heads (0..4, live ones) x 128.  A point outside the image
 *   still sends its gradient through the four non-df heads; only its d_df counts as zero.  Texel (y,x) of (frame, map) receives w_tap . d_a0[channels of the map]
 *   from every point with an in-bounds tap on it, with the forward's own fp32 tap weights (in-bounds flags folded in, coordinates clamped to [-2, R+1]); the
 *   products and the sum are fp64, rounded to fp32 once per slab (at most 8192 points, or one chunk).  Order of addition: the four base cells (y-1,x-1), (y-1,x),
 *   (y,x-1), (y,x) in that order, ascending point index within each; across slabs slab order, which is (frame, chunk) order.  No atomics, one writer per
 *   element per launch: the same inputs give the same bits on every call.  accumulate_maps == 0: every element of every requested map is written (zeros where no
 *   tap lands); != 0: added onto what is there (S stacks share their tmpx tensors, chore_triplane.py:139-149, so their gradients add).  All five upstream
 *   gradients NULL: requested maps get exact zeros, or are left alone when accumulating.
 * workspace: vt_decoder_grads_ws_bytes(B, N, chunk_points, want_maps) bytes (-1 on bad sizes), 16-byte aligned: that of vt_decoder_weight_grads (d_a0 overwrites
 *   a_0 in the tape once the weight-gradient GEMM of the slab is enqueued) and, with want_maps != 0, per map and tape row of a slab one 64-bit sort key (padded to
 *   a power of two) and one 16-byte tap entry.  It does not depend on the maps' resolutions.  Nothing in it needs initialising. */
long vt_decoder_grads_ws_bytes(int B, int N, int chunk_points, int want_maps);
int vt_decoder_grads(const float *params, const float *cam, const vt_maps *maps, const float *pts, const float *crop_center, const float *body_center,
                     int B, int N, const float *d_df, const float *d_pca, const float *d_parts, const float *d_centers, const float *d_vis,
                     float *dparams, int accumulate, const vt_maps *d_maps, int accumulate_maps, int chunk_points, void *workspace, void *stream);

/* ---- the backward of the encoders' ConvBlock (convtrain.hip): model/net_util.py:346-396, the unit conv2 / conv3 / conv4, every b1 / b2 / b2_plus / b3 of an
 * hourglass and every top_m are built from (model/HGFilters.py:4-203).  All tensors are NHWC fp32 channel slices (pointer, channel stride, channel offset; stride
 * and offset multiples of 4, pointers 16-byte aligned), weights plain fp32 device memory in the reference's (Cout, Cin, kh, kw) layout.  H % 8 == 0, W % 16 == 0,
 * B <= 65535.  ARITHMETIC: exact fp32 products accumulated in fp32 on the f32-input MFMA, no range assumption on a gradient (scaling d_out by a power of two scales
 * every result by it, bit for bit); no atomics, one writer per element per launch, fixed summation order: the same inputs give the same bits on every call.
 * Nothing in a workspace needs initialising.  `accumulate` != 0 adds onto the PARAMETER gradients (dW, dgamma, dbeta), 0 overwrites them.
 *
 * vt_conv3x3_dgrad (net_util.py:379, 383, 387, backward to the convolution's input; nn.Conv2d 3x3 / stride 1 / pad 1, bias-free: net_util.py:213-216):
 *   d_in[b,y,x,ci] = sum (co,ky,kx) W[co,ci,ky,kx] d_out[b,y-ky+1,x-kx+1,co], zero outside the image.  Cout in {32, 64, 128}, Cin % 32 == 0, Cin <= 256.
 *   workspace: vt_conv_dgrad_workspace_bytes(cout, cin, 9) (the weights in fragment order, rewritten by every call).
 * vt_conv3x3_wgrad (the same lines, backward to the weight): dW[co,ci,ky,kx] = sum (b,y,x) d_out[b,y,x,co] a[b,y+ky-1,x+kx-1,ci] with
 *   a = max((x_in - mean) rstd gamma + beta, 0) recomputed from x_in and gn_stats (B x groups {mean, rstd} float pairs, as vt_groupnorm_finalize leaves them) with
 *   the forward's own fp32 expression while the operand is staged (net_util.py:377-378, 381-382, 385-386); gn_stats NULL: a = x_in.  Split K over pixel tiles, the
 *   partials added in fp64 in (frame, split) order and rounded once.  workspace: vt_conv_wgrad_workspace_bytes(B, H, W, cout, cin, 9).
 * vt_conv1x1_dgrad / vt_conv1x1_wgrad: the same for the ConvBlock's projection (net_util.py:364-370, 391-392), Cout in {64, 128, 256}; workspaces with taps = 1.
 * vt_gn_relu_backward (nn.GroupNorm + F.relu, net_util.py:358-362, 377-386): g = the gradient to the rectified activation, m = [xhat gamma + beta > 0] evaluated
 *   with the forward's staging expression, n = HW C / groups:  dbeta = sum g m, dgamma = sum g m xhat, s1 = sum g m gamma, s2 = sum g m gamma xhat per (frame,
 *   group), d_x = base + rstd (g m gamma - (s1 + xhat s2) / n).  base: the slice holding the other contributions to that tensor (may be d_x itself: add in place;
 *   NULL: none).  d_x, dgamma, dbeta may each be NULL.  Sums and the element formula in fp64, fixed order.  workspace: vt_gn_relu_backward_workspace_bytes.
 * vt_conv_block_backward (net_util.py:374-396 backward): dy (B,H,W,c1+c2+c3); x (B,H,W,cin) the block input; raw (B,H,W,c1+c2) = o1 | o2 as the forward's
 *   convolutions wrote them; stats1..3 the {mean, rstd} areas of bn1 (of x), bn2 (of o1), bn3 (of o2); w1..3, gamma / beta 1..3 the parameters; wproj (c1+c2+c3,
 *   cin), gamma4, beta4 the projection (bn4 shares stats1) or NULL for the identity residual (then cin == c1+c2+c3).  Outputs: d_x (B,H,W,cin), dW1..3, dgamma /
 *   dbeta 1..4, dWproj; any may be NULL to skip it.  workspace: vt_conv_block_backward_workspace(B, H, W, cin, c1, c2, c3) bytes (-1 on bad sizes). */
long vt_conv_dgrad_workspace_bytes(int cout, int cin, int taps);
long vt_conv_wgrad_workspace_bytes(int B, int H, int W, int cout, int cin, int taps);
long vt_gn_relu_backward_workspace_bytes(int B, int HW, int C, int groups);
int vt_conv3x3_dgrad(const float *weight, int cout, int cin, const float *d_out, int do_cstride, int do_coff, int B, int H, int W,
                     float *d_in, int di_cstride, int di_coff, void *workspace, void *stream);
int vt_conv1x1_dgrad(const float *weight, int cout, int cin, const float *d_out, int do_cstride, int do_coff, int B, int H, int W,
                     float *d_in, int di_cstride, int di_coff, void *workspace, void *stream);
int vt_conv3x3_wgrad(const float *d_out, int do_cstride, int do_coff, const float *x_in, int xi_cstride, int xi_coff, const float *gn_stats, const float *gamma,
                     const float *beta, int groups, int B, int H, int W, int cin, int cout, float *dW, int accumulate, void *workspace, void *stream);
int vt_conv1x1_wgrad(const float *d_out, int do_cstride, int do_coff, const float *x_in, int xi_cstride, int xi_coff, const float *gn_stats, const float *gamma,
                     const float *beta, int groups, int B, int H, int W, int cin, int cout, float *dW, int accumulate, void *workspace, void *stream);
int vt_gn_relu_backward(const float *g, int g_cstride, int g_coff, const float *x_in, int x_cstride, int x_coff, const float *gn_stats, const float *gamma,
                        const float *beta, int groups, int B, int HW, int C, const float *base, int base_cstride, int base_coff,
                        float *d_x, int dx_cstride, int dx_coff, float *dgamma, float *dbeta, int accumulate, void *workspace, void *stream);
long vt_conv_block_backward_workspace(int B, int H, int W, int cin, int c1, int c2, int c3);
int vt_conv_block_backward(const float *dy, const float *x, const float *raw, const float *stats1, const float *stats2, const float *stats3,
                           const float *w1, const float *w2, const float *w3, const float *gamma1, const float *gamma2, const float *gamma3,
                           const float *beta1, const float *beta2, const float *beta3, const float *wproj, const float *gamma4, const float *beta4,
                           int B, int H, int W, int cin, int c1, int c2, int c3,
                           float *d_x, float *dW1, float *dW2, float *dW3, float *dgamma1, float *dbeta1, float *dgamma2, float *dbeta2, float *dgamma3, float *dbeta3,
                           float *dgamma4, float *dbeta4, float *dWproj, void *workspace, int accumulate, void *stream);

/* ---- the backward of the two operators that join the ConvBlocks of an hourglass (resample_bwd.hip): model/HGFilters.py:26-50.  With them
 * vt_conv_block_backward composes into the backward of a whole HourGlass (encoder.TrainableHourglass).  Tensors are NHWC fp32, pointers 16-byte aligned,
 * C % 4 == 0.  ARITHMETIC: gathers -- one writer per element, no atomics, no workspace, nothing to initialise, a fixed order of every sum: the same inputs give
 * the same bits on every call, and scaling d_out by a power of two scales the result by it, bit for bit.
 *
 * vt_avgpool2x2_backward (F.avg_pool2d(inp, 2, stride=2), HGFilters.py:32, backward; the forward is vt_avgpool2x2_stats): d_out (B,H/2,W/2,C), d_x (B,H,W,C),
 *   d_x[b,y,x,c] = 0.25 d_out[b,y/2,x/2,c]   (exact).  H, W even.
 * vt_upsample2x_bicubic_backward (F.interpolate(low3, scale_factor=2, mode='bicubic', align_corners=True), HGFilters.py:47, backward to low3; the forward is
 *   vt_upsample2x_bicubic_add[_stats]): d_out (B,2h,2w,C), d_low (B,h,w,C),
 *   d_low[b,yy,xx,c] = sum (oy,ox) Uy[oy,yy] Ux[ox,xx] d_out[b,oy,ox,c],   Uy[oy,yy] = sum of the cubic weights (A = -0.75) of the taps i = 0..3 of output row oy
 *   with clamp(floor(sy oy) - 1 + i, 0, h - 1) == yy, sy = (h - 1) / (2h - 1) and sy oy evaluated in fp32 exactly as the forward does (a tap the border clamps
 *   onto a row several times counts every time); Ux likewise.  Sums in fp64, rounded once.  The gradient to `skip` is d_out itself (HGFilters.py:50).
 *   Any h, w > 0. */
int vt_avgpool2x2_backward(const float *d_out, int B, int H, int W, int C, float *d_x, void *stream);
int vt_upsample2x_bicubic_backward(const float *d_out, int B, int h, int w, int C, float *d_low, void *stream);

/* ---- the rest of the encoder's backward (enctrain.hip; vt_gn_relu_backward_y lives with the passes it shares in convtrain.hip): the 1 x 1 tail of a stack and
 * the stem.  With vt_conv_block_backward and the two resampling backwards they compose into the backward of a whole HGFilter (model/HGFilters.py:56-203,
 * encoder.TrainableHGFilter).  Conventions of the ConvBlock section above: NHWC fp32 channel slices, exact fp32 products, fp64 partial sums in a fixed order rounded
 * once, no atomics, one writer per element, nothing in a workspace needs initialising, `accumulate` != 0 adds onto parameter gradients, a power-of-two scale of the
 * upstream gradient scales every result bit for bit, the same inputs give the same bits on every call.
 *
 * vt_bias_grad (the bias of nn.Conv2d: conv1 at HGFilters.py:120, conv_last / l / bl / al at HGFilters.py:146-160, backward): db[c] = sum (b, pixel)
 *   d_out[b, pixel, c] over a channel slice.  Any HW > 0, C % 4 == 0, C <= 1024.  Per-block fp64 partials (256 pixels a block, at most 64 blocks a frame), finished
 *   in (frame, block) order.  workspace: vt_bias_grad_workspace_bytes(B, HW, C) (-1 on bad sizes).
 * vt_stem7x7_wgrad (conv1 = nn.Conv2d(Cin, Cout, 7, stride 2, padding 3), HGFilters.py:120, 167, backward to the weight; the forward is vt_stem7x7_forward):
 *   dW[co,ci,ky,kx] = sum (b,oy,ox) d_y[b,oy,ox,co] x[b,2oy+ky-3,2ox+kx-3,ci], zero outside the image; d_y (B, (H-1)/2+1, (W-1)/2+1, Cout) a channel slice, x the
 *   input slice of vt_stem7x7_forward (any stride and offset), dW (Cout, Cin, 7, 7).  Cout in {32, 64}, Cin in 1..8, any H, W > 0.  Split K over 16 x 16 output
 *   tiles, fp32 accumulation on the f32-input MFMA within a split, the partials added in fp64 in (frame, split) order.  No data gradient (the image needs none).
 *   workspace: vt_stem7x7_wgrad_workspace_bytes(B, H, W, cin, cout) (-1 on bad sizes).
 * vt_gn_relu_backward_y (bn1 + ReLU of the stem, HGFilters.py:125, 167, backward): vt_gn_relu_backward with the mask m = [y > 0] READ from the forward's saved
 *   rectified output y instead of recomputed -- vt_groupnorm_nhwc evaluates (x - mean) rstd gamma + beta, not the staging expression, and the two can differ in
 *   sign.  Same passes, same sums, same workspace (vt_gn_relu_backward_workspace_bytes); beta is not needed.
 * vt_stack_tail_backward (HGFilters.py:191-201 backward; forward of one stack: raw = conv_last(ll) + b, a = ReLU(bn_end(raw)), out = l(a) + b,
 *   previous' = previous + bl(a) + b + al(out) + b): d_out (B,H,W,Co) the gradient to outputs[i], d_prev (B,H,W,C) the gradient to previous'; either may be NULL =
 *   zero (not both).  ll, raw (B,H,W,C), out (B,H,W,Co) as the forward wrote them, stats the {mean, rstd} area of bn_end (of raw).  wcl (C,C), wl (Co,C), wbl (C,C),
 *   wal (C,Co); wbl, wal, out may be NULL when d_prev is (the last stack has neither bl nor al).  g_out = d_out + Wal^T d_prev; d_a = Wl^T g_out + Wbl^T d_prev
 *   (each one fp32 addition per element, operands in this order); d_raw = vt_gn_relu_backward of d_a at raw; d_ll = Wcl^T d_raw; dWal = d_prev (x) out,
 *   dWbl = d_prev (x) a, dWl = g_out (x) a, dWcl = d_raw (x) ll with a recomputed in the staging; dbal = dbbl = sum d_prev, dbl = sum g_out, dbcl = sum d_raw.
 *   Any output may be NULL to skip it.  The gradient to `previous` is d_prev itself.  C, Co in {64, 128, 256}, H % 8 == 0, W % 16 == 0.
 *   workspace: vt_stack_tail_backward_workspace(B, H, W, C, Co) bytes (-1 on bad sizes). */
long vt_bias_grad_workspace_bytes(int B, int HW, int C);
int vt_bias_grad(const float *d_out, int do_cstride, int do_coff, int B, int HW, int C, float *db, int accumulate, void *workspace, void *stream);
long vt_stem7x7_wgrad_workspace_bytes(int B, int H, int W, int cin, int cout);
int vt_stem7x7_wgrad(const float *d_y, int dy_cstride, int dy_coff, const float *x, int x_cstride, int x_coff, int B, int H, int W, int cin, int cout,
                     float *dW, int accumulate, void *workspace, void *stream);
int vt_gn_relu_backward_y(const float *g, int g_cstride, int g_coff, const float *x_in, int x_cstride, int x_coff, const float *y, int y_cstride, int y_coff,
                          const float *gn_stats, const float *gamma, int groups, int B, int HW, int C, const float *base, int base_cstride, int base_coff,
                          float *d_x, int dx_cstride, int dx_coff, float *dgamma, float *dbeta, int accumulate, void *workspace, void *stream);
long vt_stack_tail_backward_workspace(int B, int H, int W, int C, int Co);
int vt_stack_tail_backward(const float *d_out, const float *d_prev, const float *ll, const float *raw, const float *out, const float *stats,
                           const float *wcl, const float *gamma, const float *beta, const float *wl, const float *wbl, const float *wal,
                           int B, int H, int W, int C, int Co,
                           float *d_ll, float *dWcl, float *dbcl, float *dgamma, float *dbeta, float *dWl, float *dbl, float *dWbl, float *dbbl, float *dWal, float *dbal,
                           void *workspace, int accumulate, void *stream);

/* ---- packed forward weights built on the device (csrc/repack.hip) ------------------------------------------------------------------------------------------
 * Replaces, for a network that trains, the host side of vt_conv3x3_create / vt_conv1x1_create / vt_stem7x7_create (no counterpart in the reference, whose
 * nn.Conv2d reads its fp32 weight directly: model/net_util.py:213-216, HGFilters.py:120, 146-160): after an optimiser step the new weights exist only in device
 * memory, and so does max |w|, which fixes the power-of-two scale s_W of the split-f16 kinds.  Everything below reads fp32 (Cout, Cin, k, k) weights and (Cout)
 * biases IN DEVICE MEMORY and writes the packed bytes of the host functions bit for bit (hi = (f16)(w s_W), lo = (f16)(w s_W - hi), round to nearest even, f16
 * denormals kept, rows beyond Cout = 32 zero; the stem: the [Cin][7][7][Cout] transpose + the bias row, zeros without a bias).  The scale rule is the host's: NaN
 * entries do not take part in the maximum, a zero or non-finite maximum gives s_W = 1.  The split-f16 kinds also write the SCALE WORD 1 / (16 s_W) to device memory;
 * the forward kernel reads it from there when the handle has one (handles of the host functions pass it by value as before).  A packing is two launches queued on
 * `stream` (the maxima per workgroup without atomics, then the fragments): ordering on the stream protects launches that still read the old packing.
 *
 * sizes: vt_conv3x3_packed_bytes / vt_stem7x7_packed_bytes(cout, cin) = the packed bytes of a handle; vt_conv1x1_packed_bytes = of ONE of the vt_conv1x1_parts(cout)
 *   parts (2 for Cout = 256), which lie one after the other; vt_repack_workspace_bytes() = the partial maxima.  -1 for a shape the forward does not serve.
 * vt_*_pack: into caller-supplied device buffers (packed_dev 16-byte aligned; scale_dev one float; ws_dev vt_repack_workspace_bytes(); the 1 x 1 copies bias_dev to
 *   bias_out_dev when both are given).
 * vt_*_create_device: a handle for the existing forward entry points, packed from device weights: one hipMalloc, no host staging, no synchronisation.
 * vt_*_repack: overwrite such a handle's own buffers in place; the handle's address and buffers stay.  3 x 3 and 1 x 1 need a handle of *_create_device (the host
 *   handles have no scale word) and a bias exactly when the handle was created with one; the stem takes any handle.
 * vt_repack_plan_*: n handles (kinds[i] one of VT_REPACK_*, handles[i], weights[i], biases[i] or NULL) repacked by vt_repack_plan_run in two launches
 *   whatever n.  The pointers are captured at creation: the weights must stay where they are.
 * DIAGNOSTIC ONLY, not part of the training path (used by the tests and by tools/bench_scripts/repackbench.py; may change without notice):
 *   vt_repack_plan_launches: the number of launches of one vt_repack_plan_run; vt_repack_handle_snapshot: a handle's packed bytes (and scale word, host- or
 *   device-made) copied to device buffers. */
#define VT_REPACK_CONV3X3 0
#define VT_REPACK_CONV1X1 1
#define VT_REPACK_STEM7X7 2
typedef struct vt_repack_plan vt_repack_plan;
long vt_conv3x3_packed_bytes(int cout, int cin);
long vt_conv1x1_packed_bytes(int cout, int cin);
int vt_conv1x1_parts(int cout);
long vt_stem7x7_packed_bytes(int cout, int cin);
long vt_repack_workspace_bytes(void);
int vt_conv3x3_pack(const float *w_dev, int cout, int cin, void *packed_dev, float *scale_dev, void *ws_dev, void *stream);
int vt_conv1x1_pack(const float *w_dev, const float *bias_dev, int cout, int cin, void *packed_dev, float *bias_out_dev, float *scale_dev, void *ws_dev,
                    void *stream);
int vt_stem7x7_pack(const float *w_dev, const float *bias_dev, int cout, int cin, void *packed_dev, void *stream);
int vt_conv3x3_create_device(vt_conv3x3 **out, const float *w_dev, int cout, int cin, void *stream);
int vt_conv1x1_create_device(vt_conv1x1 **out, const float *w_dev, const float *bias_dev, int cout, int cin, void *stream);
int vt_stem7x7_create_device(vt_stem7x7 **out, const float *w_dev, const float *bias_dev, int cout, int cin, void *stream);
int vt_conv3x3_repack(vt_conv3x3 *h, const float *w_dev, void *stream);
int vt_conv1x1_repack(vt_conv1x1 *h, const float *w_dev, const float *bias_dev, void *stream);
int vt_stem7x7_repack(vt_stem7x7 *h, const float *w_dev, const float *bias_dev, void *stream);
int vt_repack_plan_create(vt_repack_plan **out, int n, const int *kinds, void *const *handles, const float *const *weights, const float *const *biases);
int vt_repack_plan_run(const vt_repack_plan *plan, void *stream);
void vt_repack_plan_destroy(vt_repack_plan *plan);
/* diagnostic only (see above) */
int vt_repack_plan_launches(const vt_repack_plan *plan);
int vt_repack_handle_snapshot(int kind, const void *handle, void *packed_out_dev, float *scale_out_dev, void *stream);

/* ---- data-parallel training: the rank-ordered gradient mean (csrc/gradreduce.hip) ----------------------------------------------------------------------------
 * Replaces the gradient average of torch.nn.parallel.DistributedDataParallel that the reference's Trainer.train_step relies on under "multi_gpus": true
 * (trainer/trainer.py:97-106: loss.backward() on the DDP-wrapped model all-reduces every gradient and divides by the world size before optimizer.step()).  A ring
 * all-reduce adds in an order that depends on the ring and its chunking; here the ranks' gradients are first GATHERED (a pure copy: RCCL all_gather, or the
 * caller's own copies for micro-batches) and then averaged by one kernel in a fixed order:
 *
 *   parts: W rows of `stride` >= n floats, row r = rank r's gradient.  For every i < n
 *   out[i] = (float)((((double)parts[0*stride+i] + parts[1*stride+i]) + ... + parts[(W-1)*stride+i]) / (double)W)
 *
 * added in rank order, left to right, in fp64; one fp64 division; one rounding to fp32.  `out` may be one of the rows of `parts` (in place into the local
 * gradient): an element is read from all W rows by the one thread that then writes it.  Any other overlap of `out` with the rows is an error.  No atomics, no
 * workspace: the same bits on every call and on every rank.  W = 1 returns the input bit for bit; scaling every input by a power of two scales the output bit for
 * bit short of overflow and underflow; NaN and Inf propagate as IEEE addition propagates them.  Pointers are 4-byte aligned; the body moves 16 bytes per access
 * (scalar head and tail) when stride % 4 == 0 and `out` and `parts` sit alike in their 16 bytes, as torch allocations and rows of `parts` do; scalar otherwise.
 * VT_ERR_ARG: W < 1, stride < n, a NULL pointer with n > 0.  n = 0: VT_OK, nothing launched.  `stream`: a hipStream_t. */
int vt_grad_rank_mean(const float *parts, int W, size_t n, size_t stride, float *out, void *stream);

/* ---- the gradient record and the non-finite step guard (gradstat.hip) -----------------------------------------------------------------------------------------
 * The reference's train_step runs under torch.autograd.set_detect_anomaly(True) (trainer/trainer.py:97-106): a NaN in its backward stops the run.  Here the step
 * has no host wait, so the decision is taken on the device: the gradients are measured per tensor, the step is closed by one small launch that decides whether it
 * is skipped and how far it is clipped, and the optimiser kernels take that decision as their stop flag (vt_adam_step's `stop_flag`).  After vt_grad_rank_mean
 * every rank holds the same gradient bits, so every rank takes the same decision with no collective.
 *
 * vt_grad_stats: `g` holds n floats; `seg_off` holds 2 * n_seg ascending offsets into it: segment s is [seg_off[2s], seg_off[2s+1]), and what lies between the end
 * of one segment and the start of the next (the 64-float padding of the encoders' flat buffers), before the first or after the last belongs to no segment and is
 * not read into any result.  (Begin / end pairs and not n_seg + 1 boundaries: boundaries alone cannot leave a gap out.)  Per segment:
 *   nonfinite[s] = the number of NaN or +-Inf elements
 *   sumsq[s]     = the sum of g^2 over the FINITE elements, each squared in fp64 (exact) and added in fp64: a NaN does not erase the norm of its tensor
 *   maxabs[s]    = the largest |g| over the finite elements, 0 for none
 * Denormals count with their value.  No atomics; the order of the additions is fixed by the element's index in its segment alone (chunks of VT_GRAD_STATS_CHUNK
 * elements from the segment's start, one wave each, finished in chunk order), so the bits are the same on every call, on every rank, and wherever the buffer
 * lies.  Loads are 16 bytes per lane where a chunk starts on a 16-byte boundary.  Offsets are clamped into [0, n]; a table that is not ascending gives
 * meaningless results, never a read out of bounds.  `ws`: vt_grad_stats_workspace_bytes(n, n_seg) bytes, 8-byte aligned.  Three launches.
 *
 * vt_grad_guard_close: closes a step from the results of up to three vt_grad_stats calls (a buffer that is not used: n_seg = 0).
 *   total = all sumsq added in index order, buffer after buffer, in fp64;  norm = sqrt(total)
 *   skip  = any nonfinite[] > 0, or *error (a device double, may be NULL) is NaN or +-Inf
 *   coef  = max_norm > 0 ? (float)min(1.0, max_norm / (norm + 1e-6)) : 1.f        (torch's clip_grad_norm_, evaluated in fp64 and rounded once)
 * `record` (device, 8-byte aligned, vt_grad_guard_record_bytes(n_seg_total, ring) bytes, zeroed once by the caller):
 *   long steps @0, long skipped @8 (both advanced by this call), then 1 + ring slots of VT_GUARD_SLOT_HEAD + 16 * n_seg_total bytes each: slot 0 is the last
 *   step, slot 1 + steps % ring (steps before this call) the ring's.  A slot: double norm @VT_GUARD_NORM, double error @VT_GUARD_ERROR, float coef @VT_GUARD_COEF,
 *   int skip @VT_GUARD_SKIP, long step @VT_GUARD_STEP, then double sumsq[n_seg_total], float maxabs[n_seg_total], int nonfinite[n_seg_total].
 *   record + VT_GUARD_HEAD + VT_GUARD_SKIP is the stop flag of the optimiser launches, record + VT_GUARD_HEAD + VT_GUARD_COEF the factor of vt_grad_scale.
 *
 * vt_grad_scale: g[i] *= *coef in place, one fp32 multiplication per element; nothing is written when *skip is set (NULL: never) or *coef is 1. */
#define VT_GRAD_STATS_CHUNK 4096
#define VT_GUARD_HEAD 16
#define VT_GUARD_SLOT_HEAD 32
#define VT_GUARD_NORM 0
#define VT_GUARD_ERROR 8
#define VT_GUARD_COEF 16
#define VT_GUARD_SKIP 20
#define VT_GUARD_STEP 24
long vt_grad_stats_workspace_bytes(long n, int n_seg);
int vt_grad_stats(const float *g, long n, const long *seg_off, int n_seg, double *sumsq, float *maxabs, int *nonfinite, void *ws, void *stream);
long vt_grad_guard_record_bytes(int n_seg_total, int ring);
int vt_grad_guard_close(const double *sumsq0, const float *maxabs0, const int *nonfinite0, int n_seg0,
                        const double *sumsq1, const float *maxabs1, const int *nonfinite1, int n_seg1,
                        const double *sumsq2, const float *maxabs2, const int *nonfinite2, int n_seg2,
                        const double *error, double max_norm, void *record, int ring, void *stream);
int vt_grad_scale(float *g, long n, const float *coef, const int *skip, void *stream);

/* ---- HVOP-Net training, first block (formertrain.hip): one pre-norm transformer encoder layer with a taped forward and a hand-written backward, and the final
 * LayerNorm of a TransformerV2.  fp32 row-major tensors; x, y, d_y, d_x are (B, T, D); pos (T, D); key_padding_mask (B, T) bytes, 1 = key ignored, NULL = none.
 * `params`: a HOST array of twelve device pointers in the reference's layouts and this order: self_attn.in_proj_weight (3D, D), self_attn.in_proj_bias,
 * self_attn.out_proj.weight, self_attn.out_proj.bias, linear1.weight (F, D), linear1.bias, linear2.weight (D, F), linear2.bias, norm1.weight, norm1.bias,
 * norm2.weight, norm2.bias.  activation: 0 relu, 1 gelu (exact erf), 2 leaky_relu 0.01.  Dropout p in [0, 1) with a 64-bit seed: keep-masks from
 * csrc/dropout_hash.h at the four sites named there; p = 0 hashes nothing and is the identity.
 * SHAPES: 1 <= T <= 192, D % 16 == 0 <= 160, F % 16 == 0 <= 256, D / H in {16, 32, 160}; anything else is VT_ERR_ARG and launches nothing (the size queries
 * return -1).  ARITHMETIC: exact fp32 products on v_mfma_f32_16x16x4_f32, LayerNorm statistics and backward sums in fp64, sums over the B T rows in chunks of 512
 * rows added in fp64 in chunk order; no atomics, the same bits on every call, a power-of-two scale of d_y scales every result bit for bit; with p = 0 a clip's y
 * and d_x rows do not depend on the other clips.  A clip whose keys are all masked is outside the contract (memory-safe, value undefined).  Pointers 8-byte aligned.
 *
 * vt_former_layer_forward (TransformerEncoderLayer.forward_pre, former_deci.py:77-93): y = y1 + drop2(linear2(drop(act(linear1(LN2(y1)))))),
 *   y1 = x + drop1(self_attn(LN1(x) + pos, LN1(x) + pos, LN1(x))).  tape: vt_former_layer_tape_floats floats (layout in formertrain.hip), or NULL for the
 *   inference-only forward, which needs `workspace` of 4 B T D floats instead (NULL otherwise).
 * vt_former_layer_backward (the autograd backward of the same lines): d_x and `d_params`, a HOST array of twelve device pointers in the order of `params` (or NULL);
 *   a NULL pointer skips that output, accumulate != 0 adds onto every output.  workspace: vt_former_layer_workspace_floats floats, nothing to initialise.
 * vt_layernorm_forward / vt_layernorm_backward (encoder.norm of TransformerEncoder, former_deci.py:64-65): x, y (M, D); stats (M, 2) fp64 {mean, rstd}, NULL in
 *   the forward to skip them; d_x / d_weight / d_bias may be NULL; workspace: vt_layernorm_backward_workspace_floats(M, D) floats. */
long vt_former_layer_tape_floats(int B, int T, int D, int H, int F);
long vt_former_layer_workspace_floats(int B, int T, int D, int H, int F);
int vt_former_layer_forward(const float *x, const float *pos, const unsigned char *key_padding_mask, const float *const *params, int B, int T, int D, int H,
                            int F, int activation, float p, unsigned long long seed, float *y, float *tape, float *workspace, void *stream);
int vt_former_layer_backward(const float *d_y, const float *tape, const float *x, const float *pos, const unsigned char *key_padding_mask,
                             const float *const *params, int B, int T, int D, int H, int F, int activation, float p, unsigned long long seed,
                             float *d_x, float *const *d_params, int accumulate, float *workspace, void *stream);
long vt_layernorm_backward_workspace_floats(long M, int D);
int vt_layernorm_forward(const float *x, const float *weight, const float *bias, long M, int D, float *y, double *stats, void *stream);
int vt_layernorm_backward(const float *d_y, const float *x, const double *stats, const float *weight, long M, int D, float *d_x, float *d_weight,
                          float *d_bias, int accumulate, float *workspace, void *stream);

/* ---- HVOP-Net training, third block (infillhead.hip): the ends of the network and its objective.  fp32 row-major tensors over the M = B T rows; conventions
 * and ARITHMETIC as formertrain.hip above (exact fp32 products on v_mfma_f32_16x16x4_f32 accumulated in a fixed order, sums over rows in chunks of 512 added
 * in fp64 in chunk order, no atomics, the same bits on every call, a power-of-two scale of the incoming gradient scales every result bit for bit, clips
 * independent).  An unsupported shape is VT_ERR_ARG and launches nothing; the size queries return -1.  Workspaces 8-byte aligned, nothing to initialise.
 *
 * vt_infill_proj_forward / _backward (feat_proj_smpl, feat_proj_obj of ConditionalMInfiller.forward, mfiller_cond.py:82-96, and their autograd backward): a table of
 *   nprob <= 4 problems over the same M rows in one launch: ys[i] (M, n[i]) = xs[i] (M, kin[i]) weights[i]^T + biases[i]; kin in 1 .. 160, n % 16 == 0 in
 *   16 .. 160.  xs .. ys, d_ys .. d_biases: HOST arrays of device pointers, kin / n HOST arrays.  Backward: d_weights[i] (n, kin) = d_ys[i]^T xs[i], d_biases[i] =
 *   sum over rows of d_ys[i]; a NULL array or pointer skips that output, accumulate != 0 adds onto the outputs; no d_x (the inputs are data).
 *   workspace: vt_infill_proj_workspace_floats(kin, n, nprob, M) floats.
 * vt_infill_head_forward (the predictor of mfiller_cond.py:97-104 and, with `terms`, motion_losses of trainer_infiller.py:33-47): h = f W1^T + b1,
 *   pred = leaky_relu(h, 0.01) W2^T + b2.  f (M, D), D % 16 == 0 in 16 .. 160; hidden % 16 == 0 in 16 .. 64; out_dim in 1 .. 16; T >= 3 (the reference's mean over
 *   no acceleration row is NaN).  params: HOST array {W1 (hidden, D), b1, W2 (out_dim, hidden), b2}.  h (M, hidden) may be NULL (not saved).  terms (2 fp64,
 *   device) may be NULL; else gt (M, out_dim) and a workspace of vt_infill_head_workspace_floats are needed and terms = {lw_pose mean |pred - gt|,
 *   lw_accel mean |acc(pred) - acc(gt)|}, acc(a)[t] = a[t] - 2 a[t+1] + a[t+2] inside a clip, differences and sums in fp64 (per 16-row tile, the tiles of a
 *   512-row chunk in order, the chunks in order).
 * vt_infill_head_backward (the autograd backward of the same lines): with d_pred_in == NULL the gradient of loss_pos + loss_accel times `upstream`,
 *   d_pred[t] = upstream (c_pos s[t] + c_acc (sa[t-2] - 2 sa[t-1] + sa[t])), s = sign(pred - gt), sa = sign(acc(pred) - acc(gt)), sign(0) = 0, rows outside the
 *   clip dropped, c_pos = lw_pose / (B T out_dim), c_acc = lw_accel / (B (T - 2) out_dim), evaluated in fp64 and rounded once; else the given d_pred_in (terms
 *   must then be NULL).  Then d_h = (d_pred W2) (h > 0 ? 1 : 0.01), d_f = d_h W1 and d_params, a HOST array in the order of params.  d_pred (always
 *   overwritten), d_f, d_params and each of its pointers, terms may be NULL; accumulate != 0 adds onto d_f and d_params. */
long vt_infill_proj_workspace_floats(const int *kin, const int *n, int nprob, long M);
int vt_infill_proj_forward(const float *const *xs, const float *const *weights, const float *const *biases, const int *kin, const int *n, int nprob, long M,
                           float *const *ys, void *stream);
int vt_infill_proj_backward(const float *const *d_ys, const float *const *xs, const int *kin, const int *n, int nprob, long M, float *const *d_weights,
                            float *const *d_biases, int accumulate, float *workspace, void *stream);
long vt_infill_head_workspace_floats(int B, int T, int D, int hidden, int out_dim);
int vt_infill_head_forward(const float *f, const float *const *params, const float *gt, int B, int T, int D, int hidden, int out_dim, double lw_pose,
                           double lw_accel, float *pred, float *h, double *terms, float *workspace, void *stream);
int vt_infill_head_backward(const float *d_pred_in, const float *gt, const float *pred, const float *h, const float *f, const float *const *params, int B, int T,
                            int D, int hidden, int out_dim, double lw_pose, double lw_accel, double upstream, double *terms, float *d_pred, float *d_f,
                            float *const *d_params, int accumulate, float *workspace, void *stream);

/* ---- HVOP-Net training, the data set (clipdata.hip): the decisions of a clip and the assembly of a batch of clips on the device.  The packed data of all
 * sequences is fp32, concatenated over N frames: poses (N, 72) = columns [:69] + [111:114] of the SMPL-H pose (traindata_mfiller.py:102-105), trans, roots,
 * obj_angles, obj_trans (N, 3); w2c_R (n_dates, 4, 3, 3) and w2c_t (n_dates, 4, 3) are KinectTransform's world2local_R / world2local_t per date and camera.
 *
 * vt_clip_draw replaces the np.random calls of TrainDataCMotionFiller.get_item and gen_masks (traindata_cmfiller.py:24-28, 46; traindata_mfiller.py:222-229) for
 *   B clips, one thread a clip: kid in [0, 4) when multi_kinects, else 1; drop_len in [min_drop_len, max_drop_len]; start_fr in [start_fr_min,
 *   min(T - drop_len, start_fr_max)); aug_start (B, aug_num) in [0, T - aug_num).  A decision is a function of (seed, epoch, clip_index[b], draw number) through
 *   the hash and the sites of csrc/dropout_hash.h, mapped by multiply-shift: integers only, independent of the batch and of the launch.  A range that can be empty
 *   (min(T - max_drop_len, start_fr_max) <= start_fr_min, T <= aug_num, max_drop_len < min_drop_len) is VT_ERR_ARG; nothing is clamped.  aug_num <= 64.
 * vt_clip_build replaces get_smpl_input / get_obj_input (traindata_mfiller.py:231-296), the masking and the noise augmentation (traindata_cmfiller.py:34-51) and
 *   utils/geometry_utils.py:63-77, 92-246, 284-354 under them.  start, date, kid, drop_len, start_fr (B,), aug_start (B, aug_num): clip b is frames
 *   [start[b], start[b] + T) seen from camera kid[b] of date date[b].  Outputs: data_smpl, gt_smpl (B, T, 147) = 24 x 6D | translation; data_obj, gt_obj
 *   (B, T, obj_dim), obj_dim 6 (6D) or 9 (6D | translation); mask_obj (B, T) bytes, 1 on [start_fr, start_fr + drop_len); mask_smpl all 0.  gt_* are taken
 *   before masking; data_obj is multiplied by (1 - mask); with aug_num > 0 the aug_num windows of aug_num frames get 6D(axis(data_obj) + 0.5 z), the window with
 *   the highest number winning an overlap and every window reading the masked, un-noised row.  z: `noise` (B, aug_num^2, 3), value (j aug_num + frame in window)
 *   of window j, or with noise == NULL the Box-Muller normal of two hashed words (needs clip_index, seed, epoch as vt_clip_draw).  kid == 1 copies the
 *   translations bit for bit.  fp32, one thread per rotation slot, no atomics, no workspace, the same bits on every call, clips independent of each other.
 *   A clip whose start, kid or date lies outside its table reads nothing and comes out as zeros.  VT_ERR_ARG: a NULL pointer, obj_dim, aug_num, N < T. */
int vt_clip_draw(const int *clip_index, int B, unsigned long long seed, unsigned int epoch, int T, int multi_kinects, int min_drop_len, int max_drop_len,
                 int start_fr_min, int start_fr_max, int aug_num, int *kid, int *drop_len, int *start_fr, int *aug_start, void *stream);
int vt_clip_build(const float *poses, const float *trans, const float *roots, const float *obj_angles, const float *obj_trans, long N,
                  const float *w2c_R, const float *w2c_t, int n_dates, const int *start, const int *date, const int *kid, const int *drop_len,
                  const int *start_fr, const int *aug_start, int B, int T, int obj_dim, int aug_num, const float *noise, const int *clip_index,
                  unsigned long long seed, unsigned int epoch, float *data_smpl, float *data_obj, float *gt_smpl, float *gt_obj,
                  unsigned char *mask_obj, unsigned char *mask_smpl, void *stream);

/* ---- box calibration (measurement infrastructure of bench.py; no counterpart in the reference, which times whole processes: README.md:55) ------------------
 * Two fixed micro-kernels exercising the resources the dominant kernel of the fit is limited by: out[0] = dense f16 MFMA TFLOP/s (v_mfma_f32_16x16x32_f16, two
 * workgroups of 256 threads per CU, non-trivial operands), out[1] = shader clock sustained during it (MHz: s_memtime against the 100 MHz s_memrealtime),
 * out[2] = L2 -> register delivery of lane-linear 16-byte loads (TB/s), out[3], out[4] = their durations in ms.  `work`: vt_calibrate_workspace_bytes() bytes
 * of device memory.  Synchronises `stream`; ~25 ms. */
/* clock probe of the fused-objective query kernels (measurement only): while `counters` (3 device-side 64-bit words, zeroed by the caller) is set, every 1024th
 * workgroup of every vt_query_* launch adds its life time in shader clocks, in 100 MHz ticks, and 1 -- counters[0] / counters[1] x 100 = the shader clock in MHz the
 * chip sustained DURING those launches.  NULL switches it off (the default). */
int vt_query_set_clock_probe(unsigned long long *counters);
long vt_calibrate_workspace_bytes(void);
int vt_calibrate(void *work, double *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VISTRACKER_H */
