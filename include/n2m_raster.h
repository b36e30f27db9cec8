/*
 * n2m_raster.h -- stage-1 differentiable rasterisation primitives.
 *
 * Replaces, for nerf2mesh's call sites, the three nvdiffrast operators the reference imports as
 * `import nvdiffrast.torch as dr` (nerf/renderer.py:15):
 *     dr.rasterize   :126-128,338,860,968      dr.interpolate :339-340,862-863      dr.antialias :886-887
 * nvdiffrast is NOT vendored in the reference (unpinned git HEAD, readme.md:28-29) and is absent here, so these entry
 * points implement the published semantics -- parity with an nvdiffrast build is UNPINNED; the
 * checks are an independent C oracle (oracle/n2m_raster_oracle.c) plus analytic / finite-difference properties.
 *
 * Conventions: as n2m_hip.h (device pointers, void* stream, int status).  One image per call (minibatch 1, which is what
 * every call site uses: `vertices_clip ... .unsqueeze(0)`, nerf/renderer.py:858).
 *   pos  [V,4] f32 clip-space (x,y,z,w)      tri [F,3] i32      rast [H,W,4] f32 = (u, v, z/w, triangle_id+1)
 * Image row 0 is y_ndc = -1 (OpenGL bottom-up), pixel centres at half-integers.
 */
#ifndef N2M_RASTER_H
#define N2M_RASTER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* dr.rasterize.  zbuf: scratch [H*W] u64 (any contents).  rast: output.
 * Visibility: nearest z/w wins, ties -> lower triangle id; both windings are drawn (no culling); coverage uses 1/256-pixel
 * fixed-point edge functions with a top-left tie rule (each pixel centre on a shared edge belongs to exactly one of the
 * two triangles); triangles with a vertex at w <= 0 take a float homogeneous path.  (u,v) are the perspective-correct
 * barycentric weights of the triangle's FIRST TWO vertices; z/w is clamped to [-1,1]; empty pixels are all-zero. */
int n2m_rasterize_forward(const float* pos, const int32_t* tri, uint32_t V, uint32_t F, uint32_t H, uint32_t W,
                          unsigned long long* zbuf, float* rast, void* stream);

/* Gradient of (u,v) w.r.t. pos: grad_pos [V,4] += ...  (z/w and the id carry no gradient).  d_rast [H,W,4]. */
int n2m_rasterize_backward(const float* pos, const int32_t* tri, const float* rast, const float* d_rast, uint32_t V,
                           uint32_t F, uint32_t H, uint32_t W, float* grad_pos, void* stream);

/* dr.interpolate: out[h,w,:] = u*attr[i0] + v*attr[i1] + (1-u-v)*attr[i2] for covered pixels, 0 elsewhere.
 * attr [V,A] f32, out [H,W,A]. */
int n2m_interpolate_forward(const float* attr, const float* rast, const int32_t* tri, uint32_t V, uint32_t F, uint32_t A,
                            uint32_t H, uint32_t W, float* out, void* stream);

/* grad_attr [V,A] += scatter of d_out; grad_rast [H,W,4] (channels 0,1 written, 2,3 zero) may be NULL. */
int n2m_interpolate_backward(const float* attr, const float* rast, const int32_t* tri, const float* d_out, uint32_t V,
                             uint32_t F, uint32_t A, uint32_t H, uint32_t W, float* grad_attr, float* grad_rast,
                             void* stream);
/* The same with d_out pixels `d_out_stride` floats apart (>= A): the gradient of one channel of a wider image (the coverage channel of an RGBA
 * gradient, say) without an extraction pass.  Only covered pixels are read. */
int n2m_interpolate_backward_strided(const float* attr, const float* rast, const int32_t* tri, const float* d_out, uint32_t d_out_stride,
                                     uint32_t V, uint32_t F, uint32_t A, uint32_t H, uint32_t W, float* grad_attr, float* grad_rast,
                                     void* stream);

/* Edge -> opposite-vertex hash used by antialias.  table: [capacity] entries of 4 x i32 (va, vb, op0, op1), capacity a
 * power of two >= 4*F (caller allocates 16*capacity bytes; contents are overwritten).  An edge with more than two faces keeps
 * op1 = -2: it has no single neighbour, and antialias treats it as a silhouette for every incident face, so the result does
 * not depend on the order of the faces or of the table's construction. */
int n2m_antialias_build_topology(const int32_t* tri, uint32_t F, int32_t* table, uint32_t capacity, void* stream);

/* dr.antialias.  color [H,W,C] f32 -> out [H,W,C]: for every horizontally / vertically adjacent pixel pair whose
 * triangle ids differ, the nearer surface's triangle is examined; if one of its SILHOUETTE edges (boundary edge, edge with
 * more than two faces, or the two adjacent triangles lie on the same screen-space side) crosses the segment joining the two pixel centres at
 * fraction d (measured from the covered pixel), the pixel on the far side of the midpoint is blended toward its
 * neighbour by |0.5 - d|. */
int n2m_antialias_forward(const float* color, const float* rast, const float* pos, const int32_t* tri,
                          const int32_t* table, uint32_t capacity, uint32_t V, uint32_t F, uint32_t C, uint32_t H,
                          uint32_t W, float* out, void* stream);

/* Gradients: grad_color [H,W,C] (written), grad_pos [V,4] += (through d; scaled by pos_gradient_boost). */
int n2m_antialias_backward(const float* color, const float* rast, const float* pos, const int32_t* tri,
                           const int32_t* table, uint32_t capacity, const float* d_out, uint32_t V, uint32_t F, uint32_t C,
                           uint32_t H, uint32_t W, float pos_gradient_boost, float* grad_color, float* grad_pos,
                           void* stream);
/* The same when grad_color (a buffer other than d_out) ALREADY holds a copy of d_out: the identity part of the operator costs no pass. */
int n2m_antialias_backward_seeded(const float* color, const float* rast, const float* pos, const int32_t* tri,
                                  const int32_t* table, uint32_t capacity, const float* d_out, uint32_t V, uint32_t F, uint32_t C,
                                  uint32_t H, uint32_t W, float pos_gradient_boost, float* grad_color, float* grad_pos,
                                  void* stream);

/* World -> clip space of the mesh, `torch.matmul(F.pad(vertices, (0, 1), value=1.0), mvp.T)` (nerf/renderer.py:858): clip [V, 4] =
 * [v, 1] @ mvp^T (mvp [4, 4] row-major), and the gradient w.r.t. the vertices d_v = d_clip @ mvp[:, :3]; one launch each (a BLAS GEMM of
 * this shape ran as a single workgroup: 2.7 ms for 159 k vertices; the broadcast torch form is seven launches forward, ten backward). */
int n2m_to_clip(const float* vertices, const float* mvp, uint32_t V, float* clip, void* stream);
int n2m_to_clip_backward(const float* d_clip, const float* mvp, uint32_t V, float* d_vertices, void* stream);

/* The two mesh regularisers of stage 1.  Uniform-Laplacian smoothness, `laplacian_smooth_loss(verts, faces)` of nerf/utils.py:176-221: with
 * L = D - A over the unique directed edges (diagonal = number of distinct neighbours), mean_i || (L v)_i ||_2; the adjacency as CSR (row_ptr
 * [V + 1], col [E] int32, a vertex's neighbours in ascending order; symmetric).  Offset penalty (nerf/utils.py:772-789): mean_i |off_i|^2, or
 * with bound > 1 the inner mesh's mean + 0.1 x the outer meshes' (vertices [0, n_in) inner).
 * forward: Lv [V, 3] = L v, norm [V], partial [ceil(V / 256)] = per-workgroup sums of lam_lap / V * norm_i + w_i |off_i|^2 with w_i = w_in for
 *   i < n_in, else w_out (the caller folds lambda_offsets and the group sizes into them; offsets = NULL: the smoothness term alone):
 *   value = sum(partial).
 * backward: d_verts [V, 3] from the saved Lv / norm and the incoming gradient (device scalar): d v_i = deg_i gL_i - sum_{j in N(i)} gL_j,
 *   gL_k = grad lam_lap / V * Lv_k / norm_k (0 where the norm is 0); d_offsets [V, 3] = grad w_i 2 off_i (with offsets, else NULL). */
int n2m_laplacian_forward(const float* verts, const int32_t* row_ptr, const int32_t* col, uint32_t V, const float* offsets, float lam_lap, float w_in,
                          float w_out, uint32_t n_in, float* Lv, float* norm, float* partial, void* stream);
int n2m_laplacian_backward(const float* Lv, const float* norm, const int32_t* row_ptr, const int32_t* col, uint32_t V, const float* grad, float lam_lap,
                           const float* offsets, float w_in, float w_out, uint32_t n_in, float* d_verts, float* d_offsets, void* stream);
/* The same two gradients ADDED onto d_verts, which already holds the rendering gradient of the vertex positions: with verts = base + offsets
 * (nerf/renderer.py:855) all three are the offsets' gradient, so d_verts <- (d_verts + smoothness) + offset penalty in one pass; found_inf
 * (device float, optional) is raised when the sum is not finite -- the check torch.amp's unscale_ would make on that gradient. */
int n2m_laplacian_backward_acc(const float* Lv, const float* norm, const int32_t* row_ptr, const int32_t* col, uint32_t V, const float* grad,
                               float lam_lap, const float* offsets, float w_in, float w_out, uint32_t n_in, float* d_verts, float* found_inf,
                               void* stream);

/* Normal-consistency and edge-length losses of the mesh, pytorch3d's `mesh_normal_consistency` / `mesh_edge_loss` as nerf/utils.py:759-769
 * calls them (one mesh, target edge length 0), on a topology built once per mesh (trainer.MeshEdgeTerms):
 *   edges [E, 2] int32: the unique undirected edges, v0 < v1;  pairs [P, 4] int32 (16-byte aligned): (v0, v1, a, b) for every pair of faces
 *   on an edge (an edge with k faces gives k (k - 1) / 2), v0 < v1 the edge's endpoints, a / b the vertices opposite it in the two faces.
 *   Per pair, with e = v1 - v0, n0 = e x (a - v0), n1 = -(e x (b - v0)): 1 - n0 . n1 / (max(|n0|, 1e-8) max(|n1|, 1e-8)); per edge |v0 - v1|^2.
 * forward: partial [ceil(P / 256) + ceil(E / 256)] = per-workgroup sums of w_normal * (pair term), then of w_edge * (edge term), in a fixed
 *   order: value = sum(partial).  The caller folds 1 / P, 1 / E and the loss weights into w_normal / w_edge.
 * backward: d_verts [V, 3] = grad (device scalar) times the gradient of that value.  One thread per vertex walks two CSRs (pair_ptr / edge_ptr
 *   [V + 1]; pair_ref = 4 * pair + corner, edge_ref = 2 * edge + corner of every term the vertex takes part in, ascending) and recomputes each
 *   term's gradient for its corner: a fixed summation order, no atomics.  Where a norm is below 1e-8 the gradient is that of the clamped
 *   expression (finite for a zero-area face), as torch's is.  _acc ADDS the result onto d_verts.
 * P = 0 leaves the pair arrays unread (they may be NULL), E = 0 the edge arrays; with P = E = 0 or V = 0 nothing is launched or written. */
int n2m_mesh_losses_forward(const float* verts, const int32_t* pairs, uint32_t P, const int32_t* edges, uint32_t E, float w_normal, float w_edge,
                            float* partial, void* stream);
int n2m_mesh_losses_backward(const float* verts, const int32_t* pairs, const int32_t* pair_ptr, const int32_t* pair_ref, uint32_t P,
                             const int32_t* edges, const int32_t* edge_ptr, const int32_t* edge_ref, uint32_t E, uint32_t V, const float* grad,
                             float w_normal, float w_edge, float* d_verts, void* stream);
int n2m_mesh_losses_backward_acc(const float* verts, const int32_t* pairs, const int32_t* pair_ptr, const int32_t* pair_ref, uint32_t P,
                                 const int32_t* edges, const int32_t* edge_ptr, const int32_t* edge_ref, uint32_t E, uint32_t V, const float* grad,
                                 float w_normal, float w_edge, float* d_verts, void* stream);

/* Rows of a [N, C] fp32 array by index -- the boolean-mask gather / scatter around the shading of a stage-1 frame (nerf/renderer.py:864,
 * 875-881: `xyzs[mask]`, `rgbs[mask] = ...`) once the covered pixels are an index list: out[k, :] = x[idx[k], :] and dst[idx[k], :] = src[k, :]
 * (idx int64 [K], unique for the scatter; rows of dst that are not listed keep their value). */
int n2m_gather_rows(const float* x, const int64_t* idx, uint32_t K, uint32_t C, float* out, void* stream);
int n2m_scatter_rows(const float* src, const int64_t* idx, uint32_t K, uint32_t C, float* dst, void* stream);
/* The same over rows that are `*_stride` floats apart (>= C): the C leading floats of each row move, the rest of the row keeps its value --
 * the RGB of an RGBA image without a repacking copy either side. */
int n2m_gather_rows_strided(const float* x, const int64_t* idx, uint32_t K, uint32_t C, uint32_t x_stride, float* out, uint32_t out_stride,
                            void* stream);
int n2m_scatter_rows_strided(const float* src, const int64_t* idx, uint32_t K, uint32_t C, uint32_t src_stride, float* dst, uint32_t dst_stride,
                             void* stream);

/* The scene contraction of the unbounded recipes and its inverse (nerf/renderer.py:25-41) on N rows of three floats:
 *   contract:    mag = max(|x|, |y|, |z|);  mag <= 1 ? x : x * (2 - 1 / mag) / mag
 *   uncontract:  mag = max(|x|, |y|, |z|);  mag <= 1 ? x : x * (1 / (2 * mag - mag * mag))
 * in the operation order of the torch statements, every operation rounded on its own: the result equals the statement's on CPU fp32
 * tensors bit for bit, rows with NaN (-> all NaN, torch.amax hands a NaN on) or infinite components included.  out may be xyz.
 * N == 0 launches nothing; a NULL tensor with N > 0 is N2M_EINVAL. */
int n2m_contract(const float* xyz, uint32_t N, float* out, void* stream);
int n2m_uncontract(const float* xyz, uint32_t N, float* out, void* stream);
/* The stage-1 executor's surface points in one launch: pts[k, :] = img[idx[k], 0:3] of an image whose rows are `cols_in_stride` (>= 3; 4 for
 * the RGBA image) floats apart, contracted as above when `contract` is set, and x01[k, :] = pts[k, :] mapped from [-bound, bound] to [0, 1] the
 * way the grid encoder's caller does it on the device: 0.5 + pts * (0.5 / bound) for a power-of-two bound, else
 * (pts + bound) * (1 / (2 bound)) (torch's device division by a host scalar multiplies by the reciprocal).  With contract == 0 both outputs
 * equal n2m_gather_rows_strided followed by those torch statements bit for bit.  img is only read.  K == 0 launches nothing; a NULL tensor
 * with K > 0, a stride below 3 or a bound that is not positive and finite is N2M_EINVAL. */
int n2m_gather_contract_x01(const float* img, const int64_t* idx, uint32_t K, uint32_t cols_in_stride, int contract, float bound, float* pts,
                            float* x01, void* stream);

/* Stage-1 image head, forward AND backward in one launch: what nerf/renderer.py:886-913 does with the two antialias outputs (clamp,
 * image = alpha * rgb, depth = alpha * z/w, T = 1 - alpha, ssaa reduction by `scale_img_hwc` = bilinear minification (exactly the 2 x 2
 * mean for ssaa 2) and nearest for the triangle id, image + T * bg, weights_sum = 1 - T) plus the per-pixel loss of nerf/utils.py:708-721
 * (lambda_rgb * mean_c (image - gt_rgb)^2 + lambda_mask * (weights_sum - gt_a)^2, gt_rgb = gt * gt_a + bg * (1 - gt_a)).
 *   aa_alpha [h0 s, w0 s] f32, aa_rgb [h0 s, w0 s, 3] f32: the antialias outputs BEFORE the clamp; rast [h0 s, w0 s, 4]; s = ssaa (1 | 2)
 *   gt_rgba [h0 w0, 4]; bg [h0 w0, 3] or NULL (then bg_scalar)
 *   out: image [h0 w0, 3], depth / weights_sum / trig_id (id - 1 as float, -1 = empty) / loss_px [h0 w0]; partial [ceil(h0 w0 / 256)] =
 *        per-workgroup sums of loss_px (mean = sum(partial) / (h0 w0), summed by the caller in index order)
 *   d_alpha [h0 s, w0 s], d_rgb [h0 s, w0 s, 3] (both or neither): gradient of mean(loss_px) w.r.t. aa_alpha / aa_rgb; the caller scales
 *        them by its incoming gradient (the loss scale).
 *   tri_err, tri_cnt [faces] f32 (both or neither): `update_triangles_errors` (nerf/renderer.py:924-943) in the same pass -- loss_px added to
 *        tri_err[trig_id], 1 to tri_cnt[trig_id] for every pixel that shows a face (float atomics, like torch's scatter_add_).
 *   packed_rgba != 0: the two antialias calls were ONE call on an [h0 s, w0 s, 4] image (RGB + alpha: the silhouette blend is per channel, so
 *        the values are the same): aa_rgb = that image, aa_alpha = aa_rgb + 3, pixel stride 4 for both; d_rgb / d_alpha likewise point into
 *        one [h0 s, w0 s, 4] gradient image.
 *   seed (device scalar or NULL): factor on d_alpha / d_rgb -- the loss scale, when the caller knows that the gradient flowing into the mean
 *        is exactly that scalar (it then skips its own multiplication of the two full-resolution images).
 *   d_copy (packed layout only, or NULL): a second [h0 s, w0 s, 4] image that receives the same gradient -- what n2m_antialias_backward_seeded
 *        takes as its pre-filled grad_color, in place of a copy pass over the image. */
int n2m_stage1_head(const float* aa_alpha, const float* aa_rgb, const float* rast, uint32_t h0, uint32_t w0, uint32_t ssaa,
                    const float* gt_rgba, const float* bg, float bg_scalar, float lambda_rgb, float lambda_mask, float* image, float* depth,
                    float* weights_sum, float* trig_id, float* loss_px, float* d_alpha, float* d_rgb, float* partial, float* tri_err,
                    float* tri_cnt, int packed_rgba, const float* seed, float* d_copy, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* N2M_RASTER_H */
