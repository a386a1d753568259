/*
 * ured_hip.h — C-ABI of libured_hip.so, the MI355X (gfx950) hot path of the
 * U-RED retrieval-and-deformation training step.
 *
 * Conventions (all entry points):
 *   - plain device pointers + sizes, no torch types; fp32 point sets are
 *     contiguous AoS [.., 3]; indices are int32.
 *   - `stream` is a hipStream_t (0 = null stream); nothing synchronises the
 *     host, nothing allocates: callers pass workspaces where one is needed.
 *   - return 0 on success, otherwise a non-zero code (a hipError_t or
 *     URED_EINVAL); ured_last_error() then holds a thread-local message.
 *     (The reference returns 1/0 after printf and its wrapper ignores it,
 *     chamfer3D.cu:145-151 / dist_chamfer_3D.py:45; our wrapper raises.)
 *
 * Reference interfaces replaced (paths relative to the reference root):
 *   ured_nn_fwd      <- chamfer_3D.forward   chamfer_cuda.cpp:17-19 -> chamfer3D.cu:136-154
 *   ured_nn_bwd      <- chamfer_3D.backward  chamfer_cuda.cpp:22-28 -> chamfer3D.cu:176-195
 *     (both under Density_aware_Chamfer_Distance/utils_v2/metrics/CD/chamfer3D/)
 *   ured_nn_seg_fwd  <- the per-sample loops of loss/chamfer_loss.py:13-30
 *                       (Shape_Measure ChamferLoss calls) and
 *                       loss/basic_loss.py:249-265 (pytorch3d knn_points K=1),
 *                       batched into one ragged launch.
 *   ured_nn_fwd_ws / ured_nn_seg_fwd_ws <- the same two, both directions in one pass
 *   ured_get_shape_fwd/bwd <- get_shape's torch.bmm (dataset/dataset_utils.py:691-726)
 *   ured_emd_fwd / ured_emd_bwd <- emd.forward / emd.backward (utils_v2/metrics/EMD/emd.cpp:14-24)
 *   ured_nn_seg_bwd  <- autograd of the above (NmDistanceGradKernel semantics,
 *                       chamfer3D.cu:155-174, made deterministic).
 *   ured_node_gemm / ured_node_bn_fwd / ured_node_bn_bwd <- the graph-node Conv1d / BatchNorm1d
 *                       layers of DeformNet_MatchingNet (network/deformation_net.py:61,90,
 *                       attention_graph/attention_gnn.py:20-54, attention_utils.py:62-86).
 *   ured_fps / ured_ball_query / ured_group_fwd / ured_group_bwd <- farthest_point_sample,
 *                       query_ball_point, index_points + sample_and_group and their autograd
 *                       (network/pointnet/pointnet2_utils.py:43-138).
 *   ured_interp_fwd / ured_interp_bwd <- the three-neighbour inverse-distance interpolation and
 *                       the cat of PointNetFeaturePropagation (pointnet2_utils.py:293-309) and
 *                       their autograd.
 *   ured_gcn_dirs / ured_gcn_conv_fwd / ured_gcn_conv_bwd / ured_gcn_pool_fwd / ured_gcn_pool_bwd <-
 *                       get_neighbor_direction_norm, Conv_surface, Conv_layer and Pool_layer of 3D-GCN
 *                       (network/P_3DGC.py:60-190) and their autograd.
 *   ured_vn_knn / ured_vn_act_fwd / ured_vn_act_bwd / ured_vn_maxpool_fwd / ured_vn_maxpool_bwd /
 *   ured_vn_frame_fwd / ured_vn_frame_bwd <- knn and get_graph_feature (network/VN/vn_dgcnn_util.py:11-47),
 *                       VNLinearLeakyReLU, VNBatchNorm, VNMaxPool and VNStdFeature's einsum
 *                       (network/VN/vn_layers.py:48-77, 112-149, 199) and their autograd.
 *   ured_dcd_loss_fwd / ured_dcd_loss_bwd <- the torch tail of calc_dcd under autograd
 *                       (Density_aware_Chamfer_Distance/utils_v2/model_utils.py:13-51) and its autograd.
 *   ured_pcn_relu / ured_pcn_pool_bwd / ured_pcn_fold_fwd / ured_pcn_fold_bwd / ured_pcn_center_fwd /
 *   ured_pcn_center_bwd <- the ReLUs, max-pools, concatenations and the `+ center` of PCN_encoder /
 *                       PCN_decoder (Density_aware_Chamfer_Distance/models/pcn.py:13-71) and their autograd.
 *   ured_vrc_sa_fwd / ured_vrc_sa_bwd / ured_vrc_sk_mean_fwd / ured_vrc_sk_mean_bwd / ured_vrc_sk_mix_fwd /
 *   ured_vrc_sk_mix_bwd / ured_vrc_pool_fwd / ured_vrc_pool_bwd / ured_vrc_unpool_fwd / ured_vrc_unpool_bwd
 *                       <- the attention core of SA_module, the branch selection of SK_SA_module,
 *                       edge_preserve_sampling's gather + max and three_interpolate
 *                       (Density_aware_Chamfer_Distance/models/vrcnet.py:15-290) and their autograd.
 *   ured_vrc_ef_edge_fwd / ured_vrc_ef_edge_bwd / ured_vrc_ef_max_fwd / ured_vrc_ef_max_bwd / ured_vrc_fold_fwd /
 *   ured_vrc_fold_bwd   <- the per-edge part of EF_expansion (utils/model_utils.py:137-166) and Folding's
 *                       repeat + concatenation + ReLU (models/vrcnet.py:54-86) and their autograd.
 *   ured_vrc_latent_fwd / ured_vrc_latent_bwd / ured_vrc_gauss_fwd / ured_vrc_gauss_bwd
 *                       <- Model's softplus, rsample, kl_divergence and compute_kernel
 *                       (models/vrcnet.py:430-501) and their autograd.
 */
#ifndef URED_HIP_H
#define URED_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define URED_OK 0
#define URED_EINVAL 1001

/* Library identification: returns URED_ABI_VERSION. */
#define URED_ABI_VERSION 19  /* 19: ured_vrc_latent_fwd / ured_vrc_latent_bwd / ured_vrc_gauss_fwd / ured_vrc_gauss_bwd; 18: ured_vrc_ef_edge_fwd / ured_vrc_ef_edge_bwd / ured_vrc_ef_max_fwd / ured_vrc_ef_max_bwd / ured_vrc_fold_fwd / ured_vrc_fold_bwd; 17: ured_vrc_sa_fwd / ured_vrc_sa_bwd / ured_vrc_sk_mean_fwd / ured_vrc_sk_mean_bwd / ured_vrc_sk_mix_fwd / ured_vrc_sk_mix_bwd / ured_vrc_pool_fwd / ured_vrc_pool_bwd / ured_vrc_unpool_fwd / ured_vrc_unpool_bwd; 16: ured_dcd_loss_fwd / ured_dcd_loss_bwd, ured_pcn_relu / ured_pcn_pool_bwd / ured_pcn_fold_fwd / ured_pcn_fold_bwd / ured_pcn_center_fwd / ured_pcn_center_bwd; 15:ured_vn_parts / ured_vn_knn / ured_vn_act_fwd / ured_vn_act_bwd / ured_vn_maxpool_fwd / ured_vn_maxpool_bwd / ured_vn_frame_fwd / ured_vn_frame_bwd; 14: ured_gcn_dirs / ured_gcn_conv_fwd / ured_gcn_conv_bwd / ured_gcn_conv_bwd_parts / ured_gcn_pool_fwd / ured_gcn_pool_bwd; 13: ured_interp_fwd / ured_interp_bwd; 12: ured_fps / ured_ball_query / ured_group_fwd / ured_group_bwd; 11: ured_knn_fwd / ured_knn_bwd; 10: ured_occlude; 9: ured_attn_fwd_sets / ured_attn_bwd_sets, ured_get_shape_src_fwd / _bwd; 8: ured_nn_bwd_set; 7: ured_copy_batch; 6: ured_part_rows_bwd_add; 5: node BN SyncBN fields (stats_out/stats_in, sums_out/sums_in); ured_bn_stats et al. */
int ured_abi_version(void);
/* Thread-local message for the last failing call on this thread ("" if none). */
const char* ured_last_error(void);

/* ---------------- nearest neighbour (chamfer) ---------------- */

/* Dense NN, both directions (reference chamfer_3D.forward).
 * xyz1 [b,n,3], xyz2 [b,m,3] ->
 *   dist1[b,n] = min_k |xyz2[k]-xyz1[j]|^2, idx1[b,n] its argmin (lowest index on ties)
 *   dist2[b,m], idx2[b,m] vice versa.
 * Distance formula (bit-exact contract): d = fmaf(dz,dz, fmaf(dy,dy, dx*dx)), dx = q2.x - q1.x.
 * dirs: bit 0 -> compute (dist1, idx1); bit 1 -> compute (dist2, idx2). */
int ured_nn_fwd(const float* xyz1, const float* xyz2, int b, int n, int m, int dirs,
                float* dist1, int* idx1, float* dist2, int* idx2, void* stream);

/* Dense NN backward (reference chamfer_3D.backward): accumulates
 *   gxyz1[j] += 2 gd1[j] (p1_j - p2_idx1[j]) - sum_{k: idx2[k]=j} 2 gd2[k] (p2_k - p1_j)
 * and symmetrically into gxyz2. Deterministic (gather form, k ascending), no atomics.
 * gd1/gd2 may be NULL (treated as zero). */
int ured_nn_bwd(const float* xyz1, const float* xyz2, int b, int n, int m,
                const float* gd1, const float* gd2, const int* idx1, const int* idx2,
                float* gxyz1, float* gxyz2, void* stream);
/* The same gradient WRITTEN instead of accumulated (every element of gxyz1 / gxyz2 is set, so
 * the caller needs no zero fill; n, m > 0). The autograd Function behind chamfer_3DDist uses it;
 * ured_nn_bwd keeps the reference's accumulate-into-caller-zeroed-buffers contract. */
int ured_nn_bwd_set(const float* xyz1, const float* xyz2, int b, int n, int m,
                    const float* gd1, const float* gd2, const int* idx1, const int* idx2,
                    float* gxyz1, float* gxyz2, void* stream);

/* Ragged NN over segment pairs. segs is a DEVICE int32 array [nseg][4] =
 * {a_off, a_len, b_off, b_len} in points of the two buffers a [*,3] and b [*,3].
 * Within one call, a-ranges must be pairwise disjoint and so must b-ranges.
 * For every pair: dist_a[a_off+i], idx_a[a_off+i] = NN of a-point i among the
 * pair's b-points (idx relative to b_off); and vice versa into dist_b/idx_b.
 * Points not covered by any pair are left untouched. max_a_len / max_b_len are
 * host-side upper bounds of a_len / b_len (they size the grid; no host sync).
 * A pair with an empty other side writes dist 0, idx 0. */
int ured_nn_seg_fwd(const float* a, const float* b, const int* segs, int nseg,
                    int max_a_len, int max_b_len, int dirs,
                    float* dist_a, int* idx_a, float* dist_b, int* idx_b, void* stream);

/* Fused forward (both directions from ONE evaluation of every pair distance; same results,
 * bit for bit, as ured_nn_fwd / ured_nn_seg_fwd with dirs = 3). The caller passes a device
 * workspace of ured_nn_fwd_workspace(...) bytes (no initialisation needed; contents are
 * scratch). a_total / b_total = number of points in the a / b buffers (dense: b*n, b*m).
 * ured_nn_fwd_workspace returns 0 when the fused path does not apply (dirs != 3, empty
 * sizes); the _ws entry points then (or with workspace == NULL) run the two-pass kernel. */
#include <stddef.h>
size_t ured_nn_fwd_workspace(int nseg, int max_a_len, int max_b_len, int a_total, int b_total, int dirs);
int ured_nn_fwd_ws(const float* xyz1, const float* xyz2, int b, int n, int m, int dirs,
                   float* dist1, int* idx1, float* dist2, int* idx2, void* workspace, size_t ws_bytes,
                   void* stream);
int ured_nn_seg_fwd_ws(const float* a, const float* b, const int* segs, int nseg,
                       int max_a_len, int max_b_len, int dirs, int a_total, int b_total,
                       float* dist_a, int* idx_a, float* dist_b, int* idx_b,
                       void* workspace, size_t ws_bytes, void* stream);

/* K nearest neighbours (pytorch3d.ops.knn_points semantics; the reference's call sites are
 * loss/basic_loss.py:257 with K = 1 and dataset/gen_occ_point.py:31-33 with K = N / 2).
 * p1 [b,n,3] queries, p2 [b,m,3] refs -> dists [b,n,K], idx [b,n,K]: row i of sample b lists the
 * min(K, len2) valid p2 points with the smallest (distance, index), ascending in that order
 * (lowest index on ties), by the contract distance of ured_nn_fwd with the p1 point as the query;
 * column 0 is bitwise dist1 / idx1 of ured_nn_fwd. lengths1 / lengths2: DEVICE int32 [b] numbers
 * of valid points per sample (NULL = n / m), clamped into [0, n] / [0, m] on the device (no host
 * read). Slots k >= len2 and every slot of a row i >= len1 are written as dist 0, idx 0.
 * Limits: 1 <= K <= 1024; K <= 32: any m (one thread per query, the K best in registers);
 * K > 32: m <= 4096 (one workgroup per query, a sort in LDS); K > m is allowed (padding);
 * b <= 65535, n * K < 2^31. No workspace. */
int ured_knn_fwd(const float* p1, const float* p2, int b, int n, int m, int K, const int* lengths1,
                 const int* lengths2, float* dists, int* idx, void* stream);
/* Its backward, WRITTEN as by ured_nn_bwd_set (every element of grad_p1 [b,n,3] and grad_p2
 * [b,m,3] is set; rows beyond len1 and points beyond len2 get zeros). Over the valid slots, with
 * g = grad_dists[b,i,k] and j = idx[b,i,k]:
 *   grad_p1[b,i] = sum_k 2 g (p1_i - p2_j)        grad_p2[b,j] = - sum_{(i,k): idx = j} 2 g (p1_i - p2_j)
 * Deterministic (gather form, (i,k) ascending), no atomics. */
int ured_knn_bwd(const float* p1, const float* p2, int b, int n, int m, int K, const int* lengths1,
                 const int* lengths2, const float* grad_dists, const int* idx, float* grad_p1, float* grad_p2,
                 void* stream);

/* get_shape (dataset/dataset_utils.py:691-726): out[j, r] = sum_k A[j, r, k] p[j, k] for every
 * part slot j (A [nparts, rows, 6] contiguous, 8-byte aligned; p [nparts, 6] = weight*param +
 * default); the backward gives grad_p[j, k] = sum_r A[j, r, k] grad_out[j, r] (deterministic). */
int ured_get_shape_fwd(const float* A, const float* p, int nparts, int rows, float* out, void* stream);
int ured_get_shape_bwd(const float* A, const float* grad_out, int nparts, int rows, float* grad_p, void* stream);
/* The training step's form (engine/train.py:222-223: get_source_info + get_shape): part slot j reads
 * mats + src_j * rows * 6, src_j = labels[j] (int64; + nsrc when negative, python indexing), so no
 * gathered copy of the source matrices; p[j] = weight * param[j] + dflt[j] (dflt may be NULL) is
 * formed in-kernel with get_shape's separate mul and add; the backward writes
 * grad_param = weight * sum_r A grad_out. */
int ured_get_shape_src_fwd(const float* mats, const long long* labels, int nsrc, const float* param,
                           const float* dflt, float weight, int nparts, int rows, float* out, void* stream);
int ured_get_shape_src_bwd(const float* mats, const long long* labels, int nsrc, const float* grad_out, float weight,
                           int nparts, int rows, float* grad_param, void* stream);

/* Per-part axis-aligned boxes (compute_aabbox, dataset/dataset_utils.py:77-85, as used by
 * get_part, engine/train.py:119-128): x [R,3] points sorted by segment, off int32 [G+1] row
 * offsets -> out [G,6] = (center, half extent) of each segment; empty segments give zeros. */
int ured_seg_aabb(const float* x, const int* off, int G, float* out, void* stream);

/* Backward of get_part's per-point regrouping (engine/train.py:103-136: the points of every
 * sample sorted by part label, and the per-part sums of their features): for R = B*N rows of C
 * floats, out[b*N + i] = d_sorted[s] + d_sums[gid[s]] with s = b*N + inv[b, i] (the row's
 * position after the sort, inv int64 [B, N]; gid int32 [R] the part slot of each sorted row).
 * Either gradient may be NULL (zero). One pass: replaces an index_select, a gather and an add. */
int ured_part_rows_bwd(const float* d_sorted, const float* d_sums, const long long* inv, const int* gid, int B, int N,
                       int C, float* out, void* stream);
/* The same plus `add` [R,C] (may be NULL, or `out` itself: in-place accumulation): out = (d_sorted
 * + d_sums) + add, where add is another consumer's gradient of the same per-point features (the
 * reconstruction decoder's input gradient, engine/train.py:240,250): the sum autograd would form
 * in a separate pass (ABI 6). */
int ured_part_rows_bwd_add(const float* d_sorted, const float* d_sums, const long long* inv, const int* gid, int B,
                           int N, int C, const float* add, float* out, void* stream);

/* ---------------- EMD (auction algorithm) ---------------- */
/* Approximate EMD matching of xyz1 [b,n,3] to xyz2 [b,n,3] (reference emd.forward,
 * utils_v2/metrics/EMD/emd.cpp:14-19 -> emd_cuda.cu:183-256): `iters` auction rounds with
 * parameter eps; assignment[b,n] = matched xyz2 index, dist[b,n] = squared distance to it.
 * Deterministic (highest increment wins an object, ties to the lowest bidder index; scan ties to
 * the lowest object index). Workspace: ured_emd_workspace(b, n) bytes, no initialisation. */
size_t ured_emd_workspace(int b, int n);
int ured_emd_fwd(const float* xyz1, const float* xyz2, int b, int n, float eps, int iters,
                 float* dist, int* assignment, void* workspace, size_t ws_bytes, void* stream);
/* gradxyz1 += 2 graddist (xyz1 - xyz2[assignment]) (reference emd.backward, emd_cuda.cu:283-304;
 * xyz2 gets no gradient, as in emd_module.py:76-80). */
int ured_emd_bwd(const float* xyz1, const float* xyz2, int b, int n, const float* graddist, const int* assignment,
                 float* gradxyz1, void* stream);

/* Backward of ured_nn_seg_fwd: accumulates into ga (a-points) and gb (b-points)
 * exactly the per-pair formula of ured_nn_bwd. gd_a / gd_b may be NULL; gb may be NULL when
 * the b points need no gradient (only the a side is computed). */
int ured_nn_seg_bwd(const float* a, const float* b, const int* segs, int nseg,
                    int max_a_len, int max_b_len,
                    const float* gd_a, const float* gd_b, const int* idx_a, const int* idx_b,
                    float* ga, float* gb, void* stream);


/* Density-aware chamfer reduction of dense NN outputs (replaces the torch tail of
 * calc_dcd, Density_aware_Chamfer_Distance/utils_v2/model_utils.py:13-51, and the
 * cd_p / cd_t of calc_cd, :53-70; the NN itself is ured_nn_fwd with xyz1 = gt,
 * xyz2 = x, as calc_cd calls cham_loss(gt, output)).
 * dist1/idx1 [b,n1]: gt -> x; dist2/idx2 [b,n2]: x -> gt. Per item:
 *   w1 = frac_21 / (count_x(idx1)^n_lambda + 1e-6),  loss1 = mean(1 - exp(-alpha d1) w1)
 *   w2 = frac_12 / (count_gt(idx2)^n_lambda + 1e-6), loss2 = mean(1 - exp(-alpha d2) w2)
 *   loss = (loss1 + loss2)/2, cd_p = (mean sqrt d1 + mean sqrt d2)/2, cd_t = mean d1 + mean d2.
 * Forward only (no autograd), deterministic. n1 + n2 <= 16384. */
int ured_dcd(const float* dist1, const int* idx1, const float* dist2, const int* idx2, int b, int n1, int n2,
             float alpha, int n_lambda, float frac_12, float frac_21, float* loss, float* cd_p, float* cd_t,
             void* stream);

/* The same reduction as a training loss (calc_dcd under autograd). The exponent is a float:
 * count^lambda is 1, c, c*c or sqrtf(c) for lambda = 0, 1, 2, 0.5 and powf(c, lambda) otherwise;
 * for those integral lambdas loss / cd_p / cd_t equal ured_dcd's bit for bit. cd_p and cd_t may be
 * NULL. coef1 [b,n1] / coef2 [b,n2] (each may be NULL) receive the derivative of the item's loss
 * with respect to each squared distance, the weights detached as in the reference
 * (model_utils.py:35,41):
 *   coef1[j] = alpha exp(-alpha d1[j]) w1[j] / (2 n1),  coef2[j] = alpha exp(-alpha d2[j]) w2[j] / (2 n2).
 * Deterministic; n1 + n2 <= 16384, lambda >= 0, checked before any device work. */
int ured_dcd_loss_fwd(const float* dist1, const int* idx1, const float* dist2, const int* idx2, int b, int n1, int n2,
                      float alpha, float lambda, float frac_12, float frac_21, float* loss, float* cd_p, float* cd_t,
                      float* coef1, float* coef2, void* stream);
/* Its backward, ONE launch for both point sets: xyz1 [b,n1,3] = gt, xyz2 [b,n2,3] = x, the
 * indices and coefficients of the forward. The gradient of squared distance j of item i is
 *   g1[j] = g_loss[i] coef1[j] + gd1[j]   (g_loss NULL: no gradient through the loss;
 *                                          gd1 / gd2 NULL: no further gradient of dist1 / dist2)
 * and goes through the gather form of ured_nn_bwd_set (own term first, then the other side's
 * entries in ascending index; no float atomics). Every element of gxyz1 [b,n1,3] / gxyz2 [b,n2,3]
 * is WRITTEN; a NULL output skips that side. */
int ured_dcd_loss_bwd(const float* xyz1, const float* xyz2, const int* idx1, const int* idx2, const float* coef1,
                      const float* coef2, const float* g_loss, const float* gd1, const float* gd2, int b, int n1,
                      int n2, float* gxyz1, float* gxyz2, void* stream);

/* ---------------- per-point MLP (1x1 conv) on fp32 MFMA ---------------- *
 * Replaces the Conv1d(k=1)+BatchNorm1d+ReLU chains of TargetEncoder
 * (network/simple_encoder.py:52-107) and re_residual_net / FeedForwardNet_norm
 * (network/deformation_net.py:96-107, attention_graph/attention_utils.py:62-86),
 * forward and backward, with activations stored point-major [M][C].
 *
 * ured_gemm computes C[M][N] = sum_k A'[m][k] B'[k][n] on v_mfma_f32_32x32x2_f32
 * (exact fp32 fma chains), 128x128x32 tiles, where
 *   A'[m][k] = a_kmajor ? A[k*lda+m] : (k < k1 ? pro(A[m*lda+k]) : A2[m*lda2+k-k1])
 *   B'[k][n] = b_kmajor ? pro_b(B[k*ldb+n]) : B[n*ldb+k]
 *   pro(x)   = PRO_ENC: max(x*s[c]+t[c],0)   (Conv->BN->ReLU; c = channel = contiguous index)
 *              PRO_RES: max(x,0)*s[c]+t[c]   (Conv->ReLU->BN)
 * and an epilogue:
 *   EPI_STORE : C = acc (+bias[n])
 *   EPI_FWD   : Y = acc + bias[n] + rowbias[grp(m)][n] stored to C; per-128-row block
 *               column partials {mean, M2} of p (p = Y, or relu(Y) if stat_relu) into
 *               stat_ws[2][N][blk] (one column's block partials contiguous); if pool_ws: per block column {max,argmax,min,argmin}
 *               of Y into pool_ws[blk][4][N] (group_rows multiple of 128)
 *   EPI_BNBWD : dh = acc (+ pool_grad[g][n] where pool_idx[g][n] == m) (+ gadd[m][n]); with
 *               the previous layer's (Y, mean, invstd, scale, shift): ENC g = dh*(Y*scale+shift > 0),
 *               xhat = (Y-mean)*invstd; RES g = dh, xhat = (relu(Y)-mean)*invstd; BN g = dh,
 *               xhat = (Y-mean)*invstd. K = 0 is allowed (acc = 0: a pooled / extra gradient only);
 *               stores g to C and block column partials {sum g, sum g*xhat} to bwd_ws
 *   EPI_SPLITK: partial sums of the k-range of blockIdx.z stored to C + z*M*ldc
 */
#define URED_PRO_NONE 0
#define URED_PRO_ENC 1
#define URED_PRO_RES 2
#define URED_EPI_STORE 0
#define URED_EPI_FWD 1
#define URED_EPI_BNBWD 2
#define URED_EPI_SPLITK 3
/* EPI_BNBWD activation order of the layer whose output is being differentiated (bwd_res field) */
#define URED_ACT_ENC 0   /* Conv -> BN -> ReLU */
#define URED_ACT_RES 1   /* Conv -> ReLU -> BN */
#define URED_ACT_BN 2    /* Conv -> BN (no activation; PointNet's conv3, pointnet_utils.py:126) */

typedef struct UredGemmDesc {
    int M, N, K;
    int a_kmajor, b_kmajor, pro_a, pro_b, epi;
    const float* A; int lda;
    const float* A2; int lda2; int k1;         /* k >= k1 read from A2 (row-major A only); k1 = K if unused */
    const float* B; int ldb;
    const float* pro_s; const float* pro_t;     /* prologue per-channel affine */
    float* C; int ldc;
    const float* bias;                          /* [N] or NULL */
    const float* rowbias; int ldr;              /* [G][ldr] or NULL */
    const int* gidx; int group_rows;            /* row -> group: gidx[m] or m / group_rows */
    int stat_relu;
    float* stat_ws;                             /* [2][N][ceil(M/128)] */
    float* pool_ws;                             /* [ceil(M/128)][4][N] or NULL */
    const float* Yp; int ldy;                   /* EPI_BNBWD: previous layer's raw output */
    const float* bn_mean; const float* bn_invstd; const float* bn_scale; const float* bn_shift;
    int bwd_res;                                /* URED_ACT_ENC / URED_ACT_RES / URED_ACT_BN */
    const int* pool_idx; const float* pool_grad; int pool_group_rows;
    float* bwd_ws;                              /* [2][N][ceil(M/128)] */
    int splits;                                 /* EPI_SPLITK: gridDim.z (k-range per split = ceil(K/splits/32)*32) */
    const float* gadd; int ldg;                 /* EPI_BNBWD: optional extra gradient, dh += gadd[m*ldg+n] */
} UredGemmDesc;

int ured_gemm(const UredGemmDesc* d, void* stream);

/* Optimizer tail of the training step (reference engine/train.py:331-346: clip_grad_norm_(5.0)
 * per module, then torch.optim.Adam with L2 weight decay, train_utils/optimizer_dm.py:68-104)
 * over flat buffers param/grad/exp_avg/exp_avg_sq. Chunk c covers [chunk_beg[c], chunk_end[c])
 * (16-B aligned, lengths multiples of 4) of parameter chunk_param[c] in module segment
 * chunk_seg[c]; segment s owns chunks [seg_chunk0[s], seg_chunk0[s+1]). Only the chunks of the
 * parameters that take this step are listed (those with a gradient: torch's clip_grad_norm_
 * and Adam skip the others). max_norm > 0: per-segment L2 norm (fp64 chunk partials in
 * `partial`, fixed order) -> coef[s] = min(max_norm / (norm + 1e-6), 1), gradient scaled in
 * place; a non-finite norm propagates as in clip_grad_norm_ (nan norm -> nan coefficient, so
 * the whole segment becomes nan; infinite norm -> 0); max_norm <= 0: no clipping. param_step[active_params[i]] (device, one step count per
 * parameter as in torch's Adam) is incremented for i < n_active, then every listed element takes
 * one Adam step with *lr (device) and its parameter's bias corrections. Deterministic. */
int ured_adam_clip_step(float* param, float* grad, float* exp_avg, float* exp_avg_sq,
                        const long long* chunk_beg, const long long* chunk_end, const int* chunk_seg,
                        const int* chunk_param, int nchunks, const int* seg_chunk0, int nseg, float max_norm,
                        const float* lr, float* param_step, const int* active_params, int n_active,
                        double beta1, double beta2, double eps, double weight_decay, double* partial, float* coef,
                        void* stream);

/* Weight gradient of an edge layer (min(Cout, Kin) <= 4, the other <= 256):
 * out[co*ldo + ki] (+)= sum_m dY[m*ldd + co] * pro(X[m*ldx + ki]), deterministic (row-block
 * partials in ws, then a fixed-order tree per output). ws holds URED_SKINNY_WS_BLOCKS*Cout*Kin
 * floats. Replaces the MFMA wgrad for the 3-channel layers (a 128x128 tile would be mostly padding). */
#define URED_SKINNY_WS_BLOCKS 256
int ured_wgrad_skinny(const float* dY, int ldd, const float* X, int ldx, int Cout, int Kin, int M, int pro,
                      const float* pro_s, const float* pro_t, float* out, int ldo, int accumulate, float* ws,
                      void* stream);

/* Sum split-K partials: out[m][n] = (accumulate ? out : 0) + sum_z ws[z][m][n] (+ bias[n] if non-NULL);
 * fixed combine order (deterministic). */
int ured_splitk_reduce(const float* ws, int splits, int M, int N, float* out, int ldo, int accumulate,
                       const float* bias, void* stream);

/* BN forward finalize over the per-block partials of EPI_FWD (M rows, blocks of 128):
 * fp64 Chan merge -> mean, invstd = 1/sqrt(var_biased+eps), scale = gamma*invstd,
 * shift = beta - mean*scale; running stats (if non-NULL) updated in place with
 * momentum and the unbiased variance (torch.nn.BatchNorm1d semantics).
 * Row multiplicities (unique-row training): if group_w is non-NULL, each stored row of
 * group g = row / group_rows (group_rows a multiple of 128) stands for group_w[g] identical
 * rows of the batch; statistics are those of the expanded batch (count sum_g w_g*rows_g).
 * The same (group_w, group_rows) pair goes to the two backward calls below.
 * num_batches_tracked (nullable, int64 on the device) is incremented by one (the module's
 * counter update of a training-mode forward, folded into this launch). */
int ured_bn_fwd_finalize(const float* stat_ws, int M, int N, const float* gamma, const float* beta,
                         float eps, float momentum, float* running_mean, float* running_var,
                         float* mean, float* invstd, float* scale, float* shift,
                         const float* group_w, int group_rows, long long* num_batches_tracked, void* stream);

/* BN backward finalize over EPI_BNBWD partials: dbeta = sum g, dgamma = sum g*xhat
 * (fp64, fixed order; written, or added if accumulate) and the coefficients of
 * dY = coef_a*g + coef_b*(p - mean) + coef_c (see ured_bn_bwd_apply). */
int ured_bn_bwd_finalize(const float* bwd_ws, int M, int N, const float* gamma, const float* invstd,
                         float* dgamma, float* dbeta, int accumulate,
                         float* coef_a, float* coef_b, float* coef_c,
                         const float* group_w, int group_rows, void* stream);

/* ---- SyncBN (optional, cfg["sync_bn"]; csrc/syncbn.hip): the two finalizes above split
 * around a cross-rank exchange of fp64 per-column statistics, torch SyncBatchNorm semantics.
 * ured_bn_stats: the Chan merge of ured_bn_fwd_finalize stopped before normalising:
 *   out [3][N] = (weighted count, mean, M2) of this rank's rows.
 * ured_bn_finalize_stats: ured_bn_fwd_finalize's outputs from merged stats [3][N].
 * ured_bn_bwd_sums: out [3][N] = (sum g, sum g*xhat, weighted count) of this rank.
 * ured_bn_bwd_finalize_sums: dbeta / dgamma from `local` (written or added), the
 *   ured_bn_bwd_apply coefficients from `global` (the all-reduced sums and count). */
int ured_bn_stats(const float* stat_ws, int M, int N, const float* group_w, int group_rows, double* out,
                  void* stream);
int ured_bn_finalize_stats(const double* stats, int N, const float* gamma, const float* beta, float eps,
                           float momentum, float* running_mean, float* running_var, float* mean, float* invstd,
                           float* scale, float* shift, long long* num_batches_tracked, void* stream);
int ured_bn_bwd_sums(const float* bwd_ws, int M, int N, const float* group_w, int group_rows, double* out,
                     void* stream);
int ured_bn_bwd_finalize_sums(const double* local, const double* global, int N, const float* gamma,
                              const float* invstd, float* dgamma, float* dbeta, int accumulate, float* coef_a,
                              float* coef_b, float* coef_c, void* stream);

/* dY[m][n] = coef_a*g + coef_b*(p-mean) + coef_c with p = Y (ENC) or relu(Y) (RES, then
 * times (Y > 0)). Also writes per-128-row column partial sums of dY to colsum_ws[blk][N].
 * With group_w, G holds the multiplicity-summed gradient of each stored row and the
 * mean terms are scaled by the row's weight: dY = coef_a*g + w*(coef_b*(p-mean) + coef_c). */
int ured_bn_bwd_apply(const float* G, const float* Y, int M, int N, int ld, int res,
                      const float* mean, const float* coef_a, const float* coef_b, const float* coef_c,
                      float* dY, float* colsum_ws, const float* group_w, int group_rows, void* stream);

/* Max-pool finalize (TargetEncoder max_pool1d over each group of group_rows points of
 * relu(scale*Y+shift), simple_encoder.py:105; relu = 0: of scale*Y+shift, PointNet's
 * torch.max over bn3(conv3(x)), pointnet_utils.py:126-127): pooled[g][n] and the winning
 * row index argidx[g][n] (lowest row on ties). */
int ured_pool_finalize(const float* pool_ws, int M, int N, int group_rows, const float* scale,
                       const float* shift, int relu, float* pooled, int* argidx, void* stream);

/* Same result as EPI_FWD pooling + ured_pool_finalize for any group size (a direct scan of Y [M][N]). */
int ured_pool_rows(const float* Y, int M, int N, int group_rows, const float* scale, const float* shift,
                   int relu, float* pooled, int* argidx, void* stream);

/* out[m][n] = act(Y[m*ldy+n]*scale[n] + shift[n]), act = relu (relu != 0) or identity: a
 * BatchNorm(+ReLU) output materialised (PointNet pointfeat, pointnet_utils.py:120,124). */
int ured_bn_act(const float* Y, int M, int N, int ldy, const float* scale, const float* shift, int relu,
                float* out, int ldo, void* stream);

/* out[g][n] = sum_{m in [off[g], off[g+1])} X[m*ldx+n] (rows ascending); off == NULL means
 * fixed groups of group_rows rows. G groups. */
int ured_group_colsum(const float* X, int ldx, int N, const int* off, int group_rows, int G,
                      float* out, int ldo, void* stream);
/* As ured_group_colsum, with each group's rows cut into `splits` equal ranges summed by
 * separate workgroups into ws [G][splits][N], then the partials summed in split order
 * (deterministic; for few, long groups). splits == 1: ws may be NULL. */
int ured_group_colsum_split(const float* X, int ldx, int N, const int* off, int group_rows, int G, int splits,
                            float* ws, float* out, int ldo, void* stream);

/* ---------------- graph attention (DeformNet_MatchingNet) ---------------- */

/* Multi-head softmax attention over graph nodes, node-major layout
 * (replaces attention_graph/attention.py:8-19 as called by attention_gnn.py:20-32).
 * Row r of sample b: q + (b*n + r)*ldq, k/v + (b*m + r)*ld{k,v}; head h occupies columns
 * [h*d, (h+1)*d) (the reference's view(B, H, d, nodes) channel split).
 *   weights[b][h][i][j] = softmax_j(scale * <q_bi^h, k_bj^h>),  out_bi^h = sum_j weights * v_bj^h
 * weights [B*H*n*m] is written by the forward and read by the backward, which overwrites
 * dq [B,n,*], dk/dv [B,m,*] (may be column slices of one buffer). Limits: n, m <= 32,
 * d <= 128; every such shape runs forward and backward (the backward's LDS image reaches
 * 74,240 B at the maxima, above the 64 KB a launch may ask for by default: the library raises
 * the backward kernel's limit before the first launch that needs it). */
#define URED_ATTN_MAX_NODES 32
#define URED_ATTN_MAX_HEAD_DIM 128
int ured_attn_fwd(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv,
                  int B, int H, int n, int m, int d, float scale, float* out, int ldo, float* weights,
                  void* stream);
int ured_attn_bwd(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* weights,
                  const float* dout, int lddo, int B, int H, int n, int m, int d, float scale,
                  float* dq, int lddq, float* dk, int lddk, float* dv, int lddv, void* stream);

/* Up to URED_ATTN_MAX_SETS independent attention calls (e.g. the two node sets of one
 * DescriptorsSelfAttention layer, attention_gnn.py:120-127: desc0 and desc1 through the same module)
 * in ONE launch; each set is exactly the call above with its own fields (fwd: out / ldo / weights,
 * bwd: weights / dout / dq / dk / dv), so the results are those of separate calls, bitwise. */
#define URED_ATTN_MAX_SETS 2
typedef struct {
    const float* q; int ldq;
    const float* k; int ldk;
    const float* v; int ldv;
    int B, H, n, m, d;
    float scale;
    float* out; int ldo;            /* forward output */
    float* weights;                 /* [B*H*n*m]: written by the forward, read by the backward */
    const float* dout; int lddo;    /* backward only */
    float* dq; int lddq;
    float* dk; int lddk;
    float* dv; int lddv;
} UredAttnSet;
int ured_attn_fwd_sets(int nsets, const UredAttnSet* sets, void* stream);
int ured_attn_bwd_sets(int nsets, const UredAttnSet* sets, void* stream);

/* ---------------- graph-node layers (DeformNet_MatchingNet, node.hip) ----------------
 * Replace the node-level Conv1d(k=1) layers (in_proj_q/k/v, out_proj, the FeedForwardNet_norm
 * convs and param_decoder: network/deformation_net.py:61,90, attention_graph/attention_gnn.py:
 * 20-32,50-54, attention_graph/attention_utils.py:62-86), forward and both backward GEMMs,
 * and the BatchNorm1d of FeedForwardNet_norm (Conv -> ReLU -> BN).
 *
 * ured_node_gemm: C[m][n] (+)= epi( sum_k A(m,k) B(k,n) ), M rows of graph nodes (small), with
 *   A(m,k) = A [m*sam + k*sak]           for k <  k1
 *          = A2[m*sam2 + (k-k1)*sak2]    for k >= k1   (cat([x, message]) along K, read in place)
 *   B(k,n) = B [k*sbk + n*sbn]           for n <  n1 (W^T: sbk = 1, sbn = ldW; W: sbk = ldW, sbn = 1)
 *          = B2[k*sbk2 + (n-n1)*sbn2]    for n >= n1 when B2 != NULL (wgrad of cat([x, message]))
 *   v = sum + bias[n] + rowbias[(m/rdiv)*ldrb + n]; relu_out: v = max(v, 0);
 *   gate: v = gate[m*ldgate+n] > 0 ? v : 0; v += R[m*ldR+n] for n < R_ncols;
 *   accumulate: C += v, else C = v.
 * k1 >= K or k1 % 16 == 0. Nullable: A2, B2, bias, rowbias, gate, R. Deterministic (fixed split
 * and summation order).
 * kind URED_NODE_COLSUM (a bias gradient riding in the same batched launch): C[n] (+)= sum over
 * m < M of A[m*sam + n*sak], n < N (B, K unused). */
#define URED_NODE_GEMM 0
#define URED_NODE_COLSUM 1
typedef struct {
    int M, N, K;
    const float* A; long long sam, sak;
    const float* A2; long long sam2, sak2; int k1;
    const float* B; long long sbk, sbn;
    const float* B2; long long sbk2, sbn2; int n1;
    float* C; long long ldc; int accumulate;
    const float* bias;
    const float* rowbias; long long ldrb; int rdiv;
    int relu_out;
    const float* gate; long long ldgate;
    const float* R; long long ldR; int R_ncols;
    int kind;
} UredNodeGemmDesc;
int ured_node_gemm(const UredNodeGemmDesc* d, void* stream);
/* Up to URED_NODE_MAX_JOBS independent node GEMMs in one launch (no ordering between them). */
#define URED_NODE_MAX_JOBS 6
int ured_node_gemm_batch(const UredNodeGemmDesc* const* d, int n, void* stream);

/* BatchNorm1d over node sets: rows [off[s], off[s+1]) are one call of the module (the two node
 * sets of a self-attention layer share it: the reference calls it once per set, in order).
 * x = relu_in ? max(Y, 0) : Y. training: per-set batch mean / biased variance (fp64 sums),
 * running stats updated per set in order (unbiased variance, momentum), num_batches_tracked
 * (nullable) += nsets; eval: running stats. Writes mean/invstd [nsets][N] and
 * act[m*ld_act+n] = (x - mean) * invstd * gamma + beta.
 * SyncBN (training only): stats_out non-NULL -> ONLY write each set's local fp64 (count, mean,
 * M2) to stats_out [nsets][3][N] and return (nothing else is written); stats_in non-NULL -> use
 * those (cross-rank merged) per-set statistics instead of this call's rows (running stats
 * updated with the merged count's unbiased variance). */
#define URED_NODE_MAX_SETS 4
typedef struct {
    int N, nsets, off[URED_NODE_MAX_SETS + 1];
    const float* Y; long long ldy; int relu_in, training;
    const float* gamma; const float* beta;
    float* running_mean; float* running_var; long long* num_batches_tracked;
    float momentum, eps;
    float* mean; float* invstd;
    float* act; long long ld_act;
    double* stats_out; const double* stats_in;
} UredNodeBNDesc;
int ured_node_bn_fwd(const UredNodeBNDesc* d, void* stream);

/* Backward of ured_node_bn_fwd: G = d loss / d act -> dY (through the ReLU when relu_in),
 * dgamma / dbeta summed over the sets (written, or added if accumulate).
 * SyncBN: sums_out non-NULL -> ONLY write each set's local fp64 (sum g, sum g*xhat, count) to
 * sums_out [nsets][3][N] and return; sums_in non-NULL -> the input gradient uses those
 * (cross-rank summed) sums and counts, dgamma / dbeta stay this rank's local sums. */
typedef struct {
    int N, nsets, off[URED_NODE_MAX_SETS + 1];
    const float* G; long long ldg;
    const float* Y; long long ldy; int relu_in, training;
    const float* gamma; const float* mean; const float* invstd;
    float* dY; long long lddy;
    float* dgamma; float* dbeta; int accumulate;
    double* sums_out; const double* sums_in;
} UredNodeBNBwdDesc;
int ured_node_bn_bwd(const UredNodeBNBwdDesc* d, void* stream);


/* get_part's per-sample bookkeeping (engine/train.py:103-136, compute_aabbox dataset_utils.py:77-85)
 * in one launch (csrc/parts.hip): labels int64 [B,N] (part ids in [0,P)), x [B,N,3] ->
 * x_sorted [B,N,3] (points stably sorted by label), perm / inv_perm int64 [B,N], gid int32 [B*N]
 * (part slot b*P + rank of each sorted point), off int32 [B*P+1] (row offsets of the slots),
 * counts int64 [B,P], k int64 [B], mask float [B,P], rank_of_label int64 [B,P] (cumsum(present)-1),
 * present uint8 [B,P], aabb [B,P,6] by slot and param_def [B,P,6] by label value ((center,
 * half extent), 0 for absent labels). Replaces the per-part Python loop / torch.unique. */
int ured_build_parts(const long long* labels, const float* x, int B, int N, int P, float* x_sorted,
                     long long* perm, long long* inv_perm, int* gid, int* off, long long* counts,
                     long long* k, float* mask, long long* rank_of_label, unsigned char* present,
                     float* aabb, float* param_def, void* stream);

/* Partial (occluded) target clouds (csrc/occ.hip; the reference's dataset/gen_occ_point.py, and the
 * centring / random rotation of partnet_dataset.py:60-78) in one launch, one workgroup per sample:
 * x [B,N,3], labels / sem int64 [B,N], 16 <= N <= 4096, K = N / 2 points kept ->
 * mask int64 [B,K] (kept point indices, ascending), ori_point_occ [B,K,3] = x[mask], point_occ
 * [B,K,3] = R (x[mask] - occ_mean), labels_occ / sem_occ int64 [B,K], occ_mean [B,3], occ_rot
 * [B,3,3] (identity unless `rotate`), and the plan used: plan_i int32 [B,URED_OCC_PLAN_I] (mode
 * 0 ball / 1 random / 2 slice / 3 part, ncenter, 8 centre indices, slice centre index, part probe
 * index), plan_f [B,URED_OCC_PLAN_F] (slice direction, 3 angles in degrees). Randomness is a
 * stateless Philox-4x32-10 hash of (seed, step, sample, stream, counter) (exact function: the
 * header comment of csrc/occ.hip): the same arguments give the same bits on every call.
 * modes int32 [B] (optional device array; -1 = draw) or mode_all (-1 = none, else 0..3 for every
 * sample; not both) overrides the drawn mode; plan_i_in / plan_f_in (optional,
 * together, without modes / mode_all) replace the whole drawn plan (indices are clamped into the sample). */
#define URED_OCC_PLAN_I 12
#define URED_OCC_PLAN_F 6
int ured_occlude(const float* x, const long long* labels, const long long* sem, int B, int N,
                 unsigned long long seed, unsigned long long step, const int* modes, int mode_all,
                 const int* plan_i_in,
                 const float* plan_f_in, int rotate, long long* mask, float* ori_point_occ, float* point_occ,
                 long long* labels_occ, long long* sem_occ, float* occ_mean, float* occ_rot, int* plan_i,
                 float* plan_f, void* stream);

/* Several device-to-device copies in one launch (csrc/copy.hip): the HIP-graph step refreshes its
 * static input batch before each replay (engine/graph.py) with this instead of one blit per
 * tensor. dst[i][0, bytes[i]) = src[i][0, bytes[i]); regions must not overlap; 16-B moves where
 * both addresses and the size allow, else 4-B or 1-B moves for that item. */
#define URED_COPY_MAX 16
typedef struct { void* dst; const void* src; long long bytes; } UredCopyItem;
int ured_copy_batch(const UredCopyItem* items, int n, void* stream);

/* ---------------- set abstraction (csrc/group.hip) ---------------- */
/* The sampling and grouping primitives of PointNet++ (network/pointnet/pointnet2_utils.py:63-138).
 * Contract distance of all three: d = ((dx*dx) + (dy*dy)) + (dz*dz) in fp32, no FMA contraction.
 *
 * Farthest-point sampling (farthest_point_sample, :63-84). xyz [B,N,3], start DEVICE int32 [B]
 * (clamped into [0,N) on the device, never read on the host) -> idx_out int32 [B,npoint].
 * The reference's recurrence: dmin[j] starts at 1e10f; step i writes the current f to
 * idx_out[b,i], sets dmin[j] = d wherever d < dmin[j] (d to point f), and the next f is the lowest
 * index among the maxima of dmin. npoint > N is allowed (the recurrence stays defined).
 * Limits: 1 <= N <= URED_FPS_NMAX (one workgroup per cloud holds the cloud in registers: 1024
 * threads x 16 points), npoint >= 1, B <= 65535, B * npoint < 2^31. */
#define URED_FPS_NMAX 16384
int ured_fps(const float* xyz, const int* start, int B, int N, int npoint, int* idx_out, void* stream);
/* Ball query (query_ball_point, :87-107). xyz [B,N,3], new_xyz [B,S,3] -> idx_out int32
 * [B,S,nsample]: row s lists the first nsample indices j, ascending, with !(d(new_xyz[s], xyz[j])
 * > r2) (inclusive boundary); a shorter row is padded with its first index; a row without a hit
 * is N in every slot (the reference's value). Limits: N >= 1, nsample >= 1 (nsample > N is
 * allowed), r2 >= 0, B <= 65535, B * S * nsample * 3 < 2^31, B * N * 3 < 2^31. */
int ured_ball_query(const float* xyz, const float* new_xyz, int B, int N, int S, float r2, int nsample, int* idx_out,
                    void* stream);
/* Grouping (index_points + the centring and cat of sample_and_group, :122-134). idx int32 [B,S,K] ->
 * out [B*S*K, C] point-major, C = 3 + D: columns 0..2 = xyz[b,idx] - new_xyz[b,s] (one fp32
 * subtract), the rest = points[b,idx] (points [B,N,D]; NULL with D = 0). xyz and new_xyz may both
 * be NULL: a plain gather, C = D. An index outside [0,N) (the ball query's N) gives a zero row.
 * Limits: N, K >= 1, B <= 65535, B * S * K * (3 + D) < 2^31, B * N * max(D, 3) < 2^31. */
int ured_group_fwd(const float* xyz, const float* new_xyz, const float* points, const int* idx, int B, int N, int S,
                   int K, int D, float* out, void* stream);
/* Its backward, WRITTEN (every element of grad_xyz [B,N,3], grad_new_xyz [B,S,3] and grad_points
 * [B,N,D] is set): each element of grad_xyz / grad_points is the fp32 sum of its (s,k)
 * contributions in ascending (s,k) order, grad_new_xyz[b,s] = - sum_k grad_out[(b,s,k), 0:3];
 * rows whose index lies outside [0,N) contribute nothing. grad_xyz and grad_new_xyz go together
 * (NULL: grad_out has D columns); grad_points is NULL exactly when D = 0. No atomics; a second
 * run is bitwise identical. Limits as the forward's, and S * K < 2^31. */
int ured_group_bwd(const float* grad_out, const int* idx, int B, int N, int S, int K, int D, float* grad_xyz,
                   float* grad_new_xyz, float* grad_points, void* stream);

/* ---------------- feature propagation (csrc/interp.hip) ---------------- */
/* Inverse-distance interpolation of coarse features over the K nearest coarse points, with the skip
 * features in front (PointNetFeaturePropagation, pointnet2_utils.py:293-309). points2 [B,S,D2], idx
 * int32 [B,N,K] (rows of points2, in [0,S)), d2 [B,N,K] (their squared distances), points1 [B,N,D1]
 * (NULL with D1 = 0) -> out [B*N, D1 + D2] point-major: columns 0..D1-1 a copy of points1, then
 *   r_k = 1.0f / (d_k + 1e-8f), R = (r_0 + r_1) + r_2, w_k = r_k / R,
 *   out_c = ((w_0 * f_0c) + (w_1 * f_1c)) + w_2 * f_2c, f_k = points2[b, idx[b,n,k]]
 * in fp32, IEEE divisions, no FMA contraction (K = 2: two terms; K = 1: w_0 = 1 and out = f_0 bit
 * for bit). The weights go to w_out [B,N,K] for the backward. One launch.
 * Limits: 1 <= K <= 3, N >= 1, S >= 1, D2 >= 1, B <= 65535, B * N * (D1 + D2) < 2^31,
 * B * S * D2 < 2^31, N * K < 2^31. B = 0 is a no-op. */
int ured_interp_fwd(const float* points2, const int* idx, const float* d2, const float* points1, int B, int N, int S,
                    int K, int D1, int D2, float* out, float* w_out, void* stream);
/* Its backward from grad_out [B*N, D1 + D2], WRITTEN (every element of both outputs is set):
 *   grad_points2[b,s,c] = sum over the (n,k) with idx[b,n,k] = s of w[b,n,k] * grad_out[(b,n), D1 + c],
 *     in fp32 from 0 in ascending (n,k) order (a product, then an add); no atomics, a second run is
 *     bitwise identical;
 *   grad_d2[b,n,k] = -((r_k * w_k) * sum_{j != k} w_j * (A_k - A_j)), A_k = sum_c grad_out_c * f_kc
 *     (the gradient through the weights in the form that stays accurate where d_k = 0; K = 1: 0).
 * The gradient of points1 is the first D1 columns of grad_out (the caller's view). Limits as the
 * forward's. */
int ured_interp_bwd(const float* grad_out, const float* points2, const int* idx, const float* w, const float* d2, int B,
                    int N, int S, int K, int D1, int D2, float* grad_points2, float* grad_d2, void* stream);

/* ---------------- 3D-GCN graph convolution (csrc/gcn.hip) ---------------- */
/* Conv_surface, Conv_layer and Pool_layer of network/P_3DGC.py without their [B, V, n, S*C] tensors.
 * Activations are point-major fp32 rows [B*V, .]; idx int32 [B,V,n] holds rows of the same cloud.
 * An index outside [0,V) reads as a zero row (ured_gcn_dirs: a zero direction) and takes no
 * gradient. Limits of all entry points: V, C >= 1, 1 <= n (k) <= URED_GCN_NMAX (the winning slot is
 * stored as a uint8), 1 <= S <= URED_GCN_SMAX (a lane keeps its 3 * S support components in
 * registers), B <= 65535, B * V * (S + 1) * C < 2^31, B * V * n * 3 < 2^31. B = 0 is a no-op. */
#define URED_GCN_NMAX 255
#define URED_GCN_SMAX 8
/* get_neighbor_direction_norm (:60-69). vertices [B,V,3] -> out [B,V,n,3]:
 *   d = vertices[b, idx[b,v,j]] - vertices[b,v]; out = d / max(sqrt(((d.x*d.x) + (d.y*d.y)) + (d.z*d.z)), 1e-12f)
 * (IEEE sqrt and division); a coincident neighbour gives the zero vector. */
int ured_gcn_dirs(const float* vertices, const int* idx, int B, int V, int n, float* out, void* stream);
/* The fused convolution. dirn [B,V,n,3], sdn [3, S*C], feat [B*V, (S+1)*C] or NULL, idx [B,V,n] ->
 * out [B*V, C], slot uint8 [B*V, S, C]:
 *   theta = max(((d.x*a.x) + (d.y*a.y)) + (d.z*a.z), 0), d = dirn[b,v,j,:], a = sdn[:, s*C + c]
 *   with feat (Conv_layer, :136-163): m_s = max_j theta * feat[b, idx[b,v,j], C + s*C + c],
 *        out[b,v,c] = feat[b,v,c] + ((m_0 + m_1) + ... + m_{S-1})
 *   feat NULL (Conv_surface, :88-112): m_s = max_j theta, out[b,v,c] = (m_0 + m_1) + ... + m_{S-1}
 * in fp32 without FMA contraction; slot[b,v,s,c] is the lowest j that attains m_s. One launch. */
int ured_gcn_conv_fwd(const float* dirn, const float* sdn, const float* feat, const int* idx, int B, int V, int n, int S,
                      int C, float* out, unsigned char* slot, void* stream);
/* Its backward from grad_out [B*V, C], WRITTEN (every element of both outputs is set), with
 * j* = slot[b,v,s,c], theta* the forward's theta at j* (relu passes a gradient iff theta* > 0):
 *   grad_feat [B*V, (S+1)*C] (NULL exactly when feat is): columns 0..C-1 a copy of grad_out; element
 *     (b, r, C + s*C + c) the sum over the (v, j) with idx[b,v,j] = r and j = j* of
 *     grad_out[b,v,c] * theta*, in fp32 from 0 in ascending (v, j) order;
 *   grad_sdn [3, S*C]: element (k, s*C + c) the sum over the vertices with theta* > 0 of
 *     (grad_out[b,v,c] * f) * dirn[b,v,j*,k], f = feat[b, idx[b,v,j*], C + s*C + c] (1 without
 *     feat): ured_gcn_conv_bwd_parts(B, V) workgroups sum ranges of consecutive vertices (four
 *     interleaved sequences each, combined in a fixed order) into rows of ws, which are added in
 *     ascending order.
 * No atomics; a second run is bitwise identical. ws: ured_gcn_conv_bwd_parts(B, V) * 3 * S * C floats
 * (ws_floats: its size, checked); parts = clamp(ceil(B * V / URED_GCN_BWD_ROWS), 1, URED_GCN_BWD_PARTS).
 * Further limit: V * n < 2^31. Three launches (two without feat). */
#define URED_GCN_BWD_ROWS 16
#define URED_GCN_BWD_PARTS 512
int ured_gcn_conv_bwd_parts(int B, int V);
int ured_gcn_conv_bwd(const float* grad_out, const float* dirn, const float* sdn, const float* feat, const int* idx,
                      const unsigned char* slot, int B, int V, int n, int S, int C, float* grad_feat, float* grad_sdn,
                      float* ws, size_t ws_floats, void* stream);
/* Pool_layer's pooling for the sampled vertices only (:172-190). feat [B*V, C], idx int32 [B,V,k],
 * sample int32 [P] (vertex ids, the same for every cloud) -> out [B*P, C], slot uint8 [B*P, C]:
 *   out[b,p,c] = max_j feat[b, idx[b, sample[p], j], c], slot the lowest j that attains it.
 * A sample outside [0,V) gives a zero row and no gradient. Limits: V, C >= 1, 1 <= k <= URED_GCN_NMAX,
 * B <= 65535, B * V * C, B * P * C, B * V * k and P * k < 2^31. */
int ured_gcn_pool_fwd(const float* feat, const int* idx, const int* sample, int B, int V, int k, int P, int C, float* out,
                      unsigned char* slot, void* stream);
/* Its backward, WRITTEN: grad_feat[b,r,c] = the sum over the (p, j) with idx[b, sample[p], j] = r and
 * slot[b,p,c] = j of grad_out[b,p,c], in fp32 from 0 in ascending (p, j) order. No atomics. */
int ured_gcn_pool_bwd(const float* grad_out, const int* idx, const int* sample, const unsigned char* slot, int B, int V,
                      int k, int P, int C, float* grad_feat, void* stream);

/* ---------------- Vector-Neuron DGCNN layers (csrc/vn.hip) ---------------- */
/* get_graph_feature + VNLinearLeakyReLU, VNMaxPool, VNStdFeature's frame product and the feature-space
 * kNN of network/VN/ without the [B, 2C, 3, N, k] tensors of the torch composition. A VN feature is
 * point-major with the channel innermost, [B, N, 3, C] fp32 (so [B*N*3, C] is a GEMM operand); idx
 * int32 [B,N,k] holds rows of the same cloud; an index outside [0,N) reads as a zero row and takes no
 * gradient. fp32 without FMA contraction, IEEE sqrt and division. No float atomics anywhere; a
 * second run of any entry point is bitwise identical. B = 0 (rows = 0) is a no-op. */
#define URED_VN_KMAX 32      /* neighbours per point */
#define URED_VN_DMAX 256     /* dimensions of ured_vn_knn (the encoders use 3, 63 and 126) */
#define URED_VN_COMAX 384    /* output channels: a wave keeps 6 chunks of 64 channels in registers */
#define URED_VN_STAT_ROWS 16
#define URED_VN_PARTS 256
/* Partial rows of the BatchNorm workspaces: clamp(ceil(B * N / URED_VN_STAT_ROWS), 1, URED_VN_PARTS). */
int ured_vn_parts(int B, int N);
/* Self-kNN inside each cloud in D dimensions. x [B,N,D] -> idx int32 [B,N,K]: the K rows of the same
 * cloud nearest to row n, the row itself included, sorted by (distance, index):
 *   dist(n, i) = (...((0 + e_0*e_0) + e_1*e_1) + ...) + e_{D-1}*e_{D-1},  e_d = x[b,i,d] - x[b,n,d]
 * and of two candidates at the same distance the lower index comes first. ws: B * N * N floats (ws_floats:
 * its size, checked), the clouds' distance matrices, written by the first of the two launches (64 x 64
 * tiles through LDS) and read by the second (one wave per row, K rounds of a lexicographic minimum).
 * A row with fewer than K comparable distances (NaN input) ends in -1 entries. Limits: N >= 1,
 * 1 <= D <= URED_VN_DMAX, 1 <= K <= min(N, URED_VN_KMAX), B <= 65535, N <= 64 * 65535,
 * B * N * max(D, K) < 2^31. */
int ured_vn_knn(const float* x, int B, int N, int D, int K, int* idx, float* ws, size_t ws_floats, void* stream);
/* The normalise + directional leaky ReLU pair of VNLinearLeakyReLU (vn_layers.py:48-77, VNBatchNorm
 * :112-132) after its two linear maps, which the caller runs as one per-point GEMM:
 *   edge form  (idx != NULL; get_graph_feature, vn_dgcnn_util.py:20-47, + dim = 5): the maps act on
 *     [x_j - x_i, x_i], so W . edge = W_a x_j + (W_b - W_a) x_i and
 *     uv [B*N*3, 2W] = x [B*N*3, C] @ [Wf_a; Wd_a; Wf_b - Wf_a; Wd_b - Wd_a]^T, W = Co + Cd, columns
 *     [Uf (Co) | Ud (Cd) | Vf (Co) | Vd (Cd)];  p = Uf[b, idx[b,n,j]] + Vf[b,n], d = Ud[b, idx[b,n,j]] + Vd[b,n]
 *   point form (idx == NULL, k = 1; dim = 4): uv [B*N*3, W] = [P (Co) | D (Cd)], p = P[b,n], d = D[b,n]
 *   Cd = Co (map_to_dir per channel) or 1 (share_nonlinearity).
 * Per (b, n, j, c), p and d in R^3:
 *   nrm = sqrt(((p.x*p.x) + (p.y*p.y)) + (p.z*p.z)) + 1e-6f
 *   nb  = nrm * scale[c] + shift[c],  scale = gamma * invstd, shift = beta - mean * scale
 *   ph  = (p / nrm) * nb
 *   t   = ((ph.x*d.x) + (ph.y*d.y)) + (ph.z*d.z),  q = (((d.x*d.x) + (d.y*d.y)) + (d.z*d.z)) + 1e-6f
 *   mask = t >= 0,  o = mask ? ph : 0.2f * ph + 0.8f * (ph - (t / q) * d)
 *   pool_mean: out [B,N,3,Co] = (the sum of o over ascending j from 0) / k;  else out [B,N,k,3,Co] = o
 * mask uint8 [B,N,k,Co] is the branch taken. training: mean and biased variance of nrm over all
 * B*N*k edges per channel, summed in float64 (ured_vn_parts(B, N) workgroups over ranges of
 * consecutive points, four interleaved sequences each, combined in a fixed order, the partial rows
 * added in ascending order), invstd = 1 / sqrt(var + eps); running_mean / running_var (unbiased) move
 * by `momentum` and *num_batches_tracked grows by 1 as in nn.BatchNorm (each may be NULL); needs
 * B*N*k > 1. eval: mean / var are the running statistics. stat [4, Co] receives mean, invstd,
 * scale, shift (the backward reads it). ws: ured_vn_parts(B, N) * 2 * Co doubles (training only;
 * ws_doubles: its size, checked). Limits: N >= 1, 1 <= k <= URED_VN_KMAX, 1 <= Co <= URED_VN_COMAX,
 * B <= 65535, B * N * k * 6 * (Co + Cd) < 2^31. Three launches (two in eval). */
int ured_vn_act_fwd(const float* uv, const int* idx, int B, int N, int k, int Co, int Cd, int training, const float* gamma,
                    const float* beta, float* running_mean, float* running_var, long long* num_batches_tracked,
                    float momentum, float eps, int pool_mean, double* ws, size_t ws_doubles, float* stat, float* out,
                    unsigned char* mask, void* stream);
/* Its backward from grad_out (the shape of out), WRITTEN (every element of every output is set). The
 * branch is read from mask, not recomputed. With go the gradient of o (grad_out / k under pool_mean):
 *   mask: g_ph = go, g_d = 0;  else s = t / q, gs = -0.8f * (go . d), gt = gs / q:
 *         g_ph = go + gt * d,  g_d = ((-0.8f * s) * go + gt * ph) + (2 * -(gt * s)) * d
 *   g_nb = (g_ph . p) / nrm,  nhat = (nrm - mean) * invstd
 *   grad_beta [Co] = sum g_nb, grad_gamma [Co] = sum g_nb * nhat (float64 sums, the forward's order)
 *   g_nrm = -((g_ph . p) * nb) / (nrm * nrm) + scale * ((g_nb - m1) - nhat * m2), m1 / m2 the means
 *           of g_nb / g_nb * nhat over the edges in training and 0 in eval (coef [2, Co] receives them)
 *   g_p = g_ph * (nb / nrm) + g_nrm * (p / |p|)   (the second term is 0 at p = 0, as torch.norm's)
 * grad_uv (the shape of uv): the V (point form: all) columns of row (b,n) are the sums of g_p / g_d
 * over ascending j (a shared direction's g_d summed over the lane's channels in ascending order, then
 * across the wave by a fixed butterfly); the U columns of row (b,r) are the sums over the (n, j)
 * with idx[b,n,j] = r in ascending (n, j) order, read from edge_ws [B*N*k, 3, W], the per-edge
 * (g_p | g_d) that the call writes first (edge form only; edge_ws_floats: its size, checked).
 * ws as in the forward. Further limit: N * k < 2^31. Four launches (three in the point form). */
int ured_vn_act_bwd(const float* grad_out, const float* uv, const int* idx, const unsigned char* mask, int B, int N, int k,
                    int Co, int Cd, int training, int pool_mean, const float* stat, double* ws, size_t ws_doubles, float* coef,
                    float* edge_ws, size_t edge_ws_floats, float* grad_uv, float* grad_gamma, float* grad_beta, void* stream);
/* VNMaxPool (vn_layers.py:135-149) after its linear map. x, d [B,N,k,3,C] -> out [B,N,3,C], slot uint8
 * [B,N,C]: the j with the largest ((x.x*d.x) + (x.y*d.y)) + (x.z*d.z), the lowest j on a tie;
 * out[b,n,:,c] = x[b,n,slot,:,c]. Limits: N, C >= 1, 1 <= k <= URED_VN_KMAX, B * N * k * 3 * C < 2^31. */
int ured_vn_maxpool_fwd(const float* x, const float* d, int B, int N, int k, int C, float* out, unsigned char* slot,
                        void* stream);
/* Its backward, WRITTEN: grad_x[b,n,j,:,c] = j == slot[b,n,c] ? grad_out[b,n,:,c] : 0 (d takes no
 * gradient, as in the reference, whose index selection cuts it off). */
int ured_vn_maxpool_bwd(const float* grad_out, const unsigned char* slot, int B, int N, int k, int C, float* grad_x,
                        void* stream);
/* VNStdFeature's einsum('bijm,bjkm->bikm') (vn_layers.py:199). x [rows,3,C], z [rows,3,3] (z[r,j,kk]) ->
 *   out[r,kk,c] = ((x[r,0,c]*z[r,0,kk]) + (x[r,1,c]*z[r,1,kk])) + (x[r,2,c]*z[r,2,kk])
 * Backward, WRITTEN: grad_x[r,j,c] = ((g[r,0,c]*z[r,j,0]) + (g[r,1,c]*z[r,j,1])) + (g[r,2,c]*z[r,j,2]);
 * grad_z[r,j,kk] = sum_c x[r,j,c] * g[r,kk,c], per lane over c = lane, lane + 64, ... and then across
 * the wave by a fixed butterfly. Limits: C >= 1, rows * 3 * C < 2^31. */
int ured_vn_frame_fwd(const float* x, const float* z, int rows, int C, float* out, void* stream);
int ured_vn_frame_bwd(const float* grad_out, const float* x, const float* z, int rows, int C, float* grad_x, float* grad_z,
                      void* stream);

/* ---------------- PCN completion network (csrc/pcn.hip) ---------------- */
/* The pieces of models/pcn.py that are not GEMMs; activations point-major [rows][C] fp32.
 * ured_pcn_relu: out[i] = max(y[i], 0), or with g: out[i] = y[i] > 0 ? g[i] : 0 (n elements).
 * ured_pcn_pool_bwd: backward of pooled[grp][c] = max over the `rows` rows of group grp of Y [G*rows][C],
 *   win [G][C] the winning global row (lowest index on a tie): accumulate 0 WRITES every element of
 *   dY (g at the winner, 0 elsewhere); accumulate 1 adds g at the winners only. A winner outside its
 *   group is never written.
 * ured_pcn_fold_fwd: Y[((b*num_coarse + c)*scale + s)][ch] = (Gb[b][ch] + Pc[b*num_coarse + c][ch]) + Gs[s][ch]
 *   (the decoder's conv1 pre-activation; Gb [B][C] carries the bias).
 * ured_pcn_fold_bwd: with G = dH where Y > 0 else 0 (both [B*num_coarse*scale][C]):
 *   dPc[p][ch] = sum_s G[p*scale + s][ch] (s ascending), WRITTEN; ws[k][s][ch] = the sum of G[p*scale + s][ch]
 *   over the points p (ascending) of chunk k = p / chunk, WRITTEN ([ceil(B*num_coarse / chunk)][scale][C]).
 *   scale <= 16. No float atomics.
 * ured_pcn_center_fwd: out[r][k] = y[r][k] + cp[r / scale][k] over [B*num_coarse*scale][3].
 * ured_pcn_center_bwd: out[q][k] = sum_s dF[q*scale + s][k] (s ascending) (+ add[q][k]) over [B*num_coarse][3]. */
int ured_pcn_relu(const float* y, const float* g, long long n, float* out, void* stream);
int ured_pcn_pool_bwd(const float* g, const int* win, int G, int rows, int C, float* dY, int accumulate, void* stream);
int ured_pcn_fold_fwd(const float* Gb, const float* Pc, const float* Gs, int B, int num_coarse, int scale, int C, float* Y,
                      void* stream);
int ured_pcn_fold_bwd(const float* dH, const float* Y, int B, int num_coarse, int scale, int C, int chunk, float* dPc,
                      float* ws, void* stream);
int ured_pcn_center_fwd(const float* y, const float* cp, int B, int num_coarse, int scale, float* out, void* stream);
int ured_pcn_center_bwd(const float* dF, const float* add, int B, int num_coarse, int scale, float* out, void* stream);

/* ---------------- VRCNet self-attention encoder (csrc/vrc.hip) ---------------- */
/* The pieces of models/vrcnet.py:15-290 that are not GEMMs; activations point-major [B*N][C] fp32,
 * products and adds rounded separately, sums in the stated order, no float atomics, every output
 * element written. B <= 65535 and every element count below 2^31 throughout.
 *
 * ured_vrc_sa_fwd: the attention core of SA_module per point n of cloud b.
 *   P [B*N][2 rel + mid] = [x1 | x2p | x3p] (the three 1x1 convolutions of max(x, 0), per point),
 *   idx int32 [B][N][k] (rows of the same cloud; an index outside [0, N) reads as a zero row),
 *   Wa [ms][rel (k+1)], Wb [k ms][ms], bb [k ms], ms = mid / share_planes.
 *     u[i] = max(x1[n][i], 0) for i < rel; u[rel + r k + j] = max(x2p[idx[n][j]][r], 0)
 *     h[s] = max(sum_i Wa[s][i] u[i], 0): 64 interleaved partial sums (i = l, l + 64, .. ascending),
 *            combined by a butterfly over l (xor 32, 16, .., 1)
 *     w[t] = (sum_s Wb[t][s] h[s], s ascending) + bb[t], read as w[s][j] = w[s k + j]
 *     o[n][c] = max(sum_j w[c mod ms][j] x3p[idx[n][j]][c], 0), j ascending
 *   Writes o [B*N][mid], h [B*N][ms], w [B*N][k ms].
 *   Limits: 1 <= k <= min(32, N), rel <= 32, mid <= 128, ms <= 16, ms divides mid.
 * ured_vrc_sa_bwd: with G = go where o > 0 else 0 (written to gm [B*N][mid]):
 *   dw[n][s k + j] = sum over c = s, s + ms, .. of G[n][c] x3p[idx[n][j]][c]      (written, [B*N][k ms])
 *   dh[n][s] = (sum_t Wb[t][s] dw[n][t], t ascending) where h[n][s] > 0 else 0     (written, [B*N][ms])
 *   dP[n][r] = (sum_s Wa[s][r] dh[n][s]) where x1[n][r] > 0 else 0, r < rel
 *   dP[m][rel + r] = (sum over the entries idx[n][j] = m, ascending (n, j), of
 *                     sum_s Wa[s][rel + r k + j] dh[n][s]) where x2p[m][r] > 0 else 0
 *   dP[m][2 rel + c] = sum over the entries idx[n][j] = m, ascending (n, j), of G[n][c] w[n][(c mod ms) k + j]
 *   wa_ws[q][s][i] = sum over the points n of chunk q (n / chunk = q, ascending) of dh[n][s] u[n][i]
 *                    ([ceil(B*N / chunk)][ms][rel (k+1)]; the caller sums the chunks).
 *   Every element of dP is written; a point no row names gets 0; an index outside [0, N) takes no
 *   gradient. dWb = dw^T h and dbb = column sums of dw are left to the GEMM library.
 *
 * ured_vrc_sk_mean_fwd: s[b][c] = (sum_n sum_i max(y_i[b][n][c], 0)) / N for the m <= 4 branches y_i
 *   [B*N][C] (i ascending inside; 4 interleaved row sums n = g, g + 4, .. combined in ascending g).
 * ured_vrc_sk_mean_bwd: dy[b][n][c] = ds[b][c] / N where y[b][n][c] > 0 else 0 (one branch per call).
 * ured_vrc_sk_mix_fwd: out = sum_i a[b][i][c] max(y_i[b][n][c], 0) (i ascending), a [B][m][C]; relu != 0
 *   applies max(., 0) after it.
 * ured_vrc_sk_mix_bwd: G = g where (relu == 0 or out > 0) else 0; dy_i = a_i G where y_i > 0 else 0;
 *   da[b][i][c] = sum_n G max(y_i, 0) in the order of ured_vrc_sk_mean_fwd. `out` may be null when relu == 0.
 *
 * ured_vrc_pool_fwd: edge-preserved pooling. feat [B][N][C], p_idx int32 [B][S], pn_idx int32 [B][S][pk]:
 *   out[b*S + s][c] = feat[b][p_idx[b][s]][c]; out[b*S + s][C + c] = max_j feat[b][pn_idx[b][s][j]][c],
 *   slot[b][s][c] = the winning j, the lowest on a tie. An index outside [0, N) reads as a zero row.
 *   pk <= 32.
 * ured_vrc_pool_bwd: dfeat[b][m][c] = sum over s with p_idx[b][s] = m (ascending s) of g[b*S + s][c], then
 *   + sum over (s, j) with pn_idx[b][s][j] = m and slot[b][s][c] = j (ascending (s, j)) of g[b*S + s][C + c].
 *
 * ured_vrc_unpool_fwd: out[b*N + n][c] = ((w0 f0 + w1 f1) + w2 f2)[c] for c < D2, f_q = feat2[b][idx[b][n][q]],
 *   w = weight[b][n][q] as given (K <= 3 columns); out[b*N + n][D2 + c] = skip[b*N + n][c] for c < D1
 *   (skip null iff D1 = 0). The interpolation first, the skip features after it.
 * ured_vrc_unpool_bwd: dfeat2[b][m][c] = sum over the entries idx[b][n][q] = m, ascending (n, q), of
 *   weight[b][n][q] * g[b*N + n][c]; dskip = the last D1 columns of g. No gradient to idx or weight. */
#define URED_VRC_KMAX 32
#define URED_VRC_RELMAX 32
#define URED_VRC_MIDMAX 128
#define URED_VRC_MSMAX 16
#define URED_VRC_MMAX 4
#define URED_VRC_PKMAX 32
int ured_vrc_sa_fwd(const float* P, const int* idx, const float* Wa, const float* Wb, const float* bb, int B, int N, int k,
                    int rel, int mid, int ms, float* o, float* h, float* w, void* stream);
int ured_vrc_sa_bwd(const float* go, const float* o, const float* P, const int* idx, const float* Wa, const float* Wb,
                    const float* h, const float* w, int B, int N, int k, int rel, int mid, int ms, int chunk, float* gm,
                    float* dw, float* dh, float* dP, float* wa_ws, void* stream);
int ured_vrc_sk_mean_fwd(const float* y0, const float* y1, const float* y2, const float* y3, int m, int B, int N, int C,
                         float* s, void* stream);
int ured_vrc_sk_mean_bwd(const float* y, const float* ds, int B, int N, int C, float* dy, void* stream);
int ured_vrc_sk_mix_fwd(const float* y0, const float* y1, const float* y2, const float* y3, const float* a, int m, int B, int N,
                        int C, int relu, float* out, void* stream);
int ured_vrc_sk_mix_bwd(const float* g, const float* out, const float* y0, const float* y1, const float* y2, const float* y3,
                        const float* a, int m, int B, int N, int C, int relu, float* dy0, float* dy1, float* dy2, float* dy3,
                        float* da, void* stream);
int ured_vrc_pool_fwd(const float* feat, const int* p_idx, const int* pn_idx, int B, int N, int S, int pk, int C, float* out,
                      unsigned char* slot, void* stream);
int ured_vrc_pool_bwd(const float* g, const int* p_idx, const int* pn_idx, const unsigned char* slot, int B, int N, int S,
                      int pk, int C, float* dfeat, void* stream);
int ured_vrc_unpool_fwd(const float* feat2, const int* idx, const float* w, const float* skip, int B, int N, int S, int K,
                        int D2, int D1, float* out, void* stream);
int ured_vrc_unpool_bwd(const float* g, const int* idx, const float* w, int B, int N, int S, int K, int D2, int D1,
                        float* dfeat2, float* dskip, void* stream);

/* The decoder's expansion units (EF_expansion, Density_aware_Chamfer_Distance/utils/model_utils.py:137-166;
 * Folding, models/vrcnet.py:54-86). The 1x1 convolutions on [centre | neighbour] features commute with the
 * gather, so their two halves are per-point GEMMs and only these kernels run per edge.
 *
 * ured_vrc_ef_edge_fwd: P [B*N][2 W] = [centre half | neighbour half], idx int32 [B][N][k], G [B*N*k][W] or null:
 *   out[(n k + j)][c] = max((G[(n k + j)][c] + P[n][c]) + P[idx[n][j]][W + c], 0); without G the first add
 *   drops out. An index outside [0, N) reads as a zero neighbour row.
 *   Limits: 1 <= k <= min(32, N), W <= URED_VRC_OMAX * URED_VRC_RMAX.
 * ured_vrc_ef_edge_bwd: with M = g where out > 0 else 0 ([B*N*k][W]):
 *   dG = M (written when dG is not null); dP[n][c] = sum_j M[(n k + j)][c], j ascending;
 *   dP[m][W + c] = sum over the entries idx[n][j] = m, ascending (n, j), of M[(n k + j)][c].
 *   Every element of dP is written; a point no row names gets 0 in the neighbour half; an index outside
 *   [0, N) takes no gradient.
 * ured_vrc_ef_max_fwd: H [B*N*k*r][O] read as [n][j][s][c] (the rows of conv3 on the [B*N*k][O r] rows of
 *   conv2, a view of the same memory): out[(n r + s)][c] = max_j H[((n k + j) r + s)][c],
 *   slot[(n r + s)][c] = the winning j, the lowest on a tie. k <= 32, r <= URED_VRC_RMAX, O <= URED_VRC_OMAX.
 * ured_vrc_ef_max_bwd: dH[((n k + j) r + s)][c] = g[(n r + s)][c] where slot[(n r + s)][c] = j else 0.
 *
 * ured_vrc_fold_fwd: out[(n r + s)][c] = max(U[n][c] + T[s][c], 0), U [B*N][Co], T [r][Co]; r <= URED_VRC_RMAX.
 * ured_vrc_fold_bwd: with M = g where out > 0 else 0: dU[n][c] = sum_s M[(n r + s)][c], s ascending;
 *   ws[q][s][c] = sum over the points n of chunk q (n / chunk = q, ascending) of M[(n r + s)][c]
 *   ([ceil(B*N / chunk)][r][Co]; the caller sums the chunks). */
#define URED_VRC_CMAX 512
#define URED_VRC_OMAX 256
#define URED_VRC_RMAX 16
int ured_vrc_ef_edge_fwd(const float* G, const float* P, const int* idx, int B, int N, int k, int W, float* out, void* stream);
int ured_vrc_ef_edge_bwd(const float* g, const float* out, const int* idx, int B, int N, int k, int W, float* dG, float* dP,
                         void* stream);
int ured_vrc_ef_max_fwd(const float* H, int B, int N, int k, int r, int O, float* out, unsigned char* slot, void* stream);
int ured_vrc_ef_max_bwd(const float* g, const unsigned char* slot, int B, int N, int k, int r, int O, float* dH, void* stream);
int ured_vrc_fold_fwd(const float* U, const float* T, int B, int N, int r, int Co, float* out, void* stream);
int ured_vrc_fold_bwd(const float* g, const float* out, int B, int N, int r, int Co, int chunk, float* dU, float* ws,
                      void* stream);

/* Model's variational part (Density_aware_Chamfer_Distance/models/vrcnet.py:430-501).
 *
 * ured_vrc_latent_fwd: oq [B][2Z] (the posterior head's output), op [B][2Z] (the prior head's) or null,
 *   eps_q, eps_p [B][Z] standard-normal draws. With mu = o[:, :Z] and s = softplus(o[:, Z:]), torch's softplus
 *   (x > 20 ? x : log1p(exp(x))):
 *   training (op not null): z [2B][Z], rows 0..B-1 = mu_q + s_q eps_q, rows B..2B-1 = mu_p + s_p eps_p (the
 *     generator's input, no concatenation); kl_rec [B][Z] = KL(N(0, 1) || N(mu_p, s_p)); kl_g [B][Z] =
 *     KL(N(mu_p, s_p) || N(mu_q, s_q)); both as torch's kl_divergence, 0.5 (((r + t) - 1) - log r) with
 *     r = (s_a / s_b)^2 and t = ((mu_a - mu_b) / s_b)^2 for KL(a || b). Equal distributions give exactly 0.
 *   evaluation (op null): z [B][Z] = mu_q + s_q eps_q; eps_p, kl_rec and kl_g are not touched.
 * ured_vrc_latent_bwd: the same inputs and the cotangents dz ([2B][Z], or [B][Z] in the evaluation form),
 *   d_kl_rec, d_kl_g [B][Z], each of which may be null (= zero). Writes every element of d_oq [B][2Z] and, in the
 *   training form, of d_op [B][2Z]. kl_g sends gradient to the posterior only (the reference detaches the prior
 *   there), kl_rec to the prior only. The softplus derivative is z / (z + 1) with z = exp(x), and 1 above the
 *   threshold. Nothing is saved between forward and backward but the inputs.
 *   Limits: 1 <= Z <= URED_VRC_ZMAX, 1 <= B <= 65535, 2 B Z < 2^31.
 *
 * ured_vrc_gauss_fwd: x [n][Z], y [m][Z] -> K [n][m], K[i][j] = exp(-(sum_d (x[i][d] - y[j][d])^2 / Z) / Z) from
 *   direct differences (x_i == y_j gives exactly 1). The sum over d: lane l of one wave adds d = l, l + 64, ..
 *   ascending, then the 64 lane sums meet in a butterfly (xor 32, 16, .., 1); the order does not depend on the
 *   launch geometry. x and y may be the same memory.
 * ured_vrc_gauss_bwd: with w[i][j] = dK[i][j] K[i][j] and c = 2 / Z^2:
 *   dx[i][d] = sum_j (w[i][j] * -c) (x[i][d] - y[j][d]), j ascending;
 *   dy[j][d] = sum_i (w[i][j] *  c) (x[i][d] - y[j][d]), i ascending. Every element is written; no atomics.
 *   When x and y are the same memory the caller adds dx and dy.
 *   Limits: 1 <= n, m <= URED_VRC_GAUSS_MAX, 1 <= Z <= URED_VRC_ZMAX. */
#define URED_VRC_ZMAX 4096
#define URED_VRC_GAUSS_MAX 4096
int ured_vrc_latent_fwd(const float* oq, const float* op, const float* eps_q, const float* eps_p, int B, int Z, float* z,
                        float* kl_rec, float* kl_g, void* stream);
int ured_vrc_latent_bwd(const float* oq, const float* op, const float* eps_q, const float* eps_p, const float* dz,
                        const float* d_kl_rec, const float* d_kl_g, int B, int Z, float* d_oq, float* d_op, void* stream);
int ured_vrc_gauss_fwd(const float* x, const float* y, int n, int m, int Z, float* K, void* stream);
int ured_vrc_gauss_bwd(const float* x, const float* y, const float* K, const float* dK, int n, int m, int Z, float* dx,
                       float* dy, void* stream);

/* ---------------- loss head (csrc/loss.hip) ---------------- */
/* compute_cm_loss of the deformed shape `out` [B,S,3] and of its mirror image (x -> -x,
 * get_symmetric) against the same target x [B,N,3] (engine/train.py:288,302 ->
 * loss/chamfer_loss.py:13-30, the Shape_Measure ChamferLoss calls per sample and per part):
 *   prep   : A = [out; mirror(out)] [2B,S,3], X2 = [x; x], XS2 = [x_sorted; x_sorted] [2B,N,3] and
 *            the segment tables of ured_nn_seg_fwd: full family int32 [2B,4] (a = the first
 *            k_b*NP points of half-sample s, b = its x) and part family [2B*P,4] (chunk i < k_b of
 *            NP points vs the points of part i: off int32 [B*P+1] / counts int64 [B,P] of
 *            x_sorted, k int64 [B] parts per sample);
 *   reduce : the four scalars [full, part, mirror full, mirror part] from the two families' NN
 *            distances (dist_a_* [2B*S], dist_b_* [2B*N]); CD = mean(cost1) + mean(cost2), part
 *            CD = mean over the sample's parts, both averaged over B. ws: 3*2B*(P+1) floats;
 *            counter: a device uint that is 0 before the launch (it is left at 0); 2B <= 256 and
 *            2B(P+1) <= 8448, less where the device's LDS per workgroup cannot stage the
 *            workspace (the call is then refused, nothing is launched);
 *   grad   : d terms g4 [4] -> the per-distance upstream weights of ured_nn_seg_bwd (gid int32
 *            [B*N]: part slot of each sorted row) and ga [2B*S*3] zeroed for its accumulation;
 *   fold   : grad_out [B,S,3] = ga[:B] + mirror(ga[B:]).
 * Replace the per-sample / per-part Python loops, means and masks of the reference (and their
 * autograd) with 4 + 3 launches around the two NN launches. */
int ured_cd_pair_prep(const float* out, const float* x, const float* x_sorted, const long long* k,
                      const long long* counts, const int* off, int B, int S, int N, int P, int NP, float* A,
                      float* X2, float* XS2, int* segs_full, int* segs_part, void* stream);
int ured_cd_pair_reduce(const float* dist_a_full, const float* dist_b_full, const float* dist_a_part,
                        const float* dist_b_part, const long long* k, const long long* counts, const int* off,
                        int B, int S, int N, int P, int NP, float* ws, unsigned* counter, float* terms, void* stream);
int ured_cd_pair_grad(const float* g4, const long long* k, const long long* counts, const int* gid, int B, int S,
                      int N, int P, int NP, float* gd_a_full, float* gd_b_full, float* gd_a_part, float* gd_b_part,
                      float* ga, void* stream);
int ured_cd_pair_fold(const float* ga, int B, int S, float* grad_out, void* stream);

/* residual_retrieval_loss (loss/basic_loss.py:249-265: x -> out nearest neighbour knn [B,N]
 * relative to the sample's rows, terms mean_n sum|x + res - out[nn]| and mean_n sum|res|),
 * compute_pc_consistency(rec, x) and compute_pc_consistency_weighted(recon_src, src_points, mask)
 * (loss/basic_consistency_loss.py:4-22), the last over the U distinct source parts of the batch
 * (recu / ptsu [U,NP,3]; slot r of the R = B*P part slots holds part inv[r], weight mask[r]).
 * Forward -> terms [4]; backward: upstream g4 [4] -> dres, drec [B,N,3], drecu [U,NP,3].
 * ws: 3 * (ceil(B*N / 256) + U) floats. knn is not checked: it must lie in [0, S).
 * A call with U == 0 (R, recu, ptsu, inv, mask, drecu unused) returns terms 0-2 and dres / drec
 * as usual and terms[3] = nan, the reference's 0/0 of an empty weighted mean; so does a mask
 * that sums to 0, and then every row of drecu is nan as well (autograd's too, but for the rows
 * of a part that no slot refers to, which it leaves at 0). A part that no slot refers to, or
 * only masked slots, adds nothing to terms[3] and gets drecu rows of 0. */
typedef struct {
    int B, N, S, U, NP, R;
    const float* x; const float* out; const int* knn; const float* res; const float* rec;
    const float* recu; const float* ptsu; const long long* inv; const float* mask;
} UredPointLossDesc;
int ured_point_losses_fwd(const UredPointLossDesc* d, float* ws, unsigned* counter, float* terms, void* stream);
int ured_point_losses_bwd(const UredPointLossDesc* d, const float* g4, float* dres, float* drec, float* drecu,
                          void* stream);

/* compute_contrast_loss_loss (loss/contrast_loss.py:61-102): t [n,C] target part features,
 * s_all [n_all,C] source codes of every rank (this rank's rows start at s_off), src_labels int64
 * [n] (-1: row ignored, else its label is s_off + i); loss = CE(scale * norm(t) norm(s_all)^T).
 * Forward writes inv norms [n + n_all], lse [n], ws [2n] and loss [1]; backward (g: d loss)
 * writes dt [n,C] and, when ds is not NULL, ds [n,C] for this rank's rows (the other ranks' rows
 * of s_all are constants). Both need C % 4 == 0, 16-byte aligned t and s_all, n_all <= 4096 and
 * C + n_all (backward: 2C + n_all) floats within the device's LDS per workgroup; a call outside
 * that is refused and launches nothing. A batch whose rows are all ignored returns loss = nan
 * (0/0, as F.cross_entropy does) and dt = ds = 0. */
int ured_contrast_fwd(const float* t, const float* s_all, const long long* src_labels, int n, int n_all, int C,
                      int s_off, float scale, float* inv, float* lse, float* ws, unsigned* counter, float* loss,
                      void* stream);
int ured_contrast_bwd(const float* t, const float* s_all, const long long* src_labels, int n, int n_all, int C,
                      int s_off, float scale, const float* inv, const float* lse, const float* g, float* dt, float* ds,
                      void* stream);

/* loss_all = sum_i weights[i] * *terms[i] in order (engine/train.py:278-335), one thread; the
 * backward writes gterms[i] = weights[i] * g. */
#define URED_ASSEMBLE_MAX 16
int ured_loss_assemble(int K, const float* const* terms, const float* weights, float* out, void* stream);
int ured_loss_assemble_bwd(int K, const float* weights, const float* g, float* gterms, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* URED_HIP_H */
