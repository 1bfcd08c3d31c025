/* l3d_prnet.h -- entry points of libl3d_hip.so for PRNet (prnet.hip): the keypoint selection of KeyPointNet
 * (models/prnet.py, reference :218-243) with the channel means the temperature head starts from, and the soft correspondences of
 * both directions of the SVD head (:176-190) under a per-cloud temperature that lives on the device.
 * Same conventions as l3d_rpmnet.h and l3d_pointconv.h: device pointers, fp32, contiguous, asynchronous on `stream`, status codes
 * of l3d_status (null pointer / non-positive size -> -1, a shape the kernels are not built for -> -2, both before any launch).  No
 * float atomics, a fixed summation order: the same bits on every call, whatever the outputs held before. */
#ifndef L3D_PRNET_H
#define L3D_PRNET_H
#include "../l3d_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define L3D_PRNET_MAX_N 16384         /* points per cloud of l3d_prnet_keypoints: a cloud's keys live in one workgroup's LDS */
#define L3D_SOFTCORR_PAIR_MAX_C 512   /* channels of l3d_soft_correspondence_pair (a multiple of 16, at least 16) */

/* emb, emb_p [B,C,N] (emb_p NULL: zeros), xyz [B,3,N].  With e = emb + emb_p (one fp32 addition per element):
 *   key[b,i]  = sum_c e[b,c,i]^2      fp32, c ascending, every product rounded before it is added (no fused multiply-add)
 *   rank(i)   = the number of points j of the cloud with key[j] > key[i], or key[j] == key[i] and j < i; a NaN key is above every
 *               number (NaN keys among themselves: by index).  This is l3d_mask_select's rule.
 *   point i is selected iff rank(i) < K; the selected points in ASCENDING index order are s_0 < s_1 < ... < s_{K-1}
 *   idx   int64 [B,K]  = s_p                         (may be NULL)
 *   xyz_k [B,3,K]      = xyz[b,d,s_p]                (may be NULL)
 *   emb_k [B,C,K]      = e[b,c,s_p]                  (may be NULL)
 *   mean  [B,C]        = (sum_p e[b,c,s_p]) / K      fp32, ascending p in a fixed association: per chunk of 64 keypoints four chains
 *                                                    of 16, joined pairwise, the chunk sums added in ascending order with
 *                                                    Kahan's compensation term
 * K == N: nothing is ranked (the keys are not formed): s_p = p, emb_k = e, xyz_k = xyz.
 * 1 <= K <= N (K > N -> L3D_ERR_INVALID_ARG); N <= L3D_PRNET_MAX_N and B <= 65535, else L3D_ERR_UNSUPPORTED.  Any C >= 1. */
int l3d_prnet_keypoints(const float *emb, const float *emb_p, const float *xyz, int B, int C, int N, int K, int64_t *idx, float *xyz_k,
                        float *emb_k, float *mean, l3d_stream_t stream);

/* Bytes of `workspace` for l3d_soft_correspondence_pair.  0 in this build: the two directions are two slices of one grid and
 * nothing crosses workgroups; `workspace` may then be NULL. */
size_t l3d_soft_correspondence_pair_workspace_bytes(int B, int N, int M);

/* src_emb [B,C,N], tgt_emb [B,C,M], src [B,3,N], tgt [B,3,M], temperature [B] (device memory).  With
 * S_ij = sum_c src_emb[b,c,i] tgt_emb[b,c,j]  (v_mfma_f32_16x16x4_f32: an fp32 fma chain in ascending c) and
 * L_ij = S_ij (temperature[b] / sqrt(C)):
 *   corr_ab [B,3,N]:  corr_ab[b,:,i] = sum_j softmax_j(L_ij) tgt[b,:,j]        (may be NULL)
 *   corr_ba [B,3,M]:  corr_ba[b,:,j] = sum_i softmax_i(L_ij) src[b,:,i]        (may be NULL; not both)
 * Flash-style: the scores stay in the accumulators, a running maximum, sum and three weighted sums per query; keys in ascending
 * tiles of 64.  One launch serves both directions (grid slices); a NULL output's slice is not launched.
 * workspace: l3d_soft_correspondence_pair_workspace_bytes(B,N,M) bytes of scratch (see there).
 * C % 16 == 0, 16 <= C <= L3D_SOFTCORR_PAIR_MAX_C, B <= 65535; else L3D_ERR_UNSUPPORTED.  Any N, M >= 1. */
int l3d_soft_correspondence_pair(const float *src_emb, const float *tgt_emb, const float *src, const float *tgt, const float *temperature,
                                 int B, int C, int N, int M, void *workspace, float *corr_ab, float *corr_ba, l3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
