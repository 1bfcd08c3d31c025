/* l3d_rpmnet_train.h -- entry points of libl3d_hip.so for the backward of PPFNet's conv -> GroupNorm -> ReLU (-> maximum over the
 * neighbours) layers (rpmnet_train.hip): what models/ppfnet.py's autograd function runs between l3d_gn_conv (dgrad), l3d_wgrad and
 * l3d_channel_stats.  Conventions are l3d_rpmnet.h's: device pointers, fp32 data, fp64 statistics, contiguous, every call
 * asynchronous on `stream`, status codes of l3d_status (null pointer / non-positive size -> -1, a shape the kernels are not built
 * for -> -2, both before any launch).  No atomics: the same bits on every call, whatever outputs and workspaces held before.
 *
 * One layer, in the notation of every entry point below.  y [B,C,P] is the convolution's fp32 output (l3d_gn_conv's y), in_a / in_s
 * [B,C] the GroupNorm as l3d_gn_affine gave it, stat fp64 [B,groups,2] = (mean, rstd) per (cloud, group):
 *   h = fmaf(in_a, y, in_s)      the single-rounded value l3d_gn_conv forms as it loads its operand
 *   u = max(0, h)                the layer's output
 *   zhat = (y - mean) rstd       fp64
 *   g = du [h > 0]               du the gradient that arrives at u
 * The gradient arrives in one of two forms:
 *   dense  (K == 0, widx NULL): du [B,C,P];
 *   pooled (K >= 1): the layer's output went through the maximum over k of P = K N' positions p = k N' + n.  du is [B,C,N'], the
 *           gradient at the pooled value, and lives at p = widx[b,c,n] N' + n alone; every other position's du is zero.  The dense
 *           scatter is never formed.  P % K != 0 -> L3D_ERR_INVALID_ARG.  A widx entry >= K is read as K - 1.
 * A zero or negative GroupNorm weight is ordinary input: nothing divides by gamma or by in_a.
 * Limits of every entry point: C % groups == 0, 0 <= K <= L3D_PPF_MAX_K, B <= 65535, C <= 65535, P <= L3D_GN_BWD_MAX_P (the kernels
 * index a row in int, a block past its end included); else L3D_ERR_UNSUPPORTED.  Any P from 1 to that limit, any N' >= 1.  No
 * alignment requirement beyond the element types': where P (pooled: N') is a multiple of 4 and the [B,C,P] / [B,C,N'] pointers lie
 * on 16 bytes (widx on 4) the streaming kernels move 16 bytes per lane, else they take their scalar route. */
#ifndef L3D_RPMNET_TRAIN_H
#define L3D_RPMNET_TRAIN_H
#include "../l3d_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define L3D_GN_BWD_CHUNK 8192     /* positions of one (cloud, channel) row per workgroup of l3d_gn_backward_stats */
#define L3D_GN_BWD_MAX_P 2147475455 /* most positions per row: INT_MAX - L3D_GN_BWD_CHUNK */

/* stat[b,grp] = (mean, rstd) of the GroupNorm over `count` positions and C / groups channels from l3d_gn_conv's moments [B,C,2]:
 * the same sums in the same order as l3d_gn_affine, so these are the very values in_a and in_s were rounded from. */
int l3d_gn_mean_rstd(const double *moments, int B, int C, int groups, int count, float eps, double *stat, l3d_stream_t stream);

/* The pooling winner of a pooled layer: widx[b,c,n] = the lowest k at which y[b,c,k N' + n] attains its maximum over k where
 * in_a[b,c] >= 0, its minimum else -- the position whose value the forward's (in_a >= 0 ? ymax : ymin) is.  y [B,C,K N'], widx [B,C,N'].
 * 1 <= K <= L3D_PPF_MAX_K. */
int l3d_gn_pool_winner(const float *y, const float *in_a, int B, int C, int K, int NP, unsigned char *widx, l3d_stream_t stream);

/* u = max(0, fmaf(in_a, y, in_s)) [B,C,P]: a layer's output written out, the second operand of the next layer's l3d_wgrad. */
int l3d_gn_relu(const float *y, const float *in_a, const float *in_s, int B, int C, int P, float *u, l3d_stream_t stream);

/* part fp64 [B,C,2] = (S1, S2) = (sum_p g, sum_p g zhat) per (cloud, channel); pooled: sums over n of the pooled gradient alone.
 * A workgroup sums L3D_GN_BWD_CHUNK positions of a row in a fixed order; a row of more than one chunk goes through `workspace`
 * (SCRATCH of l3d_gn_backward_workspace_bytes(B, C, P) bytes, 8-byte aligned, required for every P), its chunks added in
 * ascending order by a second launch. */
size_t l3d_gn_backward_workspace_bytes(int B, int C, int P);
int l3d_gn_backward_stats(const float *du, const unsigned char *widx, int K, const float *y, const float *in_a, const float *in_s,
                          const double *stat, int B, int C, int groups, int P, double *part, void *workspace, l3d_stream_t stream);

/* The group reduction, one launch.  With n = (C / groups) count and `count` = P:
 *   m[b,grp] = (M1, M2) = (sum_{c in grp} gamma_c S1[b,c] / n, sum_{c in grp} gamma_c S2[b,c] / n)         fp64 [B,groups,2]
 *   dbeta[c] = sum_b S1[b,c],  dgamma[c] = sum_b S2[b,c]      clouds added in cloud order in fp64, rounded once; either may be NULL */
int l3d_gn_backward_reduce(const double *part, const float *gamma, int B, int C, int groups, int count, double *m, float *dgamma,
                           float *dbeta, l3d_stream_t stream);

/* dz[b,c,p] = rstd (gamma_c g - M1 - zhat M2), evaluated in fp64 and rounded once: the gradient at y, dense [B,C,P] in both forms. */
int l3d_gn_backward_apply(const float *du, const unsigned char *widx, int K, const float *y, const float *in_a, const float *in_s,
                          const double *stat, const float *gamma, const double *m, int B, int C, int groups, int P, float *dz,
                          l3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
