/* l3d_rpmnet_match.h -- entry points of libl3d_hip.so for RPMNet's matching stage under autograd (rpmnet_match.hip): the slack
 * Sinkhorn of l3d_rpmnet.h with every iteration's potentials kept, and its backward from those potentials.  Conventions are
 * l3d_rpmnet.h's: device pointers, fp32 data, fp64 statistics, contiguous, every call asynchronous on `stream`, status codes of
 * l3d_status (null pointer / non-positive size -> -1, a shape the kernels are not built for -> -2, both before any launch).  No
 * atomics: the same bits on every call, whatever outputs and workspaces held before.
 *
 * The function.  A [B,J,K] is log_alpha padded with a slack row and column of zeros, u[J] = v[K] = 0, v_0 = 0, and for t = 1..n
 *   u_t[j] = logsumexp over k = 0..K of (A[j,k] - v_{t-1}[k])   for j < J
 *   v_t[k] = logsumexp over j = 0..J of (A[j,k] - u_t[j])       for k < K
 *   P = exp(A - u_n - v_n) [J,K],  r[j] = sum_k P[j,k],  w[j] = (P x)[j] / (r[j] + eps)  with x = xyz_ref [K,3].
 * The backward.  With the cotangents dP [J,K], dr [J], dw [J,3] and dAff [J,K] (each may be absent, not all of them):
 *   g[j] = dw[j] / (r[j] + eps),  c0[j] = dr[j] - g[j] . w[j],  G[j,k] = P[j,k] (dP[j,k] + c0[j] + g[j] . x[k])
 *   ubar_n[j] = -sum_k G[j,k],  vbar_n[k] = -sum_j G[j,k],  and for t = n..1
 *     Q_t[j,k] = exp(A[j,k] - u_t[j] - v_t[k]),      ubar_t[j] = (t == n ? ubar_n[j] : 0) - sum_{k<K} vbar_t[k] Q_t[j,k]
 *     R_t[j,k] = exp(A[j,k] - v_{t-1}[k] - u_t[j]),  vbar_{t-1}[k] = -sum_{j<J} ubar_t[j] R_t[j,k]      (not needed for t = 1)
 *   dA[j,k] = dAff[j,k] + G[j,k] + sum_t (vbar_t[k] Q_t[j,k] + ubar_t[j] R_t[j,k])          for j < J, k < K
 * The slack row and column take part in the forward's sums and receive no gradient.  Every exponential, P itself and every sum is
 * fp64, from the fp32 log_alpha and the fp64 potentials; each output is rounded once.  This is the derivative of the fp64 function;
 * it differs from the derivative of the fp32-rounded outputs of the forward by no more than that rounding.
 * Limits of every entry point: J, K >= 1, n_iters >= 0, B <= 65535; else L3D_ERR_UNSUPPORTED.  No alignment requirement beyond the
 * element types'. */
#ifndef L3D_RPMNET_MATCH_H
#define L3D_RPMNET_MATCH_H
#include "../l3d_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* l3d_sinkhorn_slack with its potentials as an output: potentials fp64 [n_iters, B, J + K], per (t, cloud) the J values of u_t and
 * then the K values of v_t, every element written (n_iters = 0: no element; the pointer is not read and may be NULL).  log_perm,
 * perm, rowsum and weighted are bit for bit l3d_sinkhorn_slack's (the same sums in the same order; any of them may be NULL, not
 * all; weighted needs xyz_ref).  2 n_iters + 1 launches. */
int l3d_sinkhorn_slack_keep(const float *log_alpha, int B, int J, int K, int n_iters, const float *xyz_ref, float eps, float *log_perm,
                            float *perm, float *rowsum, float *weighted, double *potentials, l3d_stream_t stream);

/* The backward above.  log_alpha [B,J,K], potentials as l3d_sinkhorn_slack_keep wrote them (n_iters = 0: may be NULL), xyz_ref
 * [B,K,3] or NULL, the cotangents d_perm [B,J,K], d_rowsum [B,J], d_weighted [B,J,3], d_affinity [B,J,K], each or NULL: at least one
 * must be given and d_weighted needs xyz_ref, else L3D_ERR_INVALID_ARG.
 * dist [B,J,K], beta [B], alpha [B]: all three or none (else L3D_ERR_INVALID_ARG).  They state that log_alpha = -beta (dist - alpha)
 * per cloud, and the gradient is folded through that:
 *   with them     d_out [B,J,K] = dD = -beta dA;  d_beta[b] = -sum_{j,k} dA (dist - alpha),  d_alpha[b] = beta[b] sum_{j,k} dA, from
 *                 per-row fp64 partials added in ascending row order; either of d_beta, d_alpha [B] may be NULL, and with both NULL
 *                 no partial is formed
 *   without them  d_out = dA; d_beta and d_alpha must be NULL.
 * `workspace`: SCRATCH of l3d_sinkhorn_backward_workspace_bytes(B, J, K, n_iters) bytes, 8-byte aligned: c0 and g per row, ubar_t
 * and vbar_t of every t, the fold's partials.
 * Launches: one row pass (two sweeps of its row: r and P x, from them c0 and g, then ubar_n), one column
 * pass (vbar_n), 2 n_iters - 1 alternating row and column reductions (a wave per row; 64 columns per workgroup), one output pass
 * (Q_n is P: 2 n_iters exponentials per element), and with d_beta or d_alpha one launch that adds the partials.  n_iters = 0: the
 * row pass and the output pass, dA = dAff + G.  log_alpha is read once per pass, d_perm by the row pass, the column pass and the
 * output pass; nothing of size [B,J+1,K+1] exists.  Where K is a multiple of 4 and the [B,J,K] pointers a row kernel touches lie
 * on 16 bytes it moves 16 bytes per lane, else it takes its scalar route (other lanes sum other columns: the last bits differ). */
size_t l3d_sinkhorn_backward_workspace_bytes(int B, int J, int K, int n_iters);
int l3d_sinkhorn_slack_backward(const float *log_alpha, const double *potentials, int B, int J, int K, int n_iters, const float *xyz_ref,
                                float eps, const float *d_perm, const float *d_rowsum, const float *d_weighted, const float *d_affinity,
                                const float *dist, const float *beta, const float *alpha, float *d_out, float *d_beta, float *d_alpha,
                                void *workspace, l3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
