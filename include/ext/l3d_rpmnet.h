/* l3d_rpmnet.h -- entry points of libl3d_hip.so for RPMNet and PPFNet (rpmnet.hip): the grouped point-pair features of PPFNet's
 * input (utils/ppfnet_util.py:173-244), a pointwise convolution whose operand carries the previous layer's GroupNorm + ReLU and
 * whose epilogue gathers the next GroupNorm's statistics (models/ppfnet.py:15-49), the slack Sinkhorn normalisation
 * (models/rpmnet.py:157-202) and the weighted Kabsch step (:221-254).
 * Same conventions as models/l3d_deepgmr.h: device pointers, fp32, contiguous, every call asynchronous on `stream`, status codes of
 * l3d_status (null pointer / non-positive size -> -1, a shape the kernels are not built for -> -2, both before any launch).  No
 * float atomics: every kernel gives the same bits on every call, whatever its outputs and workspaces held before.
 *
 * include/ext/ is the OPEN header table: a later model adds its header here (learning3d_amd/_lib.py reads every *.h of this
 * directory into EXT_PROTOTYPES); no test pins this table's size or contents. */
#ifndef L3D_RPMNET_H
#define L3D_RPMNET_H
#include "../l3d_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define L3D_PPF_MAX_K 64          /* neighbours per point of l3d_ppf_group */
#define L3D_GN_CONV_MAX_COUT 256  /* output channels of l3d_gn_conv (a multiple of 16) */
#define L3D_GN_CONV_MAX_CIN 4096  /* input channels of l3d_gn_conv */
#define L3D_GN_CONV_PARTS 64      /* most per-workgroup partial moments per (cloud, channel) in l3d_gn_conv's workspace */

/* PPFNet's grouped input.  xyz, normals [B,N,3] (normals NULL: zeros, a cloud without normals), idx int64 [B,N,K], each in
 * [0,N) (values outside are clamped into it) -> feat [B,10,K,N], channel-first as the pre-pool convolutions read it:
 *   0-2  the centre's xyz, the same for every k
 *   3-5  d = xyz[idx] - centre
 *   6-9  angle(n_r, d), angle(n_i, d), angle(n_r, n_i), |d|  with angle(a, b) = atan2(|a x b|, a . b), n_r the centre's normal
 *        and n_i the neighbour's
 * A padded slot (idx equal to the centre) gives exact zeros in channels 3-9.  d, the cross products, their norms, the dot
 * products and atan2 are formed in fp64 from the fp32 inputs and rounded once.  A lane per (n, k), lanes along n.
 * 1 <= K <= L3D_PPF_MAX_K, B <= 65535; else L3D_ERR_UNSUPPORTED. */
int l3d_ppf_group(const float *xyz, const float *normals, const int64_t *idx, int B, int N, int K, float *feat, l3d_stream_t stream);

/* Pointwise convolution between two GroupNorms.  x [B,Cin,P], w [Cout,Cin], bias [Cout] or NULL, in_a / in_s [B,Cin] or both NULL:
 *   u = x                                   when in_a is NULL
 *   u = max(0, in_a[b,ci] x + in_s[b,ci])   else: the previous layer's GroupNorm and ReLU, applied as the operand is loaded
 *   y[b,co,p] = bias[co] + sum_ci w[co,ci] u[b,ci,p]        (v_mfma_f32_16x16x4_f32: an fp32 fma chain in ascending ci)
 * pool == 0: y [B,Cout,P] is written.
 * pool == K > 0: P = K N' with p = k N' + n (P % K != 0 -> L3D_ERR_INVALID_ARG).  ymax, ymin [B,Cout,N'] are the extremes over k of
 *   y; y may be NULL and is then never stored.  Both extremes, because the next GroupNorm's scale can be negative: the pooled
 *   activation is max(0, a (a >= 0 ? ymax : ymin) + s).
 * Always: moments fp64 [B,Cout,2] = (sum_p y, sum_p y^2) of the fp32 y, from per-workgroup fp64 partials in `workspace`
 * (l3d_gn_conv_workspace_bytes(B, Cout, P) bytes, 8-byte aligned), reduced in ascending order by a second launch.
 * Raw moments are enough here because they are carried in fp64: var = E y^2 - (E y)^2 loses (mean / deviation)^2 2^-53 of its
 * value to cancellation, which stays below fp32's 2^-24 while |mean| / deviation < 2^14 (about 2e4).  A convolution's output
 * in front of a GroupNorm has a ratio of order one; past 2e4 a two-pass or Welford form would be needed.
 * Cout % 16 == 0, 16 <= Cout <= L3D_GN_CONV_MAX_COUT, 1 <= Cin <= L3D_GN_CONV_MAX_CIN (any value: the channel tile is padded with
 * zeros in LDS, not in memory), any P >= 1, any N' >= 1, B <= 65535; else L3D_ERR_UNSUPPORTED.  No alignment requirement beyond
 * the element types'. */
int l3d_gn_conv(const float *x, const float *in_a, const float *in_s, const float *w, const float *bias, int B, int Cin, int Cout,
                int P, int pool, float *y, float *ymax, float *ymin, double *moments, void *workspace, l3d_stream_t stream);
size_t l3d_gn_conv_workspace_bytes(int B, int Cout, int P);

/* GroupNorm as a per-(cloud, channel) affine map, from l3d_gn_conv's moments [B,C,2]: per (b, group) the mean and the biased
 * variance over the group's C / groups channels and `count` positions in fp64, rstd = 1 / sqrt(var + eps), then
 *   a[b,c] = gamma[c] rstd,  s[b,c] = beta[c] - mean a[b,c]       (fp64, rounded once)
 * C % groups == 0, B <= 65535; else L3D_ERR_UNSUPPORTED. */
int l3d_gn_affine(const double *moments, const float *gamma, const float *beta, int B, int C, int groups, int count, float eps,
                  float *a, float *s, l3d_stream_t stream);

/* Sinkhorn with a slack row and column (sinkhorn(..., slack=True), :176-202) on log_alpha [B,J,K].  The padded matrix is never
 * written: each half step subtracts a constant per row or per column, so after n iterations the result is A[j,k] - u[j] - v[k]
 * with A the zero-padded input, u[J] = v[K] = 0 and, per iteration,
 *   u[j] = logsumexp over k = 0..K of (A[j,k] - v[k])   for j < J,   then
 *   v[k] = logsumexp over j = 0..J of (A[j,k] - u[j])   for k < K.
 * Only the potentials live in `workspace` (fp64, l3d_sinkhorn_workspace_bytes(B, J, K) bytes, 8-byte aligned); log_alpha is read
 * once per half step.  Every logsumexp is a one-pass running (maximum, sum) in fp64, so inputs of +-200 neither overflow nor
 * underflow to -inf.  2 n_iters + 2 plain stream-ordered launches.  The last pass writes whichever outputs are not NULL:
 *   log_perm [B,J,K];  perm = exp(log_perm);  rowsum [B,J] = sum_k perm;  weighted [B,J,3] = (perm @ xyz_ref) / (rowsum + eps)
 * (weighted needs xyz_ref [B,K,3], else L3D_ERR_INVALID_ARG; at least one output must be given).  n_iters = 0 returns the input.
 * log_alpha must be finite: an entry of -inf against an empty running state is -inf - -inf, a NaN.
 * J, K >= 1, n_iters >= 0, B <= 65535; else L3D_ERR_UNSUPPORTED. */
int l3d_sinkhorn_slack(const float *log_alpha, int B, int J, int K, int n_iters, const float *xyz_ref, float eps, float *log_perm,
                       float *perm, float *rowsum, float *weighted, void *workspace, l3d_stream_t stream);
size_t l3d_sinkhorn_workspace_bytes(int B, int J, int K);

/* compute_rigid_transform (:221-254): a, b [B,M,3], weights [B,M] -> T [B,3,4] = [R | t] with T a = b in the weighted least-squares
 * sense.  wn = w / (sum w + eps); c_a = sum wn a, c_b = sum wn b; cov = sum wn (a - c_a)(b - c_b)^T, all sums in fp64 in a fixed
 * order; cov = U S V^T by the 3x3 SVD of svd3x3.h; R = V U^T, with the column of V of the smallest singular value negated when
 * det(V U^T) < 0, as the reference chooses; t = c_b - R c_a.  One workgroup per cloud; no host read, no assertion.
 * M >= 1, B <= 65535; else L3D_ERR_UNSUPPORTED. */
int l3d_rigid_transform_weighted(const float *a, const float *b, const float *weights, int B, int M, float eps, float *T,
                                 l3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
