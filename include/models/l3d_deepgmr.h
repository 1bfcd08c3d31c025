/* l3d_deepgmr.h -- entry points of libl3d_hip.so for DeepGMR (deepgmr.hip): the rotation-invariant RRI features of its input
 * (data_utils/dataloaders.py:126-147, get_rri), the soft-assignment GMM fit (models/deepgmr.py:13-31, gmm_params) and the closed-form
 * registration of two mixtures (:34-54, gmm_register).  Same conventions as l3d_masknet2.h: device pointers, fp32, contiguous, every
 * call asynchronous on `stream`, status codes of l3d_status (null pointer / non-positive size -> -1, a shape the kernels are not
 * built for -> -2, both before any launch).  No float atomics: every kernel gives the same bits on every call. */
#ifndef L3D_DEEPGMR_H
#define L3D_DEEPGMR_H
#include "../l3d_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define L3D_RRI_MAX_K 64 /* neighbours per point of l3d_rri_features */
#define L3D_GMM_MAX_J 64 /* mixture components of l3d_gmm_params / l3d_gmm_register */

/* RRI features of xyz [B,N,3] over the neighbours idx [B,N,k] (int64, each in [0,N); values outside are clamped into it).
 * feat [B,N,4k], neighbour-major, (rp, rq, theta, phi) per neighbour a; channel_first = 1: feat [B,4k,N].
 *   rp = |p|, rq = |q_a|, dot = p/rp . q_a/rq, theta = acos(clamp(dot, -1, 1)), T_a = q_a - dot p (p NOT normalised, as :139),
 *   psi_ab = atan2((T_b x T_a) . p/rp, T_b . T_a) mod 2 pi, phi_a = min over b != a of psi_ab
 * which is the reference's second smallest over all b, since psi_aa = 0 and every psi >= 0.  xyz is used as given (the caller
 * centres it); a point at the origin gives NaN as it does in the reference.
 * A lane per (point, a), the point's T_b in LDS, a loop over b.  The geometry (norms, dot, T, the sine and cosine of psi) is
 * formed in fp64 and rounded once; acos in fp64; one fp32 atan2 per (a, b).
 * 2 <= k <= L3D_RRI_MAX_K, B <= 65535; else L3D_ERR_UNSUPPORTED.  No alignment requirement. */
int l3d_rri_features(const float *xyz, const int64_t *idx, int B, int N, int k, int channel_first, float *feat, l3d_stream_t stream);

/* GMM fit from soft assignments: logits [B,J,N] channel-first (as the last conv writes them), pts [B,N,3].
 *   gamma[b,n,:] = softmax_J(logits[b,:,n])              -> gamma_out [B,N,J], or NULL for none
 *   pi[b,j]  = mean_n gamma                              -> pi [B,J]
 *   mu[b,j]  = sum_n gamma p_n / (N pi)                  -> mu [B,J,3]
 *   var[b,j] = sum_n gamma |p_n - mu_j|^2 / (N pi)       -> var [B,J]      (the reference's sigma before `* eye`)
 * One workgroup per cloud and two passes over the logits: the moments about the COMPUTED mean, as the reference has them, never
 * the raw-moment form.  Sums run in fp64 in a fixed order (lane partials, a butterfly, the tiles in ascending order); gamma is
 * recomputed in the second pass by the same code, so the moments are the same bits with and without gamma_out.
 * 1 <= J <= L3D_GMM_MAX_J, any N >= 1, B <= 65535; else L3D_ERR_UNSUPPORTED.  No [B,N,J,3] tensor exists. */
int l3d_gmm_params(const float *logits, const float *pts, int B, int J, int N, float *gamma_out, float *pi, float *mu, float *var,
                   l3d_stream_t stream);

/* Closed-form registration of two mixtures with shared weights: pi_s [B,J], mu_s, mu_t [B,J,3], var_t [B,J] -> T [B,4,4].
 *   c_s = pi_s . mu_s, c_t = pi_s . mu_t, Ms = sum_j pi_j (mu_s_j - c_s) (mu_t_j - c_t)^T / var_t_j
 *   R = V diag(1, 1, det(V U^T)) U^T from Ms = U S V^T, t = c_t - R c_s, T = [R t; 0 0 0 1]
 * One wave per pair, a lane per component, fp64 sums (butterfly), the 3x3 SVD of svd.hip (svd3x3.h) in lane 0.  No host read.
 * 1 <= J <= L3D_GMM_MAX_J, B <= 65535; else L3D_ERR_UNSUPPORTED. */
int l3d_gmm_register(const float *pi_s, const float *mu_s, const float *mu_t, const float *var_t, int B, int J, float *T,
                     l3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
