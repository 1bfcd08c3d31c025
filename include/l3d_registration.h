/* l3d_registration.h -- entry points of libl3d_hip.so for the iterative registration models (PointNetLK, iPCRNet): what runs
 * BETWEEN two PointNet passes of their loops (registration.hip).  Same conventions as l3d_hip.h: device pointers, fp32 unless
 * said otherwise, every call asynchronous on `stream`, status codes of l3d_status (null pointer / non-positive size -> -1,
 * a shape the kernels are not built for -> -2, both before any launch). */
#ifndef L3D_REGISTRATION_H
#define L3D_REGISTRATION_H
#include "l3d_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Pose + first layer (se3.transform, ops/se3.py:112-122, then conv1 (+BN, +ReLU) of models/pointnet.py:25-46):
 *   q[b,t,n] = R[b,t] cloud[b,n] + p[b,t]   formed in fp32, ((r0 x + r1 y) + r2 z) + p
 *   y[b T + t, c, n] = act(scale[c] (w1[c] . q) + shift[c])        [B T, C1, N], what l3d_pointwise_conv reads next
 *   posed[b T + t, n, :] = q                                        (optional)
 * cloud [B,N,3]; the transforms are EITHER T [B,Tn,4,4] OR, with T == NULL, the 6 finite-difference transforms exp(-dt[k] e_k)
 * of approx_Jic (models/pointnetlk.py:122-126) made from dt [6] inside the launch (Tn must be 6).  w1 [C1,3]; scale, shift [C1]
 * or NULL; y or posed may be NULL (not both).  C1 % 16 == 0, C1 <= 1024, B Tn <= 65535. */
int l3d_reg_pose_first_layer(const float *cloud, const float *T, const float *dt, int B, int Tn, int N, const float *w1,
                             const float *scale, const float *shift, int C1, int relu, float *y, float *posed,
                             l3d_stream_t stream);

/* Finite-difference Jacobian -> pseudo-inverse (approx_Jic + compute_inverse_jacobian, models/pointnetlk.py:109-152), one
 * workgroup per cloud: J[c][k] = (f0[c] - f[k][c]) / dt[k], H = J^T J and H^-1 (Gauss-Jordan, partial pivoting) in fp64,
 * pinv [B,6,K] = H^-1 J^T rounded to fp32 once.  f0 [B,K], f [B,6,K], dt [6].  singular: int32 [1 + B], IN-OUT, zeroed by the caller;
 * an exactly zero pivot sets singular[1 + b] and singular[0] (and that cloud's pinv to 0) where torch.inverse raises. */
int l3d_reg_jac_pinv(const float *f0, const float *f, const float *dt, int B, int K, float *pinv, int32_t *singular,
                     l3d_stream_t stream);

/* One iteration of the inverse-compositional loop (models/pointnetlk.py:70-88), launch `step` of `maxiter`:
 *   r = f - f0,  dx = -pinv r (fp64 sums),  m = max_b |dx_b|;   m < xtol: done <- 1;   else est_T <- exp(dx) est_T;
 *   est_T_series[step + 1] <- est_T.
 * Launch 0 takes est_T = identity and writes est_T_series[0] itself; once done is set (or singular[0] is), a launch leaves est_T, r
 * and the counter as they are and only fills its slot of est_T_series (nothing at all when singular).
 * state: int32 [4] = {done, iterations begun, stopped in iteration 0, ticket}, IN-OUT, zeroed by the caller once (the ticket returns
 * to 0 after every launch); ws: fp32 [B,8] SCRATCH; est_T [B,4,4], series [maxiter + 1,B,4,4] and r [B,K] are IN-OUT: state the
 * launches of one loop hand on (launch 0 reads none of them). */
int l3d_reg_iclk_step(const float *f, const float *f0, const float *pinv, int B, int K, int step, int maxiter, float xtol,
                      const int32_t *singular, float *ws, int32_t *state, float *est_T, float *series, float *r,
                      l3d_stream_t stream);

/* iPCRNet's pose update (models/pcrnet.py:33-50): pose7 [B,7] = the head's output (quaternion w x y z, translation) ->
 * q normalised (eps 1e-12), est_R <- R_q est_R [B,3,3], est_t <- R_q est_t + t_q [B,3], est_T [B,4,4] = [est_R est_t; 0 0 0 1].
 * est_R / est_t are IN-OUT; first != 0: the incoming pose is the identity and est_R / est_t are not read (then fully written).  fp64
 * inside, rounded to fp32 once. */
int l3d_reg_quat_update(const float *pose7, int B, int first, float *est_R, float *est_t, float *est_T, l3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
