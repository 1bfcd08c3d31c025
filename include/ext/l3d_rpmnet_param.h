/* l3d_rpmnet_param.h -- entry points of libl3d_hip.so for the layer of RPMNet's ParameterPredictionNet that ends in a maximum over
 * ALL positions of a cloud (rpmnet_param.hip): conv -> GroupNorm -> ReLU -> AdaptiveMaxPool1d(1), forward and backward, with the
 * [B,Cout,P] convolution output never stored in either direction.  Conventions are l3d_rpmnet.h's and l3d_rpmnet_train.h's:
 * device pointers, fp32 data, fp64 statistics, contiguous, every call asynchronous on `stream`, status codes of l3d_status (null
 * pointer / non-positive size -> -1, a shape the kernels are not built for -> -2, both before any launch).  No atomics: the same
 * bits on every call, whatever outputs and workspaces held before.  No alignment requirement beyond the element types'.
 *
 * Both entry points form y[b,co,p] = bias[co] + sum_ci w[co,ci] u[b,ci,p] from l3d_gn_conv's operands (x [B,Cin,P], in_a / in_s
 * [B,Cin] or both NULL, w [Cout,Cin], bias [Cout] or NULL) on l3d_gn_conv's tile, with the same v_mfma_f32_16x16x4_f32 fma chain in
 * ascending ci and the same transform of the operand on load: bit for bit the y that l3d_gn_conv(pool = 0) writes.
 * Limits of both: Cout % 16 == 0, 16 <= Cout <= L3D_GN_GPOOL_MAX_COUT, 1 <= Cin <= L3D_GN_CONV_MAX_CIN, 1 <= P <= L3D_GN_GPOOL_MAX_P,
 * B <= 65535; else L3D_ERR_UNSUPPORTED. */
#ifndef L3D_RPMNET_PARAM_H
#define L3D_RPMNET_PARAM_H
#include "../l3d_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define L3D_GN_GPOOL_MAX_COUT 4096     /* output channels of both entry points (a multiple of 16) */
#define L3D_GN_GPOOL_PARTS 16          /* most per-workgroup partials per (cloud, channel) in l3d_gn_conv_gpool's workspace */
#define L3D_GN_GPOOL_MAX_P 2147483520  /* most positions: the kernels index a row in int, a 64-wide block past its end included */

/* The forward.  Over all p < P of the y above:
 *   ymax, ymin [B,Cout]         the extremes; both, because the GroupNorm's scale can be zero or negative (see l3d_gn_conv): the
 *                               pooled activation is max(0, a (a >= 0 ? ymax : ymin) + s)
 *   pmax, pmin int32 [B,Cout]   the lowest p that attains each (-0 and +0 compare equal)
 *   moments fp64 [B,Cout,2]     (sum_p y, sum_p y^2) of the fp32 y: l3d_gn_affine's and l3d_gn_mean_rstd's input with count = P
 * A workgroup owns 64 output channels and ceil(blocks / L3D_GN_GPOOL_PARTS) blocks of 64 positions; its partial (extremes, their
 * positions, two fp64 sums) goes through `workspace` (l3d_gn_conv_gpool_workspace_bytes(B, Cout, P) bytes, 8-byte aligned) and a
 * second launch reduces the partials of a (cloud, channel) in ascending position order.  Columns past P in a partial block enter
 * neither the extremes nor the moments. */
size_t l3d_gn_conv_gpool_workspace_bytes(int B, int Cout, int P);
int l3d_gn_conv_gpool(const float *x, const float *in_a, const float *in_s, const float *w, const float *bias, int B, int Cin,
                      int Cout, int P, float *ymax, float *ymin, int32_t *pmax, int32_t *pmin, double *moments, void *workspace,
                      l3d_stream_t stream);

/* The backward: the gradient at y, dense dz [B,Cout,P], with y formed again tile by tile instead of kept.  In l3d_rpmnet_train.h's
 * notation, with C = Cout and the layer's own GroupNorm (out_a, out_s) from l3d_gn_affine(moments, count = P): the gradient du
 * [B,C] arrives at the pooled value and lives at one position per (cloud, channel), the winner pw = out_a >= 0 ? pmax : pmin, so
 *   g[b,c]  = du [pooled > 0]                     the caller's, with the mask of the forward's own pooled value
 *   S1 = g,  S2 = g zhat(ext)                     ext the winning extreme: the caller's part [B,C,2] for l3d_gn_backward_reduce
 *                                                 (count = P), which gives m = (M1, M2) per (cloud, group), dgamma and dbeta
 *   dz[b,c,p] = rstd (gamma_c g [p == pw] - M1 - zhat M2),  zhat = (y - mean) rstd      evaluated in fp64 and rounded once
 * g [B,C]; pw int32 [B,C] (a value outside [0,P) matches no position); stat fp64 [B,groups,2] = (mean, rstd) from
 * l3d_gn_mean_rstd; gamma [C]; m fp64 [B,groups,2].  A zero or negative gamma is ordinary input: nothing divides by it.
 * The limits above, and C % groups == 0. */
int l3d_gn_gpool_backward(const float *x, const float *in_a, const float *in_s, const float *w, const float *bias, const float *g,
                          const int32_t *pw, const double *stat, const float *gamma, const double *m, int B, int Cin, int Cout,
                          int groups, int P, float *dz, l3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
