/* l3d_pointconv.h -- entry point of libl3d_hip.so for PointConv (pointconv.hip): the density-scaled weight-net aggregation of a
 * PointConv set-abstraction layer (utils/pointconv_util.py:261-371) as one launch.
 * Same conventions as l3d_rpmnet.h: device pointers, fp32, contiguous, asynchronous on `stream`, status codes of l3d_status (null
 * pointer / non-positive size -> -1, a shape the kernel is not built for -> -2, both before any launch).  No float atomics, a fixed
 * summation order: the same bits on every call, whatever the output held before. */
#ifndef L3D_POINTCONV_H
#define L3D_POINTCONV_H
#include "../l3d_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define L3D_POINTCONV_MAX_C 1024      /* channels of feat (a multiple of 16) */
#define L3D_POINTCONV_WN_FLOATS 248   /* WeightNet 3 -> 8 -> 8 -> 16 folded: per layer w [cout][cin] then b [cout]: 32 + 72 + 144 */
#define L3D_POINTCONV_DN_FLOATS 177   /* DensityNet 1 -> 16 -> 8 -> 1 folded, same packing: 32 + 136 + 9 */

/* Per centre (b, s), over its K neighbours:
 *   d[k]      = DensityNet(ginv[b,s,k] / max_k ginv[b,s,k])       (1 when ginv is NULL: the layer without density)
 *   w[k,0:16] = WeightNet(gxyz[b,s,k,0:3])
 *   out[b, 16 c + j, s] = sum_k feat[b,c,k,s] (d[k] w[k,j])       (an fp32 fma chain in ascending k)
 * feat [B,C,K,S]: the last mlp_convs activation, channel-first as the conv kernels write it (position p = k S + s).
 * gxyz [B,S,K,3]: the centred neighbour coordinates, as the grouping writes them (grouped_xyz_norm; no permute).
 * ginv [B,S,K] or NULL: the grouped inverse density.
 * wn [L3D_POINTCONV_WN_FLOATS], dn [L3D_POINTCONV_DN_FLOATS] (dn may be NULL when ginv is): every layer Conv + eval-mode BatchNorm
 *   folded into y = max(0, w x + b); every layer has the ReLU, the last one included.
 * out [B,16 C,S]: CHANNEL-FIRST, row 16 c + j being the reference's flattened index (.view(B, npoint, -1)).  The Linear(16 C -> C')
 *   behind it is then W [C',16 C] times out[b] [16 C,S] per cloud -- l3d_bmm_f32 with the weight broadcast over the batch, or any
 *   of the channel-first conv kernels over [B, Cin = 16 C, N = S] -- whose output [B,C',S] is the layer's own output layout; for
 *   S = 1 the same memory is the rows [B,16 C].  No transpose or copy in between.
 * C % 16 == 0, 16 <= C <= L3D_POINTCONV_MAX_C, any K >= 1, any S >= 1, B <= 65535; else L3D_ERR_UNSUPPORTED.  ginv given without
 * dn -> L3D_ERR_INVALID_ARG.  No alignment requirement beyond the element types'. */
int l3d_pointconv_aggregate(const float *feat, const float *gxyz, const float *ginv, const float *wn, const float *dn, int B, int C,
                            int K, int S, float *out, l3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
