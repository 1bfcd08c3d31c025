/* l3d_masknet2.h -- entry points of libl3d_hip.so for MaskNet2 (masknet2.hip): the Mish activation behind its folded Conv+BN layers,
 * the self-attention of its feature model whose query, key and value are ONE tensor (models/masknet2.py:35-70), and the outer-product
 * softmax between the two clouds' global features (:124-163).  Same conventions as l3d_masknet.h: device pointers, fp32, contiguous,
 * every call asynchronous on `stream`, status codes of l3d_status (null pointer / non-positive size -> -1, a shape the kernels are
 * not built for -> -2, both before any launch). */
#ifndef L3D_MASKNET2_H
#define L3D_MASKNET2_H
#include "l3d_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* tile sizes of l3d_self_attention_shared: queries per workgroup (4 waves x 32) and keys per LDS tile */
#define L3D_SELF_ATTN_TQ 128
#define L3D_SELF_ATTN_TK 32

/* y[i] = x[i] tanh(softplus(x[i])), softplus(x) = x for x > 20 (torch's rule), i < count; y may be x.
 * One exp and one division per element: n = e^x, t = n (n + 2), y = x t / (t + 2); x > 20 -> x.  No overflow for any finite x; NaN
 * propagates; where e^x underflows (x < -87.3, -inf included) the result is -0.  16 bytes at a time when x and y are both 16-byte
 * aligned, one float at a time for the tail and for misaligned pointers: the same bits on both routes. */
int l3d_mish(const float *x, long count, float *y, l3d_stream_t stream);

/* Self-attention with one operand: q, out [B,D,N] channel-first, beta one float on the device, out must not overlap q.
 *   out[b,c,i] = q[b,c,i] + beta sum_j p_ij q[b,c,j],   p_ij = softmax_j(sum_c q[b,c,i] q[b,c,j])   (no scale)
 * Flash-style: online softmax per query, the [N,N] scores stay in registers.  Both products run on the fp32 matrix cores (exact
 * fp32 fma chains: ascending channel for a logit, ascending key within a tile for a context value); exp is v_exp_f32 of the
 * logit minus the running maximum.  Keys >= N weigh 0; queries >= N are not stored.
 * D % 32 == 0, 32 <= D <= 256, any N >= 1, B <= 65535; else L3D_ERR_UNSUPPORTED.  No alignment requirement. */
int l3d_self_attention_shared(const float *q, const float *beta, int B, int D, int N, float *out, l3d_stream_t stream);

/* self_attention_fc's mixing of two feature vectors per cloud: px, py, outx, outy [B,C], beta one float on the device.
 *   outx[b,i] = px_i + beta sum_j softmax_j(px_i py_j) px_j
 *   outy[b,j] = py_j + beta sum_i softmax_i(px_i py_j) py_i
 * One workgroup per cloud, one thread per index; the row maximum is analytic (px_i times the largest or the smallest py, by px_i's
 * sign), so every output is one pass and no [C,C] tensor exists.  1 <= C <= 1024, B <= 65535; else L3D_ERR_UNSUPPORTED.
 * The outputs must not overlap the inputs. */
int l3d_outer_softmax_mix(const float *px, const float *py, const float *beta, int B, int C, float *outx, float *outy,
                          l3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
