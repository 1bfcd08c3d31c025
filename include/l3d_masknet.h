/* l3d_masknet.h -- entry points of libl3d_hip.so for MaskNet's two ends (masknet.hip): the tail of its per-point head h3
 * (models/masknet.py:14-18, Conv(256->128)+ReLU, Conv(128->1)+Sigmoid) and the point selection of MaskNet.forward (:68-77), each
 * one launch.  Same conventions as l3d_hip.h: device pointers, fp32 unless said otherwise, every call asynchronous on `stream`,
 * status codes of l3d_status (null pointer / non-positive size -> -1, a shape the kernels are not built for -> -2, both before
 * any launch).
 * A per-model header like l3d_curvenet.h and l3d_registration.h: _lib.py reads every header of include/ into one table. */
#ifndef L3D_MASKNET_H
#define L3D_MASKNET_H
#include "l3d_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The last two layers of a per-point head whose final width is 1: x [B,C,N] channel-first, w4 [H,C], b4 [H], w5 [H], b5 [1]
 *   mask[b,n] = sigmoid(b5 + sum_h w5[h] relu(b4[h] + sum_c w4[h,c] x[b,c,n]))        [B,N]
 * The C -> H product runs on the fp32 matrix cores (an fp32 fma chain per hidden unit, ascending c); the H -> 1 dot product is taken
 * from the accumulators (per lane ascending h within its rows, then across the four lane groups); the [B,H,N] map is never written.
 * C % 16 == 0, C <= 256, H % 32 == 0, H <= 128, any N >= 1 (the last point tile is ragged); else L3D_ERR_UNSUPPORTED.
 * x is read 16 bytes at a time when it and its rows are 16-byte aligned (N % 4 == 0), one float at a time otherwise. */
int l3d_mask_tail(const float *x, const float *w4, const float *b4, const float *w5, const float *b5, int B, int C, int H, int N,
                  float *mask, l3d_stream_t stream);

/* Select points by their mask value, one workgroup per cloud: mask [B,N], points [B,N,3].
 *   k > 0  (torch.topk(mask, k, sorted=False) with a defined order): point i is selected iff rank(i) < k, where
 *          rank(i) = #{j : m_j > m_i, or m_j == m_i and j < i}; a NaN orders above every number and equal to another NaN; -0 == +0.
 *          Exactly k points per cloud (k <= N).  idx int64 [B,k], out [B,k,3].
 *   k == 0 (mask > threshold of a single pair, B == 1): selected iff m_i > threshold (never a NaN).  idx int64 [1,N] and out [1,N,3],
 *          of which the first count[0] entries are written (the rest is left as it was).
 * In both modes the selected indices are written in ascending order, out[b,s,:] = points[b, idx[b,s], :], count int32 [B] = the
 * number selected.  N <= 16384 (a cloud's keys live in one workgroup's LDS), else L3D_ERR_UNSUPPORTED; k < 0, k > N, or k == 0 with
 * B != 1 -> L3D_ERR_INVALID_ARG. */
int l3d_mask_select(const float *mask, const float *points, int B, int N, int k, float threshold, int64_t *idx, float *out,
                    int32_t *count, l3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
