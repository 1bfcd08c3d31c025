/* l3d_curvenet.h -- entry points of libl3d_hip.so for CurveNet's curve grouping (curvenet.hip): the start-point attention and
 * the whole curve walk of utils/curvenet_util.py:78-195, each one launch.  Same conventions as l3d_hip.h: device pointers, fp32
 * unless said otherwise, every call asynchronous on `stream`, status codes of l3d_status (null pointer / non-positive size -> -1,
 * a shape the kernels are not built for -> -2, both before any launch). */
#ifndef L3D_CURVENET_H
#define L3D_CURVENET_H
#include "l3d_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Start-point attention of CurveGrouping (utils/curvenet_util.py:505-508): x [B,C,N], w_att [C] (the 1-channel conv, no bias)
 *   att[b,n] = sigmoid(sum_c w_att[c] x[b,c,n])        [B,N]
 *   xa[b,n,c] = x[b,c,n] att[b,n]                       [B,N,C] channel-last, what l3d_curve_walk reads
 * C % 16 == 0, C <= 128, B <= 65535. */
int l3d_curve_prepare(const float *x, const float *w_att, int B, int C, int N, float *xa, float *att, l3d_stream_t stream);

/* Walk.forward (utils/curvenet_util.py:116-195) with both BatchNorms on running statistics, all curve_length steps in one launch,
 * one workgroup per cloud, one wavefront per curve and one lane per candidate:
 *   step 0:   pre = x[start]
 *   step > 0: m = m_scale (w_m . [cur; pre]) + m_shift  [2],  s = softmax(m) stored as [2][curve_num] per cloud; like the reference's
 *             view of that array as [curve_num][2] (:147), curve q takes att0, att1 = the values at flat positions 2 q, 2 q + 1;
 *             pre <- cur att0 + pre att1
 *   every step, for the k candidates j = adj[current point]:
 *             logit_j = a_scale (w_a[:C] . x[j] + w_a[C:] . pre) + a_shift
 *             step > 0: logit_j *= clamp(1 + cos(cur - pre, x[j] - cur), 0, 1), the cosine's divider clamped at 1e-8
 *             the largest logit is picked (the lowest j among equal ones); cur <- x[picked]; curves[..., step] = cur
 * x [B,N,C] channel-last (already scaled by the attention), adj int64 [B,N,k], start int64 [B,curve_num] (entries outside
 * [0,N) are clamped into it), w_a [2C], a_scale / a_shift [1], w_m [2,2C], m_scale / m_shift [2].
 * curves [B,C,curve_num,curve_length]; path int32 [B,curve_num,curve_length]: the point picked at each step.
 * C % 16 == 0, C <= 128, k <= 64, curve_num <= N, curve_num (2 C + 3) <= 16384 (a cloud's curves share one workgroup's LDS),
 * x 16-byte aligned (its rows are read 16 bytes at a time); else L3D_ERR_UNSUPPORTED. */
int l3d_curve_walk(const float *x, const int64_t *adj, const int64_t *start, int B, int N, int C, int k, int curve_num,
                   int curve_length, const float *w_a, const float *a_scale, const float *a_shift, const float *w_m,
                   const float *m_scale, const float *m_shift, float *curves, int32_t *path, l3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
