/* l3d_partial.h -- entry point of libl3d_hip.so for partial and noisy registration pairs (partial.hip): the crop of the reference's
 * data_utils/dataloaders.py (farthest_subsample_points :69-77, planar_crop :106-119) with the jitter of jitter_pointcloud (:63-67)
 * fused into the gather, one workgroup per cloud.
 * Same conventions as l3d_prnet.h: device pointers, contiguous, asynchronous on `stream`, status codes of l3d_status (null pointer /
 * non-positive size -> -1, a shape the kernel is not built for -> -2, both before any launch).  No float atomics: the same bits on
 * every call, whatever the outputs held before.  One route for every alignment (4-byte accesses only). */
#ifndef L3D_PARTIAL_H
#define L3D_PARTIAL_H
#include "../l3d_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define L3D_CROP_NEAREST 0            /* the K points nearest vec[b], nearest first */
#define L3D_CROP_PLANE 1              /* the K points farthest along vec[b] from centre[b], in ascending index order */
#define L3D_CROP_MAX_N 8192           /* points per cloud: a cloud's 64-bit keys live in one workgroup's LDS (64 KB of them) */

/* points [B,N,C] fp32 (C >= 3, columns 0..2 are x y z; the other columns ride along), vec [B,3] fp64, centre [B,3] fp32 (read in
 * plane mode only; may be NULL in nearest mode).  Every operation below is rounded on its own (no fused multiply-add).
 *   L3D_CROP_NEAREST  d = (double)xyz_i - vec[b];  key_i = (dx dx + dy dy) + dz dz in fp64.  The K SMALLEST keys are selected; the
 *                     selected points are listed in ASCENDING KEY order, equal keys in ascending index order.
 *   L3D_CROP_PLANE    f = xyz_i - centre[b] in fp32;  key_i = ((double)fx vec_x + (double)fy vec_y) + (double)fz vec_z in fp64.  The K
 *                     LARGEST keys are selected; the selected points are listed in ASCENDING INDEX order.
 * In both modes keys are ordered by l3d_mask_select's rule: a NaN key is above every number (it is selected first in plane mode,
 * last in nearest mode), NaN keys among themselves and equal keys rank by index, the lower index first; -0 == +0.  Exactly K points.
 * With s_0 .. s_{K-1} the selected points in the mode's order:
 *   idx  int64 [B,K]  = s_p                                                     (may be NULL)
 *   mask float [B,N]  = 1.0 at the selected points, 0.0 elsewhere, every element written   (may be NULL)
 *   out  [B,K,C]      = points[b, s_p, :] + e,  e = clamp(sigma[b] noise[b,p,:], -clip, clip)     (may be NULL; not all three)
 *                       noise [B,K,C] NULL: no addition at all, out is a bit copy of the rows.  sigma [B] NULL: 1 (no
 *                       multiplication).  clip <= 0: no clamp.  A NaN in e stays a NaN.  fp32: one multiplication, one addition.
 * L3D_CROP_PLANE with K == N ranks nothing (the keys are not formed, vec and centre are not read): s_p = p -- the jitter alone.
 * 1 <= K <= N (K > N -> L3D_ERR_INVALID_ARG), as are an unknown mode, a NULL vec (unless plane mode with K == N) and a NULL centre
 * in plane mode with K < N; N <= L3D_CROP_MAX_N, B <= 65535 and C >= 3, else L3D_ERR_UNSUPPORTED. */
int l3d_crop_select(const float *points, const double *vec, const float *centre, int B, int N, int C, int mode, int K, const float *noise,
                    const float *sigma, float clip, int64_t *idx, float *mask, float *out, l3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
