/* l3d_conv_f16_route.h -- which form of conv_f16.hip's kernel an l3d_pointwise_conv_f16 call runs.  The plain two-plane form (flags ==
 * L3D_CONV_F16_TWO_PLANE, fp32 y and nothing else: DGCNN's conv5) has two: the chunk loop, in which all of a wave's accumulators become
 * final in the last K chunk, and the tile-major tail, which takes the last L3D_CONV_F16_TAIL_CHUNKS chunks MFMA tile by MFMA tile and
 * stores each tile as it becomes final.  The tail needs two chunks in front of it, so Cin / 16 >= L3D_CONV_F16_TAIL_CHUNKS + 2; shorter
 * K, and every other combination of flags and outputs, runs the loop.  Both forms give the same bits. */
#ifndef L3D_CONV_F16_ROUTE_H
#define L3D_CONV_F16_ROUTE_H
#include "../l3d_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define L3D_CONV_F16_ROUTE_LOOP 0
#define L3D_CONV_F16_ROUTE_TAIL 1
#define L3D_CONV_F16_TAIL_CHUNKS 3

/* The form a call l3d_pointwise_conv_f16(..., Cin, Cout, N, ..., flags, y, NULL, NULL, NULL, NULL, ...) takes (y alone: no residual,
 * image, pool or maxima): L3D_CONV_F16_ROUTE_TAIL or L3D_CONV_F16_ROUTE_LOOP; L3D_ERR_UNSUPPORTED for sizes or flags that call
 * refuses, L3D_ERR_INVALID_ARG for a non-positive size or an unknown flag.  Launches nothing. */
int l3d_conv_f16_route(int Cin, int Cout, int N, int flags);

#ifdef __cplusplus
}
#endif
#endif
