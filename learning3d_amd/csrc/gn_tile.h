// gn_tile.h -- what the GroupNorm-conv kernels of rpmnet.hip (gn_conv_kernel, gn_affine_kernel), rpmnet_param.hip (the two gpool
// kernels) and rpmnet_train.hip (gn_mean_rstd_kernel) share, so that "the same bits" between them holds by construction:
//
//   gn_tile         a 64-channel x 64-position tile of y = W relu(in_a x + in_s) + bias.  A workgroup of 256 threads owns 64 output
//                   channels (a 16-row MFMA tile per wave) and a block of 64 positions; input channels go through LDS in chunks of
//                   64, zero-padded there; the accumulator starts at the bias and takes v_mfma_f32_16x16x4_f32 steps in ascending ci
//                   over the operand transformed on load.  Each kernel keeps its own epilogue.
//   gn_group_stats  moments -> (mean, rstd) of a GroupNorm group, a wave per (cloud, group).
#pragma once
#include "common.h"

#define GN_TP 64                // positions per block
#define GN_TC 64                // input channels per LDS chunk
#define GN_LDU 80               // row pitch of the operand tile: the four k rows of an MFMA step land 16 banks apart
#define GN_LDW 65               // row pitch of the weight tile: 16 consecutive rows on 16 different banks

// what a workgroup knows of itself; grid (parts, ceil(Cout / 64), B)
struct GnCtx {
    int tid, wave, g, m, co0, cow, b, nchunks;
    bool wave_on, w_once;
};

__device__ __forceinline__ GnCtx gn_ctx(int Cin, int Cout)
{
    GnCtx c;
    c.tid = threadIdx.x;
    c.wave = c.tid >> 6;
    c.g = (c.tid >> 4) & 3;                            // lane = tid & 63 as 4 row groups g of 16 columns m
    c.m = c.tid & 15;
    c.co0 = blockIdx.y * 64;
    c.b = blockIdx.z;
    c.cow = c.co0 + c.wave * 16;                       // this wave's row tile
    c.wave_on = c.cow < Cout;                          // Cout % 16 == 0: a tile is whole or absent
    c.w_once = Cin <= GN_TC;
    c.nchunks = (Cin + GN_TC - 1) / GN_TC;
    return c;
}

// the whole weight tile of a workgroup whose Cin fits one chunk: loaded once, in front of the first block
__device__ __forceinline__ void gn_weights_once(const GnCtx &c, const float *__restrict__ w, int Cin, int Cout, float *sW)
{
    if (!c.w_once) return;
    for (int e = c.tid; e < GN_TC * GN_TC; e += 256) {
        const int row = e >> 6, col = e & 63;
        sW[row * GN_LDW + col] = (c.co0 + row < Cout && col < Cin) ? w[(size_t)(c.co0 + row) * Cin + col] : 0.f;
    }
}

// acc[t][r] = y of output channel cow + 4 g + r at column p0 + 16 t + m of its row, for the 64 columns from p0 on.  xb: the cloud's
// operand [Cin][P].  Column j of the block exists while c0 + j < n (c0, n: the block's place in a run of n columns, which is the whole
// row, or one pooled level of it); the others hold the bias alone and are the caller's to leave out.  Every thread of the workgroup
// calls it (it synchronises).  sW [GN_TC GN_LDW] as [co][ci], sU [GN_TC GN_LDU] as [ci][position].
__device__ __forceinline__ void gn_tile(const GnCtx &c, const float *__restrict__ xb, const float *__restrict__ in_a,
                                        const float *__restrict__ in_s, const float *__restrict__ w, const float (&bv)[4], int Cin,
                                        int Cout, int P, size_t p0, int c0, int n, float *sW, float *sU, f32x4 (&acc)[4])
{
#pragma unroll
    for (int t = 0; t < 4; t++) acc[t] = f32x4{bv[0], bv[1], bv[2], bv[3]};

    for (int ch = 0; ch < c.nchunks; ch++) {
        const int ci0 = ch * GN_TC, cn = min(GN_TC, Cin - ci0);
        __syncthreads();                               // the previous tile's MFMA reads are done
        if (!c.w_once) {
            for (int e = c.tid; e < GN_TC * GN_TC; e += 256) {
                const int row = e >> 6, col = e & 63;
                sW[row * GN_LDW + col] = (c.co0 + row < Cout && col < cn) ? w[(size_t)(c.co0 + row) * Cin + ci0 + col] : 0.f;
            }
        }
        const int cn4 = (cn + 3) & ~3;                 // rows up to the next multiple of 4 are read by the last MFMA step: zeros
        for (int e = c.tid; e < cn4 * GN_TP; e += 256) {
            const int ci = e >> 6, j = e & 63;
            float u = 0.f;
            if (ci < cn && c0 + j < n) {
                u = xb[(size_t)(ci0 + ci) * P + p0 + j];
                if (in_a) u = fmaxf(fmaf(in_a[(size_t)c.b * Cin + ci0 + ci], u, in_s[(size_t)c.b * Cin + ci0 + ci]), 0.f);
            }
            sU[ci * GN_LDU + j] = u;
        }
        __syncthreads();
        if (c.wave_on) {
            const int steps = cn4 >> 2;
            for (int s = 0; s < steps; s++) {
                const float a = sW[(c.wave * 16 + c.m) * GN_LDW + 4 * s + c.g];
                const float *ur = sU + (4 * s + c.g) * GN_LDU + c.m;
#pragma unroll
                for (int t = 0; t < 4; t++) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, ur[16 * t], acc[t], 0, 0, 0);
            }
        }
    }
}

// (mean, rstd) of group grp of cloud b from the raw moments [B,C,2] of its C / groups channels over `count` positions each.  The
// 64 lanes of a wave call it together and all receive the result.
__device__ __forceinline__ void gn_group_stats(const double *__restrict__ moments, int b, int C, int groups, int grp, int lane,
                                               double count, double eps, double &mean, double &rstd)
{
    const int cpg = C / groups;
    double m1 = 0.0, m2 = 0.0;
    for (int c = lane; c < cpg; c += 64) {
        const double *mo = moments + ((size_t)b * C + grp * cpg + c) * 2;
        m1 += mo[0];
        m2 += mo[1];
    }
    m1 = l3d_wave_sum(m1);
    m2 = l3d_wave_sum(m2);
    const double n = count * cpg;
    mean = m1 / n;
    double var = m2 / n - mean * mean;
    var = var < 0.0 ? 0.0 : var;
    rstd = 1.0 / sqrt(var + eps);
}
