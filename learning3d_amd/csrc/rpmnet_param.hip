// rpmnet_param.hip -- the layer of RPMNet's ParameterPredictionNet that ends in a maximum over all positions of a cloud
// (include/ext/l3d_rpmnet_param.h; models/rpmnet.py): conv -> GroupNorm -> ReLU -> AdaptiveMaxPool1d(1) with the [B,Cout,P]
// convolution output y never stored, forward or backward.
//
//   l3d_gn_conv_gpool      y tile by tile; per (cloud, channel) the extremes of y over all positions, the lowest position of each
//                          and the GroupNorm's raw moments (fp64): per-workgroup partials, a second launch in ascending order
//   l3d_gn_gpool_backward  y again; dz = rstd (gamma g [p == winner] - M1 - zhat M2) in fp64, rounded once, dense [B,Cout,P]
// Both form y on l3d_gn_conv's tile (rpmnet.hip: a workgroup owns 64 output channels, a 16-row MFMA tile per wave, and walks blocks
// of 64 positions; input channels through LDS in chunks of 64, zero-padded there) by gp_tile below, which is gn_conv_kernel's
// accumulation statement for statement: the accumulator starts at the bias and takes v_mfma_f32_16x16x4_f32 steps in ascending
// ci over the operand transformed on load, so y is l3d_gn_conv(pool = 0)'s, bit for bit.
#include "common.h"
#include "../../include/ext/l3d_rpmnet.h"
#include "../../include/ext/l3d_rpmnet_param.h"

typedef float gp_f32x4 __attribute__((ext_vector_type(4)));

#define GP_TP 64                // positions per block
#define GP_TC 64                // input channels per LDS chunk
#define GP_LDU 80               // row pitch of the operand tile: the four k rows of an MFMA step land 16 banks apart
#define GP_LDW 65               // row pitch of the weight tile: 16 consecutive rows on 16 different banks

struct GpPlan {
    int nblocks, bpp, nparts;
};

static GpPlan gp_plan(int P)
{
    GpPlan g;
    g.nblocks = l3d_divup(P, GP_TP);
    g.bpp = l3d_divup(g.nblocks, L3D_GN_GPOOL_PARTS);
    g.nparts = l3d_divup(g.nblocks, g.bpp);
    return g;
}

// what a workgroup of either kernel knows of itself
struct GpCtx {
    int tid, lane, wave, g, m, co0, cow, b, nchunks;
    bool wave_on, w_once;
};

__device__ __forceinline__ GpCtx gp_ctx(int Cin, int Cout)
{
    GpCtx c;
    c.tid = threadIdx.x;
    c.lane = c.tid & 63;
    c.wave = c.tid >> 6;
    c.g = c.lane >> 4;
    c.m = c.lane & 15;
    c.co0 = blockIdx.y * 64;
    c.b = blockIdx.z;
    c.cow = c.co0 + c.wave * 16;                       // this wave's row tile
    c.wave_on = c.cow < Cout;                          // Cout % 16 == 0: a tile is whole or absent
    c.w_once = Cin <= GP_TC;
    c.nchunks = (Cin + GP_TC - 1) / GP_TC;
    return c;
}

// the whole weight tile of a workgroup whose Cin fits one chunk: loaded once, in front of the first block
__device__ __forceinline__ void gp_weights_once(const GpCtx &c, const float *__restrict__ w, int Cin, int Cout, float *sW)
{
    if (!c.w_once) return;
    for (int e = c.tid; e < GP_TC * GP_TC; e += 256) {
        const int row = e >> 6, col = e & 63;
        sW[row * GP_LDW + col] = (c.co0 + row < Cout && col < Cin) ? w[(size_t)(c.co0 + row) * Cin + col] : 0.f;
    }
}

// acc[t][r] = y of output channel cow + 4 g + r at position c0 + 16 t + m, for the block of 64 positions at c0.  Every thread of the
// workgroup calls it (it synchronises); columns at or past P hold the bias alone and are the caller's to leave out.
__device__ __forceinline__ void gp_tile(const GpCtx &c, const float *__restrict__ xb, const float *__restrict__ in_a,
                                        const float *__restrict__ in_s, const float *__restrict__ w, const float (&bv)[4], int Cin,
                                        int Cout, int P, int c0, float *sW, float *sU, gp_f32x4 (&acc)[4])
{
#pragma unroll
    for (int t = 0; t < 4; t++) acc[t] = gp_f32x4{bv[0], bv[1], bv[2], bv[3]};

    for (int ch = 0; ch < c.nchunks; ch++) {
        const int ci0 = ch * GP_TC, cn = min(GP_TC, Cin - ci0);
        __syncthreads();                               // the previous tile's MFMA reads are done
        if (!c.w_once) {
            for (int e = c.tid; e < GP_TC * GP_TC; e += 256) {
                const int row = e >> 6, col = e & 63;
                sW[row * GP_LDW + col] = (c.co0 + row < Cout && col < cn) ? w[(size_t)(c.co0 + row) * Cin + ci0 + col] : 0.f;
            }
        }
        const int cn4 = (cn + 3) & ~3;                 // rows up to the next multiple of 4 are read by the last MFMA step: zeros
        for (int e = c.tid; e < cn4 * GP_TP; e += 256) {
            const int ci = e >> 6, j = e & 63;
            float u = 0.f;
            if (ci < cn && c0 + j < P) {
                u = xb[(size_t)(ci0 + ci) * P + c0 + j];
                if (in_a) u = fmaxf(fmaf(in_a[(size_t)c.b * Cin + ci0 + ci], u, in_s[(size_t)c.b * Cin + ci0 + ci]), 0.f);
            }
            sU[ci * GP_LDU + j] = u;
        }
        __syncthreads();
        if (c.wave_on) {
            const int steps = cn4 >> 2;
            for (int s = 0; s < steps; s++) {
                const float a = sW[(c.wave * 16 + c.m) * GP_LDW + 4 * s + c.g];
                const float *ur = sU + (4 * s + c.g) * GP_LDU + c.m;
#pragma unroll
                for (int t = 0; t < 4; t++) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, ur[16 * t], acc[t], 0, 0, 0);
            }
        }
    }
}

// (value, position) of a maximum / minimum: the better value, the lower position between equal values (-0 == +0)
__device__ __forceinline__ void gp_take_max(float &v, int &p, float ov, int op)
{
    const bool take = ov > v || (ov == v && op < p);
    v = take ? ov : v;
    p = take ? op : p;
}

__device__ __forceinline__ void gp_take_min(float &v, int &p, float ov, int op)
{
    const bool take = ov < v || (ov == v && op < p);
    v = take ? ov : v;
    p = take ? op : p;
}

// ------------------------------------------------------------------------------------------------------------------------------
// grid (nparts, ceil(Cout / 64), B).  Partials of (row = b Cout + co, part): sums[(row nparts + part) 2 + {0,1}] = (s1, s2),
// ext[...] = (max, min), pos[...] = (pmax, pmin).
__global__ __launch_bounds__(256) void gn_conv_gpool_kernel(const float *__restrict__ x, const float *__restrict__ in_a,
                                                            const float *__restrict__ in_s, const float *__restrict__ w,
                                                            const float *__restrict__ bias, int Cin, int Cout, int P, int nblocks,
                                                            int bpp, int nparts, double *__restrict__ sums, float *__restrict__ ext,
                                                            int *__restrict__ pos)
{
    __shared__ float sW[GP_TC * GP_LDW];               // [co][ci]
    __shared__ float sU[GP_TC * GP_LDU];               // [ci][position]
    const GpCtx c = gp_ctx(Cin, Cout);
    const int part = blockIdx.x;
    const float *xb = x + (size_t)c.b * Cin * P;

    float bv[4];
#pragma unroll
    for (int r = 0; r < 4; r++) bv[r] = (c.wave_on && bias) ? bias[c.cow + 4 * c.g + r] : 0.f;
    double s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
    float mx[4], mn[4];
    int px[4], pn[4];
#pragma unroll
    for (int r = 0; r < 4; r++) { mx[r] = -INFINITY; mn[r] = INFINITY; px[r] = pn[r] = 0x7fffffff; }

    gp_weights_once(c, w, Cin, Cout, sW);

    const int cb_end = min((part + 1) * bpp, nblocks);
    for (int cb = part * bpp; cb < cb_end; cb++) {
        const int c0 = cb * GP_TP;
        gp_f32x4 acc[4];
        gp_tile(c, xb, in_a, in_s, w, bv, Cin, Cout, P, c0, sW, sU, acc);
        if (c.wave_on) {
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const int p = c0 + 16 * t + c.m;       // ascending in t and in cb: a lane meets its positions in order
                if (p < P) {
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const float v = acc[t][r];
                        s1[r] += (double)v;
                        s2[r] += (double)v * (double)v;
                        gp_take_max(mx[r], px[r], v, p);
                        gp_take_min(mn[r], pn[r], v, p);
                    }
                }
            }
        }
    }

    // the 16 lanes of a row group hold disjoint columns of the same four channels: a butterfly within the group, lane m = 0 writes
#pragma unroll
    for (int r = 0; r < 4; r++) {
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) {
            s1[r] += __shfl_xor(s1[r], off, 64);
            s2[r] += __shfl_xor(s2[r], off, 64);
            const float ox = __shfl_xor(mx[r], off, 64), on = __shfl_xor(mn[r], off, 64);
            const int opx = __shfl_xor(px[r], off, 64), opn = __shfl_xor(pn[r], off, 64);
            gp_take_max(mx[r], px[r], ox, opx);
            gp_take_min(mn[r], pn[r], on, opn);
        }
    }
    if (c.wave_on && c.m == 0) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const size_t at = (((size_t)c.b * Cout + c.cow + 4 * c.g + r) * nparts + part) * 2;
            sums[at] = s1[r];
            sums[at + 1] = s2[r];
            ext[at] = mx[r];
            ext[at + 1] = mn[r];
            pos[at] = px[r];
            pos[at + 1] = pn[r];
        }
    }
}

// a thread per (cloud, channel): its partials in ascending part, which is ascending position
__global__ __launch_bounds__(256) void gn_gpool_reduce_kernel(const double *__restrict__ sums, const float *__restrict__ ext,
                                                              const int *__restrict__ pos, long rows, int nparts,
                                                              float *__restrict__ ymax, float *__restrict__ ymin,
                                                              int *__restrict__ pmax, int *__restrict__ pmin,
                                                              double *__restrict__ moments)
{
    const long row = (long)blockIdx.x * 256 + threadIdx.x;
    if (row >= rows) return;
    double s1 = 0.0, s2 = 0.0;
    float mx = -INFINITY, mn = INFINITY;
    int px = 0x7fffffff, pn = 0x7fffffff;
    for (int p = 0; p < nparts; p++) {
        const size_t at = ((size_t)row * nparts + p) * 2;
        s1 += sums[at];
        s2 += sums[at + 1];
        gp_take_max(mx, px, ext[at], pos[at]);
        gp_take_min(mn, pn, ext[at + 1], pos[at + 1]);
    }
    ymax[row] = mx;
    ymin[row] = mn;
    pmax[row] = px;
    pmin[row] = pn;
    moments[row * 2] = s1;
    moments[row * 2 + 1] = s2;
}

// the guards both entry points share
static int gp_check(int B, int Cin, int Cout, int P)
{
    if (Cout % 16 || Cout > L3D_GN_GPOOL_MAX_COUT || Cin > L3D_GN_CONV_MAX_CIN || P > L3D_GN_GPOOL_MAX_P || B > 65535)
        return L3D_ERR_UNSUPPORTED;
    return L3D_OK;
}

extern "C" size_t l3d_gn_conv_gpool_workspace_bytes(int B, int Cout, int P)
{
    if (B <= 0 || Cout <= 0 || P <= 0) return 0;
    // per (cloud, channel, part): two doubles, two floats, two ints
    return (size_t)B * Cout * gp_plan(P).nparts * (2 * sizeof(double) + 2 * sizeof(float) + 2 * sizeof(int));
}

extern "C" int l3d_gn_conv_gpool(const float *x, const float *in_a, const float *in_s, const float *w, const float *bias, int B,
                                 int Cin, int Cout, int P, float *ymax, float *ymin, int32_t *pmax, int32_t *pmin, double *moments,
                                 void *workspace, l3d_stream_t stream)
{
    L3D_REQUIRE(x && w && ymax && ymin && pmax && pmin && moments && workspace && B > 0 && Cin > 0 && Cout > 0 && P > 0);
    L3D_REQUIRE((in_a == nullptr) == (in_s == nullptr));
    const int st = gp_check(B, Cin, Cout, P);
    if (st != L3D_OK) return st;
    const GpPlan g = gp_plan(P);
    const size_t n = (size_t)B * Cout * g.nparts * 2;
    double *sums = (double *)workspace;
    float *ext = (float *)(sums + n);
    int *pos = (int *)(ext + n);
    hipLaunchKernelGGL(gn_conv_gpool_kernel, dim3(g.nparts, l3d_divup(Cout, 64), B), dim3(256), 0, (hipStream_t)stream, x, in_a, in_s,
                       w, bias, Cin, Cout, P, g.nblocks, g.bpp, g.nparts, sums, ext, pos);
    const int err = l3d_check_launch();
    if (err != L3D_OK) return err;
    const long rows = (long)B * Cout;
    hipLaunchKernelGGL(gn_gpool_reduce_kernel, dim3(l3d_divup(rows, 256)), dim3(256), 0, (hipStream_t)stream, (const double *)sums,
                       (const float *)ext, (const int *)pos, rows, g.nparts, ymax, ymin, pmax, pmin, moments);
    return l3d_check_launch();
}

// ------------------------------------------------------------------------------------------------------------------------------
// grid (nparts, ceil(Cout / 64), B)
__global__ __launch_bounds__(256) void gn_gpool_backward_kernel(const float *__restrict__ x, const float *__restrict__ in_a,
                                                                const float *__restrict__ in_s, const float *__restrict__ w,
                                                                const float *__restrict__ bias, const float *__restrict__ gr,
                                                                const int *__restrict__ pw, const double *__restrict__ stat,
                                                                const float *__restrict__ gamma, const double *__restrict__ mm,
                                                                int Cin, int Cout, int groups, int P, int nblocks, int bpp,
                                                                float *__restrict__ dz)
{
    __shared__ float sW[GP_TC * GP_LDW];               // [co][ci]
    __shared__ float sU[GP_TC * GP_LDU];               // [ci][position]
    const GpCtx c = gp_ctx(Cin, Cout);
    const int part = blockIdx.x;
    const float *xb = x + (size_t)c.b * Cin * P;

    // the constants of this lane's four channels
    float bv[4];
    double mean[4], rstd[4], m1[4], m2[4], gg[4];     // gg = gamma g, the winner's term
    int win[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        bv[r] = 0.f;
        mean[r] = rstd[r] = m1[r] = m2[r] = gg[r] = 0.0;
        win[r] = -1;
        if (c.wave_on) {
            const int ch = c.cow + 4 * c.g + r;
            const size_t row = (size_t)c.b * Cout + ch, grp = ((size_t)c.b * groups + ch / (Cout / groups)) * 2;
            if (bias) bv[r] = bias[ch];
            mean[r] = stat[grp];
            rstd[r] = stat[grp + 1];
            m1[r] = mm[grp];
            m2[r] = mm[grp + 1];
            gg[r] = (double)gamma[ch] * (double)gr[row];
            win[r] = pw[row];
        }
    }

    gp_weights_once(c, w, Cin, Cout, sW);

    const int cb_end = min((part + 1) * bpp, nblocks);
    for (int cb = part * bpp; cb < cb_end; cb++) {
        const int c0 = cb * GP_TP;
        gp_f32x4 acc[4];
        gp_tile(c, xb, in_a, in_s, w, bv, Cin, Cout, P, c0, sW, sU, acc);
        if (c.wave_on) {
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const int p = c0 + 16 * t + c.m;
                if (p < P) {
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const double top = p == win[r] ? gg[r] : 0.0;
                        dz[((size_t)c.b * Cout + c.cow + 4 * c.g + r) * P + p] =
                            (float)(rstd[r] * ((top - m1[r]) - (((double)acc[t][r] - mean[r]) * rstd[r]) * m2[r]));
                    }
                }
            }
        }
    }
}

extern "C" int l3d_gn_gpool_backward(const float *x, const float *in_a, const float *in_s, const float *w, const float *bias,
                                     const float *g, const int32_t *pw, const double *stat, const float *gamma, const double *m, int B,
                                     int Cin, int Cout, int groups, int P, float *dz, l3d_stream_t stream)
{
    L3D_REQUIRE(x && w && g && pw && stat && gamma && m && dz && B > 0 && Cin > 0 && Cout > 0 && groups > 0 && P > 0);
    L3D_REQUIRE((in_a == nullptr) == (in_s == nullptr));
    const int st = gp_check(B, Cin, Cout, P);
    if (st != L3D_OK) return st;
    if (Cout % groups) return L3D_ERR_UNSUPPORTED;
    const GpPlan pl = gp_plan(P);
    hipLaunchKernelGGL(gn_gpool_backward_kernel, dim3(pl.nparts, l3d_divup(Cout, 64), B), dim3(256), 0, (hipStream_t)stream, x, in_a,
                       in_s, w, bias, g, pw, stat, gamma, m, Cin, Cout, groups, P, pl.nblocks, pl.bpp, dz);
    return l3d_check_launch();
}
