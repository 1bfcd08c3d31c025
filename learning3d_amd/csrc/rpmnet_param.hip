// rpmnet_param.hip -- the layer of RPMNet's ParameterPredictionNet that ends in a maximum over all positions of a cloud
// (include/ext/l3d_rpmnet_param.h; models/rpmnet.py): conv -> GroupNorm -> ReLU -> AdaptiveMaxPool1d(1) with the [B,Cout,P]
// convolution output y never stored, forward or backward.
//
//   l3d_gn_conv_gpool      y tile by tile; per (cloud, channel) the extremes of y over all positions, the lowest position of each
//                          and the GroupNorm's raw moments (fp64): per-workgroup partials, a second launch in ascending order
//   l3d_gn_gpool_backward  y again; dz = rstd (gamma g [p == winner] - M1 - zhat M2) in fp64, rounded once, dense [B,Cout,P]
// Both form y by gn_tile (gn_tile.h), the tile l3d_gn_conv's kernel (rpmnet.hip) calls too, so y is l3d_gn_conv(pool = 0)'s, bit for
// bit; the epilogues are this file's.
#include "common.h"
#include "gn_tile.h"
#include "../../include/ext/l3d_rpmnet.h"
#include "../../include/ext/l3d_rpmnet_param.h"

struct GpPlan {
    int nblocks, bpp, nparts;
};

static GpPlan gp_plan(int P)
{
    GpPlan g;
    g.nblocks = l3d_divup(P, GN_TP);
    g.bpp = l3d_divup(g.nblocks, L3D_GN_GPOOL_PARTS);
    g.nparts = l3d_divup(g.nblocks, g.bpp);
    return g;
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
    __shared__ float sW[GN_TC * GN_LDW];               // [co][ci]
    __shared__ float sU[GN_TC * GN_LDU];               // [ci][position]
    const GnCtx c = gn_ctx(Cin, Cout);
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

    gn_weights_once(c, w, Cin, Cout, sW);

    const int cb_end = min((part + 1) * bpp, nblocks);
    for (int cb = part * bpp; cb < cb_end; cb++) {
        const int c0 = cb * GN_TP;
        f32x4 acc[4];
        gn_tile(c, xb, in_a, in_s, w, bv, Cin, Cout, P, c0, c0, P, sW, sU, acc);
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
    __shared__ float sW[GN_TC * GN_LDW];               // [co][ci]
    __shared__ float sU[GN_TC * GN_LDU];               // [ci][position]
    const GnCtx c = gn_ctx(Cin, Cout);
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

    gn_weights_once(c, w, Cin, Cout, sW);

    const int cb_end = min((part + 1) * bpp, nblocks);
    for (int cb = part * bpp; cb < cb_end; cb++) {
        const int c0 = cb * GN_TP;
        f32x4 acc[4];
        gn_tile(c, xb, in_a, in_s, w, bv, Cin, Cout, P, c0, c0, P, sW, sU, acc);
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
