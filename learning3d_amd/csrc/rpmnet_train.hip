// rpmnet_train.hip -- the backward of PPFNet's conv -> GroupNorm -> ReLU (-> maximum over the neighbours) layers
// (include/ext/l3d_rpmnet_train.h; models/ppfnet.py's autograd function).  The forward keeps only the convolution outputs y; the
// ReLU mask and the normalised value are recomputed here from y and the per-(cloud, channel) affine (in_a, in_s) as the forward's
// l3d_gn_conv forms them on load: h = fmaf(in_a, y, in_s), one rounding.
//
//   l3d_gn_mean_rstd        moments -> (mean, rstd) per (cloud, group) by gn_group_stats (gn_tile.h), as l3d_gn_affine forms them
//   l3d_gn_pool_winner      the lowest k attaining the extreme in_a's sign selects; a lane per n, k rows read in runs along n
//   l3d_gn_relu             u = max(0, h) written out: the second operand of the next layer's l3d_wgrad
//   l3d_gn_backward_stats   (sum g, sum g zhat) per (cloud, channel): a workgroup per 8192-position chunk of a row, fp64, fixed order;
//                           rows of several chunks through the workspace and a second launch in ascending order
//   l3d_gn_backward_reduce  the group sums M1, M2 and dgamma / dbeta in one launch
//   l3d_gn_backward_apply   dz = rstd (gamma g - M1 - zhat M2) in fp64, rounded once
// The pooled forms take the gradient at the pooled value [B,C,N'] and the winner index; the dense scatter is never formed.
// stats and apply stream [B,C,P] tensors and are HBM-bound: 16 bytes per lane where P (pooled: N') is a multiple of 4 and the pointers
// allow, a scalar route otherwise; grids are (chunks, C, B), so B = 2 fills the machine as B = 32 does.  Nothing divides by gamma.
#include "common.h"
#include "gn_tile.h"
#include "../../include/ext/l3d_rpmnet.h"
#include "../../include/ext/l3d_rpmnet_train.h"

static bool gt_aligned(const void *p, size_t to)
{
    return p == nullptr || (((size_t)p) & (to - 1)) == 0;
}

// ------------------------------------------------------------------------------------------------------------------------------
// a wave per (cloud, group); gn_group_stats (gn_tile.h) is gn_affine_kernel's too
__global__ __launch_bounds__(64) void gn_mean_rstd_kernel(const double *__restrict__ moments, int C, int groups, double count,
                                                          double eps, double *__restrict__ stat)
{
    const int lane = threadIdx.x, grp = blockIdx.x, b = blockIdx.y;
    double mean, rstd;
    gn_group_stats(moments, b, C, groups, grp, lane, count, eps, mean, rstd);
    if (lane == 0) {
        double *o = stat + ((size_t)b * groups + grp) * 2;
        o[0] = mean;
        o[1] = rstd;
    }
}

extern "C" int l3d_gn_mean_rstd(const double *moments, int B, int C, int groups, int count, float eps, double *stat, l3d_stream_t stream)
{
    L3D_REQUIRE(moments && stat && B > 0 && C > 0 && groups > 0 && count > 0);
    if (C % groups || B > 65535) return L3D_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(gn_mean_rstd_kernel, dim3(groups, B), dim3(64), 0, (hipStream_t)stream, moments, C, groups, (double)count,
                       (double)eps, stat);
    return l3d_check_launch();
}

// ------------------------------------------------------------------------------------------------------------------------------
// grid (ceil(N' / 256), C, B)
__global__ __launch_bounds__(256) void gn_pool_winner_kernel(const float *__restrict__ y, const float *__restrict__ in_a, int C, int K,
                                                             int NP, unsigned char *__restrict__ widx)
{
    const int n = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y, b = blockIdx.z;
    if (n >= NP) return;
    const size_t row = (size_t)b * C + c;
    const float *yr = y + row * (size_t)K * NP + n;
    const bool up = in_a[row] >= 0.f;
    float best = yr[0];
    int at = 0;
    for (int k = 1; k < K; k++) {
        const float v = yr[(size_t)k * NP];
        if (up ? v > best : v < best) {                // strict: the lowest k on ties
            best = v;
            at = k;
        }
    }
    widx[row * NP + n] = (unsigned char)at;
}

extern "C" int l3d_gn_pool_winner(const float *y, const float *in_a, int B, int C, int K, int NP, unsigned char *widx,
                                  l3d_stream_t stream)
{
    L3D_REQUIRE(y && in_a && widx && B > 0 && C > 0 && K > 0 && NP > 0);
    if (K > L3D_PPF_MAX_K || B > 65535 || C > 65535 || NP > L3D_GN_BWD_MAX_P / K) return L3D_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(gn_pool_winner_kernel, dim3(l3d_divup(NP, 256), C, B), dim3(256), 0, (hipStream_t)stream, y, in_a, C, K, NP, widx);
    return l3d_check_launch();
}

// ------------------------------------------------------------------------------------------------------------------------------
// grid (ceil(P / 1024) or ceil(P / 256), C, B)
template <bool VEC>
__global__ __launch_bounds__(256) void gn_relu_kernel(const float *__restrict__ y, const float *__restrict__ in_a,
                                                      const float *__restrict__ in_s, int C, int P, float *__restrict__ u)
{
    const int c = blockIdx.y, b = blockIdx.z;
    const size_t row = (size_t)b * C + c;
    const float a = in_a[row], s = in_s[row];
    if (VEC) {
        const long p = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
        if (p >= P) return;
        const float4 v = *(const float4 *)(y + row * P + p);
        *(float4 *)(u + row * P + p) = make_float4(fmaxf(fmaf(a, v.x, s), 0.f), fmaxf(fmaf(a, v.y, s), 0.f), fmaxf(fmaf(a, v.z, s), 0.f),
                                                   fmaxf(fmaf(a, v.w, s), 0.f));
    } else {
        const long p = (long)blockIdx.x * 256 + threadIdx.x;
        if (p >= P) return;
        u[row * P + p] = fmaxf(fmaf(a, y[row * P + p], s), 0.f);
    }
}

extern "C" int l3d_gn_relu(const float *y, const float *in_a, const float *in_s, int B, int C, int P, float *u, l3d_stream_t stream)
{
    L3D_REQUIRE(y && in_a && in_s && u && B > 0 && C > 0 && P > 0);
    if (B > 65535 || C > 65535 || P > L3D_GN_BWD_MAX_P) return L3D_ERR_UNSUPPORTED;
    if (P % 4 == 0 && gt_aligned(y, 16) && gt_aligned(u, 16))
        hipLaunchKernelGGL(gn_relu_kernel<true>, dim3(l3d_divup(P, 1024), C, B), dim3(256), 0, (hipStream_t)stream, y, in_a, in_s, C, P, u);
    else
        hipLaunchKernelGGL(gn_relu_kernel<false>, dim3(l3d_divup(P, 256), C, B), dim3(256), 0, (hipStream_t)stream, y, in_a, in_s, C, P, u);
    return l3d_check_launch();
}

// ------------------------------------------------------------------------------------------------------------------------------
// The row of (cloud b, channel c): its constants, read once per workgroup
struct GtRow {
    float a, s;
    double mean, rstd;
};

__device__ __forceinline__ GtRow gt_row(const float *__restrict__ in_a, const float *__restrict__ in_s, const double *__restrict__ stat,
                                        int b, int c, int C, int groups)
{
    GtRow r;
    const size_t row = (size_t)b * C + c;
    const double *st = stat + ((size_t)b * groups + c / (C / groups)) * 2;
    r.a = in_a[row];
    r.s = in_s[row];
    r.mean = st[0];
    r.rstd = st[1];
    return r;
}

// NP = the positions summed per row (dense: P; pooled: N').  grid (nparts, C, B); out = part when nparts == 1, the workspace else.
// POOL: du [B,C,N'] at the winner's position widx N' + n.  VEC (dense only): 16-byte loads, four positions per trip.
template <bool VEC, bool POOL>
__global__ __launch_bounds__(256) void gn_backward_stats_kernel(const float *__restrict__ du, const unsigned char *__restrict__ widx,
                                                                int K, const float *__restrict__ y, const float *__restrict__ in_a,
                                                                const float *__restrict__ in_s, const double *__restrict__ stat,
                                                                int C, int groups, int NP, int nparts, double *__restrict__ out)
{
    __shared__ double sRed[4];
    const int tid = threadIdx.x, part = blockIdx.x, c = blockIdx.y, b = blockIdx.z;
    const GtRow r = gt_row(in_a, in_s, stat, b, c, C, groups);
    const size_t row = (size_t)b * C + c;
    const float *dr = du + row * (size_t)NP;
    const float *yr = y + row * (size_t)NP * (POOL ? K : 1);
    const int p0 = part * L3D_GN_BWD_CHUNK, p1 = (int)min((long)p0 + L3D_GN_BWD_CHUNK, (long)NP);
    double s1 = 0.0, s2 = 0.0;
    if (VEC) {
        for (int p = p0 + tid * 4; p < p1; p += 1024) {          // NP % 4 == 0: a trip is whole
            const float4 d4 = *(const float4 *)(dr + p), y4 = *(const float4 *)(yr + p);
            const float dv[4] = {d4.x, d4.y, d4.z, d4.w}, yv[4] = {y4.x, y4.y, y4.z, y4.w};
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const double g = fmaf(r.a, yv[e], r.s) > 0.f ? (double)dv[e] : 0.0;
                s1 += g;
                s2 += g * (((double)yv[e] - r.mean) * r.rstd);
            }
        }
    } else {
        for (int p = p0 + tid; p < p1; p += 256) {
            float yv;
            if (POOL) yv = yr[(size_t)min((int)widx[row * NP + p], K - 1) * NP + p];
            else yv = yr[p];
            const double g = fmaf(r.a, yv, r.s) > 0.f ? (double)dr[p] : 0.0;
            s1 += g;
            s2 += g * (((double)yv - r.mean) * r.rstd);
        }
    }
    s1 = l3d_block_sum(s1, sRed);
    s2 = l3d_block_sum(s2, sRed);
    if (tid == 0) {
        double *o = out + (row * nparts + part) * 2;
        o[0] = s1;
        o[1] = s2;
    }
}

// part[row][q] = the row's chunks in ascending order; a thread per (row, q)
__global__ __launch_bounds__(256) void gn_backward_parts_kernel(const double *__restrict__ ws, long rows, int nparts,
                                                                double *__restrict__ part)
{
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= rows * 2) return;
    const long row = e >> 1;
    const int q = (int)(e & 1);
    double s = 0.0;
    for (int p = 0; p < nparts; p++) s += ws[(row * nparts + p) * 2 + q];
    part[e] = s;
}

// the checks every streaming entry point shares; P % K is an argument error, the rest a shape the kernels are not built for
static int gt_check(int B, int C, int groups, int P, int K)
{
    if (K < 0 || (K > 0 && P % K)) return L3D_ERR_INVALID_ARG;
    if (C % groups || K > L3D_PPF_MAX_K || B > 65535 || C > 65535 || P > L3D_GN_BWD_MAX_P) return L3D_ERR_UNSUPPORTED;
    return L3D_OK;
}

extern "C" size_t l3d_gn_backward_workspace_bytes(int B, int C, int P)
{
    if (B <= 0 || C <= 0 || P <= 0) return 0;
    return (size_t)B * C * l3d_divup(P, L3D_GN_BWD_CHUNK) * 2 * sizeof(double);      // pooled or not, never more than this
}

extern "C" int l3d_gn_backward_stats(const float *du, const unsigned char *widx, int K, const float *y, const float *in_a,
                                     const float *in_s, const double *stat, int B, int C, int groups, int P, double *part,
                                     void *workspace, l3d_stream_t stream)
{
    L3D_REQUIRE(du && y && in_a && in_s && stat && part && workspace && B > 0 && C > 0 && groups > 0 && P > 0);
    L3D_REQUIRE((K > 0) == (widx != nullptr));
    const int st = gt_check(B, C, groups, P, K);
    if (st != L3D_OK) return st;
    const int NP = K > 0 ? P / K : P, nparts = l3d_divup(NP, L3D_GN_BWD_CHUNK);
    double *out = nparts == 1 ? part : (double *)workspace;
    const dim3 grid(nparts, C, B);
    if (K > 0)
        hipLaunchKernelGGL((gn_backward_stats_kernel<false, true>), grid, dim3(256), 0, (hipStream_t)stream, du, widx, K, y, in_a, in_s,
                           stat, C, groups, NP, nparts, out);
    else if (P % 4 == 0 && gt_aligned(du, 16) && gt_aligned(y, 16))
        hipLaunchKernelGGL((gn_backward_stats_kernel<true, false>), grid, dim3(256), 0, (hipStream_t)stream, du, widx, K, y, in_a, in_s,
                           stat, C, groups, NP, nparts, out);
    else
        hipLaunchKernelGGL((gn_backward_stats_kernel<false, false>), grid, dim3(256), 0, (hipStream_t)stream, du, widx, K, y, in_a, in_s,
                           stat, C, groups, NP, nparts, out);
    int err = l3d_check_launch();
    if (err != L3D_OK || nparts == 1) return err;
    const long rows = (long)B * C;
    hipLaunchKernelGGL(gn_backward_parts_kernel, dim3(l3d_divup(rows * 2, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const double *)workspace, rows, nparts, part);
    return l3d_check_launch();
}

// ------------------------------------------------------------------------------------------------------------------------------
// thread e < B groups: (M1, M2) of (cloud, group) e; thread e < C: dgamma, dbeta of channel e
__global__ __launch_bounds__(256) void gn_backward_reduce_kernel(const double *__restrict__ part, const float *__restrict__ gamma, int B,
                                                                 int C, int groups, double count, double *__restrict__ m,
                                                                 float *__restrict__ dgamma, float *__restrict__ dbeta)
{
    const int e = blockIdx.x * 256 + threadIdx.x, cpg = C / groups;
    if (e < B * groups) {
        const int b = e / groups, grp = e - b * groups;
        double m1 = 0.0, m2 = 0.0;
        for (int c = grp * cpg; c < (grp + 1) * cpg; c++) {
            const double *pr = part + ((size_t)b * C + c) * 2;
            const double gm = (double)gamma[c];
            m1 += gm * pr[0];
            m2 += gm * pr[1];
        }
        const double n = count * cpg;
        m[(size_t)e * 2] = m1 / n;
        m[(size_t)e * 2 + 1] = m2 / n;
    }
    if (e < C && (dgamma || dbeta)) {
        double t1 = 0.0, t2 = 0.0;
        for (int b = 0; b < B; b++) {
            const double *pr = part + ((size_t)b * C + e) * 2;
            t1 += pr[0];
            t2 += pr[1];
        }
        if (dbeta) dbeta[e] = (float)t1;
        if (dgamma) dgamma[e] = (float)t2;
    }
}

extern "C" int l3d_gn_backward_reduce(const double *part, const float *gamma, int B, int C, int groups, int count, double *m,
                                      float *dgamma, float *dbeta, l3d_stream_t stream)
{
    L3D_REQUIRE(part && gamma && m && B > 0 && C > 0 && groups > 0 && count > 0);
    if (C % groups || B > 65535 || C > 65535) return L3D_ERR_UNSUPPORTED;
    const long threads = (long)B * groups > C ? (long)B * groups : C;
    hipLaunchKernelGGL(gn_backward_reduce_kernel, dim3(l3d_divup(threads, 256)), dim3(256), 0, (hipStream_t)stream, part, gamma, B, C,
                       groups, (double)count, m, dgamma, dbeta);
    return l3d_check_launch();
}

// ------------------------------------------------------------------------------------------------------------------------------
// position p = k NP + n (dense: k = 0, NP = P).  grid (Kk nb, C, B) with nb blocks along n; VEC: four n per lane (NP % 4 == 0).
template <bool VEC, bool POOL>
__global__ __launch_bounds__(256) void gn_backward_apply_kernel(const float *__restrict__ du, const unsigned char *__restrict__ widx,
                                                                const float *__restrict__ y, const float *__restrict__ in_a,
                                                                const float *__restrict__ in_s, const double *__restrict__ stat,
                                                                const float *__restrict__ gamma, const double *__restrict__ m, int C,
                                                                int groups, int NP, int Kk, int nb, float *__restrict__ dz)
{
    const int c = blockIdx.y, b = blockIdx.z;
    const int k = POOL ? blockIdx.x / nb : 0, j = POOL ? blockIdx.x - k * nb : blockIdx.x;
    const int n = (j * 256 + threadIdx.x) * (VEC ? 4 : 1);
    if (n >= NP) return;
    const GtRow r = gt_row(in_a, in_s, stat, b, c, C, groups);
    const double *mg = m + ((size_t)b * groups + c / (C / groups)) * 2;
    const double gam = (double)gamma[c], m1 = mg[0], m2 = mg[1];
    const size_t row = (size_t)b * C + c, at = row * (size_t)NP * Kk + (size_t)k * NP + n, pat = row * (size_t)NP + n;
    if (VEC) {
        const float4 y4 = *(const float4 *)(y + at), d4 = *(const float4 *)(du + pat);
        const float yv[4] = {y4.x, y4.y, y4.z, y4.w};
        float dv[4] = {d4.x, d4.y, d4.z, d4.w}, o[4];
        if (POOL) {
            const unsigned w4 = *(const unsigned *)(widx + pat);
#pragma unroll
            for (int e = 0; e < 4; e++) dv[e] = (int)((w4 >> (8 * e)) & 255u) == k ? dv[e] : 0.f;
        }
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const double g = fmaf(r.a, yv[e], r.s) > 0.f ? (double)dv[e] : 0.0;
            o[e] = (float)(r.rstd * ((gam * g - m1) - (((double)yv[e] - r.mean) * r.rstd) * m2));
        }
        *(float4 *)(dz + at) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
        const float yv = y[at];
        float dv = du[pat];
        if (POOL) dv = (int)widx[pat] == k ? dv : 0.f;
        const double g = fmaf(r.a, yv, r.s) > 0.f ? (double)dv : 0.0;
        dz[at] = (float)(r.rstd * ((gam * g - m1) - (((double)yv - r.mean) * r.rstd) * m2));
    }
}

extern "C" int l3d_gn_backward_apply(const float *du, const unsigned char *widx, int K, const float *y, const float *in_a,
                                     const float *in_s, const double *stat, const float *gamma, const double *m, int B, int C,
                                     int groups, int P, float *dz, l3d_stream_t stream)
{
    L3D_REQUIRE(du && y && in_a && in_s && stat && gamma && m && dz && B > 0 && C > 0 && groups > 0 && P > 0);
    L3D_REQUIRE((K > 0) == (widx != nullptr));
    const int st = gt_check(B, C, groups, P, K);
    if (st != L3D_OK) return st;
    const int Kk = K > 0 ? K : 1, NP = P / Kk;
    const bool vec = NP % 4 == 0 && gt_aligned(du, 16) && gt_aligned(y, 16) && gt_aligned(dz, 16) && gt_aligned(widx, 4);
    const int nb = l3d_divup(NP, vec ? 1024 : 256);
    const dim3 grid((unsigned)Kk * nb, C, B);
#define GT_APPLY(V, Q)                                                                                                                  \
    hipLaunchKernelGGL((gn_backward_apply_kernel<V, Q>), grid, dim3(256), 0, (hipStream_t)stream, du, widx, y, in_a, in_s, stat, gamma, \
                       m, C, groups, NP, Kk, nb, dz)
    if (K > 0) {
        if (vec) GT_APPLY(true, true);
        else GT_APPLY(false, true);
    } else {
        if (vec) GT_APPLY(true, false);
        else GT_APPLY(false, false);
    }
#undef GT_APPLY
    return l3d_check_launch();
}
