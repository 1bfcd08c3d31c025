// rpmnet.hip -- the kernels of RPMNet and its feature network PPFNet (models/rpmnet.py, models/ppfnet.py) that no other kernel of
// the library serves (include/ext/l3d_rpmnet.h):
//
//   l3d_ppf_group      sample_and_group_multi's features behind the ball query, channel-first [B,10,K,N] as the pre-pool stack reads
//                      them: a lane per (n, k), lanes along n so that every channel row is written in runs.  Geometry in fp64.
//   l3d_gn_conv        1x1 convolution whose operand is the previous GroupNorm + ReLU applied on load and whose epilogue sums the
//                      next GroupNorm's raw moments (fp64) and, pooled, keeps the maximum and minimum over the K neighbours: the
//                      [B,C,K,N] activations of the pre-pool stack are read once and written at most once per layer, the last one
//                      never.  A workgroup owns 64 output channels and walks blocks of 64 positions; the tile itself is gn_tile
//                      (gn_tile.h), which rpmnet_param.hip's kernels call too; the epilogue is this file's.
//   l3d_gn_affine      moments -> the per-(cloud, channel) scale and shift of the GroupNorm (the group's mean and rstd: gn_tile.h).
//   l3d_sinkhorn_slack the slack Sinkhorn as two potentials: a row pass (a wave per row), a column pass (64 columns per workgroup,
//                      4 row slices merged through LDS) and one output pass.  One-pass logsumexp in fp64.
//   l3d_rigid_transform_weighted   weighted Kabsch, one workgroup per cloud, the 3x3 SVD of svd3x3.h in thread 0.
#include "common.h"
#include "gn_tile.h"
#include "svd3x3.h"
#include "../../include/ext/l3d_rpmnet.h"

// ------------------------------------------------------------------------------------------------------------------------------
#define PPF_THREADS 256

__device__ __forceinline__ double ppf_angle(double ax, double ay, double az, double bx, double by, double bz)
{
    const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
    // + 0.0: a sum of -0 products (a zero d against negative normal components) must be +0, as torch.sum's is: atan2(0, -0) is pi
    return atan2(sqrt((cx * cx + cy * cy) + cz * cz), ((ax * bx + ay * by) + az * bz) + 0.0);
}

__global__ __launch_bounds__(PPF_THREADS) void ppf_group_kernel(const float *__restrict__ xyz, const float *__restrict__ normals,
                                                                const int64_t *__restrict__ idx, int N, int K, float *__restrict__ feat)
{
    const int n = blockIdx.x * PPF_THREADS + threadIdx.x, k = blockIdx.y, b = blockIdx.z;
    if (n >= N) return;
    const float *xb = xyz + (size_t)b * N * 3;
    long long q = idx[((size_t)b * N + n) * K + k];
    q = q < 0 ? 0 : (q >= N ? N - 1 : q);
    const float cx = xb[(size_t)n * 3], cy = xb[(size_t)n * 3 + 1], cz = xb[(size_t)n * 3 + 2];
    const double dx = (double)xb[(size_t)q * 3] - cx, dy = (double)xb[(size_t)q * 3 + 1] - cy, dz = (double)xb[(size_t)q * 3 + 2] - cz;
    double rx = 0, ry = 0, rz = 0, ix = 0, iy = 0, iz = 0;
    if (normals) {
        const float *nb = normals + (size_t)b * N * 3;
        rx = nb[(size_t)n * 3]; ry = nb[(size_t)n * 3 + 1]; rz = nb[(size_t)n * 3 + 2];
        ix = nb[(size_t)q * 3]; iy = nb[(size_t)q * 3 + 1]; iz = nb[(size_t)q * 3 + 2];
    }
    const float o[10] = {cx, cy, cz, (float)dx, (float)dy, (float)dz,
                         (float)ppf_angle(rx, ry, rz, dx, dy, dz), (float)ppf_angle(ix, iy, iz, dx, dy, dz),
                         (float)ppf_angle(rx, ry, rz, ix, iy, iz), (float)sqrt((dx * dx + dy * dy) + dz * dz)};
    float *f = feat + ((size_t)b * 10 * K + k) * N + n;
#pragma unroll
    for (int c = 0; c < 10; c++) f[(size_t)c * K * N] = o[c];
}

extern "C" int l3d_ppf_group(const float *xyz, const float *normals, const int64_t *idx, int B, int N, int K, float *feat,
                             l3d_stream_t stream)
{
    L3D_REQUIRE(xyz && idx && feat && B > 0 && N > 0 && K > 0);
    if (K > L3D_PPF_MAX_K || B > 65535) return L3D_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(ppf_group_kernel, dim3(l3d_divup(N, PPF_THREADS), K, B), dim3(PPF_THREADS), 0, (hipStream_t)stream, xyz,
                       normals, idx, N, K, feat);
    return l3d_check_launch();
}

// ------------------------------------------------------------------------------------------------------------------------------
struct GcPlan {
    int K, NP, nblocks, bpp, nparts;
};

static GcPlan gc_plan(int P, int pool)
{
    GcPlan g;
    g.K = pool > 0 ? pool : 1;
    g.NP = P / g.K;
    g.nblocks = l3d_divup(g.NP, GN_TP);
    g.bpp = l3d_divup(g.nblocks, L3D_GN_CONV_PARTS);
    g.nparts = l3d_divup(g.nblocks, g.bpp);
    return g;
}

// position p = k NP + c: k < K the pooled axis (K = 1 without pooling), c < NP.  grid (nparts, ceil(Cout / 64), B).
__global__ __launch_bounds__(256) void gn_conv_kernel(const float *__restrict__ x, const float *__restrict__ in_a,
                                                      const float *__restrict__ in_s, const float *__restrict__ w,
                                                      const float *__restrict__ bias, int Cin, int Cout, int P, int K, int NP,
                                                      int nblocks, int bpp, int nparts, float *__restrict__ y,
                                                      float *__restrict__ ymax, float *__restrict__ ymin, double *__restrict__ partials)
{
    __shared__ float sW[GN_TC * GN_LDW];               // [co][ci]
    __shared__ float sU[GN_TC * GN_LDU];               // [ci][position]
    const GnCtx cx = gn_ctx(Cin, Cout);
    const int part = blockIdx.x, b = cx.b, cow = cx.cow, g = cx.g, m = cx.m;
    const bool wave_on = cx.wave_on;
    const float *xb = x + (size_t)b * Cin * P;

    float bv[4];
#pragma unroll
    for (int r = 0; r < 4; r++) bv[r] = (wave_on && bias) ? bias[cow + 4 * g + r] : 0.f;
    double s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};

    gn_weights_once(cx, w, Cin, Cout, sW);

    const int cb_end = min((part + 1) * bpp, nblocks);
    for (int cb = part * bpp; cb < cb_end; cb++) {
        const int c0 = cb * GN_TP;
        float mx[4][4], mn[4][4];
#pragma unroll
        for (int t = 0; t < 4; t++)
#pragma unroll
            for (int r = 0; r < 4; r++) { mx[t][r] = -INFINITY; mn[t][r] = INFINITY; }

        for (int k = 0; k < K; k++) {
            f32x4 acc[4];
            gn_tile(cx, xb, in_a, in_s, w, bv, Cin, Cout, P, (size_t)k * NP + c0, c0, NP, sW, sU, acc);

            // acc[t][r] = output channel cow + 4 g + r at column c0 + 16 t + m of level k
            if (wave_on) {
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    const int c = c0 + 16 * t + m;
                    if (c < NP) {
#pragma unroll
                        for (int r = 0; r < 4; r++) {
                            const float v = acc[t][r];
                            if (y) y[((size_t)b * Cout + cow + 4 * g + r) * P + (size_t)k * NP + c] = v;
                            s1[r] += (double)v;
                            s2[r] += (double)v * (double)v;
                            mx[t][r] = fmaxf(mx[t][r], v);
                            mn[t][r] = fminf(mn[t][r], v);
                        }
                    }
                }
            }
        }

        if (wave_on && ymax) {
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const int c = c0 + 16 * t + m;
                if (c < NP) {
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const size_t at = ((size_t)b * Cout + cow + 4 * g + r) * NP + c;
                        ymax[at] = mx[t][r];
                        ymin[at] = mn[t][r];
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
        }
    }
    if (wave_on && m == 0) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            double *o = partials + (((size_t)b * Cout + cow + 4 * g + r) * nparts + part) * 2;
            o[0] = s1[r];
            o[1] = s2[r];
        }
    }
}

// moments[row][q] = the row's partials in ascending order; a thread per (row, q)
__global__ __launch_bounds__(256) void gn_moments_kernel(const double *__restrict__ partials, long rows, int nparts,
                                                         double *__restrict__ moments)
{
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= rows * 2) return;
    const long row = e >> 1;
    const int q = (int)(e & 1);
    double s = 0.0;
    for (int p = 0; p < nparts; p++) s += partials[(row * nparts + p) * 2 + q];
    moments[e] = s;
}

extern "C" size_t l3d_gn_conv_workspace_bytes(int B, int Cout, int P)
{
    if (B <= 0 || Cout <= 0 || P <= 0) return 0;
    const long blocks = l3d_divup(P, GN_TP), parts = blocks < L3D_GN_CONV_PARTS ? blocks : L3D_GN_CONV_PARTS;      // pooled or not, never more than this
    return (size_t)B * Cout * parts * 2 * sizeof(double);
}

extern "C" int l3d_gn_conv(const float *x, const float *in_a, const float *in_s, const float *w, const float *bias, int B, int Cin,
                           int Cout, int P, int pool, float *y, float *ymax, float *ymin, double *moments, void *workspace,
                           l3d_stream_t stream)
{
    L3D_REQUIRE(x && w && moments && workspace && B > 0 && Cin > 0 && Cout > 0 && P > 0 && pool >= 0);
    L3D_REQUIRE((in_a == nullptr) == (in_s == nullptr));
    if (pool > 0) L3D_REQUIRE(ymax && ymin && P % pool == 0);
    else L3D_REQUIRE(y);
    if (Cout % 16 || Cout > L3D_GN_CONV_MAX_COUT || Cin > L3D_GN_CONV_MAX_CIN || B > 65535) return L3D_ERR_UNSUPPORTED;
    const GcPlan g = gc_plan(P, pool);
    hipLaunchKernelGGL(gn_conv_kernel, dim3(g.nparts, l3d_divup(Cout, 64), B), dim3(256), 0, (hipStream_t)stream, x, in_a, in_s, w,
                       bias, Cin, Cout, P, g.K, g.NP, g.nblocks, g.bpp, g.nparts, y, pool > 0 ? ymax : nullptr,
                       pool > 0 ? ymin : nullptr, (double *)workspace);
    int st = l3d_check_launch();
    if (st != L3D_OK) return st;
    const long rows = (long)B * Cout;
    hipLaunchKernelGGL(gn_moments_kernel, dim3(l3d_divup(rows * 2, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const double *)workspace, rows, g.nparts, moments);
    return l3d_check_launch();
}

// ------------------------------------------------------------------------------------------------------------------------------
// a wave per (cloud, group)
__global__ __launch_bounds__(64) void gn_affine_kernel(const double *__restrict__ moments, const float *__restrict__ gamma,
                                                       const float *__restrict__ beta, int C, int groups, double count, double eps,
                                                       float *__restrict__ a, float *__restrict__ s)
{
    const int lane = threadIdx.x, grp = blockIdx.x, b = blockIdx.y, cpg = C / groups;
    double mean, rstd;
    gn_group_stats(moments, b, C, groups, grp, lane, count, eps, mean, rstd);
    for (int c = lane; c < cpg; c += 64) {
        const int ch = grp * cpg + c;
        const double av = (double)gamma[ch] * rstd;
        a[(size_t)b * C + ch] = (float)av;
        s[(size_t)b * C + ch] = (float)((double)beta[ch] - mean * av);
    }
}

extern "C" int l3d_gn_affine(const double *moments, const float *gamma, const float *beta, int B, int C, int groups, int count,
                             float eps, float *a, float *s, l3d_stream_t stream)
{
    L3D_REQUIRE(moments && gamma && beta && a && s && B > 0 && C > 0 && groups > 0 && count > 0);
    if (C % groups || B > 65535) return L3D_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(gn_affine_kernel, dim3(groups, B), dim3(64), 0, (hipStream_t)stream, moments, gamma, beta, C, groups,
                       (double)count, (double)eps, a, s);
    return l3d_check_launch();
}

// ------------------------------------------------------------------------------------------------------------------------------
// running logsumexp: (m, s) stands for m + log(s); the empty state is (-inf, 0)
struct Lse {
    double m, s;
};

__device__ __forceinline__ void lse_add(Lse &a, double t)
{
    if (t > a.m) {
        a.s = a.s * exp(a.m - t) + 1.0;                // exp(-inf) = 0 on the first element
        a.m = t;
    } else {
        a.s += exp(t - a.m);
    }
}

__device__ __forceinline__ Lse lse_merge(Lse a, Lse b)
{
    Lse o;
    o.m = fmax(a.m, b.m);
    if (o.m == -INFINITY) {
        o.s = 0.0;
        return o;
    }
    o.s = a.s * exp(a.m - o.m) + b.s * exp(b.m - o.m);
    return o;
}

__global__ __launch_bounds__(256) void sk_init_kernel(double *__restrict__ pot, long n)
{
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e < n) pot[e] = 0.0;
}

// u[j] = logsumexp_k (A[j,k] - v[k]) over k = 0..K, the slack column contributing A = 0, v = 0.  A wave per row.
__global__ __launch_bounds__(256) void sk_row_kernel(const float *__restrict__ A, int J, int K, double *__restrict__ u,
                                                     const double *__restrict__ v)
{
    const int lane = threadIdx.x & 63, j = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
    if (j >= J) return;
    const float *row = A + ((size_t)b * J + j) * K;
    const double *vb = v + (size_t)b * K;
    Lse acc = {-INFINITY, 0.0};
    for (int k = lane; k < K; k += 64) lse_add(acc, (double)row[k] - vb[k]);
    if (lane == 0) lse_add(acc, 0.0);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        Lse o;
        o.m = __shfl_xor(acc.m, off, 64);
        o.s = __shfl_xor(acc.s, off, 64);
        acc = lse_merge(acc, o);
    }
    if (lane == 0) u[(size_t)b * J + j] = acc.m + log(acc.s);
}

// v[k] = logsumexp_j (A[j,k] - u[j]) over j = 0..J, the slack row contributing 0.  64 columns per workgroup, 4 row slices.
__global__ __launch_bounds__(256) void sk_col_kernel(const float *__restrict__ A, int J, int K, const double *__restrict__ u,
                                                     double *__restrict__ v)
{
    __shared__ double sM[4][64], sS[4][64];
    const int kx = threadIdx.x & 63, jy = threadIdx.x >> 6, k = blockIdx.x * 64 + kx, b = blockIdx.y;
    const float *Ab = A + (size_t)b * J * K;
    const double *ub = u + (size_t)b * J;
    Lse acc = {-INFINITY, 0.0};
    if (k < K)
        for (int j = jy; j < J; j += 4) lse_add(acc, (double)Ab[(size_t)j * K + k] - ub[j]);
    sM[jy][kx] = acc.m;
    sS[jy][kx] = acc.s;
    __syncthreads();
    if (jy == 0 && k < K) {
        Lse t = {0.0, 1.0};                            // the slack row
        for (int q = 0; q < 4; q++) {
            Lse o = {sM[q][kx], sS[q][kx]};
            t = lse_merge(t, o);
        }
        v[(size_t)b * K + k] = t.m + log(t.s);
    }
}

// log_perm = A - u - v, perm = exp(log_perm), their row sums and the weighted reference points.  A wave per row.
__global__ __launch_bounds__(256) void sk_out_kernel(const float *__restrict__ A, int J, int K, const double *__restrict__ u,
                                                     const double *__restrict__ v, const float *__restrict__ xyz_ref, double eps,
                                                     float *__restrict__ log_perm, float *__restrict__ perm,
                                                     float *__restrict__ rowsum, float *__restrict__ weighted)
{
    const int lane = threadIdx.x & 63, j = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
    if (j >= J) return;
    const size_t at = ((size_t)b * J + j) * K;
    const double uj = u[(size_t)b * J + j];
    const double *vb = v + (size_t)b * K;
    double rs = 0.0, wx = 0.0, wy = 0.0, wz = 0.0;
    for (int k = lane; k < K; k += 64) {
        const float lp = (float)(((double)A[at + k] - uj) - vb[k]);
        if (log_perm) log_perm[at + k] = lp;
        if (perm || rowsum || weighted) {
            const float pv = (float)exp((double)lp);   // exp of the rounded logarithm, as the reference's torch.exp(log_perm)
            if (perm) perm[at + k] = pv;
            rs += (double)pv;
            if (weighted) {
                const float *q = xyz_ref + ((size_t)b * K + k) * 3;
                wx += (double)pv * q[0]; wy += (double)pv * q[1]; wz += (double)pv * q[2];
            }
        }
    }
    if (rowsum || weighted) {
        rs = l3d_wave_sum(rs);
        if (rowsum && lane == 0) rowsum[(size_t)b * J + j] = (float)rs;
        if (weighted) {
            wx = l3d_wave_sum(wx); wy = l3d_wave_sum(wy); wz = l3d_wave_sum(wz);
            if (lane == 0) {
                // the reference divides by the fp32 row sum plus eps
                const double den = (double)(float)rs + eps;
                float *o = weighted + ((size_t)b * J + j) * 3;
                o[0] = (float)(wx / den); o[1] = (float)(wy / den); o[2] = (float)(wz / den);
            }
        }
    }
}

extern "C" size_t l3d_sinkhorn_workspace_bytes(int B, int J, int K)
{
    if (B <= 0 || J <= 0 || K <= 0) return 0;
    return (size_t)B * ((size_t)J + K) * sizeof(double);
}

extern "C" int l3d_sinkhorn_slack(const float *log_alpha, int B, int J, int K, int n_iters, const float *xyz_ref, float eps,
                                  float *log_perm, float *perm, float *rowsum, float *weighted, void *workspace, l3d_stream_t stream)
{
    L3D_REQUIRE(log_alpha && workspace && B > 0 && J > 0 && K > 0);
    L3D_REQUIRE(log_perm || perm || rowsum || weighted);
    L3D_REQUIRE(!weighted || xyz_ref);
    if (n_iters < 0 || B > 65535) return L3D_ERR_UNSUPPORTED;
    double *u = (double *)workspace, *v = u + (size_t)B * J;
    const long n = (long)B * ((long)J + K);
    hipLaunchKernelGGL(sk_init_kernel, dim3(l3d_divup(n, 256)), dim3(256), 0, (hipStream_t)stream, u, n);
    for (int it = 0; it < n_iters; it++) {
        hipLaunchKernelGGL(sk_row_kernel, dim3(l3d_divup(J, 4), B), dim3(256), 0, (hipStream_t)stream, log_alpha, J, K, u, v);
        hipLaunchKernelGGL(sk_col_kernel, dim3(l3d_divup(K, 64), B), dim3(256), 0, (hipStream_t)stream, log_alpha, J, K, u, v);
    }
    hipLaunchKernelGGL(sk_out_kernel, dim3(l3d_divup(J, 4), B), dim3(256), 0, (hipStream_t)stream, log_alpha, J, K, u, v, xyz_ref,
                       (double)eps, log_perm, perm, rowsum, weighted);
    return l3d_check_launch();
}

// ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rigid_weighted_kernel(const float *__restrict__ a, const float *__restrict__ bpts,
                                                             const float *__restrict__ weights, int M, double eps, float *__restrict__ T)
{
    __shared__ double sRed[4];
    const int tid = threadIdx.x, b = blockIdx.x;
    const float *ab = a + (size_t)b * M * 3, *bb = bpts + (size_t)b * M * 3, *wb = weights + (size_t)b * M;
    double acc[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int i = tid; i < M; i += 256) {
        const double w = wb[i];
        acc[0] += w;
#pragma unroll
        for (int d = 0; d < 3; d++) {
            acc[1 + d] += w * ab[(size_t)i * 3 + d];
            acc[4 + d] += w * bb[(size_t)i * 3 + d];
        }
    }
#pragma unroll
    for (int q = 0; q < 7; q++) acc[q] = l3d_block_sum(acc[q], sRed);
    const double inv = 1.0 / (acc[0] + eps);
    double ca[3], cb[3];
#pragma unroll
    for (int d = 0; d < 3; d++) { ca[d] = acc[1 + d] * inv; cb[d] = acc[4 + d] * inv; }
    double h[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = tid; i < M; i += 256) {
        const double w = (double)wb[i] * inv;
        double da[3], db[3];
#pragma unroll
        for (int d = 0; d < 3; d++) { da[d] = (double)ab[(size_t)i * 3 + d] - ca[d]; db[d] = ((double)bb[(size_t)i * 3 + d] - cb[d]) * w; }
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int q = 0; q < 3; q++) h[r * 3 + q] += da[r] * db[q];
    }
#pragma unroll
    for (int q = 0; q < 9; q++) h[q] = l3d_block_sum(h[q], sRed);
    if (tid == 0) {
        float r[9];
        rotation_from_H(h, r);
        float *o = T + (size_t)b * 12;
#pragma unroll
        for (int q = 0; q < 3; q++) {
#pragma unroll
            for (int d = 0; d < 3; d++) o[q * 4 + d] = r[q * 3 + d];
            o[q * 4 + 3] = (float)(cb[q] - (((double)r[q * 3] * ca[0] + (double)r[q * 3 + 1] * ca[1]) + (double)r[q * 3 + 2] * ca[2]));
        }
    }
}

extern "C" int l3d_rigid_transform_weighted(const float *a, const float *b, const float *weights, int B, int M, float eps, float *T,
                                            l3d_stream_t stream)
{
    L3D_REQUIRE(a && b && weights && T && B > 0 && M > 0);
    if (B > 65535) return L3D_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(rigid_weighted_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, a, b, weights, M, (double)eps, T);
    return l3d_check_launch();
}
