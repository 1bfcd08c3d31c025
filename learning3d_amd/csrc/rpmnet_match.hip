// rpmnet_match.hip -- RPMNet's matching stage under autograd (include/ext/l3d_rpmnet_match.h; models/rpmnet.py RPMNet._Match):
//
//   l3d_sinkhorn_slack_keep      l3d_sinkhorn_slack (rpmnet.hip) with the potentials of every iteration written out.  The kernels
//                                repeat that file's row, column and output pass sum for sum (the same lanes take the same columns, the
//                                same merges in the same order), so the four outputs are the same bits; only the addressing of the
//                                potentials differs: [n, B, J + K], a stride of J + K per cloud.
//   l3d_sinkhorn_slack_backward  the reverse sweep from those potentials.  Every half step is one row reduction (a wave per row, four
//                                rows per workgroup) or one column reduction (64 columns per workgroup, 4 row slices added through LDS
//                                in slice order) over log_alpha; the adjoints of the potentials are vectors in the workspace, and the
//                                dense gradient is written once by the output pass.  fp64 throughout, no atomics.
// The row kernels come in two forms: W = 4 moves 16 bytes per lane (K % 4 == 0 and every [B,J,K] pointer the kernel touches on 16
// bytes), W = 1 is the scalar route.
#include "common.h"
#include "../../include/ext/l3d_rpmnet_match.h"

// running logsumexp, as rpmnet.hip's: (m, s) stands for m + log(s); the empty state is (-inf, 0)
struct MtLse {
    double m, s;
};

__device__ __forceinline__ void mt_lse_add(MtLse &a, double t)
{
    if (t > a.m) {
        a.s = a.s * exp(a.m - t) + 1.0;
        a.m = t;
    } else {
        a.s += exp(t - a.m);
    }
}

__device__ __forceinline__ MtLse mt_lse_merge(MtLse a, MtLse b)
{
    MtLse o;
    o.m = fmax(a.m, b.m);
    if (o.m == -INFINITY) {
        o.s = 0.0;
        return o;
    }
    o.s = a.s * exp(a.m - o.m) + b.s * exp(b.m - o.m);
    return o;
}

template <int W>
__device__ __forceinline__ void mt_load(float (&d)[W], const float *__restrict__ p)
{
    if constexpr (W == 4) {
        const f32x4 t = *reinterpret_cast<const f32x4 *>(p);
        d[0] = t.x; d[1] = t.y; d[2] = t.z; d[3] = t.w;
    } else {
        d[0] = p[0];
    }
}

template <int W>
__device__ __forceinline__ void mt_store(float *__restrict__ p, const float (&d)[W])
{
    if constexpr (W == 4) {
        f32x4 t;
        t.x = d[0]; t.y = d[1]; t.z = d[2]; t.w = d[3];
        *reinterpret_cast<f32x4 *>(p) = t;
    } else {
        p[0] = d[0];
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// the forward.  u, v point at iteration t's potentials of cloud 0; ps = J + K is the stride per cloud; vprev NULL: v_0 = 0
__global__ __launch_bounds__(256) void mt_fwd_row_kernel(const float *__restrict__ A, int J, int K, int ps, double *__restrict__ u,
                                                         const double *__restrict__ vprev)
{
    const int lane = threadIdx.x & 63, j = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
    if (j >= J) return;
    const float *row = A + ((size_t)b * J + j) * K;
    MtLse acc = {-INFINITY, 0.0};
    if (vprev) {
        const double *vb = vprev + (size_t)b * ps;
        for (int k = lane; k < K; k += 64) mt_lse_add(acc, (double)row[k] - vb[k]);
    } else {
        for (int k = lane; k < K; k += 64) mt_lse_add(acc, (double)row[k]);
    }
    if (lane == 0) mt_lse_add(acc, 0.0);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        MtLse o;
        o.m = __shfl_xor(acc.m, off, 64);
        o.s = __shfl_xor(acc.s, off, 64);
        acc = mt_lse_merge(acc, o);
    }
    if (lane == 0) u[(size_t)b * ps + j] = acc.m + log(acc.s);
}

__global__ __launch_bounds__(256) void mt_fwd_col_kernel(const float *__restrict__ A, int J, int K, int ps, const double *__restrict__ u,
                                                         double *__restrict__ v)
{
    __shared__ double sM[4][64], sS[4][64];
    const int kx = threadIdx.x & 63, jy = threadIdx.x >> 6, k = blockIdx.x * 64 + kx, b = blockIdx.y;
    const float *Ab = A + (size_t)b * J * K;
    const double *ub = u + (size_t)b * ps;
    MtLse acc = {-INFINITY, 0.0};
    if (k < K)
        for (int j = jy; j < J; j += 4) mt_lse_add(acc, (double)Ab[(size_t)j * K + k] - ub[j]);
    sM[jy][kx] = acc.m;
    sS[jy][kx] = acc.s;
    __syncthreads();
    if (jy == 0 && k < K) {
        MtLse t = {0.0, 1.0};                          // the slack row
        for (int q = 0; q < 4; q++) {
            MtLse o = {sM[q][kx], sS[q][kx]};
            t = mt_lse_merge(t, o);
        }
        v[(size_t)b * ps + k] = t.m + log(t.s);
    }
}

// u, v: the last iteration's potentials of cloud 0, or both NULL (n = 0: zeros)
__global__ __launch_bounds__(256) void mt_fwd_out_kernel(const float *__restrict__ A, int J, int K, int ps, const double *__restrict__ u,
                                                         const double *__restrict__ v, const float *__restrict__ xyz_ref, double eps,
                                                         float *__restrict__ log_perm, float *__restrict__ perm,
                                                         float *__restrict__ rowsum, float *__restrict__ weighted)
{
    const int lane = threadIdx.x & 63, j = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
    if (j >= J) return;
    const size_t at = ((size_t)b * J + j) * K;
    const double uj = u ? u[(size_t)b * ps + j] : 0.0;
    const double *vb = v ? v + (size_t)b * ps : nullptr;
    double rs = 0.0, wx = 0.0, wy = 0.0, wz = 0.0;
    for (int k = lane; k < K; k += 64) {
        const float lp = (float)(((double)A[at + k] - uj) - (vb ? vb[k] : 0.0));
        if (log_perm) log_perm[at + k] = lp;
        if (perm || rowsum || weighted) {
            const float pv = (float)exp((double)lp);
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
                const double den = (double)(float)rs + eps;
                float *o = weighted + ((size_t)b * J + j) * 3;
                o[0] = (float)(wx / den); o[1] = (float)(wy / den); o[2] = (float)(wz / den);
            }
        }
    }
}

extern "C" int l3d_sinkhorn_slack_keep(const float *log_alpha, int B, int J, int K, int n_iters, const float *xyz_ref, float eps,
                                       float *log_perm, float *perm, float *rowsum, float *weighted, double *potentials,
                                       l3d_stream_t stream)
{
    L3D_REQUIRE(log_alpha && B > 0 && J > 0 && K > 0);
    L3D_REQUIRE(log_perm || perm || rowsum || weighted);
    L3D_REQUIRE(!weighted || xyz_ref);
    if (n_iters < 0 || B > 65535) return L3D_ERR_UNSUPPORTED;
    L3D_REQUIRE(potentials || n_iters == 0);
    const int ps = J + K;
    const size_t per_t = (size_t)B * ps;
    hipStream_t s = (hipStream_t)stream;
    for (int t = 0; t < n_iters; t++) {
        double *u = potentials + t * per_t, *v = u + J;
        const double *vprev = t ? v - per_t : nullptr;
        hipLaunchKernelGGL(mt_fwd_row_kernel, dim3(l3d_divup(J, 4), B), dim3(256), 0, s, log_alpha, J, K, ps, u, vprev);
        hipLaunchKernelGGL(mt_fwd_col_kernel, dim3(l3d_divup(K, 64), B), dim3(256), 0, s, log_alpha, J, K, ps, u, v);
    }
    const double *un = n_iters ? potentials + (n_iters - 1) * per_t : nullptr;
    hipLaunchKernelGGL(mt_fwd_out_kernel, dim3(l3d_divup(J, 4), B), dim3(256), 0, s, log_alpha, J, K, ps, un, un ? un + J : nullptr,
                       xyz_ref, (double)eps, log_perm, perm, rowsum, weighted);
    return l3d_check_launch();
}

// ------------------------------------------------------------------------------------------------------------------------------
// the backward.  rowstat [B,J,4] = (c0, g) per row.

// The first row pass, two sweeps of the row: r and P x, from them c0 and g, then ubar_n = -sum_k G[j,k] term by term (the second
// sweep finds its row in the cache).  u, v: the last iteration's potentials (NULL: zeros)
template <int W>
__global__ __launch_bounds__(256) void mt_bwd_first_row_kernel(const float *__restrict__ A, int J, int K, int ps,
                                                               const double *__restrict__ u, const double *__restrict__ v,
                                                               const float *__restrict__ xyz_ref, double eps,
                                                               const float *__restrict__ d_perm, const float *__restrict__ d_rowsum,
                                                               const float *__restrict__ d_weighted, double *__restrict__ rowstat,
                                                               double *__restrict__ ubar_n)
{
    const int lane = threadIdx.x & 63, j = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
    if (j >= J) return;
    const size_t rj = (size_t)b * J + j, at = rj * K;
    const double uj = u ? u[(size_t)b * ps + j] : 0.0;
    const double *vb = v ? v + (size_t)b * ps : nullptr;
    const bool want_x = d_weighted != nullptr;
    double r = 0.0, px = 0.0, py = 0.0, pz = 0.0;
    for (int k0 = lane * W; k0 < K; k0 += 64 * W) {
        float a[W];
        mt_load<W>(a, A + at + k0);
#pragma unroll
        for (int i = 0; i < W; i++) {
            const int k = k0 + i;
            const double p = exp(((double)a[i] - uj) - (vb ? vb[k] : 0.0));
            r += p;
            if (want_x) {
                const float *q = xyz_ref + ((size_t)b * K + k) * 3;
                px += p * (double)q[0]; py += p * (double)q[1]; pz += p * (double)q[2];
            }
        }
    }
    r = l3d_wave_sum(r);
    const double den = r + eps;
    double gx = 0.0, gy = 0.0, gz = 0.0, c0 = 0.0;
    if (want_x) {
        px = l3d_wave_sum(px); py = l3d_wave_sum(py); pz = l3d_wave_sum(pz);
        const float *dw = d_weighted + rj * 3;
        gx = (double)dw[0] / den; gy = (double)dw[1] / den; gz = (double)dw[2] / den;
        c0 = -((gx * (px / den) + gy * (py / den)) + gz * (pz / den));
    }
    if (d_rowsum) c0 += (double)d_rowsum[rj];
    double sg = 0.0;
    for (int k0 = lane * W; k0 < K; k0 += 64 * W) {
        float a[W], dp[W];
        mt_load<W>(a, A + at + k0);
        if (d_perm) mt_load<W>(dp, d_perm + at + k0);
#pragma unroll
        for (int i = 0; i < W; i++) {
            const int k = k0 + i;
            const double p = exp(((double)a[i] - uj) - (vb ? vb[k] : 0.0));
            double t = c0;
            if (want_x) {
                const float *q = xyz_ref + ((size_t)b * K + k) * 3;
                t += (gx * (double)q[0] + gy * (double)q[1]) + gz * (double)q[2];
            }
            if (d_perm) t += (double)dp[i];
            sg += p * t;
        }
    }
    sg = l3d_wave_sum(sg);
    if (lane == 0) {
        double *st = rowstat + rj * 4;
        st[0] = c0; st[1] = gx; st[2] = gy; st[3] = gz;
        ubar_n[rj] = -sg;
    }
}

// vbar_n[k] = -sum_j G[j,k]
__global__ __launch_bounds__(256) void mt_bwd_first_col_kernel(const float *__restrict__ A, int J, int K, int ps,
                                                               const double *__restrict__ u, const double *__restrict__ v,
                                                               const float *__restrict__ xyz_ref, const float *__restrict__ d_perm,
                                                               const double *__restrict__ rowstat, bool want_x,
                                                               double *__restrict__ vbar_n)
{
    __shared__ double sAcc[4][64];
    const int kx = threadIdx.x & 63, jy = threadIdx.x >> 6, k = blockIdx.x * 64 + kx, b = blockIdx.y;
    const float *Ab = A + (size_t)b * J * K;
    double acc = 0.0;
    if (k < K) {
        const double *ub = u + (size_t)b * ps;
        const double vk = v[(size_t)b * ps + k];
        double x0 = 0.0, x1 = 0.0, x2 = 0.0;
        if (want_x) {
            const float *q = xyz_ref + ((size_t)b * K + k) * 3;
            x0 = q[0]; x1 = q[1]; x2 = q[2];
        }
        for (int j = jy; j < J; j += 4) {
            const size_t e = (size_t)j * K + k;
            const double p = exp(((double)Ab[e] - ub[j]) - vk);
            const double *st = rowstat + ((size_t)b * J + j) * 4;
            double t = st[0];
            if (want_x) t += (st[1] * x0 + st[2] * x1) + st[3] * x2;
            if (d_perm) t += (double)d_perm[(size_t)b * J * K + e];
            acc += p * t;
        }
    }
    sAcc[jy][kx] = acc;
    __syncthreads();
    if (jy == 0 && k < K) vbar_n[(size_t)b * K + k] = -(((sAcc[0][kx] + sAcc[1][kx]) + sAcc[2][kx]) + sAcc[3][kx]);
}

// ubar_t[j] = (init ? init[j] : 0) - sum_k vbar_t[k] exp(A[j,k] - u_t[j] - v_t[k])
template <int W>
__global__ __launch_bounds__(256) void mt_bwd_row_kernel(const float *__restrict__ A, int J, int K, int ps, const double *__restrict__ u,
                                                         const double *__restrict__ v, const double *__restrict__ vbar,
                                                         const double *__restrict__ init, double *__restrict__ ubar)
{
    const int lane = threadIdx.x & 63, j = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
    if (j >= J) return;
    const size_t rj = (size_t)b * J + j, at = rj * K;
    const double uj = u[(size_t)b * ps + j];
    const double *vb = v + (size_t)b * ps, *vbb = vbar + (size_t)b * K;
    double acc = 0.0;
    for (int k0 = lane * W; k0 < K; k0 += 64 * W) {
        float a[W];
        mt_load<W>(a, A + at + k0);
#pragma unroll
        for (int i = 0; i < W; i++) acc += vbb[k0 + i] * exp(((double)a[i] - uj) - vb[k0 + i]);
    }
    acc = l3d_wave_sum(acc);
    if (lane == 0) ubar[rj] = (init ? init[rj] : 0.0) - acc;
}

// vbar_{t-1}[k] = -sum_j ubar_t[j] exp(A[j,k] - v_{t-1}[k] - u_t[j]); u = u_t, vprev = v_{t-1}
__global__ __launch_bounds__(256) void mt_bwd_col_kernel(const float *__restrict__ A, int J, int K, int ps, const double *__restrict__ u,
                                                         const double *__restrict__ vprev, const double *__restrict__ ubar,
                                                         double *__restrict__ vbar_prev)
{
    __shared__ double sAcc[4][64];
    const int kx = threadIdx.x & 63, jy = threadIdx.x >> 6, k = blockIdx.x * 64 + kx, b = blockIdx.y;
    const float *Ab = A + (size_t)b * J * K;
    double acc = 0.0;
    if (k < K) {
        const double *ub = u + (size_t)b * ps, *ubb = ubar + (size_t)b * J;
        const double vk = vprev[(size_t)b * ps + k];
        for (int j = jy; j < J; j += 4) acc += ubb[j] * exp(((double)Ab[(size_t)j * K + k] - vk) - ub[j]);
    }
    sAcc[jy][kx] = acc;
    __syncthreads();
    if (jy == 0 && k < K) vbar_prev[(size_t)b * K + k] = -(((sAcc[0][kx] + sAcc[1][kx]) + sAcc[2][kx]) + sAcc[3][kx]);
}

// dA = dAff + G + sum_t (vbar_t Q_t + ubar_t R_t), t ascending, written once; with the fold d_out = -beta dA and the row's partials
// (sum_k dA (dist - alpha), sum_k dA) into part [B,J,2] (NULL: not wanted).  pot: iteration 1's potentials of cloud 0; per_t the
// stride between iterations; ubar [n,B,J], vbar [n,B,K]
template <int W>
__global__ __launch_bounds__(256) void mt_bwd_out_kernel(const float *__restrict__ A, int B, int J, int K, int n, const double *__restrict__ pot,
                                                         const float *__restrict__ xyz_ref, const double *__restrict__ rowstat,
                                                         const double *__restrict__ ubar, const double *__restrict__ vbar,
                                                         const float *__restrict__ d_perm, const float *__restrict__ d_affinity, bool want_x,
                                                         const float *__restrict__ dist, const float *__restrict__ beta,
                                                         const float *__restrict__ alpha, float *__restrict__ d_out, double *__restrict__ part)
{
    const int lane = threadIdx.x & 63, j = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
    if (j >= J) return;
    const int ps = J + K;
    const size_t rj = (size_t)b * J + j, at = rj * K, per_t = (size_t)B * ps;
    const double *st = rowstat + rj * 4;
    const double c0 = st[0], gx = st[1], gy = st[2], gz = st[3];
    const double *pb = pot + (size_t)b * ps;           // u_1 of this cloud; v_1 at + J
    const double un = n ? pb[(n - 1) * per_t + j] : 0.0;
    const double nbeta = dist ? -(double)beta[b] : 0.0, al = dist ? (double)alpha[b] : 0.0;
    double s1 = 0.0, s2 = 0.0;
    for (int k0 = lane * W; k0 < K; k0 += 64 * W) {
        float a[W], dp[W], da[W], dd[W], o[W];
        double p[W], acc[W], vprev[W];
        mt_load<W>(a, A + at + k0);
        if (d_perm) mt_load<W>(dp, d_perm + at + k0);
        if (d_affinity) mt_load<W>(da, d_affinity + at + k0);
        if (dist) mt_load<W>(dd, dist + at + k0);
#pragma unroll
        for (int i = 0; i < W; i++) {
            const int k = k0 + i;
            p[i] = exp(((double)a[i] - un) - (n ? pb[(n - 1) * per_t + J + k] : 0.0));
            double t = c0;
            if (want_x) {
                const float *q = xyz_ref + ((size_t)b * K + k) * 3;
                t += (gx * (double)q[0] + gy * (double)q[1]) + gz * (double)q[2];
            }
            if (d_perm) t += (double)dp[i];
            acc[i] = p[i] * t;
            if (d_affinity) acc[i] += (double)da[i];
            vprev[i] = 0.0;
        }
        for (int t = 1; t <= n; t++) {
            const double ut = pb[(t - 1) * per_t + j], ubt = ubar[(size_t)(t - 1) * B * J + rj];
            const double *vt = pb + (t - 1) * per_t + J, *vbt = vbar + ((size_t)(t - 1) * B + b) * K;
#pragma unroll
            for (int i = 0; i < W; i++) {
                const int k = k0 + i;
                const double vk = vt[k];
                const double q = t == n ? p[i] : exp(((double)a[i] - ut) - vk);          // Q_n is P, term for term
                const double rr = exp(((double)a[i] - vprev[i]) - ut);
                acc[i] += vbt[k] * q + ubt * rr;
                vprev[i] = vk;
            }
        }
#pragma unroll
        for (int i = 0; i < W; i++) {
            if (dist) {
                o[i] = (float)(nbeta * acc[i]);
                s1 += acc[i] * ((double)dd[i] - al);
                s2 += acc[i];
            } else {
                o[i] = (float)acc[i];
            }
        }
        mt_store<W>(d_out + at + k0, o);
    }
    if (part) {
        s1 = l3d_wave_sum(s1);
        s2 = l3d_wave_sum(s2);
        if (lane == 0) {
            part[rj * 2] = s1;
            part[rj * 2 + 1] = s2;
        }
    }
}

// the fold's partials added in ascending row order, a thread per cloud
__global__ __launch_bounds__(64) void mt_bwd_fold_kernel(const double *__restrict__ part, const float *__restrict__ beta, int B, int J,
                                                         float *__restrict__ d_beta, float *__restrict__ d_alpha)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const double *pb = part + (size_t)b * J * 2;
    double s1 = 0.0, s2 = 0.0;
    for (int j = 0; j < J; j++) {
        s1 += pb[2 * j];
        s2 += pb[2 * j + 1];
    }
    if (d_beta) d_beta[b] = (float)(-s1);
    if (d_alpha) d_alpha[b] = (float)((double)beta[b] * s2);
}

extern "C" size_t l3d_sinkhorn_backward_workspace_bytes(int B, int J, int K, int n_iters)
{
    if (B <= 0 || J <= 0 || K <= 0 || n_iters < 0) return 0;
    // rowstat [B,J,4], ubar_n [B,J], part [B,J,2], ubar [n,B,J], vbar [n,B,K]
    return ((size_t)B * J * 7 + (size_t)n_iters * B * ((size_t)J + K)) * sizeof(double);
}

static inline bool mt_on16(const void *p) { return ((uintptr_t)p & 15) == 0; }

extern "C" int l3d_sinkhorn_slack_backward(const float *log_alpha, const double *potentials, int B, int J, int K, int n_iters,
                                           const float *xyz_ref, float eps, const float *d_perm, const float *d_rowsum,
                                           const float *d_weighted, const float *d_affinity, const float *dist, const float *beta,
                                           const float *alpha, float *d_out, float *d_beta, float *d_alpha, void *workspace,
                                           l3d_stream_t stream)
{
    L3D_REQUIRE(log_alpha && d_out && workspace && B > 0 && J > 0 && K > 0);
    L3D_REQUIRE(d_perm || d_rowsum || d_weighted || d_affinity);
    L3D_REQUIRE(!d_weighted || xyz_ref);
    const bool fold = dist && beta && alpha;
    L3D_REQUIRE(fold || (!dist && !beta && !alpha && !d_beta && !d_alpha));
    if (n_iters < 0 || B > 65535) return L3D_ERR_UNSUPPORTED;
    L3D_REQUIRE(potentials || n_iters == 0);
    const int n = n_iters, ps = J + K;
    const size_t per_t = (size_t)B * ps, BJ = (size_t)B * J, BK = (size_t)B * K;
    double *rowstat = (double *)workspace, *ubar_n = rowstat + BJ * 4, *part = ubar_n + BJ, *ubar = part + BJ * 2, *vbar = ubar + n * BJ;
    const bool want_part = fold && (d_beta || d_alpha), want_x = d_weighted != nullptr;
    hipStream_t s = (hipStream_t)stream;
    const dim3 rows(l3d_divup(J, 4), B), cols(l3d_divup(K, 64), B), wg(256);
    const bool k4 = K % 4 == 0 && mt_on16(log_alpha);
    const double *un = n ? potentials + (n - 1) * per_t : nullptr, *vn = n ? un + J : nullptr;

    if (k4 && (!d_perm || mt_on16(d_perm)))
        hipLaunchKernelGGL(mt_bwd_first_row_kernel<4>, rows, wg, 0, s, log_alpha, J, K, ps, un, vn, xyz_ref, (double)eps, d_perm, d_rowsum,
                           d_weighted, rowstat, ubar_n);
    else
        hipLaunchKernelGGL(mt_bwd_first_row_kernel<1>, rows, wg, 0, s, log_alpha, J, K, ps, un, vn, xyz_ref, (double)eps, d_perm, d_rowsum,
                           d_weighted, rowstat, ubar_n);
    if (n) {
        hipLaunchKernelGGL(mt_bwd_first_col_kernel, cols, wg, 0, s, log_alpha, J, K, ps, un, vn, xyz_ref, d_perm, rowstat, want_x,
                           vbar + (n - 1) * BK);
        for (int t = n; t >= 1; t--) {
            const double *ut = potentials + (t - 1) * per_t, *vt = ut + J;
            if (k4)
                hipLaunchKernelGGL(mt_bwd_row_kernel<4>, rows, wg, 0, s, log_alpha, J, K, ps, ut, vt, vbar + (t - 1) * BK,
                                   t == n ? ubar_n : nullptr, ubar + (t - 1) * BJ);
            else
                hipLaunchKernelGGL(mt_bwd_row_kernel<1>, rows, wg, 0, s, log_alpha, J, K, ps, ut, vt, vbar + (t - 1) * BK,
                                   t == n ? ubar_n : nullptr, ubar + (t - 1) * BJ);
            if (t > 1)
                hipLaunchKernelGGL(mt_bwd_col_kernel, cols, wg, 0, s, log_alpha, J, K, ps, ut, vt - per_t, ubar + (t - 1) * BJ,
                                   vbar + (t - 2) * BK);
        }
    }
    const bool out4 = k4 && mt_on16(d_out) && (!d_perm || mt_on16(d_perm)) && (!d_affinity || mt_on16(d_affinity)) && (!fold || mt_on16(dist));
    if (out4)
        hipLaunchKernelGGL(mt_bwd_out_kernel<4>, rows, wg, 0, s, log_alpha, B, J, K, n, potentials, xyz_ref, rowstat, ubar, vbar, d_perm,
                           d_affinity, want_x, fold ? dist : nullptr, beta, alpha, d_out, want_part ? part : nullptr);
    else
        hipLaunchKernelGGL(mt_bwd_out_kernel<1>, rows, wg, 0, s, log_alpha, B, J, K, n, potentials, xyz_ref, rowstat, ubar, vbar, d_perm,
                           d_affinity, want_x, fold ? dist : nullptr, beta, alpha, d_out, want_part ? part : nullptr);
    if (want_part)
        hipLaunchKernelGGL(mt_bwd_fold_kernel, dim3(l3d_divup(B, 64)), dim3(64), 0, s, part, beta, B, J, d_beta, d_alpha);
    return l3d_check_launch();
}
