// deepgmr.hip -- the three kernels of DeepGMR (models/deepgmr.py) that no other kernel of the library serves:
//
//   l3d_rri_features   get_rri (data_utils/dataloaders.py:126-147): 4 rotation-invariant numbers per (point, neighbour).  A lane per
//                      (point, a); 256 / k points per workgroup; the point's tangent vectors T_b in LDS (fp64), a loop over b.  The
//                      reference builds [N,k,k,3] cross products on the host; here nothing larger than the output exists.
//                      Everything that cancels (q - dot p, the cross products, the projections) is formed in fp64: gfx950's fp64
//                      vector rate makes the k^2 inner loop as cheap as its fp32 atan2, and the result is the fp64 definition
//                      rounded once rather than a second fp32 rounding sequence beside the reference's.
//   l3d_gmm_params     gmm_params (models/deepgmr.py:13-31) with the softmax over J in front: one workgroup per cloud, tiles of
//                      one point per thread; the tile's gamma [J][TN] in LDS, then a wave per component reduces the tile (lane
//                      partials, butterfly) into fp64 accumulators in LDS.  Two passes: (sum gamma, sum gamma p), then
//                      sum gamma |p - mu|^2 about the computed mean.  Latency-bound: B workgroups.
//   l3d_gmm_register   gmm_register (:34-54): one wave per pair, a lane per component, the SVD head of svd.hip in lane 0.
#include "common.h"
#include "svd3x3.h"
#include "../../include/models/l3d_deepgmr.h"

// ------------------------------------------------------------------------------------------------------------------------------
#define RRI_THREADS 256
#define RRI_TWO_PI 6.283185307179586476925286766559

__global__ __launch_bounds__(RRI_THREADS) void rri_kernel(const float *__restrict__ xyz, const int64_t *__restrict__ idx, int N, int k,
                                                          int pb /* points per workgroup: RRI_THREADS / k */, int channel_first,
                                                          float *__restrict__ feat)
{
    __shared__ double sT[RRI_THREADS * 3];             // T_a of thread pl k + a
    const int t = threadIdx.x, pl = t / k, a = t - pl * k;
    const int b = blockIdx.y, n = blockIdx.x * pb + pl;
    const bool active = pl < pb && n < N;
    const float *xb = xyz + (size_t)b * N * 3;

    double pnx = 0, pny = 0, pnz = 0, tx = 0, ty = 0, tz = 0, rp = 0, rq = 0, theta = 0;
    if (active) {
        const double px = xb[(size_t)n * 3], py = xb[(size_t)n * 3 + 1], pz = xb[(size_t)n * 3 + 2];
        long long qi = idx[((size_t)b * N + n) * k + a];
        qi = qi < 0 ? 0 : (qi >= N ? N - 1 : qi);
        const double qx = xb[(size_t)qi * 3], qy = xb[(size_t)qi * 3 + 1], qz = xb[(size_t)qi * 3 + 2];
        rp = sqrt(px * px + py * py + pz * pz);
        rq = sqrt(qx * qx + qy * qy + qz * qz);
        pnx = px / rp; pny = py / rp; pnz = pz / rp;
        const double dot = (pnx * (qx / rq) + pny * (qy / rq)) + pnz * (qz / rq);
        theta = acos(dot < -1.0 ? -1.0 : (dot > 1.0 ? 1.0 : dot));        // a NaN stays one, as under np.clip
        tx = qx - dot * px; ty = qy - dot * py; tz = qz - dot * pz;       // p not normalised (:139)
        sT[t * 3] = tx; sT[t * 3 + 1] = ty; sT[t * 3 + 2] = tz;
    }
    __syncthreads();
    if (!active) return;

    // phi_a = min over b != a of atan2((T_b x T_a) . pn, T_b . T_a) mod 2 pi
    const double *tb = sT + (size_t)pl * k * 3;
    float best = INFINITY;
    bool nan = false;
    for (int j = 0; j < k; j++) {
        const double bx = tb[j * 3], by = tb[j * 3 + 1], bz = tb[j * 3 + 2];
        const double cx = by * tz - bz * ty, cy = bz * tx - bx * tz, cz = bx * ty - by * tx;
        const float s = (float)((cx * pnx + cy * pny) + cz * pnz), c = (float)((bx * tx + by * ty) + bz * tz);
        float psi = atan2f(s, c);
        if (psi < 0.f) psi = (float)((double)psi + RRI_TWO_PI);
        if (j != a) {
            nan = nan || psi != psi;
            best = fminf(best, psi);
        }
    }
    const float phi = nan ? __int_as_float(0x7fc00000) : best;
    const float o[4] = {(float)rp, (float)rq, (float)theta, phi};
    if (channel_first) {
        float *f = feat + ((size_t)b * 4 * k + 4 * a) * N + n;
#pragma unroll
        for (int c = 0; c < 4; c++) f[(size_t)c * N] = o[c];
    } else {
        float *f = feat + (((size_t)b * N + n) * k + a) * 4;
#pragma unroll
        for (int c = 0; c < 4; c++) f[c] = o[c];
    }
}

extern "C" int l3d_rri_features(const float *xyz, const int64_t *idx, int B, int N, int k, int channel_first, float *feat,
                                l3d_stream_t stream)
{
    L3D_REQUIRE(xyz && idx && feat && B > 0 && N > 0 && k > 0);
    if (k < 2 || k > L3D_RRI_MAX_K || B > 65535) return L3D_ERR_UNSUPPORTED;
    const int pb = RRI_THREADS / k;
    hipLaunchKernelGGL(rri_kernel, dim3(l3d_divup(N, pb), B), dim3(RRI_THREADS), 0, (hipStream_t)stream, xyz, idx, N, k, pb,
                       channel_first != 0, feat);
    return l3d_check_launch();
}

// ------------------------------------------------------------------------------------------------------------------------------
#define GMM_TILE_FLOATS 8192         // J TN <= 8192: TN = 256 for J <= 32, 128 for J <= 64

template <int TN>
__global__ __launch_bounds__(TN) void gmm_params_kernel(const float *__restrict__ logits, const float *__restrict__ pts, int J, int N,
                                                        float *__restrict__ gamma_out, float *__restrict__ pi, float *__restrict__ mu,
                                                        float *__restrict__ var)
{
    constexpr int NW = TN / 64;
    __shared__ float sG[GMM_TILE_FLOATS];              // gamma of the tile, [J][TN]
    __shared__ float sP[TN * 3];                       // the tile's points
    __shared__ double sAcc[L3D_GMM_MAX_J * 4];         // per component: sum gamma, sum gamma (x, y, z)
    __shared__ double sVar[L3D_GMM_MAX_J];             // per component: sum gamma |p - mu|^2
    __shared__ double sMu[L3D_GMM_MAX_J * 3];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, b = blockIdx.x;
    const float *lb = logits + (size_t)b * J * N;
    const float *pb = pts + (size_t)b * N * 3;
    for (int i = t; i < L3D_GMM_MAX_J * 4; i += TN) sAcc[i] = 0.0;
    for (int i = t; i < L3D_GMM_MAX_J; i += TN) sVar[i] = 0.0;
    __syncthreads();

    for (int pass = 0; pass < 2; pass++) {
        for (int n0 = 0; n0 < N; n0 += TN) {
            const int n = n0 + t;
            const bool in = n < N;
            // this thread's point: softmax over J (maximum, exp, sum, division: torch's sequence), written down the tile's column
            float m = -INFINITY, s = 0.f;
            if (in) {
                for (int j = 0; j < J; j++) m = fmaxf(m, lb[(size_t)j * N + n]);
                for (int j = 0; j < J; j++) {
                    const float e = expf(lb[(size_t)j * N + n] - m);
                    sG[j * TN + t] = e;
                    s += e;
                }
            }
            for (int j = 0; j < J; j++) sG[j * TN + t] = in ? sG[j * TN + t] / s : 0.f;
#pragma unroll
            for (int c = 0; c < 3; c++) sP[t * 3 + c] = in ? pb[(size_t)n * 3 + c] : 0.f;
            __syncthreads();
            if (pass == 0 && gamma_out) {
                const int cnt = min(TN, N - n0) * J;               // [points of the tile][J] is one contiguous run of gamma_out
                float *g = gamma_out + ((size_t)b * N + n0) * J;
                for (int e = t; e < cnt; e += TN) {
                    const int p = e / J;
                    g[e] = sG[(e - p * J) * TN + p];
                }
            }
            // a wave per component: lane partials over the tile's points in ascending order, then the butterfly
            for (int j = wave; j < J; j += NW) {
                if (pass == 0) {
                    double a0 = 0, a1 = 0, a2 = 0, a3 = 0;
                    for (int i = lane; i < TN; i += 64) {
                        const double g = sG[j * TN + i];
                        a0 += g; a1 += g * sP[i * 3]; a2 += g * sP[i * 3 + 1]; a3 += g * sP[i * 3 + 2];
                    }
                    a0 = l3d_wave_sum(a0); a1 = l3d_wave_sum(a1); a2 = l3d_wave_sum(a2); a3 = l3d_wave_sum(a3);
                    if (lane == 0) { sAcc[j * 4] += a0; sAcc[j * 4 + 1] += a1; sAcc[j * 4 + 2] += a2; sAcc[j * 4 + 3] += a3; }
                } else {
                    const double mx = sMu[j * 3], my = sMu[j * 3 + 1], mz = sMu[j * 3 + 2];
                    double a0 = 0;
                    for (int i = lane; i < TN; i += 64) {
                        const double dx = sP[i * 3] - mx, dy = sP[i * 3 + 1] - my, dz = sP[i * 3 + 2] - mz;
                        a0 += (double)sG[j * TN + i] * ((dx * dx + dy * dy) + dz * dz);
                    }
                    a0 = l3d_wave_sum(a0);
                    if (lane == 0) sVar[j] += a0;
                }
            }
            __syncthreads();
        }
        if (t < J) {
            const double s0 = sAcc[t * 4];
            if (pass == 0) {
                pi[(size_t)b * J + t] = (float)(s0 / N);
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const double v = sAcc[t * 4 + 1 + c] / s0;
                    sMu[t * 3 + c] = v;
                    mu[((size_t)b * J + t) * 3 + c] = (float)v;
                }
            } else {
                var[(size_t)b * J + t] = (float)(sVar[t] / s0);
            }
        }
        __syncthreads();
    }
}

extern "C" int l3d_gmm_params(const float *logits, const float *pts, int B, int J, int N, float *gamma_out, float *pi, float *mu,
                              float *var, l3d_stream_t stream)
{
    L3D_REQUIRE(logits && pts && pi && mu && var && B > 0 && J > 0 && N > 0);
    if (J > L3D_GMM_MAX_J || B > 65535) return L3D_ERR_UNSUPPORTED;
    if (J <= GMM_TILE_FLOATS / 256)
        hipLaunchKernelGGL((gmm_params_kernel<256>), dim3(B), dim3(256), 0, (hipStream_t)stream, logits, pts, J, N, gamma_out, pi, mu, var);
    else
        hipLaunchKernelGGL((gmm_params_kernel<128>), dim3(B), dim3(128), 0, (hipStream_t)stream, logits, pts, J, N, gamma_out, pi, mu, var);
    return l3d_check_launch();
}

// ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void gmm_register_kernel(const float *__restrict__ pi_s, const float *__restrict__ mu_s,
                                                          const float *__restrict__ mu_t, const float *__restrict__ var_t, int J,
                                                          float *__restrict__ T)
{
    const int lane = threadIdx.x, b = blockIdx.x;
    const bool in = lane < J;
    const size_t at = (size_t)b * J + lane;
    const double w = in ? (double)pi_s[at] : 0.0, iv = in ? 1.0 / (double)var_t[at] : 0.0;
    double ms[3], mt[3], c[6];
#pragma unroll
    for (int d = 0; d < 3; d++) {
        ms[d] = in ? (double)mu_s[at * 3 + d] : 0.0;
        mt[d] = in ? (double)mu_t[at * 3 + d] : 0.0;
    }
#pragma unroll
    for (int d = 0; d < 3; d++) {
        c[d] = l3d_wave_sum(in ? w * ms[d] : 0.0);
        c[3 + d] = l3d_wave_sum(in ? w * mt[d] : 0.0);
    }
    double h[9];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int q = 0; q < 3; q++) h[r * 3 + q] = l3d_wave_sum(in ? w * (ms[r] - c[r]) * (mt[q] - c[3 + q]) * iv : 0.0);
    if (lane == 0) {
        float r[9];
        rotation_from_H(h, r);
        float *o = T + (size_t)b * 16;
#pragma unroll
        for (int q = 0; q < 3; q++) {
#pragma unroll
            for (int d = 0; d < 3; d++) o[q * 4 + d] = r[q * 3 + d];
            o[q * 4 + 3] = (float)(c[3 + q] - (((double)r[q * 3] * c[0] + (double)r[q * 3 + 1] * c[1]) + (double)r[q * 3 + 2] * c[2]));
        }
        o[12] = 0.f; o[13] = 0.f; o[14] = 0.f; o[15] = 1.f;
    }
}

extern "C" int l3d_gmm_register(const float *pi_s, const float *mu_s, const float *mu_t, const float *var_t, int B, int J, float *T,
                                l3d_stream_t stream)
{
    L3D_REQUIRE(pi_s && mu_s && mu_t && var_t && T && B > 0 && J > 0);
    if (J > L3D_GMM_MAX_J || B > 65535) return L3D_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(gmm_register_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, pi_s, mu_s, mu_t, var_t, J, T);
    return l3d_check_launch();
}
