// svd.hip -- batched 3x3 SVD / Kabsch head for gfx950.
//
// Replaces the host loop of utils/svd.py:38-49 (B x { torch.svd, torch.det, `if r_det < 0`
// device->host sync }) and the surrounding centring / H / t algebra (:29-33, :58) with one
// launch: one workgroup per batch element reduces the means and the 3x3 cross-covariance over N,
// then a single lane runs a one-sided (Hestenes) Jacobi SVD in fp64 registers, applies the
// reflection fix and writes R and t.  No host synchronisation anywhere.
//
// Why one-sided Jacobi in fp64: the parity bar is |R - R_ref| <= 1e-5 against LAPACK gesdd in fp32
// (itself ~4e-6 from the fp64 truth for well-conditioned H); forming H^T H
// would square the condition number, and MI355X's fp64 vector rate makes 3x3 fp64 work free.
#include "common.h"
#include "svd3x3.h"

__global__ __launch_bounds__(64) void svd3x3_rotation_kernel(const float *__restrict__ H, int B,
                                                             float *__restrict__ R)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    double h[9];
    float r[9];
    for (int e = 0; e < 9; e++) h[e] = (double)H[(size_t)i * 9 + e];
    rotation_from_H(h, r);
    for (int e = 0; e < 9; e++) R[(size_t)i * 9 + e] = r[e];
}

extern "C" int l3d_svd3x3_rotation(const float *H, int B, float *R, l3d_stream_t stream)
{
    L3D_REQUIRE(H && R && B > 0);
    hipLaunchKernelGGL(svd3x3_rotation_kernel, dim3(l3d_divup(B, 64)), dim3(64), 0,
                       (hipStream_t)stream, H, B, R);
    return l3d_check_launch();
}

// block-wide sum of NV doubles per thread; result valid in thread 0
template <int NV>
__device__ static void block_sum(double (&v)[NV], double *sh /* [NV][4] */)
{
#pragma unroll
    for (int e = 0; e < NV; e++)
        for (int off = 32; off > 0; off >>= 1) v[e] += __shfl_down(v[e], off, 64);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();
    if (lane == 0)
        for (int e = 0; e < NV; e++) sh[e * 4 + wave] = v[e];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int e = 0; e < NV; e++) v[e] = sh[e * 4] + sh[e * 4 + 1] + sh[e * 4 + 2] + sh[e * 4 + 3];
}

// src, corr: [B,3,N].  One 256-thread workgroup per batch element.
__global__ __launch_bounds__(256) void kabsch_kernel(const float *__restrict__ src,
                                                     const float *__restrict__ corr, int N,
                                                     float *__restrict__ R, float *__restrict__ t,
                                                     float *__restrict__ Hout)
{
    __shared__ double sh[9 * 4];
    __shared__ float mean_s[3], mean_c[3];
    const int b = blockIdx.x;
    const float *s = src + (size_t)b * 3 * N;
    const float *c = corr + (size_t)b * 3 * N;
    double m[6] = {0, 0, 0, 0, 0, 0};
    for (int i = threadIdx.x; i < N; i += blockDim.x)
        for (int d = 0; d < 3; d++) { m[d] += s[d * N + i]; m[3 + d] += c[d * N + i]; }
    block_sum<6>(m, sh);
    if (threadIdx.x == 0)
        for (int d = 0; d < 3; d++) { mean_s[d] = (float)(m[d] / N); mean_c[d] = (float)(m[3 + d] / N); }
    __syncthreads();
    // H = src_centred (3xN) * corr_centred^T (Nx3): centring in fp32 like the reference (:29-31)
    double h[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = threadIdx.x; i < N; i += blockDim.x) {
        float sc[3], cc[3];
        for (int d = 0; d < 3; d++) { sc[d] = s[d * N + i] - mean_s[d]; cc[d] = c[d * N + i] - mean_c[d]; }
        for (int r = 0; r < 3; r++)
            for (int q = 0; q < 3; q++) h[r * 3 + q] += (double)sc[r] * (double)cc[q];
    }
    block_sum<9>(h, sh);
    if (threadIdx.x == 0) {
        float r[9];
        double hf[9];
        for (int e = 0; e < 9; e++) hf[e] = (double)(float)h[e];      // H is an fp32 tensor in the reference
        rotation_from_H(hf, r);
        for (int e = 0; e < 9; e++) R[(size_t)b * 9 + e] = r[e];
        if (Hout) for (int e = 0; e < 9; e++) Hout[(size_t)b * 9 + e] = (float)h[e];
        // t = -R mean(src) + mean(corr)      (utils/svd.py:58)
        for (int q = 0; q < 3; q++)
            t[(size_t)b * 3 + q] = (-r[q * 3] * mean_s[0] + -r[q * 3 + 1] * mean_s[1]) + -r[q * 3 + 2] * mean_s[2] + mean_c[q];
    }
}

extern "C" int l3d_kabsch(const float *src, const float *corr, int B, int N, float *R, float *t,
                          float *H_out, l3d_stream_t stream)
{
    L3D_REQUIRE(src && corr && R && t && B > 0 && N > 0);
    hipLaunchKernelGGL(kabsch_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, src, corr, N, R, t, H_out);
    return l3d_check_launch();
}
