// pointconv.hip -- the aggregation step of a PointConv set-abstraction layer (reference utils/pointconv_util.py:261-371) as one
// kernel: WeightNet on the local coordinates, DensityNet on the normalised inverse density, their product and the per-centre
// contraction with the [B,C,K,S] activation.  Declared in include/ext/l3d_pointconv.h.
//
// A lane per centre s, lanes along s: every read of feat and every write of out is a run of consecutive floats per wave.  A
// workgroup of four waves covers 64 centres x (4 CPW) channels.  Per chunk of KC neighbours the four waves first form
// dw[k][j][s] = d[k] w[k,j] for their 64 centres in LDS (each wave a quarter of the chunk's k: the two small networks are
// evaluated once per workgroup, not once per wave), then every wave runs its own CPW channels over the chunk:
//   acc[i][j] = fma(feat[c0 + i, k, s], dw[k][j][s], acc[i][j])        k ascending: one fma chain per output, no atomics.
// VALU, not the matrix cores: with lanes along s the contraction of one centre lives in ONE lane; an MFMA form would need
// feat[c, k] of one centre across lanes, a stride of S or K S floats, staged through LDS.  The VALU form needs 16 fmas per
// loaded float (2 flops per byte read + written x 5.3), well under what the kernel's HBM traffic allows.
// LDS: dw is indexed [k][j][lane]: every access has consecutive lanes on consecutive banks.
// S == 1 (one centre per cloud, the group_all layer) has its own kernel, lanes along k and then along c: see there.
#include "common.h"
#include "../../include/ext/l3d_pointconv.h"


__device__ __forceinline__ float pc_relu(float v) { return fmaxf(v, 0.f); }

// y[o] = max(0, b[o] + sum_i w[o][i] x[i]), i ascending; parameters at uniform addresses (scalar loads)
template <int CIN, int COUT>
__device__ __forceinline__ void pc_layer(const float *__restrict__ p, const float (&x)[CIN], float (&y)[COUT])
{
#pragma unroll
    for (int o = 0; o < COUT; o++) {
        float a = p[CIN * COUT + o];
#pragma unroll
        for (int i = 0; i < CIN; i++) a = fmaf(p[o * CIN + i], x[i], a);
        y[o] = pc_relu(a);
    }
}

// w[0:16] = DensityNet(gi[k] / gmax) WeightNet(gx[3 k : 3 k + 3]) of one centre's neighbour k (gi NULL: no density factor)
__device__ __forceinline__ void pc_neighbour_weights(const float *wn, const float *dn, const float *__restrict__ gx,
                                                     const float *__restrict__ gi, float gmax, int k, float (&w)[16])
{
    // the 425 parameters are re-read through the scalar cache at every call: hoisted out of the caller's k loop they do not fit
    // the SGPR file and were spilled into VGPR lanes
    asm volatile("" : "+s"(wn), "+s"(dn));
    float dens = 1.f;
    if (gi) {
        float x0[1] = {gi[k] / gmax}, h1[16], h2[8], h3[1];
        pc_layer<1, 16>(dn, x0, h1);
        pc_layer<16, 8>(dn + 32, h1, h2);
        pc_layer<8, 1>(dn + 32 + 136, h2, h3);
        dens = h3[0];
    }
    float x[3] = {gx[k * 3 + 0], gx[k * 3 + 1], gx[k * 3 + 2]}, h1[8], h2[8];
    pc_layer<3, 8>(wn, x, h1);
    pc_layer<8, 8>(wn + 32, h1, h2);
    pc_layer<8, 16>(wn + 32 + 72, h2, w);
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = dens * w[j];
}

#define PA_KC 64                // neighbours per chunk of the one-centre kernel
#define PA_CT 64                // channels per workgroup of the one-centre kernel (one wave)

// S == 1, the group_all layer: one centre per cloud, so with lanes along s one lane of a wave would work.  Here a wave owns 64
// channels of one cloud.  Per chunk of 64 neighbours: lanes along k read feat[c, k0 + lane] row by row (consecutive floats) into
// LDS and evaluate the two small networks for neighbour k0 + lane; then lanes along c, each running its own fma chain over the
// chunk in ascending k with feat from its LDS row (pitch 65: 64 lanes on 64 banks) and dw[k][0:16] as broadcasts.
__global__ __launch_bounds__(64) void pointconv_aggregate_one_kernel(const float *__restrict__ feat, const float *__restrict__ gxyz,
                                                                     const float *__restrict__ ginv, const float *__restrict__ wn,
                                                                     const float *__restrict__ dn, int C, int K,
                                                                     float *__restrict__ out)
{
    __shared__ float fl[PA_CT][PA_KC + 1];
    __shared__ float dwl[PA_KC][16];
    const int lane = threadIdx.x, b = blockIdx.y, c0 = blockIdx.x * PA_CT;
    const int nch = min(PA_CT, C - c0);
    const float *gx = gxyz + (size_t)b * K * 3;
    const float *gi = ginv ? ginv + (size_t)b * K : nullptr;
    float gmax = 1.f;
    if (gi) {
        float m = -INFINITY;
        for (int k = lane; k < K; k += 64) m = fmaxf(m, gi[k]);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
        gmax = m;
    }
    float acc[16];
#pragma unroll
    for (int j = 0; j < 16; j++) acc[j] = 0.f;
    const float *fb = feat + ((size_t)b * C + c0) * K;
    for (int k0 = 0; k0 < K; k0 += PA_KC) {
        const int kn = min(PA_KC, K - k0);
        const int kc = min(k0 + lane, K - 1);              // a lane past the tail reads the last neighbour and its column is not used
        __syncthreads();                                   // the previous chunk has been consumed
#pragma unroll 8
        for (int ci = 0; ci < nch; ci++) fl[ci][lane] = fb[(size_t)ci * K + kc];
        float w[16];
        pc_neighbour_weights(wn, dn, gx, gi, gmax, kc, w);
#pragma unroll
        for (int j = 0; j < 16; j++) dwl[lane][j] = w[j];
        __syncthreads();
        if (lane < nch) {
            for (int kk = 0; kk < kn; kk++) {
                const float f = fl[lane][kk];
#pragma unroll
                for (int j = 0; j < 16; j++) acc[j] = fmaf(f, dwl[kk][j], acc[j]);
            }
        }
    }
    if (lane < nch) {
        float *o = out + ((size_t)b * C + c0 + lane) * 16;
#pragma unroll
        for (int j = 0; j < 16; j++) o[j] = acc[j];
    }
}

template <int CPW>
__global__ __launch_bounds__(256, 2) void pointconv_aggregate_kernel(const float *__restrict__ feat, const float *__restrict__ gxyz,
                                                                  const float *__restrict__ ginv, const float *__restrict__ wn,
                                                                  const float *__restrict__ dn, int C, int K, int S,
                                                                  float *__restrict__ out)
{
    // neighbours per chunk: the chunk's feat values wait in KC x CPW registers beside the 16 CPW accumulators
    constexpr int KC = CPW == 8 ? 4 : 8;
    __shared__ float dw[KC][16][64];
    __shared__ float red[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = blockIdx.x * 64 + lane, b = blockIdx.z;
    const bool live = s < S;
    const int sc = live ? s : S - 1;                       // a lane past the tail reads the last centre and stores nothing
    const int c0 = (blockIdx.y * 4 + wave) * CPW;
    const size_t centre = (size_t)b * S + sc;
    const float *gx = gxyz + centre * K * 3;
    const float *gi = ginv ? ginv + centre * K : nullptr;

    float gmax = 1.f;
    if (gi) {                                              // max_k ginv: exact in any order
        float m = -INFINITY;
        for (int k = wave; k < K; k += 4) m = fmaxf(m, gi[k]);
        red[wave][lane] = m;
        __syncthreads();
        gmax = fmaxf(fmaxf(red[0][lane], red[1][lane]), fmaxf(red[2][lane], red[3][lane]));
    }

    float acc[CPW][16];
#pragma unroll
    for (int i = 0; i < CPW; i++)
#pragma unroll
        for (int j = 0; j < 16; j++) acc[i][j] = 0.f;

    const float *fbase = feat + ((size_t)b * C + c0) * K * S + sc;
    const size_t cstride = (size_t)K * S;

    for (int k0 = 0; k0 < K; k0 += KC) {
        const int kn = min(KC, K - k0);
        // the chunk's feat values are requested before the two small networks are evaluated: their latency runs under that
        // arithmetic.  (A k past the tail reads the last neighbour again and is not used.)
        float f[KC][CPW];
#pragma unroll
        for (int kk = 0; kk < KC; kk++)
#pragma unroll
            for (int i = 0; i < CPW; i++) f[kk][i] = fbase[i * cstride + (size_t)min(k0 + kk, K - 1) * S];
        __syncthreads();                                   // the previous chunk has been consumed
        for (int kk = wave; kk < kn; kk += 4) {
            float w[16];
            pc_neighbour_weights(wn, dn, gx, gi, gmax, k0 + kk, w);
#pragma unroll
            for (int j = 0; j < 16; j++) dw[kk][j][lane] = w[j];
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < KC; kk++) {
            if (kk < kn) {                                 // uniform: f is indexed by constants only, it stays in registers
                float w[16];
#pragma unroll
                for (int j = 0; j < 16; j++) w[j] = dw[kk][j][lane];
#pragma unroll
                for (int i = 0; i < CPW; i++)
#pragma unroll
                    for (int j = 0; j < 16; j++) acc[i][j] = fmaf(f[kk][i], w[j], acc[i][j]);
            }
        }
    }

    if (live) {
        float *o = out + ((size_t)b * C + c0) * 16 * S + s;
#pragma unroll
        for (int i = 0; i < CPW; i++)
#pragma unroll
            for (int j = 0; j < 16; j++) o[(size_t)(i * 16 + j) * S] = acc[i][j];
    }
}

extern "C" int l3d_pointconv_aggregate(const float *feat, const float *gxyz, const float *ginv, const float *wn, const float *dn,
                                       int B, int C, int K, int S, float *out, l3d_stream_t stream)
{
    L3D_REQUIRE(feat && gxyz && wn && out && B > 0 && C > 0 && K > 0 && S > 0);
    L3D_REQUIRE(!ginv || dn);
    if (C % 16 || C < 16 || C > L3D_POINTCONV_MAX_C || B > 65535) return L3D_ERR_UNSUPPORTED;
    if (S == 1)
        hipLaunchKernelGGL(pointconv_aggregate_one_kernel, dim3(l3d_divup(C, PA_CT), B), dim3(64), 0, (hipStream_t)stream, feat, gxyz,
                           ginv, wn, dn, C, K, out);
    else if (C % 32 == 0)
        hipLaunchKernelGGL(pointconv_aggregate_kernel<8>, dim3(l3d_divup(S, 64), C / 32, B), dim3(256), 0, (hipStream_t)stream, feat,
                           gxyz, ginv, wn, dn, C, K, S, out);
    else
        hipLaunchKernelGGL(pointconv_aggregate_kernel<4>, dim3(l3d_divup(S, 64), C / 16, B), dim3(256), 0, (hipStream_t)stream, feat,
                           gxyz, ginv, wn, dn, C, K, S, out);
    return l3d_check_launch();
}
