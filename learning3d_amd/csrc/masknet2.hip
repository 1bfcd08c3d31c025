// masknet2.hip -- the three kernels of MaskNet2 (models/masknet2.py) that no other kernel of the library serves:
//
//   l3d_mish                   x tanh(softplus(x)) behind the folded Conv+BN layers, one exp and one division per element.
//   l3d_self_attention_shared  Self_Attn (:35-70): query = key = value = q [B,D,N], logits unscaled, out = q + beta ctx, flash-style on
//                              v_mfma_f32_32x32x2_f32 (exact fp32 fma chains).  The point is the single operand: a key tile of q,
//                              [D][32] exactly as it lies in memory (key-contiguous), is staged into LDS ONCE and read twice,
//                                S^T[key][query] = sum_c K[key][c] Q^T[c][query]     A = the tile, lanes along keys (row 2 s + h)
//                                O^T[c][query]  += sum_key V^T[c][key] P[key][query] A = the tile again, lanes along channels
//                              The row stride is 33 floats: ds_read_b32 banks are (address / 4) % 32 per 32-lane half, so the first
//                              pattern (33 row + m) and the second (33 (32 dt + m) + key) both touch 32 distinct banks.
//                              A lane of the S^T accumulator holds keys 8 (r / 4) + 4 h + r % 4, r = 0 .. 15, of ONE query (h = lane / 32),
//                              which is what the B operand of a 32x32x2 k-step wants of the lane pair (l, l + 32) if k-step r takes the
//                              keys 8 (r / 4) + r % 4 and 8 (r / 4) + 4 + r % 4: the probabilities go from the accumulators into the
//                              second product with no lane movement and no LDS (as attention.hip picks its key slots).
//                              A wave owns 32 queries and all keys; its Q^T fragments (D / 2 registers) stay in registers for the
//                              whole kernel, O^T is D / 2 accumulator registers.
//   l3d_outer_softmax_mix      self_attention_fc (:124-163): the softmax over the outer product of two vectors, rows and columns,
//                              with the row maximum known in closed form.
#include "common.h"
#include "split_bf16.h"          // f32x16
#include "../../include/l3d_masknet2.h"

// ------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float mish1(float x)
{
    if (x > 20.f) return x;
    const float n = expf(x);
    const float t = n * (n + 2.f);          // x <= 20: t < 2.4e17
    const float r = t / (t + 2.f);          // tanh(log(1 + n)) = ((1 + n)^2 - 1) / ((1 + n)^2 + 1)
    return r == 0.f ? -0.f : x * r;         // e^x underflowed (x < -87.3): -0, also for -inf (whose product with 0 is a NaN)
}

template <bool VEC>
__global__ __launch_bounds__(256) void mish_kernel(const float *x, long count, float *y)
{
    const long tid = (long)blockIdx.x * 256 + threadIdx.x, step = (long)gridDim.x * 256;
    if constexpr (VEC) {
        const long quads = count >> 2;
        for (long i = tid; i < quads; i += step) {
            float4 v = reinterpret_cast<const float4 *>(x)[i];
            v.x = mish1(v.x); v.y = mish1(v.y); v.z = mish1(v.z); v.w = mish1(v.w);
            reinterpret_cast<float4 *>(y)[i] = v;
        }
        for (long i = 4 * quads + tid; i < count; i += step) y[i] = mish1(x[i]);
    } else {
        for (long i = tid; i < count; i += step) y[i] = mish1(x[i]);
    }
}

extern "C" int l3d_mish(const float *x, long count, float *y, l3d_stream_t stream)
{
    L3D_REQUIRE(x && y && count > 0);
    const bool vec = ((((size_t)x) | ((size_t)y)) & 15) == 0;
    const long work = vec ? (count + 3) / 4 : count;
    const int grid = (int)(work / 256 + 1 < 16384 ? work / 256 + 1 : 16384);
    if (vec)
        hipLaunchKernelGGL((mish_kernel<true>), dim3(grid), dim3(256), 0, (hipStream_t)stream, x, count, y);
    else
        hipLaunchKernelGGL((mish_kernel<false>), dim3(grid), dim3(256), 0, (hipStream_t)stream, x, count, y);
    return l3d_check_launch();
}

// ------------------------------------------------------------------------------------------------------------------------------
#define SA_TQ L3D_SELF_ATTN_TQ
#define SA_TK L3D_SELF_ATTN_TK
#define SA_STRIDE 33             // floats per channel row of the key tile in LDS (see the head of the file)
#define SA_LOG2E 1.44269504088896340736f
static_assert(SA_TQ == 128 && SA_TK == 32, "the lane maps below are written for 4 waves x 32 queries and 32-key tiles");

// thread t stages key t % 32 of the channels t / 32 + 8 i: 128 contiguous bytes per 32 lanes; keys past the end read key N - 1
// (their weight is set to 0 where the probabilities are formed)
template <int ND>
__device__ __forceinline__ void sa_load_tile(const float *__restrict__ qb, int N, int j0, int t, float (&kr)[4 * ND])
{
    const float *p = qb + (size_t)(t >> 5) * N + min(j0 + (t & 31), N - 1);
#pragma unroll
    for (int i = 0; i < 4 * ND; i++) kr[i] = p[(size_t)(8 * i) * N];
}

template <int ND>
__device__ __forceinline__ void sa_put_tile(float *__restrict__ sK, int t, const float (&kr)[4 * ND])
{
    float *p = sK + (t >> 5) * SA_STRIDE + (t & 31);
#pragma unroll
    for (int i = 0; i < 4 * ND; i++) p[8 * i * SA_STRIDE] = kr[i];
}

template <int ND /* D / 32 */>
__global__ __launch_bounds__(256) void self_attn_kernel(const float *__restrict__ q, const float *__restrict__ beta, int N,
                                                        float *__restrict__ out)
{
    constexpr int D = 32 * ND;
    __shared__ float sK[D * SA_STRIDE];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, m = lane & 31, h = lane >> 5;
    const int b = blockIdx.y, i0 = blockIdx.x * SA_TQ + wave * 32;
    const float *qb = q + (size_t)b * D * N;
    const bool active = i0 < N;                        // per wave: a wave past the end only helps staging
    const int qi = min(i0 + m, N - 1);

    // Q^T[c][query] as the B operand of k-step s: channel 2 s + h of this lane's query
    float qf[D / 2];
#pragma unroll
    for (int s = 0; s < D / 2; s++) qf[s] = qb[(size_t)(2 * s + h) * N + qi];

    f32x16 o[ND];
#pragma unroll
    for (int dt = 0; dt < ND; dt++)
#pragma unroll
        for (int r = 0; r < 16; r++) o[dt][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;              // of this lane's query over this lane's half of the keys (l_run) / all keys (m_run)

    float kr[4 * ND];
    sa_load_tile<ND>(qb, N, 0, t, kr);
    sa_put_tile<ND>(sK, t, kr);
    __syncthreads();

    const float *a1 = sK + h * SA_STRIDE + m;          // + 2 s SA_STRIDE
    const float *a2 = sK + m * SA_STRIDE + 4 * h;      // + 32 dt SA_STRIDE + 8 (r / 4) + r % 4

    for (int j0 = 0; j0 < N; j0 += SA_TK) {
        const bool more = j0 + SA_TK < N;
        if (more) sa_load_tile<ND>(qb, N, j0 + SA_TK, t, kr);       // in flight under this tile's MFMAs
        if (active) {
            f32x16 s;
#pragma unroll
            for (int r = 0; r < 16; r++) s[r] = 0.f;
#pragma unroll
            for (int ks = 0; ks < D / 2; ks++)
                s = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[2 * ks * SA_STRIDE], qf[ks], s, 0, 0, 0);

            // s[r] = logit of key j0 + 8 (r / 4) + 4 h + r % 4 with this lane's query.  Key j0 is always inside, so the maximum over
            // the lane pair is a number.
            const int kbase = j0 + 4 * h;
            float mx = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; r++)
                if (kbase + 8 * (r >> 2) + (r & 3) < N) mx = fmaxf(mx, s[r]);
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float m_new = fmaxf(m_run, mx);
            const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * SA_LOG2E);      // first tile: exp2(-inf) = 0
            m_run = m_new;
            float p[16], psum = 0.f;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const float e = __builtin_amdgcn_exp2f((s[r] - m_new) * SA_LOG2E);
                p[r] = kbase + 8 * (r >> 2) + (r & 3) < N ? e : 0.f;
                psum += p[r];
            }
            l_run = fmaf(l_run, alpha, psum);
#pragma unroll
            for (int dt = 0; dt < ND; dt++)
#pragma unroll
                for (int r = 0; r < 16; r++) o[dt][r] *= alpha;
            // k-step r: keys 8 (r / 4) + r % 4 (h = 0) and + 4 (h = 1), the ones p[r] of the two lanes of a pair belongs to
#pragma unroll
            for (int r = 0; r < 16; r++)
#pragma unroll
                for (int dt = 0; dt < ND; dt++)
                    o[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a2[32 * dt * SA_STRIDE + 8 * (r >> 2) + (r & 3)], p[r], o[dt], 0, 0, 0);
        }
        __syncthreads();                               // every wave is done reading the tile
        if (more) sa_put_tile<ND>(sK, t, kr);
        __syncthreads();
    }

    const float l = l_run + __shfl_xor(l_run, 32, 64);
    if (active && i0 + m < N) {
        const float inv = 1.f / l, bt = beta[0];
        const size_t at = (size_t)b * D * N + (size_t)(i0 + m);
#pragma unroll
        for (int dt = 0; dt < ND; dt++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const size_t e = at + (size_t)(32 * dt + 8 * (r >> 2) + 4 * h + (r & 3)) * N;
                out[e] = fmaf(bt, o[dt][r] * inv, q[e]);
            }
    }
}

template <int ND>
static int sa_launch(dim3 grid, hipStream_t st, const float *q, const float *beta, int N, float *out)
{
    hipLaunchKernelGGL((self_attn_kernel<ND>), grid, dim3(256), 0, st, q, beta, N, out);
    return l3d_check_launch();
}

extern "C" int l3d_self_attention_shared(const float *q, const float *beta, int B, int D, int N, float *out, l3d_stream_t stream)
{
    L3D_REQUIRE(q && beta && out && B > 0 && D > 0 && N > 0);
    if (D % 32 || D > 256 || B > 65535) return L3D_ERR_UNSUPPORTED;
    const dim3 grid(l3d_divup(N, SA_TQ), B);
    hipStream_t st = (hipStream_t)stream;
    switch (D / 32) {
    case 1: return sa_launch<1>(grid, st, q, beta, N, out);
    case 2: return sa_launch<2>(grid, st, q, beta, N, out);
    case 3: return sa_launch<3>(grid, st, q, beta, N, out);
    case 4: return sa_launch<4>(grid, st, q, beta, N, out);
    case 5: return sa_launch<5>(grid, st, q, beta, N, out);
    case 6: return sa_launch<6>(grid, st, q, beta, N, out);
    case 7: return sa_launch<7>(grid, st, q, beta, N, out);
    default: return sa_launch<8>(grid, st, q, beta, N, out);
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
#define OM_MAXC 1024

// sum_j softmax_j(a v_j) w_j with the maximum a * (a >= 0 ? vmax : vmin) known beforehand; v, w in LDS (every lane reads the same word)
__device__ __forceinline__ float om_mix(float a, const float *__restrict__ v, const float *__restrict__ w, int C, float vmax, float vmin)
{
    const float mx = a * (a >= 0.f ? vmax : vmin);
    float num = 0.f, den = 0.f;
    for (int j = 0; j < C; j++) {
        const float e = expf(fmaf(a, v[j], -mx));
        num = fmaf(e, w[j], num);
        den += e;
    }
    return num / den;
}

__global__ __launch_bounds__(1024) void outer_softmax_mix_kernel(const float *__restrict__ px, const float *__restrict__ py,
                                                                 const float *__restrict__ beta, int C, float *__restrict__ outx,
                                                                 float *__restrict__ outy)
{
    __shared__ float sX[OM_MAXC], sY[OM_MAXC];
    __shared__ float sRed[4][16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    const size_t row = (size_t)blockIdx.x * C;
    const bool mine = tid < C;
    const float x = mine ? px[row + tid] : 0.f, y = mine ? py[row + tid] : 0.f;
    if (mine) { sX[tid] = x; sY[tid] = y; }
    float r[4] = {mine ? x : -INFINITY, mine ? -x : -INFINITY, mine ? y : -INFINITY, mine ? -y : -INFINITY};   // max x, -min x, max y, -min y
#pragma unroll
    for (int k = 0; k < 4; k++) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) r[k] = fmaxf(r[k], __shfl_xor(r[k], off, 64));
        if (lane == 0) sRed[k][wave] = r[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; k++) {
        float v = sRed[k][0];
        for (int w = 1; w < nw; w++) v = fmaxf(v, sRed[k][w]);
        r[k] = v;
    }
    if (mine) {
        const float bt = beta[0];
        outx[row + tid] = fmaf(bt, om_mix(x, sY, sX, C, r[2], -r[3]), x);
        outy[row + tid] = fmaf(bt, om_mix(y, sX, sY, C, r[0], -r[1]), y);
    }
}

extern "C" int l3d_outer_softmax_mix(const float *px, const float *py, const float *beta, int B, int C, float *outx, float *outy,
                                     l3d_stream_t stream)
{
    L3D_REQUIRE(px && py && beta && outx && outy && B > 0 && C > 0);
    if (C > OM_MAXC || B > 65535) return L3D_ERR_UNSUPPORTED;
    const int threads = 64 * l3d_divup(C, 64);
    hipLaunchKernelGGL(outer_softmax_mix_kernel, dim3(B), dim3(threads), 0, (hipStream_t)stream, px, py, beta, C, outx, outy);
    return l3d_check_launch();
}
