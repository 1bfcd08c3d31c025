// masknet.hip -- the two ends of MaskNet (models/masknet.py) that no other kernel of the library serves:
//
//   l3d_mask_tail    the last two layers of the per-point head h3, Conv(C -> H)+ReLU and Conv(H -> 1)+Sigmoid, in one pass over
//                    x [B,C,N]: the C -> H product on v_mfma_f32_16x16x4_f32 (an exact fp32 fma chain per output, ascending input
//                    channel, like sa_fused.hip), the H -> 1 dot product straight from the accumulators.  The [B,H,N] map is never
//                    written.  Hidden units are the MFMA's rows and points its columns, so a lane ends up with 4 hidden units of
//                    one point per accumulator: the dot product is a per-lane sum over its rows and two cross-lane adds.
//   l3d_mask_select  torch.topk(mask, k, sorted=False) / mask > threshold followed by index_points, with a defined result: one
//                    workgroup per cloud, the cloud's order-preserving integer keys in LDS, a 4 x 8-bit radix search for the k-th
//                    largest key, then a prefix-sum compaction in ascending point index (ties: lowest index first).
#include "common.h"
#include "split_bf16.h"          // f32x4
#include "../../include/l3d_masknet.h"

#define MT_KC 16                 // input channels per k-chunk of w4 staged through LDS (C % 16 == 0: every chunk is full)
#define MT_PTS 256               // points per workgroup: 4 waves x 64
#define MT_MAXC 256
#define MT_MAXH 128

// A wave owns 64 consecutive points, lane (m = lane % 16, g = lane / 16) the four points n0 + 4 m + t, t = 0 .. 3: column m of
// the four column tiles t.  So the B operand of k-step s (channel 16 kc + 4 s + g) of all four tiles is ONE 16-byte load per lane,
// 256 contiguous bytes per channel row and wave, and the lanes g == 0 store their four results as 16 bytes.
template <bool VEC>
__device__ __forceinline__ void mt_load_x(const float *__restrict__ xb, int N, int kc, int g, int n0, float (&xv)[4][4])
{
#pragma unroll
    for (int s = 0; s < 4; s++) {
        const float *p = xb + (size_t)(kc * MT_KC + 4 * s + g) * N + n0;
        if constexpr (VEC) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (n0 < N) v = *reinterpret_cast<const float4 *>(p);        // N % 4 == 0: a group of four is inside or outside
            xv[s][0] = v.x; xv[s][1] = v.y; xv[s][2] = v.z; xv[s][3] = v.w;
        } else {
#pragma unroll
            for (int t = 0; t < 4; t++) xv[s][t] = n0 + t < N ? p[t] : 0.f;
        }
    }
}

// chunk kc of w4 [H][C] -> registers (NHT floats per thread, 64-byte runs per hidden unit) -> LDS as [g][h][s] = w4[h][16 kc + 4 s + g]:
// the A operand of row tile ht for lane (m, g) is then the float4 at (g H + 16 ht + m), 16 consecutive cells per 16-lane phase
template <int NHT>
__device__ __forceinline__ void mt_load_w(const float *__restrict__ w4, int C, int kc, int tid, float (&wr)[NHT])
{
#pragma unroll
    for (int i = 0; i < NHT; i++) {
        const int e = tid + 256 * i;
        wr[i] = w4[(size_t)(e >> 4) * C + kc * MT_KC + (e & 15)];
    }
}

template <int NHT>
__device__ __forceinline__ void mt_put_w(float *__restrict__ buf, int tid, const float (&wr)[NHT])
{
    constexpr int H = 16 * NHT;
#pragma unroll
    for (int i = 0; i < NHT; i++) {
        const int e = tid + 256 * i, h = e >> 4, cl = e & 15;
        buf[((cl & 3) * H + h) * 4 + (cl >> 2)] = wr[i];
    }
}

template <int NHT, bool VEC>
__global__ __launch_bounds__(256) void mask_tail_kernel(const float *__restrict__ x, const float *__restrict__ w4,
                                                        const float *__restrict__ b4, const float *__restrict__ w5,
                                                        const float *__restrict__ b5, int C, int N, int tiles, float *__restrict__ mask)
{
    constexpr int H = 16 * NHT;
    __shared__ __attribute__((aligned(16))) float sW[2][H * MT_KC];
    __shared__ __attribute__((aligned(16))) float sB4[H];
    __shared__ __attribute__((aligned(16))) float sW5[H];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, m = lane & 15;
    const int b = blockIdx.x / tiles, n0 = (blockIdx.x - b * tiles) * MT_PTS + wave * 64 + 4 * m;
    const float *xb = x + (size_t)b * C * N;
    const int nk = C / MT_KC;

    f32x4 acc[NHT][4];
#pragma unroll
    for (int ht = 0; ht < NHT; ht++)
#pragma unroll
        for (int t = 0; t < 4; t++) acc[ht][t] = f32x4{0.f, 0.f, 0.f, 0.f};

    float wr[NHT], xc[4][4], xn[4][4];
    mt_load_w<NHT>(w4, C, 0, tid, wr);
    mt_load_x<VEC>(xb, N, 0, g, n0, xc);
    mt_put_w<NHT>(sW[0], tid, wr);
    if (tid < H) { sB4[tid] = b4[tid]; sW5[tid] = w5[tid]; }
    __syncthreads();

    for (int kc = 0; kc < nk; kc++) {
        const bool more = kc + 1 < nk;
        if (more) {                                        // the next chunk's loads are in flight under this chunk's MFMAs
            mt_load_w<NHT>(w4, C, kc + 1, tid, wr);
            mt_load_x<VEC>(xb, N, kc + 1, g, n0, xn);
        }
        const float *wb = sW[kc & 1];
#pragma unroll
        for (int ht = 0; ht < NHT; ht++) {
            const float4 a = *reinterpret_cast<const float4 *>(wb + (g * H + 16 * ht + m) * 4);
            const float av[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
            for (int s = 0; s < 4; s++)
#pragma unroll
                for (int t = 0; t < 4; t++)
                    acc[ht][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], xc[s][t], acc[ht][t], 0, 0, 0);
        }
        if (more) {
            // the other buffer: every wave left chunk kc - 1's reads of it behind at the barrier that ended that chunk
            mt_put_w<NHT>(sW[(kc + 1) & 1], tid, wr);
#pragma unroll
            for (int s = 0; s < 4; s++)
#pragma unroll
                for (int t = 0; t < 4; t++) xc[s][t] = xn[s][t];
        }
        __syncthreads();
    }

    // acc[ht][t][r] = hidden unit 16 ht + 4 g + r of point n0 + t.  The H -> 1 layer: per lane ascending h over its rows, then the
    // four lane groups by a butterfly (every lane of a column ends with the same bits).
    float part[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ht = 0; ht < NHT; ht++) {
        const float4 bb = *reinterpret_cast<const float4 *>(sB4 + 16 * ht + 4 * g);
        const float4 ww = *reinterpret_cast<const float4 *>(sW5 + 16 * ht + 4 * g);
        const float bv[4] = {bb.x, bb.y, bb.z, bb.w}, wv[4] = {ww.x, ww.y, ww.z, ww.w};
#pragma unroll
        for (int r = 0; r < 4; r++)
#pragma unroll
            for (int t = 0; t < 4; t++) part[t] += wv[r] * fmaxf(acc[ht][t][r] + bv[r], 0.f);
    }
    const float bias = b5[0];
    float res[4];
#pragma unroll
    for (int t = 0; t < 4; t++) {
        float v = part[t];
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        res[t] = 1.f / (1.f + expf(-(v + bias)));
    }
    if (g == 0) {
        float *o = mask + (size_t)b * N + n0;
        if constexpr (VEC) {
            if (n0 < N) *reinterpret_cast<float4 *>(o) = make_float4(res[0], res[1], res[2], res[3]);
        } else {
#pragma unroll
            for (int t = 0; t < 4; t++)
                if (n0 + t < N) o[t] = res[t];
        }
    }
}

template <int NHT>
static int mt_launch(bool vec, int grid, hipStream_t st, const float *x, const float *w4, const float *b4, const float *w5,
                     const float *b5, int C, int N, int tiles, float *mask)
{
    if (vec)
        hipLaunchKernelGGL((mask_tail_kernel<NHT, true>), dim3(grid), dim3(256), 0, st, x, w4, b4, w5, b5, C, N, tiles, mask);
    else
        hipLaunchKernelGGL((mask_tail_kernel<NHT, false>), dim3(grid), dim3(256), 0, st, x, w4, b4, w5, b5, C, N, tiles, mask);
    return l3d_check_launch();
}

extern "C" int l3d_mask_tail(const float *x, const float *w4, const float *b4, const float *w5, const float *b5, int B, int C, int H,
                             int N, float *mask, l3d_stream_t stream)
{
    L3D_REQUIRE(x && w4 && b4 && w5 && b5 && mask && B > 0 && C > 0 && H > 0 && N > 0);
    if (C % 16 || C > MT_MAXC || H % 32 || H > MT_MAXH) return L3D_ERR_UNSUPPORTED;
    const long tiles = l3d_divup(N, MT_PTS);
    if ((long)B * tiles > 0x7fffffffL) return L3D_ERR_UNSUPPORTED;
    const bool vec = N % 4 == 0 && ((((size_t)x) | ((size_t)mask)) & 15) == 0;
    const int grid = (int)(B * tiles);
    hipStream_t st = (hipStream_t)stream;
    switch (H / 32) {
    case 1: return mt_launch<2>(vec, grid, st, x, w4, b4, w5, b5, C, N, (int)tiles, mask);
    case 2: return mt_launch<4>(vec, grid, st, x, w4, b4, w5, b5, C, N, (int)tiles, mask);
    case 3: return mt_launch<6>(vec, grid, st, x, w4, b4, w5, b5, C, N, (int)tiles, mask);
    default: return mt_launch<8>(vec, grid, st, x, w4, b4, w5, b5, C, N, (int)tiles, mask);
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
#define MS_THREADS 1024
#define MS_MAXN 16384
#define MS_AUX 512               // words of dynamic LDS after the keys: histogram [256], the search's verdict [2], wave totals [16]

// order-preserving key: a > b as floats <=> key(a) > key(b); -0 and +0 share a key, every NaN has the largest one
__device__ __forceinline__ uint32_t ms_key(float v)
{
    if (v != v) return 0xFFFFFFFFu;
    const uint32_t u = v == 0.f ? 0u : __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(MS_THREADS) void mask_select_kernel(const float *__restrict__ mask, const float *__restrict__ points, int N,
                                                                 int k, float threshold, int64_t *__restrict__ idx,
                                                                 float *__restrict__ out, int32_t *__restrict__ count)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t ms_lds[];
    uint32_t *sKey = ms_lds, *sHist = ms_lds + N, *sSel = sHist + 256, *sWave = sSel + 2;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    const float *mrow = mask + (size_t)b * N;

    // threshold mode keeps the comparison's verdict as the key: 1 > T = 0 selects, and no `equal` element is taken (need = 0)
    for (int i = tid; i < N; i += MS_THREADS) {
        const float v = mrow[i];
        sKey[i] = k > 0 ? ms_key(v) : (v > threshold ? 1u : 0u);
    }
    uint32_t T = 0, need = 0;
    if (k > 0) {
        // the k-th largest key, eight bits at a time from the top: among the keys that share the digits found so far, the digit
        // whose bin holds the rem-th largest
        uint32_t prefix = 0, rem = (uint32_t)k;
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (tid < 256) sHist[tid] = 0;
            __syncthreads();                                   // (first trip: the keys are written, too)
            const uint32_t himask = shift == 24 ? 0u : (0xFFFFFFFFu << (shift + 8));
            for (int i = tid; i < N; i += MS_THREADS) {
                const uint32_t key = sKey[i];
                if ((key & himask) == prefix) atomicAdd(&sHist[(key >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (tid < 64) {                                    // lane l: bins 255 - 4 l .. 252 - 4 l, the largest digit first
                uint32_t c[4], s = 0;
#pragma unroll
                for (int j = 0; j < 4; j++) { c[j] = sHist[255 - (4 * tid + j)]; s += c[j]; }
                uint32_t incl = s;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const uint32_t o = __shfl_up(incl, off, 64);
                    if (lane >= off) incl += o;
                }
                uint32_t cum = incl - s;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    if (cum < rem && rem <= cum + c[j]) { sSel[0] = 255u - (uint32_t)(4 * tid + j); sSel[1] = rem - cum; }
                    cum += c[j];
                }
            }
            __syncthreads();
            prefix |= sSel[0] << shift;
            rem = sSel[1];
        }
        T = prefix;                                            // keys above T are in; of the keys equal to T, the first `need` by index
        need = rem;
    } else {
        __syncthreads();
    }

    // compaction in ascending index: thread t owns the points [t per, (t + 1) per)
    const int per = (N + MS_THREADS - 1) / MS_THREADS;
    const int i0 = min(tid * per, N), i1 = min(i0 + per, N);
    uint32_t cg = 0, ce = 0;
    for (int i = i0; i < i1; i++) {
        const uint32_t key = sKey[i];
        cg += key > T;
        ce += key == T;
    }
    const uint32_t mine = (ce << 16) | cg;                     // both totals <= 16384: no carry between the halves
    uint32_t incl = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(incl, off, 64);
        if (lane >= off) incl += o;
    }
    if (lane == 63) sWave[wave] = incl;
    __syncthreads();
    uint32_t before = incl - mine, total = 0;
    for (int w = 0; w < MS_THREADS / 64; w++) {
        const uint32_t s = sWave[w];
        if (w < wave) before += s;
        total += s;
    }
    uint32_t gb = before & 0xFFFFu, eb = before >> 16;
    const size_t stride = k > 0 ? (size_t)k : (size_t)N;
    int64_t *ib = idx + (size_t)b * stride;
    float *ob = out + (size_t)b * stride * 3;
    const float *pb = points + (size_t)b * N * 3;
    for (int i = i0; i < i1; i++) {
        const uint32_t key = sKey[i];
        const bool gt = key > T, eq = key == T;
        if (gt || (eq && eb < need)) {
            const uint32_t p = gb + min(eb, need);
            ib[p] = i;
            ob[3 * (size_t)p] = pb[3 * (size_t)i];
            ob[3 * (size_t)p + 1] = pb[3 * (size_t)i + 1];
            ob[3 * (size_t)p + 2] = pb[3 * (size_t)i + 2];
        }
        gb += gt;
        eb += eq;
    }
    if (tid == 0) count[b] = (int32_t)((total & 0xFFFFu) + min(total >> 16, need));
}

extern "C" int l3d_mask_select(const float *mask, const float *points, int B, int N, int k, float threshold, int64_t *idx, float *out,
                               int32_t *count, l3d_stream_t stream)
{
    L3D_REQUIRE(mask && points && idx && out && count && B > 0 && N > 0);
    L3D_REQUIRE(k >= 0 && k <= N && (k > 0 || B == 1));
    if (N > MS_MAXN) return L3D_ERR_UNSUPPORTED;
    const size_t lds = ((size_t)N + MS_AUX) * sizeof(uint32_t);
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void *)mask_select_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) { g_l3d_last_hip_error = (int)e; return L3D_ERR_LAUNCH; }
    }
    hipLaunchKernelGGL(mask_select_kernel, dim3(B), dim3(MS_THREADS), lds, (hipStream_t)stream, mask, points, N, k, threshold, idx, out,
                       count);
    return l3d_check_launch();
}
