// curvenet.hip -- CurveNet's curve grouping (utils/curvenet_util.py:78-195, :493-518) on the device:
//
//   l3d_curve_prepare  x [B,C,N] -> att = sigmoid(w_att . x) [B,N] and x att as [B,N,C] channel-last: the 1-channel conv, the
//                      sigmoid, the scale and the transpose of CurveGrouping.forward in one pass over x (a 64-point tile through LDS,
//                      read and written with unit stride).
//   l3d_curve_walk     Walk.forward for eval-mode BatchNorm, every step of every curve in ONE launch.  The reference runs ~30 tiny
//                      torch ops per step (gathers, two 1-channel convs, softmax, scatter, argmax, batched_index_select); the walk is
//                      a loop over its own picks, so those launches cannot overlap.  Here one workgroup owns a cloud and one wavefront a curve: lane j < k
//                      reads candidate j's contiguous C-float row and forms its logit and crossover factor, the pick is a cross-lane
//                      arg-max (lowest lane among equal logits, like torch's max), and the curve's descriptor (`pre`) and current
//                      feature (`cur`) live in LDS, lane c updating channels c and c + 64.  The straight-through one-hot's forward value (y_hard - y) + y is taken as exactly 1.
#include "common.h"
#include "../../include/l3d_curvenet.h"

#define CW_MAXC 128          // widest feature row (two channels per lane)
#define CW_WAVES 16          // wavefronts per workgroup (one workgroup per cloud)
#define CW_MAX_LDS 65536      // dynamic LDS of the walk: curve_num (2 C + 3) words
#define CP_TILE 64           // points per workgroup of the prepare kernel

// One workgroup walks all curves of one cloud, a wavefront per curve (curve q on wave q % CW_WAVES).  The curves of a cloud are NOT
// independent: the reference views the momentum softmax [bs,2,n] as [bs,1,n,2] (:147) without transposing it, so curve q blends with
// the values at flat positions 2 q and 2 q + 1 of its cloud's [2][n] array -- two OTHER curves' outputs.  Hence a barrier per step:
// phase A writes every curve's softmax pair to sSm, phase B reads the pair the view hands each curve.  Per-curve state (pre, cur,
// current point) lives in dynamic LDS.
__global__ __launch_bounds__(CW_WAVES * 64) void curve_walk_kernel(const float *__restrict__ x, const int64_t *__restrict__ adj,
                                                                   const int64_t *__restrict__ start, int N, int C, int k,
                                                                   int curve_num, int curve_length, const float *__restrict__ w_a,
                                                                   const float *__restrict__ a_scale, const float *__restrict__ a_shift,
                                                                   const float *__restrict__ w_m, const float *__restrict__ m_scale,
                                                                   const float *__restrict__ m_shift, float *__restrict__ curves,
                                                                   int32_t *__restrict__ path)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int n = curve_num;
    float *sPre = smem, *sCur = sPre + (size_t)n * C, *sSm = sCur + (size_t)n * C;
    int *sPt = reinterpret_cast<int *>(sSm + 2 * n);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, b = blockIdx.x;
    const float *xb = x + (size_t)b * N * C;
    const int64_t *adjb = adj + (size_t)b * N * k;
    const int c0 = lane, c1 = lane + 64;
    const bool has0 = c0 < C, has1 = c1 < C;
    const float sa = a_scale[0], ha = a_shift[0];
    const float sm0 = m_scale[0], sm1 = m_scale[1], hm0 = m_shift[0], hm1 = m_shift[1];

    for (int q = w; q < n; q += CW_WAVES) {
        const int pt = (int)min(max(start[(size_t)b * n + q], (int64_t)0), (int64_t)(N - 1));
        if (lane == 0) sPt[q] = pt;
        if (has0) { sPre[q * C + c0] = xb[(size_t)pt * C + c0]; sCur[q * C + c0] = 0.f; }
        if (has1) { sPre[q * C + c1] = xb[(size_t)pt * C + c1]; sCur[q * C + c1] = 0.f; }
    }
    __syncthreads();

    for (int step = 0; step < curve_length; step++) {
        if (step > 0) {
            // phase A, dynamic momentum (:146-147): two logits from [cur; pre], softmax over the two
            for (int q = w; q < n; q += CW_WAVES) {
                float p0 = 0.f, p1 = 0.f;
                if (has0) {
                    const float cu = sCur[q * C + c0], pr = sPre[q * C + c0];
                    p0 = w_m[c0] * cu + w_m[C + c0] * pr;
                    p1 = w_m[2 * C + c0] * cu + w_m[3 * C + c0] * pr;
                }
                if (has1) {
                    const float cu = sCur[q * C + c1], pr = sPre[q * C + c1];
                    p0 += w_m[c1] * cu + w_m[C + c1] * pr;
                    p1 += w_m[2 * C + c1] * cu + w_m[3 * C + c1] * pr;
                }
                const float m0 = sm0 * l3d_wave_sum(p0) + hm0, m1 = sm1 * l3d_wave_sum(p1) + hm1;
                const float mx = fmaxf(m0, m1), e0 = expf(m0 - mx), e1 = expf(m1 - mx), den = e0 + e1;
                if (lane == 0) { sSm[q] = e0 / den; sSm[n + q] = e1 / den; }
            }
            __syncthreads();
        }
        // phase B: descriptor update, candidates, pick
        for (int q = w; q < n; q += CW_WAVES) {
            float cur0 = has0 ? sCur[q * C + c0] : 0.f, cur1 = has1 ? sCur[q * C + c1] : 0.f;
            float pre0 = has0 ? sPre[q * C + c0] : 0.f, pre1 = has1 ? sPre[q * C + c1] : 0.f;
            float n1sq = 0.f;
            if (step > 0) {
                const float att0 = sSm[2 * q], att1 = sSm[2 * q + 1];          // the [2][n] array read as [n][2] (:147)
                pre0 = cur0 * att0 + pre0 * att1;                             // pre <- cur att0 + pre att1 (:151)
                pre1 = cur1 * att0 + pre1 * att1;
                if (has0) sPre[q * C + c0] = pre0;
                if (has1) sPre[q * C + c1] = pre1;
                const float d0 = cur0 - pre0, d1 = cur1 - pre1;
                n1sq = l3d_wave_sum(d0 * d0 + d1 * d1);
            }
            // the descriptor's half of the agent's logit is the same for every candidate
            const float pp = l3d_wave_sum((has0 ? w_a[C + c0] * pre0 : 0.f) + (has1 ? w_a[C + c1] * pre1 : 0.f));
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");            // this wave's LDS writes above, read by all its lanes below
            const int at = sPt[q];

            // one candidate per lane (lanes >= k repeat the last one and are left out of the pick)
            const int64_t cand64 = adjb[(size_t)at * k + min(lane, k - 1)];
            const int cand = (int)min(max(cand64, (int64_t)0), (int64_t)(N - 1));
            const float4 *row = reinterpret_cast<const float4 *>(xb + (size_t)cand * C);
            float acc = 0.f, dot = 0.f, nb = 0.f;
            if (step == 0) {
                for (int c4 = 0; c4 < C / 4; c4++) {
                    const float4 v = row[c4];
                    acc += w_a[4 * c4] * v.x;
                    acc += w_a[4 * c4 + 1] * v.y;
                    acc += w_a[4 * c4 + 2] * v.z;
                    acc += w_a[4 * c4 + 3] * v.w;
                }
            } else {
                const float4 *cu = reinterpret_cast<const float4 *>(sCur + q * C), *pr = reinterpret_cast<const float4 *>(sPre + q * C);
                for (int c4 = 0; c4 < C / 4; c4++) {
                    const float4 v = row[c4], cc = cu[c4], pv = pr[c4];
                    acc += w_a[4 * c4] * v.x;
                    acc += w_a[4 * c4 + 1] * v.y;
                    acc += w_a[4 * c4 + 2] * v.z;
                    acc += w_a[4 * c4 + 3] * v.w;
                    const float bx = v.x - cc.x, by = v.y - cc.y, bz = v.z - cc.z, bw = v.w - cc.w;
                    dot += (cc.x - pv.x) * bx; dot += (cc.y - pv.y) * by; dot += (cc.z - pv.z) * bz; dot += (cc.w - pv.w) * bw;
                    nb += bx * bx; nb += by * by; nb += bz * bz; nb += bw * bw;
                }
            }
            float logit = sa * (acc + pp) + ha;
            if (step > 0) {
                // crossover suppression (:99-114): 1 + cos(cur - pre, x[cand] - cur), clamped to [0, 1]
                const float divider = fmaxf(sqrtf(n1sq) * sqrtf(nb), 1e-8f);
                logit *= fminf(fmaxf(1.f + dot / divider, 0.f), 1.f);
            }
            if (lane >= k) logit = -INFINITY;
            float bv = logit;
            int bl = lane;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const float ov = __shfl_xor(bv, off, 64);
                const int ol = __shfl_xor(bl, off, 64);
                if (ov > bv || (ov == bv && ol < bl)) { bv = ov; bl = ol; }
            }
            const int pt = __shfl(cand, bl, 64);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");            // the candidates' loop is done with this curve's sCur
            const size_t o = (((size_t)b * C) * n + q) * curve_length + step;  // curves[b][c][q][step]
            if (has0) { cur0 = xb[(size_t)pt * C + c0]; sCur[q * C + c0] = cur0; curves[o + (size_t)c0 * n * curve_length] = cur0; }
            if (has1) { cur1 = xb[(size_t)pt * C + c1]; sCur[q * C + c1] = cur1; curves[o + (size_t)c1 * n * curve_length] = cur1; }
            if (lane == 0) { sPt[q] = pt; path[((size_t)b * n + q) * curve_length + step] = pt; }
        }
        __syncthreads();                                 // every curve's state is written before the next step's phase A reads sSm's slots anew
    }
}

__global__ __launch_bounds__(256) void curve_prepare_kernel(const float *__restrict__ x, const float *__restrict__ w_att, int C, int N,
                                                            float *__restrict__ xa, float *__restrict__ att)
{
    __shared__ float tile[CW_MAXC][CP_TILE + 1];
    __shared__ float sAtt[CP_TILE];
    const int b = blockIdx.y, n0 = blockIdx.x * CP_TILE, tid = threadIdx.x;
    const float *xb = x + (size_t)b * C * N;
    for (int e = tid; e < C * CP_TILE; e += 256) {
        const int c = e / CP_TILE, n = e % CP_TILE;
        tile[c][n] = n0 + n < N ? xb[(size_t)c * N + n0 + n] : 0.f;
    }
    __syncthreads();
    if (tid < CP_TILE) {
        float s = 0.f;
        for (int c = 0; c < C; c++) s += w_att[c] * tile[c][tid];
        const float a = 1.f / (1.f + expf(-s));
        sAtt[tid] = a;
        if (n0 + tid < N) att[(size_t)b * N + n0 + tid] = a;
    }
    __syncthreads();
    float *ob = xa + ((size_t)b * N + n0) * C;
    const int nvalid = min(CP_TILE, N - n0);
    for (int e = tid; e < nvalid * C; e += 256) {
        const int n = e / C, c = e - n * C;
        ob[e] = tile[c][n] * sAtt[n];
    }
}

extern "C" int l3d_curve_prepare(const float *x, const float *w_att, int B, int C, int N, float *xa, float *att, l3d_stream_t stream)
{
    L3D_REQUIRE(x && w_att && xa && att && B > 0 && C > 0 && N > 0);
    if (C % 16 || C > CW_MAXC || B > 65535) return L3D_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(curve_prepare_kernel, dim3(l3d_divup(N, CP_TILE), B), dim3(256), 0, (hipStream_t)stream, x, w_att, C, N, xa, att);
    return l3d_check_launch();
}

extern "C" int l3d_curve_walk(const float *x, const int64_t *adj, const int64_t *start, int B, int N, int C, int k, int curve_num,
                              int curve_length, const float *w_a, const float *a_scale, const float *a_shift, const float *w_m,
                              const float *m_scale, const float *m_shift, float *curves, int32_t *path, l3d_stream_t stream)
{
    L3D_REQUIRE(x && adj && start && w_a && a_scale && a_shift && w_m && m_scale && m_shift && curves && path);
    L3D_REQUIRE(B > 0 && N > 0 && C > 0 && k > 0 && curve_num > 0 && curve_length > 0);
    // the candidates' rows of x are read 16 bytes at a time (C % 16 == 0: every row starts where x does, modulo 16)
    if (C % 16 || C > CW_MAXC || k > 64 || curve_num > N || B > (1 << 24) || (((size_t)x) & 15)) return L3D_ERR_UNSUPPORTED;
    const size_t lds = (size_t)curve_num * (2 * C + 3) * sizeof(float);
    if (lds > CW_MAX_LDS) return L3D_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(curve_walk_kernel, dim3(B), dim3(CW_WAVES * 64), lds, (hipStream_t)stream, x, adj, start, N, C, k, curve_num,
                       curve_length, w_a, a_scale, a_shift, w_m, m_scale, m_shift, curves, path);
    return l3d_check_launch();
}
