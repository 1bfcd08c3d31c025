// partial.hip -- partial and noisy registration pairs on the device.  Declared in include/ext/l3d_partial.h.
//
//   l3d_crop_select   the crop of the reference's farthest_subsample_points (the K points nearest a far view point, nearest first)
//                     and planar_crop (the K points farthest along a normal, in index order), with jitter_pointcloud's clamped noise
//                     added in the gather.  One workgroup per cloud.  The fp64 keys go into LDS as order-preserving 64-bit integers
//                     (nearest mode stores the complement, so both modes select the K LARGEST integers, ties to the lower index);
//                     the K-th largest is found by masknet.hip's radix search, 8 x 8 bits here; a prefix-sum compaction in
//                     ascending point index gives the selected list (uint16 in LDS).  Nearest mode then ranks the selected among
//                     themselves: a thread keeps the keys of its (up to 8) list entries in registers and walks the list once, every
//                     lane reading the same LDS word (a broadcast), and writes entry p to position rank(p) of a second list.  The
//                     gather runs from the final list with lanes along the output's floats: coalesced writes and noise reads.
//                     Latency-bound by construction: B workgroups on 256 CUs, ~30 barriers each.
#include "common.h"
#include "../../include/ext/l3d_partial.h"

#define CS_THREADS 1024
#define CS_AUX 512               // words of LDS behind the keys: histogram [256], the search's verdict [2], wave totals [16]
#define CS_SLOTS (L3D_CROP_MAX_N / CS_THREADS)      // list entries a thread ranks in nearest mode

// order-preserving key: a > b as doubles <=> key(a) > key(b); every NaN has the largest one; -0 == +0
__device__ __forceinline__ uint64_t cs_key(double v)
{
    if (v != v) return ~0ull;
    const uint64_t u = v == 0.0 ? 0ull : (uint64_t)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__global__ __launch_bounds__(CS_THREADS) void crop_select_kernel(const float *__restrict__ points, const double *__restrict__ vec,
                                                                 const float *__restrict__ centre, int N, int C, int mode, int K,
                                                                 const float *__restrict__ noise, const float *__restrict__ sigma,
                                                                 float clip, int64_t *__restrict__ idx, float *__restrict__ mask,
                                                                 float *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) uint64_t cs_lds[];
    const int kpad = (K + 7) & ~7;                             // uint16 entries per list: a multiple of 16 bytes
    uint64_t *sKey = cs_lds;
    uint32_t *sHist = reinterpret_cast<uint32_t *>(cs_lds + N), *sSel = sHist + 256, *sWave = sSel + 2;
    uint16_t *sIdx = reinterpret_cast<uint16_t *>(sHist + CS_AUX), *sOrd = sIdx + kpad;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    const float *pb = points + (size_t)b * N * C;
    const bool nearest = mode == L3D_CROP_NEAREST;
    const bool all = !nearest && K == N;                       // the jitter alone: nothing is ranked
    const uint16_t *list = sIdx;                               // the selected points in the mode's order

    if (!all) {
        if (nearest) {
            const double vx = vec[3 * b], vy = vec[3 * b + 1], vz = vec[3 * b + 2];
            for (int i = tid; i < N; i += CS_THREADS) {
                const float *p = pb + (size_t)i * C;
                const double dx = (double)p[0] - vx, dy = (double)p[1] - vy, dz = (double)p[2] - vz;
                const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
                sKey[i] = ~cs_key((xx + yy) + zz);             // the complement: the nearest point has the largest integer
            }
        } else {
            const double nx = vec[3 * b], ny = vec[3 * b + 1], nz = vec[3 * b + 2];
            const float cx = centre[3 * b], cy = centre[3 * b + 1], cz = centre[3 * b + 2];
            for (int i = tid; i < N; i += CS_THREADS) {
                const float *p = pb + (size_t)i * C;
                const float fx = p[0] - cx, fy = p[1] - cy, fz = p[2] - cz;
                const double xx = (double)fx * nx, yy = (double)fy * ny, zz = (double)fz * nz;
                sKey[i] = cs_key((xx + yy) + zz);
            }
        }
        // the K-th largest key, eight bits at a time from the top
        uint64_t prefix = 0;
        uint32_t rem = (uint32_t)K;
        for (int shift = 56; shift >= 0; shift -= 8) {
            if (tid < 256) sHist[tid] = 0;
            __syncthreads();                                   // (first trip: the keys are written, too)
            const uint64_t himask = shift == 56 ? 0ull : (~0ull << (shift + 8));
            for (int i = tid; i < N; i += CS_THREADS) {
                const uint64_t key = sKey[i];
                if ((key & himask) == prefix) atomicAdd(&sHist[(uint32_t)(key >> shift) & 255u], 1u);
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
            prefix |= (uint64_t)sSel[0] << shift;
            rem = sSel[1];
        }
        const uint64_t T = prefix;                             // keys above T are in; of the keys equal to T, the first `need` by index
        const uint32_t need = rem;

        // compaction in ascending index: thread t owns the points [t per, (t + 1) per), per <= CS_SLOTS, and keeps their keys in
        // registers, so that the selected keys can be packed to the front of sKey behind the barrier of the scan (nearest mode
        // ranks them there: one LDS read per comparison partner instead of two dependent ones)
        const int per = (N + CS_THREADS - 1) / CS_THREADS;
        const int i0 = min(tid * per, N);
        uint64_t kr[CS_SLOTS];
        uint32_t cg = 0, ce = 0;
#pragma unroll
        for (int s = 0; s < CS_SLOTS; s++) {
            kr[s] = 0;
            if (s < per && i0 + s < N) {
                kr[s] = sKey[i0 + s];
                cg += kr[s] > T;
                ce += kr[s] == T;
            }
        }
        const uint32_t mine = (ce << 16) | cg;                 // both totals <= 8192: no carry between the halves
        uint32_t incl = mine;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t o = __shfl_up(incl, off, 64);
            if (lane >= off) incl += o;
        }
        if (lane == 63) sWave[wave] = incl;
        __syncthreads();                                       // every thread has read its keys
        uint32_t before = incl - mine;
        for (int w = 0; w < wave; w++) before += sWave[w];
        uint32_t gb = before & 0xFFFFu, ebq = before >> 16;
#pragma unroll
        for (int s = 0; s < CS_SLOTS; s++) {
            if (s < per && i0 + s < N) {
                const bool gt = kr[s] > T, eq = kr[s] == T;
                const bool in = gt || (eq && ebq < need);
                if (in) {
                    const uint32_t p = gb + min(ebq, need);    // < K: exactly K points pass the test
                    sIdx[p] = (uint16_t)(i0 + s);
                    sKey[p] = kr[s];
                }
                if (mask) mask[(size_t)b * N + i0 + s] = in ? 1.f : 0.f;
                gb += gt;
                ebq += eq;
            }
        }
        __syncthreads();                                       // the list is complete: sKey[p] is the key of point sIdx[p]

        if (nearest) {
            // rank among the selected: entry p goes to position #{q : key_q > key_p, or key_q == key_p and q < p} (the list is in
            // ascending index order, so q < p is the lower index)
            const int nslot = (K + CS_THREADS - 1) / CS_THREADS;         // uniform
            uint64_t kp[CS_SLOTS];
            uint32_t rk[CS_SLOTS];
#pragma unroll
            for (int s = 0; s < CS_SLOTS; s++) {
                rk[s] = 0;
                kp[s] = 0;
                if (s < nslot) kp[s] = sKey[min(s * CS_THREADS + tid, K - 1)];
            }
#pragma unroll 4
            for (int q = 0; q < K; q++) {
                const uint64_t kq = sKey[q];                   // one address per wave: a broadcast
#pragma unroll
                for (int s = 0; s < CS_SLOTS; s++)
                    if (s < nslot) rk[s] += (kq > kp[s]) || (kq == kp[s] && q < s * CS_THREADS + tid);
            }
#pragma unroll
            for (int s = 0; s < CS_SLOTS; s++)
                if (s < nslot && s * CS_THREADS + tid < K) sOrd[rk[s]] = sIdx[s * CS_THREADS + tid];
            __syncthreads();
            list = sOrd;
        }
    } else if (mask) {
        for (int i = tid; i < N; i += CS_THREADS) mask[(size_t)b * N + i] = 1.f;
    }

    if (idx)
        for (int p = tid; p < K; p += CS_THREADS) idx[(size_t)b * K + p] = all ? p : (int)list[p];

    if (out) {
        const size_t ob = (size_t)b * K * C;
        const float sg = (noise && sigma) ? sigma[b] : 1.f;
        for (int t = tid; t < K * C; t += CS_THREADS) {
            const int p = t / C, c = t - p * C;
            float v = pb[(size_t)(all ? p : (int)list[p]) * C + c];
            if (noise) {
                float e = noise[ob + t];
                if (sigma) e = sg * e;
                if (clip > 0.f) e = e < -clip ? -clip : (e > clip ? clip : e);      // a NaN passes both tests and stays
                v = v + e;
            }
            out[ob + t] = v;
        }
    }
}

extern "C" int l3d_crop_select(const float *points, const double *vec, const float *centre, int B, int N, int C, int mode, int K,
                               const float *noise, const float *sigma, float clip, int64_t *idx, float *mask, float *out,
                               l3d_stream_t stream)
{
    L3D_REQUIRE(points && B > 0 && N > 0 && C > 0 && K > 0 && K <= N);
    L3D_REQUIRE(mode == L3D_CROP_NEAREST || mode == L3D_CROP_PLANE);
    L3D_REQUIRE(idx || mask || out);
    const bool all = mode == L3D_CROP_PLANE && K == N;
    L3D_REQUIRE(all || vec);
    L3D_REQUIRE(all || mode == L3D_CROP_NEAREST || centre);
    if (N > L3D_CROP_MAX_N || B > 65535 || C < 3 || (long)N * C > 0x7FFFFFFFl) return L3D_ERR_UNSUPPORTED;
    const size_t kpad = ((size_t)K + 7) & ~(size_t)7;
    const size_t lds = (size_t)N * sizeof(uint64_t) + CS_AUX * sizeof(uint32_t) + 2 * kpad * sizeof(uint16_t);
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void *)crop_select_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) { g_l3d_last_hip_error = (int)e; return L3D_ERR_LAUNCH; }
    }
    hipLaunchKernelGGL(crop_select_kernel, dim3(B), dim3(CS_THREADS), lds, (hipStream_t)stream, points, vec, centre, N, C, mode, K, noise,
                       sigma, clip, idx, mask, out);
    return l3d_check_launch();
}
