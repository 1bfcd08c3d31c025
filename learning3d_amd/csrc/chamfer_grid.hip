// chamfer_grid.hip -- Chamfer nearest-neighbour search (fwd) with exact grid pruning, 1 <= N, M <= 2048.
//
// Same inputs, same outputs and the same bits as chamfer_fwd_packed_kernel<false, ...> (chamfer.hip): for every query the
// lexicographic minimum of (d, candidate index) with d = (dx*dx + dy*dy) + dz*dz, dx = p2 - p1, no contraction -- what one
// sequential strict-'<' scan over the candidates returns.  The all-pairs kernels evaluate every (query, candidate) pair; here a
// workgroup sorts the candidate cloud into G x G x G cells in LDS (counting sort, about two candidates per cell), a query looks
// at the 3 x 3 x 3 cells around its own, and an exact bound decides whether that answer is final.  Queries the bound does not
// decide are answered by an exact scan over all candidates afterwards, so the result never depends on the pruning.
//
// Cells.  lo = per-axis minimum of the candidates, ext = the largest of the three extents, G = clamp(floor(cbrt(Nc / 2)), 1, 12),
// s = fl(G / ext), rinv = fl(ext / G).  Along an axis cell(v) = clamp((int)fl(fl(v - lo) * s), 0, G - 1) (two separately rounded
// fp32 operations), linear id (cz * G + cy) * G + cx.  The 27 cells around a query are nine runs of the sorted image, because
// three x-adjacent cells are neighbours in id.
//
// The bound.  A query's answer from its 27 cells is final iff best < thr, thr = fl(fl(rinv * rinv) * (1 - 2^-12)):
//   - cell() is a monotone function of the coordinate, so a candidate outside the 27 cells differs from the query by >= 2 cells
//     on some axis (a query outside the candidates' box is clamped into a border cell, which only widens the difference);
//   - hence the two values fl(fl(v - lo) * s) of candidate and query differ by more than 1 on that axis;
//   - undoing the two roundings (each relative 2^-24, values at most G <= 16) gives |p2 - p1| >= (1 - 2^-18) / s on that axis;
//   - so the candidate's computed d >= rinv^2 (1 - 2^-17) > thr: no candidate outside the 27 cells can win or tie.
// The relative bounds need rinv^2 inside the normal range with room to spare: a cloud with rinv^2 outside [1e-30, 1e30] (ext == 0
// is the common case: one repeated point), or with any non-finite coordinate in the candidates or in the workgroup's queries,
// is answered by the exact scan for the whole workgroup.
//
// Every loop's trip count is known before it starts (a run's length from the scan, the list's length, Nc); no waits on other
// workgroups, no global atomic (the counters of the STATS instantiation aside, which only tests launch), no state after the launch.
#include "common.h"

#define GRID_THREADS 256
#define GRID_QPW 128                                       // queries per workgroup: two lanes per query, which split every run
#define GRID_MAXC 2048                                     // candidates: the sorted image is 16 B per point (MAXC = 1024 or 2048 per instantiation)
#define GRID_GMAX 12
#define GRID_SUB 64                                        // lanes per listed query in the exact scan: one wave

// The exact scan: list[e] = (x, y, z, query's slot) for e < L, img[t] = (x, y, z, candidate index) for t < Nc in any order.  A wave
// shares a query (4 queries per trip of the workgroup), lane j takes candidates j, j + 64, ... and the 64 partial
// (min, argmin) pairs meet by shuffle: lower d wins, equal d the lower index; NaN never wins; a query without a finite distance
// gets (inf, 0) as in chamfer_fwd_kernel.  A read clamped to the last candidate evaluates it twice, which changes nothing.
__device__ __forceinline__ void chamfer_grid_exact_scan(const float4 *img, int Nc, const float4 *list, int L, float *__restrict__ dq,
                                                        int32_t *__restrict__ iq, int tid)
{
    const int sub = tid & (GRID_SUB - 1), grp = tid / GRID_SUB;       // lane, wave
    for (int e0 = 0; e0 < L; e0 += GRID_THREADS / GRID_SUB) {
        const int e = e0 + grp;
        const float4 q = list[min(e, L - 1)];
        float best = INFINITY;
        int besti = 0x7fffffff;
        for (int t = sub; t < Nc; t += GRID_SUB * 8) {
            float4 c[8];
#pragma unroll
            for (int v = 0; v < 8; v++) c[v] = img[min(t + GRID_SUB * v, Nc - 1)];
#pragma unroll
            for (int v = 0; v < 8; v++) {
                const float dx = c[v].x - q.x, dy = c[v].y - q.y, dz = c[v].z - q.z;
                const float d = (dx * dx + dy * dy) + dz * dz;
                const int ci = __float_as_int(c[v].w);
                const bool take = d < best || (d == best && ci < besti);
                best = take ? d : best;
                besti = take ? ci : besti;
            }
        }
#pragma unroll
        for (int off = GRID_SUB / 2; off > 0; off >>= 1) {
            const float od = __shfl_xor(best, off, 64);
            const int oi = __shfl_xor(besti, off, 64);
            const bool take = od < best || (od == best && oi < besti);
            best = take ? od : best;
            besti = take ? oi : besti;
        }
        if (sub == 0 && e < L) {
            const int ql = __float_as_int(q.w);
            dq[ql] = best;
            iq[ql] = best < INFINITY ? besti : 0;
        }
    }
}

__device__ __forceinline__ int chamfer_grid_cell(float v, float lo, float s, float gm1)
{
    const float t = (v - lo) * s;                          // two roundings (-ffp-contract=off)
    return (int)fminf(fmaxf(t, 0.f), gm1);                 // == clamp((int)t, 0, G - 1), without converting a value outside int's range
}

// grid (ceil(max(N, M) / 128), B, 2 directions); MAXC: the most candidates the instantiation's LDS holds (1024: 21.7 KB, two
// workgroups fit on a CU beside two of knn_mfma_kernel's at N = 1024; 2048: 39 KB, one).  STATS: stats[0] += queries the bound decided,
// stats[1] += queries sent to the list, stats[2] += workgroups that took the exact scan as a whole (l3d_chamfer_forward_grid_stats;
// the product carries no counter)
template <int MAXC, bool STATS>
__global__ __launch_bounds__(GRID_THREADS) void chamfer_fwd_grid_kernel(const float *__restrict__ xyz1, const float *__restrict__ xyz2,
                                                                        int N, int M, float *__restrict__ dist1,
                                                                        float *__restrict__ dist2, int32_t *__restrict__ idx1,
                                                                        int32_t *__restrict__ idx2, int32_t *__restrict__ stats)
{
    constexpr int NS = MAXC / GRID_THREADS;                // candidates per thread, held in registers from the load to the scatter
    constexpr int PER = MAXC == 1024 ? 3 : 4;              // cells per thread in the scan: G <= 8 (513 entries) / G <= 10 (1001 entries)
    static_assert(MAXC == 1024 ? 2 * 9 * 9 * 9 > MAXC && PER * GRID_THREADS >= 8 * 8 * 8 + 1
                               : 2 * 11 * 11 * 11 > MAXC && PER * GRID_THREADS >= 10 * 10 * 10 + 1, "cellstart holds G^3 + 1 entries");
    __shared__ float4 img[MAXC];                           // candidates (x, y, z, index), sorted by cell
    __shared__ int cellstart[PER * GRID_THREADS];          // counts, then their exclusive scan; [G^3] = Nc
    __shared__ float4 list[GRID_QPW];                      // queries for the exact scan (x, y, z, slot in the block)
    __shared__ float red[GRID_THREADS / 64][8];
    __shared__ int wsum[GRID_THREADS / 64];
    __shared__ int listn;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ql = tid >> 1, half = tid & 1;               // lanes 2 ql and 2 ql + 1 share query ql of the block
    const int b = blockIdx.y;
    const int dir = blockIdx.z;
    const float *qs = dir == 0 ? xyz1 : xyz2;
    const float *cs = dir == 0 ? xyz2 : xyz1;
    const int Nq = dir == 0 ? N : M;
    const int Nc = dir == 0 ? M : N;
    const int q0 = blockIdx.x * GRID_QPW;
    if (q0 >= Nq) return;                                  // whole block out of range (grid is sized for max(N, M))
    float *dq = (dir == 0 ? dist1 : dist2) + (size_t)b * Nq + q0;
    int32_t *iq = (dir == 0 ? idx1 : idx2) + (size_t)b * Nq + q0;
    const int nq = min(GRID_QPW, Nq - q0);
    const bool qvalid = ql < nq;

    // 1. stage and bound.  Every load in flight before the first use, from clamped indices (chamfer_fwd_packed_kernel's staging): a
    // clamped duplicate is a point of the cloud (or a query of the block) and changes neither the bounds nor the finiteness test
    const float *cbase = cs + (size_t)b * Nc * 3;
    float px[NS], py[NS], pz[NS];
#pragma unroll
    for (int i = 0; i < NS; i++) {
        const float *cp = cbase + (size_t)min(tid + i * GRID_THREADS, Nc - 1) * 3;
        px[i] = cp[0]; py[i] = cp[1]; pz[i] = cp[2];
    }
    const float *qp = qs + ((size_t)b * Nq + q0 + min(ql, nq - 1)) * 3;
    const float qx = qp[0], qy = qp[1], qz = qp[2];
#pragma unroll
    for (int i = 0; i < PER; i++) cellstart[tid * PER + i] = 0;
    if (tid == 0) listn = 0;

    float lox = INFINITY, loy = INFINITY, loz = INFINITY, hix = -INFINITY, hiy = -INFINITY, hiz = -INFINITY;
    bool bad = !(fabsf(qx) < INFINITY) || !(fabsf(qy) < INFINITY) || !(fabsf(qz) < INFINITY);
#pragma unroll
    for (int i = 0; i < NS; i++)
        if (i * GRID_THREADS < Nc) {                       // uniform
            lox = fminf(lox, px[i]); loy = fminf(loy, py[i]); loz = fminf(loz, pz[i]);
            hix = fmaxf(hix, px[i]); hiy = fmaxf(hiy, py[i]); hiz = fmaxf(hiz, pz[i]);
            bad = bad || !(fabsf(px[i]) < INFINITY) || !(fabsf(py[i]) < INFINITY) || !(fabsf(pz[i]) < INFINITY);
        }
    {   // wave reduction on the VALU's DPP lanes up to 32 (l3d_group_max), one exchange for the last level; min(a, b) = -max(-a, -b)
        float r[6] = {-lox, -loy, -loz, hix, hiy, hiz};
#pragma unroll
        for (int i = 0; i < 6; i++) {
            r[i] = l3d_group_max(r[i], 32);
            r[i] = fmaxf(r[i], __shfl_xor(r[i], 32, 64));
        }
        lox = -r[0]; loy = -r[1]; loz = -r[2]; hix = r[3]; hiy = r[4]; hiz = r[5];
    }
    bad = __any(bad);
    if (lane == 0) {
        red[wave][0] = lox; red[wave][1] = loy; red[wave][2] = loz;
        red[wave][3] = hix; red[wave][4] = hiy; red[wave][5] = hiz;
        red[wave][6] = bad ? 1.f : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < GRID_THREADS / 64; w++) {
        lox = fminf(lox, red[w][0]); loy = fminf(loy, red[w][1]); loz = fminf(loz, red[w][2]);
        hix = fmaxf(hix, red[w][3]); hiy = fmaxf(hiy, red[w][4]); hiz = fmaxf(hiz, red[w][5]);
        bad = bad || red[w][6] != 0.f;
    }
    const float ext = fmaxf(fmaxf(hix - lox, hiy - loy), hiz - loz);

    // 2. cells
    int G = 1;
#pragma unroll
    for (int g = 2; g <= GRID_GMAX; g++) G = 2 * g * g * g <= Nc ? g : G;
    const float Gf = (float)G, gm1 = (float)(G - 1);
    const float s = Gf / ext, rinv = ext / Gf;
    const float r2 = rinv * rinv;
    const float thr = r2 * 0.999755859375f;                // 1 - 2^-12
    const bool whole = bad || !(r2 >= 1e-30f && r2 <= 1e30f);

    if (whole) {                                           // uniform: the exact scan for every query of the workgroup
#pragma unroll
        for (int i = 0; i < NS; i++) {
            const int t = tid + i * GRID_THREADS;
            if (t < Nc) img[t] = make_float4(px[i], py[i], pz[i], __int_as_float(t));
        }
        if (qvalid && half == 0) list[ql] = make_float4(qx, qy, qz, __int_as_float(ql));
        __syncthreads();
        chamfer_grid_exact_scan(img, Nc, list, nq, dq, iq, tid);
        if (STATS && tid == 0) atomicAdd(&stats[2], 1);
        return;
    }

    // 3. counting sort: the counting atomic's return value is the candidate's slot inside its cell
    int cid[NS], rank[NS];
#pragma unroll
    for (int i = 0; i < NS; i++) {
        cid[i] = 0; rank[i] = 0;
        if (tid + i * GRID_THREADS < Nc) {
            const int cx = chamfer_grid_cell(px[i], lox, s, gm1), cy = chamfer_grid_cell(py[i], loy, s, gm1), cz = chamfer_grid_cell(pz[i], loz, s, gm1);
            cid[i] = (cz * G + cy) * G + cx;
            rank[i] = atomicAdd(&cellstart[cid[i]], 1);
        }
    }
    __syncthreads();
    {
        int c[PER], sum = 0;
#pragma unroll
        for (int i = 0; i < PER; i++) { c[i] = cellstart[tid * PER + i]; sum += c[i]; }
        int incl = sum;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_up(incl, off, 64);
            incl += lane >= off ? o : 0;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        int pre = incl - sum;
#pragma unroll
        for (int w = 0; w < GRID_THREADS / 64 - 1; w++) pre += w < wave ? wsum[w] : 0;
#pragma unroll
        for (int i = 0; i < PER; i++) { cellstart[tid * PER + i] = pre; pre += c[i]; }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NS; i++) {
        const int t = tid + i * GRID_THREADS;
        if (t < Nc) img[cellstart[cid[i]] + rank[i]] = make_float4(px[i], py[i], pz[i], __int_as_float(t));
    }

    // 4. query: nine runs; rows outside the grid read cellstart[0] twice and are empty.  The query's two lanes take alternate
    // groups of four candidates of every run and merge once at the end.
    int rb[9], re[9];
    {
        const int cx = chamfer_grid_cell(qx, lox, s, gm1), cy = chamfer_grid_cell(qy, loy, s, gm1), cz = chamfer_grid_cell(qz, loz, s, gm1);
        const int x0 = max(cx - 1, 0), x1 = min(cx + 1, G - 1);
#pragma unroll
        for (int dz = -1; dz <= 1; dz++)
#pragma unroll
            for (int dy = -1; dy <= 1; dy++) {
                const int zz = cz + dz, yy = cy + dy;
                const bool ok = zz >= 0 && zz < G && yy >= 0 && yy < G;
                const int row = (zz * G + yy) * G;
                rb[(dz + 1) * 3 + dy + 1] = cellstart[ok ? row + x0 : 0] + 4 * half;
                re[(dz + 1) * 3 + dy + 1] = cellstart[ok ? row + x1 + 1 : 0];
            }
    }
    __syncthreads();
    // finite inputs: d is never NaN and never negative, so (d's bits, index) orders as one unsigned 64-bit key
    unsigned long long best = ((unsigned long long)0x7f800000u << 32) | 0x7fffffffu;
#pragma unroll
    for (int r = 0; r < 9; r++) {
        const int e = re[r];
        for (int p = rb[r]; p < e; p += 8) {
            float4 c[4];
#pragma unroll
            for (int v = 0; v < 4; v++) c[v] = img[min(p + v, e - 1)];        // a clamped read evaluates the run's last candidate again
#pragma unroll
            for (int v = 0; v < 4; v++) {
                const float dx = c[v].x - qx, dy = c[v].y - qy, dz = c[v].z - qz;
                const float d = (dx * dx + dy * dy) + dz * dz;
                const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | __float_as_uint(c[v].w);
                best = key < best ? key : best;
            }
        }
    }
    {
        const unsigned long long other = __shfl_xor(best, 1, 64);
        best = other < best ? other : best;
    }

    // 5. accept or list
    const float bd = __uint_as_float((unsigned)(best >> 32));
    if (qvalid && half == 0) {
        if (bd < thr) {
            dq[ql] = bd;
            iq[ql] = (int)(unsigned)best;
        } else {
            list[atomicAdd(&listn, 1)] = make_float4(qx, qy, qz, __int_as_float(ql));
        }
    }
    __syncthreads();
    const int L = listn;
    if (STATS && tid == 0) {
        atomicAdd(&stats[0], nq - L);
        atomicAdd(&stats[1], L);
    }
    chamfer_grid_exact_scan(img, Nc, list, L, dq, iq, tid);
}

template <int MAXC>
static void chamfer_grid_launch_maxc(dim3 grid, const float *xyz1, const float *xyz2, int N, int M, float *dist1, float *dist2, int32_t *idx1,
                                     int32_t *idx2, int32_t *stats, hipStream_t stream)
{
    if (stats)
        hipLaunchKernelGGL((chamfer_fwd_grid_kernel<MAXC, true>), grid, dim3(GRID_THREADS), 0, stream, xyz1, xyz2, N, M, dist1, dist2, idx1, idx2, stats);
    else
        hipLaunchKernelGGL((chamfer_fwd_grid_kernel<MAXC, false>), grid, dim3(GRID_THREADS), 0, stream, xyz1, xyz2, N, M, dist1, dist2, idx1, idx2,
                           (int32_t *)nullptr);
}

static int chamfer_grid_launch(const float *xyz1, const float *xyz2, int B, int N, int M, float *dist1, float *dist2, int32_t *idx1,
                               int32_t *idx2, int32_t *stats, hipStream_t stream)
{
    const int mx = N > M ? N : M;
    if (mx > GRID_MAXC) return L3D_ERR_UNSUPPORTED;
    dim3 grid(l3d_divup(mx, GRID_QPW), B, 2);
    if (mx <= 1024) chamfer_grid_launch_maxc<1024>(grid, xyz1, xyz2, N, M, dist1, dist2, idx1, idx2, stats, stream);
    else chamfer_grid_launch_maxc<GRID_MAXC>(grid, xyz1, xyz2, N, M, dist1, dist2, idx1, idx2, stats, stream);
    return l3d_check_launch();
}

// l3d_chamfer_forward_variant 4 (chamfer.hip); arguments checked there
int l3d_chamfer_forward_grid(const float *xyz1, const float *xyz2, int B, int N, int M, float *dist1, float *dist2, int32_t *idx1,
                             int32_t *idx2, hipStream_t stream)
{
    return chamfer_grid_launch(xyz1, xyz2, B, N, M, dist1, dist2, idx1, idx2, nullptr, stream);
}

extern "C" int l3d_chamfer_forward_grid_stats(const float *xyz1, const float *xyz2, int B, int N, int M, float *dist1, float *dist2,
                                              int32_t *idx1, int32_t *idx2, int32_t *stats, l3d_stream_t stream)
{
    L3D_REQUIRE(xyz1 && xyz2 && dist1 && dist2 && idx1 && idx2 && stats && B > 0 && N > 0 && M > 0);
    L3D_REQUIRE(B <= 65535);
    return chamfer_grid_launch(xyz1, xyz2, B, N, M, dist1, dist2, idx1, idx2, stats, (hipStream_t)stream);
}
