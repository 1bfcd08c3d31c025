// prnet.hip -- the two steps of PRNet's iteration (models/prnet.py) that no other kernel of the library serves.  Declared in
// include/ext/l3d_prnet.h.
//
//   l3d_prnet_keypoints           KeyPointNet (reference :218-243) behind `emb + emb_p`: one workgroup per cloud.  The squared norms
//                                 go into LDS as order-preserving integer keys, the K-th largest is found by masknet.hip's 4 x 8-bit
//                                 radix search, a prefix-sum compaction in ascending point index gives the selected list (uint16 in
//                                 LDS: N <= 16384), and the gathers run from that list: lanes along the keypoints, so a wave writes runs
//                                 of consecutive floats and reads ascending, mostly adjacent, addresses.  The channel means the
//                                 temperature head starts from are taken on the way: a wave passes its 8 x 64 tile through LDS and one
//                                 lane per channel adds the tile's 64 values (four chains of 16, joined pairwise) to its running sum.
//   l3d_soft_correspondence_pair  both directions of the SVD head's softmax(temperature S / sqrt(C)) and weighted point sum, flash-style
//                                 on v_mfma_f32_16x16x4_f32.  The two directions are the same kernel with the roles of the clouds
//                                 exchanged (grid.z).  Keys are the MFMA's rows and queries its columns: a lane (m = lane % 16, g = lane
//                                 / 16) holds the scores of keys 16 t + 4 g + r (t, r = 0 .. 3) of a 64-key tile with query m, so the
//                                 softmax over keys is a per-lane pass over 16 registers and two cross-lane maxima per tile, and the
//                                 value side (three floats per key) is VALU work on those registers.  A wave owns 16 queries; their
//                                 embedding columns stay in registers for the whole kernel (C / 4 of them: the B operands), the key
//                                 tile passes through LDS in chunks of 16 channels, double buffered, one barrier per chunk.
#include "common.h"
#include "split_bf16.h"          // f32x4
#include "../../include/ext/l3d_prnet.h"

// ------------------------------------------------------------------------------------------------------------------------------
#define PK_THREADS 1024
#define PK_AUX 512               // words of LDS behind the keys: histogram [256], the search's verdict [2], wave totals [16]
#define PK_CT 8                  // channels per wave tile of the gather
#define PK_PITCH 65              // floats per channel row of a tile: 64 keypoints + 1 (a lane per channel reads its row: 8 banks)
#define PK_TILE_WORDS ((PK_THREADS / 64) * PK_CT * PK_PITCH)

// order-preserving key (masknet.hip's): a > b as floats <=> key(a) > key(b); every NaN has the largest one
__device__ __forceinline__ uint32_t pk_key(float v)
{
    if (v != v) return 0xFFFFFFFFu;
    const uint32_t u = v == 0.f ? 0u : __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(PK_THREADS) void prnet_keypoints_kernel(const float *__restrict__ emb, const float *__restrict__ emb_p,
                                                                     const float *__restrict__ xyz, int C, int N, int K,
                                                                     int64_t *__restrict__ idx, float *__restrict__ xyz_k,
                                                                     float *__restrict__ emb_k, float *__restrict__ mean)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t pk_lds[];
    const int region = max(N, PK_TILE_WORDS);              // the keys first, the waves' gather tiles afterwards
    uint32_t *sKey = pk_lds, *sHist = pk_lds + region, *sSel = sHist + 256, *sWave = sSel + 2;
    uint16_t *sIdx = reinterpret_cast<uint16_t *>(pk_lds + region + PK_AUX);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    const float *eb = emb + (size_t)b * C * N;
    const float *pb = emb_p ? emb_p + (size_t)b * C * N : nullptr;
    const bool all = K == N;

    if (!all) {
        for (int i = tid; i < N; i += PK_THREADS) {
            float key = 0.f;
            if (pb) {
#pragma unroll 16
                for (int c = 0; c < C; c++) {
                    const float e = eb[(size_t)c * N + i] + pb[(size_t)c * N + i];
                    key = key + e * e;
                }
            } else {
#pragma unroll 16
                for (int c = 0; c < C; c++) {
                    const float e = eb[(size_t)c * N + i];
                    key = key + e * e;
                }
            }
            sKey[i] = pk_key(key);
        }
        // the K-th largest key, eight bits at a time from the top
        uint32_t prefix = 0, rem = (uint32_t)K;
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (tid < 256) sHist[tid] = 0;
            __syncthreads();                                   // (first trip: the keys are written, too)
            const uint32_t himask = shift == 24 ? 0u : (0xFFFFFFFFu << (shift + 8));
            for (int i = tid; i < N; i += PK_THREADS) {
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
        const uint32_t T = prefix, need = rem;                 // keys above T are in; of the keys equal to T, the first `need` by index

        // compaction in ascending index: thread t owns the points [t per, (t + 1) per)
        const int per = (N + PK_THREADS - 1) / PK_THREADS;
        const int i0 = min(tid * per, N), i1 = min(i0 + per, N);
        uint32_t cg = 0, ce = 0;
        for (int i = i0; i < i1; i++) {
            const uint32_t key = sKey[i];
            cg += key > T;
            ce += key == T;
        }
        const uint32_t mine = (ce << 16) | cg;                 // both totals <= 16384: no carry between the halves
        uint32_t incl = mine;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t o = __shfl_up(incl, off, 64);
            if (lane >= off) incl += o;
        }
        if (lane == 63) sWave[wave] = incl;
        __syncthreads();
        uint32_t before = incl - mine;
        for (int w = 0; w < wave; w++) before += sWave[w];
        uint32_t gb = before & 0xFFFFu, ebq = before >> 16;
        for (int i = i0; i < i1; i++) {
            const uint32_t key = sKey[i];
            const bool gt = key > T, eq = key == T;
            if (gt || (eq && ebq < need)) {
                const uint32_t p = gb + min(ebq, need);        // < K: exactly K points pass the test
                sIdx[p] = (uint16_t)i;
                if (idx) idx[(size_t)b * K + p] = i;
            }
            gb += gt;
            ebq += eq;
        }
        __syncthreads();                                       // the list is complete; the keys are not read again
    } else if (idx) {
        for (int p = tid; p < K; p += PK_THREADS) idx[(size_t)b * K + p] = p;
    }

    if (xyz_k) {
        const float *xb = xyz + (size_t)b * 3 * N;
        float *ob = xyz_k + (size_t)b * 3 * K;
        for (int t = tid; t < 3 * K; t += PK_THREADS) {
            const int d = t / K, p = t - d * K;
            ob[t] = xb[(size_t)d * N + (all ? p : (int)sIdx[p])];
        }
    }

    // the embedding: wave w takes the channels [256 r + 8 w, + 8) of round r, 64 keypoints at a time
    float *tile = reinterpret_cast<float *>(pk_lds) + wave * (PK_CT * PK_PITCH);
    const int rounds = (C + (PK_THREADS / 64) * PK_CT - 1) / ((PK_THREADS / 64) * PK_CT);
    for (int r = 0; r < rounds; r++) {
        const int c0 = (r * (PK_THREADS / 64) + wave) * PK_CT;
        const int nch = max(0, min(PK_CT, C - c0));            // uniform per wave; every wave runs every barrier
        float acc = 0.f, comp = 0.f;
        for (int k0 = 0; k0 < K; k0 += 64) {
            const int kn = min(64, K - k0);
            const int kk = min(k0 + lane, K - 1);              // a lane past the tail reads the last keypoint and stores nothing
            const int s = all ? kk : (int)sIdx[kk];
            float v[PK_CT];
#pragma unroll
            for (int ci = 0; ci < PK_CT; ci++) {
                v[ci] = 0.f;
                if (ci < nch) {
                    const size_t at = (size_t)(c0 + ci) * N + s;
                    v[ci] = pb ? eb[at] + pb[at] : eb[at];
                }
            }
            __syncthreads();                                   // the previous chunk's tile has been read
#pragma unroll
            for (int ci = 0; ci < PK_CT; ci++) {
                if (ci < nch) {
                    if (emb_k && k0 + lane < K) emb_k[((size_t)b * C + c0 + ci) * K + k0 + lane] = v[ci];
                    tile[ci * PK_PITCH + lane] = v[ci];
                }
            }
            __syncthreads();
            if (lane < nch) {
                // four chains over the chunk's quarters, joined pairwise, then onto the running sum: a fixed order
                float part[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int qd = 0; qd < 4; qd++)
#pragma unroll
                    for (int j = 16 * qd; j < 16 * qd + 16; j++)
                        if (j < kn) part[qd] = part[qd] + tile[lane * PK_PITCH + j];
                // Kahan's compensated step: with hundreds of chunks (K in the thousands) a plain running sum carried five times the
                // error of torch's blocked mean
                const float y = ((part[0] + part[1]) + (part[2] + part[3])) - comp;
                const float tsum = acc + y;
                comp = (tsum - acc) - y;
                acc = tsum;
            }
        }
        if (lane < nch) mean[(size_t)b * C + c0 + lane] = acc / (float)K;
    }
}

extern "C" int l3d_prnet_keypoints(const float *emb, const float *emb_p, const float *xyz, int B, int C, int N, int K, int64_t *idx,
                                   float *xyz_k, float *emb_k, float *mean, l3d_stream_t stream)
{
    L3D_REQUIRE(emb && mean && B > 0 && C > 0 && N > 0 && K > 0 && K <= N);
    L3D_REQUIRE(xyz || !xyz_k);
    if (N > L3D_PRNET_MAX_N || B > 65535) return L3D_ERR_UNSUPPORTED;
    const size_t region = (size_t)(N > PK_TILE_WORDS ? N : PK_TILE_WORDS);
    const size_t lds = (region + PK_AUX + ((size_t)K + 1) / 2) * sizeof(uint32_t);
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void *)prnet_keypoints_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) { g_l3d_last_hip_error = (int)e; return L3D_ERR_LAUNCH; }
    }
    hipLaunchKernelGGL(prnet_keypoints_kernel, dim3(B), dim3(PK_THREADS), lds, (hipStream_t)stream, emb, emb_p, xyz, C, N, K, idx, xyz_k,
                       emb_k, mean);
    return l3d_check_launch();
}

// ------------------------------------------------------------------------------------------------------------------------------
#define SP_TQ 64                 // queries per workgroup: 4 waves x 16
#define SP_TK 64                 // keys per tile: four 16-row MFMA tiles
#define SP_KC 16                 // channels per staged chunk (C % 16 == 0: every chunk is full)
#define SP_PITCH 80              // floats per channel row of a chunk in LDS: lane (m, g) reads row 4 s + g at 16 t + m, and
                                 // 80 g + m puts the two g of a 32-lane half on banks m and 16 + m
#define SP_LOG2E 1.44269504088896340736f

template <int CMAX>
__global__ __launch_bounds__(256) void softcorr_pair_kernel(const float *__restrict__ src_emb, const float *__restrict__ tgt_emb,
                                                            const float *__restrict__ src, const float *__restrict__ tgt,
                                                            const float *__restrict__ temperature, int C, int N, int M,
                                                            float inv_sqrt_c, int first_dir, float *__restrict__ corr_ab,
                                                            float *__restrict__ corr_ba)
{
    __shared__ float sK[2][SP_KC * SP_PITCH];
    __shared__ __attribute__((aligned(16))) float sV[3][3 * SP_TK];     // three buffers: see where the next tile's values are put
    const int dir = first_dir + blockIdx.z, b = blockIdx.y;
    const int NQ = dir ? M : N, NK = dir ? N : M;
    if ((int)blockIdx.x * SP_TQ >= NQ) return;                 // the grid is as wide as the longer direction
    const float *qe = (dir ? tgt_emb : src_emb) + (size_t)b * C * NQ;
    const float *ke = (dir ? src_emb : tgt_emb) + (size_t)b * C * NK;
    const float *val = (dir ? src : tgt) + (size_t)b * 3 * NK;
    float *out = (dir ? corr_ba : corr_ab) + (size_t)b * 3 * NQ;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, m = lane & 15, g = lane >> 4;
    const int i0 = blockIdx.x * SP_TQ + wave * 16;
    const bool active = i0 < NQ;                               // per wave: a wave past the end only helps staging
    const int qi = min(i0 + m, NQ - 1);

    // the B operand of k-step s: channel 4 s + g of this lane's query
    float qf[CMAX / 4];
#pragma unroll
    for (int s = 0; s < CMAX / 4; s++) qf[s] = 4 * s < C ? qe[(size_t)(4 * s + g) * NQ + qi] : 0.f;

    const float sc = temperature[b] * inv_sqrt_c;
    const int nch = C / SP_KC, ntile = (NK + SP_TK - 1) / SP_TK;

    // staging: thread t carries key t % 64 of the channels t / 64 + 4 i (256 contiguous bytes per wave and channel row); keys past
    // the end read key NK - 1 and get weight 0 where the probabilities are formed.  Threads < 192 carry the tile's values.
    const int skey = t & 63, sch = t >> 6;
    float kr[4], vr = 0.f;
    {
        const float *p = ke + (size_t)sch * NK + min(skey, NK - 1);
#pragma unroll
        for (int i = 0; i < 4; i++) kr[i] = p[(size_t)(4 * i) * NK];
        if (t < 192) vr = val[(size_t)sch * NK + min(skey, NK - 1)];
#pragma unroll
        for (int i = 0; i < 4; i++) sK[0][(sch + 4 * i) * SP_PITCH + skey] = kr[i];
        if (t < 192) sV[0][t] = vr;
    }
    __syncthreads();

    float m_run = -INFINITY, l_run = 0.f, o0 = 0.f, o1 = 0.f, o2 = 0.f;   // of this lane's query over this lane's keys (m_run: all keys)
    int cnt = 0, vb = 0;                                       // vb = tile % 3: the value buffer of this tile
    for (int tile = 0; tile < ntile; tile++) {
        const int vnext = vb == 2 ? 0 : vb + 1;
        f32x4 acc[4];
#pragma unroll
        for (int tt = 0; tt < 4; tt++) acc[tt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ch = 0; ch < CMAX / SP_KC; ch++) {
            if (ch < nch) {                                    // uniform
                const bool last = ch + 1 == nch;
                const int nt = last ? tile + 1 : tile, nc = last ? 0 : ch + 1;
                const bool more = nt < ntile;
                if (more) {                                    // the next chunk's loads are in flight under this chunk's MFMAs
                    const float *p = ke + (size_t)(nc * SP_KC + sch) * NK + min(nt * SP_TK + skey, NK - 1);
#pragma unroll
                    for (int i = 0; i < 4; i++) kr[i] = p[(size_t)(4 * i) * NK];
                    if (last && t < 192) vr = val[(size_t)sch * NK + min(nt * SP_TK + skey, NK - 1)];
                }
                if (active) {
                    const float *a = sK[cnt & 1] + g * SP_PITCH + m;
#pragma unroll
                    for (int ss = 0; ss < 4; ss++)
#pragma unroll
                        for (int tt = 0; tt < 4; tt++)
                            acc[tt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * ss * SP_PITCH + 16 * tt], qf[4 * ch + ss], acc[tt], 0, 0, 0);
                }
                if (more) {
                    // the other buffer: every wave left the previous chunk's reads of it behind at the barrier that ended that chunk
                    float *d = sK[(cnt + 1) & 1];
#pragma unroll
                    for (int i = 0; i < 4; i++) d[(sch + 4 * i) * SP_PITCH + skey] = kr[i];
                    // tile + 1's values go into the buffer tile - 2 used.  With one chunk per tile (C == 16) a slower wave may still be
                    // in tile - 1's softmax, which runs behind that tile's only barrier and reads tile - 1's buffer: two buffers
                    // would be a race there.  Tile - 2's softmax lies before the barrier of tile - 1, which this wave has passed.
                    if (last && t < 192) sV[vnext][t] = vr;
                }
                __syncthreads();
                cnt++;
            }
        }
        if (active) {
            // acc[tt][r] = S of key j0 + 16 tt + 4 g + r with this lane's query.  Key j0 is always inside, so the maximum over the
            // four lanes of a query is a number.
            const int kb = tile * SP_TK + 4 * g;
            const float *vt = sV[vb] + 4 * g;
            float lg[16], mx = -INFINITY;
#pragma unroll
            for (int tt = 0; tt < 4; tt++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    lg[4 * tt + r] = acc[tt][r] * sc;
                    if (kb + 16 * tt + r < NK) mx = fmaxf(mx, lg[4 * tt + r]);
                }
            mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float m_new = fmaxf(m_run, mx);
            const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * SP_LOG2E);      // first tile: exp2(-inf) = 0
            m_run = m_new;
            l_run *= alpha; o0 *= alpha; o1 *= alpha; o2 *= alpha;
#pragma unroll
            for (int tt = 0; tt < 4; tt++) {
                const float4 v0 = *reinterpret_cast<const float4 *>(vt + 16 * tt);
                const float4 v1 = *reinterpret_cast<const float4 *>(vt + SP_TK + 16 * tt);
                const float4 v2 = *reinterpret_cast<const float4 *>(vt + 2 * SP_TK + 16 * tt);
                const float a0[4] = {v0.x, v0.y, v0.z, v0.w}, a1[4] = {v1.x, v1.y, v1.z, v1.w}, a2[4] = {v2.x, v2.y, v2.z, v2.w};
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    float e = __builtin_amdgcn_exp2f((lg[4 * tt + r] - m_new) * SP_LOG2E);
                    e = kb + 16 * tt + r < NK ? e : 0.f;
                    l_run += e;
                    o0 = fmaf(e, a0[r], o0);
                    o1 = fmaf(e, a1[r], o1);
                    o2 = fmaf(e, a2[r], o2);
                }
            }
        }
        vb = vnext;
    }

    if (active) {                                              // the four lanes of a query: the same bits in each
        l_run += __shfl_xor(l_run, 16, 64); o0 += __shfl_xor(o0, 16, 64); o1 += __shfl_xor(o1, 16, 64); o2 += __shfl_xor(o2, 16, 64);
        l_run += __shfl_xor(l_run, 32, 64); o0 += __shfl_xor(o0, 32, 64); o1 += __shfl_xor(o1, 32, 64); o2 += __shfl_xor(o2, 32, 64);
        if (g < 3 && i0 + m < NQ) out[(size_t)g * NQ + i0 + m] = (g == 0 ? o0 : g == 1 ? o1 : o2) / l_run;
    }
}

extern "C" size_t l3d_soft_correspondence_pair_workspace_bytes(int B, int N, int M)
{
    (void)B; (void)N; (void)M;
    return 0;
}

template <int CMAX>
static int sp_launch(dim3 grid, hipStream_t st, const float *src_emb, const float *tgt_emb, const float *src, const float *tgt,
                     const float *temperature, int C, int N, int M, int first_dir, float *corr_ab, float *corr_ba)
{
    hipLaunchKernelGGL((softcorr_pair_kernel<CMAX>), grid, dim3(256), 0, st, src_emb, tgt_emb, src, tgt, temperature, C, N, M,
                       1.0f / sqrtf((float)C), first_dir, corr_ab, corr_ba);
    return l3d_check_launch();
}

extern "C" int l3d_soft_correspondence_pair(const float *src_emb, const float *tgt_emb, const float *src, const float *tgt,
                                            const float *temperature, int B, int C, int N, int M, void *workspace, float *corr_ab,
                                            float *corr_ba, l3d_stream_t stream)
{
    (void)workspace;
    L3D_REQUIRE(src_emb && tgt_emb && temperature && (corr_ab || corr_ba) && B > 0 && C > 0 && N > 0 && M > 0);
    L3D_REQUIRE((!corr_ab || tgt) && (!corr_ba || src));
    if (C % 16 || C < 16 || C > L3D_SOFTCORR_PAIR_MAX_C || B > 65535) return L3D_ERR_UNSUPPORTED;
    const int first_dir = corr_ab ? 0 : 1, ndir = (corr_ab ? 1 : 0) + (corr_ba ? 1 : 0);
    const int nq = ndir == 2 ? (N > M ? N : M) : (corr_ab ? N : M);
    const dim3 grid(l3d_divup(nq, SP_TQ), B, ndir);
    hipStream_t st = (hipStream_t)stream;
    if (C <= 64) return sp_launch<64>(grid, st, src_emb, tgt_emb, src, tgt, temperature, C, N, M, first_dir, corr_ab, corr_ba);
    if (C <= 128) return sp_launch<128>(grid, st, src_emb, tgt_emb, src, tgt, temperature, C, N, M, first_dir, corr_ab, corr_ba);
    if (C <= 256) return sp_launch<256>(grid, st, src_emb, tgt_emb, src, tgt, temperature, C, N, M, first_dir, corr_ab, corr_ba);
    return sp_launch<512>(grid, st, src_emb, tgt_emb, src, tgt, temperature, C, N, M, first_dir, corr_ab, corr_ba);
}
