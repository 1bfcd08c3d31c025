// conv_split.hip -- per-point linear layer (1x1 conv + folded BN + ReLU) with fp32 operands split
// into three bf16 planes and multiplied on the bf16 matrix cores ("bf16x3", 6 products).
//
// Why.  v_mfma_f32_32x32x2_f32 runs at the fp32 VECTOR rate (157 TFLOP/s); v_mfma_f32_32x32x16_bf16
// runs 16x faster.  An fp32 value x is EXACTLY h + m + l with h = bf16(x), m = bf16(x - h),
// l = bf16(x - h - m) (8 + 8 + 8 significand bits, every remainder exact in fp32).  Then
//     w * x = wh*xh + (wh*xm + wm*xh) + (wh*xl + wl*xh + wm*xm) + O(2^-26 |w x|)
// and each bf16 x bf16 product is exact in the fp32 accumulator, so six bf16 MFMAs reproduce the fp32
// product to ~2^-24 relative -- the rounding level of an fp32 FMA chain -- at 6/16 of the cost of the
// fp32 MFMA.  (tests/test_gpu_parity.py::test_conv_split_accuracy checks the error against an fp64
// reference and against the fp32-MFMA kernel's own error.)  models/dgcnn.py:48, pointnet.py:22-49,
// pcn.py:84-125 are the layers this serves.
//
// Shape of the kernel.  y[b][co][n] = act(scale[co] * sum_k W[co][k] x[b][n][k] + shift[b][co]).
//   * workgroup tile 256 (co) x 256 (n), 512 threads = 8 waves (2 x 4), wave tile 128 x 64 =
//     4 x 2 MFMA tiles of 32x32 (128 accumulator registers).  A 256x256 tile keeps the L2 -> LDS
//     operand stream at ~13 B/clk/CU (~8 TB/s chip-wide, L2 gives ~34): with 2.7x less MFMA time per
//     FLOP than the fp32 kernel the 128x128 tile of mlp.hip would be operand-bound.
//   * K chunks of 16 (one MFMA k-step), double-buffered in LDS (2 x 48.75 KB), ONE barrier per chunk.
//   * both operands are "K-contiguous rows": lane (i = l&31, kg = l>>5) of the 32x32x16 MFMA needs
//     8 consecutive k of row i = one ds_read_b128.  LDS layout per plane: [kg][row][8 bf16], so the
//     16 lanes one b128 read cycle serves touch 16 distinct 4-bank slots (no padding needed).
//   * W arrives pre-split and pre-tiled ([k-chunk][plane][kg][Cout][8], l3d_conv_split_weights):
//     each (chunk, plane, kg) block of a tile is one contiguous 4 KB run.
//   * x arrives as fp32 (channel-last or channel-first) and is split while it is staged
//     (11 VALU per pair of elements, once per element per workgroup), or pre-split in the same tiled
//     layout as W (XMODE 2; written by the split EdgeConv kernel's epilogue).
#include "common.h"

#include "split_bf16.h"

#ifndef CS_PROBE
#define CS_PROBE 0          // tools/probe_conv_split.hip: bit 0 no global loads, 1 no LDS stores, 2 no MFMA, 3 no LDS reads, 4 no barrier
#endif
#define CS_TM 256
#define CS_TN 256
#define CS_TK 16
#define CS_REGION (256 * 16 + 64)           // bytes of one (plane, kg) region (+64: write-side bank skew)
#define CS_BUF (12 * CS_REGION)             // W: 6 regions, X: 6 regions
#define CS_LDS (3 * CS_BUF)                 // three LDS chunk buffers: the next-but-one chunk is staged inside the MFMA stream

// ---------------------------------------------------------------------------------------------
// Weight (or activation) splitter: src [R][C] fp32 row-major -> dst [ceil(C/16)][3][2][R][8] bf16.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void split_rows_kernel(const float *__restrict__ src, int R, int C,
                                                         uint4 *__restrict__ dst)
{
    const int nkc = (C + 15) / 16;
    const long total = (long)R * nkc * 2;
    const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= total) return;
    const int row = (int)(id % R);
    const int oct = (int)(id / R);                 // kc*2 + kg
    const int k0 = oct * 8;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; e++) v[e] = (k0 + e < C) ? src[(size_t)row * C + k0 + e] : 0.f;
    uint4 h, m, l;
    split8(v, h, m, l);
    const int kc = oct >> 1, kg = oct & 1;
    dst[(((size_t)kc * 3 + 0) * 2 + kg) * R + row] = h;
    dst[(((size_t)kc * 3 + 1) * 2 + kg) * R + row] = m;
    dst[(((size_t)kc * 3 + 2) * 2 + kg) * R + row] = l;
}

// ---------------------------------------------------------------------------------------------
// XMODE 0: x [B][Cin][N] fp32   1: x [B][N][Cin] fp32   2: x pre-split [Cin/16][3][2][B*N][8] bf16
// Requires Cout % 256 == 0, N % 256 == 0, Cin % 16 == 0 (dispatcher checks).
// ---------------------------------------------------------------------------------------------
template <int XMODE>
__global__ __launch_bounds__(512) void conv_split_kernel(const void *__restrict__ xin,
                                                         const uint4 *__restrict__ wsplit,
                                                         const float *__restrict__ scale,
                                                         const float *__restrict__ shift, int shift_bstride,
                                                         int Bn, int Cin, int Cout, int N, int relu,
                                                         float *__restrict__ y, int pool)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int n0 = blockIdx.x * CS_TN, co0 = blockIdx.y * CS_TM, b = blockIdx.z;
    const int nk = Cin / CS_TK;
    // Every workgroup walks the K chunks in a different rotation: otherwise all ~256 resident
    // workgroups request the SAME 24 KB of W from L2 in the same microsecond (measured: W loads
    // 3x slower than the x loads).  Workgroups that share an x tile (same blockIdx.x/z) share the
    // rotation, so their x reads still coincide in L2.
#ifndef CS_ROT
#define CS_ROT 0
#endif
    const int rot = ((blockIdx.x + gridDim.x * blockIdx.z) * CS_ROT) % nk;

    // ---- staging assignments
    const int wrow = t & 255, wkg = t >> 8;                           // W (and pre-split X): 3 planes each
    const int xrow = (XMODE == 1) ? (t >> 1) : (t & 255);             // fp32 X: one octet of one row
    const int xkg = (XMODE == 1) ? (t & 1) : (t >> 8);
    const uint4 *wsrc = wsplit + (size_t)wkg * Cout + co0 + wrow;      // + ((kc*3 + p)*2) * Cout
    const size_t BN = (size_t)Bn * N;
    const uint4 *xsrc2 = (const uint4 *)xin + (size_t)wkg * BN + (size_t)b * N + n0 + wrow;
    const float *xsrc1 = (const float *)xin + ((size_t)b * N + n0 + xrow) * Cin + xkg * 8;
    const float *xsrc0 = (const float *)xin + ((size_t)b * Cin + xkg * 8) * N + n0 + xrow;
    const int w_lds = wkg * CS_REGION + wrow * 16;                     // + p * 2 * CS_REGION
    const int x_lds = 6 * CS_REGION + ((XMODE == 2) ? w_lds : (xkg * CS_REGION + xrow * 16));

    // staging registers (plain scalars: arrays captured by lambdas ended up in scratch memory)
    uint4 w0, w1, w2, x0, x1, x2;
    f32x4 xa, xb;

#define CS_LOAD_GLOBAL(KCI)                                                                          \
    do {                                                                                             \
        const int kc_ = ((KCI) + rot >= nk) ? (KCI) + rot - nk : (KCI) + rot;                        \
        w0 = wsrc[((size_t)kc_ * 3 + 0) * 2 * Cout];                                                 \
        w1 = wsrc[((size_t)kc_ * 3 + 1) * 2 * Cout];                                                 \
        w2 = wsrc[((size_t)kc_ * 3 + 2) * 2 * Cout];                                                 \
        if (XMODE == 2) {                                                                            \
            x0 = xsrc2[((size_t)kc_ * 3 + 0) * 2 * BN];                                              \
            x1 = xsrc2[((size_t)kc_ * 3 + 1) * 2 * BN];                                              \
            x2 = xsrc2[((size_t)kc_ * 3 + 2) * 2 * BN];                                              \
        } else if (XMODE == 1) {                                                                     \
            xa = *(const f32x4 *)(xsrc1 + kc_ * CS_TK);                                              \
            xb = *(const f32x4 *)(xsrc1 + kc_ * CS_TK + 4);                                          \
        } else {                                                                                     \
            const float *q_ = xsrc0 + (size_t)kc_ * CS_TK * N;                                       \
            xa[0] = q_[0]; xa[1] = q_[(size_t)N]; xa[2] = q_[(size_t)2 * N]; xa[3] = q_[(size_t)3 * N];                   \
            xb[0] = q_[(size_t)4 * N]; xb[1] = q_[(size_t)5 * N]; xb[2] = q_[(size_t)6 * N]; xb[3] = q_[(size_t)7 * N];   \
        }                                                                                            \
    } while (0)

#define CS_STORE_LDS(BUF)                                                                            \
    do {                                                                                             \
        unsigned char *base_ = lds + (BUF) * CS_BUF;                                                 \
        if (XMODE != 2) {                                                                            \
            split_pair(xa[0], xa[1], x0.x, x1.x, x2.x);                                              \
            split_pair(xa[2], xa[3], x0.y, x1.y, x2.y);                                              \
            split_pair(xb[0], xb[1], x0.z, x1.z, x2.z);                                              \
            split_pair(xb[2], xb[3], x0.w, x1.w, x2.w);                                              \
        }                                                                                            \
        *(uint4 *)(base_ + w_lds) = w0;                                                              \
        *(uint4 *)(base_ + w_lds + 2 * CS_REGION) = w1;                                              \
        *(uint4 *)(base_ + w_lds + 4 * CS_REGION) = w2;                                              \
        *(uint4 *)(base_ + x_lds) = x0;                                                              \
        *(uint4 *)(base_ + x_lds + 2 * CS_REGION) = x1;                                              \
        *(uint4 *)(base_ + x_lds + 4 * CS_REGION) = x2;                                              \
    } while (0)

    f32x16 acc[4][2];
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int c = 0; c < 2; c++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[a][c][r] = 0.f;

    const int frag_kg = (lane >> 5) * CS_REGION;
    const int a_off = frag_kg + (wm * 128 + (lane & 31)) * 16;                       // + a*32*16 + p*2*REGION
    const int b_off = 6 * CS_REGION + frag_kg + (wn * 64 + (lane & 31)) * 16;        // + c*32*16 + p*2*REGION

    // Three LDS chunk buffers: chunk kc+2 is loaded at the top of chunk kc and split / written to LDS in
    // the MIDDLE of chunk kc's MFMA stream (its buffer was last read in chunk kc-1), so the staging tail
    // no longer sits between the last MFMA and the barrier with the matrix pipe idle.
    CS_LOAD_GLOBAL(0);
    CS_STORE_LDS(0);
    if (nk > 1) {
        CS_LOAD_GLOBAL(1);
        CS_STORE_LDS(1);
    }
    __syncthreads();
    int buf = 0;
    for (int kc = 0; kc < nk; kc++) {
        const bool more = kc + 2 < nk;
        const int wbuf = buf == 0 ? 2 : buf - 1;                  // (kc + 2) % 3
        if (more) CS_LOAD_GLOBAL(kc + 2);
        const unsigned char *base = lds + buf * CS_BUF;
        // operand reads one W plane at a time (l, m, h): the 8 + 16 + 24 MFMAs of a plane run while the
        // next plane's four fragments are still in flight, instead of all 18 reads landing first with
        // every wave of the workgroup -- and the matrix pipe -- waiting (measured: 1.1 k of 4.6 k cycles/chunk)
        bf16x8 Bf[2][3];
#pragma unroll
        for (int p = 0; p < 3; p++)
#pragma unroll
            for (int c = 0; c < 2; c++) Bf[c][p] = *(const bf16x8 *)(base + b_off + c * 512 + p * 2 * CS_REGION);
#pragma unroll
        for (int pa = 2; pa >= 0; pa--) {
            bf16x8 A[4];
#pragma unroll
            for (int a = 0; a < 4; a++) A[a] = *(const bf16x8 *)(base + a_off + a * 512 + pa * 2 * CS_REGION);
#pragma unroll
            for (int pb = 2; pb >= 0; pb--) {
                if (pa + pb > 2) continue;
#pragma unroll
                for (int a = 0; a < 4; a++)
#pragma unroll
                    for (int c = 0; c < 2; c++)
                        acc[a][c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[a], Bf[c][pb], acc[a][c], 0, 0, 0);
            }
            if (pa == 1) {                  // after the l and m planes (24 of 48 MFMAs): stage chunk kc+2 ...
                __builtin_amdgcn_sched_barrier(0);
                if (more) CS_STORE_LDS(wbuf);
            }
            if (pa == 0) {                  // ... its split VALU / LDS stores issued between the h plane's 24 MFMAs
#pragma unroll
                for (int i = 0; i < 24; i++) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
                    if (i % 4 == 3) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        __syncthreads();
        buf = buf == 2 ? 0 : buf + 1;
    }
#undef CS_LOAD_GLOBAL
#undef CS_STORE_LDS

    // ---- epilogue: D[co = 32a + (r&3) + 8(r>>2) + 4(lane>>5)][n = 32c + (lane&31)]
    if (pool) {
        // max over every `pool` (8 / 16 / 32 / 64) consecutive points: y [B][Cout][N / pool]  (as mlp.hip's POOL epilogue)
        const int Np = N / pool;
        float *yp = y + (size_t)b * Cout * Np;
        const int span = pool < 32 ? pool : 32;
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int co = co0 + wm * 128 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                const float sc = scale ? scale[co] : 1.f;
                const float sh = shift ? shift[(size_t)b * shift_bstride + co] : 0.f;
                float v0 = acc[a][0][r] * sc + sh, v1 = acc[a][1][r] * sc + sh;
                if (relu) { v0 = l3d_act(v0, relu); v1 = l3d_act(v1, relu); }
                if (pool == 64) v0 = fmaxf(v0, v1);
                v0 = l3d_group_max(v0, span);
                v1 = l3d_group_max(v1, span);
                if (((lane & 31) & (span - 1)) == 0) {
                    const int nb = n0 + wn * 64 + (lane & 31);
                    yp[(size_t)co * Np + nb / pool] = v0;
                    if (pool != 64) yp[(size_t)co * Np + (nb + 32) / pool] = v1;
                }
            }
        return;
    }
    float *yb = y + (size_t)b * Cout * N;
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int co = co0 + wm * 128 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            const float sc = scale ? scale[co] : 1.f;
            const float sh = shift ? shift[(size_t)b * shift_bstride + co] : 0.f;
#pragma unroll
            for (int c = 0; c < 2; c++) {
                float v = acc[a][c][r] * sc + sh;
                if (relu) v = l3d_act(v, relu);
                yb[(size_t)co * N + n0 + wn * 64 + c * 32 + (lane & 31)] = v;
            }
        }
}

// ---------------------------------------------------------------------------------------------
// Second kernel shape: 256 (co) x 128 (n) tile, 256 threads (4 waves, 2 x 2, wave tile 128 x 64 as
// above), 72 KB of LDS -> TWO workgroups per CU.  The two workgroups run out of phase, so one's
// barrier / staging / epilogue bubbles are filled by the other's MFMAs (with one 512-thread workgroup
// per CU both waves of a SIMD hit the same barrier together).  W goes global -> LDS directly
// (global_load_lds_dwordx4: wave-uniform LDS base + lane x 16 B, which is exactly the [kg][row][16 B]
// region order), so the doubled per-thread W share costs no staging registers.
// ---------------------------------------------------------------------------------------------
#define CD_TM 256
#define CD_TN 128
#define CD_WREG (256 * 16)
#define CD_XREG (128 * 16 + 64)
#define CD_BUF (6 * CD_WREG + 6 * CD_XREG)
#define CD_LDS (2 * CD_BUF)

typedef __attribute__((address_space(3))) void *lds_ptr_t;
typedef const __attribute__((address_space(1))) void *gbl_ptr_t;

template <int XMODE>
__global__ __launch_bounds__(256, 2) void conv_split_dma_kernel(const void *__restrict__ xin,
                                                                const uint4 *__restrict__ wsplit,
                                                                const float *__restrict__ scale,
                                                                const float *__restrict__ shift, int shift_bstride,
                                                                int Bn, int Cin, int Cout, int N, int relu,
                                                                float *__restrict__ y)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int n0 = blockIdx.x * CD_TN, co0 = blockIdx.y * CD_TM, b = blockIdx.z;
    const int nk = Cin / CS_TK;
    const size_t BN = (size_t)Bn * N;

    // W: wave w copies rows 64w .. 64w+63 of each of the 6 (plane, kg) regions
    const uint4 *wsrc = wsplit + co0 + wave * 64 + lane;               // + ((kc*3 + p)*2 + kg) * Cout
    const int w_lds = wave * 64 * 16;                                  // + (p*2 + kg) * CD_WREG   (wave-uniform)
    // pre-split X (XMODE 2): 12 half-regions of 64 rows, 3 per wave
    // fp32 X: thread -> (row, kg) octet
    const int xrow = (XMODE == 1) ? (t >> 1) : (t & 127);
    const int xkg = (XMODE == 1) ? (t & 1) : (t >> 7);
    const float *xsrc1 = (const float *)xin + ((size_t)b * N + n0 + xrow) * Cin + xkg * 8;
    const float *xsrc0 = (const float *)xin + ((size_t)b * Cin + xkg * 8) * N + n0 + xrow;
    const int x_lds = 6 * CD_WREG + xkg * CD_XREG + xrow * 16;         // + p * 2 * CD_XREG

    // fp32 x comes from HBM (W from L2): its loads are issued TWO chunks ahead into two alternating
    // register sets (the K loop is unrolled by two so the sets have static names).
    f32x4 xa0, xb0, xa1, xb1;

#define CD_ISSUE_W(KC, BUF)                                                                           \
    do {                                                                                              \
        unsigned char *base_ = lds + (BUF) * CD_BUF;                                                  \
        _Pragma("unroll") for (int r_ = 0; r_ < 6; r_++)                                              \
            __builtin_amdgcn_global_load_lds((gbl_ptr_t)(wsrc + ((size_t)(KC) * 6 + r_) * Cout),    \
                                             (lds_ptr_t)(base_ + w_lds + r_ * CD_WREG), 16, 0, 0);    \
        if (XMODE == 2) {                                                                             \
            _Pragma("unroll") for (int i_ = 0; i_ < 3; i_++) {                                        \
                const int it_ = wave * 3 + i_, reg_ = it_ >> 1, half_ = it_ & 1;                      \
                __builtin_amdgcn_global_load_lds(                                                     \
                    (gbl_ptr_t)((const uint4 *)xin + ((size_t)(KC) * 6 + reg_) * BN + (size_t)b * N + n0 + half_ * 64 + lane), \
                    (lds_ptr_t)(base_ + 6 * CD_WREG + reg_ * CD_XREG + half_ * 64 * 16), 16, 0, 0);   \
            }                                                                                         \
        }                                                                                             \
    } while (0)

#define CD_LOAD_X(KC, XA, XB)                                                                         \
    do {                                                                                              \
        if (XMODE == 1) {                                                                             \
            XA = *(const f32x4 *)(xsrc1 + (KC) * CS_TK);                                              \
            XB = *(const f32x4 *)(xsrc1 + (KC) * CS_TK + 4);                                          \
        } else if (XMODE == 0) {                                                                      \
            const float *q_ = xsrc0 + (size_t)(KC) * CS_TK * N;                                       \
            XA[0] = q_[0]; XA[1] = q_[(size_t)N]; XA[2] = q_[(size_t)2 * N]; XA[3] = q_[(size_t)3 * N];                   \
            XB[0] = q_[(size_t)4 * N]; XB[1] = q_[(size_t)5 * N]; XB[2] = q_[(size_t)6 * N]; XB[3] = q_[(size_t)7 * N];   \
        }                                                                                             \
    } while (0)

#define CD_STORE_X(BUF, XA, XB)                                                                       \
    do {                                                                                              \
        if (XMODE != 2) {                                                                             \
            unsigned char *base_ = lds + (BUF) * CD_BUF;                                              \
            uint4 x0, x1, x2;                                                                         \
            split_pair(XA[0], XA[1], x0.x, x1.x, x2.x);                                               \
            split_pair(XA[2], XA[3], x0.y, x1.y, x2.y);                                               \
            split_pair(XB[0], XB[1], x0.z, x1.z, x2.z);                                               \
            split_pair(XB[2], XB[3], x0.w, x1.w, x2.w);                                               \
            *(uint4 *)(base_ + x_lds) = x0;                                                           \
            *(uint4 *)(base_ + x_lds + 2 * CD_XREG) = x1;                                             \
            *(uint4 *)(base_ + x_lds + 4 * CD_XREG) = x2;                                             \
        }                                                                                             \
    } while (0)

    f32x16 acc[4][2];
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int c = 0; c < 2; c++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[a][c][r] = 0.f;

    const int a_off = (lane >> 5) * CD_WREG + (wm * 128 + (lane & 31)) * 16;                  // + a*512 + p*2*CD_WREG
    const int b_off = 6 * CD_WREG + (lane >> 5) * CD_XREG + (wn * 64 + (lane & 31)) * 16;     // + c*512 + p*2*CD_XREG

    // one K chunk: W(kc+1) and x(kc+2) issued, chunk kc multiplied, x(kc+1) split into the other buffer
#define CD_CHUNK(KC, XCUR_A, XCUR_B, XNEXT_A, XNEXT_B)                                                \
    do {                                                                                              \
        const int buf = (KC) & 1;                                                                     \
        if (!(CS_PROBE & 1) && (KC) + 1 < nk) CD_ISSUE_W((KC) + 1, buf ^ 1);                          \
        if (!(CS_PROBE & 2) && (KC) + 2 < nk) CD_LOAD_X((KC) + 2, XCUR_A, XCUR_B);                    \
        const unsigned char *base = lds + buf * CD_BUF;                                               \
        bf16x8 A[4][3], Bf[2][3];                                                                     \
        _Pragma("unroll") for (int p = 0; p < 3; p++) {                                               \
            if ((CS_PROBE & 8) && (KC) > 0) break;                                                    \
            _Pragma("unroll") for (int a = 0; a < 4; a++)                                             \
                A[a][p] = *(const bf16x8 *)(base + a_off + a * 512 + p * 2 * CD_WREG);                \
            _Pragma("unroll") for (int c = 0; c < 2; c++)                                             \
                Bf[c][p] = *(const bf16x8 *)(base + b_off + c * 512 + p * 2 * CD_XREG);               \
        }                                                                                             \
        _Pragma("unroll") for (int a = 0; a < 4; a++)                                                 \
            _Pragma("unroll") for (int c = 0; c < 2; c++) {                                           \
                f32x16 d = acc[a][c];                                                                 \
                if (CS_PROBE & 4) {                                                                   \
                    asm volatile("" ::"v"(A[a][0]), "v"(A[a][1]), "v"(A[a][2]), "v"(Bf[c][0]), "v"(Bf[c][1]), "v"(Bf[c][2])); \
                    continue;                                                                         \
                }                                                                                     \
                d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[a][2], Bf[c][0], d, 0, 0, 0);           \
                d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[a][0], Bf[c][2], d, 0, 0, 0);           \
                d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[a][1], Bf[c][1], d, 0, 0, 0);           \
                d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[a][1], Bf[c][0], d, 0, 0, 0);           \
                d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[a][0], Bf[c][1], d, 0, 0, 0);           \
                d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[a][0], Bf[c][0], d, 0, 0, 0);           \
                acc[a][c] = d;                                                                        \
            }                                                                                         \
        if (!(CS_PROBE & 2) && (KC) + 1 < nk) CD_STORE_X(buf ^ 1, XNEXT_A, XNEXT_B);                  \
        if (!(CS_PROBE & 16)) __syncthreads();                                                        \
    } while (0)

    CD_ISSUE_W(0, 0);
    CD_LOAD_X(0, xa0, xb0);
    if (nk > 1) CD_LOAD_X(1, xa1, xb1);
    CD_STORE_X(0, xa0, xb0);
    __syncthreads();

    for (int kc = 0; kc < nk; kc += 2) {
        CD_CHUNK(kc, xa0, xb0, xa1, xb1);                 // x(kc+2) -> set 0 (x(kc) already in LDS); stores x(kc+1) from set 1
        if (kc + 1 < nk) CD_CHUNK(kc + 1, xa1, xb1, xa0, xb0);
    }
#undef CD_CHUNK
#undef CD_ISSUE_W
#undef CD_LOAD_X
#undef CD_STORE_X

    float *yb = y + (size_t)b * Cout * N;
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int co = co0 + wm * 128 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            const float sc = scale ? scale[co] : 1.f;
            const float sh = shift ? shift[(size_t)b * shift_bstride + co] : 0.f;
#pragma unroll
            for (int c = 0; c < 2; c++) {
                float v = acc[a][c][r] * sc + sh;
                if (relu) v = l3d_act(v, relu);
                yb[(size_t)co * N + n0 + wn * 64 + c * 32 + (lane & 31)] = v;
            }
        }
}

extern "C" size_t l3d_split_bytes(int rows, int cols)
{
    return (size_t)((cols + 15) / 16) * 3 * 2 * (size_t)rows * 16;
}

extern "C" int l3d_split_rows(const float *src, int rows, int cols, void *dst, l3d_stream_t stream)
{
    L3D_REQUIRE(src && dst && rows > 0 && cols > 0);
    const long total = (long)rows * ((cols + 15) / 16) * 2;
    hipLaunchKernelGGL(split_rows_kernel, dim3(l3d_divup(total, 256)), dim3(256), 0, (hipStream_t)stream, src,
                       rows, cols, (uint4 *)dst);
    return l3d_check_launch();
}

static int launch_conv_split(const void *x, int x_mode, const void *w_split, const float *scale, const float *shift,
                             int shift_bstride, int B, int Cin, int Cout, int N, int relu, int pool, float *y,
                             hipStream_t st)
{
    if (Cout % CS_TM || N % CD_TN || Cin % CS_TK || B > 65535 || ((((size_t)x) | ((size_t)w_split)) & 15)) return L3D_ERR_UNSUPPORTED;
    if (pool && N % CS_TN) return L3D_ERR_UNSUPPORTED;          // the pooled epilogue lives in the 256x256 kernel only
    // Both shapes run conv5 in ~170 us (tools/probe_conv_split.hip ablations: the 256x128 shape moves
    // 1.6x the bytes per FLOP through the CU's vector-memory path, which cancels what its two
    // out-of-phase workgroups gain); the 256x256 shape is the default, the 256x128 one takes
    // N % 256 == 128.
#ifndef CS_USE_DMA
#define CS_USE_DMA 0
#endif
    if (!pool && (CS_USE_DMA || N % CS_TN)) {
        dim3 grid2(N / CD_TN, Cout / CD_TM, B), block2(256);
        if (x_mode == 0)
            hipLaunchKernelGGL(conv_split_dma_kernel<0>, grid2, block2, CD_LDS, st, x, (const uint4 *)w_split, scale,
                               shift, shift_bstride, B, Cin, Cout, N, relu, y);
        else if (x_mode == 1)
            hipLaunchKernelGGL(conv_split_dma_kernel<1>, grid2, block2, CD_LDS, st, x, (const uint4 *)w_split, scale,
                               shift, shift_bstride, B, Cin, Cout, N, relu, y);
        else
            hipLaunchKernelGGL(conv_split_dma_kernel<2>, grid2, block2, CD_LDS, st, x, (const uint4 *)w_split, scale,
                               shift, shift_bstride, B, Cin, Cout, N, relu, y);
        return l3d_check_launch();
    }
    dim3 grid(N / CS_TN, Cout / CS_TM, B), block(512);
    if (x_mode == 0)
        hipLaunchKernelGGL(conv_split_kernel<0>, grid, block, CS_LDS, st, x, (const uint4 *)w_split, scale, shift,
                           shift_bstride, B, Cin, Cout, N, relu, y, pool);
    else if (x_mode == 1)
        hipLaunchKernelGGL(conv_split_kernel<1>, grid, block, CS_LDS, st, x, (const uint4 *)w_split, scale, shift,
                           shift_bstride, B, Cin, Cout, N, relu, y, pool);
    else
        hipLaunchKernelGGL(conv_split_kernel<2>, grid, block, CS_LDS, st, x, (const uint4 *)w_split, scale, shift,
                           shift_bstride, B, Cin, Cout, N, relu, y, pool);
    return l3d_check_launch();
}

// pool = 0: y [B,Cout,N]; pool = 8, 16, 32, 64: the max over every `pool` consecutive points in the epilogue, y [B,Cout,N/pool]
extern "C" int l3d_pointwise_conv_split(const void *x, int x_mode, const void *w_split, const float *scale,
                                        const float *shift, int shift_bstride, int B, int Cin, int Cout,
                                        int N, int relu, int pool, float *y, l3d_stream_t stream)
{
    L3D_REQUIRE(x && w_split && y && B > 0 && Cin > 0 && Cout > 0 && N > 0 && x_mode >= 0 && x_mode <= 2 && pool >= 0);
    if (pool && pool != 8 && pool != 16 && pool != 32 && pool != 64) return L3D_ERR_UNSUPPORTED;
    return launch_conv_split(x, x_mode, w_split, scale, shift, shift_bstride, B, Cin, Cout, N, relu, pool, y, (hipStream_t)stream);
}
