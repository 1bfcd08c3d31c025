// edgeconv_f16b.hip -- the TWO-PLANE, PERSISTENT f16x2 EdgeConv kernel (the default of the benchmark step); derived from
// edgeconv_f16.hip (the three-plane kernel of round 2, kept unchanged as the fallback for parameter blocks whose plane
// exponents cannot be chained, see edgeconv_layout.h "fifth copy").  Entry point l3d_edgeconv_forward_f16b.  What follows is
// that file's description; the differences are listed under "EF_V2" below.
//
// the register-chained EdgeConv stack of edgeconv_split.hip with layers 2-4 as "f16x2":
// every fp32 operand is carried as an fp16 HIGH part and a 2^12-SCALED fp16 residual, and one fp32 product costs
// THREE fp16 MFMA products (half of bf16x3's six) at fp32-level accuracy.  models/dgcnn.py:32-46.
//
// Arithmetic (the error-corrected fp16 split of Ootomo & Yokota, IJHPCA 2022, adapted to the MFMA):
//   activation x (fp32):  h = f16(x),  m' = f16((x - h) * 2^12)            -> x = h + m' 2^-12 up to 2^-22 |x| (worst case of two 11-bit roundings)
//   weight     w (fp32):  W = w 2^S (S per layer, static, so that max|W| is in [4,8)),
//                         H = f16(W),  M = f16(W - H),  Hs = f16(H 2^-12)  -> W = H + M up to 2^-22 |W|
//   one accumulator:      acc = b 2^S + sum_k ( M h  +  Hs m'  +  H h )     = 2^S (b + w.x) up to the dropped
//                         M m' 2^-12 term (2^-24 relative), every fp16 x fp16 product exact in the fp32 accumulator;
//   epilogue:             y = max(acc, 0) 2^-S  (a power of two: exact).
// Scaling the residual keeps it a NORMAL fp16 number whenever x is one (an unscaled residual of x < 0.25 is
// subnormal and loses the bits it exists to carry); scaling the weights does the same for M.  CPU emulation
// (K = 64..512, activations scaled 1e-3 .. 1e2): max error 0.5-1.1x, rms 0.7-1.2x of the fp32-MFMA kernel's own error
// against fp64 (bf16x3: 0.7-1.1x / 0.7-0.9x); tests/test_gpu_parity.py holds this kernel to the same <= 2x / 1.5x bar.
// Range: fp16 tops out at 65504.  Activations are post-ReLU, so the max-pooled outputs the kernel writes anyway ARE
// the largest activations: each wave tracks their maximum and raises *range_flag if a layer-1..3 output exceeds
// 60000 (results are then invalid; the host falls back to edgeconv_split.hip, whose bf16 planes have fp32's range).
//
// The split is 4 VALU instructions per value pair instead of bf16x3's 10: v_fma_mixlo/hi_f16 convert WITH the
// power-of-two scale, v_fma_mix_f32 forms the residual straight from the packed fp16 halves.
//
// Chaining with v_mfma_f32_16x16x32_f16 is that of edgeconv_split.hip: every layer transposed,
// D[ch][row] = sum_k W'[ch][k] act[row][k], weights = A operand, activations = B operand, one wave
// owns MT row tiles of 16 rows (4 points x 4*MT neighbours); lane (j = row, g) register r holds channel
// 16m + 4g + r of M-tile m; the B operand of k-step s is the pair of previous-layer accumulators (2s, 2s+1) of the
// same lane after ReLU and the split: no LDS, no barriers, no cross-lane traffic.  The A operand is pre-split and
// pre-permuted on the host (l3d_edgeconv_pack, fourth block) and streamed as 1 KB fragments.
//
// EF_V2 (always set in this file): the TWO-PLANE variant.
//   * the residual is carried unscaled, m = f16(x - h): with the planes placed so that typical activations sit near 2^11
//     (the packer's T_l), a subnormal residual costs 2^-25 ABSOLUTE in plane units -- below fp32's own rounding of any
//     activation that matters to the sum -- so the Hs = H 2^-12 weight plane is not needed: products M h + H m + H h,
//     two weight fragments per step instead of three (a third fewer global_load issues beside the MFMA stream);
//   * accumulators of layers 1-3 come out in plane units (edgeconv_layout.h, fifth copy), so the split needs no scale
//     and no v_fma_mix: v_cvt_pk_f16_f32 (gfx950) rounds the pair to h, two v_cvt_f32_f16 + two v_sub_f32 form the exact
//     residuals, a second v_cvt_pk_f16_f32 rounds them to m -- six full-rate VALU instructions where the three-plane
//     kernel issues six v_fma_mix* (measured ~2.4x the issue cost of a plain VALU beside the MFMA stream, LABLOG R2.2).
//
// The finish schedule (LABLOG R28.1; tools/ef_gap_model.py prints the model below from the compiled code).  With one wave per SIMD a
// 16x16x32 MFMA holds the vector issue for 8 of its 16 cycles and every other vector, LDS or VMEM instruction or s_nop costs >= 4:
// an MFMA gap runs ~ max(16, 8 + 4 c) cycles for c such fillers, two are nearly free, each further one costs its issue.  Layers
// 2-3 have 60 MFMAs per M-tile pair to hide a ~170-instruction finish behind (every gap overfull), layer 4 has 120 for ~40 (most
// gaps empty).  So:
//   * no wait state that an independent instruction can stand in for: the split interleaves two value pairs, the quad reduce of
//     both M-tiles is two asm blocks with the selects in front of the DPP maxima, a unit is ONE asm block (see "Wait states");
//   * units are spread over a pair's MFMAs by their instruction count; a layer's first pair runs the deferred pool and
//     quad-reduce units behind the MFMAs of k-step S-1, which only the plane-making units had to precede;
//   * PLANES: what happens to a pooled value of layers 1-3 after the quad reduce (range guard, scale, h / m split, staging
//     stores) is done inside layer 4, two instructions per otherwise empty gap (EfOut, ef_unpark).  PLANES = false keeps its
//     multiply and 4-byte store where they were: two instructions per value, nothing to stage.
// The arithmetic, the order of accumulation and every output expression are those of the kernel before: same output bits.
#include <type_traits>
#include "common.h"
#include "edgeconv_layout.h"
#include "split_bf16.h"      // f32x2 / f32x4 typedefs

#define EF_V2 1
// Layer 4's weight fragments (128 KB as two planes) are copied to LDS once per workgroup and read from there by every tile -- a
// ds_read_b128 beside the MFMA stream costs about half of a global_load_dwordx4 (LABLOG R2.2: +19 vs +43 cycles per 5 MFMAs) and
// layer 4 issues 128 of them per tile.
#define EF_W4_BYTES ((EC_C4 / 16) * (EC_C3 / 32) * 2 * 1024)
// LDS of a workgroup (dynamic, 159 808 of the CU's 163 840 bytes):
//   [0, EF_PAR_BYTES)  the packed block's tail, copied once: layer 4's fragments (128 KB) | b2 | b3 | b4 | W1 | b1 | scales
//                      (contiguous in the fifth copy, edgeconv_layout.h) -- every bias and layer 1's weights are read from
//                      here with ds_read, so that NO parameter of layers 1 and 4 travels through vmcnt (a global load's
//                      s_waitcnt also waits for every store issued before it: vmcnt is one in-order counter)
//   EF_STG_A           per wave 4 KB: the pooled planes of layers 1-3 of the current tile, [plane 2][cell row 32][point 4][8 f16]
//   EF_STG_B           per wave 2 x 1 KB: the pooled planes of two layer-4 pairs each, [slot 2][plane 2][cell row 4][point 4][8 f16]
// The staged values leave as 16-byte stores from inside layer 4 (64 two-byte stores per wave and tile before).
#define EF_PAR_FLOATS (EC5_OFF_SC + 16 - EC5_OFF_W4)
#define EF_PAR_BYTES (EF_PAR_FLOATS * 4)
#define EF_LOFF_B2 (EF_W4_BYTES)
#define EF_LOFF_B3 (EF_LOFF_B2 + 4 * EC_C2)
#define EF_LOFF_B4 (EF_LOFF_B3 + 4 * EC_C3)
#define EF_LOFF_W1 (EF_LOFF_B4 + 4 * EC_C4)
#define EF_LOFF_B1 (EF_LOFF_W1 + 4 * 8 * EC_C1)
#define EF_STG_A (EF_PAR_BYTES)
#define EF_STG_B (EF_STG_A + 4 * 4096)
#define EF_LDS_BYTES (EF_STG_B + 4 * 2048)
static_assert(EC5_OFF_B2 == EC5_OFF_W4 + EF_W4_BYTES / 4 && EC5_OFF_B1 == EC5_OFF_W1 + 8 * EC_C1 && EC5_OFF_SC == EC5_OFF_B1 + EC_C1,
              "the fifth copy's tail is one contiguous run");
static_assert(EF_PAR_BYTES % 16 == 0 && EF_LDS_BYTES <= 163840, "LDS budget");
#define EF_NPL 2
#define EFO_W2 EC5_OFF_W2
#define EFO_W3 EC5_OFF_W3
#define EFO_W4 EC5_OFF_W4
#define EFO_B2 EC5_OFF_B2
#define EFO_B3 EC5_OFF_B3
#define EFO_B4 EC5_OFF_B4
#define EFO_SC EC5_OFF_SC
#define EFO_W1 EC5_OFF_W1
#define EFO_B1 EC5_OFF_B1
#define EF_KERNEL edgeconv_f16b_kernel
#define EF_ENTRY l3d_edgeconv_forward_f16b

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
struct EfBase { const char *p; };     // the packed parameter block
typedef __attribute__((address_space(3))) const char *ef_lds_t;
typedef __attribute__((address_space(3))) const float *ef_ldsf_t;     // parameters that live in LDS (biases, layer 1's weights)
typedef __attribute__((address_space(3))) char *ef_ldsw_t;            // the pooled-output staging areas
typedef EfBase ef_rsrc_t;

// ---------------------------------------------------------------------------------------------
// Register homes.  With __launch_bounds__(256, 1) hipcc selects the AGPR form of every MFMA builtin: accumulators
// live in AGPRs and each value the finish work touches costs a v_accvgpr_read first -- measured at ~15 cycles apiece
// beside the MFMA stream (4.7 k of layer 4's 22 k cycles went on moving accumulators, tools/probe_ef.hip).  The dense
// layers therefore issue their MFMAs as volatile inline asm with the homes fixed by constraints:
//     accumulators  VGPRs ("+v")  -- the finish VALU reads and writes them in place, no copies;
//     B operands    AGPRs ("a")   -- the split activation planes are only ever MFMA operands (<= 240 registers);
//     A operands    AGPRs ("a")   -- weight fragments arrive by global_load, which writes AGPRs directly.
// Volatile asm statements keep their program order, so the interleave of finish work and MFMAs below is the issue
// order; the compiler still places the fragment loads, address arithmetic and s_waitcnt (asm operands are uses).
// What it no longer does is pad MFMA hazards: every read of an accumulator by VALU code is >= 5 MFMAs after the
// MFMA that wrote it (see the unit order), and the two places where that does not hold by construction carry s_nop.
// ---------------------------------------------------------------------------------------------
#define EF_ACON "a"          // weight fragments (MFMA A operand) live in AGPRs: global_load writes them directly
__device__ __forceinline__ void ef_mfma_init(f32x4 &d, const u32x4 &a, const f16x8 &b, const f32x4 &c)
{
    asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %3" : "=&v"(d) : EF_ACON(a), "a"(b), "v"(c));
}
__device__ __forceinline__ void ef_mfma_acc(f32x4 &d, const u32x4 &a, const f16x8 &b)
{
    asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(d) : EF_ACON(a), "a"(b));
}
// a freshly split 16-byte fragment -> an AGPR tuple, once, at its creation
__device__ __forceinline__ f16x8 ef_home_agpr(u32x4 v)
{
    f16x8 r = __builtin_bit_cast(f16x8, v);
    asm("" : "+a"(r));
    return r;
}

// VALU written out (volatile: issue position = program position)
__device__ __forceinline__ float ef_vmax(float a, float b)
{
    float r;
    asm volatile("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// Wait states.  Nothing pads a hazard inside inline asm, and the compiler's hazard recogniser counts an asm statement as ZERO
// wait states: wherever one asm statement reads a register that an earlier one wrote, with only asm statements in between (MFMAs
// included), it places an `s_nop 0` in front of the reader -- a full issue slot beside the MFMA stream.  So each finish unit below
// is ONE asm block, ordered so that every hazard inside it is covered by independent instructions of the same block:
//   * VALU write -> DPP read of that VGPR needs 2 wait states: every DPP source is written >= 3 instructions before it is read;
//   * v_cvt_pk / v_fma_mixlo results are read >= 2 instructions after they are written (two value pairs interleaved).
// What is left to the compiler is one s_nop where a block reads what another block wrote.

// max over the MT row tiles of one accumulator register
template <int MT>
__device__ __forceinline__ float ef_pool_rows(float a0, float a1, float a2, float a3, float a4)
{
    float r;
    if constexpr (MT == 3) asm volatile("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a0), "v"(a1), "v"(a2));
    if constexpr (MT == 4) asm volatile("v_max3_f32 %0, %1, %2, %3\n\tv_max_f32 %0, %0, %4" : "=&v"(r) : "v"(a0), "v"(a1), "v"(a2), "v"(a3));
    if constexpr (MT == 5)
        asm volatile("v_max3_f32 %0, %1, %2, %3\n\tv_max3_f32 %0, %0, %4, %5" : "=&v"(r) : "v"(a0), "v"(a1), "v"(a2), "v"(a3), "v"(a4));
    return r;
}

// Transposing quad reduce, step 1, of BOTH M-tiles of a pair: per M-tile the four row maxima (a 0..3 / b 0..3) -> two values per
// lane, x[.][0] = max(give[lane ^ 1], keep) of registers (0, 2), x[.][1] of registers (1, 3); odd = the lanes with q & 1 set.
// The eight selects stand in front of the four DPP maxima.
__device__ __forceinline__ void ef_quad_step1(const f32x4 &a, const f32x4 &b, uint64_t odd, f32x2 &xa, f32x2 &xb)
{
    float k0, g0, k1, g1, k2, g2, k3, g3, r0, r1, r2, r3;
    asm volatile("v_cndmask_b32 %[k0], %[a0], %[a2], %[odd]\n\t"
                 "v_cndmask_b32 %[g0], %[a2], %[a0], %[odd]\n\t"
                 "v_cndmask_b32 %[k1], %[a1], %[a3], %[odd]\n\t"
                 "v_cndmask_b32 %[g1], %[a3], %[a1], %[odd]\n\t"
                 "v_cndmask_b32 %[k2], %[b0], %[b2], %[odd]\n\t"
                 "v_cndmask_b32 %[g2], %[b2], %[b0], %[odd]\n\t"
                 "v_cndmask_b32 %[k3], %[b1], %[b3], %[odd]\n\t"
                 "v_cndmask_b32 %[g3], %[b3], %[b1], %[odd]\n\t"
                 "v_max_f32_dpp %[r0], %[g0], %[k0] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
                 "v_max_f32_dpp %[r1], %[g1], %[k1] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
                 "v_max_f32_dpp %[r2], %[g2], %[k2] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
                 "v_max_f32_dpp %[r3], %[g3], %[k3] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf"
                 : [k0] "=&v"(k0), [g0] "=&v"(g0), [k1] "=&v"(k1), [g1] "=&v"(g1), [k2] "=&v"(k2), [g2] "=&v"(g2), [k3] "=&v"(k3),
                   [g3] "=&v"(g3), [r0] "=&v"(r0), [r1] "=&v"(r1), [r2] "=&v"(r2), [r3] "=&v"(r3)
                 : [a0] "v"(a[0]), [a1] "v"(a[1]), [a2] "v"(a[2]), [a3] "v"(a[3]), [b0] "v"(b[0]), [b1] "v"(b[1]), [b2] "v"(b[2]),
                   [b3] "v"(b[3]), [odd] "s"(odd));
    xa[0] = r0; xa[1] = r1; xb[0] = r2; xb[1] = r3;
}

// Step 2 of both M-tiles: v = max(give[lane ^ 2], keep); hi = the lanes with q & 2 set.  Between the two DPP maxima stands the
// first value's own follow-up (which is what keeps the second one's sources two wait states old):
//   LAST:      v = max(v, 0)                          (the other layers' values were ReLU'd before pooling)
//   otherwise: ovf = max(ovf, v * split)              (in plane units: what the next layer's fp16 planes hold)
template <bool LAST>
__device__ __forceinline__ void ef_quad_step2(const f32x2 &xa, const f32x2 &xb, uint64_t hi, float split, float &va, float &vb, float &ovf)
{
    float k0, g0, k1, g1, t0, t1;
    if constexpr (LAST) {
        (void)split; (void)t0; (void)t1; (void)ovf;
        asm volatile("v_cndmask_b32 %[k0], %[a0], %[a1], %[hi]\n\t"
                     "v_cndmask_b32 %[g0], %[a1], %[a0], %[hi]\n\t"
                     "v_cndmask_b32 %[k1], %[b0], %[b1], %[hi]\n\t"
                     "v_cndmask_b32 %[g1], %[b1], %[b0], %[hi]\n\t"
                     "v_max_f32_dpp %[va], %[g0], %[k0] quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
                     "v_max_f32_e64 %[va], %[va], 0\n\t"
                     "v_max_f32_dpp %[vb], %[g1], %[k1] quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
                     "v_max_f32_e64 %[vb], %[vb], 0"
                     : [k0] "=&v"(k0), [g0] "=&v"(g0), [k1] "=&v"(k1), [g1] "=&v"(g1), [va] "=&v"(va), [vb] "=&v"(vb)
                     : [a0] "v"(xa[0]), [a1] "v"(xa[1]), [b0] "v"(xb[0]), [b1] "v"(xb[1]), [hi] "s"(hi));
    } else {
        asm volatile("v_cndmask_b32 %[k0], %[a0], %[a1], %[hi]\n\t"
                     "v_cndmask_b32 %[g0], %[a1], %[a0], %[hi]\n\t"
                     "v_cndmask_b32 %[k1], %[b0], %[b1], %[hi]\n\t"
                     "v_cndmask_b32 %[g1], %[b1], %[b0], %[hi]\n\t"
                     "v_max_f32_dpp %[va], %[g0], %[k0] quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
                     "v_mul_f32 %[t0], %[va], %[sp]\n\t"
                     "v_max_f32_dpp %[vb], %[g1], %[k1] quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
                     "v_mul_f32 %[t1], %[vb], %[sp]\n\t"
                     "v_max_f32 %[ovf], %[ovf], %[t0]\n\t"
                     "v_max_f32 %[ovf], %[ovf], %[t1]"
                     : [k0] "=&v"(k0), [g0] "=&v"(g0), [k1] "=&v"(k1), [g1] "=&v"(g1), [va] "=&v"(va), [vb] "=&v"(vb), [t0] "=&v"(t0),
                       [t1] "=&v"(t1), [ovf] "+v"(ovf)
                     : [a0] "v"(xa[0]), [a1] "v"(xa[1]), [b0] "v"(xb[0]), [b1] "v"(xb[1]), [hi] "s"(hi), [sp] "v"(split));
    }
}

// relu'd accumulators (already in plane units) of TWO value pairs -> packed fp16 (h, m) words: v_cvt_pk_f16_f32 rounds a pair to
// h, v_fma_mixlo/hi_f16 form a * 1.0 - f32(h half) in fp32 (exact: a - h is representable) and round it to the fp16 half of m in the
// same instruction -- the same bits as convert, subtract, convert.  The two pairs alternate, so every result is read two
// instructions after it is written (one wait state between, as the hand-placed s_nop gave it before).
__device__ __forceinline__ void ef_split_2pairs(float a0, float a1, float b0, float b1, uint32_t &ha, uint32_t &ma, uint32_t &hb, uint32_t &mb)
{
    asm volatile("v_cvt_pk_f16_f32 %0, %4, %5\n\t"
                 "v_cvt_pk_f16_f32 %2, %6, %7\n\t"
                 "v_fma_mixlo_f16 %1, %4, 1.0, -%0 op_sel_hi:[0,0,1]\n\t"
                 "v_fma_mixlo_f16 %3, %6, 1.0, -%2 op_sel_hi:[0,0,1]\n\t"
                 "v_fma_mixhi_f16 %1, %5, 1.0, -%0 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
                 "v_fma_mixhi_f16 %3, %7, 1.0, -%2 op_sel:[0,0,1] op_sel_hi:[0,0,1]"
                 : "=&v"(ha), "=&v"(ma), "=&v"(hb), "=&v"(mb)
                 : "v"(a0), "v"(a1), "v"(b0), "v"(b1));
}

// Lane-constant context of the pooled stores.  q = lane & 3 (neighbour slot inside the quad); after the transposing
// quad reduce lane q holds channel register {0,2,1,3}[q] of its point, and stores it to pooled[point][ch0 + 4g + that].
struct EfLane {
    uint64_t odd, hi;        // the lanes with q & 1 / q & 2 set, as lane masks (a scalar register pair: the selects read them as such)
    unsigned laneoff;        // lane * 16: byte offset of the lane's 16 bytes inside a 1 KB fragment
    ef_rsrc_t rs;            // the packed parameter block
    ef_lds_t w4lds;          // layer 4's fragment block in LDS
    float *prow;             // out_mode 0: pooled + (b N + point) CTOT + 4 g + {0,2,1,3}[q]
    ef_ldsw_t stgA, stgB;    // out_mode 1, 2: this lane's 2-byte cell of its wave's staging areas (channel cl within an M-tile, its point)
    float mres;              // scale of the pooled planes' residual: 4096 (out_mode 1: m' = (v - h) 2^12) or 1 (out_mode 2: unscaled)
    size_t bn;               // B N: channel ch0 + 16 k lies (ch0 + 16 k) * bn halfs further, the m' plane 512 * bn beyond that
};

// Power-of-two scales of one layer's accumulators (edgeconv_layout.h): to its split planes, to the pooled output
struct EfScale {
    float split, pool;
};

// What a lane carries out of the finish units.  PLANES: the pooled values of layers 1-3 -- after the quad reduce ONE value per
// lane and M-tile, 16 per tile -- are PARKED here (AGPRs) by layers 1-3 and go through the rest of their way out (range guard,
// scale, h / m split, staging stores) in layer 4's empty MFMA gaps (ef_unpark): nothing but the image store waits for them,
// and in layers 1-3 every issue slot past two per gap costs its full price.
struct EfOut {
    float ovf;               // range guard: the largest value (plane units) handed to fp16 planes
    float park[(EC_C1 + EC_C2 + EC_C3) / 16];
    float last[2];           // PLANES: the two pooled values of the layer-4 pair whose finish is under way, on the same way out (ef_pair)
};

// One parked value's way out, as five STAGES of two instructions.  Successive stages of a value are issued a whole execution
// step (3 MT MFMAs) apart, so the step's fragment reads -- compiler-visible instructions -- stand between the asm statement that
// writes a register and the one that reads it: no s_nop from the compiler, no hazard.
struct EfStage {
    float v, t;              // v = pooled value times sc.pool; t: (float)h, then the residual
    uint32_t h, m;           // fp16 h and m (low halves)
};
// PARKED: the value comes from an AGPR (layers 1-3; staging area A, m plane 2048 bytes behind h) or from a VGPR (layer 4; area
// B, 256 bytes).
template <int G, bool PARKED>
__device__ __forceinline__ void ef_unpark(EfStage &s, float parked, float pool, float mres, float &ovf, ef_ldsw_t cell)
{
    typedef __attribute__((address_space(3))) _Float16 *lh_t;
    if constexpr (G == 0 && PARKED) asm volatile("v_accvgpr_read_b32 %0, %1\n\tv_mul_f32 %0, %2, %0" : "=&v"(s.v) : "a"(parked), "s"(pool));
    if constexpr (G == 0 && !PARKED) asm volatile("v_mul_f32 %0, %2, %1" : "=v"(s.v) : "v"(parked), "s"(pool));
    if constexpr (G == 1) asm volatile("v_max_f32 %0, %0, %2\n\tv_cvt_f16_f32 %1, %2" : "+v"(ovf), "=&v"(s.h) : "v"(s.v));
    if constexpr (G == 2) asm volatile("v_cvt_f32_f16 %0, %1\n\tv_sub_f32 %0, %2, %0" : "=&v"(s.t) : "v"(s.h), "v"(s.v));
    if constexpr (G == 3) asm volatile("v_mul_f32 %0, %2, %1\n\tv_cvt_f16_f32 %0, %0" : "=&v"(s.m) : "v"(s.t), "s"(mres));
    if constexpr (G == 4) {
        *(lh_t)cell = __builtin_bit_cast(_Float16, (uint16_t)s.h);
        *(lh_t)(cell + (PARKED ? 2048 : 256)) = __builtin_bit_cast(_Float16, (uint16_t)s.m);
    }
}

// Scratch values that live from one micro-unit to the next
struct EfTmp {
    f32x4 mx[2];             // max over the row tiles, per M-tile
    u32x4 qh, qm;            // the 16-byte h / m' fragments being assembled for one row tile
    f32x2 xs[2];             // quad reduce, after its first step
};

// ---------------------------------------------------------------------------------------------
// The finish work of a completed M-tile pair (ReLU, two-plane split, max-pool) as MICRO-UNITS of 2-12 VALU instructions,
// issued between the MFMAs of the next pair (with one wave per SIMD nothing else hides VALU work):
//   not LAST:  per row tile t: 2 x [relu half of h0[t]] 2 x [of h1[t]] [split value pairs 0, 1] [pairs 2, 3 + the two fragments -> AGPRs]
//              then 8 x [pool one register of one M-tile], [quad reduce step 1, both M-tiles] [step 2 + store]   = 6 MT + 10
//   LAST:      the 8 pool and 2 quad units on the raw accumulators, ReLU on the one pooled value per lane        = 10
// ORDER is the MFMA -> VALU hazard cover: the first units touch M-tile 0 only (finished a whole step earlier);
// h1[t], written by the pair's MFMA MT - t from its end, is first read by unit 6 t + 2 resp. pool unit 4 -- at least five MFMAs
// later wherever the units are spread over the next pair's MFMAs by EfN::first (unit 6 t + 2 never rides before slot t + 1).
// The quad reduce is a transposing butterfly: 4 registers x 4 lanes -> ONE value per lane in 3 DPP max (+6 selects),
// and every lane stores its dword -- no `if (writer)` exec-mask branch.
// RAW = false: the accumulators come from MFMA builtins and the first reader of each is a compiler-visible instruction, so
// the compiler pads the hazard (no caller at present: layer 1 issues its MFMAs as asm too).
// ---------------------------------------------------------------------------------------------
template <int MT, bool LAST> struct EfN {
    static constexpr int NT = LAST ? 0 : 6 * MT;             // units before the pool units
    static constexpr int UNITS = NT + 10;
    // issue slots of a unit, roughly (a split unit's AGPR homes and the output path behind the quad reduce are the compiler's to
    // place: counted with their unit)
    static constexpr int weight(int u) { return u < NT ? (u % 6 < 4 ? 2 : 8) : u < NT + 8 ? 2 : u == NT + 8 ? 12 : LAST ? 20 : 12; }
    // Units [u0, u1) spread over n MFMA slots BY WEIGHT (unit u rides behind slot cum(u) n / W, cum = the weights in front of it):
    // the first unit that rides at or behind slot s; slot s takes [first(s), first(s + 1)).
    static constexpr int first(int u0, int u1, int n, int s)
    {
        int W = 0, cum = 0;
        for (int u = u0; u < u1; u++) W += weight(u);
        for (int u = u0; u < u1; u++) {
            if (cum * n / W >= s) return u;
            cum += weight(u);
        }
        return u1;
    }
};

template <int MT, bool LAST, bool RAW, bool PLANES, int U>
__device__ __forceinline__ void ef_micro(f32x4 (&h)[2][MT], f16x8 (&pl)[2][MT], EfTmp &T, int ch0, const EfLane &L, const EfScale &sc, EfOut &O)
{
    constexpr int NT = EfN<MT, LAST>::NT;
    if constexpr (U < NT) {
        constexpr int t = U / 6, k = U % 6;
        if constexpr (k < 4) {                               // relu of M-tile k / 2, row tile t, two registers
#pragma unroll
            for (int r = 2 * (k & 1); r < 2 * (k & 1) + 2; r++) h[k >> 1][t][r] = RAW ? ef_vmax(h[k >> 1][t][r], 0.f) : fmaxf(h[k >> 1][t][r], 0.f);
        } else {                                             // split the four values of M-tile k-4, row tile t: words 2 (k-4), 2 (k-4) + 1 of the fragment
            constexpr int m = k - 4;
            uint32_t ha, ma, hb, mb;
            ef_split_2pairs(h[m][t][0], h[m][t][1], h[m][t][2], h[m][t][3], ha, ma, hb, mb);
            T.qh[2 * m] = ha;
            T.qm[2 * m] = ma;
            T.qh[2 * m + 1] = hb;
            T.qm[2 * m + 1] = mb;
            if constexpr (m == 1) {                          // whole 16-byte fragments, homed in AGPRs: the type the MFMA reads
                pl[0][t] = ef_home_agpr(T.qh);
                pl[1][t] = ef_home_agpr(T.qm);
            }
        }
    } else if constexpr (U < NT + 8) {                       // max over the row tiles (= 4 MT neighbours), one register
        constexpr int k = (U - NT) / 4, r = (U - NT) % 4;
        static_assert(MT >= 3 && MT <= 5, "row tiles per wave");
        if constexpr (RAW) {
            T.mx[k][r] = ef_pool_rows<MT>(h[k][0][r], h[k][1][r], h[k][2][r], h[k][MT > 3 ? 3 : 0][r], h[k][MT > 4 ? 4 : 0][r]);
        } else {
            float m = h[k][0][r];
#pragma unroll
            for (int t = 1; t < MT; t++) m = fmaxf(m, h[k][t][r]);
            T.mx[k][r] = m;
        }
    } else if constexpr (U == NT + 8) {                      // transposing quad reduce of both M-tiles, step 1
        ef_quad_step1(T.mx[0], T.mx[1], L.odd, T.xs[0], T.xs[1]);
    } else {                                                 // step 2, ReLU (LAST), range guard, scale, store
        float vk[2];
        ef_quad_step2<LAST>(T.xs[0], T.xs[1], L.hi, sc.split, vk[0], vk[1], O.ovf);
#pragma unroll
        for (int k = 0; k < 2; k++) {
            if constexpr (PLANES && !LAST) {                 // layers 1-3: parked; the way out is ef_unpark's, inside layer 4
                float p = vk[k];                             // (ch0 is a literal at every call site: the index folds to a constant)
                asm("" : "+a"(p));
                O.park[(ch0 >> 4) + k] = p;
            } else if constexpr (PLANES) {                   // layer 4: the way out is ef_last_stage's, behind later MFMAs of the same pair
                O.last[k] = vk[k];
            } else {
                L.prow[ch0 + 16 * k] = vk[k] * sc.pool;
            }
        }
    }
}

// Compile-time loops: every register-array index in this file must be a constant, and `#pragma unroll`
// is only a request (bodies this large exceed the unroller's pragma threshold, the loop stays rolled,
// the index becomes dynamic and the accumulators / planes land in scratch memory).
template <int I0, int I1, class F>
__device__ __forceinline__ void ef_static_for(F &&f)
{
    if constexpr (I0 < I1) {
        f(std::integral_constant<int, I0>{});
        ef_static_for<I0 + 1, I1>(f);
    }
}

// Stage G of the way out of O.last[k], the pooled value of M-tile k of the layer-4 pair at channel ch0 (pair m: area B, chunk
// (m >> 1) & 1, slot m & 1, cell rows 2 k (+ 1)).
template <int G>
__device__ __forceinline__ void ef_last_stage(EfStage &s, EfOut &O, int k, int ch0, const EfLane &L, const EfScale &sc)
{
    const int m = (ch0 - (EC_C1 + EC_C2 + EC_C3)) >> 5;
    ef_unpark<G, false>(s, O.last[k], sc.pool, L.mres, O.ovf, L.stgB + ((m >> 1) & 1) * 1024 + (m & 1) * 512 + (2 * k) * 64);
}

template <int MT, bool LAST, bool RAW, bool PLANES>
__device__ __forceinline__ void ef_finish_all(f32x4 (&h)[2][MT], f16x8 (&pl)[2][MT], int ch0, const EfLane &L, const EfScale &sc, EfOut &O)
{
    EfTmp T;
    ef_static_for<0, EfN<MT, LAST>::UNITS>([&](auto u) { ef_micro<MT, LAST, RAW, PLANES, decltype(u)::value>(h, pl, T, ch0, L, sc, O); });
    if constexpr (LAST && PLANES) {
        EfStage s[2];
        ef_static_for<0, 5>([&](auto g) {
            ef_last_stage<decltype(g)::value>(s[0], O, 0, ch0, L, sc);
            ef_last_stage<decltype(g)::value>(s[1], O, 1, ch0, L, sc);
        });
    }
}

// EF_PIN: the compiler's IR passes sink a load towards its first use (two steps later) regardless of
// sched_barrier, which collapses the prefetch distance; a memory clobber right after the issue pins it
// (the fragment pointer is deliberately NOT __restrict__, or the clobber would not order the load).
#define EF_PIN() asm volatile("" ::: "memory")

// Weight fragments are prefetched EF_PD execution steps ahead into a ring of registers that is handed from pair to
// pair and from layer to layer.  A step is only 3 x MT MFMAs (~250 cycles): two steps ahead (what the bf16x3 kernel,
// with 6 x MT MFMAs per step, gets away with) is less than an L2 hit under load and stalled every step.
#ifndef EF_PD
#define EF_PD 4
#endif
struct EfRing {
    u32x4 a[EF_PD][EF_NPL];  // fragments (H, Hs, M planes; EF_V2: H, M) of the next EF_PD steps
    f32x4 bv[2];             // bias (pre-scaled) of the current pair's two M-tiles
};
struct EfNext {              // where the pair executed after this one finds its fragments / bias
    int woff;                // byte offset of the layer's fragment block inside the packed parameters
    ef_ldsf_t bias;          // layer's scaled bias + 4 g (LDS)
    int mp;                  // pair index inside that layer
    int steps;               // 2 S of that layer
};

// fragment `frag` (1 KB each) of the layer block at byte offset `byte_off` of the packed parameters.
// Measured alternatives for the addressing (tools/probe_ef.hip, layer 4): plain pointers as here 19.9 k cycles (the
// compiler spends ~50 VALU per 240 MFMAs on 64-bit address arithmetic); a buffer descriptor with scalar offsets
// (no VALU at all) 20.9 k -- the cost beside the MFMAs is the issue of the load itself (one global_load_dwordx4 per
// 5 MFMAs costs the stream ~40 cycles, tools/probe_mfma_filler.hip), not its address.
__device__ __forceinline__ u32x4 ef_ldfrag(ef_rsrc_t rs, int byte_off, int frag, unsigned laneoff)
{
    return *(const u32x4 *)(rs.p + (size_t)byte_off + (size_t)frag * 1024 + laneoff);
}

__device__ __forceinline__ u32x4 ef_ldfrag_lds(ef_lds_t base, int frag, unsigned laneoff)
{
    return *(__attribute__((address_space(3))) const u32x4 *)(base + frag * 1024 + laneoff);
}

__device__ __forceinline__ void ef_ring_fill(EfRing &R, ef_rsrc_t rs, int woff, ef_ldsf_t bias4g, int mp, int steps, int lane)
{
#pragma unroll
    for (int d = 0; d < EF_PD; d++)
#pragma unroll
        for (int p = 0; p < EF_NPL; p++) R.a[d][p] = ef_ldfrag(rs, woff, (mp * steps + d) * EF_NPL + p, (unsigned)lane * 16u);
    R.bv[0] = *(__attribute__((address_space(3))) const f32x4 *)(bias4g + 32 * mp);
    R.bv[1] = *(__attribute__((address_space(3))) const f32x4 *)(bias4g + 32 * mp + 16);
}

// One output M-tile pair of a dense layer: 2 x S steps (k-step outer, M-tile inner -- the order the
// fragments are packed in) of {prefetch fragment step+EF_PD, 3 products x MT MFMAs}, with the micro-units of the finish
// of a PREVIOUS pair (hp) spread BY THEIR WEIGHT (EfN::first) behind the MFMAs.  That previous pair is the preceding pair of
// this layer (NSL = every MFMA slot) or, for a layer's first pair, the LAST pair of the previous layer, whose planes are this
// layer's k-step S-1: the units that make those planes (ReLU, split, AGPR homes) then ride on the MFMAs of k-steps 0 .. S-2
// only and are complete (plus an s_nop for the accvgpr-write -> MFMA-read hazard) before the first MFMA that reads them,
// and its pool and quad-reduce units, which no MFMA waits for, ride on the MFMAs of k-step S-1.
// mp = this pair; nx = the pair executed after it, in this layer or the first of the next (fragment and bias
// prefetches cross both boundaries); pairs may be executed in any order.  R.bv: this pair's bias (the MFMA C operand of
// each M-tile's first product); replaced by the next pair's on return.  c_prev: 2^-S of hp's layer.
struct EfNoHook { template <class... I> __device__ __forceinline__ void operator()(I...) const {} };

// extra(slot): further work that rides behind MFMA slot `slot` of this pair (layer 4: the parked values' way out).
template <int MT, int S, bool PREV_LAST, bool PREV_RAW, bool PLANES, int NSL, bool OWN_LDS = false, bool NX_LDS = false, class EXTRA = EfNoHook>
__device__ __forceinline__ void ef_pair(int mp, const EfNext &nx, const f16x8 (&pin)[S][2][MT], const f16x8 (&pin_last)[2][MT],
                                        int woff, EfRing &R,
                                        f32x4 (&acc)[2][MT], f32x4 (&hp)[2][MT], f16x8 (&po_prev)[2][MT],
                                        int ch_prev, const EfLane &L, const EfScale &c_prev, EfOut &O, EXTRA &&extra = EfNoHook())
{
    static_assert(2 * S >= EF_PD, "a pair is at least EF_PD steps long");
    typedef EfN<MT, PREV_LAST> E;
    constexpr int NU = E::UNITS, NS = 2 * S * 3 * MT;                // micro-units to hide; MFMA slots of the pair
    // deferred finish (NSL < NS): only the units that make the planes must be complete before k-step S-1; the pool and quad units,
    // which no MFMA waits for, ride on the MFMAs of k-step S-1
    constexpr int NA = NSL < NS ? E::NT : NU;
    // the finish of a layer-4 pair with PLANES: its units ride on the first steps, the two pooled values then take their way out
    // one stage per step over the last five (behind slots 5 and 10 of the step)
    constexpr bool WAYOUT = PREV_LAST && PLANES;
    constexpr int NSU = WAYOUT ? (2 * S - 5) * 3 * MT : NSL;          // slots that carry units
    static_assert(!WAYOUT || (2 * S > 5 && NSL == NS), "five steps for the way out");
    EfStage TS[2];
    static_assert(NSL == NS || !PREV_LAST, "a deferred finish is the finish of a layer that has planes");
    EfTmp T;
    ef_static_for<0, 2 * S>([&](auto rc) {
        // execution step r = 2 s + mm; fragment EF_PD steps ahead: inside this pair, or the first steps of the next
        constexpr int r = decltype(rc)::value, s = r >> 1, mm = r & 1;
        u32x4 an[EF_NPL];
        if constexpr (r + EF_PD < 2 * S) {
#pragma unroll
            for (int p = 0; p < EF_NPL; p++)
                an[p] = OWN_LDS ? ef_ldfrag_lds(L.w4lds, (mp * 2 * S + r + EF_PD) * EF_NPL + p, L.laneoff)
                                : ef_ldfrag(L.rs, woff, (mp * 2 * S + r + EF_PD) * EF_NPL + p, L.laneoff);
        } else {
#pragma unroll
            for (int p = 0; p < EF_NPL; p++)
                an[p] = NX_LDS ? ef_ldfrag_lds(L.w4lds, (nx.mp * nx.steps + (r + EF_PD - 2 * S)) * EF_NPL + p, L.laneoff)
                               : ef_ldfrag(L.rs, nx.woff, (nx.mp * nx.steps + (r + EF_PD - 2 * S)) * EF_NPL + p, L.laneoff);
        }
        EF_PIN();
        if constexpr (s == S - 1 && mm == 0 && NSL < 2 * S * 3 * MT)
            asm volatile("s_nop 7");                                  // pin_last was written by v_accvgpr_write just now
        // three products, smallest first (M h, Hs m', H h); MT independent accumulators between dependent MFMAs
        ef_static_for<0, 3>([&](auto pc) {
            constexpr int prod = decltype(pc)::value;
            constexpr int pa = prod == 0 ? 1 : 0;                                     // W plane: M  H  H   (packed H, M)
            constexpr int pb = prod == 1 ? 1 : 0;                                     // x plane: h  m' h
            ef_static_for<0, MT>([&](auto tc) {
                constexpr int t = decltype(tc)::value;
                const f16x8 &bop = s == S - 1 ? pin_last[pb][t] : pin[s][pb][t];
                if constexpr (s == 0 && prod == 0) ef_mfma_init(acc[mm][t], R.a[0][pa], bop, R.bv[mm]);
                else ef_mfma_acc(acc[mm][t], R.a[0][pa], bop);
                constexpr int slot = (r * 3 + prod) * MT + t;
                constexpr int ub = slot < NSU ? E::first(0, NA, NSU, slot) : WAYOUT ? NU : E::first(NA, NU, NS - NSL, slot - NSL);
                constexpr int ue = slot < NSU ? E::first(0, NA, NSU, slot + 1) : WAYOUT ? NU : E::first(NA, NU, NS - NSL, slot + 1 - NSL);
                ef_static_for<ub, ue>([&](auto u) {
                    ef_micro<MT, PREV_LAST, PREV_RAW, PLANES, decltype(u)::value>(hp, po_prev, T, ch_prev, L, c_prev, O);
                });
                if constexpr (WAYOUT && slot >= NSU && (slot % (3 * MT) == 5 || slot % (3 * MT) == 10))
                    ef_last_stage<(slot - NSU) / (3 * MT)>(TS[slot % (3 * MT) == 10], O, slot % (3 * MT) == 10, ch_prev, L, c_prev);
                extra(std::integral_constant<int, slot>{});
            });
        });
        if constexpr (r == 1) {                                       // both M-tiles have consumed their bias: fetch the next pair's
            R.bv[0] = *(__attribute__((address_space(3))) const f32x4 *)(nx.bias + 32 * nx.mp);
            R.bv[1] = *(__attribute__((address_space(3))) const f32x4 *)(nx.bias + 32 * nx.mp + 16);
            EF_PIN();
        }
#pragma unroll
        for (int p = 0; p < EF_NPL; p++) {
#pragma unroll
            for (int d = 0; d + 1 < EF_PD; d++) R.a[d][p] = R.a[d + 1][p];
            R.a[EF_PD - 1][p] = an[p];
        }
    });
}

// One dense layer: S input k-steps (32 channels each, planes in pin), NPAIR output M-tile pairs,
// software-pipelined over pairs (accumulators double-buffered: pair i's MFMAs hide pair i-1's finish).
// On entry accB holds the previous layer's last, unfinished pair (its planes are pin[S-1], its pooled
// output goes to channel ch_in) and R the fragments / bias of this layer's first pair; on return accB holds THIS
// layer's last unfinished pair (pair index *mp_out) and R what `after` (the next layer's first pair) needs.
// wl: [step = (pair*S + s)*2 + mm][plane][lane] fragments.  rot (only for the rolled LAST layer, where no register
// array is indexed by the pair): this workgroup starts at pair `rot`.
// IN_RAW: accB on entry was produced by asm MFMAs (layers >= 2) rather than builtins (layer 1).
// c_in / c_own: 2^-S of the previous layer (whose last pair is finished here) and of this layer; bias is pre-scaled.

template <int MT, int S, int NPAIR, bool LAST, bool UNROLL, bool IN_RAW, bool PLANES, class HOOK = EfNoHook, bool OWN_LDS = false, bool AFTER_LDS = false,
          class EXTRA = EfNoHook>
__device__ __forceinline__ void ef_layer(const f16x8 (&pin)[S][2][MT], f16x8 (&pout)[LAST ? 1 : NPAIR][2][MT],
                                         int woff, ef_ldsf_t bias4g, const EfNext &after, EfRing &R, int ch_own,
                                         f32x4 (&accA)[2][MT], f32x4 (&accB)[2][MT], int ch_in,
                                         int *mp_out, const EfLane &L, int rot, const EfScale &c_in, const EfScale &c_own, EfOut &O,
                                         HOOK &&hook = EfNoHook(), EXTRA &&extra = EfNoHook())
{
    static_assert(NPAIR % 2 == 0 && S >= 2, "pairs are processed two at a time; deferred finish needs S >= 2");
    constexpr int NS = 2 * S * 3 * MT, NSD = (S - 1) * 6 * MT;      // MFMA slots of a pair; of its k-steps 0 .. S-2
    f16x8 last[2][MT];              // planes of k-step S-1: produced here by the deferred finish (pin[S-1] is never written)
    auto in_layer = [&](int mp) { return EfNext{woff, bias4g, mp, 2 * S}; };
    if constexpr (UNROLL) {
        // written out (NPAIR is 2 or 4): a `#pragma unroll` loop over this much code is not always
        // unrolled, and a rolled loop indexes pout dynamically, which sends the planes to scratch
        static_assert(NPAIR == 2 || NPAIR == 4, "unrolled layers have 2 or 4 output pairs");
        static_assert(!OWN_LDS, "only the rolled (last) layer keeps its weights in LDS");
        ef_pair<MT, S, false, IN_RAW, PLANES, NSD>(0, in_layer(1), pin, last, woff, R, accA, accB, last, ch_in, L, c_in, O);
        if constexpr (NPAIR > 2)
            ef_pair<MT, S, LAST, true, PLANES, NS>(1, in_layer(2), pin, last, woff, R, accB, accA, pout[0], ch_own, L, c_own, O);
        else
            ef_pair<MT, S, LAST, true, PLANES, NS, false, AFTER_LDS>(1, after, pin, last, woff, R, accB, accA, pout[0], ch_own, L, c_own, O);
        if constexpr (NPAIR == 4) {
            ef_pair<MT, S, LAST, true, PLANES, NS>(2, in_layer(3), pin, last, woff, R, accA, accB, pout[1], ch_own + 32, L, c_own, O);
            ef_pair<MT, S, LAST, true, PLANES, NS, false, AFTER_LDS>(3, after, pin, last, woff, R, accB, accA, pout[2], ch_own + 64, L, c_own, O);
        }
        *mp_out = NPAIR - 1;
    } else {
        // the last layer, written out over its NPAIR pairs too (no register array is indexed by the pair, so a loop would do --
        // but a rolled loop whose body differs per trip (hook) made the compiler merge its memory counters at every join:
        // `s_waitcnt vmcnt(0)` inside the MFMA stream, behind all stores in flight).  hook(i) runs in front of pair i.
        (void)rot;
        ef_pair<MT, S, false, IN_RAW, PLANES, NSD, OWN_LDS, OWN_LDS>(0, in_layer(1), pin, last, woff, R, accA, accB, last, ch_in, L, c_in, O);
        ef_static_for<1, NPAIR>([&](auto ic) {
            constexpr int i = decltype(ic)::value;
            hook(ic);
            constexpr bool more = i + 1 < NPAIR;
            const EfNext nx = more ? in_layer(i + 1) : after;
            auto ex = [&](auto sc) { extra(ic, sc); };                // extra(pair, slot)
            if constexpr (i & 1)
                ef_pair<MT, S, LAST, true, PLANES, NS, OWN_LDS, more ? OWN_LDS : AFTER_LDS, decltype(ex) &>(i, nx, pin, last, woff, R, accB, accA, pout[0],
                                                                                                           ch_own + 32 * (i - 1), L, c_own, O, ex);
            else
                ef_pair<MT, S, LAST, true, PLANES, NS, OWN_LDS, more ? OWN_LDS : AFTER_LDS, decltype(ex) &>(i, nx, pin, last, woff, R, accA, accB, pout[0],
                                                                                                           ch_own + 32 * (i - 1), L, c_own, O, ex);
        });
        *mp_out = NPAIR - 1;
    }
}

// PLANES = false: pooled [B*N][512] fp32 (channel-last).  PLANES = true: `pooled` is an fp16 activation image for
// conv_f16.hip -- h | m' planes [512/8][B*N][8] of the pooled values times 2^T_out, then 2^-T_out (written here too).
//
// EF_PERSIST (default): one workgroup per CU walks the tiles (16 points each) with stride gridDim.x, and the gather of the
// NEXT tile -- neighbour indices, then the coordinates they point to: two dependent trips to memory, ~4.9 k of a tile's
// ~40 k cycles when they stood at the head of every workgroup with nothing to hide behind (tools/probe_ef.hip) -- is issued
// from inside layer 4 of the current one (indices at its second pair, coordinates at its fourth) and consumed a tile later.
// The weight ring is handed across tiles like across layers: layer 4's last pair prefetches layer 2's first fragments.
// (the three-plane kernel, edgeconv_f16.hip, keeps one workgroup per tile: with its 36-register ring the prefetched gather spills)

// EF_GATHER1: what a lane needs of a tile before its first MFMA is ONE dword per row tile -- layer 1's B operand of k-step 0 is
// component g of the neighbour (g < 3) or the centre's x (g == 3), of k-step 1 the centre's y / z (g = 0 / 1) or zero -- so the lane
// selects the ADDRESS and issues one unconditional load.  (Loading the neighbour's three coordinates and selecting the value, as the
// first version did, was compiled into exec-masked branches per lane group with an `s_waitcnt vmcnt(0)` in each: five serialised
// memory round trips in the middle of layer 4's MFMA stream, behind every store in flight.)
template <int MT>
struct EfGather {                      // what a lane needs of a tile before its first MFMA
    int nb[MT];                        // neighbour indices of its MT rows (< N: the low dword of the int64)
    float c;                           // centre y (g == 0) / z (g >= 1)
    float b1[MT];                      // layer 1's B operand, k-step 0 (after the second trip)
    int b, nc;
};

template <int MT>
__device__ __forceinline__ void ef_gather_idx(EfGather<MT> &G, int tile, int tiles_per_cloud, int N, int k, const float *__restrict__ xyz,
                                              const int64_t *__restrict__ idx, int wave, int j, int g)
{
    const int b = tile / tiles_per_cloud, xb = tile - b * tiles_per_cloud;     // uniform: a tile lies inside one cloud
    const int n = (xb * 4 + wave) * 4 + (j >> 2);
    const int nc = min(n, N - 1);                                   // lanes past N recompute point N-1
    G.b = b;
    G.nc = nc;
    const float *cloud = xyz + (size_t)b * N * 3;                   // scalar base + 32-bit lane offsets
    G.c = cloud[nc * 3 + (g == 0 ? 1 : 2)];
    const int64_t *row = idx + (size_t)b * N * k;
#pragma unroll
    for (int t = 0; t < MT; t++) {
        const int jj = 4 * t + (j & 3);
        G.nb[t] = (int)row[nc * k + (jj < k ? jj : 0)];             // pad k up to 4*MT with a duplicate
    }
}

template <int MT>
__device__ __forceinline__ void ef_gather_xyz(EfGather<MT> &G, int N, const float *__restrict__ xyz, int g)
{
    const float *cloud = xyz + (size_t)G.b * N * 3;
    const int comp = g < 3 ? g : 0;
#pragma unroll
    for (int t = 0; t < MT; t++) {
        int r = g < 3 ? G.nb[t] : G.nc;
        asm("" : "+v"(r));                                          // one address, one load: keep the select off the loaded values
        G.b1[t] = cloud[r * 3 + comp];
    }
}

template <int MT, bool PLANES>
__global__ __launch_bounds__(256, 1) void EF_KERNEL(const float *__restrict__ xyz,
                                                              const int64_t *__restrict__ idx, int B, int N, int k,
                                                              const float *packed,
                                                              float *__restrict__ pooled,
                                                              int *__restrict__ range_flag, float mres)
{
#define EF_T(i)
    EF_T(0);
    constexpr int CTOT = EC_C1 + EC_C2 + EC_C3 + EC_C4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 15, g = lane >> 4;
    const int tiles_per_cloud = (N + 15) / 16, ntiles = B * tiles_per_cloud;
    // pooled stores: after the transposing quad reduce lane q = j & 3 holds channel register {0,2,1,3}[q] of its point;
    // lanes past N recompute point N-1 and store the same bits to the same place
    EfLane L;
    L.laneoff = (unsigned)lane * 16u;
    L.rs.p = (const char *)packed;
    L.odd = __ballot(j & 1);
    L.hi = __ballot(j & 2);
    const int cl = 4 * g + ((j & 1) * 2 + ((j >> 1) & 1));       // this lane's channel inside a 16-channel M-tile
    L.bn = (size_t)B * N;
    L.mres = mres;
    extern __shared__ __attribute__((aligned(16))) unsigned char ef_lds[];
    L.w4lds = (ef_lds_t)ef_lds;
    // this lane's 2-byte cell inside its wave's staging areas: cell row (cl >> 3), point j >> 2, channel cl & 7
    {
        const int cell = (cl >> 3) * 64 + (j >> 2) * 16 + (cl & 7) * 2;
        L.stgA = (ef_ldsw_t)ef_lds + EF_STG_A + wave * 4096 + cell;
        L.stgB = (ef_ldsw_t)ef_lds + EF_STG_B + wave * 2048 + cell;
    }
    typedef __attribute__((address_space(3))) const u32x4 *ef_ldsq_t;
    const ef_ldsq_t rdA = (ef_ldsq_t)((ef_lds_t)ef_lds + EF_STG_A + wave * 4096 + lane * 16);     // read-out: 16 bytes per lane, 1 KB per trip
    const ef_ldsq_t rdB = (ef_ldsq_t)((ef_lds_t)ef_lds + EF_STG_B + wave * 2048 + lane * 16);
    if (PLANES && blockIdx.x == 0 && threadIdx.x == 0)
        *(float *)((_Float16 *)pooled + 2 * 512 * L.bn) = packed[EFO_SC + 12];        // the image's 2^-T_out
    // power-of-two scales of the four layers' accumulators (uniform: scalar loads), see edgeconv_layout.h
    const int po = PLANES ? 8 : 4;
    const EfScale s1 = {packed[EFO_SC + 0], packed[EFO_SC + po + 0]}, s2 = {packed[EFO_SC + 1], packed[EFO_SC + po + 1]},
                  s3 = {packed[EFO_SC + 2], packed[EFO_SC + po + 2]}, s4 = {1.0f, packed[EFO_SC + po + 3]};
    EfOut O;
    O.ovf = 0.f;
    constexpr int w2 = EFO_W2 * 4, w3 = EFO_W3 * 4, w4 = EFO_W4 * 4;      // byte offsets inside the descriptor
    const ef_ldsf_t bs2 = (ef_ldsf_t)((ef_lds_t)ef_lds + EF_LOFF_B2) + 4 * g, bs3 = (ef_ldsf_t)((ef_lds_t)ef_lds + EF_LOFF_B3) + 4 * g,
                    bs4 = (ef_ldsf_t)((ef_lds_t)ef_lds + EF_LOFF_B4) + 4 * g;

    int tile = blockIdx.x;                                      // grid <= ntiles: every workgroup has a first tile
    // Prologue, once per workgroup: the first tile's neighbour indices are requested first, then the parameter tail (135 KB) as
    // LDS-DMA (as eight-load batches through registers behind `s_waitcnt vmcnt(0)` the copy took five memory round trips), the
    // coordinates the indices point to in between: their trip overlaps the copy.
    EfGather<MT> G;
    ef_gather_idx<MT>(G, tile, tiles_per_cloud, N, k, xyz, idx, wave, j, g);
    EF_PIN();
    ef_gather_xyz<MT>(G, N, xyz, g);                             // vmcnt is one in-order counter: behind the DMA block these would wait for all of it
    EF_PIN();
    {
        // LDS-DMA (global_load_lds_dwordx4: 64 lanes x 16 bytes -> 1 KB of LDS per instruction, no registers, no ds_write): wave w
        // moves chunks w, w + 4, ... -- 33 instructions per wave, all in flight behind the index loads; the 64-byte remainder by hand
        typedef const __attribute__((address_space(1))) void *gp_t;
        typedef __attribute__((address_space(3))) void *lp_t;
        constexpr int NCH = EF_PAR_BYTES / 1024;                 // full 1 KB chunks
        const char *src = (const char *)(packed + EFO_W4);
#pragma unroll
        for (int c = 0; c < (NCH + 3) / 4; c++) {
            const int ch = c * 4 + wave;
            if (ch < NCH) __builtin_amdgcn_global_load_lds((gp_t)(src + ch * 1024 + lane * 16), (lp_t)(ef_lds + ch * 1024), 16, 0, 0);
        }
        EF_PIN();
        constexpr int REM = EF_PAR_BYTES - NCH * 1024;           // 64 bytes: the scale constants' tail
        static_assert(REM % 16 == 0 && REM < 1024, "remainder in 16-byte pieces");
        if (threadIdx.x < REM / 16) ((uint4 *)(ef_lds + NCH * 1024))[threadIdx.x] = ((const uint4 *)(src + NCH * 1024))[threadIdx.x];
    }
    // the compiler does not wait for LDS-DMA in front of a barrier (waves 1-3 skip the remainder branch and with it the only
    // vmcnt(0) it emitted): every wave's own DMA pieces have landed, then the barrier publishes them
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                                            // the parameter tail is in LDS
    // layer 2's first fragments and bias
    EfRing R;
    ef_ring_fill(R, L.rs, EFO_W2 * 4, bs2, 0, 2 * (EC_C1 / 32), lane);
    EF_PIN();
    // the gathered values count as arrived on BOTH edges into the loop (here, and in front of layer 4's pair 7 for the next
    // tile): otherwise the loop header merges "loads pending" with "nothing pending" into an `s_waitcnt vmcnt(0)` at the top
    // of every tile, which also waits for the 16-byte stores the previous tile issued last
#pragma unroll
    for (int t = 0; t < MT; t++) asm volatile("" : "+v"(G.b1[t]));
    asm volatile("" : "+v"(G.c));

    for (; tile < ntiles; tile += gridDim.x) {
    const int b = G.b;
    L.prow = pooled + ((size_t)b * N + G.nc) * CTOT + cl;
    // read-out addresses of this tile: lane -> (row of the image = plane * 64 + cell row, point lane & 3); rows times B N * 16 bytes
    const int n_st = min(((tile - b * tiles_per_cloud) * 4 + wave) * 4 + (lane & 3), N - 1);
    char *const img_pt = (char *)pooled + ((size_t)b * N + n_st) * 16;
    const size_t row_bytes = L.bn * 16;
    float b1[MT][2];
#pragma unroll
    for (int t = 0; t < MT; t++) { b1[t][0] = G.b1[t]; b1[t][1] = g < 2 ? G.c : 0.f; }
    const int tile_next = tile + (int)gridDim.x;
    const bool has_next = tile_next < ntiles;                    // uniform

    // ---- layer 1 on the fp32 MFMA (as edgeconv2.hip): graph feature rows as B operands, k-step s,
    //      lane group g -> channel 4s + g of (neighbour xyz, centre xyz, 0, 0)          dgcnn.py:32
    EF_T(1);
    f16x8 p1[EC_C1 / 32][2][MT];
    f32x4 accA[2][MT], accB[2][MT];                    // accB: the pair whose finish is pending
    {
        typedef __attribute__((address_space(3))) const f32x2 *lw1_t;
        typedef __attribute__((address_space(3))) const f32x4 *lb1_t;
        const lw1_t w1 = (lw1_t)((ef_lds_t)ef_lds + EF_LOFF_W1);
        const ef_ldsf_t b1p = (ef_ldsf_t)((ef_lds_t)ef_lds + EF_LOFF_B1) + 4 * g;
        f32x2 a1[EC_C1 / 16];
        f32x4 bv1[EC_C1 / 16];
#pragma unroll
        for (int m = 0; m < EC_C1 / 16; m++) { a1[m] = w1[m * 64 + lane]; bv1[m] = *(lb1_t)(b1p + 16 * m); }
        // pair 0 -> accA, pair 1 -> accB; pair 0's finish (ReLU, split into p1[0], pooling: 6 MT + 10 micro-units) rides on pair 1's
        // MFMAs -- a v_mfma_f32_16x16x4_f32 holds the matrix pipe for 32 cycles -- instead of standing between the two pairs
        static_assert(EC_C1 == 64, "layer 1 is two M-tile pairs");
        auto mfma1 = [&](f32x4 &d, float a, float b, const f32x4 &c, bool first) {
            if (first) asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, %3" : "=&v"(d) : "v"(a), "v"(b), "v"(c));
            else asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, %0" : "+v"(d) : "v"(a), "v"(b));
        };
        // b1 comes from VALU selects and nothing pads a VALU write in front of an asm MFMA that reads it (the compiler had placed the
        // v_cndmask of b1[.][1] directly in front of the first k-step-1 MFMA: stale operand, 15 % of the pooled values wrong): the
        // operands are inputs of the s_nop, so they are computed before it
#pragma unroll
        for (int t = 0; t < MT; t++) asm volatile("" ::"v"(b1[t][0]), "v"(b1[t][1]));
        asm volatile("s_nop 3");
#pragma unroll
        for (int mm = 0; mm < 2; mm++)
#pragma unroll
            for (int s = 0; s < 2; s++)
#pragma unroll
                for (int t = 0; t < MT; t++) mfma1(accA[mm][t], a1[mm][s], b1[t][s], bv1[mm], s == 0);
        constexpr int NU1 = EfN<MT, false>::UNITS, NSL1 = 4 * MT;
        EfTmp T1;
        ef_static_for<0, NSL1>([&](auto sc) {
            constexpr int slot = decltype(sc)::value, mm = slot / (2 * MT), s = (slot / MT) % 2, t = slot % MT;
            mfma1(accB[mm][t], a1[2 + mm][s], b1[t][s], bv1[2 + mm], s == 0);
            ef_static_for<EfN<MT, false>::first(0, NU1, NSL1, slot), EfN<MT, false>::first(0, NU1, NSL1, slot + 1)>([&](auto u) {
                ef_micro<MT, false, true, PLANES, decltype(u)::value>(accA, p1[0], T1, 0, L, s1, O);
            });
        });
        // An MFMA reads its C operand over its passes, and nothing pads an asm MFMA: the bias registers must not be handed out as
        // VALU temporaries while the last init MFMAs are in flight (the compiler did exactly that with bv1[3], three instructions
        // behind the MFMA reading it: 15 % of the image wrong).  A use behind the last slot keeps all four alive until then.
#pragma unroll
        for (int m = 0; m < EC_C1 / 16; m++) asm volatile("" ::"v"(bv1[m]), "v"(a1[m]));
    }
    int mp_last;

    EF_T(2);
    // ---- layer 2: 64 -> 64   (its first pair hides the finish of layer 1's last pair, and so on down)
    f16x8 p2[EC_C2 / 32][2][MT];
    ef_layer<MT, EC_C1 / 32, EC_C2 / 32, false, true, true, PLANES>(
        p1, p2, w2, bs2, EfNext{w3, bs3, 0, 2 * (EC_C2 / 32)}, R, EC_C1, accA, accB,
        32 * (EC_C1 / 32 - 1), &mp_last, L, 0, s1, s2, O);
    EF_T(3);
    // ---- layer 3: 64 -> 128; its last pair prefetches layer 4's first fragments from LDS
    f16x8 p3[EC_C3 / 32][2][MT];
    ef_layer<MT, EC_C2 / 32, EC_C3 / 32, false, true, true, PLANES, EfNoHook, false, true>(
        p2, p3, w3, bs3, EfNext{w4, bs4, 0, 2 * (EC_C3 / 32)}, R, EC_C1 + EC_C2, accA, accB,
        EC_C1 + 32 * (EC_C2 / 32 - 1), &mp_last, L, 0, s2, s3, O);
    EF_T(4);
    // ---- layer 4: 128 -> 256, only max-pooled; its last pair prefetches layer 2's first fragments for the next tile.
    // In front of its pairs (hook): the staged pooled planes of this tile leave as 16-byte stores -- one ds_read_b128 per trip,
    // stored one pair later (area A: layers 1-3, staged by the parked values' way out behind pairs 1 and 2, read in front of
    // pairs 3 .. 6; area B: two layer-4 pairs per 1 KB chunk, chunk (m >> 1) & 1) -- and the next tile's gather goes out (indices before pair 2, the coordinates they
    // point to before pair 6), waited for before pair 7, where every count is known, instead of behind the loop's back edge.
    f16x8 dummy[1][2][MT];
    u32x4 X, XA;                                                 // 16 bytes on their way from LDS to the image: of area B, of area A
#define EF_ST16(ptr, val) (*(u32x4 *)(ptr) = (val))
    auto st_a = [&](int c) { EF_ST16(img_pt + (size_t)((c >> 1) * 64 + (c & 1) * 16 + (lane >> 2)) * row_bytes, XA); EF_PIN(); };
    auto st_b = [&](int m0) {                                    // chunk of pairs m0, m0 + 1: lane -> slot, plane, cell row, point
        const int row = ((lane >> 4) & 1) * 64 + (EC_C1 + EC_C2 + EC_C3) / 8 + 4 * (m0 + (lane >> 5)) + ((lane >> 2) & 3);
        EF_ST16(img_pt + (size_t)row * row_bytes, X);
        EF_PIN();
    };
    auto hook = [&](auto ic) {
        constexpr int i = decltype(ic)::value;
        if constexpr (PLANES) {
            if constexpr (i >= 4) st_a(i - 4);
            if constexpr (i == 6) st_b(0);
            if constexpr (i == 7) st_b(2);
            if constexpr (i >= 3 && i <= 6) XA = rdA[(i - 3) * 64];
            if constexpr (i == 5 || i == 7) X = rdB[0];
            if constexpr (i == 6) X = rdB[64];
            EF_PIN();
        }
        if (has_next) {
            if constexpr (i == 2) { ef_gather_idx<MT>(G, tile_next, tiles_per_cloud, N, k, xyz, idx, wave, j, g); EF_PIN(); }
            if constexpr (i == 6) { ef_gather_xyz<MT>(G, N, xyz, g); EF_PIN(); }
            if constexpr (i == 7) {
#pragma unroll
                for (int t = 0; t < MT; t++) asm volatile("" : "+v"(G.b1[t]));       // a use: the compiler's counted wait lands here
                asm volatile("" : "+v"(G.c));
            }
        }
    };
    // The parked values (layers 1-3: 16 per lane, complete once pair 0 has finished layer 3's last pair) take their way out behind
    // the MFMAs of pairs 1 and 2, 16 execution steps of 3 MT slots: values 2 e and 2 e + 1 run their five stages at steps e .. e + 4,
    // every stage in a gap of its own.
    EfStage stg[(EC_C1 + EC_C2 + EC_C3) / 16];
    auto unpark = [&](auto ic, auto sc) {
        constexpr int i = decltype(ic)::value, slot = decltype(sc)::value;
        if constexpr (PLANES && (i == 1 || i == 2)) {
            constexpr int step = (i - 1) * 2 * (EC_C3 / 32) + slot / (3 * MT), pos = slot % (3 * MT);
            // (stage, value parity) -> slot of the step: 1 2 3 4 6 | 7 8 9 11 0 -- below 3 MT for MT = 4 too, and not 5 or 10, where
            // the layer-4 pair's own two values ride (ef_pair); the last stage of the odd values shares slot 0 with the fragment reads
            static_assert(3 * MT >= 12, "ten stage slots and two of ef_pair's in a step");
            constexpr int pi = pos == 1 ? 0 : pos == 2 ? 1 : pos == 3 ? 2 : pos == 4 ? 3 : pos == 6 ? 4
                             : pos == 7 ? 5 : pos == 8 ? 6 : pos == 9 ? 7 : pos == 11 ? 8 : pos == 0 ? 9 : -1;
            if constexpr (pi >= 0) {
                constexpr int g = pi % 5, e = step - g, w = 2 * e + pi / 5;
                if constexpr (e >= 0 && e < (EC_C1 + EC_C2 + EC_C3) / 32)
                    ef_unpark<g, true>(stg[w], O.park[w], w < 4 ? s1.pool : w < 8 ? s2.pool : s3.pool, L.mres, O.ovf, L.stgA + 128 * w);
            }
        }
    };
    ef_layer<MT, EC_C3 / 32, EC_C4 / 32, true, false, true, PLANES, decltype(hook) &, true, false, decltype(unpark) &>(
        p3, dummy, w4, bs4, EfNext{w2, bs2, 0, 2 * (EC_C1 / 32)}, R, EC_C1 + EC_C2 + EC_C3, accA, accB,
        EC_C1 + EC_C2 + 32 * (EC_C3 / 32 - 1), &mp_last, L, 0, s3, s4, O, hook, unpark);
    if constexpr (PLANES) st_b(4);                              // pairs 4, 5 (read before pair 7)
    asm volatile("s_nop 15\n\ts_nop 15");                       // the last asm MFMAs must have written accB (no compiler padding)
    ef_finish_all<MT, true, true, PLANES>(accB, dummy[0], EC_C1 + EC_C2 + EC_C3 + 32 * mp_last, L, s4, O);
    if constexpr (PLANES) { X = rdB[64]; st_b(6); }             // pairs 6, 7
    EF_T(5);
    }
    // fp16 range guard: ovf = the largest value (in plane units) this lane handed to fp16 planes -- layers 1-3, and the
    // pooled planes when PLANES; activations are post-ReLU, so the pooled maxima are the maxima.  Not taken while the
    // activations stay within 16x of the magnitude the packer was told; the host re-runs on the bf16x3 kernel if it is.
    if (!(O.ovf <= 60000.f) && range_flag) *(volatile int *)range_flag = 1; // may live in mapped host memory: plain store
}

// workgroups to launch: one per CU (persistent), or one per tile
static int ef_grid(int ntiles)
{
    static thread_local int cus[16] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) dev = 0;
    if (cus[dev] == 0) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cus[dev] = n;
    }
    return ntiles < cus[dev] ? ntiles : cus[dev];
}

extern "C" int EF_ENTRY(const float *xyz, const int64_t *idx, int B, int N, int k,
                                        const float *packed, void *out, int out_mode, int *range_flag, l3d_stream_t stream)
{
    L3D_REQUIRE(xyz && idx && packed && out && B > 0 && N > 0 && k > 0 && out_mode >= 0 && out_mode <= 2);
    const float mres = out_mode == 2 ? 1.0f : 4096.0f;           // out_mode 2: the image's residual plane unscaled (l3d_pointwise_conv_f16 with L3D_CONV_F16_TWO_PLANE)
    if (k > 20 || B > 65535 || (((size_t)packed) & 15) || (((size_t)out) & 15)) return L3D_ERR_UNSUPPORTED;
    const long ntiles = (long)B * l3d_divup(N, 16);
    if (ntiles > 0x7fffffffL / 2) return L3D_ERR_UNSUPPORTED;
    dim3 grid(ef_grid((int)ntiles)), block(256);
    hipStream_t st = (hipStream_t)stream;
    float *o = (float *)out;
    const size_t lds = EF_LDS_BYTES;
    if (out_mode == 0) {
        if (k <= 16) hipLaunchKernelGGL((EF_KERNEL<4, false>), grid, block, lds, st, xyz, idx, B, N, k, packed, o, range_flag, mres);
        else              hipLaunchKernelGGL((EF_KERNEL<5, false>), grid, block, lds, st, xyz, idx, B, N, k, packed, o, range_flag, mres);
    } else {
        if (k <= 16) hipLaunchKernelGGL((EF_KERNEL<4, true>), grid, block, lds, st, xyz, idx, B, N, k, packed, o, range_flag, mres);
        else              hipLaunchKernelGGL((EF_KERNEL<5, true>), grid, block, lds, st, xyz, idx, B, N, k, packed, o, range_flag, mres);
    }
    return l3d_check_launch();
}
