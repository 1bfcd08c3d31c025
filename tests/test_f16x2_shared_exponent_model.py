"""CPU model of the f16x2 arithmetic with ONE exponent shared by many dot products, held to a per-output bar.

test_f16x2_arithmetic_model.py gives every dot product its own exponents; the kernels do not.  A weight image (conv_f16.hip
l3d_conv_f16_split_weights, l3d_split_f16_operand kind 1) used to take one exponent for the whole matrix, and activations take one per
tensor.  The weight residual M = f16(W - H) is never scaled, so a row whose weights sit far below the matrix's largest has a subnormal
M -- a fixed absolute error of 2^-25 in plane units -- and its outputs lose relative precision in proportion, while a global
max-error ratio (dominated by the large rows) stays below 1.

The bar, per output row c over its columns j (points), against fp64 and against an fp32 product of the same inputs:
  max_j |e_cj| <= 2 max_j |e32_cj| + 2^-24 max_j sum_k |w_ck x_kj|,     rms_j e_cj <= 1.5 rms_j e32_cj + 2^-24 max_j sum_k |w_ck x_kj|
Column (point) magnitudes may spread within the one activation exponent: the floor is the row's largest column, so a column far below
it is held to what an fp32 result of that row could resolve."""
import numpy as np
import pytest

F = np.float32


def _exp_of(mx, hi_exp):
    """hi_exp - e with mx = f 2^e, f in [0.5, 1) (frexp), 0 for a zero maximum; clamped to [-126, 126] like cf_clamp_exp"""
    e = np.frexp(mx)[1]
    return np.where(mx > 0, np.clip(hi_exp - e, -126, 126), 0)


def _planes(v, hi_exp, scaled, per_row):
    """v [R][K] fp32 -> (h, m, 2^-T [R][1]) of v 2^T with the maximum placed in [2^(hi_exp-1), 2^hi_exp): T per row, or one T for v"""
    mx = np.abs(v).max(axis=1, keepdims=True) if per_row else np.full((v.shape[0], 1), np.abs(v).max())
    T = _exp_of(mx.astype(np.float64), hi_exp)
    X = (v.astype(np.float64) * np.exp2(T)).astype(F)                           # a power of two: exact
    h = X.astype(np.float16)
    r = (X - h.astype(F)).astype(F)                                              # exact in fp32
    m = (r * F(4096.0)).astype(np.float16) if scaled else r.astype(np.float16)
    return h, m, np.exp2(-T.astype(np.float64))


def _gemm_f16x2(w, x, scaled, per_row_w):
    """y [C][J] = w [C][K] x [K][J]: weights with max |W| in [4, 8) (per row or per matrix, residual unscaled), activations with ONE
    exponent for the tensor and max |X| in [2^11, 2^12) (residual scaled by 2^12, or unscaled: the two-plane form); three fp16 products,
    each exact in fp32, summed in fp32 smallest first"""
    H, M, cw = _planes(w, 3, False, per_row_w)
    h, m, cx = _planes(x.T, 12, scaled, False)                                  # rows = points; one exponent for all of them
    f = lambda a: a.astype(F)
    Hs = (f(H) * F(2.0 ** -12)).astype(np.float16) if scaled else H
    acc = f(M) @ f(h).T
    acc = (acc + f(Hs) @ f(m).T).astype(F)
    acc = (acc + f(H) @ f(h).T).astype(F)
    return acc.astype(np.float64) * cw * cx[0, 0]


def _inputs(rng, C=192, K=512, J=96):
    """weight rows x 10^U(-5, 0) with the edges among them -- a row whose maximum is exactly a power of two, one a ulp below it, an
    all-zero row -- and post-ReLU activations whose columns (points) spread over 10^U(-7, 0)"""
    w = (rng.standard_normal((C, K)) / np.sqrt(K)) * 10.0 ** rng.uniform(-5, 0, (C, 1))
    w = w.astype(F)
    w[0] = 0.0
    for r, top in ((1, F(2.0 ** -9)), (2, np.nextafter(F(2.0 ** -9), F(0))), (3, F(4.0)), (4, np.nextafter(F(2.0 ** -20), F(0)))):
        w[r] = (w[r] / np.abs(w[r]).max() * F(0.5) * top).astype(F)
        w[r, 7] = top                                                            # the row's maximum, exactly
    x = np.maximum(rng.standard_normal((K, J)), 0) * 10.0 ** rng.uniform(-7, 0, (1, J))
    return w, x.astype(F)


def _worst_ratios(w, x, y):
    """per-row (max-error ratio, rms ratio) of y against fp64, each over the fp32 product's own error plus the floor; worst rows"""
    want = w.astype(np.float64) @ x.astype(np.float64)
    e32 = np.abs((w @ x).astype(np.float64) - want)                             # fp32 BLAS product: fp32 accumulation
    e = np.abs(y - want)
    floor = 2.0 ** -24 * (np.abs(w).astype(np.float64) @ np.abs(x).astype(np.float64)).max(axis=1)
    rmax = e.max(axis=1) / (2.0 * e32.max(axis=1) + floor + 1e-300)
    rrms = np.sqrt((e ** 2).mean(axis=1)) / (1.5 * np.sqrt((e32 ** 2).mean(axis=1)) + floor + 1e-300)
    return rmax, rrms


@pytest.mark.parametrize("scaled", [True, False], ids=["three-plane", "two-plane"])
def test_per_row_weight_exponent_meets_the_per_output_bar(scaled):
    """the form the kernels use: one weight exponent per output row, one activation exponent per tensor"""
    rng = np.random.default_rng(11 if scaled else 12)
    for _ in range(3):
        w, x = _inputs(rng)
        rmax, rrms = _worst_ratios(w, x, _gemm_f16x2(w, x, scaled, per_row_w=True))
        assert rmax.max() <= 1.0 and rrms.max() <= 1.0, (scaled, rmax.max(), int(rmax.argmax()), rrms.max())
        assert np.all(_gemm_f16x2(w, x, scaled, True)[0] == 0.0)                # the all-zero row stays exactly zero


@pytest.mark.xfail(strict=True, reason="one exponent for the whole weight matrix: rows 1e-4 .. 1e-5 of the largest keep ~2^-13 relative "
                                       "precision in the unscaled residual -- their outputs' error is 100x and more the fp32 product's")
@pytest.mark.parametrize("scaled", [True, False], ids=["three-plane", "two-plane"])
def test_matrix_wide_weight_exponent_fails_the_per_output_bar(scaled):
    """the form the weight images had before: documented, not skipped -- a global max-error ratio still passes, the per-row bar not"""
    rng = np.random.default_rng(11 if scaled else 12)
    w, x = _inputs(rng)
    rmax, rrms = _worst_ratios(w, x, _gemm_f16x2(w, x, scaled, per_row_w=False))
    assert rmax.max() <= 1.0 and rrms.max() <= 1.0, (scaled, rmax.max(), rrms.max())


@pytest.mark.parametrize("scaled", [True, False], ids=["three-plane", "two-plane"])
def test_matrix_wide_weight_exponent_passes_a_global_bar(scaled):
    """... while the global bar the GPU tests held before, max error <= 2x the fp32 product's over the whole output, does not see it"""
    rng = np.random.default_rng(11 if scaled else 12)
    w, x = _inputs(rng)
    y = _gemm_f16x2(w, x, scaled, per_row_w=False)
    want = w.astype(np.float64) @ x.astype(np.float64)
    e32 = np.abs((w @ x).astype(np.float64) - want)
    assert np.abs(y - want).max() <= 2.0 * e32.max()
    assert _worst_ratios(w, x, y)[0].max() > 100.0                              # the per-row bar misses by two orders of magnitude and more


def test_exponents_of_tiny_maxima_stay_finite():
    """cf_scale_exp / cf_act_exp: 3 - e and 12 - e exceed 127 for a maximum below ~2^-124 (1e-36, fp32 subnormals) -- 2^S would be inf
    and every plane NaN; clamped to 126 the planes are finite and the split still represents the values"""
    for mx in (F(1e-36), F(1e-40), F(2.0 ** -149)):
        for hi in (3, 12):
            T = int(_exp_of(np.float64(mx), hi))
            assert -126 <= T <= 126 and np.isfinite(np.exp2(float(T))) and np.exp2(-float(T)) > 0
            v = np.array([[mx, mx * F(0.5), 0]], F)
            h, m, c = _planes(v, hi, True, True)
            back = (h.astype(np.float64) + m.astype(np.float64) * 2.0 ** -12) * c
            assert np.all(np.isfinite(back)) and np.allclose(back, v.astype(np.float64), rtol=2.0 ** -20, atol=0)
