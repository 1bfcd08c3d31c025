"""Both routes of every kernel that chooses between 16-byte and scalar accesses to a caller's tensor.

Many entry points decide at launch time, from the alignment of the caller's pointers and from sizes / strides modulo 4, whether a
lane moves 16 bytes or 4; others refuse a misaligned pointer (L3D_ERR_UNSUPPORTED) and leave it to their Python wrapper to copy.
A tensor fresh from the allocator is always 16-byte aligned, so without these tests one route of each had never run.  The
inventory -- entry point, class, the condition of each route -- is DESIGN.md, "16-byte accesses to a caller's pointer"; the classes:
  (b) dispatch between a vector and a scalar route: both run here, against the reference and bar of the op's existing test;
  (c) refusal: the public op must still compute (a realigning copy: same kernel, same bits), the entry point itself must refuse;
  (d) were: 16-byte accesses gated on sizes only (l3d_wgrad, l3d_chamfer_partials, l3d_chamfer_loss_local_mb, l3d_pointwise_conv,
      l3d_split_f16_rows / l3d_split_f16_operand, l3d_curve_walk) -- now (b) or (c), and tested as such.
Misaligned inputs are contiguous copies at a 4-byte offset into a slightly larger buffer (at_offset): what x[1:] of a flat buffer is.

train.hip's kernels are also held, one by one through _lib.call, to fp64 (or to an fp32 replay, bit for bit) of the formulas in its
header comment: both routes, the three activation codes, the pooled-gradient arguments in every dy / K combination."""
import functools
import os
import struct
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LRELU = struct.unpack("<i", struct.pack("<f", 0.2))[0]          # activation code of LeakyReLU(0.2): the slope's fp32 bits (common.h)
SLOPE = torch.tensor(0.2, dtype=torch.float32)
SENTINEL = 12345.0


def at_offset(t, k):
    """a contiguous copy of t whose data_ptr() % 16 == 4 * k, k in 0..3"""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0 and t.element_size() == 4
    v = buf[k:k + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 * k
    return v


def out_at_offset(shape, k, dtype=torch.float32):
    """an output tensor at offset k whose buffer is filled with a sentinel: (tensor, check) -- check() asserts that nothing
    outside the tensor was written (a 16-byte store on the scalar route's tensor would reach past its end)"""
    n = int(np.prod(shape))
    buf = torch.full((n + 4,), SENTINEL, dtype=dtype, device="cuda")
    v = buf[k:k + n].view(shape)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 * k

    def check():
        assert bool((buf[:k] == SENTINEL).all()) and bool((buf[k + n:] == SENTINEL).all()), "wrote outside the output tensor"
    return v, check


def same_bits(a, b):
    a, b = a.detach().contiguous().cpu(), b.detach().contiguous().cpu()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


def call(*args, **kw):
    from learning3d_amd._lib import call as c
    return c(*args, **kw)


def refused(name, *args):
    """the entry point returns L3D_ERR_UNSUPPORTED for these arguments (a refusal launches nothing)"""
    from learning3d_amd import _lib
    with pytest.raises(_lib.L3DError, match=rf"\(status {_lib.L3D_ERR_UNSUPPORTED},"):
        _lib.call(name, *args)


# ------------------------------------------------------------------------------------------------ train.hip, kernel by kernel
B_, C_ = 2, 5


@functools.lru_cache(maxsize=None)
def train_case(P):
    """z [2,5,P] with exact zeros of the pre-activation v = z scale + shift mixed in (channel 0: z = 0, shift = 0; channel 1: z = 1,
    scale = 0.5, shift = -0.5), one negative scale, a gradient, and arbitrary fp64 per-channel constants.  CPU tensors, never modified."""
    g = torch.Generator().manual_seed(1000 + P)
    z = torch.randn((B_, C_, P), generator=g)
    z[torch.rand(z.shape, generator=g) < 0.15] = 0.0
    z[:, 1][torch.rand((B_, P), generator=g) < 0.15] = 1.0
    scale = torch.rand(C_, generator=g) + 0.5
    shift = torch.randn(C_, generator=g) * 0.3
    shift[0] = 0.0
    scale[1], shift[1] = 0.5, -0.5
    scale[3] = -0.75
    dy = torch.randn((B_, C_, P), generator=g)
    c64 = {n: (torch.randn(C_, generator=g, dtype=torch.float64) * 0.5 + (1.0 if n in ("rstd", "gr") else 0.0))
           for n in ("mean", "rstd", "gr", "m1", "m2")}
    v = pre_act(z, scale, shift)
    assert int((v == 0).sum()) > 0 or P < 8
    return dict(z=z, scale=scale, shift=shift, dy=dy, **c64)


def pre_act(z, scale, shift):
    """v = z scale + shift in fp32 with two roundings, as the kernels form it (the library is built without contraction)"""
    return z * scale[None, :, None] + shift[None, :, None]


def act_forward(v, act):
    """common.h l3d_act in fp32: ReLU fmaxf(v, 0); LeakyReLU fmaxf(v, v slope)"""
    if act == 0:
        return v
    return torch.maximum(v, torch.zeros_like(v)) if act == 1 else torch.maximum(v, v * SLOPE)


def act_grad(v, act):
    """train.hip tr_act_grad: 1 where there is no activation or v > 0, else 0 (ReLU) or the slope: v == 0 takes the second branch"""
    one = torch.ones_like(v)
    if act == 0:
        return one
    return torch.where(v > 0, one, torch.zeros_like(v) if act == 1 else one * SLOPE)


def grad_reference(c, act, dy, dense_pool):
    """(g fp32, zhat fp64): the gradient that enters the two backward kernels and the normalised pre-activation.  dy + the dense
    scatter of the pooled gradient is formed in fp64 and rounded to fp32 once -- the kernel's single fp32 add (at most one pooled term
    per position) -- and multiplied by act'(v) in fp32: g is an fp32 quantity by the kernels' contract, everything behind it is fp64.
    The branch of act' is taken on the fp32 v the kernels recompute, not on an fp64 one."""
    gin = torch.zeros_like(c["z"], dtype=torch.float64)
    if dy is not None:
        gin = gin + dy.double()
    if dense_pool is not None:
        gin = gin + dense_pool
    g = gin.float() * act_grad(pre_act(c["z"], c["scale"], c["shift"]), act)
    zhat = (c["z"].double() - c["mean"][None, :, None]) * c["rstd"][None, :, None]
    return g, zhat


def check_partials(got, terms, what):
    """fp64 partial sums [B,C] against numpy: rtol 1e-12 and atol 1e-12 x the sum of the absolute terms (the bar of the per-cloud
    partial sums in test_train_conv_bn_relu_matches_torch)"""
    want = terms.sum(-1).numpy()
    tol = 1e-12 * np.abs(want) + 1e-12 * terms.abs().sum(-1).numpy()
    err = np.abs(got.cpu().numpy() - want)
    print(f"{what}: max error / tolerance {float((err / np.maximum(tol, 1e-300)).max()):.3g}")
    assert (err <= tol).all(), (what, float((err / np.maximum(tol, 1e-300)).max()))


def check_one_ulp(got, want64, what):
    """fp32 values computed in fp64 and rounded once: within one fp32 ulp of the fp64 reference rounded to fp32"""
    want = want64.float().numpy()
    err = np.abs(got.cpu().numpy().astype(np.float64) - want.astype(np.float64))
    ulp = np.spacing(np.abs(want)).astype(np.float64)
    print(f"{what}: max error {float((err / ulp).max()):.3g} ulp")
    assert (err <= ulp).all(), (what, float((err / ulp).max()))


def dz_reference(c, g, zhat):
    """dz = gr (g - m1 - zhat m2) in fp64, in the kernel's order"""
    ch = lambda n: c[n][None, :, None]
    return ch("gr") * (g.double() - ch("m1") - zhat * ch("m2"))


def run_backward_pair(c, act, k, dy, dpool, pidx, K):
    """l3d_bn_backward_stats and l3d_bn_act_backward with z / dy / dz at offset k -> (part [B,C,2] fp64, dz fp32), and which route ran"""
    P = c["z"].shape[-1]
    z = at_offset(c["z"].cuda(), k)
    dyd = at_offset(dy.cuda(), k) if dy is not None else None
    scale, shift = c["scale"].cuda(), c["shift"].cuda()
    consts = [c[n].cuda() for n in ("mean", "rstd", "gr", "m1", "m2")]
    part = torch.full((B_, C_, 2), float("nan"), dtype=torch.float64, device="cuda")
    call("l3d_bn_backward_stats", dyd, z, scale, shift, consts[0], consts[1], B_, C_, P, act, part, dpool, pidx, K)
    dz, untouched = out_at_offset((B_, C_, P), k)
    call("l3d_bn_act_backward", dyd, z, scale, shift, *consts, B_, C_, P, act, dz, dpool, pidx, K)
    torch.cuda.synchronize()
    untouched()
    vec = P % 4 == 0 and (dpool is None or K % 4 == 0) and all(t is None or t.data_ptr() % 16 == 0 for t in (z, dyd, dz))
    return part, dz, vec


@pytest.mark.parametrize("P", [2052, 1023, 7])
def test_channel_stats_both_routes(P):
    """l3d_channel_stats: per-(cloud, channel) (sum z, sum z^2) in fp64; a row takes the 16-byte loop when P % 4 == 0 and the row starts
    on a 16-byte boundary (P = 2052 at offset 0: two trips of 1024 values and a tail trip), the scalar loop otherwise"""
    c = train_case(P)
    z64 = c["z"].double()
    for k in (0, 1):
        z = at_offset(c["z"].cuda(), k)
        part = torch.full((B_, C_, 2), float("nan"), dtype=torch.float64, device="cuda")
        call("l3d_channel_stats", z, B_, C_, P, part)
        check_partials(part[..., 0], z64, f"channel_stats sum P={P} offset {k}")
        check_partials(part[..., 1], z64 * z64, f"channel_stats sum of squares P={P} offset {k}")


@pytest.mark.parametrize("act", [0, 1, LRELU])
@pytest.mark.parametrize("P", [2052, 1023, 7])
def test_bn_act_forward_is_the_fp32_formula_on_both_routes(P, act):
    """l3d_bn_act_forward: y = act(z scale + shift), fp32 arithmetic -- the same bits as the formula replayed in fp32 torch, on the
    16-byte route (P % 4 == 0, z and y aligned) and on the scalar one (offset 1, or P = 1023 / 7)"""
    c = train_case(P)
    want = act_forward(pre_act(c["z"], c["scale"], c["shift"]), act)
    for k in (0, 1):
        z = at_offset(c["z"].cuda(), k)
        y, untouched = out_at_offset((B_, C_, P), k)
        call("l3d_bn_act_forward", z, c["scale"].cuda(), c["shift"].cuda(), B_, C_, P, act, y)
        torch.cuda.synchronize()
        untouched()
        assert same_bits(y, want), (P, act, k, float((y.cpu() - want).abs().max()))


@pytest.mark.parametrize("act", [0, 1, LRELU])
@pytest.mark.parametrize("P", [2052, 1023, 7])
def test_bn_backward_kernels_vs_fp64_on_both_routes(P, act):
    """l3d_bn_backward_stats (sum g, sum g zhat per cloud and channel, fp64) and l3d_bn_act_backward (dz = gr (g - m1 - zhat m2), fp64,
    rounded once) without a pooled gradient: the partial sums at the 1e-12 bar, dz within one fp32 ulp of the fp64 reference (what
    may differ is the order of the fp64 operations), and the 16-byte and the scalar route give the same dz bit for bit (both do the
    same arithmetic per element)."""
    c = train_case(P)
    g, zhat = grad_reference(c, act, c["dy"], None)
    dzs = []
    for k in (0, 1):
        part, dz, vec = run_backward_pair(c, act, k, c["dy"], None, None, 0)
        assert vec == (P == 2052 and k == 0)
        check_partials(part[..., 0], g.double(), f"bn_backward_stats sum g P={P} act={act} offset {k}")
        check_partials(part[..., 1], g.double() * zhat, f"bn_backward_stats sum g zhat P={P} act={act} offset {k}")
        check_one_ulp(dz, dz_reference(c, g, zhat), f"bn_act_backward P={P} act={act} offset {k}")
        dzs.append(dz)
    assert same_bits(dzs[0], dzs[1])


@pytest.mark.parametrize("K", [4, 20, 256, 1, 3, 5, 9, 255])
def test_pooled_gradient_arguments_every_cell(K):
    """dpool / pidx / K of l3d_bn_backward_stats and l3d_bn_act_backward (a layer whose output is also max-pooled over runs of K): K
    in {4, 20, 256} takes the 16-byte route (one pidx / dpool load serves four positions), every other K the scalar one even where
    P % 4 == 0 (K = 5, 8 runs: P = 40); with and without dy; ReLU and LeakyReLU.  pidx is l3d_max_last's arg-max of a tensor with
    exact ties (ReLU zeros, duplicated maxima) that includes 0 and K - 1.  Reference: dy + the dense scatter of dpool at pidx."""
    N = 8
    P = N * K
    c = train_case(P)
    y = act_forward(pre_act(c["z"], c["scale"], c["shift"]), 1).view(B_, C_, N, K).clone()
    y[0, 0, 0] = 0.0; y[0, 0, 0, K - 1] = 7.0                       # arg-max K - 1
    y[0, 0, 1] = 0.0; y[0, 0, 1, 0] = 7.0                           # arg-max 0
    y[0, 0, 2] = 0.0                                                # all ReLU zeros: the first one
    if K >= 3:
        y[0, 0, 3] = 0.5; y[0, 0, 3, 1] = 9.0; y[0, 0, 3, 2] = 9.0  # a duplicated maximum: the first one
    y[1, 4, 7] = 0.0; y[1, 4, 7, K - 1] = 3.0                       # arg-max K - 1 in the last run of the tensor
    R = B_ * C_ * N
    ymax = torch.empty(R, dtype=torch.float32, device="cuda")
    pidx = torch.empty(R, dtype=torch.uint8, device="cuda")
    call("l3d_max_last", y.cuda(), R, K, ymax, pidx)
    want_idx = y.numpy().reshape(R, K).argmax(axis=1)               # numpy: the first maximum
    assert np.array_equal(pidx.cpu().numpy(), want_idx) and want_idx.min() == 0 and want_idx.max() == K - 1
    gen = torch.Generator().manual_seed(K)
    dpool = torch.randn((B_, C_, N), generator=gen)
    dense = torch.zeros((R, K), dtype=torch.float64)
    dense[torch.arange(R), torch.from_numpy(want_idx)] = dpool.double().reshape(R)
    dense = dense.view(B_, C_, P)
    dpool_d = dpool.cuda()
    for dy in (c["dy"], None):
        for act in (1, LRELU):
            g, zhat = grad_reference(c, act, dy, dense)
            dzs = []
            for k in ((0, 1) if K % 4 == 0 else (0,)):
                part, dz, vec = run_backward_pair(c, act, k, dy, dpool_d, pidx, K)
                assert vec == (K % 4 == 0 and k == 0)
                what = f"K={K} dy={'given' if dy is not None else 'NULL'} act={act} offset {k}"
                check_partials(part[..., 0], g.double(), "pooled bn_backward_stats sum g " + what)
                check_partials(part[..., 1], g.double() * zhat, "pooled bn_backward_stats sum g zhat " + what)
                check_one_ulp(dz, dz_reference(c, g, zhat), "pooled bn_act_backward " + what)
                dzs.append(dz)
            assert all(same_bits(dzs[0], d) for d in dzs[1:])


def test_sum_clouds_f64_is_the_left_to_right_sum():
    """l3d_sum_clouds_f64: tot[j] = part[0][j] + part[1][j] + ... in cloud order: the same bits as that loop in numpy"""
    part = torch.randn((5, 777), generator=torch.Generator().manual_seed(2), dtype=torch.float64) * 1e3
    tot = torch.empty(777, dtype=torch.float64, device="cuda")
    call("l3d_sum_clouds_f64", part.cuda(), 5, 777, tot)
    want = np.zeros(777)
    for b in range(5):
        want = want + part[b].numpy()
    assert np.array_equal(tot.cpu().numpy(), want)


def finalize_replay(C, part, n, bias, gamma, beta, eps, mode, mom, rm, rv):
    """bn_finalize_kernel in numpy, operation by operation: fp64 throughout, the running statistics updated in fp32 as its code says
    (rm keep + m (float)(mean + b), keep = (float)(1 - mom), m = (float)mom)"""
    b = bias.astype(np.float64) if bias is not None else np.zeros(C)
    mean, rstd, var = -b, np.ones(C), None
    if mode == 0:
        t0, t1 = np.zeros(C), np.zeros(C)
        for k in range(part.shape[0]):
            t0, t1 = t0 + part[k, :, 0], t1 + part[k, :, 1]
        mean = t0 / n
        var = t1 / n - mean * mean
        var = np.where(var > 0.0, var, 0.0)
        if rm is not None:
            unbiased = var * (n / (n - 1.0 if n - 1.0 > 1.0 else 1.0))
            m, keep = np.float32(mom), np.float32(1.0 - mom)
            rm = rm * keep + m * (mean + b).astype(np.float32)
            rv = rv * keep + m * unbiased.astype(np.float32)
        rstd = 1.0 / np.sqrt(var + eps)
    if mode == 1:
        mean = rm.astype(np.float64) - b
        rstd = 1.0 / np.sqrt(rv.astype(np.float64) + eps)
    g = gamma.astype(np.float64) if gamma is not None else np.ones(C)
    be = beta.astype(np.float64) if beta is not None else np.zeros(C)
    return mean, rstd, g * rstd, be, rm, rv


@pytest.mark.parametrize("mode,bias,affine,running,mom", [(0, True, True, True, 0.1), (0, False, True, True, 1.0), (0, True, False, False, 0.0),
                                                          (0, False, False, True, 0.1), (1, True, True, True, 0.0), (1, False, False, True, 0.0),
                                                          (2, True, False, False, 0.0), (2, False, True, False, 0.0)])
def test_bn_finalize_vs_numpy_replay(mode, bias, affine, running, mom):
    """l3d_bn_finalize, modes 0 (batch statistics) / 1 (running statistics) / 2 (none), with and without bias / gamma / beta / running
    statistics, C = 300 (two workgroups).  mean64 comes from fp64 sums and one division: the replay's bits.  rstd64 and gr64 add a
    square root, a division and a product: within 4 fp64 ulp (one each, were the device's not correctly rounded, and one to spare).
    scale and shift are the kernel's own fp64 values rounded once: bit-equal to that rounding of what it wrote.  The running
    statistics (fp32 arithmetic on fp64 inputs that involve no square root) equal the replay's bits."""
    C, Bc, P, eps = 300, 3, 500, 1e-5
    rng = np.random.default_rng(100 * mode + 10 * bias + affine)
    z = rng.standard_normal((Bc, C, P)) * rng.uniform(0.5, 2.0, (1, C, 1)) + rng.uniform(-1, 1, (1, C, 1))
    part = np.stack([z.sum(-1), (z * z).sum(-1)], axis=-1) if mode == 0 else None
    n = float(Bc * P)
    f32 = lambda a: a.astype(np.float32)
    b = f32(rng.standard_normal(C)) if bias else None
    ga, be = (f32(rng.uniform(0.5, 1.5, C)), f32(rng.standard_normal(C))) if affine else (None, None)
    rm, rv = (f32(rng.standard_normal(C)), f32(rng.uniform(0.5, 2.0, C))) if running else (None, None)
    d = lambda a: torch.from_numpy(a).cuda() if a is not None else None
    rm_d, rv_d = d(rm), d(rv)
    out64 = [torch.full((C,), float("nan"), dtype=torch.float64, device="cuda") for _ in range(3)]
    out32 = [torch.full((C,), float("nan"), dtype=torch.float32, device="cuda") for _ in range(2)]
    call("l3d_bn_finalize", d(part), Bc if mode == 0 else 0, C, n, d(b), d(ga), d(be), eps, mode, float(mom), rm_d, rv_d, *out64, *out32)
    mean, rstd, gr, bet, rm_w, rv_w = finalize_replay(C, part, n, b, ga, be, eps, mode, mom, rm, rv)
    mean_g, rstd_g, gr_g = [t.cpu().numpy() for t in out64]
    assert np.array_equal(mean_g, mean)
    for name, got, want in (("rstd", rstd_g, rstd), ("gr", gr_g, gr)):
        assert (np.abs(got - want) <= 4 * np.spacing(np.abs(want))).all(), (name, float(np.abs(got / want - 1).max()))
    assert np.array_equal(out32[0].cpu().numpy(), gr_g.astype(np.float32))
    assert np.array_equal(out32[1].cpu().numpy(), (bet - mean_g * gr_g).astype(np.float32))
    if running:
        assert np.array_equal(rm_d.cpu().numpy(), rm_w) and np.array_equal(rv_d.cpu().numpy(), rv_w)
        assert (mode == 0) == (not np.array_equal(rm_w, rm))            # updated in train mode only


def test_bn_backward_finalize_vs_numpy_replay():
    """l3d_bn_backward_finalize: m1 / m2 = the batch sums over every rank's clouds (part_all; NULL: the local ones) over n, zeros without
    batch statistics; dbeta / dgamma = this rank's sums, dbias = 0 with batch statistics else gr x this rank's sum of g -- fp64 sums in
    cloud order and one division: the replay's bits, the fp32 outputs one rounding of them.  Each of dbias / dgamma / dbeta NULL in turn."""
    C, Bl, Ba, n = 300, 2, 5, 4000.0
    rng = np.random.default_rng(7)
    pl, pa, gr = rng.standard_normal((Bl, C, 2)) * 50, rng.standard_normal((Ba, C, 2)) * 50, rng.uniform(0.5, 2.0, C)
    d = lambda a: torch.from_numpy(a).cuda()

    def seq(p, j):
        s = np.zeros(C)
        for k in range(p.shape[0]):
            s = s + p[k, :, j]
        return s
    for with_all in (True, False):
        for batch_stats in (0, 1):
            for absent in (None, 0, 1, 2):
                outs = [None if i == absent else torch.full((C,), float("nan"), dtype=torch.float32, device="cuda") for i in range(3)]
                m1 = torch.full((C,), float("nan"), dtype=torch.float64, device="cuda")
                m2 = torch.full_like(m1, float("nan"))
                call("l3d_bn_backward_finalize", d(pl), Bl, d(pa) if with_all else None, Ba if with_all else 0, C, n, batch_stats, d(gr),
                     m1, m2, *outs)
                l0, l1 = seq(pl, 0), seq(pl, 1)
                t0, t1 = (seq(pa, 0), seq(pa, 1)) if with_all else (l0, l1)
                assert np.array_equal(m1.cpu().numpy(), t0 / n if batch_stats else np.zeros(C))
                assert np.array_equal(m2.cpu().numpy(), t1 / n if batch_stats else np.zeros(C))
                want = [np.zeros(C, np.float32) if batch_stats else (gr * l0).astype(np.float32), l1.astype(np.float32), l0.astype(np.float32)]
                for i, o in enumerate(outs):
                    assert o is None or np.array_equal(o.cpu().numpy(), want[i]), (with_all, batch_stats, absent, i)


def test_conv_layer_cumulative_average_momentum_none():
    """_ConvAffineAct with BatchNorm(momentum=None): the running statistics are the cumulative average (momentum 1 / num_batches_tracked)
    -- against torch.nn.BatchNorm1d(momentum=None) in fp64 over two steps, at the bars of test_conv_layer_eval_bias_and_leaky_variants_vs_fp64"""
    from learning3d_amd.models import _train
    torch.manual_seed(5)
    Cin, Cout, P = 6, 64, 256
    conv = torch.nn.Conv1d(Cin, Cout, 1, bias=True).cuda()
    bn = torch.nn.BatchNorm1d(Cout, momentum=None).cuda().train()
    c64 = torch.nn.Conv1d(Cin, Cout, 1, bias=True).cuda().double()
    c64.load_state_dict({k: v.double() for k, v in conv.state_dict().items()})
    b64 = torch.nn.BatchNorm1d(Cout, momentum=None).cuda().double().train()
    for step in (1, 2):
        x = torch.randn(3, Cin, P, device="cuda") * (0.5 * step) + 0.3 * step
        ya = _train.conv_bn_act(x, conv, bn, relu=1, sync=False)
        yb = torch.relu(b64(c64(x.double())))
        np.testing.assert_allclose(ya.detach().cpu().numpy(), yb.detach().cpu().numpy(), rtol=1e-4, atol=1e-5)
        assert int(bn.num_batches_tracked) == step
        np.testing.assert_allclose(bn.running_mean.cpu().numpy(), b64.running_mean.cpu().numpy(), rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(bn.running_var.cpu().numpy(), b64.running_var.cpu().numpy(), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("K", [3, 4, 33, 256])
def test_max_last_both_routes_equal_torch(K):
    """l3d_max_last / l3d_max_last_backward: K % 4 == 0 with a 16-byte aligned x (gx) reads (writes) 16 bytes per lane, everything
    else -- K % 4 != 0, or offset 1 -- the scalar loop: values, first-maximum indices under exact ties and the dense gradient equal
    torch.max's bit for bit, as test_max_over_last_matches_torch asks of the aligned case.  Then the public op on a misaligned input
    with a misaligned upstream gradient (it raised L3DError for K % 4 == 0 before l3d_max_last had a scalar route for that)."""
    from learning3d_amd.models import _train
    gen = torch.Generator().manual_seed(30 + K)
    shape = (2, 5, 31, K)                                             # 310 rows: two workgroups
    x = torch.randn(shape, generator=gen)
    x = torch.where(torch.rand(shape, generator=gen) < 0.3, torch.zeros_like(x), x).relu()
    x[..., 1] = x[..., 0]
    x[0, 0, 0] = 0.0; x[0, 0, 0, K // 2] = 9.0; x[0, 0, 0, K - 1] = 9.0       # a duplicated maximum away from the row's start
    R = x.numel() // K
    want_i = torch.from_numpy(x.numpy().reshape(R, K).argmax(axis=1)).view(shape[:-1])      # numpy: the first maximum, torch.max's rule
    want_v = x.max(dim=-1)[0]
    gr = torch.randn(R, generator=gen)
    want_gx = torch.zeros((R, K))
    want_gx[torch.arange(R), want_i.reshape(R)] = gr
    for k in (0, 1):
        xd = at_offset(x.cuda(), k)
        v, idx = torch.empty(R, dtype=torch.float32, device="cuda"), torch.empty(R, dtype=torch.uint8, device="cuda")
        call("l3d_max_last", xd, R, K, v, idx)
        assert same_bits(v, want_v.reshape(R)) and np.array_equal(idx.cpu().numpy(), want_i.numpy().reshape(R)), (K, k)
        gx, untouched = out_at_offset((R, K), k)
        call("l3d_max_last_backward", at_offset(gr.cuda(), k), idx, R, K, gx)
        torch.cuda.synchronize()
        untouched()
        assert same_bits(gx, want_gx), (K, k)
        a = at_offset(x.cuda(), k).detach().requires_grad_()
        va = _train.max_over_last(a)
        assert same_bits(va, want_v.unsqueeze(-1))
        va.backward(at_offset(gr.cuda().view(va.shape), k))
        assert same_bits(a.grad, want_gx.view(shape)), (K, k)
    nanrow = at_offset(torch.tensor([[1.0, float("nan"), 3.0, 2.0]], device="cuda"), 1)
    assert torch.isnan(_train.max_over_last(nanrow)).all()


# ------------------------------------------------------------------------------------------------ class (b) outside train.hip
def test_wgrad_both_routes_vs_fp64_and_deterministic():
    """l3d_wgrad: 16-byte loads along P when P % 4 == 0 AND dz, x are 16-byte aligned (the alignment was not looked at before), scalar
    loads otherwise.  Bar of test_wgrad_kernel_vs_fp64_and_deterministic: 2e-6 of max |dW|, the same bits on every run -- and, the
    products and their order being the same, the same bits on both routes."""
    from learning3d_amd.models import _train
    rng = np.random.default_rng(9)
    for (Bc, Cout, Cin, P) in [(3, 128, 64, 1000), (3, 128, 64, 1001), (5, 100, 37, 333)]:
        dz = torch.from_numpy(rng.standard_normal((Bc, Cout, P)).astype(np.float32)).cuda()
        x = torch.from_numpy((rng.standard_normal((Bc, Cin, P)) + 0.5).astype(np.float32)).cuda()
        want = torch.einsum("bop,bip->oi", dz.double(), x.double())
        runs = []
        for kd, kx in ((0, 0), (1, 1), (0, 1)):
            a, b = at_offset(dz, kd), at_offset(x, kx)
            got = _train.wgrad(a, b)
            assert float((got.double() - want).abs().max() / want.abs().max()) <= 2e-6, (Bc, Cout, Cin, P, kd, kx)
            assert torch.equal(got, _train.wgrad(a, b))
            assert torch.equal(_train.wgrad(a, b, pc=256), _train.wgrad(a, b, pc=256))
            runs.append(got)
        assert all(torch.equal(runs[0], r) for r in runs[1:])


def test_chamfer_loss_tails_both_routes():
    """l3d_chamfer_partials and l3d_chamfer_loss_local_mb: the sqrt-sums read dist1 / dist2 16 bytes at a time when the tensor is 16-byte
    aligned (not looked at before) and through the scalar loop otherwise.  Bars of test_chamfer_loss_local_equals_partials_plus_combine."""
    from learning3d_amd.losses.chamfer_distance import chamfer_combine, chamfer_loss_local, chamfer_partials
    rng = np.random.default_rng(44)
    for (Bc, N, M) in [(3, 77, 130), (1, 5, 2)]:
        d1 = torch.from_numpy(rng.uniform(0, 2, (Bc, N)).astype(np.float32)).cuda()
        d2 = torch.from_numpy(rng.uniform(0, 2, (Bc, M)).astype(np.float32)).cuda()
        s1, s2 = np.sqrt(d1.cpu().numpy()).astype(np.float64), np.sqrt(d2.cpu().numpy()).astype(np.float64)      # the kernels' sqrtf, summed in fp64
        want = (np.sqrt(d1.cpu().numpy().astype(np.float64)).mean() + np.sqrt(d2.cpu().numpy().astype(np.float64)).mean()) / 2
        for k1, k2 in ((0, 0), (1, 1), (1, 0), (0, 3)):
            a1, a2 = at_offset(d1, k1), at_offset(d2, k2)
            part = chamfer_partials(a1, a2)
            np.testing.assert_allclose(part.cpu().numpy(), [s1.sum(), s2.sum(), s1.size, s2.size], rtol=1e-12)
            b = chamfer_combine(part)
            for _ in range(2):                                       # the multi-workgroup kernel re-arms its ticket
                a = chamfer_loss_local(a1, a2)
                assert abs(a.item() - b.item()) <= 1.2e-7 * max(1.0, abs(b.item()))
            assert abs(a.item() - want) < 1e-6, (Bc, N, M, k1, k2)


def test_pointwise_conv_fp32_mfma_both_routes():
    """l3d_pointwise_conv (mlp.hip): the unconditional 16-byte tile loads need full tiles and aligned x, w; the ragged kernel loads 16
    bytes where the row length (Cin for w and a channel-last x, N for a channel-first x) is a multiple of 4 AND the tensor is aligned
    (the alignment was not looked at before), 4 bytes otherwise.  Shapes of test_pointwise_conv_ragged_shapes with their vector routes
    and the neighbouring sizes that flip them, at its bar (rtol 1e-4, atol 1e-5 against fp64); x and w at offset 0 and 1."""
    from learning3d_amd.models._fused import pointwise_conv
    rng = np.random.default_rng(9)
    for (Bc, Cin, Cout, N) in [(2, 3, 64, 100), (2, 3, 64, 101), (1, 132, 70, 257), (1, 130, 70, 256), (1, 16, 128, 128)]:
        x = rng.standard_normal((Bc, Cin, N)).astype(np.float32)
        w = (rng.standard_normal((Cout, Cin)) / np.sqrt(Cin)).astype(np.float32)
        sc = rng.uniform(0.5, 1.5, Cout).astype(np.float32)
        sh = rng.uniform(-0.5, 0.5, (Bc, Cout)).astype(np.float32)
        want = np.maximum(np.einsum("oc,bcn->bon", w.astype(np.float64), x) * sc[None, :, None] + sh[:, :, None], 0)
        xd, xl, wd = torch.from_numpy(x).cuda(), torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1))).cuda(), torch.from_numpy(w).cuda()
        scd, shd = torch.from_numpy(sc).cuda(), torch.from_numpy(sh).cuda()
        for kx, kw in ((0, 0), (1, 1), (1, 0), (0, 1)):
            got = pointwise_conv(at_offset(xd, kx), at_offset(wd, kw), scd, shd, relu=True, split=False)
            np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-4, atol=1e-5, err_msg=str((Bc, Cin, Cout, N, kx, kw)))
            got = pointwise_conv(at_offset(xl, kx), at_offset(wd, kw), scd, shd, relu=True, channel_last=True, split=False)
            np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-4, atol=1e-5, err_msg=str((Bc, Cin, Cout, N, kx, kw, "cl")))


def bm_mode(t, R, K, swap):
    """bmm.hip bm_mode of an operand as _rows.bmm passes it: 1 = 16-byte loads along k, 2 = along the rows, 0 = scalar"""
    from learning3d_amd.models import _rows
    s = list(_rows._as4(t).stride())
    if swap:                                                           # B is given as [K x N]: seen as [N rows x K]
        s[2], s[3] = s[3], s[2]
    al = t.data_ptr() % 16 == 0 and s[0] % 4 == 0 and s[1] % 4 == 0 and K % 16 == 0
    if s[3] == 1 and al and s[2] % 4 == 0:
        return 1
    if s[2] == 1 and al and s[3] % 4 == 0 and R % 8 == 0:
        return 2
    return 0


def bmm_check(name, x, y):
    """the two bars of test_bmm_f32_vs_fp64: the fp32 dot-product bound per element, and 4 x torch.matmul's own error"""
    from learning3d_amd.models import _rows
    got = _rows.bmm(x, y)
    want = torch.matmul(x.double(), y.double())
    ref = torch.matmul(x, y)
    bound = torch.matmul(x.double().abs(), y.double().abs()) * (x.shape[-1] * 2.0 ** -24) + 1e-30
    err, err_t = (got.double() - want).abs(), (ref.double() - want).abs()
    assert bool((err <= bound).all()), (name, float((err / bound).max()))
    assert float(err.max()) <= 4 * float(err_t.max()) + 1e-6 * float(want.abs().max()), (name, float(err.max()), float(err_t.max()))


def test_bmm_all_nine_operand_mode_pairs():
    """l3d_bmm_f32 picks a fetch form per operand (bm_mode: alignment, strides % 4, K % 16, rows % 8).  All nine (A mode, B mode) pairs at
    one small shape -- that the intended pair runs is asserted by recomputing bm_mode's rule from the tensors' pointers and strides --
    then the sizes that flip a vector form to the scalar one: K = 17, M % 8 != 0, N % 8 != 0."""
    gen = torch.Generator().manual_seed(3)
    M, N, K = 72, 40, 32
    a, b = torch.randn((2, M, K), generator=gen).cuda(), torch.randn((2, K, N), generator=gen).cuda()
    tr = lambda t, k: at_offset(t.transpose(1, 2).contiguous(), k).transpose(1, 2)        # the same values, the other axis contiguous
    a_forms = {1: at_offset(a, 0), 2: tr(a, 0), 0: at_offset(a, 1)}
    b_forms = {1: tr(b, 0), 2: at_offset(b, 0), 0: at_offset(b, 1)}
    seen = set()
    for am, x in a_forms.items():
        for bmd, y in b_forms.items():
            assert (bm_mode(x, M, K, False), bm_mode(y, N, K, True)) == (am, bmd)
            bmm_check((am, bmd), x, y)
            seen.add((am, bmd))
    assert len(seen) == 9
    assert bm_mode(tr(a, 1), M, K, False) == 0 and bm_mode(tr(b, 1), N, K, True) == 0
    bmm_check("transposed, misaligned", tr(a, 1), tr(b, 1))
    for (m, n, kk) in [(72, 40, 17), (76, 40, 32), (72, 44, 32)]:
        a2, b2 = torch.randn((2, m, kk), generator=gen).cuda(), torch.randn((2, kk, n), generator=gen).cuda()
        x, y = tr(a2, 0), at_offset(b2, 0)                                                 # (2, 2) at (72, 40, 32)
        assert (bm_mode(x, m, kk, False), bm_mode(y, n, kk, True)) == ((0, 0) if kk == 17 else (0, 2) if m == 76 else (2, 0))
        bmm_check((m, n, kk), x, y)
        assert (bm_mode(at_offset(a2, 0), m, kk, False), bm_mode(tr(b2, 0), n, kk, True)) == ((0, 0) if kk == 17 else (1, 1))
        bmm_check((m, n, kk, "along k"), at_offset(a2, 0), tr(b2, 0))


def test_colsum_rows_both_routes():
    """l3d_colsum_rows: float4 columns when cols % 4 == 0, row_stride % 4 == 0 and x is 16-byte aligned, a thread per column otherwise.
    Bar of test_colsum_rows_vs_fp64_and_repeatable: the fp32 summation bound against fp64, the same bits on every run."""
    from learning3d_amd.models import _rows
    gen = torch.Generator().manual_seed(9)
    for R, Cn in ((1000, 300), (1000, 301), (127, 5)):
        x = torch.randn((R, Cn + 8), generator=gen).cuda()
        for v in (at_offset(x[:, :Cn].contiguous(), 0), at_offset(x[:, :Cn].contiguous(), 1), at_offset(x, 0)[:, :Cn], at_offset(x, 1)[:, :Cn],
                  at_offset(x, 0)[:, 3:3 + Cn], at_offset(x[:, :Cn + 7].contiguous(), 0)[:, :Cn]):
            got = _rows.colsum(v)
            assert torch.equal(got, _rows.colsum(v))
            want = v.double().sum(0)
            bound = v.double().abs().sum(0) * (R * 2.0 ** -24) + 1e-30
            assert bool(((got.double() - want).abs() <= bound).all()), (R, Cn, v.data_ptr() % 16, v.stride())


def test_scatter_add_det_source_row_alignment():
    """l3d_scatter_add_det stages a cloud's source row of one channel in LDS with 16-byte loads when the ROW is 16-byte aligned (S = 50
    floats per row: every other row of an aligned tensor, the other rows of one at offset 2) and with scalar loads otherwise.  Its
    contract (tests/test_gpu_limits.py): every target's entries summed in ascending entry order in fp32 -- np.add.at's bits -- on
    every run."""
    from learning3d_amd.utils import pointnet2_utils as P
    Bc, C, S, div, T = 2, 3, 50, 4, 20
    rng = np.random.default_rng(12)
    src = rng.standard_normal((Bc, C, S)).astype(np.float32)
    idx = rng.integers(0, T, (Bc, S * div)).astype(np.int32)
    wgt = rng.uniform(0.5, 1.5, (Bc, S * div)).astype(np.float32)
    for weight in (None, wgt):
        want = np.zeros((Bc, C, T), np.float32)
        for bb in range(Bc):
            for c in range(C):
                vals = np.repeat(src[bb, c], div)
                np.add.at(want[bb, c], idx[bb], vals * weight[bb] if weight is not None else vals)
        for k in (0, 1, 2, 3):
            s = at_offset(torch.from_numpy(src).cuda(), k)
            w = at_offset(torch.from_numpy(weight).cuda(), k) if weight is not None else None
            for _ in range(2):
                got = P._scatter_add_det(s, torch.from_numpy(idx).cuda(), w, T, div)
                assert same_bits(got, torch.from_numpy(want)), (k, weight is not None)


def test_absmax4_partials_head_and_tail():
    """l3d_absmax4_partials: a 16-byte aligned tensor is read as float4 with a scalar tail, a misaligned one entirely through the scalar
    loop: the 4 x 64 block maxima reduce to exactly max |x| of each tensor either way (an absent tensor: zeros)."""
    gen = torch.Generator().manual_seed(4)
    U, V = torch.randn((2, 50, 12), generator=gen).cuda(), torch.randn((2, 7, 12), generator=gen).cuda()
    xyz, cen = torch.randn((2, 50, 3), generator=gen).cuda(), torch.randn((2, 7, 3), generator=gen).cuda() * 3     # 42 values: a tail
    for ks in ((0, 0, 0, 0), (1, 1, 1, 1), (1, 0, 2, 3)):
        for with_v in (True, False):
            ts = [at_offset(t, k) for t, k in zip((U, V, xyz, cen), ks)]
            part = torch.full((256,), float("nan"), dtype=torch.float32, device="cuda")
            call("l3d_absmax4_partials", ts[0], ts[0].numel(), ts[1] if with_v else None, ts[1].numel() if with_v else 0, ts[2], ts[2].numel(),
                 ts[3], ts[3].numel(), part)
            got = part.view(4, 64).max(dim=1)[0].cpu()
            want = torch.stack([t.abs().max() if (j != 1 or with_v) else torch.zeros((), device="cuda") for j, t in enumerate(ts)]).cpu()
            assert torch.equal(got, want), (ks, with_v)


def test_split_f16_images_are_the_same_for_a_misaligned_source():
    """l3d_split_f16_rows (channel-last) and l3d_split_f16_operand read a source row 16 bytes at a time when C % 4 == 0, the row stride
    % 4 == 0 and the tensor is 16-byte aligned (the alignment was not looked at before), by scalar loads otherwise: the image of a
    misaligned copy equals the aligned tensor's byte for byte (same values, same arithmetic).  Shape of test_conv_f16_accuracy's
    smallest case."""
    from learning3d_amd import _lib
    from learning3d_amd.models import _fused, _rows
    rng = np.random.default_rng(22)
    x = torch.from_numpy((np.maximum(rng.standard_normal((1, 256, 32)), 0) * 1e-3).astype(np.float32)).cuda()
    pb = _lib.lib().l3d_f16_image_bytes(0, 256, 32)                     # one plane
    written = lambda img: img[:2 * pb + 8]                               # h | m' planes, 2^-T, the maximum (then 8 bytes of scratch)
    want = _fused.split_rows_f16(x)
    for k in (1, 2):
        assert torch.equal(written(_fused.split_rows_f16(at_offset(x, k))), written(want))
    _fused.check_range(x.device, sync=True)
    x2 = x.reshape(256, 32)
    wide = torch.zeros((256, 40), device="cuda")
    wide[:, :32] = x2
    for kind in (0, 1):
        # kind 1 puts its two planes into slots 0 and 2 of a weight image and leaves slot 1 alone
        written = (lambda img: img) if kind == 0 else (lambda img: torch.cat([img[:pb], img[2 * pb:]]))
        want = written(_rows._operand(x2, kind))
        assert torch.equal(written(_rows._operand(at_offset(x2, 1), kind)), want)
        assert torch.equal(written(_rows._operand(at_offset(wide, 1)[:, :32], kind)), want)           # a row stride, misaligned
        assert torch.equal(written(_rows._operand(at_offset(wide, 0)[:, :32], kind)), want)


def test_attention_f16b_value_rows_and_maxima_pass_both_routes():
    """l3d_attention_forward_f16b: V's 8-key runs are two 16-byte loads when M % 8 == 0, the batch stride % 4 == 0 and v is 16-byte
    aligned (v_vec8), scalar loads otherwise; the pass over q, k, v for their maxima has the same choice per tensor.  The vector
    shape of test_flash_attention_vs_fp64, its neighbour M % 8 != 0, q / k / v at offset 0 and 1: rtol 1e-5, atol 2e-6 against fp64,
    and within 2x (max) / 1.5x (rms) of the bf16x3 kernel's own error, as there."""
    rng = np.random.default_rng(41)
    for (Bc, H, D, N, M) in [(2, 4, 128, 256, 256), (2, 4, 128, 256, 252)]:
        q = rng.standard_normal((Bc, H, D, N)).astype(np.float32)
        kk = rng.standard_normal((Bc, H, D, M)).astype(np.float32)
        v = rng.standard_normal((Bc, H, D, M)).astype(np.float32)
        s = np.einsum("bhdn,bhdm->bhnm", q.astype(np.float64), kk.astype(np.float64)) / np.sqrt(D)
        s = np.exp(s - s.max(axis=-1, keepdims=True))
        s /= s.sum(axis=-1, keepdims=True)
        want = np.einsum("bhdm,bhnm->bhdn", v.astype(np.float64), s)
        qd, kd, vd = [torch.from_numpy(t.reshape(Bc, H * D, -1)).cuda() for t in (q, kk, v)]
        out = torch.empty_like(qd)
        call("l3d_attention_forward_strided", qd, kd, vd, Bc, H, D, N, M, H * D * N, H * D * M, H * D * M, float(1 / np.sqrt(D)), out)
        e3 = out.cpu().numpy().reshape(Bc, H, D, N) - want
        for ks in ((0, 0, 0), (1, 1, 1), (0, 0, 1)):
            qa, ka, va = [at_offset(t, k) for t, k in zip((qd, kd, vd), ks)]
            ws = torch.zeros(4, dtype=torch.int32, device="cuda")
            outb = torch.empty_like(qd)
            call("l3d_attention_forward_f16b", qa, ka, va, Bc, H, D, N, M, H * D * N, H * D * M, H * D * M, float(1 / np.sqrt(D)), ws, 0, outb, None)
            assert np.array_equal(ws[:3].cpu().numpy().view(np.float32), [np.abs(q).max(), np.abs(kk).max(), np.abs(v).max()])
            gotb = outb.cpu().numpy().reshape(Bc, H, D, N)
            np.testing.assert_allclose(gotb, want, rtol=1e-5, atol=2e-6)
            eb = gotb - want
            assert np.abs(eb).max() <= 2.0 * np.abs(e3).max() + 1e-9 and np.sqrt((eb ** 2).mean()) <= 1.5 * np.sqrt((e3 ** 2).mean()) + 1e-10, \
                (M, ks, np.abs(eb).max(), np.abs(e3).max())


# ------------------------------------------------------------------------------------------------ class (c): the public ops
def test_layernorm_ops_take_a_misaligned_input():
    """l3d_layernorm_planes and l3d_layernorm_ref_backward refuse a misaligned x / a / b / g / dx; layer_norm_ref / _LayerNormRef and
    utils.transformer.LayerNorm copy such an operand first (both raised L3DError before): with autograd live y, dx, da, db -- and under
    no_grad y, with and without the fp16 plane image riding on it -- equal the aligned run's bit for bit (the same kernels on a copy)."""
    from learning3d_amd.utils.transformer import LayerNorm
    gen = torch.Generator().manual_seed(5)
    for shape in [(3, 77, 64), (1, 256, 64)]:
        ln = LayerNorm(shape[-1]).cuda()
        with torch.no_grad():
            ln.a_2.copy_(torch.randn(shape[-1], generator=gen) * 0.5 + 1.0)
            ln.b_2.copy_(torch.randn(shape[-1], generator=gen) * 0.3)
        x = (torch.randn(shape, generator=gen) * 2.0 + 0.7).cuda()
        w = torch.randn(shape, generator=gen).cuda()
        runs = []
        for k in (0, 1):
            xa = at_offset(x, k).detach().requires_grad_()
            ln.zero_grad()
            y = ln(xa)
            y.backward(at_offset(w, k))
            with torch.no_grad():
                y0 = ln(at_offset(x, k))
            img = getattr(y0, "_l3d_planes", None)                   # h | m' planes, 2^-T, then 12 bytes of scratch
            runs.append((y.detach(), xa.grad, ln.a_2.grad.clone(), ln.b_2.grad.clone(), y0, img[:-12] if img is not None else None))
        for a, b in zip(*runs):
            assert (a is None and b is None) or (same_bits(a, b) if a.dtype == torch.float32 else torch.equal(a, b))
        assert (runs[0][5] is not None) == (shape[1] % 256 == 0)
        x64 = x.double().requires_grad_()
        a64, b64 = ln.a_2.detach().double().requires_grad_(), ln.b_2.detach().double().requires_grad_()
        y64 = a64 * (x64 - x64.mean(-1, keepdim=True)) / (x64.std(-1, keepdim=True) + ln.eps) + b64
        (y64 * w.double()).sum().backward()
        for got, want in zip(runs[1][:4], (y64.detach(), x64.grad, a64.grad, b64.grad)):      # test_layernorm_hip_forward_backward_vs_fp64's bar
            assert float((got.double() - want).abs().max()) <= 1e-5 * float(want.abs().max())


def test_linear_rows_and_split_conv_take_a_misaligned_input():
    """l3d_linear_rows (x, w) and l3d_pointwise_conv_split (x) refuse a misaligned pointer; _fused.linear_rows, pointwise_conv's bf16x3
    route and pointwise_conv_maxpool's copy such an operand first: the aligned run's bits, and no L3DError."""
    from learning3d_amd.models import _fused
    rng = np.random.default_rng(88)
    lin = torch.nn.Linear(512, 40).cuda()
    x = torch.from_numpy(rng.standard_normal((70, 512)).astype(np.float32)).cuda()
    with torch.no_grad():
        want = _fused.linear_rows(x, lin, True)
        assert same_bits(_fused.linear_rows(at_offset(x, 1), lin, True), want)
    ref = torch.relu(x.double() @ lin.weight.detach().double().t() + lin.bias.detach().double())
    np.testing.assert_allclose(want.cpu().numpy(), ref.cpu().numpy(), rtol=1e-5, atol=1e-5 * float(ref.abs().max()))   # test_linear_rows_kernel's bar
    Bc, Cin, Cout, N = 1, 64, 256, 256
    xl = torch.from_numpy(np.maximum(rng.standard_normal((Bc, N, Cin)), 0).astype(np.float32)).cuda()
    w = torch.from_numpy((rng.standard_normal((Cout, Cin)) / np.sqrt(Cin)).astype(np.float32)).cuda()
    sc = torch.from_numpy(rng.uniform(0.5, 1.5, Cout).astype(np.float32)).cuda()
    sh = torch.from_numpy(rng.uniform(-0.5, 0.5, (Bc, Cout)).astype(np.float32)).cuda()
    xf = xl.transpose(1, 2).contiguous()
    assert _fused.split_eligible(Cin, Cout, N)
    want = _fused.pointwise_conv(xl, w, sc, sh, channel_last=True, split=True)
    for k in (1, 3):
        assert same_bits(_fused.pointwise_conv(at_offset(xl, k), at_offset(w, k), sc, sh, channel_last=True, split=True), want)
        assert same_bits(_fused.pointwise_conv(at_offset(xf, k), at_offset(w, k), sc, sh, split=True), want)
    pooled = _fused.pointwise_conv_maxpool(xf, w, sc, sh[0], True, 16)
    assert same_bits(_fused.pointwise_conv_maxpool(at_offset(xf, 1), w, sc, sh[0], True, 16), pooled)
    assert same_bits(pooled, _fused.pointwise_conv(xf, w, sc, sh[0], relu=True, split=True).view(Bc, Cout, N // 16, 16).max(dim=-1)[0])


def test_curve_walk_takes_a_misaligned_input(golden):
    """l3d_curve_walk reads the candidates' rows of x 16 bytes at a time and now refuses a misaligned x (it checked C % 16 only);
    curvenet_util.curve_walk copies such a tensor first: the aligned run's curves and paths."""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_curvenet_cpu import T, seeded_grouping, walk_case
    from learning3d_amd.utils.curvenet_util import curve_walk
    z, shape = walk_case(golden("curve_walk"), 0)
    grp = seeded_grouping(0, shape)[0].cuda()
    with torch.no_grad():
        x = T(z["x"]).cuda()
        xa = (x * torch.sigmoid(grp.att(x))).transpose(1, 2).contiguous()
        idx, start, params = T(z["idx"]).cuda(), T(z["start_run"]).cuda(), grp.walk.folded(x.device)
        curves, path = curve_walk(xa, idx, start, params, shape[5])
        curves1, path1 = curve_walk(at_offset(xa, 1), idx, start, params, shape[5])
    assert same_bits(curves1, curves) and torch.equal(path1, path)


def test_refusing_entry_points_refuse_a_misaligned_pointer():
    """one call each, with valid sizes and one misaligned pointer, of the entry points that read a caller's tensor 16 bytes at a time
    without a scalar route: L3D_ERR_UNSUPPORTED"""
    from learning3d_amd import _lib
    from learning3d_amd.models import _fused
    f = lambda *shape: torch.zeros(shape, dtype=torch.float32, device="cuda")
    mis = lambda *shape: at_offset(f(*shape), 1)
    # l3d_attention_forward_strided: v
    refused("l3d_attention_forward_strided", f(1, 32, 64), f(1, 32, 64), mis(1, 32, 64), 1, 1, 32, 64, 64, 2048, 2048, 2048, 1.0, f(1, 32, 64))
    # ... and a batch stride of v that is no multiple of 4
    refused("l3d_attention_forward_strided", f(1, 32, 64), f(1, 32, 64), f(1, 32, 64), 1, 1, 32, 64, 64, 2048, 2048, 2049, 1.0, f(1, 32, 64))
    # l3d_linear_rows: x, w
    refused("l3d_linear_rows", mis(2, 256), f(4, 256), None, 2, 256, 4, 0, f(2, 4))
    refused("l3d_linear_rows", f(2, 256), mis(4, 256), None, 2, 256, 4, 0, f(2, 4))
    # l3d_pointwise_conv_split: x
    w_split = _fused.split_rows(f(256, 16))
    refused("l3d_pointwise_conv_split", mis(1, 16, 128), 0, w_split, None, None, 0, 1, 16, 256, 128, 0, 0, f(1, 256, 128))
    # l3d_group_first_layer: U, V, out
    gfl = lambda U, V, out: refused("l3d_group_first_layer", U, V, None, f(4, 3), f(1, 8, 3), f(1, 2, 3), torch.zeros((1, 2, 2), dtype=torch.int32, device="cuda"),
                                    1, 8, 2, 2, 4, 1, out)
    gfl(mis(1, 8, 4), f(1, 2, 4), f(1, 4, 4))
    gfl(f(1, 8, 4), mis(1, 2, 4), f(1, 4, 4))
    gfl(f(1, 8, 4), f(1, 2, 4), mis(1, 4, 4))
    # l3d_group_first_layer_planes_auto (the same layer written as an fp16 plane image): U, V
    img = torch.zeros(_lib.lib().l3d_f16_image_bytes(1, 4, 64), dtype=torch.uint8, device="cuda")
    gfp = lambda U, V: refused("l3d_group_first_layer_planes_auto", U, V, None, f(64, 3), f(1, 8, 3), f(1, 2, 3),
                               torch.zeros((1, 2, 2), dtype=torch.int32, device="cuda"), 1, 8, 2, 2, 64, 1, f(256), 1.0, 0.0, img,
                               torch.zeros(1, dtype=torch.int32, device="cuda"))
    gfp(mis(1, 8, 64), f(1, 2, 64))
    gfp(f(1, 8, 64), mis(1, 2, 64))
    # l3d_sa_mlp3_fused: params
    # (3712 parameter floats for D = 0, (32, 32, 64): sa_fused.hip l3d_sa_mlp3_param_floats)
    refused("l3d_sa_mlp3_fused", f(1, 16, 3), f(1, 2, 3), None, torch.zeros((1, 2, 8), dtype=torch.int32, device="cuda"), mis(3712), 1, 16, 2, 8, 0,
            32, 32, 64, f(1, 64, 2))
    # l3d_layernorm_planes (values only): x, y, a, b
    for bad in range(4):
        t = [mis(4, 8) if bad == 0 else f(4, 8), mis(8) if bad == 1 else f(8), mis(8) if bad == 2 else f(8), mis(4, 8) if bad == 3 else f(4, 8)]
        refused("l3d_layernorm_planes", t[0], t[1], t[2], 1e-6, 4, 8, t[3], None)
    # l3d_layernorm_ref_backward: x, a, g, dx
    ws = f(_lib.lib().l3d_layernorm_backward_workspace_floats(4, 8))
    for bad in range(4):
        t = [mis(4, 8) if bad == 0 else f(4, 8), mis(8) if bad == 1 else f(8), mis(4, 8) if bad == 2 else f(4, 8), mis(4, 8) if bad == 3 else f(4, 8)]
        refused("l3d_layernorm_ref_backward", t[0], t[1], t[2], 1e-6, 4, 8, t[3], ws, f(8), f(8))
    # l3d_curve_walk: x
    i64 = lambda *shape: torch.zeros(shape, dtype=torch.int64, device="cuda")
    refused("l3d_curve_walk", mis(1, 8, 16), i64(1, 8, 2), i64(1, 2), 1, 8, 16, 2, 2, 2, f(32), f(1), f(1), f(64), f(2), f(2), f(1, 16, 2, 2),
            torch.zeros((1, 2, 2), dtype=torch.int32, device="cuda"))
