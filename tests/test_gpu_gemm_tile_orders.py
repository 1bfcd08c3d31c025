"""The three hand-written matrix-core GEMM families on the far side of the switches that pick their instantiation and their
workgroup-to-tile order -- the side the kernels' own unit tests (test_bmm_kernel_every_layout_vs_fp64, test_flash_attention_vs_fp64,
test_gpu_conv_f16_tail.py) do not reach.  Random inputs from seeded generators (no two tiles of an output agree), fp64 references,
the bars of those tests; every case first asserts the route it means to take, so a case that lands on the near side fails.

bmm.hip (through models/_rows.bmm; the route from l3d_bmm_f32_route, which shares bm_route() with l3d_bmm_f32):
  * YT: bm_route(), `wide >= 512 && N > 64` with wide = ceil(N / 128) ceil(M / 128) nb1 nb2 parts -- 128 x 128 workgroup tiles
    (bmm_f32_kernel<2, ..>) from 512 tiles on, 128 x 64 (<1, ..>) below.  Cases on both sides, YT = 2 with all nine (A, B) fetch forms
    of bm_mode() (16-byte loads along k, along the rows, scalar loads), ragged M / N / K, the epilogue flags and split K.
  * the tile order: bmm_f32_kernel, `(gridDim.y & 7) == 0` -- with a multiple of 8 row tiles the linear workgroup index is remapped
    (XCD = L & 7, slot = L >> 3).  16 and 8 row tiles (remapped) against 17 and 9 (not), for both YT.
attention_f16b.hip (l3d_attention_forward_f16b beside l3d_attention_forward_strided):
  * attention_f16b_kernel, `((gridDim.x / nq) & 7) == 0` with nq = ceil(N / AB_TQ) query blocks of 256: B H a multiple of 8 remaps the
    grid, and only N > 256 makes `slot % nq`, `slot / nq` more than the identity.  nq = 3 (ragged last block) and nq = 2.
conv_f16.hip (through _fused.pointwise_conv_f16(..., unscaled=True); the route from l3d_conv_f16_route):
  * cf_launch() / cf_tail_route(): Cin / 16 >= 5 runs conv_f16_tail_kernel, below that conv_f16_kernel<.., 2>'s chunk loop.
  * conv_f16_tail_kernel's tile order, `npt % 8 == 0` with npt = B N / 256 point tiles: 8 (remapped), 9 and 1 (not).
  * its ring: the tail's chunks sit in stages (nk - 3 + j) & 3 -- nk = 5, 6, 7, 8 are the four starting stages.
  * its epilogue addressing: clouds b > 0 in y's base and in a per-cloud shift (shift_bstride = Cout), scale / shift NULL.
  Every case also against the residual form with an all-zero residual (conv_f16_kernel<.., 2, RESID>: the chunk loop at any Cin),
  value for value: l3d_conv_f16_route.h's "both forms give the same bits"."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------------------------ bmm.hip
def _rnd(seed, *shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).cuda()


def _offset_by_one(t):
    """t's values in t's own memory order, in a view that starts one element into its storage: not 16-byte aligned"""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = flat[1:].as_strided(t.shape, t.stride())
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and torch.equal(v, t)
    return v


def _bmm_vs_fp64(name, x, y, route, ref=None):
    """test_bmm_kernel_every_layout_vs_fp64's bars: every element within the fp32 dot-product bound K 2^-24 (|a| . |b|) + 1e-30 of
    fp64, and the largest error at most 4x that of torch's own fp32 matmul + 1e-6 max|want|.  ref: (want, bound, torch's error)
    of operands with the same values, computed once."""
    from learning3d_amd.models import _rows
    assert _rows.bmm_route(x, y) == route, (name, _rows.bmm_route(x, y))
    got = _rows.bmm(x, y)
    if ref is None:
        want = torch.matmul(x.double(), y.double())
        bound = torch.matmul(x.double().abs(), y.double().abs()) * (x.shape[-1] * 2.0 ** -24) + 1e-30
        ref = (want, bound, float((torch.matmul(x, y).double() - want).abs().max()))
    want, bound, err_t = ref
    err = (got.double() - want).abs()
    bar = 4 * err_t + 1e-6 * float(want.abs().max())
    print(f"bmm {name}: route YT={route[0]} A={route[1]} B={route[2]} remapped={route[3]}: worst err / bound {float((err / bound).max()):.3f}, "
          f"max err {float(err.max()):.3e} = {float(err.max()) / bar:.3f} of the bar (torch {err_t:.3e})")
    assert bool((err <= bound).all()), (name, float((err / bound).max()))
    assert float(err.max()) <= bar, (name, float(err.max()), err_t)
    return got, ref


@pytest.mark.parametrize("nb,M,N,route", [
    pytest.param(4, 2045, 1019, (2, 0, 0, True), id="yt2-16-row-tiles-remapped"),       # 16 x 8 x 4 = 512 tiles
    pytest.param(4, 2100, 1019, (2, 0, 0, False), id="yt2-17-row-tiles-plain"),         # 17 x 8 x 4 = 544
    pytest.param(2, 1019, 130, (1, 0, 0, True), id="yt1-8-row-tiles-remapped"),         # 8 x 2 x 2 = 32 of the 128 x 128 kind: grid 3 x 8 x 2
    pytest.param(2, 1100, 130, (1, 0, 0, False), id="yt1-9-row-tiles-plain"),
])
def test_bmm_ragged_on_both_tiles_and_both_grid_orders(nb, M, N, route):
    """M, N and K off every tile edge (K = 19: one full chunk and a ragged one, scalar loads), more than one cloud."""
    _bmm_vs_fp64(f"ragged {nb} x {M} x {N} x 19", _rnd(M, nb, M, 19), _rnd(N + 1, nb, 19, N), route)


def test_bmm_yt2_all_nine_fetch_mode_pairs():
    """Batch 4, M 2048, N 1024, K 32 (512 tiles, remapped): the same values behind three layouts per operand.  The arithmetic per
    output element is one fma chain over ascending k whatever the loads were: all nine products have the same bits."""
    a, b = _rnd(31, 4, 2048, 32), _rnd(32, 4, 32, 1024)
    a_forms = {1: a,                                                      # k contiguous
               2: a.transpose(1, 2).contiguous().transpose(1, 2),         # a transposed view of [K, M]: rows contiguous
               0: _offset_by_one(a)}
    b_forms = {2: b,                                                      # [K, N] plain: as an [N rows x K] operand its rows are contiguous
               1: b.transpose(1, 2).contiguous().transpose(1, 2),         # a transposed view of [N, K]: k contiguous
               0: _offset_by_one(b)}
    ref, first = None, None
    for am, x in a_forms.items():
        for bm, y in b_forms.items():
            got, ref = _bmm_vs_fp64(f"fetch forms A {am} B {bm}", x, y, (2, am, bm, True), ref)
            first = got if first is None else first
            assert torch.equal(got.view(torch.int32), first.view(torch.int32)), (am, bm)


def test_bmm_yt2_epilogue_flags_and_strided_destination():
    """bias[n] + ReLU, bias[m] with alpha, accumulate and a strided destination on the 128 x 128 tile at the ragged, remapped shape;
    1e-5 max|want| as in test_bmm_kernel_every_layout_vs_fp64."""
    from learning3d_amd.models import _rows
    nb, M, N, K = 4, 2045, 1019, 19
    x, y = _rnd(41, nb, M, K), _rnd(42, nb, K, N)
    assert _rows.bmm_route(x, y) == (2, 0, 0, True)
    prod = torch.matmul(x.double(), y.double())

    def held(what, got, want):
        err, bar = float((got.double() - want).abs().max()), 1e-5 * float(want.abs().max())
        print(f"bmm YT=2 epilogue, {what}: max err {err:.3e} = {err / bar:.3f} of the bar")
        assert err <= bar, (what, err, bar)

    bn, bm_ = _rnd(43, N), _rnd(44, M)
    held("bias[n] + ReLU", _rows.bmm(x, y, bias=bn, relu=True), torch.relu(prod + bn.double()))
    held("bias[m], alpha 0.5", _rows.bmm(x, y, bias=bm_, bias_axis="m", alpha=0.5), 0.5 * prod + bm_.double()[:, None])
    acc = _rnd(45, nb, M, N)
    want = acc.double() + prod
    _rows.bmm(x, y, out=acc, accumulate=True)
    held("accumulate", acc, want)
    wide = torch.zeros((nb, M, N + 81), device="cuda")
    _rows.bmm(x, y, out=wide[:, :, 40:40 + N])
    held("strided destination", wide[:, :, 40:40 + N], prod)
    assert float(wide[:, :, :40].abs().max()) == 0 and float(wide[:, :, 40 + N:].abs().max()) == 0


def test_bmm_yt2_split_k():
    """M = N = 1024, K = 300 in 8 parts: 64 tiles x 8 = 512, so the partial products run on the 128 x 128 tile (8 row tiles: remapped;
    19 chunks over 8 parts: three per part, the last part with one ragged chunk and one part empty)."""
    from learning3d_amd.models import _rows
    a, b = _rnd(51, 1024, 300), _rnd(52, 300, 1024)
    assert _rows.bmm_route(a, b, parts=8) == (2, 0, 0, True) and _rows.bmm_route(a, b) == (1, 0, 0, True)
    want = a.double() @ b.double()
    r1, r2 = _rows.bmm(a, b, parts=8), _rows.bmm(a, b, parts=8)
    assert torch.equal(r1.view(torch.int32), r2.view(torch.int32))
    err, bar = float((r1.double() - want).abs().max()), 2e-5 * float(want.abs().max())
    print(f"bmm YT=2 split K, 8 parts: max err {err:.3e} = {err / bar:.3f} of the bar")
    assert err <= bar, (err, bar)


# ------------------------------------------------------------------------------------------------------- attention_f16b.hip
@pytest.mark.parametrize("B,H,D,N,M,image", [(2, 4, 32, 600, 100, True), (4, 4, 64, 512, 333, False)])
def test_attention_f16b_remapped_grid_with_several_query_blocks(B, H, D, N, M, image):
    """test_flash_attention_vs_fp64's operands and bars (rtol 1e-5 / atol 2e-6 against fp64; max error <= 2x, rms <= 1.5x the bf16x3
    kernel's own) where the remapped workgroup order is more than the identity."""
    from learning3d_amd._lib import lib, check, ptr, stream_ptr
    # the kernel's grid is nq B H workgroups, nq = ceil(N / 256): `((gridDim.x / nq) & 7) == 0` is (B H) % 8 == 0, and the remapped
    # (query block, group) = (slot % nq, (slot / nq) 8 + xcd) differs from the plain (L % nq, L / nq) only when nq > 1
    nq = -(-N // 256)
    assert (B * H) % 8 == 0 and N > 256 and nq in (2, 3)
    rng = np.random.default_rng(1000 * N + M)
    q = rng.standard_normal((B, H, D, N)).astype(np.float32)
    k = rng.standard_normal((B, H, D, M)).astype(np.float32)
    v = rng.standard_normal((B, H, D, M)).astype(np.float32)
    s = np.einsum("bhdn,bhdm->bhnm", q.astype(np.float64), k.astype(np.float64)) / np.sqrt(D)
    s = np.exp(s - s.max(axis=-1, keepdims=True))
    s /= s.sum(axis=-1, keepdims=True)
    want = np.einsum("bhdm,bhnm->bhdn", v.astype(np.float64), s)
    qd, kd, vd = dev(q.reshape(B, H * D, N)), dev(k.reshape(B, H * D, M)), dev(v.reshape(B, H * D, M))
    out = torch.empty_like(qd)
    check(lib().l3d_attention_forward_strided(ptr(qd), ptr(kd), ptr(vd), B, H, D, N, M, H * D * N, H * D * M, H * D * M,
                                              float(1 / np.sqrt(D)), ptr(out), stream_ptr()), "l3d_attention_forward_strided")
    ws = torch.zeros(4, dtype=torch.int32, device=qd.device)
    outb = torch.empty_like(qd)
    imgb = torch.empty(lib().l3d_f16_image_bytes(1, B * N, H * D), dtype=torch.uint8, device=qd.device)
    check(lib().l3d_attention_forward_f16b(ptr(qd), ptr(kd), ptr(vd), B, H, D, N, M, H * D * N, H * D * M, H * D * M,
                                           float(1 / np.sqrt(D)), ptr(ws), 0, ptr(outb), ptr(imgb) if image else None, stream_ptr()),
          "l3d_attention_forward_f16b")
    got3, gotb = out.cpu().numpy().reshape(B, H, D, N), outb.cpu().numpy().reshape(B, H, D, N)
    e3, eb = got3 - want, gotb - want
    tol = 2e-6 + 1e-5 * np.abs(want)
    print(f"attention_f16b B H = {B * H}, nq = {nq} (N {N}, M {M}, D {D}): worst err / (atol + rtol |want|) {(np.abs(eb) / tol).max():.3f}, "
          f"max err {np.abs(eb).max():.3e} ({np.abs(eb).max() / np.abs(e3).max():.2f}x bf16x3), "
          f"rms {np.sqrt((eb ** 2).mean()):.3e} ({np.sqrt((eb ** 2).mean()) / np.sqrt((e3 ** 2).mean()):.2f}x)")
    np.testing.assert_allclose(got3, want, rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(gotb, want, rtol=1e-5, atol=2e-6)
    assert np.abs(eb).max() <= 2.0 * np.abs(e3).max() + 1e-9 and np.sqrt((eb ** 2).mean()) <= 1.5 * np.sqrt((e3 ** 2).mean()) + 1e-10, \
        (np.abs(eb).max(), np.abs(e3).max())
    if image:                                              # the plane image of the same context, decoded as test_flash_attention_vs_fp64 does
        raw = imgb.cpu().numpy()
        pb = (H * D // 8) * B * N * 16
        ph = raw[:pb].view(np.float16).reshape(H * D // 8, B * N, 8).astype(np.float64)
        pm = raw[pb:2 * pb].view(np.float16).reshape(H * D // 8, B * N, 8).astype(np.float64)
        xinv = float(raw[2 * pb:2 * pb + 4].view(np.float32)[0])
        dec = ((ph + pm / 4096.0) * xinv).transpose(1, 0, 2).reshape(B, N, H * D).transpose(0, 2, 1).reshape(B, H, D, N)
        np.testing.assert_allclose(dec, gotb.astype(np.float64), rtol=2.0 ** -21, atol=np.abs(gotb).max() * 2.0 ** -30)


# ------------------------------------------------------------------------------------------------ conv_f16.hip: conv5's tail
_CONV = {}


def _conv_case(B, N, Cout, Cin, scale, shift):
    """inputs, images, the fp64 product and the fp32-MFMA kernel's outputs of one case, made once.  shift: None, "co" ([Cout]) or
    "b,co" (one per cloud: shift_bstride = Cout)"""
    key = (B, N, Cout, Cin, scale, shift)
    if key not in _CONV:
        from learning3d_amd.models import _fused, _rows
        rng = np.random.default_rng(100000 * B + 100 * N + Cin)
        x = np.maximum(rng.standard_normal((B, N, Cin)), 0).astype(np.float32)                    # post-ReLU like
        w = (rng.standard_normal((Cout, Cin)) / np.sqrt(Cin)).astype(np.float32)
        sc = rng.uniform(0.5, 1.5, Cout).astype(np.float32) if scale else None
        sh = rng.uniform(-0.5, 0.5, (B, Cout) if shift == "b,co" else Cout).astype(np.float32) if shift else None
        want = np.einsum("oc,bnc->bon", w.astype(np.float64), x.astype(np.float64))               # [B, Cout, N]
        if scale:
            want = want * sc[None, :, None]
        if shift:
            want = want + (sh[:, :, None] if shift == "b,co" else sh[None, :, None])
        d = dict(x=dev(x), w=dev(w), sc=dev(sc) if scale else None, sh=dev(sh) if shift else None,
                 want={False: want, True: np.maximum(want, 0)})
        d["xi"], d["wi"] = _rows._operand(d["x"].reshape(B * N, Cin), 0), _fused.split_weights_f16(d["w"])
        d["f32"] = {r: _fused.pointwise_conv(d["x"], d["w"], d["sc"], d["sh"], relu=r, channel_last=True, split=False).cpu().numpy()
                    for r in (False, True)}
        _CONV[key] = d
    return _CONV[key]


def _tail_case(B, N, Cout, Cin, relu, scale=True, shift="b,co"):
    """(a) per cloud against fp64: max error <= 2x, rms <= 1.5x the fp32-MFMA kernel's own on that cloud (test_gpu_conv_f16_tail.py's
    bar); (b) a second call gives equal bits; (c) the residual form -- the chunk loop -- with an all-zero residual gives equal
    values (residual + act(v) turns a -0 into +0: compared as floats, not as bits)."""
    from learning3d_amd import _lib
    from learning3d_amd.models import _fused
    route = _lib.lib().l3d_conv_f16_route(Cin, Cout, N, _lib.L3D_CONV_F16_TWO_PLANE)
    assert route == (_lib.L3D_CONV_F16_ROUTE_TAIL if Cin >= 80 else _lib.L3D_CONV_F16_ROUTE_LOOP), (Cin, route)
    c = _conv_case(B, N, Cout, Cin, scale, shift)

    def run(**kw):
        y = _fused.pointwise_conv_f16(c["xi"], B, N, c["wi"], Cin, Cout, c["sc"], c["sh"], relu=relu, unscaled=True, **kw)
        _fused.check_range(y.device, sync=True)
        return y

    y = run()
    got, want, f32 = y.cpu().numpy(), c["want"][relu], c["f32"][relu]
    assert got.shape == (B, Cout, N)
    worst_max = worst_rms = 0.0
    for b in range(B):
        es, e32 = np.abs(got[b] - want[b]), np.abs(f32[b] - want[b])
        rs, r32 = np.sqrt((es ** 2).mean()), np.sqrt((e32 ** 2).mean())
        worst_max, worst_rms = max(worst_max, es.max() / (2.0 * e32.max())), max(worst_rms, rs / (1.5 * r32))
    npt = B * (N // 256)
    print(f"two-plane conv B={B} N={N} Cout={Cout} Cin={Cin} (nk {Cin // 16}) relu={relu} scale={scale} shift={shift}: route "
          f"{'tail' if route else 'loop'}, {npt} point tiles ({'remapped' if npt % 8 == 0 else 'plain order'}); worst cloud: max err "
          f"{worst_max:.3f} of its bar, rms {worst_rms:.3f} of its bar")
    for b in range(B):
        es, e32 = np.abs(got[b] - want[b]), np.abs(f32[b] - want[b])
        assert es.max() <= 2.0 * e32.max() + 1e-30, (b, es.max(), e32.max())
        assert np.sqrt((es ** 2).mean()) <= 1.5 * np.sqrt((e32 ** 2).mean()), (b, np.sqrt((es ** 2).mean()), np.sqrt((e32 ** 2).mean()))
    assert torch.equal(y.view(torch.int32), run().view(torch.int32))
    yres = run(residual=torch.zeros((B, Cout, N), device=y.device))
    differ = int((y != yres).sum())
    assert differ == 0, f"{differ} of {y.numel()} values differ between the plain two-plane form and the residual form"


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("Cin", [64, 80, 96, 112, 128])
def test_conv_tail_every_ring_position_under_the_remapped_grid(Cin, relu):
    """B 2, N 1024, Cout 512: 8 point tiles x 2 channel tiles, remapped; the second cloud's rows, outputs and shift.  Cin 64 stays on the
    loop; nk = 5, 6, 7, 8 start the tail's three chunks at stages 2, 3, 0, 1."""
    assert (2 * (1024 // 256)) % 8 == 0
    _tail_case(2, 1024, 512, Cin, relu)


@pytest.mark.parametrize("relu", [False, True])
def test_conv_tail_plain_grid_order_with_more_than_eight_tiles(relu):
    """B 3, N 768, Cout 256: 9 point tiles, the plain order; three clouds with a shift each."""
    assert (3 * (768 // 256)) % 8 == 1
    _tail_case(3, 768, 256, 112, relu)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("scale,shift", [(False, "co"), (True, None), (False, None)])
def test_conv_tail_null_scale_and_shift(scale, shift, relu):
    """scale == NULL, shift == NULL and both (one workgroup: B 1, N 256, Cout 256, Cin 80)"""
    _tail_case(1, 256, 256, 80, relu, scale=scale, shift=shift)
