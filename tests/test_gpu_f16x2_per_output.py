"""f16x2 kernels held to fp32-level error PER OUTPUT GROUP (an output channel of a conv, an output row of a rows-as-weights product),
with magnitudes spread inside one scale group -- what a global max-error bar cannot see (tests/test_f16x2_shared_exponent_model.py
has the arithmetic).  Per group g, against fp64 and against the fp32-MFMA kernel (or l3d_bmm_f32) on the same inputs:
  max |e| <= 2 max |e32| + floor_g,   rms e <= 1.5 rms e32 + floor_g,   floor_g = 2^-24 max_j (|scale_g| sum_k |w_gk x_kj| + |shift_g|)
Inputs: weight rows x 10^U(-4, 0), BatchNorm-folded scales over 10^4, points x 10^U(-6, 0), gradient rows x 10^U(-6, 0); edges: a row
whose maximum is exactly a power of two and one a ulp below it, an all-zero row, an all-zero tensor, a tensor whose maximum is 1e-36."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TINY = 2.0 ** -24


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def per_group(name, got, want, f32, floor):
    """got / want / f32 [G, ...] (group first), floor [G]: assert the per-group bar, print the worst ratios against fp32"""
    G = got.shape[0]
    e = np.abs(got.reshape(G, -1).astype(np.float64) - want.reshape(G, -1))
    e32 = np.abs(f32.reshape(G, -1).astype(np.float64) - want.reshape(G, -1))
    assert np.all(np.isfinite(got)), name
    emax, e32max = e.max(axis=1), e32.max(axis=1)
    erms, e32rms = np.sqrt((e ** 2).mean(axis=1)), np.sqrt((e32 ** 2).mean(axis=1))
    floor = floor + 2.0 ** -149                                                  # fp32's subnormal spacing: no fp32 result resolves less
    rmax = emax / (2.0 * e32max + floor)
    rrms = erms / (1.5 * e32rms + floor)
    worst = int(rmax.argmax())
    live = e32max > 0
    vs32 = (emax[live] / e32max[live]).max() if live.any() else 0.0
    print(f"{name}: worst group max-error {rmax.max():.3f} of the bar (group {worst}), rms {rrms.max():.3f}; "
          f"worst max-error ratio against fp32 {vs32:.2f}x")
    assert rmax.max() <= 1.0, (name, worst, emax[worst], e32max[worst], floor[worst])
    assert rrms.max() <= 1.0, (name, int(rrms.argmax()))


def spread_weights(rng, Cout, Cin):
    w = rng.standard_normal((Cout, Cin)) / np.sqrt(Cin) * 10.0 ** rng.uniform(-4, 0, (Cout, 1))
    w = w.astype(np.float32)
    w[5] = 0.0                                                                   # an all-zero row beside non-zero ones
    for r, top in ((6, np.float32(2.0 ** -7)), (7, np.nextafter(np.float32(2.0 ** -7), np.float32(0)))):
        w[r] = w[r] / np.abs(w[r]).max() * np.float32(0.5) * top
        w[r, 3] = top                                                            # the row's maximum: a power of two / a ulp below
    return w


def bn_fold(rng, Cout):
    """BatchNorm (eval) folded to (scale, shift) with gamma / sqrt(var + eps) over 10^4"""
    gamma = rng.uniform(0.5, 1.5, Cout) * 10.0 ** rng.uniform(-2, 0, Cout)
    var = 10.0 ** rng.uniform(-4, 0, Cout)
    scale = (gamma / np.sqrt(var + 1e-5)).astype(np.float32)
    shift = (rng.uniform(-0.1, 0.1, Cout) * scale * 1e-3).astype(np.float32)
    return scale, shift


def decode_image(img, rows, C, unscaled):
    """an activation image (h | m planes [C/8][rows][8] + 2^-T) -> [rows][C] float64"""
    from learning3d_amd._lib import lib
    pb = lib().l3d_f16_image_bytes(0, rows, C)
    raw = img.cpu().numpy()
    h = raw[:pb].view(np.float16).reshape(C // 8, rows, 8).transpose(1, 0, 2).reshape(rows, C).astype(np.float64)
    m = raw[pb:2 * pb].view(np.float16).reshape(C // 8, rows, 8).transpose(1, 0, 2).reshape(rows, C).astype(np.float64)
    inv = float(raw[2 * pb:2 * pb + 4].view(np.float32)[0])
    return (h + (m if unscaled else m * 2.0 ** -12)) * inv, inv


def image_split(vmax, oinv, unscaled):
    """what an activation image adds to a value of magnitude <= vmax: 22 bits, and half the residual plane's subnormal step"""
    return 2.0 ** -22 * vmax + (2.0 ** -25 if unscaled else 2.0 ** -37) * oinv


CONV_CASES = [
    # (B, Cin, Cout, N, x kind)
    (2, 256, 512, 512, "spread"),
    (1, 64, 256, 256, "spread"),
    (1, 128, 256, 256, "zero"),
    (1, 128, 256, 256, "tiny"),
]


def conv_inputs(rng, B, Cin, Cout, N, kind):
    x = np.maximum(rng.standard_normal((B, N, Cin)), 0) * 10.0 ** rng.uniform(-6, 0, (B, N, 1))
    if kind == "zero":
        x = np.zeros_like(x)
    elif kind == "tiny":
        x = x / x.max() * 1e-36                                                  # largest |x| 1e-36: 2^T beyond 2^127 unclamped
    w = spread_weights(rng, Cout, Cin)
    sc, sh = bn_fold(rng, Cout)
    if kind == "tiny":
        sh[:] = 0.0                                                              # the product itself is checked, not the shift
    return x.astype(np.float32), w, sc, sh


def conv_reference(x, w, sc, sh):
    """fp64 y [B][Cout][N] and the floor per channel"""
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    want = np.einsum("oc,bnc->bon", w64, x64) * sc[None, :, None] + sh[None, :, None]
    mag = np.einsum("oc,bnc->bon", np.abs(w64), np.abs(x64)) * np.abs(sc)[None, :, None] + np.abs(sh)[None, :, None]
    return want, TINY * mag.max(axis=(0, 2))


@pytest.mark.parametrize("B,Cin,Cout,N,kind", CONV_CASES)
def test_pointwise_conv_f16_per_channel(B, Cin, Cout, N, kind):
    """l3d_pointwise_conv_f16: three-plane (channel-last and channel-first splits), two-plane, plane output (both residual forms),
    pooled epilogue -- each channel against the fp32-MFMA kernel's error on that channel"""
    from learning3d_amd.models import _fused, _rows
    rng = np.random.default_rng(1000 + Cin + N + len(kind))
    x, w, sc, sh = conv_inputs(rng, B, Cin, Cout, N, kind)
    want, floor = conv_reference(x, w, sc, sh)
    xd, wd, scd, shd = dev(x), dev(w), dev(sc), dev(sh)
    f32 = _fused.pointwise_conv(xd, wd, scd, shd, channel_last=True, split=False).cpu().numpy()
    g = lambda a: np.ascontiguousarray(np.moveaxis(a, 1, 0))                     # [B,Cout,N] -> [Cout,B,N]: channel first
    wimg = _fused.split_weights_f16(wd)
    y3 = _fused.pointwise_conv_f16(_fused.split_rows_f16(xd), B, N, wimg, Cin, Cout, scd, shd).cpu().numpy()
    per_group(f"conv f16x2 three-plane {kind} {Cin}->{Cout}", g(y3), g(want), g(f32), floor)
    xcf = dev(np.ascontiguousarray(x.transpose(0, 2, 1)))
    ycf = _fused.pointwise_conv_f16(_fused.split_rows_f16(xcf, channel_first=True), B, N, wimg, Cin, Cout, scd, shd).cpu().numpy()
    np.testing.assert_array_equal(ycf, y3)                                       # same planes, same products, same order
    x2 = _rows._operand(xd.view(B * N, Cin), 0)                                  # unscaled residual plane: the two-plane form
    y2 = _fused.pointwise_conv_f16(x2, B, N, wimg, Cin, Cout, scd, shd, unscaled=True).cpu().numpy()
    per_group(f"conv f16x2 two-plane {kind} {Cin}->{Cout}", g(y2), g(want), g(f32), floor)
    # plane outputs: the output image holds y to fp32-level error per channel too (one more rounding: the output split)
    for unscaled, img_in in ((False, _fused.split_rows_f16(xd)), (True, x2)):
        img = _fused.pointwise_conv_f16(img_in, B, N, wimg, Cin, Cout, scd, shd, out_planes=True, unscaled=unscaled)
        yo, oinv = decode_image(img, B * N, Cout, unscaled)
        yo = yo.reshape(B, N, Cout).transpose(0, 2, 1)
        # one more rounding, the output's own split (one exponent for the image): 22 bits of each value, and half a subnormal step of the
        # residual plane -- 2^-25 plane units unscaled, 2^-37 with the 2^12-scaled residual
        split = image_split(np.abs(want).max(axis=(0, 2)), oinv, unscaled)
        per_group(f"conv f16x2 plane output {'two' if unscaled else 'three'}-plane {kind}", g(yo), g(want), g(f32), floor + split)
    if N % 128 == 0:
        _, pooled = _fused.pointwise_conv_f16_pool(_fused.split_rows_f16(xd), B, N, wimg, Cin, Cout, scd, shd, pool=True)
        e32 = np.abs(f32 - want).max(axis=(0, 2))
        ep = np.abs(pooled.cpu().numpy().astype(np.float64) - want.max(axis=2)).max(axis=0)
        assert np.all(ep <= 2.0 * e32 + floor), ("pool", int((ep / (2.0 * e32 + floor + 1e-300)).argmax()))
    _fused.check_range(xd.device, sync=True)


def test_fold_mlp_f16_spread_w6_rows():
    """PCN's folding decoder (fold_mlp_f16.hip) with W6 rows x 10^U(-4, 0) and an all-zero row: every fine point within the bf16x3
    kernel's own error (per point) plus the floor"""
    from learning3d_amd._lib import check, lib, ptr, stream_ptr
    from learning3d_amd.models import _fused
    rng = np.random.default_rng(78)
    B, N = 2, 600
    g = rng.standard_normal((B, N, 5)).astype(np.float32)
    w5g = (rng.standard_normal((512, 5)) * 0.5).astype(np.float32)
    s5 = rng.standard_normal((B, 512)).astype(np.float32)
    w6 = spread_weights(rng, 512, 512)
    b6 = (rng.standard_normal(512) * 0.01).astype(np.float32)
    w7 = (rng.standard_normal((3, 512)) / 512 ** 0.5 * 10.0 ** rng.uniform(-2, 2, 512)).astype(np.float32)
    b7 = rng.standard_normal(3).astype(np.float32)
    ce = rng.standard_normal((B, N, 3)).astype(np.float32)
    h5 = np.maximum(s5[:, None, :].astype(np.float64) + g.astype(np.float64) @ w5g.astype(np.float64).T, 0)
    h6 = np.maximum(h5 @ w6.astype(np.float64).T + b6, 0)
    want = h6 @ w7.astype(np.float64).T + b7 + ce
    # the floor carried through conv7: 2^-24 sum_co |W7_j,co| (sum_k |W6_co,k h5_k| + |b6_co|), the conv6 GEMM's own floor per channel
    mag = (np.abs(h5) @ np.abs(w6.astype(np.float64)).T + np.abs(b6)) @ np.abs(w7.astype(np.float64)).T + np.abs(b7) + np.abs(ce)
    dv = {k: dev(v) for k, v in dict(g=g, w5g=w5g, s5=s5, w6=w6, b6=b6, w7=w7, b7=b7, ce=ce).items()}
    outs = {}
    for name, fn, wimg in (("bf16x3", lib().l3d_fold_mlp, _fused.split_rows(dv["w6"])),
                           ("f16x2", lib().l3d_fold_mlp_f16, _fused.split_weights_f16(dv["w6"]))):
        out = torch.empty((B, N, 3), dtype=torch.float32, device="cuda")
        check(fn(ptr(dv["g"]), 5, ptr(dv["w5g"]), ptr(dv["s5"]), ptr(wimg), ptr(dv["b6"]), ptr(dv["w7"]), ptr(dv["b7"]),
                 ptr(dv["ce"]), B, N, ptr(out), stream_ptr()), name)
        outs[name] = out.cpu().numpy()
    pts = lambda a: a.reshape(B * N, 3)
    per_group("fold_mlp f16x2 (vs bf16x3) per point", pts(outs["f16x2"]), pts(want), pts(outs["bf16x3"]), TINY * pts(mag).max(axis=1))


@pytest.mark.parametrize("kind", ["spread", "tiny"])
def test_rows_linear_f16x2_per_row(kind):
    """models/_rows.linear forward (rows of x as the weight operand, l3d_split_f16_operand kind 1) and its dgrad (gradient rows as the
    weight operand) on the f16x2 route, per output row, against the same products on l3d_bmm_f32 (TRAIN_GEMM = fp32)"""
    from learning3d_amd import _lib
    from learning3d_amd.models import _rows
    rng = np.random.default_rng(90 + len(kind))
    R, Cin, Cout = 4096, 256, 512
    x = rng.standard_normal((R, Cin)) * 10.0 ** rng.uniform(-6, 0, (R, 1))
    gr = rng.standard_normal((R, Cout)) * 10.0 ** rng.uniform(-6, 0, (R, 1))
    x[11] = 0.0
    gr[12] = 0.0
    x[13] = x[13] / np.abs(x[13]).max() * 0.5
    x[13, 0] = 1.0                                                                # row maximum exactly a power of two
    x[14] = x[14] / np.abs(x[14]).max() * 0.5
    x[14, 0] = np.nextafter(np.float32(1.0), np.float32(0))
    if kind == "tiny":
        x, gr = x / np.abs(x).max() * 1e-36, gr / np.abs(gr).max() * 1e-36
        b0 = 0.0                                                                  # the product itself is checked, not the bias
    else:
        b0 = 1e-3
    x, gr = x.astype(np.float32), gr.astype(np.float32)
    lin = torch.nn.Linear(Cin, Cout).cuda()
    with torch.no_grad():
        lin.weight.copy_(dev((rng.standard_normal((Cout, Cin)) / 16).astype(np.float32)))
        lin.bias.copy_(dev((rng.standard_normal(Cout) * b0).astype(np.float32)))
    w64, b64 = lin.weight.detach().double().cpu().numpy(), lin.bias.detach().double().cpu().numpy()

    def run(route):
        old = _rows.TRAIN_GEMM
        _rows.TRAIN_GEMM = route
        _lib.LAUNCH_LOG = []
        try:
            xt = dev(x).requires_grad_()
            y = _rows.linear(xt, lin)
            y.backward(dev(gr))
            return y.detach().cpu().numpy(), xt.grad.cpu().numpy(), list(_lib.LAUNCH_LOG)
        finally:
            _rows.TRAIN_GEMM = old
            _lib.LAUNCH_LOG = None

    y16, gx16, log = run("f16x2")
    assert log.count("l3d_pointwise_conv_f16[rows]") == 2, log                   # forward and dgrad took the f16x2 route
    y32, gx32, log32 = run("fp32")
    assert "l3d_pointwise_conv_f16[rows]" not in log32
    x64, g64 = x.astype(np.float64), gr.astype(np.float64)
    want_y = x64 @ w64.T + b64
    floor_y = TINY * (np.abs(x64) @ np.abs(w64).T + np.abs(b64)).max(axis=1)
    per_group(f"rows linear f16x2 forward ({kind})", y16, want_y, y32, floor_y)
    want_gx = g64 @ w64
    floor_gx = TINY * (np.abs(g64) @ np.abs(w64)).max(axis=1)
    per_group(f"rows linear f16x2 dgrad ({kind})", gx16, want_gx, gx32, floor_gx)


# --------------------------------------------------------------------------- producers of activation images, EdgeConv, attention, kNN

@pytest.mark.parametrize("kind", ["spread", "tiny"])
def test_first_layer_f16_planes_per_channel(kind):
    """l3d_first_layer_f16_planes (Cin 3 -> 128 written straight as an activation image, one exponent for the image): weight rows x 10^U(-4, 0)
    and an all-zero row; 'tiny': coordinates of 1e-36 and no shift (the clamped exponent).  Decoded per channel against fp64 and the
    fp32-MFMA conv, with the image's own resolution (image_split) on top of the bar."""
    from learning3d_amd.models import _fused
    rng = np.random.default_rng(120 + len(kind))
    B, N, Cout = 2, 512, 128
    x = rng.uniform(-1, 1, (B, N, 3)) * (1e-36 if kind == "tiny" else 1.0)
    w = (rng.standard_normal((Cout, 3)) * 10.0 ** rng.uniform(-4, 0, (Cout, 1))).astype(np.float32)
    w[5] = 0.0
    sh = np.zeros(Cout, np.float32) if kind == "tiny" else (rng.standard_normal(Cout) * 1e-3).astype(np.float32)
    x = x.astype(np.float32)
    for channel_last in (True, False):
        xd = dev(x if channel_last else np.ascontiguousarray(x.transpose(0, 2, 1)))
        img = _fused.first_layer_f16_planes(xd, dev(w), dev(sh), True, channel_last)
        f32 = _fused.pointwise_conv(xd, dev(w), None, dev(sh), relu=True, channel_last=channel_last, split=False).cpu().numpy()
        pre = np.einsum("oc,bnc->bon", w.astype(np.float64), x.astype(np.float64)) + sh[None, :, None]
        want = np.maximum(pre, 0)
        floor = TINY * (np.einsum("oc,bnc->bon", np.abs(w.astype(np.float64)), np.abs(x.astype(np.float64))) + np.abs(sh)[None, :, None]).max(axis=(0, 2))
        yo, oinv = decode_image(img, B * N, Cout, False)
        yo = yo.reshape(B, N, Cout).transpose(0, 2, 1)
        g = lambda a: np.ascontiguousarray(np.moveaxis(a, 1, 0))
        per_group(f"first_layer_f16_planes {kind} channel_last={channel_last}", g(yo), g(want), g(f32),
                  floor + image_split(want.max(axis=(0, 2)), oinv, False))
    _fused.check_range(sync=True)


@pytest.mark.parametrize("kind", ["spread", "tiny", "offset"])
def test_group_first_layer_planes_per_channel(kind):
    """l3d_group_first_layer_planes_auto (FlowNet3D's factored first layer, act(U[idx] + shift + Wx (xyz[idx] - centre)) as an activation
    image): U channels x 10^U(-4, 0), Wx rows x 10^U(-4, 0); 'tiny': every input 1e-36, no shift; 'offset': points and centres moved by
    (1000, -50, 3), so the image's scale, taken from max|xyz| + max|new_xyz|, is a thousand times the coordinate differences it holds
    (the bar follows that scale through oinv).  Per channel against fp64 and the fp32 kernel (l3d_group_first_layer)."""
    from learning3d_amd._lib import check, lib, ptr, stream_ptr
    from learning3d_amd.models import _fused
    rng = np.random.default_rng(130 + len(kind))
    B, N, S, K, C1 = 2, 300, 64, 16, 128
    f = 1e-36 if kind == "tiny" else 1.0
    U = (rng.standard_normal((B, N, C1)) * 10.0 ** rng.uniform(-4, 0, (1, 1, C1)) * f).astype(np.float32)
    wx = (rng.standard_normal((C1, 3)) * 10.0 ** rng.uniform(-4, 0, (C1, 1))).astype(np.float32)
    sh = np.zeros(C1, np.float32) if kind == "tiny" else (rng.standard_normal(C1) * 1e-3).astype(np.float32)
    xyz = (rng.uniform(-1, 1, (B, N, 3)) * f).astype(np.float32)
    if kind == "offset":
        xyz = xyz + np.array([1000.0, -50.0, 3.0], np.float32)
    ctr = xyz[:, :S].copy()
    idx = rng.integers(0, N, (B, S, K)).astype(np.int32)
    Ud, wxd, shd, xd, cd, idd = dev(U), dev(wx), dev(sh), dev(xyz), dev(ctr), dev(idx)
    part = torch.empty(256, dtype=torch.float32, device="cuda")
    check(lib().l3d_absmax4_partials(ptr(Ud), Ud.numel(), None, 0, ptr(xd), xd.numel(), ptr(cd), cd.numel(), ptr(part), stream_ptr()), "absmax4")
    wxr = float(np.abs(wx).sum(axis=1).max())
    img = torch.empty(lib().l3d_f16_image_bytes(1, B * S * K, C1), dtype=torch.uint8, device="cuda")
    check(lib().l3d_group_first_layer_planes_auto(ptr(Ud), None, ptr(shd), ptr(wxd), ptr(xd), ptr(cd), ptr(idd), B, N, S, K, C1, 1, ptr(part),
                                                  wxr, float(np.abs(sh).max()), ptr(img), ptr(_fused.range_flag(Ud.device)), stream_ptr()),
          "l3d_group_first_layer_planes_auto")
    out = torch.empty((B, S * K, C1), dtype=torch.float32, device="cuda")
    check(lib().l3d_group_first_layer(ptr(Ud), None, ptr(shd), ptr(wxd), ptr(xd), ptr(cd), ptr(idd), B, N, S, K, C1, 1, ptr(out), stream_ptr()),
          "l3d_group_first_layer")
    _fused.check_range(sync=True)
    bi = np.arange(B)[:, None, None]
    d = (xyz[bi, idx].astype(np.float64) - ctr[:, :, None, :].astype(np.float64)).reshape(B, S * K, 3)
    ug = U[bi, idx].reshape(B, S * K, C1).astype(np.float64)
    want = np.maximum(ug + sh + d @ wx.astype(np.float64).T, 0)
    floor = TINY * (np.abs(ug) + np.abs(sh) + np.abs(d) @ np.abs(wx.astype(np.float64)).T).max(axis=(0, 1))
    yo, oinv = decode_image(img, B * S * K, C1, False)
    g = lambda a: np.ascontiguousarray(a.reshape(-1, C1).T)
    per_group(f"group_first_layer_planes {kind}", g(yo), g(want), g(out.cpu().numpy()),
              floor + image_split(want.max(axis=(0, 1)), oinv, False))


def test_layernorm_planes_then_conv_per_channel():
    """l3d_layernorm_planes' activation image (LayerNorm gain a over 10^U(-4, 0) per channel) into the three-plane conv with spread weight rows:
    each conv output channel against fp64 and against the fp32 LayerNorm values through the fp32-MFMA conv"""
    from learning3d_amd._lib import check, lib, ptr, stream_ptr
    from learning3d_amd.models import _fused
    rng = np.random.default_rng(140)
    rows, C, Cout = 1024, 256, 256
    x = (rng.standard_normal((rows, C)) * 3 + 1).astype(np.float32)
    a = (rng.uniform(0.5, 1.5, C) * 10.0 ** rng.uniform(-4, 0, C)).astype(np.float32)
    b = (rng.standard_normal(C) * 1e-4).astype(np.float32)
    w = spread_weights(rng, Cout, C)
    xd, ad, bd = dev(x), dev(a), dev(b)
    y = torch.empty_like(xd)
    img = torch.empty(lib().l3d_f16_image_bytes(1, rows, C), dtype=torch.uint8, device="cuda")
    check(lib().l3d_layernorm_planes(ptr(xd), ptr(ad), ptr(bd), 1e-6, rows, C, ptr(y), ptr(img), stream_ptr()), "l3d_layernorm_planes")
    x64 = x.astype(np.float64)
    ln = a * (x64 - x64.mean(1, keepdims=True)) / (x64.std(1, ddof=1, keepdims=True) + 1e-6) + b
    want = ln @ w.astype(np.float64).T                                             # [rows, Cout]
    floor = TINY * (np.abs(ln) @ np.abs(w.astype(np.float64)).T).max(axis=0)
    got = _fused.pointwise_conv_f16(img, 1, rows, _fused.split_weights_f16(dev(w)), C, Cout).cpu().numpy()[0]       # [Cout, rows]
    f32 = _fused.pointwise_conv(y.view(1, rows, C), dev(w), channel_last=True, split=False).cpu().numpy()[0]
    per_group("layernorm_planes -> conv f16x2", got, want.T, f32, floor)


@pytest.mark.xfail(strict=True, reason="EdgeConv layers 2-4 keep one static exponent per layer with the BatchNorm scale folded into the "
                                       "weights: measured 38x over the per-channel bar (rms 61x), 1033x the fp32 kernel's error on the worst "
                                       "channel; per-channel exponents at pack time (mlp.hip) are not built yet")
def test_edgeconv_f16b_per_channel():
    """DGCNN's EdgeConv stack on the f16x2 kernel (l3d_edgeconv_forward_f16b: layers 2-4 with the BatchNorm scale folded into the weights,
    one static exponent per layer) with BatchNorm statistics that spread the folded scales over 10^4 within each layer: every output
    channel of the [B, N, 512] result against fp64 and against the fp32-MFMA kernel and torch's fp32 evaluation (the larger error)"""
    from learning3d_amd.models import DGCNN, _fused
    import learning3d_amd.utils as U
    torch.manual_seed(5)
    rng = np.random.default_rng(150)
    net = DGCNN(emb_dims=64).cuda().eval()
    with torch.no_grad():
        for bn in (net.bn2, net.bn3, net.bn4):
            n = bn.num_features
            bn.running_var.copy_(dev(10.0 ** rng.uniform(-2, 2, n)).float())
            bn.weight.copy_(dev(rng.uniform(0.5, 1.5, n) * 10.0 ** rng.uniform(-1, 1, n)).float())
            bn.running_mean.uniform_(-0.01, 0.01)
    B, N, k = 2, 1024, 20
    x = dev(rng.uniform(0, 1, (B, N, 3)).astype(np.float32))
    with torch.no_grad():
        idx = U.knn(x.permute(0, 2, 1), k)
        packed = net._packed.get([net.conv1, net.conv2, net.conv3, net.conv4], [net.bn1, net.bn2, net.bn3, net.bn4], x.device)
        assert net._packed.v2_ok, "the f16x2 kernel must take this stack"
        f16 = _fused.edgeconv_forward(x, idx, packed, kernel="f16", v2=True).cpu().numpy()
        f32 = _fused.edgeconv_forward(x, idx, packed, kernel="lds").cpu().numpy()
        _fused.check_range(x.device, sync=True)
        nb = torch.gather(x.unsqueeze(1).expand(B, N, N, 3), 2, idx.unsqueeze(-1).expand(B, N, k, 3))
        h = torch.cat([nb, x.unsqueeze(2).expand(B, N, k, 3)], dim=3).permute(0, 3, 1, 2).double()
        h32 = h.float()
        outs, outs32, floors = [], [], []
        for conv, bn in [(net.conv1, net.bn1), (net.conv2, net.bn2), (net.conv3, net.bn3), (net.conv4, net.bn4)]:
            w, sc, sh = _fused.fold_conv_bn(conv, bn)
            mag = torch.einsum("oc,bcnk->bonk", w.double().abs(), h.abs()) * sc.double().abs().view(1, -1, 1, 1) + sh.double().abs().view(1, -1, 1, 1)
            floors.append(TINY * mag.amax(dim=(0, 2, 3)))
            h = torch.relu(torch.einsum("oc,bcnk->bonk", w.double(), h) * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1))
            h32 = torch.relu(torch.einsum("oc,bcnk->bonk", w, h32) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))
            outs.append(h.max(dim=-1)[0])
            outs32.append(h32.max(dim=-1)[0])
        want = torch.cat(outs, dim=1).permute(0, 2, 1).cpu().numpy()
        t32 = torch.cat(outs32, dim=1).permute(0, 2, 1).cpu().numpy()
        floor = torch.cat(floors).cpu().numpy()
    # control: whichever fp32 evaluation is further from fp64 on the channel
    worse32 = np.where(np.abs(f32 - want).max(axis=(0, 1)) >= np.abs(t32 - want).max(axis=(0, 1)), 0, 1)
    ctrl = np.where(worse32[None, None, :] == 0, f32, t32)
    g = lambda a: np.ascontiguousarray(a.reshape(-1, a.shape[-1]).T)
    per_group("edgeconv f16x2 (layers 2-4 static exponents)", g(f16), g(want), g(ctrl), floor)


@pytest.mark.xfail(strict=True, reason="one exponent per q / k / v tensor: measured 1.06x over the per-query bar on the worst query "
                                       "(3.4x the bf16x3 kernel's error there); per-token exponents are not built yet")
def test_attention_f16b_per_query():
    """l3d_attention_forward_f16b with q, k, v tokens spread x 10^U(-3, 0) inside their one tensor exponent: every query's context vector
    against fp64 and against the bf16x3 kernel (l3d_attention_forward_strided)"""
    from learning3d_amd._lib import check, lib, ptr, stream_ptr
    rng = np.random.default_rng(160)
    B, H, D, N, M = 2, 4, 64, 256, 384
    q = rng.standard_normal((B, H, D, N)) * 10.0 ** rng.uniform(-3, 0, (B, 1, 1, N))
    k = rng.standard_normal((B, H, D, M)) * 10.0 ** rng.uniform(-3, 0, (B, 1, 1, M))
    v = rng.standard_normal((B, H, D, M)) * 10.0 ** rng.uniform(-3, 0, (B, 1, 1, M))
    q, k, v = (a.astype(np.float32) for a in (q, k, v))
    sc = 1.0 / np.sqrt(D)
    s = np.einsum("bhdn,bhdm->bhnm", q.astype(np.float64), k.astype(np.float64)) * sc
    p = np.exp(s - s.max(axis=-1, keepdims=True))
    p /= p.sum(axis=-1, keepdims=True)
    want = np.einsum("bhdm,bhnm->bhdn", v.astype(np.float64), p)
    # floor: 2^-24 of sum_m p |v| (the product) plus the scores' own fp32 rounding carried through the softmax, |s| 2^-24 sum_m p |v - out|
    mag = np.einsum("bhdm,bhnm->bhdn", np.abs(v.astype(np.float64)), p)
    smag = np.einsum("bhdn,bhdm->bhnm", np.abs(q.astype(np.float64)), np.abs(k.astype(np.float64))) * sc
    spread = np.einsum("bhnm,bhnm,bhdm->bhdn", smag, p, np.abs(v.astype(np.float64)))
    qd, kd, vd = dev(q.reshape(B, H * D, N)), dev(k.reshape(B, H * D, M)), dev(v.reshape(B, H * D, M))
    ref = torch.empty_like(qd)
    check(lib().l3d_attention_forward_strided(ptr(qd), ptr(kd), ptr(vd), B, H, D, N, M, H * D * N, H * D * M, H * D * M, float(sc), ptr(ref),
                                              stream_ptr()), "l3d_attention_forward_strided")
    out = torch.empty_like(qd)
    ws = torch.zeros(4, dtype=torch.int32, device=qd.device)
    check(lib().l3d_attention_forward_f16b(ptr(qd), ptr(kd), ptr(vd), B, H, D, N, M, H * D * N, H * D * M, H * D * M, float(sc), ptr(ws), 0,
                                           ptr(out), None, stream_ptr()), "l3d_attention_forward_f16b")
    g = lambda a: np.ascontiguousarray(np.moveaxis(a.reshape(B, H, D, N), 2, 3).reshape(-1, D))       # one group per (b, h, query)
    floor = TINY * (mag + 2 * spread).max(axis=2).reshape(-1)
    per_group("attention f16x2 per query", g(out.cpu().numpy()), g(want), g(ref.cpu().numpy()), floor)


def test_feature_knn_per_query_tolerance():
    """utils.knn on feature maps (featknn.hip: f16x2 GEMM with one exponent per 128-row tile) with one outlier point x 10^3 in every tile:
    each query's k-th returned distance within a per-query tolerance built from its own |x_i|^2 and its k-th neighbour's |x_j|^2 (16 fp32
    ulps), instead of one tolerance from the cloud's largest |x|^2"""
    from learning3d_amd.utils import knn
    rng = np.random.default_rng(170)
    B, C, N, k = 2, 64, 1024, 20
    x = rng.standard_normal((B, C, N)) * 10.0 ** rng.uniform(-1, 0, (B, 1, N))
    x[:, :, ::128] *= 1e3
    x = x.astype(np.float32)
    idx = knn(dev(x), k).cpu().numpy()
    xd = x.astype(np.float64)
    sq = (xd ** 2).sum(axis=1)
    d = sq[:, :, None] + sq[:, None, :] - 2 * np.einsum("bci,bcj->bij", xd, xd)
    order = np.argsort(d, axis=-1, kind="stable")
    kth = np.take_along_axis(d, order[:, :, k - 1:k], axis=-1)[..., 0]
    sq_kth = np.take_along_axis(sq[:, None, :].repeat(N, 1), order[:, :, k - 1:k], axis=-1)[..., 0]
    got = np.take_along_axis(d, idx, axis=-1)
    sq_got = np.take_along_axis(sq[:, None, :].repeat(N, 1), idx, axis=-1).max(axis=-1)
    tol = 16 * TINY * (sq + np.maximum(sq_kth, sq_got))
    excess = (got.max(axis=-1) - kth) / tol
    print(f"featknn per query: worst k-th distance excess {excess.max():.3f} of the per-query tolerance "
          f"(the global one, 4e-6 max|x|^2, is {4e-6 * sq.max() / tol.min():.0f}x the smallest per-query one)")
    assert np.all(excess <= 1.0), (np.unravel_index(excess.argmax(), excess.shape), excess.max())
    assert np.all(np.diff(got, axis=-1) >= -tol[..., None]), "ascending within the per-query tolerance"
