"""The f16x2 EdgeConv kernel (edgeconv_f16b.hip) across the hand-offs its schedule depends on: between layers, between a
workgroup's consecutive tiles (a persistent workgroup walks tiles with stride gridDim.x, prefetching the next tile's gather and
weight ring from inside layer 4), at a ragged last tile, and on a grid below one tile per CU.  A value that is parked, staged or
waited for correctly for a workgroup's first tile and wrongly for a later one (or the reverse) shows as a cloud that differs from
its copies; a wait state removed wrongly shows as wrong values, not as a fault.

Shapes: N = 256 with B = 40 (640 tiles over <= 256 workgroups: first, second and third tiles), N = 250 (ragged last tile: lanes
past N recompute point N-1), B = 3 with N = 64 (12 tiles: every workgroup runs one tile, nothing follows it); k = 20 / 18 / 16 / 12
= 5 row tiles, 5 with padded neighbours, 4, 4 padded; the three output forms (pooled fp32, fp16 planes, planes with an unscaled
residual).  Error bars are those of tests/test_gpu_parity.py (test_edgeconv_all_kernels_agree_and_ragged,
test_edgeconv_f16_planes_output_equals_pooled, test_edgeconv_f16_range_flag), restated here."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(40, 256), (5, 250), (3, 64)]
KS = [20, 18, 16, 12]


def _rand(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g)


@pytest.fixture(scope="module")
def net():
    from learning3d_amd.models import DGCNN
    torch.manual_seed(4)
    net = DGCNN(emb_dims=64).cuda().eval()
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.uniform_(-0.1, 0.1); m.running_var.uniform_(0.8, 1.2)
    return net


def _packed(net, device):
    packed = net._packed.get([net.conv1, net.conv2, net.conv3, net.conv4], [net.bn1, net.bn2, net.bn3, net.bn4], device)
    assert net._packed.v2_ok                                # the two-plane block is usable: "f16" IS edgeconv_f16b.hip
    return packed


def _decode(img, B, N):
    """The plane image -> (h plane, m plane as fp64 [64][B N][8], 2^-T_out)."""
    raw = img.cpu().numpy()
    pb = 64 * B * N * 16
    h = raw[:pb].view(np.float16).reshape(64, B * N, 8).astype(np.float64)
    m = raw[pb:2 * pb].view(np.float16).reshape(64, B * N, 8).astype(np.float64)
    return h, m, float(raw[2 * pb:2 * pb + 4].view(np.float32)[0])


def _fp64_and_fp32(net, x, idx):
    """dgcnn.py:32-46 on the given graph in fp64, and in plain fp32 by torch: [B][N][512] each."""
    from learning3d_amd.models import _fused
    B, N, k = idx.shape
    nb = torch.gather(x.unsqueeze(1).expand(B, N, N, 3), 2, idx.unsqueeze(-1).expand(B, N, k, 3))
    g32 = torch.cat([nb, x.unsqueeze(2).expand(B, N, k, 3)], dim=3).permute(0, 3, 1, 2).contiguous()
    res = []
    for h in (g32.double(), g32):
        outs = []
        for conv, bn in [(net.conv1, net.bn1), (net.conv2, net.bn2), (net.conv3, net.bn3), (net.conv4, net.bn4)]:
            w, sc, sh = _fused.fold_conv_bn(conv, bn)
            h = torch.relu(torch.einsum("oc,bcnk->bonk", w.to(h.dtype), h) * sc.to(h.dtype).view(1, -1, 1, 1) + sh.to(h.dtype).view(1, -1, 1, 1))
            outs.append(h.max(dim=-1)[0])
        res.append(torch.cat(outs, dim=1).permute(0, 2, 1).cpu().numpy())
    return res


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("B,N", SHAPES)
def test_tile_position_values_and_determinism(net, B, N, k):
    from learning3d_amd.models import _fused
    import learning3d_amd.utils as U
    one = _rand((1, N, 3), 1000 + N + k).cuda()
    with torch.no_grad():
        idx1 = U.knn(one.permute(0, 2, 1), k)
        x = one.expand(B, N, 3).contiguous()                # B copies of one cloud, each with that cloud's own indices
        idx = idx1.expand(B, N, k).contiguous()
        packed = _packed(net, x.device)
        forms = {}
        for name, kw in (("pooled", dict(kernel="f16")), ("planes", dict(planes=True)), ("unscaled", dict(planes=True, unscaled=True))):
            out = _fused.edgeconv_forward(x, idx, packed, v2=True, **kw)
            again = _fused.edgeconv_forward(x, idx, packed, v2=True, **kw)
            _fused.check_range(x.device, sync=True)         # magnitudes the packer was told of: the flag stays down
            used = out.numel() if name == "pooled" else 2 * 64 * B * N * 16 + 4      # the image: h | m planes, 2^-T_out; then padding
            assert torch.equal(out.view(-1)[:used], again.view(-1)[:used]), f"{name}: two calls differ"
            forms[name] = out
        lds = _fused.edgeconv_forward(one, idx1, packed, kernel="lds").cpu().numpy()       # the fp32-MFMA kernel, cloud 0 only
        want64, t32 = _fp64_and_fp32(net, one, idx1)

    # 1. tile position does not show: every cloud equals cloud 0 bit for bit, in all three forms
    pooled = forms["pooled"].cpu().numpy()
    for b in range(1, B):
        assert np.array_equal(pooled[b].view(np.uint32), pooled[0].view(np.uint32)), f"pooled: cloud {b} differs from cloud 0"
    dec = {}
    for name in ("planes", "unscaled"):
        h, m, xinv = _decode(forms[name], B, N)
        hb, mb = h.reshape(64, B, N, 8), m.reshape(64, B, N, 8)
        for b in range(1, B):
            assert np.array_equal(hb[:, b], hb[:, 0]) and np.array_equal(mb[:, b], mb[:, 0]), f"{name}: cloud {b} differs from cloud 0"
        dec[name] = (h, m, xinv)

    # 2. values: cloud 0 against fp64, held to the fp32 evaluations' own error (max <= 2x, rms <= 1.5x)
    got = pooled[:1]
    np.testing.assert_allclose(got, want64.astype(np.float32), rtol=1e-4, atol=1e-5)
    e_c = max(np.abs(lds - want64).max(), np.abs(t32 - want64).max())
    r_c = max(np.sqrt(((lds - want64) ** 2).mean()), np.sqrt(((t32 - want64) ** 2).mean()))
    e_s = np.abs(got - want64)
    print(f"f16x2 B={B} N={N} k={k}: max err {e_s.max():.3e} ({e_s.max() / e_c:.2f}x fp32), rms {np.sqrt((e_s ** 2).mean()):.3e} "
          f"({np.sqrt((e_s ** 2).mean()) / r_c:.2f}x)")
    assert e_s.max() <= 2.0 * e_c, (B, N, k, e_s.max(), e_c)
    assert np.sqrt((e_s ** 2).mean()) <= 1.5 * r_c, (B, N, k, np.sqrt((e_s ** 2).mean()), r_c)
    #    the plane images decode to the pooled output within the representation error of the split
    want = pooled.astype(np.float64)
    h, m, xinv = dec["planes"]
    assert np.log2(xinv) == np.round(np.log2(xinv))         # a power of two
    np.testing.assert_allclose(((h + m / 4096.0) * xinv).transpose(1, 0, 2).reshape(B, N, 512), want, rtol=2.0 ** -22,
                               atol=np.abs(want).max() * 2.0 ** -40)
    h2, m2, xinv2 = dec["unscaled"]
    assert xinv2 == xinv and np.array_equal(h2, h)          # the same h plane
    np.testing.assert_allclose(((h2 + m2) * xinv).transpose(1, 0, 2).reshape(B, N, 512), want, rtol=2.0 ** -22, atol=xinv * 2.0 ** -24)


@pytest.mark.parametrize("k", [20, 16])
def test_range_flag_in_every_output_form(net, k):
    """Coordinates 3e4 times larger than the BatchNorm statistics describe put layer 1's outputs beyond 60000 in plane units: the
    flag is raised in every output form (the guard's maxima sit on the pooled values' way out); the same clouds unscaled never
    raise it."""
    from learning3d_amd.models import _fused
    import learning3d_amd.utils as U
    x = _rand((2, 256, 3), 77).cuda()
    with torch.no_grad():
        idx = U.knn(x.permute(0, 2, 1), k)
        packed = _packed(net, x.device)
        for kw in (dict(kernel="f16"), dict(planes=True), dict(planes=True, unscaled=True)):
            _fused.edgeconv_forward(x, idx, packed, v2=True, **kw)
            _fused.check_range(x.device, sync=True)         # fine
            _fused.edgeconv_forward(x * 3.0e4, idx, packed, v2=True, **kw)
            with pytest.raises(_fused.L3DRangeError):
                _fused.check_range(x.device, sync=True)
            _fused.check_range(x.device, sync=True)         # the flag was cleared by the raise
