"""The tile-major tail of conv_f16.hip's plain two-plane form (DGCNN's conv5) on the GPU, through _fused.pointwise_conv_f16 on a
two-plane image: the last L3D_CONV_F16_TAIL_CHUNKS K chunks run MFMA tile by MFMA tile and every tile is stored as it becomes final.
K chunks below, at and just above the tail's entry condition (TAIL + 2 = 5 chunks, Cin = 80) and conv5's own K; one workgroup tile
(N 256, Cout 256) and four (N 512, Cout 512)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(256, 256), (512, 512)]                  # (N, Cout), B = 1
CINS = [16, 48, 64, 80, 96, 512]
_CASES = {}


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _planes(x2d, w):
    """x [rows, Cin] -> a two-plane activation image (unscaled residual), w [Cout, Cin] -> a weight image"""
    from learning3d_amd.models import _fused, _rows
    return _rows._operand(x2d, 0), _fused.split_weights_f16(w)


def _conv(x, w, sc, sh, relu):
    from learning3d_amd.models import _fused
    N, Cin = x.shape
    Cout = w.shape[0]
    xi, wi = _planes(x, w)
    y = _fused.pointwise_conv_f16(xi, 1, N, wi, Cin, Cout, sc, sh, relu=relu, unscaled=True)
    _fused.check_range(x.device, sync=True)
    return y


def _case(N, Cout, Cin):
    """inputs, the fp64 product and the fp32-MFMA kernel's outputs of one shape, made once"""
    key = (N, Cout, Cin)
    if key not in _CASES:
        from learning3d_amd.models import _fused
        rng = np.random.default_rng(1000 * N + Cin)
        x = np.maximum(rng.standard_normal((N, Cin)), 0).astype(np.float32)                    # post-ReLU like
        w = (rng.standard_normal((Cout, Cin)) / np.sqrt(Cin)).astype(np.float32)
        sc = rng.uniform(0.5, 1.5, Cout).astype(np.float32)                                    # a scale and a shift of its own for every row
        sh = rng.uniform(-0.5, 0.5, Cout).astype(np.float32)
        want = (w.astype(np.float64) @ x.astype(np.float64).T) * sc[:, None] + sh[:, None]     # [Cout, N]
        d = dict(x=dev(x), w=dev(w), sc=dev(sc), sh=dev(sh), want={False: want, True: np.maximum(want, 0)})
        d["f32"] = {r: _fused.pointwise_conv(d["x"][None], d["w"], d["sc"], d["sh"], relu=r, channel_last=True, split=False)[0].cpu().numpy()
                    for r in (False, True)}
        _CASES[key] = d
    return _CASES[key]


def _route(Cin, Cout, N):
    from learning3d_amd import _lib
    return _lib.lib().l3d_conv_f16_route(Cin, Cout, N, _lib.L3D_CONV_F16_TWO_PLANE)


@pytest.mark.parametrize("N,Cout", SHAPES)
def test_route_boundary(N, Cout):
    """Cin < 16 (TAIL + 2) stays on the chunk loop; from there on the plain two-plane call takes the tail.  Other flag sets never do."""
    from learning3d_amd import _lib
    assert _lib.L3D_CONV_F16_TAIL_CHUNKS == 3
    for Cin in CINS:
        want = _lib.L3D_CONV_F16_ROUTE_TAIL if Cin >= 16 * (_lib.L3D_CONV_F16_TAIL_CHUNKS + 2) else _lib.L3D_CONV_F16_ROUTE_LOOP
        assert _route(Cin, Cout, N) == want, Cin
        assert _lib.lib().l3d_conv_f16_route(Cin, Cout, N, 0) == _lib.L3D_CONV_F16_ROUTE_LOOP
        assert _lib.lib().l3d_conv_f16_route(Cin, Cout, N, _lib.L3D_CONV_F16_TWO_PLANE | _lib.L3D_CONV_F16_SHIFT_N) == _lib.L3D_CONV_F16_ROUTE_LOOP
    assert _lib.lib().l3d_conv_f16_route(72, Cout, N, _lib.L3D_CONV_F16_TWO_PLANE) == _lib.L3D_ERR_UNSUPPORTED
    assert _lib.lib().l3d_conv_f16_route(0, Cout, N, 0) == _lib.L3D_ERR_INVALID_ARG


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("Cin", CINS)
@pytest.mark.parametrize("N,Cout", SHAPES)
def test_accuracy_scale_shift_relu_and_determinism(N, Cout, Cin, relu):
    """Against the fp64 product of the same fp32 inputs: max error <= 2x, rms <= 1.5x the fp32-MFMA kernel's own (the bar of
    test_gpu_parity.py::test_conv_f16_accuracy), with a per-row scale and shift, with and without ReLU; two calls give equal bits."""
    c = _case(N, Cout, Cin)
    y = _conv(c["x"], c["w"], c["sc"], c["sh"], relu)
    got = y[0].cpu().numpy()
    assert got.shape == (Cout, N)
    es, e32 = np.abs(got - c["want"][relu]), np.abs(c["f32"][relu] - c["want"][relu])
    rs, r32 = np.sqrt((es ** 2).mean()), np.sqrt((e32 ** 2).mean())
    print(f"two-plane conv N={N} Cout={Cout} Cin={Cin} relu={relu} route {_route(Cin, Cout, N)}: max err {es.max():.3e} "
          f"({es.max() / e32.max():.2f}x fp32-MFMA), rms {rs:.3e} ({rs / r32:.2f}x)")
    assert es.max() <= 2.0 * e32.max() + 1e-30, (es.max(), e32.max())
    assert rs <= 1.5 * r32, (rs, r32)
    again = _conv(c["x"], c["w"], c["sc"], c["sh"], relu)
    assert torch.equal(y.view(torch.int32), again.view(torch.int32))


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("N,Cout", SHAPES)
def test_same_bits_on_both_sides_of_the_route_boundary(N, Cout, relu):
    """Cin = 80 with sixteen zero channels behind 64 real ones (the tail) against Cin = 64 on those (the loop): the zero products add
    +0 to sums that are positive (weights > 0, activations >= 0 with a positive one in every row), so every bit must agree."""
    from learning3d_amd import _lib
    rng = np.random.default_rng(7 + N)
    x64 = np.maximum(rng.standard_normal((N, 64)), 0).astype(np.float32)
    x64[:, 0] = rng.uniform(0.5, 1.0, N).astype(np.float32)
    w64 = rng.uniform(0.01, 1.0, (Cout, 64)).astype(np.float32)
    x80 = np.concatenate([x64, np.zeros((N, 16), np.float32)], axis=1)
    w80 = np.concatenate([w64, w64[:, :16]], axis=1)           # the added weights change no row's maximum, so no row's exponent
    assert (w80 > 0).all() and (x80 >= 0).all() and (x64.max(axis=1) > 0).all() and not np.signbit(x80).any()
    sc = rng.uniform(0.5, 1.5, Cout).astype(np.float32)
    sh = (-rng.uniform(0.0, 0.8, Cout) * w64.sum(axis=1)).astype(np.float32)   # a good part of the outputs below zero: ReLU has work to do
    assert _route(64, Cout, N) == _lib.L3D_CONV_F16_ROUTE_LOOP and _route(80, Cout, N) == _lib.L3D_CONV_F16_ROUTE_TAIL
    y64 = _conv(dev(x64), dev(w64), dev(sc), dev(sh), relu)
    y80 = _conv(dev(x80), dev(w80), dev(sc), dev(sh), relu)
    assert torch.equal(y64.view(torch.int32), y80.view(torch.int32))
    neg = float((y64 == 0).float().mean()) if relu else float((y64 < 0).float().mean())
    assert 0.05 < neg < 0.95, neg
