"""Every op at its kernel's size limit, one past it and well past it, through the public Python functions.

Each kernel's C entry point refuses the shapes it cannot take (L3D_ERR_UNSUPPORTED); the Python wrapper must route those shapes
somewhere else and still compute the same thing.  Checked against a plain high-precision (or bit-exact) reference of the op:

* feature-space knn (l3d_knn_feature: N <= 16384; past it the reference's op sequence a block of queries at a time) against fp64
  distances of 512 seeded query rows, with the criteria of test_gpu_parity.test_knn_feature_space_matches_exact_topk;
* farthest / furthest point sampling (register-resident kernel up to 512 x 32 points, the temp-array kernel past it) bit for bit
  against the oracle's restatements of both tie rules (the reference's own kernel: test_gpu_ref_kernels.py);
* the deterministic scatter behind grouping / gather / three_interpolate / index_points backward (l3d_scatter_add_det: T * ranges
  < 2^22, windows of targets past it) bit for bit against np.add.at in float32 -- the header's "ascending e in fp32" -- and
  the same bits on a second run;
* _rows.linear with an expanded output gradient (a sum over rows backpropagated from a [Cout] vector: strides (0, 1)) against
  fp64 autograd;
* _rows.linear after the library rewrote its input through a raw pointer (no stale f16 image of the rows);
* l3d_edge_gather_max (N <= 32768) bit for bit against the torch expression, and PRNet's DGCNN past it.

Cost on one MI355X, measured with `pytest tests -m gpu -k "limits or fps_ties or fps_equals"` (this file and the FPS tests of
test_gpu_ref_kernels.py): 86 tests in 4.9 s, peak torch.cuda.max_memory_allocated() 3.6 GiB.
Tolerances are written where they are applied."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def rand(shape, seed, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * (hi - lo) + lo).numpy()


class launch_log:
    def __enter__(self):
        from learning3d_amd import _lib
        self.lib = _lib
        _lib.LAUNCH_LOG = []
        return _lib.LAUNCH_LOG

    def __exit__(self, *exc):
        self.lib.LAUNCH_LOG = None
        return False


def _rel(a, b):
    """max |a - b| over the scale max |b| (both numpy, b the fp64 truth)"""
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


# --------------------------------------------------------------------------------------------- feature-space kNN
@pytest.mark.parametrize("N", [16384, 16385, 20000])
@pytest.mark.parametrize("C,k", [(64, 20), (64, 64), (9, 20), (9, 64)])
def test_knn_feature_space_across_the_kernel_limit(C, k, N):
    from learning3d_amd.utils import knn
    B = 2 if N == 16385 else 1
    rng = np.random.default_rng(N * 7 + C + k)
    x = rng.standard_normal((B, C, N)).astype(np.float32)
    with launch_log() as log:
        idx = knn(dev(x), k).cpu().numpy()
    assert ("l3d_knn_feature" in log) == (N <= 16384), log
    assert idx.shape == (B, N, k) and idx.dtype == np.int64
    q = np.unique(np.concatenate([rng.choice(N, 509, replace=False), [0, 16383, N - 1]]))   # 512 query rows (and the edges)
    xd = x.astype(np.float64)
    sq = (xd ** 2).sum(axis=1)                                                     # [B,N]
    for b in range(B):
        d = sq[b, q][:, None] + sq[b][None, :] - 2 * xd[b][:, q].T @ xd[b]           # [512,N] fp64
        kth = np.partition(d, k - 1, axis=-1)[:, k - 1]
        got = np.take_along_axis(d, idx[b, q], axis=-1)
        tol = 4e-6 * sq.max()                                                      # as test_knn_feature_space_matches_exact_topk
        assert np.all(got.max(axis=-1) <= kth + tol), (C, k, N, b)
        assert np.all(np.diff(got, axis=-1) >= -tol), (C, k, N, b)
        assert np.all(idx[b, q, 0] == q)                                            # self first
        srt = np.sort(idx[b, q], axis=-1)
        assert np.all(srt[:, 1:] != srt[:, :-1])                                    # no repeats


def test_graph_feature_one_past_the_feature_knn_limit():
    from learning3d_amd.utils import get_graph_feature
    B, C, N = 2, 64, 16385
    x = dev(np.random.default_rng(5).standard_normal((B, C, N)).astype(np.float32))
    f = get_graph_feature(x, k=20)
    assert f.shape == (B, 2 * C, N, 20)
    assert torch.equal(f[:, C:], x[:, :, :, None].expand(B, C, N, 20))            # the centre half is x itself


# --------------------------------------------------------------------------------------------- farthest point sampling
FPS_N = [16384, 16385, 24577, 32768, 32769, 65536, 262144]


@pytest.mark.parametrize("N", FPS_N)
@pytest.mark.parametrize("cloud", ["uniform", "ties"])
def test_fps_both_variants_across_the_register_limit(N, cloud):
    """uniform clouds, and N(0,1) clipped to [-1,1] (duplicated corner points: ties in the early rounds, resolved by each variant's
    own rule -- lowest index for the torch twin, the pointnet2 kernel's block tree for pointnet2_utils)"""
    import oracle
    from learning3d_amd.utils import farthest_point_sample
    from learning3d_amd.utils import pointnet2_utils as P
    B, m = (3 if N <= 32769 else 2), 64
    if cloud == "uniform":
        x = rand((B, N, 3), N, -1, 1)
    else:
        x = np.clip(np.random.default_rng(N).standard_normal((B, N, 3)), -1.0, 1.0).astype(np.float32)
    xyz = dev(x)
    got32 = P.furthest_point_sample(xyz, m)
    got64 = farthest_point_sample(xyz, m, start_with_first_point=True)
    assert got32.dtype == torch.int32 and got64.dtype == torch.int64
    assert np.array_equal(got32.cpu().numpy(), oracle.furthest_point_sampling(x, m)), (N, cloud)
    assert np.array_equal(got64.cpu().numpy(), oracle.farthest_point_sample(x, m)), (N, cloud)


# --------------------------------------------------------------------------------------------- deterministic scatter
def _add_at(vals_ce, idx_e, T):
    """the contract of l3d_scatter_add_det: every target's contributions in ascending entry order, in fp32"""
    out = np.zeros((vals_ce.shape[0], T), np.float32)
    for c in range(vals_ce.shape[0]):
        np.add.at(out[c], idx_e, vals_ce[c])
    return out


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def test_gather_backward_at_2_to_the_22_targets():
    """T = 2^22 with 1024 entries: the old guard let it through and target 2^22 - 1 at lane 1023 sorted as padding"""
    from learning3d_amd.utils import pointnet2_utils as P
    T, S, C = 1 << 22, 1024, 2
    rng = np.random.default_rng(22)
    idx = rng.integers(0, T, (1, S)).astype(np.int32)
    idx[0, 1023] = T - 1
    idx[0, [0, 17, 511, 1000]] = T - 1
    go = rng.standard_normal((1, C, S)).astype(np.float32)
    want = _add_at(go[0], idx[0], T)
    runs = []
    for _ in range(2):
        feat = torch.zeros((1, C, T), device="cuda", requires_grad=True)
        P.gather_operation(feat, dev(idx)).backward(dev(go))
        runs.append(feat.grad.cpu().numpy()[0])
    assert _bits_equal(runs[0], want) and _bits_equal(runs[1], runs[0])
    assert runs[0][:, T - 1].any()


@pytest.mark.parametrize("T,npoint,nsample", [(524289, 1024, 8), (524288, 1024, 8), (524287, 1024, 8)])
def test_grouping_backward_past_the_scatter_limit(T, npoint, nsample):
    """E = 8192 entries -> eight placement ranges: the kernel takes T * 8 < 2^22, i.e. T <= 524287"""
    from learning3d_amd.utils import pointnet2_utils as P
    C = 2
    rng = np.random.default_rng(T)
    idx = rng.integers(0, T, (1, npoint, nsample)).astype(np.int32)
    idx[0, -1, -1] = T - 1
    idx[0, :4, :2] = T - 1
    idx[0, 5, :] = 0
    go = rng.standard_normal((1, C, npoint, nsample)).astype(np.float32)
    want = _add_at(go[0].reshape(C, -1), idx[0].reshape(-1), T)
    runs = []
    for _ in range(2):
        feat = torch.zeros((1, C, T), device="cuda", requires_grad=True)
        P.grouping_operation(feat, dev(idx)).backward(dev(go))
        runs.append(feat.grad.cpu().numpy()[0])
    assert _bits_equal(runs[0], want) and _bits_equal(runs[1], runs[0])


def test_three_interpolate_backward_past_the_scatter_limit():
    """m = 2^21 + 1 known points, n = 700 queries (E = 2100: two ranges, T * 2 >= 2^22)"""
    from learning3d_amd.utils import pointnet2_utils as P
    B, C, m, n = 2, 3, (1 << 21) + 1, 700
    rng = np.random.default_rng(31)
    idx = rng.integers(0, m, (B, n, 3)).astype(np.int32)
    idx[:, -1, :] = m - 1
    w = rng.uniform(0, 1, (B, n, 3)).astype(np.float32)
    go = rng.standard_normal((B, C, n)).astype(np.float32)
    runs = []
    for _ in range(2):
        feat = torch.zeros((B, C, m), device="cuda", requires_grad=True)
        P.three_interpolate(feat, dev(idx), dev(w)).backward(dev(go))
        runs.append(feat.grad.cpu().numpy())
    for b in range(B):
        vals = (np.repeat(go[b], 3, axis=1) * w[b].reshape(1, -1)).astype(np.float32)     # src[e / 3] * weight[e] in fp32
        assert _bits_equal(runs[0][b], _add_at(vals, idx[b].reshape(-1), m)), b
    assert _bits_equal(runs[1], runs[0])


def test_index_points_backward_at_2_to_the_22_points():
    from learning3d_amd.utils import index_points
    T, S, C = 1 << 22, 1024, 2
    rng = np.random.default_rng(23)
    idx = rng.integers(0, T, (1, S)).astype(np.int64)
    idx[0, -1] = T - 1
    idx[0, :8] = T - 1
    go = rng.standard_normal((1, S, C)).astype(np.float32)
    pts = torch.zeros((1, T, C), device="cuda", requires_grad=True)
    with launch_log() as log:
        index_points(pts, dev(idx)).backward(dev(go))
    assert "l3d_scatter_add_det" in log, log
    want = _add_at(go[0].T.copy(), idx[0], T)
    assert _bits_equal(pts.grad.cpu().numpy()[0].T, want)


# --------------------------------------------------------------------------------------------- _rows.linear, expanded gradients
@pytest.mark.parametrize("shape,Cin,Cout,f16", [((4096,), 64, 256, True), ((4, 1024), 64, 256, True),
                                                 ((333,), 40, 24, False), ((3, 111), 40, 24, False)])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("reduce", ["sum", "mean"])
def test_linear_rows_with_expanded_output_gradient(monkeypatch, shape, Cin, Cout, f16, bias, relu, reduce):
    """y.sum(0) of a [R, Cout] output, or a [B, N, Cout] output summed over (0, 1), backpropagated from a seeded [Cout] vector: without
    ReLU the gradient reaching the layer (and the bias gradient's colsum) is an expanded [R, Cout] view with strides (0, 1).  The mean
    and the ReLU mask hand it a dense gradient; those cases are checked against fp64 as well."""
    from learning3d_amd.models import _rows
    seen = []
    colsum = _rows.colsum
    monkeypatch.setattr(_rows, "colsum", lambda g: seen.append(g.stride()) or colsum(g))
    torch.manual_seed(len(shape) * 100 + Cin)
    lin = torch.nn.Linear(Cin, Cout, bias=bias).cuda()
    x = dev(rand(shape + (Cin,), Cin + len(shape), -1, 1)).requires_grad_()
    v = rand((Cout,), Cout + len(shape), -1, 1)                         # a non-constant upstream gradient
    dims = tuple(range(len(shape)))
    with launch_log() as log:
        y = _rows.linear(x, lin, relu=relu)
        (y.sum(dims) if reduce == "sum" else y.mean(dims)).backward(dev(v))
    assert ("l3d_pointwise_conv_f16[rows]" in log) == f16, log
    assert len(seen) == int(bias)
    if bias and reduce == "sum" and not relu:
        assert seen[0] == (0, 1), seen                                   # the shape l3d_colsum_rows refuses (row stride < cols)
    lin64 = torch.nn.Linear(Cin, Cout, bias=bias).cuda().double()
    lin64.load_state_dict({k: v.double() for k, v in lin.state_dict().items()})
    x64 = x.detach().double().requires_grad_()
    y64 = lin64(x64)
    if relu:                                                       # on the fp32 run's own branches
        y64 = y64 * (y.detach() > 0)
    (y64.sum(dims) if reduce == "sum" else y64.mean(dims)).backward(dev(v).double())
    pairs = [("dx", x.grad, x64.grad, 2e-5), ("dW", lin.weight.grad, lin64.weight.grad, 2e-5)]   # test_linear_rows_f16x2_route_vs_fp64
    if bias:
        pairs.append(("db", lin.bias.grad, lin64.bias.grad, 1e-5))                               # test_colsum_rows_vs_fp64_and_repeatable
    for name, got, want, bar in pairs:
        assert _rel(got.double().cpu().numpy(), want.cpu().numpy()) <= bar, (name, shape, bias, relu, reduce)


def test_linear_rows_after_a_raw_pointer_write_to_its_input():
    """_rows keeps the last row operand's f16 image keyed on the tensor's version; l3d_bmm_f32 writing into x (out=, and
    accumulate=True) must make the next linear(x) split the new values"""
    from learning3d_amd.models import _rows
    torch.manual_seed(41)
    lin = torch.nn.Linear(64, 256).cuda()
    lin64 = torch.nn.Linear(64, 256).cuda().double()
    lin64.load_state_dict({k: v.double() for k, v in lin.state_dict().items()})
    x = dev(rand((4096, 64), 42, -1, 1))
    a, b = dev(rand((4096, 32), 43, -1, 1)), dev(rand((32, 64), 44, -1, 1))
    with torch.no_grad():
        y1 = _rows.linear(x, lin)
        for accumulate in (False, True):
            _rows.bmm(a, b, out=x, accumulate=accumulate)
            with launch_log() as log:
                y2 = _rows.linear(x, lin)
            assert "l3d_pointwise_conv_f16[rows]" in log, log
            want = lin64(x.double())
            assert _rel(y2.double().cpu().numpy(), want.cpu().numpy()) <= 1e-5, accumulate      # the f16x2 product's fp32 level
            assert not torch.equal(y2, y1)
            y1 = y2


# --------------------------------------------------------------------------------------------- EdgeConv gather-max, PRNet
@pytest.mark.parametrize("N", [8192, 32768])
def test_edge_gather_max_at_its_lds_limit(N):
    from learning3d_amd._lib import check, lib, ptr, stream_ptr
    from learning3d_amd.models.prnet import ACT_LRELU
    B, Cout, k = 1, 64, 20
    rng = np.random.default_rng(N)
    pq = dev(rng.standard_normal((B, 2 * Cout, N)).astype(np.float32))
    idx = dev(rng.integers(0, N, (B, N, k)).astype(np.int64))
    out = torch.empty((B, Cout, N), device="cuda")
    check(lib().l3d_edge_gather_max(ptr(pq), ptr(idx), B, Cout, N, k, ACT_LRELU, ptr(out), Cout * N, stream_ptr()),
          "l3d_edge_gather_max")
    P, Q = pq[:, :Cout], pq[:, Cout:]
    z = P[:, :, idx[0]].amax(dim=-1) + Q                                             # one add and a max: exact
    want = torch.where(z > 0, z, z * torch.tensor(0.2, dtype=torch.float32, device="cuda"))
    assert torch.equal(out, want)


def test_prnet_dgcnn_eval_past_the_edge_gather_limit():
    """N = 32769, B = 1: the fused inference route would need a 128 KiB + 4 B channel row in LDS; the module takes its per-layer
    route instead, and agrees with the differentiable route at test_prnet_dgcnn_dynamic_graphs_golden's bar"""
    from learning3d_amd.models import _fused
    from learning3d_amd.models.prnet import DGCNN as PRNetDGCNN
    torch.manual_seed(7)
    net = PRNetDGCNN(emb_dims=512).cuda().eval()
    x = dev(rand((1, 3, 32769), 8, -1, 1))
    with torch.no_grad(), launch_log() as log:
        out = net(x)
    assert "l3d_edge_gather_max" not in log, log
    assert out.shape == (1, 512, 32769) and bool(torch.isfinite(out).all())
    with _fused.per_layer_route():
        ref = net(x.clone().requires_grad_()).detach()
    bad = (out - ref).abs() > 1e-4 + 1e-4 * ref.abs()
    assert bad.float().mean().item() < 1e-3, bad.float().mean().item()
