"""Every model's eval forward reads weight images the library prepares once and caches (BN-folded weights, packed EdgeConv blocks,
set-abstraction blocks, f16x2 / bf16x3 weight planes).  These tests run each model once on its fused eval route (the
route is asserted through the launch log), change its state, run it again and compare with a freshly built model of the same class
loaded with the same state_dict, on the same input.  Bar: bit-identical -- the same kernels on the same values; only the caches differ.
Each change is also required to move that output well beyond rounding, or a stale cache would pass.  A few changed outputs are held
against fp64 evaluations of the reference's op sequence as well.  The CPU counterpart is tests/test_weight_cache_state.py."""
import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _pts(shape, seed, scale=0.5):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(shape, generator=g) * 2 - 1) * scale).cuda()


class _log:
    def __enter__(self):
        from learning3d_amd import _lib
        _lib.LAUNCH_LOG = []
        return _lib.LAUNCH_LOG

    def __exit__(self, *exc):
        from learning3d_amd import _lib
        _lib.LAUNCH_LOG = None
        return False


def _bns(net):
    return [m for m in net.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]


def _flownet_inputs(n, seed):
    g = torch.Generator().manual_seed(seed)
    pc1 = torch.clamp(torch.randn((2, 3, n), generator=g), -2, 2)
    pc2 = pc1 + 0.05 * torch.randn((2, 3, n), generator=g)
    return pc1.cuda(), pc2.contiguous().cuda(), torch.rand((2, 3, n), generator=g).cuda(), torch.rand((2, 3, n), generator=g).cuda()


def _dcp_inputs(n, seed):
    t = _pts((2, n, 3), seed)
    rot = torch.tensor([[0.8, -0.6, 0.0], [0.6, 0.8, 0.0], [0.0, 0.0, 1.0]], device="cuda")
    return t, (t @ rot.t() + 0.1).contiguous()


def _make(name):
    from learning3d_amd.models import DCP, DGCNN, PCN, Classifier, FlowNet3D, PointNet, prnet
    return {
        "pointnet_global_bn": lambda: PointNet(emb_dims=256, use_bn=True),
        "pointnet_global": lambda: PointNet(emb_dims=256, use_bn=False),
        "pointnet_per_point_bn": lambda: PointNet(emb_dims=256, use_bn=True, global_feat=False),
        "pointnet_per_point": lambda: PointNet(emb_dims=256, use_bn=False, global_feat=False),
        "dgcnn": lambda: DGCNN(emb_dims=256),
        "pcn": lambda: PCN(emb_dims=1024, num_coarse=64, grid_size=2, detailed_output=True),
        "dcp": lambda: DCP(DGCNN(emb_dims=512)),
        "prnet_dgcnn": lambda: prnet.DGCNN(emb_dims=512),
        "flownet3d": lambda: FlowNet3D(),
        "classifier": lambda: Classifier(PointNet(emb_dims=1024, use_bn=True)),
    }[name]()


# name -> (inputs(n, seed), point counts: the first on the default fused route, the second on another route of the same model,
#          launches that must appear on the first)
SPECS = {
    "pointnet_global_bn": (lambda n, s: (_pts((2, n, 3), s),), (512, 500), ("l3d_pointwise_conv_split",)),
    "pointnet_global": (lambda n, s: (_pts((2, n, 3), s),), (512, 500), ("l3d_pointwise_conv_split",)),
    "pointnet_per_point_bn": (lambda n, s: (_pts((2, n, 3), s),), (512, 500), ("l3d_pointwise_conv_split",)),
    "pointnet_per_point": (lambda n, s: (_pts((2, n, 3), s),), (512, 500), ("l3d_pointwise_conv_split",)),
    "dgcnn": (lambda n, s: (_pts((2, n, 3), s),), (512, 320), ("l3d_edgeconv_forward_f16b", "l3d_pointwise_conv_f16")),
    "pcn": (lambda n, s: (_pts((2, n, 3), s),), (512, 500), ("l3d_first_layer_f16_planes", "l3d_pointwise_conv_f16[pool]",
                                                              "l3d_linear_rows", "l3d_fold_mlp_f16")),
    "dcp": (_dcp_inputs, (256,), ("l3d_edgeconv_forward_f16b", "l3d_attention_forward", "l3d_layernorm_planes", "l3d_kabsch")),
    "prnet_dgcnn": (lambda n, s: (_pts((2, 3, n), s),), (512,), ("l3d_knn_feature", "l3d_edge_gather_max", "l3d_pointwise_conv")),
    "flownet3d": (_flownet_inputs, (2048, 1100), ("l3d_sa_mlp3_fused", "l3d_group_first_layer")),
    "classifier": (lambda n, s: (_pts((2, n, 3), s),), (512,), ("l3d_pointwise_conv_split[maxpool]",)),
}


def _build(name, seed=0):
    torch.manual_seed(seed)
    net = _make(name).cuda()
    g = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():
        for bn in _bns(net):          # affine parameters and running statistics away from their defaults
            bn.weight.copy_(torch.rand(bn.weight.shape, generator=g) + 0.5)
            bn.bias.copy_(torch.randn(bn.bias.shape, generator=g) * 0.2)
            bn.running_mean.copy_(torch.randn(bn.running_mean.shape, generator=g) * 0.2)
            bn.running_var.copy_(torch.rand(bn.running_var.shape, generator=g) + 0.5)
    return net.eval()


def _outputs(out):
    if isinstance(out, dict):
        return [out[k].detach().clone() for k in sorted(out)]
    if isinstance(out, (tuple, list)):
        return [o.detach().clone() for o in out]
    return [out.detach().clone()]


def _run(net, inputs):
    with torch.no_grad():
        return _outputs(net(*inputs))


def _fresh(name, net, inputs):
    f = _make(name).cuda()
    f.load_state_dict(net.state_dict())
    return _run(f.eval(), inputs)


def _moved(a, b):
    return max(float((x - y).abs().max() / y.abs().max().clamp_min(1e-30)) for x, y in zip(a, b))


def _assert_same(got, want, what):
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), f"{what}: output {i} differs from a fresh model's by {float((a - b).abs().max()):.3g} (stale cache)"


# ------------------------------------------------------------------------------------------------------------ state changes
def _optimizer_step(net, name):
    opt = torch.optim.SGD(net.parameters(), lr=0.05)
    g = torch.Generator().manual_seed(11)
    for p in net.parameters():
        p.grad = torch.randn(p.shape, generator=g).cuda() * float(p.detach().abs().mean().clamp_min(1e-3)) * 4.0
    opt.step()


def _load_other(net, name):
    net.load_state_dict(_build(name, seed=1).state_dict())


def _edit_weight(net, name):
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, (torch.nn.Conv1d, torch.nn.Conv2d, torch.nn.Linear)):
                m.weight.mul_(1.25)


def _edit_buffer(net, name):
    with torch.no_grad():
        for bn in _bns(net):
            bn.running_var.mul_(2.0)


def _reset(net, name):
    for bn in _bns(net):
        bn.reset_running_stats()


def _train_forwards(net, name):
    """the reference PointNetLK's handle_batchNorm (models/pointnetlk.py:157-163): the feature model in train mode on template and
    source with its weights frozen, under no_grad, then eval()"""
    inputs, sizes, _ = SPECS[name]
    net.train()
    with torch.no_grad():
        net(*inputs(sizes[0], 21))
        net(*inputs(sizes[0], 22))
    net.eval()


def _train_forwards_torch_bn(net, name):
    from learning3d_amd.models import _fused
    prev = _fused.TRAIN_HIP
    _fused.TRAIN_HIP = False                # torch's BatchNorm updates the running statistics
    try:
        _train_forwards(net, name)
    finally:
        _fused.TRAIN_HIP = prev


def _half_float(net, name):
    net.half().float()


CHANGES = {"optimizer_step": _optimizer_step, "load_state_dict": _load_other, "no_grad_weight": _edit_weight,
           "no_grad_bn_buffer": _edit_buffer, "reset_running_stats": _reset, "train_forwards_hip": _train_forwards,
           "train_forwards_torch_bn": _train_forwards_torch_bn, "half_float": _half_float}
BN_ONLY = {"no_grad_bn_buffer", "reset_running_stats", "train_forwards_hip", "train_forwards_torch_bn"}
NO_BN = {"pointnet_global", "pointnet_per_point", "pcn"}

CASES = [(m, c) for m in SPECS for c in CHANGES if not (c in BN_ONLY and m in NO_BN)]


@pytest.mark.parametrize("model,change", CASES)
def test_eval_output_follows_state_change(model, change):
    inputs, sizes, route = SPECS[model]
    net = _build(model)
    x = inputs(sizes[0], 1)
    with _log() as log:
        before = _run(net, x)
    for r in route:
        assert any(n.startswith(r) for n in log), (model, r, sorted(set(log)))
    assert "l3d_bn_act_forward" not in log, (model, "took the per-layer route")
    CHANGES[change](net, model)
    got = _run(net, x)
    want = _fresh(model, net, x)
    _assert_same(got, want, f"{model} after {change}")
    assert _moved(before, want) > 2e-5, (model, change, _moved(before, want))


@pytest.mark.parametrize("model", [m for m in SPECS if len(SPECS[m][1]) > 1])
def test_two_routes_with_state_changes_in_between(model):
    """eval at the first point count, a state change, eval at a point count that takes another route, a second change, and back:
    a cache the second route does not consult must not be served stale when the first route comes back"""
    inputs, sizes, _ = SPECS[model]
    net = _build(model)
    xa, xb = inputs(sizes[0], 1), inputs(sizes[1], 2)
    a0 = _run(net, xa)
    _optimizer_step(net, model)
    _assert_same(_run(net, xb), _fresh(model, net, xb), f"{model} at {sizes[1]} after a step")
    net.half().float()
    _edit_weight(net, model)
    got = _run(net, xa)
    want = _fresh(model, net, xa)
    _assert_same(got, want, f"{model} back at {sizes[0]}")
    assert _moved(a0, want) > 2e-5


# ------------------------------------------------------------------------------------------------------------ BatchNorm variants
@pytest.mark.parametrize("variant", ["no_running_stats", "no_affine"])
def test_batchnorm_variants_in_eval_match_torch(variant):
    """A BatchNorm with track_running_stats=False normalises by the batch in eval mode (torch's rule): not a pure function of the
    parameters, so the per-layer route with batch statistics must serve it.  affine=False folds with weight 1, bias 0 on the fused
    route.  Against the module's own torch layers in fp64."""
    from learning3d_amd.models import PointNet
    torch.manual_seed(5)
    net = PointNet(emb_dims=256, use_bn=True)
    if variant == "no_running_stats":
        net.bn3 = torch.nn.BatchNorm1d(64, track_running_stats=False)
    else:
        net.bn2 = torch.nn.BatchNorm1d(64, affine=False)
        with torch.no_grad():
            net.bn2.running_mean.uniform_(-0.2, 0.2)
            net.bn2.running_var.uniform_(0.5, 1.5)
    net = net.cuda().eval()
    x = _pts((2, 512, 3), 6)
    with _log() as log, torch.no_grad():
        y = net(x)
    if variant == "no_running_stats":
        assert "l3d_channel_stats" in log, sorted(set(log))
    else:
        assert "l3d_bn_act_forward" not in log and "l3d_pointwise_conv_split" in log, sorted(set(log))
    n64 = copy.deepcopy(net).double()
    h = x.double().permute(0, 2, 1)
    with torch.no_grad():
        for conv, bn in n64._stack():
            h = F.relu(bn(conv(h)))
    err = float((y.double() - h).abs().max() / h.abs().max())
    assert err <= 1e-5, err


# ------------------------------------------------------------------------------------------------------------ fp64 spot checks
def test_changed_outputs_against_fp64():
    """One changed output per model family against an fp64 evaluation of the reference's op sequence: PointNet after PointNetLK's
    train-mode forwards (running statistics), DGCNN after the same, PCN after an optimizer step.  Bar, relative to the output's
    scale: 1e-5 for PointNet (bf16x3 / fp32 kernels), 1e-4 for the f16x2 chains of DGCNN and PCN, whose per-output bars live in
    tests/test_gpu_f16x2_per_output.py.  A stale fold misses these by orders of magnitude."""
    from test_gpu_grad_routes import _dgcnn_fp64
    # PointNet
    net = _build("pointnet_global_bn")
    x = SPECS["pointnet_global_bn"][0](512, 1)
    _run(net, x)
    _train_forwards(net, "pointnet_global_bn")
    y = _run(net, x)[0]
    n64 = copy.deepcopy(net).double()
    h = x[0].double().permute(0, 2, 1)
    with torch.no_grad():
        for conv, bn in n64._stack():
            h = F.relu(bn(conv(h)))
    err = float((y.double() - h).abs().max() / h.abs().max())
    print("PointNet after train-mode forwards vs fp64:", err)
    assert err <= 1e-5, err
    # DGCNN
    net = _build("dgcnn")
    x = SPECS["dgcnn"][0](512, 1)
    _run(net, x)
    _train_forwards(net, "dgcnn")
    y = _run(net, x)[0]
    with torch.no_grad():
        _, _, y64 = _dgcnn_fp64(net, x[0])
    err = float((y.double() - y64).abs().max() / y64.abs().max())
    print("DGCNN after train-mode forwards vs fp64:", err)
    assert err <= 1e-4, err
    # PCN (models/pcn.py:110-153 in fp64)
    net = _build("pcn")
    x = SPECS["pcn"][0](512, 1)
    _run(net, x)
    _optimizer_step(net, "pcn")
    coarse, fine = _run(net, x)                    # sorted keys: coarse_output, fine_output
    n64 = copy.deepcopy(net).double()
    with torch.no_grad():
        x64 = x[0].double().permute(0, 2, 1)
        h = n64.conv2(F.relu(n64.conv1(x64)))
        h = torch.cat([h, h.max(dim=2, keepdim=True)[0].expand(-1, -1, h.shape[2])], dim=1)
        gfeat = n64.conv4(F.relu(n64.conv3(h))).max(dim=2)[0]
        c64 = n64.linear3(F.relu(n64.linear2(F.relu(n64.linear1(gfeat))))).view(2, 64, 3)
        n64.num_points = 512
        f64 = n64._fine_torch(c64, gfeat)
    for got, want in ((coarse, c64), (fine, f64)):
        err = float((got.double() - want).abs().max() / want.abs().max())
        print("PCN after an optimizer step vs fp64:", err)
        assert err <= 1e-4, err


# ------------------------------------------------------------------------------------------------------------ the known limit
@pytest.mark.xfail(strict=True, reason="an edit through param.data bumps no version counter: the caches cannot see it without "
                                       "reading the tensors (DESIGN.md §3)")
def test_data_edit_is_not_seen():
    net = _build("dgcnn")
    x = SPECS["dgcnn"][0](512, 1)
    _run(net, x)
    net.bn5.running_mean.data.add_(0.5)
    _assert_same(_run(net, x), _fresh("dgcnn", net, x), "dgcnn after a .data edit")
