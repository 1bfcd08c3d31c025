"""The folded / packed parameter caches on CPU modules follow every change to a module's state (cached per parameter
version).  Each probe returns what the eval-mode forward would read from its cache; after a state change it must equal, bit for bit,
what a freshly built module loaded with the same state_dict gives, and it must have moved well beyond rounding (a stale cache would
otherwise pass).  The GPU counterpart, tests/test_gpu_state_changes.py, runs the models themselves."""
import pytest
import torch

from learning3d_amd.models import DGCNN, PointNetSetAbstraction, _fused
from learning3d_amd.models import prnet


def _randomise(net, seed):
    """weights and every BatchNorm's affine parameters and running statistics away from their defaults"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.3)
        for m in net.modules():
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.5)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)
    return net


def _bns(net):
    return [m for m in net.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]


def _edgeconv(net):
    return (net._packed.get([net.conv1, net.conv2, net.conv3, net.conv4], [net.bn1, net.bn2, net.bn3, net.bn4], "cpu"),)


def _sa():
    return PointNetSetAbstraction(npoint=16, radius=0.4, nsample=16, in_channel=3, mlp=[32, 32, 64], group_all=False)


class _ConvBN(torch.nn.Module):
    """a 1x1 conv over a 24-channel concatenation (8 + 16) with the BatchNorm behind it, and one (`plain`) with none"""

    def __init__(self):
        super().__init__()
        self.conv, self.bn = torch.nn.Conv1d(24, 16, 1), torch.nn.BatchNorm1d(16)
        self.plain = torch.nn.Conv1d(24, 16, 1)


def _blocks_without_bn(n):
    """A conv with no BatchNorm behind it, as MaskNet's h3[0] is split: its blocks stay in their cache slot across the change (nothing
    else writes it).  A BatchNorm-only change leaves them where they were, as it must; the fold of the model's other layer, a cache
    of its own on another conv, is what such a change moves."""
    wa, wb, scale, bias = _fused.conv_column_blocks(n.plain, None, 8)
    assert scale is None
    return (wa, wb, bias) + _fused.fold_conv_bn(n.conv, n.bn)


# name -> (model factory, probe: model -> tuple of the cached tensors an eval forward reads)
PROBES = {
    "fold_conv_bn": (lambda: DGCNN(emb_dims=64), lambda n: _fused.fold_conv_bn(n.conv5, n.bn5)),
    "EdgeConvParams.get": (lambda: DGCNN(emb_dims=64), _edgeconv),
    "DGCNN._conv5_folded": (lambda: DGCNN(emb_dims=64), lambda n: n._conv5_folded()[:3]),
    "sa_mlp3_params": (_sa, lambda n: _fused.sa_mlp3_params(list(n.mlp_convs), list(n.mlp_bns), torch.device("cpu"))[:1]),
    "prnet._layer_params": (lambda: prnet.DGCNN(emb_dims=64),
                            lambda n: n._layer_params("2", n.conv2, n.bn2, True)[:2] + n._layer_params("5", n.conv5, n.bn5, False)[:2]),
    "conv_column_blocks": (_ConvBN, lambda n: _fused.conv_column_blocks(n.conv, n.bn, 8)),
    "conv_column_blocks[scale_block=1]": (_ConvBN, lambda n: _fused.conv_column_blocks(n.conv, n.bn, 8, scale_block=1)),
    "conv_column_blocks[no bn]": (_ConvBN, _blocks_without_bn),
}


def _train_forward(net):
    """the reference PointNetLK's handle_batchNorm: train-mode forwards under no_grad with frozen weights, then eval()"""
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for bn in _bns(net):
            bn.train()
            shape = (4, bn.num_features, 8) + ((2,) if isinstance(bn, torch.nn.BatchNorm2d) else ())
            bn(torch.randn(shape, generator=g) * 2.0 + 1.0)
            bn.eval()


def _reset(net):
    for bn in _bns(net):
        bn.reset_running_stats()


def _half_float(net):
    net.half().float()


def _load_other(net):
    import copy
    net.load_state_dict(_randomise(copy.deepcopy(net), 99).state_dict())


def _optimizer_step(net):
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    for p in net.parameters():
        p.grad = torch.ones_like(p)
    opt.step()


def _no_grad_edit_weight(net):
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, (torch.nn.Conv1d, torch.nn.Conv2d)):
                m.weight.mul_(1.5)


def _no_grad_edit_buffer(net):
    with torch.no_grad():
        for bn in _bns(net):
            bn.running_var.mul_(2.0)


CHANGES = {"train_mode_forward": _train_forward, "reset_running_stats": _reset, "half_float": _half_float,
           "load_state_dict": _load_other, "optimizer_step": _optimizer_step, "no_grad_weight": _no_grad_edit_weight,
           "no_grad_buffer": _no_grad_edit_buffer}


def _fresh(factory, net):
    f = factory()
    f.load_state_dict(net.state_dict())
    return f.eval()


@pytest.mark.parametrize("change", list(CHANGES))
@pytest.mark.parametrize("probe", list(PROBES))
def test_cached_parameters_follow_state_changes(probe, change):
    factory, get = PROBES[probe]
    torch.manual_seed(3)
    net = _randomise(factory(), 5).eval()
    before = [t.clone() for t in get(net)]
    CHANGES[change](net)
    got = get(net)
    want = get(_fresh(factory, net))
    for a, b in zip(got, want):
        assert torch.equal(a, b), f"{probe} after {change}: stale cache (max diff {float((a - b).abs().max()):.3g})"
    # the change moved the cached values well beyond fp32 rounding: otherwise a stale cache would pass
    moved = max(float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)) for a, b in zip(before, want))
    assert moved > 1e-5, (probe, change, moved)


def test_conv_column_blocks_without_bn_has_no_scale_to_fold():
    with pytest.raises(ValueError, match="scale_block"):
        _fused.conv_column_blocks(torch.nn.Conv1d(24, 16, 1), None, 8, scale_block=1)


def test_fold_follows_the_running_statistics_of_a_train_mode_forward():
    """The issue's reproduction: fold, one train-mode forward under no_grad, eval, fold again -> the shift of the CURRENT statistics,
    checked against an fp64 fold written out here."""
    torch.manual_seed(0)
    conv, bn = torch.nn.Conv1d(8, 16, 1), torch.nn.BatchNorm1d(16)
    bn.eval()
    _fused.fold_conv_bn(conv, bn)
    with torch.no_grad():
        bn.train()
        bn(torch.randn(4, 16, 32) * 3.0 + 2.0)
        bn.eval()
    w, sc, sh = _fused.fold_conv_bn(conv, bn)
    s64 = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)
    t64 = bn.bias.detach().double() - bn.running_mean.double() * s64 + s64 * conv.bias.detach().double()
    assert float((sc.double() - s64).abs().max()) <= 1e-6 * float(s64.abs().max())
    assert float((sh.double() - t64).abs().max()) <= 1e-6 * float(t64.abs().max())


def test_batchnorm_without_running_statistics_or_affine_parameters():
    """track_running_stats=False normalises by the batch in eval mode too (not a pure function of the parameters: the fused route must
    not take it); affine=False folds with weight 1 and bias 0."""
    net = DGCNN(emb_dims=64).eval()
    assert not _fused._stochastic_or_batch_dependent(net)
    net.bn5 = torch.nn.BatchNorm2d(64, track_running_stats=False).eval()
    assert _fused._stochastic_or_batch_dependent(net)
    torch.manual_seed(1)
    conv, bn = torch.nn.Conv1d(8, 16, 1), torch.nn.BatchNorm1d(16, affine=False)
    with torch.no_grad():
        bn.running_mean.uniform_(-1, 1)
        bn.running_var.uniform_(0.5, 2)
    bn.eval()
    x = torch.randn(2, 8, 10)
    w, sc, sh = _fused.fold_conv_bn(conv, bn)
    want = bn(conv(x)).double()
    got = sc.double()[:, None] * torch.einsum("oi,bin->bon", w.double(), x.double()) + sh.double()[:, None]
    assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max())


@pytest.mark.xfail(strict=True, reason="an edit through .data bumps no version counter: the caches cannot see it without reading "
                                       "the tensors (DESIGN.md §3); use an in-place op under torch.no_grad() instead")
def test_data_edit_is_not_seen_by_the_cache():
    torch.manual_seed(2)
    conv, bn = torch.nn.Conv1d(8, 16, 1), torch.nn.BatchNorm1d(16).eval()
    _fused.fold_conv_bn(conv, bn)
    bn.running_mean.data.add_(1.0)
    _, _, sh = _fused.fold_conv_bn(conv, bn)
    s = bn.weight.detach() / torch.sqrt(bn.running_var + bn.eps)
    assert torch.allclose(sh, bn.bias.detach() - bn.running_mean * s + s * conv.bias.detach(), atol=1e-6)
