"""Gradients of the FlowNet3D modules and of PRNet's DGCNN against fp64, module by module.

A `.backward()` through an eval-mode FlowNet3D (or PRNet DGCNN) recomputes the network on the per-layer route
(_fused.checkpointed): the module's own grouping ops, then _train.conv_bn_act per layer.  Each test here builds ONE module,
differentiates it on that route, spells the route out again under no_grad while recording every discrete choice it makes
(furthest-point samples, ball-query / kNN / 3-NN indices, each layer's activation mask, the arg-max of each max over K),
proves with torch.equal that the recorded branches belong to the function that was differentiated, and evaluates the
reference's op sequence (reference models/flownet3d.py, line ranges at each mirror) in fp64 with plain torch ops on exactly
those branches: the mask as `z * mask`, the max as a gather at the arg-max, the 3-NN weights recomputed from the positions.

Bar: the project's tier, max |got - fp64| <= 1e-5 * max |fp64| per gradient tensor, flat, for every tensor of every
test.  The same mirror is also run in fp32 (plain torch autograd, same pinned branches) and every test prints module / tensor /
HIP error / fp32-mirror error / bar.  Measured on an MI355X (LABLOG.md R10.1 has the whole table): the HIP route's largest error
over all 100 tensors is 6.9e-7, the fp32 torch mirror's 2.0e-6 (both at mlp_convs.1.weight of the train-mode set abstraction), so no bar
is widened.

Only parameter and input gradients are compared: ball-query padding repeats an index, a max over K then has exact ties
between duplicate columns, and which duplicate gets the gradient differs between kernels -- both scatter to the same source."""
import copy
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_grad_routes import _lib_log          # noqa: E402

pytestmark = pytest.mark.gpu

TIER = 1e-5
BN_EPS, BN_MOMENTUM = 1e-5, 0.1                    # torch.nn.BatchNorm's defaults, which every module here keeps


def _rnd(shape, seed, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * (hi - lo) + lo).cuda()


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).cuda()


def _randomise_bn(module):
    """random running statistics and affine parameters (as tests/test_gpu_parity.py's FlowNet3D module test does)"""
    for sub in module.modules():
        if isinstance(sub, torch.nn.modules.batchnorm._BatchNorm):
            sub.running_mean.uniform_(-0.2, 0.2); sub.running_var.uniform_(0.5, 1.5)
            sub.weight.data.uniform_(0.5, 1.5); sub.bias.data.uniform_(-0.3, 0.3)
    return module


def _group(feat, idx):
    """feat [B,C,N], idx [B,S,K] -> feat[b, :, idx[b,s,k]] as [B,C,S,K]: grouping_operation in plain torch"""
    B, Cc, _ = feat.shape
    _, S, K = idx.shape
    return feat.gather(2, idx.long().reshape(B, 1, S * K).expand(B, Cc, S * K)).view(B, Cc, S, K)


class _Record:
    """the discrete choices of one fp32 run: index tensors by name, activation masks / multipliers and arg-maxima in call order"""

    def __init__(self):
        self.idx, self.mult, self.arg = {}, [], []

    def replay(self):
        self._m, self._a = iter(self.mult), iter(self.arg)
        return self


def _layers32(h, layers, rec):
    """[conv1x1 + BN + ReLU]* on the HIP layer kernels, as models/flownet3d.py's _mlp_stack runs them with autograd live"""
    from learning3d_amd.models import _train
    for conv, bn in layers:
        h = _train.conv_bn_act(h.contiguous(), conv, bn)
        rec.mult.append(h > 0)
    return h


def _max32(h, rec):
    v, a = torch.max(h, -1, keepdim=True)
    rec.arg.append(a)
    return v.squeeze(-1)


class _Mirror:
    """A module's parameters and BatchNorm buffers in `dtype`, and its layers as plain torch ops on recorded branches."""

    def __init__(self, module, buffers, dtype, training):
        self.p = {n: p.detach().to(dtype).clone().requires_grad_() for n, p in module.named_parameters()}
        self.b = {n: v.to(dtype) for n, v in buffers.items() if v.is_floating_point()}
        self.new_b, self.training = {}, training

    def layer(self, h, conv, bn, mult):
        """act(BN(W h + bias)) for h [B,C,...]: a 1x1 conv is a matrix product over the channel axis; BatchNorm by its definition
        (batch statistics and the momentum update of the running ones in train mode, running statistics in eval mode); the
        activation as a product with the fp32 run's multiplier (0 / 1 for ReLU, 0.2 / 1 for LeakyReLU)"""
        shp = h.shape
        w = self.p[conv + ".weight"]
        z = torch.matmul(w.reshape(w.shape[0], -1), h.reshape(shp[0], shp[1], -1))
        if conv + ".bias" in self.p:
            z = z + self.p[conv + ".bias"].view(1, -1, 1)
        if bn is not None:
            if self.training:
                n = z.shape[0] * z.shape[2]
                mean, var = z.mean(dim=(0, 2)), z.var(dim=(0, 2), unbiased=False)
                self.new_b[bn + ".running_mean"] = (1 - BN_MOMENTUM) * self.b[bn + ".running_mean"] + BN_MOMENTUM * mean.detach()
                self.new_b[bn + ".running_var"] = ((1 - BN_MOMENTUM) * self.b[bn + ".running_var"]
                                                   + BN_MOMENTUM * var.detach() * (n / (n - 1.0)))
            else:
                mean, var = self.b[bn + ".running_mean"], self.b[bn + ".running_var"]
            z = (z - mean.view(1, -1, 1)) / torch.sqrt(var.view(1, -1, 1) + BN_EPS)
            z = z * self.p[bn + ".weight"].view(1, -1, 1) + self.p[bn + ".bias"].view(1, -1, 1)
        h = z * mult.reshape(shp[0], z.shape[1], -1).to(z.dtype)
        return h.view(shp[0], z.shape[1], *shp[2:])

    def stack(self, h, names, rec):
        for conv, bn in names:
            h = self.layer(h, conv, bn, next(rec._m))
        return h

    @staticmethod
    def max(h, rec):
        return torch.gather(h, 3, next(rec._a)).squeeze(-1)


def _relerr(got, want):
    return float((got.double() - want.double()).abs().max()) / max(float(want.abs().max()), 1e-300)


def _report_and_assert(label, rows):
    """rows: (tensor name, HIP gradient, fp32-mirror gradient, fp64 gradient).  Prints the table, then holds every tensor to the tier."""
    failed = []
    print(f"\n{label}: relative to max |fp64 gradient|")
    print(f"  {'tensor':<28} {'HIP':>10} {'fp32 torch':>11} {'bar':>10}")
    for name, got, m32, want in rows:
        assert got is not None and want is not None and m32 is not None, (label, name, "every parameter and input takes part in the output")
        assert got.shape == want.shape and torch.isfinite(got).all(), (label, name)
        e_hip, e_32 = _relerr(got, want), _relerr(m32, want)
        bar = TIER
        print(f"  {name:<28} {e_hip:>10.2e} {e_32:>11.2e} {bar:>10.1e}")
        if not e_hip <= bar:
            failed.append((name, e_hip, e_32, bar))
    assert not failed, (label, failed)


def _mirror_and_compare(label, module, buffers, training, inputs, diff, mirror, rec, w, forwards, got_params, got_inputs):
    """The part of the method behind the record: `mirror(M, rec, **inputs)` in fp64 and in fp32 on the recorded branches, each
    differentiated under the output weights w; every fp32 output of `forwards` (name -> tensor) against the fp64 mirror's at
    rtol 1e-4, atol 1e-5 of the output's scale (that validates the mirror); then every parameter gradient (got_params) and input
    gradient (got_inputs) against fp64.  -> the fp64 mirror's new running statistics (train mode)."""
    grads = {}
    for tag, dt in (("fp64", torch.float64), ("fp32", torch.float32)):
        M = _Mirror(module, buffers, dt, training)
        li = {k: (v.detach().to(dt).requires_grad_(k in diff) if v is not None else None) for k, v in inputs.items()}
        o = mirror(M, rec.replay(), **li)
        (o * w.to(dt)).sum().backward()
        grads[tag] = ({n: p.grad for n, p in M.p.items()}, {k: li[k].grad for k in diff}, o.detach(), M.new_b)
    o64 = grads["fp64"][2]
    scale = float(o64.abs().max())
    for name, o in forwards.items():
        err = (o.detach().double() - o64).abs()
        print(f"\n{label}: {name} forward against the fp64 mirror {float(err.max()):.2e} at scale {scale:.2e}")
        assert bool((err <= 1e-4 * o64.abs() + 1e-5 * scale).all()), (label, name, "forward against the mirror", float(err.max()), scale)
    rows = [(n, got_params[n], grads["fp32"][0][n], grads["fp64"][0][n]) for n, _ in module.named_parameters()]
    rows += [("d " + k, got_inputs[k], grads["fp32"][1][k], grads["fp64"][1][k]) for k in sorted(diff)]
    _report_and_assert(label, rows)
    return grads["fp64"][3]


def _check_module(label, module, inputs, diff, call, respell, mirror, training=False, expect=()):
    """The method of this file for one module.  inputs: name -> fp32 device tensor (None allowed); diff: the names that require
    grad; call(module, **inputs) -> output on the route under test; respell(module, rec, **inputs) -> the same output spelled
    out under no_grad, filling rec; mirror(M, rec, **inputs) -> the output from plain torch ops on the recorded branches."""
    module.train(training)
    buffers = {n: b.detach().clone() for n, b in module.named_buffers()}
    twin = copy.deepcopy(module)                                        # the re-spelling's (train mode updates running statistics)
    for p in module.parameters():
        assert p.requires_grad
    leaf = {k: (v.clone().requires_grad_(k in diff) if v is not None else None) for k, v in inputs.items()}
    with _lib_log() as log:
        out = call(module, **leaf)
        w = _randn(tuple(out.shape), 977)
        n_fwd = len(log)
        (out * w).sum().backward()
        back = log[n_fwd:]
    for name in ("l3d_wgrad", "l3d_bn_act_backward", "l3d_scatter_add_det") + tuple(expect):
        assert name in back, (label, name, sorted(set(back)))           # the backward ran on the HIP layer kernels
    rec = _Record()
    with torch.no_grad():
        out_r = respell(twin, rec, **inputs)
    assert torch.equal(out_r, out.detach()), (label, "the re-spelt route is not the function that was differentiated",
                                              float((out_r - out.detach()).abs().max()))
    new = _mirror_and_compare(label, module, buffers, training, inputs, diff, mirror, rec, w, {"module": out},
                              {n: p.grad for n, p in module.named_parameters()}, {k: leaf[k].grad for k in diff})
    if training:
        assert len(new) == 2 * sum(isinstance(s, torch.nn.modules.batchnorm._BatchNorm) for s in module.modules())
        for n, b in module.named_buffers():
            if "running" in n:
                assert not torch.equal(b, buffers[n]), n
                torch.testing.assert_close(b.double(), new[n], rtol=1e-5, atol=1e-6, msg=n)
    return rec


# ------------------------------------------------------------------------------------------- PointNetSetAbstraction
def _sa_respell(m, rec, xyz, points):
    """PointNetSetAbstraction.forward's autograd route (models/flownet3d.py; QueryAndGroup's composed branch of
    utils/pointnet2_utils.py) on its own ops"""
    from learning3d_amd.utils import pointnet2_utils as pu
    xyz_t = xyz.permute(0, 2, 1).contiguous()
    fps = pu.furthest_point_sample(xyz_t, m.npoint)
    new_xyz = pu.gather_operation(xyz.contiguous(), fps)
    idx = pu.ball_query(m.radius, m.nsample, xyz_t, new_xyz.transpose(2, 1).contiguous())
    rec.idx["fps"], rec.idx["ball"] = fps, idx
    h = pu.grouping_operation(xyz_t.transpose(1, 2).contiguous(), idx) - new_xyz.unsqueeze(-1)
    if points is not None:
        h = torch.cat([h, pu.grouping_operation(points.contiguous(), idx)], dim=1)
    return _max32(_layers32(h, zip(m.mlp_convs, m.mlp_bns), rec), rec)


def _sa_mirror(M, rec, xyz, points):
    """reference models/flownet3d.py:104-122 with pointnet2_utils.py:259-292 (QueryAndGroup: grouped_xyz - new_xyz, then the
    features) as gathers at the recorded furthest-point samples and ball-query indices"""
    fps, idx = rec.idx["fps"], rec.idx["ball"]
    B, S = fps.shape
    new_xyz = torch.gather(xyz, 2, fps.long().view(B, 1, S).expand(B, 3, S))
    h = _group(xyz, idx) - new_xyz.unsqueeze(-1)
    if points is not None:
        h = torch.cat([h, _group(points, idx)], dim=1)
    names = [(f"mlp_convs.{i}", f"mlp_bns.{i}") for i in range(len(M.p) // 3)]
    return M.max(M.stack(h, names, rec), rec)


@pytest.mark.parametrize("mode,with_points", [("eval", True), ("train", True), ("eval", False)])
def test_set_abstraction_gradients_vs_fp64(mode, with_points):
    """PointNetSetAbstraction (reference :73-123) at B 2, N 200, 48 samples, 16 neighbours, 5 feature channels (Cin 8: no multiple
    of 16), mlp [32, 48, 64]; the radius leaves some centroids with fewer than 16 neighbours (padded duplicates) and some with
    16.  Gradients of every parameter, of the features and of the coordinates (through grouped_xyz - new_xyz: grouping AND the
    centroid gather).  Also in train mode -- batch statistics over a [B,C,S,K] tensor, running statistics against fp64 -- and
    without features (D = 0)."""
    from learning3d_amd.models.flownet3d import PointNetSetAbstraction
    torch.manual_seed(101)
    m = _randomise_bn(PointNetSetAbstraction(npoint=48, radius=0.6, nsample=16, in_channel=5 if with_points else 0,
                                             mlp=[32, 48, 64], group_all=False)).cuda()
    inputs = {"xyz": _rnd((2, 3, 200), 102), "points": _randn((2, 5, 200), 103) if with_points else None}
    diff = {"xyz", "points"} if with_points else {"xyz"}
    expect = ("l3d_bn_backward_stats",) if mode == "train" else ()
    rec = _check_module(f"PointNetSetAbstraction[{mode}, D={5 if with_points else 0}]", m, inputs, diff,
                        lambda mod, xyz, points: mod(xyz, points)[1], _sa_respell, _sa_mirror, training=mode == "train",
                        expect=expect)
    distinct = torch.tensor([[len(set(row)) for row in cloud] for cloud in rec.idx["ball"].cpu().tolist()])
    assert bool((distinct < 16).any()) and bool((distinct == 16).any()), distinct     # padded AND full neighbourhoods


# ------------------------------------------------------------------------------------------- FlowEmbedding
def _fe_respell(m, rec, pos1, pos2, feature1, feature2):
    from learning3d_amd.utils import pointnet2_utils as pu
    B, _, N = pos1.shape
    _, idx = pu.knn(m.nsample, pos1.permute(0, 2, 1).contiguous(), pos2.permute(0, 2, 1).contiguous())
    rec.idx["knn"] = idx
    pos_diff = pu.grouping_operation(pos2.contiguous(), idx) - pos1.view(B, -1, N, 1)
    feat_diff = torch.cat([pu.grouping_operation(feature2.contiguous(), idx), feature1.view(B, -1, N, 1).repeat(1, 1, 1, m.nsample)], dim=1)
    return _max32(_layers32(torch.cat([pos_diff, feat_diff], dim=1), zip(m.mlp_convs, m.mlp_bns), rec), rec)


def _fe_mirror(M, rec, pos1, pos2, feature1, feature2):
    """reference models/flownet3d.py:153-179 (knn branch): [pos2[idx] - pos1 | feature2[idx] | feature1 repeated], conv stack, max"""
    idx = rec.idx["knn"]
    K = idx.shape[2]
    pos_diff = _group(pos2, idx) - pos1.unsqueeze(-1)
    h = torch.cat([pos_diff, _group(feature2, idx), feature1.unsqueeze(-1).expand(-1, -1, -1, K)], dim=1)
    names = [(f"mlp_convs.{i}", f"mlp_bns.{i}") for i in range(len(M.p) // 3)]
    return M.max(M.stack(h, names, rec), rec)


def test_flow_embedding_gradients_vs_fp64():
    """FlowEmbedding (reference :125-180, knn) with 96 points in cloud 1, 80 in cloud 2, 24 channels, 16 neighbours,
    mlp [64, 64, 32]: gradients of every parameter, both feature inputs and both position inputs (pos_diff carries one to each)."""
    from learning3d_amd.models.flownet3d import FlowEmbedding
    torch.manual_seed(111)
    m = _randomise_bn(FlowEmbedding(radius=10.0, nsample=16, in_channel=24, mlp=[64, 64, 32], pooling="max", corr_func="concat")).cuda()
    inputs = {"pos1": _rnd((2, 3, 96), 112), "pos2": _rnd((2, 3, 80), 113),
              "feature1": _randn((2, 24, 96), 114), "feature2": _randn((2, 24, 80), 115)}
    _check_module("FlowEmbedding[knn]", m, inputs, set(inputs), lambda mod, **kw: mod(**kw)[1], _fe_respell, _fe_mirror)


# ------------------------------------------------------------------------------------------- PointNetSetUpConv
def _su_index(m, pos1, pos2):
    from learning3d_amd.utils import pointnet2_utils as pu
    from learning3d_amd.utils.model_common_utils import query_ball_point
    p1, p2 = pos1.permute(0, 2, 1).contiguous(), pos2.permute(0, 2, 1).contiguous()
    return pu.knn(m.nsample, p1, p2)[1] if m.knn else query_ball_point(m.radius, m.nsample, p2, p1)


def _su_respell(m, rec, pos1, pos2, feature1, feature2):
    from learning3d_amd.utils import pointnet2_utils as pu
    B, _, N = pos1.shape
    idx = _su_index(m, pos1, pos2)
    rec.idx["nbr"] = idx
    pos_diff = pu.grouping_operation(pos2.contiguous(), idx) - pos1.view(B, -1, N, 1)
    h = torch.cat([pu.grouping_operation(feature2.contiguous(), idx), pos_diff], dim=1)
    h = _max32(_layers32(h, [(s[0], s[1]) for s in m.mlp1_convs], rec), rec)
    if feature1 is not None:
        h = torch.cat([h, feature1], dim=1)
    return _layers32(h, [(s[0], s[1]) for s in m.mlp2_convs], rec)


def _su_mirror(M, rec, pos1, pos2, feature1, feature2):
    """reference models/flownet3d.py:218-242: [feature2[idx] | pos2[idx] - pos1], mlp1 on the grouped tensor, max over the
    neighbours, feature1 appended, mlp2 per point"""
    idx = rec.idx["nbr"]
    h = torch.cat([_group(feature2, idx), _group(pos2, idx) - pos1.unsqueeze(-1)], dim=1)
    n1 = len({n.split(".")[1] for n in M.p if n.startswith("mlp1_convs.")})
    n2 = len({n.split(".")[1] for n in M.p if n.startswith("mlp2_convs.")})
    h = M.max(M.stack(h, [(f"mlp1_convs.{i}.0", f"mlp1_convs.{i}.1") for i in range(n1)], rec), rec)
    if feature1 is not None:
        h = torch.cat([h, feature1], dim=1)
    return M.stack(h, [(f"mlp2_convs.{i}.0", f"mlp2_convs.{i}.1") for i in range(n2)], rec)


@pytest.mark.parametrize("variant", ["max_of_raw_concat", "no_feature1", "ball_query_padded"])
def test_set_upconv_gradients_vs_fp64(variant):
    """PointNetSetUpConv (reference :182-242) with 96 points receiving from 40, 8 neighbours:
    mlp [] + mlp2 [64, 32] (su1's shape: the max over K of the raw grouped concat, no conv in front of it); mlp [32, 64] +
    mlp2 [48] without feature1; knn=False with mlp [32], mlp2 [] and a radius at which query_ball_point pads.  Gradients of every
    parameter, the features and both position inputs."""
    from learning3d_amd.models.flownet3d import PointNetSetUpConv
    torch.manual_seed(121)
    C1, C2 = 12, 20
    pos2 = _rnd((2, 3, 40), 122)
    # every receiving point lies next to some source point, so no ball is empty (the reference indexes out of range there)
    pos1 = (pos2[:, :, torch.arange(96) % 40] + 0.05 * _randn((2, 3, 96), 123)).contiguous()
    f1, f2 = _randn((2, C1, 96), 124), _randn((2, C2, 40), 125)
    if variant == "max_of_raw_concat":
        m = PointNetSetUpConv(nsample=8, radius=2.4, f1_channel=C1, f2_channel=C2, mlp=[], mlp2=[64, 32])
    elif variant == "no_feature1":
        m, f1 = PointNetSetUpConv(nsample=8, radius=2.4, f1_channel=0, f2_channel=C2, mlp=[32, 64], mlp2=[48]), None
    else:
        m = PointNetSetUpConv(nsample=8, radius=0.55, f1_channel=C1, f2_channel=C2, mlp=[32], mlp2=[], knn=False)
    m = _randomise_bn(m).cuda()
    inputs = {"pos1": pos1, "pos2": pos2, "feature1": f1, "feature2": f2}
    diff = {k for k, v in inputs.items() if v is not None}
    rec = _check_module(f"PointNetSetUpConv[{variant}]", m, inputs, diff, lambda mod, **kw: mod(**kw), _su_respell, _su_mirror)
    if variant == "ball_query_padded":
        idx = rec.idx["nbr"]
        assert int(idx.min()) >= 0 and int(idx.max()) < 40
        distinct = torch.tensor([[len(set(row)) for row in cloud] for cloud in idx.cpu().tolist()])
        assert bool((distinct < 8).any()), "query_ball_point did not pad at this radius"


# ------------------------------------------------------------------------------------------- PointNetFeaturePropogation
def _fp_respell(m, rec, pos1, pos2, feature1, feature2):
    from learning3d_amd.utils import pointnet2_utils as pu
    dists, idx = pu.three_nn(pos1.permute(0, 2, 1).contiguous(), pos2.permute(0, 2, 1).contiguous())
    rec.idx["three_nn"], rec.idx["dists"] = idx, dists
    weight = 1.0 / dists.clamp_min(1e-10)
    weight = weight / torch.sum(weight, -1, keepdim=True)
    h = torch.cat([pu.three_interpolate(feature2.contiguous(), idx, weight.contiguous()), feature1], 1)
    return _layers32(h, zip(m.mlp_convs, m.mlp_bns), rec)


def _fp_mirror(M, rec, pos1, pos2, feature1, feature2):
    """reference models/flownet3d.py:265-286: inverse-distance weights over the three nearest known points (distances below 1e-10
    set to 1e-10), recomputed here from the positions at the recorded indices; the weighted sum; feature1 appended; Conv1d stack"""
    idx = rec.idx["three_nn"]
    B, N, _ = idx.shape
    p1, p2 = pos1.permute(0, 2, 1), pos2.permute(0, 2, 1)
    nb = p2.gather(1, idx.long().reshape(B, N * 3, 1).expand(B, N * 3, 3)).view(B, N, 3, 3)
    dists = ((p1.unsqueeze(2) - nb) ** 2).sum(-1).sqrt().clamp_min(1e-10)
    weight = 1.0 / dists
    weight = weight / torch.sum(weight, -1, keepdim=True)
    h = torch.sum(_group(feature2, idx) * weight.view(B, 1, N, 3), dim=-1)
    h = torch.cat([h, feature1], 1)
    return M.stack(h, [(f"mlp_convs.{i}", f"mlp_bns.{i}") for i in range(len(M.p) // 4)], rec)


def test_feature_propagation_gradients_vs_fp64():
    """PointNetFeaturePropogation (reference :244-286): 150 unknown points, 40 known, 32 + 3 channels (a concat width that is no
    multiple of 16, like the model's 259), mlp [64, 32] on Conv1d WITH bias.  Two unknown points coincide exactly with a known
    one (distance 0 -> the 1e-10 clamp).  three_nn carries no gradient to the positions in the reference, so only parameters and
    features are differentiated."""
    from learning3d_amd.models.flownet3d import PointNetFeaturePropogation
    torch.manual_seed(131)
    m = _randomise_bn(PointNetFeaturePropogation(in_channel=32 + 3, mlp=[64, 32])).cuda()
    pos1, pos2 = _rnd((2, 3, 150), 132), _rnd((2, 3, 40), 133)
    pos1[:, :, 0], pos1[:, :, 77] = pos2[:, :, 5], pos2[:, :, 11]
    inputs = {"pos1": pos1.contiguous(), "pos2": pos2, "feature1": _randn((2, 3, 150), 134), "feature2": _randn((2, 32, 40), 135)}
    rec = _check_module("PointNetFeaturePropogation", m, inputs, {"feature1", "feature2"}, lambda mod, **kw: mod(**kw),
                        _fp_respell, _fp_mirror)
    d = rec.idx["dists"]
    assert bool((d[:, [0, 77], 0] < 1e-10).all()), d[:, [0, 77]]                      # the clamp acted
    assert rec.idx["three_nn"][:, [0, 77], 0].cpu().tolist() == [[5, 11], [5, 11]]


# ------------------------------------------------------------------------------------------- _GraphFeature alone
@pytest.mark.parametrize("Cc,N", [(64, 200), (64, 65), (128, 200), (128, 65), (64, 21)])
def test_graph_feature_forward_backward_vs_fp64(Cc, N):
    """utils/model_common_utils._GraphFeature (the graph feature of PRNet's layers 2-4: 64 / 128 learned channels) on a drawn index
    in which one hub point sits in most neighbourhoods and a quarter of the points in none; B 3, k 20 (N 21: the smallest cloud).
    Forward: exactly the fp64 gather.  Backward: dx[b,c,t] = sum of the m(t) neighbour-half gradients that point at t, plus the
    sum of the k centre-half gradients of t.  A sum of m fp32 terms, in any order, is within (m - 1) 2^-24 sum|terms| of the exact
    one to first order; (m + 1) 2^-24 sum|terms| covers that, the rounding of the final add of the two halves and the second-order
    terms; the centre half has m = k.  The bound is evaluated per element in fp64.  Two backward calls give the same bits."""
    from learning3d_amd.utils.model_common_utils import _GraphFeature
    B, k, hub = 3, 20, 3
    g = torch.Generator().manual_seed(1000 * Cc + N)
    allowed = N - max(1, N // 4)
    idx = torch.randint(0, allowed, (B, N, k), generator=g)
    idx[:, :, 0] = torch.where(torch.rand((B, N), generator=g) < 0.8, torch.full((B, N), hub), idx[:, :, 0])
    idx = idx.cuda()
    m = torch.zeros((B, N), dtype=torch.float64, device="cuda").scatter_add_(1, idx.view(B, -1), torch.ones((B, N * k), dtype=torch.float64, device="cuda"))
    assert bool((m[:, hub] > N / 2).all()) and bool((m == 0).any(dim=1).all())
    x = torch.randn((B, Cc, N), generator=g).cuda().requires_grad_()
    w = torch.randn((B, N, k, 2 * Cc), generator=g).cuda()
    with _lib_log() as log:
        out = _GraphFeature.apply(x, idx)
        (out * w).sum().backward()
    assert log == ["l3d_graph_feature", "l3d_scatter_add_det"], log
    x64 = x.detach().double().requires_grad_()
    xt = x64.transpose(1, 2)                                                               # [B,N,C]
    flat = idx.view(B, N * k, 1).expand(B, N * k, Cc)
    out64 = torch.cat([xt.gather(1, flat).view(B, N, k, Cc), xt.unsqueeze(2).expand(B, N, k, Cc)], dim=3)
    assert torch.equal(out.detach().double(), out64.detach())
    (out64 * w.double()).sum().backward()
    s_nbr = torch.zeros((B, N, Cc), dtype=torch.float64, device="cuda").scatter_add_(1, flat, w[..., :Cc].double().abs().reshape(B, N * k, Cc))
    s_ctr = w[..., Cc:].double().abs().sum(dim=2)                                          # [B,N,C]
    bound = (((m + 1).unsqueeze(-1) * s_nbr + (k + 1) * s_ctr) * 2.0 ** -24).transpose(1, 2)
    err = (x.grad.double() - x64.grad).abs()
    print(f"\n_GraphFeature[C={Cc}, N={N}]: max error / bound {float((err / bound).max()):.3f}, "
          f"max error / max |fp64| {float(err.max() / x64.grad.abs().max()):.2e}")
    assert bool((err <= bound).all()), float((err / bound).max())
    first = x.grad.clone()
    x.grad = None
    (_GraphFeature.apply(x, idx) * w).sum().backward()
    assert torch.equal(first, x.grad)


# ------------------------------------------------------------------------------------------- PRNet's DGCNN, eval backward
_PRNET_LAYERS = (("conv1", "bn1"), ("conv2", "bn2"), ("conv3", "bn3"), ("conv4", "bn4"))


def _prnet_respell(net, rec, x):
    """models/prnet.py's per-layer route: per layer a kNN graph (xyz space for layer 1, the previous layer's feature space for
    layers 2-4), the graph feature, Conv2d + BatchNorm2d + LeakyReLU(0.2) and the max over k on the HIP layer kernels"""
    from learning3d_amd.models import _train
    from learning3d_amd.models.prnet import ACT_LRELU
    from learning3d_amd.utils.model_common_utils import _GraphFeature, knn
    B, _, N = x.shape
    h, xs = x, []
    for i, (conv, bn) in enumerate(_PRNET_LAYERS):
        idx = knn(h, k=20)
        rec.idx[i] = idx
        gf = _GraphFeature.apply(h, idx).permute(0, 3, 1, 2).contiguous()
        y, ymax = _train.conv_bn_act_max(gf, getattr(net, conv), getattr(net, bn), relu=ACT_LRELU)
        rec.mult.append(torch.where(y > 0, 1.0, 0.2))
        arg = y.max(dim=-1, keepdim=True)[1]
        assert torch.equal(torch.gather(y, 3, arg), ymax)
        rec.arg.append(arg)
        xs.append(ymax)
        h = ymax.view(B, -1, N)
    out = _train.conv_bn_act(torch.cat(xs, dim=1), net.conv5, net.bn5, relu=ACT_LRELU)
    rec.mult.append(torch.where(out > 0, 1.0, 0.2))
    return out.view(B, -1, N)


def _prnet_mirror(M, rec, x):
    """reference models/prnet.py:76-97 with utils/model_common_utils.py:132-156 (graph feature = cat(neighbour, centre)) on the
    recorded graphs; leaky_relu as a product with where(mask, 1, 0.2), each max over k as a gather at the recorded arg-max"""
    B, _, N = x.shape
    h, xs = x, []
    for i, (conv, bn) in enumerate(_PRNET_LAYERS):
        idx = rec.idx[i]
        gf = torch.cat([_group(h, idx), h.unsqueeze(-1).expand(-1, -1, -1, idx.shape[2])], dim=1)
        y = M.layer(gf, conv, bn, next(rec._m))
        xs.append(torch.gather(y, 3, next(rec._a)))
        h = xs[-1].squeeze(-1)
    return M.layer(torch.cat(xs, dim=1), "conv5", "bn5", next(rec._m)).view(B, -1, N)


def test_prnet_dgcnn_eval_backward_vs_fp64():
    """PRNet's DGCNN (emb 64, B 2, N 128, random BatchNorm state) in eval mode with grad on: the forward is the fused route, the
    backward recomputes the per-layer route, whose layers 2-4 differentiate through _GraphFeature.backward behind a feature-space
    kNN.  Every parameter gradient and the input gradient against fp64 on the recorded graphs, LeakyReLU signs and arg-maxima."""
    from learning3d_amd.models import _fused
    from learning3d_amd.models.prnet import DGCNN
    torch.manual_seed(141)
    net = _randomise_bn(DGCNN(emb_dims=64)).cuda().eval()
    buffers = {n: b.detach().clone() for n, b in net.named_buffers()}
    x0 = _rnd((2, 3, 128), 142)
    w = _randn((2, 64, 128), 143)
    x = x0.clone().requires_grad_()
    with _lib_log() as log:
        out = net(x)
        assert "l3d_edge_gather_max" in log and "l3d_graph_feature" not in log, sorted(set(log))     # the fused forward
        n_fwd = len(log)
        (out * w).sum().backward()
        back = log[n_fwd:]
    for name in ("l3d_graph_feature", "l3d_wgrad", "l3d_bn_act_backward", "l3d_scatter_add_det"):
        assert name in back, (name, sorted(set(back)))
    # the function the backward differentiated: the per-layer route, run directly with autograd live ...
    got = {n: p.grad.clone() for n, p in net.named_parameters()}
    net.zero_grad()
    x2 = x0.clone().requires_grad_()
    with _fused.per_layer_route():
        out_pl = net(x2)
    (out_pl * w).sum().backward()
    assert torch.equal(x.grad, x2.grad) and all(torch.equal(got[n], p.grad) for n, p in net.named_parameters())
    # ... is the route spelled out here, whose branches are therefore the differentiated ones
    rec = _Record()
    with torch.no_grad():
        out_r = _prnet_respell(net, rec, x0)
    assert torch.equal(out_r, out_pl.detach())
    _mirror_and_compare("PRNet DGCNN[eval backward]", net, buffers, False, {"x": x0}, {"x"}, _prnet_mirror, rec, w,
                        {"per-layer": out_pl, "fused": out}, got, {"x": x.grad})


# ------------------------------------------------------------------------------------------- the recompute plumbing
def test_flownet3d_recompute_backward_is_the_per_layer_backward():
    """_fused._Recompute on the whole FlowNet3D (eval, B 1, N 1100: sa1 draws 1024 samples), random BatchNorm state.  Gradients
    (a) through net(...) -- fused forward, per-layer recomputation inside _Recompute.backward, its needs_input_grad / parameter
    bookkeeping -- and (b) through net._forward called directly under _fused.per_layer_route() with autograd live run the same
    deterministic kernels on the same inputs (every gather-type backward is l3d_scatter_add_det, no atomics anywhere), so every
    parameter gradient and the gradients of both feature inputs are bit-identical, and none is missing on one side only.  The
    coordinates take no gradient here: a mis-numbered needs_input_grad then shows as a missing feature gradient."""
    from learning3d_amd.models import FlowNet3D, _fused
    torch.manual_seed(151)
    net = _randomise_bn(FlowNet3D()).cuda().eval()
    N = 1100
    g = torch.Generator().manual_seed(152)
    pc1 = torch.clamp(torch.randn((1, 3, N), generator=g), -2, 2).cuda()
    pc2 = (pc1 + 0.05 * torch.randn((1, 3, N), generator=g).cuda()).contiguous()
    f1, f2 = torch.rand((1, 3, N), generator=g).cuda(), torch.rand((1, 3, N), generator=g).cuda()
    w = _randn((1, 3, N), 153)
    fa1, fa2 = f1.clone().requires_grad_(), f2.clone().requires_grad_()
    with _lib_log() as log:
        out_a = net(pc1, pc2, fa1, fa2)
        assert "l3d_group_first_layer" in log and "l3d_bn_act_forward" not in log, sorted(set(log))      # the fused forward
        n_fwd = len(log)
        (out_a * w).sum().backward()
        back = log[n_fwd:]
    for name in ("l3d_bn_act_forward", "l3d_wgrad", "l3d_bn_act_backward", "l3d_scatter_add_det"):
        assert name in back, (name, sorted(set(back)))
    grads_a = {n: (p.grad.clone() if p.grad is not None else None) for n, p in net.named_parameters()}
    net.zero_grad()
    fb1, fb2 = f1.clone().requires_grad_(), f2.clone().requires_grad_()
    with _lib_log() as log_b, _fused.per_layer_route():
        out_b = net._forward(pc1, pc2, fb1, fb2)
        (out_b * w).sum().backward()
    for name in ("l3d_bn_act_forward", "l3d_wgrad", "l3d_bn_act_backward", "l3d_scatter_add_det"):
        assert name in log_b, (name, sorted(set(log_b)))                                  # (b) is the HIP per-layer route too
    assert "l3d_group_first_layer" not in log_b
    scale = float(out_b.detach().abs().max())
    assert float((out_a.detach() - out_b.detach()).abs().max()) <= 1e-4 * scale          # fused forward against the per-layer one
    for name, a, b in [(n, grads_a[n], p.grad) for n, p in net.named_parameters()] + [("d feature1", fa1.grad, fb1.grad),
                                                                                     ("d feature2", fa2.grad, fb2.grad)]:
        assert a is not None and b is not None, (name, a is None, b is None)
        assert float(b.abs().max()) > 0 and torch.equal(a, b), (name, float((a - b).abs().max()), float(b.abs().max()))
