"""The models on clouds that arrive as views, under the launch audit: `xyzn[..., :3]` of an xyz-plus-normals array (row stride 6),
the transpose of a buffer stored in the other convention, and -- for the two-cloud models -- one template expanded over the batch
(stride 0).  The eval-mode fused route of every model, and one training step (forward and backward in train() mode) of PointNet,
DGCNN, DCP and PCN, must give, bit for bit, what they give on contiguous clones -- every tensor leaf of a dict result, and for
the training step every parameter gradient -- after the same launches.  Strides of the results are not compared: what torch's own
glue ops return follows their input's layout.  Weights are seeded by state_dict key (tests/golden/seeded.py).

FUSED names, per model, an entry point only the fused route launches: the shapes are the smallest at which the log still has it."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import layout_audit                                                                     # noqa: E402
from seeded import seeded_params                                                        # noqa: E402
from view_cases import JUNK, assert_identical, has_entry, leaves, logged, whole_storage  # noqa: E402

pytestmark = pytest.mark.gpu

B = 2


@pytest.fixture(autouse=True)
def audit(monkeypatch):
    return layout_audit.install(monkeypatch)


def clouds(n, seed, count=1, B=B):
    """`count` clouds [B,n,3] in the unit ball; the second a slightly turned and shifted copy of the first (a registration pair)"""
    g = torch.Generator().manual_seed(5000 + seed)
    a = torch.rand((B, n, 3), generator=g) * 2 - 1
    a = a / a.norm(dim=2).max(dim=1)[0].view(B, 1, 1)
    if count == 1:
        return [a.cuda()]
    c, s = 0.9800666, 0.1986693
    rot = torch.tensor([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    return [a.cuda(), (a @ rot.t() + torch.tensor([0.05, -0.02, 0.03]) + 0.01 * torch.randn((B, n, 3), generator=g)).cuda()]


def cloud_view(x, kind, shape):
    """x [B,N,3] contiguous -> a non-contiguous view holding a cloud, in the model's input_shape"""
    if kind == "xyzn":                                   # cloud[..., :3] of an xyz-plus-normals array
        wide = torch.full((x.shape[0], x.shape[1], 6), JUNK, device=x.device)
        wide[..., :3] = x
        v = wide[..., :3]
        return v if shape == "bnc" else v.transpose(1, 2)
    if kind == "transposed":                             # the transpose of a buffer stored in the other convention
        return x.transpose(1, 2).contiguous().transpose(1, 2) if shape == "bnc" else x.transpose(1, 2)
    assert kind == "expand"                              # one cloud for the whole batch
    v = x[:1].clone().expand(x.shape)
    return v if shape == "bnc" else v.transpose(1, 2)


def _seeded(net, seed):
    return seeded_params(net, seed).cuda().eval()


# name -> () -> (module, call(module, *clouds) -> result, number of clouds, points, input_shape[, clouds per batch])
MODELS = {}


def model(f):
    MODELS[f.__name__] = f
    return f


def _single(net, n=128, shape="bnc"):
    return net, (lambda m, x: m(x)), 1, n, shape


def _pointnet(shape, bn, seed):
    from learning3d_amd.models import PointNet
    return _single(_seeded(PointNet(emb_dims=64, input_shape=shape, use_bn=bn), seed), shape=shape)


@model
def pointnet_bnc():
    return _pointnet("bnc", False, 1)


@model
def pointnet_bnc_bn():
    return _pointnet("bnc", True, 2)


@model
def pointnet_bcn():
    return _pointnet("bcn", False, 3)


@model
def pointnet_bcn_bn():
    return _pointnet("bcn", True, 4)


@model
def dgcnn():
    from learning3d_amd.models import DGCNN
    return _single(_seeded(DGCNN(emb_dims=64), 5))


@model
def classifier():
    from learning3d_amd.models import Classifier, PointNet
    return _single(_seeded(Classifier(feature_model=PointNet(emb_dims=64, use_bn=True)), 6))


@model
def pcn():
    from learning3d_amd.models import PCN
    return _single(_seeded(PCN(emb_dims=1024, num_coarse=64, grid_size=2, detailed_output=True), 7), n=256)


@model
def dcp():
    from learning3d_amd.models import DCP, DGCNN
    return _seeded(DCP(feature_model=DGCNN(emb_dims=64), cycle=False), 8), (lambda m, t, s: m(t, s)), 2, 128, "bnc"


@model
def pointnetlk():
    from learning3d_amd.models import PointNet, PointNetLK
    return _seeded(PointNetLK(PointNet(emb_dims=64, use_bn=True)), 9), (lambda m, t, s: m(t, s, maxiter=3)), 2, 128, "bnc"


@model
def ipcrnet():
    from learning3d_amd.models import PointNet, iPCRNet
    return _seeded(iPCRNet(feature_model=PointNet(emb_dims=64)), 10), (lambda m, t, s: m(t, s, max_iteration=2)), 2, 128, "bnc"


@model
def flownet3d():
    from learning3d_amd.models import FlowNet3D
    feats = [c.transpose(1, 2).contiguous() for c in clouds(2048, 30, 2)]
    return _seeded(FlowNet3D(), 11), (lambda m, a, b: m(a, b, feats[0], feats[1])), 2, 2048, "bcn"


@model
def curvenet():
    from learning3d_amd.models import CurveNet
    return _single(_seeded(CurveNet(num_classes=40, k=20, setting='default'), 12), n=1024)


def _mask_call(m, t, s):
    out = m(t, s, "topk")
    return out, m.mask_idx


@model
def masknet():
    from learning3d_amd.models import MaskNet, PointNet
    return _seeded(MaskNet(feature_model=PointNet(use_bn=True), is_training=False), 13), _mask_call, 2, 128, "bnc"


def _masknet2():
    from learning3d_amd.models import MaskNet2
    from learning3d_amd.models.masknet2 import PointNet
    return _seeded(MaskNet2(feature_model=PointNet(use_bn=True), is_training=False), 14)


@model
def masknet2_masks():
    return _masknet2(), (lambda m, t, s: m.maskNet(t, s)), 2, 128, "bnc"          # the masks of a batch


@model
def masknet2_pair():
    def call(m, t, s):                                                           # MaskNet2.forward: one pair, mask > threshold
        return m(t, s), m.template_idx, m.source_idx
    return _masknet2(), call, 2, 128, "bnc", 1


@model
def segmentation():
    from learning3d_amd.models import PointNet, Segmentation
    return _single(_seeded(Segmentation(PointNet(emb_dims=64, use_bn=True, global_feat=False)), 15))


# an entry point that only the model's fused eval route launches (read off LAUNCH_LOG at these shapes)
FUSED = {"pointnet_bnc": "l3d_pointwise_conv", "pointnet_bnc_bn": "l3d_pointwise_conv", "pointnet_bcn": "l3d_pointwise_conv",
         "pointnet_bcn_bn": "l3d_pointwise_conv", "dgcnn": "l3d_edgeconv_forward_f16b", "classifier": "l3d_pointwise_conv[maxpool]",
         "pcn": "l3d_fold_mlp_f16", "dcp": "l3d_soft_correspondence", "pointnetlk": "l3d_reg_iclk_step", "ipcrnet": "l3d_pointwise_conv",
         "flownet3d": "l3d_sa_mlp3_fused", "curvenet": "l3d_curve_walk", "masknet": "l3d_mask_tail", "masknet2_masks": "l3d_self_attention_shared",
         "masknet2_pair": "l3d_mask_select", "segmentation": "l3d_pointwise_conv[maxpool]"}


def view_cases(base, shape, count):
    """[(what, views)]: each cloud in turn as an xyzn slice and as a transposed buffer, the others contiguous in the model's input
    shape; for two-cloud models also the template expanded"""
    plain = [b if shape == "bnc" else b.transpose(1, 2).contiguous() for b in base]
    out = []
    for i in range(count):
        for kind in ("xyzn", "transposed") + (("expand",) if count == 2 and i == 0 and base[i].shape[0] > 1 else ()):
            args = list(plain)
            args[i] = cloud_view(base[i], kind, shape)
            assert not args[i].is_contiguous()
            out.append((f"cloud {i} as {kind} {tuple(args[i].shape)} / {args[i].stride()}", args, i))
    return out


def run_pair(call, net, args, i, case, entry):
    dense = list(args)
    dense[i] = args[i].clone(memory_format=torch.contiguous_format)
    call(net, *dense)                                      # (the first call fills the caches of weight images: not compared)
    want, log = logged(call, net, *dense)
    again, log2 = logged(call, net, *dense)
    assert log, f"{case}: nothing launched"
    assert entry is None or has_entry(log, entry), f"{case}: the fused route's {entry} was not launched: {sorted(set(log))}"
    assert log2 == log, f"{case}: two runs on the same contiguous clouds launched different things"
    assert_identical(again, want, case + ": two runs on the SAME contiguous clouds (determinism precondition)", strides=False)
    before = whole_storage(args[i]).clone()
    got, vlog = logged(call, net, *args)
    assert vlog == log, f"{case}: launched {vlog}, on contiguous clones {log}"
    assert_identical(got, want, case, strides=False)
    assert torch.equal(whole_storage(args[i]), before), f"{case}: the caller's buffer was written to"


@pytest.mark.parametrize("name", sorted(MODELS))
def test_eval_route_on_view_clouds(name):
    net, call, count, n, shape, *batch = MODELS[name]()
    base = clouds(n, sum(map(ord, name)), count, *batch)
    for what, args, i in view_cases(base, shape, count):
        with torch.no_grad():
            run_pair(call, net, args, i, f"{name}, {what}", FUSED[name])


def _step(call, net, *args):
    """forward and backward in train() mode -> (the result's leaves, every parameter's gradient)"""
    torch.manual_seed(0)
    net.zero_grad(set_to_none=True)
    out = call(net, *args)
    outs = [t for _, t in leaves(out) if t.requires_grad]
    assert outs, "nothing to differentiate"
    loss = sum((t * torch.linspace(-1.0, 1.0, t.numel(), device=t.device).view(t.shape)).sum() for t in outs)
    loss.backward()
    grads = {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}
    assert grads
    return [t.detach() for t in outs], grads


@pytest.mark.parametrize("name", ["pointnet_bnc_bn", "pointnet_bcn", "dgcnn", "dcp", "pcn"])
def test_training_step_on_view_clouds(name):
    net, call, count, n, shape = MODELS[name]()[:5]
    net.train()
    base = clouds(n, 1 + sum(map(ord, name)), count)
    for what, args, i in view_cases(base, shape, count):
        run_pair(lambda m, *a: _step(call, m, *a), net, args, i, f"{name} training step, {what}", None)
