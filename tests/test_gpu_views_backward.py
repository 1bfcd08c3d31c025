"""The backward of every autograd.Function of the package on gradients that arrive as views, under the launch audit.

Autograd hands `grad_outputs` to a custom backward as they are: a transposed view, a stride-2 slice, a stride-0 expand of a
[1, C, 1]-like tensor.  Each backward decides by hand how its kernels read them.  For every differentiable Function,
torch.autograd.grad with such a gradient must return, bit for bit and in shape, dtype and strides, what it returns with
g.contiguous(), after the same launches; two-output Functions also get one gradient alone (the other undefined).  Then the
forward runs on view INPUTS and the backward behind it (tensors saved for backward that came from views) against the same on
contiguous clones.  There the gradients' strides are not compared: a gradient laid out like its operand is torch's own convention
and models/_rows._like's purpose.

Of the 21 Functions, FurthestPointSampling, KNN, ThreeNN and BallQuery return only non-differentiable outputs (their backward
returns None for every input): their view handling is the assert of test_gpu_views_ops.py.  GatherOperation, ThreeInterpolate and
GroupingOperation assert contiguous inputs like the reference, so only their gradients are views here."""
import os
import sys

import pytest
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import layout_audit                                                                     # noqa: E402
from seeded import seeded_params                                                        # noqa: E402
from view_cases import assert_identical, float_views, grad_views, has_entry, logged, whole_storage    # noqa: E402

pytestmark = pytest.mark.gpu

B, N, M, K = 2, 128, 96, 8
INPUT_KINDS = ("transposed", "channels", "rows", "expand")


@pytest.fixture(autouse=True)
def audit(monkeypatch):
    return layout_audit.install(monkeypatch)


def rnd(*shape, seed=0, scale=1.0):
    return (torch.rand(shape, generator=torch.Generator().manual_seed(3000 + seed)) * 2 - 1).mul_(scale).cuda()


def rint(hi, *shape, seed=0, dtype=torch.int64):
    return torch.randint(0, hi, shape, generator=torch.Generator().manual_seed(4000 + seed)).to(dtype).cuda()


class Leaves:
    """leaf(t): t as a graph input that requires grad -- contiguous, a view of the given kind, or that view's contiguous clone"""

    def __init__(self, kind=None, dense=True):
        self.kind, self.dense, self.inputs, self.views = kind, dense, [], []

    def __call__(self, t):
        if self.kind is not None:
            vs = float_views(t, (self.kind,))
            if vs:
                v = vs[0][1]
                t = v.clone(memory_format=torch.contiguous_format) if self.dense else v
                if not self.dense:
                    self.views.append(v)
        t = t.detach().requires_grad_(True)
        self.inputs.append(t)
        return t

    def params(self, module):
        self.inputs += [p for p in module.parameters() if p.requires_grad]
        return module


# name -> (build(leaf) -> output or tuple of outputs, the entry point the backward must launch or None, view inputs allowed)
CASES = {}


def case(entry, view_inputs=True):
    def add(f):
        CASES[f.__name__] = (f, entry, view_inputs)
        return f
    return add


@case("l3d_scatter_add_det")
def graph_feature(leaf):
    from learning3d_amd.utils.model_common_utils import _GraphFeature
    return _GraphFeature.apply(leaf(rnd(B, 8, N, seed=1)), rint(N, B, N, K, seed=1))


@case(None)
def exp_map(leaf):
    from learning3d_amd.ops.se3 import ExpMap
    return ExpMap.apply(leaf(rnd(B, 6, seed=2, scale=0.5)))


@case("l3d_scatter_add_det", view_inputs=False)
def gather_operation(leaf):
    from learning3d_amd.utils.pointnet2_utils import gather_operation
    return gather_operation(leaf(rnd(B, 8, N, seed=3)), rint(N, B, 32, seed=3, dtype=torch.int32))


@case("l3d_scatter_add_det", view_inputs=False)
def three_interpolate(leaf):
    from learning3d_amd.utils.pointnet2_utils import three_interpolate
    return three_interpolate(leaf(rnd(B, 8, 32, seed=4)), rint(32, B, N, 3, seed=4, dtype=torch.int32), rnd(B, N, 3, seed=5).abs_())


@case("l3d_scatter_add_det", view_inputs=False)
def grouping_operation(leaf):
    from learning3d_amd.utils.pointnet2_utils import grouping_operation
    return grouping_operation(leaf(rnd(B, 8, N, seed=6)), rint(N, B, 32, K, seed=6, dtype=torch.int32))


@case(None)
def kabsch(leaf):
    from learning3d_amd.utils.svd import _KabschFunction
    return _KabschFunction.apply(leaf(rnd(B, 3, N, seed=7)), leaf(rnd(B, 3, N, seed=8)))


@case("l3d_bmm_f32")
def matmul(leaf):
    from learning3d_amd.models import _rows
    return _rows.matmul(leaf(rnd(B, N, 32, seed=9)), leaf(rnd(B, 32, M, seed=10)), alpha=0.5)


@case("l3d_softmax_rows")
def softmax_rows(leaf):
    from learning3d_amd.models import _rows
    return _rows.softmax_rows(leaf(rnd(B, N, M, seed=11, scale=4.0)), 0.5)


def _linear(leaf, relu, seed):
    from learning3d_amd.models import _rows
    lin = leaf.params(seeded_params(nn.Linear(32, 48), seed).cuda())
    return _rows.linear(leaf(rnd(B, N, 32, seed=seed)), lin, relu=relu)


@case("l3d_bmm_f32")
def linear_rows(leaf):
    return _linear(leaf, False, 12)


@case("l3d_bmm_f32")
def linear_rows_relu(leaf):
    return _linear(leaf, True, 13)


@case("l3d_bmm_f32")
def square_distance(leaf):
    from learning3d_amd.models import _rows
    return _rows.square_distance(leaf(rnd(B, N, 3, seed=14)), leaf(rnd(B, M, 3, seed=15)))


@case("l3d_scatter_add_det")
def index_points(leaf):
    from learning3d_amd.models import _rows
    return _rows.index_points(leaf(rnd(B, N, 8, seed=16)), rint(N, B, 24, 6, seed=16))


def _conv(leaf, bn, pool, seed):
    from learning3d_amd.models import _train
    conv = leaf.params(seeded_params(nn.Conv2d(16, 32, 1), seed).cuda())
    norm = leaf.params(seeded_params(nn.BatchNorm2d(32), seed + 1).cuda().train()) if bn else None
    x = leaf(rnd(B, 16, 32, 4, seed=seed))
    return _train.conv_bn_act_max(x, conv, norm, relu=True) if pool else _train.conv_bn_act(x, conv, norm, relu=True)


@case("l3d_bn_act_backward")
def conv_act(leaf):
    return _conv(leaf, False, False, 17)


@case("l3d_bn_act_backward")
def conv_bn_act(leaf):
    return _conv(leaf, True, False, 19)


@case("l3d_bn_act_backward")
def conv_act_pool(leaf):
    return _conv(leaf, False, True, 21)


@case("l3d_bn_act_backward")
def conv_bn_act_pool(leaf):
    return _conv(leaf, True, True, 23)


@case("l3d_max_last_backward", view_inputs=False)          # max_over_last gates the Function on x.is_contiguous(): test_gpu_views_ops.py
def max_last(leaf):
    from learning3d_amd.models import _train
    return _train.max_over_last(leaf(rnd(B, 16, N, K, seed=25)))


@case("l3d_layernorm_ref_backward")
def layer_norm_ref(leaf):
    from learning3d_amd.models import _train
    return _train.layer_norm_ref(leaf(rnd(B, N, 64, seed=26)), leaf(rnd(64, seed=27)), leaf(rnd(64, seed=28)), 1e-6)


@case("l3d_chamfer_backward")
def chamfer_distance(leaf):
    from learning3d_amd.losses.chamfer_distance import ChamferDistanceFunction
    return ChamferDistanceFunction.apply(leaf(rnd(B, N, 3, seed=29)), leaf(rnd(B, M, 3, seed=30)))


@case("l3d_emd_backward")
def emd(leaf):
    from learning3d_amd.losses.emd import EMDFunction
    return EMDFunction.apply(leaf(rnd(B, N, 3, seed=31)), leaf(rnd(B, N, 3, seed=32)))


@case("l3d_bn_act_backward")
def recompute(leaf):
    """_fused._Recompute: PointNet in eval mode with autograd live -- the fused forward, and in the backward the per-layer route again"""
    from learning3d_amd.models import PointNet
    net = leaf.params(seeded_params(PointNet(emb_dims=64), 33).cuda().eval())
    return net(leaf(rnd(B, N, 3, seed=33)))


def backward(outs, inputs, grads):
    return torch.autograd.grad(list(outs), inputs, grad_outputs=list(grads), retain_graph=True, allow_unused=True)


def output_subsets(outs):
    """every output alone (the gradients of the others stay undefined), then all of them together"""
    n = len(outs)
    return [(i,) for i in range(n)] + ([tuple(range(n))] if n > 1 else [])


@pytest.mark.parametrize("name", sorted(CASES))
def test_backward_on_view_gradients(name):
    build, entry, _ = CASES[name]
    leaf = Leaves()
    outs = build(leaf)
    outs = tuple(outs) if isinstance(outs, (tuple, list)) else (outs,)
    if name == "recompute":
        assert type(outs[0].grad_fn).__name__ == "_RecomputeBackward"
    ran = 0
    for subset in output_subsets(outs):
        picked = [outs[i] for i in subset]
        per_output = [grad_views(o.shape, seed=50 + i) for i, o in zip(subset, picked)]
        for kind in ("transposed", "stride2", "expand"):
            gs = [dict(views).get(kind) for views in per_output]
            if any(g is None for g in gs):
                continue
            case = f"{name}: gradient of output {subset} as {kind} views {[g.stride() for g in gs]}"
            dense = [g.contiguous() for g in gs]
            want, log = logged(backward, picked, leaf.inputs, dense)
            again, log2 = logged(backward, picked, leaf.inputs, dense)
            assert log2 == log, case
            assert entry is None or has_entry(log, entry), f"{case}: {entry} not launched: {log}"
            assert any(w is not None for w in want), case
            assert_identical(again, want, case + ": two backward runs on the SAME contiguous gradient (determinism precondition)")
            before = [whole_storage(g).clone() for g in gs]
            got, vlog = logged(backward, picked, leaf.inputs, gs)
            assert vlog == log, f"{case}: launched {vlog}, with contiguous gradients {log}"
            assert_identical(got, want, case)
            assert all(torch.equal(whole_storage(g), b) for g, b in zip(gs, before)), f"{case}: the gradient's buffer was written to"
            ran += 1
    assert ran >= 2, f"{name}: only {ran} gradient layouts applied"


@pytest.mark.parametrize("name", sorted(n for n, c in CASES.items() if c[2]))
def test_forward_on_view_inputs_then_backward(name):
    build, entry, _ = CASES[name]
    ran = 0
    for kind in INPUT_KINDS:
        on_view, on_dense = Leaves(kind, dense=False), Leaves(kind, dense=True)
        probe = Leaves(kind, dense=False)
        with torch.no_grad():
            build(probe)
        if not probe.views:
            continue
        case = f"{name}: inputs as {kind} views {[v.stride() for v in probe.views]}"
        results = {}
        for side, leaf in (("dense", on_dense), ("dense again", Leaves(kind, dense=True)), ("view", on_view)):
            outs, flog = logged(build, leaf)
            outs = tuple(outs) if isinstance(outs, (tuple, list)) else (outs,)
            gs = [dict(grad_views(o.shape, seed=70 + i))["stride2"] for i, o in enumerate(outs)]
            before = [whole_storage(v).clone() for v in leaf.views]
            grads, blog = logged(backward, outs, leaf.inputs, gs)
            assert all(torch.equal(whole_storage(v), b) for v, b in zip(leaf.views, before)), f"{case}: an input's buffer was written to"
            results[side] = (outs, grads, flog, blog)
        want = results["dense"]
        assert entry is None or has_entry(want[3], entry), f"{case}: {entry} not launched: {want[3]}"
        assert results["dense again"][2:] == want[2:], case
        assert_identical(results["dense again"][:2], want[:2], case + ": two runs on the SAME contiguous inputs (determinism precondition)")
        got = results["view"]
        assert got[2] == want[2], f"{case}: forward launched {got[2]}, on contiguous clones {want[2]}"
        assert got[3] == want[3], f"{case}: backward launched {got[3]}, on contiguous clones {want[3]}"
        assert_identical(got[0], want[0], case + ", forward")
        assert_identical(got[1], want[1], case + ", backward", strides=False)
        ran += 1
    assert ran >= 2, f"{name}: only {ran} view kinds applied"


def test_every_function_of_the_package_is_accounted_for():
    """the Functions this file and test_gpu_views_ops.py name are the package's: a new one shows up here"""
    import inspect
    found = {f"{m.__name__.rsplit('.', 1)[-1]}.{n}" for m in layout_audit.package_modules() for n, c in vars(m).items()
             if inspect.isclass(c) and issubclass(c, torch.autograd.Function) and c.__module__ == m.__name__}
    assert found == {"model_common_utils._GraphFeature", "se3.ExpMap", "pointnet2_utils.FurthestPointSampling",
                     "pointnet2_utils.GatherOperation", "pointnet2_utils.KNN", "pointnet2_utils.ThreeNN", "pointnet2_utils.ThreeInterpolate",
                     "pointnet2_utils.GroupingOperation", "pointnet2_utils.BallQuery", "svd._KabschFunction", "_rows._MatMul",
                     "_rows._SoftmaxRows", "_rows._LinearRows", "_rows._SquareDistance", "_rows._IndexPoints", "_train._ConvAffineAct",
                     "_train._MaxLast", "_train._LayerNormRef", "chamfer_distance.ChamferDistanceFunction", "emd.EMDFunction",
                     "_fused._Recompute"}
